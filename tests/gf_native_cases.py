"""Cases, judge and bar of the native-size guided-filter tests (tests/test_gpu_gf_native.py, tests/test_gf_native_cases_cpu.py).
Plain numpy on the CPU: nothing here touches the device, and the device is never its own judge.  Window means, kinds and the
boundary-aware bar are gf_cases' (imported, not changed).

The pipeline (He and Sun, "Fast Guided Filter"): the colour guided filter is solved at the coefficient size (h, w) from a
low-resolution guide and the source, its mean planes (mean a_ck, mean b_c) are upsampled bilinearly to (H, W) >= (h, w) and
applied to the NATIVE guide: q_c = sum_k A_ck I_k + B_c.  ``pipeline`` restates all of it with a dtype switch: window means as
gf_cases.box_mean in float64 cast to the dtype (as the oracle's _box_mean does), the solve, both stages, the bilinear step and
the apply in the dtype.  q64 is its float64 run, q32 its float32 run.

Bilinear taps (half-pixel centres, edge replication: F.interpolate(mode="bilinear", align_corners=False)) come from INTEGERS
(``taps``): along an axis of n coefficient and N output samples, num = (2Y + 1) n - N, i0 = floor(num / 2N),
f = (num - 2N i0) / 2N, taps clamp(i0, 0, n - 1) and clamp(i0 + 1, 0, n - 1); horizontally first, then vertically, each as
(1 - f) v0 + f v1.

Bar: gf_cases.judge(q64, device_u8, tau) with tau = 2 max|q32 - q64| + 1e-3 -- the generic path's "twice the fp32 floor plus
1e-3" with the floor taken over ALL values, from the reference alone; everywhere |device - rint(q64)| <= 1.

``pipeline(defect=...)`` seeds what a tiled upsampling kernel gets wrong, so that the CPU test can show that the cases SEE it:
  "nohalf"  tap positions without the half-pixel offset (Y n / N in place of (Y + 0.5) n / N - 0.5);
  "lastcol" a 64-column output tile whose staged footprint lacks its last column: the taps that read it get the column before;
  "zeros"   zeros in place of edge replication outside the plane.
"""
import functools

import numpy as np

import gf_cases as G

EPS = G.EPS
TILE_W = 64                   # output columns of a block of gf_apply_up_kernel (and of the "lastcol" defect)
TILE_H = 16


def taps(n, N, half=True):
    """-> (i0 (N,) int64, rem (N,) int64, den): output sample Y reads clamp(i0), clamp(i0 + 1) with fraction rem / den"""
    Y = np.arange(N, dtype=np.int64)
    num = (2 * Y + 1) * n - N if half else 2 * Y * n
    den = 2 * N
    i0 = num // den                                   # numpy's // floors
    return i0, num - i0 * den, den


def _interp(P, n, N, axis, dtype, defect):
    """bilinear along ``axis`` (-1 or -2) of P (..., h, w), n -> N samples"""
    i0, rem, den = taps(n, N, half=defect != "nohalf")
    f = (rem.astype(dtype) / dtype(den)).astype(dtype)
    i1 = i0 + 1
    if defect == "lastcol" and axis == -1:
        X = np.arange(N)
        last = i0[np.minimum(X // TILE_W * TILE_W + TILE_W - 1, N - 1)] + 1      # last footprint column of X's tile
        i1 = np.where(i1 == last, i0, i1)
    c0, c1 = np.clip(i0, 0, n - 1), np.clip(i1, 0, n - 1)
    v0, v1 = np.take(P, c0, axis=axis), np.take(P, c1, axis=axis)
    if defect == "zeros":
        shape = (-1,) if axis == -1 else (-1, 1)
        v0 = v0 * ((i0 >= 0) & (i0 <= n - 1)).reshape(shape)
        v1 = v1 * ((i1 >= 0) & (i1 <= n - 1)).reshape(shape)
    f = f.reshape((-1,) if axis == -1 else (-1, 1))
    return ((dtype(1) - f) * v0 + f * v1).astype(dtype)


def mean_planes(guide_lo, src, r, eps=EPS, dtype=np.float64):
    """(h,w,3) uint8 x 2 -> (12,h,w) of ``dtype``: plane 4c + k, k = 0..2 mean a_ck, k = 3 mean b_c (the order gf_solve_kernel
    writes); the arithmetic of oracle.guided_filter_color up to the second box mean"""
    I = np.moveaxis(guide_lo.astype(dtype), -1, 0)
    P = np.moveaxis(src.astype(dtype), -1, 0)
    bm = lambda a: G.box_mean(a, r).astype(dtype)
    mI = [bm(I[i]) for i in range(3)]
    cov = {}
    for i in range(3):
        for j in range(i, 3):
            cov[(i, j)] = bm(I[i] * I[j]) - mI[i] * mI[j]
            if i == j:
                cov[(i, j)] = cov[(i, j)] + dtype(eps)
    a00, a01, a02 = cov[(0, 0)], cov[(0, 1)], cov[(0, 2)]
    a11, a12, a22 = cov[(1, 1)], cov[(1, 2)], cov[(2, 2)]
    c00 = a11 * a22 - a12 * a12
    c01 = a02 * a12 - a01 * a22
    c02 = a01 * a12 - a02 * a11
    c11 = a00 * a22 - a02 * a02
    c12 = a02 * a01 - a00 * a12
    c22 = a00 * a11 - a01 * a01
    det = a00 * c00 + a01 * c01 + a02 * c02
    inv = [[c00 / det, c01 / det, c02 / det], [c01 / det, c11 / det, c12 / det], [c02 / det, c12 / det, c22 / det]]
    out = np.empty((12,) + guide_lo.shape[:2], dtype)
    for ch in range(3):
        mp = bm(P[ch])
        cp = [bm(I[i] * P[ch]) - mI[i] * mp for i in range(3)]
        a = [inv[k][0] * cp[0] + inv[k][1] * cp[1] + inv[k][2] * cp[2] for k in range(3)]
        b = mp - a[0] * mI[0] - a[1] * mI[1] - a[2] * mI[2]
        for k in range(3):
            out[4 * ch + k] = bm(a[k])
        out[4 * ch + 3] = bm(b)
    return out


def apply_planes(planes, guide_native, dtype=np.float64, defect=None):
    """(12,h,w) planes, (H,W,3) uint8 -> unrounded q (H,W,3) of ``dtype``: bilinear upsample (horizontally, then vertically), apply"""
    h, w = planes.shape[-2:]
    H, W = guide_native.shape[:2]
    up = _interp(_interp(planes.astype(dtype), w, W, -1, dtype, defect), h, H, -2, dtype, defect)
    I = np.moveaxis(guide_native.astype(dtype), -1, 0)
    q = np.empty((H, W, 3), dtype)
    for c in range(3):
        q[..., c] = up[4 * c] * I[0] + up[4 * c + 1] * I[1] + up[4 * c + 2] * I[2] + up[4 * c + 3]
    return q


def pipeline(guide_lo, src, guide_native, r, eps=EPS, dtype=np.float64, defect=None):
    return apply_planes(mean_planes(guide_lo, src, r, eps, dtype), guide_native, dtype, defect)


# ------------------------------------------------------------------------------------------------------------------ inputs
def native_inputs(kind, h, w, H, W):
    """-> (native guide (H,W,3), low-resolution guide (h,w,3), source (h,w,3)), uint8.  The native guide is the kind's guide at
    (h, w) with every pixel grown to a block of the ratio (a lattice whose blocks scale with it) plus +-2 LSB of per-pixel
    noise -- detail the low resolution does not have; the low-resolution guide is Pillow's bicubic resize of the native one (what
    imageio.preprocess makes); the source is the kind's at (h, w)."""
    from PIL import Image
    g, s = G.KINDS[kind](h, w)
    rng = np.random.default_rng([h, w, H, W, 4])
    yy = np.arange(H) * h // H
    xx = np.arange(W) * w // W
    native = np.clip(g[yy][:, xx].astype(np.int64) + rng.integers(-2, 3, (H, W, 3)), 0, 255).astype(np.uint8)
    lo = native if (H, W) == (h, w) else np.array(Image.fromarray(native).resize((w, h), Image.BICUBIC))
    return native, np.ascontiguousarray(lo), np.ascontiguousarray(s)


class Ref:
    """everything the bar needs for one case, from the reference alone"""

    def __init__(self, kind, h, w, H, W, r, eps=EPS):
        self.native, self.lo, self.src = native_inputs(kind, h, w, H, W)
        self.r, self.eps = r, eps
        self.planes64 = mean_planes(self.lo, self.src, r, eps, np.float64)
        self.planes32 = mean_planes(self.lo, self.src, r, eps, np.float32)
        self.q64 = apply_planes(self.planes64, self.native, np.float64)
        self.q32 = apply_planes(self.planes32, self.native, np.float32)
        self.floor32 = float(np.abs(self.q32.astype(np.float64) - self.q64).max())
        self.tau = 2 * self.floor32 + 1e-3
        self.expect = G.round_u8(self.q64)
        d, _ = G.boundary_distance(self.q64)
        self.exempt = float((d <= self.tau).mean())
        self.saturating = float(((self.q64 < 0) | (self.q64 > 255)).mean())

    def defect(self, name):
        return G.round_u8(apply_planes(self.planes64, self.native, np.float64, name))


# (kind, h, w, H, W, r): coefficient grid -> native size.
CASES = [
    ("blocks", 70, 90, 140, 180, 7),          # exact 2x
    ("blocks", 70, 90, 211, 333, 16),         # non-integer, anisotropic
    ("flat", 70, 90, 140, 180, 7),
    ("blocks", 97, 193, 388, 772, 30),        # 4x, several tiles both ways
    ("flat", 97, 193, 300, 500, 30),
    ("blocks", 65, 65, 129, 131, 31),         # 2x plus one / plus three
    ("blocks", 64, 64, 512, 512, 7),          # 8x
    ("blocks", 33, 40, 1000, 77, 2),          # 30x by < 2x, W barely above a tile
    ("flat", 33, 40, 35, 650, 16),            # nearly 1x by 16x
    ("saturating", 70, 90, 280, 270, 7),      # a large share of q64 outside 0..255
    ("blocks", 70, 90, 70, 90, 7),            # scale 1: no tap defect shows; kept for the clamp path and the largest footprint
]
# the extents the kernel's 64 x 16 tiles make special (gf_apply_up_kernel): one row / column either side of a tile edge at scale
# 2, and the largest footprint (17 x 65 coefficient samples: scale 1, above; and barely above 1, where it starts at tap -1)
TILE_CASES = [
    ("blocks", 33, 40, 63, 127, 7),           # one short of 4 x 2 tiles
    ("blocks", 33, 40, 64, 128, 7),           # exactly 4 x 2 tiles
    ("blocks", 33, 40, 65, 129, 7),           # one past: a tile of one row, a tile of one column
    ("flat", 70, 90, 71, 91, 7),              # scale 1.01: footprint of 17 x 65 from tap -1, two tiles wide, five high
]
ALL_CASES = CASES + TILE_CASES
# the cases on which every seeded defect has to violate the bar: every scale above 1 (at scale 1 every fraction is 0 and no tap
# leaves the plane: no tap defect can show)
DEFECTS = ("nohalf", "lastcol", "zeros")
SENSITIVE = [c for c in ALL_CASES if c[3] > c[1] and c[4] > c[2]]

# coefficient planes alone: (kind, h, w, r)
PLANE_CASES = [("blocks", 70, 90, 7), ("blocks", 70, 90, 16), ("blocks", 70, 90, 30), ("blocks", 200, 193, 60)]


def case_id(c):
    return "%s-%dx%d-to-%dx%d-r%d" % c


@functools.lru_cache(maxsize=None)
def ref(*case):
    return Ref(*case)


@functools.lru_cache(maxsize=None)
def plane_ref(kind, h, w, r):
    """-> (guide, src, planes64, bar): bar = 2 max|planes32 - planes64| + 1e-6 max|planes64|"""
    g, s = G.inputs(kind, h, w)
    p64 = mean_planes(g, s, r, EPS, np.float64)
    p32 = mean_planes(g, s, r, EPS, np.float32)
    return g, s, p64, 2 * float(np.abs(p32.astype(np.float64) - p64).max()) + 1e-6 * float(np.abs(p64).max())
