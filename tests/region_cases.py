"""Cases, judges and bars of the region-swap tests (tests/test_gpu_region.py, tests/test_region_cases_cpu.py): an aligned crop of
a photograph under a similarity transform (ppst_extract_similarity) and the guided filter's coefficients pasted back through
the same transform (ppst_guided_filter_paste).  Plain numpy on the CPU: nothing here touches the device, and the device is never
its own judge.  The boundary-aware bar is gf_cases.judge, the coefficient planes are gf_native_cases.mean_planes (both imported,
not changed).

The transform is four integers (a, b, cu, cv) (``crop_xf`` restates ppst_amd.imageio.crop_transform; the CPU test holds the two
together): photo pixel (X, Y) lies at U = a (2X + 1) + b (2Y + 1) + cu, V = -b (2X + 1) + a (2Y + 1) + cv in units of 2^-24 crop
pixel.  Everything that DECIDES something -- which photo pixels enter a crop pixel's sum, which lie inside the crop square, which
coefficient samples a pixel taps -- is computed on these int64 values; only weights and fractions are floats, in the dtype of
the run.

``extract``: out[j, i] = sum w p / sum w over every integer (X, Y) with |U - Uc| < 2^25 and |V - Vc| < 2^25,
w = k((U - Uc) / 2^24) k((V - Vc) / 2^24), (Uc, Vc) = ((2i + 1) 2^23, (2j + 1) 2^23), k the bicubic (a = -0.5), the photo read
with edge replication.  ``paste``: inside 0 <= U, V < n 2^24 the 12 planes by bilinear interpolation at (U - 2^23, V - 2^23) / 2^24
(floor by shift, fraction = low 24 bits, taps clamped, horizontally then vertically), q = A I + B on the photo's pixel,
g q + (1 - g) I with g the smoothstep of (distance to the square's edge) / feather; outside, the photo's byte.

Bar: gf_cases.judge(ref64, device_u8, tau), tau = 2 max|ref32 - ref64| + 1e-3 from the restatement alone (``ExtractRef``,
``PasteRef``); bytes outside the crop square must be EQUAL to the photo's.

Seeded defects (``defect=``), so that the CPU test can show that the cases see them through the bar:
  "nohalf"   pixel centres without the 1/2: U = a 2X + b 2Y + cu;
  "mirror"   the sign of b flipped in V;
  "zeros"    zeros in place of edge replication (photo pixels in extract, coefficient taps in paste);
  "nonorm"   extract: the weights divided by the nominal s^2 instead of their sum;
  "hardedge" paste: the feather ignored;
  "tilefoot" paste: a PASTE_T x PASTE_T photo tile's staged coefficient footprint one column short: the taps that read its last
             column get the column before (gf_native_cases' "lastcol" for a rotated tile).
"""
import functools
import math

import numpy as np

import gf_cases as G
import gf_native_cases as N

ONE, HALF = 1 << 24, 1 << 23
# the kernels' tiles: gf_paste_kernel's photo tile (GP_T in csrc/guided_filter.hip) and extract_similarity_kernel's crop tiles
# (16 x 16 crop pixels up to s = 4, 8 x 8 above: csrc/imageio.hip).  tests/test_region_cases_cpu.py reads them from the sources.
PASTE_T = 16
EXTRACT_T = ((4.0, 16), (8.0, 8))
R = 7                          # radius of the coefficient planes


def crop_xf(centre, side, angle_deg, n):
    """ppst_amd.imageio.crop_transform, restated"""
    s = float(side) / n
    q = round(float(angle_deg) / 90.0)
    if float(angle_deg) == 90.0 * q:
        co, si = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))[q % 4]
    else:
        co, si = math.cos(math.radians(angle_deg)), math.sin(math.radians(angle_deg))
    a, b = round(HALF * co / s), round(HALF * si / s)
    x, y = float(centre[0]), float(centre[1])
    return a, b, round(n * HALF - 2.0 * (a * x + b * y)), round(n * HALF - 2.0 * (-b * x + a * y))


def uv(xf, X, Y, defect=None):
    """int64 (U, V) of the photo pixels (X, Y) (int64 arrays)"""
    a, b, cu, cv = (int(v) for v in xf)
    h = 0 if defect == "nohalf" else 1
    px, py = 2 * X + h, 2 * Y + h
    bv = -b if defect == "mirror" else b
    return a * px + b * py + cu, -bv * px + a * py + cv


def _k(x, dtype):
    x = np.abs(x).astype(dtype)
    a = dtype(-0.5)
    near = ((a + dtype(2)) * x - (a + dtype(3))) * x * x + dtype(1)
    far = (((x - dtype(5)) * x + dtype(8)) * x - dtype(4)) * a
    return np.where(x < 1, near, np.where(x < 2, far, dtype(0))).astype(dtype)


def extract(photo, xf, n, dtype=np.float64, defect=None):
    """(H,W,3) uint8 -> unrounded crop (n,n,3) of ``dtype``"""
    H, W = photo.shape[:2]
    a, b, cu, cv = (int(v) for v in xf)
    D = float(a * a + b * b)
    ii, jj = np.meshgrid(np.arange(n, dtype=np.int64), np.arange(n, dtype=np.int64))       # ii: column, jj: row
    Uc, Vc = ((2 * ii + 1) * HALF).reshape(-1, 1), ((2 * jj + 1) * HALF).reshape(-1, 1)
    # a window of photo pixels that holds every tap: the centre mapped back in float64, +- the support's box + 2
    dU, dV = (Uc - cu).astype(np.float64), (Vc - cv).astype(np.float64)
    xc = np.floor(((a * dU - b * dV) / D - 1) / 2).astype(np.int64)
    yc = np.floor(((b * dU + a * dV) / D - 1) / 2).astype(np.int64)
    K = int(math.ceil((abs(a) + abs(b)) * float(1 << 25) / D / 2)) + 2
    oy, ox = np.meshgrid(np.arange(-K, K + 1, dtype=np.int64), np.arange(-K, K + 1, dtype=np.int64), indexing="ij")
    X, Y = xc + ox.reshape(1, -1), yc + oy.reshape(1, -1)
    U, V = uv(xf, X, Y, defect)
    du, dv = U - Uc, V - Vc
    taps = (np.abs(du) < (1 << 25)) & (np.abs(dv) < (1 << 25))
    w = _k(du.astype(dtype) / dtype(ONE), dtype) * _k(dv.astype(dtype) / dtype(ONE), dtype)
    w = np.where(taps, w, dtype(0)).astype(dtype)
    p = photo[np.clip(Y, 0, H - 1), np.clip(X, 0, W - 1)].astype(dtype)                     # (n n, taps, 3)
    if defect == "zeros":
        p = p * ((X >= 0) & (X < W) & (Y >= 0) & (Y < H))[..., None]
    num = (w[..., None] * p).sum(axis=1, dtype=dtype)
    den = np.full((n * n,), dtype((1 << 46) / D)) if defect == "nonorm" else w.sum(axis=1, dtype=dtype)
    with np.errstate(invalid="ignore", divide="ignore"):                                    # (a seeded defect may leave a pixel without taps)
        out = num / den[:, None]
    return np.nan_to_num(out).astype(dtype).reshape(n, n, 3)


def inside(xf, n, H, W, defect=None):
    """-> (mask (H,W) of the photo pixels inside the crop square, U, V)"""
    X, Y = np.meshgrid(np.arange(W, dtype=np.int64), np.arange(H, dtype=np.int64))
    U, V = uv(xf, X, Y, defect)
    return (U >= 0) & (U < n * ONE) & (V >= 0) & (V < n * ONE), U, V


def _tile_last(xf, n, H, W, defect):
    """per photo pixel: the last coefficient column its PASTE_T x PASTE_T tile stages (the tile's largest tap, clamped)"""
    X, Y = np.meshgrid(np.arange(W, dtype=np.int64), np.arange(H, dtype=np.int64))
    X0, Y0 = X // PASTE_T * PASTE_T, Y // PASTE_T * PASTE_T
    XL, YL = np.minimum(X0 + PASTE_T - 1, W - 1), np.minimum(Y0 + PASTE_T - 1, H - 1)
    us = [uv(xf, x, y, defect)[0] - HALF for x in (X0, XL) for y in (Y0, YL)]
    hi = np.clip((np.maximum.reduce(us) >> 24) + 1, 0, n - 1)
    lo = np.clip(np.minimum.reduce(us) >> 24, 0, n - 1)
    return hi, lo


def paste(planes, photo, xf, feather, dtype=np.float64, defect=None):
    """(12,n,n) planes, (H,W,3) uint8 -> unrounded output (H,W,3) of ``dtype`` (outside the square: the photo's bytes, exactly)"""
    n = planes.shape[-1]
    H, W = photo.shape[:2]
    m, U, V = inside(xf, n, H, W, defect)
    out = photo.astype(dtype)
    if not m.any():
        return out
    P = planes.astype(dtype)
    Ui, Vi = U[m] - HALF, V[m] - HALF
    i0, j0 = Ui >> 24, Vi >> 24
    fx = ((Ui & (ONE - 1)).astype(dtype) / dtype(ONE)).astype(dtype)
    fy = ((Vi & (ONE - 1)).astype(dtype) / dtype(ONE)).astype(dtype)
    c0, c1, r0, r1 = np.clip(i0, 0, n - 1), np.clip(i0 + 1, 0, n - 1), np.clip(j0, 0, n - 1), np.clip(j0 + 1, 0, n - 1)
    if defect == "tilefoot":
        hi, lo = _tile_last(xf, n, H, W, defect)
        hi, lo = hi[m], lo[m]
        c0 = np.where((c0 == hi) & (hi > lo), c0 - 1, c0)
        c1 = np.where((c1 == hi) & (hi > lo), c1 - 1, c1)
    z = lambda v, ok: v * ok if defect == "zeros" else v
    okc0, okc1, okr0, okr1 = (i0 >= 0), (i0 + 1 <= n - 1), (j0 >= 0), (j0 + 1 <= n - 1)
    one = dtype(1)
    top = ((one - fx) * z(P[:, r0, c0], okc0 & okr0) + fx * z(P[:, r0, c1], okc1 & okr0)).astype(dtype)
    bot = ((one - fx) * z(P[:, r1, c0], okc0 & okr1) + fx * z(P[:, r1, c1], okc1 & okr1)).astype(dtype)
    co = ((one - fy) * top + fy * bot).astype(dtype)                                        # (12, pixels)
    I = photo[m].astype(dtype)                                                              # (pixels, 3)
    if feather > 0 and defect != "hardedge":
        d = np.minimum(np.minimum(U[m], n * ONE - U[m]), np.minimum(V[m], n * ONE - V[m]))
        t = np.clip(d.astype(dtype) / dtype(ONE) / dtype(feather), 0, 1).astype(dtype)
        g = (t * t * (dtype(3) - dtype(2) * t)).astype(dtype)
    else:
        g = np.ones(I.shape[0], dtype)
    res = np.empty_like(I)
    for c in range(3):
        q = co[4 * c] * I[:, 0] + co[4 * c + 1] * I[:, 1] + co[4 * c + 2] * I[:, 2] + co[4 * c + 3]
        res[:, c] = g * q + (one - g) * I[:, c]
    out[m] = res
    return out


# ------------------------------------------------------------------------------------------------------------------ cases
# (name, H, W, n, cx, cy, s, angle_deg, feather): photo H x W, crop n x n of side s n centred at (cx, cy)
CASES = [
    ("copy-s1-0deg", 90, 70, 24, 35.0, 45.0, 1.0, 0.0, 0),                    # integer offset: extract is a byte copy
    ("inside-s1.5-30deg", 150, 200, 40, 100.0, 75.0, 1.5, 30.0, 1),
    ("inside-s2-m45deg", 150, 200, 40, 98.3, 70.6, 2.0, -45.0, 20),
    ("inside-s2-90deg", 110, 130, 24, 60.5, 50.5, 2.0, 90.0, 12),
    ("inside-s4-30deg", 70, 90, 8, 45.0, 35.0, 4.0, 30.0, 4),
    ("over-s7.999-m45deg", 90, 120, 8, 60.0, 45.0, 7.999, -45.0, 0),          # the 8 x 8 crop tile's largest box (s = 8 turned may round past the rule)
    ("inside-s8-0deg", 90, 120, 8, 60.25, 44.5, 8.0, 0.0, 1),
    ("over-left-s1.5-30deg", 90, 70, 24, 5.0, 45.0, 1.5, 30.0, 1),
    ("over-right-s1.5-30deg", 90, 70, 24, 66.0, 40.0, 1.5, 30.0, 12),
    ("over-top-s1.5-m45deg", 90, 70, 24, 33.0, 4.0, 1.5, -45.0, 0),
    ("over-bottom-s1.5-90deg", 90, 70, 24, 36.5, 87.0, 1.5, 90.0, 1),
    ("whole-s5-0deg", 70, 90, 24, 45.0, 35.0, 5.0, 0.0, 12),                   # the square covers the photo; 3 x 3 crop tiles of 8
    ("whole-s6-30deg", 70, 90, 24, 45.0, 35.0, 6.0, 30.0, 0),
    ("foot-s1.001-m45deg", 100, 100, 40, 50.0, 50.0, 1.001, -45.0, 20),        # the paste tile's largest footprint: s barely above 1 at 45 degrees
    ("foot-s1.001-30deg", 100, 100, 40, 50.3, 49.6, 1.001, 30.0, 1),
]
# photo extents and quad positions one pixel either side of the paste kernel's tile edges (PASTE_T = 16): photo widths 63 / 64 / 65
# and heights 81 / 80 / 79, the square's corner at (15, 16), (16, 17), (17, 15), its far side 1 or 2 pixels from the photo's
TILE_CASES = [
    ("tile-short", 79, 65, 40, 35.0, 36.0, 1.0, 0.0, 0),
    ("tile-exact", 80, 64, 40, 36.0, 37.0, 1.0, 0.0, 1),
    ("tile-past", 81, 63, 40, 37.0, 35.0, 1.0, 0.0, 20),
    ("tile-past-s2-30deg", 81, 65, 24, 32.5, 40.5, 2.0, 30.0, 1),
]
ALL_CASES = CASES + TILE_CASES
EXTRACT_DEFECTS = ("nohalf", "mirror", "zeros", "nonorm")
PASTE_DEFECTS = ("nohalf", "mirror", "zeros", "hardedge", "tilefoot")
# three different transforms, one photo size: a batch
BATCH = ["inside-s2-90deg", ("b1", 110, 130, 24, 20.0, 100.0, 1.5, 30.0, 1), ("b2", 110, 130, 24, 70.0, 40.0, 3.0, -45.0, 12)]


def case_id(c):
    return c[0]


def case_xf(c):
    _, H, W, n, cx, cy, s, ang, _ = c
    return crop_xf((cx, cy), s * n, ang, n)


@functools.lru_cache(maxsize=None)
def photo_of(H, W):
    p = G.blocks(H, W, seed=3)[0]
    p.setflags(write=False)
    return p


class _Bar:
    def _bar(self, ref64, ref32, over):
        self.floor32 = float(np.abs(ref32.astype(np.float64) - ref64).max())
        self.tau = 2 * self.floor32 + 1e-3
        self.expect = G.round_u8(ref64)
        d, _ = G.boundary_distance(ref64[over])
        self.exempt = float((d <= self.tau).mean()) if d.size else 0.0


class ExtractRef(_Bar):
    """the crop of one case in float64 and float32, and the bar from the two"""

    def __init__(self, case):
        _, H, W, n, *_ = case
        self.case, self.n, self.photo, self.xf = case, n, photo_of(H, W), case_xf(case)
        self.ref64 = extract(self.photo, self.xf, n, np.float64)
        self.ref32 = extract(self.photo, self.xf, n, np.float32)
        self._bar(self.ref64, self.ref32, np.ones((n, n), bool))

    def defect(self, name):
        return G.round_u8(extract(self.photo, self.xf, self.n, np.float64, name))


class PasteRef(_Bar):
    """the paste of one case: the coefficient planes are gf_native_cases.mean_planes (float64, radius R) of the case's own crop --
    the float64 crop, rounded -- as guide and a hard-edged lattice as source, ROUNDED TO float32: those fp32 planes are the
    input of both runs of the restatement and of the device"""

    def __init__(self, case):
        _, H, W, n, _, _, _, _, feather = case
        E = extract_ref(case)
        self.case, self.n, self.photo, self.xf, self.feather = case, n, E.photo, E.xf, feather
        src = G.blocks(n, n, seed=5)[1]
        self.planes = N.mean_planes(np.ascontiguousarray(E.expect), src, R, N.EPS, np.float64).astype(np.float32)
        self.ref64 = paste(self.planes, self.photo, self.xf, feather, np.float64)
        self.ref32 = paste(self.planes, self.photo, self.xf, feather, np.float32)
        self.inside = inside(self.xf, n, H, W)[0]
        self._bar(self.ref64, self.ref32, self.inside)

    def defect(self, name):
        return G.round_u8(paste(self.planes, self.photo, self.xf, self.feather, np.float64, name))


def lookup(c):
    return c if not isinstance(c, str) else next(k for k in ALL_CASES if k[0] == c)


@functools.lru_cache(maxsize=None)
def extract_ref(case):
    return ExtractRef(lookup(case))


@functools.lru_cache(maxsize=None)
def paste_ref(case):
    return PasteRef(lookup(case))


def judge_paste(Rf, got_u8):
    """gf_cases.judge on the whole photo + byte equality outside the square -> list of violated clauses"""
    bad = G.judge(Rf.ref64, got_u8, Rf.tau)
    out = ~Rf.inside
    if not np.array_equal(got_u8[out], Rf.photo[out]):
        bad.append("%d bytes outside the crop square differ from the photo" % int((got_u8[out] != Rf.photo[out]).sum()))
    return bad
