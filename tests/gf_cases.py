"""Inputs, judge and bar of the guided-filter tests (tests/test_gpu_guided_filter.py, tests/test_guided_filter_cases_cpu.py).
Plain numpy on the CPU: nothing here touches the device, and the device is never its own judge.

The judge is ``restate``: the published colour guided filter (He et al., as oracle/ppst_oracle.py:guided_filter_color states
it) in float64, returning the UNROUNDED output q64 and the (a, b) planes.  It has three switches that seed the defects a strip /
halo / border kernel makes -- the stage-2 box window one row late, BORDER_REFLECT_101 in place of BORDER_REFLECT, and the last
segment of a 192-column strip reading its entering column one short -- so that the CPU test can show that the inputs SEE such a
defect through the bar before the device is trusted by them.

The bar (``judge``) is boundary-aware.  With e = clip(rint(q64), 0, 255) and d = the distance of q64 from the nearest rounding
boundary k + 0.5 (k = 0 .. 254: the clip leaves no boundary below 0.5 or above 254.5):
  * a uint8 result must equal e wherever d > tau;
  * within tau of a boundary it may be e or the value across that boundary;
  * everywhere |result - e| <= 1 (the project's bar, never relaxed).
tau comes from the reference alone (``Ref``): tau = tau_ref + 2 tau_half for the radius-30 path, 2 tau_ref + 1e-3 for the
generic path (fp32 planes), where
  * tau_ref is the largest d at which the float32 oracle disagrees with e on that input (the floor of an fp32 solve);
  * tau_half = (2 * 2^-11 / (2r + 1)) * (255 sum_k max|a_k| + max|b|) bounds what IEEE-half storage of (a, b) with error
    diffusion can do to q: a vertical window sum of the stored halves differs from the exact sum by the end residuals, each
    <= 2^-11 |v|; the horizontal mean over 2r + 1 such column sums keeps that bound; the maxima are the float64 planes', per
    output channel, and the largest channel's figure is the case's.  tau_half counts TWO residuals (one run of rows).  The
    first launch restarts the diffusion every 32 (or 64) rows, so a 61-row window spans up to three runs and carries up to
    FOUR residuals (the one before its first row, and the last of each run): exactly the 2 tau_half of the bar; the fp32
    sliding sums of stage 2 (<= 63 roundings of a 61-term sum) are orders of magnitude below that.
"""
import functools

import numpy as np

EPS = (0.02 * 255) ** 2
EXEMPT_CAP = 0.15


# ------------------------------------------------------------------------------------------------------------------ judge
STRIP, SEG = 192, 16          # the fused launches' geometry: columns per strip, outputs per sliding segment


def box_mean(a, r, border="symmetric", dy=0, seam=False):
    """(..., H, W) float64 -> mean over the (2r+1)^2 window centred dy rows below the pixel; border 'symmetric' repeats the
    edge pixel (cv2.BORDER_REFLECT), 'reflect' does not (cv2.BORDER_REFLECT_101).  Integral image in float64, the
    arithmetic of the oracle's _box_mean.  ``seam``: the last SEG-output segment of every STRIP-column strip slides its
    horizontal window with the entering column read one short (its outputs 1 .. SEG - 1 keep the segment's first entering
    column in place of their own)."""
    lead = [(0, 0)] * (a.ndim - 2)
    ap = np.pad(a, lead + [(r - min(dy, 0), r + max(dy, 0)), (r, r)], mode=border).astype(np.float64)
    c = np.cumsum(np.cumsum(ap, axis=-2), axis=-1)
    c = np.pad(c, lead + [(1, 0), (1, 0)])
    n = 2 * r + 1
    H, W = a.shape[-2:]
    o = max(dy, 0)                                   # row of ap at which the window of image row 0 starts
    s = c[..., o + n:o + n + H, n:n + W] - c[..., o:o + H, n:n + W] - c[..., o + n:o + n + H, 0:W] + c[..., o:o + H, 0:W]
    if seam:
        c1 = np.pad(np.cumsum(ap, axis=-2), lead + [(1, 0), (0, 0)])
        V = c1[..., o + n:o + n + H, :] - c1[..., o:o + H, :]          # vertical window sums of the padded columns
        for x in range(W):
            j = x % STRIP - (STRIP - SEG)
            if j >= 1:
                s[..., x] += V[..., x - j + 2 * r] - V[..., x + 2 * r]
    return s / (n * n)


def restate(guide_u8, src_u8, r=30, eps=EPS, border="symmetric", shift2=0, seam=0):
    """(H,W,3) uint8 x 2 -> (q64 (H,W,3), a (3,3,H,W) [channel][k], b (3,H,W)), all float64.  ``border`` / ``shift2`` / ``seam``
    seed the defects (every box of both stages with the other border; the stage-2 windows shift2 rows late; the strip-seam
    defect of box_mean in the boxes of stage ``seam`` = 1 or 2)."""
    I = np.moveaxis(guide_u8.astype(np.float64), -1, 0)
    P = np.moveaxis(src_u8.astype(np.float64), -1, 0)
    bm = functools.partial(box_mean, r=r, border=border, seam=seam == 1)
    mI = bm(I)
    cov = {}
    for i in range(3):
        for j in range(i, 3):
            cov[(i, j)] = bm(I[i] * I[j]) - mI[i] * mI[j]
            if i == j:
                cov[(i, j)] = cov[(i, j)] + np.float64(eps)
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
    H, W = guide_u8.shape[:2]
    q = np.empty((H, W, 3), np.float64)
    A = np.empty((3, 3, H, W), np.float64)
    Bp = np.empty((3, H, W), np.float64)
    for ch in range(3):
        p = P[ch]
        mp = bm(p)
        cp = [bm(I[i] * p) - mI[i] * mp for i in range(3)]
        a = [inv[k][0] * cp[0] + inv[k][1] * cp[1] + inv[k][2] * cp[2] for k in range(3)]
        b = mp - a[0] * mI[0] - a[1] * mI[1] - a[2] * mI[2]
        ma = [box_mean(a[k], r, border, shift2, seam == 2) for k in range(3)]
        mb = box_mean(b, r, border, shift2, seam == 2)
        q[..., ch] = ma[0] * I[0] + ma[1] * I[1] + ma[2] * I[2] + mb
        A[ch] = a
        Bp[ch] = b
    return q, A, Bp


def round_u8(q):
    return np.clip(np.rint(q), 0, 255).astype(np.uint8)


def boundary_distance(q64):
    """distance of q64 from the nearest rounding boundary that survives the clip (k + 0.5, k = 0 .. 254)"""
    k = np.clip(np.floor(q64), 0, 254)
    return np.abs(q64 - (k + 0.5)), k


def min_tau(q64, got_u8):
    """the smallest tau at which ``got_u8`` passes the exact-outside-tau clause: the largest boundary distance among the
    values that differ from clip(rint(q64)) (0 if none differs)"""
    d, _ = boundary_distance(q64)
    bad = got_u8 != round_u8(q64)
    return float(d[bad].max()) if bad.any() else 0.0


def judge(q64, got_u8, tau):
    """-> list of violated clauses (empty = passes the bar of the module docstring)"""
    e = round_u8(q64).astype(np.int64)
    g = got_u8.astype(np.int64)
    d, k = boundary_distance(q64)
    other = (2 * k + 1 - e).astype(np.int64)                 # the value across the nearest boundary
    out = []
    if np.abs(g - e).max() > 1:
        out.append("max |diff| %d LSB > 1" % np.abs(g - e).max())
    far = (g != e) & (d > tau)
    if far.any():
        out.append("%d values differ farther than tau = %.3g from a boundary (largest distance %.4f)" % (far.sum(), tau, d[far].max()))
    near = (g != e) & (d <= tau) & (g != other)
    if near.any():
        out.append("%d values near a boundary are neither of its two neighbours" % near.sum())
    return out


def tau_half(A, Bp, r):
    per_ch = [255.0 * sum(np.abs(A[c, k]).max() for k in range(3)) + np.abs(Bp[c]).max() for c in range(3)]
    return 2.0 * 2.0 ** -11 / (2 * r + 1) * max(per_ch)


class Ref:
    """everything the bar needs for one (guide, src, r, eps): q64, tau_ref, tau_half, tau, the exempt share"""

    def __init__(self, guide, src, r=30, eps=EPS):
        import ppst_oracle as O
        self.r, self.eps = r, eps
        self.q64, A, Bp = restate(guide, src, r, eps)
        self.expect = round_u8(self.q64)
        self.oracle32 = O.guided_filter_color(guide, src, r, eps, dtype=np.float32)
        self.tau_ref = min_tau(self.q64, self.oracle32)
        self.tau_half = tau_half(A, Bp, r)
        # (the radius-30 path stores (a, b) as halves; every other radius keeps fp32 planes: tau_half is printed, not used)
        self.tau = self.tau_ref + 2 * self.tau_half if r == 30 else 2 * self.tau_ref + 1e-3
        d, _ = boundary_distance(self.q64)
        self.exempt = float((d <= self.tau).mean())
        self.saturating = float(((self.q64 < 0) | (self.q64 > 255)).mean())


# ----------------------------------------------------------------------------------------------------------------- inputs
def _lattice(rng, H, W, bh, bw, lo=0, hi=255, channels=3, oy=0, ox=0):
    """(H,W,channels) random block lattice: blocks of bh x bw pixels (origin shifted by oy, ox), one value in lo..hi each"""
    ny, nx = (H + oy) // bh + 1, (W + ox) // bw + 1
    v = rng.integers(lo, hi + 1, (ny, nx, channels))
    yy = (np.arange(H) + oy) // bh
    xx = (np.arange(W) + ox) // bw
    return v[yy][:, xx]


def _u8(x):
    return np.clip(np.rint(x), 0, 255).astype(np.uint8)


def blocks(H, W, seed=0):
    """guide and source on different random 0..255 block lattices (11 x 7 and 37 x 19 pixels: mutually prime, no divisor of
    16 / 32 / 64 / 192), + 3 LSB of noise: hard edges at every phase of the kernel's strips, segments and row blocks.  (With
    23 x 29 guide blocks a 61 x 61 window holds so few guide colours that max|a| reaches 7..10 per channel, and the exempt
    share 17..21 % at 31 x 400, 40 x 2048, 512^2 and 1024^2: over the cap.  Smaller guide blocks keep it near 4 %.)"""
    rng = np.random.default_rng([seed, H, W, 1])
    g = _lattice(rng, H, W, 11, 7, oy=5, ox=3) + rng.integers(-3, 4, (H, W, 3))
    s = _lattice(rng, H, W, 37, 19, oy=13, ox=7) + rng.integers(-3, 4, (H, W, 3))
    return _u8(g), _u8(s)


def flat_guide(H, W, seed=0):
    """guide in a narrow band (levels 110 / 120 / 130, +-2 of noise: within 100..140), source a hard-edged 0 / 255 lattice of
    3 x 41 blocks: a ~ 0 (a few tenths), the output is close to a double box mean of the source.  The thin blocks keep
    adjacent rows different, which is what a one-row window shift shows up on when the image has barely more rows than r."""
    rng = np.random.default_rng([seed, H, W, 2])
    g = np.array([110.0, 120.0, 130.0]) + rng.integers(-2, 3, (H, W, 3))
    s = 255 * _lattice(rng, H, W, 3, 41, 0, 1, oy=1, ox=2)
    return _u8(g), _u8(s)


def saturating(H, W, seed=0):
    """a low-contrast guide (two levels 40 apart per channel, +-2 noise) over the SAME lattice as a 0 / 255 source: a ~ 255 / 40
    in total, so the guide's noise carries q64 past 0 and 255 on a large share of the pixels -- the clip is exercised"""
    rng = np.random.default_rng([seed, H, W, 3])
    s = _lattice(rng, H, W, 17, 13, 0, 1, channels=1, oy=4, ox=9)
    g = np.array([100.0, 110.0, 95.0]) + np.array([40.0, 30.0, 45.0]) * s + rng.integers(-2, 3, (H, W, 3))
    return _u8(g), _u8(255 * np.repeat(s, 3, axis=-1))


def constant(H, W, which):
    """'guide': constant guide, blocks source; 'src': blocks guide, constant source; 'both'.  The variance is exactly 0."""
    g, s = blocks(H, W, seed=7)
    if which in ("guide", "both"):
        g = np.broadcast_to(np.array([77, 130, 201], np.uint8), (H, W, 3)).copy()
    if which in ("src", "both"):
        s = np.broadcast_to(np.array([255, 0, 93], np.uint8), (H, W, 3)).copy()
    return g, s


def aliased(H, W, seed=0):
    """guide is src (one array, as bench.py passes one tensor twice): q ~ I wherever the variance is far above eps"""
    g, _ = blocks(H, W, seed=seed + 11)
    return g, g


def smooth(H, W, seed=5):
    """the pair of tests/gpu_diag.py:t_guided: a sinusoid plus noise, the source nearly a linear function of the guide"""
    rng = np.random.default_rng([seed, H, W])
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    sx, sy = (9.0, 7.0) if max(H, W) <= 128 else (19.0, 13.0)
    g = np.stack([(128 + 100 * np.sin(xx / sx + c) * np.cos(yy / sy)) for c in range(3)], -1)
    g = np.clip(g + rng.normal(0, 12, g.shape), 0, 255).astype(np.uint8)
    s = np.clip(g.astype(np.float64) * 0.6 + 50 + rng.normal(0, 25, g.shape), 0, 255).astype(np.uint8)
    return g, s


KINDS = {"blocks": blocks, "flat": flat_guide, "saturating": saturating, "aliased": aliased, "smooth": smooth,
         "const_guide": lambda H, W: constant(H, W, "guide"), "const_src": lambda H, W: constant(H, W, "src"),
         "const_both": lambda H, W: constant(H, W, "both")}

# radius 30: the extents of the strip / row-block / halo geometry (192-column strips, 32 and 64 rows per block, 16-output segments)
EXTENTS_R30 = ([(31, 31), (31, 400), (400, 31)] + [(h, 200) for h in (32, 33, 63, 64, 65, 97)] +
               [(70, w) for w in (191, 192, 193, 383, 385)] + [(40, 2048), (600, 530), (512, 512)])
CASES_R30 = ([(k, h, w) for (h, w) in EXTENTS_R30 for k in ("blocks", "flat")] + [("blocks", 1024, 1024)] +
             [("saturating", 97, 200), ("saturating", 70, 193), ("saturating", 31, 31),
              ("const_guide", 65, 200), ("const_src", 65, 200), ("const_both", 65, 200), ("const_both", 31, 31),
              ("aliased", 70, 193), ("aliased", 512, 512), ("smooth", 96, 96), ("smooth", 600, 530)])
# the cases on which a seeded defect has to violate the bar
SENSITIVE_KINDS = ("blocks", "flat")

# generic path: (kind, H, W, r, eps)
GENERIC_EXTENTS = ((70, 90), (200, 193))
CASES_GENERIC = ([(k, h, w, r, EPS) for (h, w) in GENERIC_EXTENTS for r in (1, 2, 7, 16, 31, 64) if r < min(h, w)
                  for k in ("blocks", "flat")] + [("blocks", 200, 193, 7, 1e-2 * 255 * 255), ("flat", 70, 90, 16, 1.0)])

# tuned instances of the fused launches: (rows per block of launch 1, of launch 2), on two blocks cases
TUNES = ((64, 64), (32, 32), (32, 128), (64, 128))
TUNE_CASES = (("blocks", 97, 193), ("blocks", 512, 512))


def case_id(c):
    return "%s-%dx%d" % c[:3] + ("-r%d" % c[3] + ("" if c[4] == EPS else "-eps%g" % c[4]) if len(c) > 3 else "")


@functools.lru_cache(maxsize=None)
def inputs(kind, H, W):
    g, s = KINDS[kind](H, W)
    g.setflags(write=False)
    s.setflags(write=False)
    return g, s


@functools.lru_cache(maxsize=None)
def ref(kind, H, W, r=30, eps=EPS):
    g, s = inputs(kind, H, W)
    return Ref(g, s, r, eps)
