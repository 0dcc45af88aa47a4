"""Cases, restatements and bars of the guided-matte tests (tests/test_gpu_gmatte.py, tests/test_gmatte_cases_cpu.py): a matte
refined by the photo's own pixels -- the colour guided filter with the matte as its one source channel
(ppst_guided_matte_coeffs, csrc/guided_filter.hip) and the paste that evaluates the matte from those coefficients on each photo
pixel (ppst_guided_filter_paste_gmatte).  Plain numpy on the CPU: nothing here touches the device, and the device is never its own
judge.  Guides, window means, planes, transforms, photos, mattes and the boundary-aware bar are gf_cases', gf_native_cases',
region_cases' and matte_cases' (imported, not changed).

Semantics (include/ppst_hip.h).  Source p = rint(255 clamp(m, 0, 1)), ties to even, a NaN gives 0.  Matte coefficients: planes 0..3
of the colour filter's mean planes on the source (p, p, p): mean a_0..2, mean b.  Paste: matte_cases.paste_matte with
m^ = clamp((M0 I0 + M1 I1 + M2 I2 + Mb) (1/255), 0, 1), (M0, M1, M2, Mb) the four planes sampled like the 12 colour planes and I the
photo's own pixel; g = g_edge m^; a pixel with g == 0 keeps the photo's byte; the weight output is rint(255 g) inside the square.

Restatements, each in the dtype of the run: ``quantise``, ``mcoeffs``, ``paste_gmatte``.

Bars.  Coefficients on the device: bit-equal to ops.guided_filter_coeffs on (p, p, p); against float64 gf_native_cases.plane_ref's
rule, 2 max|planes32 - planes64| + 1e-6 max|planes64|.  Paste: gf_cases.judge(ref64, got, tau), tau = 2 max|ref32 - ref64| + 1e-3;
bytes outside the square and bytes where the float64 run's g is exactly 0 EQUAL the photo's.  Weight: the same judge against
255 g64 with a tau from its own two runs; 0 outside the square.

Seeded defects of the paste (``defect=``), so that the CPU test can show that the cases see them:
  "nearest"   the matte coefficients sampled at the nearest tap instead of bilinearly;
  "noclamp"   m^ not clamped;
  "clamplow"  m^ clamped below only;
  "grey"      the three a planes applied to the grey mean of I;
  "bonly"     m^ from the b plane alone;
  "zeros"     matte-coefficient taps outside the plane read as 0;
  "tilefoot"  the matte coefficients' staged footprint of a PASTE_T tile one column short.
"""
import functools

import numpy as np

import gf_cases as G
import gf_native_cases as N
import matte_cases as M
import region_cases as C

R = 8                                   # the defaults of ops.guided_matte_coeffs
EPS = (0.01 * 255) ** 2
PASTE_DEFECTS = ("nearest", "noclamp", "clamplow", "grey", "bonly")
GEOMETRIC_DEFECTS = ("zeros", "tilefoot")


# ------------------------------------------------------------------------------------------------------------ restatements
def quantise(m, dtype=np.float64):
    """matte values -> the filter's source rint(255 clamp(m, 0, 1)) in ``dtype``: an integer in 0..255, ties to even, NaN -> 0"""
    m = np.asarray(m).astype(dtype)
    c = np.fmin(np.fmax(m, dtype(0)), dtype(1)).astype(dtype)          # (fmax / fmin drop a NaN, as fmaxf / fminf do)
    return np.rint((dtype(255) * c).astype(dtype)).astype(dtype)


def mcoeffs(guide, m, r, eps=EPS, dtype=np.float64):
    """(h,w,3) uint8 guide, (h,w) matte -> (4,h,w) of ``dtype``: mean a_0..2 and mean b of the filter on the source (p, p, p)"""
    p = quantise(m, dtype)
    return N.mean_planes(guide, np.stack([p, p, p], -1), r, eps, dtype)[:4]


def paste_gmatte(planes, mco, photo, xf, feather, dtype=np.float64, defect=None, want_g=False):
    """matte_cases.paste_matte with the matte evaluated from its coefficients on the photo's pixel: (12,n,n) colour planes,
    (4,n,n) matte coefficients, (H,W,3) uint8 -> unrounded output (H,W,3) of ``dtype``; pixels outside the square and pixels with
    g == 0 hold the photo's bytes, exactly.  ``want_g``: also the (H,W) blend weight (0 outside the square)."""
    n = planes.shape[-1]
    H, W = photo.shape[:2]
    m, U, V = C.inside(xf, n, H, W)
    out = photo.astype(dtype)
    gmap = np.zeros((H, W), dtype)
    if not m.any():
        return (out, gmap) if want_g else out
    P = np.concatenate([planes, mco], 0).astype(dtype)
    Ui, Vi = U[m] - C.HALF, V[m] - C.HALF
    i0, j0 = Ui >> 24, Vi >> 24
    fx = ((Ui & (C.ONE - 1)).astype(dtype) / dtype(C.ONE)).astype(dtype)
    fy = ((Vi & (C.ONE - 1)).astype(dtype) / dtype(C.ONE)).astype(dtype)
    c0, c1, r0, r1 = np.clip(i0, 0, n - 1), np.clip(i0 + 1, 0, n - 1), np.clip(j0, 0, n - 1), np.clip(j0 + 1, 0, n - 1)
    one = dtype(1)

    def sample(Q, c0, c1, r0, r1, w00=1, w01=1, w10=1, w11=1):
        top = ((one - fx) * (Q[:, r0, c0] * w00) + fx * (Q[:, r0, c1] * w01)).astype(dtype)
        bot = ((one - fx) * (Q[:, r1, c0] * w10) + fx * (Q[:, r1, c1] * w11)).astype(dtype)
        return ((one - fy) * top + fy * bot).astype(dtype)
    co = sample(P[:12], c0, c1, r0, r1)
    if defect == "nearest":
        mc = P[12:, np.where(fy < 0.5, r0, r1), np.where(fx < 0.5, c0, c1)]
    elif defect == "zeros":
        okc0, okc1, okr0, okr1 = (i0 >= 0), (i0 + 1 <= n - 1), (j0 >= 0), (j0 + 1 <= n - 1)
        mc = sample(P[12:], c0, c1, r0, r1, okc0 & okr0, okc1 & okr0, okc0 & okr1, okc1 & okr1)
    elif defect == "tilefoot":
        hi, lo = C._tile_last(xf, n, H, W, None)
        hi, lo = hi[m], lo[m]
        d0 = np.where((c0 == hi) & (hi > lo), c0 - 1, c0)
        d1 = np.where((c1 == hi) & (hi > lo), c1 - 1, c1)
        mc = sample(P[12:], d0, d1, r0, r1)
    else:
        mc = sample(P[12:], c0, c1, r0, r1)
    I = photo[m].astype(dtype)
    if defect == "grey":
        grey = ((I[:, 0] + I[:, 1] + I[:, 2]) / dtype(3)).astype(dtype)
        v = (mc[0] + mc[1] + mc[2]) * grey + mc[3]
    elif defect == "bonly":
        v = mc[3]
    else:
        v = mc[0] * I[:, 0] + mc[1] * I[:, 1] + mc[2] * I[:, 2] + mc[3]
    # (a true division: the kernel multiplies by the rounded 1 / 255, one more rounding in float32 -- the restatement's float32
    #  floor, and with it tau, is the smaller of the two: 6.4e-5 against 7.3e-5 over the 19 cases)
    v = (v.astype(dtype) / dtype(255)).astype(dtype)
    if defect == "noclamp":
        mh = np.where(np.isnan(v), dtype(0), v)
    elif defect == "clamplow":
        mh = np.fmax(v, dtype(0))
    else:
        mh = np.fmin(np.fmax(v, dtype(0)), one)                          # (a NaN gives 0)
    if feather > 0:
        d = np.minimum(np.minimum(U[m], n * C.ONE - U[m]), np.minimum(V[m], n * C.ONE - V[m]))
        t = np.clip(d.astype(dtype) / dtype(C.ONE) / dtype(feather), 0, 1).astype(dtype)
        g = (t * t * (dtype(3) - dtype(2) * t)).astype(dtype)
    else:
        g = np.ones(I.shape[0], dtype)
    g = (g * mh).astype(dtype)
    res = np.empty_like(I)
    for c in range(3):
        q = co[4 * c] * I[:, 0] + co[4 * c + 1] * I[:, 1] + co[4 * c + 2] * I[:, 2] + co[4 * c + 3]
        with np.errstate(invalid="ignore"):
            res[:, c] = np.where(g == 0, I[:, c], g * q + (one - g) * I[:, c])
    out[m] = res
    gmap[m] = g
    return (out, gmap) if want_g else out


# ------------------------------------------------------------------------------------------------------ coefficient cases
# the device is compared bit for bit with ops.guided_filter_coeffs on (p, p, p): (kind, h, w, r), r < min(h, w)
COEFF_KINDS = ("blocks", "flat")
COEFF_EXTENTS = ((70, 90), (200, 193))
COEFF_RADII = (1, 3, 8, 16, 64)
COEFF_CASES = [(k, h, w, r) for (h, w) in COEFF_EXTENTS for r in COEFF_RADII if r < min(h, w) for k in COEFF_KINDS]
MATTES = ("blob", "zeros", "ones", "uniform-nan", "ties")


@functools.lru_cache(maxsize=None)
def blob_matte(h, w):
    """matte_cases' blob labels through its matte at (feather, grow) = (16, 8), fp32"""
    m = M.matte(M.sd2_separable(M._blob(h, w, 4), M.FACE, 16, 8), 16, 8, np.float32)
    m.setflags(write=False)
    return m


def matte_of(name, h, w):
    """the fp32 matte fields of the coefficient tests"""
    if name == "blob":
        return blob_matte(h, w)
    if name == "zeros":
        return np.zeros((h, w), np.float32)
    if name == "ones":
        return np.ones((h, w), np.float32)
    rng = np.random.default_rng([h, w, 11])
    if name == "uniform-nan":                                             # values below 0 and above 1, one NaN in 16
        m = rng.uniform(-0.5, 1.5, (h, w)).astype(np.float32)
        m[rng.random((h, w)) < 1.0 / 16] = np.nan
        return m
    if name == "ties":                                                    # (k + 0.5) / 255 as fp32 holds it
        return ((rng.integers(0, 255, (h, w)).astype(np.float64) + 0.5) / 255.0).astype(np.float32)
    raise KeyError(name)


def source_u8(m):
    """the source bytes the device forms from an fp32 matte: ``quantise`` in float32, as uint8"""
    return quantise(np.asarray(m, np.float32), np.float32).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def plane_ref(kind, h, w, r):
    """gf_native_cases.plane_ref's rule on the blob matte -> (guide, matte, planes64, bar, floor32):
    bar = 2 max|planes32 - planes64| + 1e-6 max|planes64|, from the restatement alone"""
    g = G.inputs(kind, h, w)[0]
    m = blob_matte(h, w)
    p64 = mcoeffs(g, m, r, EPS, np.float64)
    p32 = mcoeffs(g, m, r, EPS, np.float32)
    floor32 = float(np.abs(p32.astype(np.float64) - p64).max())
    return g, m, p64, 2 * floor32 + 1e-6 * float(np.abs(p64).max()), floor32


# ------------------------------------------------------------------------------------------------------------- paste cases
class PasteGRef(C._Bar):
    """the guided-matte paste of one region case: matte_cases.paste_ref's photo, transform, feather, fp32 colour planes and fp32
    matte; the guide of the matte filter is the case's crop (region_cases.extract_ref, rounded); its radius min(3, n - 1); the
    matte coefficients fed to both runs of the restatement (and to the device) are the float64 restatement's, rounded to fp32"""

    def __init__(self, case):
        P = M.paste_ref(case)
        self.case, self.n, self.photo, self.xf, self.feather, self.planes, self.inside = case, P.n, P.photo, P.xf, P.feather, P.planes, P.inside
        self.M, self.r = P.M, min(3, P.n - 1)
        self.guide = np.ascontiguousarray(C.extract_ref(case).expect)
        self.mco = mcoeffs(self.guide, self.M, self.r, EPS, np.float64).astype(np.float32)
        self.ref64, self.g64 = paste_gmatte(self.planes, self.mco, self.photo, self.xf, self.feather, np.float64, want_g=True)
        self.ref32, g32 = paste_gmatte(self.planes, self.mco, self.photo, self.xf, self.feather, np.float32, want_g=True)
        self.untouched = ~self.inside | (self.g64 == 0)
        self._bar(self.ref64, self.ref32, self.inside)
        # the weight output: 255 g, judged like the image, with a tau from its own two runs
        self.w64 = 255.0 * self.g64
        self.wfloor32 = float(np.abs(255.0 * g32.astype(np.float64) - self.w64).max())
        self.wtau = 2 * self.wfloor32 + 1e-3
        for a in (self.mco, self.ref64, self.ref32, self.g64, self.w64):
            a.setflags(write=False)

    def defect(self, name):
        return G.round_u8(paste_gmatte(self.planes, self.mco, self.photo, self.xf, self.feather, np.float64, name))


@functools.lru_cache(maxsize=None)
def paste_ref(case):
    return PasteGRef(C.lookup(case))


def judge_paste(Rf, got_u8):
    """gf_cases.judge on the whole photo + byte equality outside the square and where g64 == 0 -> list of violated clauses"""
    return M.judge_paste(Rf, got_u8)


def judge_weight(Rf, got_u8):
    """the weight plane (H,W) uint8 against 255 g64 -> list of violated clauses"""
    bad = G.judge(Rf.w64, got_u8, Rf.wtau)
    if got_u8[~Rf.inside].any():
        bad.append("%d weights outside the square are not 0" % int((got_u8[~Rf.inside] != 0).sum()))
    return bad


# -------------------------------------------------------------------------------------------------------------- leak cases
LEAK_CASES = [c for c in C.ALL_CASES if c[3] >= 24]
LEAK_R = 2


def disc_matte(n):
    """a speck-free centred disc of radius n / 4 as a hard 0 / 1 matte: matte_cases' transform at (feather, grow) = (0, 0)"""
    yy, xx = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    lab = (((yy - (n - 1) / 2.0) ** 2 + (xx - (n - 1) / 2.0) ** 2) <= (n / 4.0) ** 2).astype(np.uint8)
    return M.matte(M.sd2_separable(lab, M.FACE, 0, 0), 0, 0, np.float32)


def poison(planes, mco):
    """the colour planes with NaN wherever all four matte-coefficient planes are exactly 0 at every sample within 2 pixels"""
    return M.poison(planes, (mco != 0).any(0).astype(np.float32))
