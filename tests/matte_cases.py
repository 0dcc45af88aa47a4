"""Cases, restatements and bars of the matte tests (tests/test_gpu_matte.py, tests/test_matte_cases_cpu.py): a label map turned
into a feathered matte by an exact, clipped, signed Euclidean distance transform (ppst_label_matte, csrc/matte.hip) and the guided
filter's coefficients pasted into a photograph through that matte (ppst_guided_filter_paste_matte, csrc/guided_filter.hip).  Plain
numpy on the CPU: nothing here touches the device, and the device is never its own judge.  The transform, the photos, the
coefficient planes and the boundary-aware bar are region_cases', gf_cases' and gf_native_cases' (imported, not changed).

Semantics (include/ppst_hip.h).  A pixel is inside iff its label L < 32 and bit L of ``keep`` is set.  R = max(grow, max(feather -
grow, 0)) + 1.  D2(p) = min(R^2, min |p - q|^2) over the pixels q of the plane whose inside-ness differs from p's (no such pixel:
R^2; the plane's edge is no boundary); sd2 = +D2 inside, -D2 outside.  sd = sign (sqrt(D2) - 1/2); feather > 0:
t = clamp((sd + grow) / feather, 0, 1), m = t^2 (3 - 2t); feather == 0: m = [sd + grow > 0].  The paste is region_cases.paste with
g = g_edge m^, m^ the matte sampled like a 13th coefficient plane; a pixel with g == 0 keeps the photo's byte.

Restatements: ``sd2_brute`` (the definition: a minimum over all opposite pixels), ``sd2_separable`` (columns, then rows),
``matte`` and ``paste_matte`` in the dtype of the run.

Bars.  sd2: bit-equal.  Matte: |got - m64| <= 2 max|m32 - m64| + 1e-6 (the 1e-6: fused or differently rounded fp32 steps, at most
8 operations on values <= 3).  Paste: gf_cases.judge(ref64, got, tau), tau = 2 max|ref32 - ref64| + 1e-3; bytes outside the square
and bytes where the restatement's g is exactly 0 EQUAL the photo's.

Seeded defects (``defect=``), so that the CPU test can show that the cases see them:
  transform  "chebyshev", "cityblock" (the metric); "edge" (the plane's edge counted as outside); "outzero" (outside pixels get 0);
             "clip" (clipped at (R - 1)^2); "nohalo" (column segments of MT_SEG rows that do not look past their own rows);
             "rowseam" (row windows that stop at the MT_ROW seam); "keepshift" (keep shifted by one bit); "wrap31" (labels >= 32
             wrapped with & 31)
  matte      "nohalf" (no - 1/2), "nogrow" (grow ignored), "linear" (t instead of the smoothstep)
  paste      "nomatte" (matte ignored), "nearest" (matte sampled at the nearest tap), "zeros" (matte taps outside the plane read
             as 0), "tilefoot" (the matte's staged footprint of a PASTE_T tile one column short)
"""
import functools

import numpy as np

import gf_cases as G
import gf_native_cases as N
import region_cases as C

# csrc/matte.hip: rows of a column segment of launch 1, threads of a row block of launch 2 (test_matte_cases_cpu reads them)
MT_SEG = 32
MT_ROW = 256

FG = [(0, 0), (1, 0), (1, 1), (6, 3), (16, 8), (0, 5), (255, 0), (255, 255)]      # (feather, grow)
SD2_DEFECTS = ("chebyshev", "cityblock", "edge", "outzero", "clip", "nohalo", "rowseam", "keepshift", "wrap31")
MATTE_DEFECTS = ("nohalf", "nogrow", "linear")
PASTE_DEFECTS = ("nomatte", "nearest", "zeros", "tilefoot")


def radius(feather, grow):
    return max(grow, max(feather - grow, 0)) + 1


def keep_mask(keep):
    m = 0
    for k in keep:
        m |= 1 << int(k)
    return m


def inside_of(labels, keep, defect=None):
    """(…,h,w) uint8 labels, ``keep`` a 32-bit mask -> bool"""
    L = labels.astype(np.int64)
    keep = int(keep) >> 1 if defect == "keepshift" else int(keep)
    bit = (keep >> np.minimum(L & 31 if defect == "wrap31" else L, 31)) & 1
    return (bit == 1) & ((L < 32) | (defect == "wrap31"))


# ------------------------------------------------------------------------------------------------------------ restatements
def sd2_brute(labels, keep, feather, grow):
    """the definition: for every pixel the minimum over ALL pixels of the other class.  (h,w) uint8 -> (h,w) int32"""
    ins = inside_of(labels, keep)
    h, w = ins.shape
    R2 = radius(feather, grow) ** 2
    yy, xx = np.meshgrid(np.arange(h, dtype=np.int64), np.arange(w, dtype=np.int64), indexing="ij")
    d2 = np.full((h, w), R2, np.int64)
    for cls in (True, False):
        py, px = yy[ins == cls], xx[ins == cls]                     # the pixels of this class ...
        qy, qx = yy[ins != cls], xx[ins != cls]                     # ... and all of the other
        if not py.size or not qy.size:
            continue
        best = np.empty(py.size, np.int64)
        for k in range(0, py.size, 1024):
            dy, dx = py[k:k + 1024, None] - qy[None], px[k:k + 1024, None] - qx[None]
            best[k:k + 1024] = (dy * dy + dx * dx).min(axis=1)
        d2[ins == cls] = np.minimum(best, R2)
    return np.where(ins, d2, -d2).astype(np.int32)


def _column_distance(target, R, nohalo):
    """(h,w) bool -> per pixel the vertical distance, clipped to R, to the nearest True pixel of its column"""
    h, w = target.shape
    out = np.full((h, w), R, np.int64)
    for rows in (range(h), range(h - 1, -1, -1)):
        d = np.full(w, R, np.int64)
        for y in rows:
            if nohalo and (y % MT_SEG == 0 if rows.step == 1 else y % MT_SEG == MT_SEG - 1):
                d[:] = R
            d = np.where(target[y], 0, np.minimum(d + 1, R))
            out[y] = np.minimum(out[y], d)
    return out


def sd2_separable(labels, keep, feather, grow, defect=None):
    """the same by columns, then rows: g = vertical distance to the nearest pixel of the OTHER class in the column (clipped to R),
    D2 = min(R^2, min_dx dx^2 + g(x + dx)^2).  (h,w) uint8 -> (h,w) int32"""
    ins = inside_of(labels, keep, defect)
    h, w = ins.shape
    R = radius(feather, grow)
    hh, ww = h, w
    to_out, to_in = _column_distance(~ins, R, defect == "nohalo"), _column_distance(ins, R, defect == "nohalo")
    clip = (R - 1) ** 2 if defect == "clip" else R * R
    xs = np.arange(ww)
    best = {}
    for cls, g in ((True, to_out), (False, to_in)):
        b = np.full((hh, ww), clip, np.int64)
        for dx in range(0, min(R, ww)):
            for sgn in ((1, -1) if dx else (1,)):
                src = xs + sgn * dx
                ok = (src >= 0) & (src < ww)
                if defect == "rowseam":
                    ok &= (np.clip(src, 0, ww - 1) // MT_ROW) == (xs // MT_ROW)
                gg = g[:, np.clip(src, 0, ww - 1)]
                if defect == "chebyshev":
                    cand = np.maximum(dx, gg) ** 2
                elif defect == "cityblock":
                    cand = (dx + gg) ** 2
                else:
                    cand = dx * dx + gg * gg
                b = np.where(ok[None], np.minimum(b, cand), b)
        best[cls] = b
    d2 = np.where(ins, best[True], best[False])
    if defect == "edge":                                             # (the nearest pixel beyond the edge lies straight across it)
        yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        e = np.minimum(np.minimum(yy + 1, h - yy), np.minimum(xx + 1, w - xx))
        d2 = np.where(ins, np.minimum(d2, e * e), d2)
    sd2 = np.where(ins, d2, 0 if defect == "outzero" else -d2)
    return sd2.astype(np.int32)


def matte(sd2, feather, grow, dtype=np.float64, defect=None):
    """int32 sd2 -> matte of ``dtype``, step by step in that dtype"""
    s = np.sqrt(np.abs(sd2).astype(dtype)).astype(dtype)
    if defect != "nohalf":
        s = (s - dtype(0.5)).astype(dtype)
    u = (np.where(sd2 > 0, s, -s).astype(dtype) + dtype(0 if defect == "nogrow" else grow)).astype(dtype)
    if feather == 0:
        return (u > 0).astype(dtype)
    t = np.clip((u / dtype(feather)).astype(dtype), dtype(0), dtype(1))
    if defect == "linear":
        return t.astype(dtype)
    return (t * t * (dtype(3) - dtype(2) * t)).astype(dtype)


def paste_matte(planes, M, photo, xf, feather, dtype=np.float64, defect=None, want_g=False):
    """region_cases.paste's arithmetic with the matte as a 13th plane: (12,n,n) planes, (n,n) matte, (H,W,3) uint8 -> unrounded
    output (H,W,3) of ``dtype``; pixels outside the square and pixels with g == 0 hold the photo's bytes, exactly.
    ``want_g``: also the (H,W) blend weight (0 outside the square)."""
    n = planes.shape[-1]
    H, W = photo.shape[:2]
    m, U, V = C.inside(xf, n, H, W)
    out = photo.astype(dtype)
    gmap = np.zeros((H, W), dtype)
    if not m.any():
        return (out, gmap) if want_g else out
    P = np.concatenate([planes, M[None]], 0).astype(dtype)
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
    if defect == "nomatte":
        mh = np.ones_like(fx)
    elif defect == "nearest":
        mh = P[12, np.where(fy < 0.5, r0, r1), np.where(fx < 0.5, c0, c1)]
    elif defect == "zeros":
        okc0, okc1, okr0, okr1 = (i0 >= 0), (i0 + 1 <= n - 1), (j0 >= 0), (j0 + 1 <= n - 1)
        mh = sample(P[12:], c0, c1, r0, r1, okc0 & okr0, okc1 & okr0, okc0 & okr1, okc1 & okr1)[0]
    elif defect == "tilefoot":
        hi, lo = C._tile_last(xf, n, H, W, None)
        hi, lo = hi[m], lo[m]
        d0 = np.where((c0 == hi) & (hi > lo), c0 - 1, c0)
        d1 = np.where((c1 == hi) & (hi > lo), c1 - 1, c1)
        mh = sample(P[12:], d0, d1, r0, r1)[0]
    else:
        mh = sample(P[12:], c0, c1, r0, r1)[0]
    I = photo[m].astype(dtype)
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


# ------------------------------------------------------------------------------------------------------------ label patterns
def _blob(h, w, seed):
    """an ellipse face (1) under a hair cap (2) on background (0), + single-pixel specks of face in the background and
    single-pixel holes in the face"""
    rng = np.random.default_rng([seed, h, w])
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    cy, cx = (h - 1) / 2.0 + 0.04 * h, (w - 1) / 2.0
    ry, rx = max(0.33 * h, 0.6), max(0.26 * w, 0.6)
    e = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2
    L = np.zeros((h, w), np.uint8)
    L[(((yy - cy) / (1.25 * ry)) ** 2 + ((xx - cx) / (1.3 * rx)) ** 2 <= 1) & (yy < cy - 0.3 * ry)] = 2
    L[e <= 1] = 1
    k = min(max(1, h * w // 150), 12)                               # (a few: grown specks must not fill a large background)
    ys, xs = rng.integers(0, h, 2 * k), rng.integers(0, w, 2 * k)
    L[ys[:k], xs[:k]] = np.where(L[ys[:k], xs[:k]] == 0, 1, 0)      # a speck in the background, a hole in the face or hair
    L[ys[k:], xs[k:]] = np.where(L[ys[k:], xs[k:]] == 0, 2, 0)
    return L


def _values(h, w, seed):
    rng = np.random.default_rng([seed, h, w, 7])
    vals = np.array([0, 1, 2, 3, 31, 32, 255], np.uint8)
    bh, bw = 5, 7
    idx = rng.integers(0, len(vals), (h // bh + 1, w // bw + 1))
    return vals[np.kron(idx, np.ones((bh, bw), np.int64))[:h, :w]]


def _seam(h, w, axis):
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    if axis == 0:
        return (yy < (MT_SEG if h > MT_SEG else h // 2)).astype(np.uint8)
    return (xx < (MT_ROW if w > MT_ROW else w // 2)).astype(np.uint8)


def _grid(h, w):
    return np.meshgrid(np.arange(h), np.arange(w), indexing="ij")


FACE = keep_mask((1, 2))
# name -> (labels(h, w), keep mask)
PATTERNS = {
    "blob": lambda h, w: (_blob(h, w, 1), FACE),
    "dot": lambda h, w: (((_grid(h, w)[0] == h // 2) & (_grid(h, w)[1] == w // 2)).astype(np.uint8), FACE),
    "hole": lambda h, w: (1 - ((_grid(h, w)[0] == h // 2) & (_grid(h, w)[1] == w // 2)).astype(np.uint8), FACE),
    "full": lambda h, w: (np.full((h, w), 2, np.uint8), FACE),
    "empty": lambda h, w: (np.zeros((h, w), np.uint8), FACE),
    "checker": lambda h, w: (((_grid(h, w)[0] + _grid(h, w)[1]) & 1).astype(np.uint8), FACE),
    "diagonal": lambda h, w: ((2 * (_grid(h, w)[0] * w + _grid(h, w)[1] * h) < h * w + max(h, w)).astype(np.uint8), FACE),
    "seam-row": lambda h, w: (_seam(h, w, 0), FACE),
    "seam-col": lambda h, w: (_seam(h, w, 1), FACE),
    "values": lambda h, w: (_values(h, w, 2), keep_mask((0, 2, 31))),
    "values-hi": lambda h, w: (_values(h, w, 3), keep_mask((3, 31))),
}
SHAPES = [(1, 1), (1, 37), (37, 1), (8, 8), (24, 24), (40, 40), (MT_SEG - 1, 33), (MT_SEG, 33), (MT_SEG + 1, 33), (2 * MT_SEG + 1, 70),
          (20, MT_ROW - 1), (20, MT_ROW), (20, MT_ROW + 1), (70, 2 * MT_ROW + 3)]
BIG = (520, 520)                                     # judged by sd2_separable only
BIG_PATTERNS = ("blob", "seam-row", "seam-col", "values")


def _table():
    out, i = [], 0
    for (h, w) in SHAPES + [BIG]:
        for p in (BIG_PATTERNS if (h, w) == BIG else PATTERNS):
            f, g = FG[i % len(FG)]
            i += 3                                               # (3 and 8 are coprime: every pattern meets every pair)
            out.append(("%s-%dx%d-f%d-g%d" % (p, h, w, f, g), h, w, p, f, g))
    return out


# (name, h, w, pattern, feather, grow)
CASES = _table()


def case_id(c):
    return c[0]


def cases_of(shape):
    return [c for c in CASES if (c[1], c[2]) == tuple(shape)]


class MatteRef:
    """one case: labels, keep, the restatement's sd2 and the matte in float64 and float32, and the matte's bar from the two"""

    def __init__(self, case):
        _, h, w, p, f, g = case
        self.case, self.feather, self.grow = case, f, g
        self.labels, self.keep = PATTERNS[p](h, w)
        self.sd2 = sd2_separable(self.labels, self.keep, f, g)
        self.m64, self.m32 = matte(self.sd2, f, g, np.float64), matte(self.sd2, f, g, np.float32)
        self.floor32 = float(np.abs(self.m32.astype(np.float64) - self.m64).max())
        self.tol = 2 * self.floor32 + 1e-6
        for a in (self.labels, self.sd2, self.m64, self.m32):
            a.setflags(write=False)

    def sd2_defect(self, name):
        return sd2_separable(self.labels, self.keep, self.feather, self.grow, name)

    def matte_defect(self, name):
        return matte(self.sd2, self.feather, self.grow, np.float64, name)


@functools.lru_cache(maxsize=None)
def matte_ref(case):
    return MatteRef(case)


# ------------------------------------------------------------------------------------------------------------- paste cases
def _paste_fg():
    out, i = {}, 0
    for c in C.ALL_CASES:
        while radius(*FG[i % len(FG)]) > c[3]:
            i += 1
        out[c[0]] = FG[i % len(FG)]
        i += 1
    return out


PASTE_FG = _paste_fg()                               # region case name -> (matte_feather, matte_grow), R <= n


class PasteMatteRef(C._Bar):
    """the matte paste of one region case: region_cases.PasteRef's photo, transform, feather and fp32 planes; the blob labels at
    the case's n; the matte plane fed to both runs of the restatement (and to the device) is the fp32 restatement's matte"""

    def __init__(self, case):
        P = C.paste_ref(case)
        self.case, self.n, self.photo, self.xf, self.feather, self.planes, self.inside = case, P.n, P.photo, P.xf, P.feather, P.planes, P.inside
        self.mf, self.mg = PASTE_FG[case[0]]
        self.labels = _blob(P.n, P.n, 4)
        self.M = matte(sd2_separable(self.labels, FACE, self.mf, self.mg), self.mf, self.mg, np.float32)
        self.ref64, g64 = paste_matte(self.planes, self.M, self.photo, self.xf, self.feather, np.float64, want_g=True)
        self.ref32 = paste_matte(self.planes, self.M, self.photo, self.xf, self.feather, np.float32)
        self.untouched = ~self.inside | (g64 == 0)
        self._bar(self.ref64, self.ref32, self.inside)

    def defect(self, name):
        return G.round_u8(paste_matte(self.planes, self.M, self.photo, self.xf, self.feather, np.float64, name))


@functools.lru_cache(maxsize=None)
def paste_ref(case):
    return PasteMatteRef(C.lookup(case))


def judge_paste(Rf, got_u8):
    """gf_cases.judge on the whole photo + byte equality outside the square and where g == 0 -> list of violated clauses"""
    bad = G.judge(Rf.ref64, got_u8, Rf.tau)
    u = Rf.untouched
    if not np.array_equal(got_u8[u], Rf.photo[u]):
        bad.append("%d bytes outside the square or under a zero weight differ from the photo" % int((got_u8[u] != Rf.photo[u]).sum()))
    return bad


def poison(planes, M):
    """the planes with NaN wherever every matte sample within 2 pixels is 0"""
    n = M.shape[-1]
    pad = np.pad(M > 0, 2, constant_values=False)
    near = np.zeros((n, n), bool)
    for dy in range(5):
        for dx in range(5):
            near |= pad[dy:dy + n, dx:dx + n]
    out = planes.copy()
    out[:, ~near] = np.nan
    return out
