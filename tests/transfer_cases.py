"""Case table and judges of the colour-transfer baselines (csrc/colour_transfer.hip; include/ppst_hip.h "colour transfer").
Importing this needs no GPU.  test_transfer_cases_cpu.py pins the judges; test_gpu_transfer.py holds the kernels to them.

The cases are those of colour_cases.CASES (the same shapes, seeds and label maps: 1 x 1, no labels, an odd batch, flat images, four
regions over several blocks, label 255 with a region empty on one side only, a crop view, the {0, 255}^3 extremes); the style
batch is a second seeded batch of the same shape whose label maps are the content's in reverse batch order.

Judges:
  * ``lut_judge``: the histogram-specification rule in numpy int64 (np.searchsorted on the monotone left side); ``lut_loop`` is
    its second, loop-written form in Python integers;
  * ``apply_lut`` / ``apply_affine``: both apply modes from the same integers, labels, maps and weights, in float64 (the judge)
    or float32 (sets the bar).  They return the UNROUNDED byte values q (a pixel of no region: its input bytes), so the device is
    judged by the project's boundary-aware bar, ``gf_cases.judge(q64, device, tau)`` with ``tau = 2 max|q32 - q64| + 1e-3``;
  * ``gaussian_rows``: the Monge-Kantorovich and Reinhard rows in float64 numpy.
The keyword switches of the judges seed the defects a kernel of this kind makes (DEFECTS); the CPU test shows that the cases SEE
each of them through the bar before the device is trusted by them.
"""
import numpy as np
import torch

import colour_cases as C
import gf_cases as G

CASES = C.CASES
NAMES = list(CASES)
EXEMPT_CAP = 0.01          # share of values within tau of a rounding boundary, where either neighbour passes
FLOOR, MAX_GAIN = 1e-2, 8.0
# the style batch's seed is 900 + the case's place in the table, except where that batch puts a whole cluster of equal pixels
# within tau of a rounding boundary: "extremes" has 8 colours x 2 regions, so one such value is 1.3 % of the case
STYLE_SEED = {"extremes": 914}


def make_case(name):
    """-> dict(img, labels, img_s, labels_s (torch uint8; labels None without a map), R, weights (numpy fp32 (B, R, H, W)), and
    the view entries of colour_cases.make_case)"""
    c = C.make_case(name)
    k = NAMES.index(name)
    B, H, W, _ = c["img"].shape
    kind = CASES[name].get("kind", "smooth")
    c["img_s"] = C.make_images(STYLE_SEED.get(name, 900 + k), B, H, W, kind="corners" if kind == "corners" else "smooth")
    c["labels_s"] = None if c["labels"] is None else c["labels"].flip(0).contiguous()
    c["weights"] = make_weights(1300 + k, B, c["R"], H, W)
    return c


def make_weights(seed, B, R, H, W):
    """fp32 (B, R, H, W) >= 0, NOT normalised (sums between 0 and about 3): a seeded random field; about a tenth of the pixels
    have all weights 0 (the hard label decides) and about a tenth are one-hot"""
    rng = np.random.default_rng(seed)
    w = rng.random((B, R, H, W)) ** 2 * 1.5
    sel = rng.random((B, 1, H, W))
    hot = rng.integers(0, R, (B, 1, H, W)) == np.arange(R).reshape(1, R, 1, 1)
    w = np.where(sel < 0.1, 0.0, np.where(sel < 0.2, hot * 1.0, w))
    return w.astype(np.float32)


# ------------------------------------------------------------------------------------------------------------ the tables
def lut_judge(hc, hs, cdf="midpoint", swap_counts=False):
    """LUT[v] = min{u : 2 cumS(u) nC >= (cumC(v - 1) + cumC(v)) nS} in int64; the identity where a side is empty.
    Defects: ``cdf="inclusive"`` (2 cumC(v) in place of the mid-point), ``swap_counts`` (nS and nC exchanged)."""
    hc, hs = np.asarray(hc, dtype=np.int64), np.asarray(hs, dtype=np.int64)
    cc, cs = np.cumsum(hc), np.cumsum(hs)
    nC, nS = int(cc[-1]), int(cs[-1])
    if nC == 0 or nS == 0:
        return np.arange(256, dtype=np.uint8)
    if swap_counts:
        nC, nS = nS, nC
    below = np.concatenate(([0], cc[:-1]))
    rhs = (2 * cc if cdf == "inclusive" else below + cc) * nS
    return np.minimum(np.searchsorted(2 * cs * nC, rhs, side="left"), 255).astype(np.uint8)


def lut_loop(hc, hs):
    """the same rule, level by level, in Python integers"""
    hc, hs = [int(v) for v in hc], [int(v) for v in hs]
    nC, nS = sum(hc), sum(hs)
    if nC == 0 or nS == 0:
        return np.arange(256, dtype=np.uint8)
    out, cum_c = [], 0
    for v in range(256):
        rhs = (cum_c + cum_c + hc[v]) * nS
        cum_c += hc[v]
        cum_s = 0
        for u in range(256):
            cum_s += hs[u]
            if 2 * cum_s * nC >= rhs:
                break
        out.append(u)
    return np.array(out, dtype=np.uint8)


def luts_judge(hist_c, hist_s, pairs, **defect):
    """(K, R, 3, 256) uint8 from the judges' histograms (B, R, P, 256), projections 0..2"""
    R = hist_c.shape[1]
    return np.stack([np.stack([np.stack([lut_judge(hist_c[i, r, c], hist_s[j, r, c], **defect) for c in range(3)]) for r in range(R)])
                     for i, j in pairs])


# ------------------------------------------------------------------------------------------------------------ Lab both ways
def lab_forward(u8, dtype=np.float64, linear_branch=True):
    """uint8 (..., 3) numpy -> Lab (..., 3) in ``dtype`` (colour_cases.lab_of's definition, in numpy).  Defect:
    ``linear_branch=False`` takes the cube root everywhere."""
    tab, M = C.srgb_table().astype(dtype), C.lab_matrix().astype(dtype)
    xyz = tab[np.asarray(u8).astype(np.int64)] @ M.T
    cube = np.cbrt(xyz)
    f = cube if not linear_branch else np.where(xyz > dtype((6.0 / 29.0) ** 3), cube, xyz * dtype(841.0 / 108.0) + dtype(4.0 / 29.0))
    return np.stack((dtype(116.0) * f[..., 1] - dtype(16.0), dtype(500.0) * (f[..., 0] - f[..., 1]), dtype(200.0) * (f[..., 1] - f[..., 2])), -1)


def inverse_matrix():
    """the float64 inverse of the float64 (sRGB rows / white point), rounded once to fp32"""
    return np.linalg.inv(C.XYZ / C.WHITE[:, None]).astype(np.float32).astype(np.float64)


def lab_inverse(lab, dtype=np.float64, clamp=True):
    """Lab (..., 3) -> the unrounded byte values 255 s (..., 3) in ``dtype``.  Defect: ``clamp=False`` leaves linear RGB outside
    [0, 1] (the value then leaves 0 .. 255, and ``wrap_u8`` shows what a byte store makes of it)."""
    lab = lab.astype(dtype)
    fy = (lab[..., 0] + dtype(16.0)) / dtype(116.0)
    f = np.stack((fy + lab[..., 1] / dtype(500.0), fy, fy - lab[..., 2] / dtype(200.0)), -1)
    t = np.where(f > dtype(6.0 / 29.0), f * f * f, (f - dtype(4.0 / 29.0)) * dtype(108.0 / 841.0))
    c = t @ inverse_matrix().astype(dtype).T
    if clamp:
        c = np.clip(c, dtype(0.0), dtype(1.0))
    s = np.where(c <= dtype(0.0031308), dtype(12.92) * c,
                 dtype(1.055) * np.power(np.maximum(c, dtype(0.0)), dtype(1.0 / 2.4)) - dtype(0.055))
    return dtype(255.0) * s


def wrap_u8(q):
    """what an unclamped kernel stores: the low byte of rint(q)"""
    return (np.rint(q).astype(np.int64) & 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------ the apply modes
def _regions(img, labels, R, recolour_ignored):
    lab = np.zeros(img.shape[:3], dtype=np.int64) if labels is None else np.asarray(labels, dtype=np.int64)
    valid = np.ones_like(lab, dtype=bool) if recolour_ignored else lab < R
    return np.where(lab < R, lab, 0), valid


def _blend(per_region, weights, dtype, normalise):
    """sum_r w_r v_r / sum_r w_r, both sums in region order; ``per_region``: (B, R, H, W, n); -> (value, sum w > 0)"""
    w = np.asarray(weights).astype(dtype)
    num, den = np.zeros_like(per_region[:, 0]), np.zeros_like(w[:, 0])
    for r in range(w.shape[1]):
        num = num + w[:, r][..., None] * per_region[:, r]
        den = den + w[:, r]
    on = den > 0
    return (num / np.where(on, den, dtype(1.0))[..., None] if normalise else num), on


def apply_lut(img, labels, luts, weights=None, dtype=np.float64, normalise=True, recolour_ignored=False):
    """-> q (B, H, W, 3) in ``dtype``: LUT[label][c][v] (an integer), or with weights sum_r w_r LUT[r][c][v] / sum_r w_r; a pixel of
    no region: its input.  Defects: ``normalise=False``, ``recolour_ignored`` (label >= R treated as region 0)."""
    img, luts = np.asarray(img), np.asarray(luts)
    B, R = luts.shape[:2]
    li, valid = _regions(img, labels, R, recolour_ignored)
    v = img.astype(np.int64)
    b = np.arange(B).reshape(B, 1, 1, 1)
    ch = np.arange(3).reshape(1, 1, 1, 3)
    q = luts[b, li[..., None], ch, v].astype(dtype)
    if weights is not None:
        per = np.stack([luts[b, r, ch, v] for r in range(R)], 1).astype(dtype)
        mix, on = _blend(per, weights, dtype, normalise)
        q = np.where(on[..., None], mix, q)
    return np.where(valid[..., None], q, img.astype(dtype))


def apply_affine(img, labels, rows, weights=None, dtype=np.float64, normalise=True, recolour_ignored=False, linear_branch=True,
                 clamp=True):
    """-> q (B, H, W, 3) in ``dtype``: lab' = T lab + t with the row of the pixel's label (or the weights' blend of the 12
    coefficients), back through ``lab_inverse``; a pixel of no region: its input.  ``rows``: (B, R, 12), fp32 values."""
    img = np.asarray(img)
    rows = np.asarray(rows).astype(dtype)
    B, R = rows.shape[:2]
    li, valid = _regions(img, labels, R, recolour_ignored)
    k = rows[np.arange(B).reshape(B, 1, 1), li]
    if weights is not None:
        per = np.broadcast_to(rows[:, :, None, None, :], (B, R) + img.shape[1:3] + (12,))
        mix, on = _blend(per, weights, dtype, normalise)
        k = np.where(on[..., None], mix, k)
    lab = lab_forward(img, dtype, linear_branch)
    out = np.stack([k[..., 3 * i] * lab[..., 0] + (k[..., 3 * i + 1] * lab[..., 1] + (k[..., 3 * i + 2] * lab[..., 2] + k[..., 9 + i]))
                    for i in range(3)], -1)
    q = lab_inverse(out, dtype, clamp)
    return np.where(valid[..., None], q, img.astype(dtype))


# ------------------------------------------------------------------------------------------------------------ the Gaussian maps
def _sqrtm(m):
    w, v = np.linalg.eigh(m)
    return (v * np.sqrt(np.clip(w, 0.0, None))) @ v.T


def gaussian_row(mean_c, cov_c, n_c, mean_s, cov_s, n_s, method, floor=FLOOR, max_gain=MAX_GAIN):
    """one (T row-major | mu_S - T mu_C) row, float64: "mkl" T = Sc^-1/2 (Sc^1/2 Ss Sc^1/2)^1/2 Sc^-1/2 with Sc's eigenvalues
    clamped from below by ``floor`` and T's from above by ``max_gain``; "reinhard" T = diag(min(sqrt(var_S / max(var_C, floor)),
    max_gain)); the identity row where a side is empty"""
    if n_c == 0 or n_s == 0:
        return np.concatenate((np.eye(3).ravel(), np.zeros(3)))
    mc, Sc, ms, Ss = (np.asarray(v, dtype=np.float64) for v in (mean_c, cov_c, mean_s, cov_s))
    if method == "mkl":
        w, v = np.linalg.eigh(Sc)
        w = np.maximum(w, floor)
        root, iroot = (v * np.sqrt(w)) @ v.T, (v / np.sqrt(w)) @ v.T
        T = iroot @ _sqrtm(root @ Ss @ root) @ iroot
        w, v = np.linalg.eigh(0.5 * (T + T.T))
        T = (v * np.minimum(w, max_gain)) @ v.T
    else:
        T = np.diag(np.minimum(np.sqrt(np.clip(np.diag(Ss), 0.0, None) / np.maximum(np.diag(Sc), floor)), max_gain))
    return np.concatenate((T.ravel(), ms - T @ mc))


def gaussian_rows(mean_c, cov_c, count_c, mean_s, cov_s, count_s, pairs, method, **kw):
    """(K, R, 12) float64 from the judges' moments (B, R, 3), (B, R, 3, 3) and counts (B, R)"""
    R = mean_c.shape[1]
    return np.stack([np.stack([gaussian_row(mean_c[i, r], cov_c[i, r], int(count_c[i, r]), mean_s[j, r], cov_s[j, r], int(count_s[j, r]),
                                            method, **kw) for r in range(R)]) for i, j in pairs])


# ------------------------------------------------------------------------------------------------------------ a case's references
_REFS = {}


def reference(name):
    """The case with the judges' statistics of both batches (axes histograms, counts, float64 Lab moments), the maps for the pairs
    n -> n -- ``luts`` (B, R, 3, 256), ``rows_mkl`` / ``rows_reinhard`` (B, R, 12) fp32 -- and for each apply mode ``key`` in
    MODES the unrounded judges ``q64[key]`` / ``q32[key]`` and ``tau[key]``.  Computed once, shared, never written to."""
    if name in _REFS:
        return _REFS[name]
    c = make_case(name)
    R, B = c["R"], c["img"].shape[0]
    pairs = [(n, n) for n in range(B)]
    axes = np.array(C.AXES, dtype=np.int16)
    for tag in ("", "_s"):
        img, lab = c["img" + tag], c["labels" + tag]
        c["hist" + tag], c["count" + tag] = C.hist_judge(img.numpy(), None if lab is None else lab.numpy(), R, axes)
        mean, cov = C.lab_judge(img, lab, R)
        c["mean" + tag], c["cov" + tag] = mean.numpy(), cov.numpy()
    c["pairs"] = pairs
    c["luts"] = luts_judge(c["hist"], c["hist_s"], pairs)
    for m in ("mkl", "reinhard"):
        c["rows_" + m] = gaussian_rows(c["mean"], c["cov"], c["count"], c["mean_s"], c["cov_s"], c["count_s"], pairs, m).astype(np.float32)
    img = c["img"].numpy()
    lab = None if c["labels"] is None else c["labels"].numpy()
    c["q64"], c["q32"], c["tau"] = {}, {}, {}
    for key in MODES:
        c["q64"][key] = run_mode(key, img, lab, c, np.float64)
        c["q32"][key] = run_mode(key, img, lab, c, np.float32)
        c["tau"][key] = 2.0 * float(np.abs(c["q32"][key].astype(np.float64) - c["q64"][key]).max()) + 1e-3
    _REFS[name] = c
    return c


# apply modes judged by the bar: name -> (map key, weighted)
MODES = {"lut-weighted": ("luts", True), "mkl": ("rows_mkl", False), "mkl-weighted": ("rows_mkl", True),
         "reinhard": ("rows_reinhard", False), "reinhard-weighted": ("rows_reinhard", True)}


def run_mode(key, img, lab, c, dtype, **defect):
    maps, weighted = MODES[key]
    fn = apply_lut if maps == "luts" else apply_affine
    return fn(img, lab, c[maps], c["weights"] if weighted else None, dtype, **defect)


def exempt_share(q64, tau):
    d, _ = G.boundary_distance(q64)
    return float((d <= tau).mean())


# name -> (what it replaces, the modes it can show in).  "lut" defects change the TABLE: they are judged by equality.
DEFECTS = {
    "inclusive-cdf": ("lut", dict(cdf="inclusive")),
    "counts-exchanged": ("lut", dict(swap_counts=True)),
    "weights-not-normalised": ("apply", dict(normalise=False)),
    "ignored-label-recoloured": ("apply", dict(recolour_ignored=True)),
    "no-linear-branch": ("affine", dict(linear_branch=False)),
    "no-gamut-clamp": ("affine", dict(clamp=False)),
}


def to_torch(a):
    return torch.from_numpy(np.ascontiguousarray(a))
