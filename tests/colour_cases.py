"""Case table of the colour statistics (csrc/colour_stats.hip): shapes, seeded uint8 inputs and the judges -- restatements of the
definitions in include/ppst_hip.h ("colour statistics"): the histograms in numpy int64 (np.bincount), the CIELAB moments in
torch (float64 is the judge, float32 sets the bar), the exact W1 numerator in Python integers, the distances of
``metrics.colour_distance`` in float64 numpy.  Importing this needs no GPU.  test_colour_cpu.py pins the judges (a second,
loop-written form; closed forms); test_gpu_colour.py holds the kernels to them.

The bar of the Lab moments is the project's convention for fp32 streaming kernels (tests/BACKWARD_KERNELS.md section 3):
``bar = max(2e-6, 4 x |float32 torch evaluation of this judge - its float64 evaluation|)``, relative to max |ref|.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

WAVE_CHUNK = 1024          # CS_WCHUNK of csrc/colour_stats.hip: pixels one wave owns at a time; a block has four waves
AXES = ((4096, 0, 0), (0, 4096, 0), (0, 0, 4096))
LUMA = (1225, 2404, 467)
# mixed signs: t reaches 0 and 255 on the corner colours (row 0 maps red 255 -> 0, red 0 -> 255)
SIGNED_DIRS = ((-4096, 0, 0), (2048, -2048, 0), (-1365, -1365, -1365), (1000, -96, -3000), (4096, 0, 0), (-1, 0, 4095))

# name -> B, H, W, R (regions), labels ("none" | "map"), dirs ("k<n>": axes + luma + n random rows of the project's table, or
# "signed"), kind ("smooth" | "flat" | "corners"), and what else is special.  Which edge each one reaches:
CASES = {
    "1x1": dict(B=2, H=1, W=1, R=2, labels="map", dirs="k2"),                # one pixel: fewer pixels than lanes; image 0 is region 0, image 1 region 1
    "7x5": dict(B=1, H=7, W=5, R=1, labels="none", dirs="k0"),               # no label map: one region
    "33x70": dict(B=3, H=33, W=70, R=3, labels="map", dirs="k12"),           # odd batch, rows no multiple of anything, 3 wave chunks (the last ragged)
    "64x64-flat": dict(B=2, H=64, W=64, R=3, labels="map", dirs="k12", kind="flat"),   # one colour per image: every (region, projection) is one bin, the covariance exactly 0
    "257x130": dict(B=2, H=257, W=130, R=4, labels="map", dirs="k12"),       # 33 wave chunks -> 9 blocks, a ragged last one; R * P = 64: the full 64 KB of LDS
    "40x52-ignore": dict(B=2, H=40, W=52, R=3, labels="map", dirs="k12", ignore=True),   # labels hold 255; region 2 is empty in image 1 only
    "48x48-view": dict(B=2, H=48, W=48, R=3, labels="map", dirs="k4", view=(64, 80, 5, 9)),   # crop [5:53, 9:57] of 64 x 80: row stride != 3 W
    "extremes": dict(B=2, H=16, W=24, R=2, labels="map", dirs="signed", kind="corners"),     # pixels from {0, 255}^3, directions of mixed signs: t reaches 0 and 255
}


def directions(k=12, seed=0):
    """the project's direction table restated: rows 0-2 the axes, row 3 BT.601 luma, then trunc(theta / |theta|_1 * 4096)"""
    theta = torch.randn(k, 3, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).numpy()
    rand = np.trunc(theta / np.abs(theta).sum(1, keepdims=True) * 4096.0).astype(np.int16).reshape(k, 3)
    return np.concatenate((np.array(AXES + (LUMA,), dtype=np.int16), rand), 0)


def case_dirs(case):
    d = CASES[case]["dirs"]
    return np.array(SIGNED_DIRS, dtype=np.int16) if d == "signed" else directions(int(d[1:]))


def make_images(seed, B, H, W, kind="smooth"):
    """uint8 (B, H, W, 3): a smooth random field plus noise (as ssim_cases.make_pair makes them), quantised; "flat": one seeded
    colour per image; "corners": every channel 0 or 255"""
    gen = torch.Generator().manual_seed(seed)
    if kind == "flat":
        return torch.randint(0, 256, (B, 1, 1, 3), generator=gen, dtype=torch.uint8).expand(B, H, W, 3).contiguous()
    if kind == "corners":
        return (torch.randint(0, 2, (B, H, W, 3), generator=gen) * 255).to(torch.uint8)
    coarse = torch.randn(B, 3, H // 8 + 3, W // 8 + 3, generator=gen, dtype=torch.float64)
    a = 0.6 * F.interpolate(coarse, size=(H, W), mode="bicubic", align_corners=True)
    a = (a + 0.05 * torch.randn(B, 3, H, W, generator=gen, dtype=torch.float64)).clamp(-1.0, 1.0)
    return ((a + 1.0) * 127.5).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def make_labels(seed, B, H, W, R):
    """uint8 (B, H, W) in 0 .. R - 1: a coarse random map, every region present in every image where H * W >= R"""
    gen = torch.Generator().manual_seed(seed)
    coarse = torch.randint(0, R, (B, H // 8 + 1, W // 8 + 1), generator=gen)
    lab = coarse.repeat_interleave(8, 1).repeat_interleave(8, 2)[:, :H, :W].contiguous()
    flat = lab.view(B, -1)
    for r in range(min(R, H * W)):                 # pixel r of every image is region r
        flat[:, r] = r
    return lab.to(torch.uint8)


def make_case(name):
    """-> dict(img, labels (or None), R, dirs (numpy int16), and for the view case ``big_img`` / ``big_labels`` / ``window``).
    Seeded by the case's place in the table."""
    c = CASES[name]
    seed = 500 + list(CASES).index(name)
    B, H, W, R = c["B"], c["H"], c["W"], c["R"]
    out = dict(R=R, dirs=case_dirs(name))
    if "view" in c:
        BH, BW, y0, x0 = c["view"]
        out["big_img"], out["big_labels"] = make_images(seed, B, BH, BW), make_labels(seed + 50, B, BH, BW, R)
        out["window"] = (slice(y0, y0 + H), slice(x0, x0 + W))
        out["img"] = out["big_img"][:, y0:y0 + H, x0:x0 + W].contiguous()
        out["labels"] = out["big_labels"][:, y0:y0 + H, x0:x0 + W].contiguous()
        return out
    out["img"] = make_images(seed, B, H, W, c.get("kind", "smooth"))
    lab = make_labels(seed + 50, B, H, W, R) if c["labels"] == "map" else None
    if name == "1x1":
        lab = torch.tensor([0, 1], dtype=torch.uint8).view(2, 1, 1)
    if c.get("ignore"):
        gen = torch.Generator().manual_seed(seed + 99)
        lab[torch.rand(lab.shape, generator=gen) < 0.1] = 255
        lab[1][lab[1] == 2] = 255                  # region 2: empty in image 1 only
        assert int((lab[0] == 2).sum()) > 0 and int((lab[1] == 2).sum()) == 0 and int((lab[1] == 1).sum()) > 0
    out["labels"] = lab
    return out


# ------------------------------------------------------------------------------------------------------------ the judges
def projection_offsets(dirs):
    d = np.asarray(dirs, dtype=np.int64)
    return 255 * np.where(d < 0, -d, 0).sum(1)


def project(img, dirs):
    """t = (d . rgb + 255 sum_{d_c < 0} |d_c|) >> 12 for every pixel and row: int64 (..., P)"""
    d = np.asarray(dirs, dtype=np.int64)
    return (np.asarray(img, dtype=np.int64) @ d.T + projection_offsets(d)) >> 12


def hist_judge(img, labels, R, dirs):
    """-> (hist (B, R, P, 256), count (B, R)) int64 by np.bincount over the combined (region, projection, bin) index"""
    img = np.asarray(img)
    B, H, W, _ = img.shape
    P = len(dirs)
    lab = np.zeros((B, H, W), dtype=np.int64) if labels is None else np.asarray(labels, dtype=np.int64)
    t = project(img, dirs)                                                   # (B, H, W, P)
    assert t.min() >= 0 and t.max() <= 255
    hist, count = np.zeros((B, R, P, 256), dtype=np.int64), np.zeros((B, R), dtype=np.int64)
    for b in range(B):
        ok = lab[b] < R
        idx = (lab[b][ok][:, None] * P + np.arange(P)[None, :]) * 256 + t[b][ok]
        hist[b] = np.bincount(idx.ravel(), minlength=R * P * 256).reshape(R, P, 256)
        count[b] = np.bincount(lab[b][ok], minlength=R)
    return hist, count


def srgb_table():
    """256 entries, float64 arithmetic, rounded once to fp32 (returned as float64 values of those fp32 numbers)"""
    c = np.arange(256, dtype=np.float64) / 255.0
    lin = np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)
    return lin.astype(np.float32).astype(np.float64)


XYZ = np.array([[0.4124564, 0.3575761, 0.1804375], [0.2126729, 0.7151522, 0.0721750], [0.0193339, 0.1191920, 0.9503041]])
WHITE = np.array([0.95047, 1.0, 1.08883])


def lab_matrix():
    """the sRGB -> XYZ rows over the D65 white, float64 arithmetic, rounded once to fp32"""
    return (XYZ / WHITE[:, None]).astype(np.float32).astype(np.float64)


def lab_of(img, dtype=torch.float64):
    """uint8 (..., 3) tensor -> (L*, a*, b*) (..., 3) in ``dtype``"""
    tab = torch.from_numpy(srgb_table()).to(dtype)
    M = torch.from_numpy(lab_matrix()).to(dtype)
    lin = tab[img.long()]
    xyz = lin @ M.T
    f = torch.where(xyz > (6.0 / 29.0) ** 3, xyz.clamp(min=1e-30) ** (1.0 / 3.0), xyz * (841.0 / 108.0) + 4.0 / 29.0)
    return torch.stack((116.0 * f[..., 1] - 16.0, 500.0 * (f[..., 0] - f[..., 1]), 200.0 * (f[..., 1] - f[..., 2])), -1)


def lab_judge(img, labels, R, dtype=torch.float64):
    """-> (mean (B, R, 3), cov (B, R, 3, 3)) in ``dtype``: the mean and the population covariance (centred form) of the Lab
    values of each region's pixels; zeros for an empty region"""
    B = img.shape[0]
    lab = lab_of(img, dtype)
    mean, cov = torch.zeros(B, R, 3, dtype=dtype), torch.zeros(B, R, 3, 3, dtype=dtype)
    for b in range(B):
        for r in range(R):
            sel = lab[b].reshape(-1, 3) if labels is None else lab[b][labels[b] == r]
            if sel.shape[0]:
                m = sel.mean(0)
                mean[b, r] = m + (sel - m).mean(0)          # one correction step: the mean of equal values is that value, exactly
                d = sel - mean[b, r]
                cov[b, r] = d.T @ d / sel.shape[0]
    return mean, cov


def w1_numerator(ha, hb):
    """sum_v |cumA(v) nB - cumB(v) nA| in Python integers"""
    ha, hb = [int(v) for v in ha], [int(v) for v in hb]
    na, nb, ca, cb, s = sum(ha), sum(hb), 0, 0, 0
    for va, vb in zip(ha, hb):
        ca, cb = ca + va, cb + vb
        s += abs(ca * nb - cb * na)
    return s


def w1_sorted(xa, xb):
    """W1 of two 1-D samples by the quantile definition, float64: the integral of |F_a^-1 - F_b^-1| over (0, 1), on the merged
    grid of both samples' quantile steps"""
    xa, xb = np.sort(np.asarray(xa, dtype=np.float64)), np.sort(np.asarray(xb, dtype=np.float64))
    na, nb = len(xa), len(xb)
    qs = np.unique(np.concatenate((np.arange(1, na + 1) / na, np.arange(1, nb + 1) / nb)))
    total, prev = 0.0, 0.0
    for q in qs:
        mid = 0.5 * (prev + q)
        total += abs(xa[min(int(mid * na), na - 1)] - xb[min(int(mid * nb), nb - 1)]) * (q - prev)
        prev = q
    return total


def frechet(mean_a, cov_a, mean_b, cov_b):
    """|dmu|^2 + tr(Sa) + tr(Sb) - 2 sum sqrt(eig(Sa Sb)) -- the eigenvalues of Sa Sb are those of Sa^1/2 Sb Sa^1/2 -- float64
    numpy, one pair"""
    ma, mb, Sa, Sb = (np.asarray(v, dtype=np.float64) for v in (mean_a, mean_b, cov_a, cov_b))
    ev = np.linalg.eigvals(Sa @ Sb).real.clip(min=0.0)
    return float(((ma - mb) ** 2).sum() + np.trace(Sa) + np.trace(Sb) - 2.0 * np.sqrt(ev).sum())


def distance_judge(hist_a, count_a, mean_a, cov_a, hist_b, count_b, mean_b, cov_b, dirs, pairs):
    """``metrics.colour_distance`` restated on the judges' own statistics: {name: float64 numpy (K, R)}, NaN where a region is
    empty on either side"""
    d = np.asarray(dirs, dtype=np.float64)
    K, R, P = len(pairs), hist_a.shape[1], len(d)
    out = {k: np.full((K, R), np.nan) for k in ("w1_rgb", "w1_luma", "swd", "delta_e", "frechet")}
    for k, (i, j) in enumerate(pairs):
        for r in range(R):
            na, nb = int(count_a[i, r]), int(count_b[j, r])
            if na == 0 or nb == 0:
                continue
            w1 = np.array([w1_numerator(hist_a[i, r, p], hist_b[j, r, p]) / (na * nb) for p in range(P)])
            out["w1_rgb"][k, r] = w1[:3].mean()
            if P >= 4:
                out["w1_luma"][k, r] = w1[3]
            if P > 4:
                out["swd"][k, r] = (w1[4:] * 4096.0 / np.sqrt((d[4:] ** 2).sum(1))).mean()
            ma, mb = np.asarray(mean_a[i, r], dtype=np.float64), np.asarray(mean_b[j, r], dtype=np.float64)
            out["delta_e"][k, r] = math.sqrt(((ma - mb) ** 2).sum())
            out["frechet"][k, r] = frechet(ma, cov_a[i, r], mb, cov_b[j, r])
    return out


# ------------------------------------------------------------------------------------------------------------ the bars
def moment_bar(ref64, val32):
    """max(2e-6, 4 x |float32 evaluation - float64 evaluation|), relative to max |ref| (0 / 0 counts as 0: a reference that is
    exactly zero -- a flat image's covariance -- has to be met exactly)"""
    return max(2e-6, 4.0 * relative_error(ref64, val32))


def relative_error(ref64, got):
    err = (got.double().cpu() - ref64).abs().max().item()
    scale = ref64.abs().max().item()
    if err == 0.0:
        return 0.0
    return err / scale if scale > 0.0 else math.inf


def distance_bars(mean_bar, mean_scale, cov_bar, cov_scale, delta_e, frechet_value):
    """The bars of ``delta_e`` and ``frechet`` for one (pair, region), propagated from the moments' bars.
    Each mean component may be off by em = mean_bar * mean_scale on either side, each covariance entry by ec = cov_bar * cov_scale.
      delta_e = |dmu|_2: the difference vector moves by at most e = 2 sqrt(3) em (two sides, three components), and so does its norm.
      frechet = |dmu|^2 + dB^2 with dB the Bures distance between the covariances.  |dmu|^2 moves by at most 2 |dmu| e + e^2.
      dB is a metric with dB(S, S')^2 <= |S^1/2 - S'^1/2|_F^2 <= |S - S'|_1 (Powers-Stormer), and the trace norm of a symmetric
      3 x 3 perturbation with entries <= ec is at most sqrt(3) |.|_F <= 3 sqrt(3) ec; so each side moves dB by at most
      h = sqrt(3 sqrt(3) ec), and dB^2 by at most 2 dB (2 h) + (2 h)^2 (triangle inequality), with dB^2 = frechet - |dmu|^2.
    Plus 1e-9 for the float64 eigen-decompositions on both sides."""
    em, ec = mean_bar * mean_scale, cov_bar * cov_scale
    e = 2.0 * math.sqrt(3.0) * em
    h = 2.0 * math.sqrt(3.0 * math.sqrt(3.0) * ec)
    dB = math.sqrt(max(frechet_value - delta_e ** 2, 0.0))
    return e + 1e-9, 2.0 * delta_e * e + e * e + 2.0 * dB * h + h * h + 1e-9
