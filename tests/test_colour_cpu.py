"""CPU: the judges of the colour statistics (tests/colour_cases.py) pinned by a second, loop-written form and by closed forms, so
that they are not their own witnesses; and what of ppst_amd/metrics.py, evaluation.style_fidelity, training.HeldOutEvaluator and
the ppst_colour_stats / ppst_hist_w1 entry points (include/ppst_hip.h "colour statistics") can be checked without a GPU.
Nothing here launches a kernel."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import colour_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _loop_stats(img, labels, R, dirs):
    """per pixel, plain Python: the histogram bin by integer arithmetic with floor division, the Lab value from the formulas with
    math.pow on the float64 definitions (no table, no matrix product), two-pass moments"""
    B, H, W, _ = img.shape
    P = len(dirs)
    hist = np.zeros((B, R, P, 256), dtype=np.int64)
    labs = [[[] for _ in range(R)] for _ in range(B)]
    tab, M = C.srgb_table(), C.lab_matrix()
    f = lambda t: t ** (1.0 / 3.0) if t > 216.0 / 24389.0 else t * 841.0 / 108.0 + 4.0 / 29.0
    for b in range(B):
        for y in range(H):
            for x in range(W):
                r = 0 if labels is None else int(labels[b, y, x])
                if r >= R:
                    continue
                rgb = [int(v) for v in img[b, y, x]]
                for p, d in enumerate(dirs):
                    d = [int(v) for v in d]
                    t = (sum(dc * c for dc, c in zip(d, rgb)) + 255 * sum(-dc for dc in d if dc < 0)) // 4096
                    hist[b, r, p, t] += 1
                lin = [float(tab[c]) for c in rgb]
                fx, fy, fz = (f(sum(float(M[i][k]) * lin[k] for k in range(3))) for i in range(3))
                labs[b][r].append((116.0 * fy - 16.0, 500.0 * (fx - fy), 200.0 * (fy - fz)))
    mean, cov = np.zeros((B, R, 3)), np.zeros((B, R, 3, 3))
    for b in range(B):
        for r in range(R):
            v = labs[b][r]
            if not v:
                continue
            n = len(v)
            mu = [math.fsum(q[i] for q in v) / n for i in range(3)]
            mean[b, r] = mu
            for i in range(3):
                for k in range(3):
                    cov[b, r, i, k] = math.fsum((q[i] - mu[i]) * (q[k] - mu[k]) for q in v) / n
    return hist, mean, cov


@pytest.mark.parametrize("name", ["7x5", "extremes"])
def test_judges_against_the_loop_form(name):
    c = C.make_case(name)
    img, lab = c["img"], c["labels"]
    hist, count = C.hist_judge(img.numpy(), None if lab is None else lab.numpy(), c["R"], c["dirs"])
    mean, cov = C.lab_judge(img, lab, c["R"])
    h2, m2, c2 = _loop_stats(img.numpy(), None if lab is None else lab.numpy(), c["R"], c["dirs"])
    assert np.array_equal(hist, h2) and np.array_equal(count, h2[:, :, 0].sum(-1))
    assert hist.sum() == img.shape[0] * img.shape[1] * img.shape[2] * len(c["dirs"])
    em, ec = np.abs(mean.numpy() - m2).max(), np.abs(cov.numpy() - c2).max()
    print("\n%s: loop form vs vector form: mean err %.3g, cov err %.3g (max |cov| %.3g)" % (name, em, ec, np.abs(c2).max()))
    assert em <= 1e-11 and ec <= 1e-9
    if name == "extremes":                                      # t reaches both ends along the signed rows
        t = C.project(img.numpy(), c["dirs"])
        assert t.min() == 0 and t.max() == 255 and hist[:, :, 0, 0].sum() > 0 and hist[:, :, 0, 255].sum() > 0


def test_lab_landmarks():
    """white is (100, 0, 0) and black (0, 0, 0) to the rounding of the fp32 constants; sRGB red is the textbook (53.24, 80.09,
    67.20); the linear branch of f is used below (6/29)^3 and the two branches meet there"""
    px = torch.tensor([[255, 255, 255], [0, 0, 0], [255, 0, 0], [1, 1, 1], [128, 128, 128]], dtype=torch.uint8)
    lab = C.lab_of(px)
    assert (lab[0] - torch.tensor([100.0, 0.0, 0.0], dtype=torch.float64)).abs().max() <= 1e-4
    assert lab[1].abs().max() <= 1e-12
    assert (lab[2] - torch.tensor([53.2408, 80.0925, 67.2032], dtype=torch.float64)).abs().max() <= 2e-3
    assert abs(lab[3, 0].item() - 903.3 * C.srgb_table()[1]) <= 1e-3 and lab[3, 1:].abs().max() <= 1e-5   # L = kappa Y
    assert abs(lab[4, 0].item() - 53.585) <= 1e-2 and lab[4, 1:].abs().max() <= 1e-4                       # greys have a = b = 0
    d = 6.0 / 29.0
    assert abs(d ** 3 * 841.0 / 108.0 + 4.0 / 29.0 - d) <= 1e-15


def test_colour_directions():
    from ppst_amd import metrics
    d = metrics.colour_directions()
    assert d.dtype == torch.int16 and tuple(d.shape) == (16, 3) and not d.is_cuda
    assert d[:4].tolist() == [[4096, 0, 0], [0, 4096, 0], [0, 0, 4096], [1225, 2404, 467]]
    assert metrics.colour_directions(12, 0) is d                                     # cached per (k, seed)
    assert np.array_equal(d.numpy(), C.directions(12, 0))                            # the stated recipe
    assert tuple(metrics.colour_directions(0).shape) == (4, 3)
    other = metrics.colour_directions(12, 1)
    assert torch.equal(other[:4], d[:4]) and not torch.equal(other[4:], d[4:])
    assert torch.equal(metrics.colour_directions(5, 3), torch.from_numpy(C.directions(5, 3)))
    corners = np.array([[r, g, b] for r in (0, 255) for g in (0, 255) for b in (0, 255)])
    for table in (d, other, metrics.colour_directions(5, 3), torch.tensor(C.SIGNED_DIRS, dtype=torch.int16)):
        assert int(table.to(torch.int32).abs().sum(1).max()) <= 4096
        t = C.project(corners, table.numpy())
        assert t.min() >= 0 and t.max() <= 255
    assert int(d[4:].to(torch.int32).abs().sum(1).min()) >= 4094                    # truncation loses less than 1 per channel
    assert C.project(corners, d.numpy())[:, 0].tolist() == corners[:, 0].tolist()   # (4096, 0, 0): the red channel itself
    with pytest.raises(ValueError):
        metrics.colour_directions(13)


def test_w1_numerator_closed_forms():
    rng = np.random.default_rng(5)
    h = rng.integers(0, 50, 256)
    assert C.w1_numerator(h, h) == 0
    assert C.w1_numerator(h, 3 * h) == 0                                             # the same distribution at another count
    for v1, v2, na, nb in ((3, 200, 7, 7), (255, 0, 5, 11), (17, 17, 1, 9)):
        a, b = np.zeros(256, dtype=np.int64), np.zeros(256, dtype=np.int64)
        a[v1], b[v2] = na, nb
        assert C.w1_numerator(a, b) == abs(v1 - v2) * na * nb
    # unequal counts: the quantile definition on the samples themselves
    for na, nb in ((40, 40), (37, 101), (1, 64)):
        xa, xb = rng.integers(0, 256, na), rng.integers(0, 256, nb)
        ref = C.w1_sorted(xa, xb)
        got = C.w1_numerator(np.bincount(xa, minlength=256), np.bincount(xb, minlength=256)) / (na * nb)
        assert abs(ref - got) <= 1e-10 * max(ref, 1.0), (na, nb, ref, got)
    full = np.zeros(256, dtype=np.int64)
    full[0] = 1 << 22
    other = np.zeros(256, dtype=np.int64)
    other[255] = 1 << 22
    assert C.w1_numerator(full, other) == 255 << 44 < 1 << 52                       # the largest numerator there is


def test_frechet_closed_forms():
    from ppst_amd import metrics
    rng = np.random.default_rng(9)
    A = rng.normal(size=(3, 3))
    S = A @ A.T + 0.1 * np.eye(3)
    mu = rng.normal(size=3)
    both = lambda ma, Sa, mb, Sb: (C.frechet(ma, Sa, mb, Sb),
                                   float(metrics.gaussian_w2_squared(*(torch.from_numpy(np.asarray(v, dtype=np.float64)) for v in (ma, Sa, mb, Sb)))))
    for got in both(mu, S, mu, S):                                                    # equal Gaussians
        assert abs(got) <= 1e-12
    sa, sb, dm = np.array([1.0, 4.0, 0.25]), np.array([2.25, 0.0, 9.0]), np.array([0.5, -2.0, 1.0])
    exact = ((np.sqrt(sa) - np.sqrt(sb)) ** 2).sum() + (dm ** 2).sum()               # diagonal covariances, one of them singular
    for got in both(mu, np.diag(sa), mu + dm, np.diag(sb)):
        assert abs(got - exact) <= 1e-12
    B = rng.normal(size=(3, 3))
    T = B @ B.T
    a, b = both(mu, S, mu + dm, T)                                                    # the judge's form and the module's agree
    assert abs(a - b) <= 1e-10 and a > (dm ** 2).sum()
    assert abs(both(mu, S, mu + dm, T)[0] - both(mu + dm, T, mu, S)[0]) <= 1e-10      # symmetric
    # batched, as colour_distance calls it
    covs = torch.from_numpy(np.stack([S, T]))
    got = metrics.gaussian_w2_squared(torch.zeros(2, 2, 3), covs[:, None].expand(2, 2, 3, 3), torch.zeros(2, 2, 3), covs[None].expand(2, 2, 3, 3))
    assert tuple(got.shape) == (2, 2) and abs(got[0, 0]) <= 1e-12 and abs(got[1, 1]) <= 1e-12 and abs(got[0, 1] - got[1, 0]) <= 1e-10


def test_distance_bars_are_the_stated_propagation():
    e, f = C.distance_bars(2e-6, 80.0, 2e-6, 400.0, 10.0, 125.0)
    em, ec = 2e-6 * 80.0, 2e-6 * 400.0
    ee, h = 2 * math.sqrt(3) * em, 2 * math.sqrt(3 * math.sqrt(3) * ec)
    assert abs(e - ee - 1e-9) <= 1e-15 and abs(f - (20.0 * ee + ee * ee + 2 * 5.0 * h + h * h + 1e-9)) <= 1e-12


def test_argument_errors_need_no_gpu():
    from ppst_amd._lib import lib
    tok = ctypes.c_void_p(16)          # a non-null token: validation runs before anything is dereferenced or launched
    dirs = (ctypes.c_int16 * 6)(4096, 0, 0, -2000, 96, 2000)
    bad_dirs = (ctypes.c_int16 * 6)(4096, 0, 0, -2000, 97, 2000)

    def cs(img=tok, sx=3, labels=tok, B=1, H=8, W=8, R=3, d=dirs, P=2, hist=tok, count=tok, mean=tok, cov=tok, ws=tok):
        return lib.ppst_colour_stats(img, 8 * 8 * 3, 8 * 3, sx, labels, 64, 8, B, H, W, R, d, P, hist, count, mean, cov, ws, None)

    for kw in (dict(R=0), dict(R=5), dict(P=0), dict(P=17), dict(H=2049, W=2048), dict(H=1 << 22, W=2), dict(sx=4), dict(sx=1),
               dict(B=-1), dict(H=0), dict(W=0)):
        assert cs(**kw) == -1, kw
    assert cs(B=0, img=None, labels=None, d=None, hist=None, count=None, mean=None, cov=None, ws=None) == 0      # empty batch
    assert cs(R=5, img=None, d=None, hist=None) == -1                                # sizes are judged ahead of the pointers
    for hole in ("img", "d", "hist", "count", "mean", "cov", "ws"):
        assert cs(**{hole: None}) == -3, hole
    assert cs(d=bad_dirs) == -1                                                      # sum |d| = 4097 in row 1
    assert lib.ppst_colour_stats_ws(1, 2048, 2048) > 0 and lib.ppst_colour_stats_ws(0, 8, 8) >= 0
    assert lib.ppst_colour_stats_ws(1, 2049, 2048) == -1 and lib.ppst_colour_stats_ws(-1, 8, 8) == -1
    assert lib.ppst_colour_stats_ws(1, 0, 8) == -1
    assert lib.ppst_colour_stats_ws(2, 64, 64) - lib.ppst_colour_stats_ws(1, 64, 64) == 4 * 4 * 16 * 4      # 4 wave chunks x 4 regions x 64 bytes

    w1 = lambda a=tok, Ba=1, b=tok, Bb=1, pairs=tok, K=1, R=3, P=2, num=tok: lib.ppst_hist_w1(a, Ba, b, Bb, pairs, K, R, P, num, None)
    for kw in (dict(R=0), dict(R=5), dict(P=0), dict(P=17), dict(K=-1), dict(Ba=-1), dict(Bb=-1)):
        assert w1(**kw) == -1, kw
    assert w1(a=None, b=None, pairs=None, num=None, K=0) == 0
    for hole in ("a", "b", "pairs", "num"):
        assert w1(**{hole: None}) == -3, hole
    assert lib.ppst_version() == 3                                                   # functions were added; no struct changed


def test_header_binding_and_library_agree():
    from ppst_amd import _lib
    text = open(os.path.join(ROOT, "include", "ppst_hip.h")).read()
    assert "colour statistics ---- */" in text
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, nargs in (("ppst_colour_stats_ws", 3), ("ppst_colour_stats", 19), ("ppst_hist_w1", 10)):
        m = re.search(r"\b(?:int|int64_t)\s+%s\s*\(([^)]*)\)" % name, text)
        assert m and len(m.group(1).split(",")) == nargs, name
        restype, argtypes = _lib._SIGS[name]
        assert len(argtypes) == nargs and hasattr(_lib.lib, name)
        assert restype is (ctypes.c_int64 if name.endswith("_ws") else ctypes.c_int)
    from ppst_amd import build
    assert "colour_stats.hip" in build.SOURCES


def test_ops_and_metrics_refuse_cpu_tensors():
    from ppst_amd import evaluation, metrics, ops
    u = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    h = torch.zeros(1, 1, 3, 256, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.colour_stats(u)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.hist_w1(h, h, [(0, 0)])
    with pytest.raises(RuntimeError, match="CUDA"):
        metrics.colour_stats(u)
    with pytest.raises(RuntimeError, match="CUDA"):
        metrics.colour_stats(torch.zeros(1, 3, 8, 8))
    with pytest.raises(RuntimeError, match="CUDA"):
        evaluation.style_fidelity(u, u)


def test_signatures_and_the_one_image_refusal():
    from ppst_amd import evaluation
    from ppst_amd.training import HeldOutEvaluator
    sig = inspect.signature(HeldOutEvaluator.__init__)
    assert list(sig.parameters) == ["self", "images", "log_path", "batch", "swaps", "labels"]
    assert [sig.parameters[k].default for k in ("log_path", "batch", "swaps", "labels")] == [None, 8, False, None]
    sig = inspect.signature(evaluation.style_fidelity)
    assert list(sig.parameters) == ["styles", "outputs", "style_labels", "content_labels", "regions"]
    assert [sig.parameters[k].default for k in ("style_labels", "content_labels", "regions")] == [None, None, 3]
    from ppst_amd import metrics, ops
    assert list(inspect.signature(metrics.colour_stats).parameters) == ["images", "labels", "regions", "dirs"]
    assert list(inspect.signature(metrics.colour_distance).parameters) == ["stats_a", "stats_b", "pairs"]
    assert list(inspect.signature(ops.colour_stats).parameters) == ["u8", "labels", "regions", "dirs"]
    assert list(inspect.signature(ops.hist_w1).parameters) == ["hist_a", "hist_b", "pairs"]
    x = torch.zeros(1, 3, 16, 16)
    with pytest.raises(ValueError, match="two images"):
        HeldOutEvaluator(x, swaps=True)
    ev = HeldOutEvaluator(x)                                    # one image without swaps: as before
    assert ev.swaps is False and ev.labels is None and ev.batch == 8
    with pytest.raises(ValueError, match="both sides"):
        evaluation.style_fidelity(x, x, style_labels=torch.zeros(1, 16, 16))


def test_case_table_reaches_the_stated_edges():
    assert list(C.CASES) == ["1x1", "7x5", "33x70", "64x64-flat", "257x130", "40x52-ignore", "48x48-view", "extremes"]
    c = C.make_case("64x64-flat")
    assert all(len(np.unique(c["img"][b].reshape(-1, 3).numpy(), axis=0)) == 1 for b in range(2))
    c = C.make_case("257x130")
    assert c["R"] * len(c["dirs"]) == 64 and -(-257 * 130 // C.WAVE_CHUNK) == 33
    c = C.make_case("40x52-ignore")
    assert int((c["labels"] == 255).sum()) > 0
    c = C.make_case("48x48-view")
    y, x = c["window"]
    v = c["big_img"][:, y, x]
    assert tuple(v.shape) == (2, 48, 48, 3) and v.stride(1) == 80 * 3 and torch.equal(v, c["img"])
    c = C.make_case("extremes")
    assert set(np.unique(c["img"].numpy()).tolist()) == {0, 255}
