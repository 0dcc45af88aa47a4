"""CPU: the judges of the colour-transfer baselines (tests/transfer_cases.py) pinned against second forms and closed forms, the
cases shown to SEE each seeded defect through the bar the device is held to, and every refusal of the ppst_hist_match_lut /
ppst_colour_transfer_apply entry points and of the ops (include/ppst_hip.h "colour transfer") checked without a GPU.
"""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import colour_cases as C
import gf_cases as G
import transfer_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _histogram_pairs():
    """(content, style) histograms: random, Gaussian, flat, two-level, and of very different counts"""
    rng = np.random.default_rng(11)
    lv = np.arange(256)
    gauss = lambda mu, s, n: np.bincount(np.clip(np.rint(rng.normal(mu, s, n)), 0, 255).astype(int), minlength=256)
    flat = lambda v, n: np.bincount([v], minlength=256) * n
    two = lambda a, b, na, nb: flat(a, na) + flat(b, nb)
    out = [(rng.integers(0, 50, 256), rng.integers(0, 50, 256)), (gauss(90, 20, 5000), gauss(160, 35, 777)),
           (flat(17, 4096), gauss(120, 30, 3000)), (gauss(120, 30, 3000), flat(200, 9)), (two(0, 255, 10, 30), two(40, 41, 7, 7)),
           (flat(0, 1), flat(255, 1 << 22)), (np.full(256, 1 << 14), gauss(30, 60, 1 << 22)), (rng.integers(0, 3, 256), rng.integers(0, 3, 256) * (lv % 7 == 0))]
    return [(np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)) for a, b in out]


def test_lut_judge_against_the_loop_form():
    for hc, hs in _histogram_pairs():
        assert np.array_equal(T.lut_judge(hc, hs), T.lut_loop(hc, hs))
    c = T.reference("40x52-ignore")
    for r in range(c["R"]):
        assert np.array_equal(T.lut_judge(c["hist"][1, r, 0], c["hist_s"][1, r, 0]), T.lut_loop(c["hist"][1, r, 0], c["hist_s"][1, r, 0]))


def test_lut_properties():
    """monotone; a histogram matched to itself maps every level it contains to itself; an empty side gives the identity; a flat
    content goes to the style's median"""
    ident = np.arange(256, dtype=np.uint8)
    for hc, hs in _histogram_pairs():
        lut = T.lut_judge(hc, hs)
        assert lut.dtype == np.uint8 and (np.diff(lut.astype(int)) >= 0).all()
        own = T.lut_judge(hc, hc)
        assert np.array_equal(own[hc > 0], ident[hc > 0])
        assert np.array_equal(T.lut_judge(hc * 0, hs), ident) and np.array_equal(T.lut_judge(hc, hs * 0), ident)
    style = np.bincount([10, 20, 30, 40, 50], minlength=256)
    assert T.lut_judge(np.bincount([99], minlength=256) * 8, style)[99] == 30
    assert T.lut_judge(np.bincount([99], minlength=256) * 8, style, cdf="inclusive")[99] == 50       # the defect: the maximum
    # every product stays below 2^46 at the largest counts the statistics allow
    big = np.bincount([255], minlength=256) * (1 << 22)
    assert int((2 * np.cumsum(big) * (1 << 22)).max()) < 1 << 46 and T.lut_judge(big, big)[255] == 255


def _lab_pixels(seed, n, spread):
    rng = np.random.default_rng(seed)
    base = rng.integers(40, 216, 3)
    return np.clip(base + rng.normal(0, spread, (n, 3)), 0, 255).astype(np.uint8).reshape(1, n, 1, 3)


def test_gaussian_maps_reproduce_the_style_moments():
    """"mkl" in float64, before quantisation, carries the content's Lab mean and covariance onto the style's to 1e-9 (relative to
    the largest entry) where neither floor nor cap is active; "reinhard" the mean and the three variances"""
    a, b = _lab_pixels(1, 4000, 25.0), _lab_pixels(2, 3000, 18.0)
    la, lb = T.lab_forward(a).reshape(-1, 3), T.lab_forward(b).reshape(-1, 3)
    mom = lambda x: (x.mean(0), (x - x.mean(0)).T @ (x - x.mean(0)) / len(x))
    (ma, Sa), (mb, Sb) = mom(la), mom(lb)
    assert np.linalg.eigvalsh(Sa).min() > 100 * T.FLOOR
    for method in ("mkl", "reinhard"):
        row = T.gaussian_row(ma, Sa, len(la), mb, Sb, len(lb), method)
        Tm, off = row[:9].reshape(3, 3), row[9:]
        assert np.linalg.eigvalsh(0.5 * (Tm + Tm.T)).max() < T.MAX_GAIN
        m2, S2 = mom(la @ Tm.T + off)
        assert np.abs(m2 - mb).max() <= 1e-9 * np.abs(mb).max()
        if method == "mkl":
            assert np.allclose(Tm, Tm.T, rtol=0, atol=1e-12) and np.abs(S2 - Sb).max() <= 1e-9 * np.abs(Sb).max()
        else:
            assert np.count_nonzero(Tm - np.diag(np.diag(Tm))) == 0 and np.abs(np.diag(S2) - np.diag(Sb)).max() <= 1e-9 * np.abs(Sb).max()
    # the clamps: a flat content region is amplified by at most max_gain, an empty side gives the identity row
    row = T.gaussian_row(ma, np.zeros((3, 3)), 5, mb, Sb, 9, "mkl")
    assert np.linalg.eigvalsh(row[:9].reshape(3, 3)).max() <= T.MAX_GAIN + 1e-12
    row = T.gaussian_row(ma, np.zeros((3, 3)), 5, mb, Sb, 9, "reinhard")
    assert row[:9].max() <= T.MAX_GAIN
    ident = np.concatenate((np.eye(3).ravel(), np.zeros(3)))
    assert np.array_equal(T.gaussian_row(ma, Sa, 0, mb, Sb, 9, "mkl"), ident) and np.array_equal(T.gaussian_row(ma, Sa, 5, mb, Sb, 0, "reinhard"), ident)


def test_the_project_rows_are_the_judges():
    """``metrics.gaussian_transfer_rows`` (torch, batched) against ``transfer_cases.gaussian_rows`` (numpy, one row at a time) on
    the judges' own moments: two float64 eigen-decompositions each, 1e-9 relative to the largest entry"""
    from ppst_amd import metrics
    for name in ("33x70", "40x52-ignore", "64x64-flat"):
        c = T.reference(name)
        t = lambda k: torch.from_numpy(c[k])
        for method in ("mkl", "reinhard"):
            got = metrics.gaussian_transfer_rows(t("mean"), t("cov"), t("count"), t("mean_s"), t("cov_s"), t("count_s"), method).numpy()
            want = T.gaussian_rows(c["mean"], c["cov"], c["count"], c["mean_s"], c["cov_s"], c["count_s"], c["pairs"], method)
            assert got.shape == want.shape and np.abs(got - want).max() <= 1e-9 * np.abs(want).max(), (name, method)
    with pytest.raises(ValueError, match="method"):
        metrics.gaussian_transfer_rows(t("mean"), t("cov"), t("count"), t("mean_s"), t("cov_s"), t("count_s"), "idt")


def test_lab_round_trip_is_exact():
    """Lab -> sRGB o sRGB -> Lab through the identity row returns a seeded 2^16 sample of byte triples and the eight cube corners
    exactly, in the float64 judge and in the float32 one"""
    rng = np.random.default_rng(5)
    corners = np.array([[r, g, b] for r in (0, 255) for g in (0, 255) for b in (0, 255)])
    img = np.concatenate((rng.integers(0, 256, (1 << 16, 3)), corners)).astype(np.uint8).reshape(1, -1, 1, 3)
    ident = np.concatenate((np.eye(3).ravel(), np.zeros(3))).reshape(1, 1, 12)
    for dtype in (np.float64, np.float32):
        q = T.apply_affine(img, None, ident, dtype=dtype)
        assert np.array_equal(G.round_u8(q), img)
        assert np.abs(q - img).max() < (1e-3 if dtype is np.float64 else 2e-2)


@pytest.mark.parametrize("name", T.NAMES)
def test_float32_judge_meets_the_bar(name):
    c = T.reference(name)
    for key in T.MODES:
        q64, q32, tau = c["q64"][key], c["q32"][key], c["tau"][key]
        assert q64.shape == tuple(c["img"].shape) and q64.dtype == np.float64 and q32.dtype == np.float32
        assert G.judge(q64, G.round_u8(q32), tau) == [], (name, key)
        assert T.exempt_share(q64, tau) <= T.EXEMPT_CAP, (name, key, tau)
    # the hard-label table look-up is an integer: no bar
    hard = T.apply_lut(c["img"].numpy(), None if c["labels"] is None else c["labels"].numpy(), c["luts"])
    assert np.array_equal(hard, np.rint(hard)) and hard.min() >= 0 and hard.max() <= 255


@pytest.mark.parametrize("defect", list(T.DEFECTS))
def test_each_seeded_defect_is_seen(defect):
    kind, kw = T.DEFECTS[defect]
    seen = []
    for name in T.NAMES:
        c = T.reference(name)
        if kind == "lut":                                       # the tables are held to equality
            if not np.array_equal(T.luts_judge(c["hist"], c["hist_s"], c["pairs"], **kw), c["luts"]):
                seen.append(name)
            continue
        img, lab = c["img"].numpy(), None if c["labels"] is None else c["labels"].numpy()
        for key, (maps, weighted) in T.MODES.items():
            if (kind == "affine" and maps == "luts") or ("normalise" in kw and not weighted):
                continue
            q = T.run_mode(key, img, lab, c, np.float64, **kw)
            got = T.wrap_u8(q) if "clamp" in kw else G.round_u8(q)
            if G.judge(c["q64"][key], got, c["tau"][key]):
                seen.append((name, key))
    assert seen, defect
    if defect == "ignored-label-recoloured":                    # only the case with label 255 can show it, in every mode
        assert sorted({n for n, _ in seen}) == ["40x52-ignore"] and len(seen) == len(T.MODES)
        c = T.reference("40x52-ignore")
        bad = T.apply_lut(c["img"].numpy(), c["labels"].numpy(), c["luts"], recolour_ignored=True)
        assert not np.array_equal(bad, T.apply_lut(c["img"].numpy(), c["labels"].numpy(), c["luts"]))     # and the exact mode too


def test_case_table_reaches_the_stated_edges():
    assert T.NAMES == ["1x1", "7x5", "33x70", "64x64-flat", "257x130", "40x52-ignore", "48x48-view", "extremes"]
    c = T.reference("40x52-ignore")
    assert (c["count"][:, 2] > 0).tolist() == [True, False] and (c["count_s"][:, 2] > 0).tolist() == [False, True]
    assert np.array_equal(c["luts"][1, 2], np.broadcast_to(np.arange(256, dtype=np.uint8), (3, 256)))       # empty on one side: identity
    assert np.array_equal(c["rows_mkl"][0, 2], np.concatenate((np.eye(3).ravel(), np.zeros(3))).astype(np.float32))
    c = T.reference("257x130")
    assert c["R"] == 4 and 257 * 130 > 8 * 4096                # nine blocks of 4096 pixels an image, the last ragged
    assert (257 * 130) % 4 != 0 and (257 * 130 * 3) % 4 != 0   # a partial last quad, and image 1 starts off a dword
    c = T.reference("7x5")
    assert c["labels"] is None and 5 % 4 != 0                  # quads cross row ends
    c = T.reference("64x64-flat")
    assert all(np.linalg.eigvalsh(c["cov"][b, r]).max() == 0 for b in range(2) for r in range(3) if c["count"][b, r])   # the floor is active
    w = c["weights"]
    assert w.dtype == np.float32 and w.min() == 0 and (w.sum(1) == 0).any() and (w.sum(1) > 1.5).any()
    c = T.reference("extremes")
    assert set(np.unique(c["img"].numpy())) == {0, 255}


def test_argument_errors_need_no_gpu():
    from ppst_amd._lib import lib
    tok = ctypes.c_void_p(16)          # a non-null token: validation runs before anything is dereferenced or launched

    lut = lambda a=tok, Bc=1, b=tok, Bs=1, pairs=tok, K=1, R=3, P=3, out=tok: lib.ppst_hist_match_lut(a, Bc, b, Bs, pairs, K, R, P, out, None)
    for kw in (dict(R=0), dict(R=5), dict(P=2), dict(P=17), dict(K=-1), dict(Bc=-1), dict(Bs=-1), dict(K=1 << 30)):
        assert lut(**kw) == -1, kw
    assert lut(a=None, b=None, pairs=None, out=None, K=0) == 0
    assert lut(R=5, a=None) == -1                                # sizes are judged ahead of the pointers
    for hole in ("a", "b", "pairs", "out"):
        assert lut(**{hole: None}) == -3, hole

    def app(img=tok, sx=3, labels=tok, B=1, H=8, W=8, R=3, mode=0, maps=tok, weights=tok, out=tok):
        return lib.ppst_colour_transfer_apply(img, 8 * 8 * 3, 8 * 3, sx, labels, 64, 8, B, H, W, R, mode, maps, weights, out, None)

    for kw in (dict(R=0), dict(R=5), dict(H=2049, W=2048), dict(H=1 << 22, W=2), dict(sx=4), dict(sx=1), dict(B=-1), dict(H=0),
               dict(W=0), dict(mode=2), dict(mode=-1), dict(B=1 << 22, H=2048, W=2048)):
        assert app(**kw) == -1, kw
    assert app(B=0, img=None, labels=None, maps=None, weights=None, out=None) == 0       # empty batch
    assert app(mode=3, img=None) == -1
    for hole in ("img", "maps", "out"):
        assert app(**{hole: None}) == -3, hole
        assert app(mode=1, **{hole: None}) == -3, hole
    assert lib.ppst_version() == 3                               # functions were added; no struct changed


def test_header_binding_and_library_agree():
    from ppst_amd import _lib, build
    text = open(os.path.join(ROOT, "include", "ppst_hip.h")).read()
    assert "colour transfer ---- */" in text and "#define PPST_ABI_VERSION 3" in text
    assert re.search(r"#define PPST_CT_LUT 0\s", text) and re.search(r"#define PPST_CT_AFFINE 1\s", text)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, nargs in (("ppst_hist_match_lut", 10), ("ppst_colour_transfer_apply", 16)):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, text)
        assert m and len(m.group(1).split(",")) == nargs, name
        restype, argtypes = _lib._SIGS[name]
        assert len(argtypes) == nargs and hasattr(_lib.lib, name) and restype is ctypes.c_int
    assert "colour_transfer.hip" in build.SOURCES and any(h.endswith("colour_lab.h") for h in build.HEADERS)
    for src in ("colour_stats.hip", "colour_transfer.hip"):     # the conversion is stated once, in the header both include
        body = open(os.path.join(ROOT, "ppst_amd", "csrc", src)).read()
        assert '#include "colour_lab.h"' in body and "cbrtf" not in body and "0.4124564" not in body


def test_ops_and_layers_refuse_without_a_gpu():
    from ppst_amd import evaluation, metrics, ops
    from ppst_amd.training import HeldOutEvaluator
    u = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    h = torch.zeros(1, 1, 3, 256, dtype=torch.int32)
    luts = torch.zeros(1, 1, 3, 256, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.hist_match_lut(h, h, [(0, 0)])
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.colour_transfer_apply(u, None, luts=luts)
    with pytest.raises(RuntimeError, match="CUDA"):
        metrics.colour_transfer(u, None)
    with pytest.raises(RuntimeError, match="CUDA"):
        evaluation.baseline_swap(u, u)
    with pytest.raises(RuntimeError, match="CUDA"):
        evaluation.baseline_grid(torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 8, 8))
    with pytest.raises(ValueError, match="both sides"):
        evaluation.baseline_swap(u, u, content_labels=torch.zeros(1, 8, 8))
    with pytest.raises(ValueError, match="method"):
        metrics.colour_transfer_maps(None, None, "idt")
    assert list(inspect.signature(ops.hist_match_lut).parameters) == ["hist_c", "hist_s", "pairs"]
    assert list(inspect.signature(ops.colour_transfer_apply).parameters) == ["u8", "labels", "luts", "affine", "weights", "out"]
    sig = inspect.signature(metrics.colour_transfer_maps)
    assert list(sig.parameters) == ["stats_c", "stats_s", "method", "pairs", "floor", "max_gain"]
    assert (sig.parameters["floor"].default, sig.parameters["max_gain"].default) == (1e-2, 8.0) == (T.FLOOR, T.MAX_GAIN)
    sig = inspect.signature(evaluation.baseline_swap)
    assert list(sig.parameters)[:8] == ["contents", "styles", "content_labels", "style_labels", "method", "regions", "feather", "smooth"]
    assert [sig.parameters[k].default for k in ("method", "regions", "feather", "smooth")] == ["hist", 3, 0, False]
    x = torch.zeros(2, 3, 16, 16)
    ev = HeldOutEvaluator(x, swaps=True)
    assert ev.baseline is None and ev.set_baseline("mkl") is ev and ev.baseline == "mkl" and ev.set_baseline(None).baseline is None
    with pytest.raises(ValueError, match="one of"):
        ev.set_baseline("idt")
    with pytest.raises(ValueError, match="swaps=True"):
        HeldOutEvaluator(x).set_baseline("hist")
