"""CPU: the cases, restatements and bars of tests/test_gpu_gmatte.py (tests/gmatte_cases.py), and what the guided-matte entry
points refuse without a GPU -- nothing here touches one.

  * ``quantise`` on ties, negatives, values above 1 and NaN; ``mcoeffs`` is planes 0..3 of gf_native_cases.mean_planes on the
    replicated source, and its two runs quantise the blob mattes alike;
  * on the 19 region cases the float32 run of the paste restatement passes its own bar, its floor is <= 7.2e-5, tau <= 1.14e-3 and
    the exempt share <= 1 %; the weight's float32 run passes the weight's bar;
  * every seeded arithmetic defect violates the bar on at least 10 cases, the two geometric ones on at least one;
  * the three symbols are declared, bound and exported, PPST_ABI_VERSION stays 3, the entry points reject bad arguments before any
    launch; ops, the model command and the front ends refuse from types, shapes and integers alone; the new signatures, and the
    pinned ones of the existing functions.
"""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gf_cases as G  # noqa: E402
import gf_native_cases as N  # noqa: E402
import gmatte_cases as GM  # noqa: E402
import matte_cases as M  # noqa: E402
import region_cases as C  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS_DEFAULT = (0.01 * 255) ** 2


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
def test_quantise_on_ties_negatives_values_above_one_and_nan(dtype):
    m = np.array([0.0, 1.0, -0.25, -1e30, 1.5, 1e30, np.nan, np.inf, -np.inf, 0.5 / 255, 1.5 / 255, 2.5 / 255, 100.0 / 255, 0.999], np.float64)
    q = GM.quantise(m, dtype)
    assert q.dtype == dtype and np.isfinite(q).all() and (q == np.rint(q)).all() and q.min() >= 0 and q.max() <= 255
    assert q[:9].tolist() == [0, 255, 0, 0, 255, 255, 0, 255, 0]
    assert q[12] == 100 and q[13] == 255
    # exact ties go to the even neighbour: k + 0.5 is 255 m exactly for m = (k + 0.5) / 255 only where the division is exact, so
    # the ties are made from the product's side: values whose product with 255 IS k + 0.5 in the dtype
    k = np.arange(0, 255, dtype=np.float64)
    ties = ((k + 0.5) / 255).astype(dtype)
    prod = (dtype(255) * ties).astype(dtype)
    exact = prod == (k + 0.5).astype(dtype)
    assert exact.sum() >= 20, "too few exact ties to show the rounding mode"
    want = np.where(k % 2 == 0, k, k + 1)                                  # k + 0.5 -> the even one of k, k + 1
    assert np.array_equal(GM.quantise(ties, dtype)[exact], want[exact].astype(dtype))
    assert np.array_equal(GM.quantise(ties, dtype)[~exact], np.rint(prod[~exact]))
    assert GM.source_u8(np.array([np.nan, -3.0, 7.0, 0.5], np.float32)).tolist() == [0, 0, 255, 128]


def test_mcoeffs_is_planes_0_to_3_of_the_colour_filter_on_the_replicated_source():
    g = G.inputs("blocks", 40, 52)[0]
    m = GM.blob_matte(40, 52)
    for dtype in (np.float64, np.float32):
        p = GM.quantise(m, dtype)
        full = N.mean_planes(g, np.stack([p, p, p], -1), 3, GM.EPS, dtype)
        got = GM.mcoeffs(g, m, 3, GM.EPS, dtype)
        assert got.dtype == dtype and got.shape == (4, 40, 52) and np.array_equal(got, full[:4])
        assert np.array_equal(full[:4], full[4:8]) and np.array_equal(full[:4], full[8:])     # (every channel of (p, p, p) alike)
    assert GM.R == 8 and GM.EPS == EPS_DEFAULT
    zero = GM.mcoeffs(g, np.zeros((40, 52), np.float32), 3)
    assert (zero == 0).all(), "an all-zero matte must give all-zero coefficients"
    one = GM.mcoeffs(g, np.ones((40, 52), np.float32), 3)
    assert np.abs(one[:3]).max() < 1e-9 and np.abs(one[3] - 255).max() < 1e-9    # a constant source: a = 0, b = p


@pytest.mark.parametrize("case", N.PLANE_CASES, ids=lambda c: "%s-%dx%d-r%d" % c)
def test_plane_bar_comes_from_two_runs_that_quantise_alike(case):
    g, m, p64, bar, floor32 = GM.plane_ref(*case)
    differ = int((GM.quantise(m, np.float64) != GM.quantise(m, np.float32)).sum())
    print("%s %dx%d r %d: max|planes64| %.4g  max|planes32 - planes64| %.3e  bar %.3e  source bytes differing between the runs %d"
          % (case + (np.abs(p64).max(), floor32, bar, differ)))
    assert differ == 0, "a float32 product fell on the other side of a tie: the bar would hold a whole source level"
    assert 0 < bar < 1e-2 * np.abs(p64).max()
    assert np.array_equal(GM.source_u8(m).astype(np.float64), GM.quantise(m, np.float64))


def test_coefficient_cases_are_the_issues():
    assert set(GM.COEFF_CASES) == {(k, h, w, r) for k in ("blocks", "flat") for (h, w) in ((70, 90), (200, 193)) for r in (1, 3, 8, 16, 64)
                                   if r < min(h, w)}
    assert len(GM.COEFF_CASES) == 20 and GM.MATTES == ("blob", "zeros", "ones", "uniform-nan", "ties")
    u = GM.matte_of("uniform-nan", 70, 90)
    assert np.isnan(u).sum() > 100 and np.nanmin(u) < -0.4 and np.nanmax(u) > 1.4
    t = GM.matte_of("ties", 70, 90)
    prod = np.float32(255) * t
    assert (prod == np.floor(prod) + 0.5).mean() > 0.1, "the tie field holds too few exact ties in float32"
    assert (GM.matte_of("zeros", 5, 6) == 0).all() and (GM.matte_of("ones", 5, 6) == 1).all()
    assert all(a.dtype == np.float32 for a in (u, t, GM.matte_of("blob", 24, 24)))


@pytest.mark.parametrize("case", C.ALL_CASES, ids=C.case_id)
def test_paste_case_conditions_from_the_restatement_alone(case):
    P = GM.paste_ref(case)
    Pm = M.paste_ref(case)
    share0 = float((P.untouched & P.inside).sum()) / max(int(P.inside.sum()), 1)
    print("%-24s r %d  max|r32-r64| %.2e tau %.3e exempt %.4f  weight: max|w32-w64| %.2e tau %.3e  zero-weight share of the square %.2f"
          % (case[0], P.r, P.floor32, P.tau, P.exempt, P.wfloor32, P.wtau, share0))
    assert P.photo is Pm.photo and P.xf == Pm.xf and P.feather == Pm.feather and P.planes is Pm.planes and P.M is Pm.M
    assert P.r == min(3, P.n - 1) and P.mco.dtype == np.float32 and P.mco.shape == (4, P.n, P.n)
    assert np.array_equal(P.mco, GM.mcoeffs(P.guide, P.M, P.r, GM.EPS, np.float64).astype(np.float32))
    assert P.tau == 2 * P.floor32 + 1e-3 and P.wtau == 2 * P.wfloor32 + 1e-3
    assert P.exempt <= 0.01
    assert not GM.judge_paste(P, G.round_u8(P.ref32)), "the float32 run of the paste judge misses its own bar"
    w32 = 255.0 * GM.paste_gmatte(P.planes, P.mco, P.photo, P.xf, P.feather, np.float32, want_g=True)[1].astype(np.float64)
    assert not GM.judge_weight(P, G.round_u8(w32)), "the float32 run of the weight misses its own bar"
    assert P.inside.any() and P.g64.min() >= 0 and P.g64.max() <= 1 and (P.g64[~P.inside] == 0).all()
    assert np.array_equal(P.ref64[P.untouched], P.photo[P.untouched].astype(np.float64))


def test_floor_and_tau_over_the_19_cases():
    assert len(C.ALL_CASES) == 19
    floor32 = max(GM.paste_ref(c).floor32 for c in C.ALL_CASES)
    tau = max(GM.paste_ref(c).tau for c in C.ALL_CASES)
    exempt = max(GM.paste_ref(c).exempt for c in C.ALL_CASES)
    print("guided-matte paste over 19 cases: largest max|r32 - r64| %.3e, largest tau %.4e, largest exempt share %.4f" % (floor32, tau, exempt))
    assert floor32 <= 7.2e-5 and tau <= 1.14e-3 and exempt <= 0.01


@pytest.mark.parametrize("defect", GM.PASTE_DEFECTS)
def test_every_arithmetic_defect_violates_the_bar_on_ten_cases(defect):
    seen = [c[0] for c in C.ALL_CASES if GM.judge_paste(GM.paste_ref(c), GM.paste_ref(c).defect(defect))]
    print(defect, "seen by", len(seen), "cases:", seen)
    assert len(seen) >= 10, (defect, seen)


@pytest.mark.parametrize("defect", GM.GEOMETRIC_DEFECTS)
def test_every_geometric_defect_is_seen(defect):
    seen = [c[0] for c in C.ALL_CASES if GM.judge_paste(GM.paste_ref(c), GM.paste_ref(c).defect(defect))]
    print(defect, "seen by", len(seen), "cases:", seen)
    assert len(seen) >= 1, (defect, seen)


def test_coefficients_of_a_constant_matte_are_the_plain_paste_or_the_photo():
    for c in C.ALL_CASES[:6]:
        P = GM.paste_ref(c)
        ones = np.zeros((4, P.n, P.n), np.float32)
        ones[3] = 255
        assert np.array_equal(GM.paste_gmatte(P.planes, ones, P.photo, P.xf, P.feather, np.float32), C.paste_ref(c).ref32), c[0]
        assert np.array_equal(GM.paste_gmatte(P.planes, 0 * ones, P.photo, P.xf, P.feather), P.photo.astype(np.float64)), c[0]
        nan = np.full((4, P.n, P.n), np.nan, np.float32)
        assert np.array_equal(GM.paste_gmatte(P.planes, nan, P.photo, P.xf, P.feather), P.photo.astype(np.float64)), c[0]


@pytest.mark.parametrize("case", GM.LEAK_CASES, ids=C.case_id)
def test_leak_cases_have_a_poisoned_set(case):
    P = GM.paste_ref(case)
    assert P.n >= 24
    D = GM.disc_matte(P.n)
    assert set(np.unique(D).tolist()) == {0.0, 1.0}
    mco = GM.mcoeffs(P.guide, D, GM.LEAK_R).astype(np.float32)
    yy, xx = np.meshgrid(np.arange(P.n), np.arange(P.n), indexing="ij")
    far = np.hypot(yy - (P.n - 1) / 2.0, xx - (P.n - 1) / 2.0) > P.n / 4.0 + 6
    # by geometry the coefficients vanish beyond n / 4 + 6 from the centre (the disc, + 1/2, + 2 r, + the diagonal): the
    # restatement's integral images leave a residue of cancellation there, the device's direct sums leave exact zeros
    assert far.any() and np.abs(mco[:, far]).max() < 1e-9 < np.abs(mco).max()
    mco[:, far] = 0
    bad = GM.poison(P.planes, mco)
    assert np.isnan(bad).any() and np.isnan(bad[0]).mean() < 0.9
    _, g = GM.paste_gmatte(P.planes, mco, P.photo, P.xf, P.feather, np.float64, want_g=True)
    assert np.array_equal(GM.paste_gmatte(bad, mco, P.photo, P.xf, P.feather), GM.paste_gmatte(P.planes, mco, P.photo, P.xf, P.feather))
    assert g.max() > 0.5


def test_symbols_constants_and_abi():
    header_text = open(os.path.join(ROOT, "include", "ppst_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header_text, flags=re.S)
    gf = open(os.path.join(ROOT, "ppst_amd", "csrc", "guided_filter.hip")).read()
    assert int(re.search(r"#define GP_T (\d+)", gf).group(1)) == C.PASTE_T
    import __graft_entry__ as g
    g.build()
    from ppst_amd import _lib
    for name, ret in (("ppst_guided_matte_ws", "int64_t"), ("ppst_guided_matte_coeffs", "int"), ("ppst_guided_filter_paste_gmatte", "int")):
        assert re.search(r"\b%s\s+%s\s*\(" % (ret, name), header), name
        assert name in _lib._SIGS and hasattr(_lib.lib, name), name
    assert "#define PPST_ABI_VERSION 3" in header_text and _lib.ABI_VERSION == 3
    assert _lib.lib.ppst_guided_matte_ws(3, 70, 90) == 3 * 26 * 70 * 90 * 4
    assert _lib.lib.ppst_guided_matte_ws(1, 512, 512) * 21 == _lib.lib.ppst_guided_filter_ws(1, 512, 512) * 13


def test_entry_points_reject_bad_arguments_before_any_launch():
    import __graft_entry__ as g
    g.build()
    from ppst_amd._lib import lib
    d = ctypes.c_void_p(16)            # a non-null token: validation happens before anything on the device is touched

    def co(guide=d, matte=d, out=d, B=1, h=24, w=30, r=3, eps=6.5, work=d):
        return lib.ppst_guided_matte_coeffs(guide, matte, out, B, h, w, r, eps, work, None)

    for bad in (dict(r=0), dict(r=-1), dict(r=65), dict(r=90), dict(r=24), dict(r=30, h=40), dict(w=2049, h=100), dict(B=-1), dict(h=0), dict(w=0)):
        assert co(**bad) == -1, bad
    for null in ("guide", "matte", "out", "work"):
        assert co(**{null: None}) == -3, null
    assert co(B=0, guide=None, matte=None, out=None, work=None) == 0 and co(B=0, r=0) == -1

    table = lambda *rows: (ctypes.c_int64 * (4 * len(rows)))(*[v for r in rows for v in r])
    ok = table((1 << 23, 0, 0, 0))

    def paste(co=d, mco=d, n=24, photo=d, out=d, weight=None, B=1, H=90, W=70, xh=ok, xd=d, feather=1):
        return lib.ppst_guided_filter_paste_gmatte(co, mco, n, photo, out, weight, B, H, W, xh, xd, feather, None)

    for null in ("co", "mco", "photo", "out", "xh", "xd"):
        assert paste(**{null: None}) == -3, null
        assert paste(weight=d, **{null: None}) == -3, null
    for bad in (dict(B=-1), dict(H=0), dict(W=0), dict(n=0), dict(n=4097), dict(H=1 << 14, W=(1 << 14) + 1), dict(feather=-1), dict(feather=13)):
        assert paste(**bad) == -1, bad
    for rows in (((1 << 23) + 1, 0, 0, 0), (1 << 19, 0, 0, 0), (0, 0, 0, 0), (1 << 23, 0, (1 << 56) + 1, 0)):
        assert paste(xh=table(rows)) == -1, rows
    assert paste(B=0, co=None, mco=None, photo=None, out=None, xh=None, xd=None) == 0 and paste(B=0, feather=13) == -1
    assert paste(xh=table((1 << 23, 0, 1 << 40, 0))) == 0       # a square that does not meet its photo: nothing to launch


class FakeCuda(torch.Tensor):
    is_cuda = True


def _fake(t):
    return t.as_subclass(FakeCuda)


def test_ops_refuse_from_types_and_shapes_alone():
    from ppst_amd import ops
    guide, m = torch.zeros((2, 24, 30, 3), dtype=torch.uint8), torch.zeros((2, 24, 30))
    with pytest.raises(RuntimeError, match="CUDA uint8 guide"):
        ops.guided_matte_coeffs(guide, m)
    with pytest.raises(RuntimeError, match="CUDA uint8 guide"):
        ops.guided_matte_coeffs(_fake(guide.float()), m)
    with pytest.raises(RuntimeError, match="CUDA uint8 guide"):
        ops.guided_matte_coeffs("guide", m)
    for bad in (guide[0], guide[..., :2]):
        with pytest.raises(RuntimeError, match=r"\(B,h,w,3\)"):
            ops.guided_matte_coeffs(_fake(bad), m)
    for bad in (m[:1], m[:, :, :29], m.double(), m[0], m.unsqueeze(1), "matte", None):
        with pytest.raises(RuntimeError, match="float32 matte"):
            ops.guided_matte_coeffs(_fake(guide), bad)
    sig = inspect.signature(ops.guided_matte_coeffs).parameters
    assert [(k, v.default) for k, v in sig.items()] == [("guide_u8", inspect.Parameter.empty), ("matte", inspect.Parameter.empty), ("r", 8),
                                                        ("eps", EPS_DEFAULT)]

    photo, co, mco = torch.zeros((1, 90, 70, 3), dtype=torch.uint8), torch.zeros((1, 12, 24, 24)), torch.zeros((1, 4, 24, 24))
    xf = [(1 << 23, 0, 0, 0)]
    with pytest.raises(RuntimeError, match="CUDA float32 coefficients"):
        ops.guided_filter_paste_gmatte(co, mco, _fake(photo), xf)
    with pytest.raises(RuntimeError, match="CUDA uint8 photo"):
        ops.guided_filter_paste_gmatte(_fake(co), mco, photo, xf)
    for bad_co in (co[:, :11], co[:, :, :23], torch.zeros((2, 12, 24, 24))):
        with pytest.raises(RuntimeError, match=r"\(B,12,n,n\)"):
            ops.guided_filter_paste_gmatte(_fake(bad_co), mco, _fake(photo), xf)
    for bad in (mco[:, :3], torch.zeros((1, 12, 24, 24)), torch.zeros((1, 4, 24, 23)), torch.zeros((2, 4, 24, 24)), mco.double(), mco[0], "m", None):
        with pytest.raises(RuntimeError, match="float32 matte coefficients"):
            ops.guided_filter_paste_gmatte(_fake(co), bad, _fake(photo), xf)
    for bad_out in (torch.zeros((1, 90, 70, 3)), torch.zeros((1, 90, 71, 3), dtype=torch.uint8), "out"):
        with pytest.raises(RuntimeError, match="out must be"):
            ops.guided_filter_paste_gmatte(_fake(co), mco, _fake(photo), xf, out=bad_out)
    sig = inspect.signature(ops.guided_filter_paste_gmatte).parameters
    assert [(k, v.default) for k, v in sig.items()][4:] == [("feather", 0), ("out", None), ("want_weight", False)]
    assert list(sig)[:4] == ["coeffs", "mcoeffs", "photo_u8", "xf"]
    # the existing paste keeps its parameter list and its refusals
    assert list(inspect.signature(ops.guided_filter_paste).parameters) == ["coeffs", "photo_u8", "xf", "feather", "out", "matte"]
    with pytest.raises(RuntimeError, match="guided_filter_paste: out must be"):
        ops.guided_filter_paste(_fake(co), _fake(photo), xf, out=torch.zeros((1, 90, 70, 3)))


def test_model_and_front_ends_refuse_before_anything_runs_and_keep_their_signatures():
    from ppst_amd import evaluation as EV, imageio
    from ppst_amd.ppst_model import PPSTModel, guided_matte_radius
    model = PPSTModel()
    target = torch.zeros((1, 3, 40, 40))
    with pytest.raises(ValueError, match="needs a matte"):
        model.decode_region_gmatte(None, None, target, None, None)
    for r in (0, -1, 65, 40, 2.5):
        with pytest.raises(ValueError, match="matte_radius"):
            model.decode_region_gmatte(None, None, target, None, None, 0, torch.zeros((1, 40, 40)), r)     # (before the generator runs)
    assert guided_matte_radius(8, 512) == 8 and guided_matte_radius(64, 65) == 64 and guided_matte_radius(8.0, 9) == 8
    with pytest.raises(ValueError, match="needs a matte"):
        model(None, None, target, None, None, command="decode_region_gmatte")
    sig = inspect.signature(model.decode_region_gmatte).parameters
    assert list(sig)[:7] == list(inspect.signature(model.decode_region_matte).parameters)
    assert [(k, sig[k].default) for k in list(sig)[5:]] == [("feather", 0), ("matte", None), ("matte_radius", 8), ("matte_eps", EPS_DEFAULT),
                                                          ("want_weight", False)]

    big = torch.zeros((1, 3000, 4000, 3), dtype=torch.uint8)
    good = imageio.crop_transform((2000.0, 1500.0), 1024.0, 10.0)
    style = torch.zeros((1, 3, 512, 512))
    lab512 = torch.zeros((1, 512, 512), dtype=torch.uint8)
    with pytest.raises(ValueError, match="needs labels or a matte"):
        EV.simple_swap_region_gmatte(None, big, good, style)
    with pytest.raises(ValueError, match="simple_swap_region_gmatte takes labels or a matte, not both"):
        EV.simple_swap_region_gmatte(None, big, good, style, labels=lab512, matte=torch.zeros((1, 512, 512)))
    with pytest.raises(ValueError, match="crop's frame"):
        EV.simple_swap_region_gmatte(None, big, good, style, labels=lab512[:, :500])
    with pytest.raises(ValueError, match="uint8 or int64"):
        EV.simple_swap_region_gmatte(None, big, good, style, labels=lab512.float())
    with pytest.raises(ValueError, match="< 1"):
        EV.simple_swap_region_gmatte(None, big, imageio.crop_transform((2000.0, 1500.0), 300.0, 10.0), style, labels=lab512)
    for r in (0, 65, 512):
        with pytest.raises(ValueError, match="matte_radius"):
            EV.simple_swap_region_gmatte(None, big, good, style, labels=lab512, matte_radius=r)
    sig = inspect.signature(EV.simple_swap_region_gmatte).parameters
    old = inspect.signature(EV.simple_swap_region_matte).parameters
    assert list(sig)[:len(old)] == list(old) and all(sig[k].default == old[k].default for k in old)
    assert [(k, sig[k].default) for k in list(sig)[len(old):]] == [("matte_radius", 8), ("matte_eps", EPS_DEFAULT), ("want_weight", False)]

    box = (2000.0, 1500.0, 1024.0, 0.0)
    with pytest.raises(ValueError, match="needs label_path"):
        EV.evaluate_swap_files_region_gmatte(None, "a.png", "t.png", "unused", box)
    with pytest.raises(ValueError, match="matte_radius"):
        EV.evaluate_swap_files_region_gmatte(None, "a.png", "t.png", "unused", box, label_path="l.png", matte_radius=0)
    with pytest.raises(ValueError, match="label paths"):
        EV.evaluate_swap_files_region_gmatte(None, ["a.png", "b.png"], "t.png", "unused", box, label_path=["x", "y", "z"])
    sig = inspect.signature(EV.evaluate_swap_files_region_gmatte).parameters
    old = inspect.signature(EV.evaluate_swap_files_region).parameters
    assert list(sig)[:len(old)] == list(old) and all(sig[k].default == old[k].default for k in old)
    assert [(k, sig[k].default) for k in list(sig)[len(old):]] == [("matte_radius", 8), ("matte_eps", EPS_DEFAULT)]

    # the pinned parameter lists of the existing functions are what their own tests state
    assert list(inspect.signature(model.decode_region).parameters) == ["spatial_code", "global_code", "target", "photo_u8", "xf", "feather"]
    assert list(inspect.signature(model.decode_region_matte).parameters) == ["spatial_code", "global_code", "target", "photo_u8", "xf", "feather",
                                                                            "matte"]
    assert list(inspect.signature(EV.simple_swap_region).parameters) == ["model", "photo_u8", "xf", "style", "alphas", "load_size", "feather",
                                                                         "style_xf"]
    assert list(old)[-4:] == ["label_path", "keep", "matte_feather", "matte_grow"]
    assert list(inspect.signature(EV.simple_swap_region_matte).parameters)[8:] == ["labels", "keep", "matte_feather", "matte_grow", "matte"]
    with pytest.raises(ValueError, match="simple_swap_region_matte takes labels or a matte, not both"):
        EV.simple_swap_region_matte(None, big, good, style, labels=lab512, matte=torch.zeros((1, 512, 512)))
