"""CPU: the cases, restatements and bars of tests/test_gpu_matte.py (tests/matte_cases.py), and what the matte entry points
refuse without a GPU -- nothing here touches one.

  * sd2_separable == sd2_brute on every case of side <= 64; the constants of the cases module are the source's; both symbols
    are declared, bound and exported, and matte.hip is a build source;
  * every seeded transform defect breaks bit-equality on at least two cases; every seeded matte or paste defect violates its bar
    on at least two cases; the fp32 restatements pass their own bars; the paste bar's exempt share is <= 1 % on every case;
  * ppst_label_matte and ppst_guided_filter_paste_matte reject bad arguments before any launch; ops and the front ends refuse
    from types, shapes and integers alone.
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
import matte_cases as M  # noqa: E402
import region_cases as C  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [c for c in M.CASES if (c[1], c[2]) != M.BIG]


def test_the_table_has_the_issues_cases():
    assert {(c[1], c[2]) for c in M.CASES} == set(M.SHAPES) | {M.BIG} and len(M.CASES) == len(set(M.CASES))
    S, W = M.MT_SEG, M.MT_ROW
    assert {(1, 1), (1, 37), (37, 1), (8, 8), (24, 24), (40, 40), (S - 1, 33), (S, 33), (S + 1, 33), (2 * S + 1, 70), (20, W - 1), (20, W),
            (20, W + 1), (70, 2 * W + 3)} == set(M.SHAPES) and M.BIG == (520, 520)
    assert M.FG == [(0, 0), (1, 0), (1, 1), (6, 3), (16, 8), (0, 5), (255, 0), (255, 255)]
    for p in M.PATTERNS:                                           # every pattern meets every (feather, grow)
        assert {(c[4], c[5]) for c in M.CASES if c[3] == p} == set(M.FG), p
    vals = set(np.unique(M.PATTERNS["values"](40, 40)[0]).tolist())
    assert vals == {0, 1, 2, 3, 31, 32, 255} and (M.PATTERNS["values"](40, 40)[1] >> 31) & 1 and (M.PATTERNS["values-hi"](8, 8)[1] >> 31) & 1
    # the seam half-planes end exactly on the kernels' seams where the plane reaches them
    assert M.PATTERNS["seam-row"](2 * S + 1, 70)[0][:, 0].sum() == S and M.PATTERNS["seam-col"](20, W + 1)[0][0].sum() == W
    assert M.radius(255, 0) == M.radius(255, 255) == 256 > max(h for h, _ in M.SHAPES)   # R exceeds the plane's height
    assert len(M.PASTE_FG) == len(C.ALL_CASES) == 19 and all(M.radius(*M.PASTE_FG[c[0]]) <= c[3] for c in C.ALL_CASES)
    assert len(set(M.PASTE_FG.values())) >= 6


@pytest.mark.parametrize("shape", [s for s in M.SHAPES if max(s) <= 64], ids=lambda s: "%dx%d" % s)
def test_separable_is_the_definition(shape):
    for c in M.cases_of(shape):
        R = M.matte_ref(c)
        assert np.array_equal(R.sd2, M.sd2_brute(R.labels, R.keep, R.feather, R.grow)), c[0]
        assert R.sd2.dtype == np.int32 and np.abs(R.sd2).max() <= M.radius(R.feather, R.grow) ** 2 and (R.sd2 != 0).all()


def test_constants_symbols_and_build_source():
    src = open(os.path.join(ROOT, "ppst_amd", "csrc", "matte.hip")).read()
    assert int(re.search(r"#define MT_SEG (\d+)", src).group(1)) == M.MT_SEG
    assert int(re.search(r"#define MT_ROW (\d+)", src).group(1)) == M.MT_ROW
    gf = open(os.path.join(ROOT, "ppst_amd", "csrc", "guided_filter.hip")).read()
    assert int(re.search(r"#define GP_T (\d+)", gf).group(1)) == C.PASTE_T
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ppst_hip.h")).read(), flags=re.S)
    import __graft_entry__ as g
    g.build()
    from ppst_amd import _lib, build
    assert "matte.hip" in build.SOURCES
    for name in ("ppst_label_matte", "ppst_guided_filter_paste_matte"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib._SIGS and hasattr(_lib.lib, name), name
    assert "#define PPST_ABI_VERSION 3" in open(os.path.join(ROOT, "include", "ppst_hip.h")).read() and _lib.ABI_VERSION == 3


def test_entry_points_reject_bad_arguments_before_any_launch():
    import __graft_entry__ as g
    g.build()
    from ppst_amd._lib import lib
    d = ctypes.c_void_p(16)            # a non-null token: validation happens before anything on the device is touched

    def lm(labels=d, B=1, h=24, w=24, keep=6, feather=16, grow=8, sd2=d, matte=d):
        return lib.ppst_label_matte(labels, B, h, w, keep, feather, grow, sd2, matte, None)

    for bad in (dict(B=-1), dict(h=0), dict(w=0), dict(h=4097), dict(w=4097), dict(h=-3), dict(feather=-1), dict(feather=256), dict(grow=-1),
                dict(grow=256)):
        assert lm(**bad) == -1, bad
    assert lm(labels=None) == -3 and lm(sd2=None) == -3
    assert lm(B=0, labels=None, sd2=None, matte=None) == 0
    assert lm(B=0, h=0) == -1 and lm(B=0, grow=256) == -1

    table = lambda *rows: (ctypes.c_int64 * (4 * len(rows)))(*[v for r in rows for v in r])
    ok = table((1 << 23, 0, 0, 0))

    def paste(co=d, matte=d, n=24, photo=d, out=d, B=1, H=90, W=70, xh=ok, xd=d, feather=1):
        return lib.ppst_guided_filter_paste_matte(co, matte, n, photo, out, B, H, W, xh, xd, feather, None)

    for null in ("co", "matte", "photo", "out", "xh", "xd"):
        assert paste(**{null: None}) == -3, null
    for bad in (dict(B=-1), dict(H=0), dict(W=0), dict(n=0), dict(n=4097), dict(H=1 << 14, W=(1 << 14) + 1), dict(feather=-1), dict(feather=13)):
        assert paste(**bad) == -1, bad
    for rows in (((1 << 23) + 1, 0, 0, 0), (1 << 19, 0, 0, 0), (0, 0, 0, 0), (1 << 23, 0, (1 << 56) + 1, 0)):
        assert paste(xh=table(rows)) == -1, rows
    assert paste(B=0, co=None, matte=None, photo=None, out=None, xh=None, xd=None) == 0 and paste(B=0, feather=13) == -1
    assert paste(xh=table((1 << 23, 0, 1 << 40, 0))) == 0       # a square that does not meet its photo: nothing to launch


@pytest.mark.parametrize("defect", M.SD2_DEFECTS)
def test_every_transform_defect_breaks_bit_equality_on_two_cases(defect):
    seen = [c[0] for c in SMALL if not np.array_equal(M.matte_ref(c).sd2, M.matte_ref(c).sd2_defect(defect))]
    print(defect, "seen by", len(seen), "cases:", seen[:12])
    assert len(seen) >= 2, (defect, seen)


@pytest.mark.parametrize("defect", M.MATTE_DEFECTS)
def test_every_matte_defect_violates_the_bar_on_two_cases(defect):
    seen = [c[0] for c in SMALL if np.abs(M.matte_ref(c).matte_defect(defect) - M.matte_ref(c).m64).max() > M.matte_ref(c).tol]
    print(defect, "seen by", len(seen), "cases:", seen[:12])
    assert len(seen) >= 2, (defect, seen)


def test_fp32_mattes_pass_their_own_bar():
    worst = max(M.matte_ref(c).floor32 for c in M.CASES)
    print("matte: largest max|m32 - m64| over %d cases %.3e" % (len(M.CASES), worst))
    for c in M.CASES:
        R = M.matte_ref(c)
        assert np.abs(R.m32.astype(np.float64) - R.m64).max() <= R.tol and R.m64.min() >= 0 and R.m64.max() <= 1, c[0]
        if R.grow == 0:
            assert (R.m64[R.sd2 < 0] == 0).all(), c[0]             # grow = 0 feathers inwards only
    assert worst <= 1e-6


@pytest.mark.parametrize("case", C.ALL_CASES, ids=C.case_id)
def test_paste_case_conditions_from_the_restatement_alone(case):
    P = M.paste_ref(case)
    share0 = float((P.untouched & P.inside).sum()) / max(int(P.inside.sum()), 1)
    print("%-24s matte (f %d, g %d)  max|r32-r64| %.2e tau %.2e exempt %.4f  inside %.2f  zero-weight share of the square %.2f"
          % (case[0], P.mf, P.mg, P.floor32, P.tau, P.exempt, P.inside.mean(), share0))
    assert P.exempt <= 0.01
    assert not M.judge_paste(P, G.round_u8(P.ref32)), "the float32 run of the paste judge misses its own bar"
    assert P.inside.any() and 0 < P.M.max() <= 1 and P.M.min() >= 0


@pytest.mark.parametrize("defect", M.PASTE_DEFECTS)
def test_every_paste_defect_violates_the_bar_on_two_cases(defect):
    seen = [c[0] for c in C.ALL_CASES if M.judge_paste(M.paste_ref(c), M.paste_ref(c).defect(defect))]
    print(defect, "seen by", seen)
    assert len(seen) >= 2, (defect, seen)


def test_an_all_ones_matte_is_the_plain_paste_and_zeros_leave_the_photo():
    for c in C.ALL_CASES[:6]:
        P = C.paste_ref(c)
        one = np.ones((P.n, P.n), np.float32)
        assert np.array_equal(M.paste_matte(P.planes, one, P.photo, P.xf, P.feather, np.float32), P.ref32), c[0]
        assert np.array_equal(M.paste_matte(P.planes, 0 * one, P.photo, P.xf, P.feather), P.photo.astype(np.float64)), c[0]


def test_ops_and_front_ends_refuse_from_types_and_shapes_alone():
    from ppst_amd import evaluation as EV, imageio, ops
    from ppst_amd.ppst_model import PPSTModel

    class FakeCuda(torch.Tensor):
        is_cuda = True
    fake = lambda t: t.as_subclass(FakeCuda)
    lab = torch.zeros((1, 24, 24), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="CUDA uint8"):
        ops.label_matte(lab)
    with pytest.raises(RuntimeError, match="CUDA uint8"):
        ops.label_matte(fake(lab.long()))
    with pytest.raises(RuntimeError, match="B,h,w"):
        ops.label_matte(fake(lab[0]))
    for keep in ((32,), (-1,), (1, 2.5)):
        with pytest.raises(RuntimeError, match="0..31"):
            ops.label_matte(fake(lab), keep)
    photo, co = torch.zeros((1, 90, 70, 3), dtype=torch.uint8), torch.zeros((1, 12, 24, 24))
    xf = [(1 << 23, 0, 0, 0)]
    for bad in (torch.zeros((1, 24, 23)), torch.zeros((2, 24, 24)), torch.zeros((1, 24, 24), dtype=torch.float64), "matte"):
        with pytest.raises(RuntimeError, match="float32 matte"):
            ops.guided_filter_paste(fake(co), fake(photo), xf, 0, matte=bad)
    assert list(inspect.signature(ops.guided_filter_paste).parameters) == ["coeffs", "photo_u8", "xf", "feather", "out", "matte"]
    sig = inspect.signature(ops.label_matte).parameters
    assert [(k, v.default) for k, v in sig.items()][1:] == [("keep", (1, 2)), ("feather", 16), ("grow", 8), ("want_distance", False)]
    big = torch.zeros((1, 3000, 4000, 3), dtype=torch.uint8)
    good = imageio.crop_transform((2000.0, 1500.0), 1024.0, 10.0)
    style = torch.zeros((1, 3, 512, 512))
    lab512 = torch.zeros((1, 512, 512), dtype=torch.uint8)
    with pytest.raises(ValueError, match="not both"):
        EV.simple_swap_region_matte(None, big, good, style, labels=lab512, matte=torch.zeros((1, 512, 512)))
    with pytest.raises(ValueError, match="crop's frame"):
        EV.simple_swap_region_matte(None, big, good, style, labels=lab512[:, :500])
    with pytest.raises(ValueError, match="uint8 or int64"):
        EV.simple_swap_region_matte(None, big, good, style, labels=lab512.float())
    with pytest.raises(ValueError, match="< 1"):
        EV.simple_swap_region_matte(None, big, imageio.crop_transform((2000.0, 1500.0), 300.0, 10.0), style, labels=lab512)
    onehot = torch.zeros((2, 4, 8, 8))
    onehot[:, 3] = 1
    assert torch.equal(EV.crop_labels(onehot, 2, 8), torch.full((2, 8, 8), 3, dtype=torch.uint8))
    assert EV.crop_labels(torch.full((1, 8, 8), 300, dtype=torch.int64), 1, 8).max() == 255
    sig = inspect.signature(EV.simple_swap_region_matte).parameters
    assert list(sig)[:8] == list(inspect.signature(EV.simple_swap_region).parameters)
    assert [(k, sig[k].default) for k in list(sig)[8:]] == [("labels", None), ("keep", (1, 2)), ("matte_feather", 16), ("matte_grow", 8),
                                                           ("matte", None)]
    sig = inspect.signature(EV.evaluate_swap_files_region).parameters
    assert [(k, sig[k].default) for k in list(sig)[-4:]] == [("label_path", None), ("keep", (1, 2)), ("matte_feather", 16), ("matte_grow", 8)]
    with pytest.raises(ValueError, match="label paths"):
        EV.evaluate_swap_files_region(None, ["a.png", "b.png"], "t.png", "unused", (2000.0, 1500.0, 1024.0, 0.0), label_path=["x", "y", "z"])
    assert list(inspect.signature(PPSTModel().decode_region_matte).parameters) == ["spatial_code", "global_code", "target", "photo_u8", "xf",
                                                                                   "feather", "matte"]
