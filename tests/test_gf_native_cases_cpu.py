"""CPU: the cases, the judge and the bar of tests/test_gpu_gf_native.py (tests/gf_native_cases.py), the integer tap arithmetic,
and what the native-size entry points refuse without a GPU -- nothing here touches one.

  * per case, from the reference alone: the exempt share stays at or below gf_cases.EXEMPT_CAP, the float32 run of the judge
    passes the bar, and every seeded defect (no half-pixel offset, a 64-column tile without its last footprint column, zeros
    outside the plane) violates it wherever the scale exceeds 1;
  * the integer taps equal floor and fraction of the float64 position (Y + 0.5) n / N - 0.5 for every Y at sizes up to 8192;
  * both C entry points reject bad arguments before any launch; ops refuse CPU tensors; simple_swap_native and decode_native
    refuse from shapes alone.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gf_cases as G  # noqa: E402
import gf_native_cases as C  # noqa: E402


@pytest.mark.parametrize("case", C.ALL_CASES, ids=C.case_id)
def test_case_conditions_from_the_reference_alone(case):
    R = C.ref(*case)
    print("%-40s max|q32-q64| %.2e  tau %.2e  exempt %.4f  outside 0..255 %.3f" % (C.case_id(case), R.floor32, R.tau, R.exempt, R.saturating))
    assert R.exempt <= G.EXEMPT_CAP
    assert not G.judge(R.q64, G.round_u8(R.q32), R.tau), "the float32 run of the judge misses its own bar"
    if case[0] == "saturating":
        assert R.saturating > 0.25
    if case in C.SENSITIVE:
        for d in C.DEFECTS:
            assert G.judge(R.q64, R.defect(d), R.tau), "seeded defect %r passes the bar" % d


def test_the_table_has_the_issues_cases_and_the_tile_edges():
    assert len(C.CASES) == 11 and set(C.SENSITIVE) == set(C.ALL_CASES) - {("blocks", 70, 90, 70, 90, 7)}
    Ws, Hs = {c[4] for c in C.ALL_CASES}, {c[3] for c in C.ALL_CASES}
    assert {C.TILE_W * 2 - 1, C.TILE_W * 2, C.TILE_W * 2 + 1} <= Ws and {C.TILE_H * 4 - 1, C.TILE_H * 4, C.TILE_H * 4 + 1} <= Hs
    # the largest footprint, (TILE_H + 1) x (TILE_W + 1) coefficient samples under one tile: scale 1, and barely above it
    for c in (("blocks", 70, 90, 70, 90, 7), ("flat", 70, 90, 71, 91, 7)):
        assert c in C.ALL_CASES
        iy, _, _ = C.taps(c[1], c[3])
        ix, _, _ = C.taps(c[2], c[4])
        assert iy[C.TILE_H - 1] + 1 - iy[0] + 1 == C.TILE_H + 1 and ix[C.TILE_W - 1] + 1 - ix[0] + 1 == C.TILE_W + 1
    # n <= N: i0 grows by 0 or 1 per output sample, so no tile's footprint is larger than that
    for n, N in ((70, 70), (70, 71), (33, 1000), (512, 1024), (8191, 8192)):
        i0, _, _ = C.taps(n, N)
        assert i0[0] >= -1 and set(np.diff(i0)) <= {0, 1}


TAP_SIZES = [(512, 512), (512, 1024), (512, 2048), (512, 4096), (512, 8192), (1024, 8192), (70, 211), (97, 388), (33, 1000), (40, 77),
             (33, 35), (65, 129), (65, 131), (1, 8192), (2, 3), (2047, 8192), (4096, 8191), (8191, 8192), (8192, 8192), (3000, 7919)]


@pytest.mark.parametrize("n,N", TAP_SIZES, ids=["%d-to-%d" % s for s in TAP_SIZES])
def test_integer_taps_are_floor_and_fraction_of_the_float64_position(n, N):
    i0, rem, den = C.taps(n, N)
    pos = (np.arange(N, dtype=np.float64) + 0.5) * n / N - 0.5
    assert np.array_equal(i0, np.floor(pos).astype(np.int64))
    assert np.abs(rem / den - (pos - np.floor(pos))).max() < 1e-9
    assert rem.min() >= 0 and rem.max() < den and i0.min() >= -1 and i0.max() <= n - 1


def test_entry_points_reject_bad_arguments_before_any_launch():
    import __graft_entry__ as g
    g.build()
    from ppst_amd._lib import lib
    d = ctypes.c_void_p(16)            # a non-null token: validation happens before anything is dereferenced or launched
    eps = float(G.EPS)

    def coeffs(guide=d, src=d, out=d, B=1, h=70, w=90, r=7, work=d):
        return lib.ppst_guided_filter_coeffs(guide, src, out, B, h, w, r, eps, work, None)

    def apply(co=d, h=70, w=90, guide=d, u8=d, f32=d, B=1, H=140, W=180):
        return lib.ppst_guided_filter_apply(co, h, w, guide, u8, f32, B, H, W, None)

    for null in ("guide", "src", "out", "work"):
        assert coeffs(**{null: None}) == -3, null
    for bad in (dict(r=65), dict(r=90, h=200, w=200), dict(r=70), dict(r=71), dict(h=7), dict(w=7), dict(r=0), dict(r=-1),
                dict(w=2049, h=100), dict(h=0), dict(B=-1)):
        assert coeffs(**bad) == -1, bad
    assert coeffs(B=0, guide=None, src=None, out=None, work=None) == 0
    assert coeffs(B=0, r=65) == -1
    for null in ("co", "guide"):
        assert apply(**{null: None}) == -3, null
    assert apply(u8=None, f32=None) == -3                     # both outputs absent
    for bad in (dict(H=69), dict(W=89), dict(H=1 << 14, W=(1 << 14) + 1), dict(h=0), dict(w=0), dict(B=-1)):
        assert apply(**bad) == -1, bad
    assert apply(B=0, co=None, guide=None, u8=None, f32=None) == 0
    assert apply(B=0, H=69) == -1


def test_ops_refuse_cpu_tensors_and_malformed_shapes():
    from ppst_amd import ops
    g = torch.zeros((1, 70, 90, 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.guided_filter_coeffs(g, g, 7)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.guided_filter_apply(torch.zeros((1, 12, 70, 90)), torch.zeros((1, 140, 180, 3), dtype=torch.uint8))


def test_simple_swap_native_size_rule_from_shapes_alone():
    from ppst_amd import evaluation as EV
    style = torch.zeros((1, 3, 512, 512))
    u8 = lambda H, W: torch.zeros((1, H, W, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="square"):
        EV.simple_swap_native(None, u8(1024, 1000), style)
    with pytest.raises(ValueError, match="at least load_size"):
        EV.simple_swap_native(None, u8(500, 500), style)
    with pytest.raises(ValueError, match="at least load_size"):
        EV.simple_swap_native(None, u8(640, 640), style, load_size=1024)
    with pytest.raises(ValueError, match="multiple of 512"):
        EV.simple_swap_native(None, u8(640, 640), style, load_size=600)
    with pytest.raises(ValueError, match="B,H,W,3"):
        EV.simple_swap_native(None, torch.zeros((1, 3, 640, 640), dtype=torch.uint8), style)
    EV.native_size_rule((2, 512, 512, 3), 512)
    EV.native_size_rule((1, 4096, 4096, 3), 1024)


def test_decode_native_refuses_a_radius_the_coefficient_entry_does_not_run():
    """"scaled" at 1536^2 is radius 90, which exists only as fused launches: ValueError from shapes alone, before the generator"""
    from ppst_amd.ppst_model import PPSTModel
    m = PPSTModel()
    m.opt.gf_radius = "scaled"
    with pytest.raises(ValueError, match="r = 90"):
        m(None, None, torch.empty((1, 3, 1536, 1536)), None, command="decode_native")
    m.opt.gf_radius = 65
    with pytest.raises(ValueError, match="r <= 64"):
        m.decode_native(None, None, torch.empty((1, 3, 512, 512)), None)


def test_new_front_ends_have_the_issues_signatures():
    import inspect
    from ppst_amd import evaluation as EV
    assert list(inspect.signature(EV.simple_swap_native).parameters) == ["model", "content_native_u8", "style", "alphas", "load_size"]
    assert list(inspect.signature(EV.evaluate_swap_files_native).parameters) == list(inspect.signature(EV.evaluate_swap_files).parameters)
    for a, b in zip(inspect.signature(EV.evaluate_swap_files_native).parameters.values(),
                    inspect.signature(EV.evaluate_swap_files).parameters.values()):
        assert a.default == b.default
