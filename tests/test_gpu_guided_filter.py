"""GPU: the colour guided filter (csrc/guided_filter.hip, ops.guided_filter) against a float64 restatement of the published
filter on the CPU (tests/gf_cases.py) -- pytest -m gpu.  The device is never its own judge.

The bar is boundary-aware (gf_cases.judge): the device's uint8 output must equal rint(q64) wherever the float64 result q64 lies
farther than tau from a rounding boundary k + 0.5; within tau it may be either neighbour; everywhere |device - rint(q64)| <= 1.
tau is computed per case from the reference alone (gf_cases.Ref):
  * radius 30 (two fused launches, (a, b) stored as IEEE half with error diffusion): tau = tau_ref + 2 tau_half;
  * every other radius (fp32 planes): tau = 2 tau_ref + 1e-3;
tau_ref = where the float32 oracle still disagrees with rint(q64); tau_half = the bound of the half storage.  Every test prints
tau and the smallest tau at which the device would have passed.  The CPU file tests/test_guided_filter_cases_cpu.py shows that
the inputs see a shifted window, a wrong border mode and a strip seam through this bar, and that at most 15 % of a case's
values are exempt.

Shown once on the device, with three libraries that carried a seeded defect (not kept):
  * the stage-2 fused kernel's vertical window one row late: 41 of the 88 tests fail -- every blocks and flat case of
    test_radius30_against_float64 (35), const_guide, aliased x 2, smooth x 2, and test_tuned_instances_against_float64;
  * reflect_idx in the BORDER_REFLECT_101 form: 67 fail -- the same 41 and all 26 cases of test_generic_radius_against_float64;
  * the last 16-output segment of a strip reading its entering column one short (stage-2 fused kernel): 34 fail -- every blocks
    and flat case with W > 177 (31), const_guide-65x200, smooth-600x530, and test_tuned_instances_against_float64.
The bit-equality tests (batch, stream, repeat, views) pass under all three by construction: they compare the device with itself.

Inputs are hard-edged block lattices (guide and source on different lattices), a flat guide over a 0 / 255 source, a pair
whose result leaves [0, 255], constant images, guide-is-source, and the smooth pair of gpu_diag.t_guided; extents sit on the
kernel's geometry: 31 x 31 (the minimum), fewer rows than a block, 191 / 192 / 193 columns around a strip, 2048 columns.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gf_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", 0)


def _filter(guide, src, r=30, eps=C.EPS):
    """(H,W,3) or (B,H,W,3) uint8 arrays -> (uint8 (B,H,W,3), fp32 (B,3,H,W)) numpy; one array passed twice stays one tensor"""
    from ppst_amd import ops
    g = torch.from_numpy(np.array(guide if guide.ndim == 4 else guide[None])).to(_dev())
    s = g if src is guide else torch.from_numpy(np.array(src if src.ndim == 4 else src[None])).to(_dev())
    out, u8 = ops.guided_filter(g, s, r, eps, want_u8=True)
    torch.cuda.synchronize()
    return u8.cpu().numpy(), out.cpu().numpy()


def _consistent(u8, out):
    """the fp32 output is (u8 / 255 - 0.5) * 2 of the device's own uint8 output, exactly (consistency, not parity)"""
    want = (torch.from_numpy(u8).permute(0, 3, 1, 2).float() / 255.0 - 0.5) * 2.0
    assert torch.equal(torch.from_numpy(out), want), "fp32 output is not (u8 / 255 - 0.5) * 2 of the uint8 output"


def _hold(label, R, u8):
    need = C.min_tau(R.q64, u8)
    d = np.abs(u8.astype(int) - R.expect.astype(int))
    print("%-32s tau %.5f (tau_ref %.5f, tau_half %.5f)  device needs %.5f  max |diff| %d  differing %.4f  exempt %.4f"
          % (label, R.tau, R.tau_ref, R.tau_half, need, d.max(), (d > 0).mean(), R.exempt))
    bad = C.judge(R.q64, u8, R.tau)
    assert not bad, "%s: %s" % (label, "; ".join(bad))


# ----------------------------------------------------------------------------------------------- radius 30, default tuning
@pytest.mark.parametrize("case", C.CASES_R30, ids=C.case_id)
def test_radius30_against_float64(case):
    g, s = C.inputs(*case)
    u8, out = _filter(g, s)
    _consistent(u8, out)
    _hold(C.case_id(case), C.ref(*case), u8[0])


def _batch5(H, W):
    pairs = [C.inputs(k, H, W) for k in ("blocks", "flat", "saturating", "smooth", "const_guide")]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


@pytest.mark.parametrize("H,W", [(70, 193), (65, 200), (31, 31)])
def test_batch_stream_repeat_and_want_u8(H, W):
    """Five different images in one call: each bit-equal to its single-image call; the same bytes on a side stream and on a
    repeat; want_u8 off returns the fp32 tensor alone, with the same values."""
    from ppst_amd import ops
    G, S = _batch5(H, W)
    u8, out = _filter(G, S)
    _consistent(u8, out)
    for i in range(5):
        u1, o1 = _filter(G[i], S[i])
        assert np.array_equal(u1[0], u8[i]) and np.array_equal(o1[0], out[i]), "image %d of the batch differs from its single call" % i
    u8b, outb = _filter(G, S)
    assert np.array_equal(u8b, u8) and np.array_equal(outb, out), "two runs differ"
    dev = _dev()
    g, s = torch.from_numpy(G).to(dev), torch.from_numpy(S).to(dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        o_side, u_side = ops.guided_filter(g, s, 30, C.EPS, want_u8=True)
    side.synchronize()
    assert np.array_equal(u_side.cpu().numpy(), u8) and np.array_equal(o_side.cpu().numpy(), out), "side stream differs"
    only = ops.guided_filter(g, s, 30, C.EPS)
    assert isinstance(only, torch.Tensor) and only.dtype == torch.float32 and tuple(only.shape) == (5, 3, H, W)
    assert np.array_equal(only.cpu().numpy(), out)
    only2 = ops.guided_filter(g, s, 30, C.EPS, want_u8=False)
    assert isinstance(only2, torch.Tensor) and np.array_equal(only2.cpu().numpy(), out)


def test_slices_of_larger_tensors_are_handled():
    """ops takes views: a crop of a larger image (strided rows and columns), one image out of a batch, and a channel-sliced
    RGBA tensor give the bytes of the contiguous copy (ops makes the copy)."""
    from ppst_amd import ops
    dev = _dev()
    bg, bs = C.inputs("blocks", 97, 200)
    big_g, big_s = torch.from_numpy(np.array(bg[None])).to(dev), torch.from_numpy(np.array(bs[None])).to(dev)
    crop_g, crop_s = big_g[:, 9:79, 5:198], big_s[:, 9:79, 5:198]
    assert not crop_g.is_contiguous()
    want, _ = _filter(bg[9:79, 5:198], bs[9:79, 5:198])
    _, u = ops.guided_filter(crop_g, crop_s, 30, C.EPS, want_u8=True)
    assert np.array_equal(u.cpu().numpy(), want)
    G, S = _batch5(70, 193)
    g, s = torch.from_numpy(G).to(dev), torch.from_numpy(S).to(dev)
    want3, _ = _filter(G[3], S[3])
    _, u = ops.guided_filter(g[3:4], s[3:4], 30, C.EPS, want_u8=True)          # (storage offset, contiguous)
    assert np.array_equal(u.cpu().numpy(), want3)
    _, u = ops.guided_filter(g[1::2], s[1::2], 30, C.EPS, want_u8=True)        # (batch stride 2)
    assert np.array_equal(u.cpu().numpy()[1], want3[0])
    rgba = torch.zeros((1, 70, 193, 4), dtype=torch.uint8, device=dev)
    rgba[..., :3] = g[3]
    _, u = ops.guided_filter(rgba[..., :3], s[3:4], 30, C.EPS, want_u8=True)   # (pixel stride 4)
    assert np.array_equal(u.cpu().numpy(), want3)


REFUSED = [("W = 2049", 40, 2049, 30), ("r = H", 30, 200, 30), ("r > H", 20, 200, 30), ("r = W", 200, 30, 30),
           ("r = W, generic", 70, 16, 16), ("r = 0", 70, 90, 0), ("r = 65", 200, 193, 65), ("r < 0", 70, 90, -1)]


@pytest.mark.parametrize("why,H,W,r", REFUSED, ids=[x[0] for x in REFUSED])
def test_refusals_raise_and_write_nothing(why, H, W, r):
    """ops raises; the entry point itself returns its error code with the outputs and the workspace untouched"""
    from ppst_amd import ops
    from ppst_amd._lib import lib
    dev = _dev()
    g = torch.full((1, H, W, 3), 90, dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="ppst_guided_filter"):
        ops.guided_filter(g, g, r, C.EPS, want_u8=True)
    out = torch.full((1, 3, H, W), 7.0, device=dev)
    out_u8 = torch.full((1, H, W, 3), 201, dtype=torch.uint8, device=dev)
    ws = torch.full((lib.ppst_guided_filter_ws(1, H, W),), 55, dtype=torch.uint8, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = lib.ppst_guided_filter(p(g), p(g), p(out), p(out_u8), 1, H, W, r, float(C.EPS), p(ws),
                                ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    assert rc != 0
    assert bool((out == 7.0).all()) and bool((out_u8 == 201).all()) and bool((ws == 55).all()), "a refused call wrote"


def test_mismatched_or_malformed_inputs_are_refused():
    """guide and source of different shapes, or not (B, H, W, 3), would make the kernels read past the smaller tensor"""
    from ppst_amd import ops
    dev = _dev()
    g = torch.zeros((1, 70, 90, 3), dtype=torch.uint8, device=dev)
    for bad in (torch.zeros((1, 69, 90, 3), dtype=torch.uint8, device=dev), torch.zeros((1, 70, 90, 1), dtype=torch.uint8, device=dev),
                torch.zeros((70, 90, 3), dtype=torch.uint8, device=dev)):
        with pytest.raises(RuntimeError):
            ops.guided_filter(g, bad, 30, C.EPS)
        with pytest.raises(RuntimeError):
            ops.guided_filter(bad, g, 30, C.EPS)
    with pytest.raises(RuntimeError):
        ops.guided_filter(g.float(), g, 30, C.EPS)
    with pytest.raises(RuntimeError):
        ops.guided_filter(g.cpu(), g, 30, C.EPS)


def test_empty_batch_returns_empty_outputs():
    from ppst_amd import ops
    g = torch.zeros((0, 70, 90, 3), dtype=torch.uint8, device=_dev())
    out, u8 = ops.guided_filter(g, g, 30, C.EPS, want_u8=True)
    assert tuple(out.shape) == (0, 3, 70, 90) and out.dtype == torch.float32
    assert tuple(u8.shape) == (0, 70, 90, 3) and u8.dtype == torch.uint8
    out = ops.guided_filter(g, g, 7, C.EPS)
    assert tuple(out.shape) == (0, 3, 70, 90)


# ---------------------------------------------------------------------------------------------------------- generic radius
@pytest.mark.parametrize("case", C.CASES_GENERIC, ids=C.case_id)
def test_generic_radius_against_float64(case):
    kind, H, W, r, eps = case
    g, s = C.inputs(kind, H, W)
    u8, out = _filter(g, s, r, eps)
    _consistent(u8, out)
    _hold(C.case_id(case), C.ref(*case), u8[0])


def test_generic_radius_batch_matches_single_calls():
    G, S = _batch5(70, 90)
    u8, out = _filter(G, S, 7)
    _consistent(u8, out)
    for i in range(5):
        u1, _ = _filter(G[i], S[i], 7)
        assert np.array_equal(u1[0], u8[i]), i


# --------------------------------------------------------------------------------------------------------- tuned instances
def test_tuned_instances_against_float64():
    """ppst_guided_filter_tune selects other template instances of the two fused launches (rows per block).  They restart the
    error diffusion at other rows, so they are held to the bar against float64, not to each other's bytes.  The setting is
    process-global: (0, 0) is restored, and the default call then reproduces its earlier bytes."""
    from ppst_amd._lib import lib
    before = {c: _filter(*C.inputs(*c))[0] for c in C.TUNE_CASES}
    try:
        for vs1, vs2 in C.TUNES:
            assert lib.ppst_guided_filter_tune(vs1, vs2) == 0
            for c in C.TUNE_CASES:
                u8, out = _filter(*C.inputs(*c))
                _consistent(u8, out)
                _hold("%s tune (%d, %d)" % (C.case_id(c), vs1, vs2), C.ref(*c), u8[0])
    finally:
        lib.ppst_guided_filter_tune(0, 0)
    for c in C.TUNE_CASES:
        assert np.array_equal(_filter(*C.inputs(*c))[0], before[c]), "the default setting was not restored"
