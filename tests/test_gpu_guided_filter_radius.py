"""GPU: the guided filter's fused radii 60 and 90 (csrc/guided_filter.hip: the two fused launches with a strip geometry per
radius) against the float64 restatement of tests/gf_cases.py -- pytest -m gpu.  The device is never its own judge.

Cases and bar: tests/gf_radius_cases.py (tau = tau_ref + ((runs + 1) / 2) tau_half, derived from the number of diffusion runs a
(2r + 1)-row window spans); tests/test_guided_filter_radius_cases_cpu.py shows that the inputs see a shifted window, a wrong
border mode and a strip seam of these geometries through it.  Every test prints tau and the smallest tau at which the device
would have passed.  Also: bit-equality of batch / stream / repeat / views per radius, the refusals around the new radius, and
PPSTModel.decode following Options.gf_radius.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gf_cases as C  # noqa: E402
import gf_radius_cases as RC  # noqa: E402

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", 0)


def _filter(guide, src, r, eps=C.EPS):
    """(H,W,3) or (B,H,W,3) uint8 arrays -> (uint8 (B,H,W,3), fp32 (B,3,H,W)) numpy; one array passed twice stays one tensor"""
    from ppst_amd import ops
    g = torch.from_numpy(np.array(guide if guide.ndim == 4 else guide[None])).to(_dev())
    s = g if src is guide else torch.from_numpy(np.array(src if src.ndim == 4 else src[None])).to(_dev())
    out, u8 = ops.guided_filter(g, s, r, eps, want_u8=True)
    torch.cuda.synchronize()
    return u8.cpu().numpy(), out.cpu().numpy()


def _consistent(u8, out):
    want = (torch.from_numpy(u8).permute(0, 3, 1, 2).float() / 255.0 - 0.5) * 2.0
    assert torch.equal(torch.from_numpy(out), want), "fp32 output is not (u8 / 255 - 0.5) * 2 of the uint8 output"


@pytest.mark.parametrize("case", RC.CASES, ids=C.case_id)
def test_fused_radius_against_float64(case):
    kind, H, W, r, eps = case
    g, s = C.inputs(kind, H, W)
    u8, out = _filter(g, s, r, eps)
    _consistent(u8, out)
    R = RC.ref(*case)
    need = C.min_tau(R.q64, u8[0])
    d = np.abs(u8[0].astype(int) - R.expect.astype(int))
    print("%-34s tau %.5f (tau_ref %.5f, tau_half %.5f)  device needs %.5f  max |diff| %d  differing %.4f  exempt %.4f"
          % (C.case_id(case), R.tau, R.tau_ref, R.tau_half, need, d.max(), (d > 0).mean(), R.exempt))
    bad = C.judge(R.q64, u8[0], R.tau)
    assert not bad, "%s: %s" % (C.case_id(case), "; ".join(bad))


def _batch5(H, W):
    pairs = [C.inputs(k, H, W) for k in ("blocks", "flat", "saturating", "smooth", "const_guide")]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


@pytest.mark.parametrize("r", RC.RADII)
def test_batch_stream_repeat_and_views(r):
    """Five different images in one call: each bit-equal to its single-image call; the same bytes on a side stream and on a
    repeat; a strided crop of a larger image gives the bytes of its contiguous copy."""
    from ppst_amd import ops
    H, W = RC.BITS_EXTENT[r]
    G, S = _batch5(H, W)
    u8, out = _filter(G, S, r)
    _consistent(u8, out)
    for i in range(5):
        u1, o1 = _filter(G[i], S[i], r)
        assert np.array_equal(u1[0], u8[i]) and np.array_equal(o1[0], out[i]), "image %d of the batch differs from its single call" % i
    u8b, outb = _filter(G, S, r)
    assert np.array_equal(u8b, u8) and np.array_equal(outb, out), "two runs differ"
    dev = _dev()
    g, s = torch.from_numpy(G).to(dev), torch.from_numpy(S).to(dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        o_side, u_side = ops.guided_filter(g, s, r, C.EPS, want_u8=True)
    side.synchronize()
    assert np.array_equal(u_side.cpu().numpy(), u8) and np.array_equal(o_side.cpu().numpy(), out), "side stream differs"
    bg, bs = C.inputs("blocks", H + 20, W + 12)
    big_g, big_s = torch.from_numpy(np.array(bg[None])).to(dev), torch.from_numpy(np.array(bs[None])).to(dev)
    crop_g, crop_s = big_g[:, 9:9 + H, 5:5 + W], big_s[:, 9:9 + H, 5:5 + W]
    assert not crop_g.is_contiguous()
    want, _ = _filter(bg[9:9 + H, 5:5 + W], bs[9:9 + H, 5:5 + W], r)
    _, u = ops.guided_filter(crop_g, crop_s, r, C.EPS, want_u8=True)
    assert np.array_equal(u.cpu().numpy(), want), "a strided crop differs from its contiguous copy"


REFUSED = [("r = 65", 200, 193, 65), ("r = 89", 200, 193, 89), ("r = 91", 200, 193, 91), ("r = 128", 200, 193, 128),
           ("r = 90 = H", 90, 200, 90), ("r = 90 = W", 200, 90, 90), ("r = 90, W = 2049", 100, 2049, 90)]


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


def test_decode_follows_the_radius_option():
    """PPSTModel.decode at 1024^2: with Options(gf_radius="scaled") the post-process is the r = 60 filter of the decoded image,
    with the default options (the same weights) the r = 30 filter, bit for bit (seeded weights as in tests/test_gpu_hires_swap.py)."""
    from ppst_amd import glue, ops
    from ppst_amd import weights as W
    from ppst_amd.ppst_model import Options, create_model
    sd = W.make_state_dict(2, with_D=False, with_nce=False, bias_std=0.1)
    imgs = W.synthetic_images(31, 2, size=1024)
    content, style = imgs[0:1].cuda(), imgs[1:2].cuda()
    eps = (0.02 * 255) ** 2
    with torch.no_grad():
        m = create_model(opt=Options(gf_radius="scaled"), state_dict=sd, device="cuda")
        m.noise = None
        sp = m(content, command="encode")[0]
        gl = m(style, command="encode")[1]
        plain = m(sp, gl, command="decode")
        c8, p8 = glue.tensor2im(content), glue.tensor2im(plain)
        got = m(sp, gl, target=content, command="decode")
        assert got.shape == (1, 3, 1024, 1024)
        assert torch.equal(got, ops.guided_filter(c8, p8, 60, eps)), "scaled: decode is not the r = 60 filter of the decoded image"
        m.opt = Options()                                        # the same weights under the default options
        got30 = m(sp, gl, target=content, command="decode")
        assert torch.equal(got30, ops.guided_filter(c8, p8, 30, eps)), "default options: decode is not the r = 30 filter"
        assert not torch.equal(got, got30)
