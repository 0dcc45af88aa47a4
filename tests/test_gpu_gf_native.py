"""GPU: the native-size guided filter (csrc/guided_filter.hip: ppst_guided_filter_coeffs, gf_apply_up_kernel;
ops.guided_filter_coeffs / guided_filter_apply; PPSTModel.decode_native; evaluation.simple_swap_native /
evaluate_swap_files_native) against the float64 restatement of the whole pipeline on the CPU (tests/gf_native_cases.py) --
pytest -m gpu.  The device is never its own judge.

Bar (gf_cases.judge): the device's uint8 output equals rint(q64) wherever q64 lies farther than tau from a rounding boundary,
may be either neighbour within tau, and everywhere |device - rint(q64)| <= 1; tau = 2 max|q32 - q64| + 1e-3 from the reference
alone.  Every test prints tau and the tau the device would have needed.  tests/test_gf_native_cases_cpu.py shows that the cases
see a missing half-pixel offset, a tile without its last footprint column and zeros outside the plane through this bar.

Cases beyond the issue's table, at the extents the kernel's 64-column x 16-row tiles make special (gf_native_cases.TILE_CASES):
(33,40) -> (63,127), (64,128), (65,129) -- one short of, exactly, and one past 4 x 2 tiles at scale 2, the last with a tile of
one row and a tile of one column -- and (70,90) -> (71,91), whose tiles have the largest footprint (17 x 65 coefficient
samples) starting at tap -1; (70,90) -> (70,90) of the table is the largest footprint at scale 1, where LDS column 64 is staged.
Not covered: an output past 2^31 bytes (B H W 12 > 2^31 needs 8 GB of fp32 output); every index that can pass 2^31 is int64
by construction.
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

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", 0)


def _t(a):
    return torch.from_numpy(np.array(a if a.ndim == 4 else a[None])).to(_dev())


def _run(lo, src, native, r, eps=C.EPS):
    """uint8 arrays (h,w,3) x 2, (H,W,3) (or batches) -> (uint8 (B,H,W,3), fp32 (B,3,H,W), coeffs (B,12,h,w)) numpy"""
    from ppst_amd import ops
    co = ops.guided_filter_coeffs(_t(lo), _t(src), r, eps)
    u8, f32 = ops.guided_filter_apply(co, _t(native), want_f32=True)
    torch.cuda.synchronize()
    return u8.cpu().numpy(), f32.cpu().numpy(), co.cpu().numpy()


def _consistent(u8, f32):
    want = (torch.from_numpy(u8).permute(0, 3, 1, 2).float() / 255.0 - 0.5) * 2.0
    assert torch.equal(torch.from_numpy(f32), want), "fp32 output is not (u8 / 255 - 0.5) * 2 of the uint8 output"


@pytest.mark.parametrize("case", C.ALL_CASES, ids=C.case_id)
def test_native_output_against_float64(case):
    R = C.ref(*case)
    u8, f32, _ = _run(R.lo, R.src, R.native, R.r)
    _consistent(u8, f32)
    need = G.min_tau(R.q64, u8[0])
    d = np.abs(u8[0].astype(int) - R.expect.astype(int))
    print("%-40s tau %.5f (max|q32-q64| %.2e)  device needs %.5f  max |diff| %d  differing %.5f  exempt %.4f"
          % (C.case_id(case), R.tau, R.floor32, need, d.max(), (d > 0).mean(), R.exempt))
    bad = G.judge(R.q64, u8[0], R.tau)
    assert not bad, "%s: %s" % (C.case_id(case), "; ".join(bad))


@pytest.mark.parametrize("case", C.PLANE_CASES, ids=lambda c: "%s-%dx%d-r%d" % c)
def test_coefficient_planes_against_float64(case):
    """the 12 mean planes alone, at generic radii and at 30 / 60 (which run the fp32-plane launches here, not the fused ones).
    Bar: 2 max|planes32 - planes64| + 1e-6 max|planes64|, from the reference alone.  The entry's V pass accumulates in double
    and divides once, and its solve is compiled without contraction (gfc_v_kernel, gfc_solve_kernel), so the device's error is
    the float32 run's own: MI355X 1.08e-3 / 2.7e-5 / 2.0e-5 / 1.9e-5 against bars of 2.47e-3 / 2.8e-4 / 2.5e-4 / 1.9e-4."""
    from ppst_amd import ops
    g, s, p64, bar = C.plane_ref(*case)
    co = ops.guided_filter_coeffs(_t(g), _t(s), case[3], C.EPS).cpu().numpy()[0].astype(np.float64)
    err = float(np.abs(co - p64).max())
    print("planes %-24s bar %.3e  device error %.3e  max|planes64| %.1f" % ("%s-%dx%d-r%d" % case, bar, err, np.abs(p64).max()))
    assert err <= bar


def test_scale_one_against_the_filter_itself():
    """at scale 1 the pipeline IS the guided filter: reported, not a bar -- compiler contraction may differ"""
    from ppst_amd import ops
    g, s = G.inputs("blocks", 70, 90)
    u8, _, _ = _run(g, s, g, 7)
    _, ref = ops.guided_filter(_t(g), _t(s), 7, C.EPS, want_u8=True)
    diff = (torch.from_numpy(u8) != ref.cpu())
    print("scale 1, r = 7, blocks 70x90: %d of %d bytes differ from ops.guided_filter" % (int(diff.sum()), diff.numel()))
    assert int((torch.from_numpy(u8).int() - ref.cpu().int()).abs().max()) <= 1


def _batch3():
    cs = [("blocks", 33, 40, 65, 129, 7), ("flat", 33, 40, 65, 129, 7), ("saturating", 33, 40, 65, 129, 7)]
    ins = [C.native_inputs(*c[:5]) for c in cs]
    return np.stack([i[1] for i in ins]), np.stack([i[2] for i in ins]), np.stack([i[0] for i in ins])


def test_batch_stream_repeat_and_views():
    """three different images in one call: each bit-equal to its single call; the same bytes on a repeat and on a side stream;
    want_f32 off returns the uint8 tensor alone; sliced, non-contiguous and unaligned inputs give the bytes of their copies"""
    from ppst_amd import ops
    LO, SRC, NAT = _batch3()
    u8, f32, co = _run(LO, SRC, NAT, 7)
    _consistent(u8, f32)
    for i in range(3):
        u1, f1, c1 = _run(LO[i], SRC[i], NAT[i], 7)
        assert np.array_equal(u1[0], u8[i]) and np.array_equal(f1[0], f32[i]) and np.array_equal(c1[0], co[i]), "image %d" % i
    u8b, f32b, cob = _run(LO, SRC, NAT, 7)
    assert np.array_equal(u8b, u8) and np.array_equal(f32b, f32) and np.array_equal(cob, co), "two runs differ"
    dev = _dev()
    lo, src, nat = _t(LO), _t(SRC), _t(NAT)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        co_s = ops.guided_filter_coeffs(lo, src, 7, C.EPS)
        u_s, f_s = ops.guided_filter_apply(co_s, nat, want_f32=True)
    side.synchronize()
    assert np.array_equal(u_s.cpu().numpy(), u8) and np.array_equal(f_s.cpu().numpy(), f32) and np.array_equal(co_s.cpu().numpy(), co)
    only = ops.guided_filter_apply(co_s, nat)
    assert isinstance(only, torch.Tensor) and only.dtype == torch.uint8 and np.array_equal(only.cpu().numpy(), u8)
    # views: one image of the batch (storage offset 65 * 129 * 3: odd, so no row span of guide or output starts on a dword),
    # batch stride 2, a crop of a larger native image, a channel slice of RGBA
    co_t = torch.from_numpy(co).to(dev)
    assert np.array_equal(ops.guided_filter_apply(co_t[1:2], nat[1:2]).cpu().numpy(), u8[1:2])
    assert np.array_equal(ops.guided_filter_apply(co_t[0::2], nat[0::2]).cpu().numpy(), u8[0::2])
    assert np.array_equal(ops.guided_filter_coeffs(lo[0::2], src[0::2], 7, C.EPS).cpu().numpy(), co[0::2])
    big = torch.zeros((3, 80, 140, 4), dtype=torch.uint8, device=dev)
    big[:, 9:74, 5:134, :3] = nat
    crop = big[:, 9:74, 5:134, :3]
    assert not crop.is_contiguous()
    assert np.array_equal(ops.guided_filter_apply(co_t, crop).cpu().numpy(), u8)
    pad = torch.zeros((3, 12, 40, 50), device=dev)
    pad[:, :, 3:36, 4:44] = co_t
    assert np.array_equal(ops.guided_filter_apply(pad[:, :, 3:36, 4:44], nat).cpu().numpy(), u8)


def test_the_u8_output_alone_and_the_f32_output_alone():
    """either output of the entry point may be absent: the other one keeps its bytes"""
    from ppst_amd._lib import lib
    dev = _dev()
    LO, SRC, NAT = _batch3()
    u8, f32, co = _run(LO, SRC, NAT, 7)
    co_t, nat = torch.from_numpy(co).to(dev), _t(NAT)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    out = torch.full((3, 3, 65, 129), 7.0, device=dev)
    assert lib.ppst_guided_filter_apply(p(co_t), 33, 40, p(nat), None, p(out), 3, 65, 129, st) == 0
    o8 = torch.full((3, 65, 129, 3), 201, dtype=torch.uint8, device=dev)
    assert lib.ppst_guided_filter_apply(p(co_t), 33, 40, p(nat), p(o8), None, 3, 65, 129, st) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), f32) and np.array_equal(o8.cpu().numpy(), u8)


REFUSED_COEFFS = [("r = 65", 200, 193, 65), ("r = 90", 200, 193, 90), ("r = h", 30, 200, 30), ("r = w", 200, 30, 30), ("w = 2049", 40, 2049, 7),
                  ("r = 0", 70, 90, 0)]
REFUSED_APPLY = [("H < h", 70, 90, 69, 180), ("W < w", 70, 90, 140, 89)]


@pytest.mark.parametrize("why,h,w,r", REFUSED_COEFFS, ids=[x[0] for x in REFUSED_COEFFS])
def test_coefficient_refusals_raise_and_write_nothing(why, h, w, r):
    from ppst_amd import ops
    from ppst_amd._lib import lib
    dev = _dev()
    g = torch.full((1, h, w, 3), 90, dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="ppst_guided_filter_coeffs"):
        ops.guided_filter_coeffs(g, g, r, C.EPS)
    co = torch.full((1, 12, h, w), 7.0, device=dev)
    ws = torch.full((lib.ppst_guided_filter_ws(1, h, w),), 55, dtype=torch.uint8, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = lib.ppst_guided_filter_coeffs(p(g), p(g), p(co), 1, h, w, r, float(C.EPS), p(ws), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    assert rc == -1 and bool((co == 7.0).all()) and bool((ws == 55).all()), "a refused call wrote"


@pytest.mark.parametrize("why,h,w,H,W", REFUSED_APPLY, ids=[x[0] for x in REFUSED_APPLY])
def test_apply_refusals_raise_and_write_nothing(why, h, w, H, W):
    from ppst_amd import ops
    from ppst_amd._lib import lib
    dev = _dev()
    co = torch.zeros((1, 12, h, w), device=dev)
    g = torch.full((1, H, W, 3), 90, dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="ppst_guided_filter_apply"):
        ops.guided_filter_apply(co, g)
    out = torch.full((1, 3, H, W), 7.0, device=dev)
    o8 = torch.full((1, H, W, 3), 201, dtype=torch.uint8, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = lib.ppst_guided_filter_apply(p(co), h, w, p(g), p(o8), p(out), 1, H, W, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    assert rc == -1 and bool((out == 7.0).all()) and bool((o8 == 201).all()), "a refused call wrote"


def test_malformed_inputs_and_empty_batches():
    from ppst_amd import ops
    dev = _dev()
    g = torch.zeros((1, 70, 90, 3), dtype=torch.uint8, device=dev)
    co = torch.zeros((1, 12, 70, 90), device=dev)
    for bad in (torch.zeros((1, 69, 90, 3), dtype=torch.uint8, device=dev), torch.zeros((70, 90, 3), dtype=torch.uint8, device=dev)):
        with pytest.raises(RuntimeError, match="one shape"):
            ops.guided_filter_coeffs(g, bad, 7)
    with pytest.raises(RuntimeError, match="uint8"):
        ops.guided_filter_coeffs(g.float(), g, 7)
    for bc, bg in ((co[:, :11], g), (co, g[..., :2]), (co, torch.zeros((2, 70, 90, 3), dtype=torch.uint8, device=dev)), (co[0], g)):
        with pytest.raises(RuntimeError, match="B,12,h,w"):
            ops.guided_filter_apply(bc, bg)
    with pytest.raises(RuntimeError, match="float32"):
        ops.guided_filter_apply(co.half(), g)
    with pytest.raises(RuntimeError, match="uint8"):
        ops.guided_filter_apply(co, g.float())
    e = ops.guided_filter_coeffs(g[:0], g[:0], 7)
    assert tuple(e.shape) == (0, 12, 70, 90) and e.dtype == torch.float32
    u8, f32 = ops.guided_filter_apply(e, torch.zeros((0, 140, 180, 3), dtype=torch.uint8, device=dev), want_f32=True)
    assert tuple(u8.shape) == (0, 140, 180, 3) and u8.dtype == torch.uint8 and tuple(f32.shape) == (0, 3, 140, 180)


# ------------------------------------------------------------------------------------------------------------- model level
def _model():
    from ppst_amd import weights as W
    from ppst_amd.ppst_model import create_model
    sd = W.make_state_dict(3, with_D=False, with_nce=False, bias_std=0.1, noise_weight=0.0)
    return create_model(state_dict=sd, device=_dev())


def _native_u8(seed, n, side):
    """n seeded pictures as (n,side,side,3) uint8 on the host: synthetic 512^2 images resized by Pillow, detail included"""
    from PIL import Image
    from ppst_amd import weights as W
    base = W.synthetic_images(seed, n, size=512)
    u8 = ((base.clamp(-1, 1) + 1) * 127.5).to(torch.uint8).permute(0, 2, 3, 1).numpy()
    return np.stack([np.array(Image.fromarray(a).resize((side, side), Image.BICUBIC)) for a in u8])


@pytest.fixture(scope="module")
def model():
    return _model()


@pytest.mark.parametrize("side", [1024, 640])
def test_simple_swap_native_is_its_steps_by_hand(model, side, monkeypatch):
    """simple_swap_native, 512^2 model size, against encode / extract_feat_from_image / Rselfcorr / corrm / encode2 /
    decode_native through the facade, bit for bit; and decode_native's coefficients come from the pair decode(target=...) filters"""
    from ppst_amd import evaluation as EV, glue, imageio, ops
    dev = _dev()
    nat = torch.from_numpy(_native_u8(41, 2, side)).to(dev)
    native, style = nat[0:1], imageio.preprocess(nat[1:2], 512)
    alphas = (0.5, 1.0)
    with torch.no_grad():
        got = EV.simple_swap_native(model, native, style, alphas, 512)
        content = imageio.preprocess(native, 512)
        assert tuple(content.shape) == (1, 3, 512, 512)
        sp, gl_c = model(content, command="encode")
        fea_c, fea_c1 = model(content, command="extract_feat_from_image")
        fea_s, fea_s1 = model(style, command="extract_feat_from_image")
        fea_c = torch.cat((fea_c, model(fea_c1, command="Rselfcorr")), dim=1)
        fea_s = torch.cat((fea_s, model(fea_s1, command="Rselfcorr")), dim=1)
        corr = model(fea_s, fea_c, command="corrm")
        _, gl_w = model(style, corr, command="encode2")
        seen = {}
        real_f, real_c = ops.guided_filter, ops.guided_filter_coeffs
        monkeypatch.setattr(ops, "guided_filter", lambda g, s, r, eps, **kw: seen.__setitem__("decode", (g.clone(), s.clone(), r, eps)) or real_f(g, s, r, eps, **kw))
        monkeypatch.setattr(ops, "guided_filter_coeffs", lambda g, s, r, eps: seen.__setitem__("native", (g.clone(), s.clone(), r, eps)) or real_c(g, s, r, eps))
        for alpha in alphas:
            code = glue.lerp(gl_c, gl_w, alpha)
            hand = model(sp, code, content, native, command="decode_native")
            assert hand.dtype == torch.uint8 and tuple(hand.shape) == (1, side, side, 3)
            assert torch.equal(hand, got[alpha]), "alpha %g: simple_swap_native differs from its steps by hand" % alpha
            model(sp, code, target=content, command="decode")
            (g1, s1, r1, e1), (g2, s2, r2, e2) = seen["decode"], seen["native"]
            assert torch.equal(g1, g2) and torch.equal(s1, s2) and (r1, e1) == (r2, e2) == (30, (0.02 * 255) ** 2)
            # ... and the result is the coefficients of that pair applied to the native image
            assert torch.equal(hand, ops.guided_filter_apply(real_c(g2, s2, r2, e2), native))
        assert not torch.equal(got[0.5], got[1.0])


def test_evaluate_swap_files_native_writes_what_the_recipe_returns(model, tmp_path):
    """two 640^2 PNG files: the written files decode to simple_swap_native's tensors; host and device decoders give the same
    bytes; the device encoder writes the same pictures"""
    from PIL import Image
    from ppst_amd import evaluation as EV, imageio
    dev = _dev()
    arr = _native_u8(43, 2, 640)
    cp, sp_ = str(tmp_path / "c0.png"), str(tmp_path / "s1.png")
    Image.fromarray(arr[0]).save(cp)
    Image.fromarray(arr[1]).save(sp_)
    alphas = (0.5, 1.0)
    with torch.no_grad():
        want = EV.simple_swap_native(model, torch.from_numpy(arr[0:1]).to(dev), imageio.preprocess(torch.from_numpy(arr[1:2]).to(dev), 512), alphas, 512)
        ph = EV.evaluate_swap_files_native(model, cp, sp_, str(tmp_path / "host"), alphas=alphas)
        with EV.decoder("device"):
            pd = EV.evaluate_swap_files_native(model, cp, sp_, str(tmp_path / "device"), alphas=alphas)
        pe = EV.evaluate_swap_files_native(model, [cp], [sp_], str(tmp_path / "enc"), alphas=alphas, png="device")
    assert [os.path.basename(p) for p in ph] == [os.path.basename(p) for p in pd] == [os.path.basename(p) for p in pe] == ["c0_s1_0.50.png", "c0_s1_1.00.png"]
    for alpha, a, b, c in zip(alphas, ph, pd, pe):
        w = want[alpha][0].cpu().numpy()
        assert w.shape == (640, 640, 3)
        for path in (a, b, c):
            assert np.array_equal(np.asarray(Image.open(path)), w), path
