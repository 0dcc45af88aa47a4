"""GPU: the two native ops -- ppst_upfirdn2d (csrc/upfirdn2d.hip) and ppst_fused_bias_act (csrc/fused_bias_act.hip) -- called through
ops.upfirdn2d_raw / ops.fused_bias_act_raw on every case of tests/fir_cases.py and compared with its float64 reference -- pytest -m
gpu.  The device is never its own judge.

Each case names the launch form its dispatcher picks (fir_cases.uf_form / fba_form restate the ``if``s; printed with the error, pytest
-s shows the table); tests/test_fir_cases_cpu.py shows on the CPU that the references are right, that every form and facet has a case
and that the comparison used here, at the bar used here, rejects every seeded defect on these very inputs.

Next to the references: every output is written into a NaN-filled buffer whose guard elements on both sides must stay NaN, a repeat is
bit-identical, a half-stored launch equals the fp32 launch on the widened input rounded once, empty calls return, refused calls leave
their output untouched -- and the adjoints the train step and the R1 penalty run (stylegan2_op.upfirdn2d and fused_leaky_relu to second
order, autograd.BlurDownFn, the input gradient of autograd.blur_conv) equal float64 autograd of the reference.  No test sets process
environment.
"""
import os
import sys
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fir_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 256
f64 = torch.float64


def _dev():
    return torch.device("cuda", 0)


def _np(t):
    return t.detach().double().cpu().numpy()


def _place(shape, dtype, off, src=None, fill=float("nan")):
    """a dense tensor of ``shape`` that starts GUARD + off elements into a buffer the test owns (fill in front and behind); -> (buffer, view)"""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD + off,), fill, device=_dev(), dtype=dtype)
    view = buf[GUARD + off:GUARD + off + n].view(*shape)
    if src is not None:
        view.copy_(src.to(_dev()).to(dtype))
    return buf, view


def _guards_intact(buf, off, n, what):
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:GUARD + off]).all()) and bool(torch.isnan(buf[GUARD + off + n:]).all()), "%s: wrote outside its output" % what


def _launch(c, widen=False):
    from ppst_amd import ops
    p, inp = c.p, C.inputs(c.id)
    dt = torch.float32 if widen else C.TD[p["st"]]
    off = p["off"]
    _, x = _place(inp["x"].shape, dt, off, inp["x"])
    if c.op == "upfirdn2d":
        shape = (p["M"],) + C.uf_out_hw(p) + (p["C"],)
        buf, y = _place(shape, dt, off)
        k = inp["k"].to(_dev())                              # (fp32 taps; double in a float64 call)
        got = ops.upfirdn2d_raw(x, k, *p["up"], *p["down"], *p["pads"], out=y)
    else:
        shape = p["shape"]
        buf, y = _place(shape, dt, off)
        b = inp["b"].to(_dev()).to(dt) if "b" in inp else None
        ref = _place(shape, dt, off, inp["ref"])[1] if "ref" in inp else None
        got = ops.fused_bias_act_raw(x, b, ref, p["act"], p["grad"], p["alpha"], p["scale"], out=y)
    assert got.data_ptr() == y.data_ptr() and (y.data_ptr() - buf.data_ptr()) == (GUARD + off) * y.element_size()
    _guards_intact(buf, off, int(np.prod(shape)), c.id)
    return y.detach().cpu()


def _run(c, widen=False):
    try:
        return _launch(c, widen)
    except RuntimeError as e:
        if any(s in str(e) for s in ("illegal memory access", "HIP error", "hipError")):
            pytest.exit("the device faulted in %s: nothing more is launched (%s)" % (c.id, e), returncode=3)
        raise


# --------------------------------------------------------------------------------------------- against the float64 reference
@pytest.mark.parametrize("cid", [c.id for c in C.CASES])
def test_against_float64_reference(cid):
    c = C.by_id(cid)
    st = c.p["st"]
    got = _run(c)
    assert got.dtype == C.TD[st]
    bad, err = C.judge(c, "y", _np(got))
    unit = st != "f32" and C.reference(cid)["y"].any()          # half / float64: err comes in units of the allowed error
    b = C.bar(c, "y") if st != "f64" else float("nan")
    print("FIR %-62s %-20s err %.3e  bar %.2e  of-bar %.3f" % (cid, C.branch_of(c), err, b, err if unit else (err / b if err else 0.0)))
    assert not bad, "%s [%s]: %s" % (cid, C.branch_of(c), "; ".join(bad))
    assert torch.equal(_run(c).view(torch.uint8), got.view(torch.uint8)), "two runs differ"
    if st in C.A.HALF:
        wide = _run(c, widen=True)                              # f_st(x_half) == round(f(float(x_half))), rounded once by torch
        assert wide.dtype == torch.float32
        assert torch.equal(wide.to(got.dtype).view(torch.uint8), got.view(torch.uint8)), "the %s launch is not the fp32 launch rounded once" % C.branch_of(c)


def test_empty_calls_return_without_a_launch():
    from ppst_amd import ops
    k = torch.ones(3, 3, device=_dev())
    for dt in (torch.float32, torch.float16, torch.float64):
        y = ops.upfirdn2d_raw(torch.empty(0, 5, 6, 4, device=_dev(), dtype=dt), k, 1, 1, 1, 1, 1, 1, 1, 1)
        assert tuple(y.shape) == (0, 5, 6, 4) and y.dtype == dt
        y = ops.fused_bias_act_raw(torch.empty(0, 3, 4, device=_dev(), dtype=dt), torch.ones(3, device=_dev(), dtype=dt), None, 3, 0, 0.2, 1.0)
        assert tuple(y.shape) == (0, 3, 4) and y.dtype == dt
    torch.cuda.synchronize()


def test_refusals_leave_the_output_untouched():
    from ppst_amd import ops
    lib, p_, s_ = ops.lib, ops._p, ops._stream
    dev = _dev()

    def fir(x, k, y, kh, kw, up=1, dtype=0):
        M, H, W, Cc = x.shape
        return lib.ppst_upfirdn2d(p_(x), p_(k), p_(y), M, H, W, Cc, kh, kw, up, up, 1, 1, 4, 4, 4, 4, dtype, s_())

    x = torch.ones(2, 6, 7, 4, device=dev)
    y = torch.full((2 * 32 * 32 * 4,), 7.0, device=dev)
    k9 = torch.ones(9, 9, device=dev)
    assert fir(x, k9, y, 9, 9) != 0, "kh > 8 accepted"
    assert fir(x, k9, y, 3, 3, up=0) != 0 and fir(x, k9, y, 3, 3, up=-1) != 0, "up <= 0 accepted"
    with pytest.raises(RuntimeError, match="ppst_upfirdn2d"):
        ops.upfirdn2d_raw(x, k9, 1, 1, 1, 1, 4, 4, 4, 4)
    xh = torch.ones(2 * 6 * 7 * 4 + 8, device=dev, dtype=torch.float16)
    yh = torch.full((2 * 32 * 32 * 4,), 7.0, device=dev, dtype=torch.float16)
    for xo, yo in ((1, 0), (0, 1), (2, 2)):                      # 2 and 4 bytes off the 8-byte grid, either pointer
        assert fir(xh[xo:xo + 336].view(2, 6, 7, 4), k9, yh[yo:], 3, 3, dtype=1) != 0, "a half pointer off the 8-byte grid accepted"
    n = x.numel()
    b = torch.ones(6, device=dev)

    def fba(grad=0, step_b=28, bias=b):
        return lib.ppst_fused_bias_act(p_(x), p_(bias), None, p_(y), n, step_b, 6, 3, grad, 0.2, 1.0, 0, s_())
    assert fba(grad=3) != 0 and fba(grad=-1) != 0, "grad outside 0..2 accepted"
    assert fba(step_b=0) != 0 and fba(step_b=-4) != 0, "step_b <= 0 with a bias accepted"
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()) and bool((yh == 7.0).all()), "a refused call wrote"
    assert fba(step_b=0, bias=None) == 0                         # (without a bias step_b is not read)
    torch.cuda.synchronize()
    assert bool((y[:n] == x.reshape(-1)).all()) and bool((y[n:] == 7.0).all())


def test_blur_nhwc_refuses_an_fp32_tensor_off_the_16_byte_grid():
    """ppst_blur_nhwc_st has float4 forms only: a 4-byte-offset view is refused (ppst_upfirdn2d sends the same geometry to its generic
    kernel: the -off1 cases of the table), nothing is written, and the aligned call on the same values runs"""
    from ppst_amd import ops
    g = torch.Generator().manual_seed(5)
    src = torch.randn(2, 7, 10, 4, generator=g)
    _, x = _place(src.shape, torch.float32, 1, src)
    k = torch.randn(3, 3, generator=g).to(_dev())
    assert x.data_ptr() % 16 == 4
    with pytest.raises(RuntimeError, match="ppst_blur_nhwc"):
        ops.blur_nhwc(x, k, 1, 1)
    y, hw = ops.blur_nhwc(x.clone(), k, 1, 1)
    want = C.upfirdn_ref(src, k.cpu(), (1, 1), (1, 1), (1, 1, 1, 1)).numpy()
    bad, _ = C.compare(want, _np(y), C.BAR_EW)
    assert tuple(hw) == (7, 10) and not bad, bad


# ------------------------------------------------------------------------------- adjoints against float64 autograd of the reference
def _ref_nchw(x, k, up, down, pad):
    N, Cc, H, W = x.shape
    y = C.upfirdn_ref(x.reshape(N * Cc, H, W, 1), k, (up, up), (down, down), (pad[0], pad[1], pad[0], pad[1]), x.dtype)
    return y.reshape(N, Cc, y.shape[1], y.shape[2])


def _orders(fn, x, gy, v):
    """-> (y, d<y, gy>/dx, d<that, v>/d gy) of a differentiable fn"""
    x, gy = x.detach().clone().requires_grad_(True), gy.detach().clone().requires_grad_(True)
    y = fn(x)
    gx, = torch.autograd.grad(y, x, gy, create_graph=True)
    gg, = torch.autograd.grad((gx * v).sum(), gy)
    return y.detach(), gx.detach(), gg.detach()


_ADJ = [
    ("planes-k3", "f32", (3, 3), 1, 1, (1, 1), (9, 11)), ("planes-k4", "f32", (4, 4), 1, 1, (2, 1), (8, 9)),
    ("planes-k3-crop", "f32", (3, 3), 1, 1, (-1, -1), (9, 11)), ("generic-up2", "f32", (4, 4), 2, 1, (2, 1), (8, 9)),
    ("generic-down2", "f32", (4, 4), 1, 2, (1, 1), (9, 8)), ("generic-up2-crop", "f32", (3, 3), 2, 1, (-1, 2), (9, 8)),
    ("f64-up2", "f64", (3, 3), 2, 1, (2, 1), (6, 5)), ("f64-down2-crop", "f64", (4, 4), 1, 2, (-1, 3), (9, 8))]


@pytest.mark.parametrize("name,dt,ks,up,down,pad,hw", _ADJ, ids=[a[0] for a in _ADJ])
def test_upfirdn2d_first_and_second_order(name, dt, ks, up, down, pad, hw):
    """the public NCHW op: its gradient is the op again with the flipped taps, up and down exchanged and fir._adjoint_pad's pads (up 2 /
    down 1 and its reverse are each other's adjoint), so d/dx and the second-order term d<d/dx, v>/d(gy) run the forms of the table"""
    from ppst_amd.stylegan2_op import upfirdn2d
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    x = torch.randn(2, 3, *hw, generator=g, dtype=f64)
    k = torch.randn(*ks, generator=g, dtype=f64)
    tdt = C.TD[dt]
    x, k = x.to(tdt).double(), k.to(tdt).double()               # (the operands as stored)
    ref_fn = lambda d: (lambda t: _ref_nchw(t, k.to(d), up, down, pad))
    y0 = ref_fn(f64)(x)
    gy, v = torch.randn(y0.shape, generator=g, dtype=f64).to(tdt).double(), torch.randn(x.shape, generator=g, dtype=f64).to(tdt).double()
    want = _orders(ref_fn(f64), x, gy, v)
    kd = k.to(tdt).to(_dev())
    got = _orders(lambda t: upfirdn2d(t, kd, up=up, down=down, pad=pad), x.to(tdt).to(_dev()), gy.to(tdt).to(_dev()), v.to(tdt).to(_dev()))
    if dt == "f64":
        ka = k.abs()
        lim = _orders(lambda t: _ref_nchw(t, ka, up, down, pad), x.abs(), gy.abs(), v.abs())
    else:
        w32 = _orders(ref_fn(torch.float32), x.float(), gy.float(), v.float())
    for i, what in enumerate(("forward", "d/dx", "second order")):
        r, a = want[i].numpy(), _np(got[i])
        assert got[i].dtype == tdt
        if dt == "f64":
            allowed = 2.0 * (ks[0] * ks[1] + 1) * 2.0 ** -53 * lim[i].numpy()
            assert (np.abs(a - r) <= allowed).all(), "%s %s: outside the float64 bound, worst %.2f x" % (name, what, (np.abs(a - r) / np.maximum(allowed, 1e-300)).max())
        else:
            s = np.abs(r).max()
            bar = max(C.BAR_EW, 4.0 * float(np.abs(w32[i].double().numpy() - r).max() / s))
            bad, err = C.compare(r, a, bar)
            print("FIR-ADJ upfirdn2d %-18s %-12s err %.3e bar %.2e" % (name, what, err, bar))
            assert not bad, "%s %s: %s" % (name, what, bad)


@pytest.mark.parametrize("st", ["f32", "f16", "bf16"])
def test_fused_leaky_relu_first_and_second_order(st):
    """y = lrelu(x + b) sqrt 2; d/dx = g (y > 0 ? 1 : 0.2) sqrt 2 gated by the saved OUTPUT (mode 31), d/db its sum over all but dim 1, and the
    second-order term the same diagonal map.  The gate is taken from the device's own output (as gstep_diag.check_block does): an
    element within rounding of 0 may fall on either side, and every value is then held to float64."""
    from ppst_amd.stylegan2_op import fused_leaky_relu
    dt = C.TD[st]
    g = torch.Generator().manual_seed(17)
    rn = lambda *s: torch.randn(*s, generator=g).to(dt)
    x, b = rn(3, 6, 5, 7), rn(6)
    x = C._fix_gate(x.float(), lambda t: t + b.float().view(1, -1, 1, 1), st).to(dt)
    gy, v = rn(3, 6, 5, 7), rn(3, 6, 5, 7)
    xd, bd = x.to(_dev()).requires_grad_(True), b.to(_dev()).requires_grad_(True)
    gyd = gy.to(_dev()).requires_grad_(True)
    y = fused_leaky_relu(xd, bd)
    gx, gb = torch.autograd.grad(y, [xd, bd], gyd, create_graph=True)
    gg, = torch.autograd.grad((gx * v.to(_dev())).sum(), gyd)
    assert y.dtype == gx.dtype == gg.dtype == gb.dtype == dt
    al, sc = float(np.float32(0.2)), float(np.float32(2 ** 0.5))        # (they cross the ABI as C floats)
    z = x.double() + b.double().view(1, -1, 1, 1)
    gate = y.detach().double().cpu() > 0
    assert bool((gate == (z > 0)).all()), "the device's output has the wrong sign somewhere (|x + b| >= 1e-3)"
    wants = {"forward": torch.where(gate, z, z * al) * sc, "d/dx": torch.where(gate, gy.double(), gy.double() * al) * sc,
             "second order": torch.where(gate, v.double(), v.double() * al) * sc}
    for (what, r), a in zip(wants.items(), (y, gx, gg)):
        r, a = r.numpy(), _np(a)
        if st == "f32":
            bad, err = C.compare(r, a, C.BAR_EW)
        else:
            bad, err = C.A.compare_half(r, a, C.BAR_EW, st)
        print("FIR-ADJ fused_leaky_relu %-5s %-12s err %.3e" % (st, what, err))
        assert not bad, "%s %s: %s" % (st, what, bad)
    # the bias gradient: torch's sum of the stored d/dx (fp32 accumulation), rounded once to the bias's type.  Allowed: the class
    # bar of a sum (BAR_SUM of tests/bwd_cases.py) on max|ref| plus, in a half type, one rounding of every term and of the sum
    r = wants["d/dx"].sum((0, 2, 3)).numpy()
    allowed = 1e-5 * np.abs(r).max() + (2.0 ** -C.A.PBITS[st] * (wants["d/dx"].abs().sum((0, 2, 3)).numpy() + np.abs(r)) if st != "f32" else 0.0)
    assert (np.abs(_np(gb) - r) <= allowed).all(), (st, np.abs(_np(gb) - r) / allowed)


_BLOCKS = [("k4-zero-p11", (1, 3, 3, 1), 1, 1, 0), ("k4-zero-p22", (1, 3, 3, 1), 2, 2, 0), ("k3-reflect-p21", (1, 2, 1), 2, 1, 1), ("k3-zero-p10", (1, 2, 1), 1, 0, 0)]


def _taps(t):
    k = torch.tensor(t, dtype=f64)
    k = k[:, None] * k[None, :]
    return k / k.sum()


def _rel(got, want):
    return float((got.double().cpu() - want).abs().max() / want.abs().max())


@pytest.mark.parametrize("hw", [(8, 9), (9, 8), (9, 13)], ids=lambda t: "%dx%d" % t)
@pytest.mark.parametrize("tag,taps,p0,p1,mode", _BLOCKS, ids=[b[0] for b in _BLOCKS])
def test_blur_blocks_of_the_train_step(tag, taps, p0, p1, mode, hw):
    """autograd.BlurDownFn (zero padding) and the input gradient of autograd.blur_conv with the taps and pads the networks use, at
    extents that are no multiple of anything (gstep_diag.t_blocks takes them at 32 x 40 only); tolerances: check_block's 5e-6 and 3e-5"""
    import gstep_diag as D
    from ppst_amd import autograd as A
    g = torch.Generator().manual_seed(hw[0] * 100 + hw[1] + p0)
    k = _taps(taps)
    x = torch.randn(2, 32, *hw, generator=g)
    if mode == 0:
        net = D.MiniNet(k=k.float())
        xd = D.nhwc(x).to(_dev()).requires_grad_(True)
        y = A.BlurDownFn.apply(xd, net, "k", p0, p1)
        xr = x.double().requires_grad_(True)
        yr = _ref_nchw(xr, k, 1, 2, (p0, p1))
        gr = torch.randn(yr.shape, generator=g, dtype=f64)
        gx, = torch.autograd.grad(y, xd, D.nhwc(gr).float().to(_dev()))
        gxr, = torch.autograd.grad(yr, xr, gr)
        e = (_rel(D.nchw(y.detach()), yr.detach()), _rel(D.nchw(gx), gxr))
        print("FIR-ADJ BlurDownFn %-14s %dx%d fwd %.3e d/dx %.3e" % (tag, hw[0], hw[1], e[0], e[1]))
        assert max(e) <= 5e-6, e
    if (tag, mode) in (("k4-zero-p22", 0), ("k3-reflect-p21", 1)):
        w, b = torch.randn(64, 32, 3, 3, generator=g) * 0.1, torch.randn(64, generator=g) * 0.1
        net = D.MiniNet(w=w, k=k.float())
        pm = A.REFLECT if mode else A.Z
        xd = D.nhwc(x).to(_dev()).requires_grad_(True)
        y = A.blur_conv(xd, net.p("w"), net, "w", "k", bias=b.to(_dev()), scale=0.6, p0=p0, p1=p1, pad_mode=pm, act=A.LRELU)
        xr = x.double().requires_grad_(True)
        xb = _ref_nchw(F.pad(xr, (p0, p1, p0, p1), mode="reflect"), k, 1, 1, (0, 0)) if mode else _ref_nchw(xr, k, 1, 1, (p0, p1))
        gate = D.nchw(y.detach()).double().cpu()
        yr = D.lrelu_gated(F.conv2d(xb, w.double() * 0.6, stride=2), b.double(), gate)
        gr = torch.randn(yr.shape, generator=g, dtype=f64)
        gx, = torch.autograd.grad(y, xd, D.nhwc(gr).float().to(_dev()))
        gxr, = torch.autograd.grad(yr, xr, gr)
        e = (_rel(D.nchw(y.detach()), yr.detach()), _rel(D.nchw(gx), gxr))
        print("FIR-ADJ blur_conv  %-14s %dx%d fwd %.3e d/dx %.3e" % (tag, hw[0], hw[1], e[0], e[1]))
        assert max(e) <= 3e-5, e
    torch.cuda.synchronize()
