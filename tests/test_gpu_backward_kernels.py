"""GPU: the backward kernels of csrc/train.hip and csrc/train_g.hip, called through the ppst_amd.ops entry points on every case of
tests/bwd_cases.py and compared with its float64 reference -- pytest -m gpu.  The device is never its own judge.

Each case names the kernel family its launcher picks (bwd_cases.branch_of restates the launcher's condition; printed with the
error, pytest -s shows the table); tests/test_backward_cases_cpu.py shows on the CPU that the references are right, that every
family has a case and that the comparison used here, at the bar used here, rejects a dropped border row, a tie sent to the last
pixel, a dropped ragged tail, an ignored slice offset, an overwriting accumulate, zero scalar-tail channels and zero batch rows
17.. on these very inputs.

Next to the references: the adjoint identity <op(x), dy> = <x, op_bwd(dy)> of the linear pairs (float64 on the host, from the
device's outputs), bit-identical repeats of every kernel without float atomics, a batch equal to its single-image calls, and
guard values around the outputs the caller places (out= destinations, the in-place softmax gradient, and dx reached through the
C entry with dx_ld > C).  Outputs that ops allocates itself sit in the allocator's blocks and carry no guard.

The half-storage (`_st`) instances run through the same path: the operands a launcher types travel as float16 / bfloat16 (the case's
``st``), a half-stored output is judged by the half rule of bwd_cases, and where the fp32 launch takes the same kernel form the half
launch must equal it, rounded once, bit for bit.  What a half tensor may not be is refused through the C entries, nothing written.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bwd_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu
POISON = 12345.0


def _dev():
    return torch.device("cuda", 0)


def _dt(c, name):
    """the type an operand travels in: the case's storage type for the operands its launcher types (C.TYPED), else float32.  (The
    case's float32 values are exactly the stored ones: the conversion rounds nothing.)"""
    return C.DTYPE[C.st_of(c)] if name in C.TYPED.get(c.op, ()) else torch.float32


def _whole(c, inp, name):
    return inp[name].to(_dev()).to(_dt(c, name))


def _put(c, inp, name, C_=None):
    """the operand on the device, as the case stores it: the channel slice of the wider tensor (a view: ld and offset kept)"""
    t = _whole(c, inp, name)
    C_ = c.p["C"] if C_ is None else C_
    off = c.p.get(name + "_off", 0)
    return t[..., off:off + C_] if t.shape[-1] != C_ else t


def _np(t):
    return t.detach().double().cpu().numpy()


def _guarded(shape, fill=None, dtype=torch.float32):
    """a contiguous tensor of ``shape`` and ``dtype`` inside a larger buffer the test owns, POISON before and after; -> (view, check)
    (256 elements in front: the view starts 512 or 1024 bytes in, aligned for every launcher)"""
    n = int(np.prod(shape))
    buf = torch.full((n + 512,), POISON, device=_dev(), dtype=dtype)
    view = buf[256:256 + n].view(*shape)
    if fill is not None:
        view.copy_(fill)

    poison = torch.full((1,), POISON, device=_dev(), dtype=dtype)        # (POISON as the buffer's type holds it)

    def check():
        assert bool((buf[:256] == poison).all()) and bool((buf[256 + n:] == poison).all()), "wrote outside its output"
    return view, check


# ------------------------------------------------------------------------------------------------------------- runners
def _run_bilinear_bwd(c, inp, ops):
    return {"dx": ops.bilinear_bwd(_put(c, inp, "dy"), c.p["H"], c.p["W"])}


def _run_pad2d(c, inp, ops):
    p = c.p
    return {"y": ops.pad2d(_put(c, inp, "x"), *p["pads"], p["mode"]), "dx": ops.pad2d_bwd(_whole(c, inp, "dy"), *p["pads"], p["mode"])}


def _run_avgpool_bwd(c, inp, ops):
    return {"dx": ops.avgpool_bwd(_put(c, inp, "dy"), c.p["f"])}


def _run_gap_gmp_bwd(c, inp, ops):
    dev = _dev()
    mask = inp["mask"].to(dev) if "mask" in inp else None
    out, check = (None, lambda: None)
    if "out0" in inp:        # (the buffer added into has x's storage type: a half out= sits between POISON values of that type)
        out, check = _guarded(inp["out0"].shape, _whole(c, inp, "out0"), _dt(c, "out0"))
    dx = ops.gap_gmp_bwd(_put(c, inp, "x"), mask, inp["v"].to(dev), inp["g"].to(dev), out=out)
    torch.cuda.synchronize()
    check()
    return {"dx": dx}


def _run_gap_gmp_multi_bwd(c, inp, ops):
    dev = _dev()
    out, check = (None, lambda: None)
    if "out0" in inp:
        out, check = _guarded(inp["out0"].shape, _whole(c, inp, "out0"), _dt(c, "out0"))
    dx = ops.gap_gmp_multi_bwd(_put(c, inp, "x"), inp["masks"].to(dev), inp["v"].to(dev), inp["g"].to(dev), with_plain=c.p["plain"], out=out)
    torch.cuda.synchronize()
    check()
    return {"dx": dx}


def _run_colsum(c, inp, ops):
    out, check = _guarded((c.p["C"],), inp["out0"].to(_dev()) if "out0" in inp else None)
    r = ops.colsum(_put(c, inp, "x"), scale=c.p.get("scale", 1.0), out=out, accumulate="out0" in inp)
    torch.cuda.synchronize()
    check()
    return {"out": r}


def _run_linear(c, inp, ops):
    dev, p = _dev(), c.p
    s = p.get("scale", 1.0)
    dy, w, x, gate = (inp[k].to(dev) for k in ("dy", "w", "x", "gate"))
    acc = bool(p.get("acc"))
    fresh = lambda k: inp[k].to(dev).clone() if acc else None
    out = {"dx": ops.linear_dgrad(dy, w, s), "dx_gate": ops.linear_dgrad_gate(dy, w, gate, s),
           "dw": ops.linear_wgrad(dy, x, s, out=fresh("dw0"), accumulate=acc)}
    if p["K"] % 4 == 0:
        dwf, check = _guarded((p["N"], p["K"]), inp["dw0"].to(dev) if acc else None)
        out["dw_fused"], out["db"] = ops.linear_wgrad_fused(dy, x, s, out=dwf, accumulate=acc, relu_in=bool(p.get("relu_in")), bias_out=fresh("db0"),
                                                            bias_scale=p.get("bscale", 1.0), bias_accumulate=acc, want_bias=True)
        torch.cuda.synchronize()
        check()
    return out


def _run_noise_wgrad(c, inp, ops):
    out, check = _guarded((1,), inp["out0"].to(_dev()) if "out0" in inp else None)
    r = ops.noise_wgrad(_put(c, inp, "dpre"), inp["noise"].to(_dev()), out=out, accumulate="out0" in inp)
    torch.cuda.synchronize()
    check()
    return {"out": r}


def _run_wgrad_small_cin(c, inp, ops):
    p = c.p
    out, check = _guarded((p["cout"], p["cin"], 1, 1), inp["out0"].to(_dev()) if "out0" in inp else None)
    r = ops.wgrad_small_cin(_put(c, inp, "x", p["cin"]), _whole(c, inp, "dy"), p.get("scale", 1.0), out=out, accumulate="out0" in inp)
    torch.cuda.synchronize()
    check()
    return {"dw": r.view(p["cout"], p["cin"], 1, 1)}


def _run_l2norm_rows_bwd(c, inp, ops):
    return {"dx": ops.l2norm_rows_bwd(inp["g"].to(_dev()), inp["x"].to(_dev()), c.p["eps"], c.p["mode"])}


def _run_softmax_rows_bwd_(c, inp, ops):
    g, check = _guarded(inp["g"].shape, inp["g"].to(_dev()))
    r = ops.softmax_rows_bwd_(inp["p"].to(_dev()), g, c.p["div"])
    torch.cuda.synchronize()
    check()
    return {"g": r}


def _run_corr_prep_bwd(c, inp, ops):
    return {"dx": ops.corr_prep_bwd(inp["g"].to(_dev()), inp["x"].to(_dev()), c.p["ncenter"])}


def _run_l1(c, inp, ops):
    a, b = inp["a"].to(_dev()), inp["b"].to(_dev())
    return {"grad": ops.l1_grad(a, b, c.p["weight"]), "loss": ops.l1_mean(a, b, c.p["weight"])}


def _run_prelu_bwd(c, inp, ops):
    dev = _dev()
    gpre, ds = ops.prelu_bwd(_put(c, inp, "g"), _put(c, inp, "y"), inp["prelu"].to(dev), inp["ss"].to(dev) if "ss" in inp else None,
                             _put(c, inp, "res") if "res" in inp else None)
    return {"gpre": gpre, "dslope": ds}


def _run_in_bwd(c, inp, ops):
    dev, p = _dev(), c.p
    g, y = _put(c, inp, "g"), _put(c, inp, "y")
    gate = _put(c, inp, "gate") if "gate" in inp else None
    part = ops.dual_stats(g, y, gate)
    out = {"sums": part.double().sum(1)}                 # (the chunks' partial sums, added on the host in float64)
    style = inp["style"].to(dev) if "style" in inp else None
    if not p.get("norm", True):
        out["dstyle"] = ops.in_bwd_finalize(part, p["hw"], None)[1]
        return out
    coef, dstyle = ops.in_bwd_finalize(part, p["hw"], inp["mr"].to(dev), style, want_dstyle=bool(p.get("want_dstyle")))
    out["dx"] = ops.in_bwd_apply(g, y, coef, gate, post_gate=bool(p.get("post_gate")))
    if p.get("want_dstyle"):
        out["dstyle"] = dstyle
    return out


def _run_in_finalize_train(c, inp, ops):
    dev = _dev()
    ss, mr = ops.in_finalize_train(inp["partial"].to(dev), c.p["n"] * c.p["per"], inp["style"].to(dev) if "style" in inp else None,
                                   inp["post_bias"].to(dev))
    return {"ss": ss, "mr": mr}


def _run_lsgan(c, inp, ops):
    loss, grad = ops.lsgan(inp["pred"].to(_dev()), c.p["target"], c.p["weight"])
    return {"loss": loss, "grad": grad}


def _run_rscl(c, inp, ops):
    q, k, k0, queue, gout = (inp[n].to(_dev()) for n in ("q", "k", "k0", "queue", "gout"))
    return {"loss": ops.rscl_loss(q, k, k0, queue, 0.07), "dq": ops.rscl_loss_bwd(q, k, k0, queue, gout, 0.07)}


def _run_rselfcorr_bwd(c, inp, ops):
    return {"dfea": ops.rselfcorr_bwd(inp["fea"].to(_dev()), _put(c, inp, "dout", 256))}


def _run_unfold_rows_bwd(c, inp, ops):
    p = c.p
    return {"dx": ops.unfold_rows_bwd(inp["g"].to(_dev()), (p["B"], p["H"], p["W"], p["C"]), p["k"])}


def _run_upscale_weight_bwd(c, inp, ops):
    p = c.p
    out, check = _guarded((p["cout"], p["cin"], 3, 3), inp["out0"].to(_dev()) if "out0" in inp else None)
    r = ops.upscale_weight_bwd(inp["dw4"].to(_dev()), p["cout"], p["cin"], p["scale"], out=out, accumulate="out0" in inp)
    torch.cuda.synchronize()
    check()
    return {"dw": r}


def _run_scale_by(c, inp, ops):
    return {"y": ops.scale_by(inp["x"].to(_dev()), inp["s"].to(_dev()))}


def _run_transpose_last2(c, inp, ops):
    return {"y": ops.transpose_last2(inp["x"].to(_dev()))}


def _run_space_to_depth(c, inp, ops):
    s = ops.space_to_depth(_put(c, inp, "x"))
    return {"s": s, "back": ops.depth_to_space(s, (c.p["H"], c.p["W"]))} if c.p["C"] % 8 == 0 else {"s": s}


def _run_conv_wgrad(c, inp, ops):
    dev, p = _dev(), c.p
    kind = p.get("kind", "conv")
    xc, dc = C._cw_chan(c)
    plan = ops.ConvPlan(inp["w"].to(dev), kind, scale=p["scale"], precision=p["prec"])
    acc = bool(p.get("acc"))
    wshape = C._cw_wshape(c)
    out, check = _guarded(wshape, inp["dw0"].to(dev) if acc else None)             # (not accumulated into: it starts as POISON)
    bias_out = None
    if "db0" in inp and p.get("bias"):
        bias_out = inp["db0"].to(dev).clone() if C._cw_bias_acc(c) else torch.full((p["cout"],), POISON, device=dev)
    r = ops.conv_wgrad(plan, _put(c, inp, "x", xc), _put(c, inp, "dy", dc), splits=p.get("splits"), out=out, accumulate=acc,
                       bias_out=bias_out, bias_accumulate=C._cw_bias_acc(c), want_bias=bool(p.get("bias")), dy_scale=p.get("dy_scale", 1.0))
    torch.cuda.synchronize()
    check()
    dw, db = r if isinstance(r, tuple) else (r, None)
    res = {"dw": dw.view(wshape)}
    if p.get("bias"):
        res["db"] = db
    if kind == "dgradT" and not acc:       # the parameter's gradient, as ConvFn.backward takes it from the blurred kernel's
        res["dw3"] = ops.upscale_weight_bwd(dw, plan.cin, plan.cout, plan.fwd_scale)
    return res


def _wgrad_p1(c, inp, ops, dtype):
    """ops.conv_wgrad in precision mode 1 on operands stored as ``dtype`` (the case's values are bfloat16-representable)"""
    dev, p = _dev(), c.p
    xc, dc = C._cw_chan(c)
    prev = ops.PRECISION["value"]
    ops.set_precision(1)
    try:
        plan = ops.ConvPlan(inp["w"].to(dev), p.get("kind", "conv"), scale=p["scale"], precision=1)
        r = ops.conv_wgrad(plan, _put(c, inp, "x", xc).to(dtype), _put(c, inp, "dy", dc).to(dtype), splits=p.get("splits"),
                           want_bias=bool(p.get("bias")))
        torch.cuda.synchronize()
    finally:
        ops.set_precision(prev)
    dw, db = r if isinstance(r, tuple) else (r, None)
    res = {"dw": dw.view(C._cw_wshape(c))}
    if p.get("bias"):
        res["db"] = db
    return res


def _run_conv_wgrad_p1(c, inp, ops):
    return _wgrad_p1(c, inp, ops, torch.float32)           # single pass on fp32 tiles: the form the float64 table judges


class _OneWeightNet:
    """what ops.dgrad_s2d asks of a network: the parameter and its plans"""

    def __init__(self, w, ops, prec):
        self.w, self.ops, self.prec = w, ops, prec

    def p(self, name):
        return self.w

    def plan(self, name, kind, scale):
        return self.ops.ConvPlan(self.w, kind, scale=scale, precision=self.prec)


def _run_conv_dgrad(c, inp, ops):
    dev, p = _dev(), c.p
    w, g = inp["w"].to(dev), _put(c, inp, "g", p["cout"])
    if p.get("via") == "entry":
        return {"dx": ops.dgrad_s2d(_OneWeightNet(w, ops, p["prec"]), "w", p["scale"], g, p["bhw"])}
    plan = ops.ConvPlan(w, p["kind"], scale=p["scale"], precision=p["prec"])
    if p["kind"] == "dgrad":
        return {"dx": plan(g)}
    if p["kind"] == "dgrad_s2d":
        return {"dx": plan(g, out_hw=p["bhw"])}
    ys = plan(g, out_hw=((p["bhw"][0] + 1) // 2, (p["bhw"][1] + 1) // 2))
    return {"dx": ops.depth_to_space(ys, p["bhw"])}


RUN = {k[5:]: v for k, v in list(globals().items()) if k.startswith("_run_")}
ATOMIC = {"bilinear_bwd:scatter"}          # float atomics: equal to the reference within the bar, not bit for bit between runs


def _run(c, inp=None, raw=False):
    from ppst_amd import ops
    out = RUN[c.op](c, C.inputs(c.id) if inp is None else inp, ops)
    torch.cuda.synchronize()
    return out if raw else {k: _np(v) for k, v in out.items()}


# --------------------------------------------------------------------------------------------- against the float64 reference
@pytest.mark.parametrize("cid", [c.id for c in C.CASES])
def test_against_float64_reference(cid):
    c = C.by_id(cid)
    ref, raw = C.reference(cid), _run(c, raw=True)
    got = {k: _np(v) for k, v in raw.items()}
    assert set(got) == set(ref)
    fails = []
    for k in sorted(ref):
        b, st = C.bar(c, k), C.out_st(c, k)
        if C.st_of(c) != "f32":          # the activation-shaped outputs take the case's type, every sum stays fp32
            assert raw[k].dtype == (C.DTYPE[st] if c.op != "conv_dgrad" else torch.bfloat16) or (st == "f32" and k == "sums"), (k, raw[k].dtype)
        bad, err = C.judge(c, k, got[k])
        # (a half-stored output: err in units of the allowed error b s + 2^-p (|ref| + b s), <= 1 passes)
        print("%-58s %-9s err %.2e%s  bar %.2e  %s" % (cid, k, err, " x allowed (%s)" % st if (st != "f32" and b) else "", b, C.branch_of(c)))
        fails += ["%s: %s" % (k, m) for m in bad]
    if c.op in ("gap_gmp_bwd", "gap_gmp_multi_bwd") and not c.p.get("acc"):
        # the routed term is exact: where no gradient arrives the kernel writes 0, bit for bit
        assert np.all(got["dx"][ref["dx"] == 0] == 0), "non-zero values where the reference is 0"
    if c.op == "pad2d" and c.p["mode"]:
        once = C.pad_count(c.p["H"], c.p["W"], c.p["pads"], c.p["mode"]) <= 1       # interior of reflect / replicate: a copy
        assert np.array_equal(got["dx"][:, once], ref["dx"][:, once].astype(np.float32)), "the interior of the gradient is not a copy"
    assert not fails, "%s [%s]: %s" % (cid, C.branch_of(c), "; ".join(fails))
    if C.branch_of(c) not in ATOMIC:
        again = _run(c)
        for k in got:
            assert np.array_equal(again[k], got[k]), "%s: two runs differ" % k


# --------------------------------------------------------------------- a half launch is the fp32 launch, rounded once
HALF_SAME_FORM = [c.id for c in C.CASES if C.st_of(c) != "f32" and C.same_form_as_f32(c)]


@pytest.mark.parametrize("cid", HALF_SAME_FORM)
def test_half_launch_is_the_fp32_launch_rounded_once(cid):
    """the 2^-p of the half rule cannot see a double rounding or a half-precision accumulator: where the fp32 launch takes the same
    kernel form (bwd_cases.same_form_as_f32), the half launch equals it on the widened operands bit for bit -- statistics and
    parameter gradients as they are, activation-shaped outputs after ONE rounding of the fp32 result (common.h; what
    gpu_diag.t_train_half asks at its one shape)"""
    c = C.by_id(cid)
    half, wide = _run(c, raw=True), _run(C.as_f32(c), C.inputs(cid), raw=True)
    assert set(half) == set(wide)
    for k in sorted(half):
        st = C.out_st(c, k)
        want = wide[k].to(C.DTYPE[st]) if st != "f32" else wide[k]
        assert half[k].dtype == want.dtype and wide[k].dtype != C.DTYPE[C.st_of(c)], (k, half[k].dtype, wide[k].dtype)
        same = torch.equal(half[k], want)
        print("%-58s %-9s %s == fp32 launch%s: %s" % (cid, k, C.st_of(c), " rounded once" if st != "f32" else "", same))
        assert same, "%s: %d values differ from the fp32 launch%s, max %.3e" % (
            k, int((half[k] != want).sum()), " rounded once" if st != "f32" else "", float((half[k].double() - want.double()).abs().max()))


# ------------------------------------------------------------------------- the weight gradient's two single-pass operand forms
@pytest.mark.parametrize("cid", [c.id for c in C.CASES if c.op == "conv_wgrad_p1"])
def test_wgrad_single_pass_forms_against_float64_and_each_other(cid):
    """precision mode 1 on bfloat16-representable operands: fp32 storage (conv_wgrad_tr2_kernel, one pass on fp32 tiles) against
    float64 at the case's bar; bf16 storage (conv_wgrad_tr2b_kernel) against the fp32-storage result at C.STORAGE_BAR"""
    from ppst_amd import ops
    c, inp = C.by_id(cid), C.inputs(cid)
    ref = C.reference(cid)
    f32 = {k: _np(v) for k, v in _wgrad_p1(c, inp, ops, torch.float32).items()}
    b16 = {k: _np(v) for k, v in _wgrad_p1(c, inp, ops, torch.bfloat16).items()}
    assert set(f32) == set(b16) == set(ref)
    fails = []
    for k in sorted(ref):
        bad, err = C.judge(c, k, f32[k])
        bad2, err2 = C.storage_violations(f32[k], b16[k])
        print("%-58s %-3s fp32-stored vs float64 %.2e (bar %.2e)  bf16-stored vs fp32-stored %.2e (bar %.0e) bit-equal %s  %s"
              % (cid, k, err, C.bar(c, k), err2, C.STORAGE_BAR, np.array_equal(f32[k], b16[k]), C.branch_of(c)))
        fails += ["%s fp32-stored: %s" % (k, m) for m in bad] + ["%s bf16-stored: %s" % (k, m) for m in bad2]
    assert not fails, "%s [%s]: %s" % (cid, C.branch_of(c), "; ".join(fails))


# ------------------------------------------------------------------------------------------------------ adjoint identities
def _adjoint(y, dy, x, dx, bar):
    """<y, dy> = <x, dx> in float64 on the host; each side carries the kernels' relative error bar on every product"""
    lhs, rhs = float((y.double() * dy.double()).sum()), float((x.double() * dx.double()).sum())
    tol = bar * float((y.double() * dy.double()).abs().sum() + (x.double() * dx.double()).abs().sum())
    print("adjoint: %.9e vs %.9e (tolerance %.1e)" % (lhs, rhs, tol))
    assert abs(lhs - rhs) <= tol, (lhs, rhs, tol)


# (the forwards ppst_bilinear and ppst_avgpool take C % 4 == 0 only: the adjoint of the scalar backward forms has no forward to meet)
def _adjoint_bar(c):
    """fp32: the elementwise class bar; a half case: the half rule's relative term 2^-p (each output is rounded once to its type)"""
    return C.BAR_EW if C.st_of(c) == "f32" else 2.0 ** -C.PBITS[C.st_of(c)]


# (one half case each: the outputs are widened to float64 on the host)
@pytest.mark.parametrize("c", [c for c in C.CASES if c.op == "bilinear_bwd" and not c.p.get("dy_off") and c.p["C"] % 4 == 0
                               and (C.st_of(c) == "f32" or c.id == "bilinear_bwd-bf16-C8-5x7-to-12x9")], ids=lambda c: c.id)
def test_bilinear_pair_is_adjoint(c):
    from ppst_amd import ops
    inp = C.inputs(c.id)
    x, dy = _whole(c, inp, "x"), _whole(c, inp, "dy")
    # (the forward is an fp32 kernel: it reads the stored values of x widened)
    _adjoint(ops.bilinear(x.float(), c.p["OH"], c.p["OW"]).cpu(), dy.cpu(), x.cpu(), ops.bilinear_bwd(dy, c.p["H"], c.p["W"]).cpu(), _adjoint_bar(c))


@pytest.mark.parametrize("c", [c for c in C.CASES if c.op == "pad2d" and not c.p.get("x_off")
                               and (C.st_of(c) == "f32" or c.id == "pad2d-f16-reflect-C8-asym")], ids=lambda c: c.id)
def test_pad_pair_is_adjoint(c):
    from ppst_amd import ops
    inp = C.inputs(c.id)
    x, dy = _whole(c, inp, "x"), _whole(c, inp, "dy")
    _adjoint(ops.pad2d(x, *c.p["pads"], c.p["mode"]).cpu(), dy.cpu(), x.cpu(), ops.pad2d_bwd(dy, *c.p["pads"], c.p["mode"]).cpu(), _adjoint_bar(c))


@pytest.mark.parametrize("c", [c for c in C.CASES if c.op == "avgpool_bwd" and not c.p.get("dy_off") and c.p["C"] % 4 == 0], ids=lambda c: c.id)
def test_avgpool_pair_is_adjoint(c):
    from ppst_amd import ops
    p = c.p
    dy = C.inputs(c.id)["dy"].to(_dev())
    x = torch.randn(p["B"], p["oh"] * p["f"], p["ow"] * p["f"], p["C"], generator=torch.Generator().manual_seed(5)).to(_dev())
    _adjoint(ops.avgpool(x, p["f"]).cpu(), dy.cpu(), x.cpu(), ops.avgpool_bwd(dy, p["f"]).cpu(), C.BAR_EW)


@pytest.mark.parametrize("H,W,Cc", [(33, 37, 8), (6, 5, 4), (1, 7, 12)])
def test_space_to_depth_and_depth_to_space_are_adjoint_and_inverse(H, W, Cc):
    """pure data movement: depth_to_space(space_to_depth(x)) is x bit for bit, and <s2d(x), d> = <x, d2s(d)> exactly (every
    product appears once on either side; the padding row / column of an odd extent is dropped by d2s)"""
    from ppst_amd import ops
    g = torch.Generator().manual_seed(H * 100 + W)
    x = torch.randn(2, H, W, Cc, generator=g).to(_dev())
    d = torch.randn(2, (H + 1) // 2, (W + 1) // 2, 4 * Cc, generator=g).to(_dev())
    s = ops.space_to_depth(x)
    assert torch.equal(ops.depth_to_space(s, (H, W)), x)
    want = torch.zeros(2, 2 * ((H + 1) // 2), 2 * ((W + 1) // 2), Cc)
    want[:, :H, :W] = x.cpu()
    want = want.view(2, (H + 1) // 2, 2, (W + 1) // 2, 2, Cc).permute(0, 1, 3, 2, 4, 5).reshape(s.shape)
    assert torch.equal(s.cpu(), want), "space_to_depth is not the phase-major copy"
    lhs, rhs = (s.double() * d.double()).sum().item(), (x.double() * ops.depth_to_space(d, (H, W)).double()).sum().item()
    assert abs(lhs - rhs) <= 1e-12 * (s.double() * d.double()).abs().sum().item()


@pytest.mark.parametrize("st", ["f16", "bf16"])
@pytest.mark.parametrize("H,W", [(33, 37), (6, 5)])
def test_half_space_to_depth_and_depth_to_space_are_adjoint(st, H, W):
    """the 8-byte and 16-byte items of the half forms (the copies themselves: the space_to_depth cases of bwd_cases): every product
    of <s2d(x), d> appears once in <x, d2s(d)>, exactly, in float64 on the host"""
    from ppst_amd import ops
    g = torch.Generator().manual_seed(H * 100 + W)
    x = torch.randn(2, H, W, 8, generator=g).to(_dev()).to(C.HALF[st])
    d = torch.randn(2, (H + 1) // 2, (W + 1) // 2, 32, generator=g).to(_dev()).to(C.HALF[st])
    s, back = ops.space_to_depth(x), ops.depth_to_space(d, (H, W))
    assert s.dtype == back.dtype == C.HALF[st]
    lhs, rhs = (s.double() * d.double()).sum().item(), (x.double() * back.double()).sum().item()
    assert abs(lhs - rhs) <= 1e-12 * (s.double() * d.double()).abs().sum().item()


@pytest.mark.parametrize("Cc,ld,off", [(3, 3, 0), (8, 14, 4), (8, 16, 2)])
def test_space_to_depth_scalar_form_is_the_phase_major_copy(Cc, ld, off):
    """C % 4 != 0, x_ld % 4 != 0 or a pointer off the 16-byte grid: the one-channel-per-thread form of ppst_space_to_depth"""
    from ppst_amd import ops
    wide = torch.randn(2, 5, 7, ld, generator=torch.Generator().manual_seed(Cc + ld + off))
    s = ops.space_to_depth(wide.to(_dev())[..., off:off + Cc])
    assert torch.equal(s.cpu(), C._s2d_stack(wide[..., off:off + Cc].contiguous()))


# -------------------------------------------------------------------------------------------- a batch is its single calls
@pytest.mark.parametrize("cid", ["bilinear_bwd-C4-5x7-to-12x9", "bilinear_bwd-C4-64x64-to-8x8", "avgpool_bwd-f4-C3-16x24", "pad2d-reflect-C8-asym",
                                 "pad2d-replicate-C3-asym", "gap_gmp_bwd-strip-C8-16x12-quant-ties", "gap_gmp_bwd-4e-C8-15x7-quant-ties",
                                 "gap_gmp_bwd-scalar-C6-15x7-quant-ties", "prelu_bwd-C32-ss",
                                 "bilinear_bwd-bf16-C8-5x7-to-12x9", "pad2d-f16-reflect-C8-asym", "gap_gmp_bwd-bf16-strip-C8-16x12-quant-ties"])
def test_batch_equals_single_calls(cid):
    from ppst_amd import ops
    c = C.by_id(cid)
    inp = C.inputs(cid)
    whole = _run(c)
    for b in range(c.p["B"]):
        one = {k: (v[b:b + 1] if (v.dim() > 0 and v.shape[0] == c.p["B"] and k != "prelu") else v) for k, v in inp.items()}
        c1 = c._replace(p=dict(c.p, B=1))
        got = {k: _np(v) for k, v in RUN[c.op](c1, one, ops).items()}
        compared = 0
        for k in got:
            if got[k].shape[0] == 1 and whole[k].shape[0] == c.p["B"]:
                assert np.array_equal(got[k][0], whole[k][b]), "%s: image %d of the batch differs from its single call" % (k, b)
                compared += 1
        assert compared, "no output of %s has a batch axis: nothing was compared" % cid


# ------------------------------------------------------------------------- outputs the entry points place (dx_ld > C): guards
def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


@pytest.mark.parametrize("cid,dx_ld", [("bilinear_bwd-C8-5x7-to-12x9", 12), ("bilinear_bwd-C8-5x7-to-12x9", 10), ("bilinear_bwd-C3-5x7-to-12x9", 5),
                                       ("avgpool_bwd-f2-C3-16x24", 7), ("avgpool_bwd-f4-C32-16x24", 40)])
def test_strided_output_through_the_c_entry_keeps_its_neighbours(cid, dx_ld):
    """ops always passes dx_ld = C; the launchers also take an output that is a channel slice of a wider tensor (dx_ld > C, and
    for bilinear_bwd dx_ld % 4 != 0 sends C % 4 == 0 to the scatter form).  Reached through the C entry: the slice holds the
    reference, the channels beside it and the values before and after the buffer keep their fill."""
    from ppst_amd._lib import lib
    c = C.by_id(cid)
    p, inp, dev = c.p, C.inputs(cid), _dev()
    dy = inp["dy"].to(dev)
    H, W = (p["H"], p["W"]) if c.op == "bilinear_bwd" else (p["oh"] * p["f"], p["ow"] * p["f"])
    wide, check = _guarded((p["B"], H, W, dx_ld), torch.full((p["B"], H, W, dx_ld), POISON))
    off = dx_ld - p["C"] if (dx_ld - p["C"]) % 4 == 0 else 1
    dx = wide[..., off:off + p["C"]]
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    if c.op == "bilinear_bwd":
        dx.zero_()
        rc = lib.ppst_bilinear_bwd(_vp(dy), _vp(dx), p["B"], H, W, p["C"], dx_ld, p["OH"], p["OW"], p["C"], st)
    else:
        rc = lib.ppst_avgpool_bwd(_vp(dy), _vp(dx), p["B"], H, W, p["C"], dx_ld, p["f"], p["C"], st)
    torch.cuda.synchronize()
    assert rc == 0
    check()
    keep = torch.ones(dx_ld, dtype=torch.bool)
    keep[off:off + p["C"]] = False
    assert bool((wide[..., keep.to(dev)] == POISON).all()), "wrote channels beside its slice"
    bad, err = C.compare(C.reference(cid)["dx"], _np(dx), C.bar(c, "dx"))
    print("%-40s dx_ld %d  err %.2e" % (cid, dx_ld, err))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_return_einval_and_write_nothing():
    """out-of-range arguments: the entry returns PPST_EINVAL, launches nothing, writes nothing"""
    from ppst_amd._lib import lib
    dev = _dev()
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    x = torch.full((1, 5, 4, 8), 3.0, device=dev)
    y = torch.full((1, 12, 12, 8), 7.0, device=dev)
    calls = [
        ("reflect pad = extent", lambda: lib.ppst_pad2d(_vp(x), _vp(y), 1, 5, 4, 8, 8, 5, 0, 0, 0, 1, st)),
        ("reflect pad_bwd = extent", lambda: lib.ppst_pad2d_bwd(_vp(x), _vp(y), 1, 5, 4, 8, 0, 0, 4, 0, 1, st)),
        ("pad mode 3", lambda: lib.ppst_pad2d(_vp(x), _vp(y), 1, 5, 4, 8, 8, 1, 1, 1, 1, 3, st)),
        ("crop to nothing", lambda: lib.ppst_pad2d(_vp(x), _vp(y), 1, 5, 4, 8, 8, -3, -2, 0, 0, 0, st)),
        ("pad x_ld < C", lambda: lib.ppst_pad2d(_vp(x), _vp(y), 1, 5, 4, 8, 4, 1, 1, 1, 1, 0, st)),
        ("bilinear dy_ld < C", lambda: lib.ppst_bilinear_bwd(_vp(x), _vp(y), 1, 12, 12, 8, 8, 5, 4, 4, st)),
        ("bilinear dx_ld < C", lambda: lib.ppst_bilinear_bwd(_vp(x), _vp(y), 1, 12, 12, 8, 4, 5, 4, 8, st)),
        ("avgpool H % f", lambda: lib.ppst_avgpool_bwd(_vp(x), _vp(y), 1, 12, 12, 8, 8, 5, 8, st)),
        ("avgpool f = 0", lambda: lib.ppst_avgpool_bwd(_vp(x), _vp(y), 1, 12, 12, 8, 8, 0, 8, st)),
        ("colsum ld < C", lambda: lib.ppst_colsum(_vp(x), _vp(y), _vp(y), 20, 8, 4, 1.0, 0, st)),
        ("colsum rows = 0", lambda: lib.ppst_colsum(_vp(x), _vp(y), _vp(y), 0, 8, 8, 1.0, 0, st)),
        ("linear_wgrad_fused K % 4", lambda: lib.ppst_linear_wgrad_fused(_vp(x), _vp(x), _vp(y), None, 2, 4, 6, 1.0, 1.0, 0, 0, 0, st)),
        ("linear_dgrad B = 0", lambda: lib.ppst_linear_dgrad(_vp(x), _vp(x), _vp(y), _vp(y), 0, 4, 4, 1.0, st)),
        ("wgrad_small_cin cin = 5", lambda: lib.ppst_wgrad_small_cin(_vp(x), _vp(x), _vp(y), _vp(y), 4, 5, 5, 8, 1.0, 0, st)),
        ("l2norm mode 2", lambda: lib.ppst_l2norm_rows_bwd(_vp(x), _vp(x), _vp(y), 2, 8, 1e-7, 2, st)),
        ("softmax div = 0", lambda: lib.ppst_softmax_rows_bwd(_vp(x), _vp(y), 2, 8, 0.0, st)),
        ("corr_prep ncenter > C", lambda: lib.ppst_corr_prep_bwd(_vp(x), _vp(x), _vp(y), 2, 8, 9, 1e-16, st)),
    ]
    for why, call in calls:
        rc = call()
        torch.cuda.synchronize()
        assert rc == -1, "%s: returned %d, not PPST_EINVAL" % (why, rc)
        assert bool((x == 3.0).all()) and bool((y == 7.0).all()), "%s: a refused call wrote" % why
    from ppst_amd import ops
    with pytest.raises(RuntimeError, match="ppst_pad2d"):
        ops.pad2d(x, 5, 0, 0, 0, ops.PAD_REFLECT)
    with pytest.raises(RuntimeError, match="ppst_gap_gmp_multi_bwd"):       # the strip form only: hw % 16 != 0 is refused
        ops.gap_gmp_multi_bwd(torch.zeros(1, 5, 3, 8, device=dev), torch.ones(1, 5, 3, 1, device=dev), torch.zeros(1, 16, device=dev),
                              torch.zeros(1, 16, device=dev), with_plain=False)


def test_dgrad_s2d_names_the_cin_no_conv_plan_takes():
    """bwd_cases.CIN12: the cin at which the half and fp32 rules of ops.dgrad_s2d part has no conv plan in either form -- refused by
    name (the message once failed to format and surfaced as a ValueError about a format character)"""
    from ppst_amd import ops
    c = C.CIN12
    inp = C.OPS[c.op].make(c)
    with pytest.raises(AssertionError, match="Cin % 32 == 0 .got 12."):
        _run_conv_dgrad(c, inp, ops)


def test_half_storage_refusals_return_einval_and_write_nothing():
    """the `_st` entries on what a half tensor may not be: a channel count or pixel stride that is no multiple of 4 (8 for
    depth_to_space), a pointer off the 8-byte grid, hw % 16 != 0 for the pooling adjoint, a cout whose quads do not divide 256, and a
    storage type that is none.  Each returns PPST_EINVAL before any launch or memset: every buffer passed -- workspaces included --
    keeps its fill."""
    from ppst_amd._lib import lib
    dev = _dev()
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    n = 1 << 14
    fills = {"a": (torch.bfloat16, 3.0), "b": (torch.bfloat16, 7.0), "f": (torch.float32, 5.0), "f2": (torch.float32, 6.0), "w": (torch.float32, 9.0),
             "wi": (torch.int32, 77)}
    buf = {k: torch.full((n,), v, device=dev, dtype=dt) for k, (dt, v) in fills.items()}
    a, b, f, f2, w, wi = (_vp(buf[k]) for k in ("a", "b", "f", "f2", "w", "wi"))
    a_off = ctypes.c_void_p(buf["a"].data_ptr() + 2)                    # 2 bytes past the 8-byte grid
    assert buf["a"].data_ptr() % 16 == 0

    def entries(st, C_=8, ld=8, hw=16, cout=32, d2s_c=8, x=a):
        """every `_st` entry on one small valid problem, but for the named deviation"""
        return {
            "dual_stats": lambda: lib.ppst_dual_stats_st(x, a, None, f, 1, hw, C_, ld, ld, 0, None, st, stream),
            "in_bwd_apply": lambda: lib.ppst_in_bwd_apply_st(x, a, None, f, b, 1, hw, C_, ld, ld, 0, C_, 0, st, stream),
            "pad2d": lambda: lib.ppst_pad2d_st(x, b, 1, 5, 4, C_, ld, 1, 1, 1, 1, 0, st, stream),
            "pad2d_bwd": lambda: lib.ppst_pad2d_bwd_st(x, b, 1, 5, 4, C_, 1, 1, 1, 1, 0, st, stream),
            "bilinear_bwd": lambda: lib.ppst_bilinear_bwd_st(x, b, 1, 5, 4, C_, C_, 8, 8, ld, st, stream),
            "colsum": lambda: lib.ppst_colsum_st(x, f, w, 20, C_, ld, 1.0, 0, st, stream),
            "noise_wgrad": lambda: lib.ppst_noise_wgrad_st(x, f, f2, w, 20, C_, ld, 0, st, stream),
            "space_to_depth": lambda: lib.ppst_space_to_depth_st(x, b, 1, 5, 4, C_, ld, st, stream),
            "gap_gmp_bwd": lambda: lib.ppst_gap_gmp_bwd_st(x, None, f, f2, b, wi, 1, hw, C_, ld, 0, st, stream),
            "gap_gmp_multi_bwd": lambda: lib.ppst_gap_gmp_multi_bwd(x, f, f, f2, b, wi, 1, hw, C_, ld, 1, 0, 0, st, stream),
            "wgrad_small_cin": lambda: lib.ppst_wgrad_small_cin_st(f, x, f2, w, 20, 3, 3, cout, 1.0, 0, st, stream),
            "depth_to_space": lambda: lib.ppst_depth_to_space_st(x, b, 1, 4, 4, 8, 8, d2s_c, st, stream),
        }

    calls = []
    for st in (1, 2):
        e6, e10 = entries(st, C_=6, ld=6), entries(st, ld=10)
        calls += [("%s C = 6, st %d" % (k, st), e6[k]) for k in ("dual_stats", "in_bwd_apply", "pad2d", "pad2d_bwd", "bilinear_bwd", "colsum", "noise_wgrad",
                                                                 "space_to_depth")]
        calls += [("%s x_ld = 10, st %d" % (k, st), e10[k]) for k in ("pad2d", "space_to_depth")]
        calls += [("gap_gmp_bwd hw = 15, st %d" % st, entries(st, hw=15)["gap_gmp_bwd"]),
                  ("wgrad_small_cin cout = 12, st %d" % st, entries(st, cout=12)["wgrad_small_cin"]),
                  ("depth_to_space C = 12, st %d" % st, entries(st, d2s_c=12)["depth_to_space"])]
    calls.append(("pad2d pointer 2 bytes past the 8-byte grid, st 2", entries(2, x=a_off)["pad2d"]))
    calls += [("%s st = 3" % k, call) for k, call in entries(3).items()]
    for why, call in calls:
        rc = call()
        torch.cuda.synchronize()
        assert rc == -1, "%s: returned %d, not PPST_EINVAL" % (why, rc)
        for k, (dt, v) in fills.items():
            assert bool((buf[k] == torch.full((1,), v, device=dev, dtype=dt)).all()), "%s: a refused call wrote %s" % (why, k)
