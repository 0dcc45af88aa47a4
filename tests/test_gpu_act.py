"""GPU: the activation-path kernels of csrc/elementwise.hip and the NHWC blur of csrc/upfirdn2d.hip, called through the ppst_amd.ops
entry points on every case of tests/act_cases.py and compared with its float64 reference -- pytest -m gpu.  The device is never
its own judge.

Each case names the kernel form its launcher picks (act_cases.branch_of restates the launcher's condition; printed with the error,
pytest -s shows the table); tests/test_act_cases_cpu.py shows on the CPU that the references are right, that every form and facet
has a case and that the comparison used here, at the bar used here, rejects every seeded defect on these very inputs.

Next to the references: a half-stored launch equals the fp32 launch on the widened inputs rounded once (include/ppst_hip.h; for
the 4 x 4 blur that is sliding form == patch form, the fp32 launch never slides), a repeat of every kernel is bit-identical, a
batch of the statistics kernels equals its single-image calls, gap_gmp_levels equals gap_gmp per map, guard values around every
destination the caller places and the untouched channels of a wide destination keep their fill.  No test sets process environment.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import act_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu
POISON = 12345.0


def _dev():
    return torch.device("cuda", 0)


def _st(c, key, widen):
    return "f32" if widen else c.p.get(key, "f32")


def _put(c, inp, name, C_=None, st="f32"):
    """the operand on the device in its storage type, as the case stores it: the channel slice of the wider tensor (a view)"""
    t = inp[name].to(_dev()).to(C.DTYPE[st])
    C_ = c.p["C"] if C_ is None else C_
    off = c.p.get(name + "_off", 0)
    return t[..., off:off + C_] if t.shape[-1] != C_ else t


def _opt(inp, name):
    return inp[name].to(_dev()) if name in inp else None


def _np(t):
    return t.detach().double().cpu().numpy()


def _dest(c, name, shape, st="f32"):
    """the destination of an out= argument: ``shape`` (its last axis C channels) inside a buffer the test owns, POISON in front,
    behind and -- where the case makes it a channel slice (<name>_ld, <name>_off) -- in the channels beside it; -> (view, check)"""
    C_ = shape[-1]
    ld, off = c.p.get(name + "_ld", C_), c.p.get(name + "_off", 0)
    wide = tuple(shape[:-1]) + (ld,)
    n = int(np.prod(wide))
    buf = torch.full((n + 512,), POISON, device=_dev(), dtype=C.DTYPE[st])
    fill = buf[0].clone()
    body = buf[256:256 + n].view(*wide)
    view = body[..., off:off + C_]
    keep = torch.ones(ld, dtype=torch.bool, device=_dev())
    keep[off:off + C_] = False

    def check():
        torch.cuda.synchronize()
        assert bool((buf[:256] == fill).all()) and bool((buf[256 + n:] == fill).all()), "%s: wrote outside its destination" % name
        assert bool((body[..., keep] == fill).all()), "%s: wrote channels beside its slice" % name
    return view, check


# ------------------------------------------------------------------------------------------------------------- runners
def _run_in_stats(c, inp, ops, widen):
    p = c.p
    part = ops.in_stats(_put(c, inp, "x"), rep_pad=bool(p.get("rep_pad")))
    ss = ops.in_finalize(part, C.stats_count(p), _opt(inp, "style"), _opt(inp, "post_bias"))
    sums = part.double().sum(1)                         # (the chunks' partial sums, added on the host in float64)
    return {"sum": sums[..., 0], "sumsq": sums[..., 1], "scale": ss[..., 0], "shift": ss[..., 1]}


def _aa_args(c, inp, st):
    p = c.p
    return dict(scale_shift=_opt(inp, "ss"), res=_put(c, inp, "res", st=st) if "res" in inp else None, act=p.get("act", 0), prelu=_opt(inp, "prelu"),
                out_scale=p.get("out_scale", 1.0), res_before_act=bool(p.get("before")), res_scale_shift=_opt(inp, "rss"), res_up2=p.get("res") == "up2")


def _run_affine_act(c, inp, ops, widen):
    p = c.p
    st, yst = _st(c, "st", widen), "f32" if widen else p.get("yst", p.get("st", "f32"))
    out, check = _dest(c, "out", (p["B"], p["H"], p["W"], p["C"]), yst)
    y = ops.affine_act(_put(c, inp, "x", st=st), out=out, **_aa_args(c, inp, st))
    check()
    assert y.data_ptr() == out.data_ptr()
    return {"y": y}


def _run_affine_act_stats(c, inp, ops, widen):
    y, part = ops.affine_act_stats(_put(c, inp, "x"), rep_pad=bool(c.p.get("rep_pad")), **_aa_args(c, inp, "f32"))
    sums = part.double().sum(1)
    return {"y": y, "sum": sums[..., 0], "sumsq": sums[..., 1]}


def _run_gap_gmp(c, inp, ops, widen):
    out = ops.gap_gmp(_put(c, inp, "x", st=_st(c, "st", widen)), _opt(inp, "mask"))
    return {"mean": out[:, :c.p["C"]], "max": out[:, c.p["C"]:]}


def _run_gap_gmp_multi(c, inp, ops, widen):
    out = ops.gap_gmp_multi(_put(c, inp, "x", st=_st(c, "st", widen)), inp["masks"].to(_dev()), with_plain=c.p["plain"])
    return {"mean": out[:, :c.p["C"]], "max": out[:, c.p["C"]:]}


def _level_maps(c, inp, st):
    xs, ms = [], []
    for i, (H, W, C_, ld, off, masked) in enumerate(c.p["maps"]):
        xs.append(inp["x%d" % i].to(_dev()).to(C.DTYPE[st])[..., off:off + C_])
        ms.append(_opt(inp, "mask%d" % i))
    return xs, ms


def _run_gap_gmp_levels(c, inp, ops, widen):
    xs, ms = _level_maps(c, inp, _st(c, "st", widen))
    out = {}
    for i, o in enumerate(ops.gap_gmp_levels(xs, ms)):
        C_ = c.p["maps"][i][2]
        out["mean%d" % i], out["max%d" % i] = o[:, :C_], o[:, C_:]
    return out


def _run_avgpool(c, inp, ops, widen):
    p = c.p
    out, check = _dest(c, "out", (p["B"], p["H"] // p["f"], p["W"] // p["f"], p["C"]))
    y = ops.avgpool(_put(c, inp, "x"), p["f"], out=out)
    check()
    return {"y": y}


def _run_bilinear(c, inp, ops, widen):
    p = c.p
    out, check = _dest(c, "out", (p["B"], p["OH"], p["OW"], p["C"]))
    y = ops.bilinear(_put(c, inp, "x"), p["OH"], p["OW"], out=out)
    check()
    return {"y": y}


def _run_maxpool2(c, inp, ops, widen):
    return {"y": ops.maxpool2(inp["x"].to(_dev()))}


def _run_upsample_nearest2(c, inp, ops, widen):
    return {"y": ops.upsample_nearest2(_put(c, inp, "x", st=_st(c, "st", widen)))}


def _run_head_tail(c, inp, ops, widen):
    p = c.p
    feat, check = _dest(c, "feat", (p["B"], p["H"] // p["P"], p["W"] // p["P"], p["C"]))
    feat1, check1 = _dest(c, "feat1", (p["B"], p["H"] // p["D"], p["W"] // p["D"], p["C"]))
    ops.head_tail(_put(c, inp, "x"), inp["ss"].to(_dev()), feat, feat1, act=p.get("act", 0), prelu=_opt(inp, "prelu"))
    check()
    check1()
    return {"feat": feat, "feat1": feat1}


def _run_blur_nhwc(c, inp, ops, widen):
    p = c.p
    x = _put(c, inp, "x", st=_st(c, "st", widen))
    if p.get("off"):                                   # the tensor starts ``off`` elements into its buffer
        x = torch.empty(x.numel() + p["off"], device=_dev(), dtype=x.dtype)[p["off"]:].view(x.shape).copy_(x)
    y, hw = ops.blur_nhwc(x, inp["k"].to(_dev()), p["pads"][0], p["pads"][1], p.get("mode", 0), p.get("down", 1),
                          bool(p.get("s2d")), _opt(inp, "ss"), C.ACT_LRELU if p.get("in_ss") == "lrelu" else C.ACT_NONE)
    assert tuple(hw) == C.blur_out_hw(p)
    return {"y": y}


def _run_conv1x1_small_cin(c, inp, ops, widen):
    p = c.p
    return {"y": ops.conv1x1_small_cin(_put(c, inp, "x", p["cin"]), inp["w"].to(_dev()), inp["bias"].to(_dev()) if p.get("bias", True) else None, p["wscale"],
                                       p.get("act", 0), out_dtype=C.DTYPE[_st(c, "yst", widen)])}


def _run_conv1x1_small_cout(c, inp, ops, widen):
    p = c.p
    return {"y": ops.conv1x1_small_cout(inp["x"].to(_dev()).to(C.DTYPE[_st(c, "st", widen)]), inp["w"].to(_dev()),
                                        inp["bias"].to(_dev()) if p.get("bias", True) else None, p["wscale"])}


def _run_torgb_apply(c, inp, ops, widen):
    p = c.p
    st = _st(c, "st", widen)
    return {"y": ops.torgb_apply(_put(c, inp, "x", st=st), inp["ss"].to(_dev()), _put(c, inp, "res", st=st) if "res" in inp else None, p["out_scale"],
                                 inp["w"].to(_dev()), inp["bias"].to(_dev()), p["wscale"])}


def _run_spatial_modulation(c, inp, ops, widen):
    return {"y": ops.spatial_modulation(inp["x"].to(_dev()), inp["scale"].to(_dev()), inp["bias"].to(_dev()), out_dtype=C.DTYPE[_st(c, "yst", widen)])}


def _run_lerp(c, inp, ops, widen):
    n = len(c.p["sizes"])
    pairs = [(inp["a%d" % i].to(_dev()), inp["b%d" % i].to(_dev())) for i in range(n)]
    ys = ops.lerp_grouped(pairs, c.p["r"]) if c.p.get("grouped") else [ops.lerp(pairs[0][0], pairs[0][1], c.p["r"])]
    return {"y%d" % i: y for i, y in enumerate(ys)}


def _run_tensor2im_u8(c, inp, ops, widen):
    return {"y": ops.tensor2im_u8(inp["x"].to(_dev()))}


RUN = {k[5:]: v for k, v in list(globals().items()) if k.startswith("_run_")}


def _run(c, widen=False, inp=None):
    """-> {output: the tensor as the kernel stored it, on the host}"""
    from ppst_amd import ops
    try:
        out = RUN[c.op](c, C.inputs(c.id) if inp is None else inp, ops, widen)
        torch.cuda.synchronize()
    except RuntimeError as e:
        if any(s in str(e) for s in ("illegal memory access", "HIP error", "hipError")):
            pytest.exit("the device faulted in %s: nothing more is launched (%s)" % (c.id, e), returncode=3)
        raise
    return {k: v.detach().cpu() for k, v in out.items()}


def _half(c):
    return any(c.p.get(k, "f32") != "f32" for k in ("st", "yst"))


# --------------------------------------------------------------------------------------------- against the float64 reference
@pytest.mark.parametrize("cid", [c.id for c in C.CASES])
def test_against_float64_reference(cid):
    c = C.by_id(cid)
    ref, got = C.reference(cid), _run(c)
    assert set(got) == set(ref)
    fails = []
    for k in sorted(ref):
        if C.out_st(c, k) != "f32":
            assert got[k].dtype == C.DTYPE[C.out_st(c, k)], (k, got[k].dtype)
        bad, err = C.judge(c, k, _np(got[k]))
        print("%-64s %-6s err %.2e  bar %.2e%s  %s" % (cid, k, err, C.bar(c, k), "" if C.out_st(c, k) == "f32" or not C.bar(c, k) else
                                                     " (%s: err in units of the allowed error)" % C.out_st(c, k), C.branch_of(c)))
        fails += ["%s: %s" % (k, m) for m in bad]
    assert not fails, "%s [%s]: %s" % (cid, C.branch_of(c), "; ".join(fails))
    again = _run(c)
    for k in got:
        assert torch.equal(again[k], got[k]), "%s: two runs differ" % k
    if _half(c):
        # f_st(x_half) == round(f(float(x_half))): the fp32 launch on the widened inputs, rounded once by torch
        wide = _run(c, widen=True)
        for k in got:
            assert wide[k].dtype == torch.float32
            assert torch.equal(wide[k].to(got[k].dtype), got[k]), "%s: the %s launch is not the fp32 launch rounded once" % (k, C.branch_of(c))


# -------------------------------------------------------------------------------------------- a batch is its single calls
@pytest.mark.parametrize("cid", ["in_stats-C3-7x9-rep_pad", "in_stats-C12-13x11-rep_pad", "in_stats-C64-16x16-style-rep_pad", "in_stats-C8-slice-ld16-off2",
                                 "in_stats-C1028-5x5", "gap_gmp-scalar-C3-13x11-mask01-allneg", "gap_gmp-vec4-C64-16x16-maskfrac-allneg",
                                 "gap_gmp-f16-C12-13x11-mask01-allneg", "gap_gmp-bf16-C8-slice-ld16-off4-maskfrac", "gap_gmp_multi-f32-nm3-plain-C12-13x11",
                                 "affine_act_stats-C12-13x11-ss-lrelu-rep_pad", "affine_act_stats-C8-12x10-up2-rep_pad",
                                 "affine_act_stats-C8-12x10-ss-prelu-res-before-rss"])
def test_batch_equals_single_calls(cid):
    """the chunking depends on the image alone: the image-sharded grid evaluator relies on N single calls reproducing one batch"""
    c = C.by_id(cid)
    B = c.p["B"]
    assert B > 1
    inp = C.inputs(cid)
    whole = _run(c)
    heads = (c.p["nm"] + c.p["plain"]) if c.op == "gap_gmp_multi" else 1
    for b in range(B):
        one = {k: (v[b:b + 1] if (v.dim() > 1 and v.shape[0] == B) else v) for k, v in inp.items()}
        got = _run(c._replace(p=dict(c.p, B=1)), inp=one)
        for k in got:
            rows = whole[k].reshape(heads, B, *whole[k].shape[1:])[:, b]
            assert torch.equal(got[k].reshape(rows.shape), rows), "%s: image %d of the batch differs from its single call" % (k, b)


@pytest.mark.parametrize("cid", [c.id for c in C.CASES if c.op == "gap_gmp_levels"])
def test_gap_gmp_levels_equals_gap_gmp_per_map(cid):
    from ppst_amd import ops
    c = C.by_id(cid)
    xs, ms = _level_maps(c, C.inputs(cid), c.p.get("st", "f32"))
    outs = ops.gap_gmp_levels(xs, ms)
    assert len(outs) == len(xs)
    for i, (x, m, o) in enumerate(zip(xs, ms, outs)):
        assert torch.equal(o, ops.gap_gmp(x, m)), "map %d differs from gap_gmp on the map alone" % i


# ------------------------------------------------------------------------------------------------------------- refusals
def test_launchers_refuse_what_their_kernels_cannot_handle():
    """res_up2 exists in the vector forms only: a call the launcher would send to the one-channel form (a pointer off the 16-byte
    grid) is refused, not run with the residual read at full resolution; nothing is written"""
    from ppst_amd import ops
    dev = _dev()
    x = torch.zeros(1, 4, 4, 8, device=dev)
    res = torch.zeros(1, 2, 2, 8, device=dev)
    wide = torch.full((1, 4, 4, 16), 7.0, device=dev)
    with pytest.raises(RuntimeError, match="ppst_affine_act"):
        ops.affine_act(x, res=res, res_up2=True, out=wide[..., 2:10])
    torch.cuda.synchronize()
    assert bool((wide == 7.0).all()), "a refused call wrote"
    with pytest.raises(RuntimeError, match="ppst_affine_act"):           # half storage: the vector forms only
        ops.affine_act(torch.zeros(1, 4, 4, 6, device=dev, dtype=torch.float16))
    with pytest.raises(RuntimeError, match="ppst_gap_gmp"):
        ops.gap_gmp(torch.zeros(1, 4, 4, 16, device=dev, dtype=torch.float16)[..., 2:10])
    with pytest.raises(RuntimeError, match="ppst_head_tail"):            # D must divide P, P the extents
        ops.head_tail(torch.zeros(1, 6, 6, 4, device=dev), torch.zeros(1, 4, 2, device=dev), torch.zeros(1, 2, 2, 4, device=dev),
                      torch.zeros(1, 3, 3, 4, device=dev))
