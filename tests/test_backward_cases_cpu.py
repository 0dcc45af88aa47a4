"""No GPU: the references, the inputs and the bars of tests/test_gpu_backward_kernels.py are proven here before the device is
trusted by them (tests/bwd_cases.py).
  * every explicit reference agrees with float64 autograd of the obvious forward to 1e-12 (the arg-max rule: with the backward
    of F.adaptive_max_pool2d(., 1), which routes a tie to the first maximum);
  * every seeded defect of every case is rejected by the comparison the GPU test uses, at the GPU test's bar, on the case's own
    inputs -- and the float64 reference itself, rounded to float32, passes it;
  * tie inputs tie, gate inputs stay off the boundary;
  * branch_of reaches every kernel family of the launchers.
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bwd_cases as C  # noqa: E402

IDS = [c.id for c in C.CASES]


def _of(op):
    return [c for c in C.CASES if c.op == op]


def _close(a, b, tol=1e-12):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    s = max(np.abs(b).max(), 1e-300)
    assert np.abs(a - b).max() <= tol * s, np.abs(a - b).max() / s


# ------------------------------------------------------------------------------------------------------ reference checks
@pytest.mark.parametrize("c", _of("gap_gmp_bwd") + _of("gap_gmp_multi_bwd"), ids=lambda c: c.id)
def test_gap_gmp_explicit_reference_is_autograd_with_first_maximum(c):
    inp = C.inputs(c.id)
    x = C._sl(c, inp, "x")
    if c.op == "gap_gmp_bwd":
        want = C.gmp_bwd_autograd(x, inp.get("mask"), inp["g"])
    else:
        B = c.p["B"]
        want = sum(C.gmp_bwd_autograd(x, m, inp["g"][h * B:(h + 1) * B]) for h, m in enumerate(C._gmm_heads(c, inp)))
    if "out0" in inp:
        want = want + inp["out0"].double()
    _close(C.reference(c.id)["dx"], want.numpy())


@pytest.mark.parametrize("c", [c for c in _of("gap_gmp_bwd") + _of("gap_gmp_multi_bwd") if c.p.get("ties")], ids=lambda c: c.id)
def test_tie_inputs_tie_in_most_channels(c):
    inp = C.inputs(c.id)
    x = C._sl(c, inp, "x")
    heads = [inp.get("mask")] if c.op == "gap_gmp_bwd" else C._gmm_heads(c, inp)
    for m in heads:
        mx = (x if m is None else x * m[..., None]).reshape(x.shape[0], -1, x.shape[3])
        tied = ((mx == mx.max(1, keepdim=True).values).sum(1) > 1).float().mean().item()
        assert tied > 0.5, "only %.0f %% of the (image, channel) pairs have a tied maximum" % (100 * tied)
    if c.p.get("mask") == "zero_image":                   # a fully masked image receives no gradient
        if "out0" in inp:
            assert np.array_equal(C.reference(c.id)["dx"][0], inp["out0"][0].double().numpy())
        else:
            assert np.all(C.reference(c.id)["dx"][0] == 0)


def test_forward_maximum_is_exact_in_float32():
    """the kernel finds the arg-max by comparing m * x with the forward's maximum: the float32 products of the cases are exact"""
    for c in _of("gap_gmp_bwd"):
        inp = C.inputs(c.id)
        if "mask" in inp:
            x = C._sl(c, inp, "x")
            assert torch.equal((x * inp["mask"][..., None]).double(), x.double() * inp["mask"][..., None].double()), c.id


@pytest.mark.parametrize("c", _of("pad2d"), ids=lambda c: c.id)
def test_pad_index_map_is_F_pad_and_its_autograd(c):
    p = c.p
    py0, py1, px0, px1 = p["pads"]
    if p["mode"] and min(p["pads"]) < 0:
        # F.pad states no crop for reflect / replicate: crop first, pad after (the two commute on disjoint sides)
        crop = lambda t: t[:, :, max(-py0, 0):t.shape[2] - max(-py1, 0), max(-px0, 0):t.shape[3] - max(-px1, 0)]
        pos = (max(px0, 0), max(px1, 0), max(py0, 0), max(py1, 0))
    else:
        crop, pos = (lambda t: t), (px0, px1, py0, py1)
    inp = C.inputs(c.id)
    x = C._nchw(C._sl(c, inp, "x").double()).clone().requires_grad_(True)
    y = F.pad(crop(x), pos, mode=("constant", "reflect", "replicate")[p["mode"]])
    y.backward(C._nchw(inp["dy"].double()))
    r = C.reference(c.id)
    _close(r["y"], C._nhwc(y.detach()).numpy(), 0)
    _close(r["dx"], C._nhwc(x.grad).numpy())


@pytest.mark.parametrize("c", _of("l2norm_rows_bwd"), ids=lambda c: c.id)
def test_l2norm_explicit_reference_is_autograd(c):
    inp = C.inputs(c.id)
    x = inp["x"].double().clone().requires_grad_(True)
    C._l2_fwd(x, c.p["eps"], c.p["mode"]).backward(inp["g"].double())
    # (at K = 1 the two terms cancel: measured against their size, as the bar is)
    assert np.abs(C.reference(c.id)["dx"] - x.grad.numpy()).max() <= 1e-12 * C.scale_of(c, "dx")


@pytest.mark.parametrize("c", _of("softmax_rows_bwd_"), ids=lambda c: c.id)
def test_softmax_explicit_reference_is_autograd(c):
    inp = C.inputs(c.id)
    z = inp["logits"].double().clone().requires_grad_(True)
    p = torch.softmax(z / c.p["div"], 1)
    p.backward(inp["g"].double())
    _close(C.softmax_bwd_explicit(p.detach(), inp["g"], c.p["div"], torch.float64).numpy(), z.grad.numpy())
    if c.p.get("one_hot"):
        assert p[0].max().item() > 0.999


@pytest.mark.parametrize("c", _of("prelu_bwd"), ids=lambda c: c.id)
def test_prelu_explicit_reference_is_autograd(c):
    inp = C.inputs(c.id)
    want, r = C._pr_autograd(c, inp), C.reference(c.id)
    _close(r["gpre"], want["gpre"].numpy())
    _close(r["dslope"], want["dslope"].numpy())
    assert C._pr_z(c, inp, torch.float32).abs().min().item() >= 1e-3


@pytest.mark.parametrize("c", _of("l1") + _of("linear") + _of("colsum") + _of("noise_wgrad") + _of("wgrad_small_cin"), ids=lambda c: c.id)
def test_formula_references_are_autograd_of_the_forward(c):
    inp, r, p = C.inputs(c.id), C.reference(c.id), c.p
    d = lambda t: t.double().clone().requires_grad_(True)
    if c.op == "l1":
        a = d(inp["a"])
        loss = p["weight"] * (a - inp["b"].double()).abs().mean()
        loss.backward()
        _close(r["grad"], a.grad.numpy())
        _close(r["loss"], loss.detach().numpy().reshape(1))
    elif c.op == "linear":
        s = p.get("scale", 1.0)
        x, w, b = d(inp["x"]), d(inp["w"]), torch.zeros(p["N"], dtype=torch.float64, requires_grad=True)
        (s * F.linear(x, w) + p.get("bscale", 1.0) * b).backward(inp["dy"].double())
        acc = lambda k: inp[k].double().numpy() if p.get("acc") else 0
        _close(r["dx"], x.grad.numpy())
        _close(r["dw"], w.grad.numpy() + acc("dw0"))
        if "db" in r:
            _close(r["db"], b.grad.numpy() + acc("db0"))
            xr, w2 = d(inp["x"]), d(inp["w"])
            (s * F.linear(F.relu(xr) if p.get("relu_in") else xr, w2)).backward(inp["dy"].double())
            _close(r["dw_fused"], w2.grad.numpy() + acc("dw0"))
            if p.get("relu_in"):                       # the gate of a ReLU in front of a linear, as linear_dgrad_gate applies it
                xg = d(inp["gate"])
                (s * F.linear(F.relu(xg), inp["w"].double())).backward(inp["dy"].double())
                _close(r["dx_gate"], xg.grad.numpy())
        assert inp["x"].abs().min() >= 1e-3 and inp["gate"].abs().min() >= 1e-3
    elif c.op == "colsum":
        b = torch.zeros(p["C"], dtype=torch.float64, requires_grad=True)
        g = C._sl(c, inp, "x").double()
        ((torch.zeros_like(g) + b) * g).sum().backward()               # d/db of <x + b, g>: the bias gradient
        _close(r["out"], p.get("scale", 1.0) * b.grad.numpy() + (inp["out0"].double().numpy() if "out0" in inp else 0))
    elif c.op == "noise_wgrad":
        w = torch.zeros(1, dtype=torch.float64, requires_grad=True)
        g = C._sl(c, inp, "dpre").double()
        ((w * inp["noise"].double()[..., None]).expand_as(g) * g).sum().backward()
        _close(r["out"], w.grad.numpy() + (inp["out0"].double().numpy() if "out0" in inp else 0))
    else:
        w = torch.zeros(p["cout"], p["cin"], 1, 1, dtype=torch.float64, requires_grad=True)
        x = C._nchw(C._sl(c, inp, "x", C=p["cin"]).double())
        (p.get("scale", 1.0) * F.conv2d(x, w)).backward(C._nchw(inp["dy"].double()))
        _close(r["dw"], w.grad.numpy() + (inp["out0"].double().numpy() if "out0" in inp else 0))


@pytest.mark.parametrize("c", _of("in_bwd"), ids=lambda c: c.id)
def test_instance_norm_explicit_reference_is_autograd(c):
    inp = C.inputs(c.id)
    if not c.p.get("norm", True):
        g, y = C._sl(c, inp, "g").double(), C._sl(c, inp, "y").double()
        sc, sh = (torch.zeros(c.p["B"], 1, 1, c.p["C"], dtype=torch.float64, requires_grad=True) for _ in range(2))
        ((y * sc + sh) * g).sum().backward()                      # SpatialCodeModulation: d/d(scale, shift)
        _close(C.reference(c.id)["dstyle"], torch.cat([sc.grad.flatten(1), sh.grad.flatten(1)], 1).numpy())
        return
    dx, dst, mr = C.in_bwd_autograd(c, inp)
    got = C.in_bwd_explicit(c, inp, torch.float64, mr=mr)
    _close(got["dx"].numpy(), dx.numpy(), 1e-11 if c.p.get("big_mean") else 1e-12)
    if "dstyle" in got:
        _close(got["dstyle"].numpy(), dst.numpy(), 1e-11 if c.p.get("big_mean") else 1e-12)
    assert float((mr.float() - inp["mr"]).abs().max()) <= 1e-6 * float(inp["mr"].abs().max())
    for k in ("y", "gate"):
        if k in inp:
            assert C._sl(c, inp, k).abs().min() >= 1e-3


def test_upscale_weight_forward_is_the_oracle():
    import ppst_oracle as O
    w = torch.randn(5, 3, 3, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    assert torch.equal(C.upscale_weight_fwd(w), O.upscale_weight(w))


@pytest.mark.parametrize("c", _of("in_finalize_train"), ids=lambda c: c.id)
def test_in_finalize_reference_is_instance_norm_statistics(c):
    """mean and rstd of the reference are F.instance_norm's, up to what the float32 partial sums lost"""
    inp, r = C.inputs(c.id), C.reference(c.id)
    x = inp["x"].double().reshape(c.p["B"], -1, c.p["C"])
    _close(r["mr"][..., 0], x.mean(1).numpy(), 1e-6)
    _close(r["mr"][..., 1], (1.0 / torch.sqrt(x.var(1, unbiased=False) + 1e-5)).numpy(), 1e-6)


# ----------------------------------------------------------------------------------------------------------- sensitivity
@pytest.mark.parametrize("cid", IDS)
def test_bar_passes_the_reference_and_rejects_every_seeded_defect(cid):
    c = C.by_id(cid)
    ref = C.reference(cid)
    for k, v in ref.items():
        bad, _ = C.judge(c, k, v.astype(np.float32))
        assert not bad, "%s: the float32 rounding of the reference misses its own bar: %s" % (k, bad)
    muts = C.mutations(c)
    assert len(muts) >= 2, "a case carries at least two seeded defects"
    for name, out in muts:
        assert set(out) <= set(ref)
        seen = [k for k, v in out.items() if C.judge(c, k, v.astype(np.float32))[0]]
        assert seen, "the inputs of %s cannot show the defect '%s' at the bar" % (cid, name)


@pytest.mark.parametrize("c", _of("conv_wgrad_p1"), ids=lambda c: c.id)
def test_storage_bar_passes_equal_results_and_rejects_every_seeded_defect(c):
    """the second comparison of the single-pass weight-gradient test (bf16-stored against fp32-stored operands, C.STORAGE_BAR):
    the reference passes it against itself, every seeded defect misses it in some output; the case's operands are
    bfloat16-representable and its table is the one of the issue"""
    ref = {k: v.astype(np.float32) for k, v in C.reference(c.id).items()}
    for k, v in ref.items():
        assert not C.storage_violations(v, v)[0]
    for name, out in C.mutations(c):
        assert any(C.storage_violations(ref[k], v.astype(np.float32))[0] for k, v in out.items()), (c.id, name)
    names = {n for n, _ in C.mutations(c)}
    assert "last tile column lost" in names and (not c.p.get("bias") or "column sums skip the units beyond stride" in names)
    inp = C.inputs(c.id)
    for k in ("x", "dy"):
        assert torch.equal(inp[k], inp[k].bfloat16().float())


def test_single_pass_weight_gradient_table_is_the_issues():
    got = {(c.p.get("kind", "conv"), c.p["k"], c.p["B"], c.p["H"], c.p["W"], c.p["cin"], c.p["cout"], bool(c.p.get("bias")), c.p.get("splits"))
           for c in _of("conv_wgrad_p1")}
    assert got == {("conv", 1, 2, 17, 19, 128, 64, True, None), ("conv", 1, 2, 20, 36, 64, 256, True, None), ("dgradT", 3, 2, 17, 19, 64, 32, False, None),
                   ("s2d", 3, 1, 33, 37, 32, 64, True, None), ("conv", 3, 2, 33, 37, 32, 32, True, 1), ("conv", 1, 3, 9, 11, 32, 32, False, None),
                   ("conv", 3, 1, 9, 11, 32, 96, True, None)}
    # the unit walk that is no power of two (three live slabs: NQ 24, stride 240) is in the fp32-class table as well
    assert any(C._cw_chan(c)[1] == 96 and C.branch_of(c).endswith("csum") for c in _of("conv_wgrad"))
    first = C.wg_first_pass(C.by_id("conv_wgrad_p1-k3-9x11-32to96-bias"))         # 256 // 24 = 10 pixels of a tile's first row
    assert first[0, :10].all() and not first[0, 10:].any() and not first[1].any() and first[2, :10].all()


def test_every_op_has_two_kinds_of_defect_and_the_listed_kinds_occur():
    kinds = {}
    for c in C.CASES:
        kinds.setdefault(c.op, set()).update(n for n, _ in C.mutations(c))
    for op, k in kinds.items():
        assert len(k) >= 2, (op, k)
    every = set().union(*kinds.values())
    for want in ("last output row left out of the window", "tie sent to the last pixel", "last row left out", "slice offset ignored",
                 "accumulate overwrites", "scalar tail channels zero", "batch rows 17.. zero", "ragged last slice of W left out"):
        assert want in every, want


def test_bars_print():
    """the bar of every case and output, and the float32-reference error it was taken from (pytest -s shows the table)"""
    for c in C.CASES:
        for k, e in C.err32(c.id).items():
            b = C.bar(c, k)
            print("%-58s %-9s bar %.2e  (float32 reference error %.2e)  %s" % (c.id, k, b, e, C.branch_of(c)))
            assert b == 0 or b < 1e-4, "a bar this wide says the case is ill-conditioned: fix the inputs"


# -------------------------------------------------------------------------------------------------------------- coverage
def test_branch_of_reaches_every_kernel_family():
    reached = {}
    for c in C.CASES:
        reached.setdefault(C.branch_of(c), []).append(c.id)
    missing = [f for f in C.FAMILIES if f not in reached]
    assert not missing, missing
    assert set(reached) <= set(C.FAMILIES), sorted(set(reached) - set(C.FAMILIES))


def test_the_minimum_table_of_the_issue_is_present():
    ids = set(IDS)
    for (h, w), (oh, ow) in C._BIL_SHAPES:
        for ch in (4, 8):
            assert "bilinear_bwd-C%d-%dx%d-to-%dx%d" % (ch, h, w, oh, ow) in ids
    assert {c.p["B"] for c in _of("bilinear_bwd")} >= {1, 3}
    assert {c.p["f"] for c in _of("avgpool_bwd")} == {1, 2, 4, 8}
    assert {c.p["rows"] for c in _of("colsum")} >= {1, 2047, 2048, 2049}
    assert {c.p["B"] for c in _of("linear")} >= {1, 16, 17, 33}
    assert {(c.p["cin"], c.p["npix"]) for c in _of("wgrad_small_cin")} >= {(a, b) for a in (1, 3, 4) for b in (1023, 1024, 1025)}
    assert {(c.p["nm"], c.p["plain"]) for c in _of("gap_gmp_multi_bwd")} == {(1, True), (1, False), (3, True), (3, False)}
    wg = {(c.p.get("kind", "conv"), c.p["prec"]) for c in _of("conv_wgrad")}
    assert wg == {(k, q) for k in ("conv", "s2d", "dgradT") for q in (0, 2)}
    assert any(c.p.get("kind") == "s2d" and (c.p["H"], c.p["W"]) == (33, 37) for c in _of("conv_wgrad"))
    assert {(c.p["kind"], c.p["prec"]) for c in _of("conv_dgrad")} == {(k, q) for k in ("dgrad", "dgrad_s2d", "dgrad_s2ds") for q in (0, 2)}
    ragged = {(33, 70), (30, 34), (20, 36), (33, 37)}
    assert {(c.p["H"], c.p["W"]) for c in _of("conv_dgrad")} >= ragged and {(c.p["H"], c.p["W"]) for c in _of("conv_wgrad")} >= ragged
    # bias buffers: written and added into, with dw written and added into, on either bias path
    for path in ("csum", "colsum"):
        seen = {(bool(c.p.get("acc")), C._cw_bias_acc(c), "db0" in C.inputs(c.id)) for c in _of("conv_wgrad") if C.branch_of(c).endswith(path)}
        assert seen >= {(False, False, False), (False, False, True), (False, True, True), (True, False, True), (True, True, True)}, (path, seen)


def test_space_to_depth_of_the_references_is_pixel_unshuffle():
    """the phase-major copy the s2d and dgradT references undo: F.pixel_unshuffle with the phase in front of the channel"""
    x = torch.randn(2, 7, 9, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    s = C._s2d_stack(x)
    assert torch.equal(C._s2d_unstack(s, 7, 9), x)
    want = F.pixel_unshuffle(F.pad(C._nchw(x), [0, 1, 0, 1]), 2).view(2, 3, 4, 4, 5).permute(0, 3, 4, 2, 1).reshape(2, 4, 5, 12)
    assert torch.equal(s, want)


@pytest.mark.parametrize("c", [c for c in _of("conv_wgrad") if c.p.get("kind") == "dgradT" and not c.p.get("acc")], ids=lambda c: c.id)
def test_dgradT_reference_is_the_gradient_of_blur_and_conv_transpose(c):
    """dw3 of the reference is the adjoint of the weight blur applied to dw (ops.upscale_weight_bwd's contract), times the scale"""
    r, p = C.reference(c.id), c.p
    w = torch.zeros(p["cout"], p["cin"], 3, 3, dtype=torch.float64, requires_grad=True)
    (p["scale"] * C.upscale_weight_fwd(w)).backward(torch.from_numpy(r["dw"]))
    _close(r["dw3"], w.grad.numpy())
