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
        # (as the output tensor would hold it: float32, or rounded once to the case's half type)
        bad, _ = C.judge(c, k, C.as_stored(c, k, v.astype(np.float32)))
        assert not bad, "%s: the stored rounding of the reference misses its own bar: %s" % (k, bad)
    muts = C.mutations(c)
    assert len(muts) >= 2, "a case carries at least two seeded defects"
    for name, out in muts:
        assert set(out) <= set(ref) and out, (name, set(out))
        seen = [k for k, v in out.items() if C.judge(c, k, C.as_stored(c, k, v.astype(np.float32)) if "truncation" not in name else v)[0]]
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
            # (precision mode 1 on bf16-stored tensors carries the conv tests' bar of that mode, 2e-2: a class bar, not a measured one)
            assert b == 0 or b < 1e-4 or (c.p.get("prec") == 1 and C.st_of(c) == "bf16" and 4 * e < 1e-4 and b == 2e-2), \
                "a bar this wide says the case is ill-conditioned: fix the inputs"


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
    assert {(c.p["kind"], c.p["prec"]) for c in _of("conv_dgrad") if C.st_of(c) == "f32"} == {(k, q) for k in ("dgrad", "dgrad_s2d", "dgrad_s2ds") for q in (0, 2)}
    ragged = {(33, 70), (30, 34), (20, 36), (33, 37)}
    assert {(c.p["H"], c.p["W"]) for c in _of("conv_dgrad")} >= ragged and {(c.p["H"], c.p["W"]) for c in _of("conv_wgrad")} >= ragged
    # bias buffers: written and added into, with dw written and added into, on either bias path
    for path in ("csum", "colsum"):
        seen = {(bool(c.p.get("acc")), C._cw_bias_acc(c), "db0" in C.inputs(c.id)) for c in _of("conv_wgrad") if C.branch_of(c).endswith(path)}
        assert seen >= {(False, False, False), (False, False, True), (False, True, True), (True, False, True), (True, True, True)}, (path, seen)


HALF_CASES = [c for c in C.CASES if C.st_of(c) != "f32"]


@pytest.mark.parametrize("c", HALF_CASES, ids=lambda c: c.id)
def test_half_case_inputs_hold_stored_values_and_side_operands_stay_float32(c):
    """the typed operands are exactly representable in the case's type (rounded once), what derives from them was computed after
    the rounding, gates keep their distance, masks their four values; the half rule passes a correctly rounded reference and the
    seeded half defects are there"""
    inp, st = C.inputs(c.id), C.st_of(c)
    typed = [k for k in C.TYPED[c.op] if k in inp]
    assert typed and typed[0] == C.TYPED[c.op][0]
    for k in typed:
        assert torch.equal(inp[k], inp[k].to(C.HALF[st]).float()), k
    for k in ("g", "v", "noise", "style", "mr", "w"):           # the side operands stay float32: not rounded
        if k in inp and k not in typed and inp[k].numel() > 8:
            assert not torch.equal(inp[k], inp[k].to(C.HALF[st]).float()), k
    for k in ("mask", "masks"):
        if k in inp:
            assert set(inp[k].unique().tolist()) <= {0.0, 0.25, 0.5, 1.0}
    if c.op in ("gap_gmp_bwd", "gap_gmp_multi_bwd"):          # the forward maximum is the maximum of the STORED values
        x = C._sl(c, inp, "x")
        heads = [inp.get("mask")] if c.op == "gap_gmp_bwd" else C._gmm_heads(c, inp)
        assert torch.equal(inp["v"], torch.cat([C.gmp_forward32(x, m) for m in heads], 0))
    if c.op == "in_bwd":
        for k in ("y", "gate"):
            if k in inp:
                assert C._sl(c, inp, k).abs().min() >= 2.0 ** -9
    names = [n for n, _ in C.mutations(c)]
    ref = C.reference(c.id)
    half_out = [k for k in ref if C.out_st(c, k) != "f32" and C.bar(c, k) != 0 and not np.array_equal(C.as_stored(c, k, ref[k]), ref[k])]
    assert ("half output stored by truncation" in names) == bool(half_out), (names, half_out)
    if c.op in ("in_bwd", "gap_gmp_bwd", "gap_gmp_multi_bwd") or (c.op == "pad2d" and c.p["mode"]) or (c.op == "bilinear_bwd" and c.p["H"] < 64):
        assert half_out or not c.p.get("norm", True), "a computed half output whose values the type holds exactly shows no rounding"
    if any(C.bar(c, k) != 0 for k in C.reference(c.id)):
        assert "operands read as the other half type" in names
    if any(c.p.get(k + "_off") for k in typed):
        assert any("offset" in n for n in names), names


def test_half_table_of_the_issue_is_present_and_forms_are_stated():
    ids = {c.id for c in HALF_CASES}
    for st in ("f16", "bf16"):
        want = ["in_bwd-%s-hw35-C8-plain", "in_bwd-%s-hw480-C8-gate-style-dstyle", "in_bwd-%s-hw480-C8-post-gate-style", "in_bwd-%s-hw480-C32-no-norm",
                "in_bwd-%s-hw15-C1032-gate-style-dstyle", "in_bwd-%s-hw480-C8-slices-gate-style-dstyle", "pad2d-%s-reflect-C8-largest",
                "pad2d-%s-replicate-C8-slice-ld16-off4", "bilinear_bwd-%s-C8-5x7-to-12x9", "bilinear_bwd-%s-C8-12x9-to-5x7", "bilinear_bwd-%s-C4-64x64-to-8x8",
                "bilinear_bwd-%s-C8-slice-ld16-off4", "gap_gmp_bwd-%s-strip-C8-16x12-plain", "gap_gmp_bwd-%s-strip-C8-16x12-mask",
                "gap_gmp_bwd-%s-strip-C8-16x12-quant-ties", "gap_gmp_bwd-%s-strip-C8-16x12-plateau-ties-mask", "gap_gmp_bwd-%s-strip-C8-16x12-zero-image-acc",
                "gap_gmp_bwd-%s-strip-C8-slice-ld16-off4-ties", "gap_gmp_multi_bwd-%s-nm3-plain-quant", "gap_gmp_multi_bwd-%s-nm3-plain-plateau-acc",
                "gap_gmp_multi_bwd-%s-nm1-noplain-plateau-slice-ld16-off8", "colsum-%s-rows1-C8", "colsum-%s-rows7-C8", "colsum-%s-rows2048-C8",
                "colsum-%s-rows2049-C8", "colsum-%s-rows2049-C64-slice-ld80-off8-scale-acc", "colsum-%s-rows37-C1028", "noise_wgrad-%s-C4-5x7",
                "noise_wgrad-%s-C4-5x7-acc", "noise_wgrad-%s-C96-9x11", "noise_wgrad-%s-C1024-3x3", "noise_wgrad-%s-C1028-3x3",
                "noise_wgrad-%s-C32-33x37-slice-ld40-off4", "wgrad_small_cin-%s-cin1-npix1025-cout32", "wgrad_small_cin-%s-cin3-npix1025-cout32",
                "wgrad_small_cin-%s-cin4-npix1025-cout32", "wgrad_small_cin-%s-cin3-npix77-cout32-acc", "wgrad_small_cin-%s-cin3-npix1025-cout32-slice-ld8-off5",
                "wgrad_small_cin-%s-cin3-npix5-cout1024", "space_to_depth-%s-33x37-C8", "space_to_depth-%s-6x5-C8", "space_to_depth-%s-1x7-C12",
                "space_to_depth-%s-5x7-C8-slice-ld16-off4"]
        want += ["pad2d-%%s-%s-C8-%s" % (m, k) for m in ("zero", "reflect", "replicate") for k in ("asym", "crop", "H2")]
        assert not [w % st for w in want if w % st not in ids]
    assert {"conv_dgrad-p1-bf16-s2d-entry-33x37-cin32", "conv_dgrad-p1-bf16-s2d-entry-15x9-cin96"} <= ids
    assert C.branch_of(C.by_id("conv_dgrad-p1-bf16-s2d-entry-33x37-cin32")) == "conv_dgrad:entry-stack:bf16x1:bf16"
    assert C.branch_of(C.by_id("conv_dgrad-p1-bf16-s2d-entry-15x9-cin96")) == "conv_dgrad:entry-four-group:bf16x1:bf16"
    # the half rule of the entry's switch: cin 12 goes to the four-group form, where the fp32 rule sends it to the stack (no conv plan
    # takes a cin that is no multiple of 32: the rule is stated, the case cannot run)
    assert C.branch_of(C.CIN12) == "conv_dgrad:entry-four-group:bf16x1:bf16" and C._cd_form(C.as_f32(C.CIN12)) == "entry-stack"
    assert C.CIN12.id not in ids
    # the slices of the half cases start 4 or 8 elements in: 8-byte aligned, and at 4 not 16-byte aligned
    offs = {c.p[k] for c in HALF_CASES for k in c.p if k.endswith("_off") and k[:-4] in C.TYPED[c.op]}
    assert offs == {4, 8}
    # the fp32 launch takes another kernel form for: noise_wgrad C96 (24 lanes do not divide 256), and the convs (not compared here)
    other = sorted(c.id for c in HALF_CASES if not C.same_form_as_f32(c))
    assert other == sorted(["noise_wgrad-%s-C96-9x11" % st for st in ("f16", "bf16")] + ["conv_dgrad-p1-bf16-s2d-entry-33x37-cin32",
                                                                                          "conv_dgrad-p1-bf16-s2d-entry-15x9-cin96"]), other
    names = {n for c in HALF_CASES if c.op == "noise_wgrad" for n, _ in C.mutations(c)}
    assert {"idle tail lanes take a pixel slot that their channel quads alone reach", "channels past the first 1024 left out"} <= names


def test_truncation_and_other_type_are_what_they_say():
    v = np.array([1.0 + 2.0 ** -7 - 2.0 ** -20, -(1.0 + 2.0 ** -7 - 2.0 ** -20), 3.0, 1.0 + 2.0 ** -10 - 2.0 ** -20])
    assert np.array_equal(C.truncated(v, "bf16"), [1.0, -1.0, 3.0, 1.0])
    assert np.array_equal(C.truncated(v, "f16"), [1.0 + 2.0 ** -8 + 2.0 ** -9 + 2.0 ** -10, -(1.0 + 2.0 ** -8 + 2.0 ** -9 + 2.0 ** -10), 3.0, 1.0])
    one = torch.tensor([1.0])
    assert C.as_other_half(one, "bf16").item() == 1.875 and C.as_other_half(one, "f16").item() == 2.0 ** -7


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
