"""No GPU: the references, the inputs and the bars of tests/test_gpu_act.py are proven here before the device is trusted by them
(tests/act_cases.py).
  * the references agree with independent formulations: F.instance_norm, F.interpolate, F.avg_pool2d, F.max_pool2d, F.conv2d and
    the oracle's upfirdn2d (+ F.pad), instance_norm and tensor2im;
  * every form a launcher can pick, and every facet the kernels have inside a form, has a case: FORMS and FACETS are compared for
    equality, so a case removed later fails here;
  * every seeded defect of every case is rejected by the comparison the GPU test uses, at the GPU test's bar, on the case's own
    inputs -- and the float64 reference itself, rounded once to the output's storage type, passes it;
  * the float32 evaluation of every reference passes the bar taken from it;
  * the half bar accepts ref.to(half) and rejects an error of one ulp on 1 % of the elements;
  * gate inputs stay off the boundary, mask products are exact.
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import act_cases as C  # noqa: E402

IDS = [c.id for c in C.CASES]
BIG = 1 << 18            # pixels from which a case counts as one of the four chunk-size cases

# every form a launcher of these ops can pick (its ``if``s, both sides; there is no 8-channel 4 x 4 blur) ...
FORMS = {
    "affine_act:V1:f32>f32", "affine_act:V4:bf16>bf16", "affine_act:V4:bf16>f32", "affine_act:V4:f16>f16",
    "affine_act:V4:f16>f32", "affine_act:V4:f32>bf16", "affine_act:V4:f32>f16", "affine_act:V4:f32>f32",
    "affine_act:V8:bf16>bf16", "affine_act:V8:bf16>f32", "affine_act:V8:f16>f16", "affine_act:V8:f16>f32",
    "affine_act:V8:f32>bf16", "affine_act:V8:f32>f16", "affine_act_stats:vec4", "avgpool:f1", "avgpool:f2", "avgpool:f4",
    "avgpool:f8", "bilinear", "blur:k3:bf16:CV4:patch:down2", "blur:k3:bf16:CV4:patch:plain", "blur:k3:bf16:CV4:patch:s2d",
    "blur:k3:bf16:CV8:patch:down2", "blur:k3:bf16:CV8:patch:plain", "blur:k3:bf16:CV8:patch:s2d",
    "blur:k3:f16:CV4:patch:down2", "blur:k3:f16:CV4:patch:plain", "blur:k3:f16:CV4:patch:s2d", "blur:k3:f16:CV8:patch:down2",
    "blur:k3:f16:CV8:patch:plain", "blur:k3:f16:CV8:patch:s2d", "blur:k3:f32:CV4:patch:down2", "blur:k3:f32:CV4:patch:plain",
    "blur:k3:f32:CV4:patch:s2d", "blur:k4:bf16:CV4:patch:down2", "blur:k4:bf16:CV4:patch:plain", "blur:k4:bf16:CV4:patch:s2d",
    "blur:k4:bf16:CV4:slide:plain", "blur:k4:bf16:CV4:slide:s2d", "blur:k4:f16:CV4:patch:down2",
    "blur:k4:f16:CV4:patch:plain", "blur:k4:f16:CV4:patch:s2d", "blur:k4:f16:CV4:slide:plain", "blur:k4:f16:CV4:slide:s2d",
    "blur:k4:f32:CV4:patch:down2", "blur:k4:f32:CV4:patch:plain", "blur:k4:f32:CV4:patch:s2d", "gap_gmp:bf16", "gap_gmp:f16",
    "gap_gmp:scalar", "gap_gmp:vec4", "gap_gmp_levels:bf16", "gap_gmp_levels:f16", "gap_gmp_levels:f32", "gap_gmp_multi:bf16",
    "gap_gmp_multi:f16", "gap_gmp_multi:f32", "head_tail:P2:D1", "head_tail:P2:D2", "head_tail:P4:D1", "head_tail:P4:D2",
    "head_tail:P8:D1", "head_tail:P8:D2", "in_stats:scalar", "in_stats:vec4", "lerp:grouped", "lerp:grouped:>GROUP_MAX",
    "lerp:single", "maxpool2", "small_cin:bf16", "small_cin:f16", "small_cin:f32", "small_cout:cout3:bf16",
    "small_cout:cout3:f16", "small_cout:cout3:f32", "small_cout:generic:bf16", "small_cout:generic:f16",
    "small_cout:generic:f32", "spatial_modulation:bf16", "spatial_modulation:f16", "spatial_modulation:f32", "tensor2im_u8",
    "torgb_apply:bf16", "torgb_apply:f16", "torgb_apply:f32", "upsample_nearest2:bf16", "upsample_nearest2:f16",
    "upsample_nearest2:f32",
}

# ... and every facet inside a form the issue lists
FACETS = {
    "affine_act_stats:rep_pad", "affine_act_stats:vec4:masked-lanes", "bilinear:down-fractional", "bilinear:down-integer",
    "bilinear:identity", "bilinear:up-by-2", "bilinear:up-by-4", "bilinear:up-by-8", "bilinear:up-fractional",
    "blur:CV4-by-pointer", "blur:in_ss-affine", "blur:in_ss-lrelu", "blur:in_ss-none", "blur:input-smaller-than-the-taps", "blur:out_w%4=0",
    "blur:out_w%4=1", "blur:out_w%4=2", "blur:out_w%4=3", "blur:pad-reflect-1-1", "blur:pad-reflect-2-1",
    "blur:pad-reflect-2-2", "blur:pad-zero-1-0", "blur:pad-zero-1-1", "blur:pad-zero-2-1", "blur:pad-zero-2-2",
    "blur:s2d:even-rows-odd-columns", "blur:s2d:odd-rows-even-columns", "blur:s2d:odd-rows-odd-columns",
    "blur:slide:last-band-full", "blur:slide:last-band-partial", "finalize:partials-1", "finalize:partials-2..128",
    "finalize:partials->128", "gap_gmp:bf16:all-negative", "gap_gmp:bf16:all-negative-masked", "gap_gmp:bf16:masked-lanes",
    "gap_gmp:f16:all-negative", "gap_gmp:f16:all-negative-masked", "gap_gmp:f16:masked-lanes", "gap_gmp:mask-01",
    "gap_gmp:mask-frac", "gap_gmp:scalar:all-negative", "gap_gmp:scalar:all-negative-masked",
    "gap_gmp:scalar:channel-passes>1", "gap_gmp:scalar:masked-lanes", "gap_gmp:vec4:all-negative",
    "gap_gmp:vec4:all-negative-masked", "gap_gmp:vec4:channel-passes>1", "gap_gmp:vec4:masked-lanes", "gap_gmp_levels:1-map",
    "gap_gmp_levels:2..GROUP_MAX-maps", "gap_gmp_levels:>GROUP_MAX-maps", "in_stats:rep_pad",
    "in_stats:scalar:channel-passes>1", "in_stats:scalar:masked-lanes", "in_stats:vec4:channel-passes>1",
    "in_stats:vec4:masked-lanes", "reduce:chunk1024", "reduce:chunk128", "reduce:chunk256", "reduce:chunk512",
    "reduce:chunk64", "reduce:ragged-chunk",
}


def _of(op):
    return [c for c in C.CASES if c.op == op]


def _close(a, b, tol=1e-12):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    s = max(np.abs(b).max(), 1e-300)
    assert np.abs(a - b).max() <= tol * s, np.abs(a - b).max() / s


def _small(c):
    return c.p.get("H", 1) * c.p.get("W", 1) < BIG


# ------------------------------------------------------------------------------------------------------ reference checks
@pytest.mark.parametrize("c", [c for c in _of("in_stats") if _small(c)], ids=lambda c: c.id)
def test_statistics_reference_is_instance_norm(c):
    """scale / shift of the reference normalise the (replication-padded) tensor as F.instance_norm does, then StyleMod and the bias"""
    inp, r, p = C.inputs(c.id), C.reference(c.id), c.p
    x = C._nchw(C._sl(c, inp, "x").double())
    xp = F.pad(x, [1, 1, 1, 1], mode="replicate") if p.get("rep_pad") else x
    _close(r["sum"], xp.sum((2, 3)).numpy())
    _close(r["sumsq"], (xp * xp).sum((2, 3)).numpy())
    want = F.instance_norm(xp, eps=1e-5)
    if p.get("rep_pad"):
        want = want[:, :, 1:-1, 1:-1]
    if "style" in inp:
        st = inp["style"].double()
        want = want * (st[:, :p["C"], None, None] + 1) + st[:, p["C"]:, None, None] + inp["post_bias"].double()[None, :, None, None]
    got = torch.from_numpy(r["scale"])[:, :, None, None] * x + torch.from_numpy(r["shift"])[:, :, None, None]
    _close(got.numpy(), want.numpy(), 1e-10)
    import ppst_oracle as O
    if not p.get("rep_pad") and "style" not in inp:
        _close(got.numpy(), O.instance_norm(x).numpy(), 1e-10)


def test_bilerp_is_F_interpolate():
    g = torch.Generator().manual_seed(3)
    for c in _of("bilinear"):
        x = C._sl(c, C.inputs(c.id), "x").double()
        want = F.interpolate(C._nchw(x), size=(c.p["OH"], c.p["OW"]), mode="bilinear", align_corners=False)
        _close(C.reference(c.id)["y"], C._nhwc(want).numpy())
    for h, w in ((1, 1), (3, 5), (6, 2)):                           # the x2 form of res_up2 / torgb_apply
        r = torch.randn(2, h, w, 4, generator=g, dtype=torch.float64)
        want = F.interpolate(C._nchw(r), scale_factor=2, mode="bilinear", align_corners=False)
        _close(C.bilerp(r, 2 * h, 2 * w, torch.float64).numpy(), C._nhwc(want).numpy())


@pytest.mark.parametrize("c", _of("avgpool") + _of("maxpool2") + _of("upsample_nearest2"), ids=lambda c: c.id)
def test_pooling_references_are_torch(c):
    x = C._nchw(C._sl(c, C.inputs(c.id), "x", C=c.p["C"]).double())
    if c.op == "avgpool":
        want = F.avg_pool2d(x, c.p["f"])
    elif c.op == "maxpool2":
        want = F.max_pool2d(x, 2)
    else:
        want = F.interpolate(x, scale_factor=2, mode="nearest")
    _close(C.reference(c.id)["y"], C._nhwc(want).numpy(), 0)


@pytest.mark.parametrize("c", _of("head_tail"), ids=lambda c: c.id)
def test_head_tail_reference_is_avg_pool_and_interpolate(c):
    inp, r, p = C.inputs(c.id), C.reference(c.id), c.p
    f = C._aff(C._sl(c, inp, "x").double(), inp["ss"], torch.float64)
    if p.get("act") == C.ACT_LRELU:
        f = F.leaky_relu(f, 0.2) * 2 ** 0.5
    elif p.get("act") == C.ACT_PRELU:
        f = F.prelu(f, inp["prelu"].double())
    f = C._nchw(f)
    _close(r["feat"], C._nhwc(F.avg_pool2d(f, p["P"])).numpy())
    _close(r["feat1"], C._nhwc(F.interpolate(f, size=(p["H"] // p["D"], p["W"] // p["D"]), mode="bilinear", align_corners=False)).numpy())


@pytest.mark.parametrize("c", _of("blur_nhwc"), ids=lambda c: c.id)
def test_blur_reference_is_the_oracle_upfirdn2d_on_the_padded_normalised_tensor(c):
    import ppst_oracle as O
    inp, p = C.inputs(c.id), c.p
    x = C._aff(inp["x"].double(), inp.get("ss"), torch.float64)
    if p.get("in_ss") == "lrelu":
        x = F.leaky_relu(x, 0.2) * 2 ** 0.5
    x = C._nchw(x)
    p0, p1 = p["pads"]
    if p.get("mode"):
        y = O.upfirdn2d(F.pad(x, [p0, p1, p0, p1], mode="reflect"), inp["k"].double(), down=p.get("down", 1), pad=(0, 0))
    else:
        y = O.upfirdn2d(x, inp["k"].double(), down=p.get("down", 1), pad=(p0, p1))
    y = C._nhwc(y)
    assert tuple(y.shape[1:3]) == C.blur_out_hw(p)
    if p.get("s2d"):
        oh, ow = y.shape[1:3]
        y = F.pixel_unshuffle(F.pad(C._nchw(y), [0, ow % 2, 0, oh % 2]), 2)                     # (B, C * 4, oh2, ow2), phase minor
        B, _, oh2, ow2 = y.shape
        y = y.view(B, p["C"], 4, oh2, ow2).permute(0, 3, 4, 2, 1).reshape(B, oh2, ow2, 4 * p["C"])
    _close(C.reference(c.id)["y"], y.numpy())


@pytest.mark.parametrize("c", _of("conv1x1_small_cin") + _of("conv1x1_small_cout") + _of("torgb_apply"), ids=lambda c: c.id)
def test_small_conv_references_are_F_conv2d(c):
    inp, p = C.inputs(c.id), c.p
    if c.op == "torgb_apply":
        x = C._aff(inp["x"].double(), inp["ss"], torch.float64)
        if "res" in inp:
            x = x + C._nhwc(F.interpolate(C._nchw(C._sl(c, inp, "res").double()), scale_factor=2, mode="bilinear", align_corners=False))
        x = x * p["out_scale"]
    else:
        x = C._sl(c, inp, "x", C=p["cin"]).double()
    y = F.conv2d(C._nchw(x), inp["w"].double() * p["wscale"], inp["bias"].double() if p.get("bias", True) else None)
    if p.get("act") == C.ACT_LRELU:
        assert y.abs().min() >= 1e-3
        y = F.leaky_relu(y, 0.2) * 2 ** 0.5
    _close(C.reference(c.id)["y"], C._nhwc(y).numpy())


def test_tensor2im_reference_is_the_oracle():
    import ppst_oracle as O
    for c in _of("tensor2im_u8"):
        assert np.array_equal(C.reference(c.id)["y"], O.tensor2im(C.inputs(c.id)["x"]).astype(np.float64))


def test_lerp_reference_is_the_oracle():
    import ppst_oracle as O
    for c in _of("lerp"):
        inp = C.inputs(c.id)
        for i in range(len(c.p["sizes"])):
            _close(C.reference(c.id)["y%d" % i], O.lerp(inp["a%d" % i].double(), inp["b%d" % i].double(), c.p["r"]).numpy())


@pytest.mark.parametrize("c", _of("affine_act") + _of("affine_act_stats"), ids=lambda c: c.id)
def test_affine_act_reference_is_the_torch_composition(c):
    inp, p = C.inputs(c.id), c.p
    t = C._aff(C._sl(c, inp, "x").double(), inp.get("ss"), torch.float64)
    r = 0
    if "res" in inp:
        r = C._sl(c, inp, "res").double()
        if p["res"] == "up2":
            r = C._nhwc(F.interpolate(C._nchw(r), scale_factor=2, mode="bilinear", align_corners=False))
        r = C._aff(r, inp.get("rss"), torch.float64)
    act = {C.ACT_NONE: lambda v: v, C.ACT_LRELU: lambda v: F.leaky_relu(v, 0.2) * 2 ** 0.5,
           C.ACT_PRELU: lambda v: F.prelu(v, inp["prelu"].double())}[p.get("act", 0)]
    y = (act(t + r) if p.get("before") else act(t) + r) * p.get("out_scale", 1.0)
    _close(C.reference(c.id)["y"], y.numpy())
    if p.get("act"):
        assert (t + r if p.get("before") else t).abs().min() >= 1e-3, "a gate input on the boundary"
    if p.get("st", "f32") != "f32":                    # the stored operands are what the storage type holds
        for k in ("x", "res"):
            if k in inp:
                assert torch.equal(inp[k], inp[k].to(C.HALF[p["st"]]).float())


@pytest.mark.parametrize("c", _of("gap_gmp") + _of("gap_gmp_multi"), ids=lambda c: c.id)
def test_pooled_reference_is_mean_and_amax_of_the_products(c):
    inp, r, p = C.inputs(c.id), C.reference(c.id), c.p
    x = C._sl(c, inp, "x")
    heads = [inp.get("mask")] if c.op == "gap_gmp" else C._gm_heads(c, inp)
    for h, m in enumerate(heads):
        mx = x if m is None else x * m[..., None]
        if m is not None:
            assert torch.equal(mx.double(), x.double() * m.double()[..., None]), "a product m x is not exact in float32"
        rows = slice(h * p["B"], (h + 1) * p["B"])
        assert np.array_equal(r["max"][rows], torch.amax(mx, (1, 2)).double().numpy())
        _close(r["mean"][rows], F.adaptive_avg_pool2d(C._nchw(mx.double()), 1).flatten(1).numpy())
        if p.get("allneg"):
            ch = torch.amax(mx, (1, 2))[:, 1]
            assert bool((ch == 0).all()) if (m is not None and bool((m == 0).any())) else bool((ch < 0).all())


# ----------------------------------------------------------------------------------------------------------- sensitivity
@pytest.mark.parametrize("cid", IDS)
def test_bar_passes_the_reference_and_rejects_every_seeded_defect(cid):
    c = C.by_id(cid)
    ref = C.reference(cid)
    for k, v in ref.items():
        bad, _ = C.judge(c, k, C.as_stored(c, k, v))
        assert not bad, "%s: the reference, rounded once to its storage type, misses its own bar: %s" % (k, bad)
    muts = C.mutations(c)
    assert len(muts) >= 2, "a case carries at least two seeded defects"
    for name, out in muts:
        assert set(out) <= set(ref)
        seen = [k for k, v in out.items() if C.judge(c, k, C.as_stored(c, k, v))[0]]
        assert seen, "the inputs of %s cannot show the defect '%s' at the bar" % (cid, name)


@pytest.mark.parametrize("cid", IDS)
def test_float32_evaluation_passes_its_own_bar(cid):
    c = C.by_id(cid)
    r32 = C.OPS[c.op].ref(c, C.inputs(cid), torch.float32)
    for k, v in r32.items():
        bad, _ = C.judge(c, k, C.as_stored(c, k, v.double().numpy()))
        assert not bad, (k, bad)


def test_every_listed_kind_of_defect_occurs():
    kinds = set()
    for c in C.CASES:
        if _small(c):
            kinds.update(n for n, _ in C.mutations(c))
    for want in ("zero padding applied before normalise-on-load", "odd s2d row or column left non-zero", "last sliding band's rows dropped",
                 "last column strip dropped", "last pixel chunk dropped", "rep_pad corner weight 2 instead of 4", "mean divided by the mask count",
                 "max taken over x, not m x", "residual on the wrong side of the activation", "res_scale_shift ignored",
                 "up2 sample shifted by half a pixel", "up2 border not clamped", "ss of batch row 0 used for every row", "slice offset ignored",
                 "tail channels zero", "feat1 written at the wrong D", "out_scale applied before the residual"):
        assert want in kinds, want


@pytest.mark.parametrize("st", ["f16", "bf16"])
def test_half_bar_accepts_one_rounding_and_rejects_one_ulp_on_one_percent(st):
    g = torch.Generator().manual_seed(11)
    ref = (torch.randn(4096, generator=g, dtype=torch.float64) * 3).clamp(-60, 60)
    ref = torch.where(ref.abs() < 0.05, ref.sign() * 0.05 + (ref == 0) * 0.05, ref)         # (inside fp16's normal range)
    h = ref.to(C.HALF[st])
    assert not C.compare_half(ref.numpy(), h.double().numpy(), C.BAR_EW, st)[0]
    # a value the fp32 launch may produce (within b s of ref), rounded once, passes as well
    near = ref + C.BAR_EW * float(ref.abs().max()) * torch.sign(torch.randn(4096, generator=g, dtype=torch.float64))
    assert not C.compare_half(ref.numpy(), near.to(C.HALF[st]).double().numpy(), C.BAR_EW, st)[0]
    bits = h.view(torch.int16).clone()
    hit = torch.randperm(4096, generator=g)[:41]                    # 1 % of the elements, one ulp away from zero
    bits[hit] += 1
    off = bits.view(C.HALF[st]).double()
    assert bool((off != h.double()).sum() == 41)
    bad, _ = C.compare_half(ref.numpy(), off.numpy(), C.BAR_EW, st)
    assert bad, "an error of one ulp on 1 % of the elements passes the half bar"


def test_stored_operands_are_what_their_storage_type_holds():
    for c in C.CASES:
        st = c.p.get("st", "f32")
        if st != "f32":
            for k, v in C.inputs(c.id).items():
                if k == "x" or k == "res" or (k.startswith("x") and k[1:].isdigit()):
                    assert torch.equal(v, v.to(C.HALF[st]).float()), (c.id, k)


def test_bars_print():
    """the bar of every case and output, and the float32-reference error it was taken from (pytest -s shows the table)"""
    for c in C.CASES:
        for k, e in C.err32(c.id).items():
            b = C.bar(c, k)
            print("%-64s %-6s bar %.2e  (float32 reference error %.2e)  %s" % (c.id, k, b, e, C.branch_of(c)))
            assert b == 0 or b < 1e-4, "a bar this wide says the case is ill-conditioned: fix the inputs"


# -------------------------------------------------------------------------------------------------------------- coverage
def test_every_form_and_every_facet_has_a_case():
    assert {C.branch_of(c) for c in C.CASES} == FORMS
    assert {f for c in C.CASES for f in C.facets_of(c)} == FACETS


def test_the_table_of_the_issue_is_present():
    st = _of("in_stats")
    assert {c.p["C"] for c in st} >= {3, 12, 20, 64, 258, 1028}
    assert {C.pix_chunk(c.p["H"] * c.p["W"]) for c in st if c.p["B"] == 1 and c.p["C"] == 4} >= {128, 256, 512, 1024}
    assert all(c.p["B"] == 1 and c.p["C"] == 4 for c in C.CASES if not _small(c)), "the chunk-size cases are the only large inputs"
    for c in C.CASES:
        if _small(c) and "H" in c.p:
            assert c.p.get("C", 4) * c.p["H"] * c.p["W"] <= 64 * 64 * 64, c.id
    assert any(c.p["B"] == 3 for c in st) and any(c.p.get("style") for c in st) and any(c.p.get("rep_pad") for c in st)
    aa = _of("affine_act")
    assert {(c.p.get("res"), bool(c.p.get("before"))) for c in aa} >= {(None, False), ("plain", False), ("plain", True), ("up2", False), ("up2", True)}
    assert {c.p.get("act", 0) for c in aa} == {0, 1, 2} and any(c.p.get("rss") for c in aa) and any(not c.p.get("ss") for c in aa)
    assert all(any(c.p.get(n + "_ld") for c in aa) for n in ("x", "res", "out"))
    assert any(c.p.get("res") == "up2" and (c.p["H"], c.p["W"]) == (2, 2) for c in aa) and any(c.p.get("res") == "up2" and c.p["H"] != c.p["W"] for c in aa)
    assert {(c.p["P"], c.p["D"]) for c in _of("head_tail")} == {(a, b) for a in (2, 4, 8) for b in (1, 2)}
    assert {c.p.get("act", 0) for c in _of("head_tail")} == {0, 1, 2} and all(c.p["H"] != c.p["W"] for c in _of("head_tail"))
    assert {c.p["f"] for c in _of("avgpool")} == {1, 2, 4, 8} and any(c.p["H"] != c.p["W"] for c in _of("avgpool"))
    assert any(c.p["H"] % 2 and c.p["W"] % 2 for c in _of("maxpool2"))
    sl = [c for c in _of("blur_nhwc") if C.blur_form(c)[1]]
    assert {C.blur_form(c)[2] for c in sl} == {192, 198, 209} and {c.p["C"] for c in sl} == {4, 12}
    assert {(bool(c.p.get("s2d")), c.p.get("mode", 0), bool(c.p.get("in_ss"))) for c in sl} >= {(True, 0, True), (True, 1, False), (False, 0, False), (False, 1, True)}
    assert {c.p["pads"] for c in _of("blur_nhwc")} == {(1, 1), (2, 1), (2, 2), (1, 0)}
    off4 = [c for c in _of("blur_nhwc") if c.p.get("off")]
    assert {(c.p["st"], c.p["off"], c.p["B"], c.p["H"], c.p["W"], c.p["C"], c.p["ks"], c.p["pads"]) for c in off4} == {(s, 4, 2, 7, 10, 8, 3, (1, 1)) for s in ("bf16", "f16")}
    assert {C.branch_of(c) for c in off4} == {"blur:k3:%s:CV4:patch:plain" % s for s in ("bf16", "f16")}
    assert all(C.blur_form(c._replace(p=dict(c.p, off=0)))[0] == 8 for c in off4), "on the 16-byte grid the same tensor takes 8 channels"
    assert {c.p["cin"] for c in _of("conv1x1_small_cin")} == {1, 2, 3, 4} and {c.p["cout"] for c in _of("conv1x1_small_cin")} == {4, 32, 36}
    assert {c.p["cout"] for c in _of("conv1x1_small_cout")} == {1, 2, 3, 4}
    assert any(c.p["cout"] == 3 and c.p["npix"] % 8 for c in _of("conv1x1_small_cout"))
    assert {(c.p.get("st", "f32"), bool(c.p.get("res"))) for c in _of("torgb_apply")} == {(s, r) for s in ("f32", "f16", "bf16") for r in (True, False)}
    assert {len(c.p["maps"]) for c in _of("gap_gmp_levels")} >= {1, 4, C.GROUP_MAX + 3}
