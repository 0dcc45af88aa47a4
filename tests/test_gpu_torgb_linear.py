"""GPU: the RGB ends of the swap step -- pytest -m gpu.

(1) ToRGB by linearity (ops.torgb_apply, conv1x1_cout3_lin_kernel): the last upsampling block's merge (a*x + s + up2(skip)) * os is
never formed; the skip is projected to 3 channels at its own resolution and that projection is sampled where the outputs are
stored.  Reference: the unfused formula in float64 on the CPU -- the merge as ppst_affine_act defines it, then the 1x1 conv -- on
the operands as stored.  Bar: the largest absolute error of the new path may be at most TWICE that of the existing two-pass path
(ops.affine_act with res_up2, then ops.conv1x1_small_cout) on the same inputs: taking the skip's 128-term sum in front of the
interpolation changes which roundings happen, not how many.  No absolute bound is derived; both errors are printed (pytest -s).
Inputs have a per-channel mean of the size of their standard deviation (the case behind a leaky ReLU) and s = -a * mean + noise as
an instance norm gives it, so the cancellation between a*x and s is there.
(2) The ToRGB kernels' instance-norm partials against ops.in_stats of the same output, both summed in float64 on the host, and the
one-pass end (ops.rgb_affine_nchw) against nhwc_to_nchw(affine_act(...)), bit for bit: the same arithmetic per element.
(3) FromRGB reading the NCHW image (ops.conv1x1_small_cin_nchw) against the NHWC form on the transposed input, bit for bit: the
same products in the same order.
Shapes: 6 x 10 with B = 2 (60 pixels per image: a group of 8 pixels would straddle the two images in a flat numbering, the last
group is ragged; the 3 x 5 skip meets every edge clamp of the bilinear), 1 x 8, and 24 x 26 (624 pixels: two blocks per image, the
second ragged)."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
OS = 1.0 / math.sqrt(2.0)


def _dev():
    return torch.device("cuda", 0)


def _ops():
    from ppst_amd import ops
    return ops


def _inputs(seed, B, H, W, cin, st, res):
    """operands as stored (CPU): x (B,H,W,cin) and the skip in storage type st, ss (B,cin,2), w (3,cin,1,1), bias (3)"""
    g = torch.Generator().manual_seed(seed)
    mean = (torch.rand(cin, generator=g) + 0.5) * (torch.randint(0, 2, (cin,), generator=g) * 2 - 1).float()
    x = (torch.randn(B, H, W, cin, generator=g) + mean).to(DT[st])
    a = torch.rand(B, cin, generator=g) + 0.5
    s = -a * mean + 0.1 * torch.randn(B, cin, generator=g)
    inp = {"x": x, "ss": torch.stack([a, s], dim=-1).contiguous(), "w": torch.randn(3, cin, 1, 1, generator=g), "bias": torch.randn(3, generator=g)}
    if res:
        ld = cin + 24 if res == "slice" else cin
        wide = (torch.randn(B, H // 2, W // 2, ld, generator=g) + 1.0).to(DT[st])
        inp["skip_wide"], inp["skip_off"] = wide, (8 if res == "slice" else 0)
    return inp


def _skip(inp, cin, dev=None):
    if "skip_wide" not in inp:
        return None
    t = inp["skip_wide"] if dev is None else inp["skip_wide"].to(dev)
    return t[..., inp["skip_off"]:inp["skip_off"] + cin] if t.shape[-1] != cin else t


def _ref64(inp, cin, out_scale, wscale):
    f64 = torch.float64
    x, ss = inp["x"].to(f64), inp["ss"].to(f64)
    m = ss[:, None, None, :, 0] * x + ss[:, None, None, :, 1]
    sk = _skip(inp, cin)
    if sk is not None:
        up = F.interpolate(sk.to(f64).permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
        m = m + up
    m = m * out_scale
    return torch.einsum("bhwi,oi->bhwo", m, inp["w"].to(f64).reshape(3, cin)) * wscale + inp["bias"].to(f64)


LIN = [(B, H, W, cin, st, "dense") for (B, H, W) in ((2, 6, 10),) for cin in (8, 128, 256) for st in DT]
LIN += [(2, 6, 10, 128, st, res) for st in DT for res in ("slice", None)]
LIN += [(2, 24, 26, 128, "f32", "dense")]


@pytest.mark.parametrize("B,H,W,cin,st,res", LIN, ids=lambda v: str(v))
def test_linear_torgb_vs_float64(B, H, W, cin, st, res):
    ops, dev = _ops(), _dev()
    wscale = 1.0 / math.sqrt(cin)
    inp = _inputs(1000 + cin + H, B, H, W, cin, st, res)
    ref = _ref64(inp, cin, OS, wscale)
    x, ss, w, bias = inp["x"].to(dev), inp["ss"].to(dev), inp["w"].to(dev), inp["bias"].to(dev)
    sk = _skip(inp, cin, dev)
    two = ops.conv1x1_small_cout(ops.affine_act(x, ss, res=sk, out_scale=OS, res_up2=sk is not None, out_dtype=torch.float32), w, bias, wscale)
    new = ops.torgb_apply(x, ss, sk, OS, w, bias, wscale)
    torch.cuda.synchronize()
    e_two = (two.double().cpu() - ref).abs().max().item()
    e_new = (new.double().cpu() - ref).abs().max().item()
    print("torgb linear B%d %dx%d cin%d %s skip=%s: max abs err new %.3e two-pass %.3e (|ref| max %.3f)" % (B, H, W, cin, st, res, e_new, e_two, ref.abs().max().item()))
    assert e_new <= 2.0 * e_two, "new %.3e > 2 x two-pass %.3e" % (e_new, e_two)


def _sum64(part):
    return part.double().sum(dim=1).cpu()


@pytest.mark.parametrize("B,H,W,merge", [(2, 6, 10, True), (2, 6, 10, False), (1, 1, 8, False), (2, 24, 26, True), (2, 24, 26, False)], ids=lambda v: str(v))
def test_torgb_partials_and_nchw_end(B, H, W, merge):
    """Both forms of the ToRGB kernel (with the merge and the skip's projection; the plain conv, scale_shift = None): the partials
    (B, n, 3, 2) summed in float64 against ops.in_stats of the same output, 1e-6 relative -- to sum |y| for the sums and to sum y^2
    for the squares, the magnitudes the fp32 accumulations of both sides round at; then the one-pass end against the two passes."""
    ops, dev = _ops(), _dev()
    cin = 128
    inp = _inputs(77 + H, B, H, W, cin, "f32", "dense" if merge else None)
    x, w, bias = inp["x"].to(dev), inp["w"].to(dev), inp["bias"].to(dev)
    if merge:
        y, part = ops.torgb_apply(x, inp["ss"].to(dev), _skip(inp, cin, dev), OS, w, bias, 0.1, stats=True)
    else:
        y, part = ops.torgb_apply(x, None, None, 1.0, w, bias, 0.1, stats=True)
        plain = ops.conv1x1_small_cout(x, w, bias, 0.1)
        assert torch.equal(y, plain), "scale_shift = None: not the plain ToRGB conv"
    assert part.shape[0] == B and tuple(part.shape[2:]) == (3, 2) and part.shape[1] == (H * W + 511) // 512
    got, want = _sum64(part), _sum64(ops.in_stats(y))
    y64 = y.double().cpu().reshape(B, -1, 3)
    scale = torch.stack([y64.abs().sum(1), (y64 * y64).sum(1)], dim=-1)
    exact = torch.stack([y64.sum(1), (y64 * y64).sum(1)], dim=-1)
    rel = ((got - want).abs() / scale).max().item()
    print("torgb partials B%d %dx%d merge=%s: vs in_stats %.3e, vs float64 sums %.3e (relative)" % (B, H, W, merge, rel, ((got - exact).abs() / scale).max().item()))
    assert rel <= 1e-6
    g = torch.Generator().manual_seed(5)
    ss = torch.stack([torch.rand(B, 3, generator=g) + 0.5, torch.randn(B, 3, generator=g)], dim=-1).contiguous().to(dev)
    end = ops.rgb_affine_nchw(y, ss)
    two = ops.nhwc_to_nchw(ops.affine_act(y, ss))
    assert end.shape == (B, 3, H, W) and torch.equal(end, two)


def test_weight_inside_a_flat_parameter_buffer():
    """the trainers keep every parameter as a view of one flat buffer: ToRGB's weight then starts at any 4-byte address"""
    ops, dev = _ops(), _dev()
    inp = _inputs(3, 2, 6, 10, 128, "f32", None)
    x, bias = inp["x"].to(dev), inp["bias"].to(dev)
    flat = torch.zeros(1 + 3 * 128, device=dev)
    w = flat[1:].view(3, 128, 1, 1)
    w.copy_(inp["w"].to(dev))
    assert w.data_ptr() % 16 != 0
    y, part = ops.torgb_apply(x, None, None, 1.0, w, bias, 0.1, stats=True)
    assert torch.equal(y, ops.torgb_apply(x, None, None, 1.0, inp["w"].to(dev), bias, 0.1))


def test_nchw_end_several_blocks():
    ops, dev = _ops(), _dev()
    g = torch.Generator().manual_seed(9)
    y = torch.randn(2, 17, 19, 3, generator=g).to(dev)
    ss = torch.stack([torch.rand(2, 3, generator=g) + 0.5, torch.randn(2, 3, generator=g)], dim=-1).contiguous().to(dev)
    assert torch.equal(ops.rgb_affine_nchw(y, ss), ops.nhwc_to_nchw(ops.affine_act(y, ss)))


@pytest.mark.parametrize("cout", [32, 36])
@pytest.mark.parametrize("st", list(DT))
def test_fromrgb_nchw_equals_nhwc(cout, st):
    """cout 36: 9 lanes per pixel, not a divisor of the block; B = 2, 5 x 7: 35 pixels per plane, unaligned plane starts"""
    ops, dev = _ops(), _dev()
    g = torch.Generator().manual_seed(cout)
    img = torch.randn(2, 3, 5, 7, generator=g).to(dev)
    w, b = torch.randn(cout, 3, 1, 1, generator=g).to(dev), torch.randn(cout, generator=g).to(dev)
    for act in (ops.ACT_LRELU, ops.ACT_NONE):
        want = ops.conv1x1_small_cin(ops.nchw_to_nhwc(img), w, b, 0.37, act, out_dtype=DT[st])
        got = ops.conv1x1_small_cin_nchw(img, w, b, 0.37, act, out_dtype=DT[st])
        assert got.shape == (2, 5, 7, cout) and torch.equal(got, want)
    want64 = F.leaky_relu(torch.einsum("bihw,oi->bhwo", img.double().cpu(), w.double().cpu().reshape(cout, 3)) * 0.37 + b.double().cpu(), 0.2) * math.sqrt(2.0)
    got = ops.conv1x1_small_cin_nchw(img, w, b, 0.37, ops.ACT_LRELU, out_dtype=torch.float32)
    assert (got.double().cpu() - want64).abs().max().item() < 1e-5
