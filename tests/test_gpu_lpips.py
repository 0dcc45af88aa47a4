"""GPU: the LPIPS-AlexNet metric (ppst_amd/lpips.py, csrc/lpips.hip) against a float64 PyTorch-CPU restatement of its
definition, synthetic weights ``LPIPSAlex.synthetic_state_dict(1)`` -- pytest -m gpu.

Bars (none of them taken from the device's own output):
  * features: each of the five maps within 3e-5 of the map's max-norm (the project's fp32-class conv bar);
  * value: relative error <= 1e-3 (the project's bar for a whole network);
  * gradient with the gates REPLAYED -- the float64 backward takes its ReLU masks and pool arg-max from the device's own
    feature maps, so that a decision within rounding of a tie cannot move single elements by O(1) --: within 1e-3 of the
    gradient's max-norm, for a alone, b alone and both;
  * gates: per layer the ReLU + pool decisions that differ from the free float64 forward are at most 1e-3 of the layer's
    decisions (or 2); torch-CPU fp32's own counts are printed beside the device's;
  * free-running gradient: cosine >= 0.99 against the float64 gradient (coarse guard; the relative L2 is printed, beside
    torch-fp32's own, and is not a bar).
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SLICE = ((1, 0), (2, 3), (3, 6), (4, 8), (5, 10))
PADS = (2, 2, 1, 1, 1)


# ---- the definition, restated (float64 on the CPU when fed float64) ------------------------------------------------------
def _trunk(sd, x, gates=None):
    """the five post-ReLU maps; gates = (relu masks [5], pool indices [2]) replaces the decisions by recorded ones"""
    dt = x.dtype
    x = (x - sd["scaling_layer.shift"].to(dt)) / sd["scaling_layer.scale"].to(dt)
    feats = []
    for l, (s, i) in enumerate(SLICE):
        pre = F.conv2d(x, sd["net.slice%d.%d.weight" % (s, i)].to(dt), sd["net.slice%d.%d.bias" % (s, i)].to(dt),
                       stride=4 if l == 0 else 1, padding=PADS[l])
        f = F.relu(pre) if gates is None else pre * gates[0][l].to(dt)
        feats.append(f)
        if l < 2:
            if gates is None:
                x = F.max_pool2d(f, 3, 2)
            else:
                idx = gates[1][l]
                x = f.flatten(2).gather(2, idx.flatten(2)).view(idx.shape)
        else:
            x = f
    return feats


def _safe_norm(f):
    """sqrt(sum_c f^2) whose derivative at 0 is 0 (the project's definition; equal to the plain form everywhere else)"""
    s = (f * f).sum(1, keepdim=True)
    pos = s > 0
    return torch.where(pos, torch.where(pos, s, torch.ones_like(s)).sqrt(), torch.zeros_like(s))


def _lpips(sd, a, b, gates_a=None, gates_b=None):
    fa, fb = _trunk(sd, a, gates_a), _trunk(sd, b, gates_b)
    out = 0
    for l in range(5):
        d = (fa[l] / (_safe_norm(fa[l]) + 1e-10) - fb[l] / (_safe_norm(fb[l]) + 1e-10)) ** 2
        out = out + (d * sd["lin%d.model.1.weight" % l].to(a.dtype)).sum(1, keepdim=True).mean((2, 3), keepdim=True)
    return out


def _gates_of(feats):
    """decisions of a forward, read off its feature maps: ReLU masks and the pools' arg-max"""
    masks = [f > 0 for f in feats]
    idx = [F.max_pool2d(f, 3, 2, return_indices=True)[1] for f in feats[:2]]
    return masks, idx


def _flips(g1, g2):
    """per layer (differing decisions, decisions): ReLU masks + pool arg-max"""
    out = []
    for l in range(5):
        n, k = g1[0][l].numel(), int((g1[0][l] != g2[0][l]).sum())
        if l < 2:
            n, k = n + g1[1][l].numel(), k + int((g1[1][l] != g2[1][l]).sum())
        out.append((k, n))
    return out


def _grad(sd, a, b, dtype, gates_a=None, gates_b=None, gout=None):
    a, b = a.detach().clone().to(dtype).requires_grad_(True), b.detach().clone().to(dtype).requires_grad_(True)
    out = _lpips(sd, a, b, gates_a, gates_b)
    (out.sum() if gout is None else (out * gout.to(dtype)).sum()).backward()
    return out.detach(), a.grad, b.grad


def _images(S, H=None, W=None, n=4):
    from ppst_amd import weights as W_
    x = W_.synthetic_images(3, n, size=S)
    if H is not None:
        x = x[:, :, :H, :W].contiguous()
    h = n // 2
    return 0.7 * x[:h] + 0.3 * x[h:], x[h:].clone()


@pytest.fixture(scope="module")
def sd():
    from ppst_amd.lpips import LPIPSAlex
    return LPIPSAlex.synthetic_state_dict(1)


@pytest.fixture(scope="module")
def metric(sd):
    from ppst_amd.lpips import LPIPSAlex
    return LPIPSAlex.from_state_dict(sd)


def _device_grads(metric, a, b, which, gout=None):
    ad = a.detach().cuda().requires_grad_("a" in which)
    bd = b.detach().cuda().requires_grad_("b" in which)
    out = metric(ad, bd)
    (out.sum() if gout is None else (out * gout.cuda()).sum()).backward()
    torch.cuda.synchronize()
    return out.detach().cpu(), (ad.grad.cpu() if ad.grad is not None else None), (bd.grad.cpu() if bd.grad is not None else None)


CASES = [("512", 512, None, None), ("256", 256, None, None), ("272x208", 272, 272, 208), ("31", 31, None, None)]


@pytest.mark.parametrize("name,S,H,W", CASES, ids=[c[0] for c in CASES])
def test_against_float64(metric, sd, name, S, H, W):
    a, b = _images(S, H, W)
    B = a.shape[0]
    # ---- the float64 truth and torch's own fp32 run on the same inputs
    out64, ga64, gb64 = _grad(sd, a, b, torch.float64)
    out32, ga32, gb32 = _grad(sd, a, b, torch.float32)
    with torch.no_grad():
        f64 = _trunk(sd, torch.cat((a, b)).double())
        f32 = _trunk(sd, torch.cat((a, b)))
    g64, g32 = _gates_of(f64), _gates_of(f32)
    print("\n[%s] value f64 %s" % (name, out64.flatten().tolist()))
    print("[%s] smallest channel norm over the layers: %.3g" % (name, min(float(_safe_norm(f).min()) for f in f64)))
    print("[%s] torch-fp32 value rel err %.2e; flips per layer %s" % (name, float(((out32 - out64).abs() / out64.abs()).max()), _flips(g32, g64)))
    # ---- features
    fd = [f.cpu() for f in metric.features(torch.cat((a, b)).cuda())]
    for l in range(5):
        assert fd[l].shape == f64[l].shape and fd[l].dtype == torch.float32
        err = float((fd[l].double() - f64[l]).abs().max() / f64[l].abs().max())
        err32 = float((f32[l].double() - f64[l]).abs().max() / f64[l].abs().max())
        print("[%s] relu%d %s: device %.2e, torch-fp32 %.2e of the max-norm" % (name, l + 1, tuple(fd[l].shape), err, err32))
        assert err <= 3e-5, (l, err)
    # ---- gates
    gd = _gates_of(fd)
    flips = _flips(gd, g64)
    print("[%s] device flips per layer (differing, decisions): %s" % (name, flips))
    for l, (k, n) in enumerate(flips):
        assert k <= max(2, 1e-3 * n), (l, k, n)
    # ---- value and gradients: a alone, b alone, both
    ha = B
    gates_a = ([m[:ha] for m in gd[0]], [i[:ha] for i in gd[1]])
    gates_b = ([m[ha:] for m in gd[0]], [i[ha:] for i in gd[1]])
    _, ga_r, gb_r = _grad(sd, a, b, torch.float64, gates_a, gates_b)
    res = {w: _device_grads(metric, a, b, w) for w in ("a", "b", "ab")}
    for w, (out, ga, gb) in res.items():
        assert out.shape == (B, 1, 1, 1)
        rel = float(((out.double() - out64).abs() / out64.abs()).max())
        print("[%s] grads to %s: value rel err %.2e" % (name, w, rel))
        assert rel <= 1e-3
        assert (ga is None) == ("a" not in w) and (gb is None) == ("b" not in w)
        for tag, g, gr, gfree, g32_ in (("a", ga, ga_r, ga64, ga32), ("b", gb, gb_r, gb64, gb32)):
            if g is None:
                continue
            assert g.shape == gr.shape and bool(torch.isfinite(g).all())
            replay = float((g.double() - gr).abs().max() / gr.abs().max())
            cos = float(F.cosine_similarity(g.double().flatten(), gfree.flatten(), dim=0))
            l2 = float((g.double() - gfree).norm() / gfree.norm())
            l2_32 = float((g32_.double() - gfree).norm() / gfree.norm())
            print("[%s] d/d%s (asked: %s): replayed max-norm err %.2e; free cosine %.6f, rel L2 %.2e (torch-fp32: %.2e)"
                  % (name, tag, w, replay, cos, l2, l2_32))
            assert replay <= 1e-3, (tag, w, replay)
            assert cos >= 0.99, (tag, w, cos)
    # the half that is asked for alone equals the one computed with both, bit for bit
    assert torch.equal(res["a"][1], res["ab"][1]) and torch.equal(res["b"][2], res["ab"][2])
    assert torch.equal(res["a"][0], res["ab"][0])


def test_bit_identical_repeat_and_weighted_grad_output(metric, sd):
    a, b = _images(256)
    go = torch.tensor([0.25, -3.0]).view(2, 1, 1, 1)
    r1 = _device_grads(metric, a, b, "ab", go)
    r2 = _device_grads(metric, a, b, "ab", go)
    for t1, t2 in zip(r1, r2):
        assert torch.equal(t1, t2)
    gd = _gates_of([f.cpu() for f in metric.features(torch.cat((a, b)).cuda())])
    _, ga_r, gb_r = _grad(sd, a, b, torch.float64, ([m[:2] for m in gd[0]], [i[:2] for i in gd[1]]),
                          ([m[2:] for m in gd[0]], [i[2:] for i in gd[1]]), gout=go)
    for g, gr in ((r1[1], ga_r), (r1[2], gb_r)):
        assert float((g.double() - gr).abs().max() / gr.abs().max()) <= 1e-3


def test_equal_inputs_give_exactly_zero(metric):
    a, _ = _images(256)
    out, ga, gb = _device_grads(metric, a, a.clone(), "ab")
    assert torch.equal(out, torch.zeros_like(out))
    assert torch.equal(ga, torch.zeros_like(ga)) and torch.equal(gb, torch.zeros_like(gb))


def test_zero_norm_pixels_have_zero_not_nan_gradient(sd):
    """conv1 with negative biases and an image region that equals the scaling layer's shift: the scaled input is 0 there, the
    first map's pixels whose window lies inside it are all-zero, and autograd of the plain formula gives NaN.  The device's
    gradient is finite and equals the float64 gradient of the definition with d sqrt / d0 := 0, gates replayed."""
    from ppst_amd.lpips import LPIPSAlex
    sd = dict(sd)
    sd["net.slice1.0.bias"] = -(sd["net.slice1.0.bias"].abs() + 0.05)
    m = LPIPSAlex.from_state_dict(sd)
    a, b = _images(256)
    shift = sd["scaling_layer.shift"].view(3, 1, 1)
    a[:, :, :, :128] = shift
    b[:, :, 64:, :96] = shift
    fd = [f.cpu() for f in m.features(torch.cat((a, b)).cuda())]
    zero_pix = int((fd[0].abs().sum(1) == 0).sum())
    print("\nall-zero pixels of relu1: %d of %d" % (zero_pix, fd[0][:, 0].numel()))
    assert zero_pix > 1000
    # autograd of the plain formula gives NaN at such a pixel (d sqrt / d0 = inf, times 0): what the definition replaces.  (Through
    # the whole network torch's ReLU backward masks it again; a caller of the tail alone would see it.)
    f1 = fd[0][:2].double().requires_grad_(True)
    ((f1 / (f1.pow(2).sum(1, keepdim=True).sqrt() + 1e-10) - fd[0][2:].double()) ** 2).sum().backward()
    assert not bool(torch.isfinite(f1.grad).all())
    out, ga, gb = _device_grads(m, a, b, "ab")
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(ga).all()) and bool(torch.isfinite(gb).all())
    gd = _gates_of(fd)
    out_r, ga_r, gb_r = _grad(sd, a, b, torch.float64, ([x[:2] for x in gd[0]], [x[:2] for x in gd[1]]), ([x[2:] for x in gd[0]], [x[2:] for x in gd[1]]))
    assert float(((out.double() - out_r).abs() / out_r.abs()).max()) <= 1e-3
    for g, gr in ((ga, ga_r), (gb, gb_r)):
        assert float(gr.abs().max()) > 0
        assert float((g.double() - gr).abs().max() / gr.abs().max()) <= 1e-3


@pytest.mark.parametrize("B", [1, 3])
def test_batch_one_and_odd_batch(metric, sd, B):
    from ppst_amd import weights as W_
    x = W_.synthetic_images(5, 2 * B, size=96)
    a, b = 0.7 * x[:B] + 0.3 * x[B:], x[B:].clone()
    out, ga, gb = _device_grads(metric, a, b, "ab")
    out64, _, _ = _grad(sd, a, b, torch.float64)
    assert out.shape == (B, 1, 1, 1) and float(((out.double() - out64).abs() / out64.abs()).max()) <= 1e-3
    # every image pair is computed on its own: the batch equals its single pairs, bit for bit
    for i in range(B):
        o1, g1, _ = _device_grads(metric, a[i:i + 1], b[i:i + 1], "a")
        assert torch.equal(o1[0], out[i]) and torch.equal(g1[0], ga[i])


def test_non_contiguous_input_and_side_stream(metric):
    a, b = _images(256)
    ref = _device_grads(metric, a, b, "ab")
    # channels-last storage behind an NCHW view, and a strided crop of a wider tensor
    ad = a.cuda().permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2).requires_grad_(True)
    wide = torch.zeros(2, 3, 256, 300, device="cuda")
    wide[..., 20:276] = b.cuda()
    bd = wide[..., 20:276].requires_grad_(True)
    assert not ad.is_contiguous() and not bd.is_contiguous()
    out = metric(ad, bd)
    out.sum().backward()
    assert torch.equal(out.cpu(), ref[0]) and torch.equal(ad.grad.cpu(), ref[1]) and torch.equal(bd.grad.cpu(), ref[2])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        a2, b2 = a.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
        out2 = metric(a2, b2)
        out2.sum().backward()
    side.synchronize()
    assert torch.equal(out2.cpu(), ref[0]) and torch.equal(a2.grad.cpu(), ref[1]) and torch.equal(b2.grad.cpu(), ref[2])


def test_too_small_image_is_refused(metric):
    x = torch.zeros(1, 3, 30, 64, device="cuda")
    with pytest.raises(RuntimeError, match="31"):
        metric(x, x)
    with pytest.raises(RuntimeError, match="shape"):
        metric(torch.zeros(1, 3, 64, 64, device="cuda"), torch.zeros(2, 3, 64, 64, device="cuda"))


def test_cycwarp_term_in_the_generator_step(sd):
    """Options(training_stage=2, lambda_Cycwarp=5) with the "lpips" metric: ``image_warp_reg`` = 5 x the metric evaluated by the
    module on the inference-path double warp (the construction of test_cycwarp_branch_with_injected_metric, same 2e-3); G's
    gradient differs from the lambda = 0 run, E1 / E2's are bit-equal to it (the correspondence heads read x.detach())."""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import gstep_diag as D
    from ppst_amd import weights as W_
    from ppst_amd.lpips import LPIPSAlex
    from ppst_amd.ppst_model import Options, create_model
    real, mask, noise = D.gstep_inputs()
    real, mask = real.cuda(), mask.cuda()
    lp = {"loss_fn_alex." + k: v for k, v in sd.items()}
    grads = {}
    for lam in (0.0, 5.0):
        wsd = W_.make_state_dict(17, bias_std=0.1, noise_weight=0.1)
        m = create_model(Options(training_stage=2, lambda_Cycwarp=lam), state_dict=wsd, with_D=True, with_nce=True)
        m.noise = {k: v.cuda() for k, v in noise.items()}
        if lam > 0.0:
            with pytest.raises(RuntimeError, match="perceptual_metric"):
                m.trainer().losses_and_grads(real, mask)
            m.set_perceptual_metric("lpips", state_dict=lp, prefix="loss_fn_alex.")
            assert isinstance(m.perceptual_metric, LPIPSAlex) and len(m.state_dict()) == len(wsd)
        out = m.trainer().losses_and_grads(real, mask)
        grads[lam] = {k: f.grad.clone() for k, f in m.trainer().fp.items()}
        if lam > 0.0:
            v = out["image_warp_reg"].detach().float().cpu().flatten()
            assert bool(torch.isfinite(v).all()) and float(v.min()) > 0.0
            with torch.no_grad():
                fea, fea1 = m.extract_feat_from_image(real)
                sps = torch.cat((fea, m.Rselfcorr(fea1)), dim=1)
                corr = m.corrm(sps, m.swap(sps))
                rec = m.warp(m.warp(real, corr), m.swap(corr))
                ref = 5.0 * m.perceptual_metric(rec, real).float().cpu().flatten()
            print("\nimage_warp_reg", v.tolist(), "5 x metric on the inference-path double warp", ref.tolist())
            assert v.shape == ref.shape == (real.shape[0],)
            assert bool(((v - ref).abs() <= 2e-3 * ref).all()), (v, ref)
        else:
            assert "image_warp_reg" not in out
    assert not torch.equal(grads[0.0]["G"], grads[5.0]["G"])
    for k in ("E1", "E2"):
        assert torch.equal(grads[0.0][k], grads[5.0][k]), k
