"""GPU: SSIM / MS-SSIM / PSNR and the SSIM gradient (ppst_amd/metrics.py, csrc/ssim.hip) against the float64 judge of
tests/ssim_cases.py (pinned on the CPU by test_ssim_cpu.py), and their places in the Cycwarp term, in
``evaluation.evaluate_reconstruction`` and in ``train_loop(evaluator=...)`` -- pytest -m gpu.

The bar of every comparison is the project's rule for fp32 streaming kernels (tests/BACKWARD_KERNELS.md section 3), computed per
case, never a constant chosen here: ``max(2e-6, 4 x |float32 torch evaluation of the judge - its float64 evaluation|)``; absolute
for the per-image values (they lie in [-1, 1]), relative to max |ref| for the gradient, relative to the mean squared error for
PSNR.  Each test prints its err / bar table (-s shows it).  Which kernel edge each shape reaches: ssim_cases.SSIM_SHAPES.
"""
import math
import os

import pytest
import torch

import ssim_cases as S

pytestmark = pytest.mark.gpu

L = 2.0
_CASES = {}


def _case(shape, seed=None):
    """inputs, float64 references and bars of one shape -- computed once, shared by the tests, never written to"""
    name, B, C, H, W = shape
    if name not in _CASES:
        a, b = S.make_pair(seed if seed is not None else 100 + len(_CASES), B, C, H, W)
        a64, b64 = a.double(), b.double()
        gout = torch.tensor([0.7, -1.3, 2.1, 0.4][:B], dtype=torch.float32)
        c = dict(a=a, b=b, gout=gout)
        c["ssim"] = S.ssim(a64, b64, L)
        c["ssim_bar"] = S.bar_from(c["ssim"], S.ssim(a, b, L))
        c["grad"] = S.ssim_grad(a64, b64, gout.double(), L)
        c["grad_bar"] = S.bar_from(c["grad"], S.ssim_grad(a, b, gout, L), relative=True)
        c["mse"], c["l1"] = S.mse(a64, b64), S.l1(a64, b64)
        c["mse_bar"] = max(2e-6, 4.0 * ((S.mse(a, b).double() - c["mse"]).abs() / c["mse"]).max().item())
        c["l1_bar"] = max(2e-6, 4.0 * ((S.l1(a, b).double() - c["l1"]).abs() / c["l1"]).max().item())
        _CASES[name] = c
    return _CASES[name]


def _row(what, name, err, bar):
    print("  %-10s %-12s err %.3g  bar %.3g" % (what, name, err, bar))


@pytest.mark.parametrize("shape", S.SSIM_SHAPES, ids=[s[0] for s in S.SSIM_SHAPES])
def test_ssim_psnr_and_gradient_against_float64(shape):
    from ppst_amd import metrics, ops
    c = _case(shape)
    a = c["a"].cuda().requires_grad_(True)
    b = c["b"].cuda()
    got = metrics.ssim(a, b)
    assert got.shape == (shape[1],) and got.dtype == torch.float32
    (got * c["gout"].cuda()).sum().backward()
    assert a.grad.shape == a.shape and a.grad.is_contiguous()
    print()
    err = S.error_of(c["ssim"], got.detach())
    _row("ssim", shape[0], err, c["ssim_bar"])
    assert err <= c["ssim_bar"]
    gerr = S.error_of(c["grad"], a.grad, relative=True)
    _row("grad", shape[0], gerr, c["grad_bar"])
    assert gerr <= c["grad_bar"]                                   # gout's different weights per image are in the reference
    sq = ops.sqerr(a.detach(), b).cpu().double()
    merr = ((sq[:, 0] - c["mse"]).abs() / c["mse"]).max().item()
    _row("mse", shape[0], merr, c["mse_bar"])
    assert merr <= c["mse_bar"]
    lerr = ((sq[:, 1] - c["l1"]).abs() / c["l1"]).max().item()
    _row("l1", shape[0], lerr, c["l1_bar"])
    assert lerr <= c["l1_bar"]
    psnr = metrics.psnr(a.detach(), b).cpu().double()
    assert (psnr - 10.0 * torch.log10(L * L / sq[:, 0])).abs().max().item() <= 1e-5        # the same pass: PSNR of that mse
    # the per-(image, channel) means behind the per-image value
    _, s_bc, cs_bc = ops.ssim_forward(a.detach(), b)
    smap, csmap = S.ssim_maps(c["a"].double(), c["b"].double(), L)
    s32, cs32 = S.ssim_maps(c["a"], c["b"], L)
    for what, g, ref, r32 in (("ssim_bc", s_bc, smap.mean(dim=(2, 3)), s32.mean(dim=(2, 3))), ("cs_bc", cs_bc, csmap.mean(dim=(2, 3)), cs32.mean(dim=(2, 3)))):
        bar = S.bar_from(ref, r32)
        e = S.error_of(ref, g)
        _row(what, shape[0], e, bar)
        assert e <= bar


def test_non_contiguous_view_on_a_side_stream():
    """33 x 70 handed over as a channel slice of a wider channels-last tensor (strides (H W 5, 1, W 5, 5)), on a side stream"""
    from ppst_amd import metrics, ops
    shape = S.SSIM_SHAPES[-1]
    assert shape[0] == "33x70"
    c = _case(shape)
    B, C, H, W = shape[1:]

    def view_of(t):
        wide = torch.full((B, H, W, 5), 9.0, device="cuda")
        v = wide.permute(0, 3, 1, 2)[:, 1:4]
        v.copy_(t)
        assert not v.is_contiguous() and v.stride() == (H * W * 5, 1, W * 5, 5)
        return v

    a, b = view_of(c["a"].cuda()), view_of(c["b"].cuda())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        a.requires_grad_(True)
        got = metrics.ssim(a, b)
        (got * c["gout"].cuda()).sum().backward()
        sq = ops.sqerr(a.detach(), b)
    side.synchronize()
    print()
    err, gerr = S.error_of(c["ssim"], got.detach()), S.error_of(c["grad"], a.grad, relative=True)
    _row("ssim", "33x70 view", err, c["ssim_bar"])
    _row("grad", "33x70 view", gerr, c["grad_bar"])
    assert err <= c["ssim_bar"] and gerr <= c["grad_bar"]
    assert ((sq[:, 0].cpu().double() - c["mse"]).abs() / c["mse"]).max().item() <= c["mse_bar"]
    # the same bits as from the contiguous copies (the walk order of the SSIM kernels does not depend on the layout)
    a2 = c["a"].cuda().requires_grad_(True)
    got2 = metrics.ssim(a2, c["b"].cuda())
    (got2 * c["gout"].cuda()).sum().backward()
    assert torch.equal(got2.detach(), got.detach()) and torch.equal(a2.grad, a.grad)


def test_uint8_images():
    """uint8 (B, H, W, 3) as glue.tensor2im makes them, data range 255 by default; the judge runs at L = 255 on the raw values"""
    from ppst_amd import metrics, ops
    name, B, C, H, W = S.U8_SHAPE
    a, b = S.make_pair(41, B, C, H, W)
    ua, ub = S.to_u8(a), S.to_u8(b)
    ra, rb = S.from_u8(ua), S.from_u8(ub)
    ref = S.ssim(ra, rb, 255.0)
    bar = S.bar_from(ref, S.ssim(ra.float(), rb.float(), 255.0))
    got = metrics.ssim(ua.cuda(), ub.cuda())
    err = S.error_of(ref, got)
    print()
    _row("ssim", name, err, bar)
    assert got.shape == (B,) and err <= bar
    mse = S.mse(ra, rb)
    mbar = max(2e-6, 4.0 * ((S.mse(ra.float(), rb.float()).double() - mse).abs() / mse).max().item())
    sq = ops.sqerr(ua.cuda(), ub.cuda()).cpu().double()
    merr = ((sq[:, 0] - mse).abs() / mse).max().item()
    _row("mse", name, merr, mbar)
    assert merr <= mbar
    assert (metrics.psnr(ua.cuda(), ub.cuda()).cpu().double() - S.psnr(ra, rb, 255.0)).abs().max().item() <= 1e-4
    assert ((sq[:, 1] - S.l1(ra, rb)).abs() / S.l1(ra, rb)).max().item() <= 2e-6
    with pytest.raises(RuntimeError, match="forward only"):
        ops.ssim_backward(ua.cuda(), ub.cuda(), torch.ones(B, device="cuda"))
    with pytest.raises(RuntimeError, match="differ"):
        metrics.ssim(ua.cuda(), b.cuda())


@pytest.mark.parametrize("shape", S.MS_SHAPES, ids=[s[0] for s in S.MS_SHAPES])
def test_ms_ssim_against_float64(shape):
    from ppst_amd import metrics
    name, B, C, H, W = shape
    a, b = S.make_pair(51 + H, B, C, H, W)
    ref = S.ms_ssim(a.double(), b.double(), L)
    bar = S.bar_from(ref, S.ms_ssim(a, b, L))
    got = metrics.ms_ssim(a.cuda(), b.cuda())
    err = S.error_of(ref, got)
    print()
    _row("ms_ssim", name, err, bar)
    print("   values", ref.tolist())
    assert got.shape == (B,) and err <= bar
    assert torch.equal(got, metrics.ms_ssim(a.cuda(), b.cuda()))                      # bit-identical repeats
    one = metrics.ms_ssim(a.cuda(), a.cuda())
    assert (one.cpu().double() - 1.0).abs().max().item() <= S.bar_from(torch.ones(B, dtype=torch.float64), S.ms_ssim(a, a, L))
    with pytest.raises(ValueError, match="176"):
        metrics.ms_ssim(a.cuda()[:, :, :175], b.cuda()[:, :, :175])


def test_repeats_are_bit_identical():
    from ppst_amd import metrics, ops
    c = _case(S.SSIM_SHAPES[1])                                                        # 12 x 75, B = 3
    a, b, w = c["a"].cuda(), c["b"].cuda(), c["gout"].cuda()
    runs = []
    for _ in range(3):
        x = a.clone().requires_grad_(True)
        v = metrics.ssim(x, b)
        (v * w).sum().backward()
        runs.append((v.detach(), x.grad, ops.sqerr(a, b)))
    for r in runs[1:]:
        assert all(torch.equal(p, q) for p, q in zip(runs[0], r))
    # an image's value does not depend on its batch (the partial sums are per plane)
    assert torch.equal(metrics.ssim(a[1:2], b[1:2]), runs[0][0][1:2])
    # gout's weights: the gradient of image n scales with gout[n] alone
    x = a.clone().requires_grad_(True)
    metrics.ssim(x, b).sum().backward()
    for n in range(a.shape[0]):
        e = (x.grad[n] * w[n] - runs[0][1][n]).abs().max().item() / runs[0][1][n].abs().max().item()
        assert e <= 1e-6, (n, e)


def test_equal_and_constant_images():
    from ppst_amd import metrics
    c = _case(S.SSIM_SHAPES[3])                                                        # 64 x 64
    a = c["a"].cuda()
    one = metrics.ssim(a, a.clone())
    bar = S.bar_from(torch.ones(a.shape[0], dtype=torch.float64), S.ssim(c["a"], c["a"], L))
    err = (one.cpu().double() - 1.0).abs().max().item()
    print()
    _row("ssim(x,x)", "64x64", err, bar)
    assert err <= bar
    p = metrics.psnr(a, a.clone())
    assert bool(torch.isinf(p).all()) and bool((p > 0).all())
    assert bool((metrics.l1(a, a.clone()) == 0).all())
    # constant images: the luminance term alone, (2 c d + C1) / (c^2 + d^2 + C1)
    C1 = (0.01 * L) ** 2
    for cv, dv in ((0.3, -0.7), (0.0, 0.0), (0.8, 0.25)):
        ca, cb = torch.full((2, 3, 20, 45), cv), torch.full((2, 3, 20, 45), dv)
        closed = torch.full((2,), (2 * cv * dv + C1) / (cv * cv + dv * dv + C1), dtype=torch.float64)
        bar = S.bar_from(S.ssim(ca.double(), cb.double(), L), S.ssim(ca, cb, L))
        err = S.error_of(closed, metrics.ssim(ca.cuda(), cb.cuda()))
        _row("constant", "%g,%g" % (cv, dv), err, bar)
        assert err <= bar
    # SSIMLoss: 1 - ssim in the shape LPIPSAlex returns
    loss = metrics.SSIMLoss()(a, c["b"].cuda())
    assert loss.shape == (a.shape[0], 1, 1, 1)
    assert S.error_of(1.0 - c["ssim"], loss.flatten()) <= c["ssim_bar"]


def test_cycwarp_term_with_the_ssim_metric():
    """Options(training_stage=2, lambda_Cycwarp=5) with the "ssim" metric: ``image_warp_reg`` = 5 x the metric on the
    inference-path double warp (the construction of test_gpu_lpips.py::test_cycwarp_term_in_the_generator_step, same 2e-3), every
    gradient of the step finite; G's gradient differs from the lambda = 0 run, E1 / E2's are bit-equal to it."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import gstep_diag as D
    from ppst_amd import weights as W_
    from ppst_amd.metrics import SSIMLoss
    from ppst_amd.ppst_model import Options, create_model
    real, mask, noise = D.gstep_inputs()
    real, mask = real.cuda(), mask.cuda()
    grads = {}
    for lam in (0.0, 5.0):
        wsd = W_.make_state_dict(17, bias_std=0.1, noise_weight=0.1)
        m = create_model(Options(training_stage=2, lambda_Cycwarp=lam), state_dict=wsd, with_D=True, with_nce=True)
        m.noise = {k: v.cuda() for k, v in noise.items()}
        if lam > 0.0:
            with pytest.raises(RuntimeError, match="perceptual_metric"):
                m.trainer().losses_and_grads(real, mask)
            m.set_perceptual_metric("ssim")
            assert isinstance(m.perceptual_metric, SSIMLoss) and len(m.state_dict()) == len(wsd)
        out = m.trainer().losses_and_grads(real, mask)
        grads[lam] = {k: f.grad.clone() for k, f in m.trainer().fp.items()}
        assert all(bool(torch.isfinite(g).all()) for g in grads[lam].values())
        if lam > 0.0:
            v = out["image_warp_reg"].detach().float().cpu().flatten()
            assert bool(torch.isfinite(v).all()) and float(v.min()) > 0.0
            with torch.no_grad():
                fea, fea1 = m.extract_feat_from_image(real)
                sps = torch.cat((fea, m.Rselfcorr(fea1)), dim=1)
                corr = m.corrm(sps, m.swap(sps))
                rec = m.warp(m.warp(real, corr), m.swap(corr))
                ref = 5.0 * m.perceptual_metric(rec, real).float().cpu().flatten()
                judge = 5.0 * (1.0 - S.ssim(rec.cpu().double(), real.cpu().double(), L))
            print("\nimage_warp_reg", v.tolist(), "5 x (1 - ssim) on the inference-path double warp", ref.tolist(), "judge", judge.tolist())
            assert v.shape == ref.shape == (real.shape[0],)
            assert bool(((v - ref).abs() <= 2e-3 * ref).all()), (v, ref)
            assert (ref.double() - judge).abs().max().item() <= 5.0 * S.bar_from(judge / 5.0, 1.0 - S.ssim(rec.cpu(), real.cpu(), L))
        else:
            assert "image_warp_reg" not in out
    assert not torch.equal(grads[0.0]["G"], grads[5.0]["G"])
    for k in ("E1", "E2"):
        assert torch.equal(grads[0.0][k], grads[5.0][k]), k


def test_evaluate_reconstruction_and_content_preservation():
    """a seeded model at 512^2 (no noise): every number evaluate_reconstruction returns equals the judge on the DEVICE-made
    reconstructions copied to the CPU -- the metric is judged, not the network"""
    from ppst_amd import evaluation as EV
    from ppst_amd import weights as W
    from ppst_amd.lpips import LPIPSAlex
    from ppst_amd.ppst_model import create_model
    sd = W.make_state_dict(2, with_D=False, with_nce=False, bias_std=0.1)
    m = create_model(state_dict=sd, device="cuda")
    m.noise = None
    x = W.synthetic_images(31, 3, size=512).cuda()
    res = EV.evaluate_reconstruction(m, x, batch=2)                                    # 3 images in batches of 2: a ragged tail
    assert sorted(res) == ["l1", "ms_ssim", "psnr", "ssim"]
    assert all(v.shape == (3,) and v.dtype == torch.float32 and v.is_cuda for v in res.values())
    with torch.no_grad():
        rec = torch.cat([m(*m(x[i:i + 2], command="encode"), target=None, command="decode") for i in (0, 2)], 0)
    r32, x32 = rec.cpu(), x.cpu()
    r64, x64 = r32.double(), x32.double()
    print()
    for name, ref, v32 in (("ssim", S.ssim(r64, x64, L), S.ssim(r32, x32, L)), ("ms_ssim", S.ms_ssim(r64, x64, L), S.ms_ssim(r32, x32, L))):
        bar, err = S.bar_from(ref, v32), S.error_of(ref, res[name])
        _row(name, "rec 512", err, bar)
        print("   values", ref.tolist())
        assert err <= bar
    mse = S.mse(r64, x64)
    mbar = max(2e-6, 4.0 * ((S.mse(r32, x32).double() - mse).abs() / mse).max().item())
    got_mse = L * L * 10.0 ** (-res["psnr"].cpu().double() / 10.0)
    merr = ((got_mse - mse).abs() / mse).max().item()
    _row("psnr (mse)", "rec 512", merr, mbar)
    assert merr <= mbar
    l1 = S.l1(r64, x64)
    lbar = max(2e-6, 4.0 * ((S.l1(r32, x32).double() - l1).abs() / l1).max().item())
    lerr = ((res["l1"].cpu().double() - l1).abs() / l1).max().item()
    _row("l1", "rec 512", lerr, lbar)
    assert lerr <= lbar
    # with an LPIPSAlex installed the same call reports it too: the module's own value on the same reconstructions
    lp = LPIPSAlex.from_state_dict(LPIPSAlex.synthetic_state_dict(1))
    m.set_perceptual_metric(lp)
    res2 = EV.evaluate_reconstruction(m, x[:2], batch=8)
    assert sorted(res2) == ["l1", "lpips", "ms_ssim", "psnr", "ssim"]
    assert torch.equal(res2["lpips"], lp(rec[:2], x[:2]).flatten()) and torch.equal(res2["ssim"], res["ssim"][:2])
    # content preservation: SSIM(content, output) per pair, from a tensor or from swapping_grid's dict
    cp = EV.content_preservation(x, rec)
    assert torch.equal(cp, res["ssim"])
    as_dict = EV.content_preservation(x, {(0, 1): rec[0], (2, 0): rec[2]})
    assert sorted(as_dict) == [(0, 1), (2, 0)]
    assert as_dict[(0, 1)] == float(res["ssim"][0]) and as_dict[(2, 0)] == float(res["ssim"][2])


def test_train_loop_with_a_held_out_evaluator(tmp_path):
    """evaluation_freq = one batch: the evaluator fires on every iteration after the first (IterationCounter.needs_evaluation);
    one line per firing in eval_log.txt and through ``log``, every result in ``.history``.  Without an evaluator: no such line,
    no file, and ``evaluation_freq`` is not even needed."""
    from ppst_amd import weights as W
    from ppst_amd.ppst_model import Options, create_model
    from ppst_amd.train_g import PPSTOptimizer
    from ppst_amd.training import HeldOutEvaluator, SyntheticMaskDataset, train_loop
    held_out = W.synthetic_images(77, 2, size=512).cuda()
    for with_eval in (True, False):
        name = "with" if with_eval else "without"
        kw = dict(training_stage=2, lambda_Cycwarp=0.0, checkpoints_dir=str(tmp_path), name=name, isTrain=True, batch_size=2,
                  total_nimgs=1000, save_freq=1000, print_freq=1000, local_rank=0, continue_train=False, dataset_mode="celebamask")
        if with_eval:
            kw["evaluation_freq"] = 2
        opt = Options(**kw)
        assert hasattr(opt, "evaluation_freq") == with_eval
        m = create_model(opt, state_dict=W.make_state_dict(3, bias_std=0.1, noise_weight=0.1), with_D=True, with_nce=True)
        ev = HeldOutEvaluator(held_out) if with_eval else None
        logs = []
        train_loop(opt, m, SyntheticMaskDataset(batch_size=2), PPSTOptimizer(m), log=logs.append, max_iterations=2, evaluator=ev)
        path = os.path.join(str(tmp_path), name, "eval_log.txt")
        lines = [s for s in logs if s.startswith("(eval iters:")]
        if with_eval:
            assert len(ev.history) == 1 and ev.history[0][0] == 2 and ev.log_path == path
            res = ev.history[0][1]
            assert {"l1", "psnr", "ssim", "ms_ssim"} == set(res) and all(math.isfinite(v) for v in res.values())
            assert -1.0 <= res["ssim"] <= 1.0 and res["l1"] > 0.0
            with open(path) as f:
                written = f.read().splitlines()
            assert written == lines == [HeldOutEvaluator.format(2, res)]
            print("\n" + written[0])
        else:
            assert not lines and not os.path.exists(path)
