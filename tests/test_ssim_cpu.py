"""CPU: the float64 judge of the image-quality metrics (tests/ssim_cases.py) pinned three ways -- a second form written
independently, closed forms, central differences -- so that it is not its own witness; and what of ppst_amd/metrics.py,
the ppst_ssim_* / ppst_sqerr entry points (include/ppst_hip.h) and the model's "ssim" metric can be checked without a GPU.
Nothing here launches a kernel."""
import ctypes
import math

import pytest
import torch

import ssim_cases as S


def _loop_ssim(a, b, L):
    """per output pixel: explicit loops over the 11 x 11 window with the outer-product weights (no convolution, no
    separability), plain Python floats"""
    g = [float(v) for v in S.window()]
    B, C, H, W = a.shape
    C1, C2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    A, Bt = a.tolist(), b.tolist()
    out = []
    for n in range(B):
        tot = 0.0
        for c in range(C):
            for y in range(H - 10):
                for x in range(W - 10):
                    ma = mb = saa = sbb = sab = 0.0
                    for i in range(11):
                        for j in range(11):
                            w = g[i] * g[j]
                            va, vb = A[n][c][y + i][x + j], Bt[n][c][y + i][x + j]
                            ma += w * va; mb += w * vb
                            saa += w * va * va; sbb += w * vb * vb; sab += w * va * vb
                    va, vb, cov = saa - ma * ma, sbb - mb * mb, sab - ma * mb
                    tot += (2 * ma * mb + C1) / (ma * ma + mb * mb + C1) * (2 * cov + C2) / (va + vb + C2)
        out.append(tot / (C * (H - 10) * (W - 10)))
    return torch.tensor(out, dtype=torch.float64)


def test_judge_against_the_loop_form():
    a, b = S.make_pair(3, 3, 2, 13, 14)
    a, b = a.double(), b.double()
    ref, got = _loop_ssim(a, b, 2.0), S.ssim(a, b, 2.0)
    err = (ref - got).abs().max().item()
    print("\nloop form vs conv form at 13 x 14:", ref.tolist(), "err %.3g" % err)
    assert err <= 1e-12
    assert ref.min().item() < 0.1 and 0.9 < ref.max().item() < 1.0      # the three noise levels spread the values


def test_judge_closed_forms():
    a, b = S.make_pair(4, 3, 3, 24, 29)
    a, b = a.double(), b.double()
    assert (S.ssim(a, a, 2.0) - 1.0).abs().max().item() <= 1e-12                               # ssim(x, x) = 1
    assert (S.ssim(a, b, 2.0) - S.ssim(b, a, 2.0)).abs().max().item() <= 1e-14                  # symmetry
    for c, d in ((0.3, -0.7), (0.0, 0.0), (1.0, 0.25)):                                          # constants: the luminance term alone
        ca, cb = torch.full((1, 2, 15, 17), c, dtype=torch.float64), torch.full((1, 2, 15, 17), d, dtype=torch.float64)
        C1, C2 = (0.01 * 2.0) ** 2, (0.03 * 2.0) ** 2
        got = S.ssim(ca, cb, 2.0).item()
        # the window is rounded to fp32 AFTER it was normalised, so its 2-D sum is s = 1 - delta (delta about 2e-9), not 1:
        # mu = s c, var = s (1 - s) c^2, cov = s (1 - s) c d.  With s the closed form is exact; without it, it holds to
        # delta (c - d)^2 / C2 (the cs term's deviation from 1)
        s = float(S.window().sum()) ** 2
        exact = ((2 * s * s * c * d + C1) / (s * s * (c * c + d * d) + C1)
                 * (2 * s * (1 - s) * c * d + C2) / (s * (1 - s) * (c * c + d * d) + C2))
        assert abs(got - exact) <= 1e-12
        assert abs(got - (2 * c * d + C1) / (c * c + d * d + C1)) <= 1.1 * abs(1 - s) * ((c - d) ** 2 / C2 + 1.0) + 1e-12
    for k in (0.5, 127.5, 3.0):                                                                  # (k a, k b, k L) gives the same value
        assert (S.ssim(k * a, k * b, k * 2.0) - S.ssim(a, b, 2.0)).abs().max().item() <= 1e-12
    a, b = S.make_pair(5, 2, 1, 176, 181)
    a, b = a.double(), b.double()
    assert (S.ms_ssim(a, a, 2.0) - 1.0).abs().max().item() <= 1e-12                             # MS-SSIM of equal images
    v = S.ms_ssim(a, b, 2.0)
    assert bool(((v > 0.0) & (v < 1.0)).all())
    assert math.isinf(S.psnr(a, a, 2.0)[0].item())
    assert abs(S.psnr(torch.zeros(1, 1, 4, 4, dtype=torch.float64), torch.full((1, 1, 4, 4), 0.2, dtype=torch.float64), 2.0).item()
               - 10 * math.log10(4 / 0.04)) <= 1e-12


def test_judge_gradient_against_central_differences():
    a, b = S.make_pair(6, 2, 1, 12, 13)
    a, b = a.double(), b.double()
    gout = torch.tensor([0.7, -1.3], dtype=torch.float64)
    grad = S.ssim_grad(a, b, gout, 2.0)
    h = 1e-6
    num = torch.zeros_like(a)
    flat, nflat = a.view(-1), num.view(-1)
    for i in range(flat.numel()):
        keep = flat[i].item()
        flat[i] = keep + h
        up = (S.ssim(a, b, 2.0) * gout).sum().item()
        flat[i] = keep - h
        dn = (S.ssim(a, b, 2.0) * gout).sum().item()
        flat[i] = keep
        nflat[i] = (up - dn) / (2 * h)
    err = (grad - num).abs().max().item() / grad.abs().max().item()
    print("\nautograd vs central differences at 12 x 13: relative err %.3g" % err)
    assert err <= 1e-7


def test_inputs_cover_the_range():
    """the seeded inputs spread SSIM over about 0.04 .. 0.99 and MS-SSIM over about 0.5 .. 0.99 (what the GPU tests rely on)"""
    a, b = S.make_pair(11, 3, 3, 64, 64)
    v = S.ssim(a.double(), b.double(), 2.0)
    print("\nssim at 64 x 64:", v.tolist())
    assert v[0] > 0.9 and v[2] < 0.15
    a, b = S.make_pair(12, 3, 1, 176, 177)
    m = S.ms_ssim(a.double(), b.double(), 2.0)
    print("ms-ssim at 176 x 177:", m.tolist())
    assert m[0] > 0.95 and 0.2 < m[2] < 0.8


def test_argument_errors_need_no_gpu():
    from ppst_amd._lib import lib
    tok = ctypes.c_void_p(16)          # a non-null token: validation runs before anything is dereferenced or launched
    st = (ctypes.c_int64 * 4)(3 * 16 * 16, 16 * 16, 16, 1)
    fwd = lambda a, sa, b, sb, u8, B, C, H, W, L, out, s, cs, ws: lib.ppst_ssim_forward(a, sa, b, sb, u8, B, C, H, W, L, out, s, cs, ws, None)
    ok = (tok, st, tok, st)
    assert fwd(*ok, 0, 1, 3, 10, 16, 2.0, tok, tok, tok, tok) == -1           # H < 11
    assert fwd(*ok, 0, 1, 3, 16, 10, 2.0, tok, tok, tok, tok) == -1           # W < 11
    assert fwd(*ok, 0, -1, 3, 16, 16, 2.0, tok, tok, tok, tok) == -1          # B < 0
    assert fwd(*ok, 0, 1, 0, 16, 16, 2.0, tok, tok, tok, tok) == -1           # C < 1
    assert fwd(*ok, 0, 1, 3, 16, 16, 0.0, tok, tok, tok, tok) == -1           # data range
    assert fwd(*ok, 2, 1, 3, 16, 16, 2.0, tok, tok, tok, tok) == -1           # no such input type
    assert fwd(*ok, 0, 2, 3, 40000, 40000, 2.0, tok, tok, tok, tok) == -1     # beyond 32-bit element indices
    assert fwd(None, None, None, None, 0, 2, 3, 40000, 40000, 2.0, None, None, None, None) == -1    # ... ahead of the null check
    assert fwd(None, None, None, None, 0, 0, 3, 16, 16, 2.0, None, None, None, None) == 0           # empty batch
    for hole in range(4):
        args = list(ok)
        args[hole] = None
        assert fwd(*args, 0, 1, 3, 16, 16, 2.0, tok, tok, tok, tok) == -3
    assert fwd(*ok, 0, 1, 3, 16, 16, 2.0, tok, None, tok, tok) == -3
    assert fwd(*ok, 0, 1, 3, 16, 16, 2.0, tok, tok, None, tok) == -3
    assert fwd(*ok, 0, 1, 3, 16, 16, 2.0, tok, tok, tok, None) == -3
    assert lib.ppst_ssim_ws(1, 3, 10, 16) == -1 and lib.ppst_ssim_ws(-1, 3, 16, 16) == -1 and lib.ppst_ssim_ws(1, 3, 16, 16) > 0
    assert lib.ppst_ssim_ws(0, 3, 16, 16) >= 0 and lib.ppst_ssim_ws(2, 3, 40000, 40000) == -1

    bwd = lambda a, sa, b, sb, g, B, C, H, W, L, grad: lib.ppst_ssim_backward(a, sa, b, sb, g, B, C, H, W, L, grad, None)
    assert bwd(*ok, tok, 1, 3, 10, 16, 2.0, tok) == -1
    assert bwd(*ok, tok, 1, 3, 16, 10, 2.0, tok) == -1
    assert bwd(*ok, tok, -1, 3, 16, 16, 2.0, tok) == -1
    assert bwd(*ok, tok, 1, 0, 16, 16, 2.0, tok) == -1
    assert bwd(*ok, tok, 1, 3, 16, 16, -1.0, tok) == -1
    assert bwd(*ok, tok, 2, 3, 40000, 40000, 2.0, tok) == -1
    assert bwd(None, None, None, None, None, 0, 3, 16, 16, 2.0, None) == 0
    assert bwd(*ok, None, 1, 3, 16, 16, 2.0, tok) == -3
    assert bwd(*ok, tok, 1, 3, 16, 16, 2.0, None) == -3
    assert bwd(None, st, tok, st, tok, 1, 3, 16, 16, 2.0, tok) == -3
    assert bwd(tok, st, tok, None, tok, 1, 3, 16, 16, 2.0, tok) == -3

    assert lib.ppst_pool2x2(tok, st, 0, 1, 3, 1, 16, tok, None) == -1         # nothing to pool
    assert lib.ppst_pool2x2(tok, st, 3, 1, 3, 16, 16, tok, None) == -1
    assert lib.ppst_pool2x2(tok, st, 0, -1, 3, 16, 16, tok, None) == -1
    assert lib.ppst_pool2x2(None, None, 0, 0, 3, 16, 16, None, None) == 0
    assert lib.ppst_pool2x2(None, st, 0, 1, 3, 16, 16, tok, None) == -3
    assert lib.ppst_pool2x2(tok, None, 0, 1, 3, 16, 16, tok, None) == -3
    assert lib.ppst_pool2x2(tok, st, 0, 1, 3, 16, 16, None, None) == -3

    assert lib.ppst_msssim_combine(tok, -1, 3, tok, None) == -1 and lib.ppst_msssim_combine(tok, 1, 0, tok, None) == -1
    assert lib.ppst_msssim_combine(None, 0, 3, None, None) == 0
    assert lib.ppst_msssim_combine(None, 1, 3, tok, None) == -3 and lib.ppst_msssim_combine(tok, 1, 3, None, None) == -3

    sq = lambda a, sa, b, sb, u8, B, C, H, W, L, out, ws: lib.ppst_sqerr(a, sa, b, sb, u8, B, C, H, W, L, out, ws, None)
    assert sq(*ok, 0, 1, 3, 0, 16, 2.0, tok, tok) == -1
    assert sq(*ok, 0, 1, 0, 16, 16, 2.0, tok, tok) == -1
    assert sq(*ok, 0, -1, 3, 16, 16, 2.0, tok, tok) == -1
    assert sq(*ok, 0, 1, 3, 16, 16, 0.0, tok, tok) == -1
    assert sq(*ok, 5, 1, 3, 16, 16, 2.0, tok, tok) == -1
    assert sq(*ok, 0, 2, 3, 40000, 40000, 2.0, tok, tok) == -1
    assert sq(None, None, None, None, 0, 0, 3, 16, 16, 2.0, None, None) == 0
    assert sq(*ok, 0, 1, 3, 16, 16, 2.0, None, tok) == -3
    assert sq(*ok, 0, 1, 3, 16, 16, 2.0, tok, None) == -3
    assert sq(tok, None, tok, st, 0, 1, 3, 16, 16, 2.0, tok, tok) == -3
    assert lib.ppst_sqerr_ws(1, 3, 0, 16) == -1 and lib.ppst_sqerr_ws(1, 3, 16, 16) > 0
    assert lib.ppst_version() == 3                                              # no struct or existing entry point changed


def test_metrics_refuse_cpu_tensors():
    from ppst_amd import metrics
    a = torch.zeros(1, 3, 176, 176)
    for fn in (metrics.psnr, metrics.ssim, metrics.ms_ssim, metrics.l1, metrics.SSIMLoss()):
        with pytest.raises(RuntimeError, match="CUDA"):
            fn(a, a)
    with pytest.raises(RuntimeError, match="CUDA"):
        metrics.ssim(torch.zeros(1, 16, 16, 3, dtype=torch.uint8), torch.zeros(1, 16, 16, 3, dtype=torch.uint8))


def test_ms_ssim_below_176_is_a_value_error():
    """refused from the shape alone, ahead of everything else (so it can be seen without a GPU)"""
    from ppst_amd import metrics, ops
    for H, W in ((175, 176), (176, 175), (64, 64)):
        x = torch.zeros(1, 3, H, W)
        with pytest.raises(ValueError, match="176"):
            metrics.ms_ssim(x, x)
    u = torch.zeros(1, 175, 200, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="176"):
        metrics.ms_ssim(u, u)
    assert ops.MS_SSIM_MIN_SIDE == 176


def test_ssim_metric_is_outside_the_checkpoint_contract():
    from ppst_amd import weights as W_
    from ppst_amd.metrics import SSIMLoss
    from ppst_amd.ppst_model import Options
    from ppst_amd.ppst_model import PPSTModel
    m = PPSTModel(Options(), with_D=False)
    m.load_weights(W_.make_state_dict(3, with_D=False, with_nce=False))
    keys = list(m.state_dict())
    assert m.perceptual_metric is None
    assert m.set_perceptual_metric("ssim") is m
    assert isinstance(m.perceptual_metric, SSIMLoss)
    assert list(m.state_dict()) == keys and not any(isinstance(c, SSIMLoss) for c in m.modules())
    with pytest.raises(ValueError, match="unknown perceptual metric"):
        m.set_perceptual_metric("psnr")
    fn = lambda a, b: (a - b).abs().mean()
    assert m.set_perceptual_metric(fn).perceptual_metric is fn                  # callables keep working
