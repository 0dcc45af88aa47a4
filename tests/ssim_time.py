"""Tuning aid (not a test): time the image-quality metric kernels (csrc/ssim.hip) by HIP events, next to a device copy of the
same bytes taken in the same process.

    python tests/ssim_time.py [--B 8] [--C 3] [--sizes 512 1024] [--reps 50] [--step]

Reported per size: the SSIM forward (both inputs read once), the backward alone (both inputs read, the gradient written; its
three intermediate planes are extra traffic and are NOT counted as bytes it must move), the five-scale MS-SSIM (both inputs
once: the pooled copies are extra traffic too) and the squared-error pass; median / min ms over ``reps`` and GB/s of the bytes
each MUST move at the median.  The copy rate is torch's device copy of 2 x the input bytes (read + write).
--step: the generator iteration (losses + grads, B = 2 at 512^2) with lambda_Cycwarp = 5 and the "ssim" metric against the same
iteration with the L1 stand-in tests/test_gpu_gstep.py injects, alternating, minima and medians of 8 runs each.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ppst_amd import ops                               # noqa: E402
from ppst_amd import weights as W                      # noqa: E402


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(reps):
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def kernels(o):
    print("image-quality metrics on %s, B = %d, C = %d, %d reps (median / min ms, GB/s of the bytes that must move at the median)"
          % (torch.cuda.get_device_name(0), o.B, o.C, o.reps))
    for size in o.sizes:
        g = torch.Generator().manual_seed(size)
        a = torch.rand(o.B, o.C, size, size, generator=g).mul_(2).sub_(1).cuda()
        b = (a + 0.1 * torch.randn(a.shape, generator=torch.Generator(device="cuda").manual_seed(1), device="cuda")).clamp_(-1, 1)
        gout = torch.ones(o.B, device="cuda")
        in_bytes = 2 * a.numel() * 4
        dst = torch.empty(2 * a.numel(), device="cuda")
        src = torch.cat((a.flatten(), b.flatten()))
        rows = (("copy (read + write)", lambda: dst.copy_(src), 2 * in_bytes),
                ("ssim forward", lambda: ops.ssim_forward(a, b, 2.0), in_bytes),
                ("ssim backward", lambda: ops.ssim_backward(a, b, gout, 2.0), in_bytes + a.numel() * 4),
                ("ms-ssim (5 scales)", lambda: ops.ms_ssim_forward(a, b, 2.0), in_bytes),
                ("sqerr (psnr, l1)", lambda: ops.sqerr(a, b, 2.0), in_bytes))
        print(" %d x %d (%.1f MB per input)" % (size, size, a.numel() * 4 / 1e6))
        for name, fn, nbytes in rows:
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
            med, lo = timed(fn, o.reps)
            print("  %-22s %8.3f / %8.3f ms   %7.0f GB/s" % (name, med, lo, nbytes / med / 1e6))


def step(o):
    from ppst_amd import autograd as A
    from ppst_amd.ppst_model import Options, create_model
    real = W.synthetic_images(40, 2).cuda()
    g = torch.Generator().manual_seed(7)
    lab = torch.randint(0, 3, (2, 32, 32), generator=g).repeat_interleave(16, 1).repeat_interleave(16, 2)
    mask = torch.nn.functional.one_hot(lab, 3).permute(0, 3, 1, 2).float().contiguous().cuda()
    models = {}
    for name in ("l1", "ssim"):
        m = create_model(Options(training_stage=2, lambda_Cycwarp=5.0), state_dict=W.make_state_dict(0, bias_std=0.1, noise_weight=0.1),
                         with_D=True, with_nce=True)
        m.noise = "random"
        m.set_perceptual_metric("ssim" if name == "ssim" else (lambda x, y: A.L1LossFn.apply(x, y, 1.0)))
        models[name] = m
        for _ in range(2):
            m.trainer().losses_and_grads(real, mask)
    torch.cuda.synchronize()
    ts = {k: [] for k in models}
    for _ in range(8):
        for name, m in models.items():
            ts[name].append(timed(lambda: m.trainer().losses_and_grads(real, mask), 1)[0])
    for name, v in ts.items():
        v.sort()
        print("G iteration (losses + grads), Cycwarp %-5s: median %.2f ms  min %.2f  max %.2f  (8 alternating runs)" % (name, v[len(v) // 2], v[0], v[-1]))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--C", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--step", action="store_true")
    o = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    step(o) if o.step else kernels(o)
