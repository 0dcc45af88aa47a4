"""Tuning aid (not a test): time the LPIPS-AlexNet metric alone -- forward, and forward + backward to ``a`` -- by HIP events.

    python tests/lpips_time.py [--B 2] [--size 512] [--reps 50] [--once]

--once: one warm-up and one forward + backward only (the run to put under ``rocprofv3 --kernel-trace --stats --``).
Weights: LPIPSAlex.synthetic_state_dict(1); inputs as in tests/test_gpu_lpips.py.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ppst_amd import weights as W                      # noqa: E402
from ppst_amd.lpips import LPIPSAlex                   # noqa: E402


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
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=2)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--once", action="store_true")
    o = ap.parse_args()
    m = LPIPSAlex.from_state_dict(LPIPSAlex.synthetic_state_dict(1))
    x = W.synthetic_images(3, 2 * o.B, size=o.size).cuda()
    a = (0.7 * x[:o.B] + 0.3 * x[o.B:]).requires_grad_(True)
    b = x[o.B:].contiguous()

    def fwd():
        with torch.no_grad():
            m(a, b)

    def fwd_bwd():
        a.grad = None
        m(a, b).sum().backward()

    fwd_bwd()
    torch.cuda.synchronize()
    if o.once:
        fwd_bwd()
        torch.cuda.synchronize()
        return
    for _ in range(5):
        fwd()
        fwd_bwd()
    torch.cuda.synchronize()
    f = timed(fwd, o.reps)
    fb = timed(fwd_bwd, o.reps)
    print("LPIPS-alex B=%d %dx%d on %s, %d reps (median / min / max ms)" % (o.B, o.size, o.size, torch.cuda.get_device_name(0), o.reps))
    print("  forward             %.3f / %.3f / %.3f" % f)
    print("  forward + backward  %.3f / %.3f / %.3f   (gradient to a only)" % fb)


if __name__ == "__main__":
    main()
