"""Tuning aid (not a test): time the colour-statistics pass (csrc/colour_stats.hip) by HIP events, next to the same statistics
composed from torch ops on the device in the same process.

    python tests/colour_stats_time.py [--reps 30]

Shapes: B = 8 at 512^2 and B = 4 at 1024^2, R = 3 regions (16 x 16 label blocks), P = 16 directions.  Inputs: a smooth synthetic
portrait (weights.synthetic_images) AND a flat single-colour image -- every pixel of a region in one bin, the worst case for the
LDS adds.  The yardstick: torch.bincount over the combined (image, region, projection, bin) index plus the Lab moments (table
gather, 3 x 3 product, cube roots, masked means and centred covariances) in fp32 torch.  Reported: median / min ms over ``reps``
after warm-up, their ratio, and ns per pixel; the kernel reads 3 + 1 bytes per pixel.  Also the W1 kernel over B pairs.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ppst_amd import glue, metrics, ops                # noqa: E402
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


def torch_stats(u8, labels, R, dirs, tab, M):
    """the same outputs from torch ops: (hist (B, R, P, 256), count (B, R), mean (B, R, 3), cov (B, R, 3, 3))"""
    B, H, Wd, _ = u8.shape
    P = dirs.shape[0]
    x = u8.long()
    off = 255 * torch.where(dirs < 0, -dirs, torch.zeros_like(dirs)).sum(1)
    t = ((x.unsqueeze(-2) * dirs).sum(-1) + off) >> 12                                   # (B, H, W, P)
    lab = labels.long()
    ok = lab < R
    base = (torch.arange(B, device=u8.device).view(B, 1, 1) * R + lab.clamp(max=R - 1)) * P
    idx = (base.unsqueeze(-1) + torch.arange(P, device=u8.device)) * 256 + t
    hist = torch.bincount(idx[ok].flatten(), minlength=B * R * P * 256).view(B, R, P, 256)
    lin = tab[x]
    f = lin @ M.T
    f = torch.where(f > (6.0 / 29.0) ** 3, f.clamp(min=1e-30) ** (1.0 / 3.0), f * (841.0 / 108.0) + 4.0 / 29.0)
    cie = torch.stack((116.0 * f[..., 1] - 16.0, 500.0 * (f[..., 0] - f[..., 1]), 200.0 * (f[..., 1] - f[..., 2])), -1).view(B, H * Wd, 3)
    mask = torch.stack([(lab == r) for r in range(R)], 1).view(B, R, H * Wd).float()
    count = mask.sum(-1)
    mean = (mask @ cie) / count.clamp(min=1.0).unsqueeze(-1)
    d = cie.unsqueeze(1) - mean.unsqueeze(2)                                             # (B, R, HW, 3)
    cov = torch.einsum("brn,brni,brnj->brij", mask, d, d) / count.clamp(min=1.0).view(B, R, 1, 1)
    return hist, count, mean, cov


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    o = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    R = 3
    dirs = metrics.colour_directions()
    dirs_dev = dirs.long().cuda()
    import colour_cases as C                            # the constants of the definition (tests/ is the script's directory)
    tab, M = torch.from_numpy(C.srgb_table()).float().cuda(), torch.from_numpy(C.lab_matrix()).float().cuda()
    print("colour statistics on %s, R = %d, P = %d, %d reps (median / min ms)" % (torch.cuda.get_device_name(0), R, dirs.shape[0], o.reps))
    for B, size in ((8, 512), (4, 1024)):
        g = torch.Generator().manual_seed(size)
        s = size // 16
        labels = torch.randint(0, R, (B, s, s), generator=g).repeat_interleave(16, 1).repeat_interleave(16, 2).to(torch.uint8).cuda()
        smooth = glue.tensor2im(W.synthetic_images(size, B, size=size).cuda())
        flat = torch.tensor([200, 120, 40], dtype=torch.uint8).cuda().expand(B, size, size, 3).contiguous()
        print(" B = %d at %d x %d (%.1f MB of pixels and labels)" % (B, size, size, B * size * size * 4 / 1e6))
        for name, img in (("smooth portrait", smooth), ("flat colour", flat)):
            hip = lambda: ops.colour_stats(img, labels, R, dirs)
            ref = lambda: torch_stats(img, labels, R, dirs_dev, tab, M)
            h, c = hip()[:2], ref()[:2]
            assert torch.equal(h[0].long(), c[0]) and torch.equal(h[1].long(), c[1].long())   # the same histograms and counts
            res = []
            for fn in (hip, ref):
                for _ in range(3):
                    fn()
                torch.cuda.synchronize()
                res.append(timed(fn, o.reps))
            px = B * size * size
            print("  %-16s HIP %8.3f / %8.3f ms (%.2f ns per pixel)   torch %8.3f / %8.3f ms   torch / HIP = %.1f"
                  % (name, res[0][0], res[0][1], res[0][0] * 1e6 / px, res[1][0], res[1][1], res[1][0] / res[0][0]))
        hist = ops.colour_stats(smooth, labels, R, dirs)[0]
        pairs = [(n, (n + 1) % B) for n in range(B)]
        w1 = lambda: ops.hist_w1(hist, hist, pairs)
        for _ in range(3):
            w1()
        torch.cuda.synchronize()
        print("  %-16s HIP %8.3f / %8.3f ms (%d pairs x %d histograms, pair upload included)" % (("hist_w1",) + timed(w1, o.reps) + (B, R * dirs.shape[0])))
