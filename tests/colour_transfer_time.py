"""Tuning aid (not a test): time the colour-transfer entry points (csrc/colour_transfer.hip) by HIP events, next to the same
arithmetic composed from torch ops on the device in the same process.

    python tests/colour_transfer_time.py [--reps 30]

Shapes: B = 8 at 512^2 and B = 4 at 1024^2, R = 3 regions (16 x 16 label blocks).  Timed: ``ops.hist_match_lut`` (B pairs), and
``ops.colour_transfer_apply`` in both modes, with and without weights.  The yardsticks: torch.cumsum + torch.searchsorted in int64
for the tables; a gather per channel for the LUT mode; the Lab chain (table gather, two 3 x 3 products, cube roots, powers,
selects) in fp32 for the affine mode; weighted forms blend the per-region results (the coefficients) with normalised weights.
Reported: median / min ms over ``reps`` after warm-up, their ratio, ns per pixel and the effective GB/s of the HIP pass over the
bytes it has to move (7 per pixel: 3 + 1 in, 3 out; + 4 R with weights).
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


def torch_luts(hc, hs):
    """(B, R, 3, 256) tables for the pairs n -> n from (B, R, P, 256) histograms"""
    cc, cs = hc[:, :, :3].long().cumsum(-1), hs[:, :, :3].long().cumsum(-1)
    nC, nS = cc[..., -1:], cs[..., -1:]
    rhs = (cc + cc - hc[:, :, :3].long()) * nS
    lut = torch.searchsorted((2 * cs * nC).contiguous(), rhs.contiguous()).clamp(max=255)
    ident = torch.arange(256, device=hc.device).expand_as(lut)
    return torch.where((nC == 0) | (nS == 0), ident, lut).to(torch.uint8)


def torch_lut_apply(u8, labels, luts, weights=None):
    B, H, Wd, _ = u8.shape
    R = luts.shape[1]
    v = u8.long()
    per = torch.stack([torch.gather(luts[:, :, c].reshape(B, R * 256), 1,
                                    (torch.arange(R, device=u8.device).view(1, R, 1) * 256 + v[..., c].reshape(B, 1, -1)).reshape(B, -1))
                       .view(B, R, H, Wd) for c in range(3)], -1)                       # (B, R, H, W, 3)
    hard = torch.gather(per, 1, labels.long().clamp(max=R - 1).view(B, 1, H, Wd, 1).expand(B, 1, H, Wd, 3))[:, 0]
    if weights is None:
        return hard
    den = weights.sum(1)
    mix = torch.round((weights.unsqueeze(-1) * per.float()).sum(1) / den.clamp(min=1e-30).unsqueeze(-1)).to(torch.uint8)
    return torch.where((den > 0).unsqueeze(-1), mix, hard)


def torch_affine_apply(u8, labels, rows, tab, M, Mi, weights=None):
    B, H, Wd, _ = u8.shape
    R = rows.shape[1]
    k = torch.gather(rows, 1, labels.long().clamp(max=R - 1).view(B, -1, 1).expand(B, H * Wd, 12)).view(B, H, Wd, 12)
    if weights is not None:
        den = weights.sum(1)
        mix = torch.einsum("brhw,brk->bhwk", weights, rows) / den.clamp(min=1e-30).unsqueeze(-1)
        k = torch.where((den > 0).unsqueeze(-1), mix, k)
    f = tab[u8.long()] @ M.T
    f = torch.where(f > (6.0 / 29.0) ** 3, f.clamp(min=1e-30) ** (1.0 / 3.0), f * (841.0 / 108.0) + 4.0 / 29.0)
    lab = torch.stack((116.0 * f[..., 1] - 16.0, 500.0 * (f[..., 0] - f[..., 1]), 200.0 * (f[..., 1] - f[..., 2])), -1)
    out = (k[..., :9].view(B, H, Wd, 3, 3) @ lab.unsqueeze(-1)).squeeze(-1) + k[..., 9:]
    fy = (out[..., 0] + 16.0) / 116.0
    g = torch.stack((fy + out[..., 1] / 500.0, fy, fy - out[..., 2] / 200.0), -1)
    t = torch.where(g > 6.0 / 29.0, g * g * g, (g - 4.0 / 29.0) * (108.0 / 841.0))
    c = (t @ Mi.T).clamp(0.0, 1.0)
    s = torch.where(c <= 0.0031308, 12.92 * c, 1.055 * c ** (1.0 / 2.4) - 0.055)
    return torch.round(255.0 * s).to(torch.uint8)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    o = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    R = 3
    import colour_cases as C                            # the constants of the definition (tests/ is the script's directory)
    import transfer_cases as T
    tab, M = torch.from_numpy(C.srgb_table()).float().cuda(), torch.from_numpy(C.lab_matrix()).float().cuda()
    Mi = torch.from_numpy(T.inverse_matrix()).float().cuda()
    print("colour transfer on %s, R = %d, %d reps (median / min ms)" % (torch.cuda.get_device_name(0), R, o.reps))

    def bench(name, hip, ref, px, nbytes, same):
        a, b = hip(), ref()
        diff = (a.int() - b.int()).abs()
        note = "" if int(diff.max()) == 0 else "   [yardstick differs: max %d, share %.2g%s]" % (
            int(diff.max()), float((diff > 0).float().mean()), "" if not same else ", expected equal")
        res = []
        for fn in (hip, ref):
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            res.append(timed(fn, o.reps))
        print("  %-22s HIP %8.3f / %8.3f ms (%.3f ns per pixel, %6.0f GB/s)   torch %8.3f / %8.3f ms   torch / HIP = %.1f"
              % (name, res[0][0], res[0][1], res[0][0] * 1e6 / px, nbytes / res[0][1] / 1e6, res[1][0], res[1][1], res[1][0] / res[0][0]) + note)

    for B, size in ((8, 512), (4, 1024)):
        g = torch.Generator().manual_seed(size)
        s = size // 16
        labels = torch.randint(0, R, (B, s, s), generator=g).repeat_interleave(16, 1).repeat_interleave(16, 2).to(torch.uint8).cuda()
        img = glue.tensor2im(W.synthetic_images(size, B, size=size).cuda())
        sty = glue.tensor2im(W.synthetic_images(size + 1, B, size=size).cuda())
        weights = metrics.region_weights(labels, R, 8)
        st_c, st_s = metrics.colour_stats(img, labels, R), metrics.colour_stats(sty, labels.flip(0).contiguous(), R)
        pairs = torch.tensor([(n, n) for n in range(B)])
        luts = ops.hist_match_lut(st_c.hist, st_s.hist, pairs)
        rows = metrics.colour_transfer_maps(st_c, st_s, "mkl")
        px = B * size * size
        print(" B = %d at %d x %d (%.1f MB at 7 bytes per pixel)" % (B, size, size, px * 7 / 1e6))
        bench("hist_match_lut", lambda: ops.hist_match_lut(st_c.hist, st_s.hist, pairs), lambda: torch_luts(st_c.hist, st_s.hist), px,
              B * R * 3 * 256 * 9, True)
        bench("apply LUT", lambda: ops.colour_transfer_apply(img, labels, luts=luts), lambda: torch_lut_apply(img, labels, luts), px, px * 7, True)
        bench("apply LUT weighted", lambda: ops.colour_transfer_apply(img, labels, luts=luts, weights=weights),
              lambda: torch_lut_apply(img, labels, luts, weights), px, px * (7 + 4 * R), False)
        bench("apply affine", lambda: ops.colour_transfer_apply(img, labels, affine=rows),
              lambda: torch_affine_apply(img, labels, rows, tab, M, Mi), px, px * 7, False)
        bench("apply affine weighted", lambda: ops.colour_transfer_apply(img, labels, affine=rows, weights=weights),
              lambda: torch_affine_apply(img, labels, rows, tab, M, Mi, weights), px, px * (7 + 4 * R), False)
