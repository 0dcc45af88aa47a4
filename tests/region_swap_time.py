"""Timing aid (GPU), not a test: a swap inside a photograph (DESIGN.md "Swaps inside a photograph").

    python tests/region_swap_time.py [--out FILE]

One process; HIP events around repeated calls after warm-up, five groups, the line gives the fastest, the median and the
slowest group.  Every step runs under a watchdog of its own (faulthandler: the process exits if the step has not returned in
time, even inside a blocked device call), and a step that raises ends the run.

A 4096 x 3072 photo, a 2048-pixel square (s = 4 -> 512^2) at 0 and at 30 degrees:
* ops.extract_similarity against what a user could compose from torch ops (F.interpolate(antialias=True) of the photo by 1/s, then
  F.grid_sample(mode="bicubic") along the transform), with the bytes each crop pixel moves (3 s^2 photo bytes + 3 written);
* ops.guided_filter_paste against the same arithmetic from torch ops (F.grid_sample(mode="bilinear", padding_mode="border") of
  the 12 planes along the transform, multiply-add, smoothstep, round, torch.where over the photo), against
  ops.guided_filter_apply 512^2 -> 2048^2 (the same pixel count, axis-aligned), and the bytes a quad pixel moves (3 read, 3
  written, 48 / s^2 of coefficients);
* evaluation.simple_swap_region per swap at B = 1 beside simple_swap at 512^2.
"""
import faulthandler
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from ppst_amd import imageio, ops, weights as W  # noqa: E402
from ppst_amd.evaluation import simple_swap, simple_swap_region  # noqa: E402
from ppst_amd.ppst_model import create_model  # noqa: E402

EPS = (0.02 * 255) ** 2
H, WID, N, SIDE = 3072, 4096, 512, 2048.0
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def step(seconds, fn, *a):
    faulthandler.dump_traceback_later(seconds, exit=True)
    try:
        return fn(*a)
    finally:
        faulthandler.cancel_dump_traceback_later()


def groups_ms(fn, reps=10, warm=3, groups=5):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(groups):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / reps)
    ms.sort()
    return ms[0], ms[len(ms) // 2], ms[-1]


def uv_grid(xf, dev):
    """(U, V) / 2^24 of every photo pixel, float64 on the device"""
    a, b, cu, cv = xf
    px = (2 * torch.arange(WID, device=dev, dtype=torch.float64) + 1)[None, :]
    py = (2 * torch.arange(H, device=dev, dtype=torch.float64) + 1)[:, None]
    return (a * px + b * py + cu) / 2.0 ** 24, (-b * px + a * py + cv) / 2.0 ** 24


def torch_extract(photo, xf, s):
    a, b, cu, cv = xf
    D = float(a * a + b * b)
    x = photo.permute(0, 3, 1, 2).float()
    small = F.interpolate(x, scale_factor=1.0 / s, mode="bicubic", antialias=True, align_corners=False)
    c = (2 * torch.arange(N, device=photo.device, dtype=torch.float64) + 1) * 2.0 ** 23
    dU, dV = c[None, :] - cu, c[:, None] - cv
    X, Y = (a * dU - b * dV) / D / 2, (b * dU + a * dV) / D / 2                       # photo positions of the crop's pixel centres
    grid = torch.stack((X / WID * 2 - 1, Y / H * 2 - 1), -1).float()[None]
    out = F.grid_sample(small, grid, mode="bicubic", padding_mode="border", align_corners=False)
    return out.round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def torch_paste(co, photo, xf, feather):
    u, v = uv_grid(xf, photo.device)
    grid = torch.stack((u / N * 2 - 1, v / N * 2 - 1), -1).float()[None]
    up = F.grid_sample(co, grid, mode="bilinear", padding_mode="border", align_corners=False).view(1, 3, 4, H, WID)
    I = photo.permute(0, 3, 1, 2).float()
    q = (up[:, :, :3] * I[:, None]).sum(2) + up[:, :, 3]
    inside = (u >= 0) & (u < N) & (v >= 0) & (v < N)
    if feather:
        t = (torch.minimum(torch.minimum(u, N - u), torch.minimum(v, N - v)) / feather).clamp(0, 1).float()
        g = t * t * (3 - 2 * t)
        q = g * q + (1 - g) * I
    q = torch.where(inside[None, None], q.round().clamp(0, 255), I)
    return q.to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def kernel_step(angle, gen):
    photo = torch.randint(0, 256, (1, H, WID, 3), dtype=torch.uint8, device="cuda", generator=gen)
    xf = imageio.crop_transform((WID / 2 + 0.3, H / 2 - 0.2), SIDE, angle, N)
    s = SIDE / N
    crop = ops.extract_similarity(photo, xf, N)
    src = torch.randint(0, 256, (1, N, N, 3), dtype=torch.uint8, device="cuda", generator=gen)
    co = ops.guided_filter_coeffs(crop, src, 30, EPS)
    feather = 16
    diff = (ops.guided_filter_paste(co, photo, xf, feather).int() - torch_paste(co, photo, xf, feather).int()).abs()
    ex = groups_ms(lambda: ops.extract_similarity(photo, xf, N))
    ext = groups_ms(lambda: torch_extract(photo, xf, s), reps=3, warm=2)
    out = photo.clone()
    pa = groups_ms(lambda: ops.guided_filter_paste(co, photo, xf, feather, out=out))
    pat = groups_ms(lambda: torch_paste(co, photo, xf, feather), reps=3, warm=2)
    native = photo[:, :int(SIDE), :int(SIDE)].contiguous()
    ap = groups_ms(lambda: ops.guided_filter_apply(co, native))
    quad = SIDE * SIDE
    say("extract %dx%d, s=%g, %g deg -> %d^2: %.1f us (min %.1f, max %.1f); %.0f B per crop pixel = %.1f MB, %.0f GB/s; torch composition "
        "%.1f us (%.1f x)" % (WID, H, s, angle, N, 1e3 * ex[1], 1e3 * ex[0], 1e3 * ex[2], 3 * s * s + 3, (3 * s * s + 3) * N * N / 1e6,
                              (3 * s * s + 3) * N * N / ex[1] / 1e6, 1e3 * ext[1], ext[1] / ex[1]))
    say("paste over the same quad (%.1f M pixels), feather %d: %.1f us (min %.1f, max %.1f); %.1f B per quad pixel = %.1f MB, %.0f GB/s; torch "
        "composition %.1f us (%.1f x); guided_filter_apply 512^2 -> %d^2: %.1f us; bytes that differ from the composition by 1: %.5f, by more: %d"
        % (quad / 1e6, feather, 1e3 * pa[1], 1e3 * pa[0], 1e3 * pa[2], 6 + 48 / (s * s), (6 + 48 / (s * s)) * quad / 1e6,
           (6 + 48 / (s * s)) * quad / pa[1] / 1e6, 1e3 * pat[1], pat[1] / pa[1], int(SIDE), 1e3 * ap[1], float((diff == 1).float().mean()),
           int((diff > 1).sum())))


def swap_step(model, gen):
    with torch.no_grad():
        photo = torch.randint(0, 256, (1, H, WID, 3), dtype=torch.uint8, device="cuda", generator=gen)
        xf = imageio.crop_transform((WID / 2 + 0.3, H / 2 - 0.2), SIDE, 30.0, N)
        style = W.synthetic_images(5, 1, size=512).cuda()
        content = imageio.to_tensor_normalized(ops.extract_similarity(photo, xf, N))
        reg = groups_ms(lambda: simple_swap_region(model, photo, xf, style, (1.0,), 512, 16), reps=5, warm=2)
        low = groups_ms(lambda: simple_swap(model, content, style, (1.0,)), reps=5, warm=2)
        cl = groups_ms(lambda: photo.clone())
    say("simple_swap_region, 2048-pixel square of a %dx%d photo, B=1: %.2f ms per swap (min %.2f, max %.2f); simple_swap at 512^2 (no "
        "filter): %.2f ms; the clone of the photo inside it: %.3f ms" % (WID, H, reg[1], reg[0], reg[2], low[1], cl[1]))


def main():
    gen = torch.Generator(device="cuda").manual_seed(0)
    step(120, kernel_step, 0.0, gen)
    step(120, kernel_step, 30.0, gen)
    sd = W.make_state_dict(0, with_D=False, with_nce=False, bias_std=0.1)
    model = step(120, lambda: create_model(state_dict=sd, device=torch.device("cuda", 0)))
    model.noise = None
    step(180, swap_step, model, gen)
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
