"""Timing aid (GPU), not a test: the native-size guided filter (DESIGN.md "Native-size swap output").

    python tests/gf_native_time.py [--out FILE]

One process; HIP events around repeated calls after warm-up, five groups, the line gives the fastest, the median and the
slowest group.  Every step runs under a watchdog of its own (faulthandler: the process exits if the step has not returned in
time, even inside a blocked device call), and a step that raises ends the run.

* ops.guided_filter_apply alone, 512^2 coefficients -> 1024^2 and 2048^2, B = 4, against
    - the bytes it has to move: 3 guide + 3 output bytes per native pixel and 48 B per coefficient sample (12 fp32 planes),
      beside a device copy of the same byte count in this process (the measure of tests/copy_bw.py);
    - the same arithmetic composed from torch ops (F.interpolate of the 12 planes, multiply-add, round): what a user could
      run without the kernel.  The one ordering the feature promises -- the launch is not slower -- fails the run if broken.
* ops.guided_filter_coeffs at 512^2, r = 30 (the five-launch fp32-plane path) beside the fused ops.guided_filter.
* evaluation.simple_swap_native 512^2 -> 1024^2 per swap at B = 1, beside simple_swap at 512^2 and at 1024^2.
"""
import faulthandler
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from ppst_amd import imageio, ops, weights as W  # noqa: E402
from ppst_amd.evaluation import simple_swap, simple_swap_native  # noqa: E402
from ppst_amd.ppst_model import create_model  # noqa: E402

EPS = (0.02 * 255) ** 2
LINES, BROKEN = [], []


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


def torch_apply(co, guide):
    B, H, W, _ = guide.shape
    up = F.interpolate(co, size=(H, W), mode="bilinear", align_corners=False).view(B, 3, 4, H, W)
    I = guide.permute(0, 3, 1, 2).float()
    q = (up[:, :, :3] * I[:, None]).sum(2) + up[:, :, 3]
    return q.round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def apply_step(B, side, Side, gen):
    g = torch.randint(0, 256, (B, side, side, 3), dtype=torch.uint8, device="cuda", generator=gen)
    s = torch.randint(0, 256, (B, side, side, 3), dtype=torch.uint8, device="cuda", generator=gen)
    native = torch.randint(0, 256, (B, Side, Side, 3), dtype=torch.uint8, device="cuda", generator=gen)
    co = ops.guided_filter_coeffs(g, s, 30, EPS)
    diff = (ops.guided_filter_apply(co, native).int() - torch_apply(co, native).int()).abs()
    hip = groups_ms(lambda: ops.guided_filter_apply(co, native))
    ref = groups_ms(lambda: torch_apply(co, native), reps=3, warm=2)
    nbytes = B * (6 * Side * Side + 48 * side * side)
    a = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    cp = groups_ms(lambda: b.copy_(a))
    say("apply %d^2 -> %d^2, B=%d: %.1f us (min %.1f, max %.1f); %.1f B per native pixel = %.1f MB, %.0f GB/s; a copy of the same bytes %.1f us "
        "(%.0f GB/s); torch composition %.1f us (%.1f x); bytes that differ from it by 1: %.5f, by more: %d"
        % (side, Side, B, 1e3 * hip[1], 1e3 * hip[0], 1e3 * hip[2], nbytes / (B * Side * Side), nbytes / 1e6, nbytes / hip[1] / 1e6, 1e3 * cp[1],
           nbytes / cp[1] / 1e6, 1e3 * ref[1], ref[1] / hip[1], float((diff == 1).float().mean()), int((diff > 1).sum())))
    if hip[1] > ref[1]:
        BROKEN.append("the apply launch is slower than the torch composition at %d^2 -> %d^2, B=%d" % (side, Side, B))


def coeffs_step(B, gen):
    g = torch.randint(0, 256, (B, 512, 512, 3), dtype=torch.uint8, device="cuda", generator=gen)
    s = torch.randint(0, 256, (B, 512, 512, 3), dtype=torch.uint8, device="cuda", generator=gen)
    co = groups_ms(lambda: ops.guided_filter_coeffs(g, s, 30, EPS), reps=5)
    fu = groups_ms(lambda: ops.guided_filter(g, s, 30, EPS))
    say("coefficients 512^2 r=30, B=%d (five launches through fp32 planes): %.3f ms (min %.3f, max %.3f); the fused filter: %.3f ms (%.1f x)"
        % (B, co[1], co[0], co[2], fu[1], co[1] / fu[1]))


def swap_step(model, imgs):
    with torch.no_grad():
        native = ((imgs[0:1].clamp(-1, 1) + 1) * 127.5).to(torch.uint8).permute(0, 2, 3, 1).contiguous()      # (1,1024,1024,3)
        big_c, big_s = imgs[0:1].contiguous(), imgs[1:2].contiguous()
        content, style = imageio.preprocess(native, 512), imageio.resize_tensor(big_s, 512, 512, clamp=(-1, 1))
        nat = groups_ms(lambda: simple_swap_native(model, native, style, (1.0,), 512), reps=5, warm=2)
        low = groups_ms(lambda: simple_swap(model, content, style, (1.0,)), reps=5, warm=2)
        big = groups_ms(lambda: simple_swap(model, big_c, big_s, (1.0,)), reps=3, warm=2)
    say("simple_swap_native 512^2 -> 1024^2, B=1: %.2f ms per swap (min %.2f, max %.2f); simple_swap at 512^2 (no filter): %.2f ms; "
        "simple_swap at 1024^2 (the full-size model path, no filter): %.2f ms" % (nat[1], nat[0], nat[2], low[1], big[1]))


def main():
    gen = torch.Generator(device="cuda").manual_seed(0)
    step(120, apply_step, 4, 512, 1024, gen)
    step(120, apply_step, 4, 512, 2048, gen)
    step(120, apply_step, 1, 512, 4096, gen)
    step(60, coeffs_step, 1, gen)
    step(60, coeffs_step, 4, gen)
    sd = W.make_state_dict(0, with_D=False, with_nce=False, bias_std=0.1)
    model = step(120, lambda: create_model(state_dict=sd, device=torch.device("cuda", 0)))
    model.noise = None
    imgs = W.synthetic_images(4, 2, size=1024).cuda()
    step(180, swap_step, model, imgs)
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("\n".join(LINES) + "\n")
    if BROKEN:
        raise SystemExit("; ".join(BROKEN))


if __name__ == "__main__":
    main()
