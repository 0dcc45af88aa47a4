"""Timing aid (GPU), not a test: region swaps through a matte (DESIGN.md "Region swaps through a matte").

    python tests/matte_time.py [--out FILE]

One process; HIP events around repeated calls after warm-up, five groups of ten calls, the line gives the fastest, the median
and the slowest group (tests/region_swap_time.py's scheme).  Every step runs under a watchdog of its own (faulthandler: the
process exits if the step has not returned in time), and a step that raises ends the run.

* ops.label_matte (both launches and its two allocations) at 512^2, B = 1 and B = 8, (feather, grow) = (16, 8), (64, 32), (255, 0);
  scipy's distance_transform_edt (two calls: inside and outside) on one CPU thread beside it where scipy is importable;
* ops.guided_filter_paste with and without a matte: a 4096 x 3072 photo, a 2048-pixel square at 0 and 30 degrees, feather 16;
* evaluation.simple_swap_region_matte with and without labels, B = 1.
"""
import faulthandler
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import matte_cases as M  # noqa: E402
from ppst_amd import imageio, ops, weights as W  # noqa: E402
from ppst_amd.evaluation import simple_swap_region, simple_swap_region_matte  # noqa: E402
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


def matte_step():
    lab = M._blob(N, N, 5)
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    for B in (1, 8):
        labels = torch.from_numpy(np.stack([np.roll(lab, 11 * i, axis=1) for i in range(B)])).cuda()
        for f, g in ((16, 8), (64, 32), (255, 0)):
            t = groups_ms(lambda: ops.label_matte(labels, (1, 2), f, g))
            line = "label_matte %d^2 B=%d feather %d grow %d (R = %d): %.1f us (min %.1f, max %.1f), %.1f us per plane" % (
                N, B, f, g, M.radius(f, g), 1e3 * t[1], 1e3 * t[0], 1e3 * t[2], 1e3 * t[1] / B)
            if ndimage is not None and B == 1:
                torch.set_num_threads(1)
                ins = M.inside_of(lab, M.FACE)
                best = 1e9
                for _ in range(3):
                    t0 = time.perf_counter()
                    ndimage.distance_transform_edt(ins)
                    ndimage.distance_transform_edt(~ins)
                    best = min(best, time.perf_counter() - t0)
                line += "; scipy distance_transform_edt, both signs, one CPU thread (unclipped): %.1f ms" % (1e3 * best)
            say(line)
    if ndimage is None:
        say("scipy is not importable here: no CPU distance transform beside it")


def paste_step(angle, gen):
    photo = torch.randint(0, 256, (1, H, WID, 3), dtype=torch.uint8, device="cuda", generator=gen)
    xf = imageio.crop_transform((WID / 2 + 0.3, H / 2 - 0.2), SIDE, angle, N)
    crop = ops.extract_similarity(photo, xf, N)
    src = torch.randint(0, 256, (1, N, N, 3), dtype=torch.uint8, device="cuda", generator=gen)
    co = ops.guided_filter_coeffs(crop, src, 30, EPS)
    matte = ops.label_matte(torch.from_numpy(M._blob(N, N, 5)[None]).cuda(), (1, 2), 16, 8)
    ones = torch.ones_like(matte)
    feather, out = 16, photo.clone()
    plain = groups_ms(lambda: ops.guided_filter_paste(co, photo, xf, feather, out=out))
    full = groups_ms(lambda: ops.guided_filter_paste(co, photo, xf, feather, out=out, matte=ones))
    blob = groups_ms(lambda: ops.guided_filter_paste(co, photo, xf, feather, out=out, matte=matte))
    plain2 = groups_ms(lambda: ops.guided_filter_paste(co, photo, xf, feather, out=out))
    say("paste, 2048-pixel square at %g deg of a %dx%d photo, feather %d: no matte %.1f us (min %.1f, max %.1f; again after the others: %.1f); "
        "all-ones matte %.1f us (min %.1f, max %.1f) = %.3f x; face matte (%.0f %% of the crop is 0: those pixels are not written) %.1f us "
        "(min %.1f, max %.1f) = %.3f x" % (angle, WID, H, feather, 1e3 * plain[1], 1e3 * plain[0], 1e3 * plain[2], 1e3 * plain2[1],
                                          1e3 * full[1], 1e3 * full[0], 1e3 * full[2], full[1] / plain[1],
                                          100 * float((matte == 0).float().mean()), 1e3 * blob[1], 1e3 * blob[0], 1e3 * blob[2], blob[1] / plain[1]))


def swap_step(model, gen):
    with torch.no_grad():
        photo = torch.randint(0, 256, (1, H, WID, 3), dtype=torch.uint8, device="cuda", generator=gen)
        xf = imageio.crop_transform((WID / 2 + 0.3, H / 2 - 0.2), SIDE, 30.0, N)
        style = W.synthetic_images(5, 1, size=512).cuda()
        labels = torch.from_numpy(M._blob(N, N, 5)[None]).cuda()
        reg = groups_ms(lambda: simple_swap_region(model, photo, xf, style, (1.0,), 512, 16), reps=5, warm=2)
        lab = groups_ms(lambda: simple_swap_region_matte(model, photo, xf, style, (1.0,), 512, 16, labels=labels), reps=5, warm=2)
        reg2 = groups_ms(lambda: simple_swap_region(model, photo, xf, style, (1.0,), 512, 16), reps=5, warm=2)
    say("simple_swap_region, 2048-pixel square of a %dx%d photo, B=1: %.3f ms per swap (min %.3f, max %.3f; again afterwards %.3f); with "
        "labels (matte 16 / 8): %.3f ms (min %.3f, max %.3f): %+.3f ms per swap"
        % (WID, H, reg[1], reg[0], reg[2], reg2[1], lab[1], lab[0], lab[2], lab[1] - min(reg[1], reg2[1])))


def main():
    gen = torch.Generator(device="cuda").manual_seed(0)
    step(120, matte_step)
    step(120, paste_step, 0.0, gen)
    step(120, paste_step, 30.0, gen)
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
