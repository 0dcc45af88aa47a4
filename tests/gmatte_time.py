"""Timing aid (GPU), not a test: region swaps through a guided matte (DESIGN.md "Region swaps through a guided matte").

    python tests/gmatte_time.py [--out FILE]

One process; tests/matte_time.py's scheme and helpers: HIP events around repeated calls after warm-up, five groups of ten calls,
the line gives the fastest, the median and the slowest group; every step under a watchdog of its own.

* ops.guided_matte_coeffs at 512^2, r = 8, B = 1 and B = 8, beside the composition the library offered before it:
  ops.guided_filter_coeffs on the source bytes replicated to three channels (the replication is not timed);
* ops.guided_filter_paste without a matte, with a matte plane, and ops.guided_filter_paste_gmatte with and without the weight
  output: matte_time.py's 4096 x 3072 photo, a 2048-pixel square at 0 and 30 degrees, feather 16;
* evaluation.simple_swap_region, simple_swap_region_matte and simple_swap_region_gmatte with labels, B = 1.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matte_time as T  # noqa: E402
import numpy as np  # noqa: E402
import torch  # noqa: E402
import matte_cases as M  # noqa: E402
from ppst_amd import imageio, ops, weights as W  # noqa: E402
from ppst_amd.evaluation import simple_swap_region, simple_swap_region_gmatte, simple_swap_region_matte  # noqa: E402
from ppst_amd.ppst_model import create_model  # noqa: E402

R, EPS = 8, (0.01 * 255) ** 2
H, WID, N, SIDE = T.H, T.WID, T.N, T.SIDE
us = lambda t: "%.1f us (min %.1f, max %.1f)" % (1e3 * t[1], 1e3 * t[0], 1e3 * t[2])


def coeffs_step(gen):
    lab = M._blob(N, N, 5)
    for B in (1, 8):
        guide = torch.randint(0, 256, (B, N, N, 3), dtype=torch.uint8, device="cuda", generator=gen)
        labels = torch.from_numpy(np.stack([np.roll(lab, 11 * i, axis=1) for i in range(B)])).cuda()
        matte = ops.label_matte(labels, (1, 2), 16, 8)
        src = (255 * matte.clamp(0, 1)).round().to(torch.uint8)[..., None].expand(B, N, N, 3).contiguous()
        assert torch.equal(ops.guided_matte_coeffs(guide, matte, R, EPS), ops.guided_filter_coeffs(guide, src, R, EPS)[:, :4])
        one = T.groups_ms(lambda: ops.guided_matte_coeffs(guide, matte, R, EPS))
        three = T.groups_ms(lambda: ops.guided_filter_coeffs(guide, src, R, EPS))
        one2 = T.groups_ms(lambda: ops.guided_matte_coeffs(guide, matte, R, EPS))
        T.say("guided_matte_coeffs %d^2 r=%d B=%d: %s (again after the other: %.1f); guided_filter_coeffs on the replicated source: %s; "
              "ratio %.3f (13 / 21 and 4 / 12 of the planes)" % (N, R, B, us(one), 1e3 * one2[1], us(three), one[1] / three[1]))


def paste_step(angle, gen):
    photo = torch.randint(0, 256, (1, H, WID, 3), dtype=torch.uint8, device="cuda", generator=gen)
    xf = imageio.crop_transform((WID / 2 + 0.3, H / 2 - 0.2), SIDE, angle, N)
    crop = ops.extract_similarity(photo, xf, N)
    src = torch.randint(0, 256, (1, N, N, 3), dtype=torch.uint8, device="cuda", generator=gen)
    co = ops.guided_filter_coeffs(crop, src, 30, T.EPS)
    matte = ops.label_matte(torch.from_numpy(M._blob(N, N, 5)[None]).cuda(), (1, 2), 16, 8)
    mco = ops.guided_matte_coeffs(crop, matte, R, EPS)
    feather, out = 16, photo.clone()
    plain = T.groups_ms(lambda: ops.guided_filter_paste(co, photo, xf, feather, out=out))
    plane = T.groups_ms(lambda: ops.guided_filter_paste(co, photo, xf, feather, out=out, matte=matte))
    gm = T.groups_ms(lambda: ops.guided_filter_paste_gmatte(co, mco, photo, xf, feather, out=out))
    gmw = T.groups_ms(lambda: ops.guided_filter_paste_gmatte(co, mco, photo, xf, feather, out=out, want_weight=True))
    plain2 = T.groups_ms(lambda: ops.guided_filter_paste(co, photo, xf, feather, out=out))
    w = ops.guided_filter_paste_gmatte(co, mco, photo, xf, feather, out=out, want_weight=True)[1]
    T.say("paste, 2048-pixel square at %g deg of a %dx%d photo, feather %d: no matte %s (again after the others: %.1f); matte plane %s "
          "= %.3f x; guided matte (weight 0 on %.0f %% of the photo) %s = %.3f x the plane form; with the weight output (its zero-filled "
          "%d MB plane allocated per call) %s" % (angle, WID, H, feather, us(plain), 1e3 * plain2[1], us(plane), plane[1] / plain[1],
                                                   100 * float((w == 0).float().mean()), us(gm), gm[1] / plane[1], H * WID >> 20, us(gmw)))


def swap_step(model, gen):
    with torch.no_grad():
        photo = torch.randint(0, 256, (1, H, WID, 3), dtype=torch.uint8, device="cuda", generator=gen)
        xf = imageio.crop_transform((WID / 2 + 0.3, H / 2 - 0.2), SIDE, 30.0, N)
        style = W.synthetic_images(5, 1, size=512).cuda()
        labels = torch.from_numpy(M._blob(N, N, 5)[None]).cuda()
        ms = lambda t: "%.3f ms (min %.3f, max %.3f)" % (t[1], t[0], t[2])
        reg = T.groups_ms(lambda: simple_swap_region(model, photo, xf, style, (1.0,), 512, 16), reps=5, warm=2)
        lab = T.groups_ms(lambda: simple_swap_region_matte(model, photo, xf, style, (1.0,), 512, 16, labels=labels), reps=5, warm=2)
        gm = T.groups_ms(lambda: simple_swap_region_gmatte(model, photo, xf, style, (1.0,), 512, 16, labels=labels), reps=5, warm=2)
        lab2 = T.groups_ms(lambda: simple_swap_region_matte(model, photo, xf, style, (1.0,), 512, 16, labels=labels), reps=5, warm=2)
    T.say("2048-pixel square of a %dx%d photo, B=1, per swap: simple_swap_region %s; simple_swap_region_matte with labels %s (again "
          "afterwards %.3f); simple_swap_region_gmatte with labels (r = 8) %s: %+.3f ms per swap over the plane matte"
          % (WID, H, ms(reg), ms(lab), lab2[1], ms(gm), gm[1] - min(lab[1], lab2[1])))


def main():
    gen = torch.Generator(device="cuda").manual_seed(0)
    T.step(120, coeffs_step, gen)
    T.step(120, paste_step, 0.0, gen)
    T.step(120, paste_step, 30.0, gen)
    sd = W.make_state_dict(0, with_D=False, with_nce=False, bias_std=0.1)
    model = T.step(120, lambda: create_model(state_dict=sd, device=torch.device("cuda", 0)))
    model.noise = None
    T.step(180, swap_step, model, gen)
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("\n".join(T.LINES) + "\n")


if __name__ == "__main__":
    main()
