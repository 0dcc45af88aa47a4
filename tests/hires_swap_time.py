"""Timing aid (GPU), not a test: the two-resolution swap at 1024^2 (DESIGN.md "Swaps above 512^2").

    python tests/hires_swap_time.py [--out FILE]

* ms per evaluation.simple_swap of a 1024^2 pair at batch 1 and 4, in the fp32-class mode (bf16x3) and in fp16 (HIP events
  around ``reps`` calls after 2 warm-up calls);
* the share of the two 512^2 correspondence passes (resample + PPSTModel.correspondence_features of contents and styles as
  one batch, the way the recipe issues them), timed alone the same way;
* the resample launch alone, 1024^2 -> 512^2 on B x 3 planes, against the bytes it has to move: 12 values read + 3 written per
  output pixel at 2 : 1 (4 inputs per output and channel), fp32: 48 B + 12 B.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ppst_amd import imageio, ops, weights as W
from ppst_amd.evaluation import simple_swap
from ppst_amd.ppst_model import create_model


def event_ms(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    sd = W.make_state_dict(0, with_D=False, with_nce=False, bias_std=0.1)
    model = create_model(state_dict=sd, device=dev)
    model.noise = None            # (zero noise weights: one pinned noise dict cannot serve both resolutions)
    imgs = W.synthetic_images(4, 8, size=1024).to(dev)
    with torch.no_grad():
        for B in (1, 4, 8):
            x = imgs[:B].contiguous()
            ms = event_ms(lambda: imageio.resize_tensor(x, 512, 512, clamp=(-1, 1)), reps=50, warm=5)
            nbytes = B * 3 * 512 * 512 * (16 + 4)
            say("resample 1024^2 -> 512^2, B=%d (%d planes): %.1f us, %.2f MB moved = %.0f GB/s"
                % (B, 3 * B, 1e3 * ms, nbytes / 1e6, nbytes / ms / 1e6))
        for mode, p in (("bf16x3", 0), ("fp16", 3)):
            ops.set_precision(p)
            for B in (1, 4):
                content, style = imgs[:B].contiguous(), imgs[4:4 + B].contiguous()

                def corr_passes():
                    small = torch.cat((model(content, command="correspondence_image"), model(style, command="correspondence_image")), 0)
                    return model(small, command="correspondence_features")
                reps = 5 if B == 1 else 3
                total = event_ms(lambda: simple_swap(model, content, style, (1.0,)), reps)
                part = event_ms(corr_passes, reps)
                say("%-6s simple_swap 1024^2 B=%d: %.1f ms per call = %.1f ms per swap; the two 512^2 correspondence passes: %.1f ms (%.0f %%)"
                    % (mode, B, total, total / B, part, 100.0 * part / total))
        ops.set_precision(0)
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
