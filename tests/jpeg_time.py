"""Tuning aid (GPU), not a test: the JPEG encoder's time.

    python tests/jpeg_time.py [--no-files]

* ops.jpeg_encode per image at B = 8 for 512^2 and 1024^2 RGB, q = 90, both subsamplings (HIP events around 20 calls after
  3 warm-up calls), and ops.png_encode in the same process as the yardstick;
* wall time of evaluation.save_images for 64 images of 512^2 on 8 worker threads with format="jpeg", encoder="device", next to
  the PNG device figure and the two host encoders, each measured twice in this process.
"""
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ppst_amd import evaluation as EV, ops, weights as W


def device_ms(call, reps=20):
    for _ in range(3):
        call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        files, sizes = call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, sizes


def main():
    dev = torch.device("cuda", 0)
    B = 8
    for size in (512, 1024):
        x = W.synthetic_images(3, B, size=size).to(dev)
        u8 = ((x.clamp(-1, 1) + 1) * 127.5).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
        for ss in ("4:2:0", "4:4:4"):
            ms, sizes = device_ms(lambda: ops.jpeg_encode(u8, 90, ss))
            print("jpeg_encode B=%d %dx%dx3 q 90 %s: %.3f ms per call = %.1f us per image (%.0f file bytes per image)"
                  % (B, size, size, ss, ms, 1e3 * ms / B, sizes.float().mean().item()))
        ms, sizes = device_ms(lambda: ops.png_encode(u8))
        print("png_encode  B=%d %dx%dx3: %.3f ms per call = %.1f us per image (%.0f file bytes per image)"
              % (B, size, size, ms, 1e3 * ms / B, sizes.float().mean().item()))
    if "--no-files" in sys.argv:
        return
    from concurrent.futures import ThreadPoolExecutor
    imgs = W.synthetic_images(4, 64, size=512).to(dev)
    runs = [("png", "host"), ("png", "device"), ("jpeg", "host"), ("jpeg", "device")]
    with tempfile.TemporaryDirectory() as d:
        for fmt, enc in runs + runs:
            paths = [os.path.join(d, "%s_%s_%02d%s" % (fmt, enc, i, EV.FORMATS[fmt])) for i in range(64)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with ThreadPoolExecutor(max_workers=8) as pool:
                futs = []
                for k in range(0, 64, 8):
                    futs += EV.save_images(imgs[k:k + 8], paths[k:k + 8], pool, encoder=enc, format=fmt)
                for f in futs:
                    f.result()
            dt = time.perf_counter() - t0
            print("save_images 64 x 512^2, format=%-4s encoder=%-6s workers=8: %.1f ms wall (%.2f ms per image), %.1f MB written"
                  % (fmt, enc, 1e3 * dt, 1e3 * dt / 64, sum(os.path.getsize(p) for p in paths) / 1e6))


if __name__ == "__main__":
    main()
