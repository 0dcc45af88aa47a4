"""Tuning aid (GPU), not a test: the PNG encoder's time.

    python tests/png_time.py [--no-files]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o png -- python tests/png_time.py --no-files
    python tests/png_time.py --stats DIR/.../png_kernel_stats.csv

* ops.png_encode per image at B = 8 for 512^2 and 1024^2 RGB (HIP events around 20 calls after 3 warm-up calls), and the same
  on constant images (one literal to code: what the launches cost when deflate has almost nothing to emit);
* the split over the three stages: one call is four launches on one stream, so the split is read from a kernel trace of this
  script -- ``--stats FILE`` sums the trace's kernel statistics per stage (filter / deflate / assemble = layout + gather);
* wall time of evaluation.save_images for 64 images of 512^2 with encoder="host" on 8 worker threads against "device".
"""
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ppst_amd import evaluation as EV, ops, weights as W


def device_ms(u8, reps=20):
    for _ in range(3):
        ops.png_encode(u8)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        files, sizes = ops.png_encode(u8)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, sizes


STAGES = {"png_filter_kernel": "filter", "png_deflate_kernel": "deflate", "png_layout_kernel": "assemble", "png_gather_kernel": "assemble"}


def stage_split(path):
    """Per-stage share of the encoder's kernel time from a rocprofv3 ``*_kernel_stats.csv``."""
    import csv
    tot = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            ns = float(row.get("TotalDurationNs") or row.get("TotalDuration") or 0)
            for k, stage in STAGES.items():
                if k in name:
                    tot[stage] = tot.get(stage, 0.0) + ns
    allns = sum(tot.values())
    for stage in ("filter", "deflate", "assemble"):
        print("%-9s %10.3f ms  %5.1f %%" % (stage, tot.get(stage, 0.0) / 1e6, 100.0 * tot.get(stage, 0.0) / max(allns, 1.0)))


def main():
    if "--stats" in sys.argv:
        return stage_split(sys.argv[sys.argv.index("--stats") + 1])
    dev = torch.device("cuda", 0)
    B = 8
    for size in (512, 1024):
        x = W.synthetic_images(3, B, size=size).to(dev)
        u8 = ((x.clamp(-1, 1) + 1) * 127.5).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
        ms, sizes = device_ms(u8)
        flat = torch.full_like(u8, 128)
        ms_flat, _ = device_ms(flat)
        print("png_encode B=%d %dx%dx3: %.3f ms per call = %.1f us per image (%.0f file bytes per image); constant images: %.1f us per image"
              % (B, size, size, ms, 1e3 * ms / B, sizes.float().mean().item(), 1e3 * ms_flat / B))
    if "--no-files" in sys.argv:
        return
    from concurrent.futures import ThreadPoolExecutor
    imgs = W.synthetic_images(4, 64, size=512).to(dev)
    with tempfile.TemporaryDirectory() as d:
        for enc in ("host", "device", "host", "device"):
            paths = [os.path.join(d, "%s_%02d.png" % (enc, i)) for i in range(64)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with ThreadPoolExecutor(max_workers=8) as pool:
                futs = []
                for k in range(0, 64, 8):
                    futs += EV.save_images(imgs[k:k + 8], paths[k:k + 8], pool, encoder=enc)
                for f in futs:
                    f.result()
            dt = time.perf_counter() - t0
            print("save_images 64 x 512^2, encoder=%-6s workers=8: %.1f ms wall (%.2f ms per image), %.1f MB written"
                  % (enc, 1e3 * dt, 1e3 * dt / 64, sum(os.path.getsize(p) for p in paths) / 1e6))


if __name__ == "__main__":
    main()
