"""Tuning aid (GPU), not a test: the JPEG decoder's time.

    python tests/jpeg_decode_time.py

B = 8 photo-like images of 512^2 and 1024^2 at q 90, 4:2:0, written by Pillow (no restart markers: one Huffman stream per file) and
by our encoder (DRI 16 MCUs).  HIP events around 20 calls after 3 warm-up calls: the kernels alone (ppst_jpeg_decode on files that
are already on the device) and the whole ops.jpeg_decode (parse, pack, the copy, kernels).  Rounds to convergence per file.
Yardstick, same process: Pillow's decode of the same files on 8 threads (what evaluation.load_images does with decode="host")
and on one thread."""
import io
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from PIL import Image
from ppst_amd import imageio, ops, weights as W


def device_ms(call, reps=20):
    for _ in range(3):
        call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def host_decode(blob):
    return np.array(Image.open(io.BytesIO(blob)).convert("RGB"))


def wall_ms(fn, reps=20):
    for _ in range(3):
        fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return 1e3 * (time.perf_counter() - t0) / reps


def main():
    dev = torch.device("cuda", 0)
    B = 8
    for size in (512, 1024):
        x = W.synthetic_images(3, B, size=size)
        u8 = ((x.clamp(-1, 1) + 1) * 127.5).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
        files = {"pillow (no DRI)": [], "device encoder (DRI 16)": imageio.encode_jpeg(u8.to(dev), 90, "4:2:0")}
        for a in u8.numpy():
            buf = io.BytesIO()
            Image.fromarray(a).save(buf, format="JPEG", quality=90, subsampling=2)
            files["pillow (no DRI)"].append(buf.getvalue())
        for who, blobs in files.items():
            for sw in (0, 8, 128):
                call = ops._JpegDecodeCall(blobs, None, sw, dev, expand_grey=False)
                ms_k = device_ms(call.launch)
                torch.cuda.synchronize()
                assert call.status.cpu().tolist() == [0] * B
                for v, blob in zip(call.views(), blobs):
                    assert np.array_equal(v.cpu().numpy(), host_decode(blob))
                print("%d^2 q 90 4:2:0 %-24s B=%d, %4d-word subsequences: kernels %.3f ms per call = %.1f us per image; rounds per file %s"
                      % (size, who, B, sw or 32, ms_k, 1e3 * ms_k / B, call.rounds().cpu().tolist()))
            ms_all = device_ms(lambda: ops.jpeg_decode(blobs))
            print("%d^2 q 90 4:2:0 %-24s B=%d: ops.jpeg_decode (parse, pack, copies, kernels) %.3f ms per call = %.1f us per image (%.0f file bytes per image)"
                  % (size, who, B, ms_all, 1e3 * ms_all / B, sum(map(len, blobs)) / B))
            with ThreadPoolExecutor(max_workers=8) as pool:
                ms8 = wall_ms(lambda: list(pool.map(host_decode, blobs)))
            ms1 = wall_ms(lambda: [host_decode(b) for b in blobs], reps=5)
            print("%d^2 q 90 4:2:0 %-24s B=%d: Pillow on 8 threads %.3f ms per batch = %.1f us per image; on one thread %.1f us per image"
                  % (size, who, B, ms8, 1e3 * ms8 / B, 1e3 * ms1 / B))


if __name__ == "__main__":
    main()
