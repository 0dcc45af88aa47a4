"""Tuning aid (GPU), not a test: the PNG decoder's time.

    python tests/png_decode_time.py [output file]

B = 8 photo-like images (weights.synthetic_images) of 512^2 and 1024^2 RGB as written by Pillow and by the device encoder, and a
512^2 label map of 16-pixel blocks.  HIP events around 20 calls after 3 warm-up calls: the kernels alone (ppst_png_decode on files
that are already on the device) at the default subsequence length and at four others, and the whole ops.png_decode (parse, pack,
the copy, kernels).  Rounds of the subsequence iteration per file (the largest over its windows).  Yardstick, same process:
Pillow's decode of the same files on 8 threads (what evaluation.load_images does with decode="host") and on one thread."""
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

WORDS = (0, 2, 8, 16, 32)      # 0: the default (DEFAULT_WORDS)
DEFAULT_WORDS = 4


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
    return np.array(Image.open(io.BytesIO(blob)))


def wall_ms(fn, reps=20):
    for _ in range(3):
        fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return 1e3 * (time.perf_counter() - t0) / reps


def pillow_file(a):
    buf = io.BytesIO()
    Image.fromarray(a[:, :, 0] if a.shape[2] == 1 else a).save(buf, format="PNG")
    return buf.getvalue()


def main():
    dev = torch.device("cuda", 0)
    B = 8
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    sets = []
    for size in (512, 1024):
        x = W.synthetic_images(3, B, size=size)
        u8 = ((x.clamp(-1, 1) + 1) * 127.5).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
        sets.append(("%d^2 RGB pillow" % size, [pillow_file(a) for a in u8.numpy()]))
        sets.append(("%d^2 RGB device encoder" % size, imageio.encode_png(u8.to(dev))))
    rng = np.random.default_rng(3)
    labels = [np.kron(rng.integers(0, 3, (32, 32), dtype=np.uint8), np.ones((16, 16), np.uint8))[:, :, None] for _ in range(B)]
    sets.append(("512^2 labels pillow", [pillow_file(a) for a in labels]))
    for who, blobs in sets:
        for sw in WORDS:
            call = ops._PngDecodeCall(blobs, None, sw, dev, expand_grey=False, drop_alpha=False)
            ms_k = device_ms(call.launch)
            torch.cuda.synchronize()
            assert call.status.cpu().tolist() == [0] * B
            for v, blob in zip(call.views(), blobs):
                ref = host_decode(blob)
                assert np.array_equal(v.cpu().numpy(), ref.reshape(ref.shape[0], ref.shape[1], -1))
            say("%-26s B=%d, %3d-word subsequences: kernels %8.3f ms per call = %8.1f us per image; rounds per file %s"
                % (who, B, sw or DEFAULT_WORDS, ms_k, 1e3 * ms_k / B, call.rounds().cpu().tolist()))
        ms_all = device_ms(lambda: ops.png_decode(blobs))
        say("%-26s B=%d: ops.png_decode (parse, pack, copy, kernels) %8.3f ms per call = %8.1f us per image (%.0f file bytes per image)"
            % (who, B, ms_all, 1e3 * ms_all / B, sum(map(len, blobs)) / B))
        with ThreadPoolExecutor(max_workers=8) as pool:
            ms8 = wall_ms(lambda: list(pool.map(host_decode, blobs)))
        ms1 = wall_ms(lambda: [host_decode(b) for b in blobs], reps=5)
        say("%-26s B=%d: Pillow on 8 threads %8.3f ms per batch = %8.1f us per image; on one thread %8.1f us per image"
            % (who, B, ms8, 1e3 * ms8 / B, 1e3 * ms1 / B))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
