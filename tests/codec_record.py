"""Run the PNG and the JPEG encoder on the GPU over a fixed set of images and record the size and sha256 of every file.

    python tests/codec_record.py [OUT.json]        (default: tests/golden/codec_parent.json)

Both encoders are integer code: the bytes of a file are a function of the pixels alone, and the pixels come from closed
formulas below (no random generator), so two commits can be compared to the byte.  tests/golden/codec_parent.json was written by
this tool on an MI355X with the library of commit 321bf68, the last one in which each of the four coders had its own copy of the
workgroup scan, the slot-to-file copy and the Adler-32 join, before csrc/codec_common.h stated them once;
tests/test_gpu_codec_parent.py runs the working tree and asserts the same sizes and hashes.  Check out that commit, copy this file
over, build, and run it to see where the JSON comes from.

Every case is the smallest shape at which a path of the shared code can go wrong; ``count`` is the number of deflate pieces
(PNG_PIECE = 32768 bytes of the filtered stream, csrc/png.hip) or of restart intervals (JPEG_NBLK = 96 blocks, csrc/jpeg.hip) per
image that the case is there for: ``check_counts`` works them out from the shapes, on the CPU.
"""
import collections
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np

PNG_PIECE, JPEG_NBLK = 32768, 96
DOC = ("size and sha256 of every file the PNG and the JPEG encoder write for the cases of tests/codec_record.py, written by that tool "
       "on an MI355X with the library of commit 321bf68 (the parent of the commit that added csrc/codec_common.h)")


def gradient(B, H, W, C):
    b, y, x, c = np.ogrid[:B, :H, :W, :C]
    return ((7 * x + 13 * y + 29 * c + 31 * b + (x * y) % 251) & 255).astype(np.uint8)


def noise(B, H, W, C, seed=20240229):
    """the top byte of a 32-bit LCG (x <- 1664525 x + 1013904223), filled by doubling: x[i + m] = A_m x[i] + C_m"""
    n = B * H * W * C
    v = np.empty(n, np.uint64)
    v[0] = seed
    a, c, m = 1664525, 1013904223, 1
    while m < n:
        k = min(m, n - m)
        v[m:m + k] = (v[:k] * np.uint64(a) + np.uint64(c)) & np.uint64(0xFFFFFFFF)
        a, c, m = (a * a) & 0xFFFFFFFF, (a * c + c) & 0xFFFFFFFF, 2 * m
    return (v >> np.uint64(24)).astype(np.uint8).reshape(B, H, W, C)


def constant(B, H, W, C):
    return np.full((B, H, W, C), 77, np.uint8)


# coder, image formula, (B, H, W, C), encoder settings, pieces / intervals per image, what the case reaches
Case = collections.namedtuple("Case", "id coder make shape settings count reaches")
CASES = [
    Case("png-1x1-grey", "png", gradient, (1, 1, 1, 1), (), 1, "smallest image"),
    Case("png-3x5-rgb", "png", gradient, (1, 3, 5, 3), (), 1, "small RGB"),
    Case("png-constant-40x40", "png", constant, (1, 40, 40, 3), (), 1, "a code with fewer than two symbols: a stored block"),
    Case("png-noise-64x64", "png", noise, (1, 64, 64, 3), (), 1, "stored wins on size"),
    Case("png-gradient-97x113", "png", gradient, (1, 97, 113, 3), (), 2, "two pieces, the aligning empty stored block"),
    Case("png-gradient-2900-grey", "png", gradient, (1, 2900, 2900, 1), (), 257, "the layout kernel's second round"),
    Case("png-batch3-5x7", "png", gradient, (3, 5, 7, 3), (), 1, "a batch through the shared copy"),
    Case("jpeg-1x1-grey", "jpeg", gradient, (1, 1, 1, 1), (90, "4:2:0"), 1, "smallest image"),
    Case("jpeg-8x8-grey", "jpeg", gradient, (1, 8, 8, 1), (90, "4:2:0"), 1, "one block"),
    Case("jpeg-17x23-420", "jpeg", gradient, (1, 17, 23, 3), (90, "4:2:0"), 1, "partial MCUs of 16 x 16"),
    Case("jpeg-17x23-444", "jpeg", gradient, (1, 17, 23, 3), (90, "4:4:4"), 1, "partial MCUs of 8 x 8"),
    Case("jpeg-64x48-444", "jpeg", gradient, (1, 64, 48, 3), (90, "4:4:4"), 2, "144 blocks: two restart intervals"),
    Case("jpeg-1280-grey", "jpeg", gradient, (1, 1280, 1280, 1), (90, "4:2:0"), 267, "the layout kernel's second scan round"),
    Case("jpeg-batch3-17x23", "jpeg", gradient, (3, 17, 23, 3), (90, "4:2:0"), 1, "batched slots"),
    Case("jpeg-17x23-q25", "jpeg", gradient, (1, 17, 23, 3), (25, "4:2:0"), 1, "another quantisation table"),
    Case("jpeg-17x23-q100", "jpeg", gradient, (1, 17, 23, 3), (100, "4:2:0"), 1, "quantisers of 1"),
]


def count(c):
    """deflate pieces / restart intervals per image of a case, from its shape"""
    B, H, W, C = c.shape
    if c.coder == "png":
        return -(-H * (1 + W * C) // PNG_PIECE)
    mcu, bpm = (8, 1) if C == 1 else ((16, 6) if c.settings[1] == "4:2:0" else (8, 3))
    return -(-(-(-H // mcu) * -(-W // mcu)) // (JPEG_NBLK // bpm))


def check_counts():
    for c in CASES:
        assert count(c) == c.count, (c.id, count(c), c.count)
    by = {c.id: c for c in CASES}
    assert by["png-gradient-2900-grey"].count > 256 and by["jpeg-1280-grey"].count > 256      # a second round of 256 threads


def record(imageio, device="cuda"):
    """-> {case id: {"sizes": [...], "sha256": [...]}}, one entry per file of the case's batch"""
    import torch
    check_counts()
    out = {}
    for c in CASES:
        u8 = torch.from_numpy(c.make(*c.shape)).to(device)
        files = imageio.encode_png(u8) if c.coder == "png" else imageio.encode_jpeg(u8, *c.settings)
        out[c.id] = {"sizes": [len(f) for f in files], "sha256": [hashlib.sha256(f).hexdigest() for f in files]}
    return out


if __name__ == "__main__":
    from ppst_amd import imageio
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "codec_parent.json")
    rec = record(imageio)
    rec["_doc"] = DOC
    with open(path, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path, len(rec) - 1, "cases")
