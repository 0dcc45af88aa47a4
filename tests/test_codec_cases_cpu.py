"""CPU: the cases of tests/codec_record.py reach what they are there for -- the piece and interval counts come out as stated, the
images are a function of their formula alone."""
import hashlib

import numpy as np

import codec_record as R


def test_piece_and_interval_counts():
    R.check_counts()
    assert R.PNG_PIECE == 32768 and R.JPEG_NBLK == 96
    for name, text in (("png.hip", "#define PNG_PIECE 32768"), ("jpeg.hip", "#define JPEG_NBLK 96")):
        with open(R.os.path.join(R.ROOT, "ppst_amd", "csrc", name)) as f:
            assert text in f.read()


def test_images_come_from_their_formulas():
    g = R.gradient(2, 5, 7, 3)
    assert g.dtype == np.uint8 and g[1, 4, 6, 2] == (7 * 6 + 13 * 4 + 29 * 2 + 31 + (6 * 4) % 251) & 255
    n = R.noise(1, 64, 64, 3).ravel()
    x = 20240229
    for i in range(1000):                                    # the doubling fill equals the LCG stepped one at a time
        assert n[i] == x >> 24
        x = (1664525 * x + 1013904223) & 0xFFFFFFFF
    assert len(np.unique(n)) == 256                          # noise: nothing for a Huffman code to gain
    assert hashlib.sha256(R.noise(1, 64, 64, 3).tobytes()).hexdigest() == hashlib.sha256(n.tobytes()).hexdigest()
    assert np.unique(R.constant(1, 40, 40, 3)).tolist() == [77]
