"""CPU: the JPEG encoder's host side (include/ppst_hip.h ppst_jpeg_*: header, bound, workspace, argument checks), the
``format="jpeg"`` switch of the file front ends, and the judges of tests/jpeg_cases.py themselves -- nothing here launches a
kernel.  Pillow (libjpeg-turbo) is the outside reference: its tables for the header, its decoder and encoder for the model."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_cases as J  # noqa: E402

SIZES = [(1, 1), (17, 3), (41, 77), (600, 530), (1536, 2064)]
PNG_SHAPES = [(1, 1, 1), (1, 1, 3), (1, 640, 3), (480, 1, 1), (17, 3, 3), (200, 131, 1), (256, 256, 3), (512, 512, 3), (600, 530, 3),
              (1024, 1024, 3), (1024, 1024, 1), (4096, 4096, 3), (85, 257, 3)]          # test_png_cpu.SHAPES


def _header(H, W, C, quality, subsampling, cap=None):
    from ppst_amd._lib import lib
    ss = J.SS_NUMBER[subsampling]
    n = lib.ppst_jpeg_header(H, W, C, quality, ss, None, 0)
    assert n > 0, (H, W, C, quality, subsampling)
    buf = ctypes.create_string_buffer(b"\xa5" * (n + 8), n + 8)
    assert lib.ppst_jpeg_header(H, W, C, quality, ss, buf, n if cap is None else cap) == (n if cap is None or cap >= n else -1)
    return n, buf.raw


@pytest.mark.parametrize("C", [1, 3])
def test_header_segments_and_tables_equal_pillows(C):
    """Every quality 1 .. 100, both subsamplings, five sizes: the header parses, its segments come in the stated order, SOF0
    carries the size and the sampling factors, DRI the 96-block interval, and the DQT and DHT payloads are byte-equal to those
    of a file Pillow writes for the same settings; it also equals the host model's header; a cap too small writes nothing."""
    pillow = {}
    arr = J.field(1, 16, 16, 1.4)[:, :, :C].copy()
    for q in range(1, 101):
        for ss in J.SUBSAMPLINGS:
            pillow[(q, ss)] = J.parse(J.pillow_encode(arr, q, ss))
    for H, W in SIZES:
        for q in range(1, 101):
            for ss in J.SUBSAMPLINGS:
                n, raw = _header(H, W, C, q, ss)
                assert raw[n:] == b"\xa5" * 8, "wrote past the header"
                head = raw[:n]
                assert n == J.header_len(C) and head == J.header(H, W, C, q, ss, J.dri_mcus(C, ss)), (H, W, C, q, ss)
                p = J.parse(head + b"\xff\xd9")
                assert p["order"] == [0xD8, 0xE0] + [0xDB] * (1 if C == 1 else 2) + [0xC0] + [0xC4] * (2 if C == 1 else 4) + [0xDD, 0xDA]
                assert p["app0"] == b"JFIF\0\x01\x01\x00\x00\x01\x00\x01\x00\x00"
                f = 2 if (C == 3 and ss == "4:2:0") else 1
                assert p["sof"] == (8, H, W, [(1, f, f, 0)] + [(2, 1, 1, 1), (3, 1, 1, 1)][:C - 1])
                assert p["sos"] == [(1, 0, 0), (2, 1, 1), (3, 1, 1)][:C]
                assert p["dri"] == J.dri_mcus(C, ss) == 96 // (1 if C == 1 else (6 if f == 2 else 3))
                ref = pillow[(q, ss)]
                assert p["dqt"] == ref["dqt"], (C, q, ss)
                assert p["dht"] == ref["dht"], (C, q, ss)
    n, raw = _header(41, 77, C, 90, "4:2:0", cap=J.header_len(C) - 1)
    assert raw == b"\xa5" * (n + 8), "a refused call wrote"


def test_quantisation_tables_are_pillows_own():
    """The model's scaling is libjpeg's: Image.quantization of a Pillow file at the same quality, q = 1 .. 100."""
    import io
    from PIL import Image
    arr = J.field(1, 16, 16, 1.4)
    for q in range(1, 101):
        im = Image.open(io.BytesIO(J.pillow_encode(arr, q, "4:2:0")))
        got = {k: list(v) for k, v in im.quantization.items()}
        want = J.qtables(q)
        for t in (0, 1):
            assert got[t] in (want[t][J.ZIGZAG].tolist(), want[t].tolist()), (q, t)      # (zigzag or natural: Pillow's version decides)


def test_bound_is_the_stated_worst_case_and_monotonic():
    """ppst_jpeg_bound is the derivation of jpeg_cases.worst_case_bytes (a block's longest codes, x 2 for stuffing, pad and marker
    per interval, the header) rounded up to 16, positive for the PNG test's shapes, monotonic in H and in W; the workspace is
    positive, also for B = 0."""
    from ppst_amd._lib import lib
    for ss in J.SUBSAMPLINGS:
        n = J.SS_NUMBER[ss]
        for H, W, C in PNG_SHAPES + [(h, w, c) for h, w in SIZES for c in (1, 3)]:
            b = lib.ppst_jpeg_bound(H, W, C, n)
            want = J.worst_case_bytes(H, W, C, ss)
            assert b > 0 and b % 16 == 0 and want <= b < want + 16, (H, W, C, ss, b, want)
            for B in (0, 1, 8):
                assert lib.ppst_jpeg_ws(B, H, W, C, n) > 0, (B, H, W, C, ss)
        for C in (1, 3):
            for H in (1, 2, 17, 255, 256, 600):
                prev = 0
                for W in range(1, 700, 7):
                    b = lib.ppst_jpeg_bound(H, W, C, n)
                    assert b >= prev, (H, W, C)
                    prev = b
            for W in (1, 2, 17, 255, 256, 530):
                prev = 0
                for H in range(1, 700, 7):
                    b = lib.ppst_jpeg_bound(H, W, C, n)
                    assert b >= prev, (H, W, C)
                    prev = b
    # the model's files stay below it, the densest of them (uniform random pixels at q 100) included
    for name in ("random96", "random96_grey", "checker1", "17x3"):
        arr = J.image_set()[name]
        for ss in J.SUBSAMPLINGS:
            assert len(J.model_encode(arr, 100, ss)) <= lib.ppst_jpeg_bound(*arr.shape, J.SS_NUMBER[ss])


def test_argument_errors_need_no_gpu():
    from ppst_amd._lib import lib
    tok = ctypes.c_void_p(16)        # a non-null token: validation runs before anything is dereferenced or launched
    enc = lambda img, files, sizes, B, H, W, C, q, ss, work: lib.ppst_jpeg_encode(img, files, sizes, B, H, W, C, q, ss, work, None)
    assert enc(tok, tok, tok, 1, 8, 8, 2, 90, 2, tok) == -1            # C not in {1, 3}
    assert enc(tok, tok, tok, 1, 8, 8, 4, 90, 2, tok) == -1
    assert enc(tok, tok, tok, 1, 0, 8, 3, 90, 2, tok) == -1            # H < 1
    assert enc(tok, tok, tok, 1, 8, -3, 3, 90, 2, tok) == -1           # W < 1
    assert enc(tok, tok, tok, 1, 8, 65536, 3, 90, 2, tok) == -1        # beyond SOF0's 16 bits
    assert enc(tok, tok, tok, -1, 8, 8, 3, 90, 2, tok) == -1           # B < 0
    assert enc(tok, tok, tok, 1, 8, 8, 3, 0, 2, tok) == -1             # quality
    assert enc(tok, tok, tok, 1, 8, 8, 3, 101, 2, tok) == -1
    assert enc(tok, tok, tok, 1, 8, 8, 3, 90, 1, tok) == -1            # 4:2:2 is not built
    assert enc(tok, tok, tok, 1, 8, 8, 1, 90, 3, tok) == -1            # grey ignores WHICH of the two, not any number
    assert enc(tok, tok, tok, 1, 40000, 40000, 3, 90, 0, tok) == -1    # scan offsets beyond 32 bits
    assert enc(None, None, None, 1, 40000, 40000, 3, 90, 0, None) == -1   # ... reported ahead of the null check
    assert enc(None, None, None, 0, 8, 8, 3, 90, 2, None) == 0         # empty batch
    assert enc(None, tok, tok, 1, 8, 8, 3, 90, 2, tok) == -3
    assert enc(tok, None, tok, 1, 8, 8, 3, 90, 2, tok) == -3
    assert enc(tok, tok, None, 1, 8, 8, 3, 90, 2, tok) == -3
    assert enc(tok, tok, tok, 1, 8, 8, 3, 90, 2, None) == -3
    assert lib.ppst_jpeg_bound(8, 8, 2, 0) == -1 and lib.ppst_jpeg_bound(0, 8, 3, 0) == -1 and lib.ppst_jpeg_bound(8, 8, 3, 1) == -1
    assert lib.ppst_jpeg_bound(40000, 40000, 3, 2) == -1
    assert lib.ppst_jpeg_ws(1, 8, 8, 2, 0) == -1 and lib.ppst_jpeg_ws(-1, 8, 8, 3, 0) == -1
    assert lib.ppst_jpeg_header(8, 8, 3, 0, 0, None, 0) == -1 and lib.ppst_jpeg_header(8, 8, 2, 90, 0, None, 0) == -1
    assert lib.ppst_version() == 3                                      # no struct or existing entry point changed


def test_front_ends_refuse_bad_settings_before_the_tensor_is_touched():
    from ppst_amd import evaluation as EV

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError("the tensor was touched (.%s) before the settings were checked" % name)

    with pytest.raises(ValueError, match="gif"):
        EV.save_images(Untouchable(), ["a.gif"], format="gif")
    with pytest.raises(ValueError, match="quality"):
        EV.save_images(Untouchable(), ["a.jpg"], None, "device", format="jpeg", jpeg_quality=0)
    with pytest.raises(ValueError, match="quality"):
        EV.write_png_batch(Untouchable(), ["a.jpg"], None, "host", "jpeg", 101)
    with pytest.raises(ValueError, match="quality"):
        EV.write_png_batch(Untouchable(), ["a.jpg"], format="jpeg", jpeg_quality=90.0)
    with pytest.raises(ValueError, match="subsampling"):
        EV.write_png_batch(Untouchable(), ["a.jpg"], format="jpeg", jpeg_subsampling="4:2:2")
    with pytest.raises(ValueError, match="zip"):
        EV.save_images(Untouchable(), ["a.jpg"], encoder="zip", format="jpeg")
    with pytest.raises(ValueError):
        EV.evaluate_grid_folder(None, "/nonexistent", "/nonexistent", format="jpg")
    with pytest.raises(ValueError):
        EV.evaluate_grid_folder(None, "/nonexistent", "/nonexistent", format="jpeg", jpeg_subsampling=2)
    with pytest.raises(ValueError):
        EV.evaluate_swap_files(None, "a.png", "b.png", "/nonexistent", format="jpeg", jpeg_quality=500)
    with pytest.raises(ValueError):
        EV.evaluate_swap_files(None, "a.png", "b.png", "/nonexistent", png="gpu", format="jpeg")


def test_front_end_signatures_only_grew_at_the_end():
    import inspect
    from ppst_amd import evaluation as EV
    tail = ["format", "jpeg_quality", "jpeg_subsampling"]
    assert list(inspect.signature(EV.save_images).parameters) == ["images", "paths", "pool", "encoder"] + tail
    assert list(inspect.signature(EV.write_png_batch).parameters) == ["u8", "paths", "pool", "encoder"] + tail
    assert list(inspect.signature(EV.evaluate_swap_files).parameters) == [
        "model", "structure_path", "texture_path", "out_dir", "alphas", "load_size", "device", "png"] + tail
    assert list(inspect.signature(EV.evaluate_grid_folder).parameters) == [
        "model", "dataroot", "out_dir", "rank", "world", "smooth", "load_size", "device", "workers", "pair_batch", "image_batch", "png"] + tail
    for f in (EV.save_images, EV.write_png_batch, EV.evaluate_swap_files, EV.evaluate_grid_folder):
        d = {k: v.default for k, v in inspect.signature(f).parameters.items()}
        assert (d["format"], d["jpeg_quality"], d["jpeg_subsampling"]) == ("png", 90, "4:2:0")


def test_device_encoder_refuses_cpu_tensors():
    """No CPU fallback: the device encoder raises on a host tensor, like every op of the library; bad settings are a ValueError."""
    from ppst_amd import imageio, ops
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.jpeg_encode(torch.zeros(1, 4, 4, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="CUDA"):
        imageio.encode_jpeg(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), 50, "4:4:4")
    with pytest.raises(ValueError):
        ops.jpeg_encode(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), quality=0)
    with pytest.raises(ValueError):
        ops.jpeg_encode(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), subsampling="4:1:1")


# ------------------------------------------------------------------------------------------------------ the judge itself
@pytest.mark.parametrize("name", sorted(J.image_set()))
def test_model_files_decode_and_its_coder_inverts(name):
    """The float64 model's file of every image of the set (q 5 / 50 / 90 / 100, both subsamplings): Pillow decodes it to the
    right mode and size, the entropy decoder returns the model's coefficients, and coding them again returns the scan."""
    arr = J.image_set()[name]
    H, W, C = arr.shape
    for q in J.QUALITIES:
        for ss in J.SUBSAMPLINGS:
            blob = J.model_encode(arr, q, ss)
            mode, size, dec = J.pillow_decode(blob)
            assert mode == ("RGB" if C == 3 else "L") and size == (W, H), (name, q, ss)
            coefs, p = J.entropy_decode(blob)
            assert np.array_equal(coefs, J.model_coefficients(arr, q, ss)), (name, q, ss)
            assert J.entropy_encode(coefs, C, ss, p["dri"]) == p["scan"], (name, q, ss)
            if q >= 50 and min(H, W) >= 8 and name not in ("checker1", "random96", "random96_grey", "8x8", "16x16"):
                assert J.psnr(dec, arr) > 24.0, (name, q, ss, J.psnr(dec, arr))           # a picture, not noise


def test_model_other_restart_intervals_decode():
    """The model with one MCU row per interval (and with one interval): still Pillow's picture, the same coefficients."""
    arr = J.image_set()["41x77"]
    for ss, row in (("4:4:4", 10), ("4:2:0", 5)):
        want = J.model_coefficients(arr, 90, ss)
        for R in (row, 1, 1000):
            blob = J.model_encode(arr, 90, ss, R=R)
            assert J.pillow_decode(blob)[1] == (77, 41)
            coefs, p = J.entropy_decode(blob)
            assert p["dri"] == R and np.array_equal(coefs, want), (ss, R)


def test_model_against_pillows_encoder():
    """On the photo-like fields at q 50 / 90 / 100 the model's PSNR (through Pillow's decoder) is within 0.1 dB of Pillow's own
    encode or above it, and its files total at most 1.05 x Pillow's: the bars the device encoder is held to."""
    nm = npil = 0
    for name in J.PHOTO:
        arr = J.image_set()[name]
        for q in (50, 90, 100):
            for ss in J.SUBSAMPLINGS:
                m, p = J.model_encode(arr, q, ss), J.pillow_encode(arr, q, ss)
                pm, pp = J.psnr(J.pillow_decode(m)[2], arr), J.psnr(J.pillow_decode(p)[2], arr)
                print("%-12s q %3d %s model %6d  Pillow %6d  ratio %.4f  PSNR %+.3f dB" % (name, q, ss, len(m), len(p), len(m) / len(p), pm - pp))
                assert pm >= pp - 0.1, (name, q, ss, pm, pp)
                nm, npil = nm + len(m), npil + len(p)
    assert nm <= 1.05 * npil


def test_fixed_point_dct_error_is_what_is_stated():
    """The kernels' integer DCT, emulated in int64, against float64 over every image of the set and both subsamplings: the
    largest absolute error is the EPS_MEASURED jpeg_cases states (not above it, not far below), and EPS is twice that."""
    worst = 0.0
    for name, arr in J.image_set().items():
        for ss in J.SUBSAMPLINGS:
            blocks, _ = J.scan_blocks(arr, ss)
            worst = max(worst, np.abs(J.dct_fixed(blocks) / 2.0 ** 20 - J.dct_f64(blocks)).max())
    print("fixed-point DCT: largest error %.4f (stated %.4f, EPS %.4f)" % (worst, J.EPS_MEASURED, J.EPS))
    assert 0.9 * J.EPS_MEASURED <= worst <= J.EPS_MEASURED and J.EPS == 2 * J.EPS_MEASURED
    # and the integer quantiser is the float one wherever the fixed-point value is not within its error of a half
    arr = J.image_set()["photo96x136"]
    blocks, comps = J.scan_blocks(arr, "4:2:0")
    for q in J.QUALITIES:
        a, b = J.quantise(J.dct_fixed(blocks), J.block_q(comps, q)), J.quantise(J.dct_f64(blocks), J.block_q(comps, q))
        assert np.abs(a - b).max() <= 1 and (a != b).mean() < 0.02
