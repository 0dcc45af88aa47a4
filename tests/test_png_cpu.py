"""CPU: the PNG encoder's size contract and argument checks (include/ppst_hip.h ppst_png_*), and the ``encoder`` switch of
evaluation.save_images -- nothing here launches a kernel."""
import ctypes

import pytest
import torch

SHAPES = [(1, 1, 1), (1, 1, 3), (1, 640, 3), (480, 1, 1), (17, 3, 3), (200, 131, 1), (256, 256, 3), (512, 512, 3), (600, 530, 3),
          (1024, 1024, 3), (1024, 1024, 1), (4096, 4096, 3), (85, 257, 3)]
PIECE = 32768            # bytes of the filtered stream per deflate block / IDAT chunk (PNG_PIECE of csrc/png.hip)


def stream_bytes(H, W, C):
    return H * (1 + W * C)


def all_stored_size(H, W, C):
    """A PNG whose zlib stream is stored blocks only, one IDAT chunk: signature, IHDR, IDAT frame, zlib header, the bytes,
    five per stored block, Adler-32, IEND."""
    n = stream_bytes(H, W, C)
    return 8 + 25 + 12 + 2 + n + 5 * -(-n // 65535) + 4 + 12


def all_stored_size_of_layout(H, W, C):
    """The same worst case in the encoder's own layout: every 32 KB piece is an IDAT chunk of its own (12) around one stored
    block (5), which needs no aligning block behind it; the Adler-32 travels in a last IDAT chunk (12 + 4)."""
    n = stream_bytes(H, W, C)
    return 8 + 25 + 2 + n + (12 + 5) * -(-n // PIECE) + (12 + 4) + 12


def test_bound_covers_the_all_stored_file():
    from ppst_amd._lib import lib
    assert len(SHAPES) >= 12
    for H, W, C in SHAPES:
        b = lib.ppst_png_bound(H, W, C)
        assert all_stored_size_of_layout(H, W, C) >= all_stored_size(H, W, C)
        assert b >= all_stored_size_of_layout(H, W, C), (H, W, C, b)
        assert b <= all_stored_size_of_layout(H, W, C) + 16, (H, W, C, b)        # and is not a guess far above it


def test_bound_is_monotonic_and_workspace_positive():
    from ppst_amd._lib import lib
    for C in (1, 3):
        for H in (1, 2, 17, 255, 256, 600):
            prev = 0
            for W in range(1, 700, 7):
                b = lib.ppst_png_bound(H, W, C)
                assert b >= prev, (H, W, C)
                prev = b
        for W in (1, 2, 17, 255, 256, 530):
            prev = 0
            for H in range(1, 700, 7):
                b = lib.ppst_png_bound(H, W, C)
                assert b >= prev, (H, W, C)
                prev = b
    for B in (0, 1, 8):
        for H, W, C in SHAPES:
            assert lib.ppst_png_ws(B, H, W, C) > 0, (B, H, W, C)


def test_argument_errors_need_no_gpu():
    from ppst_amd._lib import lib
    tok = ctypes.c_void_p(16)        # a non-null token: validation runs before anything is dereferenced or launched
    enc = lambda img, files, sizes, B, H, W, C, work: lib.ppst_png_encode(img, files, sizes, B, H, W, C, work, None)
    assert enc(tok, tok, tok, 1, 8, 8, 2, tok) == -1               # C not in {1, 3}
    assert enc(tok, tok, tok, 1, 8, 8, 4, tok) == -1
    assert enc(tok, tok, tok, 1, 0, 8, 3, tok) == -1               # H < 1
    assert enc(tok, tok, tok, 1, 8, -3, 3, tok) == -1              # W < 1
    assert enc(tok, tok, tok, -1, 8, 8, 3, tok) == -1              # B < 0
    assert enc(tok, tok, tok, 1, 40000, 40000, 3, tok) == -1       # filtered stream beyond 32-bit offsets
    assert enc(None, None, None, 1, 40000, 40000, 3, None) == -1   # ... reported ahead of the null check
    assert enc(None, None, None, 0, 8, 8, 3, None) == 0            # empty batch
    assert enc(None, tok, tok, 1, 8, 8, 3, tok) == -3
    assert enc(tok, None, tok, 1, 8, 8, 3, tok) == -3
    assert enc(tok, tok, None, 1, 8, 8, 3, tok) == -3
    assert enc(tok, tok, tok, 1, 8, 8, 3, None) == -3
    assert lib.ppst_png_bound(8, 8, 2) == -1 and lib.ppst_png_bound(0, 8, 3) == -1 and lib.ppst_png_bound(40000, 40000, 3) == -1
    assert lib.ppst_png_ws(1, 8, 8, 2) == -1 and lib.ppst_png_ws(-1, 8, 8, 3) == -1
    assert lib.ppst_version() == 3                                  # no struct or existing entry point changed


def test_unknown_encoder_is_refused_before_the_tensor_is_touched():
    from ppst_amd import evaluation as EV

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError("save_images touched its tensor (.%s) before checking the encoder" % name)

    with pytest.raises(ValueError, match="zip"):
        EV.save_images(Untouchable(), ["a.png"], encoder="zip")
    with pytest.raises(ValueError):
        EV.write_png_batch(Untouchable(), ["a.png"], None, "")
    with pytest.raises(ValueError):
        EV.evaluate_grid_folder(None, "/nonexistent", "/nonexistent", png="zip")
    with pytest.raises(ValueError):
        EV.evaluate_swap_files(None, "a.png", "b.png", "/nonexistent", png="gpu")


def test_device_encoder_refuses_cpu_tensors():
    """No CPU fallback: the device encoder raises on a host tensor, like every op of the library."""
    from ppst_amd import imageio, ops
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.png_encode(torch.zeros(1, 4, 4, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="CUDA"):
        imageio.encode_png(torch.zeros(1, 4, 4, 3, dtype=torch.uint8))
