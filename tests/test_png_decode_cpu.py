"""CPU: the PNG decoder's host half (ppst_png_parse, the entry points' argument checks) and the host model of its device half
(tests/png_decode_cases.py: gather, tables, the subsequence iteration, prefix and second decode, pointer jumping in an adversarial
order, unfilter and store, every array index checked).  The judges are Pillow (pixels) and ``zlib.decompress`` (the inflate)."""
import ctypes
import os
import re
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_decode_cases as P  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# The Python model walks files up to MODEL_BYTES in every family and the larger ones (200x232, 8x2100, 2100x8, 64x700_grey,
# 600x530, field512, far_match, ...) in MODEL_FAMILIES only; at 2- and 4-word subsequences the larger ones are LARGE_AT_SHORT of
# "mixed".  tests/test_gpu_png_decode.py runs every file of every family at all three lengths on the device.
MODEL_BYTES = 24000
MODEL_FAMILIES = ("mixed", "pillow")
LARGE_AT_SHORT = ("far_match", "600x530", "200x232")
FIELDS = ("H", "W", "colour", "channels", "nspans", "first_idat", "nidat", "idat_bytes", "file_len")


def _c_parse(blob):
    from ppst_amd import ops
    rc, d, spans = ops.png_parse(blob)
    return rc, {k: getattr(d, k) for k in FIELDS}, [(s.type, s.off, s.len, s.crc, s.idat) for s in spans[:d.nspans]] if rc == 0 else []


def _zs(blob, spans):
    return b"".join(blob[s[1]:s[1] + s[2]] for s in spans if s[4])


@pytest.mark.parametrize("family", P.all_families())
def test_parser_accepts_the_whole_set_and_agrees_with_the_python_parser(family):
    """every file of every family: code 0 (the GPU test may leave out no case), and descriptor and span table equal field by
    field to the Python parser's"""
    names, blobs = P.family_files(family)
    assert len(names) >= len(P.image_set())
    for name, blob in zip(names, blobs):
        rc, d, spans = _c_parse(blob)
        prc, pd, pspans = P.parse(blob)
        assert rc == 0 and prc == 0, (family, name, rc, prc)
        assert d == pd, (family, name, d, pd)
        assert spans == pspans, (family, name)


@pytest.mark.parametrize("family", P.all_families())
def test_model_equals_pillow(family):
    """The whole decoder as the device runs it, in Python, on the image set (files above MODEL_BYTES in two families only: the
    model is Python): status 0, Pillow's pixels, the iteration within #subsequences rounds per window (checked inside the
    model), pointer jumping -- constant image included -- within ceil(log2 n) + 1 rounds."""
    names, blobs = P.family_files(family)
    seen_far = 0
    for name, blob in zip(names, blobs):
        if len(blob) > MODEL_BYTES and family not in MODEL_FAMILIES:
            continue
        rc, d, spans = P.parse(blob)
        out = P.model_decode(blob, d, spans)
        assert out.status == 0, (family, name, out.status)
        ref = P.pillow_pixels(blob)
        assert out.pixels.shape == ref.shape and np.array_equal(out.pixels, ref), (family, name)
        n = d["H"] * (1 + d["W"] * d["channels"])
        assert out.jump_rounds <= P.log2_ceil(n) + 1, (family, name, out.jump_rounds, n)
        seen_far += out.far
    if family == "mixed":
        assert seen_far > 100            # the far-match file does hold matches of length 258 at distance exactly 32768


@pytest.mark.parametrize("words", [2, 4, 8, 0])
def test_iteration_equals_sequential_inflate(words):
    """The subsequence iteration at 64-, 128-, 256-bit and the default (128-bit) subsequences + second decode + pointer jumping give the bytes of
    a one-token-at-a-time inflate with the same tables, which gives zlib's.  Files up to MODEL_BYTES of four families, and of
    "mixed" also the far-match file, 600 x 530 and 200 x 232 (the other large ones run at the default length in
    test_model_equals_pillow)."""
    for family in ("mixed", "pillow", "fixed", "level9"):
        names, blobs = P.family_files(family)
        for name, blob in zip(names, blobs):
            if len(blob) > MODEL_BYTES and not (family == "mixed" and name in LARGE_AT_SHORT):
                continue
            rc, d, spans = P.parse(blob)
            zs = _zs(blob, spans)
            ref = zlib.decompress(zs)
            if words == 0:
                assert P.sequential_inflate(zs) == ref, (family, name)
            inf = P.Inflate(zs, len(ref), words)
            assert inf.bits == 0 and inf.final and inf.outpos == len(ref), (family, name, inf.bits)
            assert P.jump_rounds(inf.src, seed=words) <= P.log2_ceil(len(ref)) + 1
            assert inf.raw[inf.src].tobytes() == ref, (family, name, words)


def test_mode_rgb_mirror_in_the_model():
    for name in ("1x1_grey", "41x77_rgba", "17x3", "random96_grey"):
        blob = P.make_png(P.image_set()[name])
        rc, d, spans = P.parse(blob)
        out = P.model_decode(blob, d, spans, expand_grey=True, drop_alpha=True, mirror=True)
        assert np.array_equal(out.pixels, P.pillow_pixels(blob, "RGB")[:, ::-1]), name


def test_every_refusal_has_its_code_and_text():
    from ppst_amd import _lib, imageio
    files = P.refusal_files()
    header = open(os.path.join(ROOT, "include", "ppst_hip.h")).read()
    codes = {int(v): k for k, v in re.findall(r"#define (PPST_PNG_E_\w+) \((-\d+)\)", header)}
    assert sorted(files) == sorted(c for c in codes if c != _lib.PNG_E_SPANS) and sorted(_lib.PNG_REFUSALS) == sorted(files)
    for code, blob in list(files.items()) + P.more_refusals():
        rc, d, spans = _c_parse(blob)
        prc, pd, _ = P.parse(blob)
        assert rc == code and prc == code, (codes[code], rc, prc)
        assert d == pd, (codes[code], d, pd)
        info = imageio.png_info(blob)
        assert info == {"supported": False, "code": code, "reason": _lib.PNG_REFUSALS[code]}
    bits = {int(v): k for k, v in re.findall(r"#define (PPST_PNG_S_\w+) (\d+)", header)}
    assert sorted(bits) == sorted(_lib.PNG_STATUS_BITS) == [1 << k for k in range(10)]
    good = P.make_png(P.image_set()["17x3"], idat_cuts=7)
    info = imageio.png_info(good)
    assert info["supported"] and (info["height"], info["width"], info["colour_type"], info["channels"]) == (17, 3, 2, 3)
    assert [c[0] for c in info["chunks"]] == ["IHDR"] + ["IDAT"] * info["idat_chunks"] + ["IEND"] and info["idat_chunks"] > 3


def test_span_array_too_small_is_a_code_of_its_own():
    from ppst_amd import _lib
    blob = P.make_png(P.image_set()["17x3"], idat_cuts="bytes")
    d = _lib.PngDecImage()
    spans = (_lib.PngSpan * 3)()
    assert _lib.lib.ppst_png_parse(blob, len(blob), ctypes.byref(d), spans, 3) == _lib.PNG_E_SPANS
    need = d.nspans
    assert need == P.parse(blob)[1]["nspans"] > 3
    assert _lib.lib.ppst_png_parse(blob, len(blob), ctypes.byref(d), None, 0) == _lib.PNG_E_SPANS and d.nspans == need
    spans = (_lib.PngSpan * need)()
    assert _lib.lib.ppst_png_parse(blob, len(blob), ctypes.byref(d), spans, need) == 0
    assert [(s.type, s.off, s.len, s.crc, s.idat) for s in spans] == P.parse(blob)[2]


def test_robustness_corpus():
    """Every prefix of one small file, 200 single-byte corruptions of its chunk data, 200 more with the chunk CRCs recomputed
    (so the inflate's own error paths are reached).  For each file exactly one of two things holds: the parser refuses it or the
    model sets a status; or Pillow opens the file and the pixels are equal.  The two parsers agree, and the model finishes
    within its bounds either way (its own checks raise otherwise)."""
    refused, flagged, decoded, by_bit = 0, 0, 0, {}
    for name, blob in P.corpus():
        rc, d, spans = _c_parse(blob)
        prc, pd, pspans = P.parse(blob)
        assert rc == prc, (name, rc, prc)
        if rc != 0:
            refused += 1
            continue
        assert d == pd and spans == pspans, name
        out = P.model_decode(blob, d, spans)
        if out.status:
            flagged += 1
            for k in range(10):
                if out.status & (1 << k):
                    by_bit[1 << k] = by_bit.get(1 << k, 0) + 1
            assert out.pixels is None or out.pixels.shape == (d["H"], d["W"], d["channels"])
            continue
        ref = P.pillow_pixels(blob)                 # (raises if Pillow does not open it: then the model missed a fault)
        assert np.array_equal(out.pixels, ref), name
        decoded += 1
    print("refused %d, status %d %s, decoded %d" % (refused, flagged, by_bit, decoded))
    assert refused > 1000 and flagged > 300
    # the corruptions behind recomputed CRCs do reach the inflate's own checks
    assert by_bit.get(P.S_CRC, 0) >= 190 and sum(v for k, v in by_bit.items() if k not in (P.S_CRC,)) >= 100


def test_damaged_files_in_the_model():
    """the three damaged files of the GPU test: each sets a status in the model (bad CRC; bad Adler-32 behind a good CRC; a
    stream cut in half behind a good CRC)"""
    good = P.make_png(P.image_set()["photo41x77"])
    want = (P.S_CRC, P.S_ADLER, P.S_STREAM)
    for blob, bit in zip(P.damaged_files(good), want):
        rc, d, spans = P.parse(blob)
        assert rc == 0
        assert P.model_decode(blob, d, spans).status & bit, bit


def test_argument_errors_need_no_gpu():
    import torch
    from ppst_amd import _lib, imageio, ops
    lib = _lib.lib
    d = _lib.PngDecImage()
    spans = (_lib.PngSpan * 4)()
    blob = P.make_png(P.image_set()["17x3"])
    assert lib.ppst_png_parse(blob, len(blob), None, spans, 4) == -3
    assert lib.ppst_png_parse(None, 5, ctypes.byref(d), spans, 4) == -3
    assert lib.ppst_png_parse(None, 0, ctypes.byref(d), spans, 4) == P.E_TRUNCATED
    assert lib.ppst_png_parse(blob, -1, ctypes.byref(d), spans, 4) == -1
    assert lib.ppst_png_parse(blob, len(blob), ctypes.byref(d), spans, -1) == -1
    assert lib.ppst_png_parse(blob, len(blob), ctypes.byref(d), None, 4) == -3
    rc, good, sp = ops.png_parse(blob)
    assert rc == 0
    descs = (_lib.PngDecImage * 1)(good)
    assert lib.ppst_png_decode_ws(descs, 1, 0) > 0 and lib.ppst_png_decode_ws(descs, 0, 0) > 0
    assert lib.ppst_png_decode_ws(descs, 1, 8) == lib.ppst_png_decode_ws(descs, 1, 0)      # the workspace does not depend on it
    for sw in (1, -2, 129):
        assert lib.ppst_png_decode_ws(descs, 1, sw) == -1
    assert lib.ppst_png_decode_ws(descs, -1, 0) == -1 and lib.ppst_png_decode_ws(None, 1, 0) == -3
    for field, value in (("H", 0), ("channels", 2), ("colour", 3), ("nidat", 0), ("first_idat", 5), ("idat_bytes", 1 << 29), ("file_off", -1)):
        bad = (_lib.PngDecImage * 1)(good)
        setattr(bad[0], field, value)
        assert lib.ppst_png_decode_ws(bad, 1, 0) == -1, field
    tok = ctypes.c_void_p(16)
    dec = lambda descs=descs, files=tok, nbytes=1 << 20, dd=tok, sp=tok, out=tok, ob=1 << 20, st=tok, B=1, sw=0, work=tok: \
        lib.ppst_png_decode(files, nbytes, descs, dd, sp, out, ob, st, B, sw, work, None)
    assert dec(B=0) == 0 and dec(B=0, files=None, descs=None) == 0
    assert dec(B=-1) == -1 and dec(sw=1) == -1 and dec(descs=None) == -3
    assert dec(nbytes=len(blob) - 1) == -1                      # the file would lie outside the buffer
    assert dec(ob=17 * 3 * 3 - 1) == -1                          # the image would
    for null in ("files", "dd", "sp", "out", "st", "work"):
        assert dec(**{null: None}) == -3, null
    for odd in ("dd", "sp", "out", "work"):
        assert dec(**{odd: ctypes.c_void_p(20)}) == -1, odd
    with pytest.raises(RuntimeError, match="CUDA"):
        imageio.decode_png([blob], device="cpu")
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.png_decode([blob], device=torch.device("cpu"))
    with pytest.raises(ValueError, match="mode"):
        imageio.decode_png([blob], mode="L")
