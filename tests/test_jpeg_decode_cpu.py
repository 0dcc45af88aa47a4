"""CPU: the JPEG decoder's host half.  The host model of tests/jpeg_decode_cases.py (clean stream, subsequence iteration, IDCT,
upsampling, colour) against Pillow for EQUALITY; the iteration against the sequential decode; ppst_jpeg_parse through ctypes
(fields, every refusal, truncated and corrupted files); the workspace size and the decode entry's argument checks; the front ends'
``decode=`` switch.  No GPU."""
import ctypes
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_cases as J  # noqa: E402
import jpeg_decode_cases as D  # noqa: E402

SETTINGS = [(q, ss) for q in J.QUALITIES for ss in J.SUBSAMPLINGS]


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as g
    g.build()
    from ppst_amd import ops
    return ops


def _desc(ops, blob):
    rc, d = ops.jpeg_parse(blob)
    assert rc == 0, rc
    return D.Desc(d)


def _equal_to_pillow(ops, blob, what, **kw):
    px, status, rounds, nsubs = D.model_decode(_desc(ops, blob), blob, **kw)
    mode, size, ref = J.pillow_decode(blob)
    assert status == 0, (what, status)
    assert px.shape == ref.shape and np.array_equal(px, ref), (what, int((px != ref).sum()))
    return rounds, nsubs


@pytest.mark.parametrize("opt", [False, True])
@pytest.mark.parametrize("name", D.SMALL)
def test_model_equals_pillow_small(ops, name, opt):
    """every quality x subsampling, with the standard and with per-file (optimize=True) Huffman tables; grey images are Pillow's
    "L" files with sampling factors 2 x 2"""
    arr = J.image_set()[name]
    for q, ss in SETTINGS:
        r, n = _equal_to_pillow(ops, D.pillow_file(arr, q, ss, opt), (name, q, ss, opt))
        print("%-14s q %3d %s opt %d: rounds %s of %s subsequences" % (name, q, ss, opt, r, n))
    if arr.shape[2] == 1:
        assert ops.jpeg_parse(D.pillow_file(arr, 90, "4:2:0"))[1].hs[0] == 2


@pytest.mark.parametrize("name", D.LARGE)
def test_model_equals_pillow_large(ops, name):
    r, n = _equal_to_pillow(ops, D.pillow_file(J.image_set()[name], 90, "4:2:0"), name)
    print("%-14s rounds %s of %s subsequences" % (name, r, n))


@pytest.mark.parametrize("name,R", [("41x77", None), ("160x136", None), ("64x700_grey", None), ("photo96x136", 32), ("200x232", 96)])
def test_model_equals_pillow_on_restart_files(ops, name, R):
    """jpeg_cases.model_encode's files: DRI 16 (4:2:0) / 32 (4:4:4) / 96 (grey and explicit), RSTm wraps beyond 8 intervals"""
    arr = J.image_set()[name]
    most = 0
    for ss in J.SUBSAMPLINGS:
        blob = J.model_encode(arr, 90, ss, R)
        d = _desc(ops, blob)
        assert d.dri == (R or J.dri_mcus(arr.shape[2], ss)) and d.NI == -(-d.nmcu // d.dri)
        _equal_to_pillow(ops, blob, (name, ss, R))
        most = max(most, d.NI)
    assert name != "160x136" or most > 8


ITER_CASES = [("8x8", 100, "4:4:4"), ("16x16", 90, "4:2:0"), ("17x3", 50, "4:2:0"), ("41x77", 90, "4:2:0"), ("41x77", 5, "4:4:4"),
              ("checker8", 100, "4:2:0"), ("photo41x77", 50, "4:4:4"), ("1x1_grey", 90, "4:4:4"), ("smooth", 5, "4:2:0")]


@pytest.mark.parametrize("name,quality,subsampling", ITER_CASES)
def test_iteration_equals_the_sequential_decode(ops, name, quality, subsampling):
    """The subsequence iteration at 2, 4 and the default number of words gives jpeg_cases.entropy_decode's coefficients (a plain
    sequential decode) and reaches its fixed point in at most #subsequences rounds."""
    arr = J.image_set()[name]
    files = [D.pillow_file(arr, quality, subsampling), D.pillow_file(arr, quality, subsampling, True)]
    if arr.shape[2] == 3:
        files.append(J.model_encode(arr, quality, subsampling, 4))
    for blob in files:
        d = _desc(ops, blob)
        if arr.shape[2] == 3:
            want, _ = J.entropy_decode(blob)
        for sw in (2, 4, 0):
            coefs, status, rounds, nsubs = D.model_coefficients(d, blob, sw)
            print("%-11s q %3d %s %5d bytes, %d words: rounds %s of %s subsequences" % (name, quality, subsampling, len(blob), sw or 32, rounds, nsubs))
            assert status == 0 and all(r <= n for r, n in zip(rounds, nsubs)), (sw, rounds, nsubs)
            if arr.shape[2] == 3:                 # (entropy_decode does not take Pillow's grey files: factors 2 x 2)
                assert np.array_equal(coefs, want), sw
            else:
                assert np.array_equal(coefs, D.model_coefficients(d, blob, 1 << 16)[0]), sw       # one subsequence: sequential


# ----------------------------------------------------------------------------------------------------------------- parser
def test_parser_fields_match_the_host_parser(ops):
    for name in ("41x77", "random96", "160x136"):
        arr = J.image_set()[name]
        for blob in (D.pillow_file(arr, 90, "4:2:0"), D.pillow_file(arr, 50, "4:4:4", True), J.model_encode(arr, 90, "4:2:0")):
            rc, d = ops.jpeg_parse(blob)
            p = J.parse(blob)
            _, H, W, comps = p["sof"]
            assert rc == 0 and (d.H, d.W, d.ncomp) == (H, W, len(comps)) and d.dri == p["dri"]
            assert [(d.hs[c], d.vs[c]) for c in range(3)] == [c[1:3] for c in comps] and d.ss == comps[0][1]
            assert d.scan_off == len(p["head"]) and d.scan_len == len(p["scan"])
            for c, (_, _, _, tq) in enumerate(comps):
                assert list(d.qt[c]) == p["dqt"][tq]
            for c, (_, td, ta) in enumerate(p["sos"]):
                assert (d.dc_tab[c], d.ac_tab[c]) == (td, ta)
            for (tc, ti), payload in p["dht"].items():
                t = 2 * tc + ti
                assert bytes(d.bits[t]) == payload[:16] and bytes(d.vals[t])[:len(payload) - 16] == payload[16:]


def _save(arr, **kw):
    from PIL import Image
    buf = io.BytesIO()
    im = kw.pop("image", None) or Image.fromarray(arr)
    im.save(buf, format="JPEG", **kw)
    return buf.getvalue()


def test_parser_refusals(ops):
    from PIL import Image
    arr = J.image_set()["photo41x77"]
    good = D.pillow_file(arr, 90, "4:2:0")
    code = lambda b: ops.jpeg_parse(b)[0]
    assert code(good) == 0
    assert code(_save(arr, progressive=True)) == -104
    assert code(_save(arr, subsampling=1)) == -107                               # 4:2:2
    assert code(_save(arr, image=Image.fromarray(arr).convert("CMYK"))) == -108
    try:
        rgb = _save(arr, keep_rgb=True)
    except (TypeError, OSError):
        rgb = None                                                               # a Pillow that cannot write it
    if rgb is not None and b"Adobe" in rgb:
        assert code(rgb) == -109
    # hand-made, libjpeg's rule for three components: JFIF says YCbCr; without it Adobe's transform says; without both the ids say
    adobe = b"\xff\xee" + bytes([0, 14]) + b"Adobe" + bytes([0, 100, 0, 0, 0, 0, 0])
    assert good[2:4] == b"\xff\xe0" and good[6:11] == b"JFIF\0"
    bare = good[:2] + good[4 + 256 * good[4] + good[5]:]                          # the JFIF APP0 gone
    assert code(bare) == 0
    assert code(bare[:2] + adobe + bare[2:]) == -109                             # transform 0: RGB
    assert code(bare[:2] + adobe[:-1] + b"\x01" + bare[2:]) == 0                 # transform 1: YCbCr
    assert code(good[:2] + adobe + good[2:]) == 0                                # JFIF wins: Pillow decodes this one as YCbCr too
    assert np.array_equal(J.pillow_decode(good[:2] + adobe + good[2:])[2], J.pillow_decode(good)[2])

    def with_ids(blob, ids):
        f, s_ = blob.index(b"\xff\xc0"), blob.index(b"\xff\xda")
        b = bytearray(blob)
        for c in range(3):
            b[f + 10 + 3 * c] = ids[c]
            b[s_ + 5 + 2 * c] = ids[c]
        return bytes(b)
    assert code(with_ids(bare, b"RGB")) == -109                                  # no marker, ids 'R' 'G' 'B': RGB to libjpeg
    assert code(with_ids(good, b"RGB")) == 0 and code(with_ids(bare, b"rgb")) == 0
    assert not np.array_equal(J.pillow_decode(with_ids(bare, b"RGB"))[2], J.pillow_decode(bare)[2])       # (Pillow agrees: other pixels)
    p = J.parse(good)
    sos = good.index(b"\xff\xda")
    one = good[:sos] + b"\xff\xda" + bytes([0, 8, 1, 1, 0x00, 0, 63, 0]) + good[len(p["head"]):]
    assert code(one) == -110                                                     # a scan of one component out of three
    sof = good.index(b"\xff\xc0")
    assert code(good[:sof + 4] + b"\x0c" + good[sof + 5:]) == -106               # 12 bits
    assert code(good[:sof + 5] + b"\0\0" + good[sof + 7:]) == -112               # H = 0
    assert code(good[:sof + 1] + b"\xc9" + good[sof + 2:]) == -105               # SOF9: arithmetic
    dqt = good.index(b"\xff\xdb")
    assert code(good[:dqt + 4] + b"\x10" + good[dqt + 5:]) == -111               # Pq = 1
    assert code(good[:len(p["head"]) - 3] + b"\x01\x3f\x00" + good[len(p["head"]):]) == -114        # Ss = 1
    assert code(good[:30]) == -101 and code(good[:-2]) == -101 and code(b"") == -101
    assert code(b"\x89PNG" + good) == -102
    dht = good.index(b"\xff\xc4")
    assert code(good[:dht + 5] + b"\x03" + good[dht + 6:]) == -113               # three codes of length 1
    assert code(good[:dht] + good[dht + 2 + 256 * good[dht + 2] + good[dht + 3]:]) == -113          # the first DHT segment (DC 0) gone
    # unknown and misplaced segments
    assert code(good[:2] + b"\xff\xd8" + good[2:]) == -103


def test_workspace_and_decode_arguments(ops):
    from ppst_amd import _lib
    lib = _lib.lib
    arr = J.image_set()["photo96x136"]

    def descs(blobs):
        a = (_lib.JpegDecImage * len(blobs))()
        for i, b in enumerate(blobs):
            assert lib.ppst_jpeg_parse(b, len(b), ctypes.byref(a[i])) == 0
        return a
    small, large = D.pillow_file(arr[:40, :40].copy(), 50, "4:2:0"), D.pillow_file(arr, 100, "4:4:4")
    ws = lambda blobs, sw=0: lib.ppst_jpeg_decode_ws(descs(blobs), len(blobs), sw)
    assert 0 < ws([]) < ws([small]) < ws([large]) < ws([large, small]) == ws([small, large])
    assert ws([large], 2) > ws([large], 4) > ws([large])                          # more subsequences, more state
    assert ws([small], 1) == -1 and ws([small], -3) == -1 and ws([small], 1 << 17) == -1
    assert lib.ppst_jpeg_decode_ws(None, 1, 0) == -3 and lib.ppst_jpeg_decode_ws(None, -1, 0) == -1
    bad = descs([small])
    bad[0].ss = 3
    assert lib.ppst_jpeg_decode_ws(bad, 1, 0) == -1
    # the decode entry: every refusal comes before a launch
    d = descs([small])
    tok = ctypes.c_void_p(4096)
    n, out_n = len(small), d[0].H * d[0].W * 3
    call = lambda **kw: lib.ppst_jpeg_decode(*[kw.get(k, v) for k, v in (("bytes", tok), ("nbytes", n), ("host", d), ("dev", tok), ("out", tok),
                                                                         ("out_bytes", out_n), ("status", tok), ("B", 1), ("sw", 0), ("work", tok),
                                                                         ("stream", None))])
    assert call(B=0) == 0 and call(B=-1) == -1 and call(sw=1) == -1
    assert call(nbytes=n - 3) == -1 and call(out_bytes=out_n - 1) == -1           # a file / an image outside its buffer
    for null in ("bytes", "dev", "out", "status", "work"):
        assert call(**{null: None}) == -3, null
    assert call(host=None) == -3
    assert call(work=ctypes.c_void_p(4100)) == -1                                 # alignment
    d[0].out_off = 16
    assert call() == -1
    d[0].out_off, d[0].scan_len = 0, -5
    assert call() == -1


def test_jpeg_info(ops):
    from ppst_amd import imageio
    arr = J.image_set()["41x77"]
    info = imageio.jpeg_info(J.model_encode(arr, 90, "4:2:0"))
    assert info["supported"] and (info["height"], info["width"], info["subsampling"], info["restart_interval"]) == (41, 77, "4:2:0", 16)
    assert imageio.jpeg_info(D.pillow_file(J.image_set()["1x1_grey"], 90, "4:2:0"))["subsampling"] == "grey"
    no = imageio.jpeg_info(_save(arr, progressive=True))
    assert not no["supported"] and no["code"] == -104 and "progressive" in no["reason"]


def test_front_ends_refuse_an_unknown_decoder(tmp_path):
    from ppst_amd import evaluation as EV
    from ppst_amd.training import CelebAMaskDataset
    with pytest.raises(ValueError, match="nonsense"):
        EV.load_images(["/nonexistent/a.jpg"], decode="nonsense")
    # the two evaluators' parameter lists are pinned (test_jpeg_cases_cpu): their switch is the thread's setting
    with pytest.raises(ValueError, match="nonsense"):
        with EV.decoder("nonsense"):
            pass
    EV._DECODE.value = "nonsense"                              # (behind the context manager's back: the evaluators check again)
    try:
        with pytest.raises(ValueError, match="nonsense"):
            EV.evaluate_swap_files(None, "/nonexistent/a.jpg", "/nonexistent/b.jpg", str(tmp_path / "o"))
        with pytest.raises(ValueError, match="nonsense"):
            EV.evaluate_grid_folder(None, "/nonexistent", str(tmp_path / "o"))
        with pytest.raises(ValueError, match="nonsense"):
            EV.load_images(["/nonexistent/a.jpg"])
    finally:
        EV._DECODE.value = "host"
    assert not (tmp_path / "o").exists()                       # before any work
    import threading
    seen = []
    with EV.decoder("device"):
        assert EV.current_decoder() == "device"
        t = threading.Thread(target=lambda: seen.append(EV.current_decoder()))
        t.start()
        t.join()
    assert EV.current_decoder() == "host" and seen == ["host"]  # per thread
    (tmp_path / "images").mkdir()
    (tmp_path / "images" / "a.jpg").write_bytes(b"")
    with pytest.raises(ValueError, match="nonsense"):
        CelebAMaskDataset(str(tmp_path), decode="nonsense")


# ------------------------------------------------------------------------------------------------- truncated and corrupted
def test_damaged_files_stay_in_bounds(ops):
    """Every prefix of a small file and 200 single-byte corruptions of its scan: the parser refuses or accepts each with one of its
    codes and a scan inside the file (a read past n would not show here: the stand-alone sanitizer program
    tests/jpeg_parse_san.cpp runs the same list with each file in a heap block of exactly its length);
    the host model, whose arrays raise on any index outside them, finishes every accepted one with a status and no exception."""
    files = D.damaged_files(D.damage_source())
    accepted, by_code, with_status = 0, {}, 0
    for n, blob in enumerate(files):
        rc, d = ops.jpeg_parse(blob)
        by_code[rc] = by_code.get(rc, 0) + 1
        assert rc == 0 or -114 <= rc <= -101, (n, rc)
        if rc != 0:
            continue
        accepted += 1
        assert 0 <= d.scan_off and d.scan_off + d.scan_len + 2 <= len(blob)
        for sw in (2, 0):
            px, status, rounds, nsubs = D.model_decode(D.Desc(d), blob, sw)
            assert px.shape == (d.H, d.W, 3) and all(r <= s + 1 for r, s in zip(rounds, nsubs))
        with_status += status != 0
    print("parser:", by_code, "accepted", accepted, "of them with a status", with_status)
    assert by_code.get(-101, 0) >= len(D.damage_source()) - 10 and accepted >= 150 and with_status > 0
