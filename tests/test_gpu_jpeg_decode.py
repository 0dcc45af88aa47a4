"""GPU: the JPEG decoder (csrc/jpeg_decode.hip, ops.jpeg_decode, imageio.decode_jpeg, the ``decode="device"`` front ends).
The judge is Pillow's decoder (libjpeg-turbo) on the same bytes, for EQUALITY -- never the decoder under test."""
import functools
import io
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_cases as J  # noqa: E402
import jpeg_decode_cases as D  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = sorted(J.image_set())
SETTINGS = [(q, ss) for q in J.QUALITIES for ss in J.SUBSAMPLINGS]


def _dev():
    return torch.device("cuda", 0)


@functools.lru_cache(None)
def _pillow_files(quality, subsampling, optimize):
    return tuple(D.pillow_file(J.image_set()[n], quality, subsampling, optimize) for n in NAMES)


@functools.lru_cache(None)
def _own_files(quality, subsampling):
    """imageio.encode_jpeg's files of the whole set (one call per shape: the encoder batches equal shapes)"""
    from ppst_amd import imageio
    return tuple(imageio.encode_jpeg(torch.from_numpy(J.image_set()[n][None].copy()).to(_dev()), quality, subsampling)[0] for n in NAMES)


@functools.lru_cache(None)
def _ref(blob):
    return J.pillow_decode(blob)[2]


def _check_batch(blobs, what, **kw):
    """one batched call over `blobs`: every status 0, every image equal to Pillow's decode of the same bytes"""
    from ppst_amd import ops
    views, status, rounds = ops.jpeg_decode(list(blobs), rounds=True, **kw)
    status, rounds = status.cpu().tolist(), rounds.cpu().tolist()
    print("%s: rounds %s" % (what, rounds))
    assert status == [0] * len(blobs), (what, status)
    for n, (v, blob) in enumerate(zip(views, blobs)):
        ref = _ref(blob)
        got = v.cpu().numpy()
        assert got.shape == ref.shape, (what, n, got.shape, ref.shape)
        assert np.array_equal(got, ref), (what, n, int((got != ref).sum()))
    return views


@pytest.mark.parametrize("optimize", [False, True])
@pytest.mark.parametrize("quality,subsampling", SETTINGS)
def test_pillow_files_decode_to_pillows_pixels(quality, subsampling, optimize):
    """The whole image set, 1 x 1 to 2100 x 8, grey and colour, written by Pillow (no restart markers: one Huffman stream per
    file; ``optimize``: per-file Huffman tables), in ONE batched call."""
    _check_batch(_pillow_files(quality, subsampling, optimize), "pillow q%d %s opt %d" % (quality, subsampling, optimize))


@pytest.mark.parametrize("quality,subsampling", SETTINGS)
def test_own_files_decode_to_pillows_pixels(quality, subsampling):
    """imageio.encode_jpeg's files (DRI 96 blocks, RSTm wraps at the larger images): one workgroup per interval."""
    _check_batch(_own_files(quality, subsampling), "own q%d %s" % (quality, subsampling))


@pytest.mark.parametrize("subseq_words", [2, 4])
@pytest.mark.parametrize("family", ["pillow", "pillow-optimize", "own"])
@pytest.mark.parametrize("quality,subsampling", SETTINGS)
def test_short_subsequences(quality, subsampling, family, subseq_words):
    """The same batched calls -- every setting, Pillow's files with the standard and with per-file Huffman tables, the encoder's own
    -- at 64- and 128-bit subsequences: many per tiny image, blocks that straddle several, many rounds to the fixed point."""
    blobs = _own_files(quality, subsampling) if family == "own" else _pillow_files(quality, subsampling, family == "pillow-optimize")
    _check_batch(blobs, "%s q%d %s sw %d" % (family, quality, subsampling, subseq_words), subseq_words=subseq_words)


def test_more_subsequences_than_threads():
    """256^2 random pixels at q 100, 4:4:4, 64-bit subsequences: far more of them than the workgroup has threads (the lane loop)."""
    arr = np.random.default_rng(5).integers(0, 256, (256, 256, 3), dtype=np.uint8)
    blob = D.pillow_file(arr, 100, "4:4:4")
    assert 8 * len(blob) // 64 > 4 * 1024
    _check_batch([blob], "random256 sw 2", subseq_words=2)


def test_segment_of_more_chunks_than_the_offsets_workgroup_has_threads():
    """520^2 random pixels at q 100, 4:4:4: an entropy-coded segment above 1 MiB, more than 256 chunks of 4096 bytes -- the second
    round of jd_offsets_kernel's loop over the workgroup scan (csrc/codec_common.h), whose base carries over from the first."""
    from ppst_amd import ops
    arr = np.random.default_rng(6).integers(0, 256, (520, 520, 3), dtype=np.uint8)
    blob = D.pillow_file(arr, 100, "4:4:4")
    rc, d = ops.jpeg_parse(blob)
    assert rc == 0 and d.scan_len > 256 * 4096, d.scan_len
    _check_batch([blob], "random520")


def test_mirror_expand_grey_and_batch_independence():
    from ppst_amd import ops
    blobs = list(_pillow_files(90, "4:2:0", False))
    plain, status = ops.jpeg_decode(blobs)
    assert status.cpu().tolist() == [0] * len(blobs)
    flags = [n % 2 == 0 for n in range(len(blobs))]
    mirrored, _ = ops.jpeg_decode(blobs, mirror=flags)
    for n, (a, b) in enumerate(zip(plain, mirrored)):
        want = a.cpu().numpy()[:, ::-1] if flags[n] else a.cpu().numpy()
        assert np.array_equal(b.cpu().numpy(), want), NAMES[n]
    from PIL import Image
    rgb, _ = ops.jpeg_decode(blobs, expand_grey=True)
    for n, (v, blob) in enumerate(zip(rgb, blobs)):
        assert np.array_equal(v.cpu().numpy(), np.asarray(Image.open(io.BytesIO(blob)).convert("RGB"))), NAMES[n]
    assert any(v.shape[2] == 1 for v in plain) and all(v.shape[2] == 3 for v in rgb)
    for n in (0, 3, len(blobs) - 1):                       # a batch result equals the single-image call
        one, st = ops.jpeg_decode([blobs[n]])
        assert st.item() == 0 and torch.equal(one[0], plain[n]), NAMES[n]


def test_imageio_front_end_and_refusals():
    from PIL import Image
    from ppst_amd import imageio
    arr = J.image_set()["photo41x77"]
    good = D.pillow_file(arr, 90, "4:2:0")
    out = imageio.decode_jpeg([good, D.pillow_file(J.image_set()["random96_grey"], 50, "4:4:4")], mode="RGB")
    assert np.array_equal(out[0].cpu().numpy(), _ref(good)) and out[1].shape == (96, 96, 3)
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, format="JPEG", progressive=True)
    with pytest.raises(ValueError, match="progressive"):
        imageio.decode_jpeg([good, buf.getvalue()])
    cut = _damaged(good)[0]
    with pytest.raises(OSError, match="damaged"):
        imageio.decode_jpeg([cut])


def _damaged(blob):
    """the scan cut in half (EOI put back); a byte flipped mid-scan -- the first position from the middle on at which the flip
    breaks the STRUCTURE of the scan as the host model sees it (an undefined code or a wrong block count: a flip that only changes
    a coefficient's value is a valid file with other pixels, which no decoder can tell)"""
    from ppst_amd import ops
    p = J.parse(blob)
    head, scan = len(p["head"]), p["scan"]
    mid = head + len(scan) // 2
    for at in range(mid, len(blob) - 2):
        flip = blob[:at] + bytes([blob[at] ^ 0x5A]) + blob[at + 1:]
        rc, d = ops.jpeg_parse(flip)
        if rc == 0 and D.model_decode(D.Desc(d), flip)[1] & (D.S_CODE | D.S_BLOCKS):
            return blob[:mid] + b"\xff\xd9", flip
    raise AssertionError("no structural flip found")


def test_damaged_files_do_not_touch_their_neighbours():
    """Three damaged files -- the scan cut in half, a byte flipped mid-scan, a wrong RSTm number -- in a batch with good ones: the
    damaged ones report a status, the good ones are exact, and a clean call afterwards is exact."""
    from ppst_amd import ops
    arr = J.image_set()["200x232"]
    base = D.pillow_file(arr, 90, "4:2:0")
    cut, flip = _damaged(D.pillow_file(J.image_set()["photo41x77"], 90, "4:2:0"))
    assert ops.jpeg_parse(cut)[0] == 0 and ops.jpeg_parse(flip)[0] == 0
    own = J.model_encode(arr, 90, "4:2:0")
    at = own.index(b"\xff\xd2", len(J.parse(own)["head"]))
    wrong_rst = own[:at] + b"\xff\xd5" + own[at + 2:]
    good = [base, own, D.pillow_file(J.image_set()["photo96x136"], 50, "4:4:4")]
    batch = [good[0], cut, good[1], flip, wrong_rst, good[2]]
    views, status = ops.jpeg_decode(batch)
    status = status.cpu().tolist()
    print("status", status)
    assert [bool(s) for s in status] == [False, True, False, True, True, False]
    assert status[4] & 4                                    # PPST_JPEG_S_RST_ORDER
    for n in (0, 2, 5):
        assert np.array_equal(views[n].cpu().numpy(), _ref(batch[n])), n
    _check_batch(good, "clean call after the damaged batch")


# ----------------------------------------------------------------------------------------------------------------- front ends
def _folder(root):
    """content/ and style/ with a 4:2:0 .jpg, a grey .jpg, a progressive .jpg (host fallback) and a .png, all 300 x 300"""
    from PIL import Image
    from ppst_amd import weights as W
    (root / "content").mkdir(parents=True)
    (root / "style").mkdir()
    base = W.synthetic_images(31, 4, size=256)
    u8 = ((base.clamp(-1, 1) + 1) * 127.5).to(torch.uint8).permute(0, 2, 3, 1).numpy()
    ims = [Image.fromarray(a).resize((300, 300), Image.BICUBIC) for a in u8]
    ims[0].save(str(root / "content" / "a.jpg"), quality=90, subsampling=2)
    ims[1].convert("L").save(str(root / "content" / "b.jpg"), quality=75)
    ims[2].save(str(root / "style" / "c.jpg"), quality=90, progressive=True)
    ims[3].save(str(root / "style" / "d.png"))
    return [str(root / "content" / "a.jpg"), str(root / "content" / "b.jpg"), str(root / "style" / "c.jpg"), str(root / "style" / "d.png")]


def test_load_images_device_equals_host(tmp_path):
    from ppst_amd import evaluation as EV
    paths = _folder(tmp_path / "in")
    host = EV.load_images(paths, 256, _dev())
    devd = EV.load_images(paths, 256, _dev(), decode="device")
    assert len(host) == len(devd) == 4
    for p, a, b in zip(paths, host, devd):
        assert a.shape == b.shape and torch.equal(a, b), p
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=2) as pool:
        pooled = EV.load_images(paths, 256, _dev(), pool, "device")
    assert all(torch.equal(a, b) for a, b in zip(host, pooled))


def test_swap_files_identical_with_either_decoder(tmp_path):
    """(at 512^2, the evaluator's size: the correspondence lives on the 64 x 64 code grid of a 512^2 image, a 256^2 swap is refused
    by the model with either decoder)"""
    from ppst_amd import evaluation as EV, weights as W
    from ppst_amd.ppst_model import create_model
    paths = _folder(tmp_path / "in")
    sd = W.make_state_dict(3, with_D=False, with_nce=False, bias_std=0.1, noise_weight=0.0)
    model = create_model(state_dict=sd, device=_dev())
    with torch.no_grad():
        ph = EV.evaluate_swap_files(model, paths[0], paths[1], str(tmp_path / "host"))
        with EV.decoder("device"):
            pd = EV.evaluate_swap_files(model, paths[0], paths[1], str(tmp_path / "device"))
    assert [os.path.basename(p) for p in ph] == [os.path.basename(p) for p in pd] and len(ph) == 1
    for a, b in zip(ph, pd):
        assert open(a, "rb").read() == open(b, "rb").read(), a


def test_dataset_device_decode_yields_the_host_batches(tmp_path):
    from PIL import Image
    from ppst_amd import weights as W
    from ppst_amd.training import CelebAMaskDataset
    root = tmp_path / "data"
    (root / "images").mkdir(parents=True)
    (root / "labels").mkdir()
    base = W.synthetic_images(41, 5, size=128)
    u8 = ((base.clamp(-1, 1) + 1) * 127.5).to(torch.uint8).permute(0, 2, 3, 1).numpy()
    rng = np.random.default_rng(3)
    for n, a in enumerate(u8):
        kw = dict(progressive=True) if n == 3 else {}
        Image.fromarray(a).save(str(root / "images" / ("%d.jpg" % n)), quality=90, **kw)
        Image.fromarray(rng.integers(0, 3, (128, 128), dtype=np.uint8)).save(str(root / "labels" / ("%d.png" % n)))
    flipped = 0
    for prefetch in (False, True):
        a = CelebAMaskDataset(str(root), size=64, batch_size=2, device=_dev(), seed=5, prefetch=prefetch)
        b = CelebAMaskDataset(str(root), size=64, batch_size=2, device=_dev(), seed=5, prefetch=prefetch, decode="device")
        for _ in range(4):
            x, y = next(a), next(b)
            assert torch.equal(x["real_A"], y["real_A"]) and torch.equal(x["mask_A"], y["mask_A"])
    probe = CelebAMaskDataset(str(root), size=64, batch_size=2, device=_dev(), seed=5, prefetch=False, decode="device")
    for _ in range(4):
        flipped += sum(1 for img, _ in probe._decode_batch() if isinstance(img, tuple) and img[1])
    assert flipped > 0                                      # the seed draws flips: `mirror` was exercised
