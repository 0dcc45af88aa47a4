"""GPU: the PNG decoder (csrc/png_decode.hip, ops.png_decode, imageio.decode_png, the ``decode="device"`` front ends).
The judge is Pillow on the same bytes, for EQUALITY -- never the decoder under test."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_decode_cases as P  # noqa: E402

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", 0)


@functools.lru_cache(None)
def _ref(blob, mode=None):
    return P.pillow_pixels(blob, mode)


def _check_batch(blobs, what, mode=None, **kw):
    """one batched call over `blobs`: every status 0, every image equal to Pillow's reading of the same bytes"""
    from ppst_amd import ops
    views, status, rounds = ops.png_decode(list(blobs), rounds=True, **kw)
    status, rounds = status.cpu().tolist(), rounds.cpu().tolist()
    print("%s: rounds %s" % (what, rounds))
    assert status == [0] * len(blobs), (what, status)
    for n, (v, blob) in enumerate(zip(views, blobs)):
        ref = _ref(blob, mode)
        got = v.cpu().numpy()
        assert got.shape == ref.shape, (what, n, got.shape, ref.shape)
        assert np.array_equal(got, ref), (what, n, int((got != ref).sum()))
    return views


@pytest.mark.parametrize("subseq_words", [0, 2, 4, 8])
@pytest.mark.parametrize("family", P.all_families())
def test_whole_set_decodes_to_pillows_pixels(family, subseq_words):
    """The whole image set -- 1 x 1 to 600 x 530, grey, RGB and RGBA, the band edges of the unfilter, the constant image, the
    far-match file -- in ONE batched call per family (every row filter forced, the zlib levels and strategies, the IDAT cuts,
    Pillow's own files), at the default subsequence length (128 bits) and at 64, 128 and 256 bits stated."""
    names, blobs = P.family_files(family)
    _check_batch(blobs, "%s sw %d" % (family, subseq_words), subseq_words=subseq_words)


@pytest.mark.parametrize("subseq_words", [0, 2])
def test_rounds_equal_the_models(subseq_words):
    """the rounds the device reports per file (the largest over its windows) are the host model's: the two walk alike"""
    from ppst_amd import ops
    names, blobs = P.family_files("mixed")
    pick = [names.index(n) for n in ("17x3", "41x77", "65x5", "labels128", "checker1", "160x136")]
    _, status, rounds = ops.png_decode([blobs[k] for k in pick], subseq_words=subseq_words, rounds=True)
    assert status.cpu().tolist() == [0] * len(pick)
    want = []
    for k in pick:
        rc, d, spans = P.parse(blobs[k])
        want.append(P.model_decode(blobs[k], d, spans, words=subseq_words).rounds)
    assert rounds.cpu().tolist() == want


def test_mode_rgb_mirror_and_batch_independence():
    from ppst_amd import imageio, ops
    names, blobs = P.family_files("pillow")
    blobs = list(blobs)
    assert {P.image_set()[n].shape[2] for n in names} == {1, 3, 4}
    rgb = imageio.decode_png(blobs, mode="RGB")
    for n, (v, blob) in enumerate(zip(rgb, blobs)):
        assert v.shape[2] == 3 and np.array_equal(v.cpu().numpy(), _ref(blob, "RGB")), names[n]
    plain = imageio.decode_png(blobs)
    assert sorted({v.shape[2] for v in plain}) == [1, 3, 4]
    flags = [n % 2 == 0 for n in range(len(blobs))]
    mirrored, status = ops.png_decode(blobs, mirror=flags)
    assert status.cpu().tolist() == [0] * len(blobs)
    for n, (a, b) in enumerate(zip(plain, mirrored)):
        want = a.cpu().numpy()[:, ::-1] if flags[n] else a.cpu().numpy()
        assert np.array_equal(b.cpu().numpy(), want), names[n]
    for n in (0, 3, names.index("41x77_rgba"), len(blobs) - 1):          # a batch result equals the single-image call
        one, st = ops.png_decode([blobs[n]])
        assert st.item() == 0 and torch.equal(one[0], plain[n]), names[n]


def test_own_files_come_back():
    """imageio.encode_png -> decode_png gives back the input tensor (the device encoder's layout: one IDAT chunk per 32 KB piece,
    a dynamic block of literals closed by an empty stored block, or a stored block; the Adler-32 in a chunk of its own)"""
    from ppst_amd import imageio
    for name in ("1x1", "1x1_grey", "17x3", "64x700_grey", "200x232", "const512", "field512"):
        arr = P.image_set()[name]
        x = torch.from_numpy(arr[None].copy()).to(_dev())
        blob = imageio.encode_png(x)[0]
        back = imageio.decode_png([blob])[0]
        assert torch.equal(back, x[0]), name
        assert np.array_equal(_ref(blob), arr), name


def test_front_end_refusals():
    import io
    from PIL import Image
    from ppst_amd import imageio
    good = P.make_png(P.image_set()["photo41x77"])
    buf = io.BytesIO()
    Image.fromarray(P.image_set()["photo41x77"]).convert("P").save(buf, format="PNG")
    with pytest.raises(ValueError, match="palette"):
        imageio.decode_png([good, buf.getvalue()])
    with pytest.raises(OSError, match="damaged.*Adler-32"):
        imageio.decode_png([good, P.damaged_files(good)[1]])


def test_damaged_files_do_not_touch_their_neighbours():
    """Three damaged files -- a bad chunk CRC, a bad Adler-32 behind a good CRC, a stream cut in half behind a good CRC -- in a
    batch with good ones: the damaged ones report a status, the good ones are exact, and a clean call afterwards is exact."""
    from ppst_amd import ops
    names, blobs = P.family_files("mixed")
    pick = lambda n: blobs[names.index(n)]
    bad_crc, bad_adler, cut = P.damaged_files(pick("photo41x77"))
    good = [pick("200x232"), pick("64x700_grey"), pick("41x77_rgba")]
    batch = [good[0], bad_crc, good[1], bad_adler, cut, good[2]]
    views, status = ops.png_decode(batch)
    status = status.cpu().tolist()
    print("status", status)
    assert [bool(s) for s in status] == [False, True, False, True, True, False]
    assert status[1] & P.S_CRC and status[3] == P.S_ADLER and status[4] & P.S_STREAM
    for n in (0, 2, 5):
        assert np.array_equal(views[n].cpu().numpy(), _ref(batch[n])), n
    _check_batch(good, "clean call after the damaged batch")


# ----------------------------------------------------------------------------------------------------------------- front ends
def _folder(root):
    """content/ and style/ with an RGB .png, a grey .png, an RGBA .png, a palette .png (host fallback) and a .jpg, all 520 x 520"""
    from PIL import Image
    from ppst_amd import weights as W
    (root / "content").mkdir(parents=True)
    (root / "style").mkdir()
    base = W.synthetic_images(31, 5, size=256)
    u8 = ((base.clamp(-1, 1) + 1) * 127.5).to(torch.uint8).permute(0, 2, 3, 1).numpy()
    ims = [Image.fromarray(a).resize((520, 520), Image.BICUBIC) for a in u8]
    ims[0].save(str(root / "content" / "a.png"))
    ims[1].convert("L").save(str(root / "content" / "b.png"))
    ims[2].convert("RGBA").save(str(root / "style" / "c.png"))
    ims[3].convert("P").save(str(root / "style" / "d.png"))
    ims[4].save(str(root / "style" / "e.jpg"), quality=90)
    return [str(root / "content" / "a.png"), str(root / "content" / "b.png"), str(root / "style" / "c.png"), str(root / "style" / "d.png"),
            str(root / "style" / "e.jpg")]


def test_load_images_and_swap_files_identical_with_either_decoder(tmp_path):
    """load_images and evaluate_swap_files at 512^2 on PNG inputs: bit-identical inside ``decoder("device")``"""
    from ppst_amd import evaluation as EV, weights as W
    from ppst_amd.ppst_model import create_model
    paths = _folder(tmp_path / "in")
    host = EV.load_images(paths, 512, _dev())
    with EV.decoder("device"):
        devd = EV.load_images(paths, 512, _dev())
    assert len(host) == len(devd) == 5
    for p, a, b in zip(paths, host, devd):
        assert a.shape == b.shape and torch.equal(a, b), p
    took = EV.decode_files_device([open(p, "rb").read() for p in paths], paths, _dev())
    assert [v is not None for v in took] == [True, True, True, False, True]          # the palette file is the host's
    sd = W.make_state_dict(3, with_D=False, with_nce=False, bias_std=0.1, noise_weight=0.0)
    model = create_model(state_dict=sd, device=_dev())
    with torch.no_grad():
        ph = EV.evaluate_swap_files(model, paths[0], paths[2], str(tmp_path / "host"))
        with EV.decoder("device"):
            pd = EV.evaluate_swap_files(model, paths[0], paths[2], str(tmp_path / "device"))
    assert [os.path.basename(p) for p in ph] == [os.path.basename(p) for p in pd] and len(ph) == 1
    for a, b in zip(ph, pd):
        assert open(a, "rb").read() == open(b, "rb").read(), a


def test_dataset_device_decode_yields_the_host_batches(tmp_path):
    """PNG images and 128^2 grey label files: images and labels decoded on the device (the flip as ``mirror``), one label of
    another size and one RGB label through Pillow -- the batches of ``decode="host"`` for the same seed"""
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
        im = Image.fromarray(a)
        (im.convert("P") if n == 3 else im).save(str(root / "images" / ("%d.png" % n)))
        lab = np.kron(rng.integers(0, 3, (8, 8), dtype=np.uint8), np.ones((16, 16), np.uint8))
        if n == 1:
            lab = lab[:64, :64]                                                      # another size: resized NEAREST on the host
        lab = Image.fromarray(lab)
        (lab.convert("RGB") if n == 2 else lab).save(str(root / "labels" / ("%d.png" % n)))
    for prefetch in (False, True):
        a = CelebAMaskDataset(str(root), size=128, batch_size=2, device=_dev(), seed=5, prefetch=prefetch)
        b = CelebAMaskDataset(str(root), size=128, batch_size=2, device=_dev(), seed=5, prefetch=prefetch, decode="device")
        for _ in range(4):
            x, y = next(a), next(b)
            assert torch.equal(x["real_A"], y["real_A"]) and torch.equal(x["mask_A"], y["mask_A"])
    probe = CelebAMaskDataset(str(root), size=128, batch_size=2, device=_dev(), seed=5, prefetch=False, decode="device")
    flipped = img_dev = lab_dev = lab_host = 0
    for _ in range(4):
        for img, lab in probe._decode_batch():
            img_dev += isinstance(img, tuple)
            lab_dev += isinstance(lab, tuple)
            lab_host += not isinstance(lab, tuple)
            flipped += bool(isinstance(lab, tuple) and lab[1])
    assert flipped > 0 and img_dev > 0 and lab_dev > 0 and lab_host > 0          # the seed draws flips; both label paths ran
