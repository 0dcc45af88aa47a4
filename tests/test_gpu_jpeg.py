"""GPU: the JPEG encoder (csrc/jpeg.hip, ops.jpeg_encode, imageio.encode_jpeg, the ``format="jpeg"`` front ends).
The judges are Pillow's decoder (libjpeg-turbo) and the host model of tests/jpeg_cases.py -- never the encoder itself."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_cases as J  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = sorted(J.image_set())
SETTINGS = [(q, ss) for q in J.QUALITIES for ss in J.SUBSAMPLINGS]


def _dev():
    return torch.device("cuda", 0)


def _encode(arrs, quality, subsampling):
    from ppst_amd import imageio
    return imageio.encode_jpeg(torch.from_numpy(np.stack(arrs)).to(_dev()), quality, subsampling)


@functools.lru_cache(None)
def _files(name):
    """{(quality, subsampling): the device's file} of one image of the set, encoded once for all tests."""
    arr = J.image_set()[name]
    return {(q, ss): _encode([arr], q, ss)[0] for q, ss in SETTINGS}


@functools.lru_cache(None)
def _decoded(name):
    return {key: J.entropy_decode(blob) for key, blob in _files(name).items()}


def _lib_header(H, W, C, quality, subsampling):
    from ppst_amd._lib import lib
    n = lib.ppst_jpeg_header(H, W, C, quality, J.SS_NUMBER[subsampling], None, 0)
    buf = ctypes.create_string_buffer(n)
    assert lib.ppst_jpeg_header(H, W, C, quality, J.SS_NUMBER[subsampling], buf, n) == n
    return buf.raw


@pytest.mark.parametrize("name", NAMES)
def test_valid_file(name):
    """Pillow opens and fully loads every file, with the right mode and size; the file is within ppst_jpeg_bound, starts with
    ppst_jpeg_header's bytes and ends with EOI; a grey image gives the same file whatever the subsampling."""
    from ppst_amd._lib import lib
    arr = J.image_set()[name]
    H, W, C = arr.shape
    for (q, ss), blob in _files(name).items():
        mode, size, dec = J.pillow_decode(blob)
        assert mode == ("RGB" if C == 3 else "L") and size == (W, H), (name, q, ss)
        assert len(blob) <= lib.ppst_jpeg_bound(H, W, C, J.SS_NUMBER[ss]), (name, q, ss)
        head = _lib_header(H, W, C, q, ss)
        assert blob[:len(head)] == head and blob[-2:] == b"\xff\xd9", (name, q, ss)
        print("%-14s q %3d %s %7d bytes, PSNR %.2f dB" % (name, q, ss, len(blob), J.psnr(dec, arr)))
    if C == 1:
        for q in J.QUALITIES:
            assert _files(name)[(q, "4:4:4")] == _files(name)[(q, "4:2:0")]


@pytest.mark.parametrize("name", NAMES)
def test_coefficients_are_the_nearest_to_the_float64_dct(name):
    """Entropy-decode the device's file with the host decoder: every coefficient q of every block satisfies
    |q Q - c64| <= Q / 2 + EPS, c64 the float64 DCT of the integer samples the format defines, EPS twice the error of the
    kernels' fixed-point DCT as measured on the CPU (jpeg_cases.EPS).  No coefficient is excluded."""
    arr = J.image_set()[name]
    worst = 0.0
    for (q, ss), (coefs, p) in _decoded(name).items():
        blocks, comps = J.scan_blocks(arr, ss)
        assert coefs.shape == (len(blocks), 64), (name, q, ss)
        Q = J.block_q(comps, q)[:, J.ZIGZAG].astype(np.float64)
        c64 = J.dct_f64(blocks).reshape(-1, 64)[:, J.ZIGZAG]
        over = np.abs(coefs * Q - c64) - Q / 2
        worst = max(worst, over.max())
        assert over.max() <= J.EPS, "%s q %d %s: block %d coefficient %d is %.4f beyond Q / 2" % (
            (name, q, ss) + tuple(int(i) for i in np.unravel_index(over.argmax(), over.shape)) + (over.max(),))
    print("%-14s largest |q Q - c64| - Q / 2 = %.4f (EPS %.4f)" % (name, worst, J.EPS))


@pytest.mark.parametrize("name", NAMES)
def test_entropy_coding_is_canonical(name):
    """The decoded coefficients, coded again by the host entropy encoder at the file's own DRI, give the device's scan byte for
    byte: codes, stuffing, pad bits and RST order.  DRI is the 96-block interval, and no interval passes its worst case."""
    arr = J.image_set()[name]
    H, W, C = arr.shape
    for (q, ss), (coefs, p) in _decoded(name).items():
        assert p["dri"] == J.dri_mcus(C, ss), (name, q, ss)
        assert p["order"] == [0xD8, 0xE0] + [0xDB] * (1 if C == 1 else 2) + [0xC0] + [0xC4] * (2 if C == 1 else 4) + [0xDD, 0xDA]
        again = J.entropy_encode(coefs, C, ss, p["dri"])
        assert again == p["scan"], "%s q %d %s: scans differ (device %d bytes, host %d)" % (name, q, ss, len(p["scan"]), len(again))
        assert len(_files(name)[(q, ss)]) <= J.worst_case_bytes(H, W, C, ss)


def _photo_set():
    s = {n: J.image_set()[n] for n in J.PHOTO}
    s["synthetic256"] = J.synthetic256()
    return s


@functools.lru_cache(None)
def _against_pillow():
    """[(name, quality, subsampling, device bytes, Pillow bytes, device PSNR, Pillow PSNR, PSNR of the two decodes against
    each other)] over the photo-like set."""
    rows = []
    for name, arr in _photo_set().items():
        for q in (50, 90, 100):
            for ss in J.SUBSAMPLINGS:
                d, = _encode([arr], q, ss)
                p = J.pillow_encode(arr, q, ss)
                dd, pd = J.pillow_decode(d)[2], J.pillow_decode(p)[2]
                rows.append((name, q, ss, len(d), len(p), J.psnr(dd, arr), J.psnr(pd, arr), J.psnr(dd, pd)))
    return rows


def test_quality_and_size_against_pillow():
    """Photo-like images at q 50 / 90 / 100, both subsamplings: Pillow's decode of the device's file is within 0.1 dB of (or
    above) Pillow's own encode at the same settings, and per group of images the files total at most 1.05 x Pillow's."""
    rows = _against_pillow()
    for name, q, ss, nd, npil, pd, pp, pair in rows:
        print("%-13s q %3d %s device %7d  Pillow %7d  ratio %.4f  PSNR %.3f vs %.3f (%+.3f dB)  device vs Pillow decode %.2f dB"
              % (name, q, ss, nd, npil, nd / npil, pd, pp, pd - pp, pair))
    groups = {"field": J.PHOTO, "synthetic": ("synthetic256",)}
    for g, names in groups.items():
        nd, npil = sum(r[3] for r in rows if r[0] in names), sum(r[4] for r in rows if r[0] in names)
        print("group %-10s device %8d  Pillow %8d  ratio %.4f" % (g, nd, npil, nd / npil))
    for name, q, ss, nd, npil, pd, pp, pair in rows:
        assert pd >= pp - 0.1, (name, q, ss, pd, pp)
    for g, names in groups.items():
        assert sum(r[3] for r in rows if r[0] in names) <= 1.05 * sum(r[4] for r in rows if r[0] in names), g


def test_batches_streams_and_repeatability():
    """A batch of eight different images gives the eight files of eight single-image calls, also on a non-default stream;
    two runs are byte-identical; the empty batch gives []."""
    from ppst_amd import imageio, ops, weights as W
    dev = _dev()
    x = W.synthetic_images(33, 8, size=256)
    u8 = ((x.clamp(-1, 1) + 1) * 127.5).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    u8[5] = torch.from_numpy(J.field(9, 256, 256, 1.3, noise=1.0))
    u8[6] = 7
    u8[7] = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (256, 256, 3), dtype=np.uint8))
    g = u8.to(dev)
    for q, ss in ((90, "4:2:0"), (100, "4:4:4")):
        batch = imageio.encode_jpeg(g, q, ss)
        assert len(batch) == 8 and len(set(batch)) == 8
        for i in range(8):
            mode, size, _ = J.pillow_decode(batch[i])
            assert mode == "RGB" and size == (256, 256)
            assert imageio.encode_jpeg(g[i:i + 1], q, ss) == [batch[i]], i
        assert imageio.encode_jpeg(g, q, ss) == batch
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            files, sizes = ops.jpeg_encode(g, q, ss)
        side.synchronize()
        n = sizes.cpu().tolist()
        assert [files[i, :n[i]].cpu().numpy().tobytes() for i in range(8)] == batch
    assert imageio.encode_jpeg(g[:0]) == []


def test_slots_and_files_beyond_two_gigabytes():
    """Eight 4096^2 images at 4:4:4: 65 536 interval slots of 39 840 bytes and eight worst-case file slots are 2.61 GB each, so
    the last image's slot and file offsets pass 2^31.  The last image's file is the file of a call on that image alone, and
    Pillow decodes it to the picture."""
    from ppst_amd import imageio
    from ppst_amd._lib import lib
    dev = _dev()
    B, S = 8, 4096
    assert (B - 1) * lib.ppst_jpeg_bound(S, S, 3, 0) > 2 ** 31 and lib.ppst_jpeg_ws(B, S, S, 3, 0) > 2 ** 31 + lib.ppst_jpeg_ws(1, S, S, 3, 0)
    y, x = torch.meshgrid(torch.arange(S, device=dev), torch.arange(S, device=dev), indexing="ij")
    planes = torch.stack(((x + y) // 16, (x * 3 + y) // 32, (x + 5 * y) // 64), dim=2)              # (S, S, 3) smooth ramps
    g = torch.stack([((planes + 37 * i) & 255).to(torch.uint8) for i in range(B)])
    batch = imageio.encode_jpeg(g, 90, "4:4:4")
    assert len(set(batch)) == B
    assert imageio.encode_jpeg(g[B - 1:], 90, "4:4:4") == [batch[B - 1]]
    mode, size, dec = J.pillow_decode(batch[B - 1])
    assert mode == "RGB" and size == (S, S) and J.psnr(dec, g[B - 1].cpu().numpy()) > 30.0


def test_front_ends_write_jpeg_files_with_either_encoder(tmp_path):
    """evaluate_grid_folder(format="jpeg", png="device") on a 2 x 2 folder of 512^2 inputs: the names of the host JPEG run (.jpg),
    every file decodes and is as close to the host run's decoded file as the two encoders are on the photo-like set at that
    quality (both encode the same uint8 batch); evaluate_swap_files likewise; the default call still writes PNG files."""
    from PIL import Image
    from ppst_amd import evaluation as EV, weights as W
    from ppst_amd.ppst_model import create_model
    dev = _dev()
    floor = min(r[7] for r in _against_pillow() if r[1] == 90 and r[2] == "4:2:0")
    print("device vs Pillow decode at q 90 4:2:0 on the photo-like set: at least %.2f dB" % floor)
    root = tmp_path / "data"
    (root / "content").mkdir(parents=True); (root / "style").mkdir()
    base = W.synthetic_images(21, 4, size=512)
    u8 = ((base.clamp(-1, 1) + 1) * 127.5).to(torch.uint8).permute(0, 2, 3, 1).numpy()
    names = [("content", "c0.png"), ("content", "c1.jpg"), ("style", "s0.png"), ("style", "s1.png")]
    for (sub, fn), a in zip(names, u8):
        Image.fromarray(a).resize((600, 600), Image.BICUBIC).save(str(root / sub / fn))
    sd = W.make_state_dict(3, with_D=False, with_nce=False, bias_std=0.1, noise_weight=0.0)
    model = create_model(state_dict=sd, device=dev)

    def same_pictures(host_path, dev_path):
        a, b = np.asarray(Image.open(host_path)), np.asarray(Image.open(dev_path))
        assert a.shape == b.shape == (512, 512, 3)
        v = J.psnr(a, b)
        print("%-18s device vs host decode %.2f dB" % (os.path.basename(dev_path), v))
        assert v >= floor, (dev_path, v, floor)

    with torch.no_grad():
        host = EV.evaluate_grid_folder(model, str(root), str(tmp_path / "host"), load_size=512, workers=4, format="jpeg")
        devw = EV.evaluate_grid_folder(model, str(root), str(tmp_path / "device"), load_size=512, workers=4, png="device", format="jpeg")
        plain = EV.evaluate_grid_folder(model, str(root), str(tmp_path / "plain"), load_size=512, workers=4)
    hf, df = sorted(os.listdir(str(tmp_path / "host" / "images"))), sorted(os.listdir(str(tmp_path / "device" / "images")))
    assert hf == df == sorted(["c0.jpg", "c1.jpg", "s0.jpg", "s1.jpg", "c0_s0.jpg", "c0_s1.jpg", "c1_s0.jpg", "c1_s1.jpg"])
    assert sorted(os.path.basename(p) for p in devw) == df and len(host) == 8
    for fn in df:
        assert Image.open(str(tmp_path / "device" / "images" / fn)).format == "JPEG"
        same_pictures(str(tmp_path / "host" / "images" / fn), str(tmp_path / "device" / "images" / fn))
    assert sorted(os.path.basename(p) for p in plain) == [f[:-4] + ".png" for f in df]
    for p in plain:
        im = Image.open(p)
        assert im.format == "PNG"
        jp = np.asarray(Image.open(str(tmp_path / "host" / "images" / (os.path.basename(p)[:-4] + ".jpg"))))
        assert J.psnr(np.asarray(im), jp) > 25.0          # the same picture, before and after a q 90 JPEG
    cp, sp_ = str(root / "content" / "c0.png"), str(root / "style" / "s1.png")
    with torch.no_grad():
        ph = EV.evaluate_swap_files(model, cp, sp_, str(tmp_path / "swap_host"), alphas=(0.5, 1.0), format="jpeg")
        pd = EV.evaluate_swap_files(model, cp, sp_, str(tmp_path / "swap_device"), alphas=(0.5, 1.0), png="device", format="jpeg")
        pp = EV.evaluate_swap_files(model, cp, sp_, str(tmp_path / "swap_plain"), alphas=(0.5, 1.0))
    assert [os.path.basename(p) for p in pd] == [os.path.basename(p) for p in ph] == ["c0_s1_0.50.jpg", "c0_s1_1.00.jpg"]
    assert [os.path.basename(p) for p in pp] == ["c0_s1_0.50.png", "c0_s1_1.00.png"]
    for a, b in zip(ph, pd):
        same_pictures(a, b)
