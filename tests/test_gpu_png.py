"""GPU: the PNG encoder (csrc/png.hip, ops.png_encode, imageio.encode_png, the ``png="device"`` front ends).
The judges are the decoders -- Pillow (libpng) and Python's zlib -- never the encoder itself."""
import io
import os
import struct
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------ image set
def _synthetic(size, seed=21):
    from ppst_amd import weights as W
    x = W.synthetic_images(seed, 1, size=size)
    return ((x.clamp(-1, 1) + 1) * 127.5).to(torch.uint8).permute(0, 2, 3, 1).numpy()[0]


def _smooth(seed, H, W, C, alpha, noise, border=0):
    """A seeded random field with a 1 / f^alpha amplitude spectrum around mid-grey plus ``noise`` LSB of white noise:
    photo-like content; ``border`` > 0 frames it with flat 0 (top / left) and 255 (bottom / right) bands."""
    rng = np.random.default_rng([seed, 11])
    fy, fx = np.fft.fftfreq(H)[:, None], np.fft.fftfreq(W)[None, :]
    f = np.sqrt(fy * fy + fx * fx)
    f[0, 0] = 1.0
    out = np.empty((H, W, C), dtype=np.uint8)
    for c in range(C):
        spec = np.fft.fft2(rng.standard_normal((H, W))) / f ** alpha
        spec[0, 0] = 0.0
        field = np.real(np.fft.ifft2(spec))
        field = field / field.std()
        v = 128.0 + 48.0 * field + noise * rng.standard_normal((H, W))
        out[:, :, c] = np.clip(np.rint(v), 0, 255).astype(np.uint8)
    if border:
        out[:border] = 0; out[:, :border] = 0
        out[-border:] = 255; out[:, -border:] = 255
    return out


def _image_set():
    """name -> (group, HWC uint8).  Groups: synthetic / smooth (held against Pillow's size), constant, random, tiny."""
    rng = np.random.default_rng(5)
    s = {}
    for size in (256, 512, 1024):
        s["synthetic%d" % size] = ("synthetic", _synthetic(size))
    s["smooth512"] = ("smooth", _smooth(1, 512, 512, 3, 1.2, 1.0))
    s["smooth600x530"] = ("smooth", _smooth(2, 600, 530, 3, 1.4, 0.3))
    s["smooth_border"] = ("smooth", _smooth(3, 512, 512, 3, 1.1, 4.0, border=48))
    s["smooth200x131_grey"] = ("smooth", _smooth(4, 200, 131, 1, 1.3, 1.0))
    s["zeros"] = ("constant", np.zeros((300, 200, 3), np.uint8))
    s["ones"] = ("constant", np.full((256, 256, 3), 255, np.uint8))
    s["ones_grey"] = ("constant", np.full((64, 700, 1), 255, np.uint8))
    s["random"] = ("random", rng.integers(0, 256, (256, 256, 3), dtype=np.uint8))
    s["1x1"] = ("tiny", rng.integers(0, 256, (1, 1, 3), dtype=np.uint8))
    s["1x1_grey"] = ("tiny", rng.integers(0, 256, (1, 1, 1), dtype=np.uint8))
    s["1xW"] = ("tiny", rng.integers(0, 256, (1, 333, 3), dtype=np.uint8))
    s["Hx1"] = ("tiny", rng.integers(0, 256, (421, 1, 3), dtype=np.uint8))
    s["17x3"] = ("tiny", rng.integers(0, 256, (17, 3, 3), dtype=np.uint8))
    return s


def _all_stored_size(H, W, C):
    n = H * (1 + W * C)
    return 8 + 25 + 12 + 2 + n + 5 * -(-n // 65535) + 4 + 12


def _encode(arrs, dev):
    from ppst_amd import imageio
    return imageio.encode_png(torch.from_numpy(np.stack(arrs)).to(dev))


def _chunks(blob):
    """[(type, data)] of a PNG file; every chunk's CRC-32 is checked here, with zlib's."""
    assert blob[:8] == b"\x89PNG\r\n\x1a\n"
    out, at = [], 8
    while at < len(blob):
        n, typ = struct.unpack(">I4s", blob[at:at + 8])
        data = blob[at + 8:at + 8 + n]
        assert len(data) == n, "chunk %r runs past the end of the file" % typ
        crc, = struct.unpack(">I", blob[at + 8 + n:at + 12 + n])
        assert crc == zlib.crc32(typ + data), "CRC of chunk %r at byte %d" % (typ, at)
        out.append((typ, data))
        at += 12 + n
    assert at == len(blob)
    return out


def _check_file(blob, arr):
    from PIL import Image
    H, W, C = arr.shape
    im = Image.open(io.BytesIO(blob))
    assert im.mode == ("RGB" if C == 3 else "L") and im.size == (W, H)
    got = np.asarray(im)
    assert np.array_equal(got.reshape(H, W, C), arr), "pixels differ after the round trip"
    ch = _chunks(blob)
    types = [t for t, _ in ch]
    assert types[0] == b"IHDR" and types[-1] == b"IEND" and set(types[1:-1]) == {b"IDAT"}
    assert ch[0][1] == struct.pack(">IIBBBBB", W, H, 8, 2 if C == 3 else 0, 0, 0, 0)
    idat = b"".join(d for t, d in ch if t == b"IDAT")
    raw = zlib.decompress(idat)                              # (checks the Adler-32)
    assert len(raw) == H * (1 + W * C)
    rows = np.frombuffer(raw, np.uint8).reshape(H, 1 + W * C)
    assert rows[:, 0].max() <= 4
    return idat, raw


# ------------------------------------------------------------------------------------------------------------------ tests
def test_round_trip_valid_stream_bound_and_size():
    """Every image of the set: exact round trip through Pillow, chunk CRCs, a zlib stream of exactly H (1 + W C) bytes with
    filter bytes 0..4, the file within ppst_png_bound; random bytes fall back to stored blocks; and per group of photo-like
    images the files are at most 1.05 x Pillow's (default ``save``) in total."""
    from PIL import Image
    from ppst_amd._lib import lib
    dev = torch.device("cuda", 0)
    images = _image_set()
    dev_bytes, pil_bytes, quality = {}, {}, []
    for name, (group, arr) in images.items():
        H, W, C = arr.shape
        blob, = _encode([arr], dev)
        assert len(blob) <= lib.ppst_png_bound(H, W, C), name
        idat, raw = _check_file(blob, arr)
        if group == "random":
            print("random bytes: %d file bytes, all-stored %d" % (len(blob), _all_stored_size(H, W, C)))
            assert len(blob) <= 1.002 * _all_stored_size(H, W, C)
        buf = io.BytesIO()
        Image.fromarray(arr[:, :, 0] if C == 1 else arr).save(buf, format="PNG")
        co = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_HUFFMAN_ONLY)
        honly = len(co.compress(raw) + co.flush())
        print("%-20s %4dx%-4dx%d device %8d  Pillow %8d  ratio %.4f   IDAT / zlib Z_HUFFMAN_ONLY %.4f"
              % (name, H, W, C, len(blob), buf.tell(), len(blob) / buf.tell(), len(idat) / honly))
        dev_bytes.setdefault(group, []).append(len(blob))
        pil_bytes.setdefault(group, []).append(buf.tell())
        quality.append(len(idat) / honly)
    for group in ("synthetic", "smooth"):
        d, p = sum(dev_bytes[group]), sum(pil_bytes[group])
        print("group %-10s device %9d  Pillow %9d  ratio %.4f" % (group, d, p, d / p))
    for group in ("synthetic", "smooth"):
        assert sum(dev_bytes[group]) <= 1.05 * sum(pil_bytes[group]), group


def test_batches_streams_and_repeatability():
    """A batch of eight different images gives the eight files of eight single-image calls, also on a non-default stream;
    two runs are byte-identical."""
    from ppst_amd import imageio, ops, weights as W
    dev = torch.device("cuda", 0)
    x = W.synthetic_images(33, 8, size=256)
    u8 = ((x.clamp(-1, 1) + 1) * 127.5).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    u8[5] = torch.from_numpy(_smooth(9, 256, 256, 3, 1.3, 1.0))
    u8[6] = 7
    u8[7] = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (256, 256, 3), dtype=np.uint8))
    g = u8.to(dev)
    batch = imageio.encode_png(g)
    assert len(batch) == 8 and len(set(batch)) == 8
    for i in range(8):
        _check_file(batch[i], u8[i].numpy())
        assert imageio.encode_png(g[i:i + 1]) == [batch[i]], i
    assert imageio.encode_png(g) == batch
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        files, sizes = ops.png_encode(g)
    side.synchronize()
    n = sizes.cpu().tolist()
    assert [files[i, :n[i]].cpu().numpy().tobytes() for i in range(8)] == batch
    assert imageio.encode_png(g[:0]) == []


def test_front_ends_write_the_same_pictures_with_the_device_encoder(tmp_path):
    """evaluate_grid_folder(png="device") on a 2 x 2 folder: the file names of the host run, and every file decodes to the
    pixels of the host run's file; evaluate_swap_files likewise."""
    from PIL import Image
    from ppst_amd import evaluation as EV, weights as W
    from ppst_amd.ppst_model import create_model
    dev = torch.device("cuda", 0)
    root = tmp_path / "data"
    (root / "content").mkdir(parents=True); (root / "style").mkdir()
    base = W.synthetic_images(21, 4, size=512)
    u8 = ((base.clamp(-1, 1) + 1) * 127.5).to(torch.uint8).permute(0, 2, 3, 1).numpy()
    names = [("content", "c0.png"), ("content", "c1.jpg"), ("style", "s0.png"), ("style", "s1.png")]
    for (sub, fn), a in zip(names, u8):
        Image.fromarray(a).resize((600, 600), Image.BICUBIC).save(str(root / sub / fn))
    sd = W.make_state_dict(3, with_D=False, with_nce=False, bias_std=0.1, noise_weight=0.0)
    model = create_model(state_dict=sd, device=dev)
    with torch.no_grad():
        host = EV.evaluate_grid_folder(model, str(root), str(tmp_path / "host"), load_size=512, workers=4)
        devw = EV.evaluate_grid_folder(model, str(root), str(tmp_path / "device"), load_size=512, workers=4, png="device")
    hf, df = sorted(os.listdir(str(tmp_path / "host" / "images"))), sorted(os.listdir(str(tmp_path / "device" / "images")))
    assert hf == df and len(df) == 8 and len(devw) == len(host) == 8
    assert sorted(os.path.basename(p) for p in devw) == df
    for fn in df:
        a = np.asarray(Image.open(str(tmp_path / "host" / "images" / fn)))
        blob = open(str(tmp_path / "device" / "images" / fn), "rb").read()
        _check_file(blob, a)
    cp, sp_ = str(root / "content" / "c0.png"), str(root / "style" / "s1.png")
    with torch.no_grad():
        ph = EV.evaluate_swap_files(model, cp, sp_, str(tmp_path / "swap_host"), alphas=(0.5, 1.0))
        pd = EV.evaluate_swap_files(model, cp, sp_, str(tmp_path / "swap_device"), alphas=(0.5, 1.0), png="device")
    assert [os.path.basename(p) for p in pd] == [os.path.basename(p) for p in ph] == ["c0_s1_0.50.png", "c0_s1_1.00.png"]
    for a, b in zip(ph, pd):
        _check_file(open(b, "rb").read(), np.asarray(Image.open(a)))
