"""Image preprocessing on the device.

Mirrors the evaluators' transform (data/base_dataset.py:85-171 ``get_transform`` with
``preprocess = scale_shortside``): PIL ``Image.resize(..., Image.BICUBIC)`` to the short side,
``__make_power_2`` to a multiple of 16, ``ToTensor`` and ``Normalize(0.5, 0.5)`` -- on uint8 HWC
tensors that are already in HBM (e.g. decoded by the host once, or the output of a previous swap).

Host logic here = sizes (Python ``round``: half to even, like the reference) and Pillow's
coefficient tables (Resample.c ``precompute_coeffs`` + ``normalize_coeffs_8bpc``: double-precision
bicubic weights, normalised, 22-bit fixed point); the pixel arithmetic is integer HIP kernels
(csrc/imageio.hip), bit-identical to Pillow.

The other end of the pipeline is here too: ``encode_png`` turns a uint8 batch on the device into PNG files (csrc/png.hip:
row filters, deflate and checksums as HIP kernels) and brings only the file bytes to the host; ``encode_jpeg`` does the same
for baseline JPEG files (csrc/jpeg.hip: colour conversion, integer DCT, Huffman coding and restart intervals as HIP kernels).
``decode_jpeg`` is the way in: baseline JPEG files of any origin -> uint8 tensors on the device, equal to Pillow's decode byte for
byte (csrc/jpeg_decode.hip: a parallel Huffman decoder for one sequential stream, integer IDCT, upsampling and colour).
``decode_png`` is the same for 8-bit grey / RGB / RGBA PNG files (csrc/png_decode.hip: chunk CRCs, a parallel inflate, LZ77
back-references by pointer jumping, the row filters undone).
"""
import math

import numpy as np
import torch

from . import ops
from ._lib import check, lib

PRECISION_BITS = 32 - 8 - 2
_TABLES = {}


def _bicubic(x):
    a = -0.5
    x = np.abs(x)
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1, np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * a, 0.0))


def bicubic_windows(in_size, out_size):
    """Pillow's precompute_coeffs for the bicubic filter, in float64: (ksize, bounds int32 [out][2] = (first, count),
    weights float64 [out][ksize], each row normalised to sum 1 and zero behind its count)."""
    support = 2.0
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    sup = support * filterscale
    ksize = int(math.ceil(sup)) * 2 + 1
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    weights = np.zeros((out_size, ksize), dtype=np.float64)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - sup + 0.5), 0)
        xmax = min(int(center + sup + 0.5), in_size) - xmin
        k = _bicubic((np.arange(xmax, dtype=np.float64) + xmin - center + 0.5) * ss)
        ww = 0.0
        for v in k:            # Pillow accumulates the weights left to right in double
            ww += float(v)
        if ww != 0.0:
            k = k / ww
        weights[xx, :xmax] = k
        bounds[xx] = (xmin, xmax)
    return ksize, bounds, weights


def resample_tables(in_size, out_size, device):
    """(ksize, bounds int32 [out][2], coef int32 [out][ksize]) on ``device`` for the bicubic filter."""
    key = (in_size, out_size, str(device))
    hit = _TABLES.get(key)
    if hit is not None:
        return hit
    ksize, bounds, k = bicubic_windows(in_size, out_size)
    fx = k * float(1 << PRECISION_BITS)
    coef = np.where(k < 0, np.trunc(-0.5 + fx), np.trunc(0.5 + fx)).astype(np.int64).astype(np.int32)
    out = (ksize, torch.from_numpy(bounds).to(device), torch.from_numpy(coef).to(device))
    _TABLES[key] = out
    return out


def resample_weights_f32(in_size, out_size):
    """The fp32 tables of ``resize_tensor`` on the host: (ksize, bounds int32 [out][2], coef float32 [out][ksize]) -- the
    float64 weights of ``bicubic_windows`` rounded once."""
    ksize, bounds, k = bicubic_windows(in_size, out_size)
    return ksize, bounds, k.astype(np.float32)


def resample_tables_f32(in_size, out_size, device):
    """``resample_weights_f32`` on ``device``, cached per (in, out, device) like the integer tables."""
    key = ("f32", in_size, out_size, str(device))
    hit = _TABLES.get(key)
    if hit is None:
        ksize, bounds, coef = resample_weights_f32(in_size, out_size)
        hit = _TABLES[key] = (ksize, torch.from_numpy(bounds).to(device), torch.from_numpy(coef).to(device))
    return hit


def resize_bicubic_u8(img, out_h, out_w):
    """img (B,H,W,C) uint8 CUDA -> (B,out_h,out_w,C) uint8 == PIL Image.resize((out_w,out_h), BICUBIC) per image."""
    if not img.is_cuda or img.dtype != torch.uint8:
        raise RuntimeError("resize_bicubic_u8 needs a CUDA uint8 tensor (no CPU fallback)")
    img = img.contiguous()
    B, H, W, C = img.shape
    x = img
    if out_w != W:
        ks, bnd, cf = resample_tables(W, out_w, img.device)
        y = torch.empty((B, H, out_w, C), device=img.device, dtype=torch.uint8)
        check(lib.ppst_resample_u8(ops._p(x), ops._p(y), B, H, W, C, out_w, 1, ops._p(bnd), ops._p(cf), ks, ops._stream()), "ppst_resample_u8")
        x = y
    if out_h != H:
        ks, bnd, cf = resample_tables(H, out_h, img.device)
        y = torch.empty((B, out_h, x.shape[2], C), device=img.device, dtype=torch.uint8)
        check(lib.ppst_resample_u8(ops._p(x), ops._p(y), B, H, x.shape[2], C, out_h, 0, ops._p(bnd), ops._p(cf), ks, ops._stream()), "ppst_resample_u8")
        x = y
    return x


def resize_tensor(x, out_h, out_w, clamp=None):
    """x (B,C,H,W) float32 CUDA -> (B,C,out_h,out_w): the antialiased bicubic of ``resize_bicubic_u8`` (Pillow's filter) in
    fp32, both axes in one launch (csrc/imageio.hip resample_f32_kernel).  ``clamp`` = (lo, hi) clips the result: a bicubic
    overshoots the range of its input."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 4:
        raise RuntimeError("resize_tensor needs a CUDA float32 (B,C,H,W) tensor (no CPU fallback)")
    return ops.resample_f32(x, out_h, out_w, clamp)


def to_tensor_normalized(img, mean=0.5, std=0.5):
    """(B,H,W,C) uint8 -> (B,C,H,W) float32, ToTensor + Normalize(mean, std)."""
    if not img.is_cuda or img.dtype != torch.uint8:
        raise RuntimeError("to_tensor_normalized needs a CUDA uint8 tensor (no CPU fallback)")
    img = img.contiguous()
    B, H, W, C = img.shape
    y = torch.empty((B, C, H, W), device=img.device, dtype=torch.float32)
    check(lib.ppst_u8_to_tensor(ops._p(img), ops._p(y), B, H, W, C, float(mean), float(std), ops._stream()), "ppst_u8_to_tensor")
    return y


def scale_shortside_size(ow, oh, target_width):
    """__scale_shortside (base_dataset.py:164-168)."""
    scale = target_width / min(ow, oh)
    return round(ow * scale), round(oh * scale)


def make_power_2_size(ow, oh, base=16):
    """__make_power_2 (base_dataset.py:141-149)."""
    return int(round(ow / base) * base), int(round(oh / base) * base)


def preprocess(img, load_size=512):
    """The evaluators' transform for ``preprocess=scale_shortside``: (B,H,W,3) uint8 -> (B,3,h,w) float32 in [-1,1]."""
    B, H, W, C = img.shape
    w1, h1 = scale_shortside_size(W, H, load_size)
    x = resize_bicubic_u8(img, h1, w1) if (w1, h1) != (W, H) else img
    w2, h2 = make_power_2_size(w1, h1)
    if (w2, h2) != (w1, h1):
        x = resize_bicubic_u8(x, h2, w2)
    return to_tensor_normalized(x)


def preprocess_resize(img, load_size=512):
    """The training transform of the reference's launcher (experiments/CelebA_launcher.py:17-18 ``preprocess="resize"``,
    base_dataset.py:91-95): ``transforms.Resize([load_size, load_size], BICUBIC)`` (a square, whatever the aspect), then
    ``__make_power_2``, ToTensor, Normalize: (B,H,W,3) uint8 -> (B,3,h,w) float32 in [-1,1]."""
    B, H, W, C = img.shape
    x = resize_bicubic_u8(img, load_size, load_size) if (W, H) != (load_size, load_size) else img
    w2, h2 = make_power_2_size(load_size, load_size)
    if (w2, h2) != (load_size, load_size):
        x = resize_bicubic_u8(x, h2, w2)
    return to_tensor_normalized(x)


XF_ONE = 1 << 24              # one crop pixel in the integer units of a crop transform (csrc/sim_xf.h)


def crop_transform(centre, side, angle_deg=0.0, n=512):
    """The similarity transform of a square crop inside a photograph, as four Python ints ``(a, b, cu, cv)``: the photo pixel in
    column X, row Y (centre X + 1/2, Y + 1/2) lies at

        U =  a (2X + 1) + b (2Y + 1) + cu,     V = -b (2X + 1) + a (2Y + 1) + cv      (units of 2^-24 crop pixel)

    in the frame of the n x n crop, which is the half-open square 0 <= U, V < n 2^24.  ``centre`` = (x, y) in photo pixels (pixel
    X spans [X, X + 1)) maps to the crop's centre (n/2, n/2); ``side`` is the side of the crop square in photo pixels, so
    s = side / n photo pixels make one crop pixel; (u, v) = R(angle) ((x, y) - centre) / s + n/2 with R = [[cos, sin], [-sin, cos]].
    a = round(2^23 cos / s), b = round(2^23 sin / s); cu, cv put ``centre`` at (n/2, n/2) under the ROUNDED a, b, rounded at 2^-24
    crop pixel: the map is a similarity by construction and exact at the centre, and the rounding of a, b moves a point 8192
    photo pixels from the centre by at most 2^-10 crop pixel.

    Direction: image rows grow downwards, so with a positive angle the crop SQUARE is turned clockwise on screen about its centre
    (its top edge runs from upper left to lower right), and what it shows appears turned counter-clockwise by the same angle in the
    crop: a face whose top leans to the viewer's right by t degrees is upright in the crop at angle_deg = t.

    ``crop_transform_rule`` judges the ROUNDED integers: a turned crop of exactly s = 1 or s = 8 can land a few units of
    a^2 + b^2 outside it (axis-aligned ones are exact); give such a crop a side 2^-20 inside the range."""
    x, y = float(centre[0]), float(centre[1])
    s = float(side) / n
    if not s > 0:
        raise ValueError("crop_transform: side must be positive, got %r" % (side,))
    th = math.radians(float(angle_deg))
    q = round(float(angle_deg) / 90.0)
    if float(angle_deg) == 90.0 * q:                       # whole quarter turns: exact cos / sin
        co, si = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))[q % 4]
    else:
        co, si = math.cos(th), math.sin(th)
    a, b = round((1 << 23) * co / s), round((1 << 23) * si / s)
    cu = round(n * (1 << 23) - 2.0 * (a * x + b * y))
    cv = round(n * (1 << 23) - 2.0 * (-b * x + a * y))
    return a, b, cu, cv


def crop_transform_rule(xf, n):
    """ValueError, from the integers alone, unless every transform of ``xf`` ((4,) or (B,4) ints) has 1 <= s <= 8 photo pixels per
    crop pixel -- 2^40 <= a^2 + b^2 <= 2^46 -- and n is a size the kernels take.  The rule of ``evaluation.native_size_rule``: the
    filter's coefficients are upsampled, never reduced; the upper end bounds the footprint a tile of the crop kernel stages."""
    rows = np.asarray(xf.cpu() if isinstance(xf, torch.Tensor) else xf, dtype=object).reshape(-1, 4)
    if not 1 <= int(n) <= 4096:
        raise ValueError("crop size n = %r is outside 1 .. 4096" % (n,))
    for a, b, cu, cv in rows:
        a, b, cu, cv = int(a), int(b), int(cu), int(cv)
        d = a * a + b * b
        if d > 1 << 46:
            raise ValueError("crop transform (%d, %d, ..): the crop has fewer photo pixels than crop pixels (s = %.4f < 1): "
                             "coefficients are upsampled, never reduced" % (a, b, (1 << 23) / math.sqrt(d)))
        if d < 1 << 40:
            raise ValueError("crop transform (%d, %d, ..): more than 8 photo pixels per crop pixel (s = %s > 8)"
                             % (a, b, "%.4f" % ((1 << 23) / math.sqrt(d)) if d else "inf"))
        if max(abs(cu), abs(cv)) > 1 << 56:
            raise ValueError("crop transform offsets (%d, %d) are beyond 2^56" % (cu, cv))


def extract_similarity(photo_u8, xf, n=512):
    """(B,H,W,3) uint8 photo on the GPU + crop transforms -> (B,n,n,3) uint8 aligned crops (ops.extract_similarity)."""
    return ops.extract_similarity(photo_u8, xf, n)


def encode_png(u8):
    """(B,H,W,C) uint8 on the device (C = 1: grey, 3: RGB) -> list of B ``bytes``, each a complete PNG file.
    Two device-to-host copies per batch: the B sizes, then the batch's file slots cut at the longest file."""
    return _files_to_bytes(*ops.png_encode(u8))


def encode_jpeg(u8, quality=90, subsampling="4:2:0"):
    """(B,H,W,C) uint8 on the device (C = 1: grey, 3: RGB) -> list of B ``bytes``, each a complete baseline JPEG file
    (csrc/jpeg.hip; quality 1 .. 100 with libjpeg's table scaling, subsampling "4:4:4" or "4:2:0").  The same two copies."""
    return _files_to_bytes(*ops.jpeg_encode(u8, quality, subsampling))


def jpeg_info(blob):
    """What the device decoder would do with this file, without a GPU (ppst_jpeg_parse): {"supported": True, "height", "width",
    "components", "sampling" [(h, v) per component], "subsampling" ("grey", "4:4:4" or "4:2:0"), "restart_interval" (MCUs, 0:
    none), "scan_offset", "scan_length"} or {"supported": False, "code", "reason"}."""
    from . import _lib
    rc, d = ops.jpeg_parse(blob)
    if rc != 0:
        return {"supported": False, "code": rc, "reason": _lib.JPEG_REFUSALS.get(rc, "error %d" % rc)}
    return {"supported": True, "height": d.H, "width": d.W, "components": d.ncomp,
            "sampling": [(d.hs[c], d.vs[c]) for c in range(d.ncomp)],
            "subsampling": "grey" if d.ncomp == 1 else ("4:2:0" if d.ss == 2 else "4:4:4"),
            "restart_interval": d.dri, "scan_offset": d.scan_off, "scan_length": d.scan_len}


def decode_jpeg(blobs, mode=None, device="cuda"):
    """blobs: list of baseline JPEG files (bytes; sizes and samplings may differ) -> list of (H,W,C) uint8 tensors on the device,
    each equal to ``numpy.asarray(PIL.Image.open(file))``: C = 1 for a grey file, 3 for a colour one.  ``mode="RGB"``: grey files
    come out with three equal channels (Pillow's ``convert("RGB")``).  One batched call (ops.jpeg_decode).  ValueError with the
    parser's reason for a file the decoder does not take (progressive, 4:2:2, CMYK, ...: ``jpeg_info`` tells without a GPU);
    OSError for a file whose scan the device refused (damaged data)."""
    from . import _lib
    if mode not in (None, "RGB"):
        raise ValueError("mode must be None or 'RGB', not %r" % (mode,))
    views, status = ops.jpeg_decode(blobs, expand_grey=(mode == "RGB"), device=device)
    _raise_damaged("decode_jpeg", status, _lib.JPEG_STATUS_BITS)
    return views


def png_info(blob):
    """What the device decoder would do with this file, without a GPU (ppst_png_parse): {"supported": True, "height", "width",
    "colour_type" (0, 2 or 6), "channels", "chunks" [(type, data offset, length) per chunk], "idat_chunks", "idat_bytes"} or
    {"supported": False, "code", "reason"}."""
    from . import _lib
    rc, d, spans = ops.png_parse(blob)
    if rc != 0:
        return {"supported": False, "code": rc, "reason": _lib.PNG_REFUSALS.get(rc, "error %d" % rc)}
    return {"supported": True, "height": d.H, "width": d.W, "colour_type": d.colour, "channels": d.channels,
            "chunks": [(int(s.type).to_bytes(4, "big").decode("latin-1"), s.off, s.len) for s in spans[:d.nspans]],
            "idat_chunks": d.nidat, "idat_bytes": d.idat_bytes}


def decode_png(blobs, mode=None, device="cuda"):
    """blobs: list of PNG files (bytes; 8 bits per sample, grey / RGB / RGBA, not interlaced; sizes and types may differ) -> list
    of (H,W,C) uint8 tensors on the device, each equal to ``numpy.asarray(PIL.Image.open(file))``: C = 1, 3 or 4.
    ``mode="RGB"``: every image comes out with three channels, as Pillow's ``convert("RGB")`` gives them (grey three times, alpha
    dropped).  One batched call (ops.png_decode).  ValueError with the parser's reason for a file the decoder does not take
    (palette, 16-bit, interlaced, ...: ``png_info`` tells without a GPU); OSError naming the status bits for a file the device
    found damaged."""
    from . import _lib
    if mode not in (None, "RGB"):
        raise ValueError("mode must be None or 'RGB', not %r" % (mode,))
    views, status = ops.png_decode(blobs, expand_grey=(mode == "RGB"), drop_alpha=(mode == "RGB"), device=device)
    _raise_damaged("decode_png", status, _lib.PNG_STATUS_BITS)
    return views


def _raise_damaged(who, status, bits):
    """OSError naming the status bits of the first file the device found damaged"""
    for i, st in enumerate(status.cpu().tolist()):
        if st:
            raise OSError("%s: file %d is damaged (%s)" % (who, i, ", ".join(v for k, v in sorted(bits.items()) if st & k)))


def _files_to_bytes(files, sizes):
    if files.shape[0] == 0:
        return []
    n = sizes.cpu().tolist()
    host = files[:, :max(n)].cpu().numpy()
    return [host[i, :n[i]].tobytes() for i in range(len(n))]
