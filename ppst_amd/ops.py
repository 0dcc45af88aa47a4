"""Torch-facing wrappers over the C ABI (include/ppst_hip.h).

PyTorch is used here for device memory and streams only: every arithmetic
operation of the path is a HIP kernel in libppst_hip.so.  Activations of the
fused path are NHWC fp32 tensors of shape (B, H, W, C) (or channel-slice views
of such tensors: pixel stride ``ld`` = stride(2)).
"""
import collections
import ctypes
import os
import threading
import types

import torch

from . import _lib, conv_tables
from ._lib import lib, check

PAD_ZERO, PAD_REFLECT, PAD_REPLICATE = 0, 1, 2
ACT_NONE, ACT_LRELU, ACT_PRELU = 0, 1, 2
RES_BEFORE_ACT = 1 << 8

PRECISION = {"value": 0}  # 0 = bf16x3 (fp32-class), 1 = single-pass bf16
TILE_ROWS = {"value": 16}  # conv tile rows: 8 (2 blocks per CU) or 16 (1 block per CU)
# 0: everything on the 8-wave tile kernel (conv_mfma.hip).  (1 and 3 were the one-wave-per-SIMD and the two-block forms of
# conv_mfma2.hip: measured slower -- DESIGN.md section 4 -- and removed; choose_kernel refuses them.)
# 2 (default since round 2): layers with Cout % 256 == 0 whose grid still covers the chip run on the 8-wave kernel with
# 128 px x 64 ch wave tiles and a 256-channel N tile (conv_mfma2.hip, WNW = 4): bit-identical to the 64x64-wave-tile kernel
# and 10-16 % faster on those layers (256->256 @256^2 459 vs 417 TFLOP/s, 512->512 @128^2 494 vs 440).
CONV_VARIANT = {"value": 2}
# the fused upscale with Cout % 128 == 0 (and not % 256: those run the N-256 kernel as four phases) as two phase pairs on the N-256
# kernel (ppst_conv_args.dual_b): 256 -> 128 up 2 was the slowest StyledConv layer on the tile kernel (0.42 of the ceiling)
DUAL_CONVT = {"value": True, "min_blocks": 32}
# the fused upscale (Cout % 64 == 0) as the un-blurred 3x3 transposed conv + 2x2 box sum in the epilogue (ppst_conv_args.variant 11,
# conv_mfma2.hip UP9): nine products per input pixel instead of the sixteen of the 4x4 kernel; fp32-class, not bit-identical to the
# four-phase forms (the bit-identity tests of those run with it off)
# (blocks cover 15 x 15 input positions: an extent that fills its last tile badly -- 64 = 4.27 tiles -- stays on the four-phase form)
UP9 = {"value": True, "min_blocks": 64, "min_fill": 0.85}
DIRECT_MAX = {"cout": 64, "nsteps": 40, "cout3x3": 64}   # cout3x3 = 128 was measured: 128->128 @512^2 230 vs 357 TFLOP/s
# thin layers (few channels in and out) on the direct form of that kernel
WGRAD_SPLIT = {"blocks": 1024, "min_tiles": 4}   # conv_wgrad, exact-fp32 kernels: target block count of a launch, fewest pixel tiles per block
# conv_wgrad on the bf16 matrix pipe (conv_wgrad_tr2_kernel): one partial slot per block, two 256-thread blocks per CU -> ONE round of
# <= 512 blocks (every further split is 49 KB more of partial sums per block written and re-read by the scatter), and >= 8 pixel
# tiles (2 x 32 px) per block
WGRAD_TR2_BLOCKS = 512
WGRAD_TR2_MIN_TILES = 8
STREAM_1X1 = {"value": True}       # 1x1 convs (halo 0) on the streaming kernel of conv1x1.hip
# round 5: across-block K split (ppst_conv_args.ksplit) of launches whose grid fills a fraction of the chip while every block runs
# one long serial chain of steps -- the 64^2 ... 4^2 layers of a train step at batch 2 (4-128 blocks of 72-160 steps: ~0.9 us per
# step whatever the grid).  S = the largest of 8 / 4 / 2 with S x blocks <= max_blocks, chunk count divisible by S and >= min_steps
# steps left per block.  Results equal the unsplit launch's up to fp32 summation order: batch-aware passes (the train step) only.
# PPST_KSPLIT=0 turns it off.
KSPLIT = {"value": os.environ.get("PPST_KSPLIT", "1") != "0", "max_blocks": 256, "min_steps": 16, "variants": (0, 2, 10)}
# the workspace every stream that runs a K-split launch owns (PPST_KSPLIT_SCRATCH_BYTES / PPST_KSPLIT_FLAG_WORDS of include/ppst_hip.h)
KSPLIT_SCRATCH_BYTES = 256 * 512 * 128 * 4
KSPLIT_FLAG_WORDS = 4096
# variant 7 (32 x 16 px x 128 ch blocks, conv_mfma2.hip WMW = 4) in the single-pass modes (two activation slots fit there): the
# Cout = 128-class 3x3 layers, which the tile kernel runs at 0.22 of the single-pass ceiling (128 -> 128 @1024^2 fp16)
TALL_TILE_SINGLE = {"value": True, "min_blocks": 64}
# single-pass modes on half-stored activations: 64 input channels per step on the N-256 kernel family (ppst_conv_args.k64) -- half the
# steps (barriers, fragment waits, DMA issues) per MFMA; the Cout = 128-class layers then take 24 x 16 px tiles (variant 9)
K64 = {"value": True}
# round 3: the tile kernel itself as two 4-wave blocks per CU (8 x 16 px x 128 ch tiles, 64 px x 64 ch waves, TWO activation slots,
# 77 KB of LDS each) for the Cout = 128-class layers: one block's prologue / epilogue / barrier waits overlap the other's MFMAs
TWO_BLOCK_8ROW = {"value": False, "min_blocks": 64}
# Batch-aware kernel choice (the TRAINING path only: the trainers switch it on around their passes).  The inference recipes keep
# the batch out of the choice on purpose (a shard of a batch reproduces the whole batch bit for bit); the train step runs 64 x 64
# layers at batch 1-4, where one launch has 32-128 blocks for 256 CUs: with fewer than ``fill`` blocks a Cout % 256 layer leaves
# the N-256 kernel for the tile kernel (twice the N tiles) and the tile kernel takes its 8-row form (twice the M tiles, two blocks
# per CU).  Outputs are bit-identical across these forms; tile statistics differ in the last bit.
BATCH_AWARE = {"value": False, "fill": 192}


class batch_aware:
    """``with ops.batch_aware():`` -- conv kernel choice may look at the batch size inside the block (the train step)."""

    def __enter__(self):
        self.prev = BATCH_AWARE["value"]
        BATCH_AWARE["value"] = True

    def __exit__(self, *exc):
        BATCH_AWARE["value"] = self.prev
# variant 10 (conv_wino.hip): Winograd F(2,3) along x for the plain 3x3 stride-1 layers with Cout >= 128 -- 1.5x fewer MFMAs per
# output; fp32-class (<= 3e-5 against float64) but not bit-identical to the direct kernels.  ``min_blocks``: blocks ONE image gives
# (the choice stays a function of the plan and one image's geometry).
# ``fill`` (batch-aware passes only, i.e. the train step): with fewer than this many blocks in the LAUNCH the choice falls through to
# the direct kernels' under-filled forms (8-row two-block tiles: twice the blocks)
# ``ksplit_fill`` (batch-aware passes with ops.KSPLIT on): a Cout <= 256 layer whose launch has at most this many Winograd blocks runs
# on the tile kernel with the across-block K split instead (256 -> 256 @64^2 x 2: 38 us with S = 4 against 48 on the Winograd kernel
# with S = 2 -- its 128 accumulator registers per thread make the hand-over twice as large; tests/conv_ksplit_time.py)
WINO = {"value": True, "min_blocks": 16, "fill": 0, "ksplit_fill": 64}
# round 5: apply passes whose only consumer is a 1x1 conv are applied by that conv while it loads -- layert1's resnet merge by
# layert1.1 (ConvPlan in_res), the last upsampling block's merge by ToRGB in the image pass (torgb_apply); ToRGB's conv leaves the
# instance-norm partials of its output and one pass normalises them into the NCHW image.  Off: the round-4 passes.
# "torgb": ToRGB is linear and so is the x2 bilinear, so the skip is projected to 3 channels at its own resolution and the projection
# sampled where the outputs are stored (rocprofv3, batch-8 swap step: 0.07 + 0.19 ms against 0.59 + 0.22 for the merge pass + the conv;
# the round-5 form sampled the skip per channel of every pixel and took 1.09 ms).  On: swap step 48.79 -> 48.00 ms, fp16 36.85 ->
# 35.99, hires 39.52 -> 37.23 (profiles/torgb_linear_ab.txt).  PPST_FUSE_TORGB=0: the merge pass + the plain conv.
FUSE_TAIL = {"value": os.environ.get("PPST_FUSE_TAIL", "1") != "0", "torgb": os.environ.get("PPST_FUSE_TORGB", "1") != "0"}
FAT_MIN_BLOCKS = 32         # take the 256-channel tile only when ONE image still gives >= this many blocks (B = 8: one per CU)


def _removed(what):
    """The measured-and-off conv forms are gone from the library."""
    raise RuntimeError("%s was a measured experiment and has been removed; 79feb53 is the last commit that has it" % what)


def set_precision(p):
    """0: bf16x3 (fp32-class, the measured path); 1: single-pass bf16; 2: exact fp32 MFMA (verification only, slow);
    3: single-pass fp16 (the "fp16 generator" of BASELINE configs[4]; fp32 accumulate / statistics / StyleMod)."""
    if p == 4:
        _removed("precision 4 (two-pass fp16)")
    assert p in (0, 1, 2, 3)
    PRECISION["value"] = p


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_cur_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream():
    """torch's current stream on the current device as a raw hipStream_t.  (torch.cuda.current_stream() builds a Stream object
    through several Python layers: ~9 us per call, 2000 calls per training step.)"""
    if _raw_stream is not None and _cur_device is not None:
        return ctypes.c_void_p(_raw_stream(_cur_device()))
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _chk(t, name="tensor"):
    if t is None:
        return
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError("%s must be a CUDA (HIP) tensor" % name)
    if t.dtype != torch.float32:
        raise RuntimeError("%s must be float32, got %s" % (name, t.dtype))


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


_ST = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}       # PPST_ST_* of include/ppst_hip.h
# Half-precision activation storage (round 4, ppst_conv_args.io_st and the `_st` entry points): in the single-pass precision modes
# the NHWC activations of the inference networks (E1, E2, the generator without feature extraction) live in HBM in the operand
# type of the mode -- IEEE half in mode 3, bfloat16 in mode 1 -- instead of fp32: every elementwise pass, blur and HBM-bound conv
# of those paths moves half the bytes.  Accumulation, statistics and the (scale, shift) pairs stay fp32; a kernel rounds once, at
# its store.  Off: fp32 storage in every mode (the round-3 behaviour).  Training keeps fp32 storage either way.
HALF_STORE = {"value": os.environ.get("PPST_HALF_STORE", "1") != "0"}     # (the env switch: A/B runs of bench.py / the tests)


def act_dtype():
    """storage type of the inference networks' activations in the current precision mode"""
    if HALF_STORE["value"] and not torch.is_grad_enabled():
        return {1: torch.bfloat16, 3: torch.float16}.get(PRECISION["value"], torch.float32)
    return torch.float32


# Round 5: half-precision storage of the TRAINING activations and their gradients in precision mode 1 (BASELINE configs[3]'s "bf16": the
# accuracy class of bf16 autocast, whose conv outputs and activation gradients are bfloat16 tensors).  The differentiable networks
# (train_g.py) and the discriminator tape (train.py) start their trunks in train_dtype(); every kernel downstream keeps its input's
# type, gradients take the type of the tensor they belong to.  Parameters, their gradients, Adam, statistics, pooled vectors, style
# codes and the whole correspondence branch stay fp32.
TRAIN_HALF = {"value": os.environ.get("PPST_TRAIN_HALF", "1") != "0"}


def train_dtype():
    return torch.bfloat16 if (TRAIN_HALF["value"] and PRECISION["value"] == 1) else torch.float32


def _chk_act(t, name="activation"):
    if t is None:
        return
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError("%s must be a CUDA (HIP) tensor" % name)
    if t.dtype not in _ST:
        raise RuntimeError("%s must be float32, float16 or bfloat16, got %s" % (name, t.dtype))


def _nhwc_ld(t, name="activation", half_ok=False):
    """validate a (B,H,W,C) tensor or channel-slice view; return pixel stride (elements).  half_ok: the caller's kernel takes a
    storage type (fp16 / bf16 tensors allowed); everything else insists on float32."""
    if half_ok:
        _chk_act(t, name)
    else:
        _chk(t, name)
    B, H, W, C = t.shape
    ld = t.stride(2)
    if t.stride(3) != 1 or t.stride(1) != W * ld or (B > 1 and t.stride(0) != H * W * ld):
        raise RuntimeError("%s must be NHWC-contiguous (or a channel slice of one)" % name)
    return ld


def empty_nhwc(B, H, W, C, like):
    return torch.empty((B, H, W, C), device=like.device, dtype=torch.float32)


# ---------------------------------------------------------------- layout ----
def nchw_to_nhwc(x):
    _chk(x, "x")
    x = x.contiguous()
    B, C, H, W = x.shape
    y = torch.empty((B, H, W, C), device=x.device, dtype=torch.float32)
    check(lib.ppst_nchw_to_nhwc(_p(x), _p(y), B, C, H, W, _stream()), "ppst_nchw_to_nhwc")
    return y


def nhwc_to_nchw(x):
    ld = _nhwc_ld(x)
    B, H, W, C = x.shape
    if ld != C:
        raise RuntimeError("nhwc_to_nchw needs a dense tensor")
    y = torch.empty((B, C, H, W), device=x.device, dtype=torch.float32)
    check(lib.ppst_nhwc_to_nchw(_p(x), _p(y), B, C, H, W, _stream()), "ppst_nhwc_to_nchw")
    return y


# ------------------------------------------------------ upfirdn2d / blur ----
_DT_F64 = 3          # PPST_F64: the two native ops only (every tensor of the call double, arithmetic in double)


def _chk_op(t, name):
    """tensors of the two native ops: float32 / float16 / bfloat16 / float64 (AT_DISPATCH_FLOATING_TYPES_AND_HALF)"""
    if t is None:
        return
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError("%s must be a CUDA (HIP) tensor" % name)
    if t.dtype not in _ST and t.dtype != torch.float64:
        raise RuntimeError("%s must be float32, float16, bfloat16 or float64, got %s" % (name, t.dtype))


def _raw_out(out, shape, like):
    """the destination of a native op: a fresh tensor, or the caller's dense ``out`` of that shape and type"""
    if out is None:
        return torch.empty(shape, device=like.device, dtype=like.dtype)
    _chk_op(out, "out")
    if tuple(out.shape) != tuple(shape) or out.dtype != like.dtype or not out.is_contiguous():
        raise RuntimeError("out must be a dense %s tensor of shape %s" % (like.dtype, tuple(shape)))
    return out


def upfirdn2d_raw(x4, kernel, up_x, up_y, down_x, down_y, px0, px1, py0, py1, out=None):
    """x4: [major, H, W, minor] contiguous (upfirdn2d.cpp:4-23). Returns [major, oh, ow, minor].  float32, float16, bfloat16
    or float64 like the reference's AT_DISPATCH_FLOATING_TYPES_AND_HALF (upfirdn2d_kernel.cu:225); for the 16- and 32-bit types
    the taps are used as fp32 and the products accumulate in fp32 (the reference accumulates in the tensor's type), rounded once
    to the input's type; float64: taps and accumulation in double.  ``out``: write into this tensor."""
    _chk_op(x4, "input")
    _chk_op(kernel, "kernel")
    x4 = x4.contiguous()
    f64 = x4.dtype == torch.float64
    kernel = (kernel.double() if f64 else kernel.float()).contiguous()
    major, in_h, in_w, minor = x4.shape
    kh, kw = kernel.shape
    out_h = (in_h * up_y + py0 + py1 - kh + down_y) // down_y
    out_w = (in_w * up_x + px0 + px1 - kw + down_x) // down_x
    y = _raw_out(out, (major, out_h, out_w, minor), x4)
    check(lib.ppst_upfirdn2d(_p(x4), _p(kernel), _p(y), major, in_h, in_w, minor, kh, kw, up_x, up_y, down_x, down_y,
                             px0, px1, py0, py1, _DT_F64 if f64 else _ST[x4.dtype], _stream()), "ppst_upfirdn2d")
    return y


def blur_nhwc(x, kernel, pad0, pad1, pad_mode=PAD_ZERO, down=1, s2d=False, in_ss=None, in_act=ACT_NONE):
    ld = _nhwc_ld(x, half_ok=True)
    B, H, W, C = x.shape
    if ld != C:
        raise RuntimeError("blur_nhwc needs a dense tensor")
    _chk(kernel, "kernel")
    ks = kernel.shape[0]
    oh = (H + pad0 + pad1 - ks + down) // down
    ow = (W + pad0 + pad1 - ks + down) // down
    if s2d:
        y = torch.empty((B, (oh + 1) // 2, (ow + 1) // 2, 4 * C), device=x.device, dtype=x.dtype)
    else:
        y = torch.empty((B, oh, ow, C), device=x.device, dtype=x.dtype)
    _chk(in_ss, "in_ss")
    check(lib.ppst_blur_nhwc_st(_p(x), _p(kernel.contiguous()), _p(y), B, H, W, C, ks, pad0, pad1, pad_mode, down,
                                1 if s2d else 0, _p(in_ss), in_act, _ST[x.dtype], _stream()), "ppst_blur_nhwc")
    return y, (oh, ow)


def fused_bias_act_raw(x, b, ref, act, grad, alpha, scale, out=None):
    """fused.fused_bias_act (fused_bias_act.cpp:4-20): empty tensor == absent.  float32, float16 or bfloat16 (the reference:
    AT_DISPATCH_FLOATING_TYPES_AND_HALF, fused_bias_act_kernel.cu:79): bias and refer take the input's type, fp32 arithmetic,
    one rounding.  float64 (round 5): arithmetic in double.  ``out``: write into this tensor."""
    _chk_op(x, "input")
    x = x.contiguous()
    b = None if (b is None or b.numel() == 0) else b.to(x.dtype).contiguous()
    ref = None if (ref is None or ref.numel() == 0) else ref.to(x.dtype).contiguous()
    _chk_op(b, "bias")
    _chk_op(ref, "refer")
    y = _raw_out(out, x.shape, x)
    step_b = 1
    for i in range(2, x.dim()):
        step_b *= x.size(i)
    size_b = b.numel() if b is not None else 1
    check(lib.ppst_fused_bias_act(_p(x), _p(b), _p(ref), _p(y), x.numel(), step_b, size_b, act, grad, float(alpha),
                                  float(scale), _DT_F64 if x.dtype == torch.float64 else _ST[x.dtype], _stream()), "ppst_fused_bias_act")
    return y


# ------------------------------------------------------------- fused conv ----
def _tiles(th, tw, rows, cols=16):
    """blocks that cover a (th, tw) extent with rows x cols pixel tiles"""
    return ((th + rows - 1) // rows) * ((tw + cols - 1) // cols)


def _upload(rec, dev):
    """the plan attributes of a conv_tables record: scalars and host lists as they are, every table as an int32 tensor on ``dev``
    (a source list as its three columns; the main one as ``src_dev`` next to the host list ``src``)"""
    d = dict(vars(rec))

    def tensor(rows):
        return None if rows is None else torch.tensor(rows, dtype=torch.int32, device=dev).contiguous()
    for n in ("steps", "steps_dual", "steps_up9", "steps_k64", "steps_dual_k64", "chunk_start"):
        d[n] = tensor(d[n])
    for n, attr in (("src", "src_dev"), ("src_dual", "src_dual"), ("src_k64", "src_k64"), ("src_dual_k64", "src_dual_k64")):
        s = tensor(d[n])
        d[attr] = None if s is None else (s[:, 0].contiguous(), s[:, 1].contiguous(), s[:, 2].contiguous())
    return d


def _weight_source(w, tag, scale):
    """(the tensor a plan's ``wstrides`` index, the scale left to apply) for the (Cout, Cin, k, k) parameter ``w`` and the
    ``wsource`` tag of its conv_tables record"""
    cout, cin, k, _ = w.shape
    if tag == "up4":            # the fused upscale's 4x4 kernel (Cin, Cout, 4, 4), scale folded in
        wsrc = torch.empty((cin, cout, 4, 4), device=w.device, dtype=torch.float32)
        check(lib.ppst_upscale_weight(_p(w), _p(wsrc), cout, cin, scale, _stream()), "ppst_upscale_weight")
        return wsrc, 1.0
    if tag == "flip":           # element (ky', kx') = (0, 0) is W[..][k-1][k-1]
        return w.view(-1)[k * k - 1:], scale
    if tag == "stack":          # the phase-stacked 2x2 kernel (4 Cin, Cout, 2, 2)
        wsrc = torch.empty((4 * cin, cout, 2, 2), device=w.device, dtype=torch.float32)
        check(lib.ppst_dgrad_s2d_stack_weight(_p(w), _p(wsrc), cout, cin, _stream()), "ppst_dgrad_s2d_stack_weight")
        return wsrc, scale
    assert tag == "param"
    return w, scale


# One pack of a plan, by its key in ``plan._packs``: 64 / 128 / 256 (N tile = the key), "dual" (the phase-pair form of the fused
# upscale), "k64_<bn>" / "k64_dual" (64-channel steps), "up9" / "wino" (transforms of their own: ``src`` is None, one launch per
# plan).  entry: the C function that fills it; w / strides / scale: what it reads; src: the (c, ky, kx) device columns; bn,
# n_groups, nsteps, x3 (hi + lo planes; 2: the k64 layout), f16, dual, total: the fields of a ppst_pack_job; elems: int16 elements.
_PackForm = collections.namedtuple("_PackForm", "entry w strides scale cout cin precision src bn n_groups nsteps x3 f16 dual total elems")


def _pack_form(pl, key):
    if key in ("up9", "wino"):
        if key == "up9":        # from the layer's own (Cout, Cin, 3, 3) parameter
            w, strides, scale, nbytes = pl.wparam, (pl.cin * 9, 9, 3, 1), pl.up_scale, lib.ppst_conv_pack_up9_bytes(pl.cout, pl.cin)
        else:
            w, strides, scale, nbytes = pl.wsrc, pl.wstrides, pl.scale, lib.ppst_conv_pack_wino_bytes(pl.cout, pl.cin)
        return _PackForm("ppst_conv_pack_" + key, w, strides, float(scale), pl.cout, pl.cin, pl.precision, None, 0, 0, 0, 0, 0, 0, 0,
                         nbytes // 2)
    k64 = isinstance(key, str) and key.startswith("k64_")
    dual = key in ("dual", "k64_dual")
    bn = 256 if dual else int(key[4:]) if k64 else key
    src = (pl.src_dual_k64 if dual else pl.src_k64) if k64 else (pl.src_dual if dual else pl.src_dev)
    n_groups = 2 if dual else pl.n_groups
    nsteps = src[0].numel() // n_groups
    n_tiles = -(-pl.cout // (bn // 2 if dual else bn))          # (a dual N tile holds both column phases of 128 channels)
    x3 = 2 if k64 else 1 if pl.precision == 0 else 0
    total = n_groups * n_tiles * nsteps * 4 * bn
    entry = "ppst_conv_pack_k64" if k64 else "ppst_conv_pack_dual" if dual else "ppst_conv_pack"
    return _PackForm(entry, pl.wsrc, pl.wstrides, float(pl.scale), pl.cout, pl.cin, pl.precision, src, bn, n_groups, nsteps, x3,
                     1 if pl.precision == 3 else 0, 1 if dual else 0, total, total * 8 * (2 if x3 else 1))


def _pack_launch(f, out):
    """fill the blob ``out`` of pack form ``f`` with the form's own C entry (one launch)"""
    args = (_p(f.w),) + tuple(f.strides) + (f.scale, f.cout)
    if f.src is None:
        args += (f.cin,)
    else:
        args += () if f.entry == "ppst_conv_pack_dual" else (f.bn,)
        args += tuple(_p(t) for t in f.src) + (f.nsteps, f.n_groups, f.precision)
        args += (f.dual,) if f.entry == "ppst_conv_pack_k64" else ()
    check(getattr(lib, f.entry)(*args, _p(out), _stream()), f.entry)


# what one launch of a plan reads, from (choose_kernel's variant and N tile, k64): ppst_conv_args.variant / dual_b / steps / wpack /
# n_groups / nsteps, and the groups its statistics have rows for
_LaunchForm = collections.namedtuple("_LaunchForm", "variant dual_b steps pack n_groups nsteps stat_groups")


class ConvPlan:
    """Packed weights + step table for ppst_conv2d_mfma.

    kind: 'conv' (k in {1,3}, stride 1), 's2d' (3x3 stride 2 over a space-to-depth
    input), 'convT' (fused 4x4 stride-2 transposed conv = 4 output phases of 2x2 taps), and the input gradients 'dgrad',
    'dgrad_s2d', 'dgrad_s2ds', 'dgradT' (conv_tables.py states every table).
    weight: (Cout, Cin, k, k) fp32 CUDA tensor; scale multiplies the weights.
    """

    # Step tables are a function of (kind, weight shape) only (conv_tables.build); uploading one is up to nine host-to-device copies
    # from pageable memory.  A training step rebuilds every plan whose weights it does not repack, ~150 per D + G iteration: the
    # uploaded record is shared between the plans of one (kind, weight shape, device), only the weights are new.
    _GEOMETRY = {}

    def __init__(self, weight, kind="conv", scale=1.0, precision=None):
        _chk(weight, "weight")
        w = weight.detach().contiguous()
        gkey = (kind, tuple(w.shape), str(w.device))
        geom = ConvPlan._GEOMETRY.get(gkey)
        if geom is None:
            geom = ConvPlan._GEOMETRY[gkey] = _upload(conv_tables.build(kind, *w.shape[:3]), w.device)
        self.__dict__.update(geom)
        self.precision = PRECISION["value"] if precision is None else precision
        self.wparam, self.up_scale = w, float(scale)       # (repack_plans: the fp32 parameter storage this plan was packed from)
        self.wsrc, self.scale = _weight_source(w, self.wsource, float(scale))
        if kind == "dgradT":
            self.fwd_scale = float(scale)
        self.wpack = None
        if self.precision != 2:      # (the exact-fp32 verification kernel reads the fp32 weights directly: nothing to pack)
            self._packs = {}
            self.wpack = self.pack_for(self.bn)

    def _pack(self, key):
        """the packed weight blob ``key`` (see _PackForm), built on first use"""
        hit = self._packs.get(key)
        if hit is None:
            f = _pack_form(self, key)
            hit = torch.empty(f.elems, dtype=torch.int16, device=self.steps.device)
            _pack_launch(f, hit)
            self._packs[key] = hit
        return hit

    def pack_for(self, bn):
        """packed weights for N tile ``bn`` (the fat-wave kernel wants 128 / 256)"""
        return self._pack(bn)

    def pack_dual(self):
        """weights for ppst_conv_args.dual_b"""
        return self._pack("dual")

    def pack_k64(self, bn, dual=False):
        """weights for ppst_conv_args.k64"""
        return self._pack("k64_dual" if dual else "k64_%d" % bn)

    def pack_up9(self):
        """weights for variant 11 (the un-blurred 3x3 kernel)"""
        return self._pack("up9")

    def pack_wino(self):
        """transformed weights for variant 10"""
        return self._pack("wino")

    def _launch_form(self, variant, bn, k64):
        dual, up9 = variant == "dual", variant == "up9"
        if k64:
            key, steps = ("k64_dual", self.steps_dual_k64) if dual else ("k64_%d" % bn, self.steps_k64)
        else:
            key = "wino" if variant == 10 else "up9" if up9 else "dual" if dual else bn
            steps = self.steps_up9 if up9 else self.steps_dual if dual else self.steps
        return _LaunchForm(11 if up9 else 2 if dual else variant, 1 if dual else 0, steps,
                           None if self.precision == 2 else self._pack(key), 1 if up9 else 2 if dual else self.n_groups,
                           self.nsteps // 2 if k64 else self.nsteps, 1 if up9 else self.n_groups)

    def takes_in_res(self, H, W):
        """True when a call of this plan on an (H, W) input may carry ``in_res`` (the 1x1 streaming kernel in the fp32-class mode)."""
        return (self.precision == 0 and self.kind == "conv" and self.k == 1 and
                self.choose_kernel(H, W, H, W, H, W, 1)[0] == 4)

    def wino_ok(self, th, tw, oh, ow, H, W, osy):
        # (a call with normalise-on-load and more than 1024 input channels is kept off this kernel in __call__: its LDS copy of
        # the (a, s) table is sized for 32 chunks)
        return (self.precision == 0 and self.kind in ("conv", "dgrad") and self.k == 3 and self.cout >= 128 and osy == 1
                and (th, tw) == (oh, ow) == (H, W)
                and _tiles(th, tw, 16) * ((self.cout + 127) // 128) >= WINO["min_blocks"])

    def choose_kernel(self, th, tw, oh, ow, H, W, osy, B=None, allow_up9=True, allow_wino=True):
        """(variant, N tile, tile rows) of ppst_conv_args for one launch of this plan -- a function of the plan and of ONE
        image's geometry only.  The batch size is deliberately not an argument: every variant gives bit-identical outputs,
        but their tile statistics differ in the last bit (other summation tree), and a shard of a batch has to reproduce the
        whole batch bit for bit (evaluation.grid_exchange; "2 simulated ranks == 1 rank"; tests/test_abi_cpu.py).
          0  tile kernel (64 px x 64 ch waves), bn 64 / 128;      2  its N-256 form (128 px x 64 ch waves) for Cout % 256 == 0
          4  1x1 streaming kernel;   5  direct form for thin stride-2 tables;   6  3x3 register-reuse form (thin layers)
          7  32-row tiles for the Cout = 128-class layers of the single-pass modes;   10  Winograd;   "dual" / "up9"  fused upscale."""
        cv = CONV_VARIANT["value"]
        if cv in (1, 3):
            _removed("conv variant %d" % cv)
        rows = TILE_ROWS["value"]
        variant, bn = 0, self.bn
        single = self.precision in (1, 3)
        if self.precision not in (0, 1, 3):
            return variant, bn, rows                     # exact-fp32 verification: the tile kernel only
        if allow_wino and WINO["value"] and self.wino_ok(th, tw, oh, ow, H, W, osy):
            wblocks = _tiles(th, tw, 16) * ((self.cout + 127) // 128) * (B or 1)
            aware_b = BATCH_AWARE["value"] and B is not None
            if not (aware_b and (wblocks < WINO["fill"] or (KSPLIT["value"] and 0 in KSPLIT["variants"] and self.cout <= 256
                                                             and wblocks <= WINO["ksplit_fill"]))):
                return 10, 128, 16
        tiles16 = _tiles(th, tw, 16) * self.n_groups          # blocks PER IMAGE per N tile
        if (UP9["value"] and allow_up9 and self.kind == "convT" and self.precision == 0 and getattr(self, "steps_up9", None) is not None
                and self.early_a and _tiles(th, tw, 15, 15) * (self.cout // 64) >= UP9["min_blocks"]
                and th * tw >= UP9["min_fill"] * (((th + 14) // 15) * 15) * (((tw + 14) // 15) * 15)):
            return "up9", 256, 15
        if (DUAL_CONVT["value"] and self.kind == "convT" and getattr(self, "steps_dual", None) is not None
                and self.cout % 256 != 0 and cv == 2 and self.early_a
                and _tiles(th, tw, 16) * 2 * (self.cout // 128) >= DUAL_CONVT["min_blocks"]):
            return "dual", 256, 16
        n256_ok = self.cout % 256 == 0 and tiles16 * (self.cout // 256) >= FAT_MIN_BLOCKS
        aware = BATCH_AWARE["value"] and B is not None and not single and self.bn == 128 and self.early_a and self.halo == 1
        if aware and n256_ok and tiles16 * (self.cout // 256) * B < BATCH_AWARE["fill"]:
            n256_ok = False                              # under-filled: the tile kernel has twice the N tiles
        # (with the across-block K split on, an under-filled launch keeps its 16-row tiles and splits K instead: 256 -> 256 @64^2 x 2
        #  38 us with S = 4 against 69 us on 8-row tiles with S = 2)
        small = (aware and tiles16 * ((self.cout + 127) // 128) * B < BATCH_AWARE["fill"]
                 and not (KSPLIT["value"] and 0 in KSPLIT["variants"]))
        if cv == 2 and self.early_a:
            if n256_ok:
                variant, bn = 2, 256                     # 8 waves x (128 px x 64 ch), N tile 256 (conv_mfma2.hip, WNW = 4)
            elif single:
                # single-pass modes: the N-256 geometry, and for Cout = 128-class layers with a halo the 32 x 16 px x 128 ch tile
                if (self.bn == 128 and self.halo == 1 and self.n_groups == 1 and TALL_TILE_SINGLE["value"] and
                        _tiles(th, tw, 32) * ((self.cout + 127) // 128) >= TALL_TILE_SINGLE["min_blocks"]):
                    variant, rows = 7, 32
            elif (self.bn == 128 and self.halo == 1 and (small or (TWO_BLOCK_8ROW["value"] and
                  _tiles(th, tw, 8) * self.n_groups * ((self.cout + 127) // 128) >= TWO_BLOCK_8ROW["min_blocks"]))):
                rows = 8                                 # tile kernel, two 4-wave blocks per CU
        same = (th, tw) == (oh, ow)
        if STREAM_1X1["value"] and self.halo == 0 and self.n_groups == 1 and osy == 1 and same and (oh, ow) == (H, W):
            variant, bn, rows = 4, 64, TILE_ROWS["value"]            # 1x1 convs: streaming kernel, no activation staging
        elif (self.halo == 1 and self.n_groups == 1 and osy == 1 and same and self.cout <= DIRECT_MAX["cout"]
              and self.nsteps <= DIRECT_MAX["nsteps"]):
            # thin layers: direct form of the streaming kernel; plain 3x3 stride-1 tables (order (chunk, dy, dx)) on its
            # register-reuse form
            variant, bn, rows = (6 if (self.kind in ("conv", "dgrad") and self.k == 3) else 5), 64, TILE_ROWS["value"]
        elif (not single and self.kind in ("conv", "dgrad") and self.k == 3 and 64 < self.cout <= DIRECT_MAX["cout3x3"] and same):
            variant, bn, rows = 6, 128, TILE_ROWS["value"]           # (experiment) 32 px x 128 ch waves for Cout in 65..128
        return variant, bn, rows

    def _ksplit(self, variant, a, skip):
        """ppst_conv_args.ksplit of the launch described by ``a`` (0: none) -- ops.KSPLIT."""
        if (skip or variant not in KSPLIT["variants"]
                or not (a.tile_rows == 16 or (variant == 0 and a.tile_rows == 8))):
            return 0, None
        cs = self.chunk_starts0_k64 if a.k64 else self.chunk_starts0       # chunk starts of one group of the launch's table
        if cs is None or cs[-1] != a.nsteps:
            return 0, None
        if a.dual_b or (variant == 2 and ((self.precision == 0) != (a.io_st == 0) or (a.k64 and not a.halo))):
            return 0, None              # (the N-256 kernel's K-split instances: fp32-class on fp32 tensors, single-pass on half-stored ones)
        n_tiles = -(-self.cout // a.bn)
        blocks = a.B * lib.ppst_conv_tiles(a.tile_h, a.tile_w, a.tile_rows) * a.n_groups * n_tiles
        # (the N-256 and Winograd kernels hold 128 accumulator registers per thread: S <= 4, include/ppst_hip.h)
        # -- and what the hand-over of 256 KB per block costs them (tests/conv_ksplit_time.py): the Winograd kernel gains from S = 2 with
        # >= 4 chunks left per block only, the N-256 kernel needs >= 24 steps left
        max_s, min_steps = {0: (8, KSPLIT["min_steps"]), 2: (4, 24), 10: (2, 36)}[variant]
        return _ksplit_choice(blocks, cs, KSPLIT["max_blocks"], min_steps, max_s)

    def __call__(self, x, bias=None, noise=None, noise_weight=0.0, act=ACT_NONE, prelu=None, stats=False,
                 residual=None, out=None, out_scale=1.0, pad_mode=PAD_ZERO, out_hw=None, res_after_act=False,
                 in_ss=None, in_act=ACT_NONE, in_prelu=None, in_res=None):
        in_ld = _nhwc_ld(x, "conv input", half_ok=True)
        B, H, W, xc = x.shape
        if x.dtype != torch.float32 and {torch.float16: 3, torch.bfloat16: 1}[x.dtype] != self.precision:
            raise RuntimeError("conv input stored as %s needs a plan of the matching single-pass precision mode (plan: mode %d)"
                               % (x.dtype, self.precision))
        # the step table lives on the device: the C ABI cannot check these, and the kernel indexes
        # x[.. + chan + 32), in_ss[b][chan][2] and noise[(b*oh+oy)*ow+ox] blindly
        need_c = self.max_chan + 32
        if xc < need_c:
            raise RuntimeError("conv input has %d channels (pixel stride %d); the %s plan reads %d" % (xc, in_ld, self.kind, need_c))
        if in_ss is not None and (in_ss.dim() != 3 or in_ss.shape[0] != B or in_ss.shape[1] < need_c or in_ss.shape[2] != 2
                                  or not in_ss.is_contiguous()):
            raise RuntimeError("in_ss must be a contiguous (B=%d, >=%d, 2) table, got %s" % (B, need_c, tuple(in_ss.shape)))
        if self.kind == "convT":
            th, tw, oh, ow, osy = H, W, 2 * H, 2 * W, 2
        elif self.kind == "dgrad_s2d":
            oh, ow = out_hw                      # extent of the (blurred) tensor the forward conv read
            th, tw, osy = (oh + 1) // 2, (ow + 1) // 2, 2
        elif self.kind in ("s2d", "dgrad_s2ds"):     # (dgrad_s2ds: out_hw = the stacked extents, ceil(input-grid extent / 2))
            oh, ow = out_hw
            th, tw, osy = oh, ow, 1
        else:
            th, tw, oh, ow, osy = H, W, H, W, 1
        if out is None:
            out = torch.empty((B, oh, ow, self.cout), device=x.device, dtype=x.dtype)
        out_ld = _nhwc_ld(out, "conv output", half_ok=True)
        if out.dtype != x.dtype or (residual is not None and residual.dtype != x.dtype):
            raise RuntimeError("conv input, residual and output share one storage type (ppst_conv_args.io_st): got %s / %s / %s"
                               % (x.dtype, None if residual is None else residual.dtype, out.dtype))
        if tuple(out.shape) != (B, oh, ow, self.cout):
            raise RuntimeError("conv output must be %s, got %s" % ((B, oh, ow, self.cout), tuple(out.shape)))
        if noise is not None and (noise.numel() != B * oh * ow or not noise.is_contiguous()):
            raise RuntimeError("noise must be a contiguous (B,1,%d,%d) tensor with B = %d rows, got %s" % (oh, ow, B, tuple(noise.shape)))
        if residual is not None and tuple(residual.shape) != (B, oh, ow, self.cout):
            raise RuntimeError("residual must match the output shape %s, got %s" % ((B, oh, ow, self.cout), tuple(residual.shape)))
        for t, n in ((bias, "bias"), (noise, "noise"), (prelu, "prelu")):
            _chk(t, n)
        # the nine-product upscale takes no normalise-on-load, residual, PReLU or non-zero padding: a call that carries one of them
        # falls back to the phase-pair / four-phase forms (which take all of them) instead of failing (round-4 ADVICE)
        up9_ok = in_ss is None and residual is None and act != ACT_PRELU and pad_mode == PAD_ZERO
        variant, bn, rows = self.choose_kernel(th, tw, oh, ow, H, W, osy, B, allow_up9=up9_ok)
        if variant == 10 and in_ss is not None and self.cin > 1024:      # (the Winograd kernel's LDS copy of the table: wino_ok)
            variant, bn, rows = self.choose_kernel(th, tw, oh, ow, H, W, osy, B, allow_up9=up9_ok, allow_wino=False)
        # single-pass modes on half-stored activations: 64 input channels per step where the N-256 kernel family runs the layer
        k64 = (K64["value"] and x.dtype != torch.float32 and self.precision in (1, 3) and variant in (2, 7, "dual")
               and (self.steps_dual_k64 if variant == "dual" else self.steps_k64) is not None)
        if k64 and variant == 7:
            variant, rows = 9, 24                # the Cout = 128-class layers: 24 x 16 px x 128 ch tiles (two activation slots fit)
        form = self._launch_form(variant, bn, k64)
        variant = form.variant
        st = None
        if stats:
            st = torch.empty((B, form.stat_groups * lib.ppst_conv_tiles(th, tw, rows), self.cout, 2), device=x.device, dtype=torch.float32)
            # (a block of variant 11 writes its row only for channels it owns and every block of the grid writes: no zero fill needed)
        a = _lib.ConvArgs()
        a.x, a.wpack, a.steps, a.y = _p(x), _p(form.pack), _p(form.steps), _p(out)
        a.k64 = 1 if k64 else 0
        a.variant, a.dual_b = variant, form.dual_b
        a.bias, a.noise, a.prelu, a.stats = _p(bias), _p(noise), _p(prelu), _p(st)
        a.residual = _p(residual)
        a.res_ld = _nhwc_ld(residual, "residual", half_ok=True) if residual is not None else 0
        a.io_st = _ST[x.dtype]
        a.noise_weight, a.out_scale = float(noise_weight), float(out_scale)
        a.B, a.in_h, a.in_w, a.in_ld = B, H, W, in_ld
        a.out_h, a.out_w, a.out_ld, a.cout = oh, ow, out_ld, self.cout
        a.nsteps, a.n_groups, a.pad_mode = form.nsteps, form.n_groups, pad_mode
        a.in_off_y = a.in_off_x = 0
        a.out_sy = a.out_sx = osy
        a.act, a.precision = act | (0x100 if res_after_act else 0), self.precision
        a.tile_h, a.tile_w, a.halo, a.bn, a.tile_rows = th, tw, self.halo, bn, rows
        _chk(in_ss, "in_ss"); _chk(in_prelu, "in_prelu")
        a.in_scale_shift, a.in_prelu, a.in_act = _p(in_ss), _p(in_prelu), in_act
        a.in_c = in_ss.shape[1] if in_ss is not None else 0
        if in_res is not None:       # the producer's resnet merge applied on load (ppst_conv_args.in_res): the 1x1 streaming kernel only
            if variant != 4 or in_ss is None or self.precision != 0 or x.dtype != torch.float32:
                raise RuntimeError("in_res needs a 1x1 plan on the streaming kernel (ops.STREAM_1X1), in_ss, precision 0 and fp32 storage")
            if tuple(in_res.shape) != tuple(x.shape):
                raise RuntimeError("in_res must have the conv input's shape %s, got %s" % (tuple(x.shape), tuple(in_res.shape)))
            a.in_res, a.in_res_ld = _p(in_res), _nhwc_ld(in_res, "in_res")
        a.flop_steps = self.flop_steps
        a.a_slots = min(3, self.chunks_per_group)
        a.early_a = self.early_a
        # (batch-aware passes only: the split depends on the batch in the launch and changes the summation order -- a shard of an
        #  inference batch has to reproduce the whole batch bit for bit)
        ks_S, ks_cuts = self._ksplit(variant, a, self.precision == 2) if (KSPLIT["value"] and BATCH_AWARE["value"]) else (0, None)
        stream = _stream()
        if ks_S:
            ks_arr = (ctypes.c_int32 * (ks_S + 1))(*ks_cuts)         # (alive until the call returns)
            a.ksplit, a.ksplit_starts = ks_S, ctypes.cast(ks_arr, ctypes.c_void_p)
            a.ksplit_scratch, a.ksplit_flags, a.ksplit_epoch = _ksplit_next(stream)
        if self.precision == 2:
            sn, sc, sy, sx = self.wstrides
            c_, ky_, kx_ = self.src_dev
            check(lib.ppst_conv2d_f32(ctypes.byref(a), _p(self.wsrc), sn, sc, sy, sx, self.scale, _p(c_), _p(ky_), _p(kx_), stream),
                  "ppst_conv2d_f32")
        else:
            check(lib.ppst_conv2d_mfma(ctypes.byref(a), stream), "ppst_conv2d_mfma")
        if stats:
            return out, st
        return out


class _KsWorkspace:
    """The K-split workspace of one (device, stream): hand-over scratch, zero-filled flags, launch count (include/ppst_hip.h)."""
    __slots__ = ("scratch", "flags", "ptrs", "launches")

    def __init__(self):
        self.scratch = torch.empty(KSPLIT_SCRATCH_BYTES, dtype=torch.uint8, device="cuda")
        self.flags = torch.zeros(KSPLIT_FLAG_WORDS, dtype=torch.int32, device="cuda")
        self.ptrs = self.scratch.data_ptr(), self.flags.data_ptr()
        self.launches = 0


_ks_ws = {}                     # (device index, raw stream) -> _KsWorkspace, kept for the life of the process
_ks_lock = threading.Lock()     # (autograd engine threads launch convs too)


def _ks_key(stream):
    return (_cur_device() if _cur_device is not None else torch.cuda.current_device()), stream.value


def _ksplit_next(stream):
    """(scratch, flags, epoch) of the next K-split launch on ``stream`` (the current one); the workspace is allocated (on that
    stream) at its first one.  The epoch runs 1 .. 2^32 - 1 and wraps past 0: consecutive launches on a workspace never share one."""
    key = _ks_key(stream)
    with _ks_lock:
        ws = _ks_ws.get(key)
        if ws is None:
            ws = _ks_ws[key] = _KsWorkspace()
        ws.launches += 1
        epoch = (ws.launches - 1) % 0xFFFFFFFF + 1
    return ws.ptrs + (epoch,)


def ksplit_launches():
    """Number of K-split launches on the current stream so far (0: none)."""
    ws = _ks_ws.get(_ks_key(_stream()))
    return ws.launches if ws is not None else 0


def ksplit_check():
    """True if every flag wait of the K-split launches on the current stream so far ended on its flag (or none ran), False if a
    block gave up (that launch's output is wrong).  Synchronises the stream and resets the give-up marker."""
    ws = _ks_ws.get(_ks_key(_stream()))
    if ws is None:
        torch.cuda.current_stream().synchronize()
        return True
    marker = ws.flags[KSPLIT_FLAG_WORDS - 1:]
    if marker.item() == 0:
        return True
    marker.zero_()
    return False


def _ksplit_choice(blocks, chunk_starts, max_blocks, min_steps, max_s=8):
    """(S, starts) of ppst_conv_args.ksplit / ksplit_starts for a launch of ``blocks`` blocks over a table whose chunks open at
    ``chunk_starts`` (ascending, from 0; the last entry = nsteps): the largest S of 8 / 4 / 2 that keeps S x blocks <= max_blocks with
    every share -- cut at the chunk starts nearest to equal shares -- at least ``min_steps`` long.  (0, None): no split."""
    nsteps = chunk_starts[-1]
    for S in (8, 4, 2):
        if S > max_s or blocks * S > max_blocks or (S - 1) * blocks > 256 or len(chunk_starts) - 1 < S:
            continue
        cuts = [0]
        for i in range(1, S):
            t = i * nsteps / S
            cuts.append(min(chunk_starts, key=lambda c: (abs(c - t), c)))
        cuts.append(nsteps)
        if all(b_ - a_ >= min_steps for a_, b_ in zip(cuts[:-1], cuts[1:])):
            return S, cuts
    return 0, None


# what run_repack launches: two job tables (device arrays of ppst_upscale_job / ppst_pack_job, their job and block counts), the
# phase-stacked kernels to refresh between them, and the packs that have a transform kernel of their own
_JobTable = collections.namedtuple("_JobTable", "buf njobs nblocks")
_StackJob = collections.namedtuple("_StackJob", "w out cout cin")
_Repack = collections.namedtuple("_Repack", "upscale stack pack single")


def _job_table(cls, rows, dev):
    """``rows`` (field dicts of ``cls``) as a device array with every job's block range filled in"""
    arr = (cls * len(rows))()
    b0 = 0
    for j, r in zip(arr, rows):
        for name, v in r.items():
            setattr(j, name, v)
        j.block0, j.nblocks = b0, lib.ppst_pack_job_blocks(j.total)
        b0 += j.nblocks
    return _JobTable(torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev) if rows else None, len(rows), b0)


def repack_plans(plans):
    """Refresh the packed weights of ``plans`` (ConvPlan objects whose fp32 weights changed in place -- an Adam step) with TWO
    batched launches: the fused-upscale 4x4 kernels of the 'convT' / 'dgradT' plans (ppst_upscale_weight_batch), then every pack
    with source columns of every plan (ppst_conv_pack_batch); the phase-stacked kernels and the "up9" / "wino" packs take one launch
    each.  Every pack is described by _pack_form, as on its first use.  Returns the job tables; pass them to run_repack while the
    set of plans / packs is unchanged (they hold device pointers only: nothing is rebuilt on the host)."""
    up, stack, pk, single = [], [], [], []
    for pl in plans:
        if pl.precision == 2:
            continue
        if pl.wsource == "stack":                # refreshed from the parameter before the packs read it
            stack.append(_StackJob(pl.wparam, pl.wsrc, pl.wparam.shape[0], pl.wparam.shape[1]))
        if pl.wsource == "up4":
            cin4, cout4 = pl.wsrc.shape[0], pl.wsrc.shape[1]         # wsrc is the (Cin, Cout, 4, 4) kernel of the FORWARD conv
            up.append(dict(w=pl.wparam.data_ptr(), out=pl.wsrc.data_ptr(), total=cin4 * cout4 * 16, scale=float(pl.up_scale),
                           cout=cout4, cin=cin4))
        for key, wpack in pl._packs.items():
            f = _pack_form(pl, key)
            if f.src is None:
                single.append((f, wpack))
                continue
            sn, sc, sy, sx = f.strides
            pk.append(dict(w=f.w.data_ptr(), sn=sn, sc=sc, sy=sy, sx=sx, src_c=f.src[0].data_ptr(), src_ky=f.src[1].data_ptr(),
                           src_kx=f.src[2].data_ptr(), out=wpack.data_ptr(), total=f.total, scale=f.scale, cout=f.cout, bn=f.bn,
                           nsteps=f.nsteps, n_groups=f.n_groups, x3=f.x3, f16=f.f16, dual=f.dual))
    dev = plans[0].steps.device if plans else None
    tables = _Repack(_job_table(_lib.UpscaleJob, up, dev), stack, _job_table(_lib.PackJob, pk, dev), single)
    run_repack(tables)
    return tables


def run_repack(tables):
    t = tables
    if t.upscale.njobs:
        check(lib.ppst_upscale_weight_batch(_p(t.upscale.buf), t.upscale.njobs, t.upscale.nblocks, _stream()), "ppst_upscale_weight_batch")
    for e in t.stack:
        check(lib.ppst_dgrad_s2d_stack_weight(_p(e.w), _p(e.out), e.cout, e.cin, _stream()), "ppst_dgrad_s2d_stack_weight")
    if t.pack.njobs:
        check(lib.ppst_conv_pack_batch(_p(t.pack.buf), t.pack.njobs, t.pack.nblocks, _stream()), "ppst_conv_pack_batch")
    for f, wpack in t.single:
        _pack_launch(f, wpack)


def _grad_out(out, shape, like):
    """destination of a parameter gradient: ``out`` (a contiguous view of the trainer's flat gradient, written or added into
    by the kernel itself) or a fresh tensor."""
    if out is None:
        return torch.empty(shape, device=like.device, dtype=torch.float32)
    n = 1
    for d in shape:
        n *= d
    if out.numel() != n or not out.is_contiguous() or out.dtype != torch.float32 or not out.is_cuda:
        raise RuntimeError("gradient destination must be a contiguous float32 CUDA tensor of %d elements, got %s" % (n, tuple(out.shape)))
    return out


# read by bench.py's train line (which kernel and how many MFMA passes its roofline names); nothing sets it
WGRAD_TR = types.MappingProxyType({"value": True, "form": 2, "bf16_single_pass": True})

WgradChoice = collections.namedtuple("WgradChoice", "launcher family chunks_per_block splits promises")


def wgrad_choose(kind, k, halo, max_chunk_steps, min_chunk_steps, nchunks, cout, B, hw, ohw, plan_precision, precision, aligned, splits=None):
    """The launcher conv_wgrad calls for a step table (``kind``, ``k``, ``halo``, longest / shortest chunk, ``nchunks``) on operands
    of these extents (``hw`` input, ``ohw`` output), and the pixel split: pure arithmetic, restating the launchers' own dispatch.
    ``plan_precision`` 2 (exact fp32) or operands without 16-byte rows (``aligned``) -> ppst_conv_wgrad_f32, else the
    transposed-read kernel with 4 ('quad') / 2 ('one2') chunks of a 1x1 table per block, 2 chunks of <= 4 steps ('pair'), or one
    ('single'; '-exact': every chunk has 4 / 9 steps).  ``precision`` 1 (the process's mode): one MFMA pass instead of three.
    ``splits``: the caller's, or blocks = n-tiles x chunk groups x splits filling the chip once (WGRAD_TR2_*) -- the exact-fp32
    kernels run 3 blocks per CU (768 slots): ~2 rounds, >= WGRAD_SPLIT['min_tiles'] pixel tiles per block.  (Round 1 capped
    splits at 64: the 512x512 layers with few channels ran on 64-256 blocks, a third of the chip or less.)
    -> WgradChoice; promises = (max_taps, min_taps, halo, passes) of ppst_conv_wgrad_tr2_st, None for ppst_conv_wgrad_f32."""
    ntiles = (cout + 127) // 128
    tiles_total = B * ((ohw[0] + 1) // 2) * ((ohw[1] + 31) // 32)
    if plan_precision == 2 or not aligned:
        if splits is None:
            per = nchunks * ntiles
            splits = max(1, min((WGRAD_SPLIT["blocks"] + per - 1) // per, max(1, tiles_total // WGRAD_SPLIT["min_tiles"]), 2048))
        return WgradChoice("ppst_conv_wgrad_f32", "f32-lds" if aligned else "f32-direct", 1, splits, None)
    lo, hi = min_chunk_steps, max_chunk_steps
    nohalo = kind == "conv" and k == 1 and halo == 0          # 1x1 tables: one step per chunk, offset (0, 0)
    if nohalo and lo == hi == 1 and tuple(hw) == tuple(ohw) and nchunks % 2 == 0:
        cpb, family = (4, "quad") if nchunks % 4 == 0 else (2, "one2")
    elif hi <= 4 and nchunks % 2 == 0:
        cpb, family = 2, "pair-exact" if lo == hi == 4 else "pair"
    else:
        cpb, family = 1, "single-exact" if lo == hi == 9 else "single"
    if splits is None:
        per = (nchunks // cpb) * ntiles
        splits = max(1, min(max(1, WGRAD_TR2_BLOCKS // per), max(1, tiles_total // WGRAD_TR2_MIN_TILES), 2048))
    return WgradChoice("ppst_conv_wgrad_tr2_st", family, cpb, splits, (hi, lo, 0 if nohalo else 1, 1 if precision == 1 else 3))


def conv_wgrad(plan, x, dy, splits=None, out=None, accumulate=False, bias_out=None, bias_accumulate=False, want_bias=False, dy_scale=1.0):
    """Weight gradient of the conv described by forward ``plan`` ('conv' or 's2d'):
    x = the tensor the forward conv read (NHWC, or the space-to-depth tensor for 's2d'),
    dy = gradient w.r.t. the conv output (before bias/activation).  Returns dW shaped
    (Cout, Cin, k, k), already multiplied by the plan's weight scale (EqualConv2d).
    ``out`` / ``accumulate``: write (or add) into a given destination -- the reduction over the pixel splits adds straight
    into the flat gradient buffer, so no separate accumulation pass (and no zero fill) runs.
    ``want_bias`` / ``bias_out``: also the column sums of dy (the bias gradient), from the fp32 values the weight-gradient kernel
    stages anyway (no second pass over dy): returns (dW, db).
    ``dy_scale``: the gradient is that of ``dy_scale * dy`` (a constant upstream factor rides on the split reduction instead of a
    pass that scales dy; not with the bias outputs)."""
    assert plan.kind in ("conv", "s2d", "dgradT")
    assert dy_scale == 1.0 or not (want_bias or bias_out is not None)
    in_ld = _nhwc_ld(x, "x", half_ok=True)
    dy_ld = _nhwc_ld(dy, "dy", half_ok=True)
    half = x.dtype != torch.float32 or dy.dtype != torch.float32
    if half and not (x.dtype == dy.dtype == torch.bfloat16 and PRECISION["value"] == 1):
        raise RuntimeError("conv_wgrad on half-stored operands: both bfloat16 and precision mode 1 (the single-pass kernel reads them "
                           "as its MFMA operands; got %s / %s, mode %d)" % (x.dtype, dy.dtype, PRECISION["value"]))
    B, H, W, _ = x.shape
    _, oh, ow, cout = dy.shape
    assert cout == plan.cout
    nchunks = plan.chunk_start.numel() - 1
    want_bias = want_bias or bias_out is not None
    aligned = cout % 4 == 0 and dy_ld % 4 == 0 and in_ld % 4 == 0 and x.data_ptr() % 16 == 0 and dy.data_ptr() % 16 == 0
    if half and not (aligned and cout % 8 == 0 and dy_ld % 8 == 0 and in_ld % 8 == 0):
        raise RuntimeError("conv_wgrad on bfloat16 operands needs channel counts / strides divisible by 8 and 16-byte aligned tensors")
    ch = wgrad_choose(plan.kind, plan.k, plan.halo, plan.max_chunk_steps, plan.min_chunk_steps, nchunks, cout, B, (H, W), (oh, ow),
                      plan.precision, PRECISION["value"], aligned, splits)
    splits = ch.splits
    tr2 = ch.promises is not None
    # the transposed-read kernel's staging pass also takes the bias column sums: one row per pixel split
    csum = torch.empty((splits, cout), device=x.device, dtype=torch.float32) if (tr2 and want_bias) else None
    partial = torch.empty((splits, plan.nsteps, cout, 32), device=x.device, dtype=torch.float32)
    if PROF_ON["value"]:
        lib.ppst_wgrad_flop_steps(int(plan.flop_steps))
    if tr2:
        check(lib.ppst_conv_wgrad_tr2_st(_p(x), _p(dy), _p(plan.steps), _p(plan.chunk_start), _p(partial), _p(csum), B, H, W, in_ld, oh, ow,
                                         dy_ld, cout, plan.nsteps, nchunks, splits, *ch.promises, _ST[x.dtype], _stream()), "ppst_conv_wgrad_tr2")
    else:        # precision 2 (verification) or unaligned operands: the exact fp32 MFMA
        check(lib.ppst_conv_wgrad_f32(_p(x), _p(dy), _p(plan.steps), _p(plan.chunk_start), _p(partial), B, H, W, in_ld, oh, ow, dy_ld,
                                      cout, plan.nsteps, nchunks, splits, _stream()), "ppst_conv_wgrad_f32")
    # 'dgradT': the plan's "weights" are the blurred 4x4 kernel (Cin,Cout,4,4) of the transposed conv
    shape = plan.w4_shape if plan.kind == "dgradT" else (plan.cout, plan.cin, plan.k, plan.k)
    cover = getattr(plan, "full_cover", False)
    if out is None:
        dw = (torch.empty if cover else torch.zeros)(shape, device=x.device, dtype=torch.float32)
    else:
        dw = _grad_out(out, shape, x)
        if not accumulate and not cover:
            dw.zero_()
    sn, sc, sy, sx = plan.wstrides
    c_, ky_, kx_ = plan.src_dev
    db = None
    if csum is not None:         # the split reduction also sums the bias partials: no launch of its own
        db = _grad_out(bias_out, (cout,), x)
    check(lib.ppst_wgrad_scatter(_p(partial), _p(c_), _p(ky_), _p(kx_), _p(dw), sn, sc, sy, sx, cout, plan.nsteps, splits,
                                 plan.scale * float(dy_scale), 1 if (accumulate and out is not None) else 0, _p(csum), _p(db),
                                 csum.shape[0] if csum is not None else 0, 1 if (bias_accumulate and bias_out is not None) else 0,
                                 _stream()), "ppst_wgrad_scatter")
    if not want_bias:
        return dw
    if csum is None:
        db = colsum(dy.as_strided((dy.shape[0] * oh * ow, cout), (dy_ld, 1)), out=bias_out, accumulate=bias_accumulate)
    return dw, db


def wgrad_small_cin(x, dy, scale, out=None, accumulate=False):
    """FromRGB: x (B,H,W,cin<=4), dy (B,H,W,cout) -> dW (cout, cin, 1, 1)."""
    in_ld = _nhwc_ld(x)
    B, H, W, cin = x.shape
    cout = dy.shape[3]
    assert _nhwc_ld(dy, "dy", half_ok=True) == cout
    ws = torch.empty(lib.ppst_wgrad_small_cin_ws(B * H * W, cin, cout) // 4, device=x.device, dtype=torch.float32)
    dw = _grad_out(out, (cout, cin, 1, 1), x)
    check(lib.ppst_wgrad_small_cin_st(_p(x), _p(dy), _p(dw), _p(ws), B * H * W, cin, in_ld, cout, float(scale),
                                      1 if (accumulate and out is not None) else 0, _ST[dy.dtype], _stream()), "ppst_wgrad_small_cin")
    return dw


def colsum(x2d, scale=1.0, out=None, accumulate=False):
    """x2d (rows, C) [row stride ld] -> (C,) column sums (bias gradients); x2d fp32 or half-stored, the sums fp32."""
    _chk_act(x2d)
    rows, C = x2d.shape
    ld = x2d.stride(0)
    assert x2d.stride(1) == 1
    ws = torch.empty(lib.ppst_colsum_ws(rows, C) // 4, device=x2d.device, dtype=torch.float32)
    dst = _grad_out(out, (C,), x2d)
    check(lib.ppst_colsum_st(_p(x2d), _p(dst), _p(ws), rows, C, ld, float(scale), 1 if (accumulate and out is not None) else 0,
                             _ST[x2d.dtype], _stream()), "ppst_colsum")
    return dst


def linear_wgrad(dy, x, scale=1.0, out=None, accumulate=False):
    _chk(dy); _chk(x)
    dy, x = dy.contiguous(), x.contiguous()
    B, N = dy.shape
    K = x.shape[1]
    dw = _grad_out(out, (N, K), x)
    check(lib.ppst_linear_wgrad(_p(dy), _p(x), _p(dw), B, N, K, float(scale), 1 if (accumulate and out is not None) else 0, _stream()),
          "ppst_linear_wgrad")
    return dw


def linear_wgrad_fused(dy, x, scale=1.0, out=None, accumulate=False, relu_in=False, bias_out=None, bias_scale=1.0, bias_accumulate=False,
                       want_bias=False):
    """linear_wgrad with the passes around it folded in (ppst_linear_wgrad_fused): ``relu_in`` reads x as max(x, 0); the bias
    gradient bias_scale * sum_b dy[b] comes out of the same launch (``bias_out`` / ``want_bias``).  Returns (dW, db or None)."""
    _chk(dy); _chk(x)
    dy, x = dy.contiguous(), x.contiguous()
    B, N = dy.shape
    K = x.shape[1]
    dw = _grad_out(out, (N, K), x)
    db = _grad_out(bias_out, (N,), x) if (want_bias or bias_out is not None) else None
    check(lib.ppst_linear_wgrad_fused(_p(dy), _p(x), _p(dw), _p(db), B, N, K, float(scale), float(bias_scale),
                                      1 if (accumulate and out is not None) else 0, 1 if (bias_accumulate and bias_out is not None) else 0,
                                      1 if relu_in else 0, _stream()), "ppst_linear_wgrad_fused")
    return dw, db


def linear_dgrad_gate(dy, w, gate, scale=1.0):
    """linear_dgrad whose result is multiplied by [gate > 0] in the slice reduction (the nn.ReLU in front of the linear)."""
    _chk(dy); _chk(w); _chk(gate)
    dy, w, gate = dy.contiguous(), w.detach().contiguous(), gate.contiguous()
    B, N = dy.shape
    K = w.shape[1]
    assert tuple(gate.shape) == (B, K)
    dx = torch.empty((B, K), device=dy.device, dtype=torch.float32)
    ws = torch.empty(lib.ppst_linear_dgrad_ws(B, N, K) // 4, device=dy.device, dtype=torch.float32)
    check(lib.ppst_linear_dgrad_gate(_p(dy), _p(w), _p(dx), _p(ws), _p(gate), B, N, K, float(scale), _stream()), "ppst_linear_dgrad_gate")
    return dx


def linear_dgrad(dy, w, scale=1.0):
    _chk(dy); _chk(w)
    dy, w = dy.contiguous(), w.detach().contiguous()
    B, N = dy.shape
    K = w.shape[1]
    dx = torch.empty((B, K), device=dy.device, dtype=torch.float32)
    ws = torch.empty(lib.ppst_linear_dgrad_ws(B, N, K) // 4, device=dy.device, dtype=torch.float32)
    check(lib.ppst_linear_dgrad(_p(dy), _p(w), _p(dx), _p(ws), B, N, K, float(scale), _stream()), "ppst_linear_dgrad")
    return dx


def lsgan(pred, target, weight):
    """(loss (1,), dloss/dpred) of weight*mean((pred-target)^2)."""
    _chk(pred)
    pred = pred.contiguous()
    loss = torch.empty((1,), device=pred.device, dtype=torch.float32)
    grad = torch.empty_like(pred)
    check(lib.ppst_lsgan(_p(pred), _p(loss), _p(grad), pred.numel(), float(target), float(weight), _stream()), "ppst_lsgan")
    return loss, grad


def l1_mean(a, b, weight=1.0):
    """weight * mean|a - b| -> (1,) tensor (torch.nn.L1Loss)."""
    _chk(a); _chk(b)
    a, b = a.contiguous(), b.contiguous()
    assert a.shape == b.shape
    n = a.numel()
    ws = torch.empty(lib.ppst_l1_mean_ws(n) // 4, device=a.device, dtype=torch.float32)
    out = torch.empty((1,), device=a.device, dtype=torch.float32)
    check(lib.ppst_l1_mean(_p(a), _p(b), _p(out), _p(ws), n, float(weight), _stream()), "ppst_l1_mean")
    return out


def rscl_loss(q, k, k0, queue, nce_T=0.07):
    """rsclLoss.forward: q, k (n, C), k0 (n0, C), queue (C, K) -> (1,) mean NCE loss."""
    for t in (q, k, k0, queue):
        _chk(t)
    q, k, k0, queue = q.contiguous(), k.contiguous(), k0.contiguous(), queue.contiguous()
    n, C = q.shape
    ws = torch.empty((n,), device=q.device, dtype=torch.float32)
    out = torch.empty((1,), device=q.device, dtype=torch.float32)
    check(lib.ppst_rscl_loss(_p(q), _p(k), _p(k0), _p(queue), _p(out), _p(ws), n, k0.shape[0], C, queue.shape[1], float(nce_T), _stream()),
          "ppst_rscl_loss")
    return out


def adam_step_(p, g, m, v, lr, beta1, beta2, eps, step):
    for t in (p, g, m, v):
        _chk(t)
        assert t.is_contiguous()
    check(lib.ppst_adam_step(_p(p), _p(g), _p(m), _p(v), p.numel(), float(lr), float(beta1), float(beta2), float(eps), int(step),
                             _stream()), "ppst_adam_step")


def conv1x1_small_cin(x, w, bias, wscale, act, out_dtype=torch.float32):
    ld = _nhwc_ld(x)
    B, H, W, cin = x.shape
    cout = w.shape[0]
    y = torch.empty((B, H, W, cout), device=x.device, dtype=out_dtype)
    w2 = w.detach().reshape(cout, cin).contiguous()
    check(lib.ppst_conv1x1_small_cin_st(_p(x), _p(w2), _p(bias), _p(y), B * H * W, cin, ld, cout, float(wscale), act,
                                        _ST[out_dtype], _stream()), "ppst_conv1x1_small_cin")
    return y


def conv1x1_small_cin_nchw(x, w, bias, wscale, act, out_dtype=torch.float32):
    """conv1x1_small_cin reading the NCHW image x (B,cin,H,W) itself -> (B,H,W,cout): no layout pass in front."""
    _chk(x, "x")
    B, cin, H, W = x.shape
    if not x.is_contiguous():
        raise RuntimeError("conv1x1_small_cin_nchw needs a contiguous NCHW tensor")
    cout = w.shape[0]
    y = torch.empty((B, H, W, cout), device=x.device, dtype=out_dtype)
    w2 = w.detach().reshape(cout, cin).contiguous()
    check(lib.ppst_conv1x1_small_cin_nchw_st(_p(x), _p(w2), _p(bias), _p(y), B, H * W, cin, cout, float(wscale), act, _ST[out_dtype],
                                             _stream()), "ppst_conv1x1_small_cin_nchw")
    return y


def conv1x1_small_cout(x, w, bias, wscale):
    """x (B,H,W,cin) or a channel slice of a wider tensor (pixel stride a multiple of 4)"""
    ld = _nhwc_ld(x, half_ok=True)
    B, H, W, cin = x.shape
    cout = w.shape[0]
    y = torch.empty((B, H, W, cout), device=x.device, dtype=torch.float32)
    w2 = w.detach().reshape(cout, cin).contiguous()
    check(lib.ppst_conv1x1_small_cout_ld_st(_p(x), _p(w2), _p(bias), _p(y), B * H * W, cin, ld, cout, float(wscale), _ST[x.dtype], _stream()),
          "ppst_conv1x1_small_cout")
    return y


def torgb_apply(x, scale_shift, res, out_scale, w, bias, wscale, stats=False):
    """ToRGB's 1x1 conv reading (a*x + s + bilinear_x2(res)) * out_scale: x (B,H,W,C) dense, scale_shift (B,C,2) or None, res
    (B,H/2,W/2,C) (x's storage type; may be a channel slice) or None -> (B,H,W,3) fp32.  By linearity (ppst_torgb_linear_st): the skip
    is projected to 3 channels at its own resolution (conv1x1_small_cout, scale wscale * out_scale) and that projection is sampled
    where the outputs are stored.  stats: also returns the instance-norm partials (B, n, 3, 2) of the output."""
    ld = _nhwc_ld(x, half_ok=True)
    B, H, W, cin = x.shape
    if ld != cin or w.shape[0] != 3:
        raise RuntimeError("torgb_apply needs a dense input and a 3-channel weight")
    _chk(scale_shift, "scale_shift"); _chk(bias, "bias")
    proj = None
    if res is not None:
        if res.dtype != x.dtype or tuple(res.shape) != (B, H // 2, W // 2, cin) or H % 2 or W % 2:
            raise RuntimeError("torgb_apply: res must be the half-resolution tensor of x's type")
        proj = conv1x1_small_cout(res, w, None, float(wscale) * float(out_scale))
    if scale_shift is not None and (tuple(scale_shift.shape) != (B, cin, 2) or not scale_shift.is_contiguous()):
        raise RuntimeError("torgb_apply: scale_shift must be a contiguous (B, C, 2) table")
    y = torch.empty((B, H, W, 3), device=x.device, dtype=torch.float32)
    w2 = w.detach().reshape(3, cin).contiguous()
    if w2.data_ptr() % 16:          # a view into a flat parameter buffer (the trainers'): the kernel loads 16-byte weight items
        w2 = w2.clone()
    n = ctypes.c_int(0)
    part = None
    if stats:
        check(lib.ppst_torgb_linear_st(None, None, None, 1.0, None, None, None, None, ctypes.byref(n), B, H, W, cin, 1.0, 0, None),
              "ppst_torgb_linear(size)")
        part = torch.empty((B, n.value, 3, 2), device=x.device, dtype=torch.float32)
    check(lib.ppst_torgb_linear_st(_p(x), _p(scale_shift), _p(proj), float(out_scale), _p(w2), _p(bias), _p(y), _p(part), ctypes.byref(n),
                                  B, H, W, cin, float(wscale), _ST[x.dtype], _stream()), "ppst_torgb_linear")
    return (y, part) if stats else y


def encoder_resblock_ok(x, cmid, cout):
    """May ``x`` (B,H,W,C) take encoder_resblock?  Inference in the fp32-class mode on a dense, 16-byte aligned fp32 tensor, channels
    32 -> 32 -> 64, even extents of at least 4 (what ppst_encoder_resblock accepts)."""
    if torch.is_grad_enabled() or PRECISION["value"] != 0 or x.dtype != torch.float32 or not x.is_cuda or x.dim() != 4:
        return False
    B, H, W, cin = x.shape
    return (x.is_contiguous() and x.data_ptr() % 16 == 0 and (cin, cmid, cout) == (32, 32, 64) and B >= 1 and H >= 4 and W >= 4
            and H % 2 == 0 and W % 2 == 0 and H * W * 32 < 2 ** 31)


def encoder_resblock(x, plan1, plan2, plan_s, b1, b2, blur):
    """The no-norm ResBlock 32 -> 32 -> 64 with downsampling in one launch (ppst_encoder_resblock): x (B,H,W,32) dense fp32 ->
    (B,H/2,W/2,64).  plan1 / plan2 / plan_s: the 'conv' ConvPlans (scale folded in) of conv1, conv2 and the skip's 1x1; b1, b2: the two
    activation biases; blur: the 3x3 FIR both branches use.  The entry refuses every other input (PPST_EINVAL)."""
    _chk_act(x, "x"); _chk(b1, "b1"); _chk(b2, "b2"); _chk(blur, "blur")
    B, H, W, cin = x.shape
    dense = x.stride(3) == 1 and x.stride(2) == cin and x.stride(1) == W * cin and (B == 1 or x.stride(0) == H * W * cin)
    if plan1.kind != "conv" or plan2.kind != "conv" or plan_s.kind != "conv" or (plan1.k, plan2.k, plan_s.k) != (3, 3, 1) \
            or plan1.cin != cin or plan2.cin != plan1.cout or plan_s.cin != cin or plan_s.cout != plan2.cout \
            or any(pl.precision != 0 for pl in (plan1, plan2, plan_s)) or blur.numel() != 9 or not blur.is_contiguous() \
            or b1.numel() != plan1.cout or b2.numel() != plan2.cout or not b1.is_contiguous() or not b2.is_contiguous():
        raise RuntimeError("encoder_resblock: plans must be the fp32-class 'conv' plans of a 3x3 / 3x3 / 1x1 ResBlock, blur a 3x3 FIR")
    y = torch.empty((B, H // 2, W // 2, plan2.cout), device=x.device, dtype=torch.float32)
    check(lib.ppst_encoder_resblock(_p(x), _ST[x.dtype], B, H, W, cin, plan1.cout, plan2.cout, x.stride(2) if dense else 0,
                                    _p(plan1.pack_for(64)), _p(plan2.pack_for(64)), _p(plan_s.pack_for(64)), _p(b1), _p(b2), _p(blur), _p(y),
                                    _stream()), "ppst_encoder_resblock")
    return y


def rgb_affine_nchw(y, scale_shift):
    """ToRGB's end: y (B,H,W,3), scale_shift (B,3,2) -> the image (B,3,H,W) = nhwc_to_nchw(affine_act(y, scale_shift)) in one pass."""
    _chk(y, "y"); _chk(scale_shift, "scale_shift")
    B, H, W, C = y.shape
    if C != 3 or not y.is_contiguous() or tuple(scale_shift.shape) != (B, 3, 2) or not scale_shift.is_contiguous():
        raise RuntimeError("rgb_affine_nchw needs a dense (B,H,W,3) tensor and a contiguous (B,3,2) table")
    out = torch.empty((B, 3, H, W), device=y.device, dtype=torch.float32)
    check(lib.ppst_rgb_affine_nchw(_p(y), _p(scale_shift), _p(out), B, H * W, _stream()), "ppst_rgb_affine_nchw")
    return out


def upscale_weight_bwd(dw4, cout, cin, scale=1.0, out=None, accumulate=False):
    """adjoint of the fused-upscale weight blur (stylegan2_layers.py:314-319): dw4 (Cin,Cout,4,4) -> (Cout,Cin,3,3)."""
    _chk(dw4)
    dw = _grad_out(out, (cout, cin, 3, 3), dw4)
    check(lib.ppst_upscale_weight_bwd(_p(dw4.contiguous()), _p(dw), cout, cin, float(scale), 1 if (accumulate and out is not None) else 0,
                                      _stream()), "ppst_upscale_weight_bwd")
    return dw


# round 5: thin stride-2 layers (forward Cin <= max_cin) take their input gradient as the phase-stacked stride-1 conv + depth_to_space
# (plan kind "dgrad_s2ds") instead of the four-group scattered form ("dgrad_s2d").  PPST_DGRAD_S2D_STACK=0: the four-group form.
DGRAD_S2D_STACK = {"value": os.environ.get("PPST_DGRAD_S2D_STACK", "1") != "0", "max_cin": int(os.environ.get("PPST_DGRAD_S2D_MAXCIN", "64"))}


def depth_to_space(x, out_hw):
    """x (B, th, tw, 4 C) with channel block py*2+px = output phase -> (B, oh, ow, C), y[b, 2q+py, 2p+px] = x[b, q, p, phase block]."""
    ld = _nhwc_ld(x, "depth_to_space input", half_ok=True)
    B, th, tw, c4 = x.shape
    if ld != c4 or c4 % 4:
        raise RuntimeError("depth_to_space needs a dense tensor with 4 C channels")
    oh, ow = out_hw
    y = torch.empty((B, oh, ow, c4 // 4), device=x.device, dtype=x.dtype)
    check(lib.ppst_depth_to_space_st(_p(x), _p(y), B, th, tw, oh, ow, c4 // 4, _ST[x.dtype], _stream()), "ppst_depth_to_space_st")
    return y


def dgrad_s2d(net, wname, scale, g, out_hw):
    """Input gradient of the stride-2 3x3 conv ``wname`` of ``net`` (on the blurred tensor of extent ``out_hw``) from the gradient g at
    its output: the phase-stacked form for thin layers (ops.DGRAD_S2D_STACK), else the four-group scattered form."""
    cin = net.p(wname).shape[1]
    per = 8 if g.dtype != torch.float32 else 4
    if DGRAD_S2D_STACK["value"] and cin <= DGRAD_S2D_STACK["max_cin"] and cin % per == 0:
        oh, ow = out_hw
        ys = net.plan(wname, "dgrad_s2ds", scale)(g, out_hw=((oh + 1) // 2, (ow + 1) // 2))
        return depth_to_space(ys, out_hw)
    return net.plan(wname, "dgrad_s2d", scale)(g, out_hw=out_hw)


def space_to_depth(x):
    ld = _nhwc_ld(x, half_ok=True)
    B, H, W, C = x.shape
    y = torch.empty((B, (H + 1) // 2, (W + 1) // 2, 4 * C), device=x.device, dtype=x.dtype)
    check(lib.ppst_space_to_depth_st(_p(x), _p(y), B, H, W, C, ld, _ST[x.dtype], _stream()), "ppst_space_to_depth")
    return y


# ------------------------------------------------- instance norm / affine ----
def in_stats(x, rep_pad=False):
    ld = _nhwc_ld(x)
    B, H, W, C = x.shape
    n = ctypes.c_int(0)
    check(lib.ppst_in_stats(None, None, B, H, W, C, ld, 0, ctypes.byref(n), None), "ppst_in_stats(size)")
    part = torch.empty((B, n.value, C, 2), device=x.device, dtype=torch.float32)
    check(lib.ppst_in_stats(_p(x), _p(part), B, H, W, C, ld, 1 if rep_pad else 0, ctypes.byref(n), _stream()), "ppst_in_stats")
    return part


def in_finalize(partial, count, style=None, post_bias=None, eps=1e-5):
    """partial (B, n, C, 2) -> scale_shift (B, C, 2); style (B, 2C) optional (StyleMod);
    post_bias (C,) optional, added to the shift (activation bias after the norm)."""
    _chk(partial)
    _chk(style, "style")
    _chk(post_bias, "post_bias")
    B, n, C, _ = partial.shape
    style_ld = 0
    if style is not None:  # (B, 2C) rows, possibly a column slice of a wider batched GEMV output
        assert style.shape == (B, 2 * C) and style.stride(1) == 1
        style_ld = style.stride(0) if B > 1 else max(style.stride(0), 2 * C)
    ss = torch.empty((B, C, 2), device=partial.device, dtype=torch.float32)
    check(lib.ppst_in_finalize(_p(partial), n, _p(style), style_ld, _p(post_bias), _p(ss), B, C, float(count), float(eps),
                               _stream()), "ppst_in_finalize")
    return ss


def in_finalize_train(partial, count, style=None, post_bias=None, eps=1e-5):
    """in_finalize that also returns mean_rstd (B, C, 2) for the backward of the norm."""
    _chk(partial); _chk(style, "style"); _chk(post_bias, "post_bias")
    B, n, C, _ = partial.shape
    style_ld = 0
    if style is not None:
        assert style.shape == (B, 2 * C) and style.stride(1) == 1
        style_ld = style.stride(0) if B > 1 else max(style.stride(0), 2 * C)
    ss = torch.empty((B, C, 2), device=partial.device, dtype=torch.float32)
    mr = torch.empty((B, C, 2), device=partial.device, dtype=torch.float32)
    check(lib.ppst_in_finalize_train(_p(partial), n, _p(style), style_ld, _p(post_bias), _p(ss), _p(mr), B, C, float(count), float(eps),
                                     _stream()), "ppst_in_finalize_train")
    return ss, mr


def dual_stats(g, y, gate=None):
    """per-(b, c) partial sums (sum g', sum g'*y), g' = g * lrelu'(gate) when gate is given."""
    g_ld, y_ld = _nhwc_ld(g, "g", half_ok=True), _nhwc_ld(y, "y", half_ok=True)
    gate_ld = _nhwc_ld(gate, "gate", half_ok=True) if gate is not None else 0
    B, H, W, C = g.shape
    assert y.shape == g.shape
    if y.dtype != g.dtype or (gate is not None and gate.dtype != g.dtype):
        raise RuntimeError("dual_stats: g, y and gate share one storage type (got %s / %s / %s)" % (g.dtype, y.dtype, None if gate is None else gate.dtype))
    n = ctypes.c_int(0)
    check(lib.ppst_dual_stats(None, None, None, None, B, H * W, C, g_ld, y_ld, gate_ld, ctypes.byref(n), None), "ppst_dual_stats(size)")
    part = torch.empty((B, n.value, C, 2), device=g.device, dtype=torch.float32)
    check(lib.ppst_dual_stats_st(_p(g), _p(y), _p(gate), _p(part), B, H * W, C, g_ld, y_ld, gate_ld, ctypes.byref(n), _ST[g.dtype], _stream()),
          "ppst_dual_stats")
    return part


def in_bwd_finalize(partial, count, mean_rstd=None, style=None, want_dstyle=False):
    """-> (coef (B,C,4) or None, dstyle (B,2C) or None); see ppst_in_bwd_finalize."""
    _chk(partial); _chk(mean_rstd); _chk(style)
    B, n, C, _ = partial.shape
    style_ld = 0
    if style is not None:
        assert style.shape[0] == B and style.shape[1] >= C and style.stride(1) == 1
        style_ld = style.stride(0) if B > 1 else max(style.stride(0), C)
    coef = torch.empty((B, C, 4), device=partial.device, dtype=torch.float32) if mean_rstd is not None else None
    dstyle = torch.empty((B, 2 * C), device=partial.device, dtype=torch.float32) if (want_dstyle or mean_rstd is None) else None
    check(lib.ppst_in_bwd_finalize(_p(partial), n, _p(mean_rstd), _p(style), style_ld, _p(coef), _p(dstyle), B, C, float(count),
                                   _stream()), "ppst_in_bwd_finalize")
    return coef, dstyle


def in_bwd_apply(g, y, coef, gate=None, post_gate=False):
    g_ld, y_ld = _nhwc_ld(g, "g", half_ok=True), _nhwc_ld(y, "y", half_ok=True)
    gate_ld = _nhwc_ld(gate, "gate", half_ok=True) if gate is not None else 0
    B, H, W, C = g.shape
    if y.dtype != g.dtype or (gate is not None and gate.dtype != g.dtype):
        raise RuntimeError("in_bwd_apply: g, y and gate share one storage type")
    dx = torch.empty((B, H, W, C), device=g.device, dtype=g.dtype)
    check(lib.ppst_in_bwd_apply_st(_p(g), _p(y), _p(gate), _p(coef), _p(dx), B, H * W, C, g_ld, y_ld, gate_ld, C, 1 if post_gate else 0,
                                   _ST[g.dtype], _stream()), "ppst_in_bwd_apply")
    return dx


def prelu_bwd(g, y, prelu, scale_shift=None, res=None):
    """z = a*y + s [+ res]; returns (g * prelu'(z) dense, dslope (1,))."""
    g_ld, y_ld = _nhwc_ld(g, "g"), _nhwc_ld(y, "y")
    res_ld = _nhwc_ld(res, "res") if res is not None else 0
    _chk(prelu); _chk(scale_shift)
    B, H, W, C = g.shape
    total = B * H * W * C
    ws = torch.empty(lib.ppst_prelu_bwd_ws(total) // 4, device=g.device, dtype=torch.float32)
    gpre = torch.empty((B, H, W, C), device=g.device, dtype=torch.float32)
    check(lib.ppst_prelu_bwd(_p(g), _p(y), _p(scale_shift), _p(res), _p(prelu), _p(gpre), _p(ws), B, H * W, C, g_ld, y_ld, res_ld,
                             _stream()), "ppst_prelu_bwd")
    ds = torch.empty((1,), device=g.device, dtype=torch.float32)
    check(lib.ppst_sum_partials(_p(ws), _p(ds), ws.numel(), 1.0, _stream()), "ppst_sum_partials")
    return gpre, ds


def pad2d(x, py0, py1, px0, px1, mode):
    ld = _nhwc_ld(x, half_ok=True)
    B, H, W, C = x.shape
    y = torch.empty((B, H + py0 + py1, W + px0 + px1, C), device=x.device, dtype=x.dtype)
    check(lib.ppst_pad2d_st(_p(x), _p(y), B, H, W, C, ld, py0, py1, px0, px1, mode, _ST[x.dtype], _stream()), "ppst_pad2d")
    return y


def pad2d_bwd(dy, py0, py1, px0, px1, mode):
    _chk_act(dy)
    dy = dy.contiguous()
    B, OH, OW, C = dy.shape
    H, W = OH - py0 - py1, OW - px0 - px1
    dx = torch.empty((B, H, W, C), device=dy.device, dtype=dy.dtype)
    check(lib.ppst_pad2d_bwd_st(_p(dy), _p(dx), B, H, W, C, py0, py1, px0, px1, mode, _ST[dy.dtype], _stream()), "ppst_pad2d_bwd")
    return dx


def bilinear_bwd(dy, H, W):
    dy_ld = _nhwc_ld(dy, half_ok=True)
    B, OH, OW, C = dy.shape
    dx = torch.zeros((B, H, W, C), device=dy.device, dtype=dy.dtype)
    check(lib.ppst_bilinear_bwd_st(_p(dy), _p(dx), B, H, W, C, C, OH, OW, dy_ld, _ST[dy.dtype], _stream()), "ppst_bilinear_bwd")
    return dx


def avgpool_bwd(dy, f):
    dy_ld = _nhwc_ld(dy)
    B, oh, ow, C = dy.shape
    dx = torch.empty((B, oh * f, ow * f, C), device=dy.device, dtype=torch.float32)
    check(lib.ppst_avgpool_bwd(_p(dy), _p(dx), B, oh * f, ow * f, C, C, f, dy_ld, _stream()), "ppst_avgpool_bwd")
    return dx


def gap_gmp_bwd(x, mask, v, g, out=None):
    """adjoint of gap_gmp; out given -> accumulate into it.  The gradient takes x's storage type."""
    ld = _nhwc_ld(x, half_ok=True)
    B, H, W, C = x.shape
    _chk(mask); _chk(v); _chk(g)
    acc = out is not None
    if out is None:
        out = torch.empty((B, H, W, C), device=x.device, dtype=x.dtype)
    arg = torch.empty((B, C), device=x.device, dtype=torch.int32)
    check(lib.ppst_gap_gmp_bwd_st(_p(x), _p(mask), _p(v.contiguous()), _p(g.contiguous()), _p(out), ctypes.c_void_p(arg.data_ptr()), B, H * W, C,
                                  ld, 1 if acc else 0, _ST[x.dtype], _stream()), "ppst_gap_gmp_bwd")
    return out


def gap_gmp_multi(x, masks, with_plain=True):
    """GAP || GMP of x * mask for every channel of ``masks`` (B,H,W,nm) -- and unmasked first when with_plain -- in one read of x:
    -> ((nm + with_plain) * B, 2C), head-major (ppst_gap_gmp_multi)."""
    ld = _nhwc_ld(x, half_ok=True)
    B, H, W, C = x.shape
    _chk(masks, "masks")
    masks = masks.contiguous()
    nm = masks.shape[3]
    assert tuple(masks.shape[:3]) == (B, H, W) and 1 <= nm <= 3
    heads = nm + (1 if with_plain else 0)
    ws = torch.empty(lib.ppst_gap_gmp_multi_ws(B, H * W, C, heads) // 4, device=x.device, dtype=torch.float32)
    out = torch.empty((heads * B, 2 * C), device=x.device, dtype=torch.float32)
    check(lib.ppst_gap_gmp_multi(_p(x), _p(masks), _p(out), _p(ws), B, H, W, C, ld, nm, 1 if with_plain else 0, _ST[x.dtype], _stream()),
          "ppst_gap_gmp_multi")
    return out


def gap_gmp_multi_bwd(x, masks, v, g, with_plain=True, out=None):
    """adjoint of gap_gmp_multi: the sum over the heads, one pass (out given -> accumulate into it)."""
    ld = _nhwc_ld(x, half_ok=True)
    B, H, W, C = x.shape
    _chk(masks); _chk(v); _chk(g)
    masks = masks.contiguous()
    nm = masks.shape[3]
    heads = nm + (1 if with_plain else 0)
    acc = out is not None
    if out is None:
        out = torch.empty((B, H, W, C), device=x.device, dtype=x.dtype)
    arg = torch.empty((heads * B, C), device=x.device, dtype=torch.int32)
    check(lib.ppst_gap_gmp_multi_bwd(_p(x), _p(masks), _p(v.contiguous()), _p(g.contiguous()), _p(out), ctypes.c_void_p(arg.data_ptr()), B,
                                     H * W, C, ld, nm, 1 if with_plain else 0, 1 if acc else 0, _ST[x.dtype], _stream()),
          "ppst_gap_gmp_multi_bwd")
    return out


def l2norm_rows_bwd(g, x, eps, mode):
    _chk(g); _chk(x)
    g, x = g.contiguous(), x.contiguous()
    B, K = x.shape
    dx = torch.empty_like(x)
    check(lib.ppst_l2norm_rows_bwd(_p(g), _p(x), _p(dx), B, K, float(eps), mode, _stream()), "ppst_l2norm_rows_bwd")
    return dx


def softmax_rows_bwd_(p, g, div=1.0):
    """in place on g: g <- p * (g - sum(g*p)) / div."""
    _chk(p); _chk(g)
    assert p.is_contiguous() and g.is_contiguous() and p.shape == g.shape
    cols = p.shape[-1]
    check(lib.ppst_softmax_rows_bwd(_p(p), _p(g), p.numel() // cols, cols, float(div), _stream()), "ppst_softmax_rows_bwd")
    return g


def corr_prep_bwd(g, x, ncenter=256):
    _chk(g); _chk(x)
    g, x = g.contiguous(), x.contiguous()
    B, P, C = x.shape
    dx = torch.empty_like(x)
    check(lib.ppst_corr_prep_bwd(_p(g), _p(x), _p(dx), B * P, C, ncenter, 2.220446049250313e-16, _stream()), "ppst_corr_prep_bwd")
    return dx


def l1_grad(a, b, weight=1.0):
    _chk(a); _chk(b)
    a, b = a.contiguous(), b.contiguous()
    da = torch.empty_like(a)
    check(lib.ppst_l1_grad(_p(a), _p(b), _p(da), a.numel(), float(weight), _stream()), "ppst_l1_grad")
    return da


def rscl_loss_bwd(q, k, k0, queue, gout, nce_T=0.07):
    for t in (q, k, k0, queue, gout):
        _chk(t)
    q, k, k0, queue = q.contiguous(), k.contiguous(), k0.contiguous(), queue.contiguous()
    n, C = q.shape
    dq = torch.empty_like(q)
    check(lib.ppst_rscl_loss_bwd(_p(q), _p(k), _p(k0), _p(queue), _p(gout.contiguous()), _p(dq), n, k0.shape[0], C, queue.shape[1],
                                 float(nce_T), _stream()), "ppst_rscl_loss_bwd")
    return dq


def rselfcorr_bwd(fea, dout):
    ld = _nhwc_ld(fea)
    B, H, W, C = fea.shape
    assert ld == C
    dout_ld = _nhwc_ld(dout)
    dfea = torch.empty_like(fea)
    check(lib.ppst_rselfcorr_bwd(_p(fea), _p(dout), _p(dfea), B, H, W, C, dout_ld, _stream()), "ppst_rselfcorr_bwd")
    return dfea


def transpose_last2(x):
    """(b, M, N) -> (b, N, M) contiguous (the layout-transpose kernel)."""
    _chk(x)
    x = x.contiguous()
    b, M, N = x.shape
    y = torch.empty((b, N, M), device=x.device, dtype=torch.float32)
    check(lib.ppst_nchw_to_nhwc(_p(x), _p(y), b, M, 1, N, _stream()), "ppst_nchw_to_nhwc")
    return y


def scale_by(x, s):
    """x * s[0] with s a (1,) device tensor."""
    _chk(x); _chk(s)
    x = x.contiguous()
    y = torch.empty_like(x)
    check(lib.ppst_scale_by(_p(x), _p(s.contiguous()), _p(y), x.numel(), _stream()), "ppst_scale_by")
    return y


def noise_wgrad(dpre, noise, out=None, accumulate=False):
    ld = _nhwc_ld(dpre, half_ok=True)
    B, H, W, C = dpre.shape
    _chk(noise)
    noise = noise.contiguous()
    assert noise.numel() == B * H * W
    ws = torch.empty(lib.ppst_noise_wgrad_ws(B * H * W) // 4, device=dpre.device, dtype=torch.float32)
    dst = _grad_out(out, (1,), dpre)
    check(lib.ppst_noise_wgrad_st(_p(dpre), _p(noise), _p(dst), _p(ws), B * H * W, C, ld, 1 if (accumulate and out is not None) else 0,
                                  _ST[dpre.dtype], _stream()), "ppst_noise_wgrad")
    return dst


def affine_act(x, scale_shift=None, res=None, act=ACT_NONE, prelu=None, out_scale=1.0, res_before_act=False, out=None,
               res_scale_shift=None, res_up2=False, out_dtype=None):
    """res_up2: ``res`` is a half-resolution tensor, bilinearly upsampled x2 on the fly.  x (and res, which must share its type)
    may be half-stored; the output takes out_dtype (default: x's type)."""
    x_ld = _nhwc_ld(x, half_ok=True)
    B, H, W, C = x.shape
    if out is None:
        out = torch.empty((B, H, W, C), device=x.device, dtype=out_dtype or x.dtype)
    y_ld = _nhwc_ld(out, half_ok=True)
    res_ld = _nhwc_ld(res, "res", half_ok=True) if res is not None else 0
    if res is not None and res.dtype != x.dtype:
        raise RuntimeError("affine_act: res must have the storage type of x (%s), got %s" % (x.dtype, res.dtype))
    _chk(scale_shift, "scale_shift")
    _chk(res_scale_shift, "res_scale_shift")
    _chk(prelu, "prelu")
    if res_up2:
        assert res.shape[1] * 2 == H and res.shape[2] * 2 == W
    flag = act | (RES_BEFORE_ACT if res_before_act else 0)
    check(lib.ppst_affine_act_st(_p(x), _p(scale_shift), _p(res), _p(res_scale_shift), _p(out), B, H * W, C, x_ld, res_ld, y_ld,
                                 flag, _p(prelu), float(out_scale), W if res_up2 else 0, _ST[x.dtype], _ST[out.dtype], _stream()),
          "ppst_affine_act")
    return out


def affine_act_stats(x, scale_shift=None, res=None, act=ACT_NONE, prelu=None, out_scale=1.0, res_before_act=False,
                     res_scale_shift=None, rep_pad=False, res_up2=False):
    """affine_act that also returns the instance-norm partials (B, n, C, 2) of its output."""
    x_ld = _nhwc_ld(x)
    B, H, W, C = x.shape
    out = torch.empty((B, H, W, C), device=x.device, dtype=torch.float32)
    res_ld = _nhwc_ld(res, "res") if res is not None else 0
    for t in (scale_shift, res_scale_shift, prelu):
        _chk(t)
    n = ctypes.c_int(0)
    check(lib.ppst_in_stats(None, None, B, H, W, C, x_ld, 0, ctypes.byref(n), None), "ppst_in_stats(size)")
    part = torch.empty((B, n.value, C, 2), device=x.device, dtype=torch.float32)
    flag = act | (RES_BEFORE_ACT if res_before_act else 0)
    check(lib.ppst_affine_act_stats(_p(x), _p(scale_shift), _p(res), _p(res_scale_shift), _p(out), _p(part), B, H, W, C, x_ld,
                                    res_ld, C, flag, _p(prelu), float(out_scale), 1 if rep_pad else 0, 1 if res_up2 else 0,
                                    _stream()),
          "ppst_affine_act_stats")
    return out, part


def upsample_nearest2(x):
    ld = _nhwc_ld(x, half_ok=True)
    B, H, W, C = x.shape
    assert ld == C
    y = torch.empty((B, 2 * H, 2 * W, C), device=x.device, dtype=x.dtype)
    check(lib.ppst_upsample_nearest2_st(_p(x), _p(y), B, H, W, C, _ST[x.dtype], _stream()), "ppst_upsample_nearest2")
    return y


# ------------------------------------------------------- pooling / resize ----
def gap_gmp(x, mask=None):
    """(B,H,W,C) -> (B, 2C) = cat(mean, max) over pixels; mask (B,H,W) optional multiplier."""
    ld = _nhwc_ld(x, half_ok=True)
    B, H, W, C = x.shape
    _chk(mask, "mask")
    ws = torch.empty(lib.ppst_gap_gmp_ws(B, H * W, C) // 4, device=x.device, dtype=torch.float32)
    out = torch.empty((B, 2 * C), device=x.device, dtype=torch.float32)
    check(lib.ppst_gap_gmp_st(_p(x), _p(mask), _p(out), _p(ws), B, H, W, C, ld, _ST[x.dtype], _stream()), "ppst_gap_gmp")
    return out


def gap_gmp_levels(xs, masks=None):
    """gap_gmp of several feature maps of one batch and one storage type (the pyramid levels of an E2 pass) as one reduction and
    one finalize launch (ppst_gap_gmp_multi_level); more than GROUP_MAX maps go out GROUP_MAX at a time.  -> [(B, 2C)] per map,
    each bit-equal to gap_gmp on the map alone."""
    from ._lib import GROUP_MAX, GapGmpLevel
    masks = list(masks) if masks is not None else [None] * len(xs)
    assert len(masks) == len(xs)
    if not xs:
        return []
    B, dt = xs[0].shape[0], xs[0].dtype
    outs = []
    for i0 in range(0, len(xs), GROUP_MAX):
        grp = list(zip(xs[i0:i0 + GROUP_MAX], masks[i0:i0 + GROUP_MAX]))
        lv = (GapGmpLevel * len(grp))()
        for l, (x, m) in zip(lv, grp):
            ld = _nhwc_ld(x, half_ok=True)
            _chk(m, "mask")
            if x.shape[0] != B or x.dtype != dt:
                raise RuntimeError("gap_gmp_levels: the maps of one call share the batch and the storage type")
            _, H, W, C = x.shape
            out = torch.empty((B, 2 * C), device=x.device, dtype=torch.float32)
            l.x, l.mask, l.out, l.H, l.W, l.C, l.ld = x.data_ptr(), (m.data_ptr() if m is not None else None), out.data_ptr(), H, W, C, ld
            outs.append(out)
        ws = torch.empty(max(lib.ppst_gap_gmp_multi_level_ws(lv, len(grp), B) // 4, 1), device=xs[0].device, dtype=torch.float32)
        check(lib.ppst_gap_gmp_multi_level(lv, len(grp), B, _p(ws), _ST[dt], _stream()), "ppst_gap_gmp_multi_level")
    return outs


def avgpool(x, f, out=None):
    x_ld = _nhwc_ld(x)
    B, H, W, C = x.shape
    if out is None:
        out = torch.empty((B, H // f, W // f, C), device=x.device, dtype=torch.float32)
    y_ld = _nhwc_ld(out)
    check(lib.ppst_avgpool(_p(x), _p(out), B, H, W, C, x_ld, f, y_ld, _stream()), "ppst_avgpool")
    return out


def bilinear(x, OH, OW, out=None):
    x_ld = _nhwc_ld(x)
    B, H, W, C = x.shape
    if out is None:
        out = torch.empty((B, OH, OW, C), device=x.device, dtype=torch.float32)
    y_ld = _nhwc_ld(out)
    check(lib.ppst_bilinear(_p(x), _p(out), B, H, W, C, x_ld, OH, OW, y_ld, _stream()), "ppst_bilinear")
    return out


def head_tail(x, scale_shift, feat, feat1, act=ACT_NONE, prelu=None):
    """feat <- avgpool(act(a*x+s)) to feat's grid; feat1 <- the same f resized by the exact factor 1 or 2 (see ppst_head_tail)."""
    x_ld = _nhwc_ld(x)
    B, H, W, C = x.shape
    P, D = H // feat.shape[1], H // feat1.shape[1]
    _chk(scale_shift, "scale_shift"); _chk(prelu, "prelu")
    check(lib.ppst_head_tail(_p(x), _p(scale_shift), _p(prelu), _p(feat), _p(feat1), B, H, W, C, x_ld, _nhwc_ld(feat), _nhwc_ld(feat1),
                             P, D, act, _stream()), "ppst_head_tail")


def maxpool2(x):
    ld = _nhwc_ld(x)
    B, H, W, C = x.shape
    assert ld == C
    y = torch.empty((B, H // 2, W // 2, C), device=x.device, dtype=torch.float32)
    check(lib.ppst_maxpool2(_p(x), _p(y), B, H, W, C, _stream()), "ppst_maxpool2")
    return y


# ----------------------------------------------------------------- linear ----
def linear(x, w, bias=None, wscale=1.0, bscale=1.0, relu_in=False, act=ACT_NONE):
    _chk(x, "x"); _chk(w, "weight"); _chk(bias, "bias")
    x = x.contiguous()
    w = w.detach().contiguous()
    B, K = x.shape
    N = w.shape[0]
    assert w.numel() == N * K
    y = torch.empty((B, N), device=x.device, dtype=torch.float32)
    check(lib.ppst_linear(_p(x), _p(w), _p(bias), _p(y), B, K, N, float(wscale), float(bscale), 1 if relu_in else 0, act,
                          _stream()), "ppst_linear")
    return y


def linear_grouped(problems):
    """[(x, w, bias, wscale, bscale, relu_in, act), ...] (the arguments of ``linear``; short tuples take its defaults) -> [y]:
    INDEPENDENT linears in one launch per GROUP_MAX problems (ppst_linear_grouped), each bit-equal to ``linear`` on it."""
    from ._lib import GROUP_MAX, LinearProblem
    ys, hold = [], []
    defaults = (None, 1.0, 1.0, False, ACT_NONE)
    for i0 in range(0, len(problems), GROUP_MAX):
        grp = problems[i0:i0 + GROUP_MAX]
        arr = (LinearProblem * len(grp))()
        for q, pr in zip(arr, grp):
            x, w = pr[0], pr[1]
            bias, wscale, bscale, relu_in, act = tuple(pr[2:]) + defaults[len(pr) - 2:]
            _chk(x, "x"); _chk(w, "weight"); _chk(bias, "bias")
            x = x.contiguous()
            w = w.detach().contiguous()
            B, K = x.shape
            N = w.shape[0]
            assert w.numel() == N * K
            y = torch.empty((B, N), device=x.device, dtype=torch.float32)
            q.x, q.w, q.bias, q.y = x.data_ptr(), w.data_ptr(), (bias.data_ptr() if bias is not None else None), y.data_ptr()
            q.B, q.K, q.N, q.wscale, q.bscale, q.relu_in, q.act = B, K, N, float(wscale), float(bscale), 1 if relu_in else 0, act
            ys.append(y)
            hold.append((x, w))
        check(lib.ppst_linear_grouped(arr, len(grp), _stream()), "ppst_linear_grouped")
    return ys


def l2norm_rows_grouped(xs, eps, mode):
    """l2norm_rows of several (B, K) tensors in one launch per GROUP_MAX (ppst_l2norm_rows_grouped)."""
    from ._lib import GROUP_MAX, L2normProblem
    ys, hold = [], []
    for i0 in range(0, len(xs), GROUP_MAX):
        grp = xs[i0:i0 + GROUP_MAX]
        arr = (L2normProblem * len(grp))()
        for q, x in zip(arr, grp):
            _chk(x)
            x = x.contiguous()
            y = torch.empty_like(x)
            q.x, q.y, q.B, q.K, q.eps, q.mode = x.data_ptr(), y.data_ptr(), x.shape[0], x.shape[1], float(eps), mode
            ys.append(y)
            hold.append(x)
        check(lib.ppst_l2norm_rows_grouped(arr, len(grp), _stream()), "ppst_l2norm_rows_grouped")
    return ys


def lerp_grouped(pairs, r):
    """lerp(a, b, r) of several (a, b) pairs in one launch per GROUP_MAX (ppst_lerp_grouped)."""
    from ._lib import GROUP_MAX, LerpProblem
    ys, hold = [], []
    for i0 in range(0, len(pairs), GROUP_MAX):
        grp = pairs[i0:i0 + GROUP_MAX]
        arr = (LerpProblem * len(grp))()
        for q, (a, b) in zip(arr, grp):
            _chk(a); _chk(b)
            a, b = a.contiguous(), b.contiguous()
            y = torch.empty_like(a)
            q.a, q.b, q.y, q.n, q.r = a.data_ptr(), b.data_ptr(), y.data_ptr(), a.numel(), float(r)
            ys.append(y)
            hold.append((a, b))
        check(lib.ppst_lerp_grouped(arr, len(grp), _stream()), "ppst_lerp_grouped")
    return ys


def l2norm_rows(x, eps, mode):
    _chk(x)
    x = x.contiguous()
    B, K = x.shape
    y = torch.empty_like(x)
    check(lib.ppst_l2norm_rows(_p(x), _p(y), B, K, float(eps), mode, _stream()), "ppst_l2norm_rows")
    return y


def lerp(a, b, r):
    _chk(a); _chk(b)
    a, b = a.contiguous(), b.contiguous()
    y = torch.empty_like(a)
    check(lib.ppst_lerp(_p(a), _p(b), _p(y), a.numel(), float(r), _stream()), "ppst_lerp")
    return y


def spatial_modulation(x, scale, bias, out_dtype=torch.float32):
    ld = _nhwc_ld(x)
    B, H, W, C = x.shape
    assert ld == C
    y = torch.empty(x.shape, device=x.device, dtype=out_dtype)
    check(lib.ppst_spatial_modulation_st(_p(x), _p(scale.contiguous()), _p(bias.contiguous()), _p(y), B, H * W, C, _ST[out_dtype],
                                         _stream()), "ppst_spatial_modulation")
    return y


# --------------------------------------------------------- correspondence ----
def rselfcorr(fea, out=None):
    ld = _nhwc_ld(fea)
    B, H, W, C = fea.shape
    assert ld == C
    if out is None:
        out = torch.empty((B, H // 4, W // 4, 256), device=fea.device, dtype=torch.float32)
    out_ld = _nhwc_ld(out)
    check(lib.ppst_rselfcorr(_p(fea), _p(out), B, H, W, C, out_ld, _stream()), "ppst_rselfcorr")
    return out


def corr_prep(fea, ncenter=256):
    """fea (B, P, C) dense -> centred / L2-normalised rows."""
    _chk(fea)
    fea = fea.contiguous()
    B, P, C = fea.shape
    y = torch.empty_like(fea)
    check(lib.ppst_corr_prep(_p(fea), _p(y), B, P, C, ncenter, _stream()), "ppst_corr_prep")
    return y


def unfold_rows(x, k):
    """F.unfold(x, k, padding=k // 2) of an NHWC map (B,H,W,C) as rows (B, H*W, C*k*k) (ppst_model.py:345-347; k odd)."""
    _chk(x)
    x = x.contiguous()
    B, H, W, C = x.shape
    out = torch.empty((B, H * W, C * k * k), device=x.device, dtype=torch.float32)
    check(lib.ppst_unfold_rows(_p(x), _p(out), B, H, W, C, int(k), _stream()), "ppst_unfold_rows")
    return out


def unfold_rows_bwd(g, shape, k):
    """gradient of unfold_rows: g (B, H*W, C*k*k) -> (B,H,W,C)."""
    _chk(g)
    g = g.contiguous()
    B, H, W, C = shape
    dx = torch.empty((B, H, W, C), device=g.device, dtype=torch.float32)
    check(lib.ppst_unfold_rows_bwd(_p(g), _p(dx), B, H, W, C, int(k), _stream()), "ppst_unfold_rows_bwd")
    return dx


GEMM_MODE = {"value": None}    # None: per call site ("x6" fp32-class / "x3" bf16x3); "f32": the exact-fp32 MFMA kernels everywhere


def _gemm_passes(mode, K):
    """0 = exact-fp32 MFMA kernel, 6 / 3 = bf16 planes (ppst_gemm_*_split).  Exact-conv mode (precision 2) and shapes the
    split kernels do not take (K % 16 / K % 32) use the fp32 kernel."""
    mode = GEMM_MODE["value"] or mode or "x6"
    if mode not in ("f32", "x6", "x3"):
        raise ValueError("gemm mode %r" % (mode,))
    if mode == "f32" or PRECISION["value"] == 2:
        return 0
    if mode == "x3" and K % 32 == 0:
        return 3
    return 6 if K % 16 == 0 else 0


def gemm_nt(A, Bm, alpha=1.0, mode=None):
    """A (b,M,K), Bm (b,N,K) -> (b,M,N) = alpha * A @ Bm^T.  mode: "x6" (default: three bf16 planes per operand, fp32-class),
    "x3" (bf16x3, the convs' accuracy class), "f32" (fp32 MFMA)."""
    _chk(A); _chk(Bm)
    A, Bm = A.contiguous(), Bm.contiguous()
    b, M, K = A.shape
    N = Bm.shape[1]
    passes = _gemm_passes(mode, K)
    if K % 16:
        raise ValueError("gemm_nt: K = %d; every kernel (split and fp32) takes K %% 16 == 0 only" % K)
    C = torch.empty((b, M, N), device=A.device, dtype=torch.float32)
    if passes:
        check(lib.ppst_gemm_nt_split(_p(A), _p(Bm), _p(C), b, M, N, K, float(alpha), passes, _stream()), "ppst_gemm_nt_split")
    else:
        check(lib.ppst_gemm_nt_f32(_p(A), _p(Bm), _p(C), b, M, N, K, float(alpha), _stream()), "ppst_gemm_nt_f32")
    return C


def gemm_nn(A, Bm, mode=None):
    """A (b,M,K), Bm (b,K,N) -> (b,M,N); mode as gemm_nt."""
    _chk(A); _chk(Bm)
    A, Bm = A.contiguous(), Bm.contiguous()
    b, M, K = A.shape
    N = Bm.shape[2]
    passes = _gemm_passes(mode, K) if N % 4 == 0 else 0
    if N % 4 or K % 16:       # (the fp32 kernel these fall through to reads B four columns and K sixteen rows at a time as well)
        raise ValueError("gemm_nn: N = %d, K = %d; every kernel (split and fp32) takes N %% 4 == 0 and K %% 16 == 0 only" % (N, K))
    C = torch.empty((b, M, N), device=A.device, dtype=torch.float32)
    if passes:
        check(lib.ppst_gemm_nn_split(_p(A), _p(Bm), _p(C), b, M, N, K, N, N, passes, _stream()), "ppst_gemm_nn_split")
    else:
        check(lib.ppst_gemm_nn_f32(_p(A), _p(Bm), _p(C), b, M, N, K, N, N, _stream()), "ppst_gemm_nn_f32")
    return C


def softmax_rows_(x, div=1.0):
    _chk(x)
    assert x.is_contiguous()
    cols = x.shape[-1]
    if cols % 4 or cols > 16384:
        raise ValueError("softmax_rows_: cols = %d; the kernel holds a row of cols %% 4 == 0, cols <= 16384 in registers" % cols)
    check(lib.ppst_softmax_rows(_p(x), x.numel() // cols, cols, float(div), _stream()), "ppst_softmax_rows")
    return x


def unfold_patches(x, s):
    _chk(x)
    x = x.contiguous()
    B, C, H, W = x.shape
    y = torch.empty((B, (H // s) * (W // s), C * s * s), device=x.device, dtype=torch.float32)
    check(lib.ppst_unfold_patches(_p(x), _p(y), B, C, H, W, s, _stream()), "ppst_unfold_patches")
    return y


def fold_patches(x, C, H, W, s):
    _chk(x)
    x = x.contiguous()
    B = x.shape[0]
    y = torch.empty((B, C, H, W), device=x.device, dtype=torch.float32)
    check(lib.ppst_fold_patches(_p(x), _p(y), B, C, H, W, s, _stream()), "ppst_fold_patches")
    return y


# ----------------------------------------------------------- post-process ----
def tensor2im_u8(x):
    """NCHW fp32 -> (B,H,W,C) uint8 (util.tensor2im truncation)."""
    _chk(x)
    x = x.contiguous()
    B, C, H, W = x.shape
    y = torch.empty((B, H, W, C), device=x.device, dtype=torch.uint8)
    check(lib.ppst_tensor2im_u8(_p(x), _p(y), B, C, H, W, _stream()), "ppst_tensor2im_u8")
    return y


def _need_cuda(who, what, dtype, *tensors):
    """``who`` needs ``what``: every one of ``tensors`` a CUDA tensor of ``dtype``"""
    for t in tensors:
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype:
            raise RuntimeError("%s needs %s" % (who, what))


def _need_shapes(who, what, ok, *tensors):
    """``who`` needs ``what``, the shape family that ``ok`` tested on ``tensors``"""
    if not ok:
        raise RuntimeError("%s needs %s, got %s" % (who, what, " and ".join(str(tuple(t.shape)) for t in tensors)))


def _need_match(who, what, t, shape, like, whose):
    """``who`` needs ``what`` = ``shape`` (the batch and extents of ``like``) on ``like``'s device -> ``t``, contiguous"""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != like.device or tuple(t.shape) != shape:
        raise RuntimeError("%s needs %s = %s on the %s's device" % (who, what, shape, whose))
    return t.contiguous()


_is_image = lambda t: t.dim() == 4 and t.shape[3] == 3                            # (B,H,W,3)
_is_coeffs = lambda t: t.dim() == 4 and t.shape[1] == 12                          # (B,12,h,w)


def _guide_and_source(who, guide_u8, src_u8, dims):
    """the filter's two inputs, checked -> (guide, source, workspace), the two contiguous"""
    _need_cuda(who, "CUDA uint8 tensors", torch.uint8, guide_u8, src_u8)
    _need_shapes(who, "guide and source of one shape %s" % dims, _is_image(guide_u8) and src_u8.shape == guide_u8.shape,
                 guide_u8, src_u8)                                                # (the kernels index both by the guide's extents)
    ws = torch.empty(lib.ppst_guided_filter_ws(*guide_u8.shape[:3]), device=guide_u8.device, dtype=torch.uint8)
    return guide_u8.contiguous(), src_u8.contiguous(), ws


def guided_filter(guide_u8, src_u8, r=30, eps=(0.02 * 255) ** 2, want_u8=False):
    """guide/src (B,H,W,3) uint8 -> fp32 NCHW in [-1,1] (and the uint8 HWC result).  r = 30, 60 and 90 run as two fused
    launches (the radii of 512^2, 1024^2 and 1536^2 images, ppst_model.guided_filter_radius); every other r <= 64 runs the
    five-launch generic path; any other r, r >= H, r >= W and W > 2048 are refused."""
    guide_u8, src_u8, ws = _guide_and_source("guided_filter", guide_u8, src_u8, "(B,H,W,3)")
    B, H, W, _ = guide_u8.shape
    out = torch.empty((B, 3, H, W), device=guide_u8.device, dtype=torch.float32)
    out_u8 = torch.empty((B, H, W, 3), device=guide_u8.device, dtype=torch.uint8) if want_u8 else None
    check(lib.ppst_guided_filter(_p(guide_u8), _p(src_u8), _p(out), _p(out_u8), B, H, W, r, float(eps), _p(ws), _stream()),
          "ppst_guided_filter")
    return (out, out_u8) if want_u8 else out


def guided_filter_coeffs(guide_u8, src_u8, r=30, eps=(0.02 * 255) ** 2):
    """guide/src (B,h,w,3) uint8 -> (B,12,h,w) fp32: the filter's mean coefficient planes (plane 4c + k: k = 0..2 mean a_ck,
    k = 3 mean b_c), what ``guided_filter_apply`` upsamples.  Five launches through fp32 planes at every radius: 0 < r <= 64
    (30 and 60 included, 90 refused), r < h, r < w, w <= 2048."""
    guide_u8, src_u8, ws = _guide_and_source("guided_filter_coeffs", guide_u8, src_u8, "(B,h,w,3)")
    B, h, w, _ = guide_u8.shape
    coeffs = torch.empty((B, 12, h, w), device=guide_u8.device, dtype=torch.float32)
    check(lib.ppst_guided_filter_coeffs(_p(guide_u8), _p(src_u8), _p(coeffs), B, h, w, int(r), float(eps), _p(ws), _stream()),
          "ppst_guided_filter_coeffs")
    return coeffs


def guided_filter_apply(coeffs, guide_full_u8, want_f32=False):
    """coeffs (B,12,h,w) fp32 (``guided_filter_coeffs``), guide (B,H,W,3) uint8 with H >= h, W >= w -> uint8 (B,H,W,3): the
    coefficients upsampled bilinearly (half-pixel centres, any ratio per axis) and applied to the guide at its own size, one
    launch; ``want_f32``: also the fp32 NCHW image (q/255 - 0.5)*2 of those bytes.  H < h, W < w and H W > 2^28 are refused."""
    _need_cuda("guided_filter_apply", "CUDA float32 coefficients", torch.float32, coeffs)
    _need_cuda("guided_filter_apply", "a CUDA uint8 guide", torch.uint8, guide_full_u8)
    _need_shapes("guided_filter_apply", "coefficients (B,12,h,w) and a guide (B,H,W,3) of one batch",
                 _is_coeffs(coeffs) and _is_image(guide_full_u8) and guide_full_u8.shape[0] == coeffs.shape[0], coeffs, guide_full_u8)
    coeffs, guide_full_u8 = coeffs.contiguous(), guide_full_u8.contiguous()
    B, _, h, w = coeffs.shape
    _, H, W, _ = guide_full_u8.shape
    out_u8 = torch.empty((B, H, W, 3), device=coeffs.device, dtype=torch.uint8)
    out = torch.empty((B, 3, H, W), device=coeffs.device, dtype=torch.float32) if want_f32 else None
    check(lib.ppst_guided_filter_apply(_p(coeffs), h, w, _p(guide_full_u8), _p(out_u8), _p(out), B, H, W, _stream()),
          "ppst_guided_filter_apply")
    return (out_u8, out) if want_f32 else out_u8


def _crop_transforms(xf, B, device, who):
    """crop transforms (imageio.crop_transform) as ((B,4) int64 on the host, the same table on ``device``); one transform serves
    every image of the batch"""
    if isinstance(xf, torch.Tensor):
        if xf.dtype != torch.int64:
            raise RuntimeError("%s needs int64 crop transforms, got %s" % (who, xf.dtype))
        host = xf.detach().cpu()
    else:
        host = torch.tensor([[int(v) for v in row] for row in (xf if len(xf) and hasattr(xf[0], "__len__") else [xf])], dtype=torch.int64)
    host = host.reshape(-1, 4)
    if host.shape[0] == 1 and B != 1:
        host = host.expand(B, 4)
    if host.shape[0] != B:
        raise RuntimeError("%s needs one crop transform (a, b, cu, cv) per image: %d for a batch of %d" % (who, host.shape[0], B))
    host = host.contiguous()
    return host, host.to(device)


def extract_similarity(photo_u8, xf, n=512):
    """photo (B,H,W,3) uint8 on the GPU, ``xf`` (B,4) int64 crop transforms (imageio.crop_transform; a tensor or nested ints, one
    row serves a whole batch) -> (B,n,n,3) uint8: the n x n crop of each photo under its similarity transform, Pillow's
    antialiased bicubic in the crop's frame, the photo read with edge replication (csrc/imageio.hip
    extract_similarity_kernel).  Transforms with s < 1 or s > 8 photo pixels per crop pixel are refused."""
    _need_cuda("extract_similarity", "a CUDA uint8 photo", torch.uint8, photo_u8)
    _need_shapes("extract_similarity", "a photo (B,H,W,3)", _is_image(photo_u8), photo_u8)
    photo_u8 = photo_u8.contiguous()
    B, H, W, _ = photo_u8.shape
    host, dev = _crop_transforms(xf, B, photo_u8.device, "extract_similarity")
    out = torch.empty((B, int(n), int(n), 3), device=photo_u8.device, dtype=torch.uint8)
    check(lib.ppst_extract_similarity(_p(photo_u8), B, H, W, _p(host), _p(dev), int(n), _p(out), _stream()), "ppst_extract_similarity")
    return out


def label_matte(labels, keep=(1, 2), feather=16, grow=8, want_distance=False):
    """labels (B,h,w) uint8 on the GPU, ``keep`` the label values (0..31) that count as inside -> fp32 matte (B,h,w) in [0, 1]: the
    smoothstep over ``feather`` pixels of the signed Euclidean distance to the kept region's boundary, moved outwards by ``grow``
    pixels (csrc/matte.hip; the semantics are at ppst_label_matte in include/ppst_hip.h).  grow = 0 feathers inwards only,
    grow = feather / 2 centres the ramp on the boundary; both in [0, 255].  ``want_distance``: also the exact int32 signed squared
    distance (B,h,w), clipped to +-R^2, R = max(grow, max(feather - grow, 0)) + 1."""
    _need_cuda("label_matte", "CUDA uint8 labels", torch.uint8, labels)
    _need_shapes("label_matte", "labels (B,h,w)", labels.dim() == 3, labels)
    mask = 0
    for k in keep:
        if int(k) != k or not 0 <= int(k) <= 31:
            raise RuntimeError("label_matte keeps label values 0..31, got %r" % (k,))
        mask |= 1 << int(k)
    labels = labels.contiguous()
    B, h, w = labels.shape
    sd2 = torch.empty((B, h, w), device=labels.device, dtype=torch.int32)
    matte = torch.empty((B, h, w), device=labels.device, dtype=torch.float32)
    check(lib.ppst_label_matte(_p(labels), B, h, w, mask, int(feather), int(grow), _p(sd2), _p(matte), _stream()), "ppst_label_matte")
    return (matte, sd2) if want_distance else matte


def _paste_out(photo_u8, out, who):
    """the ``out`` rule of the pastes -> (the tensor the kernel reads, the one it writes): None clones the photo, the photo itself
    works in place, any other contiguous uint8 tensor of its shape is filled with the photo first"""
    if out is None:
        out = photo_u8.clone(memory_format=torch.contiguous_format)
        return out, out                                       # (a pixel reads only its own bytes: in place is the cloned form)
    if out is photo_u8:
        if not out.is_contiguous():
            raise RuntimeError("%s in place needs a contiguous photo" % who)
        return out, out
    if not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.shape != photo_u8.shape or not out.is_contiguous() \
            or out.device != photo_u8.device:
        raise RuntimeError("%s: out must be a contiguous uint8 tensor of the photo's shape on its device" % who)
    out.copy_(photo_u8)
    return out, out


def _paste(who, coeffs, photo_u8, xf, feather, out, extra=None, want_weight=False):
    """The one body of the pastes (csrc/guided_filter.hip gf_paste<>).  ``extra``: None, or (tensor, what, planes) of the matte
    form -- planes () for a matte plane (B,n,n), (4,) for guided-matte coefficients (B,4,n,n), the form with a weight output."""
    _need_cuda(who, "CUDA float32 coefficients", torch.float32, coeffs)
    _need_cuda(who, "a CUDA uint8 photo", torch.uint8, photo_u8)
    _need_shapes(who, "coefficients (B,12,n,n) and a photo (B,H,W,3) of one batch",
                 _is_coeffs(coeffs) and coeffs.shape[2] == coeffs.shape[3] and _is_image(photo_u8) and photo_u8.shape[0] == coeffs.shape[0],
                 coeffs, photo_u8)
    B, _, n, _ = coeffs.shape
    _, H, W, _ = photo_u8.shape
    if extra is not None:
        m, what, planes = extra
        m = _need_match(who, what, m, (B,) + planes + (n, n), photo_u8, "photo")
    photo_u8, out = _paste_out(photo_u8, out, who)
    host, dev = _crop_transforms(xf, B, out.device, who)
    coeffs = coeffs.contiguous()
    geom = (B, H, W, _p(host), _p(dev), int(feather), _stream())
    if extra is None:
        check(lib.ppst_guided_filter_paste(_p(coeffs), n, _p(photo_u8), _p(out), *geom), "ppst_guided_filter_paste")
        return out
    if not planes:
        check(lib.ppst_guided_filter_paste_matte(_p(coeffs), _p(m), n, _p(photo_u8), _p(out), *geom), "ppst_guided_filter_paste_matte")
        return out
    weight = torch.zeros((B, H, W), device=out.device, dtype=torch.uint8) if want_weight else None
    check(lib.ppst_guided_filter_paste_gmatte(_p(coeffs), _p(m), n, _p(photo_u8), _p(out), _p(weight), *geom),
          "ppst_guided_filter_paste_gmatte")
    return (out, weight) if want_weight else out


def guided_filter_paste(coeffs, photo_u8, xf, feather=0, out=None, matte=None):
    """coeffs (B,12,n,n) fp32 (``guided_filter_coeffs`` of the crops ``extract_similarity`` took), photo (B,H,W,3) uint8, the same
    crop transforms -> uint8 (B,H,W,3): inside each crop square the photo's own pixels re-coloured by the bilinearly interpolated
    coefficients, blended towards the photo over ``feather`` crop pixels from the square's edge (0 <= feather <= n/2; 0: a hard
    edge); every byte outside the square is the photo's.  One launch over the tiles of the squares' bounding boxes.  ``out``:
    None clones the photo first; ``out=photo_u8`` works in place; any other contiguous uint8 tensor of the photo's shape is
    filled with the photo first.  ``matte``: fp32 (B,n,n) on the photo's device, in the crop's frame (``label_matte``): the blend
    weight is the edge feather times the matte sampled like the coefficients, and pixels of weight 0 keep the photo's byte (the
    caller keeps its values in [0, 1]); None: no matte."""
    return _paste("guided_filter_paste", coeffs, photo_u8, xf, feather, out,
                  None if matte is None else (matte, "a float32 matte (B,n,n)", ()))


def guided_matte_coeffs(guide_u8, matte, r=8, eps=(0.01 * 255) ** 2):
    """guide (B,h,w,3) uint8, matte (B,h,w) fp32 on its device -> (B,4,h,w) fp32: the mean coefficient planes (mean a_0..2, mean b)
    of the colour guided filter with the matte as its one source channel, quantised to rint(255 clamp(m, 0, 1)) on load (He et
    al.'s guided feathering; ppst_guided_matte_coeffs in include/ppst_hip.h).  Bit-equal to planes 0..3 of
    ``guided_filter_coeffs`` on the replicated source, through 13 of its 21 moment planes and 4 of its 12 coefficient planes; the
    radius rule is ``guided_filter_coeffs``'."""
    _need_cuda("guided_matte_coeffs", "a CUDA uint8 guide", torch.uint8, guide_u8)
    _need_shapes("guided_matte_coeffs", "a guide (B,h,w,3)", _is_image(guide_u8), guide_u8)
    B, h, w, _ = guide_u8.shape
    matte = _need_match("guided_matte_coeffs", "a float32 matte (B,h,w)", matte, (B, h, w), guide_u8, "guide")
    guide_u8 = guide_u8.contiguous()
    ws = torch.empty(lib.ppst_guided_matte_ws(B, h, w), device=guide_u8.device, dtype=torch.uint8)
    mcoeffs = torch.empty((B, 4, h, w), device=guide_u8.device, dtype=torch.float32)
    check(lib.ppst_guided_matte_coeffs(_p(guide_u8), _p(matte), _p(mcoeffs), B, h, w, int(r), float(eps), _p(ws), _stream()),
          "ppst_guided_matte_coeffs")
    return mcoeffs


def guided_filter_paste_gmatte(coeffs, mcoeffs, photo_u8, xf, feather=0, out=None, want_weight=False):
    """``guided_filter_paste`` through a guided matte: ``mcoeffs`` fp32 (B,4,n,n) on the photo's device (``guided_matte_coeffs``
    of the crop) are sampled like the 12 colour planes and evaluated on the photo's own pixel, m^ = clamp((a . I + b) / 255, 0, 1),
    so the matte follows the photo's edges; the blend weight is the edge feather times m^, and pixels of weight 0 keep the photo's
    byte.  ``out`` as in ``guided_filter_paste``.  ``want_weight``: also the weight rint(255 g) as uint8 (B,H,W), 0 outside the
    square."""
    return _paste("guided_filter_paste_gmatte", coeffs, photo_u8, xf, feather, out,
                  (mcoeffs, "float32 matte coefficients (B,4,n,n)", (4,)), want_weight)


def _encode(name, u8, limits, geom=(), settings=()):
    """What png_encode and jpeg_encode do: the slots from the library's bound, the workspace from torch's allocator, one call.
    ``geom``: the codec's arguments behind (H, W, C) of its bound and workspace; ``settings``: those of its encode call."""
    if not isinstance(u8, torch.Tensor) or not u8.is_cuda or u8.dtype != torch.uint8 or u8.dim() != 4:
        raise RuntimeError("%s_encode needs a CUDA uint8 (B,H,W,C) tensor (no CPU fallback)" % name)
    u8 = u8.contiguous()
    B, H, W, C = u8.shape
    bound = getattr(lib, "ppst_%s_bound" % name)(H, W, C, *geom)
    if bound < 0:
        raise RuntimeError("%s_encode: unsupported image shape %s (%s)" % (name, tuple(u8.shape), limits))
    files = torch.empty((B, bound), device=u8.device, dtype=torch.uint8)
    sizes = torch.empty((B,), device=u8.device, dtype=torch.int64)
    work = torch.empty(getattr(lib, "ppst_%s_ws" % name)(B, H, W, C, *geom), device=u8.device, dtype=torch.uint8)
    fn = "ppst_%s_encode" % name
    check(getattr(lib, fn)(_p(u8), _p(files), _p(sizes), B, H, W, C, *settings, _p(work), _stream()), fn)
    return files, sizes


def png_encode(u8):
    """(B,H,W,C) uint8 on the device, C = 1 or 3 -> (files (B, bound) uint8, sizes (B,) int64), both on the device: file i is
    files[i, :sizes[i]] (csrc/png.hip).  The workspace comes from torch's allocator; nothing synchronises the host."""
    return _encode("png", u8, "C must be 1 or 3")


JPEG_SUBSAMPLING = {"4:4:4": 0, "4:2:0": 2}        # PPST_JPEG_444 / PPST_JPEG_420 (Pillow's numbers)


def check_jpeg_settings(quality, subsampling):
    """ValueError unless quality is an integer 1 .. 100 and subsampling "4:4:4" or "4:2:0"; -> the library's subsampling number."""
    if isinstance(quality, bool) or not isinstance(quality, int) or not 1 <= quality <= 100:
        raise ValueError("JPEG quality must be an integer 1 .. 100, not %r" % (quality,))
    if not isinstance(subsampling, str) or subsampling not in JPEG_SUBSAMPLING:
        raise ValueError("JPEG subsampling must be one of %s, not %r" % (tuple(JPEG_SUBSAMPLING), subsampling))
    return JPEG_SUBSAMPLING[subsampling]


def jpeg_encode(u8, quality=90, subsampling="4:2:0"):
    """(B,H,W,C) uint8 on the device, C = 1 (grey) or 3 (RGB) -> (files (B, bound) uint8, sizes (B,) int64), both on the device:
    file i is files[i, :sizes[i]], a baseline JPEG (csrc/jpeg.hip; the format: include/ppst_hip.h).  The workspace comes from
    torch's allocator; nothing synchronises the host."""
    ss = check_jpeg_settings(quality, subsampling)
    return _encode("jpeg", u8, "C must be 1 or 3, H and W at most 65535", (ss,), (quality, ss))


def jpeg_parse(blob):
    """bytes of a JPEG file -> (ppst_jpeg_parse's return code, the descriptor it filled).  Host code: no GPU."""
    d = _lib.JpegDecImage()
    blob = blob if isinstance(blob, bytes) else bytes(blob)
    return lib.ppst_jpeg_parse(blob, len(blob), ctypes.byref(d)), d


def png_parse(blob):
    """bytes of a PNG file -> (ppst_png_parse's return code, the descriptor it filled, its span table: a ctypes array of
    ``nspans`` PngSpan).  Host code: no GPU.  The span array is sized by a first call and, when the file has more chunks than
    that, by the count the parser leaves."""
    blob = blob if isinstance(blob, bytes) else bytes(blob)
    d = _lib.PngDecImage()
    cap = 16
    while True:
        spans = (_lib.PngSpan * cap)()
        rc = lib.ppst_png_parse(blob, len(blob), ctypes.byref(d), spans, cap)
        if rc != _lib.PNG_E_SPANS:
            return rc, d, spans
        cap = d.nspans


class _DecodeCall:
    """One batched decode, prepared: the files parsed and packed into one pinned buffer with their descriptors (and, where the
    format has them, span tables) behind them, one host-to-device copy, output / status / workspace from torch's allocator.
    ``launch()`` runs the kernels (again and again: tests/jpeg_decode_time.py and tests/png_decode_time.py time them alone).
    A format supplies its descriptor type ``Desc`` (and ``Span``; None: no span tables), the two library functions ``lib_ws`` and
    ``lib_decode``, its texts (``name``, ``refusals``, ``parsed_what``, ``ws_refused``) and the methods ``parse`` (blob -> (rc,
    descriptor, spans)), ``channels`` and ``set_flags``; ``flags`` are its keyword flags."""
    Span = None

    def __init__(self, blobs, mirror, subseq_words, dev, parsed=None, **flags):
        blobs = [b if isinstance(b, bytes) else bytes(b) for b in blobs]
        B = self.B = len(blobs)
        if mirror is not None and len(mirror) != B:
            raise ValueError("mirror must be None or one flag per file")
        if parsed is not None and len(parsed) != B:
            raise ValueError("parsed must be None or one %s per file" % self.parsed_what)
        self.subseq_words, self.dev, self.flags = subseq_words, dev, flags
        self.check_flags()
        descs = self.descs = (self.Desc * max(B, 1))()
        tables = []
        file_off, out_off, span_off = 0, 0, 0
        for i, blob in enumerate(blobs):
            if parsed is not None:
                d0, spans = parsed[i] if self.Span else (parsed[i], None)
            else:
                rc, d0, spans = self.parse(blob)
                if rc != 0:
                    raise ValueError("%s_decode: file %d: %s" % (self.name, i, self.refusals.get(rc, "error %d" % rc)))
            descs[i] = d0                                        # (a copy: the caller's descriptor keeps its own fields)
            d = descs[i]
            if self.Span:
                if d.file_len != len(blob) or d.nspans < 1 or len(spans) < d.nspans:
                    raise ValueError("%s_decode: file %d: the descriptor is not this file's" % (self.name, i))
                tables.append(spans)
                d.span_off = span_off
                span_off += d.nspans
            d.file_off, d.out_off = file_off, out_off
            d.mirror = int(bool(mirror[i])) if mirror is not None else 0
            self.set_flags(d, i)
            file_off += (len(blob) + 15) & ~15
            out_off += (d.H * d.W * self.channels(d) + 15) & ~15
        self.nbytes, self.out_bytes = file_off, out_off
        self.status = torch.zeros((B,), device=dev, dtype=torch.int32)
        if B == 0:
            return
        ws = self.lib_ws(descs, B, subseq_words)
        if ws < 0:
            raise ValueError(self.ws_refused(ws))
        nd, span_size = ctypes.sizeof(self.Desc) * B, ctypes.sizeof(self.Span) if self.Span else 0
        ns = (span_off * span_size + 15) & ~15
        host = torch.empty((file_off + nd + ns,), dtype=torch.uint8).pin_memory()
        hv = host.numpy()
        for i, blob in enumerate(blobs):
            hv[descs[i].file_off:descs[i].file_off + len(blob)] = memoryview(blob)
        ctypes.memmove(host.data_ptr() + file_off, ctypes.addressof(descs), nd)       # descriptors and spans ride behind the files
        for d, spans in zip(descs, tables):
            ctypes.memmove(host.data_ptr() + file_off + nd + d.span_off * span_size, ctypes.addressof(spans), d.nspans * span_size)
        # (torch's caching host allocator keeps a pinned block from reuse until the copies recorded on it are done)
        onchip = host.to(dev, non_blocking=True)
        self.packed, self.ddesc, self.dspans = onchip[:file_off], onchip[file_off:file_off + nd], onchip[file_off + nd:]
        self.out = torch.empty((out_off,), device=dev, dtype=torch.uint8)
        self.work = torch.empty((ws,), device=dev, dtype=torch.uint8)

    def check_flags(self):
        pass

    def launch(self):
        if self.B:
            tabs = (_p(self.dspans),) if self.Span else ()
            with torch.cuda.device(self.dev):
                check(self.lib_decode(_p(self.packed), self.nbytes, self.descs, _p(self.ddesc), *tabs, _p(self.out), self.out_bytes,
                                      _p(self.status), self.B, self.subseq_words, _p(self.work), _stream()), "ppst_%s_decode" % self.name)
        return self

    def views(self):
        out = []
        for i in range(self.B):
            d = self.descs[i]
            C = self.channels(d)
            out.append(self.out[d.out_off:d.out_off + d.H * d.W * C].view(d.H, d.W, C))
        return out

    def rounds(self):
        return self.work[:4 * self.B].view(torch.int32).clone() if self.B else self.status.clone()

    @classmethod
    def run(cls, blobs, mirror, subseq_words, device, parsed, rounds, **flags):
        """the body of jpeg_decode / png_decode"""
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("%s_decode needs a CUDA (HIP) device (no CPU fallback)" % cls.name)
        call = cls(blobs, mirror, subseq_words, dev, parsed, **flags).launch()
        return (call.views(), call.status, call.rounds()) if rounds else (call.views(), call.status)


class _JpegDecodeCall(_DecodeCall):
    name, Desc, refusals, parsed_what = "jpeg", _lib.JpegDecImage, _lib.JPEG_REFUSALS, "descriptor"
    lib_ws, lib_decode = lib.ppst_jpeg_decode_ws, lib.ppst_jpeg_decode

    def ws_refused(self, ws):
        return "jpeg_decode: subseq_words must be 0 (the default) or 2 .. 65536, got %r" % (self.subseq_words,)

    @staticmethod
    def parse(blob):
        return jpeg_parse(blob) + (None,)

    def set_flags(self, d, i):
        d.expand_grey = int(bool(self.flags["expand_grey"]))

    @staticmethod
    def channels(d):
        return 3 if d.ncomp == 3 or d.expand_grey else 1


def jpeg_decode(blobs, expand_grey=False, mirror=None, subseq_words=0, device="cuda", rounds=False, parsed=None):
    """blobs: B baseline JPEG files (bytes) of any sizes and samplings -> (list of B (H,W,C) uint8 views of one device buffer,
    status (B,) int32 on the device; 0 = decoded: include/ppst_hip.h, csrc/jpeg_decode.hip).  C = 1 for a grey file, 3 for a colour
    one and for a grey one with ``expand_grey``; ``mirror``: None or B flags, image i comes out with its columns reversed.  The files
    and their descriptors are packed into one pinned buffer: one host-to-device copy.  A file the parser refuses raises
    ValueError with its reason.  ``rounds``: also return the (B,) int32 tensor of rounds the subsequence iteration took.
    ``parsed``: the files' descriptors where the caller has them already (``jpeg_parse`` returned 0 for each): nothing is parsed twice."""
    return _JpegDecodeCall.run(blobs, mirror, subseq_words, device, parsed, rounds, expand_grey=expand_grey)


class _PngDecodeCall(_DecodeCall):
    name, Desc, Span, refusals, parsed_what = "png", _lib.PngDecImage, _lib.PngSpan, _lib.PNG_REFUSALS, "(descriptor, spans) pair"
    lib_ws, lib_decode = lib.ppst_png_decode_ws, lib.ppst_png_decode
    parse = staticmethod(png_parse)

    def ws_refused(self, ws):
        return "png_decode: the library refused the descriptors (%d)" % ws

    def check_flags(self):
        for flag in self.flags.values():
            if isinstance(flag, (list, tuple)) and len(flag) != self.B:
                raise ValueError("expand_grey and drop_alpha must be one flag, or one flag per file")
        sw = self.subseq_words
        if isinstance(sw, bool) or not isinstance(sw, int) or not (sw == 0 or 2 <= sw <= 128):
            raise ValueError("png_decode: subseq_words must be 0 (the default) or 2 .. 128, got %r" % (sw,))

    def set_flags(self, d, i):
        """each one flag for the batch, or a list of one per file"""
        for name, flag in self.flags.items():
            setattr(d, name, int(bool(flag[i] if isinstance(flag, (list, tuple)) else flag)))

    @staticmethod
    def channels(d):
        return (3 if d.expand_grey else 1) if d.channels == 1 else (3 if d.channels == 3 or d.drop_alpha else 4)


def png_decode(blobs, expand_grey=False, drop_alpha=False, mirror=None, device="cuda", parsed=None, subseq_words=0, rounds=False):
    """blobs: B PNG files (bytes) of any sizes, 8-bit grey / RGB / RGBA -> (list of B (H,W,C) uint8 views of one device buffer,
    status (B,) int32 on the device; 0 = decoded: include/ppst_hip.h, csrc/png_decode.hip).  C = 1, 3 or 4 as the file has it;
    ``expand_grey``: a grey file comes out with three equal channels; ``drop_alpha``: an RGBA file comes out as RGB (each one
    flag, or a list of B flags); ``mirror``: None or B flags, image i comes out with its columns reversed.  The files, descriptors and span tables are packed into one
    pinned buffer: one host-to-device copy.  A file the parser refuses raises ValueError with its reason.  ``parsed``: the
    files' (descriptor, spans) pairs where the caller has them already (``png_parse`` returned 0 for each).  ``subseq_words``:
    32-bit words per subsequence of the parallel inflate, 0 = the default.  ``rounds``: also return the (B,) int32 tensor of
    rounds the subsequence iteration took."""
    return _PngDecodeCall.run(blobs, mirror, subseq_words, device, parsed, rounds, expand_grey=expand_grey, drop_alpha=drop_alpha)


# The table from file extension to codec: the one place that decides which coder takes a file.  ``parse``: blob -> (return
# code, what the codec's ``decode`` takes as an entry of ``parsed``, the descriptor with the file's H and W); ``rgb``: the
# decode flags that give what Pillow's convert("RGB") gives.
Codec = collections.namedtuple("Codec", "name extensions parse decode rgb")


def _jpeg_entry(blob):
    rc, d = jpeg_parse(blob)
    return rc, d, d


def _png_entry(blob):
    rc, d, spans = png_parse(blob)
    return rc, (d, spans), d


JPEG = Codec("jpeg", (".jpg", ".jpeg"), _jpeg_entry, jpeg_decode, {"expand_grey": True})
PNG = Codec("png", (".png",), _png_entry, png_decode, {"expand_grey": True, "drop_alpha": True})
CODECS = (JPEG, PNG)                                # (batched calls are made in this order)


def codec_for(path):
    """the codec whose device decoder takes a file of this name, None: the host's business"""
    return next((c for c in CODECS if path.lower().endswith(c.extensions)), None)


def resample_f32(x, out_h, out_w, clamp=None):
    """x (..., H, W) float32 on the device -> (..., out_h, out_w): Pillow's antialiased bicubic on every plane, both axes in one
    launch (ppst_resample_f32; the fp32 weight tables are imageio.resample_tables_f32).  ``clamp`` = (lo, hi) or None."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32 or x.dim() < 2:
        raise RuntimeError("resample_f32 needs a CUDA float32 (..., H, W) tensor (no CPU fallback)")
    from . import imageio
    out_h, out_w = int(out_h), int(out_w)
    if out_h <= 0 or out_w <= 0:
        raise ValueError("resample_f32: output size must be positive, got %d x %d" % (out_h, out_w))
    x = x.contiguous()
    H, W = x.shape[-2:]
    planes = x.numel() // (H * W) if H * W else 0
    kh, bh, ch = imageio.resample_tables_f32(W, out_w, x.device) if W != out_w else (1, None, None)
    kv, bv, cv = imageio.resample_tables_f32(H, out_h, x.device) if H != out_h else (1, None, None)
    lo, hi = (float(clamp[0]), float(clamp[1])) if clamp is not None else (0.0, 0.0)
    y = torch.empty(tuple(x.shape[:-2]) + (out_h, out_w), device=x.device, dtype=torch.float32)
    check(lib.ppst_resample_f32(_p(x), _p(y), planes, H, W, out_h, out_w, _p(bh), _p(ch), kh, _p(bv), _p(cv), kv,
                                int(clamp is not None), lo, hi, _stream()), "ppst_resample_f32")
    return y


# ------------------------------------------------------- LPIPS-AlexNet metric ----
LPIPS_CHANNELS = (64, 192, 384, 256, 256)


def lpips_pack(weights, biases, lins, shift, scale):
    """Five conv weights (torch layout), biases and lin vectors + the scaling layer's shift / scale, all fp32 on the device ->
    the packed forward + input-gradient weights of csrc/lpips.hip (once per weight set: they are frozen)."""
    ts = list(weights) + list(biases) + list(lins) + [shift, scale]
    for t in ts:
        _chk(t, "lpips weight")
        if not t.is_contiguous():
            raise RuntimeError("lpips_pack needs contiguous tensors")
    arr = lambda seq: (ctypes.c_void_p * 5)(*[t.data_ptr() for t in seq])
    pack = torch.empty(lib.ppst_lpips_pack_floats(), device=shift.device, dtype=torch.float32)
    check(lib.ppst_lpips_pack(arr(weights), arr(biases), arr(lins), _p(shift), _p(scale), _p(pack), _stream()), "ppst_lpips_pack")
    return pack


def lpips_dims(H, W):
    """[(h, w)] of relu1..relu5 for an H x W image; raises below 31 pixels a side."""
    hw = (ctypes.c_int * 10)()
    check(lib.ppst_lpips_dims(H, W, hw), "ppst_lpips_dims (images of at least 31 x 31)")
    return [(hw[2 * l], hw[2 * l + 1]) for l in range(5)]


def _lpips_img(t, name):
    _chk(t, name)
    if t.dim() != 4 or t.shape[1] != 3:
        raise RuntimeError("%s must be (B, 3, H, W), got %s" % (name, tuple(t.shape)))
    return (ctypes.c_int64 * 4)(*t.stride())


def lpips_trunk(pack, a, b=None):
    """a (and b) (B,3,H,W) fp32, any strides, as one batch through scaling layer + AlexNet trunk -> the workspace holding the five
    post-ReLU maps (channels-last), the pooled maps and the pools' arg-max."""
    sa = _lpips_img(a, "lpips input")
    na, _, H, W = a.shape
    nb, sb = 0, None
    if b is not None:
        sb = _lpips_img(b, "lpips input")
        if b.shape != a.shape:
            raise RuntimeError("lpips inputs differ in shape: %s and %s" % (tuple(a.shape), tuple(b.shape)))
        nb = na
    nbytes = lib.ppst_lpips_ws(na + nb, H, W)
    if nbytes < 0:
        raise RuntimeError("lpips: unsupported image size %d x %d (at least 31 x 31)" % (H, W))
    ws = torch.empty(nbytes, device=a.device, dtype=torch.uint8)
    check(lib.ppst_lpips_trunk(_p(pack), _p(a), sa, na, _p(b), sb, nb, H, W, _p(ws), _stream()), "ppst_lpips_trunk")
    return ws


def lpips_feature(ws, n, H, W, layer):
    h, w = lpips_dims(H, W)[layer]
    out = torch.empty((n, LPIPS_CHANNELS[layer], h, w), device=ws.device, dtype=torch.float32)
    check(lib.ppst_lpips_feature(_p(ws), n, H, W, layer, _p(out), _stream()), "ppst_lpips_feature")
    return out


def lpips_forward(pack, a, b):
    """-> (out (B,1,1,1), workspace for lpips_backward)"""
    ws = lpips_trunk(pack, a, b)
    B, _, H, W = a.shape
    out = torch.empty((B, 1, 1, 1), device=a.device, dtype=torch.float32)
    check(lib.ppst_lpips_tail(_p(pack), _p(ws), B, H, W, _p(out), _stream()), "ppst_lpips_tail")
    return out, ws


def lpips_backward(pack, ws, gout, B, H, W, need_a, need_b):
    """input gradients (ga, gb) (None where not asked for) of sum_b gout[b] * out[b]"""
    _chk(gout, "lpips grad_output")
    which = (1 if need_a else 0) | (2 if need_b else 0)
    if which == 0:
        return None, None
    gout = gout.reshape(-1).contiguous()
    if gout.numel() != B:
        raise RuntimeError("lpips grad_output must have %d elements" % B)
    ga = torch.empty((B, 3, H, W), device=ws.device, dtype=torch.float32) if need_a else None
    gb = torch.empty((B, 3, H, W), device=ws.device, dtype=torch.float32) if need_b else None
    bws = torch.empty(lib.ppst_lpips_bwd_ws(B, H, W, which), device=ws.device, dtype=torch.uint8)
    check(lib.ppst_lpips_backward(_p(pack), _p(ws), _p(gout), B, H, W, which, _p(ga), _p(gb), _p(bws), _stream()), "ppst_lpips_backward")
    return ga, gb


# ------------------------------------------------------ image-quality metrics ----
MS_SSIM_SCALES = 5
MS_SSIM_MIN_SIDE = 11 << (MS_SSIM_SCALES - 1)        # 176: the fifth scale must still hold the 11-tap window


def _metric_img(t, name):
    """-> (u8 flag, (B, C, H, W), the four element strides (n, c, y, x)): fp32 (B, C, H, W) in any layout, or uint8 (B, H, W, C)"""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError("%s must be a CUDA (HIP) tensor (no CPU fallback)" % name)
    if t.dim() != 4:
        raise RuntimeError("%s must have four dimensions, got %s" % (name, tuple(t.shape)))
    if t.dtype == torch.uint8:
        B, H, W, C = t.shape
        sn, sy, sx, sc = t.stride()
        return 1, (B, C, H, W), (ctypes.c_int64 * 4)(sn, sc, sy, sx)
    if t.dtype != torch.float32:
        raise RuntimeError("%s must be float32 (B, C, H, W) or uint8 (B, H, W, C), got %s" % (name, t.dtype))
    return 0, tuple(t.shape), (ctypes.c_int64 * 4)(*t.stride())


def _metric_pair(a, b, what):
    ua, shape, sa = _metric_img(a, what + " input")
    ub, shape_b, sb = _metric_img(b, what + " input")
    if ua != ub or shape != shape_b:
        raise RuntimeError("%s inputs differ: %s %s and %s %s" % (what, a.dtype, tuple(a.shape), b.dtype, tuple(b.shape)))
    return ua, shape, sa, sb


def default_data_range(t, data_range=None):
    """2.0 for float tensors (the model's [-1, 1]), 255 for uint8"""
    if data_range is None:
        return 255.0 if t.dtype == torch.uint8 else 2.0
    if not float(data_range) > 0.0:
        raise ValueError("data_range must be positive, got %r" % (data_range,))
    return float(data_range)


def ssim_forward(a, b, data_range=None):
    """SSIM (11-tap Gaussian window, sigma 1.5, valid) of two fp32 (B, C, H, W) batches in any layout, or two uint8 (B, H, W, C)
    ones -> (per-image SSIM (B,), per-(image, channel) mean ssim (B, C), mean cs (B, C)); csrc/ssim.hip."""
    u8, (B, C, H, W), sa, sb = _metric_pair(a, b, "ssim")
    L = default_data_range(a, data_range)
    nbytes = lib.ppst_ssim_ws(B, C, H, W)
    if nbytes < 0:
        raise ValueError("ssim: unsupported shape %s (H and W of at least 11, at least one channel)" % ((B, C, H, W),))
    ws = torch.empty(nbytes, device=a.device, dtype=torch.uint8)
    out = torch.empty((B,), device=a.device, dtype=torch.float32)
    s_bc = torch.empty((B, C), device=a.device, dtype=torch.float32)
    cs_bc = torch.empty((B, C), device=a.device, dtype=torch.float32)
    check(lib.ppst_ssim_forward(_p(a), sa, _p(b), sb, u8, B, C, H, W, L, _p(out), _p(s_bc), _p(cs_bc), _p(ws), _stream()), "ppst_ssim_forward")
    return out, s_bc, cs_bc


def ssim_backward(a, b, gout, data_range=None):
    """d(sum_b gout[b] * ssim[b]) / d a, (B, C, H, W) contiguous fp32; fp32 inputs only"""
    u8, (B, C, H, W), sa, sb = _metric_pair(a, b, "ssim")
    if u8:
        raise RuntimeError("ssim_backward: uint8 images are forward only")
    _chk(gout, "ssim grad_output")
    gout = gout.reshape(-1).contiguous()
    if gout.numel() != B:
        raise RuntimeError("ssim grad_output must have %d elements" % B)
    L = default_data_range(a, data_range)
    grad = torch.empty((B, C, H, W), device=a.device, dtype=torch.float32)
    check(lib.ppst_ssim_backward(_p(a), sa, _p(b), sb, _p(gout), B, C, H, W, L, _p(grad), _stream()), "ppst_ssim_backward")
    return grad


def pool2x2(x):
    """the 2 x 2 mean with stride 2 between two MS-SSIM scales (F.avg_pool2d(x, 2)): fp32 (B, C, H, W) in any layout or uint8
    (B, H, W, C) -> contiguous fp32 (B, C, H // 2, W // 2), in the input's units"""
    u8, (B, C, H, W), sx = _metric_img(x, "pool2x2 input")
    out = torch.empty((B, C, H // 2, W // 2), device=x.device, dtype=torch.float32)
    check(lib.ppst_pool2x2(_p(x), sx, u8, B, C, H, W, _p(out), _stream()), "ppst_pool2x2")
    return out


def ms_ssim_forward(a, b, data_range=None):
    """five-scale MS-SSIM -> (B,); min(H, W) >= 176"""
    u8, (B, C, H, W), _, _ = _metric_pair(a, b, "ms_ssim")
    if min(H, W) < MS_SSIM_MIN_SIDE:
        raise ValueError("ms_ssim needs images of at least %d x %d (five scales, the last one must still hold the 11-tap window), "
                         "got %d x %d" % (MS_SSIM_MIN_SIDE, MS_SSIM_MIN_SIDE, H, W))
    L = default_data_range(a, data_range)
    vals = torch.empty((MS_SSIM_SCALES, B, C), device=a.device, dtype=torch.float32)
    for j in range(MS_SSIM_SCALES):
        _, s_bc, cs_bc = ssim_forward(a, b, L)
        vals[j].copy_(s_bc if j == MS_SSIM_SCALES - 1 else cs_bc)
        if j < MS_SSIM_SCALES - 1:
            a, b = pool2x2(a), pool2x2(b)
    out = torch.empty((B,), device=vals.device, dtype=torch.float32)
    check(lib.ppst_msssim_combine(_p(vals), B, C, _p(out), _stream()), "ppst_msssim_combine")
    return out


def sqerr(a, b, data_range=None):
    """-> (B, 3) fp32: per image mean (a - b)^2, mean |a - b|, PSNR = 10 log10(L^2 / mse) (+inf for equal images)"""
    u8, (B, C, H, W), sa, sb = _metric_pair(a, b, "sqerr")
    L = default_data_range(a, data_range)
    nbytes = lib.ppst_sqerr_ws(B, C, H, W)
    if nbytes < 0:
        raise ValueError("sqerr: unsupported shape %s" % ((B, C, H, W),))
    ws = torch.empty(nbytes, device=a.device, dtype=torch.uint8)
    out = torch.empty((B, 3), device=a.device, dtype=torch.float32)
    check(lib.ppst_sqerr(_p(a), sa, _p(b), sb, u8, B, C, H, W, L, _p(out), _p(ws), _stream()), "ppst_sqerr")
    return out


# --------------------------------------------------------- colour statistics ----
COLOUR_MAX_REGIONS, COLOUR_MAX_DIRS, COLOUR_MAX_PIXELS = 4, 16, 1 << 22
COLOUR_AXES = ((4096, 0, 0), (0, 4096, 0), (0, 0, 4096))


def _u8_dev(t, name, dims):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError("%s must be a CUDA (HIP) tensor (no CPU fallback)" % name)
    if t.dtype != torch.uint8 or t.dim() != dims:
        raise RuntimeError("%s must be uint8 with %d dimensions, got %s %s" % (name, dims, t.dtype, tuple(t.shape)))


def colour_stats(u8, labels=None, regions=1, dirs=None):
    """Per-image, per-region colour statistics (csrc/colour_stats.hip).  ``u8``: (B, H, W, 3) uint8 whose pixels are contiguous
    (any batch and row stride: a crop view is read in place, anything else is copied); ``labels``: (B, H, W) uint8 or None (one
    region); a label >= ``regions`` belongs to no region; ``dirs``: (P, 3) int16 rows with sum |d| <= 4096 (default: the three
    channel axes).  -> (hist (B, R, P, 256) int32 -- the kernel's uint32 counts, all below 2^22 --, count (B, R) int32,
    lab_mean (B, R, 3) float64, lab_cov (B, R, 6) float64: LL, La, Lb, aa, ab, bb)."""
    _u8_dev(u8, "colour_stats images", 4)
    B, H, W, C = u8.shape
    if C != 3:
        raise RuntimeError("colour_stats images must be (B, H, W, 3), got %s" % (tuple(u8.shape),))
    if u8.stride(3) != 1 or (W > 1 and u8.stride(2) != 3):      # (the stride of a dimension of size 1 says nothing)
        u8 = u8.contiguous()
    if labels is not None:
        _u8_dev(labels, "colour_stats labels", 3)
        if tuple(labels.shape) != (B, H, W) or labels.device != u8.device:
            raise RuntimeError("colour_stats labels must be (B, H, W) = %s on the images' device, got %s" % ((B, H, W), tuple(labels.shape)))
        if W > 1 and labels.stride(2) != 1:
            labels = labels.contiguous()
    d = torch.tensor(COLOUR_AXES, dtype=torch.int16) if dirs is None else torch.as_tensor(dirs).detach().cpu()
    if d.dtype != torch.int16 or d.dim() != 2 or d.shape[1] != 3:
        raise ValueError("colour_stats directions must be int16 (P, 3), got %s %s" % (d.dtype, tuple(d.shape)))
    d = d.contiguous()
    R, P = int(regions), int(d.shape[0])
    nbytes = lib.ppst_colour_stats_ws(B, H, W)
    if nbytes < 0 or not 1 <= R <= COLOUR_MAX_REGIONS or not 1 <= P <= COLOUR_MAX_DIRS or int(d.to(torch.int32).abs().sum(1).max()) > 4096:
        raise ValueError("colour_stats: H * W <= 2^22, 1 .. 4 regions, 1 .. 16 directions with sum |d| <= 4096 each; got %s, %d regions, "
                         "directions %s" % ((B, H, W), R, tuple(d.shape)))
    dev = u8.device
    hist = torch.empty((B, R, P, 256), device=dev, dtype=torch.int32)
    count = torch.empty((B, R), device=dev, dtype=torch.int32)
    mean = torch.empty((B, R, 3), device=dev, dtype=torch.float64)
    cov = torch.empty((B, R, 6), device=dev, dtype=torch.float64)
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    dptr = ctypes.cast(ctypes.c_void_p(d.data_ptr()), ctypes.POINTER(ctypes.c_int16))
    check(lib.ppst_colour_stats(_p(u8), u8.stride(0), u8.stride(1), 3, _p(labels), 0 if labels is None else labels.stride(0),
                                0 if labels is None else labels.stride(1), B, H, W, R, dptr, P, _p(hist), _p(count), _p(mean), _p(cov),
                                _p(ws), _stream()), "ppst_colour_stats")
    return hist, count, mean, cov


def hist_w1(hist_a, hist_b, pairs):
    """The exact 1-Wasserstein numerators between histograms ``hist_a[i]`` and ``hist_b[j]`` for every (i, j) of ``pairs`` (a
    list of index pairs or a (K, 2) integer tensor), per region and projection: (K, R, P) int64 =
    sum_v |cumA(v) nB - cumB(v) nA|; W1 in grey levels is that over nA nB (0 where a side is empty)."""
    for t, name in ((hist_a, "hist_a"), (hist_b, "hist_b")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError("hist_w1 %s must be a CUDA (HIP) tensor (no CPU fallback)" % name)
        if t.dtype != torch.int32 or t.dim() != 4 or t.shape[3] != 256:
            raise RuntimeError("hist_w1 %s must be int32 (B, R, P, 256), got %s %s" % (name, t.dtype, tuple(t.shape)))
    if hist_a.shape[1:] != hist_b.shape[1:] or hist_a.device != hist_b.device:
        raise RuntimeError("hist_w1: the two histogram tensors differ: %s and %s" % (tuple(hist_a.shape), tuple(hist_b.shape)))
    pr = torch.as_tensor(pairs).detach().cpu().reshape(-1, 2).to(torch.int64)
    K, (Ba, R, P), Bb = int(pr.shape[0]), hist_a.shape[:3], hist_b.shape[0]
    if K and (int(pr.min()) < 0 or int(pr[:, 0].max()) >= Ba or int(pr[:, 1].max()) >= Bb):
        raise ValueError("hist_w1: a pair index is outside the histograms' batches (%d and %d)" % (Ba, Bb))
    hist_a, hist_b = hist_a.contiguous(), hist_b.contiguous()
    pr = pr.to(torch.int32).contiguous().to(hist_a.device)
    num = torch.empty((K, R, P), device=hist_a.device, dtype=torch.int64)
    check(lib.ppst_hist_w1(_p(hist_a), Ba, _p(hist_b), Bb, _p(pr), K, R, P, _p(num), _stream()), "ppst_hist_w1")
    return num


# ----------------------------------------------------------- colour transfer ----
def hist_match_lut(hist_c, hist_s, pairs):
    """The exact histogram-specification tables (csrc/colour_transfer.hip; include/ppst_hip.h "colour transfer") that send the
    channel histograms ``hist_c[i]`` onto ``hist_s[j]`` for every (i, j) of ``pairs``, per region: uint8 (K, R, 3, 256).  Both
    are ``colour_stats`` histograms (B, R, P, 256) int32 whose projections 0..2 are the channel axes (``COLOUR_AXES``; the rest
    is not read).  ``LUT[v] = min{u : 2 cumS(u) nC >= (cumC(v - 1) + cumC(v)) nS}``; the identity where a side is empty."""
    for t, name in ((hist_c, "hist_c"), (hist_s, "hist_s")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError("hist_match_lut %s must be a CUDA (HIP) tensor (no CPU fallback)" % name)
        if t.dtype != torch.int32 or t.dim() != 4 or t.shape[3] != 256 or t.shape[2] < 3:
            raise RuntimeError("hist_match_lut %s must be int32 (B, R, P >= 3, 256), got %s %s" % (name, t.dtype, tuple(t.shape)))
    if hist_c.shape[1:] != hist_s.shape[1:] or hist_c.device != hist_s.device:
        raise RuntimeError("hist_match_lut: the two histogram tensors differ: %s and %s" % (tuple(hist_c.shape), tuple(hist_s.shape)))
    pr = torch.as_tensor(pairs).detach().cpu().reshape(-1, 2).to(torch.int64)
    K, (Bc, R, P), Bs = int(pr.shape[0]), hist_c.shape[:3], hist_s.shape[0]
    if K and (int(pr.min()) < 0 or int(pr[:, 0].max()) >= Bc or int(pr[:, 1].max()) >= Bs):
        raise ValueError("hist_match_lut: a pair index is outside the histograms' batches (%d and %d)" % (Bc, Bs))
    if not 1 <= R <= COLOUR_MAX_REGIONS or P > COLOUR_MAX_DIRS:
        raise ValueError("hist_match_lut: 1 .. 4 regions and 3 .. 16 projections, got %d and %d" % (R, P))
    hist_c, hist_s = hist_c.contiguous(), hist_s.contiguous()
    pr = pr.to(torch.int32).contiguous().to(hist_c.device)
    luts = torch.empty((K, R, 3, 256), device=hist_c.device, dtype=torch.uint8)
    check(lib.ppst_hist_match_lut(_p(hist_c), Bc, _p(hist_s), Bs, _p(pr), K, R, P, _p(luts), _stream()), "ppst_hist_match_lut")
    return luts


def colour_transfer_apply(u8, labels, luts=None, affine=None, weights=None, out=None):
    """One pass that re-colours ``u8`` (B, H, W, 3) uint8 (strides as ``colour_stats``: a crop view is read in place) per region
    of ``labels`` ((B, H, W) uint8, or None: one region) -> uint8 (B, H, W, 3).  Exactly one of ``luts`` (uint8 (B, R, 3, 256):
    ``out_c = LUT[label][c][in_c]``) and ``affine`` (fp32 (B, R, 12) rows (T | t): ``lab' = T lab + t`` in CIELAB, converted back
    and quantised once).  ``weights``: fp32 (B, R, H, W) >= 0, normalised per pixel in the kernel; the tables' outputs (the 12
    coefficients) are blended by them, a pixel whose weights are all 0 follows its label.  A pixel whose label is >= R keeps its
    bytes.  ``out``: a contiguous uint8 (B, H, W, 3) tensor to write to (and return)."""
    _u8_dev(u8, "colour_transfer_apply images", 4)
    B, H, W, C = u8.shape
    if C != 3:
        raise RuntimeError("colour_transfer_apply images must be (B, H, W, 3), got %s" % (tuple(u8.shape),))
    if (luts is None) == (affine is None):
        raise ValueError("colour_transfer_apply takes exactly one of luts and affine")
    maps, mode = (luts, 0) if luts is not None else (affine, 1)
    want = torch.uint8 if mode == 0 else torch.float32
    if not isinstance(maps, torch.Tensor) or not maps.is_cuda:
        raise RuntimeError("colour_transfer_apply maps must be a CUDA (HIP) tensor (no CPU fallback)")
    ok = maps.dim() == 4 and maps.shape[2:] == (3, 256) if mode == 0 else maps.dim() == 3 and maps.shape[2] == 12
    if maps.dtype != want or not ok or maps.shape[0] != B or maps.device != u8.device:
        raise RuntimeError("colour_transfer_apply: luts must be uint8 (B, R, 3, 256), affine fp32 (B, R, 12), B = %d, on the images' "
                           "device; got %s %s" % (B, maps.dtype, tuple(maps.shape)))
    R = int(maps.shape[1])
    if u8.stride(3) != 1 or (W > 1 and u8.stride(2) != 3):
        u8 = u8.contiguous()
    if labels is not None:
        _u8_dev(labels, "colour_transfer_apply labels", 3)
        if tuple(labels.shape) != (B, H, W) or labels.device != u8.device:
            raise RuntimeError("colour_transfer_apply labels must be (B, H, W) = %s on the images' device, got %s" % ((B, H, W), tuple(labels.shape)))
        if W > 1 and labels.stride(2) != 1:
            labels = labels.contiguous()
    if weights is not None:
        if not isinstance(weights, torch.Tensor) or not weights.is_cuda:
            raise RuntimeError("colour_transfer_apply weights must be a CUDA (HIP) tensor (no CPU fallback)")
        if weights.dtype != torch.float32 or tuple(weights.shape) != (B, R, H, W) or weights.device != u8.device:
            raise RuntimeError("colour_transfer_apply weights must be fp32 (B, R, H, W) = %s, got %s %s" % ((B, R, H, W), weights.dtype, tuple(weights.shape)))
        weights = weights.contiguous()
    if H < 1 or W < 1 or H * W > COLOUR_MAX_PIXELS or not 1 <= R <= COLOUR_MAX_REGIONS:
        raise ValueError("colour_transfer_apply: 1 <= H * W <= 2^22 and 1 .. 4 regions; got %s, %d regions" % ((B, H, W), R))
    if out is None:
        out = torch.empty((B, H, W, 3), device=u8.device, dtype=torch.uint8)
    else:
        _u8_dev(out, "colour_transfer_apply out", 4)
        if tuple(out.shape) != (B, H, W, 3) or not out.is_contiguous() or out.device != u8.device:
            raise RuntimeError("colour_transfer_apply out must be a contiguous (B, H, W, 3) = %s tensor on the images' device" % ((B, H, W, 3),))
    maps = maps.contiguous()
    check(lib.ppst_colour_transfer_apply(_p(u8), u8.stride(0), u8.stride(1), 3, _p(labels), 0 if labels is None else labels.stride(0),
                                         0 if labels is None else labels.stride(1), B, H, W, R, mode, _p(maps), _p(weights), _p(out),
                                         _stream()), "ppst_colour_transfer_apply")
    return out


# --------------------------------------------------------------- profiling ----
PROF_ON = {"value": False}


def prof_enable(on):
    PROF_ON["value"] = bool(on)
    check(lib.ppst_prof_enable(1 if on else 0), "ppst_prof_enable")


def prof_collect():
    """(ms, launches, flop) of the bracketed conv launches.  Raises if the event pool overflowed (the totals
    would silently miss launches)."""
    ms, n, fl = ctypes.c_double(0), ctypes.c_int64(0), ctypes.c_double(0)
    dropped = lib.ppst_prof_dropped()
    check(lib.ppst_prof_collect(ctypes.byref(ms), ctypes.byref(n), ctypes.byref(fl)), "ppst_prof_collect")
    if dropped:
        raise RuntimeError("conv profiling pool overflowed: %d launches were not timed (use fewer --steps)" % dropped)
    return ms.value, n.value, fl.value


def prof_detail():
    """list of (ms, flop, (B, tile_h, tile_w, nsteps, cout, n_groups, halo, bn)) per bracketed conv launch."""
    out = []
    i = 0
    while True:
        ms, fl = ctypes.c_double(0), ctypes.c_double(0)
        info = (ctypes.c_int * 8)()
        if lib.ppst_prof_detail(i, ctypes.byref(ms), ctypes.byref(fl), info) != 0:
            break
        out.append((ms.value, fl.value, tuple(info)))
        i += 1
    return out
