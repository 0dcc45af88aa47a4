"""Swap recipes of the reference's evaluators on the HIP model facade.

* ``simple_swap``  = evaluation/simple_swapping_evaluator.py:38-76 (one content, one
  style, list of mix alphas) -- batched: B pairs at once.
* ``swapping_grid`` = evaluation/content_style_grid_generation_evaluator.py:36-99
  (N contents x M styles, guided-filter post-process with the content as guide) in two phases:
    1. per-IMAGE passes (encode, extract_feat, Rselfcorr), computed once per image instead of once per pair and
       sharded over ranks by image (image k of the N + M belongs to rank k mod world), batched;
    2. ONE exchange: all_gather of the spatial codes (4.2 MB per content image) and of fea || Rselfcorr (8.4 MB per
       image) -- RCCL on the GPU, the only data-path collective of inference;
    3. per-PAIR passes (corrm, encode2, decode + guided filter), pair (i, j) on rank ((i * M + j) mod world), batched.
  An 8 x 8 grid on 8 ranks costs each rank 2 image passes + 8 pair passes (~5.9 TFLOP) against 16 + 64 on one GPU.
Above 512 x 512 (square, side 1024 or 1536) both recipes compute the correspondence from a 512 x 512 resample of each image and apply
it at full size (``simple_swap_full_size``; DESIGN.md "Swaps above 512^2"); the reference cannot run that.
The recipes take and return tensors.  The folder-level front ends at the end of this file (``evaluate_swap_files``,
``evaluate_grid_folder``) add what the reference's evaluators do around them: decode (PIL, a thread pool), resize + normalise
on the device (ppst_amd/imageio.py, Pillow-exact), the uint8 quantisation on the device (glue.tensor2im), PNG encode in the
thread pool (zlib releases the GIL: the encode of one batch overlaps the next batch's kernels) or -- ``png="device"`` -- on
the GPU (imageio.encode_png: the threads only write bytes), the reference's file names.  ``format="jpeg"`` writes baseline JPEG
files instead, by the same switch: Pillow on the threads, or imageio.encode_jpeg on the GPU.
"""
import contextlib
import os
import threading

import torch

from . import glue, ops


def above_code_grid(*images):
    """True when an image is larger than the 512 x 512 the 64 x 64 correspondence grid belongs to: the recipes then compute the
    correspondence from ``model.correspondence_image`` and apply it at full size."""
    from .ppst_model import CORR_SIDE
    return any(max(int(t.shape[-2]), int(t.shape[-1])) > CORR_SIDE for t in images)


def swap_codes_full_size(model, content, style):
    """``swap_codes`` above 512 x 512: spatial code and global codes at full size, the correspondence from the 512 x 512 resamples
    of both images (PPSTModel.correspondence_features); E2's warp pools every level of the full-size style pass to the 64 x 64
    grid, applies the matrix and resizes back."""
    sp, gl_c = model(content, command="encode")
    if content.shape == style.shape:
        # both 512 x 512 passes as one batch: contents, then styles (bit-identical: nothing depends on the batch size)
        B = content.shape[0]
        small = torch.cat((model(content, command="correspondence_image"), model(style, command="correspondence_image")), 0)
        fea = model(small, command="correspondence_features")
        fea_c, fea_s = fea[:B], fea[B:]
    else:
        fea_c = model(content, command="correspondence_features")
        fea_s = model(style, command="correspondence_features")
    corr = model(fea_s, fea_c, command="corrm")
    _, gl_w = model(style, corr, command="encode2")
    return sp, gl_c, gl_w


def simple_swap_full_size(model, content, style, alphas=(1.0,)):
    """``simple_swap`` above 512 x 512: the codes of ``swap_codes_full_size``, decoded at full size."""
    sp, gl_c, gl_w = swap_codes_full_size(model, content, style)
    out = {}
    for alpha in alphas:
        out[alpha] = model(sp, glue.lerp(gl_c, gl_w, alpha), target=None, command="decode")
    return out


def swap_codes(model, content, style):
    """The recipe of ``simple_swap`` up to its codes: -> (sp, gl_c, gl_w), the content's spatial code, its global codes and the
    style's warped ones; every alpha decodes from ``(sp, lerp(gl_c, gl_w, alpha))``.  Shared by ``simple_swap`` and
    ``simple_swap_native``."""
    if above_code_grid(content, style):
        return swap_codes_full_size(model, content, style)
    if content.shape == style.shape:
        # the encoder passes of the recipe (encode(content) + the E1 / E2 inside the two extract_feat_from_image) as one batch of
        # 3B images, the two generator feature passes as one of 2B: the same work, bit-identical (nothing depends on the batch size)
        B = content.shape[0]
        sp3, gl3 = model(torch.cat((content, content, style), 0), command="encode")
        sp, gl_c = sp3[:B], [g[:B] for g in gl3]
        _, fea, fea1 = model(sp3[B:], [g[B:] for g in gl3], command="extract_feat")
        fea = torch.cat((fea, model(fea1, command="Rselfcorr")), dim=1)
        fea_c, fea_s = fea[:B], fea[B:]
    else:
        sp, gl_c = model(content, command="encode")
        fea_c, fea_c1 = model(content, command="extract_feat_from_image")
        fea_s, fea_s1 = model(style, command="extract_feat_from_image")
        fea_c = torch.cat((fea_c, model(fea_c1, command="Rselfcorr")), dim=1)
        fea_s = torch.cat((fea_s, model(fea_s1, command="Rselfcorr")), dim=1)
    corr = model(fea_s, fea_c, command="corrm")
    _, gl_w = model(style, corr, command="encode2")
    return sp, gl_c, gl_w


def simple_swap(model, content, style, alphas=(1.0,)):
    """content, style: (B,3,H,W) in [-1,1] on the GPU.  Returns {alpha: image (B,3,H,W)}."""
    if above_code_grid(content, style):
        return simple_swap_full_size(model, content, style, alphas)
    sp, gl_c, gl_w = swap_codes(model, content, style)
    out = {}
    for alpha in alphas:
        code = glue.lerp(gl_c, gl_w, alpha)
        out[alpha] = model(sp, code, target=None, command="decode")
    return out


def native_size_rule(native_shape, load_size):
    """The size rule of ``simple_swap_native`` from shapes alone: ValueError unless the native images (B,H,W,3) are square with a
    side >= load_size and load_size is a side the model runs at (``ppst_model.correspondence_side``)."""
    from .ppst_model import correspondence_side
    if len(native_shape) != 4 or native_shape[3] != 3:
        raise ValueError("simple_swap_native takes native images as (B,H,W,3) uint8, got shape %s" % (tuple(native_shape),))
    correspondence_side(int(load_size), int(load_size))
    H, W = int(native_shape[1]), int(native_shape[2])
    if H != W or H < load_size:
        raise ValueError("simple_swap_native: native images must be square with a side of at least load_size = %d (the model runs "
                         "at load_size x load_size and its filter coefficients are upsampled, never reduced), got %d x %d"
                         % (load_size, H, W))


def simple_swap_native(model, content_native_u8, style, alphas=(1.0,), load_size=512):
    """``simple_swap`` + guided filter, delivered at the content file's own size.  content_native_u8: (B,H,W,3) uint8 on the GPU,
    square, H >= load_size; style: (B,3,h,w) in [-1,1] as today.  The model runs at load_size on
    ``imageio.preprocess(content_native_u8, load_size)`` (the tensor the file front end feeds it), the codes are ``simple_swap``'s,
    and each alpha is decoded by ``decode_native``: the filter's coefficients at load_size, upsampled and applied to the native
    image.  Returns {alpha: uint8 (B,H,W,3)}."""
    native_size_rule(tuple(content_native_u8.shape), load_size)
    from . import imageio
    content = imageio.preprocess(content_native_u8, load_size)
    sp, gl_c, gl_w = swap_codes(model, content, style)
    out = {}
    for alpha in alphas:
        out[alpha] = model(sp, glue.lerp(gl_c, gl_w, alpha), content, content_native_u8, command="decode_native")
    return out


def to_uint8_image(img):
    """ToPILImage()((x.clamp(-1,1)+1)*0.5) quantisation (simple_swapping_evaluator.py:61-62):
    (B,3,H,W) -> (B,H,W,3) uint8 (mul 255, truncate)."""
    v = (img.clamp(-1.0, 1.0) + 1.0) * 0.5
    return (v * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def shard_pairs(n_content, n_style, rank=0, world=1):
    """Pairs (i, j) owned by ``rank``: round-robin over the row-major pair index."""
    return [(i, j) for i in range(n_content) for j in range(n_style) if (i * n_style + j) % world == rank]


def shard_images(n_content, n_style, rank=0, world=1):
    """Images owned by ``rank``: image k (contents first, then styles) belongs to rank k mod world.
    Returns (content indices, style indices)."""
    own = [k for k in range(n_content + n_style) if k % world == rank]
    return [k for k in own if k < n_content], [k - n_content for k in own if k >= n_content]


def grid_image_pass(model, contents, styles, rank=0, world=1, image_batch=8):
    """Phase 1: the per-image passes of this rank's images, batched.  Returns
    (ci, sp (len(ci),256,h,w), fc (len(ci),512,h,w)), (si, fs (len(si),512,h,w)) -- NCHW-shaped like the commands return."""
    ci, si = shard_images(contents.shape[0], styles.shape[0], rank, world)
    full_size = above_code_grid(contents, styles)

    def feats(imgs, want_sp):
        sps, fs = [], []
        for k in range(0, imgs.shape[0], image_batch):
            img = imgs[k:k + image_batch]
            if full_size:       # sp on the image's own grid (a content only), the features from its 512 x 512 resample
                fs.append(model(img, command="correspondence_features").contiguous())
                if want_sp:
                    sps.append(model.E1(img).contiguous())      # (encode would add an E2 pass nobody reads)
                continue
            sp, gl = model(img, command="encode")
            f0, f1 = model(sp, gl, command="extract_feat")[1:]
            fs.append(torch.cat((f0, model(f1, command="Rselfcorr")), dim=1).contiguous())
            if want_sp:
                sps.append(sp.contiguous())
        return (torch.cat(sps, 0) if sps else None), (torch.cat(fs, 0) if fs else None)
    sp_c, f_c = feats(contents[ci], True) if ci else (None, None)
    _, f_s = feats(styles[si], False) if si else (None, None)
    return (ci, sp_c, f_c), (si, f_s)


def _gather_rows(local, idx, total, world, like):
    """all_gather of per-image rows: ``local`` (len(idx), ...) of this rank -> (total, ...) table on every rank.
    One padded all_gather_into_tensor (RCCL when the tensors live on the GPU, gloo on the CPU)."""
    import torch.distributed as dist
    per = (total + world - 1) // world
    shape = tuple(like)
    buf = torch.zeros((per,) + shape[1:], device=shape[0], dtype=torch.float32)
    if local is not None:
        buf[:local.shape[0]] = local
    out = torch.empty((world * per,) + shape[1:], device=shape[0], dtype=torch.float32)
    dist.all_gather_into_tensor(out, buf)
    return out.view((world, per) + shape[1:])


def grid_exchange(local_c, local_s, n_content, n_style, world, gathered=None, like=None):
    """Phase 2: assemble the full tables {content i: (sp, fc)}, {style j: fs} from every rank's phase-1 output.
    ``gathered``: list over ranks of phase-1 outputs (single-process simulation of N ranks); otherwise the live
    process group is used.  Tensors keep the commands' NCHW shape; the storage layout is plain contiguous."""
    table_c, table_s = {}, {}
    if gathered is not None:
        for (ci, sp_c, f_c), (si, f_s) in gathered:
            for n, i in enumerate(ci):
                table_c[i] = (sp_c[n:n + 1], f_c[n:n + 1])
            for n, j in enumerate(si):
                table_s[j] = f_s[n:n + 1]
        return table_c, table_s
    (ci, sp_c, f_c), (si, f_s) = local_c, local_s
    if world == 1:
        return grid_exchange(None, None, n_content, n_style, 1, gathered=[(local_c, local_s)])
    ref = sp_c if sp_c is not None else (f_c if f_c is not None else f_s)
    if ref is not None:
        dev, h, w = ref.device, ref.shape[2], ref.shape[3]
    elif like is not None:          # a rank that owns no image (world > N + M) still takes part in both gathers, with zero rows
        dev, h, w = like
    else:
        raise RuntimeError("this rank owns no image: pass like=(device, h, w) of the code grid")
    # rows of one rank: its contents' (sp | fc) = 768 channels, its styles' fs = 512 channels
    nc_max = (n_content + world - 1) // world + 1
    ns_max = (n_style + world - 1) // world + 1
    pack_c = torch.cat((sp_c, f_c), 1) if ci else None
    g_c = _gather_rows(pack_c, ci, nc_max * world, world, (dev, 768, h, w))
    g_s = _gather_rows(f_s, si, ns_max * world, world, (dev, 512, h, w))
    for r in range(world):
        rc, rs = shard_images(n_content, n_style, r, world)
        for n, i in enumerate(rc):
            table_c[i] = (g_c[r, n:n + 1, :256], g_c[r, n:n + 1, 256:])
        for n, j in enumerate(rs):
            table_s[j] = g_s[r, n:n + 1]
    return table_c, table_s


def grid_pair_pass(model, contents, styles, table_c, table_s, rank=0, world=1, smooth=True, pair_batch=8):
    """Phase 3: this rank's (content, style) pairs, batched: corrm -> encode2 -> decode (+ guided filter with the content
    as guide, content_style_grid_generation_evaluator.py:81-93)."""
    pairs = shard_pairs(contents.shape[0], styles.shape[0], rank, world)
    out = {}
    for k in range(0, len(pairs), pair_batch):
        chunk = pairs[k:k + pair_batch]
        sp = torch.cat([table_c[i][0] for i, _ in chunk], 0)
        fc = torch.cat([table_c[i][1] for i, _ in chunk], 0)
        fs = torch.cat([table_s[j] for _, j in chunk], 0)
        st = torch.cat([styles[j:j + 1] for _, j in chunk], 0)
        ct = torch.cat([contents[i:i + 1] for i, _ in chunk], 0)
        corr = model(fs, fc, command="corrm")
        _, gl_w = model(st, corr, command="encode2")
        img = model(sp, gl_w, command="decode", target=ct if smooth else None)
        for n, (i, j) in enumerate(chunk):
            out[(i, j)] = img[n]
    return out


def swapping_grid(model, contents, styles, rank=0, world=1, smooth=True, pair_batch=8, image_batch=8):
    """contents (N,3,H,W), styles (M,3,H,W) on this rank's GPU (every rank holds all images: they are small; the image
    passes and the pair passes are sharded).  Returns {(i, j): image (3,H,W)} for the pairs this rank owns.
    Above 512 x 512 (one rank only): sp at full size, the features from PPSTModel.correspondence_features; the packed exchange
    of several ranks assumes one grid for sp and the features, so every rank refuses from the shapes alone, before any collective.
    ``smooth``: the guided-filter post-process of PPSTModel.decode, with the radius of the model's option (Options.gf_radius: 30, or
    "scaled" = 30 * side // 512); there is no parameter for it here."""
    if world > 1 and above_code_grid(contents, styles):
        raise ValueError("swapping_grid above 512 x 512 runs on one rank: the exchange packs the spatial code and the 64 x 64 "
                         "correspondence features on one grid (got %s and %s on %d ranks)"
                         % (tuple(contents.shape[2:]), tuple(styles.shape[2:]), world))
    local_c, local_s = grid_image_pass(model, contents, styles, rank, world, image_batch)
    table_c, table_s = grid_exchange(local_c, local_s, contents.shape[0], styles.shape[0], world,
                                     like=(contents.device, contents.shape[2] // 8, contents.shape[3] // 8))
    return grid_pair_pass(model, contents, styles, table_c, table_s, rank, world, smooth, pair_batch)


# ------------------------------------------------------------------------------------------------- numbers about images
def evaluate_reconstruction(model, images, batch=8):
    """How well the auto-encoder path returns held-out images: under ``no_grad``, ``rec = decode(*encode(x))`` (no target, so no
    guided filter) in batches of ``batch``, compared with ``x`` by the HIP metrics (ppst_amd/metrics.py) at data range 2.
    ``images``: (N, 3, H, W) in [-1, 1] on the GPU.  Returns {"l1", "psnr", "ssim"}, plus "ms_ssim" where min(H, W) >= 176, plus
    "lpips" where ``model.perceptual_metric`` is an LPIPSAlex; every entry an (N,) fp32 tensor."""
    from . import metrics
    from .lpips import LPIPSAlex
    N, _, H, W = images.shape
    names = ["l1", "psnr", "ssim"]
    if min(H, W) >= ops.MS_SSIM_MIN_SIDE:
        names.append("ms_ssim")
    lp = model.perceptual_metric if isinstance(getattr(model, "perceptual_metric", None), LPIPSAlex) else None
    if lp is not None:
        names.append("lpips")
    out = {k: torch.empty((N,), device=images.device, dtype=torch.float32) for k in names}
    with torch.no_grad():
        for i in range(0, N, batch):
            x = images[i:i + batch]
            sp, gl = model(x, command="encode")
            rec = model(sp, gl, target=None, command="decode")
            err = ops.sqerr(rec, x, 2.0)
            out["l1"][i:i + batch] = err[:, 1]
            out["psnr"][i:i + batch] = err[:, 2]
            out["ssim"][i:i + batch] = metrics.ssim(rec, x, 2.0)
            if "ms_ssim" in out:
                out["ms_ssim"][i:i + batch] = metrics.ms_ssim(rec, x, 2.0)
            if lp is not None:
                out["lpips"][i:i + batch] = lp(rec, x).flatten()
    return out


def content_preservation(contents, outputs):
    """SSIM(content, swap) per pair, the content-preservation number of a swap.  ``outputs``: a tensor (K, C, H, W) paired with
    ``contents`` (K, C, H, W) one to one -> (K,) tensor; or what ``swapping_grid`` returns, {(i, j): image (3, H, W)}, in which
    case pair (i, j) is compared with ``contents[i]`` and the result is {(i, j): float}.  Images in [-1, 1] (data range 2)."""
    from . import metrics
    if isinstance(outputs, dict):
        keys = sorted(outputs)
        if not keys:
            return {}
        with torch.no_grad():
            vals = metrics.ssim(torch.stack([outputs[k] for k in keys]), torch.stack([contents[i] for i, _ in keys]))
        return dict(zip(keys, vals.cpu().tolist()))
    with torch.no_grad():
        return metrics.ssim(outputs, contents)


def style_fidelity(styles, outputs, style_labels=None, content_labels=None, regions=3):
    """Did the style arrive?  ``metrics.colour_distance`` between each style image and its swap, per region: the twin of
    ``content_preservation`` (which a swap that returns the content unchanged passes perfectly).  ``outputs``: a tensor paired
    with ``styles`` one to one -> {metric: float64 (K, R) tensor}; or what ``swapping_grid`` returns, {(i, j): image (3, H, W)},
    in which case pair (i, j) is compared with ``styles[j]`` and the result is {(i, j): {metric: [per region]}}.  Labels are
    integer (N, H, W) maps or one-hot (N, R, H, W) masks: ``style_labels`` those of ``styles``; ``content_labels`` those of the
    outputs -- with the dict, of the CONTENTS (``content_labels[i]`` for pair (i, j): the output has the content's geometry).
    Without both label sets the whole image is one region.  Images: fp32 in [-1, 1] or uint8 (N, H, W, 3).  The statistics of
    every distinct style image and of every output are computed once, not once per pair."""
    from . import metrics
    if (style_labels is None) != (content_labels is None):
        raise ValueError("style_fidelity needs the labels of both sides, or of neither")
    R = regions if style_labels is not None else 1
    with torch.no_grad():
        if isinstance(outputs, dict):
            keys = sorted(outputs)
            if not keys:
                return {}
            used = sorted({j for _, j in keys})
            st_s = metrics.colour_stats(styles[used], None if style_labels is None else style_labels[used], R)
            st_o = metrics.colour_stats(torch.stack([outputs[k] for k in keys]),
                                        None if content_labels is None else torch.stack([content_labels[i] for i, _ in keys]), R)
            dist = metrics.colour_distance(st_s, st_o, [(used.index(j), n) for n, (_, j) in enumerate(keys)])
            return {k: {name: v[n].tolist() for name, v in dist.items()} for n, k in enumerate(keys)}
        return metrics.colour_distance(metrics.colour_stats(styles, style_labels, R), metrics.colour_stats(outputs, content_labels, R))


# ------------------------------------------------------------------------------------------------- classical baselines
def _baseline_inputs(images, labels):
    """-> (uint8 (N, H, W, 3), uint8 (N, H, W) labels or None), as ``metrics.colour_stats`` reads them"""
    from . import metrics
    metrics._on_device(images)
    u8 = images if images.dtype == torch.uint8 else glue.tensor2im(images)
    if labels is not None:
        metrics._on_device(labels)
        labels = (labels.argmax(dim=1) if labels.dim() == 4 else labels).to(torch.uint8)
    return u8, labels


def _baseline_images(out_u8, guide_u8, smooth, gf_radius):
    """uint8 (K, H, W, 3) -> fp32 (K, 3, H, W) in [-1, 1]: the guided filter of ``decode(target=...)`` with the content as guide,
    or -- without it -- min((v + 0.5) / 127.5 - 1, 1), which stays in [-1, 1] and which ``glue.tensor2im`` takes back to v"""
    if smooth:
        return ops.guided_filter(guide_u8.contiguous(), out_u8, gf_radius, (0.02 * 255) ** 2)
    return ((out_u8.permute(0, 3, 1, 2).float() + 0.5) / 127.5 - 1.0).clamp_(max=1.0)


def baseline_swap(contents, styles, content_labels=None, style_labels=None, method="hist", regions=3, feather=0, smooth=False,
                  gf_radius=30):
    """What a CLASSICAL colour transfer makes of the pairs ``simple_swap`` is given: content n re-coloured towards style n per
    region (``metrics.colour_transfer``: "hist" exact histogram specification per RGB channel, "mkl" the Monge-Kantorovich
    linear map between the regions' Lab Gaussians, "reinhard" per-axis mean and deviation).  Images fp32 (B, 3, H, W) in [-1, 1] or
    uint8 (B, H, W, 3); labels as ``style_fidelity`` takes them, of both sides or of neither (then the image is one region).
    -> fp32 (B, 3, H, W) in [-1, 1] like ``simple_swap``'s images.  ``feather``: blend the regions through feathered mattes;
    ``smooth``: run ``ops.guided_filter`` (radius ``gf_radius``) with the content as guide, as ``decode(target=...)`` does."""
    from . import metrics
    if (style_labels is None) != (content_labels is None):
        raise ValueError("baseline_swap needs the labels of both sides, or of neither")
    R = regions if style_labels is not None else 1
    with torch.no_grad():
        c_u8, c_lab = _baseline_inputs(contents, content_labels)
        s_u8, s_lab = _baseline_inputs(styles, style_labels)
        if c_u8.shape[0] != s_u8.shape[0]:
            raise ValueError("baseline_swap pairs contents and styles one to one (%d and %d)" % (c_u8.shape[0], s_u8.shape[0]))
        st_s = metrics.colour_stats(s_u8, s_lab, R)
        out = metrics.colour_transfer(c_u8, st_s, c_lab, method, R, feather=feather)
        return _baseline_images(out, c_u8, smooth, gf_radius)


def baseline_grid(contents, styles, content_labels=None, style_labels=None, method="hist", regions=3, feather=0, smooth=False,
                  gf_radius=30, pairs=None):
    """``baseline_swap`` for every (content i, style j) (or the ``pairs`` given): {(i, j): image (3, H, W)}, shaped like
    ``swapping_grid``'s dict, so ``content_preservation`` and ``style_fidelity`` take it as it is.  The statistics of every
    distinct image are taken once."""
    from . import metrics
    if (style_labels is None) != (content_labels is None):
        raise ValueError("baseline_grid needs the labels of both sides, or of neither")
    R = regions if style_labels is not None else 1
    with torch.no_grad():
        c_u8, c_lab = _baseline_inputs(contents, content_labels)
        s_u8, s_lab = _baseline_inputs(styles, style_labels)
        if pairs is None:
            pairs = [(i, j) for i in range(c_u8.shape[0]) for j in range(s_u8.shape[0])]
        pairs = [(int(i), int(j)) for i, j in pairs]
        if not pairs:
            return {}
        st_s = metrics.colour_stats(s_u8, s_lab, R)
        st_c = metrics.colour_stats(c_u8, c_lab, R)
        out = metrics.colour_transfer(c_u8, st_s, c_lab, method, R, pairs=pairs, feather=feather, content_stats=st_c)
        img = _baseline_images(out, c_u8[[i for i, _ in pairs]], smooth, gf_radius)
        return {k: img[n] for n, k in enumerate(pairs)}


# ------------------------------------------------------------------------------------------------- file front ends
_IMG_EXT = (".jpg", ".jpeg", ".png", ".bmp", ".webp")
_stem = lambda p: os.path.splitext(os.path.basename(p))[0]
_as_list = lambda p: [p] if isinstance(p, (str, bytes, os.PathLike)) else list(p)       # one path or a list of paths


def _decode(path):
    from PIL import Image
    import numpy as np
    return np.array(Image.open(path).convert("RGB"))


DECODERS = ("host", "device")
# Where load_images decodes when its caller does not say: the switch of evaluate_swap_files and evaluate_grid_folder, whose
# parameter lists are pinned (tests/test_jpeg_cases_cpu.py test_front_end_signatures_only_grew_at_the_end).  Per thread: two
# evaluators running side by side do not see each other's setting.  Set it with ``with evaluation.decoder("device"): ...``.
_DECODE = threading.local()


def current_decoder():
    return getattr(_DECODE, "value", "host")


def _check_decoder(decode):
    if decode not in DECODERS:
        raise ValueError("decoder must be one of %s, not %r" % (DECODERS, decode))


@contextlib.contextmanager
def decoder(name):
    """``with decoder("device"):`` -- load_images, evaluate_swap_files and evaluate_grid_folder called from THIS thread inside the
    block decode JPEG and PNG files with the HIP decoders (load_images' ``decode=`` argument still wins).  ValueError for an unknown name,
    before anything runs."""
    _check_decoder(name)
    prev = current_decoder()
    _DECODE.value = name
    try:
        yield
    finally:
        _DECODE.value = prev


def _read_file(path):
    with open(path, "rb") as f:
        return f.read()


def decode_files_device(blobs, names, device="cuda", mirror=None):
    """The device half of ``decode="device"``: blobs[i] = the bytes of file names[i].  -> list with a (H,W,3) uint8 device tensor
    where a HIP decoder took the file and decoded it with status 0 (one batched call over all .jpg / .jpeg files, ops.jpeg_decode,
    and one over all .png files, ops.png_decode), None where the host has to: another extension, a file the parser refuses, a
    non-zero status."""
    out = [None] * len(blobs)
    for codec in ops.CODECS:                                     # (the table that decides which coder takes a file)
        parsed = {i: codec.parse(b) for i, (b, n) in enumerate(zip(blobs, names)) if ops.codec_for(n) is codec}
        take = [i for i in sorted(parsed) if parsed[i][0] == 0]
        if take:                                                 # codec.rgb: what Pillow's convert("RGB") gives
            views, status = codec.decode([blobs[i] for i in take], device=device, parsed=[parsed[i][1] for i in take],
                                         mirror=None if mirror is None else [mirror[i] for i in take], **codec.rgb)
            for i, v, st in zip(take, views, status.cpu().tolist()):
                out[i] = v if st == 0 else None
    return out


def load_images(paths, load_size=512, device="cuda", pool=None, decode=None):
    """data/base_dataset.py:85-171 (scale_shortside + make_power_2 + ToTensor + Normalize) for a list of files: decode on
    host threads, everything else on the device.  Returns a list of (1,3,H,W) tensors (sizes may differ per file).
    ``decode="device"``: the threads only read the files' bytes; the .jpg / .jpeg and the .png files the HIP decoders take are
    decoded in ONE batched call each on the device (bit-identical to Pillow), every other file -- and any the device reports damaged -- goes through
    Pillow as before, so a file fails here exactly when it fails with ``"host"``.  ``decode=None``: the module's setting (``decoder``)."""
    from . import imageio
    decode = current_decoder() if decode is None else decode
    _check_decoder(decode)
    if decode == "host":
        arrs = list(pool.map(_decode, paths)) if pool is not None else [_decode(p) for p in paths]
        return [imageio.preprocess(torch.from_numpy(a[None]).to(device), load_size) for a in arrs]
    blobs = list(pool.map(_read_file, paths)) if pool is not None else [_read_file(p) for p in paths]
    imgs = decode_files_device(blobs, paths, device)
    rest = [i for i, v in enumerate(imgs) if v is None]
    host = list(pool.map(_decode, [paths[i] for i in rest])) if pool is not None else [_decode(paths[i]) for i in rest]
    for i, a in zip(rest, host):
        imgs[i] = torch.from_numpy(a).to(device)
    return [imageio.preprocess(v[None], load_size) for v in imgs]


def _save_png(args):
    from PIL import Image
    arr, path = args
    Image.fromarray(arr).save(path)
    return path


def _save_jpeg(args):
    from PIL import Image
    arr, path, quality, subsampling = args
    Image.fromarray(arr[:, :, 0] if arr.shape[2] == 1 else arr).save(path, format="JPEG", quality=quality, subsampling=subsampling)
    return path


def _write_file(args):
    blob, path = args
    with open(path, "wb") as f:
        f.write(blob)
    return path


PNG_ENCODERS = ("host", "device")


def _check_encoder(encoder):
    if encoder not in PNG_ENCODERS:
        raise ValueError("PNG encoder must be one of %s, not %r" % (PNG_ENCODERS, encoder))


FORMATS = {"png": ".png", "jpeg": ".jpg"}          # file format -> the extension of the names the front ends make up


def _check_format(format, jpeg_quality, jpeg_subsampling):
    """ValueError for an unknown format or JPEG setting (checked whatever the format: a typo shows at once)."""
    if format not in FORMATS:
        raise ValueError("file format must be one of %s, not %r" % (tuple(FORMATS), format))
    ops.check_jpeg_settings(jpeg_quality, jpeg_subsampling)


def write_png_batch(u8, paths, pool=None, encoder="host", format="png", jpeg_quality=90, jpeg_subsampling="4:2:0"):
    """u8: (B,H,W,C) uint8 on the device -> one PNG file per image, the half of the file output both front ends share.
    ``host``: one device-to-host copy of the batch, ``Image.fromarray(arr).save(path)`` per image; ``device``: the files are
    encoded on the GPU (imageio.encode_png) and only their bytes are copied and written.  The per-image jobs run on ``pool``'s
    threads when one is given (the futures are returned: the caller overlaps them with the next batch and joins at the end).
    ``format="jpeg"``: baseline JPEG files instead -- ``host`` = Pillow's ``save(format="JPEG", quality=, subsampling=)``,
    ``device`` = imageio.encode_jpeg.  ``paths`` are written as given, whatever the format."""
    _check_encoder(encoder)
    _check_format(format, jpeg_quality, jpeg_subsampling)
    if encoder == "device":
        from . import imageio
        blobs = imageio.encode_jpeg(u8, jpeg_quality, jpeg_subsampling) if format == "jpeg" else imageio.encode_png(u8)
        job, jobs = _write_file, list(zip(blobs, paths))
    elif format == "jpeg":
        arr = u8.cpu().numpy()
        job, jobs = _save_jpeg, [(arr[i], p, jpeg_quality, jpeg_subsampling) for i, p in enumerate(paths)]
    else:
        arr = u8.cpu().numpy()
        job, jobs = _save_png, [(arr[i], p) for i, p in enumerate(paths)]
    if pool is None:
        return [job(j) for j in jobs]
    return [pool.submit(job, j) for j in jobs]


def save_images(images, paths, pool=None, encoder="host", format="png", jpeg_quality=90, jpeg_subsampling="4:2:0"):
    """images: (B,3,H,W) in [-1,1] on the device -> PNG files.  util.tensor2im quantisation (util/util.py:98-131) on the
    device, then write_png_batch (``encoder``: "host" = Pillow on the pool's threads, "device" = the HIP encoder;
    ``format="jpeg"`` with its quality and subsampling: JPEG files)."""
    _check_encoder(encoder)
    _check_format(format, jpeg_quality, jpeg_subsampling)
    return write_png_batch(glue.tensor2im(images), paths, pool, encoder, format, jpeg_quality, jpeg_subsampling)


def _check_files(png, format, jpeg_quality, jpeg_subsampling):
    """what every file front end refuses before it reads a file"""
    _check_encoder(png)
    _check_format(format, jpeg_quality, jpeg_subsampling)
    _check_decoder(current_decoder())


def _swap_name(out_dir, structure, texture, alpha, format):
    """<structure>_<texture>_<alpha %.2f> with the format's extension (simple_swapping_evaluator.py:61-62)"""
    return os.path.join(out_dir, "%s_%s_%.2f%s" % (_stem(structure), _stem(texture), alpha, FORMATS[format]))


def _spread(structures, v, message):
    """one entry serves every structure, otherwise the lists pair up; an absent list (None) stays absent"""
    v = v * len(structures) if v is not None and len(v) == 1 else v
    if v is not None and len(v) != len(structures):
        raise ValueError(message % (len(structures), len(v)))
    return v


def evaluate_swap_files(model, structure_path, texture_path, out_dir, alphas=(1.0,), load_size=512, device="cuda", png="host",
                        format="png", jpeg_quality=90, jpeg_subsampling="4:2:0"):
    """evaluation/simple_swapping_evaluator.py:38-76: one structure image, one texture image, one output per mix alpha named
    <structure>_<texture>_<alpha %.2f>.png (ToPILImage quantisation of the clamped image, :61-62).  ``png``: where the files are
    encoded (write_png_batch).  ``format="jpeg"``: JPEG files of that quality and subsampling, named .jpg.  The two inputs are decoded where
    ``evaluation.decoder`` says (load_images).  Returns the paths."""
    _check_files(png, format, jpeg_quality, jpeg_subsampling)
    os.makedirs(out_dir, exist_ok=True)
    c, s_ = load_images([os.path.expanduser(structure_path), os.path.expanduser(texture_path)], load_size, device)
    outs = simple_swap(model, c, s_, alphas)
    paths = []
    for alpha in alphas:
        path = _swap_name(out_dir, structure_path, texture_path, alpha, format)
        paths += write_png_batch(to_uint8_image(outs[alpha])[:1], [path], None, png, format, jpeg_quality, jpeg_subsampling)
    return paths


def load_native(paths, device="cuda", pool=None):
    """Files -> list of (H,W,3) uint8 device tensors at the files' own sizes, decoded where ``evaluation.decoder`` says: on the
    host (Pillow), or by the HIP decoders with Pillow for whatever they do not take (the rule of ``load_images``)."""
    decode = current_decoder()
    _check_decoder(decode)
    imgs = [None] * len(paths)
    if decode == "device":
        blobs = list(pool.map(_read_file, paths)) if pool is not None else [_read_file(p) for p in paths]
        imgs = decode_files_device(blobs, paths, device)
    rest = [i for i, v in enumerate(imgs) if v is None]
    host = list(pool.map(_decode, [paths[i] for i in rest])) if pool is not None else [_decode(paths[i]) for i in rest]
    for i, a in zip(rest, host):
        imgs[i] = torch.from_numpy(a).to(device)
    return imgs


def _device_encoder_takes(shape, format, jpeg_subsampling):
    """whether the device encoder of ``format`` has a bound for images of this (H, W, C) (ops.png_encode / jpeg_encode refuse otherwise)"""
    from ._lib import lib
    H, W, C = (int(v) for v in shape)
    if format == "jpeg":
        return lib.ppst_jpeg_bound(H, W, C, ops.JPEG_SUBSAMPLING[jpeg_subsampling]) >= 0
    return lib.ppst_png_bound(H, W, C) >= 0


def evaluate_swap_files_native(model, structure_path, texture_path, out_dir, alphas=(1.0,), load_size=512, device="cuda", png="host",
                               format="png", jpeg_quality=90, jpeg_subsampling="4:2:0"):
    """``evaluate_swap_files`` with every output at the size of its structure FILE (``simple_swap_native``: the model runs at
    load_size, the guided filter's coefficients are applied to the file's own pixels).  ``structure_path`` / ``texture_path``: one
    path or a list of paths each -- one texture serves every structure, otherwise the two lists pair up.  Structure files are read
    at their own size (square, side >= load_size) where ``evaluation.decoder`` says, textures as today (load_images); structures
    of one size run as one batch.  Files are written through write_png_batch, named as evaluate_swap_files names them; a size the
    device encoder has no bound for is encoded on the host.  Returns the paths, structure by structure, alpha by alpha."""
    _check_files(png, format, jpeg_quality, jpeg_subsampling)
    structures = _as_list(structure_path)
    textures = _spread(structures, _as_list(texture_path),
                       "evaluate_swap_files_native pairs structures and textures: %d structure and %d texture paths")
    os.makedirs(out_dir, exist_ok=True)
    natives = load_native([os.path.expanduser(p) for p in structures], device)
    for n in natives:                                          # (before any model pass: a wrong size fails at once)
        native_size_rule((1,) + tuple(n.shape), load_size)
    styles = load_images([os.path.expanduser(p) for p in textures], load_size, device)
    swap = lambda idx: simple_swap_native(model, torch.stack([natives[i] for i in idx]), torch.cat([styles[i] for i in idx], 0), alphas,
                                          load_size)
    return _swap_groups_to_files(structures, textures, natives, styles, swap, out_dir, alphas, png, format, jpeg_quality, jpeg_subsampling)


def _swap_groups_to_files(structures, textures, natives, styles, swap, out_dir, alphas, png, format, jpeg_quality, jpeg_subsampling):
    """The tail of the front ends that keep the structure FILE's size: structures of one size (and one texture size) share a
    batch, ``swap(idx)`` -> {alpha: uint8 (len(idx),H,W,3)} runs it, the files are named as evaluate_swap_files names them and
    written through write_png_batch (a size the device encoder has no bound for: on the host).  Returns the paths, structure by
    structure, alpha by alpha."""
    groups = {}
    for i, n in enumerate(natives):
        groups.setdefault((tuple(n.shape), tuple(styles[i].shape)), []).append(i)
    paths = {}
    for (shape, _), idx in groups.items():
        outs = swap(idx)
        encoder = png if png == "host" or _device_encoder_takes(shape, format, jpeg_subsampling) else "host"
        for alpha in alphas:
            names = [_swap_name(out_dir, structures[i], textures[i], alpha, format) for i in idx]
            for i, p in zip(idx, write_png_batch(outs[alpha], names, None, encoder, format, jpeg_quality, jpeg_subsampling)):
                paths.setdefault(i, []).append(p)
    return [p for i in range(len(structures)) for p in paths[i]]


def region_rule(photo_shape, xf, load_size):
    """What ``simple_swap_region`` refuses from shapes and integers alone: photos that are not (B,H,W,3), a load_size the model does
    not run at, crop transforms outside 1 <= s <= 8 (``imageio.crop_transform_rule``)."""
    from . import imageio
    from .ppst_model import correspondence_side
    if len(photo_shape) != 4 or photo_shape[3] != 3:
        raise ValueError("simple_swap_region takes photos as (B,H,W,3) uint8, got shape %s" % (tuple(photo_shape),))
    correspondence_side(int(load_size), int(load_size))
    imageio.crop_transform_rule(xf, load_size)


def simple_swap_region(model, photo_u8, xf, style, alphas=(1.0,), load_size=512, feather=16, style_xf=None):
    """A swap INSIDE a photograph: photo_u8 (B,H,W,3) uint8 on the GPU, of any shape; ``xf`` the crop transforms of the region
    (``imageio.crop_transform``: centre, side and angle of the aligned square, 1 <= side / load_size <= 8).  The content is
    ``to_tensor_normalized(extract_similarity(photo, xf, load_size))``; ``style`` is a (B,3,h,w) tensor in [-1,1] as for
    ``simple_swap`` or, with ``style_xf``, a uint8 photo whose region is extracted the same way.  The codes are ``swap_codes``',
    and each alpha goes through ``decode_region``: the guided filter's coefficients at load_size, applied to the photo's own
    pixels inside the square and feathered over ``feather`` crop pixels at its edge.  Returns {alpha: uint8 (B,H,W,3)}; every
    byte outside the square is the photo's.  ``simple_swap_region_matte`` blends through a matte of the face instead of the whole
    square."""
    return simple_swap_region_matte(model, photo_u8, xf, style, alphas, load_size, feather, style_xf)


def crop_labels(labels, B, load_size):
    """Label maps of the crops as (B,n,n) uint8, n == load_size: (B,n,n) uint8 / int64, or one-hot (B,C,n,n) arg-maxed as
    ``metrics.colour_stats`` does.  Raises ValueError from shapes and dtypes alone."""
    if not isinstance(labels, torch.Tensor) or labels.dim() not in (3, 4):
        raise ValueError("labels are a (B,n,n) uint8 / int64 tensor or one-hot (B,C,n,n), got %s"
                         % (tuple(labels.shape) if isinstance(labels, torch.Tensor) else type(labels).__name__,))
    if labels.dim() == 4:
        if labels.shape[1] > 256:
            raise ValueError("one-hot labels have at most 256 classes, got %d" % labels.shape[1])
        labels = labels.argmax(1)
    elif labels.dtype not in (torch.uint8, torch.int64):
        raise ValueError("labels (B,n,n) are uint8 or int64, got %s" % labels.dtype)
    if tuple(labels.shape) != (B, int(load_size), int(load_size)):
        raise ValueError("labels lie in the crop's frame: (%d,%d,%d) for this batch and load_size, got %s"
                         % (B, load_size, load_size, tuple(labels.shape)))
    if labels.dtype != torch.uint8:
        labels = labels.clamp(0, 255).to(torch.uint8)                              # (values >= 32 are outside any matte)
    return labels


def simple_swap_region_matte(model, photo_u8, xf, style, alphas=(1.0,), load_size=512, feather=16, style_xf=None, labels=None,
                             keep=(1, 2), matte_feather=16, matte_grow=8, matte=None):
    """``simple_swap_region`` blended through a matte of the face, so that the re-coloured background of the square does not reach
    the photo.  ``labels``: per-pixel labels of the CROP (``crop_labels``: (B,n,n) uint8 / int64 or one-hot (B,C,n,n), n ==
    load_size), turned into a matte by ``ops.label_matte(labels, keep, matte_feather, matte_grow)``: label values in ``keep`` are
    the face, the ramp is ``matte_feather`` crop pixels wide and reaches ``matte_grow`` pixels outwards.  ``matte``: a ready fp32
    (B,n,n) matte in [0, 1] instead; both together raise.  Neither: ``simple_swap_region``.  Photo pixels where the matte is 0 keep
    their bytes.  ``simple_swap_region_gmatte`` refines the matte with the photo's own pixels."""
    return _swap_region("simple_swap_region_matte", model, photo_u8, xf, style, alphas, load_size, feather, style_xf, labels, keep,
                        matte_feather, matte_grow, matte, None)


def simple_swap_region_gmatte(model, photo_u8, xf, style, alphas=(1.0,), load_size=512, feather=16, style_xf=None, labels=None,
                              keep=(1, 2), matte_feather=16, matte_grow=8, matte=None, matte_radius=8, matte_eps=(0.01 * 255) ** 2,
                              want_weight=False):
    """``simple_swap_region_matte`` with the matte refined by the photo's own pixels (He et al.'s guided feathering): the matte of
    the labels (or the ready ``matte``; one of the two is required) is filtered with the crop as guide at radius ``matte_radius``
    and ``matte_eps`` (``ops.guided_matte_coeffs``) and evaluated from those coefficients on every photo pixel
    (``PPSTModel.decode_region_gmatte``), so the blend edge follows hair, ears and the jaw line of the photo instead of a ramp
    around the label boundary.  ``want_weight``: {alpha: (image, weight)}, the weight the uint8 (B,H,W) blend weight."""
    if labels is None and matte is None:
        raise ValueError("simple_swap_region_gmatte needs labels or a matte (simple_swap_region blends the whole square)")
    return _swap_region("simple_swap_region_gmatte", model, photo_u8, xf, style, alphas, load_size, feather, style_xf, labels, keep,
                        matte_feather, matte_grow, matte, (matte_radius, matte_eps, want_weight))


def _swap_region(who, model, photo_u8, xf, style, alphas, load_size, feather, style_xf, labels, keep, matte_feather, matte_grow, matte,
                 gmatte):
    """the region swaps' one body.  ``gmatte``: None, or (matte_radius, matte_eps, want_weight) of the guided matte"""
    region_rule(tuple(photo_u8.shape), xf, load_size)
    if labels is not None and matte is not None:
        raise ValueError("%s takes labels or a matte, not both" % who)
    if gmatte is not None:
        from .ppst_model import guided_matte_radius
        guided_matte_radius(gmatte[0], int(load_size))         # (before any kernel runs)
    if labels is not None:
        labels = crop_labels(labels, int(photo_u8.shape[0]), load_size)
    from . import imageio
    if labels is not None:
        matte = ops.label_matte(labels.to(photo_u8.device), keep, matte_feather, matte_grow)
    if style_xf is not None:
        imageio.crop_transform_rule(style_xf, load_size)
        style = imageio.to_tensor_normalized(ops.extract_similarity(style, style_xf, load_size))
    content = imageio.to_tensor_normalized(ops.extract_similarity(photo_u8, xf, load_size))
    sp, gl_c, gl_w = swap_codes(model, content, style)
    out = {}
    for alpha in alphas:
        code = glue.lerp(gl_c, gl_w, alpha)
        if gmatte is not None:
            out[alpha] = model(sp, code, content, photo_u8, xf, feather, matte, *gmatte, command="decode_region_gmatte")
        elif matte is None:
            out[alpha] = model(sp, code, content, photo_u8, xf, feather, command="decode_region")
        else:
            out[alpha] = model(sp, code, content, photo_u8, xf, feather, matte, command="decode_region_matte")
    return out


def evaluate_swap_files_region(model, structure_path, texture_path, out_dir, structure_box, texture_box=None, alphas=(1.0,), load_size=512,
                               feather=16, device="cuda", png="host", format="png", jpeg_quality=90, jpeg_subsampling="4:2:0",
                               label_path=None, keep=(1, 2), matte_feather=16, matte_grow=8):
    """``evaluate_swap_files`` for a face inside a photograph (``simple_swap_region``): the structure FILE keeps its size and
    every pixel outside the box.  A box is (cx, cy, side, angle_deg) in the file's pixels (``imageio.crop_transform``).
    ``structure_path`` / ``texture_path``: one path or a list each, ``structure_box`` / ``texture_box``: one box or one per path --
    one texture (and one box) serves every structure, otherwise the lists pair up.  ``texture_box=None`` loads the texture as
    ``evaluate_swap_files`` does (the whole file at load_size); with a box its region is extracted like the structure's.  Files
    are read at their own size by ``load_native`` and written through write_png_batch, named as evaluate_swap_files names them;
    a size the device encoder has no bound for is encoded on the host.  ``label_path``: one grey label PNG per structure, in the
    CROP's frame (the layout of the dataset's ``labels/``), read with ``convert("L")`` and resized NEAREST to load_size when it
    differs (the dataset's rule); the lists pair up as the boxes do, and the swap is blended through
    ``ops.label_matte(labels, keep, matte_feather, matte_grow)`` (``simple_swap_region_matte``).  Returns the paths, structure by
    structure, alpha by alpha.  ``evaluate_swap_files_region_gmatte`` refines that matte with the photo's own pixels."""
    return _swap_files_region(model, structure_path, texture_path, out_dir, structure_box, texture_box, alphas, load_size, feather, device,
                              png, format, jpeg_quality, jpeg_subsampling, label_path, keep, matte_feather, matte_grow, None)


def evaluate_swap_files_region_gmatte(model, structure_path, texture_path, out_dir, structure_box, texture_box=None, alphas=(1.0,),
                                      load_size=512, feather=16, device="cuda", png="host", format="png", jpeg_quality=90,
                                      jpeg_subsampling="4:2:0", label_path=None, keep=(1, 2), matte_feather=16, matte_grow=8,
                                      matte_radius=8, matte_eps=(0.01 * 255) ** 2):
    """``evaluate_swap_files_region`` through ``simple_swap_region_gmatte``: the matte of each structure's label file is refined by
    the photo's own pixels (guided filter of radius ``matte_radius`` and ``matte_eps`` with the crop as guide).  ``label_path`` is
    required."""
    if label_path is None:
        raise ValueError("evaluate_swap_files_region_gmatte needs label_path (evaluate_swap_files_region blends the whole square)")
    from .ppst_model import guided_matte_radius
    guided_matte_radius(matte_radius, int(load_size))          # (before any file is read)
    return _swap_files_region(model, structure_path, texture_path, out_dir, structure_box, texture_box, alphas, load_size, feather, device,
                              png, format, jpeg_quality, jpeg_subsampling, label_path, keep, matte_feather, matte_grow,
                              (matte_radius, matte_eps))


def _swap_files_region(model, structure_path, texture_path, out_dir, structure_box, texture_box, alphas, load_size, feather, device, png,
                       format, jpeg_quality, jpeg_subsampling, label_path, keep, matte_feather, matte_grow, gmatte):
    """the region file front ends' one body.  ``gmatte``: None, or (matte_radius, matte_eps) of the guided matte"""
    import functools
    region_swap = simple_swap_region_matte if gmatte is None else functools.partial(simple_swap_region_gmatte, matte_radius=gmatte[0],
                                                                                    matte_eps=gmatte[1])
    from . import imageio
    _check_files(png, format, jpeg_quality, jpeg_subsampling)
    boxes = lambda b: [tuple(b)] if not hasattr(b[0], "__len__") else [tuple(v) for v in b]
    structures = _as_list(structure_path)
    lists = ((_as_list(texture_path), "texture paths"), (boxes(structure_box), "structure boxes"),
             (None if texture_box is None else boxes(texture_box), "texture boxes"),
             (None if label_path is None else _as_list(label_path), "label paths"))
    textures, sboxes, tboxes, lpaths = [_spread(structures, v, "evaluate_swap_files_region pairs its lists: %d structure paths and %d " + what)
                                        for v, what in lists]
    os.makedirs(out_dir, exist_ok=True)
    to_xf = lambda box: imageio.crop_transform((box[0], box[1]), box[2], box[3] if len(box) > 3 else 0.0, load_size)
    sxf = [to_xf(b) for b in sboxes]
    txf = None if tboxes is None else [to_xf(b) for b in tboxes]
    imageio.crop_transform_rule(sxf, load_size)                # (before any file is read: a bad box fails at once)
    if txf is not None:
        imageio.crop_transform_rule(txf, load_size)
    photos = load_native([os.path.expanduser(p) for p in structures], device)
    if txf is None:
        styles = load_images([os.path.expanduser(p) for p in textures], load_size, device)
    else:
        tphotos = load_native([os.path.expanduser(p) for p in textures], device)
        styles = [imageio.to_tensor_normalized(ops.extract_similarity(t[None], [x], load_size)) for t, x in zip(tphotos, txf)]
    labels = None
    if lpaths is not None:
        import numpy as np
        from PIL import Image

        def read(p):
            im = Image.open(os.path.expanduser(p)).convert("L")
            return np.asarray(im if im.size == (load_size, load_size) else im.resize((load_size, load_size), Image.NEAREST))
        labels = torch.from_numpy(np.stack([read(p) for p in lpaths])).to(device)
    swap = lambda idx: region_swap(model, torch.stack([photos[i] for i in idx]), [sxf[i] for i in idx], torch.cat([styles[i] for i in idx], 0),
                                   alphas, load_size, feather, labels=None if labels is None else labels[idx], keep=keep,
                                   matte_feather=matte_feather, matte_grow=matte_grow)
    return _swap_groups_to_files(structures, textures, photos, styles, swap, out_dir, alphas, png, format, jpeg_quality, jpeg_subsampling)


def evaluate_grid_folder(model, dataroot, out_dir, rank=0, world=1, smooth=True, load_size=512, device="cuda", workers=8,
                         pair_batch=8, image_batch=8, png="host", format="png", jpeg_quality=90, jpeg_subsampling="4:2:0"):
    """evaluation/content_style_grid_generation_evaluator.py:36-99 over <dataroot>/content/* and <dataroot>/style/*: every
    (content, style) pair, guided-filter post-process with the content as guide (radius: the model's Options.gf_radius -- decode
    reads it, this function has no parameter for it); files land in <out_dir>/images/ under the
    reference's names (<content>_<style>.png, the inputs as <name>.png; util/html.py:51-75 -- the HTML index itself is not
    written).  All images must come out of the preprocessing at one size (the reference batches them the same way).
    Multi-GPU: every rank reads all inputs (they are small), computes its share (swapping_grid) and writes its own files.
    ``png``: "host" = Pillow on the worker threads, "device" = the HIP encoder (the threads only write the bytes).
    ``format="jpeg"``: JPEG files of that quality and subsampling under the same names with .jpg, by the same switch.
    Inside ``with evaluation.decoder("device"):`` the threads read bytes and the HIP decoders take the JPEG and PNG files they can in one
    batched call (load_images); otherwise Pillow decodes on the worker threads."""
    _check_files(png, format, jpeg_quality, jpeg_subsampling)
    ext, fmt = FORMATS[format], (format, jpeg_quality, jpeg_subsampling)
    from concurrent.futures import ThreadPoolExecutor
    cdir, sdir = os.path.join(dataroot, "content"), os.path.join(dataroot, "style")
    ls = lambda d: sorted(os.path.join(d, f) for f in os.listdir(d) if f.lower().endswith(_IMG_EXT))
    cpaths, spaths = ls(cdir), ls(sdir)
    if not cpaths or not spaths:
        raise RuntimeError("need images under %s and %s" % (cdir, sdir))
    img_dir = os.path.join(out_dir, "images")
    os.makedirs(img_dir, exist_ok=True)
    with ThreadPoolExecutor(max_workers=workers) as pool:
        imgs = load_images(cpaths + spaths, load_size, device, pool)
        if len({tuple(t.shape) for t in imgs}) != 1:
            raise RuntimeError("images of different sizes after preprocessing: %s" % sorted({tuple(t.shape[2:]) for t in imgs}))
        contents, styles = torch.cat(imgs[:len(cpaths)], 0), torch.cat(imgs[len(cpaths):], 0)
        futures = []
        if rank == 0:   # the top row / first column of the reference's page: the inputs themselves
            futures += save_images(torch.cat((contents, styles), 0), [os.path.join(img_dir, _stem(p) + ext) for p in cpaths + spaths], pool, png, *fmt)
        out = swapping_grid(model, contents, styles, rank, world, smooth, pair_batch, image_batch)
        keys = sorted(out)
        for k in range(0, len(keys), pair_batch):
            chunk = keys[k:k + pair_batch]
            names = [os.path.join(img_dir, "%s_%s%s" % (_stem(cpaths[i]), _stem(spaths[j]), ext)) for i, j in chunk]
            futures += save_images(torch.stack([out[ij] for ij in chunk], 0), names, pool, png, *fmt)
        written = [f.result() for f in futures]
    return written
