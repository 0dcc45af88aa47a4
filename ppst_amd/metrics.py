"""Image-quality metrics on the HIP path (csrc/ssim.hip; include/ppst_hip.h "image-quality metrics"): PSNR, SSIM (Wang et al.
2004: 11-tap Gaussian window, sigma 1.5, valid) and five-scale MS-SSIM (Wang et al. 2003).  They need no weights and are defined
by published formulas, so they are held to float64 restatements of exactly those (tests/ssim_cases.py).

Images are fp32 (B, C, H, W) in any layout, or uint8 (B, H, W, C) as ``glue.tensor2im`` / ``evaluation.to_uint8_image`` make
them.  ``data_range`` defaults to 2.0 for float tensors (the model's [-1, 1]) and to 255 for uint8.  Every function returns one
fp32 number per image, (B,).  ``ssim`` is differentiable in its FIRST argument (fp32 only); MS-SSIM and PSNR are forward only.
There is no CPU fallback: CPU tensors raise RuntimeError.

The second half of this file holds the style-fidelity metrics (csrc/colour_stats.hip; include/ppst_hip.h "colour statistics"):
``colour_stats`` / ``colour_distance``, distances between the colour distributions of two images per label region, held to
integer and float64 restatements (tests/colour_cases.py).

The last part holds the colour-transfer baselines (csrc/colour_transfer.hip; include/ppst_hip.h "colour transfer"):
``colour_transfer_maps`` / ``colour_transfer``, classical per-region histogram specification, Monge-Kantorovich and Reinhard
transfers, held to integer and float64 restatements (tests/transfer_cases.py).
"""
import torch

from . import autograd as A
from . import ops


def _on_device(*ts):
    for t in ts:
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError("metrics: inputs must be CUDA (HIP) tensors (no CPU fallback)")


def psnr(a, b, data_range=None):
    """10 log10(L^2 / mean((a - b)^2)) per image; +inf for equal images"""
    _on_device(a, b)
    return ops.sqerr(a.detach(), b.detach(), data_range)[:, 2]


def l1(a, b):
    """mean |a - b| per image, in the inputs' units (the same pass as ``psnr``)"""
    _on_device(a, b)
    return ops.sqerr(a.detach(), b.detach())[:, 1]


def ssim(a, b, data_range=None):
    _on_device(a, b)
    L = ops.default_data_range(a, data_range)
    if a.dtype == torch.float32 and (a.requires_grad or b.requires_grad) and torch.is_grad_enabled():
        return A.SsimFn.apply(a, b, L)
    return ops.ssim_forward(a.detach(), b.detach(), L)[0]


def ms_ssim(a, b, data_range=None):
    """raises ValueError below 176 pixels a side (176 -> 88 -> 44 -> 22 -> 11: the fifth scale must still hold the window)"""
    if isinstance(a, torch.Tensor) and a.dim() == 4:          # the size rule first: it needs no device to be checked
        H, W = (a.shape[1], a.shape[2]) if a.dtype == torch.uint8 else (a.shape[2], a.shape[3])
        if min(H, W) < ops.MS_SSIM_MIN_SIDE:
            raise ValueError("ms_ssim needs images of at least %d x %d (five scales, the last one must still hold the 11-tap "
                             "window), got %d x %d" % (ops.MS_SSIM_MIN_SIDE, ops.MS_SSIM_MIN_SIDE, H, W))
    _on_device(a, b)
    return ops.ms_ssim_forward(a.detach(), b.detach(), data_range)


class SSIMLoss:
    """1 - SSIM as a perceptual-metric callable: (a, b) -> (B, 1, 1, 1), the shape ``LPIPSAlex.__call__`` returns; differentiable
    in ``a`` (PPSTModel.set_perceptual_metric("ssim")).  It has no weights and no state."""

    def __init__(self, data_range=None):
        self.data_range = data_range

    def __call__(self, a, b):
        return (1.0 - ssim(a, b, self.data_range)).view(-1, 1, 1, 1)


# ------------------------------------------------------------------------------------------------- style fidelity
# Did the STYLE arrive?  Distances between the colour distributions of two images, taken per region of a label map (skin, hair,
# background: CelebAMaskDataset's three classes).  They need no weights and are defined by formulas (include/ppst_hip.h "colour
# statistics"; DESIGN.md "Style-fidelity metrics"), so the tests hold them to integer and float64 restatements.
_DIRECTIONS = {}
LUMA_601 = (1225, 2404, 467)            # BT.601 luma in 1/4096: 0.299, 0.587, 0.114


def colour_directions(k=12, seed=0):
    """The projection table of the colour histograms, int16 (4 + k, 3) on the CPU: rows 0-2 the channel axes (4096 on one
    channel), row 3 BT.601 luma, rows 4.. ``k`` seeded random directions, theta normal in float64 (a CPU generator) and
    d = trunc(theta / |theta|_1 * 4096): truncation toward zero keeps sum |d| <= 4096.  Cached per (k, seed); do not write to it."""
    key = (int(k), int(seed))
    if key not in _DIRECTIONS:
        if not 0 <= key[0] <= ops.COLOUR_MAX_DIRS - 4:
            raise ValueError("colour_directions: 0 <= k <= %d, got %r" % (ops.COLOUR_MAX_DIRS - 4, k))
        theta = torch.randn(key[0], 3, generator=torch.Generator().manual_seed(key[1]), dtype=torch.float64)
        rand = torch.trunc(theta / theta.abs().sum(1, keepdim=True) * 4096.0).to(torch.int16)
        _DIRECTIONS[key] = torch.cat((torch.tensor(ops.COLOUR_AXES + (LUMA_601,), dtype=torch.int16), rand), 0)
    return _DIRECTIONS[key]


class ColourStats:
    """What ``colour_stats`` returns: ``hist`` (B, R, P, 256) int32, ``count`` (B, R) int32, ``lab_mean`` (B, R, 3) and
    ``lab_cov`` (B, R, 3, 3) float64 on the device, and the ``dirs`` (P, 3) int16 (CPU) the histograms were taken along."""

    def __init__(self, hist, count, lab_mean, lab_cov, dirs):
        self.hist, self.count, self.lab_mean, self.lab_cov, self.dirs = hist, count, lab_mean, lab_cov, dirs

    def __len__(self):
        return int(self.hist.shape[0])

    def __getitem__(self, idx):
        """the entries ``idx`` (a slice, a list or a tensor of indices) as a ColourStats"""
        if isinstance(idx, (list, tuple)):
            idx = torch.tensor(idx, dtype=torch.int64, device=self.hist.device)
        return ColourStats(self.hist[idx], self.count[idx], self.lab_mean[idx], self.lab_cov[idx], self.dirs)


_COV_INDEX = ((0, 1, 2), (1, 3, 4), (2, 4, 5))          # the six unique entries LL, La, Lb, aa, ab, bb as a 3 x 3


def colour_stats(images, labels=None, regions=1, dirs=None):
    """``images``: uint8 (B, H, W, 3), or fp32 (B, 3, H, W) in [-1, 1] (quantised by ``glue.tensor2im``).  ``labels``: None (one
    region: the image), an integer (B, H, W) map (a value >= ``regions`` -- 255, say -- belongs to no region) or a one-hot
    (B, R, H, W) mask (arg-max).  ``dirs``: ``colour_directions()`` by default.  -> ColourStats."""
    from . import glue
    _on_device(images)
    if images.dtype != torch.uint8:
        images = glue.tensor2im(images)
    if labels is not None:
        _on_device(labels)
        if labels.dim() == 4:
            labels = labels.argmax(dim=1)
        labels = labels.to(torch.uint8)
    dirs = colour_directions() if dirs is None else dirs
    hist, count, mean, cov6 = ops.colour_stats(images, labels, regions, dirs)
    return ColourStats(hist, count, mean, cov6[..., torch.tensor(_COV_INDEX, device=cov6.device)], torch.as_tensor(dirs).cpu())


def _sqrtm_psd(m):
    """the symmetric square root of a batch of 3 x 3 positive semi-definite matrices, float64 on the host"""
    w, v = torch.linalg.eigh(m)
    return (v * w.clamp(min=0.0).sqrt().unsqueeze(-2)) @ v.transpose(-1, -2)


def gaussian_w2_squared(mean_a, cov_a, mean_b, cov_b):
    """|mu_a - mu_b|^2 + tr(Sa + Sb - 2 (Sa^1/2 Sb Sa^1/2)^1/2) of Gaussians (..., 3), (..., 3, 3): float64 on the host (nine
    numbers per entry: two 3 x 3 eigen-decompositions)"""
    mean_a, cov_a, mean_b, cov_b = (t.detach().double().cpu() for t in (mean_a, cov_a, mean_b, cov_b))
    ra = _sqrtm_psd(cov_a)
    cross = _sqrtm_psd(ra @ cov_b @ ra)
    tr = lambda m: m.diagonal(dim1=-2, dim2=-1).sum(-1)
    return ((mean_a - mean_b) ** 2).sum(-1) + tr(cov_a) + tr(cov_b) - 2.0 * tr(cross)


def w1_from_numerators(num, count_a, count_b):
    """W1 in grey levels from ppst_hist_w1's numerators (K, R, P) and the two sides' counts (K, R): float64, NaN where a side is
    empty"""
    den = (count_a.double() * count_b.double()).unsqueeze(-1)
    return torch.where(den > 0, num.double() / den.clamp(min=1.0), torch.full_like(num, float("nan"), dtype=torch.float64))


def colour_distance(stats_a, stats_b, pairs=None):
    """Distances between entry i of ``stats_a`` and entry j of ``stats_b`` for every (i, j) of ``pairs`` (None: n with n), per
    region: {name: float64 (K, R) on the host}.  ``w1_rgb``: mean W1 of the three channel histograms, in levels; ``w1_luma``: W1
    of BT.601 luma; ``swd``: mean over the random directions of W1 * 4096 / |d|_2, a sliced 1-Wasserstein distance in Euclidean
    RGB levels (NaN without random rows); ``delta_e``: CIE76 between the regions' mean Lab; ``frechet``: the Gaussian
    2-Wasserstein distance squared between the regions' Lab Gaussians.  NaN wherever the region is empty on either side."""
    if not torch.equal(stats_a.dirs, stats_b.dirs):
        raise ValueError("colour_distance: the two statistics were taken along different directions")
    if pairs is None:
        if len(stats_a) != len(stats_b):
            raise ValueError("colour_distance without pairs needs as many entries on both sides (%d and %d)" % (len(stats_a), len(stats_b)))
        pairs = [(n, n) for n in range(len(stats_a))]
    pr = torch.as_tensor(pairs).reshape(-1, 2).to(torch.int64).cpu()
    num = ops.hist_w1(stats_a.hist, stats_b.hist, pr)
    ia, ib = pr[:, 0].to(num.device), pr[:, 1].to(num.device)
    ca, cb = stats_a.count[ia], stats_b.count[ib]
    w1 = w1_from_numerators(num, ca, cb).cpu()                                        # (K, R, P)
    d = stats_a.dirs.double()
    P = d.shape[0]
    empty = ((ca == 0) | (cb == 0)).cpu()
    nan = torch.full(empty.shape, float("nan"), dtype=torch.float64)
    out = {"w1_rgb": w1[..., :3].mean(-1) if P >= 3 else nan.clone(),
           "w1_luma": w1[..., 3] if P >= 4 else nan.clone(),
           "swd": (w1[..., 4:] * (4096.0 / d[4:].norm(dim=1))).mean(-1) if P > 4 else nan.clone()}
    ma, mb = stats_a.lab_mean[ia].cpu(), stats_b.lab_mean[ib].cpu()
    out["delta_e"] = torch.where(empty, nan, (ma - mb).norm(dim=-1))
    out["frechet"] = torch.where(empty, nan, gaussian_w2_squared(ma, stats_a.lab_cov[ia], mb, stats_b.lab_cov[ib]))
    return out


# ------------------------------------------------------------------------------------------------- colour-transfer baselines
# What does a CLASSICAL per-region colour transfer score on the same images with the same labels?  The other anchor of the style
# numbers, beside "no transfer at all" (csrc/colour_transfer.hip; include/ppst_hip.h "colour transfer"; DESIGN.md "Colour-transfer
# baselines").  The maps are built from two ColourStats; one HIP pass applies them to the content's pixels.
TRANSFER_METHODS = ("hist", "mkl", "reinhard")


def _pairs_or_diagonal(na, nb, pairs, who):
    if pairs is None:
        if na != nb:
            raise ValueError("%s without pairs needs as many entries on both sides (%d and %d)" % (who, na, nb))
        pairs = [(n, n) for n in range(na)]
    return torch.as_tensor(pairs).reshape(-1, 2).to(torch.int64).cpu()


def gaussian_transfer_rows(mean_c, cov_c, count_c, mean_s, cov_s, count_s, method="mkl", floor=1e-2, max_gain=8.0):
    """The affine rows (T row-major | mu_S - T mu_C) that carry the Gaussian (mean_c, cov_c) onto (mean_s, cov_s): float64 on the
    host, (..., 12).  ``"mkl"``: the Monge-Kantorovich linear map T = Sc^-1/2 (Sc^1/2 Ss Sc^1/2)^1/2 Sc^-1/2 (Pitie & Kokaram
    2007), the optimal transport between the two Gaussians; ``"reinhard"``: T = diag(sigma_S / sigma_C) per Lab axis (Reinhard et
    al. 2001).  ``floor`` is the lower clamp on Sc's eigenvalues (on its variances) before the inverse root, ``max_gain`` the
    upper clamp on T's eigenvalues: both are PARAMETERS that keep a flat region from being amplified without bound, not findings.
    A region that is empty on either side gets the identity row."""
    mean_c, cov_c, mean_s, cov_s = (t.detach().double().cpu() for t in (mean_c, cov_c, mean_s, cov_s))
    if method == "mkl":
        w, v = torch.linalg.eigh(cov_c)
        w = w.clamp(min=floor)
        root = (v * w.sqrt().unsqueeze(-2)) @ v.transpose(-1, -2)
        iroot = (v * w.rsqrt().unsqueeze(-2)) @ v.transpose(-1, -2)
        T = iroot @ _sqrtm_psd(root @ cov_s @ root) @ iroot
        T = 0.5 * (T + T.transpose(-1, -2))
        w, v = torch.linalg.eigh(T)
        T = (v * w.clamp(max=max_gain).unsqueeze(-2)) @ v.transpose(-1, -2)
    elif method == "reinhard":
        var_c, var_s = cov_c.diagonal(dim1=-2, dim2=-1), cov_s.diagonal(dim1=-2, dim2=-1)
        T = torch.diag_embed((var_s.clamp(min=0.0) / var_c.clamp(min=floor)).sqrt().clamp(max=max_gain))
    else:
        raise ValueError("gaussian_transfer_rows: method 'mkl' or 'reinhard', got %r" % (method,))
    off = mean_s - (T @ mean_c.unsqueeze(-1)).squeeze(-1)
    rows = torch.cat((T.flatten(-2), off), -1)
    eye = torch.cat((torch.eye(3, dtype=torch.float64).flatten(), torch.zeros(3, dtype=torch.float64)))
    empty = ((count_c == 0) | (count_s == 0)).cpu().unsqueeze(-1)
    return torch.where(empty, eye.expand_as(rows), rows)


def colour_transfer_maps(stats_c, stats_s, method, pairs=None, floor=1e-2, max_gain=8.0):
    """The maps that carry entry i of ``stats_c`` (the content) onto entry j of ``stats_s`` (the style) for every (i, j) of
    ``pairs`` (None: n with n), per region.  ``"hist"``: uint8 (K, R, 3, 256) tables (``ops.hist_match_lut``; the statistics must
    have been taken with ``ops.COLOUR_AXES`` as their first three directions); ``"mkl"`` / ``"reinhard"``: fp32 (K, R, 12) rows
    (``gaussian_transfer_rows``; ``floor`` = 1e-2, the lower clamp on the content covariance's eigenvalues, and ``max_gain`` = 8,
    the upper clamp on the map's, are parameters, not findings).  On the statistics' device."""
    if method not in TRANSFER_METHODS:
        raise ValueError("colour_transfer_maps: method one of %s, got %r" % (TRANSFER_METHODS, method))
    pr = _pairs_or_diagonal(len(stats_c), len(stats_s), pairs, "colour_transfer_maps")
    if method == "hist":
        axes = torch.tensor(ops.COLOUR_AXES, dtype=torch.int16)
        for st in (stats_c, stats_s):
            if st.dirs.shape[0] < 3 or not torch.equal(st.dirs[:3].to(torch.int16), axes):
                raise ValueError("colour_transfer_maps('hist') needs statistics whose first three directions are ops.COLOUR_AXES")
        return ops.hist_match_lut(stats_c.hist, stats_s.hist, pr)
    dev = stats_c.hist.device
    ic, js = pr[:, 0].to(dev), pr[:, 1].to(dev)
    rows = gaussian_transfer_rows(stats_c.lab_mean[ic], stats_c.lab_cov[ic], stats_c.count[ic], stats_s.lab_mean[js],
                                  stats_s.lab_cov[js], stats_s.count[js], method, floor, max_gain)
    return rows.float().to(dev)


def region_weights(labels, regions, feather):
    """fp32 (B, R, H, W): one ``ops.label_matte(labels, keep=(r,), feather, grow=feather // 2)`` per region"""
    return torch.stack([ops.label_matte(labels, keep=(r,), feather=feather, grow=feather // 2) for r in range(regions)], 1)


def colour_transfer(contents, style_stats, content_labels=None, method="hist", regions=1, pairs=None, feather=0, floor=1e-2,
                    max_gain=8.0, content_stats=None):
    """Content i re-coloured towards entry j of ``style_stats`` for every (i, j) of ``pairs`` (None: n with n), per region of the
    content's labels: uint8 (K, H, W, 3).  ``contents`` / ``content_labels`` as ``colour_stats`` takes them; ``regions`` must be
    that of ``style_stats``.  It takes the contents' statistics (or ``content_stats``, if the caller has them), builds the maps
    (``colour_transfer_maps``) and applies them (``ops.colour_transfer_apply``).  ``feather`` > 0: the regions blend through
    feathered mattes of the label map (``region_weights``) instead of switching at the label boundary."""
    from . import glue
    _on_device(contents)
    if contents.dtype != torch.uint8:
        contents = glue.tensor2im(contents)
    lab = content_labels
    if lab is not None:
        _on_device(lab)
        if lab.dim() == 4:
            lab = lab.argmax(dim=1)
        lab = lab.to(torch.uint8)
    R = int(regions)
    if style_stats.hist.shape[1] != R:
        raise ValueError("colour_transfer: the style statistics have %d regions, not %d" % (style_stats.hist.shape[1], R))
    if content_stats is None:
        content_stats = colour_stats(contents, lab, R, style_stats.dirs)
    pr = _pairs_or_diagonal(len(content_stats), len(style_stats), pairs, "colour_transfer")
    maps = colour_transfer_maps(content_stats, style_stats, method, pr, floor, max_gain)
    idx = pr[:, 0].to(contents.device)
    diagonal = pr[:, 0].tolist() == list(range(contents.shape[0]))
    u8 = contents if diagonal else contents[idx]
    lab_k = lab if lab is None or diagonal else lab[idx]
    weights = None
    if feather > 0 and lab is not None:
        w = region_weights(lab.contiguous(), R, int(feather))
        weights = w if diagonal else w[idx]
    key = "luts" if method == "hist" else "affine"
    return ops.colour_transfer_apply(u8, lab_k, weights=weights, **{key: maps})
