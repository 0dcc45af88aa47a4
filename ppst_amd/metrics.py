"""Image-quality metrics on the HIP path (csrc/ssim.hip; include/ppst_hip.h "image-quality metrics"): PSNR, SSIM (Wang et al.
2004: 11-tap Gaussian window, sigma 1.5, valid) and five-scale MS-SSIM (Wang et al. 2003).  They need no weights and are defined
by published formulas, so they are held to float64 restatements of exactly those (tests/ssim_cases.py).

Images are fp32 (B, C, H, W) in any layout, or uint8 (B, H, W, C) as ``glue.tensor2im`` / ``evaluation.to_uint8_image`` make
them.  ``data_range`` defaults to 2.0 for float tensors (the model's [-1, 1]) and to 255 for uint8.  Every function returns one
fp32 number per image, (B,).  ``ssim`` is differentiable in its FIRST argument (fp32 only); MS-SSIM and PSNR are forward only.
There is no CPU fallback: CPU tensors raise RuntimeError.
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
