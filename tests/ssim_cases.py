"""Case table of the image-quality metrics (csrc/ssim.hip): shapes, seeded inputs and the float64 judge -- a restatement of the
definitions in include/ppst_hip.h ("image-quality metrics") with F.conv2d on the separable window, autograd for the gradient.
Importing this needs no GPU.  test_ssim_cpu.py pins the judge itself (a second, loop-written form; closed forms; central
differences); test_gpu_ssim.py holds the kernels to it.

The bar of a GPU check is the project's convention for fp32 streaming kernels (tests/BACKWARD_KERNELS.md section 3):
``bar = max(2e-6, 4 x the error of the float32 torch evaluation of this same judge against its float64 evaluation)``.
"""
import math

import torch
import torch.nn.functional as F

MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
TILE = 32          # SS_T of csrc/ssim.hip: the forward kernel tiles the valid grid, the gradient kernel the image

# (name, B, C, H, W): the smallest shapes that reach every path of the kernels.  Which edge each one reaches:
SSIM_SHAPES = [
    ("11x11", 2, 3, 11, 11),          # one valid pixel: every staged pixel but the window's is beyond the valid grid
    ("12x75", 3, 3, 12, 75),          # valid grid 2 x 65: three tiles wide (the last one a single column), odd batch
    ("23x27-c1", 2, 1, 23, 27),       # one channel: plane index == image index
    ("64x64", 2, 3, 64, 64),          # valid grid 54 x 54: 2 x 2 tiles, every one cut; gradient tiles exactly full
    ("42x42", 1, 2, 42, 42),          # valid grid == one full tile: nothing is masked
    ("43x21", 2, 2, 43, 21),          # H - 10 == tile + 1: a second tile row of one valid row
    ("21x43", 2, 2, 21, 43),          # W - 10 == tile + 1: a second tile column of one valid column
    ("33x70", 2, 3, 33, 70),          # gradient kernel: image rows == tile + 1 (also the non-contiguous case's shape)
]
MS_SHAPES = [("176x177", 2, 3, 176, 177),      # the smallest size; odd width: every pool drops a column (177 -> 88 -> 44 -> 22 -> 11)
             ("191x240-c1", 1, 1, 191, 240)]   # odd height at scales 1, 2, 3 (191 -> 95 -> 47 -> 23 -> 11)
U8_SHAPE = ("u8-40x52", 2, 3, 40, 52)
NOISE_LEVELS = (0.02, 0.15, 1.0)                # image n of a batch gets level n % 3: SSIM from about 0.99 down to about 0.04


def window(dtype=torch.float64):
    """11 taps exp(-(i - 5)^2 / (2 * 1.5^2)), normalised in float64, rounded ONCE to fp32 (the kernel's constants)"""
    i = torch.arange(11, dtype=torch.float64)
    g = torch.exp(-(i - 5.0) ** 2 / (2.0 * 1.5 ** 2))
    return (g / g.sum()).float().to(dtype)


def make_pair(seed, B, C, H, W):
    """a = a smooth random field plus a little noise, clamped to [-1, 1]; b = a plus noise at the image's level, clamped (fp32)"""
    gen = torch.Generator().manual_seed(seed)
    coarse = torch.randn(B, C, H // 8 + 3, W // 8 + 3, generator=gen, dtype=torch.float64)
    a = 0.6 * F.interpolate(coarse, size=(H, W), mode="bicubic", align_corners=True)
    a = (a + 0.05 * torch.randn(B, C, H, W, generator=gen, dtype=torch.float64)).clamp(-1.0, 1.0)
    lev = torch.tensor([NOISE_LEVELS[n % 3] for n in range(B)], dtype=torch.float64).view(B, 1, 1, 1)
    b = (a + lev * torch.randn(B, C, H, W, generator=gen, dtype=torch.float64)).clamp(-1.0, 1.0)
    return a.float(), b.float()


def to_u8(x):
    """(B, C, H, W) in [-1, 1] -> uint8 (B, H, W, C), the layout glue.tensor2im / evaluation.to_uint8_image produce"""
    return ((x.clamp(-1.0, 1.0) + 1.0) * 127.5).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def from_u8(u):
    """uint8 (B, H, W, C) -> the raw values as (B, C, H, W) float64: the judge runs on them at L = 255"""
    return u.permute(0, 3, 1, 2).double()


# ------------------------------------------------------------------------------------------------------------ the judge
def _filter(x, g):
    C = x.shape[1]
    x = F.conv2d(x, g.view(1, 1, 1, 11).expand(C, 1, 1, 11), groups=C)
    return F.conv2d(x, g.view(1, 1, 11, 1).expand(C, 1, 11, 1), groups=C)


def ssim_maps(a, b, L):
    """-> (ssim map, cs map), (B, C, H - 10, W - 10), in the dtype of ``a``"""
    if a.shape[-2] < 11 or a.shape[-1] < 11:
        raise ValueError("SSIM needs at least 11 x 11 pixels")
    g = window(a.dtype)
    C1, C2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    mu_a, mu_b = _filter(a, g), _filter(b, g)
    s_a = _filter(a * a, g) - mu_a * mu_a
    s_b = _filter(b * b, g) - mu_b * mu_b
    s_ab = _filter(a * b, g) - mu_a * mu_b
    cs = (2.0 * s_ab + C2) / (s_a + s_b + C2)
    return (2.0 * mu_a * mu_b + C1) / (mu_a * mu_a + mu_b * mu_b + C1) * cs, cs


def ssim(a, b, L):
    return ssim_maps(a, b, L)[0].mean(dim=(1, 2, 3))


def ssim_grad(a, b, gout, L):
    """d(sum_b gout[b] ssim[b]) / d a by autograd"""
    a = a.clone().requires_grad_(True)
    (ssim(a, b, L) * gout.to(a.dtype)).sum().backward()
    return a.grad


def ms_ssim(a, b, L):
    if min(a.shape[-2:]) < 176:
        raise ValueError("MS-SSIM needs at least 176 x 176 pixels")
    prod = None
    for j, w in enumerate(MS_WEIGHTS):
        s, cs = ssim_maps(a, b, L)
        v = (s if j == 4 else cs).mean(dim=(2, 3)).clamp(min=0.0) ** w
        prod = v if prod is None else prod * v
        if j < 4:
            a, b = F.avg_pool2d(a, 2), F.avg_pool2d(b, 2)
    return prod.mean(dim=1)


def mse(a, b):
    return ((a - b) ** 2).mean(dim=(1, 2, 3))


def l1(a, b):
    return (a - b).abs().mean(dim=(1, 2, 3))


def psnr(a, b, L):
    m = mse(a, b)
    return torch.where(m > 0, 10.0 * torch.log10(L * L / m.clamp(min=1e-300)), torch.full_like(m, math.inf))


# ------------------------------------------------------------------------------------------------------------ the bar
def bar_from(ref64, val32, relative=False):
    """max(2e-6, 4 x |float32 torch evaluation - float64 evaluation|), the error relative to max |ref| where ``relative``"""
    err = (val32.double() - ref64).abs().max().item()
    if relative:
        err /= max(ref64.abs().max().item(), 1e-300)
    return max(2e-6, 4.0 * err)


def error_of(ref64, got, relative=False):
    err = (got.double().cpu() - ref64).abs().max().item()
    if relative:
        err /= max(ref64.abs().max().item(), 1e-300)
    return err
