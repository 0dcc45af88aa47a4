"""CPU: the host side of swaps above 512 x 512 -- the fp32 tables of the antialiased bicubic resample against float64, the
argument checks of ppst_resample_f32 (validation runs before anything is dereferenced or launched) and the size rule of the
correspondence image."""
import ctypes

import numpy as np
import pytest
import torch

# (in, out): 2:1, non-integer reductions with windows clipped at both borders, upsample, a single output, a copied axis
SIZES = [(64, 32), (37, 16), (53, 24), (40, 13), (24, 48), (8, 1), (70, 70)]


def _apply(x, ksize, bounds, coef):
    """The tables applied along the last axis in float64: y[..., i] = sum_k x[..., first_i + k] * coef[i, k]."""
    y = np.zeros(x.shape[:-1] + (bounds.shape[0],), dtype=np.float64)
    for i, (first, n) in enumerate(bounds):
        assert 0 <= first and 0 < n <= ksize and first + n <= x.shape[-1]
        y[..., i] = (x[..., first:first + n] * coef[i, :n].astype(np.float64)).sum(-1)
    return y


@pytest.mark.parametrize("n_in,n_out", SIZES)
def test_fp32_tables_against_float64_antialiased_bicubic(n_in, n_out):
    from ppst_amd import imageio
    ksize, bounds, coef = imageio.resample_weights_f32(n_in, n_out)
    assert coef.dtype == np.float32 and coef.shape == (n_out, ksize) and bounds.shape == (n_out, 2)
    assert np.abs(coef.astype(np.float64).sum(1) - 1.0).max() < 1e-6          # normalised per output position
    assert not coef[np.arange(ksize)[None, :] >= bounds[:, 1:2]].any()        # zero behind each window
    x = torch.from_numpy(np.random.default_rng(n_in * 1000 + n_out).uniform(-1, 1, size=(2, 3, 5, n_in)))
    judge = torch.nn.functional.interpolate(x.double(), size=(5, n_out), mode="bicubic", antialias=True, align_corners=False)
    err = np.abs(_apply(x.numpy(), ksize, bounds, coef) - judge.numpy()).max()
    print("tables %d -> %d: ksize %d, max |err| %.3e" % (n_in, n_out, ksize, err))
    assert err <= 1e-6
    # the other axis goes through the same tables
    xt = x.transpose(2, 3).contiguous()
    judge_t = torch.nn.functional.interpolate(xt.double(), size=(n_out, 5), mode="bicubic", antialias=True, align_corners=False)
    got_t = np.swapaxes(_apply(np.swapaxes(xt.numpy(), 2, 3), ksize, bounds, coef), 2, 3)
    assert np.abs(got_t - judge_t.numpy()).max() <= 1e-6


def test_resample_f32_argument_errors_need_no_gpu():
    from ppst_amd._lib import lib
    d = ctypes.c_void_p(16)       # a non-null token: nothing is dereferenced before the checks pass
    f = lambda x, y, B, ih, iw, oh, ow, kh=9, kv=9, t=d, clamp=0, lo=0.0, hi=0.0: lib.ppst_resample_f32(
        x, y, B, ih, iw, oh, ow, t, t, kh, t, t, kv, clamp, lo, hi, None)
    # bad sizes -> PPST_EINVAL, before the empty batch and the null checks
    assert f(d, d, -1, 64, 64, 32, 32) == -1
    assert f(d, d, 1, 0, 64, 32, 32) == -1 and f(d, d, 1, 64, 64, 32, 0) == -1
    assert f(None, None, 0, 64, 64, 0, 32) == -1
    assert f(d, d, 1, 64, 64, 32, 32, kh=0) == -1 and f(d, d, 1, 64, 64, 32, 32, kv=-3) == -1
    assert f(d, d, 1, 64, 64, 32, 32, clamp=1, lo=1.0, hi=-1.0) == -1
    assert f(d, d, 1 << 20, 64, 64, 32, 32) == -1                 # 2^32 input elements: beyond the 32-bit index limit
    # empty batch -> PPST_OK, whatever the pointers
    assert f(None, None, 0, 64, 64, 32, 32, t=None) == 0
    # null data -> PPST_ENULL: images, or the tables of an axis that is filtered
    assert f(None, d, 1, 64, 64, 32, 32) == -3 and f(d, None, 1, 64, 64, 32, 32) == -3
    assert f(d, d, 1, 64, 64, 32, 32, t=None) == -3
    assert f(d, d, 1, 64, 64, 32, 64, t=None) == -3               # horizontal copy, vertical tables still needed
    # over-long filter -> PPST_EINVAL: min(in_h, 15 * in_h / out_h + ksize_v + 1) must be at most 192 rows of LDS
    from ppst_amd import imageio
    ksize = imageio.bicubic_windows(8192, 16)[0]
    assert ksize == 2049
    assert f(d, d, 1, 8192, 64, 16, 32, kv=ksize) == -1
    assert f(None, None, 0, 8192, 64, 16, 32, kv=ksize) == -1     # ... before the empty batch
    assert f(d, d, 1, 193, 64, 1, 32, kv=775) == -1               # one row over
    assert f(None, d, 1, 192, 64, 1, 32, kv=771) == -3            # fits (the whole image): goes on to the null check
    assert f(None, d, 1, 64, 8192, 32, 16, kh=ksize) == -3        # the horizontal filter needs no LDS: any length
    assert f(None, d, 1, 1024, 1024, 128, 128, kh=33, kv=33) == -3   # 8 : 1 fits


def test_resize_tensor_refuses_cpu_tensors():
    from ppst_amd import imageio, ops
    x = torch.zeros(1, 3, 8, 8)
    with pytest.raises(RuntimeError):
        ops.resample_f32(x, 4, 4)
    with pytest.raises(RuntimeError):
        imageio.resize_tensor(x, 4, 4, clamp=(-1, 1))


def test_correspondence_size_rule():
    from ppst_amd.ppst_model import CORR_MAX_SIDE, PPSTModel, correspondence_side
    x = torch.zeros(1, 3, 512, 512)
    assert PPSTModel.correspondence_image(None, x) is x           # 512: the same object, nothing runs
    assert correspondence_side(1024, 1024) == 512 and correspondence_side(1536, 1536) == 512
    assert CORR_MAX_SIDE == 1536 and (CORR_MAX_SIDE + 512) ** 2 * 128 * 4 >= 2 ** 31 > CORR_MAX_SIDE ** 2 * 128 * 4
    for h, w in ((768, 768), (1024, 512), (512, 1024), (2048, 2048), (256, 256)):
        with pytest.raises(ValueError, match="multiple of 512"):
            correspondence_side(h, w)
        with pytest.raises(ValueError, match="multiple of 512"):
            PPSTModel.correspondence_image(None, torch.empty(1, 3, h, w))
    # an accepted size gets past the rule and reaches the resample, which has no CPU form
    with pytest.raises(RuntimeError, match="CUDA"):
        PPSTModel.correspondence_image(None, torch.empty(1, 3, 1024, 1024))


def test_multi_rank_grid_above_512_is_refused_from_shapes_alone():
    from ppst_amd.evaluation import swapping_grid
    cs, ss = torch.empty(2, 3, 1024, 1024), torch.empty(2, 3, 1024, 1024)
    for rank in range(2):         # every rank decides alike, before the model or a collective is touched
        with pytest.raises(ValueError, match="one rank"):
            swapping_grid(None, cs, ss, rank=rank, world=2)
    with pytest.raises(ValueError, match="one rank"):
        swapping_grid(None, torch.empty(1, 3, 512, 512), ss, rank=0, world=4)
