"""GPU: the encoders' first ResBlock as one LDS-resident kernel (ops.encoder_resblock, ppst_encoder_resblock) -- pytest -m gpu.

Judge: the unfused formula of BaseNetwork.res_block(norm=False) in float64 on the CPU -- reflect pad + conv1 + fused leaky ReLU, the
[1,2,1]^2 blur as a depthwise conv on the reflect pad (2, 1), the stride-2 conv2 + fused leaky ReLU, the skip as the blur on the zero
pad (1, 0) keeping every second sample and the 1x1 conv, (main + skip) / sqrt 2 -- with the weights and biases that
weights.make_state_dict(0, bias_std=0.1) draws for E2.DownToGlobalCode1.ResBlockDownBy1.* and E1.DownToSpatialCode.ResBlockDownBy1.*
(E1's block carries an InstanceNorm in the network; here its weights are a second draw for the same no-norm formula) and seeded
normal inputs.
Bar: e_new = max |fused - f64| <= 2 e_old = 2 max |existing path - f64|, both taken in the same run (the rule of
tests/test_gpu_torgb_linear.py): conv2's nine taps are summed ky-major where the space-to-depth form groups them by phase, a
reassociated fp32 sum and nothing more.  Both errors and max |f64| are printed (pytest -s).  The existing path is res_block with
grad enabled, which never takes the fused entry.
Shapes (B = 2, tile = 8 x 8 outputs = 16 x 16 input pixels): 4 x 4 -- both reflections of a row land inside a three-row image
interior; 16 x 16 -- one tile touching all four borders; 12 x 20 -- ragged last tile in both axes, image shorter than a tile in y;
40 x 24 -- an interior tile in y with border tiles around it; 18 x 34 -- one ragged row and column of tiles, two pixels wide.
Only the E2 (no-norm) form of the kernel exists: the statistics / norm forms for E1's block are not built, so there is nothing of
theirs to test."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
SQRT2 = math.sqrt(2.0)
BLOCKS = {"E2": "E2.DownToGlobalCode1.ResBlockDownBy1.", "E1": "E1.DownToSpatialCode.ResBlockDownBy1."}
SHAPES = [(4, 4), (16, 16), (12, 20), (40, 24), (18, 34)]
_CACHE = {}


def _dev():
    return torch.device("cuda", 0)


def _ops():
    from ppst_amd import ops
    return ops


def _sd():
    if "sd" not in _CACHE:
        from ppst_amd import weights
        _CACHE["sd"] = weights.make_state_dict(0, with_D=False, with_nce=False, bias_std=0.1, prefixes=["E1.", "E2."])
    return _CACHE["sd"]


def _net(which):
    """the encoder that owns the block, on the GPU, with the state dict's weights"""
    if which not in _CACHE:
        from ppst_amd.networks.encoder_col import StyleGAN2ResnetEncodercol
        from ppst_amd.networks.encoder_con import StyleGAN2ResnetEncodercon
        net = (StyleGAN2ResnetEncodercol if which == "E2" else StyleGAN2ResnetEncodercon)()
        net.load_state_dict({k[3:]: v for k, v in _sd().items() if k.startswith(which + ".")})
        _CACHE[which] = net.to(_dev())
    return _CACHE[which]


def _x(H, W, B=2, c=32):
    return torch.randn(B, H, W, c, generator=torch.Generator().manual_seed(100 * H + W))


def _judge(which, x):
    """x (B,H,W,32) fp32 on the CPU -> the block's output (B,H/2,W/2,64) in float64"""
    sd, p, f64 = _sd(), BLOCKS[which], torch.float64
    w1, w2, ws = (sd[p + n + ".Conv.weight"].to(f64) for n in ("conv1", "conv2", "skip"))
    b1, b2 = (sd[p + n + ".Act.bias"].to(f64).reshape(1, -1, 1, 1) for n in ("conv1", "conv2"))
    cin = w1.shape[1]

    def fir(t, name):
        k = sd[p + name + ".Blur.kernel"].to(f64).flip(0, 1)
        return F.conv2d(t, k[None, None].expand(t.shape[1], 1, 3, 3).contiguous(), groups=t.shape[1])
    xn = x.to(f64).permute(0, 3, 1, 2)
    y1 = F.leaky_relu(F.conv2d(F.pad(xn, (1, 1, 1, 1), mode="reflect"), w1 / math.sqrt(cin * 9)) + b1, 0.2) * SQRT2
    y2 = F.leaky_relu(F.conv2d(fir(F.pad(y1, (2, 1, 2, 1), mode="reflect"), "conv2"), w2 / math.sqrt(cin * 9), stride=2) + b2, 0.2) * SQRT2
    skip = F.conv2d(fir(F.pad(xn, (1, 0, 1, 0)), "skip")[:, :, ::2, ::2], ws / math.sqrt(cin))
    return ((y2 + skip) / SQRT2).permute(0, 2, 3, 1).contiguous()


class _Count:
    """counts the calls of ops.encoder_resblock inside the block"""

    def __enter__(self):
        ops = _ops()
        self.n, self.orig = 0, ops.encoder_resblock

        def counted(*a, **k):
            self.n += 1
            return self.orig(*a, **k)
        ops.encoder_resblock = counted
        return self

    def __exit__(self, *exc):
        _ops().encoder_resblock = self.orig


def _block(which, x, fused):
    """res_block of the owning encoder on x (GPU): fused -> inference mode (the fused entry where eligible), else grad enabled"""
    ops, net = _ops(), _net(which)
    p = BLOCKS[which][3:]
    with (torch.no_grad() if fused else torch.enable_grad()):
        return net.res_block(x, p, ops.PAD_REFLECT, norm=False)


@pytest.mark.parametrize("which", list(BLOCKS))
@pytest.mark.parametrize("H,W", SHAPES, ids=lambda v: str(v))
def test_fused_block_vs_float64(which, H, W):
    x = _x(H, W)
    ref = _judge(which, x)
    xd = x.to(_dev())
    with _Count() as c:
        new = _block(which, xd, True)
        assert c.n == 1, "inference mode did not take the fused entry"
        old = _block(which, xd, False)
        assert c.n == 1, "the grad-enabled path took the fused entry"
    torch.cuda.synchronize()
    assert new.shape == (2, H // 2, W // 2, 64) and old.shape == new.shape
    e_new = (new.double().cpu() - ref).abs().max().item()
    e_old = (old.double().cpu() - ref).abs().max().item()
    print("encoder block %s B2 %dx%d: max abs err fused %.3e existing %.3e (|f64| max %.3f) fused==existing: %s"
          % (which, H, W, e_new, e_old, ref.abs().max().item(), torch.equal(new, old)))
    assert e_new <= 2.0 * e_old, "fused %.3e > 2 x existing %.3e" % (e_new, e_old)


def _plans(net, p, cin):
    sc1, scs = 1.0 / math.sqrt(cin * 9), 1.0 / math.sqrt(cin)
    return (net.plan(p + "conv1.Conv.weight", scale=sc1), net.plan(p + "conv2.Conv.weight", scale=sc1), net.plan(p + "skip.Conv.weight", scale=scs),
            net.p(p + "conv1.Act.bias"), net.p(p + "conv2.Act.bias"), net.p(p + "conv2.Blur.kernel"))


def _outcome(fn):
    try:
        out = fn()
        torch.cuda.synchronize()
        return ("ok", out)
    except Exception as e:
        return ("raised", type(e))


REFUSED = {          # (views are taken on the device: a copy to it would be dense again)
    "odd_H": lambda d: _x(5, 8).to(d),
    "H_below_4": lambda d: _x(2, 8).to(d),
    "channel_slice": lambda d: _x(8, 8, c=64).to(d)[..., :32],
    "strided_rows": lambda d: _x(16, 8).to(d)[:, ::2],
    "half": lambda d: _x(8, 8).to(d).half(),
    "channels_64_64_128": lambda d: _x(8, 8, c=64).to(d),
}


@pytest.mark.parametrize("case", list(REFUSED))
def test_entry_refuses_and_res_block_keeps_the_existing_path(case):
    ops, net = _ops(), _net("E2")
    x = REFUSED[case](_dev())
    assert case not in ("channel_slice", "strided_rows") or not x.is_contiguous()
    second = case == "channels_64_64_128"
    p = "DownToGlobalCode1.ResBlockDownBy%d." % (2 if second else 1)
    with torch.no_grad():
        assert ops.encoder_resblock_ok(_x(8, 8).to(_dev()), 32, 64)
        assert not ops.encoder_resblock_ok(x, 64 if second else 32, 128 if second else 64)
    with pytest.raises(RuntimeError, match="PPST_EINVAL"):
        ops.encoder_resblock(x, *_plans(net, p, x.shape[3]))
    with _Count() as c:
        got = _outcome(lambda: _block_at(net, x, p, True))
        want = _outcome(lambda: _block_at(net, x, p, False))
        assert c.n == 0
    assert got[0] == want[0]
    if got[0] == "ok":
        assert torch.equal(got[1], want[1])
    else:
        assert got[1] is want[1]


def _block_at(net, x, p, inference):
    with (torch.no_grad() if inference else torch.enable_grad()):
        return net.res_block(x, p, _ops().PAD_REFLECT, norm=False)


def test_encode_takes_the_fused_entry_in_mode_0_only():
    from ppst_amd import weights
    from ppst_amd.ppst_model import create_model
    ops = _ops()
    sd = weights.make_state_dict(0, with_D=False, with_nce=False, bias_std=0.1)
    img = weights.synthetic_images(0, 1, size=128).to(_dev())
    calls = {}
    try:
        for mode in (0, 1, 3):
            ops.set_precision(mode)
            m = create_model(state_dict=sd, device=_dev())
            with _Count() as c, torch.no_grad():
                m(img, command="encode")
            torch.cuda.synchronize()
            calls[mode] = c.n
    finally:
        ops.set_precision(0)
    assert calls == {0: 1, 1: 0, 3: 0}, calls
