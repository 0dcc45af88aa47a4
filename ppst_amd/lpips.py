"""LPIPS v0.1, net='alex' -- the metric of the reference's Cycwarp loss (models/ppst_model.py:61, :175-179) -- on the HIP path
(csrc/lpips.hip): ``lpips=True, spatial=False, normalize=False``, eval mode.

    x' = (x - shift) / scale;  relu1..relu5 of torchvision's AlexNet ``features``;
    per layer  n(f) = f / (sqrt(sum_c f^2) + 1e-10),  s_l = mean_hw sum_c lin_l[c] (n(fa) - n(fb))^2;   result sum_l s_l, (B,1,1,1)

The weights are frozen and come from a state dict in the ``lpips`` package's layout -- every checkpoint the reference writes
carries one under ``loss_fn_alex.`` because the metric is an attribute of its model.  Neither the package nor its weights ship
with this project: parity with the PUBLISHED weights is unpinned; the arithmetic is tested against a float64 restatement of the
definition above with synthetic weights (tests/test_gpu_lpips.py).

The module is deliberately NOT an nn.Module: hung on a PPSTModel it must add no key to the checkpoint contract.
"""
import torch

from . import ops

CHANNELS = ops.LPIPS_CHANNELS
_CIN = (3, 64, 192, 384, 256)
_K = (11, 5, 3, 3, 3)
_SLICE = ((1, 0), (2, 3), (3, 6), (4, 8), (5, 10))      # (lpips slice, torchvision features index) of the five convs
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)


def _pick(sd, prefix, names, shape, what):
    """the tensor stored under one of ``names`` (all spellings of one tensor); every spelling present must hold the same values"""
    found = [(n, sd[prefix + n]) for n in names if prefix + n in sd]
    if not found:
        raise KeyError("LPIPS state dict lacks %s: no key %s" % (what, " / ".join(repr(prefix + n) for n in names)))
    for n, t in found:
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(shape):
            raise ValueError("LPIPS key %r: shape %s, expected %s" % (prefix + n, tuple(getattr(t, "shape", ())), tuple(shape)))
    n0, t0 = found[0]
    for n, t in found[1:]:
        if not torch.equal(t.detach().cpu().float(), t0.detach().cpu().float()):
            raise ValueError("LPIPS keys %r and %r both exist and differ" % (prefix + n0, prefix + n))
    return n0, t0.detach().cpu().float().contiguous()


class LPIPSAlex:
    """``metric(a, b) -> (B,1,1,1)`` for fp32 (B,3,H,W) device tensors (images in [-1, 1], at least 31 x 31), differentiable in
    both (first order).  ``metric.features(x)`` -> the five post-ReLU maps, NCHW fp32."""

    def __init__(self, weights, biases, lins, shift, scale):
        self.weights, self.biases, self.lins, self.shift, self.scale = list(weights), list(biases), list(lins), shift, scale
        self._packs = {}

    # ---- loading -------------------------------------------------------------------------------------------------------
    @classmethod
    def from_state_dict(cls, sd, prefix=""):
        """Keys (after ``prefix``): ``scaling_layer.shift|scale`` (1,3,1,1); the convs as ``net.slice<s>.<i>.weight|bias`` (the
        lpips package) or ``features.<i>.weight|bias`` (torchvision); ``lin<l>.model.1.weight`` or ``lins.<l>.model.1.weight``
        (1,C_l,1,1).  Where two spellings of a tensor exist they must agree.  A missing key, a wrong shape and a NEGATIVE lin
        weight are errors that name the key: the arithmetic would run with a negative weight, but the published ones are
        non-negative (the metric is a weighted sum of squares) and a negative one means the file is not an LPIPS state dict."""
        _, shift = _pick(sd, prefix, ["scaling_layer.shift"], (1, 3, 1, 1), "the scaling layer's shift")
        _, scale = _pick(sd, prefix, ["scaling_layer.scale"], (1, 3, 1, 1), "the scaling layer's scale")
        if bool((scale == 0).any()):
            raise ValueError("LPIPS key %r holds a zero" % (prefix + "scaling_layer.scale"))
        ws, bs, ls = [], [], []
        for l, (s, i) in enumerate(_SLICE):
            C, cin, k = CHANNELS[l], _CIN[l], _K[l]
            ws.append(_pick(sd, prefix, ["net.slice%d.%d.weight" % (s, i), "features.%d.weight" % i], (C, cin, k, k), "conv %d weight" % (l + 1))[1])
            bs.append(_pick(sd, prefix, ["net.slice%d.%d.bias" % (s, i), "features.%d.bias" % i], (C,), "conv %d bias" % (l + 1))[1])
            name, lin = _pick(sd, prefix, ["lin%d.model.1.weight" % l, "lins.%d.model.1.weight" % l], (1, C, 1, 1), "lin %d weight" % l)
            if bool((lin < 0).any()):
                raise ValueError("LPIPS key %r has a negative weight" % (prefix + name))
            ls.append(lin.reshape(C).contiguous())
        return cls(ws, bs, ls, shift.reshape(3).contiguous(), scale.reshape(3).contiguous())

    @classmethod
    def from_checkpoint(cls, path, prefix="loss_fn_alex."):
        """A flat checkpoint of the reference's layout: the metric's tensors sit under ``loss_fn_alex.`` beside the model's."""
        sd = torch.load(path, map_location="cpu", weights_only=True)
        return cls.from_state_dict(sd, prefix=prefix)

    @staticmethod
    def synthetic_state_dict(seed):
        """Seeded stand-in weights in the lpips package's key layout (tests, timing): one generator, float64 draws in layer order
        weight, bias, lin -- conv weight randn * sqrt(2 / (Cin k^2)), bias randn * 0.1, lin |randn| / C -- stored as fp32."""
        g = torch.Generator().manual_seed(int(seed))
        sd = {"scaling_layer.shift": torch.tensor(SHIFT, dtype=torch.float32).view(1, 3, 1, 1),
              "scaling_layer.scale": torch.tensor(SCALE, dtype=torch.float32).view(1, 3, 1, 1)}
        for l, (s, i) in enumerate(_SLICE):
            C, cin, k = CHANNELS[l], _CIN[l], _K[l]
            w = torch.randn(C, cin, k, k, generator=g, dtype=torch.float64) * (2.0 / (cin * k * k)) ** 0.5
            b = torch.randn(C, generator=g, dtype=torch.float64) * 0.1
            lin = torch.randn(1, C, 1, 1, generator=g, dtype=torch.float64).abs() / C
            sd["net.slice%d.%d.weight" % (s, i)] = w.float()
            sd["net.slice%d.%d.bias" % (s, i)] = b.float()
            sd["lin%d.model.1.weight" % l] = lin.float()
        return sd

    def state_dict(self, prefix=""):
        """the tensors under the lpips package's names (what from_state_dict reads back)"""
        sd = {prefix + "scaling_layer.shift": self.shift.view(1, 3, 1, 1).clone(), prefix + "scaling_layer.scale": self.scale.view(1, 3, 1, 1).clone()}
        for l, (s, i) in enumerate(_SLICE):
            sd[prefix + "net.slice%d.%d.weight" % (s, i)] = self.weights[l].clone()
            sd[prefix + "net.slice%d.%d.bias" % (s, i)] = self.biases[l].clone()
            sd[prefix + "lin%d.model.1.weight" % l] = self.lins[l].view(1, -1, 1, 1).clone()
        return sd

    # ---- running -------------------------------------------------------------------------------------------------------
    def _pack(self, device):
        if not isinstance(device, torch.device) or device.type != "cuda":
            raise RuntimeError("LPIPSAlex input must be a CUDA (HIP) tensor (no CPU fallback)")
        key = (device.type, device.index)
        if key not in self._packs:        # once per device: the weights are frozen
            dev = lambda ts: [t.to(device) for t in ts]
            with torch.cuda.device(device):
                self._packs[key] = ops.lpips_pack(dev(self.weights), dev(self.biases), dev(self.lins), self.shift.to(device), self.scale.to(device))
                torch.cuda.current_stream().synchronize()      # later calls may come from any stream
        return self._packs[key]

    def __call__(self, a, b):
        from . import autograd as A
        if not isinstance(a, torch.Tensor) or not isinstance(b, torch.Tensor):
            raise RuntimeError("LPIPSAlex input must be a CUDA (HIP) tensor (no CPU fallback)")
        return A.LpipsFn.apply(a, b, self._pack(a.device))

    def features(self, x):
        if not isinstance(x, torch.Tensor):
            raise RuntimeError("LPIPSAlex input must be a CUDA (HIP) tensor (no CPU fallback)")
        pack = self._pack(x.device)
        ws = ops.lpips_trunk(pack, x.detach())
        n, _, H, W = x.shape
        return [ops.lpips_feature(ws, n, H, W, l) for l in range(5)]
