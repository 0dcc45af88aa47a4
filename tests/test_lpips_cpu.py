"""CPU: the LPIPS-AlexNet metric's loader, its place outside the model's checkpoint contract, and the argument checks of the
ppst_lpips_* entry points (include/ppst_hip.h) -- nothing here launches a kernel."""
import ctypes
import os

import pytest
import torch

from ppst_amd.lpips import CHANNELS, LPIPSAlex

SLICE = ((1, 0), (2, 3), (3, 6), (4, 8), (5, 10))


def _same(m1, m2):
    for t1, t2 in zip(m1.weights + m1.biases + m1.lins + [m1.shift, m1.scale], m2.weights + m2.biases + m2.lins + [m2.shift, m2.scale]):
        if t1.shape != t2.shape or not torch.equal(t1, t2):
            return False
    return True


def test_synthetic_state_dict_is_seeded_and_well_formed():
    a, b, c = LPIPSAlex.synthetic_state_dict(1), LPIPSAlex.synthetic_state_dict(1), LPIPSAlex.synthetic_state_dict(2)
    assert sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(a["net.slice1.0.weight"], c["net.slice1.0.weight"])
    assert a["net.slice1.0.weight"].shape == (64, 3, 11, 11) and a["net.slice2.3.weight"].shape == (192, 64, 5, 5)
    assert a["net.slice5.10.bias"].shape == (256,) and a["lin2.model.1.weight"].shape == (1, 384, 1, 1)
    assert all(a["lin%d.model.1.weight" % l].min() >= 0 for l in range(5)) and all(v.dtype == torch.float32 for v in a.values())
    assert a["scaling_layer.shift"].flatten().tolist() == pytest.approx([-.030, -.088, -.188])
    assert a["scaling_layer.scale"].flatten().tolist() == pytest.approx([.458, .448, .450])
    m = LPIPSAlex.from_state_dict(a)
    assert [w.shape[0] for w in m.weights] == list(CHANNELS) and [l.shape for l in m.lins] == [(c_,) for c_ in CHANNELS]


def test_key_spellings_and_prefix_give_the_same_module():
    sd = LPIPSAlex.synthetic_state_dict(3)
    ref = LPIPSAlex.from_state_dict(sd)
    # (1) `lins.<l>` instead of `lin<l>`  (2) torchvision's `features.<i>` for the trunk  (3) everything at once, equal values
    lins = {k.replace("lin", "lins.", 1) if k.startswith("lin") else k: v for k, v in sd.items()}
    assert "lins.0.model.1.weight" in lins and "lin0.model.1.weight" not in lins
    tv = {}
    for k, v in sd.items():
        for s, i in SLICE:
            k = k.replace("net.slice%d.%d." % (s, i), "features.%d." % i)
        tv[k] = v
    assert "features.10.bias" in tv and not any(k.startswith("net.") for k in tv)
    both = dict(sd)
    both.update({k: v.clone() for k, v in lins.items()})
    both.update({k: v.clone() for k, v in tv.items()})
    for other in (lins, tv, both):
        assert _same(ref, LPIPSAlex.from_state_dict(other))
    pre = {"loss_fn_alex." + k: v for k, v in sd.items()}
    pre["G.something"] = torch.zeros(3)
    assert _same(ref, LPIPSAlex.from_state_dict(pre, prefix="loss_fn_alex."))
    with pytest.raises(KeyError, match="scaling_layer.shift"):
        LPIPSAlex.from_state_dict(pre)                    # without the prefix nothing is found
    # and what the module hands back loads again
    assert _same(ref, LPIPSAlex.from_state_dict(ref.state_dict("x."), prefix="x."))


def test_loader_errors_name_the_key():
    sd = LPIPSAlex.synthetic_state_dict(4)
    for key in ("scaling_layer.scale", "net.slice3.6.weight", "net.slice4.8.bias", "lin4.model.1.weight"):
        bad = {k: v for k, v in sd.items() if k != key}
        with pytest.raises(KeyError, match=key.replace(".", r"\.")):
            LPIPSAlex.from_state_dict(bad)
        with pytest.raises(KeyError, match=r"p\." + key.replace(".", r"\.")):
            LPIPSAlex.from_state_dict({"p." + k: v for k, v in bad.items()}, prefix="p.")
    bad = dict(sd)
    bad["net.slice2.3.weight"] = torch.zeros(192, 64, 3, 3)
    with pytest.raises(ValueError, match=r"net\.slice2\.3\.weight.*\(192, 64, 5, 5\)"):
        LPIPSAlex.from_state_dict(bad)
    bad = dict(sd)
    bad["lin1.model.1.weight"] = torch.zeros(192)
    with pytest.raises(ValueError, match=r"lin1\.model\.1\.weight"):
        LPIPSAlex.from_state_dict(bad)
    bad = dict(sd)
    bad["lin3.model.1.weight"] = sd["lin3.model.1.weight"].clone()
    bad["lin3.model.1.weight"][0, 7, 0, 0] = -1e-3
    with pytest.raises(ValueError, match=r"lin3\.model\.1\.weight.*negative"):
        LPIPSAlex.from_state_dict(bad)
    # two spellings that disagree
    bad = dict(sd)
    bad["lins.2.model.1.weight"] = sd["lin2.model.1.weight"] * 2
    with pytest.raises(ValueError, match=r"lin2\.model\.1\.weight.*lins\.2\.model\.1\.weight.*differ"):
        LPIPSAlex.from_state_dict(bad)
    bad = dict(sd)
    bad["features.0.bias"] = sd["net.slice1.0.bias"] + 1
    with pytest.raises(ValueError, match=r"features\.0\.bias.*differ"):
        LPIPSAlex.from_state_dict(bad)


def test_flat_checkpoint_round_trip(tmp_path):
    """A file of the reference's layout: the metric's tensors under ``loss_fn_alex.`` beside the model's keys."""
    from ppst_amd import weights as W
    lp = LPIPSAlex.synthetic_state_dict(5)
    sd = W.make_state_dict(3, with_D=False, with_nce=False)
    n_model = len(sd)
    sd.update({"loss_fn_alex." + k: v for k, v in lp.items()})
    sd.update({"loss_fn_alex.lins.%d.model.1.weight" % l: lp["lin%d.model.1.weight" % l].clone() for l in range(5)})   # as the package stores them
    path = str(tmp_path / "latest_checkpoint.pth")
    torch.save(sd, path)
    assert _same(LPIPSAlex.from_checkpoint(path), LPIPSAlex.from_state_dict(lp))
    with pytest.raises(KeyError, match="scaling_layer"):
        LPIPSAlex.from_checkpoint(path, prefix="")
    assert len(sd) == n_model + len(lp) + 5


def test_metric_stays_out_of_the_checkpoint_contract(tmp_path):
    from ppst_amd import weights as W
    from ppst_amd.ppst_model import Options, PPSTModel
    m = PPSTModel(Options(checkpoints_dir=str(tmp_path), name="run"), with_D=False)
    m.load_weights(W.make_state_dict(3, with_D=False, with_nce=False))
    before = list(m.state_dict())
    lp = {"loss_fn_alex." + k: v for k, v in LPIPSAlex.synthetic_state_dict(6).items()}
    assert m.perceptual_metric is None
    with pytest.raises(ValueError, match="state_dict"):
        m.set_perceptual_metric("lpips")
    with pytest.raises(ValueError, match="unknown"):
        m.set_perceptual_metric("vgg", state_dict=lp)
    assert m.set_perceptual_metric("lpips", state_dict=lp, prefix="loss_fn_alex.") is m
    assert isinstance(m.perceptual_metric, LPIPSAlex)
    assert list(m.state_dict()) == before and "perceptual_metric" not in dict(m.named_modules())
    path = m.save(1000)
    saved = torch.load(path, map_location="cpu", weights_only=True)
    assert list(saved) == before and not any(k.startswith("loss_fn_alex.") for k in saved)
    # load(..., perceptual=True) picks the metric out of the file it reads anyway; a file without one is an error, not a silent skip
    full = dict(saved)
    full.update(lp)
    torch.save(full, str(tmp_path / "with_lpips.pth"))
    m2 = PPSTModel(Options(checkpoints_dir=str(tmp_path), name="run"), with_D=False)
    assert m2.load(str(tmp_path / "with_lpips.pth"), verbose=False) and m2.perceptual_metric is None       # opt-in only
    assert m2.load(str(tmp_path / "with_lpips.pth"), verbose=False, perceptual=True)
    assert _same(m2.perceptual_metric, m.perceptual_metric) and list(m2.state_dict()) == before
    with pytest.raises(KeyError, match=r"loss_fn_alex\.scaling_layer"):
        m2.load(path, verbose=False, perceptual=True)
    # any callable is still accepted
    f = lambda a, b: (a - b).abs().mean()
    assert m.set_perceptual_metric(f).perceptual_metric is f


def test_library_exports_the_lpips_entry_points():
    from ppst_amd import _lib
    names = ["ppst_lpips_pack_floats", "ppst_lpips_pack", "ppst_lpips_dims", "ppst_lpips_ws", "ppst_lpips_trunk", "ppst_lpips_feature",
             "ppst_lpips_tail", "ppst_lpips_bwd_ws", "ppst_lpips_backward"]
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(raw, n) and n in _lib.exported_symbols(), n
    assert _lib.lib.ppst_version() == 3
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ppst_hip.h")).read()
    assert all(n + "(" in header for n in names) and "#define PPST_ABI_VERSION 3" in header


def test_sizes_and_argument_errors_need_no_gpu():
    from ppst_amd import ops
    from ppst_amd._lib import lib
    # the feature-map sizes of the definition: floor((n + 2p - k) / s) + 1
    assert ops.lpips_dims(512, 512) == [(127, 127), (63, 63), (31, 31), (31, 31), (31, 31)]
    assert ops.lpips_dims(256, 256) == [(63, 63), (31, 31), (15, 15), (15, 15), (15, 15)]
    assert ops.lpips_dims(272, 208) == [(67, 51), (33, 25), (16, 12), (16, 12), (16, 12)]
    assert ops.lpips_dims(31, 31) == [(7, 7), (3, 3), (1, 1), (1, 1), (1, 1)]
    for H, W in ((224, 224), (31, 500), (333, 47)):
        x = torch.zeros(1, 3, H, W)
        f = torch.nn.functional
        h1 = f.conv2d(x, torch.zeros(1, 3, 11, 11), stride=4, padding=2)
        h2 = f.max_pool2d(h1, 3, 2)
        h3 = f.max_pool2d(h2, 3, 2)
        assert ops.lpips_dims(H, W) == [tuple(h1.shape[2:]), tuple(h2.shape[2:])] + [tuple(h3.shape[2:])] * 3
    with pytest.raises(RuntimeError):
        ops.lpips_dims(30, 64)
    hw = (ctypes.c_int * 10)()
    assert lib.ppst_lpips_dims(64, 30, hw) == -1 and lib.ppst_lpips_dims(64, 64, None) == -3
    # workspace sizes: positive, growing with the batch, EINVAL below 31 pixels a side
    assert lib.ppst_lpips_ws(4, 30, 512) == -1 and lib.ppst_lpips_ws(4, 512, 30) == -1 and lib.ppst_lpips_ws(-1, 64, 64) == -1
    assert 0 < lib.ppst_lpips_ws(2, 31, 31) < lib.ppst_lpips_ws(4, 31, 31) < lib.ppst_lpips_ws(4, 512, 512)
    floats = 4 * (127 * 127 * 64 + 63 * 63 * 192 + 31 * 31 * (384 + 256 + 256))      # the five maps alone
    assert 4 * floats < lib.ppst_lpips_ws(4, 512, 512) < 3 * 4 * floats
    assert lib.ppst_lpips_bwd_ws(2, 512, 512, 0) == -1 and lib.ppst_lpips_bwd_ws(2, 512, 512, 4) == -1 and lib.ppst_lpips_bwd_ws(2, 20, 512, 1) == -1
    assert 0 < lib.ppst_lpips_bwd_ws(2, 512, 512, 1) < lib.ppst_lpips_bwd_ws(2, 512, 512, 3)
    assert lib.ppst_lpips_bwd_ws(2, 512, 512, 1) == lib.ppst_lpips_bwd_ws(2, 512, 512, 2)
    n_pack = lib.ppst_lpips_pack_floats()
    fwd = 9 * 48 * 64 + 25 * 64 * 192 + 9 * (192 * 384 + 384 * 256 + 256 * 256)
    assert 2 * fwd <= n_pack <= 2 * fwd + 9 * 16 * 64 + 4096
    # null pointers and bad sizes are rejected before any launch; empty batches are no-ops
    d = ctypes.c_void_p(16)
    st = (ctypes.c_int64 * 4)(3 * 64 * 64, 64 * 64, 64, 1)
    assert lib.ppst_lpips_pack(None, None, None, None, None, None, None) == -3
    assert lib.ppst_lpips_trunk(d, d, st, 1, d, st, 1, 30, 64, d, None) == -1
    assert lib.ppst_lpips_trunk(d, d, st, -1, d, st, 1, 64, 64, d, None) == -1
    assert lib.ppst_lpips_trunk(d, None, st, 1, d, st, 1, 64, 64, d, None) == -3
    assert lib.ppst_lpips_trunk(d, d, st, 1, d, st, 1, 64, 64, None, None) == -3
    assert lib.ppst_lpips_trunk(None, d, st, 1, d, st, 1, 64, 64, d, None) == -3
    assert lib.ppst_lpips_trunk(None, None, None, 0, None, None, 0, 64, 64, None, None) == 0
    assert lib.ppst_lpips_feature(d, 1, 64, 64, 5, d, None) == -1 and lib.ppst_lpips_feature(None, 1, 64, 64, 0, d, None) == -3
    assert lib.ppst_lpips_tail(d, d, 1, 64, 20, d, None) == -1 and lib.ppst_lpips_tail(d, d, 1, 64, 64, None, None) == -3
    assert lib.ppst_lpips_tail(None, None, 0, 64, 64, None, None) == 0
    assert lib.ppst_lpips_backward(d, d, d, 1, 64, 64, 0, d, d, d, None) == -1
    assert lib.ppst_lpips_backward(d, d, d, 1, 64, 64, 1, None, d, d, None) == -3       # ga asked for, not given
    assert lib.ppst_lpips_backward(d, d, d, 1, 64, 64, 2, None, None, d, None) == -3
    assert lib.ppst_lpips_backward(d, d, d, 1, 64, 64, 3, d, d, None, None) == -3
    assert lib.ppst_lpips_backward(None, None, None, 0, 64, 64, 3, None, None, None, None) == 0


def test_module_refuses_cpu_tensors():
    m = LPIPSAlex.from_state_dict(LPIPSAlex.synthetic_state_dict(1))
    x = torch.zeros(1, 3, 64, 64)
    with pytest.raises(RuntimeError, match="CUDA"):
        m(x, x)
    with pytest.raises(RuntimeError, match="CUDA"):
        m.features(x)
