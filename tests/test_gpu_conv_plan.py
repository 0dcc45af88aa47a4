"""GPU: the two ways a ConvPlan's packed weights come to be agree to the byte -- the ``pack_*`` methods (first use) and
ops.repack_plans / ops.run_repack (every train step after Adam).  Packs need no image: no conv launch runs here."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

# (kind, Cout, Cin) of the 3x3 FORWARD weight: a gradient kind's launch runs Cout -> Cin (dgrad_s2ds: -> 4 Cin stacked); the second
# dgrad has 128 output channels in its launch, which is what the Winograd pack needs
PLANS = (("conv", 64, 64), ("conv", 128, 64), ("conv", 256, 64), ("s2d", 128, 64), ("convT", 128, 64), ("convT", 256, 64),
         ("dgrad", 128, 64), ("dgrad", 64, 128), ("dgradT", 128, 64), ("dgrad_s2ds", 64, 32))


def _take_every_pack(ops, pl):
    """every pack key the plan's precision mode allows, through the methods the launches use"""
    for bn in sorted({64, pl.bn} | ({256} if pl.cout % 256 == 0 else set())):
        pl.pack_for(bn)
    if pl.steps_dual is not None:
        pl.pack_dual()
    if pl.precision in (1, 3):
        if pl.steps_k64 is not None:
            for bn in sorted({pl.bn} | ({256} if pl.cout % 256 == 0 else set())):
                pl.pack_k64(bn)
        if pl.steps_dual_k64 is not None:
            pl.pack_k64(256, dual=True)
    if pl.precision == 0:
        if pl.steps_up9 is not None:
            pl.pack_up9()
        if pl.kind in ("conv", "dgrad") and pl.k == 3 and pl.cout >= 128:
            pl.pack_wino()
    return pl


def _build(ops, weights, precision):
    return [_take_every_pack(ops, ops.ConvPlan(w, kind=kind, scale=1.0 / math.sqrt(cin * 9), precision=precision))
            for w, (kind, cout, cin) in zip(weights, PLANS)]


def _assert_same(plans, fresh, what):
    keys = set()
    for (kind, cout, cin), a, b in zip(PLANS, plans, fresh):
        assert list(a._packs) == list(b._packs)
        assert a.wsrc.shape == b.wsrc.shape and torch.equal(a.wsrc, b.wsrc), (what, kind, cout, cin, "wsrc")
        for key in a._packs:
            assert a._packs[key].dtype == torch.int16 and a._packs[key].shape == b._packs[key].shape
            assert torch.equal(a._packs[key], b._packs[key]), (what, kind, cout, cin, key)
            keys.add(str(key))
    return keys


@pytest.mark.parametrize("precision", (0, 1, 3))
def test_repack_equals_a_fresh_pack(precision):
    from ppst_amd import ops
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(precision)
    weights = [torch.randn(cout, cin, 3, 3, generator=g).to(dev) for _, cout, cin in PLANS]
    plans = _build(ops, weights, precision)
    assert all(pl.wparam.data_ptr() == w.data_ptr() for pl, w in zip(plans, weights))
    before = [{k: v.clone() for k, v in pl._packs.items()} for pl in plans]
    for w in weights:                                   # what the Adam kernel does: new values in the same storage
        w.mul_(0.75).add_(0.01 * torch.randn(w.shape, generator=g).to(dev))
    tables = ops.repack_plans(plans)
    keys = _assert_same(plans, _build(ops, weights, precision), "repack_plans")
    assert all(not torch.equal(pl._packs[k], b[k]) for pl, b in zip(plans, before) for k in b)       # (the packs did change)
    want = {"64", "128", "256", "dual"} | ({"up9", "wino"} if precision == 0 else {"k64_128", "k64_256", "k64_dual"})
    assert keys == want
    for w in weights:
        w.mul_(1.25).sub_(0.01)
    ops.run_repack(tables)
    _assert_same(plans, _build(ops, weights, precision), "run_repack")
    torch.cuda.synchronize()
