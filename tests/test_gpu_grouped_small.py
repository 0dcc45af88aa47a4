"""GPU: the grouped launches of the style path (ppst_linear_grouped, ppst_l2norm_rows_grouped, ppst_lerp_grouped,
ppst_gap_gmp_multi_level) -- pytest -m gpu.

Two kinds of criteria:
  * INVARIANT: every problem of a group runs the code of its single call, so its output equals ``ops.linear`` / ``l2norm_rows``
    / ``lerp`` / ``gap_gmp`` on the same problem bit for bit (torch.equal, no tolerance);
  * against a float64 torch evaluation, at the bars of the single ops' checks in tests/gpu_diag.py (max |difference| over
    max |reference|): linear 3e-6 (t_layout_misc), l2norm 1e-6 (t_layout_misc), GAP/GMP 2e-6 (t_elementwise).  lerp's check
    there is exact equality with the fp32 formula a * (1 - r) + b * r; it is kept as that, and against float64 the bar is the
    format's: (1 - r), the two products and the sum round once each, so |y - ref| <= 3.5 * 2^-24 * (|a| (1 - r) + |b| r)
    element by element (three roundings to first order, with or without a fused multiply-add, and room for the second order).
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

LINEAR_BAR, L2NORM_BAR, GAP_BAR = 3e-6, 1e-6, 2e-6
LRELU = 1      # ops.ACT_LRELU


def _rel(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    assert a.shape == ref.shape
    return (a - ref).abs().max().item() / (ref.abs().max().item() + 1e-30)


def _dev():
    return torch.device("cuda", 0)


# ---------------------------------------------------------------------------------------------------------------- linear ----
def _linear_ref64(x, w, b, wscale, bscale, relu_in, act):
    x, w = x.double().cpu(), w.double().cpu()
    if relu_in:
        x = F.relu(x)
    y = F.linear(x, w * float(np.float32(wscale)), None if b is None else b.double().cpu() * float(np.float32(bscale)))
    if act == LRELU:
        y = F.leaky_relu(y, 0.2) * (2.0 ** 0.5)
    return y


def _linear_problem(gen, B, K, N, relu_in=False, act=0, bias=True, wscale=0.1, bscale=0.5):
    x = torch.randn(B, K, generator=gen).to(_dev())
    w = torch.randn(N, K, generator=gen).to(_dev())
    b = torch.randn(N, generator=gen).to(_dev()) if bias else None
    return (x, w, b, wscale, bscale, relu_in, act)


def _check_linear_group(problems):
    from ppst_amd import ops
    ys = ops.linear_grouped(problems)
    assert len(ys) == len(problems)
    for i, (pr, y) in enumerate(zip(problems, ys)):
        x, w, b, wscale, bscale, relu_in, act = pr
        single = ops.linear(x, w, b, wscale, bscale, relu_in, act)
        r = _rel(y, _linear_ref64(*pr))
        print("linear_grouped problem %d B%d K%d N%d relu%d act%d bias%d: rel %.3e (bar %.0e), bit-equal %s"
              % (i, x.shape[0], x.shape[1], w.shape[0], relu_in, act, b is not None, r, LINEAR_BAR, torch.equal(y, single)))
        assert torch.equal(y, single), "problem %d differs from ops.linear" % i
        assert r <= LINEAR_BAR, (i, r)


def test_grouped_linear_problem_mix():
    """Four problems across every dispatch edge of linear.hip: K below / at / above the K-split threshold (1024), K % 4 != 0 (the
    scalar loop), N not a multiple of the 4 rows of a block and N = 1, B = 1 (<1>), 8 (<8>), 9 (<16>) and 24 (16 + 8: two pieces
    inside the group), relu_in on and off, one leaky-ReLU, one problem without bias."""
    gen = torch.Generator().manual_seed(11)
    _check_linear_group([
        _linear_problem(gen, 1, 1024, 7, relu_in=False, act=0),                 # K-split form, N % 4 != 0, <1>
        _linear_problem(gen, 8, 1020, 1, relu_in=True, act=LRELU),              # row form just below the threshold, N = 1, <8>
        _linear_problem(gen, 9, 2048, 130, relu_in=True, act=0, bias=False),    # K-split, <16>, no bias
        _linear_problem(gen, 24, 70, 13, relu_in=False, act=0),                 # scalar loop (K % 4 = 2), <16> + <8> pieces
    ])
    # the same edges the other way round: 24 rows through the K-split form, one row through the row form
    _check_linear_group([
        _linear_problem(gen, 24, 1024, 9, relu_in=True, act=LRELU),
        _linear_problem(gen, 1, 64, 6, relu_in=False, act=0, bias=False),
    ])


def test_grouped_linear_group_sizes():
    """A group of one, and a group at the maximum (32 problems; with 24-row problems among them the 16-row pieces exceed the 32 one
    launch holds and the rest goes out in a second launch)."""
    from ppst_amd._lib import GROUP_MAX
    gen = torch.Generator().manual_seed(12)
    _check_linear_group([_linear_problem(gen, 3, 96, 10, relu_in=True)])
    shapes = [(1, 32, 5), (8, 1024, 3), (9, 40, 4), (24, 36, 2)]
    _check_linear_group([_linear_problem(gen, *shapes[i % 4], relu_in=bool(i & 1), act=(LRELU if i % 3 == 0 else 0), bias=(i % 5 != 0))
                         for i in range(GROUP_MAX)])


# ---------------------------------------------------------------------------------------------------------------- l2norm ----
@pytest.mark.parametrize("mode,eps", [(0, 1e-8), (1, 1e-12)])
def test_grouped_l2norm(mode, eps):
    """K = 512 and 2048, B = 1 and 24, a zero row in one problem (the eps path: rsqrt(0 + eps) in mode 0, the clamp in mode 1)."""
    from ppst_amd import ops
    gen = torch.Generator().manual_seed(13 + mode)
    xs = [torch.randn(B, K, generator=gen) for B, K in ((1, 512), (24, 2048), (24, 512), (1, 2048))]
    xs[1][5] = 0.0
    xs = [x.to(_dev()) for x in xs]
    ys = ops.l2norm_rows_grouped(xs, eps, mode)
    for i, (x, y) in enumerate(zip(xs, ys)):
        xd = x.double().cpu()
        e = float(np.float32(eps))
        s = (xd * xd).sum(1, keepdim=True)
        ref = xd * torch.rsqrt(s + e) if mode == 0 else xd / torch.clamp(s.sqrt(), min=e)
        r = _rel(y, ref)
        single = ops.l2norm_rows(x, eps, mode)
        print("l2norm_rows_grouped mode %d problem %d %s: rel %.3e (bar %.0e), bit-equal %s" % (mode, i, tuple(x.shape), r, L2NORM_BAR, torch.equal(y, single)))
        assert torch.equal(y, single)
        assert r <= L2NORM_BAR, (i, r)
    assert torch.equal(ys[1][5], torch.zeros_like(ys[1][5]))


# ------------------------------------------------------------------------------------------------------------------ lerp ----
def test_grouped_lerp():
    """Four problems, one of a length that is no multiple of 4 (nor of the block), one longer than a block's 256 elements."""
    from ppst_amd import ops
    gen = torch.Generator().manual_seed(15)
    r = 0.3
    pairs = [(torch.randn(*s, generator=gen), torch.randn(*s, generator=gen)) for s in ((8, 2048), (1, 2048), (3, 331), (1, 1))]
    dev = [(a.to(_dev()), b.to(_dev())) for a, b in pairs]
    ys = ops.lerp_grouped(dev, r)
    r32 = float(np.float32(r))
    for i, ((a, b), (ad, bd), y) in enumerate(zip(pairs, dev, ys)):
        assert torch.equal(y, ops.lerp(ad, bd, r)), i
        assert torch.equal(y.cpu(), a * (1 - r) + b * r), i                       # gpu_diag's check of ops.lerp: exact
        ref = a.double() * (1.0 - r32) + b.double() * r32
        bound = 3.5 * 2.0 ** -24 * (a.double().abs() * (1.0 - r32) + b.double().abs() * r32)
        worst = ((y.cpu().double() - ref).abs() / (bound + 1e-300)).max().item()
        print("lerp_grouped problem %d %s: worst |err| / bound = %.3f" % (i, tuple(a.shape), worst))
        assert worst <= 1.0, (i, worst)


# --------------------------------------------------------------------------------------------------------------- GAP/GMP ----
LEVELS = ((16, 32), (8, 64), (4, 256), (2, 256))      # (H = W, C): 16^2 .. 2^2 (fewer pixels than a block's pixel rows)


@pytest.fixture(scope="module")
def gap_inputs():
    gen = torch.Generator().manual_seed(17)
    xs = [torch.randn(3, s, s, c, generator=gen) for s, c in LEVELS]
    ms = [(torch.rand(3, s, s, generator=gen) > 0.4).float() for s, _ in LEVELS]
    return xs, ms


@pytest.mark.parametrize("masked", [False, True])
def test_multi_level_gap_gmp(gap_inputs, masked):
    from ppst_amd import ops
    xs, ms = gap_inputs
    xd = [x.to(_dev()) for x in xs]
    md = [m.to(_dev()) for m in ms] if masked else [None] * len(xs)
    outs = ops.gap_gmp_levels(xd, md)
    one = ops.gap_gmp_levels([x[1:2].contiguous() for x in xd], [None if m is None else m[1:2].contiguous() for m in md])
    for i, (x, o) in enumerate(zip(xs, outs)):
        C = x.shape[3]
        single = ops.gap_gmp(xd[i], md[i])
        assert torch.equal(o, single), "level %d differs from ops.gap_gmp" % i
        assert torch.equal(o[1:2], one[i]), "level %d: image 1 alone differs from image 1 inside B = 3" % i
        x64 = x.double() * (ms[i].double()[..., None] if masked else 1.0)
        ref = torch.cat([x64.mean((1, 2)), x64.amax((1, 2))], 1)
        r = _rel(o, ref)
        print("gap_gmp_levels level %d %s masked=%s: rel %.3e (bar %.0e)" % (i, tuple(x.shape), masked, r, GAP_BAR))
        assert o.shape == (3, 2 * C) and r <= GAP_BAR, (i, r)


# ------------------------------------------------------------------------------------------------------- argument checks ----
def test_grouped_argument_checks():
    """Zero problems: PPST_OK and no launch (a null table is accepted: nothing is read); more than the maximum: PPST_EINVAL; a null
    pointer in ANY problem: PPST_ENULL, found before anything is launched."""
    from ppst_amd import _lib
    lib, tok = _lib.lib, 256                                     # a non-null, aligned token: validation dereferences nothing
    n_max = _lib.GROUP_MAX
    for fn in (lib.ppst_linear_grouped, lib.ppst_l2norm_rows_grouped, lib.ppst_lerp_grouped):
        assert fn(None, 0, None) == 0
        assert fn(ctypes.c_void_p(tok), n_max + 1, None) == -1
        assert fn(None, 1, None) == -3
    assert lib.ppst_gap_gmp_multi_level(None, 0, 3, None, 0, None) == 0
    assert lib.ppst_gap_gmp_multi_level(ctypes.c_void_p(tok), n_max + 1, 3, ctypes.c_void_p(tok), 0, None) == -1
    assert lib.ppst_gap_gmp_multi_level(None, 1, 3, ctypes.c_void_p(tok), 0, None) == -3

    lin = (_lib.LinearProblem * 3)()
    for q in lin:
        q.x = q.w = q.bias = q.y = tok
        q.B, q.K, q.N, q.wscale, q.bscale = 2, 8, 4, 1.0, 1.0
    for field in ("x", "w", "y"):
        setattr(lin[2], field, None)
        assert lib.ppst_linear_grouped(lin, 3, None) == -3, field
        setattr(lin[2], field, tok)
    lin[1].K = 0
    assert lib.ppst_linear_grouped(lin, 3, None) == -1

    l2 = (_lib.L2normProblem * 2)()
    for q in l2:
        q.x = q.y = tok
        q.B, q.K, q.eps, q.mode = 2, 8, 1e-8, 0
    l2[1].y = None
    assert lib.ppst_l2norm_rows_grouped(l2, 2, None) == -3
    l2[1].y, l2[0].mode = tok, 2
    assert lib.ppst_l2norm_rows_grouped(l2, 2, None) == -1

    le = (_lib.LerpProblem * 2)()
    for q in le:
        q.a = q.b = q.y = tok
        q.n, q.r = 16, 0.5
    le[1].b = None
    assert lib.ppst_lerp_grouped(le, 2, None) == -3
    le[1].b, le[0].n = tok, -1
    assert lib.ppst_lerp_grouped(le, 2, None) == -1

    lv = (_lib.GapGmpLevel * 2)()
    for q in lv:
        q.x = q.out = tok
        q.H, q.W, q.C, q.ld = 4, 4, 8, 8
    ws = ctypes.c_void_p(tok)
    assert lib.ppst_gap_gmp_multi_level_ws(lv, 2, 3) == 2 * lib.ppst_gap_gmp_ws(3, 16, 8)
    lv[1].out = None
    assert lib.ppst_gap_gmp_multi_level(lv, 2, 3, ws, 0, None) == -3
    lv[1].out = tok
    assert lib.ppst_gap_gmp_multi_level(lv, 2, 3, None, 0, None) == -3
    lv[0].C = 6
    assert lib.ppst_gap_gmp_multi_level(lv, 2, 3, ws, 0, None) == -1
