"""No GPU: the references, the inputs and the bars of tests/test_gpu_corr.py are proven here before the device is trusted by them
(tests/corr_cases.py).
  * every reference agrees with an independent float64 formulation (torch.einsum, F.softmax, the oracle's corrm / rselfcorr
    formulas, an explicit gather for the unfolds);
  * the plane constructions of the GEMM term cases decompose exactly, and the figures the bars were taken from hold: the
    six-term (three-term) model sits within 0.5 (0.2) units of float64, every dropped term moves every element by >= 48 (100: 103 .. 106 at K = 32 on these draws);
  * every seeded defect of every case is rejected by the comparison the GPU test uses, at the GPU test's bar, on the case's own
    inputs -- and the float64 reference itself, rounded to float32, passes it;
  * the facets of the cases are exactly corr_cases.FACETS: a removed case fails here;
  * corr_cases.gemm_passes agrees with ops._gemm_passes / ops.gemm_nn for every GEMM case.
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import corr_cases as C  # noqa: E402

IDS = [c.id for c in C.CASES]


def _of(op, **kw):
    return [c for c in C.CASES if c.op == op and all(c.p.get(k) == v for k, v in kw.items())]


def _close(a, b, tol=1e-12):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    s = max(np.abs(b).max(), 1e-300)
    assert np.abs(a - b).max() <= tol * s, np.abs(a - b).max() / s


# ------------------------------------------------------------------------------------------------------ reference checks
@pytest.mark.parametrize("c", [c for c in _of("gemm") if c.p["b"] <= 2], ids=lambda c: c.id)
def test_gemm_reference_is_einsum(c):
    inp, p = C.inputs(c.id), c.p
    A, Bm = inp["A"].double(), inp["B"].double()
    want = torch.einsum("bmk,bnk->bmn", A, Bm) if p["form"] == "NT" else torch.einsum("bmk,bkn->bmn", A, Bm[..., :p["N"]])
    _close(C.reference(c.id)["C"], (p.get("alpha", 1.0) * want).numpy())
    assert not torch.equal(inp["B"][0], inp["B"][1]), "the batch elements share their data"


@pytest.mark.parametrize("c", _of("corr_prep"), ids=lambda c: c.id)
def test_corr_prep_reference_is_the_oracles_formula(c):
    import ppst_oracle as O
    assert C.EPS == O.EPS64
    f = C.inputs(c.id)["x"].double().permute(0, 2, 1)                   # (B, C, P), as corrm holds it
    nc = c.p["ncenter"]
    h1 = f[:, :nc] - f[:, :nc].mean(dim=1, keepdim=True) if nc else f[:, :0]
    f = torch.cat((h1, f[:, nc:]), dim=1)
    want = (f / (torch.norm(f, 2, 1, keepdim=True) + O.EPS64)).permute(0, 2, 1)
    _close(C.reference(c.id)["y"], want.numpy())
    if c.p.get("zero_row"):
        assert not C.reference(c.id)["y"][0, 2].any()
    if nc and not c.p.get("big_mean"):                                   # F.normalize-style: unit rows
        _close(np.linalg.norm(C.reference(c.id)["y"], axis=-1)[C.inputs(c.id)["x"].abs().sum(-1).numpy() > 0], 1.0)


@pytest.mark.parametrize("c", _of("softmax_rows_"), ids=lambda c: c.id)
def test_softmax_reference_is_F_softmax_and_the_rows_are_what_they_claim(c):
    x, p = C.inputs(c.id)["x"], c.p
    ref = C.reference(c.id)["p"]
    _close(ref, F.softmax(x.double() / float(np.float32(p["div"])), -1).numpy())
    _close(ref.sum(-1), 1.0)
    if p["rows"] == 5:
        tie, equal, dom = (ref[C._SM_KINDS.index(k)] for k in ("tie", "equal", "dominant"))
        v = (x[2] / np.float32(p["div"]))
        assert (v == v.max()).sum() == 2 and (x[2] == x[2].max()).sum() == 2, "no exact two-way tie"
        assert (tie == tie.max()).sum() == 2
        assert np.all(equal == 1.0 / p["cols"])
        assert dom.max() == 1.0 and (dom > 1e-20).sum() == 1


@pytest.mark.parametrize("c", _of("rselfcorr"), ids=lambda c: c.id)
def test_rselfcorr_reference_is_the_oracle(c):
    import ppst_oracle as O
    fea = C.inputs(c.id)["fea"].double()
    _close(C.reference(c.id)["out"], O.rselfcorr(fea.permute(0, 3, 1, 2)).permute(0, 2, 3, 1).numpy())
    if c.p.get("const_patch"):
        assert not C.reference(c.id)["out"][0, 0, 0].any()


def _gather(x, k):
    """F.unfold(x, k, padding = k // 2) of an NHWC map, one element at a time"""
    B, H, W, Cn = x.shape
    out = np.zeros((B, H * W, Cn * k * k))
    r = k // 2
    for y in range(H):
        for xx in range(W):
            for ky in range(k):
                for kx in range(k):
                    iy, ix = y + ky - r, xx + kx - r
                    if 0 <= iy < H and 0 <= ix < W:
                        out[:, y * W + xx, ky * k + kx::k * k] = x[:, iy, ix, :]
    return out


@pytest.mark.parametrize("c", _of("unfold_rows"), ids=lambda c: c.id)
def test_unfold_rows_reference_is_the_gather(c):
    _close(C.reference(c.id)["rows"], _gather(C.inputs(c.id)["x"].double().numpy(), c.p["k"]), 0)


@pytest.mark.parametrize("c", [c for c in _of("patches") if c.p["H"] <= 64], ids=lambda c: c.id)
def test_patches_reference_is_the_index_map_and_fold_inverts_unfold(c):
    p, inp, r = c.p, C.inputs(c.id), C.reference(c.id)
    s, gx = p["s"], p["W"] // p["s"]
    x = inp["x"].double().numpy()
    for (b, pt, col) in [(0, 0, 0), (1, gx + 1, p["C"] * s * s - 1), (1, r["unfold"].shape[1] - 1, s * s // 2)]:
        ch, k = divmod(col, s * s)
        assert r["unfold"][b, pt, col] == x[b, ch, (pt // gx) * s + k // s, (pt % gx) * s + k % s]
    back = F.fold(torch.from_numpy(r["unfold"]).permute(0, 2, 1), (p["H"], p["W"]), s, stride=s)
    assert torch.equal(back, inp["x"].double())


# --------------------------------------------------------------------------------------------------- plane constructions
@pytest.mark.parametrize("c", [c for c in _of("gemm", kind="term") if c.p["b"] <= 2 and c.p["mode"] != "f32"], ids=lambda c: c.id)
def test_planes_decompose_exactly_and_a_dropped_term_moves_every_element(c):
    inp, p = C.inputs(c.id), c.p
    n, unit = p["planes"], C.unit(c)
    Bo32 = C._opB(c, inp, torch.float32).contiguous()
    pa, ra = C.split_planes(inp["A"], n)
    pb, rb = C.split_planes(Bo32, n)
    assert not ra.any() and not rb.any(), "the planes do not add up to the operand"
    assert all((q > 0).all() for q in pa + pb), "a plane has a non-positive element"
    assert all(torch.equal(q, q.bfloat16().float()) for q in pa + pb)
    ref, S = C.reference(c.id)["C"], C.gemm_scale(c)
    kept = [(0, 0), (0, 1), (1, 0)] + ([(1, 1), (0, 2), (2, 0)] if n == 3 else [])
    model = sum(torch.matmul(pa[i].double(), pb[j].double()) for i, j in kept).numpy()
    full = np.abs(model - ref) / S / unit
    assert full.max() <= (0.5 if n == 3 else 0.2), full.max()
    moved = min(float((torch.matmul(pa[i].double(), pb[j].double()).numpy() / S / unit).min()) for i, j in kept[1:])
    print("%-44s model %.3f units, smallest dropped term %.1f units, bar %.0f" % (c.id, full.max(), moved, C.bar(c, "C") / unit))
    assert moved >= (48 if n == 3 else 100), moved
    assert C.bar(c, "C") / unit <= moved / 4


# ----------------------------------------------------------------------------------------------------------- sensitivity
@pytest.mark.parametrize("cid", IDS)
def test_bar_passes_the_reference_and_rejects_every_seeded_defect(cid):
    c = C.by_id(cid)
    ref = C.reference(cid)
    for k, v in ref.items():
        bad, _ = C.judge(c, k, v.astype(np.float32))
        assert not bad, "%s: the float32 rounding of the reference misses its own bar: %s" % (k, bad)
    muts = C.mutations(c)
    assert muts, "a case carries at least one seeded defect"
    for name, out in muts:
        assert set(out) <= set(ref)
        seen = [k for k, v in out.items() if C.judge(c, k, v.astype(np.float32))[0]]
        assert seen, "the inputs of %s cannot show the defect '%s' at the bar" % (cid, name)


def test_every_op_has_two_kinds_of_defect_and_the_listed_kinds_occur():
    kinds = {}
    for c in C.CASES:
        if c.op == "gemm" and c.p["b"] > 2:             # (the names depend on p alone; the big products are left to the test above)
            continue
        kinds.setdefault(c.op, set()).update(n for n, _ in C.mutations(c))
    for op, k in kinds.items():
        assert len(k) >= 2, (op, k)
    every = set().union(*kinds.values())
    for want in ("product term m.m left out", "product term h.l left out", "product term l.h left out", "last K tile left out",
                 "ragged tail row zero", "ragged tail columns zero", "batch element 1 computed from element 0's B", "alpha ignored",
                 "B read with ldb = N", "ncenter rounded down to a multiple of 64", "the mean taken over C", "rows >= 8192 untouched",
                 "the last rows % 4 rows untouched", "the last cols % 1024 columns left out of the sum",
                 "the max taken over the first wave only", "div applied after the exp", "patches >= 8192 untouched",
                 "x and y patch index swapped", "elements >= 4096 * 256 untouched"):
        assert want in every, want


def test_odd_tile_cases_carry_the_dropped_last_tile():
    for c in _of("gemm"):
        if "tiles-odd" in " ".join(C.facets(c)) and c.p.get("kind") != "term":
            ps, BM, BN, BK = C.gemm_geometry(c.p)
            assert c.p["K"] > BK and (c.p["K"] // BK) % 2


def test_the_big_mean_bar_comes_from_the_float32_reference():
    for c in _of("corr_prep", big_mean=True):
        b = C.bar(c, "y")
        print("%-40s bar %.2e (float32 reference error %.2e)" % (c.id, b, C.err32(c.id)["y"]))
        assert C.BAR_EW <= b < 1e-4


# -------------------------------------------------------------------------------------------------------------- coverage
def test_facets_are_exactly_the_expected_set():
    reached = {}
    for c in C.CASES:
        for f in C.facets(c):
            reached.setdefault(f, []).append(c.id)
    missing = [f for f in C.FACETS if f not in reached]
    assert not missing, missing
    assert set(reached) <= set(C.FACETS), sorted(set(reached) - set(C.FACETS))
    assert len(set(C.FACETS)) == len(C.FACETS)
    # x3-big runs BK = 16 at K % 32 == 0: its tile count is even in every case, by construction of the dispatch
    for c in _of("gemm"):
        if C.branch(c).endswith("x3:big"):
            assert (c.p["K"] // 16) % 2 == 0
    # x6-big and both small kernels meet an odd tile count > 1
    odd = {C.branch(c) for c in _of("gemm") if any(f.endswith("tiles-odd") for f in C.facets(c))}
    assert odd >= {"split:%s:%s" % (f, k) for f in ("NT", "NN") for k in ("x6:small", "x6:big", "x3:small:BK32")}, odd


def test_the_minimum_table_of_the_issue_is_present():
    g = _of("gemm")
    shapes = {(c.p["form"], C.branch(c), c.p["b"], c.p["M"], c.p["N"]) for c in g}
    for f in ("NT", "NN"):
        for ps in ("x6", "x3"):
            big = "split:%s:%s:big" % (f, ps)
            assert {(f, big, 56, 300, 260), (f, big, 56, 512, 512), (f, big, 224, 129, 132)} <= shapes
        assert any(c.p["M"] == 1 and c.p["form"] == f and C.gemm_geometry(c.p)[0] for c in g)
        f32 = [c for c in g if c.p["form"] == f and c.p["mode"] == "f32" and c.p.get("kind") != "term" and "ldb" not in c.p]
        assert {c.p["N"] for c in f32} == set(C._F32_N[f])
        assert {c.p["M"] for c in f32} == {1, 130} and {c.p["K"] for c in f32} == {16, 48}
    assert all(c.p["alpha"] != 1 for c in g if c.p["form"] == "NT" and c.p["mode"] == "f32" and c.p.get("kind") != "term")
    assert {(c.p["K"], C.gemm_geometry(c.p)[3]) for c in g if C.gemm_geometry(c.p)[0]} >= {(16, 16), (48, 16), (64, 16), (32, 32), (96, 32), (128, 32)}
    terms = {(c.p["form"], c.p["mode"], "big" if C.gemm_big(c.p) else "small", c.p["K"]) for c in _of("gemm", kind="term")}
    assert terms == ({(f, m, s, k) for f in ("NT", "NN") for m in ("x6", "f32") for s in ("small", "big") for k in (16, 48)}
                     | {(f, "x3", s, k) for f in ("NT", "NN") for s, k in (("small", 32), ("small", 96), ("big", 32))})
    assert all(c.p["K"] <= 128 for c in g)
    cp = _of("corr_prep")
    assert {(c.p["C"], c.p["ncenter"]) for c in cp} == {(64, 0), (64, 64), (128, 100), (512, 256), (1024, 256), (72, 72), (1088, 256), (4608, 256)}
    assert {c.p["B"] * c.p["P"] for c in cp} == {7, 8200}
    sm = _of("softmax_rows_")
    assert {(c.p["cols"], c.p["rows"], c.p["div"]) for c in sm} == {(a, b, d) for a in (4, 8, 252, 1028, 4096, 16384) for b in (1, 5) for d in (1.0, 0.01)}
    assert {(c.p["H"], c.p["W"]) for c in _of("rselfcorr")} == {(4, 4), (8, 12), (264, 252)}
    assert {(c.p["H"], c.p["W"], c.p["C"], c.p["k"]) for c in _of("unfold_rows")} == (
        {(h, w, ch, k) for h, w, ch in ((5, 7, 3), (4, 4, 8), (1, 6, 4)) for k in (1, 3, 5)} | {(3, 3, 100, 3)})
    assert {(c.p["H"], c.p["W"], c.p["s"]) for c in _of("patches")} == {(16, 24, 1), (16, 24, 4), (16, 24, 8), (512, 512, 8)}


def test_branch_agrees_with_ops_gemm_passes():
    from ppst_amd import ops
    assert ops.GEMM_MODE["value"] is None and ops.PRECISION["value"] != 2
    for c in _of("gemm"):
        p = c.p
        want = ops._gemm_passes(p["mode"], p["K"]) if (p["form"] == "NT" or p["N"] % 4 == 0) else 0
        assert C.gemm_passes(p["mode"], p["K"], p["N"], p["form"]) == want, c.id
    for mode in ("f32", "x6", "x3"):
        for K in (16, 24, 32, 48, 64, 96):
            assert C.gemm_passes(mode, K) == ops._gemm_passes(mode, K), (mode, K)
    # the fall-throughs, restated: x3 at K % 32 != 0 runs six passes; K % 16 != 0 and (NN) N % 4 != 0 go to the fp32 entry
    assert C.gemm_passes("x3", 48) == 6 and C.gemm_passes("x3", 24) == 0 and C.gemm_passes("x6", 32, 6, "NN") == 0
    mk = lambda **p: C.Case("gemm", "x", dict(b=2, M=129, **p), 0)
    assert C.branch(mk(form="NN", mode="x3", N=132, K=48)) == "split:NN:x6:small"
    assert C.branch(mk(form="NN", mode="x6", N=6, K=32)) == "f32:NN:NTL1"
    assert C.branch(mk(form="NT", mode="x3", N=132, K=96)) == "split:NT:x3:small:BK32"
