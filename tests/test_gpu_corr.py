"""GPU: the correspondence kernels of csrc/corr.hip, called through the ppst_amd.ops entry points on every case of
tests/corr_cases.py and compared with its float64 reference -- pytest -m gpu.  The device is never its own judge.

Each case names the kernel its launcher picks (corr_cases.branch restates the launcher's condition and ops._gemm_passes; printed
with the error in the case's units, pytest -s shows the table: profiles/corr_cases_table.txt is that output);
tests/test_corr_cases_cpu.py shows on the CPU that the references are right, that every kernel, edge, K-tile count and loop trip
has a case, and that the comparison used here, at the bar used here, rejects a dropped product term, a dropped last K tile, a zero
ragged tail, a batch element read from its neighbour, an ignored alpha and a wrong ldb on these very inputs.

Next to the references: every kernel is run twice and must repeat bit for bit (no atomics in this file), a batched GEMM equals
its per-element calls, outputs the caller places (NN with ldb > N and ldc > N through the C entry, NT through the C entry, the
in-place softmax, rselfcorr with out_ld = 260) sit between guard values that must survive, and what the entries refuse is
refused without a write.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import corr_cases as C  # noqa: E402
from test_gpu_backward_kernels import POISON, _dev, _guarded, _np, _vp  # noqa: E402

pytestmark = pytest.mark.gpu


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)


# ------------------------------------------------------------------------------------------------------------- runners
def _gemm_entry(c, A, Bm, Cm, ldb, ldc):
    """the C entry of the kernel ops would pick for the case, with the leading dimensions the caller states"""
    from ppst_amd._lib import lib
    p = c.p
    ps = C.gemm_passes(p["mode"], p["K"], p["N"], p["form"])
    b, M, N, K = p["b"], p["M"], p["N"], p["K"]
    if p["form"] == "NT":
        if ps:
            return lib.ppst_gemm_nt_split(_vp(A), _vp(Bm), _vp(Cm), b, M, N, K, p.get("alpha", 1.0), ps, _st())
        return lib.ppst_gemm_nt_f32(_vp(A), _vp(Bm), _vp(Cm), b, M, N, K, p.get("alpha", 1.0), _st())
    if ps:
        return lib.ppst_gemm_nn_split(_vp(A), _vp(Bm), _vp(Cm), b, M, N, K, ldb, ldc, ps, _st())
    return lib.ppst_gemm_nn_f32(_vp(A), _vp(Bm), _vp(Cm), b, M, N, K, ldb, ldc, _st())


def _run_gemm(c, inp, ops):
    p = c.p
    A, Bm = inp["A"].to(_dev()), inp["B"].to(_dev())
    if "ldb" in p:                                 # B and C are the first N columns of wider matrices: the C entry
        wide, check = _guarded((p["b"], p["M"], p["ldc"]))
        rc = _gemm_entry(c, A, Bm, wide, p["ldb"], p["ldc"])
        torch.cuda.synchronize()
        assert rc == 0
        check()
        assert bool((wide[..., p["N"]:] == POISON).all()), "wrote the columns N .. ldc"
        return {"C": wide[..., :p["N"]]}
    if p["form"] == "NT":
        return {"C": ops.gemm_nt(A, Bm, p.get("alpha", 1.0), mode=p["mode"])}
    return {"C": ops.gemm_nn(A, Bm, mode=p["mode"])}


def _run_corr_prep(c, inp, ops):
    return {"y": ops.corr_prep(inp["x"].to(_dev()), c.p["ncenter"])}


def _run_softmax_rows_(c, inp, ops):
    x, check = _guarded(inp["x"].shape, inp["x"].to(_dev()))
    r = ops.softmax_rows_(x, c.p["div"])
    torch.cuda.synchronize()
    check()
    return {"p": r}


def _run_rselfcorr(c, inp, ops):
    p = c.p
    fea = inp["fea"].to(_dev())
    if "out_ld" not in p:
        return {"out": ops.rselfcorr(fea)}
    wide, check = _guarded((p["B"], p["H"] // 4, p["W"] // 4, p["out_ld"]))
    out = ops.rselfcorr(fea, out=wide[..., :256])
    torch.cuda.synchronize()
    check()
    assert bool((wide[..., 256:] == POISON).all()), "wrote the channels 256 .. out_ld"
    return {"out": out}


def _run_unfold_rows(c, inp, ops):
    return {"rows": ops.unfold_rows(inp["x"].to(_dev()), c.p["k"])}


def _run_patches(c, inp, ops):
    p = c.p
    x = inp["x"].to(_dev())
    un = ops.unfold_patches(x, p["s"])
    assert torch.equal(ops.fold_patches(un, p["C"], p["H"], p["W"], p["s"]), x), "fold(unfold(x)) is not x"
    return {"unfold": un, "fold": ops.fold_patches(inp["y"].to(_dev()), p["C"], p["H"], p["W"], p["s"])}


RUN = {k[5:]: v for k, v in list(globals().items()) if k.startswith("_run_")}


def _run(c):
    from ppst_amd import ops
    out = RUN[c.op](c, C.inputs(c.id), ops)
    torch.cuda.synchronize()
    return {k: _np(v) for k, v in out.items()}


def _row(c, k, err):
    u, b = C.unit(c, k), C.bar(c, k)
    what = {C.U24: "2^-24 S", C.U17: "2^-17 S"}.get(u, "bars" if b else "(bit equal)")
    return "%-46s %-7s %-26s err %9.3f  bar %7.2f  %s" % (c.id, k, C.branch(c), err / u, b / u, what)


# --------------------------------------------------------------------------------------------- against the float64 reference
@pytest.mark.parametrize("cid", [c.id for c in C.CASES])
def test_against_float64_reference(cid):
    c = C.by_id(cid)
    ref, got = C.reference(cid), _run(c)
    assert set(got) == set(ref)
    fails = []
    for k in sorted(ref):
        bad, err = C.judge(c, k, got[k])
        print(_row(c, k, err))
        fails += ["%s: %s" % (k, m) for m in bad]
    assert not fails, "%s [%s]: %s" % (cid, C.branch(c), "; ".join(fails))
    again = _run(c)
    for k in got:
        assert np.array_equal(again[k], got[k]), "%s: two runs differ" % k


# ---------------------------------------------------------------------------------------- a batch is its per-element calls
@pytest.mark.parametrize("cid", [c.id for c in C.CASES if c.op == "gemm" and c.p["b"] == 2 and "ldb" not in c.p and c.p.get("kind") != "term"])
def test_batched_gemm_equals_its_per_element_calls(cid):
    from ppst_amd import ops
    c = C.by_id(cid)
    inp = C.inputs(cid)
    whole = _run(c)["C"]
    for b in range(c.p["b"]):
        c1 = c._replace(p=dict(c.p, b=1))
        assert C.branch(c1) == C.branch(c), "the single call would take another kernel"
        one = _np(_run_gemm(c1, {k: v[b:b + 1] for k, v in inp.items()}, ops)["C"])
        assert np.array_equal(one[0], whole[b]), "element %d of the batch differs from its single call" % b


# ------------------------------------------------------------------------------------- NT through the C entry: guards
@pytest.mark.parametrize("cid", ["gemm-NT-x6-small-ragged-2x129x132x48", "gemm-NT-x3-small-ragged-2x129x132x96", "gemm-NT-x6-big-one-block-224x129x132x16",
                                 "gemm-NT-f32-2x130x128x16", "gemm-NT-f32-2x1x132x48", "gemm-NT-f32-2x1x70x16"])
def test_nt_entries_write_their_output_and_nothing_else(cid):
    c = C.by_id(cid)
    inp, p = C.inputs(cid), c.p
    out, check = _guarded((p["b"], p["M"], p["N"]))
    rc = _gemm_entry(c, inp["A"].to(_dev()), inp["B"].to(_dev()), out, None, None)
    torch.cuda.synchronize()
    assert rc == 0
    check()
    bad, err = C.judge(c, "C", _np(out))
    print(_row(c, "C", err))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_raise_and_write_nothing():
    from ppst_amd import ops
    from ppst_amd._lib import lib
    dev = _dev()
    a24, b24 = torch.ones(1, 8, 24, device=dev), torch.ones(1, 8, 24, device=dev)
    a16, b6 = torch.ones(1, 8, 16, device=dev), torch.ones(1, 16, 6, device=dev)
    dst = torch.full((4, 16388), POISON, device=dev)
    calls = [
        ("gemm_nt_split K = 24", lambda: lib.ppst_gemm_nt_split(_vp(a24), _vp(b24), _vp(dst), 1, 8, 8, 24, 1.0, 6, _st())),
        ("gemm_nt_f32 K = 24", lambda: lib.ppst_gemm_nt_f32(_vp(a24), _vp(b24), _vp(dst), 1, 8, 8, 24, 1.0, _st())),
        ("gemm_nt_split x3 K = 48", lambda: lib.ppst_gemm_nt_split(_vp(dst), _vp(dst), _vp(dst), 1, 8, 8, 48, 1.0, 3, _st())),
        ("gemm_nt_split passes = 4", lambda: lib.ppst_gemm_nt_split(_vp(dst), _vp(dst), _vp(dst), 1, 8, 8, 32, 1.0, 4, _st())),
        ("gemm_nn_split N = 6", lambda: lib.ppst_gemm_nn_split(_vp(a16), _vp(b6), _vp(dst), 1, 8, 6, 16, 6, 6, 6, _st())),
        ("gemm_nn_f32 N = 6", lambda: lib.ppst_gemm_nn_f32(_vp(a16), _vp(b6), _vp(dst), 1, 8, 6, 16, 6, 6, _st())),
        ("gemm_nn_split ldb < N", lambda: lib.ppst_gemm_nn_split(_vp(dst), _vp(dst), _vp(dst), 1, 8, 8, 16, 4, 8, 6, _st())),
        ("gemm_nn_f32 ldc < N", lambda: lib.ppst_gemm_nn_f32(_vp(dst), _vp(dst), _vp(dst), 1, 8, 8, 16, 8, 4, _st())),
        ("softmax cols = 6", lambda: lib.ppst_softmax_rows(_vp(dst), 4, 6, 1.0, _st())),
        ("softmax cols = 16388", lambda: lib.ppst_softmax_rows(_vp(dst), 4, 16388, 1.0, _st())),
        ("softmax div = 0", lambda: lib.ppst_softmax_rows(_vp(dst), 4, 8, 0.0, _st())),
        ("corr_prep ncenter > C", lambda: lib.ppst_corr_prep(_vp(dst), _vp(dst), 1, 4, 64, 65, _st())),
        ("rselfcorr C = 32", lambda: lib.ppst_rselfcorr(_vp(dst), _vp(dst), 1, 4, 4, 32, 256, _st())),
        ("rselfcorr out_ld = 258", lambda: lib.ppst_rselfcorr(_vp(dst), _vp(dst), 1, 4, 4, 64, 258, _st())),
        ("unfold_rows k = 2", lambda: lib.ppst_unfold_rows(_vp(dst), _vp(dst), 1, 4, 4, 4, 2, _st())),
        ("unfold_patches H % s", lambda: lib.ppst_unfold_patches(_vp(dst), _vp(dst), 1, 3, 6, 8, 4, _st())),
    ]
    for why, call in calls:
        rc = call()
        torch.cuda.synchronize()
        assert rc == -1, "%s: returned %d, not PPST_EINVAL" % (why, rc)
        assert bool((dst == POISON).all()), "%s: a refused call wrote" % why
    # ops names the constraint before any entry is reached
    with pytest.raises(ValueError, match="K % 16"):
        ops.gemm_nt(a24, b24)
    with pytest.raises(ValueError, match="N % 4"):
        ops.gemm_nn(a16, b6)
    with pytest.raises(ValueError, match="K % 16"):
        ops.gemm_nn(a24, torch.ones(1, 24, 8, device=dev), mode="x3")
    for cols in (6, 16388):
        with pytest.raises(ValueError, match="cols"):
            ops.softmax_rows_(dst[:, :cols].contiguous() if cols == 6 else dst, 1.0)
    torch.cuda.synchronize()
    assert bool((dst == POISON).all())
