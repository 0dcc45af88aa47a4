"""CPU: the case list of the conv-epilogue tests (tests/conv_epi_cases.py) is what it claims -- every kernel family is there with all
nine (activation, residual) combinations and its bare run, and every case, run through ops.ConvPlan without a device
(tests/conv_plan_record.py's proxy library), ends in the launch its family names: a mis-specified case cannot silently test
another kernel."""
import pytest
import torch

import conv_epi_cases as CE
import conv_plan_record as CPR


def test_every_family_and_combination_is_present():
    variants = {(f.expect["entry"], f.expect.get("variant"), f.expect["tile_rows"], f.expect["dual_b"], f.expect["k64"])
                for f in CE.FAMILIES.values()}
    mfma = "ppst_conv2d_mfma"
    # tile kernel and its 8-row form; N-256, phase pairs, nine products, K64 on N-256 and on the 24-row tile; streaming 1x1 and the two
    # direct forms; Winograd; exact fp32
    assert variants >= {(mfma, 0, 16, 0, 0), (mfma, 0, 8, 0, 0), (mfma, 2, 16, 0, 0), (mfma, 2, 16, 1, 0), (mfma, 11, 15, 0, 0),
                        (mfma, 2, 16, 0, 1), (mfma, 9, 24, 0, 1), (mfma, 4, 16, 0, 0), (mfma, 5, 16, 0, 0), (mfma, 6, 16, 0, 0),
                        (mfma, 10, 16, 0, 0), ("ppst_conv2d_f32", None, 16, 0, 0)}
    assert {f.expect["bn"] for f in CE.FAMILIES.values() if f.expect.get("variant") == 0} == {64, 128}
    for name in CE.FULL_FAMILIES:
        got = {(c.act, c.res) for c in CE.CASES if c.family == name and c.full}
        # the nine-product upscale refuses a residual and PReLU at its entry
        assert got == ({("none", "none"), ("lrelu", "none")} if name == "up9" else set(CE.NINE)), name
    for name, f in CE.FAMILIES.items():
        assert sum(1 for c in CE.CASES if c.family == name and not c.full) == 1, name
        assert any(c.family == name and c.full for c in CE.CASES), name
    assert {(f.precision, f.dtype) for f in CE.FAMILIES.values() if f.dtype != torch.float32} == {(1, torch.bfloat16), (3, torch.float16)}
    assert any(f.precision == 2 for f in CE.FAMILIES.values())
    for group in CE.EQUAL:
        assert len({CE.data_name(CE.FAMILIES[n]) for n in group}) == 1 and all(n in CE.FULL_FAMILIES for n in group)


@pytest.mark.parametrize("cid", [c.id for c in CE.CASES])
def test_case_reaches_the_launch_its_family_names(cid):
    c = CE.by_id(cid)
    f = CE.FAMILIES[c.family]
    (ih, iw, ic), (oh, ow) = CE.geometry(f)
    assert (oh, ow) == ((18, 20) if f.kind == "convT" else (17, 19))
    with CPR.host_only_ops() as (ops, proxy):
        t = {"x": CPR.fake(CE.B, ih, iw, ic, dtype=f.dtype), "w": torch.empty(f.cout, f.cin, f.k, f.k), "bias": CPR.fake(f.cout),
             "noise": CPR.fake(CE.B, 1, oh, ow), "res": CPR.fake(CE.B, oh, ow, f.cout, dtype=f.dtype), "prelu": CPR.fake(1),
             "out": CPR.fake(CE.B, oh, ow, f.cout, dtype=f.dtype)}
        before = {n: (dict(v) if isinstance(v, dict) else v) for n, v in vars(ops).items() if n in f.switches}
        proxy.calls.clear()
        CE.call(ops, c, t)
        assert before == {n: (dict(v) if isinstance(v, dict) else v) for n, v in vars(ops).items() if n in f.switches}
        launches = [call for call in proxy.calls if call[0].startswith("ppst_conv2d")]
    assert len(launches) == 1
    entry, args, _ = launches[0]
    a = args[0]._obj
    got = {k: (entry if k == "entry" else getattr(a, k)) for k in f.expect}
    assert got == f.expect
    assert (a.B, a.tile_h, a.tile_w, a.out_h, a.out_w, a.cout, a.precision) == ((CE.B,) + ((9, 10) if f.kind == "convT" else (17, 19))
                                                                                 + (oh, ow, f.cout, f.precision))
    # the epilogue options of the case arrive in the launch
    assert (bool(a.bias), bool(a.noise), bool(a.stats), bool(a.residual)) == (c.full, c.full, c.full, c.full and c.res != "none")
    want_act = {"none": ops.ACT_NONE, "lrelu": ops.ACT_LRELU, "prelu": ops.ACT_PRELU}[c.act] | (0x100 if c.res == "after" else 0)
    assert a.act == want_act and bool(a.prelu) == (c.full and c.act == "prelu")
    if c.full:
        assert abs(a.noise_weight - CE.NOISE_WEIGHT) < 1e-7 and abs(a.out_scale - CE.OUT_SCALE) < 1e-7
    else:
        assert a.noise_weight == 0.0 and a.out_scale == 1.0
