"""GPU: the output arithmetic of every forward conv kernel family (csrc/conv_common.h: conv_epi_value and the shared transposition
epilogue) over the cross product no other test walks -- (none, lrelu, prelu) x (no residual, before, after the activation), each
with bias, noise, out_scale and tile statistics, and one bare run per family (tests/conv_epi_cases.py).

  * against float64 torch at the bars of tests/gpu_diag.py t_conv (3e-5 bf16x3, 2e-2 / 3e-3 single-pass bf16 / fp16, 5e-6 fp32;
    the statistics' sums at 1e-5);
  * the direct families that compute the same sum agree to the bit (tile / N-256 / 8-row; direct 3x3, direct, streaming 1x1
    against the tile kernel);
  * every output and statistics tensor has the sha256 the parent commit produced (tests/golden/conv_epilogue_parent.json,
    tests/conv_epi_record.py): restating the epilogue once moved no bit.

Every case is launched once (module fixture); a launch is a few hundred microseconds."""
import json
import os

import pytest
import torch

import conv_epi_cases as CE
import conv_epi_record

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def outputs():
    from ppst_amd import ops
    return conv_epi_record.run_all(ops)


def _rel(got, ref):
    assert tuple(got.shape) == tuple(ref.shape)
    return (got.double() - ref).abs().max().item() / ref.abs().max().item()


@pytest.mark.parametrize("cid", [c.id for c in CE.CASES])
def test_case_against_float64(outputs, cid):
    c = CE.by_id(cid)
    f = CE.FAMILIES[c.family]
    y, st = outputs[cid]
    ref, ref_st = CE.reference(c)
    assert y.dtype == f.dtype
    err = _rel(y, ref)
    print("%-32s output rel %.3e (bar %.0e)" % (cid, err, CE.BAR[f.precision]))
    assert err <= CE.BAR[f.precision], err
    assert (st is None) == (ref_st is None)
    if st is not None:
        sums = st.double().sum(1)                    # (B, tiles, Cout, 2) -> per image and channel
        for i, what in enumerate(("sum", "sum of squares")):
            e = _rel(sums[..., i], ref_st[..., i])
            print("%-32s %s rel %.3e (bar %.0e)" % (cid, what, e, CE.BAR_STATS[f.precision]))
            assert e <= CE.BAR_STATS[f.precision], (what, e)


@pytest.mark.parametrize("group", CE.EQUAL, ids=lambda g: "=".join(g))
def test_direct_families_agree_to_the_bit(outputs, group):
    first = CE.FAMILIES[group[0]]
    for other in group[1:]:
        assert CE.data_name(CE.FAMILIES[other]) == CE.data_name(first)
        cases = [c for c in CE.CASES if c.family == other]
        assert len(cases) == 10
        for c in cases:
            y0 = outputs[c.id.replace(other, group[0], 1)][0]
            assert torch.equal(outputs[c.id][0], y0), c.id


def test_hashes_equal_the_parent_commit(outputs):
    with open(os.path.join(HERE, "golden", "conv_epilogue_parent.json")) as fh:
        want = json.load(fh)
    want.pop("_doc")
    assert sorted(want) == sorted(c.id for c in CE.CASES)
    got = {cid: {"y": conv_epi_record.sha(y), "stats": conv_epi_record.sha(st)} for cid, (y, st) in outputs.items()}
    assert [cid for cid in sorted(want) if got[cid] != want[cid]] == []
