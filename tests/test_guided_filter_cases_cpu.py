"""CPU: the judge, the bar and the inputs of tests/test_gpu_guided_filter.py (tests/gf_cases.py) -- nothing here touches a GPU.

  * the float64 restatement is pinned to the oracle: clip(rint(q64)) equals oracle.guided_filter_color(dtype=float64) exactly,
    on every case the GPU file runs;
  * at most 15 % of a case's values lie within tau of a rounding boundary (and are so exempt from exact comparison);
  * the saturating pair leaves [0, 255] on a visible share of its values;
  * the inputs can SEE an error: a stage-2 window one row late and BORDER_REFLECT_101 borders, seeded into the restatement,
    each violate the bar on the blocks and flat-guide inputs at every extent and radius used; a strip-seam defect (the last
    16-output segment of a 192-column strip reads its entering column one short) seeded into the stage-2 boxes violates it on
    both kinds at every radius-30 extent wide enough to hold such a segment (W > 177), and seeded into the stage-1 boxes on the
    blocks inputs (the flat guide, whose a ~ 0, passes a stage-1 seam at 33 x 200 and 97 x 200: max |dq| 0.03 against tau 0.02).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gf_cases as C  # noqa: E402
import ppst_oracle as O  # noqa: E402

ALL_CASES = list(C.CASES_R30) + list(C.CASES_GENERIC)


def _args(case):
    return case if len(case) > 3 else case + (30, C.EPS)


# ------------------------------------------------------------------------------------------------------ the helper itself
def test_box_mean_against_direct_sums():
    rng = np.random.default_rng(3)
    a = rng.normal(size=(9, 11))
    r = 3
    for border, refl in (("symmetric", lambda i, n: -i - 1 if i < 0 else (2 * n - 1 - i if i >= n else i)),
                         ("reflect", lambda i, n: -i if i < 0 else (2 * n - 2 - i if i >= n else i))):
        for dy in (0, 1):
            want = np.empty_like(a)
            for y in range(9):
                for x in range(11):
                    want[y, x] = np.mean([a[refl(y + dy + j, 9), refl(x + i, 11)] for j in range(-r, r + 1) for i in range(-r, r + 1)])
            assert np.allclose(C.box_mean(a, r, border, dy), want, rtol=0, atol=1e-13), (border, dy)
    # the seam switch: outputs 177 .. 191 of a strip keep the entering column of output 176; every other output is untouched
    a = rng.normal(size=(4, 200))
    ap = np.pad(a, r, mode="symmetric")
    want = C.box_mean(a, r).copy()
    for x in range(177, 192):
        want[:, x] += np.array([ap[y:y + 2 * r + 1, 176 + 2 * r].sum() - ap[y:y + 2 * r + 1, x + 2 * r].sum() for y in range(4)]) / (2 * r + 1) ** 2
    assert np.allclose(C.box_mean(a, r, seam=True), want, rtol=0, atol=1e-13)


def test_boundary_distance_and_judge_clauses():
    q = np.array([3.2, 3.49, 3.51, -7.0, -0.4, 0.2, 254.7, 255.0, 300.0, 254.49])
    d, k = C.boundary_distance(q)
    assert np.allclose(d, [0.3, 0.01, 0.01, 7.5, 0.9, 0.3, 0.2, 0.5, 45.5, 0.01])
    e = C.round_u8(q)
    assert list(e) == [3, 3, 4, 0, 0, 0, 255, 255, 255, 254]
    assert C.judge(q, e, 0.0) == [] and C.min_tau(q, e) == 0.0
    g = e.copy(); g[1] = 4; g[2] = 3; g[9] = 255                    # the value across the boundary, within 0.01 of it
    assert C.judge(q, g, 0.02) == [] and abs(C.min_tau(q, g) - 0.01) < 1e-12
    assert C.judge(q, g, 0.005)                                      # ... but not at a smaller tau
    g = e.copy(); g[1] = 2                                           # within tau of 3.5, yet the neighbour on the wrong side
    assert C.judge(q, g, 0.02)
    g = e.copy(); g[0] = 4                                           # 0.3 from the boundary
    assert C.judge(q, g, 0.02)
    g = e.copy(); g[3] = 1                                           # a clipped value has no boundary near it
    assert C.judge(q, g, 0.02)
    g = e.copy(); g[6] = 253                                         # two LSB
    assert any("> 1" in m for m in C.judge(q, g, 0.49))


# -------------------------------------------------------------------------------------------------------------- every case
@pytest.mark.parametrize("case", ALL_CASES, ids=C.case_id)
def test_case_reference_and_sensitivity(case):
    kind, H, W, r, eps = _args(case)
    g, s = C.inputs(kind, H, W)
    R = C.ref(kind, H, W, r, eps)
    # the judge is the oracle's filter
    assert np.array_equal(R.expect, O.guided_filter_color(g, s, r, eps, dtype=np.float64))
    # the float32 oracle itself passes the bar (tau >= tau_ref by construction) and stays within 1 LSB
    assert C.judge(R.q64, R.oracle32, R.tau) == []
    assert 0 < R.tau < 0.5
    print("%-30s tau %.5f (tau_ref %.5f, tau_half %.5f) exempt %.4f saturating %.4f" % (C.case_id(case), R.tau, R.tau_ref, R.tau_half, R.exempt, R.saturating))
    assert R.exempt <= C.EXEMPT_CAP, "%.3f of the values are within tau of a boundary" % R.exempt
    if kind == "saturating":
        assert R.saturating > 0.01, "the clip is not exercised"
    if kind.startswith("const"):
        assert (g == g[0, 0]).all() or (s == s[0, 0]).all()
    if kind == "aliased":
        assert g is s
    if kind in C.SENSITIVE_KINDS:
        seeded = [("stage-2 window one row late", dict(shift2=1)), ("BORDER_REFLECT_101", dict(border="reflect"))]
        if r == 30 and W > C.STRIP - C.SEG + 1:                  # the image holds outputs 1 .. of a strip's last segment
            seeded.append(("strip seam in stage 2", dict(seam=2)))
            if kind == "blocks":
                seeded.append(("strip seam in stage 1", dict(seam=1)))
        for name, kw in seeded:
            q, _, _ = C.restate(g, s, r, eps, **kw)
            assert C.judge(R.q64, C.round_u8(q), R.tau), "the bar does not see: %s" % name
