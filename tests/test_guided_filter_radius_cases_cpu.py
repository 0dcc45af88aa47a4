"""CPU: the cases and the bar of tests/test_gpu_guided_filter_radius.py (tests/gf_radius_cases.py), and the radius rule of the
model (ppst_model.guided_filter_radius) -- nothing here touches a GPU.

For every case of the fused radii 60 and 90:
  * clip(rint(q64)) equals oracle.guided_filter_color(dtype=float64) exactly;
  * the float32 oracle passes the bar, 0 < tau < 0.5, and at most 15 % of the values lie within tau of a rounding boundary;
  * the inputs SEE a defect through the bar (blocks and flat guide): BORDER_REFLECT_101 at every extent; a stage-2 window one
    row late wherever H >= r + 2 (at H = r + 1 the window already spans the whole reflected image and a one-row shift moves
    too little: not required there); with gf_cases.STRIP / SEG set to the radius's geometry, a strip seam in stage 2 on both
    kinds and in stage 1 on the blocks inputs, at every width that holds a strip's last segment (the flat guide, whose a ~ 0,
    is not required to see a stage-1 seam, as at radius 30).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gf_cases as C  # noqa: E402
import gf_radius_cases as RC  # noqa: E402
import ppst_oracle as O  # noqa: E402


def test_cases_sit_on_the_geometry():
    assert RC.RADII == (60, 90)
    for r in RC.RADII:
        S, seg, vs1 = RC.GEOM[r]["strip"], RC.GEOM[r]["seg"], RC.GEOM[r]["vs1"]
        assert S % seg == 0 and vs1 in (32, 64, 128)
        ext = RC.extents(r)
        assert (r + 1, r + 1) in ext and (r + 2, r + 1) in ext and (600, 530) in ext
        widths = {w for (_, w) in ext}
        assert {min(w, 2048) for w in (S - 1, S, S + 1, 2 * S - 1, 2 * S + 1)} <= widths and 2048 in widths
        for kind in ("saturating", "const_both", "aliased", "smooth"):
            assert (kind, 130, S + 1, r, C.EPS) in RC.CASES
        assert any(c[3] == r and c[4] == RC.EPS_LARGE for c in RC.CASES)
        assert all(h > r and w > r and w <= 2048 for (_, h, w, rr, _) in RC.CASES if rr == r)
    assert ("blocks", 1024, 1024, 60, C.EPS) in RC.CASES
    assert not any(h * w > 1024 * 1024 for (_, h, w, _, _) in RC.CASES)
    # the factor of tau_half: (runs + 1) / 2, which is 2 at r = 30 with 32 rows; 32 rows give 3 at r = 60 and 4 at r = 90, 64 rows 2.5
    assert (2 * 30 - 1) // 32 + 2 == 3
    assert {(r, RC.GEOM[r]["vs1"]): (RC.runs(r) + 1) / 2 for r in RC.RADII} == {(60, 32): 3.0, (90, 64): 2.5}
    assert (2 * 90 - 1) // 32 + 2 == 7


@pytest.mark.parametrize("case", RC.CASES, ids=C.case_id)
def test_case_reference_and_sensitivity(case, monkeypatch):
    kind, H, W, r, eps = case
    g, s = C.inputs(kind, H, W)
    R = RC.ref(*case)
    assert np.array_equal(R.expect, O.guided_filter_color(g, s, r, eps, dtype=np.float64))
    assert C.judge(R.q64, R.oracle32, R.tau) == []
    print("%-34s tau %.5f (tau_ref %.5f, tau_half %.5f, factor %.1f) exempt %.4f saturating %.4f"
          % (C.case_id(case), R.tau, R.tau_ref, R.tau_half, (RC.runs(r) + 1) / 2, R.exempt, R.saturating))
    assert 0 < R.tau < 0.5
    assert R.exempt <= C.EXEMPT_CAP, "%.3f of the values are within tau of a boundary" % R.exempt
    if kind == "saturating":
        assert R.saturating > 0.01, "the clip is not exercised"
    if kind == "aliased":
        assert g is s
    if kind in C.SENSITIVE_KINDS:
        S, seg = RC.GEOM[r]["strip"], RC.GEOM[r]["seg"]
        monkeypatch.setattr(C, "STRIP", S)
        monkeypatch.setattr(C, "SEG", seg)
        seeded = [("BORDER_REFLECT_101", dict(border="reflect"))]
        if H >= r + 2:
            seeded.append(("stage-2 window one row late", dict(shift2=1)))
        if W > S - seg + 1:                                       # the image holds outputs 1 .. of a strip's last segment
            seeded.append(("strip seam in stage 2", dict(seam=2)))
            if kind == "blocks":
                seeded.append(("strip seam in stage 1", dict(seam=1)))
        for name, kw in seeded:
            q, _, _ = C.restate(g, s, r, eps, **kw)
            assert C.judge(R.q64, C.round_u8(q), R.tau), "the bar does not see: %s" % name


def test_seam_switch_follows_the_patched_geometry(monkeypatch):
    """box_mean(seam=True) with STRIP / SEG set to a fused radius's geometry touches outputs 1 .. SEG - 1 of each strip's last
    segment and nothing else"""
    rng = np.random.default_rng(5)
    for r in RC.RADII:
        S, seg = RC.GEOM[r]["strip"], RC.GEOM[r]["seg"]
        monkeypatch.setattr(C, "STRIP", S)
        monkeypatch.setattr(C, "SEG", seg)
        a = rng.normal(size=(3, 2 * S + 1))
        changed = np.abs(C.box_mean(a, 2, seam=True) - C.box_mean(a, 2)).max(axis=0) > 0
        want = np.array([x % S - (S - seg) >= 1 for x in range(2 * S + 1)])
        assert np.array_equal(changed, want), r


def test_guided_filter_radius_rule():
    from ppst_amd.ppst_model import Options, guided_filter_radius

    class Bare:                                                    # an option object built elsewhere, without the attribute
        pass

    for h in (256, 512, 1024, 1536):
        assert guided_filter_radius(Options(), h, h) == 30
        assert guided_filter_radius(Bare(), h, h) == 30
        assert guided_filter_radius(Options(gf_radius=45), h, h) == 45
    assert Options().gf_radius == 30
    scaled = Options(gf_radius="scaled")
    assert [guided_filter_radius(scaled, h, h) for h in (256, 512, 1024, 1536)] == [30, 30, 60, 90]
    assert guided_filter_radius(scaled, 300, 512) == 30
    for h, w in ((2048, 2048), (1024, 512), (768, 768)):           # sizes the correspondence refuses
        with pytest.raises(ValueError):
            guided_filter_radius(scaled, h, w)
    with pytest.raises(ValueError):
        guided_filter_radius(Options(gf_radius="auto"), 512, 512)
