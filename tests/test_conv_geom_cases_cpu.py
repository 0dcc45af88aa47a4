"""CPU: the case list of the conv-geometry tests (tests/conv_geom_cases.py) is what it claims.

  * every family has every facet that applies to it (FACETS below states the expected set; what a family's matrix leaves out is
    DROPPED, with the reason);
  * every case, run through ops.ConvPlan without a device (tests/conv_plan_record.py's proxy library, caller-owned fake tensors),
    ends in exactly one conv launch whose fields are the family's ``expect`` and the case's geometry, and that launch's argument
    block, replayed through the real entry point with B = 0, is accepted: no case can be refused on the GPU by a shape check;
  * ``judge`` rejects every seeded defect at the case's own bar on the case's own data, every defect changes the reference where it
    applies, and every family sees every defect that can apply to it;
  * the float32 evaluation of the reference stays under a quarter of every bar: the reference alone is never the reason.

Measured where this was written (CPU only): the whole file 19 s, of which the defect sweep 13 s and the float32 evaluation 3 s."""
import ctypes

import pytest
import torch

import conv_geom_cases as G
import conv_plan_record as CPR

_HALO_PADS = {(1, 1): ("zero", "replicate"), (1, 5): ("zero", "replicate"), (5, 1): ("zero", "replicate"), (2, 3): G.PADS, (16, 16): G.PADS,
              (33, 35): G.PADS}


def _matrix(pads_of, loads=("plain", "ss_prelu"), extra=("ss", "ss_lrelu")):
    out = set()
    for (h, w) in _HALO_PADS:
        for pad in pads_of((h, w)):
            for load in loads + (extra if ((h, w) == (33, 35) and pad == "zero") else ()):
                out.add("%dx%d/%s/%s" % (h, w, pad, load))
    return out


_HALO = _matrix(lambda hw: _HALO_PADS[hw]) | {"slices/plain", "slices/ss_prelu"}
_NO_HALO = _matrix(lambda hw: ("zero",)) | {"slices/plain", "slices/ss_prelu"}
_PLAIN = _matrix(lambda hw: ("zero",), ("plain",), ()) | {"slices/plain"}          # stride-2 convs, nine-product upscale
_CIN = {"cin1", "cin2", "cin3", "cin5"}
FACETS = {
    "tile64": _HALO | _CIN | {"nlast"}, "tile128": _HALO | _CIN | {"nlast"}, "tile256": _HALO | _CIN, "row8": _HALO | _CIN | {"nlast"},
    "tile1x1": _NO_HALO | _CIN, "tile_s2d": _PLAIN | _CIN | {"nlast"}, "convT4": _HALO | _CIN | {"nlast"},
    "n256": _HALO | _CIN | {"nlast"}, "dual": _HALO | _CIN | {"nlast"}, "up9": _PLAIN | _CIN | {"nlast"},
    "stream1": _NO_HALO | {"slices/ss_res", "cin1", "cin2", "cin4", "nlast"}, "direct5": _PLAIN | {"cin1", "cin2", "cin4", "nlast"},
    "direct3": _HALO | {"cin1", "cin2", "cin4", "nlast"}, "wino": _HALO | _CIN | {"nlast", "32x32/zero/ss_prelu"},
    "tile_bf16": _HALO | _CIN, "tile_fp16": _HALO | _CIN, "k64_n256_bf16": _HALO | {"cin2", "cin6"}, "k64_row24_fp16": _HALO | {"cin2", "cin6"},
    "f32": _HALO | _CIN, "row32_bf16x1": _HALO | _CIN | {"nlast"},
}


def test_every_family_has_every_applicable_facet():
    assert set(G.FAMILIES) == set(G.CE.FAMILIES) | {"row32_bf16x1"} == set(FACETS)
    f = G.FAMILIES["row32_bf16x1"]
    assert (f.kind, f.cin, f.cout, f.k, f.precision, f.dtype) == ("conv", 64, 128, 3, 1, torch.float32)
    assert {k: f.expect[k] for k in ("variant", "bn", "tile_rows", "io_st")} == dict(variant=7, bn=128, tile_rows=32, io_st=0)
    for name in G.FAMILIES:
        assert {c.facet for c in G.CASES if c.family == name} == FACETS[name], name
        assert len([c for c in G.CASES if c.family == name]) == len(FACETS[name]), name
    # what the matrices leave out: reflect at an extent of 1 everywhere, everything but (zero, plain) for the nine-product upscale
    # and in_ss for the stride-2 convs
    want = set()
    for name, f in G.FAMILIES.items():
        full = (_HALO if G.has_halo(f) else _NO_HALO) | {"%dx%d/reflect/%s" % (h, w, l) for (h, w) in ((1, 1), (1, 5), (5, 1))
                                                         for l in ("plain", "ss_prelu") if G.has_halo(f)}
        want |= {(name, facet) for facet in full - FACETS[name]}
    assert set(G.DROPPED) == want
    for (name, facet), why in G.DROPPED.items():
        if "/reflect/" in facet and facet.split("/")[0] in ("1x1", "1x5", "5x1"):
            assert "undefined" in why
        else:
            assert name in ("up9", "tile_s2d", "direct5") and ("nine-product" in why) == (name == "up9")
    assert all(c.hw != (1, 1) or c.pad != "reflect" for c in G.CASES)
    # the channel counts: Cin in chunks, the last N tile
    for c in G.CASES:
        if c.facet.startswith("cin"):
            assert c.cin == int(c.facet[3:]) * (64 if c.family.startswith("k64") else 32) and c.hw == (17, 19)
        if c.facet == "nlast":
            bn = G.FAMILIES[c.family].expect["bn"]
            # (the streaming and direct kernels walk their N tile in 16-channel sub-tiles, two of them for Cout <= 32: Cout 36 is the
            #  first that leaves four channels in a third)
            assert (c.cout % (32 if c.family in ("stream1", "direct3", "direct5") else bn) == 4
                    or (c.family, c.cout) in (("n256", 512), ("dual", 384), ("up9", 64)))
    for group in G.EQUAL:
        shared = [{G.conv_name(c) for c in G.CASES if c.family == n} for n in group]
        assert len(set.intersection(*shared)) >= len(_PLAIN), group


def test_inputs_are_what_the_docstring_says():
    c = G.by_id("wino-33x35-zero-ss_prelu-dense-c64x128")
    t = G.make(c)
    ss = t["ss"]
    assert tuple(ss.shape) == (3, 64, 2) and float(ss.abs().min()) >= 0.5 and float(ss.abs().max()) <= 1.5
    assert bool((ss[..., 0] < 0).any()) and bool((ss[..., 0] > 0).any()) and bool((ss[..., 1] < 0).any()) and not torch.equal(ss[0], ss[1])
    assert G.make(G.by_id("tile128-33x35-zero-ss_prelu-dense-c32x160")) is not t
    for a, b in (("tile256", "n256"), ("tile256", "row8")):       # one group, one set of tensors and one reference
        ca, cb = (G.by_id("%s-33x35-reflect-ss_prelu-dense-c64x256" % n) for n in (a, b))
        assert G.make(ca) is G.make(cb) and G.reference(ca) is G.reference(cb)
    # the border of x is never zero (zero padding would equal replicate padding there), slices start on 16-byte items
    for c in G.CASES:
        if c.hw == (2, 3):
            assert float(G.view(G.make(c)["x"]).float().abs().min()) > 0
    t = G.make(G.by_id("tile_fp16-33x35-zero-ss_prelu-slices-c32x96"))
    assert t["x"].wide.dtype == torch.float16 and (t["x"].lo, t["x"].wide.shape[-1]) == (32, 96) and (t["res"].lo, t["res"].wide.shape[-1]) == (32, 128)


def test_convT_reference_by_padding_equals_the_zero_padding_one():
    """conv_transpose2d over the explicitly padded input, cropped, is the transposed conv for mode ``constant`` (float64)"""
    import ppst_oracle as O
    c = G.by_id("convT4-33x35-zero-plain-dense-c32x96")
    t = G.make(c)
    x, w = G.view(t["x"]).double().permute(0, 3, 1, 2), t["w"].double()
    direct = torch.nn.functional.conv_transpose2d(x, O.upscale_weight(w), stride=2, padding=1) + t["bias"].double()[:, None, None]
    got = G.reference(c)[0].permute(0, 3, 1, 2)
    assert got.shape == direct.shape and float((got - direct).abs().max()) <= 1e-13 * float(direct.abs().max())


def test_tile_counts_of_the_large_extent():
    from ppst_amd._lib import lib
    t = lambda rows: lib.ppst_conv_tiles(33, 35, rows)
    assert (t(16), t(8), t(24), t(32), t(15)) == (3 * 3, 5 * 3, 2 * 3, 2 * 3, 3 * 3)
    assert lib.ppst_conv_tiles(16, 16, 16) == 1 and lib.ppst_conv_tiles(17, 19, 16) == 4
    # the interior tile (1, 1): rows 16 .. 31 with the halo row 32 = the last row; last tile row 1 high, last tile column 3 wide
    assert 16 + 16 == 33 - 1 and 33 - 32 == 1 and 35 - 32 == 3


def _a_slots(f, c):
    return 3 if f.kind == "s2d" else min(3, c.cin // 32)


@pytest.mark.parametrize("cid", [c.id for c in G.CASES])
def test_case_reaches_its_launch_and_passes_the_entry(cid):
    from ppst_amd import _lib
    c = G.by_id(cid)
    f = G.FAMILIES[c.family]
    (ih, iw, ic), (oh, ow), osy = G.geometry(c)
    sl = c.layout == "slices"
    wide = lambda h, w, ch, lo, extra: CPR.fake(G.B, h, w, ch + (extra if sl else 0), dtype=f.dtype)[..., (lo if sl else 0):(lo if sl else 0) + ch]
    with CPR.host_only_ops() as (ops, proxy):
        t = {"x": wide(ih, iw, ic, G.X_LO, G.X_EXTRA), "w": torch.empty(c.cout, c.cin, f.k, f.k), "bias": CPR.fake(c.cout),
             "out": wide(oh, ow, c.cout, G.OUT_LO, G.OUT_EXTRA), "ss": CPR.fake(G.B, ic, 2), "prelu": CPR.fake(1),
             "in_res": wide(ih, iw, ic, G.INRES_LO, G.INRES_EXTRA), "res": wide(oh, ow, c.cout, G.RES_LO, G.RES_EXTRA)}
        names = set(f.switches) | {"DIRECT_MAX", "FAT_MIN_BLOCKS"}
        snap = lambda: {n: (dict(v) if isinstance(v, dict) else v) for n, v in vars(ops).items() if n in names}
        before = snap()
        proxy.calls.clear()
        G.call(ops, c, t)
        assert snap() == before
        launches = [call for call in proxy.calls if call[0].startswith("ppst_conv2d")]
        want_pad, want_act = getattr(ops, G.PAD_NAME[c.pad]), getattr(ops, G.IN_ACT_NAME[c.load])
    assert len(launches) == 1
    entry, args, _ = launches[0]
    a = args[0]._obj
    assert {k: (entry if k == "entry" else getattr(a, k)) for k in f.expect} == f.expect
    assert (a.B, a.tile_h, a.tile_w, a.in_h, a.in_w, a.out_h, a.out_w, a.cout, a.precision) == (G.B,) + c.hw + (ih, iw, oh, ow, c.cout, f.precision)
    ss = c.load != "plain"
    assert (a.pad_mode, a.in_act, a.in_c, bool(a.in_scale_shift), bool(a.in_prelu), bool(a.in_res)) == (
        want_pad, want_act, ic if ss else 0, ss, c.load in ("ss_prelu", "ss_res"), c.load == "ss_res")
    res = G.epilogue(c) == "lrelu_after"
    assert (a.in_ld, a.out_ld, a.res_ld, a.in_res_ld) == (ic + (G.X_EXTRA if sl else 0), c.cout + (G.OUT_EXTRA if sl else 0),
                                                          c.cout + G.RES_EXTRA if res else 0, ic + G.INRES_EXTRA if c.load == "ss_res" else 0)
    assert bool(a.residual) == res and a.act == ((ops.ACT_LRELU | 0x100) if res else ops.ACT_NONE) and bool(a.bias) and bool(a.stats)
    assert a.a_slots == _a_slots(f, c) and a.ksplit == 0
    # the slices start where the case says, on the 16-byte grid of the kernels' items
    es = 4 if f.dtype == torch.float32 else 2
    assert a.x == t["x"].data_ptr() and a.y == t["out"].data_ptr() and (a.x - t["x"]._base.data_ptr() if sl else 0) == (G.X_LO * es if sl else 0)
    assert (G.X_LO * es) % 16 == 0 and (G.OUT_LO * es) % 16 == 0 and (G.RES_LO * es) % 16 == 0 and (G.INRES_LO * 4) % 16 == 0
    # ---- the real entry, B = 0: every shape check runs, nothing is dereferenced or launched
    a.B = 0
    if entry == "ppst_conv2d_f32":
        rc = _lib.lib.ppst_conv2d_f32(*((ctypes.byref(a),) + tuple(args[1:])))
    else:
        rc = _lib.lib.ppst_conv2d_mfma(ctypes.byref(a), None)
    assert rc == 0, rc


def test_reference_in_float32_is_within_a_quarter_of_every_bar():
    seen = set()
    for c in G.CASES:
        key = (G.conv_name(c), G.FAMILIES[c.family].precision)
        if key in seen:
            continue
        seen.add(key)
        p = G.FAMILIES[c.family].precision
        ey, es, eq = G.err32(c)
        assert ey <= G.BAR[p] / 4 and es <= G.BAR_STATS[p] / 4 and eq <= G.BAR_STATS[p] / 4, (c.id, ey, es, eq)


def test_judge_accepts_the_reference_and_rejects_every_seeded_defect():
    """Every defect, on every case it applies to, changes the reference and is rejected by ``judge`` at the case's bar; every family
    sees every defect that can apply to it."""
    seen = {}
    for c in G.CASES:
        ref = G.reference(c)
        bad, errs = G.judge(c, *ref)
        assert bad == [] and all(e == 0 for e, _ in errs.values()), c.id
        for d, (y, st) in G.mutations(c):
            assert not (torch.equal(y, ref[0]) and torch.equal(st, ref[1])), (c.id, d)
            bad, _ = G.judge(c, y, st)
            assert bad, (c.id, d)
            seen.setdefault(c.family, set()).add(d)
    assert set().union(*seen.values()) == set(G.DEFECTS)
    for name, f in G.FAMILIES.items():
        want = set(G.DEFECTS)
        if not G.has_halo(f):
            want -= {"zero_top", "zero_right", "reflect_as_replicate", "pad_act_s", "pad_act_s_seam", "seam_shift"}
        if f.kind == "s2d" or name == "up9":
            want -= {"zero_top", "zero_right", "reflect_as_replicate", "pad_act_s", "pad_act_s_seam", "ss_image0", "prelu_slope_0"}
        if f.kind != "convT":
            want.discard("convT_last_odd_row")
        if name not in G.NLAST:
            want.discard("nlast_zero")
        assert seen[name] == want, (name, seen[name] ^ want)
    # a NaN is a violation, and so is a wrong shape
    c = G.by_id("tile64-2x3-reflect-plain-dense-c32x96")
    y, st = (t.clone() for t in G.reference(c))
    y[1, 1, 2, 5] = float("nan")
    assert G.judge(c, y, st)[0] and G.judge(c, y[:, :1], st)[0]
