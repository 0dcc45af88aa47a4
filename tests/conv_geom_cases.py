"""Cases of the conv-geometry tests (tests/test_conv_geom_cases_cpu.py, tests/test_gpu_conv_geometry.py): the INPUT side of every
forward conv kernel family -- staging, padding index, zero padding, normalise-on-load, tile seams, ragged tiles, channel slices and
channel counts -- against float64 torch of the operation itself.  tests/conv_epi_cases.py walks the output arithmetic at one
geometry; this module walks the geometry with one output arithmetic (bias and tile statistics; the layout cases add the family's
leaky-ReLU + residual-after where it has one).  Plain torch on the CPU: nothing here touches the device.

A case is (family, extent, pad mode, load mode, layout, channels); its id is built from those fields and its tensors are seeded by
the id of the CONVOLUTION -- everything but the family -- so the families of one bit-identity group (EQUAL) read the same tensors.
The weights are seeded by (kind, Cin, Cout, k) alone: one plan serves every case of those.

  B = 3 everywhere: a dropped image stride shows on two images.
  extents (output H x W; the transposed convs read H x W and write 2 H x 2 W, the stride-2 convs read the (H + 1) x (W + 1) x 4 Cin
  space-to-depth stack):  1 x 1;  1 x 5 and 5 x 1 (every halo row / column is padding);  2 x 3 (the smallest legal reflect:
  -1 -> 1, n -> n - 2);  16 x 16 (exactly one tile);  33 x 35 (3 x 3 tiles of 16 with an interior tile (1, 1) whose halo touches the
  last row, a last tile row one pixel high, a last tile column three wide; 5 tile rows of 8, 2 of 24 and of 32, 3 x 3 blocks of 15).
  Reflect padding of an extent of 1 is undefined (torch refuses it; the kernels clamp, which is no contract): 1 x 1, 1 x 5 and 5 x 1
  run under zero and replicate padding only.
  The Winograd kernel also runs 32 x 32 under zero padding with in_ss: 2 x 2 tiles that all end on the image's edge, none interior.
  load modes: plain, in_ss + PReLU(0.25); at 33 x 35 under zero padding also in_ss alone and in_ss + leaky ReLU.  The (a, s) table
  is per (image, channel), both signs, 0.5 <= |a|, |s| <= 1.5: padding that wrongly received act(s) is an O(1) error.
  layout cases (33 x 35, zero padding): x is channels [32, 32 + C) of a tensor 64 wider, out channels [64, 64 + Cout) of one 96 wider,
  the residual (families with a leaky-ReLU + residual-after combination) a slice with a third pixel stride; the streaming 1x1
  kernel also with in_res.  Slice starts are multiples of 32 elements: the kernels read 16-byte items.
  channel cases (17 x 19, zero padding, plain): Cin of 1 / 2 / 3 / 5 chunks (a_slots 1 / 2 / 3 and a ring that wraps; 1 / 2 / 4 for the
  direct forms, whose step limit ends them there; 2 / 6 chunks of 64 for the 64-channel-step families) and a last N tile of four
  channels (or the smallest Cout over one N tile that the family's divisibility rule takes).

DROPPED lists what a family's matrix leaves out and why.  ``mutations`` returns the reference with one thing a staging routine could
get wrong; tests/test_conv_geom_cases_cpu.py shows ``judge`` rejects each at the case's own bar.
"""
import collections
import functools
import math

import torch
import torch.nn.functional as F

import conv_epi_cases as CE

B = 3
PRELU_SLOPE = CE.PRELU_SLOPE
EXTENTS = ((1, 1), (1, 5), (5, 1), (2, 3), (16, 16), (33, 35))
BIG, CHAN_HW = (33, 35), (17, 19)
PADS = ("zero", "reflect", "replicate")
LOADS = ("plain", "ss_prelu")
EXTRA_LOADS = ("ss", "ss_lrelu")              # 33 x 35 under zero padding only
X_LO, X_EXTRA, OUT_LO, OUT_EXTRA, RES_LO, RES_EXTRA, INRES_LO, INRES_EXTRA = 32, 64, 64, 96, 32, 32, 64, 128
BAR, BAR_STATS, EQUAL, switched = CE.BAR, CE.BAR_STATS, CE.EQUAL, CE.switched

FAMILIES = dict(CE.FAMILIES, row32_bf16x1=CE._fam(
    "conv", 64, 128, 3, {"CONV_VARIANT": {"value": 2}, "TALL_TILE_SINGLE": {"value": True, "min_blocks": 0}},
    dict(variant=7, bn=128, tile_rows=32), 1, torch.float32, ()))

Case = collections.namedtuple("Case", "id family facet hw pad load layout cin cout")

# Cin of the channel cases, in chunks (32 channels; 64 for the 64-channel-step families)
_DIRECT, _K64 = ("stream1", "direct3", "direct5"), ("k64_n256_bf16", "k64_row24_fp16")
# Cout whose last N tile holds four channels -- or, where the family's divisibility rule forbids that, the next Cout it takes
NLAST = {"tile64": 68, "tile_s2d": 68, "convT4": 68, "stream1": 36, "direct3": 36, "direct5": 36, "tile128": 132, "row8": 132, "wino": 132,
         "row32_bf16x1": 132, "n256": 512, "dual": 384, "up9": 64}
WINO_EDGE = "32x32/zero/ss_prelu"
DROPPED = {}            # (family, facet) -> why the family's matrix leaves it out


def cin_chunks(name):
    return (1, 2, 4) if name in _DIRECT else (2, 6) if name in _K64 else (1, 2, 3, 5)


def has_halo(f):
    return f.k == 3 and f.kind != "s2d"


def has_residual(f):
    return ("lrelu", "after") in f.combos


def _refused(name, f, hw, pad, load):
    if pad == "reflect" and min(hw) == 1:
        return "reflect padding of an extent of 1 is undefined (torch refuses it)"
    if name == "up9" and (pad != "zero" or load != "plain"):
        return "the nine-product upscale takes zero padding and no in_ss: the plan falls back to the four-phase form"
    if f.kind == "s2d" and load != "plain":
        return "no network calls the stride-2 conv with in_ss: the blur in front of it applies the table"
    return None


def _case(name, facet, hw, pad, load, layout, cin, cout):
    cid = "%s-%dx%d-%s-%s-%s-c%dx%d" % (name, hw[0], hw[1], pad, load, layout, cin, cout)
    return Case(cid, name, facet, hw, pad, load, layout, cin, cout)


def _build():
    cases = []
    for name, f in FAMILIES.items():
        pads = PADS if has_halo(f) else ("zero",)          # no halo / every tap inside the stack: nothing to pad
        for hw in EXTENTS:
            for pad in pads:
                for load in LOADS + (EXTRA_LOADS if (hw == BIG and pad == "zero") else ()):
                    facet = "%dx%d/%s/%s" % (hw[0], hw[1], pad, load)
                    why = _refused(name, f, hw, pad, load)
                    if why:
                        DROPPED[(name, facet)] = why
                    else:
                        cases.append(_case(name, facet, hw, pad, load, "dense", f.cin, f.cout))
        if name == "wino":      # every tile ends on the image's edge: an ``interior`` test that took ty0 + 16 == in_h would show here
            cases.append(_case(name, WINO_EDGE, (32, 32), "zero", "ss_prelu", "dense", f.cin, f.cout))
        for load in LOADS + (("ss_res",) if name == "stream1" else ()):
            why = _refused(name, f, BIG, "zero", load)
            if why:
                DROPPED[(name, "slices/" + load)] = why
            else:
                cases.append(_case(name, "slices/" + load, BIG, "zero", load, "slices", f.cin, f.cout))
        step = 64 if name in _K64 else 32
        for n in cin_chunks(name):
            cases.append(_case(name, "cin%d" % n, CHAN_HW, "zero", "plain", "dense", n * step, f.cout))
        if name in NLAST:
            cases.append(_case(name, "nlast", CHAN_HW, "zero", "plain", "dense", f.cin, NLAST[name]))
    return cases


CASES = _build()
_BY_ID = {c.id: c for c in CASES}
assert len(_BY_ID) == len(CASES)


def by_id(cid):
    return _BY_ID[cid]


def geometry(c):
    """((input H, W, channels), (output H, W), output pixels per tile position) of a case's launch"""
    f, (h, w) = FAMILIES[c.family], c.hw
    if f.kind == "convT":
        return (h, w, c.cin), (2 * h, 2 * w), 2
    if f.kind == "s2d":
        return (h + 1, w + 1, 4 * c.cin), (h, w), 1
    return (h, w, c.cin), (h, w), 1


def epilogue(c):
    return "lrelu_after" if (c.layout == "slices" and has_residual(FAMILIES[c.family])) else "bias"


def conv_name(c):
    """the id of the convolution a case computes: everything but the family"""
    f = FAMILIES[c.family]
    return "%s%d-%s-%s-%s" % (f.kind, f.k, str(f.dtype).split(".")[-1], epilogue(c), c.id.split("-", 1)[1])


_BY_CONV = {}
for _c in CASES:
    _BY_CONV.setdefault(conv_name(_c), _c)          # (any case of a convolution describes its tensors)


def _seed(name):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) % (1 << 31)


@functools.lru_cache(maxsize=None)
def weight(kind, cin, cout, k):
    g = torch.Generator().manual_seed(_seed("w-%s-%d-%d-%d" % (kind, cin, cout, k)))
    return torch.randn(cout, cin, k, k, generator=g) / math.sqrt(cin * k * k)


def _signed(g, *shape):
    """both signs, magnitudes in [0.5, 1.5]"""
    mag = 0.5 + torch.rand(*shape, generator=g)
    return torch.where(torch.rand(*shape, generator=g) < 0.5, -mag, mag)


Slice = collections.namedtuple("Slice", "wide lo width")       # channels [lo, lo + width) of the NHWC tensor ``wide``


def view(s):
    return s.wide[..., s.lo:s.lo + s.width]


@functools.lru_cache(maxsize=None)
def _make(name):
    c = _BY_CONV[name]
    f = FAMILIES[c.family]
    g = torch.Generator().manual_seed(_seed(name))
    (ih, iw, ic), (oh, ow), _ = geometry(c)
    sl = c.layout == "slices"

    def act(h, w, ch, lo, extra):
        """NHWC tensor in the storage type, rounded once: the values the kernel reads"""
        wide = torch.randn(B, h, w, ch + (extra if sl else 0), generator=g).to(f.dtype)
        return Slice(wide, lo if sl else 0, ch)
    t = {"x": act(ih, iw, ic, X_LO, X_EXTRA), "w": weight(f.kind, c.cin, c.cout, f.k), "bias": torch.randn(c.cout, generator=g)}
    if c.load != "plain":
        t["ss"] = _signed(g, B, ic, 2)
        t["prelu"] = torch.tensor([PRELU_SLOPE])
    if c.load == "ss_res":
        t["in_res"] = act(ih, iw, ic, INRES_LO, INRES_EXTRA)
    if epilogue(c) == "lrelu_after":
        t["res"] = act(oh, ow, c.cout, RES_LO, RES_EXTRA)
    return t


def make(c):
    """CPU tensors of a case, shared by every case of the same convolution: x / res / in_res as Slice (what the kernel reads, in
    the family's storage type), w, bias, and under normalise-on-load ss (B, C, 2) and prelu (1,)"""
    return _make(conv_name(c))


# ---------------------------------------------------------------------------------------------------------------- reference
def _in_act(t, load, slope):
    if load == "ss_lrelu":
        return F.leaky_relu(t, 0.2) * math.sqrt(2.0)
    if load in ("ss_prelu", "ss_res"):
        return torch.where(t >= 0, t, slope * t)
    return t


def _op(f, c, xp, w, padded):
    """the convolution over the already padded NCHW tensor"""
    if f.kind == "convT":
        import ppst_oracle as O
        y = F.conv_transpose2d(xp, O.upscale_weight(w), stride=2, padding=1)
        return y[..., 2:-2, 2:-2] if padded else y
    if f.kind == "s2d":              # channel block py * 2 + px of pixel (Y, X) is pixel (2 Y + py, 2 X + px) of the tensor the conv reads
        b, c4, h, w_ = xp.shape
        full = torch.zeros(b, c.cin, 2 * h, 2 * w_, dtype=xp.dtype)
        for p in range(4):
            full[:, :, p // 2::2, p % 2::2] = xp[:, p * c.cin:(p + 1) * c.cin]
        return F.conv2d(full, w, stride=2)[:, :, :c.hw[0], :c.hw[1]]
    return F.conv2d(xp, w)


_MODE = {"zero": "constant", "reflect": "reflect", "replicate": "replicate"}


def _forward(c, t, dt=torch.float64, defect=None):
    """(output NHWC, statistics (B, Cout, 2)) in ``dt``; ``defect``: one staging error (``mutations``)"""
    f = FAMILIES[c.family]
    (ih, iw, ic), (oh, ow), osy = geometry(c)
    xs = t["x"]
    if defect == "x_slice_start":
        xs = Slice(xs.wide, 0, xs.width)
    x = view(xs).to(dt).permute(0, 3, 1, 2)              # slices are cut before anything else
    w = t["w"].to(dt)
    act_s = None
    if c.load != "plain":
        ss = t["ss"].to(dt)
        if defect == "ss_image0":
            ss = ss.clone()
            ss[1] = ss[0]
        slope = 0.0 if defect == "prelu_slope_0" else PRELU_SLOPE
        a, s = ss[:, :, 0, None, None], ss[:, :, 1, None, None]
        u = a * x + s
        if c.load == "ss_res":
            u = u + view(t["in_res"]).to(dt).permute(0, 3, 1, 2)
        x, act_s = _in_act(u, c.load, slope), _in_act(s, c.load, slope)
    if defect in ("cin_last_dropped", "cin_chunk0_twice"):
        x = x.clone()
        if defect == "cin_last_dropped":
            x[:, -32:] = 0
        else:                                            # chunk 1's activations are chunk 0's
            x[:, 32:64] = x[:, :32]
    halo = has_halo(f)

    def run(xa):
        if not halo:
            return _op(f, c, xa, w, False)
        xp = F.pad(xa, (1, 1, 1, 1), "replicate" if defect == "reflect_as_replicate" else _MODE[c.pad])
        if defect == "zero_top":
            xp[:, :, 0, :] = 0
        elif defect == "zero_right":
            xp[:, :, :, -1] = 0
        elif defect in ("pad_act_s", "pad_act_s_seam"):
            # seam: only the padding in the halo of the four tiles next to the interior tile (1, 1) -- rows / columns 16 .. 31 --
            # as an ``interior`` test off by one would give
            m = torch.zeros(ih + 2, iw + 2, dtype=torch.bool)
            if defect == "pad_act_s":
                m[0], m[-1], m[:, 0], m[:, -1] = True, True, True, True
            else:
                m[0, 17:33], m[-1, 17:33], m[17:33, 0], m[17:33, -1] = True, True, True, True
            xp = torch.where(m, act_s.expand_as(xp), xp)
        return _op(f, c, xp, w, True)
    y = run(x)
    if defect == "seam_shift":                           # the halo row of tile row 1 taken from row 16 instead of 15
        x2 = x.clone()
        x2[:, :, 15] = x[:, :, 16]
        y[:, :, 16 * osy:17 * osy] = run(x2)[:, :, 16 * osy:17 * osy]
    y = (y + t["bias"].to(dt)[:, None, None]).permute(0, 2, 3, 1)
    if epilogue(c) == "lrelu_after":
        y = F.leaky_relu(y, 0.2) * math.sqrt(2.0) + view(t["res"]).to(dt)
    y = y.contiguous()
    if defect == "last_tile_row":
        y[:, 32 * osy:] = 0
    elif defect == "last_tile_col":
        y[:, :, 32 * osy:] = 0
    elif defect == "nlast_zero":
        y[..., -4:] = 0
    elif defect == "convT_last_odd_row":
        y[:, -1] = 0
    ys = y[:, :32 * osy, :32 * osy] if defect == "stats_miss_ragged" else y
    return y, torch.stack([ys.sum((1, 2)), (ys * ys).sum((1, 2))], -1)


@functools.lru_cache(maxsize=None)
def _reference(name):
    return _forward(_BY_CONV[name], _make(name))


def reference(c):
    """float64: (output NHWC, statistics (B, Cout, 2) = sum and sum of squares over the pixels); one evaluation per convolution"""
    return _reference(conv_name(c))


def err32(c):
    """error of the float32 evaluation of the reference against the float64 one, relative to max |ref|: (output, sums, sums of squares)"""
    (y64, s64), (y32, s32) = reference(c), _forward(c, make(c), torch.float32)
    rel = lambda a, b: ((a.double() - b).abs().max() / b.abs().max()).item()
    return rel(y32, y64), rel(s32[..., 0], s64[..., 0]), rel(s32[..., 1], s64[..., 1])


# ---------------------------------------------------------------------------------------------------------------- judge
def edge_mask(oh, ow, osy):
    """border rows and columns, and the rows / columns on both sides of the tile seams 15|16 and 31|32 (of tile positions)"""
    m = torch.zeros(oh, ow, dtype=torch.bool)
    m[0], m[-1], m[:, 0], m[:, -1] = True, True, True, True
    for s in (16, 32):
        for i in range((s - 1) * osy, (s + 1) * osy):
            if i < oh:
                m[i] = True
            if i < ow:
                m[:, i] = True
    return m


def judge(c, y, stats, ref=None):
    """-> (violations, {what: (error, bar)}) of an output NHWC and per-(image, channel) sums (B, Cout, 2) against float64 at the
    case's bar: the whole output against max |ref|, the border and seam rows / columns again against their own max |ref|, the sums
    and sums of squares against theirs.  No element is left out."""
    f = FAMILIES[c.family]
    ref_y, ref_s = ref if ref is not None else reference(c)
    _, (oh, ow), osy = geometry(c)
    bad, errs = [], {}
    if tuple(y.shape) != tuple(ref_y.shape) or tuple(stats.shape) != tuple(ref_s.shape):
        return ["shape %s / %s" % (tuple(y.shape), tuple(stats.shape))], errs

    def one(what, got, want, bar):
        e = ((got.double() - want).abs().max() / want.abs().max()).item()
        errs[what] = (e, bar)
        if not e <= bar:                                 # (a NaN is a violation)
            bad.append("%s: %.3e > %.0e" % (what, e, bar))
    one("output", y, ref_y, BAR[f.precision])
    m = edge_mask(oh, ow, osy)
    one("border", y[:, m], ref_y[:, m], BAR[f.precision])
    one("sum", stats[..., 0], ref_s[..., 0], BAR_STATS[f.precision])
    one("sumsq", stats[..., 1], ref_s[..., 1], BAR_STATS[f.precision])
    return bad, errs


# ---------------------------------------------------------------------------------------------------------------- seeded defects
DEFECTS = ("zero_top", "zero_right", "reflect_as_replicate", "pad_act_s", "pad_act_s_seam", "ss_image0", "prelu_slope_0", "seam_shift",
           "last_tile_row", "last_tile_col", "stats_miss_ragged", "x_slice_start", "cin_last_dropped", "cin_chunk0_twice", "nlast_zero",
           "convT_last_odd_row")


def defects_of(c):
    """the defects that can apply to a case (each changes the reference: asserted by the CPU test)"""
    f = FAMILIES[c.family]
    halo, big, matrix = has_halo(f), c.hw == BIG, "/" in c.facet and c.layout == "dense"
    out = []
    if matrix and halo and c.pad != "zero":
        out += ["zero_top", "zero_right"]
    if matrix and halo and c.pad == "reflect":
        out.append("reflect_as_replicate")
    if matrix and halo and c.pad == "zero" and c.load != "plain":
        out.append("pad_act_s")
        if big:
            out.append("pad_act_s_seam")
    if matrix and c.load != "plain":
        out.append("ss_image0")
    if matrix and c.load == "ss_prelu":
        out.append("prelu_slope_0")
    if matrix and big:
        out += ["last_tile_row", "last_tile_col", "stats_miss_ragged"] + (["seam_shift"] if halo else [])
    if c.layout == "slices":
        out.append("x_slice_start")
    if c.facet.startswith("cin"):
        out.append("cin_last_dropped")
        if c.cin >= 64:
            out.append("cin_chunk0_twice")
    if c.facet == "nlast":
        out.append("nlast_zero")
    if matrix and f.kind == "convT":
        out.append("convT_last_odd_row")
    return out


def mutations(c):
    """[(defect, (output, statistics))]: the float64 reference with one thing a staging routine could get wrong"""
    return [(d, _forward(c, make(c), defect=d)) for d in defects_of(c)]


# ---------------------------------------------------------------------------------------------------------------- the launch
PAD_NAME = {"zero": "PAD_ZERO", "reflect": "PAD_REFLECT", "replicate": "PAD_REPLICATE"}
IN_ACT_NAME = {"plain": "ACT_NONE", "ss": "ACT_NONE", "ss_lrelu": "ACT_LRELU", "ss_prelu": "ACT_PRELU", "ss_res": "ACT_PRELU"}


def plan_of(ops, c, w):
    f = FAMILIES[c.family]
    return ops.ConvPlan(w, kind=f.kind, precision=f.precision)


def call(ops, c, t, plan=None):
    """run a case: ``t`` holds x, w, bias, out (the caller's, shaped like the output) and, where the case has them, ss, prelu, in_res,
    res -- device tensors or views -> (out, statistics (B, tiles, Cout, 2))"""
    f = FAMILIES[c.family]
    with switched(ops, f.switches):
        plan = plan or plan_of(ops, c, t["w"])
        kw = dict(bias=t["bias"], stats=True, out=t["out"], pad_mode=getattr(ops, PAD_NAME[c.pad]))
        if f.kind == "s2d":
            kw["out_hw"] = c.hw
        if c.load != "plain":
            kw.update(in_ss=t["ss"], in_act=getattr(ops, IN_ACT_NAME[c.load]))
            if IN_ACT_NAME[c.load] == "ACT_PRELU":
                kw["in_prelu"] = t["prelu"]
        if c.load == "ss_res":
            kw["in_res"] = t["in_res"]
        if epilogue(c) == "lrelu_after":
            kw.update(act=ops.ACT_LRELU, residual=t["res"], res_after_act=True)
        return plan(t["x"], **kw)
