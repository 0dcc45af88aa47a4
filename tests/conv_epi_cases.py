"""Cases of the conv-epilogue tests (tests/test_conv_epi_cases_cpu.py, tests/test_gpu_conv_epilogue.py, tests/conv_epi_record.py):
every forward conv kernel family x every (activation, residual mode) of the output arithmetic

    ((acc + bias) + noise_weight * noise) [+ res] -> lrelu * sqrt 2 | prelu -> [+ res] -> * out_scale        (csrc/conv_common.h)

with bias, noise (weight 0.3), out_scale 0.7 and tile statistics, plus one run per family with none of them.  Plain torch on the CPU:
nothing here touches the device.  Inputs come from a CPU generator seeded by the family's ``data`` name, so families that run the
same convolution (the bit-identity groups of EQUAL) read the same tensors.

Shapes: B = 2, 17 x 19 outputs -- ragged 16 x 16 tiles in both directions, four tiles per image; the transposed convs read 9 x 10
and write 18 x 20.  Cin = 32 (one chunk), 64 for the N-256, Winograd and 64-channel-step kernels.  Cout = 96 where the family's N tile
is 64 wide (tile kernel, streaming 1x1, both direct forms: a ragged second tile); the tile kernel's 128-wide N tile gets its ragged
tile from Cout = 160 (a plan takes that tile from Cout >= 128 on, so 96 cannot reach it); 128 for Winograd, the phase pairs, the
nine-product upscale and the 24-row tile; 256 for the N-256 kernel and the two tile-kernel forms it is bit-identical to.

A family names the ops switches that force its kernel and the launch it must end in (``expect``: fields of ppst_conv_args);
tests/test_conv_epi_cases_cpu.py runs every case through ops.ConvPlan without a device and compares.
"""
import collections
import contextlib
import functools
import math

import torch
import torch.nn.functional as F

B, OUT_HW, CONVT_IN_HW = 2, (17, 19), (9, 10)
NOISE_WEIGHT, OUT_SCALE, PRELU_SLOPE = 0.3, 0.7, 0.25
ACTS = ("none", "lrelu", "prelu")
RESS = ("none", "before", "after")
NINE = tuple((a, r) for a in ACTS for r in RESS)

Family = collections.namedtuple("Family", "kind cin cout k precision dtype switches expect combos")
Case = collections.namedtuple("Case", "id family act res full")

_OFF = {"value": False}
_NO_WINO = {"WINO": _OFF}
_BIG = 1 << 30


def _fam(kind, cin, cout, k, switches, expect, precision=0, dtype=torch.float32, combos=NINE):
    e = dict(entry="ppst_conv2d_mfma", dual_b=0, k64=0, io_st={torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}[dtype], tile_rows=16)
    e.update(expect)
    return Family(kind, cin, cout, k, precision, dtype, switches, e, combos)


FAMILIES = {
    # ---- conv_mfma.hip: the 64 x 64 wave-tile kernel (variant 0)
    "tile64": _fam("conv", 32, 96, 3, {"CONV_VARIANT": {"value": 0}}, dict(variant=0, bn=64)),
    "tile128": _fam("conv", 32, 160, 3, {"CONV_VARIANT": {"value": 0}, **_NO_WINO}, dict(variant=0, bn=128)),
    "tile256": _fam("conv", 64, 256, 3, {"CONV_VARIANT": {"value": 0}, **_NO_WINO}, dict(variant=0, bn=128)),
    "row8": _fam("conv", 64, 256, 3, {"CONV_VARIANT": {"value": 2}, "FAT_MIN_BLOCKS": _BIG, "TWO_BLOCK_8ROW": {"value": True, "min_blocks": 0},
                                      **_NO_WINO}, dict(variant=0, bn=128, tile_rows=8)),
    "tile1x1": _fam("conv", 32, 96, 1, {"STREAM_1X1": _OFF}, dict(variant=0, bn=64, halo=0)),
    "tile_s2d": _fam("s2d", 32, 96, 3, {"CONV_VARIANT": {"value": 0}}, dict(variant=0, bn=64)),
    "convT4": _fam("convT", 32, 96, 3, {"CONV_VARIANT": {"value": 0}}, dict(variant=0, bn=64, n_groups=4)),
    # ---- conv_mfma2.hip: N-256, phase pairs, nine products (no residual, no PReLU: its entry check)
    "n256": _fam("conv", 64, 256, 3, {"CONV_VARIANT": {"value": 2}, "FAT_MIN_BLOCKS": 0, **_NO_WINO}, dict(variant=2, bn=256)),
    "dual": _fam("convT", 32, 128, 3, {"CONV_VARIANT": {"value": 2}, "DUAL_CONVT": {"value": True, "min_blocks": 0}, "UP9": _OFF},
                 dict(variant=2, bn=256, dual_b=1, n_groups=2)),
    "up9": _fam("convT", 32, 128, 3, {"UP9": {"value": True, "min_blocks": 0, "min_fill": 0.0}},
                dict(variant=11, bn=256, tile_rows=15, n_groups=1), combos=(("none", "none"), ("lrelu", "none"))),
    # ---- conv1x1.hip: streaming 1x1 (4), direct (5), direct 3x3 (6)
    "stream1": _fam("conv", 32, 96, 1, {"STREAM_1X1": {"value": True}}, dict(variant=4, bn=64)),
    "direct5": _fam("s2d", 32, 96, 3, {"DIRECT_MAX": {"cout": 96}}, dict(variant=5, bn=64)),
    "direct3": _fam("conv", 32, 96, 3, {"DIRECT_MAX": {"cout": 96}}, dict(variant=6, bn=64)),
    # ---- conv_wino.hip
    "wino": _fam("conv", 64, 128, 3, {"WINO": {"value": True, "min_blocks": 1}}, dict(variant=10, bn=128)),
    # ---- half storage in the single-pass modes: the run-time (EpiR) instance of the arithmetic
    "tile_bf16": _fam("conv", 32, 96, 3, {"CONV_VARIANT": {"value": 0}}, dict(variant=0, bn=64), 1, torch.bfloat16, (("prelu", "before"),)),
    "tile_fp16": _fam("conv", 32, 96, 3, {"CONV_VARIANT": {"value": 0}}, dict(variant=0, bn=64), 3, torch.float16, (("lrelu", "after"),)),
    "k64_n256_bf16": _fam("conv", 64, 256, 3, {"CONV_VARIANT": {"value": 2}, "FAT_MIN_BLOCKS": 0, "K64": {"value": True}},
                          dict(variant=2, bn=256, k64=1), 1, torch.bfloat16, (("lrelu", "after"),)),
    "k64_row24_fp16": _fam("conv", 64, 128, 3, {"CONV_VARIANT": {"value": 2}, "K64": {"value": True},
                                                "TALL_TILE_SINGLE": {"value": True, "min_blocks": 0}},
                           dict(variant=9, bn=128, tile_rows=24, k64=1), 3, torch.float16, (("prelu", "before"),)),
    # ---- conv_f32.hip
    "f32": _fam("conv", 32, 96, 3, {}, dict(entry="ppst_conv2d_f32"), 2, torch.float32, (("lrelu", "after"),)),
}
# the fp32-class families walk all nine combinations (the nine-product upscale: the two its entry check takes)
FULL_FAMILIES = tuple(n for n, f in FAMILIES.items() if f.precision == 0)
# outputs equal to the bit (tests/gpu_diag.py t_conv_variants, t_conv1x1_stream): same MFMA sequence per output element
EQUAL = (("tile256", "n256", "row8"), ("tile64", "direct3"), ("tile1x1", "stream1"), ("tile_s2d", "direct5"))
# bars against float64 torch, relative to the largest |reference| (tests/gpu_diag.py t_conv): per precision mode
BAR = {0: 3e-5, 1: 2e-2, 3: 3e-3, 2: 5e-6}
# the statistics' sums: t_conv's bar where the outputs are fp32-class; in the single-pass modes a sum of outputs that are each within
# the mode's bar of the largest output is within that bar of the largest sum
BAR_STATS = {0: 1e-5, 2: 1e-5, 1: BAR[1], 3: BAR[3]}

CASES = []
for _n, _f in FAMILIES.items():
    for _a, _r in _f.combos:
        CASES.append(Case("%s-%s-res_%s" % (_n, _a, _r), _n, _a, _r, True))
    CASES.append(Case("%s-plain" % _n, _n, "none", "none", False))
_BY_ID = {c.id: c for c in CASES}
assert len(_BY_ID) == len(CASES)


def by_id(cid):
    return _BY_ID[cid]


def data_name(f):
    return "%s-%d-%d-%d-%s" % (f.kind, f.cin, f.cout, f.k, str(f.dtype).split(".")[-1])


def geometry(f):
    """((input H, W, channels), (output H, W)) of a family's launch"""
    if f.kind == "convT":
        return CONVT_IN_HW + (f.cin,), (2 * CONVT_IN_HW[0], 2 * CONVT_IN_HW[1])
    if f.kind == "s2d":                  # the space-to-depth copy of the (2 H + 2) x (2 W + 2) blurred tensor
        return (OUT_HW[0] + 1, OUT_HW[1] + 1, 4 * f.cin), OUT_HW
    return OUT_HW + (f.cin,), OUT_HW


@functools.lru_cache(maxsize=None)
def _inputs(name):
    f = next(f for f in FAMILIES.values() if data_name(f) == name)
    g = torch.Generator().manual_seed(sum(ord(ch) * (i + 1) for i, ch in enumerate(name)))
    rnd = lambda *s: torch.randn(*s, generator=g)
    (ih, iw, ic), (oh, ow) = geometry(f)
    return {"x": rnd(B, ih, iw, ic).to(f.dtype), "w": rnd(f.cout, f.cin, f.k, f.k) / math.sqrt(f.cin * f.k * f.k), "bias": rnd(f.cout),
            "noise": rnd(B, 1, oh, ow), "res": rnd(B, oh, ow, f.cout).to(f.dtype), "prelu": torch.tensor([PRELU_SLOPE])}


def inputs(case):
    """CPU tensors of a case (shared by every case of the same convolution): x, res NHWC in the family's storage type"""
    return _inputs(data_name(FAMILIES[case.family]))


@functools.lru_cache(maxsize=None)
def _conv64(name):
    import ppst_oracle as O
    f = next(f for f in FAMILIES.values() if data_name(f) == name)
    t = _inputs(name)
    x, w = t["x"].double().permute(0, 3, 1, 2), t["w"].double()
    if f.kind == "convT":
        y = F.conv_transpose2d(x, O.upscale_weight(w), stride=2, padding=1)
    elif f.kind == "s2d":                # channel block py * 2 + px of pixel (Y, X) is pixel (2 Y + py, 2 X + px) of the tensor the conv reads
        b, c4, h, w_ = x.shape
        full = torch.zeros(b, f.cin, 2 * h, 2 * w_, dtype=torch.float64)
        for p in range(4):
            full[:, :, p // 2::2, p % 2::2] = x[:, p * f.cin:(p + 1) * f.cin]
        y = F.conv2d(full, w, stride=2)[:, :, :OUT_HW[0], :OUT_HW[1]]
    else:
        y = F.conv2d(x, w, padding=f.k // 2)
    return y.permute(0, 2, 3, 1).contiguous()


def reference(case):
    """float64: (output NHWC, statistics (B, Cout, 2) = sum and sum of squares over the pixels, or None)"""
    f = FAMILIES[case.family]
    t, y = inputs(case), _conv64(data_name(f))
    if not case.full:
        return y, None
    y = (y + t["bias"].double()) + NOISE_WEIGHT * t["noise"].double().permute(0, 2, 3, 1)
    res = t["res"].double()
    if case.res == "before":
        y = y + res
    if case.act == "lrelu":
        y = F.leaky_relu(y, 0.2) * math.sqrt(2.0)
    elif case.act == "prelu":
        y = torch.where(y >= 0, y, PRELU_SLOPE * y)
    if case.res == "after":
        y = y + res
    y = y * OUT_SCALE
    return y, torch.stack([y.sum((1, 2)), (y * y).sum((1, 2))], -1)


@contextlib.contextmanager
def switched(ops, switches):
    """the ops switches of a family (dicts are updated, FAT_MIN_BLOCKS is set), put back afterwards"""
    saved = {n: (dict(getattr(ops, n)) if isinstance(getattr(ops, n), dict) else getattr(ops, n)) for n in switches}
    try:
        for n, v in switches.items():
            if isinstance(v, dict):
                getattr(ops, n).update(v)
            else:
                setattr(ops, n, v)
        yield
    finally:
        for n, v in saved.items():
            if isinstance(v, dict):
                getattr(ops, n).clear()
                getattr(ops, n).update(v)
            else:
                setattr(ops, n, v)


def call(ops, case, t):
    """run a case on the tensors ``t`` (those of ``inputs``, moved to the device; ``out`` if the caller owns the output):
    -> (y, stats), stats None for the plain run"""
    f = FAMILIES[case.family]
    with switched(ops, f.switches):
        plan = ops.ConvPlan(t["w"], kind=f.kind, precision=f.precision)
        kw = {"out_hw": OUT_HW} if f.kind == "s2d" else {}
        if "out" in t:
            kw["out"] = t["out"]
        if not case.full:
            return plan(t["x"], **kw), None
        kw.update(bias=t["bias"], noise=t["noise"], noise_weight=NOISE_WEIGHT, out_scale=OUT_SCALE, stats=True,
                  act={"none": ops.ACT_NONE, "lrelu": ops.ACT_LRELU, "prelu": ops.ACT_PRELU}[case.act])
        if case.act == "prelu":
            kw["prelu"] = t["prelu"]
        if case.res != "none":
            kw.update(residual=t["res"], res_after_act=case.res == "after")
        return plan(t["x"], **kw)
