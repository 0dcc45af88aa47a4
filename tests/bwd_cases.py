"""Cases, float64 references, seeded defects and bars of the backward-kernel tests (tests/test_backward_cases_cpu.py,
tests/test_gpu_backward_kernels.py).  Plain torch / numpy on the CPU: nothing here touches the device, and the device is never
its own judge.

A case is a ``Case(op, id, p, seed)``; ``p`` holds the shapes and the layout facts the launcher branches on (``<operand>_ld`` /
``<operand>_off``: the operand is the channel slice [off, off + C) of a tensor ld channels wide; ``acc``: the kernel adds into a
given buffer).  Per op (``OPS[op]``):
  make(c)            -> dict of float32 CPU tensors: the operands AS STORED (the wide tensor where the operand is a slice)
  ref(c, inp, dt)    -> dict of outputs, evaluated in dtype dt (float64: the judge; float32: the measure of the bar)
  branch(c)          -> the kernel family the host launcher picks for the case, restated from its ``if`` (csrc/train.hip,
                        csrc/train_g.hip): this is what stands in for observing which kernel ran
  mutations(c, inp)  -> [(name, outputs)]: the reference with one defect a kernel could have (a dropped border row, a tie sent
                        to the last pixel, a ragged tail dropped, the slice offset ignored, accumulate overwriting, the scalar
                        tail channels zero, batch rows 17.. zero); the CPU test shows that ``compare`` at the case's bar rejects
                        every one of them on the case's own inputs
  cls                -> the project's bar of the kernel class (tests/test_gpu_parity.py, gstep_diag.t_blocks)

Bar of a case (``bar``): max(class bar, 4 x the error of the float32 evaluation of the same reference against float64 on the
case's inputs).  The factor 4 allows a different summation order, not a different formula.  Data movement has bar 0 (bit equal).
``compare`` applies it twice: max|a - b| <= bar max|ref|, and element-wise |a - b| <= bar max|ref| + bar |ref|.  ``judge`` is what
both test files call: ``compare`` on the whole output and, for the spatial gradients (bilinear_bwd, pad2d, avgpool_bwd), once more
on the border rows and columns alone with THEIR max|ref| as the scale, so that a border cannot hide under a larger interior.

Decisions (arg-max, gates, ReLU) are taken from the float32 operands handed to the kernel, never from a rounded intermediate;
tie inputs are quantised so that the products m * x are exact and tie exactly; gate inputs keep |value| >= 1e-3.  No element is
left out of any comparison.

Storage (the convention tests/act_cases.py shares): ``st`` in a case's p names the storage type of the operands its launcher types
(``TYPED``: f32 -- the default --, f16, bf16); every other operand, every statistic and every parameter gradient is float32.
``make`` returns float32 tensors that hold exactly the stored values (rounded once), and whatever derives from a stored operand
(the forward maximum, mean / rstd, the ties) is computed after the rounding: the float64 reference reads what the kernel reads.
``OUT_ST`` names the half-stored outputs; one is judged element by element with the allowed error b s + 2^-p (|ref| + b s): one
round to nearest (p = 11 fp16, 8 bf16) of a value within the case's bar b of the reference, s = max|ref|.  An fp32 output of a half
case keeps the bar of the text above, data movement stays bit equal to the stored values.  The half launchers take the four-channel
forms only; ``same_form_as_f32`` says whether the fp32 launch of the same (widened) operands takes the same kernel form -- where it
does the GPU test also asks for bit equality with that launch, rounded once.  ``mutations`` adds to a half case the defects only a
half kernel can have: a half output stored by truncation, the operands read as the other half type.
"""
import collections
import functools
import zlib

import numpy as np
import torch
import torch.nn.functional as F

BAR_MOVE, BAR_EW, BAR_SUM = 0.0, 2e-6, 1e-5     # data movement / fp32 elementwise, resize, pooling, sums / sums of >= 4096 terms


def _sum_bar(terms):
    return BAR_SUM if terms >= 4096 else BAR_EW

HALF = {"f16": torch.float16, "bf16": torch.bfloat16}
PBITS = {"f16": 11, "bf16": 8}
DTYPE = dict(HALF, f32=torch.float32)
# op -> the operands its launcher types (stored as the case's ``st``; on the device they travel as HALF[st])
TYPED = {"bilinear_bwd": ("dy", "x"), "pad2d": ("x", "dy"), "gap_gmp_bwd": ("x", "out0"), "gap_gmp_multi_bwd": ("x", "out0"), "colsum": ("x",),
         "noise_wgrad": ("dpre",), "wgrad_small_cin": ("dy",), "in_bwd": ("g", "y", "gate"), "space_to_depth": ("x",), "conv_dgrad": ("g",)}
# op -> the outputs that take the storage type of the case (every sum and parameter gradient stays float32)
OUT_ST = {"bilinear_bwd": ("dx",), "pad2d": ("y", "dx"), "gap_gmp_bwd": ("dx",), "gap_gmp_multi_bwd": ("dx",), "in_bwd": ("dx",),
          "space_to_depth": ("s", "back")}
# (conv_dgrad's dx is bf16-stored as well, but the bar the conv tests hold precision mode 1 to already covers that rounding: plain ``compare``)

Case = collections.namedtuple("Case", "op id p seed")
Spec = collections.namedtuple("Spec", "make ref branch mutations cls")
OPS = {}
SCALES = {}      # op -> fn(c, inp) -> {output: the size errors are measured against}; default: max|ref| of the output
CASES = []


def _case(op, cid, seed=0, **p):
    CASES.append(Case(op, "%s-%s" % (op, cid), p, seed))


def _gen(c):
    return torch.Generator().manual_seed(zlib.crc32(c.id.encode()) + c.seed)       # (from the id: adding a case moves no other case's inputs)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float32)


def st_of(c):
    return c.p.get("st", "f32")


def _store(t, st):
    """the float32 tensor holding what a tensor of storage type st holds (one round to nearest)"""
    return t if st == "f32" else t.to(HALF[st]).float()


def out_st(c, name):
    return st_of(c) if name in OUT_ST.get(c.op, ()) else "f32"


def _away(t, lo=1e-3):
    """push values off a decision boundary at 0: |t| >= lo (sign kept; half-stored operands: lo = 2^-9, which every type holds)"""
    return torch.where(t.abs() < lo, torch.where(t < 0, -lo, lo).to(t.dtype), t)


def _sl(c, inp, name, C=None, off=None):
    """the logical operand: channels [off, off + C) of the stored tensor"""
    C = c.p["C"] if C is None else C
    off = c.p.get(name + "_off", 0) if off is None else off
    return inp[name][..., off:off + C]


def _wide(c, g, name, *lead, C=None):
    C = c.p["C"] if C is None else C
    return _randn(g, *lead, c.p.get(name + "_ld", C))


def _vec_ok(c, C, *names):
    """the launchers' common test for the four-channel forms: C, every ld and every slice start multiples of 4 (a slice start
    that is no multiple of 4 floats leaves the pointer off the 16-byte grid)"""
    return C % 4 == 0 and all(c.p.get(n + "_ld", C) % 4 == 0 and c.p.get(n + "_off", 0) % 4 == 0 for n in names)


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _zero_tail(out, n):
    o = out.clone()
    if n:
        o[..., -n:] = 0
    return o


def scale_of(c, out_name):
    if c.op in SCALES:
        return SCALES[c.op](c, inputs(c.id))[out_name]
    return float(np.abs(reference(c.id)[out_name]).max())


def compare(ref, got, bar, scale=None):
    """-> (violations, err): err = max|got - ref| / scale (default max|ref|).  bar 0: bit equality with the float32 rounding of ref."""
    ref = np.asarray(ref, np.float64)
    got = np.asarray(got, np.float64)
    assert ref.shape == got.shape, (ref.shape, got.shape)
    out = []
    if not np.isfinite(got).all():
        return ["%d non-finite values" % (~np.isfinite(got)).sum()], float("inf")
    scale = np.abs(ref).max() if scale is None else scale
    d = np.abs(got - ref)
    err = float(d.max() / scale) if scale > 0 else float(d.max())
    if bar == 0:
        bad = got != ref.astype(np.float32).astype(np.float64)
        if bad.any():
            out.append("%d values differ (data movement: bit equality)" % bad.sum())
        return out, err
    if d.max() > bar * scale:
        out.append("max|a - b| / max|ref| = %.3e > %.1e" % (err, bar))
    far = d > bar * scale + bar * np.abs(ref)
    if far.any():
        out.append("%d values outside bar * (max|ref| + |ref|)" % far.sum())
    return out, err


def half_allowed(ref, b, s, st):
    """the error a half-stored output may carry: one round to nearest of a value within b s of ref"""
    return b * s + 2.0 ** -PBITS[st] * (np.abs(ref) + b * s)


def compare_half(ref, got, b, st, scale=None):
    """-> (violations, err): ``compare`` for an output stored in st; err in units of the allowed error (<= 1 passes)"""
    ref, got = np.asarray(ref, np.float64), np.asarray(got, np.float64)
    assert ref.shape == got.shape, (ref.shape, got.shape)
    if not np.isfinite(got).all():
        return ["%d non-finite values" % (~np.isfinite(got)).sum()], float("inf")
    s = np.abs(ref).max() if scale is None else scale
    d, lim = np.abs(got - ref), half_allowed(ref, b, s, st)
    ratio = np.where(d > 0, d / np.where(lim > 0, lim, 1e-300), 0.0)       # (an all-zero reference allows nothing but zeros)
    bad = ratio > 1.0
    return (["%d values outside b s + 2^-%d (|ref| + b s), worst %.2f x" % (bad.sum(), PBITS[st], ratio.max())] if bad.any() else []), float(ratio.max())


def as_stored(c, name, arr):
    """a float64 result as the output tensor would hold it: rounded once to the output's storage type"""
    return torch.from_numpy(np.asarray(arr, np.float64)).to(DTYPE[out_st(c, name)]).double().numpy()


BORDER_OPS = ("bilinear_bwd", "pad2d", "avgpool_bwd")


def judge(c, out_name, got):
    """-> (violations, err) of one output of a case against its float64 reference, at the case's bar.  A half-stored output: the
    half rule (err in units of the allowed error); data movement: bit equality; the rest: ``compare``."""
    ref, b, st = reference(c.id)[out_name], bar(c, out_name), out_st(c, out_name)
    got = np.asarray(got, np.float64)
    if b == 0 or st == "f32":
        cmp_ = lambda r, g, s=None: compare(r, g, b, s)
    else:
        cmp_ = lambda r, g, s=None: compare_half(r, g, b, st, s)
    bad, err = cmp_(ref, got, scale_of(c, out_name))
    if c.op in BORDER_OPS and ref.ndim == 4:
        edge = np.zeros(ref.shape[1:3], bool)
        edge[[0, -1], :] = True
        edge[:, [0, -1]] = True
        bad2, err2 = cmp_(ref[:, edge], got[:, edge])
        bad += ["border: " + m for m in bad2]
        err = max(err, err2)
    return bad, err


@functools.lru_cache(maxsize=None)
def inputs(c_id):
    c = by_id(c_id)
    return OPS[c.op].make(c)


@functools.lru_cache(maxsize=None)
def reference(c_id):
    c = by_id(c_id)
    with torch.enable_grad():
        r = OPS[c.op].ref(c, inputs(c_id), torch.float64)
    return {k: v.detach().numpy() for k, v in r.items()}


@functools.lru_cache(maxsize=None)
def err32(c_id):
    """per output: error of the float32 evaluation of the reference against float64, relative to max|ref|"""
    c = by_id(c_id)
    with torch.enable_grad():
        r32 = OPS[c.op].ref(c, inputs(c_id), torch.float32)
    r64 = reference(c_id)
    out = {}
    for k, v in r64.items():
        s = scale_of(c, k)
        out[k] = float(np.abs(r32[k].detach().double().numpy() - v).max() / (s if s > 0 else 1.0))
    return out


def bar(c, out_name):
    cls = OPS[c.op].cls(c, out_name) if callable(OPS[c.op].cls) else OPS[c.op].cls
    if cls == 0:
        return 0.0
    return max(cls, 4.0 * err32(c.id)[out_name])


def by_id(cid):
    return _BY_ID[cid]


def branch_of(c):
    return OPS[c.op].branch(c)


def truncated(arr, st):
    """float64 values stored in st by truncation (round toward zero) instead of round to nearest"""
    t = np.asarray(arr, np.float64).astype(np.float32)
    if st == "bf16":
        return (t.view(np.uint32) & np.uint32(0xffff0000)).view(np.float32).astype(np.float64)
    h = t.astype(np.float16)
    over = np.abs(h.astype(np.float32)) > np.abs(t)           # rounded away from zero: one step back
    bits = h.view(np.uint16).copy()
    bits[over] -= 1
    return bits.view(np.float16).astype(np.float64)


def as_other_half(t, st):
    """the stored values of t, their 16 bits read as the other half type"""
    other = torch.bfloat16 if st == "f16" else torch.float16
    return t.to(HALF[st]).view(torch.int16).view(other).float()


def _half_mutations(c, inp):
    """the defects only a half kernel can have, on top of the op's own: a half output stored by truncation (every half-stored
    output that is computed, not copied) and the typed operands read as the other half type (where the kernel computes with them:
    a copy moves the same bits whatever it calls them)"""
    st, out = st_of(c), []
    ref = reference(c.id)
    cut = {k: torch.from_numpy(truncated(v, st)) for k, v in ref.items() if out_st(c, k) != "f32" and bar(c, k) != 0}
    # (an output whose every value the type holds exactly -- the x8 reduction's 0.25 dy -- is stored alike by either rounding: no defect)
    cut = {k: v for k, v in cut.items() if not np.array_equal(v.numpy(), as_stored(c, k, ref[k]))}
    if cut:
        out.append(("half output stored by truncation", cut))
    computes = any(bar(c, k) != 0 for k in ref)
    if computes and c.op not in ("gap_gmp_bwd", "gap_gmp_multi_bwd"):        # (those seed it themselves: the match with the forward's maximum)
        i2 = dict(inp)
        for k in TYPED[c.op]:
            if k in inp and k != "out0" and not (c.op == "bilinear_bwd" and k == "x"):
                i2[k] = as_other_half(inp[k], st)
        r = OPS[c.op].ref(c, i2, torch.float64)
        out.append(("operands read as the other half type", {k: v for k, v in r.items() if bar(c, k) != 0}))
    return out


def mutations(c):
    with torch.enable_grad():
        inp = inputs(c.id)
        muts = list(OPS[c.op].mutations(c, inp))
        if st_of(c) != "f32":
            muts += _half_mutations(c, inp)
        return [(n, {k: v.detach().numpy() for k, v in o.items()}) for n, o in muts]


def as_f32(c):
    """the fp32 twin of a half case: the same operands (the stored values, widened), fp32 storage"""
    return c._replace(p=dict(c.p, st="f32"))


def same_form_as_f32(c):
    """does the fp32 launch on the widened operands take the kernel form of the half launch?  The half launchers take the
    four-channel forms only, and every half case's shapes send fp32 there too -- but for noise_wgrad, whose fp32 launcher keeps the
    scalar kernel where C / 4 < 256 does not divide 256, and ops.dgrad_s2d, whose stack form needs cin % 8 of a half gradient (and
    the convs round their operands inside the kernel: their storage forms are compared by the conv tests, not here)."""
    assert st_of(c) != "f32"
    if c.op == "conv_dgrad":
        return False
    twin = branch_of(as_f32(c))
    if c.op == "noise_wgrad":
        return twin == "noise_wgrad:four"
    assert not any(w in twin for w in ("scalar", "scatter", "float:", ":4e")), (c.id, twin)
    return True


def _fam(name, c):
    """the family name of a launcher's branch: the half instances are families of their own"""
    return name if st_of(c) == "f32" else "%s:%s" % (name, st_of(c))


# ======================================================================================================== bilinear_bwd
# launcher (ppst_bilinear_bwd_st): C % 4 == 0 and dx_ld % 4 == 0 and dy_ld % 4 == 0 and 16-byte pointers -> gather, else scatter
def _bil_make(c):
    g = _gen(c)
    p = c.p
    return {"dy": _store(_wide(c, g, "dy", p["B"], p["OH"], p["OW"]), st_of(c)), "x": _store(_randn(g, p["B"], p["H"], p["W"], p["C"]), st_of(c))}


def _bil_bwd(dy, H, W, dt):
    B, OH, OW, C = dy.shape
    x = torch.zeros(B, C, H, W, dtype=dt, requires_grad=True)
    y = F.interpolate(x, size=(OH, OW), mode="bilinear", align_corners=False)
    y.backward(_nchw(dy.to(dt)))
    return _nhwc(x.grad)


def _bil_ref(c, inp, dt):
    return {"dx": _bil_bwd(_sl(c, inp, "dy"), c.p["H"], c.p["W"], dt)}


def _bil_branch(c):
    return _fam("bilinear_bwd:gather" if _vec_ok(c, c.p["C"], "dy") else "bilinear_bwd:scatter", c)


def _bil_mut(c, inp):
    p = c.p
    dy = _sl(c, inp, "dy").clone()
    out = []
    a = dy.clone(); a[:, -1] = 0
    out.append(("last output row left out of the window", {"dx": _bil_bwd(a, p["H"], p["W"], torch.float64)}))
    a = dy.clone(); a[:, :, 0] = 0
    out.append(("first output column left out of the window", {"dx": _bil_bwd(a, p["H"], p["W"], torch.float64)}))
    if p.get("dy_off", 0):
        out.append(("slice offset ignored", {"dx": _bil_bwd(_sl(c, inp, "dy", off=0), p["H"], p["W"], torch.float64)}))
    if p["C"] % 4:
        out.append(("scalar tail channels zero", {"dx": _zero_tail(_bil_bwd(dy, p["H"], p["W"], torch.float64), p["C"] % 4)}))
    return out


OPS["bilinear_bwd"] = Spec(_bil_make, _bil_ref, _bil_branch, _bil_mut, BAR_EW)
_BIL_SHAPES = [((5, 7), (12, 9)), ((12, 9), (5, 7)), ((64, 64), (8, 8)), ((8, 8), (64, 64)), ((1, 6), (4, 6)), ((6, 1), (6, 5)),
               ((16, 16), (16, 16))]
for (_h, _w), (_oh, _ow) in _BIL_SHAPES:
    for _C in (4, 8):
        _case("bilinear_bwd", "C%d-%dx%d-to-%dx%d" % (_C, _h, _w, _oh, _ow), B=3 if _C == 4 else 1, C=_C, H=_h, W=_w, OH=_oh, OW=_ow)
for _C in (3, 6):
    _case("bilinear_bwd", "C%d-5x7-to-12x9" % _C, B=3, C=_C, H=5, W=7, OH=12, OW=9)
    _case("bilinear_bwd", "C%d-12x9-to-5x7" % _C, B=1, C=_C, H=12, W=9, OH=5, OW=7)
_case("bilinear_bwd", "C8-slice-ld16-off4", B=3, C=8, H=5, W=7, OH=12, OW=9, dy_ld=16, dy_off=4)
_case("bilinear_bwd", "C8-slice-ld14-off4", B=3, C=8, H=12, W=9, OH=5, OW=7, dy_ld=14, dy_off=4)      # ld % 4 != 0 -> scatter
_case("bilinear_bwd", "C8-slice-ld16-off2", B=1, C=8, H=5, W=7, OH=12, OW=9, dy_ld=16, dy_off=2)      # pointer off the 16-byte grid
# half storage (bilinear_bwd_gather_kernel<ST>; the scatter form is fp32 only): up, down, the x8 reduction, and a slice whose start
# (4 halves) is 8-byte but not 16-byte aligned
for _st in ("f16", "bf16"):
    _case("bilinear_bwd", "%s-C8-5x7-to-12x9" % _st, st=_st, B=3, C=8, H=5, W=7, OH=12, OW=9)
    _case("bilinear_bwd", "%s-C8-12x9-to-5x7" % _st, st=_st, B=1, C=8, H=12, W=9, OH=5, OW=7)
    _case("bilinear_bwd", "%s-C4-64x64-to-8x8" % _st, st=_st, B=1, C=4, H=64, W=64, OH=8, OW=8)
    _case("bilinear_bwd", "%s-C8-slice-ld16-off4" % _st, st=_st, B=3, C=8, H=5, W=7, OH=12, OW=9, dy_ld=16, dy_off=4)


# ================================================================================================== pad2d, pad2d_bwd
# launchers (ppst_pad2d_st / ppst_pad2d_bwd_st, fp32): C % 4 == 0 (and x_ld % 4 == 0, 16-byte pointers) -> four channels per thread (pad2d_kernel<float4>, pad2d_bwd_kernel<4>), else one (<float>, <1>)
def pad_src(n, p0, p1, mode):
    """source index of every padded position (-1: zero), F.pad semantics; negative pads crop"""
    t = np.arange(n + p0 + p1) - p0
    if mode == 0:
        return np.where((t >= 0) & (t < n), t, -1)
    if mode == 1:
        t = np.abs(t)
        t = np.where(t >= n, 2 * (n - 1) - t, t)
        return t
    return np.clip(t, 0, n - 1)


def _pad_fwd(x, pads, mode):
    py0, py1, px0, px1 = pads
    sy, sx = pad_src(x.shape[1], py0, py1, mode), pad_src(x.shape[2], px0, px1, mode)
    y = x[:, torch.from_numpy(np.maximum(sy, 0))][:, :, torch.from_numpy(np.maximum(sx, 0))]
    keep = torch.from_numpy(((sy >= 0)[:, None] & (sx >= 0)[None, :]))
    return y * keep[None, :, :, None].to(y.dtype)


def _pad_bwd(dy, H, W, pads, mode):
    py0, py1, px0, px1 = pads
    sy, sx = pad_src(H, py0, py1, mode), pad_src(W, px0, px1, mode)
    dy = dy[:, torch.from_numpy(sy >= 0)][:, :, torch.from_numpy(sx >= 0)]
    dx = torch.zeros(dy.shape[0], H, W, dy.shape[3], dtype=dy.dtype)
    tmp = torch.zeros(dy.shape[0], H, dy.shape[2], dy.shape[3], dtype=dy.dtype)
    tmp.index_add_(1, torch.from_numpy(sy[sy >= 0]), dy)
    dx.index_add_(2, torch.from_numpy(sx[sx >= 0]), tmp)
    return dx


def pad_count(H, W, pads, mode):
    """number of padded positions that read each input pixel (<= 1: the gradient there is a copy, bit equal)"""
    return _pad_bwd(torch.ones(1, H + pads[0] + pads[1], W + pads[2] + pads[3], 1, dtype=torch.float64), H, W, pads, mode)[0, :, :, 0].numpy()


def _pad_make(c):
    g = _gen(c)
    p = c.p
    py0, py1, px0, px1 = p["pads"]
    return {"x": _store(_wide(c, g, "x", p["B"], p["H"], p["W"]), st_of(c)),
            "dy": _store(_randn(g, p["B"], p["H"] + py0 + py1, p["W"] + px0 + px1, p["C"]), st_of(c))}


def _pad_ref(c, inp, dt):
    p = c.p
    return {"y": _pad_fwd(_sl(c, inp, "x").to(dt), p["pads"], p["mode"]), "dx": _pad_bwd(inp["dy"].to(dt), p["H"], p["W"], p["pads"], p["mode"])}


def _pad_branch(c):
    # two launchers: the forward looks at C, x_ld and the pointers; the backward (dy and dx dense) at C alone
    if st_of(c) != "f32":        # half: four channels as one 8-byte item (pad2d_kernel<uint2>) and pad2d_bwd_kernel<4, ST>, or refused
        assert _vec_ok(c, c.p["C"], "x")
        return _fam("pad2d:fwd-uint2:bwd-float4", c)
    return "pad2d:fwd-%s:bwd-%s" % ("float4" if _vec_ok(c, c.p["C"], "x") else "float", "float4" if c.p["C"] % 4 == 0 else "float")


def _pad_mut(c, inp):
    p = c.p
    py0, py1, px0, px1 = p["pads"]
    x, dy = _sl(c, inp, "x").double(), inp["dy"].double()
    out = []

    def both(name, pads, mode):
        # (a defect of the index map moves the data but keeps the extents: the same shapes, other sources)
        out.append((name, {"y": _pad_fwd(x, pads, mode), "dx": _pad_bwd(dy, p["H"], p["W"], pads, mode)}))
    shifts = [("origin one row late", (py0 + 1, py1 - 1, px0, px1)), ("origin one column early", (py0, py1, px0 - 1, px1 + 1)),
              ("origin one row early", (py0 - 1, py1 + 1, px0, px1)), ("origin one column late", (py0, py1, px0 + 1, px1 - 1))]
    # (reflect needs every pad below the extent: keep the shifts the reference itself can state)
    ok = [(n, q) for n, q in shifts if p["mode"] != 1 or (max(q[0], q[1]) < p["H"] and max(q[2], q[3]) < p["W"])]
    for n, q in ok[:2]:
        both(n, q, p["mode"])
    if p["mode"] and max(p["pads"]) > 0:
        both("reflect and replicate exchanged", p["pads"], 3 - p["mode"])
    if p.get("x_off", 0):
        out.append(("slice offset ignored", {"y": _pad_fwd(_sl(c, inp, "x", off=0).double(), p["pads"], p["mode"]),
                                             "dx": _pad_bwd(dy, p["H"], p["W"], p["pads"], p["mode"])}))
    return out


def _pad_cls(c, name):
    # forward, zero pad and crop: pure data movement; reflect / replicate gradients add up to (py + 1)(px + 1) values
    return BAR_MOVE if (name == "y" or c.p["mode"] == 0) else BAR_EW


OPS["pad2d"] = Spec(_pad_make, _pad_ref, _pad_branch, _pad_mut, _pad_cls)
for _m, _mn in ((0, "zero"), (1, "reflect"), (2, "replicate")):
    for _C in (3, 8):
        _case("pad2d", "%s-C%d-asym" % (_mn, _C), B=2, C=_C, H=6, W=9, pads=(2, 1, 0, 3), mode=_m)
        _case("pad2d", "%s-C%d-crop" % (_mn, _C), B=1, C=_C, H=7, W=8, pads=(-2, 1, 2, -3), mode=_m)
        _case("pad2d", "%s-C%d-H2" % (_mn, _C), B=2, C=_C, H=2, W=5, pads=(1, 1, 2, 1), mode=_m)
_case("pad2d", "reflect-C8-largest", B=1, C=8, H=5, W=4, pads=(4, 3, 3, 2), mode=1)        # the entry refuses pad >= extent
_case("pad2d", "reflect-C3-largest", B=2, C=3, H=5, W=4, pads=(4, 3, 3, 2), mode=1)
_case("pad2d", "replicate-C8-slice-ld16-off4", B=2, C=8, H=6, W=9, pads=(2, 1, 0, 3), mode=2, x_ld=16, x_off=4)
_case("pad2d", "reflect-C8-slice-ld14-off4", B=2, C=8, H=6, W=9, pads=(2, 1, 0, 3), mode=1, x_ld=14, x_off=4)
# half storage: the forward's third instantiation (uint2 items) and pad2d_bwd_kernel<4, ST>
for _st in ("f16", "bf16"):
    for _m, _mn in ((0, "zero"), (1, "reflect"), (2, "replicate")):
        _case("pad2d", "%s-%s-C8-asym" % (_st, _mn), st=_st, B=2, C=8, H=6, W=9, pads=(2, 1, 0, 3), mode=_m)
        _case("pad2d", "%s-%s-C8-crop" % (_st, _mn), st=_st, B=1, C=8, H=7, W=8, pads=(-2, 1, 2, -3), mode=_m)
        _case("pad2d", "%s-%s-C8-H2" % (_st, _mn), st=_st, B=2, C=8, H=2, W=5, pads=(1, 1, 2, 1), mode=_m)
    _case("pad2d", "%s-reflect-C8-largest" % _st, st=_st, B=1, C=8, H=5, W=4, pads=(4, 3, 3, 2), mode=1)
    _case("pad2d", "%s-replicate-C8-slice-ld16-off4" % _st, st=_st, B=2, C=8, H=6, W=9, pads=(2, 1, 0, 3), mode=2, x_ld=16, x_off=4)


# ======================================================================================================== avgpool_bwd
# launcher (ppst_avgpool_bwd): one scalar kernel; the divisions by C, W, H, f are FastDiv (f = 1 and C = 3 are its edge divisors)
def _avg_make(c):
    p = c.p
    return {"dy": _wide(c, _gen(c), "dy", p["B"], p["oh"], p["ow"])}


def _avg_bwd(dy, f, dt):
    B, oh, ow, C = dy.shape
    x = torch.zeros(B, C, oh * f, ow * f, dtype=dt, requires_grad=True)
    F.adaptive_avg_pool2d(x, (oh, ow)).backward(_nchw(dy.to(dt)))
    return _nhwc(x.grad)


def _avg_ref(c, inp, dt):
    return {"dx": _avg_bwd(_sl(c, inp, "dy"), c.p["f"], dt)}


def _avg_mut(c, inp):
    f = c.p["f"]
    r = _avg_bwd(_sl(c, inp, "dy"), f, torch.float64)
    a = r.clone(); a[:, -1] = 0
    b = r.clone(); b[:, :, -1] = r[:, :, -1 - f]
    out = [("last row not written", {"dx": a}), ("last column reads the block to its left", {"dx": b})]
    if c.p.get("dy_off", 0):
        out.append(("slice offset ignored", {"dx": _avg_bwd(_sl(c, inp, "dy", off=0), f, torch.float64)}))
    return out


OPS["avgpool_bwd"] = Spec(_avg_make, _avg_ref, lambda c: "avgpool_bwd:scalar", _avg_mut, BAR_EW)
for _f in (1, 2, 4, 8):
    for _C in (3, 32):
        _case("avgpool_bwd", "f%d-C%d-16x24" % (_f, _C), B=2, C=_C, oh=16 // _f, ow=24 // _f, f=_f)
_case("avgpool_bwd", "f2-C8-slice-ld13-off5", B=2, C=8, oh=5, ow=7, f=2, dy_ld=13, dy_off=5)


# ================================================================================== gap_gmp_bwd, gap_gmp_multi_bwd
# launcher (ppst_gap_gmp_bwd_st, fp32): C % 4 == 0 and ld % 4 == 0 and 16-byte pointers -> (hw % 16 == 0 ? the strip kernel :
# gmp_argmax_kernel<4>) + gap_gmp_bwd_kernel<4>, else the <1> pair.  ppst_gap_gmp_multi_bwd: the strip form only (refuses everything else).
def _quant(g, kind, *shape, top=4):
    """float32 values on a 0.5 grid in [-top / 2, top / 2] ('quant'), or that with constant 4 x 4 plateaus ('plateau'): ties in most
    channels.  (The half cases take top = 3: 2.0 is 0x4000 in fp16 AND in bfloat16, so a maximum of 2.0 could not tell the types apart.)"""
    B, H, W, C = shape
    if kind == "plateau":
        small = torch.round(_randn(g, B, (H + 3) // 4, (W + 3) // 4, C) * 2).clamp(-top, top) / 2
        return small.repeat_interleave(4, 1).repeat_interleave(4, 2)[:, :H, :W].contiguous()
    return torch.round(_randn(g, *shape) * 2).clamp(-top, top) / 2


def _mask_vals(g, *shape):
    """mask values in {0, 0.25, 0.5, 1}: every product m * x of a float32 x is exact"""
    return torch.tensor([0.0, 0.25, 0.5, 1.0])[torch.randint(0, 4, shape, generator=g)]


def gmp_forward32(x, mask):
    """what the forward hands the backward: v = cat(mean_p, max_p) of the float32 products m * x (the max is exact)"""
    mx = x if mask is None else x * mask[..., None]
    B, H, W, C = mx.shape
    mx = mx.reshape(B, H * W, C)
    return torch.cat([mx.double().mean(1).float(), mx.max(1).values], 1)


def _gmp_make(c):
    g = _gen(c)
    p = c.p
    B, H, W, C = p["B"], p["H"], p["W"], p["C"]
    ld = p.get("x_ld", C)
    top = 4 if st_of(c) == "f32" else 3
    x = _store(_quant(g, p["ties"], B, H, W, ld, top=top) if p.get("ties") else _randn(g, B, H, W, ld), st_of(c))    # (the 0.5 grid: exact in every type)
    inp = {"x": x, "g": _randn(g, B, 2 * C)}
    if p.get("mask"):
        m = _mask_vals(g, B, H, W)
        if p["mask"] == "zero_image":
            m[0] = 0
        inp["mask"] = m
    if p.get("acc"):
        inp["out0"] = _store(_randn(g, B, H, W, C), st_of(c))      # the gradient buffer added into: of x's storage type
    inp["v"] = gmp_forward32(_sl(c, inp, "x"), inp.get("mask"))
    return inp


def gmp_bwd_explicit(x, mask, g, dt, last=False, vmax=None):
    """dx = m (g_mean / P + g_max [p == arg]); arg = numpy.argmax over the row-major pixels of the float32 products m * x
    (first occurrence by contract; ``last``: the seeded defect, the last occurrence).  ``vmax`` (B, C): the kernel's own rule, seeded
    defects only -- arg = the first pixel whose product EQUALS the forward's maximum, no pixel: no routed term (what a kernel
    finds that reads x as another type than the forward did)"""
    B, H, W, C = x.shape
    P = H * W
    mx = (x if mask is None else x * mask[..., None]).reshape(B, P, C).numpy()
    arg = P - 1 - np.argmax(mx[:, ::-1], axis=1) if last else np.argmax(mx, axis=1)          # (B, C)
    if vmax is not None:
        eq = mx == vmax.numpy()[:, None, :]
        arg = np.where(eq.any(1), np.argmax(eq, axis=1), -1)
    hit = torch.from_numpy(np.arange(P)[None, :, None] == arg[:, None, :]).to(dt)
    g = g.to(dt)
    dx = g[:, None, :C] / P + g[:, None, C:] * hit
    if mask is not None:
        dx = dx * mask.reshape(B, P, 1).to(dt)
    return dx.reshape(B, H, W, C)


def gmp_bwd_autograd(x, mask, g):
    """float64 autograd of cat(mean, adaptive_max_pool2d(., 1)) of m * x (routes a tie to the first maximum)"""
    x = x.double().clone().requires_grad_(True)
    mx = _nchw(x if mask is None else x * mask.double()[..., None])
    v = torch.cat([mx.mean((2, 3)), F.adaptive_max_pool2d(mx, 1).flatten(1)], 1)
    v.backward(g.double())
    return x.grad


def _gmp_ref(c, inp, dt):
    dx = gmp_bwd_explicit(_sl(c, inp, "x"), inp.get("mask"), inp["g"], dt)
    return {"dx": dx + inp["out0"].to(dt) if "out0" in inp else dx}


def _gmp_branch(c):
    if not _vec_ok(c, c.p["C"], "x"):
        assert st_of(c) == "f32", "half storage: the strip form only"
        return "gap_gmp_bwd:scalar"
    if (c.p["H"] * c.p["W"]) % 16:
        assert st_of(c) == "f32", "half storage: the strip form only"
        return "gap_gmp_bwd:4e"
    return _fam("gap_gmp_bwd:strip", c)


def _gmp_mut(c, inp):
    p = c.p
    x, m, g = _sl(c, inp, "x"), inp.get("mask"), inp["g"]
    acc = inp["out0"].double() if "out0" in inp else 0
    out = []
    if p.get("ties"):
        out.append(("tie sent to the last pixel", {"dx": gmp_bwd_explicit(x, m, g, torch.float64, last=True) + acc}))
    else:
        sw = torch.cat([g[:, p["C"]:], g[:, :p["C"]]], 1)
        out.append(("mean and max halves of g exchanged", {"dx": gmp_bwd_explicit(x, m, sw, torch.float64) + acc}))
    if m is not None:
        r = gmp_bwd_explicit(x, None, g, torch.float64) * m.double()[..., None]
        out.append(("arg-max of x, not of mask * x", {"dx": r + acc}))
    else:
        B, P = p["B"], p["H"] * p["W"]
        mean = (g.double()[:, None, :p["C"]] / P).expand(B, P, p["C"])
        routed = gmp_bwd_explicit(x, None, g, torch.float64).reshape(B, P, -1) - mean
        out.append(("routed term one pixel late", {"dx": (mean + routed.roll(1, 1)).reshape(B, p["H"], p["W"], -1) + acc}))
    if "out0" in inp:
        out.append(("accumulate overwrites", {"dx": gmp_bwd_explicit(x, m, g, torch.float64)}))
    if p.get("x_off", 0):
        out.append(("slice offset ignored", {"dx": gmp_bwd_explicit(_sl(c, inp, "x", off=0), m, g, torch.float64) + acc}))
    if p["C"] % 4:
        out.append(("scalar tail channels zero", {"dx": _zero_tail(gmp_bwd_explicit(x, m, g, torch.float64) + acc, p["C"] % 4)}))
    if st_of(c) != "f32":        # (the 16 bits of either type order alike: the arg-max of the misread x is that of x, but no value equals v's)
        out.append(("operands read as the other half type",
                    {"dx": gmp_bwd_explicit(as_other_half(x, st_of(c)), m, g, torch.float64, vmax=inp["v"][:, p["C"]:]) + acc}))
    return out


OPS["gap_gmp_bwd"] = Spec(_gmp_make, _gmp_ref, _gmp_branch, _gmp_mut, BAR_EW)
for _name, _kw in (("strip-C8-16x12", dict(C=8, H=16, W=12)), ("4e-C8-15x7", dict(C=8, H=15, W=7)), ("scalar-C6-15x7", dict(C=6, H=15, W=7)),
                   ("scalar-C6-16x12", dict(C=6, H=16, W=12))):
    _case("gap_gmp_bwd", _name + "-plain", B=2, **_kw)
    _case("gap_gmp_bwd", _name + "-mask", B=2, mask="rand", **_kw)
    _case("gap_gmp_bwd", _name + "-quant-ties", B=3, ties="quant", **_kw)
    _case("gap_gmp_bwd", _name + "-plateau-ties-mask", B=2, ties="plateau", mask="rand", **_kw)
    _case("gap_gmp_bwd", _name + "-zero-image-acc", B=2, ties="quant", mask="zero_image", acc=True, **_kw)
_case("gap_gmp_bwd", "strip-C8-slice-ld16-off4-ties", B=2, C=8, H=16, W=12, ties="plateau", x_ld=16, x_off=4)
_case("gap_gmp_bwd", "4e-C8-slice-ld12-off4-mask", B=2, C=8, H=15, W=7, ties="plateau", mask="rand", x_ld=12, x_off=4)
_case("gap_gmp_bwd", "scalar-C8-slice-ld14-off3", B=2, C=8, H=16, W=12, ties="quant", x_ld=14, x_off=3)      # ld % 4 != 0 -> scalar
# half storage: gmp_argmax4_kernel<ST> + gap_gmp_bwd_kernel<4, ST> (the strip form only); zero-image-acc adds into a half buffer
for _st in ("f16", "bf16"):
    _kw = dict(st=_st, C=8, H=16, W=12)
    _case("gap_gmp_bwd", "%s-strip-C8-16x12-plain" % _st, B=2, **_kw)
    _case("gap_gmp_bwd", "%s-strip-C8-16x12-mask" % _st, B=2, mask="rand", **_kw)
    _case("gap_gmp_bwd", "%s-strip-C8-16x12-quant-ties" % _st, B=3, ties="quant", **_kw)
    _case("gap_gmp_bwd", "%s-strip-C8-16x12-plateau-ties-mask" % _st, B=2, ties="plateau", mask="rand", **_kw)
    _case("gap_gmp_bwd", "%s-strip-C8-16x12-zero-image-acc" % _st, B=2, ties="quant", mask="zero_image", acc=True, **_kw)
    _case("gap_gmp_bwd", "%s-strip-C8-slice-ld16-off4-ties" % _st, B=2, ties="plateau", x_ld=16, x_off=4, **_kw)


def _gmm_make(c):
    g = _gen(c)
    p = c.p
    B, H, W, C, nm = p["B"], p["H"], p["W"], p["C"], p["nm"]
    heads = nm + (1 if p["plain"] else 0)
    inp = {"x": _store(_quant(g, p["ties"], B, H, W, p.get("x_ld", C), top=4 if st_of(c) == "f32" else 3), st_of(c)), "masks": _mask_vals(g, B, H, W, nm), "g": _randn(g, heads * B, 2 * C)}
    if p.get("acc"):
        inp["out0"] = _store(_randn(g, B, H, W, C), st_of(c))
    x = _sl(c, inp, "x")
    inp["v"] = torch.cat([gmp_forward32(x, m) for m in _gmm_heads(c, inp)], 0)
    return inp


def _gmm_heads(c, inp):
    return ([None] if c.p["plain"] else []) + [inp["masks"][..., i] for i in range(c.p["nm"])]


def _gmm_sum(c, inp, g, dt, last=False, off=None, misread=False):
    B, C = c.p["B"], c.p["C"]
    x = _sl(c, inp, "x", off=off)
    if misread:
        x = as_other_half(x, st_of(c))
    dx = sum(gmp_bwd_explicit(x, m, g[h * B:(h + 1) * B], dt, last=last, vmax=inp["v"][h * B:(h + 1) * B, C:] if misread else None)
             for h, m in enumerate(_gmm_heads(c, inp)))
    return dx + inp["out0"].to(dt) if "out0" in inp else dx


def _gmm_mut(c, inp):
    B = c.p["B"]
    heads = c.p["nm"] + (1 if c.p["plain"] else 0)
    g = inp["g"]
    out = [("tie sent to the last pixel", {"dx": _gmm_sum(c, inp, g, torch.float64, last=True)})]
    if heads > 1 and B > 1:
        gb = g.reshape(heads, B, -1).transpose(0, 1).reshape(heads * B, -1)
        out.append(("rows of g taken batch-major", {"dx": _gmm_sum(c, inp, gb, torch.float64)}))
    else:
        out.append(("mean and max halves of g exchanged", {"dx": _gmm_sum(c, inp, torch.cat([g[:, c.p["C"]:], g[:, :c.p["C"]]], 1), torch.float64)}))
    if "out0" in inp:
        out.append(("accumulate overwrites", {"dx": _gmm_sum(c, inp, g, torch.float64) - inp["out0"].double()}))
    if c.p.get("x_off", 0):
        out.append(("slice offset ignored", {"dx": _gmm_sum(c, inp, g, torch.float64, off=0)}))
    if st_of(c) != "f32":
        out.append(("operands read as the other half type", {"dx": _gmm_sum(c, inp, g, torch.float64, misread=True)}))
    return out


OPS["gap_gmp_multi_bwd"] = Spec(_gmm_make, lambda c, inp, dt: {"dx": _gmm_sum(c, inp, inp["g"], dt)}, lambda c: _fam("gap_gmp_multi_bwd:strip", c),
                                _gmm_mut, BAR_EW)
for _nm in (1, 3):
    for _pl in (True, False):
        _case("gap_gmp_multi_bwd", "nm%d-%s-quant" % (_nm, "plain" if _pl else "noplain"), B=2, C=8, H=16, W=12, nm=_nm, plain=_pl, ties="quant")
_case("gap_gmp_multi_bwd", "nm3-plain-plateau-acc", B=3, C=8, H=8, W=20, nm=3, plain=True, ties="plateau", acc=True)
_case("gap_gmp_multi_bwd", "nm1-noplain-plateau-slice-ld16-off8", B=1, C=4, H=8, W=20, nm=1, plain=False, ties="plateau", x_ld=16, x_off=8)
for _st in ("f16", "bf16"):
    _case("gap_gmp_multi_bwd", "%s-nm3-plain-quant" % _st, st=_st, B=2, C=8, H=16, W=12, nm=3, plain=True, ties="quant")
    _case("gap_gmp_multi_bwd", "%s-nm3-plain-plateau-acc" % _st, st=_st, B=3, C=8, H=8, W=20, nm=3, plain=True, ties="plateau", acc=True)
    # (B = 6: with one head and four channels only the routed elements stand above b s, where a rounding shows -- one image has four)
    _case("gap_gmp_multi_bwd", "%s-nm1-noplain-plateau-slice-ld16-off8" % _st, st=_st, B=6, C=4, H=8, W=20, nm=1, plain=False, ties="plateau",
          x_ld=16, x_off=8)


# ============================================================================================================= colsum
# launcher (ppst_colsum_st, fp32): C % 4 == 0 and ld % 4 == 0 and 16-byte x -> colsum4 else scalar; cdiv(rows, 2048) blocks
def _cs_make(c):
    g = _gen(c)
    inp = {"x": _store(_wide(c, g, "x", c.p["rows"]), st_of(c))}
    if c.p.get("acc"):
        inp["out0"] = _randn(g, c.p["C"])
    return inp


def _cs_eval(c, inp, dt, x=None, scale=None, acc=True):
    x = _sl(c, inp, "x") if x is None else x
    s = x.to(dt).sum(0) * (c.p.get("scale", 1.0) if scale is None else scale)
    return {"out": s + inp["out0"].to(dt) if ("out0" in inp and acc) else s}


def _cs_mut(c, inp):
    x = _sl(c, inp, "x")
    out = [("last row left out", _cs_eval(c, inp, torch.float64, x=x[:-1]) if x.shape[0] > 1 else {"out": torch.zeros(c.p["C"], dtype=torch.float64)}),
           ("last column not written", {"out": _zero_tail(_cs_eval(c, inp, torch.float64)["out"], 1)})]
    if c.p["rows"] > 2048:
        out.append(("second block's partial left out", _cs_eval(c, inp, torch.float64, x=x[:2048])))
    if c.p.get("scale", 1.0) != 1.0:
        out.append(("scale ignored", _cs_eval(c, inp, torch.float64, scale=1.0)))
    if "out0" in inp:
        out.append(("accumulate overwrites", _cs_eval(c, inp, torch.float64, acc=False)))
    if c.p.get("x_off", 0):
        out.append(("slice offset ignored", _cs_eval(c, inp, torch.float64, x=_sl(c, inp, "x", off=0))))
    if c.p["C"] % 4:
        out.append(("scalar tail channels zero", {"out": _zero_tail(_cs_eval(c, inp, torch.float64)["out"], c.p["C"] % 4)}))
    if c.p["C"] > 1024 and _vec_ok(c, c.p["C"], "x"):        # colsum4_partial_kernel: 256 lanes of 4 channels per pass
        out.append(("channels beyond the first channel pass zero", {"out": _zero_tail(_cs_eval(c, inp, torch.float64)["out"], c.p["C"] - 1024)}))
    return out


def _cs_branch(c):
    assert st_of(c) == "f32" or _vec_ok(c, c.p["C"], "x"), "half storage: the four-channel form only"
    return _fam(("colsum:four" if _vec_ok(c, c.p["C"], "x") else "colsum:scalar") + (":blocks>1" if c.p["rows"] > 2048 else ":one-block"), c)


OPS["colsum"] = Spec(_cs_make, _cs_eval, _cs_branch, _cs_mut, lambda c, n: _sum_bar(c.p["rows"]))
for _rows in (1, 2047, 2048, 2049):
    for _C in (3, 64):
        _case("colsum", "rows%d-C%d" % (_rows, _C), rows=_rows, C=_C)
_case("colsum", "rows2049-C64-slice-ld80-off8-scale-acc", rows=2049, C=64, x_ld=80, x_off=8, scale=0.37, acc=True)
_case("colsum", "rows300-C8-slice-ld11-off3-scale", rows=300, C=8, x_ld=11, x_off=3, scale=-1.5)
_case("colsum", "rows4100-C3-acc", rows=4100, C=3, acc=True)
# half storage (colsum4_partial_kernel<ST>; the sums fp32): the four-in-flight loop and its tail at C = 8 (2 lanes, 128 row slots: rows 1,
# 7 tail only, 2048 the unrolled loop alone, 2049 a second block), a slice, and C = 1028: 257 lanes of 4, a second channel pass
for _st in ("f16", "bf16"):
    for _rows in (1, 7, 2048, 2049):
        _case("colsum", "%s-rows%d-C8" % (_st, _rows), st=_st, rows=_rows, C=8)
    _case("colsum", "%s-rows2049-C64-slice-ld80-off8-scale-acc" % _st, st=_st, rows=2049, C=64, x_ld=80, x_off=8, scale=0.37, acc=True)
    _case("colsum", "%s-rows37-C1028" % _st, st=_st, rows=37, C=1028)


# ============================================================================================================= linear
# launchers: ppst_linear_dgrad[_gate]: one partial launch per LDG_BMAX = 16 batch rows, slices of LDG_ROWS = 16 rows of W (a full
# slice takes the unrolled form, the ragged last one the loop), 256 columns per block.  ppst_linear_wgrad: K % 4 == 0 (16-byte
# x, dw) -> four columns per thread, else scalar.  ppst_linear_wgrad_fused: K % 4 == 0 only (refuses the rest).
def _lin_make(c):
    g = _gen(c)
    p = c.p
    B, N, K = p["B"], p["N"], p["K"]
    inp = {"dy": _randn(g, B, N), "w": _randn(g, N, K), "x": _away(_randn(g, B, K)), "gate": _away(_randn(g, B, K))}
    if p.get("acc"):
        inp["dw0"], inp["db0"] = _randn(g, N, K), _randn(g, N)
    return inp


def _lin_eval(c, inp, dt, B=None, N=None, gate=True, relu=True, acc=True, scale=None):
    """every gradient of the case: dx, dx_gate (dgrad), dw, dw_fused, db (wgrad); B / N: only the first B batch rows / N rows of
    W take part (seeded defects)"""
    p = c.p
    s = p.get("scale", 1.0) if scale is None else scale
    dy, w, x = inp["dy"].to(dt).clone(), inp["w"].to(dt), inp["x"].to(dt)
    dyd = dy.clone()
    if N is not None:
        dyd[:, N:] = 0
    dx = s * (dyd @ w)
    if B is not None:
        dx[B:] = 0
        dy[B:] = 0
    xr = torch.where(inp["x"] > 0, x, torch.zeros_like(x)) if (p.get("relu_in") and relu) else x
    out = {"dx": dx, "dx_gate": dx * (inp["gate"] > 0).to(dt) if gate else dx, "dw": s * (dy.t() @ x)}
    if p["K"] % 4 == 0:
        out["dw_fused"] = s * (dy.t() @ xr)
        out["db"] = p.get("bscale", 1.0) * dy.sum(0)
    if "dw0" in inp and acc:
        for k in ("dw", "dw_fused"):
            if k in out:
                out[k] = out[k] + inp["dw0"].to(dt)
        if "db" in out:
            out["db"] = out["db"] + inp["db0"].to(dt)
    return out


def _lin_mut(c, inp):
    p = c.p
    out = [("gate ignored", _lin_eval(c, inp, torch.float64, gate=False))]
    if p["B"] > 16:
        out.append(("batch rows 17.. zero", _lin_eval(c, inp, torch.float64, B=16)))
    else:
        out.append(("last batch row zero", _lin_eval(c, inp, torch.float64, B=p["B"] - 1)))
    if p["N"] % 16:
        out.append(("ragged last slice of W left out", _lin_eval(c, inp, torch.float64, N=p["N"] - p["N"] % 16)))
    if p.get("relu_in"):
        out.append(("relu_in ignored", _lin_eval(c, inp, torch.float64, relu=False)))
    if p.get("acc"):
        out.append(("accumulate overwrites", _lin_eval(c, inp, torch.float64, acc=False)))
    if p.get("scale", 1.0) != 1.0:
        out.append(("scale ignored", _lin_eval(c, inp, torch.float64, scale=1.0)))
    return out



def _lin_branch(c):
    p = c.p
    return "linear_dgrad:%s:%s:%s" % ("batches>16" if p["B"] > 16 else "one-batch-launch", "ragged-slice" if p["N"] % 16 else "full-slices",
                                      "wgrad4" if p["K"] % 4 == 0 else "wgrad-scalar")


OPS["linear"] = Spec(_lin_make, _lin_eval, _lin_branch, _lin_mut, lambda c, n: _sum_bar(c.p["N"] if n.startswith("dx") else c.p["B"]))
_case("linear", "B1-N32-K300", B=1, N=32, K=300)
_case("linear", "B16-N40-K300-relu-acc", B=16, N=40, K=300, relu_in=True, acc=True, scale=0.25, bscale=0.5)
_case("linear", "B17-N37-K259", B=17, N=37, K=259, scale=1.7)
_case("linear", "B33-N37-K260-relu-acc", B=33, N=37, K=260, relu_in=True, acc=True, scale=0.25, bscale=3.0)
_case("linear", "B33-N48-K7", B=33, N=48, K=7)
_case("linear", "B3-N1100-K64-relu", B=3, N=1100, K=64, relu_in=True)


# ==================================================================================== noise_wgrad, wgrad_small_cin
# ppst_noise_wgrad_st (fp32): C % 4 == 0, ld % 4 == 0, 16-byte dpre and (C / 4 >= 256 or 256 % (C / 4) == 0) -> four-channel, else scalar
def _nw_make(c):
    g = _gen(c)
    p = c.p
    inp = {"dpre": _store(_wide(c, g, "dpre", p["B"], p["H"], p["W"]), st_of(c)), "noise": _randn(g, p["B"], p["H"], p["W"])}
    if p.get("acc"):
        inp["out0"] = _randn(g, 1)
    return inp


def _nw_eval(c, inp, dt, drop=0, off=None, acc=True, ctail=0, idle_slots=False):
    d = _sl(c, inp, "dpre", off=off).to(dt).reshape(-1, c.p["C"])
    n = inp["noise"].to(dt).reshape(-1)
    if idle_slots:
        # the seeded defect of the widths where C / 4 does not divide 256 (noise_wgrad4_kernel): the 256 % (C / 4) threads behind the
        # last whole pixel slot take a pixel of their own, one more slot per pass, which only their channel quads reach
        lanes = c.p["C"] // 4
        slots, tail = 256 // lanes + 1, 256 % lanes
        d = d.clone()
        d[slots - 1::slots, 4 * tail:] = 0
    if ctail:
        d = d[:, :-ctail]
    if drop:
        d, n = d[:-drop], n[:-drop]
    s = (d.sum(1) * n).sum().reshape(1)
    return {"out": s + inp["out0"].to(dt) if ("out0" in inp and acc) else s}


def _nw_mut(c, inp):
    out = [("last pixel left out", _nw_eval(c, inp, torch.float64, drop=1)), ("last channel left out", _nw_eval(c, inp, torch.float64, ctail=1))]
    if "out0" in inp:
        out.append(("accumulate overwrites", _nw_eval(c, inp, torch.float64, acc=False)))
    if c.p.get("dpre_off", 0):
        out.append(("slice offset ignored", _nw_eval(c, inp, torch.float64, off=0)))
    C = c.p["C"]
    if _nw_branch(c).startswith("noise_wgrad:four"):
        if C // 4 < 256 and 256 % (C // 4):
            out.append(("idle tail lanes take a pixel slot that their channel quads alone reach", _nw_eval(c, inp, torch.float64, idle_slots=True)))
        if C // 4 > 256:
            out.append(("channels past the first 1024 left out", _nw_eval(c, inp, torch.float64, ctail=C - 1024)))
    return out


def _nw_branch(c):
    C = c.p["C"]
    if st_of(c) != "f32":          # a half tensor takes the four-channel form at every width (or is refused)
        assert _vec_ok(c, C, "dpre")
        return _fam("noise_wgrad:four", c)
    return "noise_wgrad:four" if (_vec_ok(c, C, "dpre") and (C // 4 >= 256 or 256 % (C // 4) == 0)) else "noise_wgrad:scalar"


OPS["noise_wgrad"] = Spec(_nw_make, _nw_eval, _nw_branch, _nw_mut, lambda c, n: _sum_bar(c.p["B"] * c.p["H"] * c.p["W"] * c.p["C"]))
_case("noise_wgrad", "C4-5x7", B=2, C=4, H=5, W=7)
_case("noise_wgrad", "C4-5x7-acc", B=2, C=4, H=5, W=7, acc=True)
_case("noise_wgrad", "C12-9x11-acc", B=1, C=12, H=9, W=11, acc=True)                 # 256 % 3 != 0 -> scalar
_case("noise_wgrad", "C32-33x37-slice-ld40-off8", B=2, C=32, H=33, W=37, dpre_ld=40, dpre_off=8)
_case("noise_wgrad", "C6-9x11-slice-ld9-off2", B=2, C=6, H=9, W=11, dpre_ld=9, dpre_off=2)
_case("noise_wgrad", "C1024-3x3", B=1, C=1024, H=3, W=3)                             # C / 4 >= 256
# half storage: noise_wgrad4_kernel<ST> at every width.  C96: 24 lanes, 10 pixel slots, threads 240..255 idle -- fp32 takes the scalar
# kernel there (same_form_as_f32: float64 alone judges it); C1028: 257 channel quads on 256 lanes, the `c += lanes` loop
for _st in ("f16", "bf16"):
    _case("noise_wgrad", "%s-C4-5x7" % _st, st=_st, B=2, C=4, H=5, W=7)
    _case("noise_wgrad", "%s-C4-5x7-acc" % _st, st=_st, B=2, C=4, H=5, W=7, acc=True)
    _case("noise_wgrad", "%s-C96-9x11" % _st, st=_st, B=1, C=96, H=9, W=11)
    _case("noise_wgrad", "%s-C1024-3x3" % _st, st=_st, B=1, C=1024, H=3, W=3)
    _case("noise_wgrad", "%s-C1028-3x3" % _st, st=_st, B=1, C=1028, H=3, W=3)
    _case("noise_wgrad", "%s-C32-33x37-slice-ld40-off4" % _st, st=_st, B=2, C=32, H=33, W=37, dpre_ld=40, dpre_off=4)


# ppst_wgrad_small_cin_st (fp32 dy): cout % 4 == 0 and 256 % (cout / 4) == 0 and 16-byte dy -> four-channel, else scalar; 1024 pixels per block
def _wsc_make(c):
    g = _gen(c)
    p = c.p
    inp = {"x": _wide(c, g, "x", 1, 1, p["npix"], C=p["cin"]), "dy": _store(_randn(g, 1, 1, p["npix"], p["cout"]), st_of(c))}
    if p.get("acc"):
        inp["out0"] = _randn(g, p["cout"], p["cin"], 1, 1)
    return inp


def _wsc_eval(c, inp, dt, drop=0, off=None, acc=True):
    p = c.p
    x = _sl(c, inp, "x", C=p["cin"], off=off).to(dt).reshape(-1, p["cin"])
    dy = inp["dy"].to(dt).reshape(-1, p["cout"])
    if drop:
        x, dy = x[:-drop], dy[:-drop]
    dw = (p.get("scale", 1.0) * (dy.t() @ x)).reshape(p["cout"], p["cin"], 1, 1)
    return {"dw": dw + inp["out0"].to(dt) if ("out0" in inp and acc) else dw}


def _wsc_mut(c, inp):
    out = [("last pixel left out", _wsc_eval(c, inp, torch.float64, drop=1))]
    if c.p["npix"] > 1024:
        out.append(("second block's partial left out", _wsc_eval(c, inp, torch.float64, drop=c.p["npix"] - 1024)))
    else:
        out.append(("last 3 pixels left out", _wsc_eval(c, inp, torch.float64, drop=3)))
    if "out0" in inp:
        out.append(("accumulate overwrites", _wsc_eval(c, inp, torch.float64, acc=False)))
    if c.p.get("x_off", 0):
        out.append(("slice offset ignored", _wsc_eval(c, inp, torch.float64, off=0)))
    return out


def _wsc_branch(c):
    co = c.p["cout"]
    four = co % 4 == 0 and co // 4 <= 256 and 256 % (co // 4) == 0
    assert four or st_of(c) == "f32", "a half dy: the four-channel form only"
    return _fam(("wgrad_small_cin:four" if four else "wgrad_small_cin:scalar") + (":blocks>1" if c.p["npix"] > 1024 else ":one-block"), c)


OPS["wgrad_small_cin"] = Spec(_wsc_make, _wsc_eval, _wsc_branch, _wsc_mut, lambda c, n: _sum_bar(c.p["npix"]))
for _cin in (1, 3, 4):
    for _np in (1023, 1024, 1025):
        _case("wgrad_small_cin", "cin%d-npix%d-cout32" % (_cin, _np), cin=_cin, npix=_np, cout=32, scale=0.5)
_case("wgrad_small_cin", "cin3-npix1025-cout12-acc", cin=3, npix=1025, cout=12, acc=True)         # 256 % 3 != 0 -> scalar
_case("wgrad_small_cin", "cin3-npix77-cout70-acc", cin=3, npix=77, cout=70, acc=True, scale=2.0)  # two passes of 64 lanes
_case("wgrad_small_cin", "cin3-npix1025-cout32-slice-ld8-off5", cin=3, npix=1025, cout=32, x_ld=8, x_off=5)
# a half dy (wgrad_small_cin4_kernel<ST>; x and dw fp32): Q = 8 channel quads, 32 pixel slots -- 1025 pixels: the four-in-flight loop, its
# tail and a second block of one pixel; 77: two passes and a ragged tail; cout 1024: Q = 256, ONE pixel slot
for _st in ("f16", "bf16"):
    for _cin in (1, 3, 4):
        _case("wgrad_small_cin", "%s-cin%d-npix1025-cout32" % (_st, _cin), st=_st, cin=_cin, npix=1025, cout=32, scale=0.5)
    _case("wgrad_small_cin", "%s-cin3-npix77-cout32-acc" % _st, st=_st, cin=3, npix=77, cout=32, acc=True, scale=2.0)
    _case("wgrad_small_cin", "%s-cin3-npix1025-cout32-slice-ld8-off5" % _st, st=_st, cin=3, npix=1025, cout=32, x_ld=8, x_off=5)
    _case("wgrad_small_cin", "%s-cin3-npix5-cout1024" % _st, st=_st, cin=3, npix=5, cout=1024)


# ============================================================================================================ row ops
# one kernel each (no launcher branch); the cases sit on the kernels' loops: K, cols below / at / above 256 threads and 64 lanes
def _l2_make(c):
    g = _gen(c)
    x = _randn(g, c.p["B"], c.p["K"])
    if c.p.get("zero_row"):
        x[1] = 0
        x[2] *= 0.1 / x[2].norm()                          # a row below the mode-1 eps of the case (0.5)
    return {"g": _randn(g, c.p["B"], c.p["K"]), "x": x}


def _l2_fwd(x, eps, mode):
    if mode == 0:
        return x * torch.rsqrt((x * x).sum(1, keepdim=True) + eps)              # util.normalize
    return F.normalize(x, dim=1, eps=eps)                                        # x / max(||x||, eps)


def l2norm_bwd_explicit(g, x, eps, mode, dt):
    g, x = g.to(dt), x.to(dt)
    ss = (x * x).sum(1, keepdim=True)
    gx = (g * x).sum(1, keepdim=True)
    if mode == 0:
        s = torch.rsqrt(ss + eps)
        return s * g - s ** 3 * gx * x
    nrm = ss.sqrt()
    small = nrm < eps
    s = torch.where(small, torch.full_like(nrm, 1.0 / eps), 1.0 / nrm.clamp_min(1e-300))
    return s * g - torch.where(small, torch.zeros_like(nrm), s ** 3 * gx) * x


def _l2_mut(c, inp):
    p = c.p
    r = l2norm_bwd_explicit(inp["g"], inp["x"], p["eps"], p["mode"], torch.float64)
    out = [("projection term left out", {"dx": _l2_noproj(inp, p)})]
    if p["K"] > 1:
        a = r.clone(); a[:, -1] = 0
        out.append(("last column not written", {"dx": a}))
    else:
        i2 = {"g": inp["g"][:1].expand_as(inp["g"]), "x": inp["x"][:1].expand_as(inp["x"])}
        out.append(("every row takes the sums of row 0", {"dx": _l2_noproj(inp, p) - (_l2_noproj(i2, p) - l2norm_bwd_explicit(i2["g"], i2["x"], p["eps"], p["mode"], torch.float64)) / i2["x"].double() * inp["x"].double()}))
    return out


def _l2_noproj(inp, p):
    g, x = inp["g"].double(), inp["x"].double()
    ss = (x * x).sum(1, keepdim=True)
    s = torch.rsqrt(ss + p["eps"]) if p["mode"] == 0 else 1.0 / ss.sqrt().clamp_min(p["eps"])
    return s * g


OPS["l2norm_rows_bwd"] = Spec(_l2_make, lambda c, inp, dt: {"dx": l2norm_bwd_explicit(inp["g"], inp["x"], c.p["eps"], c.p["mode"], dt)},
                              lambda c: "l2norm_rows_bwd:mode%d" % c.p["mode"], _l2_mut, lambda c, n: _sum_bar(c.p["K"]))
def _l2_scale(c, inp):
    """dx is the difference of two terms of the size of s * g (at K = 1 they cancel): errors are measured against that size"""
    return {"dx": float(_l2_noproj(inp, c.p).abs().max())}


SCALES["l2norm_rows_bwd"] = _l2_scale
for _mode, _eps in ((0, 1e-7), (1, 1e-12)):
    for _K in (1, 63, 2048):
        _case("l2norm_rows_bwd", "mode%d-K%d" % (_mode, _K), B=3, K=_K, mode=_mode, eps=_eps)
# a zero row and a row of norm 0.1: below eps = 0.5 in mode 1 (dx = g / eps), plain small rows in mode 0
_case("l2norm_rows_bwd", "mode0-K63-zero-row", B=4, K=63, mode=0, eps=0.5, zero_row=True)
_case("l2norm_rows_bwd", "mode1-K63-zero-row", B=4, K=63, mode=1, eps=0.5, zero_row=True)


def _sm_make(c):
    g = _gen(c)
    logits = _randn(g, c.p["rows"], c.p["cols"])
    if c.p.get("one_hot"):
        logits = logits * 0.05
        logits[0, c.p["cols"] // 3] += 0.4                 # / div = 0.01: forty above the mean of the rest -> a near-one-hot row
    return {"logits": logits, "p": torch.softmax(logits.double() / c.p["div"], 1).float(), "g": _randn(g, c.p["rows"], c.p["cols"])}


def softmax_bwd_explicit(p, g, div, dt):
    p, g = p.to(dt), g.to(dt)
    return p * (g - (p * g).sum(1, keepdim=True)) / div


def _sm_mut(c, inp):
    p, g = inp["p"].double(), inp["g"].double()
    r = softmax_bwd_explicit(p, g, c.p["div"], torch.float64)
    out = [("1 / div left out", {"g": r * c.p["div"]})] if c.p["div"] != 1.0 else [("row sum left out", {"g": p * g})]
    if c.p["cols"] > 1:
        w0 = (torch.arange(c.p["cols"]) % 256 < 64).double() if c.p["cols"] > 64 else (torch.arange(c.p["cols"]) < c.p["cols"] - 1).double()
        d = (p * g * w0).sum(1, keepdim=True)
        out.append(("row sum of the first wave only" if c.p["cols"] > 64 else "last column left out of the row sum", {"g": p * (g - d) / c.p["div"]}))
    else:
        out.append(("row sum left out", {"g": p * g / c.p["div"]}))
    return out


OPS["softmax_rows_bwd_"] = Spec(_sm_make, lambda c, inp, dt: {"g": softmax_bwd_explicit(inp["p"], inp["g"], c.p["div"], dt)},
                                lambda c: "softmax_rows_bwd", _sm_mut, lambda c, n: _sum_bar(c.p["cols"]))
_case("softmax_rows_bwd_", "cols1", rows=3, cols=1, div=1.0)
_case("softmax_rows_bwd_", "cols63", rows=5, cols=63, div=1.0)
_case("softmax_rows_bwd_", "cols4096-div0.01-one-hot", rows=2, cols=4096, div=0.01, one_hot=True)


def _cp_make(c):
    g = _gen(c)
    return {"g": _randn(g, c.p["B"], c.p["P"], c.p["C"]), "x": _randn(g, c.p["B"], c.p["P"], c.p["C"]) + 0.5}


def _cp_fwd(x, nc, eps=2.220446049250313e-16):
    z = torch.cat([x[..., :nc] - x[..., :nc].mean(-1, keepdim=True), x[..., nc:]], -1) if nc else x
    return z / (z.norm(dim=-1, keepdim=True) + eps)


def _cp_bwd(c, inp, dt, nc=None):
    x = inp["x"].to(dt).clone().requires_grad_(True)
    _cp_fwd(x, c.p["ncenter"] if nc is None else nc).backward(inp["g"].to(dt))
    return {"dx": x.grad}


def _cp_mut(c, inp):
    nc, C = c.p["ncenter"], c.p["C"]
    out = [("centring covers one channel too %s" % ("few" if nc else "many"), _cp_bwd(c, inp, torch.float64, nc=nc - 1 if nc else 2))]
    r = _cp_bwd(c, inp, torch.float64)["dx"]
    if C > 64:
        a = r.clone(); a[..., 64:] = 0
        out.append(("channels past the first 64 lanes zero", {"dx": a}))
    else:
        out.append(("last row not written", {"dx": torch.cat([r[:, :-1], torch.zeros_like(r[:, -1:])], 1)}))
    return out


OPS["corr_prep_bwd"] = Spec(_cp_make, _cp_bwd, lambda c: "corr_prep_bwd", _cp_mut, BAR_EW)
for _C in (64, 512):
    for _nc in (0, _C // 2, _C):
        _case("corr_prep_bwd", "C%d-ncenter%d" % (_C, _nc), B=2, P=7, C=_C, ncenter=_nc)


def _l1_make(c):
    g = _gen(c)
    n = c.p["n"]
    a = _randn(g, n)
    b = a + _away(_randn(g, n) * 0.1)
    if n > 4:
        b[::5] = a[::5]                                   # equal elements: sign(0) = 0
    return {"a": a, "b": b}


def _l1_eval(c, inp, dt, drop=0, zero=True, weight=None):
    a, b = inp["a"].to(dt), inp["b"].to(dt)
    d32 = inp["a"] - inp["b"]                             # the decision from the float32 operands
    n, w = c.p["n"], c.p.get("weight", 1.0) if weight is None else weight
    s = torch.where(d32 > 0, 1.0, torch.where(d32 < 0, -1.0, 0.0 if zero else 1.0)).to(dt)
    ab = (a - b).abs()
    return {"grad": s * (w / n), "loss": (w * ab[:n - drop].sum() / n).reshape(1)}


def _l1_mut(c, inp):
    out = [("last element left out of the mean", _l1_eval(c, inp, torch.float64, drop=1)), ("weight ignored", _l1_eval(c, inp, torch.float64, weight=1.0))]
    if c.p["n"] > 4:
        out.append(("sign(0) = 1", _l1_eval(c, inp, torch.float64, zero=False)))
    return out


OPS["l1"] = Spec(_l1_make, _l1_eval, lambda c: "l1_grad+l1_mean:%s" % ("blocks>1" if c.p["n"] > 4096 else "one-block"), _l1_mut,
                 lambda c, n: _sum_bar(c.p["n"] if n == "loss" else 1))
for _n in (1, 4095, 4097):
    _case("l1", "n%d" % _n, n=_n, weight=10.0)


def _pr_make(c):
    g = _gen(c)
    p = c.p
    B, H, W, C = p["B"], p["H"], p["W"], p["C"]
    inp = {"g": _wide(c, g, "g", B, H, W), "y": _wide(c, g, "y", B, H, W), "prelu": torch.tensor([0.25])}
    if p.get("ss"):
        inp["ss"] = torch.stack([_randn(g, B, C) * 0.5 + 1.0, _randn(g, B, C) * 0.3], -1).contiguous()
    if p.get("res"):
        inp["res"] = _wide(c, g, "res", B, H, W)
    # |z| >= 1e-3 by construction: nudge y where the float32 pre-activation falls inside the band
    for _ in range(4):
        z = _pr_z(c, inp, torch.float32)
        near = z.abs() < 2e-3
        if not near.any():
            break
        _sl(c, inp, "y")[near] += 0.05
    assert _pr_z(c, inp, torch.float64).abs().min() >= 1e-3
    return inp


def _pr_z(c, inp, dt, off=None):
    z = _sl(c, inp, "y", off=off).to(dt)
    if "ss" in inp:
        z = inp["ss"][:, None, None, :, 0].to(dt) * z + inp["ss"][:, None, None, :, 1].to(dt)
    if "res" in inp:
        z = z + _sl(c, inp, "res").to(dt)
    return z


def _pr_eval(c, inp, dt, off=None, slope_all=False):
    g = _sl(c, inp, "g").to(dt)
    z = _pr_z(c, inp, dt, off=off)
    neg = _pr_z(c, inp, torch.float64, off=off) < 0          # (|z| >= 1e-3: float32 and float64 agree on the sign)
    a = inp["prelu"].to(dt)
    return {"gpre": torch.where(neg, g * a, g), "dslope": torch.where(neg | slope_all, g * z, torch.zeros_like(g)).sum().reshape(1)}


def _pr_autograd(c, inp):
    a = inp["prelu"].double().clone().requires_grad_(True)
    z = _pr_z(c, inp, torch.float64).clone().requires_grad_(True)
    F.prelu(z, a).backward(_sl(c, inp, "g").double())
    return {"gpre": z.grad, "dslope": a.grad}


def _pr_mut(c, inp):
    out = [("slope gradient summed over every element", _pr_eval(c, inp, torch.float64, slope_all=True))]
    if "ss" in inp:
        i2 = dict(inp); del i2["ss"]
        out.append(("scale_shift ignored", _pr_eval(c, i2, torch.float64)))
    if "res" in inp:
        i2 = dict(inp); del i2["res"]
        out.append(("residual ignored", _pr_eval(c, i2, torch.float64)))
    if len(out) < 2:
        i2 = dict(inp); i2["prelu"] = torch.tensor([1.0])
        out.append(("slope read as 1", {"gpre": _pr_eval(c, i2, torch.float64)["gpre"], "dslope": _pr_eval(c, inp, torch.float64)["dslope"]}))
    if c.p.get("y_off", 0):
        out.append(("slice offset of y ignored", _pr_eval(c, inp, torch.float64, off=0)))
    return out


OPS["prelu_bwd"] = Spec(_pr_make, _pr_eval, lambda c: "prelu_bwd", _pr_mut,
                        lambda c, n: _sum_bar(c.p["B"] * c.p["H"] * c.p["W"] * c.p["C"] if n == "dslope" else 1))
for _C in (3, 32):
    _case("prelu_bwd", "C%d-plain" % _C, B=2, C=_C, H=5, W=7)
    _case("prelu_bwd", "C%d-ss" % _C, B=2, C=_C, H=5, W=7, ss=True)
    _case("prelu_bwd", "C%d-ss-res" % _C, B=3, C=_C, H=9, W=11, ss=True, res=True)
_case("prelu_bwd", "C8-ss-res-slices", B=2, C=8, H=5, W=7, ss=True, res=True, g_ld=12, g_off=4, y_ld=11, y_off=3, res_ld=16, res_off=8)

# ===================================================================================================== instance norm
# ppst_dual_stats_st / ppst_in_bwd_apply_st (fp32): C % 4 == 0, every ld % 4 == 0, 16-byte pointers -> dual_stats_kernel<4> /
# in_bwd_apply_kernel<4>, else <1>; pixel chunks of pix_chunk(hw) (64 at these sizes).  ppst_in_bwd_finalize: one kernel; mean_rstd == null is the no-norm path.
SQRT2 = 2.0 ** 0.5


def _lg(t, dt):
    """lrelu'(t) * sqrt(2), the sign from the float32 tensor handed to the kernel"""
    return torch.where(t > 0, torch.tensor(1.0, dtype=dt), torch.tensor(0.2, dtype=dt)) * SQRT2


def _in_make(c):
    g = _gen(c)
    p = c.p
    B, hw, C = p["B"], p["hw"], p["C"]
    st = st_of(c)
    lo = 1e-3 if st == "f32" else 2.0 ** -9             # (a bound every storage type holds exactly)
    y = _wide(c, g, "y", B, hw, 1)
    if p.get("big_mean"):
        y = y + 100.0                                    # channel mean 100 x its standard deviation
    inp = {"g": _store(_wide(c, g, "g", B, hw, 1), st), "y": _away(_store(y, st), lo)}
    if p.get("gate"):
        inp["gate"] = _away(_store(_wide(c, g, "gate", B, hw, 1), st), lo)
    if p.get("style"):
        inp["style"] = _randn(g, B, 2 * C) * 0.3
    y64 = _sl(c, inp, "y").double()
    mean = y64.mean((1, 2))
    rstd = 1.0 / torch.sqrt(y64.var((1, 2), unbiased=False) + 1e-5)
    inp["mr"] = torch.stack([mean, rstd], -1).float().contiguous()      # what ppst_in_finalize_train hands the backward
    return inp


def in_bwd_explicit(c, inp, dt, mr=None, drop=0, gate=True, post=True, style=True, mean_term=True, off=None):
    """dy = rstd A (g' - mean(g') - n mean(g' n)) [* lrelu'(y)], dstyle = (sum g' n, sum g'); no norm: dstyle = (sum g y, sum g).
    ``mr``: (mean, rstd) (default: the float32 pair handed to the kernel).  The flags seed the defects."""
    p = c.p
    C, hw = p["C"], p["hw"]
    g, y = _sl(c, inp, "g").to(dt), _sl(c, inp, "y", off=off).to(dt)
    if "gate" in inp and gate:
        g = g * _lg(_sl(c, inp, "gate"), dt)
    gs, ys = (g[:, :hw - drop], y[:, :hw - drop]) if drop else (g, y)
    s0, s1 = gs.sum((1, 2)), (gs * ys).sum((1, 2))
    out = {"sums": torch.stack([s0, s1], -1)}
    if not p.get("norm", True):
        out["dstyle"] = torch.cat([s1, s0], 1)
        return out
    mr = inp["mr"].to(dt) if mr is None else mr.to(dt)
    mean, rstd = mr[..., 0], mr[..., 1]
    A = inp["style"][:, :C].to(dt) + 1.0 if ("style" in inp and style) else torch.ones_like(mean)
    m1, m2 = s0 / hw, s1 / hw
    qn = rstd * (m2 - mean * m1)
    n = (y - mean[:, None, None]) * rstd[:, None, None]
    dx = (rstd * A)[:, None, None] * (g - (m1[:, None, None] if mean_term else 0) - n * qn[:, None, None])
    if p.get("post_gate") and post:
        dx = dx * _lg(_sl(c, inp, "y", off=off), dt)
    out["dx"] = dx
    if p.get("want_dstyle"):
        out["dstyle"] = torch.cat([qn * hw, s0], 1)
    return out


def in_bwd_autograd(c, inp):
    """float64 autograd of sum(g' * (norm(y) A + s1)) -- with post_gate, of y = lrelu(x) sqrt(2) in front of the norm -- with the
    exact statistics"""
    p = c.p
    C = p["C"]
    g = _sl(c, inp, "g").double()
    if "gate" in inp:
        g = g * _lg(_sl(c, inp, "gate"), torch.float64)
    y0 = _sl(c, inp, "y").double()
    x = (torch.where(y0 > 0, y0, y0 / 0.2) / SQRT2).requires_grad_(True) if p.get("post_gate") else y0.clone().requires_grad_(True)
    y = F.leaky_relu(x, 0.2) * SQRT2 if p.get("post_gate") else x
    st = inp["style"].double().clone().requires_grad_(True) if "style" in inp else None
    mean, var = y.mean((1, 2), keepdim=True), y.var((1, 2), unbiased=False, keepdim=True)
    out = (y - mean) / torch.sqrt(var + 1e-5)
    if st is not None:
        out = out * (st[:, None, None, :C] + 1.0) + st[:, None, None, C:]
    (out * g).sum().backward()
    return x.grad, (st.grad if st is not None else None), torch.stack([mean.detach()[:, 0, 0], 1.0 / torch.sqrt(var.detach()[:, 0, 0] + 1e-5)], -1)


def _in_mut(c, inp):
    p = c.p
    f = lambda **kw: in_bwd_explicit(c, inp, torch.float64, **kw)
    out = [("last pixel left out of the sums", f(drop=1))]
    if p["hw"] % 64:
        out.append(("ragged last chunk left out of the sums", f(drop=p["hw"] % 64)))
    if p.get("norm", True):
        out.append(("mean(g) term left out", f(mean_term=False)))
    if "gate" in inp:
        out.append(("gate ignored", f(gate=False)))
    if p.get("post_gate"):
        out.append(("post_gate ignored", f(post=False)))
    if "style" in inp and p.get("norm", True):
        out.append(("style scale ignored", f(style=False)))
    if p.get("y_off", 0):
        out.append(("slice offset of y ignored", f(off=0)))
    if p["C"] % 4:
        out.append(("scalar tail channels zero", {k: (_zero_tail(v, p["C"] % 4) if k != "dstyle" else v) for k, v in f().items()}))
    first = 1024 if _in_branch(c).startswith("in_bwd:four") else 256      # channels of one pass of the statistics kernel's channel loop
    if p["C"] > first:
        out.append(("channels beyond the first channel pass zero",
                    {k: (_zero_tail(v, p["C"] - first) if k != "dstyle" else v) for k, v in f().items()}))
    return out


def _in_branch(c):
    four = _vec_ok(c, c.p["C"], "g", "y", "gate")
    assert four or st_of(c) == "f32", "half storage: the four-channel forms only"
    return _fam("in_bwd:%s:%s:%s" % ("four" if four else "scalar", "chunks>1" if c.p["hw"] > 64 else "one-chunk",
                                     "norm" if c.p.get("norm", True) else "no-norm"), c)


OPS["in_bwd"] = Spec(_in_make, in_bwd_explicit, _in_branch, _in_mut, BAR_EW)
for _hw in (35, 64, 480):
    for _C in (3, 6, 32):
        _case("in_bwd", "hw%d-C%d-plain" % (_hw, _C), B=2, hw=_hw, C=_C)
        _case("in_bwd", "hw%d-C%d-gate-style-dstyle" % (_hw, _C), B=2, hw=_hw, C=_C, gate=True, style=True, want_dstyle=True)
        _case("in_bwd", "hw%d-C%d-post-gate-style" % (_hw, _C), B=3, hw=_hw, C=_C, post_gate=True, style=True)
_case("in_bwd", "hw480-C32-no-norm", B=2, hw=480, C=32, norm=False)
_case("in_bwd", "hw35-C6-no-norm", B=2, hw=35, C=6, norm=False)
_case("in_bwd", "hw480-C8-slices-gate-style-dstyle", B=2, hw=480, C=8, gate=True, style=True, want_dstyle=True, g_ld=12, g_off=4, y_ld=16, y_off=8,
      gate_ld=8 + 4, gate_off=0)
_case("in_bwd", "hw35-C8-slices-ld-odd-gate", B=2, hw=35, C=8, gate=True, g_ld=11, g_off=3, y_ld=9, y_off=1, gate_ld=10, gate_off=2)
_case("in_bwd", "hw480-C32-big-mean-style-dstyle", B=2, hw=480, C=32, style=True, want_dstyle=True, big_mean=True)
# dual_stats_kernel<V> walks the channels 256 lanes of V at a time: more than one pass only for C > 256 (V = 1) and C > 1024 (V = 4)
_case("in_bwd", "hw15-C258-gate-style-dstyle", B=2, hw=15, C=258, gate=True, style=True, want_dstyle=True)      # scalar, two channel passes
_case("in_bwd", "hw15-C1032-gate-style-dstyle", B=2, hw=15, C=1032, gate=True, style=True, want_dstyle=True)    # 258 lanes of 4: two passes
# half storage of g, y, gate and dx (dual_stats_kernel<4, ST>, in_bwd_apply_kernel<4, ST>; partial sums, coef and dstyle fp32): one
# ragged chunk, several partial rows, both gates, no norm, two channel passes, and slices that start 4 and 8 halves in -- 8-byte
# aligned pointers, g and gate not 16-byte aligned
for _st in ("f16", "bf16"):
    _case("in_bwd", "%s-hw35-C8-plain" % _st, st=_st, B=2, hw=35, C=8)
    _case("in_bwd", "%s-hw480-C8-gate-style-dstyle" % _st, st=_st, B=2, hw=480, C=8, gate=True, style=True, want_dstyle=True)
    _case("in_bwd", "%s-hw480-C8-post-gate-style" % _st, st=_st, B=3, hw=480, C=8, post_gate=True, style=True)
    _case("in_bwd", "%s-hw480-C32-no-norm" % _st, st=_st, B=2, hw=480, C=32, norm=False)
    _case("in_bwd", "%s-hw15-C1032-gate-style-dstyle" % _st, st=_st, B=2, hw=15, C=1032, gate=True, style=True, want_dstyle=True)
    _case("in_bwd", "%s-hw480-C8-slices-gate-style-dstyle" % _st, st=_st, B=2, hw=480, C=8, gate=True, style=True, want_dstyle=True,
          g_ld=12, g_off=4, y_ld=16, y_off=8, gate_ld=12, gate_off=4)


# ppst_in_finalize_train: one kernel; partial rows of (sum, sum of squares) -> scale_shift, mean_rstd.  The judge takes the float32
# partials handed to the kernel (what rounding the pixel sums lost is the matter of the statistics kernel, not of this one).
def _fin_make(c):
    g = _gen(c)
    p = c.p
    x = _randn(g, p["B"], p["n"], p["per"], p["C"]) * 1.5 + 0.7
    inp = {"x": x, "partial": torch.stack([x.double().sum(2), (x.double() ** 2).sum(2)], -1).float().contiguous(), "post_bias": _randn(g, p["C"])}
    if p.get("style"):
        inp["style"] = _randn(g, p["B"], 2 * p["C"]) * 0.3
    return inp


def _fin_eval(c, inp, dt, drop=0, bias=True, swap=False):
    p = c.p
    C, count = p["C"], p["n"] * p["per"]
    part = inp["partial"].to(dt)
    s = part[:, :p["n"] - drop].sum(1)
    mean = s[..., 0] / count
    rstd = 1.0 / torch.sqrt((s[..., 1] / count - mean * mean).clamp_min(0) + 1e-5)
    a, sh = rstd, -mean * rstd
    if "style" in inp:
        st = inp["style"].to(dt)
        s0, s1 = (st[:, C:], st[:, :C]) if swap else (st[:, :C], st[:, C:])
        a = rstd * (s0 + 1.0)
        sh = s1 - mean * a
    if bias:
        sh = sh + inp["post_bias"].to(dt)
    return {"ss": torch.stack([a, sh], -1), "mr": torch.stack([mean, rstd], -1)}


def _fin_mut(c, inp):
    out = [("last partial row left out", _fin_eval(c, inp, torch.float64, drop=1)), ("post_bias ignored", _fin_eval(c, inp, torch.float64, bias=False))]
    if "style" in inp:
        out.append(("style scale and shift exchanged", _fin_eval(c, inp, torch.float64, swap=True)))
    return out


OPS["in_finalize_train"] = Spec(_fin_make, _fin_eval, lambda c: "in_finalize_train", _fin_mut, BAR_EW)
_case("in_finalize_train", "C3-n1", B=2, C=3, n=1, per=35)
_case("in_finalize_train", "C6-n8-style", B=2, C=6, n=8, per=60, style=True)
_case("in_finalize_train", "C32-n130-style", B=3, C=32, n=130, per=16, style=True)       # more partial rows than one pass of 4 x 32


# ============================================================================================== losses, small ops
def _ls_make(c):
    return {"pred": _randn(_gen(c), c.p["n"]) + 0.3}


def _ls_eval(c, inp, dt, target=None, drop=0):
    n, w = c.p["n"], c.p["weight"]
    d = inp["pred"].to(dt) - (c.p["target"] if target is None else target)
    return {"loss": (w * (d[:n - drop] ** 2).sum() / n).reshape(1), "grad": w * 2.0 * d / n}


OPS["lsgan"] = Spec(_ls_make, _ls_eval, lambda c: "lsgan",
                    lambda c, inp: [("target ignored", _ls_eval(c, inp, torch.float64, target=0.0)), ("last element left out of the mean", _ls_eval(c, inp, torch.float64, drop=1))],
                    BAR_EW)
for _n in (1, 70, 1000):
    _case("lsgan", "n%d" % _n, n=_n, target=1.0, weight=0.5)


def _rs_make(c):
    g = _gen(c)
    p = c.p
    nrm = lambda t: t / t.norm(dim=-1, keepdim=True)
    return {"q": nrm(_randn(g, p["n"], p["C"])), "k": nrm(_randn(g, p["n"], p["C"])), "k0": nrm(_randn(g, p["n0"], p["C"])),
            "queue": nrm(_randn(g, p["K"], p["C"])).t().contiguous(), "gout": torch.tensor([1.7])}


def _rs_eval(c, inp, dt, masked=True, k0=True, T=None):
    """mean_i CE([q.k | n entries at -10 | q.queue | q.k0] / T, 0) and its gradient to q (keys and queue detached)"""
    T = 0.07 if T is None else T
    q = inp["q"].to(dt).clone().requires_grad_(True)
    cols = [(q * inp["k"].to(dt)).sum(1, keepdim=True)]
    if masked:
        cols.append(torch.full((c.p["n"], c.p["n"]), -10.0, dtype=dt))
    cols.append(q @ inp["queue"].to(dt))
    if k0:
        cols.append(q @ inp["k0"].to(dt).t())
    logits = torch.cat(cols, 1) / T
    loss = (torch.logsumexp(logits, 1) - logits[:, 0]).mean()
    (loss * inp["gout"].to(dt)[0]).backward()
    return {"loss": loss.reshape(1), "dq": q.grad}


OPS["rscl"] = Spec(_rs_make, _rs_eval, lambda c: "rscl_loss+rscl_loss_bwd",
                   # (the n current-batch entries sit at exp(-10 / T) = e^-143: leaving them out is no defect a bar can see)
                   lambda c, inp: [("k0 negatives left out", _rs_eval(c, inp, torch.float64, k0=False)), ("T read as 0.1", _rs_eval(c, inp, torch.float64, T=0.1))],
                   BAR_EW)
_case("rscl", "n1-n0_3-C64-K100", n=1, n0=3, C=64, K=100)
_case("rscl", "n6-n0_4-C256-K300", n=6, n0=4, C=256, K=300)
_case("rscl", "n6-n0_1-C30-K7", n=6, n0=1, C=30, K=7)


def _rc_make(c):
    g = _gen(c)
    p = c.p
    return {"fea": _randn(g, p["B"], p["H"], p["W"], 64), "dout": _wide(c, g, "dout", p["B"], p["H"] // 4, p["W"] // 4, C=256)}


def _rc_fwd(fea, center=True):
    B, H, W, C = fea.shape
    X = fea.reshape(B, H // 4, 4, W // 4, 4, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H // 4, W // 4, 16, C)
    d = X - X.mean(-1, keepdim=True) if center else X
    z = d / (d.norm(dim=-1, keepdim=True) + 2.220446049250313e-16)
    return (z @ z.transpose(-1, -2)).reshape(B, H // 4, W // 4, 256)


def _rc_eval(c, inp, dt, off=None, sym=True, center=True):
    fea = inp["fea"].to(dt).clone().requires_grad_(True)
    dout = _sl(c, inp, "dout", C=256, off=off).to(dt)
    if not sym:       # the defect: dz from dG alone, not dG + dG^T (half the gradient for a symmetric dG, a different one here)
        B, h, w, _ = dout.shape
        G = _rc_fwd(fea, center).reshape(B, h, w, 16, 16)
        (torch.triu(G) * dout.reshape(B, h, w, 16, 16)).sum().backward()
        return {"dfea": fea.grad}
    _rc_fwd(fea, center).backward(dout)
    return {"dfea": fea.grad}


def _rc_mut(c, inp):
    out = [("upper triangle of dG only", _rc_eval(c, inp, torch.float64, sym=False)), ("channel mean not removed", _rc_eval(c, inp, torch.float64, center=False))]
    if c.p.get("dout_off", 0):
        out.append(("slice offset ignored", _rc_eval(c, inp, torch.float64, off=0)))
    return out


OPS["rselfcorr_bwd"] = Spec(_rc_make, _rc_eval, lambda c: "rselfcorr_bwd", _rc_mut, BAR_EW)
_case("rselfcorr_bwd", "4x4", B=2, H=4, W=4)
_case("rselfcorr_bwd", "8x12", B=2, H=8, W=12)
_case("rselfcorr_bwd", "8x12-slice-ld260-off4", B=2, H=8, W=12, dout_ld=260, dout_off=4)


def _uf_make(c):
    p = c.p
    return {"g": _randn(_gen(c), p["B"], p["H"] * p["W"], p["C"] * p["k"] ** 2)}


def _uf_eval(c, inp, dt, g=None):
    p = c.p
    x = torch.zeros(p["B"], p["C"], p["H"], p["W"], dtype=dt, requires_grad=True)
    F.unfold(x, p["k"], padding=p["k"] // 2).transpose(1, 2).backward((inp["g"] if g is None else g).to(dt))
    return {"dx": _nhwc(x.grad)}


def _uf_mut(c, inp):
    p = c.p
    g = inp["g"]
    a = g.clone(); a[:, -p["W"]:] = 0
    sw = g.reshape(p["B"], -1, p["C"], p["k"], p["k"]).transpose(-1, -2).reshape(g.shape)
    return [("last image row left out", _uf_eval(c, inp, torch.float64, g=a)), ("ky and kx exchanged", _uf_eval(c, inp, torch.float64, g=sw))]


OPS["unfold_rows_bwd"] = Spec(_uf_make, _uf_eval, lambda c: "unfold_rows_bwd", _uf_mut, BAR_EW)
_case("unfold_rows_bwd", "k3-5x7-C3", B=2, H=5, W=7, C=3, k=3)
_case("unfold_rows_bwd", "k3-4x4-C8", B=1, H=4, W=4, C=8, k=3)
_case("unfold_rows_bwd", "k3-1x6-C4", B=2, H=1, W=6, C=4, k=3)


def upscale_weight_fwd(w):
    """(Cout, Cin, 3, 3) -> (Cin, Cout, 4, 4): the sum of the four one-pixel shifts of the zero-padded kernel"""
    w = F.pad(w.permute(1, 0, 2, 3), [1, 1, 1, 1])
    return w[:, :, 1:, 1:] + w[:, :, :-1, 1:] + w[:, :, 1:, :-1] + w[:, :, :-1, :-1]


def _uw_make(c):
    g = _gen(c)
    p = c.p
    inp = {"dw4": _randn(g, p["cin"], p["cout"], 4, 4)}
    if p.get("acc"):
        inp["out0"] = _randn(g, p["cout"], p["cin"], 3, 3)
    return inp


def _uw_eval(c, inp, dt, acc=True, scale=None, swap=False):
    p = c.p
    w = torch.zeros(p["cout"], p["cin"], 3, 3, dtype=dt, requires_grad=True)
    d = inp["dw4"].to(dt)
    if swap:
        d = d.reshape(p["cout"], p["cin"], 4, 4).transpose(0, 1)
    ((p.get("scale", 1.0) if scale is None else scale) * upscale_weight_fwd(w)).backward(d)
    return {"dw": w.grad + inp["out0"].to(dt) if ("out0" in inp and acc) else w.grad}


def _uw_mut(c, inp):
    out = [("dw4 indexed [cout][cin]", _uw_eval(c, inp, torch.float64, swap=True)), ("scale ignored", _uw_eval(c, inp, torch.float64, scale=1.0))]
    if "out0" in inp:
        out.append(("accumulate overwrites", _uw_eval(c, inp, torch.float64, acc=False)))
    return out


OPS["upscale_weight_bwd"] = Spec(_uw_make, _uw_eval, lambda c: "upscale_weight_bwd", _uw_mut, BAR_EW)
_case("upscale_weight_bwd", "cout5-cin3", cout=5, cin=3, scale=0.7)
_case("upscale_weight_bwd", "cout40-cin24-acc", cout=40, cin=24, scale=0.125, acc=True)


def _sb_make(c):
    g = _gen(c)
    return {"x": _randn(g, c.p["n"]), "s": torch.tensor([-0.37])}


OPS["scale_by"] = Spec(_sb_make, lambda c, inp, dt: {"y": inp["x"].to(dt) * inp["s"].to(dt)[0]}, lambda c: "scale_by",
                       lambda c, inp: [("s read as 1", {"y": inp["x"].double()}), ("last element not written", {"y": _zero_tail(inp["x"].double() * -0.37, 1)})], BAR_EW)
_case("scale_by", "n1", n=1)
_case("scale_by", "n4097", n=4097)


def _tr_make(c):
    return {"x": _randn(_gen(c), c.p["b"], c.p["M"], c.p["N"])}


def _tr_mut(c, inp):
    x = inp["x"].double()
    t = x.transpose(1, 2).contiguous()
    out = [("copied, not transposed", {"y": x.reshape(t.shape)})] if min(c.p["M"], c.p["N"]) > 1 else [("first element not written", {"y": t.flip(1).flip(1) * (torch.arange(t.numel()).reshape(t.shape) > 0)})]
    out.append(("last row not written", {"y": torch.cat([t[:, :-1], torch.zeros_like(t[:, -1:])], 1)}))
    return out


OPS["transpose_last2"] = Spec(_tr_make, lambda c, inp, dt: {"y": inp["x"].to(dt).transpose(1, 2).contiguous()}, lambda c: "transpose_last2", _tr_mut, BAR_MOVE)
_case("transpose_last2", "2x33x70", b=2, M=33, N=70)
_case("transpose_last2", "1x1x5", b=1, M=1, N=5)
_case("transpose_last2", "3x64x64", b=3, M=64, N=64)


# ========================================================================================================= conv_wgrad
# ops.conv_wgrad on the three plan kinds it takes.  What the kernel reads as x / dy, and the forward whose weight gradient it is:
#   'conv'    x (B,H,W,cin), dy (B,H,W,cout): F.conv2d(x, scale w, padding = k // 2), k = 1 or 3
#   's2d'     x = the space-to-depth copy (B,H+1,W+1,4 cin) of a (2H+1, 2W+1) tensor, dy (B,H,W,cout): F.conv2d(., scale w, stride = 2)
#   'dgradT'  x = the space-to-depth copy (B,H,W,4 cout) of the gradient at the transposed conv's (2H, 2W) output, dy = that conv's
#             INPUT (B,H,W,cin): dw = the gradient of the blurred 4x4 kernel w4 (cin,cout,4,4) of F.conv_transpose2d(., w4, stride = 2,
#             padding = 1); dw3 = ops.upscale_weight_bwd of it, the gradient of the (cout,cin,3,3) parameter through the blur
# Launchers (ops.conv_wgrad -- its choice is ops.wgrad_choose, which tests/test_abi_cpu.py holds against _cw_branch below -- then
# ppst_conv_wgrad_tr2_st / ppst_conv_wgrad_f32, csrc/train.hip):
#   cout % 4 == 0, both ld % 4 == 0, 16-byte pointers and plan precision != 2 -> conv_wgrad_tr2_kernel (bf16x3), instantiated by the
#     table's chunk lengths: 1x1 tables (no halo) with chunks % 4 == 0 -> four chunks per block ('quad'), chunks % 2 == 0 -> two
#     ('one2'); else every chunk <= 4 steps and an even chunk count -> 'pair' ('pair-exact': every chunk exactly 4 steps); else
#     'single' ('single-exact': every chunk 9 steps).  The bias sums ride on the kernel's staging pass ('csum').
#   else ppst_conv_wgrad_f32: aligned -> conv_wgrad_lds_kernel ('f32-lds'), else conv_wgrad_kernel ('f32-direct'); the bias sums are a
#     ppst_colsum launch ('colsum').
def _s2d_stack(t):
    """(B,H,W,C) -> (B,ceil(H/2),ceil(W/2),4 C): channel block py * 2 + px holds the pixels (2q + py, 2p + px); odd extents zero-padded"""
    B, H, W, Cc = t.shape
    t = F.pad(t, [0, 0, 0, W % 2, 0, H % 2])
    return t.view(B, (H + 1) // 2, 2, (W + 1) // 2, 2, Cc).permute(0, 1, 3, 2, 4, 5).reshape(B, (H + 1) // 2, (W + 1) // 2, 4 * Cc).contiguous()


def _s2d_unstack(t, H, W):
    B, th, tw, c4 = t.shape
    return t.reshape(B, th, tw, 2, 2, c4 // 4).permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * th, 2 * tw, c4 // 4)[:, :H, :W]


def _cw_kind(c):
    return c.p.get("kind", "conv")


def _cw_chan(c):
    """channels of the kernel's x and dy operands"""
    p = c.p
    return {"conv": (p["cin"], p["cout"]), "s2d": (4 * p["cin"], p["cout"]), "dgradT": (4 * p["cout"], p["cin"])}[_cw_kind(c)]


def _cw_wshape(c):
    p = c.p
    return (p["cin"], p["cout"], 4, 4) if _cw_kind(c) == "dgradT" else (p["cout"], p["cin"], p["k"], p["k"])


def _cw_make(c):
    g = _gen(c)
    p, kind = c.p, _cw_kind(c)
    xc, dc = _cw_chan(c)
    if kind == "conv":
        x = _wide(c, g, "x", p["B"], p["H"], p["W"], C=xc)
    elif kind == "s2d":
        x = _s2d_stack(_randn(g, p["B"], 2 * p["H"] + 1, 2 * p["W"] + 1, p["cin"]))
    else:
        x = _s2d_stack(_randn(g, p["B"], 2 * p["H"], 2 * p["W"], p["cout"]))
    inp = {"x": x, "dy": _wide(c, g, "dy", p["B"], p["H"], p["W"], C=dc), "w": _randn(g, p["cout"], p["cin"], p["k"], p["k"])}
    if p.get("acc"):
        inp["dw0"] = _randn(g, *_cw_wshape(c)) * 30
    if p.get("acc") or p.get("bias_dst"):
        inp["db0"] = _randn(g, p["cout"]) * 30
    return inp


def _cw_bias_acc(c):
    """the bias sums are added into the given buffer (default: whenever dw is)"""
    return bool(c.p.get("bias_acc", c.p.get("acc")))


def wg_first_pass(c):
    """(H, W, dc) mask of the (pixel, channel) pairs the FIRST pass of the weight-gradient kernels' unit walk reaches
    (csrc/train.hip, wg_units): a 128-channel n tile with nslab live 32-channel slabs has NQ = 8 nslab channel quads, and the
    block's threads cover the pixels 0 .. 256 // NQ - 1 of each 2 x 32-pixel tile in one pass"""
    p = c.p
    dc = _cw_chan(c)[1]
    pix = (torch.arange(p["H"])[:, None] % 2) * 32 + torch.arange(p["W"])[None, :] % 32          # index within the tile
    nslab = torch.tensor([min(4, -(-(dc - n // 128 * 128) // 32)) for n in range(dc)])
    return pix[:, :, None] < (256 // (8 * nslab))[None, None, :]


def _cw_eval(c, inp, dt, drop_row=False, dy_scale=None, acc=True, off=None, flip=False, wscale=None, drop_tap=None, drop_cols=0,
             csum_first_pass=False):
    p, kind = c.p, _cw_kind(c)
    xc, dc = _cw_chan(c)
    x = _sl(c, inp, "x", C=xc, off=off).to(dt)
    dy = _sl(c, inp, "dy", C=dc).to(dt).clone()
    if drop_cols:                        # the kernel's dy operand without its last pixel columns (all three kinds)
        dy[:, :, -drop_cols:] = 0
    scale = p["scale"] if wscale is None else wscale
    w = torch.zeros(p["cout"], p["cin"], p["k"], p["k"], dtype=dt, requires_grad=True)
    if kind == "dgradT":
        gout = _nchw(_s2d_unstack(x, 2 * p["H"], 2 * p["W"])).clone()        # the gradient at the transposed conv's output
        if drop_row:
            gout[:, :, -1] = 0
        xin = _nchw(dy)
        w4 = torch.zeros(p["cin"], p["cout"], 4, 4, dtype=dt, requires_grad=True)
        F.conv_transpose2d(xin, w4, stride=2, padding=1).backward(gout)
        out = {"dw": w4.grad}
        if not p.get("acc"):             # (the 3x3 gradient is taken from dw alone: not where dw also holds the buffer's old values)
            F.conv_transpose2d(xin, scale * upscale_weight_fwd(w), stride=2, padding=1).backward(gout)
            out["dw3"] = w.grad
    else:
        if drop_row:
            dy[:, -1] = 0
        gout = (p.get("dy_scale", 1.0) if dy_scale is None else dy_scale) * _nchw(dy)
        if kind == "conv":
            (scale * F.conv2d(_nchw(x), w, padding=p["k"] // 2)).backward(gout)
        else:
            (scale * F.conv2d(_nchw(_s2d_unstack(x, 2 * p["H"] + 1, 2 * p["W"] + 1)), w, stride=2)).backward(gout)
        out = {"dw": w.grad}
    if flip:
        out = {k: v.flip(2) for k, v in out.items()}
    if drop_tap is not None:
        out["dw"] = out["dw"].clone()
        out["dw"][:, :, drop_tap[0], drop_tap[1]] = 0
    if p.get("bias"):
        out["db"] = (dy * wg_first_pass(c).to(dt) if csum_first_pass else dy).sum((0, 1, 2))
        if "db0" in inp and acc and _cw_bias_acc(c):
            out["db"] = out["db"] + inp["db0"].to(dt)
    if "dw0" in inp and acc:
        out["dw"] = out["dw"] + inp["dw0"].to(dt)
    return out


def _cw_last_cols(c):
    """pixel columns of the last (ragged) column of 2 x 32-pixel tiles"""
    return c.p["W"] - (c.p["W"] - 1) // 32 * 32


def _cw_mut(c, inp):
    p, kind = c.p, _cw_kind(c)
    f = lambda **kw: _cw_eval(c, inp, torch.float64, **kw)
    out = [("last image row left out", f(drop_row=True)), ("last tile column lost", f(drop_cols=_cw_last_cols(c)))]
    if _cw_branch(c).endswith("csum"):
        out.append(("column sums skip the units beyond stride", f(csum_first_pass=True)))
    if not (kind == "dgradT" and p.get("acc")):       # (the blurred kernel's own gradient carries no scale)
        out.append(("weight scale ignored", f(wscale=1.0)))
    if p["k"] == 3:
        out.append(("ky flipped", f(flip=True)))
    if kind == "s2d":
        out.append(("the single tap of phase (1, 1) lost with its zero-weight pad step", f(drop_tap=(1, 1))))
    if kind == "dgradT":
        out.append(("tap (3, 3) of the 4x4 kernel never written", f(drop_tap=(3, 3))))
    if p.get("dy_scale", 1.0) != 1.0:
        out.append(("dy_scale ignored", f(dy_scale=1.0)))
    if p.get("acc"):
        out.append(("accumulate overwrites", f(acc=False)))
    if p.get("x_off", 0):
        out.append(("slice offset ignored", f(off=0)))
    return out


def _cw_aligned(c):
    p = c.p
    xc, dc = _cw_chan(c)
    return dc % 4 == 0 and all(p.get(n + "_ld", 4) % 4 == 0 and p.get(n + "_off", 0) % 4 == 0 for n in ("x", "dy"))


def _cw_chunks(c):
    """(lengths of the step table's chunks) of ops.ConvPlan for the case's kind"""
    p, kind = c.p, _cw_kind(c)
    if kind == "conv":
        return [p["k"] * p["k"]] * (p["cin"] // 32)
    if kind == "s2d":
        return [n for n in (4, 2, 2, 2) for _ in range(p["cin"] // 32)]      # phase (1, 1): one tap and a zero-weight pad step
    return [4] * (4 * (p["cout"] // 32))


def _cw_branch(c):
    p, kind = c.p, _cw_kind(c)
    tr2 = _cw_aligned(c) and p["prec"] != 2
    if tr2:
        lens = _cw_chunks(c)
        n, lo, hi = len(lens), min(lens), max(lens)
        if kind == "conv" and p["k"] == 1 and n % 2 == 0:
            kern = "tr2-quad" if n % 4 == 0 else "tr2-one2"
        elif hi <= 4 and n % 2 == 0:
            kern = "tr2-pair-exact" if lo == hi == 4 else "tr2-pair"
        else:
            kern = "tr2-single-exact" if lo == hi == 9 else "tr2-single"
    else:
        kern = "f32-lds" if _cw_aligned(c) else "f32-direct"
    bias = "nobias" if not p.get("bias") else ("csum" if tr2 else "colsum")
    return "conv_wgrad:%s:%s:%s" % (kind, kern, bias)


def _cw_cls(c, name):
    # the project's bar of the bf16x3 weight gradients; the fp32 kernels and the bias column sums: the fp32 class, sums of B H W terms
    # (dw3: sixteen-term blur of dw, the class of dw)
    if name in ("dw", "dw3") and _cw_aligned(c) and c.p["prec"] != 2:
        return 3e-5
    return _sum_bar(c.p["B"] * c.p["H"] * c.p["W"])


OPS["conv_wgrad"] = Spec(_cw_make, _cw_eval, _cw_branch, _cw_mut, _cw_cls)
for _prec in (0, 2):
    _case("conv_wgrad", "p%d-k3-33x70-32to32-bias" % _prec, prec=_prec, k=3, B=1, H=33, W=70, cin=32, cout=32, scale=0.5, bias=True)
    _case("conv_wgrad", "p%d-k3-30x34-96to160" % _prec, prec=_prec, k=3, B=1, H=30, W=34, cin=96, cout=160, scale=0.5)
    _case("conv_wgrad", "p%d-k1-20x36-64to256-bias" % _prec, prec=_prec, k=1, B=2, H=20, W=36, cin=64, cout=256, scale=0.5, bias=True)
    _case("conv_wgrad", "p%d-k1-17x19-128to64-acc-bias" % _prec, prec=_prec, k=1, B=2, H=17, W=19, cin=128, cout=64, scale=0.5, bias=True, acc=True)
    # the bias sums written into a given buffer while dw is added into its own, and the other way round
    _case("conv_wgrad", "p%d-k3-33x37-acc-bias-written" % _prec, prec=_prec, k=3, B=1, H=33, W=37, cin=32, cout=32, scale=0.5, bias=True, acc=True,
          bias_acc=False)
    _case("conv_wgrad", "p%d-k3-33x37-bias-added" % _prec, prec=_prec, k=3, B=1, H=33, W=37, cin=32, cout=32, scale=0.5, bias=True, bias_dst=True,
          bias_acc=True)
    _case("conv_wgrad", "p%d-k3-33x37-bias-dst-written" % _prec, prec=_prec, k=3, B=1, H=33, W=37, cin=32, cout=32, scale=0.5, bias=True, bias_dst=True,
          bias_acc=False)
    _case("conv_wgrad", "p%d-s2d-33x37-32to64-bias" % _prec, kind="s2d", prec=_prec, k=3, B=1, H=33, W=37, cin=32, cout=64, scale=0.5, bias=True)
    _case("conv_wgrad", "p%d-s2d-33x37-64to32-dyscale-acc" % _prec, kind="s2d", prec=_prec, k=3, B=2, H=33, W=37, cin=64, cout=32, scale=0.5,
          dy_scale=0.37, acc=True)
    _case("conv_wgrad", "p%d-dgradT-17x19-64to32" % _prec, kind="dgradT", prec=_prec, k=3, B=2, H=17, W=19, cin=64, cout=32, scale=0.5)
    _case("conv_wgrad", "p%d-dgradT-33x9-32to64-acc" % _prec, kind="dgradT", prec=_prec, k=3, B=1, H=33, W=9, cin=32, cout=64, scale=0.25, acc=True)
_case("conv_wgrad", "p0-k1-9x11-32to32", prec=0, k=1, B=3, H=9, W=11, cin=32, cout=32, scale=0.5)              # one chunk of one step
_case("conv_wgrad", "p0-k3-33x70-32to30-unaligned-bias", prec=0, k=3, B=1, H=33, W=70, cin=32, cout=30, scale=0.5, bias=True)
_case("conv_wgrad", "p0-k3-33x37-slices", prec=0, k=3, B=2, H=33, W=37, cin=32, cout=32, scale=0.5, x_ld=48, x_off=16, dy_ld=40, dy_off=8)
_case("conv_wgrad", "p0-k3-33x37-splits1", prec=0, k=3, B=2, H=33, W=37, cin=32, cout=64, scale=0.5, splits=1)
_case("conv_wgrad", "p0-k3-33x37-splits-many-dyscale-acc", prec=0, k=3, B=2, H=33, W=37, cin=32, cout=64, scale=0.5, splits=10000, dy_scale=0.37, acc=True)
_case("conv_wgrad", "p0-k3-33x37-dyscale", prec=0, k=3, B=2, H=33, W=37, cin=32, cout=64, scale=0.5, dy_scale=0.37)
_case("conv_wgrad", "p2-k3-33x37-dyscale-acc", prec=2, k=3, B=2, H=33, W=37, cin=32, cout=64, scale=0.5, dy_scale=0.37, acc=True)
# three live slabs of dY: NQ = 24 channel quads, stride 240 -- the one unit walk (wg_units) that is no power of two
_case("conv_wgrad", "p0-k3-9x11-32to96-bias", prec=0, k=3, B=1, H=9, W=11, cin=32, cout=96, scale=0.5, bias=True)


# ====================================================================================================== conv_wgrad_p1
# The two single-pass operand forms of ppst_conv_wgrad_tr2_st (process precision mode 1, ops.set_precision(1)): passes == 1 on
# fp32-stored operands -> conv_wgrad_tr2_kernel<.., X1 = true, ..>, and bf16-stored operands (st == PPST_ST_BF16: cout and both ld
# multiples of 8) -> conv_wgrad_tr2b_kernel; the table's chunk lengths pick the instantiation as for three passes (_cw_branch).
# x and dy are rounded to bfloat16 first: every product is then exact in fp32, and both forms differ from float64 by their fp32
# accumulation alone -- the bar of the same case at precision 0 (``bar``: _cw_cls).  The GPU test runs a case through both forms:
# fp32 storage against float64 at that bar, bf16 storage against the fp32-storage result at STORAGE_BAR.
# ``slabs``: live 32-channel slabs of dY in the last n tile -- 4: conv_wgrad_tr2_kernel's unrolled conversion pass, fewer: its unit
# walk; conv_wgrad_tr2b_kernel's column sums take the walk at every count.
STORAGE_BAR = 1e-6            # gpu_diag.t_train_half's: max|bf16-stored - fp32-stored| <= 1e-6 max|fp32-stored|


def storage_violations(ref, got):
    ref, got = np.asarray(ref, np.float64), np.asarray(got, np.float64)
    err = np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300)
    return (["max|a - b| / max|ref| = %.3e > %.0e" % (err, STORAGE_BAR)] if not err <= STORAGE_BAR else []), float(err)


def _cp_make(c):
    inp = _cw_make(c)
    for k in ("x", "dy"):
        inp[k] = inp[k].bfloat16().float()
    return inp


def _cp_eval(c, inp, dt, **kw):
    out = _cw_eval(c, inp, dt, **kw)
    out.pop("dw3", None)                     # (the blur of dw: not this kernel's)
    return out


def _cp_branch(c):
    xc, dc = _cw_chan(c)
    assert _cw_aligned(c) and dc % 8 == 0 and xc % 8 == 0, "bf16 storage: channel counts and strides multiples of 8"
    kind, kern, bias = _cw_branch(c).split(":")[1:]
    return "conv_wgrad_p1:%s:%s:slabs%d:%s" % (kind, kern, min(4, -(-(dc % 128 or 128) // 32)), bias)


def _cp_mut(c, inp):
    f = lambda **kw: _cp_eval(c, inp, torch.float64, **kw)
    out = [("last tile column lost", f(drop_cols=_cw_last_cols(c))), ("last image row left out", f(drop_row=True))]
    if c.p.get("bias"):
        out.append(("column sums skip the units beyond stride", f(csum_first_pass=True)))
    return out


OPS["conv_wgrad_p1"] = Spec(_cp_make, _cp_eval, _cp_branch, _cp_mut, _cw_cls)
# one case per dispatch branch, at the smallest extents with a ragged last tile in both directions and several tiles per block
_case("conv_wgrad_p1", "k1-17x19-128to64-bias", prec=1, k=1, B=2, H=17, W=19, cin=128, cout=64, scale=0.5, bias=True)
_case("conv_wgrad_p1", "k1-20x36-64to256-bias", prec=1, k=1, B=2, H=20, W=36, cin=64, cout=256, scale=0.5, bias=True)
_case("conv_wgrad_p1", "dgradT-17x19-64to32", kind="dgradT", prec=1, k=3, B=2, H=17, W=19, cin=64, cout=32, scale=0.5)
_case("conv_wgrad_p1", "s2d-33x37-32to64-bias", kind="s2d", prec=1, k=3, B=1, H=33, W=37, cin=32, cout=64, scale=0.5, bias=True)
# 68 tiles in ONE block: conv_wgrad_tr2b_kernel's two image buffers alternate
_case("conv_wgrad_p1", "k3-33x37-32to32-bias-splits1", prec=1, k=3, B=2, H=33, W=37, cin=32, cout=32, scale=0.5, bias=True, splits=1)
_case("conv_wgrad_p1", "k1-9x11-32to32", prec=1, k=1, B=3, H=9, W=11, cin=32, cout=32, scale=0.5)
_case("conv_wgrad_p1", "k3-9x11-32to96-bias", prec=1, k=3, B=1, H=9, W=11, cin=32, cout=96, scale=0.5, bias=True)


# ========================================================================================================= conv_dgrad
# The input-gradient plans (ops.ConvPlan kinds 'dgrad', 'dgrad_s2d', 'dgrad_s2ds') and ops.dgrad_s2d, which picks between the last
# two: forward cin <= 64 (and cin % 4 == 0) -> the phase-stacked stride-1 conv + ops.depth_to_space ('stack'), else the four-group
# scattered form ('four-group').  Reference: the input gradient of F.conv2d in float64 --
#   'dgrad'       F.conv2d(x, scale w, padding = k // 2) at (H, W); g (B,H,W,cout)
#   the s2d kinds F.conv2d(xb, scale w, stride = 2) on a tensor of extent ``bhw``; g (B,H,W,cout) with H = (bhw - 3) // 2 + 1
# ``via``: 'plan' calls the ConvPlan of ``kind``; 'entry' calls ops.dgrad_s2d and lets it choose.
def _cd_make(c):
    g = _gen(c)
    p = c.p
    return {"g": _store(_wide(c, g, "g", p["B"], p["H"], p["W"], C=p["cout"]), st_of(c)), "w": _randn(g, p["cout"], p["cin"], p["k"], p["k"])}


def _cd_eval(c, inp, dt, drop_row=False, off=None, flip=False, wscale=None, odd_rows=True):
    p = c.p
    g = _nchw(_sl(c, inp, "g", C=p["cout"], off=off).to(dt)).clone()
    if drop_row:
        g[:, :, -1] = 0
    w = inp["w"].to(dt)
    w = (p["scale"] if wscale is None else wscale) * (w.flip(2) if flip else w)
    if p["kind"] == "dgrad":
        x = torch.zeros(p["B"], p["cin"], p["H"], p["W"], dtype=dt, requires_grad=True)
        F.conv2d(x, w, padding=p["k"] // 2).backward(g)
    else:
        x = torch.zeros(p["B"], p["cin"], p["bhw"][0], p["bhw"][1], dtype=dt, requires_grad=True)
        F.conv2d(x, w, stride=2).backward(g)
    dx = _nhwc(x.grad)
    if not odd_rows:
        dx[:, 1::2] = 0
    return {"dx": dx}


def _cd_mut(c, inp):
    p = c.p
    f = lambda **kw: _cd_eval(c, inp, torch.float64, **kw)
    out = [("last image row left out", f(drop_row=True)), ("weight scale ignored", f(wscale=1.0))]
    if p["k"] == 3:
        out.append(("ky flipped", f(flip=True)))
    if p["kind"] != "dgrad":
        out.append(("the odd row phases never written", f(odd_rows=False)))
    if p.get("g_off", 0):
        out.append(("slice offset ignored", f(off=0)))
    return out


def _cd_form(c):
    p = c.p
    if p.get("via") == "entry":
        per = 4 if st_of(c) == "f32" else 8       # ops.depth_to_space moves 16-byte items: 8 channels of a half gradient
        return "entry-stack" if (p["cin"] <= 64 and p["cin"] % per == 0) else "entry-four-group"
    return {"dgrad": "k%d" % p["k"], "dgrad_s2d": "four-group", "dgrad_s2ds": "stack"}[p["kind"]]


def _cd_branch(c):
    return _fam("conv_dgrad:%s:%s" % (_cd_form(c), {0: "bf16x3", 1: "bf16x1", 2: "fp32"}[c.p["prec"]]), c)


def _cd_cls(c, name):
    # the project's bar of the bf16x3 convs; the exact-fp32 conv: the fp32 class, sums of cout k k terms; the single-pass bf16 conv on
    # bf16-stored tensors (precision mode 1): the bar the conv tests hold that mode to (tests/conv_epi_cases.py BAR[1], gpu_diag.t_conv)
    return {0: 3e-5, 1: 2e-2, 2: _sum_bar(c.p["cout"] * c.p["k"] ** 2)}[c.p["prec"]]


OPS["conv_dgrad"] = Spec(_cd_make, _cd_eval, _cd_branch, _cd_mut, _cd_cls)
for _prec in (0, 2):
    _case("conv_dgrad", "p%d-k3-33x70-32to32" % _prec, kind="dgrad", prec=_prec, k=3, B=1, H=33, W=70, cin=32, cout=32, scale=0.5)
    _case("conv_dgrad", "p%d-k3-30x34-96to160" % _prec, kind="dgrad", prec=_prec, k=3, B=1, H=30, W=34, cin=96, cout=160, scale=0.5)
    _case("conv_dgrad", "p%d-k1-20x36-64to256" % _prec, kind="dgrad", prec=_prec, k=1, B=2, H=20, W=36, cin=64, cout=256, scale=0.5)
    _case("conv_dgrad", "p%d-k1-17x19-128to64" % _prec, kind="dgrad", prec=_prec, k=1, B=2, H=17, W=19, cin=128, cout=64, scale=0.5)
    _case("conv_dgrad", "p%d-k3-33x37-slice" % _prec, kind="dgrad", prec=_prec, k=3, B=2, H=33, W=37, cin=32, cout=32, scale=0.5, g_ld=48, g_off=8)
    # the stride-2 conv's input: extent 67 x 75 (odd, the blur's) and 68 x 75 (even rows: the last row is read by no output)
    _case("conv_dgrad", "p%d-s2d-four-group-33x37-of-67x75" % _prec, kind="dgrad_s2d", prec=_prec, k=3, B=1, H=33, W=37, bhw=(67, 75), cin=32, cout=64, scale=0.5)
    _case("conv_dgrad", "p%d-s2d-stack-33x37-of-67x75" % _prec, kind="dgrad_s2ds", prec=_prec, k=3, B=1, H=33, W=37, bhw=(67, 75), cin=32, cout=64, scale=0.5)
    _case("conv_dgrad", "p%d-s2d-four-group-33x37-of-68x75" % _prec, kind="dgrad_s2d", prec=_prec, k=3, B=2, H=33, W=37, bhw=(68, 75), cin=64, cout=32, scale=0.5)
    _case("conv_dgrad", "p%d-s2d-stack-33x37-of-68x75" % _prec, kind="dgrad_s2ds", prec=_prec, k=3, B=2, H=33, W=37, bhw=(68, 75), cin=64, cout=32, scale=0.5)
_case("conv_dgrad", "p0-s2d-entry-33x37-cin32", kind="dgrad_s2ds", via="entry", prec=0, k=3, B=1, H=33, W=37, bhw=(67, 75), cin=32, cout=32, scale=0.5)
_case("conv_dgrad", "p0-s2d-entry-15x9-cin96", kind="dgrad_s2d", via="entry", prec=0, k=3, B=1, H=15, W=9, bhw=(31, 19), cin=96, cout=32, scale=0.5)
# a bf16-stored gradient through ops.dgrad_s2d (precision mode 1): cin 32 takes the stack form, cin 96 the four-group form.  The
# entry's switch asks cin % 8 of a half gradient where it asks cin % 4 of an fp32 one (_cd_form restates both) -- but no ConvPlan exists
# for a forward Cin that is no multiple of 32 (conv_tables.build), so a cin such as 12, where the two rules part, never reaches either
# form: CIN12 states the rule for the CPU test, the GPU test shows that ops refuses it by name.
_case("conv_dgrad", "p1-bf16-s2d-entry-33x37-cin32", kind="dgrad_s2ds", via="entry", prec=1, st="bf16", k=3, B=1, H=33, W=37, bhw=(67, 75), cin=32, cout=32,
      scale=0.5)
_case("conv_dgrad", "p1-bf16-s2d-entry-15x9-cin96", kind="dgrad_s2d", via="entry", prec=1, st="bf16", k=3, B=1, H=15, W=9, bhw=(31, 19), cin=96, cout=32,
      scale=0.5)
CIN12 = Case("conv_dgrad", "conv_dgrad-p1-bf16-s2d-entry-15x9-cin12", dict(kind="dgrad_s2d", via="entry", prec=1, st="bf16", k=3, B=1, H=15, W=9,
                                                                           bhw=(31, 19), cin=12, cout=32, scale=0.5), 0)


# ============================================================================================= space_to_depth, depth_to_space
# ppst_space_to_depth_st, half storage: four channels travel as one 8-byte item (s2d_kernel<uint2>; C % 4, x_ld % 4, 8-byte pointers);
# ppst_depth_to_space_st moves 16-byte items, 8 channels of a half tensor (C % 8).  's': the phase-major copy; 'back' (C % 8 == 0):
# depth_to_space of it at the input's extent, the input again.  (The fp32 forms: tests/test_gpu_backward_kernels.py, on their own.)
def _sd_stack(x, edge="zero"):
    if edge == "replicate":
        x = _nhwc(F.pad(_nchw(x), [0, x.shape[2] % 2, 0, x.shape[1] % 2], mode="replicate"))
    return _s2d_stack(x.contiguous())


def _sd_eval(c, inp, dt, off=None, edge="zero", swap=False):
    p = c.p
    x = _sl(c, inp, "x", off=off).to(dt)
    s = _sd_stack(x, edge)
    if swap:
        s = torch.cat([s[..., :p["C"]], s[..., 2 * p["C"]:3 * p["C"]], s[..., p["C"]:2 * p["C"]], s[..., 3 * p["C"]:]], -1)
    out = {"s": s}
    if p["C"] % 8 == 0:
        out["back"] = _s2d_unstack(s, p["H"], p["W"]).contiguous()
    return out


def _sd_mut(c, inp):
    out = [("phases (0, 1) and (1, 0) exchanged", _sd_eval(c, inp, torch.float64, swap=True)),
           ("the row / column beyond an odd extent copied from the edge, not zero", {"s": _sd_eval(c, inp, torch.float64, edge="replicate")["s"]})]
    if c.p.get("x_off", 0):
        out.append(("slice offset ignored", _sd_eval(c, inp, torch.float64, off=0)))
    return out


OPS["space_to_depth"] = Spec(lambda c: {"x": _store(_wide(c, _gen(c), "x", c.p["B"], c.p["H"], c.p["W"]), st_of(c))}, _sd_eval,
                             lambda c: _fam("space_to_depth:uint2" + ("+depth_to_space" if c.p["C"] % 8 == 0 else ""), c), _sd_mut, BAR_MOVE)
for _st in ("f16", "bf16"):
    _case("space_to_depth", "%s-33x37-C8" % _st, st=_st, B=2, H=33, W=37, C=8)
    _case("space_to_depth", "%s-6x5-C8" % _st, st=_st, B=2, H=6, W=5, C=8)
    _case("space_to_depth", "%s-1x7-C12" % _st, st=_st, B=2, H=1, W=7, C=12)
    _case("space_to_depth", "%s-5x7-C8-slice-ld16-off4" % _st, st=_st, B=2, H=5, W=7, C=8, x_ld=16, x_off=4)

_BY_ID = {c.id: c for c in CASES}
assert len(_BY_ID) == len(CASES), "case ids must be unique"

# every kernel family a launcher of these ops can pick (its `if`s, both sides)
FAMILIES = ["bilinear_bwd:gather", "bilinear_bwd:scatter", "pad2d:fwd-float4:bwd-float4", "pad2d:fwd-float:bwd-float4", "pad2d:fwd-float:bwd-float", "avgpool_bwd:scalar",
            "gap_gmp_bwd:strip", "gap_gmp_bwd:4e", "gap_gmp_bwd:scalar", "gap_gmp_multi_bwd:strip",
            "colsum:four:one-block", "colsum:four:blocks>1", "colsum:scalar:one-block", "colsum:scalar:blocks>1",
            "linear_dgrad:one-batch-launch:full-slices:wgrad4", "linear_dgrad:one-batch-launch:ragged-slice:wgrad4",
            "linear_dgrad:batches>16:ragged-slice:wgrad-scalar", "linear_dgrad:batches>16:ragged-slice:wgrad4",
            "linear_dgrad:batches>16:full-slices:wgrad-scalar",
            "noise_wgrad:four", "noise_wgrad:scalar", "wgrad_small_cin:four:one-block", "wgrad_small_cin:four:blocks>1",
            "wgrad_small_cin:scalar:one-block", "wgrad_small_cin:scalar:blocks>1",
            "l2norm_rows_bwd:mode0", "l2norm_rows_bwd:mode1", "softmax_rows_bwd", "corr_prep_bwd", "l1_grad+l1_mean:one-block",
            "l1_grad+l1_mean:blocks>1", "prelu_bwd",
            "in_bwd:four:one-chunk:norm", "in_bwd:four:chunks>1:norm", "in_bwd:scalar:one-chunk:norm", "in_bwd:scalar:chunks>1:norm",
            "in_bwd:four:chunks>1:no-norm", "in_bwd:scalar:one-chunk:no-norm", "in_finalize_train", "lsgan", "rscl_loss+rscl_loss_bwd",
            "rselfcorr_bwd", "unfold_rows_bwd", "upscale_weight_bwd", "scale_by", "transpose_last2",
            # conv_wgrad: every instantiation of the fp32-storage transposed-read kernel that a 'conv', 's2d' or 'dgradT' table can
            # select, both fp32 kernels, and both bias paths (csum: with the bf16x3 kernel; colsum: with the fp32 kernels)
            "conv_wgrad:conv:tr2-single-exact:nobias", "conv_wgrad:conv:tr2-single-exact:csum", "conv_wgrad:conv:tr2-single:nobias",
            "conv_wgrad:conv:tr2-one2:csum", "conv_wgrad:conv:tr2-quad:csum", "conv_wgrad:conv:f32-lds:nobias", "conv_wgrad:conv:f32-lds:colsum",
            "conv_wgrad:conv:f32-direct:colsum", "conv_wgrad:s2d:tr2-pair:csum", "conv_wgrad:s2d:tr2-pair:nobias", "conv_wgrad:s2d:f32-lds:colsum",
            "conv_wgrad:s2d:f32-lds:nobias", "conv_wgrad:dgradT:tr2-pair-exact:nobias", "conv_wgrad:dgradT:f32-lds:nobias",
            # conv_wgrad_p1: the same six instantiations in their single-pass forms (fp32 tiles and bf16 storage), at every count of
            # live dY slabs
            "conv_wgrad_p1:conv:tr2-quad:slabs2:csum", "conv_wgrad_p1:conv:tr2-one2:slabs4:csum", "conv_wgrad_p1:dgradT:tr2-pair-exact:slabs2:nobias",
            "conv_wgrad_p1:s2d:tr2-pair:slabs2:csum", "conv_wgrad_p1:conv:tr2-single-exact:slabs1:csum", "conv_wgrad_p1:conv:tr2-single:slabs1:nobias",
            "conv_wgrad_p1:conv:tr2-single-exact:slabs3:csum",
            "conv_dgrad:k3:bf16x3", "conv_dgrad:k3:fp32", "conv_dgrad:k1:bf16x3", "conv_dgrad:k1:fp32", "conv_dgrad:four-group:bf16x3",
            "conv_dgrad:four-group:fp32", "conv_dgrad:stack:bf16x3", "conv_dgrad:stack:fp32", "conv_dgrad:entry-stack:bf16x3",
            "conv_dgrad:entry-four-group:bf16x3",
            # a bf16 gradient through ops.dgrad_s2d (precision mode 1): its switch to the stack form is cin % 8
            "conv_dgrad:entry-stack:bf16x1:bf16", "conv_dgrad:entry-four-group:bf16x1:bf16"]
# the half-storage (`_st`) instances: every form a half tensor can take (the launchers refuse it the one-channel forms), in both types
HALF_FAMILIES = ["bilinear_bwd:gather", "pad2d:fwd-uint2:bwd-float4", "gap_gmp_bwd:strip", "gap_gmp_multi_bwd:strip", "colsum:four:one-block",
                 "colsum:four:blocks>1", "noise_wgrad:four", "wgrad_small_cin:four:one-block", "wgrad_small_cin:four:blocks>1",
                 "in_bwd:four:one-chunk:norm", "in_bwd:four:chunks>1:norm", "in_bwd:four:chunks>1:no-norm", "space_to_depth:uint2",
                 "space_to_depth:uint2+depth_to_space"]
FAMILIES += ["%s:%s" % (f, st) for f in HALF_FAMILIES for st in ("f16", "bf16")]
# In no case: the lpips entries (tests/test_gpu_lpips.py), and the convs' input gradient on an fp16-stored tensor (precision mode 3 does
# not train: ops.train_dtype is bfloat16 or float32).
