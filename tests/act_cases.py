"""Cases, float64 references, seeded defects and bars of the activation-path kernel tests (tests/test_act_cases_cpu.py,
tests/test_gpu_act.py): csrc/elementwise.hip -- statistics, affine_act, GAP/GMP, pooling, resize, head_tail, the small 1x1
convs, glue -- and the NHWC blur of csrc/upfirdn2d.hip.  Plain torch / numpy on the CPU: nothing here touches the device, and the
device is never its own judge.

The conventions are those of tests/bwd_cases.py (``Case``, ``Spec``, ``_gen`` seeded from the case id, ``compare``, a bar of
max(class bar, 4 x the float32 evaluation of the same reference)).  What is new:

  storage     ``st`` / ``yst`` in a case's p name the storage type of the activations (f32, f16, bf16).  ``make`` returns float32
              tensors that hold exactly the stored values (rounded once to the storage type), so the float64 reference reads
              what the kernel reads.  A half-stored OUTPUT is judged element by element with the allowed error
              b s + 2^-p (|ref| + b s): one round-to-nearest (p = 11 fp16, 8 bf16) of a value within the fp32 bar b of the
              reference, s = max|ref|.  The GPU test also asks for bit equality with the fp32 launch on the widened inputs
              rounded once (include/ppst_hip.h), which for the blur is sliding form == patch form (fp32 never slides).
  facets      ``branch(c)`` restates the launcher's ``if`` (kernel family and form); ``facets(c)`` adds what the case reaches
              inside that kernel (channel passes, masked lanes, chunk size, partial count, ragged chunk).  FORMS / FACETS are
              the full expected sets.
  borders     blur_nhwc, bilinear, affine_act with res_up2 and head_tail are judged once more on their border rows and columns
              alone, against the border's own max|ref|.

Gate inputs (LRELU, PReLU) keep |value| >= 1e-3 at the decision, evaluated from the float32 operands handed to the kernel; mask
values are in {0, 0.25, 0.5, 1} so that every product m * x is exact and the maximum is judged bit for bit.  No element is left
out of any comparison.
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from bwd_cases import (BAR_EW, BAR_MOVE, DTYPE, HALF, PBITS, Case, Spec, _gen, _mask_vals, _nchw, _nhwc, _pad_fwd, _randn,  # noqa: F401
                       _s2d_stack, _sl, _store, _sum_bar, _vec_ok, _wide, _zero_tail, compare, compare_half, half_allowed)

ACT_NONE, ACT_LRELU, ACT_PRELU = 0, 1, 2           # ops.ACT_*
SQRT2 = 1.41421356237309515
GROUP_MAX = 32                                      # PPST_GROUP_MAX
UF_SLIDE = 16                                       # csrc/upfirdn2d.hip

OPS = {}
CASES = []
OUT_ST = {}      # op -> fn(c, output name) -> storage type of that output (default f32)
BORDER = {}      # op -> fn(c) -> True: judge the border rows and columns again on their own scale


def _case(op, cid, seed=0, **p):
    CASES.append(Case(op, "%s-%s" % (op, cid), p, seed))


def cdiv(a, b):
    return (a + b - 1) // b


def _act(t, act, slope=0.0):
    if act == ACT_LRELU:
        return torch.where(t > 0, t, t * 0.2) * SQRT2
    if act == ACT_PRELU:
        return torch.where(t >= 0, t, t * slope)
    return t


def _fix_gate(x, gate, st):
    """move the stored values of x whose gate value (same shape as x, a function of x) lies within 2e-3 of the decision"""
    for _ in range(8):
        bad = gate(x).abs() < 2e-3
        if not bad.any():
            return x
        x = _store(torch.where(bad, x + 0.5, x), st)
    raise AssertionError("gate inputs stay on the boundary")


def _ss(g, B, C):
    """(B, C, 2) scale / shift pairs: |scale| in [0.5, 1.5] with both signs, shift of the size of the data"""
    a = (0.5 + torch.rand(B, C, generator=g)) * torch.where(torch.rand(B, C, generator=g) < 0.3, -1.0, 1.0)
    return torch.stack([a, _randn(g, B, C) * 0.5], -1).contiguous()


def _aff(x, ss, dt, row0=False):
    """a x + s per (image, channel) of an NHWC tensor"""
    if ss is None:
        return x
    ss = ss.to(dt)
    if row0:
        ss = ss[:1].expand_as(ss)
    return ss[:, None, None, :, 0] * x + ss[:, None, None, :, 1]


def _set_sl(c, inp, name, val, C=None):
    C = c.p["C"] if C is None else C
    off = c.p.get(name + "_off", 0)
    inp[name][..., off:off + C] = val


def _axis(n, on, dt, shift=False, clamp=True):
    """source rows and weight of F.interpolate(bilinear, align_corners=False) along one axis, the coordinate evaluated in dt as the
    kernels do: f = max((o + 0.5) n / on - 0.5, 0), i0 = (int) f, i1 = i0 + (i0 < n - 1).  shift / clamp: seeded defects."""
    o = torch.arange(on, dtype=dt)
    f = (o + 0.5) * (torch.tensor(float(n), dtype=dt) / torch.tensor(float(on), dtype=dt)) - (0.0 if shift else 0.5)
    if clamp:
        f = f.clamp_min(0)
    i0 = f.trunc().clamp(0, n - 1)
    l = f - i0
    i0 = i0.long()
    return i0, (i0 + 1).clamp_max(n - 1), l


def bilerp(x, OH, OW, dt, shift=False, clamp=True):
    """(B,H,W,C) -> (B,OH,OW,C), the kernels' expression hy (hx v00 + lx v01) + ly (hx v10 + lx v11)"""
    x = x.to(dt)
    y0, y1, ly = _axis(x.shape[1], OH, dt, shift, clamp)
    x0, x1, lx = _axis(x.shape[2], OW, dt, shift, clamp)
    ly, lx = ly[None, :, None, None], lx[None, None, :, None]
    top, bot = x[:, y0], x[:, y1]
    return (1 - ly) * ((1 - lx) * top[:, :, x0] + lx * top[:, :, x1]) + ly * ((1 - lx) * bot[:, :, x0] + lx * bot[:, :, x1])


def _pool(f, k):
    """k x k mean of an NHWC tensor whose extents k divides"""
    B, H, W, C = f.shape
    return f.reshape(B, H // k, k, W // k, k, C).mean((2, 4))


# ====================================================================================== in_stats + in_finalize, statistics
# launcher (ppst_in_stats): C % 4 == 0 and ld % 4 == 0 and 16-byte x -> chan_reduce_kernel<0, false, 4> (lane = 4 channels, lanes
# = C / 4 rounded up to a power of two <= 256 and masked, one pass per 1024 channels) else <0, false, 1> (lane = 1 channel, one
# pass per 256 channels); pix_chunk(hw) pixels per block, n_partials = ceil(hw / chunk); in_finalize_kernel walks the partials 32
# rows at a time, four-way unrolled from 128 rows on.
def pix_chunk(hw):
    chunk = 1024
    while chunk > 64 and cdiv(hw, chunk) < 2048:
        chunk >>= 1
    return chunk


def rep_w(H, W, corner=4):
    """multiplicity of every pixel in the ReplicationPad2d(1)-padded tensor"""
    wy, wx = torch.ones(H, dtype=torch.float64), torch.ones(W, dtype=torch.float64)
    wy[0] += 1; wy[-1] += 1; wx[0] += 1; wx[-1] += 1
    w = wy[:, None] * wx[None, :]
    if corner != 4:
        for i in (0, -1):
            for j in (0, -1):
                w[i, j] = corner
    return w


def _stats_x(c, g):
    """data with per-channel mean and spread of their own (a wrong channel or a wrong image shows in every statistic)"""
    p = c.p
    ld = p.get("x_ld", p["C"])
    ch = torch.arange(ld, dtype=torch.float32)
    im = torch.arange(p["B"], dtype=torch.float32)[:, None, None, None]
    return _randn(g, p["B"], p["H"], p["W"], ld) * (0.5 + (ch % 5) * 0.25) + ((ch % 7) - 3) * 0.3 + 0.2 * im


def _is_make(c):
    g = _gen(c)
    p = c.p
    inp = {"x": _stats_x(c, g)}
    if p.get("style"):
        inp["style"] = _randn(g, p["B"], 2 * p["C"]) * 0.5
        inp["post_bias"] = _randn(g, p["C"])
    return inp


def _moments(y, dt, rep_pad, drop=0, corner=4):
    B, H, W, C = y.shape
    w = (rep_w(H, W, corner) if rep_pad else torch.ones(H, W, dtype=torch.float64)).to(dt).reshape(1, H * W, 1)
    yf = y.to(dt).reshape(B, H * W, C)
    if drop:
        yf, w = yf[:, :-drop], w[:, :-drop]
    return (w * yf).sum(1), (w * yf * yf).sum(1)


def stats_count(p):
    return (p["H"] + 2) * (p["W"] + 2) if p.get("rep_pad") else p["H"] * p["W"]


def _is_eval(c, inp, dt, x=None, drop=0, corner=4, row0=False, ctail=0):
    p = c.p
    x = _sl(c, inp, "x") if x is None else x
    C = p["C"]
    s, q = _moments(x, dt, p.get("rep_pad"), drop, corner)
    if ctail:
        s, q = _zero_tail(s, ctail), _zero_tail(q, ctail)
    mean = s / stats_count(p)
    var = (q / stats_count(p) - mean * mean).clamp_min(0)
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    a, sh = rstd, -mean * rstd
    if "style" in inp:
        st = inp["style"].to(dt)
        if row0:
            st = st[:1].expand_as(st)
        a = rstd * (st[:, :C] + 1.0)
        sh = st[:, C:] - mean * a + inp["post_bias"].to(dt)
    return {"sum": s, "sumsq": q, "scale": a, "shift": sh}


def _reduce_facets(name, c, vec, C, hw):
    per = 4 if vec else 1
    lanes_needed = C // per
    out = []
    if lanes_needed > 256:
        out.append(name + ":channel-passes>1")
    elif lanes_needed & (lanes_needed - 1):
        out.append(name + ":masked-lanes")
    chunk = pix_chunk(hw)
    n = cdiv(hw, chunk)
    out.append("reduce:chunk%d" % chunk)
    out.append("finalize:partials-%s" % ("1" if n == 1 else ("2..128" if n <= 128 else ">128")))
    if hw % chunk:
        out.append("reduce:ragged-chunk")
    return out


def _last_chunk(hw):
    """pixels of the last chunk (a single chunk: the last pixel)"""
    chunk = pix_chunk(hw)
    return (hw - (cdiv(hw, chunk) - 1) * chunk) if hw > chunk else 1


def _tail_channels(vec, C):
    """channels a kernel that forgets its tail leaves at zero: C % 4 of the scalar form, those beyond the first channel pass"""
    first = 1024 if vec else 256
    return C - first if C > first else C % 4


def _is_branch(c):
    return "in_stats:vec4" if _vec_ok(c, c.p["C"], "x") else "in_stats:scalar"


def _is_facets(c):
    p = c.p
    br = _is_branch(c)
    return _reduce_facets(br, c, br.endswith("vec4"), p["C"], p["H"] * p["W"]) + (["in_stats:rep_pad"] if p.get("rep_pad") else [])


def _is_mut(c, inp):
    p = c.p
    hw = p["H"] * p["W"]
    d = _last_chunk(hw)
    out = [("last pixel chunk dropped" if hw > pix_chunk(hw) else "last pixel dropped", _is_eval(c, inp, torch.float64, drop=d)),
           ("last channel zero", _is_eval(c, inp, torch.float64, ctail=1))]
    if p.get("rep_pad"):
        out.append(("rep_pad corner weight 2 instead of 4", _is_eval(c, inp, torch.float64, corner=2)))
    if p.get("x_off", 0):
        out.append(("slice offset ignored", _is_eval(c, inp, torch.float64, x=_sl(c, inp, "x", off=0))))
    t = _tail_channels(_is_branch(c).endswith("vec4"), p["C"])
    if t:
        out.append(("tail channels zero", _is_eval(c, inp, torch.float64, ctail=t)))
    if "style" in inp and p["B"] > 1:
        out.append(("style of batch row 0 used for every row", _is_eval(c, inp, torch.float64, row0=True)))
    return out


OPS["in_stats"] = Spec(_is_make, _is_eval, _is_branch, _is_mut, lambda c, n: _sum_bar(c.p["H"] * c.p["W"]))
_case("in_stats", "C3-7x9", B=3, C=3, H=7, W=9)                                                   # 63 pixels: one partial
_case("in_stats", "C3-7x9-rep_pad", B=3, C=3, H=7, W=9, rep_pad=True)
_case("in_stats", "C12-13x11-rep_pad", B=3, C=12, H=13, W=11, rep_pad=True)                        # 3 lanes of 4: masked; ragged chunk
_case("in_stats", "C20-13x11-style", B=3, C=20, H=13, W=11, style=True)
_case("in_stats", "C64-16x16-style-rep_pad", B=3, C=64, H=16, W=16, style=True, rep_pad=True)
_case("in_stats", "C64-16x16", B=3, C=64, H=16, W=16)
_case("in_stats", "C1028-5x5", B=2, C=1028, H=5, W=5)                                             # 257 lanes of 4: two passes
_case("in_stats", "C258-5x5-rep_pad", B=2, C=258, H=5, W=5, rep_pad=True)                         # scalar, two passes, C % 4 != 0
_case("in_stats", "C8-slice-ld16-off4", B=3, C=8, H=13, W=11, x_ld=16, x_off=4, style=True)
_case("in_stats", "C8-slice-ld16-off2", B=3, C=8, H=13, W=11, x_ld=16, x_off=2, rep_pad=True)     # pointer off the 16-byte grid -> scalar
_case("in_stats", "C4-96x96", B=1, C=4, H=96, W=96)                                               # 144 partials
_case("in_stats", "C3-96x97-rep_pad", B=1, C=3, H=96, W=97, rep_pad=True)                         # scalar, 146 partials, ragged
for _h, _w in ((512, 512), (1024, 512), (1024, 1024), (2048, 1024)):                               # pix_chunk 128 / 256 / 512 / 1024
    _case("in_stats", "C4-%dx%d-chunk%d" % (_h, _w, pix_chunk(_h * _w)), B=1, C=4, H=_h, W=_w, rep_pad=(_h == 1024))


# ================================================================================================ affine_act[_stats]
# launcher (ppst_affine_act_st): vec = C, every ld multiples of 4 and the pointers on 16 bytes (8 with a half tensor); a half
# tensor takes the vector forms only; V = 8 when a half tensor is involved and C, every ld are multiples of 8 and the pointers on
# 16 bytes; else V = 4; not vec: V = 1 (fp32 only; res_up2 refused).
def _aa_make(c):
    g = _gen(c)
    p = c.p
    B, H, W, C = p["B"], p["H"], p["W"], p["C"]
    st = p.get("st", "f32")
    inp = {"x": _store(_wide(c, g, "x", B, H, W), st)}
    if p.get("ss"):
        inp["ss"] = _ss(g, B, C)
    if p.get("res"):
        h, w = (H // 2, W // 2) if p["res"] == "up2" else (H, W)
        inp["res"] = _store(_wide(c, g, "res", B, h, w), st)
        if p.get("rss"):
            inp["rss"] = _ss(g, B, C)
    if p.get("act") == ACT_PRELU:
        inp["prelu"] = torch.tensor([0.25])
    if p.get("act"):
        r = _aa_res(c, inp, torch.float32) if (p.get("res") and p.get("before")) else 0.0
        a = inp["ss"][:, None, None, :, 0] if "ss" in inp else 1.0
        b = inp["ss"][:, None, None, :, 1] if "ss" in inp else 0.0
        _set_sl(c, inp, "x", _fix_gate(_sl(c, inp, "x").clone(), lambda x: a * x + b + r, st))
        assert _aa_pre(c, inp, torch.float32)[0].abs().min() >= 1e-3
    return inp


def _aa_res(c, inp, dt, rss=True, shift=False, clamp=True, res_off=None):
    p = c.p
    if "res" not in inp:
        return None
    r = _sl(c, inp, "res", off=res_off).to(dt)
    if p["res"] == "up2":
        r = bilerp(r, p["H"], p["W"], dt, shift, clamp)
    return _aff(r, inp.get("rss") if rss else None, dt)


def _aa_pre(c, inp, dt, **kw):
    """-> (the value the activation decides on, the residual term)"""
    r = _aa_res(c, inp, dt, **{k: v for k, v in kw.items() if k in ("rss", "shift", "clamp", "res_off")})
    t = _aff(_sl(c, inp, "x", off=kw.get("x_off")).to(dt), inp.get("ss"), dt, row0=kw.get("row0", False))
    if r is not None and c.p.get("before"):
        t = t + r
    return t, r


def _aa_y(c, inp, dt, swap=False, scale_first=False, **kw):
    p = c.p
    before = bool(p.get("before")) != swap
    r = _aa_res(c, inp, dt, **{k: v for k, v in kw.items() if k in ("rss", "shift", "clamp", "res_off")})
    t = _aff(_sl(c, inp, "x", off=kw.get("x_off")).to(dt), inp.get("ss"), dt, row0=kw.get("row0", False))
    slope = float(inp["prelu"][0]) if "prelu" in inp else 0.0
    os_ = p.get("out_scale", 1.0)
    if r is None:
        return _act(t, p.get("act", 0), slope) * os_
    if before:
        return _act(t + r, p.get("act", 0), slope) * os_
    if scale_first:
        return _act(t, p.get("act", 0), slope) * os_ + r
    return (_act(t, p.get("act", 0), slope) + r) * os_


def _zero_last_pixel(y):
    y = y.clone()
    y[:, -1, -1] = 0
    return y


def _aa_defects(c, inp):
    """[(name, y)]: the defects of the apply pass (shared by affine_act, affine_act_stats)"""
    p = c.p
    f64 = torch.float64
    y = _aa_y(c, inp, f64)
    out = [("last pixel not written", _zero_last_pixel(y)), ("last channel zero", _zero_tail(y, 1))]
    if "res" in inp and p.get("act"):
        out.append(("residual on the wrong side of the activation", _aa_y(c, inp, f64, swap=True)))
    if "rss" in inp:
        out.append(("res_scale_shift ignored", _aa_y(c, inp, f64, rss=False)))
    if p.get("res") == "up2" and max(p["H"], p["W"]) > 2:            # (a 1 x 1 residual has one sample: nothing to shift or clamp)
        out.append(("up2 sample shifted by half a pixel", _aa_y(c, inp, f64, shift=True)))
        out.append(("up2 border not clamped", _aa_y(c, inp, f64, clamp=False)))
    if "ss" in inp and p["B"] > 1:
        out.append(("ss of batch row 0 used for every row", _aa_y(c, inp, f64, row0=True)))
    if p.get("x_off", 0):
        out.append(("slice offset ignored", _aa_y(c, inp, f64, x_off=0)))
    if p.get("res_off", 0):
        out.append(("slice offset of res ignored", _aa_y(c, inp, f64, res_off=0)))
    if p["C"] % 4:
        out.append(("tail channels zero", _zero_tail(y, p["C"] % 4)))
    if "res" in inp and not p.get("before") and p.get("out_scale", 1.0) != 1.0:
        out.append(("out_scale applied before the residual", _aa_y(c, inp, f64, scale_first=True)))
    return out


def _ptr_ok(c, names, st, half_items, f32_items):
    """every named tensor's ld and slice start a multiple of half_items (half tensors) / f32_items (fp32 tensors)"""
    for n, s in names:
        k = f32_items if s == "f32" else half_items
        if c.p.get(n + "_ld", c.p["C"]) % k or c.p.get(n + "_off", 0) % k:
            return False
    return True


def aa_form(c):
    p = c.p
    st, yst = p.get("st", "f32"), p.get("yst", p.get("st", "f32"))
    names = [("x", st), ("out", yst)] + ([("res", st)] if p.get("res") else [])
    half = st != "f32" or yst != "f32"
    # ld % 4 for every tensor; pointers: 16 bytes in an all-fp32 call (4 floats), 8 bytes with a half tensor (4 halves / 2 floats)
    vec = p["C"] % 4 == 0 and all(p.get(n + "_ld", p["C"]) % 4 == 0 for n, _ in names) and _ptr_ok(c, names, st, 4, 2 if half else 4)
    if not vec:
        return 1
    w8 = half and p["C"] % 8 == 0 and all(p.get(n + "_ld", p["C"]) % 8 == 0 for n, _ in names) and _ptr_ok(c, names, st, 8, 4)
    return 8 if w8 else 4


def _aa_branch(c):
    p = c.p
    return "affine_act:V%d:%s>%s" % (aa_form(c), p.get("st", "f32"), p.get("yst", p.get("st", "f32")))


OPS["affine_act"] = Spec(_aa_make, lambda c, inp, dt: {"y": _aa_y(c, inp, dt)}, _aa_branch,
                         lambda c, inp: [(n, {"y": y}) for n, y in _aa_defects(c, inp)], BAR_EW)
OUT_ST["affine_act"] = lambda c, n: c.p.get("yst", c.p.get("st", "f32"))
BORDER["affine_act"] = lambda c: c.p.get("res") == "up2"
_L, _P = ACT_LRELU, ACT_PRELU
# V = 1: C % 4 != 0, ld % 4 != 0, a pointer off the 16-byte grid
_case("affine_act", "V1-C3-plain", B=2, C=3, H=5, W=7)
_case("affine_act", "V1-C6-ss-lrelu-res-after", B=3, C=6, H=5, W=7, ss=True, act=_L, res="plain", out_scale=0.7)
_case("affine_act", "V1-C6-ss-prelu-res-before-rss", B=3, C=6, H=5, W=7, ss=True, act=_P, res="plain", rss=True, before=True)
_case("affine_act", "V1-C8-x-slice-ld14-off3", B=2, C=8, H=5, W=7, ss=True, act=_L, x_ld=14, x_off=3)
_case("affine_act", "V1-C8-out-slice-ld16-off2", B=2, C=8, H=5, W=7, ss=True, res="plain", res_ld=11, res_off=3, out_ld=16, out_off=2)
# V = 4, fp32
_case("affine_act", "V4-C4-plain", B=2, C=4, H=5, W=7)
_case("affine_act", "V4-C12-ss-lrelu", B=3, C=12, H=5, W=7, ss=True, act=_L, out_scale=1.3)
_case("affine_act", "V4-C8-ss-prelu-res-after-rss", B=3, C=8, H=6, W=5, ss=True, act=_P, res="plain", rss=True, out_scale=0.7)
_case("affine_act", "V4-C8-ss-lrelu-res-before", B=3, C=8, H=6, W=5, ss=True, act=_L, res="plain", before=True, out_scale=0.7)
_case("affine_act", "V4-C8-slices", B=2, C=8, H=6, W=5, ss=True, act=_L, res="plain", x_ld=16, x_off=4, res_ld=12, res_off=4, out_ld=20,
      out_off=8)
_case("affine_act", "V4-C4-up2-2x2", B=3, C=4, H=2, W=2, ss=True, res="up2", out_scale=0.7)                      # the smallest legal extent
_case("affine_act", "V4-C8-up2-2x6-rss-lrelu-before", B=2, C=8, H=2, W=6, ss=True, res="up2", rss=True, act=_L, before=True)
_case("affine_act", "V4-C8-up2-6x4-prelu-after-slices", B=2, C=8, H=6, W=4, ss=True, res="up2", act=_P, out_scale=0.7, res_ld=12, res_off=4,
      out_ld=16, out_off=4)
_case("affine_act", "V4-C64-20x24-ss-lrelu-res-after", B=2, C=64, H=20, W=24, ss=True, act=_L, res="plain", out_scale=1.0 / SQRT2)
# half storage: the six pairs at V = 4 (C % 8 != 0) and V = 8
for _st, _yst in (("f16", "f16"), ("f16", "f32"), ("f32", "f16"), ("bf16", "bf16"), ("bf16", "f32"), ("f32", "bf16")):
    _case("affine_act", "V4-C12-%s-%s-ss-lrelu-res-after" % (_st, _yst), B=3, C=12, H=5, W=7, st=_st, yst=_yst, ss=True, act=_L, res="plain",
          out_scale=0.7)
    _case("affine_act", "V8-C16-%s-%s-ss-prelu-res-before-rss" % (_st, _yst), B=3, C=16, H=5, W=7, st=_st, yst=_yst, ss=True, act=_P, res="plain",
          rss=True, before=True)
_case("affine_act", "V8-C8-f16-up2-2x2", B=3, C=8, H=2, W=2, st="f16", ss=True, res="up2", out_scale=0.7)
_case("affine_act", "V8-C8-bf16-up2-4x6-lrelu-before-slices", B=2, C=8, H=4, W=6, st="bf16", ss=True, res="up2", act=_L, before=True, x_ld=16,
      x_off=8, res_ld=24, res_off=16, out_ld=16, out_off=8)
_case("affine_act", "V4-C8-f16-slices-off4", B=2, C=8, H=5, W=7, st="f16", ss=True, act=_L, res="plain", x_ld=16, x_off=4, out_ld=12, out_off=4)
_case("affine_act", "V4-C8-f16-up2-6x4-rss", B=2, C=8, H=6, W=4, st="f16", yst="f32", ss=True, res="up2", rss=True, res_ld=12, res_off=4)


# ppst_affine_act_stats: chan_reduce_kernel<0, true, 4> only (C, every ld multiples of 4); the statistics are those of the OUTPUT
def _as_eval(c, inp, dt, y=None, drop=0, corner=4):
    y = _aa_y(c, inp, dt) if y is None else y.to(dt)
    s, q = _moments(y, dt, c.p.get("rep_pad"), drop, corner)
    return {"y": y, "sum": s, "sumsq": q}


def _as_mut(c, inp):
    hw = c.p["H"] * c.p["W"]
    out = [(n, _as_eval(c, inp, torch.float64, y=y)) for n, y in _aa_defects(c, inp)]
    out.append(("last pixel chunk dropped" if hw > pix_chunk(hw) else "last pixel dropped", _as_eval(c, inp, torch.float64, drop=_last_chunk(hw))))
    if c.p.get("rep_pad"):
        out.append(("rep_pad corner weight 2 instead of 4", _as_eval(c, inp, torch.float64, corner=2)))
    return out


def _as_facets(c):
    p = c.p
    return _reduce_facets("affine_act_stats:vec4", c, True, p["C"], p["H"] * p["W"]) + (["affine_act_stats:rep_pad"] if p.get("rep_pad") else [])


OPS["affine_act_stats"] = Spec(_aa_make, _as_eval, lambda c: "affine_act_stats:vec4", _as_mut,
                               lambda c, n: BAR_EW if n == "y" else _sum_bar(c.p["H"] * c.p["W"]))
BORDER["affine_act_stats"] = lambda c: False
_case("affine_act_stats", "C4-7x9-plain", B=3, C=4, H=7, W=9)
_case("affine_act_stats", "C12-13x11-ss-lrelu-rep_pad", B=3, C=12, H=13, W=11, ss=True, act=_L, rep_pad=True)
_case("affine_act_stats", "C8-12x10-ss-prelu-res-before-rss", B=3, C=8, H=12, W=10, ss=True, act=_P, res="plain", rss=True, before=True,
      out_scale=0.7)
_case("affine_act_stats", "C8-12x10-ss-lrelu-res-after-rep_pad", B=2, C=8, H=12, W=10, ss=True, act=_L, res="plain", rep_pad=True, out_scale=0.7)
_case("affine_act_stats", "C8-12x10-up2-rep_pad", B=2, C=8, H=12, W=10, ss=True, res="up2", rep_pad=True, out_scale=0.7)
_case("affine_act_stats", "C8-2x2-up2-lrelu-before", B=3, C=8, H=2, W=2, ss=True, res="up2", act=_L, before=True)
_case("affine_act_stats", "C8-slices", B=2, C=8, H=12, W=10, ss=True, act=_L, res="plain", x_ld=16, x_off=4, res_ld=12, res_off=4)
_case("affine_act_stats", "C4-96x96-ss", B=1, C=4, H=96, W=96, ss=True)                                # 144 partials


# ============================================================================ gap_gmp, gap_gmp_multi, gap_gmp_levels
# launcher (ppst_gap_gmp_st): a half tensor -> chan_reduce_kernel<1, false, 4, f16 | bf16> (C % 4, ld % 4, 8-byte x or refused);
# fp32: C % 4 == 0, ld % 4 == 0, 16-byte x -> chan_reduce_kernel<1, false, 4> else <1, false, 1>.  The mean divides by H W; the
# maximum is that of the products m x (a masked-out pixel counts as 0).
def _pool_x(c, g, shape, st):
    x = _randn(g, *shape)
    if c.p.get("allneg"):
        ch = c.p.get("x_off", 0) + 1
        x[..., ch] = -x[..., ch].abs() - 0.5           # every value of channel 1 negative: its maximum is < 0 unmasked, 0 under a mask
    return _store(x, st)


def _mask(c, g, *shape):
    kind = c.p.get("mask")
    if not kind:
        return None
    m = _mask_vals(g, *shape)
    m[:, -1, -1] = 1.0                                  # (the last pixel counts: a kernel that drops it shows)
    return (m > 0.25).float() if kind == "01" else m


def _last_kept(m):
    m[:, -1, -1] = 1.0
    return m


def pool_eval(x, mask, dt, drop=0, by_count=False, max_of_x=False):
    """-> (mean, max) of m x over the pixels, (B, C) each"""
    B, H, W, C = x.shape
    xf = x.to(dt).reshape(B, H * W, C)
    m = None if mask is None else mask.to(dt).reshape(B, H * W, 1)
    mx = xf if m is None else xf * m
    src = xf if max_of_x else mx
    if drop:
        mx, src = mx[:, :-drop], src[:, :-drop]
    den = m.sum(1).clamp_min(1.0) if by_count else float(H * W)
    return mx.sum(1) / den, src.max(1).values


def _gg_make(c):
    g = _gen(c)
    p = c.p
    inp = {"x": _pool_x(c, g, (p["B"], p["H"], p["W"], p.get("x_ld", p["C"])), p.get("st", "f32"))}
    m = _mask(c, g, p["B"], p["H"], p["W"])
    if m is not None:
        inp["mask"] = m
    return inp


def _gg_eval(c, inp, dt, x=None, **kw):
    mean, mx = pool_eval(_sl(c, inp, "x") if x is None else x, inp.get("mask"), dt, **kw)
    return {"mean": mean, "max": mx}


def _gg_branch(c):
    st = c.p.get("st", "f32")
    if st != "f32":
        return "gap_gmp:" + st
    return "gap_gmp:vec4" if _vec_ok(c, c.p["C"], "x") else "gap_gmp:scalar"


def _gg_facets(c):
    p = c.p
    br = _gg_branch(c)
    out = _reduce_facets(br, c, not br.endswith("scalar"), p["C"], p["H"] * p["W"])
    if p.get("mask"):
        out.append("gap_gmp:mask-" + p["mask"])
    if p.get("allneg"):
        out.append(br + (":all-negative-masked" if p.get("mask") else ":all-negative"))
    return out


def _pool_muts(ev, p, hw, vec, has_mask, C):
    """the defects of a pooled (mean, max) pair; ev(**kw) evaluates the case with the defect"""
    r = ev()
    out = [("last pixel chunk dropped" if hw > pix_chunk(hw) else "last pixel dropped", ev(drop=_last_chunk(hw))),
           ("last channel zero", {k: _zero_tail(v, 1) for k, v in r.items()})]
    if has_mask:
        out.append(("mean divided by the mask count", ev(by_count=True)))
        out.append(("max taken over x, not m x", ev(max_of_x=True)))
    t = _tail_channels(vec, C)
    if t:
        out.append(("tail channels zero", {k: _zero_tail(v, t) for k, v in r.items()}))
    return out


def _gg_mut(c, inp):
    p = c.p
    out = _pool_muts(lambda **kw: _gg_eval(c, inp, torch.float64, **kw), p, p["H"] * p["W"], not _gg_branch(c).endswith("scalar"), "mask" in inp,
                     p["C"])
    if p.get("x_off", 0):
        out.append(("slice offset ignored", _gg_eval(c, inp, torch.float64, x=_sl(c, inp, "x", off=0))))
    return out


def _pool_cls(hw):
    return lambda c, n: BAR_MOVE if n.startswith("max") else _sum_bar(hw(c))


OPS["gap_gmp"] = Spec(_gg_make, _gg_eval, _gg_branch, _gg_mut, _pool_cls(lambda c: c.p["H"] * c.p["W"]))
_case("gap_gmp", "scalar-C3-7x9", B=3, C=3, H=7, W=9, allneg=True)
_case("gap_gmp", "scalar-C3-13x11-mask01-allneg", B=3, C=3, H=13, W=11, mask="01", allneg=True)
_case("gap_gmp", "scalar-C258-5x5-maskfrac", B=2, C=258, H=5, W=5, mask="frac")
_case("gap_gmp", "scalar-C8-slice-ld16-off2-maskfrac-allneg", B=3, C=8, H=13, W=11, x_ld=16, x_off=2, mask="frac", allneg=True)
_case("gap_gmp", "vec4-C12-13x11", B=3, C=12, H=13, W=11, allneg=True)
_case("gap_gmp", "vec4-C12-13x11-mask01-allneg", B=3, C=12, H=13, W=11, mask="01", allneg=True)
_case("gap_gmp", "vec4-C64-16x16-maskfrac-allneg", B=3, C=64, H=16, W=16, mask="frac", allneg=True)
_case("gap_gmp", "vec4-C1028-5x5-mask01", B=2, C=1028, H=5, W=5, mask="01")
_case("gap_gmp", "vec4-C8-slice-ld16-off4-mask01", B=3, C=8, H=13, W=11, x_ld=16, x_off=4, mask="01")
_case("gap_gmp", "vec4-C4-96x96-maskfrac", B=1, C=4, H=96, W=96, mask="frac")
_case("gap_gmp", "scalar-C3-96x97", B=1, C=3, H=96, W=97)
_case("gap_gmp", "vec4-C4-1024x1024-chunk512-mask01", B=1, C=4, H=1024, W=1024, mask="01")
for _st in ("f16", "bf16"):
    _case("gap_gmp", "%s-C12-13x11-mask01-allneg" % _st, B=3, C=12, H=13, W=11, st=_st, mask="01", allneg=True)
    _case("gap_gmp", "%s-C8-slice-ld16-off4-maskfrac" % _st, B=3, C=8, H=7, W=9, st=_st, x_ld=16, x_off=4, mask="frac")
    _case("gap_gmp", "%s-C16-16x16" % _st, B=2, C=16, H=16, W=16, st=_st, allneg=True)


# ppst_gap_gmp_multi: one kernel (C % 4, ld % 4, aligned x or refused), heads = [plain] + one per mask channel, head-major rows
def _gm_make(c):
    g = _gen(c)
    p = c.p
    return {"x": _pool_x(c, g, (p["B"], p["H"], p["W"], p.get("x_ld", p["C"])), p.get("st", "f32")), "masks": _last_kept(_mask_vals(g, p["B"], p["H"], p["W"], p["nm"]))}


def _gm_heads(c, inp):
    return ([None] if c.p["plain"] else []) + [inp["masks"][..., i] for i in range(c.p["nm"])]


def _gm_eval(c, inp, dt, x=None, batch_major=False, **kw):
    x = _sl(c, inp, "x") if x is None else x
    rows = [pool_eval(x, m, dt, **(kw if m is not None else {k: v for k, v in kw.items() if k == "drop"})) for m in _gm_heads(c, inp)]
    mean, mx = torch.stack([r[0] for r in rows]), torch.stack([r[1] for r in rows])         # (heads, B, C)
    if batch_major:
        mean, mx = mean.transpose(0, 1), mx.transpose(0, 1)
    return {"mean": mean.reshape(-1, c.p["C"]), "max": mx.reshape(-1, c.p["C"])}


def _gm_mut(c, inp):
    p = c.p
    out = _pool_muts(lambda **kw: _gm_eval(c, inp, torch.float64, **kw), p, p["H"] * p["W"], True, True, p["C"])
    if p["B"] > 1 and p["nm"] + p["plain"] > 1:
        out.append(("rows written batch-major", _gm_eval(c, inp, torch.float64, batch_major=True)))
    if p.get("x_off", 0):
        out.append(("slice offset ignored", _gm_eval(c, inp, torch.float64, x=_sl(c, inp, "x", off=0))))
    return out


OPS["gap_gmp_multi"] = Spec(_gm_make, _gm_eval, lambda c: "gap_gmp_multi:" + c.p.get("st", "f32"), _gm_mut, _pool_cls(lambda c: c.p["H"] * c.p["W"]))
_case("gap_gmp_multi", "f32-nm3-plain-C12-13x11", B=3, C=12, H=13, W=11, nm=3, plain=True, allneg=True)
_case("gap_gmp_multi", "f32-nm1-noplain-C8-slice-ld16-off4", B=2, C=8, H=7, W=9, nm=1, plain=False, x_ld=16, x_off=4, allneg=True)
_case("gap_gmp_multi", "f32-nm2-plain-C1028-5x5", B=2, C=1028, H=5, W=5, nm=2, plain=True)
_case("gap_gmp_multi", "f16-nm3-noplain-C12-13x11", B=3, C=12, H=13, W=11, nm=3, plain=False, st="f16", allneg=True)
_case("gap_gmp_multi", "bf16-nm2-plain-C8-16x16", B=2, C=8, H=16, W=16, nm=2, plain=True, st="bf16", allneg=True)


# ppst_gap_gmp_multi_level: every level on the vector form (refuses the rest); ops sends more than GROUP_MAX maps GROUP_MAX at a time
def _gl_make(c):
    g = _gen(c)
    p = c.p
    inp = {}
    for i, (H, W, C, ld, off, masked) in enumerate(p["maps"]):
        x = _randn(g, p["B"], H, W, ld)
        x[..., off + 1] = -x[..., off + 1].abs() - 0.5
        inp["x%d" % i] = _store(x, p.get("st", "f32"))
        if masked:
            inp["mask%d" % i] = _last_kept(_mask_vals(g, p["B"], H, W))
    return inp


def _gl_x(c, inp, i, off=None):
    H, W, C, ld, o, _ = c.p["maps"][i]
    o = o if off is None else off
    return inp["x%d" % i][..., o:o + C]


def _gl_eval(c, inp, dt, off=None, swap=False, **kw):
    out = {}
    n = len(c.p["maps"])
    for i in range(n):
        j = (i + 12) % n if (swap and c.p["maps"][i][:3] == c.p["maps"][(i + 12) % n][:3]) else i      # (the extents repeat every 12 maps)
        m = inp.get("mask%d" % j)
        out["mean%d" % i], out["max%d" % i] = pool_eval(_gl_x(c, inp, j, off), m, dt, **(kw if m is not None else {k: v for k, v in kw.items() if k == "drop"}))
    return out


def _gl_mut(c, inp):
    out = [("last pixel dropped", _gl_eval(c, inp, torch.float64, drop=1)), ("mean divided by the mask count", _gl_eval(c, inp, torch.float64, by_count=True)),
           ("max taken over x, not m x", _gl_eval(c, inp, torch.float64, max_of_x=True))]
    if any(m[4] for m in c.p["maps"]):
        out.append(("slice offset ignored", _gl_eval(c, inp, torch.float64, off=0)))
    if len(c.p["maps"]) > GROUP_MAX:
        out.append(("maps of the second group exchanged", _gl_eval(c, inp, torch.float64, swap=True)))
    return out


def _gl_facets(c):
    n = len(c.p["maps"])
    return ["gap_gmp_levels:%s" % ("1-map" if n == 1 else ("2..GROUP_MAX-maps" if n <= GROUP_MAX else ">GROUP_MAX-maps"))]


OPS["gap_gmp_levels"] = Spec(_gl_make, _gl_eval, lambda c: "gap_gmp_levels:" + c.p.get("st", "f32"), _gl_mut, _pool_cls(lambda c: 64))
_case("gap_gmp_levels", "f32-1-map", B=2, maps=((13, 11, 12, 12, 0, True),))
_case("gap_gmp_levels", "f32-4-maps", B=3, maps=((16, 16, 8, 8, 0, True), (8, 8, 16, 16, 0, False), (13, 11, 12, 16, 4, True), (3, 5, 32, 32, 0, True)))
_case("gap_gmp_levels", "f16-4-maps", B=2, st="f16", maps=((16, 16, 8, 8, 0, True), (8, 8, 16, 16, 0, False), (13, 11, 12, 16, 4, True), (3, 5, 32, 32, 0, True)))
_case("gap_gmp_levels", "bf16-1-map", B=2, st="bf16", maps=((7, 9, 8, 16, 8, True),))
_case("gap_gmp_levels", "f32-35-maps", B=2, maps=tuple((3 + i % 4, 4 + i % 3, 4 * (1 + i % 3), 4 * (1 + i % 3), 0, i % 2 == 0) for i in range(GROUP_MAX + 3)))


# ========================================================================== avgpool, bilinear, maxpool2, upsample_nearest2
# one kernel each (C % 4 == 0 and every ld % 4 == 0 or refused; maxpool2 one channel per thread)
def _rs_make(c):
    p = c.p
    return {"x": _store(_wide(c, _gen(c), "x", p["B"], p["H"], p["W"]), p.get("st", "f32"))}


def _avg_mut(c, inp):
    f = c.p["f"]
    x = _sl(c, inp, "x").double()
    r = _pool(x, f)
    a = r.clone(); a[:, -1, -1] = 0
    out = [("last pixel not written", {"y": a})]
    if f > 1:
        out.append(("divided by f, not f f", {"y": r * f}))
        b = x.clone(); b[:, f - 1::f] = 0
        out.append(("last row of every window left out", {"y": _pool(b, f)}))
    else:
        out.append(("last channel zero", {"y": _zero_tail(r, 1)}))
    if c.p.get("x_off", 0):
        out.append(("slice offset ignored", {"y": _pool(_sl(c, inp, "x", off=0).double(), f)}))
    if c.p["H"] != c.p["W"]:
        t = x.transpose(1, 2).reshape(x.shape)                      # rows walked with the stride of the other extent
        out.append(("H and W exchanged in the row stride", {"y": _pool(t, f)}))
    return out


OPS["avgpool"] = Spec(_rs_make, lambda c, inp, dt: {"y": _pool(_sl(c, inp, "x").to(dt), c.p["f"])}, lambda c: "avgpool:f%d" % c.p["f"], _avg_mut, BAR_EW)
for _f in (1, 2, 4, 8):
    _case("avgpool", "f%d-C4-16x24" % _f, B=3, C=4, H=16, W=24, f=_f)
_case("avgpool", "f2-C12-6x10-slices", B=2, C=12, H=6, W=10, f=2, x_ld=16, x_off=4, out_ld=20, out_off=8)
_case("avgpool", "f4-C8-8x4", B=2, C=8, H=8, W=4, f=4)


def _bi_facets(c):
    def one(n, on):
        if on == n:
            return "identity"
        if on > n:
            return "up-by-%d" % (on // n) if on % n == 0 else "up-fractional"
        return "down-integer" if n % on == 0 else "down-fractional"
    p = c.p
    return sorted({"bilinear:" + one(p["H"], p["OH"]), "bilinear:" + one(p["W"], p["OW"])})


def _bi_mut(c, inp):
    p = c.p
    x = _sl(c, inp, "x")
    r = bilerp(x, p["OH"], p["OW"], torch.float64)
    out = [("last pixel not written", {"y": _zero_last_pixel(r)})]
    if (p["OH"], p["OW"]) != (p["H"], p["W"]):
        out.append(("sample shifted by half a pixel", {"y": bilerp(x, p["OH"], p["OW"], torch.float64, shift=True)}))
        if (p["OH"] > p["H"] > 1) or (p["OW"] > p["W"] > 1):
            out.append(("border not clamped", {"y": bilerp(x, p["OH"], p["OW"], torch.float64, clamp=False)}))
    else:
        out.append(("last channel zero", {"y": _zero_tail(r, 1)}))
    if p.get("x_off", 0):
        out.append(("slice offset ignored", {"y": bilerp(_sl(c, inp, "x", off=0), p["OH"], p["OW"], torch.float64)}))
    return out


OPS["bilinear"] = Spec(_rs_make, lambda c, inp, dt: {"y": bilerp(_sl(c, inp, "x"), c.p["OH"], c.p["OW"], dt)},
                       lambda c: "bilinear", _bi_mut, BAR_EW)
BORDER["bilinear"] = lambda c: True
for (_h, _w), (_oh, _ow) in (((5, 7), (10, 14)), ((3, 2), (24, 16)), ((5, 7), (12, 9)), ((12, 9), (5, 7)), ((16, 12), (4, 6)), ((6, 9), (6, 9)),
                             ((1, 6), (4, 6)), ((7, 5), (3, 10)), ((64, 48), (9, 64))):
    _case("bilinear", "C4-%dx%d-to-%dx%d" % (_h, _w, _oh, _ow), B=3, C=4, H=_h, W=_w, OH=_oh, OW=_ow)
_case("bilinear", "C8-5x7-to-12x9-slices", B=2, C=8, H=5, W=7, OH=12, OW=9, x_ld=16, x_off=4, out_ld=12, out_off=4)


def _mp(x):
    B, H, W, C = x.shape
    x = x[:, :H // 2 * 2, :W // 2 * 2]
    return torch.maximum(torch.maximum(x[:, 0::2, 0::2], x[:, 0::2, 1::2]), torch.maximum(x[:, 1::2, 0::2], x[:, 1::2, 1::2]))


def _mp_mut(c, inp):
    x = inp["x"].double()
    H, W = x.shape[1:3]
    out = [("the bottom row of every window left out", {"y": torch.maximum(x[:, 0:H // 2 * 2:2, 0:W // 2 * 2:2], x[:, 0:H // 2 * 2:2, 1:W // 2 * 2:2])}),
           ("last channel zero", {"y": _zero_tail(_mp(x), 1)})]
    if W % 2:
        # the row stride of the even extent: rows of W - 1 pixels
        flat = x.reshape(x.shape[0], H * W, -1)[:, :H * (W - 1)].reshape(x.shape[0], H, W - 1, -1)
        out.append(("rows walked with the even extent", {"y": _mp(flat)}))
    if H % 2 or W % 2:
        out.append(("windows anchored at the far edge", {"y": _mp(x[:, H % 2:, W % 2:])}))
    return out


OPS["maxpool2"] = Spec(_rs_make, lambda c, inp, dt: {"y": _mp(inp["x"].to(dt))}, lambda c: "maxpool2", _mp_mut, BAR_MOVE)
_case("maxpool2", "C3-7x9", B=3, C=3, H=7, W=9)
_case("maxpool2", "C8-6x5", B=2, C=8, H=6, W=5)
_case("maxpool2", "C5-5x8", B=2, C=5, H=5, W=8)
_case("maxpool2", "C4-8x8", B=2, C=4, H=8, W=8)


def _un(x, late=False):
    B, H, W, C = x.shape
    iy = (torch.arange(2 * H) + (1 if late else 0)).clamp_max(2 * H - 1) // 2
    ix = torch.arange(2 * W) // 2
    return x[:, iy][:, :, ix]


def _un_mut(c, inp):
    x = inp["x"].double()
    return [("source row taken one output row late", {"y": _un(x, late=True)}),
            ("columns doubled as rows", {"y": x.repeat_interleave(2, 2).repeat(1, 2, 1, 1)}), ("last channel zero", {"y": _zero_tail(_un(x), 1)})]


OPS["upsample_nearest2"] = Spec(_rs_make, lambda c, inp, dt: {"y": _un(inp["x"].to(dt))}, lambda c: "upsample_nearest2:" + c.p.get("st", "f32"), _un_mut,
                                BAR_MOVE)
OUT_ST["upsample_nearest2"] = lambda c, n: c.p.get("st", "f32")
_case("upsample_nearest2", "f32-C4-3x5", B=3, C=4, H=3, W=5)
_case("upsample_nearest2", "f32-C12-5x3", B=2, C=12, H=5, W=3)
_case("upsample_nearest2", "f16-C8-3x5", B=3, C=8, H=3, W=5, st="f16")
_case("upsample_nearest2", "bf16-C24-5x3", B=2, C=24, H=5, W=3, st="bf16")


# ============================================================================================================ head_tail
# one kernel; P in {2, 4, 8}, D in {1, 2}: feat = P x P mean of f = act(a x + s), feat1 = f (D = 1) or its 2 x 2 mean (D = 2: the
# bilinear resize by the exact factor 2)
def _ht_make(c):
    g = _gen(c)
    p = c.p
    inp = {"x": _wide(c, g, "x", p["B"], p["H"], p["W"]), "ss": _ss(g, p["B"], p["C"])}
    if p.get("act") == ACT_PRELU:
        inp["prelu"] = torch.tensor([0.25])
    if p.get("act"):
        _set_sl(c, inp, "x", _fix_gate(_sl(c, inp, "x").clone(), lambda x: _aff(x, inp["ss"], torch.float32), "f32"))
    return inp


def _ht_eval(c, inp, dt, off=None, row0=False, wrong_d=False):
    p = c.p
    f = _act(_aff(_sl(c, inp, "x", off=off).to(dt), inp["ss"], dt, row0), p.get("act", 0), float(inp["prelu"][0]) if "prelu" in inp else 0.0)
    if p["D"] == 1:
        f1 = _pool(f, 2).repeat_interleave(2, 1).repeat_interleave(2, 2) if wrong_d else f
    else:
        f1 = f[:, ::2, ::2] if wrong_d else _pool(f, 2)
    return {"feat": _pool(f, p["P"]), "feat1": f1}


def _ht_mut(c, inp):
    r = _ht_eval(c, inp, torch.float64)
    out = [("feat1 written at the wrong D", _ht_eval(c, inp, torch.float64, wrong_d=True)),
           ("last pixel not written", {k: _zero_last_pixel(v) for k, v in r.items()})]
    if c.p["B"] > 1:
        out.append(("ss of batch row 0 used for every row", _ht_eval(c, inp, torch.float64, row0=True)))
    if c.p.get("x_off", 0):
        out.append(("slice offset ignored", _ht_eval(c, inp, torch.float64, off=0)))
    return out


OPS["head_tail"] = Spec(_ht_make, _ht_eval, lambda c: "head_tail:P%d:D%d" % (c.p["P"], c.p["D"]), _ht_mut, BAR_EW)
BORDER["head_tail"] = lambda c: True
for _i, (_pp, _d) in enumerate(((2, 1), (2, 2), (4, 1), (4, 2), (8, 1), (8, 2))):
    _case("head_tail", "P%d-D%d-C%d" % (_pp, _d, (4, 12, 8)[_i % 3]), B=2 + _i % 2, C=(4, 12, 8)[_i % 3], H=2 * _pp, W=3 * _pp, P=_pp, D=_d,
          act=(ACT_NONE, ACT_LRELU, ACT_PRELU)[_i % 3])
_case("head_tail", "P4-D2-C8-slices-lrelu", B=2, C=8, H=12, W=8, P=4, D=2, act=_L, x_ld=16, x_off=4, feat_ld=12, feat_off=4, feat1_ld=16, feat1_off=8)
_case("head_tail", "P2-D1-C8-slices-prelu", B=3, C=8, H=6, W=4, P=2, D=1, act=_P, x_ld=12, x_off=4, feat_ld=16, feat_off=8, feat1_ld=12, feat1_off=4)


# ============================================================================================================ blur_nhwc
# launcher (ppst_blur_nhwc_st -> launch_chan<K, K, ST, CV>): CV = 8 for a half tensor with C % 8 == 0 and 3 x 3 taps, else 4
# (``off``: x starts that many elements into its buffer -- a half tensor off the 16-byte grid takes CV = 4, its items are 8 bytes);
# the sliding form for 4 x 4 taps, down == 1, a half tensor and eh >= 192 (eh: out_h, rounded up to even with s2d), else the
# patch form: templates <DOWN = 1, S2D>, <DOWN = 2>, <DOWN = 1>.  Taps: true convolution (the kernel is flipped).
def _bk(ks):
    """taps the networks' make_kernel([1, 2, 1] / [1, 3, 3, 1]) would give, made asymmetric: a flip or a transposition shows"""
    t = torch.tensor([1.0, 2.0, 1.0] if ks == 3 else [1.0, 3.0, 3.0, 1.0], dtype=torch.float64)
    k = t[:, None] * t[None, :] * (1.0 + 0.07 * torch.arange(ks * ks, dtype=torch.float64).reshape(ks, ks))
    return (k / k.sum()).float()


def blur_out_hw(p):
    ks, (p0, p1), down = p["ks"], p["pads"], p.get("down", 1)
    return (p["H"] + p0 + p1 - ks + down) // down, (p["W"] + p0 + p1 - ks + down) // down


def _bn_make(c):
    g = _gen(c)
    p = c.p
    st = p.get("st", "f32")
    inp = {"x": _store(_randn(g, p["B"], p["H"], p["W"], p["C"]), st), "k": _bk(p["ks"])}
    if p.get("in_ss"):
        inp["ss"] = _ss(g, p["B"], p["C"])
        if p["in_ss"] == "lrelu":
            inp["x"] = _fix_gate(inp["x"], lambda x: _aff(x, inp["ss"], torch.float32), st)
    return inp


def _bn_plain(c, inp, dt, pad_first=False, flip=False, row0=False, extra=0, mode=None):
    """(B, out_h, out_w, C) before the s2d stacking; extra: one more padded row and column at the far side"""
    p = c.p
    p0, p1 = p["pads"]
    mode = p.get("mode", 0) if mode is None else mode
    pads = (p0, p1 + extra, p0, p1 + extra)
    norm = lambda t: _act(_aff(t, inp.get("ss"), dt, row0), ACT_LRELU if p.get("in_ss") == "lrelu" else ACT_NONE)
    x = inp["x"].to(dt)
    xp = norm(_pad_fwd(x, pads, mode)) if pad_first else _pad_fwd(norm(x), pads, mode)
    k = inp["k"].to(dt)
    kf = k if flip else torch.flip(k, [0, 1])
    ks = p["ks"]
    oh, ow = xp.shape[1] - ks + 1, xp.shape[2] - ks + 1
    out = torch.zeros(x.shape[0], oh, ow, x.shape[3], dtype=dt)
    for ky in range(ks):
        for kx in range(ks):
            out = out + xp[:, ky:ky + oh, kx:kx + ow] * kf[ky, kx]
    d = p.get("down", 1)
    return out[:, ::d, ::d]


def _bn_eval(c, inp, dt, plain=None, **kw):
    y = _bn_plain(c, inp, dt, **kw) if plain is None else plain
    return {"y": _s2d_stack(y.contiguous()) if c.p.get("s2d") else y}


def blur_form(c):
    p = c.p
    st = p.get("st", "f32")
    cv = 8 if (st != "f32" and p["C"] % 8 == 0 and p["ks"] == 3 and (p.get("off", 0) * 2) % 16 == 0) else 4
    oh, ow = blur_out_hw(p)
    eh = (oh + 1) & ~1 if p.get("s2d") else oh
    slide = p["ks"] == 4 and p.get("down", 1) == 1 and st != "f32" and eh >= 192
    return cv, slide, eh, ((ow + 1) & ~1 if p.get("s2d") else ow)


def _bn_branch(c):
    p = c.p
    cv, slide, _, _ = blur_form(c)
    return "blur:k%d:%s:CV%d:%s:%s" % (p["ks"], p.get("st", "f32"), cv, "slide" if slide else "patch",
                                       "s2d" if p.get("s2d") else ("down2" if p.get("down", 1) == 2 else "plain"))


def _bn_facets(c):
    p = c.p
    cv, slide, eh, ew = blur_form(c)
    oh, ow = blur_out_hw(p)
    out = ["blur:pad-%s-%d-%d" % ("reflect" if p.get("mode") else "zero", p["pads"][0], p["pads"][1]), "blur:in_ss-%s" % (p.get("in_ss") or "none"),
           "blur:out_w%%4=%d" % (ow % 4)]
    if slide:
        out.append("blur:slide:last-band-%s" % ("partial" if eh % UF_SLIDE else "full"))
    if p.get("s2d"):
        out.append("blur:s2d:%s-rows-%s-columns" % ("odd" if oh % 2 else "even", "odd" if ow % 2 else "even"))
    if p["H"] < p["ks"] and p["W"] < p["ks"]:
        out.append("blur:input-smaller-than-the-taps")
    if cv == 4 and p.get("st", "f32") != "f32" and p["C"] % 8 == 0 and p["ks"] == 3:
        out.append("blur:CV4-by-pointer")
    return out


def _bn_mut(c, inp):
    p = c.p
    f64 = torch.float64
    _, slide, eh, ew = blur_form(c)
    oh, ow = blur_out_hw(p)
    r = _bn_plain(c, inp, f64)
    a = r.clone(); a[:, -1] = 0
    out = [("taps not flipped", _bn_eval(c, inp, f64, flip=True)), ("last row not written", _bn_eval(c, inp, f64, plain=a))]
    if p.get("in_ss") and not p.get("mode") and max(p["pads"]) > 0:
        out.append(("zero padding applied before normalise-on-load", _bn_eval(c, inp, f64, pad_first=True)))
    if p.get("s2d") and (oh % 2 or ow % 2) and (not p.get("mode") or p["pads"][1] + 1 < min(p["H"], p["W"])):
        ext = _bn_plain(c, inp, f64, extra=1)[:, :eh, :ew]
        out.append(("odd s2d row or column left non-zero", {"y": _s2d_stack(ext.contiguous())}))
    if slide and eh % UF_SLIDE:
        a = r.clone(); a[:, eh // UF_SLIDE * UF_SLIDE:] = 0
        out.append(("last sliding band's rows dropped", _bn_eval(c, inp, f64, plain=a)))
    if ew % 4:
        a = r.clone(); a[:, :, ew // 4 * 4:] = 0
        out.append(("last column strip dropped", _bn_eval(c, inp, f64, plain=a)))
    if p.get("mode") and max(p["pads"]) > 0:
        out.append(("reflect padding left zero", _bn_eval(c, inp, f64, mode=0)))
    if p.get("in_ss") and p["B"] > 1:
        out.append(("ss of batch row 0 used for every row", _bn_eval(c, inp, f64, row0=True)))
    return out


OPS["blur_nhwc"] = Spec(_bn_make, _bn_eval, _bn_branch, _bn_mut, BAR_EW)
OUT_ST["blur_nhwc"] = lambda c, n: c.p.get("st", "f32")
BORDER["blur_nhwc"] = lambda c: not c.p.get("s2d")        # (the stacked layout has no border rows of its own: see judge)
_Z, _R = 0, 1


def _bcase(name, **p):
    _case("blur_nhwc", name, **p)


# fp32, patch form: every template, pad pair, padding mode, normalise-on-load mode and ragged extent
_bcase("k4-zero-p21-s2d-f32-C4-13x11", B=2, C=4, H=13, W=11, ks=4, pads=(2, 1), mode=_Z, s2d=True)                       # 13 x 11 out: odd, odd
_bcase("k4-zero-p21-s2d-f32-C4-13x11-lrelu", B=2, C=4, H=13, W=11, ks=4, pads=(2, 1), mode=_Z, s2d=True, in_ss="lrelu")
_bcase("k4-reflect-p21-s2d-f32-C8-14x9-affine", B=2, C=8, H=14, W=9, ks=4, pads=(2, 1), mode=_R, s2d=True, in_ss="affine")
_bcase("k4-zero-p21-down2-f32-C4-13x10-lrelu", B=2, C=4, H=13, W=10, ks=4, pads=(2, 1), mode=_Z, down=2, in_ss="lrelu")
_bcase("k4-reflect-p11-down2-f32-C8-9x12", B=2, C=8, H=9, W=12, ks=4, pads=(1, 1), mode=_R, down=2)
_bcase("k4-zero-p11-plain-f32-C4-7x10-affine", B=2, C=4, H=7, W=10, ks=4, pads=(1, 1), mode=_Z, in_ss="affine")           # 6 x 9 out
_bcase("k4-reflect-p22-plain-f32-C12-9x6-lrelu", B=3, C=12, H=9, W=6, ks=4, pads=(2, 2), mode=_R, in_ss="lrelu")          # 10 x 7 out
_bcase("k4-zero-p10-plain-f32-C4-8x9", B=2, C=4, H=8, W=9, ks=4, pads=(1, 0), mode=_Z)                                   # 6 x 7 out
_bcase("k4-zero-p21-plain-f32-C4-2x3-affine", B=3, C=4, H=2, W=3, ks=4, pads=(2, 1), mode=_Z, in_ss="affine")             # smaller than one patch
_bcase("k4-zero-p21-s2d-f32-C4-2x3-lrelu", B=2, C=4, H=2, W=3, ks=4, pads=(2, 1), mode=_Z, s2d=True, in_ss="lrelu")
_bcase("k3-zero-p11-plain-f32-C4-5x5-affine", B=2, C=4, H=5, W=5, ks=3, pads=(1, 1), mode=_Z, in_ss="affine")
_bcase("k3-reflect-p11-plain-f32-C4-2x3-affine", B=3, C=4, H=2, W=3, ks=3, pads=(1, 1), mode=_R, in_ss="affine")
_bcase("k3-reflect-p11-down2-f32-C8-9x7", B=2, C=8, H=9, W=7, ks=3, pads=(1, 1), mode=_R, down=2)
_bcase("k3-zero-p21-s2d-f32-C4-6x7-lrelu", B=2, C=4, H=6, W=7, ks=3, pads=(2, 1), mode=_Z, s2d=True, in_ss="lrelu")       # 7 x 8 out
_bcase("k3-reflect-p22-s2d-f32-C4-5x6", B=2, C=4, H=5, W=6, ks=3, pads=(2, 2), mode=_R, s2d=True)                         # 7 x 8 out
_bcase("k3-zero-p10-down2-f32-C4-8x9-affine", B=2, C=4, H=8, W=9, ks=3, pads=(1, 0), mode=_Z, down=2, in_ss="affine")
# half storage, patch form: every (taps, type, CV, output) template
_VAR = (dict(pads=(2, 1), mode=_Z, in_ss="lrelu"), dict(pads=(1, 1), mode=_R, in_ss="affine"), dict(pads=(2, 2), mode=_Z), dict(pads=(1, 1), mode=_R, in_ss="lrelu"),
        dict(pads=(2, 1), mode=_R), dict(pads=(1, 0), mode=_Z, in_ss="affine"))
_n = 0
for _ks in (3, 4):
    for _st in ("f16", "bf16"):
        for _out in ("plain", "down2", "s2d"):
            for _C in (8, 12):
                _v = dict(_VAR[_n % len(_VAR)])
                _H, _W = ((9, 7), (7, 10), (13, 6))[_n % 3]
                _n += 1
                _bcase("k%d-%s-%s-C%d-%dx%d-%s-p%d%d-%s" % (_ks, _st, _out, _C, _H, _W, "reflect" if _v["mode"] else "zero", _v["pads"][0], _v["pads"][1],
                                                              _v.get("in_ss", "raw")),
                       B=2, C=_C, H=_H, W=_W, ks=_ks, st=_st, s2d=_out == "s2d", down=2 if _out == "down2" else 1, **_v)
_bcase("k3-f16-plain-C4-7x10-zero-p11", B=2, C=4, H=7, W=10, ks=3, st="f16", pads=(1, 1), mode=_Z)
_bcase("k3-bf16-s2d-C4-7x10-reflect-p21-affine", B=2, C=4, H=7, W=10, ks=3, st="bf16", pads=(2, 1), mode=_R, s2d=True, in_ss="affine")
# a half tensor 8 bytes into the 16-byte grid: the 4-channel form where the aligned tensor takes the 8-channel one
for _st in ("bf16", "f16"):
    _bcase("k3-%s-plain-C8-7x10-zero-p11-off4" % _st, B=2, C=8, H=7, W=10, ks=3, st=_st, pads=(1, 1), mode=_Z, off=4)
# the sliding form: eh in {192, 198, 209}, about 10 wide, C in {4, 12}
_bcase("k4-f16-slide-C4-192x10-zero-p21", B=2, C=4, H=192, W=10, ks=4, st="f16", pads=(2, 1), mode=_Z)                                  # 12 full bands
_bcase("k4-bf16-slide-C12-208x9-reflect-p22-lrelu", B=2, C=12, H=208, W=9, ks=4, st="bf16", pads=(2, 2), mode=_R, in_ss="lrelu")           # 209 x 10 out
_bcase("k4-f16-slide-s2d-C12-197x11-zero-p21-affine", B=2, C=12, H=197, W=11, ks=4, st="f16", pads=(2, 1), mode=_Z, s2d=True, in_ss="affine")  # eh 198
_bcase("k4-bf16-slide-s2d-C4-199x10-reflect-p11", B=1, C=4, H=199, W=10, ks=4, st="bf16", pads=(1, 1), mode=_R, s2d=True)                  # 198 x 9 out
_bcase("k4-bf16-slide-C4-209x11-zero-p21-lrelu", B=1, C=4, H=209, W=11, ks=4, st="bf16", pads=(2, 1), mode=_Z, in_ss="lrelu")               # 209 x 11 out
_bcase("k4-f16-patch-C4-191x10-zero-p21", B=1, C=4, H=191, W=10, ks=4, st="f16", pads=(2, 1), mode=_Z)                                   # eh 191: one below


# ================================================= conv1x1_small_cin / _small_cout, torgb_apply, spatial_modulation, lerp, u8
# ppst_conv1x1_small_cin_st: one kernel per output type (cin <= 4, cout % 4 == 0); the grid is rounded to a multiple of cout / 4
def _sci_make(c):
    g = _gen(c)
    p = c.p
    w, b = _randn(g, p["cout"], p["cin"], 1, 1), _randn(g, p["cout"])
    x = _wide(c, g, "x", p["B"], p["H"], p["W"], C=p["cin"])
    if p.get("act"):
        off = p.get("x_off", 0)
        for _ in range(40):
            t = torch.einsum("bhwi,oi->bhwo", x[..., off:off + p["cin"]], w.reshape(p["cout"], p["cin"])) * p["wscale"] + b
            bad = (t.abs() < 2e-3).any(-1)
            if not bad.any():
                break
            x[bad] = _randn(g, int(bad.sum()), x.shape[-1])
        assert not bad.any()
    return {"x": x, "w": w, "bias": b}


def _sci_eval(c, inp, dt, off=None, no_bias=False, cin=None):
    p = c.p
    cin = p["cin"] if cin is None else cin
    x = _sl(c, inp, "x", C=p["cin"], off=off).to(dt)[..., :cin]
    w = inp["w"].to(dt).reshape(p["cout"], p["cin"])[:, :cin]
    t = torch.einsum("bhwi,oi->bhwo", x, w) * p["wscale"]
    if p.get("bias", True) and not no_bias:
        t = t + inp["bias"].to(dt)
    return {"y": _act(t, p.get("act", 0))}


def _sci_mut(c, inp):
    r = _sci_eval(c, inp, torch.float64)["y"]
    out = [("last pixel not written", {"y": _zero_last_pixel(r)}), ("last four output channels zero", {"y": _zero_tail(r, 4)})]
    if c.p["cin"] > 1:
        out.append(("last input channel left out", _sci_eval(c, inp, torch.float64, cin=c.p["cin"] - 1)))
    if c.p.get("bias", True):
        out.append(("bias left out", _sci_eval(c, inp, torch.float64, no_bias=True)))
    if c.p.get("x_off", 0):
        out.append(("slice offset ignored", _sci_eval(c, inp, torch.float64, off=0)))
    return out


OPS["conv1x1_small_cin"] = Spec(_sci_make, _sci_eval, lambda c: "small_cin:" + c.p.get("yst", "f32"), _sci_mut, BAR_EW)
OUT_ST["conv1x1_small_cin"] = lambda c, n: c.p.get("yst", "f32")
for _cin, _co, _kw in ((1, 4, {}), (2, 32, dict(act=_L)), (3, 36, dict(act=_L)), (4, 32, dict(bias=False)), (3, 32, dict(x_ld=8, x_off=5, act=_L)),
                       (1, 36, dict(x_ld=4, x_off=3))):
    _case("conv1x1_small_cin", "cin%d-cout%d%s%s" % (_cin, _co, "-slice" if "x_ld" in _kw else "", "-lrelu" if _kw.get("act") else ""), B=2, H=7, W=9,
          cin=_cin, cout=_co, wscale=0.37, **_kw)
_case("conv1x1_small_cin", "cin3-cout32-f16-lrelu", B=2, H=7, W=9, cin=3, cout=32, wscale=0.37, act=_L, yst="f16")
_case("conv1x1_small_cin", "cin3-cout36-bf16-slice", B=2, H=7, W=9, cin=3, cout=36, wscale=0.37, yst="bf16", x_ld=4, x_off=1)


# ppst_conv1x1_small_cout_st: cout == 3 with aligned x, w -> conv1x1_cout3_kernel (8 pixels per half wave, the tail pixels clamped),
# else conv1x1_small_cout_kernel; 32 lanes stride the input channels by 128
def _sco_make(c):
    g = _gen(c)
    p = c.p
    return {"x": _store(_randn(g, 1, 1, p["npix"], p["cin"]), p.get("st", "f32")), "w": _randn(g, p["cout"], p["cin"], 1, 1), "bias": _randn(g, p["cout"])}


def _sco_eval(c, inp, dt, cin=None, no_bias=False):
    p = c.p
    cin = p["cin"] if cin is None else cin
    t = torch.einsum("bhwi,oi->bhwo", inp["x"].to(dt)[..., :cin], inp["w"].to(dt).reshape(p["cout"], p["cin"])[:, :cin]) * p["wscale"]
    return {"y": t if (no_bias or not p.get("bias", True)) else t + inp["bias"].to(dt)}


def _sco_mut(c, inp):
    p = c.p
    r = _sco_eval(c, inp, torch.float64)["y"]
    a = r.clone(); a[:, :, p["npix"] // 8 * 8 if p["npix"] % 8 else p["npix"] - 1:] = 0
    b = r.clone(); b[:, :, -1] = r[:, :, -2] if p["npix"] > 1 else 0
    out = [("pixels beyond the last group of 8 not written", {"y": a}), ("last pixel takes the one before it", {"y": b}),
           ("last four input channels left out", _sco_eval(c, inp, torch.float64, cin=p["cin"] - 4))]
    if p["cin"] > 128:
        out.append(("input channels from 128 on left out", _sco_eval(c, inp, torch.float64, cin=128)))
    if p.get("bias", True):
        out.append(("bias left out", _sco_eval(c, inp, torch.float64, no_bias=True)))
    return out


OPS["conv1x1_small_cout"] = Spec(_sco_make, _sco_eval, lambda c: "small_cout:%s:%s" % ("cout3" if c.p["cout"] == 3 else "generic", c.p.get("st", "f32")),
                                 _sco_mut, BAR_EW)
for _co, _cin, _np in ((1, 8, 67), (2, 64, 67), (4, 132, 67), (3, 8, 64), (3, 64, 67), (3, 132, 69), (3, 12, 3)):
    _case("conv1x1_small_cout", "cout%d-cin%d-npix%d" % (_co, _cin, _np), cout=_co, cin=_cin, npix=_np, wscale=0.21, bias=_np != 64)
for _st in ("f16", "bf16"):
    _case("conv1x1_small_cout", "cout3-cin64-npix67-%s" % _st, cout=3, cin=64, npix=67, wscale=0.21, st=_st)
    _case("conv1x1_small_cout", "cout2-cin12-npix67-%s" % _st, cout=2, cin=12, npix=67, wscale=0.21, st=_st)


# ppst_torgb_apply_st: conv1x1_cout3_apply_kernel per storage type; the input read as (a x + s + up2(res)) out_scale
def _tg_make(c):
    g = _gen(c)
    p = c.p
    st = p.get("st", "f32")
    inp = {"x": _store(_randn(g, p["B"], p["H"], p["W"], p["C"]), st), "ss": _ss(g, p["B"], p["C"]), "w": _randn(g, 3, p["C"], 1, 1), "bias": _randn(g, 3)}
    if p.get("res"):
        inp["res"] = _store(_wide(c, g, "res", p["B"], p["H"] // 2, p["W"] // 2), st)
    return inp


def _tg_eval(c, inp, dt, cin=None, **kw):
    p = c.p
    xe = _aa_y(c, inp, dt, **kw)
    cin = p["C"] if cin is None else cin
    return {"y": torch.einsum("bhwi,oi->bhwo", xe[..., :cin], inp["w"].to(dt).reshape(3, p["C"])[:, :cin]) * p["wscale"] + inp["bias"].to(dt)}


def _tg_mut(c, inp):
    p = c.p
    f64 = torch.float64
    r = _tg_eval(c, inp, f64)["y"]
    out = [("last pixel not written", {"y": _zero_last_pixel(r)}), ("last four input channels left out", _tg_eval(c, inp, f64, cin=p["C"] - 4)),
           ("ss of batch row 0 used for every row", _tg_eval(c, inp, f64, row0=True))]
    if p.get("res"):
        out.append(("out_scale applied before the residual", _tg_eval(c, inp, f64, scale_first=True)))
        if max(p["H"], p["W"]) > 2:
            out += [("up2 sample shifted by half a pixel", _tg_eval(c, inp, f64, shift=True)), ("up2 border not clamped", _tg_eval(c, inp, f64, clamp=False))]
        if p.get("res_off", 0):
            out.append(("slice offset of res ignored", _tg_eval(c, inp, f64, res_off=0)))
    return out


OPS["torgb_apply"] = Spec(_tg_make, _tg_eval, lambda c: "torgb_apply:" + c.p.get("st", "f32"), _tg_mut, BAR_EW)
for _st in ("f32", "f16", "bf16"):
    _case("torgb_apply", "%s-C8-6x10-res" % _st, B=3, C=8, H=6, W=10, st=_st, res="up2", out_scale=0.7, wscale=0.3)
    _case("torgb_apply", "%s-C132-3x7" % _st, B=2, C=132, H=3, W=7, st=_st, out_scale=1.3, wscale=0.09)
_case("torgb_apply", "f32-C16-2x2-res-slice", B=3, C=16, H=2, W=2, res="up2", out_scale=0.7, wscale=0.25, res_ld=24, res_off=8)


def _sm_make(c):
    g = _gen(c)
    p = c.p
    return {"x": _randn(g, p["B"], p["H"], p["W"], p["C"]), "scale": _randn(g, p["B"], p["C"]), "bias": _randn(g, p["B"], p["C"])}


def _sm_eval(c, inp, dt, row0=False):
    s, b = inp["scale"].to(dt), inp["bias"].to(dt)
    if row0:
        s, b = s[:1].expand_as(s), b[:1].expand_as(b)
    return {"y": inp["x"].to(dt) * s[:, None, None] + b[:, None, None]}


def _sm_mut(c, inp):
    r = _sm_eval(c, inp, torch.float64)["y"]
    return [("last pixel not written", {"y": _zero_last_pixel(r)}), ("scale and bias of batch row 0 used for every row", _sm_eval(c, inp, torch.float64, row0=True))]


OPS["spatial_modulation"] = Spec(_sm_make, _sm_eval, lambda c: "spatial_modulation:" + c.p.get("yst", "f32"), _sm_mut, BAR_EW)
OUT_ST["spatial_modulation"] = lambda c, n: c.p.get("yst", "f32")
for _st in ("f32", "f16", "bf16"):
    _case("spatial_modulation", "%s-C12-5x7" % _st, B=3, C=12, H=5, W=7, yst=_st)


def _lp_make(c):
    g = _gen(c)
    return {k: _randn(g, n) for i, n in enumerate(c.p["sizes"]) for k in ("a%d" % i, "b%d" % i)}


def _lp_eval(c, inp, dt, r=None, late=False):
    r = c.p["r"] if r is None else r
    n = len(c.p["sizes"])
    out = {}
    for i in range(n):
        j = (i + 3) % n if (late and c.p["sizes"][i] == c.p["sizes"][(i + 3) % n]) else i                # (the sizes repeat every 3 problems)
        out["y%d" % i] = inp["a%d" % j].to(dt) * (1.0 - r) + inp["b%d" % j].to(dt) * r
    return out


def _lp_mut(c, inp):
    r = _lp_eval(c, inp, torch.float64)
    out = [("a and b exchanged", _lp_eval(c, inp, torch.float64, r=1.0 - c.p["r"])), ("last element not written", {k: _zero_tail(v, 1) for k, v in r.items()})]
    if len(c.p["sizes"]) > GROUP_MAX:
        out.append(("problems of the second group exchanged", _lp_eval(c, inp, torch.float64, late=True)))
    return out


OPS["lerp"] = Spec(_lp_make, _lp_eval, lambda c: "lerp:%s" % ("single" if not c.p.get("grouped") else ("grouped" if len(c.p["sizes"]) <= GROUP_MAX else
                                                                                                   "grouped:>GROUP_MAX")), _lp_mut, BAR_EW)
_case("lerp", "single-n1", sizes=(1,), r=0.3)
_case("lerp", "single-n2053", sizes=(2053,), r=0.7)
_case("lerp", "grouped-4", sizes=(2048, 1, 300, 2053), r=0.3, grouped=True)
_case("lerp", "grouped-35", sizes=tuple(5 + 7 * (i % 3) for i in range(GROUP_MAX + 3)), r=0.6, grouped=True)


def tensor2im_ref(x):
    """util.tensor2im in its own arithmetic (float32, (x + 1) / 2 * 255, clip, truncate) -> (B, H, W, C)"""
    a = (np.transpose(x.numpy().astype(np.float32), (0, 2, 3, 1)) + np.float32(1)) / np.float32(2.0) * np.float32(255.0)
    return np.clip(a, 0, 255).astype(np.uint8)


def _u8_make(c):
    g = _gen(c)
    p = c.p
    x = _randn(g, p["B"], p["C"], p["H"], p["W"]) * 0.8
    flat = x.view(-1)
    flat[:6] = torch.tensor([-1.0, 1.0, 0.0, -1.5, 1.5, 1.0 - 2.0 ** -24])
    return {"x": x}


def _u8_eval(c, inp, dt):
    return {"y": torch.from_numpy(tensor2im_ref(inp["x"])).to(dt)}


def _u8_mut(c, inp):
    x = inp["x"]
    r = tensor2im_ref(x).astype(np.float64)
    rnd = np.clip(np.round((np.transpose(x.double().numpy(), (0, 2, 3, 1)) + 1) / 2 * 255), 0, 255)
    out = [("rounded, not truncated", {"y": torch.from_numpy(rnd)}), ("not clipped below", {"y": torch.from_numpy(np.where(r == 0, 255.0, r))})]
    if c.p["C"] > 1:
        out.append(("layout kept NCHW", {"y": torch.from_numpy(np.ascontiguousarray(r.transpose(0, 3, 1, 2)).reshape(r.shape))}))
    return out


OPS["tensor2im_u8"] = Spec(_u8_make, _u8_eval, lambda c: "tensor2im_u8", _u8_mut, BAR_MOVE)
_case("tensor2im_u8", "C3-7x9", B=2, C=3, H=7, W=9)
_case("tensor2im_u8", "C1-5x300", B=1, C=1, H=5, W=300)


# ================================================================================================= the table's machinery
_BY_ID = {c.id: c for c in CASES}
assert len(_BY_ID) == len(CASES), "case ids must be unique"
_FACETS = {"in_stats": _is_facets, "affine_act_stats": _as_facets, "gap_gmp": _gg_facets, "gap_gmp_levels": _gl_facets, "bilinear": _bi_facets,
           "blur_nhwc": _bn_facets}


def register(op, spec, cases, out_st=None, border=None, facets=None):
    """another table's op (tests/fir_cases.py) judged by this module's machinery: its cases resolve through ``by_id`` -- and so through
    ``inputs``, ``reference``, ``bar``, ``judge``, ``mutations`` -- without joining CASES, the table of tests/test_gpu_act.py"""
    assert op not in OPS and not any(c.id in _BY_ID for c in cases)
    OPS[op] = spec
    _BY_ID.update((c.id, c) for c in cases)
    if out_st is not None:
        OUT_ST[op] = out_st
    if border is not None:
        BORDER[op] = border
    if facets is not None:
        _FACETS[op] = facets


def by_id(cid):
    return _BY_ID[cid]


def branch_of(c):
    return OPS[c.op].branch(c)


def facets_of(c):
    return _FACETS[c.op](c) if c.op in _FACETS else []


def out_st(c, name):
    return OUT_ST[c.op](c, name) if c.op in OUT_ST else "f32"


@functools.lru_cache(maxsize=None)
def inputs(c_id):
    c = by_id(c_id)
    return OPS[c.op].make(c)


@functools.lru_cache(maxsize=None)
def reference(c_id):
    c = by_id(c_id)
    return {k: v.detach().numpy() for k, v in OPS[c.op].ref(c, inputs(c_id), torch.float64).items()}


def scale_of(c, name):
    return float(np.abs(reference(c.id)[name]).max())


@functools.lru_cache(maxsize=None)
def err32(c_id):
    """per output: error of the float32 evaluation of the reference against float64, relative to max|ref|"""
    c = by_id(c_id)
    r32, r64 = OPS[c.op].ref(c, inputs(c_id), torch.float32), reference(c_id)
    out = {}
    for k, v in r64.items():
        s = scale_of(c, k)
        out[k] = float(np.abs(r32[k].detach().double().numpy() - v).max() / (s if s > 0 else 1.0))
    return out


def bar(c, name):
    cls = OPS[c.op].cls(c, name) if callable(OPS[c.op].cls) else OPS[c.op].cls
    if cls == 0:
        return 0.0
    return max(cls, 4.0 * err32(c.id)[name])


def as_stored(c, name, arr):
    """a float64 result as the output tensor would hold it: rounded once to the output's storage type"""
    t = torch.from_numpy(np.asarray(arr, np.float64))
    return t.to(DTYPE[out_st(c, name)]).double().numpy()


def _edge(shape):
    e = np.zeros(shape, bool)
    e[[0, -1], :] = True
    e[:, [0, -1]] = True
    return e


def judge(c, name, got):
    """-> (violations, err) of one output of a case against its float64 reference, at the case's bar.  Half-stored outputs: the
    half formula (err in units of the allowed error); data movement: bit equality; the rest: ``compare``.  The border rows and
    columns of the spatial ops are judged again against their own scale."""
    ref, b, st = reference(c.id)[name], bar(c, name), out_st(c, name)
    got = np.asarray(got, np.float64)
    if b == 0 or st == "f32":
        cmp_ = lambda r, g, s=None: compare(r, g, b, s)
    else:
        cmp_ = lambda r, g, s=None: compare_half(r, g, b, st, s)
    bad, err = cmp_(ref, got)
    if b and c.op in BORDER and BORDER[c.op](c) and ref.ndim == 4:
        edge = _edge(ref.shape[1:3])
        bad2, err2 = cmp_(ref[:, edge], got[:, edge])
        bad = bad + ["border: " + m for m in bad2]
        err = max(err, err2)
    return bad, err


def mutations(c):
    return [(n, {k: v.detach().numpy() for k, v in o.items()}) for n, o in OPS[c.op].mutations(c, inputs(c.id))]


