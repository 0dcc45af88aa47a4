"""Cases, float64 references, seeded defects and bars of the tests of the two native ops (tests/test_fir_cases_cpu.py,
tests/test_gpu_fir.py): ``ppst_upfirdn2d`` of csrc/upfirdn2d.hip and ``ppst_fused_bias_act`` of csrc/fused_bias_act.hip -- the
drop-in contract of ppst_amd/stylegan2_op and, on the train step, the adjoint of every decimating blur (up 2, down 1) and every
activation gate of the backward pass (act 3, grad 1).  Plain torch / numpy on the CPU: nothing here touches the device, and the
device is never its own judge.

The conventions are those of tests/act_cases.py, whose machinery judges these cases too (``register``): ``Case``, ``Spec``, ``_gen``
seeded from the case id, ``compare``, ``half_allowed``, ``judge``, a bar of max(BAR_EW, 4 x the float32 evaluation of the same
reference).  What is particular here:

  references  ``upfirdn_ref`` is the definition in NHWC [major, H, W, minor]: zero-insert by (up_x, up_y), pad or crop with four
              independent pads, true convolution with the taps, keep every (down_x, down_y)-th sample.  ``fba_ref`` is
              f(x + b[(i / step_b) % size_b]) * scale with f chosen by act * 10 + grad; alpha and scale are rounded to float32
              first (they cross the ABI as C floats).  ``upfirdn_gather`` is the same operation seen from an output element (the
              shape a kernel has); the seeded defects that live inside the index arithmetic are wrong evaluations of it.
  storage     ``st`` in {f32, f16, bf16, f64}.  A half output is judged with ``half_allowed``; the GPU test also asks for bit
              equality with the fp32 launch on the widened input rounded once.  f64 is judged element by element with a bound
              that is derived, not measured: |got - ref| <= 2 (kh kw + 1) 2^-53 (|x| (*) |k|) for the FIR (both sides sum at
              most kh kw products in double, the device may contract them into fused multiply-adds), one rounding of the final
              product for the bias-activation.
  pointers    ``off``: x, y (and ref) start ``off`` elements into their buffers -- off the 16-byte grid the fp32 four-wide forms
              give way to the generic / scalar kernel; a half tensor on the 8-byte grid but off the 16-byte one keeps its four-wide
              form (its items are 8 bytes).
  inputs      taps are random with mixed sign (asymmetric under a flip and under a transposition); mode 30 keeps |x + b| >= 1e-3,
              mode 31 draws ``ref`` independently of x (about half of the signs disagree) with |ref| >= 1e-3.

``uf_form`` / ``fba_form`` restate the dispatchers' ``if``s; ``facets`` adds what a case reaches inside a form.  No element is left
out of any comparison.
"""
import math

import numpy as np
import torch

import act_cases as A
from act_cases import BAR_EW, Case, Spec, _fix_gate, _gen, _randn, _store, compare, half_allowed, judge as _judge  # noqa: F401

SQRT2 = math.sqrt(2.0)
TD = dict(A.DTYPE, f64=torch.float64)
ITEM = {"f32": 4, "f16": 2, "bf16": 2, "f64": 8}
UF_MAXK = 8
UF_SLIDE = A.UF_SLIDE
IDX32_MAX = 2 ** 31 - 1
UF_TRIP = 256 * 32 * 256          # work items of one grid-stride trip: generic (elements), up2 (groups of four channels)
FBA_TRIP = 256 * 16 * 256         # fused_bias_act (elements of the scalar form, groups of four of the vec form)
UNWRITTEN = 12345.0               # what an element a kernel never stores holds in the seeded defects (the GPU test fills with NaN)
BIG = 1 << 21                     # a quarter of this many output elements and a case is one of the second-trip cases

CASES = []


def _uf(cid, st="f32", M=2, C=1, k=(3, 3), up=(1, 1), down=(1, 1), pads=(0, 0, 0, 0), off=0, **p):
    CASES.append(Case("upfirdn2d", "upfirdn2d-" + cid, dict(p, st=st, M=M, C=C, k=k, up=up, down=down, pads=pads, off=off), 0))


def _fb(cid, shape, st="f32", bias=False, act=3, grad=0, alpha=0.2, scale=SQRT2, off=0):
    CASES.append(Case("fba", "fba-" + cid, dict(st=st, shape=shape, bias=bias, act=act, grad=grad, alpha=alpha, scale=scale, off=off), 0))


# ============================================================================================================ upfirdn2d
def uf_out_hw(p):
    (kh, kw), (ux, uy), (dx, dy), (px0, px1, py0, py1) = p["k"], p["up"], p["down"], p["pads"]
    return (p["H"] * uy + py0 + py1 - kh + dy) // dy, (p["W"] * ux + px0 + px1 - kw + dx) // dx


def upfirdn_ref(x, k, up, down, pads, dt=torch.float64):
    """the definition: [major, H, W, minor] -> [major, out_h, out_w, minor]"""
    (ux, uy), (dx, dy), (px0, px1, py0, py1) = up, down, pads
    x, k = x.to(dt), k.to(dt)
    M, H, W, C = x.shape
    kh, kw = k.shape
    z = x.new_zeros(M, H * uy, W * ux, C)                      # zero-insert
    z[:, ::uy, ::ux] = x
    ph, pw = H * uy + py0 + py1, W * ux + px0 + px1            # pad (> 0) or crop (< 0): canvas[Y][X] = z[Y - py0][X - px0]
    canvas = x.new_zeros(M, ph, pw, C)
    y0, y1, x0, x1 = max(py0, 0), min(ph, py0 + H * uy), max(px0, 0), min(pw, px0 + W * ux)
    if y1 > y0 and x1 > x0:
        canvas[:, y0:y1, x0:x1] = z[:, y0 - py0:y1 - py0, x0 - px0:x1 - px0]
    oh, ow = ph - kh + 1, pw - kw + 1
    kf = torch.flip(k, [0, 1])                                 # true convolution
    out = x.new_zeros(M, oh, ow, C)
    for ky in range(kh):
        for kx in range(kw):
            out = out + canvas[:, ky:ky + oh, kx:kx + ow] * kf[ky, kx]
    return out[:, ::dy, ::dx]                                  # decimate


def upfirdn_gather(x, k, up, down, pads, out_hw, dt=torch.float64, flip=True, phase=0, first=0):
    """the same operation from the output's side: out[oy][ox] = sum over the taps whose upsampled coordinate
    Y = oy down_y + ky - pad_y0 is a multiple of up_y inside the input.  flip / phase / first: seeded defects (taps read
    unflipped; the zero-insert puts sample i at i up + phase; the decimation keeps samples first, first + down, ...)."""
    (ux, uy), (dx, dy), (px0, _, py0, _) = up, down, pads
    x, k = x.to(dt), k.to(dt)
    M, H, W, C = x.shape
    kh, kw = k.shape
    oh, ow = out_hw
    out = x.new_zeros(M, oh, ow, C)
    oy, ox = torch.arange(oh), torch.arange(ow)
    for ky in range(kh):
        Y = oy * dy + first + ky - py0 - phase
        vy = (Y >= 0) & (Y % uy == 0) & (Y // uy < H)
        iy = (Y // uy).clamp(0, H - 1)
        for kx in range(kw):
            X = ox * dx + first + kx - px0 - phase
            vx = (X >= 0) & (X % ux == 0) & (X // ux < W)
            ix = (X // ux).clamp(0, W - 1)
            f = k[kh - 1 - ky, kw - 1 - kx] if flip else k[ky, kx]
            out = out + x[:, iy][:, :, ix] * (vy[:, None] & vx[None, :]).to(dt)[None, :, :, None] * f
    return out


def _uf_make(c):
    g = _gen(c)
    p = c.p
    shape = (p["M"], p["H"], p["W"], p["C"])
    if p["st"] == "f64":
        return {"x": torch.randn(*shape, generator=g, dtype=torch.float64), "k": torch.randn(*p["k"], generator=g, dtype=torch.float64)}
    x, k = _store(_randn(g, *shape), p["st"]), _randn(g, *p["k"])
    if k.numel() > 1 and (bool((k > 0).all()) or bool((k < 0).all())):
        k.view(-1)[0].neg_()                                   # (mixed sign also where there are two taps)
    return {"x": x, "k": k}


def _uf_eval(c, inp, dt):
    return {"y": upfirdn_ref(inp["x"], inp["k"], c.p["up"], c.p["down"], c.p["pads"], dt)}


def _aligned(p, grid):
    return (p["off"] * ITEM[p["st"]]) % grid == 0


def uf_form(c):
    """the dispatcher of ppst_upfirdn2d, restated"""
    p = c.p
    st, C, (kh, kw), up, down = p["st"], p["C"], p["k"], p["up"], p["down"]
    if st == "f64":
        return "f64:generic"
    oh, ow = uf_out_hw(p)
    fast = up == (1, 1) and down == (1, 1) and (C == 1 or C % 4 == 0) and kh == kw
    down2 = up == (1, 1) and down == (2, 2) and C % 4 == 0 and kh == kw
    al16 = st != "f32" or _aligned(p, 16)                      # (a half pointer off the 8-byte grid is refused: no case has one)
    if C != 1 and not al16:
        fast = down2 = False
    if fast and kh in (3, 4):
        if C == 1:
            return "planes:k%d:%s" % (kh, st)
        if kh == 4 and st != "f32" and oh >= 192:
            return "chan:k4:slide:%s" % st
        return "chan:k%d:plain:%s" % (kh, st)
    if down2 and kh in (3, 4):
        return "chan:k%d:down2:%s" % (kh, st)
    if up == (2, 2) and down == (1, 1) and C % 4 == 0 and p["M"] * oh * ow * C // 4 <= IDX32_MAX and al16:
        return "up2_chan:%s" % st
    return "generic:%s" % st


def _uf_facets(c):
    p = c.p
    form = uf_form(c)
    (kh, kw), (ux, uy), (dx, dy), (px0, px1, py0, py1), C = p["k"], p["up"], p["down"], p["pads"], p["C"]
    oh, ow = uf_out_hw(p)
    n = p["M"] * oh * ow * C
    out = []
    neg0, neg1 = px0 < 0 or py0 < 0, px1 < 0 or py1 < 0
    if neg0 or neg1:
        out.append("pad:both<0" if (neg0 and neg1) else ("pad:pad0<0" if neg0 else "pad:pad1<0"))
    if (px0, px1) != (py0, py1):
        out.append("pad:px!=py")
    if p["M"] == 1:
        out.append("major=1")
    if p["st"] in ("f16", "bf16") and not _aligned(p, 16):
        out.append("half:on-8-off-16-byte-grid")
    if form.startswith("generic"):
        if kh != kw:
            out.append("generic:kh!=kw")
        out += ["generic:taps-%d" % t for t in sorted({kh, kw} & {1, 2, 5, 8})]
        if (ux, uy) == (2, 2) and C == 1:
            out.append("generic:up2-minor1")
        if ux != uy:
            out.append("generic:up_x!=up_y")
        if 3 in (dx, dy):
            out.append("generic:down3")
        if dx != dy:
            out.append("generic:down_x!=down_y")
        if C == 6:
            out.append("generic:minor6")
        if p["st"] == "f32" and C % 4 == 0 and not _aligned(p, 16) and kh == kw:
            if (ux, uy, dx, dy) == (2, 2, 1, 1):
                out.append("generic:up2-off-grid")
            elif (ux, uy) == (1, 1) and (dx, dy) in ((1, 1), (2, 2)) and kh in (3, 4):
                out.append("generic:%s-off-grid" % ("blur" if dx == 1 else "down2"))
        if n > UF_TRIP:
            out.append("generic:second-trip")
    elif form.startswith("planes"):
        if (oh, ow) == (1, 1):
            out.append("planes:1x1-out")
        elif (oh, ow) == (32, 64):
            out.append("planes:32x64-exact")
        elif oh <= 32 and ow <= 64:
            out.append("planes:one-tile")
        if oh > 32 and ow > 64:
            out.append("planes:33x65-seams" if (oh, ow) == (33, 65) else "planes:seams")
        if p["H"] < kh and p["W"] < kw:
            out.append("planes:input-smaller-than-the-taps")
    elif form.startswith("up2_chan"):
        if p["H"] % 2 or p["W"] % 2:
            out.append("up2:odd-in")
        if not (p["H"] % 2 and p["W"] % 2):
            out.append("up2:even-in")
        if p.get("adj"):
            out.append("up2:adjoint-k%d-p%d%d" % p["adj"][:3])
        if n // 4 > UF_TRIP:
            out.append("up2:second-trip")
    elif ":slide:" in form:
        out.append("slide:last-band-%s" % ("partial" if oh % UF_SLIDE else "full"))
    return out


def _uf_mut(c, inp):
    p = c.p
    f64 = torch.float64
    form = uf_form(c)
    (kh, kw), up, down, pads = p["k"], p["up"], p["down"], p["pads"]
    ohw = uf_out_hw(p)
    r = torch.from_numpy(A.reference(c.id)["y"])
    a = r.clone(); a[:, -1] = UNWRITTEN
    b = r.clone(); b[:, :, -1] = UNWRITTEN
    out = [("last row not written", a), ("last column not written", b)]
    if is_big(c):                                              # the two second-trip cases: the defects of the trip alone
        a = r.clone()
        a.view(-1)[(4 if form.startswith("up2") else 1) * UF_TRIP:] = 0
        return [(n, {"y": v}) for n, v in out + [("second-trip elements left zero", a)]]
    x, k = inp["x"], inp["k"]
    ev = lambda **kw_: upfirdn_gather(x, kw_.pop("k", k), kw_.pop("up", up), down, kw_.pop("pads", pads), ohw, f64, **kw_)
    if kh * kw > 1:
        out.append(("taps not flipped", ev(flip=False)))
    if kh == kw and kh > 1:
        out.append(("taps transposed", ev(k=k.t())))
    if pads[0] != pads[2]:
        out.append(("px and py exchanged", ev(pads=(pads[2], pads[3], pads[0], pads[1]))))
    if up[0] != up[1]:
        out.append(("up_x and up_y exchanged", ev(up=(up[1], up[0]))))
    if pads[0] < 0 or pads[2] < 0:
        out.append(("a crop treated as zero padding", ev(pads=(max(pads[0], 0), pads[1], max(pads[2], 0), pads[3]))))
    if max(up) > 1:
        out.append(("zero-insert phase off by one", ev(phase=1)))
    if max(down) > 1:
        out.append(("decimation starting at sample 1", ev(first=1)))
    if form.startswith("planes"):
        if ohw[0] > 32:
            a = r.clone(); a[:, 32] = r[:, 31]
            out.append(("the row after a 32-row seam taken from the row above", a))
        if ohw[1] > 64:
            a = r.clone(); a[:, :, 64] = r[:, :, 63]
            out.append(("the column after a 64-column seam taken from the column before", a))
    if ":slide:" in form:
        a = r.clone(); a[:, (ohw[0] - 1) // UF_SLIDE * UF_SLIDE:] = 0
        out.append(("last sliding band dropped", a))
    return [(n, {"y": v}) for n, v in out]


def _adj(ks, p0, p1, H, W):
    """the up-2 launch BlurDownFn.backward emits for a forward blur (ks taps, zero pads (p0, p1), every second sample) of an H x W map"""
    oh, ow = (H + p0 + p1 - ks + 2) // 2, (W + p0 + p1 - ks + 2) // 2
    g0 = ks - p0 - 1
    return dict(H=oh, W=ow, k=(ks, ks), up=(2, 2), pads=(g0, W - 2 * ow + p0, g0, H - 2 * oh + p0), adj=(ks, p0, p1, H, W))


# f64: one kernel, the generic form
_uf("f64-k4-up2-C1-5x7-p21", st="f64", H=5, W=7, k=(4, 4), up=(2, 2), pads=(2, 1, 2, 1))
_uf("f64-k5x3-down2x3-C3-9x11-crop", st="f64", H=9, W=11, C=3, k=(5, 3), down=(2, 3), pads=(1, -1, -1, 2))
_uf("f64-k3-blur-C4-7x6-p11", st="f64", H=7, W=6, C=4, pads=(1, 1, 1, 1))
# planes (minor 1, up = down = 1, 3 x 3 / 4 x 4): 32 x 64 output tiles
for _st in ("f32", "f16", "bf16"):
    _uf("planes-k3-%s-33x65-p11" % _st, st=_st, H=33, W=65, pads=(1, 1, 1, 1))                 # a seam in both directions, last tile 1 x 1
    _uf("planes-k4-%s-33x65-p21" % _st, st=_st, H=33, W=65, k=(4, 4), pads=(2, 1, 2, 1))
_uf("planes-k3-f32-one-tile-7x9-p11", M=3, H=7, W=9, pads=(1, 1, 1, 1))
_uf("planes-k4-f32-32x64-exact-p12", H=32, W=64, k=(4, 4), pads=(1, 2, 1, 2))
_uf("planes-k3-f32-1x1-out", H=3, W=3)
_uf("planes-k4-f32-2x3-smaller-than-the-taps", H=2, W=3, k=(4, 4), pads=(2, 1, 2, 1))
_uf("planes-k3-f32-crop-both-9x11", H=9, W=11, pads=(-1, -1, -1, -1))                           # the golden vector's pad pair
_uf("planes-k4-f32-crop-pad0-40x70", H=40, W=70, k=(4, 4), pads=(-1, 2, -2, 3))                 # 38 x 68 out: seams under a crop
_uf("planes-k3-f32-crop-pad1-9x11", H=9, W=11, pads=(1, -1, 2, -2))
_uf("planes-k3-f32-pxpy-major1-8x10", M=1, H=8, W=10, pads=(2, 0, 0, 2))
_uf("planes-k4-f16-crop-both-9x11", st="f16", H=9, W=11, k=(4, 4), pads=(-1, -1, -1, -1))
_uf("planes-k3-bf16-one-tile-7x9-p20", st="bf16", M=3, H=7, W=9, pads=(2, 0, 2, 0))
# chan (minor % 4 == 0): the patch form, plain and every second sample, every type
_PV = ((1, 1, 1, 1), (2, 1, 2, 1), (-1, 2, 1, -1), (0, 2, 2, 0))
_n = 0
for _st in ("f32", "f16", "bf16"):
    for _ks in (3, 4):
        for _dn in (1, 2):
            _H, _W = ((7, 10), (9, 6), (6, 11))[_n % 3]
            _uf("chan-k%d-%s-%s-C%d-%dx%d-p%s" % (_ks, "plain" if _dn == 1 else "down2", _st, (4, 8, 12)[_n % 3], _H, _W, "".join(map(str, _PV[_n % 4]))),
                st=_st, H=_H, W=_W, C=(4, 8, 12)[_n % 3], k=(_ks, _ks), down=(_dn, _dn), pads=_PV[_n % 4])
            _n += 1
_uf("chan-k4-plain-f32-C4-192x6-p21", H=192, W=6, C=4, k=(4, 4), pads=(2, 1, 2, 1))            # fp32 never slides
_uf("chan-k4-plain-f16-C4-191x6-p21", st="f16", M=1, H=191, W=6, C=4, k=(4, 4), pads=(2, 1, 2, 1))   # one row below the threshold
# half tensors on the 8-byte grid, off the 16-byte one: the same forms (an fp32 tensor there goes to the generic kernel)
_uf("chan-k3-plain-bf16-C8-7x10-p1111-off4", st="bf16", H=7, W=10, C=8, pads=(1, 1, 1, 1), off=4)
_uf("chan-k4-down2-f16-C4-9x6-p1111-off4", st="f16", H=9, W=6, C=4, k=(4, 4), down=(2, 2), pads=(1, 1, 1, 1), off=4)
_uf("up2-k4-bf16-C4-4x6-p2121-off4", st="bf16", H=4, W=6, C=4, k=(4, 4), up=(2, 2), pads=(2, 1, 2, 1), off=4)
# the sliding form reached through ppst_upfirdn2d: 4 x 4 taps, half storage, >= 192 output rows
_uf("slide-k4-f16-C4-192x6-p21", st="f16", H=192, W=6, C=4, k=(4, 4), pads=(2, 1, 2, 1))       # 12 full bands
_uf("slide-k4-bf16-C8-205x5-p12", st="bf16", H=205, W=5, C=8, k=(4, 4), pads=(1, 2, 1, 2))      # 205 rows: the last band has 13
_uf("slide-k4-bf16-C4-193x5-crop", st="bf16", M=1, H=193, W=5, C=4, k=(4, 4), pads=(2, 1, -1, 3))       # 192 rows under a crop
_uf("slide-k4-f16-C4-201x7-p21", st="f16", M=1, H=201, W=7, C=4, k=(4, 4), pads=(2, 1, 2, 1))
# up2 (minor % 4 == 0, up 2, down 1): the adjoint of the decimating blur
_n = 0
for _ks, _p0, _p1 in ((3, 1, 0), (4, 1, 1), (4, 2, 1), (4, 2, 2)):
    for _H, _W in ((8, 9), (9, 8)):
        _st = ("f32", "f16", "bf16")[_n % 3]
        _n += 1
        _uf("up2-adjoint-k%d-p%d%d-of-%dx%d-%s" % (_ks, _p0, _p1, _H, _W, _st), st=_st, C=4, **_adj(_ks, _p0, _p1, _H, _W))
_uf("up2-k3-f32-C4-5x7-p11", H=5, W=7, C=4, up=(2, 2), pads=(1, 1, 1, 1))
_uf("up2-k4-f16-C8-4x6-p21", st="f16", H=4, W=6, C=8, k=(4, 4), up=(2, 2), pads=(2, 1, 2, 1))
_uf("up2-k2-bf16-C4-3x4-p10-major1", st="bf16", M=1, H=3, W=4, C=4, k=(2, 2), up=(2, 2), pads=(1, 0, 1, 0))
_uf("up2-k5x3-f32-C8-5x6-crop", H=5, W=6, C=8, k=(5, 3), up=(2, 2), pads=(-1, 2, 3, -2))
_uf("up2-k2-f32-C4-724x724-second-trip", M=1, H=724, W=724, C=4, k=(2, 2), up=(2, 2), pads=(1, 1, 1, 0))   # 1448 x 1449 x 4: 33.6 MB
# generic, each with the reason it was chosen
_uf("generic-f32-k5x3-C1-9x11-p21", H=9, W=11, k=(5, 3), pads=(2, 1, 2, 1))                     # kh != kw
_uf("generic-f32-k1-C1-5x7", H=5, W=7, k=(1, 1))                                               # one tap
_uf("generic-f32-k2-C1-5x7-p10", H=5, W=7, k=(2, 2), pads=(1, 0, 1, 0))                        # square, but neither 3 nor 4
_uf("generic-f32-k8-C2-9x10-p43", H=9, W=10, C=2, k=(8, 8), pads=(4, 3, 4, 3))                  # the largest taps
_uf("generic-f32-k4-up2-C1-6x5-p21", H=6, W=5, k=(4, 4), up=(2, 2), pads=(2, 1, 2, 1))          # the public NCHW op's up = 2
_uf("generic-f32-k3-up2x3-C1-5x6", H=5, W=6, up=(2, 3), pads=(1, 1, 2, 0))                      # up_x != up_y
_uf("generic-f32-k4-down3-C1-13x11-p21", H=13, W=11, k=(4, 4), down=(3, 3), pads=(2, 1, 2, 1))
_uf("generic-f32-k3-down1x2-C4-9x8-p11", H=9, W=8, C=4, down=(1, 2), pads=(1, 1, 1, 1))         # down_x != down_y
_uf("generic-f32-k3-C6-7x9-p11", H=7, W=9, C=6, pads=(1, 1, 1, 1))                              # minor neither 1 nor a multiple of 4
_uf("generic-f32-k4-down2-C1-9x12-p11", H=9, W=12, k=(4, 4), down=(2, 2), pads=(1, 1, 1, 1))    # the public NCHW op's down = 2
_uf("generic-f32-k3-up3-down2-C3-7x5-crop", H=7, W=5, C=3, up=(3, 3), down=(2, 2), pads=(-2, 1, -1, -1))
_uf("generic-f32-k4-up2-C4-4x5-off1", H=4, W=5, C=4, k=(4, 4), up=(2, 2), pads=(2, 1, 2, 1), off=1)   # the up-2 geometry off the 16-byte grid
_uf("generic-f32-k3-blur-C4-7x10-off1", H=7, W=10, C=4, pads=(1, 1, 1, 1), off=1)               # the chan forms' geometry off the grid
_uf("generic-f32-k4-down2-C8-9x6-off1", H=9, W=6, C=8, k=(4, 4), down=(2, 2), pads=(1, 1, 1, 1), off=1)
for _st in ("f16", "bf16"):
    _uf("generic-%s-k5x3-up2x1-down1x3-C6-7x9" % _st, st=_st, H=7, W=9, C=6, k=(5, 3), up=(2, 1), down=(1, 3), pads=(1, 1, 2, 2))
    _uf("generic-%s-k4-up2-C1-6x5-p21" % _st, st=_st, H=6, W=5, k=(4, 4), up=(2, 2), pads=(2, 1, 2, 1))
    _uf("generic-%s-k3-down3-C2-11x13-crop" % _st, st=_st, H=11, W=13, C=2, down=(3, 3), pads=(-1, 2, 1, -1))
_uf("generic-f32-k2x1-C1-1025x2050-second-trip", M=1, H=1025, W=2050, k=(2, 1))                 # 1024 x 2050: 8.4 MB


# ====================================================================================================== fused_bias_act
def fba_geom(p):
    shape = p["shape"]
    return int(np.prod(shape)), int(np.prod(shape[2:])), shape[1]          # n, step_b, size_b (ops.fused_bias_act_raw)


def fba_ref(x, b, ref, mode, alpha, scale, step_b, dt=torch.float64, abi=True, gate_x=False, no_div=False, group0=False, scale_first=False,
            zero_modes_x=False):
    """f(x + b[(i / step_b) % size_b]) * scale; abi: alpha and scale as the C floats they cross the ABI as.  The other flags: defects."""
    if abi:
        alpha, scale = float(np.float32(alpha)), float(np.float32(scale))
    a, s = torch.tensor(alpha, dtype=dt), torch.tensor(scale, dtype=dt)
    v = x.to(dt).reshape(-1)
    if b is not None:
        i = torch.arange(v.numel())
        if group0:
            i = i // 4 * 4
        v = v + b.to(dt)[(i if no_div else i // step_b) % b.numel()]
    if scale_first:
        v = v * s
    if mode == 30:
        o = torch.where(v > 0, v, v * a)
    elif mode == 31:
        o = torch.where((v if gate_x else ref.to(dt).reshape(-1)) > 0, v, v * a)
    elif mode in (12, 32):
        o = v if zero_modes_x else torch.zeros_like(v)
    else:
        o = v
    return (o if scale_first else o * s).reshape(x.shape)


def fba_mode(p):
    return p["act"] * 10 + p["grad"]


def _fb_make(c):
    g = _gen(c)
    p = c.p
    n, step_b, size_b = fba_geom(p)
    st = p["st"]
    if st == "f64":
        rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
        store = lambda t: t
    else:
        rn = lambda *s: _randn(g, *s)
        store = lambda t: _store(t, st)
    inp = {"x": store(rn(*p["shape"]))}
    if p["bias"]:
        inp["b"] = store(rn(size_b))
    if fba_mode(p) == 30:                                      # the gate is x + b: keep it off 0
        bb = inp["b"][(torch.arange(n) // step_b) % size_b].reshape(p["shape"]) if p["bias"] else 0.0
        inp["x"] = _fix_gate(inp["x"], lambda x: x + bb, st) if st != "f64" else torch.where((inp["x"] + bb).abs() < 2e-3, inp["x"] + 0.5, inp["x"])
    if p["grad"] == 1:                                         # drawn independently of x: about half of the signs disagree
        r = rn(*p["shape"])
        inp["ref"] = store(torch.where(r.abs() < 2e-3, torch.where(r < 0, -0.5, 0.5).to(r.dtype), r))
    return inp


def _fb_eval(c, inp, dt, **kw):
    p = c.p
    return {"y": fba_ref(inp["x"], inp.get("b"), inp.get("ref"), fba_mode(p), p["alpha"], p["scale"], fba_geom(p)[1], dt, **kw)}


def fba_reasons(p):
    """why the scalar form is chosen (empty: the vec form)"""
    n, step_b, _ = fba_geom(p)
    grid = 16 if p["st"] == "f32" else 8
    return [r for r, hit in (("n", n % 4 != 0), ("step_b", p["bias"] and step_b % 4 != 0), ("pointer", (p["off"] * ITEM[p["st"]]) % grid != 0)) if hit]


def fba_form(c):
    if c.p["st"] == "f64":
        return "fba:f64"
    return "fba:%s:%s" % ("scalar" if fba_reasons(c.p) else "vec", c.p["st"])


def _fb_facets(c):
    p = c.p
    n, step_b, _ = fba_geom(p)
    out = ["fba:mode-%d" % fba_mode(p), "fba:alpha-%g" % p["alpha"]]
    if p["st"] != "f64":
        out += ["fba:scalar-by-" + r for r in fba_reasons(p)]
        vec = not fba_reasons(p)
        if (n // 4 if vec else n) > FBA_TRIP:
            out.append("fba:%s:second-trip" % ("vec" if vec else "scalar"))
    if not p["bias"]:
        out.append("fba:no-bias")
    elif len(p["shape"]) == 2:
        out.append("fba:2-D")
    elif step_b % 4 == 0:
        out.append("fba:step_b%4==0")
    elif step_b == 35:
        out.append("fba:step_b-35")
    if p["scale"] != 1.0:
        out.append("fba:scale!=1")
    return out


def _fb_mut(c, inp):
    p = c.p
    f64 = torch.float64
    n, step_b, _ = fba_geom(p)
    mode = fba_mode(p)
    r = torch.from_numpy(A.reference(c.id)["y"])
    a = r.clone(); a.view(-1)[-1] = UNWRITTEN
    out = [("last element not written", a)]
    if is_big(c):                                              # the second-trip cases
        vec = not fba_reasons(p)
        a = r.clone(); a.view(-1)[(4 if vec else 1) * FBA_TRIP:] = 0
        out.append(("second-trip elements left zero", a))
    ev = lambda **kw: _fb_eval(c, inp, f64, **kw)["y"]
    if mode == 31:
        out.append(("gate by x instead of ref", ev(gate_x=True)))
    if p["bias"] and step_b > 1 and mode not in (12, 32):
        out.append(("bias index without / step_b", ev(no_div=True)))
    if p["bias"] and step_b % 4 and mode not in (12, 32):
        out.append(("bias of element 0 of a 4-group used where step_b % 4 != 0", ev(group0=True)))
    if mode == 30 and p["scale"] < 0:                          # (the leaky ReLU commutes with a positive factor)
        out.append(("scale applied before the activation", ev(scale_first=True)))
    if mode in (30, 31):
        out.append(("alpha ignored", fba_ref(inp["x"], inp.get("b"), inp.get("ref"), mode, 1.0 if p["alpha"] == 0.2 else 0.2, p["scale"], step_b, f64)))
    if mode in (12, 32):
        out += [("modes 12 and 32 returning x", ev(zero_modes_x=True)),
                ("modes 12 and 32 taken as grad 0", fba_ref(inp["x"], inp.get("b"), None, mode - 2, p["alpha"], p["scale"], step_b, f64))]
    return [(n_, {"y": v}) for n_, v in out]


_fb("vec-f32-m30-bias-2x3x4x8", (2, 3, 4, 8), bias=True)
_fb("vec-f32-m31-nobias-2x3x4x8", (2, 3, 4, 8), grad=1)
_fb("vec-f32-m31-bias-alpha1.5-negscale-2x5x2x6", (2, 5, 2, 6), bias=True, grad=1, alpha=1.5, scale=-0.7)
_fb("vec-f32-m31-alpha0-scale1-3x8x4", (3, 8, 4), grad=1, alpha=0.0, scale=1.0)                  # the ReLU gate of the projectors
_fb("vec-f32-m30-bias-alpha1.5-negscale-2x5x2x6", (2, 5, 2, 6), bias=True, alpha=1.5, scale=-0.7)
_fb("vec-f32-m30-nobias-alpha0-2x3x8", (2, 3, 8), alpha=0.0)
_fb("vec-f32-m32-bias-2x3x4x8", (2, 3, 4, 8), bias=True, grad=2)
_fb("vec-f32-m12-nobias-2x3x4x8", (2, 3, 4, 8), act=1, grad=2)
_fb("vec-f32-m10-bias-2x3x4x8", (2, 3, 4, 8), bias=True, act=1, scale=0.6)
_fb("vec-f32-m11-bias-2x3x4x8", (2, 3, 4, 8), bias=True, act=1, grad=1, scale=1.0)
_fb("scalar-f32-m30-bias-step35-4x3x5x7", (4, 3, 5, 7), bias=True)                              # n % 4 == 0: step_b alone
_fb("scalar-f32-m31-nobias-3x5x7", (3, 5, 7), grad=1)                                           # n = 105: n alone
_fb("scalar-f32-m30-bias-off1-2x4x4x4", (2, 4, 4, 4), bias=True, off=1)                          # the pointer alone
_fb("scalar-f32-m30-bias-2D-6x10", (6, 10), bias=True)                                           # step_b = 1
_fb("scalar-f32-m31-bias-step35-2x3x5x7", (2, 3, 5, 7), bias=True, grad=1, alpha=1.5)
_fb("scalar-f32-m32-bias-2x3x5x7", (2, 3, 5, 7), bias=True, grad=2)
_fb("scalar-f32-m10-bias-alpha0-2x3x5x7", (2, 3, 5, 7), bias=True, act=1, alpha=0.0, scale=-0.7)
for _st in ("f16", "bf16"):
    _fb("vec-%s-m30-bias-2x3x4x8" % _st, (2, 3, 4, 8), st=_st, bias=True)
    _fb("vec-%s-m31-nobias-alpha1.5-negscale-2x3x4x8" % _st, (2, 3, 4, 8), st=_st, grad=1, alpha=1.5, scale=-0.7)
    _fb("scalar-%s-m30-bias-step35-4x3x5x7" % _st, (4, 3, 5, 7), st=_st, bias=True, scale=-0.7)
    _fb("scalar-%s-m31-nobias-off2-2x4x4x4" % _st, (2, 4, 4, 4), st=_st, grad=1, alpha=0.0, off=2)
    _fb("scalar-%s-m11-bias-2D-6x10" % _st, (6, 10), st=_st, bias=True, act=1, grad=1)
    _fb("vec-%s-m12-bias-2x3x4x8" % _st, (2, 3, 4, 8), st=_st, bias=True, act=1, grad=2)
_fb("f64-m30-bias-step35-2x3x5x7", (2, 3, 5, 7), st="f64", bias=True)
_fb("f64-m31-nobias-alpha1.5-negscale-2x3x4x8", (2, 3, 4, 8), st="f64", grad=1, alpha=1.5, scale=-0.7)
_fb("f64-m32-bias-2x3x4x8", (2, 3, 4, 8), st="f64", bias=True, grad=2)
_fb("vec-f32-m30-bias-1x2x1024x2049-second-trip", (1, 2, 1024, 2049), bias=True)                 # 16.8 MB
_fb("scalar-f32-m31-nobias-1x1x1025x1025-second-trip", (1, 1, 1025, 1025), grad=1)               # 4.2 MB


# ================================================================================================= the table's machinery
A.register("upfirdn2d", Spec(_uf_make, _uf_eval, uf_form, _uf_mut, BAR_EW), [c for c in CASES if c.op == "upfirdn2d"],
           out_st=lambda c, n: c.p["st"], border=lambda c: True, facets=_uf_facets)
A.register("fba", Spec(_fb_make, _fb_eval, fba_form, _fb_mut, BAR_EW), [c for c in CASES if c.op == "fba"], out_st=lambda c, n: c.p["st"], facets=_fb_facets)

by_id, inputs, reference, bar, err32, branch_of, facets_of, mutations = A.by_id, A.inputs, A.reference, A.bar, A.err32, A.branch_of, A.facets_of, A.mutations


def out_numel(c):
    return c.p["M"] * int(np.prod(uf_out_hw(c.p))) * c.p["C"] if c.op == "upfirdn2d" else fba_geom(c.p)[0]


def is_big(c):
    """one of the four second-trip cases, the only large ones"""
    return out_numel(c) > BIG // 4


def f64_allowed(c):
    """the elementwise error a float64 launch may carry (module docstring)"""
    inp, p = inputs(c.id), c.p
    if c.op == "fba":
        return 2.0 ** -52 * np.abs(reference(c.id)["y"])
    kh, kw = p["k"]
    return 2.0 * (kh * kw + 1) * 2.0 ** -53 * upfirdn_ref(inp["x"].abs(), inp["k"].abs(), p["up"], p["down"], p["pads"]).numpy()


def judge(c, name, got):
    """-> (violations, err): act_cases.judge; a float64 case: element by element against ``f64_allowed`` (err in its units)"""
    ref, got = reference(c.id)[name], np.asarray(got, np.float64)
    if c.p["st"] != "f64":
        # (modes 12 and 32: the reference is 0 everywhere, the half formula allows 0 -- exact equality, as ``compare`` asks at scale 0)
        return _judge(c, name, got) if ref.any() else compare(ref, got, bar(c, name))
    assert ref.shape == got.shape, (ref.shape, got.shape)
    if not np.isfinite(got).all():
        return ["%d non-finite values" % (~np.isfinite(got)).sum()], float("inf")
    d, lim = np.abs(got - ref), f64_allowed(c)
    bad = d > lim
    ratio = np.where(lim > 0, d / np.where(lim > 0, lim, 1.0), np.where(d > 0, np.inf, 0.0))
    return (["%d values outside the float64 bound, worst %.2f x" % (bad.sum(), ratio.max())] if bad.any() else []), float(ratio.max())


def as_stored(c, name, arr):
    """a float64 result as the output tensor would hold it: rounded once to the output's storage type"""
    return torch.from_numpy(np.asarray(arr, np.float64)).to(TD[c.p["st"]]).double().numpy()
