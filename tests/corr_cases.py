"""Cases, float64 references, seeded defects and bars of the correspondence-kernel tests (tests/test_corr_cases_cpu.py,
tests/test_gpu_corr.py): csrc/corr.hip -- rselfcorr, corr_prep, unfold_rows, the fp32 and split-bf16 GEMMs, softmax_rows,
unfold / fold_patches.  Plain torch / numpy on the CPU: nothing here touches the device, and the device is never its own judge.

The conventions are those of tests/bwd_cases.py (``Case``, ``Spec``, ``_gen`` seeded from the case id, ``compare``); what is new
is the size an error is measured against.  The logits this path produces are cosines divided by T = 0.01, so the GEMMs are not
judged against max|ref| alone but element by element against S = |alpha| (|A| @ |op(B)|), the sum of the magnitudes of the
products of that element, in units of 2^-24 S (fp32 and six-pass kernels) or 2^-17 S (three-pass kernels):

  term cases   every plane of every operand element is positive (x = h + m + l, or h + l, built so that the kernel's bf16
               round-to-nearest split recovers the planes exactly): every product term has one sign, nothing cancels over K, a
               dropped pass moves EVERY element by >= 48 units (x6) / >= 100 units (x3).  Bars: 12 units (x6, and the exact-fp32
               kernel on the same construction), 8 units (x3).
  randn cases  the worst-case bound of an fp32 accumulation in any order plus the dropped plane products:
               (K + 8) 2^-24 S (fp32, x6), (3 2^-17 + (K + 8) 2^-24) S (x3); the project's max-norm class bars (2e-6, 1e-5 from
               K = 4096, 3e-5 for x3) are applied next to them.

``branch(c)`` restates each launcher's ``if`` (corr.hip) and ops._gemm_passes; ``facets(c)`` adds what the case exercises inside
the kernel it reaches (even / ragged edge, K-tile count 1 / odd / even per BK, loop trip).  FACETS is the full expected set.
x3-big (BK = 16) takes K % 32 == 0 only, so its tile count is always even: no odd case exists for it.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from bwd_cases import BAR_EW, BAR_MOVE, Case, Spec, _gen, _randn, compare  # noqa: F401

U24, U17 = 2.0 ** -24, 2.0 ** -17
EPS = 2.220446049250313e-16
BAR_RSELF, BAR_SOFTMAX = 1e-5, 2e-5

OPS = {}
CASES = []


def _case(op, cid, seed=0, **p):
    CASES.append(Case(op, "%s-%s" % (op, cid), p, seed))


def cdiv(a, b):
    return (a + b - 1) // b


# ================================================================================================================ GEMM
# p: form NT | NN, mode x6 | x3 | f32 (as ops takes it), b, M, N, K, alpha (NT), kind randn | term, planes 3 | 2 (term),
#    ldb / ldc (NN through the C entry: B is the first N columns of a K x ldb matrix, C the first N of an M x ldc one)
def gemm_passes(mode, K, N=4, form="NT"):
    """ops._gemm_passes with ops.gemm_nn's N % 4 test in front: 0 = the exact-fp32 MFMA kernel, 6 / 3 = bf16 planes"""
    if form == "NN" and N % 4:
        return 0                                  # (ppst_gemm_nn_f32 refuses N % 4 as well: ops raises ValueError)
    if mode == "f32":
        return 0
    if mode == "x3" and K % 32 == 0:
        return 3
    return 6 if K % 16 == 0 else 0                # x3 with K % 32 != 0 falls through to six passes; K % 16 != 0 to fp32 (refused)


def gemm_big(p):
    return cdiv(p["M"], 256) * cdiv(p["N"], 256) * p["b"] >= 224 and p["N"] > 128 and p["M"] > 128


def gemm_ntl(N):
    ntl = 5 if N >= 160 else (4 if N >= 128 else (N + 31) // 32)
    if N % 160 != 0 and N % 128 == 0:
        ntl = 4
    return ntl


def gemm_geometry(p):
    """-> (passes, BM, BN, BK) of the kernel gemm_dispatch / gemm_split_dispatch launches"""
    ps = gemm_passes(p["mode"], p["K"], p["N"], p["form"])
    if ps == 0:
        return 0, 128, 32 * gemm_ntl(p["N"]), 16
    if gemm_big(p):
        return ps, 256, 256, 16
    return ps, 128, 128, 16 if ps == 6 else 32


def _gemm_branch(c):
    p = c.p
    ps, BM, BN, BK = gemm_geometry(p)
    if ps == 0:
        return "f32:%s:NTL%d" % (p["form"], BN // 32)
    return "split:%s:x%d:%s%s" % (p["form"], ps, "big" if BM == 256 else "small", ":BK32" if BK == 32 else "")


def _gemm_facets(c):
    p = c.p
    ps, BM, BN, BK = gemm_geometry(p)
    br = _gemm_branch(c)
    out = [br]
    if ps:
        out.append(br + (":even" if p["M"] % BM == 0 and p["N"] % BN == 0 else ":ragged"))
        nk = p["K"] // BK
        out.append("split:BK%d:tiles-%s" % (BK, "1" if nk == 1 else ("odd" if nk % 2 else "even")))
    return out


def split_planes(x, n):
    """the kernel's split: p[0] = bf16(x), then bf16 of the successive remainders (round to nearest even), as float32"""
    out, r = [], x.clone()
    for _ in range(n):
        q = r.bfloat16().float()
        out.append(q)
        r = r - q
    return out, r


def _term_operand(g, planes, *shape):
    ri = lambda n: torch.randint(0, n, shape, generator=g).double()
    h = 1 + ri(128) / 128
    if planes == 3:
        m = 2.0 ** -9 * (1.5 + ri(64) / 128)
        l = 2.0 ** -18 + ri(32) * 2.0 ** -23
        parts = [h, m, l]
    else:
        parts = [h, 2.0 ** -10 * (1 + ri(128) / 128)]
    x64 = sum(parts)
    x = x64.float()
    assert torch.equal(x.double(), x64), "the sum of the planes is not a float32"
    got, rest = split_planes(x, planes)
    for a, b in zip(got, parts):
        assert torch.equal(a.double(), b), "the bf16 split does not recover the planes"
    assert not rest.any()
    return x


def _gemm_make(c):
    p = c.p
    g = _gen(c._replace(id=p.get("data", c.id)))          # (twins -- the f32 run of an x6 term case -- share their operands)
    b, M, N, K = p["b"], p["M"], p["N"], p["K"]
    bshape = (b, N, K) if p["form"] == "NT" else (b, K, p.get("ldb", N))
    if p.get("kind") == "term":
        return {"A": _term_operand(g, p["planes"], b, M, K), "B": _term_operand(g, p["planes"], *bshape)}
    return {"A": _randn(g, b, M, K), "B": _randn(g, *bshape)}


def _opB(c, inp, dt=torch.float64):
    """op(B) as (b, K, N)"""
    Bm = inp["B"].to(dt)
    return Bm.transpose(1, 2) if c.p["form"] == "NT" else Bm[..., :c.p["N"]]


def _gemm_ref(c, inp, dt):
    return {"C": c.p.get("alpha", 1.0) * torch.matmul(inp["A"].to(dt), _opB(c, inp, dt))}


def gemm_scale(c):
    return _gemm_scale(c.id)


@functools.lru_cache(maxsize=2)
def _gemm_scale(c_id):
    """S: per element, |alpha| (|A| @ |op(B)|) in float64"""
    c = by_id(c_id)
    inp = inputs(c.id)
    return (abs(c.p.get("alpha", 1.0)) * torch.matmul(inp["A"].double().abs(), _opB(c, inp).abs())).numpy()


def gemm_bar(c):
    """-> (bar relative to S, the unit the table prints it in, the max-norm class bar)"""
    p = c.p
    ps = gemm_geometry(p)[0]
    cls = 3e-5 if ps == 3 else (1e-5 if p["K"] >= 4096 else 2e-6)
    if p.get("kind") == "term":
        return (8 * U17, U17, cls) if ps == 3 else (12 * U24, U24, cls)
    if ps == 3:
        return 3 * U17 + (p["K"] + 8) * U24, U17, cls
    return (p["K"] + 8) * U24, U24, cls


def _gemm_mut(c, inp):
    p = c.p
    ps, BM, BN, BK = gemm_geometry(p)
    A, Bo, alpha = inp["A"].double(), _opB(c, inp), p.get("alpha", 1.0)
    ref = alpha * torch.matmul(A, Bo)
    out = []
    if p.get("kind") == "term":
        n = p["planes"]
        pa, pb = split_planes(inp["A"], n)[0], split_planes(_opB(c, inp, torch.float32).contiguous(), n)[0]
        terms = [(0, 1), (1, 0)] if n == 2 else [(1, 1), (0, 2), (2, 0), (0, 1), (1, 0)]
        for i, j in terms:
            out.append(("product term %s.%s left out" % ("hml"[i] if n == 3 else "hl"[i], "hml"[j] if n == 3 else "hl"[j]),
                        {"C": ref - alpha * torch.matmul(pa[i].double(), pb[j].double())}))
        return out
    if p["K"] > BK:
        out.append(("last K tile left out", {"C": alpha * torch.matmul(A[..., :p["K"] - BK], Bo[:, :p["K"] - BK])}))
    if p["M"] % BM:
        a = ref.clone(); a[:, -1] = 0
        out.append(("ragged tail row zero", {"C": a}))
    if p["N"] % BN:
        a = ref.clone(); a[..., -(p["N"] % 4 or 4):] = 0
        out.append(("ragged tail columns zero", {"C": a}))
    if p["b"] > 1:
        a = ref.clone(); a[1] = alpha * torch.matmul(A[1], Bo[0])
        out.append(("batch element 1 computed from element 0's B", {"C": a}))
    if alpha != 1.0:
        out.append(("alpha ignored", {"C": ref / alpha}))
    if p.get("ldb", p["N"]) > p["N"]:
        flat = inp["B"].double().reshape(p["b"], -1)[:, :p["K"] * p["N"]].reshape(p["b"], p["K"], p["N"])
        out.append(("B read with ldb = N", {"C": torch.matmul(A, flat)}))
    return out


OPS["gemm"] = Spec(_gemm_make, _gemm_ref, _gemm_branch, _gemm_mut, None)

# --- split kernels, randn edge cases: {NT, NN} x {x6, x3} x {small, big}; K-tile counts 1 / odd / even per BK
_SPLIT_SHAPES = {     # (mode, size): [(tag, b, M, N, K)]
    ("x6", "small"): [("even", 2, 128, 128, 16), ("ragged", 2, 129, 132, 48), ("row", 2, 1, 132, 64)],
    ("x3", "small"): [("even", 2, 128, 128, 32), ("ragged", 2, 129, 132, 96), ("row", 2, 1, 132, 128)],
    ("x6", "big"): [("even", 56, 512, 512, 64), ("ragged", 56, 300, 260, 48), ("one-block", 224, 129, 132, 16)],
    ("x3", "big"): [("even", 56, 512, 512, 64), ("ragged", 56, 300, 260, 32), ("one-block", 224, 129, 132, 96)],
}
for _form in ("NT", "NN"):
    for (_mode, _size), _shapes in _SPLIT_SHAPES.items():
        for _tag, _b, _M, _N, _K in _shapes:
            _case("gemm", "%s-%s-%s-%s-%dx%dx%dx%d" % (_form, _mode, _size, _tag, _b, _M, _N, _K), form=_form, mode=_mode, b=_b, M=_M, N=_N, K=_K,
                  alpha=0.37 if _form == "NT" and _tag == "ragged" else 1.0)
    # x3 asked for at K % 32 != 0: six passes run (ops._gemm_passes), and the six-pass bar holds
    _case("gemm", "%s-x3-falls-to-x6-2x129x132x48" % _form, form=_form, mode="x3", b=2, M=129, N=132, K=48)
# NN through the C entry: B and C are the first N columns of wider matrices
_case("gemm", "NN-x6-small-ld-2x129x132x48", form="NN", mode="x6", b=2, M=129, N=132, K=48, ldb=140, ldc=136)
_case("gemm", "NN-x3-big-ld-56x300x260x32", form="NN", mode="x3", b=56, M=300, N=260, K=32, ldb=264, ldc=268)
_case("gemm", "NN-f32-ld-2x130x68x48", form="NN", mode="f32", b=2, M=130, N=68, K=48, ldb=72, ldc=76)

# --- the exact-fp32 MFMA kernel: NTL 1 .. 5, the ragged last block of each, M in {1, 130}, K in {16, 48}
_F32_N = {"NT": (20, 32, 40, 64, 70, 96, 128, 132, 160, 192), "NN": (4, 8, 20, 32, 40, 64, 68, 96, 128, 132, 160, 192)}
for _form, _ns in _F32_N.items():
    for _i, _N in enumerate(_ns):
        _M, _K = ((1, 16), (130, 48), (130, 16), (1, 48))[_i % 4]
        _case("gemm", "%s-f32-2x%dx%dx%d" % (_form, _M, _N, _K), form=_form, mode="f32", b=2, M=_M, N=_N, K=_K, alpha=-1.7 if _form == "NT" else 1.0)

# --- term cases: 300 x K against 260 x K; small = batch 2, big = batch 56.  The f32 twin runs the x6 operands.
for _form in ("NT", "NN"):
    for _size, _b in (("small", 2), ("big", 56)):
        for _K in (16, 48):
            _id = "%s-x6-%s-term-%dx300x260x%d" % (_form, _size, _b, _K)
            _case("gemm", _id, form=_form, mode="x6", kind="term", planes=3, b=_b, M=300, N=260, K=_K)
            _case("gemm", _id.replace("-x6-", "-f32-"), form=_form, mode="f32", kind="term", planes=3, b=_b, M=300, N=260, K=_K, data="gemm-" + _id)
        for _K in ((32, 96) if _size == "small" else (32,)):
            _case("gemm", "%s-x3-%s-term-%dx300x260x%d" % (_form, _size, _b, _K), form=_form, mode="x3", kind="term", planes=2, b=_b, M=300, N=260, K=_K)


# =========================================================================================================== corr_prep
# launcher (ppst_corr_prep): C % 64 or C > 1024 -> corr_prep_loop_kernel, else corr_prep_kernel; at most 2048 blocks of 4 rows
def _cp_make(c):
    p = c.p
    x = _randn(_gen(c), p["B"], p["P"], p["C"])
    if p.get("zero_row"):
        x[0, 2] = 0
    if p.get("big_mean"):
        x = x + 1e3
    return {"x": x}


def corr_prep_fwd(x, nc, mean_over=None, center=True):
    x = x.clone()
    if nc and center:
        x[..., :nc] = x[..., :nc] - x[..., :nc].sum(-1, keepdim=True) / (mean_over or nc)
    return x / (x.norm(2, -1, keepdim=True) + EPS)


def _cp_ref(c, inp, dt):
    return {"y": corr_prep_fwd(inp["x"].to(dt), c.p["ncenter"])}


def _cp_branch(c):
    return "corr_prep:loop" if c.p["C"] % 64 or c.p["C"] > 1024 else "corr_prep:wave"


def _trip(n, cap):
    return "trip2" if n > cap else "trip1"


def _cp_facets(c):
    return [_cp_branch(c), "corr_prep:" + _trip(c.p["B"] * c.p["P"], 8192)]


def _cp_mut(c, inp):
    p = c.p
    x, nc, C = inp["x"].double(), p["ncenter"], p["C"]
    ref = corr_prep_fwd(x, nc)
    rows = p["B"] * p["P"]
    out = []
    if nc % 64:
        out.append(("ncenter rounded down to a multiple of 64", {"y": corr_prep_fwd(x, nc // 64 * 64)}))
        if min(C, cdiv(nc, 64) * 64) != nc:
            out.append(("ncenter rounded up to a multiple of 64", {"y": corr_prep_fwd(x, min(C, cdiv(nc, 64) * 64))}))
    if 0 < nc < C:
        out.append(("the mean taken over C", {"y": corr_prep_fwd(x, nc, mean_over=C)}))
    if nc:
        out.append(("not centred", {"y": corr_prep_fwd(x, nc, center=False)}))
    else:
        out.append(("centred although ncenter = 0", {"y": corr_prep_fwd(x, C)}))
    if rows > 8192:
        a = ref.clone(); a.view(rows, C)[8192:] = 0
        out.append(("rows >= 8192 untouched", {"y": a}))
    if rows % 4:
        a = ref.clone(); a.view(rows, C)[rows - rows % 4:] = 0
        out.append(("the last rows % 4 rows untouched", {"y": a}))
    return out


OPS["corr_prep"] = Spec(_cp_make, _cp_ref, _cp_branch, _cp_mut, BAR_EW)
for _C, _nc in ((64, 0), (64, 64), (128, 100), (512, 256), (1024, 256), (72, 72), (1088, 256), (4608, 256)):
    _case("corr_prep", "C%d-nc%d-rows7" % (_C, _nc), B=1, P=7, C=_C, ncenter=_nc)
for _nc in (0, 64):
    _case("corr_prep", "C64-nc%d-rows8200" % _nc, B=2, P=4100, C=64, ncenter=_nc)
_case("corr_prep", "C512-nc256-zero-row", B=1, P=7, C=512, ncenter=256, zero_row=True)
_case("corr_prep", "C72-nc72-zero-row", B=1, P=7, C=72, ncenter=72, zero_row=True)
_case("corr_prep", "C128-nc100-mean1e3", B=1, P=7, C=128, ncenter=100, big_mean=True)
_case("corr_prep", "C1088-nc256-mean1e3", B=1, P=7, C=1088, ncenter=256, big_mean=True)


# ============================================================================================================= softmax
# ppst_softmax_rows: one block of 256 threads per row, float4 idx = thread + 256 i (i < 16) while idx < cols / 4
_SM_KINDS = ("randn", "cos", "tie", "equal", "dominant")


def _sm_make(c):
    p = c.p
    g = _gen(c)
    cols, div = p["cols"], p["div"]
    hot = 300 if cols > 300 else cols - 1       # (float4 75: thread 75, the second wave)
    rows = []
    for kind in (_SM_KINDS if p["rows"] == 5 else ("cos",)):
        if kind == "randn":
            r = _randn(g, cols)
        elif kind == "cos":
            r = torch.rand(cols, generator=g) * 2 - 1
            r[cols - 1] = 1.0                     # (the match itself, in the last column: the tail of the row carries weight)
        elif kind == "tie":                       # multiples of 1/8 below the maximum, the maximum twice, far apart
            r = -(torch.randint(1, 32, (cols,), generator=g).float() / 8) * div
            r[1], r[hot] = 0.5 * div, 0.5 * div
        elif kind == "equal":
            r = torch.full((cols,), 0.25)
        else:
            r = torch.rand(cols, generator=g) * 2 - 1
            r[hot] = float(r[torch.arange(cols) != hot].max()) + 50.0 / div
        rows.append(r)
    return {"x": torch.stack(rows)}


def softmax_fwd(x, div, dt):
    return torch.softmax(x.to(dt) / torch.tensor(np.float32(div)).to(dt), -1)


def _sm_ref(c, inp, dt):
    return {"p": softmax_fwd(inp["x"], c.p["div"], dt)}


def _sm_first_wave(cols):
    idx = torch.arange(cols // 4)
    return ((idx % 256) < 64).repeat_interleave(4)


def _sm_mut(c, inp):
    p = c.p
    cols, div = p["cols"], p["div"]
    x = inp["x"]
    ref = softmax_fwd(x, div, torch.float64)
    v = x.double() / float(np.float32(div))
    e = torch.exp(v - v.max(-1, keepdim=True).values)
    out = []
    if cols % 1024:
        out.append(("the last cols % 1024 columns left out of the sum", {"p": e / e[:, :cols - cols % 1024].sum(-1, keepdim=True)}))
    if cols >= 1024:
        keep = (torch.arange(cols // 4) % 256 < 192).repeat_interleave(4)
        out.append(("the fourth wave's partial sum left out", {"p": e / e[:, keep].sum(-1, keepdim=True)}))
    if cols > 256:                                # float32, as the kernel evaluates it: exp overflows where the shift is too small
        v32 = x / np.float32(div)
        e32 = torch.exp(v32 - v32[:, _sm_first_wave(cols)].max(-1, keepdim=True).values)
        m = (e32 / e32.sum(-1, keepdim=True)).double()
        if not torch.isfinite(m).all():
            out.append(("the max taken over the first wave only", {"p": m}))
    if div != 1:
        out.append(("div applied after the exp", {"p": softmax_fwd(x, 1.0, torch.float64)}))
    if p["rows"] > 1:
        out.append(("every row normalised by row 0's sum", {"p": e / e[:1].sum(-1, keepdim=True)}))
    return out


OPS["softmax_rows_"] = Spec(_sm_make, _sm_ref, lambda c: "softmax_rows", _sm_mut, BAR_SOFTMAX)
for _cols in (4, 8, 252, 1028, 4096, 16384):
    for _rows in (1, 5):
        for _div in (1.0, 0.01):
            _case("softmax_rows_", "%dx%d-div%g" % (_rows, _cols, _div), rows=_rows, cols=_cols, div=_div)


# =========================================================================================================== rselfcorr
# ppst_rselfcorr: one wave per 4 x 4 patch, at most 2048 blocks of 4 waves: patches from 8192 on take the second trip
def _rs_make(c):
    p = c.p
    fea = _randn(_gen(c), p["B"], p["H"], p["W"], 64)
    if p.get("const_patch"):                      # every pixel of patch (0, 0) of image 0 constant over its channels
        fea[0, :4, :4, :] = torch.arange(16.0).view(4, 4, 1) / 4 - 1
    return {"fea": fea}


def rselfcorr_fwd(fea, center=True, swap_pixels=False):
    """NHWC (B,H,W,64) -> (B,H/4,W/4,256), channel = i * 16 + j over the 16 pixels of the patch, row-major"""
    B, H, W, C = fea.shape
    x = fea.reshape(B, H // 4, 4, W // 4, 4, C)
    x = x.permute(0, 1, 3, 4, 2, 5) if swap_pixels else x.permute(0, 1, 3, 2, 4, 5)
    x = x.reshape(B, H // 4, W // 4, 16, C)
    if center:
        x = x - x.mean(-1, keepdim=True)
    x = x / (x.norm(2, -1, keepdim=True) + EPS)
    return torch.matmul(x, x.transpose(-1, -2)).reshape(B, H // 4, W // 4, 256)


def _rs_ref(c, inp, dt):
    return {"out": rselfcorr_fwd(inp["fea"].to(dt))}


def _rs_facets(c):
    return ["rselfcorr", "rselfcorr:" + _trip(c.p["B"] * (c.p["H"] // 4) * (c.p["W"] // 4), 8192)]


def _rs_mut(c, inp):
    p = c.p
    fea = inp["fea"].double()
    ref = rselfcorr_fwd(fea)
    gy, gx = p["H"] // 4, p["W"] // 4
    out = [("not centred", {"out": rselfcorr_fwd(fea, center=False)}),
           ("pixel rows and columns of the patch swapped", {"out": rselfcorr_fwd(fea, swap_pixels=True)})]
    if p["B"] * gy * gx > 8192:
        a = ref.clone(); a.view(-1, 256)[8192:] = 0
        out.append(("patches >= 8192 untouched", {"out": a}))
    if gy != gx:
        out.append(("x and y patch index swapped", {"out": ref.reshape(p["B"], gx, gy, 256).transpose(1, 2)}))
    return out


OPS["rselfcorr"] = Spec(_rs_make, _rs_ref, lambda c: "rselfcorr", _rs_mut, BAR_RSELF)
_case("rselfcorr", "2x4x4", B=2, H=4, W=4)
_case("rselfcorr", "2x8x12", B=2, H=8, W=12)
_case("rselfcorr", "2x264x252-second-trip", B=2, H=264, W=252)
_case("rselfcorr", "2x8x12-out-ld260", B=2, H=8, W=12, out_ld=260)
_case("rselfcorr", "2x8x12-constant-patch", B=2, H=8, W=12, const_patch=True)


# ========================================================================================================= unfold_rows
def _ur_make(c):
    p = c.p
    return {"x": _randn(_gen(c), p["B"], p["H"], p["W"], p["C"])}


def unfold_rows_fwd(x, k, swap_taps=False, clamp=False):
    xc = x.permute(0, 3, 1, 2)
    if clamp and k > 1:
        u = F.unfold(F.pad(xc, [k // 2] * 4, mode="replicate"), k)
    else:
        u = F.unfold(xc, k, padding=k // 2)
    u = u.permute(0, 2, 1)
    if swap_taps:
        B, P, K = u.shape
        u = u.reshape(B, P, K // (k * k), k, k).transpose(-1, -2).reshape(B, P, K)
    return u.contiguous()


def _ur_ref(c, inp, dt):
    return {"rows": unfold_rows_fwd(inp["x"].to(dt), c.p["k"])}


def _ur_mut(c, inp):
    p = c.p
    x, k = inp["x"].double(), p["k"]
    ref = unfold_rows_fwd(x, k)
    out = [("every row one pixel late", {"rows": torch.roll(ref.reshape(-1, ref.shape[-1]), 1, 0).reshape(ref.shape)})]
    if k > 1:
        out.append(("ky and kx swapped", {"rows": unfold_rows_fwd(x, k, swap_taps=True)}))
        out.append(("the border clamped, not zero", {"rows": unfold_rows_fwd(x, k, clamp=True)}))
    if ref.shape[-1] > 256:
        a = ref.clone(); a[..., 256:] = 0
        out.append(("columns >= 256 untouched", {"rows": a}))
    return out


OPS["unfold_rows"] = Spec(_ur_make, _ur_ref, lambda c: "unfold_rows", _ur_mut, BAR_MOVE)
for _H, _W, _C in ((5, 7, 3), (4, 4, 8), (1, 6, 4)):
    for _k in (1, 3, 5):
        _case("unfold_rows", "%dx%dxC%d-k%d" % (_H, _W, _C, _k), B=2, H=_H, W=_W, C=_C, k=_k)
_case("unfold_rows", "3x3xC100-k3", B=2, H=3, W=3, C=100, k=3)


# ============================================================================================================= patches
# ppst_unfold_patches / ppst_fold_patches: one element per thread, at most 4096 blocks of 256: the stride loop starts above 2^20
def _pt_make(c):
    p = c.p
    g = _gen(c)
    s = p["s"]
    return {"x": _randn(g, p["B"], p["C"], p["H"], p["W"]), "y": _randn(g, p["B"], (p["H"] // s) * (p["W"] // s), p["C"] * s * s)}


def _pt_ref(c, inp, dt):
    p = c.p
    s = p["s"]
    return {"unfold": F.unfold(inp["x"].to(dt), s, stride=s).permute(0, 2, 1).contiguous(),
            "fold": F.fold(inp["y"].to(dt).permute(0, 2, 1), (p["H"], p["W"]), s, stride=s)}


def _pt_facets(c):
    return ["patches", "patches:" + _trip(c.p["B"] * c.p["C"] * c.p["H"] * c.p["W"], 4096 * 256)]


def _pt_mut(c, inp):
    p = c.p
    s, B, C, H, W = p["s"], p["B"], p["C"], p["H"], p["W"]
    ref = _pt_ref(c, inp, torch.float64)
    gy, gx = H // s, W // s
    out = []
    if gy != gx:
        out.append(("x and y patch index swapped", {"unfold": ref["unfold"].reshape(B, gx, gy, -1).transpose(1, 2).reshape(ref["unfold"].shape),
                                                    "fold": F.fold(inp["y"].double().reshape(B, gx, gy, -1).transpose(1, 2).reshape(B, gy * gx, -1).permute(0, 2, 1),
                                                                   (H, W), s, stride=s)}))
    if s > 1:
        sw = lambda t: t.reshape(B, gy * gx, C, s, s).transpose(-1, -2).reshape(B, gy * gx, C * s * s)
        out.append(("ky and kx swapped", {"unfold": sw(ref["unfold"]), "fold": F.fold(sw(inp["y"].double()).permute(0, 2, 1), (H, W), s, stride=s)}))
    if B * C * H * W > 4096 * 256:
        a = ref["unfold"].clone(); a.view(-1)[4096 * 256:] = 0
        out.append(("elements >= 4096 * 256 untouched", {"unfold": a}))
    out.append(("image 1 from image 0", {"unfold": torch.cat([ref["unfold"][:1]] * B), "fold": torch.cat([ref["fold"][:1]] * B)}))
    return out


OPS["patches"] = Spec(_pt_make, _pt_ref, lambda c: "patches", _pt_mut, BAR_MOVE)
for _s in (1, 4, 8):
    _case("patches", "2x3x16x24-s%d" % _s, B=2, C=3, H=16, W=24, s=_s)
_case("patches", "2x3x512x512-s8-stride-loop", B=2, C=3, H=512, W=512, s=8)


# ====================================================================================================== the case table
_BY_ID = {c.id: c for c in CASES}
assert len(_BY_ID) == len(CASES), "case ids must be unique"
_FACETS = {"gemm": _gemm_facets, "corr_prep": _cp_facets, "rselfcorr": _rs_facets, "patches": _pt_facets}


def by_id(cid):
    return _BY_ID[cid]


def branch(c):
    return OPS[c.op].branch(c)


def facets(c):
    return _FACETS[c.op](c) if c.op in _FACETS else [branch(c)]


@functools.lru_cache(maxsize=4)
def inputs(c_id):
    c = by_id(c_id)
    return OPS[c.op].make(c)


@functools.lru_cache(maxsize=4)
def reference(c_id):
    c = by_id(c_id)
    return {k: v.numpy() for k, v in OPS[c.op].ref(c, inputs(c_id), torch.float64).items()}


def mutations(c):
    return [(n, {k: v.numpy() for k, v in o.items()}) for n, o in OPS[c.op].mutations(c, inputs(c.id))]


@functools.lru_cache(maxsize=4)
def err32(c_id):
    """error of the float32 evaluation of the reference against float64, relative to max|ref| (as bwd_cases.err32)"""
    c = by_id(c_id)
    r64 = reference(c_id)
    return {k: float(np.abs(v.double().numpy() - r64[k]).max() / max(np.abs(r64[k]).max(), 1e-300))
            for k, v in OPS[c.op].ref(c, inputs(c_id), torch.float32).items()}


def bar(c, out_name):
    """the bar ``judge`` applies; for a GEMM the one relative to S"""
    if c.op == "gemm":
        return gemm_bar(c)[0]
    if c.p.get("big_mean"):
        return max(BAR_EW, 4.0 * err32(c.id)[out_name])
    return OPS[c.op].cls


def unit(c, out_name="C"):
    """what the table prints errors in: 2^-24 S / 2^-17 S for a GEMM, the bar itself elsewhere (1 for bit equality)"""
    if c.op == "gemm":
        return gemm_bar(c)[1]
    return bar(c, out_name) or 1.0


def judge(c, out_name, got):
    """-> (violations, err) of one output of a case against its float64 reference, at the case's bar.  err: the largest error
    relative to the scale the bar is stated against (S per element for a GEMM, the row's max for the softmax, max|ref| elsewhere)"""
    ref, b = reference(c.id)[out_name], bar(c, out_name)
    got = np.asarray(got, np.float64)
    if c.op == "gemm":
        S = gemm_scale(c)
        assert (S > 0).all()
        bad, err = compare(ref / S, got / S, b, 1.0)
        bad = ["per element, against |alpha| |A| |op(B)|: " + m for m in bad]
        bad += ["max-norm class bar: " + m for m in compare(ref, got, gemm_bar(c)[2])[0]]
        return bad, err
    if c.op == "softmax_rows_":
        top = ref.max(-1, keepdims=True)
        bad, err = compare(ref / top, got / top, b, 1.0)
        if np.isfinite(got).all():
            off = np.abs(got.sum(-1) - 1.0).max()
            if off > c.p["cols"] * 2.0 ** -23:
                bad.append("a row sums to 1 %+.2e: outside cols * 2^-23" % off)
        return bad, err
    return compare(ref, got, b)


# every kernel a launcher of corr.hip can pick, and every edge / tile count / loop trip the cases must reach inside it
FACETS = (["split:%s:x%d:%s%s%s" % (f, ps, size, ":BK32" if (ps, size) == (3, "small") else "", edge)
           for f in ("NT", "NN") for ps in (6, 3) for size in ("small", "big") for edge in ("", ":even", ":ragged")]
          + ["split:BK%d:tiles-%s" % (bk, t) for bk in (16, 32) for t in ("1", "odd", "even")]
          + ["f32:%s:NTL%d" % (f, n) for f in ("NT", "NN") for n in (1, 2, 3, 4, 5)]
          + ["corr_prep:wave", "corr_prep:loop", "corr_prep:trip1", "corr_prep:trip2", "softmax_rows", "rselfcorr", "rselfcorr:trip1",
             "rselfcorr:trip2", "unfold_rows", "patches", "patches:trip1", "patches:trip2"])
