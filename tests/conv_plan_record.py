"""Record what ops.ConvPlan and ops.repack_plans produce, without a GPU: step tables and derived scalars, the launch descriptors
of a matrix of calls, and the pack / upscale jobs of repack_plans.

    python tests/conv_plan_record.py [OUT.json]        (default: tests/conv_plan_parent.json)

Everything recorded is discrete data, so two commits can be compared to the byte: tests/conv_plan_parent.json was written by this
tool at the commit before ConvPlan's host code was restated (adcf59b); tests/test_conv_plan_cpu.py records the working tree and
asserts equality.  Check out that commit, copy this file over and run it to see where the JSON comes from.

Plans are built from CPU weights; ops.lib is replaced by a proxy that forwards the host-only entries (ppst_conv_tiles, *_bytes,
ppst_pack_job_blocks) and answers 0 for everything else, recording the call.  Device pointers are recorded as the name(s) of the
plan tensor they point at.  Only public plan attributes are read.
"""
import contextlib
import ctypes
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch

KINDS = ("conv", "s2d", "convT", "dgrad", "dgrad_s2d", "dgrad_s2ds", "dgradT")
SHAPES = ((32, 32, 3), (64, 32, 1), (128, 64, 3), (256, 128, 3), (512, 512, 3), (96, 160, 3))      # (Cout, Cin, k) of the weight
HOST_ONLY = ("ppst_conv_tiles", "ppst_pack_job_blocks")
TABLES = ("steps", "steps_dual", "steps_up9", "steps_k64", "steps_dual_k64", "chunk_start")
SOURCES = ("src_dev", "src_dual", "src_k64", "src_dual_k64")
SCALARS = ("kind", "cout", "cin", "k", "bn", "halo", "n_groups", "nsteps", "flop_steps", "wstrides", "early_a", "precision", "scale",
           "up_scale", "fwd_scale", "w4_shape", "full_cover", "max_chan", "chunk_starts0", "chunk_starts0_k64", "chunks_per_group",
           "max_chunk_steps", "min_chunk_steps")


class FakeCuda(torch.Tensor):
    is_cuda = True


def fake(*shape, dtype=torch.float32):
    return torch.empty(*shape, dtype=dtype).as_subclass(FakeCuda)


class LibProxy:
    """ops.lib without a device: host-only entries run, every other entry returns 0 and is kept in ``calls``."""

    def __init__(self, real):
        self._real, self.calls = real, []

    def __getattr__(self, name):
        if name in HOST_ONLY or name.endswith("_bytes"):
            return getattr(self._real, name)

        def entry(*args):
            # (the K-split cuts live in an array of the caller's that is gone once the call returns: read them now)
            cuts = [list((ctypes.c_int32 * (v._obj.ksplit + 1)).from_address(v._obj.ksplit_starts))
                    for v in args if hasattr(v, "_obj") and v._obj.ksplit_starts]
            self.calls.append((name, args, cuts))
            return 0
        return entry


@contextlib.contextmanager
def host_only_ops():
    from ppst_amd import ops
    saved = {n: getattr(ops, n) for n in ("lib", "_chk", "_stream", "_ksplit_next")}
    saved_switch = {n: dict(getattr(ops, n)) for n in ("PRECISION", "TILE_ROWS", "CONV_VARIANT", "DUAL_CONVT", "UP9", "KSPLIT", "K64",
                                                       "BATCH_AWARE", "WINO", "TWO_BLOCK_8ROW", "TALL_TILE_SINGLE", "STREAM_1X1")}
    proxy = LibProxy(saved["lib"])
    ops.lib, ops._chk, ops._stream = proxy, (lambda t, name="tensor": None), (lambda: None)
    ops._ksplit_next = lambda stream: (0x1000, 0x2000, 7)
    cache = getattr(ops.ConvPlan, "_GEOMETRY", None)
    cached = dict(cache) if cache is not None else None
    if cache is not None:
        cache.clear()          # the first plan of a geometry below is the first of the process
    try:
        yield ops, proxy
    finally:
        for n, v in saved.items():
            setattr(ops, n, v)
        for n, v in saved_switch.items():
            getattr(ops, n).clear()
            getattr(ops, n).update(v)
        if cache is not None:
            cache.clear()
            cache.update(cached)


def _sha(data):
    return hashlib.sha256(data).hexdigest()[:20]


def _tensor(t):
    if t is None:
        return None
    return {"shape": list(t.shape), "dtype": str(t.dtype), "sha": _sha(t.contiguous().numpy().tobytes())}


def _plain(v):
    if isinstance(v, (tuple, list)):
        return [_plain(e) for e in v]
    if isinstance(v, torch.Size):
        return list(v)
    return v


def plan_record(plan):
    """every table and derived scalar of one plan"""
    rec = {n: _tensor(getattr(plan, n, None)) for n in TABLES}
    for n in SOURCES:
        s = getattr(plan, n, None)
        rec[n] = None if s is None else [_tensor(t) for t in s]
    for n in SCALARS:
        rec[n] = _plain(getattr(plan, n, None))
    src = _plain(plan.src)
    rec["src"] = {"len": len(src), "sha": _sha(json.dumps(src).encode())}
    # the weight source: the parameter itself, a view of it (element offset), or a tensor of its own
    off = plan.wsrc.data_ptr() - plan.wparam.data_ptr()
    inside = 0 <= off < plan.wparam.numel() * 4
    rec["wsrc"] = {"shape": list(plan.wsrc.shape), "of_param": off // 4 if inside else None}
    rec["packs"] = None if plan.precision == 2 else {str(k): int(v.numel()) for k, v in plan._packs.items()}
    return rec


def record_tables(ops):
    out = {}
    for kind in KINDS:
        for cout, cin, k in SHAPES:
            if k == 1 and kind not in ("conv", "dgrad"):
                continue
            w = torch.empty(cout, cin, k, k)
            first = plan_record(ops.ConvPlan(w, kind=kind, scale=0.5, precision=2))
            again = plan_record(ops.ConvPlan(w, kind=kind, scale=0.5, precision=2))      # the cached geometry
            out["%s %dx%dx%d" % (kind, cout, cin, k)] = {"first": first, "cached": again}
    return out


def _names(plan, tensors):
    """data pointer -> name(s) of the tensors of a plan and of a call"""
    named = dict(tensors)
    for n in TABLES + ("wparam", "wsrc"):
        named["plan." + n] = getattr(plan, n, None)
    for n in SOURCES:
        for i, t in enumerate(getattr(plan, n, None) or ()):
            named["plan.%s[%d]" % (n, i)] = t
    for k, t in (getattr(plan, "_packs", None) or {}).items():
        named["plan.pack[%s]" % k] = t
    by_ptr = {}
    for n, t in named.items():
        if t is not None:
            by_ptr.setdefault(t.data_ptr(), []).append(n)
    return {p: "|".join(sorted(ns)) for p, ns in by_ptr.items()}


def _ptr(v, names):
    if isinstance(v, ctypes.c_void_p):
        v = v.value
    if not v:
        return None
    return names.get(v, "?0x%x" % v)


def _conv_args(a, names, cuts):
    from ppst_amd import _lib
    rec = {}
    for f, t in _lib.ConvArgs._fields_:
        v = getattr(a, f)
        if f == "ksplit_starts":
            rec[f] = cuts[0] if v else None
        elif t is ctypes.c_void_p:
            rec[f] = _ptr(v, names)
        else:
            rec[f] = v
    return rec


def _call_args(args, names, cuts=()):
    out = []
    for v in args:
        if isinstance(v, ctypes.c_void_p):
            out.append(_ptr(v, names))
        elif hasattr(v, "_obj"):                   # ctypes.byref(ConvArgs)
            out.append(_conv_args(v._obj, names, cuts))
        elif isinstance(v, ctypes.c_float):
            out.append(v.value)
        else:
            out.append(v)
    return out


def _launch(ops, proxy, plan, x, kw):
    """one plan call: the launch entry's arguments, or the error the call raised"""
    if "out" not in kw:          # (an output the plan allocates itself would be a plain CPU tensor, which its own checks refuse)
        B, H, W, _ = x.shape
        oh, ow = (2 * H, 2 * W) if plan.kind == "convT" else kw.get("out_hw", (H, W))
        kw = dict(kw, out=fake(B, oh, ow, plan.cout, dtype=x.dtype))
    tensors = {"x": x}
    tensors.update({k: v for k, v in kw.items() if isinstance(v, torch.Tensor)})
    proxy.calls.clear()
    try:
        res = plan(x, **kw)
    except RuntimeError as e:
        return {"error": str(e)}
    y, st = res if isinstance(res, tuple) else (res, None)
    tensors["stats"] = st
    names = _names(plan, tensors)
    launches = [c for c in proxy.calls if c[0].startswith("ppst_conv2d")]
    assert len(launches) == 1, [c[0] for c in proxy.calls]
    rec = {"entry": launches[0][0], "args": _call_args(launches[0][1], names, launches[0][2]),
           "y": list(y.shape), "stats": None if st is None else list(st.shape)}
    proxy.calls.clear()
    return rec


def record_launches(ops):
    """a matrix of calls that reaches every launch form (the comments name the form a case is there for)"""
    f16, bf16 = torch.float16, torch.bfloat16
    plans = {}

    def plan(kind, cout, cin, k, precision):
        key = (kind, cout, cin, k, precision)
        if key not in plans:
            plans[key] = ops.ConvPlan(torch.empty(cout, cin, k, k), kind=kind, scale=0.25, precision=precision)
        return plans[key]
    # (name, plan, input shape, input dtype, call arguments as a function of B, switches, batch-aware)
    ss = lambda c: (lambda B: {"in_ss": fake(B, c, 2)})
    none = lambda B: {}
    cases = [
        ("tile 16-row 128->128 @32", plan("conv", 128, 128, 3, 0), (1, 32, 32, 128), None, none, {}, False),
        ("tile 16-row stats bias noise act", plan("conv", 128, 128, 3, 0), (2, 33, 35, 128), None,
         lambda B: {"stats": True, "bias": fake(128), "noise": fake(B, 1, 33, 35), "noise_weight": 0.5, "act": ops.ACT_LRELU,
                    "out_scale": 0.75, "pad_mode": ops.PAD_REFLECT}, {}, False),
        ("tile residual after act, out slice", plan("conv", 128, 128, 3, 0), (1, 32, 32, 128), None,
         lambda B: {"residual": fake(B, 32, 32, 128), "res_after_act": True, "act": ops.ACT_PRELU, "prelu": fake(128),
                    "out": fake(B, 32, 32, 256)[..., 128:]}, {}, False),
        ("tile 8-row (batch-aware, K split off)", plan("conv", 128, 128, 3, 0), (2, 32, 32, 128), None, none,
         {"KSPLIT": {"value": False}}, True),
        ("tile 8-row stats", plan("conv", 128, 128, 3, 0), (2, 32, 32, 128), None, lambda B: {"stats": True},
         {"KSPLIT": {"value": False}}, True),
        ("tile 8-row (TWO_BLOCK_8ROW)", plan("conv", 128, 128, 3, 0), (1, 128, 128, 128), None, none,
         {"TWO_BLOCK_8ROW": {"value": True}, "WINO": {"value": False}}, False),
        ("TILE_ROWS 8", plan("conv", 128, 128, 3, 0), (1, 32, 32, 128), None, none, {"TILE_ROWS": {"value": 8}}, False),
        ("N-256 s2d 128->256", plan("s2d", 256, 128, 3, 0), (1, 97, 97, 512), None, lambda B: {"out_hw": (96, 96)}, {}, False),
        ("N-256 off (CONV_VARIANT 0)", plan("s2d", 256, 128, 3, 0), (1, 97, 97, 512), None, lambda B: {"out_hw": (96, 96)},
         {"CONV_VARIANT": {"value": 0}}, False),
        ("N-256 convT 64->256 four phases", plan("convT", 256, 64, 3, 0), (1, 64, 64, 64), None, none, {}, False),
        ("dual convT 64->128 @64", plan("convT", 128, 64, 3, 0), (1, 64, 64, 64), None, none, {}, False),
        ("dual stats", plan("convT", 128, 64, 3, 0), (2, 64, 64, 64), None, lambda B: {"stats": True}, {}, False),
        ("dual off -> four phases", plan("convT", 128, 64, 3, 0), (1, 64, 64, 64), None, none, {"DUAL_CONVT": {"value": False}}, False),
        ("up9 convT 64->128 @90", plan("convT", 128, 64, 3, 0), (1, 90, 90, 64), None, none, {}, False),
        ("up9 stats noise", plan("convT", 128, 64, 3, 0), (2, 90, 90, 64), None,
         lambda B: {"stats": True, "noise": fake(B, 1, 180, 180), "noise_weight": 0.1, "bias": fake(128), "act": ops.ACT_LRELU}, {}, False),
        ("up9 refused: in_ss", plan("convT", 128, 64, 3, 0), (1, 90, 90, 64), None, ss(64), {}, False),
        ("up9 refused: residual", plan("convT", 128, 64, 3, 0), (1, 90, 90, 64), None,
         lambda B: {"residual": fake(B, 180, 180, 128)}, {}, False),
        ("up9 refused: PReLU", plan("convT", 128, 64, 3, 0), (1, 90, 90, 64), None,
         lambda B: {"act": ops.ACT_PRELU, "prelu": fake(128)}, {}, False),
        ("up9 refused: padding", plan("convT", 128, 64, 3, 0), (1, 90, 90, 64), None, lambda B: {"pad_mode": ops.PAD_REPLICATE}, {}, False),
        ("up9 off", plan("convT", 128, 64, 3, 0), (1, 90, 90, 64), None, none, {"UP9": {"value": False}}, False),
        ("up9 Cout 64 (no dual form)", plan("convT", 64, 32, 3, 0), (1, 120, 120, 32), None, none, {}, False),
        ("convT four phases, stats", plan("convT", 64, 32, 3, 0), (1, 17, 19, 32), None, lambda B: {"stats": True}, {}, False),
        ("Winograd 256->256 @64", plan("conv", 256, 256, 3, 0), (1, 64, 64, 256), None, none, {}, False),
        ("Winograd in_ss stats", plan("conv", 256, 256, 3, 0), (2, 64, 64, 256), None,
         lambda B: {"in_ss": fake(B, 256, 2), "in_act": ops.ACT_LRELU, "stats": True}, {}, False),
        ("Winograd dgrad 128->256", plan("dgrad", 128, 256, 3, 0), (1, 64, 64, 128), None, none, {}, False),
        ("Winograd Cin 1056", plan("conv", 128, 1056, 3, 0), (1, 64, 64, 1056), None, none, {}, False),
        ("Winograd refused: in_ss, Cin 1056", plan("conv", 128, 1056, 3, 0), (1, 64, 64, 1056), None, ss(1056), {}, False),
        ("Winograd off", plan("conv", 256, 256, 3, 0), (1, 64, 64, 256), None, none, {"WINO": {"value": False}}, False),
        ("1x1 streaming", plan("conv", 64, 32, 1, 0), (1, 40, 40, 32), None, none, {}, False),
        ("1x1 streaming in_res", plan("conv", 64, 32, 1, 0), (2, 40, 40, 32), None,
         lambda B: {"in_ss": fake(B, 32, 2), "in_res": fake(B, 40, 40, 32), "in_act": ops.ACT_PRELU, "in_prelu": fake(32)}, {}, False),
        ("1x1 in_res without in_ss: error", plan("conv", 64, 32, 1, 0), (1, 40, 40, 32), None,
         lambda B: {"in_res": fake(B, 40, 40, 32)}, {}, False),
        ("1x1 streaming off", plan("conv", 64, 32, 1, 0), (1, 40, 40, 32), None, none, {"STREAM_1X1": {"value": False}}, False),
        ("1x1 dgrad", plan("dgrad", 64, 32, 1, 0), (1, 40, 40, 64), None, none, {}, False),
        ("variant 5 s2d 32->32", plan("s2d", 32, 32, 3, 0), (1, 21, 21, 128), None, lambda B: {"out_hw": (20, 20)}, {}, False),
        ("variant 5 dgradT", plan("dgradT", 32, 32, 3, 0), (1, 21, 21, 128), None, none, {}, False),
        ("variant 6 conv 32->32", plan("conv", 32, 32, 3, 0), (1, 50, 50, 32), None, none, {}, False),
        ("variant 6 dgrad 64->32", plan("dgrad", 64, 32, 3, 0), (1, 50, 50, 64), None, none, {}, False),
        ("dgrad_s2d four groups", plan("dgrad_s2d", 128, 64, 3, 0), (1, 20, 20, 128), None, lambda B: {"out_hw": (41, 39)}, {}, False),
        ("dgrad_s2ds stacked", plan("dgrad_s2ds", 64, 32, 3, 0), (1, 20, 20, 64), None, lambda B: {"out_hw": (21, 20)}, {}, False),
        ("dgradT 128->64", plan("dgradT", 128, 64, 3, 0), (1, 33, 33, 512), None, none, {}, False),
        ("exact fp32", plan("conv", 128, 128, 3, 2), (1, 32, 32, 128), None, lambda B: {"stats": True}, {}, False),
        ("exact fp32 convT", plan("convT", 128, 64, 3, 2), (1, 90, 90, 64), None, none, {}, False),
        ("variant 7 fp16 on fp32 storage", plan("conv", 128, 128, 3, 3), (1, 256, 256, 128), None, none, {}, False),
        ("variant 7 bf16 on fp32 storage", plan("conv", 128, 128, 3, 1), (1, 256, 256, 128), None, none, {}, False),
        ("variant 7 off", plan("conv", 128, 128, 3, 3), (1, 256, 256, 128), None, none, {"TALL_TILE_SINGLE": {"value": False}}, False),
        ("variant 9 k64 fp16", plan("conv", 128, 128, 3, 3), (1, 256, 256, 128), f16, none, {}, False),
        ("variant 9 k64 bf16 stats", plan("conv", 128, 128, 3, 1), (1, 256, 256, 128), bf16, lambda B: {"stats": True}, {}, False),
        ("k64 off on half storage", plan("conv", 128, 128, 3, 3), (1, 256, 256, 128), f16, none, {"K64": {"value": False}}, False),
        ("k64 N-256 fp16", plan("s2d", 256, 128, 3, 3), (1, 97, 97, 512), f16, lambda B: {"out_hw": (96, 96)}, {}, False),
        ("k64 N-256 bf16", plan("s2d", 256, 128, 3, 1), (1, 97, 97, 512), bf16, lambda B: {"out_hw": (96, 96)}, {}, False),
        ("k64 N-256 conv 256->256 bf16", plan("conv", 256, 256, 3, 1), (1, 128, 128, 256), bf16, none, {}, False),
        ("k64 dual fp16", plan("convT", 128, 64, 3, 3), (1, 64, 64, 64), f16, none, {}, False),
        ("k64 dual bf16 stats", plan("convT", 128, 64, 3, 1), (2, 64, 64, 64), bf16, lambda B: {"stats": True}, {}, False),
        ("k64 convT 64->256 four phases fp16", plan("convT", 256, 64, 3, 3), (1, 64, 64, 64), f16, none, {}, False),
        ("single pass, thin layer", plan("conv", 64, 64, 3, 3), (1, 64, 64, 64), f16, none, {}, False),
        ("storage / mode mismatch: error", plan("conv", 128, 128, 3, 1), (1, 32, 32, 128), f16, none, {}, False),
        ("too few input channels: error", plan("conv", 128, 128, 3, 0), (1, 32, 32, 96), None, none, {}, False),
        ("batch-aware K split 256->256 @64 x2", plan("conv", 256, 256, 3, 0), (2, 64, 64, 256), None, none, {}, True),
        ("batch-aware K split off (Winograd)", plan("conv", 256, 256, 3, 0), (2, 64, 64, 256), None, none, {"KSPLIT": {"value": False}}, True),
        ("batch-aware Winograd K split 512->512 @32 x2", plan("dgrad", 512, 512, 3, 0), (2, 32, 32, 512), None, none, {}, True),
        ("batch-aware K split 512->512 @16 x2", plan("dgrad", 512, 512, 3, 0), (2, 16, 16, 512), None, none, {}, True),
        ("batch-aware k64 N-256 K split", plan("conv", 256, 512, 3, 1), (2, 96, 96, 512), bf16, none, {}, True),
        ("batch-aware K split 512->512 @8 x2", plan("conv", 512, 512, 3, 0), (2, 8, 8, 512), None, none, {}, True),
        ("batch-aware K split off 512->512 @8 x2", plan("conv", 512, 512, 3, 0), (2, 8, 8, 512), None, none,
         {"KSPLIT": {"value": False}}, True),
        ("batch-aware K split s2d 128->256 @16 x2", plan("s2d", 256, 128, 3, 0), (2, 17, 17, 512), None,
         lambda B: {"out_hw": (16, 16)}, {}, True),
        ("batch-aware N-256 under-filled", plan("s2d", 256, 128, 3, 0), (2, 97, 97, 512), None, lambda B: {"out_hw": (96, 96)},
         {"KSPLIT": {"value": False}}, True),
        ("batch-aware N-256 filled", plan("s2d", 256, 128, 3, 0), (8, 97, 97, 512), None, lambda B: {"out_hw": (96, 96)}, {}, True),
        ("batch-aware dgrad_s2d K split", plan("dgrad_s2d", 128, 128, 3, 0), (2, 8, 8, 128), None, lambda B: {"out_hw": (16, 16)}, {}, True),
        ("batch-aware convT 256->256 @8", plan("convT", 256, 256, 3, 0), (2, 8, 8, 256), None, none, {}, True),
        ("batch-aware bf16 train storage", plan("conv", 256, 256, 3, 1), (2, 32, 32, 256), bf16, none, {}, True),
        ("batch-aware 1x1", plan("conv", 256, 256, 1, 0), (2, 16, 16, 256), None, none, {}, True),
        ("batch-aware exact fp32", plan("conv", 256, 256, 3, 2), (2, 16, 16, 256), None, none, {}, True),
    ]
    out = {}
    for name, pl, shape, dtype, kw, switches, aware in cases:
        saved = {n: dict(getattr(ops, n)) for n in switches}
        for n, v in switches.items():
            getattr(ops, n).update(v)
        try:
            x = fake(*shape, dtype=dtype or torch.float32)
            with (ops.batch_aware() if aware else contextlib.nullcontext()):
                assert name not in out
                out[name] = _launch(ops, ops.lib, pl, x, kw(shape[0]))
        finally:
            for n, v in saved.items():
                getattr(ops, n).update(v)
    out["_packs"] = {"%s %d->%d k%d mode %d" % (k[0], k[2], k[1], k[3], k[4]):
                     (None if pl.precision == 2 else {str(n): int(t.numel()) for n, t in pl._packs.items()})
                     for k, pl in plans.items()}
    return out


def _struct(j, names):
    return {f: (_ptr(getattr(j, f), names) if t is ctypes.c_void_p else getattr(j, f)) for f, t in type(j)._fields_}


def record_repack(ops):
    """repack_plans / run_repack over plans that hold every pack key: the job rows and the per-plan launches, in order"""
    from ppst_amd import _lib
    plans = []
    for mode in (0, 1, 3):
        mk = lambda kind, cout, cin, k=3: ops.ConvPlan(torch.empty(cout, cin, k, k), kind=kind, scale=0.125 * (len(plans) + 1), precision=mode)
        for kind, cout, cin, k in (("conv", 64, 64, 3), ("conv", 128, 64, 3), ("conv", 256, 64, 3), ("conv", 64, 32, 1), ("s2d", 128, 64, 3),
                                   ("convT", 128, 64, 3), ("convT", 256, 64, 3), ("convT", 64, 32, 3), ("dgrad", 128, 64, 3),
                                   ("dgrad", 64, 128, 1), ("dgrad_s2d", 128, 64, 3), ("dgrad_s2ds", 64, 32, 3), ("dgradT", 128, 64, 3)):
            pl = mk(kind, cout, cin, k)
            for bn in (64, 128, 256):
                if bn >= pl.bn and (bn < 256 or pl.cout % 256 == 0):
                    pl.pack_for(bn)
            if pl.steps_dual is not None:
                pl.pack_dual()
            if mode != 0 and pl.steps_k64 is not None:
                for bn in (128, 256):
                    if bn < 256 or pl.cout % 256 == 0:
                        pl.pack_k64(bn)
            if mode != 0 and pl.steps_dual_k64 is not None:
                pl.pack_k64(256, dual=True)
            if mode == 0 and pl.steps_up9 is not None:
                pl.pack_up9()
            if mode == 0 and pl.kind in ("conv", "dgrad") and pl.k == 3 and pl.cout >= 128:
                pl.pack_wino()
            plans.append(pl)
    plans.append(ops.ConvPlan(torch.empty(64, 64, 3, 3), kind="conv", precision=2))        # (exact fp32: nothing to repack)
    names = {}
    for i, pl in enumerate(plans):
        for p, n in _names(pl, {}).items():
            names[p] = (names[p] + "|" if p in names else "") + n.replace("plan.", "p%d." % i)
    proxy = ops.lib

    def calls():
        out = []
        for name, args, _ in proxy.calls:
            row = {"entry": name, "args": _call_args(args, names)}
            if name in ("ppst_conv_pack_batch", "ppst_upscale_weight_batch"):
                cls = _lib.PackJob if name == "ppst_conv_pack_batch" else _lib.UpscaleJob
                row["args"][0] = "table"
                row["jobs"] = [_struct(j, names) for j in (cls * args[1]).from_address(args[0].value)]
            out.append(row)
        proxy.calls.clear()
        return out
    proxy.calls.clear()
    tables = ops.repack_plans(plans)
    first = calls()
    ops.run_repack(tables)
    again = calls()
    return {"packs": [None if pl.precision == 2 else {str(k): int(v.numel()) for k, v in pl._packs.items()} for pl in plans],
            "repack_plans": first, "run_repack_equals_repack_plans": again == first}


def record():
    with host_only_ops() as (ops, proxy):
        return {"tables": record_tables(ops), "launches": record_launches(ops), "repack": record_repack(ops)}


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "conv_plan_parent.json")
    with open(path, "w") as f:
        json.dump(record(), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path)
