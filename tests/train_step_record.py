"""Record what four iterations of the train step do on the GPU: every library entry point they call, in order, with its scalar
arguments, and the bits they leave behind.

    python tests/train_step_record.py [OUT.json]        (default: train_step_record.json in the working directory)

The model, inputs and noise are those of tests/test_gpu_gstep.py::test_generator_adam_step_and_alternation (seed 17,
gstep_diag.gstep_inputs()); ``PPSTOptimizer(m, R1_once_every=2)`` runs D, G, D with its lazy R1 pass, G.  While they run, ops.lib
is a proxy that forwards every call and keeps the entry's name and arguments: integers and floats as they are, pointers only as
null / non-null (device addresses depend on the allocator's history), structures field by field.  Afterwards the flat parameters
and Adam moments of the four networks are recorded as SHA-256 and every returned loss as ``float.hex()``.

Everything recorded is discrete, so two commits whose host code is meant to drive the same kernels can be compared to the byte:
check out the older commit, copy this file over, run it there and here, and compare the two files.  profiles/train_host_refactor.txt
holds the digests of one such pair.
"""
import ctypes
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in (ROOT, os.path.join(ROOT, "tests")):
    if d not in sys.path:
        sys.path.insert(0, d)

import torch

POINTERS = (ctypes.c_void_p, ctypes.c_char_p, ctypes._Pointer)


def _is_pointer_type(t):
    return t is not None and issubclass(t, POINTERS)


def _struct(s):
    return {f: (bool(getattr(s, f)) if _is_pointer_type(t) else _value(getattr(s, f))) for f, t in type(s)._fields_}


def _value(v, argtype=None):
    """one argument as plain data; ``argtype``: the entry's declared type of it (an address may arrive as a plain integer)"""
    if hasattr(v, "_obj"):                         # ctypes.byref(structure or number), as it stands when the call is made
        return _value(v._obj)
    if isinstance(v, ctypes.Structure):
        return _struct(v)
    if isinstance(v, ctypes.Array):                # a host array of the caller's
        return [bool(e) for e in v] if _is_pointer_type(v._type_) else [_value(e) for e in v]
    if _is_pointer_type(argtype) or isinstance(v, POINTERS):
        return bool(v.value if isinstance(v, ctypes.c_void_p) else v)
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    if isinstance(v, ctypes._SimpleCData):
        return v.value
    return "?" + type(v).__name__


class LibRecorder:
    """ops.lib with a memory: every entry runs as before and leaves (name, arguments) in ``calls``."""

    def __init__(self, real):
        self._real, self.calls = real, []

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        types = fn.argtypes or ()

        def entry(*args):
            row = [_value(v, types[i] if i < len(types) else None) for i, v in enumerate(args)]
            for v in args:                         # (the K-split cuts live in a host array of the caller's: read them now)
                if hasattr(v, "_obj") and getattr(v._obj, "ksplit_starts", None):
                    row.append(list((ctypes.c_int32 * (v._obj.ksplit + 1)).from_address(v._obj.ksplit_starts)))
            self.calls.append([name, row])
            return fn(*args)
        self.__dict__[name] = entry
        return entry


def _sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def record():
    import gstep_diag as D
    from ppst_amd import ops, weights as W
    from ppst_amd.ppst_model import Options, create_model
    from ppst_amd.train_g import PPSTOptimizer
    sd = W.make_state_dict(17, bias_std=0.1, noise_weight=0.1)
    m = create_model(Options(training_stage=2, lambda_Cycwarp=0.0), state_dict=sd, with_D=True, with_nce=True)
    real, mask, noise = D.gstep_inputs()
    m.noise = {k: v.cuda() for k, v in noise.items()}
    opt = PPSTOptimizer(m, R1_once_every=2)
    data = {"real_A": real.cuda(), "mask_A": mask.cuda()}
    real_lib, losses = ops.lib, []
    ops.lib = rec = LibRecorder(real_lib)
    try:
        for step in range(4):
            out = opt.train_one_step(data, 2 * step)
            losses.append({k: float(v).hex() for k, v in sorted(out.items())})
        torch.cuda.synchronize()
    finally:
        ops.lib = real_lib
    owners = dict(opt.gen.fp, D=opt.dis)
    state = {k: {"flat": _sha(f.flat), "m": _sha(f.m), "v": _sha(f.v), "step": f.step_count} for k, f in sorted(owners.items())}
    return {"calls": rec.calls, "losses": losses, "state": state}


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else "train_step_record.json"
    res = record()
    with open(path, "w") as f:
        json.dump(res, f, indent=0, sort_keys=True)
        f.write("\n")
    with open(path, "rb") as f:
        digest = hashlib.sha256(f.read()).hexdigest()
    unknown = sorted({a for _, row in res["calls"] for a in row if isinstance(a, str) and a.startswith("?")})
    print("wrote %s: %d calls, sha256 %s%s" % (path, len(res["calls"]), digest, ("  UNRECORDED TYPES %s" % unknown) if unknown else ""))
