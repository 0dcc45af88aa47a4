"""Run every case of tests/conv_epi_cases.py on the GPU and record the sha256 of each output and statistics tensor.

    python tests/conv_epi_record.py [OUT.json]        (default: tests/golden/conv_epilogue_parent.json)

The outputs of a conv launch are a function of its inputs alone (no atomics, fixed summation order), and the inputs come from a
seeded CPU generator, so two commits can be compared to the byte: tests/golden/conv_epilogue_parent.json was written by this tool
on an MI355X at commit 029de64, the last one with a copy of the epilogue per kernel family, before csrc/conv_common.h stated it
once; tests/test_gpu_conv_epilogue.py runs the working tree and asserts the same hashes.  Check out that commit, copy this file
and tests/conv_epi_cases.py over, build, and run it to see where the JSON comes from.
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch

import conv_epi_cases as CE

DOC = ("sha256 of the output / statistics tensor of every case of tests/conv_epi_cases.py, written by tests/conv_epi_record.py "
       "on an MI355X at commit 029de64 (the parent of the commit that added csrc/conv_common.h)")


def sha(t):
    if t is None:
        return None
    t = t.detach().cpu().contiguous()
    if t.dtype != torch.float32:
        t = t.view(torch.int16)              # (numpy has no bfloat16: the raw 16 bits)
    return hashlib.sha256(t.numpy().tobytes()).hexdigest()


def run_all(ops, device="cuda"):
    """-> {case id: (y, stats)} as CPU tensors; every case launched once"""
    out, moved = {}, {}
    for c in CE.CASES:
        name = CE.data_name(CE.FAMILIES[c.family])
        if name not in moved:
            moved[name] = {k: v.to(device) for k, v in CE.inputs(c).items()}
        y, st = CE.call(ops, c, moved[name])
        out[c.id] = (y.cpu(), None if st is None else st.cpu())
    torch.cuda.synchronize()
    return out


def record(ops):
    return {cid: {"y": sha(y), "stats": sha(st)} for cid, (y, st) in run_all(ops).items()}


if __name__ == "__main__":
    from ppst_amd import ops
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "conv_epilogue_parent.json")
    rec = record(ops)
    rec["_doc"] = DOC
    with open(path, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path, len(rec) - 1, "cases")
