"""Timing aid (GPU): ops.guided_filter at one radius on a batch of square images, HIP events around repeated calls after warm-up.

    python tests/gf_radius_time.py B SIDE R            # e.g. 4 1024 60, 4 1536 90
    GF_VS="32,64;64,128" python tests/gf_radius_time.py 4 1536 90    # rows per block of the two fused launches, one line per pair

Five groups of ten calls; the line gives the fastest, the median and the slowest group in ms per call.  PPST_HIP_LIB selects
another build of the library (ppst_amd/_lib.py), which is how two builds are compared on one box.  tests/gf_time.py is the
radius-30 form of this and stays as it is."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from ppst_amd import ops  # noqa: E402
from ppst_amd._lib import lib  # noqa: E402

B, S, R = (int(v) for v in sys.argv[1:4])
EPS = (0.02 * 255) ** 2
gen = torch.Generator(device="cuda").manual_seed(0)
g = torch.randint(0, 256, (B, S, S, 3), dtype=torch.uint8, device="cuda", generator=gen)
s = torch.randint(0, 256, (B, S, S, 3), dtype=torch.uint8, device="cuda", generator=gen)
pairs = [tuple(int(v) for v in p.split(",")) for p in os.environ["GF_VS"].split(";")] if os.environ.get("GF_VS") else [(0, 0)]
for vs1, vs2 in pairs:
    lib.ppst_guided_filter_tune(vs1, vs2)
    for _ in range(5):
        ops.guided_filter(g, s, R, EPS)
    ms = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            ops.guided_filter(g, s, R, EPS)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / 10)
    ms.sort()
    print("guided filter r=%d B=%d %dx%d vs=(%d, %d): min %.3f  median %.3f  max %.3f ms" % (R, B, S, S, vs1, vs2, ms[0], ms[2], ms[4]), flush=True)
lib.ppst_guided_filter_tune(0, 0)
