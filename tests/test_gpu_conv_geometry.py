"""GPU: the input side of every forward conv kernel family -- staging, padding, normalise-on-load, tile seams, ragged tiles, channel
slices and channel counts (tests/conv_geom_cases.py) -- one launch per case, with the kernel pinned by the family's switches
(tests/test_conv_geom_cases_cpu.py shows without a device that every case reaches the launch its family names).

  * against float64 torch of the operation itself at the bars of tests/gpu_diag.py t_conv (3e-5 bf16x3, 2e-2 / 3e-3 single-pass
    bf16 / fp16, 5e-6 fp32; the statistics' sums at 1e-5, in the single-pass modes at the mode's bar): the whole output, and the
    border and tile-seam rows / columns again against their own largest value;
  * the output is the caller's: a channel slice inside a buffer pre-filled with one NaN bit pattern, 64 guard pixels in front of
    and behind it and guard channels around the slice -- every guard element keeps its bits, no sentinel stays inside the output,
    and the output has the family's storage type;
  * the families that compute the same sum agree to the bit in every case they share (statistics to the bar);
  * image 1 of every 33 x 35 case, launched alone, equals image 1 of the batch to the bit, statistics included: which kernel runs
    is a function of one image (ops.ConvPlan.choose_kernel).

Every case is launched once (module fixture); a launch is microseconds, most of the module's time is the float64 reference on the
host.  Nothing here provokes a fault: reads beyond an image are the kernels' own range-checked buffer loads, every pointer is
aligned as the entry point requires, and the first launch that raises ends the run.

Largest error per family on an MI355X, relative to max |ref| (output / border and seams / sum / sum of squares), as first measured:
  tile64          4.9e-06 / 4.9e-06 / 3.6e-06 / 4.5e-06
  tile128         5.5e-06 / 4.5e-06 / 4.5e-06 / 5.4e-06
  tile256         5.1e-06 / 5.1e-06 / 3.1e-06 / 4.7e-06
  row8            5.1e-06 / 5.1e-06 / 3.1e-06 / 4.7e-06
  tile1x1         1.1e-05 / 1.1e-05 / 3.3e-06 / 4.1e-06
  tile_s2d        4.3e-06 / 3.9e-06 / 3.9e-06 / 3.9e-06
  convT4          6.5e-06 / 6.1e-06 / 2.8e-06 / 2.5e-06
  n256            5.1e-06 / 5.1e-06 / 3.1e-06 / 4.7e-06
  dual            5.7e-06 / 5.7e-06 / 2.8e-06 / 3.3e-06
  up9             4.5e-06 / 4.2e-06 / 1.9e-06 / 2.5e-06
  stream1         1.1e-05 / 1.1e-05 / 3.3e-06 / 4.0e-06
  direct5         4.3e-06 / 3.9e-06 / 3.9e-06 / 3.9e-06
  direct3         4.9e-06 / 4.9e-06 / 3.6e-06 / 4.5e-06
  wino            5.4e-06 / 5.4e-06 / 4.6e-06 / 6.0e-06
  tile_bf16       4.0e-03 / 4.0e-03 / 1.9e-03 / 3.1e-03
  tile_fp16       5.6e-04 / 5.7e-04 / 2.8e-04 / 3.0e-04
  k64_n256_bf16   4.0e-03 / 3.7e-03 / 2.0e-03 / 3.0e-03
  k64_row24_fp16  5.3e-04 / 5.4e-04 / 2.5e-04 / 4.9e-04
  f32             1.2e-06 / 1.0e-06 / 3.4e-07 / 4.2e-07
  row32_bf16x1    2.3e-03 / 2.4e-03 / 2.1e-03 / 2.5e-03
(bars: 3e-5 and 1e-5 for the sums; tile_bf16, k64_n256_bf16 and row32_bf16x1 2e-2; tile_fp16 and k64_row24_fp16 3e-3; f32 5e-6 and 1e-5)
"""
import collections
import hashlib

import pytest
import torch

import conv_geom_cases as G

pytestmark = pytest.mark.gpu
GUARD_PX = 64
SENTINEL = {torch.float32: (torch.int32, 0x7FC0DEAD), torch.float16: (torch.int16, 0x7E5A), torch.bfloat16: (torch.int16, 0x7FD5)}
X_GUARD = 1.0e3                 # around the input: finite, and far from any input value

Result = collections.namedtuple("Result", "dtype bad errs stats sha sha_image1 guard_bad sentinel_inside alone error")


def _sha(t):
    t = t.contiguous()
    return hashlib.sha256(t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).numpy().tobytes()).hexdigest()


def _guarded(b, h, w, ld, dtype, dev):
    """(flat buffer of GUARD_PX + b h w + GUARD_PX pixels of ld elements, its (b, h, w, ld) middle)"""
    n = b * h * w
    buf = torch.empty((n + 2 * GUARD_PX) * ld, dtype=dtype, device=dev)
    return buf, buf[GUARD_PX * ld:(GUARD_PX + n) * ld].view(b, h, w, ld)


def _upload(s, dev):
    """a Slice of a CPU tensor -> the same slice of a device copy that sits between guard pixels"""
    b, h, w, ld = s.wide.shape
    buf, mid = _guarded(b, h, w, ld, s.wide.dtype, dev)
    buf.fill_(X_GUARD)
    mid.copy_(s.wide)
    return mid[..., s.lo:s.lo + s.width]


def _launch(ops, c, dev_t, plan, image=None):
    """one launch into a sentinel-filled guarded buffer -> (output on the CPU, raw statistics on the CPU, guard elements changed,
    sentinels left inside the output).  image: launch that image alone."""
    f = G.FAMILIES[c.family]
    _, (oh, ow), _ = G.geometry(c)
    sl = c.layout == "slices"
    ld, lo = c.cout + (G.OUT_EXTRA if sl else 0), (G.OUT_LO if sl else 0)
    t = dict(dev_t)
    nb = G.B
    if image is not None:
        nb = 1
        for k in ("x", "ss", "in_res", "res"):
            if k in t:
                t[k] = t[k][image:image + 1]
    buf, mid = _guarded(nb, oh, ow, ld, f.dtype, "cuda")
    bits_t, bits = SENTINEL[f.dtype]
    buf.view(bits_t).fill_(bits)
    t["out"] = mid[..., lo:lo + c.cout]
    y, st = G.call(ops, c, t, plan)
    assert y.data_ptr() == t["out"].data_ptr()
    raw = buf.view(bits_t).cpu()
    n = nb * oh * ow
    inner = raw[GUARD_PX * ld:(GUARD_PX + n) * ld].view(n, ld)
    guard_bad = int((raw[:GUARD_PX * ld] != bits).sum() + (raw[(GUARD_PX + n) * ld:] != bits).sum()
                    + (inner[:, :lo] != bits).sum() + (inner[:, lo + c.cout:] != bits).sum())
    inside = int((inner[:, lo:lo + c.cout] == bits).sum())
    return y.cpu(), st.cpu(), guard_bad, inside


@pytest.fixture(scope="module")
def results():
    """{case id: Result}: every case launched once (the 33 x 35 ones a second time on image 1 alone) and judged"""
    from ppst_amd import ops
    out, moved, plans, stopped = {}, {}, {}, None
    for c in G.CASES:
        f = G.FAMILIES[c.family]
        if stopped:
            out[c.id] = Result(None, None, None, None, None, None, None, None, None, "not run: %s" % stopped)
            continue
        name = G.conv_name(c)
        if name not in moved:
            t = G.make(c)
            moved[name] = {k: (_upload(v, "cuda") if isinstance(v, G.Slice) else v.to("cuda")) for k, v in t.items()}
        pkey = (f.kind, c.cin, c.cout, f.k, f.precision)
        try:
            if pkey not in plans:
                plans[pkey] = G.plan_of(ops, c, moved[name]["w"])
            y, st, guard_bad, inside = _launch(ops, c, moved[name], plans[pkey])
            alone = None
            if c.hw == G.BIG:
                y1, st1, g1, i1 = _launch(ops, c, moved[name], plans[pkey], image=1)
                alone = (_sha(y1[0]), _sha(st1[0]), g1, i1)
        except Exception as e:          # (no retry, and nothing more is launched)
            stopped = "%s raised %r" % (c.id, e)
            out[c.id] = Result(None, None, None, None, None, None, None, None, None, stopped)
            continue
        sums = st.double().sum(1)                        # (B, tiles, Cout, 2) -> per image and channel
        bad, errs = G.judge(c, y, sums)
        out[c.id] = Result(y.dtype, bad, errs, sums, _sha(y), (_sha(y[1]), _sha(st[1])), guard_bad, inside, alone, None)
    if not stopped:
        torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("cid", [c.id for c in G.CASES])
def test_case_against_float64(results, cid):
    c, r = G.by_id(cid), results[cid]
    assert r.error is None, r.error
    for what, (e, bar) in r.errs.items():
        print("%-52s %-7s rel %.3e (bar %.0e)" % (cid, what, e, bar))
    assert r.dtype == G.FAMILIES[c.family].dtype
    assert r.bad == [], r.bad
    assert r.guard_bad == 0, "%d guard elements around the output were written" % r.guard_bad
    assert r.sentinel_inside == 0, "%d output elements were never written" % r.sentinel_inside


@pytest.mark.parametrize("group", G.EQUAL, ids=lambda g: "=".join(g))
def test_direct_families_agree_to_the_bit(results, group):
    first = {G.conv_name(c): c for c in G.CASES if c.family == group[0]}
    for other in group[1:]:
        shared = [c for c in G.CASES if c.family == other and G.conv_name(c) in first]
        assert len(shared) >= 7, (other, len(shared))        # at the least the zero-padding, plain matrix and its layout case
        for c in shared:
            r, r0 = results[c.id], results[first[G.conv_name(c)].id]
            assert r.error is None and r0.error is None, (r.error, r0.error)
            assert r.sha == r0.sha, c.id
            bar = G.BAR_STATS[G.FAMILIES[c.family].precision]
            for i in (0, 1):
                e = ((r.stats[..., i] - r0.stats[..., i]).abs().max() / r0.stats[..., i].abs().max()).item()
                assert e <= bar, (c.id, i, e)


def test_one_image_alone_equals_its_place_in_the_batch(results):
    """the shard invariant: image 1 of every 33 x 35 case, launched alone -- output and tile statistics to the bit"""
    seen = 0
    for c in G.CASES:
        r = results[c.id]
        assert r.error is None, r.error
        if c.hw == G.BIG:
            seen += 1
            assert r.alone[:2] == r.sha_image1, c.id
            assert r.alone[2:] == (0, 0), (c.id, r.alone[2:])
        else:
            assert r.alone is None
    assert seen >= 2 * len(G.FAMILIES)               # (every family has its plain 33 x 35 case, dense and in slices)


def test_print_the_largest_error_per_family(results):
    """(what the module docstring records)"""
    for name in G.FAMILIES:
        worst = {}
        for c in G.CASES:
            r = results[c.id]
            assert r.error is None, r.error
            if c.family == name:
                for what, (e, bar) in r.errs.items():
                    worst[what] = max(worst.get(what, 0.0), e)
        print("  %-15s %.1e / %.1e / %.1e / %.1e" % (name, worst["output"], worst["border"], worst["sum"], worst["sumsq"]))
