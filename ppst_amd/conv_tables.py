"""Step tables of the fused conv (ppst_conv2d_mfma, include/ppst_hip.h) -- pure host code: Python lists and ints, no device.

A step ``(chan, dy, dx, first)`` reads 32 input channels from ``chan`` at pixel offset (dy, dx); its source ``(c, ky, kx)`` names
the weights it multiplies them with: ``wsrc[n * sn + (c + j) * sc + ky * sy + kx * sx]`` for output channel n and j < 32, with
``wstrides = (sn, sc, sy, sx)``; c = -1 is a zero-weight step.  ``first`` opens a chunk (the steps of one 32-channel slice).
Groups are output phases: group g = (py, px) writes the outputs (2 y + py, 2 x + px).

One builder per kind returns a ``Kind``; ``build`` encodes its tables and derives every scalar the launches read.
"""
import collections
import math
import types

# steps / src: the main table.  cout, cin: the roles in the LAUNCH (gradient kinds swap them).  wsource: which tensor the strides
# index -- "param" (the parameter), "flip" (the parameter from its last tap, negative tap strides), "up4" (the 4x4 kernel of the
# fused upscale, (Cin, Cout, 4, 4), scale folded in), "stack" (the phase-stacked 2x2 kernel, (4 Cin, Cout, 2, 2)).
# dual: (steps, src) of the phase-pair form; up9: steps of the nine-product form (convT only).
Kind = collections.namedtuple("Kind", "steps src wstrides n_groups halo cout cin wsource dual up9", defaults=(None, None))

PAD = [(0, 0, 0, 0)] * 4          # the kernel prefetches the descriptor of step s + 3 without a bounds test


def _table():
    return [], []


def _chunk(tab, chan, c, taps):
    """one chunk: a step per tap (dy, dx, ky, kx); None is a zero-weight step at offset (0, 0)"""
    for i, t in enumerate(taps):
        dy, dx, ky, kx = t or (0, 0, 0, 0)
        tab[0].append((chan, dy, dx, 1 if i == 0 else 0))
        tab[1].append((c if t else -1, ky, kx))


def conv(cout, cin, k):
    assert k in (1, 3)
    tab = _table()
    for c in range(0, cin, 32):
        _chunk(tab, c, c, [(ky - k // 2, kx - k // 2, ky, kx) for ky in range(k) for kx in range(k)])
    return Kind(*tab, (cin * k * k, k * k, k, 1), 1, 0 if k == 1 else 1, cout, cin, "param")


def s2d(cout, cin, k):
    """3x3 stride 2 over the space-to-depth input: tap k = 2 e + p reads phase p at offset e"""
    assert k == 3
    tab = _table()
    for py in range(2):
        for px in range(2):
            for c in range(0, cin, 32):
                taps = [(ey, ex, 2 * ey + py, 2 * ex + px) for ey in range(2 - py) for ex in range(2 - px)]
                # the (1,1) phase has a single tap: a zero-weight step pads the chunk (8-row tile kernels need >= 2 steps per chunk)
                _chunk(tab, (py * 2 + px) * cin + c, c, taps + [None] * (py * px))
    return Kind(*tab, (cin * 9, 9, 3, 1), 1, 1, cout, cin, "param")


def convT(cout, cin, k):
    """the fused 4x4 stride-2 transposed conv, F.conv_transpose2d(x, w4, stride=2, padding=1): oy = 2 iy - 1 + ky"""
    assert k == 3
    taps = {0: [(-1, 3), (0, 1)], 1: [(0, 2), (1, 0)]}
    tab, dual, up9 = _table(), None, None
    for a in range(2):
        for b in range(2):
            for c in range(0, cin, 32):
                _chunk(tab, c, c, [(dy, dx, ky, kx) for dy, ky in taps[a] for dx, kx in taps[b]])
    if cout % 128 == 0:
        # TWO row phases whose N tile holds both column phases (ppst_conv_args.dual_b): a step is a tap row dy with one tap column
        # per column phase -- the per-element tap order stays (dy major), outputs bit-identical
        dual = _table()
        pairs = [((dx0 + 1) | ((dx1 + 1) << 8), kx0 | (kx1 << 8)) for (dx0, kx0), (dx1, kx1) in zip(taps[0], taps[1])]
        for a in range(2):
            for c in range(0, cin, 32):
                _chunk(dual, c, c, [(dy, dx, ky, kx) for dy, ky in taps[a] for dx, kx in pairs])
    if cout % 64 == 0:
        # variant 11: per chunk the four input shifts; the u types each shift feeds are the kernel's (ppst_hip.h)
        up9 = _table()
        for c in range(0, cin, 32):
            _chunk(up9, c, c, [(dy, dx, 0, 0) for dy, dx in ((0, 0), (-1, 0), (0, -1), (-1, -1))])
        up9 = up9[0]
    return Kind(*tab, (16, cout * 16, 4, 1), 4, 1, cout, cin, "up4", dual, up9)


def dgrad(cout, cin, k):
    """input gradient of a stride-1 conv (zero padding): a conv of dY with the transposed, flipped weights
    Wd[c][n][ky][kx] = W[n][c][k-1-ky][k-1-kx] -- same memory, other strides; the reduction runs over the forward's Cout"""
    assert cout % 32 == 0
    t = conv(cin, cout, k)
    return t._replace(wstrides=(k * k, cin * k * k, -k, -1), wsource="flip")


def dgrad_s2d(cout, cin, k):
    """input gradient of the stride-2 3x3 conv: element i = 2 q + p of the (blurred) input grid receives
    sum_{ky = p (mod 2)} W[.,.,ky,.]^T dY[q - ky // 2] -> 4 output phases scattered with stride 2; groups padded to 4 steps per chunk"""
    assert k == 3 and cout % 32 == 0
    taps = {0: [(0, 0), (-1, 2)], 1: [(0, 1)]}
    tab = _table()
    for py in range(2):
        for px in range(2):
            for c in range(0, cout, 32):
                tl = [(dy, dx, ky, kx) for dy, ky in taps[py] for dx, kx in taps[px]]
                _chunk(tab, c, c, tl + [None] * (4 - len(tl)))
    return Kind(*tab, (9, cin * 9, 3, 1), 4, 1, cin, cout, "param")          # n' = c (stride 9), c' = n (stride cin * 9), no flip


def dgrad_s2ds(cout, cin, k):
    """the same input gradient with the four output phases STACKED as 4 x Cin output channels of ONE stride-1 conv with 2 x 2 taps
    (offsets 0 / -1 per axis), followed by ops.depth_to_space: one group, every step real"""
    assert k == 3 and cout % 32 == 0
    tab = _table()
    for c in range(0, cout, 32):
        _chunk(tab, c, c, [(-ty, -tx, ty, tx) for ty in range(2) for tx in range(2)])
    return Kind(*tab, (cout * 4, 4, 2, 1), 1, 1, 4 * cin, cout, "stack")


def dgradT(cout, cin, k):
    """input gradient of 'convT': a stride-2 4x4 conv (pad 1) of dY over the space-to-depth copy of dY: oy = 2 iy - 1 + ky ->
    (dq, phase, ky) per axis in {(-1,1,0), (0,0,1), (0,1,2), (+1,0,3)}"""
    assert k == 3 and cout % 32 == 0
    taps = {0: [(0, 1), (1, 3)], 1: [(-1, 0), (0, 2)]}
    tab = _table()
    for py in range(2):
        for px in range(2):
            for c in range(0, cout, 32):
                _chunk(tab, (py * 2 + px) * cout + c, c, [(dqy, dqx, ky, kx) for dqy, ky in taps[py] for dqx, kx in taps[px]])
    return Kind(*tab, (cout * 16, 16, 4, 1), 1, 1, cin, cout, "up4")       # w4[c][n][ky][kx]: output channel = c, reduction = n


KINDS = {f.__name__: f for f in (conv, s2d, convT, dgrad, dgrad_s2d, dgrad_s2ds, dgradT)}


def encode(steps, n_groups, k64=False):
    """device rows (chan, dy, dx, flags) + PAD.  flags: bit 0 = this step opens a chunk; bit 1 = the NEXT step of the group opens
    one, bits 8.. = its channel offset (lets the kernel request a chunk's activations a step early); k64: bit 2 = parity of the
    chunk within its group"""
    per = len(steps) // n_groups
    enc, chunk = [], -1
    for i, (c, dy, dx, f) in enumerate(steps):
        chunk = f - 1 if i % per == 0 else chunk + f
        nxt = steps[i + 1] if (i + 1) % per else None
        ahead = (2 | (nxt[0] << 8)) if nxt is not None and nxt[3] else 0
        enc.append((c, dy, dx, f | ahead | (((chunk & 1) << 2) if k64 else 0)))
    return enc + PAD


def k64(steps, src, n_groups):
    """(steps, src) of the 64-channel-step form: every second 32-channel chunk of a group opens a 64-channel step group with the
    same taps (needs an even chunk count per group and plain 32-channel chunk order)"""
    per = len(steps) // n_groups
    keep, chunk = [], -1
    for i, t in enumerate(steps):
        chunk = t[3] - 1 if i % per == 0 else chunk + t[3]
        if chunk % 2 == 0:
            keep.append(i)
    return [steps[i] for i in keep], [src[i] for i in keep]


def _chunk_starts(steps):
    return [i for i, t in enumerate(steps) if t[3]] + [len(steps)]


def build(kind, cout, cin, k):
    """the record of one (kind, weight shape): ``cout, cin, k`` are the FORWARD weight's (Cout, Cin, k)"""
    if kind not in KINDS:
        raise ValueError(kind)
    assert cin % 32 == 0, "fused conv needs Cin %% 32 == 0 (got %d)" % cin
    t = KINDS[kind](cout, cin, k)
    r = types.SimpleNamespace(kind=kind, cout=t.cout, cin=t.cin, k=k, bn=128 if t.cout >= 128 else 64, n_groups=t.n_groups,
                              halo=t.halo, wstrides=t.wstrides, wsource=t.wsource, src=t.src)
    r.w4_shape = (cin, cout, 4, 4) if kind == "dgradT" else None
    ns = r.nsteps = len(t.steps) // t.n_groups
    r.max_chan = max(s[0] for s in t.steps)             # highest first-channel of any step (the input needs max_chan + 32)
    r.flop_steps = sum(1 for s in t.src if s[0] >= 0) // t.n_groups
    # every element of the weight tensor is the target of exactly one (step, output channel, k) of the table: the weight gradient's
    # split reduction then WRITES all of dW and no zero fill has to run in front of it
    live = [s for s in t.src if s[0] >= 0]
    target = math.prod(r.w4_shape) if r.w4_shape else cout * cin * k * k          # what conv_wgrad(plan, ...) returns
    r.full_cover = bool(t.n_groups == 1 and len(set(live)) == len(live) and len(live) * 32 * t.cout == target)
    r.chunk_start = _chunk_starts(t.steps)
    lens = [b - a for a, b in zip(r.chunk_start[:-1], r.chunk_start[1:])]
    r.chunk_starts0 = _chunk_starts(t.steps[:ns])       # chunk starts of ONE group (every group has the same)
    r.chunks_per_group = len(r.chunk_starts0) - 1       # ring depth hint for the kernel
    r.max_chunk_steps, r.min_chunk_steps = max(lens), min(lens)
    r.early_a = 1 if (min(lens) >= 2 and ns >= 3) else 0
    r.steps = encode(t.steps, t.n_groups)
    r.steps_dual, r.src_dual = (encode(t.dual[0], 2), t.dual[1]) if t.dual else (None, None)
    r.steps_up9 = encode(t.up9, 1) if t.up9 else None
    r.steps_k64 = r.src_k64 = r.steps_dual_k64 = r.src_dual_k64 = r.chunk_starts0_k64 = None
    if kind in ("conv", "s2d", "convT") and t.halo == 1 and t.cin % 64 == 0 and t.cout >= 128 and r.early_a:
        st, r.src_k64 = k64(t.steps, t.src, t.n_groups)
        r.steps_k64 = encode(st, t.n_groups, k64=True)
        r.chunk_starts0_k64 = _chunk_starts(st[:len(st) // t.n_groups])
        if t.dual:
            st, r.src_dual_k64 = k64(*t.dual, 2)
            r.steps_dual_k64 = encode(st, 2, k64=True)
    return r
