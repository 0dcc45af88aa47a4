"""CPU: what ops.ConvPlan builds is what it built before its host code was restated (tests/conv_plan_parent.json, written by
tests/conv_plan_record.py at commit adcf59b), and every kind's step table means the convolution it stands for."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

import conv_plan_record
import ppst_oracle as O
from ppst_amd import conv_tables

HERE = os.path.dirname(os.path.abspath(__file__))


def test_plans_launches_and_repack_jobs_equal_the_recorded_parent():
    with open(os.path.join(HERE, "conv_plan_parent.json")) as f:
        want = json.load(f)
    got = json.loads(json.dumps(conv_plan_record.record()))
    assert sorted(got) == sorted(want) == ["launches", "repack", "tables"]
    for part in sorted(want):
        assert sorted(got[part]) == sorted(want[part]), part
        for name in sorted(want[part]):
            assert got[part][name] == want[part][name], (part, name)
    # the matrix reaches every launch form (read from the recorded file: these hold for the parent's code too)
    seen = {(r["args"][0]["variant"], r["args"][0]["tile_rows"], r["args"][0]["dual_b"], r["args"][0]["k64"])
            for n, r in want["launches"].items() if n != "_packs" and "error" not in r}
    assert {(0, 16, 0, 0), (0, 8, 0, 0), (2, 16, 0, 0), (2, 16, 1, 0), (11, 15, 0, 0), (10, 16, 0, 0), (4, 16, 0, 0), (5, 16, 0, 0),
            (6, 16, 0, 0), (7, 32, 0, 0), (9, 24, 0, 1), (2, 16, 0, 1), (2, 16, 1, 1)} <= seen
    assert {r["args"][0]["ksplit"] for n, r in want["launches"].items() if n != "_packs" and "error" not in r} == {0, 2, 4, 8}
    assert {k for p in want["repack"]["packs"] if p for k in p} == {"64", "128", "256", "dual", "k64_128", "k64_256", "k64_dual", "up9", "wino"}
    assert want["repack"]["run_repack_equals_repack_plans"] is True


def test_conv_tables_is_host_code():
    assert not {"torch", "lib", "_lib", "ops"} & set(vars(conv_tables))
    r = conv_tables.build("convT", 128, 64, 3)
    assert all(isinstance(t, (list, type(None))) for t in (r.steps, r.steps_dual, r.steps_up9, r.steps_k64, r.steps_dual_k64, r.src))
    with pytest.raises(ValueError):
        conv_tables.build("conv2", 64, 64, 3)


# ---- meaning of a table: interpret it in float64, compare with torch in float64 --------------------------------------------
def _interpret(rec, x, wflat, tile, out_hw, base=0):
    """run the main table of ``rec`` over x (H, W, C): a step (chan, dy, dx) with source (c, ky, kx) adds the 32 input channels
    from ``chan`` at offset (dy, dx) times wflat[n * sn + (c + j) * sc + ky * sy + kx * sx]; c = -1 is a zero step; group
    g = (py, px) of four writes the outputs (2 y + py, 2 x + px) (include/ppst_hip.h).  ``base``: where in wflat the weight source
    starts (the flipped view starts at the parameter's last tap and indexes backwards)"""
    (th, tw), (oh, ow) = tile, out_hw
    H, W, _ = x.shape
    pad = 2 + max(th - H, tw - W, 0)
    xp = F.pad(x, (0, 0, pad, pad, pad, pad))               # zero padding, and tiles that reach past the input
    sn, sc, sy, sx = rec.wstrides
    n = base + torch.arange(rec.cout)[:, None] * sn + torch.arange(32)[None, :] * sc
    out = torch.zeros(oh, ow, rec.cout, dtype=torch.float64)
    assert len(rec.steps) == rec.n_groups * rec.nsteps + 4 and len(rec.src) == rec.n_groups * rec.nsteps
    for g in range(rec.n_groups):
        acc = torch.zeros(th, tw, rec.cout, dtype=torch.float64)
        for (chan, dy, dx, _), (c, ky, kx) in zip(rec.steps[g * rec.nsteps:(g + 1) * rec.nsteps], rec.src[g * rec.nsteps:]):
            if c < 0:
                continue
            patch = xp[pad + dy:pad + dy + th, pad + dx:pad + dx + tw, chan:chan + 32]
            idx = n + c * sc + ky * sy + kx * sx
            assert 0 <= int(idx.min()) and int(idx.max()) < wflat.numel()
            acc += patch @ wflat[idx].T
        if rec.n_groups == 1:
            assert (th, tw) == (oh, ow)
            out = acc
        else:
            py, px = divmod(g, 2)
            out[py::2, px::2] = acc[:(oh - py + 1) // 2, :(ow - px + 1) // 2]
    return out


def _nhwc(t):
    return t[0].permute(1, 2, 0).contiguous()


def _nchw(t):
    return t.permute(2, 0, 1)[None]


def _s2d(t):
    """(H, W, C) -> (ceil(H / 2), ceil(W / 2), 4 C), channel block py * 2 + px = input phase; zero where the input ends"""
    H, W, C = t.shape
    t = F.pad(t, (0, 0, 0, W % 2, 0, H % 2))
    return torch.cat([t[py::2, px::2] for py in range(2) for px in range(2)], dim=2)


def _stack_weight(w):
    """ppst_dgrad_s2d_stack_weight (include/ppst_hip.h): out[(py*2+px)*cin + n][c][ty][tx] = w[c][n][ky][kx], tap offset 0 with
    k = (p == 0 ? 0 : 1), offset 1 with k = 2 for p == 0 only, zero elsewhere"""
    cout, cin = w.shape[:2]
    out = torch.zeros(4, cin, cout, 2, 2, dtype=w.dtype)
    tap = {(0, 0): 0, (0, 1): 1, (1, 0): 2}                  # (t, p) -> k
    for (ty, py), ky in tap.items():
        for (tx, px), kx in tap.items():
            out[py * 2 + px, :, :, ty, tx] = w[:, :, ky, kx].T
    return out.reshape(4 * cin, cout, 2, 2)


def _grad(f, x, dy):
    x = x.clone().requires_grad_(True)
    return torch.autograd.grad(f(x), x, dy)[0]


CASES = [(kind, cout, cin, k) for kind in conv_tables.KINDS for cout in (32, 64) for cin in (32, 64)
         for k in ((1, 3) if kind in ("conv", "dgrad") else (3,))]


@pytest.mark.parametrize("kind,cout,cin,k", CASES)
def test_main_table_means_its_convolution(kind, cout, cin, k):
    """B = 1, extents 5 x 6 (odd and even: the phase edges); the stride-2 kinds pair 5 x 6 with the 10 x 12 layer above it, whose
    blurred copy -- what the 3x3 stride-2 conv reads -- is 11 x 13.  Bar: 1e-10 of max |reference| (both sides are double sums of
    at most a few thousand products)."""
    g = torch.Generator().manual_seed(cout * 7 + cin * 3 + k)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    w = rnd(cout, cin, k, k)
    rec = conv_tables.build(kind, cout, cin, k)
    w4 = O.upscale_weight(w) if k == 3 else None
    wflat = {"param": w, "flip": w, "up4": w4, "stack": _stack_weight(w) if k == 3 else None}[rec.wsource].reshape(-1)
    if kind == "conv":
        x = rnd(1, cin, 5, 6)
        ref, got = F.conv2d(x, w, padding=k // 2), _interpret(rec, _nhwc(x), wflat, (5, 6), (5, 6))
    elif kind == "s2d":
        x = rnd(1, cin, 11, 13)
        ref, got = F.conv2d(x, w, stride=2), _interpret(rec, _s2d(_nhwc(x)), wflat, (5, 6), (5, 6))
    elif kind == "convT":
        x = rnd(1, cin, 5, 6)
        ref, got = F.conv_transpose2d(x, w4, stride=2, padding=1), _interpret(rec, _nhwc(x), wflat, (5, 6), (10, 12))
    elif kind == "dgrad":
        dy = rnd(1, cout, 5, 6)
        ref = _grad(lambda x: F.conv2d(x, w, padding=k // 2), rnd(1, cin, 5, 6), dy)
        got = _interpret(rec, _nhwc(dy), wflat, (5, 6), (5, 6), base=k * k - 1)
    elif kind in ("dgrad_s2d", "dgrad_s2ds"):
        dy = rnd(1, cout, 5, 6)
        ref = _grad(lambda x: F.conv2d(x, w, stride=2), rnd(1, cin, 11, 13), dy)
        if kind == "dgrad_s2d":
            got = _interpret(rec, _nhwc(dy), wflat, (6, 7), (11, 13))
        else:                                               # the four phases stacked, then ops.depth_to_space
            st = _interpret(rec, _nhwc(dy), wflat, (6, 7), (6, 7))
            got = torch.zeros(12, 14, cin, dtype=torch.float64)
            for p in range(4):
                got[p // 2::2, p % 2::2] = st[:, :, p * cin:(p + 1) * cin]
            got = got[:11, :13]
    else:
        assert kind == "dgradT"
        dy = rnd(1, cout, 10, 12)
        ref = _grad(lambda x: F.conv_transpose2d(x, w4, stride=2, padding=1), rnd(1, cin, 5, 6), dy)
        got = _interpret(rec, _s2d(_nhwc(dy)), wflat, (5, 6), (5, 6))
    assert rec.max_chan + 32 == (4 if kind in ("s2d", "dgradT") else 1) * rec.cin
    assert tuple(_nchw(got).shape) == tuple(ref.shape)
    err = (_nchw(got) - ref).abs().max().item() / ref.abs().max().item()
    assert err <= 1e-10, err
