"""CPU: the cases, the judges and the bars of tests/test_gpu_region.py (tests/region_cases.py), the integer crop transform, and
what the region-swap entry points refuse without a GPU -- nothing here touches one.

  * per case, from the restatement alone: the exempt share stays at or below gf_cases.EXEMPT_CAP, and the float32 run of each
    judge passes its own bar; every seeded defect violates the bar on at least one case;
  * the table has the issue's sizes, angles, scales, placements, feathers and the extents around the kernels' tile edges, and the
    tile constants of the cases module are the ones in the sources;
  * imageio.crop_transform is the cases module's restatement, maps centre, side and angle back to within 2^-10 crop pixel over
    a 16384-pixel photo, and crop_transform_rule refuses s < 1 and s > 8;
  * both C entry points reject bad arguments before any launch; ops refuse CPU tensors and wrong dtypes; decode_region and
    simple_swap_region refuse from shapes and integers alone.
"""
import ctypes
import inspect
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gf_cases as G  # noqa: E402
import region_cases as C  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", C.ALL_CASES, ids=C.case_id)
def test_case_conditions_from_the_restatement_alone(case):
    E, P = C.extract_ref(case), C.paste_ref(case)
    print("%-24s extract: max|r32-r64| %.2e tau %.2e exempt %.4f   paste: max|r32-r64| %.2e tau %.2e exempt %.4f inside %.2f"
          % (case[0], E.floor32, E.tau, E.exempt, P.floor32, P.tau, P.exempt, P.inside.mean()))
    assert E.exempt <= G.EXEMPT_CAP and P.exempt <= G.EXEMPT_CAP
    assert not G.judge(E.ref64, G.round_u8(E.ref32), E.tau), "the float32 run of the extract judge misses its own bar"
    assert not C.judge_paste(P, G.round_u8(P.ref32)), "the float32 run of the paste judge misses its own bar"
    assert P.inside.any()
    from ppst_amd import imageio
    imageio.crop_transform_rule(E.xf, E.n)                      # every case is one the entry points take


@pytest.mark.parametrize("defect", C.EXTRACT_DEFECTS)
def test_every_extract_defect_violates_the_bar_somewhere(defect):
    seen = [c[0] for c in C.ALL_CASES if G.judge(C.extract_ref(c).ref64, C.extract_ref(c).defect(defect), C.extract_ref(c).tau)]
    print(defect, "seen by", seen)
    assert seen


@pytest.mark.parametrize("defect", C.PASTE_DEFECTS)
def test_every_paste_defect_violates_the_bar_somewhere(defect):
    seen = [c[0] for c in C.ALL_CASES if C.judge_paste(C.paste_ref(c), C.paste_ref(c).defect(defect))]
    print(defect, "seen by", seen)
    assert seen


def test_the_table_has_the_issues_cases_and_the_tile_edges():
    cs = C.ALL_CASES
    assert {c[3] for c in cs} == {8, 24, 40}
    assert {0.0, 90.0, 30.0, -45.0} == {c[7] for c in cs}
    assert {1.0, 1.5, 2.0, 4.0, 8.0} <= {c[6] for c in cs} and all(c[3] == 8 for c in cs if c[6] in (4.0, 8.0))
    for c in cs:
        assert 63 <= min(c[1], c[2]) and max(c[1], c[2]) <= 200 and c[8] in (0, 1, c[3] // 2)
    assert {0, 1} <= {c[8] for c in cs} and any(c[8] == c[3] // 2 for c in cs)
    # placement: fully inside, over each photo edge, covering the whole photo -- from the square's corners mapped back
    where = set()
    for c in cs:
        _, H, W, n, cx, cy, s, ang, _ = c
        th = math.radians(ang)
        cor = [(cx + s * n / 2 * (sx * math.cos(th) - sy * math.sin(th)), cy + s * n / 2 * (sx * math.sin(th) + sy * math.cos(th)))
               for sx in (-1, 1) for sy in (-1, 1)]
        xs, ys = [p[0] for p in cor], [p[1] for p in cor]
        if min(xs) >= 0 and max(xs) <= W and min(ys) >= 0 and max(ys) <= H:
            where.add("inside")
        where |= {k for k, v in (("left", min(xs) < 0), ("right", max(xs) > W), ("top", min(ys) < 0), ("bottom", max(ys) > H)) if v}
        if C.paste_ref(c).inside.all():
            where.add("whole")
    assert where == {"inside", "left", "right", "top", "bottom", "whole"}
    # one pixel either side of the paste kernel's tile edges: photo extents, and the first column / row of the square
    T = C.PASTE_T
    assert {4 * T - 1, 4 * T, 4 * T + 1} <= {c[2] for c in cs} and {5 * T - 1, 5 * T, 5 * T + 1} <= {c[1] for c in cs}
    firsts = [(int(np.argmax(C.paste_ref(c).inside.any(0))), int(np.argmax(C.paste_ref(c).inside.any(1)))) for c in C.TILE_CASES]
    assert {T - 1, T, T + 1} <= {f[0] for f in firsts} and {T - 1, T, T + 1} <= {f[1] for f in firsts}
    # both crop tiles with more than one block: n > 16 at s <= 4, n > 8 at s > 4; and s = 8 itself
    assert any(c[3] > 16 and c[6] <= 4 for c in cs) and any(c[3] > 8 and c[6] > 4 for c in cs) and any(c[6] == 8.0 for c in cs)
    # the batch: three different transforms on one photo size
    b = [C.lookup(c) for c in C.BATCH]
    assert len(b) == 3 and len({(c[1], c[2], c[3]) for c in b}) == 1 and len({C.case_xf(c) for c in b}) == 3


def test_tile_constants_are_the_sources():
    gf = open(os.path.join(ROOT, "ppst_amd", "csrc", "guided_filter.hip")).read()
    io = open(os.path.join(ROOT, "ppst_amd", "csrc", "imageio.hip")).read()
    assert int(re.search(r"#define GP_T (\d+)", gf).group(1)) == C.PASTE_T
    assert re.search(r"extract_similarity_kernel<16, EX_FS16>", io) and re.search(r"extract_similarity_kernel<8, EX_FS8>", io)
    assert C.EXTRACT_T == ((4.0, 16), (8.0, 8)) and "dmin >= ((int64_t)1 << 42)" in io          # s <= 4 <=> a^2 + b^2 >= 2^42
    # the staged boxes hold a tile's taps: (T + 3) s sqrt(2) + 3 photo pixels a side; the paste footprint 15 sqrt(2) + 3 samples
    fs16, fs8 = (int(re.search(r"#define %s (\d+)" % k, io).group(1)) for k in ("EX_FS16", "EX_FS8"))
    assert fs16 >= math.ceil(19 * 4 * math.sqrt(2) + 3) and fs8 >= math.ceil(11 * 8 * math.sqrt(2) + 3)
    assert fs16 * fs16 * 3 <= 65536 and fs8 * fs8 * 3 <= 65536
    fs = int(re.search(r"#define GP_FS (\d+)", gf).group(1))
    assert fs >= math.floor(15 * math.sqrt(2)) + 3 and fs * fs * 48 <= 65536


XF_CASES = [((8000.25, 9000.5), 512.0, 0.0, 512), ((8192.0, 8192.0), 4095.5, 30.0, 512), ((100.0, 16000.0), 700.0, -45.0, 512),
            ((12345.678, 4321.0), 1536.0, 90.0, 512), ((8192.0, 8192.0), 777.7, 171.3, 512), ((5000.0, 7000.0), 320.0, -12.5, 40),
            ((9000.0, 9000.0), 63.99, 33.0, 8)]


@pytest.mark.parametrize("centre,side,angle,n", XF_CASES, ids=["%g-%g-%g" % (c[1], c[2], c[3]) for c in XF_CASES])
def test_crop_transform_round_trips_centre_side_and_angle(centre, side, angle, n):
    """the integers against the float64 map they round: centre, side and angle recovered, and no point within 8192 photo pixels
    of the centre (a 16384-pixel photo around it) moves by more than 2^-10 crop pixel: a and b are rounded at 2^-24 crop pixel
    per HALF photo pixel (2 x 8192 x 0.5 x 2^-24 = 2^-11 each), the offsets are exact at the centre up to their own 2^-25"""
    from ppst_amd import imageio
    xf = imageio.crop_transform(centre, side, angle, n)
    assert xf == C.crop_xf(centre, side, angle, n) and all(isinstance(v, int) for v in xf)
    imageio.crop_transform_rule(xf, n)
    a, b, cu, cv = xf
    s = side / n
    assert abs((1 << 23) / math.hypot(a, b) * n - side) <= side * 2.0 ** -20
    assert abs((math.degrees(math.atan2(b, a)) - angle + 180) % 360 - 180) <= 1e-4
    D = a * a + b * b                                          # the photo position of the crop's centre
    px, py = (a * (n * C.HALF - cu) - b * (n * C.HALF - cv)) / D, (b * (n * C.HALF - cu) + a * (n * C.HALF - cv)) / D
    assert abs(px / 2 - centre[0]) <= 2.0 ** -20 and abs(py / 2 - centre[1]) <= 2.0 ** -20
    th = math.radians(angle)
    worst = 0.0
    for X in (math.floor(centre[0]) - 8192, math.floor(centre[0]), math.floor(centre[0]) + 8191):
        for Y in (math.floor(centre[1]) - 8192, math.floor(centre[1]), math.floor(centre[1]) + 8191):
            U, V = C.uv(xf, np.int64(X), np.int64(Y))
            dx, dy = X + 0.5 - centre[0], Y + 0.5 - centre[1]
            u = (math.cos(th) * dx + math.sin(th) * dy) / s + n / 2
            v = (-math.sin(th) * dx + math.cos(th) * dy) / s + n / 2
            worst = max(worst, abs(int(U) / C.ONE - u), abs(int(V) / C.ONE - v))
    print("worst |integer map - float64 map| %.3e crop pixel (2^-10 = %.3e)" % (worst, 2.0 ** -10))
    assert worst <= 2.0 ** -10


def test_crop_transform_rule_refuses_out_of_range_scales():
    from ppst_amd import imageio
    for side, angle in ((512.0, 0.0), (4096.0, 90.0), (1000.0, 17.0), (512.001, 17.0), (4095.99, 17.0)):
        imageio.crop_transform_rule(imageio.crop_transform((900.0, 700.0), side, angle, 512), 512)
    imageio.crop_transform_rule([imageio.crop_transform((9.0, 7.0), 512.0, 0.0, 512), imageio.crop_transform((9.0, 7.0), 4096.0, 90.0, 512)], 512)
    with pytest.raises(ValueError, match="s = 0.99.* < 1"):
        imageio.crop_transform_rule(imageio.crop_transform((900.0, 700.0), 511.0, 17.0, 512), 512)
    with pytest.raises(ValueError, match="> 8"):
        imageio.crop_transform_rule(imageio.crop_transform((900.0, 700.0), 4100.0, -30.0, 512), 512)
    with pytest.raises(ValueError, match="> 8"):
        imageio.crop_transform_rule([(1 << 23, 0, 0, 0), (1 << 19, 0, 0, 0)], 512)          # the second of a batch
    with pytest.raises(ValueError, match="inf"):
        imageio.crop_transform_rule((0, 0, 0, 0), 512)
    with pytest.raises(ValueError, match="2\\^56"):
        imageio.crop_transform_rule((1 << 23, 0, 1 << 57, 0), 512)
    with pytest.raises(ValueError, match="4096"):
        imageio.crop_transform_rule((1 << 23, 0, 0, 0), 5000)
    with pytest.raises(ValueError, match="positive"):
        imageio.crop_transform((1.0, 1.0), 0.0)
    # the ends themselves: s = 1 and s = 8 are accepted
    imageio.crop_transform_rule([(1 << 23, 0, 0, 0), (1 << 20, 0, 0, 0), (0, -(1 << 23), 0, 0)], 8)


def test_entry_points_reject_bad_arguments_before_any_launch():
    import __graft_entry__ as g
    g.build()
    from ppst_amd._lib import lib
    d = ctypes.c_void_p(16)            # a non-null token: validation happens before anything on the device is touched
    table = lambda *rows: (ctypes.c_int64 * (4 * len(rows)))(*[v for r in rows for v in r])
    ok = table((1 << 23, 0, 0, 0))

    def extract(photo=d, B=1, H=90, W=70, xh=ok, xd=d, n=24, out=d):
        return lib.ppst_extract_similarity(photo, B, H, W, xh, xd, n, out, None)

    def paste(co=d, n=24, photo=d, out=d, B=1, H=90, W=70, xh=ok, xd=d, feather=1):
        return lib.ppst_guided_filter_paste(co, n, photo, out, B, H, W, xh, xd, feather, None)

    for null in ("photo", "xh", "xd", "out"):
        assert extract(**{null: None}) == -3 and paste(**{null: None}) == -3, null
    assert paste(co=None) == -3
    for bad in (dict(B=-1), dict(H=0), dict(W=0), dict(n=0), dict(n=4097), dict(H=1 << 14, W=(1 << 14) + 1)):
        assert extract(**bad) == -1 and paste(**bad) == -1, bad
    for bad in (dict(feather=-1), dict(feather=13)):
        assert paste(**bad) == -1, bad
    assert paste(feather=12, xh=table((1 << 19, 0, 0, 0))) == -1
    for rows in (((1 << 23) + 1, 0, 0, 0), (1 << 19, 0, 0, 0), (0, 0, 0, 0), (1 << 23, 0, (1 << 56) + 1, 0), (1 << 23, 0, 0, -(1 << 56) - 1),
                 (1 << 24, 0, 0, 0), (-(1 << 40), 5, 0, 0)):
        assert extract(xh=table(rows)) == -1 and paste(xh=table(rows)) == -1, rows
    assert extract(B=2, xh=table((1 << 23, 0, 0, 0), (1 << 19, 0, 0, 0))) == -1           # every row is checked
    assert extract(B=0, photo=None, xh=None, xd=None, out=None) == 0 and paste(B=0, co=None, photo=None, out=None, xh=None, xd=None) == 0
    assert extract(B=0, n=0) == -1 and paste(B=0, feather=13) == -1
    # a square that does not meet its photo: nothing to launch
    assert paste(xh=table((1 << 23, 0, 1 << 40, 0))) == 0


def test_ops_refuse_cpu_tensors_and_wrong_dtypes():
    from ppst_amd import ops

    class FakeCuda(torch.Tensor):
        is_cuda = True
    fake = lambda t: t.as_subclass(FakeCuda)
    photo = torch.zeros((1, 90, 70, 3), dtype=torch.uint8)
    co = torch.zeros((1, 12, 24, 24))
    xf = [(1 << 23, 0, 0, 0)]
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.extract_similarity(photo, xf, 24)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.guided_filter_paste(co, photo, xf)
    with pytest.raises(RuntimeError, match="CUDA uint8 photo"):
        ops.guided_filter_paste(fake(co), photo, xf)
    with pytest.raises(RuntimeError, match="CUDA float32"):
        ops.guided_filter_paste(co, fake(photo), xf)
    with pytest.raises(RuntimeError, match="uint8"):
        ops.extract_similarity(fake(photo.float()), xf, 24)
    with pytest.raises(RuntimeError, match="float32"):
        ops.guided_filter_paste(fake(co.half()), fake(photo), xf)
    with pytest.raises(RuntimeError, match="uint8"):
        ops.guided_filter_paste(fake(co), fake(photo.float()), xf)
    with pytest.raises(RuntimeError, match="B,H,W,3"):
        ops.extract_similarity(fake(photo[0]), xf, 24)
    for bc, bp in ((co[:, :11], photo), (co[..., :23], photo), (co, photo[..., :2]), (co, torch.zeros((2, 90, 70, 3), dtype=torch.uint8))):
        with pytest.raises(RuntimeError, match="B,12,n,n"):
            ops.guided_filter_paste(fake(bc), fake(bp), xf)
    with pytest.raises(RuntimeError, match="int64"):
        ops._crop_transforms(torch.zeros((1, 4), dtype=torch.int32), 1, "cpu", "t")
    with pytest.raises(RuntimeError, match="per image"):
        ops._crop_transforms([(1, 2, 3, 4), (1, 2, 3, 4)], 3, "cpu", "t")
    host, _ = ops._crop_transforms((1 << 23, 0, -(1 << 50), 7), 3, "cpu", "t")
    assert host.dtype == torch.int64 and host.tolist() == [[1 << 23, 0, -(1 << 50), 7]] * 3 and host.is_contiguous()


def test_region_front_ends_refuse_from_shapes_and_integers_alone():
    from ppst_amd import evaluation as EV, imageio
    from ppst_amd.ppst_model import PPSTModel
    style = torch.zeros((1, 3, 512, 512))
    photo = torch.zeros((1, 3000, 4000, 3), dtype=torch.uint8)
    good = imageio.crop_transform((2000.0, 1500.0), 1024.0, 10.0)
    with pytest.raises(ValueError, match="B,H,W,3"):
        EV.simple_swap_region(None, photo[0], good, style)
    with pytest.raises(ValueError, match="multiple of 512"):
        EV.simple_swap_region(None, photo, good, style, load_size=600)
    with pytest.raises(ValueError, match="< 1"):
        EV.simple_swap_region(None, photo, imageio.crop_transform((2000.0, 1500.0), 300.0, 10.0), style)
    with pytest.raises(ValueError, match="> 8"):
        EV.simple_swap_region(None, photo, imageio.crop_transform((2000.0, 1500.0), 4200.0, 10.0), style)
    with pytest.raises(ValueError, match="> 8"):
        EV.evaluate_swap_files_region(None, "no-such-file.png", "no-such-file.png", "unused", (2000.0, 1500.0, 4200.0, 0.0))
    m = PPSTModel()
    m.opt.gf_radius = 65
    with pytest.raises(ValueError, match="r <= 64"):       # before the generator: the codes are None
        m(None, None, torch.empty((1, 3, 512, 512)), None, good, 16, command="decode_region")
    assert list(inspect.signature(EV.simple_swap_region).parameters) == ["model", "photo_u8", "xf", "style", "alphas", "load_size", "feather",
                                                                         "style_xf"]
    sig = inspect.signature(EV.simple_swap_region).parameters
    assert (sig["alphas"].default, sig["load_size"].default, sig["feather"].default, sig["style_xf"].default) == ((1.0,), 512, 16, None)
    assert list(inspect.signature(EV.evaluate_swap_files_region).parameters)[:6] == ["model", "structure_path", "texture_path", "out_dir",
                                                                                    "structure_box", "texture_box"]
    assert list(inspect.signature(m.decode_region).parameters) == ["spatial_code", "global_code", "target", "photo_u8", "xf", "feather"]
