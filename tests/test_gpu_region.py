"""GPU: a swap inside a photograph -- the aligned crop under a similarity transform (csrc/imageio.hip extract_similarity_kernel;
ops.extract_similarity) and the guided filter's coefficients pasted back through it (csrc/guided_filter.hip gf_paste_kernel;
ops.guided_filter_paste; PPSTModel.decode_region; evaluation.simple_swap_region / evaluate_swap_files_region) against the float64
restatements on the CPU (tests/region_cases.py) -- pytest -m gpu.  The device is never its own judge.

Bar (gf_cases.judge): the device's bytes equal rint(ref64) wherever ref64 lies farther than tau from a rounding boundary, may be
either neighbour within tau, and everywhere |device - rint(ref64)| <= 1; tau = 2 max|ref32 - ref64| + 1e-3 from the restatement
alone; bytes outside the crop square EQUAL the photo's.  Every test prints tau and the tau the device would have needed.
tests/test_region_cases_cpu.py shows that the cases see every seeded defect through this bar.  The paste is judged on
coefficient planes computed on the CPU (gf_native_cases.mean_planes, rounded to fp32), so each stage stands alone.
Not covered: photos past 2^31 bytes (H W <= 2^28 is the entry points' limit: 805 MB); every byte offset is int64.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gf_cases as G  # noqa: E402
import region_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", 0)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _extract(photos, xfs, n):
    from ppst_amd import ops
    out = ops.extract_similarity(_t(np.stack(photos)), list(xfs), n)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _paste(planes, photos, xfs, feather, **kw):
    from ppst_amd import ops
    out = ops.guided_filter_paste(_t(np.stack(planes)), _t(np.stack(photos)), list(xfs), feather, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("case", C.ALL_CASES, ids=C.case_id)
def test_extract_against_float64(case):
    R = C.extract_ref(case)
    got = _extract([R.photo], [R.xf], R.n)[0]
    d = np.abs(got.astype(int) - R.expect.astype(int))
    print("%-24s tau %.5f (max|r32-r64| %.2e)  device needs %.5f  max |diff| %d  differing %.5f  exempt %.4f"
          % (case[0], R.tau, R.floor32, G.min_tau(R.ref64, got), d.max(), (d > 0).mean(), R.exempt))
    bad = G.judge(R.ref64, got, R.tau)
    assert not bad, "%s: %s" % (case[0], "; ".join(bad))


@pytest.mark.parametrize("case", C.ALL_CASES, ids=C.case_id)
def test_paste_against_float64(case):
    R = C.paste_ref(case)
    got = _paste([R.planes], [R.photo], [R.xf], R.feather)[0]
    d = np.abs(got.astype(int) - R.expect.astype(int))
    print("%-24s tau %.5f (max|r32-r64| %.2e)  device needs %.5f  max |diff| %d  differing %.5f  exempt %.4f  inside %.2f"
          % (case[0], R.tau, R.floor32, G.min_tau(R.ref64, got), d.max(), (d > 0).mean(), R.exempt, R.inside.mean()))
    bad = C.judge_paste(R, got)
    assert not bad, "%s: %s" % (case[0], "; ".join(bad))


def test_extract_at_an_integer_offset_is_the_slice():
    """angle 0, s = 1, integer offset: every weight is 0 or 1 -- a byte copy, also where the square hangs over the photo's edge
    (edge replication)"""
    from ppst_amd import imageio
    photo = C.photo_of(90, 70)
    got = _extract([photo], [imageio.crop_transform((35.0, 45.0), 24, 0.0, 24)], 24)[0]
    assert np.array_equal(got, photo[33:57, 23:47])
    over = _extract([photo], [imageio.crop_transform((3.0, 85.0), 40, 0.0, 40)], 40)[0]
    yy, xx = np.clip(np.arange(65, 105), 0, 89), np.clip(np.arange(-17, 23), 0, 69)
    assert np.array_equal(over, photo[yy][:, xx])


def _batch():
    cs = [C.lookup(c) for c in C.BATCH]
    Es = [C.ExtractRef(c) for c in cs]
    return cs, Es


def test_batch_in_place_and_views():
    """three different transforms in one call: every image bit-equal to its single call; the paste in place and into a given
    tensor equal the cloned form; non-contiguous and misaligned views (a photo sliced from a padded buffer, one image of a batch
    at an odd byte offset) give the bytes of their copies; one transform serves a whole batch"""
    from ppst_amd import ops
    cs, Es = _batch()
    n, xfs, photo = Es[0].n, [e.xf for e in Es], Es[0].photo
    photos = [np.ascontiguousarray(np.roll(photo, 7 * i, axis=1)) for i in range(3)]
    crops = _extract(photos, xfs, n)
    src = G.blocks(n, n, seed=5)[1]
    planes = [C.N.mean_planes(np.ascontiguousarray(crops[i]), src, C.R, C.N.EPS, np.float64).astype(np.float32) for i in range(3)]
    feather = 3
    out = _paste(planes, photos, xfs, feather)
    for i in range(3):
        assert np.array_equal(_extract([photos[i]], [xfs[i]], n)[0], crops[i]), "extract, image %d" % i
        assert np.array_equal(_paste([planes[i]], [photos[i]], [xfs[i]], feather)[0], out[i]), "paste, image %d" % i
        want = C.paste(planes[i], photos[i], xfs[i], feather, np.float64)
        assert np.abs(out[i].astype(int) - G.round_u8(want).astype(int)).max() <= 1
    assert not np.array_equal(out[0], out[1])
    dev = _dev()
    P, CO = _t(np.stack(photos)), _t(np.stack(planes))
    same = ops.guided_filter_paste(CO, P, xfs, feather, out=P.clone())
    assert np.array_equal(same.cpu().numpy(), out)
    given = torch.full_like(P, 201)
    assert ops.guided_filter_paste(CO, P, xfs, feather, out=given) is given and np.array_equal(given.cpu().numpy(), out)
    inplace = P.clone()
    assert ops.guided_filter_paste(CO, inplace, xfs, feather, out=inplace) is inplace and np.array_equal(inplace.cpu().numpy(), out)
    assert np.array_equal(P.cpu().numpy(), np.stack(photos)), "the cloned form wrote into its photo"
    # a tensor of transforms (host or device) is the nested list; one row serves the batch
    xt = torch.tensor(xfs, dtype=torch.int64)
    assert np.array_equal(ops.extract_similarity(P, xt.to(dev), n).cpu().numpy(), crops)
    assert np.array_equal(ops.guided_filter_paste(CO, P, xt, feather).cpu().numpy(), out)
    one = ops.extract_similarity(P, xfs[1], n).cpu().numpy()
    for i in range(3):
        assert np.array_equal(one[i], _extract([photos[i]], [xfs[1]], n)[0])
    # views: one image of the batch, batch stride 2, a photo sliced from a padded RGBA buffer, a photo at an odd byte address,
    # coefficient planes sliced from a padded tensor
    assert np.array_equal(ops.extract_similarity(P[1:2], xfs[1:2], n).cpu().numpy(), crops[1:2])
    assert np.array_equal(ops.guided_filter_paste(CO[0::2], P[0::2], xfs[0::2], feather).cpu().numpy(), out[0::2])
    H, W = photo.shape[:2]
    big = torch.zeros((3, H + 9, W + 7, 4), dtype=torch.uint8, device=dev)
    big[:, 5:5 + H, 3:3 + W, :3] = P
    view = big[:, 5:5 + H, 3:3 + W, :3]
    assert not view.is_contiguous()
    assert np.array_equal(ops.extract_similarity(view, xfs, n).cpu().numpy(), crops)
    assert np.array_equal(ops.guided_filter_paste(CO, view, xfs, feather).cpu().numpy(), out)
    odd = torch.zeros((3 * H * W * 3 + 1,), dtype=torch.uint8, device=dev)
    mis = odd[1:].view(3, H, W, 3)
    mis.copy_(P)
    assert mis.data_ptr() % 4 == 1
    assert np.array_equal(ops.extract_similarity(mis, xfs, n).cpu().numpy(), crops)
    assert np.array_equal(ops.guided_filter_paste(CO, mis, xfs, feather, out=mis).cpu().numpy(), out)
    pad = torch.zeros((3, 12, n + 5, n + 9), device=dev)
    pad[:, :, 2:2 + n, 4:4 + n] = CO
    assert np.array_equal(ops.guided_filter_paste(pad[:, :, 2:2 + n, 4:4 + n], P, xfs, feather).cpu().numpy(), out)


def test_refusals_raise_and_write_nothing_and_empty_batches():
    from ppst_amd import imageio, ops
    dev = _dev()
    photo = torch.full((1, 90, 70, 3), 90, dtype=torch.uint8, device=dev)
    co = torch.zeros((1, 12, 24, 24), device=dev)
    good = imageio.crop_transform((35.0, 45.0), 36.0, 30.0, 24)
    for bad in (imageio.crop_transform((35.0, 45.0), 23.0, 30.0, 24), imageio.crop_transform((35.0, 45.0), 200.0, 30.0, 24)):
        with pytest.raises(RuntimeError, match="ppst_extract_similarity"):
            ops.extract_similarity(photo, bad, 24)
        keep = photo.clone()
        with pytest.raises(RuntimeError, match="ppst_guided_filter_paste"):
            ops.guided_filter_paste(co, keep, bad, 0, out=keep)
        assert torch.equal(keep, photo)
    with pytest.raises(RuntimeError, match="ppst_guided_filter_paste"):
        ops.guided_filter_paste(co, photo, good, 13)
    with pytest.raises(RuntimeError, match="ppst_guided_filter_paste"):
        ops.guided_filter_paste(co, photo, good, -1)
    with pytest.raises(RuntimeError, match="per image"):
        ops.extract_similarity(photo, [good, good], 24)
    with pytest.raises(RuntimeError, match="contiguous uint8"):
        ops.guided_filter_paste(co, photo, good, 0, out=torch.zeros((1, 90, 71, 3), dtype=torch.uint8, device=dev))
    # a square that does not meet its photo: every byte is the photo's
    far = imageio.crop_transform((5000.0, 45.0), 36.0, 30.0, 24)
    assert torch.equal(ops.guided_filter_paste(co, photo, far, 2), photo)
    e = ops.extract_similarity(photo[:0], torch.zeros((0, 4), dtype=torch.int64), 24)
    assert tuple(e.shape) == (0, 24, 24, 3) and e.dtype == torch.uint8
    p = ops.guided_filter_paste(co[:0], photo[:0], torch.zeros((0, 4), dtype=torch.int64), 0)
    assert tuple(p.shape) == (0, 90, 70, 3) and p.dtype == torch.uint8


# ------------------------------------------------------------------------------------------------------------- model level
def _model():
    from ppst_amd import weights as W
    from ppst_amd.ppst_model import create_model
    sd = W.make_state_dict(3, with_D=False, with_nce=False, bias_std=0.1, noise_weight=0.0)
    return create_model(state_dict=sd, device=_dev())


def _photos(seed, n, H, W):
    """n seeded pictures as (n,H,W,3) uint8 on the host: synthetic 512^2 images resized by Pillow"""
    from PIL import Image
    from ppst_amd import weights as Wt
    base = Wt.synthetic_images(seed, n, size=512)
    u8 = ((base.clamp(-1, 1) + 1) * 127.5).to(torch.uint8).permute(0, 2, 3, 1).numpy()
    return np.stack([np.array(Image.fromarray(a).resize((W, H), Image.BICUBIC)) for a in u8])


@pytest.fixture(scope="module")
def model():
    return _model()


def test_simple_swap_region_is_its_steps_by_hand(model):
    """simple_swap_region at load_size 512 against extract -> swap_codes -> generator -> guided_filter_coeffs -> guided_filter_paste
    run by hand, bit for bit; every byte outside the quad is the photo's; a style photo with its own box is extracted the same
    way; the bad-radius ValueError comes before any model pass"""
    from ppst_amd import evaluation as EV, glue, imageio, ops
    dev = _dev()
    arr = _photos(47, 2, 700, 900)
    photo, style_photo = torch.from_numpy(arr[0:1]).to(dev), torch.from_numpy(arr[1:2]).to(dev)
    xf = imageio.crop_transform((470.0, 340.0), 600.0, 20.0, 512)
    sxf = imageio.crop_transform((400.0, 350.0), 640.0, -10.0, 512)
    alphas, feather = (0.5, 1.0), 16
    with torch.no_grad():
        got = EV.simple_swap_region(model, photo, xf, style_photo, alphas, 512, feather, style_xf=sxf)
        crop = ops.extract_similarity(photo, xf, 512)
        content = imageio.to_tensor_normalized(crop)
        style = imageio.to_tensor_normalized(ops.extract_similarity(style_photo, sxf, 512))
        assert tuple(content.shape) == (1, 3, 512, 512)
        sp, gl_c, gl_w = EV.swap_codes(model, content, style)
        for alpha in alphas:
            g_out = model(sp, glue.lerp(gl_c, gl_w, alpha), target=None, command="decode")
            coeffs = ops.guided_filter_coeffs(glue.tensor2im(content), glue.tensor2im(g_out), 30, (0.02 * 255) ** 2)
            hand = ops.guided_filter_paste(coeffs, photo, xf, feather)
            assert hand.dtype == torch.uint8 and tuple(hand.shape) == (1, 700, 900, 3)
            assert torch.equal(hand, got[alpha]), "alpha %g: simple_swap_region differs from its steps by hand" % alpha
        assert not torch.equal(got[0.5], got[1.0])
        # a style tensor in place of a style photo
        again = EV.simple_swap_region(model, photo, xf, style, (1.0,), 512, feather)
        assert torch.equal(again[1.0], got[1.0])
        inside = C.inside(xf, 512, 700, 900)[0]
        out = got[1.0][0].cpu().numpy()
        assert np.array_equal(out[~inside], arr[0][~inside]) and 0.3 < inside.mean() < 0.7
        assert (out[inside] != arr[0][inside]).mean() > 0.5, "the swap left the quad as it was"
        # the crop is judged too: the device's 512^2 crop against the float64 restatement at this size
        ref64 = C.extract(arr[0], xf, 512, np.float64)
        tau = 2 * float(np.abs(C.extract(arr[0], xf, 512, np.float32).astype(np.float64) - ref64).max()) + 1e-3
        assert not G.judge(ref64, crop[0].cpu().numpy(), tau)
        calls = []
        forward, radius = model.G.forward, model.opt.gf_radius
        model.G.forward = lambda *a, **k: calls.append(1) or forward(*a, **k)
        model.opt.gf_radius = 65
        try:
            with pytest.raises(ValueError, match="r <= 64"):
                model(sp, gl_c, content, photo, xf, feather, command="decode_region")
            assert not calls
            model.opt.gf_radius = radius
            model(sp, gl_c, content, photo, xf, feather, command="decode_region")
            assert calls                                       # (the probe does see a generator pass)
        finally:
            model.opt.gf_radius = radius
            del model.G.forward


def test_evaluate_swap_files_region_writes_what_the_recipe_returns(model, tmp_path):
    """a 600 x 800 PNG structure file with a box; a square texture file taken whole, and a 600 x 800 one with a box of its own: the
    written files decode to simple_swap_region's tensors, at the structure file's size"""
    from PIL import Image
    from ppst_amd import evaluation as EV, imageio
    dev = _dev()
    arr = _photos(49, 2, 600, 800)
    sq = _photos(51, 1, 640, 640)
    cp, tp, qp = str(tmp_path / "c0.png"), str(tmp_path / "t1.png"), str(tmp_path / "q2.png")
    Image.fromarray(arr[0]).save(cp)
    Image.fromarray(arr[1]).save(tp)
    Image.fromarray(sq[0]).save(qp)
    box, tbox = (400.0, 300.0, 560.0, 15.0), (390.0, 310.0, 580.0, 0.0)
    xf, txf = imageio.crop_transform(box[:2], box[2], box[3]), imageio.crop_transform(tbox[:2], tbox[2], tbox[3])
    photo = torch.from_numpy(arr[0:1]).to(dev)
    with torch.no_grad():
        whole = EV.load_images([qp], 512, dev)[0]
        want_a = EV.simple_swap_region(model, photo, xf, whole, (1.0,), 512, 16)
        want_b = EV.simple_swap_region(model, photo, xf, torch.from_numpy(arr[1:2]).to(dev), (1.0,), 512, 8, style_xf=txf)
        pa = EV.evaluate_swap_files_region(model, cp, qp, str(tmp_path / "a"), box)
        pb = EV.evaluate_swap_files_region(model, [cp], [tp], str(tmp_path / "b"), [box], [tbox], feather=8, png="device")
    assert [os.path.basename(p) for p in pa] == ["c0_q2_1.00.png"] and [os.path.basename(p) for p in pb] == ["c0_t1_1.00.png"]
    assert np.array_equal(np.asarray(Image.open(pa[0])), want_a[1.0][0].cpu().numpy())
    assert np.array_equal(np.asarray(Image.open(pb[0])), want_b[1.0][0].cpu().numpy())
    assert np.asarray(Image.open(pa[0])).shape == (600, 800, 3)
