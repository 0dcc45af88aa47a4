"""GPU: a label map turned into a matte (csrc/matte.hip; ops.label_matte) and the guided filter's coefficients pasted into a
photograph through it (csrc/guided_filter.hip gf_paste_kernel<true>; ops.guided_filter_paste(matte=); PPSTModel.decode_region_matte;
evaluation.simple_swap_region_matte / evaluate_swap_files_region(label_path=)) against the restatements on the CPU
(tests/matte_cases.py) -- pytest -m gpu.  The device is never its own judge.

Bars: sd2 bit-equal to the restatement; matte |device - m64| <= 2 max|m32 - m64| + 1e-6; paste gf_cases.judge(ref64, device, tau),
tau = 2 max|ref32 - ref64| + 1e-3, on the fp32 restatement's matte plane (each stage stands alone), and bytes outside the square
or under a zero weight EQUAL the photo's.  Every test prints the tolerance the device needed.  tests/test_matte_cases_cpu.py shows
that the cases see every seeded defect through these bars.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gf_cases as G  # noqa: E402
import matte_cases as M  # noqa: E402
import region_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", 0)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _keep(mask):
    return tuple(k for k in range(32) if (mask >> k) & 1)


def _matte(labels, keep, feather, grow):
    from ppst_amd import ops
    m, sd2 = ops.label_matte(_t(labels), _keep(keep), feather, grow, want_distance=True)
    torch.cuda.synchronize()
    return m.cpu().numpy(), sd2.cpu().numpy()


def _paste(planes, mattes, photos, xfs, feather, **kw):
    from ppst_amd import ops
    out = ops.guided_filter_paste(_t(np.stack(planes)), _t(np.stack(photos)), list(xfs), feather,
                                  matte=None if mattes is None else _t(np.stack(mattes)), **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("shape", M.SHAPES + [M.BIG], ids=lambda s: "%dx%d" % s)
def test_distance_and_matte_against_the_restatement(shape):
    need, bad = 0.0, []
    for c in M.cases_of(shape):
        R = M.matte_ref(c)
        m, sd2 = _matte(R.labels[None], R.keep, R.feather, R.grow)
        assert sd2.dtype == np.int32 and m.dtype == np.float32 and sd2.shape == m.shape == (1,) + tuple(shape)
        err = float(np.abs(m[0].astype(np.float64) - R.m64).max())
        need = max(need, err)
        print("%-32s sd2 differing %d  matte: tol %.3e (max|m32-m64| %.2e)  device needs %.3e"
              % (c[0], int((sd2[0] != R.sd2).sum()), R.tol, R.floor32, err))
        if not np.array_equal(sd2[0], R.sd2):
            bad.append("%s: sd2 differs at %d pixels" % (c[0], int((sd2[0] != R.sd2).sum())))
        if err > R.tol:
            bad.append("%s: matte off by %.3e > %.3e" % (c[0], err, R.tol))
    print("%dx%d: the device's matte needed %.3e" % (shape + (need,)))
    assert not bad, "; ".join(bad)


def test_matte_batch_views_and_distance_only():
    """a batch of different planes equals the single calls; non-contiguous labels equal contiguous ones; the matte without the
    distance is the matte with it; an empty batch"""
    from ppst_amd import ops
    cs = [c for c in M.cases_of((40, 40)) if c[3] in ("blob", "checker", "values", "diagonal")]
    labs = np.stack([M.PATTERNS[c[3]](40, 40)[0] for c in cs])
    keep = M.keep_mask((0, 2, 31))
    m, sd2 = _matte(labs, keep, 6, 3)
    for i in range(len(cs)):
        mi, si = _matte(labs[i:i + 1], keep, 6, 3)
        assert np.array_equal(mi[0], m[i]) and np.array_equal(si[0], sd2[i]), i
        assert np.array_equal(sd2[i], M.sd2_separable(labs[i], keep, 6, 3)), i
    big = torch.zeros((len(cs), 47, 90), dtype=torch.uint8, device=_dev())
    big[:, 3:43, 5:85:2] = _t(labs)
    view = big[:, 3:43, 5:85:2]
    assert not view.is_contiguous()
    mv, sv = ops.label_matte(view, _keep(keep), 6, 3, want_distance=True)
    assert np.array_equal(mv.cpu().numpy(), m) and np.array_equal(sv.cpu().numpy(), sd2)
    only = ops.label_matte(_t(labs), _keep(keep), 6, 3)
    assert isinstance(only, torch.Tensor) and np.array_equal(only.cpu().numpy(), m)
    e = ops.label_matte(_t(labs)[:0], (1, 2))
    assert tuple(e.shape) == (0, 40, 40) and e.dtype == torch.float32
    with pytest.raises(RuntimeError, match="ppst_label_matte"):
        ops.label_matte(_t(labs), (1, 2), 256, 0)


@pytest.mark.parametrize("case", C.ALL_CASES, ids=C.case_id)
def test_paste_through_a_matte_against_float64(case):
    R = M.paste_ref(case)
    got = _paste([R.planes], [R.M], [R.photo], [R.xf], R.feather)[0]
    d = np.abs(got.astype(int) - R.expect.astype(int))
    print("%-24s matte (f %d, g %d) tau %.5f (max|r32-r64| %.2e)  device needs %.5f  max |diff| %d  differing %.5f  exempt %.4f"
          % (case[0], R.mf, R.mg, R.tau, R.floor32, G.min_tau(R.ref64, got), d.max(), (d > 0).mean(), R.exempt))
    bad = M.judge_paste(R, got)
    assert not bad, "%s: %s" % (case[0], "; ".join(bad))


@pytest.mark.parametrize("case", C.ALL_CASES, ids=C.case_id)
def test_all_ones_matte_is_the_plain_paste_and_poison_cannot_leak(case):
    R = M.paste_ref(case)
    plain = _paste([R.planes], None, [R.photo], [R.xf], R.feather)[0]
    ones = _paste([R.planes], [np.ones_like(R.M)], [R.photo], [R.xf], R.feather)[0]
    assert np.array_equal(ones, plain), "an all-ones matte differs from the paste without one"
    zeros = _paste([R.planes], [np.zeros_like(R.M)], [R.photo], [R.xf], R.feather)[0]
    assert np.array_equal(zeros, R.photo), "an all-zero matte wrote"
    clean = _paste([R.planes], [R.M], [R.photo], [R.xf], R.feather)[0]
    bad = M.poison(R.planes, R.M)
    got = _paste([bad], [R.M], [R.photo], [R.xf], R.feather)[0]
    print("%-24s poisoned share of the planes %.2f" % (case[0], float(np.isnan(bad[0]).mean())))
    assert np.array_equal(got, clean), "non-finite coefficients under a zero matte leaked"


def test_paste_matte_batch_in_place_and_given():
    """three transforms in one call: every image bit-equal to its single call; in place equals cloned equals into a given tensor;
    a non-contiguous matte equals its copy; refusals"""
    from ppst_amd import ops
    cs = [C.lookup(c) for c in C.BATCH]
    Ps = [C.PasteRef(c) for c in cs]
    n, xfs, feather = Ps[0].n, [p.xf for p in Ps], 3
    photos = [np.ascontiguousarray(np.roll(Ps[0].photo, 7 * i, axis=1)) for i in range(3)]
    planes = [p.planes for p in Ps]
    mattes = [M.matte(M.sd2_separable(M._blob(n, n, 10 + i), M.FACE, f, g), f, g, np.float32) for i, (f, g) in enumerate(((6, 3), (1, 0), (0, 2)))]
    out = _paste(planes, mattes, photos, xfs, feather)
    for i in range(3):
        assert np.array_equal(_paste([planes[i]], [mattes[i]], [photos[i]], [xfs[i]], feather)[0], out[i]), "image %d" % i
        want = M.paste_matte(planes[i], mattes[i], photos[i], xfs[i], feather, np.float64)
        assert np.abs(out[i].astype(int) - G.round_u8(want).astype(int)).max() <= 1
    assert not np.array_equal(out[0], out[1])
    P, CO, MT = _t(np.stack(photos)), _t(np.stack(planes)), _t(np.stack(mattes))
    given = torch.full_like(P, 201)
    assert ops.guided_filter_paste(CO, P, xfs, feather, out=given, matte=MT) is given and np.array_equal(given.cpu().numpy(), out)
    inplace = P.clone()
    assert ops.guided_filter_paste(CO, inplace, xfs, feather, out=inplace, matte=MT) is inplace and np.array_equal(inplace.cpu().numpy(), out)
    assert np.array_equal(P.cpu().numpy(), np.stack(photos)), "the cloned form wrote into its photo"
    pad = torch.zeros((3, n + 5, n + 9), device=_dev())
    pad[:, 2:2 + n, 4:4 + n] = MT
    assert np.array_equal(ops.guided_filter_paste(CO, P, xfs, feather, matte=pad[:, 2:2 + n, 4:4 + n]).cpu().numpy(), out)
    with pytest.raises(RuntimeError, match="float32 matte"):
        ops.guided_filter_paste(CO, P, xfs, feather, matte=MT[:, :-1])
    with pytest.raises(RuntimeError, match="float32 matte"):
        ops.guided_filter_paste(CO, P, xfs, feather, matte=MT.cpu())
    keep = P.clone()
    with pytest.raises(RuntimeError, match="ppst_guided_filter_paste_matte"):
        ops.guided_filter_paste(CO, keep, xfs, n, out=keep, matte=MT)
    assert torch.equal(keep, P)
    p = ops.guided_filter_paste(CO[:0], P[:0], torch.zeros((0, 4), dtype=torch.int64), 0, matte=MT[:0])
    assert tuple(p.shape) == (0,) + tuple(P.shape[1:])


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


def test_simple_swap_region_matte_is_its_steps_by_hand(model):
    """simple_swap_region_matte(labels=) at load_size 512 inside a 700 x 900 photo against extract -> swap_codes -> generator ->
    guided_filter_coeffs -> label_matte -> guided_filter_paste(matte=) by hand, bit for bit; int64 and one-hot labels and a ready
    matte give the same bytes; with every label kept and matte_feather = matte_grow = 0 it is simple_swap_region, bit for bit;
    photo pixels whose matte taps are all 0 keep their bytes"""
    from ppst_amd import evaluation as EV, glue, imageio, ops
    dev = _dev()
    arr = _photos(47, 2, 700, 900)
    photo, style_photo = torch.from_numpy(arr[0:1]).to(dev), torch.from_numpy(arr[1:2]).to(dev)
    xf = imageio.crop_transform((470.0, 340.0), 600.0, 20.0, 512)
    sxf = imageio.crop_transform((400.0, 350.0), 640.0, -10.0, 512)
    feather, mf, mg = 16, 24, 12
    lab = M._blob(512, 512, 5)
    labels = torch.from_numpy(lab[None]).to(dev)
    with torch.no_grad():
        got = EV.simple_swap_region_matte(model, photo, xf, style_photo, (1.0,), 512, feather, style_xf=sxf, labels=labels, keep=(1, 2),
                                          matte_feather=mf, matte_grow=mg)[1.0]
        content = imageio.to_tensor_normalized(ops.extract_similarity(photo, xf, 512))
        style = imageio.to_tensor_normalized(ops.extract_similarity(style_photo, sxf, 512))
        sp, gl_c, gl_w = EV.swap_codes(model, content, style)
        g_out = model(sp, glue.lerp(gl_c, gl_w, 1.0), target=None, command="decode")
        coeffs = ops.guided_filter_coeffs(glue.tensor2im(content), glue.tensor2im(g_out), 30, (0.02 * 255) ** 2)
        matte = ops.label_matte(labels, (1, 2), mf, mg)
        hand = ops.guided_filter_paste(coeffs, photo, xf, feather, matte=matte)
        assert hand.dtype == torch.uint8 and tuple(hand.shape) == (1, 700, 900, 3)
        assert torch.equal(hand, got), "simple_swap_region_matte differs from its steps by hand"
        assert np.array_equal(matte[0].cpu().numpy().astype(np.float64) > 0, M.matte(M.sd2_separable(lab, M.FACE, mf, mg), mf, mg) > 0)
        onehot = torch.nn.functional.one_hot(labels.long(), 3).permute(0, 3, 1, 2).float()
        for kw in (dict(labels=labels.long()), dict(labels=onehot), dict(matte=matte)):
            again = EV.simple_swap_region_matte(model, photo, xf, style, (1.0,), 512, feather, keep=(1, 2), matte_feather=mf, matte_grow=mg, **kw)
            assert torch.equal(again[1.0], got), sorted(kw)
        plain = EV.simple_swap_region(model, photo, xf, style, (1.0,), 512, feather)[1.0]
        kept = EV.simple_swap_region_matte(model, photo, xf, style, (1.0,), 512, feather, labels=labels, keep=(0, 1, 2), matte_feather=0,
                                           matte_grow=0)[1.0]
        assert torch.equal(kept, plain), "every label kept, no feather, no grow: not the swap without labels"
        assert not torch.equal(got, plain)
    out, pl = got[0].cpu().numpy(), plain[0].cpu().numpy()
    # where the restatement's weight is 0 the bytes are the photo's; where the matte is 1 around a pixel they are the plain swap's
    M32 = matte[0].cpu().numpy()
    _, g64 = M.paste_matte(np.zeros((12, 512, 512), np.float32), M32, arr[0], xf, feather, np.float64, want_g=True)
    _, g1 = M.paste_matte(np.zeros((12, 512, 512), np.float32), np.ones_like(M32), arr[0], xf, feather, np.float64, want_g=True)
    inside = C.inside(xf, 512, 700, 900)[0]
    zero, full = g64 == 0, inside & (g64 == g1)
    assert np.array_equal(out[zero], arr[0][zero]) and 0.2 < (zero & inside).mean() / inside.mean() < 0.9
    assert np.array_equal(out[full], pl[full]) and full.mean() > 0.05
    assert (pl[zero & inside] != arr[0][zero & inside]).mean() > 0.3, "the plain swap left the background as it was: nothing is shown"


def test_evaluate_swap_files_region_with_label_files(model, tmp_path):
    """two structure files with a label PNG each (one at load_size, one at 256 x 256, resized NEAREST): the written files decode to
    simple_swap_region_matte's tensors"""
    from PIL import Image
    from ppst_amd import evaluation as EV, imageio
    dev = _dev()
    arr = _photos(49, 2, 600, 800)
    sq = _photos(51, 1, 640, 640)
    cp, dp, qp = str(tmp_path / "c0.png"), str(tmp_path / "d1.png"), str(tmp_path / "q2.png")
    Image.fromarray(arr[0]).save(cp)
    Image.fromarray(arr[1]).save(dp)
    Image.fromarray(sq[0]).save(qp)
    l0, l1 = M._blob(512, 512, 6), M._blob(256, 256, 7)
    lp0, lp1 = str(tmp_path / "l0.png"), str(tmp_path / "l1.png")
    Image.fromarray(l0).save(lp0)
    Image.fromarray(l1).save(lp1)
    l1_512 = np.asarray(Image.fromarray(l1).resize((512, 512), Image.NEAREST))
    boxes = [(400.0, 300.0, 560.0, 15.0), (390.0, 310.0, 580.0, -5.0)]
    xfs = [imageio.crop_transform(b[:2], b[2], b[3]) for b in boxes]
    photos = torch.from_numpy(arr).to(dev)
    labels = torch.from_numpy(np.stack([l0, l1_512])).to(dev)
    with torch.no_grad():
        whole = EV.load_images([qp], 512, dev)[0]
        want = EV.simple_swap_region_matte(model, photos, xfs, torch.cat([whole, whole], 0), (1.0,), 512, 8, labels=labels, keep=(1,),
                                           matte_feather=10, matte_grow=4)[1.0]
        paths = EV.evaluate_swap_files_region(model, [cp, dp], qp, str(tmp_path / "o"), boxes, feather=8, label_path=[lp0, lp1], keep=(1,),
                                              matte_feather=10, matte_grow=4)
    assert [os.path.basename(p) for p in paths] == ["c0_q2_1.00.png", "d1_q2_1.00.png"]
    for i, p in enumerate(paths):
        assert np.array_equal(np.asarray(Image.open(p)), want[i].cpu().numpy()), p
    assert not np.array_equal(want[0].cpu().numpy(), arr[0])
