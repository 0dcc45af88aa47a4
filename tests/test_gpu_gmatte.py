"""GPU: a matte refined by the photo's own pixels -- the guided filter's coefficients for a one-channel source
(csrc/guided_filter.hip gfm_h_kernel / gfm_solve_kernel; ops.guided_matte_coeffs) and the paste that evaluates the matte from them
on each photo pixel (gf_paste_kernel<GP_COEFFS>; ops.guided_filter_paste_gmatte; PPSTModel.decode_region_gmatte;
evaluation.simple_swap_region_gmatte / evaluate_swap_files_region_gmatte) against the restatements on the CPU
(tests/gmatte_cases.py) -- pytest -m gpu.  The device is never its own judge, except where the issue is equality of two of its own
entries: the matte coefficients are BIT-EQUAL to planes 0..3 of ops.guided_filter_coeffs on the replicated source.

Bars: coefficients against float64 2 max|planes32 - planes64| + 1e-6 max|planes64| (gf_native_cases.plane_ref's rule); paste
gf_cases.judge(ref64, device, tau), tau = 2 max|ref32 - ref64| + 1e-3, bytes outside the square or under a zero weight EQUAL the
photo's; the weight output likewise against 255 g64, 0 outside the square.  Every test prints the tolerance the device needed.
tests/test_gmatte_cases_cpu.py shows that the cases see every seeded defect through these bars.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gf_cases as G  # noqa: E402
import gf_native_cases as N  # noqa: E402
import gmatte_cases as GM  # noqa: E402
import matte_cases as M  # noqa: E402
import region_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", 0)


def _t(a):
    return torch.from_numpy(np.array(a, order="C")).to(_dev())        # (a copy: the cached references are read-only)


def _mco(guides, mattes, r, eps=GM.EPS):
    from ppst_amd import ops
    out = ops.guided_matte_coeffs(_t(np.stack(guides)), _t(np.stack(mattes)), r, eps)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _colour(guides, mattes, r, eps=GM.EPS):
    """planes 0..3 of the 12-plane entry on the replicated source bytes"""
    from ppst_amd import ops
    src = np.stack([np.repeat(GM.source_u8(m)[..., None], 3, axis=-1) for m in mattes])
    out = ops.guided_filter_coeffs(_t(np.stack(guides)), _t(src), r, eps)[:, :4]
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _paste(planes, mcos, photos, xfs, feather, **kw):
    from ppst_amd import ops
    out = ops.guided_filter_paste_gmatte(_t(np.stack(planes)), _t(np.stack(mcos)), _t(np.stack(photos)), list(xfs), feather, **kw)
    torch.cuda.synchronize()
    if isinstance(out, tuple):
        return out[0].cpu().numpy(), out[1].cpu().numpy()
    return out.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------- coefficients
@pytest.mark.parametrize("case", GM.COEFF_CASES, ids=lambda c: "%s-%dx%d-r%d" % c)
def test_coefficients_are_bit_equal_to_the_colour_entry_on_the_replicated_source(case):
    kind, h, w, r = case
    g = G.inputs(kind, h, w)[0]
    for name in GM.MATTES:
        m = GM.matte_of(name, h, w)
        got, want = _mco([g], [m], r), _colour([g], [m], r)
        assert got.shape == (1, 4, h, w)
        differ = int((got.view(np.uint32) != want.view(np.uint32)).sum())
        print("%s-%dx%d-r%d %-12s differing words %d  max|planes| %.4g" % (case + (name, differ, float(np.abs(want).max()))))
        assert _same_bits(got, want), "%s: %d words differ from planes 0..3 of guided_filter_coeffs" % (name, differ)
        if name == "zeros":
            assert (got == 0).all(), "an all-zero matte must give exactly zero coefficients"


def test_coefficients_at_512_and_in_a_batch():
    g = G.inputs("blocks", 512, 512)[0]
    m = GM.blob_matte(512, 512)
    assert _same_bits(_mco([g], [m], 8), _colour([g], [m], 8)), "512 x 512, r = 8"
    h, w = 70, 90
    gs = [G.inputs(k, h, w)[0] for k in ("blocks", "flat", "saturating")]
    ms = [GM.matte_of(n, h, w) for n in ("blob", "uniform-nan", "ties")]
    both = _mco(gs, ms, 3, 1.0)
    assert both.shape == (3, 4, h, w) and _same_bits(both, _colour(gs, ms, 3, 1.0))
    for i in range(3):
        assert _same_bits(_mco(gs[i:i + 1], ms[i:i + 1], 3, 1.0)[0], both[i]), "image %d of the batch differs from its single call" % i
    assert not np.array_equal(both[0], both[1])


@pytest.mark.parametrize("case", N.PLANE_CASES, ids=lambda c: "%s-%dx%d-r%d" % c)
def test_coefficients_against_float64(case):
    g, m, p64, bar, floor32 = GM.plane_ref(*case)
    got = _mco([g], [m], case[3])[0]
    err = float(np.abs(got.astype(np.float64) - p64).max())
    print("%s-%dx%d-r%d: max|planes64| %.4g  bar %.3e (max|planes32 - planes64| %.2e)  device needs %.3e"
          % (case + (float(np.abs(p64).max()), bar, floor32, err)))
    assert err <= bar, "matte coefficients off by %.3e > %.3e" % (err, bar)


def test_coefficient_views_empty_batch_and_refusals():
    from ppst_amd import ops
    h, w = 70, 90
    g, m = G.inputs("blocks", h, w)[0], GM.blob_matte(h, w)
    want = _mco([g], [m], 3)
    pad = torch.zeros((1, h + 5, 2 * w + 9), device=_dev())
    pad[:, 2:2 + h, 4:4 + 2 * w:2] = _t(m[None])
    view = pad[:, 2:2 + h, 4:4 + 2 * w:2]
    assert not view.is_contiguous()
    assert _same_bits(ops.guided_matte_coeffs(_t(g[None]), view, 3).cpu().numpy(), want), "a non-contiguous matte differs from its copy"
    e = ops.guided_matte_coeffs(_t(g[None])[:0], _t(m[None])[:0], 3)
    assert tuple(e.shape) == (0, 4, h, w) and e.dtype == torch.float32
    for r in (0, 65, 70, 90):
        with pytest.raises(RuntimeError, match="ppst_guided_matte_coeffs"):
            ops.guided_matte_coeffs(_t(g[None]), _t(m[None]), r)
    with pytest.raises(RuntimeError, match="float32 matte"):
        ops.guided_matte_coeffs(_t(g[None]), _t(m[None]).cpu(), 3)


# -------------------------------------------------------------------------------------------------------------------- paste
@pytest.mark.parametrize("case", C.ALL_CASES, ids=C.case_id)
def test_paste_and_weight_against_float64(case):
    R = GM.paste_ref(case)
    got, wgt = _paste([R.planes], [R.mco], [R.photo], [R.xf], R.feather, want_weight=True)
    got, wgt = got[0], wgt[0]
    d = np.abs(got.astype(int) - R.expect.astype(int))
    print("%-24s r %d tau %.5f (max|r32-r64| %.2e)  device needs %.5f  max |diff| %d  differing %.5f  exempt %.4f | weight tau %.5f  device needs %.5f"
          % (case[0], R.r, R.tau, R.floor32, G.min_tau(R.ref64, got), d.max(), (d > 0).mean(), R.exempt, R.wtau, G.min_tau(R.w64, wgt)))
    assert wgt.dtype == np.uint8 and wgt.shape == R.photo.shape[:2]
    bad = GM.judge_paste(R, got) + ["weight: " + b for b in GM.judge_weight(R, wgt)]
    assert not bad, "%s: %s" % (case[0], "; ".join(bad))
    plain = _paste([R.planes], [R.mco], [R.photo], [R.xf], R.feather)[0]
    assert np.array_equal(plain, got), "want_weight changed the image"


@pytest.mark.parametrize("case", GM.LEAK_CASES, ids=C.case_id)
def test_poison_under_zero_matte_coefficients_cannot_leak(case):
    R = GM.paste_ref(case)
    mco = _mco([R.guide], [GM.disc_matte(R.n)], GM.LEAK_R)[0]
    bad = GM.poison(R.planes, mco)
    share = float(np.isnan(bad[0]).mean())
    print("%-24s poisoned share of the planes %.2f" % (case[0], share))
    assert share > 0, "no coefficient sample is poisoned: the case shows nothing"
    clean = _paste([R.planes], [mco], [R.photo], [R.xf], R.feather)[0]
    got = _paste([bad], [mco], [R.photo], [R.xf], R.feather)[0]
    assert np.array_equal(got, clean), "non-finite coefficients under zero matte coefficients leaked"
    assert not np.array_equal(clean, R.photo), "the clean run wrote nothing"


def test_paste_batch_in_place_given_views_and_refusals():
    """three transforms in one call: every image bit-equal to its single call; in place equals cloned equals into a given tensor;
    non-contiguous matte coefficients equal their copy; refusals write nothing"""
    from ppst_amd import ops
    cs = [C.lookup(c) for c in C.BATCH]
    Ps = [C.PasteRef(c) for c in cs]
    n, xfs, feather = Ps[0].n, [p.xf for p in Ps], 3
    photos = [np.ascontiguousarray(np.roll(Ps[0].photo, 7 * i, axis=1)) for i in range(3)]
    planes = [p.planes for p in Ps]
    guides = [np.ascontiguousarray(C.extract_ref(c).expect) for c in cs]
    mattes = [M.matte(M.sd2_separable(M._blob(n, n, 10 + i), M.FACE, f, g), f, g, np.float32) for i, (f, g) in enumerate(((6, 3), (1, 0), (0, 2)))]
    mcos = list(_mco(guides, mattes, 3))
    out, wgt = _paste(planes, mcos, photos, xfs, feather, want_weight=True)
    for i in range(3):
        oi, wi = _paste([planes[i]], [mcos[i]], [photos[i]], [xfs[i]], feather, want_weight=True)
        assert np.array_equal(oi[0], out[i]) and np.array_equal(wi[0], wgt[i]), "image %d" % i
        want = GM.paste_gmatte(planes[i], mcos[i], photos[i], xfs[i], feather, np.float64)
        assert np.abs(out[i].astype(int) - G.round_u8(want).astype(int)).max() <= 1
    assert not np.array_equal(out[0], out[1])
    P, CO, MC = _t(np.stack(photos)), _t(np.stack(planes)), _t(np.stack(mcos))
    given = torch.full_like(P, 201)
    assert ops.guided_filter_paste_gmatte(CO, MC, P, xfs, feather, out=given) is given and np.array_equal(given.cpu().numpy(), out)
    inplace = P.clone()
    assert ops.guided_filter_paste_gmatte(CO, MC, inplace, xfs, feather, out=inplace) is inplace and np.array_equal(inplace.cpu().numpy(), out)
    assert np.array_equal(P.cpu().numpy(), np.stack(photos)), "the cloned form wrote into its photo"
    pad = torch.zeros((3, 4, n + 5, n + 9), device=_dev())
    pad[:, :, 2:2 + n, 4:4 + n] = MC
    assert np.array_equal(ops.guided_filter_paste_gmatte(CO, pad[:, :, 2:2 + n, 4:4 + n], P, xfs, feather).cpu().numpy(), out)
    with pytest.raises(RuntimeError, match="float32 matte coefficients"):
        ops.guided_filter_paste_gmatte(CO, MC[:, :3], P, xfs, feather)
    with pytest.raises(RuntimeError, match="float32 matte coefficients"):
        ops.guided_filter_paste_gmatte(CO, MC.cpu(), P, xfs, feather)
    keep = P.clone()
    with pytest.raises(RuntimeError, match="ppst_guided_filter_paste_gmatte"):
        ops.guided_filter_paste_gmatte(CO, MC, keep, xfs, n, out=keep)
    assert torch.equal(keep, P), "a refused paste wrote"
    p, w = ops.guided_filter_paste_gmatte(CO[:0], MC[:0], P[:0], torch.zeros((0, 4), dtype=torch.int64), 0, want_weight=True)
    assert tuple(p.shape) == (0,) + tuple(P.shape[1:]) and tuple(w.shape) == (0,) + tuple(P.shape[1:3])


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


def test_simple_swap_region_gmatte_is_its_steps_by_hand(model):
    """simple_swap_region_gmatte(labels=) at load_size 512 inside a 700 x 900 photo against extract -> swap_codes -> generator ->
    guided_filter_coeffs -> label_matte -> guided_matte_coeffs -> guided_filter_paste_gmatte by hand through facade commands, bit
    for bit; a ready matte gives the same bytes; want_weight returns the same image beside the weight; the result differs from
    the plane matte's, and bytes under a zero weight are the photo's"""
    from ppst_amd import evaluation as EV, glue, imageio, ops
    dev = _dev()
    arr = _photos(47, 2, 700, 900)
    photo, style_photo = torch.from_numpy(arr[0:1]).to(dev), torch.from_numpy(arr[1:2]).to(dev)
    xf = imageio.crop_transform((470.0, 340.0), 600.0, 20.0, 512)
    sxf = imageio.crop_transform((400.0, 350.0), 640.0, -10.0, 512)
    feather, mf, mg, mr, me = 16, 24, 12, 5, 9.0
    labels = torch.from_numpy(M._blob(512, 512, 5)[None]).to(dev)
    with torch.no_grad():
        got = EV.simple_swap_region_gmatte(model, photo, xf, style_photo, (1.0,), 512, feather, style_xf=sxf, labels=labels, keep=(1, 2),
                                           matte_feather=mf, matte_grow=mg, matte_radius=mr, matte_eps=me)[1.0]
        content = imageio.to_tensor_normalized(ops.extract_similarity(photo, xf, 512))
        style = imageio.to_tensor_normalized(ops.extract_similarity(style_photo, sxf, 512))
        sp, gl_c, gl_w = EV.swap_codes(model, content, style)
        code = glue.lerp(gl_c, gl_w, 1.0)
        g_out = model(sp, code, target=None, command="decode")
        coeffs = ops.guided_filter_coeffs(glue.tensor2im(content), glue.tensor2im(g_out), 30, (0.02 * 255) ** 2)
        matte = ops.label_matte(labels, (1, 2), mf, mg)
        mco = ops.guided_matte_coeffs(glue.tensor2im(content), matte, mr, me)
        hand, hand_w = ops.guided_filter_paste_gmatte(coeffs, mco, photo, xf, feather, want_weight=True)
        assert hand.dtype == torch.uint8 and tuple(hand.shape) == (1, 700, 900, 3) and tuple(hand_w.shape) == (1, 700, 900)
        assert torch.equal(hand, got), "simple_swap_region_gmatte differs from its steps by hand"
        cmd = model(sp, code, content, photo, xf, feather, matte, mr, me, command="decode_region_gmatte")
        assert torch.equal(cmd, got), "the facade command differs from its steps by hand"
        again = EV.simple_swap_region_gmatte(model, photo, xf, style, (1.0,), 512, feather, matte=matte, matte_radius=mr, matte_eps=me,
                                             want_weight=True)[1.0]
        assert isinstance(again, tuple) and torch.equal(again[0], got) and torch.equal(again[1], hand_w)
        plane = EV.simple_swap_region_matte(model, photo, xf, style, (1.0,), 512, feather, matte=matte)[1.0]
        assert not torch.equal(got, plane), "the guided matte changed nothing"
    out, w = got[0].cpu().numpy(), hand_w[0].cpu().numpy()
    inside = C.inside(xf, 512, 700, 900)[0]
    assert (w[~inside] == 0).all() and w.max() == 255 and 0.1 < (w[inside] == 0).mean() < 0.9
    # the device's own weight plane cannot judge the device: the float64 restatement's weight on the device's coefficients does
    mc = mco[0].cpu().numpy()
    _, g64 = GM.paste_gmatte(np.zeros((12, 512, 512), np.float32), mc, arr[0], xf, feather, np.float64, want_g=True)
    zero = g64 == 0
    assert np.array_equal(out[zero], arr[0][zero]) and (zero & inside).any()
    # rint(255 g): half a level, + the fp32 evaluation of 255 m^ -- at most 16 roundings (4 taps, 3 interpolations and a 4-term
    # dot product per plane, the scale, the feather) of partial sums bounded by 255 sum|M_k| + |Mb|
    tol = 0.5 + 16 * 2.0 ** -24 * float((255.0 * np.abs(mc[:3]).sum(0) + np.abs(mc[3])).max())
    err = float(np.abs(w.astype(np.float64) - 255.0 * g64).max())
    print("weight of the 512^2 swap: |device - 255 g64| %.4f, bound %.4f" % (err, tol))
    assert err <= tol


def test_evaluate_swap_files_region_gmatte_is_the_tensor_path(model, tmp_path):
    """two structure files with a label PNG each: the written files decode to simple_swap_region_gmatte's tensors"""
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
        want = EV.simple_swap_region_gmatte(model, photos, xfs, torch.cat([whole, whole], 0), (1.0,), 512, 8, labels=labels, keep=(1,),
                                            matte_feather=10, matte_grow=4, matte_radius=4, matte_eps=20.0)[1.0]
        paths = EV.evaluate_swap_files_region_gmatte(model, [cp, dp], qp, str(tmp_path / "o"), boxes, feather=8, label_path=[lp0, lp1],
                                                     keep=(1,), matte_feather=10, matte_grow=4, matte_radius=4, matte_eps=20.0)
    assert [os.path.basename(p) for p in paths] == ["c0_q2_1.00.png", "d1_q2_1.00.png"]
    for i, p in enumerate(paths):
        assert np.array_equal(np.asarray(Image.open(p)), want[i].cpu().numpy()), p
    assert not np.array_equal(want[0].cpu().numpy(), arr[0])
