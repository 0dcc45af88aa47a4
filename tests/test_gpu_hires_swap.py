"""GPU: swaps above 512 x 512 (DESIGN.md "Swaps above 512^2") -- the fp32 resample kernel against float64, E2's warp at 1024^2,
the two-resolution recipe against its by-hand composition and against the CPU oracle's functions, and the front ends.

The reference cannot run a swap above 512^2 (its Rselfcorr / G.forward / E2.warp hard-code the 64 x 64 grid), so parity is pinned
per stage: the resample against torch's float64 antialiased bicubic, every network stage against the oracle's own layer functions
(imported, not edited) with the warp generalised here in three lines (pool to 64 x 64, matmul, bilinear back)."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
pytestmark = pytest.mark.gpu

# two fp32 passes of at most 17 taps, weight L1 norm about 1.3 per axis, |x| <= 1: about 3e-6 worst case (torch's own fp32 CPU
# kernel measures 1.2e-7 .. 2.4e-6 against the same judge on these shapes)
RESAMPLE_BOUND = 5e-6
# (B, C, H, W, OH, OW)
RESAMPLE_SHAPES = [
    (2, 3, 64, 64, 32, 32),        # the 2 : 1 case
    (1, 3, 37, 53, 16, 24),        # unequal non-integer scales, windows clipped at both borders
    (1, 1, 33, 70, 33, 35),        # one copied axis
    (1, 3, 40, 40, 13, 40),
    (1, 3, 24, 24, 48, 48),        # upsample
    (1, 3, 8, 8, 1, 1),
    (3, 3, 200, 300, 100, 150),    # several blocks on both axes
]


def _judge(x, oh, ow):
    return F.interpolate(x.double(), size=(oh, ow), mode="bicubic", antialias=True, align_corners=False)


def _uniform(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g) * 2 - 1


@pytest.mark.parametrize("shape", RESAMPLE_SHAPES, ids=lambda s: "%dx%dx%dx%d_to_%dx%d" % s)
def test_resample_f32_against_float64(shape):
    from ppst_amd import imageio, ops
    B, C, H, W, OH, OW = shape
    x = _uniform((B, C, H, W), 11 * H + W)
    ref = _judge(x, OH, OW)
    y = imageio.resize_tensor(x.cuda(), OH, OW)
    assert y.shape == (B, C, OH, OW) and y.dtype == torch.float32
    err = (y.cpu().double() - ref).abs().max().item()
    print("resample %s: max |err| %.3e" % (shape, err))
    assert err <= RESAMPLE_BOUND
    # the op under the front end takes any leading dimensions
    assert torch.equal(ops.resample_f32(x.cuda().view(B * C, H, W), OH, OW), y.view(B * C, OH, OW))


def test_resample_f32_clamp_and_empty_batch():
    from ppst_amd import imageio
    x = _uniform((1, 1, 33, 70), 179)          # (a seed whose float64 result overshoots at both ends: most do at one or none)
    ref = _judge(x, 33, 35)
    assert ref.min().item() < -1.0 and ref.max().item() > 1.0, "the case must overshoot for the clamp to be seen"
    y = imageio.resize_tensor(x.cuda(), 33, 35, clamp=(-1, 1)).cpu()
    assert y.min().item() >= -1.0 and y.max().item() <= 1.0
    err = (y.double() - ref.clamp(-1.0, 1.0)).abs().max().item()
    print("clamped resample: max |err| %.3e, unclamped range %.4f .. %.4f" % (err, ref.min().item(), ref.max().item()))
    assert err <= RESAMPLE_BOUND
    free = imageio.resize_tensor(x.cuda(), 33, 35).cpu()
    assert free.min().item() < -1.0 and free.max().item() > 1.0               # without the clamp the kernel overshoots too
    empty = imageio.resize_tensor(torch.empty(0, 3, 64, 64, device="cuda"), 32, 32, clamp=(-1, 1))
    assert empty.shape == (0, 3, 32, 32)
    with pytest.raises(RuntimeError):
        imageio.resize_tensor(x, 33, 35)                                        # host tensor: no fallback


# ------------------------------------------------------------------------------------------------ the model at 1024^2
_CTX = {}


def _ctx():
    """One model, one 1024^2 pair and the device-made 512^2 images for every test below (seeded weights with non-zero biases;
    the noise weights are zero: a pinned noise dict cannot serve the 512^2 and the 1024^2 generator passes of one recipe)."""
    if not _CTX:
        from ppst_amd import weights as W
        from ppst_amd.ppst_model import create_model
        sd = W.make_state_dict(2, with_D=False, with_nce=False, bias_std=0.1)
        m = create_model(state_dict=sd, device="cuda")
        m.noise = None
        imgs = W.synthetic_images(31, 2, size=1024)
        _CTX.update(sd=sd, m=m, content=imgs[0:1].cuda(), style=imgs[1:2].cuda(), imgs=imgs)
    return _CTX


def _e2_levels_cpu(c):
    """The four E2 trunk levels of the 1024^2 style image by the oracle's conv_layer / res_block (computed once)."""
    if "levels" not in c:
        import ppst_oracle as O
        sd, ch = c["sd"], [32, 64, 128, 256]
        with torch.no_grad():
            x = O.conv_layer(c["imgs"][1:2], sd, "E2.FromRGB.", 3, 32, 1)
            levels = [x]
            for i in range(3):
                x = O.res_block(x, sd, "E2.DownToGlobalCode1.ResBlockDownBy%d." % (2 ** i), ch[i], ch[i + 1], (1, 2, 1), reflection_pad=True)
                levels.append(x)
        c["levels"] = levels
    return c["levels"]


def _e2_codes_cpu(c, corr):
    """(gl, gl_w) of the oracle's heads; the warp of the reference (pool to 64 x 64, corr @ features, bilinear back) with the
    level's own size where the reference hard-codes the factors of a 512^2 image."""
    import ppst_oracle as O
    gl, gl_w = [], []
    with torch.no_grad():
        for tag, x in zip(["9", "0", "1", "2"], _e2_levels_cpu(c)):
            b, ch, h, w = x.shape
            gl.append(O._e2_head(c["sd"], "E2.", tag, x))
            pooled = F.adaptive_avg_pool2d(x, (64, 64)).reshape(b, ch, -1).permute(0, 2, 1)
            wf = torch.matmul(corr, pooled).permute(0, 2, 1).reshape(b, ch, 64, 64)
            if h != 64:
                wf = F.interpolate(wf, size=(h, w), mode="bilinear", align_corners=False)
            gl_w.append(O._e2_head(c["sd"], "E2.", tag, wf))
    return gl, gl_w


def _rel(a, b):
    return float((a.detach().cpu().double() - b.double()).abs().max() / b.double().abs().max())


def test_encode2_at_1024_with_a_correspondence_matrix():
    c = _ctx()
    m = c["m"]
    g = torch.Generator().manual_seed(7)
    corr = torch.softmax(4.0 * torch.randn((1, 4096, 4096), generator=g), dim=-1)
    with torch.no_grad():
        gl, gl_w = m(c["style"], corr.cuda(), command="encode2")
        gl_plain = m(c["style"], command="encode")[1]
    ref_gl, ref_gl_w = _e2_codes_cpu(c, corr)
    assert len(gl) == len(gl_w) == 4
    for lvl in range(4):
        assert gl_w[lvl].shape == (1, 2048)
        e, e_w = _rel(gl[lvl], ref_gl[lvl]), _rel(gl_w[lvl], ref_gl_w[lvl])
        print("E2 at 1024^2, level %d: rel err code %.3e, warped code %.3e" % (lvl, e, e_w))
        assert e < 1e-3 and e_w < 1e-3
        assert torch.equal(gl[lvl], gl_plain[lvl])
        assert _rel(gl_w[lvl], ref_gl[lvl]) > 1e-2, "the warped code must differ from the plain one"


def _by_hand(m, content, style, alphas):
    from ppst_amd import glue
    sp, gl_c = m(content, command="encode")
    corr = m(m(style, command="correspondence_features"), m(content, command="correspondence_features"), command="corrm")
    _, gl_w = m(style, corr, command="encode2")
    return sp, gl_w, {a: m(sp, glue.lerp(gl_c, gl_w, a), target=None, command="decode") for a in alphas}


def _swap_1024(c):
    if "swap" not in c:
        from ppst_amd.evaluation import simple_swap
        with torch.no_grad():
            c["swap"] = simple_swap(c["m"], c["content"], c["style"], alphas=(0.5, 1.0))
    return c["swap"]


def test_recipe_at_1024_is_its_by_hand_composition():
    c = _ctx()
    out = _swap_1024(c)
    with torch.no_grad():
        _, _, hand = _by_hand(c["m"], c["content"], c["style"], (0.5, 1.0))
    for a in (0.5, 1.0):
        assert out[a].shape == (1, 3, 1024, 1024) and torch.isfinite(out[a]).all()
        assert torch.equal(out[a], hand[a]), "alpha %.1f" % a
    assert not torch.equal(out[0.5], out[1.0])


def test_recipe_at_1024_against_the_oracle_functions():
    """The same four steps by the CPU oracle, fed the device-made 512^2 images (the resample has its own test)."""
    import ppst_oracle as O
    c = _ctx()
    m, sd = c["m"], c["sd"]
    out = _swap_1024(c)[1.0]
    with torch.no_grad():
        small_c = m(c["content"], command="correspondence_image").cpu()
        small_s = m(c["style"], command="correspondence_image").cpu()
        assert small_c.shape == (1, 3, 512, 512) and small_c.abs().max().item() <= 1.0
        orc = O.PPSTOracle(sd, noise=None)
        sp = O.encoder_con(sd, c["imgs"][0:1])
        fea_c, fea_c1 = orc.extract_feat_from_image(small_c)
        fea_s, fea_s1 = orc.extract_feat_from_image(small_s)
        corr = O.corrm(torch.cat((fea_s, O.rselfcorr(fea_s1)), 1), torch.cat((fea_c, O.rselfcorr(fea_c1)), 1))
        _, gl_w = _e2_codes_cpu(c, corr)
        ref = O.generator(sd, sp, gl_w, noise=None)            # alpha = 1: lerp(gl_c, gl_w, 1) = gl_w
    err = _rel(out, ref)
    print("1024^2 swap against the oracle's functions: rel err %.3e" % err)
    assert err < 1e-3


def test_recipe_at_512_is_unchanged():
    from ppst_amd import weights as W
    from ppst_amd.evaluation import simple_swap
    c = _ctx()
    m = c["m"]
    imgs = W.synthetic_images(32, 2).cuda()
    content, style = imgs[0:1], imgs[1:2]
    assert m(content, command="correspondence_image") is content          # the passthrough is an identity
    with torch.no_grad():
        out = simple_swap(m, content, style, alphas=(1.0,))[1.0]
        sp, gl_c = m(content, command="encode")
        fea_c, fea_c1 = m(content, command="extract_feat_from_image")
        fea_s, fea_s1 = m(style, command="extract_feat_from_image")
        corr = m(torch.cat((fea_s, m(fea_s1, command="Rselfcorr")), 1), torch.cat((fea_c, m(fea_c1, command="Rselfcorr")), 1), command="corrm")
        _, gl_w = m(style, corr, command="encode2")
        hand = m(sp, gl_w, target=None, command="decode")
        assert torch.equal(m(content, command="correspondence_features"), torch.cat((fea_c, m(fea_c1, command="Rselfcorr")), 1))
    assert out.shape == (1, 3, 512, 512) and torch.equal(out, hand)


# ------------------------------------------------------------------------------------------------------- front ends
def test_swapping_grid_at_1024():
    from ppst_amd import weights as W
    from ppst_amd.evaluation import swapping_grid
    c = _ctx()
    m = c["m"]
    cs = torch.cat((c["content"], W.synthetic_images(33, 1, size=1024).cuda()), 0)
    ss = torch.cat((c["style"], W.synthetic_images(34, 1, size=1024).cuda()), 0)
    with torch.no_grad():
        grid = swapping_grid(m, cs, ss, rank=0, world=1, smooth=True)
        assert sorted(grid) == [(0, 0), (0, 1), (1, 0), (1, 1)]
        for (i, j), img in sorted(grid.items()):
            assert img.shape == (3, 1024, 1024) and torch.isfinite(img).all()
            sp, gl_w, _ = _by_hand(m, cs[i:i + 1], ss[j:j + 1], ())
            want = m(sp, gl_w, target=cs[i:i + 1], command="decode")[0]
            assert torch.equal(img, want), "pair %s" % ((i, j),)
    assert not torch.equal(grid[(0, 0)], grid[(0, 1)]) and not torch.equal(grid[(0, 0)], grid[(1, 0)])


def test_evaluate_swap_files_at_1024(tmp_path):
    from PIL import Image
    from ppst_amd.evaluation import evaluate_swap_files, to_uint8_image
    c = _ctx()
    u8 = to_uint8_image(c["imgs"]).numpy()
    paths = []
    for name, arr in zip(("structure", "texture"), u8):
        paths.append(str(tmp_path / (name + ".png")))
        Image.fromarray(arr).save(paths[-1])
    with torch.no_grad():
        written = evaluate_swap_files(c["m"], paths[0], paths[1], str(tmp_path / "out"), alphas=(1.0,), load_size=1024)
    assert [os.path.basename(p) for p in written] == ["structure_texture_1.00.png"]
    with Image.open(written[0]) as im:
        im.load()
        assert im.size == (1024, 1024) and im.mode == "RGB"
