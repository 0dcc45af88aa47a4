"""GPU: the colour statistics and the style-fidelity metrics (csrc/colour_stats.hip, ppst_amd/metrics.py, evaluation.style_fidelity,
training.HeldOutEvaluator(swaps=True)) against the judges of tests/colour_cases.py (pinned on the CPU by test_colour_cpu.py) --
pytest -m gpu.

Histograms, counts and W1 numerators are integers and must be EQUAL to the judges'.  The Lab moments follow the project's rule
for fp32 streaming kernels (tests/BACKWARD_KERNELS.md section 3), computed per case, never a constant chosen here:
``max(2e-6, 4 x |float32 torch evaluation of the judge - its float64 evaluation|)`` relative to max |ref|; ``delta_e`` and
``frechet`` are judged from the judge's own moments with bars propagated from the moments' bars (colour_cases.distance_bars
states the propagation).  Each test prints its err / bar rows (-s shows them).  Which kernel edge each case reaches:
colour_cases.CASES.  Every argument the entry points refuse is checked on the CPU (test_colour_cpu.py); nothing here drives a
kernel with one.
"""
import math
import os

import numpy as np
import pytest
import torch

import colour_cases as C

pytestmark = pytest.mark.gpu

NAMES = list(C.CASES)
_CASES = {}


def _case(name):
    """inputs, the judges' statistics of them and the bars -- computed once, shared by the tests, never written to.  ``img2`` /
    ``labels2``: a second batch of the same shape (another seed, the label maps in reverse batch order) for the distances."""
    if name not in _CASES:
        c = C.make_case(name)
        kind = C.CASES[name].get("kind", "smooth")
        c["img2"] = C.make_images(900 + NAMES.index(name), *c["img"].shape[:3], kind="corners" if kind == "corners" else "smooth")
        c["labels2"] = None if c["labels"] is None else c["labels"].flip(0).contiguous()
        for tag, img, lab in (("", c["img"], c["labels"]), ("2", c["img2"], c["labels2"])):
            c["hist" + tag], c["count" + tag] = C.hist_judge(img.numpy(), None if lab is None else lab.numpy(), c["R"], c["dirs"])
            c["mean" + tag], c["cov" + tag] = C.lab_judge(img, lab, c["R"])
            m32, c32 = C.lab_judge(img, lab, c["R"], torch.float32)
            c["mean_bar" + tag], c["cov_bar" + tag] = C.moment_bar(c["mean" + tag], m32), C.moment_bar(c["cov" + tag], c32)
        _CASES[name] = c
    return _CASES[name]


def _stats(c, tag=""):
    from ppst_amd import metrics
    lab = c["labels" + tag]
    return metrics.colour_stats(c["img" + tag].cuda(), None if lab is None else lab.cuda(), c["R"], torch.from_numpy(c["dirs"]))


def _same_bits(a, b):
    return (torch.equal(a.hist, b.hist) and torch.equal(a.count, b.count) and torch.equal(a.lab_mean, b.lab_mean)
            and torch.equal(a.lab_cov, b.lab_cov))


def _row(what, name, err, bar):
    print("  %-10s %-14s err %.3g  bar %.3g" % (what, name, err, bar))


@pytest.mark.parametrize("name", NAMES)
def test_statistics_against_the_judges(name):
    c = _case(name)
    st = _stats(c)
    B, R, P = c["img"].shape[0], c["R"], len(c["dirs"])
    assert tuple(st.hist.shape) == (B, R, P, 256) and tuple(st.count.shape) == (B, R)
    assert tuple(st.lab_mean.shape) == (B, R, 3) and tuple(st.lab_cov.shape) == (B, R, 3, 3) and st.lab_mean.dtype == torch.float64
    assert np.array_equal(st.hist.cpu().numpy().astype(np.int64), c["hist"])
    assert np.array_equal(st.count.cpu().numpy().astype(np.int64), c["count"])
    assert torch.equal(st.lab_cov, st.lab_cov.transpose(-1, -2))
    print()
    for what, got, ref, bar in (("lab_mean", st.lab_mean, c["mean"], c["mean_bar"]), ("lab_cov", st.lab_cov, c["cov"], c["cov_bar"])):
        err = C.relative_error(ref, got)
        _row(what, name, err, bar)
        assert err <= bar
    empty = torch.from_numpy(c["count"] == 0)
    assert torch.count_nonzero(st.lab_mean.cpu()[empty]) == 0 and torch.count_nonzero(st.lab_cov.cpu()[empty]) == 0
    if C.CASES[name].get("kind") == "flat":                     # every pixel of a region has one value: it cancels exactly
        assert torch.count_nonzero(st.lab_cov) == 0
        assert torch.equal(st.lab_mean, st.lab_mean.float().double())                  # and the mean is the pixels' fp32 value
    if "window" in c:                                           # the crop view is read in place and gives the copy's bits
        from ppst_amd import metrics
        y, x = c["window"]
        view, lview = c["big_img"].cuda()[:, y, x], c["big_labels"].cuda()[:, y, x]
        assert not view.is_contiguous() and view.stride(1) != 3 * view.shape[2] and view.stride(2) == 3
        assert _same_bits(st, metrics.colour_stats(view, lview, R, torch.from_numpy(c["dirs"])))


@pytest.mark.parametrize("name", NAMES)
def test_w1_numerators_and_distances(name):
    """pairs: every (n, n), the batch rotated by one (for B > 1 a permutation without fixed points), and -- in the ignore case
    -- both images whose region 2 is empty (image 1 of the first batch, image 0 of the second)"""
    from ppst_amd import metrics, ops
    c = _case(name)
    a, b = _stats(c), _stats(c, "2")
    B, R, P = c["img"].shape[0], c["R"], len(c["dirs"])
    pairs = [(n, n) for n in range(B)] + [(n, (n + 1) % B) for n in range(B)]
    num = ops.hist_w1(a.hist, b.hist, pairs)
    assert tuple(num.shape) == (len(pairs), R, P) and num.dtype == torch.int64
    ref = [[[C.w1_numerator(c["hist"][i, r, p], c["hist2"][j, r, p]) for p in range(P)] for r in range(R)] for i, j in pairs]
    assert num.cpu().tolist() == ref
    assert ops.hist_w1(a.hist, a.hist, [(n, n) for n in range(B)]).abs().max().item() == 0          # a histogram with itself
    got = metrics.colour_distance(a, b, pairs)
    want = C.distance_judge(c["hist"], c["count"], c["mean"], c["cov"], c["hist2"], c["count2"], c["mean2"], c["cov2"], c["dirs"], pairs)
    assert sorted(got) == sorted(want)
    nan = np.isnan(want["w1_rgb"])
    assert np.array_equal(nan, (c["count"][[i for i, _ in pairs]] == 0) | (c["count2"][[j for _, j in pairs]] == 0))
    if C.CASES[name].get("ignore"):                             # region 2 is empty in image 1 of the first batch and image 0 of the second:
        assert nan[:, 2].tolist() == [True, True, False, True] and not nan[:, :2].any()     # pairs (0,0) (1,1) (0,1) (1,0); the rest is finite
    mean_scale = max(c["mean"].abs().max().item(), c["mean2"].abs().max().item())
    cov_scale = max(c["cov"].abs().max().item(), c["cov2"].abs().max().item())
    mean_bar, cov_bar = max(c["mean_bar"], c["mean_bar2"]), max(c["cov_bar"], c["cov_bar2"])
    print()
    for key in sorted(want):
        g, w = got[key].numpy(), want[key]
        assert g.shape == w.shape == (len(pairs), R) and g.dtype == np.float64
        if P <= 4 and key == "swd" or P < 4 and key == "w1_luma":
            assert np.isnan(g).all()
            continue
        assert np.array_equal(np.isnan(g), nan), key
        if key in ("w1_rgb", "w1_luma", "swd"):                 # exact numerators over exact counts, then float64 means
            err = np.nanmax(np.abs(g - w) / np.maximum(np.abs(w), 1.0)) if (~nan).any() else 0.0
            _row(key, name, err, 1e-13)
            assert err <= 1e-13
            continue
        worst = 0.0
        for k in range(len(pairs)):
            for r in range(R):
                if nan[k, r]:
                    continue
                bars = C.distance_bars(mean_bar, mean_scale, cov_bar, cov_scale, want["delta_e"][k, r], want["frechet"][k, r])
                bar = bars[0] if key == "delta_e" else bars[1]
                worst = max(worst, abs(g[k, r] - w[k, r]) / bar)
                assert abs(g[k, r] - w[k, r]) <= bar, (key, k, r, g[k, r], w[k, r], bar)
        _row(key, name, worst, 1.0)                             # (the largest err / bar over pairs and regions)


def test_repeats_batches_and_streams_give_the_same_bits():
    from ppst_amd import metrics
    c = _case("33x70")
    first = _stats(c)
    for _ in range(2):
        assert _same_bits(first, _stats(c))
    img, lab, d = c["img"].cuda(), c["labels"].cuda(), torch.from_numpy(c["dirs"])
    for n in range(img.shape[0]):                               # an image alone: the bits it has inside its batch
        assert _same_bits(first[n:n + 1], metrics.colour_stats(img[n:n + 1], lab[n:n + 1], c["R"], d))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = metrics.colour_stats(img, lab, c["R"], d)
        dist = metrics.colour_distance(on_side, on_side, [(0, 1), (2, 0)])
    side.synchronize()
    assert _same_bits(first, on_side)
    ref = metrics.colour_distance(first, first, [(0, 1), (2, 0)])
    assert all(torch.equal(dist[k], ref[k]) for k in ref)


def test_float_images_and_one_hot_masks():
    from ppst_amd import glue, metrics
    c = _case("33x70")
    B, H, W, _ = c["img"].shape
    x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(3)).mul_(2.4).sub_(1.2).cuda()    # some of it beyond [-1, 1]
    lab = c["labels"].cuda()
    from_float = metrics.colour_stats(x, lab, c["R"])
    assert _same_bits(from_float, metrics.colour_stats(glue.tensor2im(x), lab, c["R"]))
    assert tuple(from_float.hist.shape) == (B, c["R"], 16, 256)                                           # the default table
    assert _same_bits(from_float, metrics.colour_stats(x, glue.one_hot_mask(lab.long(), c["R"]), c["R"]))
    assert _same_bits(from_float, metrics.colour_stats(x, lab.long(), c["R"]))                            # any integer type


def test_style_fidelity():
    """on a tensor and on a hand-made {(i, j): image} dict it is ``colour_distance`` of the by-hand statistics; an image against
    itself scores 0 everywhere; a "swap" that returns the content unchanged scores exactly the distance between style and content"""
    from ppst_amd import evaluation as EV
    from ppst_amd import metrics
    c = _case("33x70")
    R = c["R"]
    u8, lab = c["img"].cuda(), c["labels"].cuda()
    u8b, labb = c["img2"].cuda(), c["labels2"].cuda()
    styles, contents = u8, u8b
    got = EV.style_fidelity(styles, contents, lab, labb)
    want = metrics.colour_distance(metrics.colour_stats(styles, lab, R), metrics.colour_stats(contents, labb, R))
    assert sorted(got) == ["delta_e", "frechet", "swd", "w1_luma", "w1_rgb"]
    for k in want:
        assert tuple(got[k].shape) == (3, R) and got[k].dtype == torch.float64 and torch.equal(got[k], want[k]), k
    assert float(got["w1_rgb"].min()) > 0.5 and float(got["delta_e"].min()) > 0.1      # different images: nothing near zero
    same = EV.style_fidelity(styles, styles, lab, lab)
    trace = metrics.colour_stats(styles, lab, R).lab_cov.diagonal(dim1=-2, dim2=-1).sum(-1).cpu()
    for k in same:                                              # exactly 0, but for the rounding of frechet's float64 square roots
        assert torch.count_nonzero(same[k]) == 0 or (k == "frechet" and bool((same[k].abs() <= 1e-12 * 2.0 * trace).all())), k
    whole = EV.style_fidelity(styles, contents)                                         # without labels: one region
    assert all(tuple(v.shape) == (3, 1) for v in whole.values())
    assert torch.equal(whole["w1_rgb"], metrics.colour_distance(metrics.colour_stats(styles), metrics.colour_stats(contents))["w1_rgb"])
    # the dict of swapping_grid: pair (i, j) against styles[j], with the CONTENT's regions
    outs = {(0, 2): contents[0], (1, 0): contents[1], (2, 2): contents[2]}             # "swaps" that return the content unchanged
    by_pair = EV.style_fidelity(styles, outs, lab, labb)
    assert sorted(by_pair) == [(0, 2), (1, 0), (2, 2)]
    st_s, st_c = metrics.colour_stats(styles, lab, R), metrics.colour_stats(contents, labb, R)
    blind = metrics.colour_distance(st_s, st_c, [(2, 0), (0, 1), (2, 2)])              # colour_distance(style, content)
    for n, key in enumerate(sorted(by_pair)):
        for k in blind:
            assert by_pair[key][k] == blind[k][n].tolist(), (key, k)
        assert min(by_pair[key]["w1_rgb"]) > 0.5                                         # ... which is far from a perfect score
    assert EV.style_fidelity(styles, {}) == {}
    # fp32 images in [-1, 1] go through the same quantisation
    x = (u8.permute(0, 3, 1, 2).float() + 0.5) / 127.5 - 1.0
    assert torch.equal(EV.style_fidelity(x, x[[1, 2, 0]])["swd"], metrics.colour_distance(metrics.colour_stats(x), metrics.colour_stats(x[[1, 2, 0]]))["swd"])


def test_held_out_evaluator_with_swaps(tmp_path):
    """a seeded model at 512^2, no noise, two images: the old keys keep their values bit for bit, the new ones are finite,
    non-negative and equal the by-hand composition, and the log line carries them"""
    from ppst_amd import evaluation as EV
    from ppst_amd import weights as W
    from ppst_amd.ppst_model import create_model
    from ppst_amd.training import HeldOutEvaluator
    m = create_model(state_dict=W.make_state_dict(2, with_D=False, with_nce=False, bias_std=0.1), device="cuda")
    m.noise = None
    x = W.synthetic_images(31, 2, size=512).cuda()
    g = torch.Generator().manual_seed(7)
    labels = torch.randint(0, 3, (2, 32, 32), generator=g).repeat_interleave(16, 1).repeat_interleave(16, 2).cuda()
    old = HeldOutEvaluator(x)(m, 10)
    path = os.path.join(str(tmp_path), "eval_log.txt")
    ev = HeldOutEvaluator(x, log_path=path, swaps=True, labels=labels)
    res = ev(m, 20)
    assert sorted(old) == ["l1", "ms_ssim", "psnr", "ssim"] and all(res[k] == old[k] for k in old)
    style_keys = ["swap_style_w1", "swap_style_swd", "swap_style_delta_e"]
    new = ["swap_content_ssim", "identity_style_w1"] + style_keys + ["%s_r%d" % (k, r) for k in style_keys for r in range(3)]
    assert sorted(res) == sorted(list(old) + new)
    assert all(math.isfinite(res[k]) and res[k] >= 0.0 for k in new)
    with torch.no_grad():
        out = EV.simple_swap(m, x, x[[1, 0]])[1.0]
    assert res["swap_content_ssim"] == float(EV.content_preservation(x, out).double().mean().item())
    fid = EV.style_fidelity(x[[1, 0]], out, labels[[1, 0]], labels)
    nanmean = lambda t: float(t[~t.isnan()].mean().item())     # over pairs and non-empty regions
    for key, name in (("swap_style_w1", "w1_rgb"), ("swap_style_swd", "swd"), ("swap_style_delta_e", "delta_e")):
        assert not fid[name].isnan().any() and res[key] == nanmean(fid[name])
        for r in range(3):
            assert res["%s_r%d" % (key, r)] == nanmean(fid[name][:, r])
    assert res["identity_style_w1"] == nanmean(EV.style_fidelity(x[[1, 0]], x, labels[[1, 0]], labels)["w1_rgb"])
    assert res["identity_style_w1"] > 0.0
    plain = HeldOutEvaluator(x, swaps=True).evaluate_swaps(m)   # without labels: the whole image is one region, no per-region keys
    assert sorted(plain) == sorted(["swap_content_ssim", "identity_style_w1"] + style_keys)
    assert plain["swap_content_ssim"] == res["swap_content_ssim"] and plain["swap_style_w1"] > 0.0
    with open(path) as f:
        written = f.read().splitlines()
    assert written == [HeldOutEvaluator.format(20, res)] and all(("%s: " % k) in written[0] for k in new)
    print("\n" + written[0])
