"""GPU: the colour-transfer baselines (csrc/colour_transfer.hip, ops.hist_match_lut / ops.colour_transfer_apply,
metrics.colour_transfer, evaluation.baseline_swap / baseline_grid, training.HeldOutEvaluator.set_baseline) against the judges of
tests/transfer_cases.py (pinned on the CPU by test_transfer_cases_cpu.py) -- pytest -m gpu.

The tables and the hard-label table look-up are integers and must be EQUAL to the judges'.  The weighted look-up and both affine
modes are held to the project's boundary-aware bar, ``gf_cases.judge(q64, device, tau)`` with ``tau = 2 max|q32 - q64| + 1e-3``
from the judges alone; each test prints the tau the device needed (-s shows it).  Bytes of pixels of no region must be the
input's.  Which kernel edge each case reaches: colour_cases.CASES and test_transfer_cases_cpu.test_case_table_reaches_the_stated_edges.
Every argument the entry points refuse is checked on the CPU; nothing here drives a kernel with one.
"""
import numpy as np
import pytest
import torch

import colour_cases as C
import gf_cases as G
import transfer_cases as T

pytestmark = pytest.mark.gpu


def _dev(c):
    """the case's tensors on the device (made once per case)"""
    if "dev" not in c:
        cu = lambda t: None if t is None else t.cuda()
        c["dev"] = dict(img=cu(c["img"]), labels=cu(c["labels"]), img_s=cu(c["img_s"]), labels_s=cu(c["labels_s"]),
                        weights=torch.from_numpy(c["weights"]).cuda(), luts=torch.from_numpy(c["luts"]).cuda(),
                        rows_mkl=torch.from_numpy(c["rows_mkl"]).cuda(), rows_reinhard=torch.from_numpy(c["rows_reinhard"]).cuda())
    return c["dev"]


def _apply(d, key, img=None, labels=None, sel=slice(None), out=None):
    from ppst_amd import ops
    maps, weighted = T.MODES[key] if key in T.MODES else ("luts", False)
    kw = {"luts" if maps == "luts" else "affine": d[maps][sel]}
    img = d["img"][sel] if img is None else img
    labels = (None if d["labels"] is None else d["labels"][sel]) if labels is None else labels
    return ops.colour_transfer_apply(img, labels, weights=d["weights"][sel] if weighted else None, out=out, **kw)


ALL_MODES = ["lut-hard"] + list(T.MODES)


@pytest.mark.parametrize("name", T.NAMES)
def test_tables_equal_the_integer_judge(name):
    from ppst_amd import metrics, ops
    c = T.reference(name)
    d = _dev(c)
    R, B = c["R"], c["img"].shape[0]
    st_c = metrics.colour_stats(d["img"], d["labels"], R)
    st_s = metrics.colour_stats(d["img_s"], d["labels_s"], R)
    luts = metrics.colour_transfer_maps(st_c, st_s, "hist")
    assert luts.dtype == torch.uint8 and tuple(luts.shape) == (B, R, 3, 256)
    assert np.array_equal(luts.cpu().numpy(), c["luts"])
    pairs = [(n, (n + 1) % B) for n in range(B)] + [(B - 1, 0)]
    got = ops.hist_match_lut(st_c.hist, st_s.hist, pairs)
    assert np.array_equal(got.cpu().numpy(), T.luts_judge(c["hist"], c["hist_s"], pairs))
    own = ops.hist_match_lut(st_c.hist, st_c.hist, [(n, n) for n in range(B)]).cpu().numpy()      # matched to itself: present levels stay
    present = c["hist"][:, :, :3] > 0
    assert np.array_equal(own[present], np.broadcast_to(np.arange(256, dtype=np.uint8), own.shape)[present])
    assert tuple(ops.hist_match_lut(st_c.hist, st_s.hist, []).shape) == (0, R, 3, 256)
    with pytest.raises(ValueError, match="COLOUR_AXES"):
        metrics.colour_transfer_maps(metrics.colour_stats(d["img"], d["labels"], R, torch.tensor(C.SIGNED_DIRS, dtype=torch.int16)), st_s, "hist")


@pytest.mark.parametrize("name", T.NAMES)
def test_apply_against_the_judges(name):
    c = T.reference(name)
    d = _dev(c)
    img = c["img"].numpy()
    lab = None if c["labels"] is None else c["labels"].numpy()
    none = np.zeros(img.shape[:3], dtype=bool) if lab is None else lab >= c["R"]
    got = _apply(d, "lut-hard")
    assert got.dtype == torch.uint8 and tuple(got.shape) == tuple(img.shape) and got.is_contiguous()
    assert np.array_equal(got.cpu().numpy(), T.apply_lut(img, lab, c["luts"]).astype(np.uint8))            # integers: EQUAL
    print()
    for key in T.MODES:
        got = _apply(d, key).cpu().numpy()
        q64, tau = c["q64"][key], c["tau"][key]
        print("  %-13s %-18s tau needed %.3g  tau %.3g" % (name, key, G.min_tau(q64, got), tau))
        assert G.judge(q64, got, tau) == [], (name, key)
        assert np.array_equal(got[none], img[none])                                                         # no region: the input's bytes
    if CASE_HAS_IGNORE(name):
        assert none.any()
    if "window" in c:                                           # the crop view is read in place and gives the copy's bits
        y, x = c["window"]
        view, lview = c["big_img"].cuda()[:, y, x], c["big_labels"].cuda()[:, y, x]
        assert not view.is_contiguous() and view.stride(1) != 3 * view.shape[2] and view.stride(2) == 3
        for key in ALL_MODES:
            assert torch.equal(_apply(d, key, view, lview), _apply(d, key)), key


def CASE_HAS_IGNORE(name):
    return bool(T.CASES[name].get("ignore"))


@pytest.mark.parametrize("name", ["33x70", "257x130"])
def test_bit_equalities(name):
    """batch = single calls (in 257x130 the second image starts off a dword in the batch and on one alone), ``out=`` given =
    returned, repeat = repeat -- in all four kernel forms"""
    c = T.reference(name)
    d = _dev(c)
    for key in ("lut-hard", "lut-weighted", "mkl", "mkl-weighted"):
        first = _apply(d, key)
        assert torch.equal(first, _apply(d, key)), key
        for n in range(first.shape[0]):
            assert torch.equal(first[n:n + 1], _apply(d, key, sel=slice(n, n + 1))), (key, n)
        out = torch.full_like(first, 7)
        assert _apply(d, key, out=out) is out and torch.equal(out, first), key


def test_ops_refuse_wrong_arguments():
    """dtypes, shapes and the one-of-two rule are refused in Python, before the library is called"""
    from ppst_amd import metrics, ops
    d = _dev(T.reference("33x70"))
    img, lab, luts, rows, w = d["img"], d["labels"], d["luts"], d["rows_mkl"], d["weights"]
    with pytest.raises(ValueError, match="exactly one"):
        ops.colour_transfer_apply(img, lab)
    with pytest.raises(ValueError, match="exactly one"):
        ops.colour_transfer_apply(img, lab, luts=luts, affine=rows)
    for bad in (dict(luts=luts.float()), dict(luts=luts[:2]), dict(luts=luts[:, :, :2]), dict(affine=rows.double()), dict(affine=rows[..., :9]),
                dict(affine=rows.cpu()), dict(luts=luts, weights=w[:, :2]), dict(luts=luts, weights=w.double()), dict(luts=luts, weights=w.cpu()),
                dict(luts=luts, out=torch.empty(3, 33, 70, 4, dtype=torch.uint8, device="cuda")),
                dict(luts=luts, out=torch.empty(3, 33, 140, 3, dtype=torch.uint8, device="cuda")[:, :, ::2])):
        with pytest.raises(RuntimeError):
            ops.colour_transfer_apply(img, lab, **bad)
    for bad_img, bad_lab in ((img.float(), lab), (img[..., :2], lab), (img, lab.long()), (img, lab[:, :32])):
        with pytest.raises(RuntimeError):
            ops.colour_transfer_apply(bad_img, bad_lab, luts=luts)
    st = metrics.colour_stats(img, lab, 3)
    for a, b in ((st.hist.float(), st.hist), (st.hist, st.hist[:, :2]), (st.hist[:, :, :2], st.hist[:, :, :2]), (st.hist, st.hist.cpu())):
        with pytest.raises(RuntimeError):
            ops.hist_match_lut(a, b, [(0, 0)])
    for pairs in ([(0, 3)], [(3, 0)], [(-1, 0)]):
        with pytest.raises(ValueError, match="outside"):
            ops.hist_match_lut(st.hist, st.hist, pairs)
    with pytest.raises(ValueError, match="regions"):
        metrics.colour_transfer(img, st, lab, "hist", regions=2)


def test_maps_are_their_steps_by_hand():
    """``colour_transfer_maps`` for the Gaussian methods is ``gaussian_transfer_rows`` of the device's moments, rounded to fp32; it
    differs from the judges' rows (of the judges' moments) by the moments' fp32 error only (printed)"""
    from ppst_amd import metrics
    c = T.reference("33x70")
    d = _dev(c)
    R = c["R"]
    st_c, st_s = metrics.colour_stats(d["img"], d["labels"], R), metrics.colour_stats(d["img_s"], d["labels_s"], R)
    print()
    for method in ("mkl", "reinhard"):
        rows = metrics.colour_transfer_maps(st_c, st_s, method)
        assert rows.dtype == torch.float32 and tuple(rows.shape) == (3, R, 12) and rows.is_cuda
        hand = metrics.gaussian_transfer_rows(st_c.lab_mean, st_c.lab_cov, st_c.count, st_s.lab_mean, st_s.lab_cov, st_s.count, method)
        assert torch.equal(rows.cpu(), hand.float())
        print("  %-9s max |row - judge's row| %.3g" % (method, np.abs(rows.cpu().numpy() - c["rows_" + method]).max()))
        pairs = [(2, 0), (0, 0)]
        some = metrics.colour_transfer_maps(st_c, st_s, method, pairs)
        assert torch.equal(some[1], rows[0]) and tuple(some.shape) == (2, R, 12)


def test_baseline_swap_is_its_steps_by_hand():
    from ppst_amd import evaluation as EV
    from ppst_amd import glue, metrics, ops
    c = T.reference("33x70")
    d = _dev(c)
    R = c["R"]
    u8, lab, u8s, labs = d["img"], d["labels"], d["img_s"], d["labels_s"]
    st_c, st_s = metrics.colour_stats(u8, lab, R), metrics.colour_stats(u8s, labs, R)
    to_float = lambda o: ((o.permute(0, 3, 1, 2).float() + 0.5) / 127.5 - 1.0).clamp(max=1.0)
    for method in metrics.TRANSFER_METHODS:
        maps = metrics.colour_transfer_maps(st_c, st_s, method)
        hand = ops.colour_transfer_apply(u8, lab, **{"luts" if method == "hist" else "affine": maps})
        got = EV.baseline_swap(u8, u8s, lab, labs, method=method)
        assert got.dtype == torch.float32 and tuple(got.shape) == (3, 3, 33, 70) and float(got.abs().max()) <= 1.0
        assert torch.equal(got, to_float(hand)) and torch.equal(glue.tensor2im(got), hand), method
        assert torch.equal(metrics.colour_transfer(u8, st_s, lab, method, R), hand)
        assert not torch.equal(hand, u8)
        # fp32 images in [-1, 1] and one-hot masks go through the same quantisation
        assert torch.equal(EV.baseline_swap(to_float(u8), to_float(u8s), glue.one_hot_mask(lab.long(), R), labs.long(), method=method), got)
    whole = EV.baseline_swap(u8, u8s)                            # without labels: one region
    assert torch.equal(glue.tensor2im(whole), ops.colour_transfer_apply(u8, None, luts=metrics.colour_transfer_maps(
        metrics.colour_stats(u8), metrics.colour_stats(u8s), "hist")))
    # feather: one label matte per region as the weights
    w = torch.stack([ops.label_matte(lab, keep=(r,), feather=6, grow=3) for r in range(R)], 1)
    hand = ops.colour_transfer_apply(u8, lab, luts=metrics.colour_transfer_maps(st_c, st_s, "hist"), weights=w)
    assert torch.equal(EV.baseline_swap(u8, u8s, lab, labs, feather=6), to_float(hand))
    assert not torch.equal(hand, ops.colour_transfer_apply(u8, lab, luts=metrics.colour_transfer_maps(st_c, st_s, "hist")))
    # smooth: the guided filter of decode(target=...), the content as guide
    plain = ops.colour_transfer_apply(u8, lab, luts=metrics.colour_transfer_maps(st_c, st_s, "hist"))
    assert torch.equal(EV.baseline_swap(u8, u8s, lab, labs, smooth=True, gf_radius=8), ops.guided_filter(u8, plain, 8, (0.02 * 255) ** 2))


def test_baseline_grid_goes_through_the_metrics():
    """every pair of the grid is ``baseline_swap`` of that pair; ``style_fidelity`` and ``content_preservation`` take the dict as
    it is; on the pairs n -> n the device's W1 of the matched image is the judges', and it is below the unmatched content's
    wherever the judges' own numbers show that"""
    from ppst_amd import evaluation as EV
    c = T.reference("33x70")
    d = _dev(c)
    R = c["R"]
    u8, lab, u8s, labs = d["img"], d["labels"], d["img_s"], d["labels_s"]
    grid = EV.baseline_grid(u8, u8s, lab, labs)
    assert sorted(grid) == [(i, j) for i in range(3) for j in range(3)] and all(tuple(v.shape) == (3, 33, 70) for v in grid.values())
    for (i, j) in ((0, 0), (1, 2), (2, 1)):
        assert torch.equal(grid[(i, j)], EV.baseline_swap(u8[i:i + 1], u8s[j:j + 1], lab[i:i + 1], labs[j:j + 1])[0]), (i, j)
    assert EV.baseline_grid(u8, u8s, lab, labs, pairs=[]) == {} and sorted(EV.baseline_grid(u8, u8s, pairs=[(2, 0)])) == [(2, 0)]
    fid = EV.style_fidelity(u8s, grid, labs, lab)
    keep = EV.content_preservation((u8.permute(0, 3, 1, 2).float() + 0.5) / 127.5 - 1.0, grid)
    ident = EV.style_fidelity(u8s, u8, labs, lab)["w1_rgb"]
    assert sorted(fid) == sorted(grid) == sorted(keep) and all(0.0 < keep[k] <= 1.0 for k in keep)
    img, labn = c["img"].numpy(), c["labels"].numpy()
    matched = T.apply_lut(img, labn, c["luts"]).astype(np.uint8)
    axes = np.array(C.AXES, dtype=np.int16)
    hm, cm = C.hist_judge(matched, labn, R, axes)
    w1 = lambda ha, na, hb, nb: np.mean([C.w1_numerator(ha[p], hb[p]) / (na * nb) for p in range(3)])
    print()
    for n in range(3):
        for r in range(R):
            after = w1(c["hist_s"][n, r], c["count_s"][n, r], hm[n, r], cm[n, r])
            before = w1(c["hist_s"][n, r], c["count_s"][n, r], c["hist"][n, r], c["count"][n, r])
            print("  pair %d region %d  w1_rgb content %.3f  matched %.3f" % (n, r, before, after))
            assert abs(fid[(n, n)]["w1_rgb"][r] - after) <= 1e-12 * max(after, 1.0)
            assert abs(float(ident[n, r]) - before) <= 1e-12 * max(before, 1.0)
            if after < before:
                assert fid[(n, n)]["w1_rgb"][r] < float(ident[n, r])


def test_held_out_evaluator_reports_the_baseline():
    """a seeded model at 512^2 (the smallest size simple_swap takes), two images: ``set_baseline("hist")`` adds the four numbers
    (and their per-region forms) and changes none of the others; they are the by-hand composition; without it none is reported"""
    from ppst_amd import evaluation as EV
    from ppst_amd import weights as W
    from ppst_amd.ppst_model import create_model
    from ppst_amd.training import HeldOutEvaluator
    m = create_model(state_dict=W.make_state_dict(2, with_D=False, with_nce=False, bias_std=0.1), device="cuda")
    m.noise = None
    x = W.synthetic_images(31, 2, size=512).cuda()
    g = torch.Generator().manual_seed(7)
    labels = torch.randint(0, 3, (2, 32, 32), generator=g).repeat_interleave(16, 1).repeat_interleave(16, 2).cuda()
    plain = HeldOutEvaluator(x, swaps=True, labels=labels).evaluate_swaps(m)
    res = HeldOutEvaluator(x, swaps=True, labels=labels).set_baseline("hist").evaluate_swaps(m)
    four = ["baseline_content_ssim", "baseline_style_w1", "baseline_style_swd", "baseline_style_delta_e"]
    new = four + ["%s_r%d" % (k, r) for k in four[1:] for r in range(3)]
    assert not any(k.startswith("baseline") for k in plain)
    assert sorted(res) == sorted(list(plain) + new) and all(res[k] == plain[k] for k in plain)
    assert all(np.isfinite(res[k]) and res[k] >= 0.0 for k in new)
    base = EV.baseline_swap(x, x[[1, 0]], labels, labels[[1, 0]], method="hist")
    assert res["baseline_content_ssim"] == float(EV.content_preservation(x, base).double().mean().item())
    fid = EV.style_fidelity(x[[1, 0]], base, labels[[1, 0]], labels)
    nanmean = lambda t: float(t[~t.isnan()].mean().item())
    for key, name in (("baseline_style_w1", "w1_rgb"), ("baseline_style_swd", "swd"), ("baseline_style_delta_e", "delta_e")):
        assert res[key] == nanmean(fid[name])
        for r in range(3):
            assert res["%s_r%d" % (key, r)] == nanmean(fid[name][:, r])
    no_labels = HeldOutEvaluator(x, swaps=True).set_baseline("reinhard").evaluate_swaps(m)
    assert sorted(k for k in no_labels if k.startswith("baseline")) == sorted(four)
    print("\n" + HeldOutEvaluator.format(0, res))
