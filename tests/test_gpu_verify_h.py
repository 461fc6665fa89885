"""The VERIFY-H family on the device (sfm_verify_h_models / _score / _select and verify.verify_pairs(homography=...)): every output
equal to the restatement tests/np_verify_h.py word for word, floats as integer views with a NaN equal to a NaN, outputs in front of
sentinel words (include/sfm_hip.h, "VERIFY-H"; docs/tracks.md §13)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

import np_verify as nv  # noqa: E402
import np_verify_h as nh  # noqa: E402
import fuzz_verify_h as fz  # noqa: E402
import verify_cases as vc  # noqa: E402
import verify_h_cases as hc  # noqa: E402
from fuzz_verify import dev, first, flat_out, same  # noqa: E402
from fuzz_verify_h import as_i64  # noqa: E402

FUZZ_FLOOR = 4000               # a tenth of the cases the committed logs hold, rounded down to one figure (docs/tracks.md §13.6)


@functools.lru_cache(maxsize=None)
def inputs(kind="planar", m=513, frac=0.8, seed=1, H=24, sample_seed=7):
    """A planted pair with its restated survivors, samples and models: computed once, never changed (copy before editing)."""
    c = hc.planted_pair_h(kind, m, frac, seed)
    xn = nv.normalise(c["kp"], c["K"])
    surv, mm = nv.survivors(c["store"], c["nq"], c["pairs"], c["img_off"], 0.7)
    samp = nv.samples(mm, H, sample_seed)
    ok, Hm = nh.models(samp, surv, mm, c["pairs"], c["img_off"], xn)
    return dict(case=c, xn=xn, surv=surv, m=mm, samp=samp, ok=ok, Hm=Hm, thr2h=float(nv.thr2_of(c["K"], 1.2)))


def part_of(st, **over):
    return tuple(over.get(k, st[k] if k in st else st["case"][k]) for k in ("surv", "m", "pairs", "img_off", "xn"))


# ---- models -----------------------------------------------------------------------------------------------------------------------

def models_both(samp, part):
    from sfm_mvs_amd import verify
    want = nh.models(samp, *part)
    ok, chk_o = flat_out(want[0].shape, torch.int32)
    Hm, chk_H = flat_out(want[1].shape, torch.float64)
    verify.h_models(dev(samp), *(dev(t) for t in part), out=(ok, Hm))
    msg = first(same("ok", ok, want[0]), same("Hm", Hm, want[1]), chk_o(), chk_H())
    assert not msg, msg
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("H", [1, 64, 65, 1024])
def test_models_at_every_survivor_count_and_budget(hip, H):
    st = inputs(m=257)
    for m_cut in (0, 4, 5, 6, 255, 256, 257):
        m = np.array([m_cut], np.int32)
        ok, Hm = models_both(nv.samples(m, H, 11), part_of(st, m=m))
        assert (ok.sum() > 0) == (m_cut >= 5) and (Hm[ok == 0] == 0).all() and (Hm[ok != 0][:, 8] == 1).all()


@pytest.mark.gpu
def test_models_are_the_host_function_bit_for_bit_on_three_planted_pairs(hip):
    from sfm_mvs_amd import hostgeom
    for kind in hc.KINDS:
        st = inputs(kind, 300, 0.5, 2, 64, 5)
        ok, Hm = models_both(st["samp"], part_of(st))
        pts = nv._pair_points(st["surv"][0], int(st["m"][0]), 0, 1, st["case"]["img_off"].astype(np.int64), st["xn"])[1]
        assert ok.sum() >= 60
        for s in range(64):
            sel = pts[st["samp"][0, s, :4]]
            H = hostgeom.homography4(sel[:, :2], sel[:, 2:])
            assert (H is not None) == bool(ok[0, s]) and (H is None or np.array_equal(H.reshape(9).view(np.int64), Hm[0, s].view(np.int64))), (kind, s)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["one point", "an axis", "a line", "nan", "huge"])
def test_models_on_degenerate_coordinates(hip, name):
    st = inputs(H=64)
    xn = st["xn"].copy()
    if name == "one point":
        xn[:] = xn[0]
    if name == "an axis":
        xn[:513, 1] = 0.0                                            # image 0 on the line b = 0: three collinear points in every sample
    if name == "a line":
        xn[:, 1] = 2 * xn[:, 0] + 0.1
    if name == "nan":
        xn[::7] = np.nan
    if name == "huge":
        xn[::5] = 1e150
        xn[3::10, 0] = -1e150
    ok, Hm = models_both(st["samp"], part_of(st, xn=xn))
    assert np.isfinite(Hm).all()
    if name in ("one point", "an axis"):
        assert not ok.any()                                          # exactly zero pivots: no model
    if name == "nan":
        assert 0 < ok.sum() < ok.size


@pytest.mark.gpu
def test_models_with_bad_samples_nodes_and_images(hip):
    st = inputs(H=64)
    samp = st["samp"].copy()
    samp[0, 0] = -1                                                  # a sample that could not be drawn
    samp[0, 1, 2] = -1
    samp[0, 2, 0] = int(st["m"][0])                                  # a slot past m'
    samp[0, 3, 3] = 2 ** 31 - 1
    samp[0, 4, 4] = -1                                               # the fifth slot is not read
    ok, _ = models_both(samp, part_of(st))
    assert ok[0, :5].tolist() == [0, 0, 0, 0, 1]
    surv = st["surv"].copy()
    surv[0, samp[0, 5, 1]] = (5, 2 ** 31 - 1)                        # a node past the last
    surv[0, samp[0, 6, 0]] = (-1, -1)
    ok, _ = models_both(samp, part_of(st, surv=surv))
    assert ok[0, 5] == 0 and ok[0, 6] == 0
    for pair in ([0, 2], [-1, 1], [2 ** 31 - 1, 0]):
        ok, Hm = models_both(samp, part_of(st, pairs=np.array([pair], np.int32)))
        assert not ok.any() and not Hm.any()
    models_both(samp[:0], tuple(t[:0] if k < 3 else t for k, t in enumerate(part_of(st))))               # no pairs


# ---- score ------------------------------------------------------------------------------------------------------------------------

def score_both(Hm, ok, part, thr2h):
    from sfm_mvs_amd import verify
    want_c, want_b = nh.score(Hm, ok, *part, thr2h)
    counts, chk_c = flat_out(want_c.shape, torch.int32)
    best, chk_b = flat_out(want_b.shape, torch.int64)
    verify.h_score(dev(Hm), dev(ok), *(dev(t) for t in part), thr2h, out=(counts, best))
    msg = first(same("counts", counts, want_c), same("best", best.cpu().numpy().view(np.uint64), want_b), chk_c(), chk_b())
    assert not msg, msg
    return want_c, want_b


@pytest.mark.gpu
@pytest.mark.parametrize("m_cut", [0, 1, 255, 256, 257, 511, 512, 513])
def test_score_on_both_sides_of_the_tile(hip, m_cut):
    st = inputs()
    counts, best = score_both(st["Hm"], st["ok"], part_of(st, m=np.array([m_cut], np.int32)), st["thr2h"])
    assert counts.max() <= m_cut and (best[0] != 0) == bool(st["ok"].any())
    if m_cut == 513:
        assert counts.max() > 100 and int(best[0]) >> 32 == counts.max()


@pytest.mark.gpu
@pytest.mark.parametrize("H", [1, 255, 256, 257, 1024])
def test_score_at_every_budget_around_a_workgroup_of_samples(hip, H):
    st = inputs(m=120, H=H)
    score_both(st["Hm"], st["ok"], part_of(st), st["thr2h"])


@pytest.mark.gpu
def test_score_without_models_with_equal_counts_and_a_threshold_that_is_a_survivors_value(hip):
    st = inputs()
    counts, best = score_both(st["Hm"], np.zeros_like(st["ok"]), part_of(st), st["thr2h"])
    assert not counts.any() and best[0] == 0
    s_best = nv.M32 - (int(nh.score(st["Hm"], st["ok"], *part_of(st), st["thr2h"])[1][0]) & nv.M32)
    Hm, ok = np.repeat(st["Hm"][:, s_best:s_best + 1], 24, 1), np.ones_like(st["ok"])                     # one model under every sample
    ok[0, :3] = 0
    counts, best = score_both(np.ascontiguousarray(Hm), ok, part_of(st), st["thr2h"])
    assert nv.M32 - (int(best[0]) & nv.M32) == 3 and len(set(counts[0, 3:].tolist())) == 1              # the lowest sample with a model wins
    ok[0, 5] = -7                                                    # any non-zero word is a model
    score_both(np.ascontiguousarray(Hm), ok, part_of(st), st["thr2h"])
    pts = nv._pair_points(st["surv"][0], 513, 0, 1, st["case"]["img_off"].astype(np.int64), st["xn"])[1]
    w, d = nh.transfer_value(st["Hm"][0, s_best], pts)
    v = np.sort(d[w > 0])
    assert v[40] < v[41]
    n_at = score_both(st["Hm"], st["ok"], part_of(st), float(v[40]))[0][0, s_best]
    n_below = score_both(st["Hm"], st["ok"], part_of(st), float(np.nextafter(v[40], np.float32(0))))[0][0, s_best]
    assert n_at == 41 and n_below == 40                              # thr2h = one survivor's float32 value exactly: it is in
    for thr in (0.0, np.inf, -1.0):
        score_both(st["Hm"], st["ok"], part_of(st), thr)


@pytest.mark.gpu
def test_score_of_survivors_at_and_behind_the_plane_of_w_zero(hip):
    """H = (1, 0, 0; 0, 1, 0; -1, 0, 1): w = 1 - a1.  Four survivors whose transfer error is exactly 0 where w is not 0: w = 0.5, w = -1
    (behind: not an inlier), w = 0 (u = x / 0: not an inlier) and w = 1."""
    xn = np.array([[0.5, 0.25], [2.0, 1.0], [1.0, 3.0], [0.0, 0.0], [1.0, 0.5], [-2.0, -1.0], [7.0, 7.0], [0.0, 0.0]])
    surv = np.array([[[0, 0], [1, 1], [2, 2], [3, 3], [-1, -1]]], np.int32)
    part = (surv, np.array([4], np.int32), np.array([[0, 1]], np.int32), np.array([0, 4, 8], np.int32), xn)
    Hm = np.array([[[1.0, 0, 0, 0, 1, 0, -1, 0, 1]]])
    counts, best = score_both(Hm, np.ones((1, 1), np.int32), part, 0.0)
    cls = nh.transfer_class(Hm[0, 0], np.hstack([xn[:4], xn[4:]]), 0.0)[0]
    assert cls.tolist() == [1, -1, 0, 1] and counts[0, 0] == 2
    from sfm_mvs_amd import verify
    keep_h, H_out, sv, info = select_both(Hm, np.ones((1, 1), np.int32), best, part, 0.0, 1)
    assert keep_h[0].tolist() == [1, 0, 0, 1, 0] and info[0].tolist() == [4, 1, 2, 2, 0, -1, 0, verify.FEW_SURVIVORS]


# ---- select -----------------------------------------------------------------------------------------------------------------------

def select_both(Hm, ok, best, part, thr2h, refit, trace=None):
    from sfm_mvs_amd import verify
    want = nh.select(Hm, ok, best, *part, thr2h, refit, trace=trace)
    n_pairs, cap = part[0].shape[:2]
    outs = [flat_out(s, t) for s, t in (((n_pairs, cap), torch.uint8), ((n_pairs, 9), torch.float64), ((n_pairs, 3), torch.float64), ((n_pairs, 8), torch.int32))]
    got = verify.h_select(dev(Hm), dev(ok), dev(as_i64(best)), *(dev(t) for t in part), thr2h, refit, out=tuple(o for o, _ in outs))
    msg = first(*[same(n, g, w) for n, g, w in zip(("keep_h", "H", "h_sv", "h_info"), got, want)], *[c() for _, c in outs])
    assert not msg, msg
    return want


def best_of(st, thr2h, **over):
    return nh.score(st["Hm"], st["ok"], *part_of(st, **over), thr2h)[1]


@pytest.mark.gpu
def test_select_at_the_floor_of_the_refit(hip):
    """7, 8 and 9 inliers of the best sample: the refit runs from eight."""
    st = inputs()
    part = part_of(st)
    s = nv.M32 - (int(best_of(st, st["thr2h"])[0]) & nv.M32)
    pts = nv._pair_points(st["surv"][0], 513, 0, 1, st["case"]["img_off"].astype(np.int64), st["xn"])[1]
    w, d = nh.transfer_value(st["Hm"][0, s], pts)
    v = np.sort(d[w > 0])
    assert v[5] < v[6] < v[7] < v[8] < v[9]
    key = np.array([(7 << 32) | (nv.M32 - s)], np.uint64)            # select reads the sample of the key, not its count
    for n in (7, 8, 9):
        tr = []
        info = select_both(st["Hm"], st["ok"], key, part, float(v[n - 1]), 1, trace=tr)[3]
        assert info[0, 3] == n and len(tr) == (n >= 8) and info[0, 2] >= n and info[0, 4] == s


@pytest.mark.gpu
def test_select_where_the_refit_wins_loses_is_switched_off_and_goes_non_finite(hip):
    from sfm_mvs_amd import hostgeom
    st = inputs()
    part = part_of(st)
    won = set()
    for scale in (1.0, 0.05, 25.0):                                  # the default threshold, a twentieth and twenty-five times it
        thr2h = st["thr2h"] * scale
        best = best_of(st, thr2h)
        tr = []
        keep_h, H_out, sv, info = select_both(st["Hm"], st["ok"], best, part, thr2h, 1, trace=tr)
        assert len(tr) == 1 and info[0, 2] >= info[0, 3] >= 8 and keep_h.sum() == info[0, 2] and sv[0, 1] == 1.0
        won.add(int(info[0, 5]))
        if info[0, 5] == 0:                                          # the device's words are the host refit's on the restatement's M
            c = hostgeom.verify_h_refit(tr[0][1]).reshape(9)
            assert np.array_equal(c.view(np.int64), tr[0][2].view(np.int64))
            Hn = hostgeom.verify_h_normalise(c)[0].reshape(9)
            assert np.array_equal(np.abs(Hn).view(np.int64), np.abs(H_out[0]).view(np.int64))
        off = select_both(st["Hm"], st["ok"], best, part, thr2h, 0)
        assert off[3][0, 5] == -1 and off[3][0, 2] == off[3][0, 3] == info[0, 3]
    assert won == {0, -1}, won
    # every survivor with w > 0 an inlier (thr2h = inf), on huge coordinates of both signs: the sums are not finite, the refit is dropped
    xn = st["xn"].copy()
    xn[::5] = 1e150
    xn[3::10, 0] = -1e150
    over = dict(xn=xn)
    tr = []
    info = select_both(st["Hm"], st["ok"], best_of(st, np.inf, **over), part_of(st, **over), np.inf, 1, trace=tr)[3]
    assert len(tr) == 1 and not np.isfinite(tr[0][1]).all() and not np.isfinite(tr[0][2]).all() and info[0, 5] == -1
    # every survivor an inlier on the scene's own coordinates
    tr = []
    keep_h, _, _, info = select_both(st["Hm"], st["ok"], best_of(st, np.inf), part, np.inf, 1, trace=tr)
    assert info[0, 3] == 513 and keep_h.sum() == 513 and len(tr) == 1


@pytest.mark.gpu
def test_select_without_a_model_and_of_padded_keys(hip):
    from sfm_mvs_amd import verify
    st = inputs()
    part = part_of(st)
    for key in (0, (9 << 32) | (nv.M32 - 24), (9 << 32) | (nv.M32 - 1000), 5):                          # best = 0, a sample that is >= H
        keep_h, H_out, sv, info = select_both(st["Hm"], st["ok"], np.array([key], np.uint64), part, st["thr2h"], 1)
        assert not keep_h.any() and not H_out.any() and not sv.any() and info[0].tolist() == [513, 0, 0, 0, -1, -1, 0, verify.NO_MODEL]
    few = part_of(st, m=np.array([4], np.int32))
    info = select_both(st["Hm"], st["ok"], np.zeros(1, np.uint64), few, st["thr2h"], 1)[3]
    assert info[0, 7] == verify.FEW_SURVIVORS | verify.NO_MODEL
    for pair in ([0, 2], [-1, 1]):                                   # an image out of range: no survivors, the model keeps its words
        info = select_both(st["Hm"], st["ok"], best_of(st, st["thr2h"]), part_of(st, pairs=np.array([pair], np.int32)), st["thr2h"], 1)[3]
        assert info[0, 2] == 0 and info[0, 4] >= 0
    surv = st["surv"].copy()
    surv[0, 5] = (2 ** 31 - 1, 3)
    surv[0, 300] = (-1, -1)
    surv[0, 301, 1] = 2 * 513                                        # past the last node
    select_both(st["Hm"], st["ok"], best_of(st, st["thr2h"], surv=surv), part_of(st, surv=surv), st["thr2h"], 1)
    empty = tuple(t[:0] if k < 3 else t for k, t in enumerate(part))
    select_both(st["Hm"][:0], st["ok"][:0], np.zeros(0, np.uint64), empty, st["thr2h"], 1)


# ---- verify_pairs -----------------------------------------------------------------------------------------------------------------

def multi_pair_case():
    from test_gpu_verify import multi_pair_case as base
    return base()


LO = dict(top=2, rounds=1, widen=(3.0,))
HS = dict(threshold=1.2, min_ratio=0.246, rot_spread=1.525, min_inliers=8, refit=1)
H_NAMES = ("keep_h", "H", "h_sv", "h_info", "config")


@pytest.mark.gpu
@pytest.mark.parametrize("lo", [None, LO])
def test_verify_pairs_with_homography_is_the_composition_twice_without_a_host_wait(hip, lo):
    from sfm_mvs_amd import _lib, tracks, verify
    case = multi_pair_case()
    want = nh.verify_pairs(case["store"], case["nq"], case["pairs"], case["img_off"], case["kp"], case["K"], 0.7, budget=64, seed=3,
                           lo=None if lo is None else (lo["top"], lo["widen"]), threshold_h=HS["threshold"], min_ratio=HS["min_ratio"],
                           rot_spread=HS["rot_spread"], min_inliers=HS["min_inliers"], refit=HS["refit"])
    args = (dev(case["store"]), dev(case["nq"]), dev(case["pairs"]), dev(case["img_off"]), dev(case["kp"]), case["K"], 0.7)
    kw = dict(budget=64, seed=3, lo=lo)
    without = verify.verify_pairs(*args, **kw)
    verify.verify_pairs(*args, homography=HS, **kw)                   # allocations and module loading happen here
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    waits = _lib.lib().sfm_host_sync_count()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = verify.verify_pairs(*args, homography=HS, **kw)
        again = verify.verify_pairs(*args, homography=HS, **kw)
        ones = verify.verify_pairs(*args, homography=HS, max_models_bytes=1, **kw)                     # one pair a chunk
        threes = verify.verify_pairs(*args, homography=HS, max_models_bytes=3 * 64 * 720, **kw)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert _lib.lib().sfm_host_sync_count() == waits
    names = ("keep", "E", "Rt", "info") + H_NAMES + (("lo_info",) if lo else ())
    assert sorted(got) == sorted(names)
    for name in names:
        for out in (got, again, ones, threes):
            msg = same(name, out[name], want[name])
            assert not msg, msg
        assert torch.equal(got[name].view(torch.uint8), again[name].view(torch.uint8))                   # a second run gives the same bits
    for name in without:                                             # keep, E, Rt, info (lo_info): the words they are without the argument
        assert torch.equal(got[name].view(torch.uint8), without[name].view(torch.uint8)), name
    assert got["config"].dtype == torch.int32 and want["h_info"][2].tolist() == [4, 0, 0, 0, -1, -1, 0, 3] and want["config"][2] == 0
    assert want["keep_h"][0].sum() == want["h_info"][0, 2] > 0
    kps = [dev(k) for k in case["kps"]]
    batched = tracks.verify_keep(args[0], case["nq"], case["pairs"], kps, case["K"], batched=True, budget=64, seed=3, lo=lo, homography=True)
    assert torch.equal(batched, without["keep"])                     # verify_keep forwards the argument and keeps returning keep alone
    assert verify.workspace_bytes(4, 300, 64, homography=HS) - verify.workspace_bytes(4, 300, 64) == 4 * (64 * 80 + 8)


@pytest.mark.gpu
def test_verify_pairs_without_homography_is_the_composition_of_todays_wrappers(hip):
    from sfm_mvs_amd import verify
    case = multi_pair_case()
    store, nq, pairs, img_off, kp = (dev(case[k]) for k in ("store", "nq", "pairs", "img_off", "kp"))
    got = verify.verify_pairs(store, nq, pairs, img_off, kp, case["K"], 0.7, budget=64, seed=3, homography=None)
    assert sorted(got) == ["E", "Rt", "info", "keep"]
    thr2 = verify.thr2_of(case["K"], 0.4)
    xn = verify.normalise_keypoints(kp, case["K"])
    surv, m = verify.survivors(store, nq, pairs, img_off, 0.7)
    part = (surv, m, pairs, img_off, xn)
    samp = verify.samples(m, 64, 3)
    nmodels, E = verify.models(samp, *part)
    counts, best = verify.score(E, nmodels, *part, thr2)
    want = verify.select(E, nmodels, best, *part, thr2)
    for name, w in zip(("keep", "E", "Rt", "info"), want):
        assert torch.equal(got[name].view(torch.uint8), w.view(torch.uint8)), name
    # and with the argument, the three new wrappers after them
    hs = verify.homography_settings(True)
    thr2h = verify.thr2_of(case["K"], hs["threshold"])
    ok, Hm = verify.h_models(samp, *part)
    h_counts, h_best = verify.h_score(Hm, ok, *part, thr2h)
    h_want = verify.h_select(Hm, ok, h_best, *part, thr2h, hs["refit"])
    full = verify.verify_pairs(store, nq, pairs, img_off, kp, case["K"], 0.7, budget=64, seed=3, homography=True)
    for name, w in zip(("keep_h", "H", "h_sv", "h_info"), h_want):
        assert torch.equal(full[name].view(torch.uint8), w.view(torch.uint8)), name
    assert torch.equal(full["config"], verify.pair_config(full["info"], full["h_info"], full["h_sv"], hs))


# ---- the planted scenes -----------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("kind", hc.KINDS)
def test_every_asserted_scene_gets_its_planted_configuration_on_the_device(hip, kind):
    """36 scenes: three kinds x shares 0.5, 0.8 x m 500, 5 000 x seeds 0..2 at the defaults; the nine scenes of m = 50 and seed 0 (never
    asserted for their word) equal the restatement word for word."""
    from sfm_mvs_amd import verify
    for frac in hc.ASSERTED_FRACTIONS:
        for m in hc.ASSERTED_SIZES:
            for seed in hc.SEEDS:
                case = hc.planted_pair_h(kind, m, frac, seed)
                out = verify.verify_pairs(dev(case["store"]), dev(case["nq"]), dev(case["pairs"]), dev(case["img_off"]), dev(case["kp"]), case["K"], 0.7,
                                          seed=seed, homography=True)
                n_E, n_H, sv = int(out["info"][0, 2]), int(out["h_info"][0, 2]), out["h_sv"][0].tolist()
                print(f"{kind} inliers {frac} m {m} seed {seed}: n_E {n_E} n_H {n_H} sv0 / sv2 {sv[0] / sv[2]:.3f} config {int(out['config'][0])}")
                assert int(out["config"][0]) == hc.PLANTED_CONFIG[kind], (kind, frac, m, seed)
    s = verify.DEFAULT_HOMOGRAPHY
    for frac in vc.FRACTIONS:
        case = hc.planted_pair_h(kind, 50, frac, 0)
        want = nh.verify_pairs(case["store"], case["nq"], case["pairs"], case["img_off"], case["kp"], case["K"], 0.7, threshold_h=s["threshold"],
                               min_ratio=s["min_ratio"], rot_spread=s["rot_spread"], min_inliers=s["min_inliers"], refit=s["refit"])
        got = verify.verify_pairs(dev(case["store"]), dev(case["nq"]), dev(case["pairs"]), dev(case["img_off"]), dev(case["kp"]), case["K"], 0.7, homography=True)
        msg = first(*[same(n, got[n], want[n]) for n in ("keep", "E", "Rt", "info") + H_NAMES])
        assert not msg, (frac, msg)


# ---- registration -----------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_register_tracks_skips_the_rotating_pair_that_shares_the_most_tracks(hip):
    from sfm_mvs_amd import register, verify
    from sfm_mvs_amd._lib import SfmHipError
    case = hc.ring_with_a_turned_camera()
    pairs = np.array(case["pairs"], np.int32)
    store, nq, kps = dev(case["store"]), dev(case["nq"]), [dev(k) for k in case["kps"]]
    out = verify.verify_pairs(store, nq, dev(pairs), dev(case["img_off"]), dev(case["kp"]), case["K"], 0.7, homography=True)
    config = out["config"].cpu().numpy()
    turned = case["pairs"].index((0, 8))
    assert config[turned] == verify.CONFIG_ROTATING and (config == verify.CONFIG_GENERAL).sum() >= 8, config.tolist()
    lines = []
    try:                                                             # today's order: the first candidate is the pair without a baseline
        register.register_tracks(store, case["nq"], case["pairs"], kps, case["K"], (968.0, 648.0), seed_tries=1, log=lines.append)
    except SfmHipError:
        pass
    assert lines and lines[0].startswith("register: seed (0, 8) shares"), lines[:1]
    res = register.register_tracks(store, case["nq"], case["pairs"], kps, case["K"], (968.0, 648.0), pair_config=config)
    assert res["seeds"][0]["config"] == verify.CONFIG_GENERAL and res["seeds"][0]["pair"] != (0, 8) and res["registered"].all()
    assert all(s["config"] in (verify.CONFIG_GENERAL, verify.CONFIG_PLANAR) for s in res["seeds"])


# ---- fuzzing ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_a_short_fixed_seed_fuzz_run(hip):
    counts, bad, dt = fz.run(4.0, 20262, log=print)
    print(f"fuzz_verify_h: {sum(counts.values())} cases {counts} in {dt:.1f} s")
    assert bad == 0 and sum(counts.values()) >= 3


@pytest.mark.gpu
def test_committed_fuzz_logs_are_clean_and_of_this_code(hip):
    """profiles/verify_h_fuzz_seed*.log: no mismatch, and run on the code of csrc/verify_h.hip and csrc/common.h that the loaded library
    was built from (scripts/knn_code_hash.py: comments and whitespace do not count)."""
    import glob
    import re
    from sfm_mvs_amd import _lib
    have = _lib.code_hashes_of_binary()
    logs = sorted(glob.glob(os.path.join(ROOT, "profiles", "verify_h_fuzz_seed*.log")))
    assert len(logs) >= 2, logs
    total = 0
    for path in logs:
        text = open(path).read()
        m = re.search(r"fuzz_verify_h: seed \d+, (\d+) cases .*?, (\d+) mismatches", text)
        assert m and int(m.group(2)) == 0, f"{path}: no clean summary line"
        ids = re.findall(r"sfm_build_id (knn\.hip:\S+(?: \S+:\S+)*)", text)
        assert ids, f"{path} does not name the build it ran on"
        logged = dict(tok.split(":", 1) for tok in ids[-1].split() if ":" in tok)
        for name in ("verify_h.hip", "common.h"):
            assert logged.get(name) == have[name], f"{path} was produced by another csrc/{name} than the loaded binary's"
        total += int(m.group(1))
    assert total >= FUZZ_FLOOR, total
