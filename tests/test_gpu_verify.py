"""The VERIFY family on the device (sfm_verify_* and verify.verify_pairs): every output equal to the restatement tests/np_verify.py word
for word, floats as integer views with a NaN equal to a NaN; a tolerance only where the device result is set beside another algorithm's
(include/sfm_hip.h, "VERIFY"; docs/tracks.md §11)."""
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
import fuzz_verify as fz  # noqa: E402
import verify_cases as vc  # noqa: E402
from fuzz_verify import dev, first, flat_out, same  # noqa: E402

INT32_MAX = 2 ** 31 - 1
FUZZ_FLOOR = 4000               # a tenth of the cases the committed logs hold, rounded down to one figure (docs/tracks.md §11)
# tests/test_oracle_solvers.py sets the host five-point beside tests/np_solvers.py's independent one at 1e-9 (largest element of the
# difference to the closest model, sign-aligned, on exact projections); the device copy is held to the same bound on such data.
NP_SOLVER_TOL = 1e-9


@pytest.fixture(scope="module")
def planted():
    """Three planted pairs with their restated stages at a budget of 48, computed once."""
    cases = [vc.planted_pair(m, frac, seed) for m, frac, seed in ((60, 0.8, 0), (300, 0.5, 1), (700, 0.3, 2))]
    return [(c, nv.verify_pairs(c["store"], c["nq"], c["pairs"], c["img_off"], c["kp"], c["K"], 0.7, budget=48, seed=7, stages=True)) for c in cases]


def device_stage_inputs(case, st):
    return dict(surv=dev(st["surv"]), m=dev(st["m"]), pairs=dev(case["pairs"]), img_off=dev(case["img_off"]), xn=dev(st["xn"]))


# ---- survivors ------------------------------------------------------------------------------------------------------------------

def survivor_store(rng, n_pairs, cap, sizes):
    store = np.zeros((n_pairs, 2, cap, 2), np.int32)
    store[:, 0] = rng.integers(-1, max(sizes) + 2, (n_pairs, cap, 2))
    d1 = rng.choice([1.0, 2.0, 10.0, np.inf, np.nan, 0.0], (n_pairs, cap), p=[0.4, 0.3, 0.2, 0.04, 0.03, 0.03]).astype(np.float32)
    d0 = (d1 * rng.choice([0.25, 0.5, 0.75, 1.0], (n_pairs, cap))).astype(np.float32)                   # ties with 0.5 and 0.75 are exact
    store[:, 1] = np.stack([d0, d1], -1).view(np.int32)
    return store


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [1, 63, 64, 65, 257])
def test_survivors_at_every_capacity_and_query_count(hip, cap):
    from sfm_mvs_amd import verify
    rng = np.random.default_rng(cap)
    sizes = [cap, max(cap - 3, 1), cap + 4]                          # image 1 is smaller than nq: n_i < n_query
    img_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    for n_pairs in (0, 1, 3):
        for nq_of in (0, cap, cap + 5):
            for ratio in (0.5, 0.75):
                store = survivor_store(rng, n_pairs, cap, sizes)
                pairs = np.array([[0, 1], [1, 2], [2, 0]], np.int32)[:n_pairs]
                nq = np.full(n_pairs, nq_of, np.int32)
                want_s, want_m = nv.survivors(store, nq, pairs, img_off, ratio)
                surv, chk_s = flat_out(want_s.shape, torch.int32)
                m, chk_m = flat_out(want_m.shape, torch.int32)
                verify.survivors(dev(store), dev(nq), dev(pairs), dev(img_off), ratio, out=(surv, m))
                msg = first(same("surv", surv, want_s), same("m", m, want_m), chk_s(), chk_m())
                assert not msg, (n_pairs, nq_of, ratio, msg)
                if n_pairs == 3 and nq_of and cap >= 63:           # (the comparison was of survivors and of rejected queries)
                    assert want_m.max() > 0 and (want_m < min(nq_of, cap)).any()


@pytest.mark.gpu
def test_survivors_of_pairs_that_name_no_two_images(hip):
    from sfm_mvs_amd import verify
    rng = np.random.default_rng(5)
    cap, sizes = 70, [70, 70]
    img_off = np.array([0, 70, 140], np.int32)
    pairs = np.array([[0, 0], [1, 1], [-1, 0], [0, 2], [INT32_MAX, 1], [1, 0]], np.int32)
    store = survivor_store(rng, len(pairs), cap, sizes)
    nq = np.full(len(pairs), cap, np.int32)
    want_s, want_m = nv.survivors(store, nq, pairs, img_off, 0.75)
    assert want_m[:5].tolist() == [0] * 5 and want_m[5] > 0 and (want_s[:5] == -1).all()
    surv, m = verify.survivors(dev(store), dev(nq), dev(pairs), dev(img_off), 0.75)
    assert not first(same("surv", surv, want_s), same("m", m, want_m))


# ---- samples --------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("H", [1, 64, 65, 1024])
def test_samples_equal_the_restatement(hip, H):
    from sfm_mvs_amd import verify
    m = np.array([0, 4, 5, 6, 255, 256, 257], np.int32)
    want = nv.samples(m, H, 12345)
    out, chk = flat_out(want.shape, torch.int32)
    verify.samples(dev(m), H, 12345, out=out)
    assert not first(same("samp", out, want), chk())
    assert (want[:2] == -1).all() and (want[2:] >= 0).all()
    assert (np.sort(want[2], axis=1) == np.arange(5)).all()          # m = 5: every sample is the whole set


# ---- models ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_models_are_the_bits_of_the_host_five_point(hip, planted):
    from sfm_mvs_amd import verify
    total = 0
    for case, st in planted:
        d = device_stage_inputs(case, st)
        nm, chk_n = flat_out(st["nmodels"].shape, torch.int32)
        E, chk_E = flat_out(st["E_all"].shape, torch.float64)
        verify.models(dev(st["samp"]), d["surv"], d["m"], d["pairs"], d["img_off"], d["xn"], out=(nm, E))
        msg = first(same("nmodels", nm, st["nmodels"]), same("E", E, st["E_all"]), chk_n(), chk_E())
        assert not msg, msg
        total += int(st["nmodels"].sum())
    assert total > 100                                               # the comparison was not of empty lists


def degenerate_samples():
    """xn [40, 2] and five-tuples over it: five equal points, points on a line, a NaN coordinate, coordinates of 1e150."""
    rng = np.random.default_rng(11)
    xn = rng.normal(0, 0.3, (40, 2))
    xn[0:5] = xn[0]
    xn[5:10, 1] = 2 * xn[5:10, 0] + 0.25
    xn[25:30] = xn[5:10] * 0.5                                       # the second image's points of the collinear sample: on a line too
    xn[12, 0] = np.nan
    xn[17, 1] = 1e150
    surv = np.stack([np.arange(20), np.arange(20)], 1).astype(np.int32)[None]        # survivor e = (e, e): nodes e and 20 + e
    samp = np.array([[[0, 1, 2, 3, 4], [5, 6, 7, 8, 9], [10, 11, 12, 13, 14], [15, 16, 17, 18, 19], [0, 5, 10, 15, 19], [-1] * 5, [0, 1, 2, 3, 20]]], np.int32)
    return xn, surv, np.array([20], np.int32), samp, np.array([[0, 1]], np.int32), np.array([0, 20, 40], np.int32)


@pytest.mark.gpu
def test_models_of_degenerate_samples(hip):
    from sfm_mvs_amd import verify
    xn, surv, m, samp, pairs, img_off = degenerate_samples()
    want_n, want_E = nv.models(samp, surv, m, pairs, img_off, xn)
    print("models of the degenerate samples:", want_n.tolist())
    assert want_n[0, 5] == 0 and want_n[0, 6] == 0                  # an undrawn sample and a slot past m give no model
    nm, E = verify.models(dev(samp), dev(surv), dev(m), dev(pairs), dev(img_off), dev(xn))
    assert not first(same("nmodels", nm, want_n), same("E", E, want_E))


@pytest.mark.gpu
def test_models_beside_the_independent_numpy_solver(hip):
    import np_solvers
    from sfm_mvs_amd import verify
    case = vc.planted_pair(60, 1.0, 9, noise=0.0)                    # exact projections, as the host-solver test's (sigma = 0)
    st = nv.verify_pairs(case["store"], case["nq"], case["pairs"], case["img_off"], case["kp"], case["K"], 0.7, budget=16, seed=1, stages=True)
    d = device_stage_inputs(case, st)
    nm, E = verify.models(dev(st["samp"]), d["surv"], d["m"], d["pairs"], d["img_off"], d["xn"])
    nm, E = nm.cpu().numpy(), E.cpu().numpy()
    checked, worst = 0, 0.0
    for s in range(16):
        idx = st["samp"][0, s]
        q, t = st["surv"][0, idx, 0], st["surv"][0, idx, 1]
        ref = np.asarray(np_solvers.five_point(st["xn"][q], st["xn"][case["img_off"][1] + t])).reshape(-1, 9)
        for j in range(nm[0, s]):
            if not len(ref):
                continue
            err = min(min(np.abs(E[0, s, j] - r).max(), np.abs(E[0, s, j] + r).max()) for r in ref)
            worst = max(worst, err)
            checked += 1
    print(f"{checked} device models beside np_solvers.five_point: largest difference {worst:.3e}")
    assert checked > 10 and worst <= NP_SOLVER_TOL


# ---- score ----------------------------------------------------------------------------------------------------------------------

def score_both(case, st, E, nm, thr2, m=None):
    from sfm_mvs_amd import verify
    m = st["m"] if m is None else m
    want_c, want_b = nv.score(E, nm, st["surv"], m, case["pairs"], case["img_off"], st["xn"], thr2)
    d = device_stage_inputs(case, st)
    counts, chk = flat_out(want_c.shape, torch.int32)
    got_c, got_b = verify.score(dev(E), dev(nm), d["surv"], dev(m), d["pairs"], d["img_off"], d["xn"], thr2,
                                out=(counts, torch.empty(len(nm), dtype=torch.int64, device="cuda")))
    msg = first(same("counts", got_c, want_c), same("best", got_b.cpu().numpy().view(np.uint64), want_b), chk())
    assert not msg, msg
    return want_c, want_b


@pytest.mark.gpu
@pytest.mark.parametrize("m_cut", [0, 1, 255, 256, 257, 511, 513, None])
def test_score_on_both_sides_of_the_tile(hip, planted, m_cut):
    case, st = planted[2]                                            # 700 survivors
    m = st["m"] if m_cut is None else np.array([m_cut], np.int32)
    c, b = score_both(case, st, st["E_all"], st["nmodels"], float(st["thr2"]), m)
    if m_cut != 0:
        assert c.max() > 0 and b[0] >> np.uint64(32) == np.uint64(c.max())


@pytest.mark.gpu
def test_score_without_models_with_ties_and_at_the_threshold(hip, planted):
    case, st = planted[1]
    thr2 = float(st["thr2"])
    _, b = score_both(case, st, st["E_all"], np.zeros_like(st["nmodels"]), thr2)
    assert b[0] == 0
    # ties: the best model passed in under several (s, j): the smallest slot wins
    s0, j0 = divmod(int(nv.M32 - (int(st["best"][0]) & nv.M32)), nv.SLOTS)
    E, nm = st["E_all"].copy(), st["nmodels"].copy()
    for s, j in ((40, 3), (9, 2), (9, 1), (30, 0)):
        E[0, s, j] = st["E_all"][0, s0, j0]
        nm[0, s] = max(nm[0, s], j + 1)
    _, b = score_both(case, st, E, nm, thr2)
    assert int(nv.M32 - (int(b[0]) & nv.M32)) == min(nv.SLOTS * s0 + j0, 91)
    # a survivor whose error is exactly thr2: the threshold set to the float32 error of one survivor under the best model
    Em = st["E_all"][0, s0, j0]
    _, pts = nv._pair_points(st["surv"][0], int(st["m"][0]), 0, 1, case["img_off"].astype(np.int64), st["xn"])
    a1, b1, a2, b2 = pts.T
    e0, e1, e2 = Em[0] * a1 + Em[1] * b1 + Em[2], Em[3] * a1 + Em[4] * b1 + Em[5], Em[6] * a1 + Em[7] * b1 + Em[8]
    f0, f1 = Em[0] * a2 + Em[3] * b2 + Em[6], Em[1] * a2 + Em[4] * b2 + Em[7]
    sv = a2 * e0 + b2 * e1 + e2
    err = (sv * sv / (e0 * e0 + e1 * e1 + f0 * f0 + f1 * f1)).astype(np.float32)
    edge = float(np.sort(err)[len(err) // 2])
    c, _ = score_both(case, st, st["E_all"], st["nmodels"], edge)
    assert c[0, s0, j0] == int((err <= np.float32(edge)).sum()) and (err == np.float32(edge)).any()
    below = float(np.nextafter(np.float32(edge), np.float32(0)))
    c2, _ = score_both(case, st, st["E_all"], st["nmodels"], below)
    assert c2[0, s0, j0] < c[0, s0, j0]


# ---- select ---------------------------------------------------------------------------------------------------------------------

def select_both(case, st, best, thr2, vote_fn=nv.vote):
    from sfm_mvs_amd import verify
    want = nv.select(st["E_all"], st["nmodels"], best, st["surv"], st["m"], case["pairs"], case["img_off"], st["xn"], thr2, vote_fn=vote_fn)
    d = device_stage_inputs(case, st)
    n_pairs, cap = st["surv"].shape[:2]
    outs = [flat_out(s, t) for s, t in (((n_pairs, cap), torch.uint8), ((n_pairs, 9), torch.float64), ((n_pairs, 12), torch.float64), ((n_pairs, 8), torch.int32))]
    got = verify.select(dev(st["E_all"]), dev(st["nmodels"]), dev(best.view(np.int64)), d["surv"], d["m"], d["pairs"], d["img_off"], d["xn"], thr2,
                        out=tuple(o for o, _ in outs))
    msg = first(*[same(n, g, w) for n, g, w in zip(("keep", "E", "Rt", "info"), got, want)], *[c() for _, c in outs])
    assert not msg, msg
    return want


@pytest.mark.gpu
def test_select_equals_the_restatement(hip, planted):
    for case, st in planted:
        keep, E, Rt, info = select_both(case, st, st["best"], float(st["thr2"]))
        assert info[0, 7] == 0 and info[0, 3] == keep.sum() > 0 and info[0, 2] >= info[0, 3]
        R = Rt[0].reshape(3, 4)[:, :3]
        assert abs(np.linalg.det(R) - 1) < 1e-9 and abs(np.linalg.norm(Rt[0].reshape(3, 4)[:, 3]) - 1) < 1e-9
        none = select_both(case, st, np.zeros(1, np.uint64), float(st["thr2"]))
        assert none[3][0].tolist() == [int(st["m"][0]), int(st["nmodels"].sum()), 0, 0, -1, -1, -1, nv.NO_MODEL] and not none[0].any() and not none[1].any()


@pytest.mark.gpu
def test_select_when_no_candidate_gets_a_vote_and_when_two_tie(hip, planted):
    case, st = planted[0]
    # the winner's vote is 0: with thr2 = 0 the best model has no Sampson inlier, so no candidate gets a vote and candidate 0 wins
    want = select_both(case, st, st["best"], 0.0)
    assert want[3][0, 7] == nv.NO_VOTE and want[3][0, 6] == 0 and want[3][0, 2] == 0 and not want[0].any() and want[1].any() and want[2].any()
    # thr2 = inf: every survivor is a Sampson inlier, the wrong matches included, and the vote alone decides
    select_both(case, st, st["best"], float("inf"))
    # ties: with one, two and three survivors the four counts are small integers and several candidates share the largest
    tied = 0
    for mc in (0, 1, 2, 3):
        st1 = dict(st, m=np.array([mc], np.int32))
        tie = select_both(case, st1, st["best"], float("inf"))
        info = tie[3][0]
        pts = nv._pair_points(st["surv"][0], mc, 0, 1, case["img_off"].astype(np.int64), st["xn"])[1]
        cnt = nv.vote(np.stack([np.hstack([R, (sg * t)[:, None]]).reshape(12) for R, sg, t in _cands(st["E_all"][0, info[4], info[5]])]), pts).sum(1)
        tied += int((cnt == cnt.max()).sum() > 1)
        assert info[6] == int(np.argmax(cnt)) and info[3] == cnt.max() and info[7] & nv.FEW_SURVIVORS
    assert tied >= 1                                                 # (mc = 0: all four tie at 0 and candidate 0 wins)


def _cands(E):
    from sfm_mvs_amd import hostgeom
    R1, R2, t = hostgeom.decompose_essential(E)
    return (R1, 1.0, t), (R2, 1.0, t), (R1, -1.0, t), (R2, -1.0, t)


# ---- verify_pairs ---------------------------------------------------------------------------------------------------------------

def multi_pair_case():
    """Three planted pairs of different sizes and inlier shares in one store, with a pair i == j and a pair of four survivors."""
    parts = [vc.planted_pair(m, frac, seed) for m, frac, seed in ((300, 0.5, 3), (120, 0.8, 4), (4, 1.0, 5), (90, 0.8, 6))]
    cap = max(len(p["planted"]) for p in parts)
    store = np.zeros((len(parts), 2, cap, 2), np.int32)
    store[:, 1] = vc.dist_bits(4.0, 1.0)                             # the padding fails the ratio test
    kps, pairs, nq = [], [], []
    for k, p in enumerate(parts):
        m = len(p["planted"])
        store[k, :, :m] = p["store"][0]
        kps += p["kps"]
        pairs.append([2 * k, 2 * k + 1] if k != 3 else [6, 6])
        nq.append(m)
    sizes = [len(k) for k in kps]
    return dict(store=store, nq=np.array(nq, np.int32), pairs=np.array(pairs, np.int32), img_off=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32),
                kp=np.concatenate(kps), kps=kps, K=parts[0]["K"], planted=[p["planted"] for p in parts])


@pytest.mark.gpu
def test_verify_pairs_is_the_composition_twice_without_a_host_wait(hip):
    from sfm_mvs_amd import tracks, verify
    case = multi_pair_case()
    want = nv.verify_pairs(case["store"], case["nq"], case["pairs"], case["img_off"], case["kp"], case["K"], 0.7, budget=64, seed=3)
    args = (dev(case["store"]), dev(case["nq"]), dev(case["pairs"]), dev(case["img_off"]), dev(case["kp"]), case["K"], 0.7)
    verify.verify_pairs(*args, budget=64, seed=3)                    # allocations and module loading happen here
    torch.cuda.synchronize()
    from sfm_mvs_amd import _lib
    mode = torch.cuda.get_sync_debug_mode()
    waits = _lib.lib().sfm_host_sync_count()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = verify.verify_pairs(*args, budget=64, seed=3)
        again = verify.verify_pairs(*args, budget=64, seed=3, max_models_bytes=1)         # one pair a chunk
        pairs_of_three = verify.verify_pairs(*args, budget=64, seed=3, max_models_bytes=3 * 64 * 720)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert _lib.lib().sfm_host_sync_count() == waits                # the library itself did not wait either
    assert verify.pairs_per_chunk(64, 1) == 1 and verify.pairs_per_chunk(64, 3 * 64 * 720) == 3 and verify.pairs_per_chunk() == 364
    for name in ("keep", "E", "Rt", "info"):
        assert not same(name, pairs_of_three[name], want[name])
    for name in ("keep", "E", "Rt", "info"):
        assert not same(name, got[name], want[name]) and not same(name, again[name], want[name])
    info = want["info"]
    assert info[2, 7] == (nv.FEW_SURVIVORS | nv.NO_MODEL) and info[3, 0] == 0 and not want["keep"][2:].any() and want["keep"][0].any() and want["keep"][1].any()
    # match_edges takes the mask, and keeps exactly its queries
    edges = tracks.match_edges(args[0], args[1], args[2], args[3], 0.7, keep=got["keep"]).cpu().numpy().reshape(len(case["nq"]), -1, 2)
    assert ((edges[:, :, 0] >= 0) == (want["keep"] != 0)).all()
    other = verify.verify_pairs(*args, budget=64, seed=4)
    assert same("keep", other["keep"], want["keep"])                 # another seed draws other samples
    iters = verify.confidence_iters(got["info"])
    assert np.array_equal(iters, nv.confidence_iters(info)) and np.isinf(iters[2:]).all() and (iters[:2] > 0).all()


def per_pair_loop(store, n_query, pairs, keypoints, K, ratio=0.70):
    """tracks.verify_keep as it stood before `batched` was added."""
    from sfm_mvs_amd import ops, ransac
    dev_ = store.device
    n_pairs, cap = int(store.shape[0]), int(store.shape[2])
    keep = torch.zeros((n_pairs, cap), dtype=torch.uint8, device=dev_)
    for p, (i, j) in enumerate(pairs):
        nq = int(n_query[p])
        block = store[p]
        out_q, out_t, count = ops.ratio_compact(block[0, :nq], block[1, :nq].view(torch.float32), ratio)
        pts0, pts1 = ops.gather_matches(keypoints[i], keypoints[j], out_q, out_t, count)
        m = int(count.item())
        if m < 5:
            continue
        pts0, pts1 = pts0[:m], pts1[:m]
        E, mask = ransac.find_essential_mat(pts0, pts1, K, 0.999, 0.4, return_device_mask=True)
        if E is None:
            continue
        first_ = ops.mask_indices(mask).long()
        _, _, _, mask2 = ransac.recover_pose(E[:3], pts0[first_], pts1[first_], K, return_device_mask=True)
        second = ops.mask_indices(mask2, nonzero=True).long()
        keep[p].index_fill_(0, out_q[:m].long()[first_[second]], 1)
    return keep


@pytest.mark.gpu
def test_verify_keep_without_batched_is_unchanged_and_batched_is_verify_pairs(hip):
    from sfm_mvs_amd import tracks, verify
    case = multi_pair_case()
    store, kps = dev(case["store"]), [dev(k) for k in case["kps"]]
    pairs = [tuple(int(v) for v in p) for p in case["pairs"][:3]]    # (the per-pair path gathers from two different images)
    old = per_pair_loop(store[:3], case["nq"][:3], pairs, kps, case["K"])
    new = tracks.verify_keep(store[:3], case["nq"][:3], pairs, kps, case["K"])
    assert torch.equal(old, new) and int(new.sum()) > 0
    batched = tracks.verify_keep(store, case["nq"], case["pairs"], kps, case["K"], batched=True, budget=64, seed=3)
    direct = verify.verify_pairs(store, dev(case["nq"]), dev(case["pairs"]), dev(case["img_off"]), dev(case["kp"]), case["K"], 0.7, budget=64, seed=3)
    assert torch.equal(batched, direct["keep"])
    with pytest.raises(TypeError):
        tracks.verify_keep(store[:3], case["nq"][:3], pairs, kps, case["K"], budget=64)


@pytest.mark.gpu
@pytest.mark.parametrize("m", vc.SIZES)
def test_batched_beside_the_per_pair_path_on_the_planted_scenes(hip, m):
    """Recall of planted inliers and share of planted outliers kept, batched (default budget) beside the per-pair path, on every planted
    scene of the calibration: inlier shares 0.3, 0.5, 0.8 x m = 50, 500, 5 000 x seeds 0, 1, 2 (the seed draws the scene and the samples,
    as in the calibration).  Each scene is asserted.  The margins are the issue's two points and one point, widened to the seed-to-seed
    spread the CPU calibration records for (share, m) at the default budget where that is larger (tests/golden/verify_calibration.json;
    docs/tracks.md §11.4 holds the figures of every scene).  At 30 % inliers that spread is 7 to 39 points: there the test does not
    constrain the recall, it records it."""
    from sfm_mvs_amd import tracks, verify
    cal = vc.load_calibration()
    rows = []
    for frac in vc.FRACTIONS:
        spread = cal[(frac, m, verify.DEFAULT_BUDGET)]
        mr, mo = max(0.02, spread[2]), max(0.01, spread[3])
        for seed in (0, 1, 2):
            case = vc.planted_pair(m, frac, seed)
            store, kps = dev(case["store"]), [dev(k) for k in case["kps"]]
            b = vc.rates(tracks.verify_keep(store, case["nq"], case["pairs"], kps, case["K"], batched=True, seed=seed).cpu().numpy()[0], case["planted"])
            s = vc.rates(tracks.verify_keep(store, case["nq"], [(0, 1)], kps, case["K"]).cpu().numpy()[0], case["planted"])
            rows.append((frac, seed, b, s, mr, mo))
            print(f"inliers {frac} m {m} seed {seed}: batched recall {b[0]:.3f} outliers kept {b[1]:.4f}; per pair recall {s[0]:.3f} outliers kept {s[1]:.4f}; "
                  f"margins {mr:.3f} / {mo:.4f}")
        mean = lambda k, j: float(np.mean([r[k][j] for r in rows[-3:]]))  # noqa: E731
        print(f"inliers {frac} m {m} mean of the seeds: batched {mean(2, 0):.3f} / {mean(2, 1):.4f}; per pair {mean(3, 0):.3f} / {mean(3, 1):.4f}")
    bad = [(frac, seed, b, s) for frac, seed, b, s, mr, mo in rows if b[0] < s[0] - mr or b[1] > s[1] + mo]
    assert not bad, bad


# ---- fuzzing --------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_a_short_fixed_seed_fuzz_run(hip):
    counts, bad, dt = fz.run(4.0, 20260, log=print)
    print(f"fuzz_verify: {sum(counts.values())} cases {counts} in {dt:.1f} s")
    assert bad == 0 and sum(counts.values()) >= 3


@pytest.mark.gpu
def test_committed_fuzz_logs_are_clean_and_of_this_code(hip):
    """profiles/verify_fuzz_seed*.log: no mismatch, and run on the code of csrc/verify.hip and csrc/common.h that the loaded library
    was built from (scripts/knn_code_hash.py: comments and whitespace do not count)."""
    import glob
    import re
    from sfm_mvs_amd import _lib
    have = _lib.code_hashes_of_binary()
    logs = sorted(glob.glob(os.path.join(ROOT, "profiles", "verify_fuzz_seed*.log")))
    assert len(logs) >= 2, logs
    total = 0
    for path in logs:
        text = open(path).read()
        m = re.search(r"fuzz_verify: seed \d+, (\d+) cases .*?, (\d+) mismatches", text)
        assert m and int(m.group(2)) == 0, f"{path}: no clean summary line"
        ids = re.findall(r"sfm_build_id (knn\.hip:\S+(?: \S+:\S+)*)", text)
        assert ids, f"{path} does not name the build it ran on"
        logged = dict(tok.split(":", 1) for tok in ids[-1].split() if ":" in tok)
        for name in ("verify.hip", "common.h"):
            assert logged.get(name) == have[name], f"{path} was produced by another csrc/{name} than the loaded binary's"
        total += int(m.group(1))
    assert total >= FUZZ_FLOOR, total
