"""The MVS-PLAN family on the device (sfm_view_pair_counts / _depth_ranges / _select, mvs_plan.plan_views + host_plan, run_mvs's
neighbours / ranges keywords, tracks.densify_tracks) against the restatement tests/np_mvs_plan.py: every word exactly, float outputs as
integer views, repeated runs bit for bit, nothing written past a stated size (include/sfm_hip.h, "MVS-PLAN"; docs/mvs.md §8)."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

import fuzz_mvs_plan as fz  # noqa: E402
import mvs_plan_cases as mc  # noqa: E402
import np_mvs_plan as npl  # noqa: E402
from fuzz_tracks import dev  # noqa: E402
from test_mvs_plan_cpu import PLAN_BAR, RANGE_COVERAGE  # noqa: E402

INT32_MAX = 2 ** 31 - 1
LDS_CAMS = 96                   # SFM_PLAN_LDS_CAMS: the last ncam that counts in LDS
GROUP = 16                      # SFM_PLAN_GROUP
FUZZ_FLOOR = 400                # a tenth of the cases the committed logs hold, rounded down to one figure (docs/mvs.md §8.6)
WINDOW = (float(np.cos(np.deg2rad(60.0))), float(np.cos(np.deg2rad(1.0))))


def problem(seed, ncam, npt, lengths, deg=-1):
    return fz.make_problem(np.random.default_rng(seed), ncam, npt, lengths, deg)


@pytest.mark.gpu
@pytest.mark.parametrize("ncam", [1, 2, 3, 64, 65, LDS_CAMS, LDS_CAMS + 1])
def test_pair_counts_at_every_camera_and_track_count(hip, ncam):
    """Track counts around a workgroup's round (16 tracks) and its grid; lengths 2, 3 and ncam (65 and up: more than one tile of 64);
    both sides of the LDS switch-over."""
    for T in (0, 1, 2, 255, 256, 257):
        for length in sorted({min(2, ncam), min(3, ncam), ncam}):
            p = problem(1000 * ncam + 10 * T + length, ncam, T, np.full(T, length))
            msg, got, want = fz.check_pairs(p, *WINDOW)
            assert not msg, (ncam, T, length, msg)
            pairs = T * length * (length - 1) // 2
            assert int(got[0].sum()) == 2 * pairs and int(got[1].sum()) <= 2 * pairs


@pytest.mark.gpu
@pytest.mark.parametrize("ncam", [20, LDS_CAMS + 4])
def test_pair_counts_edge_inputs(hip, ncam):
    """A track one longer than the lane group; cam_idx from {-1, ncam, INT32_MAX}; NaN and infinite points; track_off rows outside 0..nobs;
    identical camera centres; a camera named twice by a track: on the LDS path and on the global one."""
    p = problem(3, ncam, 40, np.full(40, GROUP + 1))
    msg, got, _ = fz.check_pairs(p, *WINDOW)
    assert not msg, msg
    assert int(got[0].sum()) == 40 * (GROUP + 1) * GROUP
    for deg in (0, 1, 2, 3, 4, 7):
        for seed in (1, 2):
            p = problem(100 * seed + deg, ncam, 80, np.random.default_rng(seed).integers(2, min(ncam, 24) + 1, 80), deg)
            msg, got, want = fz.check_pairs(p, *WINDOW)
            assert not msg, (deg, seed, msg)
            if seed == 1:
                msg, _, _ = fz.check_pairs(p, -1.0, 1.0)
                assert not msg, (deg, seed, msg)
    # the out-of-range cameras, each by name: their pairs are missing from shared
    p = problem(5, ncam, 30, np.full(30, 4))
    p["cam_idx"][[0, 5, 10]] = [-1, ncam, INT32_MAX]
    msg, got, _ = fz.check_pairs(p, *WINDOW)
    assert not msg, msg
    assert int(got[0].sum()) == 2 * (30 * 6 - 3 * 3)
    # identical centres: every ray pair of two such cameras has c = 1 (or its neighbour): inside [-1, 1] or not, as the restatement says
    p = problem(6, ncam, 50, np.full(50, 5))
    p["P"][:] = p["P"][0]
    for win in ((-1.0, 1.0), (0.0, np.nextafter(1.0, 0.0)), WINDOW):
        msg, _, _ = fz.check_pairs(p, *win)
        assert not msg, (win, msg)


def ranges_problem(counts, seed=0, quantum=None):
    """Camera 2k observes counts[k] points of its own, the odd cameras none."""
    rng = np.random.default_rng(seed)
    ncam, nobs = 2 * len(counts), int(np.sum(counts))
    p = fz.make_problem(rng, ncam, nobs, np.ones(nobs, np.int64))
    p["cam_idx"] = np.repeat(2 * np.arange(len(counts)), counts).astype(np.int32)
    if quantum:
        p["X"] = np.round(p["X"] / quantum) * quantum
    p["cam_off"], p["cam_obs"] = npl.csr(p["cam_idx"], ncam)
    return p


@pytest.mark.gpu
def test_depth_ranges_at_every_count(hip):
    counts = [0, 1, 2, 7, 8, 255, 256, 257, 513]
    p = ranges_problem(counts)
    for lo, hi in ((20, 980), (0, 1000), (500, 500), (0, 0), (1000, 1000), (333, 667)):
        msg, got, want = fz.check_ranges(p, lo, hi)
        assert not msg, (lo, hi, msg)
        assert got[0][::2].tolist() == counts and not got[0][1::2].any()
    p = ranges_problem([1500], seed=2)                                          # all observations in one camera of two
    msg, got, _ = fz.check_ranges(p, 20, 980)
    assert not msg and got[0].tolist() == [1500, 0], msg


@pytest.mark.gpu
def test_depth_ranges_ties_last_bits_and_invalid_depths(hip):
    """The third row of P is (0, 0, 1, 0): the depth is the point's z.  Depths one float32 apart, runs of equal depths across the chosen
    ranks, denormals, +inf, NaN, zero and negative depths in between."""
    rng = np.random.default_rng(9)
    base = np.float32(3.0)
    near = base + np.arange(40, dtype=np.float32) * np.spacing(base)             # 40 neighbours in float32
    runs = np.repeat(np.array([1.5, 2.5, 2.5000002, 7.0], np.float32), [30, 50, 50, 30])
    junk = np.array([0.0, -0.0, -1.0, np.inf, -np.inf, np.nan, 1e-40, 1e-45, 3e-39, 1e39, -1e-40] * 6)
    for z in (near, runs, np.concatenate([near, junk, runs]), junk):
        z = rng.permutation(np.asarray(z, np.float64))
        n = len(z)
        p = ranges_problem([n])
        p["X"] = np.stack([rng.normal(size=n), rng.normal(size=n), z], 1)
        p["P"][:] = 0.0
        p["P"][:, 2, 2] = 1.0
        zf = z.astype(np.float32)
        valid = np.sort(zf[np.isfinite(zf) & (zf > 0)])
        for lo, hi in ((20, 980), (0, 1000), (500, 500), (250, 750), (310, 690)):
            msg, got, want = fz.check_ranges(p, lo, hi)
            assert not msg, (lo, hi, msg)
            m = len(valid)
            assert got[0][0] == m
            assert got[1][0] == valid[lo * (m - 1) // 1000].view(np.int32) and got[2][0] == valid[(hi * (m - 1) + 999) // 1000].view(np.int32)


@pytest.mark.gpu
def test_depth_ranges_with_a_corrupt_camera_list(hip):
    for seed in (1, 2, 3):
        for deg in (3, 5, 8, 6):
            p = problem(50 * seed + deg, 9, 400, np.random.default_rng(seed).integers(1, 7, 400), deg)
            msg, _, _ = fz.check_ranges(p, 20, 980)
            assert not msg, (seed, deg, msg)
    p = problem(8, 4, 60, np.full(60, 3))
    row = int(np.searchsorted(p["cam_off"], 90, side="right")) - 1                # the camera whose list holds entry 90
    other = int(np.flatnonzero(p["cam_idx"] != row)[0])                          # an observation of another camera
    p["cam_obs"][[3, 30, 60, 90]] = [-1, len(p["cam_idx"]), INT32_MAX, other]
    msg, got, want = fz.check_ranges(p, 0, 1000)
    assert not msg, msg
    assert int(got[0].sum()) == len(p["cam_idx"]) - 4


@pytest.mark.gpu
@pytest.mark.parametrize("nsrc", range(1, 9))
def test_select_with_ties_and_empty_rows(hip, nsrc):
    rng = np.random.default_rng(nsrc)
    for n in (1, 2, 5, 70, 130):                                                # more candidates than a wave has lanes
        shared = rng.integers(0, 4, (n, n)).astype(np.int32)
        good = np.minimum(shared, rng.integers(0, 4, (n, n))).astype(np.int32)   # many exact ties on good, broken by shared, then by index
        good[::3] = 0                                                           # rows that are all zero
        for min_good in (0, 1, 3, 4):
            msg = fz.check_select(shared, good, nsrc, min_good)
            assert not msg, (n, min_good, msg)
    good = np.full((9, 9), 2, np.int32)
    shared = np.full((9, 9), 5, np.int32)                                       # every key ties: ascending index, the view itself left out
    from sfm_mvs_amd import mvs_plan
    nbr, cnt = mvs_plan.select(dev(shared), dev(good), nsrc, 1)
    want = [[j for j in range(9) if j != i][:nsrc] for i in range(9)]
    assert nbr.cpu().numpy().tolist() == want and cnt.cpu().numpy().tolist() == [min(nsrc, 8)] * 9


@pytest.mark.gpu
def test_select_at_4096_views(hip):
    """A sparse matrix built on the device: view i shares points with i + d for d in 1, 2, 3, 5, 8 (and so with i - d), with counts that
    tie across d."""
    from sfm_mvs_amd import mvs_plan
    n, nsrc = 4096, 6
    good = torch.zeros((n, n), dtype=torch.int32, device="cuda")
    shared = torch.zeros((n, n), dtype=torch.int32, device="cuda")
    i = torch.arange(n, device="cuda")
    value = {1: (9, 20), 2: (9, 20), 3: (9, 25), 5: (4, 30), 8: (0, 50)}        # d -> (good, shared)
    for d, (g, s) in value.items():
        j = (i + d) % n
        good[i, j] = g; good[j, i] = g
        shared[i, j] = s; shared[j, i] = s
    nbr, cnt = mvs_plan.select(shared, good, nsrc, 1)
    nbr, cnt = nbr.cpu().numpy(), cnt.cpu().numpy()
    for row in (0, 1, 7, 2048, 4090, 4095):
        cand = sorted((-g, -s, (row + sign * d) % n) for d, (g, s) in value.items() for sign in (1, -1) if g >= 1)
        assert nbr[row].tolist() == [c[2] for c in cand][:nsrc], row
    assert np.all(cnt == nsrc) and np.all(nbr >= 0)
    # all rows at once: the first two are i +- 3 (good 9, shared 25), in ascending index order
    first = np.sort(nbr[:, :2], 1)
    want = np.sort(np.stack([(np.arange(n) + 3) % n, (np.arange(n) - 3) % n], 1), 1)
    assert np.array_equal(first, want)


@pytest.mark.gpu
def test_plan_views_never_waits_and_host_plan_waits_once(hip):
    from sfm_mvs_amd import _lib, mvs_plan
    P, X, cam_idx, pt_idx = mc.ring_tracks()
    p = dict(ncam=8, npt=len(X), P=P, X=X, cam_idx=cam_idx, pt_idx=pt_idx)
    p["track_off"], _ = npl.csr(pt_idx, len(X))
    p["cam_off"], p["cam_obs"] = npl.csr(cam_idx, 8)
    pl, Xd, Pd = fz.device_plan(p), dev(X), dev(P.reshape(8, 12))
    mvs_plan.host_plan(mvs_plan.plan_views(pl, Xd, Pd, 4, 1.0, 60.0, 8))        # warm
    torch.cuda.synchronize()
    lib0 = int(_lib.lib().sfm_host_sync_count())
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        planned = mvs_plan.plan_views(pl, Xd, Pd, 4, 1.0, 60.0, 8)
        torch.cuda.set_sync_debug_mode("warn")
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            hp = mvs_plan.host_plan(planned)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    syncs = [str(w.message) for w in caught if "synchroniz" in str(w.message).lower()]
    assert len(syncs) == 1, syncs
    assert int(_lib.lib().sfm_host_sync_count()) == lib0
    # the ring scene on the device: the restatement's plan, and what follows from the geometry
    want = npl.plan_views(cam_idx, pt_idx, X, P, 4, 1.0, 60.0, 8)
    assert hp["neighbours"] == want["neighbours"] and np.array_equal(hp["ranges"].view(np.int64), want["ranges"].view(np.int64))
    assert np.array_equal(hp["shared"], want["shared"]) and np.array_equal(hp["good"], want["good"])
    for i in range(8):
        assert set(hp["neighbours"][i][:2]) == {(i - 1) % 8, (i + 1) % 8}
    assert not fz.check_composed(p | dict(deg=-1), 4, (1.0, 60.0), 8, 2, 98)


def _scene5(ndepth=32):
    from mvs_scenes import render_scene, scene_cloud
    imgs, K, P, gt = render_scene(n=5, w=160, h=120, seed=0)
    return imgs, K, P, np.hstack([K.ravel()] + [q.ravel() for q in P]), scene_cloud(K, P, gt)


@pytest.mark.gpu
def test_run_mvs_keywords_at_the_sequence_defaults_change_no_bit(hip):
    from sfm_mvs_amd import mvs
    imgs, K, P, posearr, X = _scene5()
    n, nsrc = 5, 4
    base = mvs.run_mvs(imgs, K, posearr, X, ndepth=32, nsrc=nsrc)
    out = mvs.run_mvs(imgs, K, posearr, X, ndepth=32, nsrc=nsrc, neighbours=[mvs.neighbours(i, n, nsrc) for i in range(n)],
                      ranges=[mvs.depth_range(X, P[i], P_all=P) for i in range(n)])
    for a, b in zip(base["depths"], out["depths"]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert len(base["points"]) > 1000
    assert np.array_equal(base["points"], out["points"]) and np.array_equal(base["colors"], out["colors"])


@pytest.mark.gpu
def test_run_mvs_view_with_an_empty_list(hip):
    from sfm_mvs_amd import mvs
    imgs, K, P, posearr, X = _scene5()
    rng = [mvs.depth_range(X, P[i], P_all=P) for i in range(5)]
    full = mvs.run_mvs(imgs, K, posearr, X, ndepth=32, nsrc=2)
    out = mvs.run_mvs(imgs, K, posearr, X, ndepth=32, nsrc=2, neighbours=[[], [2, 3], [1, 3], [2, 1], []], ranges=rng)
    assert not out["depths"][0].any() and not out["depths"][4].any() and all(bool(out["depths"][i].any()) for i in (1, 2, 3))
    # views 0 and 4 contribute no point: the cloud is that of the three middle views run on their own
    sub = mvs.run_mvs(imgs[1:4], K, np.hstack([K.ravel()] + [q.ravel() for q in P[1:4]]), X, ndepth=32, nsrc=2, neighbours=[[1, 2], [0, 2], [1, 0]],
                      ranges=rng[1:4])
    assert len(out["points"]) > 1000 and np.array_equal(out["points"], sub["points"]) and np.array_equal(out["colors"], sub["colors"])
    assert torch.equal(out["depths"][2].view(torch.int32), full["depths"][2].view(torch.int32))          # view 2 keeps its sequence neighbours
    none = mvs.run_mvs(imgs, K, posearr, X, ndepth=32, neighbours=[[]] * 5, ranges=rng)
    assert none["points"].shape == (0, 3) and none["colors"].shape == (0, 3) and not any(bool(d.any()) for d in none["depths"])
    one = mvs.run_mvs(imgs, K, posearr, X, ndepth=32, neighbours=[[1], [0], [], [], []], ranges=rng, topk=2, min_consistent=2)   # the length caps both
    assert len(one["points"]) > 0


@pytest.mark.gpu
def test_densify_tracks_on_permuted_frames_end_to_end(hip):
    """The calibrated scene of docs/mvs.md §8.4 on the device: the planned run meets the thresholds of the 5-view end-to-end test at the
    arc's middle view, the sequence-neighbour run on the same frames does not and is worse by the calibrated margin; the planned ranges
    cover the ground truth."""
    from sfm_mvs_amd import mvs, tracks
    from test_mvs_cpu import MIN_VALID_FRACTION, MIN_WITHIN_1PCT, depth_accuracy
    imgs, K, P, gt, perm = mc.permuted_scene()
    X, cam_idx, pt_idx = mc.synth_tracks(K, P, gt)
    result = dict(points=X.astype(np.float32), cam_idx=cam_idx, pt_idx=pt_idx)
    out = tracks.densify_tracks(result, imgs, K, P, points=X, nsrc=mc.NSRC, ndepth=mc.NDEPTH)
    want = npl.plan_views(cam_idx, pt_idx, X, P, mc.NSRC)
    plan = out["plan"]
    assert plan["neighbours"] == want["neighbours"] and np.array_equal(plan["ranges"].view(np.int64), want["ranges"].view(np.int64))
    i = mc.MIDDLE
    depth = out["depths"][i].cpu().numpy()
    valid, within = depth_accuracy(depth, gt[i], 3)
    print(f"planned: valid {valid:.4f} within {within:.4f} wrong {mc.wrong_share(depth, gt[i]):.4f}, {len(out['points'])} points")
    assert valid >= MIN_VALID_FRACTION and within >= MIN_WITHIN_1PCT, (valid, within)
    posearr = np.hstack([K.ravel()] + [q.ravel() for q in P])
    seq = mvs.run_mvs(imgs, K, posearr, X, nsrc=mc.NSRC, ndepth=mc.NDEPTH)
    sdepth = seq["depths"][i].cpu().numpy()
    svalid, swithin = depth_accuracy(sdepth, gt[i], 3)
    print(f"sequence: valid {svalid:.4f} within {swithin:.4f} wrong {mc.wrong_share(sdepth, gt[i]):.4f}, {len(seq['points'])} points")
    assert not (svalid >= MIN_VALID_FRACTION and swithin >= MIN_WITHIN_1PCT), (svalid, swithin)
    assert mc.wrong_share(depth, gt[i]) <= PLAN_BAR * mc.wrong_share(sdepth, gt[i])
    cover = [mc.coverage(plan["ranges"][k], gt[k]) for k in range(len(P))]
    assert min(cover) >= RANGE_COVERAGE - (1.0 - RANGE_COVERAGE) / 2.0, cover
    assert len(out["points"]) > 5000 and np.all(np.isfinite(out["points"]))


@pytest.mark.gpu
def test_a_short_fixed_seed_fuzz_run_finds_no_mismatch(hip):
    counts, bad, dt = fz.run(10.0, 4242)
    print(f"fuzz_mvs_plan: seed 4242, {sum(counts.values())} cases {counts}, {bad} mismatches, {dt:.0f} s")
    assert bad == 0 and all(c > 0 for c in counts.values()), counts


@pytest.mark.gpu
def test_committed_fuzz_logs_are_clean_and_name_this_code(hip):
    """profiles/mvs_plan_fuzz_seed*.log: no mismatch, and run on the code of csrc/mvs_plan.hip and csrc/common.h that the loaded library
    was built from (scripts/knn_code_hash.py: comments and whitespace do not count)."""
    import glob
    import re
    from sfm_mvs_amd import _lib
    have = _lib.code_hashes_of_binary()
    logs = sorted(glob.glob(os.path.join(ROOT, "profiles", "mvs_plan_fuzz_seed*.log")))
    assert len(logs) >= 2, logs
    total = 0
    for path in logs:
        text = open(path).read()
        m = re.search(r"fuzz_mvs_plan: seed \d+, (\d+) cases .*?, (\d+) mismatches", text)
        assert m and int(m.group(2)) == 0, f"{path}: no clean summary line"
        ids = re.findall(r"sfm_build_id (knn\.hip:\S+(?: \S+:\S+)*)", text)
        assert ids, f"{path} does not name the build it ran on"
        logged = dict(tok.split(":", 1) for tok in ids[-1].split() if ":" in tok)
        for name in ("mvs_plan.hip", "common.h"):
            assert logged.get(name) == have[name], f"{path} was produced by another csrc/{name} than the loaded binary's"
        total += int(m.group(1))
    assert total >= FUZZ_FLOOR, total
