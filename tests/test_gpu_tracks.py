"""The TRACKS family on the device (sfm_match_edges, sfm_track_components, sfm_track_build, sfm_track_triangulate and tracks.run_tracks):
every output equal to the restatement tests/np_tracks.py, float rows as int32 views; there is no tolerance except where the device
result is set beside another algorithm's (include/sfm_hip.h, "TRACKS"; docs/tracks.md)."""
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

import np_tracks as nt  # noqa: E402
import fuzz_tracks as fz  # noqa: E402
from fuzz_tracks import dev, differ  # noqa: E402
from test_tracks_cpu import RING_BAR, hand_store, purity, ring_case, two_view  # noqa: E402

INT32_MAX = 2 ** 31 - 1
SIZES = (0, 1, 2, 3, 255, 256, 257, 65537)
FUZZ_FLOOR = 8000               # a tenth of the cases the committed logs hold, rounded down to one figure (docs/tracks.md §6)
# A 2-view track beside sfm_triangulate_dlt(rows = 4, normalise_w = 1), 3 000 points within the unit ball at 0.3 px noise: both solve
# the same 4 x 4 system, one by one-sided Jacobi on A and one by two-sided Jacobi on A^T A, which squares the condition number, so
# the float64 vectors agree to ~1e-8 only and a third of the float32 coordinates round to the neighbouring value.  Measured on that
# case: the largest difference of a coordinate is 1.192e-7 = 2^-23, one rounding step below 1 (docs/tracks.md section 4).  The bound is 4 x that.
TWO_VIEW_BOUND = 2.0 ** -21


def labels_of(edges, n, final, rounds=None):
    """Converged device labels of an edge list, checked state by state against `final`."""
    from sfm_mvs_amd import tracks
    labels, batches, lowered, msg = fz.converge(dev(np.asarray(edges, np.int32).reshape(-1, 2)), n, tracks.TRACK_ROUNDS if rounds is None else rounds, final)
    assert not msg, msg
    assert not differ("labels", labels, final)
    return labels, batches, lowered


@pytest.mark.gpu
@pytest.mark.parametrize("n_img", [1, 2, 3, 64, 65, 300])
def test_edge_soups_of_every_size(hip, n_img):
    rng = np.random.default_rng(1000 + n_img)
    for n in SIZES:
        img_off = fz.gen_offsets(rng, n_img, n)
        for ne in SIZES:
            e = rng.integers(0, max(n, 1), (ne, 2))
            bad = rng.random(e.shape) < 0.25                       # a quarter of the ends name no node
            e[bad] = rng.choice([-1, n, INT32_MAX], int(bad.sum()))
            final = nt.components(e, n)
            labels_of(e, n, final)
            msg = fz.check_build(img_off, final, 2, None)
            assert not msg, (n, ne, msg)


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["ascending", "descending", "permuted"])
def test_a_long_path_at_the_default_rounds_and_round_by_round(hip, order):
    n = 100000
    ids = {"ascending": np.arange(n), "descending": np.arange(n)[::-1], "permuted": np.random.default_rng(5).permutation(n)}[order]
    e = np.stack([ids[:-1], ids[1:]], 1)
    final = np.zeros(n, np.int32)
    _, batches, lowered = labels_of(e, n, final)
    _, single, lowered1 = labels_of(e, n, final, rounds=1)
    print(f"path of {n} nodes, {order} ids: {lowered} lowering rounds in {batches} batches at the default; {lowered1} single rounds")
    assert single == lowered1 + 1                                  # the last call is the round that lowers nothing


@pytest.mark.gpu
def test_a_hub_and_the_all_pairs_cliques(hip):
    n = 70002
    hub = 4711
    others = np.delete(np.arange(n), hub)
    e = np.stack([np.full(n - 1, hub), np.random.default_rng(2).permutation(others)], 1)
    labels_of(e, n, np.zeros(n, np.int32))
    # 20 000 tracks of 64 nodes, one per image, every one of the 2 016 pairs an edge: ordered pair by pair as a match store is
    rng = np.random.default_rng(3)
    n_tracks, n_img = 20000, 64
    nodes = np.stack([i * n_tracks + rng.permutation(n_tracks) for i in range(n_img)], 1).astype(np.int32)      # [track][image]
    iu, ju = np.triu_indices(n_img, 1)
    e = np.stack([nodes[:, iu].T.reshape(-1), nodes[:, ju].T.reshape(-1)], 1)
    assert e.shape == (2016 * n_tracks, 2)
    final = np.empty(n_tracks * n_img, np.int32)
    final[nodes.reshape(-1)] = np.repeat(nodes[:, 0], n_img)
    labels, batches, lowered = labels_of(e, n_tracks * n_img, final)
    print(f"20 000 cliques of 64: {lowered} lowering rounds in {batches} batches")
    img_off = (np.arange(n_img + 1) * n_tracks).astype(np.int32)
    want = nt.build(final, img_off)
    msg = fz.check_build(img_off, final, 2, None, want)
    assert not msg, msg
    assert want[3].tolist() == [n_tracks, n_tracks * n_img, n_tracks, 0, n_img, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("n_img", [64, 65])
def test_tracks_as_long_as_there_are_images(hip, n_img):
    rng = np.random.default_rng(n_img)
    per, n_tracks = 7, 5
    img_off = (np.arange(n_img + 1) * per).astype(np.int32)
    nodes = np.stack([i * per + rng.permutation(per)[:n_tracks] for i in range(n_img)], 1)
    e = np.vstack([np.stack([nodes[:, :-1].reshape(-1), nodes[:, 1:].reshape(-1)], 1), [[nodes[0, 3], nodes[1, 3] + 0]]])   # tracks 0 and 1 meet in image 3
    final = nt.components(e, per * n_img)
    labels_of(e, per * n_img, final)
    for lo, hi in ((2, None), (n_img, n_img), (n_img + 1, None), (2, n_img - 1)):
        msg = fz.check_build(img_off, final, lo, hi)
        assert not msg, (lo, hi, msg)
    counts = nt.build(final, img_off)[3].tolist()
    assert counts == [n_tracks - 2, (n_tracks - 2) * n_img, n_tracks - 1, 1, n_img, (per - n_tracks) * n_img]
    assert nt.build(final, img_off, n_img + 1)[3].tolist()[:2] == [0, 0]


@pytest.mark.gpu
def test_a_conflicting_giant_beside_clean_tracks(hip):
    rng = np.random.default_rng(6)
    n_img, n = 8, 6000
    img_off = fz.gen_offsets(rng, n_img, n)
    tracks_ = fz.planted_tracks(rng, img_off, 0.5)
    used = np.zeros(n, bool); used[[u for t in tracks_ for u in t]] = True
    giant = rng.permutation(np.flatnonzero(~used))[:2000]
    e = np.vstack([fz.track_edges(rng, tracks_, 2), np.stack([giant[:-1], giant[1:]], 1)])
    final = nt.components(e, n)
    labels_of(e[rng.permutation(len(e))], n, final)
    msg = fz.check_build(img_off, final, 2, None)
    assert not msg, msg
    counts = nt.build(final, img_off)[3].tolist()
    assert counts[:4] == [len(tracks_), sum(len(t) for t in tracks_), len(tracks_) + 1, 1]


@pytest.mark.gpu
def test_match_edges_on_hand_made_and_random_stores(hip):
    from sfm_mvs_amd import tracks
    store, nq, pair, off = hand_store()
    keep = np.array([[0, 1, 1, 1], [1, 1, 0, 1]], np.uint8)
    for ratio, k in ((0.5, None), (np.nextafter(0.5, 1.0), None), (0.5, keep), (0.7, keep * 255)):
        want = nt.match_edges(store, nq, pair, off, ratio, k)
        got = tracks.match_edges(dev(store), dev(nq), dev(pair), dev(off), ratio, None if k is None else dev(k))
        assert not differ("edges", got, want), (ratio, k)
    assert nt.match_edges(store, nq, pair, off, 0.5)[1].tolist() == [-1, -1]            # d0 == ratio * d1 exactly is no survivor
    for seed in range(40):
        msg = fz.fuzz_edges(np.random.default_rng(seed))
        assert not msg, (seed, msg)


def pinhole_tracks(kind):
    """Five 3-view tracks over three cameras, as sfm_track_build would leave them -> (img_off, kp, P, track_off, obs_node, counts)."""
    rng = np.random.default_rng(11)
    P = fz.random_cameras(rng, 3)
    if kind == "identical":
        P[:] = P[0]
    X = rng.normal(size=(5, 3)) * 0.4
    if kind == "behind":
        c = np.linalg.svd(P[1].reshape(3, 4))[2][-1]
        X[2] = 1.5 * c[:3] / c[3]                                    # beyond camera 1's centre, which looks at the origin
    img_off = np.array([0, 5, 10, 15], np.int32)
    h = np.einsum("kij,nj->kni", P.reshape(3, 3, 4), np.c_[X, np.ones(5)])
    kp = (h[..., :2] / h[..., 2:]).reshape(15, 2).astype(np.float32)
    if kind == "nan":
        kp[6, 0] = np.nan
    obs_node = np.array([[t, 5 + t, 10 + t] for t in range(5)], np.int32).reshape(-1)
    return img_off, kp, P, (3 * np.arange(6)).astype(np.int32), obs_node, np.array([5, 15, 0, 0, 0, 0], np.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["plain", "identical", "behind", "nan"])
def test_triangulation_degeneracies(hip, kind):
    case = pinhole_tracks(kind)
    msg = fz.check_tri(*case)
    assert not msg, msg
    X, err, depth, flags, worst = nt.triangulate(case[3], case[4], case[0], case[1], case[2])
    if kind == "plain":
        assert flags.tolist() == [3] * 5 and worst.max() < 0.05
    if kind == "behind":
        assert flags[2] & 1 == 0 and depth[3 * 2 + 1] < 0            # the point lies behind camera 1
        assert [f for k, f in enumerate(flags.tolist()) if k != 2] == [3] * 4
    if kind == "nan":
        assert flags[1] == 0 and np.isnan(worst[1]) and worst.view(np.uint32)[1] == 0x7FC00000 and np.isnan(X[1]).all()
        assert [f for k, f in enumerate(flags.tolist()) if k != 1] == [3] * 4
    for seed in range(30):
        g = fz.gen_tri(np.random.default_rng(seed))
        msg = fz.check_tri(*g[:6])
        assert not msg, (seed, g[6], msg)


@pytest.mark.gpu
def test_two_view_tracks_beside_the_pair_triangulation(hip):
    rng = np.random.default_rng(21)
    P = fz.random_cameras(rng, 2)
    n = 3000
    X = rng.normal(size=(n, 3)); X = X / np.maximum(np.linalg.norm(X, axis=1, keepdims=True), 1.0) * 0.9
    h = np.einsum("kij,nj->kni", P.reshape(2, 3, 4), np.c_[X, np.ones(n)])
    kp = (h[..., :2] / h[..., 2:] + rng.normal(0, 0.3, (2, n, 2))).reshape(2 * n, 2).astype(np.float32)
    img_off = np.array([0, n, 2 * n], np.int32)
    obs_node = np.stack([np.arange(n), n + np.arange(n)], 1).reshape(-1).astype(np.int32)
    track_off = (2 * np.arange(n + 1)).astype(np.int32)
    msg = fz.check_tri(img_off, kp, P, track_off, obs_node, np.array([n, 2 * n, 0, 0, 0, 0], np.int32))
    assert not msg, msg
    mine = nt.triangulate(track_off, obs_node, img_off, kp, P)[0]
    X4 = hip.triangulate(P[0].reshape(3, 4), P[1].reshape(3, 4), dev(kp[:n]).t(), dev(kp[n:]).t(), normalise_w=True).cpu().numpy()
    gap = float(np.abs(mine - X4[:3].T).max())
    print(f"2-view tracks beside sfm_triangulate_dlt(rows=4, normalise_w=1): largest coordinate difference {gap:.3e} (bound {TWO_VIEW_BOUND:.3e}), "
          f"{int((mine != X4[:3].T).sum())} of {3 * n} coordinates differ")
    assert np.abs(mine).max() < 1.0 and gap <= TWO_VIEW_BOUND


def ring_device():
    from sfm_mvs_amd import sharded
    case = ring_case()
    des = [torch.from_numpy(d).cuda() for d in case["des"]]
    store, nq = sharded.match_pairs_sharded(des, case["pairs"], batch=4)
    return case, store.contiguous(), nq, [torch.from_numpy(k).cuda() for k in case["kps"]]


def same_run(got, want):
    for key in ("counts", "points", "obs", "cam_idx", "pt_idx", "track_len"):
        msg = differ(key, got[key].reshape(-1), want[key].reshape(-1))
        assert not msg, msg


@pytest.mark.gpu
def test_counts_are_chained_on_the_device(hip):
    """match_edges -> track_components -> build_tracks -> triangulate_tracks with torch's sync debug mode at "error": nobody waits."""
    from sfm_mvs_amd import tracks
    case = ring_case()
    store, nq, pr, off, kp, P = (dev(case["store"]), dev(case["nq"]), dev(np.array(case["pairs"], np.int32)), dev(case["img_off"]), dev(case["kp"]),
                                 dev(case["P"].reshape(-1, 12)))
    tracks.track_components(tracks.match_edges(store, nq, pr, off), int(case["img_off"][-1]))    # warm: the workspace
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        edges = tracks.match_edges(store, nq, pr, off)
        labels, status = tracks.track_components(edges, int(case["img_off"][-1]))
        node_track, track_off, obs_node, counts = tracks.build_tracks(labels, off)
        out = tracks.triangulate_tracks(counts, track_off, obs_node, off, kp, P)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    want = nt.run(case["store"], case["nq"], case["pairs"], case["img_off"], case["kp"], case["P"])
    T, nobs = int(want["counts"][0]), int(want["counts"][1])
    assert status.tolist()[0] == 1 and not differ("counts", counts, want["counts"])
    assert not differ("node_track", node_track, want["node_track"]) and not differ("track_off", track_off[:T + 1], want["track_off"])
    assert not differ("obs_node", obs_node[:nobs], want["obs_node"]) and not differ("X", out[0][:T].reshape(-1), want["X"].reshape(-1))
    assert not differ("err", out[1][:nobs], want["err"]) and not differ("depth", out[2][:nobs], want["depth"])
    assert not differ("flags", out[3][:T], want["flags"]) and not differ("max_err", out[4][:T], want["max_err"])


@pytest.mark.gpu
def test_ring_scene_end_to_end(hip):
    from datagen import ring_cameras
    from sfm_mvs_amd import ba, sharded, tracks
    case, store, nq, kps = ring_device()
    assert np.array_equal(store.cpu().numpy(), case["store"])                           # the matcher's store is the oracle's
    got = tracks.run_tracks(store, nq, case["pairs"], kps, case["P"])
    want = nt.run(case["store"], case["nq"], case["pairs"], case["img_off"], case["kp"], case["P"])
    same_run(got, want)
    assert got["status"][0] == 1 and 1 <= got["status"][1] <= tracks.TRACK_ROUNDS
    # the two calibration bars: every track pure, and the N-view points closer to the planted ones than the first two views' are
    n, pure, ids = purity(case, want)
    assert n == 400 == len(got["points"]) and pure == n and np.all(got["track_len"] == 8)
    truth = case["X"][ids]
    en = np.median(np.linalg.norm(got["points"].astype(np.float64) - truth, axis=1))
    e2 = np.median(np.linalg.norm(two_view(case, want).astype(np.float64) - truth, axis=1))
    print(f"ring end to end: {n} tracks, median error N-view {en:.5f} two-view {e2:.5f} ratio {en / e2:.3f} (bar {RING_BAR:.3f})")
    assert en <= RING_BAR * e2
    # max_reproj and min_len filter on the host side of the one download
    same_run(tracks.run_tracks(store, nq, case["pairs"], kps, case["P"], min_len=3, max_reproj=1.0),
             nt.run(case["store"], case["nq"], case["pairs"], case["img_off"], case["kp"], case["P"], min_len=3, max_reproj=1.0))
    # a permuted pair order gives the same tracks
    perm = np.random.default_rng(8).permutation(len(case["pairs"]))
    again = tracks.run_tracks(store[torch.from_numpy(perm).cuda()].contiguous(), [nq[p] for p in perm], [case["pairs"][p] for p in perm], kps, case["P"])
    same_run(again, want)
    # the verified matches as keep: as many per pair as verify_pairs_sharded counts, and the tracks of the restatement under that mask
    keep = tracks.verify_keep(store, nq, case["pairs"], kps, case["K"])
    counts = sharded.verify_pairs_sharded(store, nq, case["pairs"], kps, case["K"])
    assert keep.dtype == torch.uint8 and tuple(keep.shape) == (len(case["pairs"]), store.shape[2])
    assert np.array_equal(keep.sum(dim=1).cpu().numpy(), np.maximum(counts.numpy(), 0)) and int(counts.min()) > 100
    kept = tracks.run_tracks(store, nq, case["pairs"], kps, case["P"], keep=keep)
    same_run(kept, nt.run(case["store"], case["nq"], case["pairs"], case["img_off"], case["kp"], case["P"], keep=keep.cpu().numpy()))
    assert len(kept["points"]) > 350
    # the points go through the sparse Schur bundle adjustment from perturbed poses: the cost falls
    cams = ring_cameras(8) * (1 + 0.002 * np.random.default_rng(4).standard_normal((8, 6)))
    _, _, hist = ba.bundle_adjust_schur(dev(cams), case["K"], dev(got["points"]), dev(got["obs"]), dev(got["cam_idx"]), dev(got["pt_idx"]), iters=3)
    print(f"schur BA on the tracks: cost {hist[0]:.4g} -> {hist[-1]:.4g} over {len(hist) - 1} iterations")
    assert len(hist) >= 2 and all(b <= a for a, b in zip(hist, hist[1:])) and hist[-1] < hist[0]


@pytest.mark.gpu
def test_run_tracks_waits_for_the_host_twice(hip):
    from sfm_mvs_amd import _lib, tracks
    case, store, nq, kps = ring_device()
    tracks.run_tracks(store, nq, case["pairs"], kps, case["P"])          # warm: the pinned host pool, the workspace
    torch.cuda.synchronize()
    lib0 = int(_lib.lib().sfm_host_sync_count())
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            out = tracks.run_tracks(store, nq, case["pairs"], kps, case["P"], max_reproj=2.0)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    syncs = [str(w.message) for w in caught if "synchroniz" in str(w.message).lower()]
    assert len(syncs) == 2, syncs                                     # the counts with the status, the one download
    assert int(_lib.lib().sfm_host_sync_count()) == lib0 and len(out["points"]) > 0
    # a labelling cut short is resumed: one round per call still ends converged, with the same tracks
    slow = tracks.run_tracks(store, nq, case["pairs"], kps, case["P"], max_reproj=2.0, rounds=1)
    assert slow["status"][0] == 1 and slow["status"][1] >= 1
    same_run(slow, out)


@pytest.mark.gpu
def test_a_short_fixed_seed_fuzz_run_finds_no_mismatch(hip):
    counts, bad, dt = fz.run(10.0, 4444)
    print(f"fuzz_tracks: seed 4444, {sum(counts.values())} cases {counts}, {bad} mismatches, {dt:.0f} s")
    assert bad == 0 and all(c > 0 for c in counts.values()), counts


@pytest.mark.gpu
def test_committed_fuzz_logs_are_clean_and_name_this_code(hip):
    """profiles/tracks_fuzz_seed*.log: no mismatch, and run on the code of csrc/tracks.hip and csrc/common.h that the loaded library
    was built from (scripts/knn_code_hash.py: comments and whitespace do not count)."""
    import glob
    import re
    from sfm_mvs_amd import _lib
    have = _lib.code_hashes_of_binary()
    logs = sorted(glob.glob(os.path.join(ROOT, "profiles", "tracks_fuzz_seed*.log")))
    assert len(logs) >= 2, logs
    total = 0
    for path in logs:
        text = open(path).read()
        m = re.search(r"fuzz_tracks: seed \d+, (\d+) cases .*?, (\d+) mismatches", text)
        assert m and int(m.group(2)) == 0, f"{path}: no clean summary line"
        ids = re.findall(r"sfm_build_id (knn\.hip:\S+(?: \S+:\S+)*)", text)
        assert ids, f"{path} does not name the build it ran on"
        logged = dict(tok.split(":", 1) for tok in ids[-1].split() if ":" in tok)
        for name in ("tracks.hip", "common.h"):
            assert logged.get(name) == have[name], f"{path} was produced by another csrc/{name} than the loaded binary's"
        total += int(m.group(1))
    assert total >= FUZZ_FLOOR, total
