"""The TRACKS-REFINE family on the device (sfm_track_refine, sfm_track_prune, tracks.run_tracks(robust=True)): every output equal to
the restatement tests/np_tracks_refine.py, float rows as int32 views; there is no tolerance (include/sfm_hip.h, "TRACKS-REFINE";
docs/tracks.md §8)."""
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
import np_tracks_refine as nr  # noqa: E402
import fuzz_tracks as fz  # noqa: E402
import fuzz_tracks_refine as fr  # noqa: E402
from fuzz_tracks import dev, differ  # noqa: E402
from test_tracks_refine_cpu import corrupted_ring, crossing_case  # noqa: E402

INT32_MAX = 2 ** 31 - 1
FUZZ_FLOOR = 6000              # a tenth of the cases the committed logs hold, rounded down to one figure (docs/tracks.md §8.5)


def grid_tracks(rng, T, L, noise=0.3, displaced=0.25):
    """T tracks of exactly L observations over L cameras (node = image * T + track) -> (img_off, kp, P, track_off, obs_node, counts)."""
    P = fz.random_cameras(rng, L)
    X = rng.normal(size=(T, 3)); X /= np.maximum(np.linalg.norm(X, axis=1, keepdims=True), 1.0)
    h = np.einsum("kij,tj->kti", P.reshape(L, 3, 4), np.c_[X, np.ones(T)])
    kp = (h[..., :2] / h[..., 2:] + rng.normal(0, noise, (L, T, 2))).astype(np.float32)
    hit = np.flatnonzero(rng.random(T) < displaced)
    kp[rng.integers(0, L, len(hit)), hit] += (rng.uniform(20, 100, (len(hit), 1)) * np.sign(rng.normal(size=(len(hit), 2)))).astype(np.float32)
    obs_node = (np.arange(L)[None, :] * T + np.arange(T)[:, None]).reshape(-1).astype(np.int32)
    return ((np.arange(L + 1) * T).astype(np.int32), kp.reshape(L * T, 2), P, (L * np.arange(T + 1)).astype(np.int32), obs_node,
            np.array([T, L * T, 0, 0, 0, 0], np.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("length", [2, 3, 64, 65])
def test_tracks_of_every_count_and_length(hip, length):
    """Track counts around a workgroup and a wave; lengths 64 and 65 put 64 and 65 inliers at the cap of the angle's pair loop."""
    rng = np.random.default_rng(3000 + length)
    for T in (0, 1, 2, 3, 255, 256, 257):
        case = grid_tracks(rng, T, length)
        msg, out, want = fr.check_refine(*case)
        assert not msg, (T, length, msg)
        if T >= 255:
            assert want[4].max() == length and want[7].max() > 0
        if T >= 255 and length >= 64:                                        # 63 views outvote a displaced keypoint
            assert (want[8] == 3).all() and (want[1] == 0).sum() >= 1 and want[6].max() < 0.0 and want[4].min() >= length - 2
        ok = fr.check_prune(int(case[0][-1]), case[3], case[4], want[0], want[1], want[4], want[5], want[6], want[8], dict(min_len=2, max_reproj=2.0, max_cos=1.0))
        assert not ok, (T, length, ok)


def small_tracks(kind):
    """Five tracks of four views, 0.3 px noise; `kind` plants one degeneracy -> (case tuple, X_in or None, flags_in or None)."""
    rng = np.random.default_rng(77)
    img_off, kp, P, track_off, obs_node, counts = grid_tracks(rng, 5, 4, displaced=0.0)
    X_in = flags_in = None
    if kind == "all_outliers":
        kp[obs_node[4:8]] += np.float32([[60, 10], [-45, 30], [25, -70], [-30, -55]])
    if kind == "identical":
        P[:] = P[0]
    if kind == "affine":                                                     # the second camera's 3 x 3 part is singular: its centre is no point
        P.reshape(-1, 3, 4)[1, 2, :3] = 0.0
    if kind == "nan":                                                        # NaN from the start: the DLT point is NaN, the track is not started
        kp[obs_node[5]] = np.nan
    if kind == "bad_node":
        obs_node[[6, 13]] = (-1, 20)
    if kind in ("behind", "nan_start", "flag_clear", "nan_later"):
        X_in, _, _, flags_in, _ = nt.triangulate(track_off, obs_node, img_off, kp, P)
    if kind == "nan_later":                                                  # a good start, then a NaN keypoint: that observation is unusable
        kp[obs_node[5]] = np.nan
    if kind == "behind":                                                     # track 2 starts beyond the centre of its second camera
        X_in[2] = (1.5 * nr.centres(P)[1]).astype(np.float32)
    if kind == "nan_start":
        X_in[3, 1] = np.nan
    if kind == "flag_clear":
        flags_in[0] = 1
    return (img_off, kp, P, track_off, obs_node, counts), X_in, flags_in


@pytest.mark.gpu
def test_a_trial_step_behind_the_cameras_is_refused(hip):
    """The hand-built track of test_tracks_refine_cpu.crossing_case: from depth 10 the linear step ends at depth -30.  The device takes
    the steps the restatement takes (it counts five attempts refused for a trial point behind the cameras) and arrives at depth 2."""
    track_off, obs_node, img_off, kp, P, X_in, flags_in = crossing_case()
    case = (np.int32(img_off), kp, P, np.int32(track_off), np.int32(obs_node), np.array([1, 2, 0, 0, 0, 0], np.int32), X_in, flags_in)
    for iters, steps, crossed in ((10, 4, 5), (50, 11, 5)):
        msg, out, want = fr.check_refine(*case, iters=iters)
        assert not msg, (iters, msg)
        assert nr.refine(track_off, obs_node, img_off, kp, P, X_in, flags_in, iters=iters, detail=True)[11].tolist() == [crossed]
        assert out[7][:1].tolist() == [steps] and float(out[3][:2].min()) > 0.0
    assert out[1][:2].tolist() == [1, 1] and abs(float(out[0][0, 2]) - 2.0) < 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["plain", "all_outliers", "behind", "nan", "nan_later", "nan_start", "flag_clear", "identical", "affine", "bad_node"])
def test_degenerate_tracks(hip, kind):
    case, X_in, flags_in = small_tracks(kind)
    msg, out, want = fr.check_refine(*case, X_in, flags_in)
    assert not msg, msg
    X, inl, err, depth, n_inl, worst, cosm, steps, flags = want
    inl = inl.reshape(5, 4)
    if kind == "plain":
        assert inl.all() and flags.tolist() == [3] * 5 and worst.max() < 2.0 and steps.min() >= 1
    if kind == "all_outliers":
        assert n_inl[1] < 2 and flags[1] & 1 == 0 and [f for k, f in enumerate(flags.tolist()) if k != 1] == [3] * 4
    if kind == "behind":
        assert inl[2, 1] == 0 and depth.reshape(5, 4)[2, 1] == depth.reshape(5, 4)[2, 1]      # unusable from the start, its depth still reported
    if kind == "nan":
        assert not inl[1].any() and flags[1] == 0 and X.view(np.uint32)[1].tolist() == [0x7FC00000] * 3 and err.view(np.uint32)[5] == 0x7FC00000
    if kind == "nan_later":
        assert inl[1].tolist() == [1, 0, 1, 1] and err.view(np.uint32)[5] == 0x7FC00000 and flags[1] == 3
    if kind in ("nan_start", "flag_clear"):
        t = 3 if kind == "nan_start" else 0
        assert (flags[t], n_inl[t], steps[t], cosm[t]) == (0, 0, 0, 1.0) and not inl[t].any() and [f for k, f in enumerate(flags.tolist()) if k != t] == [3] * 4
    if kind == "affine":
        assert not np.isfinite(nr.centres(case[2])[1]).any() and np.isfinite(cosm).all()      # a pair with that centre is NaN and skipped
    if kind == "bad_node":
        assert inl[1].tolist() == [1, 1, 0, 1] and inl[3].tolist() == [1, 0, 1, 1] and err.view(np.uint32)[[6, 13]].tolist() == [0x7FC00000] * 2
    for seed in range(25 if kind == "plain" else 0):                         # once: the fuzzer's generator with its degeneracies
        g = fr.gen_refine(np.random.default_rng(seed))
        keep = int(np.searchsorted(g[3], 600, side="right")) - 1             # the first tracks, some 600 observations
        off = g[3][:keep + 1]
        counts = np.array([keep, off[-1], 0, 0, 0, 0], np.int32)
        start = (None, None) if g[6] is None else (g[6][0][:keep], g[6][1][:keep])
        msg = fr.check_refine(g[0], g[1], g[2], off, g[4][:off[-1]], counts, *start, **g[7])[0]
        assert not msg, (seed, msg)


@pytest.mark.gpu
@pytest.mark.parametrize("params", [dict(huber=float("inf")), dict(iters=0), dict(iters2=0), dict(iters=0, iters2=0), dict(iters=50, iters2=50),
                                    dict(huber=0.25, obs_thresh=0.5)])
def test_parameters(hip, params):
    from sfm_mvs_amd import tracks
    case = grid_tracks(np.random.default_rng(5), 300, 6)
    msg, out, want = fr.check_refine(*case, **params)
    assert not msg, (params, msg)
    if params.get("iters") == 0 and params.get("iters2") == 0:               # no attempt: the triangulation's own errors and depths
        n = int(case[0][-1])
        tri = tracks.triangulate_tracks(dev(case[5]), dev(fr.padded(case[3], n // 2 + 2)), dev(case[4]), dev(case[0]), dev(case[1]), dev(case[2]))
        assert not differ("err", out[2], tri[1]) and not differ("depth", out[3], tri[2]) and not differ("X", out[0][:300].reshape(-1), tri[0][:300].reshape(-1))
        assert not want[7].any()
    if params.get("iters") == 50:
        assert want[7].max() <= 100


@pytest.mark.gpu
def test_garbage_device_counts_are_clamped(hip):
    """counts = (INT32_MAX, -7): every row of the capacity is a track, offsets and nodes are clamped, nothing lands outside the buffers."""
    from sfm_mvs_amd import tracks
    img_off, kp, P, track_off, obs_node, _ = grid_tracks(np.random.default_rng(9), 5, 8, displaced=0.0)
    n, cap = 40, 21
    counts = np.array([INT32_MAX, -7, 0, 0, 0, 0], np.int32)
    off_full, obs_full = fr.padded(track_off, n // 2 + 2), fr.padded(obs_node, n)
    args = (dev(counts), dev(off_full), dev(obs_full), dev(img_off), dev(kp), dev(P))
    X, _, _, flags, _ = tracks.triangulate_tracks(*args)
    out = fr.refine_buffers(n)
    tracks.refine_tracks(*args, X, flags, out=out)
    lo = np.clip(off_full[:-1].astype(np.int64), 0, n)
    hi = np.minimum(np.maximum(off_full[1:].astype(np.int64), lo), n)
    assert hi[:5].tolist() == [8, 16, 24, 32, 40] and lo[5:].tolist() == [40] * 16                # the rows after the five tracks are empty
    want = nr.refine(np.r_[lo, n], obs_full, img_off, kp, P, X.cpu().numpy(), flags.cpu().numpy())
    msg = fr.compare_refine(out, want, cap, n)
    assert not msg, msg
    pruned = tracks.prune_tracks(args[0], args[1], args[2], *[out[k] for k in (0, 1, 4, 5, 6, 8)], max_reproj=2.0)
    wp = nr.prune(np.r_[lo, n], obs_full, *[want[k] for k in (0, 1, 4, 5, 6, 8)], 2, 2.0)
    assert not differ("counts2", pruned[4], wp[4]) and wp[4].tolist() == [5, 40, 16, 0]
    assert not differ("track_off2", pruned[0][:6], wp[0]) and not differ("obs_node2", pruned[1][:40], wp[1]) and not differ("src", pruned[3][:5], wp[3])


def guarded(rows, dtype, width=None):
    """(whole, view): `rows` rows between two guards of 64 rows, every byte of it 0x5A."""
    shape = (rows + 128,) if width is None else (rows + 128, width)
    nbytes = (rows + 128) * (width or 1) * torch.empty(0, dtype=dtype).element_size()
    whole = torch.full((nbytes,), fr.BYTE, dtype=torch.uint8, device="cuda").view(dtype).view(shape)
    return whole, whole[64:64 + rows]


def guards_intact(whole, rows):
    b = whole.view(-1).view(torch.uint8).view(whole.shape[0], -1)
    return bool((b[:64] == fr.BYTE).all()) and bool((b[64 + rows:] == fr.BYTE).all())


@pytest.mark.gpu
def test_overlapping_ranges_stay_inside_the_buffers(hip):
    """counts = (INT32_MAX, -7) over offsets past the true T that lie INSIDE 0..nobs and in no order: the ranges of 901 extra tracks
    overlap those of the 300 real ones and each other, so lanes read rows of depth_dev that other lanes write.  The words are then
    unspecified (include/sfm_hip.h); what is checked is that nothing lands outside the arrays and that the flags are flags."""
    from sfm_mvs_amd import tracks
    rng = np.random.default_rng(31)
    img_off, kp, P, track_off, obs_node, _ = grid_tracks(rng, 300, 8)
    n, cap = 2400, 1201
    off_full = np.r_[track_off, rng.integers(0, n + 1, n // 2 + 2 - len(track_off))].astype(np.int32)
    lo = np.clip(off_full[:-1].astype(np.int64), 0, n)
    hi = np.minimum(np.maximum(off_full[1:].astype(np.int64), lo), n)
    assert (hi[300:] > lo[300:]).sum() > 300 and int((hi - lo).sum()) > 40 * n                     # the ranges cover every row many times
    args = (dev(np.array([INT32_MAX, -7, 0, 0, 0, 0], np.int32)), dev(off_full), dev(obs_node), dev(img_off), dev(kp), dev(P))
    X, _, _, flags, _ = tracks.triangulate_tracks(*args)
    f32, i32 = torch.float32, torch.int32
    bufs = [guarded(cap, f32, 3), guarded(n, torch.uint8), guarded(n, f32), guarded(n, f32), guarded(cap, i32), guarded(cap, f32), guarded(cap, f32),
            guarded(cap, i32), guarded(cap, i32)]
    out = tracks.refine_tracks(*args, X, flags, out=tuple(v for _, v in bufs))
    pb = [guarded(n // 2 + 2, i32), guarded(n, i32), guarded(cap, f32, 3), guarded(cap, i32), guarded(4, i32)]
    tracks.prune_tracks(args[0], args[1], args[2], *[out[k] for k in (0, 1, 4, 5, 6, 8)], max_reproj=2.0, out=tuple(v for _, v in pb))
    torch.cuda.synchronize()
    for (whole, view), rows in zip(bufs + pb, [cap, n, n, n, cap, cap, cap, cap, cap, n // 2 + 2, n, cap, cap, 4]):
        assert guards_intact(whole, rows), rows
    assert set(out[1].unique().tolist()) <= {0, 1} and set(out[8].unique().tolist()) <= {0, 1, 2, 3} and 0 <= int(out[4].min()) and int(out[4].max()) <= n
    c2 = pb[4][1].tolist()
    assert 0 <= c2[0] <= cap and c2[0] + c2[2] == cap


def ring_tensors(c):
    case = c["case"]
    return (dev(case["store"]), dev(case["nq"]), dev(np.array(case["pairs"], np.int32)), dev(case["img_off"]), dev(c["kp"]), dev(case["P"].reshape(-1, 12)))


@pytest.mark.gpu
def test_the_chain_never_waits_and_a_second_refine_flags_nothing_more(hip):
    """match_edges -> ... -> triangulate -> refine -> prune -> triangulate -> refine with torch's sync debug mode at "error"."""
    from sfm_mvs_amd import tracks
    c = corrupted_ring()
    store, nq, pr, off, kp, P = ring_tensors(c)
    n = int(c["case"]["img_off"][-1])

    def chain():
        labels, _ = tracks.track_components(tracks.match_edges(store, nq, pr, off), n)
        _, track_off, obs_node, counts = tracks.build_tracks(labels, off)
        tri = tracks.triangulate_tracks(counts, track_off, obs_node, off, kp, P)
        ref = tracks.refine_tracks(counts, track_off, obs_node, off, kp, P, tri[0], tri[3])
        pruned = tracks.prune_tracks(counts, track_off, obs_node, ref[0], ref[1], ref[4], ref[5], ref[6], ref[8], 2, 2.0)
        tri2 = tracks.triangulate_tracks(pruned[4], pruned[0], pruned[1], off, kp, P)
        return ref, pruned, tracks.refine_tracks(pruned[4], pruned[0], pruned[1], off, kp, P, tri2[0], tri2[3])

    chain()                                                                  # warm: the workspaces
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ref, pruned, ref2 = chain()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    b = c["base"]
    want = nr.refine(b["track_off"], b["obs_node"], c["case"]["img_off"], c["kp"], c["case"]["P"], b["X"], b["flags"])
    for k, name in enumerate(("X", "inlier", "err", "depth", "n_inl", "max_err", "cos_min", "steps", "flags")):
        rows = 3200 if k in (1, 2, 3) else 400
        got = ref[k][:rows].cpu().numpy()
        assert np.array_equal(got.view(np.uint8), np.asarray(want[k]).view(np.uint8)), name
    wp = nr.prune(b["track_off"], b["obs_node"], *[want[k] for k in (0, 1, 4, 5, 6, 8)], 2, 2.0)
    T2, nobs2 = int(wp[4][0]), int(wp[4][1])
    assert (T2, nobs2, int(wp[4][2])) == (400, 3200 - 107, 0) and not differ("counts2", pruned[4], wp[4])
    assert not differ("track_off2", pruned[0][:T2 + 1], wp[0]) and not differ("obs_node2", pruned[1][:nobs2], wp[1])
    assert not differ("X2", pruned[2][:T2].reshape(-1), wp[2].reshape(-1)) and not differ("track_src", pruned[3][:T2], wp[3])
    # refining the pruned set again keeps every observation it has left
    assert int(ref2[1][:nobs2].sum()) == nobs2 and ref2[4][:T2].cpu().numpy().tolist() == np.diff(wp[0]).tolist() and (ref2[8][:T2] == 3).all()


@pytest.mark.gpu
def test_prune_nothing_everything_and_the_exact_boundaries(hip):
    rng = np.random.default_rng(12)
    for _ in range(5):
        g = list(fr.gen_prune(rng))
        T = len(g[1]) - 1
        for kw in (dict(min_len=2, max_reproj=float("inf"), max_cos=1.0), dict(min_len=INT32_MAX, max_reproj=float("inf"), max_cos=1.0),
                   dict(min_len=2, max_reproj=0.0, max_cos=-2.0)):
            g[9] = kw
            msg = fr.check_prune(*g)
            assert not msg, (kw, msg)
    # all tracks good: nothing goes; the bounds exactly at the values that occur, and one step inside them
    n, T = 600, 257
    track_off = (2 * np.arange(T + 1)).astype(np.int32)
    obs_node = rng.permutation(n)[:2 * T].astype(np.int32)
    X = rng.normal(size=(T, 3)).astype(np.float32)
    inlier = np.ones(2 * T, np.uint8)
    n_inl, flags = np.full(T, 2, np.int32), np.full(T, 3, np.int32)
    worst = rng.choice(np.float32([0.5, 1.0, 2.0]), T)
    cosm = rng.choice(np.float32([0.25, 0.9990482, 1.0]), T)
    below = lambda v: float(np.nextafter(np.float32(v), np.float32(-9)))  # noqa: E731
    for kw, kept in ((dict(min_len=2, max_reproj=float("inf"), max_cos=1.0), T), (dict(min_len=3, max_reproj=float("inf"), max_cos=1.0), 0),
                     (dict(min_len=2, max_reproj=2.0, max_cos=1.0), T), (dict(min_len=2, max_reproj=below(2.0), max_cos=1.0), int((worst < 2).sum())),
                     (dict(min_len=2, max_reproj=9.0, max_cos=float(np.float32(0.9990482))), int((cosm < 1).sum())),
                     (dict(min_len=2, max_reproj=9.0, max_cos=below(0.9990482)), int((cosm < 0.5).sum()))):
        msg = fr.check_prune(n, track_off, obs_node, X, inlier, n_inl, worst, cosm, flags, kw)
        assert not msg, (kw, msg)
        assert int(nr.prune(track_off, obs_node, X, inlier, n_inl, worst, cosm, flags, **kw)[4][0]) == kept, kw


def corrupted_device():
    from sfm_mvs_amd import sharded
    c = corrupted_ring()
    case = c["case"]
    des = [torch.from_numpy(d).cuda() for d in case["des"]]
    store, nq = sharded.match_pairs_sharded(des, case["pairs"], batch=4)
    kps = [torch.from_numpy(c["kp"][a:b]).cuda() for a, b in zip(case["img_off"][:-1], case["img_off"][1:])]
    return c, store.contiguous(), nq, kps


def same(got, want, keys=("counts", "points", "obs", "cam_idx", "pt_idx", "track_len")):
    for key in keys:
        msg = differ(key, got[key].reshape(-1), want[key].reshape(-1))
        assert not msg, msg


@pytest.mark.gpu
def test_corrupted_ring_scene_end_to_end(hip):
    """match_pairs_sharded -> run_tracks(robust=True) -> three iterations of ba.bundle_adjust_schur, one keypoint of 107 tracks displaced."""
    from datagen import ring_cameras
    from sfm_mvs_amd import _lib, ba, tracks
    c, store, nq, kps = corrupted_device()
    case = c["case"]
    assert np.array_equal(store.cpu().numpy(), case["store"])
    tracks.run_tracks(store, nq, case["pairs"], kps, case["P"], max_reproj=2.0, robust=True)       # warm: the pinned host pool, the workspaces
    torch.cuda.synchronize()
    lib0 = int(_lib.lib().sfm_host_sync_count())
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            got = tracks.run_tracks(store, nq, case["pairs"], kps, case["P"], max_reproj=2.0, robust=True)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    syncs = [str(w.message) for w in caught if "synchroniz" in str(w.message).lower()]
    assert len(syncs) == 2, syncs                                            # the counts with the status and the pruned counts, the one download
    assert int(_lib.lib().sfm_host_sync_count()) == lib0
    want = nr.run_robust(c["base"], case["img_off"], c["kp"], case["P"], 2, 2.0)
    same(got, want)
    plain = tracks.run_tracks(store, nq, case["pairs"], kps, case["P"], max_reproj=2.0)
    print(f"corrupted ring end to end: robust {len(got['points'])} points, {got['obs_dropped']} observations and {got['tracks_dropped']} tracks dropped; "
          f"max_reproj alone {len(plain['points'])} points")
    assert len(got["points"]) == 400 and got["tracks_dropped"] == 0 and got["obs_dropped"] == want["obs_dropped"] >= 107
    assert len(plain["points"]) == 400 - 107 < len(got["points"])
    # a minimum angle no ring track fails (the rays span the ring) and one that only opposite cameras meet
    assert len(tracks.run_tracks(store, nq, case["pairs"], kps, case["P"], robust=True, min_angle_deg=5.0)["points"]) == 400
    wide = tracks.run_tracks(store, nq, case["pairs"], kps, case["P"], robust=True, min_angle_deg=178.0)
    same(wide, nr.run_robust(c["base"], case["img_off"], c["kp"], case["P"], 2, None, max_cos=float(np.cos(np.deg2rad(178.0)))))
    assert 0 < len(wide["points"]) < 400 and wide["tracks_dropped"] == 400 - len(wide["points"])
    cams = ring_cameras(8) * (1 + 0.002 * np.random.default_rng(4).standard_normal((8, 6)))
    _, _, hist = ba.bundle_adjust_schur(dev(cams), case["K"], dev(got["points"]), dev(got["obs"]), dev(got["cam_idx"]), dev(got["pt_idx"]), iters=3)
    print(f"schur BA on the robust tracks: cost {hist[0]:.4g} -> {hist[-1]:.4g} over {len(hist) - 1} iterations")
    assert len(hist) >= 2 and all(b <= a for a, b in zip(hist, hist[1:])) and hist[-1] < hist[0]


@pytest.mark.gpu
def test_without_robust_run_tracks_returns_what_it_returned(hip):
    from sfm_mvs_amd import tracks
    c, store, nq, kps = corrupted_device()
    case = c["case"]
    for kw in (dict(), dict(max_reproj=2.0), dict(min_len=3, max_reproj=1.0)):
        got = tracks.run_tracks(store, nq, case["pairs"], kps, case["P"], robust=False, **kw)
        same(got, nt.run(case["store"], case["nq"], case["pairs"], case["img_off"], c["kp"], case["P"], **kw))
        assert sorted(got) == ["cam_idx", "counts", "obs", "points", "pt_idx", "status", "track_len"]


@pytest.mark.gpu
def test_a_short_fixed_seed_fuzz_run_finds_no_mismatch(hip):
    counts, bad, dt = fr.run(10.0, 5555)
    print(f"fuzz_tracks_refine: seed 5555, {sum(counts.values())} cases {counts}, {bad} mismatches, {dt:.0f} s")
    assert bad == 0 and all(c > 0 for c in counts.values()), counts


@pytest.mark.gpu
def test_committed_fuzz_logs_are_clean_and_name_this_code(hip):
    """profiles/tracks_refine_fuzz_seed*.log: no mismatch, and run on the code of csrc/tracks_refine.hip and csrc/common.h that the loaded
    library was built from (scripts/knn_code_hash.py: comments and whitespace do not count)."""
    import glob
    import re
    from sfm_mvs_amd import _lib
    have = _lib.code_hashes_of_binary()
    logs = sorted(glob.glob(os.path.join(ROOT, "profiles", "tracks_refine_fuzz_seed*.log")))
    assert len(logs) >= 2, logs
    total = 0
    for path in logs:
        text = open(path).read()
        m = re.search(r"fuzz_tracks_refine: seed \d+, (\d+) cases .*?, (\d+) mismatches", text)
        assert m and int(m.group(2)) == 0, f"{path}: no clean summary line"
        ids = re.findall(r"sfm_build_id (knn\.hip:\S+(?: \S+:\S+)*)", text)
        assert ids, f"{path} does not name the build it ran on"
        logged = dict(tok.split(":", 1) for tok in ids[-1].split() if ":" in tok)
        for name in ("tracks_refine.hip", "common.h"):
            assert logged.get(name) == have[name], f"{path} was produced by another csrc/{name} than the loaded binary's"
        total += int(m.group(1))
    assert total >= FUZZ_FLOOR, total
