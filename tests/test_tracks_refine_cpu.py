"""The TRACKS-REFINE family without a GPU (include/sfm_hip.h, "TRACKS-REFINE"; docs/tracks.md §8): the C-ABI declares, binds, documents
and validates the entry points; the restatement tests/np_tracks_refine.py stands apart from the product, gives hand-checked results on
small tracks, reaches the cost SciPy's minimiser reaches, and meets the calibration bars on the corrupted ring scene."""
import ast
import ctypes
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import np_tracks as nt  # noqa: E402
import np_tracks_refine as nr  # noqa: E402
from test_tracks_cpu import ring_case  # noqa: E402

NEW_SYMBOLS = ("sfm_track_refine_ws_bytes", "sfm_track_refine", "sfm_track_prune_ws_bytes", "sfm_track_prune")

# Measured here with the restatement (docs/tracks.md §8.3) on ring_scene(8, 600, 400, seed=3) with one keypoint of 107 tracks displaced
# by 20 to 100 px (`corrupt`), each recorded with its margin.
# The Huber cost (1 px) at the end of phase 1 (10 attempts) against scipy.optimize.minimize (BFGS, then Nelder-Mead from its point)
# on a cost written here, from the same DLT start, first 50 corrupted tracks: the largest cost1 / scipy - 1 is 9.73e-13 (ten
# attempts end within rounding of the minimum).  The bound is 4 x that.
SCIPY_MARGIN = 3.9e-12
# Median distance of the 107 corrupted tracks' points to the planted ones: DLT 0.07368, refined 0.00164: r = 0.0223; the bar is
# (1 + r) / 2, the rule of RING_BAR.
REFINE_RATIO = 0.0223
REFINE_BAR = (1.0 + REFINE_RATIO) / 2.0
# The same refined median over the median of the same tracks triangulated WITHOUT their planted observation (7 views, DLT): 0.00164 /
# 0.00163 = 1.007; the bar is the mean of the measured value and twice it.
CLEAN_RATIO = 1.007
CLEAN_BAR = (CLEAN_RATIO + 2.0 * CLEAN_RATIO) / 2.0


def test_header_declares_binds_and_documents_the_refine_entry_points():
    from sfm_mvs_amd import _lib
    from test_abi import declared_symbols
    syms = declared_symbols()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    doc = open(os.path.join(ROOT, "docs", "tracks.md")).read()
    header = open(os.path.join(ROOT, "include", "sfm_hip.h")).read()
    assert "TRACKS-REFINE" in header and "no word depends on" in header and "huber * (e - huber / 2)" in header
    for s in NEW_SYMBOLS:
        assert s in syms and s in _lib.SIGNATURES and hasattr(handle, s), s
        assert s in doc, f"docs/tracks.md does not mention {s}"
    assert _lib.lib().sfm_abi_version() == 3 and _lib.ABI_VERSION == 3
    assert "tracks_refine.hip" in _lib.code_hashes_of_binary()


def test_python_layer_exposes_the_entry_points():
    import inspect
    from sfm_mvs_amd import tracks
    sig = inspect.signature(tracks.refine_tracks).parameters
    assert list(sig)[:8] == ["counts", "track_off", "obs_node", "img_off", "keypoints", "P", "X", "flags"]
    assert (sig["huber"].default, sig["obs_thresh"].default, sig["iters"].default, sig["iters2"].default, sig["out"].default) == (1.0, 2.0, 10, 5, None)
    sig = inspect.signature(tracks.prune_tracks).parameters
    assert sig["min_len"].default == 2 and sig["max_reproj"].default is None and sig["min_angle_deg"].default is None
    sig = inspect.signature(tracks.run_tracks).parameters
    assert list(sig)[-5:] == ["robust", "huber", "obs_thresh", "min_angle_deg", "refine_iters"]
    assert [sig[k].default for k in list(sig)[-5:]] == [False, 1.0, 2.0, None, 10]
    assert tracks.max_cos_of(None) == 1.0 and tracks.max_cos_of(0.0) == 1.0 and abs(tracks.max_cos_of(60.0) - 0.5) < 1e-15


def test_argument_errors_are_reported_before_the_device():
    """Every argument error of the header: SFM_ERR_ARG with its message, before any device call (the pointers are never read)."""
    from sfm_mvs_amd import _lib
    L = _lib.lib()
    f = [ctypes.c_void_p(16 * (k + 1)) for k in range(24)]
    big, nan, inf = 1 << 31, float("nan"), float("inf")

    def refine(counts=f[0], to=f[1], on=f[2], off=f[3], n_img=5, kp=f[4], P=f[5], n=100, X=f[6], fl=f[7], huber=1.0, thresh=2.0, iters=10, iters2=5,
               Xo=f[8], inl=f[9], err=f[10], depth=f[11], n_inl=f[12], worst=f[13], cosm=f[14], steps=f[15], flo=f[16], ws=f[17], wsb=1 << 20):
        return L.sfm_track_refine(counts, to, on, off, n_img, kp, P, n, X, fl, huber, thresh, iters, iters2, Xo, inl, err, depth, n_inl, worst, cosm,
                                  steps, flo, ws, wsb, None)

    def prune(counts=f[0], to=f[1], on=f[2], n=100, X=f[3], inl=f[4], n_inl=f[5], worst=f[6], cosm=f[7], fl=f[8], min_len=2, max_reproj=2.0, max_cos=1.0,
              to2=f[9], on2=f[10], X2=f[11], src=f[12], c2=f[13], ws=f[14], wsb=1 << 20):
        return L.sfm_track_prune(counts, to, on, n, X, inl, n_inl, worst, cosm, fl, min_len, max_reproj, max_cos, to2, on2, X2, src, c2, ws, wsb, None)

    cases = [
        (refine, dict(n=-1), b"n_nodes"), (refine, dict(n=big), b"n_nodes"), (refine, dict(n_img=0), b"n_img"), (refine, dict(n_img=65537), b"n_img"),
        (refine, dict(huber=nan), b"huber"), (refine, dict(huber=0.0), b"huber"), (refine, dict(huber=-1.0), b"huber"),
        (refine, dict(thresh=nan), b"obs_thresh"), (refine, dict(thresh=0.0), b"obs_thresh"), (refine, dict(thresh=-2.0), b"obs_thresh"),
        (refine, dict(iters=-1), b"iters"), (refine, dict(iters=51), b"iters"), (refine, dict(iters2=-1), b"iters2"), (refine, dict(iters2=51), b"iters2"),
        (refine, dict(wsb=16), b"workspace"),
    ] + [(refine, {k: None}, b"null") for k in ("counts", "to", "on", "off", "kp", "P", "X", "fl", "Xo", "inl", "err", "depth", "n_inl", "worst", "cosm",
                                                "steps", "flo", "ws")] + [
        (refine, dict(n=0, counts=None), b"null"), (refine, dict(n=0, Xo=None), b"null"),
        (prune, dict(n=-1), b"n_nodes"), (prune, dict(n=big), b"n_nodes"), (prune, dict(min_len=1), b"min_len"), (prune, dict(min_len=-4), b"min_len"),
        (prune, dict(min_len=big), b"min_len"), (prune, dict(max_cos=nan), b"max_cos"), (prune, dict(max_reproj=nan), b"max_reproj"),
        (prune, dict(wsb=16), b"workspace"),
    ] + [(prune, {k: None}, b"null") for k in ("counts", "to", "on", "X", "inl", "n_inl", "worst", "cosm", "fl", "to2", "on2", "X2", "src", "c2", "ws")] + [
        (prune, dict(n=0, c2=None), b"null"), (prune, dict(n=0, to2=None), b"null"),
    ]
    for call, kw, msg in cases:
        assert call(**kw) == -1, (call.__name__, kw)
        assert msg in L.sfm_last_error(), (call.__name__, kw, L.sfm_last_error())
    assert L.sfm_track_refine_ws_bytes(0) == 0 and L.sfm_track_refine_ws_bytes(65537) == 0 and L.sfm_track_prune_ws_bytes(big) == 0
    assert L.sfm_track_prune_ws_bytes(-1) == 0
    assert L.sfm_track_refine_ws_bytes(64) >= 64 * 24 and L.sfm_track_prune_ws_bytes(640000) >= 4 * 320001 and L.sfm_track_prune_ws_bytes(0) > 0


def test_the_restatement_does_not_import_the_product():
    tree = ast.parse(open(os.path.join(ROOT, "tests", "np_tracks_refine.py")).read())
    for node in ast.walk(tree):
        names = [a.name for a in node.names] if isinstance(node, ast.Import) else [node.module or ""] if isinstance(node, ast.ImportFrom) else []
        assert names in ([], ["numpy"]), names


# ---- hand-checked tracks ------------------------------------------------------------------------------------------------------

K = np.array([[900.0, 0, 480.0], [0, 900.0, 320.0], [0, 0, 1.0]])


def turned(deg):
    """K [R | (0, 0, 8)] with R a turn about the y axis: the origin projects to the principal point exactly."""
    c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    if deg % 90 == 0:
        c, s = float(round(c)), float(round(s))
    R = np.array([[c, 0, s], [0, 1.0, 0], [-s, 0, c]])
    return (K @ np.c_[R, [0, 0, 8.0]]).reshape(12)


def project(P, X):
    h = P.reshape(3, 4) @ np.r_[X, 1.0]
    return h[:2] / h[2]


def test_a_two_view_track_with_no_noise_takes_no_step():
    P = np.stack([turned(0), turned(90)])
    kp = np.array([[480.0, 320.0], [480.0, 320.0]], np.float32)
    out = nr.refine([0, 2], [0, 1], [0, 1, 2], kp, P, np.zeros((1, 3), np.float32), [3])
    X, inl, err, depth, n_inl, worst, cosm, steps, flags = out
    assert steps.tolist() == [0] and inl.tolist() == [1, 1] and n_inl.tolist() == [2] and flags.tolist() == [3]
    assert X.tolist() == [[0.0, 0.0, 0.0]] and err.tolist() == [0.0, 0.0] and depth.tolist() == [8.0, 8.0] and worst.tolist() == [0.0]
    assert np.array_equal(nr.centres(P), [[0.0, 0.0, -8.0], [8.0, 0.0, 0.0]]) and cosm.tolist() == [0.0]          # the two rays are at right angles


def test_one_observation_moved_by_50_px_is_the_one_flagged():
    """Three cameras turned about the y axis, one keypoint moved 50 px along y: beyond the Huber width the moved observation pulls the
    point with a constant weight of 1 px while the two others resist with their own errors, so they settle near 0.5 px each, inside
    obs_thresh = 2, and phase 2 then fits them alone.  (Three views cannot outvote every displacement: one with a large component
    along the epipolar lines is matched by a wrong depth instead.)"""
    P = np.stack([turned(0), turned(40), turned(-35)])
    Xt = np.array([0.3, -0.2, 0.4])
    kp = np.stack([project(p, Xt) for p in P]).astype(np.float32)
    img_off, track_off, obs_node = [0, 1, 2, 3], [0, 3], [0, 1, 2]
    for moved in range(3):
        bad = kp.copy()
        bad[moved] += np.float32([0.0, 50.0])
        X0, _, _, fl0, w0 = nt.triangulate(track_off, obs_node, img_off, bad, P)
        X, inl, err, depth, n_inl, worst, cosm, steps, flags = nr.refine(track_off, obs_node, img_off, bad, P, X0, fl0)
        assert inl.tolist() == [int(k != moved) for k in range(3)] and n_inl.tolist() == [2] and flags.tolist() == [3] and steps[0] > 0
        assert w0[0] > 5.0 and worst[0] < 0.01 and err[moved] > 45.0 and np.abs(X[0] - Xt).max() < 1e-4 < np.abs(X0[0] - Xt).max()
        off2, obs2, X2, src, c2 = nr.prune(track_off, obs_node, X, inl, n_inl, worst, cosm, flags, 2, 2.0)
        assert c2.tolist() == [1, 2, 0, 1] and obs2.tolist() == [k for k in range(3) if k != moved] and off2.tolist() == [0, 2]


def test_an_unstarted_track_and_unusable_observations():
    P = np.stack([turned(0), turned(40), turned(-35)])
    kp = np.stack([project(p, np.zeros(3)) for p in P]).astype(np.float32)
    nan3 = np.full((1, 3), np.nan, np.float32)
    for X_in, fl in ((nan3, [3]), (np.zeros((1, 3), np.float32), [1])):
        X, inl, err, depth, n_inl, worst, cosm, steps, flags = nr.refine([0, 3], [0, 1, 2], [0, 1, 2, 3], kp, P, X_in, fl)
        assert X.view(np.uint32).tolist() == nr.canonical(X_in).view(np.uint32).tolist() and inl.tolist() == [0, 0, 0]
        assert (n_inl[0], steps[0], flags[0], worst[0], cosm[0]) == (0, 0, 0, 0.0, 1.0)
    # a node outside 0..N-1 and a NaN keypoint are unusable: NaN error (and depth for the node), no inlier; the other two carry the track
    kp4 = np.vstack([kp, [[np.nan, 5.0]]]).astype(np.float32)
    P4 = np.vstack([P, turned(70)[None]])
    out = nr.refine([0, 4], [0, 7, 2, 3], [0, 1, 2, 3, 4], kp4, P4, np.zeros((1, 3), np.float32), [3])
    assert out[1].tolist() == [1, 0, 1, 0] and out[4].tolist() == [2] and out[8].tolist() == [3]
    assert out[2].view(np.uint32)[[1, 3]].tolist() == [0x7FC00000] * 2 and out[3].view(np.uint32)[1] == 0x7FC00000 and out[3][3] == 8.0


def crossing_case():
    """Two cameras side by side (centres (0, 0, 0) and (1, 0, 0), both looking along z) see a point at depth 2 on the first one's axis,
    a disparity of 450 px; the start lies at depth 10, where the disparity is 90 -> (track_off, obs_node, img_off, kp, P, X_in, flags_in)."""
    P = np.stack([(K @ np.c_[np.eye(3), [0.0, 0, 0]]).reshape(12), (K @ np.c_[np.eye(3), [-1.0, 0, 0]]).reshape(12)])
    return [0, 2], [0, 1], [0, 1, 2], np.float32([[480, 320], [30, 320]]), P, np.float32([[0, 0, 10]]), [3]


def test_a_trial_step_behind_the_cameras_is_refused():
    """The disparity falls as 1 / z, so from depth 10 the linear step towards 450 px is z (1 - z / 2) = -40: the trial point lies at
    depth -30, behind both cameras.  The attempt is refused and lam grows tenfold until the damped step stays in front; five attempts
    are refused for that reason (the restatement counts them) before the point has walked in to depth 2."""
    out = nr.refine(*crossing_case(), iters=50, detail=True)
    X, inl, err, depth, n_inl, worst, cosm, steps, flags, _, _, crossed = out
    assert crossed.tolist() == [5] and steps.tolist() == [11] and inl.tolist() == [1, 1] and flags.tolist() == [3]
    assert np.abs(X[0] - [0, 0, 2]).max() < 1e-6 and depth.tolist() == [2.0, 2.0] and err.max() < 1e-3
    assert abs(cosm[0] - 2 / np.sqrt(5)) < 1e-6                                            # rays (0, 0, 2) and (-1, 0, 2)
    short = nr.refine(*crossing_case(), detail=True)                                       # ten attempts: five refused, still on the way
    assert short[11].tolist() == [5] and short[7].tolist() == [4] and 0 < short[3].min() < 2.0 and short[1].tolist() == [1, 0]


def test_prune_at_its_boundaries():
    track_off, obs_node = [0, 3, 6, 8], [0, 4, 8, 1, 5, 9, 2, 6]
    X = np.arange(9, dtype=np.float32).reshape(3, 3)
    inlier = [1, 1, 1, 1, 0, 1, 1, 1]
    n_inl, worst, cosm, flags = [3, 2, 2], np.float32([1.5, 2.0, 0.25]), np.float32([0.5, 0.75, 0.99]), [3, 3, 3]
    run = lambda **kw: nr.prune(track_off, obs_node, X, inlier, n_inl, worst, cosm, flags, **kw)  # noqa: E731
    off2, obs2, X2, src, c2 = run()
    assert c2.tolist() == [3, 7, 0, 1] and off2.tolist() == [0, 3, 5, 7] and obs2.tolist() == [0, 4, 8, 1, 9, 2, 6] and src.tolist() == [0, 1, 2]
    assert run(min_len=3)[3].tolist() == [0] and run(min_len=3)[4].tolist() == [1, 3, 2, 0]        # n_inl == min_len stays, min_len - 1 goes
    assert run(min_len=4)[4].tolist() == [0, 0, 3, 0] and run(min_len=4)[0].tolist() == [0]
    assert run(max_reproj=2.0)[3].tolist() == [0, 1, 2] and run(max_reproj=float(np.nextafter(np.float32(2.0), np.float32(0))))[3].tolist() == [0, 2]
    assert run(max_cos=0.75)[3].tolist() == [0, 1] and run(max_cos=float(np.nextafter(0.75, 0.0)))[3].tolist() == [0]
    assert run(max_cos=0.75)[2].tolist() == X[:2].tolist() and run(max_cos=0.75)[1].tolist() == [0, 4, 8, 1, 9]
    # flags other than 3 and a NaN largest error fail, whatever the bounds
    assert nr.prune(track_off, obs_node, X, inlier, n_inl, np.float32([np.nan, 1, 1]), cosm, [3, 2, 3])[3].tolist() == [2]
    assert nr.prune([0], [], np.zeros((0, 3)), [], [], [], [], [])[4].tolist() == [0, 0, 0, 0]


# ---- the corrupted ring scene -------------------------------------------------------------------------------------------------

def corrupt(track_off, obs_node, kp, seed=7):
    """One keypoint of a quarter of the tracks displaced by 20 to 100 px -> (kp', corrupted tracks, their displaced observation rows)."""
    rng = np.random.default_rng(seed)
    track_off = np.asarray(track_off, np.int64)
    bad = np.flatnonzero(rng.random(len(track_off) - 1) < 0.25)
    rows = track_off[bad] + rng.integers(0, np.diff(track_off)[bad])
    mag, ang = rng.uniform(20.0, 100.0, len(bad)), rng.uniform(0.0, 2.0 * np.pi, len(bad))
    out = np.array(kp, np.float32)
    out[np.asarray(obs_node)[rows]] += np.stack([mag * np.cos(ang), mag * np.sin(ang)], 1).astype(np.float32)
    return out, bad, rows


@functools.lru_cache(maxsize=None)
def corrupted_ring():
    """-> dict: the ring case, its plain tracks on the corrupted keypoints (`base`), the planted ids, the corrupted tracks and rows."""
    case = ring_case()
    clean = nt.run(case["store"], case["nq"], case["pairs"], case["img_off"], case["kp"], case["P"])
    kp, bad, rows = corrupt(clean["track_off"], clean["obs_node"], case["kp"])
    base = nt.run(case["store"], case["nq"], case["pairs"], case["img_off"], kp, case["P"])
    ids = case["ids"][base["obs_node"][base["track_off"][:-1]]]
    return dict(case=case, kp=kp, bad=bad, rows=rows, base=base, truth=case["X"][ids], clean=clean)


@functools.lru_cache(maxsize=None)
def refined_ring():
    c = corrupted_ring()
    return nr.refine(c["base"]["track_off"], c["base"]["obs_node"], c["case"]["img_off"], c["kp"], c["case"]["P"], c["base"]["X"], c["base"]["flags"],
                     detail=True)


def test_no_iterations_reproduce_the_triangulation_word_for_word():
    c = corrupted_ring()
    b = c["base"]
    out = nr.refine(b["track_off"], b["obs_node"], c["case"]["img_off"], c["kp"], c["case"]["P"], b["X"], b["flags"], iters=0, iters2=0)
    assert np.array_equal(out[0].view(np.uint32), b["X"].view(np.uint32)) and not out[7].any()
    assert np.array_equal(out[2].view(np.uint32), b["err"].view(np.uint32)) and np.array_equal(out[3].view(np.uint32), b["depth"].view(np.uint32))
    assert np.array_equal(out[1] != 0, b["err"] <= 2.0)                                          # float32 errors of 2 px sit far from the bound


def test_the_restatement_reaches_the_cost_scipy_reaches():
    """Phase 1 alone against scipy.optimize.minimize on a Huber cost written here, from the same DLT start, 50 corrupted tracks."""
    from scipy.optimize import minimize
    c = corrupted_ring()
    b, P, off = c["base"], c["case"]["P"].reshape(-1, 3, 4), c["case"]["img_off"]
    cost1 = refined_ring()[9]
    worst = -np.inf
    for t in c["bad"][:50]:
        nodes = b["obs_node"][b["track_off"][t]:b["track_off"][t + 1]]
        Pt, z = P[nt.image_of(off, nodes)], c["kp"][nodes].astype(np.float64)

        def huber_cost(x):
            h = Pt @ np.r_[x, 1.0]
            e = np.linalg.norm(h[:, :2] / h[:, 2:] - z, axis=1)
            return float(np.where(e <= 1.0, 0.5 * e ** 2, e - 0.5).sum())

        first = minimize(huber_cost, b["X"][t].astype(np.float64), method="BFGS", options=dict(gtol=1e-12))
        best = minimize(huber_cost, first.x, method="Nelder-Mead", options=dict(xatol=1e-13, fatol=1e-15, maxiter=4000))
        low = min(first.fun, best.fun)
        assert cost1[t] <= low * (1.0 + SCIPY_MARGIN), (t, cost1[t], low)
        worst = max(worst, cost1[t] / low - 1.0)
    print(f"phase-1 Huber cost against scipy on 50 corrupted tracks: largest cost / scipy - 1 = {worst:.3e} (bound {SCIPY_MARGIN:.1e})")


def test_calibration_on_the_corrupted_ring_scene():
    c = corrupted_ring()
    b, case = c["base"], c["case"]
    X, inl, err, depth, n_inl, worst, cosm, steps, flags = refined_ring()[:9]
    assert len(c["bad"]) == 107 and len(b["X"]) == 400 and len(inl) == 3200
    planted = np.zeros(len(inl), bool)
    planted[c["rows"]] = True
    flagged_clean = int((inl[~planted] == 0).sum())
    assert not inl[planted].any(), "a planted outlier was not flagged"
    assert (~planted).sum() == 3093 and flagged_clean <= 3, flagged_clean
    # max_reproj = 2 drops every corrupted track whole; the prune keeps all 400 and drops the 107 observations
    plain = nt.run(case["store"], case["nq"], case["pairs"], case["img_off"], c["kp"], case["P"], max_reproj=2.0)
    off2, obs2, X2, src, c2 = nr.prune(b["track_off"], b["obs_node"], X, inl, n_inl, worst, cosm, flags, 2, 2.0)
    assert len(plain["points"]) == 400 - 107 and c2.tolist() == [400, 3200 - 107 - flagged_clean, 0, 107 + flagged_clean]
    bad = c["bad"]
    dist = lambda Y: float(np.median(np.linalg.norm(Y[bad].astype(np.float64) - c["truth"][bad], axis=1)))  # noqa: E731
    e_dlt, e_ref = dist(b["X"]), dist(X)
    # the same tracks triangulated without their planted observation
    keep = ~planted
    tr = np.repeat(np.arange(400), np.diff(b["track_off"]))
    off7 = np.concatenate([[0], np.cumsum(np.bincount(tr[keep], minlength=400))])
    e_without = dist(nt.triangulate(off7, b["obs_node"][keep], case["img_off"], c["kp"], case["P"])[0])
    print(f"corrupted ring: 107 tracks, median distance DLT {e_dlt:.5f} refined {e_ref:.5f} (r = {e_ref / e_dlt:.4f}, bar {REFINE_BAR:.4f}); without the "
          f"planted observation {e_without:.5f} (ratio {e_ref / e_without:.3f}, bar {CLEAN_BAR:.3f}); clean observations flagged {flagged_clean}; "
          f"steps up to {steps.max()}, smallest cosine {cosm.min():.4f} .. {cosm.max():.4f}")
    assert e_ref <= REFINE_BAR * e_dlt, (e_ref, e_dlt)
    assert e_ref <= CLEAN_BAR * e_without, (e_ref, e_without)
