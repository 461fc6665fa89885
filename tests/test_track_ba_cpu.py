"""The TRACKS-BA family without a GPU (include/sfm_hip.h, "TRACKS-BA"; docs/tracks.md §9): the C-ABI declares, binds, documents and
validates the entry points; the restatement tests/np_track_ba.py stands apart from the product, agrees with np_ba at huber = inf,
gives hand-checked results on small problems, reaches the cost SciPy's minimiser reaches, and meets the calibration bars on the
corrupted ring scene."""
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

import np_ba  # noqa: E402
import np_track_ba as nb  # noqa: E402
import np_tracks as nt  # noqa: E402
from test_tracks_refine_cpu import K, corrupted_ring, crossing_case  # noqa: E402

NEW_SYMBOLS = ("sfm_track_ba_ws_bytes", "sfm_track_ba_sweep", "sfm_track_ba_product", "sfm_track_ba_step")

# Measured here with the restatement (docs/tracks.md §9.3).
# The corrupted ring scene (corrupted_ring()["base"], all 3 200 observations, one keypoint of 107 tracks displaced by 20 to 100 px), the
# cameras ring_cameras(8) * (1 + 0.002 * default_rng(4).standard_normal((8, 6))), iters = 15, camera 0 fixed.  Median camera-centre
# error after the similarity alignment to ring_cameras(8): start 0.01741; plain least squares 0.14303 (5 iterations, cost 347 738 ->
# 341 742: worse than the start); Huber 1 px 0.004904 (7 iterations, robust cost 22 663 -> 13 010): r = 0.0343.  The bar is (1 + r) / 2.
BA_RATIO = 0.0343
BA_BAR = (1.0 + BA_RATIO) / 2.0
# The Huber cost (1 px) the restatement's LM ends at against scipy.optimize.minimize (L-BFGS-B, then Powell from its point) on a cost
# written here, from the same start: 3 cameras, 20 points, 5 displaced observations, camera 0 fixed.  The LM stops by its own rule
# (relative gain below 1e-9) after 54 iterations at 346.091945078; SciPy reaches 346.091943957 in both stages: cost / scipy - 1 =
# 3.241e-09, the size of the stopping rule.  The bound is 4 x that.
SCIPY_MARGIN = 1.3e-8


def test_header_declares_binds_and_documents_the_entry_points():
    from sfm_mvs_amd import _lib
    from test_abi import declared_symbols
    syms = declared_symbols()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    doc = open(os.path.join(ROOT, "docs", "tracks.md")).read()
    header = open(os.path.join(ROOT, "include", "sfm_hip.h")).read()
    assert "TRACKS-BA" in header and "NO FLOATING-POINT ATOMICS" in header and "2 * huber * e - huber * huber" in header
    for s in NEW_SYMBOLS:
        assert s in syms and s in _lib.SIGNATURES and hasattr(handle, s), s
        assert s in doc, f"docs/tracks.md does not mention {s}"
    assert _lib.lib().sfm_abi_version() == 3 and _lib.ABI_VERSION == 3
    assert "tracks_ba.hip" in _lib.code_hashes_of_binary()
    src = open(os.path.join(ROOT, "sfm_mvs_amd", "csrc", "tracks_ba.hip")).read()
    assert "atomicAdd" not in src and "unsafeAtomic" not in src                                     # the summation-order contract


def test_python_layer_exposes_the_entry_points():
    import inspect
    from sfm_mvs_amd import track_ba, tracks
    sig = inspect.signature(track_ba.bundle_adjust_tracks).parameters
    assert list(sig) == ["cams", "K", "X", "obs", "cam_idx", "pt_idx", "huber", "iters", "lam", "fix_first_camera", "cg_tol", "cg_iters", "log"]
    assert [sig[k].default for k in list(sig)[6:]] == [None, 10, 1e-3, True, 1e-10, 200, None]
    for name in ("plan", "sweep", "product", "step", "cams_from_P", "P_from_cams"):
        assert callable(getattr(track_ba, name)), name
    assert list(inspect.signature(tracks.adjust_tracks).parameters)[:3] == ["result", "P", "K"]
    # cams_from_P / P_from_cams are each other's inverse on cameras K [R | t] (host code of the library: no GPU)
    from datagen import ring_cameras
    cams = ring_cameras(5)
    P = track_ba.P_from_cams(cams, K)
    assert P.shape == (5, 3, 4) and np.abs(track_ba.cams_from_P(P, K) - cams).max() < 1e-12
    R = np_ba.rotation(cams[:, :3])
    assert np.abs(P - np.einsum("ab,ibc->iac", K, np.concatenate([R, cams[:, 3:, None]], 2))).max() < 1e-9


def test_argument_errors_are_reported_before_the_device():
    """Every argument error of the header: a negative status with its message, before any device call (the pointers are never read)."""
    from sfm_mvs_amd import _lib
    L = _lib.lib()
    f = [ctypes.c_void_p(256 * (k + 1)) for k in range(24)]
    Kh = (ctypes.c_double * 9)(900, 0, 480, 0, 900, 320, 0, 0, 1)
    it, st = ctypes.c_int32(0), ctypes.c_int32(0)
    big, nan = 1 << 31, float("nan")

    def sweep(cams=f[0], ncam=4, K=ctypes.cast(Kh, ctypes.c_void_p), X=f[1], npt=10, obs=f[2], to=f[3], ci=f[4], pi=f[5], co=f[6], cob=f[7], nobs=30,
              huber=1.0, mode=0, act=f[8], B=f[9], gc=f[10], C=f[11], gp=f[12], stat=f[13], cnt=f[14], ws=f[15], wsb=1 << 24):
        return L.sfm_track_ba_sweep(cams, ncam, K, X, npt, obs, to, ci, pi, co, cob, nobs, huber, mode, act, B, gc, C, gp, stat, cnt, ws, wsb, None)

    def product(ncam=4, npt=10, to=f[3], ci=f[4], pi=f[5], co=f[6], cob=f[7], nobs=30, mode=0, vin=f[8], vout=f[9], ws=f[15], wsb=1 << 24):
        return L.sfm_track_ba_product(ncam, npt, to, ci, pi, co, cob, nobs, mode, vin, vout, ws, wsb, None)

    def step(ncam=4, npt=10, to=f[3], ci=f[4], pi=f[5], co=f[6], cob=f[7], nobs=30, B=f[9], gc=f[10], C=f[11], gp=f[12], lam=1e-3, fix=1, tol=1e-10,
             iters=200, dc=f[13], dp=f[14], ws=f[15], wsb=1 << 24):
        return L.sfm_track_ba_step(ncam, npt, to, ci, pi, co, cob, nobs, B, gc, C, gp, lam, fix, tol, iters, dc, dp, ctypes.byref(it), ctypes.byref(st),
                                   ws, wsb, None)

    sizes = [(dict(ncam=0), b"sizes"), (dict(ncam=1 << 24), b"sizes"), (dict(npt=0), b"sizes"), (dict(npt=big), b"sizes"), (dict(nobs=-1), b"sizes"),
             (dict(nobs=big), b"sizes")]
    csr = [({k: None}, b"null") for k in ("to", "ci", "pi", "co", "cob")]
    cases = [(call, kw, msg, -1) for call in (sweep, product, step) for kw, msg in sizes + csr]
    cases += [(call, dict(wsb=64), b"workspace", -2) for call in (sweep, product, step)] + [(call, dict(ws=None), b"workspace", -2) for call in (sweep, product, step)]
    cases += [(sweep, dict(mode=2), b"mode", -1), (sweep, dict(mode=-1), b"mode", -1), (sweep, dict(huber=nan), b"huber", -1), (sweep, dict(huber=0.0), b"huber", -1),
              (sweep, dict(huber=-1.0), b"huber", -1)]
    cases += [(sweep, {k: None}, b"null", -1) for k in ("cams", "K", "X", "obs", "act", "B", "gc", "C", "gp", "stat", "cnt")]
    cases += [(sweep, dict(nobs=0, stat=None), b"null", -1), (sweep, dict(nobs=0, to=None), b"null", -1)]
    cases += [(product, dict(mode=2), b"mode", -1), (product, dict(vin=None), b"null", -1), (product, dict(vout=None), b"null", -1)]
    cases += [(step, dict(iters=-1), b"cg_iters", -1), (step, dict(lam=-1.0), b"lam", -1), (step, dict(lam=nan), b"lam", -1), (step, dict(tol=-1.0), b"cg_tol", -1)]
    cases += [(step, {k: None}, b"null", -1) for k in ("B", "gc", "C", "gp", "dc", "dp")]
    for call, kw, msg, rc in cases:
        assert call(**kw) == rc, (call.__name__, kw)
        assert msg in L.sfm_last_error(), (call.__name__, kw, L.sfm_last_error())
    W = L.sfm_track_ba_ws_bytes
    assert W(0, 1, 1) == 0 and W(1 << 24, 1, 1) == 0 and W(1, 0, 1) == 0 and W(1, big, 1) == 0 and W(1, 1, -1) == 0 and W(1, 1, big) == 0
    assert W(1, 1, 0) > 0 and W(64, 7000, 448000) >= 448000 * 160 + (448000 // 256 + 64) * 216


def test_the_restatement_imports_only_numpy_and_np_ba():
    tree = ast.parse(open(os.path.join(ROOT, "tests", "np_track_ba.py")).read())
    for node in ast.walk(tree):
        names = [a.name for a in node.names] if isinstance(node, ast.Import) else [node.module or ""] if isinstance(node, ast.ImportFrom) else []
        assert names in ([], ["numpy"], ["np_ba"]), names


# ---- a small sparse problem -----------------------------------------------------------------------------------------------

def small_problem(ncam=3, npt=20, displaced=5, seed=11, noise=0.3, f32_points=False):
    """Cameras on a ring, points near the origin, every third (camera, point) pair dropped, `displaced` observations moved by 30 px
    -> (cams, X, obs float32, cam_idx, pt_idx), point-major."""
    from datagen import ring_cameras
    rng = np.random.default_rng(seed)
    truth = ring_cameras(max(ncam, 3))[:ncam]
    X = rng.normal(0, 0.6, (npt, 3))
    see = rng.random((npt, ncam)) < 0.7
    see[:, :2] |= ~see.any(1, keepdims=True) | (see.sum(1, keepdims=True) < 2)                          # every point in at least two views
    pt_idx, cam_idx = np.nonzero(see)
    obs = np_ba.project(truth[cam_idx], K, X[pt_idx][:, None, :])[:, 0] + rng.normal(0, noise, (len(pt_idx), 2))
    hit = rng.choice(len(obs), displaced, replace=False)
    obs[hit] += 30.0 * np.sign(rng.normal(size=(displaced, 2)))
    cams = truth * (1 + 0.002 * rng.standard_normal(truth.shape))
    X0 = X + rng.normal(0, 0.01, X.shape)
    if f32_points:
        X0 = X0.astype(np.float32).astype(np.float64)
    return cams, X0, obs.astype(np.float32), cam_idx.astype(np.int32), pt_idx.astype(np.int32)


def linearise(cams, X, obs, ci, pi, huber=np.inf, active=None):
    off, coff, cobs = nb.plan(ci, pi, len(cams), len(X))
    return nb.sweep(cams, K, X, obs, ci, pi, off, coff, cobs, huber, active), (off, coff, cobs)


def test_at_huber_inf_the_blocks_and_the_step_are_np_ba_s():
    cams, X, obs, ci, pi = small_problem(f32_points=True)
    out, _ = linearise(cams, X, obs, ci, pi)
    B, C, gc, gp, res2 = np_ba.indexed_normal_blocks(cams, K, X, obs, ci, pi)
    for got, want in ((out["B"], B), (out["C"], C), (out["gc"], gc), (out["gp"], gp), (out["stat"], np.array([res2, res2]))):
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    assert out["count"].tolist() == [len(obs), 0, 0] and out["active"].all()
    Jc, Jp = np_ba.pair_jacobians(cams, K, X, ci, pi)
    W = np.zeros((len(cams), len(X), 6, 3))
    np.add.at(W, (ci, pi), np.einsum("oka,okb->oab", Jc, Jp))
    assert np.abs(nb.dense_w(out["rows"], ci, pi, len(cams), len(X)) - W).max() <= 1e-12 * np.abs(W).max()
    for fix in (True, False):
        dc, dp, status = nb.step(out["B"], out["C"], out["gc"], out["gp"], W, 1e-3, fix)
        wc, wp = np_ba.solve_direct(B, C, gc, gp, W, 1e-3, fix)
        assert status == 0 and np.abs(dc - wc).max() <= 1e-9 * np.abs(wc).max() and np.abs(dp - wp).max() <= 1e-9 * np.abs(wp).max()
    x, v = np.random.default_rng(1).normal(size=(len(cams), 6)), np.random.default_rng(2).normal(size=(len(X), 3))
    u, w = np_ba.indexed_products(cams, K, X, ci, pi, x, v)
    off, coff, cobs = nb.plan(ci, pi, len(cams), len(X))
    assert np.abs(nb.product(out["rows"], ci, pi, off, coff, cobs, len(cams), len(X), x, 0) - u).max() <= 1e-12 * np.abs(u).max()
    assert np.abs(nb.product(out["rows"], ci, pi, off, coff, cobs, len(cams), len(X), v, 1) - w).max() <= 1e-12 * np.abs(w).max()


# ---- hand-checked cases ---------------------------------------------------------------------------------------------------

def side_by_side():
    """The two cameras of crossing_case() as (rvec, tvec): centres (0, 0, 0) and (1, 0, 0), both looking along z."""
    return np.array([[0, 0, 0, 0, 0, 0], [0, 0, 0, -1.0, 0, 0]])


def test_two_cameras_and_one_point_without_noise_take_no_step():
    cams, X = side_by_side(), np.array([[0.0, 0, 2]])
    obs = np.float32([[480, 320], [30, 320]])                                                          # exact: 900 * (-1 / 2) + 480 = 30
    out, _ = linearise(cams, X, obs, [0, 1], [0, 0], 1.0)
    assert out["stat"].tolist() == [0.0, 0.0] and out["count"].tolist() == [2, 0, 0] and not out["gc"].any() and not out["gp"].any()
    assert abs(out["C"][0, 0, 0] - 2 * 450.0 ** 2) < 1e-6 and abs(out["B"][1, 3, 3] - 450.0 ** 2) < 1e-6                    # d u / d X = fx / Z = 450 in both views
    W = nb.dense_w(out["rows"], [0, 1], [0, 0], 2, 1)
    dc, dp, status = nb.step(out["B"], out["C"], out["gc"], out["gp"], W, 1e-3, True)
    assert not dc.any() and not dp.any()
    c2, X2, hist, info = nb.bundle_adjust(cams, K, X, obs, [0, 1], [0, 0], huber=1.0, iters=3)
    assert hist == [0.0, 0.0] and np.array_equal(c2, cams) and np.array_equal(X2, X)                  # no strictly lower cost: it stops


def test_the_weight_and_the_cost_on_both_sides_of_huber():
    cams, X = side_by_side()[:1], np.array([[0.0, 0, 2]])
    huber = 2.0
    below, above = np.nextafter(np.float32(482.0), np.float32(0)), np.nextafter(np.float32(482.0), np.float32(999))
    rho = []
    for u in (below, np.float32(482.0), above):
        out, _ = linearise(cams, X, np.float32([[u, 320]]), [0], [0], huber)
        e = float(u) - 480.0
        w = 1.0 if e <= huber else huber / e
        assert out["w"].tolist() == [w] and out["count"].tolist() == [1, 0, int(e > huber)]
        assert abs(out["rows"][0, 18] + np.sqrt(w) * e) < 1e-12 and abs(out["rows"][0, 12] - np.sqrt(w) * 450.0) < 1e-12
        assert abs(out["stat"][0] - (e * e if e <= huber else 2 * huber * e - huber * huber)) < 1e-12 and abs(out["stat"][1] - e * e) < 1e-12
        rho.append(out["stat"][0])
    assert rho[0] < rho[1] == 4.0 < rho[2] and rho[2] - rho[0] < 1e-3                                  # continuous at e = huber
    far, _ = linearise(cams, X, np.float32([[580, 320]]), [0], [0], huber)
    assert far["w"].tolist() == [0.02] and far["stat"].tolist() == [2 * 2.0 * 100.0 - 4.0, 10000.0]


def test_an_observation_behind_its_camera_is_inactive_and_its_blocks_lack_it():
    cams, X, obs, ci, pi = small_problem()
    full, _ = linearise(cams, X, obs, ci, pi, 1.0)
    Xb = X.copy()
    o = int(np.flatnonzero(pi == 4)[0])
    C = nb.centres(cams)[ci[o]]
    Xb[4] = C + 1.5 * (C - Xb[4])                                                                      # beyond the centre of that camera
    out, _ = linearise(cams, Xb, obs, ci, pi, 1.0)
    gone = np.flatnonzero(out["active"] == 0)
    assert o in gone and set(pi[gone]) == {4} and not out["rows"][gone].any()
    assert out["count"][0] == len(obs) - len(gone) and out["count"][1] == 0
    keep = np.ones(len(obs), bool)
    keep[gone] = False
    less, _ = linearise(cams, Xb, obs[keep], ci[keep], pi[keep], 1.0)                                   # the same problem without them
    for name in ("B", "C", "gc", "gp", "stat"):
        assert np.abs(out[name] - less[name]).max() <= 1e-12 * np.abs(less[name]).max(), name
    assert np.abs(out["B"] - full["B"]).max() > 1.0


def crossing_problem():
    """crossing_case() as a bundle adjustment: its two cameras, its point started at depth 10 (true depth 2, 450 px of disparity),
    and twelve exact points that hold the second camera in place -> (cams, X, obs, cam_idx, pt_idx)."""
    _, _, _, kp, _, X_in, _ = crossing_case()
    cams = side_by_side()
    rng = np.random.default_rng(5)
    Xs = np.c_[rng.uniform(-1, 1, (12, 2)), rng.uniform(3, 6, 12)]
    X = np.vstack([X_in.astype(np.float64), Xs])
    pi = np.repeat(np.arange(13), 2).astype(np.int32)
    ci = np.tile([0, 1], 13).astype(np.int32)
    obs = np_ba.project(cams[ci], K, X[pi][:, None, :])[:, 0]
    obs[:2] = kp
    return cams, X, obs.astype(np.float32), ci, pi


def test_a_trial_that_crosses_a_camera_plane_is_refused_and_lambda_grows():
    cams, X, obs, ci, pi = crossing_problem()
    c2, X2, hist, info = nb.bundle_adjust(cams, K, X, obs, ci, pi, huber=None, iters=30)
    lams = info["lams"]
    assert info["crossed_refusals"] >= 1 and lams[1] == 4.0 * lams[0], (info["crossed_refusals"], lams[:4])    # the first attempt is refused
    first, _ = linearise(cams, X, obs, ci, pi)
    dc, dp, _ = nb.step(first["B"], first["C"], first["gc"], first["gp"], nb.dense_w(first["rows"], ci, pi, 2, 13), 1e-3, True)
    trial, _ = linearise(cams - dc, X - dp, obs, ci, pi, np.inf, first["active"])
    assert (X - dp)[0, 2] < 0 and trial["count"][1] == 2 and trial["count"][0] == len(obs) - 2          # behind both cameras
    assert all(b <= a for a, b in zip(hist, hist[1:])) and hist[-1] < 1e-6 * hist[0] and info["active"] == 26
    assert abs(X2[0, 2] / np.linalg.norm(nb.centres(c2)[1] - nb.centres(c2)[0]) - 2.0) < 1e-3        # depth 2 in units of the baseline (the scale is free)
    print(f"crossing problem: {info['crossed_refusals']} attempts refused for crossing, cost {hist[0]:.4g} -> {hist[-1]:.3g} in {len(hist) - 1} iterations")


def test_a_camera_without_observations_and_a_point_with_all_observations_inactive():
    cams, X, obs, ci, pi = small_problem()
    cams4 = np.vstack([cams, cams[:1] + 0.1])                                                            # camera 3 sees nothing
    Xn = np.vstack([X, [[np.nan, 0, 0]]])                                                              # point 20: every observation inactive
    ci2, pi2 = np.r_[ci, [0, 1]].astype(np.int32), np.r_[pi, [20, 20]].astype(np.int32)
    obs2 = np.vstack([obs, np.float32([[1, 2], [3, 4]])])
    out, _ = linearise(cams4, Xn, obs2, ci2, pi2, 1.0)
    ref, _ = linearise(cams, X, obs, ci, pi, 1.0)
    assert not out["B"][3].any() and not out["gc"][3].any() and not out["C"][20].any() and not out["gp"][20].any()
    assert out["active"][-2:].tolist() == [0, 0] and out["count"].tolist() == ref["count"].tolist()
    for name, sl in (("B", slice(0, 3)), ("C", slice(0, 20)), ("gc", slice(0, 3)), ("gp", slice(0, 20))):
        assert np.array_equal(out[name][sl], ref[name])
    W = nb.dense_w(out["rows"], ci2, pi2, 4, 21)
    dc, dp, status = nb.step(out["B"], out["C"], out["gc"], out["gp"], W, 1e-3, True)
    wc, wp, _ = nb.step(ref["B"], ref["C"], ref["gc"], ref["gp"], nb.dense_w(ref["rows"], ci, pi, 3, 20), 1e-3, True)
    assert status == 3 and not dc[3].any() and not dp[20].any() and np.isfinite(dc).all() and np.isfinite(dp).all()
    assert np.abs(dc[:3] - wc).max() <= 1e-9 * np.abs(wc).max() and np.abs(dp[:20] - wp).max() <= 1e-9 * np.abs(wp).max()
    # and through the loop: the extra camera and point stay where they are, the rest moves as without them
    c2, X2, hist, _ = nb.bundle_adjust(cams4, K, Xn, obs2, ci2, pi2, huber=1.0, iters=4)
    c1, X1, hist1, _ = nb.bundle_adjust(cams, K, X, obs, ci, pi, huber=1.0, iters=4)
    assert np.array_equal(c2[3], cams4[3]) and np.isnan(X2[20, 0]) and np.allclose(hist, hist1, rtol=1e-9) and np.allclose(c2[:3], c1, atol=1e-9)


def test_the_restatement_reaches_the_cost_scipy_reaches():
    from scipy.optimize import minimize
    cams, X, obs, ci, pi = small_problem()
    c2, X2, hist, info = nb.bundle_adjust(cams, K, X, obs, ci, pi, huber=1.0, iters=100)
    o64 = obs.astype(np.float64)

    def huber_cost(p):
        c = np.vstack([cams[:1], p[:12].reshape(2, 6)])                                                  # camera 0 fixed, as in the LM
        e = np.linalg.norm(np_ba.project(c[ci], K, p[12:].reshape(-1, 3)[pi][:, None, :])[:, 0] - o64, axis=1)
        return float(np.where(e <= 1.0, e * e, 2.0 * e - 1.0).sum())

    p0 = np.r_[cams[1:].ravel(), X.ravel()]
    assert abs(huber_cost(p0) - hist[0]) <= 1e-9 * hist[0] and abs(huber_cost(np.r_[c2[1:].ravel(), X2.ravel()]) - hist[-1]) <= 1e-9 * hist[-1]
    first = minimize(huber_cost, p0, method="L-BFGS-B", options=dict(maxiter=20000, maxfun=2000000, ftol=1e-16, gtol=1e-10))
    best = minimize(huber_cost, first.x, method="Powell", options=dict(xtol=1e-10, ftol=1e-14, maxiter=200))
    low = min(first.fun, best.fun)
    print(f"Huber LM against scipy: LM {hist[-1]:.12g} after {len(hist) - 1} iterations ({info['outliers']} outliers), scipy {first.fun:.12g} / {best.fun:.12g}; "
          f"cost / scipy - 1 = {hist[-1] / low - 1:.3e} (bound {SCIPY_MARGIN:.1e})")
    assert info["outliers"] >= 5 and hist[-1] < hist[0] and len(hist) - 1 < 100                            # it stopped by its own rule
    assert hist[-1] <= low * (1.0 + SCIPY_MARGIN), (hist[-1], low)


def test_pcg_distance_from_the_direct_solve():
    """How far the reference PCG ends from the direct solve on the shapes of the GPU step test: the figures track_ba_cases records,
    which bound what the device is allowed (PCG_ALLOW times them)."""
    import track_ba_cases as tc
    for ncam in tc.PCG_CAMS:
        B, C, gc, gp, W = tc.host_step_inputs(tc.step_problem(ncam))
        for fix in (True, False):
            wc, wp = np_ba.solve_direct(B, C, gc, gp, W, tc.PCG_LAM, fix)
            dc, dp, it = np_ba.solve_pcg(B, C, gc, gp, W, tc.PCG_LAM, fix, tol=tc.PCG_TOL, iters=tc.PCG_ITERS)
            fig = (tc.rel(dc, wc), tc.rel(dp, wp))
            print(f"ncam {ncam} fix_first={fix}: {it} iterations, dc {fig[0]:.2e} dp {fig[1]:.2e} (recorded {tc.PCG_FIGURES[(ncam, fix)]})")
            assert 0 < it < tc.PCG_ITERS and it % 5 == 0
            for f, rec in zip(fig, tc.PCG_FIGURES[(ncam, fix)]):
                assert 0.1 * rec < f <= rec, (ncam, fix, fig)


# ---- the calibration on the corrupted ring scene ----------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def ring_problem():
    """-> dict: the BA input of corrupted_ring()["base"] (all 3 200 observations), the perturbed cameras of the GPU tests, the clean rows."""
    from datagen import ring_cameras
    c = corrupted_ring()
    b, case = c["base"], c["case"]
    planted = np.zeros(len(b["obs_node"]), bool)
    planted[c["rows"]] = True
    truth = ring_cameras(8)
    return dict(K=case["K"], truth=truth, cams=truth * (1 + 0.002 * np.random.default_rng(4).standard_normal((8, 6))), X=b["X"].astype(np.float64),
                obs=c["kp"][b["obs_node"]], cam_idx=nt.image_of(case["img_off"], b["obs_node"]).astype(np.int32),
                pt_idx=np.repeat(np.arange(len(b["X"])), np.diff(b["track_off"])).astype(np.int32), clean=np.flatnonzero(~planted))


def calibration_figures(p, adjust):
    """adjust(huber) -> (cams, X): (median centre error L2, Huber, clean rms at the start, under Huber)."""
    centre = lambda c: float(np.median(nb.aligned_centre_errors(c, p["truth"])))  # noqa: E731
    rms = lambda c, X: nb.rms_error(c, p["K"], X, p["obs"], p["cam_idx"], p["pt_idx"], p["clean"])  # noqa: E731
    c_l2, _ = adjust(None)
    c_h, X_h = adjust(1.0)
    return centre(c_l2), centre(c_h), rms(p["cams"], p["X"]), rms(c_h, X_h), centre(p["cams"])


def test_calibration_on_the_corrupted_ring_scene():
    p = ring_problem()
    assert len(p["obs"]) == 3200 and len(p["clean"]) == 3093 and len(p["X"]) == 400
    e_l2, e_h, rms0, rms_h, e0 = calibration_figures(p, lambda h: nb.bundle_adjust(p["cams"], p["K"], p["X"], p["obs"], p["cam_idx"], p["pt_idx"], huber=h, iters=15)[:2])
    print(f"corrupted ring BA: median camera-centre error start {e0:.5f}, L2 {e_l2:.5f}, Huber {e_h:.6f} (r = {e_h / e_l2:.4f}, bar {BA_BAR:.4f}); "
          f"clean rms start {rms0:.3f} px, Huber {rms_h:.3f} px")
    assert e_h <= BA_BAR * e_l2, (e_h, e_l2)
    assert rms_h < rms0, (rms_h, rms0)
