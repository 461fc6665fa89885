"""The TRACKS-CAL family without a GPU (include/sfm_hip.h, "TRACKS-CAL"; docs/tracks.md §15): the C-ABI declares, binds, documents and
validates the entry points; the restatement tests/np_track_cal.py stands apart from the product, has the Jacobians of its own
projection, is np_track_ba's with nothing free and no distortion, reaches the cost SciPy reaches, inverts its own forward model, and
meets the calibration bars of tests/golden/track_cal_calibration.json."""
import ast
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import np_track_ba as nb  # noqa: E402
import np_track_cal as nc  # noqa: E402
import track_cal_cases as cc  # noqa: E402
from test_track_ba_cpu import small_problem  # noqa: E402

K = cc.K
NEW_SYMBOLS = ("sfm_track_cal_ws_bytes", "sfm_track_cal_sweep", "sfm_track_cal_product", "sfm_track_cal_step", "sfm_undistort_points",
               "sfm_undistort_image")

# Central differences of np_track_cal.project against its complex-step Jacobians on the observations of cal_problem() at theta =
# (900, 480, 320, -0.12, 0.03), a = 1.1: step 1e-5 (times max(1, |theta_k|) for theta), largest difference over the largest entry of
# the Jacobian (of the column, for theta, whose columns differ by five orders) 1.6e-8; 1e-6 gives 1.3e-7, 1e-7 gives 1.3e-6
# (rounding takes over).  The bound is 1e-7.
FD_STEP, FD_BOUND = 1e-5, 1e-7
# The plain least-squares cost the restatement's LM ends at with (f, k1) free against scipy.optimize.least_squares (trf, x_scale
# "jac", all tolerances 1e-15) on residuals written here, from the same start: cal_problem(), 3 cameras, 60 points, camera 0 fixed,
# start f = 1000, k1 = 0 (planted 900, -0.12).  The LM stops by its own rule (relative gain below 1e-9) after 6 iterations at
# 9.09309701353832 (f = 899.9452, k1 = -0.118177); SciPy ends at 9.093097013538253 after 36 evaluations: cost / scipy - 1 = 7.3e-15.
# The bound is the stopping rule's 1e-9.
SCIPY_MARGIN = 1e-9
# undistort_points(float32(distort(p))) against p over a 97 x 65 grid of the 960 x 640 frame (f = 900), k1 in {-0.3, -0.12, 0, 0.12,
# 0.3}, k2 in {0, 0.03}: at most 6.1e-5 px = one float32 spacing at 512..1024 px.  The input is rounded to float32 (half a spacing,
# carried through an inverse map whose derivative stays below 1.6 on this frame), the output once more (half a spacing): 1.3
# spacings at the most.  The bound is two spacings; the ten Newton steps leave nothing visible at this scale.
INVERSE_BOUND = 2 * 2.0 ** -14


def test_header_declares_binds_and_documents_the_entry_points():
    from sfm_mvs_amd import _lib
    from test_abi import declared_symbols
    syms = declared_symbols()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    doc = open(os.path.join(ROOT, "docs", "tracks.md")).read()
    header = open(os.path.join(ROOT, "include", "sfm_hip.h")).read()
    assert "TRACKS-CAL" in header and "NO FLOATING-POINT ATOMICS in csrc/tracks_cal.hip" in header and "u = f*d*x + cx" in header
    for s in NEW_SYMBOLS:
        assert s in syms and s in _lib.SIGNATURES and hasattr(handle, s), s
        assert s in doc, f"docs/tracks.md does not mention {s}"
    assert "## 15." in doc and "tracks_cal.hip" in open(os.path.join(ROOT, "README.md")).read() and "tracks_cal.hip" in open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "tracks_cal.hip" in _lib.code_hashes_of_binary()
    src = open(os.path.join(ROOT, "sfm_mvs_amd", "csrc", "tracks_cal.hip")).read()
    assert "atomicAdd" not in src and "unsafeAtomic" not in src                                     # the summation-order contract
    assert "#pragma clang fp" not in src                                                            # contraction stays off: the undistortions are held to the bit
    # tracks_ba.hip is the parent's: the family is a sibling, not an edit
    assert "tcal" not in open(os.path.join(ROOT, "sfm_mvs_amd", "csrc", "tracks_ba.hip")).read()


def test_python_layer_exposes_the_entry_points():
    import inspect
    from sfm_mvs_amd import register, track_ba, track_cal, tracks
    sig = inspect.signature(track_cal.bundle_adjust_calibrated).parameters
    assert list(sig) == ["cams", "K", "dist", "X", "obs", "cam_idx", "pt_idx", "free", "huber", "iters", "lam", "fix_first_camera", "cg_tol", "cg_iters", "log"]
    assert [sig[k].default for k in list(sig)[7:]] == [("f", "k1"), None, 10, 1e-3, True, 1e-10, 200, None]
    for name in ("sweep", "product", "step", "rows_of", "undistort_points", "undistort_images"):
        assert callable(getattr(track_cal, name)), name
    assert track_cal.plan is track_ba.plan and track_cal.Plan is track_ba.Plan
    assert inspect.signature(tracks.adjust_tracks).parameters["calibrate"].default is None
    assert inspect.signature(tracks.densify_tracks).parameters["dist"].default is None
    assert inspect.signature(register.register_tracks).parameters["calibrate"].default is None
    assert track_cal.free_mask(("f", "k1")) == 9 and track_cal.free_mask(()) == 0 and track_cal.free_mask(track_cal.NAMES) == 31 and track_cal.free_mask(17) == 17
    for bad in (("fx",), 32, -1):
        with pytest.raises(track_cal.SfmHipError):
            track_cal.free_mask(bad)
    theta, a = track_cal.theta_of([[900, 0, 480], [0, 1350, 320], [0, 0, 1]], (-0.1, 0.02))                  # a = 1.5: a * f is exact
    assert theta.tolist() == [900.0, 480.0, 320.0, -0.1, 0.02] and a == 1.5 and np.array_equal(track_cal.K_of(theta, a), [[900, 0, 480], [0, 1350, 320], [0, 0, 1]])


def test_argument_errors_are_reported_before_the_device():
    """Every argument error of the header: a negative status with its message, before any device call (the pointers are never read)."""
    from sfm_mvs_amd import _lib
    L = _lib.lib()
    f = [ctypes.c_void_p(256 * (k + 1)) for k in range(32)]
    it, st = ctypes.c_int32(0), ctypes.c_int32(0)
    big, nan, inf = 1 << 31, float("nan"), float("inf")

    def vec(*v):
        arr = (ctypes.c_double * len(v))(*v)
        return ctypes.cast(arr, ctypes.c_void_p), arr

    good, keep = vec(900, 480, 320, -0.1, 0.01)
    Kout, keep2 = vec(900, 0, 480, 0, 900, 320, 0, 0, 1)

    def sweep(cams=f[0], ncam=4, theta=good, a=1.0, dth=None, X=f[1], npt=10, obs=f[2], to=f[3], ci=f[4], pi=f[5], co=f[6], cob=f[7], nobs=30,
              huber=1.0, mode=0, act=f[8], B=f[9], gc=f[10], C=f[11], gp=f[12], E=f[16], G=f[17], gi=f[18], F=f[19], stat=f[13], cnt=f[14], ws=f[15],
              wsb=1 << 24):
        return L.sfm_track_cal_sweep(cams, ncam, theta, a, dth, X, npt, obs, to, ci, pi, co, cob, nobs, huber, mode, act, B, gc, C, gp, E, G, gi, F,
                                     stat, cnt, ws, wsb, None)

    def product(ncam=4, npt=10, to=f[3], ci=f[4], pi=f[5], co=f[6], cob=f[7], nobs=30, mode=0, vin=f[8], vth=f[20], vout=f[9], oth=f[21], ws=f[15],
                wsb=1 << 24):
        return L.sfm_track_cal_product(ncam, npt, to, ci, pi, co, cob, nobs, mode, vin, vth, vout, oth, ws, wsb, None)

    def step(ncam=4, npt=10, to=f[3], ci=f[4], pi=f[5], co=f[6], cob=f[7], nobs=30, B=f[9], gc=f[10], C=f[11], gp=f[12], E=f[16], G=f[17], gi=f[18],
             lam=1e-3, free=9, fix=1, tol=1e-10, iters=200, dc=f[13], di=f[22], dp=f[14], ws=f[15], wsb=1 << 24):
        return L.sfm_track_cal_step(ncam, npt, to, ci, pi, co, cob, nobs, B, gc, C, gp, E, G, gi, lam, free, fix, tol, iters, dc, di, dp,
                                    ctypes.byref(it), ctypes.byref(st), ws, wsb, None)

    def points(px=f[0], n=10, theta=good, a=1.0, Ko=Kout, out=f[1]):
        return L.sfm_undistort_points(px, n, theta, a, Ko, out, None)

    def image(src=f[0], n=2, H=48, W=64, C=3, theta=good, a=1.0, Ko=Kout, dst=f[1], mask=None):
        return L.sfm_undistort_image(src, n, H, W, C, theta, a, Ko, dst, mask, None)

    sizes = [(dict(ncam=0), b"sizes"), (dict(ncam=1 << 24), b"sizes"), (dict(npt=0), b"sizes"), (dict(npt=big), b"sizes"), (dict(nobs=-1), b"sizes"),
             (dict(nobs=big), b"sizes")]
    csr = [({k: None}, b"null") for k in ("to", "ci", "pi", "co", "cob")]
    cases = [(call, kw, msg, -1) for call in (sweep, product, step) for kw, msg in sizes + csr]
    cases += [(call, dict(wsb=64), b"workspace", -2) for call in (sweep, product, step)] + [(call, dict(ws=None), b"workspace", -2) for call in (sweep, product, step)]
    cases += [(sweep, dict(mode=2), b"mode", -1), (sweep, dict(mode=-1), b"mode", -1), (sweep, dict(huber=nan), b"huber", -1), (sweep, dict(huber=0.0), b"huber", -1),
              (sweep, dict(huber=-1.0), b"huber", -1)]
    cases += [(sweep, {k: None}, b"null", -1) for k in ("cams", "theta", "X", "obs", "act", "B", "gc", "C", "gp", "E", "G", "gi", "F", "stat", "cnt")]
    cases += [(sweep, dict(nobs=0, stat=None), b"null", -1), (sweep, dict(nobs=0, to=None), b"null", -1)]
    # theta not finite, f <= 0, a <= 0: in every entry point that takes them
    for call in (sweep, points, image):
        for k in range(5):
            for v in (nan, inf, -inf):
                t = [900, 480, 320, -0.1, 0.01]
                t[k] = v
                th, _k = vec(*t)
                cases.append((call, dict(theta=th, _keep=_k), b"not finite", -1))
        for fv in (0.0, -900.0):
            th, _k = vec(fv, 480, 320, 0, 0)
            cases.append((call, dict(theta=th, _keep=_k), b"focal", -1))
        cases += [(call, dict(a=v), b"aspect", -1) for v in (0.0, -1.0, nan, inf)]
    cases += [(product, dict(mode=2), b"mode", -1), (product, dict(vin=None), b"null", -1), (product, dict(vout=None), b"null", -1),
              (product, dict(mode=0, vth=None), b"null", -1), (product, dict(mode=1, oth=None), b"null", -1)]
    cases += [(step, dict(iters=-1), b"cg_iters", -1), (step, dict(lam=-1.0), b"lam", -1), (step, dict(lam=nan), b"lam", -1), (step, dict(tol=-1.0), b"cg_tol", -1),
              (step, dict(free=32), b"free", -1), (step, dict(free=-1), b"free", -1)]
    cases += [(step, {k: None}, b"null", -1) for k in ("B", "gc", "C", "gp", "E", "G", "gi", "dc", "di", "dp")]
    bad_k, _k2 = vec(900, 0, 480, 0, -900, 320, 0, 0, 1)
    nan_k, _k3 = vec(nan, 0, 480, 0, 900, 320, 0, 0, 1)
    cases += [(points, dict(n=-1), b"outside", -1), (points, dict(n=big), b"outside", -1), (points, dict(px=None), b"null", -1), (points, dict(out=None), b"null", -1),
              (points, dict(Ko=None), b"K_out", -1), (points, dict(Ko=bad_k), b"K_out", -1), (points, dict(Ko=nan_k), b"K_out", -1)]
    cases += [(image, dict(n=-1), b"sizes", -1), (image, dict(n=65536), b"sizes", -1), (image, dict(H=0), b"sizes", -1), (image, dict(W=0), b"sizes", -1),
              (image, dict(W=65537), b"sizes", -1), (image, dict(C=2), b"channels", -1), (image, dict(C=4), b"channels", -1), (image, dict(src=None), b"null", -1),
              (image, dict(dst=None), b"null", -1), (image, dict(dst=f[0]), b"same buffer", -1), (image, dict(Ko=None), b"K_out", -1), (image, dict(Ko=bad_k), b"K_out", -1)]
    for call, kw, msg, rc in cases:
        kw = {k: v for k, v in kw.items() if k != "_keep"}
        assert call(**kw) == rc, (call.__name__, kw)
        assert msg in L.sfm_last_error(), (call.__name__, kw, L.sfm_last_error())
    assert points(n=0, px=None, out=None) == 0 and image(n=0, src=None, dst=None) == 0             # nothing to do: no device call either
    W = L.sfm_track_cal_ws_bytes
    assert W(0, 1, 1) == 0 and W(1 << 24, 1, 1) == 0 and W(1, 0, 1) == 0 and W(1, big, 1) == 0 and W(1, 1, -1) == 0 and W(1, 1, big) == 0
    assert W(1, 1, 0) > 0 and W(64, 7000, 448000) >= 448000 * 240 + (448000 // 256 + 64) * 456
    assert W(64, 7000, 448000) > L.sfm_track_ba_ws_bytes(64, 7000, 448000)


def test_the_restatement_imports_only_numpy_np_ba_and_np_track_ba():
    tree = ast.parse(open(os.path.join(ROOT, "tests", "np_track_cal.py")).read())
    for node in ast.walk(tree):
        names = [a.name for a in node.names] if isinstance(node, ast.Import) else [node.module or ""] if isinstance(node, ast.ImportFrom) else []
        assert names in ([], ["numpy"], ["np_ba"], ["np_track_ba"]), names


# ---- a small problem with planted intrinsics --------------------------------------------------------------------------------

def cal_problem(ncam=3, npt=60, seed=3):
    """3 cameras of datagen.ring_cameras, 60 points in a cube of side 3, four fifths of the pairs observed, 0.3 px of noise, planted
    f = 900 and k1 = -0.12 -> (cams, K with the nominal f = 1000, X, obs, cam_idx, pt_idx)."""
    from datagen import ring_cameras
    rng = np.random.default_rng(seed)
    truth = ring_cameras(ncam)
    Xt = rng.uniform(-1.5, 1.5, (npt, 3))
    see = rng.random((npt, ncam)) < 0.8
    see[:, :2] |= see.sum(1, keepdims=True) < 2
    pi, ci = np.nonzero(see)
    obs = (nc.project(truth[ci], np.array([900.0, 480, 320, -0.12, 0.0]), 1.0, Xt[pi]) + rng.normal(0, 0.3, (len(pi), 2))).astype(np.float32)
    cams = truth * (1 + 0.002 * rng.standard_normal(truth.shape))
    X0 = Xt + rng.normal(0, 0.01, Xt.shape)
    return cams, np.array([[1000.0, 0, 480], [0, 1000.0, 320], [0, 0, 1]]), X0, obs, ci.astype(np.int32), pi.astype(np.int32)


def test_the_jacobians_agree_with_central_differences_of_the_projection():
    cams, _, X, _, ci, pi = cal_problem()
    theta, a = np.array([900.0, 480, 320, -0.12, 0.03]), 1.1
    c, x = cams[ci], X[pi]
    Jc, Ji, Jp = nc.jacobians(c, theta, a, x)
    worst = 0.0
    for k in range(6):
        d = np.zeros(6)
        d[k] = FD_STEP
        worst = max(worst, np.abs((nc.project(c + d, theta, a, x) - nc.project(c - d, theta, a, x)) / (2 * FD_STEP) - Jc[..., k]).max() / np.abs(Jc).max())
    for k in range(5):
        h = FD_STEP * max(1.0, abs(theta[k]))
        d = np.zeros(5)
        d[k] = h
        worst = max(worst, np.abs((nc.project(c, theta + d, a, x) - nc.project(c, theta - d, a, x)) / (2 * h) - Ji[..., k]).max() / np.abs(Ji[..., k]).max())
    for k in range(3):
        d = np.zeros(3)
        d[k] = FD_STEP
        worst = max(worst, np.abs((nc.project(c, theta, a, x + d) - nc.project(c, theta, a, x - d)) / (2 * FD_STEP) - Jp[..., k]).max() / np.abs(Jp).max())
    print(f"central differences, step {FD_STEP:g}: largest relative difference {worst:.3g} (bound {FD_BOUND:g})")
    assert worst <= FD_BOUND
    # the header's closed forms of Ji
    p = nc.project(c, theta, a, x)
    xd, yd = (p[:, 0] - theta[1]) / theta[0], (p[:, 1] - theta[2]) / (a * theta[0])                  # d x, d y
    assert np.abs(Ji[:, 0, 0] - xd).max() < 1e-12 and np.abs(Ji[:, 1, 0] - a * yd).max() < 1e-12
    assert np.array_equal(Ji[:, 0, 1:3], np.tile([1.0, 0.0], (len(c), 1))) and np.array_equal(Ji[:, 1, 1:3], np.tile([0.0, 1.0], (len(c), 1)))


def test_with_nothing_free_and_no_distortion_it_is_np_track_ba_exactly():
    cams, X, obs, ci, pi = small_problem()
    theta, a = nc.theta_of(K)
    off, coff, cobs = nb.plan(ci, pi, len(cams), len(X))
    for huber in (np.inf, 1.0):
        old = nb.sweep(cams, K, X, obs, ci, pi, off, coff, cobs, huber)
        new = nc.sweep(cams, theta, a, X, obs, ci, pi, off, coff, cobs, huber)
        Jc, Ji, Jp, r = nc.split(new["rows"])
        assert np.array_equal(Jc.reshape(-1, 12), old["rows"][:, :12]) and np.array_equal(Jp.reshape(-1, 6), old["rows"][:, 12:18]) and np.array_equal(r, old["rows"][:, 18:])
        for name in ("B", "C", "gc", "gp", "stat", "count", "active"):
            assert np.array_equal(new[name], old[name]), name
        assert np.array_equal(nc.dense_w(new["rows"], ci, pi, len(cams), len(X)), nb.dense_w(old["rows"], ci, pi, len(cams), len(X)))
    # the adjustment takes the same steps: lambdas, costs, cameras and points
    c1, X1, h1, i1 = nb.bundle_adjust(cams, K, X, obs, ci, pi, huber=1.0, iters=6)
    c2, X2, K2, d2, h2, i2 = nc.bundle_adjust(cams, K, None, X, obs, ci, pi, free=0, huber=1.0, iters=6)
    assert i1["lams"] == i2["lams"] and np.allclose(h1, h2, rtol=1e-12, atol=0) and len(h1) == len(h2)
    assert np.abs(c1 - c2).max() <= 1e-10 and np.abs(X1 - X2).max() <= 1e-10 and np.array_equal(K2, K) and not d2.any()


def test_a_parameter_that_is_not_free_takes_no_step():
    cams, K0, X, obs, ci, pi = cal_problem()
    theta, a = nc.theta_of(K0)
    off, coff, cobs = nb.plan(ci, pi, 3, 60)
    o = nc.sweep(cams, theta, a, X, obs, ci, pi, off, coff, cobs)
    W = nc.dense_w(o["rows"], ci, pi, 3, 60)
    args = (o["B"], o["C"], o["gc"], o["gp"], o["E"], o["G"], o["gi"], o["F"], W, 1e-3)
    for mask in range(32):
        dc, di, dp, status = nc.step(*args, mask, True)
        on = np.array([(mask >> k) & 1 for k in range(5)], bool)
        assert not di[~on].any() and (not on.any() or di[on].all()) and status == 0, mask
        pc, pi_, pp, it = nc.solve_pcg(*args, mask, True, 1e-13, 400)
        assert not pi_[~on].any() and cc.rel(pc, dc) < 1e-9 and cc.rel(pp, dp) < 1e-9, mask
    # ONE unknown (camera 0 alone and fixed, cy free): the recurrence solves it in one iteration and must not divide 0 by 0 afterwards
    one = ci == 0
    o1 = nc.sweep(cams[:1], theta, a, X, obs[one], ci[one], pi[one], *nb.plan(ci[one], pi[one], 1, 60))
    a1 = (o1["B"], o1["C"], o1["gc"], o1["gp"], o1["E"], o1["G"], o1["gi"], o1["F"], nc.dense_w(o1["rows"], ci[one], pi[one], 1, 60), 1e-3, 4, True)
    d1, p1 = nc.step(*a1), nc.solve_pcg(*a1, 1e-10, 200)
    assert p1[3] == 5 and np.isfinite(p1[1]).all() and np.isfinite(p1[2]).all() and abs(p1[1][2] - d1[1][2]) <= 1e-9 * abs(d1[1][2]) and not p1[0].any()
    # G restricted to a free set that nothing observes is singular: bit 2
    assert nc.step(o["B"], o["C"], o["gc"], o["gp"], o["E"], np.zeros((5, 5)), o["gi"], o["F"], W, 1e-3, 9, True)[3] == 4
    assert nc.step(o["B"], o["C"], o["gc"], o["gp"], o["E"], np.zeros((5, 5)), o["gi"], o["F"], W, 1e-3, 0, True)[3] == 0


def test_the_weight_and_the_cost_on_both_sides_of_huber():
    cams, X = np.zeros((1, 6)), np.array([[0.0, 0, 2]])
    theta, a = nc.theta_of(K, (-0.1, 0.02))                                                           # the point is on the axis: d = 1
    huber = 2.0
    below, above = np.nextafter(np.float32(482.0), np.float32(0)), np.nextafter(np.float32(482.0), np.float32(999))
    rho = []
    for u in (below, np.float32(482.0), above):
        out = nc.sweep(cams, theta, a, X, np.float32([[u, 320]]), [0], [0], [0, 1], [0, 1], [0], huber)
        e = float(u) - 480.0
        w = 1.0 if e <= huber else huber / e
        assert out["w"].tolist() == [w] and out["count"].tolist() == [1, 0, int(e > huber)]
        assert abs(out["rows"][0, 28] + np.sqrt(w) * e) < 1e-12 and abs(out["rows"][0, 22] - np.sqrt(w) * 450.0) < 1e-12
        assert abs(out["stat"][0] - (e * e if e <= huber else 2 * huber * e - huber * huber)) < 1e-12 and abs(out["stat"][1] - e * e) < 1e-12
        rho.append(out["stat"][0])
    assert rho[0] < rho[1] == 4.0 < rho[2] and rho[2] - rho[0] < 1e-3                                  # continuous at e = huber
    far = nc.sweep(cams, theta, a, X, np.float32([[580, 320]]), [0], [0], [0, 1], [0, 1], [0], huber)
    assert far["w"].tolist() == [0.02] and far["stat"].tolist() == [2 * 2.0 * 100.0 - 4.0, 10000.0]
    # theta that cannot project: nothing is active (mode 0), everything active crossed (mode 1)
    bad = np.array([-900.0, 480, 320, 0, 0])
    assert nc.sweep(cams, bad, a, X, np.float32([[480, 320]]), [0], [0], [0, 1], [0, 1], [0])["count"].tolist() == [0, 0, 0]
    assert nc.sweep(cams, bad, a, X, np.float32([[480, 320]]), [0], [0], [0, 1], [0, 1], [0], np.inf, np.uint8([1]))["count"].tolist() == [0, 1, 0]


def test_the_restatement_reaches_the_cost_scipy_reaches():
    from scipy.optimize import least_squares
    cams, K0, X, obs, ci, pi = cal_problem()
    c2, X2, K2, d2, hist, info = nc.bundle_adjust(cams, K0, None, X, obs, ci, pi, ("f", "k1"), None, 100)
    o64 = obs.astype(np.float64)

    def resid(p):
        cm = np.vstack([cams[:1], p[:12].reshape(2, 6)])                                                 # camera 0 fixed, as in the LM
        return (nc.project(cm[ci], np.array([p[12], 480.0, 320.0, p[13], 0.0]), 1.0, p[14:].reshape(-1, 3)[pi]) - o64).ravel()

    p0 = np.r_[cams[1:].ravel(), 1000.0, 0.0, X.ravel()]
    assert abs((resid(p0) ** 2).sum() - hist[0]) <= 1e-9 * hist[0]
    ls = least_squares(resid, p0, method="trf", x_scale="jac", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=2000)
    low = 2.0 * ls.cost
    print(f"calibrating LM against scipy: LM {hist[-1]:.15g} after {len(hist) - 1} iterations (f {K2[0, 0]:.4f}, k1 {d2[0]:.6f}), scipy {low:.15g} "
          f"(f {ls.x[12]:.4f}, k1 {ls.x[13]:.6f}); cost / scipy - 1 = {hist[-1] / low - 1:.3e} (bound {SCIPY_MARGIN:.1e})")
    assert len(hist) - 1 < 100 and hist[-1] < 1e-3 * hist[0]                                          # it stopped by its own rule
    assert hist[-1] <= low * (1.0 + SCIPY_MARGIN), (hist[-1], low)
    assert abs(K2[0, 0] - 900.0) < 2.0 and abs(d2[0] + 0.12) < 0.01 and d2[1] == 0.0 and K2[0, 2] == 480.0 and K2[1, 1] == K2[0, 0]
    fixed = nc.bundle_adjust(cams, K0, None, X, obs, ci, pi, 0, None, 100)
    assert fixed[4][-1] > 10 * hist[-1]                                                               # the wrong K cannot be absorbed


def test_pcg_distance_from_the_direct_solve():
    """How far the reference PCG ends from the direct solve on the shapes of the GPU step test, and how many iterations the border
    costs against §9's PCG on the same problems: the figures track_cal_cases records."""
    import np_ba
    import track_ba_cases as tc
    for ncam in cc.PCG_CAMS:
        p = cc.with_border(tc.step_problem(ncam))
        args = cc.host_step_inputs(p)
        B, C, gc, gp, W0 = tc.host_step_inputs(p)
        for fix in (True, False):
            dc, di, dp, status = nc.step(*args, cc.PCG_LAM, cc.PCG_FREE, fix)
            pc, pi_, pp, it = nc.solve_pcg(*args, cc.PCG_LAM, cc.PCG_FREE, fix, cc.PCG_TOL, cc.PCG_ITERS)
            red = nc.solve_pcg(*args, cc.PCG_LAM, cc.PCG_FREE, fix, cc.PCG_TOL, cc.PCG_ITERS, reduced_border=True)[3]
            it9 = np_ba.solve_pcg(B, C, gc, gp, W0, cc.PCG_LAM, fix, tol=cc.PCG_TOL, iters=cc.PCG_ITERS)[2]
            fig = (cc.rel(pc, dc), cc.rel(pi_, di), cc.rel(pp, dp))
            print(f"ncam {ncam} fix_first={fix}: {it} iterations (reduced border block {red}, §9 without border {it9}), dc {fig[0]:.2e} di {fig[1]:.2e} "
                  f"dp {fig[2]:.2e} (recorded {cc.PCG_FIGURES[(ncam, fix)]})")
            assert status == 0 and (it, it9) == cc.PCG_ITERATIONS[(ncam, fix)] and red == it and it % 5 == 0 and it <= 1.25 * it9
            for f_, rec in zip(fig, cc.PCG_FIGURES[(ncam, fix)]):
                assert 0.1 * rec < f_ <= rec, (ncam, fix, fig)


# ---- the calibration scenes -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", cc.SCENES)
def test_calibration_scenes_meet_the_bars_of_the_fixture(name):
    fx = cc.fixture()
    rec, s = fx["scenes"][name], cc.scene(name)
    assert fx["free"] == list(cc.FREE) and rec["nobs"] == len(s["obs"]) and rec["ncam"] == len(s["cams"]) and rec["start_f"] == s["K"][0, 0]
    got = cc.run_scene(s, cc.host_adjust, cc.FREE)
    bar = cc.bars(name, rec)
    print(f"{name}: calibrated " + ", ".join(f"{k} {got[k]:.6g} (bar {bar[k]:.6g}, fixed K {rec['fixed'][k]:.6g})" for k in bar) + f"; {got['iterations']} iterations")
    for k in cc.BAR_KEYS:
        assert abs(got[k] - rec["calibrated"][k]) <= 1e-6 * max(rec["calibrated"][k], 1e-6), (k, got[k], rec["calibrated"][k])     # the fixture is this code's
    for k, b in bar.items():
        assert got[k] <= b and rec["calibrated"][k] < rec["fixed"][k], (k, got[k], b)
    if name != "corrupted":                                                                           # the measured claims of §15.4
        assert got["f_rel"] < 1e-3 and got["rms"] < 0.3 * rec["fixed"]["rms"]


# ---- the undistortions --------------------------------------------------------------------------------------------------------

def test_undistort_points_inverts_the_forward_model():
    Kf = np.array([[900.0, 0, 480], [0, 900.0, 320], [0, 0, 1]])
    gx, gy = np.meshgrid(np.linspace(0, 959, 97), np.linspace(0, 639, 65))
    ideal = np.stack([gx.ravel(), gy.ravel()], 1)
    worst = 0.0
    for k1 in (-0.3, -0.12, 0.0, 0.12, 0.3):
        for k2 in (0.0, 0.03):
            theta = np.array([900.0, 480, 320, k1, k2])
            back = nc.undistort_points(nc.distort_points(ideal, theta, 1.0, Kf).astype(np.float32), theta, 1.0, Kf)
            assert back.dtype == np.float32
            worst = max(worst, float(np.abs(back - ideal).max()))
    print(f"undistort_points(distort(p)) - p over the frame, |k1| <= 0.3: {worst:.3g} px (bound {INVERSE_BOUND:.3g})")
    assert worst <= INVERSE_BOUND
    # another K_out, an aspect, the centre, NaN and inf keypoints
    theta, a = np.array([900.0, 470, 330, -0.2, 0.05]), 1.05
    Ko = np.array([[700.0, 0, 400], [0, 650.0, 300], [0, 0, 1]])
    px = np.float32([[470, 330], [100, 50], [np.nan, 5], [7, np.inf], [900, 600]])
    out = nc.undistort_points(px, theta, a, Ko)
    assert out[0].tolist() == [400.0, 300.0] and np.isnan(out[2:4]).all() and np.isfinite(out[[1, 4]]).all()
    again = nc.distort_points(out[[1, 4]].astype(np.float64), theta, a, Ko)
    assert np.abs(again - px[[1, 4]]).max() < 1e-3
    assert nc.undistort_points(np.zeros((0, 2), np.float32), theta, a, Ko).shape == (0, 2)


def test_the_identity_cases_of_undistort_image():
    rng = np.random.default_rng(1)
    for H, W in ((1, 1), (1, 65), (65, 1), (64, 64), (65, 63)):
        for C in (1, 3):
            img = rng.integers(0, 256, (2, H, W, C), dtype=np.uint8)
            for Kf in (np.array([[900.0, 0, 480], [0, 900.0, 320], [0, 0, 1]]), np.array([[731.7, 0, W / 3.0], [0, 655.1, H / 7.0], [0, 0, 1]])):
                theta, a = nc.theta_of(Kf)
                out, mask = nc.undistort_image(img, theta, a, Kf)
                assert np.array_equal(out, img) and mask.all() and mask.shape == (2, H, W), (H, W, C)
    # a shift by whole pixels through K_out: columns move, the uncovered ones are 0 and invalid
    img = rng.integers(1, 256, (8, 12, 3), dtype=np.uint8)
    Kf = np.array([[100.0, 0, 6], [0, 100.0, 4], [0, 0, 1]])
    theta, a = nc.theta_of(Kf)
    Ko = Kf.copy()
    Ko[0, 2] += 2                                                                                      # output pixel xo reads source xo - 2
    out, mask = nc.undistort_image(img, theta, a, Ko)
    assert np.array_equal(out[:, 2:], img[:, :-2]) and not out[:, :2].any() and not mask[:, :2].any() and mask[:, 2:].all()
    # half a pixel: the mean of two neighbours, rounded half up; the last column needs a tap past the frame and is invalid
    Ko = Kf.copy()
    Ko[0, 2] -= 0.5
    out, mask = nc.undistort_image(img, theta, a, Ko)
    want = np.floor((img[:, :-1].astype(np.float32) + img[:, 1:].astype(np.float32)) * np.float32(0.5) + np.float32(0.5)).astype(np.uint8)
    assert np.array_equal(out[:, :-1], want) and not out[:, -1].any() and not mask[:, -1].any() and mask[:, :-1].all()
    # barrel distortion: the corners of the ideal image fall outside the source only for k1 > 0 (the forward map pushes them out)
    big = rng.integers(0, 256, (64, 96, 1), dtype=np.uint8)
    Kb = np.array([[60.0, 0, 47.5], [0, 60.0, 31.5], [0, 0, 1]])
    _, m_in = nc.undistort_image(big, np.array([60.0, 47.5, 31.5, -0.2, 0.0]), 1.0, Kb)
    _, m_out = nc.undistort_image(big, np.array([60.0, 47.5, 31.5, 0.2, 0.0]), 1.0, Kb)
    assert m_in.all() and not m_out[0, 0] and not m_out[-1, -1] and m_out[32, 48]
