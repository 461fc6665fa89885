"""Shapes, scenes and recorded figures shared by tests/test_track_cal_cpu.py, tests/test_gpu_track_cal.py and
scripts/calibrate_track_cal.py (docs/tracks.md §15)."""
import functools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.dirname(os.path.abspath(__file__)), os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

import np_track_ba as nb  # noqa: E402
import np_track_cal as nc  # noqa: E402
import track_ba_cases as tc  # noqa: E402

K = tc.K
FIXTURE = os.path.join(ROOT, "tests", "golden", "track_cal_calibration.json")
PCG_LAM, PCG_TOL, PCG_ITERS, PCG_ALLOW = tc.PCG_LAM, tc.PCG_TOL, tc.PCG_ITERS, tc.PCG_ALLOW
PCG_CAMS = (169, 170)           # 6 * ncam + 5 = 1019 and 1025 unknowns: the second just takes the CG kernels' second trip over 1024 lanes
PCG_FREE = 9                    # f and k1, the default
# max|pcg - direct| / max|direct| (dc, di, dp) of the float64 NumPy PCG (np_track_cal.solve_pcg: the kernel's recurrence, cg_tol =
# 1e-13, looked at every fifth iteration, preconditioner blockdiag(Bd^-1, Gd^-1)) against np_track_cal.step at lam = 1e-2 on
# step_problem(ncam) of tests/track_ba_cases.py linearised at theta = (900, 480, 320, 0, 0), Huber 1 px, f and k1 free, measured on
# the CPU by test_track_cal_cpu.py::test_pcg_distance_from_the_direct_solve.  Iterations: 115 in all four cases, against 110, 105,
# 105, 110 of §9's PCG on the same problems (np_ba.solve_pcg, no border); with all five parameters free 130.  The reduced block
# Gd - F^T Cd^-1 F in the place of Gd takes exactly as many (115, 130): the plain Gd stays.  The device is allowed PCG_ALLOW times
# these figures.
PCG_FIGURES = {
    (169, True): (1.7e-13, 2.7e-13, 8.4e-14),
    (169, False): (1.7e-13, 5.3e-13, 8.0e-14),
    (170, True): (1.2e-13, 1.3e-13, 5.8e-14),
    (170, False): (1.5e-13, 3.9e-13, 7.5e-14),
}
PCG_ITERATIONS = {(169, True): (115, 110), (169, False): (115, 105), (170, True): (115, 105), (170, False): (115, 110)}   # (bordered, §9)


def with_border(p, theta=None):
    """step_problem's dict with the intrinsics of the linearisation."""
    p = dict(p)
    p["theta"], p["aspect"] = nc.theta_of(K) if theta is None else (np.asarray(theta, np.float64), 1.0)
    return p


def host_sweep(p, huber=None, active=None, at=None):
    cams, theta, X = at if at is not None else (p["cams"], p["theta"], p["X"])
    return nc.sweep(cams, theta, p["aspect"], X, p["obs"], p["cam_idx"], p["pt_idx"], p["track_off"], p["cam_off"], p["cam_obs"],
                    p["huber"] if huber is None else huber, active)


def host_step_inputs(p):
    """(B, C, gc, gp, E, G, gi, F, W) of the restatement at (cams, theta, X)."""
    o = host_sweep(p)
    return (o["B"], o["C"], o["gc"], o["gp"], o["E"], o["G"], o["gi"], o["F"], nc.dense_w(o["rows"], p["cam_idx"], p["pt_idx"], len(p["cams"]), len(p["X"])))


def rel(got, want):
    return float(np.abs(np.asarray(got) - want).max() / np.abs(want).max())


# ---- the calibration scenes (docs/tracks.md §15.4) ------------------------------------------------------------------------------

PLANTED = dict(f=900.0, k1=-0.12, k2=0.03)
NOMINAL_F = 1000.0
CX, CY = 480.0, 320.0


def ring_scene(ncam, seed=7):
    """ncam cameras of datagen.ring_cameras, 400 points in a cube of side 3, two thirds of the (camera, point) pairs observed, 0.3 px
    of noise; planted f = 900, k1 = -0.12, k2 = 0.03, the start at the nominal f = 1000 without distortion, cameras perturbed by
    0.2 %, points by 0.01."""
    from datagen import ring_cameras
    rng = np.random.default_rng(seed + ncam)
    truth = ring_cameras(ncam)
    X = rng.uniform(-1.5, 1.5, (400, 3))
    see = rng.random((400, ncam)) < 2.0 / 3.0
    see[:, :2] |= (see.sum(1, keepdims=True) < 2)
    pt_idx, cam_idx = np.nonzero(see)
    theta = np.array([PLANTED["f"], CX, CY, PLANTED["k1"], PLANTED["k2"]])
    obs = nc.project(truth[cam_idx], theta, 1.0, X[pt_idx]) + rng.normal(0, 0.3, (len(pt_idx), 2))
    return dict(name=f"ring{ncam}", K=np.array([[NOMINAL_F, 0, CX], [0, NOMINAL_F, CY], [0, 0, 1.0]]), truth=truth, theta_true=theta,
                cams=truth * (1 + 0.002 * rng.standard_normal(truth.shape)), X=X + rng.normal(0, 0.01, X.shape), obs=obs.astype(np.float32),
                cam_idx=cam_idx.astype(np.int32), pt_idx=pt_idx.astype(np.int32), clean=np.arange(len(obs)), huber=None, iters=30)


def corrupted_scene(k1=-0.3):
    """The corrupted ring of §9 (test_track_ba_cpu.ring_problem: 3 200 observations, one keypoint of 107 tracks displaced) with a
    planted k1: every keypoint pushed through the forward model; the start is the K of the scene without distortion; Huber 1 px."""
    from test_track_ba_cpu import ring_problem
    p = ring_problem()
    Kc = np.asarray(p["K"], np.float64)
    theta = np.array([Kc[0, 0], Kc[0, 2], Kc[1, 2], k1, 0.0])
    obs = nc.distort_points(p["obs"].astype(np.float64), theta, Kc[1, 1] / Kc[0, 0], Kc).astype(np.float32)
    return dict(name="corrupted", K=Kc, truth=p["truth"], theta_true=theta, cams=p["cams"], X=p["X"], obs=obs, cam_idx=p["cam_idx"],
                pt_idx=p["pt_idx"], clean=p["clean"], huber=1.0, iters=30)


@functools.lru_cache(maxsize=None)
def scene(name):
    return {"ring8": lambda: ring_scene(8), "ring16": lambda: ring_scene(16), "corrupted": corrupted_scene}[name]()


SCENES = ("ring8", "ring16", "corrupted")
FREE = ("f", "k1")


def figures(s, cams, X, K_new, dist):
    """(clean rms px, |f'/f - 1|, |k1' - k1|, median aligned centre error) of a result on scene s."""
    theta, a = nc.theta_of(K_new, dist)
    t = s["theta_true"]
    return dict(rms=nc.rms_error(cams, theta, a, X, s["obs"], s["cam_idx"], s["pt_idx"], s["clean"]), f_rel=abs(theta[0] / t[0] - 1.0),
                k1_abs=abs(theta[3] - t[3]), centre=float(np.median(nb.aligned_centre_errors(cams, s["truth"]))))


def run_scene(s, adjust, free):
    """adjust(cams, K, dist, X, obs, cam_idx, pt_idx, free, huber, iters) -> (cams, X, K', dist', history, info); -> figures."""
    c, X, K_new, dist, hist, info = adjust(s["cams"], s["K"], None, s["X"], s["obs"], s["cam_idx"], s["pt_idx"], free, s["huber"], s["iters"])
    out = figures(s, np.asarray(c), np.asarray(X), K_new, dist)
    out.update(iterations=len(hist) - 1, cost=float(hist[-1]))
    return out


def host_adjust(cams, K_, dist, X, obs, ci, pi, free, huber, iters):
    return nc.bundle_adjust(cams, K_, dist, X, obs, ci, pi, free, huber, iters)


def fixture():
    with open(FIXTURE) as fh:
        return json.load(fh)


BAR_KEYS = ("rms", "f_rel", "k1_abs", "centre")


def bar_keys(name):
    """The corrupted scene starts at its true f: the fixed-K figure of f_rel is 0 by construction and no bar lies halfway to it."""
    return tuple(k for k in BAR_KEYS if not (name == "corrupted" and k == "f_rel"))


def bars(name, rec):
    """Halfway between the calibrated and the fixed-K figure of the restatement, as BA_BAR of §9."""
    return {k: 0.5 * (rec["calibrated"][k] + rec["fixed"][k]) for k in bar_keys(name)}
