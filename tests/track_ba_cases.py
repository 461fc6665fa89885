"""Shapes and recorded figures shared by tests/test_track_ba_cpu.py and tests/test_gpu_track_ba.py (docs/tracks.md §9)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.dirname(os.path.abspath(__file__)), os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

import np_ba  # noqa: E402
import np_track_ba as nb  # noqa: E402

K = np.array([[900.0, 0, 480.0], [0, 900.0, 320.0], [0, 0, 1.0]])
PCG_LAM, PCG_TOL, PCG_ITERS = 1e-2, 1e-13, 400
PCG_CAMS = (170, 171)           # 6 * ncam = 1020 and 1026 unknowns: the second just takes the CG kernels' second trip over 1024 lanes
# max|pcg - direct| / max|direct| (dc, dp) of the float64 NumPy PCG (np_ba.solve_pcg: the kernel's recurrence, cg_tol = 1e-13, looked
# at every fifth iteration) against np_ba.solve_direct at lam = 1e-2 on step_problem(ncam), Huber 1 px, measured on the CPU by
# test_track_ba_cpu.py::test_pcg_distance_from_the_direct_solve.  The device sums in another order and contracts to FMAs: it is
# allowed PCG_ALLOW times these figures, as tests/test_gpu_ba_schur.py allows its solver.
PCG_FIGURES = {
    (170, True): (2.4e-13, 1.5e-13),           # 105 iterations
    (170, False): (1.1e-13, 4.1e-14),          # 110
    (171, True): (2.5e-13, 8.4e-14),           # 110
    (171, False): (2.0e-13, 9.0e-14),          # 110
}
PCG_ALLOW = 10.0


def step_problem(ncam, npt=300, views=6, seed=21):
    """ncam cameras on a ring, npt points each seen by `views` neighbouring cameras (a window that walks round the ring), 0.3 px
    noise, a tenth of the observations displaced -> the dict of fuzz_track_ba.make_problem."""
    import fuzz_track_ba as fz
    rng = np.random.default_rng(seed + ncam)
    p = fz.make_problem(rng, ncam, npt, np.full(npt, views))
    first = (np.arange(npt) * ncam // npt)[:, None]
    cam = np.sort((first + np.arange(views)[None, :] * 7) % ncam, axis=1).reshape(-1).astype(np.int32)   # stride 7: the windows interlock
    p["cam_idx"] = cam
    rng2 = np.random.default_rng(seed)
    obs = np_ba.project(p["truth"][cam], K, (p["X"])[p["pt_idx"]][:, None, :])[:, 0] + rng2.normal(0, 0.3, (len(cam), 2))
    hit = rng2.random(len(cam)) < 0.1
    obs[hit] += 30.0
    p["obs"] = obs.astype(np.float32)
    p["track_off"], p["cam_off"], p["cam_obs"] = nb.plan(cam, p["pt_idx"], ncam, npt)
    p["huber"], p["deg"] = 1.0, -1
    return p


def host_step_inputs(p):
    """(B, C, gc, gp, W) of the restatement at (cams, X)."""
    out = nb.sweep(p["cams"], K, p["X"], p["obs"], p["cam_idx"], p["pt_idx"], p["track_off"], p["cam_off"], p["cam_obs"], p["huber"])
    return out["B"], out["C"], out["gc"], out["gp"], nb.dense_w(out["rows"], p["cam_idx"], p["pt_idx"], len(p["cams"]), len(p["X"]))


def rel(got, want):
    return float(np.abs(np.asarray(got) - want).max() / np.abs(want).max())
