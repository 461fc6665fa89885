"""Randomised parity sweep of the TRACKS-CAL family on the GPU box: sfm_track_cal_sweep / _product / _step,
track_cal.bundle_adjust_calibrated, sfm_undistort_points and sfm_undistort_image (through sfm_mvs_amd.track_cal, into sentinel-filled
buffers) vs the restatement tests/np_track_cal.py.  Values are compared to 1e-10 of the largest entry of the reference (the bar of
docs/geometry.md), bytes and counts exactly, the undistortions to the bit.

  python scripts/fuzz_track_cal.py [seconds] [seed] [family:case_seed]

Families (one case = one random draw; the problems and their degeneracies are scripts/fuzz_track_ba.py's, sizes log-uniform from 0,
one case in four a degeneracy; theta is drawn around (900, 480, 320) with k1 in -0.3..0.3, k2 in -0.05..0.05, a in 0.9..1.1):
  rows      mode 0 at a random huber, then mode 1 at a perturbed point (cameras, X and a step of theta left on the device) with the
            active set of the first: the rows of 30, the active bytes, stat and count
  blocks    B, g_c, C, g_p and the border E, G, g_i, F of both sweeps
  products  both modes over the rows of a sweep against the restatement, and <v, out0(xc, xi)> = <xc, out_c(v)> + <xi, out_i(v)>
  step      the damped step at a random lam and a random free mask, fix_first_camera on and off: the bordered system's residual
            against the stopping rule (|S y - rhs| <= 10 cg_tol |rhs| with S, rhs formed in NumPy from the device's own blocks and
            rows), the back-substitution to 1e-10, entries of parameters that are not free exactly 0, the status bits
  adjust    bundle_adjust_calibrated against the restatement's loop (direct solves): the histories agree to 1e-6 over their common
            length, which differs by one attempt at the most
  undistort points (n log-uniform from 0, NaN and inf keypoints in a degenerate case) and frames (1 to 3 frames, sides 1..96, C in
            {1, 3}, with and without the mask, K_out at random) to the bit
  composed  undistort_points of distorted keypoints, then the fixed-K sweep of TRACKS-BA at the pinhole camera: every observation is
            active on both sides and the rms residual (about 1 px: the points start 0.01 off) is that of the calibrated sweep on the
            distorted keypoints to a tenth (the local magnification of the lens, below 6 % on these scenes) plus 2e-3 px
No case is skipped: a degenerate case compares counts and status words.  The script stops at the first mismatch, prints the family and
the case seed that rebuilds the inputs without a GPU, and exits non-zero.
"""
import os
import sys
import time

os.environ.setdefault("OMP_WAIT_POLICY", "passive")

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "scripts"))
import np_track_ba as nb
import np_track_cal as nc
import fuzz_track_ba as fz
from fuzz_tracks import dev, log_uniform_from_zero

TOL = 1e-10
close = fz.close


def random_theta(rng, distorted=True):
    k1, k2 = (rng.uniform(-0.3, 0.3), rng.uniform(-0.05, 0.05)) if distorted else (0.0, 0.0)
    return np.array([rng.uniform(700, 1100), rng.uniform(440, 520), rng.uniform(290, 350), k1, k2]), float(rng.choice([1.0, rng.uniform(0.9, 1.1)]))


def with_theta(p, rng, distorted=True):
    """A fuzz_track_ba problem with intrinsics: the observations stay (they are residual noise to the model), theta is random."""
    p["theta"], p["aspect"] = random_theta(rng, distorted)
    return p


def gen_problem(rng, max_obs=fz.MAX_OBS, deg=None):
    return with_theta(fz.gen_problem(rng, max_obs, deg), rng)


# ---- device side ----------------------------------------------------------------------------------------------------------

def device_sweep(pl, p, cams, theta, X, huber, mode=0, active=None, ws=None, dtheta=None):
    """The sweep into sentinel-padded outputs -> (out dict of views, message if a word past a size was written)."""
    import torch
    from sfm_mvs_amd import track_cal
    f64 = torch.float64
    bufs = dict(JtJ_cam=fz.padded((pl.ncam, 36), f64), Jtr_cam=fz.padded((pl.ncam, 6), f64), JtJ_pt=fz.padded((pl.npt, 9), f64),
                Jtr_pt=fz.padded((pl.npt, 3), f64), E=fz.padded((pl.ncam, 30), f64), G=fz.padded((25,), f64), Jtr_theta=fz.padded((5,), f64),
                F=fz.padded((pl.npt, 15), f64), stat=fz.padded((2,), f64), count=fz.padded((3,), torch.int32))
    act_whole = None
    if active is None:
        act_whole, active = fz.padded((pl.nobs,), torch.uint8)
    out = track_cal.sweep(pl, dev(cams), theta, p["aspect"], dev(X), dev(p["obs"]), huber, mode, active, ws, out={k: v[1] for k, v in bufs.items()},
                          dtheta=None if dtheta is None else dev(dtheta))
    for name, (whole, view) in bufs.items():
        if not fz.untouched(whole, view.shape[0]):
            return out, f"{name}: written past its size"
    if act_whole is not None and not fz.untouched(act_whole, pl.nobs):
        return out, "active: written past its size"
    return out, ""


def want_sweep(p, cams, theta, X, huber, active=None):
    return nc.sweep(cams, theta, p["aspect"], X, p["obs"], p["cam_idx"], p["pt_idx"], p["track_off"], p["cam_off"], p["cam_obs"], huber, active)


def compare_rows(pl, out, want):
    from sfm_mvs_amd import track_cal
    if not np.array_equal(out["active"].cpu().numpy(), want["active"]):
        return f"active: differs at {np.flatnonzero(out['active'].cpu().numpy() != want['active'])[:3].tolist()}"
    if out["count"].cpu().numpy().tolist() != want["count"].tolist():
        return f"count: {out['count'].cpu().numpy().tolist()} vs {want['count'].tolist()}"
    return close("rows", track_cal.rows_of(pl, out["ws"]), want["rows"]) or close("stat", out["stat"], want["stat"])


def compare_blocks(out, want):
    return (close("JtJ_cam", out["JtJ_cam"], want["B"].reshape(-1, 36)) or close("Jtr_cam", out["Jtr_cam"], want["gc"]) or
            close("JtJ_pt", out["JtJ_pt"], want["C"].reshape(-1, 9)) or close("Jtr_pt", out["Jtr_pt"], want["gp"]) or
            close("E", out["E"], want["E"].reshape(-1, 30)) or close("G", out["G"], want["G"].reshape(25)) or
            close("Jtr_theta", out["Jtr_theta"], want["gi"]) or close("F", out["F"], want["F"].reshape(-1, 15)))


def check_sweep(p, huber=None, trial=None, what=("rows", "blocks")):
    """Mode 0 at (cams, theta, X), then mode 1 at `trial` = (cams', dtheta, X') (default: a small random move) with the first sweep's
    active set; the step of theta goes to the device as dtheta_dev."""
    huber = p["huber"] if huber is None else huber
    pl = fz.device_plan(p)
    out, msg = device_sweep(pl, p, p["cams"], p["theta"], p["X"], huber)
    want = want_sweep(p, p["cams"], p["theta"], p["X"], huber)
    cmp = lambda o, w: ("rows" in what and compare_rows(pl, o, w)) or ("blocks" in what and compare_blocks(o, w)) or ""  # noqa: E731
    msg = msg or cmp(out, want)
    if msg:
        return "mode 0 " + msg, out, want
    if trial is None:
        rng = np.random.default_rng(len(p["obs"]))
        trial = (p["cams"] * (1 + 1e-3 * rng.standard_normal(p["cams"].shape)), p["theta"] * 1e-3 * rng.standard_normal(5), p["X"] + rng.normal(0, 0.02, p["X"].shape))
    from sfm_mvs_amd import track_cal
    out1, msg = device_sweep(pl, p, trial[0], p["theta"], trial[2], huber, 1, out["active"], track_cal.workspace(pl), trial[1])
    want1 = want_sweep(p, trial[0], p["theta"] - trial[1], trial[2], huber, want["active"])
    msg = msg or cmp(out1, want1)
    return ("mode 1 " + msg if msg else ""), out, want


def check_product(p, seed=0):
    from sfm_mvs_amd import track_cal
    pl = fz.device_plan(p)
    out, msg = device_sweep(pl, p, p["cams"], p["theta"], p["X"], p["huber"])
    if msg:
        return msg
    rows = track_cal.rows_of(pl, out["ws"]).cpu().numpy()
    rng = np.random.default_rng(seed)
    xc, xi, v = rng.normal(size=(pl.ncam, 6)), rng.normal(size=5), rng.normal(size=(pl.npt, 3))
    u = track_cal.product(pl, out["ws"], dev(xc), 0, dev(xi))
    wc, wi = track_cal.product(pl, out["ws"], dev(v), 1)
    args = (rows, p["cam_idx"], p["pt_idx"], p["track_off"], p["cam_off"], p["cam_obs"], pl.ncam, pl.npt)
    want_c, want_i = nc.product(*args, v, None, 1)
    msg = close("out0", u, nc.product(*args, xc, xi, 0)) or close("out_c", wc, want_c)
    msg = msg or close("out_theta", wi, want_i)
    if msg or p["deg"] in (4, 5, 6):                                          # inconsistent CSRs: the two sides see different observations
        return msg
    un, wn, wi_n = u.cpu().numpy(), wc.cpu().numpy(), wi.cpu().numpy()
    lhs, rhs = float((v * un).sum()), float((xc * wn).sum() + (xi * wi_n).sum())
    scale = float((np.abs(v) * np.abs(un)).sum() + (np.abs(xc) * np.abs(wn)).sum() + (np.abs(xi) * np.abs(wi_n)).sum())
    return "" if abs(lhs - rhs) <= 1e-11 * scale else f"adjointness: {lhs!r} vs {rhs!r} (scale {scale:.3g})"


def device_blocks(out):
    """The sweep's blocks on the host in the restatement's shapes: (B, C, gc, gp, E, G, gi, F)."""
    g = lambda k, s: out[k].cpu().numpy().reshape(s)  # noqa: E731
    return (g("JtJ_cam", (-1, 6, 6)), g("JtJ_pt", (-1, 3, 3)), g("Jtr_cam", (-1, 6)), g("Jtr_pt", (-1, 3)), g("E", (-1, 6, 5)), g("G", (5, 5)), g("Jtr_theta", (5,)),
            g("F", (-1, 3, 5)))


def check_step(p, lam=1e-3, free=9, fix_first=True, cg_tol=1e-10, cg_iters=400):
    from sfm_mvs_amd import track_cal
    pl = fz.device_plan(p)
    out, msg = device_sweep(pl, p, p["cams"], p["theta"], p["X"], p["huber"])
    if msg:
        return msg
    dc, di, dp, it, status = track_cal.step(pl, out, lam, free, fix_first, cg_tol, cg_iters)
    dc, di, dp = dc.cpu().numpy(), di.cpu().numpy(), dp.cpu().numpy()
    if not (np.isfinite(dc).all() and np.isfinite(di).all() and np.isfinite(dp).all()):
        return "step: not finite"
    blocks = device_blocks(out)
    W = nc.dense_w(track_cal.rows_of(pl, out["ws"]).cpu().numpy(), p["cam_idx"], p["pt_idx"], pl.ncam, pl.npt)
    s = nc.system(*blocks, W, lam, free, fix_first)
    if status != s["status"]:
        return f"status {status} vs {s['status']}"
    y = np.r_[dc.ravel(), di]
    if y[s["held"]].any():
        return "step: camera 0 or a parameter that is not free moved"
    _, bad_p = nb.singular_blocks(blocks[0], blocks[1], lam)
    if dp[bad_p].any():
        return "step: a point with a singular block moved"
    msg = close("dp", dp, nc._back(s, y)[2])
    if msg or it >= cg_iters or status & 4:                                   # a singular Gd: the identity preconditions, convergence is not promised
        return msg
    live = ~s["held"]
    res, scale = np.linalg.norm((s["S"] @ y - s["rhs"])[live]), np.linalg.norm(s["rhs"][live])
    return "" if res <= 10 * cg_tol * scale else f"step: |S y - rhs| {res:.3g} > 10 * {cg_tol:g} * {scale:.3g} after {it} iterations"


def check_adjust(p, free=("f", "k1"), iters=4):
    import torch
    from sfm_mvs_amd import track_cal
    huber = None if np.isinf(p["huber"]) else p["huber"]
    Kp, dist = nc.K_of(p["theta"], p["aspect"]), p["theta"][3:]
    try:
        wc, wX, wK, wd, whist, winfo = nc.bundle_adjust(p["cams"], Kp, dist, p["X"], p["obs"], p["cam_idx"], p["pt_idx"], free, huber, iters)
    except np.linalg.LinAlgError:                                             # a reduced system the direct solve cannot take: no reference
        wc = None                                                             # for the steps; the first sweep's counts and cost still compare
    c, X, Kn, dn, hist, info = track_cal.bundle_adjust_calibrated(dev(p["cams"]), Kp, dist, dev(p["X"]), dev(p["obs"]), dev(p["cam_idx"]), dev(p["pt_idx"]),
                                                                  free, huber, iters)
    if X.dtype != torch.float64 or not np.isfinite(hist).all() or not np.isfinite(Kn).all():
        return "adjust: not finite"
    if wc is None:
        off, coff, cobs = nb.plan(p["cam_idx"], p["pt_idx"], len(p["cams"]), len(p["X"]))
        first = nc.sweep(p["cams"], p["theta"], p["aspect"], p["X"], p["obs"], p["cam_idx"], p["pt_idx"], off, coff, cobs, np.inf if huber is None else huber)
        if info["active"] != int(first["count"][0]) or not np.isclose(hist[0], first["stat"][0], rtol=1e-9, atol=1e-12):
            return f"adjust: active {info['active']}, first cost {hist[0]} vs {int(first['count'][0])}, {first['stat'][0]}"
        return "" if all(b <= a for a, b in zip(hist, hist[1:])) else f"adjust: the history rises: {hist}"
    if abs(len(hist) - len(whist)) > 1:
        return f"adjust: {len(hist)} vs {len(whist)} history entries"
    n = min(len(hist), len(whist))
    if not np.allclose(hist[:n], whist[:n], rtol=1e-6, atol=1e-12):
        return f"adjust: history {hist[:n]} vs {whist[:n]}"
    if len(hist) == len(whist) and not np.allclose(np.r_[Kn[0, 0], dn], np.r_[wK[0, 0], wd], rtol=1e-5, atol=1e-7):
        return f"adjust: f, k1, k2 {Kn[0, 0]}, {dn} vs {wK[0, 0]}, {wd}"
    return "" if info["active"] == winfo["active"] else f"adjust: active {info['active']} vs {winfo['active']}"


def check_points(px, theta, a, K_out):
    import torch
    from sfm_mvs_amd import track_cal
    whole, view = fz.padded((len(px), 2), torch.float32)
    view.copy_(dev(px))
    got = track_cal.undistort_points(view, nc.K_of(theta, a), theta[3:], K_out).cpu().numpy()
    want = nc.undistort_points(px, theta, a, K_out)
    same = np.array_equal(got.view(np.int32), want.view(np.int32)) or (np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(got)], want[~np.isnan(want)]))
    return "" if same else f"undistort_points: differs at {np.argwhere(got != want)[:3].tolist()}"


def check_image(img, theta, a, K_out, want_mask=True):
    import torch
    from sfm_mvs_amd import track_cal
    res = track_cal.undistort_images(dev(img), nc.K_of(theta, a), theta[3:], K_out, want_mask)
    got, mask = (res if want_mask else (res, None))
    want, wmask = nc.undistort_image(img, theta, a, K_out)
    if got.dtype != torch.uint8 or not np.array_equal(got.cpu().numpy(), want):
        return f"undistort_image: differs at {np.argwhere(got.cpu().numpy() != want)[:3].tolist()}"
    return "" if mask is None or np.array_equal(mask.cpu().numpy(), wmask) else "undistort_image: the mask differs"


# ---- families ---------------------------------------------------------------------------------------------------------------

def fuzz_rows(rng):
    return check_sweep(gen_problem(rng), what=("rows",))[0]


def fuzz_blocks(rng):
    return check_sweep(gen_problem(rng), what=("blocks",))[0]


def fuzz_products(rng):
    return check_product(gen_problem(rng), int(rng.integers(1 << 30)))


def fuzz_step(rng):
    p = gen_problem(rng, 1 << 10, deg=int(rng.choice([0, 1, 2, 7])) if rng.integers(4) == 0 else -1)
    return check_step(p, float(rng.choice([1e-3, 1e-1, 1.0])), int(rng.integers(32)), bool(rng.integers(2)))


def fuzz_adjust(rng):
    ncam, npt = int(rng.integers(2, 7)), max(4, log_uniform_from_zero(rng, 64))
    p = fz.make_problem(rng, ncam, npt, np.maximum(2, rng.integers(ncam // 2 + 1, ncam + 1, npt)))
    p["theta"], p["aspect"] = np.array([900.0 * rng.uniform(0.9, 1.1), 480.0, 320.0, rng.uniform(-0.1, 0.1), 0.0]), 1.0
    p["huber"], p["deg"] = float(rng.choice([1.0, 3.0, np.inf])), -1
    if rng.integers(4) == 0 and len(p["obs"]):
        p["obs"][rng.integers(len(p["obs"]))] = np.nan
    return check_adjust(p, [("f", "k1"), ("f",), ("k1",), ("f", "k1", "k2"), ()][int(rng.integers(5))])


def fuzz_undistort(rng):
    theta, a = random_theta(rng)
    K_out = nc.K_of(theta, a) if rng.integers(2) else np.array([[rng.uniform(500, 1200), 0, rng.uniform(300, 600)], [0, rng.uniform(500, 1200), rng.uniform(200, 400)], [0, 0, 1.0]])
    n = log_uniform_from_zero(rng, 1 << 12)
    px = rng.uniform(-50, 1010, (n, 2)).astype(np.float32)
    if rng.integers(4) == 0 and n:
        px[rng.random(n) < 0.1, int(rng.integers(2))] = rng.choice([np.nan, np.inf, -np.inf])
    msg = check_points(px, theta, a, K_out)
    if msg:
        return msg
    H, W, C = int(rng.integers(1, 97)), int(rng.integers(1, 97)), int(rng.choice([1, 3]))
    img = rng.integers(0, 256, (int(rng.integers(1, 4)), H, W, C), dtype=np.uint8)
    ti = np.array([rng.uniform(0.5, 1.5) * W, rng.uniform(0.3, 0.7) * W, rng.uniform(0.3, 0.7) * H, theta[3], theta[4]])
    Ki = nc.K_of(ti, a) if rng.integers(2) else np.array([[rng.uniform(0.5, 1.5) * W, 0, rng.uniform(0.2, 0.8) * W], [0, rng.uniform(0.5, 1.5) * W, rng.uniform(0.2, 0.8) * H], [0, 0, 1.0]])
    return check_image(img, ti, a, Ki, bool(rng.integers(2)))


def fuzz_composed(rng):
    """Keypoints of a distorted camera, undistorted on the device, then the fixed-K sweep of TRACKS-BA at the pinhole camera."""
    import torch
    from sfm_mvs_amd import track_ba, track_cal
    ncam, npt = int(rng.choice([2, 3, 8])), max(1, log_uniform_from_zero(rng, 512))
    p = fz.make_problem(rng, ncam, npt, np.full(npt, min(ncam, 3)), displaced=0.0, perturb=0.0)
    theta, a = np.array([900.0, 480.0, 320.0, rng.uniform(-0.2, 0.2), rng.uniform(-0.03, 0.03)]), 1.0
    Kp = nc.K_of(theta, a)
    p["obs"] = nc.distort_points(p["obs"].astype(np.float64), theta, a, Kp).astype(np.float32)       # what the distorted camera sees
    p["theta"], p["aspect"], p["huber"], p["deg"] = theta, a, np.inf, -1
    pl = fz.device_plan(p)
    cal = track_cal.sweep(pl, dev(p["cams"]), theta, a, dev(p["X"]), dev(p["obs"]))
    und = track_cal.undistort_points(dev(p["obs"]), Kp, theta[3:])
    pin = track_ba.sweep(pl, dev(p["cams"]), Kp, dev(p["X"]), und)
    c_cal, c_pin, n = float(cal["stat"][0]), float(pin["stat"][0]), int(cal["count"][0])
    if n != int(pin["count"][0]) or n != len(p["obs"]):
        return f"composed: {n} vs {int(pin['count'][0])} active of {len(p['obs'])}"
    e_cal, e_pin = np.sqrt(c_cal / max(n, 1)), np.sqrt(c_pin / max(n, 1))                           # rms px on both sides of the lens
    return "" if abs(e_cal - e_pin) <= 0.1 * max(e_cal, e_pin) + 2e-3 else f"composed: rms {e_cal:.5f} px distorted vs {e_pin:.5f} px undistorted"


FAMILIES = [("rows", fuzz_rows, 2), ("blocks", fuzz_blocks, 2), ("products", fuzz_products, 2), ("step", fuzz_step, 2), ("adjust", fuzz_adjust, 1),
            ("undistort", fuzz_undistort, 2), ("composed", fuzz_composed, 1)]


def run(budget, seed, log=print):
    """Cases for `budget` seconds from `seed`; stops at the first mismatch -> (counts per family, mismatches, seconds)."""
    fns = {name: fn for name, fn, _ in FAMILIES}
    rng = np.random.default_rng(seed)
    weights = np.array([w for _, _, w in FAMILIES], float); weights /= weights.sum()
    t0 = time.time(); counts = {name: 0 for name, _, _ in FAMILIES}; bad = 0
    while time.time() - t0 < budget and not bad:
        name = FAMILIES[int(rng.choice(len(FAMILIES), p=weights))][0]
        case_seed = int(rng.integers(1 << 31))
        try:
            msg = fns[name](np.random.default_rng(case_seed))
        except Exception as e:  # noqa: BLE001
            msg = f"EXCEPTION {e!r}"[:300]
        counts[name] += 1
        if msg:
            bad += 1
            log(f"MISMATCH {name} (seed {seed}, case seed {case_seed}; replay: fuzz_track_cal.py 0 0 {name}:{case_seed}) {msg}")
    return counts, bad, time.time() - t0


def main():
    import sfm_mvs_amd
    from sfm_mvs_amd import _lib
    budget = float(sys.argv[1]) if len(sys.argv) > 1 else 120.0
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    sfm_mvs_amd.lib()
    if len(sys.argv) > 3:                               # replay one case
        name, case_seed = sys.argv[3].split(":")
        msg = {n: fn for n, fn, _ in FAMILIES}[name](np.random.default_rng(int(case_seed)))
        print(f"fuzz_track_cal replay {name}:{case_seed}: {msg or 'no mismatch'}")
        return 1 if msg else 0
    counts, bad, dt = run(budget, seed, log=lambda s: print(s, flush=True))
    print(f"fuzz_track_cal: seed {seed}, {sum(counts.values())} cases {counts}, {bad} mismatches, {dt:.0f} s")
    print(f"sfm_build_id {_lib.build_id()}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
