"""Randomised parity sweep of the TRACKS-BA family on the GPU box: sfm_track_ba_sweep / _product / _step and
track_ba.bundle_adjust_tracks (through sfm_mvs_amd.track_ba, into sentinel-filled buffers) vs the restatement tests/np_track_ba.py.
Values are compared to 1e-10 of the largest entry of the reference (the bar of docs/geometry.md), bytes and counts exactly.

  python scripts/fuzz_track_ba.py [seconds] [seed] [family:case_seed]

Families (one case = one random draw; sizes log-uniform from 0 up to a cap that keeps the NumPy side well under a second):
  sweep     random cameras on a ring, points near the origin, random visibility, pixel noise and displaced keypoints; mode 0 at a
            random huber (inf and 1e-3 included), then mode 1 at a perturbed point with the active set of the first
  product   both products over the rows of a sweep against the restatement, and <v, W^T x> = <x, W v> to 1e-11 of the sum of magnitudes
  step      the damped step at a random lam, fix_first_camera on and off: the reduced system's residual against the stopping rule
            (|S dc - rhs| <= 10 cg_tol |rhs| with S, rhs formed in NumPy from the device's own blocks and rows) and the
            back-substitution to 1e-10; the status bits
  composed  bundle_adjust_tracks against the restatement's loop (direct solves): the histories agree to 1e-6 over their common length,
            which differs by one attempt at the most
One case in four carries a degeneracy: no observation, NaN keypoints, a NaN point, a point behind a camera, indices from {-1, ncam,
npt, INT32_MAX} in cam_idx, pt_idx and cam_obs, CSR offsets outside 0..nobs, a camera without observations, every observation an
outlier.  The script stops at the first mismatch, prints the family and the case seed that rebuilds the inputs without a GPU, and
exits non-zero.
"""
import os
import sys
import time

os.environ.setdefault("OMP_WAIT_POLICY", "passive")

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "scripts"))
import np_ba
import np_track_ba as nb
from fuzz_tracks import SENTINEL, dev, log_uniform_from_zero

K = np.array([[900.0, 0, 480.0], [0, 900.0, 320.0], [0, 0, 1.0]])
INT32_MAX = 2 ** 31 - 1
TOL = 1e-10
MAX_OBS = 1 << 13


def random_cams(rng, ncam):
    """[ncam, 6] (rvec, tvec): cameras on a ring of radius ~8 that look at the origin."""
    from scipy.spatial.transform import Rotation
    cams = np.zeros((ncam, 6))
    for k in range(ncam):
        a = rng.uniform(0, 2 * np.pi)
        C = np.array([8 * np.cos(a), rng.uniform(-1, 1), 8 * np.sin(a)]) * rng.uniform(0.8, 1.3)
        z = -C / np.linalg.norm(C)
        x = np.cross([0.0, 1.0, 0.0], z); x /= np.linalg.norm(x)
        R = np.stack([x, np.cross(z, x), z])
        cams[k, :3] = Rotation.from_matrix(R).as_rotvec()
        cams[k, 3:] = -R @ C
    return cams


def make_problem(rng, ncam, npt, lengths, noise=0.3, displaced=0.1, perturb=0.002):
    """Point-major observations: track t is seen by lengths[t] distinct cameras (ascending) -> dict of the BA inputs and the plan."""
    truth = random_cams(rng, ncam)
    X = rng.normal(0, 0.6, (npt, 3))
    lengths = np.minimum(np.asarray(lengths, np.int64), ncam)
    pt_idx = np.repeat(np.arange(npt), lengths).astype(np.int32)
    cam_idx = (np.concatenate([np.sort(rng.permutation(ncam)[:n]) for n in lengths]) if len(pt_idx) else np.zeros(0)).astype(np.int32)
    nobs = len(pt_idx)
    obs = np_ba.project(truth[cam_idx], K, X[pt_idx][:, None, :])[:, 0] + rng.normal(0, noise, (nobs, 2)) if nobs else np.zeros((0, 2))
    hit = rng.random(nobs) < displaced
    obs[hit] += rng.uniform(20, 100, (int(hit.sum()), 1)) * np.sign(rng.normal(size=(int(hit.sum()), 2)))
    cams = truth * (1 + perturb * rng.standard_normal(truth.shape))
    X0 = X + rng.normal(0, 0.01, X.shape)
    off, coff, cobs = nb.plan(cam_idx, pt_idx, ncam, npt)
    return dict(cams=cams, X=X0, obs=obs.astype(np.float32), cam_idx=cam_idx, pt_idx=pt_idx, track_off=off, cam_off=coff, cam_obs=cobs, truth=truth)


def gen_problem(rng, max_obs=MAX_OBS, deg=None):
    """A random problem; one in four with a degeneracy (deg 0..8)."""
    if deg is None:
        deg = int(rng.integers(9)) if rng.integers(4) == 0 else -1
    ncam = int(rng.choice([1, 2, 3, 8, 64, 65]))
    nobs_target = 0 if deg == 0 else log_uniform_from_zero(rng, max_obs)
    mean_len = int(rng.choice([2, 3, min(ncam, 16)]))
    npt = max(1, nobs_target // max(mean_len, 1))
    lengths = np.full(npt, mean_len) if nobs_target else np.zeros(npt, np.int64)
    if nobs_target and rng.integers(2):
        lengths = rng.integers(0, 2 * mean_len + 1, npt)
    p = make_problem(rng, ncam, npt, lengths)
    nobs = len(p["obs"])
    bad = [-1, ncam, npt, INT32_MAX]
    pick = lambda n, share=0.05: np.flatnonzero(rng.random(n) < share)  # noqa: E731
    if deg == 1 and nobs:
        p["obs"][pick(nobs), int(rng.integers(2))] = np.nan
    if deg == 2:
        p["X"][pick(npt, 0.1), int(rng.integers(3))] = rng.choice([np.nan, np.inf])
    if deg == 3 and nobs:                                                    # points beyond the centre of a camera that sees them
        for o in pick(nobs, 0.03):
            C = nb.centres(p["cams"])[p["cam_idx"][o]]
            p["X"][p["pt_idx"][o]] = C + 1.5 * (C - p["X"][p["pt_idx"][o]])
    if deg == 4 and nobs:                                                    # the CSRs stay those of the true indices
        rows = pick(nobs)
        p["cam_idx"][rows] = rng.choice(bad, len(rows))
        rows = pick(nobs)
        p["pt_idx"][rows] = rng.choice(bad, len(rows))
    if deg == 5 and nobs:
        rows = pick(nobs)
        p["cam_obs"][rows] = rng.choice(bad + [nobs], len(rows))
    if deg == 6:
        for name in ("track_off", "cam_off"):
            rows = pick(len(p[name]), 0.1)
            p[name][rows] = rng.choice([-5, nobs + 7, INT32_MAX, 0, nobs // 2], len(rows))
    if deg == 7 and ncam > 1 and nobs:                                       # a camera without observations
        gone = int(rng.integers(ncam))
        keep = p["cam_idx"] != gone
        p["obs"], p["cam_idx"], p["pt_idx"] = p["obs"][keep], p["cam_idx"][keep], p["pt_idx"][keep]
        p["track_off"], p["cam_off"], p["cam_obs"] = nb.plan(p["cam_idx"], p["pt_idx"], ncam, npt)
    p["huber"] = 1e-3 if deg == 8 else float(rng.choice([0.5, 1.0, 3.0, np.inf]))
    p["deg"] = deg
    return p


# ---- device side ----------------------------------------------------------------------------------------------------------

def padded(shape, dtype, extra=2):
    """A sentinel-filled device buffer with `extra` rows behind the `shape` the call sees -> (whole, view)."""
    import torch
    size = torch.empty(0, dtype=dtype).element_size()
    if size == 1:
        whole = torch.full((shape[0] + 8,), SENTINEL & 0xFF, dtype=torch.uint8, device="cuda")
    else:
        rows, width = shape[0] + extra, int(np.prod(shape[1:]))
        whole = torch.full((rows * width * size // 4,), SENTINEL, dtype=torch.int32, device="cuda").view(dtype).view((rows,) + tuple(shape[1:]))
    return whole, whole[:shape[0]]


def untouched(whole, rows):
    import torch
    tail = whole[rows:].contiguous().reshape(-1)
    if tail.element_size() == 1:
        return bool((tail == (SENTINEL & 0xFF)).all())
    return bool((tail.view(torch.int32) == SENTINEL).all())


def device_plan(p):
    from sfm_mvs_amd import track_ba
    return track_ba.Plan(len(p["cams"]), len(p["X"]), dev(p["track_off"].astype(np.int32)), dev(p["cam_idx"].astype(np.int32)),
                         dev(p["pt_idx"].astype(np.int32)), dev(p["cam_off"].astype(np.int32)), dev(p["cam_obs"].astype(np.int32)))


def device_sweep(pl, p, cams, X, huber, mode=0, active=None, ws=None):
    """The sweep into sentinel-padded outputs -> (out dict of views, message if a word past a size was written)."""
    import torch
    from sfm_mvs_amd import track_ba
    bufs = dict(JtJ_cam=padded((pl.ncam, 36), torch.float64), Jtr_cam=padded((pl.ncam, 6), torch.float64), JtJ_pt=padded((pl.npt, 9), torch.float64),
                Jtr_pt=padded((pl.npt, 3), torch.float64), stat=padded((2,), torch.float64), count=padded((3,), torch.int32))
    act_whole = None
    if active is None:
        act_whole, active = padded((pl.nobs,), torch.uint8)
    out = track_ba.sweep(pl, dev(cams), K, dev(X), dev(p["obs"]), huber, mode, active, ws, out={k: v[1] for k, v in bufs.items()})
    for name, (whole, view) in bufs.items():
        if not untouched(whole, view.shape[0]):
            return out, f"{name}: written past its size"
    if act_whole is not None and not untouched(act_whole, pl.nobs):
        return out, "active: written past its size"
    return out, ""


def close(name, got, want, tol=TOL):
    import torch
    g = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    w = np.asarray(want, np.float64).reshape(g.shape)
    if not np.isfinite(g).all():
        return f"{name}: not finite"
    scale = np.abs(w).max() if w.size else 0.0
    err = np.abs(g - w).max() if w.size else 0.0
    return "" if err <= tol * scale else f"{name}: |got - want| {err:.3g} > {tol:g} * {scale:.3g} at {np.unravel_index(np.argmax(np.abs(g - w)), g.shape)}"


def compare_sweep(pl, out, want):
    from sfm_mvs_amd import track_ba
    if not np.array_equal(out["active"].cpu().numpy(), want["active"]):
        return f"active: differs at {np.flatnonzero(out['active'].cpu().numpy() != want['active'])[:3].tolist()}"
    if out["count"].cpu().numpy().tolist() != want["count"].tolist():
        return f"count: {out['count'].cpu().numpy().tolist()} vs {want['count'].tolist()}"
    return (close("rows", track_ba.rows_of(pl, out["ws"]), want["rows"]) or close("stat", out["stat"], want["stat"]) or
            close("JtJ_cam", out["JtJ_cam"], want["B"].reshape(-1, 36)) or close("Jtr_cam", out["Jtr_cam"], want["gc"]) or
            close("JtJ_pt", out["JtJ_pt"], want["C"].reshape(-1, 9)) or close("Jtr_pt", out["Jtr_pt"], want["gp"]))


def want_sweep(p, cams, X, huber, active=None):
    return nb.sweep(cams, K, X, p["obs"], p["cam_idx"], p["pt_idx"], p["track_off"], p["cam_off"], p["cam_obs"], huber, active)


def check_sweep(p, huber=None, trial=None):
    """Mode 0 at (cams, X), then mode 1 at `trial` = (cams', X') (default: a small random move) with the first sweep's active set."""
    huber = p["huber"] if huber is None else huber
    pl = device_plan(p)
    out, msg = device_sweep(pl, p, p["cams"], p["X"], huber)
    want = want_sweep(p, p["cams"], p["X"], huber)
    msg = msg or compare_sweep(pl, out, want)
    if msg:
        return "mode 0 " + msg, out, want
    if trial is None:
        rng = np.random.default_rng(len(p["obs"]))
        trial = (p["cams"] * (1 + 1e-3 * rng.standard_normal(p["cams"].shape)), p["X"] + rng.normal(0, 0.02, p["X"].shape))
    out1, msg = device_sweep(pl, p, trial[0], trial[1], huber, 1, out["active"], pl.workspace())
    want1 = want_sweep(p, trial[0], trial[1], huber, want["active"])
    msg = msg or compare_sweep(pl, out1, want1)
    return ("mode 1 " + msg if msg else ""), out, want


def check_product(p, seed=0):
    from sfm_mvs_amd import track_ba
    pl = device_plan(p)
    out, msg = device_sweep(pl, p, p["cams"], p["X"], p["huber"])
    if msg:
        return msg
    rows = track_ba.rows_of(pl, out["ws"]).cpu().numpy()
    rng = np.random.default_rng(seed)
    x, v = rng.normal(size=(pl.ncam, 6)), rng.normal(size=(pl.npt, 3))
    u = track_ba.product(pl, out["ws"], dev(x), 0)
    w = track_ba.product(pl, out["ws"], dev(v), 1)
    args = (rows, p["cam_idx"], p["pt_idx"], p["track_off"], p["cam_off"], p["cam_obs"], pl.ncam, pl.npt)
    msg = close("W^T x", u, nb.product(*args, x, 0)) or close("W v", w, nb.product(*args, v, 1))
    if msg or p["deg"] in (4, 5, 6):                                         # inconsistent CSRs: the two sides see different observations
        return msg
    un, wn = u.cpu().numpy(), w.cpu().numpy()
    lhs, rhs, scale = float((v * un).sum()), float((x * wn).sum()), float((np.abs(v) * np.abs(un)).sum() + (np.abs(x) * np.abs(wn)).sum())
    return "" if abs(lhs - rhs) <= 1e-11 * scale else f"adjointness: {lhs!r} vs {rhs!r} (scale {scale:.3g})"


def reduced_system(B, C, gc, gp, W, lam, fix_first):
    """(S, rhs, Cinv, W matrix) of the damped step in NumPy, singular blocks as the header treats them."""
    ncam, npt = len(B), len(C)
    _, bad_p = nb.singular_blocks(B, C, lam)
    d6, d3 = np.arange(6), np.arange(3)
    Bd, Cd = B.copy(), C.copy()
    Bd[:, d6, d6] *= 1 + lam
    Cd[:, d3, d3] *= 1 + lam
    Cd[bad_p] = np.eye(3)
    Cinv = np.linalg.inv(Cd)
    Cinv[bad_p] = 0.0
    Wm = W.transpose(0, 2, 1, 3).reshape(6 * ncam, 3 * npt)
    Y = np.einsum("ijab,jbc->ijac", W, Cinv).transpose(0, 2, 1, 3).reshape(6 * ncam, 3 * npt)
    S = -Y @ Wm.T
    for i in range(ncam):
        S[6 * i:6 * i + 6, 6 * i:6 * i + 6] += Bd[i]
    rhs = gc.ravel() - Y @ gp.ravel()
    if fix_first:
        S[:6], S[:, :6], rhs[:6] = 0.0, 0.0, 0.0
    return S, rhs, Cinv, Wm


def check_step(p, lam=1e-3, fix_first=True, cg_tol=1e-10, cg_iters=400):
    from sfm_mvs_amd import track_ba
    pl = device_plan(p)
    out, msg = device_sweep(pl, p, p["cams"], p["X"], p["huber"])
    if msg:
        return msg
    dc, dp, it, status = track_ba.step(pl, out, lam, fix_first, cg_tol, cg_iters)
    B, C = out["JtJ_cam"].cpu().numpy().reshape(-1, 6, 6), out["JtJ_pt"].cpu().numpy().reshape(-1, 3, 3)
    gc, gp = out["Jtr_cam"].cpu().numpy(), out["Jtr_pt"].cpu().numpy()
    dc, dp = dc.cpu().numpy(), dp.cpu().numpy()
    if not (np.isfinite(dc).all() and np.isfinite(dp).all()):
        return "step: not finite"
    bad_c, bad_p = nb.singular_blocks(B, C, lam)
    want_status = int(bad_c.any()) | 2 * int(bad_p.any())
    if status != want_status:
        return f"status {status} vs {want_status}"
    if fix_first and dc[0].any():
        return "step: camera 0 moved"
    if dp[bad_p].any():
        return "step: a point with a singular block moved"
    W = nb.dense_w(track_ba.rows_of(pl, out["ws"]).cpu().numpy(), p["cam_idx"], p["pt_idx"], pl.ncam, pl.npt)
    S, rhs, Cinv, Wm = reduced_system(B, C, gc, gp, W, lam, fix_first)
    msg = close("dp", dp, np.einsum("jab,jb->ja", Cinv, (gp.ravel() - Wm.T @ dc.ravel()).reshape(-1, 3)))
    if msg or it >= cg_iters:
        return msg
    res, scale = np.linalg.norm(S @ dc.ravel() - rhs), np.linalg.norm(rhs)
    return "" if res <= 10 * cg_tol * scale else f"step: |S dc - rhs| {res:.3g} > 10 * {cg_tol:g} * {scale:.3g} after {it} iterations"


def check_composed(p, iters=4):
    import torch
    from sfm_mvs_amd import track_ba
    huber = None if np.isinf(p["huber"]) else p["huber"]
    try:
        wc, wX, whist, winfo = nb.bundle_adjust(p["cams"], K, p["X"], p["obs"], p["cam_idx"], p["pt_idx"], huber, iters)
    except np.linalg.LinAlgError:                                             # a reduced system the direct solve cannot take: no reference
        return ""
    c, X, hist, info = track_ba.bundle_adjust_tracks(dev(p["cams"]), K, dev(p["X"]), dev(p["obs"]), dev(p["cam_idx"]), dev(p["pt_idx"]), huber, iters)
    if X.dtype != torch.float64 or abs(len(hist) - len(whist)) > 1:
        return f"composed: {len(hist)} vs {len(whist)} history entries"
    n = min(len(hist), len(whist))
    if not np.allclose(hist[:n], whist[:n], rtol=1e-6, atol=1e-12):
        return f"composed: history {hist[:n]} vs {whist[:n]}"
    return "" if info["active"] == winfo["active"] else f"composed: active {info['active']} vs {winfo['active']}"


def fuzz_sweep(rng):
    return check_sweep(gen_problem(rng))[0]


def fuzz_product(rng):
    return check_product(gen_problem(rng), int(rng.integers(1 << 30)))


def fuzz_step(rng):
    p = gen_problem(rng, 1 << 10, deg=int(rng.choice([0, 1, 2, 7])) if rng.integers(4) == 0 else -1)
    return check_step(p, float(rng.choice([1e-3, 1e-1, 1.0])), bool(rng.integers(2)))


def fuzz_composed(rng):
    ncam, npt = int(rng.integers(2, 7)), max(4, log_uniform_from_zero(rng, 64))
    p = make_problem(rng, ncam, npt, np.maximum(2, rng.integers(ncam // 2 + 1, ncam + 1, npt)))
    p["huber"], p["deg"] = float(rng.choice([1.0, 3.0, np.inf])), -1
    if rng.integers(4) == 0 and len(p["obs"]):
        p["obs"][rng.integers(len(p["obs"]))] = np.nan
    return check_composed(p)


FAMILIES = [("sweep", fuzz_sweep, 3), ("product", fuzz_product, 2), ("step", fuzz_step, 2), ("composed", fuzz_composed, 1)]


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
            log(f"MISMATCH {name} (seed {seed}, case seed {case_seed}; replay: fuzz_track_ba.py 0 0 {name}:{case_seed}) {msg}")
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
        print(f"fuzz_track_ba replay {name}:{case_seed}: {msg or 'no mismatch'}")
        return 1 if msg else 0
    counts, bad, dt = run(budget, seed, log=lambda s: print(s, flush=True))
    print(f"fuzz_track_ba: seed {seed}, {sum(counts.values())} cases {counts}, {bad} mismatches, {dt:.0f} s")
    print(f"sfm_build_id {_lib.build_id()}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
