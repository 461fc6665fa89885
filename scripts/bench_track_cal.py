"""Times the TRACKS-CAL family against TRACKS-BA on a problem of §9's bench shape (64 cameras of datagen.ring_cameras, 7 000 tracks
seen by every camera = 448 000 observations, 0.3 px of noise, the cameras perturbed as in the tests; built directly, without the
matching that docs/tracks.md §9 goes through) and writes one JSON line (default: profiles/track_cal_bench.json).

  python scripts/bench_track_cal.py [--out PATH] [--once]

HIP events on the current stream, the median of 10 calls after 3 warm-ups, the calibrated call and the §9 call on the same data
ALTERNATING call by call in one process: the sweep, a product pair, one step of 25 CG iterations (cg_tol = 0), and the wall time of
a 4-iteration adjustment.  The byte floors count every word of the inputs and outputs once, over 6.3 TB/s, a product pair as
scripts/bench_track_ba.py counts it (the row columns the pair uses once).  --once runs every entry point once and leaves (for a kernel
trace collected in a run of its own)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bench_track_ba import HBM_BYTES_PER_S, alternating
from bench_tracks import timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_cal_bench.json"))
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    import torch
    import np_track_cal as nc
    from datagen import ring_cameras
    from sfm_mvs_amd import _lib, track_ba, track_cal
    dev = torch.device("cuda:0")
    ncam, npt = 64, 7000
    rng = np.random.default_rng(11)
    truth = ring_cameras(ncam)
    Xt = rng.uniform(-1.5, 1.5, (npt, 3))
    pi_h, ci_h = np.repeat(np.arange(npt), ncam).astype(np.int32), np.tile(np.arange(ncam), npt).astype(np.int32)
    theta_true = np.array([900.0, 480.0, 320.0, -0.12, 0.03])
    obs_h = (nc.project(truth[ci_h], theta_true, 1.0, Xt[pi_h]) + rng.normal(0, 0.3, (len(pi_h), 2))).astype(np.float32)
    K = np.array([[1000.0, 0, 480], [0, 1000.0, 320], [0, 0, 1]])
    theta, aspect = track_cal.theta_of(K)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    cams = up(truth * (1 + 0.002 * np.random.default_rng(4).standard_normal((ncam, 6))))
    X, obs, ci, pi = up(Xt + rng.normal(0, 0.01, Xt.shape)), up(obs_h), up(ci_h), up(pi_h)
    nobs = len(obs_h)

    pl = track_ba.plan(ci, pi, ncam, npt)
    ws_ba, ws_cal = pl.workspace(), track_cal.workspace(pl)
    first_ba = track_ba.sweep(pl, cams, K, X, obs, 1.0, ws=ws_ba)
    first_cal = track_cal.sweep(pl, cams, theta, aspect, X, obs, 1.0, ws=ws_cal)
    x, xi, v = (torch.randn(s, dtype=torch.float64, device=dev) for s in ((ncam, 6), (5,), (npt, 3)))
    cal_sweep = lambda: track_cal.sweep(pl, cams, theta, aspect, X, obs, 1.0, ws=ws_cal, out=first_cal)  # noqa: E731
    ba_sweep = lambda: track_ba.sweep(pl, cams, K, X, obs, 1.0, ws=ws_ba, out=first_ba)  # noqa: E731
    cal_pair = lambda: (track_cal.product(pl, ws_cal, x, 0, xi), track_cal.product(pl, ws_cal, v, 1))  # noqa: E731
    ba_pair = lambda: (track_ba.product(pl, ws_ba, x, 0), track_ba.product(pl, ws_ba, v, 1))  # noqa: E731
    cal_step = lambda: track_cal.step(pl, first_cal, 1e-3, 9, True, 0.0, 25)  # noqa: E731
    ba_step = lambda: track_ba.step(pl, first_ba, 1e-3, True, 0.0, 25)  # noqa: E731
    frames = torch.randint(0, 256, (16, 648, 968, 3), dtype=torch.uint8, device=dev)
    px = torch.rand((640_000, 2), dtype=torch.float32, device=dev) * 900
    dist = (-0.12, 0.03)
    und_px = lambda: track_cal.undistort_points(px, K, dist)  # noqa: E731
    und_im = lambda: track_cal.undistort_images(frames, K, dist, None, True)  # noqa: E731
    for fn in (cal_sweep, ba_sweep, cal_pair, ba_pair, cal_step, ba_step, und_px, und_im):
        fn()
    torch.cuda.synchronize()
    if args.once:
        track_cal.bundle_adjust_calibrated(cams, K, None, X, obs, ci, pi, huber=1.0, iters=1)
        torch.cuda.synchronize()
        print("bench_track_cal: one pass done")
        return 0

    t_sweep, t_sweep_ba = alternating(cal_sweep, ba_sweep)
    t_pair, t_pair_ba = alternating(cal_pair, ba_pair)
    t_step, t_step_ba = alternating(cal_step, ba_step)
    t_px, t_im = timed(und_px), timed(und_im)
    variants = (("calibrated_f_k1", lambda: track_cal.bundle_adjust_calibrated(cams, K, None, X, obs, ci, pi, huber=1.0, iters=4)),
                ("tracks_ba", lambda: track_ba.bundle_adjust_tracks(cams, K, X, obs, ci, pi, huber=1.0, iters=4)))
    wall, extra = {name: [] for name, _ in variants}, {}
    for rep in range(6):
        for name, fn in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            if rep:
                wall[name].append(time.perf_counter() - t0)
            extra[name] = dict(history=[float(h) for h in out[-2]], cg_iters=out[-1]["cg_iters"])
            if name == "calibrated_f_k1":
                extra[name].update(f=float(out[2][0, 0]), k1=float(out[3][0]))
    walls = {name: dict(wall_s_median=float(np.median(w)), wall_s_min=float(min(w)), wall_s_all=[round(t, 6) for t in w], **extra[name]) for name, w in wall.items()}
    row = lambda r: nobs * (8 + 4 + 4 + 4 + 8 * r + 1)  # noqa: E731  obs, cam_idx, pt_idx, cam_obs, the row, active
    sweep_bytes = row(30) + npt * (24 + 4 + 96 + 120) + ncam * (48 + 4 + 336 + 240) + 28 + 240
    sweep_bytes_ba = row(20) + npt * (24 + 4 + 96) + ncam * (48 + 4 + 336) + 28
    # a product pair in the convention of scripts/bench_track_ba.py: the columns of the rows that the pair uses ONCE (Jc and Jp, 18 doubles;
    # here Jc, Ji and Jp, 28), the three index arrays, the vectors in and out; a kernel that reads a row again is above the floor by that
    pair = lambda r: nobs * (8 * r + 4 + 4 + 4) + npt * (4 + 24 + 24) + ncam * (4 + 48 + 48)  # noqa: E731
    px_bytes, im_bytes = px.numel() * 4 * 2, frames.numel() * 2 + frames.numel() // 3
    us = lambda b: 1e6 * b / HBM_BYTES_PER_S  # noqa: E731
    res = {"workload": f"self-calibrating track bundle adjustment, the shape of §9's bench problem built directly: {ncam} cameras, {npt} tracks, {nobs} observations",
           "ms_median_min": {"cal_sweep": t_sweep[:2], "ba_sweep": t_sweep_ba[:2], "cal_product_pair": t_pair[:2], "ba_product_pair": t_pair_ba[:2],
                             "cal_step_25_cg": t_step[:2], "ba_step_25_cg": t_step_ba[:2], "undistort_points_640k": t_px, "undistort_images_16x648x968x3": t_im},
           "ms_all": {"cal_sweep": t_sweep[2], "ba_sweep": t_sweep_ba[2], "cal_product_pair": t_pair[2], "ba_product_pair": t_pair_ba[2],
                      "cal_step_25_cg": t_step[2], "ba_step_25_cg": t_step_ba[2]},
           "cal_over_ba": {"sweep": t_sweep[0] / t_sweep_ba[0], "product_pair": t_pair[0] / t_pair_ba[0], "step_25_cg": t_step[0] / t_step_ba[0],
                           "adjust_4_iterations": walls["calibrated_f_k1"]["wall_s_median"] / walls["tracks_ba"]["wall_s_median"]},
           "byte_floor_us": {"cal_sweep": us(sweep_bytes), "ba_sweep": us(sweep_bytes_ba), "cal_product_pair": us(pair(28) + 80), "ba_product_pair": us(pair(18)),
                             "undistort_points": us(px_bytes), "undistort_images": us(im_bytes)},
           "bytes": {"cal_sweep": sweep_bytes, "ba_sweep": sweep_bytes_ba, "undistort_points": px_bytes, "undistort_images": im_bytes},
           "bundle_adjust_4_iterations": walls, "library": os.path.basename(_lib.LIB_PATH),
           "build_id_tracks_cal": _lib.code_hashes_of_binary().get("tracks_cal.hip"), "build_id_tracks_ba": _lib.code_hashes_of_binary().get("tracks_ba.hip")}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
