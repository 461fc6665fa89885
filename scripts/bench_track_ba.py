"""Times the TRACKS-BA family on the bench scene of docs/tracks.md §5 (64 images x 10 000 features, 2 016 pairs, 7 000 tracks of 64
observations = 448 000 observations; the cameras perturbed as in the tests) and writes one JSON line (default:
profiles/track_ba_bench.json).

  python scripts/bench_track_ba.py [--images 64] [--out PATH] [--once] [--kernels-only]

HIP events on the current stream, the median of 10 calls after 3 warm-ups: `plan`, the sweep, a product pair, one step.  The yardstick
is the older sparse path ON THE SAME INPUT IN THE SAME PROCESS, the two ALTERNATING call by call: ops.project_residual with all
Jacobian blocks against the sweep, ops.ba_schur_wt + ops.ba_schur_w with indices against a product pair, and the wall time of
ba.bundle_adjust_schur(..., cam_idx, pt_idx, iters=4) against bundle_adjust_tracks at 4 iterations.  The byte floors count every word
of the inputs and outputs once, over 6.3 TB/s.
--once runs every entry point once and leaves (for a kernel trace collected in a run of its own); --kernels-only leaves out the
whole adjustments (for a build with another SFM_TBA_GROUP, loaded through SFM_HIP_LIB)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bench_tracks import timed

HBM_BYTES_PER_S = 6.3e12


def alternating(new, old, warm=3, reps=10):
    """Event times (ms) of `new` and `old`, one call of each in turn -> ((median, min, all) new, (median, min, all) old)."""
    import torch
    for _ in range(warm):
        new(); old()
    ms = ([], [])
    for _ in range(reps):
        for k, fn in enumerate((new, old)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return tuple((float(np.median(m)), float(min(m)), [round(v, 4) for v in m]) for m in ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_ba_bench.json"))
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--kernels-only", action="store_true")
    args = ap.parse_args()
    import torch
    from datagen import ring_scene
    from sfm_mvs_amd import _lib, ba, ops, sharded, track_ba, tracks
    dev = torch.device("cuda:0")
    n_img, n_desc, n_scene = args.images, 10_000, 7_000
    K, P, image = ring_scene(n_img, n_desc, n_scene, seed=11)
    ims = [image(k) for k in range(n_img)]
    kps = [torch.from_numpy(im[0]).to(dev) for im in ims]
    des = [torch.from_numpy(im[1]).to(dev) for im in ims]
    pairs = sharded.all_pairs(n_img)
    store, nq = sharded.match_pairs_sharded(des, pairs, batch=8)
    del des
    got = tracks.run_tracks(store.contiguous(), nq, pairs, kps, P)
    del store
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    cams_h = track_ba.cams_from_P(P, K) * (1 + 0.002 * np.random.default_rng(4).standard_normal((n_img, 6)))
    cams, X64, X32, obs = up(cams_h), up(got["points"].astype(np.float64)), up(got["points"]), up(got["obs"])
    ci, pi = up(got["cam_idx"]), up(got["pt_idx"])
    ncam, npt, nobs = n_img, len(got["points"]), len(got["obs"])

    pl = track_ba.plan(ci, pi, ncam, npt)
    ws = pl.workspace()
    first = track_ba.sweep(pl, cams, K, X64, obs, 1.0, ws=ws)
    x, v = torch.randn((ncam, 6), dtype=torch.float64, device=dev), torch.randn((npt, 3), dtype=torch.float64, device=dev)
    new_pair = lambda: (track_ba.product(pl, ws, x, 0), track_ba.product(pl, ws, v, 1))  # noqa: E731
    old_pair = lambda: (ops.ba_schur_wt(cams, K, X32, x, ci, pi), ops.ba_schur_w(cams, K, X32, v, ci, pi))  # noqa: E731
    old_sweep = lambda: ops.project_residual(cams, K, X32, obs, ci, pi, want_proj=False, want_jac=True, want_pt_jac=True, want_res2=True)  # noqa: E731
    new_sweep = lambda: track_ba.sweep(pl, cams, K, X64, obs, 1.0, ws=ws, out=first)  # noqa: E731
    new_pair(); old_pair(); old_sweep(); new_sweep()
    dc, dp, it, status = track_ba.step(pl, first, 1e-3)
    torch.cuda.synchronize()
    if args.once:
        track_ba.bundle_adjust_tracks(cams, K, X64, obs, ci, pi, huber=1.0, iters=1)
        ba.bundle_adjust_schur(cams, K, X32, obs, ci, pi, iters=1)
        torch.cuda.synchronize()
        print("bench_track_ba: one pass done")
        return 0

    t_plan = timed(lambda: track_ba.plan(ci, pi, ncam, npt))
    t_sweep, t_sweep_old = alternating(new_sweep, old_sweep)
    t_pair, t_pair_old = alternating(new_pair, old_pair)
    t_step = timed(lambda: track_ba.step(pl, first, 1e-3))
    # the whole adjustment at 4 iterations, wall, the two ALTERNATING after one untimed call of each; plain least squares on both sides
    # (the old path has no loss), and the new path with the Huber loss beside them
    variants = (("tracks_l2", lambda: track_ba.bundle_adjust_tracks(cams, K, X64, obs, ci, pi, huber=None, iters=4)),
                ("schur_indexed", lambda: ba.bundle_adjust_schur(cams, K, X32, obs, ci, pi, iters=4)),
                ("tracks_huber", lambda: track_ba.bundle_adjust_tracks(cams, K, X64, obs, ci, pi, huber=1.0, iters=4)))
    wall, hist = {name: [] for name, _ in variants}, {}
    for rep in range(0 if args.kernels_only else 8):
        for name, fn in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            if rep:
                wall[name].append(time.perf_counter() - t0)
            hist[name] = [float(h) for h in out[2]]
    walls = {name: {"wall_s_median": float(np.median(w)), "wall_s_min": float(min(w)), "wall_s_all": [round(t, 6) for t in w], "history": hist[name]}
             for name, w in wall.items() if w}
    sweep_bytes = nobs * (8 + 4 + 4 + 4 + 160 + 1) + npt * (24 + 4 + 96) + ncam * (48 + 4 + 336) + 28
    pair_bytes = nobs * (144 + 4 + 4 + 4) + npt * (4 + 24 + 24) + ncam * (4 + 48 + 48)
    res = {"workload": f"track bundle adjustment on the all-pairs ring scene: {ncam} cameras, {npt} tracks, {nobs} observations",
           "ms_median_min": {"plan": t_plan, "sweep": t_sweep[:2], "project_residual": t_sweep_old[:2], "product_pair": t_pair[:2],
                             "schur_indexed_pair": t_pair_old[:2], "step": t_step},
           "ms_all": {"sweep": t_sweep[2], "project_residual": t_sweep_old[2], "product_pair": t_pair[2], "schur_indexed_pair": t_pair_old[2]},
           "sweep_over_project_residual": t_sweep[0] / t_sweep_old[0], "pair_over_schur_indexed": t_pair[0] / t_pair_old[0],
           "step_cg_iterations": it, "step_status": status,
           "byte_floor_us": {"sweep": 1e6 * sweep_bytes / HBM_BYTES_PER_S, "product_pair": 1e6 * pair_bytes / HBM_BYTES_PER_S},
           "bytes": {"sweep": sweep_bytes, "product_pair": pair_bytes}, "bundle_adjust_4_iterations": walls,
           "tracks_l2_over_schur_indexed": walls["tracks_l2"]["wall_s_median"] / walls["schur_indexed"]["wall_s_median"] if walls else None,
           "library": os.path.basename(_lib.LIB_PATH), "build_id_tracks_ba": _lib.code_hashes_of_binary().get("tracks_ba.hip")}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
