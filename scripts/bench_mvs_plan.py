"""Times the MVS-PLAN family on the bench scene of docs/tracks.md §5 through run_tracks (64 images x 10 000 features, 2 016 pairs, 7 000
tracks of 64 observations = 448 000 observations) and writes one JSON line (default: profiles/mvs_plan_bench.json).

  python scripts/bench_mvs_plan.py [--images 64] [--out PATH] [--once] [--no-host] [--yardstick-lib PATH]

HIP events on the current stream, the median of 10 calls after 3 warm-ups: sfm_view_pair_counts, sfm_view_depth_ranges,
sfm_view_select and mvs_plan.plan_views.  The byte floors count every word of the inputs and outputs once, over 6.3 TB/s.  The
yardstick is the same plan computed on the host by tests/np_mvs_plan.py (wall time, one run).  --once runs every entry point once and
leaves (for a kernel trace collected in a run of its own).  --yardstick-lib names a shared library built outside the tree that exports
`naive_pair_counts` (a lane per pair, global atomics only; the signature is in the code below): it is run on the same input, checked
against the library's counts and timed the same way."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mvs_plan_bench.json"))
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--yardstick-lib", default=None)
    args = ap.parse_args()
    import torch
    import np_mvs_plan as npl
    from datagen import ring_scene
    from sfm_mvs_amd import _lib, mvs_plan, sharded, track_ba, tracks
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
    X, Pd = up(got["points"].astype(np.float64)), up(np.asarray(P, np.float64).reshape(n_img, 12))
    ncam, npt, nobs = n_img, len(got["points"]), len(got["obs"])
    pl = track_ba.plan(up(got["cam_idx"]), up(got["pt_idx"]), ncam, npt)
    window = (1.0, 60.0)                    # the ring's neighbours stand 360 / 64 degrees apart: the window admits the nearest ten
    cos_lo, cos_hi = mvs_plan.cos_window(*window)
    pc = mvs_plan.pair_counts(pl, X, Pd, cos_lo, cos_hi)
    dr = mvs_plan.depth_ranges(pl, X, Pd, 20, 980)
    sel = mvs_plan.select(pc[0], pc[1], 4, 8)
    planned = mvs_plan.plan_views(pl, X, Pd, 4, window[0], window[1], 8)
    torch.cuda.synchronize()
    if args.once:
        print("bench_mvs_plan: one pass done")
        return 0
    t_pairs = timed(lambda: mvs_plan.pair_counts(pl, X, Pd, cos_lo, cos_hi, out=pc))
    t_ranges = timed(lambda: mvs_plan.depth_ranges(pl, X, Pd, 20, 980, out=dr))
    t_select = timed(lambda: mvs_plan.select(pc[0], pc[1], 4, 8, out=sel))
    t_plan = timed(lambda: mvs_plan.plan_views(pl, X, Pd, 4, window[0], window[1], 8))
    hp = mvs_plan.host_plan(planned)
    t_naive = None
    if args.yardstick_lib:
        import ctypes
        from sfm_mvs_amd._lib import ptr, stream_ptr
        naive = ctypes.CDLL(os.path.abspath(args.yardstick_lib)).naive_pair_counts
        naive.restype = ctypes.c_int
        naive.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_longlong] * 3 + [ctypes.c_int, ctypes.c_double, ctypes.c_double] + [ctypes.c_void_p] * 3
        ns, ng = torch.empty_like(pc[0]), torch.empty_like(pc[1])
        lmax = int(torch.diff(pl.track_off).max())
        run_naive = lambda: naive(ptr(pl.track_off), ptr(pl.cam_idx), ptr(X), ptr(pc[2]), npt, nobs, ncam, lmax, cos_lo, cos_hi, ptr(ns), ptr(ng),  # noqa: E731
                                  stream_ptr())
        assert run_naive() == 0
        assert torch.equal(ns, pc[0]) and torch.equal(ng, pc[1]), "the yardstick's counts differ"
        t_naive = timed(run_naive)
    lengths = np.diff(pl.track_off.cpu().numpy().astype(np.int64))
    contributions = int((lengths * (lengths - 1) // 2).sum())
    host = None
    if not args.no_host:
        t0 = time.perf_counter()
        want = npl.plan_views(got["cam_idx"], got["pt_idx"], got["points"].astype(np.float64), P, 4, window[0], window[1], 8)
        host = time.perf_counter() - t0
        assert want["neighbours"] == hp["neighbours"] and np.array_equal(want["ranges"].view(np.int64), hp["ranges"].view(np.int64))
        assert np.array_equal(want["shared"], hp["shared"]) and np.array_equal(want["good"], hp["good"])
    pair_bytes = (npt + 1) * 4 + nobs * 4 + npt * 24 + ncam * (96 + 24) + 2 * ncam * ncam * 4
    range_bytes = (ncam + 1) * 4 + nobs * 12 + npt * 24 + ncam * (96 + 12)
    select_bytes = 2 * ncam * ncam * 4 + ncam * (4 * 4 + 4)
    floors = {"pair_counts": 1e6 * pair_bytes / HBM_BYTES_PER_S, "depth_ranges": 1e6 * range_bytes / HBM_BYTES_PER_S,
              "select": 1e6 * select_bytes / HBM_BYTES_PER_S}
    res = {"workload": f"view planning on the all-pairs ring scene: {ncam} cameras, {npt} tracks, {nobs} observations, {contributions} pair contributions",
           "ms_median_min": {"pair_counts": t_pairs, "depth_ranges": t_ranges, "select": t_select, "plan_views": t_plan},
           "byte_floor_us": floors, "bytes": {"pair_counts": pair_bytes, "depth_ranges": range_bytes, "select": select_bytes},
           "factor_over_floor": {"pair_counts": 1e3 * t_pairs[0] / floors["pair_counts"], "depth_ranges": 1e3 * t_ranges[0] / floors["depth_ranges"],
                                 "select": 1e3 * t_select[0] / floors["select"]},
           "pair_contributions_per_s": contributions / (1e-3 * t_pairs[0]), "host_numpy_plan_s": host,
           "naive_lane_per_pair_ms_median_min": t_naive, "naive_over_pair_counts": None if t_naive is None else t_naive[0] / t_pairs[0],
           "neighbours_of_view_0": hp["neighbours"][0], "range_of_view_0": hp["ranges"][0].tolist(), "window_deg": window,
           "library": os.path.basename(_lib.LIB_PATH), "build_id_mvs_plan": _lib.code_hashes_of_binary().get("mvs_plan.hip")}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
