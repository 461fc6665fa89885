"""Plane-sweep MVS timings on one GPU -> one JSON line (docs/mvs.md).
  python scripts/bench_mvs.py [--calls 20] [--warmup 3] [--views 57] [--sweep-only]
- depth map of one full-size 968 x 648 reference (D = 128 planes, S = 4 sources, r = 3, top 2): median of `--calls` calls after
  `--warmup`, each timed by HIP events around the entry point's launch alone
- mvs.run_mvs over `--views` gustav_views frames (pose.csv's cameras, the reference's sparse cloud for the depth ranges): wall
  time of the whole call (per-view sweeps, consistency, compaction, the download), median of 3 after one warm-up; fused points
- evaluations w*h*D*S and their rate, an operation-count model (VALU lane-operations per evaluation, counted from the kernel's
  source, not measured) and the fraction of the FP32 VALU issue bound it implies
--sweep-only: the full-size sweep alone (for a rocprofv3 --kernel-trace --stats run)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

# VALU lane-operations per (pixel, plane, source), read off plane_sweep_kernel (a model):
#   warp of the tile + halo into LDS: (16 + 2r)^2 / 256 = 1.89 samples per pixel at r = 3, ~85 operations each (18 for the
#     homography, two correctly rounded divisions ~10 each, range tests, floor / convert / clamp, 4 byte gathers + converts,
#     bilinear 9 mul / add)                                                                                        ~160
#   row sums: (16 + 2r) / 16 = 1.375 halo rows per pixel x (2r + 1) terms x (2 products + 3 adds + 1 validity or)   ~58
#   column sums of the row sums: 2r x (3 adds + 1 or)                                                                ~24
#   ZNCC (three divisions by n, sqrt, a division, clamps) + the 8-slot sorted insertion (16 min / max)              ~60
OPS_PER_EVAL = 300
# FP32 VALU issue bound: 256 CUs x 4 SIMDs x 32 lanes / clock x 2.4 GHz (a wave issues one VALU instruction over 2 clocks)
VALU_LANE_OPS_PER_S = 256 * 4 * 32 * 2.4e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--views", type=int, default=57)
    ap.add_argument("--sweep-only", action="store_true")
    a = ap.parse_args()
    from datagen import gustav_views, sparse_points
    from sfm_mvs_amd import mvs
    from sfm_mvs_amd.sift import bgr2gray
    D, S, r, k = 128, 4, 3, 2
    nview = max(a.views, 5)
    images, K, P = gustav_views(nview, scale=1, seed=0)
    h, w = images[0].shape[:2]
    X = sparse_points()
    frames = [torch.from_numpy(im).cuda() for im in images]
    grays = [bgr2gray(f) for f in frames]
    i = 2
    nb = mvs.neighbours(i, nview, S)
    dmin, dmax = mvs.depth_range(X, P[i], P_all=P)
    invd = mvs.inverse_depths(dmin, dmax, D)
    mv = mvs.sweep_matrices(K, P[i], P[nb])
    srcs = [grays[v] for v in nb]
    for _ in range(a.warmup):
        mvs.plane_sweep(grays[i], srcs, mv, invd, r, k)
    # the timed calls go straight to the entry point with every argument marshalled beforehand: the event pair brackets the
    # launch alone, not the wrapper's allocations and checks
    import ctypes
    from sfm_mvs_amd import _lib
    depth = torch.empty((h, w), dtype=torch.float32, device="cuda")
    cost = torch.empty((h, w), dtype=torch.float32, device="cuda")
    src_ptrs = (ctypes.c_void_p * S)(*[t.data_ptr() for t in srcs])
    mv32 = np.ascontiguousarray(mv, np.float32)
    args = (_lib.ptr(grays[i]), src_ptrs, mv32.ctypes.data_as(ctypes.c_void_p), S, w, h, _lib.ptr(invd), D, r, k, float(mvs.VAR_MIN),
            float(mvs.COST_MAX), _lib.ptr(depth), _lib.ptr(cost), None, None, _lib.stream_ptr())
    L = _lib.lib()
    torch.cuda.synchronize()
    times = []
    for _ in range(a.calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(L.sfm_mvs_plane_sweep(*args), "sfm_mvs_plane_sweep")
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    sweep_ms = float(np.median(times))
    evals = w * h * D * S
    res = dict(metric="mvs_depth_map_ms", w=w, h=h, ndepth=D, nsrc=S, radius=r, topk=k, calls=a.calls,
               depth_map_ms_median=round(sweep_ms, 4), depth_map_ms_min=round(float(np.min(times)), 4),
               valid_fraction=round(float((depth > 0).float().mean()), 4), evaluations=evals,
               evaluations_per_s=round(evals / (sweep_ms * 1e-3), 1), model_valu_ops_per_eval=OPS_PER_EVAL,
               model_valu_bound_ms=round(evals * OPS_PER_EVAL / VALU_LANE_OPS_PER_S * 1e3, 4),
               model_fraction_of_valu_bound=round(evals * OPS_PER_EVAL / VALU_LANE_OPS_PER_S * 1e3 / sweep_ms, 4))
    if not a.sweep_only:
        posearr = np.hstack([K.ravel()] + [p.ravel() for p in P[:a.views]])
        fr = frames[:a.views]
        mvs.run_mvs(fr, K, posearr, X)
        torch.cuda.synchronize()
        walls, out = [], None
        for _ in range(3):
            t0 = time.perf_counter()
            out = mvs.run_mvs(fr, K, posearr, X)
            torch.cuda.synchronize()
            walls.append(time.perf_counter() - t0)
        res.update(run_mvs_views=a.views, run_mvs_ms_median=round(1e3 * float(np.median(walls)), 2), fused_points=int(len(out["points"])))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
