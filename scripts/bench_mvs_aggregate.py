"""Cost-volume aggregation timings on one GPU -> one JSON line (docs/mvs.md §7).
  python scripts/bench_mvs_aggregate.py [--calls 12] [--warmup 3] [--views 57] [--kernels-only]
- the three entry points on the cost volume of one full-size 968 x 648 reference of gustav_views (D = 128 planes, 4 sources,
  r = 3, top 2; shift 3, the default penalties, 8 and 4 directions): median of `--calls` calls after `--warmup`, each timed by
  HIP events around the entry point's launches alone; their sum against the sweep itself, timed the same way
- each against its streaming floor, bytes moved / 6.3 TB/s: shift reads the float volume and writes Q; aggregate reads Q once
  per direction, writes S in the first direction and reads + writes it in each of the others; depth reads S and Q once
- mvs.run_mvs over `--views` frames with and without aggregate: wall time of the whole call (median of 3 after one warm-up)
  and the fused point count
--kernels-only: one pass of the three entry points (for a rocprofv3 --kernel-trace --stats run)."""
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

HBM_BYTES_PER_S = 6.3e12


def timed(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times)), float(np.min(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--views", type=int, default=57)
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    from datagen import gustav_views, sparse_points
    from sfm_mvs_amd import _lib, mvs
    from sfm_mvs_amd.sift import bgr2gray
    D, S, r, k, shift = 128, 4, 3, 2, 3
    nview = max(a.views, 5)
    images, K, P = gustav_views(nview, scale=1, seed=0)
    h, w = images[0].shape[:2]
    X = sparse_points()
    frames = [torch.from_numpy(im).cuda() for im in images]
    grays = [bgr2gray(f) for f in frames]
    i = 2
    nb = mvs.neighbours(i, nview, S)
    invd = mvs.inverse_depths(*mvs.depth_range(X, P[i], P_all=P), D)
    mv = mvs.sweep_matrices(K, P[i], P[nb])
    srcs = [grays[v] for v in nb]
    vol = torch.empty((D, h, w), dtype=torch.float32, device="cuda")
    q = torch.empty((D, h, w), dtype=torch.uint16, device="cuda")
    s = torch.empty((D, h, w), dtype=torch.uint16, device="cuda")
    parent_depth = mvs.plane_sweep(grays[i], srcs, mv, invd, r, k, volume_out=vol)[0]
    depth = torch.empty((h, w), dtype=torch.float32, device="cuda")
    cost = torch.empty((h, w), dtype=torch.float32, device="cuda")
    L, ptr, st = _lib.lib(), _lib.ptr, _lib.stream_ptr()
    gate = mvs.quantise_cost(mvs.COST_MAX)

    def run_shift():
        _lib.check(L.sfm_mvs_cost_shift(ptr(vol), w, h, D, shift, ptr(q), st), "sfm_mvs_cost_shift")

    def run_aggregate(ndir=8):
        _lib.check(L.sfm_mvs_cost_aggregate(ptr(q), w, h, D, mvs.P1, mvs.P2, ndir, ptr(s), st), "sfm_mvs_cost_aggregate")

    def run_depth():
        _lib.check(L.sfm_mvs_cost_depth(ptr(s), ptr(q), ptr(invd), w, h, D, gate, ptr(depth), ptr(cost), None, st), "sfm_mvs_cost_depth")

    if a.kernels_only:
        run_shift(); run_aggregate(); run_depth()
        torch.cuda.synchronize()
        print(json.dumps(dict(metric="mvs_aggregate_kernels_only", valid_fraction=round(float((depth > 0).float().mean()), 4))))
        return
    import ctypes
    src_ptrs = (ctypes.c_void_p * S)(*[t.data_ptr() for t in srcs])
    mv32 = np.ascontiguousarray(mv, np.float32)
    d0, c0 = torch.empty_like(depth), torch.empty_like(cost)

    def run_sweep(volume):
        _lib.check(L.sfm_mvs_plane_sweep(ptr(grays[i]), src_ptrs, mv32.ctypes.data_as(ctypes.c_void_p), S, w, h, ptr(invd), D, r, k,
                                         float(mvs.VAR_MIN), float(mvs.COST_MAX), ptr(d0), ptr(c0), None, ptr(vol) if volume else None, st),
                   "sfm_mvs_plane_sweep")

    sweep_ms, _ = timed(lambda: run_sweep(False), a.calls, a.warmup)
    sweep_vol_ms, _ = timed(lambda: run_sweep(True), a.calls, a.warmup)
    shift_ms, shift_min = timed(run_shift, a.calls, a.warmup)
    agg4_ms, agg4_min = timed(lambda: run_aggregate(4), a.calls, a.warmup)
    agg8_ms, agg8_min = timed(run_aggregate, a.calls, a.warmup)
    depth_ms, depth_min = timed(run_depth, a.calls, a.warmup)
    n = w * h * D
    fb, ub = 4 * n, 2 * n                                       # bytes of the float volume, of Q or S
    floor = lambda b: round(b / HBM_BYTES_PER_S * 1e3, 4)       # noqa: E731
    bytes_shift, bytes_depth = fb + ub, 2 * ub
    bytes_agg = lambda nd: nd * ub + ub + (nd - 1) * 2 * ub     # noqa: E731
    total = shift_ms + agg8_ms + depth_ms
    res = dict(metric="mvs_aggregate_ms", w=w, h=h, ndepth=D, shift=shift, p1=mvs.P1, p2=mvs.P2, calls=a.calls,
               shift_ms_median=round(shift_ms, 4), shift_ms_min=round(shift_min, 4), shift_floor_ms=floor(bytes_shift),
               aggregate8_ms_median=round(agg8_ms, 4), aggregate8_ms_min=round(agg8_min, 4), aggregate8_floor_ms=floor(bytes_agg(8)),
               aggregate4_ms_median=round(agg4_ms, 4), aggregate4_ms_min=round(agg4_min, 4), aggregate4_floor_ms=floor(bytes_agg(4)),
               depth_ms_median=round(depth_ms, 4), depth_ms_min=round(depth_min, 4), depth_floor_ms=floor(bytes_depth),
               total_ms=round(total, 4), total_floor_ms=floor(bytes_shift + bytes_agg(8) + bytes_depth),
               sweep_ms_median=round(sweep_ms, 4), sweep_with_volume_ms_median=round(sweep_vol_ms, 4),
               total_over_sweep=round(total / sweep_ms, 3),
               parent_valid_fraction=round(float((parent_depth > 0).float().mean()), 4),
               aggregated_valid_fraction=round(float((depth > 0).float().mean()), 4))
    if a.views >= 2:
        posearr = np.hstack([K.ravel()] + [p.ravel() for p in P[:a.views]])
        fr = frames[:a.views]
        del vol, q, s
        for name, flag in (("plain", False), ("aggregate", True)):
            mvs.run_mvs(fr, K, posearr, X, aggregate=flag)
            torch.cuda.synchronize()
            walls, out = [], None
            for _ in range(3):
                t0 = time.perf_counter()
                out = mvs.run_mvs(fr, K, posearr, X, aggregate=flag)
                torch.cuda.synchronize()
                walls.append(time.perf_counter() - t0)
            res[f"run_mvs_{name}_ms_median"] = round(1e3 * float(np.median(walls)), 2)
            res[f"run_mvs_{name}_fused_points"] = int(len(out["points"]))
        res["run_mvs_views"] = a.views
    print(json.dumps(res))


if __name__ == "__main__":
    main()
