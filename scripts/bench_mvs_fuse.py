"""Times the merging fusion (docs/mvs.md §10) on the bench input of scripts/bench_mvs.py — 57 gustav_views frames of 968 x 648, the
reference's sparse cloud for the depth ranges — and prints one JSON line (also written to --out, default profiles/mvs_fuse_bench.json):

  python scripts/bench_mvs_fuse.py [--out PATH] [--views 57] [--reps 7] [--once]
  python scripts/bench_mvs_fuse.py --run-mvs {off,on} [--tree DIR]

  launches   the depth maps and normals of run_mvs(refine=True) are kept; over those maps, by HIP events around entry points
             whose arguments were marshalled beforehand (median of --reps): the one sfm_mvs_fuse launch with normals and colours, with
             colours only, and bare; beside the filter's loop of one sfm_mvs_consistency launch per view over the same maps
  floors     the bytes every variant must move (each input word read once, each output word written once; the gathered neighbour
             samples are re-reads of the same maps and count nothing) over the HBM rate: 8 TB/s peak and the 6.3 TB/s a streaming
             kernel achieves (MI355X), and the ratio of the measured time to the latter
--once runs the consistency loop and then the fuse launch with normals and colours, once each, and times nothing: the input of a kernel
  trace (rocprofv3 --kernel-trace --stats -- python scripts/bench_mvs_fuse.py --once), in which the one fuse_kernel launch stands beside
  the consistency_kernel launches over the same maps (2 x 57 of them: run_mvs's own loop, then this one;
  profiles/mvs_fuse_kernel_stats.csv).
--run-mvs times mvs.run_mvs on the same frames by the wall clock (each call ends in its own download; median and min of 5 after a
  warm-up) with fuse off or on and prints one line; --tree DIR imports the package from another checkout (the parent commit's, built
  there), so that a shell loop can alternate the three variants process by process (profiles/mvs_fuse_ab.txt)."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK, HBM_STREAM = 8.0e12, 6.3e12      # bytes/s: the MI355X's specified peak, and what a streaming kernel achieves


def bench_input(views):
    import torch
    from datagen import gustav_views, sparse_points
    images, K, P = gustav_views(max(views, 5), scale=1, seed=0)
    images, P = images[:views], P[:views]
    X = sparse_points()
    posearr = np.hstack([K.ravel()] + [p.ravel() for p in P])
    return [torch.from_numpy(im).cuda() for im in images], K, P, X, posearr


def run_mvs_wall(args):
    import torch
    from sfm_mvs_amd import _lib, mvs
    frames, K, P, X, posearr = bench_input(args.views)
    kw = dict(fuse=True) if args.run_mvs == "on" else {}
    mvs.run_mvs(frames, K, posearr, X, **kw)
    torch.cuda.synchronize()
    walls, out = [], None
    for _ in range(5):
        t0 = time.perf_counter()
        out = mvs.run_mvs(frames, K, posearr, X, **kw)
        torch.cuda.synchronize()
        walls.append(1e3 * (time.perf_counter() - t0))
    print(json.dumps(dict(tool="bench_mvs_fuse", run_mvs=kw, tree="this commit" if args.tree == ROOT else os.path.basename(args.tree), views=args.views,
                          wall_ms_median=round(float(np.median(walls)), 2), wall_ms_min=round(float(np.min(walls)), 2),
                          wall_ms=[round(v, 2) for v in walls], points=int(len(out["points"])), library=os.path.basename(_lib.LIB_PATH))))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mvs_fuse_bench.json"))
    ap.add_argument("--views", type=int, default=57)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--run-mvs", choices=["off", "on"])
    ap.add_argument("--tree", default=ROOT)
    args = ap.parse_args()
    args.tree = os.path.abspath(args.tree)
    for p in (args.tree, os.path.join(args.tree, "tests")):
        sys.path.insert(0, p)
    import torch
    assert torch.cuda.is_available(), "bench_mvs_fuse needs a GPU"
    if args.run_mvs:
        return run_mvs_wall(args)
    from sfm_mvs_amd import _lib, mvs
    frames, K, P, X, posearr = bench_input(args.views)
    n = len(frames)
    h, w = frames[0].shape[:2]
    out = mvs.run_mvs(frames, K, posearr, X, refine=True)
    dstack = out["depths"][0].new_empty((n, h, w))
    nstack = out["normal_maps"][0].new_empty((n, h, w, 3))
    for i in range(n):
        dstack[i].copy_(out["depths"][i])
        nstack[i].copy_(out["normal_maps"][i])
    fstack = torch.stack(frames)
    del out
    nbrs = [mvs.neighbours(i, n, 4) for i in range(n)]
    table = mvs.fuse_table(K, P, nbrs, 2)
    table_dev = torch.from_numpy(table.view(np.uint8).reshape(n, 512)).cuda()
    L, ptr, stream = _lib.lib(), _lib.ptr, _lib.stream_ptr()
    mask = torch.empty((n, h, w), dtype=torch.uint8, device="cuda")
    support = torch.empty_like(mask)
    xyz = torch.empty((n, h, w, 3), dtype=torch.float32, device="cuda")
    nout, cout = torch.empty_like(xyz), torch.empty_like(fstack)
    cos_min = mvs._cos_min(mvs.FUSE_MAX_ANGLE)

    def fuse_call(normals, colours):
        return lambda: _lib.check(L.sfm_mvs_fuse(ptr(dstack), ptr(nstack) if normals else None, ptr(fstack) if colours else None, ptr(table_dev), n,
                                                 w, h, 0.01, cos_min, 1, ptr(mask), ptr(xyz), ptr(nout) if normals else None,
                                                 ptr(cout) if colours else None, ptr(support), stream), "sfm_mvs_fuse")

    loop_args, keep = [], []
    for i in range(n):                                          # the filter's loop as run_mvs(fuse=None) enqueues it, marshalled beforehand
        ab, bc = mvs.consistency_matrices(K, P[i], P[nbrs[i]])
        ab, bc = np.ascontiguousarray(ab, np.float32), np.ascontiguousarray(bc, np.float32)
        idx = np.ascontiguousarray(nbrs[i], np.int32)
        dptrs = (ctypes.c_void_p * len(nbrs[i]))(*[dstack[v].data_ptr() for v in nbrs[i]])
        keep.append((ab, bc, idx, dptrs))
        loop_args.append((ptr(dstack[i]), dptrs, idx.ctypes.data_as(ctypes.c_void_p), ab.ctypes.data_as(ctypes.c_void_p), len(nbrs[i]), i,
                          bc.ctypes.data_as(ctypes.c_void_p), w, h, 0.01, min(2, len(nbrs[i])), 1, ptr(mask[i]), ptr(xyz[i]), stream))

    def loop():
        for a in loop_args:
            _lib.check(L.sfm_mvs_consistency(*a), "sfm_mvs_consistency")

    variants = dict(fuse_normals_colours=fuse_call(True, True), fuse_colours=fuse_call(False, True), fuse_bare=fuse_call(False, False),
                    consistency_loop=loop)
    loop()
    torch.cuda.synchronize()
    filter_points = int(mask.sum())
    variants["fuse_normals_colours"]()
    torch.cuda.synchronize()
    if args.once:
        print(json.dumps(dict(tool="bench_mvs_fuse", once=True, width=w, height=h, views=n)))
        return 0
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()

    def timed(fn):
        ms = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return float(np.median(ms)), float(np.min(ms))

    ms = {k: timed(fn) for k, fn in variants.items()}
    variants["fuse_normals_colours"]()
    torch.cuda.synchronize()
    px = n * h * w
    per_pixel = dict(fuse_normals_colours=(4 + 12 + 3) + (1 + 12 + 12 + 3 + 1), fuse_colours=(4 + 3) + (1 + 12 + 3 + 1), fuse_bare=4 + (1 + 12 + 1),
                     consistency_loop=4 + (1 + 12))
    floors = {k: dict(bytes=px * b, ms_at_8TBps=1e3 * px * b / HBM_PEAK, ms_at_6p3TBps=1e3 * px * b / HBM_STREAM,
                      measured_over_floor_at_6p3TBps=ms[k][0] / (1e3 * px * b / HBM_STREAM)) for k, b in per_pixel.items()}
    res = dict(tool="bench_mvs_fuse", width=w, height=h, views=n, neighbours=4, reps=args.reps, max_angle=mvs.FUSE_MAX_ANGLE,
               ms_median_min={k: [round(v[0], 4), round(v[1], 4)] for k, v in ms.items()}, floors=floors,
               fuse_over_loop=round(ms["fuse_normals_colours"][0] / ms["consistency_loop"][0], 3),
               points=dict(filter=filter_points, fused_at_max_angle=int(mask.sum())),
               support_histogram=[int(c) for c in torch.bincount(support.reshape(-1).long(), minlength=10)[1:10]],
               library=os.path.basename(_lib.LIB_PATH), build_id_mvs_fuse=_lib.code_hashes_of_binary().get("mvs_fuse.hip"))
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
