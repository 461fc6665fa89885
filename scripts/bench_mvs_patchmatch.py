"""Times the PatchMatch refinement (docs/mvs.md §9) on a rendered 5-view scene and prints one JSON line (also written to --out, default
profiles/mvs_patchmatch_bench.json):

  python scripts/bench_mvs_patchmatch.py [--out PATH] [--once] [--width W --height H]

  launches   by HIP events around whole calls of sfm_mvs_patchmatch on the middle view (median of --reps): iters = 0 is the init and the
             finish launch; the difference to iters = 3, over its six half-sweeps, is one half-sweep; the sweep of the same view beside it
  run_mvs    wall time of run_mvs with and without refine=True, in alternating calls (each ends in its own download: a host clock around
             work that ends in a synchronise)
--once runs every call once and times nothing: the input of a kernel trace (rocprofv3 --kernel-trace --stats -- python ... --once), in which
plane_sweep_kernel and the three pm_* kernels of the same frame stand side by side (profiles/mvs_patchmatch_kernel_stats.csv)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mvs_patchmatch_bench.json"))
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--width", type=int, default=968)
    ap.add_argument("--height", type=int, default=648)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    from mvs_scenes import gray, render_scene, scene_cloud
    from sfm_mvs_amd import _lib, mvs
    assert torch.cuda.is_available(), "bench_mvs_patchmatch needs a GPU"
    w, h, n, view = args.width, args.height, 5, 2
    imgs, K, P, gt = render_scene(n=n, w=w, h=h, seed=0)
    X = scene_cloud(K, P, gt, step=max(7, w // 23))
    posearr = np.hstack([K.ravel()] + [p.ravel() for p in P])
    dev = torch.device("cuda:0")
    grays = [torch.from_numpy(gray(im)).to(dev) for im in imgs]
    nb = mvs.neighbours(view, n, 4)
    mv = mvs.sweep_matrices(K, P[view], P[nb])
    planes = mvs._inverse_depths_host(*mvs.depth_range(X, P[view], P_all=P), 128)
    invd = torch.from_numpy(planes).to(dev)
    srcs = [grays[v] for v in nb]

    def sweep():
        return mvs.plane_sweep(grays[view], srcs, mv, invd)[0]

    def refine(depth, iters):
        return mvs.patchmatch_refine(grays[view], srcs, mv, planes[0], planes[-1], depth, K, P[view], iters=iters)

    depth = sweep()
    refine(depth, mvs.PM_ITERS)
    torch.cuda.synchronize()
    if args.once:
        print(json.dumps(dict(tool="bench_mvs_patchmatch", once=True, width=w, height=h)))
        return 0

    def timed(fn):
        ms = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return float(np.median(ms))

    t_sweep = timed(sweep)
    t0, t1, t3 = (timed(lambda k=k: refine(depth, k)) for k in (0, 1, 3))
    wall = {False: [], True: []}
    mvs.run_mvs(imgs, K, posearr, X, refine=True)                 # warm both paths
    mvs.run_mvs(imgs, K, posearr, X)
    for _ in range(3):
        for opt in (False, True):
            t = time.perf_counter()
            mvs.run_mvs(imgs, K, posearr, X, refine=True if opt else None)
            wall[opt].append(1e3 * (time.perf_counter() - t))
    pixels, d2 = w * h, 49
    out = dict(tool="bench_mvs_patchmatch", width=w, height=h, views=n, sources=len(nb), radius=3, planes=128, reps=args.reps,
               defaults=dict(iters=mvs.PM_ITERS, far=int(mvs.PM_FAR), depth_step=mvs.PM_DEPTH_STEP),
               ms=dict(plane_sweep=t_sweep, init_and_finish=t0, iters_1=t1, iters_3=t3, half_sweep=(t3 - t0) / 6.0),
               bilinear_samples=dict(init=pixels * d2 * len(nb), half_sweep=pixels // 2 * 11 * d2 * len(nb), sweep_warps=pixels * 128 * len(nb)),
               run_mvs_wall_ms=dict(plain=wall[False], refine=wall[True], plain_median=float(np.median(wall[False])),
                                    refine_median=float(np.median(wall[True]))),
               library=os.path.basename(_lib.LIB_PATH), build_id_mvs_patchmatch=_lib.code_hashes_of_binary().get("mvs_patchmatch.hip"))
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
