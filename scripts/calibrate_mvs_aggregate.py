"""The calibration sweep of the cost-volume aggregation's defaults (docs/mvs.md §7), on the CPU model alone: the middle view of
tests/mvs_scenes.render_scene (5 views, 160 x 120, 128 planes, r = 3, top 2 of 4, VAR_MIN, COST_MAX), seeds 0..2, swept with
tests/np_mvs.py and aggregated with tests/np_mvs_aggregate.py over shift x (P1, P2) x ndir.  Prints one Markdown table row per
setting: per seed "valid share / within 1 %" over the r-interior, and the share of wrong depths relative to the parent's
winner-take-all map.  No GPU is needed.
  python scripts/calibrate_mvs_aggregate.py [--seeds 0 1 2]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

PAIRS = [(0, 0), (5, 51), (10, 102), (20, 205), (10, 51), (20, 102), (41, 410)]


def model_volume(seed, ndepth=128, radius=3):
    """(parent depth, volume, invd, truth) of the middle view, as run_mvs would sweep it."""
    import np_mvs
    from mvs_scenes import gray, render_scene, scene_cloud
    from sfm_mvs_amd import mvs
    imgs, K, P, gt = render_scene(n=5, w=160, h=120, seed=seed)
    X = scene_cloud(K, P, gt)
    nb = mvs.neighbours(2, 5, 4)
    invd = mvs._inverse_depths_host(*mvs.depth_range(X, P[2], P_all=P), ndepth)
    depth, _, _, vol = np_mvs.plane_sweep(gray(imgs[2]), [gray(imgs[v]) for v in nb], mvs.sweep_matrices(K, P[2], P[nb]), invd, radius, 2,
                                          mvs.VAR_MIN, mvs.COST_MAX)
    return depth, vol, invd, gt[2]


def accuracy(depth, truth, r):
    d, g = depth[r:-r, r:-r], truth[r:-r, r:-r]
    valid = d > 0
    return float(valid.mean()), float((np.abs(d[valid] - g[valid]) <= 0.01 * g[valid]).mean())


def main():
    import np_mvs_aggregate as agg
    from sfm_mvs_amd import mvs
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, nargs="+", default=[0, 1, 2])
    args = ap.parse_args()
    models = [model_volume(s) for s in args.seeds]
    parents = [accuracy(m[0], m[3], 3) for m in models]
    print("| shift | P1 | P2 | ndir | " + " | ".join(f"seed {s}" for s in args.seeds) + " | wrong / parent's |")
    print("|---|---|---|---|" + "---|" * (len(args.seeds) + 1))
    print("| parent (winner-take-all) | | | | " + " | ".join(f"{v:.3f} / {w:.3f}" for v, w in parents) + " | 1 |")
    gate = agg.gate_of(mvs.COST_MAX)
    for shift in (0, 1, 2, 3):
        qs = [agg.cost_shift(m[1], shift) for m in models]
        for p1, p2 in PAIRS:
            for ndir in (4, 8):
                cells, ratios = [], []
                for m, q, (pv, pw) in zip(models, qs, parents):
                    d = agg.cost_depth(agg.cost_aggregate(q, p1, p2, ndir), q, m[2], gate)[0]
                    v, w = accuracy(d, m[3], 3)
                    cells.append(f"{v:.3f} / {w:.3f}")
                    ratios.append(f"{(1 - w) / (1 - pw):.2f}")
                print(f"| {shift} | {p1} | {p2} | {ndir} | " + " | ".join(cells) + " | " + ", ".join(ratios) + " |", flush=True)


if __name__ == "__main__":
    main()
