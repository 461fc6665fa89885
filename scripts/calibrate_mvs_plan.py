"""Calibration of the MVS-PLAN defaults and test bars on the CPU (docs/mvs.md §8.4), with tests/np_mvs_plan.py and tests/np_mvs.py alone:
the permuted arc scene (planned sources and ranges against sequence neighbours and mvs.depth_range), the candidate windows, and the
ring scene's matrices.  No GPU.

  python scripts/calibrate_mvs_plan.py [arc ...]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import mvs_plan_cases as mc
import np_mvs_plan as npl


def scene_report(arc, perm_seed=mc.PERM_SEED, nsrc=mc.NSRC, views=None, ndepth=64, window=(1.0, 30.0), min_good=8):
    from sfm_mvs_amd import mvs
    from test_mvs_cpu import depth_accuracy
    imgs, K, P, gt, perm = mc.permuted_scene(perm_seed, arc=arc)
    X, cam_idx, pt_idx = mc.synth_tracks(K, P, gt)
    n = len(P)
    plan = npl.plan_views(cam_idx, pt_idx, X, P, nsrc, window[0], window[1], min_good)
    print(f"arc {arc} perm {perm.tolist()} tracks {len(X)} obs {len(cam_idx)} window {window} min_good {min_good}")
    print(" planned neighbours (as rendered views):", [[int(perm[v]) for v in row] for row in plan["neighbours"]], "of views", perm.tolist())
    rows = []
    for i in (range(n) if views is None else views):
        t0 = time.time()
        seq = mvs.neighbours(i, n, nsrc)
        old = mvs.depth_range(X, P[i], P_all=P)
        new = tuple(plan["ranges"][i])
        dp = mc.np_depth_map(imgs, K, P, i, plan["neighbours"][i], new, ndepth)
        ds = mc.np_depth_map(imgs, K, P, i, seq, old, ndepth)
        vp, wp = depth_accuracy(dp, gt[i], 3)
        vs, ws = depth_accuracy(ds, gt[i], 3)
        rows.append((i, int(perm[i]), vp, wp, vs, ws, mc.wrong_share(dp, gt[i]), mc.wrong_share(ds, gt[i]), new, old, mc.coverage(new, gt[i]),
                     mc.coverage(old, gt[i]), int(plan["m"][i])))
        print(f"  view {i} (rendered {perm[i]}): planned valid {vp:.4f} within {wp:.4f} wrong {rows[-1][6]:.4f} | sequence {seq} valid {vs:.4f} within {ws:.4f} "
              f"wrong {rows[-1][7]:.4f} | range planned ({new[0]:.3f}, {new[1]:.3f}) covers {rows[-1][10]:.4f}, depth_range ({old[0]:.3f}, {old[1]:.3f}) "
              f"covers {rows[-1][11]:.4f}, m {rows[-1][12]}  [{time.time() - t0:.0f} s]", flush=True)
    return rows


def ring_report(window=(1.0, 60.0), min_good=8):
    P, X, cam_idx, pt_idx = mc.ring_tracks()
    plan = npl.plan_views(cam_idx, pt_idx, X, P, 4, window[0], window[1], min_good)
    C = npl.centres(P)
    ang = np.degrees(np.arccos(np.clip([[(C[a] @ C[b]) / (np.linalg.norm(C[a]) * np.linalg.norm(C[b])) for b in range(8)] for a in range(8)], -1, 1)))
    print("ring scene: angle between camera centres seen from the origin, row 0:", np.round(ang[0], 1).tolist())
    print(" shared row 0:", plan["shared"][0].tolist())
    print(f" good (window {window}) row 0:", plan["good"][0].tolist())
    print(" neighbours:", plan["neighbours"])
    print(" ranges:", np.round(plan["ranges"], 3).tolist())


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "ring":
        for win in ((1.0, 30.0), (1.0, 60.0), (1.0, 100.0)):
            ring_report(win)
    elif len(sys.argv) > 1 and sys.argv[1] == "windows":
        imgs, K, P, gt, perm = mc.permuted_scene()
        X, cam_idx, pt_idx = mc.synth_tracks(K, P, gt)
        inv = np.argsort(perm)
        for win in ((0.0, 180.0), (1.0, 30.0), (2.0, 20.0), (5.0, 60.0)):
            for mg in (1, 8, 64):
                plan = npl.plan_views(cam_idx, pt_idx, X, P, mc.NSRC, win[0], win[1], mg)
                # a view's ideal sources are the nearest views on the arc: the distance of the chosen ones in rendered order
                dist = [[abs(int(perm[v]) - int(perm[i])) for v in row] for i, row in enumerate(plan["neighbours"])]
                print(f"window {win} min_good {mg}: arc distances of the chosen sources {dist}")
    else:
        for arc in [float(a) for a in sys.argv[1:]] or [mc.SCENE["arc"]]:
            scene_report(arc)
