"""Calibration of the mesh decimation step on the CPU model (docs/mesh.md §9): the model meshes of §7 (np_mvs depth maps, run_mesh's
masks, np_mesh at grid 96, cleaned at run_mesh's default share), optionally smoothed by the recommended Taubin pairs, then the
restatement tests/np_mesh_decimate.py at each cell size over run_mesh's frame, and the restatement's normals of the result.

  python scripts/calibrate_mesh_decimate.py [--seeds 0 1 2] [--resolution 96] [--cells 1.5 2 3 4]

Per row: faces out / faces in, live faces dropped as duplicates, §4's on-surface share of the vertices and §8's median angle between
the vertex normals and the ground-truth normals; `cells` 0 is the mesh before the step.  No GPU is needed.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]

CELLS = (1.5, 2.0, 3.0, 4.0)
PAIRS = (0, 10)


def table(seed, resolution=96, cells=CELLS, pairs=PAIRS, model=None):
    """{(pairs, cells): (faces out / faces in, duplicates dropped, on-surface share, median angle, vertices out, faces out)};
    cells 0.0: the mesh before the step."""
    import np_mesh_decimate as nd
    import np_mesh_finish as nf
    from calibrate_mesh_finish import angles, cleaned_model, gt_normal_maps, vertex_truth
    from mvs_scenes import scene_cloud
    from sfm_mvs_amd import mesh
    v, f, K, P, gt, origin, voxel, extent = cleaned_model(seed, resolution, model)
    org64, _, dims = mesh.volume_bounds(scene_cloud(K, P, gt), resolution)
    maps = gt_normal_maps(K, P, gt)

    def score(p, faces):
        on, scored, truth = vertex_truth(p, K, P, gt, voxel, maps)
        a = angles(nf.normals(p, faces)[scored], truth[scored])
        return float(on.mean()), float(np.median(a))

    rows = {}
    for n in pairs:
        p = nf.smooth(v, f, nf.taubin_factors(n, mesh.SMOOTH_LAMBDA, mesh.SMOOTH_MU), origin, nf.pscale_of(extent))
        rows[(n, 0.0)] = (1.0, 0) + score(p, f) + (len(p), len(f))
        for d in cells:
            fo, cell, fdims, fext = nd.frame_of(org64, voxel, dims, d)
            dv, _, df, counts = nd.decimate(p, None, f, fo, cell, fdims, nf.pscale_of(fext), True)
            assert counts[2] == 0, counts
            rows[(n, float(d))] = (len(df) / len(f), int(counts[3])) + score(dv, df) + (len(dv), len(df))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, nargs="+", default=[0, 1, 2])
    ap.add_argument("--resolution", type=int, default=96)
    ap.add_argument("--cells", type=float, nargs="+", default=list(CELLS))
    a = ap.parse_args()
    print("| seed | pairs | cells | vertices | faces | faces out / in | duplicates dropped | on surface | median angle |")
    print("|---|---|---|---|---|---|---|---|---|")
    for s in a.seeds:
        for (n, d), (ratio, dups, on, med, nv, nf_) in table(s, a.resolution, a.cells).items():
            print(f"| {s} | {n} | {d:g} | {nv} | {nf_} | {ratio:.4f} | {dups} | {on:.4f} | {med:.2f} |", flush=True)


if __name__ == "__main__":
    main()
