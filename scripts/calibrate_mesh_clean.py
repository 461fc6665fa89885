"""The calibration table of the mesh clean-up (docs/mesh.md §7), on the CPU model alone: tests/np_mvs.py depth maps of
tests/mvs_scenes.render_scene (5 views, 160 x 120) at run_mvs's defaults, the unique=False consistency masks run_mesh builds,
tests/np_mesh.py at grid 96 (the volume of the scene's own cloud) and run_mesh's defaults, then tests/np_mesh_clean.py.  Prints one Markdown table row per seed: faces,
components, components under 100 faces and face-less vertices, the on-surface share (test_mesh_cpu.on_surface_fraction) of all
vertices and after dropping the components below run_mesh's share and below 32 and 64 faces, the share of faces kept, and the
on-surface share of the dropped vertices.  No GPU is needed.
  python scripts/calibrate_mesh_clean.py [--seeds 0 1 2] [--resolution 96]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def model_mesh(seed, resolution=96):
    """run_mvs then run_mesh at their defaults, restated: (vertices, colors, faces, K, P, gt, voxel)."""
    import np_mesh
    import np_mvs
    from mvs_scenes import gray, render_scene, scene_cloud
    from sfm_mvs_amd import mesh, mvs
    imgs, K, P, gt = render_scene(n=5, w=160, h=120, seed=seed)
    X, n = scene_cloud(K, P, gt), 5
    nbrs = [mvs.neighbours(i, n, 4) for i in range(n)]
    grays = [gray(im) for im in imgs]
    depths = []
    for i in range(n):
        invd = mvs._inverse_depths_host(*mvs.depth_range(X, P[i], P_all=P), 128)
        depths.append(np_mvs.plane_sweep(grays[i], [grays[v] for v in nbrs[i]], mvs.sweep_matrices(K, P[i], P[nbrs[i]]), invd, 3, 2,
                                         mvs.VAR_MIN, mvs.COST_MAX)[0])
    masks = []
    for i in range(n):
        ab, bc = mvs.consistency_matrices(K, P[i], P[nbrs[i]])
        masks.append(np_mvs.consistency(depths[i], [depths[v] for v in nbrs[i]], nbrs[i], ab, i, bc, 0.01, 2, False)[0])
    origin, voxel, dims = mesh.volume_bounds(X, resolution)   # the volume of the scene's own cloud, as in docs/mesh.md §4
    S, W, C = np_mesh.tsdf_integrate(np.stack(depths), mesh.projection_rows(K, P), origin, voxel, dims, np.float32(mesh.TRUNC_VOXELS * voxel),
                                     mask=np.stack(masks), bgr=np.stack(imgs))
    v, c, f = np_mesh.extract_mesh(S, W, C, origin.astype(np.float32), np.float32(voxel), mesh.W_MIN)
    return v, c, f, K, P, gt, voxel


def share_threshold(nf):
    """run_mesh(clean=True)'s default threshold for a mesh of nf faces."""
    from sfm_mvs_amd import mesh
    return max(1, int(np.floor(mesh.MIN_COMPONENT_SHARE * nf)))


def row(seed, resolution):
    import np_mesh_clean
    from test_mesh_cpu import on_surface_fraction
    v, c, f, K, P, gt, voxel = model_mesh(seed, resolution)
    labels, faces_of = np_mesh_clean.components(f, len(v))
    roots = np.flatnonzero(labels == np.arange(len(v)))
    with_faces = roots[faces_of[roots] > 0]
    small = int((faces_of[with_faces] < 100).sum())
    faceless = int((faces_of[roots] == 0).sum())
    on = on_surface_fraction(v, K, P, gt, voxel)
    cells = []
    t0 = share_threshold(len(f))
    for t in (t0, 32, 64):
        kv, _, kf, counts = np_mesh_clean.clean(v, c, f, t)
        cells.append(f"{on_surface_fraction(kv, K, P, gt, voxel):.4f} ({100.0 * len(kf) / len(f):.2f} % of faces)")
    dropped = faces_of[labels] < t0
    d_on = on_surface_fraction(v[dropped], K, P, gt, voxel) if dropped.any() else float("nan")
    return (f"| {seed} | {len(f)} | {len(with_faces)} | {small} (+{faceless}) | {on:.4f} | {t0}: {cells[0]} | {cells[1]} | {cells[2]} | "
            f"{int(round(d_on * dropped.sum()))} / {int(dropped.sum())} = {d_on:.2f} |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, nargs="+", default=[0, 1, 2])
    ap.add_argument("--resolution", type=int, default=96)
    a = ap.parse_args()
    print("| seed | faces | components with faces | under 100 faces (+ face-less vertices) | on surface, all vertices | dropping below the share "
          "| below 32 | below 64 | on surface among the dropped |")
    print("|---|---|---|---|---|---|---|---|---|")
    for s in a.seeds:
        print(row(s, a.resolution), flush=True)


if __name__ == "__main__":
    main()
