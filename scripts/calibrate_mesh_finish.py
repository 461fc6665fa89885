"""The calibration table of the mesh finishing step (docs/mesh.md §8), on the CPU model alone: the mesh of
scripts/calibrate_mesh_clean.model_mesh (tests/np_mvs.py depth maps of tests/mvs_scenes.render_scene, run_mesh's masks,
tests/np_mesh.py at grid 96), tests/np_mesh_clean.py at run_mesh's default share, then tests/np_mesh_finish.py: Taubin smoothing at
0, 2, 5, 10, 20 pairs and the vertex normals of the result.

Ground-truth normals come from the ground-truth depth maps: every pixel and its four neighbours are back-projected; the forward
cross product (right x down) and the backward one (left x up) must agree within AGREE_DEG, which drops depth edges and creases;
their normalised sum, turned toward the camera, is the pixel's normal.  A vertex is scored when it is on the surface
(test_mesh_cpu.on_surface_fraction's rule) and its nearest pixel in the view where it fits best has such a normal.  Per seed and
pair count: the median and 90th-percentile angle between the vertex normal and the ground truth, the share above 30 degrees, and
the on-surface share of all vertices.  No GPU is needed.
  python scripts/calibrate_mesh_finish.py [--seeds 0 1 2] [--resolution 96] [--pairs 0 2 5 10 20]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]

AGREE_DEG = 5.0
PAIRS = (0, 2, 5, 10, 20)


def gt_normal_maps(K, P, gt):
    """Per view (normals [h, w, 3] in world axes, valid [h, w])."""
    out = []
    Kinv = np.linalg.inv(K)
    for k in range(len(P)):
        d = np.asarray(gt[k], np.float64)
        h, w = d.shape
        ys, xs = np.mgrid[0:h, 0:w]
        X = (Kinv @ np.stack([xs.ravel(), ys.ravel(), np.ones(h * w)])).T.reshape(h, w, 3) * d[..., None]
        c = X[1:-1, 1:-1]
        fwd = np.cross(X[1:-1, 2:] - c, X[2:, 1:-1] - c)
        bwd = np.cross(c - X[1:-1, :-2], c - X[:-2, 1:-1])
        known = (d[1:-1, 1:-1] > 0) & (d[1:-1, 2:] > 0) & (d[2:, 1:-1] > 0) & (d[1:-1, :-2] > 0) & (d[:-2, 1:-1] > 0)
        with np.errstate(all="ignore"):
            fu = fwd / np.linalg.norm(fwd, axis=-1, keepdims=True)
            bu = bwd / np.linalg.norm(bwd, axis=-1, keepdims=True)
            agree = known & (np.einsum("ijk,ijk->ij", fu, bu) >= np.cos(np.radians(AGREE_DEG)))
            n = fu + bu
            n /= np.linalg.norm(n, axis=-1, keepdims=True)
        n = np.where((np.einsum("ijk,ijk->ij", n, c) > 0)[..., None], -n, n)             # toward the camera (at the origin)
        R = np.linalg.solve(K, P[k])[:, :3]
        full = np.zeros((h, w, 3))
        valid = np.zeros((h, w), bool)
        full[1:-1, 1:-1] = np.where(agree[..., None], n @ R, 0.0)                        # R^T n per pixel
        valid[1:-1, 1:-1] = agree
        out.append((full, valid))
    return out


def vertex_truth(verts, K, P, gt, voxel, maps):
    """(on_surface bool [m], scored bool [m], truth [m, 3]): the ground-truth normal at the nearest pixel of the view whose depth
    the vertex fits best, for on-surface vertices."""
    v = np.asarray(verts, np.float64)
    h, w = gt[0].shape
    Xh = np.hstack([v, np.ones((len(v), 1))]).T
    best = np.full(len(v), np.inf)
    truth = np.zeros((len(v), 3))
    has = np.zeros(len(v), bool)
    zmax = np.full(len(v), -np.inf)
    for k in range(len(P)):
        q = P[k] @ Xh
        zmax = np.maximum(zmax, (np.linalg.solve(K, P[k])[2] @ Xh))
        with np.errstate(divide="ignore", invalid="ignore"):
            u = np.floor(q[0] / q[2] + 0.5)
            t = np.floor(q[1] / q[2] + 0.5)
        ok = (q[2] > 0) & (u >= 0) & (u <= w - 1) & (t >= 0) & (t <= h - 1)
        ui, ti = np.where(ok, u, 0).astype(int), np.where(ok, t, 0).astype(int)
        g = np.where(ok, gt[k][ti, ui], 0.0)
        e = np.where(ok & (g > 0), np.abs(q[2] - g) / np.where(g > 0, g, 1.0), np.inf)
        better = e < best
        best = np.where(better, e, best)
        truth[better] = maps[k][0][ti[better], ui[better]]
        has[better] = maps[k][1][ti[better], ui[better]]
    with np.errstate(invalid="ignore"):
        on = best <= 0.5 * voxel / zmax
    return on, on & has, truth


def angles(normals, truth):
    n = np.asarray(normals, np.float64)
    return np.degrees(np.arccos(np.clip(np.einsum("ij,ij->i", n, truth), -1.0, 1.0)))     # a zero normal scores 90 degrees


def cleaned_model(seed, resolution=96, model=None):
    """The model mesh after the clean-up at run_mesh's default share: (vertices, faces, K, P, gt, origin, voxel, extent).
    model: calibrate_mesh_clean.model_mesh(seed, resolution), when the caller has it."""
    import np_mesh_clean
    from calibrate_mesh_clean import model_mesh, share_threshold
    from mvs_scenes import scene_cloud
    from sfm_mvs_amd import mesh
    v, c, f, K, P, gt, voxel = model_mesh(seed, resolution) if model is None else model
    origin, voxel2, dims = mesh.volume_bounds(scene_cloud(K, P, gt), resolution)
    assert voxel2 == voxel
    kv, _, kf, _ = np_mesh_clean.clean(v, c, f, share_threshold(len(f)))
    return kv, kf, K, P, gt, origin.astype(np.float32), voxel, voxel * (max(dims) - 1)


def table(seed, resolution=96, pairs=PAIRS, model=None):
    """{pairs: (median angle, 90th percentile, share above 30 degrees, on-surface share, vertices scored)}."""
    import np_mesh_finish as nf
    from sfm_mvs_amd import mesh
    v, f, K, P, gt, origin, voxel, extent = cleaned_model(seed, resolution, model)
    maps = gt_normal_maps(K, P, gt)
    rows = {}
    for n in pairs:
        p = nf.smooth(v, f, nf.taubin_factors(n, mesh.SMOOTH_LAMBDA, mesh.SMOOTH_MU), origin, nf.pscale_of(extent))
        nrm = nf.normals(p, f)
        on, scored, truth = vertex_truth(p, K, P, gt, voxel, maps)
        a = angles(nrm[scored], truth[scored])
        rows[n] = (float(np.median(a)), float(np.percentile(a, 90)), float((a > 30.0).mean()), float(on.mean()), int(scored.sum()))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, nargs="+", default=[0, 1, 2])
    ap.add_argument("--resolution", type=int, default=96)
    ap.add_argument("--pairs", type=int, nargs="+", default=list(PAIRS))
    a = ap.parse_args()
    print("| seed | pairs | median angle | 90th percentile | above 30 degrees | on surface | vertices scored |")
    print("|---|---|---|---|---|---|---|")
    for s in a.seeds:
        for n, (med, p90, tail, on, m) in table(s, a.resolution, a.pairs).items():
            print(f"| {s} | {n} | {med:.2f} | {p90:.2f} | {100.0 * tail:.2f} % | {on:.4f} | {m} |", flush=True)


if __name__ == "__main__":
    main()
