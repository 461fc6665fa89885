"""Mesh finishing timings on one GPU -> one JSON line, printed and written to profiles/mesh_finish_bench.json (docs/mesh.md §8).
  python scripts/bench_mesh_finish.py [--views 57] [--calls 10] [--resolution 256] [--pairs 10] [--out PATH] [--kernels-only]
- the bench mesh of docs/mesh.md §5: mvs.run_mvs over `--views` gustav_views frames (968 x 648), run_mesh's masks, integration and
  extraction at the defaults (none of it timed here: scripts/bench_mvs.py, scripts/bench_mesh.py)
- sfm_mesh_normals and sfm_mesh_smooth at `--pairs` Taubin pairs (default: mesh.SMOOTH_PAIRS), each timed by HIP events around the
  entry point's launches alone: median and minimum of `--calls` after 3 warm-ups
- atomics_upper_bound: 9 and 12 adds per face; a face that is invalid or has no area, and a corner with no usable neighbour,
  issue fewer
- byte floors: faces + vertices + accumulators, each once (see `floors`), / 6.3 TB/s
- the wall time of mesh.run_mesh with the new options off, with normals, and with smoothing and normals (median of 5 after one
  warm-up each, ending in its download)
--kernels-only: the two entry points alone, `--calls` times each, for a rocprofv3 --kernel-trace --stats run."""
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

from bench_mesh_clean import HBM_BYTES_PER_S, timed  # noqa: E402


def floors(nv, nf, steps):
    """Bytes that must move, each array once per pass over it: normals read the faces (12 B) and the vertices (12 B), write and read
    the accumulators (32 B a row: zeroed, then read) and write the normals (12 B); a smoothing step reads the faces and the
    vertices, reads the accumulators and zeroes them again, and writes the vertices; the first zeroing once."""
    normals = 12 * nf + 12 * nv + 2 * 32 * nv + 12 * nv
    smooth = 32 * nv + steps * (12 * nf + 12 * nv + 2 * 32 * nv + 12 * nv)
    return normals, smooth


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=57)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--pairs", type=int, default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_finish_bench.json"))
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    from datagen import gustav_views, sparse_points
    from sfm_mvs_amd import _lib, mesh, mvs
    from sfm_mvs_amd.ops import _workspace
    pairs = mesh.SMOOTH_PAIRS if a.pairs is None else a.pairs
    images, K, P = gustav_views(a.views, scale=1, seed=0)
    h, w = images[0].shape[:2]
    n = len(P)
    posearr = np.hstack([K.ravel()] + [p.ravel() for p in P])
    frames = [torch.from_numpy(im).cuda() for im in images]
    out = mvs.run_mvs(frames, K, posearr, sparse_points())
    masks = torch.empty((n, h, w), dtype=torch.uint8, device="cuda")
    xyz = torch.empty((n, h, w, 3), dtype=torch.float32, device="cuda")
    for i in range(n):
        nb = mvs.neighbours(i, n, 4)
        ab, bc = mvs.consistency_matrices(K, P[i], P[nb])
        mvs.consistency(out["depths"][i], [out["depths"][v] for v in nb], nb, ab, i, bc, 0.01, 2, False, mask_out=masks[i], xyz_out=xyz[i])
    origin, voxel, dims = mesh.volume_bounds(out["points"], a.resolution)
    S, W, C = mesh.tsdf_integrate(torch.stack(out["depths"]), mesh.projection_rows(K, P), origin, voxel, dims, mesh.TRUNC_VOXELS * voxel,
                                  masks=masks, bgr=torch.stack(frames))
    v, c, f = mesh.extract_mesh(S, W, C, origin, voxel, mesh.W_MIN)
    del S, W, C, xyz, masks
    nv, nf = len(v), len(f)
    L = _lib.lib()
    nrm, sv = torch.empty_like(v), torch.empty_like(v)
    ws = _workspace(v.device, max(L.sfm_mesh_normals_ws_bytes(nv, nf), L.sfm_mesh_smooth_ws_bytes(nv, nf)))
    factors = np.ascontiguousarray(np.tile(np.array([mesh.SMOOTH_LAMBDA, mesh.SMOOTH_MU], np.float32), pairs))
    org = np.ascontiguousarray(np.asarray(origin, np.float64).astype(np.float32))
    pscale = mesh.smooth_scale(voxel * (max(dims) - 1))

    def normals():
        _lib.check(L.sfm_mesh_normals(_lib.ptr(v), _lib.ptr(f), nv, nf, None, _lib.ptr(nrm), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()),
                   "sfm_mesh_normals")

    def smooth():
        _lib.check(L.sfm_mesh_smooth(_lib.ptr(v), _lib.ptr(f), nv, nf, None, len(factors), factors.ctypes.data, org.ctypes.data, pscale,
                                     _lib.ptr(sv), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "sfm_mesh_smooth")

    if a.kernels_only:
        for _ in range(a.calls):
            normals()
            smooth()
        torch.cuda.synchronize()
        print(json.dumps(dict(metric="mesh_finish_kernels_only", calls=a.calls, vertices=nv, faces=nf, pairs=pairs)))
        return
    n_med, n_min = timed(normals, a.calls)
    s_med, s_min = timed(smooth, a.calls)
    fb_n, fb_s = floors(nv, nf, 2 * pairs)
    res = dict(metric="mesh_finish_ms", views=n, w=w, h=h, dims=list(dims), vertices=nv, faces=nf, pairs=pairs, steps=2 * pairs, pscale=pscale,
               normals_ms_median=round(n_med, 4), normals_ms_min=round(n_min, 4), smooth_ms_median=round(s_med, 4), smooth_ms_min=round(s_min, 4),
               smooth_ms_per_step=round(s_med / max(2 * pairs, 1), 4), normals_floor_bytes=fb_n, smooth_floor_bytes=fb_s,
               normals_floor_ms=round(1e3 * fb_n / HBM_BYTES_PER_S, 5), smooth_floor_ms=round(1e3 * fb_s / HBM_BYTES_PER_S, 5),
               normals_over_floor=round(n_med / (1e3 * fb_n / HBM_BYTES_PER_S), 1), smooth_over_floor=round(s_med / (1e3 * fb_s / HBM_BYTES_PER_S), 1),
               atomics_upper_bound=dict(normals=9 * nf, smooth_per_step=12 * nf), launches=dict(normals=3, smooth=1 + 4 * pairs))
    for key, kw in (("run_mesh_ms_median", {}), ("run_mesh_normals_ms_median", dict(normals=True)),
                    ("run_mesh_smooth_normals_ms_median", dict(normals=True, smooth=pairs)),
                    ("run_mesh_clean_smooth_normals_ms_median", dict(clean=True, normals=True, smooth=pairs))):
        mesh.run_mesh(frames, K, posearr, out, resolution=a.resolution, **kw)
        torch.cuda.synchronize()
        walls = []
        for _ in range(5):
            t0 = time.perf_counter()
            mesh.run_mesh(frames, K, posearr, out, resolution=a.resolution, **kw)
            torch.cuda.synchronize()
            walls.append(time.perf_counter() - t0)
        res[key] = round(1e3 * float(np.median(walls)), 2)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
