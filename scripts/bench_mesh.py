"""TSDF fusion + marching-tetrahedra timings on one GPU -> one JSON line (docs/mesh.md).
  python scripts/bench_mesh.py [--views 57] [--calls 10] [--resolutions 256,512] [--kernels-only]
- mvs.run_mvs over `--views` gustav_views frames (968 x 648, pose.csv's cameras, the reference's sparse cloud): the depth maps and
  fused cloud the mesh step starts from (not timed here: scripts/bench_mvs.py)
- per resolution: the volume of mesh.volume_bounds, the consistency masks run_mesh builds, then
  sfm_tsdf_integrate over all views and sfm_mesh_extract, each timed by HIP events around the entry point's launches alone
  (median of `--calls`, the sums re-zeroed before each integration); vertex and face counts; the wall time of mesh.run_mesh
  (median of 3 after one warm-up, ending in its download)
- voxel-view samples nx*ny*nz*views and their rate against the aims (integration <= 5 ms, extraction <= 2 ms at 256)
--kernels-only: integration and extraction at the first resolution, for a rocprofv3 --kernel-trace --stats run."""
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


def timed(fn, calls):
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
    ap.add_argument("--views", type=int, default=57)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--resolutions", default="256,512")
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    from datagen import gustav_views, sparse_points
    from sfm_mvs_amd import _lib, mesh, mvs
    from sfm_mvs_amd.ops import _workspace
    images, K, P = gustav_views(a.views, scale=1, seed=0)
    h, w = images[0].shape[:2]
    n = len(P)
    posearr = np.hstack([K.ravel()] + [p.ravel() for p in P])
    frames = [torch.from_numpy(im).cuda() for im in images]
    out = mvs.run_mvs(frames, K, posearr, sparse_points())
    depths = torch.stack(out["depths"])
    bgr = torch.stack(frames)
    masks = torch.empty((n, h, w), dtype=torch.uint8, device="cuda")
    xyz = torch.empty((n, h, w, 3), dtype=torch.float32, device="cuda")
    for i in range(n):
        nb = mvs.neighbours(i, n, 4)
        ab, bc = mvs.consistency_matrices(K, P[i], P[nb])
        mvs.consistency(out["depths"][i], [out["depths"][v] for v in nb], nb, ab, i, bc, 0.01, 2, False, mask_out=masks[i], xyz_out=xyz[i])
    Pd = torch.from_numpy(mesh.projection_rows(K, P)).cuda()
    L = _lib.lib()
    res = dict(metric="mesh_ms", views=n, w=w, h=h, fused_points=int(len(out["points"])), mask_fraction=round(float(masks.float().mean()), 4), trunc_voxels=mesh.TRUNC_VOXELS,
               w_min=mesh.W_MIN, aims_ms_at_256=dict(integrate=5.0, extract=2.0))
    resolutions = [int(r) for r in a.resolutions.split(",")][:1 if a.kernels_only else None]
    for r in resolutions:
        origin, voxel, dims = mesh.volume_bounds(out["points"], r)
        nx, ny, nz = dims
        trunc = mesh.TRUNC_VOXELS * voxel
        S = torch.zeros((nz, ny, nx), dtype=torch.float32, device="cuda")
        W = torch.zeros_like(S)
        C = torch.zeros((nz, ny, nx, 4), dtype=torch.float32, device="cuda")
        org = np.asarray(origin, np.float32)

        def integrate():
            _lib.check(L.sfm_tsdf_integrate(_lib.ptr(depths), _lib.ptr(masks), _lib.ptr(bgr), _lib.ptr(Pd), n, w, h, org.ctypes.data,
                                            float(voxel), nx, ny, nz, float(trunc), _lib.ptr(S), _lib.ptr(W), _lib.ptr(C), _lib.stream_ptr()),
                       "sfm_tsdf_integrate")

        def fresh_integrate():
            S.zero_()
            W.zero_()
            C.zero_()
            torch.cuda.synchronize()
            return timed(integrate, 1)

        fresh_integrate()                                            # warm-up
        ti = [fresh_integrate() for _ in range(a.calls)]
        int_med, int_min = float(np.median([t[0] for t in ti])), float(min(t[1] for t in ti))
        v, c, f = mesh.extract_mesh(S, W, C, origin, voxel, mesh.W_MIN)
        nv, nf = len(v), len(f)
        ws = _workspace(S.device, L.sfm_mesh_extract_ws_bytes(nx, ny, nz))

        def extract():
            _lib.check(L.sfm_mesh_extract(_lib.ptr(S), _lib.ptr(W), _lib.ptr(C), org.ctypes.data, float(voxel), nx, ny, nz, float(mesh.W_MIN),
                                          nv, nf, _lib.ptr(v), _lib.ptr(c), _lib.ptr(f), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()),
                       "sfm_mesh_extract")

        ext_med, ext_min = timed(extract, a.calls)
        samples = nx * ny * nz * n
        known = float((W >= mesh.W_MIN).float().mean())
        entry = dict(dims=list(dims), voxel=voxel, integrate_ms_median=round(int_med, 4), integrate_ms_min=round(int_min, 4),
                     extract_ms_median=round(ext_med, 4), extract_ms_min=round(ext_min, 4), vertices=nv, faces=nf, known_fraction=round(known, 4),
                     voxel_view_samples=samples, samples_per_s=round(samples / (int_med * 1e-3), 1))
        del S, W, C, v, c, f, ws
        if not a.kernels_only:
            mesh.run_mesh(frames, K, posearr, out, resolution=r)
            torch.cuda.synchronize()
            walls = []
            for _ in range(3):
                t0 = time.perf_counter()
                m = mesh.run_mesh(frames, K, posearr, out, resolution=r)
                torch.cuda.synchronize()
                walls.append(time.perf_counter() - t0)
            entry.update(run_mesh_ms_median=round(1e3 * float(np.median(walls)), 2), run_mesh_faces=int(len(m["faces"])))
        res["res%d" % r] = entry
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
