"""Mesh clean-up timings on one GPU -> one JSON line (docs/mesh.md §7).
  python scripts/bench_mesh_clean.py [--views 57] [--calls 10] [--resolution 256] [--kernels-only]
- the bench mesh of docs/mesh.md §5: mvs.run_mvs over `--views` gustav_views frames (968 x 648), run_mesh's masks, integration and
  extraction at the defaults (none of it timed here: scripts/bench_mvs.py, scripts/bench_mesh.py)
- sfm_mesh_components (from label[v] = v, the default rounds) and sfm_mesh_clean (the threshold of run_mesh's default share), each
  timed by HIP events around the entry point's launches alone: median and minimum of `--calls` after 3 warm-ups; the rounds the
  status reports; components, components kept, vertices and faces dropped
- byte floors: the bytes each entry point cannot avoid moving (see `floors`) / 6.3 TB/s
- the wall time of mesh.run_mesh with and without clean (median of 5 after one warm-up each, ending in its download)
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

HBM_BYTES_PER_S = 6.3e12


def timed(fn, calls, warm=3):
    for _ in range(warm):
        fn()
    times = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times)), float(np.min(times))


def floors(nv, nf, kv, kf, changing_rounds):
    """Bytes that must move: labelling reads the faces and reads + writes the labels once per round that runs (changing rounds + the
    one that finds nothing); cleaning reads the faces three times (count, flags, gather) and the labels three times, writes and
    reads faces_of and the new ids, reads the rows of the kept vertices (position + colour) and writes them and the kept faces."""
    rounds = changing_rounds + 1
    components = rounds * (12 * nf + 8 * nv) + 4 * nv
    clean = 3 * 12 * nf + 3 * 4 * nv + 4 * 4 * nv + 2 * 24 * kv + 12 * kf
    return components, clean


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=57)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--resolution", type=int, default=256)
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
    min_faces = max(1, int(np.floor(mesh.MIN_COMPONENT_SHARE * nf)))
    L = _lib.lib()
    labels = torch.empty(nv, dtype=torch.int32, device="cuda")
    status = torch.empty(2, dtype=torch.int32, device="cuda")
    counts = torch.empty(4, dtype=torch.int32, device="cuda")
    ov, oc, of = torch.empty_like(v), torch.empty_like(c), torch.empty_like(f)
    ws = _workspace(v.device, max(L.sfm_mesh_components_ws_bytes(nv, nf), L.sfm_mesh_clean_ws_bytes(nv, nf)))

    def components():
        _lib.check(L.sfm_mesh_components(_lib.ptr(f), nv, nf, mesh.COMPONENT_ROUNDS, 0, _lib.ptr(labels), _lib.ptr(status), _lib.ptr(ws),
                                         ws.numel(), _lib.stream_ptr()), "sfm_mesh_components")

    def clean():
        _lib.check(L.sfm_mesh_clean(_lib.ptr(v), _lib.ptr(c), _lib.ptr(f), nv, nf, _lib.ptr(labels), min_faces, 0, _lib.ptr(ov), _lib.ptr(oc),
                                    _lib.ptr(of), _lib.ptr(counts), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "sfm_mesh_clean")

    if a.kernels_only:
        for _ in range(a.calls):
            components()
            clean()
        torch.cuda.synchronize()
        print(json.dumps(dict(metric="mesh_clean_kernels_only", calls=a.calls, vertices=nv, faces=nf, status=status.tolist(), counts=counts.tolist())))
        return
    comp_med, comp_min = timed(components, a.calls)
    converged, changing = status.tolist()
    clean_med, clean_min = timed(clean, a.calls)
    kv, kf, ncomp, nkept = counts.tolist()
    fb_comp, fb_clean = floors(nv, nf, kv, kf, changing)
    res = dict(metric="mesh_clean_ms", views=n, w=w, h=h, dims=list(dims), vertices=nv, faces=nf, rounds_enqueued=mesh.COMPONENT_ROUNDS,
               rounds_that_changed=changing, converged=converged, min_faces=min_faces, components=ncomp, components_kept=nkept,
               vertices_dropped=nv - kv, faces_dropped=nf - kf,
               components_ms_median=round(comp_med, 4), components_ms_min=round(comp_min, 4), clean_ms_median=round(clean_med, 4),
               clean_ms_min=round(clean_min, 4), components_floor_bytes=fb_comp, clean_floor_bytes=fb_clean,
               components_floor_ms=round(1e3 * fb_comp / HBM_BYTES_PER_S, 5), clean_floor_ms=round(1e3 * fb_clean / HBM_BYTES_PER_S, 5),
               launches=dict(components=mesh.COMPONENT_ROUNDS + 2, clean=7))
    for key, kw in (("run_mesh_ms_median", {}), ("run_mesh_clean_ms_median", dict(clean=True))):
        mesh.run_mesh(frames, K, posearr, out, resolution=a.resolution, **kw)
        torch.cuda.synchronize()
        walls = []
        for _ in range(5):
            t0 = time.perf_counter()
            m = mesh.run_mesh(frames, K, posearr, out, resolution=a.resolution, **kw)
            torch.cuda.synchronize()
            walls.append(time.perf_counter() - t0)
        res[key] = round(1e3 * float(np.median(walls)), 2)
        res[key.replace("_ms_median", "_faces")] = int(len(m["faces"]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
