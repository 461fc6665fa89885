"""Mesh decimation timings on one GPU -> one JSON line, printed and written to profiles/mesh_decimate_bench.json (docs/mesh.md §9).
  python scripts/bench_mesh_decimate.py [--views 57] [--calls 10] [--resolution 256] [--cells 2 4] [--out PATH] [--kernels-only]
- the bench mesh of docs/mesh.md §5: mvs.run_mvs over `--views` gustav_views frames (968 x 648), run_mesh's masks, integration and
  extraction at the defaults (none of it timed here: scripts/bench_mvs.py, scripts/bench_mesh.py)
- sfm_mesh_decimate over run_mesh's frame at each of `--cells` voxels per cell, with colours and dedupe, timed by HIP events around
  the entry point's launches alone: median and minimum of `--calls` after 3 warm-ups; the counts it leaves
- byte floor: every array once per pass over it (see `floor_bytes`), / 6.3 TB/s; the atomics issued (upper bound)
- the wall time of mesh.run_mesh without and with decimate (median of 5 after one warm-up each, ending in its download), and the
  words each downloads and converts on the host
--kernels-only: the entry point alone, `--calls` times per cell size, for a rocprofv3 --kernel-trace --stats run."""
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

EXTRACT_MS = 0.83               # sfm_mesh_extract on this mesh (docs/mesh.md §5)


def floor_bytes(nv, nf, cells, slots, nv_out, nf_out):
    """Bytes that must move, each array once per pass over it: init writes the table (4 B a cell), the accumulator rows (64 B) and
    the face set (4 B a slot); key reads the vertices (12 B) and writes the keys (4 B); sum reads vertices, colours and keys and
    the rows come back once (64 B); count and map read the keys, map writes the new ids; vertex reads the keys and writes the new
    rows (24 B each); insert, resolve and face read the faces (12 B) three times, resolve writes and face reads a flag byte, face
    writes the new faces."""
    init = 4 * cells + 64 * nv + 4 * slots
    vertex = (12 + 4) * nv + (24 + 4 + 64) * nv + 4 * nv + (4 + 4) * nv + 4 * nv + 24 * nv_out
    face = 3 * 12 * nf + 2 * nf + 12 * nf_out
    return init + vertex + face


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=57)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--cells", type=float, nargs="+", default=[2.0, 4.0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_decimate_bench.json"))
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
    L = _lib.lib()
    ov, oc, of = torch.empty_like(v), torch.empty_like(c), torch.empty_like(f)
    on = torch.empty(4, dtype=torch.int32, device="cuda")
    slots = 2
    while slots < 2 * nf:
        slots *= 2

    def entry(cells):
        fo, cell, fdims, fext = mesh.decimate_frame(origin, voxel, dims, cells)
        org = np.ascontiguousarray(fo.astype(np.float32))
        d = np.ascontiguousarray(fdims, np.int32)
        ws = _workspace(v.device, L.sfm_mesh_decimate_ws_bytes(nv, nf, d.ctypes.data))
        pscale = mesh.smooth_scale(fext)

        def run():
            _lib.check(L.sfm_mesh_decimate(_lib.ptr(v), _lib.ptr(c), _lib.ptr(f), nv, nf, None, org.ctypes.data, float(cell), d.ctypes.data, pscale, 1,
                                           _lib.ptr(ov), _lib.ptr(oc), _lib.ptr(of), _lib.ptr(on), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()),
                       "sfm_mesh_decimate")
        return run, fdims, pscale, ws.numel()

    if a.kernels_only:
        for cells in a.cells:
            run = entry(cells)[0]
            for _ in range(a.calls):
                run()
        torch.cuda.synchronize()
        print(json.dumps(dict(metric="mesh_decimate_kernels_only", calls=a.calls, cells=a.cells, vertices=nv, faces=nf)))
        return
    res = dict(metric="mesh_decimate_ms", views=n, w=w, h=h, dims=list(dims), vertices=nv, faces=nf, set_slots=slots, launches=12,
               extract_ms=EXTRACT_MS)
    for cells in a.cells:
        run, fdims, pscale, ws_bytes = entry(cells)
        med, lo = timed(run, a.calls)
        counts = [int(x) for x in on.cpu()]
        ncell = int(np.prod(fdims, dtype=np.int64))
        fb = floor_bytes(nv, nf, ncell, slots, counts[0], counts[1])
        floor_ms = 1e3 * fb / HBM_BYTES_PER_S
        res[f"cells{cells:g}"] = dict(frame_dims=list(fdims), frame_cells=ncell, pscale=pscale, workspace_bytes=int(ws_bytes), ms_median=round(med, 4),
                                      ms_min=round(lo, 4), vertices_out=counts[0], faces_out=counts[1], unusable=counts[2], duplicates_dropped=counts[3],
                                      floor_bytes=fb, floor_ms=round(floor_ms, 5), over_floor=round(med / floor_ms, 1),
                                      over_extract=round(med / EXTRACT_MS, 2), atomics_upper_bound=dict(min=nv, add=7 * nv, cas_or_min=2 * nf))
    for key, kw in (("run_mesh", {}), ("run_mesh_decimate2", dict(decimate=2)), ("run_mesh_decimate4", dict(decimate=4)),
                    ("run_mesh_clean_smooth_normals", dict(clean=True, normals=True, smooth=mesh.SMOOTH_PAIRS)),
                    ("run_mesh_clean_smooth_normals_decimate2", dict(clean=True, normals=True, smooth=mesh.SMOOTH_PAIRS, decimate=2))):
        m = mesh.run_mesh(frames, K, posearr, out, resolution=a.resolution, **kw)
        torch.cuda.synchronize()
        walls = []
        for _ in range(5):
            t0 = time.perf_counter()
            m = mesh.run_mesh(frames, K, posearr, out, resolution=a.resolution, **kw)
            torch.cuda.synchronize()
            walls.append(time.perf_counter() - t0)
        # words downloaded: the packed buffers of mesh.py, all of the capacities' size; words converted: the counted rows
        extra = (6 if kw.get("clean") else 0)
        if kw.get("decimate"):
            down = extra + 4 + 6 * nv + 3 * nf + (3 * nv if kw.get("normals") else 0)
        else:
            down = extra + 6 * nv + 3 * nf + (3 * nv if kw.get("smooth") else 0) + (3 * nv if kw.get("normals") else 0)
        res[key] = dict(ms_median=round(1e3 * float(np.median(walls)), 2), vertices=int(len(m["vertices"])), faces=int(len(m["faces"])),
                        download_bytes=4 * down, rows_converted_bytes=int(sum(np.asarray(m[k]).nbytes for k in ("vertices", "colors", "faces", "normals") if k in m)))
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
