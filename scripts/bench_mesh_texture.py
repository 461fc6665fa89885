"""Mesh texturing timings on one GPU -> one JSON line, printed and written to profiles/mesh_texture_bench.json (docs/mesh.md §10).
  python scripts/bench_mesh_texture.py [--views 57] [--calls 10] [--resolution 256] [--texels 8] [--out PATH] [--kernels-only]
- the bench mesh of docs/mesh.md §5: mvs.run_mvs over `--views` gustav_views frames (968 x 648), run_mesh's masks, integration and
  extraction at the defaults (none of it timed here), and its decimate=2 version (mesh.decimate_mesh, the counted rows)
- sfm_mesh_render_depth, sfm_mesh_face_views and sfm_mesh_texture_fill on each of the two meshes, timed by HIP events around the
  entry point's launches alone: median and minimum of `--calls` after 3 warm-ups
- byte floors at 6.3 TB/s.  Rasteriser: per view the faces (12 B) and the vertices (12 B) once, and the map written twice (the
  +inf and the minima, 8 B a pixel).  View choice: per view the same reads plus the map once (4 B a pixel), and 8 B a face written.
  Fill: 3 B a texel written, the faces, the vertices and the faces' views once, and of the frames the pixels the charts of the
  textured faces cover: every frame once at most (3 B a pixel)
- the wall time of mesh.run_mesh with texture off and on, without and with decimate=2 (median of 5 after one warm-up each), and the
  bytes the atlas download adds
--kernels-only: the three entry points alone, `--calls` times per mesh, for a rocprofv3 --kernel-trace --stats run."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=57)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--texels", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_texture_bench.json"))
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    from datagen import gustav_views, sparse_points
    from sfm_mvs_amd import mesh, mvs
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
    stack = torch.stack(frames)
    S, W, C = mesh.tsdf_integrate(torch.stack(out["depths"]), mesh.projection_rows(K, P), origin, voxel, dims, mesh.TRUNC_VOXELS * voxel,
                                  masks=masks, bgr=stack)
    v, c, f = mesh.extract_mesh(S, W, C, origin, voxel, mesh.W_MIN)
    del S, W, C, xyz, masks
    fo, cell, fdims, fext = mesh.decimate_frame(origin, voxel, dims, 2.0)
    dv, dc, df, dn = mesh.decimate_mesh(v, c, f, fo, cell, fdims, fext)
    kv, kf = (int(x) for x in dn[:2].cpu())
    meshes = {"full": (v, c, f), "decimate2": (dv[:kv].contiguous(), dc[:kv].contiguous(), df[:kf].contiguous())}
    Pd = torch.from_numpy(mesh.projection_rows(K, P)).cuda()
    zbuf = torch.empty((n, h, w), dtype=torch.float32, device="cuda")
    res = dict(metric="mesh_texture_ms", views=n, w=w, h=h, dims=list(dims), texels=a.texels, vis_tol=mesh.VIS_TOL)
    for name, (mv, mc, mf) in meshes.items():
        nv, nf = len(mv), len(mf)
        side = mesh._layout(nf, a.texels)[0]
        atlas = torch.empty((side, side, 3), dtype=torch.uint8, device="cuda")
        mesh.render_depth(mv, mf, Pd, w, h, out=zbuf)
        fv, fs = mesh.face_views(mv, mf, Pd, zbuf)
        steps = dict(render=lambda: mesh.render_depth(mv, mf, Pd, w, h, out=zbuf), views=lambda: mesh.face_views(mv, mf, Pd, zbuf),
                     fill=lambda: mesh.texture_fill(mv, mc, mf, Pd, stack, fv, a.texels, out=atlas))
        if a.kernels_only:
            for fn in steps.values():
                for _ in range(a.calls):
                    fn()
            continue
        textured = int((fv >= 0).sum())
        covered = int(torch.isfinite(zbuf).sum())
        screen = float(fs.double().sum()) / 2.0                     # the faces' areas in their views: the score is twice the area
        views_used = int(torch.unique(fv[fv >= 0]).numel())
        floors = dict(render=n * (12 * nf + 12 * nv) + 8 * n * w * h, views=n * (12 * nf + 12 * nv + 4 * w * h) + 8 * nf,
                      fill=3 * side * side + 12 * nf + 12 * nv + 4 * nf + 3 * views_used * w * h)
        row = dict(vertices=nv, faces=nf, atlas_side=side, atlas_bytes=3 * side * side, faces_with_a_view=textured, views_used=views_used,
                   pixels_covered=covered, screen_pixels_of_textured_faces=round(screen, 1),
                   texels_per_pixel=round(textured * (a.texels + 1) * (a.texels + 2) / 2 / max(screen, 1.0), 3))
        for step, fn in steps.items():
            med, lo = timed(fn, a.calls)
            floor_ms = 1e3 * floors[step] / HBM_BYTES_PER_S
            row[step] = dict(ms_median=round(med, 4), ms_min=round(lo, 4), floor_bytes=int(floors[step]), floor_ms=round(floor_ms, 4),
                             over_floor=round(med / floor_ms, 1))
        res[name] = row
    if a.kernels_only:
        torch.cuda.synchronize()
        print(json.dumps(dict(metric="mesh_texture_kernels_only", calls=a.calls, meshes={k: [len(m[0]), len(m[2])] for k, m in meshes.items()})))
        return
    del meshes, zbuf
    for key, kw in (("run_mesh", {}), ("run_mesh_texture", dict(texture=True)), ("run_mesh_decimate2", dict(decimate=2)),
                    ("run_mesh_decimate2_texture", dict(decimate=2, texture=True))):
        kw = dict(kw, **(dict(texture_texels=a.texels) if kw.get("texture") else {}))
        m = mesh.run_mesh(frames, K, posearr, out, resolution=a.resolution, **kw)
        torch.cuda.synchronize()
        walls = []
        for _ in range(5):
            t0 = time.perf_counter()
            m = mesh.run_mesh(frames, K, posearr, out, resolution=a.resolution, **kw)
            torch.cuda.synchronize()
            walls.append(time.perf_counter() - t0)
        res[key] = dict(ms_median=round(1e3 * float(np.median(walls)), 2), ms_min=round(1e3 * float(np.min(walls)), 2), faces=int(len(m["faces"])),
                        atlas_download_bytes=int(m["atlas"].nbytes + m["face_view"].nbytes) if "atlas" in m else 0)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
