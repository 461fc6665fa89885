"""TSDF fusion and marching tetrahedra on the device (sfm_tsdf_integrate, sfm_mesh_count, sfm_mesh_extract, mesh.run_mesh,
run_sfm_images(densify=True, mesh=True)): bit-identical to the float32 restatement tests/np_mesh.py, and a surface on the rendered
scene's ground truth."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import np_mesh  # noqa: E402
from mvs_scenes import render_scene, scene_cloud  # noqa: E402


def bits(t):
    a = t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return a.view(np.int32) if a.dtype == np.float32 else a


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def scene_inputs(nview, seed=3, resolution=37):
    """Depth maps of a rendered scene with noise and holes, random masks, the frames, P and an odd-sized grid."""
    from sfm_mvs_amd import mesh
    imgs, K, P, gt = render_scene(n=nview, w=157, h=93, seed=seed, arc=0.6)
    rng = np.random.default_rng(seed)
    depth = np.stack(gt).astype(np.float32)
    depth *= (1.0 + 0.003 * rng.standard_normal(depth.shape)).astype(np.float32)
    depth[rng.random(depth.shape) < 0.05] = 0.0
    masks = (rng.random(depth.shape) < 0.8).astype(np.uint8) * rng.integers(1, 255, depth.shape).astype(np.uint8)
    bgr = np.stack(imgs)
    bgr[..., 1] = 255 - bgr[..., 1]                               # the channels differ: their order is visible
    origin, voxel, dims = mesh.volume_bounds(scene_cloud(K, P, gt), resolution)
    return depth, masks, bgr, mesh.projection_rows(K, P), origin, voxel, dims, (K, P, gt)


@pytest.mark.gpu
@pytest.mark.parametrize("nview", [1, 5, 9])
@pytest.mark.parametrize("use_mask,use_color", [(False, False), (True, False), (False, True), (True, True)])
def test_integrate_is_bit_identical_to_the_restatement(hip, nview, use_mask, use_color):
    from sfm_mvs_amd import mesh
    depth, masks, bgr, P, origin, voxel, dims, _ = scene_inputs(nview)
    assert dims[0] % 64 and dims[1] % 4 and np.prod(dims) % 256, dims   # not a multiple of any tile or block
    trunc = 3.0 * voxel
    S, W, C = mesh.tsdf_integrate(up(depth), P, origin, voxel, dims, trunc, masks=up(masks) if use_mask else None,
                                  bgr=up(bgr) if use_color else None)
    wS, wW, wC = np_mesh.tsdf_integrate(depth, P, origin, voxel, dims, trunc, mask=masks if use_mask else None,
                                        bgr=bgr if use_color else None)
    assert same(S, wS) and same(W, wW)
    assert (C is None) == (not use_color)
    if use_color:
        assert same(C, wC)
    assert (wW > 0).mean() > 0.05 and (wS < 0).any() and (wS > 0).any()


@pytest.mark.gpu
def test_two_chunked_calls_equal_one_call(hip):
    from sfm_mvs_amd import mesh
    depth, masks, bgr, P, origin, voxel, dims, _ = scene_inputs(9)
    trunc = 2.5 * voxel
    one = mesh.tsdf_integrate(up(depth), P, origin, voxel, dims, trunc, masks=up(masks), bgr=up(bgr))
    S, W, C = mesh.tsdf_integrate(up(depth[:4]), P[:4], origin, voxel, dims, trunc, masks=up(masks[:4]), bgr=up(bgr[:4]))
    S2, W2, C2 = mesh.tsdf_integrate(up(depth[4:]), up(P[4:]), origin, voxel, dims, trunc, masks=up(masks[4:]), bgr=up(bgr[4:]), S=S, W=W, C=C)
    assert S2.data_ptr() == S.data_ptr() and C2.data_ptr() == C.data_ptr()
    for a, b in zip(one, (S2, W2, C2)):
        assert same(a, b)


def sphere_field(dims, centre, radius):
    nx, ny, nz = dims
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return (np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - radius).astype(np.float32)


def fields():
    rng = np.random.default_rng(7)
    dims = (23, 19, 17)
    out = []
    S = rng.standard_normal(dims[::-1]).astype(np.float32)
    W = rng.integers(0, 4, dims[::-1]).astype(np.float32)
    C = np.concatenate([rng.uniform(0, 2000, dims[::-1] + (3,)), rng.integers(0, 3, dims[::-1] + (1,))], -1).astype(np.float32)
    out.append(("random", S * W, W, C, (0.5, -1.25, 2.0), 0.37))
    S = sphere_field(dims, (10.3, 9.1, 8.2), 6.4)
    out.append(("sphere", 2.0 * S, np.full_like(S, 2.0), None, (0.0, 0.0, 0.0), 1.0))      # F = S/W = the distance
    depth, masks, bgr, P, origin, voxel, sdims, _ = scene_inputs(9, seed=4, resolution=45)
    fS, fW, fC = np_mesh.tsdf_integrate(depth, P, origin, voxel, sdims, 3.0 * voxel, mask=masks, bgr=bgr)
    out.append(("scene", fS, fW, fC, origin, voxel))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("w_min", [1.0, 2.0, 3.5])
def test_extraction_is_bit_identical_to_the_restatement(hip, w_min):
    from sfm_mvs_amd import mesh
    for name, S, W, C, origin, voxel in fields():
        cnt = mesh.mesh_counts(up(S), up(W), w_min).cpu().numpy()
        v, c, f = mesh.extract_mesh(up(S), up(W), None if C is None else up(C), origin, voxel, w_min)
        wv, wc, wf = np_mesh.extract_mesh(S, W, C, np.asarray(origin, np.float64).astype(np.float32), np.float32(voxel), w_min)
        assert tuple(cnt) == (len(wv), len(wf)), name
        assert same(v, wv) and same(f, wf), name
        assert (c is None) == (C is None)
        if C is not None:
            assert same(c, wc), name
        if name != "random" and w_min < 3.0:
            assert len(wf) > 100, (name, len(wf))


@pytest.mark.gpu
def test_repeated_runs_are_identical(hip):
    from sfm_mvs_amd import mesh
    depth, masks, bgr, P, origin, voxel, dims, _ = scene_inputs(5, seed=6, resolution=51)
    runs = []
    for _ in range(2):
        S, W, C = mesh.tsdf_integrate(up(depth), P, origin, voxel, dims, 3.0 * voxel, masks=up(masks), bgr=up(bgr))
        runs.append([S, W, C] + list(mesh.extract_mesh(S, W, C, origin, voxel, 1.0)))
    for a, b in zip(*runs):
        assert same(a, b)
    assert len(runs[0][-1]) > 100


def mvs_of_scene(seed, **kw):
    from sfm_mvs_amd import mvs
    imgs, K, P, gt = render_scene(n=5, w=160, h=120, seed=seed)
    posearr = np.hstack([K.ravel()] + [p.ravel() for p in P])
    return imgs, K, P, gt, posearr, mvs.run_mvs(imgs, K, posearr, scene_cloud(K, P, gt), **kw)


@pytest.mark.gpu
def test_run_mesh_on_a_rendered_scene(hip):
    """run_mvs then run_mesh at the calibrated defaults: the vertices lie on the rendered surfaces (the CPU test's bar, half a
    voxel along the ray), the faces form an oriented 2-manifold with boundary, and the result equals np_mesh over the same depth
    maps and masks."""
    from test_mesh_cpu import MIN_ON_SURFACE, RUN_MESH_RESOLUTION, check_manifold, on_surface_fraction
    from sfm_mvs_amd import mesh, mvs
    imgs, K, P, gt, posearr, out = mvs_of_scene(0)
    m = mesh.run_mesh(imgs, K, posearr, out, resolution=RUN_MESH_RESOLUTION)
    v, c, f = m["vertices"], m["colors"], m["faces"]
    assert v.dtype == np.float64 and c.dtype == np.float64 and f.dtype == np.int32 and v.shape == c.shape and f.shape[1] == 3
    assert len(f) > 1000 and np.all(np.isfinite(v)) and c.min() >= 0 and c.max() <= 255
    origin, voxel, dims = mesh.volume_bounds(out["points"], RUN_MESH_RESOLUTION)
    frac = on_surface_fraction(v[np.unique(f)], K, P, gt, voxel)
    assert frac >= MIN_ON_SURFACE, frac
    check_manifold(f, len(v), closed=False)
    # the same from the restatement
    n = len(P)
    depths = [d.cpu().numpy() for d in out["depths"]]
    masks = []
    for i in range(n):
        nb = mvs.neighbours(i, n, 4)
        ab, bc = mvs.consistency_matrices(K, P[i], P[nb])
        masks.append(mvs.consistency(out["depths"][i], [out["depths"][j] for j in nb], nb, ab, i, bc, 0.01, 2, False)[0].cpu().numpy())
    S, W, C = np_mesh.tsdf_integrate(np.stack(depths), mesh.projection_rows(K, P), origin, voxel, dims,
                                     np.float32(mesh.TRUNC_VOXELS * voxel), mask=np.stack(masks), bgr=np.stack(imgs))
    wv, wc, wf = np_mesh.extract_mesh(S, W, C, origin.astype(np.float32), np.float32(voxel), mesh.W_MIN)
    assert np.array_equal(v, wv.astype(np.float64)) and np.array_equal(c, wc.astype(np.float64)) and np.array_equal(f, wf)


@pytest.mark.gpu
@pytest.mark.parametrize("on_device", [True, False])
def test_run_mesh_waits_for_the_host_only_for_the_totals_and_the_download(hip, on_device):
    import warnings
    from sfm_mvs_amd import _lib, mesh
    imgs, K, P, gt, posearr, out = mvs_of_scene(1, ndepth=32)
    frames = [up(im) for im in imgs] if on_device else imgs
    mesh.run_mesh(frames, K, posearr, out, resolution=64)            # warm: the pinned host pool, the workspace
    torch.cuda.synchronize()
    lib0 = int(_lib.lib().sfm_host_sync_count())
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            m = mesh.run_mesh(frames, K, posearr, out, resolution=64)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    syncs = [str(w.message) for w in caught if "synchroniz" in str(w.message).lower()]
    assert len(syncs) == 2, syncs
    assert int(_lib.lib().sfm_host_sync_count()) == lib0
    assert len(m["faces"]) > 0


@pytest.mark.gpu
def test_run_sfm_images_mesh_writes_dense_mesh_ply(hip, tmp_path):
    """8 Gustav frames from pixels: mesh=True adds out["mesh"], equal to run_mesh over the run's halved frames and dense result,
    and to_ply_mesh writes it (a short sequence: every observed point counts, w_min = 1)."""
    from datagen import gustav_views
    from sfm_mvs_amd import mesh
    from sfm_mvs_amd import pipeline as pl
    from sfm_mvs_amd import sift as hsift
    images, K, _ = gustav_views(8, seed=5)
    with pytest.raises(ValueError):
        pl.run_sfm_images(images, K, mesh=True)
    opts = dict(resolution=64, w_min=1.0)
    out = pl.run_sfm_images(images, K, densify=True, mvs_options=dict(ndepth=32), mesh=True, mesh_options=opts)
    assert "dense" in out and "mesh" in out
    m = out["mesh"]
    small = [hsift.pyrdown(torch.from_numpy(im).cuda()) for im in images]
    again = mesh.run_mesh(small, K, out["posearr"], out["dense"], **opts)
    for key in ("vertices", "colors", "faces"):
        assert np.array_equal(m[key], again[key]), key
    masks = sum(int((d > 0).sum()) for d in out["dense"]["depths"])
    assert len(m["faces"]) > 0, (len(m["vertices"]), len(out["dense"]["points"]), masks)
    os.makedirs(tmp_path / "Point_Cloud")
    nv, nf = pl.to_ply_mesh(str(tmp_path), m["vertices"], m["colors"], m["faces"])
    assert (nv, nf) == (len(m["vertices"]), len(m["faces"]))
    text = open(tmp_path / "Point_Cloud" / "dense_mesh.ply").read()
    assert "element vertex %d\n" % nv in text and "element face %d\n" % nf in text
