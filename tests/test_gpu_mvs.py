"""Plane-sweep MVS on the device (sfm_mvs_plane_sweep, sfm_mvs_consistency, mvs.run_mvs, run_sfm_images(densify=True)):
bit-identical to the float32 restatement tests/np_mvs.py, and accurate on a rendered scene with ground truth."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import np_mvs  # noqa: E402
from mvs_scenes import gray, render_scene, scene_cloud, surface_error  # noqa: E402
from parity_cases import np_run_mvs  # noqa: E402


def bits(t):
    a = t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return a.view(np.int32) if a.dtype == np.float32 else a


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def sweep_both(grays, K, P, i, nb, ndepth, radius, topk, var_min, cost_max, widen=1.0):
    from sfm_mvs_amd import mvs
    dmin, dmax = 1.5 / widen, 9.0 * widen
    invd = mvs.inverse_depths(dmin, dmax, ndepth)
    mv = mvs.sweep_matrices(K, P[i], P[nb])
    got = mvs.plane_sweep(up(grays[i]), [up(grays[v]) for v in nb], mv, invd, radius, topk, var_min, cost_max, plane=True, volume=True)
    want = np_mvs.plane_sweep(grays[i], [grays[v] for v in nb], mv, invd.cpu().numpy(), radius, topk, var_min, cost_max)
    return got, want, mv, invd


# (radius, nsrc, topk, ndepth, arc of the camera path: wide arcs warp much of the window out of the sources)
CASES = [(1, 1, 1, 2, 0.3), (2, 2, 2, 33, 0.3), (3, 4, 2, 33, 1.4), (4, 8, 1, 33, 0.6), (3, 4, 1, 128, 0.3), (2, 8, 2, 128, 1.4),
         (4, 2, 2, 2, 1.4), (1, 4, 2, 33, 0.8)]


@pytest.mark.gpu
@pytest.mark.parametrize("radius,nsrc,topk,ndepth,arc", CASES)
def test_plane_sweep_is_bit_identical_to_the_restatement(hip, radius, nsrc, topk, ndepth, arc):
    """157 x 93 (not a multiple of the 16 x 16 tile): depth, cost, plane and the whole cost volume equal np_mvs bit for bit."""
    imgs, K, P, _ = render_scene(n=9, w=157, h=93, seed=3, arc=arc)
    grays = [gray(im) for im in imgs]
    from sfm_mvs_amd import mvs
    nb = mvs.neighbours(4, 9, nsrc)
    (d, c, pl, vol), (wd, wc, wpl, wvol), mv, invd = sweep_both(grays, K, P, 4, nb, ndepth, radius, topk, 150.0, 0.4, widen=1.5)
    assert same(d, wd) and same(c, wc) and same(pl, wpl) and same(vol, wvol)
    assert ndepth == 2 or (wd > 0).mean() > 0.3                     # depths were found ...
    if arc > 1.0:                                                   # ... and the outermost source's warp leaves its frame often
        assert np_mvs.warp(grays[nb[-1]], mv[-1], invd[-1].item(), 157, 93)[1].mean() < 0.9


@pytest.mark.gpu
def test_optional_outputs_and_repeated_calls_change_nothing(hip):
    from sfm_mvs_amd import mvs
    imgs, K, P, _ = render_scene(n=5, w=157, h=93, seed=4, arc=0.5)
    grays = [gray(im) for im in imgs]
    nb = mvs.neighbours(2, 5, 4)
    invd = mvs.inverse_depths(2.0, 8.0, 40)
    mv = mvs.sweep_matrices(K, P[2], P[nb])
    ref, srcs = up(grays[2]), [up(grays[v]) for v in nb]
    full = mvs.plane_sweep(ref, srcs, mv, invd, 3, 2, 150.0, 0.4, plane=True, volume=True)
    for kw in (dict(), dict(plane=True), dict(volume=True), dict(plane=True, volume=True)):
        for _ in range(2):
            d, c, pl, vol = mvs.plane_sweep(ref, srcs, mv, invd, 3, 2, 150.0, 0.4, **kw)
            assert same(d, full[0]) and same(c, full[1])
            assert (pl is None) != kw.get("plane", False) and (vol is None) != kw.get("volume", False)
            if pl is not None:
                assert same(pl, full[2])
            if vol is not None:
                assert same(vol, full[3])


@pytest.mark.gpu
@pytest.mark.parametrize("min_consistent,unique,tau", [(1, True, 0.01), (2, True, 0.01), (2, False, 0.02), (0, False, 0.005)])
def test_consistency_is_bit_identical(hip, min_consistent, unique, tau):
    from sfm_mvs_amd import mvs
    n = 5
    imgs, K, P, _ = render_scene(n=n, w=157, h=93, seed=5, arc=0.5)
    grays = [up(gray(im)) for im in imgs]
    invd = mvs.inverse_depths(2.0, 8.0, 48)
    depths = [mvs.plane_sweep(grays[i], [grays[v] for v in mvs.neighbours(i, n, 4)], mvs.sweep_matrices(K, P[i], P[mvs.neighbours(i, n, 4)]),
                              invd, 2, 2, 150.0, 0.4)[0] for i in range(n)]
    host = [d.cpu().numpy() for d in depths]
    kept = 0
    for i in range(n):
        nb = mvs.neighbours(i, n, 3)
        ab, bc = mvs.consistency_matrices(K, P[i], P[nb])
        mask, xyz = mvs.consistency(depths[i], [depths[v] for v in nb], nb, ab, i, bc, tau, min_consistent, unique)
        wm, wx = np_mvs.consistency(host[i], [host[v] for v in nb], nb, ab, i, bc, tau, min_consistent, unique)
        assert same(mask, wm) and same(xyz, wx)
        kept += int(wm.sum())
    assert kept > 0.05 * n * 157 * 93


@pytest.mark.gpu
def test_full_size_depth_map_is_bit_identical(hip):
    """968 x 648 (the halved Gustav frames), r = 3, 4 sources, top 2, at 6 planes (the NumPy side's time)."""
    from datagen import gustav_views
    from sfm_mvs_amd import mvs
    imgs, K, P = gustav_views(5, scale=1, seed=2)
    assert imgs[0].shape == (648, 968, 3)
    grays = [gray(im) for im in imgs]
    from datagen import sparse_points
    dmin, dmax = mvs.depth_range(sparse_points(), P[2])
    invd = mvs.inverse_depths(dmin, dmax, 6)
    nb = mvs.neighbours(2, 5, 4)
    mv = mvs.sweep_matrices(K, P[2], P[nb])
    d, c, pl, _ = mvs.plane_sweep(up(grays[2]), [up(grays[v]) for v in nb], mv, invd, 3, 2, mvs.VAR_MIN, mvs.COST_MAX, plane=True)
    wd, wc, wpl, _ = np_mvs.plane_sweep(grays[2], [grays[v] for v in nb], mv, invd.cpu().numpy(), 3, 2, mvs.VAR_MIN, mvs.COST_MAX)
    assert same(d, wd) and same(c, wc) and same(pl, wpl)


@pytest.mark.gpu
def test_run_mvs_on_a_rendered_scene_meets_the_cpu_thresholds_and_writes_dense_ply(hip, tmp_path):
    from test_mvs_cpu import MIN_FUSED_WITHIN_1PCT, MIN_VALID_FRACTION, MIN_WITHIN_1PCT, depth_accuracy
    from sfm_mvs_amd import mvs
    from sfm_mvs_amd.pipeline import to_ply
    imgs, K, P, gt = render_scene(n=5, w=160, h=120, seed=0)
    posearr = np.hstack([K.ravel()] + [p.ravel() for p in P])
    X = scene_cloud(K, P, gt)
    out = mvs.run_mvs(imgs, K, posearr, X)
    valid, within = depth_accuracy(out["depths"][2].cpu().numpy(), gt[2], 3)
    assert valid >= MIN_VALID_FRACTION and within >= MIN_WITHIN_1PCT, (valid, within)
    pts, cols = out["points"], out["colors"]
    assert pts.dtype == np.float64 and cols.dtype == np.float64 and pts.shape == cols.shape and pts.shape[1] == 3 and len(pts) > 5000
    # the fused points lie on the rendered surfaces: in some view, within 1 % of the ground-truth depth at their pixel
    assert np.all(np.isfinite(pts))
    on_surface = float((surface_error(pts, K, P, gt) <= 0.01).mean())
    assert on_surface >= MIN_FUSED_WITHIN_1PCT, on_surface
    os.makedirs(tmp_path / "Point_Cloud")
    nv = to_ply(str(tmp_path), pts, cols, densify=True)
    text = open(tmp_path / "Point_Cloud" / "dense.ply").read()
    assert "element vertex %d" % nv in text and nv > 0.5 * len(pts)
    body = text.split("end_header\n", 1)[1].strip().splitlines()
    assert len(body) == nv and len(body[-1].split()) == 6


@pytest.mark.gpu
def test_run_sfm_images_densify_from_pixels(hip):
    """8 Gustav frames from pixels: densify=True leaves the sparse outputs as densify=False computes them and adds a dense cloud
    equal to np_mvs over the same gray frames and posearr."""
    from datagen import gustav_views
    from sfm_mvs_amd import pipeline as pl
    from sfm_mvs_amd import sift as hsift
    images, K, _ = gustav_views(8, seed=5)
    opts = dict(ndepth=6, radius=2, nsrc=2, topk=1)
    base = pl.run_sfm_images(images, K)
    out = pl.run_sfm_images(images, K, densify=True, mvs_options=opts)
    for key in ("posearr", "Xtot", "colorstot", "errors", "first_error"):
        assert np.array_equal(np.asarray(out[key]), np.asarray(base[key])), key
    assert "dense" not in base and set(out) == set(base) | {"dense"}
    small = [hsift.pyrdown(torch.from_numpy(im).cuda()) for im in images]
    grays = [hsift.bgr2gray(s).cpu().numpy() for s in small]
    bgrs = [s.cpu().numpy() for s in small]
    from sfm_mvs_amd import mvs
    d = dict(var_min=mvs.VAR_MIN, cost_max=mvs.COST_MAX, tau=0.01, min_consistent=2, unique=True)
    depths, pts, cols = np_run_mvs(grays, bgrs, K, out["posearr"], out["Xtot"], **opts, **d)
    dense = out["dense"]
    for a, b in zip(dense["depths"], depths):
        assert same(a, b)
    assert len(pts) > 100
    assert np.array_equal(dense["points"], pts) and np.array_equal(dense["colors"], cols)


@pytest.mark.gpu
@pytest.mark.parametrize("on_device", [True, False])
def test_run_mvs_waits_for_the_host_only_for_the_count_and_the_download(hip, on_device):
    """run_mvs's uploads (every view's plane inverse depths; host frames) are stream-ordered: under torch's sync debug mode the
    only synchronising operations of a call are the fused count (mask_indices) and the one download of points and colours, and
    the library itself waits for nothing."""
    import warnings
    from sfm_mvs_amd import _lib, mvs
    imgs, K, P, gt = render_scene(n=5, w=160, h=120, seed=1)
    posearr = np.hstack([K.ravel()] + [p.ravel() for p in P])
    X = scene_cloud(K, P, gt)
    frames = [up(im) for im in imgs] if on_device else imgs
    mvs.run_mvs(frames, K, posearr, X, ndepth=16)                 # warm: the pinned host pool, the workspace of mask_indices
    torch.cuda.synchronize()
    lib0 = int(_lib.lib().sfm_host_sync_count())
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            out = mvs.run_mvs(frames, K, posearr, X, ndepth=16)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    syncs = [str(w.message) for w in caught if "synchroniz" in str(w.message).lower()]
    assert len(syncs) == 2, syncs
    assert int(_lib.lib().sfm_host_sync_count()) == lib0
    assert len(out["points"]) > 0
