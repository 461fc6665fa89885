"""sfm_tsdf_integrate, sfm_mesh_count and sfm_mesh_extract at the limits of their documented ranges and on degenerate inputs, each
case compared with tests/np_mesh.py bit for bit (parity_cases.same: int32 views; a NaN equals a NaN) AND shown, on the
restatement's output, to exercise what it is named for: a grid of more than 2^20 tiles observed along its whole length, grids
smaller than a tile, no views, sums continued from non-integers, samples exactly at +-trunc, scans with a ragged last segment
checked against a count that goes through no scan, +-0 / NaN / inf field values on crossing edges, grids without a cube, and output
capacities below the counts.  docs/mesh.md, "Limits and fuzzing".

The whole file takes 19 s on the GPU box (35 cases), nearly all of it the NumPy side (the 10.5 M point line twice, five random
fields of up to 786 175 points)."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import parity_cases as pc  # noqa: E402
from mvs_scenes import scene_cloud  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
GRID_LIMIT = 1 << 20              # tsdf_kernel's grid: min(tiles, 2^20) workgroups, each striding over the tiles


def scene_views():
    """Five views of the rendered scene with their ground-truth depth maps, and the 1st..99th percentile box of its cloud."""
    from sfm_mvs_amd import mesh
    _, K, P, gt, imgs = pc.scene(n=5, w=157, h=93, seed=3, arc=0.6)
    cloud = scene_cloud(K, P, gt)
    lo, hi = np.percentile(cloud, 1, axis=0), np.percentile(cloud, 99, axis=0)
    bgr = np.stack(imgs)
    bgr[..., 1] = 255 - bgr[..., 1]
    return np.stack(gt).astype(F), bgr, mesh.projection_rows(K, P), lo, hi


def check_tsdf(*args, **kw):
    want, bad = pc.tsdf_both(*args, **kw)
    assert bad is None, f"{bad} differs from np_mesh"
    return want


@pytest.mark.parametrize("start", ["zero", "continued"])
def test_integrate_strides_over_more_than_2_pow_20_tiles(hip, start):
    """A 2 x 2 x nz line of nz = 2 * 2^20 + 2^19 + 12345 one-slice tiles: the grid-stride loop wraps twice and ends ragged.  The
    line runs along z through the centre of the scene's box, from in front of the surfaces to just behind them, with a truncation
    wide enough that every part of it is observed: a tile the loop skipped differs from one it visited."""
    depth, bgr, P, lo, hi = scene_views()
    nz = 2 * GRID_LIMIT + GRID_LIMIT // 2 + 12345
    ext = hi - lo
    origin = np.array([0.5 * (lo[0] + hi[0]), 0.5 * (lo[1] + hi[1]), lo[2] - 0.1 * ext[2]])
    voxel, trunc, dims = 0.225 * ext[2] / nz, 0.05 * ext[2], (2, 2, nz)
    S0 = W0 = C0 = None
    if start == "continued":
        rng = np.random.default_rng(5)
        S0, W0 = rng.normal(0, 2, dims[::-1]).astype(F), rng.uniform(0, 3, dims[::-1]).astype(F)
        C0 = rng.uniform(0, 700, dims[::-1] + (4,)).astype(F)
    S, W, C = check_tsdf(depth, P, origin, voxel, dims, trunc, bgr=bgr, S=S0, W=W0, C=C0)
    gained = (W != (0 if W0 is None else W0)).reshape(nz, 4)
    for b in range(0, nz, GRID_LIMIT):                               # every block of 2^20 consecutive tiles, the ragged one too
        assert gained[b:b + GRID_LIMIT].mean() >= 0.5, (b, gained[b:b + GRID_LIMIT].mean())
    dS = S if S0 is None else S - S0
    assert (dS[:GRID_LIMIT] > 0).mean() > 0.5 and (dS[2 * GRID_LIMIT:] < 0).mean() > 0.5
    assert (C[..., 3] != (0 if C0 is None else C0[..., 3])).mean() > 0.3


@pytest.mark.parametrize("dims", [(63, 3, 5), (65, 5, 2), (2, 2, 2)])
@pytest.mark.parametrize("use_mask", [False, True])
def test_integrate_grids_smaller_than_a_tile(hip, dims, use_mask):
    """nx < 64 or one past it, ny < 4 or one past it: every 64 x 4 tile is partial."""
    depth, bgr, P, lo, hi = scene_views()
    voxel = float((hi - lo).max()) / (max(dims) - 1) * (0.5 if max(dims) == 2 else 1.0)
    origin = 0.5 * (lo + hi) - 0.5 * voxel * (np.array(dims) - 1)
    rng = np.random.default_rng(sum(dims))
    mask = (rng.random(depth.shape) < 0.8).astype(np.uint8) * rng.integers(1, 255, depth.shape).astype(np.uint8) if use_mask else None
    S, W, C = check_tsdf(depth, P, origin, voxel, dims, max(3.0 * voxel, 0.3 * float((hi - lo).max())), mask=mask, bgr=bgr)
    assert (W > 0).mean() > 0.2 and (C[..., 3] > 0).any()
    if max(dims) > 2:
        assert (S < 0).any() and (S > 0).any()


@pytest.mark.parametrize("color", [False, True])
def test_integrate_without_views_leaves_the_sums_untouched(hip, color):
    dims = (65, 5, 3)
    rng = np.random.default_rng(2)
    S0, W0 = rng.normal(0, 2, dims[::-1]).astype(F), rng.uniform(0, 3, dims[::-1]).astype(F)
    C0 = rng.uniform(0, 700, dims[::-1] + (4,)).astype(F) if color else None
    S, W, C = check_tsdf(np.zeros((0, 9, 11), F), np.zeros((0, 12), F), (0.0, 0.0, 0.0), 0.1, dims, 0.3,
                         bgr=np.zeros((0, 9, 11, 3), np.uint8) if color else None, S=S0, W=W0, C=C0)
    assert pc.same(S, S0) and pc.same(W, W0) and (not color or pc.same(C, C0))


def test_integrate_planted_special_depth_samples(hip):
    """NaN, +-inf, negative and zero depth samples: only a positive sample counts (+inf as a far one: f = 1, no colour)."""
    depth, bgr, P, lo, hi = scene_views()
    rng = np.random.default_rng(9)
    planted = pc.plant_specials(depth, rng, fraction=0.04)
    dims = (37, 23, 29)
    voxel = float((hi - lo).max()) / 36
    S, W, C = check_tsdf(planted, P, lo, voxel, dims, 3.0 * voxel, bgr=bgr)
    clean = pc.np_mesh.tsdf_integrate(depth, P, lo.astype(F), F(voxel), dims, F(3.0 * voxel), bgr=bgr)
    assert (W > 0).mean() > 0.05 and not pc.same(W, clean[1]) and (C[..., 3] < W).any() and np.isfinite(S).all()


def test_integrate_points_behind_a_camera(hip):
    depth, bgr, P, lo, hi = scene_views()
    dims = (37, 29, 41)
    origin, voxel = np.array([lo[0], lo[1], -7.0]), 9.0 / 40           # the cameras stand 4 units in front of the scene's centre
    x, y, z = pc.np_mesh.lattice(origin.astype(F), F(voxel), dims)
    behind = 0
    for m in P:
        p2 = ((m[8] * x + m[9] * y) + m[10] * z) + m[11]
        assert (p2 <= 0).mean() > 0.1 and (p2 > 0).mean() > 0.1
        behind += int((p2 <= 0).sum())
    S, W, C = check_tsdf(depth, P, origin, voxel, dims, 3.0 * voxel, bgr=bgr)
    assert (W > 0).mean() > 0.05 and (W == 0).mean() > 0.1


def test_integrate_samples_exactly_at_plus_and_minus_trunc(hip):
    """P = [I|0], a constant depth map of 4, voxel 1/4, trunc 1/2, z from 3: sdf = 1, 3/4, 1/2, ..., -1 exactly.  sdf == -trunc
    still contributes (only sdf < -trunc does not), sdf == +trunc still carries colour (sdf <= trunc)."""
    voxel, trunc, dims = F(0.25), F(0.5), (4, 4, 9)
    origin = np.array([0.0, 0.0, 3.0], F)
    P = np.array([[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]], F)
    depth = np.full((1, 4, 4), 4.0, F)
    z = origin[2] + np.arange(9).astype(F) * voxel
    sdf = F(4.0) - (((F(0) * F(0) + F(0) * F(0)) + F(1) * z) + F(0))
    assert sdf[2] == trunc and sdf[6] == -trunc and sdf[1] > trunc and sdf[7] < -trunc
    bgr = np.random.default_rng(3).integers(1, 255, (1, 4, 4, 3)).astype(np.uint8)
    S, W, C = check_tsdf(depth, P, origin, voxel, dims, trunc, bgr=bgr)
    assert np.all(W[:7] == 1) and np.all(W[7:] == 0)
    assert np.all(S[2] == 1) and np.all(S[6] == -1) and np.all(S[1] == 1)
    assert np.all(C[:2, ..., 3] == 0) and np.all(C[2:7, ..., 3] == 1) and np.all(C[7:, ..., 3] == 0)


# ---- extraction --------------------------------------------------------------------------------------------------------------
def check_extract(S, W, C, origin, voxel, w_min):
    want, counts, bad = pc.extract_both(S, W, C, origin, voxel, w_min)
    assert bad is None, f"{bad} differs from np_mesh"
    assert counts == pc.counts_by_boolean_arithmetic(S, W, w_min), counts     # the totals against a count that no scan produced
    return want


@pytest.mark.parametrize("blocks", [1023, 1024, 1025, 2 * 1024 + 1, 3 * 1024 - 1])
def test_scan_segments_around_the_scan_width(hip, blocks):
    """mesh_scan_kernel scans ceil(blocks / 1024) block totals per lane: one segment each with a lane idle, exactly full, two with
    most lanes idle at the end, three with one block over, three with the last lane one short.  The point count is not a multiple
    of 256 either (a ragged last block)."""
    dims = pc.dims_with_blocks(blocks)
    n = int(np.prod(dims))
    assert -(-n // 256) == blocks and n % 256 and min(dims) >= 2, dims
    S, W, C = pc.random_field(dims, np.random.default_rng(blocks))
    assert 0.05 < (W == 0).mean() < 0.15
    v, c, f = check_extract(S, W, C, (0.5, -1.25, 2.0), 0.37, 1.0)
    assert len(f) >= 100 and len(v) >= 100


def sphere(dims, centre, radius):
    nx, ny, nz = dims
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return (np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - radius).astype(F)


@pytest.mark.parametrize("value", [0.0, -0.0, np.nan, np.inf, -np.inf])
def test_special_field_values_on_crossing_edges(hip, value):
    """+0 and -0 are outside (F < 0 is false), NaN too, and they interpolate to t = 0 / NaN; +-inf gives t = inf / inf.  Planted
    at every third end of the sphere's crossing edges along +x, alternately the lower and the upper end."""
    dims = (23, 19, 17)
    Fv = sphere(dims, (10.3, 9.1, 8.2), 6.4)
    cross = (Fv[..., :-1] < 0) != (Fv[..., 1:] < 0)
    ks, js, is_ = np.nonzero(cross)
    pick = np.arange(0, len(ks), 3)
    assert len(pick) >= 20
    S = (F(2) * Fv).copy()
    S[ks[pick], js[pick], is_[pick] + (pick // 3) % 2] = F(value)
    W = np.full_like(S, 2.0)
    C = np.concatenate([np.random.default_rng(1).uniform(0, 500, S.shape + (3,)), np.ones(S.shape + (1,))], -1).astype(F)
    v, c, f = check_extract(S, W, C, (0.0, 0.0, 0.0), 1.0, 1.0)
    clean = pc.np_mesh.extract_mesh(F(2) * Fv, W, C, np.zeros(3, F), F(1.0), 1.0)
    assert len(f) >= 100 and not (pc.same(v, clean[0]) and pc.same(f, clean[2]))
    if not np.isfinite(value):
        assert np.isnan(v).any()


def test_unseen_colour_next_to_seen_colour(hip):
    """Wc = 0 at one end of a crossing edge and > 0 at the other: the unseen end's colour is 0, not 0 / 0."""
    dims = (23, 19, 17)
    S, W, C = pc.random_field(dims, np.random.default_rng(7), unknown=0.0)
    cross = (S[..., :-1] < 0) != (S[..., 1:] < 0)
    assert (cross & ((C[..., :-1, 3] == 0) != (C[..., 1:, 3] == 0))).sum() >= 100
    v, c, f = check_extract(S, W, C, (0.5, -1.25, 2.0), 0.37, 1.0)
    assert np.isfinite(c).all() and len(f) >= 100


@pytest.mark.parametrize("dims", [(2, 2, 2), (2, 17, 9), (33, 2, 5), (40, 21, 2), (2, 2, 300)])
def test_grids_with_a_side_of_two(hip, dims):
    """No interior point: every point lies on a face of the grid (every cube touches the boundary in two directions)."""
    S, W, C = pc.random_field(dims, np.random.default_rng(sum(dims)), unknown=0.0 if dims == (2, 2, 2) else 0.1)
    v, c, f = check_extract(S, W, C, (0.5, -1.25, 2.0), 0.37, 1.0)
    assert len(v) > 0 and (len(f) > 0 or dims == (2, 2, 2))


@pytest.mark.parametrize("kind", ["unknown", "inside", "outside", "below w_min"])
def test_fields_without_a_surface_give_empty_outputs(hip, kind):
    dims = (23, 19, 17)
    rng = np.random.default_rng(4)
    S = np.abs(rng.standard_normal(dims[::-1])).astype(F) + F(0.1)
    W = np.full(dims[::-1], 2.0, F)
    if kind == "unknown":
        W[:] = 0
        S = rng.standard_normal(dims[::-1]).astype(F)
    elif kind == "inside":
        S = -S
    elif kind == "below w_min":
        S = rng.standard_normal(dims[::-1]).astype(F)
    v, c, f = check_extract(S, W, None, (0.0, 0.0, 0.0), 1.0, 3.0 if kind == "below w_min" else 1.0)
    assert v.shape == (0, 3) and f.shape == (0, 3)


def test_capacities_below_the_counts_write_nothing_past_them(hip):
    """sfm_mesh_extract with max_vertices / max_faces below the counts, into buffers of the full counted size pre-filled with a
    sentinel: the prefix is the full result's, every element past the capacity still holds the sentinel, the status is SFM_OK;
    with capacity 0 also with NULL outputs."""
    dims = (23, 19, 17)
    S, W, C = pc.random_field(dims, np.random.default_rng(11))
    origin, voxel, w_min = (0.5, -1.25, 2.0), 0.37, 1.0
    wv, wc, wf = pc.np_mesh.extract_mesh(S, W, C, np.asarray(origin, F), F(voxel), w_min)
    nv, nt = len(wv), len(wf)
    assert nv > 1000 and nt > 1000
    rc, *full = pc.extract_with_capacity(S, W, C, origin, voxel, w_min, nv, nt, nv, nt)
    assert rc == 0 and pc.same(full[0].view(F), wv) and pc.same(full[1].view(F), wc) and np.array_equal(full[2], wf)
    for mv in (0, 1, nv // 2, nv - 1):
        for mf in (0, 1, nt // 3, nt - 1):
            for null in ((False, True) if 0 in (mv, mf) else (False,)):
                rc, *part = pc.extract_with_capacity(S, W, C, origin, voxel, w_min, nv, nt, mv, mf, null_outputs=null)
                assert rc == 0, (mv, mf, null)
                if null:                                             # what was not passed cannot have been written
                    full_cmp = [None if mv == 0 else full[0], None if mv == 0 else full[1], None if mf == 0 else full[2]]
                else:
                    full_cmp = full
                bad = pc.capacity_difference(full_cmp, part, nv, nt, mv, mf)
                assert bad is None, (mv, mf, null, bad)


def test_randomised_parity_sweep(hip):
    """A few seconds of scripts/fuzz_mesh.py (tsdf, extract, capacity families; the script exits non-zero on a mismatch)."""
    root = os.path.dirname(HERE)
    r = subprocess.run([sys.executable, os.path.join(root, "scripts", "fuzz_mesh.py"), "8", "7"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert " 0 mismatches" in r.stdout
