"""TSDF fusion and marching tetrahedra without a GPU: the C-ABI declares and validates the new entry points, the float32 checker
stands apart from the product, and the algorithm itself (tests/np_mesh.py, the kernels' arithmetic) gives closed, oriented
surfaces of analytic fields and a surface on a rendered scene's ground truth — where the thresholds the GPU end-to-end test
reuses, and the defaults of mesh.run_mesh, are set.  Also volume_bounds and pipeline.to_ply_mesh."""
import ast
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import np_mesh  # noqa: E402

# Share of mesh vertices within half a voxel of a rendered surface along the ray (surface_error <= 0.5 * voxel / camera depth).
# np_mesh over the ground-truth depth maps of render_scene (5 views, 160 x 120, a 128-point grid, run_mesh's defaults):
# 97.7 / 96.6 / 97.2 % (seeds 0..2); over np_mvs depth maps with consistency masks (docs/mesh.md, "Calibration"): 96-98 % at 96.
MIN_ON_SURFACE = 0.95
RUN_MESH_RESOLUTION = 96       # the grid of the GPU end-to-end test (run_mvs on the same 5-view scene)

NEW_SYMBOLS = ("sfm_tsdf_integrate", "sfm_mesh_count_ws_bytes", "sfm_mesh_count", "sfm_mesh_extract_ws_bytes", "sfm_mesh_extract")


def check_manifold(faces, nv, closed):
    """Every directed edge once (consistent orientation); every undirected edge in exactly 2 faces (closed) or at most 2; no
    face repeats a vertex; every index names a vertex.  Returns (V referenced, E, F)."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    assert len(f) and f.min() >= 0 and f.max() < nv
    assert np.all((f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2]))
    directed = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    key = directed[:, 0] * nv + directed[:, 1]
    assert len(np.unique(key)) == len(key), "a directed edge appears twice: inconsistent orientation or a non-manifold edge"
    und = np.sort(directed, 1)
    _, cnt = np.unique(und[:, 0] * nv + und[:, 1], return_counts=True)
    assert cnt.max() <= 2
    if closed:
        assert cnt.min() == 2, "an edge with one face: the surface is not closed"
    return len(np.unique(f)), len(cnt), len(f)


def on_surface_fraction(verts, K, P, gt, voxel):
    """Share of vertices with surface_error <= 0.5 * voxel / z, z the vertex's largest camera depth over the views."""
    from mvs_scenes import surface_error
    v = np.asarray(verts, np.float64)
    Xh = np.hstack([v, np.ones((len(v), 1))])
    z = np.max([Xh @ np.linalg.solve(K, Pk)[2] for Pk in P], axis=0)
    return float((surface_error(v, K, P, gt) <= 0.5 * voxel / z).mean())


def field_of(fn, dims):
    nx, ny, nz = dims
    z, y, x = np.meshgrid(np.arange(nz, dtype=np.float64), np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64),
                          indexing="ij")
    return fn(x, y, z).astype(np.float32)


def test_header_declares_and_library_binds_the_mesh_entry_points():
    from test_abi import declared_symbols
    from sfm_mvs_amd import _lib
    syms = declared_symbols()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s in syms and s in _lib.SIGNATURES and hasattr(handle, s), s
    assert _lib.lib().sfm_abi_version() == 3


def test_argument_errors_are_reported_before_the_device():
    from sfm_mvs_amd import _lib
    L = _lib.lib()
    fake = ctypes.c_void_p(16)                       # never dereferenced: every check below fails first
    org = (ctypes.c_float * 3)(0.0, 0.0, 0.0)

    def integ(nview=2, w=64, h=48, voxel=0.1, nx=8, ny=8, nz=8, trunc=0.3, depth=fake, S=fake, C=None, bgr=None):
        return L.sfm_tsdf_integrate(depth, None, bgr, fake, nview, w, h, org, voxel, nx, ny, nz, trunc, S, fake, C, None)

    for kw, msg in [(dict(nx=1), b"grid"), (dict(nz=0), b"grid"), (dict(nx=1 << 10, ny=1 << 10, nz=129), b"2^27"),
                    (dict(nx=1 << 28, ny=2, nz=2), b"grid"), (dict(trunc=0.0), b"trunc"), (dict(trunc=-1.0), b"trunc"),
                    (dict(voxel=0.0), b"voxel"), (dict(nview=-1), b"nview"), (dict(w=0), b"frame"), (dict(depth=None), b"null"),
                    (dict(S=None), b"null"), (dict(C=fake), b"bgr")]:
        assert integ(**kw) == -1, kw
        assert msg in L.sfm_last_error(), (kw, L.sfm_last_error())
    assert L.sfm_mesh_count_ws_bytes(1 << 10, 1 << 10, 129) == 0 and L.sfm_mesh_extract_ws_bytes(1, 8, 8) == 0
    assert 0 < L.sfm_mesh_count_ws_bytes(64, 64, 64) < L.sfm_mesh_extract_ws_bytes(64, 64, 64)
    assert L.sfm_mesh_extract_ws_bytes(1 << 9, 1 << 9, 1 << 9) >= 5 * (1 << 27)

    def count(nx=8, ny=8, nz=8, w_min=1.0, ws_bytes=1 << 20, counts=fake):
        return L.sfm_mesh_count(fake, fake, nx, ny, nz, w_min, counts, fake, ws_bytes, None)

    for kw, msg in [(dict(ny=1), b"grid"), (dict(nx=512, ny=512, nz=513), b"2^27"), (dict(w_min=0.5), b"w_min"),
                    (dict(w_min=float("inf")), b"w_min"), (dict(counts=None), b"null")]:
        assert count(**kw) == -1, kw
        assert msg in L.sfm_last_error(), (kw, L.sfm_last_error())
    assert count(ws_bytes=16) == -2 and b"workspace" in L.sfm_last_error()

    def extract(nx=8, ny=8, nz=8, w_min=1.0, voxel=0.1, maxv=4, maxf=4, colors=None, C=None, ws_bytes=1 << 20):
        return L.sfm_mesh_extract(fake, fake, C, org, voxel, nx, ny, nz, w_min, maxv, maxf, fake, colors, fake, fake, ws_bytes, None)

    for kw, msg in [(dict(nx=1), b"grid"), (dict(w_min=0.0), b"w_min"), (dict(voxel=-1.0), b"voxel"), (dict(maxv=-1), b"capacity"),
                    (dict(colors=fake), b"CWc")]:
        assert extract(**kw) == -1, kw
        assert msg in L.sfm_last_error(), (kw, L.sfm_last_error())
    assert extract(ws_bytes=16) == -2


def test_the_checker_does_not_import_the_product():
    tree = ast.parse(open(os.path.join(ROOT, "tests", "np_mesh.py")).read())
    for node in ast.walk(tree):
        names = [a.name for a in node.names] if isinstance(node, ast.Import) else [node.module or ""] if isinstance(node, ast.ImportFrom) else []
        assert not any(n.split(".")[0] in ("sfm_mvs_amd", "oracle") for n in names), names


def test_the_six_tetrahedra_tile_the_cube():
    corner, ntri, _ = np_mesh.tet_table()
    vol = 0
    for t in range(6):
        p = np.array([[c & 1, c >> 1 & 1, c >> 2] for c in corner[t]], np.int64)
        vol += abs(round(np.linalg.det((p[1:] - p[0]).astype(float))))
        assert corner[t][0] == 0 and corner[t][3] == 7
    assert vol == 6                                    # six tetrahedra of volume 1/6 each
    assert np.array_equal(ntri[0], [0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0])


@pytest.mark.parametrize("centre,radius", [((11.3, 12.1, 10.7), 6.3), ((12.05, 11.9, 12.2), 5.0), ((10.5, 13.25, 11.9), 8.7)])
def test_sphere_gives_a_closed_oriented_surface_on_the_sphere(centre, radius):
    dims = (25, 27, 24)
    c = np.array(centre)
    S = field_of(lambda x, y, z: np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - radius, dims)
    v, _, f = np_mesh.extract_mesh(S, np.ones_like(S), None, (0.0, 0.0, 0.0), 1.0, 1.0)
    V, E, Fn = check_manifold(f, len(v), closed=True)
    assert V == len(v) and V - E + Fn == 2
    vv = v.astype(np.float64)
    assert np.abs(np.linalg.norm(vv - c, axis=1) - radius).max() <= 0.1
    tri = vv[f]
    normal = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    assert np.all(np.einsum("ij,ij->i", normal, tri.mean(1) - c) > 0)        # outward: from inside to outside


def test_sphere_in_world_units_and_unknown_points():
    """Origin and voxel scale the lattice; points below w_min cut the surface open (no face touches an unknown point)."""
    dims = (21, 21, 21)
    S = field_of(lambda x, y, z: np.sqrt((x - 10.2) ** 2 + (y - 9.7) ** 2 + (z - 10.1) ** 2) - 6.0, dims)
    W = np.full_like(S, 2.0)
    v1, _, f1 = np_mesh.extract_mesh(S * W, W, None, (0.0, 0.0, 0.0), 1.0, 2.0)
    v2, _, f2 = np_mesh.extract_mesh(S * W, W, None, (1.5, -2.0, 0.25), 0.5, 2.0)
    assert np.array_equal(f1, f2) and np.allclose(v2, np.array([1.5, -2.0, 0.25]) + 0.5 * v1.astype(np.float64), atol=1e-5)
    W[:, :, 15:] = 1.0                                   # x >= 15 unknown at w_min 2
    v, _, f = np_mesh.extract_mesh(S * W, W, None, (0.0, 0.0, 0.0), 1.0, 2.0)
    check_manifold(f, len(v), closed=False)
    assert v[np.unique(f)][:, 0].max() <= 14.0 and len(f) < len(f1)


def test_torus_has_euler_characteristic_zero():
    dims = (33, 31, 17)
    R, r = 9.0, 3.6
    S = field_of(lambda x, y, z: np.sqrt((np.sqrt((x - 16.2) ** 2 + (y - 15.1) ** 2) - R) ** 2 + (z - 8.3) ** 2) - r, dims)
    v, _, f = np_mesh.extract_mesh(S, np.ones_like(S), None, (0.0, 0.0, 0.0), 1.0, 1.0)
    V, E, Fn = check_manifold(f, len(v), closed=True)
    assert V == len(v) and V - E + Fn == 0


def test_restated_colours_interpolate_along_the_edge():
    S = np.full((2, 2, 2), 1.0, np.float32)
    S[0, 0, 0] = -3.0                                   # one inside corner: 7 crossing edges from the origin
    W = np.ones_like(S)
    C = np.zeros((2, 2, 2, 4), np.float32)
    C[0, 0, 0] = (10.0, 20.0, 30.0, 1.0)
    C[..., 3][1, 1, 1] = 2.0
    C[1, 1, 1, :3] = (100.0, 100.0, 100.0)
    v, c, f = np_mesh.extract_mesh(S, W, C, (0.0, 0.0, 0.0), 1.0, 1.0)
    assert len(v) == 7 and len(f) == 6
    assert np.allclose(v[0], (0.75, 0.0, 0.0)) and np.allclose(v[6], (0.75, 0.75, 0.75))
    assert np.allclose(c[0], 0.25 * np.array([10.0, 20.0, 30.0])) and np.allclose(c[6], [40.0, 42.5, 45.0])


@pytest.mark.parametrize("seed", [0, 1])
def test_ground_truth_depth_maps_give_a_surface_on_the_scene(seed):
    """np_mesh over render_scene's exact depth maps at run_mesh's truncation and w_min: the vertices lie on the rendered surfaces."""
    from mvs_scenes import render_scene, scene_cloud
    from sfm_mvs_amd import mesh
    imgs, K, P, gt = render_scene(n=5, w=160, h=120, seed=seed)
    origin, voxel, dims = mesh.volume_bounds(scene_cloud(K, P, gt), 128)
    S, W, C = np_mesh.tsdf_integrate(np.stack(gt).astype(np.float32), mesh.projection_rows(K, P), origin, voxel, dims,
                                     mesh.TRUNC_VOXELS * voxel, bgr=np.stack(imgs))
    v, c, f = np_mesh.extract_mesh(S, W, C, origin, voxel, mesh.W_MIN)
    assert len(f) > 20000
    check_manifold(f, len(v), closed=False)
    assert on_surface_fraction(v, K, P, gt, voxel) >= MIN_ON_SURFACE
    assert c.min() >= 0.0 and c.max() <= 255.0


def test_volume_bounds():
    from sfm_mvs_amd import mesh
    rng = np.random.default_rng(0)
    X = rng.uniform([-1.0, 0.0, 2.0], [3.0, 1.0, 4.0], (5000, 3))
    X[:10] = 1e6                                         # far outliers fall outside the 1st / 99th percentiles
    origin, voxel, dims = mesh.volume_bounds(X, resolution=101, pad=0.05)
    lo, hi = np.percentile(X, 1, axis=0), np.percentile(X, 99, axis=0)
    L = (hi - lo).max()
    assert np.allclose(origin, lo - 0.05 * L) and np.isclose(voxel, (1.1 * L) / 100)
    assert dims[0] == 101 and all(2 <= d <= 101 for d in dims)
    assert np.all(origin + (np.array(dims) - 1) * voxel >= hi + 0.05 * L - 1e-9)    # the grid covers the padded box
    assert np.all(origin + (np.array(dims) - 2) * voxel < hi + 0.05 * L)            # ... with no spare lattice plane
    flat = np.column_stack([rng.uniform(0, 1, 100), rng.uniform(0, 1, 100), np.zeros(100)])
    assert mesh.volume_bounds(flat, 64)[2][2] >= 2
    for bad, kw in [(np.zeros((100, 3)), {}), (X[:3], {}), (np.full((50, 3), np.nan), {}), (X, dict(resolution=1)),
                    (X, dict(resolution=2000)), (X, dict(pad=-0.1))]:
        with pytest.raises(mesh.SfmHipError):
            mesh.volume_bounds(bad, **kw)


def test_to_ply_mesh_round_trips(tmp_path):
    from sfm_mvs_amd.pipeline import to_ply_mesh
    rng = np.random.default_rng(1)
    v = rng.normal(0, 1, (50, 3))
    c = rng.uniform(-5, 260, (50, 3))
    c[0] = (0.5, 254.5, 1.49)
    f = rng.integers(0, 50, (80, 3)).astype(np.int32)
    os.makedirs(tmp_path / "Point_Cloud")
    assert to_ply_mesh(str(tmp_path), v, c, f) == (50, 80)
    text = open(tmp_path / "Point_Cloud" / "dense_mesh.ply").read()
    head, body = text.split("end_header\n")
    assert "element vertex 50\n" in head and "element face 80\n" in head and "property list uchar int vertex_indices" in head
    assert head.index("property uchar blue") < head.index("property uchar green") < head.index("property uchar red")
    rows = body.strip().splitlines()
    assert len(rows) == 130
    vt = np.array([r.split() for r in rows[:50]], np.float64)
    assert np.allclose(vt[:, :3], 200 * v, atol=1e-5)
    assert np.array_equal(vt[:, 3:], np.clip(np.floor(c + 0.5), 0, 255)) and tuple(vt[0, 3:]) == (1.0, 255.0, 1.0)
    ft = np.array([r.split() for r in rows[50:]], np.int64)
    assert np.all(ft[:, 0] == 3) and np.array_equal(ft[:, 1:], f)
    with pytest.raises(ValueError):
        to_ply_mesh(str(tmp_path), v, c, f + 1)
