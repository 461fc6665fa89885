"""The mesh decimation step without a GPU (include/sfm_hip.h, "MESH-DECIMATE"; docs/mesh.md §9): the C-ABI declares, binds and
validates the two entry points; the restatement tests/np_mesh_decimate.py stands apart from the product, gives the hand-checked
results on small meshes, keeps analytic spheres within the geometric bound of their surface; and on the CPU model of run_mvs +
run_mesh the recommended cell size removes the share of faces and keeps the share of on-surface vertices that
scripts/calibrate_mesh_decimate.py measured."""
import ast
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

import np_mesh_decimate as nd  # noqa: E402

NEW_SYMBOLS = ("sfm_mesh_decimate_ws_bytes", "sfm_mesh_decimate")

# Calibration (docs/mesh.md §9; seeds 0..2, grid 96, cleaned, 2-voxel cells, without / with 10 Taubin pairs), as measured by
# scripts/calibrate_mesh_decimate.py: the largest faces out / faces in, and the largest fall of the on-surface share below the
# undecimated mesh of the same seed and pair count.
LARGEST_FACE_RATIO = 0.0675           # seed 0 without smoothing (0.0573 .. 0.0675 over the six rows)
LARGEST_ON_SURFACE_FALL = 0.0261      # seed 1 without smoothing: 0.9668 -> 0.9407 (0.0143 .. 0.0261 over the six rows)
MAX_FACE_RATIO = 1.25 * LARGEST_FACE_RATIO
MAX_ON_SURFACE_FALL = 2.0 * LARGEST_ON_SURFACE_FALL if LARGEST_ON_SURFACE_FALL > 0 else 0.002

P20 = 2.0 ** 20


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.int32), b.view(np.int32))


def test_header_declares_and_library_binds_the_decimate_entry_points():
    from test_abi import declared_symbols
    from sfm_mvs_amd import _lib
    syms = declared_symbols()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s in syms and s in _lib.SIGNATURES and hasattr(handle, s), s
    assert _lib.lib().sfm_abi_version() == 3


def check_argument_errors():
    """Every argument error of the header: SFM_ERR_ARG with its message, before any device call (the pointers are never read)."""
    from sfm_mvs_amd import _lib
    L = _lib.lib()
    fake = [ctypes.c_void_p(16 * (k + 1)) for k in range(9)]    # never dereferenced: every check below fails first
    big = 1 << 31
    i3 = lambda *d: (ctypes.c_int32 * 3)(*d)
    f3 = lambda *o: (ctypes.c_float * 3)(*o)
    twin = L.sfm_mesh_decimate_ws_bytes
    assert twin(-1, 4, i3(4, 4, 4)) == 0 and twin(4, -1, i3(4, 4, 4)) == 0 and twin(big, 4, i3(4, 4, 4)) == 0 and twin(4, big, i3(4, 4, 4)) == 0
    assert twin(4, 4, i3(0, 4, 4)) == 0 and twin(4, 4, i3(4, -1, 4)) == 0 and twin(4, 4, i3(512, 512, 513)) == 0 and twin(4, 4, None) == 0
    assert twin(4, 4, i3(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1)) == 0
    assert twin(1000, 2000, i3(8, 8, 8)) >= 76 * 1000 + 4 * 512 + 2000 + 4 * 4096
    assert twin(0, 0, i3(512, 512, 512)) >= 4 << 27 and twin(big - 1, big - 1, i3(1, 1, 1)) >= 76 * (big - 1) + (big - 1) + (4 << 32)
    ws = twin(1000, 2000, i3(8, 8, 8))

    def call(verts=fake[0], colors=None, faces=fake[1], nv=1000, nf=2000, counts=None, origin=f3(0.0, 0.0, 0.0), cell=0.5, dims=i3(8, 8, 8),
             pscale=1024.0, dedupe=1, out_v=fake[2], out_c=None, out_f=fake[3], out_n=fake[4], wsp=fake[5], ws_bytes=1 << 24):
        return L.sfm_mesh_decimate(verts, colors, faces, nv, nf, counts, origin, cell, dims, pscale, dedupe, out_v, out_c, out_f, out_n, wsp,
                                   ws_bytes, None)

    nan, inf = float("nan"), float("inf")
    for kw, msg in [(dict(nv=-1), b"nv_cap"), (dict(nf=-2), b"nf_cap"), (dict(nv=big), b"nv_cap"), (dict(nf=big), b"nf_cap"),
                    (dict(dims=i3(0, 8, 8)), b"dims"), (dict(dims=i3(8, -3, 8)), b"dims"), (dict(dims=i3(8, 8, 0)), b"dims"),
                    (dict(dims=i3(512, 512, 513)), b"dims"), (dict(dims=i3(2 ** 31 - 1, 2 ** 31 - 1, 2)), b"dims"),
                    (dict(cell=0.0), b"cell"), (dict(cell=-1.0), b"cell"), (dict(cell=nan), b"cell"), (dict(cell=inf), b"cell"),
                    (dict(pscale=0.0), b"pscale"), (dict(pscale=-2.0), b"pscale"), (dict(pscale=nan), b"pscale"), (dict(pscale=inf), b"pscale"),
                    (dict(origin=f3(0.0, nan, 0.0)), b"origin"), (dict(origin=f3(inf, 0.0, 0.0)), b"origin"), (dict(origin=f3(0.0, 0.0, -inf)), b"origin"),
                    (dict(dedupe=2), b"dedupe"), (dict(dedupe=-1), b"dedupe"),
                    (dict(verts=None), b"null"), (dict(faces=None), b"null"), (dict(out_v=None), b"null"), (dict(out_f=None), b"null"),
                    (dict(out_n=None), b"null"), (dict(wsp=None), b"null"), (dict(origin=None), b"null"), (dict(dims=None), b"null"),
                    (dict(colors=fake[6]), b"colours"), (dict(out_c=fake[7]), b"colours"),
                    (dict(out_v=fake[0]), b"distinct"), (dict(out_f=fake[1]), b"distinct"), (dict(colors=fake[6], out_c=fake[6]), b"distinct"),
                    (dict(counts=fake[8], out_n=fake[8]), b"distinct"),
                    (dict(ws_bytes=ws - 1), b"workspace"), (dict(ws_bytes=0), b"workspace")]:
        assert call(**kw) == -1, kw
        assert msg in L.sfm_last_error(), (kw, L.sfm_last_error())


def test_argument_errors_are_reported_before_the_device():
    check_argument_errors()


def test_the_restatement_does_not_import_the_product():
    tree = ast.parse(open(os.path.join(ROOT, "tests", "np_mesh_decimate.py")).read())
    for node in ast.walk(tree):
        names = [a.name for a in node.names] if isinstance(node, ast.Import) else [node.module or ""] if isinstance(node, ast.ImportFrom) else []
        assert not any(n.split(".")[0] in ("sfm_mvs_amd", "oracle") for n in names), names


def test_eight_vertices_in_a_two_by_one_by_one_grid():
    """Four vertices per cell: two new vertices at the means (dyadic coordinates: every step is exact), mean colours, and no face
    survives, since a live face needs three different new ids."""
    v = np.array([[1.25, 0.5, 0.5], [0.25, 0.25, 0.75], [1.75, 0.75, 0.25], [0.75, 0.75, 0.25],
                  [1.5, 0.25, 0.5], [0.5, 0.5, 0.5], [1.0, 0.5, 0.75], [0.0, 0.0, 0.0]], np.float32)
    c = np.arange(24, dtype=np.float32).reshape(8, 3)
    f = np.array([[0, 1, 2], [1, 3, 5], [0, 2, 4], [7, 6, 5], [3, 4, 7]], np.int32)
    ov, oc, of, counts = nd.decimate(v, c, f, (0.0, 0.0, 0.0), 1.0, (2, 1, 1), P20)
    assert counts.tolist() == [2, 0, 0, 0] and len(of) == 0
    # vertex 0 (cell 1) is the smallest id overall, so cell 1 comes first; cell 0's leader is vertex 1
    assert same(ov, np.array([[1.375, 0.5, 0.5], [0.375, 0.375, 0.375]], np.float32))
    assert same(oc, np.array([c[[0, 2, 4, 6]].mean(0), c[[1, 3, 5, 7]].mean(0)], np.float32))
    # the same rows in a 2 x 2 x 2 grid of half the cell: vertex 7 alone in cell (0, 0, 0) keeps its position exactly
    ov, _, _, counts = nd.decimate(v, None, f, (0.0, 0.0, 0.0), 0.5, (4, 2, 2), P20)
    newid = nd.cluster(v, None, (0.0, 0.0, 0.0), 0.5, (4, 2, 2), P20, 8)[0]
    assert counts[2] == 0 and same(ov[newid[7]], v[7])


def three_cells():
    """Six vertices, two per cell of a 3 x 1 x 1 grid: new ids 0, 1, 2 for the cells in x order."""
    v = np.array([[0.25, 0.5, 0.5], [0.75, 0.25, 0.5], [1.25, 0.5, 0.25], [1.5, 0.5, 0.5], [2.25, 0.5, 0.5], [2.5, 0.75, 0.5]], np.float32)
    return v, dict(origin=(0.0, 0.0, 0.0), cell=1.0, dims=(3, 1, 1), pscale=P20)


def test_a_face_and_its_rotation_collapse_to_one_face():
    v, fr = three_cells()
    f = np.array([[1, 2, 4], [3, 5, 0], [5, 1, 3]], np.int32)                  # new triples (0 1 2), (1 2 0), (2 0 1)
    ov, _, of, counts = nd.decimate(v, None, f, dedupe=True, **fr)
    assert counts.tolist() == [3, 1, 0, 2] and of.tolist() == [[0, 1, 2]]
    ov, _, of, counts = nd.decimate(v, None, f[::-1], dedupe=True, **fr)         # the lowest input index wins, in ITS corner order
    assert counts.tolist() == [3, 1, 0, 2] and of.tolist() == [[2, 0, 1]]
    ov, _, of, counts = nd.decimate(v, None, f, dedupe=False, **fr)
    assert counts.tolist() == [3, 3, 0, 0] and of.tolist() == [[0, 1, 2], [1, 2, 0], [2, 0, 1]]
    assert same(ov, np.array([[0.5, 0.375, 0.5], [1.375, 0.5, 0.375], [2.375, 0.625, 0.5]], np.float32))


def test_a_face_and_its_flip_stay_two_faces():
    v, fr = three_cells()
    f = np.array([[0, 2, 4], [1, 5, 3], [0, 1, 4], [4, 3, 0]], np.int32)       # (0 1 2), (0 2 1), not live, (2 1 0) = a rotation of the flip
    _, _, of, counts = nd.decimate(v, None, f, dedupe=True, **fr)
    assert counts.tolist() == [3, 2, 0, 1] and of.tolist() == [[0, 1, 2], [0, 2, 1]]


def test_cell_boundaries_and_the_edge_of_the_frame():
    o = np.array([0.5, -1.0, 2.0], np.float32)
    cell = np.float32(0.25)
    fr = dict(origin=o, cell=cell, dims=(4, 4, 4), pscale=P20)
    inside = o + np.float32(0.125)
    rows = [inside.copy() for _ in range(7)]
    rows[1][0] = o[0] + cell                                                    # exactly on the boundary between cells 0 and 1: cell 1
    rows[2][0] = np.nextafter(o[0] + cell, np.float32(-np.inf))                 # just below it: cell 0
    rows[3][1] = np.nextafter(o[1], np.float32(-np.inf))                        # o - tiny: unusable
    rows[4][2] = o[2]                                                           # exactly o: cell 0
    rows[5][2] = o[2] + 4 * cell                                                # exactly o + dims * cell: unusable
    rows[6][2] = np.nextafter(o[2] + 4 * cell, np.float32(-np.inf))             # just below it: the last cell
    v = np.array(rows, np.float32)
    key, _ = nd.cells(v, **fr)
    assert key.tolist() == [0, 1, 0, -1, 0, -1, 48]
    f = np.array([[0, 1, 6], [0, 1, 3], [5, 1, 6], [2, 6, 1]], np.int32)        # a face with an unusable corner is not live
    ov, _, of, counts = nd.decimate(v, None, f, **fr)
    assert counts.tolist() == [3, 2, 2, 0] and of.tolist() == [[0, 1, 2], [0, 2, 1]]
    for bad in (np.nan, np.inf, -np.inf, 1e30):
        w = v.copy()
        w[0, 1] = bad
        assert nd.cells(w, **fr)[0][0] == -1
    # usable by its cell but beyond 2^30 quanta
    assert nd.cells(v, o, cell, (4, 4, 4), 2.0 ** 34)[0].tolist() == [-1, -1, -1, -1, -1, -1, -1]
    assert nd.cells(v, o, cell, (4, 4, 4), 2.0 ** 30)[0].tolist() == [0, 1, 0, -1, 0, -1, 48]


def test_counts_select_the_rows_and_bad_indices_drop_the_face():
    v, fr = three_cells()
    f = np.array([[0, 2, 4], [0, 2, 6], [-1, 2, 4], [0, 2, 2 ** 31 - 1], [1, 3, 5]], np.int32)
    _, _, of, counts = nd.decimate(v, None, f, dedupe=False, **fr)
    assert of.tolist() == [[0, 1, 2], [0, 1, 2]] and counts.tolist() == [3, 2, 0, 0]
    _, _, of, counts = nd.decimate(v, None, f, dedupe=False, counts=(5, 4), **fr)   # vertex 5 gone: face 4 is cut by nf, cell 2 keeps vertex 4
    assert of.tolist() == [[0, 1, 2]] and counts.tolist() == [3, 1, 0, 0]
    for weird in ((-1, 9), (7, -3), (2 ** 31 - 1, 2 ** 31 - 1)):
        assert nd.decimate(v, None, f, dedupe=False, counts=weird, **fr)[3].tolist() == [3, 2, 0, 0]


def sphere_case(centre, radius, cells=2.0):
    from test_mesh_finish_cpu import SPHERE_DIMS, sphere
    v, f, c = sphere(centre, radius)
    origin, cell, dims, extent = nd.frame_of((0.0, 0.0, 0.0), 1.0, SPHERE_DIMS, cells)
    import np_mesh_finish
    return v, f, c, dict(origin=origin, cell=cell, dims=dims, pscale=np_mesh_finish.pscale_of(extent))


@pytest.mark.parametrize("centre,radius", [((11.3, 12.1, 10.7), 6.3), ((12.05, 11.9, 12.2), 5.0), ((10.5, 13.25, 11.9), 8.7)])
def test_spheres_stay_on_the_sphere_and_every_output_face_is_live(centre, radius):
    v, f, c, fr = sphere_case(centre, radius)
    ov, _, of, counts = nd.decimate(v, None, f, dedupe=True, **fr)
    nv, nf = int(counts[0]), int(counts[1])
    print(f"sphere r {radius}: {len(v)} -> {nv} vertices, {len(f)} -> {nf} faces, {counts[3]} duplicates dropped")
    assert counts[2] == 0 and 0 < nf < len(f) / 2 and 0 < nv < len(v) / 2
    # every output face is live and no two are equal
    assert of.min() >= 0 and of.max() < nv
    assert np.all(of[:, 0] != of[:, 1]) and np.all(of[:, 1] != of[:, 2]) and np.all(of[:, 0] != of[:, 2])
    assert len(np.unique(nd.normalise(of.astype(np.int64)), axis=0)) == nf
    # every new id is referenced by an output face, or no input face that touches its cell is live
    newid = nd.cluster(v, None, fr["origin"], fr["cell"], fr["dims"], fr["pscale"], len(v))[0]
    t = newid[f]
    live = (t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])
    assert set(range(nv)) - set(np.unique(of).tolist()) == set(range(nv)) - set(np.unique(t[live]).tolist())
    assert len(nd.decimate(v, None, f, dedupe=False, **fr)[2]) == int(live.sum()) == nf + counts[3]
    # the bound: the members of a cell lie within sqrt(3) cell of each other, and their mean inside their hull
    dist = lambda p: np.abs(np.linalg.norm(p.astype(np.float64) - c, axis=1) - radius)
    e_in = dist(v).max()
    bound = e_in + radius - np.sqrt(radius ** 2 - 3.0 * float(fr["cell"]) ** 2)
    print(f"sphere r {radius}: input within {e_in:.4f}, output within {dist(ov).max():.4f}, bound {bound:.4f}")
    assert dist(ov).max() <= bound


def test_face_order_changes_only_the_order():
    v, f, c, fr = sphere_case((11.3, 12.1, 10.7), 6.3)
    rng = np.random.default_rng(3)
    ov, _, of, counts = nd.decimate(v, None, f, dedupe=True, **fr)
    perm = rng.permutation(len(f))
    pv, _, pf, pcounts = nd.decimate(v, None, f[perm], dedupe=True, **fr)
    assert same(ov, pv) and pcounts.tolist() == counts.tolist()
    key = lambda t: sorted(map(tuple, nd.normalise(t.astype(np.int64)).tolist()))
    assert key(of) == key(pf)


def test_decimate_frame_and_run_mesh_defaults():
    import inspect
    from sfm_mvs_amd import mesh
    sig = inspect.signature(mesh.run_mesh).parameters
    assert sig["decimate"].default == 0 and sig["decimate_dedupe"].default is True and mesh.DECIMATE_CELLS == 2.0
    origin, voxel, dims = np.array([0.5, -1.25, 3.0]), 0.0123, (96, 71, 50)
    for cells in (1.0, 1.5, 2.0, 3.5):
        o, cell, d, extent = mesh.decimate_frame(origin, voxel, dims, cells)
        wo, wcell, wd, wextent = nd.frame_of(origin, voxel, dims, cells)
        assert np.array_equal(o.astype(np.float32), wo) and np.float32(cell) == wcell and tuple(d) == wd and extent == wextent
        assert all(o[k] + cell * d[k] >= origin[k] + voxel * (dims[k] - 1) + cell for k in range(3))      # a margin cell on either side
    for bad in (0.5, -2.0, float("nan"), float("inf")):
        with pytest.raises(mesh.SfmHipError):
            mesh.decimate_frame(origin, voxel, dims, bad)
    with pytest.raises(mesh.SfmHipError):
        mesh.decimate_frame(origin, 1.0, (1024, 1024, 1024), 1.0)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_calibration_on_the_rendered_scenes(seed):
    """np_mvs depth maps, run_mesh's masks, np_mesh at grid 96, the clean-up at the default share, without and with the recommended
    smoothing, then the decimation at the recommended cell: the share of faces left is at most MAX_FACE_RATIO and the on-surface
    share falls by no more than MAX_ON_SURFACE_FALL."""
    from calibrate_mesh_decimate import table
    from test_mesh_clean_cpu import model
    from sfm_mvs_amd import mesh
    assert mesh.DECIMATE_CELLS == 2.0
    rows = table(seed, cells=(mesh.DECIMATE_CELLS,), model=model(seed))
    for pairs in (0, 10):
        (_, _, on0, med0, nv0, nf0), (ratio, dups, on1, med1, nv1, nf1) = rows[(pairs, 0.0)], rows[(pairs, mesh.DECIMATE_CELLS)]
        print(f"seed {seed} pairs {pairs}: {nf0} -> {nf1} faces (ratio {ratio:.4f}, {dups} duplicates dropped), {nv0} -> {nv1} vertices, "
              f"on surface {on0:.4f} -> {on1:.4f}, median angle {med0:.2f} -> {med1:.2f}")
        assert nf0 > 5000 and nf1 > 1000
        assert ratio <= MAX_FACE_RATIO, (ratio, MAX_FACE_RATIO)
        assert on1 >= on0 - MAX_ON_SURFACE_FALL, (on0, on1)
