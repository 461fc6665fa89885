"""The mesh clean-up without a GPU (include/sfm_hip.h, "MESH-CLEAN"; docs/mesh.md §7): the C-ABI declares, binds and validates the
four entry points; the integer restatement tests/np_mesh_clean.py stands apart from the product, agrees with SciPy's connected
components on np_mesh surfaces and follows every branch of the keep rule on a hand-built mesh; and on the CPU model of
run_mvs + run_mesh the clean-up at run_mesh's default share raises the on-surface share for under 1 % of the faces."""
import ast
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

import np_mesh  # noqa: E402
import np_mesh_clean as npc  # noqa: E402

NEW_SYMBOLS = ("sfm_mesh_components_ws_bytes", "sfm_mesh_components", "sfm_mesh_clean_ws_bytes", "sfm_mesh_clean")
# Calibration (docs/mesh.md §7; measured gains 0.0044 / 0.0085 / 0.0065 and >= 99.3 % of the faces kept on seeds 0..2).
MIN_GAIN = 0.002
MIN_FACES_KEPT = 0.99


def test_header_declares_and_library_binds_the_clean_entry_points():
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
    big = 1 << 31

    assert L.sfm_mesh_components_ws_bytes(-1, 4) == 0 and L.sfm_mesh_components_ws_bytes(4, -1) == 0
    assert L.sfm_mesh_components_ws_bytes(big, 4) == 0 and L.sfm_mesh_components_ws_bytes(4, big) == 0
    assert L.sfm_mesh_clean_ws_bytes(-1, 4) == 0 and L.sfm_mesh_clean_ws_bytes(4, -1) == 0 and L.sfm_mesh_clean_ws_bytes(big, 0) == 0
    cws = L.sfm_mesh_components_ws_bytes(100, 100)
    assert cws > 0 and L.sfm_mesh_components_ws_bytes(0, 0) > 0 and L.sfm_mesh_components_ws_bytes(big - 1, big - 1) > 0
    kws = L.sfm_mesh_clean_ws_bytes(1000, 2000)
    assert kws >= 8 * 1000 and L.sfm_mesh_clean_ws_bytes(0, 0) > 0
    assert L.sfm_mesh_clean_ws_bytes(big - 1, big - 1) >= 8 * (big - 1)

    def comp(faces=fake, nv=100, nf=100, rounds=8, resume=0, labels=fake, status=fake, ws=fake, ws_bytes=1 << 20):
        return L.sfm_mesh_components(faces, nv, nf, rounds, resume, labels, status, ws, ws_bytes, None)

    for kw, msg in [(dict(nv=-1), b"nv"), (dict(nf=-1), b"nf"), (dict(nv=big), b"nv"), (dict(nf=big), b"nf"), (dict(rounds=0), b"rounds"),
                    (dict(rounds=1025), b"rounds"), (dict(rounds=-3), b"rounds"), (dict(faces=None), b"null"), (dict(labels=None), b"null"),
                    (dict(status=None), b"null"), (dict(ws=None), b"null"), (dict(nv=0, nf=0, status=None), b"null"),
                    (dict(ws_bytes=cws - 1), b"workspace"), (dict(ws_bytes=0), b"workspace")]:
        assert comp(**kw) == -1, kw
        assert msg in L.sfm_last_error(), (kw, L.sfm_last_error())

    def clean(verts=fake, colors=None, faces=fake, nv=1000, nf=2000, labels=fake, min_faces=1, largest=0, out_v=fake, out_c=None,
              out_f=fake, counts=fake, ws=fake, ws_bytes=1 << 20):
        return L.sfm_mesh_clean(verts, colors, faces, nv, nf, labels, min_faces, largest, out_v, out_c, out_f, counts, ws, ws_bytes, None)

    for kw, msg in [(dict(nv=-1), b"nv"), (dict(nf=-2), b"nf"), (dict(nv=big), b"nv"), (dict(min_faces=-1), b"min_faces"),
                    (dict(largest=2), b"largest_only"), (dict(verts=None), b"null"), (dict(out_v=None), b"null"), (dict(faces=None), b"null"),
                    (dict(out_f=None), b"null"), (dict(labels=None), b"null"), (dict(counts=None), b"null"), (dict(ws=None), b"null"),
                    (dict(nv=0, nf=0, counts=None), b"null"), (dict(colors=fake), b"colours"), (dict(out_c=fake), b"colours"),
                    (dict(ws_bytes=kws - 1), b"workspace"), (dict(ws_bytes=0), b"workspace")]:
        assert clean(**kw) == -1, kw
        assert msg in L.sfm_last_error(), (kw, L.sfm_last_error())


def test_the_restatement_does_not_import_the_product():
    tree = ast.parse(open(os.path.join(ROOT, "tests", "np_mesh_clean.py")).read())
    for node in ast.walk(tree):
        names = [a.name for a in node.names] if isinstance(node, ast.Import) else [node.module or ""] if isinstance(node, ast.ImportFrom) else []
        assert not any(n.split(".")[0] in ("sfm_mvs_amd", "oracle") for n in names), names


def field_of(fn, dims):
    nx, ny, nz = dims
    z, y, x = np.meshgrid(np.arange(nz, dtype=np.float64), np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64), indexing="ij")
    return fn(x, y, z).astype(np.float32)


def surfaces():
    """(name, vertices, faces) of np_mesh meshes: two spheres in one field, a torus, the ground-truth scene with its debris."""
    from mvs_scenes import render_scene, scene_cloud
    from sfm_mvs_amd import mesh
    S = field_of(lambda x, y, z: np.minimum(np.sqrt((x - 8.3) ** 2 + (y - 9.1) ** 2 + (z - 8.2) ** 2) - 5.4,
                                            np.sqrt((x - 24.6) ** 2 + (y - 9.4) ** 2 + (z - 8.9) ** 2) - 4.1), (33, 19, 17))
    v, _, f = np_mesh.extract_mesh(S, np.ones_like(S), None, (0.0, 0.0, 0.0), 1.0, 1.0)
    yield "spheres", v, f, 2
    S = field_of(lambda x, y, z: np.sqrt((np.sqrt((x - 16.2) ** 2 + (y - 15.1) ** 2) - 9.0) ** 2 + (z - 8.3) ** 2) - 3.6, (33, 31, 17))
    v, _, f = np_mesh.extract_mesh(S, np.ones_like(S), None, (0.0, 0.0, 0.0), 1.0, 1.0)
    yield "torus", v, f, 1
    imgs, K, P, gt = render_scene(n=5, w=160, h=120, seed=0)
    origin, voxel, dims = mesh.volume_bounds(scene_cloud(K, P, gt), 64)
    S, W, _ = np_mesh.tsdf_integrate(np.stack(gt).astype(np.float32), mesh.projection_rows(K, P), origin, voxel, dims, mesh.TRUNC_VOXELS * voxel)
    v, _, f = np_mesh.extract_mesh(S, W, None, origin, voxel, mesh.W_MIN)
    yield "scene", v, f, None


def test_labels_and_face_counts_equal_scipy_connected_components():
    sparse = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import connected_components
    for name, v, f, ncomp in surfaces():
        nv = len(v)
        labels, faces_of = npc.components(f, nv)
        e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]]]).astype(np.int64)
        n, comp = connected_components(sparse.coo_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(nv, nv)), directed=False)
        low = np.full(n, nv, np.int64)
        np.minimum.at(low, comp, np.arange(nv))
        assert np.array_equal(labels, low[comp]), name
        want = np.zeros(nv, np.int64)
        np.add.at(want, low[comp[f[:, 0]]], 1)
        assert np.array_equal(faces_of, want), name
        assert n == int((labels == np.arange(nv)).sum())
        if ncomp is not None:
            assert n == ncomp, (name, n)
        else:
            assert n > 1, name


def hand_mesh():
    """7 vertices: {0, 1, 2} two faces (one of them (a, a, b)), {3, 4, 5} two faces, 6 in no valid face; one invalid face."""
    v = np.arange(21, dtype=np.float32).reshape(7, 3)
    v[6, 0] = np.nan
    c = 100.0 + v
    f = np.array([[3, 4, 5], [0, 1, 2], [6, 7, 0], [2, 2, 0], [5, 3, 4], [-1, 1, 2]], np.int32)
    return v, c, f


def test_hand_built_mesh_follows_every_branch_of_the_keep_rule():
    v, c, f = hand_mesh()
    labels, faces_of = npc.components(f, 7)
    assert labels.tolist() == [0, 0, 0, 3, 3, 3, 6] and faces_of.tolist() == [2, 0, 0, 2, 0, 0, 0]

    def run(min_faces, largest=False):
        ov, oc, of, counts = npc.clean(v, c, f, min_faces, largest)
        assert np.array_equal(oc.view(np.int32), (100.0 + ov).astype(np.float32).view(np.int32)) or np.isnan(ov).any()
        return ov[:, 1].astype(int).tolist(), of.tolist(), counts.tolist()

    # min_faces 0 keeps everything (the face-less vertex too); the invalid faces are never output
    assert run(0) == ([1, 4, 7, 10, 13, 16, 19], [[3, 4, 5], [0, 1, 2], [2, 2, 0], [5, 3, 4]], [7, 4, 3, 3])
    ov, oc, _, _ = npc.clean(v, c, f, 0)
    assert np.array_equal(ov.view(np.int32), v.view(np.int32)) and np.array_equal(oc.view(np.int32), c.view(np.int32))   # the NaN too
    # min_faces 1 drops the face-less vertex; 2 keeps both pairs; 3 nothing
    assert run(1) == ([1, 4, 7, 10, 13, 16], [[3, 4, 5], [0, 1, 2], [2, 2, 0], [5, 3, 4]], [6, 4, 3, 2])
    assert run(2) == run(1)
    assert run(3) == ([], [], [0, 0, 3, 0])
    # largest_only: two components tied on 2 faces, the lower label wins; it must pass min_faces as well
    assert run(0, True) == ([1, 4, 7], [[0, 1, 2], [2, 2, 0]], [3, 2, 3, 1])
    assert run(2, True) == run(0, True)
    assert run(3, True) == ([], [], [0, 0, 3, 0])
    # the tie broken by a third face on the higher component
    f2 = np.vstack([f, [[4, 4, 4]]]).astype(np.int32)
    ov, _, of, counts = npc.clean(v, c, f2, 0, True)
    assert ov[:, 1].astype(int).tolist() == [10, 13, 16] and of.tolist() == [[0, 1, 2], [2, 0, 1], [1, 1, 1]] and counts.tolist() == [3, 3, 3, 1]
    # no faces at all: every vertex its own component
    assert npc.clean(v, None, np.zeros((0, 3), np.int32), 0)[3].tolist() == [7, 0, 7, 7]
    assert npc.clean(v, None, np.zeros((0, 3), np.int32), 1)[3].tolist() == [0, 0, 7, 0]
    assert npc.clean(v, None, np.zeros((0, 3), np.int32), 0, True)[3].tolist() == [1, 0, 7, 1]


@functools.lru_cache(maxsize=None)
def model(seed):
    from calibrate_mesh_clean import model_mesh
    return model_mesh(seed)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_calibration_on_the_rendered_scenes(seed):
    """np_mvs depth maps, run_mesh's masks, np_mesh at grid 96, then the clean-up at run_mesh's default share: the on-surface share
    rises by at least MIN_GAIN and at least MIN_FACES_KEPT of the faces stay."""
    from calibrate_mesh_clean import share_threshold
    from test_mesh_cpu import on_surface_fraction
    v, c, f, K, P, gt, voxel = model(seed)
    t = share_threshold(len(f))
    assert 32 <= t <= 64, t                                   # inside the flat band of the table
    kv, kc, kf, counts = npc.clean(v, c, f, t)
    before, after = on_surface_fraction(v, K, P, gt, voxel), on_surface_fraction(kv, K, P, gt, voxel)
    print(f"seed {seed}: {len(f)} faces, threshold {t}, on surface {before:.4f} -> {after:.4f}, faces kept {len(kf) / len(f):.4f}, "
          f"components {counts[2]} -> {counts[3]}")
    assert after - before >= MIN_GAIN, (before, after)
    assert len(kf) >= MIN_FACES_KEPT * len(f), (len(kf), len(f))
    assert counts[3] < counts[2] and kf.max() < len(kv) and kf.min() >= 0
