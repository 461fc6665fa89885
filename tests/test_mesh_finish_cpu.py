"""The mesh finishing step without a GPU (include/sfm_hip.h, "MESH-FINISH"; docs/mesh.md §8): the C-ABI declares, binds and
validates the four entry points; the restatement tests/np_mesh_finish.py stands apart from the product, gives outward normals
and no shrinkage on analytic spheres, does not depend on the order of the faces and leaves alone what the header says it leaves
alone; pipeline.to_ply_mesh writes the normals; and on the CPU model of run_mvs + run_mesh the recommended pair count lowers the
normal error without moving vertices off the surface (scripts/calibrate_mesh_finish.py)."""
import ast
import ctypes
import math
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
import np_mesh_finish as nf  # noqa: E402

NEW_SYMBOLS = ("sfm_mesh_normals_ws_bytes", "sfm_mesh_normals", "sfm_mesh_smooth_ws_bytes", "sfm_mesh_smooth")

# The three spheres of test_mesh_cpu.py: (centre, radius, median angle to the radial, largest angle) of the restatement's normals on
# the unsmoothed np_mesh surface, in degrees, as measured; asserted within a quarter of the value.
SPHERES = [((11.3, 12.1, 10.7), 6.3, 1.909, 7.368), ((12.05, 11.9, 12.2), 5.0, 2.424, 9.337), ((10.5, 13.25, 11.9), 8.7, 1.351, 5.463)]
SPHERE_DIMS = (25, 27, 24)

# Calibration (docs/mesh.md §8, seeds 0..2 at 10 pairs): the median normal error falls by 0.68 / 0.64 / 0.80 degrees and the
# on-surface share rises on every seed (largest fall seen: none).
MIN_MEDIAN_GAIN_DEG = 0.32      # half the smallest gain seen
MAX_ON_SURFACE_FALL = 0.002     # the largest fall seen (0) plus 0.002


def sphere(centre, radius):
    from test_mesh_cpu import field_of
    c = np.array(centre)
    S = field_of(lambda x, y, z: np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - radius, SPHERE_DIMS)
    v, _, f = np_mesh.extract_mesh(S, np.ones_like(S), None, (0.0, 0.0, 0.0), 1.0, 1.0)
    return v, f, c


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.int32), b.view(np.int32))


def test_header_declares_and_library_binds_the_finish_entry_points():
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
    fake, other = ctypes.c_void_p(16), ctypes.c_void_p(32)      # never dereferenced: every check below fails first
    big = 1 << 31
    org = (ctypes.c_float * 3)(0.0, 0.0, 0.0)
    fac = (ctypes.c_float * 4)(0.5, -0.53, 0.5, -0.53)

    for twin, per_vertex in ((L.sfm_mesh_normals_ws_bytes, 32), (L.sfm_mesh_smooth_ws_bytes, 56)):
        assert twin(-1, 4) == 0 and twin(4, -1) == 0 and twin(big, 4) == 0 and twin(4, big) == 0
        assert twin(1000, 2000) >= per_vertex * 1000 and twin(big - 1, big - 1) >= per_vertex * (big - 1)
    nws, sws = L.sfm_mesh_normals_ws_bytes(1000, 2000), L.sfm_mesh_smooth_ws_bytes(1000, 2000)

    def normals(verts=fake, faces=fake, nv=1000, nf=2000, counts=None, out=other, ws=fake, ws_bytes=1 << 20):
        return L.sfm_mesh_normals(verts, faces, nv, nf, counts, out, ws, ws_bytes, None)

    for kw, msg in [(dict(nv=-1), b"nv_cap"), (dict(nf=-2), b"nf_cap"), (dict(nv=big), b"nv_cap"), (dict(nf=big), b"nf_cap"),
                    (dict(verts=None), b"null"), (dict(faces=None), b"null"), (dict(out=None), b"null"), (dict(ws=None), b"null"),
                    (dict(out=fake), b"distinct"), (dict(ws_bytes=nws - 1), b"workspace"), (dict(ws_bytes=0), b"workspace")]:
        assert normals(**kw) == -1, kw
        assert msg in L.sfm_last_error(), (kw, L.sfm_last_error())

    def smooth(verts=fake, faces=fake, nv=1000, nf=2000, counts=None, nsteps=4, factors=fac, origin=org, pscale=1024.0, out=other, ws=fake,
               ws_bytes=1 << 20):
        return L.sfm_mesh_smooth(verts, faces, nv, nf, counts, nsteps, factors, origin, pscale, out, ws, ws_bytes, None)

    nan, inf = float("nan"), float("inf")
    for kw, msg in [(dict(nv=-1), b"nv_cap"), (dict(nf=-2), b"nf_cap"), (dict(nv=big), b"nv_cap"), (dict(nf=big), b"nf_cap"),
                    (dict(verts=None), b"null"), (dict(faces=None), b"null"), (dict(out=None), b"null"), (dict(ws=None), b"null"),
                    (dict(origin=None), b"null"), (dict(factors=None), b"null"), (dict(out=fake), b"distinct"),
                    (dict(nsteps=-1), b"nsteps"), (dict(nsteps=65), b"nsteps"),
                    (dict(factors=(ctypes.c_float * 4)(0.5, nan, 0.5, 0.5)), b"factor"), (dict(factors=(ctypes.c_float * 4)(0.5, 0.5, 0.5, -inf)), b"factor"),
                    (dict(origin=(ctypes.c_float * 3)(0.0, nan, 0.0)), b"origin"), (dict(origin=(ctypes.c_float * 3)(inf, 0.0, 0.0)), b"origin"),
                    (dict(pscale=0.0), b"pscale"), (dict(pscale=-2.0), b"pscale"), (dict(pscale=nan), b"pscale"), (dict(pscale=inf), b"pscale"),
                    (dict(ws_bytes=sws - 1), b"workspace"), (dict(ws_bytes=0), b"workspace")]:
        assert smooth(**kw) == -1, kw
        assert msg in L.sfm_last_error(), (kw, L.sfm_last_error())


def test_the_restatement_does_not_import_the_product():
    tree = ast.parse(open(os.path.join(ROOT, "tests", "np_mesh_finish.py")).read())
    for node in ast.walk(tree):
        names = [a.name for a in node.names] if isinstance(node, ast.Import) else [node.module or ""] if isinstance(node, ast.ImportFrom) else []
        assert not any(n.split(".")[0] in ("sfm_mvs_amd", "oracle") for n in names), names


def radial_angles(p, n, c):
    rad = p.astype(np.float64) - c
    rad /= np.linalg.norm(rad, axis=1, keepdims=True)
    dot = np.einsum("ij,ij->i", n.astype(np.float64), rad)
    return dot, np.degrees(np.arccos(np.clip(dot, -1.0, 1.0)))


@pytest.mark.parametrize("centre,radius,median,largest", SPHERES)
def test_sphere_normals_point_outward_and_smoothing_does_not_shrink(centre, radius, median, largest):
    v, f, c = sphere(centre, radius)
    n = nf.normals(v, f)
    assert n.dtype == np.float32 and n.shape == v.shape
    assert np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1.0).max() < 1e-6
    dot, ang = radial_angles(v, n, c)
    print(f"sphere r {radius}: {len(v)} vertices, angle to the radial median {np.median(ang):.3f} max {ang.max():.3f} degrees")
    assert np.all(dot > 0)
    assert abs(np.median(ang) - median) <= median / 4 and abs(ang.max() - largest) <= largest / 4
    p = nf.smooth(v, f, nf.taubin_factors(10), (0.0, 0.0, 0.0), nf.pscale_of(max(SPHERE_DIMS) - 1))
    err = np.abs(np.linalg.norm(p.astype(np.float64) - c, axis=1) - radius).max()
    dot10, ang10 = radial_angles(p, nf.normals(p, f), c)
    print(f"sphere r {radius}: after 10 pairs radius error {err:.4f} voxels, angle median {np.median(ang10):.3f} max {ang10.max():.3f}")
    assert err <= 0.1 and np.all(dot10 > 0) and np.median(ang10) < np.median(ang)


def test_face_order_steps_zero_and_untouched_vertices():
    v, f, c = sphere(*SPHERES[0][:2])
    rng = np.random.default_rng(3)
    origin, pscale = np.array([0.5, -1.0, 0.25], np.float32), nf.pscale_of(26.0)
    fac = nf.taubin_factors(3)
    perm = rng.permutation(len(f))
    assert same(nf.normals(v, f[perm]), nf.normals(v, f))
    assert same(nf.smooth(v, f[perm], fac, origin, pscale), nf.smooth(v, f, fac, origin, pscale))
    assert not same(nf.smooth(v, f, fac, origin, pscale), v)
    # steps = 0: the rows, NaN payloads included
    odd = v.copy()
    odd.view(np.int32)[5] = (0x7FC00123, 0x7F800001, -4194304 + 77)
    assert same(nf.smooth(odd, f, [], origin, pscale), odd)
    # a vertex in no face, a vertex that is not usable (NaN, beyond 2^30 quanta) and its neighbours' sums
    extra = np.array([[3.0, 4.0, 5.0]], np.float32)                    # in no face
    w = np.vstack([v, extra])
    far = int(f[0, 0])
    w[far] = (1e9, 3.0, 3.0)                                           # |r| > 2^30 at this pscale
    nanv = int(f[100, 1])
    w.view(np.int32)[nanv] = (0x7FC00123, 0, 0)
    out = nf.smooth(w, f, fac, origin, pscale)
    for k in (len(v), far, nanv):
        assert np.array_equal(out.view(np.int32)[k], w.view(np.int32)[k]), k
    # ... and they pull nobody: the same result as with those vertices' faces' other corners seeing only each other
    r, usable = nf.quantise(w, origin, pscale)
    assert not usable[far] and not usable[nanv] and usable[len(v)] and usable.sum() == len(w) - 2
    nb = np.unique(f[np.any(f == far, axis=1)])
    nb = nb[(nb != far) & (nb != nanv)]
    one = nf.smooth_step(w, f, np.float32(1.0), origin, pscale)        # factor 1: the mean of the usable neighbours
    assert np.all(np.isfinite(one[nb])) and np.abs(one[nb]).max() < 30.0
    # normals: a face-less vertex and a vertex of zero-area faces only get (0, 0, 0); out-of-range faces contribute nothing
    flat = np.vstack([v, extra, extra])
    ff = np.vstack([f, [[len(v), len(v) + 1, 0], [0, 1, len(flat)], [-1, 0, 1]]]).astype(np.int32)
    n2 = nf.normals(flat, ff)
    assert same(n2[:len(v)], nf.normals(v, f)) and not n2[len(v):].any()
    # device counts: a prefix of the rows and faces
    nv2, nk2 = len(v) - 7, len(f) - 100
    assert same(nf.normals(v, f, (nv2, nk2)), nf.normals(v[:nv2], f[:nk2]))
    assert same(nf.normals(v, f, (-1, len(f) + 1)), nf.normals(v, f))
    assert nf.pscale_of(26.0) == 2.0 ** 24 and nf.pscale_of(2.0 ** 29) == 1.0 and nf.pscale_of(0.75) == 2.0 ** 29


def test_wrapper_scale_equals_the_restatements():
    from sfm_mvs_amd import mesh
    for extent in (26.0, 1.0, 0.75, 2.0 ** 29, 3e-5, 7e7, 1e-40, 1e39):
        assert mesh.smooth_scale(extent) == nf.pscale_of(extent), extent
        assert extent * mesh.smooth_scale(extent) <= 2.0 ** 29
    for extent in (26.0, 1.0, 0.75, 2.0 ** 29, 2.0 ** 29 + 64.0, 3e-5, 7e7, 0.1, 1.0 / 3, 12345.678, 2.0 ** -20, 1e-25, 1e30):   # not clamped
        p = mesh.smooth_scale(extent)
        assert math.frexp(p)[0] == 0.5, (extent, p)                                    # a power of two
        assert extent * p <= 2.0 ** 29 < extent * (2.0 * p), (extent, p)               # the largest one that fits
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(mesh.SfmHipError):
            mesh.smooth_scale(bad)


def test_to_ply_mesh_with_and_without_normals(tmp_path):
    from sfm_mvs_amd.pipeline import to_ply_mesh
    rng = np.random.default_rng(2)
    v = rng.normal(0, 1, (40, 3))
    c = rng.uniform(0, 255, (40, 3))
    f = rng.integers(0, 40, (60, 3)).astype(np.int32)
    n = rng.normal(0, 1, (40, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    os.makedirs(tmp_path / "Point_Cloud")
    path = tmp_path / "Point_Cloud" / "dense_mesh.ply"
    assert to_ply_mesh(str(tmp_path), v, c, f) == (40, 60)
    four = open(path, "rb").read()
    assert to_ply_mesh(str(tmp_path), v, c, f, normals=None) == (40, 60)
    assert open(path, "rb").read() == four and b"nx" not in four
    assert to_ply_mesh(str(tmp_path), v, c, f, n) == (40, 60)
    head, body = open(path).read().split("end_header\n")
    props = [ln.split()[-1] for ln in head.splitlines() if ln.startswith("property") and "list" not in ln]
    assert props == ["x", "y", "z", "nx", "ny", "nz", "blue", "green", "red"]
    assert "property float nx\n" in head and "property float nz\n" in head
    rows = body.strip().splitlines()
    assert len(rows) == 100
    vt = np.array([r.split() for r in rows[:40]], np.float64)
    assert np.allclose(vt[:, :3], 200 * v, atol=1e-5) and np.allclose(vt[:, 3:6], n, atol=1e-6)       # unscaled
    assert np.array_equal(vt[:, 6:], np.clip(np.floor(c + 0.5), 0, 255))
    ft = np.array([r.split() for r in rows[40:]], np.int64)
    assert np.all(ft[:, 0] == 3) and np.array_equal(ft[:, 1:], f)
    with pytest.raises(ValueError):
        to_ply_mesh(str(tmp_path), v, c, f, n[:-1])


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_calibration_on_the_rendered_scenes(seed):
    """np_mvs depth maps, run_mesh's masks, np_mesh at grid 96, the clean-up at the default share, then smoothing at the
    recommended pair count and the normals: against the normals of the ground-truth depth maps the median error falls by at
    least MIN_MEDIAN_GAIN_DEG and the on-surface share falls by no more than MAX_ON_SURFACE_FALL."""
    from calibrate_mesh_finish import table
    from test_mesh_clean_cpu import model
    from sfm_mvs_amd import mesh
    assert mesh.SMOOTH_PAIRS == 10
    rows = table(seed, pairs=(0, mesh.SMOOTH_PAIRS), model=model(seed))
    (m0, p0, t0, on0, k0), (m1, p1, t1, on1, k1) = rows[0], rows[mesh.SMOOTH_PAIRS]
    print(f"seed {seed}: median {m0:.2f} -> {m1:.2f}, 90th percentile {p0:.2f} -> {p1:.2f}, above 30 degrees {100 * t0:.2f} % -> {100 * t1:.2f} %, "
          f"on surface {on0:.4f} -> {on1:.4f}, scored {k0} / {k1}")
    assert k0 > 5000 and k1 > 5000
    assert m0 - m1 >= MIN_MEDIAN_GAIN_DEG, (m0, m1)
    assert on1 >= on0 - MAX_ON_SURFACE_FALL, (on0, on1)


def test_run_mesh_defaults_stay_off():
    import inspect
    from sfm_mvs_amd import mesh
    sig = inspect.signature(mesh.run_mesh).parameters
    assert sig["normals"].default is False and sig["smooth"].default == 0
    assert sig["smooth_lambda"].default == 0.5 and sig["smooth_mu"].default == -0.53
