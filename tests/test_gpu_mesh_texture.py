"""The mesh texturing step on the device (sfm_mesh_render_depth, sfm_mesh_face_views, sfm_mesh_texture_fill, mesh.texture_mesh,
run_mesh(texture=True)): every output equal to the restatement tests/np_mesh_texture.py, the depth maps and the scores as int32
views, every atlas byte; there is no tolerance anywhere (include/sfm_hip.h, "MESH-TEXTURE"; docs/mesh.md §10)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

import np_mesh  # noqa: E402
import np_mesh_texture as nt  # noqa: E402
import fuzz_mesh_texture as fz  # noqa: E402
from fuzz_mesh_clean import bits, up  # noqa: E402
from test_mesh_texture_cpu import pinhole  # noqa: E402

INT32_MAX = 2 ** 31 - 1
FUZZ_FLOOR = 1000               # cases the committed logs hold together, at least
F = np.float32


def chain(v, c, f, P, frames, vis_tol=0.02, texels=4, counts=None):
    """The three calls (into sentinel-filled buffers) against the restatement -> the restated (zbuf, face_view, face_score, atlas)."""
    bad, want = fz.check_chain(v, c, f, P, frames, vis_tol, texels, counts)
    assert not bad, (bad, len(v), len(f), frames.shape, vis_tol, texels, counts)
    return want


def random_frames(rng, n, h, w):
    return rng.integers(0, 256, (n, h, w, 3)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def real_mesh(name):
    """(vertices, colours, faces) of the restated extraction at grid 64: a sphere of radius 0.9 around the origin, or the rendered
    scene of seed 0 from its ground-truth depth maps."""
    if name == "scene":
        from calibrate_mesh_texture import model
        m = model(0, 64)
        return m["v"], m["c"], m["f"]
    from test_gpu_mesh import sphere_field
    voxel = 2.4 / 63
    S = sphere_field((64, 64, 64), (31.3, 30.9, 32.2), 0.9 / voxel)
    v, _, f = np_mesh.extract_mesh(2.0 * S, np.full_like(S, 2.0), None, np.full(3, -1.2, F), F(voxel), 1.0)
    c = (np.random.default_rng(11).random((len(v), 3)) * 255.0).astype(F)
    return v, c, f


@pytest.mark.gpu
@pytest.mark.parametrize("nviews", [3, 5])
@pytest.mark.parametrize("name", ["sphere", "scene"])
def test_real_meshes_equal_the_restatement(hip, name, nviews):
    from sfm_mvs_amd import mesh
    v, c, f = real_mesh(name)
    assert len(f) > 10000
    rng = np.random.default_rng(nviews)
    w, h = 160, 120
    Ps = fz.arc_views(rng, nviews, w, h)
    P = fz.rows_of(Ps)
    frames = random_frames(rng, nviews, h, w)
    for texels in (1, 4, 8):
        wz, wv, ws, wa = chain(v, c, f, P, frames, mesh.VIS_TOL, texels)
    assert np.isfinite(wz).mean() > 0.05 and (wv >= 0).mean() > 0.3 and len(np.unique(wv)) >= 3
    # the Python operators, one after another with no host read in between, and texture_mesh
    dv, dc, df = up(v), up(c), up(f)
    z = mesh.render_depth(dv, df, P, w, h)
    fv, fs = mesh.face_views(dv, df, P, z)
    atlas = mesh.texture_fill(dv, dc, df, P, up(frames), fv, 8)
    assert np.array_equal(bits(z), bits(wz)) and np.array_equal(fv.cpu().numpy(), wv) and np.array_equal(bits(fs), bits(ws))
    assert np.array_equal(atlas.cpu().numpy(), wa)
    out = mesh.texture_mesh(v, c, f, list(frames), np.eye(3), Ps)
    assert np.array_equal(out["atlas"], wa) and np.array_equal(out["face_view"], wv) and out["textured"] == int((wv >= 0).sum())
    assert np.array_equal(out["uv"], nt.uv_of(len(f), 8)) and out["atlas"].shape == (nt.layout(len(f), 8)[0],) * 2 + (3,)


SIZES = [0, 1, 2, 3, 255, 256, 257, 65537]


def soup_case(rng, nv, nk, w=64, h=48, n=3):
    """A face soup in front of three pinhole cameras (depth = z + 4): a quarter of the indices name no vertex, a tenth of the faces
    are (a, a, a) or repeat a face, rows that are NaN / inf / 1e30, rows behind and exactly on the camera plane, and a walk wide
    enough that triangles hang off every edge of the frame."""
    P = fz.rows_of(fz.pinhole_views(rng, n, w, h))
    v = fz.walk(rng, nv, 0.05, 3.0)
    f = fz.walk_soup(rng, nv, nk, 300)
    if nk:
        hit = rng.random((nk, 3)) < 0.25
        f[hit] = rng.choice(np.array([-1, nv, INT32_MAX], np.int64), int(hit.sum())).astype(np.int32)
    if nk > 3:
        k = rng.random(nk) < 0.1
        f[k, 1] = f[k, 0]
        f[k, 2] = f[k, 0]
        f[rng.random(nk) < 0.05] = f[1]
    if nv:
        hit = rng.random((nv, 3)) < 0.02
        v[hit] = rng.choice(np.array([np.nan, np.inf, -np.inf, 1e30, -1e30], F), int(hit.sum()))
        hit = rng.random(nv) < 0.05
        v[hit, 2] = rng.choice(np.array([-4.0, -4.5, -3.9999998, -6.0], F), int(hit.sum()))
    c = (rng.random((nv, 3)) * 255.0).astype(F)
    return v, c, f, P, random_frames(rng, n, h, w)


@pytest.mark.gpu
@pytest.mark.parametrize("nk", SIZES)
def test_random_face_soups_at_the_block_edges(hip, nk):
    """nf at 0..3, around one 256-block and past 2^16, nv independently of it; three views of 64 x 48."""
    for case, nv in enumerate((0, 3, 257, 65537) if SIZES.index(nk) % 2 == 0 else (1, 2, 255, 256)):
        rng = np.random.default_rng(1000003 * nv + 101 * nk)
        v, c, f, P, frames = soup_case(rng, nv, nk)
        wz, wv, ws, wa = chain(v, c if case % 2 else None, f, P, frames, 0.02, (1, 4, 2, 8)[case] if nk < 60000 else 1)
        if nk == 65537 and nv == 65537:
            # what the soup is meant to contain, asserted on the restatement
            stats = {}
            nt.render_depth(v, f, P, 64, 48, stats=stats)
            assert stats["over_64"] > 20 and stats["boxes"] > 10000, stats
            sx, sy, sz, ok = nt.project(P[0], v)
            good = np.all((f >= 0) & (f < nv), axis=1)
            t = f[good]
            for lo, hi in ((sx < 0, sx > 0), (sx > 63, sx < 63), (sy < 0, sy > 0), (sy > 47, sy < 47)):
                assert np.any(ok[t].all(axis=1) & lo[t].any(axis=1) & hi[t].any(axis=1)), "no triangle hangs off this edge"
            assert (~ok).sum() > 100 and (sz == 0).sum() > 10 and (sz < 0).sum() > 10 and np.isnan(v).any()
            assert np.isfinite(wz).mean() > 0.2 and (wv >= 0).sum() > 100 and (wv < 0).sum() > 1000


@pytest.mark.gpu
def test_a_triangle_over_the_whole_frame_and_one_over_a_pixel_and_a_half(hip):
    w, h = 160, 120
    P = np.stack([pinhole(w, h, tz=4.0), pinhole(w, h, tx=0.3, tz=4.0)])
    px = 4.0 / (0.9 * w)                                             # one pixel at z = 0
    v = np.array([[-40.0, -40.0, 1.0], [40.0, -40.0, 1.0], [0.0, 60.0, 1.0],
                  [4.25 * px, 4.25 * px, 0.0], [5.75 * px, 4.25 * px, 0.0], [4.25 * px, 6.25 * px, 0.0]], F)     # screen (83.75, 63.75) + (1.5, 2)
    frames = random_frames(np.random.default_rng(0), 2, h, w)
    for big in ([0, 1, 2], [0, 2, 1]):
        f = np.array([big, [3, 5, 4]], np.int32)
        stats = {}
        nt.render_depth(v, f, P, w, h, stats=stats)
        wz, wv, ws, wa = chain(v, None, f, P, frames, 0.02, 8)
        assert np.isfinite(wz).all() and stats["over_64"] == 2        # the large triangle covers both frames entirely
        near = wz < 4.5
        assert 1 <= near[0].sum() <= 4 and 1 <= near[1].sum() <= 4    # the small one: a pixel or a few
        assert wv[0] == -1 and wv[1] >= 0                             # the large one leaves the frame; the small one is seen
    # and a frame of the largest size the header takes a whole-frame triangle through quickly: 1024 x 512
    w, h = 1024, 512
    P = pinhole(w, h, tz=4.0)[None]
    z = fz.raw_render(v[:3], np.array([[0, 1, 2]], np.int32), P, w, h)
    want = nt.render_depth(v[:3], np.array([[0, 1, 2]], np.int32), P, w, h)
    assert np.array_equal(bits(z), bits(want)) and np.isfinite(want).all()


@pytest.mark.gpu
def test_two_coplanar_faces_sharing_an_edge_through_pixel_centres(hip):
    """A square split along its diagonal, corners and diagonal on pixel centres: the pixels of the diagonal belong to both faces and
    are covered (no hole), whichever face lands first."""
    w, h = 32, 24
    P = pinhole(w, h, fl=8.0, tz=4.0)[None]                          # sx = 2 x + 15.5, sy = 2 y + 11.5 at z = 0
    v = np.array([[-5.25, -3.25, 0.0], [-1.25, -3.25, 0.0], [-5.25, 0.75, 0.0], [-1.25, 0.75, 0.0]], F)       # screen (5, 5) .. (13, 13)
    sx, sy, _, _ = nt.project(P[0], v)
    assert sx.tolist() == [5.0, 13.0, 5.0, 13.0] and sy.tolist() == [5.0, 5.0, 13.0, 13.0]
    frames = random_frames(np.random.default_rng(1), 1, h, w)
    for f in ([[0, 2, 1], [1, 2, 3]], [[1, 2, 3], [0, 2, 1]], [[0, 1, 2], [1, 2, 3]]):
        wz, wv, ws, wa = chain(v, None, np.array(f, np.int32), P, frames, 0.0, 4)
        cov = np.isfinite(wz[0])
        assert cov.sum() == 81 and cov[5:14, 5:14].all()
        one = np.isfinite(nt.render_depth(v, np.array(f[:1], np.int32), P, w, h)[0])
        two = np.isfinite(nt.render_depth(v, np.array(f[1:], np.int32), P, w, h)[0])
        assert (one & two).sum() == 9 and all((one & two)[13 - k, 5 + k] for k in range(9))


@pytest.mark.gpu
def test_a_sample_exactly_at_the_visibility_bound(hip):
    """depth == zbuf * (1 + vis_tol) passes and one ulp less of zbuf fails: vis_tol = 0 with the map at the depth itself, and
    vis_tol = 0.5 with depth 3 over a map of 2."""
    w, h = 32, 24
    v = np.array([[-1.0, -1.0, 0.0], [1.0, -1.0, 0.0], [-1.0, 1.0, 0.0]], F)
    f = np.array([[0, 2, 1]], np.int32)
    for tol, tz, zmap in ((0.0, 4.0, 4.0), (0.5, 3.0, 2.0), (0.0, 3.0, 3.0)):
        P = pinhole(w, h, fl=8.0, tz=tz)[None]
        z = np.full((1, h, w), zmap, F)
        assert nt.samples_at_the_bound(v, f, P, z, tol) == 4         # the three corners and the centroid: the bound is hit
        fv, fs = fz.raw_views(v, f, P, z, tol)
        assert fv.tolist() == [0] and not fz.compare_views((fv, fs), nt.face_views(v, f, P, z, tol), 1)
        below = np.nextafter(z, F(0.0))
        for hide in range(4):                                        # one ulp less under any one of the four samples hides the face
            sx, sy, _, _ = nt.project(P[0], np.vstack([v, ((v[0] + v[2]) + v[1])[None] / F(3.0)]))
            zz = z.copy()
            zz[0, int(np.rint(sy[hide])), int(np.rint(sx[hide]))] = below[0, 0, 0]
            got = fz.raw_views(v, f, P, zz, tol)
            assert got[0].tolist() == [-1] and not fz.compare_views(got, nt.face_views(v, f, P, zz, tol), 1)


@pytest.mark.gpu
def test_ties_between_identical_views_take_the_lower_index(hip):
    v, c, f = real_mesh("sphere")
    rng = np.random.default_rng(3)
    P = fz.rows_of(fz.arc_views(rng, 2, 96, 72))
    P = np.stack([P[0], P[0], P[1], P[1], P[0]])
    wz, wv, ws, wa = chain(v, c, f, P, random_frames(rng, 5, 72, 96), 0.02, 1)
    assert set(np.unique(wv).tolist()) == {-1, 0, 2} and (wv == 0).sum() > 100 and (wv == 2).sum() > 100
    assert np.array_equal(bits(wz[0]), bits(wz[1])) and np.array_equal(bits(wz[0]), bits(wz[4]))


@pytest.mark.gpu
def test_device_counts_and_the_rows_past_them(hip):
    v, c, f = real_mesh("scene")
    nv, nk = len(v), len(f)
    rng = np.random.default_rng(4)
    P = fz.rows_of(fz.arc_views(rng, 3, 80, 60))
    frames = random_frames(rng, 3, 60, 80)
    for counts in [(nv - 300, nk - 1000), (nv, nk), (0, 0), (0, nk), (nv, 0), (-1, nk - 5), (nv - 5, -2 ** 31), (nv + 1, nk + 1),
                   (INT32_MAX, INT32_MAX), (257, 256)]:
        chain(v, c, f, P, frames, 0.02, 1, counts=counts)           # the sentinel at and past the counted rows is part of it
    # fed from clean_mesh's counts on the device (the largest of the two components): nothing reads a count on the host in between
    import np_mesh_clean as npc
    from sfm_mvs_amd import mesh
    kv, kc, kf, kcounts = npc.clean(v, c, f, 8, True)
    assert 0 < len(kf) < nk
    dv, dc, df = up(v), up(c), up(f)
    dP, dfr = up(P), up(frames)
    ov, oc, of, counts = mesh.clean_mesh(dv, dc, df, 8, True)
    z = mesh.render_depth(ov, of, dP, 80, 60, counts=counts)        # warm
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ov, oc, of, counts = mesh.clean_mesh(dv, dc, df, 8, True)
        z = mesh.render_depth(ov, of, dP, 80, 60, counts=counts)
        fv, fs = mesh.face_views(ov, of, dP, z, counts=counts)
        atlas = mesh.texture_fill(ov, oc, of, dP, dfr, fv, 2, counts=counts)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    wz = nt.render_depth(kv, kf, P, 80, 60)
    wv, ws = nt.face_views(kv, kf, P, wz, mesh.VIS_TOL)
    assert np.array_equal(bits(z), bits(wz)) and np.array_equal(fv.cpu().numpy()[:len(kf)], wv) and np.array_equal(bits(fs)[:len(kf)], bits(ws))
    full = np.full(nk, -1, np.int32)
    full[:len(kf)] = wv
    pad_v, pad_f = np.vstack([kv, v[len(kv):]]), np.vstack([kf, f[len(kf):]])
    assert np.array_equal(atlas.cpu().numpy(), nt.texture_fill(pad_v, np.vstack([kc, c[len(kc):]]), pad_f, P, frames, full, 2, counts=kcounts[:2]))


@pytest.mark.gpu
def test_frames_of_two_by_two(hip):
    rng = np.random.default_rng(6)
    v = (rng.uniform(-1.2, 1.2, (300, 3)) * [1.0, 1.0, 0.3]).astype(F)
    f = fz.walk_soup(rng, 300, 500, 100)
    P = np.stack([pinhole(2, 2, fl=2.0, tz=4.0), pinhole(2, 2, tx=0.1, fl=3.0, tz=4.0)])     # the mesh spans about -0.1 .. 1.1 pixels
    frames = random_frames(rng, 2, 2, 2)
    wz, wv, ws, wa = chain(v, None, f, P, frames, 0.5, 3)
    assert np.isfinite(wz).sum() >= 4 and (wv >= 0).sum() > 5 and wa.max() > 0


@pytest.mark.gpu
def test_fill_with_and_without_colours_and_with_no_view_at_all(hip):
    v, c, f = real_mesh("sphere")
    f = f[:2001]                                                     # an odd count: the last cell's second half belongs to no face
    rng = np.random.default_rng(7)
    P = fz.rows_of(fz.arc_views(rng, 3, 96, 72))
    frames = random_frames(rng, 3, 72, 96)
    none = np.full(len(f), -1, np.int32)
    side, cols, cell = nt.layout(len(f), 4)
    for colours in (None, c):
        for fv in (none, rng.integers(-1, 3, len(f)).astype(np.int32), rng.integers(-3, 6, len(f)).astype(np.int32)):
            a = fz.raw_fill(v, colours, f, P, frames, fv, 4)
            assert np.array_equal(a, nt.texture_fill(v, colours, f, P, frames, fv, 4))
            face = nt.texel_faces(len(f), 4)[0]
            assert np.all(a[face >= len(f)] == 0) and (face == len(f)).sum() == cell * (cell - 1) // 2      # written, with 0
            if colours is None and fv is none:
                assert not a.any()
            if colours is not None and fv is none:
                assert a.any() and np.all(a[face >= len(f)] == 0)
    c2 = c.copy()
    c2[::7] = [np.nan, 300.0, -20.0]                                 # NaN -> 0, clamped above and below
    a = fz.raw_fill(v, c2, f, P, frames, none, 4)
    assert np.array_equal(a, nt.texture_fill(v, c2, f, P, frames, none, 4)) and a.max() == 255


@pytest.mark.gpu
def test_repeated_runs_give_equal_bytes(hip):
    v, c, f = real_mesh("scene")
    rng = np.random.default_rng(8)
    P = fz.rows_of(fz.arc_views(rng, 4, 160, 120))
    frames = random_frames(rng, 4, 120, 160)
    first = None
    for f_in in (f, f, f, f[::-1].copy(), f[rng.permutation(len(f))]):
        z = fz.raw_render(v, f_in, P, 160, 120)                     # the order of the faces cannot matter to the map
        if first is None:
            first = z
            views = fz.raw_views(v, f, P, z, 0.02)
            atlas = fz.raw_fill(v, c, f, P, frames, views[0], 8)
        assert np.array_equal(bits(z), bits(first))
        again = fz.raw_views(v, f, P, z, 0.02)
        assert np.array_equal(again[0], views[0]) and np.array_equal(again[1], views[1])
        assert np.array_equal(fz.raw_fill(v, c, f, P, frames, views[0], 8), atlas)


@pytest.mark.gpu
def test_every_argument_error_of_the_header(hip):
    from test_mesh_texture_cpu import check_argument_errors
    from sfm_mvs_amd import mesh
    check_argument_errors()
    v, c, f = (up(a) for a in real_mesh("sphere"))
    P = fz.rows_of(fz.arc_views(np.random.default_rng(0), 2, 32, 24))
    frames = up(random_frames(np.random.default_rng(0), 2, 24, 32))
    z = mesh.render_depth(v, f, P, 32, 24)
    fv, _ = mesh.face_views(v, f, P, z)
    for call in (lambda: mesh.render_depth(v, f, P, 1, 24), lambda: mesh.render_depth(v.cpu(), f, P, 32, 24),
                 lambda: mesh.render_depth(v, f, P[:0], 32, 24), lambda: mesh.render_depth(v, f, P, 32, 24, out=z[:1]),
                 lambda: mesh.face_views(v, f, P, z, vis_tol=-1.0), lambda: mesh.face_views(v, f, P, z, vis_tol=float("nan")),
                 lambda: mesh.face_views(v, f, P, z[:1]), lambda: mesh.face_views(v, f, P, z.double()),
                 lambda: mesh.texture_fill(v, c, f, P, frames, fv, 0), lambda: mesh.texture_fill(v, c, f, P, frames, fv, 65),
                 lambda: mesh.texture_fill(v, c[:-1], f, P, frames, fv), lambda: mesh.texture_fill(v, c, f, P, frames[:1], fv),
                 lambda: mesh.texture_fill(v, c, f, P, frames, fv[:-1]), lambda: mesh.texture_fill(v, c, f, P, frames, fv.float()),
                 lambda: mesh.texture_mesh(v, c, f, frames[:1], np.eye(3), P.reshape(-1, 3, 4))):
        with pytest.raises(mesh.SfmHipError):
            call()


def restated_texture(m, imgs, P, texels, vis_tol):
    v, c, f = m["vertices"].astype(F), m["colors"].astype(F), m["faces"]
    rows = fz.rows_of(P)
    h, w = imgs[0].shape[:2]
    z = nt.render_depth(v, f, rows, w, h)
    fv, _ = nt.face_views(v, f, rows, z, vis_tol)
    return nt.texture_fill(v, c, f, rows, np.stack(imgs), fv, texels), fv


@pytest.mark.gpu
def test_run_mesh_equals_the_restated_composition(hip):
    from test_gpu_mesh_finish import scene_run
    from sfm_mvs_amd import mesh
    imgs, K, P, gt, posearr, out = scene_run()[:6]
    for kw in (dict(), dict(decimate=2), dict(clean=True, smooth=3, normals=True, decimate=2)):
        plain = mesh.run_mesh(imgs, K, posearr, out, resolution=64, **kw)
        off = mesh.run_mesh(imgs, K, posearr, out, resolution=64, texture=False, texture_texels=3, texture_vis_tol=0.5, **kw)
        assert sorted(plain) == sorted(off) and all(np.array_equal(plain[k], off[k]) for k in plain)
        for texels, tol in ((mesh.ATLAS_TEXELS, mesh.VIS_TOL), (3, 0.0))[:1 if kw else 2]:
            m = mesh.run_mesh(imgs, K, posearr, out, resolution=64, texture=True, texture_texels=texels, texture_vis_tol=tol, **kw)
            assert sorted(m) == sorted(list(plain) + ["atlas", "uv", "face_view"]) and all(np.array_equal(plain[k], m[k]) for k in plain)
            wa, wv = restated_texture(plain, imgs, P, texels, tol)
            nf = len(plain["faces"])
            assert m["atlas"].dtype == np.uint8 and m["atlas"].shape == wa.shape and np.array_equal(m["atlas"], wa), kw
            assert m["face_view"].dtype == np.int32 and np.array_equal(m["face_view"], wv) and np.array_equal(m["uv"], nt.uv_of(nf, texels))
            if tol == mesh.VIS_TOL:
                print(f"run_mesh {kw}: {nf} faces, {int((wv >= 0).sum())} with a view, atlas side {wa.shape[0]}")
                assert (wv >= 0).mean() > 0.8
    for bad in (dict(texture_texels=0), dict(texture_texels=65), dict(texture_vis_tol=-0.1), dict(texture_vis_tol=float("nan"))):
        with pytest.raises(mesh.SfmHipError):
            mesh.run_mesh(imgs, K, posearr, out, resolution=64, texture=True, **bad)


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(), dict(decimate=2), dict(clean=True, smooth=3, normals=True, decimate=2)], ids=["plain", "decimate", "all"])
def test_run_mesh_with_a_texture_waits_for_the_host_exactly_once_more(hip, kw):
    import warnings
    from test_gpu_mesh_finish import scene_run
    from sfm_mvs_amd import _lib, mesh
    imgs, K, P, gt, posearr, out = scene_run()[:6]
    kw = dict(resolution=64, texture=True, **kw)
    mesh.run_mesh(imgs, K, posearr, out, **kw)                        # warm: the pinned host pool, the workspace
    torch.cuda.synchronize()
    lib0 = int(_lib.lib().sfm_host_sync_count())
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            m = mesh.run_mesh(imgs, K, posearr, out, **kw)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    syncs = [str(w.message) for w in caught if "synchroniz" in str(w.message).lower()]
    assert len(syncs) == 3, syncs                                     # the totals, the one download, the atlas
    assert int(_lib.lib().sfm_host_sync_count()) == lib0
    assert len(m["faces"]) > 0 and m["atlas"].any()


@pytest.mark.gpu
def test_a_short_fixed_seed_fuzz_run_finds_no_mismatch(hip):
    counts, bad, dt = fz.run(8.0, 4343)
    print(f"fuzz_mesh_texture: seed 4343, {sum(counts.values())} cases {counts}, {bad} mismatches, {dt:.0f} s")
    assert bad == 0 and all(c > 0 for c in counts.values()), counts


@pytest.mark.gpu
def test_committed_fuzz_logs_are_clean_and_name_this_code(hip):
    """profiles/mesh_texture_fuzz_seed*.log: no mismatch, and run on the code of csrc/mesh_texture.hip and csrc/common.h that the
    loaded library was built from (scripts/knn_code_hash.py: comments and whitespace do not count)."""
    import glob
    import re
    from sfm_mvs_amd import _lib
    have = _lib.code_hashes_of_binary()
    logs = sorted(glob.glob(os.path.join(ROOT, "profiles", "mesh_texture_fuzz_seed*.log")))
    assert len(logs) >= 2, logs
    total = 0
    for path in logs:
        text = open(path).read()
        m = re.search(r"fuzz_mesh_texture: seed \d+, (\d+) cases .*?, (\d+) mismatches", text)
        assert m and int(m.group(2)) == 0, f"{path}: no clean summary line"
        ids = re.findall(r"sfm_build_id (knn\.hip:\S+(?: \S+:\S+)*)", text)
        assert ids, f"{path} does not name the build it ran on"
        logged = dict(tok.split(":", 1) for tok in ids[-1].split() if ":" in tok)
        for name in ("mesh_texture.hip", "common.h"):
            assert logged.get(name) == have[name], f"{path} was produced by another csrc/{name} than the loaded binary's"
        total += int(m.group(1))
    assert total >= FUZZ_FLOOR, total
