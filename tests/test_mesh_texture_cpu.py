"""The mesh texturing step without a GPU (include/sfm_hip.h, "MESH-TEXTURE"; docs/mesh.md §10): the C-ABI declares, binds, documents
and validates the three entry points; the atlas layout and the OBJ / MTL / PNG writer are host code and are tested in full; the
restatement tests/np_mesh_texture.py stands apart from the product, gives hand-checked results on small meshes and, on np_mesh
surfaces of the rendered scenes, the figures scripts/calibrate_mesh_texture.py measured."""
import ast
import ctypes
import functools
import os
import struct
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

import np_mesh_texture as nt  # noqa: E402

NEW_SYMBOLS = ("sfm_mesh_render_depth", "sfm_mesh_face_views", "sfm_mesh_texture_fill")

# Calibration (docs/mesh.md §10; scripts/calibrate_mesh_texture.py, ground-truth depths, grid 64, seeds 0 and 1, view 2 held out):
# the atlas differs from the held-out view by 1.636 / 1.974 grey levels mean-abs, interpolated vertex colours by 5.248 / 6.093:
# ratios 0.312 / 0.324.  The bar is the issue's 0.5: the measured ratio leaves 1.54 x of head-room under it.
# Faces with a view: 98.22 / 97.47 % of all faces; the floor lies 2 points under the smaller share.
MAX_ERROR_RATIO = 0.5
MIN_TEXTURED_SHARE = 0.9547
MIN_FACING_SHARE = 0.95         # measured 96.7 .. 98.3 % of the in-frame (face, view) pairs


def f32(*rows):
    return np.array(rows, np.float32)


def pinhole(w, h, tx=0.0, fl=None, tz=0.0):
    """K [I | (tx, 0, tz)] as float32 [12]: the depth of a point is z + tz."""
    fl = 0.9 * w if fl is None else fl
    K = np.array([[fl, 0.0, (w - 1) / 2.0], [0.0, fl, (h - 1) / 2.0], [0.0, 0.0, 1.0]])
    return (K @ np.hstack([np.eye(3), [[tx], [0.0], [tz]]])).reshape(12).astype(np.float32)


def test_header_declares_binds_and_documents_the_texture_entry_points():
    from test_abi import declared_symbols
    from sfm_mvs_amd import _lib
    syms = declared_symbols()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    doc = open(os.path.join(ROOT, "docs", "mesh.md")).read()
    header = open(os.path.join(ROOT, "include", "sfm_hip.h")).read()
    assert "MESH-TEXTURE" in header and "NO NEAR-PLANE CLIPPING" in header
    for s in NEW_SYMBOLS:
        assert s in syms and s in _lib.SIGNATURES and hasattr(handle, s), s
        assert s in doc, f"docs/mesh.md does not mention {s}"
    assert _lib.lib().sfm_abi_version() == 3
    assert "mesh_texture.hip" in _lib.code_hashes_of_binary()


def check_argument_errors():
    """Every argument error of the header: SFM_ERR_ARG with its message, before any device call (the pointers are never read)."""
    from sfm_mvs_amd import _lib
    L = _lib.lib()
    fake = [ctypes.c_void_p(16 * (k + 1)) for k in range(10)]   # never dereferenced: every check below fails first
    big = 1 << 31
    nan, inf = float("nan"), float("inf")

    def render(verts=fake[0], faces=fake[1], nv=1000, nf=2000, counts=None, P=fake[2], n=3, w=64, h=48, zbuf=fake[3]):
        return L.sfm_mesh_render_depth(verts, faces, nv, nf, counts, P, n, w, h, zbuf, None)

    def views(verts=fake[0], faces=fake[1], nv=1000, nf=2000, counts=None, P=fake[2], n=3, w=64, h=48, zbuf=fake[3], tol=0.02, fv=fake[4],
              fs=fake[5]):
        return L.sfm_mesh_face_views(verts, faces, nv, nf, counts, P, n, w, h, zbuf, tol, fv, fs, None)

    def fill(verts=fake[0], colors=None, faces=fake[1], nv=1000, nf=2000, counts=None, P=fake[2], frames=fake[6], n=3, w=64, h=48, fv=fake[4],
             texels=8, cols=32, side=416, atlas=fake[7]):
        return L.sfm_mesh_texture_fill(verts, colors, faces, nv, nf, counts, P, frames, n, w, h, fv, texels, cols, side, atlas, None)

    assert nt.layout(2000, 8) == (416, 32, 13)
    common = [(dict(nv=-1), b"nv_cap"), (dict(nf=-2), b"nf_cap"), (dict(nv=big), b"nv_cap"), (dict(nf=big), b"nf_cap"),
              (dict(n=0), b"views"), (dict(n=-3), b"views"), (dict(n=65537), b"views"),
              (dict(w=1), b"frame"), (dict(h=1), b"frame"), (dict(w=0), b"frame"), (dict(h=-5), b"frame"), (dict(w=8193, h=8192), b"frame"),
              (dict(w=1 << 40, h=1 << 40), b"frame"), (dict(w=2, h=(1 << 25) + 1), b"frame"),
              (dict(verts=None), b"null"), (dict(faces=None), b"null"), (dict(P=None), b"null")]
    for call, extra in ((render, [(dict(zbuf=None), b"null")]),
                        (views, [(dict(zbuf=None), b"null"), (dict(fv=None), b"null"), (dict(fs=None), b"null"),
                                 (dict(tol=-0.01), b"vis_tol"), (dict(tol=nan), b"vis_tol"), (dict(tol=inf), b"vis_tol"), (dict(tol=-inf), b"vis_tol")]),
                        (fill, [(dict(frames=None), b"null"), (dict(atlas=None), b"null"), (dict(fv=None), b"null"),
                                (dict(texels=0), b"texels"), (dict(texels=65), b"texels"), (dict(texels=-1), b"texels"),
                                (dict(cols=31), b"layout"), (dict(cols=33), b"layout"), (dict(side=415), b"layout"), (dict(side=32 * 14), b"layout"),
                                (dict(texels=9, cols=32, side=416), b"layout"),
                                (dict(nf=2 * 238 * 238 + 1, texels=64, cols=239, side=239 * 69), b"exceeds"),
                                (dict(nf=big - 1, texels=1, cols=32768, side=6 * 32768), b"exceeds")])):
        for kw, msg in common + extra:
            assert call(**kw) == -1, (call.__name__, kw)
            assert msg in L.sfm_last_error(), (call.__name__, kw, L.sfm_last_error())


def test_argument_errors_are_reported_before_the_device():
    check_argument_errors()


def test_the_restatement_does_not_import_the_product():
    tree = ast.parse(open(os.path.join(ROOT, "tests", "np_mesh_texture.py")).read())
    for node in ast.walk(tree):
        names = [a.name for a in node.names] if isinstance(node, ast.Import) else [node.module or ""] if isinstance(node, ast.ImportFrom) else []
        assert not any(n.split(".")[0] in ("sfm_mvs_amd", "oracle") for n in names), names


@pytest.mark.parametrize("texels", [1, 2, 8, 64])
def test_atlas_layout(texels):
    from sfm_mvs_amd import mesh
    assert mesh.ATLAS_TEXELS == 8 and mesh.atlas_layout(2000)[:3] == (416, 32, 13)
    for nf in (0, 1, 2, 3, 4, 7, 8, 9, 18, 19, 199):
        side, cols, cell, uv = mesh.atlas_layout(nf, texels)
        assert (side, cols, cell) == nt.layout(nf, texels) and cell == texels + 5 and side == cols * cell
        assert cols >= 1 and cols * cols >= (nf + 1) // 2 and (cols == 1 or (cols - 1) ** 2 < (nf + 1) // 2)
        assert uv.shape == (nf, 3, 2) and uv.dtype == np.float64 and np.array_equal(uv, nt.uv_of(nf, texels))
        if nf:
            assert uv.min() > 0.0 and uv.max() < 1.0
        # the owner of every texel: the two halves of a cell are disjoint and cover it, a face owns texels of one cell only
        face, i, j, half, proper = nt.texel_faces(nf, texels)
        assert face.shape == (side, side) and np.array_equal(face & 1, half)
        for f in range(nf):
            own = face == f
            ys, xs = np.nonzero(own)
            q = f >> 1
            assert own.sum() == (cell * (cell + 1) // 2 if f % 2 == 0 else cell * (cell - 1) // 2)
            assert xs.min() >= (q % cols) * cell and xs.max() < (q % cols + 1) * cell and ys.min() >= (q // cols) * cell and ys.max() < (q // cols + 1) * cell
            # the corners are texels of the face
            px = uv[f, :, 0] * side - 0.5
            py = (1.0 - uv[f, :, 1]) * side - 0.5
            cx, cy = np.rint(px).astype(int), np.rint(py).astype(int)
            assert np.allclose(px, cx, atol=1e-9) and np.allclose(py, cy, atol=1e-9)
            assert abs(cx[1] - cx[0]) == texels and cy[1] == cy[0] and abs(cy[2] - cy[0]) == texels and cx[2] == cx[0]
            inside = proper & own
            assert inside.sum() == (texels + 1) * (texels + 2) // 2 and all(inside[y, x] for x, y in zip(cx, cy))
            ys, xs = np.nonzero(inside)
            for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1)):      # a texel of margin to the diagonal and to the cell's border
                assert np.all(own[ys + dy, xs + dx]), f"face {f}: a texel next to the chart belongs to another face"
            # a viewer's bilinear lookup anywhere in the closed chart reads four texels of the face
            n = 4 * texels
            a, b = np.meshgrid(np.arange(n + 1) / n, np.arange(n + 1) / n)
            keep = a + b <= 1.0
            x = cx[0] + a[keep] * (cx[1] - cx[0])
            y = cy[0] + b[keep] * (cy[2] - cy[0])
            x0, y0 = np.floor(x).astype(int), np.floor(y).astype(int)
            for dx in (0, 1):
                for dy in (0, 1):
                    assert np.all(own[y0 + dy, x0 + dx]), f"face {f}: a bilinear lookup in the chart reads another face's texel"
    for bad in (0, 65, -1):
        with pytest.raises(mesh.SfmHipError):
            mesh.atlas_layout(10, bad)
    with pytest.raises(mesh.SfmHipError):
        mesh.atlas_layout(2 * 238 * 238 + 1, 64)                     # 239 cells of 69 texels: 16 491 > 16 384
    assert mesh.atlas_layout(0, texels)[3].shape == (0, 3, 2)
    with pytest.raises(mesh.SfmHipError):
        mesh.atlas_layout(-1, texels)


def decode_png(data):
    """(h, w, 3) uint8 of an 8-bit truecolour, non-interlaced PNG whose rows all use filter 0; every chunk's CRC is checked."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xFFFFFFFF, tag
        chunks.append((tag, body))
        pos += 12 + n
    assert chunks[0][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    w, h, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, comp, filt, lace) == (8, 2, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(b"".join(b for t, b in chunks if t == b"IDAT")), np.uint8).reshape(h, 1 + 3 * w)
    assert np.all(raw[:, 0] == 0)
    return raw[:, 1:].reshape(h, w, 3)


def test_to_obj_mesh_round_trips(tmp_path):
    from sfm_mvs_amd import mesh
    from sfm_mvs_amd.pipeline import png_bytes, to_obj_mesh
    rng = np.random.default_rng(2)
    nv, nf, L = 40, 61, 3
    v = rng.normal(0, 1, (nv, 3))
    f = rng.integers(0, nv, (nf, 3)).astype(np.int32)
    side, cols, cell, uv = mesh.atlas_layout(nf, L)
    atlas = rng.integers(0, 256, (side, side, 3)).astype(np.uint8)
    os.makedirs(tmp_path / "Point_Cloud")
    for normals in (None, rng.normal(0, 1, (nv, 3))):
        assert to_obj_mesh(str(tmp_path), v, f, uv, atlas, normals) == (nv, nf)
        base = tmp_path / "Point_Cloud"
        png = open(base / "dense_mesh.png", "rb").read()
        assert np.array_equal(decode_png(png), atlas[..., ::-1])       # R G B from the B G R atlas, rows top to bottom
        try:
            from PIL import Image
        except ImportError:
            Image = None
        if Image is not None:
            assert np.array_equal(np.asarray(Image.open(base / "dense_mesh.png").convert("RGB")), atlas[..., ::-1])
        mtl = open(base / "dense_mesh.mtl").read()
        assert "newmtl dense_mesh" in mtl and "map_Kd dense_mesh.png" in mtl
        rows = [r.split() for r in open(base / "dense_mesh.obj").read().splitlines()]
        assert rows[0] == ["mtllib", "dense_mesh.mtl"] and ["usemtl", "dense_mesh"] in rows
        pv = np.array([r[1:] for r in rows if r[0] == "v"], np.float64)
        pt = np.array([r[1:] for r in rows if r[0] == "vt"], np.float64)
        pn = np.array([r[1:] for r in rows if r[0] == "vn"], np.float64)
        pf = [[tuple(int(x) for x in c.split("/")) for c in r[1:]] for r in rows if r[0] == "f"]
        assert np.allclose(pv, 200 * v, atol=1e-5) and np.allclose(pt, uv.reshape(-1, 2), atol=1e-8) and len(pf) == nf
        assert np.array_equal(np.array([[c[0] for c in face] for face in pf]) - 1, f)
        assert np.array_equal(np.array([[c[1] for c in face] for face in pf]) - 1, np.arange(3 * nf).reshape(nf, 3))
        if normals is None:
            assert len(pn) == 0 and all(len(c) == 2 for face in pf for c in face)
        else:
            assert np.allclose(pn, normals, atol=1e-5) and all(c[2] == c[0] for face in pf for c in face)
        # a viewer's lookup: the texel under the first corner's coordinates is the chart's corner texel
        x, y = pt[::3, 0] * side - 0.5, (1.0 - pt[::3, 1]) * side - 0.5
        face, i, j, half, proper = nt.texel_faces(nf, L)
        assert np.array_equal(face[np.rint(y).astype(int), np.rint(x).astype(int)], np.arange(nf))
    assert np.array_equal(decode_png(png_bytes(np.zeros((1, 1, 3), np.uint8))), np.zeros((1, 1, 3), np.uint8))
    with pytest.raises(ValueError):
        to_obj_mesh(str(tmp_path), v, f + nv, uv, atlas)
    with pytest.raises(ValueError):
        to_obj_mesh(str(tmp_path), v, f, uv[:-1], atlas)
    with pytest.raises(ValueError):
        to_obj_mesh(str(tmp_path), v, f, uv, atlas.astype(np.float32))


def test_run_mesh_defaults():
    import inspect
    from calibrate_mesh_texture import VIS_TOL
    from sfm_mvs_amd import mesh
    sig = inspect.signature(mesh.run_mesh).parameters
    assert sig["texture"].default is False and sig["texture_texels"].default == mesh.ATLAS_TEXELS == 8
    assert sig["texture_vis_tol"].default == mesh.VIS_TOL == VIS_TOL == 0.02


def test_one_fronto_parallel_triangle_by_hand():
    """A right triangle at depth 4 with its legs on pixel centres: the covered pixels are the closed triangle, each at depth 4 up
    to the rounding of the interpolation; the other orientation covers the same pixels; a second, nearer triangle wins its pixels."""
    w, h = 16, 12
    P = pinhole(w, h, fl=8.0, tz=4.0)[None]                          # sx = 2 x + 7.5, sy = 2 y + 5.5 at z = 0
    v = f32([-3.25, -2.25, 0.0], [0.75, -2.25, 0.0], [-3.25, 1.75, 0.0])        # screen (1, 1), (9, 1), (1, 9)
    sx, sy, sz, ok = nt.project(P[0], v)
    assert sx.tolist() == [1.0, 9.0, 1.0] and sy.tolist() == [1.0, 1.0, 9.0] and sz.tolist() == [4.0, 4.0, 4.0] and ok.all()
    want = np.array([[1 <= x and 1 <= y and (x - 1) + (y - 1) <= 8 and y < h for x in range(w)] for y in range(h)])
    for tri in ([0, 1, 2], [0, 2, 1]):
        z = nt.render_depth(v, np.array([tri], np.int32), P, w, h)[0]
        assert np.array_equal(np.isfinite(z), want) and np.all(np.abs(z[want] - 4.0) <= 4 * 2.0 ** -22)
    near = f32([-2.25, -1.75, -1.0], [-1.25, -1.75, -1.0], [-2.25, -0.75, -1.0])   # depth 3: fl / 3 = 8 / 3 px per unit
    z = nt.render_depth(np.vstack([v, near]), np.array([[0, 1, 2], [3, 4, 5]], np.int32), P, w, h)[0]
    assert np.isclose(z[want].min(), 3.0, atol=1e-5) and (np.abs(z - 3.0) < 1e-5).sum() >= 3 and np.array_equal(np.isfinite(z), want)
    # negative screen area = wound toward the camera: (0, 2, 1) is; only that orientation is a candidate
    zz = nt.render_depth(v, np.array([[0, 1, 2], [0, 2, 1]], np.int32), P, w, h)
    fv, fs = nt.face_views(v, np.array([[0, 1, 2], [0, 2, 1]], np.int32), P, zz, 0.0)
    assert fv.tolist() == [-1, 0] and fs.tolist() == [0.0, 64.0]


def wall_and_quad():
    """A wall at z = 2 (a 6 x 4 grid of quads, two faces each, wound toward the cameras at z = -4) and a quad at z = 0 in front of
    its middle; camera 0 stands far to the right, camera 1 straight in front."""
    xs, ys = np.linspace(-3.0, 3.0, 7), np.linspace(-2.0, 2.0, 5)
    v = [[x, y, 2.0] for y in ys for x in xs]
    f = []
    for j in range(4):
        for i in range(6):
            a, b, c, d = j * 7 + i, j * 7 + i + 1, (j + 1) * 7 + i, (j + 1) * 7 + i + 1
            f += [[a, c, b], [b, c, d]]
    k = len(v)
    v += [[-0.5, -0.6, 0.0], [0.5, -0.6, 0.0], [-0.5, 0.6, 0.0], [0.5, 0.6, 0.0]]
    f += [[k, k + 2, k + 1], [k + 1, k + 2, k + 3]]
    return np.array(v, np.float32), np.array(f, np.int32)


def test_an_occluder_changes_the_view():
    """Wall faces behind the quad as camera 1 sees it: camera 1 scores higher on them (it looks at the wall head on) but does not
    see them; camera 0, from the side, sees past the quad."""
    from mvs_scenes import look_at
    w, h = 160, 120
    K = np.array([[100.0, 0.0, 79.5], [0.0, 100.0, 59.5], [0.0, 0.0, 1.0]])
    Ps = []
    for C in ([3.5, 0.0, -4.0], [0.0, 0.0, -4.0]):
        R, t = look_at(np.array(C), np.array([0.0, 0.0, 2.0]))
        Ps.append(K @ np.hstack([R, t[:, None]]))
    P = np.asarray(Ps).reshape(2, 12).astype(np.float32)
    v, f = wall_and_quad()
    z = nt.render_depth(v, f, P, w, h)
    fv, fs = nt.face_views(v, f, P, z, 0.02)
    blind, _ = nt.face_views(v, f, P, np.full_like(z, np.inf), 0.02)          # no occlusion test: the largest area alone
    assert np.all(fv >= 0) and np.all(blind[-2:] == fv[-2:])                    # everything is seen by someone; the quad itself by its best
    changed = np.flatnonzero(fv != blind)
    assert len(changed) >= 2 and np.all(blind[changed] == 1) and np.all(fv[changed] == 0)
    # the changed faces are wall faces whose centroid lies behind the quad as seen from camera 1 (|x| < 0.75, |y| < 0.9 at z = 2)
    g = v[f[changed]].mean(axis=1)
    assert np.all(changed < len(f) - 2) and np.all(np.abs(g[:, 0]) < 1.0) and np.all(np.abs(g[:, 1]) < 1.2)
    # and camera 1 does score higher on them
    for k, s, facing, vis, score, _ in nt.view_tests(v, f, P, z, 0.02):
        if k == 0:
            s0 = score[changed]
            assert np.all(facing[changed] & vis[changed])
        else:
            assert np.all(score[changed] > s0) and np.all(facing[changed]) and not np.any(vis[changed])


def sphere_mesh():
    import np_mesh
    from test_gpu_mesh import sphere_field
    S = sphere_field((23, 19, 17), (10.3, 9.1, 8.2), 6.4)
    v, _, f = np_mesh.extract_mesh(2.0 * S, np.full_like(S, 2.0), None, (0.0, 0.0, 0.0), 1.0, 1.0)
    return v, f, np.array([10.3, 9.1, 8.2])


def test_the_facing_rule_on_a_sphere():
    """Outside cameras: a face whose outward normal points at the camera has a negative screen area and the others a positive one,
    so of the pairs the depth map shows, all but the grazing ones are negative."""
    from mvs_scenes import look_at
    v, f, centre = sphere_mesh()
    w, h = 160, 120
    K = np.array([[144.0, 0.0, 79.5], [0.0, 144.0, 59.5], [0.0, 0.0, 1.0]])
    cams = [centre + 40.0 * np.array(d) / np.linalg.norm(d) for d in ([0.0, 0.0, -1.0], [1.0, 0.2, -1.0], [-1.0, -0.3, 0.5], [0.1, 1.0, 0.2])]
    Ps = []
    for C in cams:
        R, t = look_at(C, centre)
        Ps.append(K @ np.hstack([R, t[:, None]]))
    P = np.asarray(Ps).reshape(-1, 12).astype(np.float32)
    z = nt.render_depth(v, f, P, w, h)
    g = v[f].astype(np.float64).mean(axis=1)
    nrm = np.cross(v[f[:, 1]].astype(np.float64) - v[f[:, 0]], v[f[:, 2]].astype(np.float64) - v[f[:, 0]])
    agree = total = seen = seen_neg = 0
    for k, s, facing, vis, score, _ in nt.view_tests(v, f, P, z, 0.02):
        assert len(s) == len(f)
        toward = np.einsum("ij,ij->i", nrm, cams[k] - g) > 0
        sx, sy, _, ok = nt.project(P[k], v)
        a, b, c = f[:, 0], f[:, 1], f[:, 2]
        area2 = (sx[b] - sx[a]) * (sy[c] - sy[a]) - (sy[b] - sy[a]) * (sx[c] - sx[a])
        assert ok.all() and sx.min() >= 0 and sx.max() <= w - 1 and sy.min() >= 0 and sy.max() <= h - 1      # every pair is in the frame
        agree += int(((area2 < 0) == toward).sum())
        total += len(f)
        seen += int(vis.sum())
        seen_neg += int((vis & (area2 < 0)).sum())
        assert np.array_equal(facing, area2 < 0)
    print(f"sphere: sign agrees with the normal on {agree} of {total} pairs; {seen_neg} of {seen} visible pairs are negative")
    assert agree >= 0.999 * total
    assert seen > 0.3 * total and seen_neg >= MIN_FACING_SHARE * seen


@functools.lru_cache(maxsize=None)
def scene_model(seed):
    from calibrate_mesh_texture import model
    return model(seed, 64)


@pytest.mark.parametrize("seed", [0, 1])
def test_calibration_on_the_rendered_scenes(seed):
    """Ground-truth depths at grid 64: the facing rule holds for at least 95 % of the in-frame pairs; with view 2 held out, the atlas
    is closer to that view than interpolated vertex colours are, by the factor the issue asks for, and nearly every face finds a view."""
    from calibrate_mesh_texture import facing_share, held_out
    from sfm_mvs_amd import mesh
    m = scene_model(seed)
    assert len(m["f"]) > 10000
    share = facing_share(m)
    ea, ev, texels, textured = held_out(m, mesh.VIS_TOL, mesh.ATLAS_TEXELS)
    print(f"seed {seed}: {len(m['f'])} faces, facing share {share:.4f}, held-out error atlas {ea:.3f} vertex colours {ev:.3f} "
          f"ratio {ea / ev:.3f} over {texels} texels, faces with a view {textured:.4f}")
    assert share >= MIN_FACING_SHARE
    assert texels > 100000 and ea < ev and ea <= MAX_ERROR_RATIO * ev, (ea, ev)
    assert textured >= MIN_TEXTURED_SHARE, textured
