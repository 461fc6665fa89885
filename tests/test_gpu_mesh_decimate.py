"""The mesh decimation step on the device (sfm_mesh_decimate, mesh.decimate_mesh, run_mesh(decimate=...)): every output equal to
the restatement tests/np_mesh_decimate.py, float rows as int32 views; there is no tolerance anywhere (include/sfm_hip.h,
"MESH-DECIMATE"; docs/mesh.md §9)."""
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
import np_mesh_clean as npc  # noqa: E402
import np_mesh_decimate as nd  # noqa: E402
import np_mesh_finish as nf  # noqa: E402
import fuzz_mesh_decimate as fz  # noqa: E402
from fuzz_mesh_clean import SENTINEL, bits, same, up  # noqa: E402
from fuzz_mesh_finish import local_soup  # noqa: E402

INT32_MAX = 2 ** 31 - 1
FUZZ_FLOOR = 3000               # cases the committed logs hold together, at least


def check(v, c, f, origin, cell, dims, pscale, dedupe, counts=None):
    """sfm_mesh_decimate (into sentinel-filled buffers) over one mesh against the restatement -> the restatement's result."""
    want = nd.decimate(v, c, f, origin, cell, dims, pscale, dedupe, counts)
    bad = fz.compare(fz.raw_decimate(v, c, f, origin, cell, dims, pscale, dedupe, counts), want)
    assert not bad, (bad, dims, dedupe, counts)
    return want


@functools.lru_cache(maxsize=None)
def real_meshes():
    """name -> (vertices, colours, faces, origin float64, voxel, dims) of the restated extraction of test_gpu_mesh.py's sphere and
    scene fields."""
    from test_gpu_mesh import fields
    out = {}
    for name, S, W, C, origin, voxel in fields():
        if name == "random":
            continue
        org = np.asarray(origin, np.float64)
        wv, wc, wf = np_mesh.extract_mesh(S, W, C, org.astype(np.float32), np.float32(voxel), 1.0)
        if wc is None:
            wc = (np.random.default_rng(11).random((len(wv), 3)) * 255.0).astype(np.float32)
        out[name] = (wv, wc, wf, org, float(voxel), S.shape[::-1])
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sphere", "scene"])
def test_real_meshes_equal_the_restatement(hip, name):
    from sfm_mvs_amd import mesh
    wv, wc, wf, origin, voxel, dims = real_meshes()[name]
    assert len(wf) > 100
    for cells in (1.0, 2.0, 3.5):
        fo, cell, fdims, fext = nd.frame_of(origin, voxel, dims, cells)
        pscale = nf.pscale_of(fext)
        for dedupe in (0, 1):
            for c in (None, wc):
                xv, xc, xf, xn = check(wv, c, wf, fo, cell, fdims, pscale, dedupe)
                assert xn[2] == 0 and 0 < xn[1] <= len(wf) and 0 < xn[0] < len(wv)
        # the Python operator over run_mesh's frame
        go, gcell, gdims, gext = mesh.decimate_frame(origin, voxel, dims, cells)
        dv, dc, df, dn = mesh.decimate_mesh(up(wv), up(wc), up(wf), go, gcell, gdims, gext)
        k, m = int(xn[0]), int(xn[1])
        assert dn.cpu().numpy().tolist() == xn.tolist() and same(dv[:k], xv) and same(dc[:k], xc) and same(df[:m], xf), cells
    assert xn[1] < len(wf) / 4                                        # 3.5-voxel cells


SIZES = [0, 1, 2, 3, 255, 256, 257, 65537]
SOUP_DIMS = [(1, 1, 1), (3, 5, 7), (7, 5, 3), (64, 64, 64)]


@pytest.mark.gpu
@pytest.mark.parametrize("nv", SIZES)
def test_random_face_soups_at_the_block_edges(hip, nv):
    """nv and nf independently at 0..3, around one 256-block and past 2^16; one cell (no face is live), asymmetric grids (an axis
    swap in the key changes the result) and a grid with more cells than vertices; a quarter of the indices name no vertex, a
    tenth of the faces repeat an index or another face."""
    case = 0
    for nk in SIZES:
        for dims in SOUP_DIMS:
            rng = np.random.default_rng(1000003 * nv + 101 * nk + dims[0])
            v = rng.uniform(-1.0, 3.0, (nv, 3)).astype(np.float32)
            c = (rng.random((nv, 3)) * 255.0).astype(np.float32) if case % 3 else None
            f = local_soup(rng, nv, nk, 4 if (nv + nk) % 2 else max(nv, 1))
            hit = rng.random((nk, 3)) < 0.25
            f[hit] = rng.choice(np.array([-1, nv, INT32_MAX], np.int64), int(hit.sum())).astype(np.int32)
            if nk > 3:
                k = rng.random(nk) < 0.1
                f[k, 1] = f[k, 0]
                f[rng.random(nk) < 0.1] = f[1]
            cell = np.float32(4.0 / max(dims))
            want = check(v, c, f, (-1.0, -1.0, -1.0), cell, dims, nf.pscale_of(4.0), case % 2)
            if dims == (1, 1, 1):
                assert want[3][1] == 0 and want[3][0] == min(nv, 1)
            case += 1


@pytest.mark.gpu
def test_dedupe_of_repeats_rotations_and_flips(hip):
    # one face 1 000 times, with its rotations and its flip, among other faces
    rng = np.random.default_rng(17)
    nv = 64
    v = rng.uniform(0.0, 4.0, (nv, 3)).astype(np.float32)
    fr = dict(origin=(0.0, 0.0, 0.0), cell=np.float32(1.0), dims=(4, 4, 4), pscale=nf.pscale_of(4.0))
    newid = nd.cluster(v, None, fr["origin"], fr["cell"], fr["dims"], fr["pscale"], nv)[0]
    a, b, c = [int(np.flatnonzero(newid == k)[0]) for k in (0, 1, 2)]
    reps = np.array([[a, b, c], [b, c, a], [c, a, b], [a, c, b]], np.int32)[rng.integers(0, 4, 1000)]
    f = np.vstack([local_soup(rng, nv, 300, nv), reps, local_soup(rng, nv, 300, nv)]).astype(np.int32)
    xv, _, xf, xn = check(v, None, f, dedupe=1, **fr)
    assert xn[3] >= 998
    both = check(v, None, reps, dedupe=1, **fr)
    assert both[3].tolist()[1:] == [2, 0, 998] and sorted(nd.normalise(both[2].astype(np.int64)).tolist()) == [[0, 1, 2], [0, 2, 1]]
    assert check(v, None, reps, dedupe=0, **fr)[3].tolist()[1:] == [1000, 0, 0]


@pytest.mark.gpu
def test_dedupe_of_65537_distinct_faces_each_met_again_in_reverse_order(hip):
    """One vertex per cell, 65 537 distinct live faces, then the same faces rotated, in reverse input order: the set holds 65 537
    classes in 2^18 slots (collisions and probing), and the lower index of every pair wins."""
    n = 65537
    nv = n + 2
    ids = np.arange(nv)
    v = (np.stack([ids % 64, ids // 64 % 64, ids // 4096], 1) + 0.5).astype(np.float32)
    perm = np.random.default_rng(23).permutation(nv)
    v = v[perm]                                                                   # vertex ids and cells in unrelated orders
    first = np.stack([np.arange(n), np.arange(n) + 1, np.arange(n) + 2], 1).astype(np.int32)
    again = first[::-1][:, [1, 2, 0]]
    f = np.ascontiguousarray(np.vstack([first, again]), np.int32)
    fr = dict(origin=(0.0, 0.0, 0.0), cell=np.float32(1.0), dims=(64, 64, 64), pscale=nf.pscale_of(64.0))
    xv, _, xf, xn = check(v, None, f, dedupe=1, **fr)
    assert xn.tolist() == [nv, n, 0, n] and np.array_equal(xf, first)            # one vertex per cell: the ids are kept
    xv, _, xf, xn = check(v, None, f[::-1].copy(), dedupe=1, **fr)
    assert xn.tolist() == [nv, n, 0, n] and np.array_equal(xf, again[::-1])
    assert check(v, None, f, dedupe=0, **fr)[3].tolist() == [nv, 2 * n, 0, 0]


@pytest.mark.gpu
def test_frame_corners_of_the_largest_grid(hip):
    """512^3 cells: a vertex in each corner cell (the largest key is 2^27 - 1) and one just outside each face of the frame."""
    d, cell = 512, np.float32(1.0)
    lo, hi = np.float32(0.25), np.float32(d - 0.25)
    corners = np.array([[x, y, z] for z in (lo, hi) for y in (lo, hi) for x in (lo, hi)], np.float32)
    outside = np.full((6, 3), 100.5, np.float32)
    for k in range(3):
        outside[2 * k, k] = np.nextafter(np.float32(0.0), np.float32(-1.0))
        outside[2 * k + 1, k] = np.float32(d)
    v = np.vstack([corners, outside, corners + np.float32(0.125)]).astype(np.float32)
    key, _ = nd.cells(v, (0.0, 0.0, 0.0), cell, (d, d, d), nf.pscale_of(float(d)))
    assert key[:8].max() == 2 ** 27 - 1 and key[:8].min() == 0 and np.all(key[8:14] == -1) and np.array_equal(key[14:], key[:8])
    f = np.array([[0, 1, 2], [1, 3, 7], [4, 5, 6], [0, 8, 1], [9, 2, 3], [14, 15, 16], [0, 14, 1], [7, 21, 6], [3, 7, 1]], np.int32)
    want = check(v, None, f, (0.0, 0.0, 0.0), cell, (d, d, d), nf.pscale_of(float(d)), 1)
    assert want[3].tolist() == [8, 3, 6, 2]


@pytest.mark.gpu
def test_boundary_and_extreme_coordinates(hip):
    rng = np.random.default_rng(29)
    nv, nk = 3000, 9000
    dims, cell = (6, 9, 5), np.float32(0.25)
    o = np.array([-0.75, 2.0, 0.5], np.float32)
    span = np.array(dims) * float(cell)
    pscale = nf.pscale_of(float(span.max()))
    inside = (o.astype(np.float64) + rng.random((nv, 3)) * span).astype(np.float32)
    col = (rng.random((nv, 3)) * 255.0).astype(np.float32)
    f = local_soup(rng, nv, nk, 40)
    # coordinates exactly o + k * cell, k in -1..dims+1 (o itself and o + dims * cell among them), and o - 2^-20
    k = rng.integers(-1, np.array(dims) + 2, (nv, 3))
    v = np.where(rng.random((nv, 3)) < 0.5, (o.astype(np.float64) + k * float(cell)).astype(np.float32), inside)
    low = rng.random((nv, 3)) < 0.03
    v[low] = (np.broadcast_to(o, (nv, 3))[low] - np.float32(2.0 ** -20)).astype(np.float32)
    v[:3] = [o, o + np.float32(span), o - np.float32(2.0 ** -20)]
    key, _ = nd.cells(v, o, cell, dims, pscale)
    assert key[:3].tolist() == [0, -1, -1] and 0 < (key < 0).sum() < nv
    for dedupe in (0, 1):
        check(v, col, f, o, cell, dims, pscale, dedupe)
    # NaN, +-inf and 1e30 positions; NaN, inf and 1e6 colours (and the two sides of 32768)
    v = inside.copy()
    hit = rng.random((nv, 3)) < 0.1
    v[hit] = rng.choice(np.array([np.nan, np.inf, -np.inf, 1e30, -1e30], np.float32), int(hit.sum()))
    c = col.copy()
    hit = rng.random((nv, 3)) < 0.2
    c[hit] = rng.choice(np.array([np.nan, np.inf, -np.inf, 1e6, -1e6, 32768.0, -32768.0, 32768.004, -0.0], np.float32), int(hit.sum()))
    want = check(v, c, f, o, cell, dims, pscale, 1)
    assert np.isfinite(want[0]).all() and np.isfinite(want[1]).all() and 0 < want[3][2] < nv
    # usable by cell but beyond 2^30 quanta: a deliberately large pscale
    want = check(inside, col, f, o, cell, dims, pscale * 4.0, 1)
    assert 0 < want[3][2] < nv
    assert check(inside, None, f, o, cell, dims, pscale * 2.0 ** 12, 0)[3][2] >= nv - 5      # all but the rows within 2^-9 of o


@pytest.mark.gpu
def test_the_hot_cell_and_sums_past_2_to_the_53(hip):
    # 70 001 vertices in one cell of many, the rest spread out
    rng = np.random.default_rng(31)
    nv, nk = 75001, 20000
    dims, cell = (16, 16, 16), np.float32(0.125)
    v = (rng.random((nv, 3)) * 2.0).astype(np.float32)
    hot = rng.permutation(nv)[:70001]
    v[hot] = (np.array([1.0, 0.5, 1.25]) + rng.random((70001, 3)) * 0.124).astype(np.float32)
    c = (rng.random((nv, 3)) * 255.0).astype(np.float32)
    f = local_soup(rng, nv, nk, nv)
    want = check(v, c, f, (0.0, 0.0, 0.0), cell, dims, nf.pscale_of(2.0), 1)
    assert want[3][0] > 1000
    # 2^23 + 3 vertices in one cell: the x sum passes 2^53 and is odd, so no float64 holds it; the expected words from Python integers
    reps = 2 ** 23 + 3
    origin, pscale, big = np.array([0.0, -1.0, -1.0], np.float32), 2.0 ** 28, np.float32(8.0)
    two = np.array([[4.0, 0.5, 1.5], [2.0 ** -8 + 2.0 ** -28, 0.25, 1.0]], np.float32)      # x quanta: 2^30 (the bound) and 2^20 + 1
    key, r = nd.cells(two, origin, big, (1, 1, 1), pscale)
    assert key.tolist() == [0, 0] and r[:, 0].tolist() == [2 ** 30, 2 ** 20 + 1]
    r = [[int(x) for x in row] for row in r]
    v = np.tile(two[:1], (reps, 1))
    v[12345] = two[1]
    acc = [(reps - 1) * a + b for a, b in zip(r[0], r[1])]
    assert acc[0] > 2 ** 53 and acc[0] % 2 == 1 and int(float(acc[0])) != acc[0]
    want_v = np.array([[np.float32((float(a) / float(reps)) / float(pscale) + float(o)) for a, o in zip(acc, origin)]], np.float32)
    col = np.tile(np.array([[32767.99, 200.5, 0.25]], np.float32), (reps, 1))
    col[777] = [1.0 + 2.0 ** -16, 3.0, 7.0]
    q = [[int(x) for x in row] for row in nd.colour_terms(col[[0, 777]])]
    cacc = [(reps - 1) * a + b for a, b in zip(q[0], q[1])]
    assert cacc[0] > 2 ** 53 and cacc[0] % 2 == 1
    want_c = np.array([[np.float32((float(a) / float(reps)) / 65536.0) for a in cacc]], np.float32)
    f = np.array([[0, 1, 2]], np.int32)
    ov, oc, of, on = fz.raw_decimate(v, col, f, origin, big, (1, 1, 1), pscale, 1)
    assert on.tolist() == [1, 0, 0, 0]
    assert np.array_equal(ov[:1], bits(want_v)) and np.array_equal(oc[:1], bits(want_c)), (ov[:1], bits(want_v), oc[:1], bits(want_c))
    assert np.all(ov[1:] == SENTINEL) and np.all(oc[1:] == SENTINEL) and np.all(of == SENTINEL)


@pytest.mark.gpu
def test_device_counts(hip):
    from sfm_mvs_amd import mesh
    wv, wc, wf, origin, voxel, dims = real_meshes()["scene"]
    nv, nk = len(wv), len(wf)
    fo, cell, fdims, fext = nd.frame_of(origin, voxel, dims, 2.0)
    pscale = nf.pscale_of(fext)
    for counts in [(nv - 300, nk - 1000), (nv, nk), (0, 0), (0, nk), (nv, 0), (-1, nk - 5), (nv - 5, -2 ** 31), (nv + 1, nk + 1),
                   (INT32_MAX, INT32_MAX), (257, 256)]:
        check(wv, wc, wf, fo, cell, fdims, pscale, 1, counts=counts)     # the sentinel at and past the counted rows is part of it
    # fed straight from clean_mesh's counts and feeding mesh_normals: nothing reads a count on the host in between
    v, c, f = up(wv), up(wc), up(wf)
    threshold = 8
    kv, kc, kf, kcounts = npc.clean(wv, wc, wf, threshold)
    assert 0 < len(kv) < nv and 0 < len(kf) < nk
    go, gcell, gdims, gext = mesh.decimate_frame(origin, voxel, dims, 2.0)
    nr = torch.full((nv, 3), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
    ov, oc, of, counts, status, labels, buf = mesh.clean_mesh(v, c, f, threshold, packed=True)     # warm: the workspaces
    mesh.decimate_mesh(ov, oc, of, go, gcell, gdims, gext, counts=counts)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ov, oc, of, counts, status, labels, buf = mesh.clean_mesh(v, c, f, threshold, packed=True)
        dv, dc, df, dn, dbuf = mesh.decimate_mesh(ov, oc, of, go, gcell, gdims, gext, counts=counts, packed=True)
        mesh.mesh_normals(dv, df, counts=dn, out=nr)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert counts.cpu().numpy().tolist() == kcounts.tolist() and int(status[0]) == 1
    yv, yc, yf, yn = nd.decimate(kv, kc, kf, fo, cell, fdims, pscale, True)
    k, m = int(yn[0]), int(yn[1])
    assert dn.cpu().numpy().tolist() == yn.tolist() and 0 < m < len(kf)
    assert same(dv[:k], yv) and same(dc[:k], yc) and same(df[:m], yf)
    host = dbuf.cpu().numpy()                                            # the packed buffer: counts, vertices, colours, faces
    assert host[:4].tolist() == yn.tolist() and np.array_equal(host[4:4 + 3 * k], bits(yv).reshape(-1))
    assert np.array_equal(host[4 + 3 * nv:4 + 3 * nv + 3 * k], bits(yc).reshape(-1)) and np.array_equal(host[4 + 6 * nv:4 + 6 * nv + 3 * m], yf.reshape(-1))
    got_n = bits(nr)
    assert np.array_equal(got_n[:k], bits(nf.normals(yv, yf))) and np.all(got_n[k:] == SENTINEL)


@pytest.mark.gpu
def test_face_order_and_repeated_runs(hip):
    wv, wc, wf, origin, voxel, dims = real_meshes()["scene"]
    fo, cell, fdims, fext = nd.frame_of(origin, voxel, dims, 2.0)
    pscale = nf.pscale_of(fext)
    rng = np.random.default_rng(5)
    twin = fz.twins(rng, wf, 0.3)                                        # duplicates to drop: the survivor depends on the input order
    first = fz.raw_decimate(wv, wc, twin, fo, cell, fdims, pscale, 1)
    assert first[3][3] > 0
    for _ in range(3):
        again = fz.raw_decimate(wv, wc, twin, fo, cell, fdims, pscale, 1)
        assert all(np.array_equal(a, b) for a, b in zip(first, again))
    for f in (twin[rng.permutation(len(twin))], twin[::-1].copy()):
        want = check(wv, wc, f, fo, cell, fdims, pscale, 1)
        assert np.array_equal(bits(want[0]), first[0][:len(want[0])]) and want[3].tolist() == first[3].tolist()      # the vertices do not move


@pytest.mark.gpu
def test_every_argument_error_of_the_header(hip):
    from test_mesh_decimate_cpu import check_argument_errors
    from sfm_mvs_amd import mesh
    check_argument_errors()
    wv, wc, wf, origin, voxel, dims = real_meshes()["sphere"]
    v, c, f = up(wv), up(wc), up(wf)
    with pytest.raises(mesh.SfmHipError):
        mesh.decimate_mesh(v, c, f, origin, voxel, (1024, 1024, 1024), 1.0)
    with pytest.raises(mesh.SfmHipError):
        mesh.decimate_mesh(v, c, f, origin, voxel, (4, 0, 4), 1.0)
    with pytest.raises(mesh.SfmHipError):
        mesh.decimate_mesh(v, c[:-1], f, origin, voxel, (4, 4, 4), 1.0)
    with pytest.raises(mesh.SfmHipError):
        mesh.decimate_mesh(v, c, f, origin, 0.0, (4, 4, 4), 1.0)
    with pytest.raises(mesh.SfmHipError):
        mesh.decimate_mesh(v.cpu(), c, f, origin, voxel, (4, 4, 4), 1.0)


def restated_tail(bv, bc, bf, origin, voxel, dims, smooth, cells, dedupe=True):
    """(vertices, colours, faces, normals, counts) of run_mesh's steps after the clean-up, restated."""
    extent = voxel * (max(dims) - 1)
    sv = nf.smooth(bv, bf, nf.taubin_factors(smooth), origin.astype(np.float32), nf.pscale_of(extent))
    fo, cell, fdims, fext = nd.frame_of(origin, voxel, dims, cells)
    xv, xc, xf, xn = nd.decimate(sv, bc, bf, fo, cell, fdims, nf.pscale_of(fext), dedupe)
    return xv, xc, xf, nf.normals(xv, xf), xn


@pytest.mark.gpu
def test_run_mesh_equals_the_restated_composition(hip):
    from test_gpu_mesh_finish import scene_run
    from sfm_mvs_amd import mesh
    imgs, K, P, gt, posearr, out, wv, wc, wf, origin, voxel, extent = scene_run()
    _, _, dims = mesh.volume_bounds(out["points"], 64)
    threshold = max(1, int(np.floor(len(wf) / 512)))
    cleaned = npc.clean(wv, wc, wf, threshold)
    plain = mesh.run_mesh(imgs, K, posearr, out, resolution=64)
    off = mesh.run_mesh(imgs, K, posearr, out, resolution=64, decimate=0, decimate_dedupe=False)
    assert sorted(plain) == sorted(off) == ["colors", "faces", "vertices"] and all(np.array_equal(plain[k], off[k]) for k in plain)
    for clean in (False, True):
        bv, bc, bf = (wv, wc, wf) if not clean else cleaned[:3]
        for smooth in (0, 3):
            xv, xc, xf, xnr, xn = restated_tail(bv, bc, bf, origin, voxel, dims, smooth, 2.0)
            for normals in (False, True):
                m = mesh.run_mesh(imgs, K, posearr, out, resolution=64, clean=clean, smooth=smooth, normals=normals, decimate=2)
                what = (clean, smooth, normals)
                assert sorted(m) == sorted(["colors", "faces", "vertices", "decimated_from", "decimate_unusable"] +
                                           ["components", "components_kept"] * clean + ["normals"] * normals), what
                assert m["vertices"].dtype == np.float64 and np.array_equal(m["vertices"], xv.astype(np.float64)), what
                assert np.array_equal(m["colors"], xc.astype(np.float64)) and m["faces"].dtype == np.int32 and np.array_equal(m["faces"], xf), what
                assert m["decimated_from"] == (len(bv), len(bf)) and m["decimate_unusable"] == int(xn[2]) == 0, what
                if clean:
                    assert [m["components"], m["components_kept"]] == cleaned[3][2:].tolist()
                if normals:
                    assert m["normals"].dtype == np.float64 and np.array_equal(m["normals"], xnr.astype(np.float64)), what
            print(f"run_mesh clean {clean} smooth {smooth} decimate 2: {len(bf)} -> {len(xf)} faces, {len(bv)} -> {len(xv)} vertices, {xn[3]} duplicates")
            assert 0 < len(xf) < len(bf) / 4
    xv, xc, xf, xnr, xn = restated_tail(wv, wc, wf, origin, voxel, dims, 0, 3.5, dedupe=False)
    m = mesh.run_mesh(imgs, K, posearr, out, resolution=64, decimate=3.5, decimate_dedupe=False, normals=True)
    assert np.array_equal(m["vertices"], xv.astype(np.float64)) and np.array_equal(m["faces"], xf) and np.array_equal(m["normals"], xnr.astype(np.float64))
    for bad in (0.5, -1, float("nan"), float("inf")):
        with pytest.raises(mesh.SfmHipError):
            mesh.run_mesh(imgs, K, posearr, out, resolution=64, decimate=bad)


@pytest.mark.gpu
@pytest.mark.parametrize("clean,smooth,normals", [(True, 3, True), (False, 3, True), (False, 0, False), (True, 0, False), (False, 0, True)])
def test_run_mesh_still_waits_for_the_host_only_twice(hip, clean, smooth, normals):
    import warnings
    from test_gpu_mesh_finish import scene_run
    from sfm_mvs_amd import _lib, mesh
    imgs, K, P, gt, posearr, out = scene_run()[:6]
    kw = dict(resolution=64, clean=clean, smooth=smooth, normals=normals, decimate=2)
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
    assert len(syncs) == 2, syncs
    assert int(_lib.lib().sfm_host_sync_count()) == lib0
    assert len(m["faces"]) > 0 and ("normals" in m) == normals and m["decimated_from"][1] > len(m["faces"])


@pytest.mark.gpu
def test_a_short_fixed_seed_fuzz_run_finds_no_mismatch(hip):
    counts, bad, dt = fz.run(10.0, 4343)
    print(f"fuzz_mesh_decimate: seed 4343, {sum(counts.values())} cases {counts}, {bad} mismatches, {dt:.0f} s")
    assert bad == 0 and all(c > 0 for c in counts.values()), counts


@pytest.mark.gpu
def test_committed_fuzz_logs_are_clean_and_name_this_code(hip):
    """profiles/mesh_decimate_fuzz_seed*.log: no mismatch, and run on the code of csrc/mesh_decimate.hip and csrc/common.h that the
    loaded library was built from (scripts/knn_code_hash.py: comments and whitespace do not count)."""
    import glob
    import re
    from sfm_mvs_amd import _lib
    have = _lib.code_hashes_of_binary()
    logs = sorted(glob.glob(os.path.join(ROOT, "profiles", "mesh_decimate_fuzz_seed*.log")))
    assert len(logs) >= 2, logs
    total = 0
    for path in logs:
        text = open(path).read()
        m = re.search(r"fuzz_mesh_decimate: seed \d+, (\d+) cases .*?, (\d+) mismatches", text)
        assert m and int(m.group(2)) == 0, f"{path}: no clean summary line"
        ids = re.findall(r"sfm_build_id (knn\.hip:\S+(?: \S+:\S+)*)", text)
        assert ids, f"{path} does not name the build it ran on"
        logged = dict(tok.split(":", 1) for tok in ids[-1].split() if ":" in tok)
        for name in ("mesh_decimate.hip", "common.h"):
            assert logged.get(name) == have[name], f"{path} was produced by another csrc/{name} than the loaded binary's"
        total += int(m.group(1))
    assert total >= FUZZ_FLOOR, total
