"""The mesh finishing step on the device (sfm_mesh_normals, sfm_mesh_smooth, mesh.mesh_normals, mesh.smooth_mesh,
run_mesh(smooth=..., normals=True)): every output equal to the restatement tests/np_mesh_finish.py as int32 views of the float rows;
there is no tolerance anywhere (include/sfm_hip.h, "MESH-FINISH"; docs/mesh.md §8)."""
import functools
import math
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
import np_mesh_finish as nf  # noqa: E402
import fuzz_mesh_finish as fz  # noqa: E402
from fuzz_mesh_clean import SENTINEL, bits, same, up  # noqa: E402

INT32_MAX = 2 ** 31 - 1
TAUBIN = np.tile(np.array([0.5, -0.53], np.float32), 32)
FUZZ_FLOOR = 2000               # a tenth of the cases the committed logs hold, rounded down to one figure (docs/mesh.md §8)


def check(v, f, origin, extent, steps=(0, 1, 3), counts=None):
    """sfm_mesh_normals and sfm_mesh_smooth (into sentinel-filled buffers) over one mesh against the restatement."""
    pscale = nf.pscale_of(extent)
    bad = fz.compare(fz.raw_normals(v, f, counts), nf.normals(v, f, counts), "normals")
    for n in steps:
        bad += fz.compare(fz.raw_smooth(v, f, TAUBIN[:n], origin, pscale, counts), nf.smooth(v, f, TAUBIN[:n], origin, pscale, counts),
                          f"vertices after {n} steps")
    assert not bad, bad


@functools.lru_cache(maxsize=None)
def real_meshes():
    """name -> (vertices, faces, origin, extent, the field (S, W, C, origin, voxel)) of the restated extraction of test_gpu_mesh.py's
    sphere and scene fields."""
    from test_gpu_mesh import fields
    out = {}
    for name, S, W, C, origin, voxel in fields():
        if name == "random":
            continue
        org = np.asarray(origin, np.float64).astype(np.float32)
        wv, _, wf = np_mesh.extract_mesh(S, W, C, org, np.float32(voxel), 1.0)
        out[name] = (wv, wf, org, float(voxel) * (max(S.shape) - 1), (S, W, C, origin, voxel))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sphere", "scene"])
def test_real_meshes_equal_the_restatement(hip, name):
    """Normals, smoothing at 0 / 1 / 2 / 7 steps and their composition through the Python operators, on extracted surfaces."""
    from sfm_mvs_amd import mesh
    wv, wf, origin, extent, (S, W, C, org, voxel) = real_meshes()[name]
    assert len(wf) > 100
    check(wv, wf, origin, extent, steps=(0, 1, 2, 7))
    v, _, f = mesh.extract_mesh(up(S), up(W), None if C is None else up(C), org, voxel, 1.0)
    assert same(v, wv) and same(f, wf)
    for pairs in (0, 1, 3):
        sv = mesh.smooth_mesh(v, f, pairs, origin, extent)
        want = nf.smooth(wv, wf, nf.taubin_factors(pairs), origin, nf.pscale_of(extent))
        assert same(sv, want), pairs
        assert same(mesh.mesh_normals(sv, f), nf.normals(want, wf)), pairs
    n = nf.normals(wv, wf).astype(np.float64)
    assert np.abs(np.linalg.norm(n[np.unique(wf)], axis=1) - 1.0).max() < 1e-6
    other = mesh.smooth_mesh(v, f, 2, origin, extent, lam=0.33, mu=-0.34)
    assert same(other, nf.smooth(wv, wf, nf.taubin_factors(2, 0.33, -0.34), origin, nf.pscale_of(extent)))


SIZES = [0, 1, 2, 3, 255, 256, 257, 65537]


@pytest.mark.gpu
@pytest.mark.parametrize("nv", SIZES)
def test_random_face_soups_at_the_block_edges(hip, nv):
    """nv and nf independently at 0..3, around one 256-block and past 2^16 (more than one block per launch, more than one
    wave per vertex); a quarter of the indices name no vertex, a tenth of the faces repeat an index or another face."""
    for nk in SIZES:
        rng = np.random.default_rng(1000003 * nv + nk)
        v = rng.uniform(-1.0, 3.0, (nv, 3)).astype(np.float32)
        f = fz.local_soup(rng, nv, nk, 4 if (nv + nk) % 2 else max(nv, 1))
        hit = rng.random((nk, 3)) < 0.25
        f[hit] = rng.choice(np.array([-1, nv, INT32_MAX], np.int64), int(hit.sum())).astype(np.int32)
        if nk > 3:
            k = rng.random(nk) < 0.1
            f[k, 1] = f[k, 0]
            f[rng.random(nk) < 0.1] = f[1]
        check(v, f, (-1.0, -1.0, -1.0), 4.0)


def repeated_face_mesh():
    """Face (0, 1, 2) 2^23 + 3 times and face (0, 3, 4) once: at vertex 0 the x sum passes 2^53 and is odd, so no float64 holds it."""
    v = np.array([[0, 0, 0], [-5e-4, 1, 0], [-6e-4, 0, 1], [1, 0.001, 0], [0.25, 0, 1]], np.float32)
    reps = 2 ** 23 + 3
    f = np.vstack([np.tile(np.array([[0, 1, 2]], np.int32), (reps, 1)), np.array([[0, 3, 4]], np.int32)])
    return v, f, reps


@pytest.mark.gpu
def test_contention_and_sums_past_2_to_the_53(hip):
    # one hub vertex in 70 001 faces
    rng = np.random.default_rng(9)
    nv, nk = 5000, 70001
    v = rng.uniform(0.0, 2.0, (nv, 3)).astype(np.float32)
    f = fz.local_soup(rng, nv, nk, 6)
    f[np.arange(nk), rng.integers(0, 3, nk)] = 1234
    check(v, f, (0.0, 0.0, 0.0), 2.0, steps=(2,))
    # one face 2^23 + 3 times: the expected words from Python integers
    v, f, reps = repeated_face_mesh()
    q, good = nf.face_terms(v, np.array([[0, 1, 2], [0, 3, 4]], np.int64))
    assert good.all()
    q = [[int(x) for x in row] for row in q]
    acc = {0: [reps * a + b for a, b in zip(q[0], q[1])], 1: [reps * a for a in q[0]], 2: [reps * a for a in q[0]], 3: q[1], 4: q[1]}
    assert abs(acc[0][0]) > 2 ** 53 and any(int(float(a)) != a for a in acc[0])
    want = np.zeros((5, 3), np.float32)
    for k, a in acc.items():
        d = [float(x) for x in a]                                   # Python int -> float rounds to nearest even
        L = math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        want[k] = [np.float32(x / L) for x in d]
    got = fz.raw_normals(v, f)
    assert np.array_equal(got, bits(want)), (got, bits(want))
    # one smoothing step over the same faces: acc = reps * (r_j1 + r_j2) (+ the single face), cnt = 2 * reps (+ 2)
    origin, pscale, factor = np.array([-2.5, -2.5, -2.5], np.float32), 2.0 ** 28, np.float32(0.5)     # r up to 3.5 * 2^28 < 2^30
    r, usable = nf.quantise(v, origin, pscale)
    assert usable.all()
    r = [[int(x) for x in row] for row in r]
    add = lambda a, b, m=1: [m * (x + y) for x, y in zip(a, b)]
    sums = {0: ([x + y for x, y in zip(add(r[1], r[2], reps), add(r[3], r[4]))], 2 * reps + 2), 1: (add(r[0], r[2], reps), 2 * reps),
            2: (add(r[0], r[1], reps), 2 * reps), 3: (add(r[0], r[4]), 2), 4: (add(r[0], r[3]), 2)}
    assert max(abs(x) for x in sums[0][0]) > 2 ** 53
    want = v.copy()
    for k, (a, cnt) in sums.items():
        for c in range(3):
            m = (float(a[c]) / float(cnt)) / float(pscale) + float(origin[c])
            want[k, c] = np.float32(float(v[k, c]) + float(factor) * (m - float(v[k, c])))
    got = fz.raw_smooth(v, f, [factor], origin, pscale)
    assert np.array_equal(got, bits(want)), (got, bits(want))
    assert same(nf.smooth(v, f[-5:], [factor], origin, pscale)[3:], want[3:])      # the restatement agrees where it is cheap to ask


@pytest.mark.gpu
def test_degenerate_coordinates(hip):
    rng = np.random.default_rng(21)
    nv, nk = 3000, 9000
    base = rng.uniform(0.0, 1.0, (nv, 3)).astype(np.float32)
    f = fz.local_soup(rng, nv, nk, 5)
    origin, extent = (0.0, 0.0, 0.0), 1.0
    for name, values in [("nan", [np.nan]), ("inf", [np.inf, -np.inf]), ("1e30", [1e30, -1e30]), ("1e-30", [1e-30, -1e-30, 0.0, -0.0])]:
        v = base.copy()
        hit = rng.random((nv, 3)) < (0.9 if name == "1e-30" else 0.1)
        v[hit] = rng.choice(np.array(values, np.float32), int(hit.sum()))
        if name == "1e-30":
            v[~hit] *= np.float32(1e-22)                            # cross products of 1e-44: below the float32 normals
        check(v, f, origin, extent if name != "1e-30" else 1e-22)
    # collinear and coincident vertices: zero-area faces contribute nothing, their vertices still smooth
    v = base.copy()
    t = rng.random(nv).astype(np.float32)
    line = np.outer(t, np.array([0.25, 0.5, 1.0], np.float32)).astype(np.float32)
    k = rng.random(nv) < 0.5
    v[k] = line[k]
    v[rng.random(nv) < 0.2] = v[7]
    check(v, f, origin, extent)
    assert not nf.normals(line, f).any()
    assert not fz.raw_normals(line, f).any()
    # vertices beyond 2^30 quanta next to usable ones; rows no face names, with NaN payloads: back bit for bit
    v = base.copy()
    far = rng.random(nv) < 0.1
    v[far] += rng.choice(np.array([2.5, -3.0, 64.0], np.float32), (int(far.sum()), 3))
    lonely = np.setdiff1d(np.arange(nv), np.unique(f))[:50]
    some = rng.choice(nv, 200, replace=False)
    raw = v.view(np.int32)
    raw[some[:100], 0], raw[some[100:], 2] = 0x7FC00123, -4194304 + 77
    v2 = np.vstack([v, v[:40]])                                     # 40 more rows in no face
    v2.view(np.int32)[nv:, 1] = 0x7F800001
    pscale = nf.pscale_of(extent)
    _, usable = nf.quantise(v2, np.zeros(3, np.float32), pscale)
    assert 0 < (~usable).sum() < len(v2) and (~usable[:nv][far]).all()
    check(v2, f, origin, extent, steps=(1, 4))
    got = fz.raw_smooth(v2, f, TAUBIN[:4], origin, pscale)
    keep = np.concatenate([np.flatnonzero(~usable), np.arange(nv, nv + 40), lonely])
    assert np.array_equal(got[keep], bits(v2)[keep])
    moved = np.setdiff1d(np.unique(f), np.flatnonzero(~usable))
    assert np.any(got[moved] != bits(v2)[moved])


@pytest.mark.gpu
def test_device_counts(hip):
    from sfm_mvs_amd import mesh
    wv, wf, origin, extent, (S, W, C, org, voxel) = real_meshes()["scene"]
    nv, nk = len(wv), len(wf)
    for counts in [(nv - 300, nk - 1000), (nv, nk), (0, 0), (0, nk), (nv, 0), (-1, nk - 5), (nv - 5, -2 ** 31), (nv + 1, nk + 1),
                   (INT32_MAX, INT32_MAX), (257, 256)]:
        check(wv, wf, origin, extent, steps=(0, 2), counts=counts)      # the sentinel at and past the counted rows is part of it
    # fed straight from clean_mesh's counts: nothing reads them on the host in between
    v, c, f = mesh.extract_mesh(up(S), up(W), up(C), org, voxel, 1.0)
    threshold = 8
    kv, kc, kf, kcounts = npc.clean(wv, None, wf, threshold)
    assert 0 < len(kv) < nv and 0 < len(kf) < nk
    sv = torch.full((nv, 3), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
    nr = torch.full((nv, 3), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
    mesh.clean_mesh(v, c, f, threshold, packed=True)                     # warm: the workspace
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ov, oc, of, counts, status, labels, buf = mesh.clean_mesh(v, c, f, threshold, packed=True)
        mesh.smooth_mesh(ov, of, 3, origin, extent, counts=counts, out=sv)
        mesh.mesh_normals(sv, of, counts=counts, out=nr)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert counts.cpu().numpy().tolist() == kcounts.tolist() and int(status[0]) == 1
    want_v = nf.smooth(kv, kf, nf.taubin_factors(3), origin, nf.pscale_of(extent))
    assert not fz.compare(bits(sv), want_v, "vertices") and not fz.compare(bits(nr), nf.normals(want_v, kf), "normals")


@pytest.mark.gpu
def test_face_order_and_repeated_runs_give_the_same_words(hip):
    wv, wf, origin, extent, _ = real_meshes()["scene"]
    rng = np.random.default_rng(5)
    pscale = nf.pscale_of(extent)
    first = (fz.raw_normals(wv, wf), fz.raw_smooth(wv, wf, TAUBIN[:6], origin, pscale))
    for f in (wf, wf[rng.permutation(len(wf))], wf[::-1].copy()):          # (rotating a face's corners is another input: a changes)
        assert np.array_equal(fz.raw_normals(wv, f), first[0]) and np.array_equal(fz.raw_smooth(wv, f, TAUBIN[:6], origin, pscale), first[1])


@functools.lru_cache(maxsize=None)
def scene_run():
    from test_gpu_mesh import mvs_of_scene
    from test_gpu_mesh_clean import restated_run_mesh
    from sfm_mvs_amd import mesh
    imgs, K, P, gt, posearr, out = mvs_of_scene(1, ndepth=32)
    wv, wc, wf, voxel = restated_run_mesh(imgs, K, P, out, 64)
    origin, _, dims = mesh.volume_bounds(out["points"], 64)
    return imgs, K, P, gt, posearr, out, wv, wc, wf, origin, voxel, voxel * (max(dims) - 1)


def facing_share(verts, normals, K, P, gt, voxel):
    """Share, among the vertices at least one camera sees (inside its frame, within half a voxel of its ground-truth depth), of
    those whose normal faces one of the cameras that see it."""
    v, n = np.asarray(verts, np.float64), np.asarray(normals, np.float64)
    h, w = gt[0].shape
    Xh = np.hstack([v, np.ones((len(v), 1))]).T
    seen, facing = np.zeros(len(v), bool), np.zeros(len(v), bool)
    for k in range(len(P)):
        Rt = np.linalg.solve(K, P[k])
        centre = -Rt[:, :3].T @ Rt[:, 3]
        q = P[k] @ Xh
        with np.errstate(divide="ignore", invalid="ignore"):
            u, t = np.floor(q[0] / q[2] + 0.5), np.floor(q[1] / q[2] + 0.5)
        ok = (q[2] > 0) & (u >= 0) & (u <= w - 1) & (t >= 0) & (t <= h - 1)
        g = np.where(ok, gt[k][np.where(ok, t, 0).astype(int), np.where(ok, u, 0).astype(int)], 0.0)
        sees = ok & (g > 0) & (np.abs(q[2] - g) <= 0.5 * voxel)
        seen |= sees
        facing |= sees & (np.einsum("ij,ij->i", n, centre[None] - v) > 0)
    return float(facing[seen].mean()), int(seen.sum())


@pytest.mark.gpu
def test_run_mesh_equals_the_restated_composition(hip):
    from sfm_mvs_amd import mesh
    imgs, K, P, gt, posearr, out, wv, wc, wf, origin, voxel, extent = scene_run()
    pscale = nf.pscale_of(extent)
    threshold = max(1, int(np.floor(len(wf) / 512)))
    cleaned = npc.clean(wv, wc, wf, threshold)
    for clean in (False, True):
        bv, bc, bf = (wv, wc, wf) if not clean else cleaned[:3]
        for smooth in (0, 3):
            sv = nf.smooth(bv, bf, nf.taubin_factors(smooth), origin.astype(np.float32), pscale)
            for normals in (False, True):
                m = mesh.run_mesh(imgs, K, posearr, out, resolution=64, clean=clean, smooth=smooth, normals=normals)
                what = (clean, smooth, normals)
                assert sorted(m) == sorted(["colors", "faces", "vertices"] + ["components", "components_kept"] * clean + ["normals"] * normals), what
                assert m["vertices"].dtype == np.float64 and np.array_equal(m["vertices"], sv.astype(np.float64)), what
                assert np.array_equal(m["colors"], bc.astype(np.float64)) and np.array_equal(m["faces"], bf), what
                if clean:
                    assert [m["components"], m["components_kept"]] == cleaned[3][2:].tolist()
                if normals:
                    wn = nf.normals(sv, bf)
                    assert m["normals"].dtype == np.float64 and np.array_equal(m["normals"], wn.astype(np.float64)), what
                    got, seen = facing_share(m["vertices"], m["normals"], K, P, gt, voxel)
                    ref, _ = facing_share(sv, wn, K, P, gt, voxel)
                    print(f"run_mesh clean {clean} smooth {smooth}: {len(bf)} faces, {seen} vertices seen, normals facing a camera {got:.4f}")
                    assert seen > 1000 and got >= ref, (got, ref)
    assert 0 < len(cleaned[2]) < len(wf)
    with pytest.raises(mesh.SfmHipError):
        mesh.run_mesh(imgs, K, posearr, out, resolution=64, smooth=33)
    with pytest.raises(mesh.SfmHipError):
        mesh.run_mesh(imgs, K, posearr, out, resolution=64, smooth=-1)


@pytest.mark.gpu
@pytest.mark.parametrize("clean,smooth,normals", [(True, 3, True), (False, 3, True), (False, 0, True), (True, 2, False)])
def test_run_mesh_still_waits_for_the_host_only_twice(hip, clean, smooth, normals):
    import warnings
    from sfm_mvs_amd import _lib, mesh
    imgs, K, P, gt, posearr, out = scene_run()[:6]
    kw = dict(resolution=64, clean=clean, smooth=smooth, normals=normals)
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
    assert len(m["faces"]) > 0 and ("normals" in m) == normals


@pytest.mark.gpu
def test_a_short_fixed_seed_fuzz_run_finds_no_mismatch(hip):
    counts, bad, dt = fz.run(10.0, 4343)
    print(f"fuzz_mesh_finish: seed 4343, {sum(counts.values())} cases {counts}, {bad} mismatches, {dt:.0f} s")
    assert bad == 0 and all(c > 0 for c in counts.values()), counts


@pytest.mark.gpu
def test_committed_fuzz_logs_are_clean_and_name_this_code(hip):
    """profiles/mesh_finish_fuzz_seed*.log: no mismatch, and run on the code of csrc/mesh_finish.hip and csrc/common.h that the
    loaded library was built from (scripts/knn_code_hash.py: comments and whitespace do not count)."""
    import glob
    import re
    from sfm_mvs_amd import _lib
    have = _lib.code_hashes_of_binary()
    logs = sorted(glob.glob(os.path.join(ROOT, "profiles", "mesh_finish_fuzz_seed*.log")))
    assert len(logs) >= 2, logs
    total = 0
    for path in logs:
        text = open(path).read()
        m = re.search(r"fuzz_mesh_finish: seed \d+, (\d+) cases .*?, (\d+) mismatches", text)
        assert m and int(m.group(2)) == 0, f"{path}: no clean summary line"
        ids = re.findall(r"sfm_build_id (knn\.hip:\S+(?: \S+:\S+)*)", text)
        assert ids, f"{path} does not name the build it ran on"
        logged = dict(tok.split(":", 1) for tok in ids[-1].split() if ":" in tok)
        for name in ("mesh_finish.hip", "common.h"):
            assert logged.get(name) == have[name], f"{path} was produced by another csrc/{name} than the loaded binary's"
        total += int(m.group(1))
    assert total >= FUZZ_FLOOR, total
