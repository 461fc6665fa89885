"""The mesh clean-up on the device (sfm_mesh_components, sfm_mesh_clean, mesh.mesh_components, mesh.clean_mesh,
run_mesh(clean=True)): every output equal to the integer restatement tests/np_mesh_clean.py — labels, counts, faces, and the int32
views of the float rows; there is no tolerance anywhere (include/sfm_hip.h, "MESH-CLEAN"; docs/mesh.md §7)."""
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
import fuzz_mesh_clean as fz  # noqa: E402
from fuzz_mesh_clean import bits, same, up  # noqa: E402

INT32_MAX = 2 ** 31 - 1
CONFIGS = [(0, False), (1, False), (8, False), (10 ** 9, False), (0, True), (8, True)]
FUZZ_FLOOR = 3000               # a tenth of the cases the committed logs hold, rounded down to one figure (docs/mesh.md §7)


def check(v, c, f, configs, rounds=None):
    """mesh_components and sfm_mesh_clean (into sentinel-filled buffers) over one mesh against the restatement -> its parts."""
    from sfm_mvs_amd import mesh
    nv = len(v)
    parts = npc.components(f, nv)
    labels, status = mesh.mesh_components(up(f), nv, **({} if rounds is None else dict(rounds=rounds)))
    assert int(status[0]) == 1, status.tolist()
    assert np.array_equal(labels.cpu().numpy(), parts[0])
    for min_faces, largest in configs:
        bad = fz.compare_clean(fz.raw_clean(v, c, f, labels, min_faces, largest), npc.clean(v, c, f, min_faces, largest, parts))
        assert not bad, (min_faces, largest, bad)
    return parts


@functools.lru_cache(maxsize=None)
def real_fields():
    from test_gpu_mesh import fields
    return {name: rest for name, *rest in fields()}


@pytest.mark.gpu
@pytest.mark.parametrize("name,w_min", [("sphere", 1.0), ("scene", 1.0), ("scene", 3.5)])
def test_real_meshes_equal_the_restatement(hip, name, w_min):
    """Extract, label, clean: the small sphere and the resolution-45 scene field of test_gpu_mesh.py."""
    from sfm_mvs_amd import mesh
    S, W, C, origin, voxel = real_fields()[name]
    v, c, f = mesh.extract_mesh(up(S), up(W), None if C is None else up(C), origin, voxel, w_min)
    wv, wc, wf = np_mesh.extract_mesh(S, W, C, np.asarray(origin, np.float64).astype(np.float32), np.float32(voxel), w_min)
    assert same(v, wv) and same(f, wf) and len(wf) > 100
    labels, faces_of = check(wv, wc, wf, CONFIGS)
    ncomp = int((labels == np.arange(len(wv))).sum())
    assert ncomp == 1 if name == "sphere" else ncomp > 3, ncomp
    # the Python entry point: device tensors in, full-size tensors and the counts out, one packed buffer
    for min_faces, largest in [(8, False), (1, True)]:
        kv, kc, kf, counts = npc.clean(wv, wc, wf, min_faces, largest, (labels, faces_of))
        ov, oc, of, cnt, status, lab, buf = mesh.clean_mesh(v, c, f, min_faces, largest, packed=True)
        host = buf.cpu().numpy()
        assert host[:4].tolist() == counts.tolist() and host[4] == 1 and np.array_equal(lab.cpu().numpy(), labels)
        assert same(ov[:len(kv)], kv) and same(of[:len(kf)], kf) and (oc is None) == (wc is None)
        assert oc is None or same(oc[:len(kv)], kc)
        assert np.array_equal(host[6:6 + 3 * len(kv)], bits(kv).ravel())
        o2 = mesh.clean_mesh(v, c, f, min_faces, largest)
        assert len(o2) == 4 and same(o2[3], cnt) and same(o2[0][:len(kv)], kv) and same(o2[2][:len(kf)], kf)


SIZES = [0, 1, 2, 3, 255, 256, 257, 262143, 262144, 262145, 2 ** 20 + 1]


@pytest.mark.gpu
@pytest.mark.parametrize("nf", SIZES)
@pytest.mark.parametrize("nv", SIZES)
def test_random_face_soups_at_the_scan_and_block_edges(hip, nv, nf):
    """nv and nf at 0..3, around one 256-block, around 1024 blocks (one segment each of the scan's 1024 lanes, then two) and past
    2^20; indices drawn from a few hundred to nv clusters, so the component count runs from 1 to about nv."""
    rng = np.random.default_rng(1000003 * nv + nf)
    ncl = [1, 300, max(nv // 2, 1), max(nv, 1)][(SIZES.index(nv) + SIZES.index(nf)) % 4]
    f = fz.soup(rng, nv, nf, ncl)
    v = fz.rows(rng, nv)
    c = fz.rows(rng, nv) if (nv + nf) % 2 else None
    labels, faces_of = check(v, c, f, [(2, False), (1, True)] if nf else [(0, False), (1, False), (0, True)])
    assert int(faces_of.sum()) == nf * (nv > 0)               # every drawn face is valid


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["ascending", "descending", "zigzag", "permuted"])
def test_long_strips_converge_and_resume(hip, order):
    """300 000-face strips: converged at the default rounds with every label the minimum; the same labels from single rounds
    resumed from the host, every intermediate state a valid one."""
    from sfm_mvs_amd import mesh
    f, nv = fz.strip(300000, order, np.random.default_rng(5))
    fd = up(f)
    labels, status = mesh.mesh_components(fd, nv)
    done, changed = (int(s) for s in status.cpu())
    print(f"strip {order}: converged {done} after {changed} changing rounds of {mesh.COMPONENT_ROUNDS}")
    assert done == 1 and changed < mesh.COMPONENT_ROUNDS, (done, changed)
    assert int(labels.max()) == 0 and int(labels.min()) == 0
    res = fz.labels_by_resume(fd, nv, 1, np.zeros(nv, np.int64))
    assert not isinstance(res, str), res
    got, calls, total = res
    print(f"strip {order}: {calls} calls of one round, {total} of them changed something")
    assert np.array_equal(got, labels.cpu().numpy()) and calls == total + 1


def tiny_components(pairs, seed):
    """100 000 disjoint triangles and `pairs` two-face pairs, vertex ids permuted, faces shuffled."""
    rng = np.random.default_rng(seed)
    n = 100000
    tri = np.arange(3 * n).reshape(n, 3)
    extra = []
    for k in range(pairs):
        b = 3 * n + 4 * k
        extra += [[b, b + 1, b + 2], [b + 1, b + 2, b + 3]]
    f = np.vstack([tri, np.array(extra).reshape(-1, 3)])
    nv = 3 * n + 4 * pairs
    f = rng.permutation(nv)[f][rng.permutation(len(f))].astype(np.int32)
    return fz.rows(rng, nv), f


@pytest.mark.gpu
def test_many_tiny_components(hip):
    v, f = tiny_components(1, 11)
    labels, faces_of = check(v, None, f, [(1, False), (2, False), (3, False), (0, True)])
    assert npc.clean(v, None, f, 2, False, (labels, faces_of))[3].tolist() == [4, 2, 100001, 1]
    assert npc.clean(v, None, f, 3, False, (labels, faces_of))[3].tolist() == [0, 0, 100001, 0]
    v, f = tiny_components(2, 12)                             # two components tied on two faces: the lower label wins
    labels, faces_of = check(v, None, f, [(0, True), (2, True), (3, True), (2, False)])
    best = np.flatnonzero(faces_of == 2)
    assert len(best) == 2
    kv, _, kf, counts = npc.clean(v, None, f, 0, True, (labels, faces_of))
    assert counts.tolist() == [4, 2, 100002, 1] and same(kv, v[labels == best.min()])


@pytest.mark.gpu
def test_degenerate_inputs(hip):
    rng = np.random.default_rng(21)
    v, c = fz.rows(rng, 700), fz.rows(rng, 700)
    none = np.zeros((0, 3), np.int32)
    parts = check(v, c, none, [(0, False), (1, False), (0, True), (1, True)])            # nf = 0
    assert npc.clean(v, c, none, 0, False, parts)[3].tolist() == [700, 0, 700, 700]      # everything back
    assert npc.clean(v, c, none, 1, False, parts)[3].tolist() == [0, 0, 700, 0]          # nothing back
    f = fz.soup(rng, 700, 900, 40)
    check(np.zeros((0, 3), np.float32), None, f, [(0, False), (1, False), (0, True)])    # nv = 0: every face invalid
    check(np.zeros((0, 3), np.float32), None, none, [(0, False), (0, True)])
    bad = f.copy()                                                                        # every face invalid, one index each
    bad[np.arange(900), rng.integers(0, 3, 900)] = rng.choice(np.array([-1, -2 ** 31, 700, INT32_MAX]), 900).astype(np.int32)
    parts = check(v, c, bad, [(0, False), (1, False), (0, True)])
    assert npc.clean(v, c, bad, 0, False, parts)[3].tolist() == [700, 0, 700, 700]
    some = f.copy()                                                                       # a third of them
    some[::3, 1] = np.array([-1, 700, INT32_MAX] * 100, np.int32)
    check(v, c, some, [(0, False), (1, False), (3, False), (0, True)])
    dup = f.copy()                                                                        # duplicates, (a,a,a), (a,a,b)
    dup[100:200] = dup[0]
    dup[200:300, 1] = dup[200:300, 0]
    dup[300:400, 1:] = dup[300:400, :1]
    parts = check(v, c, dup, [(0, False), (1, False), (2, False), (0, True)])
    assert parts[1].sum() == 900                                                          # every one of them counts as a face
    nan = v.copy()                                                                        # NaN payloads and infinities survive
    raw = nan.view(np.int32)
    raw[::5, 0], raw[1::5, 1], raw[2::5, 2], raw[3::5, 0] = 0x7FC00123, -4194304 + 77, 0x7F800000, 0x7F800001
    assert np.isnan(nan).any() and np.isinf(nan).any()
    check(nan, nan[::-1].copy(), f, [(0, False), (2, False), (0, True)])
    check(v, None, f, [(0, False), (2, False), (0, True)])                                # colours absent


@pytest.mark.gpu
def test_min_faces_zero_returns_the_inputs_and_nothing_is_written_past_the_counts(hip):
    from sfm_mvs_amd import mesh
    S, W, C, origin, voxel = real_fields()["scene"]
    v, c, f = (t.cpu().numpy() for t in mesh.extract_mesh(up(S), up(W), up(C), origin, voxel, 1.0))
    labels, _ = mesh.mesh_components(up(f), len(v))
    ov, oc, of, counts = fz.raw_clean(v, c, f, labels, 0, False)
    assert counts[:2].tolist() == [len(v), len(f)] and counts[2] == counts[3] > 3
    assert np.array_equal(ov, bits(v)) and np.array_equal(oc, bits(c)) and np.array_equal(of, f)
    ov, oc, of, counts = fz.raw_clean(v, c, f, labels, 8, False)
    kv, kf = int(counts[0]), int(counts[1])
    assert 0 < kv < len(v) and 0 < kf < len(f) and counts[3] < counts[2]
    for buf, k in ((ov, kv), (oc, kv), (of, kf)):
        assert np.all(buf[k:] == fz.SENTINEL) and not np.any(np.all(buf[:k] == fz.SENTINEL, axis=1))
    ov, oc, of, counts = fz.raw_clean(v, c, f, labels, 10 ** 9, False)
    assert counts[[0, 1, 3]].tolist() == [0, 0, 0] and all(np.all(b == fz.SENTINEL) for b in (ov, oc, of))


@pytest.mark.gpu
def test_repeated_runs_and_other_round_counts_give_the_same(hip):
    from sfm_mvs_amd import mesh
    rng = np.random.default_rng(33)
    nv, nf = 200001, 300007
    f, v, c = fz.soup(rng, nv, nf, 5000), fz.rows(rng, nv), fz.rows(rng, nv)
    fd = up(f)
    runs = []
    for rounds in (mesh.COMPONENT_ROUNDS, mesh.COMPONENT_ROUNDS, 64, 1024):
        labels, status = mesh.mesh_components(fd, nv, rounds)
        assert int(status[0]) == 1
        runs.append([labels.cpu().numpy()] + list(fz.raw_clean(v, c, f, labels, 3, False)))
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert np.array_equal(a, b)
    again, status = mesh.mesh_components(fd, nv, 3, up(runs[0][0]))                      # resumed from converged labels: unchanged
    assert status.tolist() == [1, 0] and np.array_equal(again.cpu().numpy(), runs[0][0])


def restated_run_mesh(imgs, K, P, out, resolution):
    """run_mesh(clean=False) from the restatement, over the run's own depth maps and masks (as test_run_mesh_on_a_rendered_scene)."""
    from sfm_mvs_amd import mesh, mvs
    n = len(P)
    origin, voxel, dims = mesh.volume_bounds(out["points"], resolution)
    depths = [d.cpu().numpy() for d in out["depths"]]
    masks = []
    for i in range(n):
        nb = mvs.neighbours(i, n, 4)
        ab, bc = mvs.consistency_matrices(K, P[i], P[nb])
        masks.append(mvs.consistency(out["depths"][i], [out["depths"][j] for j in nb], nb, ab, i, bc, 0.01, 2, False)[0].cpu().numpy())
    S, W, C = np_mesh.tsdf_integrate(np.stack(depths), mesh.projection_rows(K, P), origin, voxel, dims,
                                     np.float32(mesh.TRUNC_VOXELS * voxel), mask=np.stack(masks), bgr=np.stack(imgs))
    return np_mesh.extract_mesh(S, W, C, origin.astype(np.float32), np.float32(voxel), mesh.W_MIN) + (voxel,)


@pytest.mark.gpu
def test_run_mesh_clean_on_a_rendered_scene(hip):
    from test_gpu_mesh import mvs_of_scene
    from test_mesh_cpu import MIN_ON_SURFACE, RUN_MESH_RESOLUTION, on_surface_fraction
    from sfm_mvs_amd import mesh
    imgs, K, P, gt, posearr, out = mvs_of_scene(0)
    wv, wc, wf, voxel = restated_run_mesh(imgs, K, P, out, RUN_MESH_RESOLUTION)

    def equal(m, v, c, f):
        return (m["vertices"].dtype == np.float64 and m["faces"].dtype == np.int32 and np.array_equal(m["vertices"], v.astype(np.float64))
                and np.array_equal(m["colors"], c.astype(np.float64)) and np.array_equal(m["faces"], f))

    plain = mesh.run_mesh(imgs, K, posearr, out, resolution=RUN_MESH_RESOLUTION)
    assert sorted(plain) == ["colors", "faces", "vertices"] and equal(plain, wv, wc, wf)      # clean=False: what it was
    keep_all = mesh.run_mesh(imgs, K, posearr, out, resolution=RUN_MESH_RESOLUTION, clean=True, min_component_faces=0)
    assert equal(keep_all, wv, wc, wf) and keep_all["components"] == keep_all["components_kept"] > 1
    cleaned = mesh.run_mesh(imgs, K, posearr, out, resolution=RUN_MESH_RESOLUTION, clean=True)
    threshold = max(1, int(np.floor(len(wf) / 512)))
    kv, kc, kf, counts = npc.clean(wv, wc, wf, threshold)
    assert equal(cleaned, kv, kc, kf) and [cleaned["components"], cleaned["components_kept"]] == counts[2:].tolist()
    assert 0 < len(kf) < len(wf) and counts[3] < counts[2]
    before = on_surface_fraction(plain["vertices"], K, P, gt, voxel)
    after = on_surface_fraction(cleaned["vertices"], K, P, gt, voxel)
    print(f"run_mesh: {len(wf)} faces, threshold {threshold}, {counts[2]} -> {counts[3]} components, {len(wf) - len(kf)} faces dropped, "
          f"on surface {before:.4f} -> {after:.4f}")
    assert after >= before and after >= MIN_ON_SURFACE, (before, after)
    for kw, want in [(dict(min_component_faces=10 ** 9), 0), (dict(largest_only=True), 1), (dict(min_component_share=0.0), None)]:
        m = mesh.run_mesh(imgs, K, posearr, out, resolution=RUN_MESH_RESOLUTION, clean=True, **kw)
        o = npc.clean(wv, wc, wf, kw.get("min_component_faces", 1 if "min_component_share" in kw else threshold), kw.get("largest_only", False))
        assert equal(m, *o[:3]) and (want is None or m["components_kept"] == want)


@pytest.mark.gpu
@pytest.mark.parametrize("on_device", [True, False])
def test_run_mesh_clean_waits_for_the_host_only_for_the_totals_and_the_download(hip, on_device):
    import warnings
    from test_gpu_mesh import mvs_of_scene
    from sfm_mvs_amd import _lib, mesh
    imgs, K, P, gt, posearr, out = mvs_of_scene(1, ndepth=32)
    frames = [up(im) for im in imgs] if on_device else imgs
    mesh.run_mesh(frames, K, posearr, out, resolution=64, clean=True)            # warm: the pinned host pool, the workspace
    torch.cuda.synchronize()
    lib0 = int(_lib.lib().sfm_host_sync_count())
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            m = mesh.run_mesh(frames, K, posearr, out, resolution=64, clean=True)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    syncs = [str(w.message) for w in caught if "synchroniz" in str(w.message).lower()]
    assert len(syncs) == 2, syncs
    assert int(_lib.lib().sfm_host_sync_count()) == lib0
    assert len(m["faces"]) > 0 and m["components_kept"] >= 1


@pytest.mark.gpu
def test_a_short_fixed_seed_fuzz_run_finds_no_mismatch(hip):
    counts, bad, dt = fz.run(10.0, 4242)
    print(f"fuzz_mesh_clean: seed 4242, {sum(counts.values())} cases {counts}, {bad} mismatches, {dt:.0f} s")
    assert bad == 0 and all(c > 0 for c in counts.values()), counts


@pytest.mark.gpu
def test_committed_fuzz_logs_are_clean_and_name_this_code(hip):
    """profiles/mesh_clean_fuzz_seed*.log: no mismatch, and run on the code of csrc/mesh_clean.hip and csrc/common.h that the loaded
    library was built from (scripts/knn_code_hash.py: comments and whitespace do not count)."""
    import glob
    import re
    from sfm_mvs_amd import _lib
    have = _lib.code_hashes_of_binary()
    logs = sorted(glob.glob(os.path.join(ROOT, "profiles", "mesh_clean_fuzz_seed*.log")))
    assert len(logs) >= 2, logs
    total = 0
    for path in logs:
        text = open(path).read()
        m = re.search(r"fuzz_mesh_clean: seed \d+, (\d+) cases .*?, (\d+) mismatches", text)
        assert m and int(m.group(2)) == 0, f"{path}: no clean summary line"
        ids = re.findall(r"sfm_build_id (knn\.hip:\S+(?: \S+:\S+)*)", text)
        assert ids, f"{path} does not name the build it ran on"
        logged = dict(tok.split(":", 1) for tok in ids[-1].split() if ":" in tok)
        for name in ("mesh_clean.hip", "common.h"):
            assert logged.get(name) == have[name], f"{path} was produced by another csrc/{name} than the loaded binary's"
        total += int(m.group(1))
    assert total >= FUZZ_FLOOR, total
