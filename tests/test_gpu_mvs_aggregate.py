"""The cost-volume aggregation on the device (sfm_mvs_cost_shift, sfm_mvs_cost_aggregate, sfm_mvs_cost_depth, mvs.aggregate_depth,
run_mvs(aggregate=True)): every output equal to the integer restatement tests/np_mvs_aggregate.py as integers / int32 views, at
the limits of every argument, and held to the accuracy bars of tests/test_mvs_aggregate_cpu.py on the rendered scene."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

import np_mvs  # noqa: E402
import np_mvs_aggregate as agg  # noqa: E402
from mvs_scenes import gray, render_scene, scene_cloud, surface_error  # noqa: E402

F = np.float32


def bits(t):
    a = t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return a.view(np.int32) if a.dtype == np.float32 else a


def same(a, b):
    a, b = bits(a), bits(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def invd_of(nd):
    return np.linspace(0.1, 0.7, nd, dtype=np.float64).astype(F)


def check_all(vol, invd, shift, p1, p2, ndir, gate):
    """The three entry points one by one (each fed the restatement's input) and composed; returns the restatement's outputs."""
    from sfm_mvs_amd import mvs
    wq = agg.cost_shift(vol, shift)
    ws = agg.cost_aggregate(wq, p1, p2, ndir)
    wd, wc, wpl = agg.cost_depth(ws, wq, invd, gate)
    assert same(mvs.cost_shift(up(vol), shift), wq), "Q"
    assert same(mvs.cost_aggregate(up(wq), p1, p2, ndir), ws), "S"
    d, c, pl = mvs.cost_depth(up(ws), up(wq), up(invd), gate)
    assert same(d, wd) and same(c, wc) and same(pl, wpl), "depth / cost / plane"
    d2, c2, none = mvs.cost_depth(up(ws), up(wq), up(invd), gate, plane=False)          # plane_dev NULL changes nothing else
    assert none is None and same(d2, wd) and same(c2, wc)
    # composed on the device, Q and S never leaving it
    q = mvs.cost_shift(up(vol), shift)
    s = mvs.cost_aggregate(q, p1, p2, ndir)
    d3, c3, pl3 = mvs.cost_depth(s, q, up(invd), gate)
    assert same(d3, wd) and same(c3, wc) and same(pl3, wpl), "composed"
    return wq, ws, wd, wc, wpl


def random_volume(rng, nd, h, w):
    return rng.uniform(0, 2, (nd, h, w)).astype(F)


def scene_volume(seed=0, ndepth=128, w=160, h=120):
    from sfm_mvs_amd import mvs
    imgs, K, P, gt = render_scene(n=5, w=w, h=h, seed=seed)
    X = scene_cloud(K, P, gt)
    nb = mvs.neighbours(2, 5, 4)
    invd = mvs._inverse_depths_host(*mvs.depth_range(X, P[2], P_all=P), ndepth)
    mv = mvs.sweep_matrices(K, P[2], P[nb])
    _, _, _, vol = mvs.plane_sweep(up(gray(imgs[2])), [up(gray(imgs[v])) for v in nb], mv, up(invd), 3, 2, mvs.VAR_MIN, mvs.COST_MAX, volume=True)
    return vol.cpu().numpy(), invd, gt[2]


@pytest.mark.gpu
@pytest.mark.parametrize("ndir", [4, 8])
def test_the_rendered_scenes_volume_entry_by_entry_and_composed(hip, ndir):
    from sfm_mvs_amd import mvs
    from test_mvs_aggregate_cpu import MIN_AGG_WITHIN_1PCT
    from test_mvs_cpu import depth_accuracy
    vol, invd, truth = scene_volume()
    _, _, wd, _, _ = check_all(vol, invd, mvs.SHIFT, mvs.P1, mvs.P2, ndir, mvs.quantise_cost(mvs.COST_MAX))
    got = mvs.aggregate_depth(up(vol), up(invd), ndir=ndir)
    assert same(got[0], wd)
    valid, within = depth_accuracy(wd, truth, 3)
    print(f"ndir {ndir}: valid {valid:.4f} within 1 % {within:.4f}")
    if ndir == 8:
        assert within >= MIN_AGG_WITHIN_1PCT, within


FRAMES = [(1, 1), (40, 1), (1, 40), (15, 15), (16, 16), (17, 33), (257, 65), (4099, 3), (2, 4099)]


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", FRAMES)
def test_frames_from_one_pixel_to_a_side_of_4099(hip, w, h):
    """Every frame with every shift 0..4 (windows larger than the frame included) and both ndir, on random volumes."""
    rng = np.random.default_rng(w * 10007 + h)
    for shift in range(5):
        nd = int(rng.choice([2, 5, 17]))
        vol = random_volume(rng, nd, h, w)
        check_all(vol, invd_of(nd), shift, 10, 102, 4 + 4 * (shift & 1), 307)
    check_all(random_volume(rng, 9, h, w), invd_of(9), 2, 7, 300, 4, 1024)
    check_all(random_volume(rng, 9, h, w), invd_of(9), 2, 7, 300, 8, 1024)


@pytest.mark.gpu
@pytest.mark.parametrize("nd", [2, 3, 63, 64, 65, 128, 129, 1024])
def test_plane_counts_about_the_powers_of_two_and_at_the_limits(hip, nd):
    rng = np.random.default_rng(nd)
    w, h = (37, 21) if nd < 1024 else (19, 11)
    vol = random_volume(rng, nd, h, w)
    vol[:, rng.random((h, w)) < 0.3] = 2.0
    check_all(vol, invd_of(nd), 1, 10, 102, 8, 307)
    check_all(vol, invd_of(nd), 3, 50, 400, 4, 2049)


@pytest.mark.gpu
@pytest.mark.parametrize("p1,p2", [(0, 0), (0, 2048), (2048, 2048), (None, None)])
@pytest.mark.parametrize("ndir", [4, 8])
def test_penalties_at_their_ends(hip, p1, p2, ndir):
    from sfm_mvs_amd import mvs
    p1, p2 = (mvs.P1, mvs.P2) if p1 is None else (p1, p2)
    rng = np.random.default_rng(5)
    vol = random_volume(rng, 33, 29, 45)
    wq, ws, *_ = check_all(vol, invd_of(33), 2, p1, p2, ndir, 307)
    if p2 == 0:
        assert np.array_equal(ws.astype(np.int64), ndir * wq.astype(np.int64))
    high = np.full((6, 9, 11), 5.0, F)                          # all 2048: the largest L and S
    _, ws, *_ = check_all(high, invd_of(6), 0, p1, p2, ndir, 2048)
    assert int(ws.max()) <= 32768


@pytest.mark.gpu
@pytest.mark.parametrize("gate", [0, 1, 2048, 2049])
def test_special_volumes_and_gates(hip, gate):
    rng = np.random.default_rng(gate)
    nd, h, w = 12, 23, 31
    inv = invd_of(nd)
    for const in (0.0, 2.0):                                    # every plane tied: plane 0 wins, no parabola
        _, _, wd, wc, wpl = check_all(np.full((nd, h, w), const, F), inv, 2, 10, 102, 8, gate)
        assert not wpl.any()
        q0 = 0 if const == 0.0 else 2048
        assert np.all(wd == (0 if q0 >= gate else F(1) / inv[0])) and np.all(wc == F(q0) / F(1024))
    vol = random_volume(rng, nd, h, w)
    for v in (np.nan, np.inf, -np.inf, -3.0, -0.0, 2.0, 1e-30):
        vol[rng.random((nd, h, w)) < 0.03] = F(v)
    check_all(vol, inv, 1, 10, 102, 8, gate)
    first = random_volume(rng, nd, h, w) * F(0.5) + F(0.5)
    first[0] = 0.0                                              # the winner on the first plane
    assert not check_all(first, inv, 0, 10, 102, 8, gate)[4].any()
    last = random_volume(rng, nd, h, w) * F(0.5) + F(0.5)
    last[-1] = 0.0                                              # ... and on the last
    assert np.all(check_all(last, inv, 0, 10, 102, 4, gate)[4] == nd - 1)
    ties = (rng.integers(0, 2049, (nd, h, w)) / 1024.0 + 1.0 / 2048.0).astype(F)     # exact rounding ties
    check_all(ties, inv, 1, 10, 102, 4, gate)


@pytest.mark.gpu
def test_buffers_are_reused_and_wrong_ones_refused(hip):
    from sfm_mvs_amd import mvs
    rng = np.random.default_rng(3)
    vol, inv = random_volume(rng, 8, 10, 12), invd_of(8)
    q = torch.empty((8, 10, 12), dtype=torch.uint16, device="cuda")
    s = torch.empty_like(q)
    want = agg.aggregate_depth(vol, inv, 3, 10, 102, 8, 0.3)
    for _ in range(2):
        got = mvs.aggregate_depth(up(vol), up(inv), 3, 10, 102, 8, 0.3, q_out=q, s_out=s)
        assert all(same(a, b) for a, b in zip(got, want))
    assert same(q, agg.cost_shift(vol, 3)) and same(s, agg.cost_aggregate(agg.cost_shift(vol, 3), 10, 102, 8))
    with pytest.raises(mvs.SfmHipError):
        mvs.cost_shift(up(vol), 1, out=torch.empty((8, 10, 13), dtype=torch.uint16, device="cuda"))
    with pytest.raises(mvs.SfmHipError):
        mvs.cost_aggregate(q, 10, 102, 8, out=q)                # in place
    with pytest.raises(mvs.SfmHipError):
        mvs.cost_aggregate(q, 200, 100, 8)
    with pytest.raises(mvs.SfmHipError):
        mvs.cost_shift(torch.from_numpy(vol), 1)                # a host tensor: no CPU path


def np_run_mvs_aggregate(imgs, K, P, X, ndepth=128, radius=3, shift=None, p1=None, p2=None, ndir=8):
    """run_mvs(aggregate=True) restated: np_mvs sweeps, the restated aggregation, np_mvs consistency, view-major compaction."""
    from sfm_mvs_amd import mvs
    n = len(P)
    nbrs = [mvs.neighbours(i, n, 4) for i in range(n)]
    depths = []
    for i in range(n):
        invd = mvs._inverse_depths_host(*mvs.depth_range(X, P[i], P_all=P), ndepth)
        vol = np_mvs.plane_sweep(gray(imgs[i]), [gray(imgs[v]) for v in nbrs[i]], mvs.sweep_matrices(K, P[i], P[nbrs[i]]), invd, radius, 2,
                                 mvs.VAR_MIN, mvs.COST_MAX)[3]
        depths.append(agg.aggregate_depth(vol, invd, radius if shift is None else shift, mvs.P1 if p1 is None else p1,
                                          mvs.P2 if p2 is None else p2, ndir, mvs.COST_MAX)[0])
    masks, xyzs = [], []
    for i in range(n):
        ab, bc = mvs.consistency_matrices(K, P[i], P[nbrs[i]])
        m, x = np_mvs.consistency(depths[i], [depths[v] for v in nbrs[i]], nbrs[i], ab, i, bc, 0.01, 2, True)
        masks.append(m)
        xyzs.append(x)
    idx = np.flatnonzero(np.stack(masks).reshape(-1))
    return depths, np.stack(xyzs).reshape(-1, 3)[idx].astype(np.float64), np.stack(imgs).reshape(-1, 3)[idx].astype(np.float64)


@pytest.mark.gpu
def test_run_mvs_aggregate_equals_the_restated_composition_and_meets_the_cpu_bars(hip):
    from sfm_mvs_amd import mvs
    from test_mvs_aggregate_cpu import MAX_WRONG_RATIO, MIN_AGG_WITHIN_1PCT
    from test_mvs_cpu import MIN_FUSED_WITHIN_1PCT, depth_accuracy
    imgs, K, P, gt = render_scene(n=5, w=160, h=120, seed=0)
    posearr = np.hstack([K.ravel()] + [p.ravel() for p in P])
    X = scene_cloud(K, P, gt)
    out = mvs.run_mvs(imgs, K, posearr, X, aggregate=True)
    depths, pts, cols = np_run_mvs_aggregate(imgs, K, P, X)
    for a, b in zip(out["depths"], depths):
        assert same(a, b)
    assert np.array_equal(out["points"], pts) and np.array_equal(out["colors"], cols)
    parent = mvs.run_mvs(imgs, K, posearr, X)
    pv, pw = depth_accuracy(parent["depths"][2].cpu().numpy(), gt[2], 3)
    valid, within = depth_accuracy(out["depths"][2].cpu().numpy(), gt[2], 3)
    on_surface = float((surface_error(out["points"], K, P, gt) <= 0.01).mean())
    print(f"parent {pv:.4f} / {pw:.4f} ({len(parent['points'])} points), aggregated {valid:.4f} / {within:.4f} "
          f"({len(pts)} points, {on_surface:.4f} on the surfaces)")
    assert (1 - within) <= MAX_WRONG_RATIO * (1 - pw) and valid >= pv and within >= MIN_AGG_WITHIN_1PCT
    assert len(pts) > 5000 and on_surface >= MIN_FUSED_WITHIN_1PCT
    # the option reaches run_mvs through its other arguments too: 4 directions, no shift
    out4 = mvs.run_mvs(imgs, K, posearr, X, ndepth=32, aggregate=True, shift=0, p1=5, p2=60, ndir=4)
    d4, p4, _ = np_run_mvs_aggregate(imgs, K, P, X, ndepth=32, shift=0, p1=5, p2=60, ndir=4)
    assert all(same(a, b) for a, b in zip(out4["depths"], d4)) and np.array_equal(out4["points"], p4)


@pytest.mark.gpu
def test_run_mvs_defaults_are_those_of_aggregate_false(hip):
    from sfm_mvs_amd import mvs
    imgs, K, P, gt = render_scene(n=5, w=160, h=120, seed=1)
    posearr = np.hstack([K.ravel()] + [p.ravel() for p in P])
    X = scene_cloud(K, P, gt)
    a = mvs.run_mvs(imgs, K, posearr, X, ndepth=24)
    b = mvs.run_mvs(imgs, K, posearr, X, ndepth=24, aggregate=False)
    assert all(same(x, y) for x, y in zip(a["depths"], b["depths"]))
    assert np.array_equal(a["points"], b["points"]) and np.array_equal(a["colors"], b["colors"])
    want = np_mvs.plane_sweep(gray(imgs[2]), [gray(imgs[v]) for v in mvs.neighbours(2, 5, 4)],
                              mvs.sweep_matrices(K, P[2], P[mvs.neighbours(2, 5, 4)]),
                              mvs._inverse_depths_host(*mvs.depth_range(X, P[2], P_all=P), 24), 3, 2, mvs.VAR_MIN, mvs.COST_MAX)[0]
    assert same(a["depths"][2], want)                           # ... and still the winner-take-all map of the sweep


@pytest.mark.gpu
def test_run_sfm_images_passes_the_option_through(hip):
    from datagen import gustav_views
    from sfm_mvs_amd import pipeline as pl
    images, K, _ = gustav_views(6, seed=5)
    opts = dict(ndepth=8, radius=2, nsrc=2, topk=1)
    out = pl.run_sfm_images(images, K, densify=True, mvs_options=opts, aggregate=True)
    direct = pl.run_sfm_images(images, K, densify=True, mvs_options=dict(opts, aggregate=True))
    plain = pl.run_sfm_images(images, K, densify=True, mvs_options=opts)
    for a, b in zip(out["dense"]["depths"], direct["dense"]["depths"]):
        assert same(a, b)
    assert any(not same(a, b) for a, b in zip(out["dense"]["depths"], plain["dense"]["depths"]))
    assert np.array_equal(out["posearr"], plain["posearr"])


@pytest.mark.gpu
@pytest.mark.parametrize("on_device", [True, False])
def test_run_mvs_aggregate_waits_for_the_host_twice(hip, on_device):
    """As tests/test_gpu_mvs.py counts them for the plain call: under torch's sync debug mode the aggregated call synchronises for
    the fused count and the one download, and the library itself waits for nothing."""
    import warnings
    from sfm_mvs_amd import _lib, mvs
    imgs, K, P, gt = render_scene(n=5, w=160, h=120, seed=1)
    posearr = np.hstack([K.ravel()] + [p.ravel() for p in P])
    X = scene_cloud(K, P, gt)
    frames = [up(im) for im in imgs] if on_device else imgs
    mvs.run_mvs(frames, K, posearr, X, ndepth=16, aggregate=True)
    torch.cuda.synchronize()
    lib0 = int(_lib.lib().sfm_host_sync_count())
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            out = mvs.run_mvs(frames, K, posearr, X, ndepth=16, aggregate=True)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    syncs = [str(w.message) for w in caught if "synchroniz" in str(w.message).lower()]
    assert len(syncs) == 2, syncs
    assert int(_lib.lib().sfm_host_sync_count()) == lib0
    assert len(out["points"]) > 0


@pytest.mark.gpu
def test_a_short_fixed_seed_fuzz_run_finds_no_mismatch(hip):
    import fuzz_mvs_aggregate as fz
    counts, bad, dt = fz.run(20.0, 4242)
    print(f"fuzz_mvs_aggregate: seed 4242, {sum(counts.values())} cases {counts}, {bad} mismatches, {dt:.0f} s")
    assert bad == 0 and all(c > 0 for c in counts.values()), counts


@pytest.mark.gpu
def test_committed_fuzz_logs_are_clean_and_name_this_code(hip):
    """profiles/aggregate_fuzz_seed*.log: no mismatch, and run on the code of csrc/mvs_aggregate.hip that the loaded library was
    built from (scripts/knn_code_hash.py: comments and whitespace do not count)."""
    import glob
    import re
    from sfm_mvs_amd import _lib
    have = _lib.code_hashes_of_binary()
    logs = sorted(glob.glob(os.path.join(ROOT, "profiles", "aggregate_fuzz_seed*.log")))
    assert len(logs) >= 2, logs
    total = 0
    for path in logs:
        text = open(path).read()
        m = re.search(r"fuzz_mvs_aggregate: seed \d+, (\d+) cases .*?, (\d+) mismatches", text)
        assert m and int(m.group(2)) == 0, f"{path}: no clean summary line"
        ids = re.findall(r"sfm_build_id (knn\.hip:\S+(?: \S+:\S+)*)", text)
        assert ids, f"{path} does not name the build it ran on"
        logged = dict(tok.split(":", 1) for tok in ids[-1].split() if ":" in tok)
        for name in ("mvs_aggregate.hip", "common.h"):
            assert logged.get(name) == have[name], f"{path} was produced by another csrc/{name} than the loaded binary's"
        total += int(m.group(1))
    assert total >= 300, total
