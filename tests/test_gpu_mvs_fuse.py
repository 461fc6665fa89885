"""sfm_mvs_fuse on the device (mvs.fuse, run_mvs(fuse=...)): mask, positions, normals, colours and support equal to the float32 restatement
tests/np_mvs_fuse.py word for word (floats as int32 views; a NaN equals a NaN, as in tests/parity_cases.py) on every frame shape, table
and parameter the header admits, through a raw C-ABI call into sentinel-padded buffers; the two identities against a real
sfm_mvs_consistency call; no host wait; run_mvs(fuse=None) the parent's bits; and the end-to-end clouds held to the bars of
tests/golden/mvs_fuse_calibration.json (docs/mvs.md §10)."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

import fuzz_mvs_fuse as fz  # noqa: E402
import mvs_fuse_cases as cases  # noqa: E402
import np_mvs_fuse as nf  # noqa: E402
import parity_cases as pc  # noqa: E402
from fuzz_mvs import IDENTITY  # noqa: E402

F = np.float32
FUZZ_FLOOR = 700                # a tenth of the 7004 cases the two committed logs hold, rounded down to one figure (docs/mvs.md §10)
INF = float("inf")
COS = (-INF, 0.0, fz.COS30, 1.0)


def agree(depth, table, normal=None, bgr=None, tau=0.01, cos_min=-INF, unique=1):
    got, want, bad = fz.fuse_both(depth, table, normal, bgr, tau, cos_min, unique)
    assert bad is None, bad
    return want


def inputs(n, h, w, seed, spread=0.05, slots=8):
    rng = np.random.default_rng(seed)
    return (fz.smooth_maps(rng, n, h, w), fz.random_table(rng, n, slots), fz.unit_normals(rng, n, h, w, spread),
            rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8))


def set_slots(table, i, views, abs_=None, min_consistent=0):
    """View i's neighbour list rewritten in place: `views` with near-identity motions (or the given ab rows)."""
    k = len(views)
    table[i, nf.W_NNBR], table[i, nf.W_MIN] = k, min_consistent
    table[i, nf.W_NBR:nf.W_NBR + 8] = 0
    table[i, nf.W_NBR:nf.W_NBR + k] = views
    ab = np.tile(IDENTITY, (k, 1)) if abs_ is None else np.asarray(abs_, F).reshape(k, 12)
    table.view(F)[i, nf.W_AB:nf.W_AB + 12 * k] = ab.ravel()
    return table


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["1 x 1", "1 x 40", "40 x 1", "15 x 15", "16 x 16", "17 x 33", "33 x 17", "4099 x 2"])
def test_parity_on_frame_shapes(hip, shape):
    """Tile edges in x and y, single rows, columns and pixels, more than one tile a side; normals and colours present and absent, every
    cos_min, both unique settings."""
    w, h = (int(t) for t in shape.split(" x "))
    depth, table, normal, bgr = inputs(3, h, w, 100 + w + 7 * h)
    merged = 0
    for k, (has_n, has_b) in enumerate(((1, 1), (1, 0), (0, 1), (0, 0))):
        for j, cos_min in enumerate(COS):
            want = agree(depth, table, normal if has_n else None, bgr if has_b else None, 0.01, cos_min, (j + k) & 1)
            merged += int((want["support"] > 1).sum())
    if w * h >= 40:
        assert merged > 0                                       # the case merges samples: it is no all-zero parity


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3, 9])
def test_parity_over_views_and_neighbour_lists(hip, n):
    """n = 1 has no possible neighbour; lists of length 0, 1 and 8 (with repeats where n - 1 < 8); a view listed twice; min_consistent 0 and nnbr."""
    depth, table, normal, bgr = inputs(n, 21, 37, n)
    others = lambda i: [v for v in range(n) if v != i]          # noqa: E731
    for length in (0, 1, 8):
        for mc_full in (0, 1):
            for i in range(n):
                row = [others(i)[(i + s) % (n - 1)] for s in range(length)] if n > 1 else []
                set_slots(table, i, row, min_consistent=len(row) if mc_full else 0)
                table.view(F)[i, nf.W_AB:nf.W_AB + 96] += np.random.default_rng(i).normal(0, 1e-4, 96).astype(F) * (np.arange(96) < 12 * len(row))
            for unique in (0, 1):
                want = agree(depth, table, normal, bgr, 0.01, 0.0, unique)
                if n == 1 or length == 0:
                    assert np.all(want["support"][want["mask"] == 1] == 1) and np.array_equal(want["mask"] == 1, depth > 0)
    if n >= 3:
        set_slots(table, 0, [1, 1, 2, 1], min_consistent=2)     # a repeated view counts and is summed each time
        want = agree(depth, table, normal, bgr, 0.02, -INF, 0)
        assert want["support"][0].max() == 5


@pytest.mark.gpu
def test_a_corrupt_table_reads_nothing_out_of_range(hip):
    """Indices -1, n, the view itself and far outside, nnbr 9, huge and negative, min_consistent outside 0..nnbr: the skipped slots
    count nothing, the clamp stops at 8 slots, and the words are the restatement's."""
    n = 3
    depth, table, normal, bgr = inputs(n, 18, 35, 5)
    for i in range(n):
        set_slots(table, i, [-1, n, i, (i + 1) % n, 1 << 30, -(1 << 31), (i + 2) % n, 4096])
    for nnbr, mc in ((9, 0), (1000, 2), ((1 << 31) - 1, 1), (-3, 0), (8, -5), (8, 9), (8, 1 << 30)):
        table[:, nf.W_NNBR], table[:, nf.W_MIN] = nnbr, mc
        table[:, 118:128] = 0x7fc00000                          # the padding words are not read
        want = agree(depth, table, normal, bgr, 0.02, -INF, 0)
        assert want["support"].max() <= 3                       # two real neighbours at most
        if nnbr < 0 or mc > 2:
            assert (want["mask"] == 1).sum() == (0 if mc > 2 else (depth > 0).sum())


@pytest.mark.gpu
def test_planted_depths_and_normals(hip):
    """NaN, inf, negative and zero depths in the reference and the neighbours; NaN, inf and zero normals."""
    depth, table, normal, bgr = inputs(4, 33, 47, 11)
    rng = np.random.default_rng(3)
    bad_depth = pc.plant_specials(depth, rng, fraction=0.04)
    bad_normal = pc.plant_specials(normal, rng, fraction=0.04, values=(np.nan, 0.0, np.inf, -np.inf))
    for d, nm in ((bad_depth, normal), (depth, bad_normal), (bad_depth, bad_normal)):
        for cos_min in COS:
            want = agree(d, table, nm, bgr, 0.02, cos_min, 1)
        assert np.all(want["mask"][~(d > 0)] == 0)
    want = agree(bad_depth, table, None, bgr, 0.02, 0.5, 0)
    assert (want["mask"] == 1).any()
    # a NaN normal fails the product even at cos_min = -inf, so the mask can differ from the one without normals there, and only there
    a = agree(depth, table, bad_normal, None, 0.02, -INF, 0)
    b = agree(depth, table, None, None, 0.02, -INF, 0)
    c = agree(depth, table, normal, None, 0.02, -INF, 0)
    assert pc.same(b["mask"], c["mask"]) and pc.same(b["xyz"], c["xyz"]) and not pc.same(a["support"], b["support"])


@pytest.mark.gpu
def test_tau_zero_and_projections_at_the_frame_edge(hip):
    """Whole-pixel motions over constant depths: tau = 0 keeps exactly equal depths; a shift of one pixel lands the last-but-one column
    (row) exactly on the frame's last one, a shift of half a pixel more leaves the frame at the last column (row)."""
    n, h, w = 2, 19, 23
    depth = np.full((n, h, w), 4.0, F)
    depth[1, :, 5] = F(4.0000005)                               # one column of the neighbour differs in the last bit
    bgr = np.random.default_rng(0).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    table = nf.make_table([[1], [0]], [1, 1], [IDENTITY, IDENTITY], [IDENTITY[None], IDENTITY[None]])
    f = table.view(F)
    for sx, sy in ((1.0, 0.0), (0.0, 1.0), (1.5, 0.0), (0.0, 1.5), (-0.5, -0.5), (-1.0, -1.0), (float(w - 1), float(h - 1)), (float(w), 0.0)):
        f[0, nf.W_AB + 9], f[0, nf.W_AB + 10] = F(4.0 * sx), F(4.0 * sy)            # p = 4 (x + sx, y + sy, 1)
        want = agree(depth, table, None, bgr, 0.0, -INF, 0)
        ys, xs = np.mgrid[0:h, 0:w]
        u, t = np.floor(xs + sx + 0.5), np.floor(ys + sy + 0.5)
        inside = (u >= 0) & (u <= w - 1) & (t >= 0) & (t <= h - 1)
        equal = inside & (depth[1][np.clip(t, 0, h - 1).astype(int), np.clip(u, 0, w - 1).astype(int)] == F(4.0))
        assert np.array_equal(want["mask"][0].astype(bool), equal), (sx, sy)
        assert np.all(want["support"][0][equal] == 2)
    f[0, nf.W_AB + 9], f[0, nf.W_AB + 10] = F(4.0), F(0.0)
    last = agree(depth, table, None, bgr, 0.0, -INF, 0)["mask"][0]
    assert last[:, w - 2].all() and not last[:, w - 1].any()    # x = w-2 lands exactly on the last column; x = w-1 leaves the frame


@pytest.mark.gpu
def test_opposite_normals_and_products_equal_to_the_bound(hip):
    """Opposite normals sum to zero: the pixel's own normal comes back.  A product exactly equal to cos_min passes (>=, not >)."""
    n, h, w = 2, 17, 21
    depth = np.full((n, h, w), 4.0, F)
    normal = np.zeros((n, h, w, 3), F)
    normal[0] = np.array([0.6, 0.0, -0.8], F)
    normal[1, :, :7] = -normal[0, :, :7]                        # product -1 (rounded), sum 0
    normal[1, :, 7:14] = np.array([0.0, 1.0, 0.0], F)           # product exactly 0
    normal[1, :, 14:] = np.array([0.0, 0.6, -0.8], F)           # product 0.64
    table = nf.make_table([[1], [0]], [1, 1], [IDENTITY, IDENTITY], [IDENTITY[None], IDENTITY[None]])
    want = agree(depth, table, normal, None, 0.0, -INF, 0)
    assert (want["mask"] == 1).all() and pc.same(want["normal"][0][:, :7], normal[0][:, :7])     # N = 0: the pixel's own normal
    assert not pc.same(want["normal"][0][:, 7:], normal[0][:, 7:])
    assert np.allclose(np.linalg.norm(want["normal"][0], axis=-1), 1.0, atol=1e-6)
    zero = agree(depth, table, normal, None, 0.0, 0.0, 0)
    assert not zero["mask"][0][:, :7].any() and zero["mask"][0][:, 7:].all()          # 0 >= 0 passes
    axis = np.zeros((n, h, w, 3), F)
    axis[..., 2] = -1.0
    one = agree(depth, table, axis, None, 0.0, 1.0, 0)          # equal unit normals along an axis: the product is exactly 1
    assert (one["mask"] == 1).all() and np.all(one["support"] == 2) and pc.same(one["normal"], axis)
    assert not agree(depth, table, axis, None, 0.0, INF, 0)["mask"].any()


@pytest.mark.gpu
@pytest.mark.parametrize("unique", [0, 1])
def test_identities_against_the_consistency_kernel(hip, unique):
    """A real sfm_mvs_consistency call per view: without normals, and with them at cos_min = -inf, the mask is its mask; where support is
    1 the position is its xyz word."""
    from sfm_mvs_amd import mvs
    n, h, w = 5, 45, 70
    depth, table, normal, bgr = inputs(n, h, w, 21, slots=4)
    table[3, nf.W_MIN] = 0
    ti, tf = nf.words(table)
    d_dev = [pc.up(depth[i]) for i in range(n)]
    plain = agree(depth, table, None, None, 0.01, -INF, unique)
    full = agree(depth, table, normal, bgr, 0.01, -INF, unique)
    ones = 0
    for i in range(n):
        k = int(ti[i, nf.W_NNBR])
        row = [int(v) for v in ti[i, nf.W_NBR:nf.W_NBR + k]]
        mask, xyz = mvs.consistency(d_dev[i], [d_dev[v] for v in row], row, tf[i, nf.W_AB:nf.W_AB + 12 * k].reshape(k, 12), i,
                                    tf[i, nf.W_BC:nf.W_BC + 12], 0.01, int(ti[i, nf.W_MIN]), bool(unique))
        mask, xyz = mask.cpu().numpy(), xyz.cpu().numpy()
        assert np.array_equal(plain["mask"][i], mask) and np.array_equal(full["mask"][i], mask)
        one = plain["support"][i] == 1
        ones += int(one.sum())
        assert pc.same(plain["xyz"][i][one], xyz[one]) and pc.same(full["xyz"][i][one], xyz[one])
    assert ones > 50 and (plain["support"] > 1).sum() > 1000


@pytest.mark.gpu
def test_a_second_run_gives_the_same_bits_and_the_wrapper_is_the_raw_call(hip):
    from sfm_mvs_amd import mvs
    sc = cases.scene("slant")
    rng = np.random.default_rng(0)
    depth = np.stack([(g * (1 + 0.003 * rng.standard_normal(g.shape))).astype(F) for g in sc["gt"]])
    normal = fz.unit_normals(rng, *depth.shape, 0.1)
    bgr = cases.frames("slant")
    table = mvs.fuse_table(sc["K"], sc["P"], sc["nbrs"], cases.MIN_CONSISTENT)
    args = (pc.up(depth), table, pc.up(normal), pc.up(bgr))
    a = mvs.fuse(*args, tau=0.01, max_angle=30, unique=True)
    b = mvs.fuse(*args, tau=0.01, max_angle=30, unique=True)
    assert all(pc.same(a[k].cpu().numpy(), b[k].cpu().numpy()) for k in a)
    want = agree(depth, nf.words(table)[0], normal, bgr, 0.01, float(cases.cos_of(30)), 1)
    for k, kw in (("mask", "mask"), ("xyz", "xyz"), ("normals", "normal"), ("colors", "bgr"), ("support", "support")):
        assert pc.same(a[k].cpu().numpy(), want[kw]), k
    assert (want["support"] > 1).sum() > 10000
    # a table already on the device; absent options change no other output
    c = mvs.fuse(args[0], pc.up(table.view(np.uint8).reshape(len(table), 512)), None, None, 0.01, None, True)
    assert c["normals"] is None and c["colors"] is None
    d = mvs.fuse(*args, tau=0.01, max_angle=None, unique=True)
    assert all(pc.same(c[k].cpu().numpy(), d[k].cpu().numpy()) for k in ("mask", "xyz", "support"))


@pytest.mark.gpu
def test_fuse_never_waits_for_the_host(hip):
    from sfm_mvs_amd import _lib, mvs
    sc = cases.scene("quads")
    depth = pc.up(np.stack([g.astype(F) for g in sc["gt"]]))
    normal = pc.up(fz.unit_normals(np.random.default_rng(0), *depth.shape, 0.1))
    bgr = pc.up(cases.frames("quads"))
    table = mvs.fuse_table(sc["K"], sc["P"], sc["nbrs"], cases.MIN_CONSISTENT)
    mvs.fuse(depth, table, normal, bgr, max_angle=45)
    torch.cuda.synchronize()
    lib0 = int(_lib.lib().sfm_host_sync_count())
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = mvs.fuse(depth, table, normal, bgr, max_angle=45)          # the table goes up pinned and stream-ordered
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert int(_lib.lib().sfm_host_sync_count()) == lib0 and out["mask"].shape == depth.shape


# ---- run_mvs ------------------------------------------------------------------------------------------------------------------------

def _posearr(sc):
    return np.hstack([sc["K"].ravel()] + [p.ravel() for p in sc["P"]])


def _count_waits(fn):
    from sfm_mvs_amd import _lib
    torch.cuda.synchronize()
    lib0 = int(_lib.lib().sfm_host_sync_count())
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            out = fn()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert int(_lib.lib().sfm_host_sync_count()) == lib0
    return out, [str(w.message) for w in caught if "synchroniz" in str(w.message).lower()]


@pytest.mark.gpu
def test_run_mvs_without_fuse_gives_the_parents_bits(hip):
    """fuse=None is the filter: the depth maps, then one sfm_mvs_consistency call per view written out here, the points and colours
    gathered in view order."""
    from sfm_mvs_amd import mvs
    sc = cases.scene("quads")
    posearr = _posearr(sc)
    out = mvs.run_mvs(sc["images"], sc["K"], posearr, sc["cloud"], ndepth=24, fuse=None)
    plain = mvs.run_mvs(sc["images"], sc["K"], posearr, sc["cloud"], ndepth=24)
    assert "support" not in out and "support" not in plain
    assert all(pc.same(a.cpu().numpy(), b.cpu().numpy()) for a, b in zip(out["depths"], plain["depths"]))
    pts, cols = [], []
    for i, nb in enumerate(sc["nbrs"]):
        ab, bc = mvs.consistency_matrices(sc["K"], sc["P"][i], sc["P"][nb])
        mask, xyz = mvs.consistency(out["depths"][i], [out["depths"][v] for v in nb], nb, ab, i, bc, 0.01, 2, True)
        keep = mask.cpu().numpy().astype(bool)
        pts.append(xyz.cpu().numpy()[keep].astype(np.float64))
        cols.append(sc["images"][i][keep].astype(np.float64))
    assert len(out["points"]) > 5000
    assert np.array_equal(out["points"], np.concatenate(pts)) and np.array_equal(out["colors"], np.concatenate(cols))
    assert np.array_equal(plain["points"], out["points"]) and np.array_equal(plain["colors"], out["colors"])


@pytest.mark.gpu
def test_run_mvs_fuse_waits_for_the_host_as_often_as_the_filter(hip):
    """run_mvs waits for the host once, for the fused count that sizes the result, and then downloads once: under torch's sync debug mode
    those are two synchronising operations, with and without refine (tests/test_gpu_mvs.py and tests/test_gpu_mvs_patchmatch.py assert
    the same two of the filter).  With fuse the table goes up pinned and stream-ordered and the one launch waits for nothing, so the
    count is unchanged, and the library itself never waits."""
    from sfm_mvs_amd import mvs
    sc = cases.scene("quads")
    posearr = _posearr(sc)
    opts = dict(ndepth=16, fuse=True)
    mvs.run_mvs(sc["images"], sc["K"], posearr, sc["cloud"], **opts)
    mvs.run_mvs(sc["images"], sc["K"], posearr, sc["cloud"], ndepth=16)
    _, parent_waits = _count_waits(lambda: mvs.run_mvs(sc["images"], sc["K"], posearr, sc["cloud"], ndepth=16))
    out, waits = _count_waits(lambda: mvs.run_mvs(sc["images"], sc["K"], posearr, sc["cloud"], **opts))
    assert len(waits) == len(parent_waits) == 2, (waits, parent_waits)          # the count, then the download
    m = len(out["points"])
    assert m > 1000 and out["points"].shape == (m, 3) and out["points"].dtype == np.float64 and out["colors"].shape == (m, 3)
    assert out["colors"].dtype == np.float64 and out["support"].shape == (m,) and out["support"].dtype == np.uint8
    assert out["support"].min() >= 3 and out["support"].max() <= 5 and "normals" not in out and "normal_maps" not in out
    assert all(d.data_ptr() == out["depths"][0].data_ptr() + 4 * i * d.numel() for i, d in enumerate(out["depths"]))      # views of one stack
    filt = mvs.run_mvs(sc["images"], sc["K"], posearr, sc["cloud"], ndepth=16)
    assert all(pc.same(a.cpu().numpy(), b.cpu().numpy()) for a, b in zip(out["depths"], filt["depths"]))
    assert len(filt["points"]) == m and not np.array_equal(filt["points"], out["points"])          # no normals: the filter's mask
    own = mvs.run_mvs(sc["images"], sc["K"], posearr, sc["cloud"], ndepth=16, fuse=dict(colours=False))
    assert np.array_equal(own["points"], out["points"]) and np.array_equal(own["colors"], filt["colors"])
    ropts = dict(ndepth=16, refine=dict(iters=1), fuse=dict(max_angle=60))
    mvs.run_mvs(sc["images"], sc["K"], posearr, sc["cloud"], **ropts)
    out, waits = _count_waits(lambda: mvs.run_mvs(sc["images"], sc["K"], posearr, sc["cloud"], **ropts))
    assert len(waits) == 2, waits                               # as run_mvs(refine=...) without fuse
    m = len(out["points"])
    assert m > 1000 and out["normals"].shape == (m, 3) and out["normals"].dtype == np.float64 and out["support"].shape == (m,)
    assert np.allclose(np.linalg.norm(out["normals"], axis=1), 1.0, atol=1e-5)
    assert len(out["normal_maps"]) == 5 and all(nm.shape == (cases.H, cases.W, 3) for nm in out["normal_maps"])


@pytest.mark.gpu
def test_run_mvs_fuse_with_a_view_without_sources(hip):
    from sfm_mvs_amd import mvs
    sc = cases.scene("quads")
    rng = [mvs.depth_range(sc["cloud"], sc["P"][i], P_all=sc["P"]) for i in range(5)]
    out = mvs.run_mvs(sc["images"], sc["K"], _posearr(sc), sc["cloud"], ndepth=16, neighbours=[[], [2, 3], [1, 3], [2, 1], []], ranges=rng,
                      refine=dict(iters=0), fuse=True)
    assert not out["depths"][0].any() and not out["normal_maps"][4].any() and len(out["points"]) > 1000
    assert out["support"].min() >= 3 and out["support"].max() <= 3


@pytest.mark.gpu
def test_densify_tracks_forwards_fuse(hip):
    import mvs_plan_cases as mc
    from sfm_mvs_amd import tracks
    imgs, K, P, gt, perm = mc.permuted_scene()
    X, cam_idx, pt_idx = mc.synth_tracks(K, P, gt)
    result = dict(points=X.astype(np.float32), cam_idx=cam_idx, pt_idx=pt_idx)
    out = tracks.densify_tracks(result, imgs, K, P, points=X, nsrc=mc.NSRC, ndepth=16, fuse=True)
    m = len(out["points"])
    assert m > 1000 and out["support"].shape == (m,) and out["support"].dtype == np.uint8 and out["support"].min() >= 2 and "plan" in out


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["quads", "slant"])
def test_run_mvs_fuse_meets_the_calibration_bars(hip, name):
    """run_mvs at its defaults, with fuse=True alone and with refine=True (seed 0): every map is the restatement's of the calibration,
    so the merged clouds are held to the committed rows' bars and to the three fixed conditions of docs/mvs.md §10."""
    from sfm_mvs_amd import mvs
    sc = cases.scene(name)
    doc = cases.golden()
    table = mvs.fuse_table(sc["K"], sc["P"], sc["nbrs"], cases.MIN_CONSISTENT)
    frames = pc.up(cases.frames(name))
    for config, kw, angle in (("sweep", dict(fuse=True), None), ("refine", dict(refine=True, fuse=dict(max_angle=None)), None),
                              ("refine", dict(refine=True, fuse=True), doc["default_max_angle"])):
        out = mvs.run_mvs(sc["images"], sc["K"], _posearr(sc), sc["cloud"], **kw)
        dstack = torch.stack(list(out["depths"]))
        nstack = torch.stack(list(out["normal_maps"])) if config == "refine" else None
        res = mvs.fuse(dstack, table, nstack, frames, cases.TAU, angle, True)
        dev = dict(mask=res["mask"].cpu().numpy(), xyz=res["xyz"].cpu().numpy(), support=res["support"].cpu().numpy(),
                   normal=None if nstack is None else res["normals"].cpu().numpy())
        keep = dev["mask"].astype(bool)
        assert np.array_equal(out["points"], dev["xyz"][keep].astype(np.float64)) and np.array_equal(out["support"], dev["support"][keep])
        assert np.array_equal(out["colors"], res["colors"].cpu().numpy()[keep].astype(np.float64))
        depth = dstack.cpu().numpy()
        normal = None if nstack is None else nstack.cpu().numpy()
        if config == "refine":
            assert np.array_equal(out["normals"], dev["normal"][keep].astype(np.float64))
        filt = cases.filter_cloud(name, depth) if angle is None else cases.own_samples(name, depth)[keep]
        fig = cases.fused_figures(name, normal, dev, filt)
        row = cases.row(doc, name, config, 0, angle)
        print(name, config, angle, fig)
        assert cases.meets(fig, cases.bars(row)) is None, (cases.meets(fig, cases.bars(row)), fig)
        if angle is None and (name, config) in (("quads", "sweep"), ("slant", "refine")):
            assert fig["points"] == fig["filter_points"] and fig["merged"]["median"] < fig["filter"]["median"]
            if name == "slant":
                assert fig["normal_merged_deg"] < fig["normal_reference_deg"]


# ---- fuzzing ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_a_short_fixed_seed_fuzz_run(hip):
    count, bad, dt = fz.run(4.0, 20266, log=print)
    print(f"fuzz_mvs_fuse: {count} cases in {dt:.1f} s")
    assert bad == 0 and count >= 10


@pytest.mark.gpu
def test_committed_fuzz_logs_are_clean_and_of_this_code(hip):
    """profiles/mvs_fuse_fuzz_seed*.log: no mismatch, and run on the code of csrc/mvs_fuse.hip and csrc/common.h that the loaded library
    was built from (scripts/knn_code_hash.py: comments and whitespace do not count)."""
    import glob
    import re
    from sfm_mvs_amd import _lib
    have = _lib.code_hashes_of_binary()
    logs = sorted(glob.glob(os.path.join(ROOT, "profiles", "mvs_fuse_fuzz_seed*.log")))
    assert len(logs) >= 2, logs
    total = 0
    for path in logs:
        text = open(path).read()
        m = re.search(r"fuzz_mvs_fuse: seed \d+, (\d+) cases, (\d+) mismatches", text)
        assert m and int(m.group(2)) == 0, f"{path}: no clean summary line"
        ids = re.findall(r"sfm_build_id (knn\.hip:\S+(?: \S+:\S+)*)", text)
        assert ids, f"{path} does not name the build it ran on"
        logged = dict(tok.split(":", 1) for tok in ids[-1].split() if ":" in tok)
        for fname in ("mvs_fuse.hip", "common.h"):
            assert logged.get(fname) == have[fname], f"{path} was produced by another csrc/{fname} than the loaded binary's"
        total += int(m.group(1))
    assert total >= FUZZ_FLOOR, total
