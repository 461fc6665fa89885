"""sfm_mvs_plane_sweep and sfm_mvs_consistency at the limits of their documented ranges and on degenerate inputs, each case
compared with tests/np_mvs.py bit for bit (parity_cases.same: int32 views; a NaN equals a NaN) AND shown, on the restatement's
output, to exercise what it is named for: top-k beyond 2, 129..1024 planes, winners on the first and the last plane, frames from
one interior pixel to several thousand pixels by 2r+1, sources behind the planes, non-finite matrices, flat frames, exact ties,
every kind of cost_max, and the consistency filter on planted NaN / inf / negative depths.  docs/mvs.md, "Limits and fuzzing".

The whole file takes 19 s on the GPU box (69 cases), nearly all of it the NumPy side."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import np_mvs  # noqa: E402
import parity_cases as pc  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
W, H, VAR_MIN = 157, 93, 150.0
MIN_DEPTH_FRACTION = 0.3          # interior pixels with depth > 0 where depths are expected (the bar of tests/test_gpu_mvs.py)


def scene_views(nsrc, ref=4):
    """The 9-view arc scene of tests/test_gpu_mvs.py: the reference's gray frame, its `nsrc` sequence neighbours, their matrices."""
    from sfm_mvs_amd import mvs
    grays, K, P, _, _ = pc.scene(n=9, w=W, h=H, seed=3, arc=0.3)
    nb = mvs.neighbours(ref, 9, nsrc)
    return grays[ref], [grays[v] for v in nb], mvs.sweep_matrices(K, P[ref], P[nb])


def planes(dmin, dmax, nd):
    from sfm_mvs_amd import mvs
    return mvs._inverse_depths_host(dmin, dmax, nd)


def depth_fraction(want, r):
    return float((pc.interior(want[0], r) > 0).mean())


def check(ref, srcs, mv, invd, r, topk, var_min, cost_max):
    want, bad = pc.sweep_both(ref, srcs, mv, invd, r, topk, var_min, cost_max)
    assert bad is None, f"{bad} differs from np_mvs"
    return want


@pytest.mark.parametrize("nsrc,topk", [(8, 3), (8, 5), (8, 8), (3, 3), (4, 4)])
def test_topk_beyond_two(hip, nsrc, topk):
    """Slots 2..7 of the sorted list are summed: on some plane more than half of the interior pixels have `topk` pairwise
    different smallest per-source costs, so that a list keeping fewer entries, or out of order, changes the mean."""
    ref, srcs, mv = scene_views(nsrc)
    invd = planes(1.0, 13.5, 9)
    costs = np.sort(pc.per_source_costs(ref, srcs, mv, invd, 3, VAR_MIN), axis=0)[:topk]
    distinct = np.all(np.diff(costs, axis=0) > 0, axis=0).reshape(len(invd), -1).mean(1)
    assert distinct.max() > 0.5, distinct
    want = check(ref, srcs, mv, invd, 3, topk, VAR_MIN, 0.4)
    assert depth_fraction(want, 3) >= MIN_DEPTH_FRACTION, depth_fraction(want, 3)


@pytest.mark.parametrize("ndepth", [129, 512, 1024])
def test_plane_counts_up_to_the_limit(hip, ndepth):
    ref, srcs, mv = scene_views(2)
    want = check(ref, srcs, mv, planes(2.0, 13.5, ndepth), 3, 2, VAR_MIN, 0.4)
    assert depth_fraction(want, 3) >= MIN_DEPTH_FRACTION
    assert len(np.unique(want[2])) > ndepth // 8                      # winners spread over the range ...
    assert ndepth == 129 or want[2].max() > 128                       # ... beyond any plane count the other tests use ...
    assert (pc.interior(want[3][-1], 3) < 2).mean() > 0.3             # ... and the last plane's costs are real ones


@pytest.mark.parametrize("dmin,dmax,end", [(4.6, 13.5, "last"), (1.0, 4.2, "first")])
def test_winner_on_an_end_plane_skips_the_parabola(hip, dmin, dmax, end):
    """The plane range stops inside the scene (surfaces between 3 and 6 units): pixels whose surface lies beyond the range win on
    its end plane and take that plane's depth as it is."""
    ref, srcs, mv = scene_views(4)
    invd = planes(dmin, dmax, 24)
    want = check(ref, srcs, mv, invd, 3, 2, VAR_MIN, 0.4)
    j = len(invd) - 1 if end == "last" else 0
    at_end = (want[2] == j) & (want[0] > 0)
    assert at_end.sum() >= 100, int(at_end.sum())
    assert np.all(want[0][at_end] == F(1) / invd[j])


FRAMES = [("min", "min"), ("min", 40), (15, 15), (16, 16), (17, 33), (160, 16), (4099, "min")]


@pytest.mark.parametrize("r", [1, 4])
@pytest.mark.parametrize("w,h", FRAMES)
def test_frame_sizes_around_the_tile(hip, w, h, r):
    """Frames below, at and just above the 16 x 16 tile, down to one interior pixel, and a long thin one.  With both sides >= 15
    the frame is a crop of the rendered scene about its centre (the principal point shifted with it) and its real matrices; a
    frame with a side of 2r+1 has a single interior row or column, which no real camera pair warps into itself: there the crop is
    compared as it is and depths are asked of a second pair, rectified by hand (parity_cases.rectified_pair)."""
    from sfm_mvs_amd import mvs
    w, h = (2 * r + 1 if v == "min" else v for v in (w, h))
    big_w, big_h = (4099, 9) if w > 192 else (192, 93)
    grays, K, P, _, _ = pc.scene(n=9, w=big_w, h=big_h, seed=3, arc=0.3)
    g, Kc, Pc = pc.crop(grays, K, P, (big_w - w) // 2, (big_h - h) // 2, w, h)
    nb = mvs.neighbours(4, 9, 2)
    cases = [(g[4], [g[v] for v in nb], mvs.sweep_matrices(Kc, Pc[4], Pc[nb]), planes(1.0, 13.5, 17), 2, min(w, h) >= 15)]
    if min(w, h) < 15:
        ref, src, mv, invd = pc.rectified_pair(w, h, r, 17, seed=w + h + r)
        cases.append((ref, [src], mv, invd, 1, True))
    for ref, srcs, mv, invd, topk, depths_expected in cases:
        want = check(ref, srcs, mv, invd, r, topk, 50.0, 0.4)
        assert want[0].shape == (h, w)
        if depths_expected:
            assert depth_fraction(want, r) >= MIN_DEPTH_FRACTION, depth_fraction(want, r)
        edge = np.ones((h, w), bool)
        edge[r:h - r, r:w - r] = False
        assert np.all(want[0][edge] == 0) and np.all(want[1][edge] == 2)


def test_a_source_behind_every_plane(hip):
    """One of four sources has its matrix negated (h2 < 0 everywhere): it costs 2 on every plane, the other three still give depths."""
    ref, srcs, mv = scene_views(4)
    invd = planes(1.0, 13.5, 17)
    mv = mv.copy()
    mv[1] = -mv[1]
    assert all((pc.h2_of(mv[1], q, W, H) < 0).all() for q in invd)
    assert np.all(pc.per_source_costs(ref, srcs[1:2], mv[1:2], invd, 2, VAR_MIN) == 2)
    want = check(ref, srcs, mv, invd, 2, 3, VAR_MIN, 0.4)
    assert depth_fraction(want, 2) >= MIN_DEPTH_FRACTION


def test_h2_changes_sign_across_the_frame(hip):
    """v_2 = -M_22 / invd[j0]: on plane j0 the third coordinate is what the two small perspective terms leave, negative on one part
    of the frame, positive and tiny (px, py huge or inf) on the other; the planes before j0 lie in front, those after it behind."""
    ref, srcs, mv = scene_views(2)
    invd = planes(1.0, 13.5, 17)
    mv = mv.copy()
    mv[0, 6], mv[0, 7] = F(1e-3), F(-2e-3)
    mv[0, 11] = -(mv[0, 8] + F(0.05)) / invd[8]
    h2 = pc.h2_of(mv[0], invd[8], W, H)
    assert (h2 > 0).mean() > 0.1 and (h2 <= 0).mean() > 0.1
    assert (pc.h2_of(mv[0], invd[0], W, H) > 0).all() and (pc.h2_of(mv[0], invd[-1], W, H) < 0).all()
    want = check(ref, srcs, mv, invd, 2, 1, VAR_MIN, 0.4)
    assert depth_fraction(want, 2) >= MIN_DEPTH_FRACTION                # from the untouched source


def test_tiny_h2_overflows_the_pixel_coordinates(hip):
    """M = diag(1, 1, 2e-38), v = 0: px = x / 2e-38 is inf for every x >= 7 and 0 at x = 0: only pixel (0, 0) warps into the frame."""
    ref, srcs, _ = scene_views(1)
    mv = np.array([[1, 0, 0, 0, 1, 0, 0, 0, 2e-38, 0, 0, 0]], F)
    with np.errstate(all="ignore"):
        valid = np_mvs.warp(srcs[0], mv[0], F(0.3), W, H)[1]
        assert np.isinf(F(7) / mv[0, 8])
    assert valid[0, 0] and valid.sum() == 1
    want = check(ref, srcs, mv, planes(1.0, 13.5, 5), 1, 1, VAR_MIN, 0.4)
    assert np.all(want[0] == 0) and np.all(want[3] == 2)


@pytest.mark.parametrize("same_frame", [True, False])
def test_identity_warp_reaches_the_last_column_and_row_and_ties_every_plane(hip, same_frame):
    """M = identity, v = 0: px = x and py = y exactly, so the last column has px == w-1 and the last row py == h-1 (x0 = w-2 with
    fx = 1): valid, and the warped frame is the source itself.  Every plane costs the same: the first one wins."""
    ref, srcs, _ = scene_views(1)
    src = ref if same_frame else srcs[0]
    mv = np.array([[1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]], F)
    invd = planes(1.0, 13.5, 7)
    val, valid = np_mvs.warp(src, mv[0], invd[3], W, H)
    assert valid.all() and np.array_equal(val, src.astype(F) - F(128))
    want = check(ref, [src], mv, invd, 3, 1, VAR_MIN, 2.5)
    inner = pc.interior(want[1], 3)
    assert np.all(want[2] == 0) and np.all(want[3] == want[3][0]) and (inner[:, -1] < 2).mean() > 0.5 and (inner[-1, :] < 2).mean() > 0.5
    assert np.all(pc.interior(want[0], 3) == F(1) / invd[0])
    if same_frame:
        assert (inner == 0).mean() > 0.9


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("where", ["row0", "row2", "v", "all"])
def test_non_finite_matrix_entries(hip, value, where):
    ref, srcs, mv = scene_views(3)
    mv = mv.copy()
    mv[2, {"row0": slice(0, 3), "row2": slice(6, 9), "v": slice(9, 12), "all": slice(0, 12)}[where]] = value
    want = check(ref, srcs, mv, planes(1.0, 13.5, 17), 2, 2, VAR_MIN, 0.4)
    assert np.all(pc.per_source_costs(ref, srcs[2:], mv[2:], planes(1.0, 13.5, 17), 2, VAR_MIN) == 2)   # that source never counts
    assert depth_fraction(want, 2) >= MIN_DEPTH_FRACTION


@pytest.mark.parametrize("level", [0, 128, 255])
def test_flat_frames_have_no_depth(hip, level):
    """Every variance is 0 < var_min: every cost 2, plane 0, depth 0, at every pixel."""
    _, _, mv = scene_views(4)
    flat = np.full((H, W), level, np.uint8)
    want = check(flat, [flat.copy() for _ in range(4)], mv, planes(1.0, 13.5, 9), 3, 2, VAR_MIN, 2.0)
    assert np.all(want[0] == 0) and np.all(want[1] == 2) and np.all(want[2] == 0) and np.all(want[3] == 2)


@pytest.mark.parametrize("flat_side", ["reference", "sources"])
def test_one_flat_side_has_no_depth(hip, flat_side):
    ref, srcs, mv = scene_views(2)
    flat = np.full((H, W), 255, np.uint8)
    if flat_side == "reference":
        ref = flat
    else:
        srcs = [flat, flat]
    want = check(ref, srcs, mv, planes(1.0, 13.5, 9), 3, 2, VAR_MIN, 0.4)
    assert np.all(want[0] == 0) and np.all(want[1] == 2) and np.all(want[2] == 0)


def test_checkerboard_of_0_and_255(hip):
    """Saturated one-pixel squares in every frame: the largest moments the format allows, and costs that tie across planes."""
    _, _, mv = scene_views(4)
    ys, xs = np.mgrid[0:H, 0:W]
    board = (((xs + ys) & 1) * 255).astype(np.uint8)
    want = check(board, [board] * 4, mv, planes(1.0, 13.5, 17), 3, 2, VAR_MIN, 0.4)
    inner = pc.interior(want[3], 3)
    assert (inner < 2).mean() > 0.3 and len(np.unique(inner)) > 100


@pytest.mark.parametrize("topk", [1, 5, 8])
def test_one_source_passed_eight_times(hip, topk):
    """Eight equal costs in the list: the mean of any top k equals the cost itself, up to the rounding of the sum."""
    ref, srcs, mv = scene_views(1)
    invd = planes(1.0, 13.5, 17)
    want = check(ref, srcs * 8, np.repeat(mv, 8, 0), invd, 3, topk, VAR_MIN, 0.4)
    one = pc.per_source_costs(ref, srcs, mv, invd, 3, VAR_MIN)[0]
    assert np.allclose(pc.interior(want[3], 3), one, rtol=1e-6, atol=0)
    assert depth_fraction(want, 3) >= MIN_DEPTH_FRACTION


@pytest.mark.parametrize("cost_max", [-1.0, 0.0, 0.4, 2.0, 2.5, np.inf, -np.inf])
def test_every_kind_of_cost_max(hip, cost_max):
    ref, srcs, mv = scene_views(2)
    want = check(ref, srcs, mv, planes(1.0, 13.5, 17), 3, 2, 4000.0, cost_max)    # (var_min 4000: weak windows have no valid source)
    depth, cost = pc.interior(want[0], 3), pc.interior(want[1], 3)
    assert (cost < 0.4).mean() >= MIN_DEPTH_FRACTION and (cost == 2).mean() > 0.05 and ((cost >= 0.4) & (cost < 2)).mean() > 0.02
    assert np.array_equal(depth > 0, cost < F(cost_max))
    if cost_max <= 0:
        assert np.all(want[0] == 0)
    if cost_max > 2:
        assert np.all(depth > 0)


# ---- consistency -------------------------------------------------------------------------------------------------------------
def swept_depths():
    """Depth maps of the five-view scene from the restatement's sweep (17 planes, r = 2), and the cameras."""
    from sfm_mvs_amd import mvs
    if not hasattr(swept_depths, "out"):
        grays, K, P, _, _ = pc.scene(n=5, w=W, h=H, seed=5, arc=0.5)
        invd = planes(2.0, 8.0, 32)
        depths = []
        for i in range(5):
            nb = mvs.neighbours(i, 5, 2)
            depths.append(np_mvs.plane_sweep(grays[i], [grays[v] for v in nb], mvs.sweep_matrices(K, P[i], P[nb]), invd, 2, 2, VAR_MIN, 0.4)[0])
        swept_depths.out = depths, K, P
    return swept_depths.out


def consistency_case(i, nb, rng=None, **kw):
    from sfm_mvs_amd import mvs
    depths, K, P = swept_depths()
    ab, bc = mvs.consistency_matrices(K, P[i], P[nb]) if len(nb) else (np.zeros((0, 12), F), mvs.consistency_matrices(K, P[i], P[:1])[1])
    ds = list(depths) if rng is None else [pc.plant_specials(d, rng) for d in depths]
    args = dict(tau=0.01, min_consistent=min(2, len(nb)), unique=True)
    args.update(kw)
    ab = args.pop("ab", ab)
    want, bad = pc.consistency_both(ds[i], [ds[v] for v in nb], nb, ab, args.pop("ref_index", i), bc, **args)
    assert bad is None, f"{bad} differs from np_mvs"
    return want, ds[i]


def test_consistency_without_neighbours(hip):
    """nview = 0 (and so min_consistent = 0): every pixel with a depth is kept, with its world point."""
    (mask, xyz), d = consistency_case(2, [])
    assert np.array_equal(mask == 1, d > 0) and 0.3 < mask.mean() < 1.0 and np.all(xyz[mask == 0] == 0) and np.any(xyz[mask == 1] != 0)


def test_consistency_min_consistent_zero_keeps_unseen_pixels(hip):
    (m0, _), d = consistency_case(2, [1, 3], min_consistent=0, unique=False)
    (m1, _), _ = consistency_case(2, [1, 3], min_consistent=1, unique=False)
    assert np.array_equal(m0 == 1, d > 0) and 0 < m1.sum() < m0.sum()          # some pixels have no consistent neighbour and stay


@pytest.mark.parametrize("min_consistent,unique,tau", [(0, False, 0.01), (1, True, 0.01), (2, False, 0.05), (2, True, 0.0)])
def test_consistency_on_planted_special_depths(hip, min_consistent, unique, tau):
    """NaN, +-inf, negative and zero depths at random pixels of the reference AND the neighbours' maps."""
    rng = np.random.default_rng(17)
    kept = 0
    for i in range(5):
        from sfm_mvs_amd import mvs
        (mask, xyz), d = consistency_case(i, mvs.neighbours(i, 5, 3), rng=rng, min_consistent=min_consistent, unique=unique, tau=tau)
        for kind in (np.isnan(d), np.isposinf(d), np.isneginf(d), d < 0, d == 0):
            assert kind.sum() > 50
        assert not mask[np.isnan(d) | ~(d > 0)].any()
        if min_consistent == 0:
            assert mask[np.isposinf(d)].all() and not np.isfinite(xyz[np.isposinf(d)]).all()
        kept += int(mask.sum())
    assert (kept > 0.05 * 5 * W * H) == (tau > 0), kept


def test_consistency_tau_zero_needs_equal_depths(hip):
    """tau = 0 on real maps keeps next to nothing; on a neighbour that holds exactly the depth the reference predicts, everything."""
    (mask, _), _ = consistency_case(2, [1, 3], tau=0.0, min_consistent=1)
    assert mask.mean() < 0.01
    d = np.full((H, W), 2.5, F)
    eye = np.array([[1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]], F)
    want, bad = pc.consistency_both(d, [d.copy()], [0], eye, 1, eye[0], 0.0, 1, False)
    assert bad is None and want[0].all()


def test_consistency_one_pixel_frame(hip):
    eye = np.array([[1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]], F)
    for dref, dnbr, keep in ((2.0, 2.0, 1), (2.0, 2.5, 0), (0.0, 2.0, 0), (np.nan, 2.0, 0), (2.0, np.nan, 0)):
        want, bad = pc.consistency_both(np.array([[dref]], F), [np.array([[dnbr]], F)], [0], eye, 1, eye[0] * F(3), 0.01, 1, False)
        assert bad is None and want[0].shape == (1, 1) and int(want[0][0, 0]) == keep, (dref, dnbr)
        assert keep == 0 or np.array_equal(want[1][0, 0], [0, 0, 6])


def test_consistency_repeated_neighbour_counts_twice(hip):
    (m1, _), _ = consistency_case(2, [1], min_consistent=1, unique=False)
    (m2, _), _ = consistency_case(2, [1, 1], min_consistent=2, unique=False)
    (m3, _), _ = consistency_case(2, [1, 3], min_consistent=2, unique=False)
    assert np.array_equal(m1, m2) and m1.sum() > 1000 and not np.array_equal(m2, m3)


def test_consistency_neighbour_with_the_reference_index(hip):
    """The view itself as its neighbour (identity motion): consistent wherever it has a depth, never 'lower', so unique keeps it."""
    (mask, _), d = consistency_case(2, [2], min_consistent=1, unique=True)
    assert np.array_equal(mask == 1, d > 0) and mask.sum() > 1000
    (lower, _), _ = consistency_case(2, [2], min_consistent=1, unique=True, ref_index=3)      # the same pixels seen from "below"
    assert not lower.any()


def test_consistency_neighbour_behind_the_reference(hip):
    """A neighbour whose third row is negated has p2 <= 0 for every pixel: never consistent; one with p2 of both signs is compared too."""
    from sfm_mvs_amd import mvs
    depths, K, P = swept_depths()
    ab, _ = mvs.consistency_matrices(K, P[2], P[[1, 3]])
    neg = ab.copy()
    neg[0, 6:9], neg[0, 11] = -neg[0, 6:9], -neg[0, 11]
    (m_neg, _), _ = consistency_case(2, [1, 3], ab=neg, min_consistent=1, unique=False)
    (m_one, _), _ = consistency_case(2, [3], min_consistent=1, unique=False)
    assert np.array_equal(m_neg, m_one) and m_one.sum() > 1000
    mixed = ab.copy()
    mixed[0, 11] = F(-4.0)                              # p2 = d * (~1) - 4: negative for the near half of the depths
    (m_mix, _), d = consistency_case(2, [1, 3], ab=mixed, min_consistent=1, unique=False)
    xs, ys = np.meshgrid(np.arange(W, dtype=F), np.arange(H, dtype=F))
    p2 = d * ((mixed[0, 6] * xs + mixed[0, 7] * ys) + mixed[0, 8]) + mixed[0, 11]
    assert ((p2 <= 0) & (d > 0)).sum() > 500 and ((p2 > 0) & (d > 0)).sum() > 500 and m_mix.sum() > 1000


def test_randomised_parity_sweep(hip):
    """A few seconds of scripts/fuzz_mvs.py (sweep, consistency, run_mvs families; the script exits non-zero on a mismatch)."""
    root = os.path.dirname(HERE)
    r = subprocess.run([sys.executable, os.path.join(root, "scripts", "fuzz_mvs.py"), "8", "7"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert " 0 mismatches" in r.stdout
