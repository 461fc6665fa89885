"""The MVS-PLAN family without a GPU (include/sfm_hip.h, "MVS-PLAN"; docs/mvs.md §8): the C-ABI declares, binds, documents and validates
the entry points; the restatement tests/np_mvs_plan.py stands apart from the product and gives hand-checked results; host_plan's pooling
rule; run_mvs's validation of its new keywords; and the calibration of docs/mvs.md §8.4 on the restatement."""
import ast
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import mvs_plan_cases as mc  # noqa: E402
import np_mvs_plan as npl  # noqa: E402

NEW_SYMBOLS = ("sfm_view_pair_counts", "sfm_view_depth_ranges", "sfm_view_select")

# Measured here with the restatement and np_mvs (docs/mvs.md §8.4; scripts/calibrate_mvs_plan.py) on the scene of mvs_plan_cases (9 views on
# an arc of 0.9 rad, frames permuted with default_rng(1), 4 sources, 64 planes), at the arc's middle view: planned sources and range
# 98.76 % of the interior pixels valid, 91.25 % of those within 1 %, 9.88 % of the interior pixels wrong or empty; sequence neighbours and
# mvs.depth_range on the same frames 87.62 %, 75.22 %, 34.09 %: r = 0.0988 / 0.3409 = 0.290.  The bar is (1 + r) / 2.
PLAN_RATIO = 0.290
PLAN_BAR = (1.0 + PLAN_RATIO) / 2.0
# The share of the ground-truth depths of every view that the planned range covers on that scene: 100 % (as mvs.depth_range's does: every
# camera of the arc sees the whole scene).  The margin of half the distance to 100 % is therefore zero.
RANGE_COVERAGE = 1.0


def test_header_declares_binds_and_documents_the_entry_points():
    from sfm_mvs_amd import _lib
    from test_abi import declared_symbols
    syms = declared_symbols()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    doc = open(os.path.join(ROOT, "docs", "mvs.md")).read()
    header = open(os.path.join(ROOT, "include", "sfm_hip.h")).read()
    assert "MVS-PLAN" in header and "NO FLOATING-POINT ATOMICS" in header and "SFM_PLAN_LDS_CAMS 96" in header
    for s in NEW_SYMBOLS:
        assert s in syms and s in _lib.SIGNATURES and hasattr(handle, s), s
        assert s in doc, f"docs/mvs.md does not mention {s}"
    assert _lib.lib().sfm_abi_version() == 3 and _lib.ABI_VERSION == 3
    assert "mvs_plan.hip" in _lib.code_hashes_of_binary()
    src = open(os.path.join(ROOT, "sfm_mvs_amd", "csrc", "mvs_plan.hip")).read()
    assert "unsafeAtomic" not in src and "hipStreamSynchronize" not in src and "stream_sync" not in src    # integer atomics, no host wait


def test_python_layer_exposes_the_entry_points():
    import inspect
    from sfm_mvs_amd import mvs, mvs_plan, tracks
    sig = inspect.signature(mvs_plan.plan_views).parameters
    assert list(sig) == ["pl", "X", "P", "nsrc", "min_angle_deg", "max_angle_deg", "min_good", "lo", "hi"]
    assert [sig[k].default for k in ("nsrc", "lo", "hi")] == [4, 2, 98]
    for name in ("pair_counts", "depth_ranges", "select", "host_plan", "pooled_ranges", "cos_window"):
        assert callable(getattr(mvs_plan, name)), name
    run = inspect.signature(mvs.run_mvs).parameters
    assert run["neighbours"].default is None and run["ranges"].default is None
    assert list(inspect.signature(tracks.densify_tracks).parameters)[:4] == ["result", "images", "K", "P"]
    assert mvs_plan.MAX_SRC == mvs.MAX_VIEWS == 8
    lo, hi = mvs_plan.cos_window(1.0, 30.0)
    assert lo == float(np.cos(np.deg2rad(30.0))) and hi == float(np.cos(np.deg2rad(1.0)))
    with pytest.raises(mvs_plan.SfmHipError):
        mvs_plan.cos_window(30.0, 1.0)


def test_argument_errors_are_reported_before_the_device():
    """Every argument error of the header: a negative status with its message, before any device call (the pointers are never read)."""
    from sfm_mvs_amd import _lib
    L = _lib.lib()
    f = [ctypes.c_void_p(256 * (k + 1)) for k in range(16)]
    big, nan = 1 << 31, float("nan")

    def pairs(to=f[0], ci=f[1], X=f[2], npt=10, nobs=30, P=f[3], ncam=4, lo=0.5, hi=1.0, C=f[4], sh=f[5], gd=f[6]):
        return L.sfm_view_pair_counts(to, ci, X, npt, nobs, P, ncam, lo, hi, C, sh, gd, None)

    def ranges(co=f[0], cob=f[1], ci=f[2], pi=f[3], nobs=30, X=f[4], npt=10, P=f[5], ncam=4, lo=20, hi=980, m=f[6], a=f[7], b=f[8]):
        return L.sfm_view_depth_ranges(co, cob, ci, pi, nobs, X, npt, P, ncam, lo, hi, m, a, b, None)

    def select(sh=f[0], gd=f[1], ncam=4, nsrc=4, min_good=1, nbr=f[2], cnt=f[3]):
        return L.sfm_view_select(sh, gd, ncam, nsrc, min_good, nbr, cnt, None)

    sizes = [dict(ncam=0), dict(ncam=4097), dict(npt=-1), dict(npt=big), dict(nobs=-1), dict(nobs=big)]
    cases = [(call, kw, b"sizes") for call in (pairs, ranges) for kw in sizes] + [(select, dict(ncam=0), b"sizes"), (select, dict(ncam=4097), b"sizes")]
    cases += [(pairs, dict(lo=nan), b"NaN"), (pairs, dict(hi=nan), b"NaN")]
    cases += [(pairs, {k: None}, b"null") for k in ("to", "ci", "X", "P", "C", "sh", "gd")]
    cases += [(pairs, dict(nobs=0, to=None), b"null"), (pairs, dict(npt=0, nobs=0, P=None), b"null")]
    cases += [(ranges, dict(lo=-1), b"permille"), (ranges, dict(hi=1001), b"permille"), (ranges, dict(lo=600, hi=500), b"permille")]
    cases += [(ranges, {k: None}, b"null") for k in ("co", "cob", "ci", "pi", "X", "P", "m", "a", "b")]
    cases += [(ranges, dict(nobs=0, co=None), b"null")]
    cases += [(select, dict(nsrc=0), b"nsrc"), (select, dict(nsrc=9), b"nsrc"), (select, dict(min_good=-1), b"min_good")]
    cases += [(select, {k: None}, b"null") for k in ("sh", "gd", "nbr", "cnt")]
    for call, kw, msg in cases:
        assert call(**kw) == -1, (call.__name__, kw)
        assert msg in L.sfm_last_error(), (call.__name__, kw, L.sfm_last_error())


def test_the_restatement_imports_only_numpy():
    tree = ast.parse(open(os.path.join(ROOT, "tests", "np_mvs_plan.py")).read())
    for node in ast.walk(tree):
        names = [a.name for a in node.names] if isinstance(node, ast.Import) else [node.module or ""] if isinstance(node, ast.ImportFrom) else []
        assert names in ([], ["numpy"]), names


# ---- hand-checked cases on the restatement ---------------------------------------------------------------------------------------

def _counts(cam_idx, lengths, X, C, ncam, lo, hi):
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    return npl.pair_counts(off, np.asarray(cam_idx, np.int32), np.asarray(X, np.float64), np.asarray(C, np.float64), ncam, lo, hi)


def test_two_cameras_at_right_angles():
    C = [[1.0, 0, 0], [0, 1.0, 0]]                                          # the rays from the origin: (-1, 0, 0) and (0, -1, 0), c = 0
    for lo, hi, want in ((-0.5, 0.5, 1), (0.0, 0.5, 1), (-0.5, 0.0, 1), (0.1, 1.0, 0), (-1.0, -0.1, 0)):
        shared, good = _counts([0, 1], [2], [[0.0, 0, 0]], C, 2, lo, hi)
        assert shared.tolist() == [[0, 1], [1, 0]] and good.tolist() == [[0, want], [want, 0]], (lo, hi)


def test_a_cosine_equal_to_either_bound_counts():
    C = np.array([[4.0, 0.5, -1.0], [-2.0, 3.0, 0.25]])
    X = np.array([0.3, -0.2, 0.9])
    r, s = X - C[0], X - C[1]
    n_r, n_s = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2], (s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]
    c = ((r[0] * s[0] + r[1] * s[1]) + r[2] * s[2]) / np.sqrt(n_r * n_s)
    assert _counts([0, 1], [2], [X], C, 2, c, 1.0)[1][0, 1] == 1 and _counts([0, 1], [2], [X], C, 2, -1.0, c)[1][0, 1] == 1
    assert _counts([0, 1], [2], [X], C, 2, c, c)[1][0, 1] == 1
    assert _counts([0, 1], [2], [X], C, 2, np.nextafter(c, 2.0), 1.0)[1][0, 1] == 0 and _counts([0, 1], [2], [X], C, 2, -1.0, np.nextafter(c, -2.0))[1][0, 1] == 0


def test_a_track_naming_a_camera_twice_and_a_point_at_a_centre():
    C = [[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]]
    shared, good = _counts([0, 0, 1], [3], [[0.0, 0, 0]], C, 3, -1.0, 1.0)  # pairs (0, 0): nothing; (0, 1) twice
    assert shared.tolist() == [[0, 2, 0], [2, 0, 0], [0, 0, 0]] and np.array_equal(good, shared)
    shared, good = _counts([0, 1], [2], [[1.0, 0, 0]], C, 3, -1.0, 1.0)     # the point at centre 0: a zero ray, c = 0 / 0
    assert shared[0, 1] == 1 and good[0, 1] == 0
    shared, good = _counts([0, 1, -1, 3, 2 ** 31 - 1], [5], [[0.0, 0, 0]], C, 3, -1.0, 1.0)   # cameras out of range take part in no pair
    assert shared.sum() == 2 and shared[0, 1] == 1
    shared, good = _counts([0, 1], [2], [[np.inf, 0, 0]], C, 3, -1.0, 1.0)
    assert shared[0, 1] == 1 and good[0, 1] == 0


def test_order_statistics_by_hand():
    z = np.array([5, 1, 4, 2, 3, 7, 6, 8], np.float32)
    assert npl.order_statistics(z[:0], 20, 980) == (0, 0, 0)
    assert npl.order_statistics(z[:1], 0, 1000) == (1, 5, 5) and npl.order_statistics(z[:1], 500, 500) == (1, 5, 5)
    assert npl.order_statistics(z[:2], 0, 1000) == (2, 1, 5) and npl.order_statistics(z[:2], 500, 500) == (2, 1, 5)     # floor 0.5 = 0, ceil 0.5 = 1
    assert npl.order_statistics(z[:2], 20, 980) == (2, 1, 5)
    assert npl.order_statistics(z[:7], 0, 1000) == (7, 1, 7) and npl.order_statistics(z[:7], 500, 500) == (7, 4, 4)     # rank 3 of 1..7
    assert npl.order_statistics(z[:7], 20, 980) == (7, 1, 7) and npl.order_statistics(z[:7], 200, 800) == (7, 2, 6)     # floor 1.2, ceil 4.8
    assert npl.order_statistics(z, 0, 1000) == (8, 1, 8) and npl.order_statistics(z, 500, 500) == (8, 4, 5)             # floor 3.5, ceil 3.5
    assert npl.order_statistics(z, 1000, 1000) == (8, 8, 8) and npl.order_statistics(z, 0, 0) == (8, 1, 1)
    assert npl.order_statistics(np.full(9, 2.5, np.float32), 20, 980) == (9, 2.5, 2.5)
    # through the camera-side CSR: camera 1 sees points 0 and 2 at depths 3 and 5 (P's third row (0, 0, 1, 0)); point 1 lies behind it
    P = np.zeros((2, 12)); P[:, 10] = 1.0
    X = np.array([[0, 0, 3.0], [0, 0, -1.0], [0, 0, 5.0]])
    cam_idx, pt_idx = np.array([1, 1, 1], np.int32), np.array([0, 1, 2], np.int32)
    cam_off, cam_obs = npl.csr(cam_idx, 2)
    m, a, b = npl.depth_ranges(cam_off, cam_obs, cam_idx, pt_idx, X, P, 0, 1000)
    assert m.tolist() == [0, 2] and a.tolist() == [0, 3] and b.tolist() == [0, 5]


def test_select_by_hand():
    good = np.array([[0, 5, 5, 5, 1], [5, 0, 0, 0, 0], [5, 0, 0, 9, 0], [5, 0, 9, 0, 0], [1, 0, 0, 0, 0]])
    shared = np.array([[0, 7, 9, 7, 1], [7, 0, 0, 0, 0], [9, 0, 0, 9, 0], [7, 0, 9, 0, 0], [1, 0, 0, 0, 0]])
    nbr, cnt = npl.select(shared, good, 3, 1)
    assert nbr[0].tolist() == [2, 1, 3]                                     # good ties: shared 9 first, then the lower index of the two 7s
    assert nbr[1].tolist() == [0, -1, -1] and cnt.tolist() == [3, 1, 2, 2, 1] and nbr[2].tolist() == [3, 0, -1]
    nbr, cnt = npl.select(shared, good, 2, 5)
    assert nbr[0].tolist() == [2, 1] and nbr[4].tolist() == [-1, -1] and cnt[4] == 0
    nbr, cnt = npl.select(np.zeros((1, 1)), np.zeros((1, 1)), 4, 0)
    assert nbr.tolist() == [[-1, -1, -1, -1]] and cnt.tolist() == [0]


# ---- host rules ------------------------------------------------------------------------------------------------------------------

def test_host_plan_pools_the_views_with_few_depths_and_raises_without_any():
    from sfm_mvs_amd import mvs_plan
    m = np.array([100, 7, 8, 0], np.int32)
    z_lo, z_hi = np.array([2.0, 9.0, 1.5, 0.0], np.float32), np.array([4.0, 9.5, 6.0, 0.0], np.float32)
    r = mvs_plan.pooled_ranges(m, z_lo, z_hi)
    assert np.allclose(r, [[1.6, 5.0], [1.2, 7.5], [1.2, 7.5], [1.2, 7.5]], rtol=1e-15, atol=0)
    assert np.array_equal(r, npl.pooled_ranges(m, z_lo, z_hi))
    with pytest.raises(mvs_plan.SfmHipError, match="8 sparse points"):
        mvs_plan.pooled_ranges(np.array([7, 0, 3]), z_lo[:3], z_hi[:3])
    assert npl.pooled_ranges(np.array([7, 0, 3]), z_lo[:3], z_hi[:3]) is None


def test_run_mvs_validates_its_keywords_before_any_device_call():
    """No GPU here: every one of these raises SfmHipError from the validation, which stands before the first use of the device."""
    from sfm_mvs_amd import mvs
    n = 4
    imgs = [np.zeros((12, 16, 3), np.uint8)] * n
    posearr = np.zeros(9 + 12 * n)
    X = np.zeros((10, 3))
    ok_n = [mvs.neighbours(i, n, 2) for i in range(n)]
    ok_r = [(1.0, 2.0)] * n
    bad_n = [ok_n[:3], [[0]] + ok_n[1:], [[4]] + ok_n[1:], [[-1]] + ok_n[1:], [[1.5]] + ok_n[1:], [[1, 2, 3] * 3] + ok_n[1:]]
    for nb in bad_n:
        with pytest.raises(mvs.SfmHipError, match="run_mvs"):
            mvs.run_mvs(imgs, np.eye(3), posearr, X, neighbours=nb, ranges=ok_r)
    inf, nan = float("inf"), float("nan")
    bad_r = [ok_r[:3], [(0.0, 2.0)] + ok_r[1:], [(2.0, 1.0)] + ok_r[1:], [(1.0, 1.0)] + ok_r[1:], [(1.0, inf)] + ok_r[1:], [(nan, 2.0)] + ok_r[1:],
             [(-1.0, 2.0)] + ok_r[1:], [(1.0, 2.0, 3.0)] * n]
    for rg in bad_r:
        with pytest.raises(mvs.SfmHipError, match="run_mvs"):
            mvs.run_mvs(imgs, np.eye(3), posearr, X, neighbours=ok_n, ranges=rg)
    with pytest.raises(mvs.SfmHipError, match="run_mvs"):
        mvs.run_mvs(imgs, np.eye(3), posearr, X, ranges=bad_r[1])                  # each keyword on its own, too
    assert mvs._checked_neighbours([[1], [], [0, 1], (2,)], 4) == [[1], [], [0, 1], [2]]
    planes = mvs._checked_ranges(ok_r, n, 8)
    assert planes.shape == (n, 8) and planes.dtype == np.float32 and planes[0, 0] == np.float32(0.5) and planes[0, -1] == np.float32(1.0)


# ---- calibration (docs/mvs.md §8.4) -------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def calibration_figures():
    """The arc's middle view of the permuted scene, swept with np_mvs: with the planned sources and range, and with sequence neighbours
    and mvs.depth_range -> dict."""
    from sfm_mvs_amd import mvs, mvs_plan
    from test_mvs_cpu import depth_accuracy
    imgs, K, P, gt, perm = mc.permuted_scene()
    X, cam_idx, pt_idx = mc.synth_tracks(K, P, gt)
    n, i = len(P), mc.MIDDLE
    plan = npl.plan_views(cam_idx, pt_idx, X, P, mc.NSRC, mvs_plan.MIN_ANGLE_DEG, mvs_plan.MAX_ANGLE_DEG, mvs_plan.MIN_GOOD)
    seq, old = mvs.neighbours(i, n, mc.NSRC), mvs.depth_range(X, P[i], P_all=P)
    dp = mc.np_depth_map(imgs, K, P, i, plan["neighbours"][i], plan["ranges"][i], mc.NDEPTH)
    ds = mc.np_depth_map(imgs, K, P, i, seq, old, mc.NDEPTH)
    return dict(plan=plan, perm=perm, planned=depth_accuracy(dp, gt[i], 3), sequence=depth_accuracy(ds, gt[i], 3), wrong_planned=mc.wrong_share(dp, gt[i]),
                wrong_sequence=mc.wrong_share(ds, gt[i]), coverage=[mc.coverage(plan["ranges"][k], gt[k]) for k in range(n)], depth=dp, X=X,
                cam_idx=cam_idx, pt_idx=pt_idx)


def test_calibration_on_the_permuted_arc_scene():
    from test_mvs_cpu import MIN_VALID_FRACTION, MIN_WITHIN_1PCT
    f = calibration_figures()
    perm = f["perm"]
    assert int(perm[mc.MIDDLE]) == mc.SCENE["n"] // 2
    print(f"planned {f['planned']} wrong {f['wrong_planned']:.4f}; sequence {f['sequence']} wrong {f['wrong_sequence']:.4f}; coverage {f['coverage']}")
    # every view's planned sources are its nearest views on the arc (the four at arc distance <= 2, or the nearest four at an end)
    for i, row in enumerate(f["plan"]["neighbours"]):
        assert len(row) == mc.NSRC
        assert max(abs(int(perm[v]) - int(perm[i])) for v in row) <= (2 if 2 <= perm[i] <= mc.SCENE["n"] - 3 else 4), (i, row)
    valid, within = f["planned"]
    assert valid >= MIN_VALID_FRACTION and within >= MIN_WITHIN_1PCT, f["planned"]
    valid, within = f["sequence"]
    assert not (valid >= MIN_VALID_FRACTION and within >= MIN_WITHIN_1PCT), f["sequence"]
    assert f["wrong_planned"] <= PLAN_BAR * f["wrong_sequence"], (f["wrong_planned"], f["wrong_sequence"])
    assert min(f["coverage"]) >= RANGE_COVERAGE - (1.0 - RANGE_COVERAGE) / 2.0, f["coverage"]


def test_ring_scene_sources_are_the_ring_neighbours():
    """ring_scene(8, 600, 400, seed=3) with its planted tracks: every camera sees all 400 points, so shared is 400 off the diagonal; ring
    neighbours stand 45 degrees apart as seen from the scene, the next ones 90.  A window of 1..60 degrees admits the former only."""
    P, X, cam_idx, pt_idx = mc.ring_tracks()
    plan = npl.plan_views(cam_idx, pt_idx, X, P, 4, 1.0, 60.0, 8)
    assert np.array_equal(plan["shared"], 400 * (1 - np.eye(8, dtype=np.int32)))
    for i in range(8):
        ring = {(i - 1) % 8, (i + 1) % 8}
        assert set(plan["neighbours"][i][:2]) == ring, (i, plan["neighbours"][i])
        assert all(plan["good"][i, j] == 0 for j in range(8) if j not in ring) and all(plan["good"][i, j] > 300 for j in ring)
    assert np.all(plan["m"] == 400) and np.all(plan["ranges"][:, 0] > 5.0) and np.all(plan["ranges"][:, 1] < 11.5)
    assert npl.plan_views(cam_idx, pt_idx, X, P, 4, 1.0, 30.0, 8)["neighbours"] == [[]] * 8     # the default window is too narrow for this ring
