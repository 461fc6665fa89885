"""The VERIFY-H family without a GPU: the restatement tests/np_verify_h.py with the library's host solvers (include/sfm_hip.h,
"VERIFY-H"; docs/tracks.md §13).  Argument errors, the four-point solver on exact and on degenerate data, the refit beside
numpy.linalg, the monotone refit, the calibration of the defaults, the classification of the planted scenes, and the seed order of
`register.register_loop(pair_config=...)` on a stub engine."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import np_verify as nv  # noqa: E402
import np_verify_h as nh  # noqa: E402
import verify_cases as vc  # noqa: E402
import verify_h_cases as hc  # noqa: E402


@pytest.fixture(scope="module")
def verify():
    import sfm_mvs_amd
    sfm_mvs_amd.lib()
    from oracle import oracle as O
    O.lib()
    from sfm_mvs_amd import verify
    return verify


# ---- argument errors --------------------------------------------------------------------------------------------------------------

def test_argument_errors_of_the_entry_points_come_before_any_device_call(verify):
    from sfm_mvs_amd import _lib
    L = _lib.lib()
    one = (np.zeros(16, np.int64).ctypes.data,) * 12                 # never dereferenced: every call below fails on its arguments
    nan = float("nan")

    def models(n_pairs=1, cap=4, H=8, n_img=2, n_nodes=4, img_off=one[4]):
        return L.sfm_verify_h_models(one[0], one[1], one[2], one[3], img_off, n_img, one[5], n_nodes, n_pairs, cap, H, one[6], one[7], None)

    def score(n_pairs=1, cap=4, H=8, n_img=2, n_nodes=4, img_off=one[5], thr=1.0):
        return L.sfm_verify_h_score(one[0], one[1], one[2], one[3], one[4], img_off, n_img, one[6], n_nodes, n_pairs, cap, H, thr, one[7], one[8], None)

    def select(n_pairs=1, cap=4, H=8, n_img=2, n_nodes=4, img_off=one[6], thr=1.0, refit=1):
        return L.sfm_verify_h_select(one[0], one[1], one[2], one[3], one[4], one[5], img_off, n_img, one[7], n_nodes, n_pairs, cap, H, thr, refit,
                                     one[8], one[9], one[10], one[11], None)

    for fn in (models, score, select):
        for kw in (dict(n_pairs=-1), dict(cap=-1), dict(cap=2 ** 31), dict(n_pairs=2 ** 31 // 1024 + 1), dict(n_pairs=2 ** 20, cap=2 ** 12),
                   dict(n_img=0), dict(n_img=65537), dict(n_nodes=-1), dict(n_nodes=2 ** 31)):
            assert fn(**kw) == -1 and b"bad sizes" in L.sfm_last_error(), (fn.__name__, kw)
        for H in (0, 1025, -3):
            assert fn(H=H) == -1 and b"the budget must be 1..1024" in L.sfm_last_error()
        assert fn(img_off=None) == -1 and b"null img_off" in L.sfm_last_error()
    for fn in (score, select):
        assert fn(thr=nan) == -1 and b"thr2h is NaN" in L.sfm_last_error()
    for refit in (-1, 2):
        assert select(refit=refit) == -1 and b"refit must be 0 or 1" in L.sfm_last_error()
    assert L.sfm_verify_h_models(None, None, None, None, one[0], 2, None, 4, 1, 4, 8, None, None, None) == -1 and b"null pointer" in L.sfm_last_error()
    assert L.sfm_verify_h_score(None, None, None, None, None, one[0], 2, None, 4, 1, 4, 8, 1.0, None, None, None) == -1 and b"null pointer" in L.sfm_last_error()
    assert L.sfm_verify_h_select(None, None, None, None, None, None, one[0], 2, None, 4, 1, 4, 8, 1.0, 1, None, None, None, None, None) == -1
    assert b"null pointer" in L.sfm_last_error()
    assert models(n_pairs=0) == 0 and score(n_pairs=0) == 0 and select(n_pairs=0) == 0           # nothing to do
    assert L.sfm_host_homography4(None, None, None) == -1 and L.sfm_host_verify_h_refit(None, None) == -1
    assert L.sfm_host_verify_h_normalise(None, None, None) == -1


def test_the_wrappers_reject_host_tensors_and_bad_settings(verify):
    Err = verify.SfmHipError
    z = lambda shape, dt: torch.zeros(shape, dtype=dt)                # noqa: E731
    part = (z((1, 3, 2), torch.int32), z(1, torch.int32), z((1, 2), torch.int32), z(3, torch.int32), z((4, 2), torch.float64))
    with pytest.raises(Err, match="no CPU fallback"):
        verify.h_models(z((1, 4, 5), torch.int32), *part)
    with pytest.raises(Err, match="no CPU fallback"):
        verify.h_score(z((1, 4, 9), torch.float64), z((1, 4), torch.int32), *part, 1e-6)
    with pytest.raises(Err, match="no CPU fallback"):
        verify.h_select(z((1, 4, 9), torch.float64), z((1, 4), torch.int32), z(1, torch.int64), *part, 1e-6)
    assert verify.homography_settings(None) is None and verify.homography_settings(False) is None
    assert verify.homography_settings(True) == verify.DEFAULT_HOMOGRAPHY
    assert verify.homography_settings(dict(threshold=2, refit=0)) == dict(verify.DEFAULT_HOMOGRAPHY, threshold=2.0, refit=0)
    for bad in (dict(threshold=0), dict(threshold=float("nan")), dict(min_ratio=-1), dict(rot_spread=0.5), dict(rot_spread=float("nan")),
                dict(min_inliers=-1), dict(refit=2), dict(refits=1), dict(threshold="wide"), "yes", 3):
        with pytest.raises(Err):
            verify.homography_settings(bad)
    with pytest.raises(Err):
        verify.verify_pairs(None, None, None, None, None, np.eye(3), homography=dict(refit=7))      # refused before anything is touched
    plain = verify.workspace_bytes(2016, 10000)
    assert verify.workspace_bytes(2016, 10000, homography=None) == plain
    assert verify.workspace_bytes(2016, 10000, homography=True) - plain == 364 * (1024 * 80 + 8)
    assert verify.workspace_bytes(2016, 10000, lo=True, homography=True) - verify.workspace_bytes(2016, 10000, lo=True) == 364 * (1024 * 80 + 8)
    assert (verify.CONFIG_NONE, verify.CONFIG_GENERAL, verify.CONFIG_PLANAR, verify.CONFIG_ROTATING) == (0, 1, 2, 3) == \
        (nh.CONFIG_NONE, nh.CONFIG_GENERAL, nh.CONFIG_PLANAR, nh.CONFIG_ROTATING)
    from sfm_mvs_amd import register
    assert (register.CONFIG_GENERAL, register.CONFIG_PLANAR) == (verify.CONFIG_GENERAL, verify.CONFIG_PLANAR)


# ---- the four-point solver --------------------------------------------------------------------------------------------------------

def exact_points(kind, n, seed=3):
    """Exact K-normalised projections of `n` points of the planar scene's plane, or of the ball for the rotating scene: [n, 4]."""
    rng = np.random.default_rng(seed)
    K, Rt0, Rt1, nrm = hc.cameras(kind)
    X = rng.uniform(-1.0, 1.0, (n, 3))
    if nrm is not None:
        X = X - (X @ nrm)[:, None] * nrm[None, :]
    x0, x1 = X @ Rt0[:, :3].T + Rt0[:, 3], X @ Rt1[:, :3].T + Rt1[:, 3]
    return np.hstack([x0[:, :2] / x0[:, 2:], x1[:, :2] / x1[:, 2:]])


def test_homography4_recovers_the_planted_homography_and_is_the_restatement_bit_for_bit(verify):
    """The bound is the 1e-9 tests/test_hostgeom.py holds the five-point to; measured: 2e-13 (planar), 2e-13 (rotating) at worst over
    the 40 samples."""
    from sfm_mvs_amd import hostgeom
    worst = {}
    for kind in ("planar", "rotating"):
        Hp = hc.planted_homography(kind)
        assert abs(np.linalg.svd(Hp, compute_uv=False)[1] - 1) < 1e-12
        for seed in range(20):
            pts = exact_points(kind, 4, seed)
            H = hostgeom.homography4(pts[:, :2], pts[:, 2:])
            assert H is not None and H[2, 2] == 1.0
            ok, h = nh.homography4(pts[None, :, :2], pts[None, :, 2:])
            assert ok[0] and np.array_equal(h[0].view(np.int64), H.reshape(9).view(np.int64))
            Hn = H / np.linalg.svd(H, compute_uv=False)[1]
            err = min(np.abs(Hn - Hp).max(), np.abs(Hn + Hp).max())
            worst[kind] = max(worst.get(kind, 0.0), err)
            Hl, sv = hostgeom.verify_h_normalise(H)
            assert np.abs(Hl - Hn).max() < 1e-12 and sv[1] == 1.0 and sv[0] >= 1.0 >= sv[2] > 0
            assert np.allclose(sv, np.linalg.svd(Hn, compute_uv=False), rtol=1e-12)
    print("homography4 against the planted homography, worst of 20 samples:", worst)
    assert max(worst.values()) < 1e-9


def test_homography4_returns_no_model_on_degenerate_points(verify):
    from sfm_mvs_amd import hostgeom
    rng = np.random.default_rng(1)
    x2 = rng.normal(size=(4, 2))
    same = np.tile(rng.normal(size=(1, 2)), (4, 1))
    assert hostgeom.homography4(same, np.tile(x2[:1], (4, 1))) is None               # four equal points: two exactly zero rows
    assert hostgeom.homography4(same, x2) is None
    # three collinear points on an axis: columns 1, 4 and 7 of the system have two non-zero rows between them, an exactly zero pivot
    for line in ([[0, 0], [1, 0], [2, 0], [0.3, 1]], [[0, 0.5], [0, 1], [0, -2], [1, 0.3]], [[-1, 0], [0.25, 0], [3, 0], [0, 1]]):
        x1 = np.array(line, np.float64)
        assert hostgeom.homography4(x1, x2) is None, line
        assert not nh.homography4(x1[None], x2[None])[0][0]
    x1 = rng.normal(size=(4, 2))
    for bad in (np.nan, np.inf, 1e308):
        y = x1.copy()
        y[2, 1] = bad
        assert hostgeom.homography4(y, x2) is None and not nh.homography4(y[None], x2[None])[0][0]
    assert hostgeom.homography4(x1, x2) is not None


def test_the_refit_agrees_with_numpy_on_the_smallest_eigenvector(verify):
    from sfm_mvs_amd import hostgeom
    for kind in ("planar", "rotating"):
        pts = exact_points(kind, 60) + np.random.default_rng(2).normal(0, 1e-4, (60, 4))
        M = nh.moments(pts, np.ones(len(pts), bool))
        a1, b1, a2, b2 = pts.T
        z, o = np.zeros(60), np.ones(60)
        r = np.concatenate([np.stack([-a1, -b1, -o, z, z, z, a2 * a1, a2 * b1, a2], 1), np.stack([z, z, z, -a1, -b1, -o, b2 * a1, b2 * b1, b2], 1)])
        assert np.allclose(M, r.T @ r, rtol=1e-12, atol=1e-15) and np.array_equal(M, M.T)
        c = hostgeom.verify_h_refit(M).reshape(9)
        v = np.linalg.eigh(M)[1][:, 0]
        assert abs(np.linalg.norm(c) - 1) < 1e-12 and np.abs(np.sign(c @ v) * c - v).max() < 1e-8
        assert np.array_equal(hostgeom.verify_h_refit(M).reshape(9), c)                # the same bits again
        Hp = hc.planted_homography(kind)
        Hn = hostgeom.verify_h_normalise(c)[0]
        assert min(np.abs(Hn - Hp).max(), np.abs(Hn + Hp).max()) < 1e-2
    bad = M.copy()
    bad[0, 1] = bad[1, 0] = np.inf - np.inf
    assert not np.isfinite(hostgeom.verify_h_refit(bad)).all()                          # what the non-finite stop looks at


# ---- the planted scenes -----------------------------------------------------------------------------------------------------------

def all_rows(threshold=None):
    rows = hc.calibration()
    return rows if threshold is None else [r for r in rows if r["threshold"] == threshold]


def test_the_refit_is_monotone_on_all_81_scenes(verify):
    rows = all_rows(verify.DEFAULT_HOMOGRAPHY["threshold"])
    assert len(rows) == 81
    for r in rows:
        assert r["n_H"] >= r["n_sample"] and (r["n_H"] > r["n_sample"]) == bool(r["refit_won"]), r
    for kind, m, frac, seed in (("planar", 500, 0.5, 0), ("general", 500, 0.8, 1), ("rotating", 50, 0.3, 2)):
        with_refit, without = hc.scene_row(kind, m, frac, seed, 1.2, 1), hc.scene_row(kind, m, frac, seed, 1.2, 0)
        assert without["n_H"] == without["n_sample"] == with_refit["n_sample"] and not without["refit_won"]


def test_calibration_of_the_defaults(verify):
    """The committed table is what the restatement computes, and the defaults are what the rules of docs/tracks.md §13.4 give on it."""
    rows = all_rows()
    doc = json.load(open(os.path.join(os.path.join(HERE, "golden"), hc.CALIBRATION_JSON)))
    assert len(rows) == len(doc["rows"]) == 81 * len(hc.THRESHOLDS) and doc["budget"] == hc.BUDGET == verify.DEFAULT_BUDGET
    for got, want in zip(rows, doc["rows"]):
        assert {k: got[k] for k in ("kind", "inliers", "m", "seed", "threshold")} == {k: want[k] for k in ("kind", "inliers", "m", "seed", "threshold")}
        for k in ("n_E", "n_H", "n_sample", "refit_won"):
            assert got[k] == want[k], (got, want)
        for k in ("spread", "recall_h", "outliers_h", "recall_e", "outliers_e"):
            assert (got[k] is None) == (want[k] is None) and (got[k] is None or abs(got[k] - want[k]) <= 1e-9 * max(abs(want[k]), 1.0)), (k, got, want)
    thr, table = hc.chosen_threshold(rows)
    assert thr == verify.DEFAULT_HOMOGRAPHY["threshold"] and thr > min(hc.THRESHOLDS)
    below = max(t for t in table if t < thr)
    assert any(c[2] < c[3] for c in table[below])                    # the threshold below fails the rule: the choice is the smallest
    assert all(c[4] <= 0.01 for c in table[thr])                     # planted outliers kept by keep_h on the planar scenes: under a point
    assert hc.chosen_defaults(rows) == verify.DEFAULT_HOMOGRAPHY == doc["defaults"]
    ratio, spread = hc.separation(rows, thr, "ratio"), hc.separation(rows, thr, "spread")
    assert ratio["factor"] >= 2.0                                    # general against planar and rotating: a factor of 16
    assert 1.0 < spread["factor"] < 2.0 and spread["low"] < verify.DEFAULT_HOMOGRAPHY["rot_spread"] < spread["high"]
    # sv0 / sv2 separates by less than a factor of two (docs/tracks.md §13.4 says so); the geometric mean misclassifies none of the
    # asserted scenes, so no other value can misclassify fewer
    wrong = hc.misclassified(rows, verify.DEFAULT_HOMOGRAPHY)
    assert all(w[2] == 50 for w in wrong) and len(wrong) == 8, wrong  # the 30 % scenes and m = 50 are counted, not asserted


@pytest.mark.parametrize("kind", hc.KINDS)
def test_every_asserted_scene_gets_its_planted_configuration(verify, kind):
    """36 scenes: three kinds x shares 0.5, 0.8 x m 500, 5 000 x seeds 0..2, through the restated `verify_pairs(homography=True)`."""
    s = verify.DEFAULT_HOMOGRAPHY
    for frac in hc.ASSERTED_FRACTIONS:
        for m in hc.ASSERTED_SIZES:
            for seed in hc.SEEDS:
                case, st, _ = hc.scene(kind, m, frac, seed)
                r = hc.scene_row(kind, m, frac, seed, s["threshold"])
                assert hc.classify_row(r, s) == hc.PLANTED_CONFIG[kind], r
                if m == 500:                                         # and the composed restatement says the same word
                    out = nh.verify_pairs(case["store"], case["nq"], case["pairs"], case["img_off"], case["kp"], case["K"], 0.7, budget=hc.BUDGET, seed=seed,
                                          threshold_h=s["threshold"], min_ratio=s["min_ratio"], rot_spread=s["rot_spread"], min_inliers=s["min_inliers"],
                                          refit=s["refit"], plain=st)
                    assert out["config"].tolist() == [hc.PLANTED_CONFIG[kind]] and out["h_info"][0, 2] == r["n_H"]
                    assert np.array_equal(out["keep"], st["keep"]) and np.array_equal(out["info"], st["info"])


def test_config_of_by_hand():
    info, h_info = np.zeros((6, 8), np.int32), np.zeros((6, 8), np.int32)
    info[:, 2] = (7, 8, 100, 100, 100, 100)
    h_info[:, 2] = (7, 8, 24, 25, 90, 90)
    sv = np.array([[1.0, 1, 1], [1.2, 1, 0.9], [3, 1, 0.5], [3, 1, 0.5], [1.5, 1, 1.0], [1.6, 1, 1.0]])
    got = nh.config_of(info, h_info, sv, 0.25, 1.5, 8)
    assert got.tolist() == [nh.CONFIG_NONE, nh.CONFIG_ROTATING, nh.CONFIG_GENERAL, nh.CONFIG_PLANAR, nh.CONFIG_ROTATING, nh.CONFIG_PLANAR]
    sv[4] = (np.nan, np.nan, np.nan)                                 # a homography without a middle singular value is no rotation
    sv[5] = (2.0, 1.0, 0.0)
    assert nh.config_of(info, h_info, sv, 0.25, 1.5, 8)[4:].tolist() == [nh.CONFIG_PLANAR, nh.CONFIG_PLANAR]


# ---- the seed order of the registration loop --------------------------------------------------------------------------------------

class Stop(Exception):
    pass


class StubEngine:
    """Records the seed candidates `register_loop` tries: every relative pose fails, so the loop walks its list to the end."""

    def __init__(self, n_img, shared):
        self.n_img, self.S, self.tried, self.rounds = n_img, np.zeros((n_img, n_img), np.int64), [], 0
        for (a, b), c in shared.items():
            self.S[a, b] = self.S[b, a] = c

    def tracks(self):
        return 0, 0

    def shared(self):
        return self.S

    def pair_points(self, a, b, m):
        self.tried.append((a, b))
        return np.zeros((m, 2), np.float32), np.zeros((m, 2), np.float32)

    def relative_pose(self, p0, p1):
        return None

    def round(self, registered, P):
        self.rounds += 1
        raise Stop()


PAIRS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
SHARED = {(0, 1): 90, (0, 2): 40, (0, 3): 40, (1, 2): 70, (1, 3): 0, (2, 3): 55}


def tried_with(verify, **kw):
    from sfm_mvs_amd import register
    eng = StubEngine(4, SHARED)
    with pytest.raises(verify.SfmHipError, match="no seed pair"):
        register.register_loop(eng, 4, PAIRS, np.eye(3), seed_tries=99, **kw)
    assert eng.rounds == 0
    return eng.tried


def test_register_loop_orders_its_seeds_by_the_configuration_words(verify):
    from sfm_mvs_amd import register
    G, Pl, Ro, No = verify.CONFIG_GENERAL, verify.CONFIG_PLANAR, verify.CONFIG_ROTATING, verify.CONFIG_NONE
    today = [(0, 1), (1, 2), (2, 3), (0, 2), (0, 3)]                 # most shared tracks first, stable; (1, 3) shares none
    assert tried_with(verify) == today == tried_with(verify, pair_config=None)
    assert tried_with(verify, pair_config=[G] * 6) == today
    #                                   (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)
    assert tried_with(verify, pair_config=[Ro, G, Pl, Pl, G, G]) == [(2, 3), (0, 2), (1, 2), (0, 3)]       # GENERAL, then PLANAR; never (0, 1)
    assert tried_with(verify, pair_config=np.array([No, Ro, Ro, No, G, Ro], np.int32)) == []              # (1, 3) is GENERAL and shares nothing
    assert tried_with(verify, pair_config=(Pl, Ro, G, No, G, Pl)) == [(0, 3), (0, 1), (2, 3)]
    # an explicit seed pair is honoured whatever its word
    eng = StubEngine(4, SHARED)
    with pytest.raises(verify.SfmHipError, match="no seed pair"):
        register.register_loop(eng, 4, PAIRS, np.eye(3), seed_pair=(0, 1), pair_config=[Ro] * 6)
    assert eng.tried == [(0, 1)]
    # a pose that succeeds reaches the first model round
    eng = StubEngine(4, SHARED)
    eng.relative_pose = lambda p0, p1: (np.eye(3), np.array([1.0, 0, 0]))
    with pytest.raises(Stop):
        register.register_loop(eng, 4, PAIRS, np.eye(3), pair_config=[Ro, G, Pl, Pl, G, G])
    assert eng.tried == [(2, 3)] and eng.rounds == 1
    # `seeds` carries the word of every candidate tried, and does not without pair_config: the first seed's round leaves too few points
    for config, want in (([Ro, Pl, Pl, G, G, Pl], [((1, 2), G), ((2, 3), Pl)]), (None, [((0, 1), None), ((1, 2), None)])):
        eng = StubEngine(4, SHARED)
        eng.relative_pose = lambda p0, p1: (np.eye(3), np.array([1.0, 0, 0]))
        eng.round = lambda registered, P, eng=eng: (eng.tried.append("round"), dict(points=0 if eng.tried.count("round") == 1 else 10 * register.MIN_SEED,
                                                                                     seen=np.zeros(4, np.int32), cells=np.zeros(4, np.int32)))[1]
        eng.bundle = lambda order, P, model, **kw: (P[order], [0.0], None)
        eng.result = lambda model: {}
        out = register.register_loop(eng, 4, PAIRS, np.eye(3), pair_config=config)
        assert [(s["pair"], s.get("config")) for s in out["seeds"]] == want and all(("config" in s) == (config is not None) for s in out["seeds"])


def test_register_rejects_a_bad_pair_config_before_any_work(verify):
    from sfm_mvs_amd import register
    for bad in ([1] * 5, [1] * 7, [1, 1, 1, 1, 1, 4], [1, 1, -1, 1, 1, 1], [1, 1, None, 1, 1, 1], 3):
        eng = StubEngine(4, SHARED)
        with pytest.raises(verify.SfmHipError, match="pair_config"):
            register.register_loop(eng, 4, PAIRS, np.eye(3), pair_config=bad)
        assert eng.tried == []
        with pytest.raises(verify.SfmHipError, match="pair_config"):
            register.register_tracks(None, None, PAIRS, [None] * 4, np.eye(3), (10, 10), pair_config=bad)
