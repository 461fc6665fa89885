"""The VERIFY family without a GPU: the restatement tests/np_verify.py with the library's host solvers is a complete CPU model of the
algorithm (include/sfm_hip.h, "VERIFY"; docs/tracks.md §11).  The sampler, the calibration of the hypothesis budget on planted
two-view scenes, and the degenerate pairs."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import np_verify as nv  # noqa: E402
import verify_cases as vc  # noqa: E402


@pytest.fixture(scope="module")
def host_solvers():
    import sfm_mvs_amd
    sfm_mvs_amd.lib()
    from oracle import oracle as O
    O.lib()
    from sfm_mvs_amd import verify
    return verify


# ---- the sampler ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", [5, 6, 7, 64, 10 ** 4])
def test_samples_are_distinct_and_in_range(m):
    samp = nv.samples(np.array([m, m], np.int32), 200, 99)
    assert samp.shape == (2, 200, 5) and samp.min() >= 0 and samp.max() < m
    assert all(len(set(row)) == 5 for row in samp.reshape(-1, 5).tolist())
    if m == 5:
        assert (np.sort(samp, axis=2) == np.arange(5)).all()         # every sample is the whole set
    else:
        rows = [tuple(r) for r in samp.reshape(-1, 5).tolist()]
        assert len(set(rows)) > 0.9 * len(rows) or m < 8             # draws of different (p, s) differ
        assert not np.array_equal(samp[0], samp[1])
    assert not np.array_equal(samp, nv.samples(np.array([m, m], np.int32), 200, 100)) or m == 5


def test_mix_and_draw_by_hand():
    assert nv.mix(0) == 0                                           # 0 is the fixed point of the xorshift-multiply
    x = 1
    x ^= x >> 16; x = (x * 0x7feb352d) & nv.M32; x ^= x >> 15; x = (x * 0x846ca68b) & nv.M32; x ^= x >> 16
    assert nv.mix(1) == x and 0 <= nv.draw(7, 3, 2, 1, 1000) < 1000
    h = nv.mix((nv.mix(nv.mix((7 + 0x9e3779b9 * 3) & nv.M32) ^ 2) + 1) & nv.M32)
    assert nv.draw(7, 3, 2, 1, 1000) == (h * 1000) >> 32
    assert [nv.draw(7, 3, 2, c, 2 ** 31 - 1) for c in range(3)] == [(nv.mix((nv.mix(nv.mix((7 + 0x9e3779b9 * 3) & nv.M32) ^ 2) + c) & nv.M32) * (2 ** 31 - 1)) >> 32
                                                                   for c in range(3)]


def test_fewer_than_five_survivors_and_exhausted_draws_give_no_sample():
    assert (nv.samples(np.array([0, 4, -1], np.int32), 8, 1) == -1).all()
    assert nv.fill_slots(lambda c: c % 4) is None                   # 64 draws over four values never fill five slots
    assert nv.fill_slots(lambda c: 3 if c < 60 else c) == [3, 60, 61, 62, 63]
    assert nv.fill_slots(lambda c: 3 if c < 61 else c) is None      # the fifth distinct value would be draw 64
    assert nv.fill_slots(lambda c: c) == [0, 1, 2, 3, 4]


# ---- calibration ------------------------------------------------------------------------------------------------------------------

def test_calibration_of_the_budget(host_solvers):
    """Recall of planted inliers / share of planted outliers kept for H in 32..1024 on planted pairs (inlier shares 0.3, 0.5, 0.8; m = 50,
    500, 5 000; 0.5 px keypoint noise; seeds 0, 1, 2).  The table is committed as tests/golden/verify_calibration.json and printed in
    docs/tracks.md §11; the default budget is the smallest H past which neither figure improves by more than a point at 0.3: the rule
    does not settle inside the admitted range (the recall still rises from 512 to 1 024), so the default is the cap."""
    table = vc.calibration()
    print(vc.format_table(table))
    want = vc.load_calibration()
    assert sorted(want) == sorted(table)
    for key in table:
        assert np.allclose(table[key], want[key], rtol=0, atol=1e-12), (key, table[key], want[key])
    assert host_solvers.DEFAULT_BUDGET == vc.smallest_sufficient_budget(table) == host_solvers.MAX_BUDGET
    assert np.mean([table[(0.3, m, 1024)][0] - table[(0.3, m, 512)][0] for m in vc.SIZES]) > 0.01      # not settled: the cap it is
    for frac in vc.FRACTIONS:                                       # the largest budget recalls at least what the smallest does
        for m in vc.SIZES:
            assert table[(frac, m, 512)][0] >= table[(frac, m, 32)][0]
    assert all(table[(0.8, m, 512)][1] <= 0.01 for m in vc.SIZES)


# ---- degenerate pairs -------------------------------------------------------------------------------------------------------------

def invariants(case, out, ratio=0.7):
    """What the specification says of any pair."""
    keep, E, Rt, info = out["keep"], out["E"], out["Rt"], out["info"]
    surv, m = nv.survivors(case["store"], case["nq"], case["pairs"], case["img_off"], ratio)
    for p in range(len(m)):
        assert info[p, 0] == m[p] and info[p, 3] == keep[p].sum() and info[p, 2] >= info[p, 3] and info[p, 2] <= m[p]
        assert set(np.flatnonzero(keep[p])) <= set(surv[p, :m[p], 0])
        assert bool(info[p, 7] & nv.FEW_SURVIVORS) == (m[p] < 5)
        if info[p, 7] & nv.NO_MODEL:
            assert not keep[p].any() and not E[p].any() and not Rt[p].any() and info[p, 2:7].tolist() == [0, 0, -1, -1, -1]
        else:
            assert abs(np.linalg.norm(E[p]) - 1) < 1e-9 and 0 <= info[p, 6] < 4 and 0 <= info[p, 5] < nv.SLOTS
            assert bool(info[p, 7] & nv.NO_VOTE) == (info[p, 3] == 0)


def test_degenerate_pairs(host_solvers):
    base = vc.planted_pair(40, 0.8, 3)
    for name in ("m = 0", "m = 4", "all points equal", "collinear image points"):
        case = dict(base, store=base["store"].copy(), kp=base["kp"].copy(), nq=base["nq"].copy())
        if name == "m = 0":
            case["nq"][:] = 0
        if name == "m = 4":
            case["nq"][:] = 4
        if name == "all points equal":
            case["kp"][:] = [400.5, 300.25]
        if name == "collinear image points":
            case["kp"][:, 1] = 0.5 * case["kp"][:, 0] + 20
        out = nv.verify_pairs(case["store"], case["nq"], case["pairs"], case["img_off"], case["kp"], case["K"], 0.7, budget=32, seed=1)
        print(name, out["info"].tolist())
        invariants(case, out)
        if name in ("m = 0", "m = 4"):
            assert out["info"][0].tolist() == [int(name[-1]), 0, 0, 0, -1, -1, -1, nv.FEW_SURVIVORS | nv.NO_MODEL] and not out["keep"].any()
        if name == "all points equal":
            assert out["info"][0, 0] == 40 and not (out["info"][0, 7] & nv.FEW_SURVIVORS)
    out = nv.verify_pairs(base["store"], base["nq"], base["pairs"], base["img_off"], base["kp"], base["K"], 0.7, budget=64, seed=1)
    invariants(base, out)
    assert out["info"][0, 7] == 0 and vc.rates(out["keep"][0], base["planted"])[1] == 0.0
    iters = nv.confidence_iters(out["info"])
    assert np.array_equal(iters, host_solvers.confidence_iters(out["info"])) and 0 < iters[0] < np.inf
    assert host_solvers.confidence_iters(np.array([[10, 0, 10, 9, 0, 0, 0, 0], [10, 0, 0, 0, -1, -1, -1, 2]], np.int32)).tolist() == [0.0, np.inf]


def test_thr2_and_normalisation_follow_the_per_pair_path(host_solvers, oracle):
    K = vc.planted_pair(10, 1.0, 0)["K"]
    assert np.float32(host_solvers.thr2_of(K, 0.4)) == nv.thr2_of(K, 0.4)
    kp = np.random.default_rng(0).uniform(0, 900, (50, 2)).astype(np.float32)
    assert np.array_equal(nv.normalise(kp, K), oracle.k_normalise(kp, K))


def test_verify_keep_rejects_batched_options_on_the_per_pair_path():
    from sfm_mvs_amd import tracks
    with pytest.raises(TypeError):
        tracks.verify_keep(None, [], [], [], np.eye(3), budget=4)
