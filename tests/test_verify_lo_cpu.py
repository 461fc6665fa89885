"""The VERIFY-LO family without a GPU: the restatement tests/np_verify_lo.py with the library's host refit (include/sfm_hip.h,
"VERIFY-LO"; docs/tracks.md §12).  Argument errors, the refit on exact data, the monotone property, the calibration of the defaults and
the quality figures beside the plain batched path and the per-pair path."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import np_verify as nv  # noqa: E402
import np_verify_lo as nl  # noqa: E402
import verify_cases as vc  # noqa: E402
import verify_lo_cases as lc  # noqa: E402


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
    one = (np.zeros(16, np.int64).ctypes.data,) * 12                 # never dereferenced: every call below fails on its sizes
    for n_pairs, H, T, what in ((-1, 8, 1, b"bad sizes"), (1, 0, 1, b"bad sizes"), (1, 1025, 1, b"bad sizes"), (1, 8, 0, b"bad sizes"), (1, 8, 17, b"bad sizes"),
                                (2 ** 31 // 10240 + 1, 8, 1, b"bad sizes")):
        assert L.sfm_verify_top(one[0], one[1], n_pairs, H, T, one[2], None) == -1 and what in L.sfm_last_error()
        assert L.sfm_verify_lo_pick(one[0], one[1], one[2], one[3], n_pairs, H, T, one[4], one[5], one[6], one[7], None) == -1 and what in L.sfm_last_error()
        assert L.sfm_verify_lo(one[0], one[1], T, one[2], one[3], one[4], one[5], 2, one[6], 4, n_pairs, 4, H, 1.0, 0, None, one[7], one[8], one[9], None) == -1
    w = np.array([1.0, np.nan], np.float32)
    lo = lambda **kw: L.sfm_verify_lo(one[0], one[1], kw.get("T", 1), one[2], one[3], one[4], kw.get("img_off", one[5]), kw.get("n_img", 2), one[6],  # noqa: E731
                                      kw.get("n_nodes", 4), 1, kw.get("cap", 4), 8, 1.0, kw.get("R", 0), kw.get("wide2"), one[7], one[8], one[9], None)
    assert lo(R=9) == -1 and b"rounds must be 0..8" in L.sfm_last_error()
    assert lo(R=-1) == -1 and lo(R=1) == -1 and b"null wide2" in L.sfm_last_error()
    assert lo(R=2, wide2=w.ctypes.data) == -1 and b"wide2[1] is NaN" in L.sfm_last_error()
    assert lo(img_off=None) == -1 and b"null img_off" in L.sfm_last_error()
    assert lo(n_img=0) == -1 and lo(n_img=65537) == -1 and lo(cap=-1) == -1 and lo(n_nodes=2 ** 31) == -1 and lo(cap=2 ** 31) == -1
    assert L.sfm_verify_top(None, None, 1, 8, 1, None, None) == -1 and b"null pointer" in L.sfm_last_error()
    assert L.sfm_verify_lo_pick(None, None, None, None, 1, 8, 1, None, None, None, None, None) == -1 and b"null pointer" in L.sfm_last_error()
    assert L.sfm_verify_top(None, None, 0, 8, 1, None, None) == 0   # nothing to do
    assert L.sfm_host_verify_refit(None, None) == -1


def test_the_wrappers_reject_host_tensors_and_bad_settings(verify):
    Err = verify.SfmHipError
    with pytest.raises(Err, match="no CPU fallback"):
        verify.top_models(torch.zeros((1, 4, 10), dtype=torch.int32), torch.zeros((1, 4), dtype=torch.int32), 2)
    with pytest.raises(Err, match="no CPU fallback"):
        verify.pick(torch.zeros((1, 2), dtype=torch.int64), torch.zeros((1, 2, 9), dtype=torch.float64), torch.zeros((1, 2), dtype=torch.int32),
                    torch.zeros((1, 2), dtype=torch.int32), 8)
    with pytest.raises(Err, match="no CPU fallback"):
        verify.local_optimise(torch.zeros((1, 4, 10, 9), dtype=torch.float64), torch.zeros((1, 2), dtype=torch.int64), torch.zeros((1, 3, 2), dtype=torch.int32),
                              torch.zeros(1, dtype=torch.int32), torch.zeros((1, 2), dtype=torch.int32), torch.zeros(3, dtype=torch.int32),
                              torch.zeros((4, 2), dtype=torch.float64), 1e-7, [1e-7])
    assert verify.lo_settings(None) is None
    assert verify.lo_settings(True) == (verify.DEFAULT_LO["top"], tuple(verify.DEFAULT_LO["widen"]))
    assert verify.lo_settings(dict(top=4, rounds=2, widen=(3, 1))) == (4, (3.0, 1.0))
    assert verify.lo_settings(dict(top=2, widen=(2.0, 2.0, 1.0))) == (2, (2.0, 2.0, 1.0))
    assert verify.lo_settings(dict(rounds=3)) == (verify.DEFAULT_LO["top"], (verify.DEFAULT_LO["widen"][0],) * 3)
    assert verify.lo_settings(dict(rounds=0)) == (verify.DEFAULT_LO["top"], ())
    for bad in (dict(top=0), dict(top=17), dict(rounds=9), dict(rounds=2, widen=(1.0,)), dict(widen=(1.0, -1.0)), dict(widen=(float("nan"),)),
                dict(tops=2), "yes", 3, dict(widen=(1.0,) * 9)):
        with pytest.raises(Err):
            verify.lo_settings(bad)
    with pytest.raises(Err):
        verify.verify_pairs(None, None, None, None, None, np.eye(3), lo=dict(top=99))      # refused before anything is touched
    plain = verify.workspace_bytes(2016, 10000)
    assert verify.workspace_bytes(2016, 10000, lo=None) == plain
    assert verify.workspace_bytes(2016, 10000, lo=dict(top=8, rounds=4)) - plain == 364 * (8 * 88 + 720 + 12)
    assert len(verify.DEFAULT_LO["widen"]) == verify.DEFAULT_LO["rounds"] <= verify.MAX_ROUNDS == nl.MAX_ROUNDS and verify.MAX_TOP == nl.MAX_TOP


# ---- the refit --------------------------------------------------------------------------------------------------------------------

def exact_pair(n=60, seed=5):
    """Exact K-normalised projections of `n` points in two of datagen's ring cameras, and the planted essential matrix (unit norm)."""
    from datagen import ring_cameras
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(seed)
    ring = ring_cameras(8)
    (R0, t0), (R1, t1) = ((Rotation.from_rotvec(ring[c, :3]).as_matrix(), ring[c, 3:]) for c in (0, 1))
    X = rng.uniform(-2.0, 2.0, (n, 3))
    x0, x1 = X @ R0.T + t0, X @ R1.T + t1
    R, t = R1 @ R0.T, t1 - R1 @ R0.T @ t0
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    E = tx @ R
    return np.hstack([x0[:, :2] / x0[:, 2:], x1[:, :2] / x1[:, 2:]]), E / np.linalg.norm(E)


def test_the_refit_recovers_the_planted_essential_matrix_and_agrees_with_numpy(verify):
    from sfm_mvs_amd import hostgeom
    pts, E_true = exact_pair()
    M = nl.moments(pts, np.ones(len(pts), bool))
    a = np.stack([pts[:, 2] * pts[:, 0], pts[:, 2] * pts[:, 1], pts[:, 2], pts[:, 3] * pts[:, 0], pts[:, 3] * pts[:, 1], pts[:, 3], pts[:, 0], pts[:, 1],
                  np.ones(len(pts))], 1)
    assert np.allclose(M, a.T @ a, rtol=1e-13, atol=0) and np.array_equal(M, M.T)
    E = hostgeom.verify_refit(M)
    assert abs(np.linalg.norm(E) - 1) < 1e-12
    sign = np.sign((E * E_true).sum())
    assert np.abs(sign * E - E_true).max() < 1e-9
    # numpy.linalg beside it: eigh's smallest eigenvector, projected on the essential manifold by its SVD
    F = np.linalg.eigh(M)[1][:, 0].reshape(3, 3)
    U, _, Vt = np.linalg.svd(F)
    E_np = U @ np.diag([1.0, 1.0, 0.0]) @ Vt
    E_np /= np.linalg.norm(E_np)
    assert np.abs(np.sign((E * E_np).sum()) * E - E_np).max() < 1e-9
    assert np.array_equal(hostgeom.verify_refit(M), E)                                     # and the same bits again
    bad = M.copy()
    bad[0, 1] = bad[1, 0] = np.inf - np.inf                                                # the sum of two huge products of opposite sign
    assert not np.isfinite(hostgeom.verify_refit(bad)).all()                               # what the non-finite stop looks at


def test_top_and_pick_by_hand():
    counts = np.zeros((2, 3, 10), np.int32)
    nm = np.array([[2, 0, 1], [0, 0, 0]], np.int32)
    counts[0, 0, :3] = (5, 7, 99)                                   # slot 2 is past nmodels: not a model
    counts[0, 2, 0] = 7
    keys = nl.top(counts, nm, 4)
    assert keys[0].tolist() == [(7 << 32) | (nv.M32 - 1), (7 << 32) | (nv.M32 - 20), (5 << 32) | nv.M32, 0] and not keys[1].any()
    E_lo = np.arange(2 * 4 * 9, dtype=np.float64).reshape(2, 4, 9)
    n_lo = np.array([[6, 9, 9, 50], [0, 0, 0, 0]], np.int32)       # candidate 3 has no model: its count does not matter
    rnd = np.array([[-1, 2, 0, 1], [-1, -1, -1, -1]], np.int32)
    E_sel, nm_sel, best_sel, info = nl.pick(keys, E_lo, n_lo, rnd, 3)
    assert info[0].tolist() == [7, 9, 1, 2, 2, 0, 3, 0] and info[1].tolist() == [0, 0, -1, -1, -1, -1, 0, 0]
    assert nm_sel.ravel().tolist() == [1, 0] and best_sel.tolist() == [(9 << 32) | nv.M32, 0]
    assert np.array_equal(E_sel[0, 0, 0], E_lo[0, 1]) and not E_sel[0, 0, 1:].any() and not E_sel[1].any()


# ---- the 27 planted scenes --------------------------------------------------------------------------------------------------------

def test_local_optimisation_never_loses_sampson_inliers(verify):
    """info[:, 2] with lo >= without, on every planted scene, at the default and at the largest setting: candidate 0 is the plain best
    model and round -1 is the model itself."""
    for frac in vc.FRACTIONS:
        for m in vc.SIZES:
            for seed in lc.SEEDS:
                plain = lc.plain_figures(m, frac, seed)[3]
                for T, widen in ((verify.DEFAULT_LO["top"], tuple(verify.DEFAULT_LO["widen"])), (16, lc.widen_of("linear 3 to 1", 8))):
                    assert lc.lo_figures(m, frac, seed, T, widen)[3] >= plain, (frac, m, seed, T, widen)
    out = lc.lo_result(500, 0.5, 1, 4, (2.0, 1.0))                  # and through the composition itself
    case, st = lc.scene(500, 0.5, 1)
    assert out["info"][0, 2] >= st["info"][0, 2] and out["lo_info"][0, 0] == st["info"][0, 2] and out["lo_info"][0, 1] == out["info"][0, 2]
    assert out["info"][0, 1] == st["info"][0, 1] and out["lo_info"][0, 6] == 4 and 0 <= out["lo_info"][0, 2] < 4
    s, j = out["info"][0, 4:6]
    assert nl.top(st["counts"], st["nmodels"], 1)[0, 0] == st["best"][0]
    assert nl.slot_of(nl.top(st["counts"], st["nmodels"], 4)[0, out["lo_info"][0, 2]], lc.BUDGET)[1] == 10 * s + j
    assert lc.figures(case, out) == lc.lo_figures(500, 0.5, 1, 4, (2.0, 1.0))


def test_calibration_of_the_defaults(verify):
    """The table of docs/tracks.md §12.4 (T in 1..16 x R in 1..8 x four schedules, means over the seeds per (share, m)) against
    tests/golden/verify_lo_calibration.json, and `verify.DEFAULT_LO` against the rule."""
    table = lc.calibration()
    want = lc.load_calibration()
    for part in ("plain", "lo"):
        assert sorted(want[part]) == sorted(table[part])
        for key in table[part]:
            assert np.allclose(table[part][key], want[part][key], rtol=0, atol=1e-9, equal_nan=True), (key, table[part][key], want[part][key])
    chosen = lc.chosen_setting(table)
    print("chosen:", chosen)
    for row in sorted(lc.settings_summary(table), key=lambda r: (-r[5], r[0]))[:6]:
        print("runner-up: T*R %d, outlier excess %.5f, T %d, R %d, %s, recall at 30 %% %.4f" % row)
    assert chosen is not None
    assert verify.DEFAULT_LO == dict(top=chosen["top"], rounds=chosen["rounds"], widen=chosen["widen"])
    plain30 = float(np.mean([table["plain"][(0.3, m)][0] for m in vc.SIZES]))
    print(f"mean recall at 30 %: plain {plain30:.4f}, chosen {chosen['recall']:.4f}, best setting tried {chosen['best']:.4f}")
    assert chosen["best"] >= plain30 - 0.02


@pytest.mark.parametrize("m", vc.SIZES)
def test_quality_beside_the_plain_and_the_per_pair_path(verify, m):
    """Means over the three seeds per inlier share: recall of planted inliers, share of planted outliers kept and the angle between the
    returned and the planted rotation, for the default LO, the plain batched path and the per-pair path (the oracle's
    find_essential_mat and recover_pose).  Measured (docs/tracks.md §12.5): at 30 % inliers the default LO equals plain on all nine
    scenes; it is 4.4 points behind the per-pair path at m = 50 (seeds 1 and 2: 60.0 % against 66.7 %), 9.1 points ahead at m = 500 and
    11.9 points behind at m = 5 000 (seed 0: 7.0 % against 31.5 %; seed 2: 30.2 % against 43.7 %).  The aim is asserted where it is met
    (m = 500) and LO >= plain where it is not."""
    T, widen = verify.DEFAULT_LO["top"], tuple(verify.DEFAULT_LO["widen"])
    for frac in vc.FRACTIONS:
        lo = lc.mean_figures(lambda mm, ff, s: lc.lo_figures(mm, ff, s, T, widen), m, frac)
        plain = lc.mean_figures(lc.plain_figures, m, frac)
        pp = lc.mean_figures(lc.per_pair_figures, m, frac)
        print(f"inliers {frac} m {m}: LO recall {lo[0]:.4f} outliers {lo[1]:.5f} rotation {lo[2]:.2f} deg; plain {plain[0]:.4f} / {plain[1]:.5f} / {plain[2]:.2f}; "
              f"per pair {pp[0]:.4f} / {pp[1]:.5f} / {pp[2]:.2f}")
        assert lo[0] >= plain[0] - 0.02
        assert lo[1] <= plain[1] + 0.01
        if frac == 0.3:
            if m in lc.AIM_MET_AT:
                assert lo[0] >= pp[0] - 0.02
            else:
                assert lo[0] >= plain[0]
