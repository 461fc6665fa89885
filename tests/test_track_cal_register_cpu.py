"""`register.register_loop(calibrate=...)` without a GPU (docs/tracks.md §15): on the NumPy engine of tests/register_cases.py, given the
calibrated adjustment of tests/np_track_cal.py.  calibrate=None runs the loop as before; with it the FINAL adjustment is the calibrated
one, always runs, and the result carries K and dist."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import np_track_cal as nc  # noqa: E402
import register_cases as rc  # noqa: E402


class CalEngine(rc.NumpyEngine):
    """NumpyEngine with the calibrated adjustment of the restatement; counts the calls of both adjustments."""
    plain = calibrated = 0

    def bundle(self, *a, **kw):
        self.plain += 1
        assert self.calibrated == 0, "an adjustment after the calibrated one"
        return super().bundle(*a, **kw)

    def bundle_calibrated(self, order, P, model, calibrate, huber=1.0, iters=15, **kw):
        self.calibrated += 1
        X, obs, cam, pt = self._model()
        rank = np.full(self.n_img, -1, np.int32)
        rank[np.asarray(order)] = np.arange(len(order))
        cams, _, K_new, dist, hist, info = nc.bundle_adjust(rc.cams_of(np.asarray(P)[np.asarray(order)], self.K), self.K, calibrate.get("dist"), X.astype(np.float64),
                                                            obs, rank[cam], pt, free=calibrate.get("free", ("f", "k1")), huber=huber, iters=iters, **kw)
        return rc.P_of(cams, K_new), hist, dict(info, K=K_new, dist=dist)


def test_the_final_adjustment_is_the_calibrated_one_and_the_rounds_before_it_are_untouched():
    from sfm_mvs_amd import register
    case = rc.scene("ring_corrupted")
    K = np.asarray(case["K"], np.float64)
    eng0 = CalEngine(case)
    base = register.register_loop(eng0, eng0.n_img, case["pairs"], K)
    assert eng0.calibrated == 0 and eng0.plain == len(base["ba_history"]) and "K" not in base and "dist" not in base
    wrong = K.copy()
    wrong[0, 0] *= 1.03
    wrong[1, 1] *= 1.03                                                                                # a focal length 3 % off, the aspect kept
    runs = {}
    for name, cal in (("fixed", None), ("free", dict(free=("f",)))):
        eng = CalEngine(case)
        eng.K = wrong
        out = register.register_loop(eng, eng.n_img, case["pairs"], wrong, calibrate=cal)
        runs[name] = (out, eng)
    (fixed, e_fixed), (free, e_free) = runs["fixed"], runs["free"]
    assert e_fixed.calibrated == 0 and e_free.calibrated == 1 and "K" not in fixed
    assert free["order"].tolist() == fixed["order"].tolist() and free["steps"] == fixed["steps"]       # the registrations are the same
    n = min(len(fixed["ba_history"]), len(free["ba_history"])) - 1
    assert fixed["ba_history"][:n] == free["ba_history"][:n] and len(free["ba_history"]) >= len(fixed["ba_history"])
    f_new = free["K"][0, 0]
    print(f"register_loop(calibrate): f {wrong[0, 0]:.2f} -> {f_new:.2f} (true {K[0, 0]:.2f}); final cost {free['ba_history'][-1][-1]:.6g} against {fixed['ba_history'][-1][-1]:.6g} with K fixed")
    assert abs(f_new / K[0, 0] - 1) < 0.5 * 0.03 and free["K"][1, 1] / f_new == pytest.approx(K[1, 1] / K[0, 0], rel=1e-12) and not free["dist"].any()
    assert free["ba_history"][-1][-1] < fixed["ba_history"][-1][-1]
    o = free["order"]
    assert np.allclose(np.linalg.solve(free["K"], free["P"][o[0]])[:, :3], np.linalg.solve(wrong, fixed["P"][o[0]])[:, :3], atol=1e-9)   # P rows are K' [R | t]
    with pytest.raises(register.SfmHipError):
        register.register_tracks(None, None, [(0, 1)], [None, None], K, (960, 640), calibrate=dict(fre=("f",)))
