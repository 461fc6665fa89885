"""The calibration of the local optimisation on the planted two-view scenes of tests/verify_cases.py, shared by
tests/test_verify_lo_cpu.py and tests/test_gpu_verify_lo.py (docs/tracks.md §12.4)."""
import functools
import json
import os

import numpy as np

import np_verify as nv
import np_verify_lo as nl
import verify_cases as vc

TOPS = (1, 2, 4, 8, 16)
ROUNDS = (1, 2, 4, 8)
SCHEDULES = ("constant 1", "constant 2", "constant 3", "linear 3 to 1")
SEEDS = (0, 1, 2)
BUDGET = 1024
CALIBRATION_JSON = "verify_lo_calibration.json"
# docs/tracks.md §12.5: the m at which the restatement meets the aim "no more than two points behind the per-pair path at 30 % inliers"
AIM_MET_AT = (500,)


def widen_of(schedule, R):
    """The R multipliers of the threshold."""
    if schedule.startswith("constant"):
        return (float(schedule.split()[1]),) * R
    return tuple(float(w) for w in np.linspace(3.0, 1.0, R))        # R = 1: (3,)


def planted_rotation(cams=(0, 1)):
    from datagen import ring_cameras
    from scipy.spatial.transform import Rotation
    ring = ring_cameras(8)
    R0, R1 = (Rotation.from_rotvec(ring[c, :3]).as_matrix() for c in cams)
    return R1 @ R0.T


def rotation_error_deg(Rt_row, R_true):
    """The angle between the returned rotation and the planted one, in degrees; nan without a model."""
    R = np.asarray(Rt_row, np.float64).reshape(3, 4)[:, :3]
    if not R.any():
        return float("nan")
    c = (np.trace(R.T @ R_true) - 1.0) / 2.0
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))


@functools.lru_cache(maxsize=None)
def scene(m, frac, seed):
    """(case, the staged plain result) of one planted scene at the default budget; the seed draws the scene and the samples."""
    case = vc.planted_pair(m, frac, seed)
    st = nv.verify_pairs(case["store"], case["nq"], case["pairs"], case["img_off"], case["kp"], case["K"], 0.7, budget=BUDGET, seed=seed, stages=True)
    return case, st


def figures(case, out):
    """(recall, outliers kept, rotation error in degrees, Sampson inliers) of a result on a one-pair scene."""
    r = vc.rates(out["keep"][0], case["planted"])
    return r[0], r[1], rotation_error_deg(out["Rt"][0], planted_rotation()), int(out["info"][0, 2])


def plain_figures(m, frac, seed):
    case, st = scene(m, frac, seed)
    return figures(case, st)


def lo_result(m, frac, seed, T, widen):
    case, st = scene(m, frac, seed)
    return nl.verify_pairs(case["store"], case["nq"], case["pairs"], case["img_off"], case["kp"], case["K"], 0.7, budget=BUDGET, seed=seed, lo_top=T,
                           widen=widen, plain=st)


@functools.lru_cache(maxsize=None)
def _candidates(m, frac, seed, widen):
    """The 16 candidates of a scene under one schedule: a candidate does not depend on how many stand beside it."""
    case, st = scene(m, frac, seed)
    keys = nl.top(st["counts"], st["nmodels"], max(TOPS))
    part = (st["surv"], st["m"], case["pairs"], case["img_off"], st["xn"])
    return keys, nl.lo(st["E_all"], keys, *part, st["thr2"], nl.wide2_of(case["K"], 0.4, widen))


@functools.lru_cache(maxsize=None)
def _selected(m, frac, seed, widen, win):
    """figures of the scene when candidate `win` of the schedule wins."""
    case, st = scene(m, frac, seed)
    keys, cand = _candidates(m, frac, seed, widen)
    part = (st["surv"], st["m"], case["pairs"], case["img_off"], st["xn"])
    sel = nl.pick(keys[:, win:win + 1].copy(), *(c[:, win:win + 1].copy() for c in cand), BUDGET)
    keep, Eb, Rt, info = nv.select(sel[0], sel[1], sel[2], *part, st["thr2"])
    return figures(case, dict(keep=keep, Rt=Rt, info=info))


def lo_figures(m, frac, seed, T, widen):
    keys, cand = _candidates(m, frac, seed, tuple(widen))
    info = nl.pick(np.ascontiguousarray(keys[:, :T]), *(np.ascontiguousarray(c[:, :T]) for c in cand), BUDGET)[3]
    win = int(info[0, 2])
    if win < 0:
        case, _ = scene(m, frac, seed)
        return 0.0, 0.0, float("nan"), 0
    return _selected(m, frac, seed, tuple(widen), win)


def mean_figures(fn, m, frac):
    """The means over the seeds of (recall, outliers kept, rotation error); the rotation error over the seeds that have a model."""
    rows = np.array([fn(m, frac, s)[:3] for s in SEEDS], np.float64)
    rot = rows[:, 2][~np.isnan(rows[:, 2])]
    return float(rows[:, 0].mean()), float(rows[:, 1].mean()), float(rot.mean()) if len(rot) else float("nan")


@functools.lru_cache(maxsize=None)
def calibration():
    """{"plain": {(frac, m): (recall, outliers, rotation)}, "lo": {(T, R, schedule, frac, m): (recall, outliers, rotation)}}."""
    plain = {(f, m): mean_figures(plain_figures, m, f) for f in vc.FRACTIONS for m in vc.SIZES}
    lo = {}
    for sched in SCHEDULES:
        for R in ROUNDS:
            w = widen_of(sched, R)
            for T in TOPS:
                for f in vc.FRACTIONS:
                    for m in vc.SIZES:
                        lo[(T, R, sched, f, m)] = mean_figures(lambda mm, ff, s: lo_figures(mm, ff, s, T, w), m, f)
    return dict(plain=plain, lo=lo)


def settings_summary(table, frac=0.3):
    """[(T * R, worst excess of outliers kept over plain, T, R, schedule, mean recall over the nine scenes of `frac`)] of every setting."""
    rows = []
    for sched in SCHEDULES:
        for R in ROUNDS:
            for T in TOPS:
                rec = float(np.mean([table["lo"][(T, R, sched, frac, m)][0] for m in vc.SIZES]))
                excess = max(table["lo"][(T, R, sched, f, m)][1] - table["plain"][(f, m)][1] for f in vc.FRACTIONS for m in vc.SIZES)
                rows.append((T * R, excess, T, R, sched, rec))
    return rows


def chosen_setting(table, point=0.01):
    """The rule: among the settings whose outliers kept stay within a point of plain's on every (share, m) mean, the smallest T * R whose
    mean recall at 30 % is within a point of the best setting tried; on a tie the smaller outlier excess, then the order of the grid."""
    rows = settings_summary(table)
    best = max(r[5] for r in rows)
    ok = [r for r in rows if r[1] <= point and r[5] >= best - point]
    if not ok:
        return None
    tr, excess, T, R, sched, rec = min(ok, key=lambda r: (r[0], r[1]))
    return dict(top=T, rounds=R, widen=widen_of(sched, R), schedule=sched, recall=rec, excess=excess, best=best)


def calibration_rows(table):
    rows = [dict(path="plain", inliers=f, m=m, recall=v[0], outliers_kept=v[1], rotation_deg=v[2]) for (f, m), v in sorted(table["plain"].items())]
    rows += [dict(path="lo", top=T, rounds=R, schedule=s, inliers=f, m=m, recall=v[0], outliers_kept=v[1], rotation_deg=v[2])
             for (T, R, s, f, m), v in sorted(table["lo"].items())]
    return rows


def load_calibration():
    from datagen import GOLDEN
    rows = json.load(open(os.path.join(GOLDEN, CALIBRATION_JSON)))["rows"]
    plain = {(r["inliers"], r["m"]): (r["recall"], r["outliers_kept"], r["rotation_deg"]) for r in rows if r["path"] == "plain"}
    lo = {(r["top"], r["rounds"], r["schedule"], r["inliers"], r["m"]): (r["recall"], r["outliers_kept"], r["rotation_deg"]) for r in rows if r["path"] == "lo"}
    return dict(plain=plain, lo=lo)


def per_pair_figures(m, frac, seed):
    """The per-pair path on the CPU: the oracle's find_essential_mat and recover_pose on the survivors, as `tracks.verify_keep` runs them."""
    from oracle import oracle as O
    case, st = scene(m, frac, seed)
    mp = int(st["m"][0])
    q, t = st["surv"][0, :mp, 0], st["surv"][0, :mp, 1]
    pts0, pts1 = case["kps"][0][q], case["kps"][1][t]
    keep = np.zeros(len(case["planted"]), np.uint8)
    if mp < 5:
        return 0.0, 0.0, float("nan"), 0
    E, mask = O.find_essential_mat(pts0, pts1, case["K"], 0.999, 0.4)
    if E is None:
        return 0.0, 0.0, float("nan"), 0
    first = np.flatnonzero(mask.ravel())
    _, R, tv, mask2 = O.recover_pose(E[:3], pts0[first], pts1[first], case["K"], 50.0, 4)
    keep[q[first[mask2.ravel() != 0]]] = 1
    r = vc.rates(keep, case["planted"])
    return r[0], r[1], rotation_error_deg(np.hstack([R, tv]), planted_rotation()), len(first)
