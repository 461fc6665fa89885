"""Planted two-view scenes and the calibration of the hypothesis budget, shared by tests/test_verify_cpu.py and
tests/test_gpu_verify.py (docs/tracks.md §11)."""
import functools

import numpy as np

import np_verify as nv

BUDGETS = (32, 64, 128, 256, 512, 1024)          # the issue's five and the largest budget the entry points admit
FRACTIONS = (0.3, 0.5, 0.8)
SIZES = (50, 500, 5000)
WIDTH, HEIGHT = 968.0, 648.0


def dist_bits(d0, d1):
    return np.array([d0, d1], np.float32).view(np.int32)


def planted_pair(m, frac, seed, noise=0.5, cams=(0, 1)):
    """Two of datagen's ring cameras see round(frac * m) scene points (keypoint noise `noise` px); the other queries are matched to a
    uniformly drawn wrong keypoint.  Every query passes the ratio test.  -> dict(store, nq, pairs, img_off, kp, kps, K, planted)."""
    from datagen import load_pose_csv, project, ring_cameras
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng([seed, m, int(round(100 * frac))])
    K, _ = load_pose_csv()
    ring = ring_cameras(8)
    P = [K @ np.c_[Rotation.from_rotvec(ring[c, :3]).as_matrix(), ring[c, 3:]] for c in cams]
    n_in = int(round(frac * m))
    X = rng.normal(size=(n_in, 3))
    X = X / np.maximum(np.linalg.norm(X, axis=1, keepdims=True), 1.0) * rng.uniform(0.2, 1.0, (n_in, 1))
    a = project(P[0], X)[0] + rng.normal(0, noise, (n_in, 2))
    b = project(P[1], X)[0] + rng.normal(0, noise, (n_in, 2))
    lo, hi = [1.0, 1.0], [WIDTH - 1, HEIGHT - 1]
    a = np.vstack([a, rng.uniform(lo, hi, (m - n_in, 2))])
    b = np.vstack([b, rng.uniform(lo, hi, (m - n_in, 2))])
    planted = np.arange(m) < n_in
    oq, ot = rng.permutation(m), rng.permutation(m)                      # query q shows point oq[q], train t shows point ot[t]
    where_t = np.empty(m, np.int64)
    where_t[ot] = np.arange(m)
    store = np.zeros((1, 2, m, 2), np.int32)
    store[0, 0, :, 0] = where_t[oq]
    store[0, 0, :, 1] = (where_t[oq] + 1) % max(m, 1)
    store[0, 1, :] = dist_bits(1.0, 4.0)
    kps = [a[oq].astype(np.float32), b[ot].astype(np.float32)]
    return dict(store=store, nq=np.array([m], np.int32), pairs=np.array([[0, 1]], np.int32), img_off=np.array([0, m, 2 * m], np.int32),
                kp=np.concatenate(kps), kps=kps, K=K, planted=planted[oq])


def rates(keep_row, planted):
    """(recall of planted inliers, share of planted outliers kept)."""
    keep_row = np.asarray(keep_row[:len(planted)]) != 0
    n_in, n_out = int(planted.sum()), int((~planted).sum())
    return (float((keep_row & planted).sum()) / max(n_in, 1), float((keep_row & ~planted).sum()) / max(n_out, 1))


def budget_rates(case, budgets=BUDGETS, seed=0, ratio=0.7):
    """{H: (recall, outlier share)} of the restatement on one planted pair: the models of the largest budget are solved once (sample s
    does not depend on the budget) and every smaller budget scores its prefix."""
    H = max(budgets)
    st = nv.verify_pairs(case["store"], case["nq"], case["pairs"], case["img_off"], case["kp"], case["K"], ratio, budget=H, seed=seed, stages=True)
    out = {}
    for h in budgets:
        nm, E = st["nmodels"][:, :h], st["E_all"][:, :h]
        live = np.arange(nv.SLOTS)[None, None, :] < nm[:, :, None]
        c = st["counts"][:, :h].astype(np.uint64)
        slot = (nv.SLOTS * np.arange(h)[None, :, None] + np.arange(nv.SLOTS)[None, None, :]).astype(np.uint64)
        keys = np.where(live, (c << np.uint64(32)) | (np.uint64(nv.M32) - slot), np.uint64(0))
        best = keys.reshape(len(nm), -1).max(1)
        keep = nv.select(np.ascontiguousarray(E), np.ascontiguousarray(nm), best, st["surv"], st["m"], case["pairs"], case["img_off"], st["xn"], st["thr2"])[0]
        out[h] = rates(keep[0], case["planted"])
    return out


@functools.lru_cache(maxsize=None)
def calibration(seeds=(0, 1, 2), sizes=SIZES, fractions=FRACTIONS, budgets=BUDGETS):
    """{(frac, m, H): (mean recall, mean outlier share, spread of recall over the seeds, spread of outlier share)}."""
    table = {}
    for frac in fractions:
        for m in sizes:
            per_seed = [budget_rates(planted_pair(m, frac, s), budgets, seed=s) for s in seeds]
            for h in budgets:
                r = np.array([ps[h] for ps in per_seed])
                table[(frac, m, h)] = (float(r[:, 0].mean()), float(r[:, 1].mean()), float(np.ptp(r[:, 0])), float(np.ptp(r[:, 1])))
    return table


CALIBRATION_JSON = "verify_calibration.json"


def calibration_rows(table):
    return [dict(inliers=f, m=m, budget=h, recall=v[0], outliers_kept=v[1], recall_spread=v[2], outliers_spread=v[3]) for (f, m, h), v in sorted(table.items())]


def load_calibration():
    """The committed table (tests/golden/verify_calibration.json: `calibration()` as tests/test_verify_cpu.py recomputes it)."""
    import json
    import os
    from datagen import GOLDEN
    rows = json.load(open(os.path.join(GOLDEN, CALIBRATION_JSON)))["rows"]
    return {(r["inliers"], r["m"], r["budget"]): (r["recall"], r["outliers_kept"], r["recall_spread"], r["outliers_spread"]) for r in rows}


def smallest_sufficient_budget(table, frac=0.3, sizes=SIZES, budgets=BUDGETS, point=0.01):
    """The smallest H past which neither figure improves by more than one point on the scenes of `frac`: the means over the sizes.
    When the rule does not settle inside `budgets` the last one is returned: the cap, past which nothing was measured."""
    rec = {h: np.mean([table[(frac, m, h)][0] for m in sizes]) for h in budgets}
    out = {h: np.mean([table[(frac, m, h)][1] for m in sizes]) for h in budgets}
    for k, h in enumerate(budgets):
        later = budgets[k + 1:]
        if all(rec[g] - rec[h] <= point and out[h] - out[g] <= point for g in later):
            return h
    return budgets[-1]


def format_table(table, sizes=SIZES, fractions=FRACTIONS, budgets=BUDGETS):
    lines = ["| inliers | m | " + " | ".join(f"H = {h}" for h in budgets) + " |", "|---|---|" + "---|" * len(budgets)]
    for frac in fractions:
        for m in sizes:
            cells = [f"{100 * table[(frac, m, h)][0]:.1f} / {100 * table[(frac, m, h)][1]:.1f}" for h in budgets]
            lines.append(f"| {frac} | {m} | " + " | ".join(cells) + " |")
    return "\n".join(lines)
