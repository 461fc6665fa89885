"""Planted general, planar and rotating two-view scenes and the calibration of the homography's defaults, shared by
tests/test_verify_h_cpu.py and tests/test_gpu_verify_h.py (docs/tracks.md §13)."""
import functools
import json
import os

import numpy as np

import np_verify as nv
import np_verify_h as nh
import verify_cases as vc
import verify_lo_cases as lc

KINDS = ("general", "planar", "rotating")
PLANTED_CONFIG = dict(general=nh.CONFIG_GENERAL, planar=nh.CONFIG_PLANAR, rotating=nh.CONFIG_ROTATING)
THRESHOLDS = (0.4, 0.8, 1.2, 1.6, 2.0)          # pixels
SEEDS = lc.SEEDS
BUDGET = lc.BUDGET
TURN = 0.25                                     # radians, the rotating pair's second camera about its own centre
ASSERTED_FRACTIONS, ASSERTED_SIZES = (0.5, 0.8), (500, 5000)
CALIBRATION_JSON = "verify_h_calibration.json"
MIN_INLIERS, REFIT = 8, 1


def cameras(kind):
    """(K, [R | t] of the first camera, of the second, the plane's unit normal or None)."""
    from datagen import load_pose_csv, ring_cameras
    from scipy.spatial.transform import Rotation
    K, _ = load_pose_csv()
    ring = ring_cameras(8)
    Rt = [np.c_[Rotation.from_rotvec(ring[c, :3]).as_matrix(), ring[c, 3:]] for c in (0, 1)]
    n = None
    if kind == "planar":
        C = [-rt[:, :3].T @ rt[:, 3] for rt in Rt]
        n = C[0] / np.linalg.norm(C[0]) + C[1] / np.linalg.norm(C[1])     # the bisector of the two viewing directions: both face it
        n = n / np.linalg.norm(n)
    if kind == "rotating":
        D = Rotation.from_rotvec([0.0, TURN, 0.0]).as_matrix()
        Rt[1] = D @ Rt[0]                                                 # the same centre: t2 = D t1
    return K, Rt[0], Rt[1], n


def planted_pair_h(kind, m, frac, seed, noise=0.5):
    """`verify_cases.planted_pair` with the scene of `kind`: "general" is that function unchanged; "planar" projects the same points onto
    a plane through the origin that both cameras face; "rotating" turns the first camera by 0.25 rad about its own centre to make the
    second.  The random stream is planted_pair's, so the three kinds share points, noise, outliers and permutations."""
    if kind == "general":
        return vc.planted_pair(m, frac, seed, noise)
    from datagen import project
    K, Rt0, Rt1, n = cameras(kind)
    rng = np.random.default_rng([seed, m, int(round(100 * frac))])
    n_in = int(round(frac * m))
    X = rng.normal(size=(n_in, 3))
    X = X / np.maximum(np.linalg.norm(X, axis=1, keepdims=True), 1.0) * rng.uniform(0.2, 1.0, (n_in, 1))
    if n is not None:
        X = X - (X @ n)[:, None] * n[None, :]
    a = project(K @ Rt0, X)[0] + rng.normal(0, noise, (n_in, 2))
    b = project(K @ Rt1, X)[0] + rng.normal(0, noise, (n_in, 2))
    lo, hi = [1.0, 1.0], [vc.WIDTH - 1, vc.HEIGHT - 1]
    a = np.vstack([a, rng.uniform(lo, hi, (m - n_in, 2))])
    b = np.vstack([b, rng.uniform(lo, hi, (m - n_in, 2))])
    planted = np.arange(m) < n_in
    oq, ot = rng.permutation(m), rng.permutation(m)
    where_t = np.empty(m, np.int64)
    where_t[ot] = np.arange(m)
    store = np.zeros((1, 2, m, 2), np.int32)
    store[0, 0, :, 0] = where_t[oq]
    store[0, 0, :, 1] = (where_t[oq] + 1) % max(m, 1)
    store[0, 1, :] = vc.dist_bits(1.0, 4.0)
    kps = [a[oq].astype(np.float32), b[ot].astype(np.float32)]
    return dict(store=store, nq=np.array([m], np.int32), pairs=np.array([[0, 1]], np.int32), img_off=np.array([0, m, 2 * m], np.int32),
                kp=np.concatenate(kps), kps=kps, K=K, planted=planted[oq])


RING_TURN = 0.1                                 # radians: the ring scene's ninth image is its first, turned about its own centre


@functools.lru_cache(maxsize=None)
def ring_with_a_turned_camera():
    """tests/register_cases.py's ring scene with a ninth image taken from the first camera's centre after a turn of 0.1 rad: every keypoint
    of image 0 moved by the rotation's homography K D K^-1, with its descriptor.  Pair (0, 8) shares more tracks than any other pair and
    has no baseline.  -> the case dict of test_tracks_cpu.finish_case."""
    from scipy.spatial.transform import Rotation
    import register_cases as rc
    case = rc.scene("ring")
    ids = rc._split(case)
    K = np.asarray(case["K"], np.float64).reshape(3, 3)
    D = Rotation.from_rotvec([0.0, RING_TURN, 0.0]).as_matrix()
    G = K @ D @ np.linalg.inv(K)
    x = np.c_[case["kps"][0].astype(np.float64), np.ones(len(case["kps"][0]))] @ G.T
    turned = (x[:, :2] / x[:, 2:]).astype(np.float32)
    P8 = K @ D @ np.linalg.inv(K) @ case["P"][0]
    return rc._remake(case, case["kps"] + [turned], case["des"] + [case["des"][0]], ids + [ids[0]], np.concatenate([case["P"], P8[None]]))


def planted_homography(kind):
    """The K-normalised homography x2 ~ H x1 of the planar and of the rotating scene, scaled to a middle singular value of 1."""
    K, Rt0, Rt1, n = cameras(kind)
    R = Rt1[:, :3] @ Rt0[:, :3].T
    if kind == "rotating":
        return R
    t = Rt1[:, 3] - R @ Rt0[:, 3]
    n0 = Rt0[:, :3] @ n                                                   # the plane n . X = 0 in the first camera: n0 . x = n0 . t0
    H = R + np.outer(t, n0) / float(n0 @ Rt0[:, 3])
    return H / np.linalg.svd(H, compute_uv=False)[1]


@functools.lru_cache(maxsize=None)
def scene(kind, m, frac, seed):
    """(case, the staged plain result at the default budget, (ok, Hm) of its samples); the seed draws the scene and the samples."""
    if kind == "general":
        case, st = lc.scene(m, frac, seed)
    else:
        case = planted_pair_h(kind, m, frac, seed)
        st = nv.verify_pairs(case["store"], case["nq"], case["pairs"], case["img_off"], case["kp"], case["K"], 0.7, budget=BUDGET, seed=seed, stages=True)
    part = (st["surv"], st["m"], case["pairs"], case["img_off"], st["xn"])
    return case, st, nh.models(st["samp"], *part)


@functools.lru_cache(maxsize=None)
def scene_row(kind, m, frac, seed, threshold, refit=REFIT):
    """The figures of one scene at one threshold of the homography."""
    case, st, (ok, Hm) = scene(kind, m, frac, seed)
    part = (st["surv"], st["m"], case["pairs"], case["img_off"], st["xn"])
    thr2h = nv.thr2_of(case["K"], threshold)
    counts, best = nh.score(Hm, ok, *part, thr2h)
    keep_h, H_out, sv, h_info = nh.select(Hm, ok, best, *part, thr2h, refit)
    rec_h, out_h = vc.rates(keep_h[0], case["planted"])
    rec_e, out_e = vc.rates(st["keep"][0], case["planted"])
    with np.errstate(all="ignore"):
        spread = float(sv[0, 0] / sv[0, 2])
    return dict(kind=kind, inliers=frac, m=m, seed=seed, threshold=threshold, n_E=int(st["info"][0, 2]), n_H=int(h_info[0, 2]), n_sample=int(h_info[0, 3]),
                refit_won=int(h_info[0, 5] == 0), spread=spread if np.isfinite(spread) else None, recall_h=rec_h, outliers_h=out_h, recall_e=rec_e,
                outliers_e=out_e)


def calibration(thresholds=THRESHOLDS):
    """Every scene (3 kinds x 3 shares x 3 sizes x 3 seeds) at every threshold of the grid: a list of `scene_row`s."""
    return [scene_row(kind, m, frac, seed, thr) for kind in KINDS for frac in vc.FRACTIONS for m in vc.SIZES for seed in SEEDS for thr in thresholds]


def load_calibration():
    from datagen import GOLDEN
    return json.load(open(os.path.join(GOLDEN, CALIBRATION_JSON)))["rows"]


def _asserted(r):
    return r["inliers"] in ASSERTED_FRACTIONS and r["m"] in ASSERTED_SIZES


def chosen_threshold(rows):
    """The smallest threshold of the grid at which, on every (share, m) of the asserted scenes, the planar scenes' mean recall of planted
    inliers by keep_h is not below the general scenes' mean recall by keep.  -> (threshold or None, {threshold: [(share, m, recall_h,
    recall_e, outliers_h)]})."""
    table = {}
    for thr in sorted({r["threshold"] for r in rows}):
        cells = []
        for frac in ASSERTED_FRACTIONS:
            for m in ASSERTED_SIZES:
                pl = [r for r in rows if r["threshold"] == thr and r["kind"] == "planar" and r["inliers"] == frac and r["m"] == m]
                ge = [r for r in rows if r["threshold"] == thr and r["kind"] == "general" and r["inliers"] == frac and r["m"] == m]
                cells.append((frac, m, float(np.mean([r["recall_h"] for r in pl])), float(np.mean([r["recall_e"] for r in ge])),
                              float(np.mean([r["outliers_h"] for r in pl]))))
        table[thr] = cells
    ok = [thr for thr, cells in table.items() if all(c[2] >= c[3] for c in cells)]
    return (min(ok) if ok else None), table


def separation(rows, threshold, what):
    """what = "ratio": n_H / n_E, general (largest) against planar and rotating (smallest); "spread": sv0 / sv2, rotating (largest) against
    planar (smallest); over the asserted scenes at `threshold`.  -> dict(low=, high=, value= their geometric mean, factor= high / low)."""
    at = [r for r in rows if r["threshold"] == threshold and _asserted(r)]
    if what == "ratio":
        val = lambda r: r["n_H"] / max(r["n_E"], 1)                       # noqa: E731
        low = max(val(r) for r in at if r["kind"] == "general")
        high = min(val(r) for r in at if r["kind"] != "general")
    else:
        val = lambda r: r["spread"] if r["spread"] is not None else float("inf")      # noqa: E731
        low = max(val(r) for r in at if r["kind"] == "rotating")
        high = min(val(r) for r in at if r["kind"] == "planar")
    return dict(low=float(low), high=float(high), value=float(np.sqrt(low * high)), factor=float(high / low))


def classify_row(r, settings):
    """The configuration word the rule gives a scene's figures."""
    if r["n_E"] < settings["min_inliers"]:
        return nh.CONFIG_NONE
    if r["n_H"] < np.float64(settings["min_ratio"]) * np.float64(r["n_E"]):
        return nh.CONFIG_GENERAL
    if r["spread"] is not None and r["spread"] <= settings["rot_spread"]:
        return nh.CONFIG_ROTATING
    return nh.CONFIG_PLANAR


def chosen_defaults(rows):
    thr, _ = chosen_threshold(rows)
    if thr is None:
        return None
    return dict(threshold=thr, min_ratio=round(separation(rows, thr, "ratio")["value"], 3), rot_spread=round(separation(rows, thr, "spread")["value"], 3),
                min_inliers=MIN_INLIERS, refit=REFIT)


def misclassified(rows, settings):
    """The scenes at the settings' threshold whose word is not the planted one: [(kind, share, m, seed, word)]."""
    return [(r["kind"], r["inliers"], r["m"], r["seed"], classify_row(r, settings)) for r in rows
            if r["threshold"] == settings["threshold"] and classify_row(r, settings) != PLANTED_CONFIG[r["kind"]]]


def format_table(rows, threshold):
    lines = ["| kind | inliers | m | n_H / n_E (seeds 0, 1, 2) | sv0 / sv2 | recall by keep_h / outliers kept | refit won |", "|---|---|---|---|---|---|---|"]
    for kind in KINDS:
        for frac in vc.FRACTIONS:
            for m in vc.SIZES:
                rs = sorted((r for r in rows if r["threshold"] == threshold and r["kind"] == kind and r["inliers"] == frac and r["m"] == m), key=lambda r: r["seed"])
                ratio = ", ".join(f"{r['n_H'] / max(r['n_E'], 1):.2f}" for r in rs)
                spread = ", ".join("-" if r["spread"] is None else f"{r['spread']:.2f}" for r in rs)
                lines.append(f"| {kind} | {frac} | {m} | {ratio} | {spread} | {100 * np.mean([r['recall_h'] for r in rs]):.1f} / "
                             f"{100 * np.mean([r['outliers_h'] for r in rs]):.1f} | {sum(r['refit_won'] for r in rs)} of {len(rs)} |")
    return "\n".join(lines)
