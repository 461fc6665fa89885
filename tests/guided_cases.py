"""Scenes with repeated structure and the calibration of the guided threshold, shared by tests/test_guided_cpu.py,
tests/test_gpu_guided.py, scripts/fuzz_guided.py and scripts/bench_guided.py (docs/tracks.md §14.4).

A scene is `datagen.ring_scene`'s (cameras of `ring_cameras` with the K of pose.csv, points of the unit ball, SIFT-like descriptors with
integer noise per view, clutter, shuffled per image) with one addition: a fraction of the scene points has a TWIN, a second 3-D point
elsewhere in the ball that carries the same descriptor.  The global ratio test rejects a point and its twin in every pair (the second
neighbour is as close as the first), while their epipolar lines differ."""
import functools
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import np_guided as ng  # noqa: E402
import np_tracks as nt  # noqa: E402
import np_verify as nv  # noqa: E402
from datagen import load_pose_csv, project, ring_cameras, sift_like  # noqa: E402

TWINS = (0.0, 0.25, 0.5)
SIZES = (50, 500, 2000)
SEEDS = (0, 1, 2)
MULTIPLES = (1, 2, 4, 8)                         # of the verification threshold
VERIFY_THRESHOLD = 0.4
RING_IMAGES = 4                                  # the ring scenes of the table: six pairs each
TRACK_SCENE = (6, 500, 0.25, 0)                  # one ring of six images more: the scene tests/test_gpu_guided.py feeds through run_tracks
BUDGET = 128                                     # hypotheses per pair of the calibration's verifications
RATIO = 0.7
CALIBRATION_JSON = "guided_calibration.json"


def twin_scene(n_images, n_kp, twin, seed, desc_noise=1.5, pix_noise=0.3, ring=8):
    """n_images cameras of an 8-camera ring; every image holds all scene points and clutter, n_kp keypoints in all.  0.6 n_kp points have
    a descriptor of their own, `twin` of those a twin.  -> dict(K, P, kps, descs, ids, kp, desc, img_off, pairs, nq, sizes)."""
    from scipy.spatial.transform import Rotation
    K, _ = load_pose_csv()
    cams = ring_cameras(ring)
    rng = np.random.default_rng([seed, n_kp, int(100 * twin), n_images])
    nb = int(0.6 * n_kp)
    tw = int(twin * nb)
    n_scene = nb + tw

    def ball(n):
        X = rng.normal(size=(n, 3))
        return X / np.maximum(np.linalg.norm(X, axis=1, keepdims=True), 1.0) * rng.uniform(0.2, 1.0, (n, 1))

    X = np.vstack([ball(nb), ball(tw)])
    base = sift_like(rng, nb)
    base = np.vstack([base, base[rng.permutation(nb)[:tw]]])
    P = np.stack([K @ np.c_[Rotation.from_rotvec(cams[k, :3]).as_matrix(), cams[k, 3:]] for k in range(n_images)])
    kps, descs, ids = [], [], []
    for k in range(n_images):
        x = project(P[k], X)[0] + rng.normal(0, pix_noise, (n_scene, 2))
        des = np.clip(base + np.rint(rng.normal(0, desc_noise, base.shape)), 0, 255)
        nc = n_kp - n_scene
        order = rng.permutation(n_kp)
        kps.append(np.vstack([x, rng.uniform([1, 1], [967, 647], (nc, 2))])[order].astype(np.float32))
        descs.append(np.vstack([des, sift_like(rng, nc)])[order].astype(np.float32))
        ids.append(np.hstack([np.arange(n_scene), -np.ones(nc, np.int64)])[order])
    pairs = np.array([(i, j) for i in range(n_images) for j in range(i + 1, n_images)], np.int32)
    sizes = np.full(n_images, n_kp)
    return dict(K=K, P=P, kps=kps, descs=descs, ids=ids, kp=np.concatenate(kps), desc=np.concatenate(descs),
                img_off=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32), pairs=pairs, nq=np.full(len(pairs), n_kp, np.int32), sizes=sizes,
                n_twin=tw)


def global_store(scene):
    """The KNN store of every pair by the oracle (the words `sharded.match_pairs_sharded` leaves): int32 [n_pairs, 2, n_kp, 2]."""
    from oracle import oracle as O
    cap = int(scene["sizes"].max())
    store = np.empty((len(scene["pairs"]), 2, cap, 2), np.int32)
    for p, (i, j) in enumerate(scene["pairs"]):
        idx, dist = O.knn2(scene["descs"][i], scene["descs"][j], nthreads=4)
        store[p, 0], store[p, 1] = idx, dist.view(np.int32)
    return store


@functools.lru_cache(maxsize=None)
def case(n_images, n_kp, twin, seed):
    """A scene with its global store: computed once, never changed (copy before editing)."""
    scene = twin_scene(n_images, n_kp, twin, seed)
    scene["store"] = global_store(scene)
    return scene


def edge_mask(store, nq, pairs, img_off, keep, ratio=RATIO):
    """bool [n_pairs, cap]: the queries `match_edges(store, keep=keep)` turns into edges."""
    edges = nt.match_edges(store, nq, pairs, img_off, ratio, keep).reshape(len(pairs), -1, 2)
    return edges[:, :, 0] >= 0


def tally(scene, store, keep, ratio=RATIO):
    """(correct, wrong, full-length tracks) of the edges of (store, keep): an edge is correct when both ends show one scene point."""
    mask = edge_mask(store, scene["nq"], scene["pairs"], scene["img_off"], keep, ratio)
    correct = wrong = 0
    for p, (i, j) in enumerate(scene["pairs"]):
        q = np.flatnonzero(mask[p])
        t = store[p, 0, q, 0]
        good = (scene["ids"][i][q] >= 0) & (scene["ids"][i][q] == scene["ids"][j][t])
        correct += int(good.sum())
        wrong += int((~good).sum())
    res = nt.run(store, scene["nq"], scene["pairs"], scene["img_off"], scene["kp"], scene["P"], ratio, keep)
    return correct, wrong, int((res["track_len"] == len(scene["kps"])).sum())


def scene_rows(scene, seed, multiples=MULTIPLES, budget=BUDGET):
    """{"plain" | (multiple, mutual): (correct, wrong, full tracks)} of one scene; the first verification is shared by all settings and
    the guided store of a multiple by its two mutual settings."""
    a = (scene["nq"], scene["pairs"], scene["img_off"], scene["kp"], scene["K"])
    first = nv.verify_pairs(scene["store"], *a, RATIO, VERIFY_THRESHOLD, budget, seed)
    out = {"plain": tally(scene, scene["store"], first["keep"])}
    for k in multiples:
        g = ng.guided_pairs(scene["desc"], *a, first["E"], first["info"], k * VERIFY_THRESHOLD, MIN_INLIERS, True, cap=scene["store"].shape[2])
        second = nv.verify_pairs(g["store"], *a, RATIO, VERIFY_THRESHOLD, budget, seed)
        out[(k, True)] = tally(scene, g["store"], second["keep"] & g["keep"])
        out[(k, False)] = tally(scene, g["store"], second["keep"])
        out[("stores", k)] = (first, g, second)
    return out


MIN_INLIERS = 8


@functools.lru_cache(maxsize=None)
def rows_of(n_images, n_kp, twin, seed):
    """`scene_rows` of a scene of the table: computed once, never changed."""
    return scene_rows(case(n_images, n_kp, twin, seed), seed)


def scene_list():
    """(images, keypoints, twin share, seed) of every scene of the table."""
    return [(n, m, tw, s) for n in (2, RING_IMAGES) for m in SIZES for tw in TWINS for s in SEEDS] + [TRACK_SCENE]


def calibration(scenes=None):
    """[dict(images, m, twin, seed, setting, correct, wrong, tracks)] over the table's scenes, in a fixed order."""
    rows = []
    for n, m, tw, s in scene_list() if scenes is None else scenes:
        res = rows_of(n, m, tw, s)
        for setting in ["plain"] + [(k, mu) for k in MULTIPLES for mu in (False, True)]:
            c, w, tr = res[setting]
            name = "plain" if setting == "plain" else f"x{setting[0]}{' mutual' if setting[1] else ''}"
            rows.append(dict(images=n, m=m, twin=tw, seed=s, setting=name, correct=c, wrong=w, tracks=tr))
    return rows


def load_calibration():
    with open(os.path.join(HERE, "golden", CALIBRATION_JSON)) as f:
        return json.load(f)["rows"]


def setting_name(multiple, mutual):
    return f"x{multiple}{' mutual' if mutual else ''}"


def totals(rows, setting, key="correct", **where):
    return sum(r[key] for r in rows if r["setting"] == setting and all(r[k] == v for k, v in where.items()))


def class_totals(rows, multiple):
    """{(images, m): correct matches of the mutual path at `multiple`}, the twin shares and seeds of a scene class pooled."""
    return {cls: totals(rows, setting_name(multiple, True), images=cls[0], m=cls[1]) for cls in sorted(set((r["images"], r["m"]) for r in rows))}


def default_multiple(rows, point=0.01):
    """The rule of docs/tracks.md §14.4: the smallest multiple of the grid after which the correct matches of the mutual path grow by no
    more than `point` of their value at that multiple IN EVERY SCENE CLASS (images, keypoints an image); the last one when the rule does
    not settle inside the grid.  A class is not pooled with the others: a pooled sum is the sum of the largest scenes, and the default
    has to serve an image of 50 keypoints as it serves one of 2 000."""
    c = {k: class_totals(rows, k) for k in MULTIPLES}
    for n, k in enumerate(MULTIPLES):
        if all(c[later][cls] <= c[k][cls] * (1 + point) for later in MULTIPLES[n + 1:] for cls in c[k]):
            return k
    return MULTIPLES[-1]


def wrong_share(rows, setting, **where):
    c, w = totals(rows, setting, "correct", **where), totals(rows, setting, "wrong", **where)
    return w / max(c + w, 1)


def format_table(rows):
    lines = ["| images | m | twins | plain | " + " | ".join(setting_name(k, mu) for k in MULTIPLES for mu in (False, True)) + " |",
             "|---|---|---|---|" + "---|" * (2 * len(MULTIPLES))]
    for n in (2, RING_IMAGES):
        for m in SIZES:
            for tw in TWINS:
                cells = []
                for setting in ["plain"] + [setting_name(k, mu) for k in MULTIPLES for mu in (False, True)]:
                    w = dict(images=n, m=m, twin=tw)
                    cells.append(f"{totals(rows, setting, 'correct', **w)} / {totals(rows, setting, 'wrong', **w)} / {totals(rows, setting, 'tracks', **w)}")
                lines.append(f"| {n} | {m} | {tw} | " + " | ".join(cells) + " |")
    return "\n".join(lines)


if __name__ == "__main__":                       # python tests/guided_cases.py: recompute and write the table
    import time
    t0 = time.time()
    rows = calibration()
    with open(os.path.join(HERE, "golden", CALIBRATION_JSON), "w") as f:
        json.dump(dict(budget=BUDGET, verify_threshold=VERIFY_THRESHOLD, ratio=RATIO, min_inliers=MIN_INLIERS, rows=rows), f, indent=0)
    print(format_table(rows))
    print(f"default multiple {default_multiple(rows)}; {time.time() - t0:.0f} s")
