"""Scenes with a known truth for image retrieval and the calibration of its bars, shared by tests/test_retrieval_cpu.py,
tests/test_gpu_retrieval.py, scripts/fuzz_retrieval.py, scripts/bench_retrieval.py and scripts/calibrate_retrieval.py (docs/retrieval.md §5).

`corridor_scene`: a camera walks along a wall of scene points; image i sees the window of points [i * step, i * step + window) and some
clutter of its own, so the number of points two images share falls linearly with their distance and is zero beyond window / step images.
`cluster_scene`: disjoint objects, each seen whole by a ring of cameras; two images either show the same object or share nothing.
The descriptor of a scene point is `sift_like` with integer noise per view.  Descriptors of different scene points are INDEPENDENT draws:
the scenes measure the arithmetic and the bookkeeping, not how well VLAD separates photographs."""
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

import np_retrieval as nr  # noqa: E402
from datagen import load_pose_csv, project, sift_like  # noqa: E402

CALIBRATION_JSON = "retrieval_calibration.json"
CORRIDOR = dict(n_img=48, window=600, step=60, clutter=200)          # the scene of the grid: 1 128 pairs, 38 400 keypoints
GRID_CENTRES = (16, 64)
GRID_SSR = (False, True)
GRID_K = (4, 8, 16)
DEFAULT = dict(n_centres=64, ssr=False, k=8)
TRACK_SCENE = dict(n_img=16, window=120, step=20, clutter=40, seed=0)  # small enough to match all 120 pairs and build tracks in a test
TRACK_SETTING = dict(n_centres=16, ssr=False, k=4)
CLUSTER = dict(n_obj=4, ring=6, n_pts=150, clutter=50)
RATIO = 0.7
DESC_NOISE = 1.5


def _noisy(rng, base):
    return np.clip(base + np.rint(rng.normal(0, DESC_NOISE, base.shape)), 0, 255)


def corridor_scene(n_img, window, step, clutter, seed, permute=True):
    """-> dict(descs, ids, kps, P, K, order): descs[i] float32 [window + clutter, 128], ids[i] the scene point of every keypoint (-1:
    clutter), kps[i] float32 pixels, P[i] the 3 x 4 camera.  order[i] is the position along the corridor of image i: with `permute` the
    images are shuffled, so the index carries no cue."""
    rng = np.random.default_rng([seed, n_img, window, step, clutter])
    K, _ = load_pose_csv()
    n_scene = (n_img - 1) * step + window
    dx = 6.0 / window                                                # a window spans six units at depth five: about the frame's width
    X = np.c_[np.arange(n_scene) * dx + rng.uniform(-0.3, 0.3, n_scene) * dx, rng.uniform(-1.5, 1.5, n_scene), rng.uniform(4.0, 6.0, n_scene)]
    base = sift_like(rng, n_scene)
    order = rng.permutation(n_img) if permute else np.arange(n_img)
    descs, ids, kps, Ps = [], [], [], []
    for pos in order:
        lo = int(pos) * step
        centre = np.array([(lo + 0.5 * window) * dx, 0.0, 0.0])
        P = K @ np.c_[np.eye(3), -centre]
        x = project(P, X[lo:lo + window])[0] + rng.normal(0, 0.3, (window, 2))
        shuffle = rng.permutation(window + clutter)
        descs.append(np.vstack([_noisy(rng, base[lo:lo + window]), sift_like(rng, clutter)])[shuffle].astype(np.float32))
        kps.append(np.vstack([x, rng.uniform([1, 1], [967, 647], (clutter, 2))])[shuffle].astype(np.float32))
        ids.append(np.hstack([np.arange(lo, lo + window), -np.ones(clutter, np.int64)])[shuffle])
        Ps.append(P)
    return dict(descs=descs, ids=ids, kps=kps, P=np.stack(Ps), K=K, order=order)


def cluster_scene(n_obj, ring, n_pts, clutter, seed, permute=True):
    """n_obj disjoint objects of n_pts points, each seen whole by `ring` images -> dict(descs, ids, obj): obj[i] the object of image i."""
    rng = np.random.default_rng([seed, n_obj, ring, n_pts, clutter])
    base = sift_like(rng, n_obj * n_pts)
    obj = np.repeat(np.arange(n_obj), ring)
    if permute:
        obj = obj[rng.permutation(len(obj))]
    descs, ids = [], []
    for o in obj:
        lo = int(o) * n_pts
        shuffle = rng.permutation(n_pts + clutter)
        descs.append(np.vstack([_noisy(rng, base[lo:lo + n_pts]), sift_like(rng, clutter)])[shuffle].astype(np.float32))
        ids.append(np.hstack([np.arange(lo, lo + n_pts), -np.ones(clutter, np.int64)])[shuffle])
    return dict(descs=descs, ids=ids, obj=obj)


def shared_points(ids):
    """int [n_img, n_img]: the scene points two images have in common (the truth of a pair)."""
    n = len(ids)
    sets = [set(int(v) for v in a if v >= 0) for a in ids]
    out = np.zeros((n, n), np.int64)
    for a in range(n):
        for b in range(a + 1, n):
            out[a, b] = out[b, a] = len(sets[a] & sets[b])
    return out


def measures(pairs, shared, k):
    """The three figures of a shortlist: the share of its pairs without a common point, the recall of the pairs whose overlap ranks
    within the k / 2 largest of one of their images (pairs with no common point do not count), the fraction of all pairs it keeps."""
    n = len(shared)
    sel = set((int(a), int(b)) for a, b in pairs)
    wrong = sum(1 for a, b in sel if shared[a, b] == 0)
    near = set()
    for i in range(n):
        rank = sorted((j for j in range(n) if j != i and shared[i, j] > 0), key=lambda j: (-shared[i, j], j))
        near.update((min(i, j), max(i, j)) for j in rank[:k // 2])
    return dict(selected=len(sel), wrong_share=wrong / max(len(sel), 1), recall=len(near & sel) / max(len(near), 1),
                kept_fraction=len(sel) / max(n * (n - 1) // 2, 1))


def all_pairs(n):
    return [(a, b) for a in range(n) for b in range(a + 1, n)]


def oracle_store(descs, pairs):
    """The KNN store of `pairs` by the oracle (the words `sharded.match_pairs_sharded` leaves) -> (store int32 [n_pairs, 2, cap, 2], nq)."""
    from oracle import oracle as O
    cap = max((len(descs[i]) for i, _ in pairs), default=0)
    store = np.zeros((len(pairs), 2, cap, 2), np.int32)
    store[:, 0], store[:, 1] = -1, np.float32(np.inf).view(np.int32)
    for p, (i, j) in enumerate(pairs):
        idx, dist = O.knn2(descs[i], descs[j], nthreads=4)
        store[p, 0, :len(idx)], store[p, 1, :len(idx)] = idx, dist.view(np.int32)
    return store, np.array([len(descs[i]) for i, _ in pairs], np.int32)


def tracks_of(scene, pairs):
    """`np_tracks.run` on the oracle's store of `pairs` -> the result dict (counts[0] = kept tracks)."""
    import np_tracks as nt
    store, nq = oracle_store(scene["descs"], pairs)
    sizes = [len(d) for d in scene["descs"]]
    img_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    return nt.run(store, nq, np.array(pairs, np.int32).reshape(-1, 2), img_off, np.concatenate(scene["kps"]), scene["P"], RATIO)


@functools.lru_cache(maxsize=None)
def track_case():
    """The small corridor with its restated shortlist and both track counts: computed once, never changed."""
    sc = corridor_scene(**TRACK_SCENE)
    pairs, stages = nr.select_pairs(sc["descs"], **TRACK_SETTING)
    full = tracks_of(sc, all_pairs(len(sc["descs"])))
    short = tracks_of(sc, pairs)
    return dict(scene=sc, pairs=pairs, stages=stages, tracks_all=int(len(full["track_len"])), tracks_short=int(len(short["track_len"])),
                result_short=short)


def calibration(seeds=(0, 1, 2)):
    """The rows of tests/golden/retrieval_calibration.json, in a fixed order: the grid on the corridor at seed 0, the default setting on
    every seed, the cluster scene, the track scene."""
    rows = []
    for seed in seeds:
        sc = corridor_scene(seed=seed, **CORRIDOR)
        shared = shared_points(sc["ids"])
        for C in GRID_CENTRES:
            for ssr in GRID_SSR:
                if seed != seeds[0] and (C, ssr) != (DEFAULT["n_centres"], DEFAULT["ssr"]):
                    continue
                centres = None
                for k in GRID_K:
                    pairs, st = nr.select_pairs(sc["descs"], k=k, n_centres=C, ssr=ssr, centres=centres)
                    centres = st["centres"]
                    clip = int((np.abs(st["sig"].astype(np.int32)) == 127).sum())
                    rows.append(dict(scene="corridor", seed=seed, n_centres=C, ssr=ssr, k=k, clipped=clip, **measures(pairs, shared, k)))
    cl = cluster_scene(seed=0, **CLUSTER)
    for k in (2, CLUSTER["ring"] - 1):
        pairs, _ = nr.select_pairs(cl["descs"], k=k, n_centres=16)
        crossing = sum(1 for a, b in pairs if cl["obj"][a] != cl["obj"][b])
        rows.append(dict(scene="cluster", seed=0, n_centres=16, ssr=False, k=k, selected=len(pairs), crossing=crossing))
    tc = track_case()
    rows.append(dict(scene="tracks", seed=TRACK_SCENE["seed"], k=TRACK_SETTING["k"], n_centres=TRACK_SETTING["n_centres"], ssr=False,
                     selected=len(tc["pairs"]), tracks_all=tc["tracks_all"], tracks_short=tc["tracks_short"],
                     track_fraction=tc["tracks_short"] / max(tc["tracks_all"], 1),
                     **{k_: v for k_, v in measures(tc["pairs"], shared_points(tc["scene"]["ids"]), TRACK_SETTING["k"]).items() if k_ != "selected"}))
    return rows


def load_calibration():
    with open(os.path.join(HERE, "golden", CALIBRATION_JSON)) as f:
        return json.load(f)["rows"]


def row_of(rows, **where):
    hits = [r for r in rows if all(r.get(k) == v for k, v in where.items())]
    assert len(hits) == 1, (where, len(hits))
    return hits[0]
