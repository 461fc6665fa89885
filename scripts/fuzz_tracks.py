"""Randomised parity sweep of the TRACKS family on the GPU box: sfm_match_edges / sfm_track_components / sfm_track_build /
sfm_track_triangulate (through sfm_mvs_amd.tracks, into sentinel-filled buffers) vs the restatement tests/np_tracks.py; every output
compared exactly (float rows as int32 views).

  python scripts/fuzz_tracks.py [seconds] [seed] [family:case_seed]

Families (one case = one random draw; sizes log-uniform from 0 up to a cap that keeps the NumPy side well under a second):
  edges        random match stores (train indices from -1 to past the image, distances with exact ties d0 == ratio * d1, inf, NaN, no
               second neighbour), nq below, at and above cap, pairs that name images outside the range, keep masks or none
  components   edge soups over planted tracks plus random edges: labels against the restatement at a random `rounds`, continued
               with resume until the status says converged; every intermediate state is a valid one
  build        the restatement's converged labels through sfm_track_build with min_len / max_len around the sizes that occur, into
               buffers filled with a sentinel: counts, the counted rows, the sentinel everywhere after them
  triangulate  hand-built tracks over random cameras, counts chained on the device, into sentinel-filled buffers
  composed     a planted all-pairs store with dropped and wrong matches through tracks.run_tracks against the restated composition
One case in four carries a degeneracy: N = 0, ne = 0, every edge invalid (-1, N, INT32_MAX), self-loops and duplicates, a path with
ascending / descending / permuted ids, a hub, one conflicting giant component, empty images, identical cameras (a singular M), a
point behind a camera, NaN and inf keypoints, observations that name no node.
The script stops at the first mismatch, prints the family and the case seed that rebuilds the inputs without a GPU, and exits non-zero.
"""
import os
import sys
import time

os.environ.setdefault("OMP_WAIT_POLICY", "passive")

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import np_tracks as nt

MAX_N, MAX_NE = 1 << 16, 1 << 17
SENTINEL = 0x5A5A5A5A
INT32_MAX = 2 ** 31 - 1
MAX_RESUMES = 400


def log_uniform_from_zero(rng, hi):
    """0 with probability 1/16, else log-uniform over 1..hi."""
    if rng.integers(16) == 0:
        return 0
    return int(min(hi, np.floor(np.exp(rng.uniform(0.0, np.log(hi + 1.0))))))


def gen_offsets(rng, n_img, n):
    """int32 [n_img + 1] from 0 to n, non-decreasing; about one image in five is empty."""
    cuts = np.sort(rng.integers(0, n + 1, n_img - 1)) if n_img > 1 else np.zeros(0, np.int64)
    if n_img > 1 and rng.integers(2):
        dup = rng.random(n_img - 1) < 0.2
        cuts[dup] = cuts[np.maximum(np.flatnonzero(dup) - 1, 0)]
        cuts = np.sort(cuts)
    return np.concatenate([[0], cuts, [n]]).astype(np.int32)


def planted_tracks(rng, img_off, share):
    """Disjoint node lists with at most one node per image: about `share` of the nodes."""
    img_off = np.asarray(img_off, np.int64)
    n_img = len(img_off) - 1
    free = [list(rng.permutation(np.arange(img_off[i], img_off[i + 1]))) for i in range(n_img)]
    tracks, budget = [], int(share * img_off[-1])
    while budget > 0:
        want = int(rng.integers(2, max(3, min(n_img, 12) + 1)))
        imgs = [i for i in rng.permutation(n_img)[:want] if free[i]]
        if len(imgs) < 2:
            break
        tracks.append([int(free[i].pop()) for i in imgs])
        budget -= len(imgs)
    return tracks


def track_edges(rng, tracks, shape):
    out = []
    for t in tracks:
        t = list(rng.permutation(t))
        if shape == 0:                                             # a path
            out += [(t[k], t[k + 1]) for k in range(len(t) - 1)]
        elif shape == 1:                                           # a star
            out += [(t[0], v) for v in t[1:]]
        else:                                                      # all pairs
            out += [(a, b) for k, a in enumerate(t) for b in t[k + 1:]]
    return np.array(out, np.int64).reshape(-1, 2)


def gen_graph(rng, degenerate=None):
    """-> (img_off, edges int32 [ne, 2]).  degenerate: None = one case in four."""
    deg = int(rng.integers(10)) if (rng.integers(4) == 0 if degenerate is None else degenerate) else -1
    n = log_uniform_from_zero(rng, MAX_N)
    n_img = int(rng.choice([1, 2, 3, 5, 17, 64, 65, 300]))
    if deg == 0:
        n = 0
    img_off = gen_offsets(rng, n_img, n)
    if deg == 1 or n == 0:
        ne = 0 if deg == 1 else log_uniform_from_zero(rng, 64)
        return img_off, rng.choice([-1, n, INT32_MAX, 0], (ne, 2)).astype(np.int32)
    if deg in (2, 3, 4):                                           # a path over all nodes: ascending, descending, permuted ids
        ids = np.arange(n) if deg == 2 else np.arange(n)[::-1] if deg == 3 else rng.permutation(n)
        e = np.stack([ids[:-1], ids[1:]], 1)
        return img_off, e[rng.permutation(len(e))].astype(np.int32) if rng.integers(2) else e.astype(np.int32)
    if deg == 5:                                                   # a hub
        hub = int(rng.integers(n))
        return img_off, np.stack([np.full(n, hub), rng.permutation(n)], 1).astype(np.int32)
    tracks = planted_tracks(rng, img_off, rng.uniform(0.1, 1.0))
    e = track_edges(rng, tracks, int(rng.integers(3)))
    extra = log_uniform_from_zero(rng, max(1, min(MAX_NE, n // 4)))
    if deg == 6:                                                   # one conflicting giant component beside the clean tracks
        giant = rng.permutation(n)[:max(2, n // 3)]
        e = np.vstack([e, np.stack([giant[:-1], giant[1:]], 1)])
    elif deg == 7:                                                 # every edge invalid
        e = rng.choice([-1, n, INT32_MAX], (len(e) + 1, 2))
        extra = 0
    elif deg == 8:                                                 # self-loops and duplicates
        e = np.vstack([e, e[:len(e) // 2], e[:len(e) // 3, ::-1], np.repeat(rng.integers(0, n, (extra + 1, 1)), 2, 1)])
    if extra and rng.integers(2):
        e = np.vstack([e, rng.integers(0, n, (extra, 2))])
    e = e.astype(np.int64)
    if len(e) and rng.integers(2):                                 # a quarter of the ends from {-1, N, INT32_MAX}
        bad = rng.random(e.shape) < 0.25
        e[bad] = rng.choice([-1, n, INT32_MAX], int(bad.sum()))
    return img_off, e[rng.permutation(len(e))].astype(np.int32)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def words(t):
    """A device or host array as int32 words on the host."""
    import torch
    if torch.is_tensor(t):
        t = t.detach().cpu().numpy()
    t = np.ascontiguousarray(t)
    return t.view(np.int32) if t.dtype.itemsize == 4 else t.astype(np.int32)


def differ(name, got, want, rows=None):
    """'' when the first `rows` rows of got equal want word for word and the rest still holds the sentinel."""
    g, w = words(got), words(want)
    k = len(w) if rows is None else rows
    if g[:k].shape != w[:k].shape or not np.array_equal(g[:k], w[:k]):
        bad = np.argwhere(g[:k] != w[:k])[:3].tolist() if g[:k].shape == w[:k].shape else "shape"
        return f"{name}: differs at {bad} ({g[:k].shape} vs {w[:k].shape})"
    if rows is not None and not np.all(g[k:] == np.int32(SENTINEL)):
        return f"{name}: written at or past row {k}"
    return ""


def sentinel(shape, dtype):
    import torch
    return torch.full(shape, SENTINEL, dtype=torch.int32, device="cuda").view(dtype)


# ---- families -----------------------------------------------------------------------------------------------------------------

def gen_store(rng):
    deg = int(rng.integers(4)) if rng.integers(4) == 0 else -1
    n_img = int(rng.choice([1, 2, 3, 8, 65]))
    n_pairs = log_uniform_from_zero(rng, 48)
    cap = log_uniform_from_zero(rng, 1024)
    sizes = rng.integers(0, cap + 2, n_img) if deg != 0 else np.zeros(n_img, np.int64)
    img_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    pair = rng.integers(0, n_img, (n_pairs, 2)).astype(np.int32)
    if n_pairs and deg == 1:
        pair[rng.integers(n_pairs)] = rng.choice([-1, n_img, INT32_MAX], 2)
    nq = np.minimum(sizes[np.clip(pair[:, 0], 0, n_img - 1)], cap).astype(np.int32) if n_pairs else np.zeros(0, np.int32)
    if n_pairs and rng.integers(2):
        nq = rng.integers(-1, cap + 3, n_pairs).astype(np.int32)
    ratio = float(rng.choice([0.5, 0.7, 0.75, 1.0, 0.0, np.inf]))
    store = np.zeros((n_pairs, 2, cap, 2), np.int32)
    store[:, 0] = rng.integers(-1, cap + 2, (n_pairs, cap, 2))
    d1 = rng.choice([1.0, 2.0, 3.5, 10.0, np.inf, np.nan, 0.0], (n_pairs, cap), p=[0.3, 0.2, 0.2, 0.2, 0.04, 0.03, 0.03]).astype(np.float32)
    d0 = (d1 * rng.choice([0.25, 0.5, 0.7, 0.75, 0.9, 1.0], (n_pairs, cap))).astype(np.float32)       # ties with 0.5 and 0.75 are exact
    store[:, 1] = np.stack([d0, d1], -1).view(np.int32)
    keep = ((rng.random((n_pairs, cap)) < rng.uniform(0, 1)) * int(rng.choice([1, 255]))).astype(np.uint8) if rng.integers(2) else None
    return store, nq, pair, img_off, ratio, keep


def fuzz_edges(rng):
    from sfm_mvs_amd import tracks
    store, nq, pair, img_off, ratio, keep = gen_store(rng)
    want = nt.match_edges(store, nq, pair, img_off, ratio, keep)
    out = sentinel((len(want) + 3, 2), __import__("torch").int32)
    tracks.match_edges(dev(store), dev(nq), dev(pair), dev(img_off), ratio, None if keep is None else dev(keep), out=out[:len(want)])
    return differ("edges", out, want, rows=len(want))


def converge(edges_dev, n, rounds, final, check_states=True):
    """Labels by batches of `rounds` until the status says converged -> (labels, batches, rounds that lowered a label, message)."""
    from sfm_mvs_amd import tracks
    labels, lowered = None, 0
    for batch in range(1, MAX_RESUMES + 1):
        labels, status = tracks.track_components(edges_dev, n, rounds, labels)
        st = status.cpu().numpy()
        lowered += int(st[1])
        if check_states and not nt.is_valid_state(labels.cpu().numpy(), final):
            return labels, batch, lowered, f"components: batch {batch} left an invalid state"
        if st[0]:
            return labels, batch, lowered, ""
        if st[1] != rounds:
            return labels, batch, lowered, f"components: unconverged after {st[1]} of {rounds} lowering rounds"
    return labels, MAX_RESUMES, lowered, f"components: not converged after {MAX_RESUMES} batches of {rounds}"


def fuzz_components(rng):
    img_off, edges = gen_graph(rng)
    n = int(img_off[-1])
    final = nt.components(edges, n)
    rounds = int(rng.integers(1, 13))
    labels, _, _, msg = converge(dev(edges.reshape(-1, 2)), n, rounds, final)
    return msg or differ("labels", labels, final)


def check_build(img_off, labels, min_len, max_len, want=None):
    import torch
    from sfm_mvs_amd import tracks
    n = len(labels)
    want = nt.build(labels, img_off, min_len, INT32_MAX if max_len is None else max_len) if want is None else want
    node_track, track_off, obs_node, counts = (sentinel((n + 2,), torch.int32), sentinel((n // 2 + 2 + 2,), torch.int32),
                                               sentinel((n + 2,), torch.int32), sentinel((6 + 2,), torch.int32))
    tracks.build_tracks_into(dev(labels), dev(img_off), len(img_off) - 1, min_len, max_len, node_track, track_off, obs_node, counts)
    T, nobs = int(want[3][0]), int(want[3][1])
    return (differ("counts", counts, want[3], rows=6) or differ("node_track", node_track, want[0], rows=n)
            or differ("track_off", track_off, want[1], rows=T + 1) or differ("obs_node", obs_node, want[2], rows=nobs))


def fuzz_build(rng):
    img_off, edges = gen_graph(rng)
    labels = nt.components(edges, int(img_off[-1]))
    sizes = np.unique(np.bincount(labels)) if len(labels) else np.array([2])
    lo = int(max(2, rng.choice(sizes) + rng.integers(-1, 2)))
    hi = None if rng.integers(2) else int(max(lo, rng.choice(sizes) + rng.integers(-1, 2)))
    if rng.integers(3) == 0:
        lo, hi = 2, None
    return check_build(img_off, labels, lo, hi)


def random_cameras(rng, n_img):
    """[n_img, 12] float64: cameras on a ring of radius ~8 that look at the origin, K = (900, 900, 480, 320)."""
    K = np.array([[900.0, 0, 480.0], [0, 900.0, 320.0], [0, 0, 1.0]])
    P = np.empty((n_img, 3, 4))
    for k in range(n_img):
        a = rng.uniform(0, 2 * np.pi)
        C = np.array([8 * np.cos(a), rng.uniform(-1, 1), 8 * np.sin(a)]) * rng.uniform(0.8, 1.3)
        z = -C / np.linalg.norm(C)
        x = np.cross([0.0, 1.0, 0.0], z); x /= np.linalg.norm(x)
        R = np.stack([x, np.cross(z, x), z])
        P[k] = K @ np.c_[R, -R @ C]
    return P.reshape(n_img, 12)


def gen_tri(rng):
    """-> (img_off, kp, P, track_off, obs_node, counts): hand-built tracks over random cameras."""
    deg = int(rng.integers(5)) if rng.integers(4) == 0 else -1
    n_img = int(rng.choice([2, 3, 8, 64, 65]))
    n = max(2, log_uniform_from_zero(rng, 1 << 14))
    img_off = gen_offsets(rng, n_img, n)
    P = random_cameras(rng, n_img)
    if deg == 0:                                                   # identical cameras: M is singular along the ray
        P[:] = P[0]
    tracks = planted_tracks(rng, img_off, rng.uniform(0.2, 1.0))
    tracks = [sorted(t) for t in tracks]
    T = len(tracks)
    track_off = np.concatenate([[0], np.cumsum([len(t) for t in tracks])]).astype(np.int32)
    obs_node = np.array([u for t in tracks for u in t], np.int32)
    X = rng.normal(size=(T, 3)); X /= np.maximum(np.linalg.norm(X, axis=1, keepdims=True), 1.0)
    if deg == 1 and T:                                             # points behind some cameras
        X[rng.random(T) < 0.3] *= 30.0
    kp = rng.uniform(0, 960, (n, 2)).astype(np.float32)
    if len(obs_node):
        tr = np.repeat(np.arange(T), np.diff(track_off))
        Pi = P[nt.image_of(img_off, obs_node)].reshape(-1, 3, 4)
        h = np.einsum("nij,nj->ni", Pi, np.c_[X[tr], np.ones(len(tr))])
        kp[obs_node] = (h[:, :2] / h[:, 2:] + rng.normal(0, rng.choice([0.0, 0.3, 3.0]), (len(tr), 2))).astype(np.float32)
    if deg == 2 and n:
        kp[rng.random(n) < 0.05] = np.nan
    if deg == 3 and n:
        kp[rng.random(n) < 0.05] = rng.choice([np.inf, -np.inf, 1e30])
    if deg == 4 and len(obs_node):                                 # nodes outside 0..N-1 in the list
        obs_node[rng.random(len(obs_node)) < 0.05] = rng.choice([-1, n, INT32_MAX])
    counts = np.array([T, len(obs_node), 0, 0, 0, 0], np.int32)
    return img_off, kp, P, track_off, obs_node, counts, deg


def check_tri(img_off, kp, P, track_off, obs_node, counts):
    import torch
    from sfm_mvs_amd import tracks
    n = int(img_off[-1])
    T, nobs = len(track_off) - 1, len(obs_node)
    want = nt.triangulate(track_off, obs_node, img_off, kp, P)
    cap = n // 2 + 1
    full_off = np.full(n // 2 + 2, SENTINEL, np.int32); full_off[:T + 1] = track_off
    full_obs = np.full(n, SENTINEL, np.int32); full_obs[:nobs] = obs_node
    out = (sentinel((cap, 3), torch.float32), sentinel((n,), torch.float32), sentinel((n,), torch.float32), sentinel((cap,), torch.int32),
           sentinel((cap,), torch.float32))
    tracks.triangulate_tracks(dev(counts), dev(full_off), dev(full_obs), dev(img_off), dev(kp), dev(P), out=out)
    return (differ("X", out[0].reshape(-1), want[0].reshape(-1), rows=3 * T) or differ("err", out[1], want[1], rows=nobs)
            or differ("depth", out[2], want[2], rows=nobs) or differ("flags", out[3], want[3], rows=T) or differ("max_err", out[4], want[4], rows=T))


def fuzz_triangulate(rng):
    img_off, kp, P, track_off, obs_node, counts, _ = gen_tri(rng)
    return check_tri(img_off, kp, P, track_off, obs_node, counts)


def gen_scene(rng):
    """A planted all-pairs store: every image sees a random subset of the scene points; a match is dropped, wrong or right."""
    n_img = int(rng.choice([2, 3, 5, 8]))
    n_scene = log_uniform_from_zero(rng, 300)
    P = random_cameras(rng, n_img)
    X = rng.normal(size=(n_scene, 3)); X /= np.maximum(np.linalg.norm(X, axis=1, keepdims=True), 1.0)
    kps, ids = [], []
    for k in range(n_img):
        seen = np.flatnonzero(rng.random(n_scene) < 0.8)
        h = np.c_[X[seen], np.ones(len(seen))] @ P[k].reshape(3, 4).T
        clutter = int(rng.integers(0, 20))
        kp = np.vstack([h[:, :2] / h[:, 2:] + rng.normal(0, 0.3, (len(seen), 2)), rng.uniform(0, 960, (clutter, 2))]).astype(np.float32)
        order = rng.permutation(len(kp))
        kps.append(kp[order]); ids.append(np.r_[seen, -np.ones(clutter, np.int64)][order])
    pairs = [(i, j) for i in range(n_img) for j in range(i + 1, n_img)]
    cap = max([len(kps[i]) for i, _ in pairs] + [0])
    store = np.zeros((len(pairs), 2, cap, 2), np.int32)
    wrong = rng.choice([0.0, 0.02])
    for p, (i, j) in enumerate(pairs):
        where = {int(s): t for t, s in enumerate(ids[j]) if s >= 0}
        for q, s in enumerate(ids[i]):
            t = where.get(int(s), -1)
            d = (1.0, 4.0) if t >= 0 and rng.random() > 0.1 else (3.0, 4.0)
            if rng.random() < wrong and len(ids[j]):
                t, d = int(rng.integers(len(ids[j]))), (1.0, 4.0)
            store[p, 0, q] = (max(t, 0), 0 if len(ids[j]) > 1 else -1)
            store[p, 1, q] = np.array(d, np.float32).view(np.int32)
    return kps, P, pairs, store, [len(kps[i]) for i, _ in pairs]


def fuzz_composed(rng):
    from sfm_mvs_amd import tracks
    kps, P, pairs, store, nq = gen_scene(rng)
    if not pairs:
        return ""
    kw = dict(min_len=int(rng.choice([2, 3])), max_reproj=[None, 2.0][int(rng.integers(2))])
    got = tracks.run_tracks(dev(store), nq, pairs, [dev(k) for k in kps], P.reshape(-1, 3, 4), rounds=int(rng.integers(1, 13)), **kw)
    img_off = np.concatenate([[0], np.cumsum([len(k) for k in kps])]).astype(np.int32)
    want = nt.run(store, nq, pairs, img_off, np.concatenate(kps), P, **kw)
    if not got["status"][0]:
        return "composed: run_tracks returned unconverged labels"
    for key in ("counts", "points", "obs", "cam_idx", "pt_idx", "track_len"):
        msg = differ(key, got[key].reshape(-1), want[key].reshape(-1))
        if msg:
            return msg
    return ""


FAMILIES = [("edges", fuzz_edges, 2), ("components", fuzz_components, 3), ("build", fuzz_build, 3), ("triangulate", fuzz_triangulate, 2),
            ("composed", fuzz_composed, 1)]


def run(budget, seed, log=print):
    """Cases for `budget` seconds from `seed`; stops at the first mismatch -> (counts per family, mismatches, seconds)."""
    fns = {name: fn for name, fn, _ in FAMILIES}
    rng = np.random.default_rng(seed)
    weights = np.array([w for _, _, w in FAMILIES], float); weights /= weights.sum()
    t0 = time.time(); counts = {name: 0 for name, _, _ in FAMILIES}; bad = 0
    while time.time() - t0 < budget and not bad:
        name = FAMILIES[int(rng.choice(len(FAMILIES), p=weights))][0]
        case_seed = int(rng.integers(1 << 31))
        try:
            msg = fns[name](np.random.default_rng(case_seed))
        except Exception as e:  # noqa: BLE001
            msg = f"EXCEPTION {e!r}"[:300]
        counts[name] += 1
        if msg:
            bad += 1
            log(f"MISMATCH {name} (seed {seed}, case seed {case_seed}; replay: fuzz_tracks.py 0 0 {name}:{case_seed}) {msg}")
    return counts, bad, time.time() - t0


def main():
    import sfm_mvs_amd
    from sfm_mvs_amd import _lib
    budget = float(sys.argv[1]) if len(sys.argv) > 1 else 120.0
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    sfm_mvs_amd.lib()
    if len(sys.argv) > 3:                               # replay one case
        name, case_seed = sys.argv[3].split(":")
        msg = {n: fn for n, fn, _ in FAMILIES}[name](np.random.default_rng(int(case_seed)))
        print(f"fuzz_tracks replay {name}:{case_seed}: {msg or 'no mismatch'}")
        return 1 if msg else 0
    counts, bad, dt = run(budget, seed, log=lambda s: print(s, flush=True))
    print(f"fuzz_tracks: seed {seed}, {sum(counts.values())} cases {counts}, {bad} mismatches, {dt:.0f} s")
    print(f"sfm_build_id {_lib.build_id()}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
