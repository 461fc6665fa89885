"""Randomised parity sweep of the TRACKS-REGISTER family on the GPU box: sfm_track_restrict / sfm_track_adopt / sfm_track_view_scores /
sfm_track_correspondences (through sfm_mvs_amd.register, into sentinel-filled buffers) vs the restatement tests/np_tracks_register.py;
every output compared exactly (float rows as int32 views, NaN equal to NaN).

  python scripts/fuzz_tracks_register.py [seconds] [seed] [family:case_seed]

Families (one case = one random draw; sizes log-uniform from 0):
  restrict         hand-built tracks (fuzz_tracks' planted node lists) over 1..257 images, a random registered set, min_len 1..4
  adopt            the restated restriction of such a table, then a hand-made prune (a random subset of the tracks, a random subset of
                   their observations, random point words) composed back onto the full table
  scores           a random has_point over the table, keypoints in and around the frame, grid 1..8, both sides of SFM_REGISTER_LDS_IMAGES
  correspondences  the same tables, one image (empty ones included), a capacity at, below and above the count
  composed         restrict -> triangulate -> refine -> prune -> adopt -> scores -> correspondences on the device, the counts chained
                   there, against the restated chain
One case in four carries a degeneracy: no node, nobody or everybody registered, observations that name no node (-1, N, INT32_MAX),
track indices outside 0..T-1 in node_track and in both track_src, NaN and infinite keypoints, has_point none or all.
The script stops at the first mismatch, prints the family and the case seed that rebuilds the inputs without a GPU, and exits non-zero.
"""
import os
import sys
import time

os.environ.setdefault("OMP_WAIT_POLICY", "passive")

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "scripts"))
import np_tracks as nt
import np_tracks_refine as nr
import np_tracks_register as ng
import fuzz_tracks as fz
from fuzz_tracks import INT32_MAX, SENTINEL, dev, differ, log_uniform_from_zero

BYTE = SENTINEL & 0xFF
FRAME = (968.0, 648.0)
IMAGES = (1, 2, 3, 8, 64, 65, 256, 257)
MAX_NODES = 1 << 14
PAD = 2                                                                    # sentinel rows kept behind every output


def buffer(rows, dtype, width=None):
    """(whole, view): `rows` rows in front of PAD sentinel rows, every byte 0x5A."""
    import torch
    shape = (rows + PAD,) if width is None else (rows + PAD, width)
    nbytes = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
    whole = torch.full((nbytes,), BYTE, dtype=torch.uint8, device="cuda").view(dtype).view(shape)
    return whole, whole[:rows]


def same(name, whole, want, rows):
    """'' when the first `rows` rows of the buffer equal `want` byte for byte and every later byte still is the sentinel."""
    g = whole.detach().cpu().numpy()
    g = g.reshape(g.shape[0], -1).view(np.uint8)
    w = np.ascontiguousarray(want)
    w = w.reshape(rows, -1).view(np.uint8) if rows else np.zeros((0, g.shape[1]), np.uint8)
    if g[:rows].shape != w.shape or not np.array_equal(g[:rows], w):
        bad = np.argwhere((g[:rows] != w).any(axis=1))[:3].ravel().tolist() if g[:rows].shape == w.shape else "shape"
        return f"{name}: differs at rows {bad} ({g[:rows].shape} vs {w.shape})"
    return "" if np.all(g[rows:] == BYTE) else f"{name}: written at or past row {rows}"


def padded(a, size, dtype=np.int32):
    """`a` in front of sentinel bytes, as the device buffers of capacity `size` hold it."""
    out = np.full(size * np.dtype(dtype).itemsize, BYTE, np.uint8).view(dtype)
    out[:len(a)] = np.asarray(a, dtype)
    return out


def planted_tracks(rng, img_off, share):
    """fuzz_tracks.planted_tracks (disjoint node lists, at most one node per image, about `share` of the nodes) that goes on after a draw
    of images without a free node: twenty such draws in a row end it."""
    img_off = np.asarray(img_off, np.int64)
    n_img = len(img_off) - 1
    free = [list(rng.permutation(np.arange(img_off[i], img_off[i + 1]))) for i in range(n_img)]
    tracks, budget, fails = [], int(share * img_off[-1]), 0
    while budget > 0 and fails < 20:
        want = int(rng.integers(2, max(3, min(n_img, 12) + 1)))
        imgs = [i for i in rng.permutation(n_img)[:want] if free[i]]
        if len(imgs) < 2:
            fails += 1
            continue
        fails = 0
        tracks.append([int(free[i].pop()) for i in imgs])
        budget -= len(imgs)
    return tracks


def gen_table(rng, n_img=None, n=None, deg=None, max_nodes=MAX_NODES):
    """-> dict: a table in the shape sfm_track_build leaves (unpadded), node_track, keypoints, and the degeneracy drawn."""
    deg = (int(rng.integers(6)) if rng.integers(4) == 0 else -1) if deg is None else deg
    n_img = int(rng.choice(IMAGES)) if n_img is None else n_img
    n = (0 if deg == 0 else log_uniform_from_zero(rng, max_nodes)) if n is None else n
    img_off = fz.gen_offsets(rng, n_img, n)
    tracks = [sorted(t) for t in planted_tracks(rng, img_off, rng.uniform(0.2, 1.0))] if n else []
    T = len(tracks)
    track_off = np.concatenate([[0], np.cumsum([len(t) for t in tracks])]).astype(np.int32)
    obs_node = np.array([u for t in tracks for u in t], np.int32)
    node_track = np.full(n, -1, np.int32)
    if len(obs_node):
        node_track[obs_node] = np.repeat(np.arange(T), np.diff(track_off))
    kp = np.stack([rng.uniform(-40, FRAME[0] + 40, n), rng.uniform(-40, FRAME[1] + 40, n)], 1).astype(np.float32)
    if deg == 1 and len(obs_node):                                         # observations that name no node
        obs_node[rng.random(len(obs_node)) < 0.25] = rng.choice([-1, n, INT32_MAX])
    if deg == 2 and n:                                                     # track indices outside 0..T-1
        node_track[rng.random(n) < 0.25] = rng.choice([-5, T, INT32_MAX])
    if deg == 3 and n:
        kp[rng.random(n) < 0.2, int(rng.integers(2))] = rng.choice([np.nan, np.inf, -np.inf, 1e30, -1e30])
    counts = np.array([T, len(obs_node), 0, 0, 0, 0], np.int32)
    reg = (rng.random(n_img) < rng.uniform(0, 1)).astype(np.uint8) * rng.choice(np.uint8([1, 1, 255]))
    if deg == 4:
        reg[:] = rng.integers(2)                                           # nobody or everybody
    has = (rng.random(n // 2 + 1) < rng.uniform(0, 1)).astype(np.uint8) * rng.choice(np.uint8([1, 7]))
    if deg == 5:
        has[:] = rng.integers(2)
    return dict(n=n, n_img=n_img, img_off=img_off, track_off=track_off, obs_node=obs_node, node_track=node_track, kp=kp, counts=counts, T=T,
                registered=reg, has_point=has, deg=deg)


def device_table(t):
    n = t["n"]
    return dict(counts=dev(t["counts"]), track_off=dev(padded(t["track_off"], n // 2 + 2)), obs_node=dev(padded(t["obs_node"], n)),
                img_off=dev(t["img_off"]), node_track=dev(t["node_track"]), kp=dev(t["kp"].reshape(n, 2)))


def restrict_buffers(n):
    import torch
    return [buffer(n // 2 + 2, torch.int32), buffer(n, torch.int32), buffer(n // 2 + 1, torch.int32), buffer(4, torch.int32)]


def check_restrict(t, registered, min_len, d=None):
    from sfm_mvs_amd import register
    n = t["n"]
    d = d or device_table(t)
    want = ng.restrict(t["counts"], t["track_off"], t["obs_node"], t["img_off"], registered, n, min_len)
    bufs = restrict_buffers(n)
    register.restrict_tracks(d["counts"], d["track_off"], d["obs_node"], d["img_off"], dev(np.asarray(registered, np.uint8)), min_len,
                             out=tuple(v for _, v in bufs))
    T2, nobs2 = int(want[3][0]), int(want[3][1])
    return (same("counts2", bufs[3][0], want[3], 4) or same("track_off2", bufs[0][0], want[0], T2 + 1) or same("obs_node2", bufs[1][0], want[1], nobs2)
            or same("track_src", bufs[2][0], want[2], T2))


def fuzz_restrict(rng):
    t = gen_table(rng)
    return check_restrict(t, t["registered"], int(rng.choice([1, 2, 2, 3, 4])))


def gen_adopt(rng, t=None):
    """-> (table, restricted (restated), a hand-made prune of it: counts_p, off_p, obs_p, X_p, src_p)."""
    t = t or gen_table(rng)
    r = ng.restrict(t["counts"], t["track_off"], t["obs_node"], t["img_off"], t["registered"], t["n"], 2)
    T2 = int(r[3][0])
    keep = np.flatnonzero(rng.random(T2) < rng.uniform(0, 1))
    off_p, obs_p = [0], []
    for q in keep:
        rows = np.arange(r[0][q], r[0][q + 1])
        rows = rows[rng.random(len(rows)) < 0.8]
        obs_p += r[1][rows].tolist()
        off_p.append(len(obs_p))
    X_p = rng.normal(size=(len(keep), 3)).astype(np.float32)
    if len(keep):
        X_p[rng.random(len(keep)) < 0.05] = np.nan                         # a payload NaN is copied as it is
    src_p, src_r = keep.astype(np.int32), r[2].copy()
    if t["deg"] == 2 and len(src_p):                                       # track indices outside their tables
        src_p[rng.random(len(src_p)) < 0.2] = rng.choice([-1, T2, INT32_MAX])
        if len(src_r):
            src_r[rng.random(len(src_r)) < 0.1] = rng.choice([-1, t["T"], INT32_MAX])
    c_p = np.array([len(keep), len(obs_p), 0, 0], np.int32)
    return t, (r[0], r[1], src_r, r[3]), (c_p, np.array(off_p, np.int32), np.array(obs_p, np.int32), X_p, src_p)


def adopt_buffers(n):
    import torch
    return [buffer(n // 2 + 1, torch.float32, 3), buffer(n // 2 + 1, torch.uint8), buffer(n, torch.uint8)]


def check_adopt(t, r, p, d=None):
    from sfm_mvs_amd import register
    n, cap = t["n"], t["n"] // 2 + 1
    d = d or device_table(t)
    want = ng.adopt(t["counts"], t["track_off"], t["obs_node"], n, r[3], r[2], p[0], p[1], p[2], p[3], p[4])
    restricted = (dev(padded(r[0], cap + 1)), dev(padded(r[1], n)), dev(padded(r[2], cap)), dev(r[3]))
    pruned = (dev(padded(p[1], cap + 1)), dev(padded(p[2], n)), dev(padded(p[3].reshape(-1), 3 * cap, np.float32).reshape(cap, 3)), dev(padded(p[4], cap)),
              dev(p[0]))
    bufs = adopt_buffers(n)
    register.adopt_points(d["counts"], d["track_off"], d["obs_node"], restricted, pruned, out=tuple(v for _, v in bufs))
    T, nobs = ng.clamped(t["counts"], n)
    return same("X_full", bufs[0][0], want[0], T) or same("has_point", bufs[1][0], want[1], T) or same("obs_live", bufs[2][0], want[2], nobs)


def fuzz_adopt(rng):
    return check_adopt(*gen_adopt(rng))


def check_scores(t, has, grid, frame=FRAME, d=None):
    import torch
    from sfm_mvs_amd import register
    n, n_img = t["n"], t["n_img"]
    d = d or device_table(t)
    want = ng.view_scores(t["counts"], t["node_track"], has, t["img_off"], t["kp"], n, frame[0], frame[1], grid)
    bufs = [buffer(n_img, torch.int32), buffer(n_img, torch.int64), buffer(n_img, torch.int32)]
    register.view_scores(d["counts"], d["node_track"], dev(np.asarray(has, np.uint8)), d["img_off"], d["kp"], frame, grid, out=tuple(v for _, v in bufs))
    return same("seen", bufs[0][0], want[0], n_img) or same("cover", bufs[1][0], want[1], n_img) or same("cells", bufs[2][0], want[2], n_img)


def fuzz_scores(rng):
    t = gen_table(rng)
    return check_scores(t, t["has_point"], int(rng.integers(1, 9)), (float(rng.choice([968.0, 1.0, 4000.5])), float(rng.choice([648.0, 3.0, 3000.25]))))


def check_corr(t, has, X_full, image, capacity=None, d=None):
    import torch
    from sfm_mvs_amd import register
    n = t["n"]
    d = d or device_table(t)
    want = ng.correspondences(image, t["counts"], t["node_track"], has, X_full, t["img_off"], t["kp"], n)
    k = len(want[2])
    capacity = k if capacity is None else capacity
    bufs = [buffer(capacity, torch.float32, 3), buffer(capacity, torch.float32, 2), buffer(capacity, torch.int32), buffer(1, torch.int32)]
    register.correspondences(image, d["counts"], d["node_track"], dev(np.asarray(has, np.uint8)), dev(np.asarray(X_full, np.float32).reshape(n // 2 + 1, 3)),
                             d["img_off"], d["kp"], capacity, out=tuple(v for _, v in bufs))
    rows = min(k, capacity)
    seen = ng.view_scores(t["counts"], t["node_track"], has, t["img_off"], t["kp"], n, FRAME[0], FRAME[1], 8)[0]
    if t["deg"] != 2 and int(seen[image]) != k:                            # (garbage node_track aside, img_off is ascending: both count the same nodes)
        return f"correspondences: {k} rows but seen[{image}] = {int(seen[image])}"
    return (same("count", bufs[3][0], np.array([k], np.int32), 1) or same("X_out", bufs[0][0], want[0][:rows], rows)
            or same("uv_out", bufs[1][0], want[1][:rows], rows) or same("track_out", bufs[2][0], want[2][:rows], rows))


def fuzz_correspondences(rng):
    t = gen_table(rng)
    X_full = rng.normal(size=(t["n"] // 2 + 1, 3)).astype(np.float32)
    X_full[rng.random(len(X_full)) < 0.05] = np.nan
    image = int(rng.integers(t["n_img"]))
    k = len(ng.correspondences(image, t["counts"], t["node_track"], t["has_point"], X_full, t["img_off"], t["kp"], t["n"])[2])
    return check_corr(t, t["has_point"], X_full, image, int(rng.choice([k, k, max(k - 1, 0), k // 2, k + 3])))


def gen_round(rng, max_nodes=1 << 11):
    """fuzz_tracks' hand-built tracks over random cameras with a registered set: the input of one model round."""
    img_off, kp, P, track_off, obs_node, counts, deg = fz.gen_tri(rng)
    n = int(img_off[-1])
    if n > max_nodes:                                                      # keeps the restated refinement well under a second
        keep = int(np.searchsorted(track_off, max_nodes // 2, side="right")) - 1
        track_off, counts = track_off[:keep + 1], counts.copy()
        obs_node = obs_node[:track_off[-1]]
        counts[:2] = (keep, len(obs_node))
    node_track = np.full(n, -1, np.int32)
    ok = (obs_node >= 0) & (obs_node < n)
    node_track[obs_node[ok]] = np.repeat(np.arange(len(track_off) - 1), np.diff(track_off))[ok]
    reg = (rng.random(len(img_off) - 1) < rng.uniform(0.3, 1.0)).astype(np.uint8)
    return dict(n=n, n_img=len(img_off) - 1, img_off=img_off, track_off=track_off, obs_node=obs_node, node_track=node_track, kp=kp, counts=counts,
                T=len(track_off) - 1, registered=reg, deg=-1, P=P)


def restated_round(t, reg, P, min_len=2, max_reproj=2.0, max_cos=1.0, huber=1.0, obs_thresh=2.0, iters=10, grid=8, frame=FRAME):
    n = t["n"]
    with np.errstate(all="ignore"):
        r = ng.restrict(t["counts"], t["track_off"], t["obs_node"], t["img_off"], reg, n, min_len)
        X, _, _, flags, _ = nt.triangulate(r[0], r[1], t["img_off"], t["kp"], P)
        rf = nr.refine(r[0], r[1], t["img_off"], t["kp"], P, X, flags, huber, obs_thresh, iters)
        p = nr.prune(r[0], r[1], rf[0], rf[1], rf[4], rf[5], rf[6], rf[8], min_len, max_reproj, max_cos)
        a = ng.adopt(t["counts"], t["track_off"], t["obs_node"], n, r[3], r[2], p[4], p[0], p[1], p[2], p[3])
        s = ng.view_scores(t["counts"], t["node_track"], a[1], t["img_off"], t["kp"], n, frame[0], frame[1], grid)
    return r, p, a, s


def device_round(t, d, reg, P, min_len=2, max_reproj=2.0, max_cos=1.0, huber=1.0, obs_thresh=2.0, iters=10, grid=8, frame=FRAME):
    """The chain of a model round into sentinel-filled buffers, the counts chained on the device -> (restricted, pruned, adopted, scores) buffers."""
    import torch
    from sfm_mvs_amd import register, tracks
    n, n_img, cap = t["n"], t["n_img"], t["n"] // 2 + 1
    Pd = dev(np.asarray(P, np.float64).reshape(n_img, 12))
    rb = restrict_buffers(n)
    r = register.restrict_tracks(d["counts"], d["track_off"], d["obs_node"], d["img_off"], dev(np.asarray(reg, np.uint8)), min_len, out=tuple(v for _, v in rb))
    X, _, _, flags, _ = tracks.triangulate_tracks(r[3], r[0], r[1], d["img_off"], d["kp"], Pd)
    rf = tracks.refine_tracks(r[3], r[0], r[1], d["img_off"], d["kp"], Pd, X, flags, huber, obs_thresh, iters)
    pb = [buffer(cap + 1, torch.int32), buffer(n, torch.int32), buffer(cap, torch.float32, 3), buffer(cap, torch.int32), buffer(4, torch.int32)]
    p = tracks.prune_tracks(r[3], r[0], r[1], rf[0], rf[1], rf[4], rf[5], rf[6], rf[8], min_len, max_reproj, None, max_cos, out=tuple(v for _, v in pb))
    ab = adopt_buffers(n)
    a = register.adopt_points(d["counts"], d["track_off"], d["obs_node"], r, p, out=tuple(v for _, v in ab))
    sb = [buffer(n_img, torch.int32), buffer(n_img, torch.int64), buffer(n_img, torch.int32)]
    register.view_scores(d["counts"], d["node_track"], a[1], d["img_off"], d["kp"], frame, grid, out=tuple(v for _, v in sb))
    return rb, pb, ab, sb


def compare_round(t, got, want):
    rb, pb, ab, sb = got
    r, p, a, s = want
    T, nobs = ng.clamped(t["counts"], t["n"])
    T2, nobs2, Tp, nobs_p = int(r[3][0]), int(r[3][1]), int(p[4][0]), int(p[4][1])
    return (same("counts_r", rb[3][0], r[3], 4) or same("track_off_r", rb[0][0], r[0], T2 + 1) or same("obs_node_r", rb[1][0], r[1], nobs2)
            or same("track_src_r", rb[2][0], r[2], T2) or same("counts_p", pb[4][0], p[4], 4) or same("track_off_p", pb[0][0], p[0], Tp + 1)
            or same("obs_node_p", pb[1][0], p[1], nobs_p) or same("X_p", pb[2][0], p[2], Tp) or same("track_src_p", pb[3][0], p[3], Tp)
            or same("X_full", ab[0][0], a[0], T) or same("has_point", ab[1][0], a[1], T) or same("obs_live", ab[2][0], a[2], nobs)
            or same("seen", sb[0][0], s[0], t["n_img"]) or same("cover", sb[1][0], s[1], t["n_img"]) or same("cells", sb[2][0], s[2], t["n_img"]))


def fuzz_composed(rng):
    t = gen_round(rng)
    if t["n"] == 0:
        return ""
    kw = dict(min_len=int(rng.choice([2, 3])), max_reproj=float(rng.choice([2.0, np.inf])), max_cos=float(rng.choice([1.0, np.cos(np.deg2rad(2.0))])),
              iters=int(rng.choice([3, 10])), grid=int(rng.choice([1, 4, 8])))
    P = t["P"].copy()
    P[t["registered"] == 0] = 0.0                                          # rows of unregistered images are never read
    d = device_table(t)
    want = restated_round(t, t["registered"], P, **kw)
    got = device_round(t, d, t["registered"], P, **kw)
    msg = compare_round(t, got, want)
    if msg:
        return msg
    image = int(rng.integers(t["n_img"]))
    X_full = np.full((t["n"] // 2 + 1, 3), np.nan, np.float32)
    X_full[:len(want[2][0])] = want[2][0]
    has = np.zeros(t["n"] // 2 + 1, np.uint8)
    has[:len(want[2][1])] = want[2][1]
    return check_corr(t, has, X_full, image, d=d)


FAMILIES = [("restrict", fuzz_restrict, 3), ("adopt", fuzz_adopt, 3), ("scores", fuzz_scores, 3), ("correspondences", fuzz_correspondences, 3),
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
            log(f"MISMATCH {name} (seed {seed}, case seed {case_seed}; replay: fuzz_tracks_register.py 0 0 {name}:{case_seed}) {msg}")
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
        print(f"fuzz_tracks_register replay {name}:{case_seed}: {msg or 'no mismatch'}")
        return 1 if msg else 0
    counts, bad, dt = run(budget, seed, log=lambda s: print(s, flush=True))
    print(f"fuzz_tracks_register: seed {seed}, {sum(counts.values())} cases {counts}, {bad} mismatches, {dt:.0f} s")
    print(f"sfm_build_id {_lib.build_id()}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
