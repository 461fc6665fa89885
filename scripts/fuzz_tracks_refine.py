"""Randomised parity sweep of the TRACKS-REFINE family on the GPU box: sfm_track_refine / sfm_track_prune (through sfm_mvs_amd.tracks,
into sentinel-filled buffers) vs the restatement tests/np_tracks_refine.py; every output compared exactly (float rows as int32 views).

  python scripts/fuzz_tracks_refine.py [seconds] [seed] [family:case_seed]

Families (one case = one random draw; sizes log-uniform from 0 up to a cap that keeps the NumPy side well under a second):
  refine    hand-built tracks over random cameras with pixel noise and one displaced keypoint in a quarter of them, triangulated on the
            device and refined with random huber (inf included), obs_thresh, iters and iters2 (0 included), counts chained on the device
  prune     random per-track and per-observation arrays (flags 0..3, NaN errors, cosines around the bound, inlier bytes 0 / 1 / 255)
            with min_len, max_reproj (inf included) and max_cos around the values that occur
  composed  a planted all-pairs store with dropped and wrong matches and displaced keypoints through tracks.run_tracks(robust=True)
            against the restated composition
One case in four carries a degeneracy: no node, identical cameras (a zero determinant), points close to or behind a camera (a trial
step that would cross it), NaN and inf keypoints, observations that name no node, a NaN start point, a start with flag bit 1 clear,
every observation displaced.
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
import fuzz_tracks as fz
from fuzz_tracks import SENTINEL, dev, differ, log_uniform_from_zero, sentinel

BYTE = SENTINEL & 0xFF
MAX_NODES = 1 << 12


def differ_bytes(name, got, want, rows):
    g = got.detach().cpu().numpy()
    if not np.array_equal(g[:rows], np.asarray(want, np.uint8)):
        return f"{name}: differs at {np.argwhere(g[:rows] != want)[:3].tolist()}"
    return "" if np.all(g[rows:] == BYTE) else f"{name}: written at or past row {rows}"


def padded(a, size):
    """`a` in front of sentinel words, as the device buffers of capacity `size` hold it."""
    out = np.full(size, SENTINEL, np.int32)
    out[:len(a)] = np.asarray(a, np.int32)
    return out


def refine_buffers(n):
    import torch
    cap = n // 2 + 1
    return (sentinel((cap, 3), torch.float32), torch.full((n + 8,), BYTE, dtype=torch.uint8, device="cuda")[:n], sentinel((n,), torch.float32),
            sentinel((n,), torch.float32), sentinel((cap,), torch.int32), sentinel((cap,), torch.float32), sentinel((cap,), torch.float32),
            sentinel((cap,), torch.int32), sentinel((cap,), torch.int32))


def compare_refine(out, want, T, nobs):
    names = ("X", "inlier", "err", "depth", "n_inl", "max_err", "cos_min", "steps", "flags")
    for k, name in enumerate(names):
        rows = nobs if k in (1, 2, 3) else 3 * T if k == 0 else T
        msg = differ_bytes(name, out[k], want[k], rows) if k == 1 else differ(name, out[k].reshape(-1), np.asarray(want[k]).reshape(-1), rows=rows)
        if msg:
            return msg
    return ""


def check_refine(img_off, kp, P, track_off, obs_node, counts, X_in=None, flags_in=None, **params):
    """Triangulate on the device (or take X_in / flags_in [T]), refine into sentinel-filled buffers, compare with the restatement."""
    from sfm_mvs_amd import tracks
    n, T, nobs = int(img_off[-1]), len(track_off) - 1, len(obs_node)
    args = (dev(counts), dev(padded(track_off, n // 2 + 2)), dev(padded(obs_node, n)), dev(img_off), dev(np.asarray(kp, np.float32).reshape(n, 2)),
            dev(np.asarray(P, np.float64).reshape(-1, 12)))
    X, _, _, flags, _ = tracks.triangulate_tracks(*args)
    if X_in is not None:
        X[:T] = dev(np.asarray(X_in, np.float32).reshape(T, 3))
        flags[:T] = dev(np.asarray(flags_in, np.int32))
    out = refine_buffers(n)
    tracks.refine_tracks(*args, X, flags, out=out, **params)
    want = nr.refine(track_off, obs_node, img_off, kp, P, X[:T].cpu().numpy(), flags[:T].cpu().numpy(), **params)
    return compare_refine(out, want, T, nobs), out, want


def gen_refine(rng):
    """-> (img_off, kp, P, track_off, obs_node, counts, start, params): fuzz_tracks' hand-built tracks with displaced keypoints."""
    img_off, kp, P, track_off, obs_node, counts, _ = fz.gen_tri(rng)
    deg = int(rng.integers(5)) if rng.integers(4) == 0 else -1
    T = len(track_off) - 1
    if T and len(obs_node):
        share = 1.0 if deg == 0 else 0.25                                  # deg 0: every observation displaced
        rows = np.flatnonzero(rng.random(len(obs_node)) < share) if deg == 0 else (track_off[:-1] + rng.integers(0, np.diff(track_off)))[rng.random(T) < share]
        nodes = obs_node[rows]
        nodes = nodes[(nodes >= 0) & (nodes < len(kp))]
        kp[nodes] += (rng.uniform(20, 100, (len(nodes), 1)) * np.sign(rng.normal(size=(len(nodes), 2)))).astype(np.float32)
    if deg == 1:                                                           # cameras among the points: steps that would cross one
        P = P.reshape(-1, 3, 4).copy()
        P[:, :, 3] *= rng.uniform(0.02, 0.2)
        P = P.reshape(-1, 12)
    start = None
    if deg in (2, 3) and T:                                                # a NaN start point / flag bit 1 clear, for some tracks
        X0, _, _, fl0, _ = nt.triangulate(track_off, obs_node, img_off, kp, P)
        hit = rng.random(T) < 0.3
        if deg == 2:
            X0[hit, int(rng.integers(3))] = rng.choice([np.nan, np.inf])
        else:
            fl0[hit] &= 1
        start = (X0, fl0)
    params = dict(huber=float(rng.choice([0.5, 1.0, 3.0, np.inf])), obs_thresh=float(rng.choice([0.5, 2.0, 5.0])),
                  iters=int(rng.choice([0, 1, 3, 10])), iters2=int(rng.choice([0, 2, 5])))
    return img_off, kp, P, track_off, obs_node, counts, start, params


def fuzz_refine(rng):
    img_off, kp, P, track_off, obs_node, counts, start, params = gen_refine(rng)
    if int(img_off[-1]) > MAX_NODES:                                       # keeps the restatement's attempts under a second
        keep = int(np.searchsorted(track_off, MAX_NODES // 2, side="right")) - 1
        track_off, counts = track_off[:keep + 1], counts.copy()
        obs_node = obs_node[:track_off[-1]]
        counts[:2] = (keep, len(obs_node))
        if start is not None:
            start = (start[0][:keep], start[1][:keep])
    return check_refine(img_off, kp, P, track_off, obs_node, counts, *(start or (None, None)), **params)[0]


def gen_prune(rng):
    n = max(2, log_uniform_from_zero(rng, 1 << 16))
    lengths = rng.integers(2, 12, log_uniform_from_zero(rng, max(1, n // 8)))
    lengths = lengths[np.cumsum(lengths) <= n]
    T = len(lengths)
    track_off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    nobs = int(track_off[-1])
    obs_node = rng.integers(0, n, nobs).astype(np.int32)
    inlier = rng.choice([0, 1, 255], nobs, p=[0.2, 0.7, 0.1]).astype(np.uint8)
    n_inl = np.add.reduceat((inlier != 0).astype(np.int32), track_off[:-1]) if T else np.zeros(0, np.int32)
    flags = rng.choice([0, 1, 2, 3], T, p=[0.05, 0.05, 0.05, 0.85]).astype(np.int32)
    worst = rng.choice([0.0, 0.5, 1.0, 2.0, 2.5, np.nan, np.inf], T, p=[0.1, 0.3, 0.2, 0.2, 0.1, 0.05, 0.05]).astype(np.float32)
    cosm = rng.choice([-1.0, 0.0, 0.5, 0.9990482, 1.0], T).astype(np.float32)
    X = rng.normal(size=(T, 3)).astype(np.float32)
    if T:
        X[rng.random(T) < 0.05] = np.nan
    kw = dict(min_len=int(rng.choice([2, 3, 5])), max_reproj=float(rng.choice([0.5, 2.0, np.inf])),
              max_cos=float(rng.choice([1.0, 0.5, float(np.float32(0.9990482)), np.nextafter(0.5, 0.0), -1.0])))
    return n, track_off, obs_node, X, inlier, n_inl.astype(np.int32), worst, cosm, flags, kw


def check_prune(n, track_off, obs_node, X, inlier, n_inl, worst, cosm, flags, kw):
    import torch
    from sfm_mvs_amd import tracks
    T, nobs, cap = len(track_off) - 1, len(obs_node), n // 2 + 1
    want = nr.prune(track_off, obs_node, X, inlier, n_inl, worst, cosm, flags, **kw)
    pad = lambda a, size, dt: np.concatenate([np.asarray(a, dt).reshape(-1), np.zeros(size - np.asarray(a).size, dt)])  # noqa: E731
    out = (sentinel((n // 2 + 2 + 2,), torch.int32), sentinel((n + 2,), torch.int32), sentinel((cap + 2, 3), torch.float32),
           sentinel((cap + 2,), torch.int32), sentinel((4 + 2,), torch.int32))
    counts = np.array([T, nobs, 0, 0, 0, 0], np.int32)
    tracks.prune_tracks(dev(counts), dev(padded(track_off, n // 2 + 2)), dev(padded(obs_node, n)), dev(pad(X, 3 * cap, np.float32).reshape(cap, 3)),
                        dev(pad(inlier, n, np.uint8)), dev(pad(n_inl, cap, np.int32)), dev(pad(worst, cap, np.float32)), dev(pad(cosm, cap, np.float32)),
                        dev(pad(flags, cap, np.int32)), kw["min_len"], kw["max_reproj"], None, kw["max_cos"],
                        out=(out[0][:n // 2 + 2], out[1][:n], out[2][:cap], out[3][:cap], out[4][:4]))
    T2, nobs2 = int(want[4][0]), int(want[4][1])
    return (differ("counts2", out[4], want[4], rows=4) or differ("track_off2", out[0], want[0], rows=T2 + 1) or differ("obs_node2", out[1], want[1], rows=nobs2)
            or differ("X2", out[2].reshape(-1), want[2].reshape(-1), rows=3 * T2) or differ("track_src", out[3], want[3], rows=T2))


def fuzz_prune(rng):
    return check_prune(*gen_prune(rng))


def fuzz_composed(rng):
    from sfm_mvs_amd import tracks
    kps, P, pairs, store, nq = fz.gen_scene(rng)
    if not pairs:
        return ""
    for k in kps:                                                          # displaced keypoints: a few per image
        hit = rng.random(len(k)) < 0.05
        k[hit] += (rng.uniform(20, 100, (int(hit.sum()), 1)) * np.sign(rng.normal(size=(int(hit.sum()), 2)))).astype(np.float32)
    kw = dict(min_len=int(rng.choice([2, 3])), max_reproj=[None, 2.0][int(rng.integers(2))])
    robust = dict(huber=float(rng.choice([1.0, 3.0])), obs_thresh=float(rng.choice([2.0, 4.0])), refine_iters=int(rng.choice([3, 10])))
    angle = [None, 2.0][int(rng.integers(2))]
    got = tracks.run_tracks(dev(store), nq, pairs, [dev(k) for k in kps], P.reshape(-1, 3, 4), rounds=int(rng.integers(1, 13)), robust=True,
                            min_angle_deg=angle, **kw, **robust)
    img_off = np.concatenate([[0], np.cumsum([len(k) for k in kps])]).astype(np.int32)
    kp = np.concatenate(kps)
    base = nt.run(store, nq, pairs, img_off, kp, P, min_len=kw["min_len"])
    want = nr.run_robust(base, img_off, kp, P, kw["min_len"], kw["max_reproj"], robust["huber"], robust["obs_thresh"],
                         1.0 if angle is None else float(np.cos(np.deg2rad(angle))), robust["refine_iters"], 5)
    if not got["status"][0]:
        return "composed: run_tracks returned unconverged labels"
    for key in ("counts", "points", "obs", "cam_idx", "pt_idx", "track_len"):
        msg = differ(key, got[key].reshape(-1), want[key].reshape(-1))
        if msg:
            return msg
    if (got["tracks_dropped"], got["obs_dropped"]) != (want["tracks_dropped"], want["obs_dropped"]):
        return f"composed: dropped {(got['tracks_dropped'], got['obs_dropped'])} vs {(want['tracks_dropped'], want['obs_dropped'])}"
    return ""


FAMILIES = [("refine", fuzz_refine, 3), ("prune", fuzz_prune, 2), ("composed", fuzz_composed, 1)]


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
            log(f"MISMATCH {name} (seed {seed}, case seed {case_seed}; replay: fuzz_tracks_refine.py 0 0 {name}:{case_seed}) {msg}")
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
        print(f"fuzz_tracks_refine replay {name}:{case_seed}: {msg or 'no mismatch'}")
        return 1 if msg else 0
    counts, bad, dt = run(budget, seed, log=lambda s: print(s, flush=True))
    print(f"fuzz_tracks_refine: seed {seed}, {sum(counts.values())} cases {counts}, {bad} mismatches, {dt:.0f} s")
    print(f"sfm_build_id {_lib.build_id()}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
