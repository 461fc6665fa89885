"""Randomised parity sweep of the VERIFY-LO family on the GPU box: sfm_verify_top / _lo / _lo_pick and verify.verify_pairs(lo=...)
(through sfm_mvs_amd.verify, into sentinel-filled buffers) vs the restatement tests/np_verify_lo.py; every output word compared exactly
(floats as integer views, a NaN equals a NaN).

  python scripts/fuzz_verify_lo.py [seconds] [seed] [family:case_seed]

Families (one case = one random draw; sizes log-uniform from 0):
  top         random counts (ties, zeros, negative words) and model counts from -3 to 11, budgets 1..1024, T 1..16, 0..5 pairs
  lo          the restatement's keys (some replaced by 0, by a key whose slot is past 10 H, by a repeated key) over fuzz_verify's planted
              scenes, m around the 256 lanes, T 1..16, R 0..8, thresholds from 0 over thr2 and a survivor's own value to inf
  pick        random candidates: ties between counts, candidates without a model, every count zero, T 1..16
  composed    verify.verify_pairs(lo=...) against the restated composition on planted multi-image scenes
One case in four carries a degeneracy: no points, every keypoint equal, collinear keypoints, NaN, inf and huge coordinates, cap = 0.
The script stops at the first mismatch, prints the family and the case seed that rebuilds the inputs without a GPU, exits non-zero, and
ends with one JSON line."""
import json
import os
import sys
import time

os.environ.setdefault("OMP_WAIT_POLICY", "passive")

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "scripts"))
import fuzz_verify as fv
import np_verify as nv
import np_verify_lo as nl
from fuzz_tracks import dev, log_uniform_from_zero
from fuzz_verify import first, flat_out, same


def as_i64(keys):
    return np.ascontiguousarray(keys, np.uint64).view(np.int64)


def gen_top_case(rng):
    n_pairs = log_uniform_from_zero(rng, 5)
    H = max(1, log_uniform_from_zero(rng, 1024)) if rng.integers(4) else int(rng.choice([1, 3, 26, 103, 1024]))
    T = int(rng.integers(1, nl.MAX_TOP + 1))
    style = int(rng.integers(5))
    counts = rng.integers(0, [3, 50, 5000, 2, 1][style] + 1, (n_pairs, H, nl.SLOTS)).astype(np.int32)
    if style == 4:
        counts[rng.random(counts.shape) < 0.01] = rng.choice([-1, -2 ** 31, 2 ** 31 - 1])
    nm = rng.integers(0, 11, (n_pairs, H)).astype(np.int32)
    if rng.integers(3) == 0:
        nm[rng.random(nm.shape) < 0.9] = 0                          # fewer models than T
    if rng.integers(4) == 0:
        nm[rng.random(nm.shape) < 0.3] = rng.choice([-3, 11, 100])
    if n_pairs and rng.integers(4) == 0:
        nm[rng.integers(n_pairs)] = 0
    return counts, nm, T


def fuzz_top(rng):
    import torch
    from sfm_mvs_amd import verify
    counts, nm, T = gen_top_case(rng)
    want = nl.top(counts, nm, T)
    out, chk = flat_out(want.shape, torch.int64)
    verify.top_models(dev(counts), dev(nm), T, out=out)
    return first(same("top", out.cpu().numpy().view(np.uint64), want), chk())


def gen_lo_case(rng):
    deg = int(rng.integers(5)) if rng.integers(4) == 0 else -1
    case = fv.gen_scene(rng, max_pts=int(rng.choice([12, 40, 250, 260, 600])), max_pairs=2)
    st = fv.staged(case, max(1, log_uniform_from_zero(rng, 24)), int(rng.integers(1 << 32)))
    xn = st["xn"].copy()
    if len(xn):
        if deg == 0:
            xn[:] = xn[0]
        if deg == 1:
            xn[:, 1] = 2 * xn[:, 0] + 0.1
        if deg == 2:
            xn[rng.random(len(xn)) < 0.1] = np.nan
        if deg == 3:
            xn[rng.random(len(xn)) < 0.1] = 1e150
        if deg == 4:
            xn[rng.random(len(xn)) < 0.1] = np.inf
    H = st["nmodels"].shape[1]
    T, R = int(rng.integers(1, nl.MAX_TOP + 1)), int(rng.integers(0, nl.MAX_ROUNDS + 1))
    keys = nl.top(st["counts"], st["nmodels"], T)
    bad = rng.random(keys.shape) < 0.1
    keys[bad] = rng.choice(np.array([0, 1, (5 << 32) | 0xFFFFFFFF, (7 << 32) | (0xFFFFFFFF - nl.SLOTS * H), (3 << 32) | 5], np.uint64), int(bad.sum()))
    thr2 = float(st["thr2"]) * float(rng.choice([1.0, 1.0, 100.0, 0.0, np.inf]))
    wide2 = (np.float32(st["thr2"]) * rng.choice([0.0, 1.0, 4.0, 9.0, 100.0, 1e6, np.inf], R).astype(np.float32)).astype(np.float32)
    m = st["m"].copy()
    if m.size and rng.integers(4) == 0:
        m[rng.integers(len(m))] += rng.choice([-1, 1, 1000])
    return case, st, xn, m, keys, thr2, wide2


def fuzz_lo(rng):
    import torch
    from sfm_mvs_amd import verify
    case, st, xn, m, keys, thr2, wide2 = gen_lo_case(rng)
    if len(wide2) and keys.size and rng.integers(3) == 0:            # a threshold that is one survivor's own value
        p = int(rng.integers(len(keys)))
        has, slot = nl.slot_of(keys[p, 0], st["nmodels"].shape[1])
        mp = nv._mprime(m[p], st["surv"].shape[1], int(case["pairs"][p][0]), int(case["pairs"][p][1]), len(case["img_off"]) - 1)
        if has and mp:
            valid, pts = nv._pair_points(st["surv"][p], mp, int(case["pairs"][p][0]), int(case["pairs"][p][1]), np.asarray(case["img_off"], np.int64), xn)
            v = nl.sampson_value(st["E_all"][p].reshape(-1, 9)[slot], pts)[valid]
            v = v[~np.isnan(v)]
            if len(v):
                wide2[0] = np.sort(v)[min(len(v) - 1, int(rng.choice([6, 7, 8, len(v) // 2])))]
    want = nl.lo(st["E_all"], keys, st["surv"], m, case["pairs"], case["img_off"], xn, thr2, wide2)
    n_pairs, T = keys.shape
    outs = [flat_out(s, t) for s, t in (((n_pairs, T, 9), torch.float64), ((n_pairs, T), torch.int32), ((n_pairs, T), torch.int32))]
    got = verify.local_optimise(dev(st["E_all"]), dev(as_i64(keys)), dev(st["surv"]), dev(m), dev(case["pairs"]), dev(case["img_off"]), dev(xn), thr2,
                                wide2, out=tuple(o for o, _ in outs))
    return first(*[same(n, g, w) for n, g, w in zip(("E_lo", "n_lo", "round_lo"), got, want)], *[c() for _, c in outs])


def gen_pick_case(rng):
    n_pairs, T = log_uniform_from_zero(rng, 6), int(rng.integers(1, nl.MAX_TOP + 1))
    H = max(1, log_uniform_from_zero(rng, 1024))
    slots = rng.integers(0, nl.SLOTS * H + (3 if rng.integers(3) == 0 else 0), (n_pairs, T)).astype(np.uint64)
    keys = (rng.integers(0, 50, (n_pairs, T)).astype(np.uint64) << np.uint64(32)) | (np.uint64(nl.M32) - slots)
    keys[rng.random(keys.shape) < 0.2] = 0
    n_lo = rng.integers(0, int(rng.choice([1, 3, 1000])), (n_pairs, T)).astype(np.int32)
    round_lo = rng.integers(-1, nl.MAX_ROUNDS, (n_pairs, T)).astype(np.int32)
    E_lo = rng.normal(size=(n_pairs, T, 9))
    return keys, E_lo, n_lo, round_lo, H


def fuzz_pick(rng):
    import torch
    from sfm_mvs_amd import verify
    keys, E_lo, n_lo, round_lo, H = gen_pick_case(rng)
    want = nl.pick(keys, E_lo, n_lo, round_lo, H)
    n_pairs = len(keys)
    outs = [flat_out(s, t) for s, t in (((n_pairs, 1, nl.SLOTS, 9), torch.float64), ((n_pairs, 1), torch.int32), ((n_pairs,), torch.int64),
                                        ((n_pairs, 8), torch.int32))]
    got = verify.pick(dev(as_i64(keys)), dev(E_lo), dev(n_lo), dev(round_lo), H, out=tuple(o for o, _ in outs))
    got = (got[0], got[1], got[2].cpu().numpy().view(np.uint64), got[3])
    return first(*[same(n, g, w) for n, g, w in zip(("E_sel", "nmodels_sel", "best_sel", "lo_info"), got, want)], *[c() for _, c in outs])


def fuzz_composed(rng):
    import torch
    from sfm_mvs_amd import verify
    case = fv.gen_scene(rng, max_pts=300, max_pairs=3)
    H, seed = max(1, log_uniform_from_zero(rng, 48)), int(rng.integers(1 << 32))
    T, R = int(rng.integers(1, nl.MAX_TOP + 1)), int(rng.integers(0, nl.MAX_ROUNDS + 1))
    widen = tuple(float(w) for w in rng.choice([1.0, 1.5, 2.0, 3.0, 50.0], R))
    want = nl.verify_pairs(case["store"], case["nq"], case["pairs"], case["img_off"], case["kp"], case["K"], case["ratio"], budget=H, seed=seed, lo_top=T,
                           widen=widen)
    torch.cuda.synchronize()
    chunk = {} if rng.integers(2) else dict(max_models_bytes=int(rng.choice([1, 2 * H * 720])))
    got = verify.verify_pairs(dev(case["store"]), dev(case["nq"]), dev(case["pairs"]), dev(case["img_off"]), dev(case["kp"]), case["K"], case["ratio"],
                              budget=H, seed=seed, lo=dict(top=T, rounds=R, widen=widen), **chunk)
    return first(*[same(n, got[n], want[n]) for n in ("keep", "E", "Rt", "info", "lo_info")])


FAMILIES = [("top", fuzz_top, 2), ("lo", fuzz_lo, 3), ("pick", fuzz_pick, 2), ("composed", fuzz_composed, 2)]


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
            log(f"MISMATCH {name} (seed {seed}, case seed {case_seed}; replay: fuzz_verify_lo.py 0 0 {name}:{case_seed}) {msg}")
    return counts, bad, time.time() - t0


def main():
    import sfm_mvs_amd
    from sfm_mvs_amd import _lib
    budget = float(sys.argv[1]) if len(sys.argv) > 1 else 90.0
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    sfm_mvs_amd.lib()
    if len(sys.argv) > 3:                               # replay one case
        name, case_seed = sys.argv[3].split(":")
        msg = {n: fn for n, fn, _ in FAMILIES}[name](np.random.default_rng(int(case_seed)))
        print(f"fuzz_verify_lo replay {name}:{case_seed}: {msg or 'no mismatch'}")
        return 1 if msg else 0
    counts, bad, dt = run(budget, seed, log=lambda s: print(s, flush=True))
    print(f"fuzz_verify_lo: seed {seed}, {sum(counts.values())} cases {counts}, {bad} mismatches, {dt:.0f} s")
    print(f"sfm_build_id {_lib.build_id()}")
    print(json.dumps(dict(tool="fuzz_verify_lo", seed=seed, cases=sum(counts.values()), families=counts, mismatches=bad, seconds=round(dt, 1))))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
