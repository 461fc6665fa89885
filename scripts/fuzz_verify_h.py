"""Randomised parity sweep of the VERIFY-H family on the GPU box: sfm_verify_h_models / _score / _select and
verify.verify_pairs(homography=...) (through sfm_mvs_amd.verify, into sentinel-filled buffers) vs the restatement tests/np_verify_h.py;
every output word compared exactly (floats as integer views, a NaN equals a NaN).

  python scripts/fuzz_verify_h.py [seconds] [seed] [family:case_seed]

Families (one case = one random draw; sizes log-uniform from 0):
  models      fuzz_verify's planted scenes, budgets 1..1024, samples with slots of -1, past m' and past every node, m off by one
  score       the restatement's models (some flags cleared, one model under several samples), m around the 256-survivor tile, thresholds
              from 0 over thr2h and a survivor's own value to inf
  select      the restatement's keys (some replaced by 0, by a key whose sample is past H), refit 0 and 1, thresholds as above
  composed    verify.verify_pairs(homography=...) with and without lo, whole and in chunks, against the restated composition
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
import np_verify_h as nh
from fuzz_tracks import dev, log_uniform_from_zero
from fuzz_verify import INT32_MAX, first, flat_out, same


def as_i64(keys):
    return np.ascontiguousarray(keys, np.uint64).view(np.int64)


def gen_case(rng, max_pts, max_H):
    """A planted scene with its survivors, samples and (possibly degenerate) normalised keypoints: the inputs of the three launches."""
    deg = int(rng.integers(5)) if rng.integers(4) == 0 else -1
    case = fv.gen_scene(rng, max_pts=max_pts, max_pairs=2)
    H = max(1, log_uniform_from_zero(rng, max_H)) if rng.integers(4) else int(rng.choice([1, 64, 65, 256, 257]))
    xn = nv.normalise(case["kp"], case["K"])
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
    surv, m = nv.survivors(case["store"], case["nq"], case["pairs"], case["img_off"], case["ratio"])
    samp = nv.samples(m, H, int(rng.integers(1 << 32)))
    return case, xn, surv, m, samp


def part_of(case, xn, surv, m):
    return (surv, m, case["pairs"], case["img_off"], xn)


def thr_of(rng, case):
    return float(nv.thr2_of(case["K"], 1.2)) * float(rng.choice([1.0, 1.0, 100.0, 0.0, np.inf]))


def own_value(rng, Hm, ok, part, thr2h):
    """Sometimes the float32 value of one survivor under one model: that survivor is an inlier, the next value up is not."""
    surv, m, pairs, img_off, xn = part
    if not ok.any() or rng.integers(3):
        return thr2h
    p, s = np.argwhere(ok != 0)[int(rng.integers(int((ok != 0).sum())))]
    mp, valid, pts = nh._points(surv, m, pairs, np.asarray(img_off, np.int64), xn, int(p))
    if not mp:
        return thr2h
    d = nh.transfer_value(Hm[p, s], pts)[1][valid]
    d = d[~np.isnan(d)]
    return float(np.sort(d)[int(rng.integers(len(d)))]) if len(d) else thr2h


def fuzz_models(rng):
    import torch
    from sfm_mvs_amd import verify
    case, xn, surv, m, samp = gen_case(rng, 120, 1024)
    samp = samp[:, :max(1, 4000 // max(len(m), 1))].copy()
    bad = rng.random(samp.shape) < 0.02
    samp[bad] = rng.choice([-1, surv.shape[1], INT32_MAX], int(bad.sum()))
    if m.size and rng.integers(4) == 0:
        m = m.copy()
        m[rng.integers(len(m))] += rng.choice([-1, 1, 1000])
    want = nh.models(samp, *part_of(case, xn, surv, m))
    ok, chk_o = flat_out(want[0].shape, torch.int32)
    Hm, chk_H = flat_out(want[1].shape, torch.float64)
    verify.h_models(dev(samp), dev(surv), dev(m), dev(case["pairs"]), dev(case["img_off"]), dev(xn), out=(ok, Hm))
    return first(same("ok", ok, want[0]), same("Hm", Hm, want[1]), chk_o(), chk_H())


def gen_scored(rng, max_H):
    case, xn, surv, m, samp = gen_case(rng, int(rng.choice([40, 250, 260, 600])), max_H)
    part = part_of(case, xn, surv, m)
    ok, Hm = nh.models(samp, *part)
    if ok.size and rng.integers(2):                                  # one model under several samples: the lowest must win
        p = int(rng.integers(len(ok)))
        src = np.flatnonzero(ok[p])
        if len(src):
            Hm[p] = Hm[p, src[0]]
            ok[p] = 1
    if ok.size and rng.integers(4) == 0:
        ok[rng.integers(len(ok))] = rng.choice([0, -3, 11], ok.shape[1])
    if ok.size and rng.integers(4) == 0:                              # a model that sends some survivors behind the camera or to infinity
        p, s = int(rng.integers(ok.shape[0])), int(rng.integers(ok.shape[1]))
        Hm[p, s], ok[p, s] = rng.normal(size=9) * np.array([1, 1, 0.1, 1, 1, 0.1, 1, 1, 0.05]), 1
    if m.size and rng.integers(4) == 0:
        m = m.copy()
        m[rng.integers(len(m))] += rng.choice([-1, 1, 1000])
        part = part_of(case, xn, surv, m)
    return case, part, ok, Hm


def fuzz_score(rng):
    import torch
    from sfm_mvs_amd import verify
    case, part, ok, Hm = gen_scored(rng, 300)
    thr2h = own_value(rng, Hm, ok, part, thr_of(rng, case))
    want_c, want_b = nh.score(Hm, ok, *part, thr2h)
    counts, chk_c = flat_out(want_c.shape, torch.int32)
    best, chk_b = flat_out(want_b.shape, torch.int64)
    verify.h_score(dev(Hm), dev(ok), *(dev(t) for t in part), thr2h, out=(counts, best))
    return first(same("counts", counts, want_c), same("best", best.cpu().numpy().view(np.uint64), want_b), chk_c(), chk_b())


def fuzz_select(rng):
    import torch
    from sfm_mvs_amd import verify
    case, part, ok, Hm = gen_scored(rng, 48)
    thr2h = own_value(rng, Hm, ok, part, thr_of(rng, case))
    best = nh.score(Hm, ok, *part, thr2h)[1]
    if best.size and rng.integers(4) == 0:
        best[rng.integers(len(best))] = rng.choice(np.array([0, 1, (5 << 32) | 0xFFFFFFFF, (7 << 32) | (0xFFFFFFFF - ok.shape[1]), (3 << 32) | 5], np.uint64))
    refit = int(rng.integers(2))
    want = nh.select(Hm, ok, best, *part, thr2h, refit)
    n_pairs, cap = part[0].shape[:2]
    outs = [flat_out(s, t) for s, t in (((n_pairs, cap), torch.uint8), ((n_pairs, 9), torch.float64), ((n_pairs, 3), torch.float64), ((n_pairs, 8), torch.int32))]
    got = verify.h_select(dev(Hm), dev(ok), dev(as_i64(best)), *(dev(t) for t in part), thr2h, refit, out=tuple(o for o, _ in outs))
    return first(*[same(n, g, w) for n, g, w in zip(("keep_h", "H", "h_sv", "h_info"), got, want)], *[c() for _, c in outs])


def fuzz_composed(rng):
    import torch
    from sfm_mvs_amd import verify
    case = fv.gen_scene(rng, max_pts=300, max_pairs=3)
    H, seed = max(1, log_uniform_from_zero(rng, 48)), int(rng.integers(1 << 32))
    lo = None if rng.integers(2) else (int(rng.integers(1, 5)), tuple(float(w) for w in rng.choice([1.0, 2.0, 3.0], int(rng.integers(0, 3)))))
    hs = dict(threshold=float(rng.choice([0.4, 1.2, 2.0, 50.0])), min_ratio=float(rng.choice([0.0, 0.246, 1.0])), rot_spread=float(rng.choice([1.0, 1.525, 100.0])),
              min_inliers=int(rng.choice([0, 8, 30])), refit=int(rng.integers(2)))
    want = nh.verify_pairs(case["store"], case["nq"], case["pairs"], case["img_off"], case["kp"], case["K"], case["ratio"], budget=H, seed=seed, lo=lo,
                           threshold_h=hs["threshold"], min_ratio=hs["min_ratio"], rot_spread=hs["rot_spread"], min_inliers=hs["min_inliers"], refit=hs["refit"])
    torch.cuda.synchronize()
    chunk = {} if rng.integers(2) else dict(max_models_bytes=int(rng.choice([1, 2 * H * 720])))
    got = verify.verify_pairs(dev(case["store"]), dev(case["nq"]), dev(case["pairs"]), dev(case["img_off"]), dev(case["kp"]), case["K"], case["ratio"],
                              budget=H, seed=seed, lo=None if lo is None else dict(top=lo[0], rounds=len(lo[1]), widen=lo[1]), homography=hs, **chunk)
    return first(*[same(n, got[n], want[n]) for n in ("keep", "E", "Rt", "info", "keep_h", "H", "h_sv", "h_info", "config") + (("lo_info",) if lo else ())])


FAMILIES = [("models", fuzz_models, 2), ("score", fuzz_score, 3), ("select", fuzz_select, 3), ("composed", fuzz_composed, 2)]


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
            log(f"MISMATCH {name} (seed {seed}, case seed {case_seed}; replay: fuzz_verify_h.py 0 0 {name}:{case_seed}) {msg}")
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
        print(f"fuzz_verify_h replay {name}:{case_seed}: {msg or 'no mismatch'}")
        return 1 if msg else 0
    counts, bad, dt = run(budget, seed, log=lambda s: print(s, flush=True))
    print(f"fuzz_verify_h: seed {seed}, {sum(counts.values())} cases {counts}, {bad} mismatches, {dt:.0f} s")
    print(f"sfm_build_id {_lib.build_id()}")
    print(json.dumps(dict(tool="fuzz_verify_h", seed=seed, cases=sum(counts.values()), families=counts, mismatches=bad, seconds=round(dt, 1))))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
