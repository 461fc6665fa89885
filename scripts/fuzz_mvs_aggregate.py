"""Randomised parity sweep of the cost-volume aggregation on the GPU box: the HIP path (mvs.cost_shift / cost_aggregate /
cost_depth / aggregate_depth) vs the integer restatement tests/np_mvs_aggregate.py, every output compared as integers / int32
views.

  python scripts/fuzz_mvs_aggregate.py [seconds] [seed] [family:case_seed]

Families (one case = one random draw; every integer parameter uniform over its documented range: ndepth 2..1024, shift 0..4,
0 <= p1 <= p2 <= 2048, ndir 4 or 8, gate 0..65535; the frame log-uniform over 1..32767 per side — 1..8192 where paths are walked —
and capped in area so that the NumPy side of a case stays under a second):
  shift      sfm_mvs_cost_shift on float volumes: uniform costs, sweep-like volumes (a smooth minimum per pixel over 2 elsewhere),
             costs on the rounding ties k/1024 + 1/2048, constants, NaN / +-inf / negatives / values >= 2 planted
  aggregate  sfm_mvs_cost_aggregate on uint16 volumes 0..2048: uniform, few distinct values (ties everywhere), constant, sweep-like
  depth      sfm_mvs_cost_depth on uint16 S and Q: uniform, few distinct values, every plane tied, the winner planted on the first
             or last plane; with and without plane_dev
  composed   mvs.aggregate_depth on a float volume against the composition of the three restatements
The script stops at the first mismatch, prints the family, the case's parameters and its case seed
(gen_<family>(np.random.default_rng(case_seed)) rebuilds the inputs without a GPU; the third argument replays one case), and
exits non-zero.
"""
import os
import sys
import time

os.environ.setdefault("OMP_WAIT_POLICY", "passive")

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import np_mvs_aggregate as agg

F = np.float32
ELEMENTS_SHIFT, ELEMENTS_PATHS, ELEMENTS_DEPTH = 1 << 21, 1 << 20, 1 << 22     # volume elements per case: the NumPy side's time
MAX_SIDE_PATHS = 8192                                                           # (a Python step per pixel along each path)


def log_uniform_int(rng, lo, hi):
    return int(np.clip(np.floor(np.exp(rng.uniform(np.log(lo), np.log(hi + 1)))), lo, hi))


def frame_size(rng, hi, max_area):
    """(w, h), each side log-uniform over 1..hi, redrawn towards smaller sides until w*h <= max_area."""
    max_area = max(max_area, 1)
    while True:
        w, h = log_uniform_int(rng, 1, hi), log_uniform_int(rng, 1, hi)
        if w * h <= max_area:
            return w, h
        hi = max(1, min(hi, max(w, h) - 1))


def up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    import torch
    a = t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return a.view(np.int32) if a.dtype == np.float32 else a


def same(a, b):
    a, b = bits(a), bits(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def sweep_like(rng, nd, h, w):
    """A volume as the sweep writes one: 2 off the surface, a smooth dip around a per-pixel plane that jumps along an edge."""
    ys, xs = np.mgrid[0:h, 0:w]
    centre = np.where(xs * 2 + ys > w, 0.7, 0.25) * nd + 0.02 * nd * np.sin(xs / 9.0)
    j = np.arange(nd)[:, None, None]
    vol = np.minimum(2.0, 0.05 + ((j - centre[None]) / max(2.0, nd / 16.0)) ** 2 + 0.05 * rng.random((nd, h, w)))
    vol[:, rng.random((h, w)) < 0.05] = 2.0                                      # pixels without a valid source
    return vol.astype(F)


def float_volume(rng, nd, h, w):
    kind = int(rng.integers(0, 6))
    if kind == 0:
        vol = rng.uniform(0, 2, (nd, h, w)).astype(F)
    elif kind == 1:
        vol = sweep_like(rng, nd, h, w)
    elif kind == 2:                                                              # exact rounding ties and their float32 neighbours
        k = rng.integers(0, 2049, (nd, h, w))
        vol = (k / 1024.0 + 1.0 / 2048.0).astype(F)
        vol = np.nextafter(vol, F(rng.choice([-1.0, 3.0])), dtype=F) if rng.random() < 0.5 else vol
    elif kind == 3:
        vol = np.full((nd, h, w), F(rng.choice([0.0, 2.0, 0.3, -0.0, 1.9999999])), F)
    elif kind == 4:
        vol = rng.uniform(-0.5, 2.5, (nd, h, w)).astype(F)
    else:
        vol = rng.uniform(0, 2, (nd, h, w)).astype(F)
        for v in (np.nan, np.inf, -np.inf, -1.0, 0.0, 2.0, 1e-30, 3e38):
            vol[rng.random((nd, h, w)) < 0.02] = F(v)
    return f"volume kind {kind}", vol


def u16_volume(rng, nd, h, w, top=2048):
    kind = int(rng.integers(0, 5))
    if kind == 0:
        q = rng.integers(0, top + 1, (nd, h, w))
    elif kind == 1:
        q = rng.integers(0, 4, (nd, h, w)) * int(rng.integers(1, top // 3 + 1))
    elif kind == 2:
        q = np.full((nd, h, w), int(rng.choice([0, 1, top])))
    elif kind == 3:
        q = agg.quantise(sweep_like(rng, nd, h, w)) * top // 2048
    else:
        q = rng.integers(0, top + 1, (nd, h, w)) // int(rng.integers(1, 300))
    return f"kind {kind}", q.astype(np.uint16)


def inverse_depths(rng, nd):
    lo = float(rng.uniform(0.01, 0.5))
    return np.linspace(lo, lo + float(rng.uniform(0.1, 2.0)), nd, dtype=np.float64).astype(F)


def penalties(rng):
    if rng.random() < 0.3:
        p1, p2 = [(0, 0), (0, 2048), (2048, 2048), (10, 102)][int(rng.integers(0, 4))]
    else:
        p2 = int(rng.integers(0, 2049))
        p1 = int(rng.integers(0, p2 + 1))
    return p1, p2, int(rng.choice([4, 8]))


def gen_shift(rng):
    nd, shift = int(rng.integers(2, 1025)), int(rng.integers(0, 5))
    w, h = frame_size(rng, 32767, ELEMENTS_SHIFT // nd)
    tag, vol = float_volume(rng, nd, h, w)
    return f"{w} x {h} ndepth {nd} shift {shift} {tag}", (vol, shift)


def case_shift(rng):
    from sfm_mvs_amd import mvs
    tag, (vol, shift) = gen_shift(rng)
    return None if same(mvs.cost_shift(up(vol), shift), agg.cost_shift(vol, shift)) else f"{tag}: Q differs"


def gen_aggregate(rng):
    nd = int(rng.integers(2, 1025))
    w, h = frame_size(rng, MAX_SIDE_PATHS, ELEMENTS_PATHS // nd)
    p1, p2, ndir = penalties(rng)
    tag, q = u16_volume(rng, nd, h, w)
    return f"{w} x {h} ndepth {nd} p1 {p1} p2 {p2} ndir {ndir} {tag}", (q, p1, p2, ndir)


def case_aggregate(rng):
    from sfm_mvs_amd import mvs
    tag, (q, p1, p2, ndir) = gen_aggregate(rng)
    return None if same(mvs.cost_aggregate(up(q), p1, p2, ndir), agg.cost_aggregate(q, p1, p2, ndir)) else f"{tag}: S differs"


def gen_depth(rng):
    nd = int(rng.integers(2, 1025))
    w, h = frame_size(rng, 32767, ELEMENTS_DEPTH // nd)
    tag_s, s = u16_volume(rng, nd, h, w, top=32768)
    tag_q, q = u16_volume(rng, nd, h, w)
    quirk = int(rng.integers(0, 3)) if rng.random() < 0.3 else -1
    if quirk == 0:
        s[:] = s[0]                                                              # every plane tied: plane 0 wins, no parabola
    elif quirk >= 1:
        s[0 if quirk == 1 else nd - 1][rng.random((h, w)) < 0.5] = 0             # the winner on the first / last plane
    gate = int(rng.choice([0, 1, 307, 2048, 2049, 65535])) if rng.random() < 0.5 else int(rng.integers(0, 65536))
    plane = bool(rng.integers(0, 2))
    return f"{w} x {h} ndepth {nd} gate {gate} plane {plane} S {tag_s} Q {tag_q} quirk {quirk}", (s, q, inverse_depths(rng, nd), gate, plane)


def case_depth(rng):
    from sfm_mvs_amd import mvs
    tag, (s, q, invd, gate, plane) = gen_depth(rng)
    d, c, pl = mvs.cost_depth(up(s), up(q), up(invd), gate, plane=plane)
    wd, wc, wpl = agg.cost_depth(s, q, invd, gate)
    bad = [n for n, a, b in (("depth", d, wd), ("cost", c, wc)) if not same(a, b)]
    if (pl is None) == plane or (pl is not None and not same(pl, wpl)):
        bad.append("plane")
    return f"{tag}: {', '.join(bad)} differ" if bad else None


def gen_composed(rng):
    nd, shift = int(rng.integers(2, 1025)), int(rng.integers(0, 5))
    w, h = frame_size(rng, MAX_SIDE_PATHS, ELEMENTS_PATHS // nd)
    p1, p2, ndir = penalties(rng)
    cost_max = float(rng.choice([0.3, 0.6, 0.0, 2.0, 2.5, -1.0, np.nan])) if rng.random() < 0.5 else float(rng.uniform(0.05, 1.5))
    tag, vol = float_volume(rng, nd, h, w)
    return (f"{w} x {h} ndepth {nd} shift {shift} p1 {p1} p2 {p2} ndir {ndir} cost_max {cost_max} {tag}",
            (vol, inverse_depths(rng, nd), shift, p1, p2, ndir, cost_max))


def case_composed(rng):
    from sfm_mvs_amd import mvs
    tag, (vol, invd, shift, p1, p2, ndir, cost_max) = gen_composed(rng)
    got = mvs.aggregate_depth(up(vol), up(invd), shift, p1, p2, ndir, cost_max)
    want = agg.aggregate_depth(vol, invd, shift, p1, p2, ndir, cost_max)
    bad = [n for n, a, b in zip(("depth", "cost", "plane"), got, want) if not same(a, b)]
    return f"{tag}: {', '.join(bad)} differ" if bad else None


FAMILIES = [("shift", case_shift, 2), ("aggregate", case_aggregate, 4), ("depth", case_depth, 2), ("composed", case_composed, 3)]


def run(budget, seed, log=print):
    """Cases for `budget` seconds from `seed`; stops at the first mismatch -> (counts per family, mismatches)."""
    fns = {name: fn for name, fn, _ in FAMILIES}
    rng = np.random.default_rng(seed)
    weights = np.array([w for _, _, w in FAMILIES], float); weights /= weights.sum()
    t0 = time.time(); counts = {name: 0 for name, _, _ in FAMILIES}; bad = 0
    while time.time() - t0 < budget and not bad:
        name = FAMILIES[int(rng.choice(len(FAMILIES), p=weights))][0]
        case_seed = int(rng.integers(1 << 31))
        try:
            with np.errstate(all="ignore"):
                msg = fns[name](np.random.default_rng(case_seed))
        except Exception as e:  # noqa: BLE001
            msg = f"EXCEPTION {e!r}"[:300]
        counts[name] += 1
        if msg:
            bad += 1
            log(f"MISMATCH {name} (seed {seed}, case seed {case_seed}; replay: fuzz_mvs_aggregate.py 0 0 {name}:{case_seed}) {msg}")
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
        print(f"fuzz_mvs_aggregate replay {name}:{case_seed}: {msg or 'no mismatch'}")
        return 1 if msg else 0
    counts, bad, dt = run(budget, seed, log=lambda s: print(s, flush=True))
    print(f"fuzz_mvs_aggregate: seed {seed}, {sum(counts.values())} cases {counts}, {bad} mismatches, {dt:.0f} s")
    print(f"sfm_build_id {_lib.build_id()}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
