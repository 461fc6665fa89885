"""Randomised parity sweep of the MVS kernels on the GPU box: HIP path (through the C-ABI) vs the float32 restatement tests/np_mvs.py,
bit for bit (tests/parity_cases.py: int32 views; a NaN equals a NaN).

  python scripts/fuzz_mvs.py [seconds] [seed] [family:case_seed]

Families (one case = one random draw; every integer parameter uniform over its documented range, the frame log-uniform over
2r+1 .. 32767 per side but capped in area so that the NumPy side of a case stays around a second; about one case in four
carries one of the degeneracies of tests/test_gpu_mvs_limits.py):
  sweep        sfm_mvs_plane_sweep: radius 1..4, 1..8 sources, topk 1..nsrc, 2..1024 planes; crops of a rendered scene with its
               real matrices, or textures shifted by whole pixels under near-identity matrices.  Degeneracies: a source behind
               every plane, h2 changing sign across the frame, h2 tiny, M = identity with v = 0, NaN / inf matrix rows, flat or
               checkerboard frames, one source passed nsrc times, cost_max <= 0, >= 2, +-inf.
  consistency  sfm_mvs_consistency: frames from 1 x 1, 0..8 neighbours, min_consistent 0..nview, tau from 0, smooth depth maps under
               near-identity motions.  Degeneracies: NaN / +-inf / negative / zero depths planted in every map, a neighbour
               repeated, a neighbour carrying the reference's index, a neighbour behind the reference (p2 <= 0).
  run_mvs      mvs.run_mvs on a small rendered scene (2..6 views) against the np_mvs composition (parity_cases.np_run_mvs):
               depth maps bit-identical, points and colours equal.
Inputs stay inside the contract of include/sfm_hip.h.  The script stops at the first mismatch, prints the family, the case's
parameters and its case seed (gen_<family>(np.random.default_rng(case_seed)) rebuilds the inputs without a GPU; the third
argument replays one case), and exits non-zero.  A case whose restatement raises is a mismatch unless the product raises too.
"""
import os
import sys
import time

os.environ.setdefault("OMP_WAIT_POLICY", "passive")

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import parity_cases as pc
from mvs_scenes import render_scene, scene_cloud

F = np.float32
SECONDS_PER_WARP, SECONDS_PER_TERM = 1e-7, 4.5e-9   # the NumPy side of a sweep, per pixel x plane x source: the warp, and each window sample
IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], F)


def log_uniform_int(rng, lo, hi):
    return int(np.clip(np.floor(np.exp(rng.uniform(np.log(lo), np.log(hi + 1)))), lo, hi))


def frame_size(rng, lo, hi, max_area):
    """(w, h), each side log-uniform over lo..hi, redrawn towards smaller sides until w*h <= max_area."""
    max_area = max(max_area, lo * lo)
    while True:
        w, h = log_uniform_int(rng, lo, hi), log_uniform_int(rng, lo, hi)
        if w * h <= max_area:
            return w, h
        hi = max(lo, min(hi, max(w, h) - 1))


def gen_sweep(rng):
    from sfm_mvs_amd import mvs
    r = int(rng.integers(1, 5)); nsrc = int(rng.integers(1, 9)); topk = int(rng.integers(1, nsrc + 1)); nd = int(rng.integers(2, 1025))
    w, h = frame_size(rng, 2 * r + 1, 32767, int(0.5 / (nd * nsrc * (SECONDS_PER_WARP + SECONDS_PER_TERM * (2 * r + 1) ** 2))))
    var_min = float(rng.choice([1.0, 50.0, 150.0, 1000.0])); cost_max = float(rng.uniform(0.1, 1.0))
    kind = "scene" if (w <= 192 and h <= 93 and rng.random() < 0.7) else "shift"
    if kind == "scene":
        grays, K, P, _, _ = pc.scene(n=9, w=192, h=93, seed=3, arc=float(rng.choice([0.3, 0.8])))
        g, Kc, Pc = pc.crop(grays, K, P, int(rng.integers(0, 192 - w + 1)), int(rng.integers(0, 93 - h + 1)), w, h)
        i = int(rng.integers(0, 9)); nb = mvs.neighbours(i, 9, nsrc)
        ref, srcs, mv = g[i], [g[v] for v in nb], mvs.sweep_matrices(Kc, Pc[i], Pc[nb])
        invd = mvs._inverse_depths_host(float(rng.uniform(0.8, 3.0)), float(rng.uniform(6.0, 14.0)), nd)
    else:
        pad = 4
        big = pc.texture(h + 2 * pad, w + 2 * pad, int(rng.integers(1 << 30)))
        ref = np.ascontiguousarray(big[pad:pad + h, pad:pad + w])
        invd = np.linspace(0.1, 0.5, nd, dtype=np.float64).astype(F)
        srcs, mv = [], np.tile(IDENTITY, (nsrc, 1))
        for s in range(nsrc):
            sx, sy = (int(v) for v in rng.integers(-pad, pad + 1, 2))
            srcs.append(np.ascontiguousarray(big[pad - sy:pad - sy + h, pad - sx:pad - sx + w]))      # src[y + sy, x + sx] = ref[y, x]
            mv[s, 9:11] = np.array([sx, sy], F) / invd[int(rng.integers(0, nd))]
            if rng.random() < 0.5:
                mv[s, :9] += rng.normal(0, 1e-4, 9).astype(F)
    quirk = int(rng.integers(0, 11)) if rng.random() < 0.25 else -1
    s = int(rng.integers(0, nsrc))
    if quirk == 0:
        mv[s] = -mv[s]
    elif quirk == 1:
        mv[s, 6], mv[s, 7] = F(1e-3), F(-2e-3)
        mv[s, 11] = -(mv[s, 8] + F(0.05)) / invd[nd // 2]
    elif quirk == 2:
        mv[s] = IDENTITY; mv[s, 8] = F(2e-38)
    elif quirk == 3:
        mv[s] = IDENTITY
    elif quirk == 4:
        mv[s, 3 * int(rng.integers(0, 4)):][:3] = F(rng.choice([np.nan, np.inf, -np.inf]))
    elif quirk == 5:
        flat = np.full((h, w), int(rng.choice([0, 128, 255])), np.uint8)
        if rng.random() < 0.5:
            ref = flat
        else:
            srcs = [flat for _ in srcs]
    elif quirk == 6:
        ys, xs = np.mgrid[0:h, 0:w]
        ref = (((xs + ys) & 1) * 255).astype(np.uint8); srcs = [ref for _ in srcs]
    elif quirk == 7:
        srcs = [srcs[s]] * nsrc; mv = np.repeat(mv[s:s + 1], nsrc, 0)
    elif quirk >= 8:
        cost_max = float(rng.choice([-1.0, 0.0, 2.0, 2.5, np.inf, -np.inf]))
    tag = f"{w} x {h} {kind} r {r} nsrc {nsrc} topk {topk} ndepth {nd} var_min {var_min} cost_max {cost_max} quirk {quirk}"
    return tag, (ref, srcs, np.ascontiguousarray(mv, F), invd, r, topk, var_min, cost_max)


def case_sweep(rng):
    tag, args = gen_sweep(rng)
    _, bad = pc.sweep_both(*args)
    return None if bad is None else f"{tag}: {bad} differs"


def gen_consistency(rng):
    w, h = frame_size(rng, 1, 32767, 1 << 18)
    nview = int(rng.integers(0, 9)); min_consistent = int(rng.integers(0, nview + 1)); unique = bool(rng.integers(0, 2))
    tau = float(rng.choice([0.0, 0.001, 0.01, 0.1]))
    ref_index = int(rng.integers(0, 12))
    ys, xs = np.mgrid[0:h, 0:w]
    base = (4.0 + 0.01 * xs - 0.02 * ys + 0.5 * np.sin(xs / 7.0) * np.cos(ys / 5.0)).astype(F)
    base[rng.random((h, w)) < 0.1] = 0
    noise = lambda: (base * (1 + float(rng.choice([0.0, 0.002, 0.02])) * rng.standard_normal((h, w)))).astype(F)   # noqa: E731
    depth, nbrs = noise(), [noise() for _ in range(nview)]
    ab = np.tile(IDENTITY, (nview, 1))
    ab[:, :9] += rng.normal(0, 1e-4, (nview, 9)).astype(F)
    ab[:, 9:] = rng.normal(0, [2.0, 2.0, 0.02], (nview, 3)).astype(F)
    bc = (IDENTITY + np.concatenate([rng.normal(0, 0.01, 9), rng.normal(0, 1.0, 3)])).astype(F)
    index = [int(v) for v in rng.integers(0, 12, nview)]
    quirk = int(rng.integers(0, 4)) if rng.random() < 0.25 else -1
    if quirk == 0:
        depth, nbrs = pc.plant_specials(depth, rng), [pc.plant_specials(d, rng) for d in nbrs]
    elif quirk == 1 and nview >= 2:
        nbrs[1], ab[1], index[1] = nbrs[0], ab[0], index[0]
    elif quirk == 2 and nview >= 1:
        index[0], ab[0] = ref_index, IDENTITY
    elif quirk == 3 and nview >= 1:
        ab[0, 6:9], ab[0, 11] = -ab[0, 6:9], F(rng.choice([-1.0, 4.0]))
    tag = f"{w} x {h} nview {nview} min_consistent {min_consistent} unique {unique} tau {tau} ref_index {ref_index} quirk {quirk}"
    return tag, (depth, nbrs, index, ab, ref_index, bc, tau, min_consistent, unique)


def case_consistency(rng):
    tag, args = gen_consistency(rng)
    _, bad = pc.consistency_both(*args)
    return None if bad is None else f"{tag}: {bad} differs"


def gen_run_mvs(rng):
    n = int(rng.integers(2, 7)); w = int(rng.integers(40, 97)); h = int(rng.integers(30, 73))
    opts = dict(ndepth=int(rng.integers(2, 33)), radius=int(rng.integers(1, 5)), nsrc=int(rng.integers(1, 9)), topk=int(rng.integers(1, 9)),
                var_min=float(rng.choice([50.0, 200.0])), cost_max=float(rng.choice([0.3, 0.6])), tau=float(rng.choice([0.01, 0.05])),
                min_consistent=int(rng.integers(0, 4)), unique=bool(rng.integers(0, 2)))
    scene_seed, arc = int(rng.integers(0, 1000)), float(rng.choice([0.2, 0.5, 1.0]))
    imgs, K, P, gt = render_scene(n=n, w=w, h=h, seed=scene_seed, arc=arc)
    X = scene_cloud(K, P, gt, step=int(rng.choice([3, 7, 40])))           # (step 40: a cloud too poor for a depth range on small frames)
    posearr = np.hstack([K.ravel()] + [p.ravel() for p in P])
    return f"{n} views {w} x {h} scene {scene_seed} arc {arc} cloud {len(X)} {opts}", (imgs, K, posearr, X, opts)


def case_run_mvs(rng):
    from sfm_mvs_amd import mvs
    tag, (imgs, K, posearr, X, opts) = gen_run_mvs(rng)
    n = len(imgs)
    nsrc = min(opts["nsrc"], n - 1)                    # run_mvs's own clamps, restated
    ref_opts = dict(opts, nsrc=nsrc, topk=min(opts["topk"], nsrc), min_consistent=min(opts["min_consistent"], nsrc))
    want = got = e_want = e_got = None
    try:
        with np.errstate(all="ignore"):
            want = pc.np_run_mvs([pc.gray(im) for im in imgs], imgs, K, posearr, X, **ref_opts)
    except Exception as e:  # noqa: BLE001
        e_want = e
    try:
        got = mvs.run_mvs(imgs, K, posearr, X, **opts)
    except Exception as e:  # noqa: BLE001
        e_got = e
    if (e_want is None) != (e_got is None):
        return f"{tag}: raised on one side only ({e_want!r} / {e_got!r})"
    if e_want is not None:
        return None
    if not all(pc.same(a, b) for a, b in zip(got["depths"], want[0])):
        return f"{tag}: depth maps differ"
    if not (np.array_equal(got["points"], want[1]) and np.array_equal(got["colors"], want[2])):
        return f"{tag}: fused cloud differs"
    return None


FAMILIES = [("sweep", case_sweep, 6), ("consistency", case_consistency, 3), ("run_mvs", case_run_mvs, 1)]


def main():
    import sfm_mvs_amd
    from sfm_mvs_amd import _lib
    budget = float(sys.argv[1]) if len(sys.argv) > 1 else 120.0
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    sfm_mvs_amd.lib()
    fns = {name: fn for name, fn, _ in FAMILIES}
    if len(sys.argv) > 3:                               # replay one case
        name, case_seed = sys.argv[3].split(":")
        msg = fns[name](np.random.default_rng(int(case_seed)))
        print(f"fuzz_mvs replay {name}:{case_seed}: {msg or 'no mismatch'}")
        return 1 if msg else 0
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
            print(f"MISMATCH {name} (seed {seed}, case seed {case_seed}; replay: fuzz_mvs.py 0 0 {name}:{case_seed}) {msg}", flush=True)
    print(f"fuzz_mvs: seed {seed}, {sum(counts.values())} cases {counts}, {bad} mismatches, {time.time() - t0:.0f} s")
    print(f"sfm_build_id {_lib.build_id()}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
