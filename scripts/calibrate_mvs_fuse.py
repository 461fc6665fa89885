"""Calibration of the merging fusion on the CPU (docs/mvs.md §10): the RESTATEMENT tests/np_mvs_fuse.py on all 5 views of the two scenes
of tests/mvs_fuse_cases.py, every view's map made as run_mvs makes it (restated sweep; restated refinement at the defaults on seeds 0, 1,
2), fused over max_angle {None, 90, 60, 45, 30, 20, 15} -> tests/golden/mvs_fuse_calibration.json, with the default max_angle chosen by
mvs_fuse_cases.choose_max_angle.  No GPU.  The maps of the 10 views are independent: they are computed in `--jobs` processes.

  python scripts/calibrate_mvs_fuse.py [--check] [--jobs N] [--maps FILE.npz]
      --check: recompute and compare with the committed file, write nothing;  --maps: keep / reuse the restated maps in FILE.npz"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

import mvs_fuse_cases as fc  # noqa: E402

SCENES = ("quads", "slant")


def _maps_of(task):
    name, i = task
    sweep, refined = fc.view_maps(name, i)
    return name, i, sweep, refined


def all_maps(jobs, log=print):
    """{(scene, 'sweep', 0): (depth [n, h, w], None), (scene, 'refine', seed): (depth, normal [n, h, w, 3])}."""
    import multiprocessing as mp
    tasks = [(name, i) for name in SCENES for i in range(fc.N_VIEWS)]
    with mp.get_context("spawn").Pool(jobs) as pool:
        got = {}
        for name, i, sweep, refined in pool.imap_unordered(_maps_of, tasks):
            got[name, i] = (sweep, refined)
            log(f"maps of {name} view {i}")
    out = {}
    for name in SCENES:
        out[name, "sweep", 0] = (np.stack([got[name, i][0] for i in range(fc.N_VIEWS)]), None)
        for seed in fc.SEEDS:
            out[name, "refine", seed] = (np.stack([got[name, i][1][seed][0] for i in range(fc.N_VIEWS)]),
                                         np.stack([got[name, i][1][seed][1] for i in range(fc.N_VIEWS)]))
    return out


def rows(maps, log=print):
    import np_mvs_fuse as nf
    out = []
    for (name, config, seed), (depth, normal) in sorted(maps.items()):
        sc = fc.scene(name)
        own = fc.own_samples(name, depth)
        for angle in (fc.ANGLES if config == "refine" else (None,)):
            res = nf.fuse(depth, sc["table"], normal, fc.frames(name), fc.TAU, fc.cos_of(angle), True)
            filt = fc.filter_cloud(name, depth) if angle is None else own[res["mask"].astype(bool)]
            out.append(dict(scene=name, config=config, seed=seed, max_angle=angle, **fc.fused_figures(name, normal, res, filt)))
            log(json.dumps(out[-1]))
    return out


def main():
    t0 = time.time()
    args = sys.argv[1:]
    jobs = int(args[args.index("--jobs") + 1]) if "--jobs" in args else min(8, os.cpu_count() or 1)
    cache = args[args.index("--maps") + 1] if "--maps" in args else None
    if cache and os.path.exists(cache):
        z = np.load(cache)
        maps = {}
        for key in sorted({k.rsplit("|", 1)[0] for k in z.files}):
            name, config, seed = key.split("|")
            maps[name, config, int(seed)] = (z[key + "|depth"], z[key + "|normal"] if key + "|normal" in z.files else None)
    else:
        maps = all_maps(jobs)
        if cache:
            np.savez_compressed(cache, **{f"{k[0]}|{k[1]}|{k[2]}|{what}": a for k, pair in maps.items()
                                          for what, a in zip(("depth", "normal"), pair) if a is not None})
    from sfm_mvs_amd import mvs
    table = rows(maps)
    doc = dict(tool="calibrate_mvs_fuse", views=fc.N_VIEWS, width=fc.W, height=fc.H, ndepth=fc.NDEPTH, radius=fc.RADIUS, topk=fc.TOPK,
               nsrc=fc.NSRC, tau=fc.TAU, min_consistent=fc.MIN_CONSISTENT, unique=True, var_min=mvs.VAR_MIN, cost_max=mvs.COST_MAX,
               refine=dict(iters=mvs.PM_ITERS, far=int(mvs.PM_FAR), depth_step=mvs.PM_DEPTH_STEP), seeds=list(fc.SEEDS),
               angles=list(fc.ANGLES), keep_share=fc.KEEP_SHARE, default_max_angle=fc.choose_max_angle(table), rows=table)
    if "--check" in args:
        same = json.loads(json.dumps(doc)) == fc.golden()
        print(f"calibrate_mvs_fuse: {'equal to' if same else 'DIFFERS from'} {fc.GOLDEN} ({time.time() - t0:.0f} s)")
        return 0 if same else 1
    with open(fc.GOLDEN, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"calibrate_mvs_fuse: {len(table)} rows, default max_angle {doc['default_max_angle']} -> {fc.GOLDEN} ({time.time() - t0:.0f} s)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
