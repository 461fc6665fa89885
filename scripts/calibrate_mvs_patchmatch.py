"""Calibration of the PatchMatch refinement on the CPU (docs/mvs.md §9): the RESTATEMENT tests/np_mvs_patchmatch.py on the two scenes of
tests/mvs_patchmatch_cases.py, the sweep alone and sweep + refinement over iters {1, 2, 3} x far {0, 1} x depth_step {0.05, 0.1, 0.2}
at seed 0, and the default setting on the seeds the tests assert -> tests/golden/mvs_patchmatch_calibration.json.  No GPU.

  python scripts/calibrate_mvs_patchmatch.py [--check]       --check: recompute and compare with the committed file, write nothing"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import mvs_patchmatch_cases as pc  # noqa: E402


def rows(log=print):
    from sfm_mvs_amd import mvs
    out = []
    for name in ("quads", "slant"):
        out.append(dict(scene=name, stage="sweep", **pc.figures(name, pc.sweep_depth(name))))
        log(json.dumps(out[-1]))
        runs = [(far, ds, 0) for far in pc.GRID["far"] for ds in pc.GRID["depth_step"]]
        runs += [(int(mvs.PM_FAR), mvs.PM_DEPTH_STEP, s) for s in pc.SEEDS if s != 0]
        for far, ds, seed in runs:
            snaps = {}
            pc.refine_np(name, max(pc.GRID["iters"]), far, ds, seed, snapshots=snaps)
            for iters in pc.GRID["iters"]:
                out.append(dict(scene=name, stage="refine", iters=iters, far=far, depth_step=ds, seed=seed, **pc.figures(name, *snaps[iters])))
                log(json.dumps(out[-1]))
    return out


def main():
    t0 = time.time()
    from sfm_mvs_amd import mvs
    doc = dict(tool="calibrate_mvs_patchmatch", views=pc.N_VIEWS, width=pc.W, height=pc.H, view=pc.VIEW, ndepth=pc.NDEPTH, radius=pc.RADIUS,
               topk=pc.TOPK, var_min=mvs.VAR_MIN, cost_max=mvs.COST_MAX, slope_step="1/K[0,0]",
               defaults=dict(iters=mvs.PM_ITERS, far=int(mvs.PM_FAR), depth_step=mvs.PM_DEPTH_STEP), rows=rows())
    if "--check" in sys.argv[1:]:
        same = json.loads(json.dumps(doc)) == pc.golden()
        print(f"calibrate_mvs_patchmatch: {'equal to' if same else 'DIFFERS from'} {pc.GOLDEN} ({time.time() - t0:.0f} s)")
        return 0 if same else 1
    with open(pc.GOLDEN, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"calibrate_mvs_patchmatch: {len(doc['rows'])} rows -> {pc.GOLDEN} ({time.time() - t0:.0f} s)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
