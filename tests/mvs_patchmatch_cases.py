"""The scenes, settings and figures of the PatchMatch calibration (docs/mvs.md §9), shared by scripts/calibrate_mvs_patchmatch.py,
tests/test_mvs_patchmatch_cpu.py and tests/test_gpu_mvs_patchmatch.py: the middle view of the 5-view 160 x 120 scene of mvs_scenes
("quads") and of mvs_slant_scenes ("slant"), the plane sweep at run_mvs's defaults, and the refinement from its depth map."""
import functools
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "mvs_patchmatch_calibration.json")
N_VIEWS, W, H, VIEW, NDEPTH, RADIUS, TOPK = 5, 160, 120, 2, 128, 3, 2
GRID = dict(iters=(1, 2, 3), far=(0, 1), depth_step=(0.05, 0.1, 0.2))
SEEDS = (0, 1, 2)               # the seeds on which the default setting is asserted


@functools.lru_cache(maxsize=None)
def scene(name):
    """dict(images, K, P, gt [per view], gt_normal / floor [view VIEW] or None, cloud, nbrs, mv, invd): the inputs of view VIEW."""
    from mvs_scenes import gray, render_scene, scene_cloud
    from sfm_mvs_amd import mvs
    if name == "quads":
        imgs, K, P, gt = render_scene(n=N_VIEWS, w=W, h=H, seed=0)
        gt_normal = floor = None
    else:
        from mvs_slant_scenes import FLOOR, render_slant_scene
        imgs, K, P, gt, nrm, idx = render_slant_scene(n=N_VIEWS, w=W, h=H, seed=0)
        gt_normal, floor = nrm[VIEW], idx[VIEW] == FLOOR
    X = scene_cloud(K, P, gt)
    nbrs = mvs.neighbours(VIEW, N_VIEWS, 4)
    dmin, dmax = mvs.depth_range(X, P[VIEW], P_all=P)
    return dict(images=imgs, K=K, P=P, gt=gt, gt_normal=gt_normal, floor=floor, cloud=X, nbrs=nbrs,
                ref=gray(imgs[VIEW]), srcs=[gray(imgs[v]) for v in nbrs], mv=mvs.sweep_matrices(K, P[VIEW], P[nbrs]),
                invd=np.linspace(1.0 / dmax, 1.0 / dmin, NDEPTH, dtype=np.float64).astype(np.float32),
                nmat=mvs.normal_matrix(K, P[VIEW]))


@functools.lru_cache(maxsize=None)
def sweep_depth(name):
    """The restated plane sweep's depth map of the scene's view VIEW at run_mvs's defaults (read-only)."""
    import np_mvs
    from sfm_mvs_amd import mvs
    sc = scene(name)
    d = np_mvs.plane_sweep(sc["ref"], sc["srcs"], sc["mv"], sc["invd"], RADIUS, TOPK, mvs.VAR_MIN, mvs.COST_MAX)[0]
    d.setflags(write=False)
    return d


def refine_np(name, iters, far, depth_step, seed, snapshots=None):
    """The restated refinement of sweep_depth(name) -> (state, depth, cost, normal).  snapshots: a dict that receives the depth map and
    the normals after every full iteration, {iteration count: (depth, normal)} (the state after k iterations of a longer run is the
    run with iters = k: the step 2^-it depends on the iteration alone)."""
    import np_mvs_patchmatch as pm
    from sfm_mvs_amd import mvs
    sc = scene(name)
    fr = pm.Frame(sc["ref"], sc["srcs"], sc["mv"], RADIUS, TOPK, mvs.VAR_MIN)

    def after(it, colour, state):
        if snapshots is not None and colour == 1:
            d, _, n = pm.finish(fr, state, mvs.COST_MAX, sc["nmat"])
            snapshots[it + 1] = (d, n)
    return pm.patchmatch(sc["ref"], sc["srcs"], sc["mv"], sc["invd"][0], sc["invd"][-1], RADIUS, TOPK, mvs.VAR_MIN, mvs.COST_MAX,
                         sweep_depth(name), iters, far, depth_step, 1.0 / sc["K"][0, 0], seed, sc["nmat"], after=after)


def figures(name, depth, normal=None):
    """The figures of one depth map of the scene (and its normals): shares of the interior pixels with a depth, of those within 1 % and
    0.25 % of the truth; on the slant scene the same two on the floor alone; the median angle (degrees) between normal and truth."""
    sc = scene(name)
    r = RADIUS
    d, g = np.asarray(depth, np.float64)[r:-r, r:-r], sc["gt"][VIEW][r:-r, r:-r]
    valid = (d > 0) & (g > 0)
    rel = np.abs(d - g) / np.where(g > 0, g, 1.0)
    out = dict(valid=float((d > 0).mean()), within_1pct=float((rel[valid] <= 0.01).mean()), within_025pct=float((rel[valid] <= 0.0025).mean()))
    if sc["floor"] is not None:
        fl = valid & sc["floor"][r:-r, r:-r]
        out.update(floor_within_1pct=float((rel[fl] <= 0.01).mean()), floor_within_025pct=float((rel[fl] <= 0.0025).mean()))
    if normal is not None and sc["gt_normal"] is not None:
        n, t = np.asarray(normal, np.float64)[r:-r, r:-r], sc["gt_normal"][r:-r, r:-r]
        cosang = np.clip((n * t).sum(-1)[valid], -1.0, 1.0)
        out["normal_median_deg"] = float(np.degrees(np.median(np.arccos(cosang))))
        if sc["floor"] is not None:
            out["floor_normal_median_deg"] = float(np.degrees(np.median(np.arccos(np.clip((n * t).sum(-1)[fl], -1.0, 1.0)))))
    return out


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def row(doc, scene_name, iters, far, depth_step, seed=0):
    for r in doc["rows"]:
        if r["stage"] == "refine" and (r["scene"], r["iters"],r["far"], r["depth_step"], r["seed"]) == (scene_name, iters, int(far), depth_step, seed):
            return r
    raise KeyError((scene_name, iters, far, depth_step, seed))
