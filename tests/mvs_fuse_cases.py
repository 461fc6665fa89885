"""The scenes, settings and figures of the fusion calibration (docs/mvs.md §10), shared by scripts/calibrate_mvs_fuse.py,
tests/test_mvs_fuse_cpu.py and tests/test_gpu_mvs_fuse.py: all 5 views of the two 160 x 120 scenes of mvs_patchmatch_cases ("quads",
"slant") at run_mvs's defaults, view by view as run_mvs treats them (sequence neighbours, depth_range of the scene cloud), fused."""
import functools
import json
import os

import numpy as np

from mvs_patchmatch_cases import H, N_VIEWS, NDEPTH, RADIUS, SEEDS, TOPK, W  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "mvs_fuse_calibration.json")
ANGLES = (None, 90, 60, 45, 30, 20, 15)     # the grid of max_angle (degrees; None: no bound)
TAU, MIN_CONSISTENT, NSRC = 0.01, 2, 4      # run_mvs's defaults
KEEP_SHARE = 0.95                           # the default max_angle keeps at least this share of the unbounded point count


@functools.lru_cache(maxsize=None)
def scene(name):
    """dict(images, K, P, gt, gt_normal (per view, or None), cloud, nbrs (per view), table): the inputs of every view."""
    import np_mvs_fuse as nf
    from mvs_scenes import render_scene, scene_cloud
    from sfm_mvs_amd import mvs
    if name == "quads":
        imgs, K, P, gt = render_scene(n=N_VIEWS, w=W, h=H, seed=0)
        gt_normal = None
    else:
        from mvs_slant_scenes import render_slant_scene
        imgs, K, P, gt, gt_normal, _ = render_slant_scene(n=N_VIEWS, w=W, h=H, seed=0)
    X = scene_cloud(K, P, gt)
    nbrs = [mvs.neighbours(i, N_VIEWS, NSRC) for i in range(N_VIEWS)]
    mats = [mvs.consistency_matrices(K, P[i], P[nbrs[i]]) for i in range(N_VIEWS)]
    table = nf.make_table(nbrs, [min(MIN_CONSISTENT, len(nb)) for nb in nbrs], [m[1] for m in mats], [m[0] for m in mats])
    return dict(images=imgs, K=K, P=P, gt=gt, gt_normal=gt_normal, cloud=X, nbrs=nbrs, mats=mats, table=table)


def view_maps(name, i, seeds=SEEDS):
    """The restated maps of view i as run_mvs makes them -> (sweep depth, {seed: (refined depth, normal)})."""
    import np_mvs
    import np_mvs_patchmatch as pm
    from mvs_scenes import gray
    from sfm_mvs_amd import mvs
    sc = scene(name)
    K, P, nb = sc["K"], sc["P"], sc["nbrs"][i]
    dmin, dmax = mvs.depth_range(sc["cloud"], P[i], P_all=P)
    invd = np.linspace(1.0 / dmax, 1.0 / dmin, NDEPTH, dtype=np.float64).astype(np.float32)
    ref, srcs, mv = gray(sc["images"][i]), [gray(sc["images"][v]) for v in nb], mvs.sweep_matrices(K, P[i], P[nb])
    sweep = np_mvs.plane_sweep(ref, srcs, mv, invd, RADIUS, TOPK, mvs.VAR_MIN, mvs.COST_MAX)[0]
    refined = {}
    for seed in seeds:
        out = pm.patchmatch(ref, srcs, mv, invd[0], invd[-1], RADIUS, TOPK, mvs.VAR_MIN, mvs.COST_MAX, sweep, mvs.PM_ITERS, int(mvs.PM_FAR),
                            mvs.PM_DEPTH_STEP, 1.0 / K[0, 0], seed, mvs.normal_matrix(K, P[i]))
        refined[seed] = (out[1], out[3])
    return sweep, refined


def cos_of(max_angle):
    """run_mvs's cos_min: -inf for None, else the cosine in float64 cast once."""
    return np.float32(-np.inf) if max_angle is None else np.float32(np.cos(np.deg2rad(np.float64(max_angle))))


def _cloud_figures(sc, pts):
    from mvs_scenes import surface_error
    e = surface_error(pts, sc["K"], sc["P"], sc["gt"]) if len(pts) else np.zeros(0)
    if not len(e):
        return dict(median=None, p90=None, within_1pct=None, within_025pct=None)
    return dict(median=float(np.median(e)), p90=float(np.percentile(e, 90)), within_1pct=float((e <= 0.01).mean()),
                within_025pct=float((e <= 0.0025).mean()))


def _angle(sc, keep, normals):
    """Median angle (degrees) between the unit normals at the kept pixels and the ground truth of the reference pixel."""
    t = np.stack(sc["gt_normal"])[keep]
    n = np.asarray(normals, np.float64)[keep]
    hit = np.abs(t).sum(-1) > 0
    return float(np.degrees(np.median(np.arccos(np.clip((n * t).sum(-1)[hit], -1.0, 1.0)))))


def filter_cloud(name, depth):
    """The cloud of the filter this fusion replaces: np_mvs.consistency view by view, as run_mvs(fuse=None) calls it -> (m, 3) float32."""
    import np_mvs
    sc = scene(name)
    pts = []
    for i, nb in enumerate(sc["nbrs"]):
        mask, xyz = np_mvs.consistency(depth[i], [depth[v] for v in nb], nb, sc["mats"][i][0], i, sc["mats"][i][1], TAU,
                                       min(MIN_CONSISTENT, len(nb)), True)
        pts.append(xyz[mask.astype(bool)])
    return np.concatenate(pts)


def fused_figures(name, normal, out, filter_pts):
    """The figures of one fused run: `out` the dict of np_mvs_fuse.fuse (or the device's words in the same layout); filter_pts (m, 3) the
    cloud the merged one is compared with: filter_cloud's where there is no angle bound, else the kept pixels' own samples."""
    sc = scene(name)
    keep = out["mask"].astype(bool)
    fig = dict(points=int(keep.sum()), filter_points=len(filter_pts), filter=_cloud_figures(sc, filter_pts),
               merged=_cloud_figures(sc, out["xyz"][keep]), support=[int(c) for c in np.bincount(out["support"][keep], minlength=10)[1:10]])
    if normal is not None and sc["gt_normal"] is not None:
        fig.update(normal_reference_deg=_angle(sc, keep, normal), normal_merged_deg=_angle(sc, keep, out["normal"]))
    return fig


def own_samples(name, depth):
    """[n, h, w, 3] float32: every pixel's own world sample, sfm_mvs_consistency's xyz word without the mask."""
    sc = scene(name)
    d = np.asarray(depth, np.float32)
    return np.stack([_own(d[i], sc["mats"][i][1]) for i in range(len(d))])


def _own(d, bc):
    from np_mvs import F, _grid
    h, w = d.shape
    fx, fy = _grid(w, h)
    b = np.asarray(bc, F)
    with np.errstate(all="ignore"):
        return np.stack([d * ((b[3 * i] * fx + b[3 * i + 1] * fy) + b[3 * i + 2]) + b[9 + i] for i in range(3)], -1).astype(F)


def frames(name):
    return np.stack(scene(name)["images"])


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def row(doc, scene_name, config, seed, max_angle):
    for r in doc["rows"]:
        if (r["scene"], r["config"], r["seed"], r["max_angle"]) == (scene_name, config, seed, max_angle):
            return r
    raise KeyError((scene_name, config, seed, max_angle))


def choose_max_angle(rows):
    """The smallest angle of ANGLES that keeps >= KEEP_SHARE of the unbounded point count on both scenes under refine on every seed."""
    ok = []
    for a in ANGLES[1:]:
        if all(r["points"] >= KEEP_SHARE * next(q["points"] for q in rows if (q["scene"], q["config"], q["seed"], q["max_angle"])
                                                == (r["scene"], "refine", r["seed"], None))
               for r in rows if r["config"] == "refine" and r["max_angle"] == a):
            ok.append(a)
    return min(ok) if ok else None


def round_sig(v, up):
    """v > 0 rounded up or down to two significant figures."""
    import math
    q = 10.0 ** (math.floor(math.log10(v)) - 1)
    return (math.ceil(v / q) if up else math.floor(v / q)) * q


def bars(row):
    """The asserted bars of a calibration row, each figure rounded one way to two significant figures: counts and shares down, errors
    and angles up."""
    out = dict(points=round_sig(row["points"], False))
    for cloud in ("filter", "merged"):
        for k, v in row[cloud].items():
            out[cloud, k] = round_sig(v, not k.startswith("within"))
    for k in ("normal_reference_deg", "normal_merged_deg"):
        if k in row:
            out[k] = round_sig(row[k], True)
    return out


def meets(fig, bar):
    """None, or the first figure of `fig` (fused_figures) that misses its bar."""
    for k, v in bar.items():
        got = fig[k[0]][k[1]] if isinstance(k, tuple) else fig[k]
        down = k == "points" or (isinstance(k, tuple) and k[1].startswith("within"))
        if (got < v) if down else (got > v):
            return k, got, v
    return None
