"""Scenes shared by the MVS-PLAN tests (docs/mvs.md §8.4): the rendered arc scene of mvs_scenes with its views in a permuted order and
tracks synthesised from the ground-truth depth, and the planted tracks of the ring scene.  NumPy and the test helpers only."""
import functools

import numpy as np

# The calibrated scene (docs/mvs.md §8.4): 9 views on an arc of 0.9 rad (0.11 rad between neighbours on the arc), 4 sources per view,
# the order of the frames permuted with default_rng(1): rendered views [7, 0, 1, 4, 2, 5, 8, 6, 3].  MIDDLE is the position of the
# arc's middle view (rendered view 4), the one the thresholds are held on, as the 5-view test holds them on its middle view.
SCENE = dict(n=9, w=160, h=120, seed=0, arc=0.9)
NSRC = 4
PERM_SEED = 1
MIDDLE = 3
NDEPTH = 64


@functools.lru_cache(maxsize=None)
def permuted_scene(perm_seed=PERM_SEED, **kw):
    """-> (images, K, P, gt, perm): render_scene(**SCENE) with view k of the result the rendered view perm[k]."""
    from mvs_scenes import render_scene
    args = dict(SCENE, **kw)
    imgs, K, P, gt = render_scene(**args)
    perm = np.random.default_rng(perm_seed).permutation(args["n"])
    return [imgs[k] for k in perm], K, np.ascontiguousarray(P[perm]), [gt[k] for k in perm], perm


def synth_tracks(K, P, gt, step=7, tol=0.01):
    """Tracks from the scene cloud and the ground-truth depth: point j is observed by the views into which it projects inside the frame
    with a camera depth within `tol` relative of the rendered one at its nearest pixel.  Points seen by fewer than two views are dropped.
    -> (X [npt, 3] float64, cam_idx, pt_idx int32 [nobs], point-major)."""
    from mvs_scenes import scene_cloud
    X = scene_cloud(K, P, gt, step)
    h, w = gt[0].shape
    Xh = np.hstack([X, np.ones((len(X), 1))]).T
    see = np.zeros((len(X), len(P)), bool)
    for k in range(len(P)):
        q = P[k] @ Xh
        with np.errstate(divide="ignore", invalid="ignore"):
            u, v = np.floor(q[0] / q[2] + 0.5), np.floor(q[1] / q[2] + 0.5)
        ok = (q[2] > 0) & (u >= 0) & (u <= w - 1) & (v >= 0) & (v <= h - 1)
        g = np.where(ok, gt[k][np.where(ok, v, 0).astype(int), np.where(ok, u, 0).astype(int)], 0.0)
        see[:, k] = ok & (g > 0) & (np.abs(q[2] - g) <= tol * g)
    keep = see.sum(1) >= 2
    X, see = X[keep], see[keep]
    pt_idx, cam_idx = np.nonzero(see)
    return np.ascontiguousarray(X), cam_idx.astype(np.int32), pt_idx.astype(np.int32)


def np_depth_map(imgs, K, P, i, nbrs, rng, ndepth=64, radius=3, topk=2):
    """View i swept with np_mvs against the views `nbrs` over the planes of the range `rng`, as run_mvs sweeps it."""
    import np_mvs
    from mvs_scenes import gray
    from sfm_mvs_amd import mvs
    invd = np.linspace(1.0 / rng[1], 1.0 / rng[0], ndepth).astype(np.float32)
    return np_mvs.plane_sweep(gray(imgs[i]), [gray(imgs[v]) for v in nbrs], mvs.sweep_matrices(K, P[i], P[list(nbrs)]), invd, radius,
                              min(topk, len(nbrs)), mvs.VAR_MIN, mvs.COST_MAX)[0]


def wrong_share(depth, truth, radius=3):
    """The share of interior pixels without a depth within 1 % of the truth (no depth counts as wrong)."""
    r = radius
    d, g = depth[r:-r, r:-r], truth[r:-r, r:-r]
    return float(1.0 - ((d > 0) & (np.abs(d - g) <= 0.01 * g)).mean())


def coverage(rng, truth):
    """The share of the rendered pixels of a view whose ground-truth depth lies inside the range."""
    g = truth[truth > 0]
    return float(((g >= rng[0]) & (g <= rng[1])).mean())


def ring_tracks(n_img=8, n_scene=400, seed=3):
    """The planted tracks of datagen.ring_scene(n_img, ., n_scene, seed): every image holds every scene point.
    -> (P [n_img, 3, 4], X [n_scene, 3], cam_idx, pt_idx)."""
    from datagen import ring_scene
    _, P, _ = ring_scene(n_img, n_scene + 200, n_scene, seed=seed)
    rng = np.random.default_rng(seed)                   # the scene points ring_scene draws first from its generator
    X = rng.normal(size=(n_scene, 3))
    X = X / np.maximum(np.linalg.norm(X, axis=1, keepdims=True), 1.0) * rng.uniform(0.2, 1.0, (n_scene, 1))
    pt_idx = np.repeat(np.arange(n_scene), n_img).astype(np.int32)
    cam_idx = np.tile(np.arange(n_img), n_scene).astype(np.int32)
    return np.asarray(P, np.float64), X, cam_idx, pt_idx
