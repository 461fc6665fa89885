"""Plane-sweep MVS without a GPU: the C-ABI declares and validates the two entry points, the host-side matrices agree with an
independent derivation, the float32 checker stands apart from the product, and the algorithm itself (tests/np_mvs.py, the
kernels' arithmetic) recovers the ground truth of a rendered scene — where the thresholds the GPU end-to-end test reuses, and
the defaults of mvs.run_mvs, are set."""
import ast
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

# Accuracy of a depth map on tests/mvs_scenes.render_scene (5 views, 160 x 120, reference = the middle view, its 4 neighbours as
# sources, 64 planes over the range depth_range() takes from ground-truth points, r = 3, top 2, run_mvs's var_min / cost_max).
# Measured with np_mvs: 99.9 % of interior pixels get a depth, 92 % of those within 1 % of the truth (seeds 0..2).
MIN_VALID_FRACTION = 0.95          # interior pixels (reference window in the frame) with depth > 0
MIN_WITHIN_1PCT = 0.85             # of those, |depth - truth| <= 1 % of truth
# The fused cloud of the same scene (all 5 views, 128 planes, run_mvs's defaults): 95.6 % of its points lie, in some view, within
# 1 % of the ground-truth depth at their pixel (np_mvs, seed 0).
MIN_FUSED_WITHIN_1PCT = 0.90


def test_header_declares_the_mvs_entry_points():
    from test_abi import declared_symbols
    syms = declared_symbols()
    assert "sfm_mvs_plane_sweep" in syms and "sfm_mvs_consistency" in syms


def test_argument_errors_are_reported_before_the_device():
    from sfm_mvs_amd import _lib
    L = _lib.lib()
    fake = ctypes.c_void_p(16)                       # never dereferenced: every check below fails first
    srcs = (ctypes.c_void_p * 8)(*([16] * 8))
    mv = (ctypes.c_float * 96)()

    def sweep(nsrc=2, w=64, h=48, ndepth=16, radius=3, topk=2, var_min=100.0, cost_max=0.5, ref=fake, depth=fake):
        return L.sfm_mvs_plane_sweep(ref, srcs, mv, nsrc, w, h, fake, ndepth, radius, topk, var_min, cost_max, depth, fake, None, None, None)

    for kw, msg in [(dict(radius=0), b"radius"), (dict(radius=5), b"radius"), (dict(nsrc=0), b"nsrc"), (dict(nsrc=9), b"nsrc"),
                    (dict(topk=3), b"topk"), (dict(topk=0), b"topk"), (dict(ndepth=1), b"ndepth"), (dict(ndepth=1025), b"ndepth"),
                    (dict(w=6), b"frame"), (dict(h=6, radius=3), b"frame"), (dict(var_min=0.0), b"var_min"),
                    (dict(cost_max=float("nan")), b"cost_max"), (dict(ref=None), b"null"), (dict(depth=None), b"null")]:
        assert sweep(**kw) == -1, kw
        assert msg in L.sfm_last_error(), (kw, L.sfm_last_error())
    nulls = (ctypes.c_void_p * 2)(16, 0)
    assert L.sfm_mvs_plane_sweep(fake, nulls, mv, 2, 64, 48, fake, 16, 3, 2, 100.0, 0.5, fake, fake, None, None, None) == -1
    assert b"source frame 1 is null" in L.sfm_last_error()

    idx = (ctypes.c_int32 * 8)()

    def cons(nview=2, min_consistent=2, w=64, h=48, tau=0.01, depth=fake, nbrs=srcs):
        return L.sfm_mvs_consistency(depth, nbrs, idx, mv, nview, 0, mv, w, h, tau, min_consistent, 1, fake, fake, None)

    for kw, msg in [(dict(nview=9), b"nview"), (dict(min_consistent=3), b"min_consistent"), (dict(w=0), b"frame"),
                    (dict(tau=-1.0), b"tau"), (dict(depth=None), b"null"), (dict(nbrs=None), b"null")]:
        assert cons(**kw) == -1, kw
        assert msg in L.sfm_last_error(), (kw, L.sfm_last_error())


def _cameras(seed):
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(seed)
    K = np.array([[rng.uniform(400, 900), 0.0, rng.uniform(200, 500)], [0.0, rng.uniform(400, 900), rng.uniform(150, 350)], [0, 0, 1.0]])
    Ps = []
    for _ in range(5):
        R = Rotation.from_rotvec(rng.normal(0, 0.2, 3)).as_matrix()
        Ps.append(K @ np.hstack([R, rng.normal(0, 1.0, (3, 1))]))
    return K, np.stack(Ps)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_matrices_agree_with_an_independent_derivation(seed):
    """sweep_matrices / consistency_matrices against the projection matrices themselves: the world point X at camera depth d
    behind reference pixel x solves P_r[:, :3] X = d x~ - P_r[:, 3] (P = K [R|t]); source s then sees P_s (X, 1)."""
    from sfm_mvs_amd import mvs
    K, Ps = _cameras(seed)
    rng = np.random.default_rng(100 + seed)
    mvm = mvs.sweep_matrices(K, Ps[0], Ps[1:])
    ab, bc = mvs.consistency_matrices(K, Ps[0], Ps[1:])
    assert mvm.dtype == np.float32 and mvm.shape == (4, 12) and ab.dtype == np.float32 and bc.shape == (12,)
    assert np.array_equal(ab, mvm)
    for _ in range(20):
        x = np.array([rng.uniform(0, 900), rng.uniform(0, 600), 1.0])
        d = rng.uniform(1, 50)
        X = np.linalg.solve(Ps[0][:, :3], d * x - Ps[0][:, 3])
        B, c = bc[:9].astype(np.float64).reshape(3, 3), bc[9:].astype(np.float64)
        assert np.allclose(d * (B @ x) + c, X, rtol=1e-6, atol=1e-6 * np.abs(X).max())
        for s in range(4):
            M, v = mvm[s, :9].astype(np.float64).reshape(3, 3), mvm[s, 9:].astype(np.float64)
            want = Ps[1 + s] @ np.append(X, 1.0)
            got = d * (M @ x) + v
            assert np.allclose(got, want, rtol=1e-6, atol=1e-6 * np.abs(want).max())
            got_plane = M @ x + v / d                     # the sweep's form: h = M x~ + v invd (homogeneous, = P_s X / d)
            assert np.allclose(got_plane * d, want, rtol=1e-6, atol=1e-6 * np.abs(want).max())


def test_neighbours_and_depth_range():
    from sfm_mvs_amd import mvs
    assert mvs.neighbours(5, 10, 4) == [4, 6, 3, 7]
    assert mvs.neighbours(0, 10, 4) == [1, 2, 3, 4]
    assert mvs.neighbours(9, 10, 2) == [8, 7]
    assert mvs.neighbours(1, 3, 4) == [0, 2]
    P = np.hstack([np.eye(3), np.zeros((3, 1))])
    X = np.column_stack([np.zeros(101), np.zeros(101), np.linspace(2.0, 12.0, 101)])
    lo, hi = mvs.depth_range(X, P)
    assert np.isclose(lo, 0.8 * np.percentile(X[:, 2], 2)) and np.isclose(hi, 1.25 * np.percentile(X[:, 2], 98))
    behind = np.hstack([np.eye(3), np.array([[0.0], [0.0], [-20.0]])])
    assert mvs.depth_range(X, behind, P_all=[behind, P]) == (lo, hi)       # nothing in front: all cameras' points pooled
    with pytest.raises(mvs.SfmHipError):
        mvs.depth_range(X, behind)


def test_the_checker_does_not_import_the_product():
    for rel in ("tests/np_mvs.py", "tests/mvs_scenes.py"):
        tree = ast.parse(open(os.path.join(ROOT, rel)).read())
        for node in ast.walk(tree):
            names = [a.name for a in node.names] if isinstance(node, ast.Import) else [node.module or ""] if isinstance(node, ast.ImportFrom) else []
            assert not any(n.split(".")[0] in ("sfm_mvs_amd", "oracle") for n in names), f"{rel} imports {names}"


def scene_depth_map(seed, ndepth=64, radius=3, topk=2, var_min=None, cost_max=None):
    """The middle view of a rendered 5-view scene swept with np_mvs as run_mvs would (depth range from the ground-truth cloud)."""
    import np_mvs
    from mvs_scenes import gray, render_scene
    from sfm_mvs_amd import mvs
    imgs, K, P, gt = render_scene(n=5, w=160, h=120, seed=seed)
    pts = []
    for k in range(5):                                 # a sparse cloud: every 7th ground-truth pixel of every view, in world units
        R, t = np.linalg.solve(K, P[k])[:, :3], np.linalg.solve(K, P[k])[:, 3]
        ys, xs = np.nonzero(gt[k][::7, ::7] > 0)
        ys, xs = ys * 7, xs * 7
        d = gt[k][ys, xs]
        rays = np.linalg.solve(K, np.stack([xs, ys, np.ones_like(xs)]).astype(np.float64))
        pts.append((R.T @ (rays * d - t[:, None])).T)
    X = np.vstack(pts)
    i = 2
    nb = mvs.neighbours(i, 5, 4)
    dmin, dmax = mvs.depth_range(X, P[i], P_all=P)
    invd = np.linspace(1.0 / dmax, 1.0 / dmin, ndepth).astype(np.float32)
    depth, cost, plane, _ = np_mvs.plane_sweep(gray(imgs[i]), [gray(imgs[v]) for v in nb], mvs.sweep_matrices(K, P[i], P[nb]), invd,
                                               radius, topk, mvs.VAR_MIN if var_min is None else var_min,
                                               mvs.COST_MAX if cost_max is None else cost_max)
    return depth, gt[i], radius


def depth_accuracy(depth, truth, radius):
    """(fraction of interior pixels with a depth, fraction of those within 1 % of the truth)."""
    r = radius
    d, g = depth[r:-r, r:-r], truth[r:-r, r:-r]
    valid = d > 0
    return float(valid.mean()), float((np.abs(d[valid] - g[valid]) <= 0.01 * g[valid]).mean())


@pytest.mark.parametrize("seed", [0, 1])
def test_algorithm_accuracy_on_a_rendered_scene(seed):
    depth, truth, r = scene_depth_map(seed)
    valid, within = depth_accuracy(depth, truth, r)
    assert valid >= MIN_VALID_FRACTION and within >= MIN_WITHIN_1PCT, (valid, within)


def test_fused_cloud_lies_on_the_rendered_surfaces():
    """run_mvs's defaults, restated with np_mvs on the 5-view scene: sweeps, consistency, view-major compaction."""
    import np_mvs
    from mvs_scenes import gray, render_scene, scene_cloud, surface_error
    from sfm_mvs_amd import mvs
    imgs, K, P, gt = render_scene(n=5, w=160, h=120, seed=0)
    X, n = scene_cloud(K, P, gt), 5
    nbrs = [mvs.neighbours(i, n, 4) for i in range(n)]
    depths = []
    for i in range(n):
        invd = np.linspace(*[1.0 / d for d in mvs.depth_range(X, P[i], P_all=P)[::-1]], 128).astype(np.float32)
        depths.append(np_mvs.plane_sweep(gray(imgs[i]), [gray(imgs[v]) for v in nbrs[i]], mvs.sweep_matrices(K, P[i], P[nbrs[i]]), invd,
                                         3, 2, mvs.VAR_MIN, mvs.COST_MAX)[0])
    masks, xyzs = [], []
    for i in range(n):
        ab, bc = mvs.consistency_matrices(K, P[i], P[nbrs[i]])
        m, x = np_mvs.consistency(depths[i], [depths[v] for v in nbrs[i]], nbrs[i], ab, i, bc, 0.01, 2, True)
        masks.append(m)
        xyzs.append(x)
    pts = np.stack(xyzs).reshape(-1, 3)[np.flatnonzero(np.stack(masks).reshape(-1))].astype(np.float64)
    assert len(pts) > 5000
    assert float((surface_error(pts, K, P, gt) <= 0.01).mean()) >= MIN_FUSED_WITHIN_1PCT


def _window_total(a, r):
    """Sum over the (2r+1)^2 window about every interior pixel, float64, explicit loops over the window's offsets."""
    h, w = a.shape
    out = np.zeros((h - 2 * r, w - 2 * r), np.float64)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out += a[dy:dy + h - 2 * r, dx:dx + w - 2 * r]
    return out


def zncc_cost_f64_with_bound(R, W, valid, r, var_min):
    """1 - ZNCC of the float32 frames R (reference I') and W (warped source, as given) in float64, two passes (means, then the
    moments of the deviations), and the first-order bound of what the float32 one-pass route of the header may differ by.
    -> (c64 clamped to [0, 2], ok64, bound on |c32 - c64|, near: var within its bound of var_min), all [h - 2r, w - 2r].

    float32 route: each of the five sums S_r, S_rr, S_w, S_ww, S_rw adds (2r+1)^2 terms, row sums left to right and the row sums
    top to bottom, so that any term passes k = 4r additions: |error| <= k u sum|x_i| with u = 2^-24 (recursive summation), and
    one more u for the rounded products.  var = S_xx - (S_x*S_x)/n rounds three times more, cov likewise; the quotient
    cov / sqrt(var_r*var_w) takes the relative errors of its parts to first order."""
    u = 2.0 ** -24
    k = 4 * r
    n = float((2 * r + 1) ** 2)
    R, W = R.astype(np.float64), W.astype(np.float64)
    h, w = R.shape
    ih, iw = h - 2 * r, w - 2 * r
    m_r, m_w = _window_total(R, r) / n, _window_total(W, r) / n
    var_r, var_w, cov = (np.zeros((ih, iw)) for _ in range(3))
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            a, b = R[dy:dy + ih, dx:dx + iw] - m_r, W[dy:dy + ih, dx:dx + iw] - m_w
            var_r += a * a
            var_w += b * b
            cov += a * b
    bad = _window_total((~valid).astype(np.float64), r) > 0
    # errors of the float32 sums
    e_r, e_w = k * u * _window_total(np.abs(R), r), k * u * _window_total(np.abs(W), r)
    e_rr, e_ww, e_rw = ((k + 1) * u * _window_total(np.abs(x), r) for x in (R * R, W * W, R * W))
    s_r, s_w = n * m_r, n * m_w
    e_var_r = e_rr + 2 * np.abs(s_r) * e_r / n + 2 * u * s_r * s_r / n + u * np.abs(var_r)
    e_var_w = e_ww + 2 * np.abs(s_w) * e_w / n + 2 * u * s_w * s_w / n + u * np.abs(var_w)
    e_cov = e_rw + (np.abs(s_r) * e_w + np.abs(s_w) * e_r) / n + 2 * u * np.abs(s_r * s_w) / n + u * np.abs(cov)
    near = (np.abs(var_r - var_min) <= e_var_r) | (np.abs(var_w - var_min) <= e_var_w)
    ok = ~bad & ~(var_r < var_min) & ~(var_w < var_min)
    with np.errstate(divide="ignore", invalid="ignore"):
        root = np.sqrt(np.where(ok, var_r * var_w, 1.0))
        q = cov / root
        rel_root = 0.5 * (e_var_r / np.where(ok, var_r, 1.0) + e_var_w / np.where(ok, var_w, 1.0) + u) + u
        e_q = e_cov / root + np.abs(q) * (rel_root + u)
        c = 1.0 - q
    bound = e_q + u * np.abs(c)
    return np.where(ok, np.clip(c, 0.0, 2.0), 2.0), ok, bound, near & ~bad


MAX_LEFT_OUT = 0.01                # of the interior pixel-plane pairs: variance within its error bound of var_min


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("radius", [1, 3])
def test_one_pass_float32_moments_stay_within_their_error_bound_of_float64(seed, radius):
    """The checker's own delicate step: np_mvs.plane_sweep's per-source cost (one source, topk 1, the volume) against a float64
    two-pass ZNCC over the SAME float32 warped frame, per pixel and plane within the propagated rounding bound; validity agrees
    exactly outside the band where the float64 variance lies within its bound of var_min (at most 1 % of the pairs)."""
    import np_mvs
    from mvs_scenes import gray, render_scene
    from sfm_mvs_amd import mvs
    var_min = 150.0
    imgs, K, P, _ = render_scene(n=5, w=160, h=120, seed=seed)
    grays = [gray(im) for im in imgs]
    invd = np.linspace(1.0 / 9.0, 1.0 / 1.5, 12).astype(np.float32)
    R = grays[2].astype(np.float32) - np.float32(128)
    worst, left_out, pairs = 0.0, 0, 0
    for v in mvs.neighbours(2, 5, 4):
        mv = mvs.sweep_matrices(K, P[2], P[[v]])
        c32 = np_mvs.plane_sweep(grays[2], [grays[v]], mv, invd, radius, 1, var_min, 2.5)[3][:, radius:-radius, radius:-radius]
        for j in range(len(invd)):
            W, valid = np_mvs.warp(grays[v], mv[0], invd[j], 160, 120)
            c64, ok, bound, near = zncc_cost_f64_with_bound(R, W, valid, radius, var_min)
            keep = ~near
            assert np.all(c32[j][keep & ~ok] == 2.0)
            sel = keep & ok
            ratio = np.abs(c32[j][sel].astype(np.float64) - c64[sel]) / bound[sel]
            worst = max(worst, float(ratio.max()) if ratio.size else 0.0)
            left_out += int(near.sum())
            pairs += near.size
    print(f"seed {seed} r {radius}: largest |c32 - c64| / bound {worst:.3f}, left out {left_out} of {pairs} pairs ({100.0 * left_out / pairs:.4f} %)")
    assert worst <= 1.0, worst
    assert left_out <= MAX_LEFT_OUT * pairs, (left_out, pairs)
