"""The Gauss-Newton sweeps (csrc/residual.hip, csrc/ba_dense.hip), RANSAC scoring and the float64 projection of
csrc/ransac.hip on every launch path, against the float64 complex-step reference of np_ba.py at the project's bar for these
sums: |got - want|.max() <= 1e-10 |want|.max() per output.  Masks are compared bit for bit wherever the float32 rounding
of a projected coordinate is decidable (np_ba.f32_undecidable), the inclusive `err <= thr2` on planted exact ties.

test_np_gn_cpu.py shows on the CPU that every shape of gn_cases.DENSE_SHAPES / RESIDUAL_SHAPES lands on the plan claimed
for it (PP = 2 and 4, full and partial tiles, one to three camera chunks, 4 to 512 fold rows; the one-level fold up to its
2048 rows and reduce_rows_kernel with a second chunk of 1 and of 701 rows), that the reference alone is good to 1e-11 on
these very inputs, that the C oracle agrees with it, and that at most 0.1 % of any mask is left out as undecidable."""
import numpy as np
import pytest
import torch

import ba_cases
import gn_cases
import np_ba

pytestmark = pytest.mark.gpu

BAR = 1e-10
JAC = dict(want_jac=True, want_pt_jac=True, want_res2=True)


def cu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def rel(got, want):
    """max|got - want| / max|want|"""
    return float(np.abs(np.asarray(got) - want).max() / np.abs(want).max())


def host(out, ncam, npt):
    """(B [ncam, 6, 6], C [npt, 3, 3], gc [ncam, 6], gp [npt, 3]) of a sweep's dict."""
    return (out["JtJ_cam"].cpu().numpy().reshape(ncam, 6, 6), out["JtJ_pt"].cpu().numpy().reshape(npt, 3, 3),
            out["Jtr_cam"].cpu().numpy().reshape(ncam, 6), out["Jtr_pt"].cpu().numpy().reshape(npt, 3))


def with_pad_column(x):
    """The same points as a [:, :3] view of homogeneous rows: ldx = 4."""
    X4 = torch.cat([x, torch.full((x.shape[0], 1), 7.0, dtype=torch.float32, device="cuda")], 1)
    assert X4[:, :3].stride(0) == 4
    return X4[:, :3]


def same_bits(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


def block_figures(got, ref, rows=None):
    B, C, gc, gp = got
    if rows is not None:
        C, gp = C[rows], gp[rows]
    return {"B": rel(B, ref["B"]), "C": rel(C, ref["C"]), "gc": rel(gc, ref["gc"]), "gp": rel(gp, ref["gp"])}


def sumsq_ok(got, ref):
    """The float32 metric: the bar, plus what the undecidable roundings could move it by (0 for most shapes)."""
    return abs(got - ref["sumsq"]) <= BAR * ref["sumsq"] + ref["allow"]


# ---------------------------------------------------------------- the dense sweep on every launch plan
@pytest.mark.parametrize("shape", list(gn_cases.DENSE_SHAPES))
def test_dense_sweep_on_every_launch_plan(hip, shape):
    ncam, npt = shape
    K, cams, X, obs = gn_cases.dense_problem(*shape)
    ref = gn_cases.dense_reference(*shape)
    c, x, o = cu(cams), cu(X), cu(obs)
    out = hip.ba_dense_sweep(c, K, x, o)
    got = host(out, ncam, npt)
    figs = block_figures(got, ref, ref["rows"])
    sumsq = out["sumsq"].item()
    print(f"{shape}: " + "  ".join(f"{k} {v:.3g}" for k, v in figs.items()) + f"  sumsq {abs(sumsq - ref['sumsq']) / ref['sumsq']:.3g} (allowance {ref['allow'] / ref['sumsq']:.3g})")
    assert max(figs.values()) <= BAR, figs
    assert sumsq_ok(sumsq, ref)
    assert np.array_equal(got[0], got[0].transpose(0, 2, 1)) and np.array_equal(got[1], got[1].transpose(0, 2, 1))      # exactly symmetric
    assert same_bits(out, hip.ba_dense_sweep(c, K, x, o))                        # fixed-order reductions
    assert same_bits(out, hip.ba_dense_sweep(c, K, with_pad_column(x), o))       # ldx = 4
    cam_only, pt_only = hip.ba_dense_sweep(c, K, x, o, want_pt=False), hip.ba_dense_sweep(c, K, x, o, want_cam=False)
    assert set(cam_only) == {"sumsq", "JtJ_cam", "Jtr_cam"} and set(pt_only) == {"sumsq", "JtJ_pt", "Jtr_pt"}
    assert all(torch.equal(cam_only[k], out[k]) for k in cam_only) and all(torch.equal(pt_only[k], out[k]) for k in pt_only)


# ---------------------------------------------------------------- the single-camera path and its fold
def _single(hip, nobs, **kw):
    K, cams, X, obs = gn_cases.residual_problem(nobs)
    return hip.project_residual(cu(cams), K, cu(X), cu(obs), thr2=gn_cases.THR2, **kw)


@pytest.mark.parametrize("nobs", list(gn_cases.RESIDUAL_SHAPES))
def test_single_camera_path_on_every_fold_plan(hip, nobs):
    ref = gn_cases.residual_reference(nobs)
    out = _single(hip, nobs, want_inlier=True, **JAC)
    figs = block_figures(host(out, 1, nobs), ref)
    figs["res2"] = abs(out["res2"].item() - ref["res2"]) / ref["res2"]
    sumsq = out["sumsq"].item()
    print(f"nobs {nobs}: " + "  ".join(f"{k} {v:.3g}" for k, v in figs.items()) + f"  sumsq {abs(sumsq - ref['sumsq']) / ref['sumsq']:.3g} (allowance {ref['allow'] / ref['sumsq']:.3g})")
    assert max(figs.values()) <= BAR, figs
    assert sumsq_ok(sumsq, ref)
    ok = ~ref["und"]
    assert np.array_equal(out["proj"].cpu().numpy()[ok], ref["u"].astype(np.float32)[ok])
    assert np.array_equal(out["inlier"].cpu().numpy().astype(bool)[ok], ref["inlier"][ok])
    assert same_bits(out, _single(hip, nobs, want_inlier=True, **JAC))           # no atomics meet on this path
    # every pointer combination folds the same partial rows
    assert torch.equal(_single(hip, nobs, want_proj=False, want_res2=True)["res2"], out["res2"])
    assert torch.equal(_single(hip, nobs, want_proj=False)["sumsq"], out["sumsq"])          # MODE 0: final_reduce_kernel without Jacobians
    K, cams, X, obs = gn_cases.residual_problem(nobs)
    assert same_bits(out, hip.project_residual(cu(cams), K, with_pad_column(cu(X)), cu(obs), thr2=gn_cases.THR2, want_inlier=True, **JAC))


def test_two_level_fold_continues_the_one_level_fold(hip):
    """2048 * 256 observations fold in one level, one more takes reduce_rows_kernel: the sums may differ by that one
    observation's terms (its own sweep) and the bar, nothing else."""
    n = gn_cases.REDUCE_CHUNK * 256
    assert gn_cases.RESIDUAL_SHAPES[n][1] == 1 and gn_cases.RESIDUAL_SHAPES[n + 1][1] == 2
    one, two = _single(hip, n, **JAC), _single(hip, n + 1, **JAC)
    K, cams, X, obs = gn_cases.residual_problem(n + 1)
    last = hip.project_residual(cu(cams), K, cu(X[n:]), cu(obs[n:]), thr2=gn_cases.THR2, **JAC)
    for key in ("JtJ_cam", "Jtr_cam", "res2", "sumsq"):
        a, b, d = (t[key].cpu().numpy() for t in (one, two, last))
        fig = float(np.abs(b - (a + d)).max() / np.abs(b).max())
        print(f"{key}: {fig:.3g}")
        assert fig <= BAR, key
    assert torch.equal(one["JtJ_pt"], two["JtJ_pt"][:n]) and torch.equal(last["JtJ_pt"][0], two["JtJ_pt"][n])


# ---------------------------------------------------------------- indexed and half-indexed observations
@pytest.mark.parametrize("name", list(gn_cases.indexed_cases()))
def test_indexed_and_half_indexed_sweeps(hip, name):
    """ba_cases.indexed_cases() (nobs = 0, 1, 255, 256, 257; one pair 2000 times; a list repeated verbatim; cameras and points
    nobody sees) and the half-indexed forms: pt_idx alone (camera 0 in fixed order, gathered and repeated points: the
    per-point atomics collide) and cam_idx alone (observation o is of point o)."""
    K, cams, X, _, _ = ba_cases.indexed_problem()
    ci, pi, obs = gn_cases.indexed_cases()[name]
    ref = gn_cases.indexed_reference(name)
    args = (cu(cams), K, cu(X), cu(obs), cu(ci), cu(pi))
    out = hip.project_residual(*args, thr2=gn_cases.THR2, want_inlier=True, **JAC)
    got = host(out, 8, 300)
    assert out["proj"].shape == (len(obs), 2) and out["inlier"].shape == (len(obs),)
    if len(obs) == 0:
        assert not any(g.any() for g in got) and out["res2"].item() == 0.0 and out["sumsq"].item() == 0.0
        return
    figs = block_figures(got, ref)
    figs["res2"] = abs(out["res2"].item() - ref["res2"]) / ref["res2"]
    print(f"{name}: " + "  ".join(f"{k} {v:.3g}" for k, v in figs.items()))
    assert max(figs.values()) <= BAR, figs
    assert sumsq_ok(out["sumsq"].item(), ref)
    lc, lp = gn_cases.indexed_lists(name)
    seen_c, seen_p = np.zeros(8, bool), np.zeros(300, bool)
    seen_c[lc], seen_p[lp] = True, True
    assert not got[0][~seen_c].any() and not got[2][~seen_c].any() and not got[1][~seen_p].any() and not got[3][~seen_p].any()
    ok = ~ref["und"]
    assert np.array_equal(out["inlier"].cpu().numpy().astype(bool)[ok], ref["inlier"][ok])
    assert np.array_equal(out["proj"].cpu().numpy()[ok], ref["u"].astype(np.float32)[ok])
    # want_res2 alone: MODE 1 with every Jacobian pointer null, final_reduce_kernel with with_jac = 1
    alone = hip.project_residual(*args, thr2=gn_cases.THR2, want_proj=False, want_res2=True)
    assert set(alone) == {"sumsq", "res2"} and torch.equal(alone["res2"], out["res2"]) and torch.equal(alone["sumsq"], out["sumsq"])
    if ci is None:                                                               # camera 0's block comes from the fixed-order fold
        again = hip.project_residual(*args, thr2=gn_cases.THR2, want_inlier=True, **JAC)
        assert torch.equal(again["JtJ_cam"], out["JtJ_cam"]) and torch.equal(again["Jtr_cam"], out["Jtr_cam"])


# ---------------------------------------------------------------- camera-table and depth edges through three paths
def _rows(got, want, scale):
    """max over rows of |got - want|.max(row) / scale.max(row)"""
    n = len(want)
    return float((np.abs(got - want).reshape(n, -1).max(1) / scale.reshape(n, -1).max(1)).max())


@pytest.mark.parametrize("name", ["edge_problem", "depth_problem"])
def test_camera_and_depth_edges(hip, name):
    """edge_problem: rotation-vector norms 0, 1e-20, 1e-12, 1e-8, 1e-4, pi - 1e-6, pi, 4 (both sides of the kernels'
    theta < DBL_EPSILON branch), one point with z' = 0 exactly (the z := 1 convention), points behind a camera;
    depth_problem: depths 1e-6 .. 1e6.  The dense sweep (axes w_j = (dR/dr_j) R^T, fused multiply-adds, its own reciprocal),
    the indexed sweep with full visibility and the single-camera path camera by camera: finite, at the bar against the
    reference overall and row by row against the rows' sums of magnitudes (sum |J|^T |J| and sum |J|^T |r|), and at the same
    bar against each other.  (Camera 3, theta = 1e-8, is where (1 - cos theta) / theta formed by subtraction costs
    residual.hip's paths 1.26e-9 of that camera's row of JtJ_cam; the dense sweep only takes the skew part of
    (dR/dr_j) R^T, which the lost, symmetric term does not reach.)"""
    K, cams, X, obs = gn_cases.edge_observations(name)
    ref, mag = gn_cases.edge_reference(name), gn_cases.edge_reference(name, magnitude=True)
    c, x = cu(cams), cu(X)
    paths = {"dense": host(hip.ba_dense_sweep(c, K, x, cu(obs)), 12, 600)}
    idx = hip.project_residual(c, K, x, cu(obs.reshape(-1, 2)), *(cu(i) for i in ba_cases.full_visibility(12, 600)), **JAC)
    paths["indexed"] = host(idx, 12, 600)
    per_cam = [hip.project_residual(c[i:i + 1], K, x, cu(obs[i]), **JAC) for i in range(12)]
    singles = [host(o, 1, 600) for o in per_cam]
    paths["single"] = (np.concatenate([s[0] for s in singles]), np.sum([s[1] for s in singles], 0),
                       np.concatenate([s[2] for s in singles]), np.sum([s[3] for s in singles], 0))
    figs = {}
    for what, got in paths.items():
        assert all(np.all(np.isfinite(g)) for g in got), what
        figs[what] = [rel(got[k], ref[k]) for k in range(4)] + [_rows(got[k], ref[k], mag[k]) for k in range(4)]
    for a, b in (("dense", "indexed"), ("dense", "single"), ("indexed", "single")):
        figs[a + "-" + b] = [rel(paths[a][k], paths[b][k]) for k in range(4)] + [_rows(paths[a][k], paths[b][k], mag[k]) for k in range(4)]
    res2 = {"indexed": idx["res2"].item(), "single": float(np.sum([o["res2"].item() for o in per_cam]))}
    print(name, {k: " ".join(f"{f:.2g}" for f in v) for k, v in figs.items()}, {k: f"{abs(v - ref[4]) / ref[4]:.2g}" for k, v in res2.items()})
    for what, f in figs.items():
        assert max(f) <= BAR, (what, f)
    assert all(abs(v - ref[4]) <= BAR * ref[4] for v in res2.values())


# ---------------------------------------------------------------- RANSAC scoring
def _check_scores(got_counts, got_mask, got_counts_only, counts, mask, und):
    gm, gc = got_mask.cpu().numpy().astype(bool), got_counts.cpu().numpy()
    assert gm.shape == mask.shape and gc.dtype == np.int32
    assert np.array_equal(gm[~und], mask[~und])
    assert np.array_equal(gc, gm.sum(1))                                         # the counts are the masks' sums, exactly
    clear = ~und.any(1)
    assert np.array_equal(gc[clear], counts[clear]) and np.all(np.abs(gc - counts) <= und.sum(1))
    assert torch.equal(got_counts_only, got_counts)                              # want_mask=False: the same counts


@pytest.mark.parametrize("h,n", gn_cases.SCORE_CASES)
def test_scoring_masks_and_counts(hip, h, n):
    """h = 1, 5, 64 hypotheses on n points on both sides of a wave and of a workgroup, and the grid limit h = 65 535."""
    K, poses, X, obs = gn_cases.pnp_scoring_case(h, n)
    args = (cu(poses), K, cu(X), cu(obs), gn_cases.THR2)
    _check_scores(*hip.score_pnp(*args, want_mask=True), hip.score_pnp(*args), *np_ba.score_pnp(poses, K, X, obs, gn_cases.THR2))
    Es, x1, x2 = gn_cases.essential_scoring_case(h, n)
    args = (cu(Es), cu(x1), cu(x2), gn_cases.ESSENTIAL_THR2)
    _check_scores(*hip.score_essential(*args, want_mask=True), hip.score_essential(*args), *np_ba.score_essential(Es, x1, x2, gn_cases.ESSENTIAL_THR2))


def test_scoring_hypothesis_count_limits(hip):
    """h = 65 536 exceeds the grid's y extent: refused by the argument check, which stands before the first launch; h = 0
    returns empty outputs."""
    K, _, X, obs = gn_cases.pnp_scoring_case(1, 3)
    _, x1, x2 = gn_cases.essential_scoring_case(1, 3)
    with pytest.raises(hip.SfmHipError):
        hip.score_pnp(torch.zeros((65536, 6), dtype=torch.float64, device="cuda"), K, cu(X), cu(obs), gn_cases.THR2)
    with pytest.raises(hip.SfmHipError):
        hip.score_essential(torch.zeros((65536, 9), dtype=torch.float64, device="cuda"), cu(x1), cu(x2), gn_cases.ESSENTIAL_THR2)
    counts, mask = hip.score_pnp(torch.zeros((0, 6), dtype=torch.float64, device="cuda"), K, cu(X), cu(obs), gn_cases.THR2, want_mask=True)
    assert counts.shape == (0,) and mask.shape == (0, 3)
    counts, mask = hip.score_essential(torch.zeros((0, 9), dtype=torch.float64, device="cuda"), cu(x1), cu(x2), gn_cases.ESSENTIAL_THR2, want_mask=True)
    assert counts.shape == (0,) and mask.shape == (0, 3)
    torch.cuda.synchronize()


def test_planted_ties_are_inliers(hip):
    """`err <= thr2` is inclusive.  gn_cases.pnp_tie / essential_tie put the first half of the points exactly ON the
    threshold and the second half one float32 step above it, with every intermediate exact in float32 and float64: a
    rewrite to `<`, or any inexact step on the way, changes the mask."""
    K, pose, X, obs, want = gn_cases.pnp_tie()
    counts, mask = hip.score_pnp(cu(pose), K, cu(X), cu(obs), 64.0, want_mask=True)
    assert np.array_equal(mask.cpu().numpy()[0].astype(bool), want) and counts.item() == want.sum()
    out = hip.project_residual(cu(pose), K, cu(X), cu(obs), thr2=64.0, want_inlier=True)
    assert np.array_equal(out["inlier"].cpu().numpy().astype(bool), want)
    assert np.array_equal(out["proj"].cpu().numpy(), X[:, :2])                   # u = x, v = y exactly
    E, x1, x2, thr2, want = gn_cases.essential_tie()
    counts, mask = hip.score_essential(cu(E), cu(x1), cu(x2), thr2, want_mask=True)
    assert np.array_equal(mask.cpu().numpy()[0].astype(bool), want) and counts.item() == want.sum()


# ---------------------------------------------------------------- the float64 projection
@pytest.mark.parametrize("n", gn_cases.PROJECT_N)
def test_project_points_f64(hip, n):
    """Every camera of edge_problem (the rotation norms above; camera 0 has point 0 at z' = 0 and points 1..5 behind it)
    on float64 points: 1e-13 relative + 1e-13 px."""
    K, cams, _, _, _ = ba_cases.edge_problem()
    X = gn_cases.project_points_input(n)
    x = cu(X)
    worst = 0.0
    for c in cams:
        want = np_ba.project_points(c[:3], c[3:], K, X)
        got = hip.project_points_f64(c[:3], c[3:], K, x).cpu().numpy()
        assert got.shape == (n, 2) and np.all(np.isfinite(got))
        worst = max(worst, float((np.abs(got - want) / (np.abs(want) + 1.0)).max()))
        assert np.all(np.abs(got - want) <= 1e-13 * np.abs(want) + 1e-13)
    print(f"project_points_f64 n = {n}: worst |got - want| / (|want| + 1) = {worst:.3g}")
