"""Pins the float64 NumPy reference of the BA linear algebra (np_ba.py) against independent implementations, shows that
on every product input of test_gpu_ba_schur.py the reference ALONE holds the 1e-10 bar (two summation orders agree to
1e-11), pins the launch-plan table those tests rely on, and measures how far the PCG recurrence itself lands from the
direct solve (the figures the GPU test's allowance is derived from).  No GPU."""
import numpy as np
import pytest

import ba_cases
import np_ba
from datagen import ba_problem


def _central_difference_jacobians(cams, K, X):
    ncam, npt = len(cams), len(X)
    X = X.astype(np.float64)
    Jc, Jp = np.empty((ncam, npt, 2, 6)), np.empty((ncam, npt, 2, 3))
    for a in range(6):
        h = 1e-6 * np.maximum(1.0, np.abs(cams[:, a]))
        d = np.zeros_like(cams); d[:, a] = h
        Jc[..., a] = (np_ba.project(cams + d, K, X) - np_ba.project(cams - d, K, X)) / (2 * h)[:, None, None]
    for a in range(3):
        d = np.zeros(3); d[a] = 1e-6
        Jp[..., a] = (np_ba.project(cams, K, X + d) - np_ba.project(cams, K, X - d)) / 2e-6
    return Jc, Jp


def test_rotation_matches_scipy_and_is_exact_at_tiny_angles():
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(0)
    r = rng.standard_normal((200, 3))
    r *= (rng.uniform(0, 4.0, 200) / np.linalg.norm(r, axis=1))[:, None]
    assert np.abs(np_ba.rotation(r) - Rotation.from_rotvec(r).as_matrix()).max() <= 4e-16 * 4
    for norm in ba_cases.EDGE_NORMS:
        rv = np.array([0.6, -0.48, 0.64]) * norm
        R = np_ba.rotation(rv)
        assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-15
        assert np.abs(R - Rotation.from_rotvec(rv).as_matrix()).max() <= 1e-15
    assert np.array_equal(np_ba.rotation(np.zeros(3)), np.eye(3))
    tiny = np_ba.rotation(np.array([1e-20, 0, 0]))
    assert tiny[2, 1] == 1e-20 and tiny[1, 2] == -1e-20 and tiny[0, 0] == 1.0


def test_complex_step_jacobians_match_central_differences():
    K, cams, X, _ = ba_problem(9, 700, 0.5, seed=31)
    Jc, Jp = np_ba.jacobians(cams, K, X)
    Fc, Fp = _central_difference_jacobians(cams, K, X)
    assert np.abs(Jc - Fc).max() <= 1e-6 * np.abs(Jc).max()
    assert np.abs(Jp - Fp).max() <= 1e-6 * np.abs(Jp).max()
    sub_c, sub_p = np_ba.jacobians(cams, K, X, [8, 2], [699, 0, 5])                   # the subset form is the same numbers
    assert np.array_equal(sub_c, Jc[[8, 2]][:, [699, 0, 5]]) and np.array_equal(sub_p, Jp[[8, 2]][:, [699, 0, 5]])
    ci, pi = np.array([0, 8, 3]), np.array([5, 699, 5])
    pc, pp = np_ba.pair_jacobians(cams, K, X, ci, pi)
    assert np.array_equal(pc, Jc[ci, pi]) and np.array_equal(pp, Jp[ci, pi])


def test_jacobians_at_the_identity_camera_are_the_generators():
    """theta = 0: dR/dr_k is the k-th generator, so d(RX)/dr = -[X]x — what the kernel's theta < DBL_EPSILON branch writes."""
    K = np.array([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1]])
    X = np.array([[0.5, -0.25, 2.0]], np.float32)
    Jc, Jp = np_ba.jacobians(np.zeros((1, 6)), K, X)
    x, y, z = 0.5, -0.25, 2.0
    want_u = [-(x / z) * (y / z), 1 + (x / z) ** 2, -y / z, 1 / z, 0, -x / z ** 2]
    assert np.allclose(Jc[0, 0, 0], want_u, rtol=1e-15, atol=0)
    assert np.allclose(Jp[0, 0], [[1 / z, 0, -x / z ** 2], [0, 1 / z, -y / z ** 2]], rtol=1e-15, atol=0)


def test_normal_equation_blocks_match_the_oracle(oracle):
    ncam, npt = 7, 400
    K, cams, X, obs = ba_problem(ncam, npt, 0.5, seed=3)
    B, C, gc, gp, sumsq, _ = np_ba.normal_blocks(cams, K, X, obs)
    ci, pi = ba_cases.full_visibility(ncam, npt)
    want = oracle.project_residual(cams, K, X, obs.reshape(-1, 2), ci, pi)
    for got, key in ((B, "JtJ_cam"), (C, "JtJ_pt"), (gc, "Jtr_cam"), (gp, "Jtr_pt")):
        w = want[key].reshape(got.shape)
        assert np.abs(got - w).max() <= 1e-10 * np.abs(w).max(), key
    # (the oracle's `sumsq` squares the float32-rounded residual, as the reference does; `res2` is the float64 residual's)
    assert sumsq == pytest.approx(want["res2"][0], rel=1e-10)


def test_direct_and_pcg_steps_match_the_full_normal_equations():
    ncam, npt, lam = 5, 80, 1e-2
    K, cams, X, obs = ba_problem(ncam, npt, 0.5, seed=32)
    B, C, gc, gp, _, W = np_ba.normal_blocks(cams, K, X, obs)
    fc, fp = np_ba.solve_full(B, C, gc, gp, W, lam)
    dc, dp = np_ba.solve_direct(B, C, gc, gp, W, lam, fix_first=False)
    assert np.abs(dc - fc).max() <= 1e-9 * np.abs(fc).max() and np.abs(dp - fp).max() <= 1e-9 * np.abs(fp).max()
    pc, pp, it = np_ba.solve_pcg(B, C, gc, gp, W, lam, False, tol=1e-13, iters=200)
    assert 0 < it < 200 and it % 5 == 0
    assert np.abs(pc - dc).max() <= 1e-8 * np.abs(dc).max() and np.abs(pp - dp).max() <= 1e-8 * np.abs(dp).max()
    d0, _ = np_ba.solve_direct(B, C, gc, gp, W, lam, fix_first=True)
    p0, _, _ = np_ba.solve_pcg(B, C, gc, gp, W, lam, True, tol=1e-13, iters=200)
    assert np.all(d0[0] == 0) and np.all(p0[0] == 0) and np.abs(p0 - d0).max() <= 1e-8 * np.abs(d0).max()
    assert np.abs(d0 - dc).max() > 1e-3 * np.abs(dc).max()                          # the gauge does change the step


# ---------------------------------------------------------------- the shape table
@pytest.mark.parametrize("shape", list(ba_cases.PRODUCT_SHAPES))
def test_plan_table(shape):
    """If the chunking is retuned, this names the shapes that no longer cover the path the table claims for them."""
    pp, tiles, nch_wt, nch_w, _ = ba_cases.PRODUCT_SHAPES[shape]
    assert ba_cases.schur_plan(*shape, cam_side=False) == (pp, tiles, nch_wt), shape
    assert ba_cases.schur_plan(*shape, cam_side=True) == (pp, tiles, nch_w), shape


def test_plan_table_covers_every_launch_path():
    plans = {s: ba_cases.PRODUCT_SHAPES[s] for s in ba_cases.PRODUCT_SHAPES}
    assert {p[0] for p in plans.values()} == {2, 4}                                                       # both PP kernels
    assert any(p[0] == 4 and p[2] > 1 for p in plans.values())                                            # PP = 4 with chunks
    assert any(p[2] != p[3] for p in plans.values())                                                      # differing nch per side
    uneven = [s for s, p in plans.items() if p[2] > 1 and s[0] % p[2]]
    even = [s for s, p in plans.items() if p[2] > 1 and s[0] % p[2] == 0]
    assert uneven and even
    assert ba_cases.chunk_bounds(33, 2) == [(0, 16), (16, 33)]
    assert any(4 * p[1] > 32 and (4 * p[1]) % 32 for p in plans.values())                                 # fold: second trip, ragged
    assert any(s[1] % (256 * p[0]) == 1 for s, p in plans.items())                                        # one live lane in the last tile
    # the existing Schur tests all sit on one plan: that is the gap this table closes
    for shape in ((9, 700), (5, 80), (9, 2500), (12, 3000), (8, 900)):
        assert ba_cases.schur_plan(*shape, cam_side=False) == ba_cases.schur_plan(*shape, cam_side=True)
        pp, tiles, nch = ba_cases.schur_plan(*shape, cam_side=False)
        assert (pp, nch) == (2, 1) and tiles <= 6
    assert ba_cases.schur_plan(500, 200000, False) == (4, 196, 13) and ba_cases.schur_plan(500, 200000, True) == (4, 196, 5)
    # the solve: n = 6 ncam > 1024 splits a camera's 6 x 6 block over two trips of the 1024-thread loops
    assert 6 * 173 > 1024 > 6 * 170 and ba_cases.schur_plan(173, 600, False)[2] == 10
    assert ba_cases.schur_plan(173, 600, True)[2] == 10


# ---------------------------------------------------------------- the reference alone holds the bar
@pytest.mark.parametrize("shape", list(ba_cases.PRODUCT_SHAPES))
def test_reference_products_do_not_depend_on_summation_order(shape):
    _, (u_f, u_r), _, (w_f, w_r) = ba_cases.product_reference(*shape, reverse=None)
    assert np.abs(u_f - u_r).max() <= 1e-11 * np.abs(u_f).max()
    assert np.abs(w_f - w_r).max() <= 1e-11 * np.abs(w_f).max()


def test_sampled_subsets_hit_the_tile_and_chunk_edges():
    pts = ba_cases.sample_points(200000, 4, 196)
    assert {0, 1023, 1024, 2047, 2048, 199679, 199680, 199999} <= set(pts.tolist()) and 1900 <= len(pts) <= 2100
    pts = ba_cases.sample_points(65537, 4, 65)
    assert {0, 65535, 65536} <= set(pts.tolist())
    assert ba_cases.sample_cameras(96, 5).tolist() == [0, 18, 19, 37, 38, 56, 57, 75, 76, 95]


def _no_cancellation_in_depth(cams, X):
    """max over pairs of (|R_z . X| summed termwise + |t_z|) / |z'|, exact zeros of z' excluded."""
    R = np_ba.rotation(cams[:, :3])
    Xd = X.astype(np.float64)
    z = np.einsum("ib,jb->ij", R[:, 2], Xd) + cams[:, None, 5]
    mag = np.einsum("ib,jb->ij", np.abs(R[:, 2]), np.abs(Xd)) + np.abs(cams[:, None, 5])
    return z, float((mag / np.where(z == 0, np.inf, np.abs(z))).max())


@pytest.mark.parametrize("name", ["edge_problem", "depth_problem"])
def test_edge_problems_are_what_they_claim_and_well_posed(name):
    K, cams, X, x, v = getattr(ba_cases, name)()
    z, ratio = _no_cancellation_in_depth(cams, X)
    assert ratio <= 1e3             # no depth is a difference of much larger numbers: 1 / z' is good to 1e3 eps = 1e-13
    if name == "edge_problem":
        assert np.allclose(np.linalg.norm(cams[:8, :3], axis=1), ba_cases.EDGE_NORMS, rtol=1e-15, atol=0)
        assert z[0, 0] == 0.0 and np.count_nonzero(z == 0) == 1
        assert np.all(z[0, 1:6] <= -1) and np.all(z[1:, :] > 0)
    else:
        az = np.abs(z)
        assert az.min() <= 1e-6 and az.max() >= 1e6 and np.all(z != 0)
        assert az[0, :20].max() <= 0.1 and az[0, 20:40].min() >= 10
    ci, pi = ba_cases.full_visibility(*z.shape)
    outs = []
    for reverse in (False, True):
        u = np_ba.wt_product(cams, K, X, x, reverse=reverse)
        w = np_ba.w_product(cams, K, X, v, reverse=reverse)
        ui, wi = np_ba.indexed_products(cams, K, X, ci, pi, x, v, reverse=reverse)
        assert np.all(np.isfinite(u)) and np.all(np.isfinite(w))
        assert np.abs(ui - u).max() <= 1e-11 * np.abs(u).max() and np.abs(wi - w).max() <= 1e-11 * np.abs(w).max()
        outs.append((u, w))
    (u_f, w_f), (u_r, w_r) = outs
    assert np.abs(u_f - u_r).max() <= 1e-11 * np.abs(u_f).max() and np.abs(w_f - w_r).max() <= 1e-11 * np.abs(w_f).max()
    # row by row against the magnitude sums (the scale of the rounding when the rows differ by 25 orders of magnitude)
    su, sw = np_ba.wt_product(cams, K, X, x, magnitude=True), np_ba.w_product(cams, K, X, v, magnitude=True)
    assert np.all(np.abs(u_f - u_r).max(1) <= 1e-11 * su.max(1)) and np.all(np.abs(w_f - w_r).max(1) <= 1e-11 * sw.max(1))


@pytest.mark.parametrize("name", list(ba_cases.indexed_cases()))
def test_indexed_reference_does_not_depend_on_summation_order(name):
    K, cams, X, x, v = ba_cases.indexed_problem()
    ci, pi = ba_cases.indexed_cases()[name]
    assert len(ci) == len(pi) and (len(ci) == 0 or (0 <= ci.min() and ci.max() < 8 and 0 <= pi.min() and pi.max() < 300))
    u_f, w_f = np_ba.indexed_products(cams, K, X, ci, pi, x, v)
    u_r, w_r = np_ba.indexed_products(cams, K, X, ci, pi, x, v, reverse=True)
    assert u_f.shape == (300, 3) and w_f.shape == (8, 6)
    if len(ci) == 0:
        assert not u_f.any() and not w_f.any()
        return
    assert np.abs(u_f - u_r).max() <= 1e-11 * np.abs(u_f).max() and np.abs(w_f - w_r).max() <= 1e-11 * np.abs(w_f).max()
    if name == "repeated_verbatim":                                # counted twice
        h = len(ci) // 2
        u_h, w_h = np_ba.indexed_products(cams, K, X, ci[:h], pi[:h], x, v)
        assert np.array_equal(u_f, 2 * u_h) or np.abs(u_f - 2 * u_h).max() <= 1e-14 * np.abs(u_f).max()
        assert np.abs(w_f - 2 * w_h).max() <= 1e-14 * np.abs(w_f).max()
    if name.startswith("empties"):
        assert not w_f[5].any() and not u_f[[0, 17, 299]].any() and u_f[1].any() and w_f[4].any()


# ---------------------------------------------------------------- PCG against the direct solve: the figures
@pytest.mark.parametrize("fix_first", [True, False])
@pytest.mark.parametrize("shape", ba_cases.PCG_SHAPES)
def test_pcg_distance_from_the_direct_solve(shape, fix_first):
    """Measures max|pcg - direct| / max|direct| of the float64 NumPy recurrence (same preconditioner, tolerance and
    check-every-fifth cadence as the kernel) and pins it below the figures recorded in test_gpu_ba_schur.PCG_FIGURES, from
    which the device allowance (10 x) is derived."""
    import test_gpu_ba_schur as G
    K, cams, X, obs, W = ba_cases.pcg_problem(*shape)
    B, C, gc, gp, _, _ = np_ba.normal_blocks(cams, K, X, obs)
    dc, dp = np_ba.solve_direct(B, C, gc, gp, W, ba_cases.PCG_LAM, fix_first)
    pc, pp, it = np_ba.solve_pcg(B, C, gc, gp, W, ba_cases.PCG_LAM, fix_first, tol=ba_cases.PCG_TOL, iters=ba_cases.PCG_ITERS)
    fig_c, fig_p = np.abs(pc - dc).max() / np.abs(dc).max(), np.abs(pp - dp).max() / np.abs(dp).max()
    print(f"pcg vs direct {shape} fix_first={fix_first}: it={it} dc {fig_c:.3g} dp {fig_p:.3g}")
    assert 0 < it < ba_cases.PCG_ITERS and it % 5 == 0
    rec_c, rec_p = G.PCG_FIGURES[(shape, fix_first)]
    assert fig_c <= rec_c and fig_p <= rec_p
    assert rec_c <= 4 * fig_c and rec_p <= 4 * fig_p                     # and the record is not padded
    if fix_first:
        assert np.all(pc[0] == 0) and np.all(dc[0] == 0)
