"""The Schur bundle-adjustment kernels (csrc/ba_schur.hip) on every launch path, against the float64 complex-step
reference of np_ba.py at the project's bar for these sums: |got - want|.max() <= 1e-10 |want|.max().

test_np_ba_cpu.py shows that on these very inputs the reference alone is good to 1e-11 (two summation orders), pins the
launch plan every shape below is claimed to land on (ba_cases.PRODUCT_SHAPES: PP = 2 and 4, one to six camera chunks,
even and uneven, differing chunk counts for the two products, 4 to 784 fold rows) and measures the PCG figures."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import ba_cases
import np_ba

pytestmark = pytest.mark.gpu

BAR = 1e-10

# max|pcg - direct| / max|direct| (dc, dp) of the float64 NumPy PCG (np_ba.solve_pcg: the kernel's recurrence, cg_tol =
# 1e-13, convergence looked at every fifth iteration) against np_ba.solve_direct, lam = 1e-2, measured on the CPU by
# test_np_ba_cpu.py::test_pcg_distance_from_the_direct_solve (20 to 25 iterations).  The device sums in another order and
# contracts to FMAs: it is allowed PCG_ALLOW times these figures.
PCG_FIGURES = {
    ((173, 600), True): (1.5e-15, 2.8e-15),
    ((173, 600), False): (1.3e-13, 2.4e-13),
    ((40, 1500), True): (1.4e-14, 1.1e-14),
    ((40, 1500), False): (3.5e-15, 5.1e-15),
}
PCG_ALLOW = 10.0


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def rel(got, want):
    """max|got - want| / max|want|"""
    return float(np.abs(np.asarray(got) - want).max() / np.abs(want).max())


def products(hip, K, cams, X, x, v, idx=()):
    idx = tuple(cu(i) for i in idx)
    return hip.ba_schur_wt(cu(cams), K, cu(X), cu(x), *idx), hip.ba_schur_w(cu(cams), K, cu(X), cu(v), *idx)


# ---------------------------------------------------------------- products on every launch plan
@pytest.mark.parametrize("shape", list(ba_cases.PRODUCT_SHAPES))
def test_products_match_the_reference_on_every_launch_plan(hip, shape):
    K, cams, X, x, v = ba_cases.product_problem(*shape)
    pt_sel, want_u, cam_sel, want_w = ba_cases.product_reference(*shape)
    u, w = products(hip, K, cams, X, x, v)
    un, wn = u.cpu().numpy(), w.cpu().numpy()
    assert un.shape == (shape[1], 3) and wn.shape == (shape[0], 6)
    eu = rel(un if pt_sel is None else un[pt_sel], want_u)
    ew = rel(wn if cam_sel is None else wn[cam_sel], want_w)
    print(f"{shape}: W^T x {eu:.3g}  W v {ew:.3g}")
    assert eu <= BAR and ew <= BAR
    # adjointness  <v, W^T x> = <x, W v>  to rounding
    assert float((un * v).sum()) == pytest.approx(float((wn * x).sum()), rel=1e-11)
    # fixed-order reductions: a second call gives the same bits
    u2, w2 = products(hip, K, cams, X, x, v)
    assert torch.equal(u, u2) and torch.equal(w, w2)
    # X as a view of homogeneous points: ldx = 4
    X4 = torch.cat([cu(X), torch.full((shape[1], 1), 7.0, dtype=torch.float32, device="cuda")], 1)
    assert X4[:, :3].stride(0) == 4
    assert torch.equal(u, hip.ba_schur_wt(cu(cams), K, X4[:, :3], cu(x))) and torch.equal(w, hip.ba_schur_w(cu(cams), K, X4[:, :3], cu(v)))


# ---------------------------------------------------------------- camera-table and depth edges
def _rows(got, want, scale):
    """max over rows of |got - want|.max(row) / scale.max(row)"""
    return float((np.abs(got - want).max(1) / scale.max(1)).max())


@pytest.mark.parametrize("name", ["edge_problem", "depth_problem"])
def test_camera_and_depth_edges(hip, name):
    """edge_problem: rotation-vector norms 0, 1e-20, 1e-12, 1e-8, 1e-4, pi - 1e-6, pi, 4; one point with z' = 0 exactly at
    the identity camera (the z := 1 convention); points behind a camera.  depth_problem: depths 1e-6 .. 1e6.  Dense and
    indexed (full visibility) products against the reference and against each other, at the bar — overall and, because
    the rows span 25 orders of magnitude, row by row against the row's sum of magnitudes sum |Jp|^T |Jc| |x|."""
    K, cams, X, x, v = getattr(ba_cases, name)()
    want_u, want_w = np_ba.wt_product(cams, K, X, x), np_ba.w_product(cams, K, X, v)
    scale_u, scale_w = np_ba.wt_product(cams, K, X, x, magnitude=True), np_ba.w_product(cams, K, X, v, magnitude=True)
    dense = [t.cpu().numpy() for t in products(hip, K, cams, X, x, v)]
    index = [t.cpu().numpy() for t in products(hip, K, cams, X, x, v, ba_cases.full_visibility(*cams.shape[:1], len(X)))]
    figs = {}
    for what, (gu, gw) in (("dense", dense), ("indexed", index)):
        assert np.all(np.isfinite(gu)) and np.all(np.isfinite(gw)), what
        figs[what] = (rel(gu, want_u), rel(gw, want_w), _rows(gu, want_u, scale_u), _rows(gw, want_w, scale_w))
    figs["dense-indexed"] = (rel(dense[0], index[0]), rel(dense[1], index[1]), _rows(dense[0], index[0], scale_u), _rows(dense[1], index[1], scale_w))
    print(name, {k: tuple(f"{f:.2g}" for f in v) for k, v in figs.items()})
    for what, f in figs.items():
        assert max(f) <= BAR, (what, f)


def test_reciprocal_at_the_ulp_level(hip):
    """pair_jacobians_structured takes 1 / z from the hardware estimate and two Newton steps.  One camera, the identity
    at the origin, and x = e_4 (a unit shift along the camera's x axis) make u_j[0] = (fx / Z_j)^2 with nothing else in the
    way: r = rcp(Z) refined, fxz = fx r, Pu[0] = fxz (1 - x 0) = fxz, tu = fxz, u = fma(fxz, fxz, 0).  Two Newton steps
    leave r within one ulp (2^-52 relative) of 1 / Z; fx r and the square add 2^-53 each: 2 (2^-52 + 2^-53) + 2^-53 =
    3.5 * 2^-52, so 4 * 2^-52 = 8.9e-16 is allowed, against exact rational arithmetic, over depths 1e-6 .. 1e6.  (A hardware
    estimate good to 2^-23 and ONE step would leave 2^-46 = 1.4e-14 in r.)"""
    K, _, _, _, _ = ba_cases.product_problem(1, 1)
    rng = np.random.default_rng(5)
    Z = np.exp(rng.uniform(np.log(1e-6), np.log(1e6), 2048)).astype(np.float32)
    X = np.stack([Z * rng.uniform(-0.5, 0.5, 2048).astype(np.float32), Z * rng.uniform(-0.5, 0.5, 2048).astype(np.float32), Z], 1)
    x = np.array([[0, 0, 0, 1.0, 0, 0]])
    u = hip.ba_schur_wt(cu(np.zeros((1, 6))), K, cu(X), cu(x)).cpu().numpy()
    fx = Fraction(float(K[0, 0]))
    worst = max(abs(Fraction(float(g)) / (fx / Fraction(float(z))) ** 2 - 1) for g, z in zip(u[:, 0], Z))
    print(f"reciprocal: worst relative error of (fx / Z)^2: {float(worst):.3g}")
    assert worst <= 4 * Fraction(1, 2 ** 52)
    assert not u[:, 1].any()                                   # Pu[1] = fxz (0 - x 0), Pv[1] tv = fyz * 0


# ---------------------------------------------------------------- indexed products
@pytest.mark.parametrize("name", list(ba_cases.indexed_cases()))
def test_indexed_products(hip, name):
    """nobs = 0 (exact zeros), 1, 255, 256, 257; 2000 observations of one pair (worst-case contention of the atomics);
    a list repeated verbatim (counted twice); a camera and three points without any observation (rows exactly 0)."""
    K, cams, X, x, v = ba_cases.indexed_problem()
    ci, pi = ba_cases.indexed_cases()[name]
    want_u, want_w = np_ba.indexed_products(cams, K, X, ci, pi, x, v)
    u, w = (t.cpu().numpy() for t in products(hip, K, cams, X, x, v, (ci, pi)))
    assert u.shape == (300, 3) and w.shape == (8, 6) and u.dtype == np.float64 and w.dtype == np.float64
    if len(ci) == 0:
        assert not u.any() and not w.any()
        return
    print(f"{name}: W^T x {rel(u, want_u):.3g}  W v {rel(w, want_w):.3g}")
    assert rel(u, want_u) <= BAR and rel(w, want_w) <= BAR
    seen_c, seen_p = np.zeros(8, bool), np.zeros(300, bool)
    seen_c[ci], seen_p[pi] = True, True
    assert not w[~seen_c].any() and not u[~seen_p].any()                     # untouched rows: exactly zero
    assert np.all(np.abs(w[seen_c]).max(1) > 0) and np.all(np.abs(u[seen_p]).max(1) > 0)
    if name == "empties_shuffled":                                          # the atomics are order-dependent in the last bits only
        cs, ps = ba_cases.indexed_cases()["empties_sorted"]
        us, ws = (t.cpu().numpy() for t in products(hip, K, cams, X, x, v, (cs, ps)))
        assert rel(u, us) <= BAR and rel(w, ws) <= BAR
        assert not seen_c[5] and not seen_p[[0, 17, 299]].any()


# ---------------------------------------------------------------- the device PCG
def _sweep(hip, shape):
    K, cams, X, obs, W = ba_cases.pcg_problem(*shape)
    return K, cams, X, W, hip.ba_dense_sweep(cu(cams), K, cu(X), cu(obs))


def _host_blocks(blocks, ncam, npt):
    return (blocks["JtJ_cam"].cpu().numpy().reshape(ncam, 6, 6), blocks["JtJ_pt"].cpu().numpy().reshape(npt, 3, 3),
            blocks["Jtr_cam"].cpu().numpy().reshape(ncam, 6), blocks["Jtr_pt"].cpu().numpy().reshape(npt, 3))


@pytest.mark.parametrize("fix_first", [True, False])
@pytest.mark.parametrize("shape", ba_cases.PCG_SHAPES)
def test_device_pcg_step_against_the_direct_solve(hip, shape, fix_first):
    """The step of sfm_ba_schur_solve (cg_tol = 1e-13) against np_ba.solve_direct fed the sweep's own B, C, g and the
    reference W.  (173, 600): n = 1038 > 1024 unknowns — both CG kernels take a second trip through their element loops and
    camera 170's 6 x 6 block is split between the trips — and ten camera chunks; (40, 1500): one trip, two chunks."""
    ncam, npt = shape
    K, cams, X, W, blocks = _sweep(hip, shape)
    dc, dp, it, status = hip.ba_schur_solve(cu(cams), K, cu(X), blocks, ba_cases.PCG_LAM, fix_first_camera=fix_first,
                                            cg_tol=ba_cases.PCG_TOL, cg_iters=ba_cases.PCG_ITERS)
    want_c, want_p = np_ba.solve_direct(*_host_blocks(blocks, ncam, npt), W, ba_cases.PCG_LAM, fix_first)
    fig_c, fig_p = rel(dc.cpu().numpy(), want_c), rel(dp.cpu().numpy(), want_p)
    tol_c, tol_p = (PCG_ALLOW * f for f in PCG_FIGURES[(shape, fix_first)])
    print(f"{shape} fix_first={fix_first}: it {it}  dc {fig_c:.3g} (allowed {tol_c:.3g})  dp {fig_p:.3g} (allowed {tol_p:.3g})")
    assert status == 0 and 0 < it < ba_cases.PCG_ITERS and it % 5 == 0
    if fix_first:
        assert not dc[0].any()                                              # exactly zero
    else:
        assert dc[0].any()
    assert fig_c <= tol_c and fig_p <= tol_p


def test_device_pcg_equals_the_host_driven_recurrence_beyond_1024_unknowns(hip):
    from sfm_mvs_amd import ba
    K, cams, X, W, blocks = _sweep(hip, (173, 600))
    d1 = ba.schur_step(cu(cams), K, cu(X), blocks, ba_cases.PCG_LAM, device_pcg=True)
    d2 = ba.schur_step(cu(cams), K, cu(X), blocks, ba_cases.PCG_LAM, device_pcg=False)
    assert d1[2] == d2[2] and d1[2] > 0
    for a, b in zip(d1[:2], d2[:2]):
        assert float((a - b).abs().max()) <= 1e-8 * float(b.abs().max())
    assert torch.equal(d1[0], ba.schur_step(cu(cams), K, cu(X), blocks, ba_cases.PCG_LAM)[0])


def test_iteration_control(hip):
    """The count is a multiple of 5 (convergence is looked at every fifth iteration) or the cap; cg_iters = 0 returns
    dc = 0 and dp = Cd^-1 g_p; a cap of 3 with cg_tol = 0 runs exactly 3."""
    ncam, npt = shape = (40, 1500)
    K, cams, X, W, blocks = _sweep(hip, shape)
    lam = ba_cases.PCG_LAM
    for cap in (1, 4, 5, 7, 200):
        for tol in (1e-3, 1e-10):
            it = hip.ba_schur_solve(cu(cams), K, cu(X), blocks, lam, cg_tol=tol, cg_iters=cap)[2]
            assert 0 < it <= cap and (it % 5 == 0 or it == cap), (cap, tol, it)
    loose, tight = (hip.ba_schur_solve(cu(cams), K, cu(X), blocks, lam, cg_tol=t)[2] for t in (1e-3, 1e-13))
    assert 5 <= loose < tight < 200
    dc, dp, it, status = hip.ba_schur_solve(cu(cams), K, cu(X), blocks, lam, cg_iters=0)
    B, C, gc, gp = _host_blocks(blocks, ncam, npt)
    d = np.arange(3)
    C[:, d, d] *= 1 + lam
    want = np.linalg.solve(C, gp[:, :, None])[:, :, 0]
    assert it == 0 and status == 0 and not dc.any()
    assert rel(dp.cpu().numpy(), want) <= BAR
    dc3, _, it, _ = hip.ba_schur_solve(cu(cams), K, cu(X), blocks, lam, cg_tol=0.0, cg_iters=3)
    assert it == 3 and dc3.any() and bool(torch.isfinite(dc3).all())
    want3 = np_ba.solve_pcg(*_host_blocks(blocks, ncam, npt), W, lam, True, tol=0.0, iters=3)[0]
    assert rel(dc3.cpu().numpy(), want3) <= 1e-8                         # three iterations of the same recurrence


def test_singular_point_block_sets_status_bit_1(hip):
    ncam, npt = shape = (40, 1500)
    K, cams, X, W, blocks = _sweep(hip, shape)
    dead = {k: t.clone() for k, t in blocks.items()}
    dead["JtJ_pt"][77] = 0
    dc, dp, it, status = hip.ba_schur_solve(cu(cams), K, cu(X), dead, 0.0, cg_iters=5)
    assert status & 2 and not status & 1
    keep = torch.ones(npt, dtype=torch.bool, device="cuda")
    keep[77] = False
    assert bool(torch.isfinite(dp[keep]).all()) and bool(dp[keep].any())
    assert hip.ba_schur_solve(cu(cams), K, cu(X), blocks, 0.0, cg_iters=5)[3] == 0


def test_workspace_reuse_after_larger_calls(hip):
    """The products and the solve share one grow-only scratch buffer whose partial rows are laid out by (chunks, tiles):
    a small call after larger ones, with other chunk counts, must not read anything they left behind."""
    small, large = (33, 513), (96, 200000)
    K, cams, X, x, v = ba_cases.product_problem(*small)
    first = products(hip, K, cams, X, x, v)
    Kl, cl, Xl, xl, vl = ba_cases.product_problem(*large)
    products(hip, Kl, cl, Xl, xl, vl)
    Kp, cp, Xp, _, blocks = _sweep(hip, (173, 600))
    hip.ba_schur_solve(cu(cp), Kp, cu(Xp), blocks, ba_cases.PCG_LAM)
    again = products(hip, K, cams, X, x, v)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    assert rel(again[0].cpu().numpy(), ba_cases.product_reference(*small)[1]) <= BAR
