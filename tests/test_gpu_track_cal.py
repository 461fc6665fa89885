"""The TRACKS-CAL family on the device (sfm_track_cal_sweep / _product / _step, track_cal.bundle_adjust_calibrated, sfm_undistort_points,
sfm_undistort_image, tracks.adjust_tracks(calibrate=...), tracks.densify_tracks(dist=...)) against the restatement
tests/np_track_cal.py: |got - want|.max() <= 1e-10 |want|.max(), the bar of docs/geometry.md; bytes, counts, repeated runs and the two
undistortions exactly (include/sfm_hip.h, "TRACKS-CAL"; docs/tracks.md §15)."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

import np_ba  # noqa: E402
import np_track_ba as nb  # noqa: E402
import np_track_cal as nc  # noqa: E402
import fuzz_track_ba as fz  # noqa: E402
import fuzz_track_cal as fc  # noqa: E402
import track_ba_cases as tc  # noqa: E402
import track_cal_cases as cc  # noqa: E402
from fuzz_tracks import dev  # noqa: E402

K = tc.K
INT32_MAX = 2 ** 31 - 1
CHUNK = 256                     # the camera side's chunk (include/sfm_hip.h)
THETA = np.array([880.0, 470.0, 330.0, -0.15, 0.02])
FUZZ_FLOOR = 1000               # a tenth of the cases the committed logs hold, rounded down to one figure (docs/tracks.md §15.6)


def problem(seed, ncam, npt, lengths, huber=1.0, theta=THETA, aspect=1.05):
    p = fz.make_problem(np.random.default_rng(seed), ncam, npt, lengths)
    p["huber"], p["deg"], p["theta"], p["aspect"] = huber, -1, np.asarray(theta, np.float64), aspect
    return p


@pytest.mark.gpu
@pytest.mark.parametrize("ncam", [1, 2, 3, 64, 65])
def test_sweep_and_products_at_every_camera_count_and_track_length(hip, ncam):
    """Tracks of 1, 7, 8, 9 and 17 observations (the point side's group of 8), as far as ncam cameras allow; track counts around a
    workgroup of the point side (32 tracks) at the shortest length."""
    for length in sorted({min(n, ncam) for n in (1, 7, 8, 9, 17)}):
        for T in ((1, 31, 32, 33) if length == min(1, ncam) else (37,)):
            p = problem(1000 * ncam + 10 * T + length, ncam, T, np.full(T, length))
            msg, out, want = fc.check_sweep(p)
            assert not msg, (ncam, T, length, msg)
            assert want["count"][0] == T * length and int(out["count"][0]) == T * length
            msg = fc.check_product(p, seed=T)
            assert not msg, (ncam, T, length, msg)


@pytest.mark.gpu
@pytest.mark.parametrize("degree", [CHUNK - 1, CHUNK, CHUNK + 1])
def test_one_camera_holding_every_observation_and_one_holding_none(hip, degree):
    """Camera 1 sees every point, cameras 0 and 2 see nothing: chunks just short of full, full, and one observation into the next."""
    p = problem(degree, 3, degree, np.ones(degree, np.int64))
    p["cam_idx"][:] = 1
    p["obs"] = (np_ba.project(p["truth"][p["cam_idx"]], K, p["X"][p["pt_idx"]][:, None, :])[:, 0] + 0.3).astype(np.float32)
    p["track_off"], p["cam_off"], p["cam_obs"] = nb.plan(p["cam_idx"], p["pt_idx"], 3, degree)
    msg, out, want = fc.check_sweep(p)
    assert not msg, msg
    B, E = out["JtJ_cam"].cpu().numpy(), out["E"].cpu().numpy()
    assert not B[0].any() and not B[2].any() and B[1].any() and not E[0].any() and not E[2].any() and E[1].any() and int(out["count"][0]) == degree
    msg = fc.check_product(p, seed=degree)
    assert not msg, msg


@pytest.mark.gpu
@pytest.mark.parametrize("huber", [np.inf, 1.0])
def test_sweep_edge_inputs(hip, huber):
    """No observation, NaN keypoints, a NaN point, points behind a camera, indices from {-1, ncam, npt, INT32_MAX} in cam_idx, pt_idx
    and cam_obs, CSR offsets outside 0..nobs, a camera with none; fc.device_sweep checks that nothing past a size was written."""
    for deg in (-1, 0, 1, 2, 3, 4, 5, 6, 7):
        p = fc.with_theta(fz.gen_problem(np.random.default_rng(100 + deg + 7), 1 << 11, deg=deg), np.random.default_rng(deg + 50))
        p["huber"] = huber
        msg, out, want = fc.check_sweep(p)
        assert not msg, (deg, msg)
        if deg == 0:
            assert len(p["obs"]) == 0 and not out["G"].any() and not out["JtJ_cam"].any() and out["count"].cpu().numpy().tolist() == [0, 0, 0]
        msg = fc.check_product(p, seed=deg + 1)
        assert not msg, (deg, msg)
    # the out-of-range indices, each by name, and a NaN point
    p = problem(5, 4, 40, np.full(40, 3), huber)
    for o, (ci, pi) in enumerate([(-1, None), (4, None), (INT32_MAX, None), (None, -1), (None, 40), (None, INT32_MAX)]):
        if ci is not None:
            p["cam_idx"][7 * o] = ci
        else:
            p["pt_idx"][7 * o] = pi
    p["cam_obs"][[3, 30, 60, 90]] = [-1, len(p["obs"]), INT32_MAX, 4]
    p["X"][39] = np.nan
    msg, out, want = fc.check_sweep(p)
    assert not msg, msg
    act = out["active"].cpu().numpy()
    assert not act[[0, 7, 14, 21, 28, 35]].any() and not act[p["pt_idx"] == 39].any() and int(out["count"][0]) == len(p["obs"]) - 6 - 3


@pytest.mark.gpu
def test_a_mode_1_sweep_with_a_planted_crossing_and_a_theta_that_cannot_project(hip):
    from sfm_mvs_amd import track_cal
    p = problem(61, 4, 50, np.full(50, 3))
    pl = fz.device_plan(p)
    first, msg = fc.device_sweep(pl, p, p["cams"], p["theta"], p["X"], 1.0)
    assert not msg and int(first["count"][0]) == 150
    Xb = p["X"].copy()
    o = int(np.flatnonzero(p["pt_idx"] == 4)[0])
    C = nb.centres(p["cams"])[p["cam_idx"][o]]
    Xb[4] = C + 1.5 * (C - Xb[4])                                                                      # beyond the centre of a camera that sees it
    msg, _, _ = fc.check_sweep(p, 1.0, (p["cams"], np.zeros(5), Xb))
    assert not msg, msg
    out1, _ = fc.device_sweep(pl, p, p["cams"], p["theta"], Xb, 1.0, 1, first["active"], track_cal.workspace(pl))
    crossed = int(out1["count"][1])
    assert crossed >= 1 and int(out1["count"][0]) == 150 - crossed and not track_cal.rows_of(pl, out1["ws"])[o].any()
    # a step of theta on the device that takes f below zero: every active observation crosses, nothing contributes
    out2, _ = fc.device_sweep(pl, p, p["cams"], p["theta"], p["X"], 1.0, 1, first["active"], track_cal.workspace(pl), np.array([2 * p["theta"][0], 0, 0, 0, 0]))
    assert out2["count"].cpu().numpy().tolist() == [0, 150, 0] and not out2["JtJ_cam"].any() and not out2["G"].any() and float(out2["stat"][0]) == 0.0
    out3, _ = fc.device_sweep(pl, p, p["cams"], p["theta"], p["X"], 1.0, 0, None, track_cal.workspace(pl), np.array([0, 0, 0, np.nan, 0]))
    assert out3["count"].cpu().numpy().tolist() == [0, 0, 0] and not out3["active"].any()


@pytest.mark.gpu
def test_every_free_mask_and_the_fixed_k_family_on_the_same_problem(hip):
    """All 32 masks on a 3-camera problem: dtheta is exactly 0 where the parameter is not free, the step is the restatement's.  With
    mask 0 and no distortion the blocks are track_ba.sweep's and the step's dc and dp track_ba.step's, to 1e-10 of the largest entry
    (csrc/tracks_ba.hip contracts a * b + c, csrc/tracks_cal.hip does not: the header promises a tolerance, not bits)."""
    from sfm_mvs_amd import track_ba, track_cal
    p = problem(71, 3, 60, np.full(60, 3), 1.0, nc.theta_of(K)[0], 1.0)
    pl = fz.device_plan(p)
    out, msg = fc.device_sweep(pl, p, p["cams"], p["theta"], p["X"], 1.0)
    assert not msg, msg
    old = track_ba.sweep(pl, dev(p["cams"]), K, dev(p["X"]), dev(p["obs"]), 1.0)
    for name in ("JtJ_cam", "Jtr_cam", "JtJ_pt", "Jtr_pt", "stat"):
        assert tc.rel(out[name].cpu().numpy(), old[name].cpu().numpy()) <= 1e-10, name
    assert torch.equal(out["count"], old["count"]) and torch.equal(out["active"], old["active"])
    rows, rows_old = track_cal.rows_of(pl, out["ws"]).cpu().numpy(), track_ba.rows_of(pl, old["ws"]).cpu().numpy()
    assert tc.rel(np.c_[rows[:, :12], rows[:, 22:]], rows_old) <= 1e-10
    dc0, dp0, it0, st0 = track_ba.step(pl, old, 1e-3, True, 1e-12, 200)
    dc, di, dp, it, st = track_cal.step(pl, out, 1e-3, 0, True, 1e-12, 200)
    assert st == st0 == 0 and not di.any() and tc.rel(dc.cpu().numpy(), dc0.cpu().numpy()) <= 1e-10 and tc.rel(dp.cpu().numpy(), dp0.cpu().numpy()) <= 1e-10
    q = problem(72, 3, 60, np.full(60, 3), 1.0)                                                        # and with distortion: every mask
    plq = fz.device_plan(q)
    outq, msg = fc.device_sweep(plq, q, q["cams"], q["theta"], q["X"], 1.0)
    assert not msg, msg
    blocks = fc.device_blocks(outq)
    W = nc.dense_w(track_cal.rows_of(plq, outq["ws"]).cpu().numpy(), q["cam_idx"], q["pt_idx"], 3, 60)
    for mask in range(32):
        dc, di, dp, it, st = track_cal.step(plq, outq, 1e-2, mask, True, 1e-13, 200)
        wc, wi, wp, wst = nc.step(*blocks, W, 1e-2, mask, True)
        on = np.array([(mask >> k) & 1 for k in range(5)], bool)
        di = di.cpu().numpy()
        assert st == wst == 0 and not di[~on].any() and (not on.any() or di[on].all()), (mask, di)
        assert not dc[0].any() and tc.rel(dc.cpu().numpy(), wc) <= 1e-8 and tc.rel(dp.cpu().numpy(), wp) <= 1e-8, mask
        if on.any():
            assert np.abs(di - wi).max() <= 1e-8 * np.abs(wi).max(), (mask, di, wi)


def embedded(p, seed=9):
    """p with three cameras and forty tracks appended that see only the new cameras."""
    q = problem(seed, 3, 40, np.full(40, 3), p["huber"])
    ncam, npt = len(p["cams"]), len(p["X"])
    out = dict(cams=np.vstack([p["cams"], q["cams"]]), X=np.vstack([p["X"], q["X"]]), obs=np.vstack([p["obs"], q["obs"]]),
               cam_idx=np.r_[p["cam_idx"], q["cam_idx"] + ncam].astype(np.int32), pt_idx=np.r_[p["pt_idx"], q["pt_idx"] + npt].astype(np.int32),
               huber=p["huber"], deg=-1, theta=p["theta"], aspect=p["aspect"])
    out["track_off"], out["cam_off"], out["cam_obs"] = nb.plan(out["cam_idx"], out["pt_idx"], ncam + 3, npt + 40)
    return out


@pytest.mark.gpu
def test_repeated_calls_and_an_embedded_problem_give_the_same_bits(hip):
    from sfm_mvs_amd import track_cal
    p = problem(31, 9, 700, np.random.default_rng(4).integers(2, 10, 700))
    pl = fz.device_plan(p)
    rng = np.random.default_rng(1)
    x, xi, v = dev(rng.normal(size=(9, 6))), dev(rng.normal(size=5)), dev(rng.normal(size=(700, 3)))
    names = ("JtJ_cam", "Jtr_cam", "E", "JtJ_pt", "Jtr_pt", "F", "G", "Jtr_theta", "stat", "count", "active")
    runs = []
    for _ in range(2):
        out = track_cal.sweep(pl, dev(p["cams"]), p["theta"], p["aspect"], dev(p["X"]), dev(p["obs"]), 1.0)
        runs.append([out[k].clone() for k in names] + [track_cal.rows_of(pl, out["ws"]).clone(), track_cal.product(pl, out["ws"], x, 0, xi)] +
                    list(track_cal.product(pl, out["ws"], v, 1)) + list(track_cal.step(pl, out, 1e-3)[:3]))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    Kp = nc.K_of(p["theta"], p["aspect"])
    whole = [track_cal.bundle_adjust_calibrated(dev(p["cams"]), Kp, p["theta"][3:], dev(p["X"]), dev(p["obs"]), dev(p["cam_idx"]), dev(p["pt_idx"]), huber=1.0, iters=4)
             for _ in range(2)]
    assert torch.equal(whole[0][0], whole[1][0]) and torch.equal(whole[0][1], whole[1][1]) and whole[0][4] == whole[1][4] and len(whole[0][4]) >= 3
    assert np.array_equal(whole[0][2], whole[1][2]) and np.array_equal(whole[0][3], whole[1][3]) and whole[0][5]["cg_iters"] == whole[1][5]["cg_iters"]
    big = embedded(p)
    plb = fz.device_plan(big)
    outb = track_cal.sweep(plb, dev(big["cams"]), p["theta"], p["aspect"], dev(big["X"]), dev(big["obs"]), 1.0)
    first = runs[0]
    for k, rows in enumerate((9, 9, 9, 700, 700, 700)):                                                # the per-camera and per-point blocks; G and g_i are global
        assert torch.equal(outb[names[k]][:rows], first[k]), names[k]
    assert torch.equal(track_cal.rows_of(plb, outb["ws"])[:pl.nobs], first[11]) and torch.equal(outb["active"][:pl.nobs], first[10])


@pytest.mark.gpu
@pytest.mark.parametrize("fix_first", [True, False])
@pytest.mark.parametrize("ncam", cc.PCG_CAMS)
def test_device_step_against_the_direct_solve_and_the_reference_recurrence(hip, ncam, fix_first):
    """The converged step (cg_tol = 1e-13) against np_track_cal.step fed the sweep's own blocks and the W of its rows, allowed PCG_ALLOW
    times what the reference PCG itself ends from it (track_cal_cases.PCG_FIGURES); three iterations against three of
    np_track_cal.solve_pcg to 1e-8.  6 * 169 + 5 = 1019 unknowns fit the CG kernels' 1024 lanes, 6 * 170 + 5 = 1025 take a second trip."""
    from sfm_mvs_amd import track_cal
    p = cc.with_border(tc.step_problem(ncam))
    pl = fz.device_plan(p)
    out, msg = fc.device_sweep(pl, p, p["cams"], p["theta"], p["X"], p["huber"])
    assert not msg, msg
    blocks = fc.device_blocks(out)
    W = nc.dense_w(track_cal.rows_of(pl, out["ws"]).cpu().numpy(), p["cam_idx"], p["pt_idx"], pl.ncam, pl.npt)
    dc, di, dp, it, status = track_cal.step(pl, out, cc.PCG_LAM, cc.PCG_FREE, fix_first, cc.PCG_TOL, cc.PCG_ITERS)
    wc, wi, wp, wst = nc.step(*blocks, W, cc.PCG_LAM, cc.PCG_FREE, fix_first)
    fig = (tc.rel(dc.cpu().numpy(), wc), tc.rel(di.cpu().numpy(), wi), tc.rel(dp.cpu().numpy(), wp))
    tol = tuple(cc.PCG_ALLOW * f for f in cc.PCG_FIGURES[(ncam, fix_first)])
    print(f"ncam {ncam} fix_first={fix_first}: it {it}  dc {fig[0]:.3g} di {fig[1]:.3g} dp {fig[2]:.3g} (allowed {tol[0]:.3g}, {tol[1]:.3g}, {tol[2]:.3g})")
    assert status == wst == 0 and 0 < it < cc.PCG_ITERS and it % 5 == 0
    assert bool(dc[0].any()) != fix_first and di.cpu().numpy()[[1, 2, 4]].tolist() == [0.0, 0.0, 0.0] and di[0] != 0 and di[3] != 0
    assert all(f <= t for f, t in zip(fig, tol)), (fig, tol)
    d3 = track_cal.step(pl, out, cc.PCG_LAM, cc.PCG_FREE, fix_first, 0.0, 3)
    w3 = nc.solve_pcg(*blocks, W, cc.PCG_LAM, cc.PCG_FREE, fix_first, tol=0.0, iters=3)
    assert d3[3] == 3 and all(tc.rel(d3[k].cpu().numpy(), w3[k]) <= 1e-8 for k in range(3))


@pytest.mark.gpu
def test_step_status_bits_and_iteration_control(hip):
    from sfm_mvs_amd import track_cal
    p = problem(41, 5, 60, np.full(60, 4))
    gone = p["cam_idx"] != 3                                                                            # camera 3 sees nothing
    p["obs"], p["cam_idx"], p["pt_idx"] = p["obs"][gone], p["cam_idx"][gone], p["pt_idx"][gone]
    p["X"][11] = np.nan                                                                                # point 11: every observation inactive
    p["track_off"], p["cam_off"], p["cam_obs"] = nb.plan(p["cam_idx"], p["pt_idx"], 5, 60)
    assert not fc.check_step(p, 1e-3, 9, True) and not fc.check_step(p, 1e-1, 31, False) and not fc.check_step(p, 1e-3, 0, True)
    pl = fz.device_plan(p)
    out, _ = fc.device_sweep(pl, p, p["cams"], p["theta"], p["X"], 1.0)
    dc, di, dp, it, status = track_cal.step(pl, out, 1e-3)
    assert status == 3 and not dc[3].any() and not dp[11].any() and all(bool(torch.isfinite(t).all()) for t in (dc, di, dp))
    # no observation at all: G is zero, singular on any free set (bit 2), fine when nothing is free
    e = problem(43, 2, 3, np.zeros(3, np.int64))
    ple = fz.device_plan(e)
    oute, _ = fc.device_sweep(ple, e, e["cams"], e["theta"], e["X"], 1.0)
    for mask, want in ((9, 7), (0, 3), (16, 7)):
        dc, di, dp, it, status = track_cal.step(ple, oute, 1e-3, mask)
        assert status == want and not dc.any() and not di.any() and not dp.any(), (mask, status)
    # ONE unknown (one camera, fixed; cy free): conjugate gradients solve it exactly in one iteration and the four iterations before
    # the next look are no-ops, not 0 / 0 (the fuzzer's case step:292062397)
    one = problem(44, 1, 40, np.ones(40, np.int64))
    assert not fc.check_step(one, 1e-3, 4, True)
    plo = fz.device_plan(one)
    outo, _ = fc.device_sweep(plo, one, one["cams"], one["theta"], one["X"], 1.0)
    dc, di, dp, it, status = track_cal.step(plo, outo, 1e-3, 4, True, 1e-10, 200)
    assert it == 5 and not dc.any() and di[2] != 0 and all(bool(torch.isfinite(t).all()) for t in (di, dp))
    clean = problem(42, 5, 60, np.full(60, 4))
    plc = fz.device_plan(clean)
    outc, _ = fc.device_sweep(plc, clean, clean["cams"], clean["theta"], clean["X"], 1.0)
    assert track_cal.step(plc, outc, 1e-3)[4] == 0
    for cap in (0, 1, 4, 5, 7, 200):
        for tol in (1e-3, 1e-10):
            dc, di, dp, it, _ = track_cal.step(plc, outc, 1e-3, 9, True, tol, cap)
            assert 0 <= it <= cap and (it % 5 == 0 or it == cap), (cap, tol, it)
            if cap == 0:                                                                               # y = 0 and dp = Cd^-1 g_p
                blocks = fc.device_blocks(outc)
                assert not dc.any() and not di.any() and not fz.close("dp", dp, nc._back(nc.system(*blocks, np.zeros((5, 60, 6, 3)), 1e-3, 9, True), np.zeros(35))[2])


def looks(it, cg_iters):
    """The host waits of sfm_track_cal_step: sfm_track_ba_step's formula."""
    return it // 5 + 1 if it < cg_iters else max(1, (cg_iters + 4) // 5)


@pytest.mark.gpu
def test_host_waits_of_one_attempt_and_of_a_whole_adjustment(hip):
    from sfm_mvs_amd import _lib, track_cal
    p = problem(51, 6, 200, np.full(200, 4))
    Kp, dist = nc.K_of(p["theta"], p["aspect"]), p["theta"][3:]
    args = (dev(p["cams"]), Kp, dist, dev(p["X"]), dev(p["obs"]), dev(p["cam_idx"]), dev(p["pt_idx"]))
    track_cal.bundle_adjust_calibrated(*args, huber=1.0, iters=2)                                        # warm
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()

    def counted(fn):
        lib0 = int(_lib.lib().sfm_host_sync_count())
        torch.cuda.set_sync_debug_mode("warn")
        try:
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                res = fn()
        finally:
            torch.cuda.set_sync_debug_mode(prev)
        return res, [str(w.message) for w in caught if "synchroniz" in str(w.message).lower()], int(_lib.lib().sfm_host_sync_count()) - lib0

    pl = track_cal.plan(args[5], args[6], 6, 200)
    first = track_cal.sweep(pl, args[0], p["theta"], p["aspect"], args[3], args[4], 1.0)
    spare = track_cal.workspace(pl)
    torch.cuda.synchronize()

    def attempt():
        dc, di, dp, it, status = track_cal.step(pl, first, 1e-3)
        trial = track_cal.sweep(pl, args[0] - dc, p["theta"], p["aspect"], args[3] - dp, args[4], 1.0, 1, first["active"], spare, dtheta=di)
        return it, track_cal._read(trial, di)

    (it, read), syncs, lib_syncs = counted(attempt)
    assert len(syncs) == 1, syncs                                                                      # ONE read: stat, count and the step of theta
    assert lib_syncs == looks(it, 200) and it > 0 and read[3] == 0 and read[0] < float(first["stat"][0]) and read[5][0] != 0 and read[5][1] == 0
    (_, _, _, _, hist, info), syncs, lib_syncs = counted(lambda: track_cal.bundle_adjust_calibrated(*args, huber=1.0, iters=3))
    assert len(syncs) == 1 + len(info["cg_iters"]), (syncs, info)                                      # the first sweep, then one per attempt
    assert lib_syncs == sum(looks(it, 200) for it in info["cg_iters"])
    for fn in (lambda: track_cal.undistort_points(args[4], Kp, dist), lambda: track_cal.undistort_images(torch.zeros((2, 8, 8, 3), dtype=torch.uint8, device="cuda"), Kp, dist, None, True)):
        _, syncs, lib_syncs = counted(fn)
        assert syncs == [] and lib_syncs == 0                                                          # no host wait


def device_adjust(cams, K_, dist, X, obs, ci, pi, free, huber, iters):
    from sfm_mvs_amd import track_cal
    c, Xd, Kn, dn, hist, info = track_cal.bundle_adjust_calibrated(dev(cams), K_, dist, dev(X), dev(obs), dev(ci), dev(pi), free, huber, iters)
    return c.cpu().numpy(), Xd.cpu().numpy(), Kn, dn, hist, info


@pytest.mark.gpu
@pytest.mark.parametrize("name", cc.SCENES)
def test_calibration_on_the_device(hip, name):
    """The device against the bars of tests/golden/track_cal_calibration.json (halfway between what the restatement reaches with (f,
    k1) free and with K fixed), and its figures beside the restatement's."""
    rec, s = cc.fixture()["scenes"][name], cc.scene(name)
    got = cc.run_scene(s, device_adjust, cc.FREE)
    bar = cc.bars(name, rec)
    print(f"{name} on the device: " + ", ".join(f"{k} {got[k]:.6g} (restatement {rec['calibrated'][k]:.6g}, bar {bar[k]:.6g})" for k in cc.BAR_KEYS if k in bar) +
          f"; {got['iterations']} iterations (restatement {rec['calibrated']['iterations']})")
    for k, b in bar.items():
        assert got[k] <= b, (k, got[k], b)
    assert abs(got["cost"] - rec["calibrated"]["cost"]) <= 1e-6 * rec["calibrated"]["cost"]


@pytest.mark.gpu
def test_adjust_tracks_without_calibrate_is_the_direct_call_and_with_it_closes_the_chain(hip):
    """calibrate=None returns what track_ba.bundle_adjust_tracks returns, bit for bit.  calibrate=dict(...) on the ring8 scene: P' is
    K' [R | t], info carries K and dist, and undistort_points + the fixed-K family at K' see the residual the calibrated family left."""
    from sfm_mvs_amd import track_ba, track_cal, tracks
    s = cc.scene("ring8")
    result = dict(points=s["X"], obs=s["obs"], cam_idx=s["cam_idx"], pt_idx=s["pt_idx"])
    P0 = track_ba.P_from_cams(s["cams"], s["K"])
    P1, X1, info1 = tracks.adjust_tracks(result, P0, s["K"], huber=1.0, iters=5)
    cams0 = track_ba.cams_from_P(P0, s["K"])
    c, X, hist, _ = track_ba.bundle_adjust_tracks(dev(cams0), s["K"], dev(s["X"]), dev(s["obs"]), dev(s["cam_idx"]), dev(s["pt_idx"]), huber=1.0, iters=5)
    assert np.array_equal(P1, track_ba.P_from_cams(c.cpu().numpy(), s["K"])) and np.array_equal(X1, X.cpu().numpy()) and info1["history"] == hist
    assert "K" not in info1 and "dist" not in info1
    P2, X2, info2 = tracks.adjust_tracks(result, P0, s["K"], calibrate=dict(free=("f", "k1")), iters=30)
    K2, d2 = info2["K"], info2["dist"]
    assert abs(K2[0, 0] / 900.0 - 1) < 1e-3 and K2[0, 2] == 480.0 and K2[1, 2] == 320.0 and K2[1, 1] == K2[0, 0] and d2[1] == 0.0 and abs(d2[0] + 0.12) < 0.02
    rec = cc.fixture()["scenes"]["ring8"]                                                               # plain least squares on both sides: the fixture's costs
    assert info2["history"][-1] <= 0.5 * (rec["calibrated"]["cost"] + rec["fixed"]["cost"]) and abs(info2["history"][-1] - rec["calibrated"]["cost"]) <= 1e-6 * rec["calibrated"]["cost"]
    cams2 = track_ba.cams_from_P(P2, K2)
    assert np.abs(track_ba.P_from_cams(cams2, K2) - P2).max() < 1e-8
    und = track_cal.undistort_points(dev(s["obs"]), K2, d2)
    pl = track_ba.plan(dev(s["cam_idx"]), dev(s["pt_idx"]), 8, 400)
    pin = track_ba.sweep(pl, dev(cams2), K2, dev(X2), und)
    rms_pin, rms_cal = float(np.sqrt(float(pin["stat"][0]) / len(s["obs"]))), float(np.sqrt(info2["history"][-1] / len(s["obs"])))
    print(f"ring8: rms {rms_cal:.4f} px in the distorted frames, {rms_pin:.4f} px after undistort_points at K'")
    assert int(pin["count"][0]) == len(s["obs"]) and abs(rms_pin - rms_cal) <= 0.1 * rms_cal
    with pytest.raises(tracks.SfmHipError):
        tracks.adjust_tracks(result, P0, s["K"], calibrate=dict(fre=("f",)))


@pytest.mark.gpu
def test_register_tracks_with_calibrate_on_the_device(hip):
    """register_tracks(calibrate=dict(free=("f",))) on the corrupted ring scene of §10 from a focal length 3 % off, against the same loop
    on the NumPy engine with the restatement's calibrated adjustment (tests/test_track_cal_register_cpu.py): the same registrations,
    the same K' to 1e-6, dist = 0, and rows of P that are K' [R | t].  calibrate=None from the same K: no K, no dist, the same order."""
    import register_cases as rc
    from sfm_mvs_amd import register
    from test_gpu_tracks_register import device_scene
    from test_track_cal_register_cpu import CalEngine
    case, store, nq, kps = device_scene("ring_corrupted")
    Kt = np.asarray(case["K"], np.float64)
    wrong = Kt.copy()
    wrong[0, 0] *= 1.03
    wrong[1, 1] *= 1.03
    eng = CalEngine(case)
    eng.K = wrong
    want = register.register_loop(eng, eng.n_img, case["pairs"], wrong, calibrate=dict(free=("f",)))
    got = register.register_tracks(store, nq, case["pairs"], kps, wrong, rc.FRAME, calibrate=dict(free=("f",), dist=np.zeros(2)))
    plain = register.register_tracks(store, nq, case["pairs"], kps, wrong, rc.FRAME)
    assert "K" not in plain and "dist" not in plain and plain["order"].tolist() == got["order"].tolist()
    assert got["order"].tolist() == want["order"].tolist() and got["registered"].all() and got["rounds"] == want["rounds"]
    assert len(got["ba_history"]) == len(want["ba_history"]) and np.allclose(got["ba_history"][-1], want["ba_history"][-1], rtol=1e-6)
    K2 = got["K"]
    print(f"register_tracks(calibrate) on the device: f {wrong[0, 0]:.2f} -> {K2[0, 0]:.3f} (NumPy engine {want['K'][0, 0]:.3f}, true {Kt[0, 0]:.2f}); "
          f"final cost {got['ba_history'][-1][-1]:.6g} against {plain['ba_history'][-1][-1]:.6g} with K fixed")
    assert abs(K2[0, 0] / want["K"][0, 0] - 1) <= 1e-6 and abs(K2[0, 0] / Kt[0, 0] - 1) < 0.5 * 0.03 and got["ba_history"][-1][-1] < plain["ba_history"][-1][-1]
    assert K2[0, 2] == wrong[0, 2] and K2[1, 2] == wrong[1, 2] and abs(K2[1, 1] / K2[0, 0] - wrong[1, 1] / wrong[0, 0]) < 1e-12 and got["dist"].tolist() == [0.0, 0.0]
    for i in got["order"]:
        Rt = np.linalg.solve(K2, got["P"][i])
        assert np.abs(Rt[:, :3] @ Rt[:, :3].T - np.eye(3)).max() < 1e-9 and abs(np.linalg.det(Rt[:, :3]) - 1) < 1e-9          # P is K' [R | t]


@pytest.mark.gpu
def test_adjust_tracks_calibrated_then_densify_tracks_with_dist(hip):
    """adjust_tracks(calibrate=...) -> densify_tracks(dist=...) on a rendered 3-view scene of 7 x 7 pixels, the smallest frame run_mvs
    takes at radius 3: k1 comes back from keypoints pushed through the lens, the frames reach run_mvs undistorted (the same call on
    frames undistorted by hand gives the same depth maps and points), and with dist = (0, 0) they reach it as they are."""
    import mvs_plan_cases as mc
    from mvs_scenes import render_scene
    from sfm_mvs_amd import track_ba, track_cal, tracks
    frames, Kf, P0, gt = render_scene(n=3, w=7, h=7, tex=64)
    X, ci, pi = mc.synth_tracks(Kf, P0, gt, step=1, tol=0.05)
    assert len(X) >= 30 and len(ci) >= 60
    cams = track_ba.cams_from_P(P0, Kf)
    theta = np.array([Kf[0, 0], Kf[0, 2], Kf[1, 2], -0.1, 0.0])
    obs = nc.project(cams[ci], theta, 1.0, X[pi]).astype(np.float32)                                    # what the lens shows: no noise
    result = dict(points=X, obs=obs, cam_idx=ci, pt_idx=pi)
    P1, X1, info = tracks.adjust_tracks(result, P0, Kf, calibrate=dict(free=("k1",)), iters=30)
    print(f"7 x 7 chain: k1 {info['dist'][0]:.5f} (planted -0.1), cost {info['history'][0]:.4g} -> {info['history'][-1]:.3g}")
    assert abs(info["dist"][0] + 0.1) < 0.01 and info["dist"][1] == 0.0 and np.array_equal(info["K"], Kf) and info["history"][-1] < 1e-2 * info["history"][0]
    kw = dict(nsrc=2, ndepth=16)
    with_dist = tracks.densify_tracks(result, frames, info["K"], P1, X1, dist=info["dist"], **kw)
    by_hand = [f.cpu().numpy() for f in track_cal.undistort_images(dev(np.stack(frames)), info["K"], info["dist"])]
    assert by_hand[0].shape == (7, 7, 3) and not np.array_equal(by_hand[0], frames[0])
    plain = tracks.densify_tracks(result, by_hand, info["K"], P1, X1, **kw)
    zero = tracks.densify_tracks(result, frames, info["K"], P1, X1, dist=(0.0, 0.0), **kw)
    asis = tracks.densify_tracks(result, frames, info["K"], P1, X1, **kw)
    assert any(with_dist["plan"]["neighbours"]) and with_dist["plan"]["neighbours"] == plain["plan"]["neighbours"]
    for a, b in ((with_dist, plain), (zero, asis)):
        assert len(a["depths"]) == 3 and all(torch.equal(x, y) for x, y in zip(a["depths"], b["depths"]))
        assert np.array_equal(a["points"], b["points"]) and np.array_equal(a["colors"], b["colors"])


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 300])
def test_undistort_points_matches_the_restatement_bit_for_bit(hip, n):
    rng = np.random.default_rng(n)
    px = rng.uniform(-20, 980, (n, 2)).astype(np.float32)
    if n >= 63:
        px[5], px[17, 1], px[40, 0] = [np.nan, 100], np.inf, -np.inf                                # NaN keypoints
        px[6] = [THETA[1], THETA[2]]                                                                  # the centre of distortion: rd = 0
    for theta, a, Ko in ((THETA, 1.05, None), (np.array([900.0, 480, 320, 0.3, -0.05]), 1.0, np.array([[700.0, 0, 400], [0, 650.0, 300], [0, 0, 1]])),
                         (np.array([900.0, 480, 320, 0.0, 0.0]), 1.0, None)):
        msg = fc.check_points(px, theta, a, nc.K_of(theta, a) if Ko is None else Ko)
        assert not msg, (n, theta, msg)
    if n >= 63:
        from sfm_mvs_amd import track_cal
        out = track_cal.undistort_points(dev(px), nc.K_of(THETA, 1.05), THETA[3:]).cpu().numpy()
        assert np.isnan(out[[5, 17, 40]]).all() and np.isfinite(np.delete(out, [5, 17, 40], 0)).all() and out[6].tolist() == [THETA[1], THETA[2]]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1, 1), (1, 65), (65, 1), (64, 64), (65, 63)])
@pytest.mark.parametrize("C", [1, 3])
def test_undistort_image_matches_the_restatement_bit_for_bit(hip, shape, C):
    from sfm_mvs_amd import track_cal
    H, W = shape
    rng = np.random.default_rng(100 * H + W + C)
    img = rng.integers(0, 256, (3, H, W, C), dtype=np.uint8)
    Kf = np.array([[0.8 * max(H, W), 0, (W - 1) / 2.0], [0, 0.8 * max(H, W), (H - 1) / 2.0], [0, 0, 1]])
    theta0, a = nc.theta_of(Kf)
    for mask in (True, False):                                                                        # the identity: byte for byte, everything valid
        assert not fc.check_image(img, theta0, a, Kf, mask)
    got, m = track_cal.undistort_images(dev(img), Kf, None, None, True)
    assert np.array_equal(got.cpu().numpy(), img) and bool(m.all())
    for k1, k2 in ((-0.25, 0.04), (0.3, 0.0)):
        theta = np.r_[theta0[:3], k1, k2]
        assert not fc.check_image(img, theta, a, Kf, True), (k1, k2)
        Ko = Kf.copy()
        Ko[0, 0], Ko[1, 1], Ko[0, 2] = 1.3 * Kf[0, 0], 1.1 * Kf[1, 1], Kf[0, 2] + 0.37                # another pinhole camera
        assert not fc.check_image(img, theta, 1.07, Ko, False), (k1, k2)
    # a source tap exactly on the border: whole-pixel and half-pixel shifts through K_out
    for shift in (1.0, -1.0, 0.5, -0.5):
        Ko = Kf.copy()
        Ko[0, 2] += shift
        Ko[1, 2] -= shift
        assert not fc.check_image(img, theta0, a, Ko, True), shift
    single, m1 = track_cal.undistort_images(dev(img[0]), Kf, (-0.25, 0.04), None, True)               # [H, W, C] without the batch axis
    want, wm = nc.undistort_image(img[0], np.r_[theta0[:3], -0.25, 0.04], a, Kf)
    assert np.array_equal(single.cpu().numpy(), want) and np.array_equal(m1.cpu().numpy(), wm)


@pytest.mark.gpu
def test_a_short_fixed_seed_fuzz_run_finds_no_mismatch(hip):
    counts, bad, dt = fc.run(12.0, 5555)
    print(f"fuzz_track_cal: seed 5555, {sum(counts.values())} cases {counts}, {bad} mismatches, {dt:.0f} s")
    assert bad == 0 and all(c > 0 for c in counts.values()), counts


@pytest.mark.gpu
def test_committed_fuzz_logs_are_clean_and_name_this_code(hip):
    """profiles/track_cal_fuzz_seed*.log: no mismatch, and run on the code of csrc/tracks_cal.hip and csrc/common.h that the loaded
    library was built from (scripts/knn_code_hash.py: comments and whitespace do not count)."""
    import glob
    import re
    from sfm_mvs_amd import _lib
    have = _lib.code_hashes_of_binary()
    logs = sorted(glob.glob(os.path.join(ROOT, "profiles", "track_cal_fuzz_seed*.log")))
    assert len(logs) >= 2, logs
    total = 0
    for path in logs:
        text = open(path).read()
        m = re.search(r"fuzz_track_cal: seed \d+, (\d+) cases .*?, (\d+) mismatches", text)
        assert m and int(m.group(2)) == 0, f"{path}: no clean summary line"
        ids = re.findall(r"sfm_build_id (knn\.hip:\S+(?: \S+:\S+)*)", text)
        assert ids, f"{path} does not name the build it ran on"
        logged = dict(tok.split(":", 1) for tok in ids[-1].split() if ":" in tok)
        for name in ("tracks_cal.hip", "common.h"):
            assert logged.get(name) == have[name], f"{path} was produced by another csrc/{name} than the loaded binary's"
        total += int(m.group(1))
    assert total >= FUZZ_FLOOR, total
