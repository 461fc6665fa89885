"""The TRACKS-BA family on the device (sfm_track_ba_sweep / _product / _step, track_ba.bundle_adjust_tracks, tracks.adjust_tracks)
against the restatement tests/np_track_ba.py: |got - want|.max() <= 1e-10 |want|.max(), the bar of docs/geometry.md; bytes, counts and
repeated runs exactly (include/sfm_hip.h, "TRACKS-BA"; docs/tracks.md §9)."""
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
import fuzz_track_ba as fz  # noqa: E402
import track_ba_cases as tc  # noqa: E402
from fuzz_tracks import dev  # noqa: E402
from test_track_ba_cpu import BA_BAR, calibration_figures, crossing_problem, ring_problem  # noqa: E402

K = tc.K
INT32_MAX = 2 ** 31 - 1
CHUNK = 256                     # the camera side's chunk (include/sfm_hip.h)
FUZZ_FLOOR = 2000               # a tenth of the cases the committed logs hold, rounded down to one figure (docs/tracks.md §9.5)


def problem(seed, ncam, npt, lengths, huber=1.0):
    p = fz.make_problem(np.random.default_rng(seed), ncam, npt, lengths)
    p["huber"], p["deg"] = huber, -1
    return p


@pytest.mark.gpu
@pytest.mark.parametrize("ncam", [1, 2, 3, 64, 65])
def test_sweep_and_products_at_every_camera_and_track_count(hip, ncam):
    """Track counts around a workgroup of the point side (256 lanes = 32 tracks of 8) and of its grid; lengths 2, 3 and ncam."""
    for T in (1, 2, 255, 256, 257):
        for length in sorted({min(2, ncam), min(3, ncam), ncam}):
            p = problem(1000 * ncam + 10 * T + length, ncam, T, np.full(T, length))
            msg, out, want = fz.check_sweep(p)
            assert not msg, (ncam, T, length, msg)
            assert want["count"][0] == T * length and int(out["count"][0]) == T * length
            msg = fz.check_product(p, seed=T)
            assert not msg, (ncam, T, length, msg)


@pytest.mark.gpu
@pytest.mark.parametrize("degree", [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1])
def test_one_camera_holding_every_observation_and_one_holding_none(hip, degree):
    """Camera 1 sees every point, cameras 0 and 2 see nothing: chunks just short of full, full, and one observation into the next."""
    p = problem(degree, 3, degree, np.ones(degree, np.int64))
    p["cam_idx"][:] = 1
    p["obs"] = (np_ba.project(p["truth"][p["cam_idx"]], K, p["X"][p["pt_idx"]][:, None, :])[:, 0] + 0.3).astype(np.float32)
    p["track_off"], p["cam_off"], p["cam_obs"] = nb.plan(p["cam_idx"], p["pt_idx"], 3, degree)
    msg, out, want = fz.check_sweep(p)
    assert not msg, msg
    B = out["JtJ_cam"].cpu().numpy()
    assert not B[0].any() and not B[2].any() and B[1].any() and not out["Jtr_cam"][0].any() and int(out["count"][0]) == degree
    msg = fz.check_product(p, seed=degree)
    assert not msg, msg


@pytest.mark.gpu
@pytest.mark.parametrize("huber", [np.inf, 1.0, 1e-3])
def test_sweep_options_and_edge_inputs(hip, huber):
    """NaN keypoints, a NaN point, points behind a camera, indices from {-1, ncam, npt, INT32_MAX} in cam_idx, pt_idx and cam_obs,
    CSR offsets outside 0..nobs, a camera with none; fz.device_sweep checks that nothing past a size was written."""
    for deg in (-1, 1, 2, 3, 4, 5, 6, 7):
        for seed in (1, 2):
            p = fz.gen_problem(np.random.default_rng(100 * seed + deg + 7), 1 << 11, deg=deg)
            p["huber"] = huber
            msg, out, want = fz.check_sweep(p)
            assert not msg, (deg, seed, msg)
            if huber == 1e-3:
                assert want["count"][2] == want["count"][0]                                             # every observation an outlier
            if huber == np.inf:
                assert want["count"][2] == 0 and abs(float(out["stat"][0]) - float(out["stat"][1])) <= 1e-12 * float(out["stat"][1])
            msg = fz.check_product(p, seed=seed)
            assert not msg, (deg, seed, msg)
    # the out-of-range indices, each by name
    p = problem(5, 4, 40, np.full(40, 3), huber)
    for o, (ci, pi) in enumerate([(-1, None), (4, None), (INT32_MAX, None), (None, -1), (None, 40), (None, INT32_MAX)]):
        if ci is not None:
            p["cam_idx"][7 * o] = ci
        else:
            p["pt_idx"][7 * o] = pi
    p["cam_obs"][[3, 30, 60, 90]] = [-1, len(p["obs"]), INT32_MAX, 4]
    msg, out, want = fz.check_sweep(p)
    assert not msg, msg
    assert not out["active"].cpu().numpy()[[0, 7, 14, 21, 28, 35]].any() and int(out["count"][0]) == len(p["obs"]) - 6


@pytest.mark.gpu
def test_at_huber_inf_the_blocks_are_those_of_project_residual(hip):
    """The new kernels against the old ones on the same input: float32-representable points, 1e-10 of the largest entry."""
    p = problem(77, 8, 300, np.random.default_rng(3).integers(2, 9, 300), np.inf)
    p["X"] = p["X"].astype(np.float32).astype(np.float64)
    pl = fz.device_plan(p)
    out, msg = fz.device_sweep(pl, p, p["cams"], p["X"], None)
    assert not msg, msg
    old = hip.project_residual(dev(p["cams"]), K, dev(p["X"].astype(np.float32)), dev(p["obs"]), dev(p["cam_idx"]), dev(p["pt_idx"]), want_proj=False,
                               want_jac=True, want_pt_jac=True, want_res2=True)
    for name in ("JtJ_cam", "Jtr_cam", "JtJ_pt", "Jtr_pt"):
        assert tc.rel(out[name].cpu().numpy(), old[name].cpu().numpy().reshape(out[name].shape)) <= 1e-10, name
    assert abs(float(out["stat"][0]) - float(old["res2"])) <= 1e-10 * float(old["res2"])


def embedded(p, seed=9):
    """p with three cameras and forty tracks appended that see only the new cameras."""
    q = problem(seed, 3, 40, np.full(40, 3), p["huber"])
    ncam, npt = len(p["cams"]), len(p["X"])
    out = dict(cams=np.vstack([p["cams"], q["cams"]]), X=np.vstack([p["X"], q["X"]]), obs=np.vstack([p["obs"], q["obs"]]),
               cam_idx=np.r_[p["cam_idx"], q["cam_idx"] + ncam].astype(np.int32), pt_idx=np.r_[p["pt_idx"], q["pt_idx"] + npt].astype(np.int32),
               huber=p["huber"], deg=-1)
    out["track_off"], out["cam_off"], out["cam_obs"] = nb.plan(out["cam_idx"], out["pt_idx"], ncam + 3, npt + 40)
    return out


@pytest.mark.gpu
def test_repeated_calls_and_an_embedded_problem_give_the_same_bits(hip):
    from sfm_mvs_amd import track_ba
    p = problem(31, 9, 700, np.random.default_rng(4).integers(2, 10, 700))
    pl = fz.device_plan(p)
    x, v = dev(np.random.default_rng(1).normal(size=(9, 6))), dev(np.random.default_rng(2).normal(size=(700, 3)))
    runs = []
    for _ in range(2):
        out = track_ba.sweep(pl, dev(p["cams"]), K, dev(p["X"]), dev(p["obs"]), 1.0)
        runs.append([out[k].clone() for k in ("JtJ_cam", "Jtr_cam", "JtJ_pt", "Jtr_pt", "stat", "count", "active")] + [track_ba.rows_of(pl, out["ws"]).clone()] +
                    [track_ba.product(pl, out["ws"], x, 0), track_ba.product(pl, out["ws"], v, 1)] + list(track_ba.step(pl, out, 1e-3)[:2]))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    whole = [track_ba.bundle_adjust_tracks(dev(p["cams"]), K, dev(p["X"]), dev(p["obs"]), dev(p["cam_idx"]), dev(p["pt_idx"]), huber=1.0, iters=4)
             for _ in range(2)]
    assert torch.equal(whole[0][0], whole[1][0]) and torch.equal(whole[0][1], whole[1][1]) and whole[0][2] == whole[1][2] and len(whole[0][2]) >= 3
    assert whole[0][3]["cg_iters"] == whole[1][3]["cg_iters"]
    big = embedded(p)
    plb = fz.device_plan(big)
    outb = track_ba.sweep(plb, dev(big["cams"]), K, dev(big["X"]), dev(big["obs"]), 1.0)
    first = runs[0]
    for k, (name, rows) in enumerate((("JtJ_cam", 9), ("Jtr_cam", 9), ("JtJ_pt", 700), ("Jtr_pt", 700))):
        assert torch.equal(outb[name][:rows], first[k]), name
    assert torch.equal(track_ba.rows_of(plb, outb["ws"])[:pl.nobs], first[7]) and torch.equal(outb["active"][:pl.nobs], first[6])


@pytest.mark.gpu
@pytest.mark.parametrize("fix_first", [True, False])
@pytest.mark.parametrize("ncam", tc.PCG_CAMS)
def test_device_step_against_the_direct_solve_and_the_reference_recurrence(hip, ncam, fix_first):
    """The converged step (cg_tol = 1e-13) against np_ba.solve_direct fed the sweep's own blocks and the W of its rows, allowed
    PCG_ALLOW times what the reference PCG itself ends from it (track_ba_cases.PCG_FIGURES); three iterations against three of
    np_ba.solve_pcg to 1e-8.  6 * 170 = 1020 unknowns fit the CG kernels' 1024 lanes, 6 * 171 = 1026 take a second trip."""
    from sfm_mvs_amd import track_ba
    p = tc.step_problem(ncam)
    pl = fz.device_plan(p)
    out, msg = fz.device_sweep(pl, p, p["cams"], p["X"], p["huber"])
    assert not msg, msg
    B, C = out["JtJ_cam"].cpu().numpy().reshape(-1, 6, 6), out["JtJ_pt"].cpu().numpy().reshape(-1, 3, 3)
    gc, gp = out["Jtr_cam"].cpu().numpy(), out["Jtr_pt"].cpu().numpy()
    W = nb.dense_w(track_ba.rows_of(pl, out["ws"]).cpu().numpy(), p["cam_idx"], p["pt_idx"], pl.ncam, pl.npt)
    dc, dp, it, status = track_ba.step(pl, out, tc.PCG_LAM, fix_first, tc.PCG_TOL, tc.PCG_ITERS)
    want_c, want_p = np_ba.solve_direct(B, C, gc, gp, W, tc.PCG_LAM, fix_first)
    fig_c, fig_p = tc.rel(dc.cpu().numpy(), want_c), tc.rel(dp.cpu().numpy(), want_p)
    tol_c, tol_p = (tc.PCG_ALLOW * f for f in tc.PCG_FIGURES[(ncam, fix_first)])
    print(f"ncam {ncam} fix_first={fix_first}: it {it}  dc {fig_c:.3g} (allowed {tol_c:.3g})  dp {fig_p:.3g} (allowed {tol_p:.3g})")
    assert status == 0 and 0 < it < tc.PCG_ITERS and it % 5 == 0
    assert bool(dc[0].any()) != fix_first                                                              # exactly zero when fixed
    assert fig_c <= tol_c and fig_p <= tol_p
    d3c, d3p, it3, _ = track_ba.step(pl, out, tc.PCG_LAM, fix_first, 0.0, 3)
    w3c, w3p, _ = np_ba.solve_pcg(B, C, gc, gp, W, tc.PCG_LAM, fix_first, tol=0.0, iters=3)
    assert it3 == 3 and tc.rel(d3c.cpu().numpy(), w3c) <= 1e-8 and tc.rel(d3p.cpu().numpy(), w3p) <= 1e-8


@pytest.mark.gpu
def test_step_status_bits_and_iteration_control(hip):
    from sfm_mvs_amd import track_ba
    p = problem(41, 5, 60, np.full(60, 4))
    gone = p["cam_idx"] != 3                                                                            # camera 3 sees nothing
    p["obs"], p["cam_idx"], p["pt_idx"] = p["obs"][gone], p["cam_idx"][gone], p["pt_idx"][gone]
    p["X"][11] = np.nan                                                                                # point 11: every observation inactive
    p["track_off"], p["cam_off"], p["cam_obs"] = nb.plan(p["cam_idx"], p["pt_idx"], 5, 60)
    assert not fz.check_step(p, 1e-3, True) and not fz.check_step(p, 1e-1, False)
    pl = fz.device_plan(p)
    out, _ = fz.device_sweep(pl, p, p["cams"], p["X"], 1.0)
    dc, dp, it, status = track_ba.step(pl, out, 1e-3)
    assert status == 3 and not dc[3].any() and not dp[11].any() and bool(torch.isfinite(dc).all()) and bool(torch.isfinite(dp).all())
    clean = problem(42, 5, 60, np.full(60, 4))
    plc = fz.device_plan(clean)
    outc, _ = fz.device_sweep(plc, clean, clean["cams"], clean["X"], 1.0)
    assert track_ba.step(plc, outc, 1e-3)[3] == 0
    for cap in (0, 1, 4, 5, 7, 200):
        for tol in (1e-3, 1e-10):
            dc, dp, it, _ = track_ba.step(plc, outc, 1e-3, True, tol, cap)
            assert 0 <= it <= cap and (it % 5 == 0 or it == cap), (cap, tol, it)
            if cap == 0:                                                                               # dc = 0 and dp = Cd^-1 g_p
                assert not dc.any() and not fz.close("dp", dp, nb.step(*[outc[k].cpu().numpy().reshape(s) for k, s in (
                    ("JtJ_cam", (-1, 6, 6)), ("JtJ_pt", (-1, 3, 3)), ("Jtr_cam", (-1, 6)), ("Jtr_pt", (-1, 3)))], np.zeros((5, 60, 6, 3)), 1e-3, True)[1])


def looks(it, cg_iters):
    """The host waits of sfm_track_ba_step the header states."""
    return it // 5 + 1 if it < cg_iters else max(1, (cg_iters + 4) // 5)


@pytest.mark.gpu
def test_host_waits_of_one_attempt_and_of_a_whole_adjustment(hip):
    from sfm_mvs_amd import _lib, track_ba
    p = problem(51, 6, 200, np.full(200, 4))
    args = (dev(p["cams"]), K, dev(p["X"]), dev(p["obs"]), dev(p["cam_idx"]), dev(p["pt_idx"]))
    track_ba.bundle_adjust_tracks(*args, huber=1.0, iters=2)                                            # warm
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

    pl = track_ba.plan(args[4], args[5], 6, 200)
    first = track_ba.sweep(pl, args[0], K, args[2], args[3], 1.0)
    spare = pl.workspace()
    torch.cuda.synchronize()

    def attempt():
        dc, dp, it, status = track_ba.step(pl, first, 1e-3)
        trial = track_ba.sweep(pl, args[0] - dc, K, args[2] - dp, args[3], 1.0, 1, first["active"], spare)
        return it, track_ba._read(trial)

    (it, read), syncs, lib_syncs = counted(attempt)
    assert len(syncs) == 1, syncs                                                                      # the read of stat and count
    assert lib_syncs == looks(it, 200) and it > 0 and read[3] == 0 and read[0] < float(first["stat"][0])
    _, syncs, lib_syncs = counted(lambda: track_ba.plan(args[4], args[5], 6, 200))
    assert syncs == [] and lib_syncs == 0                                                              # plumbing without a host wait
    (_, _, hist, info), syncs, lib_syncs = counted(lambda: track_ba.bundle_adjust_tracks(*args, huber=1.0, iters=3))
    assert len(syncs) == 1 + len(info["cg_iters"]), (syncs, info)                                      # the first sweep, then one per attempt
    assert lib_syncs == sum(looks(it, 200) for it in info["cg_iters"])


@pytest.mark.gpu
def test_calibration_on_the_device(hip):
    """The corrupted ring scene: Huber ends at (1 + r) / 2 of the plain adjustment's camera-centre error or below, and the clean
    observations' rms error falls below the start's; the device follows the restatement's history."""
    from sfm_mvs_amd import track_ba
    p = ring_problem()

    def adjust(h):
        c, X, hist, info = track_ba.bundle_adjust_tracks(dev(p["cams"]), p["K"], dev(p["X"]), dev(p["obs"]), dev(p["cam_idx"]), dev(p["pt_idx"]), huber=h, iters=15)
        want = nb.bundle_adjust(p["cams"], p["K"], p["X"], p["obs"], p["cam_idx"], p["pt_idx"], huber=h, iters=15)
        assert len(hist) == len(want[2]) and np.allclose(hist, want[2], rtol=1e-6), (hist, want[2])
        assert info["active"] == 3200 and info["outliers"] == want[3]["outliers"] and info["crossed_refusals"] == 0
        return c.cpu().numpy(), X.cpu().numpy()

    e_l2, e_h, rms0, rms_h, e0 = calibration_figures(p, adjust)
    print(f"corrupted ring BA on the device: median camera-centre error start {e0:.5f}, L2 {e_l2:.5f}, Huber {e_h:.6f} (r = {e_h / e_l2:.4f}, bar {BA_BAR:.4f}); "
          f"clean rms start {rms0:.3f} px, Huber {rms_h:.3f} px")
    assert e_h <= BA_BAR * e_l2, (e_h, e_l2)
    assert rms_h < rms0, (rms_h, rms0)


@pytest.mark.gpu
def test_a_trial_that_crosses_a_camera_plane_is_refused_on_the_device(hip):
    from sfm_mvs_amd import track_ba
    cams, X, obs, ci, pi = crossing_problem()
    c, Xd, hist, info = track_ba.bundle_adjust_tracks(dev(cams), K, dev(X), dev(obs), dev(ci), dev(pi), huber=None, iters=30)
    _, _, whist, winfo = nb.bundle_adjust(cams, K, X, obs, ci, pi, huber=None, iters=30)
    assert info["crossed_refusals"] == winfo["crossed_refusals"] >= 1 and info["active"] == 26
    assert all(b <= a for a, b in zip(hist, hist[1:])) and hist[-1] < 1e-6 * hist[0] and np.allclose(hist[:4], whist[:4], rtol=1e-6)
    # the first attempt by hand: the trial point lies behind both cameras, two active observations crossed, nothing of them in the blocks
    p = dict(cams=cams, X=X, obs=obs, cam_idx=ci, pt_idx=pi, huber=np.inf, deg=-1)
    p["track_off"], p["cam_off"], p["cam_obs"] = nb.plan(ci, pi, 2, 13)
    pl = fz.device_plan(p)
    first, _ = fz.device_sweep(pl, p, cams, X, None)
    dc, dp, _, _ = track_ba.step(pl, first, 1e-3)
    trial = (cams - dc.cpu().numpy(), X - dp.cpu().numpy())
    assert trial[1][0, 2] < 0
    msg, _, _ = fz.check_sweep(p, np.inf, trial)
    assert not msg, msg
    out1, _ = fz.device_sweep(pl, p, trial[0], trial[1], None, 1, first["active"], pl.workspace())
    assert out1["count"].cpu().numpy().tolist()[:2] == [24, 2] and not track_ba.rows_of(pl, out1["ws"])[:2].any()


@pytest.mark.gpu
def test_adjust_tracks_closes_the_chain(hip):
    """run_tracks(robust=True) -> adjust_tracks -> run_tracks(P'): the largest reprojection error over the kept tracks does not rise."""
    from datagen import ring_cameras
    from sfm_mvs_amd import track_ba, tracks
    from test_gpu_tracks_refine import corrupted_device
    c, store, nq, kps = corrupted_device()
    case = c["case"]
    cams = ring_cameras(8) * (1 + 0.002 * np.random.default_rng(4).standard_normal((8, 6)))
    P0 = track_ba.P_from_cams(cams, case["K"])
    got = tracks.run_tracks(store, nq, case["pairs"], kps, P0, robust=True)

    def worst(res, P):
        cam = track_ba.cams_from_P(P, case["K"])
        return float(nb.observations(cam, case["K"], res["points"].astype(np.float64), res["obs"], res["cam_idx"], res["pt_idx"])["e"].max())

    P1, X1, info = tracks.adjust_tracks(got, P0, case["K"], huber=1.0, iters=10)
    again = tracks.run_tracks(store, nq, case["pairs"], kps, P1, robust=True)
    print(f"adjust_tracks: cost {info['history'][0]:.5g} -> {info['history'][-1]:.5g}; largest error {worst(got, P0):.3f} -> {worst(again, P1):.3f} px; "
          f"points {len(got['points'])} -> {len(again['points'])}, observations {len(got['obs'])} -> {len(again['obs'])}")
    assert P1.shape == (8, 3, 4) and X1.shape == (len(got["points"]), 3) and X1.dtype == np.float64
    assert info["history"][-1] < info["history"][0] and len(again["points"]) >= len(got["points"])
    assert worst(again, P1) <= worst(got, P0)
    plain = tracks.run_tracks(store, nq, case["pairs"], kps, P0)                                        # the dict of the other variant
    P2, X2, info2 = tracks.adjust_tracks(plain, P0, case["K"], huber=1.0, iters=3)
    assert X2.shape == (len(plain["points"]), 3) and info2["history"][-1] < info2["history"][0]


@pytest.mark.gpu
def test_a_short_fixed_seed_fuzz_run_finds_no_mismatch(hip):
    counts, bad, dt = fz.run(10.0, 5555)
    print(f"fuzz_track_ba: seed 5555, {sum(counts.values())} cases {counts}, {bad} mismatches, {dt:.0f} s")
    assert bad == 0 and all(c > 0 for c in counts.values()), counts


@pytest.mark.gpu
def test_committed_fuzz_logs_are_clean_and_name_this_code(hip):
    """profiles/track_ba_fuzz_seed*.log: no mismatch, and run on the code of csrc/tracks_ba.hip and csrc/common.h that the loaded library
    was built from (scripts/knn_code_hash.py: comments and whitespace do not count)."""
    import glob
    import re
    from sfm_mvs_amd import _lib
    have = _lib.code_hashes_of_binary()
    logs = sorted(glob.glob(os.path.join(ROOT, "profiles", "track_ba_fuzz_seed*.log")))
    assert len(logs) >= 2, logs
    total = 0
    for path in logs:
        text = open(path).read()
        m = re.search(r"fuzz_track_ba: seed \d+, (\d+) cases .*?, (\d+) mismatches", text)
        assert m and int(m.group(2)) == 0, f"{path}: no clean summary line"
        ids = re.findall(r"sfm_build_id (knn\.hip:\S+(?: \S+:\S+)*)", text)
        assert ids, f"{path} does not name the build it ran on"
        logged = dict(tok.split(":", 1) for tok in ids[-1].split() if ":" in tok)
        for name in ("tracks_ba.hip", "common.h"):
            assert logged.get(name) == have[name], f"{path} was produced by another csrc/{name} than the loaded binary's"
        total += int(m.group(1))
    assert total >= FUZZ_FLOOR, total
