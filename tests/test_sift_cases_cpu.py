"""The SIFT limit table (tests/sift_cases.py) against the CPU oracle alone: the table must reach the launch paths and edges it
claims, so that tests/test_gpu_sift_limits.py — which compares the HIP path with this oracle on the same table — cannot pass
vacuously.  No GPU, nothing of sfm_mvs_amd."""
import numpy as np

import sift_cases as sc


def test_tap_counts_cover_every_blur_kernel(oracle):
    """Kernel lengths of the base blur and every layer of every parameter set, from oracle.sift_gauss_kernel: every odd length
    3..27 (the generic kernel at R = 1 and each gauss_blur_fixed_kernel<N>), 55 (the limit) and at least five lengths of 29..53
    (the generic kernel's upper range); nothing beyond 55.  The two sets the limit test rejects must really exceed it."""
    union = set()
    for nl, sg in sc.PARAM_SETS:
        taps = sc.tap_counts(oracle, nl, sg)
        print(f"nL {nl} sigma {sg}: taps {taps}")
        assert len(taps) == nl + 3 and all(t % 2 == 1 for t in taps) and max(taps) <= sc.MAX_TAPS
        union |= set(taps)
    print("union", sorted(union))
    assert set(range(3, 28, 2)) <= union and set(sc.FIXED_TAPS) <= union
    assert sc.MAX_TAPS in union
    assert len([t for t in union if 29 <= t <= 53]) >= 5
    # the 3-tap kernel is only a test of R = 1 where its outer taps move a pixel: 1.9e-22 at sigma 1.0 (an identity in float32),
    # 4.3e-3 — a grey level on 255, 2^16 ulps — at the set that is in the table for it
    base = lambda p: oracle.sift_gauss_kernel(sc.blur_sigmas(*p)[0])
    assert len(base((3, 1.0))) == 3 and base((3, 1.0))[0] * 255 < 2.0 ** -24
    assert len(base(sc.EFFECTIVE_3_TAP_SET)) == 3 and base(sc.EFFECTIVE_3_TAP_SET)[0] > 1e-3
    # the pair launches are taken by the defaults only (layers 1, 2, nL+1, nL+2 of 11, 13, 21, 27 taps)
    t = sc.tap_counts(oracle, *sc.DEFAULT)
    assert (t[1], t[2], t[4], t[5]) == (11, 13, 21, 27)
    assert max(sc.tap_counts(oracle, 3, 3.6)) == 57 and max(sc.tap_counts(oracle, 1, 1.6)) == 91


def test_blur_schedule_restates_the_oracle(oracle):
    """sift_cases.blur_sigmas is the schedule the oracle blurs with: octave 0 of its pyramid, layer to layer, equals a blur of
    the layer before with sift_gauss_kernel(blur_sigmas[i]).  float64 here against the oracle's float32 sums of up to 55 terms
    <= 255 in each of two passes: at worst 2 * 55 * 255 * 2^-24 = 1.7e-3 grey levels."""
    from scipy.ndimage import correlate1d
    g = sc.frame(65, 33)
    for nl, sg in [(3, 3.4), (8, 1.0)]:
        _, _, pyr = oracle.sift(g, n_octave_layers=nl, sigma=sg, want_pyramid=True)
        sig = sc.blur_sigmas(nl, sg)
        for i in range(1, nl + 3):
            k = oracle.sift_gauss_kernel(sig[i]).astype(np.float64)
            want = correlate1d(correlate1d(pyr[i - 1].astype(np.float64), k, axis=1, mode="mirror"), k, axis=0, mode="mirror")
            assert np.abs(pyr[i] - want).max() < 2e-3, (nl, sg, i)
    # the base blur: at sigma 1.0 its taps are (1.9e-22, 1, 1.9e-22), so layer 0 IS the doubled frame; layer 0 at 1.045 is that
    # frame under the effective 3-tap kernel, and differs from it by grey levels (the R = 1 case is not vacuous)
    up = oracle.sift(g, sigma=1.0, want_pyramid=True)[2][0].astype(np.float64)
    bil = 0.5625 * g[1:, 1:] + 0.1875 * g[1:, :-1] + 0.1875 * g[:-1, 1:] + 0.0625 * g[:-1, :-1]        # even pixels of a 2x bilinear resize
    assert np.abs(up[::2, ::2][1:, 1:] - bil).max() < 1e-6
    k = oracle.sift_gauss_kernel(sc.blur_sigmas(*sc.EFFECTIVE_3_TAP_SET)[0]).astype(np.float64)
    got = oracle.sift(g, sigma=sc.EFFECTIVE_3_TAP_SET[1], want_pyramid=True)[2][0]
    want = correlate1d(correlate1d(up, k, axis=1, mode="mirror"), k, axis=0, mode="mirror")
    assert np.abs(got - want).max() < 2e-3 and np.abs(got - up).max() > 0.5


def test_every_gpu_pair_has_keypoints_to_compare(oracle):
    """Oracle keypoint counts of every (frame, parameter set) the GPU test runs: above the table's floor; the pairs without
    keypoints are the ones the table marks with 0, at most a quarter of all."""
    pairs = sc.gpu_pairs()
    zero = 0
    for (w, h), (nl, sg) in pairs:
        floor = sc.KEYPOINT_FLOORS[(w, h)][(nl, sg)]
        kp, des = sc.oracle_sift(oracle, (w, h), sc.frame(w, h), nl, sg)
        print(f"{w}x{h} nL {nl} sigma {sg}: {len(kp)} keypoints (floor {floor})")
        assert des.shape == (len(kp), 128)
        if floor == 0:
            zero += 1
        else:
            assert len(kp) >= floor
    assert len(pairs) == sum(len(v) for v in sc.KEYPOINT_FLOORS.values())
    assert 4 * zero <= len(pairs), (zero, len(pairs))
    # every frame size of the table and every parameter set is part of some pair with keypoints
    live = [(s, p) for s, p in pairs if sc.KEYPOINT_FLOORS[s][p] > 0]
    assert {s for s, _ in live} == set(sc.FRAME_SIZES) | set(sc.TINY_SIZES)
    assert {p for _, p in live} == set(sc.PARAM_SETS)


def test_column_frame_fills_two_or_three_x_ranges_with_ties(oracle):
    """The column frame is what the ordering pass does not expect: >= 200 keypoints in <= 4 of its 256 x ranges (it assumes
    about n / 256 each) and >= 50 keypoints that share (x, y) with another (the rank comparison's tie cascade)."""
    g = sc.column_frame()
    assert g.shape == (400, 512)
    kp, _ = sc.oracle_sift(oracle, "column", g, *sc.DEFAULT)
    bk = sc.x_bucket(kp[:, 0] * np.float32(2), 2 * g.shape[1])          # the pass sees x on the doubled base
    used, members = np.unique(bk, return_counts=True)
    _, inv, cnt = np.unique(kp[:, :2].view(np.int32), axis=0, return_inverse=True, return_counts=True)
    shared = int((cnt[inv.ravel()] > 1).sum())
    print(f"column frame: {len(kp)} keypoints, ranges {used.tolist()} with {members.tolist()} members, {shared} sharing (x, y)")
    assert len(kp) >= 200 and len(used) <= 4 and shared >= 50
    assert members.max() >= 100


def test_wide_sigma_sets_need_several_orientation_chunks(oracle):
    """orientation_kernel takes 1024 window samples per pass; a window of radius >= 16 (33 x 33 = 1089 samples) needs a second
    pass.  The (3, 2.4) and (3, 3.4) sets have such keypoints on both frames of the spread; (3, 3.4) also windows of five passes."""
    for p in [(3, 2.4), (3, 3.4)]:
        for s in sc.SPREAD_SIZES:
            kp, _ = sc.oracle_sift(oracle, s, sc.frame(*s), *p)
            r = sc.orientation_radius(kp)
            many = int((r >= 16).sum())
            print(f"{s} nL {p[0]} sigma {p[1]}: {many} of {len(kp)} keypoints with radius >= 16, largest {int(r.max())}")
            assert (2 * 16 + 1) ** 2 > sc.ORI_CHUNK and many > 0
    kp, _ = sc.oracle_sift(oracle, (200, 150), sc.frame(200, 150), 3, 3.4)
    assert (2 * int(sc.orientation_radius(kp).max()) + 1) ** 2 > 4 * sc.ORI_CHUNK


def test_capacity_frames_are_the_ones_the_sweep_counts_on(oracle):
    for k, want in enumerate([556, 1201]):
        kp, _ = sc.oracle_sift(oracle, ("capacity", k), sc.capacity_frame(k), *sc.DEFAULT)
        assert len(kp) == want
    assert sc.CAPACITIES[0] == 64 and sc.CAPACITIES[-1] == 1 << 17 and sorted(sc.CAPACITIES) == sc.CAPACITIES
    assert set(sc.CAPACITIES) <= set(sc.CAPACITIES_FINE)
