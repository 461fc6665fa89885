"""The VERIFY-LO family on the device (sfm_verify_top / _lo / _lo_pick and verify.verify_pairs(lo=...)): every output equal to the
restatement tests/np_verify_lo.py word for word, floats as integer views with a NaN equal to a NaN, outputs in front of sentinel words
(include/sfm_hip.h, "VERIFY-LO"; docs/tracks.md §12)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

import np_verify as nv  # noqa: E402
import np_verify_lo as nl  # noqa: E402
import fuzz_verify_lo as fz  # noqa: E402
import verify_cases as vc  # noqa: E402
import verify_lo_cases as lc  # noqa: E402
from fuzz_verify import dev, first, flat_out, same  # noqa: E402
from fuzz_verify_lo import as_i64  # noqa: E402

FUZZ_FLOOR = 4000               # a tenth of the cases the committed logs hold, rounded down to one figure (docs/tracks.md §12.6)


@pytest.fixture(scope="module")
def planted():
    """A planted pair of 513 survivors with its restated stages at a budget of 24, computed once and never changed."""
    c = vc.planted_pair(513, 0.5, 1)
    return c, nv.verify_pairs(c["store"], c["nq"], c["pairs"], c["img_off"], c["kp"], c["K"], 0.7, budget=24, seed=7, stages=True)


# ---- top --------------------------------------------------------------------------------------------------------------------------

def top_both(counts, nm, T):
    from sfm_mvs_amd import verify
    want = nl.top(counts, nm, T)
    out, chk = flat_out(want.shape, torch.int64)
    verify.top_models(dev(counts), dev(nm), T, out=out)
    msg = first(same("top", out.cpu().numpy().view(np.uint64), want), chk())
    assert not msg, msg
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("H", [1, 3, 26, 103])
def test_top_on_both_sides_of_a_workgroup_of_slots(hip, H):
    """10 H = 10, 30, 260, 1 030: below and above 256 and 1 024 slots."""
    rng = np.random.default_rng(H)
    for n_pairs in (0, 1, 3):
        counts = rng.integers(0, 40, (n_pairs, H, 10)).astype(np.int32)
        nm = rng.integers(0, 11, (n_pairs, H)).astype(np.int32)
        for T in (1, 2, 16):
            keys = top_both(counts, nm, T)
            for p in range(n_pairs):
                k = nl.keys_of(counts[p], nm[p])
                assert keys[p, 0] == (k.max() if len(k) else 0)                          # what `score` leaves in best[p]
                assert [int(a) > int(b) for a, b in zip(keys[p, :-1], keys[p, 1:])] == [i < len(k) for i in range(T - 1)]      # descending, then zeros


@pytest.mark.gpu
def test_top_with_few_models_without_models_with_equal_counts_and_clamped_model_counts(hip):
    H = 26
    counts = np.full((3, H, 10), 7, np.int32)                        # all counts equal: the order falls to the slot
    nm = np.zeros((3, H), np.int32)
    nm[0, [3, 20]] = (2, 1)                                          # three models, fewer than T
    nm[2] = 10
    keys = top_both(counts, nm, 16)
    assert [int(nv.M32 - (int(k) & nv.M32)) for k in keys[0, :3]] == [30, 31, 200] and not keys[0, 3:].any() and not keys[1].any()
    assert [int(nv.M32 - (int(k) & nv.M32)) for k in keys[2]] == list(range(16))
    nm[1] = np.resize(np.array([-3, 11, 100, -2 ** 31, 2 ** 31 - 1], np.int32), H)      # outside 0..10: clamped as `score` clamps
    keys = top_both(counts, nm, 16)
    assert [int(nv.M32 - (int(k) & nv.M32)) for k in keys[1]] == list(range(10, 26))
    counts[1, 1, 4] = -1                                             # a word that is no count is taken as uint32
    counts[2, 0, 0] = -1                                             # at slot 0 the key is all ones
    keys = top_both(counts, nm, 2)
    assert keys[1, 0] == (np.uint64(0xFFFFFFFF) << np.uint64(32)) | np.uint64(nv.M32 - 14) and keys[2, 0] == np.uint64(2 ** 64 - 1)


@pytest.mark.gpu
def test_top_column_zero_is_the_best_of_score(hip, planted):
    from sfm_mvs_amd import verify
    case, st = planted
    keys = top_both(st["counts"], st["nmodels"], 16)
    assert keys[0, 0] == st["best"][0] and keys[0, 15] != 0
    d = dict(surv=dev(st["surv"]), m=dev(st["m"]), pairs=dev(case["pairs"]), img_off=dev(case["img_off"]), xn=dev(st["xn"]))
    counts, best = verify.score(dev(st["E_all"]), dev(st["nmodels"]), d["surv"], d["m"], d["pairs"], d["img_off"], d["xn"], float(st["thr2"]))
    assert torch.equal(verify.top_models(counts, dev(st["nmodels"]), 3)[:, 0], best)


# ---- lo ---------------------------------------------------------------------------------------------------------------------------

def lo_both(case, st, keys, thr2, wide2, m=None, xn=None, surv=None, pairs=None, trace=None):
    from sfm_mvs_amd import verify
    m = st["m"] if m is None else m
    xn = st["xn"] if xn is None else xn
    surv = st["surv"] if surv is None else surv
    pairs = case["pairs"] if pairs is None else pairs
    want = nl.lo(st["E_all"], keys, surv, m, pairs, case["img_off"], xn, thr2, wide2, trace=trace)
    n_pairs, T = keys.shape
    outs = [flat_out(s, t) for s, t in (((n_pairs, T, 9), torch.float64), ((n_pairs, T), torch.int32), ((n_pairs, T), torch.int32))]
    got = verify.local_optimise(dev(st["E_all"]), dev(as_i64(keys)), dev(surv), dev(m), dev(pairs), dev(case["img_off"]), dev(xn), thr2, wide2,
                                out=tuple(o for o, _ in outs))
    msg = first(*[same(n, g, w) for n, g, w in zip(("E_lo", "n_lo", "round_lo"), got, want)], *[c() for _, c in outs])
    assert not msg, msg
    return want


def survivor_values(case, st, key, m=None):
    """The float32 Sampson values of the survivors under the model of `key`."""
    mp = int(st["m"][0]) if m is None else m
    _, pts = nv._pair_points(st["surv"][0], mp, 0, 1, case["img_off"].astype(np.int64), st["xn"])
    return nl.sampson_value(st["E_all"][0].reshape(-1, 9)[nl.slot_of(key, st["nmodels"].shape[1])[1]], pts)


@pytest.mark.gpu
@pytest.mark.parametrize("m_cut", [0, 4, 7, 8, 9, 255, 256, 257, 513])
def test_lo_at_every_survivor_count_around_the_lanes(hip, planted, m_cut):
    case, st = planted
    thr2 = float(st["thr2"])
    keys = nl.top(st["counts"], st["nmodels"], 4)
    wide2 = nl.wide2_of(case["K"], 0.4, (3.0, 2.0, 1.0))
    E_lo, n_lo, rnd = lo_both(case, st, keys, thr2, wide2, m=np.array([m_cut], np.int32))
    assert (n_lo[0] <= m_cut).all() and (rnd[0] >= -1).all()
    if m_cut < 8:
        assert (rnd[0] == -1).all()                                  # fewer than eight survivors: no refit
    # every survivor in the wide set: the refit of all of them is reached whatever the model
    tr = []
    lo_both(case, st, keys[:, :1].copy(), thr2, [np.inf], m=np.array([m_cut], np.int32), trace=tr)
    assert len(tr) == (1 if m_cut >= 8 else 0)


@pytest.mark.gpu
def test_lo_with_a_wide_set_of_seven_and_of_eight_and_a_threshold_that_is_a_survivors_value(hip, planted):
    case, st = planted
    thr2 = float(st["thr2"])
    keys = nl.top(st["counts"], st["nmodels"], 1)
    v = np.sort(survivor_values(case, st, keys[0, 0]))
    assert v[6] < v[7] < v[8]
    for w, rounds in ((v[6], 0), (v[7], 1)):                         # wide2 = one survivor's float32 value exactly: it is in the set
        tr = []
        lo_both(case, st, keys, thr2, [float(w), float(w)], trace=tr)
        assert len(tr) >= rounds and (len(tr) == 0) == (rounds == 0)
        assert rounds == 0 or int((survivor_values(case, st, keys[0, 0]) <= np.float32(w)).sum()) == 8
    below = float(np.nextafter(np.float32(v[7]), np.float32(0)))
    tr = []
    lo_both(case, st, keys, thr2, [below], trace=tr)
    assert not tr


@pytest.mark.gpu
def test_lo_without_rounds_returns_the_candidate_with_its_count(hip, planted):
    case, st = planted
    for T in (1, 16):
        keys = nl.top(st["counts"], st["nmodels"], T)
        E_lo, n_lo, rnd = lo_both(case, st, keys, float(st["thr2"]), [])
        slots = [nl.slot_of(k, 24)[1] for k in keys[0]]
        assert np.array_equal(E_lo[0], st["E_all"][0].reshape(-1, 9)[slots]) and (rnd == -1).all()
        assert np.array_equal(n_lo[0], st["counts"][0].reshape(-1)[slots]) and n_lo[0, 0] == st["info"][0, 2]


@pytest.mark.gpu
def test_lo_of_candidates_without_a_model_and_of_padded_keys(hip, planted):
    case, st = planted
    thr2, wide2 = float(st["thr2"]), nl.wide2_of(case["K"], 0.4, (2.0, 1.0))
    keys = np.zeros((1, 16), np.uint64)
    keys[0, :3] = nl.top(st["counts"], st["nmodels"], 3)[0]          # T = 16 with `top` padded by zeros
    keys[0, 5] = np.uint64((9 << 32) | (nv.M32 - 240))               # a slot that is >= 10 H
    keys[0, 6] = np.uint64(5)                                        # a slot far past every model
    E_lo, n_lo, rnd = lo_both(case, st, keys, thr2, wide2)
    assert not E_lo[0, 3:].any() and not n_lo[0, 3:].any() and (rnd[0, 3:] == -1).all() and E_lo[0, :3].any(axis=1).all()
    lo_both(case, st, keys[:, :1].copy(), thr2, wide2)               # T = 1
    # a pair that names an image out of range has no survivors: the candidates keep their models with a count of 0
    for pair in ([0, 2], [-1, 1], [2 ** 31 - 1, 0]):
        _, n_lo, rnd = lo_both(case, st, keys, thr2, wide2, pairs=np.array([pair], np.int32))
        assert not n_lo.any() and (rnd == -1).all()
    # survivors whose node is out of range are skipped by the count and by the sums
    surv = st["surv"].copy()
    surv[0, 5] = (2 ** 31 - 1, 3)
    surv[0, 300] = (-1, -1)
    surv[0, 301, 1] = 513                                            # past the last node
    _, n_bad, _ = lo_both(case, st, keys, thr2, [], surv=surv)
    _, n_ok, _ = lo_both(case, st, keys, thr2, [])
    assert (n_bad <= n_ok).all() and (n_bad >= n_ok - 3).all()
    lo_both(case, st, keys, thr2, wide2, surv=surv)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["one point", "a line", "nan", "huge"])
def test_lo_on_degenerate_coordinates(hip, planted, name):
    case, st = planted
    xn = st["xn"].copy()
    if name == "one point":
        xn[:] = xn[0]
    if name == "a line":
        xn[:, 1] = 2 * xn[:, 0] + 0.1
    if name == "nan":
        xn[::7] = np.nan
    if name == "huge":
        xn[::5] = 1e150
        xn[3::10, 0] = -1e150
    keys = nl.top(st["counts"], st["nmodels"], 4)
    tr = []
    E_lo, n_lo, rnd = lo_both(case, st, keys, float(st["thr2"]), [np.inf, np.inf, 1.0], xn=xn, trace=tr)
    assert np.isfinite(E_lo).all() and len(tr) >= 4
    if name == "huge":                                               # sums of huge products of both signs: the non-finite stop
        from sfm_mvs_amd import hostgeom
        assert not np.isfinite(tr[0][3]).all() and not np.isfinite(hostgeom.verify_refit(tr[0][3])).all() and len(tr) == 4 and (rnd == -1).all()


@pytest.mark.gpu
def test_the_refit_on_the_device_is_the_host_refit_bit_for_bit(hip, planted):
    """E_lo shows E_new where a refit wins (round_lo = 0): at these three thresholds, with the wide set at four times the threshold, one of
    the eight candidates of this pair is beaten by its first refit.  The device's words are those of `sfm_host_verify_refit` on the M the
    restatement forms."""
    from sfm_mvs_amd import hostgeom
    case, st = planted
    keys = nl.top(st["counts"], st["nmodels"], 8)
    shown = 0
    for thr2 in (float(st["thr2"]), 1e-6, 1e-4):
        tr = []
        E_lo, n_lo, rnd = lo_both(case, st, keys, thr2, [4 * thr2], trace=tr)
        for p, t, r, M in tr:
            if rnd[p, t] == 0:
                assert np.array_equal(E_lo[p, t].view(np.int64), hostgeom.verify_refit(M).reshape(9).view(np.int64))
                shown += 1
    assert shown == 3


# ---- pick -------------------------------------------------------------------------------------------------------------------------

def pick_both(keys, E_lo, n_lo, rnd, H):
    from sfm_mvs_amd import verify
    want = nl.pick(keys, E_lo, n_lo, rnd, H)
    n_pairs = len(keys)
    outs = [flat_out(s, t) for s, t in (((n_pairs, 1, 10, 9), torch.float64), ((n_pairs, 1), torch.int32), ((n_pairs,), torch.int64), ((n_pairs, 8), torch.int32))]
    got = verify.pick(dev(as_i64(keys)), dev(E_lo), dev(n_lo), dev(rnd), H, out=tuple(o for o, _ in outs))
    msg = first(*[same(n, g, w) for n, g, w in zip(("E_sel", "nmodels_sel", "best_sel", "lo_info"), (got[0], got[1], got[2].cpu().numpy().view(np.uint64), got[3]), want)],
                *[c() for _, c in outs])
    assert not msg, msg
    return want, got


@pytest.mark.gpu
def test_pick_with_ties_without_counts_and_with_one_candidate(hip):
    rng = np.random.default_rng(3)
    H = 24
    keys = ((rng.integers(1, 30, (4, 16)).astype(np.uint64)) << np.uint64(32)) | (np.uint64(nv.M32) - rng.integers(0, 240, (4, 16)).astype(np.uint64))
    keys[3] = 0                                                      # a pair without a model
    keys[0, 0] = 0                                                   # candidate 0 without a model: a later one wins
    E_lo = rng.normal(size=(4, 16, 9))
    n_lo = rng.integers(0, 9, (4, 16)).astype(np.int32)
    n_lo[0, [0, 4, 9]] = 50                                          # a tie: the lowest t that has a model, 4
    n_lo[1] = 0                                                      # every count zero: candidate 0
    rnd = rng.integers(-1, 8, (4, 16)).astype(np.int32)
    (E_sel, nm_sel, best_sel, info), _ = pick_both(keys, E_lo, n_lo, rnd, H)
    assert info[0, 2] == 4 and info[0, 1] == 50 and info[1, 2] == 0 and info[1, 1] == 0 and nm_sel[1, 0] == 1 and best_sel[1] == nv.M32
    assert info[3].tolist() == [0, 0, -1, -1, -1, -1, 0, 0] and nm_sel[3, 0] == 0 and best_sel[3] == 0 and info[0, 6] == 15
    for n_pairs in (0, 1):
        pick_both(keys[:n_pairs, :1].copy(), E_lo[:n_pairs, :1].copy(), n_lo[:n_pairs, :1].copy(), rnd[:n_pairs, :1].copy(), H)      # T = 1
    pick_both(keys[1:3, :1].copy(), E_lo[1:3, :1].copy(), n_lo[1:3, :1].copy(), rnd[1:3, :1].copy(), H)


@pytest.mark.gpu
def test_select_takes_what_pick_writes(hip, planted):
    from sfm_mvs_amd import verify
    case, st = planted
    thr2 = float(st["thr2"])
    keys = nl.top(st["counts"], st["nmodels"], 4)
    cand = nl.lo(st["E_all"], keys, st["surv"], st["m"], case["pairs"], case["img_off"], st["xn"], thr2, nl.wide2_of(case["K"], 0.4, (3.0, 1.0)))
    (E_sel, nm_sel, best_sel, info), got = pick_both(keys, *cand, 24)
    want = nv.select(E_sel, nm_sel, best_sel, st["surv"], st["m"], case["pairs"], case["img_off"], st["xn"], thr2)
    d = dict(surv=dev(st["surv"]), m=dev(st["m"]), pairs=dev(case["pairs"]), img_off=dev(case["img_off"]), xn=dev(st["xn"]))
    out = verify.select(got[0], got[1], got[2], d["surv"], d["m"], d["pairs"], d["img_off"], d["xn"], thr2)
    msg = first(*[same(n, g, w) for n, g, w in zip(("keep", "E", "Rt", "info"), out, want)])
    assert not msg, msg
    assert want[3][0, 2] == info[0, 1] >= st["info"][0, 2] and want[3][0, 4:6].tolist() == [0, 0] and want[0].any()


# ---- verify_pairs -----------------------------------------------------------------------------------------------------------------

def multi_pair_case():
    from test_gpu_verify import multi_pair_case as base
    return base()


LO = dict(top=4, rounds=3, widen=(3.0, 2.0, 1.0))


@pytest.mark.gpu
def test_verify_pairs_with_lo_is_the_composition_twice_without_a_host_wait(hip):
    from sfm_mvs_amd import _lib, tracks, verify
    case = multi_pair_case()
    want = nl.verify_pairs(case["store"], case["nq"], case["pairs"], case["img_off"], case["kp"], case["K"], 0.7, budget=64, seed=3, lo_top=4,
                           widen=LO["widen"])
    args = (dev(case["store"]), dev(case["nq"]), dev(case["pairs"]), dev(case["img_off"]), dev(case["kp"]), case["K"], 0.7)
    verify.verify_pairs(*args, budget=64, seed=3, lo=LO)              # allocations and module loading happen here
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    waits = _lib.lib().sfm_host_sync_count()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = verify.verify_pairs(*args, budget=64, seed=3, lo=LO)
        again = verify.verify_pairs(*args, budget=64, seed=3, lo=LO)
        ones = verify.verify_pairs(*args, budget=64, seed=3, lo=LO, max_models_bytes=1)                   # one pair a chunk
        threes = verify.verify_pairs(*args, budget=64, seed=3, lo=LO, max_models_bytes=3 * 64 * 720)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert _lib.lib().sfm_host_sync_count() == waits
    for name in ("keep", "E", "Rt", "info", "lo_info"):
        for out in (got, again, ones, threes):
            msg = same(name, out[name], want[name])
            assert not msg, msg
        assert torch.equal(got[name].view(torch.uint8), again[name].view(torch.uint8))                   # a second run gives the same bits
    plain = nv.verify_pairs(case["store"], case["nq"], case["pairs"], case["img_off"], case["kp"], case["K"], 0.7, budget=64, seed=3)
    assert (want["info"][:, 2] >= plain["info"][:, 2]).all() and np.array_equal(want["info"][:, :2], plain["info"][:, :2])
    assert np.array_equal(want["lo_info"][:, 0], plain["info"][:, 2]) and want["lo_info"][2].tolist() == [0, 0, -1, -1, -1, -1, 0, 0]
    edges = tracks.match_edges(args[0], args[1], args[2], args[3], 0.7, keep=got["keep"]).cpu().numpy().reshape(len(case["nq"]), -1, 2)
    assert ((edges[:, :, 0] >= 0) == (want["keep"] != 0)).all() and want["keep"][0].any()
    kps = [dev(k) for k in case["kps"]]
    batched = tracks.verify_keep(args[0], case["nq"], case["pairs"], kps, case["K"], batched=True, budget=64, seed=3, lo=True)
    assert torch.equal(batched, verify.verify_pairs(*args, budget=64, seed=3, lo=True)["keep"])
    assert verify.workspace_bytes(4, 300, 64, lo=LO) - verify.workspace_bytes(4, 300, 64) == 4 * (4 * 88 + 720 + 12)


@pytest.mark.gpu
def test_verify_pairs_without_lo_is_the_composition_of_the_six_wrappers(hip):
    from sfm_mvs_amd import verify
    case = multi_pair_case()
    store, nq, pairs, img_off, kp = (dev(case[k]) for k in ("store", "nq", "pairs", "img_off", "kp"))
    got = verify.verify_pairs(store, nq, pairs, img_off, kp, case["K"], 0.7, budget=64, seed=3, lo=None)
    assert sorted(got) == ["E", "Rt", "info", "keep"]
    thr2 = verify.thr2_of(case["K"], 0.4)
    xn = verify.normalise_keypoints(kp, case["K"])
    surv, m = verify.survivors(store, nq, pairs, img_off, 0.7)
    part = (surv, m, pairs, img_off, xn)
    nmodels, E = verify.models(verify.samples(m, 64, 3), *part)
    counts, best = verify.score(E, nmodels, *part, thr2)
    want = verify.select(E, nmodels, best, *part, thr2)
    for name, w in zip(("keep", "E", "Rt", "info"), want):
        assert torch.equal(got[name].view(torch.uint8), w.view(torch.uint8)), name


# ---- the planted scenes -----------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("m", vc.SIZES)
def test_lo_beside_the_plain_and_the_per_pair_path_on_the_planted_scenes(hip, m):
    """The monotone property on every scene and the quality assertions of tests/test_verify_lo_cpu.py on the device: inlier shares 0.3, 0.5,
    0.8 x seeds 0, 1, 2 at this m, default budget, default LO, means over the seeds.  The per-pair path runs beside them."""
    from sfm_mvs_amd import tracks, verify
    R_true = lc.planted_rotation()
    for frac in vc.FRACTIONS:
        rows = []
        for seed in lc.SEEDS:
            case = vc.planted_pair(m, frac, seed)
            args = (dev(case["store"]), dev(case["nq"]), dev(case["pairs"]), dev(case["img_off"]), dev(case["kp"]), case["K"], 0.7)
            plain = {k: v.cpu().numpy() for k, v in verify.verify_pairs(*args, seed=seed).items()}
            lo = {k: v.cpu().numpy() for k, v in verify.verify_pairs(*args, seed=seed, lo=True).items()}
            assert lo["info"][0, 2] >= plain["info"][0, 2] and lo["lo_info"][0, 0] == plain["info"][0, 2], (frac, seed)
            pp = tracks.verify_keep(args[0], case["nq"], [(0, 1)], [dev(k) for k in case["kps"]], case["K"]).cpu().numpy()[0]
            rows.append((vc.rates(lo["keep"][0], case["planted"]), vc.rates(plain["keep"][0], case["planted"]), vc.rates(pp, case["planted"]),
                         lc.rotation_error_deg(lo["Rt"][0], R_true), lc.rotation_error_deg(plain["Rt"][0], R_true)))
            print(f"inliers {frac} m {m} seed {seed}: LO {rows[-1][0][0]:.3f} / {rows[-1][0][1]:.4f} rotation {rows[-1][3]:.2f} deg; plain {rows[-1][1][0]:.3f} / "
                  f"{rows[-1][1][1]:.4f} rotation {rows[-1][4]:.2f} deg; per pair {rows[-1][2][0]:.3f} / {rows[-1][2][1]:.4f}; lo_info {lo['lo_info'][0].tolist()}")
        mean = lambda k, j: float(np.mean([r[k][j] for r in rows]))  # noqa: E731
        print(f"inliers {frac} m {m} mean of the seeds: LO {mean(0, 0):.4f} / {mean(0, 1):.5f}; plain {mean(1, 0):.4f} / {mean(1, 1):.5f}; per pair {mean(2, 0):.4f} / "
              f"{mean(2, 1):.5f}")
        assert mean(0, 0) >= mean(1, 0) - 0.02
        assert mean(0, 1) <= mean(1, 1) + 0.01
        if frac == 0.3:
            if m in lc.AIM_MET_AT:
                assert mean(0, 0) >= mean(2, 0) - 0.02
            else:
                assert mean(0, 0) >= mean(1, 0)


# ---- fuzzing ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_a_short_fixed_seed_fuzz_run(hip):
    counts, bad, dt = fz.run(4.0, 20261, log=print)
    print(f"fuzz_verify_lo: {sum(counts.values())} cases {counts} in {dt:.1f} s")
    assert bad == 0 and sum(counts.values()) >= 3


@pytest.mark.gpu
def test_committed_fuzz_logs_are_clean_and_of_this_code(hip):
    """profiles/verify_lo_fuzz_seed*.log: no mismatch, and run on the code of csrc/verify_lo.hip and csrc/common.h that the loaded library
    was built from (scripts/knn_code_hash.py: comments and whitespace do not count)."""
    import glob
    import re
    from sfm_mvs_amd import _lib
    have = _lib.code_hashes_of_binary()
    logs = sorted(glob.glob(os.path.join(ROOT, "profiles", "verify_lo_fuzz_seed*.log")))
    assert len(logs) >= 2, logs
    total = 0
    for path in logs:
        text = open(path).read()
        m = re.search(r"fuzz_verify_lo: seed \d+, (\d+) cases .*?, (\d+) mismatches", text)
        assert m and int(m.group(2)) == 0, f"{path}: no clean summary line"
        ids = re.findall(r"sfm_build_id (knn\.hip:\S+(?: \S+:\S+)*)", text)
        assert ids, f"{path} does not name the build it ran on"
        logged = dict(tok.split(":", 1) for tok in ids[-1].split() if ":" in tok)
        for name in ("verify_lo.hip", "common.h"):
            assert logged.get(name) == have[name], f"{path} was produced by another csrc/{name} than the loaded binary's"
        total += int(m.group(1))
    assert total >= FUZZ_FLOOR, total
