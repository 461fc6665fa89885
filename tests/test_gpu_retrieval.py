"""The RETRIEVAL family on the device (sfm_vlad_accumulate / _centres / _signature / _shortlist / _pairs, retrieval.select_pairs,
tracks.retrieval_pairs): every output word equal to the restatement tests/np_retrieval.py, floats as integer views, outputs in front of
sentinel words (include/sfm_hip.h, "RETRIEVAL"; docs/retrieval.md)."""
import functools
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

import fuzz_retrieval as fz  # noqa: E402
import np_retrieval as nr  # noqa: E402
import retrieval_cases as rc  # noqa: E402
from datagen import sift_like  # noqa: E402
from fuzz_tracks import dev, gen_offsets  # noqa: E402
from fuzz_verify import same  # noqa: E402

FUZZ_FLOOR = 2000             # a tenth of the cases the committed logs hold, rounded down to one figure (docs/retrieval.md §7)
SIZES = (0, 1, 63, 64, 65, 255, 256, 257)
MAX_NORM2 = 256 * 128 * 127 * 127


@functools.lru_cache(maxsize=None)
def node_list(seed=3):
    """One image of every size of SIZES in one node list, some rows equal.  Computed once, never changed (copy before editing)."""
    rng = np.random.default_rng(seed)
    n = sum(SIZES)
    desc = sift_like(rng, n)
    desc[rng.integers(n, size=n // 8)] = desc[rng.integers(n, size=n // 8)]
    return desc, np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int32)


def centres_of(desc, C, seed=5):
    """C centres: some are descriptor rows (distances of zero), some equal each other, the rest off the integer grid."""
    rng = np.random.default_rng([seed, C])
    cen = sift_like(rng, C) + rng.normal(0, 0.37, (C, 128)).astype(np.float32)
    own = rng.random(C) < 0.4
    cen[own] = desc[rng.integers(len(desc), size=int(own.sum()))]
    if C > 1:
        cen[rng.integers(C, size=C // 4)] = cen[rng.integers(C, size=C // 4)]
    return cen


def ok(msg):
    assert not msg, msg


# ---- accumulate ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("C", [1, 2, 63, 64, 65, 255, 256])
def test_accumulate_images_around_the_wave_and_the_block_at_every_centre_count(hip, C):
    desc, img_off = node_list()
    msg, (a, acc, count) = fz.accumulate_both(desc, centres_of(desc, C), img_off, 4096.0)
    ok(msg)
    assert (a >= 0).all() and count.sum() == len(desc) and count.sum(1).tolist() == list(SIZES) and not acc[0].any()


@pytest.mark.gpu
@pytest.mark.parametrize("n_img", [1, 2, 3, 64, 65, 257])
def test_accumulate_image_counts_with_empty_images_across_the_chunk_of_1024(hip, n_img):
    rng = np.random.default_rng(n_img)
    n = 2500
    desc = sift_like(rng, n)
    msg, (_, _, count) = fz.accumulate_both(desc, centres_of(desc, 16), gen_offsets(rng, n_img, n), 4096.0)
    ok(msg)
    assert count.sum() == n
    off = np.zeros(n_img + 1, np.int32)                              # one image holds every node: the last, the first, one in the middle
    for at in sorted({0, n_img // 2, n_img - 1}):
        off[:at + 1], off[at + 1:] = 0, n
        msg, (_, _, count) = fz.accumulate_both(desc, centres_of(desc, 16), off, 4096.0)
        ok(msg)
        assert count[at].sum() == n


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [2.0 ** -3, 2.0 ** 12, 0.5, 2.0 ** 24, 3e38])
def test_accumulate_scales_from_an_eighth_to_one_that_makes_the_clamp_bite(hip, scale):
    desc, img_off = node_list()
    msg, (_, acc, _) = fz.accumulate_both(desc, centres_of(desc, 16), img_off, scale)
    ok(msg)
    if scale >= 2.0 ** 24:                                           # differences of up to 255 times 2^24: clamped terms
        assert np.abs(acc).max() >= 2 ** 30


@pytest.mark.gpu
def test_accumulate_rows_with_nan_inf_denormals_and_an_all_zero_set(hip):
    desc, img_off = node_list()
    desc = desc.copy()
    cen = centres_of(desc, 16)
    desc[5, 7], desc[70, 0], desc[71, 127], desc[300, 64], desc[400, 3] = np.nan, np.inf, -np.inf, 3e30, 1e18
    desc[500, 9], desc[501, 10], desc[502] = 1e-45, -1e-40, 1e-41
    msg, (a, acc, count) = fz.accumulate_both(desc, cen, img_off, 4096.0)
    ok(msg)
    assert (a[[5, 70, 71, 300]] == -1).all() and a[400] >= 0 and a[502] >= 0 and count.sum() == len(desc) - 4
    cen[3, 5], cen[4, 6] = np.nan, np.inf                            # centres that are nobody's candidate
    msg, (a, _, _) = fz.accumulate_both(desc, cen, img_off, 4096.0)
    ok(msg)
    assert not np.isin(a, [3, 4]).any()
    msg, (a, acc, _) = fz.accumulate_both(np.zeros_like(desc), np.zeros_like(cen), img_off, 4096.0)   # all zero: centre 0 takes everything
    ok(msg)
    assert not a.any() and not acc.any()
    ok(fz.accumulate_both(desc[:0], cen, np.zeros(4, np.int32), 1.0)[0])                                  # no keypoint at all


# ---- centres ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_centres_with_counts_of_zero_and_one_and_large_sums(hip):
    desc, _ = node_list()
    cen = centres_of(desc, 65)
    cen[7, 3], cen[7, 4] = -0.0, 1e-40                               # bits an empty centre must keep
    _, acc, count = nr.accumulate(desc, cen, [0, len(desc)], 4096.0)
    acc, count = acc[0].copy(), count[0].copy()
    count[7], count[8] = 0, 1
    acc[9] = 2 ** 62
    acc[10] = -(2 ** 53 + 1)
    msg, new = fz.centres_both(cen, acc, count, 4096.0)
    ok(msg)
    assert np.array_equal(new[7].view(np.int32), cen[7].view(np.int32))
    ok(fz.centres_both(cen, acc, count, 2.0 ** -3)[0])


@pytest.mark.gpu
def test_eight_chained_lloyd_rounds_equal_the_restated_chain_twice(hip):
    from sfm_mvs_amd import retrieval
    desc, _ = node_list()
    want = nr.train_vocabulary(desc, 16, 8, 4, 4096.0)
    d = dev(desc)
    got, again = retrieval.train_vocabulary(d, 16, 8, 4, 4096.0), retrieval.train_vocabulary(d, 16, 8, 4, 4096.0)
    ok(same("centres", got, want))
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))
    assert not np.array_equal(want, desc[nr.initial_rows(len(desc), 16, 4)])                            # the rounds moved them


# ---- signature ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("ssr", [False, True])
@pytest.mark.parametrize("qs", [1.0, 127.0, 254.0, 1000.0])
def test_signatures_of_sums_the_float64_conversion_rounds(hip, ssr, qs):
    rng = np.random.default_rng(int(qs) + ssr)
    acc = rng.integers(-2 ** 20, 2 ** 20, (3, 65, 128), dtype=np.int64)
    acc[0, 0] = 0                                                    # a block of zeros
    acc[0, 1, :6] = [1, -1, 2 ** 53 + 1, -(2 ** 53 + 1), 2 ** 62, -(2 ** 62)]
    acc[0, 2] = rng.choice([2 ** 53 + 1, -(2 ** 53 + 1), 2 ** 53 + 3], 128)
    acc[0, 3] = rng.choice([2 ** 62, -(2 ** 62), 2 ** 62 - 1], 128)
    acc[1, 4] = 0
    acc[1, 4, 17] = -1                                               # a single word: q = -127 at qs >= 127
    acc[2] = 0                                                       # an image of zeros
    msg, (sig, norm2) = fz.signature_both(acc, ssr, qs)
    ok(msg)
    assert not sig[0, :128].any() and norm2[2] == 0 and sig[1, 4 * 128 + 17] == -min(int(qs), 127)
    if qs == 1000.0:
        assert (np.abs(sig.astype(np.int32)) == 127).sum() > 100     # it clips


@pytest.mark.gpu
def test_norm2_at_its_documented_maximum(hip):
    rng = np.random.default_rng(0)
    acc = rng.choice([5, -5], (2, 256, 128)).astype(np.int64)        # equal magnitudes: 2000 / sqrt(128) = 177 clips at 127
    msg, (sig, norm2) = fz.signature_both(acc, False, 2000.0)
    ok(msg)
    assert (np.abs(sig.astype(np.int32)) == 127).all() and norm2.tolist() == [MAX_NORM2, MAX_NORM2] and MAX_NORM2 < 2 ** 31


# ---- shortlist ----------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def signature_set(n_img, C=3, seed=7):
    """Signatures with equal rows (exact ties), opposite rows (sim = -1) and zero rows.  Computed once (copy before editing)."""
    rng = np.random.default_rng([seed, n_img])
    base = rng.normal(0, 20, (1, C * 128))
    sig = np.clip(np.rint(base + rng.normal(0, 25, (n_img, C * 128))), -127, 127).astype(np.int8)
    if n_img >= 3:
        sig[2] = sig[0]
    if n_img >= 15:
        sig[7], sig[9], sig[11], sig[12] = sig[3], -sig[3], 0, sig[0]
    return sig, (sig.astype(np.int64) ** 2).sum(1).astype(np.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("n_img", [1, 2, 3, 15, 16, 17, 63, 64, 65, 257])
def test_shortlist_image_counts_around_the_tiles_at_every_k(hip, n_img):
    sig, norm2 = signature_set(n_img)
    for k in sorted({1, 2, min(max(n_img - 1, 1), 64), min(n_img, 64), 64}):
        msg, (nbr, sim) = fz.shortlist_both(sig, norm2, k, None)
        ok(msg)
        live = int((norm2 != 0).sum())
        assert ((nbr >= 0).sum(1)[norm2 != 0] == min(k, live - 1)).all() and (nbr[norm2 == 0] == -1).all()
    if n_img >= 15:
        assert nbr[3, 0] == 7 and sim[3, 0] == 1.0 and nbr[0, :2].tolist() == [2, 12] and sim[0, 0] == sim[0, 1] == 1.0
        assert not np.isin(nbr, [11]).any()                          # an image without a norm is nobody's neighbour
        if n_img <= 65:                                              # k = 64 lists every candidate: the opposite image comes last
            assert nbr[3, live - 2] == 9 and sim[3, live - 2] == -1.0


@pytest.mark.gpu
def test_shortlist_thresholds_from_minus_inf_to_inf_and_a_rows_own_value(hip):
    sig, norm2 = signature_set(65)
    k = 8
    _, base_sim = nr.shortlist(sig, norm2, k)
    own = float(base_sim[20, k - 1])
    above = float(np.nextafter(np.float32(own), np.float32(2)))
    for min_sim in (-np.inf, -1.0, 0.0, own, above, 1.0, np.inf):
        msg, (nbr, sim) = fz.shortlist_both(sig, norm2, k, min_sim)
        ok(msg)
        if min_sim == own:
            assert nbr[20, k - 1] >= 0                               # the value itself passes
        if min_sim == above:
            assert (nbr[20] >= 0).sum() == (base_sim[20] > np.float32(own)).sum() < k                  # exactly the entries at that value leave
        if min_sim == 1.0:
            assert nbr[0, :2].tolist() == [2, 12] and nbr[0, 2] == -1
        if min_sim == np.inf:
            assert (nbr == -1).all() and np.isneginf(sim).all()


@pytest.mark.gpu
def test_shortlist_products_at_plus_and_minus_the_largest_sum(hip):
    sig = np.full((5, 256 * 128), 127, np.int8)
    sig[1], sig[3] = -127, -127
    sig[4, ::2] = -127                                               # orthogonal to all others: S = 0
    norm2 = np.full(5, MAX_NORM2, np.int32)
    S, sim = nr.similarities(sig, norm2)
    assert S[0, 2] == MAX_NORM2 and S[0, 1] == -MAX_NORM2 and S[0, 4] == 0
    msg, (nbr, nsim) = fz.shortlist_both(sig, norm2, 4, None)
    ok(msg)
    assert nbr[0].tolist() == [2, 4, 1, 3] and nsim[0].tolist() == [1.0, 0.0, -1.0, -1.0]


# ---- pairs --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("mutual", [False, True])
def test_pairs_union_and_mutual_at_every_capacity(hip, mutual):
    sig, norm2 = signature_set(65)
    nbr, _ = nr.shortlist(sig, norm2, 5)
    total = int(nr.pair_list(nbr, mutual)[1][0])
    assert total > 10
    for cap in (None, 0, total - 1, total, total + 7):
        msg, (pairs, count) = fz.pairs_both(nbr, mutual, cap)
        ok(msg)
        assert count.tolist() == [total, total if cap is None else min(total, cap)]
    ok(fz.pairs_both(np.full((33, 4), -1, np.int32), mutual, None)[0])                                  # nobody names anybody
    star = np.full((70, 64), -1, np.int32)                           # everybody names image 0, and image 0's list is full
    star[1:, 0] = 0
    star[0] = np.arange(1, 65)
    msg, (pairs, count) = fz.pairs_both(star, mutual, None)
    ok(msg)
    assert count[0] == (64 if mutual else 69) and (pairs[:, 0] == 0).all()
    bad = np.array([[0, 1, 1, 5, -3, 2 ** 31 - 1], [2, 2, 2, 2, 2, 2], [1, 0, 0, 0, 0, 0]], np.int32)   # self, repeated and out-of-range entries
    ok(fz.pairs_both(bad, mutual, None)[0])
    ok(fz.pairs_both(np.zeros((1, 3), np.int32), mutual, None)[0])


# ---- launch path and composition ------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_select_pairs_waits_for_the_host_exactly_once_and_the_entry_points_never(hip):
    from sfm_mvs_amd import _lib, retrieval
    sc = rc.track_case()["scene"]
    des = [dev(d) for d in sc["descs"]]
    desc = torch.cat(des).contiguous()
    img_off = dev(np.concatenate([[0], np.cumsum([len(d) for d in sc["descs"]])]).astype(np.int32))
    kw = dict(rc.TRACK_SETTING)
    want, st = rc.track_case()["pairs"], rc.track_case()["stages"]
    retrieval.select_pairs(des, **kw)                                # allocations and module loading happen here
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    waits = _lib.lib().sfm_host_sync_count()
    torch.cuda.set_sync_debug_mode("error")
    try:                                                             # the chained entry points: no wait at all
        centres = retrieval.train_vocabulary(desc, kw["n_centres"], 8, 0, retrieval.scale_of())
        _, acc, count = retrieval.assign_accumulate(desc, centres, img_off, retrieval.scale_of())
        sig, norm2 = retrieval.signatures(acc)
        nbr, nbr_sim = retrieval.shortlist(sig, norm2, kw["k"])
        pairs, cnt = retrieval.pair_list(nbr)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            got, dv = retrieval.select_pairs(des, **kw)
            again, _ = retrieval.select_pairs(desc, img_off, centres=centres, k=kw["k"])
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    syncs = [w for w in seen if "synchroniz" in str(w.message)]
    assert len(syncs) == 2, [str(w.message) for w in seen]           # one a call
    assert _lib.lib().sfm_host_sync_count() == waits                  # and the library itself never waits
    assert got == want == again
    for name, t in dict(centres=centres, sig=sig, nbr=nbr, nbr_sim=nbr_sim).items():
        ok(same(name, t, st[name]))
        ok(same(name, dv[name], st[name]))
    ok(same("count", cnt, st["pair_count"]))
    ok(same("pairs", pairs[:len(want)], st["pairs"]))


@pytest.mark.gpu
def test_k_of_everybody_is_all_pairs_of_the_images_with_descriptors(hip):
    from sfm_mvs_amd import retrieval, sharded
    sc = rc.corridor_scene(7, 40, 5, 5, 1)
    des = [dev(d) for d in sc["descs"]]
    got, _ = retrieval.select_pairs(des, k=6, n_centres=4, iters=2)
    assert set(got) == set(sharded.all_pairs(7)) and got == sorted(got)
    des[2] = des[2][:0]
    got, _ = retrieval.select_pairs(des, k=6, n_centres=4, iters=2)
    assert set(got) == set((a, b) for a, b in rc.all_pairs(7) if 2 not in (a, b))


@pytest.mark.gpu
def test_shortlist_to_tracks_end_to_end_on_the_permuted_corridor(hip):
    """tracks.retrieval_pairs -> match_pairs_sharded -> run_tracks: the pair list of the restated composition, and the track count the
    restated composition plus np_tracks give; the calibrated bars come with the equality (tests/test_retrieval_cpu.py)."""
    from sfm_mvs_amd import sharded, tracks
    tc = rc.track_case()
    sc = tc["scene"]
    des, kps = [dev(d) for d in sc["descs"]], [dev(k) for k in sc["kps"]]
    pairs = tracks.retrieval_pairs(des, **rc.TRACK_SETTING)
    assert pairs == tc["pairs"] and 0 < len(pairs) < 120
    store, nq = sharded.match_pairs_sharded(des, pairs)
    res = tracks.run_tracks(store, nq, pairs, kps, sc["P"], rc.RATIO)
    print(f"{len(pairs)} of 120 pairs, {len(res['track_len'])} tracks (all pairs: {tc['tracks_all']})")
    assert len(res["track_len"]) == tc["tracks_short"] == len(tc["result_short"]["track_len"])
    row = rc.row_of(rc.load_calibration(), scene="tracks")
    assert len(res["track_len"]) / tc["tracks_all"] >= row["track_fraction"] - 0.05


# ---- fuzzing ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_a_short_fixed_seed_fuzz_run(hip):
    counts, bad, dt = fz.run(4.0, 20264, log=print)
    print(f"fuzz_retrieval: {sum(counts.values())} cases {counts} in {dt:.1f} s")
    assert bad == 0 and sum(counts.values()) >= 100              # about 150 cases a second in the committed logs: every family is drawn


@pytest.mark.gpu
def test_committed_fuzz_logs_are_clean_and_of_this_code(hip):
    """profiles/retrieval_fuzz_seed*.log: no mismatch, and run on the code of csrc/retrieval.hip and csrc/common.h that the loaded library
    was built from (scripts/knn_code_hash.py: comments and whitespace do not count)."""
    import glob
    import re
    from sfm_mvs_amd import _lib
    have = _lib.code_hashes_of_binary()
    logs = sorted(glob.glob(os.path.join(ROOT, "profiles", "retrieval_fuzz_seed*.log")))
    assert len(logs) >= 2, logs
    total = 0
    for path in logs:
        text = open(path).read()
        m = re.search(r"fuzz_retrieval: seed \d+, (\d+) cases .*?, (\d+) mismatches", text)
        assert m and int(m.group(2)) == 0, f"{path}: no clean summary line"
        ids = re.findall(r"sfm_build_id (knn\.hip:\S+(?: \S+:\S+)*)", text)
        assert ids, f"{path} does not name the build it ran on"
        logged = dict(tok.split(":", 1) for tok in ids[-1].split() if ":" in tok)
        for name in ("retrieval.hip", "common.h"):
            assert logged.get(name) == have[name], f"{path} was produced by another csrc/{name} than the loaded binary's"
        total += int(m.group(1))
    assert total >= FUZZ_FLOOR, total
