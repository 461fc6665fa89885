"""The GUIDED family on the device (sfm_guided_match / sfm_guided_mutual, guided.guided_pairs, tracks.guided_keep): every output word equal
to the restatement tests/np_guided.py, floats as integer views, outputs in front of sentinel words (include/sfm_hip.h, "GUIDED";
docs/tracks.md §14)."""
import functools
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

import fuzz_guided as fz  # noqa: E402
import guided_cases as gc  # noqa: E402
import np_guided as ng  # noqa: E402
import np_verify as nv  # noqa: E402
from datagen import sift_like  # noqa: E402
from fuzz_guided import match_both, mutual_both  # noqa: E402
from fuzz_verify import dev, same  # noqa: E402

FUZZ_FLOOR = 4000             # a tenth of the cases the committed logs hold, rounded down to one figure (docs/tracks.md §14.6)
N_QUERY = (0, 1, 63, 64, 65, 255, 256, 257)
N_TRAIN = (0, 1, 2, 7, 255, 256, 257, 513)


@functools.lru_cache(maxsize=None)
def star(n_query, seed=3):
    """Image 0 with n_query keypoints and one train image of every size of N_TRAIN: eight pairs (0, j), an essential matrix each.
    Computed once, never changed (copy before editing)."""
    rng = np.random.default_rng([seed, n_query])
    sizes = np.array((n_query,) + N_TRAIN)
    n = int(sizes.sum())
    desc = sift_like(rng, n)
    desc[rng.integers(n, size=n // 8)] = desc[rng.integers(n, size=n // 8)]               # some equal rows
    pairs = np.array([(0, j) for j in range(1, len(sizes))], np.int32)
    return dict(desc=desc, xn=rng.uniform(-0.6, 0.6, (n, 2)), E=np.stack([fz.random_E(rng) for _ in pairs]), active=np.ones(len(pairs), np.uint8),
                nq=np.full(len(pairs), n_query, np.int32), pairs=pairs, img_off=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32),
                cap=n_query, stride=int(max(N_TRAIN)), thr2g=np.inf)


def quotients(c, p):
    """The float32 band values of pair p, [qb, nt]."""
    qb, nt, oa, ob = ng.extent(p, c["nq"], c["pairs"], c["img_off"].astype(np.int64), len(c["img_off"]) - 1, c["cap"], c["stride"])
    return ng.quotient(c["E"][p], c["xn"][oa:oa + qb], c["xn"][ob:ob + nt])


def both(c, **over):
    """match and mutual against the restatement -> (store_g, rev, keep_g, info_g) of the restatement."""
    c = dict(c, **over)
    msg, store, rev = match_both(c)
    assert not msg, msg
    msg = mutual_both(store, rev, c)
    assert not msg, msg
    return (store, rev) + ng.guided_mutual(store, rev, c["nq"], c["pairs"], c["img_off"])


# ---- shapes -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("n_query", N_QUERY)
def test_every_shape_around_the_wave_and_the_tile_at_three_band_widths(hip, n_query):
    """n_query x every n_train of N_TRAIN in one launch: a band that admits everything (queue overflow and drain at 257 x 513), a band of
    about five per cent and one of about half a per cent."""
    c = star(n_query)
    store, rev, keep, info = both(c)
    for p, nt in enumerate(N_TRAIN):                                 # a band of everything: exactly min(nt, 2) neighbours per query
        assert info[p].tolist()[:3] == [n_query, n_query if nt >= 1 else 0, n_query if nt >= 2 else 0]
        assert (rev[p, :nt] != ng.NO_KEY).all() == (n_query > 0 or nt == 0) and (rev[p, nt:] == ng.NO_KEY).all()
    if n_query:
        v = np.sort(quotients(c, 7).ravel())
        for share in (0.05, 0.005):
            store, _, _, info = both(c, thr2g=float(v[int(share * len(v))]))
            assert 0 < info[7, 1] <= n_query


@pytest.mark.gpu
def test_a_band_of_everything_is_the_knn_store_bit_for_bit(hip):
    """Consequence 1 against `ops.knn2` at 257 x 513 and 65 x 7."""
    c = star(257)
    store = both(c)[0]
    desc, off = dev(c["desc"]), c["img_off"]
    for p in (7, 3):
        j = p + 1
        idx, dist = hip.knn2(desc[:257].contiguous(), desc[off[j]:off[j + 1]].contiguous())
        assert np.array_equal(store[p, 0], idx.cpu().numpy()) and np.array_equal(store[p, 1], dist.cpu().numpy().view(np.int32))


@pytest.mark.gpu
def test_thresholds_of_zero_minus_one_one_pairs_own_value_and_the_float_below(hip):
    c = star(65)
    v = quotients(c, 7)
    flat = np.sort(v.ravel())
    own = flat[len(flat) // 50]
    below = np.nextafter(own, np.float32(-1))
    assert below < own
    n_at = both(c, thr2g=float(own))[0]
    n_below = both(c, thr2g=float(below))[0]
    # the value itself is in the band, the float below it leaves exactly the pairs with that value out
    q_own = np.flatnonzero((v == own).any(1))
    assert len(q_own) >= 1
    cnt = lambda s, q: int((s[7, 0, q] >= 0).sum())                  # noqa: E731
    for q in q_own:
        k_at, k_below = min(int((v[q] <= own).sum()), 2), min(int((v[q] <= below).sum()), 2)
        assert cnt(n_at, q) == k_at and cnt(n_below, q) == k_below
    for thr in (0.0, -1.0):
        store = both(c, thr2g=thr)[0]
        assert (store[:, 0] == -1).all() and (store[:, 1] == ng.INF_BITS).all()
    xn = c["xn"].copy()                                              # a keypoint ON the epipolar line of query 0: s = 0 exactly, in the band at 0
    E = c["E"].copy()
    E[7] = [0, 0, 0, 0, 0, -1, 0, 1, 0]                              # a pure sideways translation: the line of (a1, b1) is b2 = b1
    xn[c["img_off"][8] + 5, 1] = xn[0, 1]
    store = both(c, xn=xn, E=E, thr2g=0.0)[0]
    assert store[7, 0, 0].tolist() == [5, -1]


@pytest.mark.gpu
def test_bands_of_exactly_zero_one_and_two_candidates(hip):
    c = star(64)
    store = both(c)[0]
    for p, nt in ((0, 0), (1, 1), (2, 2)):
        assert ((store[p, 0] >= 0).sum(1) == nt).all()
        assert ((store[p, 1].view(np.float32) < np.inf).sum(1) == nt).all()
    E = c["E"].copy()
    E[7] = [0, 0, 0, 0, 0, -1, 0, 1, 0]
    xn = c["xn"].copy()
    t0 = c["img_off"][8]
    xn[t0:t0 + 513, 1] = 5.0                                         # off every line ...
    xn[:64, 1] = np.arange(64) * 0.01
    xn[t0 + 100:t0 + 132, 1] = np.arange(32) * 0.01                  # ... but one keypoint on the lines of queries 0..31
    xn[t0 + 300:t0 + 316, 1] = np.arange(16) * 0.01                  # and a second on those of queries 0..15
    store, rev, keep, info = both(c, xn=xn, E=E, thr2g=1e-12)
    got = (store[7, 0] >= 0).sum(1)
    assert got[:16].tolist() == [2] * 16 and got[16:32].tolist() == [1] * 16 and not got[32:].any() and info[7].tolist()[1:3] == [32, 16]


@pytest.mark.gpu
def test_duplicate_rows_resolve_by_the_lowest_index_on_both_sides(hip):
    c = star(65)
    desc = c["desc"].copy()
    t0 = c["img_off"][8]
    desc[t0:t0 + 513] = desc[t0]                                     # equal train rows: the lowest t wins both slots in order
    store, rev, keep, _ = both(c, desc=desc)
    assert (store[7, 0] == [0, 1]).all() and (store[7, 1, :, 0] == store[7, 1, :, 1]).all()
    desc = c["desc"].copy()
    desc[:65] = desc[0]                                              # equal query rows: rev keeps the lowest q
    store, rev, keep, info = both(c, desc=desc)
    assert ((rev[7, :513] & np.uint64(ng.M32)) == 0).all() and keep[7, 0] == 1 and not keep[7, 1:].any() and info[7, 3] == 1


@pytest.mark.gpu
def test_descriptor_values_the_float32_sums_lose(hip):
    c = star(65)
    desc = c["desc"].copy()
    t0 = c["img_off"][8]
    desc[3, 7] = np.nan                                              # a query row
    desc[t0 + 2, 100] = np.nan
    desc[t0 + 4, 0] = np.inf
    desc[t0 + 6, 127] = 1e30                                         # the square overflows
    desc[t0 + 8, 64] = 1e18                                          # the square is finite
    desc[5, 64] = -1e18
    store, rev, _, info = both(c, desc=desc)
    assert store[7, 0, 3].tolist() == [-1, -1] and (rev[7, [2, 4, 6]] == ng.NO_KEY).all() and rev[7, 8] != ng.NO_KEY
    assert not np.isin(store[7, 0], [2, 4, 6]).any() and info[7, 1] == 64


@pytest.mark.gpu
@pytest.mark.parametrize("value", [0.0, np.nan, 1e150, np.inf])
def test_an_essential_matrix_without_a_band(hip, value):
    c = star(65)
    E = c["E"].copy()
    E[7] = value
    E[6, 4] = value if value != 0.0 else E[6, 4]
    store, rev, keep, info = both(c, E=E, thr2g=1e-3)
    if value == 1e150:                                               # squares of 1e300: finite, and the quotient does not depend on the scale of E
        assert info[7, 1] > 0
    else:                                                            # 0 / 0 and inf / inf: a NaN quotient, no band
        assert (store[7, 0] == -1).all() and (rev[7] == ng.NO_KEY).all() and not keep[7].any() and info[7].tolist() == [65, 0, 0, 0]
    both(c, E=E)                                                     # and at a threshold of +inf: a NaN quotient stays out
    both(c, E=E * 1e10 if value == 1e150 else E)                     # 1e160: the squares overflow


@pytest.mark.gpu
def test_pairs_without_a_band_empty_images_no_pairs_and_caps_on_both_sides(hip):
    c = star(65)
    pairs = c["pairs"].copy()
    pairs[0], pairs[1], pairs[2], pairs[3] = (8, 8), (0, 9), (-1, 8), (2 ** 31 - 1, 8)
    active = c["active"].copy()
    active[7] = 0
    store, rev, keep, info = both(c, pairs=pairs, active=active)
    assert (store[[0, 1, 2, 3, 7], 0] == -1).all() and info[:4, 0].tolist() == [0, 0, 0, 0] and info[7].tolist() == [65, 0, 0, 0]
    assert (store[4:7, 0, :, 0] >= 0).all()
    pairs = np.array([(1, 0), (1, 8), (8, 1), (8, 0)], np.int32)      # image 1 is empty: as query image and as train image
    both(c, pairs=pairs, E=c["E"][:4], active=c["active"][:4], nq=np.array([5, 5, 513, 513], np.int32), cap=513)
    for cap in (0, 1, 64, 66, 300):                                  # below and above the 65 queries
        store, _, _, info = both(c, cap=cap)
        assert info[7, 0] == min(cap, 65) and (store[7, 0, 65:] == -1).all()
    for nq in (-1, 0, 1, 64, 70, 2 ** 31 - 1):
        assert both(c, nq=np.full(8, nq, np.int32))[3][7, 0] == min(max(nq, 0), 65)
    for stride in (0, 1, 256, 512, 600):                             # rev shorter and longer than the largest image
        both(c, stride=stride)
    none = dict(pairs=c["pairs"][:0], E=c["E"][:0], active=c["active"][:0], nq=c["nq"][:0])
    both(c, **none)
    both(c, desc=c["desc"][:0], xn=c["xn"][:0], img_off=np.zeros(10, np.int32))                     # no keypoint at all


# ---- composition ------------------------------------------------------------------------------------------------------------------

def small_scene():
    return gc.case(4, 500, 0.5, 1)


@pytest.mark.gpu
def test_guided_pairs_in_chunks_twice_and_without_a_host_wait(hip):
    from sfm_mvs_amd import _lib, guided, verify
    sc = small_scene()
    K = sc["K"]
    a = (dev(sc["nq"]), dev(sc["pairs"]), dev(sc["img_off"]), dev(sc["kp"]), K)
    first_np = nv.verify_pairs(sc["store"], sc["nq"], sc["pairs"], sc["img_off"], sc["kp"], K, gc.RATIO, budget=64, seed=5)
    first = verify.verify_pairs(dev(sc["store"]), *a, gc.RATIO, budget=64, seed=5)
    assert not same("E", first["E"], first_np["E"]) and not same("info", first["info"], first_np["info"])
    desc = dev(sc["desc"])
    want = ng.guided_pairs(sc["desc"], sc["nq"], sc["pairs"], sc["img_off"], sc["kp"], K, first_np["E"], first_np["info"],
                           guided.DEFAULT_GUIDED_THRESHOLD, guided.DEFAULT_MIN_INLIERS)
    kw = dict(cap=500, max_size=500)
    guided.guided_pairs(desc, *a, first["E"], first["info"], **kw)   # allocations and module loading happen here
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    waits = _lib.lib().sfm_host_sync_count()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = guided.guided_pairs(desc, *a, first["E"], first["info"], **kw)
        again = guided.guided_pairs(desc, *a, first["E"], first["info"], **kw)
        ones = guided.guided_pairs(desc, *a, first["E"], first["info"], max_rev_bytes=1, **kw)          # one pair a chunk
        threes = guided.guided_pairs(desc, *a, first["E"], first["info"], max_rev_bytes=3 * 500 * 8, **kw)
        loose = guided.guided_pairs(desc, *a, first["E"], first["info"], mutual=False, **kw)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert _lib.lib().sfm_host_sync_count() == waits
    for name in ("store", "keep", "info"):
        for out in (got, again, ones, threes):
            msg = same(name, out[name], want[name])
            assert not msg, msg
        assert torch.equal(got[name], again[name])                   # a second run gives the same bits
    assert loose["keep"] is None and loose["info"] is None and torch.equal(loose["store"], got["store"])
    active = (first["info"][:, 2] >= guided.DEFAULT_MIN_INLIERS).to(torch.uint8)                        # the launch alone, rev left to the wrapper
    alone, rev = guided.guided_match(desc, verify.normalise_keypoints(a[3], K), first["E"], active, a[0], a[1], a[2], 500,
                                     verify.thr2_of(K, guided.DEFAULT_GUIDED_THRESHOLD))
    assert torch.equal(alone, got["store"]) and tuple(rev.shape) == (len(sc["pairs"]), len(sc["kp"]))
    assert torch.equal(guided.guided_pairs(desc, *a, first["E"], first["info"])["store"], got["store"])  # cap and max_size read from img_off
    off = guided.guided_pairs(desc, *a, first["E"], first["info"], min_inliers=10 ** 6, **kw)           # no pair is active
    assert (off["store"][:, 0] == -1).all() and not off["keep"].any() and off["info"][:, 1:].sum() == 0
    assert want["info"][:, 3].sum() > 300 and guided.workspace_bytes(3, 500) == 3 * 500 * 8 + 3


@pytest.mark.gpu
def test_a_verified_query_keeps_its_match_on_the_device(hip):
    """Consequence 2 against the device's `verify_pairs`, at the verification's own threshold and above it."""
    from test_guided_cpu import check_consequence_2
    from sfm_mvs_amd import guided, verify
    sc = small_scene()
    a = (dev(sc["nq"]), dev(sc["pairs"]), dev(sc["img_off"]), dev(sc["kp"]), sc["K"])
    first = verify.verify_pairs(dev(sc["store"]), *a, gc.RATIO, budget=64, seed=5)
    keep = first["keep"].cpu().numpy()
    assert keep.sum() > 300
    for mult in (1, 2, 8):
        g = guided.guided_pairs(dev(sc["desc"]), *a, first["E"], first["info"], threshold=mult * 0.4, cap=500, max_size=500)
        kept, with_second = check_consequence_2(sc["store"], g["store"].cpu().numpy(), keep)
        print(f"x{mult}: {kept} verified queries, {with_second} with a second neighbour in the band")
        assert kept == keep.sum()


@pytest.mark.gpu
def test_guided_keep_is_the_restated_composition_and_gives_more_full_length_tracks(hip):
    """The ring of six images with twins of the calibration table through `tracks.guided_keep` and `tracks.run_tracks`."""
    from sfm_mvs_amd import guided, tracks
    n, m, tw, s = gc.TRACK_SCENE
    sc = gc.case(n, m, tw, s)
    kw = dict(budget=gc.BUDGET, seed=s)
    want_store, want_keep, st = ng.guided_keep(sc["desc"], sc["store"], sc["nq"], sc["pairs"], sc["img_off"], sc["kp"], sc["K"], gc.RATIO,
                                               guided_threshold=guided.DEFAULT_GUIDED_THRESHOLD, min_inliers=guided.DEFAULT_MIN_INLIERS, stages=True, **kw)
    kps, store = [dev(k) for k in sc["kps"]], dev(sc["store"])
    got_store, got_keep = tracks.guided_keep([dev(d) for d in sc["descs"]], store, sc["nq"], sc["pairs"], kps, sc["K"], gc.RATIO, **kw)
    msg = same("store_g", got_store, want_store) or same("keep", got_keep, want_keep)
    assert not msg, msg
    plain_keep = tracks.verify_keep(store, sc["nq"], sc["pairs"], kps, sc["K"], gc.RATIO, batched=True, **kw)
    assert not same("plain keep", plain_keep, st["first"]["keep"])
    full = lambda res: int((res["track_len"] == n).sum())            # noqa: E731
    plain = full(tracks.run_tracks(store, sc["nq"], sc["pairs"], kps, sc["P"], gc.RATIO, keep=plain_keep))
    guided_n = full(tracks.run_tracks(got_store, sc["nq"], sc["pairs"], kps, sc["P"], gc.RATIO, keep=got_keep))
    table = gc.load_calibration()
    where = dict(images=n, m=m, twin=tw, seed=s)
    name = gc.setting_name(round(guided.DEFAULT_GUIDED_THRESHOLD / guided.DEFAULT_THRESHOLD), True)
    print(f"full-length tracks: plain {plain}, guided {guided_n}")
    assert plain == gc.totals(table, "plain", "tracks", **where) and guided_n == gc.totals(table, name, "tracks", **where)
    assert guided_n > plain


# ---- fuzzing ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_a_short_fixed_seed_fuzz_run(hip):
    counts, bad, dt = fz.run(4.0, 20263, log=print)
    print(f"fuzz_guided: {sum(counts.values())} cases {counts} in {dt:.1f} s")
    assert bad == 0 and sum(counts.values()) >= 3


@pytest.mark.gpu
def test_committed_fuzz_logs_are_clean_and_of_this_code(hip):
    """profiles/guided_fuzz_seed*.log: no mismatch, and run on the code of csrc/guided.hip and csrc/common.h that the loaded library was
    built from (scripts/knn_code_hash.py: comments and whitespace do not count)."""
    import glob
    import re
    from sfm_mvs_amd import _lib
    have = _lib.code_hashes_of_binary()
    logs = sorted(glob.glob(os.path.join(ROOT, "profiles", "guided_fuzz_seed*.log")))
    assert len(logs) >= 2, logs
    total = 0
    for path in logs:
        text = open(path).read()
        m = re.search(r"fuzz_guided: seed \d+, (\d+) cases .*?, (\d+) mismatches", text)
        assert m and int(m.group(2)) == 0, f"{path}: no clean summary line"
        ids = re.findall(r"sfm_build_id (knn\.hip:\S+(?: \S+:\S+)*)", text)
        assert ids, f"{path} does not name the build it ran on"
        logged = dict(tok.split(":", 1) for tok in ids[-1].split() if ":" in tok)
        for name in ("guided.hip", "common.h"):
            assert logged.get(name) == have[name], f"{path} was produced by another csrc/{name} than the loaded binary's"
        total += int(m.group(1))
    assert total >= FUZZ_FLOOR, total
