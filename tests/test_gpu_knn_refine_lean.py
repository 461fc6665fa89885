"""refine_q8_body (pairs quantised for the integer body, stats[3] = 5) after three instruction cuts, on the inputs where each of them
could go wrong.  Everything is compared bit for bit with the oracle (`orc_knn2_l2_f32` = cv2.BFMatcher().knnMatch(k=2), then the
Lowe ratio), and `stats[3]` names the body that ran.

  * The float32 row passes load unconditionally: a lane quad without a row reads row 0 of T and its sum is dropped.  Shapes with
    fewer than two train rows, dead query slots in a wave and 0 .. 5 float32 rows per query give passes with 0 .. 3 idle quads;
    strided views with a storage offset make row 0 something else than the allocation's start; the per-query passes
    (`sfm_debug_knn_refine_pooled(0)`) flush the row list from another place than the pooled ones.
  * 1 / s, eta / s, sqrt(te) and the absolute term of the slack come from `minfo`, written per pair by knn_split_images_kernel:
    batches whose pairs have different grids (u8 pairs with s = 1 among them, steps of 1e-12 and 1e+12, a batch that is repaired)
    must return, pair by pair, what the single-pair call returns.
  * U, al and dlow are 32-bit integers: queries at one end of the value range against trains at the other (the largest D there
    is, 128 * 255^2 on u8 values), D = 0 throughout, exact ties.
  * The rescan's row list goes through the same unconditional loads: an all-equal train set in ONE filter workgroup."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RATIO = 0.70
f32 = np.float32


def uniform(rng, n, lo=0.0, width=1.0):
    return (lo + width * rng.random((n, 128))).astype(f32)


def both_ways(fn):
    """fn() as released (pooled integer passes), then fn() with the per-query passes; the switch is on again afterwards."""
    from sfm_mvs_amd import _lib
    L = _lib.lib()
    pooled = fn()
    try:
        assert L.sfm_debug_knn_refine_pooled(0) == 0
        per_query = fn()
    finally:
        L.sfm_debug_knn_refine_pooled(1)
    return pooled, per_query


def strided(x):
    """x on the device as a view with row stride 160 and a storage offset: its row 0 is not where the allocation starts."""
    wide = torch.zeros((x.shape[0] + 3, 160), dtype=torch.float32, device="cuda")
    view = wide[3:, 16:144]
    view.copy_(torch.from_numpy(x))
    assert view.stride(0) == 160 and view.storage_offset() == 3 * 160 + 16 and view.data_ptr() % 16 == 0
    return view


def contiguous(x):
    return torch.from_numpy(x).cuda()


def run_pair(hip, dq, dt):
    pm = hip.PairMatcher(dq.shape[0], dt.shape[0], "cuda", ratio=RATIO)
    idx, dist, oq, ot, cnt = pm.run(dq, dt)
    torch.cuda.synchronize()
    m = int(cnt.item())
    return (idx.cpu().numpy().copy(), dist.cpu().numpy().view(np.uint32).copy(), m, oq[:m].cpu().numpy().copy(), ot[:m].cpu().numpy().copy(),
            pm.stats.cpu().numpy().copy())


def want_of(oracle, q, t):
    wi, wd = oracle.knn2(np.ascontiguousarray(q), np.ascontiguousarray(t), nthreads=8)
    wq, wt, _ = oracle.ratio_filter(wi, wd, RATIO)
    return wi, wd.view(np.uint32), wq, wt


def assert_is(got, want, mode, what):
    gi, gd, m, oq, ot, st = got
    wi, wd, wq, wt = want
    assert st[3] == mode, f"{what}: filter arithmetic {st[3]}, expected {mode}"
    bad = np.flatnonzero((gi != wi).any(1))
    assert bad.size == 0, f"{what}: queries {bad[:8].tolist()} got {gi[bad[:8]].tolist()}, oracle {wi[bad[:8]].tolist()}"
    assert np.array_equal(gd, wd), f"{what}: distance bits differ from the oracle's"
    assert m == len(wq) and np.array_equal(oq, wq) and np.array_equal(ot, wt), f"{what}: Lowe list"


def check_pair(hip, oracle, q, t, place=contiguous, mode=5):
    """One pair, pooled and per-query passes, against the oracle; returns the released run."""
    dq, dt = place(q), place(t)
    want = want_of(oracle, q, t)
    pooled, per_query = both_ways(lambda: run_pair(hip, dq, dt))
    assert_is(pooled, want, mode, "pooled")
    assert_is(per_query, want, mode, "per query")
    for a, b in zip(pooled, per_query):
        assert np.array_equal(a, b)
    return pooled


def run_batch(hip, dev, nq, nt):
    bm = hip.BatchMatcher(nq, nt, "cuda", ratio=RATIO, batch=len(dev))
    bm.run(dev)
    torch.cuda.synchronize()
    cnt = bm.count.cpu().numpy()[:, 0].copy()
    return [(bm.idx[b].cpu().numpy().copy(), bm.dist[b].cpu().numpy().view(np.uint32).copy(), int(cnt[b]), bm.out_q[b, :int(cnt[b])].cpu().numpy().copy(),
             bm.out_t[b, :int(cnt[b])].cpu().numpy().copy(), bm.stats[b].cpu().numpy().copy()) for b in range(len(dev))]


def check_batch(hip, oracle, pairs, mode, single_modes=None):
    """Every pair of the batch equals the oracle AND its own single-pair call, with the pooled and with the per-query passes."""
    nq, nt = pairs[0][0].shape[0], pairs[0][1].shape[0]
    dev = [(contiguous(q), contiguous(t)) for q, t in pairs]
    want = [want_of(oracle, q, t) for q, t in pairs]
    pooled, per_query = both_ways(lambda: run_batch(hip, dev, nq, nt))
    for name, res in (("pooled", pooled), ("per query", per_query)):
        assert res[0][5][3] == mode, f"{name}: filter arithmetic {res[0][5][3]}, expected {mode}"
        for b in range(len(pairs)):
            assert_is(res[b][:5] + (res[0][5],), want[b], mode, f"{name}, pair {b}")
    for b, (dq, dt) in enumerate(dev):
        single = run_pair(hip, dq, dt)
        if single_modes is not None:
            assert single[5][3] == single_modes[b], f"pair {b} alone: filter arithmetic {single[5][3]}, expected {single_modes[b]}"
        for x, y in zip(single[:5], pooled[b][:5]):
            assert np.array_equal(x, y), f"pair {b}: the batched result differs from the single-pair call's"


# ---------------------------------------------------------------------------------------------- idle quads, the row-0 read
def idle_case(nq, nt):
    rng = np.random.default_rng(1000 * nq + nt)
    return uniform(rng, nq), uniform(rng, nt)


@pytest.mark.parametrize("place", [contiguous, strided], ids=["contiguous", "ld160_offset"])
@pytest.mark.parametrize("nt", [1, 2, 3, 5, 33])
@pytest.mark.parametrize("nq", [1, 15, 17, 40])
def test_idle_quads_read_row_zero_and_drop_it(hip, oracle, nq, nt, place):
    """nt rows at most reach a query's float32 list: a pass of four quads holds nt % 4 real rows in its last trip (nt = 1: the second
    index stays -1, the second distance +inf); nq = 1, 15, 17 leave dead query slots in the last wave."""
    q, t = idle_case(nq, nt)
    gi, gd, m, _, _, _ = check_pair(hip, oracle, q, t, place)
    if nt == 1:
        assert (gi[:, 0] == 0).all() and (gi[:, 1] == -1).all() and (gd[:, 1] == np.array([np.inf], f32).view(np.uint32)[0]).all() and m == 0


# ---------------------------------------------------------------------------------------------- per-pair constants from minfo
NQ_B, NT_B = 100, 257


def grids_case():
    rng = np.random.default_rng(21)
    return [(uniform(rng, NQ_B, lo, w), uniform(rng, NT_B, lo, w)) for lo, w in ((0.0, 1.0), (-3.0, 8.0), (100.0, 0.5))]


def u8_pair(rng, nq, nt):
    from datagen import sift_like
    q, t = sift_like(rng, nq), sift_like(rng, nt)
    t[rng.permutation(nt)[:nq // 3]] = q[rng.permutation(nq)[:nq // 3]]
    return q, t


def mixed_u8_case():
    rng = np.random.default_rng(22)
    return [(uniform(rng, NQ_B), uniform(rng, NT_B)), u8_pair(rng, NQ_B, NT_B), (uniform(rng, NQ_B, -1.0, 2.0), uniform(rng, NT_B, -1.0, 2.0))]


def extreme_steps_case():
    """s = width / 255 ~ 1.2e-12 (the rule admits s >= 1e-12) and ~ 1e+12, beside a pair with s ~ 4e-3."""
    rng = np.random.default_rng(23)
    return [(uniform(rng, NQ_B, 0.0, 3.1e-10), uniform(rng, NT_B, 0.0, 3.1e-10)), (uniform(rng, NQ_B), uniform(rng, NT_B)),
            (uniform(rng, NQ_B, 0.0, 2.55e14), uniform(rng, NT_B, 0.0, 2.55e14))]


def test_three_grids_in_one_batch(hip, oracle):
    """Uniform on [0, 1), [-3, 5) and [100, 100.5): three steps, three offsets, three absolute terms (the last one's is 0.07 s)."""
    check_batch(hip, oracle, grids_case(), 5, (5, 5, 5))


def test_u8_pair_inside_a_quantised_batch(hip, oracle):
    """The u8 pair's words are those of s = 1, lo = 0 (alone it runs the exact-integer body, stats[3] = 4)."""
    check_batch(hip, oracle, mixed_u8_case(), 5, (5, 4, 5))


def test_steps_of_1e_minus_12_and_1e_plus_12(hip, oracle):
    check_batch(hip, oracle, extreme_steps_case(), 5, (5, 5, 5))
    for q, t in extreme_steps_case()[::2]:
        check_pair(hip, oracle, q, t)


NQ_R, NT_R = 300, 1000


def clipped_pair(rng):
    """tests/test_gpu_knn_q8.py's construction: outliers in train rows the grid's sample (rows k * nt / 16) does not read — the grid is
    taken, the MEASURED residual rejects it, the pair is repaired."""
    q, t = uniform(rng, NQ_R), uniform(rng, NT_R)
    sampled = {(k * NT_R) >> 4 for k in range(16)}
    rows = [r for r in range(5, 900, 7) if r not in sampled]
    t[rows, 3] = 9.0
    return q, t


def repaired_cases():
    rng = np.random.default_rng(24)
    gauss = lambda: (rng.standard_normal((NQ_R, 128)).astype(f32), rng.standard_normal((NT_R, 128)).astype(f32))
    uni = lambda: (uniform(rng, NQ_R), uniform(rng, NT_R))
    return {"clipped_beside_two_uniform": ([uni(), clipped_pair(rng), uni()], (5, 1, 5)),
            "uniform_beside_two_gaussian": ([gauss(), uni(), gauss()], (1, 5, 1))}


@pytest.mark.parametrize("name", ["clipped_beside_two_uniform", "uniform_beside_two_gaussian"])
def test_batch_that_is_repaired(hip, oracle, name):
    """One pair does not fit the integer body: the whole batch runs the fp16 body (stats[3] = 1) and the pairs quantised in vain are
    repaired — the words of the quantised body are written all the same, and nobody reads them."""
    pairs, single_modes = repaired_cases()[name]
    check_batch(hip, oracle, pairs, 1, single_modes)


# ---------------------------------------------------------------------------------------------- 32-bit U, al, dlow
NQ_E, NT_E = 40, 70


def ends_case(flip):
    rng = np.random.default_rng(31 + flip)
    hi, lo = uniform(rng, NQ_E if not flip else NT_E, 0.9, 0.1), uniform(rng, NT_E if not flip else NQ_E, 0.0, 0.1)
    return (lo, hi) if flip else (hi, lo)


def u8_ends_case(flip):
    """u8 values 254, 255 against 0, 1: D up to 128 * 255^2 = 8 323 200 < 2^23, the largest there is."""
    rng = np.random.default_rng(33 + flip)
    hi = rng.integers(254, 256, (NT_B if flip else NQ_B, 128)).astype(f32)
    lo = rng.integers(0, 2, (NQ_B if flip else NT_B, 128)).astype(f32)
    return (lo, hi) if flip else (hi, lo)


@pytest.mark.parametrize("flip", [0, 1], ids=["q_high_t_low", "q_low_t_high"])
def test_opposite_ends_of_the_range(hip, oracle, flip):
    q, t = ends_case(flip)
    check_pair(hip, oracle, q, t)


@pytest.mark.parametrize("flip", [0, 1], ids=["q_255_t_0", "q_0_t_255"])
def test_opposite_ends_of_the_u8_range_in_a_quantised_batch(hip, oracle, flip):
    rng = np.random.default_rng(35 + flip)
    check_batch(hip, oracle, [(uniform(rng, NQ_B), uniform(rng, NT_B)), u8_ends_case(flip)], 5, (5, 4))


def all_equal_case():
    rng = np.random.default_rng(36)
    row = uniform(rng, 1)
    return np.repeat(row, NQ_E, axis=0), np.repeat(row, NT_E, axis=0)


def test_all_equal_rows_equal_to_the_queries(hip, oracle):
    """D = 0 and U = 1 for every row; every distance is 0 and the answer is rows 0 and 1, which only the rescan can know."""
    q, t = all_equal_case()
    gi, gd, _, _, _, st = check_pair(hip, oracle, q, t)
    assert (gi == [0, 1]).all() and (gd == 0).all()


def duplicates_case():
    rng = np.random.default_rng(37)
    q, t = uniform(rng, NQ_E), uniform(rng, NT_E)
    t[3] = q[0] + f32(1e-3) * uniform(rng, 1)[0]               # query 0's nearest neighbour ...
    t[50] = t[3]; t[17] = t[3]; t[69] = t[3]                     # ... three more times: ties by index
    t[40] = q[1]; t[8] = q[1]                                    # distance 0 twice
    return q, t


def test_exact_duplicates_of_the_nearest_neighbour(hip, oracle):
    q, t = duplicates_case()
    gi, _, _, _, _, _ = check_pair(hip, oracle, q, t)
    assert gi[0].tolist() == [3, 17] and gi[1].tolist() == [8, 40]


# ---------------------------------------------------------------------------------------------- the rescan's row list
def rescan_case():
    rng = np.random.default_rng(38)
    return uniform(rng, 17), np.repeat(uniform(rng, 1), 70, axis=0)


def test_rescan_of_an_all_equal_train_set_in_one_workgroup(hip, oracle):
    """70 equal rows (three tiles, one substream) in ONE filter workgroup: every stream's third key ties with the answer, no stream
    is certified, and every query's rows come from the rescan's list, 64 to a trip, through the unconditional loads."""
    q, t = rescan_case()
    try:
        hip.debug_knn_filter_workgroups(1)
        gi, gd, _, _, _, st = check_pair(hip, oracle, q, t)
    finally:
        hip.debug_knn_filter_workgroups(0)
    assert st[1] == 1, f"{st[1]} filter workgroups ran, the hook asked for 1"
    assert st[0] == len(q), f"{st[0]} of {len(q)} queries rescanned"
    assert (gi == [0, 1]).all()
