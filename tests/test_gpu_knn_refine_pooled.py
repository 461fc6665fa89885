"""The pooled integer row passes of refine_q8_body (pairs quantised for the integer body, stats[3] = 5) against the per-query
passes they replace: every case runs twice — as released, and with `sfm_debug_knn_refine_pooled(0)`, which runs the per-query
passes — and both runs must return the same bits, which are the oracle's (`orc_knn2_l2_f32` = cv2.BFMatcher().knnMatch(k=2),
then the Lowe ratio).  The pooled loop deals the records of a wave's four queries to its eight 8-lane groups by the prefixes of
the four list lengths, so the shapes sit on the edges of that dealing: waves with one, two or three valid queries (the slots past
nq are the only EMPTY lists there are: a valid query always lists the records its threshold came from), lists of very unequal
length, an owner that receives every row of a pass, the row list filling up inside a pooled pass, the record list filling up
before the listing ends."""
import numpy as np
import pytest
import torch

from datagen import sift_like

pytestmark = pytest.mark.gpu

RATIO = 0.70


def uniform(rng, n):
    return rng.random((n, 128), dtype=np.float32)


def cluster(rng, centre, n, sigma=0.01):
    """n rows within a few quantisation steps (1 / 255) of `centre`, inside the data's range."""
    return np.clip(centre + rng.standard_normal((n, 128)).astype(np.float32) * np.float32(sigma), 0.0, 1.0).astype(np.float32)


def plant_twins(rng, q, t):
    """Near-twins of a third of the smaller side: Lowe-ratio survivors."""
    k = min(len(q), len(t)) // 3
    if k:
        twins = q[rng.permutation(len(q))[:k]] + (rng.standard_normal((k, 128)) * 1e-3).astype(np.float32)
        t[rng.permutation(len(t))[:k]] = np.clip(twins, 0.0, 1.0).astype(np.float32)


def both_ways(fn):
    """fn() as released (pooled passes), then fn() with the per-query passes; the switch is on again afterwards."""
    from sfm_mvs_amd import _lib
    L = _lib.lib()
    pooled = fn()
    try:
        assert L.sfm_debug_knn_refine_pooled(0) == 0
        per_query = fn()
    finally:
        L.sfm_debug_knn_refine_pooled(1)
    return pooled, per_query


def run_pair(hip, dq, dt):
    pm = hip.PairMatcher(dq.shape[0], dt.shape[0], "cuda", ratio=RATIO)
    idx, dist, oq, ot, cnt = pm.run(dq, dt)
    torch.cuda.synchronize()
    m = int(cnt.item())
    return (idx.cpu().numpy().copy(), dist.cpu().numpy().view(np.uint32).copy(), m, oq[:m].cpu().numpy().copy(), ot[:m].cpu().numpy().copy(),
            pm.stats.cpu().numpy().copy())


def check_pair(hip, oracle, q, t):
    dq, dt = torch.from_numpy(q).cuda(), torch.from_numpy(t).cuda()
    pooled, per_query = both_ways(lambda: run_pair(hip, dq, dt))
    wi, wd = oracle.knn2(q, t, nthreads=8)
    wq, wt, _ = oracle.ratio_filter(wi, wd, RATIO)
    for name, (gi, gd, m, oq, ot, st) in (("pooled", pooled), ("per query", per_query)):
        assert st[3] == 5, f"{name}: filter arithmetic {st[3]}, expected 5"
        assert np.array_equal(gi, wi), f"{name}: {(gi != wi).any(1).sum()} rows differ"
        assert np.array_equal(gd, wd.view(np.uint32)), name
        assert m == len(wq) and np.array_equal(oq, wq) and np.array_equal(ot, wt), name
    for a, b in zip(pooled, per_query):
        assert np.array_equal(a, b)                                  # (idx, dist, count, out_q, out_t, the whole stats row)
    return pooled


@pytest.mark.parametrize("nq,nt", [(1, 2), (3, 33), (5, 31), (17, 40), (63, 257), (1000, 1500)])
def test_wave_and_tile_edges(hip, oracle, nq, nt):
    """A wave with one, two or three valid queries, a partial last train tile, fewer than two train rows per record."""
    rng = np.random.default_rng(nq * 131 + nt)
    q, t = uniform(rng, nq), uniform(rng, nt)
    plant_twins(rng, q, t)
    check_pair(hip, oracle, q, t)


def cluster_tiles(nt):
    """Two whole 32-row train tiles (numbers 3 and 17) of every 32-tile substream: per (substream, half-wave) the filter keeps three
    records, and a whole tile is two 8-row records per half-wave, so all three kept records of every pair are cluster rows only."""
    return [tile for s in range((nt // 32 + 31) // 32) for tile in (32 * s + 3, 32 * s + 17) if tile < nt // 32]


def test_ties_fill_the_row_list_inside_a_pooled_pass(hip, oracle):
    """64 rows of one tight cluster, six times each, fill two whole tiles of each of six substreams; the queries sit in the same
    cluster.  The spread of the distances (a few per cent of 0.16) is below the quantisation slack (~0.03), so a query lists all
    36 records it has keys for and nearly all their 288 rows pass D <= dlim — twice the 144 rows a float32 list holds, in passes
    whose 64 rows all qualify.  Equal distances: the answer's order among the copies is the index order, as the oracle's.
    (scripts/q8_pass_model.py's formulas on this input: 36 records and 270-288 rows for every query.)"""
    rng = np.random.default_rng(7)
    nt = 6 * 1024
    centre = uniform(rng, 1)
    base = cluster(rng, centre, 64)
    t = uniform(rng, nt)
    tiles = cluster_tiles(nt)
    copies = np.tile(base, (6, 1))[rng.permutation(384)]
    for k, tile in enumerate(tiles):
        t[32 * tile:32 * tile + 32] = copies[32 * k:32 * k + 32]
    q = cluster(rng, centre, 37)
    q[::5] = base[rng.permutation(64)[:len(q[::5])]]                 # some queries ARE a train row: distance 0, six ways
    check_pair(hip, oracle, q, t)


def lopsided(rng, nq, nt):
    """Every fourth query (slot 0 of its wave) sits in one tight cluster, and so do two whole train tiles of every substream; the
    other queries and train rows are uniform, i.e. isolated."""
    centre = uniform(rng, 1)
    q, t = uniform(rng, nq), uniform(rng, nt)
    for tile in cluster_tiles(nt):
        t[32 * tile:32 * tile + 32] = cluster(rng, centre, 32)
    q[::4] = cluster(rng, centre, len(q[::4]))
    return q, t


def test_lopsided_wave(hip, oracle):
    """Eleven substreams (the last one holds one cluster tile): the cluster query of each wave has 64 records with keys, more than
    the kRecCapI8 = 56 its record list holds, so the list is evaluated and emptied before the listing ends, while its three
    neighbours list two to five.  The pooled passes after the short lists are used up belong to that query alone: it receives all
    64 rows of a pass, and its 512 qualifying rows overflow the row list several times.  (scripts/q8_pass_model.py's formulas on
    this input: 64 records and 512 rows for the cluster queries, a median of 5 records for the others.)"""
    rng = np.random.default_rng(8)
    q, t = lopsided(rng, 150, 10 * 1024 + 300)
    check_pair(hip, oracle, q, t)


@pytest.mark.parametrize("nq", [1, 18, 43])
def test_empty_lists_beside_full_ones(hip, oracle, nq):
    """The last wave holds one, two or three valid queries: the slots past nq list nothing (equal neighbouring prefixes), beside a
    cluster query that lists all six records of its one substream."""
    rng = np.random.default_rng(90 + nq)
    q, t = lopsided(rng, nq, 700)
    q[nq - 1] = q[0]                                                 # the last valid slot, next to the empty ones, is a long list too
    check_pair(hip, oracle, q, t)


@pytest.mark.parametrize("kinds", ["u", "usu", "uuuulusu"])
def test_batches(hip, oracle, kinds):
    """B = 1, 3 and 8 of shape (100, 257).  'u' uniform, 'l' lopsided, 's' a SIFT-like u8 pair inside the quantised body (s = 1,
    E ~ 0)."""
    rng = np.random.default_rng(40 + len(kinds))
    nq, nt = 100, 257
    pairs = []
    for k in kinds:
        if k == "u":
            q, t = uniform(rng, nq), uniform(rng, nt)
            plant_twins(rng, q, t)
        elif k == "l":
            q, t = lopsided(rng, nq, nt)
        else:
            q, t = sift_like(rng, nq), sift_like(rng, nt)
            t[rng.permutation(nt)[:nq // 3]] = q[rng.permutation(nq)[:nq // 3]]
        pairs.append((q, t))
    dev = [(torch.from_numpy(q).cuda(), torch.from_numpy(t).cuda()) for q, t in pairs]

    def run():
        bm = hip.BatchMatcher(nq, nt, "cuda", ratio=RATIO, batch=len(pairs))
        bm.run(dev)
        torch.cuda.synchronize()
        cnt = bm.count.cpu().numpy().copy()
        return (bm.idx.cpu().numpy().copy(), bm.dist.cpu().numpy().view(np.uint32).copy(), cnt,
                [bm.out_q[b, :int(cnt[b, 0])].cpu().numpy().copy() for b in range(len(pairs))],
                [bm.out_t[b, :int(cnt[b, 0])].cpu().numpy().copy() for b in range(len(pairs))], bm.stats.cpu().numpy().copy())

    pooled, per_query = both_ways(run)
    want = []
    for q, t in pairs:
        wi, wd = oracle.knn2(q, t, nthreads=8)
        want.append((wi, wd, oracle.ratio_filter(wi, wd, RATIO)))
    for name, (gi, gd, cnt, oq, ot, st) in (("pooled", pooled), ("per query", per_query)):
        assert st[0, 3] == 5, (name, st.tolist())
        for b, (wi, wd, (wq, wt, _)) in enumerate(want):
            assert np.array_equal(gi[b], wi) and np.array_equal(gd[b], wd.view(np.uint32)), (name, kinds, b)
            assert int(cnt[b, 0]) == len(wq) and np.array_equal(oq[b], wq) and np.array_equal(ot[b], wt), (name, kinds, b)
    assert np.array_equal(pooled[0], per_query[0]) and np.array_equal(pooled[1], per_query[1]) and np.array_equal(pooled[2], per_query[2])
    assert np.array_equal(pooled[5], per_query[5])
    for b in range(len(pairs)):
        assert np.array_equal(pooled[3][b], per_query[3][b]) and np.array_equal(pooled[4][b], per_query[4][b])
