"""The key flush inside the tile loop of the integer bodies' filter (`filter_i8_body`, csrc/knn.hip).  A workgroup's segment is cut
into substreams of 32 tiles (quantised floats, stats[3] = 5) or 128 tiles (u8 data, stats[3] = 4); at every boundary the three keys
of each query are stored and the stream's tile range goes to `sttab`.  The boundary round of the loop is a copy of its own, a
boundary can also fall on the odd remainder tile behind the rounds, and all eight query slots of a lane are stored whether the
query exists or not.  By the rule (`G = min(256, units)`) a workgroup spans several substreams at full size only, so every case
caps the workgroup count with `sfm_debug_knn_filter_workgroups`, builds a FRESH matcher (the count sizes the workspace), and
requires indices and distance bits identical to the oracle's (`orc_knn2_l2_f32`) and to the run under the rule, with `stats[3]`
naming the body that ran.  32 train rows per tile."""
import numpy as np
import pytest
import torch

from datagen import sift_like

pytestmark = pytest.mark.gpu

MODE = {"float": 5, "u8": 4}
FLOAT_NT = (1056, 2048, 2080, 2277)          # 33, 64, 65, 72 tiles: boundary in the remainder tile / at the segment end / two / a partial last tile


def rows(rng, kind, n):
    return sift_like(rng, n) if kind == "u8" else rng.random((n, 128), dtype=np.float32)


def with_workgroups(hip, n, fn):
    """fn() with at most n filter workgroups; the rule is back afterwards."""
    try:
        hip.debug_knn_filter_workgroups(n)
        return fn()
    finally:
        hip.debug_knn_filter_workgroups(0)


def run_pair(hip, q, t):
    pm = hip.PairMatcher(q.shape[0], t.shape[0], "cuda")
    idx, dist, _, _, _ = pm.run(torch.from_numpy(q).cuda(), torch.from_numpy(t).cuda())
    torch.cuda.synchronize()
    return idx.cpu().numpy().copy(), dist.cpu().numpy().view(np.uint32).copy(), pm.stats.cpu().numpy().copy()


def check_pair(hip, oracle, kind, q, t, G):
    wi, wd = oracle.knn2(q, t, nthreads=8)
    gi, gd, st = with_workgroups(hip, G, lambda: run_pair(hip, q, t))
    assert st[3] == MODE[kind], f"filter arithmetic {st[3]}, expected {MODE[kind]}"
    assert st[1] == G, f"{st[1]} workgroups ran, the hook asked for {G}"
    bad = np.flatnonzero((gi != wi).any(1))
    assert bad.size == 0, f"queries {bad[:8].tolist()} got {gi[bad[:8]].tolist()}, oracle {wi[bad[:8]].tolist()}"
    assert np.array_equal(gd, wd.view(np.uint32)), "distance bits differ from the oracle's"
    ri, rd, rst = run_pair(hip, q, t)                                 # the rule
    assert rst[3] == MODE[kind] and rst[1] != G, rst.tolist()
    assert np.array_equal(gi, ri) and np.array_equal(gd, rd), "differs from the run under the rule"
    return wi


@pytest.mark.parametrize("nt", FLOAT_NT)
def test_one_workgroup_walks_every_substream(hip, oracle, nt):
    """nq = 40: 984 of the row block's 1 024 query slots are dead and stored all the same."""
    rng = np.random.default_rng(nt)
    check_pair(hip, oracle, "float", rows(rng, "float", 40), rows(rng, "float", nt), 1)


@pytest.mark.parametrize("nt", FLOAT_NT)
def test_neighbours_on_both_sides_of_a_boundary(hip, oracle, nt):
    """Rows 1 023 | 1 024 and 2 047 | 2 048 are the last row of a substream and the first of the next (32 tiles of 32 rows), nt - 1
    the last real row.  Query k lies between two of those rows, nearer to the first: a key lost at a flush, or flushed into the
    neighbouring substream's slot, changes its answer."""
    rng = np.random.default_rng(7 * nt)
    t = rows(rng, "float", nt)
    special = sorted({r for r in (1023, 1024, 2047, 2048, nt - 1) if r < nt})
    pairs = [(a, b) for a in special for b in special if a != b]
    q = rows(rng, "float", 40)
    assert len(pairs) <= 40
    for k, (a, b) in enumerate(pairs):
        q[k] = np.float32(0.6) * t[a] + np.float32(0.4) * t[b]
    wi = check_pair(hip, oracle, "float", q, t, 1)
    assert wi[:len(pairs)].tolist() == [list(p) for p in pairs], "the planted order is not the oracle's"


def test_middle_workgroup_opens_a_row_block_with_numbered_substreams(hip, oracle):
    """Two row blocks of 70 tiles over three workgroups: the middle one ends the first row block in substreams numbered after the
    first workgroup's (sbase > 0) and opens the second at substream 0."""
    rng = np.random.default_rng(3)
    check_pair(hip, oracle, "float", rows(rng, "float", 1100), rows(rng, "float", 2240), 3)


def test_u8_substreams_of_128_tiles(hip, oracle):
    """131 tiles, the last partial: a boundary at tile 128 inside the rounds, then the remainder tile."""
    rng = np.random.default_rng(4)
    check_pair(hip, oracle, "u8", rows(rng, "u8", 40), rows(rng, "u8", 4163), 1)


@pytest.mark.parametrize("kind", ["float", "u8"])
def test_all_equal_train_rows(hip, oracle, kind):
    """Every train row ties with every other: the records decide nothing and the rescan walks each substream from `sttab`'s first
    tile over its tile count — both have to be right for every substream, or the lowest two indices are not found."""
    rng = np.random.default_rng(5)
    nt = 2277
    t = np.repeat(rows(rng, kind, 1), nt, axis=0)
    wi = check_pair(hip, oracle, kind, rows(rng, kind, 40), t, 1)
    assert (wi == [0, 1]).all()


def test_batch_of_three_pairs_over_two_workgroups(hip, oracle):
    """Three row blocks of 65 tiles (one per pair) over two workgroups: the boundary between them falls inside the second pair."""
    rng = np.random.default_rng(6)
    nq, nt, B = 40, 2080, 3
    pairs = [(rows(rng, "float", nq), rows(rng, "float", nt)) for _ in range(B)]
    dev = [(torch.from_numpy(q).cuda(), torch.from_numpy(t).cuda()) for q, t in pairs]

    def run():
        bm = hip.BatchMatcher(nq, nt, "cuda", batch=B)
        bm.run(dev)
        torch.cuda.synchronize()
        return bm.idx.cpu().numpy().copy(), bm.dist.cpu().numpy().view(np.uint32).copy(), bm.stats.cpu().numpy().copy()
    gi, gd, st = with_workgroups(hip, 2, run)
    ri, rd, rst = run()
    assert (st[:, 3] == 5).all() and (rst[:, 3] == 5).all(), (st.tolist(), rst.tolist())
    for b, (q, t) in enumerate(pairs):
        wi, wd = oracle.knn2(q, t, nthreads=8)
        assert np.array_equal(gi[b], wi) and np.array_equal(gd[b], wd.view(np.uint32)), b
    assert np.array_equal(gi, ri) and np.array_equal(gd, rd), "differs from the run under the rule"


def test_hook_rejects_counts_outside_the_grid(hip):
    from sfm_mvs_amd import _lib
    L = _lib.lib()
    assert L.sfm_debug_knn_filter_workgroups(257) == -1 and b"sfm_debug_knn_filter_workgroups" in L.sfm_last_error()
    assert L.sfm_debug_knn_filter_workgroups(-1) == -1
    assert L.sfm_debug_knn_filter_workgroups(0) == 0
