"""The partial last tile of the train image outside the rounds of the integer bodies' filter (`filter_i8_body`, csrc/knn.hip).
The rounds of two tiles (steady and boundary) carry neither the test for the partial tile nor the code that masks its padding
rows: they stop short of tile `tiles - 1` whenever `nt % 32 != 0` and the segment holds it, and that tile runs through a tested
instantiation — as the remainder tile (slot 0), or as slot 1 of a short tail round behind the last whole tile.  What can go wrong
is the round structure (a tile run twice or not at all, a substream boundary missed on the tile that moved, fragments loaded for
the wrong tile) and the mask (skipped on the moved tile, or applied to a whole one).

Every case caps the workgroup count with `sfm_debug_knn_filter_workgroups`, so that one workgroup (or two, three) walks the whole
train image, and requires indices and distance bits identical to the oracle's (`orc_knn2_l2_f32`) with `stats[3]` naming the
body that ran (4: exact-integer on u8 data, 5: quantised floats).  In every pair the true nearest neighbour of the first queries
is planted at row nt - 1 and the runner-up at nt - 2 (the partial tile's last real rows), and eight queries are what a padding
row of the train image decodes to (the construction of `test_gpu_knn_rowmap.py`).  32 train rows per tile; substreams of 32
tiles (floats) and 128 tiles (u8).

The mask itself is pinned by `test_padding_rows_that_would_outrank_every_real_row`: a padding row is zero bytes and scores the
init value alone, so it outranks real rows only when queries and train rows lie on opposite sides of the grid's middle.  A build
whose tested instantiation never masks (`part_cur = false` in `tile()`) fails that test in four of its eight cases — indices -1 / -1
against the oracle's on one tile of floats, 40 rescans instead of none on u8 data behind a whole tile (slot 1 of the tail round) and
at and behind a boundary — and passes everything else in this file (and `test_gpu_knn_rowmap.py::test_partial_tiles`): with queries equal to a
padding row's value the padding scores WORST and never ranks, so those cases pin the round structure only.  On floats behind a
whole tile the rescan restores the oracle's answer with or without the mask; only u8 data shows the difference there."""
import numpy as np
import pytest
import torch

from datagen import sift_like

pytestmark = pytest.mark.gpu

MODE = {"float": 5, "u8": 4}
NQ = 40
PLANTED = 6                                   # queries 0 .. 5: nearest nt - 1, runner-up nt - 2
SPECIAL = list(range(27, 35))                 # queries equal to a padding row / to level 0 of the grid
REMS = (0, 1, 7, 8, 9, 16, 31)


def rows(rng, kind, n):
    return sift_like(rng, n) if kind == "u8" else rng.random((n, 128), dtype=np.float32)


def jitter(rng, kind, x, level):
    """x plus noise: level 1 is well below level 3, and level 3 well below the distance between two random rows."""
    if kind == "u8":
        y = x.copy()
        for r in range(len(y)):
            c = rng.permutation(128)[:4 * level]
            y[r, c] = np.where(y[r, c] >= 128, y[r, c] - 1, y[r, c] + 1)
        return y
    return np.clip(x + (rng.standard_normal(x.shape) * 2e-3 * level).astype(np.float32), 0.0, 1.0).astype(np.float32)


def pad_values(kind, q, t):
    """What an all-zero byte row of the train image decodes to, and level 0 of the grid.  u8 data: train bytes are t - 128.
    Quantised floats: the grid is lo = min, s = (max - min) / 255 of a sample of sixteen evenly spaced rows of each side, a byte
    is level - 128.  The special rows hold values inside the range, so they do not move the grid."""
    if kind == "u8":
        return 128.0, 0.0
    qs = [(s * len(q)) >> 4 for s in range(16)]
    ts = [(s * len(t)) >> 4 for s in range(16)]
    sample = np.concatenate([q[[r for r in qs if r not in SPECIAL]].ravel(), t[ts].ravel()])
    lo, hi = np.float32(sample.min()), np.float32(sample.max())
    s = (hi - lo) * np.float32(1.0 / 255.0)
    return float(lo + np.float32(128.0) * s), float(lo)


def make_pair(rng, kind, nt, nq=NQ):
    q, t = rows(rng, kind, nq), rows(rng, kind, nt)
    if nt >= 2:
        t[nt - 2] = jitter(rng, kind, t[nt - 1:nt], 3)[0]
    q[:PLANTED] = jitter(rng, kind, np.repeat(t[nt - 1:nt], PLANTED, axis=0), 1)
    mid, lo = pad_values(kind, q, t)
    q[SPECIAL[:4]] = mid
    q[SPECIAL[4:]] = lo
    step = np.arange(1, 4, dtype=np.float32)[:, None]                 # some spread around the padding row's value
    q[SPECIAL[1:4], ::3] += step if kind == "u8" else np.float32(0.01) * step
    return q, t


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


def mismatch(hip, oracle, kind, q, t, G, planted=True):
    """None when the run with G workgroups is the oracle's bit for bit on the expected body and the planted order holds."""
    nt = t.shape[0]
    wi, wd = oracle.knn2(q, t, nthreads=8)
    if planted and nt >= 2 and wi[:PLANTED].tolist() != [[nt - 1, nt - 2]] * PLANTED:
        return f"the planted order is not the oracle's: {wi[:PLANTED].tolist()}"
    gi, gd, st = with_workgroups(hip, G, lambda: run_pair(hip, q, t))
    bad = []
    if st[3] != MODE[kind]:
        bad.append(f"filter arithmetic {st[3]}, expected {MODE[kind]}")
    if st[1] != G:
        bad.append(f"{st[1]} workgroups ran, the hook asked for {G}")
    if not np.array_equal(gi, wi):
        r = np.flatnonzero((gi != wi).any(1))
        bad.append(f"queries {r[:8].tolist()} got {gi[r[:8]].tolist()}, oracle {wi[r[:8]].tolist()}")
    if not np.array_equal(gd, wd.view(np.uint32)):
        bad.append("distance bits differ from the oracle's")
    return "; ".join(bad) if bad else None


def nt_of(tiles, rem):
    return 32 * tiles if rem == 0 else 32 * (tiles - 1) + rem


@pytest.mark.parametrize("kind", ["float", "u8"])
@pytest.mark.parametrize("tiles", [1, 2, 3, 4, 5])
def test_segments_of_one_to_five_tiles(hip, oracle, kind, tiles):
    """A segment shorter than a round, the partial tile on slot 0 (1, 3, 5 tiles: the remainder tile) and on slot 1 (2, 4 tiles:
    the tail round), every remainder around the records' boundaries (8, 16 rows) and none.  Only nt = 1 may leave a -1 index."""
    rng = np.random.default_rng(1000 + tiles)
    failures = []
    for rem in REMS:
        nt = nt_of(tiles, rem)
        q, t = make_pair(rng, kind, nt)
        bad = mismatch(hip, oracle, kind, q, t, 1)
        if bad:
            failures.append(f"nt = {nt} ({tiles} tiles, {rem} rows in the last): {bad}")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("kind,tiles", [("float", 33), ("float", 34), ("float", 65), ("float", 66), ("u8", 129), ("u8", 130)])
def test_partial_tile_at_a_substream_boundary(hip, oracle, kind, tiles):
    """nt % 32 = 5.  33, 65, 129 tiles: the partial tile is the boundary tile and the remainder tile at once.  34, 66, 130: the
    boundary falls on the tail round's slot-0 tile, the partial tile is the one after it."""
    rng = np.random.default_rng(2000 + tiles)
    q, t = make_pair(rng, kind, nt_of(tiles, 5))
    bad = mismatch(hip, oracle, kind, q, t, 1)
    assert bad is None, bad


@pytest.mark.parametrize("kind", ["float", "u8"])
@pytest.mark.parametrize("G", [2, 3])
@pytest.mark.parametrize("tiles", [66, 67])
def test_only_the_last_segment_holds_the_partial_tile(hip, oracle, kind, G, tiles):
    """One row block over two and three workgroups: the segments before the last end on whole tiles and run the untested
    instantiation right up to their end (an even or an odd number of tiles), the last one ends on the partial tile."""
    rng = np.random.default_rng(3000 + 10 * tiles + G)
    q, t = make_pair(rng, kind, nt_of(tiles, 5))
    bad = mismatch(hip, oracle, kind, q, t, G)
    assert bad is None, bad


@pytest.mark.parametrize("kind", ["float", "u8"])
@pytest.mark.parametrize("G", [1, 2])
def test_batch_of_three_pairs(hip, oracle, kind, G):
    """Three row blocks of 66 tiles (one per pair, nq = 40), each ending on a partial tile of 5 rows, over one and two workgroups:
    a workgroup walks more than one segment, and with two the boundary between them falls inside the second pair."""
    rng = np.random.default_rng(4000 + G)
    nt, B = nt_of(66, 5), 3
    pairs = [make_pair(rng, kind, nt) for _ in range(B)]
    dev = [(torch.from_numpy(q).cuda(), torch.from_numpy(t).cuda()) for q, t in pairs]

    def run():
        bm = hip.BatchMatcher(NQ, nt, "cuda", batch=B)
        bm.run(dev)
        torch.cuda.synchronize()
        return bm.idx.cpu().numpy().copy(), bm.dist.cpu().numpy().view(np.uint32).copy(), bm.stats.cpu().numpy().copy()
    gi, gd, st = with_workgroups(hip, G, run)
    assert (st[:, 3] == MODE[kind]).all(), st.tolist()
    for b, (q, t) in enumerate(pairs):
        wi, wd = oracle.knn2(q, t, nthreads=8)
        assert wi[:PLANTED].tolist() == [[nt - 1, nt - 2]] * PLANTED, "the planted order is not the oracle's"
        assert np.array_equal(gi[b], wi) and np.array_equal(gd[b], wd.view(np.uint32)), b


@pytest.mark.parametrize("kind", ["float", "u8"])
@pytest.mark.parametrize("tiles", [34, 35])
def test_all_equal_train_rows(hip, oracle, kind, tiles):
    """Every train row ties with every other, the partial tile's five real rows included: the records decide nothing and the
    rescan walks every substream from `sttab` — the tile ranges written by the remainder tile and the tail round have to be
    right, or the lowest two indices are not found."""
    rng = np.random.default_rng(5000 + tiles)
    nt = nt_of(tiles, 5)
    t = np.repeat(rows(rng, kind, 1), nt, axis=0)
    q = rows(rng, kind, NQ)
    bad = mismatch(hip, oracle, kind, q, t, 1, planted=False)
    assert bad is None, bad
    wi, _ = oracle.knn2(q, t, nthreads=8)
    assert (wi == [0, 1]).all()


def far_pair(rng, kind, nt, nq=NQ):
    """Queries at the top of the value range, train rows at the bottom: query bytes near +127, train bytes near -128, so every
    real row's score lies far ABOVE a padding row's (zero bytes, the init value alone) and an unmasked padding row outranks all
    of them in every record it touches."""
    if kind == "u8":
        return (rng.integers(235, 256, (nq, 128)).astype(np.float32), rng.integers(0, 21, (nt, 128)).astype(np.float32))
    return (np.float32(0.9) + np.float32(0.1) * rng.random((nq, 128), dtype=np.float32),
            np.float32(0.1) * rng.random((nt, 128), dtype=np.float32))


FAR_TILES = {"float": (1, 2, 33, 34), "u8": (1, 2, 129, 130)}


@pytest.mark.parametrize("kind,tiles", [(k, n) for k in ("float", "u8") for n in FAR_TILES[k]])
def test_padding_rows_that_would_outrank_every_real_row(hip, oracle, kind, tiles):
    """The mask on the moved tile.  With queries and train rows on opposite sides of the grid's middle a padding row scores below
    every real row: unmasked, its keys fill the records of the partial tile (the remainder tile for 1, 33 and 129 tiles, slot 1 of
    the tail round for 2, 34 and 130; nt % 32 = 1, 5, 7, so three of a tile's four records are padding alone), the refine kernel
    forms its distance limit from a padding key and drops the real rows: the answer is -1 / -1 where no stream is full, and
    every query takes the rescan path where one is.  `stats[0]` = 0 is required on u8 data: the scores are exact integers, so a
    stream's third key can reach a query's second distance only through an exact tie between the best rows of two records
    (squared distances near 7e6 spread over some 4e4: about 1e-4 per query), and one tile's stream is not even full.  On
    quantised floats the certificate carries the quantisation error and these queries open with the mask too: bits only."""
    rng = np.random.default_rng(6000 + tiles)
    failures = []
    for rem in (1, 5, 7):
        nt = nt_of(tiles, rem)
        q, t = far_pair(rng, kind, nt)
        wi, wd = oracle.knn2(q, t, nthreads=8)
        gi, gd, st = with_workgroups(hip, 1, lambda: run_pair(hip, q, t))
        print(f"{kind} nt = {nt}: stats {st.tolist()}")
        bad = []
        if st[3] != MODE[kind]:
            bad.append(f"filter arithmetic {st[3]}, expected {MODE[kind]}")
        if not np.array_equal(gi, wi):
            r = np.flatnonzero((gi != wi).any(1))
            bad.append(f"queries {r[:8].tolist()} got {gi[r[:8]].tolist()}, oracle {wi[r[:8]].tolist()}")
        if not np.array_equal(gd, wd.view(np.uint32)):
            bad.append("distance bits differ from the oracle's")
        if kind == "u8" and st[0] != 0:
            bad.append(f"{st[0]} queries took the rescan path on exact-integer data without ties")
        if bad:
            failures.append(f"nt = {nt}: " + "; ".join(bad))
    assert not failures, "\n".join(failures)
