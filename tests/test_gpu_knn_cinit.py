"""The row terms of the integer bodies' filter (`filter_i8_body`, csrc/knn.hip).  Every accumulator of a tile starts from one integer
per train row, C_t = floor(w_t / 2) - base.  `knn_split_images_kernel` writes the 32 integers of a tile into the tile's ninth KiB,
the filter stages them through a ring of two slots per wave (one LDS-DMA load per round of two tiles, two rounds ahead) and reads
them into the register block that is SrcC of the groups' first products.  What can go wrong there: the map from accumulator
register to tile row (rows 16 (r >> 3) + 8 h + (r & 7)), the ends of the admitted range of C, the ring's slots, halves and clamps
at every segment length and start, and the padding rows' value in a partial last tile.

Every case compares indices and float32 distance bits with the oracle (`orc_knn2_l2_f32`) and asserts `stats[3]` (4: u8 data,
5: quantised floats) and `stats[1]` (the workgroups that ran).  40 live queries of a row block's 1 024, the workgroup count set
through `sfm_debug_knn_filter_workgroups` on a FRESH matcher, 32 train rows per tile.  Where the data admit no tie and no stream
is full (u8, one or two tiles) `stats[0]` = 0 is required too: a rescan would hide a wrong filter behind the exact re-evaluation."""
import numpy as np
import pytest
import torch

from datagen import sift_like

pytestmark = pytest.mark.gpu

MODE = {"float": 5, "u8": 4}
NQ = 40
C_MAX, C_MIN = 508031, -503936                 # admitted range of C_t (kI8CMax, kI8CMin)


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


def mismatch(hip, oracle, mode, q, t, G, no_rescan=False):
    """None when the run with G workgroups is the oracle's bit for bit on the expected body."""
    wi, wd = oracle.knn2(q, t, nthreads=8)
    gi, gd, st = with_workgroups(hip, G, lambda: run_pair(hip, q, t))
    print(f"nq {len(q)} nt {len(t)} G {G}: stats {st.tolist()}")
    bad = []
    if st[3] != mode:
        bad.append(f"filter arithmetic {st[3]}, expected {mode}")
    if st[1] != G:
        bad.append(f"{st[1]} workgroups ran, the hook asked for {G}")
    if not np.array_equal(gi, wi):
        r = np.flatnonzero((gi != wi).any(1))
        bad.append(f"queries {r[:8].tolist()} got {gi[r[:8]].tolist()}, oracle {wi[r[:8]].tolist()}")
    if not np.array_equal(gd, wd.view(np.uint32)):
        bad.append("distance bits differ from the oracle's")
    if no_rescan and st[0] != 0:
        bad.append(f"{st[0]} queries took the rescan path on data without ties")
    return "; ".join(bad) if bad else None


def as_kind(kind, x):
    """Byte levels as u8 data, or as floats on the grid [0, 1] / 255."""
    return x.astype(np.float32) if kind == "u8" else (x.astype(np.float32) / np.float32(255.0)).astype(np.float32)


def pin_grid(kind, q):
    """Floats: the last of the sixteen query rows the grid is sampled from (row (15 nq) >> 4: query 37 of 40) holds both ends of
    [0, 1], so the quantisation grid is lo = 0, s = 1 / 255 whatever the other rows hold (byte level = 255 x) and no row
    saturates — saturated rows' residuals would send the pair to the 16-bit bodies."""
    if kind == "float":
        r = (15 * len(q)) >> 4
        q[r, 0::2] = 0.0
        q[r, 1::2] = 1.0
    return q


# ---------------------------------------------------------------- the row map of C

def level_rows(tiles):
    """Constant byte levels per row, all different and far apart in norm: tile 0 rising 2, 9, .. 219, tile 1 falling 222, 215, .. 5.
    |level - 127| <= 125 keeps floor(w_t / 2) = 64 (level - 127)^2 inside the admitted spread."""
    lv = [2 + 7 * i for i in range(32)] + [222 - 7 * i for i in range(32)]
    return np.repeat(np.array(lv[:32 * tiles], np.float64)[:, None], 128, axis=1)


def level_queries(rng, t_levels, tile):
    """Query i: row 32 tile + i with 2 added to (or, at the top levels, taken from) its first 64 elements, so that the nearest row
    is that row (d^2 = 256) and the runner-up its neighbour in level on that side (4 736 against 8 320 on the other)."""
    q = rng.integers(60, 200, (NQ, 128)).astype(np.float64)
    for i in range(32):
        row = t_levels[32 * tile + i].copy()
        row[:64] += 2.0 if row[0] < 200 else -2.0
        q[i] = row
    return q


def test_swapped_row_terms_would_change_every_answer():
    """The premise of the row-map cases, checked on the host in exact integers (no device code runs): for every row i of either
    tile and every m in {8, 16, 24}, ranking by d^2 with the C of rows i and i ^ m exchanged changes the nearest neighbour of the
    query on whichever of the two rows has the smaller C (its score rises past every other row's), so every i is covered by its
    own query or its partner's for each m."""
    for tiles in (1, 2):
        t = level_rows(tiles)
        w = ((t - 127.0) ** 2).sum(1)
        for tile in range(tiles):
            q = level_queries(np.random.default_rng(0), t, tile)
            d2 = ((q[:32, None, :] - t[None, :, :]) ** 2).sum(2)
            top2 = [np.argsort(d2[i], kind="stable")[:2].tolist() for i in range(32)]
            assert [p[0] for p in top2] == list(range(32 * tile, 32 * tile + 32))
            for i in range(32):
                for m in (8, 16, 24):
                    changed = []
                    for k in (i, i ^ m):                          # the queries on the two rows
                        s = d2[k].copy()
                        a, b = 32 * tile + i, 32 * tile + (i ^ m)
                        s[a] += 2 * (np.floor(w[b] / 2) - np.floor(w[a] / 2))
                        s[b] += 2 * (np.floor(w[a] / 2) - np.floor(w[b] / 2))
                        changed.append(np.argsort(s, kind="stable")[:2].tolist() != top2[k])
                    assert any(changed), (tiles, tile, i, m)


@pytest.mark.parametrize("kind", ["u8", "float"])
@pytest.mark.parametrize("tiles,tile", [(1, 0), (2, 0), (2, 1)])
def test_row_map_of_the_row_terms(hip, oracle, kind, tiles, tile):
    """32 rows of strongly different norms per tile; queries 0 .. 31 sit on rows 0 .. 31 of `tile`, so a row term that reaches
    another accumulator register than its row's (bits 3 and 4 of the row slot are swapped by the fragment loads) moves a
    neighbour.  u8: distances are distinct and one or two tiles fill no stream, so nothing may be rescanned."""
    rng = np.random.default_rng(100 + 10 * tiles + tile)
    t_levels = level_rows(tiles)
    q = pin_grid(kind, as_kind(kind, level_queries(rng, t_levels, tile)))
    t = as_kind(kind, t_levels)
    wi, _ = oracle.knn2(q, t, nthreads=8)
    assert wi[:32, 0].tolist() == list(range(32 * tile, 32 * tile + 32)), "the planted order is not the oracle's"
    bad = mismatch(hip, oracle, MODE[kind], q, t, 1, no_rescan=kind == "u8")
    assert bad is None, bad


# ---------------------------------------------------------------- the ends of the admitted range

def low_row(w):
    """A u8 row with sum (t - 127)^2 = w for w = 73 217 .. 73 219: 125 elements at 127 + 24 and three more."""
    tail = {73219: (33, 11, 3), 73218: (31, 16, 1), 73217: (31, 16, 0)}[w]
    assert 125 * 576 + sum(v * v for v in tail) == w
    return np.array([151.0] * 125 + [127.0 + v for v in tail], np.float32)


def extreme_pair(rng, w_low, nt=64):
    """All-255 (floor(w / 2) = 1 048 576, the largest a u8 row has), all-0 (1 032 256) and a row of floor(w / 2) = floor(w_low / 2)
    among SIFT-like rows (about 6e5), two tiles.  With w_low = 73 218 or 73 219 the spread is 1 011 967 = kI8CMax - kI8CMin exactly: base = 540 545,
    C = kI8CMax for the all-255 row and kI8CMin for the low one.  Queries 0 .. 11 are near those rows, the rest SIFT-like."""
    t = sift_like(rng, nt)
    t[5], t[37], t[50] = 255.0, 0.0, low_row(w_low)
    q = sift_like(rng, NQ)
    for k, r in enumerate((5, 37, 50) * 4):
        q[k] = t[r]
        c = rng.permutation(128)[:3 + k]
        q[k, c] += np.where(q[k, c] >= 128, -1.0, 1.0) * (1 + k % 3)
    return q, t


@pytest.mark.parametrize("w_low", [73218, 73219])
def test_row_terms_at_both_ends_of_the_range(hip, oracle, w_low):
    """C = kI8CMax and C = kI8CMin (negative) in one image, w_t even and odd; two tiles fill no stream: nothing is rescanned."""
    rng = np.random.default_rng(200)
    q, t = extreme_pair(rng, w_low)
    half = np.floor(((t.astype(np.float64) - 127.0) ** 2).sum(1) / 2)
    assert half.max() - half.min() == C_MAX - C_MIN
    bad = mismatch(hip, oracle, 4, q, t, 1, no_rescan=True)
    assert bad is None, bad


def test_spread_one_past_the_range_takes_the_16_bit_body(hip, oracle):
    """w_t of the low row one smaller, floor(w_t / 2) = 36 608: the spread is 1 011 968 and the range rule rejects the pair.  It
    runs the fp16 body (stats[3] = 0: u8 integers are exact in fp16), under that body's own workgroup rule."""
    rng = np.random.default_rng(201)
    q, t = extreme_pair(rng, 73217)
    half = np.floor(((t.astype(np.float64) - 127.0) ** 2).sum(1) / 2)
    assert half.max() - half.min() == C_MAX - C_MIN + 1
    wi, wd = oracle.knn2(q, t, nthreads=8)
    gi, gd, st = run_pair(hip, q, t)
    print(f"stats {st.tolist()}")
    assert st[3] == 0 and st[1] >= 1, st.tolist()
    assert np.array_equal(gi, wi) and np.array_equal(gd, wd.view(np.uint32))


def test_batch_of_three_pairs_with_their_own_base(hip, oracle):
    """Pair 0 spans the whole range (base 540 545), pair 1 is SIFT-like (base near 6e5), pair 2 holds low levels only
    (base near 4e4): one launch set of three row blocks of two tiles over two workgroups, the second starting inside pair 1's image."""
    rng = np.random.default_rng(202)
    nt, B = 64, 3
    p0 = extreme_pair(rng, 73218, nt)
    p1 = (sift_like(rng, NQ), sift_like(rng, nt))
    t2 = np.clip(np.repeat(rng.integers(100, 156, (nt, 1)), 128, axis=1) + rng.integers(-3, 4, (nt, 128)), 0, 255).astype(np.float32)
    q2 = t2[rng.permutation(nt)[:NQ]].copy()
    q2[:, ::5] += 1.0
    pairs = [p0, p1, (q2, t2)]
    dev = [(torch.from_numpy(q).cuda(), torch.from_numpy(t).cuda()) for q, t in pairs]

    def run():
        bm = hip.BatchMatcher(NQ, nt, "cuda", batch=B)
        bm.run(dev)
        torch.cuda.synchronize()
        return bm.idx.cpu().numpy().copy(), bm.dist.cpu().numpy().view(np.uint32).copy(), bm.stats.cpu().numpy().copy()
    gi, gd, st = with_workgroups(hip, 2, run)
    print("stats", st.tolist())
    assert (st[:, 3] == 4).all() and (st[:, 1] == 2).all(), st.tolist()
    for b, (q, t) in enumerate(pairs):
        wi, wd = oracle.knn2(q, t, nthreads=8)
        assert np.array_equal(gi[b], wi) and np.array_equal(gd[b], wd.view(np.uint32)), b


# ---------------------------------------------------------------- ring, halves and clamps

def varied_rows(rng, kind, n):
    """Rows of one level each (15 .. 235, + noise of +-3): the row terms differ by up to 8e5 from row to row and from tile to tile,
    so the terms of another tile, slot or half lose the planted neighbours."""
    lv = rng.integers(15, 236, (n, 1))
    return as_kind(kind, np.clip(np.repeat(lv, 128, axis=1) + rng.integers(-3, 4, (n, 128)), 0, 255))


def planted_queries(rng, kind, t, nq=NQ, first=0):
    """Queries first .. first + 39 of nq: each a train row with four elements moved by one level, the rows spread evenly over the
    image with its first and last row among them; the other queries are copies of them (dead weight of a full row block)."""
    nt = len(t)
    targets = np.unique(np.concatenate([[0, nt - 1], np.linspace(0, nt - 1, NQ - 2).astype(int)]))
    targets = np.resize(targets, NQ)
    step = np.float32(1.0) if kind == "u8" else np.float32(1.0 / 255.0)
    live = t[targets].copy()
    for k in range(NQ):
        c = rng.permutation(128)[:4]
        live[k, c] += np.where(live[k, c] >= 128 * step, -step, step)
    q = np.resize(live, (nq, 128)).copy()
    q[first:first + NQ] = live
    assert nq == NQ or not first <= (15 * nq) >> 4 < first + NQ
    return pin_grid(kind, q)


RING_TILES = {"u8": (1, 2, 3, 4, 5, 6, 9, 129, 131), "float": (1, 2, 3, 4, 5, 6, 9, 33, 65, 66)}


@pytest.mark.parametrize("kind,tiles", [(k, n) for k in ("u8", "float") for n in RING_TILES[k]])
def test_one_workgroup_segments_of_every_length(hip, oracle, kind, tiles):
    """One workgroup, one segment of 1 .. 6 and 9 tiles (the ring holds two rounds = 4 tiles: 3, 4, 5, 6 are ring depth x 2 - 1 ..
    + 2; in the short ones the DMAs of the rounds behind the last are clamped to it) and the lengths at which a substream
    boundary falls in the remainder tile (33, 65, 129), at a round (131) and behind one (66).  Whole tiles: the partial ones are below."""
    rng = np.random.default_rng(300 + tiles)
    t = varied_rows(rng, kind, 32 * tiles)
    q = planted_queries(rng, kind, t)
    bad = mismatch(hip, oracle, MODE[kind], q, t, 1)
    assert bad is None, bad


@pytest.mark.parametrize("kind", ["u8", "float"])
@pytest.mark.parametrize("G", [2, 3])
def test_segments_that_start_inside_the_image(hip, oracle, kind, G):
    """Nine tiles of one row block over two and three workgroups: segments of 5 + 4 and 3 + 3 + 3 tiles, all but the first
    starting mid-image (the first DMA's offset is the segment's, not the image's)."""
    rng = np.random.default_rng(400 + G)
    t = varied_rows(rng, kind, 288)
    q = planted_queries(rng, kind, t)
    bad = mismatch(hip, oracle, MODE[kind], q, t, G)
    assert bad is None, bad


@pytest.mark.parametrize("kind", ["u8", "float"])
def test_one_workgroup_walks_two_row_blocks(hip, oracle, kind):
    """1 064 queries = two row blocks of five tiles under one workgroup: two segments, the ring restarted for the second while the
    first's last DMAs may still be in flight.  The 40 queries of the second block are the live ones of this file's other cases."""
    rng = np.random.default_rng(500)
    t = varied_rows(rng, kind, 160)
    q = planted_queries(rng, kind, t, nq=1024 + NQ, first=1024)
    bad = mismatch(hip, oracle, MODE[kind], q, t, 1)
    assert bad is None, bad


# ---------------------------------------------------------------- partial last tile

def far_pair(rng, kind, nt):
    """Queries at the top of the value range, train rows at the bottom (the pattern of
    test_gpu_knn_tail_round.py::test_padding_rows_that_would_outrank_every_real_row): a padding row — zero bytes, its row term
    kI8CMax alone — scores below every real row unless the mask removes it, and with any other row term it scores lower still."""
    if kind == "u8":
        return (rng.integers(235, 256, (NQ, 128)).astype(np.float32), rng.integers(0, 21, (nt, 128)).astype(np.float32))
    return (np.float32(0.9) + np.float32(0.1) * rng.random((NQ, 128), dtype=np.float32),
            np.float32(0.1) * rng.random((nt, 128), dtype=np.float32))


@pytest.mark.parametrize("kind", ["u8", "float"])
@pytest.mark.parametrize("tiles", [1, 2, 3])
def test_partial_last_tile(hip, oracle, kind, tiles):
    """nt % 32 in {1, 7, 8, 9, 31} with the partial tile as the remainder tile (1, 3 tiles) and on slot 1 of the tail round (2).
    u8: exact scores without ties and no full stream, so nothing may be rescanned (as in the test this pattern is from)."""
    rng = np.random.default_rng(600 + tiles)
    failures = []
    for rem in (1, 7, 8, 9, 31):
        nt = 32 * (tiles - 1) + rem
        q, t = far_pair(rng, kind, nt)
        bad = mismatch(hip, oracle, MODE[kind], q, t, 1, no_rescan=kind == "u8" and nt >= 2)
        if bad:
            failures.append(f"nt = {nt}: {bad}")
    assert not failures, "\n".join(failures)


# ---------------------------------------------------------------- all-equal train sets

@pytest.mark.parametrize("kind", ["u8", "float"])
def test_all_equal_train_rows(hip, oracle, kind):
    """Every train row ties with every other (one row term for the whole image, five tiles and a partial one): the records decide
    nothing, only the rescan does."""
    rng = np.random.default_rng(700)
    one = sift_like(rng, 1) if kind == "u8" else rng.random((1, 128), dtype=np.float32)
    t = np.repeat(one, 165, axis=0)
    q = sift_like(rng, NQ) if kind == "u8" else rng.random((NQ, 128), dtype=np.float32)
    bad = mismatch(hip, oracle, MODE[kind], q, t, 1)
    assert bad is None, bad
    wi, _ = oracle.knn2(q, t, nthreads=8)
    assert (wi == [0, 1]).all()
