"""The row map of the integer bodies' records (csrc/knn.hip).  The filter's train fragments are loaded with bits 2 and 3 of the
row slot swapped (sigma), so register r of half-wave h of a tile's accumulators holds tile row 16 (r >> 3) + 8 h + (r & 7) and a
record — eight registers — names the eight ADJACENT rows 16 e + 8 h .. + 7.  Three places have to agree on that formula: the
filter's tail mask (`mask_tail`), the refine kernels' row decode (`int_row` / `eval_row`) and the rescan loop that goes through
it.  Every case here requires indices and distance bits identical to the oracle (`orc_knn2_l2_f32`) and `stats[3]` in (4, 5) —
an integer body really ran — on u8 data (exact-integer body, 4) and on uniform floats (quantised body, 5), with the refine's
pooled passes (as released) and with the per-query passes (`sfm_debug_knn_refine_pooled(0)`)."""
import numpy as np
import pytest
import torch

from datagen import sift_like

pytestmark = pytest.mark.gpu

KINDS = ("u8", "float")
MODE = {"u8": 4, "float": 5}


def sigma(m):
    """Row slot m of a 32-row tile with bits 2 and 3 swapped."""
    return (m & ~12) | ((m & 4) << 1) | ((m & 8) >> 1)


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
    return (("pooled", pooled), ("per query", per_query))


def run_pair(hip, q, t):
    dq, dt = torch.from_numpy(q).cuda(), torch.from_numpy(t).cuda()

    def one():
        gi, gd, st = hip.knn2(dq, dt, return_stats=True)
        torch.cuda.synchronize()
        return gi.cpu().numpy().copy(), gd.cpu().numpy().view(np.uint32).copy(), st.cpu().numpy().copy()
    return both_ways(one)


def mismatch(hip, oracle, kind, q, t):
    """None when both runs are the oracle's bit for bit on an integer body, else what differs.  Returns the stats rows too."""
    wi, wd = oracle.knn2(q, t, nthreads=8)
    bad, stats = [], []
    for name, (gi, gd, st) in run_pair(hip, q, t):
        stats.append(st)
        if st[3] != MODE[kind]:
            bad.append(f"{name}: filter arithmetic {st[3]}, expected {MODE[kind]}")
        if not np.array_equal(gi, wi):
            rows_ = np.flatnonzero((gi != wi).any(1))
            bad.append(f"{name}: queries {rows_[:8].tolist()} got {gi[rows_[:8]].tolist()}, oracle {wi[rows_[:8]].tolist()}")
        if not np.array_equal(gd, wd.view(np.uint32)):
            bad.append(f"{name}: distance bits differ")
    return ("; ".join(bad) if bad else None), wi, stats


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("x", [4, 8, 12])
def test_every_slot(hip, oracle, kind, x):
    """nt = nq = 64: query i is train row i plus small noise, its runner-up is planted at row i ^ x.  x = 4 and 8 are the two
    swapped bits (partner in the same record before or after the change, never both), 12 both.  A wrong row formula in any
    register or half-wave returns a wrong index for some i."""
    rng = np.random.default_rng(100 + x)
    t = rows(rng, kind, 64)
    low = x & -x
    for i in range(64):
        if not i & low:
            t[i ^ x] = jitter(rng, kind, t[i:i + 1], 3)[0]
    q = jitter(rng, kind, t, 1)
    bad, wi, _ = mismatch(hip, oracle, kind, q, t)
    assert np.array_equal(wi[:, 0], np.arange(64)) and np.array_equal(wi[:, 1], np.arange(64) ^ x), "the planted order is not the oracle's"
    assert bad is None, bad


def pad_values(kind, q, t, special):
    """What an all-zero byte row of the train image decodes to, and level 0 of the grid.  u8 data: train bytes are t - 128.
    Quantised floats: the grid is lo = min, s = (max - min) / 255 of a sample of sixteen evenly spaced rows of each side
    (q8_sample_grid), a byte is level - 128.  The special rows hold values inside the range, so they do not move the grid."""
    if kind == "u8":
        return 128.0, 0.0
    qs = [(s * len(q)) >> 4 for s in range(16)]
    ts = [(s * len(t)) >> 4 for s in range(16)]
    sample = np.concatenate([q[[r for r in qs if r not in special]].ravel(), t[ts].ravel()])
    lo, hi = np.float32(sample.min()), np.float32(sample.max())
    s = (hi - lo) * np.float32(1.0 / 255.0)
    return float(lo + np.float32(128.0) * s), float(lo)


PARTIAL_NT = list(range(1, 34)) + [39, 40, 41, 47, 48, 49, 55, 56, 57, 63, 65]


@pytest.mark.parametrize("kind", KINDS)
def test_partial_tiles(hip, oracle, kind):
    """Every length of a last, partial tile around the record boundaries (8, 16, 24 rows) of both tiles, nq = 33.  Four queries
    are what a padding row of the train image decodes to (all-zero bytes) and four the grid's lowest level: an unmasked padding
    row (score 0: the middle of the real rows' range) would enter their records.  Only nt < 2 may leave a -1 index."""
    rng = np.random.default_rng(17)
    nq, special = 33, list(range(25, 33))
    failures = []
    for nt in PARTIAL_NT:
        q, t = rows(rng, kind, nq), rows(rng, kind, nt)
        k = min(nq - len(special), nt) // 3
        q[:k] = jitter(rng, kind, t[rng.permutation(nt)[:k]], 1)
        mid, lo = pad_values(kind, q, t, special)
        q[special[:4]] = mid
        q[special[4:]] = lo
        if kind == "u8":                                             # some spread around the padding row's value
            q[special[1:4], ::3] += np.arange(1, 4, dtype=np.float32)[:, None]
        else:
            q[special[1:4], ::3] += np.float32(0.01) * np.arange(1, 4, dtype=np.float32)[:, None]
        bad, wi, _ = mismatch(hip, oracle, kind, q, t)
        if nt >= 2 and (wi < 0).any():
            bad = f"{bad}; the oracle left a -1 index"
        if bad:
            failures.append(f"nt = {nt}: {bad}")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("across", [False, True])
def test_ties_between_swapped_positions(hip, oracle, kind, across):
    """Exact duplicates at both members of every position pair (m, sigma(m)) with sigma(m) != m — in one tile, or m in the first
    tile and sigma(m) in the second (and the other way round): equal distances, the lower index wins."""
    rng = np.random.default_rng(23 + across)
    t = rows(rng, kind, 64)
    pairs = [(m, sigma(m)) for m in range(32) if m < sigma(m)]
    assert len(pairs) == 8
    for m, sm in pairs:
        if across:
            t[32 + sm] = t[m]
            t[32 + m] = t[sm]
        else:
            t[sm] = t[m]
            t[32 + sm] = t[32 + m]
    q = np.concatenate([t, jitter(rng, kind, t, 1)])                  # distance 0 twice, and a near pair of equal distances
    bad, wi, _ = mismatch(hip, oracle, kind, q, t)
    for m, sm in pairs:
        want = [m, 32 + sm] if across else [m, sm]
        assert wi[m].tolist() == want and wi[64 + m].tolist() == want, (m, wi[m].tolist(), wi[64 + m].tolist())
    assert bad is None, bad


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nt", [70, 1100])
@pytest.mark.parametrize("distinct", [False, True])
def test_rescan_path(hip, oracle, kind, nt, distinct):
    """All train rows identical (and with one distinct row): every stream is full of exact ties, none is certifiable, and the
    rescan loop — which walks every record of a stream through the same row decode — decides: stats[0] > 0."""
    rng = np.random.default_rng(31 + nt + distinct)
    t = np.repeat(rows(rng, kind, 1), nt, axis=0)
    if distinct:
        t[nt * 2 // 3 + 5] = rows(rng, kind, 1)[0]
    q = rows(rng, kind, 37)
    q[3] = t[0]
    q[4] = t[nt * 2 // 3 + 5]
    bad, _, stats = mismatch(hip, oracle, kind, q, t)
    assert bad is None, bad
    for st in stats:
        assert st[0] > 0, f"no query took the rescan path: {st.tolist()}"


@pytest.mark.parametrize("kinds,mode", [("f", 5), ("s", 4), ("fsf", 5), ("sss", 4)])
def test_batches(hip, oracle, kinds, mode):
    """Batches of 1 and 3 of shape (70, 75): 'f' uniform floats, 's' a SIFT-like u8 pair — alone it runs the exact-integer body,
    inside a quantised batch it rides along (grid s = 1)."""
    rng = np.random.default_rng(50 + len(kinds) + mode)
    nq, nt = 70, 75
    pairs = []
    for k in kinds:
        kind = "u8" if k == "s" else "float"
        q, t = rows(rng, kind, nq), rows(rng, kind, nt)
        t[rng.permutation(nt)[:nq // 3]] = jitter(rng, kind, q[rng.permutation(nq)[:nq // 3]], 1)
        t[sigma(5)] = t[5]                                           # a tie between swapped positions in every pair
        pairs.append((q, t))
    dev = [(torch.from_numpy(q).cuda(), torch.from_numpy(t).cuda()) for q, t in pairs]

    def run():
        bm = hip.BatchMatcher(nq, nt, "cuda", ratio=0.70, batch=len(pairs))
        bm.run(dev)
        torch.cuda.synchronize()
        return bm.idx.cpu().numpy().copy(), bm.dist.cpu().numpy().view(np.uint32).copy(), bm.stats.cpu().numpy().copy()

    want = [oracle.knn2(q, t, nthreads=8) for q, t in pairs]
    for name, (gi, gd, st) in both_ways(run):
        assert st[0, 3] == mode, (name, st.tolist())
        for b, (wi, wd) in enumerate(want):
            assert np.array_equal(gi[b], wi), (name, kinds, b, np.flatnonzero((gi[b] != wi).any(1))[:8].tolist())
            assert np.array_equal(gd[b], wd.view(np.uint32)), (name, kinds, b)
