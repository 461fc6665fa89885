"""knn_prep_kernel's grid is sized by the batch (256 row workgroups per pair up to four pairs, 128 for eight), and nothing a later
kernel reads may depend on it: every case runs with `sfm_debug_knn_prep_blocks` at 256, 128, 96 (no divisor of 256) and 1, all
runs must return the same bits — idx, distance bits, Lowe lists, counts, the whole stats row — and those are the oracle's
(`orc_knn2_l2_f32` = cv2.BFMatcher().knnMatch(k=2), then the Lowe ratio 0.70).  The shapes sit on the edges of the row dealing
with 128 blocks (a workgroup-trip of the pair = 2 048 rows, a look-ahead of three trips); the batches run the repair of
knn_split_images_kernel, whose own dealing stays at 256 workgroups, beside a prep grid of another size; the last tests reuse one
workspace under changing block counts, so that per-block words left by an earlier, larger grid would show."""
import numpy as np
import pytest
import torch

from datagen import sift_like

pytestmark = pytest.mark.gpu

RATIO = 0.70
BLOCKS = (256, 128, 96, 1)


def uniform(rng, n, lo=0.0, width=1.0):
    return rng.random((n, 128), dtype=np.float32) * np.float32(width) + np.float32(lo)


def make_pair(rng, kind, nq, nt, lo=0.0, width=1.0):
    """kind "u": uniform floats in [lo, lo + width) (quantised, mode 5), "s": SIFT-like u8 integers (mode 4), "g": Gaussian floats
    (the fp16 body, mode 1); near-twins / copies of a third of the smaller side give the Lowe ratio survivors."""
    k = min(nq, nt) // 3
    if kind == "u":
        q, t = uniform(rng, nq, lo, width), uniform(rng, nt, lo, width)
        if k:
            twins = q[rng.permutation(nq)[:k]] + (rng.standard_normal((k, 128)) * 1e-3 * width).astype(np.float32)
            t[rng.permutation(nt)[:k]] = np.clip(twins, np.float32(lo), np.float32(lo + width)).astype(np.float32)
        return q, t
    if kind == "s":
        q, t = sift_like(rng, nq), sift_like(rng, nt)
    else:
        q, t = rng.standard_normal((nq, 128)).astype(np.float32), rng.standard_normal((nt, 128)).astype(np.float32)
    if k:
        t[rng.permutation(nt)[:k]] = q[rng.permutation(nq)[:k]] * np.float32(1.0 if kind == "s" else 1.001)
    return q, t


MODE = {"u": 5, "s": 4, "g": 1}


def with_blocks(n, fn):
    """fn() with n row workgroups per pair in the prep launch; the rule is back afterwards."""
    from sfm_mvs_amd import _lib
    L = _lib.lib()
    try:
        assert L.sfm_debug_knn_prep_blocks(n) == 0
        return fn()
    finally:
        assert L.sfm_debug_knn_prep_blocks(0) == 0


def same(a, b):
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return np.array_equal(a, b)


def run_pair(pm, dq, dt):
    idx, dist, oq, ot, cnt = pm.run(dq, dt)
    torch.cuda.synchronize()
    m = int(cnt.item())
    return (idx.cpu().numpy().copy(), dist.cpu().numpy().view(np.uint32).copy(), m, oq[:m].cpu().numpy().copy(), ot[:m].cpu().numpy().copy(),
            pm.stats.cpu().numpy().copy())


def check_pair(hip, oracle, q, t, mode):
    dq, dt = torch.from_numpy(q).cuda(), torch.from_numpy(t).cuda()
    wi, wd = oracle.knn2(q, t, nthreads=8)
    wq, wt, _ = oracle.ratio_filter(wi, wd, RATIO)
    runs = {}
    for n in BLOCKS:
        pm = hip.PairMatcher(q.shape[0], t.shape[0], "cuda", ratio=RATIO)
        gi, gd, m, oq, ot, st = runs[n] = with_blocks(n, lambda: run_pair(pm, dq, dt))
        assert st[3] == mode, f"{n} blocks: filter arithmetic {st[3]}, expected {mode}"
        assert np.array_equal(gi, wi), f"{n} blocks: {(gi != wi).any(1).sum()} rows differ"
        assert np.array_equal(gd, wd.view(np.uint32)), n
        assert m == len(wq) and np.array_equal(oq, wq) and np.array_equal(ot, wt), n
    for n in BLOCKS[1:]:
        assert same(runs[n], runs[BLOCKS[0]]), n                     # (idx, dist, count, out_q, out_t, the whole stats row)
    default = run_pair(hip.PairMatcher(q.shape[0], t.shape[0], "cuda", ratio=RATIO), dq, dt)
    assert same(default, runs[BLOCKS[0]]), "the rule's block count"


@pytest.mark.parametrize("nq,nt", [
    (1, 2), (15, 17), (33, 31), (100, 257),
    (1024, 1024),                                                    # exactly one trip of the pair with 128 blocks
    (1024, 1040),                                                    # one workgroup has a second trip
    (2050, 40),                                                      # Q changes to T inside the second trip
    (4100, 2100),                                                    # the fourth trip is partial behind a full three-trip look-ahead
])
def test_uniform_pair_does_not_depend_on_the_block_count(hip, oracle, nq, nt):
    rng = np.random.default_rng(nq * 131 + nt)
    q, t = make_pair(rng, "u", nq, nt)
    check_pair(hip, oracle, q, t, 5)


@pytest.mark.parametrize("lo,width", [(-3.0, 7.0), (250.0, 10.0)])
def test_uniform_pair_in_other_ranges(hip, oracle, lo, width):
    rng = np.random.default_rng(int(width * 1000))
    q, t = make_pair(rng, "u", 100, 257, lo, width)
    check_pair(hip, oracle, q, t, 5)


@pytest.mark.parametrize("kind", ["s", "g"])
@pytest.mark.parametrize("nq,nt", [(100, 257), (1024, 1040)])
def test_general_loop_pair_does_not_depend_on_the_block_count(hip, oracle, kind, nq, nt):
    """SIFT-like u8 pairs (exact-integer body) and Gaussian pairs (fp16 body): the general row loop under the same dealing."""
    rng = np.random.default_rng(nq + nt + ord(kind))
    q, t = make_pair(rng, kind, nq, nt)
    check_pair(hip, oracle, q, t, MODE[kind])


def run_batch(bm, dev):
    bm.run(dev)
    torch.cuda.synchronize()
    cnt = bm.count.cpu().numpy().copy()
    B = len(dev)
    return (bm.idx[:B].cpu().numpy().copy(), bm.dist[:B].cpu().numpy().view(np.uint32).copy(), cnt[:B],
            [bm.out_q[b, :int(cnt[b, 0])].cpu().numpy().copy() for b in range(B)],
            [bm.out_t[b, :int(cnt[b, 0])].cpu().numpy().copy() for b in range(B)], bm.stats[:B].cpu().numpy().copy())


def batch_wants(oracle, pairs):
    out = []
    for q, t in pairs:
        wi, wd = oracle.knn2(q, t, nthreads=8)
        wq, wt, _ = oracle.ratio_filter(wi, wd, RATIO)
        out.append((wi, wd.view(np.uint32), wq, wt))
    return out


def assert_batch(got, wants, mode, what):
    gi, gd, cnt, oq, ot, st = got
    assert (st[:, 3] == mode).all(), (what, st.tolist())
    for b, (wi, wd, wq, wt) in enumerate(wants):
        assert np.array_equal(gi[b], wi) and np.array_equal(gd[b], wd), (what, b)
        assert int(cnt[b, 0]) == len(wq) and np.array_equal(oq[b], wq) and np.array_equal(ot[b], wt), (what, b)


@pytest.mark.parametrize("kinds,nq,nt,mode", [
    ("uuuuuuuu", 257, 100, 5),
    ("ssssssss", 257, 100, 4),
    ("uuugusuu", 100, 257, 1),                                       # the repair runs beside a prep grid of another size
    ("ugusu", 100, 257, 1),                                          # ... and at a batch size whose rule gives no power of two
])
def test_batch_does_not_depend_on_the_block_count(hip, oracle, kinds, nq, nt, mode):
    rng = np.random.default_rng(len(kinds) * 1000 + nq + mode)
    pairs = [make_pair(rng, k, nq, nt) for k in kinds]
    dev = [(torch.from_numpy(q).cuda(), torch.from_numpy(t).cuda()) for q, t in pairs]
    wants = batch_wants(oracle, pairs)
    runs = {}
    for n in BLOCKS + (0,):                                          # (0: the rule)
        bm = hip.BatchMatcher(nq, nt, "cuda", ratio=RATIO, batch=len(pairs))
        runs[n] = with_blocks(n, lambda: run_batch(bm, dev))
        assert_batch(runs[n], wants, mode, (kinds, n))
    for n in runs:
        assert same(runs[n], runs[BLOCKS[0]]), (kinds, n)


def test_entries_no_workgroup_owns_are_rewritten_on_every_launch(hip, oracle):
    """ONE workspace, used at 256 blocks, then 96, then 256: first with the same batch throughout, then with a Gaussian batch
    before a uniform one at 96 blocks.  The shape has 2 112 + 2 112 padded rows, more than 256 x 16, so at 256 blocks EVERY
    workgroup has rows and the Gaussian run leaves inexact-fp16 / not-u8 flags, large norms and residuals in all 256 per-block
    words; stale words in the entries 96 .. 255 (resp. 1 .. 255) would send the uniform batch to the fp16 body (stats[3] = 1
    instead of 5)."""
    rng = np.random.default_rng(77)
    nq, nt, B = 2100, 2100, 8
    uni = [make_pair(rng, "u", nq, nt) for _ in range(B)]
    gau = [make_pair(rng, "g", nq, nt) for _ in range(B)]
    for q, t in gau:
        q *= np.float32(40.0)
        t *= np.float32(40.0)
    dev_u = [(torch.from_numpy(q).cuda(), torch.from_numpy(t).cuda()) for q, t in uni]
    dev_g = [(torch.from_numpy(q).cuda(), torch.from_numpy(t).cuda()) for q, t in gau]
    want_u, want_g = batch_wants(oracle, uni), batch_wants(oracle, gau)
    bm = hip.BatchMatcher(nq, nt, "cuda", ratio=RATIO, batch=B)
    first = with_blocks(256, lambda: run_batch(bm, dev_u))
    assert_batch(first, want_u, 5, 256)
    for n in (96, 256):
        again = with_blocks(n, lambda: run_batch(bm, dev_u))
        assert same(again, first), n
    for n in (256, 96, 1, 256):
        assert_batch(with_blocks(256, lambda: run_batch(bm, dev_g)), want_g, 1, ("gaussian before", n))
        got = with_blocks(n, lambda: run_batch(bm, dev_u))
        assert same(got, first), n


def test_hook_rejects_counts_outside_the_per_block_arrays(hip):
    from sfm_mvs_amd import _lib
    L = _lib.lib()
    assert L.sfm_debug_knn_prep_blocks(257) == -1 and b"sfm_debug_knn_prep_blocks" in L.sfm_last_error()
    assert L.sfm_debug_knn_prep_blocks(-1) == -1
    assert L.sfm_debug_knn_prep_blocks(0) == 0
