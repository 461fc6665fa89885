"""The lean row loop of knn_prep_kernel (pairs that are quantised for the integer body, stats[3] = 5) against the general loop
it replaces for them: every case runs twice — as released, and with `sfm_debug_knn_prep_general(1)`, which sends quantised pairs
through the general loop — and both runs must return the same bits, which are the oracle's (`orc_knn2_l2_f32` =
cv2.BFMatcher().knnMatch(k=2), then the Lowe ratio).  The shapes sit on the edges of the row dealing: the 16-row trip of a
workgroup, the 32-row tile, the switch from the query rows to the train rows, the tails of the 256 x 16-row stride and of the
three-trip look-ahead."""
import numpy as np
import pytest
import torch

from datagen import sift_like

pytestmark = pytest.mark.gpu

RATIO = 0.70


def uniform(rng, n, lo=0.0, width=1.0):
    return rng.random((n, 128), dtype=np.float32) * np.float32(width) + np.float32(lo)


def plant_twins(rng, q, t, lo=0.0, width=1.0):
    """Near-twins (inside the data's range) of a third of the smaller side: Lowe-ratio survivors."""
    k = min(len(q), len(t)) // 3
    if k:
        twins = q[rng.permutation(len(q))[:k]] + (rng.standard_normal((k, 128)) * 1e-3 * width).astype(np.float32)
        t[rng.permutation(len(t))[:k]] = np.clip(twins, np.float32(lo), np.float32(lo + width)).astype(np.float32)


def with_general_loop(fn):
    """fn() as released, then fn() with quantised pairs on the general loop; the switch is off again afterwards."""
    from sfm_mvs_amd import _lib
    L = _lib.lib()
    lean = fn()
    try:
        assert L.sfm_debug_knn_prep_general(1) == 0
        general = fn()
    finally:
        L.sfm_debug_knn_prep_general(0)
    return lean, general


def run_pair(hip, dq, dt):
    pm = hip.PairMatcher(dq.shape[0], dt.shape[0], "cuda", ratio=RATIO)
    idx, dist, oq, ot, cnt = pm.run(dq, dt)
    torch.cuda.synchronize()
    m = int(cnt.item())
    return (idx.cpu().numpy().copy(), dist.cpu().numpy().view(np.uint32).copy(), m, oq[:m].cpu().numpy().copy(), ot[:m].cpu().numpy().copy(),
            pm.stats.cpu().numpy().copy())


def check_pair(hip, oracle, q, t, dq=None, dt=None, mode=5):
    dq = torch.from_numpy(q).cuda() if dq is None else dq
    dt = torch.from_numpy(t).cuda() if dt is None else dt
    lean, general = with_general_loop(lambda: run_pair(hip, dq, dt))
    wi, wd = oracle.knn2(q, t, nthreads=8)
    wq, wt, _ = oracle.ratio_filter(wi, wd, RATIO)
    for name, (gi, gd, m, oq, ot, st) in (("lean", lean), ("general", general)):
        assert st[3] == mode, f"{name}: filter arithmetic {st[3]}, expected {mode}"
        assert np.array_equal(gi, wi), f"{name}: {(gi != wi).any(1).sum()} rows differ"
        assert np.array_equal(gd, wd.view(np.uint32)), name
        assert m == len(wq) and np.array_equal(oq, wq) and np.array_equal(ot, wt), name
    for a, b in zip(lean, general):
        assert np.array_equal(a, b)                                  # (idx, dist, count, out_q, out_t, the whole stats row)
    return lean


@pytest.mark.parametrize("nq,nt,lo,width", [
    (1, 2, 0.0, 1.0),
    (15, 17, 0.0, 1.0), (16, 16, 0.0, 1.0), (17, 33, 0.0, 1.0), (31, 32, 0.0, 1.0), (33, 31, 0.0, 1.0),
    (100, 257, 0.0, 1.0), (100, 257, -3.0, 7.0), (100, 257, 250.0, 10.0),
    (4100, 40, 0.0, 1.0), (40, 4100, 0.0, 1.0),                      # a workgroup's second trip exists on one side only
    (12300, 40, 0.0, 1.0),                                           # the third look-ahead row is partial
])
def test_lean_loop_equals_general_loop_and_oracle(hip, oracle, nq, nt, lo, width):
    rng = np.random.default_rng(nq * 131 + nt + int(width * 1000))
    q, t = uniform(rng, nq, lo, width), uniform(rng, nt, lo, width)
    plant_twins(rng, q, t, lo, width)
    check_pair(hip, oracle, q, t)


def test_strided_rows(hip, oracle):
    rng = np.random.default_rng(21)
    nq, nt = 130, 97
    qw, tw = rng.random((nq, 160), dtype=np.float32), rng.random((nt, 160), dtype=np.float32)
    q, t = np.ascontiguousarray(qw[:, :128]), np.ascontiguousarray(tw[:, :128])
    plant_twins(rng, q, t)
    qw[:, :128], tw[:, :128] = q, t
    dq, dt = torch.from_numpy(qw).cuda()[:, :128], torch.from_numpy(tw).cuda()[:, :128]
    assert dq.stride(0) == 160 and dt.stride(0) == 160
    check_pair(hip, oracle, q, t, dq, dt)


def test_saturation_outside_the_sampled_range(hip, oracle):
    """The grid comes from sixteen sampled rows per side, rows (k n) >> 4.  A value far outside it in another query row saturates;
    its error is in that row's measured residual, the pair stays quantised and the row is still the oracle's."""
    rng = np.random.default_rng(22)
    nq, nt, row = 300, 400, 100
    assert row not in [(k * nq) >> 4 for k in range(16)]
    q, t = uniform(rng, nq), uniform(rng, nt)
    plant_twins(rng, q, t)
    q[row, 5] = 3.0
    gi, gd, m, oq, ot, st = check_pair(hip, oracle, q, t)
    wi, wd = oracle.knn2(q[row:row + 1], t, nthreads=1)
    assert np.array_equal(gi[row], wi[0]) and np.array_equal(gd[row], wd.view(np.uint32)[0])


@pytest.mark.parametrize("kinds,mode", [("usu", 5), ("ugu", 1)])
def test_batches_with_other_kinds_beside_quantised_pairs(hip, oracle, kinds, mode):
    """"usu": a SIFT-like u8 pair between two quantised ones — the lean and the general loop side by side in one launch.
    "ugu": a Gaussian pair sends the batch to the fp16 body — what the lean loop left must be enough for the repair."""
    rng = np.random.default_rng(23 + mode)
    nq, nt = 200, 300
    pairs = []
    for k in kinds:
        if k == "u": q, t = uniform(rng, nq), uniform(rng, nt)
        elif k == "s": q, t = sift_like(rng, nq), sift_like(rng, nt)
        else: q, t = rng.standard_normal((nq, 128)).astype(np.float32), rng.standard_normal((nt, 128)).astype(np.float32)
        if k == "u": plant_twins(rng, q, t)
        else: t[rng.permutation(nt)[:nq // 3]] = q[rng.permutation(nq)[:nq // 3]] * np.float32(1.0 if k == "s" else 1.001)
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

    lean, general = with_general_loop(run)
    for name, (gi, gd, cnt, oq, ot, st) in (("lean", lean), ("general", general)):
        assert st[0, 3] == mode, (name, st.tolist())
        for b, (q, t) in enumerate(pairs):
            wi, wd = oracle.knn2(q, t, nthreads=8)
            wq, wt, _ = oracle.ratio_filter(wi, wd, RATIO)
            assert np.array_equal(gi[b], wi) and np.array_equal(gd[b], wd.view(np.uint32)), (name, kinds, b)
            assert int(cnt[b, 0]) == len(wq) and len(wq) > 20, (name, kinds, b)
            assert np.array_equal(oq[b], wq) and np.array_equal(ot[b], wt), (name, kinds, b)
    assert np.array_equal(lean[0], general[0]) and np.array_equal(lean[1], general[1]) and np.array_equal(lean[2], general[2])
    assert np.array_equal(lean[5], general[5])
    for b in range(len(pairs)):
        assert np.array_equal(lean[3][b], general[3][b]) and np.array_equal(lean[4][b], general[4][b])
