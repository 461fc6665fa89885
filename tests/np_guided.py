"""NumPy restatement of the GUIDED family (include/sfm_hip.h, "GUIDED"; docs/tracks.md §14), written from the header alone: every word
`guided.guided_match`, `guided_mutual`, `guided_pairs` and `tracks.guided_keep` return.  NumPy evaluates one IEEE operation per ufunc
call (no FMA), in the order written; float32 sums are formed in the oracle's order (eight strided accumulators, its fold); keys are
uint64.  With tests/np_verify.py (and np_verify_lo / np_verify_h) it is a complete CPU model of `guided_keep`."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import np_verify as nv  # noqa: E402

M32 = 0xFFFFFFFF
NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
INF_BITS = np.int32(0x7F800000)
DIM = 128


def l2sqr(a, b):
    """orc_l2sqr_f32 at n = 128 on rows: a, b float32 [n, 128] -> float32 [n]."""
    a, b = np.asarray(a, np.float32).reshape(-1, DIM), np.asarray(b, np.float32).reshape(-1, DIM)
    with np.errstate(all="ignore"):
        t = a - b
        sq = t * t
        acc = np.zeros((len(t), 8), np.float32)
        for k in range(DIM // 8):
            acc = acc + sq[:, 8 * k:8 * k + 8]
        s = acc[:, :4] + acc[:, 4:]
        return ((s[:, 0] + s[:, 1]) + s[:, 2]) + s[:, 3]


def distance(a, b):
    with np.errstate(all="ignore"):
        return np.sqrt(l2sqr(a, b))


def quotient(E, x1, x2):
    """The float32 word the band compares with thr2g: E [9], x1 [nq, 2], x2 [nt, 2] -> float32 [nq, nt]."""
    E = np.asarray(E, np.float64).reshape(9)
    a1, b1 = x1[:, 0][:, None], x1[:, 1][:, None]
    a2, b2 = x2[:, 0][None, :], x2[:, 1][None, :]
    with np.errstate(all="ignore"):
        e0 = E[0] * a1 + E[1] * b1 + E[2] * 1.0
        e1 = E[3] * a1 + E[4] * b1 + E[5] * 1.0
        e2 = E[6] * a1 + E[7] * b1 + E[8] * 1.0
        f0 = E[0] * a2 + E[3] * b2 + E[6] * 1.0
        f1 = E[1] * a2 + E[4] * b2 + E[7] * 1.0
        s = a2 * e0 + b2 * e1 + 1.0 * e2
        return (s * s / (((e0 * e0 + e1 * e1) + f0 * f0) + f1 * f1)).astype(np.float32)


def extent(p, n_query, pairs, img_off, n_img, cap, rev_stride, active=True):
    """(qb, nt, oa, ob) of pair p."""
    i, j = int(pairs[p][0]), int(pairs[p][1])
    if not active or not (0 <= i < n_img and 0 <= j < n_img) or i == j:
        return 0, 0, 0, 0
    oa, ob = int(img_off[i]), int(img_off[j])
    qb = max(min(int(n_query[p]), cap, int(img_off[i + 1]) - oa), 0)
    nt = max(min(int(img_off[j + 1]) - ob, rev_stride), 0)
    return qb, nt, oa, ob


def band_of(E, xn, qb, nt, oa, ob, thr2g):
    """bool [qb, nt]: the band of a pair, a keypoint without a node in none."""
    n_nodes = len(xn)
    u, v = oa + np.arange(qb, dtype=np.int64), ob + np.arange(nt, dtype=np.int64)
    uo, vo = (u >= 0) & (u < n_nodes), (v >= 0) & (v < n_nodes)
    x1, x2 = np.zeros((qb, 2)), np.zeros((nt, 2))
    x1[uo], x2[vo] = xn[u[uo]], xn[v[vo]]
    with np.errstate(invalid="ignore"):
        return (quotient(E, x1, x2) <= np.float32(thr2g)) & uo[:, None] & vo[None, :]


def guided_match(desc, xn, E, active, n_query, pairs, img_off, cap, thr2g, rev_stride):
    """-> (store_g int32 [n_pairs, 2, cap, 2], rev uint64 [n_pairs, rev_stride])."""
    desc = np.asarray(desc, np.float32).reshape(-1, DIM)
    img_off = np.asarray(img_off, np.int64)
    n_pairs, n_img = len(pairs), len(img_off) - 1
    store = np.empty((n_pairs, 2, cap, 2), np.int32)
    store[:, 0], store[:, 1] = -1, INF_BITS
    rev = np.full((n_pairs, rev_stride), NO_KEY, np.uint64)
    for p in range(n_pairs):
        qb, nt, oa, ob = extent(p, n_query, pairs, img_off, n_img, cap, rev_stride, bool(active[p]))
        if not qb or not nt:
            continue
        band = band_of(E[p], xn, qb, nt, oa, ob, thr2g)
        for q0 in range(0, qb, 64):                                    # blocks of queries bound the memory of a band that admits everything
            qs, ts = np.nonzero(band[q0:q0 + 64])
            qs += q0
            d = distance(desc[oa + qs], desc[ob + ts])
            with np.errstate(invalid="ignore"):
                cand = d < np.inf
            qs, ts, bits = qs[cand], ts[cand], d[cand].view(np.uint32).astype(np.uint64)
            fwd, bwd = (bits << np.uint64(32)) | ts.astype(np.uint64), (bits << np.uint64(32)) | qs.astype(np.uint64)
            np.minimum.at(rev[p], ts, bwd)
            order = np.lexsort((fwd, qs))
            qs, fwd = qs[order], fwd[order]
            if not len(qs):
                continue
            new = np.r_[True, qs[1:] != qs[:-1]]
            rank = np.arange(len(qs)) - np.maximum.accumulate(np.where(new, np.arange(len(qs)), 0))      # the place of a key among its query's
            sel = rank < 2
            store[p, 0, qs[sel], rank[sel]] = (fwd[sel] & np.uint64(M32)).astype(np.int64)
            store[p, 1, qs[sel], rank[sel]] = (fwd[sel] >> np.uint64(32)).astype(np.uint32).view(np.int32)
    return store, rev


def guided_match_loops(desc, xn, E, active, n_query, pairs, img_off, cap, thr2g, rev_stride):
    """The same words by A2's sequential rule, one (q, t) at a time (small inputs only)."""
    from oracle import oracle as O
    desc = np.asarray(desc, np.float32).reshape(-1, DIM)
    img_off = np.asarray(img_off, np.int64)
    n_pairs, n_img, n_nodes = len(pairs), len(img_off) - 1, len(xn)
    store = np.empty((n_pairs, 2, cap, 2), np.int32)
    store[:, 0], store[:, 1] = -1, INF_BITS
    rev = np.full((n_pairs, rev_stride), NO_KEY, np.uint64)
    for p in range(n_pairs):
        qb, nt, oa, ob = extent(p, n_query, pairs, img_off, n_img, cap, rev_stride, bool(active[p]))
        for q in range(qb):
            d0 = d1 = np.float32(np.inf)
            i0 = i1 = -1
            for t in range(nt):
                if not (0 <= oa + q < n_nodes and 0 <= ob + t < n_nodes):
                    continue
                with np.errstate(all="ignore"):
                    if not quotient(E[p], xn[oa + q][None], xn[ob + t][None])[0, 0] <= np.float32(thr2g):
                        continue
                    d = np.sqrt(np.float32(O.l2sqr(desc[oa + q], desc[ob + t])))
                if d < d1:
                    if d < d0:
                        d1, i1, d0, i0 = d0, i0, d, t
                    else:
                        d1, i1 = d, t
                if d < np.inf:
                    key = (int(np.float32(d).view(np.uint32)) << 32) | q
                    rev[p, t] = min(int(rev[p, t]), key)
            store[p, 0, q] = (i0, i1)
            store[p, 1, q] = np.array([d0, d1], np.float32).view(np.int32)
    return store, rev


def guided_mutual(store_g, rev, n_query, pairs, img_off):
    """-> (keep_g uint8 [n_pairs, cap], info_g int32 [n_pairs, 4])."""
    img_off = np.asarray(img_off, np.int64)
    n_pairs, cap, n_img, stride = store_g.shape[0], store_g.shape[2], len(img_off) - 1, rev.shape[1]
    keep, info = np.zeros((n_pairs, cap), np.uint8), np.zeros((n_pairs, 4), np.int32)
    for p in range(n_pairs):
        qb = extent(p, n_query, pairs, img_off, n_img, cap, stride)[0]
        idx = store_g[p, 0, :qb].astype(np.int64)
        ok = (idx[:, 0] >= 0) & (idx[:, 0] < stride)
        low = rev[p, np.where(ok, idx[:, 0], 0)] & np.uint64(M32) if stride else np.zeros(qb, np.uint64)
        keep[p, :qb] = ok & (low == np.arange(qb, dtype=np.uint64))
        info[p] = (qb, (idx[:, 0] >= 0).sum(), (idx[:, 1] >= 0).sum(), keep[p].sum())
    return keep, info


def guided_pairs(desc, n_query, pairs, img_off, kp, K, E, info, threshold, min_inliers, mutual=True, cap=None, max_size=None):
    img_off = np.asarray(img_off, np.int64)
    largest = int(np.diff(img_off).max())
    cap = largest if cap is None else cap
    max_size = largest if max_size is None else max_size
    xn = nv.normalise(kp, K)
    active = (np.asarray(info)[:, 2] >= int(min_inliers)).astype(np.uint8)
    store, rev = guided_match(desc, xn, E, active, n_query, pairs, img_off, cap, nv.thr2_of(K, threshold), max_size)
    keep, info_g = guided_mutual(store, rev, n_query, pairs, img_off) if mutual else (None, None)
    return dict(store=store, keep=keep, info=info_g)


def guided_keep(desc, store, n_query, pairs, img_off, kp, K, ratio=0.70, threshold=0.4, guided_threshold=1.6, min_inliers=8, mutual=True,
                budget=1024, seed=0, stages=False):
    """`tracks.guided_keep`: verify the global store, guide, verify the guided store -> (store_g, keep)."""
    first = nv.verify_pairs(store, n_query, pairs, img_off, kp, K, ratio, threshold, budget, seed)
    g = guided_pairs(desc, n_query, pairs, img_off, kp, K, first["E"], first["info"], guided_threshold, min_inliers, mutual, cap=store.shape[2])
    second = nv.verify_pairs(g["store"], n_query, pairs, img_off, kp, K, ratio, threshold, budget, seed)
    keep = second["keep"] if g["keep"] is None else second["keep"] & g["keep"]
    if stages:
        return g["store"], keep, dict(first=first, guided=g, second=second)
    return g["store"], keep
