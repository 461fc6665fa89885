"""NumPy restatement of the VERIFY family (include/sfm_hip.h, "VERIFY"; docs/tracks.md §11), written from the header alone.

The minimal solvers are the library's HOST functions (`hostgeom.five_point`, `hostgeom.decompose_essential`: they load without a GPU)
and the cheirality vote is the oracle's `recover_pose_score`, so this module with them is a complete CPU model of the algorithm: every
word `verify.verify_pairs` returns is restated here.  NumPy evaluates one IEEE operation per ufunc call (no FMA), in the order written."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SLOTS = 10
MAX_DRAWS = 64
DIST_THRESH = 50.0
FEW_SURVIVORS, NO_MODEL, NO_VOTE = 1, 2, 4
M32 = 0xFFFFFFFF


def normalise(kp, K):
    K = np.asarray(K, np.float64).reshape(9)
    ifx, ify = 1.0 / K[0], 1.0 / K[4]
    bx, by = -K[2] * (1.0 / K[0]), -K[5] * (1.0 / K[4])
    kp = np.asarray(kp, np.float32).reshape(-1, 2).astype(np.float64)
    return np.stack([kp[:, 0] * ifx + bx, kp[:, 1] * ify + by], 1)


def thr2_of(K, threshold=0.4):
    K = np.asarray(K, np.float64).reshape(9)
    thr = float(threshold) / ((K[0] + K[4]) / 2)
    return np.float32(thr * thr)


def survivors(store, n_query, pairs, img_off, ratio):
    store = np.asarray(store, np.int32)
    n_pairs, cap = store.shape[0], store.shape[2]
    img_off = np.asarray(img_off, np.int64)
    n_img = len(img_off) - 1
    surv = np.full((n_pairs, cap, 2), -1, np.int32)
    m = np.zeros(n_pairs, np.int32)
    for p in range(n_pairs):
        i, j = int(pairs[p][0]), int(pairs[p][1])
        if not (0 <= i < n_img and 0 <= j < n_img) or i == j:
            continue
        na, nb = img_off[i + 1] - img_off[i], img_off[j + 1] - img_off[j]
        limit = max(min(int(n_query[p]), cap, int(na)), 0)
        idx = store[p, 0, :limit]
        d = store[p, 1, :limit].view(np.float32).astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            ok = (idx[:, 1] >= 0) & (idx[:, 0] >= 0) & (idx[:, 0] < nb) & (d[:, 0] < np.float64(ratio) * d[:, 1])
        q = np.flatnonzero(ok)
        m[p] = len(q)
        surv[p, :len(q), 0] = q
        surv[p, :len(q), 1] = idx[q, 0]
    return surv, m


def mix(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x7feb352d) & M32
    x ^= x >> 15
    x = (x * 0x846ca68b) & M32
    x ^= x >> 16
    return x


def draw(seed, p, s, c, m):
    h = mix((mix(mix((seed + 0x9e3779b9 * p) & M32) ^ s) + c) & M32)
    return (h * m) >> 32


def fill_slots(draw_c):
    """The slot loop: draw_c(c) is draw c; five distinct slots from at most 64 draws, or None."""
    slots = []
    for c in range(MAX_DRAWS):
        if len(slots) == 5:
            break
        idx = draw_c(c)
        if idx not in slots:
            slots.append(idx)
    return slots if len(slots) == 5 else None


def samples(m, H, seed):
    m = np.asarray(m)
    out = np.full((len(m), H, 5), -1, np.int32)
    for p in range(len(m)):
        mp = int(m[p])
        if mp < 5:
            continue
        for s in range(H):
            slots = fill_slots(lambda c: draw(int(seed) & M32, p, s, c, mp))
            if slots is not None:
                out[p, s] = slots
    return out


def _pair_points(surv_p, count, i, j, img_off, xn):
    """(valid [count], pts [count, 4]) of the first `count` survivors."""
    n_nodes = len(xn)
    q, t = surv_p[:count, 0].astype(np.int64), surv_p[:count, 1].astype(np.int64)
    u, v = img_off[i] + q, img_off[j] + t
    valid = (q >= 0) & (t >= 0) & (u < n_nodes) & (v < n_nodes)
    pts = np.zeros((count, 4))
    pts[valid, :2] = xn[u[valid]]
    pts[valid, 2:] = xn[v[valid]]
    return valid, pts


def _mprime(m_p, cap, i, j, n_img):
    if not (0 <= i < n_img and 0 <= j < n_img):
        return 0
    return max(min(int(m_p), cap), 0)


def models(samp, surv, m, pairs, img_off, xn, five_point=None):
    if five_point is None:
        from sfm_mvs_amd import hostgeom
        five_point = hostgeom.five_point
    samp = np.asarray(samp, np.int32)
    n_pairs, H = samp.shape[:2]
    cap = surv.shape[1]
    img_off = np.asarray(img_off, np.int64)
    n_img = len(img_off) - 1
    nmodels = np.zeros((n_pairs, H), np.int32)
    E = np.zeros((n_pairs, H, SLOTS, 9))
    for p in range(n_pairs):
        i, j = int(pairs[p][0]), int(pairs[p][1])
        mp = _mprime(m[p], cap, i, j, n_img)
        if mp < 5:
            continue
        valid, pts = _pair_points(surv[p], mp, i, j, img_off, xn)
        for s in range(H):
            idx = samp[p, s]
            if (idx < 0).any() or (idx >= mp).any() or not valid[idx].all():
                continue
            Es = five_point(pts[idx, :2], pts[idx, 2:])
            nmodels[p, s] = len(Es)
            E[p, s, :len(Es)] = Es.reshape(-1, 9)
    return nmodels, E


def sampson_in(E, pts, thr2):
    """[n_models, n_points] bool: score_essential_kernel's expression.  E [n_models, 9], pts [n_points, 4]."""
    E = np.asarray(E, np.float64).reshape(-1, 9)[:, :, None]
    a1, b1, a2, b2 = (pts[None, :, k] for k in range(4))
    with np.errstate(all="ignore"):
        e0 = E[:, 0] * a1 + E[:, 1] * b1 + E[:, 2] * 1.0
        e1 = E[:, 3] * a1 + E[:, 4] * b1 + E[:, 5] * 1.0
        e2 = E[:, 6] * a1 + E[:, 7] * b1 + E[:, 8] * 1.0
        f0 = E[:, 0] * a2 + E[:, 3] * b2 + E[:, 6] * 1.0
        f1 = E[:, 1] * a2 + E[:, 4] * b2 + E[:, 7] * 1.0
        s = a2 * e0 + b2 * e1 + 1.0 * e2
        err = (s * s / (e0 * e0 + e1 * e1 + f0 * f0 + f1 * f1)).astype(np.float32)
        return err <= np.float32(thr2)


def score(E, nmodels, surv, m, pairs, img_off, xn, thr2):
    n_pairs, H = nmodels.shape
    cap = surv.shape[1]
    img_off = np.asarray(img_off, np.int64)
    n_img = len(img_off) - 1
    counts = np.zeros((n_pairs, H, SLOTS), np.int32)
    best = np.zeros(n_pairs, np.uint64)
    for p in range(n_pairs):
        i, j = int(pairs[p][0]), int(pairs[p][1])
        mp = _mprime(m[p], cap, i, j, n_img)
        valid, pts = _pair_points(surv[p], mp, i, j, img_off, xn) if mp else (np.zeros(0, bool), np.zeros((0, 4)))
        nm = np.clip(nmodels[p], 0, SLOTS)
        live = np.arange(SLOTS)[None, :] < nm[:, None]
        if not live.any():
            continue
        s_idx, j_idx = np.nonzero(live)
        c = (sampson_in(E[p, s_idx, j_idx], pts, thr2) & valid[None, :]).sum(1).astype(np.int64)
        counts[p, s_idx, j_idx] = c
        keys = (c.astype(np.uint64) << np.uint64(32)) | (np.uint64(M32) - (SLOTS * s_idx + j_idx).astype(np.uint64))
        best[p] = keys.max()
    return counts, best


def vote(cands, pts):
    """[4, n] bool: sfm_recover_pose_score with rows = 4 and dist_thresh = 50."""
    from oracle import oracle as O
    if len(pts) == 0:
        return np.zeros((4, 0), bool)
    _, mask = O.recover_pose_score(np.ascontiguousarray(cands), np.ascontiguousarray(pts[:, :2]), np.ascontiguousarray(pts[:, 2:]), DIST_THRESH, 4)
    return mask.reshape(4, -1) != 0


def select(E, nmodels, best, surv, m, pairs, img_off, xn, thr2, decompose=None, vote_fn=vote):
    if decompose is None:
        from sfm_mvs_amd import hostgeom
        decompose = hostgeom.decompose_essential
    n_pairs, H = nmodels.shape
    cap = surv.shape[1]
    img_off = np.asarray(img_off, np.int64)
    n_img = len(img_off) - 1
    keep = np.zeros((n_pairs, cap), np.uint8)
    Eb, Rt, info = np.zeros((n_pairs, 9)), np.zeros((n_pairs, 12)), np.zeros((n_pairs, 8), np.int32)
    for p in range(n_pairs):
        i, j = int(pairs[p][0]), int(pairs[p][1])
        mp = _mprime(m[p], cap, i, j, n_img)
        scored = int(np.clip(nmodels[p], 0, SLOTS).sum())
        few = FEW_SURVIVORS if int(m[p]) < 5 else 0
        key = int(best[p])
        slot = M32 - (key & M32)
        if key == 0 or slot >= SLOTS * H:
            info[p] = (int(m[p]), scored, 0, 0, -1, -1, -1, few | NO_MODEL)
            continue
        s, jm = slot // SLOTS, slot % SLOTS
        Em = E[p, s, jm]
        valid, pts = _pair_points(surv[p], mp, i, j, img_off, xn) if mp else (np.zeros(0, bool), np.zeros((0, 4)))
        q = surv[p, :mp, 0]
        inl = np.flatnonzero(valid & (q < cap) & sampson_in(Em, pts, thr2)[0])
        R1, R2, t = decompose(Em)
        cands = np.stack([np.hstack([R, (sg * t)[:, None]]).reshape(12) for R, sg in ((R1, 1.0), (R2, 1.0), (R1, -1.0), (R2, -1.0))])
        votes = vote_fn(cands, pts[inl])
        cnt = votes.sum(1)
        win = int(np.argmax(cnt))                                   # the first of the largest
        keep[p, q[inl[votes[win]]]] = 1
        Eb[p], Rt[p] = Em, cands[win]
        info[p] = (int(m[p]), scored, len(inl), int(cnt[win]), s, jm, win, few | (NO_VOTE if cnt[win] == 0 else 0))
    return keep, Eb, Rt, info


def verify_pairs(store, n_query, pairs, img_off, kp, K, ratio=0.70, threshold=0.4, budget=1024, seed=0, stages=False):
    thr2 = thr2_of(K, threshold)
    xn = normalise(kp, K)
    surv, m = survivors(store, n_query, pairs, img_off, ratio)
    samp = samples(m, budget, seed)
    nmodels, E = models(samp, surv, m, pairs, img_off, xn)
    counts, best = score(E, nmodels, surv, m, pairs, img_off, xn, thr2)
    keep, Eb, Rt, info = select(E, nmodels, best, surv, m, pairs, img_off, xn, thr2)
    out = dict(keep=keep, E=Eb, Rt=Rt, info=info)
    if stages:
        out.update(xn=xn, surv=surv, m=m, samp=samp, nmodels=nmodels, E_all=E, counts=counts, best=best, thr2=thr2)
    return out


def confidence_iters(info, prob=0.999):
    """ransac_update_num_iters(prob, 1 - w, 5, inf) at w = Sampson inliers / survivors."""
    info = np.asarray(info)
    out = np.full(len(info), np.inf)
    for p, row in enumerate(info):
        m, inl = int(row[0]), int(row[2])
        if m <= 0 or inl <= 0:
            continue
        denom = 1.0 - (inl / m) ** 5
        if denom < np.finfo(np.float64).tiny:
            out[p] = 0.0
            continue
        out[p] = np.rint(np.log(max(1.0 - prob, np.finfo(np.float64).tiny)) / np.log(denom))
    return out
