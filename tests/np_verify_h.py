"""NumPy restatement of the VERIFY-H family (include/sfm_hip.h, "VERIFY-H"; docs/tracks.md §13), written from the header alone and
composed with tests/np_verify.py and tests/np_verify_lo.py: with them it is a complete CPU model of `verify_pairs(homography=...)`.
The 8 x 8 elimination is restated here, vectorised over the samples; the two Jacobi SVDs are the library's HOST functions
(`hostgeom.verify_h_refit`, `hostgeom.verify_h_normalise`: they load without a GPU); the 45 fixed-order sums are restated lane class by
lane class and the tree level by level.  NumPy evaluates one IEEE operation per ufunc call (no FMA), in the order written."""
import numpy as np

import np_verify as nv

M32 = nv.M32
LANES = 256
FEW_SURVIVORS, NO_MODEL = 1, 2
CONFIG_NONE, CONFIG_GENERAL, CONFIG_PLANAR, CONFIG_ROTATING = 0, 1, 2, 3
TRI = [(i, j) for i in range(9) for j in range(i, 9)]


def homography4(x1, x2):
    """x1, x2 [N, 4, 2] -> (ok [N] bool, h [N, 9], zero without a model)."""
    x1, x2 = np.asarray(x1, np.float64).reshape(-1, 4, 2), np.asarray(x2, np.float64).reshape(-1, 4, 2)
    N = len(x1)
    A = np.zeros((N, 8, 9))
    ar = np.arange(N)
    with np.errstate(all="ignore"):
        for k in range(4):
            a1, b1, a2, b2 = x1[:, k, 0], x1[:, k, 1], x2[:, k, 0], x2[:, k, 1]
            A[:, 2 * k, 0], A[:, 2 * k, 1], A[:, 2 * k, 2] = a1, b1, 1.0
            A[:, 2 * k, 6], A[:, 2 * k, 7], A[:, 2 * k, 8] = -(a2 * a1), -(a2 * b1), a2
            A[:, 2 * k + 1, 3], A[:, 2 * k + 1, 4], A[:, 2 * k + 1, 5] = a1, b1, 1.0
            A[:, 2 * k + 1, 6], A[:, 2 * k + 1, 7], A[:, 2 * k + 1, 8] = -(b2 * a1), -(b2 * b1), b2
        alive = np.ones(N, bool)
        for col in range(8):
            piv = np.full(N, col)
            big = np.abs(A[:, col, col])
            for r in range(col + 1, 8):
                v = np.abs(A[:, r, col])
                take = v > big
                big = np.where(take, v, big)
                piv = np.where(take, r, piv)
            top, other = A[ar, col].copy(), A[ar, piv].copy()
            A[ar, piv] = top
            A[ar, col] = other
            d = A[:, col, col]
            alive &= ~(d == 0)                                       # rows of a dead system go on through NaN and inf: never read again
            for r in range(col + 1, 8):
                f = A[:, r, col] / d
                for k in range(col + 1, 9):
                    A[:, r, k] = A[:, r, k] - f * A[:, col, k]
        h = np.zeros((N, 9))
        for col in range(7, -1, -1):
            s = A[:, col, 8].copy()
            for k in range(col + 1, 8):
                s = s - A[:, col, k] * h[:, k]
            h[:, col] = s / A[:, col, col]
        h[:, 8] = 1.0
    ok = alive & np.isfinite(h[:, :8]).all(1)
    h[~ok] = 0.0
    return ok, h


def models(samp, surv, m, pairs, img_off, xn):
    samp = np.asarray(samp, np.int32)
    n_pairs, H = samp.shape[:2]
    cap = surv.shape[1]
    img_off = np.asarray(img_off, np.int64)
    n_img = len(img_off) - 1
    ok, Hm = np.zeros((n_pairs, H), np.int32), np.zeros((n_pairs, H, 9))
    for p in range(n_pairs):
        i, j = int(pairs[p][0]), int(pairs[p][1])
        mp = nv._mprime(m[p], cap, i, j, n_img)
        if mp < 5:
            continue
        valid, pts = nv._pair_points(surv[p], mp, i, j, img_off, xn)
        idx = samp[p, :, :4]
        good = ((idx >= 0) & (idx < mp)).all(1)
        safe = np.where(good[:, None], idx, 0)
        good &= valid[safe].all(1)
        s_idx = np.flatnonzero(good)
        if not len(s_idx):
            continue
        sel = pts[idx[s_idx]]                                        # [n, 4, 4]
        o, h = homography4(sel[:, :, :2], sel[:, :, 2:])
        ok[p, s_idx], Hm[p, s_idx] = o, h
    return ok, Hm


def transfer_class(Hs, pts, thr2h):
    """[n_models, n_points] int8: +1 an inlier of H, -1 an inlier of -H, 0 neither.  Hs [n_models, 9], pts [n_points, 4]."""
    Hs = np.asarray(Hs, np.float64).reshape(-1, 9)[:, :, None]
    a1, b1, a2, b2 = (pts[None, :, k] for k in range(4))
    with np.errstate(all="ignore"):
        w = Hs[:, 6] * a1 + Hs[:, 7] * b1 + Hs[:, 8]
        u = (Hs[:, 0] * a1 + Hs[:, 1] * b1 + Hs[:, 2]) / w
        v = (Hs[:, 3] * a1 + Hs[:, 4] * b1 + Hs[:, 5]) / w
        d = (u - a2) * (u - a2) + (v - b2) * (v - b2)
        near = d.astype(np.float32) <= np.float32(thr2h)
        return np.where(near & (w > 0), 1, np.where(near & (w < 0), -1, 0)).astype(np.int8)


def transfer_value(Hs, pts):
    """(w [n_points], (float)d [n_points]) of one model: what the inlier rule compares."""
    Hs = np.asarray(Hs, np.float64).reshape(9)
    a1, b1, a2, b2 = (pts[:, k] for k in range(4))
    with np.errstate(all="ignore"):
        w = Hs[6] * a1 + Hs[7] * b1 + Hs[8]
        u = (Hs[0] * a1 + Hs[1] * b1 + Hs[2]) / w
        v = (Hs[3] * a1 + Hs[4] * b1 + Hs[5]) / w
        return w, ((u - a2) * (u - a2) + (v - b2) * (v - b2)).astype(np.float32)


def _points(surv, m, pairs, img_off, xn, p):
    cap = surv.shape[1]
    n_img = len(img_off) - 1
    i, j = int(pairs[p][0]), int(pairs[p][1])
    mp = nv._mprime(m[p], cap, i, j, n_img)
    valid, pts = nv._pair_points(surv[p], mp, i, j, img_off, xn) if mp else (np.zeros(0, bool), np.zeros((0, 4)))
    return mp, valid, pts


def score(Hm, ok, surv, m, pairs, img_off, xn, thr2h, chunk=1 << 22):
    n_pairs, H = ok.shape
    img_off = np.asarray(img_off, np.int64)
    counts, best = np.zeros((n_pairs, H), np.int32), np.zeros(n_pairs, np.uint64)
    for p in range(n_pairs):
        mp, valid, pts = _points(surv, m, pairs, img_off, xn, p)
        s_idx = np.flatnonzero(ok[p] != 0)
        if not len(s_idx):
            continue
        c = np.zeros(len(s_idx), np.int64)
        step = max(1, chunk // max(mp, 1))
        for a in range(0, len(s_idx), step):
            c[a:a + step] = ((transfer_class(Hm[p, s_idx[a:a + step]], pts, thr2h) > 0) & valid[None, :]).sum(1)
        counts[p, s_idx] = c
        best[p] = ((c.astype(np.uint64) << np.uint64(32)) | (np.uint64(M32) - s_idx.astype(np.uint64))).max()
    return counts, best


def moments(pts, inl):
    """M [9, 9]: lane l adds its survivors l, l + 256, .. in ascending order, then the tree h = 1, 2, .. 128."""
    n = len(pts)
    steps = -(-n // LANES)
    a1, b1, a2, b2 = (pts[:, k] for k in range(4))
    zero, one = np.zeros(n), np.ones(n)
    with np.errstate(all="ignore"):
        r1 = np.stack([-a1, -b1, -one, zero, zero, zero, a2 * a1, a2 * b1, a2])
        r2 = np.stack([zero, zero, zero, -a1, -b1, -one, b2 * a1, b2 * b1, b2])
        M = np.zeros((9, 9))
        for i, j in TRI:
            prod = np.zeros(steps * LANES)
            prod[:n] = np.where(inl, r1[i] * r1[j] + r2[i] * r2[j], 0.0)    # adding +0 is the identity on a sum that began at +0
            prod = prod.reshape(steps, LANES)
            s = np.zeros(LANES)
            for k in range(steps):
                s = s + prod[k]
            h = 1
            while h < LANES:
                s = s[0::2] + s[1::2]                                # s_l + s_(l + h) for l a multiple of 2 h
                h *= 2
            M[i, j] = M[j, i] = s[0]
    return M


def select(Hm, ok, best, surv, m, pairs, img_off, xn, thr2h, refit=1, refit_fn=None, normalise_fn=None, trace=None):
    if refit_fn is None or normalise_fn is None:
        from sfm_mvs_amd import hostgeom
        refit_fn, normalise_fn = refit_fn or hostgeom.verify_h_refit, normalise_fn or hostgeom.verify_h_normalise
    n_pairs, H = ok.shape
    cap = surv.shape[1]
    img_off = np.asarray(img_off, np.int64)
    keep = np.zeros((n_pairs, cap), np.uint8)
    H_out, sv, info = np.zeros((n_pairs, 9)), np.zeros((n_pairs, 3)), np.zeros((n_pairs, 8), np.int32)
    for p in range(n_pairs):
        few = FEW_SURVIVORS if int(m[p]) < 5 else 0
        key = int(best[p])
        s = M32 - (key & M32)
        if key == 0 or s >= H:
            info[p] = (int(m[p]), 0, 0, 0, -1, -1, 0, few | NO_MODEL)
            continue
        mp, valid, pts = _points(surv, m, pairs, img_off, xn, p)
        q = surv[p, :mp, 0]
        count_me = valid & (q < cap)
        Hw = Hm[p, s].copy()
        inl = count_me & (transfer_class(Hw, pts, thr2h)[0] > 0)
        n_s = n_final = int(inl.sum())
        won = -1
        if refit and n_s >= 8:
            M = moments(pts, inl)
            with np.errstate(all="ignore"):
                c = np.asarray(refit_fn(M), np.float64).reshape(9)
            if trace is not None:
                trace.append((p, M, c))
            if np.isfinite(c).all():
                cls = transfer_class(c, pts, thr2h)[0]
                n_pos, n_neg = int((count_me & (cls > 0)).sum()), int((count_me & (cls < 0)).sum())
                flip = n_neg > n_pos
                if max(n_pos, n_neg) > n_s:
                    Hw, n_final, won = (-c if flip else c), max(n_pos, n_neg), 0
                    inl = count_me & (cls == (-1 if flip else 1))
        keep[p, q[inl]] = 1
        with np.errstate(all="ignore"):
            Hn, s3 = normalise_fn(Hw)
        H_out[p], sv[p] = np.asarray(Hn).reshape(9), s3
        info[p] = (int(m[p]), int((ok[p] != 0).sum()), n_final, n_s, s, won, 0, few)
    return keep, H_out, sv, info


def config_of(info, h_info, h_sv, min_ratio, rot_spread, min_inliers):
    """The two-view configuration word of every pair."""
    n_E, n_H = np.asarray(info)[:, 2].astype(np.float64), np.asarray(h_info)[:, 2].astype(np.float64)
    with np.errstate(all="ignore"):
        spread = h_sv[:, 0] / h_sv[:, 2]
    out = np.where(spread <= np.float64(rot_spread), CONFIG_ROTATING, CONFIG_PLANAR)
    out = np.where(n_H < np.float64(min_ratio) * n_E, CONFIG_GENERAL, out)
    return np.where(n_E < min_inliers, CONFIG_NONE, out).astype(np.int32)


def verify_pairs(store, n_query, pairs, img_off, kp, K, ratio=0.70, threshold=0.4, budget=1024, seed=0, lo=None, threshold_h=1.2, min_ratio=0.246,
                 rot_spread=1.525, min_inliers=8, refit=1, stages=False, plain=None):
    """`verify.verify_pairs(lo=lo, homography=dict(threshold=threshold_h, ...))`.  lo: None or (top, widen).  plain: the staged plain
    result of np_verify to start from."""
    st = plain if plain is not None else nv.verify_pairs(store, n_query, pairs, img_off, kp, K, ratio, threshold, budget, seed, stages=True)
    if lo is None:
        out = {k: st[k] for k in ("keep", "E", "Rt", "info")}
    else:
        import np_verify_lo as nl
        out = nl.verify_pairs(store, n_query, pairs, img_off, kp, K, ratio, threshold, budget, seed, lo_top=lo[0], widen=lo[1], plain=st)
    part = (st["surv"], st["m"], pairs, img_off, st["xn"])
    thr2h = nv.thr2_of(K, threshold_h)
    ok, Hm = models(st["samp"], *part)
    counts, best = score(Hm, ok, *part, thr2h)
    keep_h, H_out, sv, h_info = select(Hm, ok, best, *part, thr2h, refit)
    out.update(H=H_out, keep_h=keep_h, h_sv=sv, h_info=h_info, config=config_of(out["info"], h_info, sv, min_ratio, rot_spread, min_inliers))
    if stages:
        out.update(ok=ok, Hm=Hm, h_counts=counts, h_best=best, thr2h=thr2h, plain=st)
    return out
