"""NumPy restatement of the VERIFY-LO family (include/sfm_hip.h, "VERIFY-LO"; docs/tracks.md §12), written from the header alone and
composed with tests/np_verify.py.  The refit is the library's HOST function (`hostgeom.verify_refit`: it loads without a GPU); the 45
fixed-order sums are restated lane class by lane class and the tree level by level.  NumPy evaluates one IEEE operation per ufunc call
(no FMA), in the order written."""
import numpy as np

import np_verify as nv

SLOTS, M32 = nv.SLOTS, nv.M32
LANES = 256
MAX_TOP, MAX_ROUNDS = 16, 8
TRI = [(i, j) for i in range(9) for j in range(i, 9)]


def keys_of(counts_p, nmodels_p):
    """The keys of a pair's models, one per live slot."""
    nm = np.clip(nmodels_p, 0, SLOTS)
    s_idx, j_idx = np.nonzero(np.arange(SLOTS)[None, :] < nm[:, None])
    c = counts_p[s_idx, j_idx].astype(np.uint32).astype(np.uint64)
    return (c << np.uint64(32)) | (np.uint64(M32) - (SLOTS * s_idx + j_idx).astype(np.uint64))


def top(counts, nmodels, T):
    counts, nmodels = np.asarray(counts, np.int32), np.asarray(nmodels, np.int32)
    out = np.zeros((len(nmodels), T), np.uint64)
    for p in range(len(nmodels)):
        keys = np.sort(keys_of(counts[p], nmodels[p]))[::-1][:T]
        out[p, :len(keys)] = keys
    return out


def slot_of(key, H):
    """(has a model, slot)."""
    key = int(key)
    slot = M32 - (key & M32)
    return key != 0 and slot < SLOTS * H, slot


def sampson_value(E, pts):
    """[n_points] float32: the value `np_verify.sampson_in` compares with thr2."""
    E = np.asarray(E, np.float64).reshape(9)
    a1, b1, a2, b2 = (pts[:, k] for k in range(4))
    with np.errstate(all="ignore"):
        e0 = E[0] * a1 + E[1] * b1 + E[2] * 1.0
        e1 = E[3] * a1 + E[4] * b1 + E[5] * 1.0
        e2 = E[6] * a1 + E[7] * b1 + E[8] * 1.0
        f0 = E[0] * a2 + E[3] * b2 + E[6] * 1.0
        f1 = E[1] * a2 + E[4] * b2 + E[7] * 1.0
        s = a2 * e0 + b2 * e1 + 1.0 * e2
        return (s * s / (e0 * e0 + e1 * e1 + f0 * f0 + f1 * f1)).astype(np.float32)


def moments(pts, in_w):
    """M [9, 9]: lane l adds its survivors l, l + 256, .. in ascending order, then the tree h = 1, 2, .. 128."""
    n = len(pts)
    steps = -(-n // LANES)
    a1, b1, a2, b2 = (pts[:, k] for k in range(4))
    with np.errstate(all="ignore"):
        a = np.stack([a2 * a1, a2 * b1, a2, b2 * a1, b2 * b1, b2, a1, b1, np.ones(n)])            # [9, n]
        M = np.zeros((9, 9))
        for i, j in TRI:
            prod = np.zeros(steps * LANES)
            prod[:n] = np.where(in_w, a[i] * a[j], 0.0)             # adding +0 is the identity on a sum that began at +0
            prod = prod.reshape(steps, LANES)
            s = np.zeros(LANES)
            for k in range(steps):
                s = s + prod[k]
            h = 1
            while h < LANES:
                s = s[0::2] + s[1::2]                               # s_l + s_(l + h) for l a multiple of 2 h
                h *= 2
            M[i, j] = M[j, i] = s[0]
    return M


def lo(E, top_keys, surv, m, pairs, img_off, xn, thr2, wide2, refit=None, trace=None):
    if refit is None:
        from sfm_mvs_amd import hostgeom
        refit = hostgeom.verify_refit
    n_pairs, H = E.shape[:2]
    T, cap = top_keys.shape[1], surv.shape[1]
    img_off = np.asarray(img_off, np.int64)
    n_img = len(img_off) - 1
    thr2 = np.float32(thr2)
    wide2 = np.asarray(wide2, np.float32).reshape(-1)
    E_lo, n_lo, round_lo = np.zeros((n_pairs, T, 9)), np.zeros((n_pairs, T), np.int32), np.full((n_pairs, T), -1, np.int32)
    for p in range(n_pairs):
        i, j = int(pairs[p][0]), int(pairs[p][1])
        mp = nv._mprime(m[p], cap, i, j, n_img)
        valid, pts = nv._pair_points(surv[p], mp, i, j, img_off, xn) if mp else (np.zeros(0, bool), np.zeros((0, 4)))
        for t in range(T):
            has, slot = slot_of(top_keys[p, t], H)
            if not has:
                continue
            E_cur = E[p].reshape(-1, 9)[slot].copy()
            v = sampson_value(E_cur, pts)
            E_best, n_best, r_best = E_cur, int((valid & (v <= thr2)).sum()), -1
            for r in range(len(wide2)):
                in_w = valid & (v <= wide2[r])
                if in_w.sum() < 8:
                    break
                M = moments(pts, in_w)
                if trace is not None:
                    trace.append((p, t, r, M))
                with np.errstate(all="ignore"):
                    E_new = np.asarray(refit(M), np.float64).reshape(9)
                if not np.isfinite(E_new).all():
                    break
                v = sampson_value(E_new, pts)
                n_new = int((valid & (v <= thr2)).sum())
                if n_new > n_best:
                    E_best, n_best, r_best = E_new, n_new, r
                E_cur = E_new
            E_lo[p, t], n_lo[p, t], round_lo[p, t] = E_best, n_best, r_best
    return E_lo, n_lo, round_lo


def pick(top_keys, E_lo, n_lo, round_lo, H):
    n_pairs, T = top_keys.shape
    E_sel, nm_sel = np.zeros((n_pairs, 1, SLOTS, 9)), np.zeros((n_pairs, 1), np.int32)
    best_sel, lo_info = np.zeros(n_pairs, np.uint64), np.zeros((n_pairs, 8), np.int32)
    for p in range(n_pairs):
        has = [slot_of(top_keys[p, t], H) for t in range(T)]
        keys = [((int(n_lo[p, t]) & M32) << 32) | (M32 - t) if has[t][0] else 0 for t in range(T)]
        key = max(keys)
        plain = int(top_keys[p, 0]) >> 32
        plain -= (1 << 32) if plain >= (1 << 31) else 0
        if key == 0:
            lo_info[p] = (plain, 0, -1, -1, -1, -1, 0, 0)
            continue
        win = M32 - (key & M32)
        n = key >> 32
        E_sel[p, 0, 0], nm_sel[p, 0], best_sel[p] = E_lo[p, win], 1, np.uint64((n << 32) | M32)
        slot = has[win][1]
        lo_info[p] = (plain, n - ((1 << 32) if n >= (1 << 31) else 0), win, int(round_lo[p, win]), slot // SLOTS, slot % SLOTS, sum(h for h, _ in has), 0)
    return E_sel, nm_sel, best_sel, lo_info


def wide2_of(K, threshold, widen):
    return [nv.thr2_of(K, w * float(threshold)) for w in widen]


def verify_pairs(store, n_query, pairs, img_off, kp, K, ratio=0.70, threshold=0.4, budget=1024, seed=0, lo_top=1, widen=(1.0,), stages=False,
                 plain=None):
    """`np_verify.verify_pairs(lo=dict(top=lo_top, rounds=len(widen), widen=widen))`.  plain: the staged plain result to start from."""
    st = plain if plain is not None else nv.verify_pairs(store, n_query, pairs, img_off, kp, K, ratio, threshold, budget, seed, stages=True)
    part = (st["surv"], st["m"], pairs, img_off, st["xn"])
    H = st["nmodels"].shape[1]
    top_keys = top(st["counts"], st["nmodels"], lo_top)
    cand = lo(st["E_all"], top_keys, *part, st["thr2"], wide2_of(K, threshold, widen))
    E_sel, nm_sel, best_sel, lo_info = pick(top_keys, *cand, H)
    keep, Eb, Rt, info = nv.select(E_sel, nm_sel, best_sel, *part, st["thr2"])
    info[:, 1] = np.clip(st["nmodels"], 0, SLOTS).sum(1)
    info[:, 4:6] = lo_info[:, 4:6]
    out = dict(keep=keep, E=Eb, Rt=Rt, info=info, lo_info=lo_info)
    if stages:
        out.update(top=top_keys, E_lo=cand[0], n_lo=cand[1], round_lo=cand[2], E_sel=E_sel, nmodels_sel=nm_sel, best_sel=best_sel, plain=st)
    return out
