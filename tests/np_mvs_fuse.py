"""Float32 NumPy restatement of sfm_mvs_fuse (include/sfm_hip.h, "MVS-FUSE"; docs/mvs.md §10), written from the specification: vectorised
over the pixels of a view, looping over views and over the neighbour slots in table order, every constant a np.float32 so that every
operation is a correctly rounded float32 one.  The checker of the device kernel bit for bit, and the CPU model of the calibration
(scripts/calibrate_mvs_fuse.py).  Imports nothing of the product."""
import numpy as np

from np_mvs import F, HALF, ONE, ZERO, _grid

RECORD_WORDS = 128              # 512 bytes per view
MAX_SLOTS = 8
W_NNBR, W_MIN, W_NBR, W_BC, W_AB = 0, 1, 2, 10, 22


def make_table(nbrs, min_consistent, bcs, abs_):
    """The table as int32 [n, 128] from per-view lists: nbrs[i] the view indices, min_consistent[i], bcs[i] float32 [12],
    abs_[i] float32 [len(nbrs[i]), 12].  (Words 118..127 stay 0.)"""
    n = len(nbrs)
    t = np.zeros((n, RECORD_WORDS), np.int32)
    f = t.view(F)
    for i in range(n):
        k = len(nbrs[i])
        assert k <= MAX_SLOTS
        t[i, W_NNBR], t[i, W_MIN] = k, min_consistent[i]
        t[i, W_NBR:W_NBR + k] = nbrs[i]
        f[i, W_BC:W_BC + 12] = np.asarray(bcs[i], F).reshape(12)
        if k:
            f[i, W_AB:W_AB + 12 * k] = np.asarray(abs_[i], F).reshape(-1)
    return t


def words(table):
    """Any array of 512-byte records -> (int32 [n, 128], float32 [n, 128]) views of one copy."""
    t = np.ascontiguousarray(table)
    t = np.frombuffer(t.tobytes(), np.int32).reshape(-1, RECORD_WORDS)
    return t, t.view(F)


def fuse(depth, table, normal=None, bgr=None, tau=0.01, cos_min=-np.inf, unique=True):
    """sfm_mvs_fuse -> dict(mask [n, h, w] u8, xyz [n, h, w, 3] f32, normal [n, h, w, 3] f32 or None, bgr [n, h, w, 3] u8 or None,
    support [n, h, w] u8)."""
    depth = np.asarray(depth, F)
    n, h, w = depth.shape
    ti, tf = words(table)
    tau, cos_min = F(tau), F(cos_min)
    fx, fy = _grid(w, h)
    mask = np.zeros((n, h, w), np.uint8)
    xyz = np.zeros((n, h, w, 3), F)
    support = np.zeros((n, h, w), np.uint8)
    normal_out = None if normal is None else np.zeros((n, h, w, 3), F)
    bgr_out = None if bgr is None else np.zeros((n, h, w, 3), np.uint8)
    with np.errstate(all="ignore"):
        for i in range(n):
            d = depth[i]
            has = d > ZERO
            b = tf[i, W_BC:W_BC + 12]
            X = [d * ((b[3 * k] * fx + b[3 * k + 1] * fy) + b[3 * k + 2]) + b[9 + k] for k in range(3)]
            if normal is not None:
                own = [np.asarray(normal[i][..., k], F) for k in range(3)]
                N = [c.copy() for c in own]
            if bgr is not None:
                S = [bgr[i][..., k].astype(np.int64) for k in range(3)]
            count = np.zeros((h, w), np.int64)
            lower = np.zeros((h, w), bool)
            for s in range(min(int(ti[i, W_NNBR]), MAX_SLOTS)):
                v = int(ti[i, W_NBR + s])
                if v < 0 or v >= n or v == i:
                    continue
                a = tf[i, W_AB + 12 * s:W_AB + 12 * s + 12]
                p = [d * ((a[3 * k] * fx + a[3 * k + 1] * fy) + a[3 * k + 2]) + a[9 + k] for k in range(3)]
                pos = p[2] > ZERO
                den = np.where(pos, p[2], ONE)
                u = np.floor(p[0] / den + HALF)
                t = np.floor(p[1] / den + HALF)
                inb = pos & (u >= ZERO) & (u <= F(w - 1)) & (t >= ZERO) & (t <= F(h - 1))
                u, t = np.where(inb, u, ZERO).astype(F), np.where(inb, t, ZERO).astype(F)
                ui, tj = u.astype(np.int64), t.astype(np.int64)
                dv = depth[v][tj, ui]
                ok = has & inb & (dv > ZERO) & (np.abs(p[2] - dv) <= tau * dv)
                if normal is not None:
                    m = [np.asarray(normal[v][..., k], F)[tj, ui] for k in range(3)]
                    ok &= ((own[0] * m[0] + own[1] * m[1]) + own[2] * m[2]) >= cos_min
                count += ok
                if v < i:
                    lower |= ok
                c = tf[v, W_BC:W_BC + 12]
                for k in range(3):
                    X[k] = np.where(ok, X[k] + (dv * ((c[3 * k] * u + c[3 * k + 1] * t) + c[3 * k + 2]) + c[9 + k]), X[k])
                    if normal is not None:
                        N[k] = np.where(ok, N[k] + m[k], N[k])
                    if bgr is not None:
                        S[k] = S[k] + np.where(ok, bgr[v][..., k].astype(np.int64)[tj, ui], 0)
            keep = has & (count >= int(ti[i, W_MIN])) & ~(bool(unique) & lower)
            k1 = 1 + count
            kf = k1.astype(F)
            mask[i] = keep
            support[i] = np.where(keep, k1, 0)
            for k in range(3):
                xyz[i][..., k] = np.where(keep, X[k] / kf, ZERO)
            if normal is not None:
                length = np.sqrt((N[0] * N[0] + N[1] * N[1]) + N[2] * N[2])
                good = length > ZERO
                for k in range(3):
                    normal_out[i][..., k] = np.where(keep, np.where(good, N[k] / np.where(good, length, ONE), own[k]), ZERO)
            if bgr is not None:
                for k in range(3):
                    bgr_out[i][..., k] = np.where(keep, (2 * S[k] + k1) // (2 * k1), 0)
    return dict(mask=mask, xyz=xyz, normal=normal_out, bgr=bgr_out, support=support)


def consistency_count(depth, table, i, tau):
    """The number of consistent slots of every pixel of view i with no normal test (what sfm_mvs_consistency counts)."""
    t, _ = words(table)
    t = t.copy()
    t[:, W_MIN] = 0
    out = fuse(depth, t, tau=tau, unique=False)
    return out["support"][i].astype(np.int64) - out["mask"][i]
