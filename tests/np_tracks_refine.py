"""NumPy restatement of the TRACKS-REFINE section of include/sfm_hip.h, written from the header alone: the camera centres, the two
Levenberg-Marquardt phases in float64 in the header's order of operations, the inlier flags, the smallest ray cosine, and the prune.
It shares no code with the product and imports nothing of it.  Tracks are vectorised; observations are walked in order."""
import numpy as np

QNAN = np.uint32(0x7FC00000)
DBL_MAX = np.finfo(np.float64).max
ANGLE_CAP = 64
LAM0 = 1e-3


def canonical(a):
    a = np.array(a, np.float32)
    a.view(np.uint32)[np.isnan(a)] = QNAN
    return a


def image_of(img_off, nodes):
    """The largest i < n_img with img_off[i] <= u."""
    img_off = np.asarray(img_off, np.int64)
    return (np.searchsorted(img_off[:-1], np.asarray(nodes, np.int64), side="right") - 1).astype(np.int64)


def centres(P):
    """C [n_img, 3] float64 = -M^-1 p4 by adjugate over determinant, in the header's order."""
    p = [np.asarray(P, np.float64).reshape(-1, 12)[:, k] for k in range(12)]
    with np.errstate(all="ignore"):
        a = [[p[5] * p[10] - p[6] * p[9], p[2] * p[9] - p[1] * p[10], p[1] * p[6] - p[2] * p[5]],
             [p[6] * p[8] - p[4] * p[10], p[0] * p[10] - p[2] * p[8], p[2] * p[4] - p[0] * p[6]],
             [p[4] * p[9] - p[5] * p[8], p[1] * p[8] - p[0] * p[9], p[0] * p[5] - p[1] * p[4]]]
        det = (p[0] * a[0][0] + p[1] * a[1][0]) + p[2] * a[2][0]
        return np.stack([-(((a[r][0] * p[3] + a[r][1] * p[7]) + a[r][2] * p[11]) / det) for r in range(3)], 1)


class Obs:
    """The observations of T tracks padded to the longest: node, slot (a row of the track), valid (node in 0..N-1), img, kx, ky, Pi."""

    def __init__(self, track_off, obs_node, img_off, kp, P):
        track_off = np.asarray(track_off, np.int64)
        obs_node = np.asarray(obs_node, np.int64)
        n = int(np.asarray(img_off)[-1])
        self.T = len(track_off) - 1
        self.length = np.diff(track_off)
        self.L = int(self.length.max()) if self.T else 0
        k = np.arange(self.L)[None, :]
        self.slot = k < self.length[:, None]
        at = np.where(self.slot, track_off[:-1, None] + k, 0)
        node = obs_node[at] if len(obs_node) else np.zeros(at.shape, np.int64)
        self.valid = self.slot & (node >= 0) & (node < n)
        node = np.where(self.valid, node, 0)
        self.img = image_of(img_off, node) if n else np.zeros(at.shape, np.int64)
        kp = np.asarray(kp, np.float32).reshape(-1, 2)
        kp = kp if len(kp) else np.zeros((1, 2), np.float32)
        self.kx, self.ky = kp[node, 0].astype(np.float64), kp[node, 1].astype(np.float64)
        self.Pi = np.asarray(P, np.float64).reshape(-1, 12)[self.img]                      # [T, L, 12]

    def project(self, q):
        """h_0, h_1, h_2 [T, L] at the points q [T, 3]."""
        q0, q1, q2 = q[:, 0:1], q[:, 1:2], q[:, 2:3]
        Pi = self.Pi
        return [((Pi[..., 4 * r] * q0 + Pi[..., 4 * r + 1] * q1) + Pi[..., 4 * r + 2] * q2) + Pi[..., 4 * r + 3] for r in range(3)]

    def residual(self, q):
        """h_2, u, v, du, dv, e [T, L] at q."""
        h = self.project(q)
        u, v = h[0] / h[2], h[1] / h[2]
        du, dv = u - self.kx, v - self.ky
        return h[2], u, v, du, dv, np.sqrt(du * du + dv * dv)

    def flat(self, a):
        """A padded [T, L] array as the rows [nobs] of an observation array."""
        return a[self.slot]


def rho(e, huber):
    return np.where(e <= huber, (e * e) / 2.0, huber * (e - huber / 2.0))


def ordered_sum(terms, active):
    """Per track, the sum of terms[:, k] over the active k in ascending order, from 0."""
    acc = np.zeros(terms.shape[0])
    for k in range(terms.shape[1]):
        acc = np.where(active[:, k], acc + terms[:, k], acc)
    return acc


def lm_phase(ob, active, x, cost, steps, run, huber, iters, crossed=None):
    """`iters` attempts on the tracks `run` over the observations `active`; huber = None in phase 2 (w = 1, rho = e * e / 2).
    crossed (optional, int [T]) counts the attempts refused because an active observation had no finite h_2 > 0 at the trial point."""
    lam = np.full(ob.T, LAM0)
    for _ in range(iters):
        h2, u, v, du, dv, e = ob.residual(x)
        w = np.ones_like(e) if huber is None else np.where(e <= huber, 1.0, huber / e)
        ja = [(ob.Pi[..., k] - u * ob.Pi[..., 8 + k]) / h2 for k in range(3)]
        jb = [(ob.Pi[..., 4 + k] - v * ob.Pi[..., 8 + k]) / h2 for k in range(3)]
        A = {}
        for a in range(3):
            for b in range(a, 3):
                acc = np.zeros(ob.T)
                for k in range(ob.L):
                    acc = np.where(active[:, k], (acc + w[:, k] * (ja[a][:, k] * ja[b][:, k])) + w[:, k] * (jb[a][:, k] * jb[b][:, k]), acc)
                A[a, b] = acc
        g = []
        for a in range(3):
            acc = np.zeros(ob.T)
            for k in range(ob.L):
                acc = np.where(active[:, k], (acc + w[:, k] * (ja[a][:, k] * du[:, k])) + w[:, k] * (jb[a][:, k] * dv[:, k]), acc)
            g.append(acc)
        s00, s11, s22 = A[0, 0] + lam * A[0, 0], A[1, 1] + lam * A[1, 1], A[2, 2] + lam * A[2, 2]
        a01, a02, a12 = A[0, 1], A[0, 2], A[1, 2]
        c00, c01, c02 = s11 * s22 - a12 * a12, a02 * a12 - a01 * s22, a01 * a12 - a02 * s11
        c11, c12, c22 = s00 * s22 - a02 * a02, a01 * a02 - s00 * a12, s00 * s11 - a01 * a01
        det = (s00 * c00 + a01 * c01) + a02 * c02
        d = np.stack([-(((c00 * g[0] + c01 * g[1]) + c02 * g[2]) / det), -(((c01 * g[0] + c11 * g[1]) + c12 * g[2]) / det),
                      -(((c02 * g[0] + c12 * g[1]) + c22 * g[2]) / det)], 1)
        ok = run & (det != 0.0) & np.isfinite(d).all(axis=1)
        xn = x + d
        h2n, _, _, _, _, en = ob.residual(xn)
        behind = (active & ~((h2n > 0.0) & (h2n <= DBL_MAX))).any(axis=1)
        if crossed is not None:
            crossed += ok & behind
        ok &= ~behind
        trial = ordered_sum((en * en) / 2.0 if huber is None else rho(en, huber), active)
        ok &= trial < cost
        x = np.where(ok[:, None], xn, x)
        cost = np.where(ok, trial, cost)
        lam = np.where(ok, lam / 10.0, lam * 10.0)
        steps = steps + ok
    return x, cost, steps


def refine(track_off, obs_node, img_off, kp, P, X_in, flags_in, huber=1.0, obs_thresh=2.0, iters=10, iters2=5, detail=False):
    """-> X_out [T, 3] f32, inlier [nobs] u8, err [nobs] f32, depth [nobs] f32, n_inl [T] i32, max_err [T] f32, cos_min [T] f32,
    steps [T] i32, flags [T] i32 (detail: also the Huber cost at the end of phase 1, the float64 point there, and per track the attempts
    refused because a trial point lay behind a camera)."""
    ob = Obs(track_off, obs_node, img_off, kp, P)
    T = ob.T
    X_in = canonical(np.asarray(X_in, np.float32).reshape(-1, 3)[:T])
    flags_in = np.asarray(flags_in, np.int32)[:T]
    with np.errstate(all="ignore"):
        x = X_in.astype(np.float64)
        start = ((flags_in & 2) != 0) & np.isfinite(x).all(axis=1)
        h2, _, _, _, _, e = ob.residual(x)
        usable = ob.valid & start[:, None] & (h2 > 0.0) & (h2 <= DBL_MAX) & np.isfinite(e)
        cost = ordered_sum(rho(e, huber), usable)
        steps, crossed = np.zeros(T, np.int64), np.zeros(T, np.int64)
        x, cost, steps = lm_phase(ob, usable, x, cost, steps, start, huber, iters, crossed)
        cost1, x1 = cost.copy(), x.copy()
        _, _, _, _, _, e = ob.residual(x)
        inl = usable & (e <= obs_thresh)
        n_inl = inl.sum(axis=1)
        cost = ordered_sum((e * e) / 2.0, inl)
        x, cost, steps = lm_phase(ob, inl, x, cost, steps, start & (n_inl >= 2), None, iters2, crossed)
        X_out = canonical(np.where(start[:, None], x.astype(np.float32), X_in))
        xf = X_out.astype(np.float64)
        h2, _, _, _, _, e = ob.residual(xf)
        err = canonical(np.where(ob.valid, e.astype(np.float32), np.float32(np.nan)))
        depth = canonical(np.where(ob.valid, h2.astype(np.float32), np.float32(np.nan)))
        worst = np.zeros(T, np.float32)
        for k in range(ob.L):
            ek = err[:, k]
            worst = np.where(inl[:, k] & ((ek > worst) | np.isnan(ek)), ek, worst)
        cos_min = smallest_cosine(ob, inl, xf, centres(P))
        point_ok = start & np.isfinite(X_out).all(axis=1)
        flags = np.where(start, (n_inl >= 2).astype(np.int32) | (point_ok.astype(np.int32) << 1), 0).astype(np.int32)
    out = (X_out, ob.flat(inl).astype(np.uint8), ob.flat(err), ob.flat(depth), n_inl.astype(np.int32), canonical(worst), cos_min,
           steps.astype(np.int32), flags)
    return out + (cost1, x1, crossed) if detail else out


def smallest_cosine(ob, inl, xf, C):
    """float32 [T]: the smallest cosine between the rays xf - C[image] of the first 64 inliers, pairs i < j in order, from 1."""
    T = ob.T
    rank = np.cumsum(inl, axis=1) - 1
    m = np.minimum(inl.sum(axis=1), ANGLE_CAP)
    simg = np.zeros((T, ANGLE_CAP), np.int64)
    take = inl & (rank < ANGLE_CAP)
    tt, kk = np.nonzero(take)
    simg[tt, rank[tt, kk]] = ob.img[tt, kk]
    rays = xf[:, None, :] - C[simg]                                                       # [T, 64, 3]
    norm = (rays[..., 0] * rays[..., 0] + rays[..., 1] * rays[..., 1]) + rays[..., 2] * rays[..., 2]
    low = np.ones(T)
    for i in range(int(m.max()) - 1 if T else 0):
        for j in range(i + 1, int(m.max())):
            dot = (rays[:, i, 0] * rays[:, j, 0] + rays[:, i, 1] * rays[:, j, 1]) + rays[:, i, 2] * rays[:, j, 2]
            c = dot / np.sqrt(norm[:, i] * norm[:, j])
            low = np.where((j < m) & (c < low), c, low)
    return low.astype(np.float32)


def prune(track_off, obs_node, X, inlier, n_inl, max_err, cos_min, flags, min_len=2, max_reproj=np.inf, max_cos=1.0):
    """-> track_off2 [T' + 1] i32, obs_node2 [nobs'] i32, X2 [T', 3] f32 (the words of X), track_src [T'] i32, counts2 [4] i32."""
    track_off = np.asarray(track_off, np.int64)
    obs_node = np.asarray(obs_node, np.int32)
    T = len(track_off) - 1
    inlier = np.asarray(inlier)[:len(obs_node)] != 0
    with np.errstate(invalid="ignore"):
        keep = ((np.asarray(flags)[:T] == 3) & (np.asarray(n_inl, np.int64)[:T] >= min_len)
                & (np.asarray(max_err, np.float32)[:T].astype(np.float64) <= max_reproj)
                & (np.asarray(cos_min, np.float32)[:T].astype(np.float64) <= max_cos))
    tr = np.repeat(np.arange(T), np.diff(track_off))
    held = np.bincount(tr[inlier], minlength=T)[:T] if T else np.zeros(0, np.int64)
    sel = keep[tr] & inlier if T else np.zeros(0, bool)
    src = np.flatnonzero(keep)
    track_off2 = np.concatenate([[0], np.cumsum(held[src])])
    counts2 = [len(src), int(sel.sum()), T - len(src), int((np.diff(track_off)[src] - held[src]).sum())]
    return (track_off2.astype(np.int32), obs_node[sel], np.asarray(X, np.float32).reshape(-1, 3)[:T][src], src.astype(np.int32),
            np.array(counts2, np.int32))


def run_robust(base, img_off, kp, P, min_len=2, max_reproj=None, huber=1.0, obs_thresh=2.0, max_cos=1.0, iters=10, iters2=5):
    """The robust composition on `base`, a dict with the track_off, obs_node, X, flags and counts of the plain one: refine, prune, and
    the pruned set in the form a sparse bundle adjustment takes."""
    r = refine(base["track_off"], base["obs_node"], img_off, kp, P, base["X"], base["flags"], huber, obs_thresh, iters, iters2)
    off2, obs2, X2, src, counts2 = prune(base["track_off"], base["obs_node"], r[0], r[1], r[4], r[5], r[6], r[8], min_len,
                                         np.inf if max_reproj is None else max_reproj, max_cos)
    nodes = obs2.astype(np.int64)
    length = np.diff(off2.astype(np.int64))
    return dict(points=X2, obs=np.asarray(kp, np.float32).reshape(-1, 2)[nodes], cam_idx=image_of(img_off, nodes).astype(np.int32),
                pt_idx=np.repeat(np.arange(len(length)), length).astype(np.int32), track_len=length.astype(np.int32), counts=base["counts"],
                tracks_dropped=int(counts2[2]), obs_dropped=int(counts2[3]), refined=r, track_off=off2, obs_node=obs2, track_src=src,
                counts2=counts2)
