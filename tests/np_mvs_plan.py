"""NumPy restatement of the MVS-PLAN family (include/sfm_hip.h, "MVS-PLAN"; docs/mvs.md §8), written from the header: loops over tracks
and cameras, np.sort for the order statistics, every float64 operation in the header's order.  The checker of sfm_view_pair_counts /
sfm_view_depth_ranges / sfm_view_select word for word, and the CPU model of the planning (tests/test_mvs_plan_cpu.py).  Imports NumPy only."""
import numpy as np

MIN_DEPTHS = 8


def centres(P):
    """C [ncam, 3] float64 = -M^-1 p4 by adjugate over determinant, in the header's order."""
    p = [np.asarray(P, np.float64).reshape(-1, 12)[:, k] for k in range(12)]
    with np.errstate(all="ignore"):
        a = [[p[5] * p[10] - p[6] * p[9], p[2] * p[9] - p[1] * p[10], p[1] * p[6] - p[2] * p[5]],
             [p[6] * p[8] - p[4] * p[10], p[0] * p[10] - p[2] * p[8], p[2] * p[4] - p[0] * p[6]],
             [p[4] * p[9] - p[5] * p[8], p[1] * p[8] - p[0] * p[9], p[0] * p[5] - p[1] * p[4]]]
        det = (p[0] * a[0][0] + p[1] * a[1][0]) + p[2] * a[2][0]
        return np.stack([-(((a[r][0] * p[3] + a[r][1] * p[7]) + a[r][2] * p[11]) / det) for r in range(3)], 1)


def _row(off, t, nobs):
    lo = min(max(int(off[t]), 0), nobs)
    hi = min(max(int(off[t + 1]), lo), nobs)
    return lo, hi


def pair_counts(track_off, cam_idx, X, C, ncam, cos_lo, cos_hi):
    """-> (shared [ncam, ncam] int32, good [ncam, ncam] int32).  Per track: the observations with a camera in range, all their pairs p < q
    at once (the pairs are independent of one another)."""
    track_off, cam_idx = np.asarray(track_off, np.int64), np.asarray(cam_idx, np.int64)
    X, C = np.asarray(X, np.float64).reshape(-1, 3), np.asarray(C, np.float64).reshape(-1, 3)
    nobs, npt = len(cam_idx), len(track_off) - 1
    shared = np.zeros((ncam, ncam), np.int64)
    good = np.zeros((ncam, ncam), np.int64)
    for t in range(npt):
        lo, hi = _row(track_off, t, nobs)
        cams = cam_idx[lo:hi]
        cams = cams[(cams >= 0) & (cams < ncam)]
        if len(cams) < 2:
            continue
        p, q = np.triu_indices(len(cams), 1)
        a, b = cams[p], cams[q]
        differ = a != b
        a, b = a[differ], b[differ]
        with np.errstate(all="ignore"):
            r, s = X[t] - C[a], X[t] - C[b]
            n_r = (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]
            n_s = (s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2]
            c = ((r[:, 0] * s[:, 0] + r[:, 1] * s[:, 1]) + r[:, 2] * s[:, 2]) / np.sqrt(n_r * n_s)
            ok = bool(np.isfinite(X[t]).all()) & (c >= cos_lo) & (c <= cos_hi)
        np.add.at(shared, (a, b), 1)
        np.add.at(shared, (b, a), 1)
        np.add.at(good, (a[ok], b[ok]), 1)
        np.add.at(good, (b[ok], a[ok]), 1)
    return shared.astype(np.int32), good.astype(np.int32)


def camera_depths(cam_off, cam_obs, cam_idx, pt_idx, X, P, i):
    """The valid float32 depths of camera i, in row order."""
    cam_obs, cam_idx, pt_idx = np.asarray(cam_obs, np.int64), np.asarray(cam_idx, np.int64), np.asarray(pt_idx, np.int64)
    X, P = np.asarray(X, np.float64).reshape(-1, 3), np.asarray(P, np.float64).reshape(-1, 12)
    nobs, npt = len(cam_idx), len(X)
    lo, hi = _row(np.asarray(cam_off, np.int64), i, nobs)
    o = cam_obs[lo:hi]
    o = o[(o >= 0) & (o < nobs)]
    o = o[cam_idx[o] == i]
    j = pt_idx[o]
    j = j[(j >= 0) & (j < npt)]
    with np.errstate(all="ignore"):
        z = (((P[i, 8] * X[j, 0] + P[i, 9] * X[j, 1]) + P[i, 10] * X[j, 2]) + P[i, 11]).astype(np.float32)
    return z[np.isfinite(z) & (z > 0)]


def order_statistics(z, lo_permille, hi_permille):
    """(m, z_lo, z_hi) of the valid depths z: ranks floor(lo (m - 1) / 1000) and ceil(hi (m - 1) / 1000) of np.sort; (0, 0, 0) for none."""
    m = len(z)
    if m == 0:
        return 0, np.float32(0), np.float32(0)
    zs = np.sort(np.asarray(z, np.float32))
    return m, zs[(int(lo_permille) * (m - 1)) // 1000], zs[(int(hi_permille) * (m - 1) + 999) // 1000]


def depth_ranges(cam_off, cam_obs, cam_idx, pt_idx, X, P, lo_permille, hi_permille):
    """-> (m [ncam] int32, z_lo [ncam] float32, z_hi [ncam] float32)."""
    ncam = len(cam_off) - 1
    out = [order_statistics(camera_depths(cam_off, cam_obs, cam_idx, pt_idx, X, P, i), lo_permille, hi_permille) for i in range(ncam)]
    return (np.array([o[0] for o in out], np.int32), np.array([o[1] for o in out], np.float32), np.array([o[2] for o in out], np.float32))


def select(shared, good, nsrc, min_good):
    """-> (nbr [ncam, nsrc] int32 padded with -1, n_nbr [ncam] int32): good descending, shared descending, index ascending."""
    shared, good = np.asarray(shared, np.int64), np.asarray(good, np.int64)
    ncam = len(good)
    nbr = np.full((ncam, nsrc), -1, np.int32)
    n_nbr = np.zeros(ncam, np.int32)
    for i in range(ncam):
        cand = sorted((-int(good[i, j]), -int(shared[i, j]), j) for j in range(ncam) if j != i and good[i, j] >= min_good)[:nsrc]
        nbr[i, :len(cand)] = [c[2] for c in cand]
        n_nbr[i] = len(cand)
    return nbr, n_nbr


def pooled_ranges(m, z_lo, z_hi):
    """ranges [ncam, 2] float64 = (0.8 z_lo, 1.25 z_hi); a view with m < 8 takes the smallest z_lo and the largest z_hi among the views
    with m >= 8; None when no view has 8."""
    m = np.asarray(m, np.int64)
    a, b = np.asarray(z_lo, np.float32).astype(np.float64), np.asarray(z_hi, np.float32).astype(np.float64)
    enough = m >= MIN_DEPTHS
    if not enough.any():
        return None
    return np.stack([0.8 * np.where(enough, a, a[enough].min()), 1.25 * np.where(enough, b, b[enough].max())], 1)


def csr(idx, n):
    """(off [n + 1], order): the stable counting sort of idx into n rows; entries outside 0..n-1 are in no row."""
    idx = np.asarray(idx, np.int64)
    key = np.where((idx >= 0) & (idx < n), idx, n)
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum(np.bincount(key, minlength=n + 1)[:n])
    return off.astype(np.int32), np.argsort(key, kind="stable").astype(np.int32)


def plan_views(cam_idx, pt_idx, X, P, nsrc=4, min_angle_deg=1.0, max_angle_deg=30.0, min_good=8, lo=2, hi=98):
    """The chain of mvs_plan.plan_views + host_plan on the host -> dict(shared, good, neighbours, ranges, m, z_lo, z_hi)."""
    P = np.asarray(P, np.float64).reshape(-1, 12)
    ncam, npt = len(P), len(np.asarray(X).reshape(-1, 3))
    track_off, _ = csr(pt_idx, npt)
    cam_off, cam_obs = csr(cam_idx, ncam)
    cos_lo, cos_hi = float(np.cos(np.deg2rad(float(max_angle_deg)))), float(np.cos(np.deg2rad(float(min_angle_deg))))
    shared, good = pair_counts(track_off, cam_idx, X, centres(P), ncam, cos_lo, cos_hi)
    m, z_lo, z_hi = depth_ranges(cam_off, cam_obs, cam_idx, pt_idx, X, P, int(round(10 * lo)), int(round(10 * hi)))
    nbr, n_nbr = select(shared, good, nsrc, min_good)
    return dict(shared=shared, good=good, nbr=nbr, n_nbr=n_nbr, neighbours=[[int(v) for v in nbr[i, :n_nbr[i]]] for i in range(ncam)],
                ranges=pooled_ranges(m, z_lo, z_hi), m=m, z_lo=z_lo, z_hi=z_hi)
