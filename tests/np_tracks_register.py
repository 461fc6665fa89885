"""NumPy restatement of the TRACKS-REGISTER section of include/sfm_hip.h, written from the header alone: the tracks restricted to the
registered images, the composition of two compactions back onto the full table, the per-image scores and the correspondences of one
image.  It shares no code with the product and imports NumPy only."""
import numpy as np

QNAN = np.uint32(0x7FC00000)
INT32_MAX = 2 ** 31 - 1


def image_of(img_off, nodes):
    """The largest i < n_img with img_off[i] <= u, by the header's binary search (its result lies in 0..n_img-1 whatever img_off holds)."""
    img_off = np.asarray(img_off, np.int64)
    nodes = np.asarray(nodes, np.int64)
    lo, hi = np.zeros(nodes.shape, np.int64), np.full(nodes.shape, len(img_off) - 1, np.int64)
    for _ in range(17):
        go = hi - lo > 1
        mid = lo + ((hi - lo) >> 1)
        left = img_off[mid] <= nodes
        lo = np.where(go & left, mid, lo)
        hi = np.where(go & ~left, mid, hi)
    return lo


def clamped(counts, n):
    """(T, nobs) as the device clamps them: a value outside 0..cap becomes cap."""
    cap = n // 2 + 1
    T, nobs = int(counts[0]), int(counts[1])
    return (cap if T < 0 or T > cap else T), (n if nobs < 0 or nobs > n else nobs)


def ranges(track_off, T, nobs):
    off = np.asarray(track_off, np.int64)
    lo = np.minimum(np.maximum(off[:T], 0), nobs)
    hi = np.minimum(np.maximum(off[1:T + 1], lo), nobs)
    return lo, hi


def live_of(obs_node, img_off, registered, n):
    node = np.asarray(obs_node, np.int64)
    ok = (node >= 0) & (node < n)
    reg = np.asarray(registered, np.uint8)
    out = np.zeros(len(node), bool)
    out[ok] = reg[image_of(img_off, node[ok])] != 0
    return out


def restrict(counts, track_off, obs_node, img_off, registered, n, min_len=2):
    """-> track_off2 [T2 + 1], obs_node2 [nobs2], track_src [T2], counts2 [4], all int32.  Tables whose ranges do not overlap only."""
    T, nobs = clamped(counts, n)
    lo, hi = ranges(track_off, T, nobs)
    obs_node = np.asarray(obs_node, np.int32)
    live = live_of(obs_node[:nobs], img_off, registered, n)
    csum = np.concatenate([[0], np.cumsum(live)])
    n_live = csum[hi] - csum[lo]
    kept = n_live >= min_len
    src = np.flatnonzero(kept)
    few = int(((n_live >= 1) & ~kept).sum())
    lost = int(((hi - lo) - n_live)[kept].sum())
    rows = np.concatenate([np.arange(a, b) for a, b in zip(lo[src], hi[src])]) if len(src) else np.zeros(0, np.int64)
    rows = rows[live[rows]] if len(rows) else rows
    track_off2 = np.concatenate([[0], np.cumsum(n_live[src])])
    return (track_off2.astype(np.int32), obs_node[rows], src.astype(np.int32), np.array([len(src), len(rows), few, lost], np.int32))


def adopt(counts, track_off, obs_node, n, counts_r, src_r, counts_p, track_off_p, obs_node_p, X_p, src_p):
    """-> X_full [T, 3] float32 (quiet NaN rows where no point), has_point [T] uint8, obs_live [nobs] uint8."""
    T, nobs = clamped(counts, n)
    Tr, _ = clamped(counts_r, n)
    Tp, nobs_p = clamped(counts_p, n)
    lo, hi = ranges(track_off, T, nobs)
    plo, phi = ranges(track_off_p, Tp, nobs_p)
    X_full = np.full((T, 3), QNAN, np.uint32)
    has = np.zeros(T, np.uint8)
    obs_live = np.zeros(nobs, np.uint8)
    Xw = np.ascontiguousarray(np.asarray(X_p, np.float32).reshape(-1, 3)).view(np.uint32)
    for p in range(Tp):
        r = int(src_p[p])
        if not 0 <= r < Tr:
            continue
        t = int(src_r[r])
        if not 0 <= t < T:
            continue
        has[t] = 1
        X_full[t] = Xw[p]
        j = int(plo[p])
        for o in range(int(lo[t]), int(hi[t])):
            if j < phi[p] and obs_node[o] == obs_node_p[j]:
                obs_live[o] = 1
                j += 1
    return X_full.view(np.float32), has, obs_live


def counting(counts, node_track, has_point, n):
    """bool [N]: the nodes whose track lies in 0..T-1 and has a point."""
    T, _ = clamped(counts, n)
    t = np.asarray(node_track, np.int64)[:n]
    ok = (t >= 0) & (t < T)
    out = np.zeros(n, bool)
    out[ok] = np.asarray(has_point, np.uint8)[t[ok]] != 0
    return out


def cell(c, grid):
    """The header's cell of float32 c: -1 for a NaN, 0 below 0, grid - 1 from grid on, else the truncation."""
    c = np.asarray(c, np.float32)
    with np.errstate(invalid="ignore"):
        inside = np.where(np.isnan(c) | (c < 0) | (c >= np.float32(grid)), np.float32(0), c).astype(np.int64)
        return np.where(np.isnan(c), -1, np.where(c < 0, 0, np.where(c >= np.float32(grid), grid - 1, inside)))


def view_scores(counts, node_track, has_point, img_off, kp, n, width, height, grid):
    """-> seen int32 [n_img], cover uint64 [n_img], cells int32 [n_img]."""
    n_img = len(img_off) - 1
    u = np.flatnonzero(counting(counts, node_track, has_point, n))
    img = image_of(img_off, u)
    seen = np.bincount(img, minlength=n_img).astype(np.int32)
    kp = np.asarray(kp, np.float32).reshape(-1, 2)
    sx, sy = np.float32(grid) / np.float32(width), np.float32(grid) / np.float32(height)
    with np.errstate(invalid="ignore", over="ignore"):
        cx, cy = cell(kp[u, 0] * sx, grid), cell(kp[u, 1] * sy, grid)
    cover = np.zeros(n_img, np.uint64)
    ok = (cx >= 0) & (cy >= 0)
    np.bitwise_or.at(cover, img[ok], np.uint64(1) << (cy[ok] * grid + cx[ok]).astype(np.uint64))
    cells = np.array([bin(int(c)).count("1") for c in cover], np.int32)
    return seen, cover, cells


def correspondences(image, counts, node_track, has_point, X_full, img_off, kp, n):
    """-> X [k, 3] float32, uv [k, 2] float32, track [k] int32 in ascending keypoint."""
    lo = min(max(int(img_off[image]), 0), n)
    hi = min(max(int(img_off[image + 1]), lo), n)
    c = counting(counts, node_track, has_point, n)
    u = lo + np.flatnonzero(c[lo:hi])
    t = np.asarray(node_track, np.int64)[u]
    return (np.asarray(X_full, np.float32).reshape(-1, 3)[t], np.asarray(kp, np.float32).reshape(-1, 2)[u], t.astype(np.int32))
