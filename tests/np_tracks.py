"""NumPy restatement of the TRACKS section of include/sfm_hip.h, written from the header alone: edges from a match store, component
minima, the conflict and length rules, tracks in label order with their nodes in ascending id, and the N-view triangulation in
float64 in the header's order of operations.  It shares no code with the product and imports nothing of it."""
import numpy as np

QNAN = np.uint32(0x7FC00000)
PIVOTS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
SWEEPS = 30


def image_of(img_off, nodes):
    """The largest i < n_img with img_off[i] <= u."""
    img_off = np.asarray(img_off, np.int64)
    return (np.searchsorted(img_off[:-1], np.asarray(nodes, np.int64), side="right") - 1).astype(np.int64)


def match_edges(store, nq, pair_img, img_off, ratio, keep=None):
    """store int32 [n_pairs, 2, cap, 2] -> edges int32 [n_pairs * cap, 2]; (-1, -1) where the slot holds no survivor."""
    store = np.asarray(store, np.int32)
    n_pairs, _, cap, _ = store.shape
    img_off = np.asarray(img_off, np.int64)
    n_img = len(img_off) - 1
    pair_img = np.asarray(pair_img, np.int64).reshape(n_pairs, 2)
    nq = np.asarray(nq, np.int64).reshape(n_pairs)
    edges = np.full((n_pairs, cap, 2), -1, np.int32)
    q = np.arange(cap, dtype=np.int64)
    for p in range(n_pairs):
        a, b = pair_img[p]
        if not (0 <= a < n_img and 0 <= b < n_img):
            continue
        na, nb = img_off[a + 1] - img_off[a], img_off[b + 1] - img_off[b]
        t0, t1 = store[p, 0, :, 0].astype(np.int64), store[p, 0, :, 1]
        d = store[p, 1].view(np.float32).astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            ok = (q < nq[p]) & (q < na) & (t1 >= 0) & (t0 >= 0) & (t0 < nb) & (d[:, 0] < ratio * d[:, 1])
        if keep is not None:
            ok &= np.asarray(keep).reshape(n_pairs, cap)[p] != 0
        edges[p, ok, 0] = (img_off[a] + q[ok]).astype(np.int32)
        edges[p, ok, 1] = (img_off[b] + t0[ok]).astype(np.int32)
    return edges.reshape(n_pairs * cap, 2)


def valid_edges(edges, n):
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    ok = (e[:, 0] >= 0) & (e[:, 0] < n) & (e[:, 1] >= 0) & (e[:, 1] < n) & (e[:, 0] != e[:, 1])
    return e[ok]


def components(edges, n):
    """label[u] = the smallest node id of u's component over the valid edges."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    if n == 0:
        return np.zeros(0, np.int32)
    e = valid_edges(edges, n)
    g = coo_matrix((np.ones(len(e), np.int8), (e[:, 0], e[:, 1])), shape=(n, n))
    _, comp = connected_components(g, directed=False)
    low = np.full(comp.max() + 1, n, np.int64)
    np.minimum.at(low, comp, np.arange(n))
    return low[comp].astype(np.int32)


def is_valid_state(labels, final):
    """An unconverged labelling: every label names a node of the node's own component, >= its minimum and <= the node."""
    labels = np.asarray(labels, np.int64)
    final = np.asarray(final, np.int64)
    n = len(final)
    if len(labels) != n:
        return False
    if n == 0:
        return True
    if labels.min() < 0 or labels.max() >= n:
        return False
    return bool(np.all(final[labels] == final) and np.all(labels >= final) and np.all(labels <= np.arange(n)))


def build(labels, img_off, min_len=2, max_len=2 ** 31 - 1):
    """-> node_track [N], track_off [T + 1], obs_node [nobs], counts [6], all int32."""
    labels = np.asarray(labels, np.int64)
    n = len(labels)
    size = np.bincount(labels, minlength=n) if n else np.zeros(0, np.int64)
    roots = np.flatnonzero(labels == np.arange(n))
    cand = roots[size[roots] >= 2]
    in_cand = size[labels] >= 2 if n else np.zeros(0, bool)
    nodes = np.flatnonzero(in_cand)
    conflict = np.zeros(n, bool)
    if len(nodes):
        pairs = np.stack([labels[nodes], image_of(img_off, nodes)], 1)
        uniq, cnt = np.unique(pairs, axis=0, return_counts=True)
        conflict[uniq[cnt > 1, 0]] = True
    kept = cand[~conflict[cand] & (size[cand] >= min_len) & (size[cand] <= max_len)]          # ascending label
    track_of = np.full(n, -1, np.int64)
    track_of[kept] = np.arange(len(kept))
    node_track = track_of[labels] if n else np.zeros(0, np.int64)
    members = np.flatnonzero(node_track >= 0)
    order = np.lexsort((members, node_track[members]))
    obs_node = members[order]
    track_off = np.concatenate([[0], np.cumsum(size[kept])])
    counts = [len(kept), len(obs_node), len(cand), int(conflict[cand].sum()), int(size[kept].max()) if len(kept) else 0,
              int((size[roots] < 2).sum())]
    return node_track.astype(np.int32), track_off.astype(np.int32), obs_node.astype(np.int32), np.array(counts, np.int32)


def canonical(a):
    a = np.array(a, np.float32)
    a.view(np.uint32)[np.isnan(a)] = QNAN
    return a


def rows_of(kp, P, img_off, nodes):
    """r0, r1 [m, 4] float64 of the observations `nodes`."""
    img = image_of(img_off, nodes)
    Pi = np.asarray(P, np.float64).reshape(-1, 12)[img]
    x = np.asarray(kp, np.float32)[nodes, 0].astype(np.float64)[:, None]
    y = np.asarray(kp, np.float32)[nodes, 1].astype(np.float64)[:, None]
    return x * Pi[:, 8:12] - Pi[:, 0:4], y * Pi[:, 8:12] - Pi[:, 4:8]


def normal_matrices(track_off, obs_node, img_off, kp, P, n):
    """M [T, 4, 4] float64, summed in observation order as the header writes it."""
    track_off = np.asarray(track_off, np.int64)
    obs_node = np.asarray(obs_node, np.int64)
    T = len(track_off) - 1
    M = np.zeros((T, 4, 4))
    length = np.diff(track_off)
    with np.errstate(all="ignore"):
        for k in range(int(length.max()) if T else 0):
            tr = np.flatnonzero(length > k)
            nodes = obs_node[track_off[tr] + k]
            ok = (nodes >= 0) & (nodes < n)
            tr, nodes = tr[ok], nodes[ok]
            r0, r1 = rows_of(kp, P, img_off, nodes)
            for a in range(4):
                for b in range(a, 4):
                    M[tr, a, b] = (M[tr, a, b] + r0[:, a] * r0[:, b]) + r1[:, a] * r1[:, b]
    for a in range(1, 4):
        for b in range(a):
            M[:, a, b] = M[:, b, a]
    return M


def jacobi_smallest(M):
    """The header's cyclic Jacobi over a stack of symmetric 4 x 4: -> v [T, 4], the column of the smallest diagonal entry."""
    M = np.array(M, np.float64)
    T = len(M)
    V = np.broadcast_to(np.eye(4), (T, 4, 4)).copy()
    active = np.ones(T, bool)
    with np.errstate(all="ignore"):
        for _ in range(SWEEPS):
            if not active.any():
                break
            rotated = np.zeros(T, bool)
            for p, q in PIVOTS:
                apq, app, aqq = M[:, p, q].copy(), M[:, p, p].copy(), M[:, q, q].copy()
                skip = (apq == 0.0) | (np.abs(apq) <= 2.0 ** -52 * np.sqrt(np.abs(app) * np.abs(aqq)))
                do = active & ~skip
                if not do.any():
                    continue
                rotated |= do
                theta = (aqq - app) / (2.0 * apq)
                root = np.sqrt(theta * theta + 1.0)
                t = np.where(theta >= 0.0, 1.0 / (theta + root), -1.0 / (root - theta))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                for k in range(4):
                    if k in (p, q):
                        continue
                    akp, akq = M[:, k, p].copy(), M[:, k, q].copy()
                    newp, newq = c * akp - s * akq, s * akp + c * akq
                    M[:, k, p] = M[:, p, k] = np.where(do, newp, akp)
                    M[:, k, q] = M[:, q, k] = np.where(do, newq, akq)
                M[:, p, p] = np.where(do, app - t * apq, app)
                M[:, q, q] = np.where(do, aqq + t * apq, aqq)
                M[:, p, q] = M[:, q, p] = np.where(do, 0.0, apq)
                for k in range(4):
                    vkp, vkq = V[:, k, p].copy(), V[:, k, q].copy()
                    V[:, k, p] = np.where(do, c * vkp - s * vkq, vkp)
                    V[:, k, q] = np.where(do, s * vkp + c * vkq, vkq)
            active &= rotated
        best = np.zeros(T, np.int64)
        diag = M[:, 0, 0].copy()
        for k in range(1, 4):
            better = M[:, k, k] < diag
            best = np.where(better, k, best)
            diag = np.where(better, M[:, k, k], diag)
    return V[np.arange(T), :, best]


def triangulate(track_off, obs_node, img_off, kp, P):
    """-> X [T, 3] f32, err [nobs] f32, depth [nobs] f32, flags [T] i32, max_err [T] f32."""
    track_off = np.asarray(track_off, np.int64)
    obs_node = np.asarray(obs_node, np.int64)
    kp = np.asarray(kp, np.float32).reshape(-1, 2)
    n = int(np.asarray(img_off)[-1])
    T, nobs = len(track_off) - 1, len(obs_node)
    v = jacobi_smallest(normal_matrices(track_off, obs_node, img_off, kp, P, n))
    with np.errstate(all="ignore"):
        X = canonical((v[:, :3] / v[:, 3:4]).astype(np.float32))
        Xd = X.astype(np.float64)
        err = np.full(nobs, np.nan, np.float32)
        depth = np.full(nobs, np.nan, np.float32)
        tr = np.repeat(np.arange(T), np.diff(track_off))
        ok = (obs_node >= 0) & (obs_node < n)
        nodes = obs_node[ok]
        Pi = np.asarray(P, np.float64).reshape(-1, 12)[image_of(img_off, nodes)]
        x, y = kp[nodes, 0].astype(np.float64), kp[nodes, 1].astype(np.float64)
        xd, yd, zd = Xd[tr[ok], 0], Xd[tr[ok], 1], Xd[tr[ok], 2]
        h = [((Pi[:, 4 * r] * xd + Pi[:, 4 * r + 1] * yd) + Pi[:, 4 * r + 2] * zd) + Pi[:, 4 * r + 3] for r in range(3)]
        du, dv = h[0] / h[2] - x, h[1] / h[2] - y
        err[ok] = np.sqrt(du * du + dv * dv).astype(np.float32)
        depth[ok] = h[2].astype(np.float32)
        err, depth = canonical(err), canonical(depth)
        front = np.ones(T, bool)
        bad = ~(np.isfinite(depth) & (depth > 0))
        front[tr[bad]] = False
        worst = np.zeros(T, np.float32)
        length = np.diff(track_off)
        for k in range(int(length.max()) if T else 0):
            sel = np.flatnonzero(length > k)
            e = err[track_off[sel] + k]
            m = worst[sel]
            worst[sel] = np.where((e > m) | np.isnan(e), e, m)
        flags = front.astype(np.int32) | (((v[:, 3] != 0.0) & np.isfinite(X).all(axis=1)).astype(np.int32) << 1)
    return X, err, depth, flags, canonical(worst)


def run(store, nq, pair_img, img_off, kp, P, ratio=0.70, keep=None, min_len=2, max_len=2 ** 31 - 1, max_reproj=None):
    """The composition, in the form a sparse bundle adjustment takes: points, obs, cam_idx, pt_idx, track_len, counts."""
    n = int(np.asarray(img_off)[-1])
    edges = match_edges(store, nq, pair_img, img_off, ratio, keep)
    labels = components(edges, n)
    node_track, track_off, obs_node, counts = build(labels, img_off, min_len, max_len)
    X, err, depth, flags, worst = triangulate(track_off, obs_node, img_off, kp, P)
    with np.errstate(invalid="ignore"):
        good = (flags == 3) & (np.ones(len(flags), bool) if max_reproj is None else worst <= np.float32(max_reproj))
    new_id = np.cumsum(good) - 1
    tr = np.repeat(np.arange(len(flags)), np.diff(track_off))
    sel = good[tr]
    nodes = obs_node[sel].astype(np.int64)
    return dict(points=X[good], obs=np.asarray(kp, np.float32).reshape(-1, 2)[nodes], cam_idx=image_of(img_off, nodes).astype(np.int32),
                pt_idx=new_id[tr[sel]].astype(np.int32), track_len=np.diff(track_off)[good].astype(np.int32), counts=counts,
                node_track=node_track, track_off=track_off, obs_node=obs_node, flags=flags, max_err=worst, err=err, depth=depth, X=X)
