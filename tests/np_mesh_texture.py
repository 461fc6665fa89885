"""NumPy restatement of the mesh texturing step (include/sfm_hip.h, "MESH-TEXTURE"; docs/mesh.md §10), written from the header
alone: float32 throughout with explicit casts, every operation in the header's order.  It stands apart from the product (no
import of sfm_mvs_amd) and is what the GPU tests compare with bit for bit.

  render_depth(v, f, P, w, h, counts)                      -> zbuf (n, h, w) float32
  face_views(v, f, P, zbuf, vis_tol, counts)               -> face_view int32 (nf,), face_score float32 (nf,) of the counted rows
  texture_fill(v, c, f, P, frames, face_view, L, counts)   -> atlas (side, side, 3) uint8
  layout(nf, L)                                            -> side, cols, cell
The rasteriser is vectorised over the faces per bounding-box offset (np.minimum.at on the uint32 bits of the map); faces with a
box wider or taller than SMALL pixels are walked one by one, vectorised over their pixels."""
import numpy as np

F = np.float32
SMALL = 12
ONE, ZERO, THREE = F(1.0), F(0.0), F(3.0)


def counts_of(counts, nv_cap, nf_cap):
    nv, nf = nv_cap, nf_cap
    if counts is not None:
        if 0 <= int(counts[0]) <= nv_cap:
            nv = int(counts[0])
        if 0 <= int(counts[1]) <= nf_cap:
            nf = int(counts[1])
    return nv, nf


def valid_faces(f, nv, nf):
    """bool (nf_cap,): among the first nf, the three indices in 0..nv-1."""
    f = np.asarray(f, np.int32).reshape(-1, 3)
    ok = np.all((f >= 0) & (f < nv), axis=1)
    ok[nf:] = False
    return ok


def project(P, X):
    """P (12,) float32, X (..., 3) float32 -> sx, sy, z, projectable."""
    P = np.asarray(P, F).reshape(12)
    x, y, z = X[..., 0], X[..., 1], X[..., 2]
    with np.errstate(all="ignore"):
        p = [((P[4 * r] * x + P[4 * r + 1] * y) + P[4 * r + 2] * z) + P[4 * r + 3] for r in range(3)]
        sx, sy = p[0] / p[2], p[1] / p[2]
    ok = (p[2] > 0) & np.isfinite(sx) & np.isfinite(sy) & np.isfinite(p[2])
    return sx.astype(F), sy.astype(F), p[2].astype(F), ok


def _edge(ax, ay, bx, by, x, y):
    return (bx - ax) * (y - ay) - (by - ay) * (x - ax)


def _shade(zu, base, w, t, x, y):
    """Pixels (x, y) (int arrays, in the frame) of the triangles t (tuple of arrays or scalars broadcasting with them)."""
    ax, ay, bx, by, cx, cy, ia, ib, ic, area2 = t
    fx, fy = x.astype(F), y.astype(F)
    with np.errstate(all="ignore"):
        wa, wb, wc = _edge(bx, by, cx, cy, fx, fy), _edge(cx, cy, ax, ay, fx, fy), _edge(ax, ay, bx, by, fx, fy)
        cov = np.where(area2 > 0, (wa >= 0) & (wb >= 0) & (wc >= 0), (wa <= 0) & (wb <= 0) & (wc <= 0))
        iz = ((wa * ia + wb * ib) + wc * ic) / area2
        d = (ONE / iz).astype(F)
    hit = cov & np.isfinite(d) & (d > 0)
    if np.any(hit):
        idx = base + y[hit].astype(np.int64) * w + x[hit].astype(np.int64)
        np.minimum.at(zu, idx, np.broadcast_to(d, hit.shape)[hit].view(np.uint32))


def render_depth(v, f, P, w, h, counts=None, stats=None):
    v = np.ascontiguousarray(v, F).reshape(-1, 3)
    f = np.ascontiguousarray(f, np.int32).reshape(-1, 3)
    P = np.ascontiguousarray(P, F).reshape(-1, 12)
    n = len(P)
    nv, nf = counts_of(counts, len(v), len(f))
    z = np.full((n, h, w), np.inf, F)
    zu = z.reshape(-1).view(np.uint32)
    ok = valid_faces(f, nv, nf)
    ff = f[ok]
    if len(ff) == 0:
        return z
    for k in range(n):
        sx, sy, sz, pr = project(P[k], v)
        a, b, c = ff[:, 0], ff[:, 1], ff[:, 2]
        use = pr[a] & pr[b] & pr[c]
        ax, ay, bx, by, cx, cy = sx[a], sy[a], sx[b], sy[b], sx[c], sy[c]
        with np.errstate(all="ignore"):
            area2 = _edge(ax, ay, bx, by, cx, cy)
            use &= (area2 < 0) | (area2 > 0)
            lox = np.maximum(ZERO, np.ceil(np.minimum(np.minimum(ax, bx), cx)))
            hix = np.minimum(F(w - 1), np.floor(np.maximum(np.maximum(ax, bx), cx)))
            loy = np.maximum(ZERO, np.ceil(np.minimum(np.minimum(ay, by), cy)))
            hiy = np.minimum(F(h - 1), np.floor(np.maximum(np.maximum(ay, by), cy)))
            use &= (lox <= hix) & (loy <= hiy)
            ia, ib, ic = ONE / sz[a], ONE / sz[b], ONE / sz[c]
        s = np.flatnonzero(use)
        if len(s) == 0:
            continue
        t = [q[s] for q in (ax, ay, bx, by, cx, cy, ia, ib, ic, area2)]
        x0, y0 = lox[s].astype(np.int64), loy[s].astype(np.int64)
        bw, bh = hix[s].astype(np.int64) - x0 + 1, hiy[s].astype(np.int64) - y0 + 1
        small = (bw <= SMALL) & (bh <= SMALL)
        if stats is not None:
            stats["boxes"] = stats.get("boxes", 0) + len(s)
            stats["over_64"] = stats.get("over_64", 0) + int((bw * bh > 64).sum())
        base = k * h * w
        m = np.flatnonzero(small)
        if len(m):
            tm = [q[m] for q in t]
            for dy in range(int(bh[m].max())):
                for dx in range(int(bw[m].max())):
                    g = (dx < bw[m]) & (dy < bh[m])
                    if np.any(g):
                        _shade(zu, base, w, [q[g] for q in tm], x0[m][g] + dx, y0[m][g] + dy)
        for i in np.flatnonzero(~small):
            ys, xs = np.mgrid[y0[i]:y0[i] + bh[i], x0[i]:x0[i] + bw[i]]
            _shade(zu, base, w, [q[i] for q in t], xs.reshape(-1), ys.reshape(-1))
    return z


def _visible(sx, sy, sz, pr, zk, w, h, tol1):
    with np.errstate(all="ignore"):
        px, py = np.rint(sx), np.rint(sy)
        inside = pr & (px >= 0) & (px <= F(w - 1)) & (py >= 0) & (py <= F(h - 1))
        ix, iy = np.where(inside, px, 0).astype(np.int64), np.where(inside, py, 0).astype(np.int64)
        return inside & (sz <= zk[iy, ix] * tol1)


def view_tests(v, f, P, zbuf, vis_tol, counts=None):
    """Per view k, over the valid faces: yields (k, rows, facing, visible, score, centroid) with rows the indices of the valid faces,
    facing = the three corners projectable, in the frame and area2 < 0, visible = the four samples pass the depth test, score =
    -area2 and centroid = (sx, sy, depth, projectable) of the centroid.  A face is a candidate of view k iff facing & visible."""
    v = np.ascontiguousarray(v, F).reshape(-1, 3)
    f = np.ascontiguousarray(f, np.int32).reshape(-1, 3)
    P = np.ascontiguousarray(P, F).reshape(-1, 12)
    n, h, w = zbuf.shape
    nv, nf = counts_of(counts, len(v), len(f))
    s = np.flatnonzero(valid_faces(f, nv, nf))
    ff = f[s]
    A, B, C = v[ff[:, 0]], v[ff[:, 1]], v[ff[:, 2]]
    with np.errstate(all="ignore"):
        G = (((A + B) + C) / THREE).astype(F)
    tol1 = F(ONE + F(vis_tol))
    for k in range(n):
        pa, pb, pc, pg = project(P[k], A), project(P[k], B), project(P[k], C), project(P[k], G)
        facing = pa[3] & pb[3] & pc[3]
        with np.errstate(all="ignore"):
            for q in (pa, pb, pc):
                facing &= (q[0] >= 0) & (q[0] <= F(w - 1)) & (q[1] >= 0) & (q[1] <= F(h - 1))
            area2 = _edge(pa[0], pa[1], pb[0], pb[1], pc[0], pc[1])
            facing &= area2 < 0
            score = (-area2).astype(F)
        vis = np.ones(len(s), bool)
        for q in (pa, pb, pc, pg):
            vis &= _visible(q[0], q[1], q[2], q[3], zbuf[k], w, h, tol1)
        yield k, s, facing, vis, score, pg


def samples_at_the_bound(v, f, P, zbuf, vis_tol, counts=None):
    """How many of the four samples of the facing (face, view) pairs have depth == zbuf * (1 + vis_tol) exactly."""
    v = np.ascontiguousarray(v, F).reshape(-1, 3)
    f = np.ascontiguousarray(f, np.int32).reshape(-1, 3)
    n, h, w = zbuf.shape
    tol1, hits = F(ONE + F(vis_tol)), 0
    for k, s, facing, _, _, pg in view_tests(v, f, P, zbuf, vis_tol, counts):
        ff = f[s]
        for X in (v[ff[:, 0]], v[ff[:, 1]], v[ff[:, 2]], None):
            sx, sy, sz, pr = pg if X is None else project(np.ascontiguousarray(P, F).reshape(-1, 12)[k], X)
            with np.errstate(all="ignore"):
                px, py = np.rint(sx), np.rint(sy)
                at = facing & pr & (px >= 0) & (px <= F(w - 1)) & (py >= 0) & (py <= F(h - 1))
                zz = zbuf[k][np.where(at, py, 0).astype(np.int64), np.where(at, px, 0).astype(np.int64)] * tol1
            hits += int((at & (sz == zz)).sum())
    return hits


def face_views(v, f, P, zbuf, vis_tol, counts=None):
    """-> (face_view int32 (nf,), face_score float32 (nf,)) of the first nf faces."""
    nv, nf = counts_of(counts, len(np.asarray(v).reshape(-1, 3)), len(np.asarray(f).reshape(-1, 3)))
    best, score = np.full(nf, -1, np.int32), np.zeros(nf, F)
    for k, s, facing, vis, sc, _ in view_tests(v, f, P, zbuf, vis_tol, counts):
        better = facing & vis & (sc > score[s])
        best[s[better]] = k
        score[s[better]] = sc[better]
    return best, score


def texel_faces(nf_cap, L):
    """Per texel of the atlas, (side, side) arrays: the face that owns it (maybe >= nf_cap), i, j in its cell, its half, and
    whether it lies inside the chart's triangle proper (0 <= u, 0 <= v, u + v <= 1) rather than in the dilated margin."""
    side, cols, cell = layout(nf_cap, L)
    ty, tx = np.mgrid[0:side, 0:side]
    i, j = tx % cell, ty % cell
    half = (i + j > cell - 1).astype(np.int64)
    face = 2 * ((ty // cell) * cols + tx // cell) + half
    a, b = np.where(half == 1, cell - 2 - i, i - 1), np.where(half == 1, cell - 2 - j, j - 1)
    return face, i, j, half, (a >= 0) & (b >= 0) & (a + b <= L)


def layout(nf, L):
    """-> (side, cols, cell) of the atlas of nf faces at L texels per leg."""
    nf, L = int(nf), int(L)
    slots = (nf + 1) // 2
    cols = int(np.floor(np.sqrt(float(slots))))
    while cols * cols < slots:
        cols += 1
    while cols > 1 and (cols - 1) * (cols - 1) >= slots:
        cols -= 1
    cols = max(cols, 1)
    return cols * (L + 5), cols, L + 5


def _clamp(x, hi):
    with np.errstate(all="ignore"):
        x = np.where(x >= 0, x, ZERO).astype(F)
        return np.where(x <= hi, x, hi).astype(F)


def texture_fill(v, c, f, P, frames, face_view, L, counts=None):
    v = np.ascontiguousarray(v, F).reshape(-1, 3)
    f = np.ascontiguousarray(f, np.int32).reshape(-1, 3)
    P = np.ascontiguousarray(P, F).reshape(-1, 12)
    frames = np.ascontiguousarray(frames, np.uint8)
    n, h, w = frames.shape[:3]
    nv, nf = counts_of(counts, len(v), len(f))
    side, cols, cell = layout(len(f), L)
    face, i, j, half, _ = texel_faces(len(f), L)
    ok = face < nf
    okf = valid_faces(f, nv, nf)
    ok &= okf[np.where(ok, face, 0)] if len(f) else False
    atlas = np.zeros((side, side, 3), np.uint8)
    s = np.nonzero(ok)
    if len(s[0]) == 0:
        return atlas
    fi, ii, jj, hh = face[s], i[s], j[s], half[s]
    fl = F(L)
    u = (np.where(hh == 1, cell - 2 - ii, ii - 1).astype(F) / fl).astype(F)
    vv = (np.where(hh == 1, cell - 2 - jj, jj - 1).astype(F) / fl).astype(F)
    w0 = (ONE - u) - vv
    tri = f[fi]
    val = np.zeros((len(fi), 3), F)
    fview = np.asarray(face_view, np.int32)[fi]
    tex = (fview >= 0) & (fview < n)
    with np.errstate(all="ignore"):
        if c is not None:
            c = np.ascontiguousarray(c, F).reshape(-1, 3)
            m = ~tex
            val[m] = (w0[m, None] * c[tri[m, 0]] + u[m, None] * c[tri[m, 1]]) + vv[m, None] * c[tri[m, 2]]
        for k in np.unique(fview[tex]):
            m = np.flatnonzero(tex & (fview == k))
            X = (w0[m, None] * v[tri[m, 0]] + u[m, None] * v[tri[m, 1]]) + vv[m, None] * v[tri[m, 2]]
            sx, sy, _, _ = project(P[k], X.astype(F))
            sx, sy = _clamp(sx, F(w - 1)), _clamp(sy, F(h - 1))
            x0 = np.minimum(np.floor(sx).astype(np.int64), w - 2)
            y0 = np.minimum(np.floor(sy).astype(np.int64), h - 2)
            fx, fy = (sx - x0.astype(F))[:, None], (sy - y0.astype(F))[:, None]
            img = frames[k].astype(F)
            p00, p10, p01, p11 = img[y0, x0], img[y0, x0 + 1], img[y0 + 1, x0], img[y0 + 1, x0 + 1]
            val[m] = ((p00 * (ONE - fx) + p10 * fx) * (ONE - fy)) + ((p01 * (ONE - fx) + p11 * fx) * fy)
        out = _clamp(np.rint(val), F(255.0))
    atlas[s] = out.astype(np.uint8)
    return atlas


def uv_of(nf, L):
    """(nf, 3, 2) float64: the texture coordinates of the three corners of every face, v up."""
    side, cols, cell = layout(nf, L)
    fidx = np.arange(int(nf))
    q, half = fidx >> 1, fidx & 1
    ox, oy = (q % cols) * cell, (q // cols) * cell
    ci = np.where(half[:, None] == 0, np.array([1, 1 + L, 1]), np.array([cell - 2, cell - 2 - L, cell - 2]))
    cj = np.where(half[:, None] == 0, np.array([1, 1, 1 + L]), np.array([cell - 2, cell - 2, cell - 2 - L]))
    return np.stack([(ox[:, None] + ci + 0.5) / side, 1.0 - (oy[:, None] + cj + 0.5) / side], -1)
