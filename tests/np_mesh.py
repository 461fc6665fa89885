"""Float32 NumPy restatement of TSDF fusion and marching tetrahedra (include/sfm_hip.h, "MESH"; docs/mesh.md §2), written from the
specification: vectorised over lattice points, looping over views in the specified order, every constant a np.float32 so that
every operation is a correctly rounded float32 one.  The checker of sfm_tsdf_integrate / sfm_mesh_count / sfm_mesh_extract bit for
bit, and the CPU model of the algorithm (tests/test_mesh_cpu.py).  Imports nothing of the product."""
import numpy as np

F = np.float32
ZERO, ONE, HALF = F(0), F(1), F(0.5)

DIR_MASK = (1, 2, 4, 3, 5, 6, 7)                # direction 0..6 -> offset bitmask (bit 0 +x, bit 1 +y, bit 2 +z)
DIR_INDEX = {m: d for d, m in enumerate(DIR_MASK)}
PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))   # xyz xzy yxz yzx zxy zyx


def _bits(c):
    return np.array([c & 1, c >> 1 & 1, c >> 2 & 1])


def tet_table():
    """The case table from the header's rules -> (corner [6][4] offset bitmasks, ntri [6][16], tri [6][16][2][3][2] corner pairs)."""
    corner = np.zeros((6, 4), np.int64)
    ntri = np.zeros((6, 16), np.int64)
    tri = np.zeros((6, 16, 2, 3, 2), np.int64)
    for t, (e1, e2, _) in enumerate(PERMS):
        corner[t] = [0, 1 << e1, (1 << e1) | (1 << e2), 7]
        pos = [_bits(int(c)) for c in corner[t]]
        for cs in range(16):
            ins = [q for q in range(4) if cs >> q & 1]
            outs = [q for q in range(4) if not cs >> q & 1]
            if len(ins) == 1 or len(outs) == 1:
                c = ins[0] if len(ins) == 1 else outs[0]
                tris = [[(c, o) for o in range(4) if o != c]]
            elif len(ins) == 2:
                (i0, i1), (o0, o1) = ins, outs
                tris = [[(i0, o0), (i0, o1), (i1, o1)], [(i0, o0), (i1, o1), (i1, o0)]]
            else:
                tris = []
            tris = [[tuple(sorted(e)) for e in tr] for tr in tris]
            g = len(ins) * sum(pos[q] for q in outs) - len(outs) * sum(pos[q] for q in ins) if tris else None
            for r, tr in enumerate(tris):
                m = [pos[a] + pos[b] for a, b in tr]
                if np.dot(np.cross(m[1] - m[0], m[2] - m[0]), g) < 0:
                    tr = [tr[0], tr[2], tr[1]]
                tri[t, cs, r] = tr
            ntri[t, cs] = len(tris)
    return corner, ntri, tri


def lattice(origin, voxel, dims):
    """x [1, 1, nx], y [1, ny, 1], z [nz, 1, 1]: ox + (float)i*voxel per axis."""
    nx, ny, nz = dims
    o, v = np.asarray(origin, F), F(voxel)
    return (o[0] + np.arange(nx).astype(F) * v)[None, None, :], (o[1] + np.arange(ny).astype(F) * v)[None, :, None], \
        (o[2] + np.arange(nz).astype(F) * v)[:, None, None]


def tsdf_integrate(depth, P, origin, voxel, dims, trunc, mask=None, bgr=None, S=None, W=None, C=None):
    """sfm_tsdf_integrate: depth [nview][h][w] f32, P [nview][12] f32, mask [nview][h][w] u8 or None, bgr [nview][h][w][3] u8 or None;
    S, W [nz][ny][nx] f32 and C [nz][ny][nx][4] f32 the sums to continue (zeros when None; C only with bgr) -> (S, W, C or None)."""
    nx, ny, nz = dims
    depth = np.asarray(depth, F)
    P = np.asarray(P, F).reshape(-1, 12)
    nview, h, w = depth.shape
    trunc = F(trunc)
    S = np.zeros((nz, ny, nx), F) if S is None else np.array(S, F)
    W = np.zeros((nz, ny, nx), F) if W is None else np.array(W, F)
    if bgr is not None:
        C = np.zeros((nz, ny, nx, 4), F) if C is None else np.array(C, F)
    else:
        C = None
    x, y, z = lattice(origin, voxel, dims)
    for v in range(nview):
        m = P[v]
        p = [((m[4 * r] * x + m[4 * r + 1] * y) + m[4 * r + 2] * z) + m[4 * r + 3] for r in range(3)]
        pos = p[2] > ZERO
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            den = np.where(pos, p[2], ONE)
            u = np.floor(p[0] / den + HALF)
            t = np.floor(p[1] / den + HALF)
        ok = pos & (u >= ZERO) & (u <= F(w - 1)) & (t >= ZERO) & (t <= F(h - 1))
        ui = np.where(ok, u, ZERO).astype(np.int64)
        ti = np.where(ok, t, ZERO).astype(np.int64)
        d = depth[v][ti, ui]
        ok &= d > ZERO
        if mask is not None:
            ok &= np.asarray(mask[v])[ti, ui] != 0
        sdf = d - p[2]
        ok &= ~(sdf < -trunc)
        f = np.minimum(sdf, trunc) / trunc
        S = np.where(ok, S + f, S)
        W = np.where(ok, W + ONE, W)
        if C is not None:
            col = ok & (sdf <= trunc)
            px = np.asarray(bgr[v])[ti, ui].astype(F)
            for ch in range(3):
                C[..., ch] = np.where(col, C[..., ch] + px[..., ch], C[..., ch])
            C[..., 3] = np.where(col, C[..., 3] + ONE, C[..., 3])
    return S.astype(F), W.astype(F), C


def _shift(a, dx, dy, dz, fill):
    """a[k+dz, j+dy, i+dx] at every point, `fill` outside the grid."""
    nz, ny, nx = a.shape[:3]
    out = np.full(a.shape, fill, a.dtype)
    out[:nz - dz, :ny - dy, :nx - dx] = a[dz:, dy:, dx:]
    return out


def extract_mesh(S, W, C, origin, voxel, w_min):
    """sfm_mesh_count + sfm_mesh_extract -> (vertices [m][3] f32, colors [m][3] f32 or None (C None), faces [k][3] int32)."""
    S, W = np.asarray(S, F), np.asarray(W, F)
    nz, ny, nx = S.shape
    n = S.size
    known = W >= F(w_min)
    with np.errstate(divide="ignore", invalid="ignore"):
        Fv = np.where(known, S / np.where(known, W, ONE), ZERO)
    inside = known & (Fv < ZERO)
    offs = [(c & 1, c >> 1 & 1, c >> 2) for c in range(8)]
    Kc = [_shift(known, *o, False).reshape(-1) for o in offs]
    Ic = [_shift(inside, *o, False).reshape(-1) for o in offs]
    Fc = [_shift(Fv, *o, ZERO).reshape(-1) for o in offs]
    cross = np.stack([Kc[0] & Kc[m] & (Ic[0] != Ic[m]) for m in DIR_MASK], 1)          # [n, 7] in (point, direction) order
    eid = (np.cumsum(cross.reshape(-1)) - cross.reshape(-1)).reshape(n, 7)            # exclusive count: the vertex ids
    # vertices
    pidx, didx = np.nonzero(cross)
    ks, rem = np.divmod(pidx, nx * ny)
    js, is_ = np.divmod(rem, nx)
    ox, oy, oz = np.asarray(origin, F)
    vx = F(voxel)
    msk = np.array(DIR_MASK)[didx]
    dx, dy, dz = msk & 1, msk >> 1 & 1, msk >> 2
    Fa = np.stack(Fc, 1)[pidx, 0]
    Fb = np.stack(Fc, 1)[pidx, msk]
    t = Fa / (Fa - Fb)
    verts = np.empty((len(pidx), 3), F)
    for ax, (o, c0, dc) in enumerate(((ox, is_, dx), (oy, js, dy), (oz, ks, dz))):
        xa = o + c0.astype(F) * vx
        xb = o + (c0 + dc).astype(F) * vx
        verts[:, ax] = xa + t * (xb - xa)
    cols = None
    if C is not None:
        C = np.asarray(C, F).reshape(n, 4)
        with np.errstate(divide="ignore", invalid="ignore"):
            cpt = np.where((C[:, 3] != ZERO)[:, None], C[:, :3] / np.where(C[:, 3] != ZERO, C[:, 3], ONE)[:, None], ZERO).astype(F)
        pb = pidx + dx + dy * nx + dz * nx * ny
        ca, cb = cpt[pidx], cpt[pb]
        cols = (ca + t[:, None] * (cb - ca)).astype(F)
    # triangles
    corner, ntri, tri = tet_table()
    p = np.arange(n)
    pk, prem = np.divmod(p, nx * ny)
    pj, pi = np.divmod(prem, nx)
    is_cube = (pi < nx - 1) & (pj < ny - 1) & (pk < nz - 1)
    step = np.array([1, nx, nx * ny])
    ids = np.zeros((n, 6, 2, 3), np.int64)
    valid = np.zeros((n, 6, 2), bool)
    for tt in range(6):
        allk = is_cube.copy()
        cs = np.zeros(n, np.int64)
        for q in range(4):
            allk &= Kc[corner[tt, q]]
            cs |= Ic[corner[tt, q]].astype(np.int64) << q
        for r in range(2):
            valid[:, tt, r] = allk & (ntri[tt, cs] > r)
            for q in range(3):
                a = corner[tt][tri[tt, cs, r, q, 0]]
                b = corner[tt][tri[tt, cs, r, q, 1]]
                pa = p + (a & 1) * step[0] + (a >> 1 & 1) * step[1] + (a >> 2) * step[2]
                d = np.array([DIR_INDEX.get(int(mm), 0) for mm in range(8)])[b & ~a]
                ids[:, tt, r, q] = eid[np.minimum(pa, n - 1), d]
    faces = ids[valid].astype(np.int32).reshape(-1, 3)
    return verts, cols, faces

