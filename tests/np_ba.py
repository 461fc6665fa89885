"""Float64 NumPy reference for the bundle-adjustment linear algebra (csrc/ba_schur.hip): projection, its Jacobians by
complex-step differentiation, the products with the camera-point coupling W, and the damped Schur step (direct and PCG);
and for the Gauss-Newton sweeps and RANSAC scoring (csrc/residual.hip, csrc/ba_dense.hip, project_f64_kernel): the
normal-equation blocks dense and indexed, both sums of squares, and inlier masks that take the kernels' float32 steps
exactly and name the entries whose float32 rounding a last-bit difference in double could flip.
Shares no code with the kernels or the C oracle.

Complex step: for an analytic f, Im f(x + ih) / h = f'(x) + O(h^2) with NO subtraction of nearly equal numbers, so with
h = 1e-30 the derivative is exact to the rounding of f itself.  Everything on the path from the parameters to the pixel
is therefore written so that it accepts complex input: theta^2 = r.r (no conjugate, no abs, no norm), branches look at
real parts only.

X always enters as float64(float32 X): exactly what the kernels read."""
import numpy as np

H = 1e-30


def _coeffs(t):
    """A = sin(th)/th and B = (1 - cos th)/th^2 as functions of t = th^2 (complex allowed).  |th| < 1e-4: Taylor series in t
    (the first omitted terms are t^4/362880 and t^4/3628800: < 1e-37) — exact to rounding at th = 0 and for tiny angles;
    elsewhere B = 2 sin^2(th/2)/th^2, which does not cancel."""
    t = np.asarray(t)
    small = np.abs(t) < 1e-8
    ts = np.where(small, t, 0)
    A_s = 1 - ts / 6 * (1 - ts / 20 * (1 - ts / 42))
    B_s = 0.5 - ts / 24 * (1 - ts / 30 * (1 - ts / 56))
    tl = np.where(small, 1.0, t)
    th = np.sqrt(tl)
    sh = np.sin(0.5 * th)
    return np.where(small, A_s, np.sin(th) / th), np.where(small, B_s, 2 * sh * sh / tl)


def rotation(r):
    """Rodrigues: r [..., 3] (real or complex) -> R [..., 3, 3] = I + A [r]x + B [r]x^2."""
    r = np.asarray(r)
    t = r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1] + r[..., 2] * r[..., 2]
    A, B = _coeffs(t)
    z = np.zeros_like(t)
    Kx = np.stack([np.stack([z, -r[..., 2], r[..., 1]], -1),
                   np.stack([r[..., 2], z, -r[..., 0]], -1),
                   np.stack([-r[..., 1], r[..., 0], z], -1)], -2)
    eye = np.eye(3, dtype=Kx.dtype)
    return eye + A[..., None, None] * Kx + B[..., None, None] * (Kx @ Kx)


def project(cams, K, X):
    """cams [ncam, 6] (rvec, tvec), X [npt, 3] or [ncam, npt, 3] -> pixels [ncam, npt, 2].  The kernels' and OpenCV's
    `z ? 1/z : 1` convention: a point exactly in the camera plane gets inverse depth 1.  OpenCV (and the kernels) then push
    that 1 through the usual derivative formulas, i.e. they use g(0) = 1, g'(0) = -1 for g(z) = 1/z; under the complex
    step this is g(z) = 1 - z on the set Re z = 0, which is what is evaluated here."""
    cams, X = np.asarray(cams), np.asarray(X)
    R = rotation(cams[:, :3])
    if X.ndim == 2:
        Xc = np.einsum("iab,jb->ija", R, X) + cams[:, None, 3:]
    else:
        Xc = np.einsum("iab,ijb->ija", R, X) + cams[:, None, 3:]
    z = Xc[..., 2]
    flat = np.real(z) == 0
    iz = np.where(flat, 1 - z, 1 / np.where(flat, 1, z))
    return np.stack([K[0, 0] * (Xc[..., 0] * iz) + K[0, 2], K[1, 1] * (Xc[..., 1] * iz) + K[1, 2]], -1)


def as_f64(X):
    """float64(float32 X[:, :3])."""
    return np.asarray(X, np.float32)[:, :3].astype(np.float64)


def jacobians(cams, K, X, cam_sel=None, pt_sel=None, which="cp"):
    """Complex-step Jacobians of the projection for the cameras cam_sel x the points pt_sel (default: all):
    Jc [nc, np, 2, 6] = d(u, v)/d(rvec, tvec),  Jp [nc, np, 2, 3] = d(u, v)/dX.  which: "c" or "p" evaluates one side only
    (the other is returned as None)."""
    cams = np.asarray(cams, np.float64).reshape(-1, 6)
    X = as_f64(X)
    if cam_sel is not None:
        cams = cams[np.asarray(cam_sel)]
    if pt_sel is not None:
        X = X[np.asarray(pt_sel)]
    nc, npts = len(cams), len(X)
    Jc = np.empty((nc, npts, 2, 6)) if "c" in which else None
    Jp = np.empty((nc, npts, 2, 3)) if "p" in which else None
    for a in range(6 if Jc is not None else 0):
        c = cams.astype(np.complex128)
        c[:, a] += 1j * H
        Jc[..., a] = project(c, K, X).imag / H
    for a in range(3 if Jp is not None else 0):
        x = X.astype(np.complex128)
        x[:, a] += 1j * H
        Jp[..., a] = project(cams, K, x).imag / H
    return Jc, Jp


def pair_jacobians(cams, K, X, cam_idx, pt_idx):
    """The same Jacobians for a list of observations (cam_idx[o], pt_idx[o]): Jc [nobs, 2, 6], Jp [nobs, 2, 3]."""
    cams = np.asarray(cams, np.float64).reshape(-1, 6)[np.asarray(cam_idx, np.int64)]
    X = as_f64(X)[np.asarray(pt_idx, np.int64)]
    n = len(cams)
    Jc, Jp = np.empty((n, 2, 6)), np.empty((n, 2, 3))
    for a in range(6):
        c = cams.astype(np.complex128)
        c[:, a] += 1j * H
        Jc[..., a] = project(c, K, X[:, None, :]).imag[:, 0] / H
    for a in range(3):
        x = X.astype(np.complex128)
        x[:, a] += 1j * H
        Jp[..., a] = project(cams, K, x[:, None, :]).imag[:, 0] / H
    return Jc, Jp


def _ordered_sum(terms, axis, reverse):
    """Sum along `axis` one slice after the other, ascending or descending: a DEFINED order (np.sum's is not)."""
    terms = np.moveaxis(terms, axis, 0)
    acc = np.zeros(terms.shape[1:])
    for t in (terms[::-1] if reverse else terms):
        acc = acc + t
    return acc


def wt_product(cams, K, X, x, pt_sel=None, reverse=False, magnitude=False, cam_block=64):
    """u = W^T x for the points pt_sel (default all): u_j = sum_i Jp_ij^T (Jc_ij x_i) — every camera, so exact per point.
    reverse: add the cameras in descending order (None: return both orders, the Jacobians evaluated once).  magnitude: sum_i |Jp_ij|^T (|Jc_ij| |x_i|) instead, the scale against
    which the rounding of u_j is measured when the entries of u differ by many orders of magnitude."""
    cams = np.asarray(cams, np.float64).reshape(-1, 6)
    ncam = len(cams)
    terms = []
    for c0 in range(0, ncam, cam_block):
        sel = np.arange(c0, min(ncam, c0 + cam_block))
        Jc, Jp = jacobians(cams, K, X, sel, pt_sel)
        if magnitude:
            Jc, Jp, x = np.abs(Jc), np.abs(Jp), np.abs(x)
        terms.append(np.einsum("ijkb,ijk->ijb", Jp, np.einsum("ijka,ia->ijk", Jc, x[sel])))
    terms = np.concatenate(terms, 0)
    if reverse is None:
        return _ordered_sum(terms, 0, False), _ordered_sum(terms, 0, True)
    return _ordered_sum(terms, 0, reverse)


def w_product(cams, K, X, v, cam_sel=None, reverse=False, magnitude=False, pt_block=1 << 16):
    """w = W v for the cameras cam_sel (default all): w_i = sum_j Jc_ij^T (Jp_ij v_j) — every point, so exact per camera.
    reverse: add the points in descending order (block partial sums keep the loop short; within a block NumPy adds along
    the point axis in memory order of the reversed or unreversed view).  magnitude: as in wt_product."""
    npt = len(X)
    blocks = []
    for p0 in range(0, npt, pt_block):
        sel = np.arange(p0, min(npt, p0 + pt_block))
        Jc, Jp = jacobians(cams, K, X, cam_sel, sel)
        if magnitude:
            Jc, Jp, v = np.abs(Jc), np.abs(Jp), np.abs(v)
        t = np.einsum("ijka,ijk->ija", Jc, np.einsum("ijkb,jb->ijk", Jp, v[sel]))
        blocks.append([np.add.reduce(t[:, ::-1] if r else t, axis=1) for r in ((False, True) if reverse is None else (reverse,))])
    sums = [_ordered_sum(np.stack([b[k] for b in blocks], 0), 0, r) for k, r in enumerate((False, True) if reverse is None else (reverse,))]
    return tuple(sums) if reverse is None else sums[0]


def indexed_products(cams, K, X, cam_idx, pt_idx, x, v, reverse=False):
    """(W^T x [npt, 3], W v [ncam, 6]) restricted to the listed observations; a repeated observation counts twice."""
    ncam, npt = len(np.asarray(cams).reshape(-1, 6)), len(X)
    ci, pi = np.asarray(cam_idx, np.int64), np.asarray(pt_idx, np.int64)
    u, w = np.zeros((npt, 3)), np.zeros((ncam, 6))
    if len(ci) == 0:
        return u, w
    Jc, Jp = pair_jacobians(cams, K, X, ci, pi)
    tu = np.einsum("okb,ok->ob", Jp, np.einsum("oka,oa->ok", Jc, x[ci]))
    tw = np.einsum("oka,ok->oa", Jc, np.einsum("okb,ob->ok", Jp, v[pi]))
    order = np.arange(len(ci))[::-1] if reverse else np.arange(len(ci))
    np.add.at(u, pi[order], tu[order])            # ufunc.at adds unbuffered, in the order given
    np.add.at(w, ci[order], tw[order])
    return u, w


def normal_blocks(cams, K, X, obs, want_w=True, pt_block=None, reverse=False, magnitude=False, pt_rows=None):
    """B [ncam, 6, 6], C [npt, 3, 3], g_c [ncam, 6], g_p [npt, 3], sumsq (the float64 residual's: `res2`) and
    W [ncam, npt, 6, 3] of the dense problem; residual = projection - observation.

    want_w=False: W is None.  pt_block: work through the points in blocks of that many — nothing of size ncam x npt x 36 is
    ever held — and add in a DEFINED order: a camera's sums run over the points ascending (reverse=True: descending; within
    a block along the point axis of the reversed or unreversed view, then block after block), a point's sums over the
    cameras ascending or descending.  reverse=None: both orders, as a pair of result tuples, the Jacobians evaluated once.
    magnitude: the sums of |Jc|^T |Jc|, |Jc|^T |r| ... instead, the scale of each row's rounding.  pt_rows (sorted point
    indices): C and g_p for those points only (the camera sums still run over every point)."""
    cams = np.asarray(cams, np.float64).reshape(-1, 6)
    Xd = as_f64(X)
    ncam, npt = len(cams), len(Xd)
    obs = np.asarray(obs, np.float64).reshape(ncam, npt, 2)
    if pt_block is None and reverse is False and not magnitude and pt_rows is None:
        Jc, Jp = jacobians(cams, K, X)
        r = project(cams, K, Xd) - obs
        B = np.einsum("ijka,ijkb->iab", Jc, Jc)
        C = np.einsum("ijka,ijkb->jab", Jp, Jp)
        gc = np.einsum("ijka,ijk->ia", Jc, r)
        gp = np.einsum("ijka,ijk->ja", Jp, r)
        W = np.einsum("ijka,ijkb->ijab", Jc, Jp) if want_w else None
        return B, C, gc, gp, float((r * r).sum()), W
    orders = (False, True) if reverse is None else (bool(reverse),)
    step = pt_block or max(npt, 1)
    cam_side = {o: [] for o in orders}
    pt_side = {o: [] for o in orders}
    Ws = []
    for p0 in range(0, npt, step):
        sel = np.arange(p0, min(npt, p0 + step))
        Jc, Jp = jacobians(cams, K, X, None, sel, "cp" if pt_rows is None or want_w else "c")
        r = project(cams, K, Xd[sel]) - obs[:, sel]
        if want_w:
            Ws.append(np.einsum("ijka,ijkb->ijab", Jc, Jp))
        if magnitude:
            Jc, r = np.abs(Jc), np.abs(r)
        tB, tg, tr = np.einsum("ijka,ijkb->ijab", Jc, Jc), np.einsum("ijka,ijk->ija", Jc, r), (r * r).sum(-1)
        for o in orders:
            cam_side[o].append([np.add.reduce(t[:, ::-1] if o else t, axis=1) for t in (tB, tg, tr)])
        if pt_rows is None:
            Jp = np.abs(Jp) if magnitude else Jp
            tC, tp = np.einsum("ijka,ijkb->ijab", Jp, Jp), np.einsum("ijka,ijk->ija", Jp, r)
            for o in orders:
                pt_side[o].append((_ordered_sum(tC, 0, o), _ordered_sum(tp, 0, o)))
    if pt_rows is not None:
        rows = np.asarray(pt_rows, np.int64)
        _, Jp = jacobians(cams, K, X, None, rows, "p")
        r = project(cams, K, Xd[rows]) - obs[:, rows]
        if magnitude:
            Jp, r = np.abs(Jp), np.abs(r)
        tC, tp = np.einsum("ijka,ijkb->ijab", Jp, Jp), np.einsum("ijka,ijk->ija", Jp, r)
        for o in orders:
            pt_side[o].append((_ordered_sum(tC, 0, o), _ordered_sum(tp, 0, o)))
    W = np.concatenate(Ws, 1) if want_w else None
    out = []
    for o in orders:
        B, gc, res2 = (_ordered_sum(np.stack([blk[k] for blk in cam_side[o]], 0), 0, o) for k in range(3))
        C, gp = (np.concatenate([blk[k] for blk in pt_side[o]], 0) for k in range(2))
        out.append((B, C, gc, gp, float(_ordered_sum(res2, 0, o)), W))
    return tuple(out) if reverse is None else out[0]


def indexed_normal_blocks(cams, K, X, obs, cam_idx=None, pt_idx=None, reverse=False, magnitude=False):
    """B [ncam, 6, 6], C [npt, 3, 3], g_c [ncam, 6], g_p [npt, 3] and res2 summed over the listed observations
    (cam_idx[o], pt_idx[o]) with obs [nobs, 2]; a repeated observation counts twice.  cam_idx None: camera 0 throughout;
    pt_idx None: observation o is of point o.  reverse: add the observations in descending order."""
    cams = np.asarray(cams, np.float64).reshape(-1, 6)
    obs = np.asarray(obs, np.float64).reshape(-1, 2)
    ncam, npt, nobs = len(cams), len(X), len(obs)
    ci = np.zeros(nobs, np.int64) if cam_idx is None else np.asarray(cam_idx, np.int64)
    pi = np.arange(nobs) if pt_idx is None else np.asarray(pt_idx, np.int64)
    B, C, gc, gp = np.zeros((ncam, 6, 6)), np.zeros((npt, 3, 3)), np.zeros((ncam, 6)), np.zeros((npt, 3))
    if nobs == 0:
        return B, C, gc, gp, 0.0
    Jc, Jp = pair_jacobians(cams, K, X, ci, pi)
    r = pair_project(cams, K, X, ci, pi) - obs
    if magnitude:
        Jc, Jp, r = np.abs(Jc), np.abs(Jp), np.abs(r)
    order = np.arange(nobs)[::-1] if reverse else np.arange(nobs)
    np.add.at(B, ci[order], np.einsum("oka,okb->oab", Jc, Jc)[order])            # ufunc.at adds unbuffered, in the order given
    np.add.at(gc, ci[order], np.einsum("oka,ok->oa", Jc, r)[order])
    np.add.at(C, pi[order], np.einsum("oka,okb->oab", Jp, Jp)[order])
    np.add.at(gp, pi[order], np.einsum("oka,ok->oa", Jp, r)[order])
    return B, C, gc, gp, float(np.cumsum((r * r).sum(1)[order])[-1])


def pair_project(cams, K, X, cam_idx, pt_idx):
    """Float64 pixels [nobs, 2] of the observations (cam_idx[o], pt_idx[o])."""
    cams = np.asarray(cams, np.float64).reshape(-1, 6)[np.asarray(cam_idx, np.int64)]
    return project(cams, K, as_f64(X)[np.asarray(pt_idx, np.int64)][:, None, :])[:, 0]


# ---------------------------------------------------------------- the float32 steps of the residual and scoring kernels
DBL_EPSILON = 2.0 ** -52


def project_points(rvec, tvec, K, X):
    """cv2.projectPoints without distortion on float64 points X [n, 3] (NOT rounded to float32) -> [n, 2] float64, with
    OpenCV's two conventions: z' = 0 -> z := 1 (project) and cv::Rodrigues' |rvec| < DBL_EPSILON -> R = I exactly."""
    rvec = np.asarray(rvec, np.float64).reshape(3)
    if np.sqrt(rvec @ rvec) < DBL_EPSILON:
        rvec = np.zeros(3)
    return project(np.hstack([rvec, np.asarray(tvec, np.float64).reshape(3)])[None], K, np.asarray(X, np.float64).reshape(-1, 3))[0]


def f32_undecidable(v, rel=1e-12):
    """True where the float64 value v lies within rel |v| of the midpoint between two neighbouring float32 values: there a
    last-bit difference of v in double can flip its float32 rounding."""
    v = np.asarray(v, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        f = v.astype(np.float32)
        lo = np.nextafter(f, np.float32(-np.inf)).astype(np.float64)
        hi = np.nextafter(f, np.float32(np.inf)).astype(np.float64)
        f = f.astype(np.float64)
        d = np.minimum(np.abs(v - 0.5 * (f + lo)), np.abs(v - 0.5 * (f + hi)))
        return d <= rel * np.abs(v)


def sumsq(u, obs, reverse=False):
    """(float32-rounded metric, float64 res2) of float64 pixels u [..., 2] against float32 observations.  The metric:
    pu = float32(u), d = float32(pu - obs), squares summed in double — what residual_kernel and the reference's cv2.norm on
    float32 arrays compute; res2 is the plain sum of (u - obs)^2.  Observations are added ascending (reverse: descending)."""
    u = np.asarray(u, np.float64).reshape(-1, 2)
    o32 = np.asarray(obs, np.float32).reshape(-1, 2)
    d32 = (u.astype(np.float32) - o32).astype(np.float64)                       # float32 - float32: one correctly rounded float32 step
    d64 = u - o32.astype(np.float64)
    t32, t64 = (d32 * d32).sum(1), (d64 * d64).sum(1)
    if reverse:
        t32, t64 = t32[::-1], t64[::-1]
    return (float(np.cumsum(t32)[-1]), float(np.cumsum(t64)[-1])) if len(u) else (0.0, 0.0)


def sumsq_flip_allowance(u, obs):
    """The most the float32 metric can move if every undecidable coordinate of u rounds the other way: pu moves by one
    float32 spacing s, d = pu - obs by s (+ its own rounding, s / 2 at the most), d^2 by at most 2 |d| (1.5 s) + (1.5 s)^2."""
    u = np.asarray(u, np.float64).reshape(-1, 2)
    und = f32_undecidable(u)
    if not und.any():
        return 0.0
    uu = u[und]
    f = uu.astype(np.float32)
    s = 1.5 * np.maximum(np.nextafter(f, np.float32(np.inf)).astype(np.float64) - f, f - np.nextafter(f, np.float32(-np.inf)).astype(np.float64))
    d = np.abs(uu - np.asarray(obs, np.float32).reshape(-1, 2).astype(np.float64)[und])
    return float((2 * d * s + s * s).sum())


def pnp_inliers(u, obs, thr2):
    """The kernels' inlier test on float64 pixels u [..., n, 2]: ex = float32(obs - float32(u)), err = float32(double(ex)^2 +
    double(ey)^2), err <= thr2 (inclusive).  Returns (mask, undecidable) — undecidable where u or v could round either way."""
    u = np.asarray(u, np.float64)
    e = (np.asarray(obs, np.float32).reshape(-1, 2) - u.astype(np.float32)).astype(np.float64)
    err = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]).astype(np.float32)
    return err <= np.float32(thr2), f32_undecidable(u).any(-1)


def score_pnp(poses, K, X, obs, thr2):
    """(counts [h], mask [h, n] bool, undecidable [h, n] bool) of sfm_score_pnp."""
    mask, und = pnp_inliers(project(np.asarray(poses, np.float64).reshape(-1, 6), K, as_f64(X)), obs, thr2)
    return mask.sum(1), mask, und


def score_essential(Es, x1n, x2n, thr2):
    """(counts [h], mask [h, n] bool, undecidable [h, n] bool) of sfm_score_essential: the Sampson distance
    (x2^T E x1)^2 / ((E x1)_0^2 + (E x1)_1^2 + (E^T x2)_0^2 + (E^T x2)_1^2) in double, ONE cast of the quotient to float32,
    err <= thr2 (inclusive).  Undecidable: the quotient could round either way."""
    E = np.asarray(Es, np.float64).reshape(-1, 3, 3)
    h1 = np.c_[np.asarray(x1n, np.float64).reshape(-1, 2), np.ones(len(x1n))]
    h2 = np.c_[np.asarray(x2n, np.float64).reshape(-1, 2), np.ones(len(x2n))]
    Ex1 = np.einsum("hab,nb->hna", E, h1)
    Etx2 = np.einsum("hba,nb->hna", E, h2)
    num = np.einsum("na,hna->hn", h2, Ex1)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = num * num / (Ex1[..., 0] ** 2 + Ex1[..., 1] ** 2 + Etx2[..., 0] ** 2 + Etx2[..., 1] ** 2)
        mask = q.astype(np.float32) <= np.float32(thr2)
    return mask.sum(1), mask, f32_undecidable(q)


def _damp(M, lam):
    M = np.array(M, np.float64)
    d = np.arange(M.shape[-1])
    M[:, d, d] *= 1.0 + lam
    return M


def _w_matrix(W):
    ncam, npt = W.shape[:2]
    return W.transpose(0, 2, 1, 3).reshape(6 * ncam, 3 * npt)


def _block_diag_apply(M, x):
    return np.einsum("iab,ib->ia", M, x.reshape(M.shape[0], -1)).ravel()


def solve_direct(B, C, gc, gp, W, lam, fix_first):
    """The damped step by a dense solve of the reduced camera system S dc = g_c - W Cd^-1 g_p, S = Bd - W Cd^-1 W^T, and
    back-substitution dp = Cd^-1 (g_p - W^T dc).  fix_first: camera 0 does not move (its rows and columns leave S)."""
    ncam, npt = W.shape[:2]
    Bd, Cinv = _damp(B.reshape(ncam, 6, 6), lam), np.linalg.inv(_damp(C.reshape(npt, 3, 3), lam))
    Wm = _w_matrix(W)
    Y = np.einsum("ijab,jbc->ijac", W, Cinv).transpose(0, 2, 1, 3).reshape(6 * ncam, 3 * npt)
    S = -Y @ Wm.T
    for i in range(ncam):
        S[6 * i:6 * i + 6, 6 * i:6 * i + 6] += Bd[i]
    rhs = gc.ravel() - Y @ gp.ravel()
    k = 6 if fix_first else 0
    dc = np.zeros(6 * ncam)
    dc[k:] = np.linalg.solve(S[k:, k:], rhs[k:])
    dp = _block_diag_apply(Cinv, gp.ravel() - Wm.T @ dc)
    return dc.reshape(ncam, 6), dp.reshape(npt, 3)


def solve_pcg(B, C, gc, gp, W, lam, fix_first, tol=1e-10, iters=200):
    """The same step by the kernels' recurrence: block-Jacobi (Bd^-1) preconditioned conjugate gradients on the reduced
    system, r.r <= tol^2 rhs.rhs looked at before iterations 0, 5, 10, ...  Returns (dc, dp, iterations run)."""
    ncam, npt = W.shape[:2]
    Bd, Cinv = _damp(B.reshape(ncam, 6, 6), lam), np.linalg.inv(_damp(C.reshape(npt, 3, 3), lam))
    Minv = np.linalg.inv(Bd)
    Wm = _w_matrix(W)
    free = np.ones(6 * ncam)
    if fix_first:
        free[:6] = 0

    def S(x):
        x = x * free
        return (_block_diag_apply(Bd, x) - Wm @ _block_diag_apply(Cinv, Wm.T @ x)) * free

    rhs = (gc.ravel() - Wm @ _block_diag_apply(Cinv, gp.ravel())) * free
    x = np.zeros_like(rhs)
    r = rhs.copy()
    z = _block_diag_apply(Minv, r) * free
    p = z.copy()
    rz = r @ z
    stop2 = tol * tol * (rhs @ rhs)
    it = 0
    while it < iters:
        if it % 5 == 0 and r @ r <= stop2:
            break
        Sp = S(p)
        alpha = rz / (p @ Sp)
        x += alpha * p
        r -= alpha * Sp
        z = _block_diag_apply(Minv, r) * free
        rz_new = r @ z
        p = z + (rz_new / rz) * p
        rz = rz_new
        it += 1
    dp = _block_diag_apply(Cinv, gp.ravel() - Wm.T @ x)
    return x.reshape(ncam, 6), dp.reshape(npt, 3), it


def solve_full(B, C, gc, gp, W, lam):
    """numpy.linalg.solve on the full assembled damped normal equations (small problems only; no gauge fixing)."""
    ncam, npt = W.shape[:2]
    n = 6 * ncam + 3 * npt
    Hm = np.zeros((n, n))
    Bd, Cd = _damp(B.reshape(ncam, 6, 6), lam), _damp(C.reshape(npt, 3, 3), lam)
    for i in range(ncam):
        Hm[6 * i:6 * i + 6, 6 * i:6 * i + 6] = Bd[i]
    for j in range(npt):
        o = 6 * ncam + 3 * j
        Hm[o:o + 3, o:o + 3] = Cd[j]
    Hm[:6 * ncam, 6 * ncam:] = _w_matrix(W)
    Hm[6 * ncam:, :6 * ncam] = _w_matrix(W).T
    sol = np.linalg.solve(Hm, np.hstack([gc.ravel(), gp.ravel()]))
    return sol[:6 * ncam].reshape(ncam, 6), sol[6 * ncam:].reshape(npt, 3)
