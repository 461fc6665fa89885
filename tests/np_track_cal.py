"""NumPy restatement of the TRACKS-CAL section of include/sfm_hip.h, written from the header: the camera model, the rows of 30, the
blocks and the border over the two CSRs, the products, the bordered damped step (direct, and by conjugate gradients in the kernel's
recurrence), the Levenberg-Marquardt loop of sfm_mvs_amd.track_cal.bundle_adjust_calibrated, and the two undistortions (to the bit).
Float64 throughout, the Jacobians by complex-step differentiation of `project`.  Imports NumPy, np_ba and np_track_ba, nothing
else; shares no code with the kernels."""
import numpy as np

import np_ba
import np_track_ba as nb

H = np_ba.H
ROW = 30
NAMES = ("f", "cx", "cy", "k1", "k2")
NEWTON = 10


def free_mask(free):
    """("f", "k1") -> 9; an int passes through."""
    if isinstance(free, (int, np.integer)):
        return int(free)
    return sum(1 << NAMES.index(n) for n in set(free))


def theta_of(K, dist=(0.0, 0.0)):
    """(theta [5], aspect) of a K and (k1, k2)."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    d = (0.0, 0.0) if dist is None else dist
    return np.array([K[0, 0], K[0, 2], K[1, 2], float(d[0]), float(d[1])]), float(K[1, 1] / K[0, 0])


def K_of(theta, a):
    return np.array([[theta[0], 0.0, theta[1]], [0.0, a * theta[0], theta[2]], [0.0, 0.0, 1.0]])


def project(cams, theta, a, X):
    """cams [n, 6], X [n, 3] paired (real or complex), theta [5] (real or complex) -> pixels [n, 2], the header's model in the
    header's order of operations."""
    cams, X = np.asarray(cams), np.asarray(X)
    R = np_ba.rotation(cams[:, :3])
    Xc = (np.einsum("iab,ijb->ija", R, X[:, None, :]) + cams[:, None, 3:])[:, 0]
    z = Xc[:, 2]
    flat = np.real(z) == 0                                                      # never active; np_ba.project's convention keeps it finite
    iz = np.where(flat, 1 - z, 1 / np.where(flat, 1, z))
    x, y = Xc[:, 0] * iz, Xc[:, 1] * iz
    f, cx, cy, k1, k2 = theta
    r2 = x * x + y * y
    d = 1 + k1 * r2 + k2 * r2 * r2
    return np.stack([f * d * x + cx, a * f * d * y + cy], -1)


def jacobians(cams, theta, a, X):
    """(Jc [n, 2, 6], Ji [n, 2, 5], Jp [n, 2, 3]) by the complex step."""
    n = len(cams)
    Jc, Ji, Jp = np.empty((n, 2, 6)), np.empty((n, 2, 5)), np.empty((n, 2, 3))
    for k in range(6):
        c = cams.astype(np.complex128)
        c[:, k] += 1j * H
        Jc[..., k] = project(c, theta, a, X).imag / H
    for k in range(5):
        t = np.asarray(theta, np.complex128).copy()
        t[k] += 1j * H
        Ji[..., k] = project(cams, t, a, X).imag / H
    for k in range(3):
        x = X.astype(np.complex128)
        x[:, k] += 1j * H
        Jp[..., k] = project(cams, theta, a, x).imag / H
    return Jc, Ji, Jp


def observations(cams, theta, a, X, obs, cam_idx, pt_idx, huber=np.inf, active=None):
    """Per observation at (cams, theta, X): dict(rows [nobs, 30], active, take, crossed, e, w, rho), as np_track_ba.observations."""
    cams = np.asarray(cams, np.float64).reshape(-1, 6)
    X = np.asarray(X, np.float64).reshape(-1, 3)
    theta = np.asarray(theta, np.float64).reshape(5)
    obs = np.asarray(obs, np.float32).reshape(-1, 2).astype(np.float64)
    ci, pi = np.asarray(cam_idx, np.int64), np.asarray(pt_idx, np.int64)
    nobs = len(obs)
    inr = nb._in_range(ci, len(cams)) & nb._in_range(pi, len(X))
    c, x = cams[np.where(inr, ci, 0)], X[np.where(inr, pi, 0)]
    rows = np.zeros((nobs, ROW))
    th_ok = bool(np.isfinite(theta).all() and theta[0] > 0)
    with np.errstate(all="ignore"):
        R = np_ba.rotation(c[:, :3])
        z = np.einsum("ob,ob->o", R[:, 2], x) + c[:, 5]
        r = project(c, theta, a, x) - obs
        ok = inr & np.isfinite(z) & (z > 0) & np.isfinite(r).all(1) & th_ok
        if active is None:
            act, crossed = ok, np.zeros(nobs, bool)
        else:
            was = inr & (np.asarray(active) != 0)
            act, crossed = was & ok, was & ~ok
        e = np.where(act, np.sqrt((r * r).sum(1)), 0.0)
        inside = e <= huber
        w = np.where(inside, 1.0, huber / np.where(e > 0, e, 1.0))
        rho = np.where(inside, e * e, 2.0 * huber * e - huber * huber) if np.isfinite(huber) else e * e
        sw = np.sqrt(w)
        Jc, Ji, Jp = jacobians(c, theta, a, x)
    t = np.flatnonzero(act)
    rows[t, :12] = (sw[t, None, None] * Jc[t]).reshape(-1, 12)
    rows[t, 12:22] = (sw[t, None, None] * Ji[t]).reshape(-1, 10)
    rows[t, 22:28] = (sw[t, None, None] * Jp[t]).reshape(-1, 6)
    rows[t, 28:] = sw[t, None] * r[t]
    return dict(rows=rows, active=(ok if active is None else np.asarray(active) != 0).astype(np.uint8), take=act, crossed=crossed,
                e=e, w=np.where(act, w, 0.0), rho=np.where(act, rho, 0.0))


def split(rows):
    """(Jc [n, 2, 6], Ji [n, 2, 5], Jp [n, 2, 3], r [n, 2]) of rows [n, 30]."""
    rows = np.asarray(rows, np.float64).reshape(-1, ROW)
    return rows[:, :12].reshape(-1, 2, 6), rows[:, 12:22].reshape(-1, 2, 5), rows[:, 22:28].reshape(-1, 2, 3), rows[:, 28:]


def sweep(cams, theta, a, X, obs, cam_idx, pt_idx, track_off, cam_off, cam_obs, huber=np.inf, active=None):
    """-> dict(B, C, gc, gp, E [ncam, 6, 5], G [5, 5], gi [5], F [npt, 3, 5], stat, count, active, rows, ...) as sfm_track_cal_sweep
    leaves them."""
    ncam, npt = len(np.asarray(cams).reshape(-1, 6)), len(np.asarray(X).reshape(-1, 3))
    out = observations(cams, theta, a, X, obs, cam_idx, pt_idx, huber, active)
    nobs = len(out["rows"])
    Jc, Ji, Jp, r = split(out["rows"])
    B, C, gc, gp = np.zeros((ncam, 6, 6)), np.zeros((npt, 3, 3)), np.zeros((ncam, 6)), np.zeros((npt, 3))
    E, F = np.zeros((ncam, 6, 5)), np.zeros((npt, 3, 5))
    t, o = nb._point_members(track_off, nobs)
    np.add.at(C, t, np.einsum("oka,okb->oab", Jp[o], Jp[o]))
    np.add.at(gp, t, np.einsum("oka,ok->oa", Jp[o], r[o]))
    np.add.at(F, t, np.einsum("oka,okb->oab", Jp[o], Ji[o]))
    c, o = nb._camera_members(cam_off, cam_obs, cam_idx, nobs)
    np.add.at(B, c, np.einsum("oka,okb->oab", Jc[o], Jc[o]))
    np.add.at(gc, c, np.einsum("oka,ok->oa", Jc[o], r[o]))
    np.add.at(E, c, np.einsum("oka,okb->oab", Jc[o], Ji[o]))
    take = out["take"]
    out.update(B=B, C=C, gc=gc, gp=gp, E=E, F=F, G=np.einsum("oka,okb->ab", Ji, Ji), gi=np.einsum("oka,ok->a", Ji, r),
               stat=np.array([out["rho"].sum(), (out["e"][take] ** 2).sum()]),
               count=np.array([take.sum(), out["crossed"].sum(), (take & (out["e"] > huber)).sum()], np.int32))
    return out


def product(rows, cam_idx, pt_idx, track_off, cam_off, cam_obs, ncam, npt, vec, vec_theta, mode):
    """mode 0: (vec [ncam, 6], vec_theta [5]) -> out [npt, 3]; mode 1: vec [npt, 3] -> (out [ncam, 6], out_theta [5])."""
    nobs = len(rows)
    ci, pi = np.asarray(cam_idx, np.int64), np.asarray(pt_idx, np.int64)
    Jc, Ji, Jp, _ = split(rows)
    vec = np.asarray(vec, np.float64)
    if mode == 0:
        out = np.zeros((npt, 3))
        t, o = nb._point_members(track_off, nobs)
        ok = nb._in_range(ci[o], ncam)
        t, o = t[ok], o[ok]
        inner = np.einsum("oka,oa->ok", Jc[o], vec[ci[o]]) + np.einsum("oka,a->ok", Ji[o], np.asarray(vec_theta, np.float64))
        np.add.at(out, t, np.einsum("okb,ok->ob", Jp[o], inner))
        return out
    out = np.zeros((ncam, 6))
    c, o = nb._camera_members(cam_off, cam_obs, cam_idx, nobs)
    ok = nb._in_range(pi[o], npt)
    c, o = c[ok], o[ok]
    np.add.at(out, c, np.einsum("oka,ok->oa", Jc[o], np.einsum("okb,ob->ok", Jp[o], vec[pi[o]])))
    both = np.flatnonzero(nb._in_range(ci, ncam) & nb._in_range(pi, npt))
    out_theta = np.einsum("oka,ok->a", Ji[both], np.einsum("okb,ob->ok", Jp[both], vec[pi[both]]))
    return out, out_theta


def dense_w(rows, cam_idx, pt_idx, ncam, npt):
    """W [ncam, npt, 6, 3] = sum over the observations of a pair of Jc^T Jp (consistent CSRs; small problems only)."""
    ci, pi = np.asarray(cam_idx, np.int64), np.asarray(pt_idx, np.int64)
    ok = nb._in_range(ci, ncam) & nb._in_range(pi, npt)
    Jc, _, Jp, _ = split(np.asarray(rows)[ok])
    W = np.zeros((ncam, npt, 6, 3))
    np.add.at(W, (ci[ok], pi[ok]), np.einsum("oka,okb->oab", Jc, Jp))
    return W


def _no_pivot5(a):
    """np_track_ba._no_pivot for a 5 x 5 block."""
    a = np.array(a, np.float64)
    bad = False
    with np.errstate(all="ignore"):
        for col in range(5):
            for r in range(col + 1, 5):
                if abs(a[r, col]) > abs(a[col, col]):
                    a[[col, r]] = a[[r, col]]
            piv = a[col, col]
            if not abs(piv) > 0.0 or not abs(piv) < 1e300:
                bad = True
            a[col] = a[col] / piv
            for r in range(5):
                if r != col:
                    a[r] = a[r] - a[r, col] * a[col]
    return bad


def restricted(G, lam, free):
    """Gd with the rows and columns of the parameters that are not free replaced by the identity."""
    m = free_mask(free)
    Gd = np.array(G, np.float64).reshape(5, 5)
    Gd[np.arange(5), np.arange(5)] *= 1.0 + lam
    on = np.array([(m >> k) & 1 for k in range(5)], bool)
    R = np.eye(5)
    R[np.ix_(on, on)] = Gd[np.ix_(on, on)]
    return Gd, R, on


def system(B, C, gc, gp, E, G, gi, F, W, lam, free, fix_first):
    """The bordered reduced system of the header -> dict(S [n, n], rhs [n], held [n] bool, Cinv, P [n, 3 npt], status), n = 6 ncam +
    5.  Singular point blocks have the zero inverse; held entries (camera 0 when fixed, parameters that are not free) keep their
    rows and columns here: the solvers leave them out."""
    B, C, gc, gp, E, F, W = (np.array(x, np.float64) for x in (B, C, gc, gp, E, F, W))
    ncam, npt = len(B), len(C)
    B, C, E, F = B.reshape(ncam, 6, 6), C.reshape(npt, 3, 3), E.reshape(ncam, 6, 5), F.reshape(npt, 3, 5)
    bad_c, bad_p = nb.singular_blocks(B, C, lam)
    Gd, Gr, on = restricted(G, lam, free)
    status = int(bad_c.any()) | 2 * int(bad_p.any()) | 4 * int(_no_pivot5(Gr))
    Bd, Cd = np_ba._damp(B, lam), np_ba._damp(C, lam)
    Cd[bad_p] = np.eye(3)
    Cinv = np.linalg.inv(Cd)
    Cinv[bad_p] = 0.0
    nc = 6 * ncam
    n = nc + 5
    P = np.zeros((n, 3 * npt))
    P[:nc] = np_ba._w_matrix(W)
    P[nc:] = F.transpose(2, 0, 1).reshape(5, 3 * npt)
    A = np.zeros((n, n))
    for i in range(ncam):
        A[6 * i:6 * i + 6, 6 * i:6 * i + 6] = Bd[i]
    A[:nc, nc:] = E.reshape(nc, 5)
    A[nc:, :nc] = E.reshape(nc, 5).T
    A[nc:, nc:] = Gd
    Y = (P.reshape(n, npt, 3)[:, :, :, None] * Cinv[None]).sum(2).reshape(n, 3 * npt)        # P Cd^-1 (Cinv symmetric)
    S = A - Y @ P.T
    rhs = np.r_[gc.ravel(), np.asarray(gi, np.float64)] - Y @ gp.ravel()
    held = np.zeros(n, bool)
    if fix_first:
        held[:6] = True
    held[nc:] = ~on
    return dict(S=S, rhs=rhs, held=held, Cinv=Cinv, P=P, status=status, Bd=Bd, Gr=Gr, bad_c=bad_c, gp=gp, ncam=ncam, npt=npt)


def _back(s, y):
    dp = np.einsum("jab,jb->ja", s["Cinv"], (s["gp"].ravel() - s["P"].T @ y).reshape(-1, 3))
    nc = 6 * s["ncam"]
    return y[:nc].reshape(-1, 6), y[nc:].copy(), dp


def step(B, C, gc, gp, E, G, gi, F, W, lam, free, fix_first=True):
    """The damped step of sfm_track_cal_step by a dense solve -> (dc, di, dp, status).  A camera with the zero block takes no step
    (its right-hand side is zero and conjugate gradients never move it), as in np_track_ba.step."""
    s = system(B, C, gc, gp, E, G, gi, F, W, lam, free, fix_first)
    n = len(s["rhs"])
    y = np.zeros(n)
    if s["rhs"][~s["held"]].any():
        zero = np.repeat(s["bad_c"] & ~np.asarray(B).reshape(s["ncam"], -1).any(1), 6)
        keep = ~s["held"]
        keep[:6 * s["ncam"]] &= ~zero
        k = np.flatnonzero(keep)
        y[k] = np.linalg.solve(s["S"][np.ix_(k, k)], s["rhs"][k])
    return _back(s, y) + (s["status"],)


def solve_pcg(B, C, gc, gp, E, G, gi, F, W, lam, free, fix_first=True, tol=1e-10, iters=200, reduced_border=False):
    """The same step by the kernels' recurrence: conjugate gradients preconditioned with blockdiag(Bd^-1, Gd^-1) (Gd restricted to
    the free set), r.r <= tol^2 rhs.rhs looked at before iterations 0, 5, 10, ... -> (dc, di, dp, iterations).
    reduced_border: the reduced block Gd - F^T Cd^-1 F in the place of Gd in the preconditioner (the alternative §15.3 measures)."""
    s = system(B, C, gc, gp, E, G, gi, F, W, lam, free, fix_first)
    nc = 6 * s["ncam"]
    live = (~s["held"]).astype(np.float64)
    Minv = np.linalg.inv(np.where(s["bad_c"][:, None, None], np.eye(6), s["Bd"]))
    Gr = s["Gr"]
    if reduced_border:
        on = ~s["held"][nc:]
        Gr = np.eye(5)
        Gr[np.ix_(on, on)] = s["S"][nc:, nc:][np.ix_(on, on)]
    Ginv = np.linalg.inv(Gr)

    def pre(r):
        return np.r_[np_ba._block_diag_apply(Minv, r[:nc]), Ginv @ r[nc:]] * live

    rhs = s["rhs"] * live
    x = np.zeros_like(rhs)
    r = rhs.copy()
    z = pre(r)
    p = z.copy()
    rz = r @ z
    stop2 = tol * tol * (rhs @ rhs)
    it = 0
    with np.errstate(all="ignore"):
        while it < iters:
            if it % 5 == 0 and r @ r <= stop2:
                break
            Sp = (s["S"] @ p) * live
            pSp = p @ Sp
            alpha = rz / pSp if pSp > 0.0 else 0.0                                 # the header's guards: no 0 / 0 after an exact solve
            x += alpha * p
            r -= alpha * Sp
            z = pre(r)
            rz_new = r @ z
            p = z + (rz_new / rz if rz > 0.0 else 0.0) * p
            rz = rz_new
            it += 1
    return _back(s, x) + (it,)


def bundle_adjust(cams, K, dist, X, obs, cam_idx, pt_idx, free=("f", "k1"), huber=None, iters=10, lam=1e-3, fix_first_camera=True):
    """The loop of track_cal.bundle_adjust_calibrated with the direct solve -> (cams, X, K', dist', history, info)."""
    cams = np.array(cams, np.float64).reshape(-1, 6)
    X = np.array(X, np.float64).reshape(-1, 3)
    ncam, npt = len(cams), len(X)
    theta, a = theta_of(K, dist)
    m = free_mask(free)
    h = np.inf if huber is None else float(huber)
    track_off, cam_off, cam_obs = nb.plan(cam_idx, pt_idx, ncam, npt)
    at = lambda c, t, x, active: sweep(c, t, a, x, obs, cam_idx, pt_idx, track_off, cam_off, cam_obs, h, active)  # noqa: E731
    cur = at(cams, theta, X, None)
    active = cur["active"]
    cost = float(cur["stat"][0])
    hist, refused, lams = [cost], 0, []
    for _ in range(iters):
        accepted, gain = False, 0.0
        for _ in range(8):
            lams.append(lam)
            dc, di, dp, _ = step(cur["B"], cur["C"], cur["gc"], cur["gp"], cur["E"], cur["G"], cur["gi"], cur["F"],
                                 dense_w(cur["rows"], cam_idx, pt_idx, ncam, npt), lam, m, fix_first_camera)
            t_new = theta - di
            trial = at(cams - dc, t_new, X - dp, active)
            crossed, cost_new = int(trial["count"][1]), float(trial["stat"][0])
            bad = crossed > 0 or not t_new[0] > 0
            refused += bad
            if not bad and cost_new < cost:
                cams, X, theta, cur, accepted = cams - dc, X - dp, t_new, trial, True
                gain = (cost - cost_new) / cost
                cost, lam = cost_new, max(lam / 3.0, 1e-12)
                break
            lam *= 4.0
        hist.append(cost)
        if not accepted or gain < 1e-9:
            break
    info = dict(active=int(cur["count"][0]), crossed_refusals=int(refused), outliers=int(cur["count"][2]), plain_cost=float(cur["stat"][1]),
                lams=lams, lam=lam, last=cur, theta=theta, aspect=a)
    return cams, X, K_of(theta, a), theta[3:].copy(), hist, info


def rms_error(cams, theta, a, X, obs, cam_idx, pt_idx, rows):
    """Root mean square reprojection error (px) of the observation rows `rows` at (cams, theta, X)."""
    e = observations(cams, theta, a, X, obs, cam_idx, pt_idx)["e"][rows]
    return float(np.sqrt((e * e).mean()))


# ---- the undistortions, to the bit ------------------------------------------------------------------------------------------

def undistort_points(px, theta, a, K_out):
    """sfm_undistort_points: float32 [n, 2] -> float32 [n, 2], every operation a float64 NumPy operation in the header's order."""
    px = np.asarray(px, np.float32).reshape(-1, 2)
    f, cx, cy, k1, k2 = (np.float64(t) for t in theta)
    a = np.float64(a)
    Ko = np.asarray(K_out, np.float64).reshape(3, 3)
    with np.errstate(all="ignore"):
        u, v = px[:, 0].astype(np.float64), px[:, 1].astype(np.float64)
        xd, yd = (u - cx) / f, (v - cy) / (a * f)
        rd = np.sqrt(xd * xd + yd * yd)
        r = rd.copy()
        for _ in range(NEWTON):
            r2 = r * r
            g = r * (1.0 + r2 * (k1 + k2 * r2)) - rd
            h = 1.0 + r2 * (3.0 * k1 + 5.0 * k2 * r2)
            r = r - g / h
        s = np.where(rd > 0.0, r / np.where(rd > 0.0, rd, 1.0), 1.0)
        ou, ov = Ko[0, 0] * (xd * s) + Ko[0, 2], Ko[1, 1] * (yd * s) + Ko[1, 2]
        ok = np.isfinite(u) & np.isfinite(v) & np.isfinite(ou) & np.isfinite(ov)
        out = np.stack([ou, ov], 1).astype(np.float32)
    out[~ok] = np.nan
    return out


def distort_points(px, theta, a, K_in):
    """The forward model on pixels of the ideal image with K_in -> float64 pixels of the distorted image (not a kernel: the
    inverse test's other half)."""
    px = np.asarray(px, np.float64).reshape(-1, 2)
    Ki = np.asarray(K_in, np.float64).reshape(3, 3)
    f, cx, cy, k1, k2 = theta
    x, y = (px[:, 0] - Ki[0, 2]) / Ki[0, 0], (px[:, 1] - Ki[1, 2]) / Ki[1, 1]
    r2 = x * x + y * y
    d = 1 + k1 * r2 + k2 * r2 * r2
    return np.stack([f * d * x + cx, a * f * d * y + cy], 1)


def undistort_image(src, theta, a, K_out):
    """sfm_undistort_image on uint8 [n, H, W, C] (or [H, W, C]) -> (dst of the same shape, mask uint8 [n, H, W] or [H, W])."""
    src = np.asarray(src, np.uint8)
    single = src.ndim == 3
    s4 = src[None] if single else src
    n, Hh, Ww, C = s4.shape
    f, cx, cy, k1, k2 = (np.float64(t) for t in theta)
    a = np.float64(a)
    Ko = np.asarray(K_out, np.float64).reshape(3, 3)
    xo, yo = np.meshgrid(np.arange(Ww, dtype=np.float64), np.arange(Hh, dtype=np.float64))
    x, y = (xo - Ko[0, 2]) / Ko[0, 0], (yo - Ko[1, 2]) / Ko[1, 1]
    r2 = x * x + y * y
    d = 1.0 + k1 * r2 + k2 * r2 * r2
    with np.errstate(all="ignore"):
        su, sv = (f * d * x + cx).astype(np.float32), (a * f * d * y + cy).astype(np.float32)
        ok = (su >= 0) & (su <= np.float32(Ww - 1)) & (sv >= 0) & (sv <= np.float32(Hh - 1))
    su, sv = np.where(ok, su, np.float32(0)), np.where(ok, sv, np.float32(0))
    fx0, fy0 = np.floor(su), np.floor(sv)
    ax, ay = (su - fx0).astype(np.float32)[None, :, :, None], (sv - fy0).astype(np.float32)[None, :, :, None]
    x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, Ww - 1), np.minimum(y0 + 1, Hh - 1)
    p = s4.astype(np.float32)
    p00, p10, p01, p11 = p[:, y0, x0], p[:, y0, x1], p[:, y1, x0], p[:, y1, x1]
    top = p00 + ax * (p10 - p00)
    bot = p01 + ax * (p11 - p01)
    val = np.floor(top + ay * (bot - top) + np.float32(0.5))
    assert val.dtype == np.float32
    dst = np.clip(val, 0, 255).astype(np.uint8) * ok[None, :, :, None].astype(np.uint8)
    mask = np.broadcast_to(ok.astype(np.uint8), (n, Hh, Ww)).copy()
    return (dst[0], mask[0]) if single else (dst, mask)
