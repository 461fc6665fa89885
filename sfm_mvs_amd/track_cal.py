"""Self-calibrating bundle adjustment of feature tracks and the undistortion of its camera model (include/sfm_hip.h, "TRACKS-CAL";
csrc/tracks_cal.hip; docs/tracks.md §15): TRACKS-BA with theta = (f, cx, cy, k1, k2), shared by all images, among the unknowns.

`sweep`, `product` and `step` take a `track_ba.Plan` and device tensors; `bundle_adjust_calibrated` follows the loop and the lambda
policy of `track_ba.bundle_adjust_tracks` with the same host waits per attempt: the step's looks at r.r and ONE read, which brings
the trial sweep's stat and count and the step of theta in one download (the trial sweep itself takes that step from the device).
`undistort_points` and `undistort_images` map keypoints and frames of the distorted camera to the ideal pinhole camera."""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import SfmHipError, check, on_device, ptr, require_cuda, stream_ptr
from .track_ba import Plan, _f64, plan  # noqa: F401  (the problem layout and its CSRs are TRACKS-BA's)

ROW = 30                        # doubles per observation in the workspace
NAMES = ("f", "cx", "cy", "k1", "k2")


def free_mask(free):
    """("f", "k1") -> 9: bit i frees theta[i]; an int 0..31 passes through."""
    if isinstance(free, (int, np.integer)):
        m = int(free)
    else:
        unknown = [n for n in free if n not in NAMES]
        if unknown:
            raise SfmHipError(f"track_cal: unknown intrinsic {unknown}; the free parameters are chosen from {NAMES}")
        m = sum(1 << NAMES.index(n) for n in set(free))
    if not 0 <= m <= 31:
        raise SfmHipError(f"track_cal: free mask {m} outside 0..31")
    return m


def theta_of(K, dist=None):
    """(theta float64 [5] = (f, cx, cy, k1, k2), aspect a = K[1, 1] / K[0, 0]) of a K and dist = (k1, k2) (None: no distortion)."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    d = (0.0, 0.0) if dist is None else tuple(float(v) for v in np.asarray(dist, np.float64).reshape(2))
    return np.array([K[0, 0], K[0, 2], K[1, 2], d[0], d[1]], np.float64), float(K[1, 1] / K[0, 0])


def K_of(theta, aspect):
    """The K of a theta: [[f, 0, cx], [0, a f, cy], [0, 0, 1]]."""
    return np.array([[theta[0], 0.0, theta[1]], [0.0, aspect * theta[0], theta[2]], [0.0, 0.0, 1.0]])


def ws_bytes(pl):
    n = _lib.lib().sfm_track_cal_ws_bytes(pl.ncam, pl.npt, pl.nobs)
    if n == 0:
        raise SfmHipError(f"track_cal: sizes ncam {pl.ncam}, npt {pl.npt}, nobs {pl.nobs} are outside the limits of sfm_track_cal_ws_bytes")
    return n


def workspace(pl):
    """A workspace of its own: it holds the rows of ONE linearisation (a trial sweep needs a second one)."""
    return torch.empty(ws_bytes(pl), dtype=torch.uint8, device=pl.device)


def rows_of(pl, ws):
    """The rows a sweep left in `ws`: float64 [nobs, 30] (a view): Jc (12), Ji (10), Jp (6), r (2)."""
    base = (-ws.data_ptr()) % 256
    return ws[base:base + pl.nobs * ROW * 8].view(torch.float64).view(pl.nobs, ROW)


def _theta_arg(theta):
    t = np.ascontiguousarray(np.asarray(theta, np.float64).reshape(5))
    return t, t.ctypes.data_as(ctypes.c_void_p)


def sweep(pl, cams, theta, aspect, X, obs, huber=None, mode=0, active=None, ws=None, out=None, dtheta=None):
    """sfm_track_cal_sweep at (cams [ncam, 6] f64, theta [5] on the host minus dtheta [5] f64 on the device (None: zero), X [npt, 3]
    f64) -> dict(JtJ_cam, Jtr_cam, JtJ_pt, Jtr_pt, E [ncam, 30], G [25], Jtr_theta [5], F [npt, 15], stat [2] f64, count [3] i32,
    active [nobs] u8, ws).  mode 0 writes `active`, mode 1 reads it.  huber None or inf: plain least squares.  No host wait."""
    dev = pl.device
    cams = _f64(cams, (pl.ncam, 6), "cams")
    X = _f64(X, (pl.npt, 3), "X")
    require_cuda(obs)
    if obs.dtype != torch.float32 or tuple(obs.shape) != (pl.nobs, 2) or not obs.is_contiguous():
        raise SfmHipError("track_cal.sweep: obs must be a contiguous float32 [nobs, 2] device tensor")
    if mode == 1 and active is None:
        raise SfmHipError("track_cal.sweep: mode 1 reads the active set of a mode-0 sweep")
    if active is None:
        active = torch.empty(pl.nobs, dtype=torch.uint8, device=dev)
    elif active.dtype != torch.uint8 or active.numel() != pl.nobs or not active.is_contiguous():
        raise SfmHipError("track_cal.sweep: active must be a contiguous uint8 [nobs] device tensor")
    if dtheta is not None:
        dtheta = _f64(dtheta, (5,), "dtheta")
    ws = workspace(pl) if ws is None else ws
    if out is None:
        f64 = dict(dtype=torch.float64, device=dev)
        out = dict(JtJ_cam=torch.empty((pl.ncam, 36), **f64), Jtr_cam=torch.empty((pl.ncam, 6), **f64), JtJ_pt=torch.empty((pl.npt, 9), **f64),
                   Jtr_pt=torch.empty((pl.npt, 3), **f64), E=torch.empty((pl.ncam, 30), **f64), G=torch.empty(25, **f64),
                   Jtr_theta=torch.empty(5, **f64), F=torch.empty((pl.npt, 15), **f64), stat=torch.empty(2, **f64),
                   count=torch.empty(3, dtype=torch.int32, device=dev))
    t, tp = _theta_arg(theta)
    h = float("inf") if huber is None else float(huber)
    with on_device(dev):
        check(_lib.lib().sfm_track_cal_sweep(ptr(cams), pl.ncam, tp, float(aspect), ptr(dtheta), ptr(X), pl.npt, ptr(obs) if pl.nobs else None,
                                             *pl._args(), h, int(mode), ptr(active) if pl.nobs else None, ptr(out["JtJ_cam"]), ptr(out["Jtr_cam"]),
                                             ptr(out["JtJ_pt"]), ptr(out["Jtr_pt"]), ptr(out["E"]), ptr(out["G"]), ptr(out["Jtr_theta"]), ptr(out["F"]),
                                             ptr(out["stat"]), ptr(out["count"]), ptr(ws), ws.numel(), stream_ptr()), "sfm_track_cal_sweep")
    out["active"], out["ws"] = active, ws
    return out


def product(pl, ws, vec, mode, vec_theta=None):
    """sfm_track_cal_product over the rows in `ws`: mode 0 (vec [ncam, 6], vec_theta [5]) -> [npt, 3]; mode 1 vec [npt, 3] ->
    ([ncam, 6], [5])."""
    vec = _f64(vec, (pl.ncam, 6) if mode == 0 else (pl.npt, 3), "vec")
    f64 = dict(dtype=torch.float64, device=pl.device)
    if mode == 0:
        vec_theta = _f64(vec_theta, (5,), "vec_theta")
        out, out_theta = torch.empty((pl.npt, 3), **f64), None
    else:
        out, out_theta = torch.empty((pl.ncam, 6), **f64), torch.empty(5, **f64)
    with on_device(pl.device):
        check(_lib.lib().sfm_track_cal_product(pl.ncam, pl.npt, *pl._args(), int(mode), ptr(vec), ptr(vec_theta) if mode == 0 else None, ptr(out),
                                               ptr(out_theta), ptr(ws), ws.numel(), stream_ptr()), "sfm_track_cal_product")
    return out if mode == 0 else (out, out_theta)


def step(pl, blocks, lam, free=("f", "k1"), fix_first_camera=True, cg_tol=1e-10, cg_iters=200):
    """sfm_track_cal_step on the blocks and rows of `blocks` (a dict `sweep` returned) -> (dc [ncam, 6], dtheta [5], dp [npt, 3], CG
    iterations, status bits).  The update is parameters - step; dtheta is exactly 0 where the parameter is not free."""
    f64 = dict(dtype=torch.float64, device=pl.device)
    dc, di, dp = torch.empty((pl.ncam, 6), **f64), torch.empty(5, **f64), torch.empty((pl.npt, 3), **f64)
    it, st = ctypes.c_int32(0), ctypes.c_int32(0)
    ws = blocks["ws"]
    with on_device(pl.device):
        check(_lib.lib().sfm_track_cal_step(pl.ncam, pl.npt, *pl._args(), ptr(_f64(blocks["JtJ_cam"], (pl.ncam, 36), "JtJ_cam")),
                                            ptr(_f64(blocks["Jtr_cam"], (pl.ncam, 6), "Jtr_cam")), ptr(_f64(blocks["JtJ_pt"], (pl.npt, 9), "JtJ_pt")),
                                            ptr(_f64(blocks["Jtr_pt"], (pl.npt, 3), "Jtr_pt")), ptr(_f64(blocks["E"], (pl.ncam, 30), "E")),
                                            ptr(_f64(blocks["G"], (25,), "G")), ptr(_f64(blocks["Jtr_theta"], (5,), "Jtr_theta")), float(lam),
                                            free_mask(free), int(bool(fix_first_camera)), float(cg_tol), int(cg_iters), ptr(dc), ptr(di), ptr(dp),
                                            ctypes.byref(it), ctypes.byref(st), ptr(ws), ws.numel(), stream_ptr()), "sfm_track_cal_step")
    return dc, di, dp, it.value, st.value


def _read(blocks, dtheta=None):
    """The ONE host wait of a sweep: (robust cost, plain cost, active, crossed, outliers, step of theta [5])."""
    parts = [blocks["stat"], blocks["count"].to(torch.float64)] + ([] if dtheta is None else [dtheta])
    h = torch.cat(parts).cpu().numpy()
    return float(h[0]), float(h[1]), int(h[2]), int(h[3]), int(h[4]), (h[5:10].copy() if dtheta is not None else np.zeros(5))


def bundle_adjust_calibrated(cams, K, dist, X, obs, cam_idx, pt_idx, free=("f", "k1"), huber=None, iters=10, lam=1e-3, fix_first_camera=True,
                             cg_tol=1e-10, cg_iters=200, log=None):
    """`track_ba.bundle_adjust_tracks` with the intrinsics theta = (f, cx, cy, k1, k2) of the model u = f d x + cx, v = a f d y + cy,
    d = 1 + k1 r2 + k2 r2^2 among the unknowns.  K [3, 3] on the host (f = K[0, 0], the principal point, the fixed aspect a =
    K[1, 1] / K[0, 0]), dist = (k1, k2) or None, `free` the names (or the mask) of the parameters that move; the other arguments,
    the loop and the lambda policy are those of `bundle_adjust_tracks`.  A trial is accepted iff no active observation crossed its
    camera plane, f' > 0 and the cost is strictly lower.  Returns (cams, X float64, K', dist' = (k1, k2), history, info)."""
    require_cuda(cams, X, obs, cam_idx, pt_idx)
    cams = cams.detach().to(torch.float64).reshape(-1, 6).contiguous().clone()
    X = X.detach().to(torch.float64).reshape(-1, 3).contiguous().clone()
    obs = obs.to(torch.float32).reshape(-1, 2).contiguous()
    theta, aspect = theta_of(K, dist)
    mask = free_mask(free)
    pl = plan(cam_idx, pt_idx, cams.shape[0], X.shape[0])
    say = log or (lambda *a: None)
    spare = workspace(pl)
    blocks = sweep(pl, cams, theta, aspect, X, obs, huber, 0)
    active = blocks["active"]
    cost, plain, n_active, _, n_out, _ = _read(blocks)
    hist, cg, refused = [cost], [], 0
    for it in range(iters):
        accepted, gain = False, 0.0
        for _ in range(8):
            dc, di, dp, ncg, status = step(pl, blocks, lam, mask, fix_first_camera, cg_tol, cg_iters)
            cg.append(ncg)
            c_new, x_new = cams - dc, X - dp
            trial = sweep(pl, c_new, theta, aspect, x_new, obs, huber, 1, active, spare, dtheta=di)
            cost_new, plain_new, _, crossed, out_new, di_host = _read(trial, di)
            t_new = theta - di_host                                             # the bits the trial sweep formed on the device
            bad = crossed > 0 or not t_new[0] > 0.0
            if bad:
                refused += 1
            if not bad and cost_new < cost:
                spare = blocks["ws"]
                cams, X, theta, blocks, accepted = c_new, x_new, t_new, trial, True
                gain = (cost - cost_new) / cost
                cost, plain, n_out, lam = cost_new, plain_new, out_new, max(lam / 3.0, 1e-12)
                say(f"track-cal iter {it}: cost {cost:.6g} lambda {lam:.2g} cg {ncg} outliers {n_out} f {theta[0]:.3f} k1 {theta[3]:.4g} k2 {theta[4]:.4g}")
                break
            lam *= 4.0
        hist.append(cost)
        if not accepted or gain < 1e-9:
            break
    info = dict(active=n_active, crossed_refusals=refused, outliers=n_out, plain_cost=plain, cg_iters=cg, lam=lam, theta=theta.copy(), aspect=aspect,
                free=mask)
    return cams, X, K_of(theta, aspect), theta[3:].copy(), hist, info


def undistort_points(px, K, dist, K_out=None):
    """sfm_undistort_points: px float32 [n, 2] pixels of the distorted camera (K, dist = (k1, k2)) on the device -> float32 [n, 2]
    pixels of the ideal pinhole camera K_out (default: K).  A non-finite keypoint gives NaN.  No host wait."""
    require_cuda(px)
    if px.dtype != torch.float32 or px.dim() != 2 or px.shape[1] != 2 or not px.is_contiguous():
        raise SfmHipError("track_cal.undistort_points: px must be a contiguous float32 [n, 2] device tensor")
    theta, aspect = theta_of(K, dist)
    t, tp = _theta_arg(theta)
    ko = np.ascontiguousarray(np.asarray(K if K_out is None else K_out, np.float64).reshape(9))
    out = torch.empty_like(px)
    n = px.shape[0]
    with on_device(px.device):
        check(_lib.lib().sfm_undistort_points(ptr(px) if n else None, n, tp, aspect, ko.ctypes.data_as(ctypes.c_void_p), ptr(out) if n else None,
                                              stream_ptr()), "sfm_undistort_points")
    return out


def undistort_images(frames, K, dist, K_out=None, want_mask=False):
    """sfm_undistort_image, one batched call: frames uint8 [n, H, W, C], [H, W, C] or [n, H, W] (C = 1) on the device -> the frames
    of the ideal pinhole camera K_out (default: K), same shape; with want_mask also uint8 [n, H, W] (or [H, W]) of 0 / 1.  A pixel
    whose source lies outside the frame is 0 and invalid.  No host wait."""
    require_cuda(frames)
    if frames.dtype != torch.uint8 or frames.dim() not in (3, 4) or not frames.is_contiguous():
        raise SfmHipError("track_cal.undistort_images: frames must be a contiguous uint8 device tensor [n, H, W, C], [H, W, C] or [n, H, W]")
    shape = tuple(frames.shape)
    if frames.dim() == 4:
        n, H, W, C = shape
    elif shape[2] in (1, 3):
        (H, W, C), n = shape, 1
    else:
        (n, H, W), C = shape, 1
    theta, aspect = theta_of(K, dist)
    t, tp = _theta_arg(theta)
    ko = np.ascontiguousarray(np.asarray(K if K_out is None else K_out, np.float64).reshape(9))
    out = torch.empty_like(frames)
    mask = torch.empty((n, H, W), dtype=torch.uint8, device=frames.device) if want_mask else None
    with on_device(frames.device):
        check(_lib.lib().sfm_undistort_image(ptr(frames) if n else None, n, H, W, C, tp, aspect, ko.ctypes.data_as(ctypes.c_void_p),
                                             ptr(out) if n else None, ptr(mask), stream_ptr()), "sfm_undistort_image")
    if not want_mask:
        return out
    return out, (mask[0] if frames.dim() == 3 and shape[2] in (1, 3) else mask)
