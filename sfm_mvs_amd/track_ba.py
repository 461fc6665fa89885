"""Bundle adjustment of feature tracks (include/sfm_hip.h, "TRACKS-BA"; csrc/tracks_ba.hip; docs/tracks.md §9): a sparse Schur
Levenberg-Marquardt whose sums run in a fixed order (no floating-point atomics: a run is reproducible to the bit), with float64
points, a Huber loss and the PCG recurrence on the device.

`plan` builds the two CSRs once per adjustment; `sweep`, `product` and `step` take and return device tensors; `bundle_adjust_tracks`
follows the loop and the lambda policy of `ba.bundle_adjust_schur`.  Host waits per attempt: the step's looks at r.r (the header
states how many) and ONE read of the trial sweep's stat and count."""
import ctypes

import numpy as np
import torch

from . import _lib, hostgeom
from ._lib import SfmHipError, check, on_device, ptr, require_cuda, stream_ptr

ROW = 20                        # doubles per observation in the workspace


class Plan:
    """The index arrays of one adjustment, all int32 device tensors: track_off [npt + 1], cam_idx, pt_idx [nobs], cam_off [ncam + 1],
    cam_obs [nobs]."""
    __slots__ = ("ncam", "npt", "nobs", "track_off", "cam_idx", "pt_idx", "cam_off", "cam_obs", "device")

    def __init__(self, ncam, npt, track_off, cam_idx, pt_idx, cam_off, cam_obs):
        self.ncam, self.npt, self.nobs = int(ncam), int(npt), int(cam_idx.numel())
        self.track_off, self.cam_idx, self.pt_idx, self.cam_off, self.cam_obs = track_off, cam_idx, pt_idx, cam_off, cam_obs
        self.device = track_off.device
        for name, n in (("track_off", self.npt + 1), ("cam_off", self.ncam + 1), ("cam_idx", self.nobs), ("pt_idx", self.nobs), ("cam_obs", self.nobs)):
            t = getattr(self, name)
            require_cuda(t)
            if t.dtype != torch.int32 or not t.is_contiguous() or t.numel() != n:
                raise SfmHipError(f"track_ba: {name} must be a contiguous int32 device tensor of {n} words")

    def ws_bytes(self):
        n = _lib.lib().sfm_track_ba_ws_bytes(self.ncam, self.npt, self.nobs)
        if n == 0:
            raise SfmHipError(f"track_ba: sizes ncam {self.ncam}, npt {self.npt}, nobs {self.nobs} are outside the limits of sfm_track_ba_ws_bytes")
        return n

    def workspace(self):
        """A workspace of its own: it holds the rows of ONE linearisation (a trial sweep needs a second one)."""
        return torch.empty(self.ws_bytes(), dtype=torch.uint8, device=self.device)

    def _args(self):
        n = self.nobs
        return (ptr(self.track_off), ptr(self.cam_idx) if n else None, ptr(self.pt_idx) if n else None, ptr(self.cam_off),
                ptr(self.cam_obs) if n else None, n)


def plan(cam_idx, pt_idx, ncam, npt):
    """track_off, cam_off and cam_obs of point-major observations (pt_idx ascending, as `tracks.run_tracks` returns them), with torch
    on the device: counts per row (index_add_), cumsum, a stable argsort.  Indices outside their range are left to the kernels, which skip them; they
    are counted in no row.  No host wait."""
    require_cuda(cam_idx, pt_idx)
    dev = cam_idx.device
    ci = cam_idx.contiguous().to(torch.int32).reshape(-1)
    pi = pt_idx.contiguous().to(torch.int32).reshape(-1)
    if ci.numel() != pi.numel():
        raise SfmHipError("track_ba.plan: cam_idx and pt_idx differ in length")
    ncam, npt = int(ncam), int(npt)

    def csr(idx, n):
        ok = (idx >= 0) & (idx < n)
        key = torch.where(ok, idx.long(), torch.full_like(idx, n, dtype=torch.int64))           # out of range: behind every row
        count = torch.zeros(n + 1, dtype=torch.int64, device=dev)                                # (torch.bincount waits for the host: it reads
        count.index_add_(0, key, torch.ones_like(key))                                          # the largest key; integer adds have no order)
        off = torch.zeros(n + 2, dtype=torch.int64, device=dev)
        off[1:] = torch.cumsum(count, 0)
        return key, off[:n + 1].to(torch.int32).contiguous()

    _, track_off = csr(pi, npt)
    key, cam_off = csr(ci, ncam)
    cam_obs = torch.argsort(key, stable=True).to(torch.int32).contiguous()
    return Plan(ncam, npt, track_off, ci, pi, cam_off, cam_obs)


def _f64(t, shape, what):
    require_cuda(t)
    if t.dtype != torch.float64 or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise SfmHipError(f"track_ba: {what} must be a contiguous float64 device tensor of shape {tuple(shape)}")
    return t


def rows_of(pl, ws):
    """The rows a sweep left in `ws`: float64 [nobs, 20] (a view)."""
    base = (-ws.data_ptr()) % 256
    return ws[base:base + pl.nobs * ROW * 8].view(torch.float64).view(pl.nobs, ROW)


def sweep(pl, cams, K, X, obs, huber=None, mode=0, active=None, ws=None, out=None):
    """sfm_track_ba_sweep at (cams [ncam, 6] f64, X [npt, 3] f64) -> dict(JtJ_cam, Jtr_cam, JtJ_pt, Jtr_pt, stat [2] f64, count [3] i32,
    active [nobs] u8, ws).  mode 0 writes `active`, mode 1 reads it.  huber None or inf: plain least squares.  No host wait."""
    dev = pl.device
    cams = _f64(cams, (pl.ncam, 6), "cams")
    X = _f64(X, (pl.npt, 3), "X")
    require_cuda(obs)
    if obs.dtype != torch.float32 or tuple(obs.shape) != (pl.nobs, 2) or not obs.is_contiguous():
        raise SfmHipError("track_ba.sweep: obs must be a contiguous float32 [nobs, 2] device tensor")
    if mode == 1 and active is None:
        raise SfmHipError("track_ba.sweep: mode 1 reads the active set of a mode-0 sweep")
    if active is None:
        active = torch.empty(pl.nobs, dtype=torch.uint8, device=dev)
    elif active.dtype != torch.uint8 or active.numel() != pl.nobs or not active.is_contiguous():
        raise SfmHipError("track_ba.sweep: active must be a contiguous uint8 [nobs] device tensor")
    ws = pl.workspace() if ws is None else ws
    if out is None:
        f64 = dict(dtype=torch.float64, device=dev)
        out = dict(JtJ_cam=torch.empty((pl.ncam, 36), **f64), Jtr_cam=torch.empty((pl.ncam, 6), **f64), JtJ_pt=torch.empty((pl.npt, 9), **f64),
                   Jtr_pt=torch.empty((pl.npt, 3), **f64), stat=torch.empty(2, **f64), count=torch.empty(3, dtype=torch.int32, device=dev))
    k = np.ascontiguousarray(np.asarray(K, np.float64).reshape(9))
    h = float("inf") if huber is None else float(huber)
    with on_device(dev):
        check(_lib.lib().sfm_track_ba_sweep(ptr(cams), pl.ncam, k.ctypes.data_as(ctypes.c_void_p), ptr(X), pl.npt, ptr(obs) if pl.nobs else None,
                                            *pl._args(), h, int(mode), ptr(active) if pl.nobs else None, ptr(out["JtJ_cam"]), ptr(out["Jtr_cam"]),
                                            ptr(out["JtJ_pt"]), ptr(out["Jtr_pt"]), ptr(out["stat"]), ptr(out["count"]), ptr(ws), ws.numel(),
                                            stream_ptr()), "sfm_track_ba_sweep")
    out["active"], out["ws"] = active, ws
    return out


def product(pl, ws, vec, mode):
    """sfm_track_ba_product over the rows in `ws`: mode 0 W^T vec ([ncam, 6] -> [npt, 3]), mode 1 W vec ([npt, 3] -> [ncam, 6])."""
    vec = _f64(vec, (pl.ncam, 6) if mode == 0 else (pl.npt, 3), "vec")
    out = torch.empty((pl.npt, 3) if mode == 0 else (pl.ncam, 6), dtype=torch.float64, device=pl.device)
    with on_device(pl.device):
        check(_lib.lib().sfm_track_ba_product(pl.ncam, pl.npt, *pl._args(), int(mode), ptr(vec), ptr(out), ptr(ws), ws.numel(), stream_ptr()),
              "sfm_track_ba_product")
    return out


def step(pl, blocks, lam, fix_first_camera=True, cg_tol=1e-10, cg_iters=200):
    """sfm_track_ba_step on the blocks and rows of `blocks` (a dict `sweep` returned) -> (dc [ncam, 6], dp [npt, 3], CG iterations,
    status bits).  The update is parameters - step."""
    dc = torch.empty((pl.ncam, 6), dtype=torch.float64, device=pl.device)
    dp = torch.empty((pl.npt, 3), dtype=torch.float64, device=pl.device)
    it, st = ctypes.c_int32(0), ctypes.c_int32(0)
    ws = blocks["ws"]
    with on_device(pl.device):
        check(_lib.lib().sfm_track_ba_step(pl.ncam, pl.npt, *pl._args(), ptr(_f64(blocks["JtJ_cam"], (pl.ncam, 36), "JtJ_cam")),
                                           ptr(_f64(blocks["Jtr_cam"], (pl.ncam, 6), "Jtr_cam")), ptr(_f64(blocks["JtJ_pt"], (pl.npt, 9), "JtJ_pt")),
                                           ptr(_f64(blocks["Jtr_pt"], (pl.npt, 3), "Jtr_pt")), float(lam), int(bool(fix_first_camera)), float(cg_tol),
                                           int(cg_iters), ptr(dc), ptr(dp), ctypes.byref(it), ctypes.byref(st), ptr(ws), ws.numel(), stream_ptr()),
              "sfm_track_ba_step")
    return dc, dp, it.value, st.value


def _read(blocks):
    """The ONE host wait of a sweep: (robust cost, plain cost, active, crossed, outliers)."""
    h = torch.cat([blocks["stat"], blocks["count"].to(torch.float64)]).cpu().numpy()
    return float(h[0]), float(h[1]), int(h[2]), int(h[3]), int(h[4])


def bundle_adjust_tracks(cams, K, X, obs, cam_idx, pt_idx, huber=None, iters=10, lam=1e-3, fix_first_camera=True, cg_tol=1e-10, cg_iters=200,
                         log=None):
    """Levenberg-Marquardt on the robust cost with the joint Schur step.  cams [ncam, 6] (rvec, tvec), X [npt, 3] (any float dtype; the
    solver keeps float64), obs [nobs, 2] float32, cam_idx / pt_idx [nobs] point-major: device tensors.  huber: the Huber width in
    px (None: plain least squares).  The loop of `ba.bundle_adjust_schur`: up to 8 attempts per iteration, lambda / 3 on success and
    * 4 on failure, stop at a relative gain below 1e-9.  A trial is accepted iff no active observation crossed its camera plane and
    the cost is strictly lower.  Returns (cams, X float64, history of robust costs, info)."""
    require_cuda(cams, X, obs, cam_idx, pt_idx)
    cams = cams.detach().to(torch.float64).reshape(-1, 6).contiguous().clone()
    X = X.detach().to(torch.float64).reshape(-1, 3).contiguous().clone()
    obs = obs.to(torch.float32).reshape(-1, 2).contiguous()
    pl = plan(cam_idx, pt_idx, cams.shape[0], X.shape[0])
    say = log or (lambda *a: None)
    spare = pl.workspace()
    blocks = sweep(pl, cams, K, X, obs, huber, 0)
    active = blocks["active"]
    cost, plain, n_active, _, n_out = _read(blocks)
    hist, cg, refused = [cost], [], 0
    for it in range(iters):
        accepted, gain = False, 0.0
        for _ in range(8):
            dc, dp, ncg, status = step(pl, blocks, lam, fix_first_camera, cg_tol, cg_iters)
            cg.append(ncg)
            c_new, x_new = cams - dc, X - dp
            trial = sweep(pl, c_new, K, x_new, obs, huber, 1, active, spare)
            cost_new, plain_new, _, crossed, out_new = _read(trial)
            if crossed > 0:
                refused += 1
            if crossed == 0 and cost_new < cost:
                spare = blocks["ws"]
                cams, X, blocks, accepted = c_new, x_new, trial, True
                gain = (cost - cost_new) / cost
                cost, plain, n_out, lam = cost_new, plain_new, out_new, max(lam / 3.0, 1e-12)
                say(f"track-ba iter {it}: cost {cost:.6g} lambda {lam:.2g} cg {ncg} outliers {n_out}")
                break
            lam *= 4.0
        hist.append(cost)
        if not accepted or gain < 1e-9:
            break
    info = dict(active=n_active, crossed_refusals=refused, outliers=n_out, plain_cost=plain, cg_iters=cg, lam=lam)
    return cams, X, hist, info


def cams_from_P(P, K):
    """[R | t] = K^-1 P -> cams [n, 6] (rvec, tvec) float64 on the host, the rotation through `hostgeom.rodrigues_mat2vec`
    (sfm_host_rodrigues orthonormalises first)."""
    P = np.asarray(P, np.float64).reshape(-1, 3, 4)
    Kinv = np.linalg.inv(np.asarray(K, np.float64).reshape(3, 3))
    cams = np.empty((len(P), 6))
    for i, p in enumerate(P):
        Rt = Kinv @ p
        cams[i, :3] = hostgeom.rodrigues_mat2vec(Rt[:, :3])
        cams[i, 3:] = Rt[:, 3]
    return cams


def P_from_cams(cams, K):
    """cams [n, 6] -> P [n, 3, 4] = K [R(rvec) | tvec] float64 on the host (`hostgeom.rodrigues_vec2mat`)."""
    cams = np.asarray(cams, np.float64).reshape(-1, 6)
    K = np.asarray(K, np.float64).reshape(3, 3)
    return np.stack([K @ np.c_[hostgeom.rodrigues_vec2mat(c[:3]), c[3:]] for c in cams]) if len(cams) else np.empty((0, 3, 4))
