"""Planning the MVS views from the sparse model (include/sfm_hip.h, "MVS-PLAN"; csrc/mvs_plan.hip; docs/mvs.md §8): which views a view
is swept against and over which depths, from the tracks instead of from the order of the frames.

`pair_counts`, `depth_ranges` and `select` take and return device tensors and never wait for the host; they take the index arrays as a
`track_ba.Plan`.  `plan_views` chains them, `host_plan` downloads the result with ONE host wait and applies `mvs.depth_range`'s
widening and pooling rule to the per-view figures: its `neighbours` and `ranges` are the keywords of `mvs.run_mvs`."""
import numpy as np
import torch

from . import _lib
from ._lib import SfmHipError, check, on_device, ptr, require_cuda, stream_ptr

MAX_SRC = 8                     # SFM_PLAN_MAX_SRC = mvs.MAX_VIEWS
LDS_CAMS = 96                   # SFM_PLAN_LDS_CAMS: above it the pair counts take the global-atomic path
MIN_DEPTHS = 8                  # a view with fewer valid depths takes the pooled range (the rule of mvs.depth_range)
# Defaults of plan_views, calibrated with tests/np_mvs_plan.py on the scenes of docs/mvs.md §8.4
MIN_ANGLE_DEG = 1.0             # a pair of rays closer than this constrains no depth
MAX_ANGLE_DEG = 30.0            # beyond it the fronto-parallel windows of the sweep stop matching
MIN_GOOD = 8                    # points a source has to share with the view inside the window


def cos_window(min_angle_deg, max_angle_deg):
    """(cos_lo, cos_hi) of an angle window in degrees: the device compares cosines."""
    lo, hi = float(min_angle_deg), float(max_angle_deg)
    if not (0.0 <= lo <= hi <= 180.0):
        raise SfmHipError(f"mvs_plan: the angle window needs 0 <= min <= max <= 180 degrees (got {lo}, {hi})")
    return float(np.cos(np.deg2rad(hi))), float(np.cos(np.deg2rad(lo)))


def _inputs(pl, X, P):
    require_cuda(X, P)
    if X.dtype != torch.float64 or tuple(X.shape) != (pl.npt, 3) or not X.is_contiguous():
        raise SfmHipError(f"mvs_plan: X must be a contiguous float64 device tensor of shape ({pl.npt}, 3)")
    if P.dtype != torch.float64 or P.numel() != 12 * pl.ncam or not P.is_contiguous():
        raise SfmHipError(f"mvs_plan: P must be a contiguous float64 device tensor of {pl.ncam} x 12 words")
    return X, P


def pair_counts(pl, X, P, cos_lo, cos_hi, out=None):
    """sfm_view_pair_counts -> (shared [ncam, ncam] i32, good [ncam, ncam] i32, C [ncam, 3] f64).  No host wait."""
    X, P = _inputs(pl, X, P)
    dev, n = pl.device, pl.ncam
    if out is None:
        out = (torch.empty((n, n), dtype=torch.int32, device=dev), torch.empty((n, n), dtype=torch.int32, device=dev),
               torch.empty((n, 3), dtype=torch.float64, device=dev))
    shared, good, C = out
    with on_device(dev):
        check(_lib.lib().sfm_view_pair_counts(ptr(pl.track_off), ptr(pl.cam_idx) if pl.nobs else None, ptr(X) if pl.npt else None, pl.npt, pl.nobs,
                                              ptr(P), n, float(cos_lo), float(cos_hi), ptr(C), ptr(shared), ptr(good), stream_ptr()),
              "sfm_view_pair_counts")
    return shared, good, C


def depth_ranges(pl, X, P, lo_permille=20, hi_permille=980, out=None):
    """sfm_view_depth_ranges -> (m [ncam] i32, z_lo [ncam] f32, z_hi [ncam] f32).  No host wait."""
    X, P = _inputs(pl, X, P)
    dev, n, k = pl.device, pl.ncam, pl.nobs
    if out is None:
        out = (torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.float32, device=dev),
               torch.empty(n, dtype=torch.float32, device=dev))
    m, z_lo, z_hi = out
    with on_device(dev):
        check(_lib.lib().sfm_view_depth_ranges(ptr(pl.cam_off), ptr(pl.cam_obs) if k else None, ptr(pl.cam_idx) if k else None,
                                               ptr(pl.pt_idx) if k else None, k, ptr(X) if pl.npt else None, pl.npt, ptr(P), n, int(lo_permille),
                                               int(hi_permille), ptr(m), ptr(z_lo), ptr(z_hi), stream_ptr()), "sfm_view_depth_ranges")
    return m, z_lo, z_hi


def select(shared, good, nsrc=4, min_good=MIN_GOOD, out=None):
    """sfm_view_select -> (nbr [ncam, nsrc] i32, -1 padded; n_nbr [ncam] i32).  No host wait."""
    require_cuda(shared, good)
    n = int(shared.shape[0]) if shared.dim() == 2 else -1
    for t in (shared, good):
        if t.dtype != torch.int32 or tuple(t.shape) != (n, n) or not t.is_contiguous():
            raise SfmHipError("mvs_plan.select: shared and good must be contiguous int32 [ncam, ncam] device tensors")
    dev = shared.device
    if out is None:
        out = (torch.empty((n, max(int(nsrc), 0)), dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev))
    nbr, n_nbr = out
    with on_device(dev):
        check(_lib.lib().sfm_view_select(ptr(shared), ptr(good), n, int(nsrc), int(min_good), ptr(nbr), ptr(n_nbr), stream_ptr()), "sfm_view_select")
    return nbr, n_nbr


def plan_views(pl, X, P, nsrc=4, min_angle_deg=MIN_ANGLE_DEG, max_angle_deg=MAX_ANGLE_DEG, min_good=MIN_GOOD, lo=2, hi=98):
    """The three kernels on one stream, no host wait: pl a `track_ba.Plan`, X [npt, 3] and P [ncam, 3, 4] float64 device tensors; the
    angle window in degrees, lo / hi in per cent (as mvs.depth_range takes them).  Returns a dict of device tensors: shared, good, C,
    nbr, n_nbr, m, z_lo, z_hi."""
    cos_lo, cos_hi = cos_window(min_angle_deg, max_angle_deg)
    shared, good, C = pair_counts(pl, X, P, cos_lo, cos_hi)
    m, z_lo, z_hi = depth_ranges(pl, X, P, int(round(10 * lo)), int(round(10 * hi)))
    nbr, n_nbr = select(shared, good, nsrc, min_good)
    return dict(shared=shared, good=good, C=C, nbr=nbr, n_nbr=n_nbr, m=m, z_lo=z_lo, z_hi=z_hi)


def pooled_ranges(m, z_lo, z_hi):
    """Host rule of `host_plan`: ranges [ncam, 2] = (0.8 z_lo, 1.25 z_hi); a view with m < 8 takes the smallest z_lo and the largest z_hi
    among the views with m >= 8 (mvs.depth_range's pooling, restated on the per-view figures)."""
    m = np.asarray(m, np.int64)
    z_lo, z_hi = np.asarray(z_lo, np.float32).astype(np.float64), np.asarray(z_hi, np.float32).astype(np.float64)
    enough = m >= MIN_DEPTHS
    if not enough.any():
        raise SfmHipError(f"mvs_plan: no view observes {MIN_DEPTHS} sparse points in front of it (the most: {int(m.max()) if len(m) else 0})")
    a = np.where(enough, z_lo, z_lo[enough].min())
    b = np.where(enough, z_hi, z_hi[enough].max())
    return np.stack([0.8 * a, 1.25 * b], 1)


def host_plan(planned):
    """Downloads what `plan_views` returned with ONE host wait -> dict(neighbours: list over views of lists of view indices,
    ranges [ncam, 2] float64 (dmin, dmax), m [ncam], shared, good [ncam, ncam])."""
    n, nsrc = planned["nbr"].shape
    words = torch.cat([planned["nbr"].reshape(-1), planned["n_nbr"], planned["m"], planned["z_lo"].view(torch.int32), planned["z_hi"].view(torch.int32),
                       planned["shared"].reshape(-1), planned["good"].reshape(-1)]).cpu().numpy()                # the one host wait
    pos = np.cumsum([0, n * nsrc, n, n, n, n, n * n, n * n])
    nbr, n_nbr, m = words[pos[0]:pos[1]].reshape(n, nsrc), words[pos[1]:pos[2]], words[pos[2]:pos[3]]
    z_lo, z_hi = words[pos[3]:pos[4]].view(np.float32), words[pos[4]:pos[5]].view(np.float32)
    return dict(neighbours=[[int(v) for v in nbr[i, :n_nbr[i]]] for i in range(n)], ranges=pooled_ranges(m, z_lo, z_hi), m=m.copy(),
                shared=words[pos[5]:pos[6]].reshape(n, n).copy(), good=words[pos[6]:pos[7]].reshape(n, n).copy())
