"""Plane-sweep multi-view stereo: the dense half of sfm-mvs (sfm.py:298 `densify = False`; the dense.ply branch of to_ply,
sfm.py:194-201, that the reference never feeds).

Thin, validating wrappers over `sfm_mvs_plane_sweep` and `sfm_mvs_consistency` (include/sfm_hip.h) and the opt-in steps between and
after them (aggregation, PatchMatch refinement, merging fusion): device tensors in, device tensors out, stream ordered, no CPU path.  The host part is the geometry of a handful of 3x3 matrices per view (float64, cast
once to float32) and the choice of the depth range from the sparse cloud.  docs/mvs.md describes the algorithm and its numbers.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import SfmHipError, check, on_device, ptr, require_cuda, stream_ptr

MAX_VIEWS = 8       # sources per sweep, neighbours per consistency check


def _rt(K, P):
    """[R|t] = K^-1 P (float64)."""
    Rt = np.linalg.solve(np.asarray(K, np.float64), np.asarray(P, np.float64).reshape(3, 4))
    return Rt[:, :3], Rt[:, 3]


def _inverse_depths_host(dmin, dmax, ndepth):
    dmin, dmax, ndepth = float(dmin), float(dmax), int(ndepth)
    if not (0.0 < dmin < dmax < np.inf) or ndepth < 2:
        raise SfmHipError(f"inverse_depths: need 0 < dmin < dmax and ndepth >= 2 (got {dmin}, {dmax}, {ndepth})")
    return np.linspace(1.0 / dmax, 1.0 / dmin, ndepth, dtype=np.float64).astype(np.float32)


def _upload(a, device):
    """Host array -> device tensor without a host wait: staged in pinned memory, copied on the current stream (the pinned block
    is kept until that copy has run).  A pageable upload would synchronise the stream."""
    return torch.from_numpy(np.ascontiguousarray(a)).pin_memory().to(device, non_blocking=True)


def inverse_depths(dmin, dmax, ndepth, device=None):
    """`ndepth` plane inverse depths uniform between 1/dmax and 1/dmin (ascending: far to near), computed in float64 and returned
    as a float32 device tensor (stream-ordered upload, no host wait)."""
    return _upload(_inverse_depths_host(dmin, dmax, ndepth), device if device is not None else torch.device("cuda"))


def _camera_depths(X, P):
    # P = K [R|t] with K's last row (0, 0, 1): P's third row is [R|t]'s, the camera depth of X
    P = np.asarray(P, np.float64).reshape(3, 4)
    return X @ P[2, :3] + P[2, 3]


def depth_range(Xtot, P_ref, lo=2, hi=98, P_all=None):
    """(dmin, dmax) of the plane sweep of the camera P_ref: the lo / hi percentiles of the sparse points' camera depths, widened
    by x0.8 and x1.25.  Monocular SfM fixes no scale, so the range has to come from the cloud.  With fewer than 8 points in front
    of P_ref, the depths of the points in front of every camera of P_all (when given) are pooled instead."""
    X = np.asarray(Xtot, np.float64).reshape(-1, 3)
    z = _camera_depths(X, P_ref)
    z = z[z > 0]
    if len(z) < 8 and P_all is not None:
        z = np.concatenate([_camera_depths(X, P) for P in np.asarray(P_all, np.float64).reshape(-1, 3, 4)])
        z = z[z > 0]
    if len(z) < 8:
        raise SfmHipError(f"depth_range: only {len(z)} sparse points lie in front of the camera(s)")
    a, b = np.percentile(z, [lo, hi])
    return 0.8 * float(a), 1.25 * float(b)


def neighbours(i, n, nsrc=4):
    """The `nsrc` views nearest to view i in sequence order (i-1, i+1, i-2, i+2, ...), clipped to 0..n-1: the reference's
    frames follow a camera path.  Near the ends of the sequence the list continues on the one side that is left."""
    out = []
    for d in range(1, n):
        for v in (i - d, i + d):
            if 0 <= v < n and len(out) < nsrc:
                out.append(v)
    return out


_sequence_neighbours = neighbours       # run_mvs has a keyword of that name


def _relative(K, P_ref, P_other):
    """(G, g): the pixel of the reference at depth d maps to d*(G x~) + g in the other camera (homogeneous, its z the camera
    depth there): G = K R_o R_r^T K^-1, g = K (t_o - R_o R_r^T t_r)."""
    K = np.asarray(K, np.float64)
    Rr, tr = _rt(K, P_ref)
    Ro, to = _rt(K, P_other)
    Rrel = Ro @ Rr.T
    return K @ Rrel @ np.linalg.inv(K), K @ (to - Rrel @ tr)


def sweep_matrices(K, P_ref, P_srcs):
    """float32 [nsrc, 12] = M_s (3x3 row-major) | v_s per source: a reference pixel on the plane of inverse depth q maps to
    M_s x~ + v_s q (homogeneous) in source s."""
    out = np.empty((len(P_srcs), 12), np.float64)
    for s, P in enumerate(P_srcs):
        M, v = _relative(K, P_ref, P)
        out[s, :9], out[s, 9:] = M.ravel(), v
    return out.astype(np.float32)


def consistency_matrices(K, P_ref, P_nbrs):
    """(ab float32 [nview, 12] = A_v | b_v per neighbour — the same formula as sweep_matrices —, bc float32 [12] = B | c with
    B = R_r^T K^-1, c = -R_r^T t_r: the world point of reference pixel x~ at depth d is d*(B x~) + c)."""
    K = np.asarray(K, np.float64)
    ab = sweep_matrices(K, P_ref, P_nbrs).reshape(-1, 12)
    Rr, tr = _rt(K, P_ref)
    bc = np.concatenate([(Rr.T @ np.linalg.inv(K)).ravel(), -Rr.T @ tr])
    return ab, bc.astype(np.float32)


def _gray(t):
    if t.dtype != torch.uint8 or t.dim() != 2:
        raise SfmHipError("mvs: gray frames must be (H, W) uint8 device tensors")
    return t.contiguous()


def plane_sweep(ref, srcs, mv, invd, radius=3, topk=2, var_min=None, cost_max=None, plane=False, volume=False, volume_out=None):
    """Depth map of the gray reference frame `ref` against the gray `srcs` (sfm_mvs_plane_sweep).
    ref, srcs: (H, W) uint8 device tensors; mv: float32 [nsrc, 12] (sweep_matrices); invd: float32 [ndepth] device tensor.
    volume_out: an optional contiguous [ndepth, H, W] float32 device tensor the volume is written to (implies volume=True).
    Returns (depth, cost, plane or None, volume or None): [H, W] float32, [H, W] float32, [H, W] int32, [ndepth, H, W] float32."""
    var_min = VAR_MIN if var_min is None else var_min
    cost_max = COST_MAX if cost_max is None else cost_max
    require_cuda(ref, invd, *srcs)
    ref = _gray(ref)
    srcs = [_gray(s) for s in srcs]
    h, w = ref.shape
    if any(s.shape != ref.shape or s.device != ref.device for s in srcs):
        raise SfmHipError("plane_sweep: every source frame must have the reference's size and device")
    if invd.dtype != torch.float32 or invd.dim() != 1 or invd.device != ref.device:
        raise SfmHipError("plane_sweep: invd must be a float32 vector on the reference's device")
    invd = invd.contiguous()
    mv = np.ascontiguousarray(np.asarray(mv, np.float32).reshape(-1, 12))
    if len(mv) != len(srcs):
        raise SfmHipError(f"plane_sweep: {len(srcs)} sources but {len(mv)} matrices")
    nd = invd.numel()
    dev = ref.device
    depth = torch.empty((h, w), dtype=torch.float32, device=dev)
    cost = torch.empty((h, w), dtype=torch.float32, device=dev)
    pl = torch.empty((h, w), dtype=torch.int32, device=dev) if plane else None
    vol = volume_out if volume_out is not None else torch.empty((nd, h, w), dtype=torch.float32, device=dev) if volume else None
    if vol is not None and (vol.shape != (nd, h, w) or vol.dtype != torch.float32 or vol.device != dev or not vol.is_contiguous()):
        raise SfmHipError("plane_sweep: volume_out must be a contiguous [ndepth, H, W] float32 tensor on the reference's device")
    src_ptrs = (ctypes.c_void_p * max(len(srcs), 1))(*[s.data_ptr() for s in srcs])
    with on_device(dev):
        check(_lib.lib().sfm_mvs_plane_sweep(ptr(ref), src_ptrs, mv.ctypes.data_as(ctypes.c_void_p), len(srcs), w, h, ptr(invd), nd,
                                             int(radius), int(topk), float(var_min), float(cost_max), ptr(depth), ptr(cost), ptr(pl),
                                             ptr(vol), stream_ptr()), "sfm_mvs_plane_sweep")
    return depth, cost, pl, vol


def consistency(depth, nbr_depths, nbr_index, ab, ref_index, bc, tau=0.01, min_consistent=2, unique=True, mask_out=None, xyz_out=None):
    """Geometric-consistency mask of a reference depth map and the world point of each kept pixel (sfm_mvs_consistency).
    depth, nbr_depths: [H, W] float32 device tensors; nbr_index: the neighbours' view indices; ab, bc: consistency_matrices.
    mask_out / xyz_out: optional contiguous [H, W] uint8 / [H, W, 3] float32 outputs (e.g. one view's slice of a stacked buffer).
    Returns (mask, xyz)."""
    require_cuda(depth, *nbr_depths)
    if depth.dtype != torch.float32 or depth.dim() != 2 or any(d.shape != depth.shape or d.dtype != torch.float32 for d in nbr_depths):
        raise SfmHipError("consistency: depth maps must be [H, W] float32 of one size")
    depth = depth.contiguous()
    nbr_depths = [d.contiguous() for d in nbr_depths]
    h, w = depth.shape
    dev = depth.device
    ab = np.ascontiguousarray(np.asarray(ab, np.float32).reshape(-1, 12))
    bc = np.ascontiguousarray(np.asarray(bc, np.float32).reshape(12))
    idx = np.ascontiguousarray(np.asarray(nbr_index, np.int32).reshape(-1))
    if len(ab) != len(nbr_depths) or len(idx) != len(nbr_depths):
        raise SfmHipError("consistency: one matrix and one view index per neighbour depth map")
    mask = torch.empty((h, w), dtype=torch.uint8, device=dev) if mask_out is None else mask_out
    xyz = torch.empty((h, w, 3), dtype=torch.float32, device=dev) if xyz_out is None else xyz_out
    if mask.shape != (h, w) or mask.dtype != torch.uint8 or not mask.is_contiguous() or xyz.shape != (h, w, 3) \
            or xyz.dtype != torch.float32 or not xyz.is_contiguous():
        raise SfmHipError("consistency: mask_out / xyz_out must be contiguous [H, W] uint8 / [H, W, 3] float32")
    dptrs = (ctypes.c_void_p * max(len(nbr_depths), 1))(*[d.data_ptr() for d in nbr_depths])
    with on_device(dev):
        check(_lib.lib().sfm_mvs_consistency(ptr(depth), dptrs, idx.ctypes.data_as(ctypes.c_void_p), ab.ctypes.data_as(ctypes.c_void_p),
                                             len(nbr_depths), int(ref_index), bc.ctypes.data_as(ctypes.c_void_p), w, h, float(tau),
                                             int(min_consistent), 1 if unique else 0, ptr(mask), ptr(xyz), stream_ptr()),
              "sfm_mvs_consistency")
    return mask, xyz


def _volume_u16(t, what):
    if not torch.is_tensor(t) or t.dtype != torch.uint16 or t.dim() != 3:
        raise SfmHipError(f"{what}: needs a [ndepth, H, W] uint16 device tensor")
    require_cuda(t)
    return t.contiguous()


def _out_like(out, shape, dtype, dev, what):
    if out is None:
        return torch.empty(shape, dtype=dtype, device=dev)
    if tuple(out.shape) != tuple(shape) or out.dtype != dtype or out.device != dev or not out.is_contiguous():
        raise SfmHipError(f"{what}: out must be a contiguous {tuple(shape)} {dtype} tensor on the input's device")
    return out


def quantise_cost(c):
    """q(c) of include/sfm_hip.h ("MVS-AGGREGATE") for one host float: the integer cost at 1/1024 (a NaN gives 2048)."""
    c = np.float32(c)
    if not c < np.float32(2):
        return 2048
    return int(np.floor(c * np.float32(1024) + np.float32(0.5))) if c > np.float32(0) else 0


def cost_shift(volume, shift, out=None):
    """Quantised, shiftable-window cost volume (sfm_mvs_cost_shift): float32 [ndepth, H, W] -> uint16 Q of the same shape, the
    minimum of round(1024 c) over the (2 shift + 1)^2 taps in the frame; shift 0..4."""
    require_cuda(volume)
    if volume.dtype != torch.float32 or volume.dim() != 3:
        raise SfmHipError("cost_shift: volume must be a [ndepth, H, W] float32 device tensor")
    volume = volume.contiguous()
    nd, h, w = volume.shape
    q = _out_like(out, volume.shape, torch.uint16, volume.device, "cost_shift")
    with on_device(volume.device):
        check(_lib.lib().sfm_mvs_cost_shift(ptr(volume), w, h, nd, int(shift), ptr(q), stream_ptr()), "sfm_mvs_cost_shift")
    return q


def cost_aggregate(q, p1=None, p2=None, ndir=8, out=None):
    """Semi-global path costs of Q summed over `ndir` (4 or 8) directions (sfm_mvs_cost_aggregate): uint16 [ndepth, H, W] -> uint16
    S of the same shape; integer penalties 0 <= p1 <= p2 <= 2048 in units of 1/1024 (defaults P1, P2)."""
    q = _volume_u16(q, "cost_aggregate")
    nd, h, w = q.shape
    s = _out_like(out, q.shape, torch.uint16, q.device, "cost_aggregate")
    with on_device(q.device):
        check(_lib.lib().sfm_mvs_cost_aggregate(ptr(q), w, h, nd, int(P1 if p1 is None else p1), int(P2 if p2 is None else p2), int(ndir),
                                                ptr(s), stream_ptr()), "sfm_mvs_cost_aggregate")
    return s


def cost_depth(s, q, invd, gate, plane=True):
    """Depth map of an aggregated volume (sfm_mvs_cost_depth): the first plane of smallest S, the sweep's parabola on S, no depth
    where Q there is >= the integer `gate`.  Returns (depth [H, W] float32, cost [H, W] float32 = Q/1024, plane [H, W] int32 or
    None)."""
    s, q = _volume_u16(s, "cost_depth"), _volume_u16(q, "cost_depth")
    require_cuda(invd)
    nd, h, w = s.shape
    if q.shape != s.shape or q.device != s.device:
        raise SfmHipError("cost_depth: S and Q must have one shape and device")
    if invd.dtype != torch.float32 or invd.dim() != 1 or invd.numel() != nd or invd.device != s.device:
        raise SfmHipError("cost_depth: invd must be a float32 vector of ndepth entries on the volumes' device")
    invd = invd.contiguous()
    dev = s.device
    depth = torch.empty((h, w), dtype=torch.float32, device=dev)
    cost = torch.empty((h, w), dtype=torch.float32, device=dev)
    pl = torch.empty((h, w), dtype=torch.int32, device=dev) if plane else None
    with on_device(dev):
        check(_lib.lib().sfm_mvs_cost_depth(ptr(s), ptr(q), ptr(invd), w, h, nd, int(gate), ptr(depth), ptr(cost), ptr(pl), stream_ptr()),
              "sfm_mvs_cost_depth")
    return depth, cost, pl


def aggregate_depth(volume, invd, shift=None, p1=None, p2=None, ndir=8, cost_max=None, q_out=None, s_out=None):
    """The aggregated depth map of a sweep's cost volume: cost_shift, cost_aggregate, cost_depth with gate = q(cost_max).
    q_out / s_out: optional uint16 buffers of the volume's shape to reuse.  Returns (depth, cost, plane)."""
    q = cost_shift(volume, SHIFT if shift is None else shift, out=q_out)
    s = cost_aggregate(q, p1, p2, ndir, out=s_out)
    return cost_depth(s, q, invd, quantise_cost(COST_MAX if cost_max is None else cost_max))


# Defaults of run_mvs, chosen on the CPU model (tests/np_mvs.py) over the rendered scenes of tests/mvs_scenes.py
# (tests/test_mvs_cpu.py::test_algorithm_accuracy_on_a_rendered_scene; docs/mvs.md, "Calibration").
VAR_MIN = 200.0     # sum of squared deviations over the window: a (2r+1)^2 = 49-pixel window with a gray-level std of ~2
COST_MAX = 0.3      # aggregated 1 - ZNCC (top 2 of 4 sources) above which a pixel gets no depth
# Defaults of the opt-in aggregation (run_mvs(aggregate=True)), chosen by the sweep of docs/mvs.md §7 over the same scenes
# (tests/test_mvs_aggregate_cpu.py::test_calibration_on_the_rendered_scenes); penalties in units of 1/1024 of the cost
SHIFT = 3           # half-width of the shiftable window's min filter (run_mvs: None = the sweep's radius)
P1 = 10             # a change of one plane between neighbouring pixels
P2 = 102            # any larger change


# Defaults of the opt-in PatchMatch refinement (run_mvs(refine=True)), chosen on the CPU model (tests/np_mvs_patchmatch.py) over the
# grid of scripts/calibrate_mvs_patchmatch.py (tests/golden/mvs_patchmatch_calibration.json; docs/mvs.md §9)
PM_ITERS = 3        # red-black iterations (two half-sweeps each)
PM_DEPTH_STEP = 0.05  # relative perturbation of the inverse depth at iteration 0, halved every iteration
PM_FAR = True       # also propagate from the neighbours at distance 3


def normal_matrix(K, P_ref):
    """float32 [9] N = -R^T K^T (float64, cast once): N (A, B, C) is the world normal, towards the camera, of the plane whose inverse
    depth in the reference camera is A x + B y + C."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    R, _ = _rt(K, P_ref)
    return (-(R.T @ K.T)).ravel().astype(np.float32)


def patchmatch_refine(ref, srcs, mv, qmin, qmax, depth_init=None, K=None, P_ref=None, radius=3, topk=2, var_min=None, cost_max=None,
                      iters=PM_ITERS, far=PM_FAR, depth_step=PM_DEPTH_STEP, slope_step=None, seed=0, normals=True):
    """PatchMatch refinement of a depth map over slanted support planes (sfm_mvs_patchmatch; docs/mvs.md §9).
    ref, srcs, mv, radius, topk, var_min, cost_max: as plane_sweep; qmin, qmax: the admissible inverse depths (the sweep's first and
    last plane); depth_init: an [H, W] float32 device depth map to start from (None: a hashed start at every pixel).
    slope_step None means 1 / K[0, 0]: a relative slope of one unit of tan per focal length (K is then required); normals=True needs
    K and P_ref.  1 + 2*iters + 1 launches on the current stream, no host wait.
    Returns (depth [H, W] float32, cost [H, W] float32, normals [H, W, 3] float32 unit world normals facing the camera or None,
    state [H, W, 4] float32 (q0, a, b, cost))."""
    var_min = VAR_MIN if var_min is None else var_min
    cost_max = COST_MAX if cost_max is None else cost_max
    require_cuda(ref, depth_init, *srcs)
    ref = _gray(ref)
    srcs = [_gray(s) for s in srcs]
    h, w = ref.shape
    dev = ref.device
    if any(s.shape != ref.shape or s.device != dev for s in srcs):
        raise SfmHipError("patchmatch_refine: every source frame must have the reference's size and device")
    mv = np.ascontiguousarray(np.asarray(mv, np.float32).reshape(-1, 12))
    if len(mv) != len(srcs):
        raise SfmHipError(f"patchmatch_refine: {len(srcs)} sources but {len(mv)} matrices")
    if depth_init is not None:
        if depth_init.dtype != torch.float32 or depth_init.shape != ref.shape or depth_init.device != dev:
            raise SfmHipError("patchmatch_refine: depth_init must be an [H, W] float32 tensor on the reference's device")
        depth_init = depth_init.contiguous()
    if slope_step is None:
        if K is None:
            raise SfmHipError("patchmatch_refine: slope_step=None means 1 / K[0, 0]: pass K or a slope_step")
        slope_step = 1.0 / float(np.asarray(K, np.float64).reshape(3, 3)[0, 0])
    seed = int(seed)
    if not 0 <= seed < 2 ** 32:
        raise SfmHipError(f"patchmatch_refine: seed must be a uint32 (got {seed})")
    nmat = None
    if normals:
        if K is None or P_ref is None:
            raise SfmHipError("patchmatch_refine: normals=True needs K and P_ref")
        nmat = normal_matrix(K, P_ref)
    state = torch.empty((h, w, 4), dtype=torch.float32, device=dev)
    depth = torch.empty((h, w), dtype=torch.float32, device=dev)
    cost = torch.empty((h, w), dtype=torch.float32, device=dev)
    nrm = torch.empty((h, w, 3), dtype=torch.float32, device=dev) if normals else None
    src_ptrs = (ctypes.c_void_p * max(len(srcs), 1))(*[s.data_ptr() for s in srcs])
    with on_device(dev):
        check(_lib.lib().sfm_mvs_patchmatch(ptr(ref), src_ptrs, mv.ctypes.data_as(ctypes.c_void_p), len(srcs), w, h, float(qmin), float(qmax),
                                            int(radius), int(topk), float(var_min), float(cost_max), ptr(depth_init), int(iters),
                                            1 if far else 0, float(depth_step), float(slope_step), seed,
                                            None if nmat is None else nmat.ctypes.data_as(ctypes.c_void_p), ptr(state), ptr(depth), ptr(cost),
                                            ptr(nrm), stream_ptr()), "sfm_mvs_patchmatch")
    return depth, cost, nrm, state


# Default of the opt-in merging fusion (run_mvs(fuse=True)): the smallest angle of the grid of scripts/calibrate_mvs_fuse.py that keeps
# >= 95 % of the unbounded point count on both scenes under refine=True on every seed (tests/golden/mvs_fuse_calibration.json;
# docs/mvs.md §10)
FUSE_MAX_ANGLE = 45.0   # degrees between the normals of a pixel and of a consistent neighbour's pixel

# One view's record of sfm_mvs_fuse's table (include/sfm_hip.h, "MVS-FUSE"): 512 bytes, view indices only
FUSE_RECORD = np.dtype([("nnbr", np.int32), ("min_consistent", np.int32), ("nbr", np.int32, (MAX_VIEWS,)), ("bc", np.float32, (12,)),
                        ("ab", np.float32, (MAX_VIEWS, 12)), ("pad", np.int32, (10,))])
assert FUSE_RECORD.itemsize == 512
FUSE_MAX_N = 4096


def fuse_table(K, Ps, nbrs, min_consistent=2):
    """The host table of sfm_mvs_fuse: a FUSE_RECORD per view with its neighbours' indices in the caller's order, its own `bc` and one
    `ab` per neighbour (consistency_matrices, unchanged) and min(min_consistent, len(nbrs[i])), as run_mvs caps it per view.
    K 3x3, Ps [n, 3, 4], nbrs per view a list of at most MAX_VIEWS view indices (none the view itself)."""
    Ps = np.asarray(Ps, np.float64).reshape(-1, 3, 4)
    nbrs = _checked_neighbours(nbrs, len(Ps))
    mc = int(min_consistent)
    if mc < 0:
        raise SfmHipError(f"fuse_table: min_consistent {mc} is negative")
    # consistency_matrices' words with every camera decomposed once (the table is made before the first launch, while the device idles):
    # the same float64 expressions in the same order as _relative and consistency_matrices, cast once
    K = np.asarray(K, np.float64)
    Kinv = np.linalg.inv(K)
    rts = [_rt(K, P) for P in Ps]
    table = np.zeros(len(Ps), FUSE_RECORD)
    for i, row in enumerate(nbrs):
        Rr, tr = rts[i]
        ab = np.empty((len(row), 12), np.float64)
        for s, v in enumerate(row):
            Ro, to = rts[v]
            Rrel = Ro @ Rr.T
            ab[s, :9], ab[s, 9:] = (K @ Rrel @ Kinv).ravel(), K @ (to - Rrel @ tr)
        table[i]["nnbr"], table[i]["min_consistent"] = len(row), min(mc, len(row))
        table[i]["nbr"][:len(row)] = row
        table[i]["bc"] = np.concatenate([(Rr.T @ Kinv).ravel(), -Rr.T @ tr]).astype(np.float32)
        table[i]["ab"][:len(row)] = ab.astype(np.float32)
    return table


def _cos_min(max_angle):
    """cos_min of sfm_mvs_fuse for a bound in degrees (None: -inf, the test is off): the cosine in float64, cast once."""
    if max_angle is None:
        return float("-inf")
    a = float(max_angle)
    if not 0.0 <= a <= 180.0:
        raise SfmHipError(f"fuse: max_angle must be None or an angle of 0..180 degrees (got {max_angle!r})")
    return float(np.float32(np.cos(np.deg2rad(np.float64(a)))))


def fuse(depths, table, normals=None, frames=None, tau=0.01, max_angle=None, unique=True):
    """Merging fusion of the stacked depth maps of all views in one launch (sfm_mvs_fuse; docs/mvs.md §10).
    depths [n, H, W] float32, normals [n, H, W, 3] float32 or None, frames [n, H, W, 3] uint8 or None: contiguous device tensors;
    table: fuse_table's array (uploaded pinned and stream-ordered) or a uint8 [n, 512] device tensor already uploaded;
    max_angle: degrees (None: normals are averaged but not tested).
    Returns dict(mask [n, H, W] uint8, xyz [n, H, W, 3] float32, normals [n, H, W, 3] float32 or None, colors [n, H, W, 3] uint8 or
    None, support [n, H, W] uint8: the samples merged, 1 + the consistent neighbours).  No host wait."""
    if not torch.is_tensor(depths) or depths.dtype != torch.float32 or depths.dim() != 3:
        raise SfmHipError("fuse: depths must be an [n, H, W] float32 device tensor")
    require_cuda(depths, normals, frames)
    n, h, w = depths.shape
    dev = depths.device
    if not 1 <= n <= FUSE_MAX_N or not (1 <= w <= 32767 and 1 <= h <= 32767):
        raise SfmHipError(f"fuse: {n} views of {w} x {h}: needs 1..{FUSE_MAX_N} views and sides of 1..32767")
    for t, dt, what in ((depths, torch.float32, "depths"), (normals, torch.float32, "normals"), (frames, torch.uint8, "frames")):
        if t is None:
            continue
        want = (n, h, w) if what == "depths" else (n, h, w, 3)
        if tuple(t.shape) != want or t.dtype != dt or t.device != dev or not t.is_contiguous():
            raise SfmHipError(f"fuse: {what} must be a contiguous {want} {dt} tensor on the depths' device")
    tau = float(tau)
    if not (0.0 <= tau < np.inf):
        raise SfmHipError("fuse: tau must be finite and >= 0")
    cos_min = _cos_min(max_angle)
    if torch.is_tensor(table):
        require_cuda(table)
        if table.dtype != torch.uint8 or tuple(table.shape) != (n, FUSE_RECORD.itemsize) or table.device != dev or not table.is_contiguous():
            raise SfmHipError(f"fuse: a device table must be a contiguous uint8 [{n}, {FUSE_RECORD.itemsize}] tensor on the depths' device")
        table_dev = table
    else:
        table = np.asarray(table)
        if table.dtype != FUSE_RECORD or table.shape != (n,):
            raise SfmHipError(f"fuse: the table must hold one FUSE_RECORD per view ({n}); fuse_table makes it")
        table_dev = _upload(table.view(np.uint8).reshape(n, FUSE_RECORD.itemsize), dev)
    mask = torch.empty((n, h, w), dtype=torch.uint8, device=dev)
    xyz = torch.empty((n, h, w, 3), dtype=torch.float32, device=dev)
    support = torch.empty((n, h, w), dtype=torch.uint8, device=dev)
    nout = None if normals is None else torch.empty((n, h, w, 3), dtype=torch.float32, device=dev)
    cout = None if frames is None else torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev)
    with on_device(dev):
        check(_lib.lib().sfm_mvs_fuse(ptr(depths), ptr(normals), ptr(frames), ptr(table_dev), n, w, h, tau, cos_min, 1 if unique else 0,
                                      ptr(mask), ptr(xyz), ptr(nout), ptr(cout), ptr(support), stream_ptr()), "sfm_mvs_fuse")
    return dict(mask=mask, xyz=xyz, normals=nout, colors=cout, support=support)


_FUSE_KEYS = ("max_angle", "colours")


def _checked_fuse(fuse_opt):
    """run_mvs's `fuse` keyword as dict(max_angle, colours) (None: the filter), or an SfmHipError."""
    if fuse_opt is None or fuse_opt is False:
        return None
    if fuse_opt is True:
        fuse_opt = {}
    if not isinstance(fuse_opt, dict) or any(k not in _FUSE_KEYS for k in fuse_opt):
        raise SfmHipError(f"run_mvs: fuse must be None, True or a dict with keys among {_FUSE_KEYS}")
    opts = dict(max_angle=fuse_opt.get("max_angle", FUSE_MAX_ANGLE), colours=bool(fuse_opt.get("colours", True)))
    _cos_min(opts["max_angle"])
    return opts


_REFINE_KEYS = ("iters", "far", "depth_step", "slope_step", "seed")


def _checked_refine(refine):
    """run_mvs's `refine` keyword as the dict of patchmatch_refine's keywords (None: no refinement), or an SfmHipError."""
    if refine is None or refine is False:
        return None
    if refine is True:
        return {}
    if not isinstance(refine, dict) or any(k not in _REFINE_KEYS for k in refine):
        raise SfmHipError(f"run_mvs: refine must be None, True or a dict with keys among {_REFINE_KEYS}")
    return dict(refine)


def _checked_neighbours(nbrs, n):
    """run_mvs's `neighbours` keyword as a list of lists of ints, or an SfmHipError: one list per view, at most MAX_VIEWS entries, each
    an index in 0..n-1 other than the view's own."""
    if len(nbrs) != n:
        raise SfmHipError(f"run_mvs: neighbours holds {len(nbrs)} lists for {n} cameras")
    out = []
    for i, row in enumerate(nbrs):
        row = list(row)
        if len(row) > MAX_VIEWS:
            raise SfmHipError(f"run_mvs: view {i} names {len(row)} neighbours, more than MAX_VIEWS = {MAX_VIEWS}")
        for v in row:
            if isinstance(v, (bool, float, np.floating)) or int(v) != v or not 0 <= int(v) < n:
                raise SfmHipError(f"run_mvs: neighbour {v!r} of view {i} is not a view index in 0..{n - 1}")
            if int(v) == i:
                raise SfmHipError(f"run_mvs: view {i} names itself as a neighbour")
        out.append([int(v) for v in row])
    return out


def _checked_ranges(ranges, n, ndepth):
    """run_mvs's `ranges` keyword as the float32 [n, ndepth] plane inverse depths, or an SfmHipError: one finite 0 < dmin < dmax per view."""
    try:
        r = np.asarray(ranges, np.float64)
    except (TypeError, ValueError) as e:
        raise SfmHipError("run_mvs: ranges must hold one (dmin, dmax) per view") from e
    if r.shape != (n, 2):
        raise SfmHipError(f"run_mvs: ranges has shape {r.shape}, not ({n}, 2)")
    if not np.all(np.isfinite(r)) or not np.all((r[:, 0] > 0) & (r[:, 0] < r[:, 1])):
        raise SfmHipError("run_mvs: every range needs finite 0 < dmin < dmax")
    return np.stack([_inverse_depths_host(a, b, ndepth) for a, b in r])


def run_mvs(images, K, posearr, Xtot, ndepth=128, radius=3, nsrc=4, topk=2, var_min=VAR_MIN, cost_max=COST_MAX, tau=0.01,
            min_consistent=2, unique=True, aggregate=False, shift=None, p1=P1, p2=P2, ndir=8, neighbours=None, ranges=None, refine=None, fuse=None):
    """Dense reconstruction of a registered sequence: a plane-sweep depth map per view, geometric-consistency filtering, and one
    coloured cloud.

    images:  BGR uint8 frames at K's resolution (the halved frames sfm.py:40 works on), device tensors or host arrays, in the
             order of posearr's cameras
    posearr: sfm.py:423's layout, K (9) then one 3x4 P per camera (pipeline.run_sfm's "posearr"); Xtot the sparse cloud
    Per view: planes uniform in inverse depth over depth_range(Xtot, P_i), the `nsrc` sequence neighbours as sources (the same
    views check its consistency), a pixel kept when >= `min_consistent` neighbours see its depth within `tau` relative, once
    (unique: by its lowest-index consistent observer).
    Defaults (VAR_MIN, COST_MAX, ndepth 128, r 3, 4 sources, top 2, tau 1 %, 2 consistent neighbours): docs/mvs.md, "Calibration".
    aggregate: True replaces every view's winner-take-all depth map by aggregate_depth of the sweep's cost volume (shiftable
             windows of half-width `shift`, None = radius; semi-global penalties p1 / p2 over `ndir` directions): docs/mvs.md §7.
             The float volume, Q and S are allocated once and reused by every view (10 bytes per pixel and plane).
    neighbours: None, or per view the list of its source views (at most MAX_VIEWS, none the view itself) instead of the sequence
             neighbours, e.g. `mvs_plan.host_plan(...)["neighbours"]` for frames in any order (docs/mvs.md §8).  The length of a view's
             list caps topk and min_consistent for that view; a view with an empty list gets an all-zero depth map, no sweep, and
             contributes no point.
    ranges:  None, or per view (dmin, dmax) of its planes instead of depth_range(Xtot, P_i) (Xtot is then not read).
             Both are validated before any launch.
    refine:  None, True or a dict of patchmatch_refine's iters / far / depth_step / slope_step / seed: every view's depth map (the
             winner-take-all one, or the aggregated one) is refined over slanted planes before the consistency pass, with the view's
             own sources and plane range (docs/mvs.md §9).  The result gains "normal_maps" (per view (H, W, 3) float32 device tensor:
             unit world normals facing the camera, 0 where there is no depth) and "normals" (m, 3) float64, the points' normals.
    fuse:    None, True or a dict of max_angle (degrees, default FUSE_MAX_ANGLE; None: no bound) and colours (default True): the
             per-view consistency filter is replaced by one launch of the merging fusion (`fuse`, sfm_mvs_fuse; docs/mvs.md §10).  A
             kept pixel is emitted as the mean of its own sample and its consistent neighbours' samples: `points` the averaged
             positions, `colors` the averaged colours (colours=False: the pixel's own), with refine `normals` the normalised sum of
             the normals, and a neighbour whose normal is more than max_angle away from the pixel's is not consistent.  Without
             refine there are no normals: positions and colours only.  The result gains "support" (m,) uint8, the samples merged
             per point; `depths` / `normal_maps` are then views of one [n, H, W] / [n, H, W, 3] stack.
    Returns dict(depths [per view (H, W) float32 device tensor], points (m, 3) float64, colors (m, 3) float64 B G R): shaped as
    Xtot / colorstot, so that pipeline.to_ply(path, points, colors, densify=True) writes Point_Cloud/dense.ply.
    One host wait per call: the fused point count (then one download of the points and colours); every upload is stream-ordered
    (pinned memory)."""
    from . import ops
    from .sift import bgr2gray
    K = np.asarray(K, np.float64).reshape(3, 3)
    Ps = np.asarray(posearr, np.float64)[9:].reshape(-1, 3, 4)
    n = len(Ps)
    if len(images) != n:
        raise SfmHipError(f"run_mvs: {len(images)} frames for {n} cameras")
    if n < 2:
        raise SfmHipError("run_mvs: needs at least two registered views")
    nsrc = min(int(nsrc), n - 1, MAX_VIEWS)
    topk = min(int(topk), nsrc)
    nbrs = [_sequence_neighbours(i, n, nsrc) for i in range(n)] if neighbours is None else _checked_neighbours(neighbours, n)
    planes = None if ranges is None else _checked_ranges(ranges, n, ndepth)
    refine = _checked_refine(refine)
    fuse_opt = _checked_fuse(fuse)
    dev = torch.device("cuda", torch.cuda.current_device())
    if all(torch.is_tensor(im) and im.is_cuda for im in images):
        frames = [im.to(dev).contiguous() for im in images]
    else:                                                       # host frames: one pinned upload for all of them
        host = [im.cpu().numpy() if torch.is_tensor(im) else np.asarray(im) for im in images]
        if any(im.shape != host[0].shape or im.dtype != np.uint8 for im in host):
            raise SfmHipError("run_mvs: frames must be (H, W, 3) uint8 BGR of one size")
        frames = list(_upload(np.stack(host), dev))
    if any(f.dtype != torch.uint8 or f.dim() != 3 or f.shape[2] != 3 or f.shape != frames[0].shape for f in frames):
        raise SfmHipError("run_mvs: frames must be (H, W, 3) uint8 BGR of one size")
    h, w = frames[0].shape[:2]
    grays = [bgr2gray(f) for f in frames]
    # every view's planes in one upload, before the first launch (a per-view upload would wait for the previous view's sweep)
    if planes is None:
        planes = np.stack([_inverse_depths_host(*depth_range(Xtot, Ps[i], P_all=Ps), ndepth) for i in range(n)])
    invd = _upload(planes, dev)
    if fuse_opt is not None:                                    # the table too goes up before the first launch; the maps are stacked
        table_dev = _upload(fuse_table(K, Ps, nbrs, min_consistent).view(np.uint8).reshape(n, FUSE_RECORD.itemsize), dev)
        dstack = torch.empty((n, h, w), dtype=torch.float32, device=dev)
        nstack = torch.empty((n, h, w, 3), dtype=torch.float32, device=dev) if refine is not None else None
    depths, normal_maps = [], []
    if aggregate:
        vol = torch.empty((int(ndepth), h, w), dtype=torch.float32, device=dev)
        qbuf = torch.empty((int(ndepth), h, w), dtype=torch.uint16, device=dev)
        sbuf = torch.empty((int(ndepth), h, w), dtype=torch.uint16, device=dev)
    for i in range(n):
        if not nbrs[i]:                                         # no source: no sweep, an all-zero map
            depths.append(torch.zeros((h, w), dtype=torch.float32, device=dev) if fuse_opt is None else dstack[i].zero_())
            if refine is not None:
                normal_maps.append(torch.zeros((h, w, 3), dtype=torch.float32, device=dev) if fuse_opt is None else nstack[i].zero_())
            continue
        mv = sweep_matrices(K, Ps[i], Ps[nbrs[i]])
        if aggregate:
            plane_sweep(grays[i], [grays[v] for v in nbrs[i]], mv, invd[i], radius, min(topk, len(nbrs[i])), var_min, cost_max, volume_out=vol)
            d, _, _ = aggregate_depth(vol, invd[i], radius if shift is None else shift, p1, p2, ndir, cost_max, q_out=qbuf, s_out=sbuf)
        else:
            d, _, _, _ = plane_sweep(grays[i], [grays[v] for v in nbrs[i]], mv, invd[i], radius, min(topk, len(nbrs[i])), var_min, cost_max)
        if refine is not None:
            d, _, nm, _ = patchmatch_refine(grays[i], [grays[v] for v in nbrs[i]], mv, planes[i, 0], planes[i, -1], d, K, Ps[i], radius,
                                            min(topk, len(nbrs[i])), var_min, cost_max, **refine)
            normal_maps.append(nm if fuse_opt is None else nstack[i].copy_(nm))
        depths.append(d if fuse_opt is None else dstack[i].copy_(d))
    if fuse_opt is not None:
        return _fused_result(depths, normal_maps, dstack, nstack, torch.stack(frames), table_dev, tau, unique, fuse_opt)
    masks = torch.empty((n, h, w), dtype=torch.uint8, device=dev)
    xyz = torch.empty((n, h, w, 3), dtype=torch.float32, device=dev)
    for i in range(n):
        if not nbrs[i]:
            masks[i].zero_()
            continue
        ab, bc = consistency_matrices(K, Ps[i], Ps[nbrs[i]])
        consistency(depths[i], [depths[v] for v in nbrs[i]], nbrs[i], ab, i, bc, tau, min(int(min_consistent), len(nbrs[i])), unique,
                    mask_out=masks[i], xyz_out=xyz[i])
    idx = ops.mask_indices(masks).long()                       # the one host wait: the count sizes the result
    cols = [xyz.reshape(-1, 3)[idx].double(), torch.stack(frames).reshape(-1, 3)[idx].double()]
    if refine is not None:
        cols.append(torch.stack(normal_maps).reshape(-1, 3)[idx].double())
    both = torch.cat(cols, 1).cpu().numpy()
    out = dict(depths=depths, points=np.ascontiguousarray(both[:, :3]), colors=np.ascontiguousarray(both[:, 3:6]))
    if refine is not None:
        out.update(normal_maps=normal_maps, normals=np.ascontiguousarray(both[:, 6:]))
    return out


def _fused_result(depths, normal_maps, dstack, nstack, fstack, table_dev, tau, unique, fuse_opt):
    """run_mvs's result with fuse: the one launch over the stacked maps, the one host wait (the point count), one download."""
    from . import ops
    res = fuse(dstack, table_dev, nstack, fstack if fuse_opt["colours"] else None, tau, fuse_opt["max_angle"], unique)
    idx = ops.mask_indices(res["mask"]).long()                  # the one host wait: the count sizes the result
    cols = [res["xyz"].reshape(-1, 3)[idx].double(), (fstack if res["colors"] is None else res["colors"]).reshape(-1, 3)[idx].double(),
            res["support"].reshape(-1, 1)[idx].double()]
    if nstack is not None:
        cols.append(res["normals"].reshape(-1, 3)[idx].double())
    both = torch.cat(cols, 1).cpu().numpy()
    out = dict(depths=depths, points=np.ascontiguousarray(both[:, :3]), colors=np.ascontiguousarray(both[:, 3:6]),
               support=both[:, 6].astype(np.uint8))
    if nstack is not None:
        out.update(normal_maps=normal_maps, normals=np.ascontiguousarray(both[:, 7:]))
    return out
