"""Feature tracks from all-pairs matches and their N-view triangulation (include/sfm_hip.h, "TRACKS"; docs/tracks.md).

A node is `img_off[image] + keypoint`.  `match_edges` turns the device-resident match store of `sharded.match_pairs_sharded` into
graph edges, `track_components` labels the connected components, `build_tracks` keeps the components that name no image twice and
orders them, `triangulate_tracks` triangulates each from all its views.  All four take and return device tensors and never wait
for the host; `run_tracks` composes them, reads the counts once and downloads once, and returns the points and observations in the
form `ba.bundle_adjust_schur(cams, K, X, obs, cam_idx, pt_idx)` takes.  `refine_tracks` and `prune_tracks` ("TRACKS-REFINE";
docs/tracks.md §8) refine each point under a Huber loss, flag observations one by one and keep a track with its inliers only:
`run_tracks(robust=True)`.  `adjust_tracks` ("TRACKS-BA"; docs/tracks.md §9) bundle-adjusts what `run_tracks` returned and gives back
the camera matrices `run_tracks` takes.  `densify_tracks` ("MVS-PLAN"; docs/mvs.md §8) plans every view's sources and depth range from
the tracks and runs `mvs.run_mvs` with them: the frames may come in any order.  `guided_keep` ("GUIDED"; docs/tracks.md §14) matches
every pair again inside the epipolar band of its verified essential matrix and returns the store and mask `run_tracks` takes.
`retrieval_pairs` ("RETRIEVAL"; docs/retrieval.md) is the pair list of images without an order: every image with its k most similar."""
import numpy as np
import torch

from . import _lib
from ._lib import SfmHipError, check, on_device, ptr, require_cuda, stream_ptr
from .mvs import _upload

TRACK_ROUNDS = 6                # labelling rounds enqueued per call: twice the most any input of scripts/bench_tracks.py needed (docs/tracks.md §5)
INT32_MAX = 2 ** 31 - 1


def image_offsets(sizes, device):
    """int32 [n_img + 1] device tensor of the node offsets of images with `sizes` keypoints."""
    off = np.zeros(len(sizes) + 1, np.int64)
    np.cumsum(np.asarray(sizes, np.int64), out=off[1:])
    if off[-1] > INT32_MAX:
        raise SfmHipError(f"tracks: {int(off[-1])} nodes exceed 2^31-1")
    return _upload(off.astype(np.int32), device)


def _i32(t, what, shape=None):
    require_cuda(t)
    if t.dtype != torch.int32 or not t.is_contiguous() or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise SfmHipError(f"tracks: {what} must be a contiguous int32 device tensor" + (f" of shape {tuple(shape)}" if shape is not None else ""))
    return t


def _offsets(img_off):
    _i32(img_off, "img_off")
    if img_off.dim() != 1 or img_off.numel() < 2:
        raise SfmHipError("tracks: img_off must be int32 [n_img + 1] with n_img >= 1")
    return int(img_off.numel()) - 1


def match_edges(store, n_query, pairs, img_off, ratio=0.70, keep=None, out=None):
    """sfm_match_edges: the Lowe survivors of store (int32 [n_pairs, 2, cap, 2]) as edges int32 [n_pairs * cap, 2], (-1, -1) in every
    other slot.  n_query int32 [n_pairs] and pairs int32 [n_pairs, 2] are device tensors; keep: optional uint8 [n_pairs, cap], a
    query must be non-zero there.  No host wait."""
    require_cuda(store, keep)
    if store.dtype != torch.int32 or store.dim() != 4 or store.shape[1] != 2 or store.shape[3] != 2 or not store.is_contiguous():
        raise SfmHipError("match_edges: store must be a contiguous int32 [n_pairs, 2, cap, 2] device tensor")
    n_pairs, cap, dev = int(store.shape[0]), int(store.shape[2]), store.device
    n_img = _offsets(img_off)
    _i32(n_query, "n_query", (n_pairs,))
    _i32(pairs, "pairs", (n_pairs, 2))
    if keep is not None and (keep.dtype != torch.uint8 or tuple(keep.shape) != (n_pairs, cap) or not keep.is_contiguous()):
        raise SfmHipError("match_edges: keep must be a contiguous uint8 [n_pairs, cap] device tensor")
    edges = torch.empty((n_pairs * cap, 2), dtype=torch.int32, device=dev) if out is None else _i32(out, "edges", (n_pairs * cap, 2))
    ne = n_pairs * cap
    with on_device(dev):
        check(_lib.lib().sfm_match_edges(ptr(store) if ne else None, n_pairs, cap, ptr(pairs) if ne else None, ptr(n_query) if ne else None,
                                         ptr(img_off), n_img, float(ratio), ptr(keep) if ne else None, ptr(edges) if ne else None, stream_ptr()),
              "sfm_match_edges")
    return edges


def track_components(edges, n_nodes, rounds=TRACK_ROUNDS, labels=None, status=None):
    """sfm_track_components: label[u] = the smallest node id of u's component over the valid edges (both ends in 0..n_nodes-1 and
    different), at most `rounds` (1..1024) rounds.  labels: an int32 [n_nodes] tensor an earlier call left, to continue from (updated
    in place).  Returns (labels, status): status int32 [2] = (converged 0/1, rounds that lowered a label).  No host wait."""
    from .ops import _workspace
    require_cuda(edges)
    if edges.dtype != torch.int32 or edges.dim() != 2 or edges.shape[1] != 2 or not edges.is_contiguous():
        raise SfmHipError("track_components: edges must be a contiguous [k, 2] int32 device tensor")
    n, ne, dev = int(n_nodes), int(edges.shape[0]), edges.device
    resume = labels is not None
    if resume:
        _i32(labels, "labels", (n,))
    else:
        labels = torch.empty(max(n, 0), dtype=torch.int32, device=dev)
    status = torch.empty(2, dtype=torch.int32, device=dev) if status is None else _i32(status, "status", (2,))
    L = _lib.lib()
    ws = _workspace(dev, L.sfm_track_components_ws_bytes(max(n, 0), ne))
    with on_device(dev):
        check(L.sfm_track_components(ptr(edges) if ne else None, n, ne, int(rounds), int(resume), ptr(labels) if n > 0 else None, ptr(status),
                                     ptr(ws), ws.numel(), stream_ptr()), "sfm_track_components")
    return labels, status


def build_tracks(labels, img_off, min_len=2, max_len=None, counts=None):
    """sfm_track_build on converged labels: a component of >= 2 nodes is kept iff no two of its nodes lie in one image and
    min_len <= size <= max_len.  Returns (node_track [N], track_off [N // 2 + 2], obs_node [N], counts [6]) int32 device tensors;
    counts = (tracks T, observations, candidates, conflicting, longest kept, nodes in components of one node); T + 1 words of
    track_off and counts[1] of obs_node are written, nothing past them.  No host wait."""
    n_img = _offsets(img_off)
    _i32(labels, "labels")
    if labels.dim() != 1:
        raise SfmHipError("build_tracks: labels must be int32 [N]")
    n, dev = int(labels.numel()), labels.device
    node_track = torch.empty(n, dtype=torch.int32, device=dev)
    track_off = torch.empty(n // 2 + 2, dtype=torch.int32, device=dev)
    obs_node = torch.empty(n, dtype=torch.int32, device=dev)
    counts = torch.empty(6, dtype=torch.int32, device=dev) if counts is None else _i32(counts, "counts", (6,))
    build_tracks_into(labels, img_off, n_img, min_len, max_len, node_track, track_off, obs_node, counts)
    return node_track, track_off, obs_node, counts


def build_tracks_into(labels, img_off, n_img, min_len, max_len, node_track, track_off, obs_node, counts):
    """build_tracks into buffers of the caller (the tests fill them with sentinels first)."""
    from .ops import _workspace
    n, dev = int(labels.numel()), labels.device
    L = _lib.lib()
    ws = _workspace(dev, L.sfm_track_build_ws_bytes(n))
    with on_device(dev):
        check(L.sfm_track_build(ptr(labels) if n else None, ptr(img_off), n, n_img, int(min_len), INT32_MAX if max_len is None else int(max_len),
                                ptr(node_track) if n else None, ptr(track_off), ptr(obs_node) if n else None, ptr(counts), ptr(ws),
                                ws.numel(), stream_ptr()), "sfm_track_build")


def triangulate_tracks(counts, track_off, obs_node, img_off, keypoints, P, out=None):
    """sfm_track_triangulate: one lane per track, the counts read on the device.  keypoints float32 [N, 2] (all images concatenated),
    P float64 [n_img, 12] or [n_img, 3, 4]: device tensors.  Returns (X [N // 2 + 1, 3] f32, err [N] f32, depth [N] f32,
    flags [N // 2 + 1] i32, max_err [N // 2 + 1] f32), of which the first counts[0] / counts[1] rows are written.  No host wait."""
    n_img = _offsets(img_off)
    require_cuda(keypoints, P)
    _i32(counts, "counts")
    _i32(track_off, "track_off")
    _i32(obs_node, "obs_node")
    n, dev = int(obs_node.numel()), obs_node.device
    if keypoints.dtype != torch.float32 or tuple(keypoints.shape) != (n, 2) or not keypoints.is_contiguous():
        raise SfmHipError("triangulate_tracks: keypoints must be a contiguous float32 [N, 2] device tensor")
    if P.dtype != torch.float64 or P.numel() != 12 * n_img or not P.is_contiguous():
        raise SfmHipError("triangulate_tracks: P must be a contiguous float64 [n_img, 12] device tensor")
    if counts.numel() < 2 or track_off.numel() < n // 2 + 2:
        raise SfmHipError("triangulate_tracks: counts must hold (tracks, observations) and track_off N // 2 + 2 words")
    cap = n // 2 + 1
    if out is None:
        out = (torch.empty((cap, 3), dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev),
               torch.empty(n, dtype=torch.float32, device=dev), torch.empty(cap, dtype=torch.int32, device=dev),
               torch.empty(cap, dtype=torch.float32, device=dev))
    X, err, depth, flags, max_err = out
    with on_device(dev):
        check(_lib.lib().sfm_track_triangulate(ptr(counts), ptr(track_off), ptr(obs_node) if n else None, ptr(img_off), n_img,
                                               ptr(keypoints) if n else None, ptr(P), n, ptr(X), ptr(err) if n else None,
                                               ptr(depth) if n else None, ptr(flags), ptr(max_err), stream_ptr()), "sfm_track_triangulate")
    return X, err, depth, flags, max_err


def _track_inputs(who, counts, track_off, obs_node, img_off, keypoints, P):
    n_img = _offsets(img_off)
    require_cuda(keypoints, P)
    _i32(counts, "counts")
    _i32(track_off, "track_off")
    _i32(obs_node, "obs_node")
    n = int(obs_node.numel())
    if keypoints.dtype != torch.float32 or tuple(keypoints.shape) != (n, 2) or not keypoints.is_contiguous():
        raise SfmHipError(f"{who}: keypoints must be a contiguous float32 [N, 2] device tensor")
    if P.dtype != torch.float64 or P.numel() != 12 * n_img or not P.is_contiguous():
        raise SfmHipError(f"{who}: P must be a contiguous float64 [n_img, 12] device tensor")
    if counts.numel() < 2 or track_off.numel() < n // 2 + 2:
        raise SfmHipError(f"{who}: counts must hold (tracks, observations) and track_off N // 2 + 2 words")
    return n_img, n


def _typed(t, dtype, shape, what):
    require_cuda(t)
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise SfmHipError(f"tracks: {what} must be a contiguous {dtype} device tensor of shape {tuple(shape)}")
    return t


def refine_tracks(counts, track_off, obs_node, img_off, keypoints, P, X, flags, huber=1.0, obs_thresh=2.0, iters=10, iters2=5, out=None):
    """sfm_track_refine: one lane per track, the counts read on the device.  X [N // 2 + 1, 3] f32 and flags [N // 2 + 1] i32 are
    `triangulate_tracks`' outputs; huber (px, > 0, inf = plain least squares) is the Huber width of phase 1, obs_thresh (px) the
    inlier bound, iters / iters2 (0..50) the Levenberg-Marquardt attempts of the two phases.  Returns (X_out [N // 2 + 1, 3] f32,
    inlier [N] u8, err [N] f32, depth [N] f32, n_inl [N // 2 + 1] i32, max_err f32, cos_min f32, steps i32, flags i32), of which the
    first counts[0] / counts[1] rows are written.  No host wait."""
    from .ops import _workspace
    n_img, n = _track_inputs("refine_tracks", counts, track_off, obs_node, img_off, keypoints, P)
    dev, cap = obs_node.device, n // 2 + 1
    _typed(X, torch.float32, (cap, 3), "X")
    _typed(flags, torch.int32, (cap,), "flags")
    if out is None:
        f32, i32 = torch.float32, torch.int32
        out = (torch.empty((cap, 3), dtype=f32, device=dev), torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=f32, device=dev),
               torch.empty(n, dtype=f32, device=dev), torch.empty(cap, dtype=i32, device=dev), torch.empty(cap, dtype=f32, device=dev),
               torch.empty(cap, dtype=f32, device=dev), torch.empty(cap, dtype=i32, device=dev), torch.empty(cap, dtype=i32, device=dev))
    X_out, inlier, err, depth, n_inl, max_err, cos_min, steps, flags_out = out
    L = _lib.lib()
    ws = _workspace(dev, L.sfm_track_refine_ws_bytes(n_img))
    with on_device(dev):
        check(L.sfm_track_refine(ptr(counts), ptr(track_off), ptr(obs_node) if n else None, ptr(img_off), n_img, ptr(keypoints) if n else None,
                                 ptr(P), n, ptr(X), ptr(flags), float(huber), float(obs_thresh), int(iters), int(iters2), ptr(X_out),
                                 ptr(inlier) if n else None, ptr(err) if n else None, ptr(depth) if n else None, ptr(n_inl), ptr(max_err),
                                 ptr(cos_min), ptr(steps), ptr(flags_out), ptr(ws), ws.numel(), stream_ptr()), "sfm_track_refine")
    return X_out, inlier, err, depth, n_inl, max_err, cos_min, steps, flags_out


def max_cos_of(min_angle_deg):
    """The cosine `sfm_track_prune` compares with: a track passes when two of its inlier rays open at least `min_angle_deg` degrees
    (None or 0: every track passes)."""
    return 1.0 if min_angle_deg is None or min_angle_deg <= 0 else float(np.cos(np.deg2rad(float(min_angle_deg))))


def prune_tracks(counts, track_off, obs_node, X, inlier, n_inl, max_err, cos_min, flags, min_len=2, max_reproj=None, min_angle_deg=None,
                 max_cos=None, out=None):
    """sfm_track_prune on `refine_tracks`' outputs: keeps the tracks with flags == 3, n_inl >= min_len, max_err <= max_reproj (None:
    no bound) and two inlier rays at least min_angle_deg apart (None: no bound; max_cos overrides the cosine the angle turns into),
    and of those the inlier observations.  Returns (track_off2 [N // 2 + 2] i32, obs_node2 [N] i32, X2 [N // 2 + 1, 3] f32,
    track_src [N // 2 + 1] i32, counts2 [4] i32 = (tracks, observations, tracks dropped, observations dropped from kept tracks)); the
    first three with counts2 have the shape `build_tracks` leaves.  No host wait."""
    from .ops import _workspace
    _i32(counts, "counts")
    _i32(track_off, "track_off")
    _i32(obs_node, "obs_node")
    n, dev = int(obs_node.numel()), obs_node.device
    cap = n // 2 + 1
    if counts.numel() < 2 or track_off.numel() < n // 2 + 2:
        raise SfmHipError("prune_tracks: counts must hold (tracks, observations) and track_off N // 2 + 2 words")
    _typed(X, torch.float32, (cap, 3), "X")
    _typed(inlier, torch.uint8, (n,), "inlier")
    _typed(n_inl, torch.int32, (cap,), "n_inl")
    _typed(max_err, torch.float32, (cap,), "max_err")
    _typed(cos_min, torch.float32, (cap,), "cos_min")
    _typed(flags, torch.int32, (cap,), "flags")
    if out is None:
        out = (torch.empty(n // 2 + 2, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
               torch.empty((cap, 3), dtype=torch.float32, device=dev), torch.empty(cap, dtype=torch.int32, device=dev),
               torch.empty(4, dtype=torch.int32, device=dev))
    track_off2, obs_node2, X2, track_src, counts2 = out
    L = _lib.lib()
    ws = _workspace(dev, L.sfm_track_prune_ws_bytes(n))
    with on_device(dev):
        check(L.sfm_track_prune(ptr(counts), ptr(track_off), ptr(obs_node) if n else None, n, ptr(X), ptr(inlier) if n else None, ptr(n_inl),
                                ptr(max_err), ptr(cos_min), ptr(flags), int(min_len), float("inf") if max_reproj is None else float(max_reproj),
                                max_cos_of(min_angle_deg) if max_cos is None else float(max_cos), ptr(track_off2), ptr(obs_node2) if n else None,
                                ptr(X2), ptr(track_src), ptr(counts2), ptr(ws), ws.numel(), stream_ptr()), "sfm_track_prune")
    return track_off2, obs_node2, X2, track_src, counts2


def _scene_tensors(n_query, pairs, keypoints, P, dev):
    sizes = [int(k.shape[0]) for k in keypoints]
    img_off = image_offsets(sizes, dev)
    kp = torch.cat([k.to(device=dev, dtype=torch.float32).reshape(-1, 2) for k in keypoints]).contiguous() if sizes else torch.empty((0, 2), device=dev)
    nq = _upload(np.asarray(n_query, np.int32).reshape(-1), dev)
    pr = _upload(np.asarray(pairs, np.int32).reshape(-1, 2), dev)
    Pd = None if P is None else _upload(np.asarray(P, np.float64).reshape(len(sizes), 12), dev)
    return img_off, kp, nq, pr, Pd, int(sum(sizes))


def run_tracks(store, n_query, pairs, keypoints, P, ratio=0.70, keep=None, min_len=2, max_len=None, max_reproj=None, rounds=TRACK_ROUNDS,
               robust=False, huber=1.0, obs_thresh=2.0, min_angle_deg=None, refine_iters=10):
    """Match store -> tracks -> N-view points.  store, n_query, pairs as `sharded.match_pairs_sharded` returns and takes them;
    keypoints: list over images of [n_i, 2] float32 device tensors; P: [n_img, 3, 4] float64 (host).  Keeps the tracks whose
    triangulation has flags == 3 (every depth positive, a finite point) and, if max_reproj is given, a largest reprojection error
    <= max_reproj.  Returns host arrays: points (T', 3) f32, obs (nobs', 2) f32, cam_idx, pt_idx (nobs',) i32, track_len (T',) i32,
    counts (6,) as sfm_track_build writes them, status (2,) of the labelling.  Two host waits: the counts (with the status) and one
    download; each batch of `rounds` rounds the labelling still needs after the first costs one more read of the status.
    robust=True: every point is refined by `refine_tracks(huber, obs_thresh, iters=refine_iters)` and `prune_tracks(min_len, max_reproj,
    min_angle_deg)` keeps a track with its inlier observations only instead of dropping it whole; the same keys come back from the
    pruned set, with `obs_dropped` and `tracks_dropped`; still two host waits (the first also reads the pruned counts)."""
    dev = store.device
    store = store.contiguous()
    img_off, kp, nq, pr, Pd, n = _scene_tensors(n_query, pairs, keypoints, P, dev)
    edges = match_edges(store, nq, pr, img_off, ratio, keep)
    head = torch.empty(12 if robust else 8, dtype=torch.int32, device=dev)
    counts, status = head[:6], head[6:8]
    labels, lowered = None, 0
    while True:
        labels, _ = track_components(edges, n, rounds, labels, status)
        node_track, track_off, obs_node, _ = build_tracks(labels, img_off, min_len, max_len, counts)
        X, err, depth, flags, max_err = triangulate_tracks(counts, track_off, obs_node, img_off, kp, Pd)
        if robust:
            refined = refine_tracks(counts, track_off, obs_node, img_off, kp, Pd, X, flags, huber, obs_thresh, refine_iters)
            pruned = prune_tracks(counts, track_off, obs_node, refined[0], refined[1], refined[4], refined[5], refined[6], refined[8], min_len,
                                  max_reproj, min_angle_deg, out=(torch.empty(n // 2 + 2, dtype=torch.int32, device=dev),
                                                                  torch.empty(n, dtype=torch.int32, device=dev),
                                                                  torch.empty((n // 2 + 1, 3), dtype=torch.float32, device=dev),
                                                                  torch.empty(n // 2 + 1, dtype=torch.int32, device=dev), head[8:]))
        host_head = head.cpu().numpy()                                # host wait 1: the counts and the status (and the pruned counts)
        lowered += int(host_head[7])
        if host_head[6]:
            break
    if robust:
        return _robust_result(host_head, lowered, pruned, img_off, kp)
    T, nobs = int(host_head[0]), int(host_head[1])
    nodes = obs_node[:nobs].long()
    cam = (torch.searchsorted(img_off[:-1].contiguous(), obs_node[:nobs], right=True) - 1).to(torch.int32)
    words = torch.cat([X[:T].reshape(-1).view(torch.int32), flags[:T], max_err[:T].view(torch.int32), track_off[:T + 1], cam,
                       kp.index_select(0, nodes).reshape(-1).view(torch.int32)])
    host = words.cpu().numpy()                                        # host wait 2: the one download
    pos = np.cumsum([0, 3 * T, T, T, T + 1, nobs])
    Xh = host[pos[0]:pos[1]].view(np.float32).reshape(T, 3)
    fl, worst = host[pos[1]:pos[2]], host[pos[2]:pos[3]].view(np.float32)
    off, camh = host[pos[3]:pos[4]].astype(np.int64), host[pos[4]:pos[5]]
    obs = host[pos[5]:].view(np.float32).reshape(nobs, 2)
    good = fl == 3
    if max_reproj is not None:
        with np.errstate(invalid="ignore"):
            good &= worst <= np.float32(max_reproj)
    length = np.diff(off)
    track = np.repeat(np.arange(T), length)
    sel = good[track]
    new_id = np.cumsum(good) - 1
    return dict(points=np.ascontiguousarray(Xh[good]), obs=np.ascontiguousarray(obs[sel]), cam_idx=np.ascontiguousarray(camh[sel]),
                pt_idx=new_id[track[sel]].astype(np.int32), track_len=length[good].astype(np.int32), counts=host_head[:6].copy(),
                status=np.array([int(host_head[6]), lowered], np.int32))


def _robust_result(host_head, lowered, pruned, img_off, kp):
    """The one download of run_tracks(robust=True): every pruned track is returned, with its inlier observations."""
    track_off2, obs_node2, X2, _, _ = pruned
    T, nobs = int(host_head[8]), int(host_head[9])
    nodes = obs_node2[:nobs].long()
    cam = (torch.searchsorted(img_off[:-1].contiguous(), obs_node2[:nobs], right=True) - 1).to(torch.int32)
    words = torch.cat([X2[:T].reshape(-1).view(torch.int32), track_off2[:T + 1], cam, kp.index_select(0, nodes).reshape(-1).view(torch.int32)])
    host = words.cpu().numpy()                                        # host wait 2: the one download
    pos = np.cumsum([0, 3 * T, T + 1, nobs])
    length = np.diff(host[pos[1]:pos[2]].astype(np.int64))
    return dict(points=np.ascontiguousarray(host[pos[0]:pos[1]].view(np.float32).reshape(T, 3)),
                obs=np.ascontiguousarray(host[pos[3]:].view(np.float32).reshape(nobs, 2)), cam_idx=np.ascontiguousarray(host[pos[2]:pos[3]]),
                pt_idx=np.repeat(np.arange(T), length).astype(np.int32), track_len=length.astype(np.int32), counts=host_head[:6].copy(),
                status=np.array([int(host_head[6]), lowered], np.int32), tracks_dropped=int(host_head[10]), obs_dropped=int(host_head[11]))


def adjust_tracks(result, P, K, device=None, calibrate=None, **kw):
    """Bundle adjustment of the tracks `run_tracks` returned (either variant) from the cameras P [n_img, 3, 4] it was given, K 3 x 3:
    `track_ba.bundle_adjust_tracks(cams_from_P(P, K), K, points, obs, cam_idx, pt_idx, **kw)` (huber, iters, lam, fix_first_camera,
    cg_tol, cg_iters, log).  Returns (P' [n_img, 3, 4] float64, points' [T, 3] float64, info) on the host; info holds the history of
    robust costs and the counts of the last sweep.  `run_tracks(..., P')` then runs on the adjusted cameras.
    calibrate: None, or dict(free=("f", "k1"), dist=None): `track_cal.bundle_adjust_calibrated` instead (docs/tracks.md §15), the
    intrinsics named in `free` among the unknowns, from K and dist = (k1, k2).  P' is then built with K', and info gains "K"
    (3 x 3) and "dist" (k1, k2): the keypoints are pixels of the DISTORTED camera, `track_cal.undistort_points` maps them to the
    pinhole camera K' that P' describes."""
    from . import track_ba
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    cams0 = track_ba.cams_from_P(P, K)
    if calibrate is not None:
        from . import track_cal
        unknown = sorted(set(calibrate) - {"free", "dist"})
        if unknown:
            raise SfmHipError(f"adjust_tracks: calibrate takes free and dist, not {unknown}")
        cams, X, K_new, dist, hist, info = track_cal.bundle_adjust_calibrated(
            _upload(cams0, dev), K, calibrate.get("dist"), _upload(np.asarray(result["points"], np.float64).reshape(-1, 3), dev),
            _upload(np.asarray(result["obs"], np.float32).reshape(-1, 2), dev), _upload(np.asarray(result["cam_idx"], np.int32), dev),
            _upload(np.asarray(result["pt_idx"], np.int32), dev), free=calibrate.get("free", ("f", "k1")), **kw)
        host = torch.cat([cams.reshape(-1), X.reshape(-1)]).cpu().numpy()
        info = dict(info, history=hist, K=K_new, dist=dist)
        return track_ba.P_from_cams(host[:cams.numel()].reshape(-1, 6), K_new), host[cams.numel():].reshape(-1, 3).copy(), info
    cams, X, hist, info = track_ba.bundle_adjust_tracks(_upload(cams0, dev), K, _upload(np.asarray(result["points"], np.float64).reshape(-1, 3), dev),
                                                        _upload(np.asarray(result["obs"], np.float32).reshape(-1, 2), dev),
                                                        _upload(np.asarray(result["cam_idx"], np.int32), dev),
                                                        _upload(np.asarray(result["pt_idx"], np.int32), dev), **kw)
    host = torch.cat([cams.reshape(-1), X.reshape(-1)]).cpu().numpy()
    info = dict(info, history=hist)
    return track_ba.P_from_cams(host[:cams.numel()].reshape(-1, 6), K), host[cams.numel():].reshape(-1, 3).copy(), info


def densify_tracks(result, images, K, P, points=None, nsrc=4, min_angle_deg=None, max_angle_deg=None, min_good=None, lo=2, hi=98, device=None, dist=None,
                   **kw):
    """Dense reconstruction of the views of a `run_tracks` result (either variant): `track_ba.plan` -> `mvs_plan.plan_views` ->
    `mvs_plan.host_plan` -> `mvs.run_mvs(images, K, posearr, points, neighbours=..., ranges=..., **kw)`.  P [n_img, 3, 4] float64 and
    `points` (default result["points"]; pass the float64 points `adjust_tracks` returned with its P') are the cameras and the cloud the
    plan is made from; the angle window and min_good default to mvs_plan's.  Returns run_mvs's dict plus "plan" (host_plan's dict).
    Host waits: host_plan's one, then run_mvs's.
    dist: None, or (k1, k2) of the camera that took `images` (`adjust_tracks(calibrate=...)` returns it with K' in info): the frames
    are undistorted on the device with the K given here (`track_cal.undistort_images`, one batched call when they share a size)
    before `run_mvs` sees them; pixels whose source lies outside the frame are black.  P stays as it is."""
    from . import mvs, mvs_plan, track_ba
    if dist is not None:
        images = _undistorted(images, K, dist, torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device))
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    K = np.asarray(K, np.float64).reshape(3, 3)
    P = np.ascontiguousarray(np.asarray(P, np.float64).reshape(-1, 3, 4))
    X = np.ascontiguousarray(np.asarray(result["points"] if points is None else points, np.float64).reshape(-1, 3))
    pl = track_ba.plan(_upload(np.asarray(result["cam_idx"], np.int32), dev), _upload(np.asarray(result["pt_idx"], np.int32), dev), len(P), len(X))
    planned = mvs_plan.plan_views(pl, _upload(X, dev), _upload(P, dev), nsrc,
                                  mvs_plan.MIN_ANGLE_DEG if min_angle_deg is None else min_angle_deg,
                                  mvs_plan.MAX_ANGLE_DEG if max_angle_deg is None else max_angle_deg,
                                  mvs_plan.MIN_GOOD if min_good is None else min_good, lo, hi)
    hp = mvs_plan.host_plan(planned)
    posearr = np.concatenate([K.ravel(), P.ravel()])
    out = mvs.run_mvs(images, K, posearr, X, nsrc=nsrc, neighbours=hp["neighbours"], ranges=hp["ranges"], **kw)
    out["plan"] = hp
    return out


def _undistorted(images, K, dist, dev):
    """The frames as device tensors, undistorted: one batched call when they share a shape, else one call per frame; no host wait."""
    from . import track_cal
    frames = [(im if torch.is_tensor(im) else torch.from_numpy(np.ascontiguousarray(im))).to(dev).contiguous() for im in images]
    if not frames:
        return frames
    if all(f.shape == frames[0].shape for f in frames):
        stack = torch.stack(frames).contiguous()
        if stack.dim() == 3:                                            # gray frames [n, H, W]
            return list(track_cal.undistort_images(stack.unsqueeze(-1).contiguous(), K, dist).squeeze(-1))
        return list(track_cal.undistort_images(stack, K, dist))
    return [track_cal.undistort_images(f if f.dim() == 3 else f.unsqueeze(-1).contiguous(), K, dist).reshape(f.shape) for f in frames]


def verify_keep(store, n_query, pairs, keypoints, K, ratio=0.70, batched=False, **kw):
    """The per-query inlier masks of `sharded.HipVerifyEngine`'s two stages (isfm.py:73-94: essential-matrix RANSAC on the Lowe
    survivors, then the cheirality vote of recoverPose on its inliers) as the `keep` tensor of `match_edges`: uint8 [n_pairs, cap],
    1 at the queries that survive both.  A pair with fewer than five survivors or without an essential matrix keeps nothing.
    Waits for the host as the engine does (per pair).
    batched=True: `verify.verify_pairs(...)["keep"]` instead (docs/tracks.md §11): all pairs in a fixed number of launches and no host wait, a fixed
    budget of hypotheses per pair; **kw (threshold, budget, seed) goes to it.  The masks of the two paths differ."""
    if batched:
        from . import verify
        dev = store.device
        to_dev = lambda v, shape: (v.to(device=dev, dtype=torch.int32) if isinstance(v, torch.Tensor) else _upload(np.asarray(v, np.int32), dev)).reshape(shape).contiguous()
        sizes = [int(k.shape[0]) for k in keypoints]
        kp = torch.cat([k.to(device=dev, dtype=torch.float32).reshape(-1, 2) for k in keypoints]).contiguous()
        return verify.verify_pairs(store.contiguous(), to_dev(n_query, (-1,)), to_dev(pairs, (-1, 2)), image_offsets(sizes, dev), kp, K, ratio, **kw)["keep"]
    if kw:
        raise TypeError(f"verify_keep: {sorted(kw)} apply to batched=True only")
    from . import ops, ransac
    dev = store.device
    n_pairs, cap = int(store.shape[0]), int(store.shape[2])
    keep = torch.zeros((n_pairs, cap), dtype=torch.uint8, device=dev)
    for p, (i, j) in enumerate(pairs):
        nq = int(n_query[p])
        block = store[p]
        out_q, out_t, count = ops.ratio_compact(block[0, :nq], block[1, :nq].view(torch.float32), ratio)
        pts0, pts1 = ops.gather_matches(keypoints[i], keypoints[j], out_q, out_t, count)
        m = int(count.item())
        if m < 5:
            continue
        pts0, pts1 = pts0[:m], pts1[:m]
        E, mask = ransac.find_essential_mat(pts0, pts1, K, 0.999, 0.4, return_device_mask=True)
        if E is None:
            continue
        first = ops.mask_indices(mask).long()
        _, _, _, mask2 = ransac.recover_pose(E[:3], pts0[first], pts1[first], K, return_device_mask=True)
        second = ops.mask_indices(mask2, nonzero=True).long()
        keep[p].index_fill_(0, out_q[:m].long()[first[second]], 1)
    return keep


def guided_keep(descriptors, store, n_query, pairs, keypoints, K, ratio=0.70, guided_threshold=None, min_inliers=None, mutual=True,
                max_rev_bytes=None, **kw):
    """Guided matching as one call (docs/tracks.md §14): `verify.verify_pairs` on the global store, `guided.guided_pairs` under the
    essential matrices it left, `verify.verify_pairs` again on the guided store.  descriptors: list over images of [n_i, 128] float32
    device tensors; store, n_query, pairs, keypoints, K, ratio as `verify_keep` takes them; guided_threshold (pixels), min_inliers,
    mutual, max_rev_bytes go to `guided_pairs` (None: its defaults); **kw (threshold, budget, seed, lo) to both verifications.
    Returns (store_g int32 [n_pairs, 2, cap, 2], keep uint8 [n_pairs, cap]): keep is the second verification's mask, and the mutual
    mask as well when `mutual`; both go to `match_edges` / `run_tracks(store_g, ..., keep=keep)` as they are.  No host wait."""
    from . import guided, verify
    if len(descriptors) != len(keypoints):
        raise SfmHipError(f"guided_keep: {len(descriptors)} descriptor sets for {len(keypoints)} images")
    require_cuda(store, *descriptors)
    dev = store.device
    to_dev = lambda v, shape: (v.to(device=dev, dtype=torch.int32) if isinstance(v, torch.Tensor) else _upload(np.asarray(v, np.int32), dev)).reshape(shape).contiguous()
    sizes = [int(k.shape[0]) for k in keypoints]
    if [int(d.shape[0]) for d in descriptors] != sizes or any(d.dim() != 2 or d.shape[1] != 128 for d in descriptors):
        raise SfmHipError("guided_keep: descriptors must be [n_i, 128] with the n_i of the keypoints")
    kp = torch.cat([k.to(device=dev, dtype=torch.float32).reshape(-1, 2) for k in keypoints]).contiguous()
    desc = torch.cat([d.to(device=dev, dtype=torch.float32) for d in descriptors]).contiguous()
    store, nq, pr, img_off = store.contiguous(), to_dev(n_query, (-1,)), to_dev(pairs, (-1, 2)), image_offsets(sizes, dev)
    first = verify.verify_pairs(store, nq, pr, img_off, kp, K, ratio, **kw)
    opts = {k: v for k, v in dict(threshold=guided_threshold, min_inliers=min_inliers, max_rev_bytes=max_rev_bytes).items() if v is not None}
    g = guided.guided_pairs(desc, nq, pr, img_off, kp, K, first["E"], first["info"], mutual=mutual, cap=int(store.shape[2]),
                            max_size=max(sizes) if sizes else 0, **opts)
    keep = verify.verify_pairs(g["store"], nq, pr, img_off, kp, K, ratio, **kw)["keep"]
    return g["store"], (keep & g["keep"] if mutual else keep)


def retrieval_pairs(descriptors, k=8, **kw):
    """The shortlist of pairs for images without an order (docs/retrieval.md): `retrieval.select_pairs` on the list over images of
    [n_i, 128] float32 device tensors `guided_keep` takes; **kw (centres, n_centres, iters, seed, ssr, mutual, min_sim, value_range)
    goes to it.  Returns the host list of (i, j), i < j, ascending: the `pairs` of `sharded.match_pairs_sharded(descriptors, pairs)`
    and of everything after it.  One host wait."""
    from . import retrieval
    return retrieval.select_pairs(descriptors, None, k, **kw)[0]
