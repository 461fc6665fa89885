"""Track-driven incremental registration of unordered images (include/sfm_hip.h, "TRACKS-REGISTER"; csrc/tracks_register.hip;
docs/tracks.md §10).

`restrict_tracks`, `adopt_points`, `view_scores` and `correspondences` are thin wrappers: device tensors in and out, an `out=`, no host
wait.  `register_tracks` is the loop: tracks once, a seed pair by essential-matrix RANSAC and recoverPose, then model rounds (restrict ->
triangulate -> refine -> prune -> adopt -> scores, one host read each), the next view by PnP on its correspondences, and the track
bundle adjustment every few registrations.  The loop is written against a small engine (`_HipEngine` here; the tests run the same loop
on the NumPy restatements and the oracle), so every decision it takes is a function of what the engine returns."""
import numpy as np
import torch

from . import _lib
from ._lib import SfmHipError, check, on_device, ptr, stream_ptr
from .mvs import _upload
from .tracks import (TRACK_ROUNDS, _i32, _offsets, _scene_tensors, _typed, build_tracks, match_edges, prune_tracks, refine_tracks,
                     track_components, triangulate_tracks)

LDS_IMAGES = 256                # SFM_REGISTER_LDS_IMAGES: above it view_scores takes the global-atomic path
MAX_IMAGES = 4096               # register_tracks: the seed order comes from sfm_view_pair_counts, which takes no more cameras
E_PROB, E_THRESHOLD = 0.999, 0.4   # the essential-matrix RANSAC of tracks.verify_keep
# Defaults of register_tracks, calibrated with the CPU twin of the loop (tests/register_cases.py) on the scenes of docs/tracks.md §10.4
CONFIG_GENERAL, CONFIG_PLANAR = 1, 2          # verify.CONFIG_GENERAL, verify.CONFIG_PLANAR
MIN_CORR = 30                   # 2D-3D correspondences an image needs to be tried, and PnP inliers it needs to register
MIN_SEED = 100                  # points the seed pair's model round has to leave
BA_EVERY = 4                    # registrations between two bundle adjustments
BA_ITERS = 15
PNP_DEFAULTS = dict(iterations_count=100, reprojection_error=8.0, confidence=0.99)


def _u8(t, shape, what):
    return _typed(t, torch.uint8, shape, what)


def restrict_tracks(counts, track_off, obs_node, img_off, registered, min_len=2, out=None):
    """sfm_track_restrict: the tracks with at least min_len observations in images whose `registered` (uint8 [n_img]) is non-zero, with
    those observations only.  Returns (track_off2 [N // 2 + 2] i32, obs_node2 [N] i32, track_src [N // 2 + 1] i32, counts2 [4] i32 =
    (tracks, observations, tracks with 1..min_len-1 live observations, observations dropped from kept tracks)): the shape
    `build_tracks` leaves.  No host wait."""
    from .ops import _workspace
    n_img = _offsets(img_off)
    _i32(counts, "counts")
    _i32(track_off, "track_off")
    _i32(obs_node, "obs_node")
    n, dev = int(obs_node.numel()), obs_node.device
    if counts.numel() < 2 or track_off.numel() < n // 2 + 2:
        raise SfmHipError("restrict_tracks: counts must hold (tracks, observations) and track_off N // 2 + 2 words")
    _u8(registered, (n_img,), "registered")
    if out is None:
        out = (torch.empty(n // 2 + 2, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
               torch.empty(n // 2 + 1, dtype=torch.int32, device=dev), torch.empty(4, dtype=torch.int32, device=dev))
    track_off2, obs_node2, track_src, counts2 = out
    _i32(track_off2, "track_off2", (n // 2 + 2,))
    _i32(obs_node2, "obs_node2", (n,))
    _i32(track_src, "track_src", (n // 2 + 1,))
    _i32(counts2, "counts2", (4,))
    L = _lib.lib()
    ws = _workspace(dev, L.sfm_track_restrict_ws_bytes(n))
    with on_device(dev):
        check(L.sfm_track_restrict(ptr(counts), ptr(track_off), ptr(obs_node) if n else None, ptr(img_off), n_img, n, ptr(registered), int(min_len),
                                   ptr(track_off2), ptr(obs_node2) if n else None, ptr(track_src), ptr(counts2), ptr(ws), ws.numel(), stream_ptr()),
              "sfm_track_restrict")
    return track_off2, obs_node2, track_src, counts2


def adopt_points(counts, track_off, obs_node, restricted, pruned, out=None):
    """sfm_track_adopt: `restricted` is what `restrict_tracks` returned on the full table (counts, track_off, obs_node), `pruned` what
    `prune_tracks` returned on the triangulated and refined restricted table.  Returns (X_full [N // 2 + 1, 3] f32, has_point
    [N // 2 + 1] u8, obs_live [N] u8) for the FULL table: the point of every track that still has one (NaN otherwise) and the
    observations that survived both compactions.  Every counted row is rewritten.  No host wait."""
    _i32(counts, "counts")
    _i32(track_off, "track_off")
    _i32(obs_node, "obs_node")
    n, dev = int(obs_node.numel()), obs_node.device
    cap = n // 2 + 1
    _, _, src_r, counts_r = restricted
    off_p, obs_p, X_p, src_p, counts_p = pruned
    for t, shape, what in ((src_r, (cap,), "restricted track_src"), (src_p, (cap,), "pruned track_src"), (off_p, (cap + 1,), "pruned track_off"),
                           (obs_p, (n,), "pruned obs_node")):
        _i32(t, what, shape)
    _i32(counts_r, "restricted counts")
    _i32(counts_p, "pruned counts")
    _typed(X_p, torch.float32, (cap, 3), "pruned X")
    if counts.numel() < 2 or counts_r.numel() < 2 or counts_p.numel() < 2 or track_off.numel() < cap + 1:
        raise SfmHipError("adopt_points: every counts must hold (tracks, observations) and track_off N // 2 + 2 words")
    if out is None:
        out = (torch.empty((cap, 3), dtype=torch.float32, device=dev), torch.empty(cap, dtype=torch.uint8, device=dev),
               torch.empty(n, dtype=torch.uint8, device=dev))
    X_full, has_point, obs_live = out
    _typed(X_full, torch.float32, (cap, 3), "X_full")
    _u8(has_point, (cap,), "has_point")
    _u8(obs_live, (n,), "obs_live")
    with on_device(dev):
        check(_lib.lib().sfm_track_adopt(ptr(counts), ptr(track_off), ptr(obs_node) if n else None, n, ptr(counts_r), ptr(src_r), ptr(counts_p),
                                         ptr(off_p), ptr(obs_p) if n else None, ptr(X_p), ptr(src_p), ptr(X_full), ptr(has_point),
                                         ptr(obs_live) if n else None, stream_ptr()), "sfm_track_adopt")
    return X_full, has_point, obs_live


def view_scores(counts, node_track, has_point, img_off, keypoints, frame_size, grid=8, out=None):
    """sfm_track_view_scores: per image the keypoints whose track has a point (`seen` int32 [n_img]), the grid x grid cells of the
    frame (width, height) they cover (`cover` int64 [n_img] holding the uint64 mask, bit cy * grid + cx) and the number of cells
    (`cells` int32 [n_img]).  A NaN coordinate counts in seen and sets no bit.  No host wait."""
    n_img = _offsets(img_off)
    _i32(counts, "counts")
    _i32(node_track, "node_track")
    n, dev = int(node_track.numel()), node_track.device
    _u8(has_point, (n // 2 + 1,), "has_point")
    _typed(keypoints, torch.float32, (n, 2), "keypoints")
    if out is None:
        out = (torch.empty(n_img, dtype=torch.int32, device=dev), torch.empty(n_img, dtype=torch.int64, device=dev),
               torch.empty(n_img, dtype=torch.int32, device=dev))
    seen, cover, cells = out
    _i32(seen, "seen", (n_img,))
    _i32(cells, "cells", (n_img,))
    _typed(cover, torch.int64, (n_img,), "cover")
    with on_device(dev):
        check(_lib.lib().sfm_track_view_scores(ptr(counts), ptr(node_track) if n else None, ptr(has_point), ptr(img_off), n_img,
                                               ptr(keypoints) if n else None, n, float(frame_size[0]), float(frame_size[1]), int(grid), ptr(seen),
                                               ptr(cover), ptr(cells), stream_ptr()), "sfm_track_view_scores")
    return seen, cover, cells


def correspondences(image, counts, node_track, has_point, X_full, img_off, keypoints, capacity=None, out=None):
    """sfm_track_correspondences: the rows (X_full[t], keypoint, t) of the keypoints of `image` whose track t has a point, in ascending
    keypoint.  Returns (X [capacity, 3] f32, uv [capacity, 2] f32, track [capacity] i32, count [1] i32); count equals
    `view_scores`' seen[image], so a caller that has read the scores slices the first two and hands them to
    `ransac.solve_pnp_ransac`.  capacity defaults to N.  No host wait."""
    from .ops import _workspace
    n_img = _offsets(img_off)
    _i32(counts, "counts")
    _i32(node_track, "node_track")
    n, dev = int(node_track.numel()), node_track.device
    cap_t = n // 2 + 1
    _u8(has_point, (cap_t,), "has_point")
    _typed(X_full, torch.float32, (cap_t, 3), "X_full")
    _typed(keypoints, torch.float32, (n, 2), "keypoints")
    capacity = n if capacity is None else int(capacity)
    if out is None:
        out = (torch.empty((capacity, 3), dtype=torch.float32, device=dev), torch.empty((capacity, 2), dtype=torch.float32, device=dev),
               torch.empty(capacity, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev))
    X, uv, track, count = out
    _typed(X, torch.float32, (capacity, 3), "X")
    _typed(uv, torch.float32, (capacity, 2), "uv")
    _i32(track, "track", (capacity,))
    _i32(count, "count", (1,))
    L = _lib.lib()
    ws = _workspace(dev, L.sfm_track_correspondences_ws_bytes(n))
    with on_device(dev):
        check(L.sfm_track_correspondences(int(image), ptr(counts), ptr(node_track) if n else None, ptr(has_point), ptr(X_full), ptr(img_off), n_img,
                                          ptr(keypoints) if n else None, n, capacity, ptr(X) if capacity else None, ptr(uv) if capacity else None,
                                          ptr(track) if capacity else None, ptr(count), ptr(ws), ws.numel(), stream_ptr()),
              "sfm_track_correspondences")
    return X, uv, track, count


# ---- the engine on the device -------------------------------------------------------------------------------------------------

class _HipEngine:
    """What the loop needs, on the device.  `tracks` builds the table once; `round` is the stateless model round (a function of the
    tracks, the registered set and P) with ONE host read; the rest are the solvers and the bundle adjustment, which wait as they do."""

    def __init__(self, store, n_query, pairs, keypoints, K, frame_size, ratio, keep, min_len, max_len, huber, obs_thresh, max_reproj,
                 min_angle_deg, refine_iters, grid, rounds=TRACK_ROUNDS):
        self.dev = store.device
        self.store, self.keep, self.ratio, self.rounds = store.contiguous(), keep, ratio, rounds
        self.pairs = [(int(a), int(b)) for a, b in pairs]
        self.K = np.asarray(K, np.float64).reshape(3, 3)
        self.frame_size, self.grid = (float(frame_size[0]), float(frame_size[1])), int(grid)
        self.min_len, self.max_len = int(min_len), max_len
        self.huber, self.obs_thresh, self.max_reproj, self.min_angle_deg, self.refine_iters = huber, obs_thresh, max_reproj, min_angle_deg, refine_iters
        self.img_off, self.kp, self.nq, self.pr, _, self.n = _scene_tensors(n_query, pairs, keypoints, None, self.dev)
        self.n_img = len(keypoints)

    def tracks(self):
        """match_edges -> track_components (resumed until converged) -> build_tracks.  Host waits: one per batch of rounds (the counts
        with the status), as `tracks.run_tracks`.  -> (T, nobs)."""
        dev, n = self.dev, self.n
        edges = match_edges(self.store, self.nq, self.pr, self.img_off, self.ratio, self.keep)
        head = torch.empty(8, dtype=torch.int32, device=dev)
        self.counts = head[:6]
        labels, lowered = None, 0
        while True:
            labels, _ = track_components(edges, n, self.rounds, labels, head[6:8])
            self.node_track, self.track_off, self.obs_node, _ = build_tracks(labels, self.img_off, self.min_len, self.max_len, self.counts)
            host = head.cpu().numpy()
            lowered += int(host[7])
            if host[6]:
                break
        self.host_counts, self.status = host[:6].copy(), np.array([int(host[6]), lowered], np.int32)
        self.T, self.nobs = int(host[0]), int(host[1])
        cap = n // 2 + 1
        i32, f32, u8 = torch.int32, torch.float32, torch.uint8
        self.head = torch.empty(8 + 2 * self.n_img, dtype=i32, device=dev)
        self.restricted = (torch.empty(cap + 1, dtype=i32, device=dev), torch.empty(n, dtype=i32, device=dev), torch.empty(cap, dtype=i32, device=dev),
                           self.head[0:4])
        self.pruned = (torch.empty(cap + 1, dtype=i32, device=dev), torch.empty(n, dtype=i32, device=dev), torch.empty((cap, 3), dtype=f32, device=dev),
                       torch.empty(cap, dtype=i32, device=dev), self.head[4:8])
        self.adopted = (torch.empty((cap, 3), dtype=f32, device=dev), torch.empty(cap, dtype=u8, device=dev), torch.empty(n, dtype=u8, device=dev))
        self.cover = torch.empty(self.n_img, dtype=torch.int64, device=dev)
        return self.T, self.nobs

    def shared(self):
        """int [n_img, n_img]: the kept tracks two images share, counted by sfm_view_pair_counts (the points and cameras it also takes are
        left NaN: only `shared` is read; that entry point takes up to 4 096 images).  One host read."""
        n_img, dev = self.n_img, self.dev
        out = torch.zeros((n_img, n_img), dtype=torch.int32, device=dev)
        if self.T == 0:
            return out.cpu().numpy()
        cam = (torch.searchsorted(self.img_off[:-1].contiguous(), self.obs_node[:self.nobs], right=True) - 1).to(torch.int32).contiguous()
        X = torch.full((self.T, 3), float("nan"), dtype=torch.float64, device=dev)
        P = torch.zeros((n_img, 12), dtype=torch.float64, device=dev)
        C = torch.empty((n_img, 3), dtype=torch.float64, device=dev)
        good = torch.empty_like(out)
        with on_device(dev):
            check(_lib.lib().sfm_view_pair_counts(ptr(self.track_off), ptr(cam), ptr(X), self.T, self.nobs, ptr(P), n_img, -1.0, 1.0, ptr(C), ptr(out),
                                                  ptr(good), stream_ptr()), "sfm_view_pair_counts")
        return out.cpu().numpy()

    def _registered(self, registered):
        return _upload(np.asarray(registered, np.uint8), self.dev)

    def pair_points(self, a, b, m):
        """The keypoints of the m kept tracks images a < b share, in track order: restrict to {a, b} leaves them as (node in a, node in b)."""
        reg = np.zeros(self.n_img, np.uint8)
        reg[[a, b]] = 1
        _, obs2, _, _ = restrict_tracks(self.counts, self.track_off, self.obs_node, self.img_off, self._registered(reg), 2)
        nodes = obs2[:2 * m].view(m, 2).long()
        return self.kp.index_select(0, nodes[:, 0].contiguous()), self.kp.index_select(0, nodes[:, 1].contiguous())

    def relative_pose(self, p0, p1):
        """findEssentialMat (the threshold of verify_keep) and recoverPose on its inliers -> (R, t) or None."""
        from . import ops, ransac
        if p0.shape[0] < 5:
            return None
        E, mask = ransac.find_essential_mat(p0, p1, self.K, E_PROB, E_THRESHOLD, return_device_mask=True)
        if E is None:
            return None
        first = ops.mask_indices(mask).long()
        good, R, t, _ = ransac.recover_pose(E[:3], p0[first], p1[first], self.K)
        return (R, t.reshape(3)) if good > 0 else None

    def round(self, registered, P):
        """restrict -> triangulate -> refine -> prune -> adopt -> scores, enqueued without a host wait, then ONE read of the head words.
        -> dict(points, obs, seen, cells, short, restricted)."""
        n_img = self.n_img
        Pd = _upload(np.ascontiguousarray(np.asarray(P, np.float64).reshape(n_img, 12)), self.dev)
        c_r = self.head[0:4]
        restrict_tracks(self.counts, self.track_off, self.obs_node, self.img_off, self._registered(registered), self.min_len, out=self.restricted)
        off_r, obs_r = self.restricted[0], self.restricted[1]
        X, _, _, flags, _ = triangulate_tracks(c_r, off_r, obs_r, self.img_off, self.kp, Pd)
        rf = refine_tracks(c_r, off_r, obs_r, self.img_off, self.kp, Pd, X, flags, self.huber, self.obs_thresh, self.refine_iters)
        prune_tracks(c_r, off_r, obs_r, rf[0], rf[1], rf[4], rf[5], rf[6], rf[8], self.min_len, self.max_reproj, self.min_angle_deg, out=self.pruned)
        adopt_points(self.counts, self.track_off, self.obs_node, self.restricted, self.pruned, out=self.adopted)
        view_scores(self.counts, self.node_track, self.adopted[1], self.img_off, self.kp, self.frame_size, self.grid,
                    out=(self.head[8:8 + n_img], self.cover, self.head[8 + n_img:]))
        h = self.head.cpu().numpy()                                   # the ONE host read of a model round
        return dict(points=int(h[4]), obs=int(h[5]), seen=h[8:8 + n_img].copy(), cells=h[8 + n_img:].copy(), short=int(h[2]), restricted=int(h[0]),
                    tracks_dropped=int(h[6]), obs_dropped=int(h[7]))

    def correspondences(self, image, n):
        X, uv, _, _ = correspondences(image, self.counts, self.node_track, self.adopted[1], self.adopted[0], self.img_off, self.kp, capacity=n)
        return X, uv

    def pnp(self, X, uv, **kw):
        """-> (ok, R, t, inliers)."""
        from . import hostgeom, ransac
        ok, rvec, tvec, inl = ransac.solve_pnp_ransac(X, uv, self.K, return_device_inliers=True, **kw)
        if not ok:
            return False, None, None, 0
        return True, hostgeom.rodrigues_vec2mat(rvec.reshape(3)), tvec.reshape(3), int(inl.shape[0])

    def _model(self, model):
        """The pruned set of the last round as device tensors: (X [T, 3] f32, obs [nobs, 2] f32, cam [nobs] i32, pt [nobs] i32, off)."""
        off_p, obs_p, X_p, _, _ = self.pruned
        T, nobs = model["points"], model["obs"]
        nodes = obs_p[:nobs]
        cam = (torch.searchsorted(self.img_off[:-1].contiguous(), nodes, right=True) - 1).to(torch.int32)
        pt = torch.searchsorted(off_p[1:T + 1].contiguous(), torch.arange(nobs, dtype=torch.int32, device=self.dev), right=True).to(torch.int32)
        return X_p[:T], self.kp.index_select(0, nodes.long()), cam, pt, off_p[:T + 1]

    def bundle(self, order, P, model, **kw):
        """track_ba.bundle_adjust_tracks over the registered cameras in registration order (the seed's first camera is the fixed one) and
        the pruned set of the last round.  -> (P rows of `order`, history, info)."""
        from . import track_ba
        X, obs, cam, pt, _ = self._model(model)
        rank = np.full(self.n_img, -1, np.int32)
        rank[np.asarray(order)] = np.arange(len(order), dtype=np.int32)
        cam_ba = _upload(rank, self.dev).index_select(0, cam.long()).contiguous()
        cams0 = track_ba.cams_from_P(np.asarray(P, np.float64)[np.asarray(order)], self.K)
        cams, _, hist, info = track_ba.bundle_adjust_tracks(_upload(cams0, self.dev), self.K, X.to(torch.float64), obs, cam_ba, pt.contiguous(), **kw)
        return track_ba.P_from_cams(cams.cpu().numpy(), self.K), hist, info

    def bundle_calibrated(self, order, P, model, calibrate, **kw):
        """`bundle` with track_cal.bundle_adjust_calibrated (docs/tracks.md §15): the rows of P are built with K'; info gains K, dist."""
        from . import track_ba, track_cal
        X, obs, cam, pt, _ = self._model(model)
        rank = np.full(self.n_img, -1, np.int32)
        rank[np.asarray(order)] = np.arange(len(order), dtype=np.int32)
        cam_ba = _upload(rank, self.dev).index_select(0, cam.long()).contiguous()
        cams0 = track_ba.cams_from_P(np.asarray(P, np.float64)[np.asarray(order)], self.K)
        cams, _, K_new, dist, hist, info = track_cal.bundle_adjust_calibrated(_upload(cams0, self.dev), self.K, calibrate.get("dist"), X.to(torch.float64), obs,
                                                                              cam_ba, pt.contiguous(), free=calibrate.get("free", ("f", "k1")), **kw)
        return track_ba.P_from_cams(cams.cpu().numpy(), K_new), hist, dict(info, K=K_new, dist=dist)

    def result(self, model):
        """The ONE download at the end: the keys of run_tracks(robust=True) for the final model."""
        X, obs, cam, pt, off = self._model(model)
        T, nobs = model["points"], model["obs"]
        src = self.restricted[2].index_select(0, self.pruned[3][:T].long()) if T else torch.empty(0, dtype=torch.int32, device=self.dev)
        words = torch.cat([X.reshape(-1).view(torch.int32), off if T else torch.zeros(1, dtype=torch.int32, device=self.dev), cam,
                           obs.reshape(-1).view(torch.int32), src, self.pruned[1][:nobs]])
        host = words.cpu().numpy()
        pos = np.cumsum([0, 3 * T, T + 1, nobs, 2 * nobs, T])
        length = np.diff(host[pos[1]:pos[2]].astype(np.int64))
        return dict(points=np.ascontiguousarray(host[pos[0]:pos[1]].view(np.float32).reshape(T, 3)),
                    obs=np.ascontiguousarray(host[pos[3]:pos[4]].view(np.float32).reshape(nobs, 2)), cam_idx=np.ascontiguousarray(host[pos[2]:pos[3]]),
                    pt_idx=np.repeat(np.arange(T), length).astype(np.int32), track_len=length.astype(np.int32),
                    track_idx=np.ascontiguousarray(host[pos[4]:pos[5]]), track_off=np.ascontiguousarray(host[pos[1]:pos[2]]),
                    obs_node=np.ascontiguousarray(host[pos[5]:]), counts=self.host_counts.copy(), status=self.status.copy(),
                    tracks_dropped=model["tracks_dropped"], obs_dropped=model["obs_dropped"])


# ---- the loop -----------------------------------------------------------------------------------------------------------------

def _camera(K, R, t):
    return K @ np.c_[np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)]


def _pair_config(pair_config, n_pairs):
    """The configuration words of the pairs as a list of ints, or None; SfmHipError on a wrong length or a word outside 0..3."""
    if pair_config is None:
        return None
    if getattr(pair_config, "is_cuda", False):
        raise SfmHipError("register_tracks: pair_config must be a host sequence (download `verify_pairs(...)[\"config\"]` first)")
    try:
        words = [int(w) for w in pair_config]
    except (TypeError, ValueError):
        raise SfmHipError(f"register_tracks: pair_config {pair_config!r} must be a sequence of configuration words") from None
    if len(words) != n_pairs:
        raise SfmHipError(f"register_tracks: pair_config holds {len(words)} words for {n_pairs} pairs")
    if any(not 0 <= w <= 3 for w in words):
        raise SfmHipError("register_tracks: pair_config words must be 0..3 (verify.CONFIG_NONE, _GENERAL, _PLANAR, _ROTATING)")
    return words


def register_loop(eng, n_img, pairs, K, seed_pair=None, min_corr=MIN_CORR, min_seed=MIN_SEED, seed_tries=5, max_tries=2, pnp=None,
                  ba_every=BA_EVERY, ba=None, log=None, pair_config=None, calibrate=None):
    """The loop of `register_tracks` on an engine (see `_HipEngine` for what one provides).  Argument errors are raised before the engine
    does any work."""
    n_img = int(n_img)
    config = _pair_config(pair_config, len(pairs))
    if n_img < 2:
        raise SfmHipError(f"register_tracks: {n_img} images; a seed pair needs two")
    if seed_pair is not None:
        try:
            sa, sb = (int(v) for v in seed_pair)
        except (TypeError, ValueError):
            raise SfmHipError(f"register_tracks: seed_pair {seed_pair!r} must be two image indices") from None
        if not (0 <= sa < n_img and 0 <= sb < n_img) or sa == sb:
            raise SfmHipError(f"register_tracks: seed_pair {(sa, sb)} must name two different images of 0..{n_img - 1}")
        seed_pair = (sa, sb)
    if int(min_corr) < 4:
        raise SfmHipError(f"register_tracks: min_corr {min_corr} must be at least 4 (solve_pnp_ransac takes no fewer correspondences)")
    if int(min_seed) < 1 or int(seed_tries) < 1 or int(max_tries) < 1 or int(ba_every) < 0:
        raise SfmHipError(f"register_tracks: min_seed {min_seed}, seed_tries {seed_tries} and max_tries {max_tries} must be at least 1 and "
                          f"ba_every {ba_every} at least 0 (0: one adjustment at the end)")
    say = log or (lambda *a: None)
    K = np.asarray(K, np.float64).reshape(3, 3)
    pnp = dict(PNP_DEFAULTS, **(pnp or {}))
    ba = dict(dict(huber=1.0, iters=BA_ITERS), **(ba or {}))
    pairs = [(int(a), int(b)) for a, b in pairs]
    eng.tracks()
    shared = eng.shared()
    if seed_pair is None:
        count = np.array([shared[a, b] if 0 <= a < n_img and 0 <= b < n_img and a != b else 0 for a, b in pairs], np.int64)
        cand = [p for p in np.argsort(-count, kind="stable") if count[p] > 0]             # most shared tracks first, ties to the lower pair index
        if config is not None:                                         # GENERAL pairs in that order, then PLANAR; no baseline or no model: never a seed
            cand = [p for p in cand if config[p] == CONFIG_GENERAL] + [p for p in cand if config[p] == CONFIG_PLANAR]
        words = [config[p] for p in cand] if config is not None else None
        cand = [pairs[p] for p in cand]
    else:
        cand, words = [seed_pair], None
    P = np.zeros((n_img, 3, 4))
    registered = np.zeros(n_img, np.uint8)
    best, rejected, model, seeds = 0, 0, None, []
    for k, (a, b) in enumerate(cand):
        if rejected >= seed_tries:
            break
        lo, hi = min(a, b), max(a, b)
        p_lo, p_hi = eng.pair_points(lo, hi, int(shared[lo, hi]))
        p_a, p_b = (p_lo, p_hi) if a < b else (p_hi, p_lo)
        pose = eng.relative_pose(p_a, p_b)
        points = 0
        if pose is not None:
            P[:], registered[:] = 0.0, 0
            P[a], P[b] = _camera(K, np.eye(3), np.zeros(3)), _camera(K, *pose)
            registered[[a, b]] = 1
            model = eng.round(registered, P)
            points = model["points"]
        seeds.append(dict(pair=(a, b), shared=int(shared[lo, hi]), points=points))
        if words is not None:
            seeds[-1]["config"] = words[k]
        say(f"register: seed {(a, b)} shares {int(shared[lo, hi])} tracks, its round leaves {points} points")
        best = max(best, points)
        if pose is not None and points >= min_seed:
            break
        rejected += 1
        model = None
    if model is None:
        raise SfmHipError(f"register_tracks: no seed pair left {min_seed} points after {rejected} candidates (the best left {best})")
    order, steps = [a, b], []
    tries = np.zeros(n_img, np.int32)
    blocked, since_ba, histories, rounds = set(), 0, [], len(seeds)
    while True:
        open_ = [i for i in range(n_img) if not registered[i] and i not in blocked and tries[i] < max_tries and model["seen"][i] >= min_corr]
        if not open_:
            break
        i = max(open_, key=lambda j: (int(model["cells"][j]), int(model["seen"][j]), -j))
        seen, cells = int(model["seen"][i]), int(model["cells"][i])
        X, uv = eng.correspondences(i, seen)
        ok, R, t, inliers = eng.pnp(X, uv, **pnp)
        accepted = bool(ok) and inliers >= min_corr
        steps.append(dict(image=i, seen=seen, cells=cells, inliers=int(inliers), accepted=accepted))
        say(f"register: image {i} sees {seen} points in {cells} cells, PnP {'fails' if not ok else f'{inliers} inliers'}")
        if not accepted:
            tries[i] += 1
            blocked.add(i)                                             # tried again only after another image has registered
            continue
        P[i] = _camera(K, R, t)
        registered[i] = 1
        order.append(i)
        blocked.clear()
        since_ba += 1
        if ba_every and since_ba >= ba_every:
            model = eng.round(registered, P)
            rounds += 1
            if model["points"]:
                P[order], hist, _ = eng.bundle(order, P, model, **ba)
                histories.append(hist)
            since_ba = 0
        model = eng.round(registered, P)
        rounds += 1
    calibrated = None
    if calibrate is not None and model["points"]:                      # the FINAL adjustment is the calibrated one; the rounds before it are untouched
        P[order], hist, calibrated = eng.bundle_calibrated(order, P, model, calibrate, **ba)
        histories.append(hist)
        model = eng.round(registered, P)
        rounds += 1
    elif (since_ba or not histories) and model["points"]:
        P[order], hist, _ = eng.bundle(order, P, model, **ba)
        histories.append(hist)
        model = eng.round(registered, P)
        rounds += 1
    out = eng.result(model)
    if calibrate is not None:
        out.update(K=calibrated["K"] if calibrated else K.copy(), dist=calibrated["dist"] if calibrated else np.asarray((0.0, 0.0) if calibrate.get("dist") is None else calibrate["dist"], np.float64).reshape(2))
    P_out = np.full((n_img, 3, 4), np.nan)
    P_out[order] = P[order]
    out.update(P=P_out, registered=registered.astype(bool), order=np.array(order, np.int32), tries=tries, steps=steps, seeds=seeds,
               seen=model["seen"], cells=model["cells"], ba_history=histories, rounds=rounds)
    return out


def register_tracks(store, n_query, pairs, keypoints, K, frame_size, ratio=0.70, keep=None, seed_pair=None, min_len=2, max_len=None, huber=1.0,
                    obs_thresh=2.0, max_reproj=2.0, min_angle_deg=2.0, refine_iters=10, grid=8, min_corr=MIN_CORR, min_seed=MIN_SEED, seed_tries=5,
                    max_tries=2, pnp=None, ba_every=BA_EVERY, ba=None, log=None, pair_config=None, calibrate=None):
    """Cameras of unordered images from their all-pairs matches.  store, n_query, pairs as `sharded.match_pairs_sharded` returns and takes
    them; keypoints: list over images of [n_i, 2] float32 device tensors, 2 to 4 096 images (the four kernels take 65 536; the seed
    order is counted by sfm_view_pair_counts, which takes 4 096); K 3 x 3 (one camera model); frame_size (width, height).  SfmHipError
    before any device work for: min_len < 2, more than 4 096 images, a seed_pair that does not name two different images, min_corr < 4
    (solve_pnp_ransac takes no fewer), min_seed, seed_tries or max_tries < 1, ba_every < 0, a pair_config of another length than pairs or
    with a word outside 0..3.

    pair_config: None, or a host sequence of len(pairs) two-view configuration words (`verify_pairs(homography=...)["config"]`,
    downloaded).  With it and no explicit seed_pair the seed candidates are the GENERAL pairs in the order below, then the PLANAR pairs;
    a ROTATING pair (no baseline) or a pair without a model is never tried, and every entry of `seeds` gains `config`.  An explicit
    seed_pair is honoured whatever its word.

    Tracks are built once.  The seed is the pair with the most shared tracks (or `seed_pair`) whose essential matrix, recoverPose and
    one model round leave at least `min_seed` points; up to `seed_tries` candidates are rejected before SfmHipError.  A model round
    (restrict -> triangulate -> refine(huber, obs_thresh, refine_iters) -> prune(min_len, max_reproj, min_angle_deg) -> adopt -> scores)
    is a function of the tracks, the registered set and P.  The next view is the unregistered image with seen >= min_corr and fewer than
    `max_tries` failures that covers the most cells of the grid x grid frame (then the most points, then the lowest index); it registers
    iff `solve_pnp_ransac(**pnp)` succeeds with at least min_corr inliers, else it is tried again only after another image has
    registered.  `track_ba.bundle_adjust_tracks(**ba)` (default huber=1, iters=15) runs every `ba_every` registrations and once at the
    end over the registered cameras in registration order, the seed's first camera fixed.

    Returns P [n_img, 3, 4] float64 (NaN rows for unregistered images), registered, order, tries, steps (per attempt: image, seen,
    cells, inliers, accepted), seeds, ba_history, rounds, and the keys of run_tracks(robust=True) for the final model (points, obs,
    cam_idx, pt_idx, track_len, counts, status, tracks_dropped, obs_dropped) plus track_idx, track_off, obs_node: `adjust_tracks` and
    `densify_tracks` take the result as it is when every image registered.  An unregistered image keeps its NaN row through
    `adjust_tracks(result, result["P"], K)`: no observation names it, so its camera has zero blocks and takes no step
    (tests/test_gpu_tracks_register.py, scene 4); `densify_tracks` plans a depth map per row of P and is not exercised on NaN rows: keep
    the registered images and renumber cam_idx before it.

    calibrate: None (the code path above exactly), or dict(free=("f", "k1"), dist=None): the FINAL adjustment is
    `track_cal.bundle_adjust_calibrated` (docs/tracks.md §15) and always runs; the rows of P are built with K', and the result gains
    "K" (3 x 3) and "dist" (k1, k2).  The registration rounds and the adjustments before it use the K given here.

    Host waits outside the solvers (E-RANSAC / recoverPose, PnP) and the bundle adjustment: the tracks' one per batch of labelling
    rounds, ONE read of the shared-track counts, ONE read per model round (a seed candidate, a registration, a bundle adjustment and the
    end cost one round each; a failed PnP costs none), and ONE download at the end."""
    if min_len < 2:
        raise SfmHipError(f"register_tracks: min_len {min_len} must be at least 2 (a point needs two views)")
    _pair_config(pair_config, len(pairs))
    if len(keypoints) > MAX_IMAGES:
        raise SfmHipError(f"register_tracks: {len(keypoints)} images exceed {MAX_IMAGES}, the limit of sfm_view_pair_counts, which counts the "
                          "tracks two images share for the seed order")
    if calibrate is not None and sorted(set(calibrate) - {"free", "dist"}):
        raise SfmHipError(f"register_tracks: calibrate takes free and dist, not {sorted(set(calibrate) - {'free', 'dist'})}")
    eng = _HipEngine(store, n_query, pairs, keypoints, K, frame_size, ratio, keep, min_len, max_len, huber, obs_thresh, max_reproj, min_angle_deg,
                     refine_iters, grid)
    return register_loop(eng, len(keypoints), pairs, K, seed_pair, min_corr, min_seed, seed_tries, max_tries, pnp, ba_every, ba, log, pair_config, calibrate)
