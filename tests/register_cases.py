"""What the TRACKS-REGISTER tests share (docs/tracks.md §10): the scenes, the CPU engine that runs `register.register_loop` on the NumPy
restatements and the oracle's three RANSAC solvers, and the figures both test files compare against."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import np_track_ba as ntb  # noqa: E402
import np_tracks as nt  # noqa: E402
import np_tracks_refine as nr  # noqa: E402
import np_tracks_register as ng  # noqa: E402

FRAME = (968.0, 648.0)          # the frame of pose.csv's K: datagen draws clutter inside it
CENTRE_BAR = 1.5                # the median aligned centre error after the final BA against the same BA started from the planted cameras
CLUTTER_IMAGE = 5               # scene 4: the image whose descriptors are random
RING_PERM = (3, 7, 0, 5, 2, 6, 1, 4)
GUSTAV_PERM = (6, 2, 5, 0, 7, 3, 1, 4)


def _remake(case, kps, des, ids, P, X=None):
    from test_tracks_cpu import finish_case
    n = len(kps)
    pairs = [(i, j) for i in range(n) for j in range(i + 1, n)]
    return finish_case(case["K"], P, kps, des, ids, pairs, case["X"] if X is None else X)


def _split(case):
    off = case["img_off"]
    return [case["ids"][off[i]:off[i + 1]] for i in range(len(off) - 1)]


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> the case dict of test_tracks_cpu.finish_case (K, P planted, kps, des, ids, pairs, store, nq, img_off, kp, X)."""
    from test_tracks_cpu import gustav_case, ring_case
    if name == "ring":
        return ring_case()
    if name in ("ring_permuted", "gustav_permuted"):
        case, perm = (ring_case(), RING_PERM) if name == "ring_permuted" else (gustav_case(), GUSTAV_PERM)
        ids = _split(case)
        return _remake(case, [case["kps"][i] for i in perm], [case["des"][i] for i in perm], [ids[i] for i in perm], case["P"][list(perm)])
    if name == "ring_duplicate":                                         # image 0 appended again as image 8
        case = ring_case()
        ids = _split(case)
        return _remake(case, case["kps"] + [case["kps"][0]], case["des"] + [case["des"][0]], ids + [ids[0]], np.concatenate([case["P"], case["P"][:1]]))
    if name == "ring_clutter":                                           # one image's descriptors replaced by random ones
        from datagen import sift_like
        case = ring_case()
        ids, des = _split(case), list(case["des"])
        des[CLUTTER_IMAGE] = sift_like(np.random.default_rng(41), len(des[CLUTTER_IMAGE])).astype(np.float32)
        ids[CLUTTER_IMAGE] = np.full(len(ids[CLUTTER_IMAGE]), -1)
        return _remake(case, case["kps"], des, ids, case["P"])
    if name == "ring_corrupted":                                         # corrupted_ring()'s keypoints: one of 107 tracks' keypoints displaced
        from test_tracks_refine_cpu import corrupted_ring
        c = corrupted_ring()
        case, off = dict(c["case"]), c["case"]["img_off"]
        case["kp"] = c["kp"]
        case["kps"] = [c["kp"][off[i]:off[i + 1]] for i in range(len(off) - 1)]
        return case
    raise KeyError(name)


class NumpyEngine:
    """The engine of `register.register_loop` on the restatements (np_tracks, np_tracks_refine, np_tracks_register, np_track_ba) and the
    oracle's find_essential_mat / recover_pose / solve_pnp_ransac."""

    def __init__(self, case, min_len=2, max_len=2 ** 31 - 1, huber=1.0, obs_thresh=2.0, max_reproj=2.0, min_angle_deg=2.0, refine_iters=10, grid=8,
                 ratio=0.70, frame_size=FRAME, keep=None):
        self.case, self.K = case, np.asarray(case["K"], np.float64).reshape(3, 3)
        self.img_off, self.kp = np.asarray(case["img_off"], np.int32), np.asarray(case["kp"], np.float32)
        self.n, self.n_img = int(self.img_off[-1]), len(self.img_off) - 1
        self.min_len, self.max_len, self.ratio, self.keep = min_len, max_len, ratio, keep
        self.huber, self.obs_thresh, self.max_reproj, self.refine_iters = huber, obs_thresh, max_reproj, refine_iters
        self.max_cos = 1.0 if not min_angle_deg else float(np.cos(np.deg2rad(float(min_angle_deg))))
        self.grid, self.frame_size = grid, frame_size
        self.pnp_calls = 0

    def tracks(self):
        c = self.case
        edges = nt.match_edges(c["store"], c["nq"], c["pairs"], self.img_off, self.ratio, self.keep)
        self.node_track, self.track_off, self.obs_node, self.counts = nt.build(nt.components(edges, self.n), self.img_off, self.min_len, self.max_len)
        return int(self.counts[0]), int(self.counts[1])

    def shared(self):
        T = int(self.counts[0])
        M = np.zeros((T, self.n_img), np.int64)
        M[np.repeat(np.arange(T), np.diff(self.track_off)), nt.image_of(self.img_off, self.obs_node)] = 1
        S = M.T @ M
        np.fill_diagonal(S, 0)
        return S

    def pair_points(self, a, b, m):
        reg = np.zeros(self.n_img, np.uint8)
        reg[[a, b]] = 1
        _, obs2, _, c2 = ng.restrict(self.counts, self.track_off, self.obs_node, self.img_off, reg, self.n, 2)
        assert int(c2[0]) == m
        nodes = obs2.reshape(m, 2)
        return self.kp[nodes[:, 0]], self.kp[nodes[:, 1]]

    def relative_pose(self, p0, p1):
        from oracle import oracle as O
        if len(p0) < 5:
            return None
        E, mask = O.find_essential_mat(p0, p1, self.K, 0.999, 0.4)
        if E is None:
            return None
        first = np.flatnonzero(mask.ravel())
        good, R, t, _ = O.recover_pose(E[:3], p0[first], p1[first], self.K)
        return (R, t.reshape(3)) if good > 0 else None

    def round(self, registered, P):
        P12 = np.asarray(P, np.float64).reshape(self.n_img, 12)
        with np.errstate(all="ignore"):
            self.restricted = r = ng.restrict(self.counts, self.track_off, self.obs_node, self.img_off, registered, self.n, self.min_len)
            X, _, _, flags, _ = nt.triangulate(r[0], r[1], self.img_off, self.kp, P12)
            rf = nr.refine(r[0], r[1], self.img_off, self.kp, P12, X, flags, self.huber, self.obs_thresh, self.refine_iters)
            self.pruned = p = nr.prune(r[0], r[1], rf[0], rf[1], rf[4], rf[5], rf[6], rf[8], self.min_len,
                                       np.inf if self.max_reproj is None else self.max_reproj, self.max_cos)
            self.adopted = ng.adopt(self.counts, self.track_off, self.obs_node, self.n, r[3], r[2], p[4], p[0], p[1], p[2], p[3])
            seen, self.cover, cells = ng.view_scores(self.counts, self.node_track, self.adopted[1], self.img_off, self.kp, self.n, *self.frame_size,
                                                     self.grid)
        return dict(points=int(p[4][0]), obs=int(p[4][1]), seen=seen, cells=cells, short=int(r[3][2]), restricted=int(r[3][0]),
                    tracks_dropped=int(p[4][2]), obs_dropped=int(p[4][3]))

    def correspondences(self, image, n):
        X, uv, _ = ng.correspondences(image, self.counts, self.node_track, self.adopted[1], self.adopted[0], self.img_off, self.kp, self.n)
        assert len(X) == n
        return X, uv

    def pnp(self, X, uv, iterations_count=100, reprojection_error=8.0, confidence=0.99):
        from oracle import oracle as O
        self.pnp_calls += 1
        ok, rvec, tvec, inl = O.solve_pnp_ransac(X, uv, self.K, iterations_count, reprojection_error, confidence)[:4]
        if not ok:
            return False, None, None, 0
        return True, O.rodrigues_vec2mat(rvec.reshape(3)), tvec.reshape(3), len(inl)

    def _model(self):
        off, obs_node, X = self.pruned[0].astype(np.int64), self.pruned[1].astype(np.int64), self.pruned[2]
        return X, self.kp[obs_node], nt.image_of(self.img_off, obs_node).astype(np.int32), np.repeat(np.arange(len(off) - 1), np.diff(off)).astype(np.int32)

    def bundle(self, order, P, model, huber=1.0, iters=15, **kw):
        X, obs, cam, pt = self._model()
        rank = np.full(self.n_img, -1, np.int32)
        rank[np.asarray(order)] = np.arange(len(order))
        cams, _, hist, info = ntb.bundle_adjust(cams_of(np.asarray(P)[np.asarray(order)], self.K), self.K, X.astype(np.float64), obs, rank[cam], pt,
                                                huber=huber, iters=iters, **kw)
        return P_of(cams, self.K), hist, info

    def result(self, model):
        X, obs, cam, pt = self._model()
        off = self.pruned[0]
        return dict(points=X, obs=obs, cam_idx=cam, pt_idx=pt, track_len=np.diff(off).astype(np.int32), track_idx=self.restricted[2][self.pruned[3]],
                    track_off=off, obs_node=self.pruned[1], counts=self.counts, status=np.array([1, 0], np.int32),
                    tracks_dropped=model["tracks_dropped"], obs_dropped=model["obs_dropped"])


class FailFirstPnp(NumpyEngine):
    """Forces the first PnP call to fail: the image costs one try and registers on its second."""

    def pnp(self, X, uv, **kw):
        if self.pnp_calls == 0:
            self.pnp_calls += 1
            return False, None, None, 0
        return super().pnp(X, uv, **kw)


def cams_of(P, K):
    """[n, 6] (rvec, tvec) of P = K [R | t], the rotation through the oracle's Rodrigues."""
    from oracle import oracle as O
    Kinv = np.linalg.inv(np.asarray(K, np.float64).reshape(3, 3))
    out = np.empty((len(P), 6))
    for i, p in enumerate(np.asarray(P, np.float64).reshape(-1, 3, 4)):
        Rt = Kinv @ p
        U, _, Vt = np.linalg.svd(Rt[:, :3])
        out[i, :3], out[i, 3:] = O.rodrigues_mat2vec(U @ Vt), Rt[:, 3]
    return out


def P_of(cams, K):
    from oracle import oracle as O
    K = np.asarray(K, np.float64).reshape(3, 3)
    return np.stack([K @ np.c_[O.rodrigues_vec2mat(c[:3]), c[3:]] for c in np.asarray(cams, np.float64).reshape(-1, 6)])


def centres_of(P):
    P = np.asarray(P, np.float64).reshape(-1, 3, 4)
    return np.stack([-np.linalg.solve(p[:, :3], p[:, 3]) for p in P])


def centre_errors(P, truth):
    """Distances of the camera centres of P to those of `truth` after the least-squares similarity (Umeyama) that maps them there."""
    A, Bt = centres_of(P), centres_of(truth)
    ma, mb = A.mean(0), Bt.mean(0)
    U, S, Vt = np.linalg.svd((Bt - mb).T @ (A - ma) / len(A))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    s = np.trace(np.diag(S) @ D) / ((A - ma) ** 2).sum(1).mean()
    return np.linalg.norm((s * (A - ma) @ (U @ D @ Vt).T + mb) - Bt, axis=1)


def truth_start(case, out, huber=1.0, iters=15):
    """The reference of the centre bar: np_track_ba.bundle_adjust on the SAME tracks (the observations of `out`), started from the
    planted cameras and the points they triangulate, cameras in `out`'s registration order.  -> (median centre error, final cost)."""
    order = np.asarray(out["order"])
    P = np.asarray(case["P"], np.float64)
    X = nt.triangulate(out["track_off"], out["obs_node"], case["img_off"], case["kp"], P.reshape(-1, 12))[0].astype(np.float64)
    rank = np.full(len(P), -1, np.int32)
    rank[order] = np.arange(len(order))
    cams, _, hist, _ = ntb.bundle_adjust(cams_of(P[order], case["K"]), case["K"], X, out["obs"], rank[out["cam_idx"]], out["pt_idx"], huber=huber,
                                         iters=iters)
    return float(np.median(centre_errors(P_of(cams, case["K"]), P[order]))), hist[-1]


def pure_tracks(case, out):
    """(tracks with a point, those that hold one scene-point id and no clutter) by test_tracks_cpu.purity."""
    from test_tracks_cpu import purity
    if len(out["track_off"]) < 2:
        return 0, 0
    n, pure, _ = purity(case, out)
    return n, pure


@functools.lru_cache(maxsize=None)
def twin(name, engine=NumpyEngine, **kw):
    """The CPU twin of register_tracks on scene `name` at the defaults -> (case, engine, result)."""
    from sfm_mvs_amd import register
    case = scene(name)
    eng = engine(case)
    out = register.register_loop(eng, eng.n_img, case["pairs"], case["K"], **kw)
    return case, eng, out
