"""Shapes, inputs and sampled subsets shared by test_np_ba_cpu.py (which proves that the float64 reference alone holds
the bar on these inputs) and test_gpu_ba_schur.py (which holds the kernels to it)."""
import functools

import numpy as np

import np_ba
from datagen import ba_problem, load_pose_csv, ring_cameras


# ---------------------------------------------------------------- the launch plan, restated
def pick_camera_chunks(tiles, ncam, slots, max_chunks=64):
    """sfm::pick_camera_chunks, sfm_mvs_amd/csrc/common.h (the function after note_host_sync / stream_sync)."""
    cap = max(1, min(ncam // 16, max_chunks))
    best, best_cost = 1, 1e300
    for n in range(1, cap + 1):
        rounds, cams = (tiles * n + slots - 1) // slots, (ncam + n - 1) // n
        cost = float(rounds * cams) * (1.0 + 0.006 * n)
        if cost < best_cost:
            best_cost, best = cost, n
    return best


def schur_plan(ncam, npt, cam_side):
    """schur_plan(), sfm_mvs_amd/csrc/ba_schur.hip: (PP, tiles, camera chunks); cam_side: the W product (1024 slots),
    otherwise the W^T product (1280 slots)."""
    pp = 4 if npt >= 64 * 1024 else 2
    tiles = (npt + 256 * pp - 1) // (256 * pp)
    return pp, tiles, pick_camera_chunks(tiles, ncam, 1024 if cam_side else 1280)


def chunk_bounds(ncam, nch):
    """[c_begin, c_end) of every camera chunk, as schur_wt_kernel / schur_w_kernel split them."""
    return [(ncam * ch // nch, ncam * (ch + 1) // nch) for ch in range(nch)]


# (ncam, npt): PP, tiles, nch of W^T, nch of W, reference ("full" or "sampled")
PRODUCT_SHAPES = {
    (1, 1): (2, 1, 1, 1, "full"),                   # minimum
    (3, 511): (2, 1, 1, 1, "full"),                 # tile edge ...
    (3, 512): (2, 1, 1, 1, "full"),
    (3, 513): (2, 2, 1, 1, "full"),                 # ... one live lane in the last tile
    (33, 513): (2, 2, 2, 2, "full"),                # two chunks, uneven 16 / 17
    (50, 4099): (2, 9, 3, 3, "full"),               # three chunks; 36 fold rows: second trip of the fold, ragged
    (3, 65535): (2, 128, 1, 1, "full"),             # the PP switch; many fold rounds
    (3, 65536): (4, 64, 1, 1, "full"),
    (32, 65537): (4, 65, 2, 2, "sampled"),          # PP = 4 with chunks; one live lane in the last tile
    (96, 200000): (4, 196, 6, 5, "sampled"),        # the two sides choose different chunk counts
}
PCG_SHAPES = [(173, 600), (40, 1500)]               # n = 6 ncam = 1038 > 1024 (ten camera chunks) and a one-trip shape
PCG_LAM = 1e-2
PCG_TOL = 1e-13
PCG_ITERS = 200


# ---------------------------------------------------------------- product inputs
@functools.lru_cache(maxsize=None)
def product_problem(ncam, npt):
    """K, cams [ncam, 6], X float32 [npt, 3] in the unit ball seen from a ring of radius 8, random x [ncam, 6], v [npt, 3]."""
    rng = np.random.default_rng(1000 * ncam + npt)
    K, _ = load_pose_csv()
    cams = ring_cameras(ncam) * (1 + 0.01 * rng.standard_normal((ncam, 6)))
    X = rng.normal(0, 1, (npt, 3))
    X /= np.maximum(1.0, np.linalg.norm(X, axis=1, keepdims=True) / rng.uniform(0.2, 1.0, (npt, 1)))
    X = X.astype(np.float32)
    return K, cams, X, rng.standard_normal((ncam, 6)), rng.standard_normal((npt, 3))


def sample_points(npt, pp, tiles, count=2000, edge_tiles=3):
    """Point 0, the last point, both sides of every multiple of 256 (hence of 256 PP) in the first and last few tiles,
    and random points up to `count`."""
    tile = 256 * pp
    pts = {0, npt - 1}
    for t in list(range(0, edge_tiles + 1)) + list(range(max(0, tiles - edge_tiles), tiles + 1)):
        for m in range(t * tile, (t + 1) * tile + 1, 256):
            pts.update(p for p in (m - 1, m) if 0 <= p < npt)
    rng = np.random.default_rng(npt)
    pts.update(rng.choice(npt, max(0, count - len(pts)), replace=False).tolist())
    return np.array(sorted(pts), np.int64)


def sample_cameras(ncam, nch):
    """First and last camera of every chunk."""
    cams = set()
    for b, e in chunk_bounds(ncam, nch):
        cams.update((b, e - 1))
    return np.array(sorted(cams), np.int64)


@functools.lru_cache(maxsize=None)
def product_reference(ncam, npt, reverse=False):
    """(pt_sel, want_u [len(pt_sel), 3], cam_sel, want_w [len(cam_sel), 6]); the selections are None for a full reference.
    reverse=None: want_u and want_w are (forward, reversed) pairs."""
    K, cams, X, x, v = product_problem(ncam, npt)
    pp, tiles, nch_wt, nch_w, kind = PRODUCT_SHAPES[(ncam, npt)]
    pt_sel = cam_sel = None
    if kind == "sampled":
        pt_sel = sample_points(npt, pp, tiles)
        cam_sel = sample_cameras(ncam, nch_w)
    return (pt_sel, np_ba.wt_product(cams, K, X, x, pt_sel, reverse), cam_sel, np_ba.w_product(cams, K, X, v, cam_sel, reverse))


# ---------------------------------------------------------------- camera and depth edges
EDGE_NORMS = [0.0, 1e-20, 1e-12, 1e-8, 1e-4, np.pi - 1e-6, np.pi, 4.0]


@functools.lru_cache(maxsize=None)
def edge_problem():
    """12 cameras x 600 points.  Cameras 0..7 carry the rotation-vector norms EDGE_NORMS about random axes, 8..11 are
    ordinary; every camera sits at t_z ~ 8 in front of the unit ball except camera 0, the identity, which has
    t_z = -Z_w of point 0 (Z_w = -2 exactly): point 0 has z' = 0 exactly there.  Points 1..5 lie behind camera 0
    (Z_w <= -3 -> z' <= -1) and in front of all others."""
    rng = np.random.default_rng(77)
    K, _ = load_pose_csv()
    ncam, npt = 12, 600
    cams = np.zeros((ncam, 6))
    for i in range(ncam):
        d = rng.standard_normal(3)
        d /= np.linalg.norm(d)
        cams[i, :3] = d * (EDGE_NORMS[i] if i < len(EDGE_NORMS) else rng.uniform(0.3, 2.5))
        cams[i, 3:] = [0.1 * rng.standard_normal(), 0.1 * rng.standard_normal(), 8.0 + 0.2 * rng.standard_normal()]
    X = rng.normal(0, 1, (npt, 3))
    X /= np.maximum(1.0, np.linalg.norm(X, axis=1, keepdims=True) / rng.uniform(0.2, 1.0, (npt, 1)))
    X[0] = [0.25, -0.5, -2.0]
    X[1:6, 2] = [-3.0, -3.5, -4.0, -4.5, -5.0]
    cams[0, 3:] = [0.125, 0.0625, 2.0]
    X = X.astype(np.float32)
    assert np_ba.rotation(cams[0, :3])[2] @ X[0].astype(np.float64) + cams[0, 5] == 0.0
    return K, cams, X, rng.standard_normal((ncam, 6)), rng.standard_normal((npt, 3))


@functools.lru_cache(maxsize=None)
def depth_problem():
    """12 cameras x 600 points with depths from 1e-6 to 1e6 in one problem.  Camera 0 is the identity at the origin, so the
    points 0..19, scaled to 1e-6 .. 1e-1 with Z_w > 0, have z' = Z_w there without any cancellation (a depth of 1e-6 formed
    as the difference of O(1) numbers would carry 1e-10 of rounding in BOTH implementations: not a reciprocal's fault);
    points 20..39 are scaled to 1e2 .. 1e6 (that deep in front of camera 0, anywhere for the ring); cameras 10 and 11 stand 1e3 and 1e6 away."""
    rng = np.random.default_rng(78)
    K, _ = load_pose_csv()
    ncam, npt = 12, 600
    cams = ring_cameras(ncam) * (1 + 0.01 * rng.standard_normal((ncam, 6)))
    cams[0] = 0
    X = rng.normal(0, 1, (npt, 3))
    X /= np.maximum(1.0, np.linalg.norm(X, axis=1, keepdims=True) / rng.uniform(0.2, 1.0, (npt, 1)))
    near = np.abs(rng.uniform(0.3, 1.0, (20, 3))) * np.logspace(-6, -1, 20)[:, None]
    X[:20] = near
    far = rng.uniform(0.3, 1.0, (20, 3)) * np.logspace(2, 6, 20)[:, None]
    far[:, 2] = np.abs(far[:, 2])
    X[20:40] = far
    X[40:] += [0, 0, 3.0]                                            # the ordinary points: in front of camera 0 as well
    cams[10, 3:] *= 1e3 / 8
    cams[11, 3:] *= 1e6 / 8
    return K, cams, X.astype(np.float32), rng.standard_normal((ncam, 6)), rng.standard_normal((npt, 3))


def full_visibility(ncam, npt):
    return np.repeat(np.arange(ncam), npt).astype(np.int32), np.tile(np.arange(npt), ncam).astype(np.int32)


# ---------------------------------------------------------------- indexed products
@functools.lru_cache(maxsize=None)
def indexed_problem():
    K, cams, X, _ = ba_problem(8, 300, 0.5, seed=91)
    rng = np.random.default_rng(92)
    return K, cams, X, rng.standard_normal((8, 6)), rng.standard_normal((300, 3))


@functools.lru_cache(maxsize=None)
def indexed_cases():
    """name -> (cam_idx, pt_idx), int32, always in range."""
    ncam, npt = 8, 300
    rng = np.random.default_rng(93)
    cases = {}
    for nobs in (0, 1, 255, 256, 257):
        sel = rng.permutation(ncam * npt)[:nobs]
        cases[f"nobs{nobs}"] = (sel // npt, sel % npt)
    cases["one_pair_2000_times"] = (np.full(2000, 3), np.full(2000, 7))               # worst-case contention
    sel = rng.permutation(ncam * npt)[:400]
    cases["repeated_verbatim"] = (np.tile(sel // npt, 2), np.tile(sel % npt, 2))
    vis = rng.random((ncam, npt)) < 0.5
    vis[5] = False                                                                      # a camera nobody sees through
    vis[:, [0, 17, 299]] = False                                                        # points nobody sees
    ci, pi = np.nonzero(vis)
    cases["empties_sorted"] = (ci, pi)
    order = rng.permutation(len(ci))
    cases["empties_shuffled"] = (ci[order], pi[order])
    return {k: (np.ascontiguousarray(c, np.int32), np.ascontiguousarray(p, np.int32)) for k, (c, p) in cases.items()}


# ---------------------------------------------------------------- the damped step
@functools.lru_cache(maxsize=None)
def pcg_problem(ncam, npt):
    """K, cams, X, obs of datagen.ba_problem and the reference W [ncam, npt, 6, 3]."""
    K, cams, X, obs = ba_problem(ncam, npt, 0.5, seed=7 * ncam + npt)
    Jc, Jp = np_ba.jacobians(cams, K, X)
    return K, cams, X, obs, np.einsum("ijka,ijkb->ijab", Jc, Jp)
