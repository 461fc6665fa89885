"""Shapes, inputs and references shared by test_np_gn_cpu.py (which proves on the CPU that every shape lands on the launch
plan claimed for it, that the float64 reference alone holds the bar on these inputs, and that the float32 roundings the
masks depend on are decidable) and test_gpu_gn_sweeps.py (which holds csrc/residual.hip, csrc/ba_dense.hip and
project_f64_kernel of csrc/ransac.hip to the reference).  Every index handed to a kernel is in range."""
import functools
import os
import re

import numpy as np

import ba_cases
import np_ba
from datagen import ba_problem, load_pose_csv, ring_cameras

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sfm_mvs_amd", "csrc")

# ---------------------------------------------------------------- the launch plans, restated
DENSE_SLOTS = 512            # dense_plan(): sfm::pick_camera_chunks(d.tiles, ncam, 512)
DENSE_PP_SWITCH = 64 * 1024  # dense_plan(): d.pp = npt >= 64 * 1024 ? 4 : 2
REDUCE_CHUNK = 2048          # residual.hip: constexpr int kReduceChunk
RESIDUAL_BLOCK = 256         # residual_kernel: one lane per observation, 256 lanes


def dense_plan(ncam, npt, switch=DENSE_PP_SWITCH, slots=DENSE_SLOTS):
    """dense_plan(), sfm_mvs_amd/csrc/ba_dense.hip: (PP, tiles, camera chunks)."""
    pp = 4 if npt >= switch else 2
    tiles = (npt + 256 * pp - 1) // (256 * pp)
    return pp, tiles, ba_cases.pick_camera_chunks(tiles, ncam, slots)


def residual_plan(nobs, chunk=REDUCE_CHUNK):
    """sfm_project_residual, sfm_mvs_amd/csrc/residual.hip: (blocks = partial rows, level1 = workgroups of reduce_rows_kernel,
    which runs only if level1 > 1)."""
    blocks = (nobs + RESIDUAL_BLOCK - 1) // RESIDUAL_BLOCK
    return blocks, (blocks + chunk - 1) // chunk


def source_constants():
    """(kReduceChunk, the PP threshold, the slot count) as the .hip text states them."""
    with open(os.path.join(CSRC, "residual.hip")) as f:
        chunk = int(re.search(r"constexpr int kReduceChunk = (\d+);", f.read()).group(1))
    with open(os.path.join(CSRC, "ba_dense.hip")) as f:
        text = f.read()
    a, b = re.search(r"d\.pp = npt >= (\d+) \* (\d+) \? 4 : 2;", text).groups()
    slots = int(re.search(r"d\.nch = sfm::pick_camera_chunks\(d\.tiles, ncam, (\d+)\);", text).group(1))
    return chunk, int(a) * int(b), slots


# (ncam, npt): PP, tiles, nch, fold rows (4 per tile: one per wave), reference ("full": every point row; "sampled": the
# point rows of ba_cases.sample_points — the camera blocks always run over every point)
DENSE_SHAPES = {
    (1, 1): (2, 1, 1, 4, "full"),                   # minimum: one live lane
    (3, 511): (2, 1, 1, 4, "full"),                 # tile edge ...
    (3, 512): (2, 1, 1, 4, "full"),                 # ... the only shape below 65 536 whose every tile is full
    (3, 513): (2, 2, 1, 8, "full"),                 # ... one live lane in the last tile
    (33, 513): (2, 2, 2, 8, "full"),                # two chunks, uneven 16 / 17
    (50, 4099): (2, 9, 3, 36, "full"),              # three chunks; 36 fold rows: groups 0..3 of the fold add two rows, ragged
    (3, 65535): (2, 128, 1, 512, "full"),           # the PP switch; 16 rows per fold group
    (3, 65536): (4, 64, 1, 256, "full"),            # PP = 4, full tiles only
    (32, 65537): (4, 65, 2, 260, "sampled"),        # PP = 4, two chunks, one live lane in the last (partial) tile; 2.1 M observations
}

# nobs of the single-camera path: blocks, level1
RESIDUAL_SHAPES = {
    1: (1, 1),
    63: (1, 1), 64: (1, 1), 65: (1, 1),             # a wave
    255: (1, 1), 256: (1, 1), 257: (2, 1),          # a workgroup
    2048 * 256: (2048, 1),                          # the one-level fold at its largest
    2048 * 256 + 1: (2049, 2),                      # reduce_rows_kernel: a second chunk of exactly one row
    2048 * 256 + 700 * 256 + 3: (2749, 2),          # ... of 701 rows: 29 fold groups add 22 rows, 3 add 21
}
RESIDUAL_MAX = max(RESIDUAL_SHAPES)
THR2 = 64.0


# ---------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def dense_problem(ncam, npt):
    """K, cams, X of ba_cases.product_problem and obs float32 [ncam, npt, 2]: the projections + 0.5 px of noise."""
    K, cams, X, _, _ = ba_cases.product_problem(ncam, npt)
    rng = np.random.default_rng(5000 * ncam + npt)
    obs = np_ba.project(cams, K, np_ba.as_f64(X)) + rng.normal(0, 0.5, (ncam, npt, 2))
    return K, cams, X, obs.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _residual_pool():
    return ba_problem(1, RESIDUAL_MAX, 4.0, seed=61)


def residual_problem(nobs):
    """K, cams [1, 6], X float32 [nobs, 3], obs float32 [nobs, 2]: the first nobs observations of ONE problem (4 px of noise,
    so thr2 = 64 splits them), which makes every shape a prefix of the larger ones."""
    K, cams, X, obs = _residual_pool()
    return K, cams, X[:nobs], obs[0, :nobs]


@functools.lru_cache(maxsize=None)
def edge_observations(name):
    """K, cams, X of ba_cases.edge_problem / depth_problem and obs float32 [12, 600, 2]: the projections with noise of
    0.5 px + 10 % of |u|.  The relative part keeps the residual u - obs from being a difference of nearly equal numbers
    where u itself is large or badly conditioned (a point 1e6 away near a camera's plane projects to 1e6 px with 1e-13 of
    relative rounding: 1e-7 px, which half a pixel of residual would turn into 2e-7 of J^T r in ANY implementation —
    with the same intent as depth_problem's depths that are not differences)."""
    K, cams, X, _, _ = getattr(ba_cases, name)()
    rng = np.random.default_rng(len(name))
    u = np_ba.project(cams, K, np_ba.as_f64(X))
    obs = u + (0.5 + 0.1 * np.abs(u)) * rng.standard_normal(u.shape)
    return K, cams, X, obs.astype(np.float32)


@functools.lru_cache(maxsize=None)
def indexed_observations():
    """obs float32 [8, 300, 2] for ba_cases.indexed_problem(): 4 px of noise."""
    K, cams, X, _, _ = ba_cases.indexed_problem()
    rng = np.random.default_rng(94)
    return (np_ba.project(cams, K, np_ba.as_f64(X)) + rng.normal(0, 4.0, (8, 300, 2))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def indexed_cases():
    """name -> (cam_idx or None, pt_idx or None, obs [nobs, 2]) on ba_cases.indexed_problem(): its fully indexed lists and
    the two half-indexed forms.  Always in range; pt_idx None keeps nobs <= npt as the C ABI demands."""
    obs = indexed_observations()
    cases = {k: (c, p, obs[c, p]) for k, (c, p) in ba_cases.indexed_cases().items()}
    rng = np.random.default_rng(95)
    pi = rng.integers(0, 300, 777).astype(np.int32)                 # camera 0 in fixed order, gathered points: nobs > npt, repeats
    pi[:40] = 11                                                    # ... forty of one point in one wave
    cases["pt_idx_only"] = (None, pi, obs[0, pi])
    ci = rng.integers(0, 8, 300).astype(np.int32)                   # observation o is of point o, the camera varies
    cases["cam_idx_only"] = (ci, None, obs[ci, np.arange(300)])
    ci = rng.integers(0, 8, 257).astype(np.int32)
    cases["cam_idx_only_257"] = (ci, None, obs[ci, np.arange(257)])
    return cases


def indexed_lists(name):
    """(cam_idx, pt_idx) of a case with the defaults spelt out, as the reference wants them."""
    ci, pi, obs = indexed_cases()[name]
    return (np.zeros(len(obs), np.int32) if ci is None else ci), (np.arange(len(obs), dtype=np.int32) if pi is None else pi)


# ---------------------------------------------------------------- references (float64, built once per shape)
def sample_points(shape):
    pp, tiles, nch, rows, kind = DENSE_SHAPES[shape]
    return None if kind == "full" else ba_cases.sample_points(shape[1], pp, tiles)


@functools.lru_cache(maxsize=None)
def dense_reference(ncam, npt, reverse=False):
    """dict(B, C, gc, gp, res2, sumsq, allow, rows): rows = the point rows C and gp hold (None: all), sumsq the float32
    metric, allow its flip allowance.  reverse=None: a pair of dicts, ascending and descending."""
    K, cams, X, obs = dense_problem(ncam, npt)
    rows = sample_points((ncam, npt))
    res = np_ba.normal_blocks(cams, K, X, obs, want_w=False, pt_block=8192, reverse=reverse, pt_rows=rows)
    u = np_ba.project(cams, K, np_ba.as_f64(X))
    out = []
    for k, rev in enumerate((False, True) if reverse is None else (reverse,)):
        B, C, gc, gp, res2, _ = res[k] if reverse is None else res
        out.append(dict(B=B, C=C, gc=gc, gp=gp, res2=res2, sumsq=np_ba.sumsq(u, obs, rev)[0], allow=np_ba.sumsq_flip_allowance(u, obs), rows=rows))
    return tuple(out) if reverse is None else out[0]


@functools.lru_cache(maxsize=None)
def residual_reference(nobs, reverse=False):
    """dict(B [1, 6, 6], C [nobs, 3, 3], gc, gp, res2, sumsq, allow, u [nobs, 2], inlier, und) of the single-camera path."""
    K, cams, X, obs = residual_problem(nobs)
    res = np_ba.normal_blocks(cams, K, X, obs[None], want_w=False, pt_block=1 << 15, reverse=reverse)
    u = np_ba.project(cams, K, np_ba.as_f64(X))[0]
    inlier, und = np_ba.pnp_inliers(u, obs, THR2)
    out = []
    for k, rev in enumerate((False, True) if reverse is None else (reverse,)):
        B, C, gc, gp, res2, _ = res[k] if reverse is None else res
        out.append(dict(B=B, C=C, gc=gc, gp=gp, res2=res2, sumsq=np_ba.sumsq(u, obs, rev)[0], allow=np_ba.sumsq_flip_allowance(u, obs),
                        u=u, inlier=inlier, und=und))
    return tuple(out) if reverse is None else out[0]


@functools.lru_cache(maxsize=None)
def indexed_reference(name, reverse=False):
    """dict(B, C, gc, gp, res2, sumsq, allow, u, inlier, und) of an indexed case."""
    K, cams, X, _, _ = ba_cases.indexed_problem()
    _, _, obs = indexed_cases()[name]
    ci, pi = indexed_lists(name)
    B, C, gc, gp, res2 = np_ba.indexed_normal_blocks(cams, K, X, obs, ci, pi, reverse=reverse)
    u = np_ba.pair_project(cams, K, X, ci, pi) if len(obs) else np.zeros((0, 2))
    inlier, und = np_ba.pnp_inliers(u, obs, THR2)
    return dict(B=B, C=C, gc=gc, gp=gp, res2=res2, sumsq=np_ba.sumsq(u, obs, reverse)[0], allow=np_ba.sumsq_flip_allowance(u, obs),
                u=u, inlier=inlier, und=und)


@functools.lru_cache(maxsize=None)
def edge_reference(name, reverse=False, magnitude=False):
    """(B, C, gc, gp, res2) of an edge problem, dense; magnitude: the rows' sums of magnitudes."""
    K, cams, X, obs = edge_observations(name)
    return np_ba.normal_blocks(cams, K, X, obs, want_w=False, pt_block=600, reverse=reverse, magnitude=magnitude)[:5]


# ---------------------------------------------------------------- RANSAC scoring
SCORE_H = (1, 5, 64)
SCORE_N = (1, 63, 64, 65, 255, 256, 257, 1000)
SCORE_CASES = [(h, n) for h in SCORE_H for n in SCORE_N] + [(65535, 3)]        # the grid's y limit
ESSENTIAL_THR2 = float(np.float32((0.4 / 1198.0) ** 2))


@functools.lru_cache(maxsize=None)
def pnp_scoring_case(h, n):
    """K, poses [h, 6], X float32 [n, 3], obs float32 [n, 2]: one true pose seen with 4 px of noise; hypothesis m is the true
    pose with 0, 1e-4, 1e-3, 1e-2, 0.1 (cycling) of noise added to its six numbers: the counts run from nearly all to nearly none."""
    rng = np.random.default_rng(100000 + 1000 * (h % 997) + n)
    K, _ = load_pose_csv()
    true = ring_cameras(9)[4]
    X = rng.normal(0, 1, (n, 3))
    X /= np.maximum(1.0, np.linalg.norm(X, axis=1, keepdims=True) / rng.uniform(0.2, 1.0, (n, 1)))
    X = X.astype(np.float32)
    obs = (np_ba.project(true[None], K, np_ba.as_f64(X))[0] + rng.normal(0, 4.0, (n, 2))).astype(np.float32)
    scale = np.array([0, 1e-4, 1e-3, 1e-2, 0.1])[np.arange(h) % 5]
    poses = true + scale[:, None] * rng.standard_normal((h, 6))
    return K, poses, X, obs


@functools.lru_cache(maxsize=None)
def essential_scoring_case(h, n):
    """Es [h, 3, 3], x1n, x2n float64 [n, 2]: a sideways translation, E = [t]x perturbed by 0, 1e-4, 1e-3, 1e-2, 0.1 (cycling)."""
    rng = np.random.default_rng(200000 + 1000 * (h % 997) + n)
    x1 = rng.uniform(-0.4, 0.4, (n, 2))
    x2 = x1 + [0.05, 0.0] + rng.normal(0, 2e-4, (n, 2))
    E = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0.]])
    scale = np.array([0, 1e-4, 1e-3, 1e-2, 0.1])[np.arange(h) % 5]
    return E + scale[:, None, None] * rng.standard_normal((h, 3, 3)), x1, x2


# ---------------------------------------------------------------- planted ties: exact in float32 and in float64
TIE_N = 514


def pnp_tie():
    """K = I, the identity camera, X = (x, y, 1) with x in [0, 8) and y multiples of 1/4: u = x and v = y exactly.  The first
    half of the observations sits at (x + 8, y): ex = 8, err = 64 = thr2 exactly — inliers of `err <= thr2` only.  The
    second half sits at the next float32 above x + 8 (spacing 2^-20 in [8, 16)): ex = 8 + 2^-20 exactly, err =
    float32(64 + 2^-16 + 2^-40) = 64 + 2^-16 > thr2.  Returns K, pose [1, 6], X, obs, the expected mask."""
    half = TIE_N // 2
    k = np.arange(TIE_N)
    x = ((k * 7) % 32) / 4.0
    y = ((k * 5) % 41 - 20) / 4.0
    X = np.stack([x, y, np.ones(TIE_N)], 1).astype(np.float32)
    ox = (x + 8).astype(np.float32)
    ox[half:] = np.nextafter(ox[half:], np.float32(np.inf))
    obs = np.stack([ox, y.astype(np.float32)], 1)
    assert np.all(ox[half:].astype(np.float64) - x[half:] == 8 + 2.0 ** -20)
    return np.eye(3), np.zeros((1, 6)), X, obs, k < half


def essential_tie():
    """E = [t]x for t = (1, 0, 0): E x1 = (0, -1, b1), E^T x2 = (0, 1, -b2), x2^T E x1 = b1 - b2 and the Sampson distance is
    (b1 - b2)^2 / 2.  First half: b1 - b2 = 2^-6, the quotient is 2^-13 = thr2 exactly; second half: b1 - b2 = 2^-6 (1 + 2^-23),
    the quotient rounds to 2^-13 (1 + 2^-22) > thr2.  Every operand is dyadic, every step exact.  Returns E, x1n, x2n, thr2, mask."""
    half = TIE_N // 2
    k = np.arange(TIE_N)
    a1, a2 = ((k * 3) % 17 - 8) / 16.0, ((k * 11) % 23 - 11) / 16.0
    b2 = ((k * 5) % 29 - 14) / 16.0
    d = np.where(k < half, 2.0 ** -6, 2.0 ** -6 * (1 + 2.0 ** -23))
    b1 = b2 + d
    assert np.all(b1 - b2 == d)
    E = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0.]])
    return E[None], np.stack([a1, b1], 1), np.stack([a2, b2], 1), 2.0 ** -13, k < half


# ---------------------------------------------------------------- project_points_f64
PROJECT_N = (1, 255, 256, 257, 100003)


@functools.lru_cache(maxsize=None)
def project_points_input(n):
    """X float64 [n, 3] (NOT float32 values, except the first 600: ba_cases.edge_problem's points, point 0 with z' = 0 at
    camera 0) in the unit ball."""
    X32 = ba_cases.edge_problem()[2].astype(np.float64)
    if n <= len(X32):
        return X32[:n].copy()
    rng = np.random.default_rng(n)
    X = rng.normal(0, 1, (n, 3))
    X /= np.maximum(1.0, np.linalg.norm(X, axis=1, keepdims=True) / rng.uniform(0.2, 1.0, (n, 1)))
    X[:len(X32)] = X32
    return X
