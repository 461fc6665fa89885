"""Inputs of the two-view glue kernels and the launch plan each lands on, shared by test_tri_cases_cpu.py (which proves on
the CPU that every case lands on the plan claimed for it and that the C oracle alone holds the bars of np_triangulate.py on
these inputs) and test_gpu_tri_paths.py (which holds csrc/triangulate.hip and csrc/assoc.hip to the references).

Reject control of the guarded triangulation (normalise_w = 3): a NaN x-coordinate makes every entry of column 0 .. 3 of the
DLT system NaN, so dlt_nullvec_fast leaves at its first pivot test `!(d0 > 0)` — a certain reject, readable from the code —
and the Jacobi sweeps of the fix-up pass return NaN for the point, as the faithful kernel does.  The reject cases below count
on nothing else, with ONE assumption: on the well-conditioned pairs used for `list_few` and `list_many` the guard's natural
reject share stays below NATURAL_REJECT_MAX = 6 % (docs/geometry.md §4.2 documents 0.7 to 2 %)."""
import functools
import os
import re

import numpy as np

from datagen import gustav_pair, load_pose_csv

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sfm_mvs_amd", "csrc")

# ---------------------------------------------------------------- the launch plan of sfm_triangulate_dlt, restated
LIST_MIN = 1 << 18           # list mode iff n >= 2^18 (and n < INT_MAX)
LIST_SHARE = 8               # cap = n / 8 entries
PASS1_BLOCK = 256
PASS1_GRID_MAX = 256 * 6     # first pass: min(ceil(n / 256), 1536) workgroups, a lane walks i, i + T, ... (T = grid * 256)
WG_QUEUE = 1024              # kQ: rejects a workgroup can queue in LDS
FIX_STEP = 256 * 8           # kFixStep
FIX_CHUNK_MAX = 10 * FIX_STEP
FIX_GRID_MAX = 1024
TM_CHUNK = 1024              # kTmChunk: queries per workgroup of sfm_triangulate_matches_batch
MASK_BLOCK = 1024            # kMaskBlock: rows per workgroup of sfm_mask_indices
PREFIX_STRIDE = 256          # lanes of the prefix loops over block_count
ASSOC_TILE = 1024            # kTile of first_match_kernel
NATURAL_REJECT_MAX = 0.06


def fixup_chunk(n):
    per = (n + 511) // 512
    c = (per + FIX_STEP - 1) // FIX_STEP * FIX_STEP
    return min(max(c, FIX_STEP), FIX_CHUNK_MAX)


def plan(n, spt=2, sxy=1, align1=0, align2=0):
    """dict(list, cap, grid1, per_lane, chunk, grid2, rounds2, packed) of a guarded call; spt / sxy: element strides between
    points / between x and y; align: the base pointers modulo 8."""
    grid1 = min((n + PASS1_BLOCK - 1) // PASS1_BLOCK, PASS1_GRID_MAX)
    chunk = fixup_chunk(n)
    chunks = (n + chunk - 1) // chunk
    grid2 = min(chunks, FIX_GRID_MAX)
    return dict(list=LIST_MIN <= n < 2 ** 31 - 1, cap=n // LIST_SHARE if LIST_MIN <= n < 2 ** 31 - 1 else 0, grid1=grid1,
                per_lane=-(-n // (grid1 * PASS1_BLOCK)) if n else 0, chunk=chunk, grid2=grid2,
                rounds2=-(-chunks // grid2) if n else 0, packed=spt == 2 and sxy == 1 and align1 % 8 == 0 and align2 % 8 == 0)


def workgroup_of(i, n):
    """First-pass workgroup that solves point i."""
    return (np.asarray(i) // PASS1_BLOCK) % plan(n)["grid1"]


def reject_plan(n, planted, natural_max=NATURAL_REJECT_MAX):
    """What the second pass does given the planted (certain) rejects and at most natural_max * n further ones anywhere:
    'list' (every reject on the compact list, whatever the natural ones do), 'scan' (certain overflow, by the planted points
    alone) or 'open' (it depends on the natural rejects).  Also the reason: 'wg' / 'cap' / None."""
    p = plan(n)
    if not p["list"]:
        return "scan", None
    planted = np.asarray(planted, np.int64)
    per_wg = np.bincount(workgroup_of(planted, n), minlength=p["grid1"]) if len(planted) else np.zeros(p["grid1"], np.int64)
    if per_wg.max() > WG_QUEUE:
        return "scan", "wg"
    if len(planted) > p["cap"]:
        return "scan", "cap"
    lanes = PASS1_BLOCK * p["per_lane"]                     # points a workgroup walks at the most
    worst_wg = np.minimum(lanes, per_wg + int(np.ceil(natural_max * n))).max()
    if worst_wg <= WG_QUEUE and len(planted) + int(np.ceil(natural_max * n)) <= p["cap"]:
        return "list", None
    return "open", None


def source_constants():
    """The same constants as csrc/triangulate.hip and csrc/assoc.hip state them."""
    with open(os.path.join(CSRC, "triangulate.hip")) as f:
        t = f.read()
    with open(os.path.join(CSRC, "assoc.hip")) as f:
        a = f.read()
    g = lambda pat, text=t: [int(v) for v in re.search(pat, text).groups()]
    step = g(r"constexpr int kFixStep = (\d+) \* (\d+), kFixChunkMax = (\d+) \* kFixStep;")
    grid1 = g(r"const dim3 pgrid\(\(unsigned\)std::min<int64_t>\(\(n \+ 255\) / 256, (\d+) \* (\d+)\)\);")
    return dict(LIST_MIN=1 << g(r"normalise_w == 3 && n >= \(1 << (\d+)\) && n < INT_MAX")[0],
                LIST_SHARE=g(r"cap = \(int\)\(n / (\d+)\);")[0], PASS1_GRID_MAX=grid1[0] * grid1[1],
                WG_QUEUE=g(r"constexpr int kQ = (\d+);")[0], FIX_STEP=step[0] * step[1], FIX_CHUNK_MAX=step[2] * step[0] * step[1],
                FIX_GRID_MAX=g(r"std::min<int64_t>\(\(n \+ chunk - 1\) / chunk, (\d+)\)\), dim3\(256\), sizeof\(unsigned short\)")[0],
                TM_CHUNK=g(r"constexpr int kTmChunk = (\d+);")[0], MASK_BLOCK=g(r"constexpr int kMaskBlock = (\d+);", a)[0],
                ASSOC_TILE=g(r"constexpr int kTile = (\d+);", a)[0])


# ---------------------------------------------------------------- sizes
SIZES_SMALL = (1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097, LIST_MIN - 1)
SIZES_LIST = (LIST_MIN,
              PASS1_GRID_MAX * PASS1_BLOCK + 1,      # 393 217: the first n at which a lane walks two points (the prefetch of nx runs)
              400_003)
POOL = LIST_MIN - 1

# ---------------------------------------------------------------- layouts of the (2, N) arguments
# name -> the first pass instantiation it must land on (True: PACKED float2 reader) for n >= 2
LAYOUTS = {
    "transposed": True,      # (N, 2).t(): the reference's own call (sfm.py:47-48)
    "contiguous": False,     # (2, N)
    "wide": False,           # (N, 3)[:, :2].t()
    "offset4": False,        # packed strides on a base pointer 4 bytes off 8-byte alignment: must fall to the strided kernel
    "mixed": False,          # pts1 transposed, pts2 contiguous: the wrapper makes both contiguous
}


def layout_views(name, x1, x2, device="cpu"):
    """The two (2, N) float32 torch views of layout `name` holding x1, x2 (NumPy (N, 2) float32)."""
    import torch
    a, b = (torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(device) for x in (x1, x2))
    n = a.shape[0]
    if name == "transposed":
        return a.t(), b.t()
    if name == "contiguous":
        return a.t().contiguous().reshape(2, n), b.t().contiguous().reshape(2, n)
    if name == "wide":
        wide = lambda t: torch.cat([t, torch.full((n, 1), 7.0, dtype=t.dtype, device=t.device)], 1)[:, :2].t()
        return wide(a), wide(b)
    if name == "offset4":
        def off(t):
            buf = torch.empty(2 * n + 1, dtype=t.dtype, device=t.device)
            buf[1:] = t.reshape(-1)
            return buf[1:].view(n, 2).t()
        return off(a), off(b)
    if name == "mixed":
        return a.t(), b.t().contiguous().reshape(2, n)
    raise KeyError(name)


def wrapper_strides(p1, p2):
    """(spt, sxy, align1, align2) as ops.triangulate hands them to sfm_triangulate_dlt."""
    if p2.stride() != p1.stride():
        p1, p2 = p1.contiguous(), p2.contiguous()
    return p1.stride(1), p1.stride(0), p1.data_ptr() % 8, p2.data_ptr() % 8


# ---------------------------------------------------------------- geometries
# name -> does the DLT system have ONE null vector (a float64 reference exists)?
GEOMETRIES = {"gustav0": True, "gustav03": True, "gustav3": True, "baseline": True, "same": False}
_GUSTAV = {"gustav0": (0, 0.0), "gustav03": (1, 0.3), "gustav3": (30, 3.0)}


def baseline_cameras():
    """pose.csv camera 1 and a copy moved by 1e-3 along its x axis (1e-4 of the depths): ill-conditioned null vectors."""
    _, P = load_pose_csv()
    P2 = P[1].copy()
    P2[:, 3] += P[1][:, :3] @ np.array([1e-3, 0.0, 0.0])
    return P[1], P2


@functools.lru_cache(maxsize=None)
def _pool(geometry, n):
    if geometry in _GUSTAV:
        k, sigma = _GUSTAV[geometry]
        _, P1, P2, _, x1, x2 = gustav_pair(k, n, sigma, seed=300 + k)
        return P1, P2, x1, x2
    rng = np.random.default_rng(77)
    P1, P2 = baseline_cameras()
    X = np.stack([rng.uniform(-6.3, 3.6, n), rng.uniform(-2.6, 5.0, n), rng.uniform(3.2, 13.0, n), np.ones(n)], 0)
    xs = []
    for P in (P1, P2):
        x = P @ X
        xs.append(((x[:2] / x[2]).T + rng.normal(0, 0.3, (n, 2))).astype(np.float32))
    if geometry == "baseline":
        return P1, P2, xs[0], xs[1]
    if geometry == "same":                                   # identical cameras AND identical rays: a 2-D null space
        return P1, P1, xs[0], xs[0]
    raise KeyError(geometry)


def pair(geometry, n):
    """(P1, P2, x1, x2): the first n correspondences of the geometry's pool (x: (n, 2) float32).  'gustav03' has the full pool
    of 2^18 - 1, the others 4097: the larger sizes run on 'gustav03' only."""
    size = POOL if geometry == "gustav03" else 4097
    assert n <= size
    P1, P2, x1, x2 = _pool(geometry, size)
    return P1, P2, x1[:n], x2[:n]


def geometries_of(n):
    return tuple(GEOMETRIES) if n <= 4097 else ("gustav03",)


# ---------------------------------------------------------------- reject cases
def planted_rejects(n, which):
    """Indices whose x-coordinate is set to NaN (ascending)."""
    if which == "none":
        return np.zeros(0, np.int64)
    if which == "sixteenth":                                 # n / 16, spread evenly
        return np.arange(n // 16, dtype=np.int64) * 16 + 5
    if which == "eighth_plus_one":                           # n / 8 + 1: one more than the global list holds
        idx = np.arange(n // 8 + 1, dtype=np.int64) * 7 + 3
        assert idx[-1] < n
        return idx
    if which == "workgroup0":                                # every point workgroup 0 walks
        i = np.arange(n, dtype=np.int64)
        return i[workgroup_of(i, n) == 0]
    raise KeyError(which)


# name -> (n, planted, geometry, second-pass plan it must land on, reason)
REJECT_CASES = {
    "list_few": (400_003, "none", "gustav03", "list", None),
    "list_many": (LIST_MIN, "sixteenth", "gustav03", "list", None),
    "cap_overflow": (LIST_MIN, "eighth_plus_one", "gustav03", "scan", "cap"),
    "wg_overflow": (4 * PASS1_GRID_MAX * PASS1_BLOCK + 256, "workgroup0", "gustav03", "scan", "wg"),
}
# all rejected: P2 == P1 and x2 == x1 (rank 2: the inverse iteration has no vector to converge to), so every workgroup's
# queue overflows (13 656 points each) and the scan pass walks 1025 chunks of 20 480 on 1024 workgroups: a second round
FIXUP_TWO_ROUNDS_N = FIX_GRID_MAX * FIX_CHUNK_MAX + 4097


def device_pair(n, seed, device, geometry="gustav03"):
    """n correspondences built on the device: points uniform in the sparse.ply bounding box seen by pose.csv cameras 1 and 2
    (the one-million test's scene), 0.3 px of noise.  Returns (P1, P2, x1, x2) with x: (n, 2) float32 device tensors."""
    import torch
    assert geometry == "gustav03"
    _, P = load_pose_csv()
    g = torch.Generator(device=device).manual_seed(seed)
    lo = torch.tensor([-6.3, -2.6, 3.2], dtype=torch.float64, device=device)
    hi = torch.tensor([3.6, 5.0, 13.0], dtype=torch.float64, device=device)
    X = lo + (hi - lo) * torch.rand((n, 3), dtype=torch.float64, device=device, generator=g)
    Xh = torch.cat([X, torch.ones((n, 1), dtype=torch.float64, device=device)], 1)
    out = []
    for Pm in (P[1], P[2]):
        x = Xh @ torch.from_numpy(Pm).to(device).t()
        noise = 0.3 * torch.randn((n, 2), dtype=torch.float64, device=device, generator=g)
        out.append((x[:, :2] / x[:, 2:] + noise).float().contiguous())
    return P[1], P[2], out[0], out[1]


# ---------------------------------------------------------------- the guard's empirical bound
GUARD_SWEEP_SIGMAS = (0.0, 0.3, 3.0)
GUARD_SWEEP_N = 4096


def guard_sweep_pair(k, sigma):
    """Consecutive pose.csv pair (k, k + 1), k in 0 .. 55, fixed seed."""
    _, P1, P2, _, x1, x2 = gustav_pair(k, GUARD_SWEEP_N, sigma, seed=9000 + 10 * k + int(round(sigma * 10)))
    return P1, P2, x1, x2


# ---------------------------------------------------------------- cheirality vote
POSE_N = (0, 1, 63, 64, 65, 255, 256, 257, 1000)
POSE_DIST = 50.0


def decompose_essential(E):
    """The four candidates [R1|t], [R2|t], [R1|-t], [R2|-t] (OpenCV's order) of an essential matrix, [4, 3, 4]."""
    U, _, Vt = np.linalg.svd(E)
    if np.linalg.det(U) < 0:
        U = -U
    if np.linalg.det(Vt) < 0:
        Vt = -Vt
    W = np.array([[0.0, 1, 0], [-1, 0, 0], [0, 0, 1]])
    R1, R2, t = U @ W @ Vt, U @ W.T @ Vt, U[:, 2]
    return np.stack([np.hstack([R, s * t[:, None]]) for R, s in ((R1, 1), (R2, 1), (R1, -1), (R2, -1))])


@functools.lru_cache(maxsize=None)
def pose_case():
    """(cands [4, 3, 4], x1n, x2n (1000, 2) float64, kind, depth in camera 1, depth in camera 2) of a planted pose (|t| = 1): K-normalised correspondences of points at
    depth 2 .. 20 (1e-4 of noise), at depth 45 .. 55 (both sides of dist = 50, in either camera), behind camera 1, behind
    camera 2 and nearly at infinity (depth 1e3 .. 1e6: Q3 near 0, rays parallel to 1e-3 .. 1e-6), shuffled so that every
    prefix holds every kind."""
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(41)
    R = Rotation.from_rotvec([0.05, -0.2, 0.03]).as_matrix()
    t = np.array([0.9, 0.1, -0.2])
    t /= np.linalg.norm(t)
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    cands = decompose_essential(tx @ R)
    n = 1000
    kind = rng.permutation(np.repeat(np.arange(5), [600, 150, 80, 80, 90]))
    d = rng.normal(0, 0.3, (n, 2))
    depth = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4],
                      [rng.uniform(2, 20, n), rng.uniform(45, 55, n), -rng.uniform(2, 20, n), rng.uniform(0.05, 0.15, n),
                       10.0 ** rng.uniform(3, 6, n)])
    X = np.c_[d * depth[:, None], depth]
    X2 = X @ R.T + t                                         # (kind 3: depth 0.05 .. 0.15 in camera 1 is behind camera 2, t_z = -0.22)
    x1n = X[:, :2] / X[:, 2:]
    x2n = X2[:, :2] / X2[:, 2:]
    noise = np.where((kind == 0)[:, None], rng.normal(0, 1e-4, (n, 2)), 0.0)
    return cands, x1n, x2n + noise, kind, X[:, 2].copy(), X2[:, 2].copy()
