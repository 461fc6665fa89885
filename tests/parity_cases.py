"""Shared pieces of the MVS / mesh limit tests (tests/test_gpu_mvs_limits.py, tests/test_gpu_mesh_limits.py), the end-to-end MVS
tests and the fuzzers (scripts/fuzz_mvs.py, scripts/fuzz_mesh.py): the comparison, the scenes, crops and hand-built inputs, and
one function per entry point that runs the HIP kernel through the C-ABI and the float32 restatement (np_mvs / np_mesh) on the same
host arrays and names the first output that differs.

Comparison: the int32 views of the float32 outputs, with ONE relaxation: where both sides hold a NaN the element counts as equal
whatever its sign and payload (include/sfm_hip.h: unspecified; IEEE 754 leaves the NaN an invalid operation produces to the
implementation: x86 makes 0xFFC00000, the GPU 0x7FC00000).  A NaN against a number differs."""
import functools

import numpy as np

import np_mesh
import np_mvs
from mvs_scenes import gray, render_scene, scene_cloud

F = np.float32
CANONICAL_NAN = np.int32(0x7FC00000)


def host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def bits(t):
    a = np.ascontiguousarray(host(t))
    if a.dtype != np.float32:
        return a
    b = a.view(np.int32).copy()
    b[np.isnan(a)] = CANONICAL_NAN
    return b


def same(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


def up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def first_difference(names, got, want):
    """None, or the name of the first output of `got` that is not `same` as its counterpart."""
    for name, g, w in zip(names, got, want):
        if (g is None) != (w is None) or (g is not None and not same(g, w)):
            return name
    return None


# ---- scenes ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def scene(n=9, w=157, h=93, seed=3, arc=0.3, tex=256):
    """render_scene, cached: (gray frames, K, P, ground-truth depth maps, BGR frames)."""
    imgs, K, P, gt = render_scene(n=n, w=w, h=h, seed=seed, arc=arc, tex=tex)
    return [gray(im) for im in imgs], K, P, gt, imgs


def crop(grays, K, P, x0, y0, w, h):
    """The frames' window [y0, y0+h) x [x0, x0+w) and the cameras that see it: the principal point moves by (-x0, -y0)."""
    T = np.array([[1.0, 0.0, -x0], [0.0, 1.0, -y0], [0.0, 0.0, 1.0]])
    return [np.ascontiguousarray(g[y0:y0 + h, x0:x0 + w]) for g in grays], T @ K, np.stack([T @ p for p in P])


def texture(h, w, seed):
    """A uint8 frame with structure at the scale of a small window: uniform noise, 3 x 3 box-filtered, stretched to 0..255."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.0, 1.0, (h + 2, w + 2))
    b = sum(a[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3))
    b = (b - b.min()) / max(b.max() - b.min(), 1e-9)
    return np.round(255.0 * b).astype(np.uint8)


def rectified_pair(w, h, r, nd, seed):
    """A reference and a source that shows it shifted by an integer disparity along the frame's longer side, M = identity and a
    v that puts that disparity on the middle plane: every warp keeps py = y (or px = x) exactly, so that a frame with a single
    interior row (or column) still has windows that stay inside the source.  A square frame of side 2r+1 leaves no room for a
    shift: v = 0 there (every plane identical).  -> (ref, src, mv [1, 12], invd [nd])."""
    shift = 0 if max(w, h) == 2 * r + 1 else min(3, max(w, h) - (2 * r + 1))
    sx, sy = (shift, 0) if w >= h else (0, shift)
    big = texture(h + sy, w + sx, seed)
    ref = np.ascontiguousarray(big[sy:sy + h, sx:sx + w])          # ref[y, x] = src[y + sy, x + sx]
    src = np.ascontiguousarray(big[0:h, 0:w])
    invd = np.linspace(0.1, 0.5, nd, dtype=np.float64).astype(F)
    q = float(invd[nd // 2])
    mv = np.array([[1, 0, 0, 0, 1, 0, 0, 0, 1, sx / q, sy / q, 0]], F)
    return ref, src, mv, invd


def per_source_costs(ref, srcs, mv, invd, r, var_min):
    """The restatement's per-source costs [nsrc, ndepth, h - 2r, w - 2r]: one sweep per source with topk = 1."""
    with np.errstate(all="ignore"):
        vols = [np_mvs.plane_sweep(ref, [s], np.asarray(mv, F).reshape(-1, 12)[k:k + 1], invd, r, 1, var_min, 2.5)[3] for k, s in enumerate(srcs)]
    return np.stack(vols)[:, :, r:ref.shape[0] - r, r:ref.shape[1] - r]


def interior(a, r):
    return a[..., r:a.shape[-2] - r, r:a.shape[-1] - r]


def h2_of(mv_row, invd, w, h):
    """The warp's third homogeneous coordinate at every pixel, in the header's float32 order."""
    m = np.asarray(mv_row, F)
    ys, xs = np.mgrid[0:h, 0:w]
    with np.errstate(all="ignore"):
        return ((m[6] * xs.astype(F) + m[7] * ys.astype(F)) + m[8]) + m[11] * F(invd)


def plant_specials(a, rng, fraction=0.02, values=(np.nan, np.inf, -np.inf, -1.5, 0.0, -0.0)):
    """A copy of the float32 array with each of `values` written at about `fraction` of its elements."""
    out = np.array(a, F)
    for v in values:
        out[rng.random(out.shape) < fraction] = F(v)
    return out


# ---- one call on both sides --------------------------------------------------------------------------------------------------
def sweep_both(ref, srcs, mv, invd, r, topk, var_min, cost_max):
    """sfm_mvs_plane_sweep and np_mvs.plane_sweep -> (want, name of the first differing output or None)."""
    from sfm_mvs_amd import mvs
    invd = np.ascontiguousarray(invd, F)
    dev = {}
    srcs_dev = [dev.setdefault(id(s), up(s)) for s in srcs]          # a frame passed twice is one device buffer passed twice
    got = mvs.plane_sweep(up(ref), srcs_dev, mv, up(invd), r, topk, var_min, cost_max, plane=True, volume=True)
    with np.errstate(all="ignore"):
        want = np_mvs.plane_sweep(ref, srcs, np.asarray(mv, F).reshape(-1, 12), invd, r, topk, var_min, cost_max)
    return want, first_difference(("depth", "cost", "plane", "volume"), got, want)


def consistency_both(depth, nbr_depths, nbr_index, ab, ref_index, bc, tau, min_consistent, unique):
    from sfm_mvs_amd import mvs
    dev = {}
    nbrs_dev = [dev.setdefault(id(d), up(d)) for d in nbr_depths]
    got = mvs.consistency(up(depth), nbrs_dev, nbr_index, ab, ref_index, bc, tau, min_consistent, unique)
    with np.errstate(all="ignore"):
        want = np_mvs.consistency(depth, nbr_depths, nbr_index, np.asarray(ab, F).reshape(-1, 12), ref_index, bc, tau, min_consistent, unique)
    return want, first_difference(("mask", "xyz"), got, want)


def tsdf_both(depth, P, origin, voxel, dims, trunc, mask=None, bgr=None, S=None, W=None, C=None):
    """sfm_tsdf_integrate and np_mesh.tsdf_integrate from the same starting sums -> (want, first differing output or None)."""
    import torch
    from sfm_mvs_amd import mesh
    depth = np.ascontiguousarray(depth, F)
    P = np.ascontiguousarray(np.asarray(P, F).reshape(-1, 12))
    origin = np.asarray(origin, np.float64).astype(F)
    Pd = up(P) if len(P) else torch.zeros((0, 12), dtype=torch.float32, device="cuda")
    got = mesh.tsdf_integrate(up(depth), Pd, origin, voxel, dims, trunc, masks=None if mask is None else up(mask),
                              bgr=None if bgr is None else up(bgr), S=None if S is None else up(S), W=None if W is None else up(W),
                              C=None if C is None else up(C))
    with np.errstate(all="ignore"):
        want = np_mesh.tsdf_integrate(depth, P, origin, F(voxel), dims, F(trunc), mask=mask, bgr=bgr, S=S, W=W, C=C)
    return want, first_difference(("S", "W", "C"), got, want)


def extract_both(S, W, C, origin, voxel, w_min):
    """sfm_mesh_count + sfm_mesh_extract and np_mesh.extract_mesh -> (want (v, c, f), counts of the device, first difference)."""
    from sfm_mvs_amd import mesh
    S, W = np.ascontiguousarray(S, F), np.ascontiguousarray(W, F)
    origin = np.asarray(origin, np.float64).astype(F)
    Sd, Wd, Cd = up(S), up(W), None if C is None else up(np.ascontiguousarray(C, F))
    counts = tuple(int(v) for v in mesh.mesh_counts(Sd, Wd, w_min).cpu())
    got = mesh.extract_mesh(Sd, Wd, Cd, origin, voxel, w_min)
    with np.errstate(all="ignore"):
        want = np_mesh.extract_mesh(S, W, C, origin, F(voxel), w_min)
    bad = first_difference(("vertices", "colors", "faces"), got, want)
    if bad is None and counts != (len(want[0]), len(want[2])):
        bad = "counts"
    return want, counts, bad


SENTINEL = np.int32(-0x35014542)                   # 0xCAFEBABE: as a float -8355166.0, as a vertex id negative


def extract_with_capacity(S, W, C, origin, voxel, w_min, nv, nt, max_vertices, max_faces, null_outputs=False):
    """sfm_mesh_extract through the C-ABI with capacities below the counts, into buffers of the FULL counted size filled with
    SENTINEL -> (status, vertices [nv, 3] as int32 bits, colors or None, faces [nt, 3]).  null_outputs passes NULL for every
    output whose capacity is 0."""
    import torch
    from sfm_mvs_amd import _lib
    from sfm_mvs_amd.ops import _workspace
    L = _lib.lib()
    S, W = np.ascontiguousarray(S, F), np.ascontiguousarray(W, F)
    nz, ny, nx = S.shape
    Sd, Wd, Cd = up(S), up(W), None if C is None else up(np.ascontiguousarray(C, F))
    dev = Sd.device

    def filled(rows):
        return torch.full((max(rows, 1), 3), int(SENTINEL), dtype=torch.int32, device=dev)

    v, c, f = filled(nv), filled(nv) if C is not None else None, filled(nt)
    ws = _workspace(dev, L.sfm_mesh_extract_ws_bytes(nx, ny, nz))
    org = np.ascontiguousarray(np.asarray(origin, np.float64).astype(F))
    pv = None if (null_outputs and max_vertices == 0) else _lib.ptr(v)
    pc = None if c is None or (null_outputs and max_vertices == 0) else _lib.ptr(c)
    pf = None if (null_outputs and max_faces == 0) else _lib.ptr(f)
    rc = L.sfm_mesh_extract(_lib.ptr(Sd), _lib.ptr(Wd), _lib.ptr(Cd) if pc is not None else None, org.ctypes.data, float(voxel), nx, ny, nz,
                            float(w_min), int(max_vertices), int(max_faces), pv, pc, pf, _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, v[:nv].cpu().numpy(), None if c is None else c[:nv].cpu().numpy(), f[:nt].cpu().numpy()


def capacity_difference(full, part, nv, nt, max_vertices, max_faces, colors_written=True):
    """None, or what is wrong with a capacity-limited extraction `part` against the full result's bits `full` (both (v, c, f) int32):
    the prefix must be the full result's prefix, everything past the capacity the sentinel."""
    for name, a, b, cap, written in (("vertices", full[0], part[0], max_vertices, True), ("colors", full[1], part[1], max_vertices, colors_written),
                                     ("faces", full[2], part[2], max_faces, True)):
        if a is None:
            continue
        cap = min(int(cap), len(a)) if written else 0
        if not np.array_equal(b[:cap], a[:cap]):
            return f"{name}: the first {cap} rows are not the full result's"
        if not np.all(b[cap:] == SENTINEL):
            return f"{name}: {int((b[cap:] != SENTINEL).sum())} elements past capacity {cap} were written"
    return None


# ---- counts that go through no scan ------------------------------------------------------------------------------------------
def counts_by_boolean_arithmetic(S, W, w_min):
    """(crossing edges, triangles) of a field from the header's rule alone: plain NumPy boolean arithmetic over shifted slices, no
    prefix sum, no case table.  A tetrahedron {000, e1, e1+e2, 111} with every corner known has 1 triangle when one or three
    corners are inside, 2 when two are."""
    S, W = np.asarray(S, F), np.asarray(W, F)
    nz, ny, nx = S.shape
    known = W >= F(w_min)
    with np.errstate(all="ignore"):
        inside = known & (np.where(known, S / np.where(known, W, F(1)), F(0)) < F(0))

    def sl(a, dx, dy, dz, span):            # a at (i + dx, j + dy, k + dz) over the points whose `span` offsets stay in the grid
        sx, sy, sz = span
        return a[dz:nz - sz + dz, dy:ny - sy + dy, dx:nx - sx + dx]

    edges = 0
    for m in (1, 2, 4, 3, 5, 6, 7):
        d = (m & 1, m >> 1 & 1, m >> 2)
        a_k, b_k = sl(known, 0, 0, 0, d), sl(known, *d, d)
        edges += int((a_k & b_k & (sl(inside, 0, 0, 0, d) != sl(inside, *d, d))).sum())
    tris = 0
    one = (1, 1, 1)
    for e1, e2, _ in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
        corners = [(0, 0, 0), tuple(int(a == e1) for a in range(3)), tuple(int(a in (e1, e2)) for a in range(3)), (1, 1, 1)]
        allk = np.ones((nz - 1, ny - 1, nx - 1), bool)
        nin = np.zeros((nz - 1, ny - 1, nx - 1), np.int64)
        for c in corners:
            allk &= sl(known, *c, one)
            nin += sl(inside, *c, one)
        tris += int((allk & ((nin == 1) | (nin == 3))).sum()) + 2 * int((allk & (nin == 2)).sum())
    return edges, tris


def dims_with_blocks(nb, rng=None):
    """A grid (nx, ny, nz) whose nx*ny*nz points fill exactly `nb` blocks of 256 with a ragged last block: the largest such n
    (a random one with `rng`) that splits into three factors >= 2, nx nearest its cube root."""
    ns = list(range(nb * 256 - 1, (nb - 1) * 256, -1))
    if rng is not None:
        rng.shuffle(ns)
    for n in ns:
        side = max(2, int(round(n ** (1.0 / 3.0))))
        for nx in sorted(range(2, 3 * side), key=lambda v: abs(v - side)):
            if n % nx:
                continue
            m = n // nx
            root = max(2, int(m ** 0.5))
            for ny in sorted(range(2, 2 * root), key=lambda v: abs(v - root)):
                if m % ny == 0 and m // ny >= 2:
                    return nx, ny, m // ny
    raise ValueError(f"no grid with {nb} blocks found")


def random_field(dims, rng, unknown=0.1, color=True):
    """S, W (and C) of a random field: about `unknown` of the points have W = 0, the others 1..3 observations and a Gaussian F."""
    shape = tuple(dims)[::-1]
    W = np.where(rng.random(shape) < unknown, 0, rng.integers(1, 4, shape)).astype(F)
    S = (rng.standard_normal(shape).astype(F) * W).astype(F)
    C = None
    if color:
        C = np.concatenate([rng.uniform(0, 2000, shape + (3,)), rng.integers(0, 3, shape + (1,))], -1).astype(F)
    return S, W, C


# ---- run_mvs restated --------------------------------------------------------------------------------------------------------
def np_run_mvs(grays, bgrs, K, posearr, Xtot, ndepth, radius, nsrc, topk, var_min, cost_max, tau, min_consistent, unique):
    """run_mvs restated with np_mvs, fed the product's float32 matrices and plane inverse depths (what the kernels got)."""
    from sfm_mvs_amd import mvs
    Ps = np.asarray(posearr)[9:].reshape(-1, 3, 4)
    n = len(Ps)
    nbrs = [mvs.neighbours(i, n, nsrc) for i in range(n)]
    depths = []
    for i in range(n):
        dmin, dmax = mvs.depth_range(Xtot, Ps[i], P_all=Ps)
        invd = mvs._inverse_depths_host(dmin, dmax, ndepth)
        depths.append(np_mvs.plane_sweep(grays[i], [grays[v] for v in nbrs[i]], mvs.sweep_matrices(K, Ps[i], Ps[nbrs[i]]), invd, radius,
                                         topk, var_min, cost_max)[0])
    masks, xyzs = [], []
    for i in range(n):
        ab, bc = mvs.consistency_matrices(K, Ps[i], Ps[nbrs[i]])
        m, x = np_mvs.consistency(depths[i], [depths[v] for v in nbrs[i]], nbrs[i], ab, i, bc, tau, min_consistent, unique)
        masks.append(m)
        xyzs.append(x)
    idx = np.flatnonzero(np.stack(masks).reshape(-1))
    return depths, np.stack(xyzs).reshape(-1, 3)[idx].astype(np.float64), np.stack(bgrs).reshape(-1, 3)[idx].astype(np.float64)
