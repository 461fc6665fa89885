"""A surface from the MVS depth maps: TSDF fusion and a watertight mesh by marching tetrahedra (the step sfm-mvs tools take after
the dense cloud; the reference's `camera_orientation` writes triangle meshes with open3d).

Thin, validating wrappers over `sfm_tsdf_integrate`, `sfm_mesh_count` and `sfm_mesh_extract` (include/sfm_hip.h, "MESH"): device
tensors in, device tensors out, stream ordered, no CPU path.  The host part is the choice of the volume from the fused cloud
(float64) and the cast of the cameras' projection matrices.  docs/mesh.md describes the algorithm and its numbers.
Opt-in after the extraction: `mesh_components` / `clean_mesh` (sfm_mesh_components, sfm_mesh_clean; "MESH-CLEAN") drop the small
connected components, `run_mesh(clean=True)` (docs/mesh.md §7); `smooth_mesh` / `mesh_normals` (sfm_mesh_smooth, sfm_mesh_normals;
"MESH-FINISH") smooth the surface and give it vertex normals, `run_mesh(smooth=..., normals=True)` (docs/mesh.md §8);
`decimate_mesh` (sfm_mesh_decimate; "MESH-DECIMATE") simplifies it by vertex clustering, `run_mesh(decimate=...)` (docs/mesh.md §9);
`render_depth`, `face_views`, `texture_fill` / `texture_mesh` (sfm_mesh_render_depth, sfm_mesh_face_views, sfm_mesh_texture_fill;
"MESH-TEXTURE") give it a texture atlas from the photographs, `run_mesh(texture=True)` (docs/mesh.md §10).
"""
import numpy as np
import torch

from . import _lib
from ._lib import SfmHipError, check, on_device, ptr, require_cuda, stream_ptr
from .mvs import _upload

MAX_POINTS = 1 << 27            # lattice points per grid

# Defaults of run_mesh, chosen on the CPU model (tests/np_mesh.py) over the rendered scenes of tests/mvs_scenes.py
# (docs/mesh.md, "Calibration").
TRUNC_VOXELS = 2.0              # truncation distance in voxels
W_MIN = 3.0                     # observations a lattice point needs to be known

# Clean-up (include/sfm_hip.h, "MESH-CLEAN"; docs/mesh.md §7).
COMPONENT_ROUNDS = 24           # labelling rounds enqueued per call: twice the most any measured mesh needed (docs/mesh.md §7)
MIN_COMPONENT_SHARE = 1.0 / 512 # run_mesh(clean=True) drops components with fewer faces than this share of all faces

# Finishing (include/sfm_hip.h, "MESH-FINISH"; docs/mesh.md §8).
SMOOTH_LAMBDA, SMOOTH_MU = 0.5, -0.53   # Taubin's pair: the pass band ends at 1/lambda + 1/mu = 0.113
MAX_SMOOTH_STEPS = 32           # pairs: sfm_mesh_smooth takes 64 steps
SMOOTH_PAIRS = 10               # the pair count the calibration recommends (docs/mesh.md §8); run_mesh's own default stays 0

# Decimation (include/sfm_hip.h, "MESH-DECIMATE"; docs/mesh.md §9).
MAX_CELLS = 1 << 27             # cells per clustering grid
DECIMATE_CELLS = 2.0            # the cell size in voxels the calibration recommends (docs/mesh.md §9); run_mesh's own default stays 0

# Texturing (include/sfm_hip.h, "MESH-TEXTURE"; docs/mesh.md §10).
ATLAS_TEXELS = 8                # texels per triangle leg: the atlas of k faces has a side of about sqrt(k / 2) * 13
MAX_ATLAS_TEXELS = 64
MAX_ATLAS_SIDE = 16384
VIS_TOL = 0.02                  # relative depth tolerance of the visibility test, calibrated (scripts/calibrate_mesh_texture.py)


def volume_bounds(points, resolution=256, pad=0.05):
    """The grid of a fused cloud: per axis the 1st / 99th percentiles of `points` ((m, 3), host float64), widened by `pad` times
    the longest extent on each side; voxel = longest padded extent / (resolution - 1).
    Returns (origin float64 (3,), voxel float, dims (nx, ny, nz)) with max(dims) == resolution.  Raises SfmHipError on a cloud
    with fewer than 4 finite points or no extent, and when the grid would exceed 2^27 lattice points."""
    X = np.asarray(points, np.float64).reshape(-1, 3)
    X = X[np.all(np.isfinite(X), axis=1)]
    resolution = int(resolution)
    if resolution < 2:
        raise SfmHipError(f"volume_bounds: resolution {resolution} < 2")
    if not (0.0 <= pad < np.inf):
        raise SfmHipError(f"volume_bounds: pad {pad} must be finite and >= 0")
    if len(X) < 4:
        raise SfmHipError(f"volume_bounds: {len(X)} finite points: too few for a volume")
    lo, hi = np.percentile(X, 1, axis=0), np.percentile(X, 99, axis=0)
    ext = hi - lo
    longest = float(ext.max())
    if not longest > 0.0:
        raise SfmHipError("volume_bounds: the cloud has no extent (all points coincide)")
    lo, hi = lo - pad * longest, hi + pad * longest
    ext = hi - lo
    voxel = float(ext.max()) / (resolution - 1)
    dims = tuple(int(max(2, min(resolution, int(np.ceil(e / voxel - 1e-9)) + 1))) for e in ext)
    if int(np.prod(dims, dtype=np.int64)) > MAX_POINTS:
        raise SfmHipError(f"volume_bounds: {dims[0]} x {dims[1]} x {dims[2]} grid exceeds 2^27 lattice points; lower the resolution")
    return lo, voxel, dims


def projection_rows(K, Ps):
    """float32 [n, 12] = K[R|t] row-major per camera: sfm.py:423's posearr stores P = K[R|t] itself (formed in float64, cast once)."""
    return np.ascontiguousarray(np.asarray(Ps, np.float64).reshape(-1, 12)).astype(np.float32)


def _origin(origin):
    return np.ascontiguousarray(np.asarray(origin, np.float64).reshape(3).astype(np.float32))


def tsdf_integrate(depths, P, origin, voxel, dims, trunc, masks=None, bgr=None, S=None, W=None, C=None):
    """Fold views into the TSDF sums (sfm_tsdf_integrate).
    depths [n, H, W] float32 device tensor; P float32 [n, 12] (host array: uploaded through pinned memory; or a device tensor);
    masks optional [n, H, W] uint8; bgr optional [n, H, W, 3] uint8; origin (3,), voxel, dims (nx, ny, nz), trunc (world units).
    S, W [nz, ny, nx] float32 and C [nz, ny, nx, 4] float32 continue earlier sums (zeros when None; the colour sums C are kept
    exactly when bgr is given).  Returns (S, W, C or None), updated in place when given."""
    require_cuda(depths, masks, bgr, S, W, C)
    nx, ny, nz = (int(d) for d in dims)
    if depths.dtype != torch.float32 or depths.dim() != 3:
        raise SfmHipError("tsdf_integrate: depths must be an [n, H, W] float32 device tensor")
    depths = depths.contiguous()
    n, h, w = depths.shape
    dev = depths.device
    if masks is not None and (masks.dtype != torch.uint8 or tuple(masks.shape) != (n, h, w)):
        raise SfmHipError("tsdf_integrate: masks must be [n, H, W] uint8 like the depths")
    if bgr is not None and (bgr.dtype != torch.uint8 or tuple(bgr.shape) != (n, h, w, 3)):
        raise SfmHipError("tsdf_integrate: bgr must be [n, H, W, 3] uint8 like the depths")
    if torch.is_tensor(P):
        require_cuda(P)
        Pd = P.to(dev, torch.float32).contiguous().reshape(-1, 12)
    else:
        Pd = _upload(np.ascontiguousarray(np.asarray(P, np.float32).reshape(-1, 12)), dev)
    if Pd.shape[0] != n:
        raise SfmHipError(f"tsdf_integrate: {n} depth maps but {Pd.shape[0]} projection matrices")
    if S is None:
        S = torch.zeros((nz, ny, nx), dtype=torch.float32, device=dev)
    if W is None:
        W = torch.zeros((nz, ny, nx), dtype=torch.float32, device=dev)
    if C is None and bgr is not None:
        C = torch.zeros((nz, ny, nx, 4), dtype=torch.float32, device=dev)
    for t, shape in ((S, (nz, ny, nx)), (W, (nz, ny, nx))) + (((C, (nz, ny, nx, 4)),) if C is not None else ()):
        if t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev:
            raise SfmHipError(f"tsdf_integrate: sums must be contiguous float32 {shape} on the depths' device")
    if (C is None) != (bgr is None):
        raise SfmHipError("tsdf_integrate: colour sums C go with bgr")
    org = _origin(origin)
    with on_device(dev):
        check(_lib.lib().sfm_tsdf_integrate(ptr(depths), ptr(None if masks is None else masks.contiguous()),
                                            ptr(None if C is None else bgr.contiguous()), ptr(Pd), n, w, h, org.ctypes.data, float(voxel),
                                            nx, ny, nz, float(trunc), ptr(S), ptr(W), ptr(C), stream_ptr()), "sfm_tsdf_integrate")
    return S, W, C


def _field(S, W, C):
    require_cuda(S, W, C)
    if S.dtype != torch.float32 or W.dtype != torch.float32 or S.dim() != 3 or S.shape != W.shape:
        raise SfmHipError("mesh: S and W must be [nz, ny, nx] float32 device tensors of one shape")
    nz, ny, nx = S.shape
    if C is not None and (C.dtype != torch.float32 or tuple(C.shape) != (nz, ny, nx, 4)):
        raise SfmHipError("mesh: C must be [nz, ny, nx, 4] float32")
    return S.contiguous(), W.contiguous(), None if C is None else C.contiguous(), (nx, ny, nz)


def mesh_counts(S, W, w_min=W_MIN):
    """sfm_mesh_count: an int32 [2] device tensor (vertices, triangles); no host wait."""
    from .ops import _workspace
    S, W, _, (nx, ny, nz) = _field(S, W, None)
    L = _lib.lib()
    out = torch.empty(2, dtype=torch.int32, device=S.device)
    ws = _workspace(S.device, L.sfm_mesh_count_ws_bytes(nx, ny, nz))
    with on_device(S.device):
        check(L.sfm_mesh_count(ptr(S), ptr(W), nx, ny, nz, float(w_min), ptr(out), ptr(ws), ws.numel(), stream_ptr()), "sfm_mesh_count")
    return out


def extract_mesh(S, W, C, origin, voxel, w_min=W_MIN, packed=False):
    """Marching tetrahedra over the field (sfm_mesh_count, one host read of the two totals, sfm_mesh_extract).
    Returns device tensors (vertices [m, 3] float32, colors [m, 3] float32 B G R or None (C None), faces [k, 3] int32).
    packed=True: also the one int32 buffer all three live in, so that a caller downloads them with a single copy."""
    from .ops import _workspace
    S, W, C, (nx, ny, nz) = _field(S, W, C)
    nv, nt = (int(v) for v in mesh_counts(S, W, w_min).cpu())        # the host wait: the totals size the outputs
    dev = S.device
    ncol = nv if C is not None else 0
    buf = torch.empty(3 * nv + 3 * ncol + 3 * nt, dtype=torch.int32, device=dev)
    verts = buf[:3 * nv].view(torch.float32).view(nv, 3)
    cols = buf[3 * nv:3 * (nv + ncol)].view(torch.float32).view(ncol, 3) if C is not None else None
    faces = buf[3 * (nv + ncol):].view(nt, 3)
    L = _lib.lib()
    ws = _workspace(dev, L.sfm_mesh_extract_ws_bytes(nx, ny, nz))
    org = _origin(origin)
    with on_device(dev):
        check(L.sfm_mesh_extract(ptr(S), ptr(W), ptr(C), org.ctypes.data, float(voxel), nx, ny, nz, float(w_min), nv, nt,
                                 ptr(verts) if nv else None, ptr(cols) if ncol else None, ptr(faces) if nt else None, ptr(ws), ws.numel(),
                                 stream_ptr()), "sfm_mesh_extract")
    return (verts, cols, faces, buf) if packed else (verts, cols, faces)


def _faces(faces, what):
    require_cuda(faces)
    if faces.dtype != torch.int32 or faces.dim() != 2 or faces.shape[1] != 3:
        raise SfmHipError(f"{what}: faces must be a [k, 3] int32 device tensor")
    return faces.contiguous()


def mesh_components(faces, nv, rounds=COMPONENT_ROUNDS, labels=None, status=None):
    """sfm_mesh_components: label[v] = the smallest vertex id of v's connected component, at most `rounds` (1..1024) rounds.
    faces [k, 3] int32 device tensor (indices outside 0..nv-1 make a face invalid: it joins nothing); labels: an int32 [nv] device
    tensor an earlier call left, to continue from (updated in place).  Returns (labels, status): status an int32 [2] device tensor
    (converged 0/1, rounds that lowered a label; written into `status` when given).  No host wait."""
    from .ops import _workspace
    faces = _faces(faces, "mesh_components")
    nv, nf, dev = int(nv), int(faces.shape[0]), faces.device
    resume = labels is not None
    if resume:
        require_cuda(labels)
        if labels.dtype != torch.int32 or tuple(labels.shape) != (nv,) or not labels.is_contiguous() or labels.device != dev:
            raise SfmHipError("mesh_components: labels must be a contiguous int32 [nv] tensor on the faces' device")
    else:
        labels = torch.empty(max(nv, 0), dtype=torch.int32, device=dev)
    if status is None:
        status = torch.empty(2, dtype=torch.int32, device=dev)
    L = _lib.lib()
    ws = _workspace(dev, L.sfm_mesh_components_ws_bytes(max(nv, 0), nf))
    with on_device(dev):
        check(L.sfm_mesh_components(ptr(faces) if nf else None, nv, nf, int(rounds), int(resume), ptr(labels) if nv > 0 else None, ptr(status),
                                    ptr(ws), ws.numel(), stream_ptr()), "sfm_mesh_components")
    return labels, status


def clean_mesh(vertices, colors, faces, min_faces=1, largest_only=False, packed=False, rounds=COMPONENT_ROUNDS, labels=None):
    """Drop the small connected components of a mesh (sfm_mesh_components, then sfm_mesh_clean); no host wait.
    vertices [m, 3] float32, colors [m, 3] float32 or None, faces [k, 3] int32: device tensors.  Component c is kept iff it has at
    least `min_faces` faces (0 keeps everything, 1 drops the vertices no face names); largest_only keeps only the component with
    the most faces (ties: the lowest vertex id), if it passes min_faces.  labels: labels an earlier call left, to continue from.
    Returns (vertices, colors or None, faces, counts): tensors of the INPUT sizes of which the first counts[0] / counts[1] rows are
    the result (kept vertices in their order, rows bit for bit; kept faces in their order, renumbered) and the rest is not
    written; counts an int32 [4] device tensor (vertices kept, faces kept, components, components kept).  The counts are
    meaningful once the labelling has converged (status[0] == 1; otherwise call again with labels=labels).
    packed=True: returns (vertices, colors, faces, counts, status, labels, buf) with buf the one int32 buffer that holds counts [4],
    status [2], vertices, colours and faces in that order, so that a caller downloads once and slices on the host."""
    from .ops import _workspace
    require_cuda(vertices, colors)
    faces = _faces(faces, "clean_mesh")
    if vertices.dtype != torch.float32 or vertices.dim() != 2 or vertices.shape[1] != 3:
        raise SfmHipError("clean_mesh: vertices must be an [m, 3] float32 device tensor")
    if colors is not None and (colors.dtype != torch.float32 or colors.shape != vertices.shape):
        raise SfmHipError("clean_mesh: colors must be [m, 3] float32 like the vertices")
    vertices = vertices.contiguous()
    colors = None if colors is None else colors.contiguous()
    nv, nf, dev = int(vertices.shape[0]), int(faces.shape[0]), vertices.device
    ncol = nv if colors is not None else 0
    buf = torch.empty(6 + 3 * nv + 3 * ncol + 3 * nf, dtype=torch.int32, device=dev)
    counts, status = buf[:4], buf[4:6]
    out_v = buf[6:6 + 3 * nv].view(torch.float32).view(nv, 3)
    out_c = buf[6 + 3 * nv:6 + 3 * (nv + ncol)].view(torch.float32).view(ncol, 3) if colors is not None else None
    out_f = buf[6 + 3 * (nv + ncol):].view(nf, 3)
    labels, _ = mesh_components(faces, nv, rounds, labels, status=status)
    L = _lib.lib()
    ws = _workspace(dev, L.sfm_mesh_clean_ws_bytes(nv, nf))
    with on_device(dev):
        check(L.sfm_mesh_clean(ptr(vertices) if nv else None, ptr(colors) if ncol else None, ptr(faces) if nf else None, nv, nf,
                               ptr(labels) if nv else None, int(min_faces), int(bool(largest_only)), ptr(out_v) if nv else None,
                               ptr(out_c) if ncol else None, ptr(out_f) if nf else None, ptr(counts), ptr(ws), ws.numel(), stream_ptr()),
              "sfm_mesh_clean")
    return (out_v, out_c, out_f, counts, status, labels, buf) if packed else (out_v, out_c, out_f, counts)


def _finish_args(vertices, faces, counts, what):
    require_cuda(vertices, counts)
    faces = _faces(faces, what)
    if vertices.dtype != torch.float32 or vertices.dim() != 2 or vertices.shape[1] != 3:
        raise SfmHipError(f"{what}: vertices must be an [m, 3] float32 device tensor")
    if faces.device != vertices.device:
        raise SfmHipError(f"{what}: vertices and faces must live on one device")
    if counts is not None and (counts.dtype != torch.int32 or counts.dim() != 1 or counts.numel() < 2 or not counts.is_contiguous()
                               or counts.device != vertices.device):
        raise SfmHipError(f"{what}: counts must be a contiguous int32 device tensor that starts with (vertices, faces)")
    return vertices.contiguous(), faces


def mesh_normals(vertices, faces, counts=None, out=None):
    """Vertex normals (sfm_mesh_normals): the normalised equal-weight sum of the unit normals of the faces at each vertex, outward
    by extract_mesh's winding; (0, 0, 0) at a vertex no face with an area names.  vertices [m, 3] float32, faces [k, 3] int32
    device tensors; counts: an int32 device tensor whose first two words are the numbers of rows in use (clean_mesh's counts),
    read on the device.  Returns an [m, 3] float32 device tensor (written into `out` when given) of which the counted rows are
    written.  No host wait; the words do not depend on the order of the faces."""
    from .ops import _workspace
    vertices, faces = _finish_args(vertices, faces, counts, "mesh_normals")
    nv, nf, dev = int(vertices.shape[0]), int(faces.shape[0]), vertices.device
    if out is None:
        out = torch.empty((nv, 3), dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or tuple(out.shape) != (nv, 3) or not out.is_contiguous() or out.device != dev:
        raise SfmHipError("mesh_normals: out must be a contiguous [m, 3] float32 tensor on the vertices' device")
    L = _lib.lib()
    ws = _workspace(dev, L.sfm_mesh_normals_ws_bytes(nv, nf))
    with on_device(dev):
        check(L.sfm_mesh_normals(ptr(vertices) if nv else None, ptr(faces) if nf else None, nv, nf, ptr(counts), ptr(out) if nv else None,
                                 ptr(ws), ws.numel(), stream_ptr()), "sfm_mesh_normals")
    return out


def smooth_scale(extent):
    """pscale of smooth_mesh: the largest power of two with extent * pscale <= 2^29 (positions are quantised to 1 / pscale; the
    factor 2 of head-room up to the 2^30 a usable vertex may reach keeps vertices that drift slightly outside the frame usable)."""
    extent = float(extent)
    if not (np.isfinite(extent) and extent > 0.0):
        raise SfmHipError(f"smooth_mesh: extent {extent} must be finite and positive")
    e = int(np.floor(np.log2(2.0 ** 29 / extent)))
    while extent * 2.0 ** (e + 1) <= 2.0 ** 29:
        e += 1
    while extent * 2.0 ** e > 2.0 ** 29:
        e -= 1
    return float(2.0 ** min(max(e, -126), 127))


def smooth_mesh(vertices, faces, steps, origin, extent, lam=SMOOTH_LAMBDA, mu=SMOOTH_MU, counts=None, out=None):
    """Taubin smoothing (sfm_mesh_smooth): `steps` (0..32) PAIRS of face-umbrella Laplacian steps with the factors lam, mu, lam,
    mu, ...  Positions are quantised relative to `origin` ((3,), the frame's corner) at the largest power-of-two scale that fits
    `extent` (its longest side) into 2^29; a vertex further than twice the extent from the origin, or not finite, neither moves nor
    pulls its neighbours.  counts as in mesh_normals.  Returns an [m, 3] float32 device tensor (`out` when given) of which the
    counted rows are written.  No host wait; the words do not depend on the order of the faces."""
    from .ops import _workspace
    vertices, faces = _finish_args(vertices, faces, counts, "smooth_mesh")
    steps = int(steps)
    if not 0 <= steps <= MAX_SMOOTH_STEPS:
        raise SfmHipError(f"smooth_mesh: steps {steps} must be in 0..{MAX_SMOOTH_STEPS}")
    nv, nf, dev = int(vertices.shape[0]), int(faces.shape[0]), vertices.device
    if out is None:
        out = torch.empty((nv, 3), dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or tuple(out.shape) != (nv, 3) or not out.is_contiguous() or out.device != dev:
        raise SfmHipError("smooth_mesh: out must be a contiguous [m, 3] float32 tensor on the vertices' device")
    factors = np.ascontiguousarray(np.tile(np.array([lam, mu], np.float32), steps))
    org = _origin(origin)
    L = _lib.lib()
    ws = _workspace(dev, L.sfm_mesh_smooth_ws_bytes(nv, nf))
    with on_device(dev):
        check(L.sfm_mesh_smooth(ptr(vertices) if nv else None, ptr(faces) if nf else None, nv, nf, ptr(counts), 2 * steps,
                                factors.ctypes.data if steps else None, org.ctypes.data, smooth_scale(extent), ptr(out) if nv else None,
                                ptr(ws), ws.numel(), stream_ptr()), "sfm_mesh_smooth")
    return out


def decimate_mesh(vertices, colors, faces, origin, cell, dims, extent, dedupe=True, counts=None, packed=False):
    """Vertex clustering (sfm_mesh_decimate): the vertices of one cell of the grid (`origin` (3,) its corner, `cell` the cell's
    side, `dims` (nx, ny, nz) cells, at most 2^27) become one vertex at the mean of their positions (quantised as in smooth_mesh,
    `extent` the frame's longest side) and of their colours; faces are renumbered, the ones left with fewer than three different
    corners are dropped, and with `dedupe` so are all but the first of the faces that became equal up to a rotation.  A vertex
    outside the grid, or not finite, is unusable: it and its faces go.  vertices [m, 3] float32, colors [m, 3] float32 or None,
    faces [k, 3] int32 device tensors; counts as in mesh_normals.
    Returns (vertices, colors or None, faces, counts): tensors of the INPUT sizes of which the first counts[0] / counts[1] rows are
    the result and the rest is not written; counts an int32 [4] device tensor (vertices out, faces out, unusable vertices, live
    faces dropped as duplicates) whose first two words mesh_normals takes as its counts.  No host wait; the words do not depend
    on the order in which anything lands.
    packed=True: returns (vertices, colors, faces, counts, buf) with buf the one int32 buffer that holds counts [4], vertices,
    colours and faces in that order, so that a caller downloads once and slices on the host."""
    from .ops import _workspace
    vertices, faces = _finish_args(vertices, faces, counts, "decimate_mesh")
    require_cuda(colors)
    if colors is not None and (colors.dtype != torch.float32 or colors.shape != vertices.shape or colors.device != vertices.device):
        raise SfmHipError("decimate_mesh: colors must be [m, 3] float32 like the vertices")
    colors = None if colors is None else colors.contiguous()
    d = np.ascontiguousarray(np.asarray(dims, np.int64).reshape(3))
    if np.any(d < 1) or int(d[0]) * int(d[1]) * int(d[2]) > MAX_CELLS:
        raise SfmHipError(f"decimate_mesh: {d[0]} x {d[1]} x {d[2]} cells: each must be >= 1 and the product <= 2^27")
    d = np.ascontiguousarray(d.astype(np.int32))
    nv, nf, dev = int(vertices.shape[0]), int(faces.shape[0]), vertices.device
    ncol = nv if colors is not None else 0
    buf = torch.empty(4 + 3 * nv + 3 * ncol + 3 * nf, dtype=torch.int32, device=dev)
    out_n = buf[:4]
    out_v = buf[4:4 + 3 * nv].view(torch.float32).view(nv, 3)
    out_c = buf[4 + 3 * nv:4 + 3 * (nv + ncol)].view(torch.float32).view(ncol, 3) if colors is not None else None
    out_f = buf[4 + 3 * (nv + ncol):].view(nf, 3)
    org = _origin(origin)
    L = _lib.lib()
    ws = _workspace(dev, L.sfm_mesh_decimate_ws_bytes(nv, nf, d.ctypes.data))
    with on_device(dev):
        check(L.sfm_mesh_decimate(ptr(vertices) if nv else None, ptr(colors) if ncol else None, ptr(faces) if nf else None, nv, nf,
                                  ptr(counts), org.ctypes.data, float(cell), d.ctypes.data, smooth_scale(extent), int(bool(dedupe)),
                                  ptr(out_v) if nv else None, ptr(out_c) if ncol else None, ptr(out_f) if nf else None, ptr(out_n),
                                  ptr(ws), ws.numel(), stream_ptr()), "sfm_mesh_decimate")
    return (out_v, out_c, out_f, out_n, buf) if packed else (out_v, out_c, out_f, out_n)


def _layout(nf, texels):
    nf, L = int(nf), int(texels)
    if not 1 <= L <= MAX_ATLAS_TEXELS:
        raise SfmHipError(f"atlas_layout: texels {texels} must be in 1..{MAX_ATLAS_TEXELS}")
    if nf < 0:
        raise SfmHipError(f"atlas_layout: {nf} faces")
    slots = (nf + 1) // 2
    cols = int(np.sqrt(float(slots)))
    while cols * cols < slots:
        cols += 1
    while cols > 1 and (cols - 1) * (cols - 1) >= slots:
        cols -= 1
    cols, cell = max(cols, 1), L + 5
    if cols * cell > MAX_ATLAS_SIDE:
        raise SfmHipError(f"atlas_layout: {nf} faces at {L} texels need a side of {cols * cell} > {MAX_ATLAS_SIDE}; lower texels or decimate")
    return cols * cell, cols, cell


def atlas_layout(nf, texels=ATLAS_TEXELS):
    """The atlas of `nf` faces at `texels` (1..64) texels per triangle leg (include/sfm_hip.h, "MESH-TEXTURE"): every face owns half
    of a square cell of texels + 5 texels a side, the cells fill a square of cols x cols row by row.
    Returns (side, cols, cell, uv): uv (nf, 3, 2) float64, the texture coordinates ((ox + i + 0.5) / side, 1 - (oy + j + 0.5) / side)
    of the three corners of every face (v up, as OBJ has it).  Host only.  Raises SfmHipError when texels is out of range or the
    side would exceed 16384."""
    side, cols, cell = _layout(nf, texels)
    nf, L = int(nf), int(texels)
    f = np.arange(nf)
    q, half = f >> 1, (f & 1)[:, None]
    ox, oy = ((q % cols) * cell)[:, None], ((q // cols) * cell)[:, None]
    ci = np.where(half == 0, np.array([1, 1 + L, 1]), np.array([cell - 2, cell - 2 - L, cell - 2]))
    cj = np.where(half == 0, np.array([1, 1, 1 + L]), np.array([cell - 2, cell - 2, cell - 2 - L]))
    uv = np.stack([(ox + ci + 0.5) / side, 1.0 - (oy + cj + 0.5) / side], -1).reshape(nf, 3, 2)
    return side, cols, cell, uv


def _view_rows(P, dev, what):
    if torch.is_tensor(P):
        require_cuda(P)
        Pd = P.to(dev, torch.float32).contiguous().reshape(-1, 12)
    else:
        Pd = _upload(np.ascontiguousarray(np.asarray(P, np.float32).reshape(-1, 12)), dev)
    if Pd.shape[0] < 1:
        raise SfmHipError(f"{what}: needs at least one view")
    return Pd


def render_depth(vertices, faces, P, w, h, counts=None, out=None):
    """A depth map of the mesh in every view (sfm_mesh_render_depth): per pixel the smallest camera depth of the faces that cover
    its centre, +inf where none does; both orientations are drawn and nothing is clipped at the near plane.  vertices [m, 3]
    float32, faces [k, 3] int32 device tensors; P float32 [n, 12] (projection_rows: a host array, uploaded through pinned memory, or
    a device tensor); counts as in mesh_normals.  Returns an [n, h, w] float32 device tensor (`out` when given).  No host wait; the
    words do not depend on the order in which anything lands."""
    vertices, faces = _finish_args(vertices, faces, counts, "render_depth")
    dev = vertices.device
    Pd = _view_rows(P, dev, "render_depth")
    n, w, h = int(Pd.shape[0]), int(w), int(h)
    if w < 2 or h < 2 or w * h > (1 << 26):
        raise SfmHipError(f"render_depth: frame {w} x {h}: w and h must be >= 2 and w * h <= 2^26")
    if out is None:
        out = torch.empty((n, h, w), dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or tuple(out.shape) != (n, h, w) or not out.is_contiguous() or out.device != dev:
        raise SfmHipError("render_depth: out must be a contiguous [n, h, w] float32 tensor on the vertices' device")
    nv, nf = int(vertices.shape[0]), int(faces.shape[0])
    with on_device(dev):
        check(_lib.lib().sfm_mesh_render_depth(ptr(vertices) if nv else None, ptr(faces) if nf else None, nv, nf, ptr(counts), ptr(Pd), n, w, h,
                                               ptr(out), stream_ptr()), "sfm_mesh_render_depth")
    return out


def face_views(vertices, faces, P, zbuf, vis_tol=VIS_TOL, counts=None):
    """The view every face is textured from (sfm_mesh_face_views): among the views in which the face lies in the frame, faces the
    camera (negative screen area) and is visible in render_depth's `zbuf` [n, h, w] at its corners and its centroid within the
    relative tolerance `vis_tol`, the one in which it is largest (the lowest index on ties).  Returns (face_view int32 [k], -1
    where there is none; face_score float32 [k], the screen area doubled) device tensors of which the counted rows are written.
    No host wait."""
    vertices, faces = _finish_args(vertices, faces, counts, "face_views")
    dev = vertices.device
    Pd = _view_rows(P, dev, "face_views")
    require_cuda(zbuf)
    if zbuf.dtype != torch.float32 or zbuf.dim() != 3 or zbuf.shape[0] != Pd.shape[0] or not zbuf.is_contiguous() or zbuf.device != dev:
        raise SfmHipError("face_views: zbuf must be render_depth's contiguous [n, h, w] float32 tensor for the same views")
    vis_tol = float(vis_tol)
    if not (np.isfinite(vis_tol) and vis_tol >= 0.0):
        raise SfmHipError(f"face_views: vis_tol {vis_tol} must be finite and >= 0")
    n, h, w = (int(d) for d in zbuf.shape)
    nv, nf = int(vertices.shape[0]), int(faces.shape[0])
    view = torch.empty(nf, dtype=torch.int32, device=dev)
    score = torch.empty(nf, dtype=torch.float32, device=dev)
    with on_device(dev):
        check(_lib.lib().sfm_mesh_face_views(ptr(vertices) if nv else None, ptr(faces) if nf else None, nv, nf, ptr(counts), ptr(Pd), n, w, h,
                                             ptr(zbuf), vis_tol, ptr(view) if nf else None, ptr(score) if nf else None, stream_ptr()),
              "sfm_mesh_face_views")
    return view, score


def texture_fill(vertices, colors, faces, P, frames, face_view, texels=ATLAS_TEXELS, counts=None, out=None):
    """The atlas (sfm_mesh_texture_fill): every texel of atlas_layout(k, texels) is the bilinear sample of frame face_view[f] at the
    projection of the texel's point on its face f; faces without a view interpolate the vertex `colors` ([m, 3] float32 B G R, or
    None: 0).  frames [n, h, w, 3] uint8 B G R, face_view int32 [k]: device tensors.  Returns a [side, side, 3] uint8 device
    tensor (`out` when given, every texel written).  No host wait."""
    vertices, faces = _finish_args(vertices, faces, counts, "texture_fill")
    dev = vertices.device
    require_cuda(colors, frames, face_view)
    if colors is not None and (colors.dtype != torch.float32 or colors.shape != vertices.shape or colors.device != dev):
        raise SfmHipError("texture_fill: colors must be [m, 3] float32 like the vertices")
    colors = None if colors is None else colors.contiguous()
    Pd = _view_rows(P, dev, "texture_fill")
    n = int(Pd.shape[0])
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[0] != n or frames.shape[3] != 3 or frames.device != dev:
        raise SfmHipError("texture_fill: frames must be an [n, h, w, 3] uint8 device tensor, one frame per view")
    frames = frames.contiguous()
    h, w = int(frames.shape[1]), int(frames.shape[2])
    nv, nf = int(vertices.shape[0]), int(faces.shape[0])
    if face_view.dtype != torch.int32 or tuple(face_view.shape) != (nf,) or not face_view.is_contiguous() or face_view.device != dev:
        raise SfmHipError("texture_fill: face_view must be a contiguous int32 [k] tensor on the vertices' device")
    side, cols, _ = _layout(nf, texels)
    if out is None:
        out = torch.empty((side, side, 3), dtype=torch.uint8, device=dev)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (side, side, 3) or not out.is_contiguous() or out.device != dev:
        raise SfmHipError(f"texture_fill: out must be a contiguous [{side}, {side}, 3] uint8 tensor on the vertices' device")
    with on_device(dev):
        check(_lib.lib().sfm_mesh_texture_fill(ptr(vertices) if nv else None, ptr(colors), ptr(faces) if nf else None, nv, nf, ptr(counts),
                                               ptr(Pd), ptr(frames), n, w, h, ptr(face_view) if nf else None, int(texels), cols, side, ptr(out),
                                               stream_ptr()), "sfm_mesh_texture_fill")
    return out


def _frames_tensor(images, dev, what):
    if torch.is_tensor(images):
        frames = images.to(dev)
    elif all(torch.is_tensor(im) and im.is_cuda for im in images):
        frames = torch.stack([im.to(dev) for im in images])
    else:
        host = [im.cpu().numpy() if torch.is_tensor(im) else np.asarray(im) for im in images]
        if any(im.shape != host[0].shape or im.dtype != np.uint8 for im in host):
            raise SfmHipError(f"{what}: frames must be (H, W, 3) uint8 BGR of one size")
        frames = _upload(np.stack(host), dev)
    if frames.dim() != 4 or frames.shape[3] != 3 or frames.dtype != torch.uint8:
        raise SfmHipError(f"{what}: frames must be (H, W, 3) uint8 BGR of one size")
    return frames.contiguous()


def _device_rows(a, integer, dev):
    """[m, 3] float32 (int32 when `integer`) on the device: a device tensor as it is, a host array through pinned memory."""
    if torch.is_tensor(a):
        require_cuda(a)
        return a.to(dev, torch.int32 if integer else torch.float32).contiguous()
    return _upload(np.ascontiguousarray(np.asarray(a).reshape(-1, 3).astype(np.int32 if integer else np.float32)), dev)


def texture_mesh(vertices, colors, faces, images, K, Ps, texels=ATLAS_TEXELS, vis_tol=VIS_TOL):
    """A texture atlas for a mesh from its photographs: render_depth, face_views and texture_fill enqueued one after another, then
    ONE download (the atlas and the faces' views in one buffer): the only host wait.
    vertices (m, 3), colors (m, 3) B G R or None, faces (k, 3): host arrays (uploaded through pinned memory on the stream) or
    device tensors; images: n BGR uint8 frames of one size (host arrays, device tensors, or one [n, h, w, 3] device tensor);
    K (3, 3), Ps (n, 3, 4) = K [R|t] per camera in the images' order (what posearr stores: projection_rows).
    Returns dict(atlas (side, side, 3) uint8 B G R, uv (k, 3, 2) float64 (atlas_layout), face_view int32 (k,), -1 where no view
    shows the face (its chart interpolates the vertex colours), textured: the faces with a view)."""
    dev = next((t.device for t in (vertices, faces) if torch.is_tensor(t) and t.is_cuda), None)
    if dev is None:
        dev = next((im.device for im in ([images] if torch.is_tensor(images) else images) if torch.is_tensor(im) and im.is_cuda),
                   torch.device("cuda", torch.cuda.current_device()))
    rows = projection_rows(K, Ps)
    with torch.cuda.device(dev):
        v, f = _device_rows(vertices, False, dev), _device_rows(faces, True, dev)
        c = None if colors is None else _device_rows(colors, False, dev)
        frames = _frames_tensor(images, dev, "texture_mesh")
        return _texture(v, c, f, frames, _upload(rows, dev), texels, vis_tol)


def _texture(v, c, f, frames, Pd, texels, vis_tol):
    """texture_mesh on device tensors."""
    if Pd.shape[0] != frames.shape[0]:
        raise SfmHipError(f"texture_mesh: {frames.shape[0]} frames for {Pd.shape[0]} cameras")
    nf, dev = int(f.shape[0]), v.device
    side, cols, cell, uv = atlas_layout(nf, texels)
    head = (4 * nf + 255) // 256 * 256
    buf = torch.empty(head + 3 * side * side, dtype=torch.uint8, device=dev)
    view = buf[:4 * nf].view(torch.int32)
    zbuf = render_depth(v, f, Pd, int(frames.shape[2]), int(frames.shape[1]))
    got, _ = face_views(v, f, Pd, zbuf, vis_tol)
    view.copy_(got)
    texture_fill(v, c, f, Pd, frames, view, texels, out=buf[head:].view(side, side, 3))
    host = buf.cpu().numpy()                                        # the one download
    fv = np.ascontiguousarray(host[:4 * nf]).view(np.int32)
    return dict(atlas=np.ascontiguousarray(host[head:].reshape(side, side, 3)), uv=uv, face_view=fv, textured=int((fv >= 0).sum()))


def decimate_frame(origin, voxel, dims, decimate):
    """run_mesh's clustering grid for a volume (origin (3,) float64, voxel, dims) and a cell of `decimate` voxels: (origin float64
    (3,), cell, dims, extent).  The grid starts one cell below the volume's origin and has floor((dims_c - 1) * voxel / cell) + 3
    cells per axis, so that vertices smoothing pushed slightly outside the volume stay usable; extent, the side the quantisation
    is scaled to, is the longest side of this padded grid.  Raises SfmHipError when `decimate` is not a finite number >= 1 or the
    grid exceeds 2^27 cells."""
    decimate = float(decimate)
    if not (np.isfinite(decimate) and decimate >= 1.0):
        raise SfmHipError(f"run_mesh: decimate {decimate} must be 0 (off) or a finite cell size >= 1 voxel")
    cell = decimate * float(voxel)
    cells = tuple(int(np.floor((int(n) - 1) * float(voxel) / cell)) + 3 for n in dims)
    if int(np.prod(cells, dtype=np.int64)) > MAX_CELLS:
        raise SfmHipError(f"run_mesh: the decimation grid {cells[0]} x {cells[1]} x {cells[2]} exceeds 2^27 cells; raise decimate")
    return np.asarray(origin, np.float64).reshape(3) - cell, cell, cells, cell * max(cells)


def run_mesh(images, K, posearr, mvs_out, resolution=256, trunc_voxels=TRUNC_VOXELS, w_min=W_MIN, tau=0.01, min_consistent=2, nsrc=4,
             pad=0.05, clean=False, min_component_share=MIN_COMPONENT_SHARE, min_component_faces=None, largest_only=False, normals=False,
             smooth=0, smooth_lambda=SMOOTH_LAMBDA, smooth_mu=SMOOTH_MU, decimate=0, decimate_dedupe=True, texture=False,
             texture_texels=ATLAS_TEXELS, texture_vis_tol=VIS_TOL):
    """A coloured triangle mesh of a registered sequence from run_mvs's depth maps.

    images:  the BGR uint8 frames run_mvs got (device tensors or host arrays, K's resolution, posearr's camera order)
    mvs_out: run_mvs's result: its per-view depth maps and its fused cloud (which fixes the volume: volume_bounds)
    Per view a consistency mask (mvs.consistency with unique=False: every pixel >= `min_consistent` of its `nsrc` sequence
    neighbours agree with, within `tau`), then one sfm_tsdf_integrate over all views (truncation `trunc_voxels` voxels),
    marching tetrahedra over the points seen `w_min` times.  Defaults: docs/mesh.md, "Calibration".
    clean=True: then the connected components with fewer than `min_component_faces` faces are dropped (clean_mesh; None:
    max(1, floor(min_component_share * faces)); largest_only: all but the largest), and the dict gains `components` and
    `components_kept`.
    smooth > 0: then that many Taubin pairs (smooth_mesh with `smooth_lambda`, `smooth_mu`, the volume's origin and its longest
    side as the frame) move the vertices; normals=True: then the dict gains `normals` (m, 3) float64, the vertex normals of the
    final surface (mesh_normals).  Both are off by default (docs/mesh.md §8) and add no host wait.
    decimate > 0: then, after the clean-up and the smoothing and before the normals, the vertices of every cell of `decimate`
    (>= 1, a float) voxels become one (decimate_mesh over decimate_frame's grid; `decimate_dedupe`: faces that became equal are
    output once); vertices, colors, faces and normals then describe the decimated mesh, and the dict gains `decimated_from`
    (vertices, faces) before the step and `decimate_unusable`, the vertices that fell outside the grid.  Off by default
    (DECIMATE_CELLS is the recommended cell, docs/mesh.md §9); no host wait is added and the rows before the step are not downloaded.
    texture=True: then, after the download, the final surface (after the clean-up, the smoothing and the decimation) gets a texture
    atlas from the frames, which are already on the device (texture_mesh's three steps at `texture_texels` texels per triangle
    leg and the visibility tolerance `texture_vis_tol`; the final rows go back up through pinned memory on the stream), and the
    dict gains `atlas` (side, side, 3) uint8 B G R, `uv` (k, 3, 2) float64 and `face_view` int32 (k,) for pipeline.to_obj_mesh.
    Off by default (docs/mesh.md §10); on, it adds exactly one host wait: the download of the atlas.
    Returns dict(vertices (m, 3) float64, colors (m, 3) float64 B G R, faces (k, 3) int32) for pipeline.to_ply_mesh.
    Two host waits per call: the mesh totals and the one download; every upload is stream-ordered (pinned memory).  (Should the
    downloaded labelling status say "not converged" the labelling is continued, and cleaned and downloaded again, until it has.)"""
    from . import mvs
    K = np.asarray(K, np.float64).reshape(3, 3)
    Ps = np.asarray(posearr, np.float64)[9:].reshape(-1, 3, 4)
    n = len(Ps)
    depths = list(mvs_out["depths"])
    if len(images) != n or len(depths) != n:
        raise SfmHipError(f"run_mesh: {len(images)} frames and {len(depths)} depth maps for {n} cameras")
    if n < 2:
        raise SfmHipError("run_mesh: needs at least two registered views")
    origin, voxel, dims = volume_bounds(mvs_out["points"], resolution, pad)
    finish = None
    if int(smooth) != 0 or normals:
        if not 0 <= int(smooth) <= MAX_SMOOTH_STEPS:
            raise SfmHipError(f"run_mesh: smooth {smooth} must be in 0..{MAX_SMOOTH_STEPS} pairs")
        finish = dict(steps=int(smooth), lam=float(smooth_lambda), mu=float(smooth_mu), normals=bool(normals), origin=origin,
                      extent=voxel * (max(dims) - 1))
    dec = None
    if decimate != 0:
        dec = dict(frame=decimate_frame(origin, voxel, dims, decimate), dedupe=bool(decimate_dedupe))
    if texture:
        _layout(0, texture_texels)                                  # the range of texels, before any work
        if not (np.isfinite(float(texture_vis_tol)) and float(texture_vis_tol) >= 0.0):
            raise SfmHipError(f"run_mesh: texture_vis_tol {texture_vis_tol} must be finite and >= 0")
    dev = depths[0].device
    require_cuda(*depths)
    if all(torch.is_tensor(im) and im.is_cuda for im in images):
        frames = torch.stack([im.to(dev) for im in images]).contiguous()
    else:
        host = [im.cpu().numpy() if torch.is_tensor(im) else np.asarray(im) for im in images]
        if any(im.shape != host[0].shape or im.dtype != np.uint8 for im in host):
            raise SfmHipError("run_mesh: frames must be (H, W, 3) uint8 BGR of one size")
        frames = _upload(np.stack(host), dev)
    h, w = depths[0].shape
    if frames.dim() != 4 or tuple(frames.shape[1:]) != (h, w, 3) or frames.dtype != torch.uint8:
        raise SfmHipError("run_mesh: frames must be (H, W, 3) uint8 BGR at the depth maps' size")
    nsrc = min(int(nsrc), n - 1, mvs.MAX_VIEWS)
    masks = torch.empty((n, h, w), dtype=torch.uint8, device=dev)
    xyz = torch.empty((n, h, w, 3), dtype=torch.float32, device=dev)
    rows = projection_rows(K, Ps)

    def textured(out):
        """run_mesh's dict, with the atlas of its surface when texture is on (enqueued after the download, one more download)."""
        if not texture:
            return out
        with torch.cuda.device(dev):
            v, c, f = _device_rows(out["vertices"], False, dev), _device_rows(out["colors"], False, dev), _device_rows(out["faces"], True, dev)
            tex = _texture(v, c, f, frames, _upload(rows, dev), texture_texels, texture_vis_tol)
        out.update(atlas=tex["atlas"], uv=tex["uv"], face_view=tex["face_view"])
        return out

    with torch.cuda.device(dev):
        for i in range(n):
            nb = mvs.neighbours(i, n, nsrc)
            ab, bc = mvs.consistency_matrices(K, Ps[i], Ps[nb])
            mvs.consistency(depths[i], [depths[v] for v in nb], nb, ab, i, bc, tau, min(int(min_consistent), len(nb)), False,
                            mask_out=masks[i], xyz_out=xyz[i])
        S, W, C = tsdf_integrate(torch.stack(depths), rows, origin, voxel, dims, float(trunc_voxels) * voxel,
                                 masks=masks, bgr=frames)
        verts, cols, faces, buf = extract_mesh(S, W, C, origin, voxel, w_min, packed=True)
        if clean:
            return textured(_clean_and_download(verts, cols, faces, min_component_share, min_component_faces, largest_only, finish, dec))
        if dec is not None:
            parts = _decimate(verts, cols, faces, None, finish, dec)
            host = (torch.cat(parts) if len(parts) > 1 else parts[0]).cpu().numpy()     # the one download
            return textured(_decimated_rows(host, len(verts), len(faces), (len(verts), len(faces)), finish))
        if finish is not None:
            buf = torch.cat([buf] + _finish(verts, faces, None, finish))
        host = buf.cpu().numpy()                                    # the one download
    nv, nt = len(verts), len(faces)
    fl = host[:6 * nv].view(np.float32)
    out = dict(vertices=fl[:3 * nv].reshape(nv, 3).astype(np.float64), colors=fl[3 * nv:].reshape(nv, 3).astype(np.float64),
               faces=np.ascontiguousarray(host[6 * nv:6 * nv + 3 * nt].reshape(nt, 3)))
    if finish is not None:
        out.update(_finished_rows(host[6 * nv + 3 * nt:], nv, nv, finish))
    return textured(out)


def _finish(verts, faces, counts, finish):
    """The finishing steps run_mesh asked for, enqueued: the flat int32 views of the smoothed vertices (when smoothing) and of the
    normals (when asked), each of the vertices' full size, to be appended to the buffer that is downloaded."""
    extra = []
    if finish["steps"]:
        verts = smooth_mesh(verts, faces, finish["steps"], finish["origin"], finish["extent"], finish["lam"], finish["mu"], counts)
        extra.append(verts.view(torch.int32).reshape(-1))
    if finish["normals"]:
        extra.append(mesh_normals(verts, faces, counts).view(torch.int32).reshape(-1))
    return extra


def _finished_rows(tail, cap, nv, finish):
    """What _finish appended, sliced from the downloaded words: dict(vertices?, normals?) with the first nv of the cap rows each."""
    out, fl = {}, tail.view(np.float32)
    if finish["steps"]:
        out["vertices"] = fl[:3 * nv].reshape(nv, 3).astype(np.float64)
        fl = fl[3 * cap:]
    if finish["normals"]:
        out["normals"] = fl[:3 * nv].reshape(nv, 3).astype(np.float64)
    return out


def _decimate(verts, cols, faces, counts, finish, dec):
    """run_mesh's steps after the clean-up when decimate is on, enqueued: the smoothing (when asked), the clustering, the normals of
    the decimated surface (when asked, read through the clustering's counts on the device).  Returns the flat int32 tensors to
    download: decimate_mesh's packed buffer and the normals, each of the input's full size."""
    if finish is not None and finish["steps"]:
        verts = smooth_mesh(verts, faces, finish["steps"], finish["origin"], finish["extent"], finish["lam"], finish["mu"], counts)
    origin, cell, cells, extent = dec["frame"]
    dv, _, df, dn, buf = decimate_mesh(verts, cols, faces, origin, cell, cells, extent, dec["dedupe"], counts, packed=True)
    parts = [buf]
    if finish is not None and finish["normals"]:
        parts.append(mesh_normals(dv, df, dn).view(torch.int32).reshape(-1))
    return parts


def _decimated_rows(words, nv_cap, nf_cap, before, finish):
    """What _decimate left, sliced from the downloaded words: run_mesh's dict of the decimated mesh."""
    kv, kf, unusable = (int(v) for v in words[:3])
    fl = words[4:4 + 6 * nv_cap].view(np.float32)
    out = dict(vertices=fl[:3 * kv].reshape(kv, 3).astype(np.float64), colors=fl[3 * nv_cap:3 * (nv_cap + kv)].reshape(kv, 3).astype(np.float64),
               faces=np.ascontiguousarray(words[4 + 6 * nv_cap:4 + 6 * nv_cap + 3 * kf].reshape(kf, 3)),
               decimated_from=(int(before[0]), int(before[1])), decimate_unusable=unusable)
    if finish is not None and finish["normals"]:
        tail = words[4 + 6 * nv_cap + 3 * nf_cap:].view(np.float32)
        out["normals"] = tail[:3 * kv].reshape(kv, 3).astype(np.float64)
    return out


def _clean_and_download(verts, cols, faces, min_component_share, min_component_faces, largest_only, finish=None, dec=None):
    """run_mesh's tail with clean=True: the cleaned mesh (smoothed, decimated, with normals: `finish`, `dec`) in one download."""
    nv, nt = len(verts), len(faces)
    if min_component_faces is None:
        if not (0.0 <= float(min_component_share) <= 1.0):
            raise SfmHipError(f"run_mesh: min_component_share {min_component_share} must lie in 0..1")
        min_faces = max(1, int(np.floor(float(min_component_share) * nt)))
    else:
        min_faces = int(min_component_faces)
        if min_faces < 0:
            raise SfmHipError(f"run_mesh: min_component_faces {min_faces} is negative")
    labels = None
    while True:
        ov, oc, of, counts, _, labels, buf = clean_mesh(verts, cols, faces, min_faces, largest_only, packed=True, labels=labels)
        if dec is not None:                                         # counts and status, then the decimated mesh alone
            buf = torch.cat([buf[:6]] + _decimate(ov, oc, of, counts, finish, dec))
        elif finish is not None:                                    # on the counted rows, the counts read on the device
            buf = torch.cat([buf] + _finish(ov, of, counts, finish))
        host = buf.cpu().numpy()                                    # the one download
        if host[4]:                                                 # converged; otherwise every batch of rounds lowers a label
            break
    kv, kf, ncomp, nkept = (int(v) for v in host[:4])
    if dec is not None:
        out = _decimated_rows(host[6:], nv, nt, (kv, kf), finish)
        out.update(components=ncomp, components_kept=nkept)
        return out
    fl = host[6:6 + 6 * nv].view(np.float32)
    out = dict(vertices=fl[:3 * kv].reshape(kv, 3).astype(np.float64), colors=fl[3 * nv:3 * (nv + kv)].reshape(kv, 3).astype(np.float64),
               faces=np.ascontiguousarray(host[6 + 6 * nv:6 + 6 * nv + 3 * kf].reshape(kf, 3)), components=ncomp, components_kept=nkept)
    if finish is not None:
        out.update(_finished_rows(host[6 + 6 * nv + 3 * nt:], nv, kv, finish))
    return out
