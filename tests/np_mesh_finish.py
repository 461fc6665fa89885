"""NumPy restatement of the mesh finishing step (include/sfm_hip.h, "MESH-FINISH"; docs/mesh.md §8), written from the header and
importing nothing of the product: vertex normals as the normalised int64 sum of quantised unit face normals, and Taubin smoothing
as face-umbrella Laplacian steps over int64 sums of quantised positions.  float32 operations are NumPy float32 operations in the
header's order, sums are np.add.at on int64, so the GPU tests compare int32 views exactly."""
import numpy as np

UNIT = np.float32(2.0 ** 30)


def resolve_counts(counts, nv_cap, nf_cap):
    """(nv, nf): the capacities, or the given pair where it lies in 0..capacity."""
    if counts is None:
        return int(nv_cap), int(nf_cap)
    nv, nf = int(counts[0]), int(counts[1])
    return (nv if 0 <= nv <= nv_cap else int(nv_cap)), (nf if 0 <= nf <= nf_cap else int(nf_cap))


def _mesh(vertices, faces, counts):
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    nv, nf = resolve_counts(counts, len(v), len(f))
    f = f[:nf]
    return v[:nv], f[np.all((f >= 0) & (f < nv), axis=1)]


def face_terms(v, f):
    """(q int64 [k, 3], contributes bool [k]) of the valid faces f over the float32 rows v."""
    with np.errstate(all="ignore"):
        a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
        e1, e2 = b - a, c - a
        nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        ln = np.sqrt((nx * nx + ny * ny) + nz * nz)
        assert ln.dtype == np.float32
        good = np.isfinite(ln) & (ln > 0)
        safe = np.where(good, ln, np.float32(1.0))
        q = np.stack([np.rint((n / safe) * UNIT) for n in (nx, ny, nz)], 1)
        q = np.where(good[:, None], q, np.float32(0.0)).astype(np.int64)
    return q, good


def normal_sums(vertices, faces, counts=None):
    """int64 [nv, 3]: the accumulators."""
    v, f = _mesh(vertices, faces, counts)
    q, good = face_terms(v, f)
    acc = np.zeros((len(v), 3), np.int64)
    for k in range(3):
        np.add.at(acc, f[good, k], q[good])
    return acc


def normalise(acc):
    """float32 [nv, 3] from the int64 accumulators (values up to 2^63: int64 -> float64 rounds to nearest even)."""
    d = np.asarray(acc, np.int64).astype(np.float64)
    with np.errstate(all="ignore"):
        L = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        out = np.where((L == 0)[:, None], 0.0, d / np.where(L == 0, 1.0, L)[:, None])
    return out.astype(np.float32)


def normals(vertices, faces, counts=None):
    """float32 [nv, 3]: the counted rows sfm_mesh_normals writes."""
    return normalise(normal_sums(vertices, faces, counts))


def quantise(p, origin, pscale):
    """(r int64 [n, 3], usable bool [n])."""
    with np.errstate(all="ignore"):
        r = np.rint((p - np.asarray(origin, np.float32)[None]) * np.float32(pscale))
        assert r.dtype == np.float32
        usable = np.all(np.abs(r) <= UNIT, axis=1)                     # NaN fails
    return np.where(usable[:, None], r, np.float32(0.0)).astype(np.int64), usable


def smooth_step(p, f, factor, origin, pscale):
    """One step over float32 rows p [nv, 3] and valid faces f -> new rows."""
    origin = np.asarray(origin, np.float32)
    r, usable = quantise(p, origin, pscale)
    nv = len(p)
    acc = np.zeros((nv, 3), np.int64)
    cnt = np.zeros(nv, np.int64)
    for k in range(3):
        for j in ((k + 1) % 3, (k + 2) % 3):
            ok = usable[f[:, j]]
            np.add.at(acc, f[ok, k], r[f[ok, j]])
            np.add.at(cnt, f[ok, k], 1)
    move = usable & (cnt > 0)
    out = p.copy()
    if move.any():
        pd = p[move].astype(np.float64)
        m = (acc[move].astype(np.float64) / cnt[move].astype(np.float64)[:, None]) / np.float64(np.float32(pscale)) + origin.astype(np.float64)[None]
        new = (pd + np.float64(np.float32(factor)) * (m - pd)).astype(np.float32)
        out.view(np.int32)[move] = new.view(np.int32)
    return out


def smooth(vertices, faces, factors, origin, pscale, counts=None):
    """float32 [nv, 3]: the counted rows sfm_mesh_smooth writes after len(factors) steps (rows that do not move keep their bits)."""
    v, f = _mesh(vertices, faces, counts)
    p = v.copy()
    for factor in np.asarray(factors, np.float32).reshape(-1):
        p = smooth_step(p, f, factor, origin, pscale)
    return p


def taubin_factors(steps, lam=0.5, mu=-0.53):
    """lambda, mu, lambda, mu, ...: `steps` pairs."""
    return np.tile(np.array([lam, mu], np.float32), int(steps))


def pscale_of(extent):
    """The largest power of two with extent * pscale <= 2^29."""
    extent = float(extent)
    if not (np.isfinite(extent) and extent > 0.0):
        raise ValueError(f"extent {extent} must be finite and positive")
    e = int(np.floor(np.log2(2.0 ** 29 / extent)))
    while extent * 2.0 ** (e + 1) <= 2.0 ** 29:
        e += 1
    while extent * 2.0 ** e > 2.0 ** 29:
        e -= 1
    return float(2.0 ** min(max(e, -126), 127))                       # a normal float32
