"""NumPy restatement of the mesh decimation step (include/sfm_hip.h, "MESH-DECIMATE"; docs/mesh.md §9), written from the header and
importing nothing of the product: vertex clustering over a regular grid with the smallest usable vertex id of a cell as its leader
(np.minimum.at), the mean of int64 sums of quantised rows (np.add.at), order-preserving compactions, and the lowest input index
among the faces that become equal up to a rotation.  float32 operations are NumPy float32 operations in the header's order, so
the GPU tests compare int32 views exactly."""
import numpy as np

UNIT = np.float32(2.0 ** 30)
COLOUR_UNIT, COLOUR_MAX = np.float32(65536.0), np.float32(32768.0)
MAX_CELLS = 2 ** 27
INT32_MAX = 2 ** 31 - 1


def resolve_counts(counts, nv_cap, nf_cap):
    """(nv, nf): the capacities, or the given pair where it lies in 0..capacity."""
    if counts is None:
        return int(nv_cap), int(nf_cap)
    nv, nf = int(counts[0]), int(counts[1])
    return (nv if 0 <= nv <= nv_cap else int(nv_cap)), (nf if 0 <= nf <= nf_cap else int(nf_cap))


def cells(p, origin, cell, dims, pscale):
    """(key int64 [n] (-1: not usable), r int64 [n, 3] (0 where not usable)) of float32 rows p."""
    o = np.asarray(origin, np.float32).reshape(3)
    d = np.asarray(dims, np.int64).reshape(3)
    assert np.all(d >= 1) and int(d[0]) * int(d[1]) * int(d[2]) <= MAX_CELLS
    with np.errstate(all="ignore"):
        t = np.floor((p.astype(np.float64) - o.astype(np.float64)[None]) / np.float64(np.float32(cell)))
        inside = np.all((t >= 0.0) & (t < d.astype(np.float64)[None]), axis=1)             # NaN and +-inf fail
        r = np.rint((p - o[None]) * np.float32(pscale))
        assert r.dtype == np.float32
        usable = inside & np.all(np.abs(r) <= UNIT, axis=1)
    ti = np.where(usable[:, None], t, 0.0).astype(np.int64)
    key = (ti[:, 2] * d[1] + ti[:, 1]) * d[0] + ti[:, 0]
    return np.where(usable, key, -1), np.where(usable[:, None], r, np.float32(0.0)).astype(np.int64)


def colour_terms(c):
    with np.errstate(all="ignore"):
        ok = np.abs(c) <= COLOUR_MAX                                                       # NaN fails
        q = np.rint(np.where(ok, c, np.float32(0.0)) * COLOUR_UNIT)
        assert q.dtype == np.float32
    return q.astype(np.int64)


def cluster(vertices, colors, origin, cell, dims, pscale, nv):
    """(newid int64 [nv] (-1: not usable), out_v float32, out_c float32 or None, sums) of the first nv rows; sums = (acc int64
    [leaders, 3], cnt int64 [leaders]) for the tests that state expected words from Python integers."""
    p = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)[:nv]
    key, r = cells(p, origin, cell, dims, pscale)
    use = np.flatnonzero(key >= 0)
    occupied, slot = np.unique(key[use], return_inverse=True)                             # a table over the occupied cells only
    table = np.full(len(occupied), INT32_MAX, np.int64)
    np.minimum.at(table, slot, use)
    leader_of = np.full(nv, -1, np.int64)
    leader_of[use] = table[slot]
    leaders = np.flatnonzero(leader_of == np.arange(nv))                                   # ascending ids
    rank = np.full(nv, -1, np.int64)
    rank[leaders] = np.arange(len(leaders))
    newid = np.where(leader_of >= 0, rank[np.maximum(leader_of, 0)], -1)
    acc = np.zeros((len(leaders), 3), np.int64)
    cnt = np.zeros(len(leaders), np.int64)
    np.add.at(acc, newid[use], r[use])
    np.add.at(cnt, newid[use], 1)
    o64 = np.asarray(origin, np.float32).reshape(3).astype(np.float64)
    cd = cnt.astype(np.float64)[:, None]
    out_v = ((acc.astype(np.float64) / cd) / np.float64(np.float32(pscale)) + o64[None]).astype(np.float32)
    out_c = None
    if colors is not None:
        c = np.ascontiguousarray(colors, np.float32).reshape(-1, 3)[:nv]
        cacc = np.zeros((len(leaders), 3), np.int64)
        np.add.at(cacc, newid[use], colour_terms(c[use]))
        out_c = ((cacc.astype(np.float64) / cd) / np.float64(65536.0)).astype(np.float32)
    return newid, out_v, out_c, (acc, cnt)


def normalise(t):
    """Rows rotated so that the smallest id comes first (the ids of a row differ pairwise)."""
    k = np.argmin(t, axis=1)
    idx = (k[:, None] + np.arange(3)[None]) % 3
    return np.take_along_axis(t, idx, axis=1)


def decimate(vertices, colors, faces, origin, cell, dims, pscale, dedupe=True, counts=None):
    """(out_v float32 [k, 3], out_c float32 [k, 3] or None, out_f int32 [m, 3], counts int64 [4]): the counted rows
    sfm_mesh_decimate writes, and (vertices out, faces out, unusable vertices, live faces dropped as duplicates)."""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    nv, nf = resolve_counts(counts, len(v), len(f))
    newid, out_v, out_c, _ = cluster(v, colors, origin, cell, dims, pscale, nv)
    f = f[:nf]
    f = f[np.all((f >= 0) & (f < nv), axis=1)]                                             # valid, in input order
    t = newid[f] if len(f) else np.zeros((0, 3), np.int64)
    live = np.all(t >= 0, axis=1) & (t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])
    t = t[live]
    dropped = 0
    if dedupe and len(t):
        _, first = np.unique(normalise(t), axis=0, return_index=True)                       # the first occurrence of each class
        dropped = len(t) - len(first)
        t = t[np.sort(first)]
    return out_v, out_c, t.astype(np.int32), np.array([len(out_v), len(t), nv - int((newid >= 0).sum()), dropped], np.int64)


def frame_of(origin, voxel, dims, decimate_cells):
    """run_mesh's frame: (origin float32 [3], cell float32, dims (3,), extent) for a volume (origin float64, voxel, dims) and a cell of
    `decimate_cells` voxels: one margin cell below the volume's origin, dims_c = floor((dims_c - 1) * voxel / cell) + 3, and the
    padded frame's longest side as the extent of the quantisation."""
    cell = float(decimate_cells) * float(voxel)
    o = (np.asarray(origin, np.float64).reshape(3) - cell).astype(np.float32)
    d = tuple(int(np.floor((int(n) - 1) * float(voxel) / cell)) + 3 for n in dims)
    return o, np.float32(cell), d, cell * max(d)
