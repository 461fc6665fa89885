"""Integer NumPy restatement of the mesh clean-up (include/sfm_hip.h, "MESH-CLEAN"; docs/mesh.md §7), written from the header and
importing nothing of the product: connected components by their smallest vertex id, faces per component, the keep rule and the
order-preserving compaction.  Everything is integer arithmetic or a bit-for-bit copy, so the GPU tests compare exactly."""
import numpy as np


def valid_faces(faces, nv):
    """Boolean [nf]: the face's three indices lie in 0..nv-1."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return np.all((f >= 0) & (f < nv), axis=1)


def components(faces, nv):
    """(labels int32 [nv], faces_of int64 [nv]): labels[v] = the smallest vertex id of v's component (two vertices are connected
    when a valid face names both); faces_of[c] = the valid faces whose vertices carry label c (0 where c is no label)."""
    nv = int(nv)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    f = f[valid_faces(f, nv)]
    label = np.arange(nv, dtype=np.int64)
    while True:
        before = label
        label = label.copy()
        m = label[f].min(axis=1) if len(f) else np.zeros(0, np.int64)
        for k in range(3):                                   # the three labels and the labels of the three current labels
            np.minimum.at(label, f[:, k], m)
            np.minimum.at(label, before[f[:, k]], m)
        while True:                                          # full pointer jumping: label[v] = label[label[v]] to the end
            nxt = label[label]
            if np.array_equal(nxt, label):
                break
            label = nxt
        if np.array_equal(label, before):
            break
    faces_of = np.bincount(label[f[:, 0]], minlength=nv).astype(np.int64) if len(f) else np.zeros(nv, np.int64)
    return label.astype(np.int32), faces_of


def keep_components(labels, faces_of, min_faces, largest_only):
    """Boolean [nv] over LABELS c (meaningful where labels[c] == c): is component c kept?"""
    labels = np.asarray(labels, np.int64)
    nv = len(labels)
    roots = np.flatnonzero(labels == np.arange(nv))
    keep = np.zeros(nv, bool)
    if not largest_only:
        keep[roots] = faces_of[roots] >= int(min_faces)
    elif len(roots):
        best = int(faces_of[roots].max())
        c = int(roots[faces_of[roots] == best].min())        # ties: the lowest label
        keep[c] = best >= int(min_faces)
    return keep


def clean(vertices, colors, faces, min_faces, largest_only=False, parts=None):
    """(vertices, colors or None, faces int32, counts int64 [4] = (vertices kept, faces kept, components, components kept)).
    Rows are copied through an int32 view: bit for bit.  parts: components(faces, nv) of these faces, when the caller has it."""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    nv = len(v)
    f = np.asarray(faces, np.int32).reshape(-1, 3)
    labels, faces_of = components(f, nv) if parts is None else parts
    keep_c = keep_components(labels, faces_of, min_faces, largest_only)
    keep_v = keep_c[labels] if nv else np.zeros(0, bool)
    new_id = np.cumsum(keep_v) - 1                            # rank among the kept vertices
    ok = valid_faces(f, nv)
    keep_f = ok.copy()
    keep_f[ok] = keep_v[f[ok, 0]]
    out_f = new_id[f[keep_f].astype(np.int64)].astype(np.int32).reshape(-1, 3)
    out_v = v.view(np.int32)[keep_v].view(np.float32)
    out_c = None
    if colors is not None:
        out_c = np.ascontiguousarray(colors, np.float32).reshape(-1, 3).view(np.int32)[keep_v].view(np.float32)
    ncomp = int((labels == np.arange(nv)).sum())
    counts = np.array([int(keep_v.sum()), int(keep_f.sum()), ncomp, int(keep_c.sum())], np.int64)
    return out_v, out_c, out_f, counts
