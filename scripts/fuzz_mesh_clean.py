"""Randomised parity sweep of the mesh clean-up on the GPU box: sfm_mesh_components / sfm_mesh_clean (mesh.mesh_components, the
C-ABI into sentinel-filled buffers, mesh.clean_mesh) vs the integer restatement tests/np_mesh_clean.py; every output compared
exactly (float rows as int32 views).

  python scripts/fuzz_mesh_clean.py [seconds] [seed] [family:case_seed]

Families (one case = one random draw; nv and nf log-uniform from 0 up to a cap that keeps the NumPy side under a second):
  components  face soups whose indices are drawn inside 1..nv clusters of vertices (so 1 to about nv components): labels against the
              restatement at a random `rounds` of 1..24, continued with resume until the status says converged; every intermediate
              state holds ids of the right component, >= its minimum and never rising
  clean       the same soups through the C-ABI with min_faces from {0, 1, 2, a face count that occurs, 10^9}, largest_only, colours or
              none, into full-size buffers filled with a sentinel: counts, the counted rows, and the sentinel everywhere after them
  composed    mesh.extract_mesh of a random field (spheres, noise, unknown points), then mesh.clean_mesh(packed=True), against
              np_mesh.extract_mesh + the restatement, sliced from the one packed buffer
One case in four carries a degeneracy: nf = 0, nv = 0, every face invalid (negative, nv, INT32_MAX), duplicate faces, (a,a,a) and
(a,a,b) faces, NaN / inf rows, a triangle strip with ascending / descending / zigzag / permuted ids, disjoint triangles.
The script stops at the first mismatch, prints the family and the case seed that rebuilds the inputs without a GPU
(gen_soup(np.random.default_rng(case_seed))), and exits non-zero.
"""
import ctypes
import os
import sys
import time

os.environ.setdefault("OMP_WAIT_POLICY", "passive")

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import np_mesh
import np_mesh_clean as npc

MAX_NV, MAX_NF = 1 << 17, 1 << 18
SENTINEL = 0x5A5A5A5A
INT32_MAX = 2 ** 31 - 1


def log_uniform_from_zero(rng, hi):
    """0 with probability 1/16, else log-uniform over 1..hi."""
    if rng.random() < 1.0 / 16:
        return 0
    return int(np.clip(np.floor(np.exp(rng.uniform(0.0, np.log(hi + 1)))), 1, hi))


def up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    import torch
    a = t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return a.view(np.int32) if a.dtype == np.float32 else a


def same(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def strip(n, order, rng=None):
    """A triangle strip of n faces over n + 2 vertices whose ids along the strip are ascending, descending, zigzag or permuted."""
    nv = n + 2
    pos = np.arange(nv, dtype=np.int64)
    if order == "descending":
        ids = pos[::-1].copy()
    elif order == "zigzag":                                   # 0, nv-1, 1, nv-2, ...
        ids = np.where(pos % 2 == 0, pos // 2, nv - 1 - pos // 2)
    elif order == "permuted":
        ids = (rng or np.random.default_rng(n)).permutation(nv)
    else:
        ids = pos
    return np.stack([ids[:-2], ids[1:-1], ids[2:]], 1).astype(np.int32), nv


def soup(rng, nv, nf, nclusters):
    """nf faces over nv vertices, each face's three indices drawn from one of `nclusters` random groups of vertices."""
    if nv == 0 or nf == 0:
        return np.zeros((nf, 3), np.int32) if nv else rng.integers(-3, 4, (nf, 3)).astype(np.int32)
    nclusters = int(np.clip(nclusters, 1, nv))
    perm = rng.permutation(nv)
    cuts = np.sort(rng.choice(np.arange(1, nv), nclusters - 1, replace=False)) if nclusters > 1 else np.zeros(0, np.int64)
    start = np.concatenate([[0], cuts]).astype(np.int64)
    size = np.diff(np.concatenate([start, [nv]]))
    c = rng.integers(0, nclusters, nf)
    idx = start[c, None] + np.floor(rng.random((nf, 3)) * size[c, None]).astype(np.int64)
    return perm[idx].astype(np.int32)


def rows(rng, nv, quirk=False):
    v = rng.standard_normal((nv, 3)).astype(np.float32)
    if quirk and nv:
        raw = v.view(np.int32)
        hit = rng.random((nv, 3)) < 0.2
        raw[hit] = rng.choice(np.array([0x7FC00000, 0x7F800001, -4194304 + 77, 0x7F800000, -8388608, 0, -2147483648], np.int64), int(hit.sum())).astype(np.int32)
    return v


def gen_soup(rng):
    """(tag, vertices, colors or None, faces)."""
    nv, nf = log_uniform_from_zero(rng, MAX_NV), log_uniform_from_zero(rng, MAX_NF)
    quirk = int(rng.integers(0, 8)) if rng.random() < 0.25 else -1
    tag = f"quirk {quirk}"
    if quirk == 0:
        nf = 0
    elif quirk == 1:
        nv = 0
    if quirk in (5, 6):
        n = max(1, min(nf, MAX_NF))
        if quirk == 5:
            order = ["ascending", "descending", "zigzag", "permuted"][int(rng.integers(0, 4))]
            f, nv = strip(n, order, rng)
            tag += f" strip {order}"
        else:
            n = min(n, MAX_NV // 3)
            nv = 3 * n
            f = rng.permutation(nv).reshape(n, 3).astype(np.int32)          # disjoint triangles
            f = np.vstack([f, f[:1] if n < 2 else [[f[0, 0], f[1, 0], f[1, 1]]]]).astype(np.int32)
    else:
        ncl = log_uniform_from_zero(rng, max(nv, 1)) if rng.random() < 0.8 else int(rng.integers(1, 400))
        f = soup(rng, nv, nf, max(ncl, 1))
        tag += f" clusters {ncl}"
    nf = len(f)
    if quirk == 2 and nf:                                     # every face invalid
        f = f.copy()
        f[np.arange(nf), rng.integers(0, 3, nf)] = rng.choice(np.array([-1, -2 ** 31, nv, INT32_MAX, nv + 7], np.int64), nf).astype(np.int32)
    elif quirk == 3 and nf:                                   # duplicates, (a,a,a), (a,a,b)
        f = f.copy()
        f[rng.random(nf) < 0.3] = f[0]
        k = rng.random(nf) < 0.3
        f[k, 1] = f[k, 0]
        k = rng.random(nf) < 0.2
        f[k, 2] = f[k, 0]
    elif quirk == 7 and nf:                                   # some faces invalid
        f = f.copy()
        k = rng.random(nf) < 0.3
        f[k, int(rng.integers(0, 3))] = rng.choice(np.array([-1, nv, INT32_MAX], np.int64), int(k.sum())).astype(np.int32)
    v = rows(rng, nv, quirk == 4 or rng.random() < 0.2)
    c = rows(rng, nv, quirk == 4) if rng.random() < 0.6 else None
    return f"nv {nv} nf {nf} {tag} colours {c is not None}", v, c, np.ascontiguousarray(f, np.int32)


def valid_intermediate(labels, want, previous=None):
    """Unconverged labels: ids of the vertex's own component, >= its minimum, never above the state before."""
    labels = np.asarray(labels, np.int64)
    nv = len(want)
    if len(labels) != nv or (nv and (labels.min() < 0 or labels.max() >= nv)):
        return False
    ok = np.array_equal(want[labels], want) and bool(np.all(labels >= want))
    return ok and (previous is None or bool(np.all(labels <= previous)))


def labels_by_resume(faces_dev, nv, rounds, want, max_calls=4096):
    """mesh_components at `rounds` per call until converged, every intermediate state checked -> (labels, calls, rounds that
    changed something in total) or a message."""
    from sfm_mvs_amd import mesh
    labels, prev, total = None, None, 0
    for call in range(1, max_calls + 1):
        labels, status = mesh.mesh_components(faces_dev, nv, rounds, labels)
        got, (done, changed) = labels.cpu().numpy(), (int(s) for s in status.cpu())
        total += changed
        if not valid_intermediate(got, want, prev):
            return f"call {call} at rounds {rounds}: not a valid intermediate state"
        if done:
            return got, call, total
        if changed != rounds:
            return f"call {call}: not converged after {changed} < {rounds} changing rounds"
        prev = got
    return f"not converged after {max_calls} calls of {rounds} rounds"


def case_components(rng):
    tag, v, c, f = gen_soup(rng)
    want, _ = npc.components(f, len(v))
    rounds = int(rng.integers(1, 25))
    res = labels_by_resume(up(f), len(v), rounds, want.astype(np.int64))
    if isinstance(res, str):
        return f"{tag}: {res}"
    return None if np.array_equal(res[0], want) else f"{tag}: labels differ (rounds {rounds})"


def raw_clean(v, c, f, labels, min_faces, largest_only):
    """sfm_mesh_clean through the C-ABI into full-size buffers filled with SENTINEL -> (out_v, out_c or None, out_f, counts) as
    host int32 arrays (all rows, the sentinel tail included)."""
    import torch
    from sfm_mvs_amd import _lib
    from sfm_mvs_amd.ops import _workspace
    L = _lib.lib()
    nv, nf = len(v), len(f)
    dv, df, dl = up(v), up(f), labels if torch.is_tensor(labels) else up(labels)
    dc = None if c is None else up(c)
    ov = torch.full((nv, 3), SENTINEL, dtype=torch.int32, device="cuda")
    oc = None if c is None else torch.full((nv, 3), SENTINEL, dtype=torch.int32, device="cuda")
    of = torch.full((nf, 3), SENTINEL, dtype=torch.int32, device="cuda")
    counts = torch.full((4,), SENTINEL, dtype=torch.int32, device="cuda")
    ws = _workspace(dv.device, L.sfm_mesh_clean_ws_bytes(nv, nf))
    p = lambda t, n: _lib.ptr(t) if (t is not None and n) else None
    _lib.check(L.sfm_mesh_clean(p(dv, nv), p(dc, nv), p(df, nf), nv, nf, p(dl, nv), int(min_faces), int(largest_only), p(ov, nv), p(oc, nv),
                                p(of, nf), _lib.ptr(counts), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "sfm_mesh_clean")
    return ov.cpu().numpy(), None if oc is None else oc.cpu().numpy(), of.cpu().numpy(), counts.cpu().numpy()


def compare_clean(got, want):
    """Names of what differs between raw_clean's buffers and the restatement's result (prefix rows, counts, sentinel tails)."""
    ov, oc, of, counts = got
    wv, wc, wf, wcounts = want
    bad = []
    if not np.array_equal(counts.astype(np.int64), wcounts):
        return [f"counts {counts.tolist()} != {wcounts.tolist()}"]
    kv, kf = int(wcounts[0]), int(wcounts[1])
    for name, g, w, k in (("vertices", ov, wv, kv), ("colours", oc, wc, kv), ("faces", of, wf, kf)):
        if (g is None) != (w is None):
            bad.append(name + " presence")
        elif g is not None:
            if not np.array_equal(g[:k], bits(w)):
                bad.append(name)
            if not np.all(g[k:] == SENTINEL):
                bad.append(name + " written past the counted rows")
    return bad


def thresholds(rng, f, nv):
    _, faces_of = npc.components(f, nv)
    occurring = faces_of[faces_of > 0]
    pool = [0, 1, 2, 10 ** 9] + ([int(rng.choice(occurring)), int(occurring.max()), int(occurring.max()) + 1] if len(occurring) else [])
    return int(pool[int(rng.integers(0, len(pool)))])


def case_clean(rng):
    from sfm_mvs_amd import mesh
    tag, v, c, f = gen_soup(rng)
    min_faces, largest = thresholds(rng, f, len(v)), bool(rng.integers(0, 2))
    labels, status = mesh.mesh_components(up(f), len(v), 1024)
    if int(status[0]) != 1:
        return f"{tag}: not converged in 1024 rounds"
    bad = compare_clean(raw_clean(v, c, f, labels, min_faces, largest), npc.clean(v, c, f, min_faces, largest))
    return f"{tag} min_faces {min_faces} largest_only {largest}: {', '.join(bad)}" if bad else None


def gen_field(rng):
    dims = tuple(int(rng.integers(2, 40)) for _ in range(3))
    nx, ny, nz = dims
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    kind = int(rng.integers(0, 3))
    if kind == 0:                                             # a few spheres: a few closed components
        S = np.full((nz, ny, nx), 1e3)
        for _ in range(int(rng.integers(1, 6))):
            ctr, r = rng.uniform(0, max(dims), 3), rng.uniform(0.7, 0.3 * max(dims) + 1)
            S = np.minimum(S, np.sqrt((x - ctr[0]) ** 2 + (y - ctr[1]) ** 2 + (z - ctr[2]) ** 2) - r)
    elif kind == 1:                                           # noise: debris everywhere
        S = rng.standard_normal((nz, ny, nx))
    else:                                                     # a plane cut into islands by unknown points
        S = z - rng.uniform(0.2, max(nz - 1.2, 0.3)) + 0.1 * rng.standard_normal((nz, ny, nx))
    W = (rng.random((nz, ny, nx)) < rng.uniform(0.5, 1.0)).astype(np.float32) * 2.0 if kind else np.full((nz, ny, nx), 2.0, np.float32)
    C = None
    if rng.random() < 0.5:
        C = np.concatenate([rng.uniform(0, 2000, (nz, ny, nx, 3)), rng.integers(0, 3, (nz, ny, nx, 1))], -1).astype(np.float32)
    return f"field {dims} kind {kind} colours {C is not None}", (S * W).astype(np.float32), W, C


def case_composed(rng):
    from sfm_mvs_amd import mesh
    tag, S, W, C = gen_field(rng)
    origin, voxel = np.zeros(3, np.float32), np.float32(0.5)
    wv, wc, wf = np_mesh.extract_mesh(S, W, C, origin, voxel, 1.0)
    min_faces, largest = thresholds(rng, wf, len(wv)), bool(rng.integers(0, 4) == 0)
    v, c, f = mesh.extract_mesh(up(S), up(W), None if C is None else up(C), origin, voxel, 1.0)
    *_, status, labels, buf = mesh.clean_mesh(v, c, f, min_faces, largest, packed=True)
    host = buf.cpu().numpy()
    if host[4] != 1:
        return f"{tag}: not converged at the default rounds (status {host[4:6].tolist()})"
    kv, kc, kf, counts = npc.clean(wv, wc, wf, min_faces, largest)
    nv, ncol = len(wv), len(wv) if C is not None else 0
    bad = []
    if not np.array_equal(host[:4].astype(np.int64), counts):
        bad.append(f"counts {host[:4].tolist()} != {counts.tolist()}")
    else:
        if not np.array_equal(host[6:6 + 3 * len(kv)], bits(kv).ravel()):
            bad.append("vertices")
        if C is not None and not np.array_equal(host[6 + 3 * nv:6 + 3 * nv + 3 * len(kv)], bits(kc).ravel()):
            bad.append("colours")
        o = 6 + 3 * (nv + ncol)
        if not np.array_equal(host[o:o + 3 * len(kf)], kf.ravel()):
            bad.append("faces")
    return f"{tag} min_faces {min_faces} largest_only {largest}: {', '.join(bad)}" if bad else None


FAMILIES = [("components", case_components, 3), ("clean", case_clean, 4), ("composed", case_composed, 2)]


def run(budget, seed, log=print):
    """Cases for `budget` seconds from `seed`; stops at the first mismatch -> (counts per family, mismatches, seconds)."""
    fns = {name: fn for name, fn, _ in FAMILIES}
    rng = np.random.default_rng(seed)
    weights = np.array([w for _, _, w in FAMILIES], float); weights /= weights.sum()
    t0 = time.time(); counts = {name: 0 for name, _, _ in FAMILIES}; bad = 0
    while time.time() - t0 < budget and not bad:
        name = FAMILIES[int(rng.choice(len(FAMILIES), p=weights))][0]
        case_seed = int(rng.integers(1 << 31))
        try:
            msg = fns[name](np.random.default_rng(case_seed))
        except Exception as e:  # noqa: BLE001
            msg = f"EXCEPTION {e!r}"[:300]
        counts[name] += 1
        if msg:
            bad += 1
            log(f"MISMATCH {name} (seed {seed}, case seed {case_seed}; replay: fuzz_mesh_clean.py 0 0 {name}:{case_seed}) {msg}")
    return counts, bad, time.time() - t0


def main():
    import sfm_mvs_amd
    from sfm_mvs_amd import _lib
    budget = float(sys.argv[1]) if len(sys.argv) > 1 else 120.0
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    sfm_mvs_amd.lib()
    if len(sys.argv) > 3:                               # replay one case
        name, case_seed = sys.argv[3].split(":")
        msg = {n: fn for n, fn, _ in FAMILIES}[name](np.random.default_rng(int(case_seed)))
        print(f"fuzz_mesh_clean replay {name}:{case_seed}: {msg or 'no mismatch'}")
        return 1 if msg else 0
    counts, bad, dt = run(budget, seed, log=lambda s: print(s, flush=True))
    print(f"fuzz_mesh_clean: seed {seed}, {sum(counts.values())} cases {counts}, {bad} mismatches, {dt:.0f} s")
    print(f"sfm_build_id {_lib.build_id()}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
