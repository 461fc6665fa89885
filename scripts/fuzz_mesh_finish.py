"""Randomised parity sweep of the mesh finishing step on the GPU box: sfm_mesh_normals / sfm_mesh_smooth (the C-ABI into
sentinel-filled buffers, mesh.mesh_normals, mesh.smooth_mesh) vs the restatement tests/np_mesh_finish.py; every output compared
exactly (float rows as int32 views), and the sentinel must survive at and past the counted rows.

  python scripts/fuzz_mesh_finish.py [seconds] [seed] [family:case_seed]

Families (one case = one random draw; nv and nf log-uniform from 0 up to a cap that keeps the NumPy side under a second):
  normals   face soups (indices near each other, so that vertices are shared, or uniform) over rows in a random box
  smooth    the same soups through 0..8 steps (sometimes up to 64 on a small mesh) with Taubin's factors or random ones
  composed  mesh.extract_mesh of a random field, mesh.clean_mesh(packed=True), then mesh.smooth_mesh and mesh.mesh_normals on its
            outputs with its counts read on the device, against np_mesh + np_mesh_clean + the restatement
One case in four carries a degeneracy: nf = 0, nv = 0, a quarter of the indices from {-1, nv, INT32_MAX}, duplicate faces and
repeated indices, NaN / inf / 1e30 / 1e-30 coordinates, collinear and zero-area faces, a hub vertex in every face, vertices beyond
the usable range next to usable ones; and one in three passes device counts (smaller, equal, (0, 0), negative, too large).
The script stops at the first mismatch, prints the family and the case seed that rebuilds the inputs without a GPU
(gen_mesh(np.random.default_rng(case_seed))), and exits non-zero.
"""
import os
import sys
import time

os.environ.setdefault("OMP_WAIT_POLICY", "passive")

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]
import np_mesh
import np_mesh_clean as npc
import np_mesh_finish as nf
from fuzz_mesh_clean import SENTINEL, bits, gen_field, log_uniform_from_zero, thresholds, up

MAX_NV, MAX_NF = 1 << 16, 1 << 17
INT32_MAX = 2 ** 31 - 1


def _counts_dev(counts):
    import torch
    return None if counts is None else torch.tensor([int(c) for c in counts], dtype=torch.int32, device="cuda")


def raw_normals(v, f, counts=None):
    """sfm_mesh_normals through the C-ABI into a full-size buffer filled with SENTINEL -> host int32 [nv_cap, 3]."""
    import torch
    from sfm_mvs_amd import _lib
    from sfm_mvs_amd.ops import _workspace
    L = _lib.lib()
    nv, nk = len(v), len(f)
    dv, df, dc = up(np.asarray(v, np.float32)), up(np.asarray(f, np.int32)), _counts_dev(counts)
    out = torch.full((nv, 3), SENTINEL, dtype=torch.int32, device="cuda")
    ws = _workspace(out.device, L.sfm_mesh_normals_ws_bytes(nv, nk))
    p = lambda t, n: _lib.ptr(t) if n else None
    _lib.check(L.sfm_mesh_normals(p(dv, nv), p(df, nk), nv, nk, _lib.ptr(dc), p(out, nv), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()),
               "sfm_mesh_normals")
    return out.cpu().numpy()


def raw_smooth(v, f, factors, origin, pscale, counts=None):
    """sfm_mesh_smooth through the C-ABI into a full-size buffer filled with SENTINEL -> host int32 [nv_cap, 3]."""
    import torch
    from sfm_mvs_amd import _lib
    from sfm_mvs_amd.ops import _workspace
    L = _lib.lib()
    nv, nk = len(v), len(f)
    dv, df, dc = up(np.asarray(v, np.float32)), up(np.asarray(f, np.int32)), _counts_dev(counts)
    out = torch.full((nv, 3), SENTINEL, dtype=torch.int32, device="cuda")
    ws = _workspace(out.device, L.sfm_mesh_smooth_ws_bytes(nv, nk))
    fac = np.ascontiguousarray(factors, np.float32).reshape(-1)
    org = np.ascontiguousarray(origin, np.float32).reshape(3)
    p = lambda t, n: _lib.ptr(t) if n else None
    _lib.check(L.sfm_mesh_smooth(p(dv, nv), p(df, nk), nv, nk, _lib.ptr(dc), len(fac), fac.ctypes.data if len(fac) else None, org.ctypes.data,
                                 float(pscale), p(out, nv), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "sfm_mesh_smooth")
    return out.cpu().numpy()


def compare(got, want, what):
    """Names of what differs between a sentinel-filled output and the restatement's counted rows."""
    k = len(want)
    bad = []
    if not np.array_equal(got[:k], bits(want)):
        bad.append(f"{what} ({int(np.any(got[:k] != bits(want), axis=1).sum())} of {k} rows)")
    if not np.all(got[k:] == SENTINEL):
        bad.append(f"{what} written at or past the counted rows")
    return bad


def local_soup(rng, nv, nk, spread):
    """nk faces over nv vertices: a random first index, the other two within `spread` ids of it (clipped), so vertices are shared."""
    if nv == 0:
        return rng.integers(-3, 4, (nk, 3)).astype(np.int32)
    a = rng.integers(0, nv, nk)
    off = rng.integers(-spread, spread + 1, (nk, 2))
    return np.clip(np.stack([a, a + off[:, 0], a + off[:, 1]], 1), 0, nv - 1).astype(np.int32)


def gen_mesh(rng):
    """(tag, vertices float32 [nv, 3], faces int32 [nk, 3], origin float32 [3], extent, counts or None)."""
    nv, nk = log_uniform_from_zero(rng, MAX_NV), log_uniform_from_zero(rng, MAX_NF)
    quirk = int(rng.integers(0, 8)) if rng.random() < 0.25 else -1
    if quirk == 0:
        nk = 0
    elif quirk == 1:
        nv = 0
    extent = float(np.exp(rng.uniform(np.log(1e-3), np.log(1e3))))
    origin = (rng.uniform(-2.0, 2.0, 3) * extent).astype(np.float32)
    v = (origin.astype(np.float64) + rng.random((nv, 3)) * extent).astype(np.float32)
    spread = int(rng.integers(1, 9)) if rng.random() < 0.7 else max(nv, 1)
    f = local_soup(rng, nv, nk, spread)
    tag = f"nv {nv} nf {nk} quirk {quirk} spread {spread} extent {extent:.3g}"
    if quirk == 2 and nk:                                     # a quarter of the indices name no vertex
        hit = rng.random((nk, 3)) < 0.25
        f[hit] = rng.choice(np.array([-1, nv, INT32_MAX], np.int64), int(hit.sum())).astype(np.int32)
    elif quirk == 3 and nk:                                   # duplicate faces, (a, a, b), (a, a, a)
        f[rng.random(nk) < 0.3] = f[0]
        k = rng.random(nk) < 0.3
        f[k, 1] = f[k, 0]
        k = rng.random(nk) < 0.2
        f[k, 2] = f[k, 0]
    elif quirk == 4 and nv:                                   # coordinates that are not finite, overflow or underflow
        hit = rng.random((nv, 3)) < 0.15
        v[hit] = rng.choice(np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 1e-30, -1e-30, 0.0, -0.0], np.float32), int(hit.sum()))
        raw = v.view(np.int32)
        pay = rng.random((nv, 3)) < 0.05
        raw[pay] = rng.choice(np.array([0x7FC00123, 0x7F800001, -4194304 + 77], np.int64), int(pay.sum())).astype(np.int32)
    elif quirk == 5 and nv:                                   # collinear and coincident vertices: zero-area faces
        t = rng.random(nv)
        line = (origin.astype(np.float64) + np.outer(t, rng.random(3)) * extent).astype(np.float32)
        k = rng.random(nv) < 0.6
        v[k] = line[k]
        k = rng.random(nv) < 0.2
        v[k] = v[0]
    elif quirk == 6 and nv and nk:                            # one hub vertex in every face
        f[:, int(rng.integers(0, 3))] = int(rng.integers(0, nv))
    elif quirk == 7 and nv:                                   # vertices beyond the usable range, next to usable ones
        k = rng.random(nv) < 0.2
        v[k] = (v[k].astype(np.float64) + rng.choice(np.array([-5.0, 2.5, 5.0, 100.0]), (int(k.sum()), 3)) * extent).astype(np.float32)
    counts = None
    if rng.random() < 1.0 / 3:
        counts = [(int(rng.integers(0, nv + 1)), int(rng.integers(0, nk + 1))), (nv, nk), (0, 0), (-1, int(rng.integers(0, nk + 1))),
                  (int(rng.integers(0, nv + 1)), -7), (nv + 1, nk + 1), (INT32_MAX, INT32_MAX)][int(rng.integers(0, 7))]
        tag += f" counts {counts}"
    return tag, v, np.ascontiguousarray(f, np.int32), origin, extent, counts


def case_normals(rng):
    tag, v, f, origin, extent, counts = gen_mesh(rng)
    bad = compare(raw_normals(v, f, counts), nf.normals(v, f, counts), "normals")
    return f"{tag}: {', '.join(bad)}" if bad else None


def gen_factors(rng, nv, nk):
    big = nv + nk > 20000
    nsteps = int(rng.integers(0, 9)) if big or rng.random() < 0.8 else int(rng.integers(9, 65))
    kind = int(rng.integers(0, 3))
    if kind == 0:
        fac = np.tile(np.array([0.5, -0.53], np.float32), 32)[:nsteps]
    elif kind == 1:
        fac = rng.uniform(-1.0, 1.0, nsteps).astype(np.float32)
    else:
        fac = rng.choice(np.array([0.0, 1.0, -1.0, 0.33, 1e-8, 2.0, -2.0], np.float32), nsteps)
    return np.ascontiguousarray(fac, np.float32)


def case_smooth(rng):
    tag, v, f, origin, extent, counts = gen_mesh(rng)
    fac = gen_factors(rng, len(v), len(f))
    pscale = nf.pscale_of(extent)
    bad = compare(raw_smooth(v, f, fac, origin, pscale, counts), nf.smooth(v, f, fac, origin, pscale, counts), "vertices")
    return f"{tag} steps {len(fac)} pscale {pscale:g}: {', '.join(bad)}" if bad else None


def case_composed(rng):
    from sfm_mvs_amd import mesh
    tag, S, W, C = gen_field(rng)
    origin, voxel = np.zeros(3, np.float32), np.float32(0.5)
    wv, wc, wf = np_mesh.extract_mesh(S, W, C, origin, voxel, 1.0)
    min_faces, largest = thresholds(rng, wf, len(wv)), bool(rng.integers(0, 4) == 0)
    steps = int(rng.integers(0, 4))
    extent = float(voxel) * (max(S.shape) - 1)
    v, c, f = mesh.extract_mesh(up(S), up(W), None if C is None else up(C), origin, voxel, 1.0)
    ov, oc, of, counts, status, labels, buf = mesh.clean_mesh(v, c, f, min_faces, largest, packed=True)
    sv = mesh.smooth_mesh(ov, of, steps, origin, extent, counts=counts)        # no host read in between
    nr = mesh.mesh_normals(sv, of, counts=counts)
    if int(status[0]) != 1:
        return f"{tag}: not converged at the default rounds"
    kv, kc, kf, kcounts = npc.clean(wv, wc, wf, min_faces, largest)
    want_v = nf.smooth(kv, kf, nf.taubin_factors(steps), origin, nf.pscale_of(extent))
    want_n = nf.normals(want_v, kf)
    bad = []
    if counts.cpu().numpy().tolist() != kcounts.tolist():
        bad.append("counts")
    else:
        k = len(kv)
        if not np.array_equal(bits(sv)[:k], bits(want_v)):
            bad.append("vertices")
        if not np.array_equal(bits(nr)[:k], bits(want_n)):
            bad.append("normals")
    return f"{tag} min_faces {min_faces} largest_only {largest} pairs {steps}: {', '.join(bad)}" if bad else None


FAMILIES = [("normals", case_normals, 4), ("smooth", case_smooth, 4), ("composed", case_composed, 2)]


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
            log(f"MISMATCH {name} (seed {seed}, case seed {case_seed}; replay: fuzz_mesh_finish.py 0 0 {name}:{case_seed}) {msg}")
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
        print(f"fuzz_mesh_finish replay {name}:{case_seed}: {msg or 'no mismatch'}")
        return 1 if msg else 0
    counts, bad, dt = run(budget, seed, log=lambda s: print(s, flush=True))
    print(f"fuzz_mesh_finish: seed {seed}, {sum(counts.values())} cases {counts}, {bad} mismatches, {dt:.0f} s")
    print(f"sfm_build_id {_lib.build_id()}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
