"""Randomised parity sweep of the mesh decimation step on the GPU box: sfm_mesh_decimate (the C-ABI into sentinel-filled buffers,
mesh.decimate_mesh) vs the restatement tests/np_mesh_decimate.py; every output compared exactly (float rows as int32 views), and
the sentinel must survive at and past the counted rows.

  python scripts/fuzz_mesh_decimate.py [seconds] [seed] [family:case_seed]

Families (one case = one random draw; nv and nf log-uniform from 0 up to a cap that keeps the NumPy side under a second):
  decimate  face soups (indices near each other, so that vertices are shared, or uniform) over rows in a random box, a random grid
            of 1..48 cells per axis over that box or a part of it, with or without colours, dedupe off
  dedupe    the same with dedupe on, half of the soups seeded with repeats, rotations and flips of their own faces
  composed  mesh.extract_mesh of a random field, mesh.clean_mesh(packed=True), mesh.smooth_mesh, mesh.decimate_mesh and
            mesh.mesh_normals, each on the counts the one before left on the device, against np_mesh + np_mesh_clean +
            np_mesh_finish + the restatement
One case in four carries a degeneracy: nf = 0, nv = 0, a quarter of the indices from {-1, nv, INT32_MAX}, repeated indices and
duplicate faces, NaN / inf / 1e30 positions and NaN / inf / 1e6 colours, coordinates exactly on cell boundaries of a power-of-two
cell (the frame's own faces included), one cell for everything, a frame so fine that vertices pass 2^30 quanta; and one in three
passes device counts (smaller, equal, (0, 0), negative, too large).
The script stops at the first mismatch, prints the family and the case seed that rebuilds the inputs without a GPU
(gen_case(np.random.default_rng(case_seed), dedupe)), and exits non-zero.
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
import np_mesh_decimate as nd
import np_mesh_finish as nf
from fuzz_mesh_clean import SENTINEL, bits, gen_field, log_uniform_from_zero, thresholds, up
from fuzz_mesh_finish import local_soup

MAX_NV, MAX_NF = 1 << 16, 1 << 17
INT32_MAX = 2 ** 31 - 1


def raw_decimate(v, c, f, origin, cell, dims, pscale, dedupe, counts=None):
    """sfm_mesh_decimate through the C-ABI into full-size buffers filled with SENTINEL -> (out_v, out_c or None, out_f, counts) as
    host int32 arrays (all rows, the sentinel tail included)."""
    import torch
    from sfm_mvs_amd import _lib
    from sfm_mvs_amd.ops import _workspace
    L = _lib.lib()
    nv, nk = len(v), len(f)
    dv, df = up(np.asarray(v, np.float32)), up(np.asarray(f, np.int32))
    dc = None if c is None else up(np.asarray(c, np.float32))
    dn = None if counts is None else torch.tensor([int(x) for x in counts], dtype=torch.int32, device="cuda")
    ov = torch.full((nv, 3), SENTINEL, dtype=torch.int32, device="cuda")
    oc = None if c is None else torch.full((nv, 3), SENTINEL, dtype=torch.int32, device="cuda")
    of = torch.full((nk, 3), SENTINEL, dtype=torch.int32, device="cuda")
    on = torch.full((4,), SENTINEL, dtype=torch.int32, device="cuda")
    d = np.ascontiguousarray(dims, np.int32).reshape(3)
    org = np.ascontiguousarray(origin, np.float32).reshape(3)
    ws = _workspace(ov.device, L.sfm_mesh_decimate_ws_bytes(nv, nk, d.ctypes.data))
    p = lambda t, n: _lib.ptr(t) if n and t is not None else None
    _lib.check(L.sfm_mesh_decimate(p(dv, nv), p(dc, nv), p(df, nk), nv, nk, _lib.ptr(dn), org.ctypes.data, float(cell), d.ctypes.data,
                                   float(pscale), int(bool(dedupe)), p(ov, nv), p(oc, nv), p(of, nk), _lib.ptr(on), _lib.ptr(ws), ws.numel(),
                                   _lib.stream_ptr()), "sfm_mesh_decimate")
    return ov.cpu().numpy(), None if oc is None or nv == 0 else oc.cpu().numpy(), of.cpu().numpy(), on.cpu().numpy()


def compare(got, want):
    """Names of what differs between raw_decimate's buffers and the restatement's result (counts, prefix rows, sentinel tails)."""
    ov, oc, of, counts = got
    wv, wc, wf, wcounts = want
    if not np.array_equal(counts.astype(np.int64), wcounts):
        return [f"counts {counts.tolist()} != {wcounts.tolist()}"]
    bad = []
    for name, g, w in (("vertices", ov, wv), ("colours", oc, wc), ("faces", of, wf)):
        if g is None:
            continue
        k = len(w)
        if not np.array_equal(g[:k], bits(w)):
            bad.append(f"{name} ({int(np.any(g[:k] != bits(w), axis=1).sum())} of {k} rows)")
        if not np.all(g[k:] == SENTINEL):
            bad.append(f"{name} written at or past the counted rows")
    return bad


def twins(rng, f, share=0.5):
    """The soup with `share` of its faces replaced by a rotation, a flip or a copy of another of its faces."""
    nk = len(f)
    if nk < 2:
        return f
    f = f.copy()
    hit = np.flatnonzero(rng.random(nk) < share)
    src = f[rng.integers(0, nk, len(hit))]
    how = rng.integers(0, 4, len(hit))
    rot = np.where((how == 1)[:, None], src[:, [1, 2, 0]], np.where((how == 2)[:, None], src[:, [2, 0, 1]], src))
    f[hit] = np.where((how == 3)[:, None], src[:, [0, 2, 1]], rot)
    return f


def gen_case(rng, dedupe):
    """(tag, vertices, colours or None, faces, origin float32 [3], cell, dims, pscale, counts or None)."""
    nv, nk = log_uniform_from_zero(rng, MAX_NV), log_uniform_from_zero(rng, MAX_NF)
    quirk = int(rng.integers(0, 9)) if rng.random() < 0.25 else -1
    if quirk == 0:
        nk = 0
    elif quirk == 1:
        nv = 0
    extent = float(np.exp(rng.uniform(np.log(1e-3), np.log(1e3))))
    box = (rng.uniform(-2.0, 2.0, 3) * extent).astype(np.float32)
    v = (box.astype(np.float64) + rng.random((nv, 3)) * extent).astype(np.float32)
    c = (rng.random((nv, 3)) * 255.0).astype(np.float32) if rng.random() < 0.6 else None
    spread = int(rng.integers(1, 9)) if rng.random() < 0.7 else max(nv, 1)
    f = local_soup(rng, nv, nk, spread)
    if dedupe and rng.random() < 0.5:
        f = twins(rng, f)
    dims = tuple(int(np.floor(np.exp(rng.uniform(0.0, np.log(49.0))))) for _ in range(3))
    cover = float(rng.choice([1.0, 1.0, 1.0, 0.6]))                    # 0.6: part of the box lies outside the frame
    cell = np.float32(cover * extent / max(dims))
    origin = box.copy()
    pscale = nf.pscale_of(float(cell) * max(dims))
    tag = f"nv {nv} nf {nk} quirk {quirk} spread {spread} extent {extent:.3g} dims {dims} cell {float(cell):.6g} colours {c is not None}"
    if quirk == 2 and nk:                                     # a quarter of the indices name no vertex
        hit = rng.random((nk, 3)) < 0.25
        f[hit] = rng.choice(np.array([-1, nv, INT32_MAX], np.int64), int(hit.sum())).astype(np.int32)
    elif quirk == 3 and nk:                                   # duplicate faces, (a, a, b), (a, a, a)
        f[rng.random(nk) < 0.3] = f[0]
        k = rng.random(nk) < 0.3
        f[k, 1] = f[k, 0]
        k = rng.random(nk) < 0.2
        f[k, 2] = f[k, 0]
    elif quirk == 4 and nv:                                   # positions and colours that are not finite or overflow
        hit = rng.random((nv, 3)) < 0.15
        v[hit] = rng.choice(np.array([np.nan, np.inf, -np.inf, 1e30, -1e30], np.float32), int(hit.sum()))
        if c is not None:
            hit = rng.random((nv, 3)) < 0.15
            c[hit] = rng.choice(np.array([np.nan, np.inf, -np.inf, 1e6, -1e6, 32768.0, -32768.0, 32768.004], np.float32), int(hit.sum()))
    elif quirk == 5 and nv:                                   # a power-of-two cell, coordinates exactly on its boundaries
        cell = np.float32(2.0 ** int(rng.integers(-6, 4)))
        origin = np.round(box / cell).astype(np.float32) * cell
        k = rng.integers(-1, np.array(dims) + 2, (nv, 3))
        on = rng.random((nv, 3)) < 0.5
        inside = (origin.astype(np.float64) + rng.random((nv, 3)) * np.array(dims) * float(cell)).astype(np.float32)
        v = np.where(on, (origin.astype(np.float64) + k * float(cell)).astype(np.float32), inside)
        low = rng.random((nv, 3)) < 0.05
        v[low] = (np.broadcast_to(origin, (nv, 3))[low] - np.float32(2.0 ** -20)).astype(np.float32)
        pscale = nf.pscale_of(float(cell) * max(dims))
    elif quirk == 6:                                          # one cell for everything
        dims, cell = (1, 1, 1), np.float32(extent)
        pscale = nf.pscale_of(extent)
    elif quirk == 7 and nv:                                   # the hot row: (nearly) all vertices in one cell of many
        k = rng.random(nv) < 0.95
        v[k] = (v[0].astype(np.float64) + (rng.random((int(k.sum()), 3)) - 0.5) * 1e-3 * float(cell)).astype(np.float32)
    elif quirk == 8:                                          # a quantum so fine that part of the frame passes 2^30 quanta
        pscale = nf.pscale_of(float(cell) * max(dims)) * float(2 ** int(rng.integers(1, 4)))
    counts = None
    if rng.random() < 1.0 / 3:
        counts = [(int(rng.integers(0, nv + 1)), int(rng.integers(0, nk + 1))), (nv, nk), (0, 0), (-1, int(rng.integers(0, nk + 1))),
                  (int(rng.integers(0, nv + 1)), -7), (nv + 1, nk + 1), (INT32_MAX, INT32_MAX)][int(rng.integers(0, 7))]
        tag += f" counts {counts}"
    return tag, v, c, np.ascontiguousarray(f, np.int32), origin, cell, dims, pscale, counts


def _case(rng, dedupe):
    tag, v, c, f, origin, cell, dims, pscale, counts = gen_case(rng, dedupe)
    bad = compare(raw_decimate(v, c, f, origin, cell, dims, pscale, dedupe, counts), nd.decimate(v, c, f, origin, cell, dims, pscale, dedupe, counts))
    return f"{tag} pscale {pscale:g}: {', '.join(bad)}" if bad else None


def case_decimate(rng):
    return _case(rng, False)


def case_dedupe(rng):
    return _case(rng, True)


def case_composed(rng):
    from sfm_mvs_amd import mesh
    tag, S, W, C = gen_field(rng)
    origin, voxel = np.zeros(3, np.float64), 0.5
    wv, wc, wf = np_mesh.extract_mesh(S, W, C, origin.astype(np.float32), np.float32(voxel), 1.0)
    min_faces, largest = thresholds(rng, wf, len(wv)), bool(rng.integers(0, 4) == 0)
    steps, dedupe = int(rng.integers(0, 3)), bool(rng.integers(0, 2))
    cells = float(rng.choice([1.0, 1.5, 2.0, 3.5]))
    dims = S.shape[::-1]
    extent = voxel * (max(dims) - 1)
    v, c, f = mesh.extract_mesh(up(S), up(W), None if C is None else up(C), origin, voxel, 1.0)
    ov, oc, of, counts, status, labels, buf = mesh.clean_mesh(v, c, f, min_faces, largest, packed=True)
    sv = mesh.smooth_mesh(ov, of, steps, origin, extent, counts=counts)        # no host read in between
    fo, fcell, fdims, fext = mesh.decimate_frame(origin, voxel, dims, cells)
    dv, dc, df, dn = mesh.decimate_mesh(sv, oc, of, fo, fcell, fdims, fext, dedupe, counts=counts)
    nr = mesh.mesh_normals(dv, df, counts=dn)
    if int(status[0]) != 1:
        return f"{tag}: not converged at the default rounds"
    kv, kc, kf, _ = npc.clean(wv, wc, wf, min_faces, largest)
    want_v = nf.smooth(kv, kf, nf.taubin_factors(steps), origin.astype(np.float32), nf.pscale_of(extent))
    go, gcell, gdims, gext = nd.frame_of(origin, voxel, dims, cells)
    xv, xc, xf, xn = nd.decimate(want_v, kc, kf, go, gcell, gdims, nf.pscale_of(gext), dedupe)
    want_n = nf.normals(xv, xf)
    bad = []
    if dn.cpu().numpy().tolist() != xn.tolist():
        bad.append(f"counts {dn.cpu().numpy().tolist()} != {xn.tolist()}")
    else:
        k, m = len(xv), len(xf)
        if not np.array_equal(bits(dv)[:k], bits(xv)):
            bad.append("vertices")
        if xc is not None and not np.array_equal(bits(dc)[:k], bits(xc)):
            bad.append("colours")
        if not np.array_equal(bits(df)[:m], xf):
            bad.append("faces")
        if not np.array_equal(bits(nr)[:k], bits(want_n)):
            bad.append("normals")
    return f"{tag} min_faces {min_faces} largest_only {largest} pairs {steps} cells {cells} dedupe {dedupe}: {', '.join(bad)}" if bad else None


FAMILIES = [("decimate", case_decimate, 4), ("dedupe", case_dedupe, 4), ("composed", case_composed, 2)]


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
            log(f"MISMATCH {name} (seed {seed}, case seed {case_seed}; replay: fuzz_mesh_decimate.py 0 0 {name}:{case_seed}) {msg}")
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
        print(f"fuzz_mesh_decimate replay {name}:{case_seed}: {msg or 'no mismatch'}")
        return 1 if msg else 0
    counts, bad, dt = run(budget, seed, log=lambda s: print(s, flush=True))
    print(f"fuzz_mesh_decimate: seed {seed}, {sum(counts.values())} cases {counts}, {bad} mismatches, {dt:.0f} s")
    print(f"sfm_build_id {_lib.build_id()}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
