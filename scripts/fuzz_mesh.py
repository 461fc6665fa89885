"""Randomised parity sweep of the mesh kernels on the GPU box: HIP path (through the C-ABI) vs the float32 restatement
tests/np_mesh.py, bit for bit (tests/parity_cases.py: int32 views; a NaN equals a NaN).

  python scripts/fuzz_mesh.py [seconds] [seed] [family:case_seed]

Families (one case = one random draw; the grid's point count log-uniform from 8 up to a cap that keeps the NumPy side of a case
around a second — the documented limit is 2^27 —, split at random into three sides >= 2; about one case in four carries one of
the degeneracies of tests/test_gpu_mesh_limits.py):
  tsdf      sfm_tsdf_integrate: 0..8 views of 1 x 1 .. 200 x 200 pixels looking at the grid, smooth positive depth maps, with and
            without masks, colours and sums to continue (random non-integers).  One case in eight is a 2 x 2 x nz line of more
            than 2^20 tiles (the grid-stride loop).  Degeneracies: NaN / +-inf / negative / zero depth samples, a grid that
            reaches behind the cameras, P = [I|0] with voxel, trunc and depth exact binary fractions (sdf == +-trunc), no views.
  extract   sfm_mesh_count + sfm_mesh_extract: random fields (some points unknown), spheres, with and without colour, w_min 1, 2,
            3.5; one case in four has ceil(n / 256) = 1023, 1024 or 1025 (the scan's segment length changes there).  The totals
            are also checked against parity_cases.counts_by_boolean_arithmetic.  Degeneracies: +-0, NaN, +-inf planted in S, a
            side of 2, nothing known, everything inside.
  capacity  sfm_mesh_extract with max_vertices in 0..count and max_faces in 0..count, into buffers of the full counted size
            filled with a sentinel (NULL outputs for a capacity of 0 in half of those cases): the prefix is the full result's,
            nothing past the capacity is written, the status is SFM_OK.
Inputs stay inside the contract of include/sfm_hip.h.  The script stops at the first mismatch, prints the family, the case's
parameters and its case seed (gen_<family>(np.random.default_rng(case_seed)) rebuilds the inputs without a GPU; the third
argument replays one case), and exits non-zero.  An exception on either side is a mismatch.
"""
import os
import sys
import time

os.environ.setdefault("OMP_WAIT_POLICY", "passive")

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import parity_cases as pc
from mvs_scenes import look_at

F = np.float32
GRID_LIMIT = 1 << 20


def log_uniform_int(rng, lo, hi):
    return int(np.clip(np.floor(np.exp(rng.uniform(np.log(lo), np.log(hi + 1)))), lo, hi))


def grid_dims(rng, max_points):
    """(nx, ny, nz) with about log-uniform(8 .. max_points) points, split at random; one time in five a side is 2."""
    n = log_uniform_int(rng, 8, max_points)
    nx = 2 if rng.random() < 0.2 else log_uniform_int(rng, 2, max(2, n // 4))
    ny = 2 if rng.random() < 0.2 else log_uniform_int(rng, 2, max(2, n // (2 * nx)))
    dims = [nx, ny, max(2, n // (nx * ny))]
    rng.shuffle(dims)
    return tuple(int(d) for d in dims)


def gen_tsdf(rng):
    nview = int(rng.integers(0, 9))
    w, h = log_uniform_int(rng, 1, 200), log_uniform_int(rng, 1, 200)
    line = rng.random() < 0.125
    if line:
        nview = min(nview, 2)
        dims = (2, 2, GRID_LIMIT + log_uniform_int(rng, 1, GRID_LIMIT // 2))
    else:
        dims = grid_dims(rng, int(1.2e7) // max(nview, 1) // 4)
    extent = 3.0
    voxel = extent / max(dims)
    origin = -0.5 * voxel * (np.array(dims, np.float64) - 1) + rng.normal(0, 0.05, 3)
    f = 0.9 * max(w, h)
    K = np.array([[f, 0.0, (w - 1) / 2.0], [0.0, f, (h - 1) / 2.0], [0.0, 0.0, 1.0]])
    P, depth = [], []
    ys, xs = np.mgrid[0:h, 0:w]
    for v in range(nview):
        a = rng.uniform(-0.6, 0.6)
        R, t = look_at([4.0 * np.sin(a), rng.uniform(-0.5, 0.5), -4.0 * np.cos(a)], rng.normal(0, 0.2, 3))
        P.append(K @ np.hstack([R, t[:, None]]))
        d = 4.0 + 0.8 * np.sin(xs / max(w, 2) * 5.0 + v) * np.cos(ys / max(h, 2) * 4.0) + 0.02 * rng.standard_normal((h, w))
        d[rng.random((h, w)) < 0.05] = 0.0
        depth.append(d)
    depth = np.asarray(depth, F).reshape(nview, h, w)
    P = np.asarray(P, np.float64).reshape(nview, 12).astype(F)
    trunc = float(rng.choice([2.0 * voxel, 5.0 * voxel, 0.1 * extent, 0.5 * extent]))
    quirk = int(rng.integers(0, 4)) if rng.random() < 0.25 else -1
    if quirk == 0:
        depth = pc.plant_specials(depth, rng, fraction=0.04)
    elif quirk == 1:
        origin[2] -= 4.0 + 0.5 * voxel * (dims[2] - 1)                 # the lattice straddles the cameras' plane z = -4
    elif quirk == 2 and nview:
        e = int(rng.integers(1, 4))
        voxel, trunc, origin = 2.0 ** -e, 2.0 ** (1 - e) * int(rng.integers(1, 3)), np.array([0.0, 0.0, 3.0])
        P[:] = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F)
        depth[:] = F(3.0 + 0.25 * int(rng.integers(1, 12)))
    elif quirk == 3:
        nview, depth, P = 0, depth[:0], P[:0]
    mask = bgr = S = W = C = None
    if rng.random() < 0.5:
        mask = ((rng.random(depth.shape) < 0.8) * rng.integers(1, 255, depth.shape)).astype(np.uint8)
    if rng.random() < 0.5:
        bgr = rng.integers(0, 256, depth.shape + (3,)).astype(np.uint8)
    if rng.random() < 0.35 or quirk == 3:
        shape = dims[::-1]
        S, W = rng.normal(0, 2, shape).astype(F), rng.uniform(0, 3, shape).astype(F)
        if bgr is not None:
            C = rng.uniform(0, 700, shape + (4,)).astype(F)
    tag = (f"grid {dims} nview {nview} frame {w} x {h} voxel {voxel} trunc {trunc} mask {mask is not None} bgr {bgr is not None} "
           f"continued {S is not None} quirk {quirk}")
    return tag, (depth, P, origin, voxel, dims, trunc), dict(mask=mask, bgr=bgr, S=S, W=W, C=C)


def case_tsdf(rng):
    tag, args, kw = gen_tsdf(rng)
    _, bad = pc.tsdf_both(*args, **kw)
    return None if bad is None else f"{tag}: {bad} differs"


def gen_field(rng, max_points):
    if rng.random() < 0.25 and max_points >= 1025 * 256:
        dims = pc.dims_with_blocks(int(rng.choice([1023, 1024, 1025])), rng)
    else:
        dims = grid_dims(rng, max_points)
    kind = str(rng.choice(["random", "random", "sphere"]))
    color = bool(rng.integers(0, 2))
    if kind == "sphere":
        nx, ny, nz = dims
        z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
        c = [rng.uniform(0, d) for d in dims]
        Fv = (np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - rng.uniform(0.5, 0.5 * max(dims))).astype(F)
        W = rng.integers(0 if rng.random() < 0.5 else 1, 5, Fv.shape).astype(F)
        S = (Fv * W).astype(F)
        C = np.concatenate([rng.uniform(0, 2000, S.shape + (3,)), rng.integers(0, 3, S.shape + (1,))], -1).astype(F) if color else None
    else:
        S, W, C = pc.random_field(dims, rng, unknown=float(rng.choice([0.0, 0.1, 0.5])), color=color)
    quirk = int(rng.integers(0, 3)) if rng.random() < 0.25 else -1
    if quirk == 0:
        S = pc.plant_specials(S, rng, fraction=0.02, values=(0.0, -0.0, np.nan, np.inf, -np.inf))
    elif quirk == 1:
        W = np.zeros_like(W)
    elif quirk == 2:
        S = -np.abs(S) - F(0.1)
        W = np.maximum(W, F(4))
    w_min = float(rng.choice([1.0, 2.0, 3.5]))
    origin = rng.normal(0, 2, 3)
    voxel = float(rng.choice([0.01, 0.37, 1.0, 25.0]))
    return f"grid {dims} {kind} color {color} w_min {w_min} voxel {voxel} quirk {quirk}", (S, W, C, origin, voxel, w_min)


def case_extract(rng):
    tag, args = gen_field(rng, 300000)
    want, counts, bad = pc.extract_both(*args)
    if bad is None and counts != pc.counts_by_boolean_arithmetic(args[0], args[1], args[5]):
        bad = "the count that goes through no scan"
    return None if bad is None else f"{tag}: {bad} differs"


def case_capacity(rng):
    tag, (S, W, C, origin, voxel, w_min) = gen_field(rng, 30000)
    with np.errstate(all="ignore"):
        wv, wc, wf = pc.np_mesh.extract_mesh(S, W, C, np.asarray(origin, np.float64).astype(F), F(voxel), w_min)
    nv, nt = len(wv), len(wf)
    mv, mf = int(rng.integers(0, nv + 1)), int(rng.integers(0, nt + 1))
    if rng.random() < 0.3:
        mv = int(rng.choice([0, min(1, nv), max(nv - 1, 0), nv]))
    if rng.random() < 0.3:
        mf = int(rng.choice([0, min(1, nt), max(nt - 1, 0), nt]))
    null = bool(rng.integers(0, 2))
    tag += f" counts {nv} {nt} max_vertices {mv} max_faces {mf} null {null}"
    rc, *part = pc.extract_with_capacity(S, W, C, origin, voxel, w_min, nv, nt, mv, mf, null_outputs=null)
    if rc != 0:
        return f"{tag}: status {rc}"
    full = [pc.bits(wv), None if wc is None else pc.bits(wc), wf]
    part = [pc.bits(part[0].view(F)), None if part[1] is None else pc.bits(part[1].view(F)), part[2]]
    sentinel_f = pc.bits(np.array([pc.SENTINEL]).view(F))[0]
    assert sentinel_f == pc.SENTINEL                     # (the sentinel is not a NaN pattern: canonicalising leaves it alone)
    if null:
        full = [None if mv == 0 else full[0], None if mv == 0 else full[1], None if mf == 0 else full[2]]
    bad = pc.capacity_difference(full, part, nv, nt, mv, mf)
    return None if bad is None else f"{tag}: {bad}"


FAMILIES = [("tsdf", case_tsdf, 4), ("extract", case_extract, 4), ("capacity", case_capacity, 2)]


def main():
    import sfm_mvs_amd
    from sfm_mvs_amd import _lib
    budget = float(sys.argv[1]) if len(sys.argv) > 1 else 120.0
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    sfm_mvs_amd.lib()
    fns = {name: fn for name, fn, _ in FAMILIES}
    if len(sys.argv) > 3:                               # replay one case
        name, case_seed = sys.argv[3].split(":")
        msg = fns[name](np.random.default_rng(int(case_seed)))
        print(f"fuzz_mesh replay {name}:{case_seed}: {msg or 'no mismatch'}")
        return 1 if msg else 0
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
            print(f"MISMATCH {name} (seed {seed}, case seed {case_seed}; replay: fuzz_mesh.py 0 0 {name}:{case_seed}) {msg}", flush=True)
    print(f"fuzz_mesh: seed {seed}, {sum(counts.values())} cases {counts}, {bad} mismatches, {time.time() - t0:.0f} s")
    print(f"sfm_build_id {_lib.build_id()}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
