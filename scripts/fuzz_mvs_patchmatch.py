"""Randomised parity sweep of sfm_mvs_patchmatch on the GPU box: the HIP path (through the C-ABI, into sentinel-padded buffers) vs the
float32 restatement tests/np_mvs_patchmatch.py, bit for bit (tests/parity_cases.py: int32 views; a NaN equals a NaN).

  python scripts/fuzz_mvs_patchmatch.py [seconds] [seed] [case_seed]

One case = one random draw: radius 1..4, 1..8 sources, topk 1..nsrc, iters 0..3 (now and then up to 16), far 0 / 1, steps from a short
list, any seed; the frame log-uniform over 2r+1 .. 32767 per side but capped in area so that the NumPy side of a case stays around a
second; crops of a rendered scene with its real matrices (the start: none, the noisy truth, or zeros) or textures shifted by whole
pixels under near-identity matrices.  About one case in four carries a degeneracy: a source behind every plane, NaN / inf matrix rows,
flat or checkerboard frames, one source passed nsrc times, cost_max <= 0, >= 2 or infinite, qmin = qmax, NaN / inf / negative / zero
depths planted in the start, both steps zero.
Inputs stay inside the contract of include/sfm_hip.h.  The script stops at the first mismatch, prints the case's parameters and its case
seed (gen_case(np.random.default_rng(case_seed)) rebuilds the inputs without a GPU; the third argument replays one case), and exits
non-zero.
"""
import os
import sys
import time

os.environ.setdefault("OMP_WAIT_POLICY", "passive")

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)
import np_mvs_patchmatch as npm  # noqa: E402
import parity_cases as pc  # noqa: E402
from fuzz_mvs import IDENTITY, frame_size  # noqa: E402

F = np.float32
SECONDS_PER_SAMPLE = 2e-7       # the NumPy side, per pixel x source x window sample x evaluated plane
PAD, SENTINEL = 64, -7.25       # floats in front of and behind every output (64 floats keep the state 16-byte aligned)
NAMES = ("state", "depth", "cost", "normal")


def patchmatch_both(ref, srcs, mv, qmin, qmax, r, topk, var_min, cost_max, depth_init, iters, far, depth_step, slope_step, seed, nmat):
    """sfm_mvs_patchmatch (raw C-ABI call into padded buffers) and np_mvs_patchmatch.patchmatch -> (want, None or what differs)."""
    import ctypes
    import torch
    from sfm_mvs_amd import _lib
    h, w = ref.shape
    dev = {}
    srcs_dev = [dev.setdefault(id(s), pc.up(s)) for s in srcs]              # a frame passed twice is one device buffer passed twice
    ref_dev = pc.up(ref)
    init_dev = None if depth_init is None else pc.up(np.ascontiguousarray(depth_init, F))
    mv = np.ascontiguousarray(mv, F).reshape(-1, 12)
    nm = None if nmat is None else np.ascontiguousarray(nmat, F)
    sizes = dict(state=h * w * 4, depth=h * w, cost=h * w, normal=h * w * 3)
    bufs = {k: torch.full((n + 2 * PAD,), SENTINEL, dtype=torch.float32, device="cuda") for k, n in sizes.items() if k != "normal" or nm is not None}
    at = lambda k: ctypes.c_void_p(bufs[k].data_ptr() + 4 * PAD) if k in bufs else None  # noqa: E731
    src_ptrs = (ctypes.c_void_p * len(srcs_dev))(*[s.data_ptr() for s in srcs_dev])
    _lib.check(_lib.lib().sfm_mvs_patchmatch(_lib.ptr(ref_dev), src_ptrs, mv.ctypes.data_as(ctypes.c_void_p), len(srcs_dev), w, h, float(qmin),
                                             float(qmax), int(r), int(topk), float(var_min), float(cost_max), _lib.ptr(init_dev), int(iters),
                                             int(far), float(depth_step), float(slope_step), int(seed),
                                             None if nm is None else nm.ctypes.data_as(ctypes.c_void_p), at("state"), at("depth"), at("cost"),
                                             at("normal"), _lib.stream_ptr()), "sfm_mvs_patchmatch")
    with np.errstate(all="ignore"):
        want = npm.patchmatch(ref, srcs, mv, qmin, qmax, r, topk, var_min, cost_max, depth_init, iters, far, depth_step, slope_step, seed, nm)
    shapes = dict(state=(h, w, 4), depth=(h, w), cost=(h, w), normal=(h, w, 3))
    for k, wv in zip(NAMES, want):
        if wv is None:
            continue
        flat = bufs[k].cpu().numpy()
        if not (np.all(flat[:PAD] == F(SENTINEL)) and np.all(flat[-PAD:] == F(SENTINEL))):
            return want, f"{k}: written outside its extent"
        if not pc.same(flat[PAD:-PAD].reshape(shapes[k]), wv):
            return want, k
    return want, None


def gen_case(rng):
    from sfm_mvs_amd import mvs
    r = int(rng.integers(1, 5)); nsrc = int(rng.integers(1, 9)); topk = int(rng.integers(1, nsrc + 1))
    iters = int(rng.integers(0, 4)) if rng.random() < 0.9 else int(rng.integers(4, 17))
    far = int(rng.integers(0, 2))
    depth_step = float(rng.choice([0.0, 0.05, 0.1, 0.2, 1.5])); slope_step = float(rng.choice([0.0, 1e-3, 7e-3, 0.05]))
    seed = int(rng.integers(0, 1 << 32))
    w, h = frame_size(rng, 2 * r + 1, 32767, int(0.6 / (nsrc * (1 + 11 * iters) * (2 * r + 1) ** 2 * SECONDS_PER_SAMPLE)))
    var_min = float(rng.choice([1.0, 50.0, 150.0, 1000.0])); cost_max = float(rng.uniform(0.1, 1.0))
    kind = "scene" if (w <= 192 and h <= 93 and rng.random() < 0.7) else "shift"
    depth_init = None
    if kind == "scene":
        grays, K, P, gt, _ = pc.scene(n=9, w=192, h=93, seed=3, arc=float(rng.choice([0.3, 0.8])))
        x0, y0 = int(rng.integers(0, 192 - w + 1)), int(rng.integers(0, 93 - h + 1))
        g, Kc, Pc = pc.crop(grays, K, P, x0, y0, w, h)
        i = int(rng.integers(0, 9)); nb = mvs.neighbours(i, 9, nsrc)
        ref, srcs, mv = g[i], [g[v] for v in nb], mvs.sweep_matrices(Kc, Pc[i], Pc[nb])
        qmin, qmax = F(1.0 / rng.uniform(6.0, 14.0)), F(1.0 / rng.uniform(0.8, 3.0))
        nmat = mvs.normal_matrix(Kc, Pc[i]) if rng.random() < 0.8 else None
        start = int(rng.integers(0, 3))
        if start == 1:
            depth_init = (gt[i][y0:y0 + h, x0:x0 + w] * (1 + 0.02 * rng.standard_normal((h, w)))).astype(F)
        elif start == 2:
            depth_init = np.zeros((h, w), F)
    else:
        pad = 4
        big = pc.texture(h + 2 * pad, w + 2 * pad, int(rng.integers(1 << 30)))
        ref = np.ascontiguousarray(big[pad:pad + h, pad:pad + w])
        qmin, qmax = F(0.1), F(0.5)
        srcs, mv = [], np.tile(IDENTITY, (nsrc, 1))
        for s in range(nsrc):
            sx, sy = (int(v) for v in rng.integers(-pad, pad + 1, 2))
            srcs.append(np.ascontiguousarray(big[pad - sy:pad - sy + h, pad - sx:pad - sx + w]))      # src[y + sy, x + sx] = ref[y, x]
            mv[s, 9:11] = np.array([sx, sy], F) / F(rng.uniform(0.1, 0.5))
            if rng.random() < 0.5:
                mv[s, :9] += rng.normal(0, 1e-4, 9).astype(F)
        nmat = rng.normal(0, 1, 9).astype(F) if rng.random() < 0.8 else None
        if rng.random() < 0.5:
            depth_init = rng.uniform(1.5, 12.0, (h, w)).astype(F)           # partly outside 1/qmax .. 1/qmin = 2 .. 10
    quirk = int(rng.integers(0, 10)) if rng.random() < 0.25 else -1
    s = int(rng.integers(0, nsrc))
    if quirk == 0:
        mv[s] = -mv[s]
    elif quirk == 1:
        mv[s, 3 * int(rng.integers(0, 4)):][:3] = F(rng.choice([np.nan, np.inf, -np.inf]))
    elif quirk == 2:
        flat = np.full((h, w), int(rng.choice([0, 128, 255])), np.uint8)
        if rng.random() < 0.5:
            ref = flat
        else:
            srcs = [flat for _ in srcs]
    elif quirk == 3:
        ys, xs = np.mgrid[0:h, 0:w]
        ref = (((xs + ys) & 1) * 255).astype(np.uint8); srcs = [ref for _ in srcs]
    elif quirk == 4:
        srcs = [srcs[s]] * nsrc; mv = np.repeat(mv[s:s + 1], nsrc, 0)
    elif quirk in (5, 6):
        cost_max = float(rng.choice([-1.0, 0.0, 2.0, 2.5, np.inf, -np.inf]))
    elif quirk == 7:
        qmax = qmin
    elif quirk == 8:
        depth_init = pc.plant_specials(depth_init if depth_init is not None else np.full((h, w), 4.0, F), rng, fraction=0.05)
    elif quirk == 9:
        depth_step = slope_step = 0.0
    tag = (f"{w} x {h} {kind} r {r} nsrc {nsrc} topk {topk} iters {iters} far {far} steps {depth_step} {slope_step} seed {seed} q {qmin}..{qmax} "
           f"var_min {var_min} cost_max {cost_max} start {'none' if depth_init is None else 'map'} normals {nmat is not None} quirk {quirk}")
    return tag, (ref, srcs, np.ascontiguousarray(mv, F), float(qmin), float(qmax), r, topk, var_min, cost_max, depth_init, iters, far, depth_step,
                 slope_step, seed, nmat)


def case(rng):
    tag, args = gen_case(rng)
    _, bad = patchmatch_both(*args)
    return None if bad is None else f"{tag}: {bad} differs"


def run(budget, seed, log=print):
    """Cases until `budget` seconds have passed or one mismatches -> (cases, mismatches, seconds)."""
    rng = np.random.default_rng(seed)
    t0 = time.time(); count = bad = 0
    while time.time() - t0 < budget and not bad:
        case_seed = int(rng.integers(1 << 31))
        try:
            msg = case(np.random.default_rng(case_seed))
        except Exception as e:  # noqa: BLE001
            msg = f"EXCEPTION {e!r}"[:300]
        count += 1
        if msg:
            bad += 1
            log(f"MISMATCH (seed {seed}, case seed {case_seed}; replay: fuzz_mvs_patchmatch.py 0 0 {case_seed}) {msg}")
    return count, bad, time.time() - t0


def main():
    import sfm_mvs_amd
    from sfm_mvs_amd import _lib
    budget = float(sys.argv[1]) if len(sys.argv) > 1 else 120.0
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    sfm_mvs_amd.lib()
    if len(sys.argv) > 3:                               # replay one case
        msg = case(np.random.default_rng(int(sys.argv[3])))
        print(f"fuzz_mvs_patchmatch replay {sys.argv[3]}: {msg or 'no mismatch'}")
        return 1 if msg else 0
    count, bad, dt = run(budget, seed, log=lambda m: print(m, flush=True))
    print(f"fuzz_mvs_patchmatch: seed {seed}, {count} cases, {bad} mismatches, {dt:.0f} s")
    print(f"sfm_build_id {_lib.build_id()}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
