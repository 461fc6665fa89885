"""Randomised parity sweep of sfm_mvs_fuse on the GPU box: the HIP path (through the C-ABI, into sentinel-padded buffers) vs the float32
restatement tests/np_mvs_fuse.py, every output word (tests/parity_cases.py: floats as int32 views; a NaN equals a NaN).

  python scripts/fuzz_mvs_fuse.py [seconds] [seed] [case_seed]

One case = one random draw: 1..4096 views and frames from 1 x 1 to 32767 a side, all three log-uniform but capped so that the NumPy side
of a case stays well under a second; 0..8 neighbours per view drawn from all views, min_consistent 0..nnbr, tau from 0, unique 0 / 1,
normals and colours each present or absent, cos_min from -inf, -1, 0, cos 30 degrees, 1, +inf; smooth depth maps, normals scattered
about one direction and smooth colours under near-identity motions, so that every branch of the consistency test is taken by many
pixels.  About one case in four carries a degeneracy: NaN / inf / negative / zero depths planted in every map, NaN and zero normals, a view
listed twice, a corrupt table (indices -1, n, the view itself, nnbr 9, 1000 or negative, min_consistent outside 0..nnbr), a neighbour
behind the reference, opposite normals (sums of zero length), whole-pixel motions with exact depths and tau = 0, all-zero maps.
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
import np_mvs_fuse as nf  # noqa: E402
import parity_cases as pc  # noqa: E402
from fuzz_mvs import IDENTITY, frame_size, log_uniform_int  # noqa: E402

F = np.float32
PAD = 64                        # elements in front of and behind every output
SENTINEL_F, SENTINEL_B = -7.25, 0xA5
MAX_TERMS = 1 << 21             # views x slots x pixels of one case (the NumPy side: about 0.1 us a term)
COS30 = float(np.float32(np.cos(np.deg2rad(30.0))))
NAMES = ("mask", "xyz", "normal", "bgr", "support")


def fuse_both(depth, table, normal, bgr, tau, cos_min, unique, check=True):
    """sfm_mvs_fuse (raw C-ABI call into padded buffers) and np_mvs_fuse.fuse -> (got dict, want dict, None or what differs).
    check=False: the device side alone (want is None)."""
    import ctypes
    import torch
    from sfm_mvs_amd import _lib
    depth = np.ascontiguousarray(depth, F)
    n, h, w = depth.shape
    table = np.ascontiguousarray(table)
    assert table.nbytes == 512 * n
    d_dev, t_dev = pc.up(depth), pc.up(table.view(np.uint8).reshape(n, 512))
    n_dev = None if normal is None else pc.up(np.ascontiguousarray(normal, F))
    b_dev = None if bgr is None else pc.up(np.ascontiguousarray(bgr, np.uint8))
    px = n * h * w
    spec = dict(mask=(px, torch.uint8, (n, h, w)), xyz=(3 * px, torch.float32, (n, h, w, 3)), support=(px, torch.uint8, (n, h, w)))
    if normal is not None:
        spec["normal"] = (3 * px, torch.float32, (n, h, w, 3))
    if bgr is not None:
        spec["bgr"] = (3 * px, torch.uint8, (n, h, w, 3))
    bufs = {k: torch.full((cnt + 2 * PAD,), SENTINEL_F if dt == torch.float32 else SENTINEL_B, dtype=dt, device="cuda")
            for k, (cnt, dt, _) in spec.items()}
    at = lambda k: ctypes.c_void_p(bufs[k].data_ptr() + PAD * bufs[k].element_size()) if k in bufs else None  # noqa: E731
    _lib.check(_lib.lib().sfm_mvs_fuse(_lib.ptr(d_dev), _lib.ptr(n_dev), _lib.ptr(b_dev), _lib.ptr(t_dev), n, w, h, float(tau), float(cos_min),
                                       int(unique), at("mask"), at("xyz"), at("normal"), at("bgr"), at("support"), _lib.stream_ptr()),
               "sfm_mvs_fuse")
    got, bad = {}, None
    for k, (cnt, dt, shape) in spec.items():
        flat = bufs[k].cpu().numpy()
        sent = F(SENTINEL_F) if dt == torch.float32 else np.uint8(SENTINEL_B)
        if not (np.all(flat[:PAD] == sent) and np.all(flat[-PAD:] == sent)):
            bad = bad or f"{k}: written outside its extent"
        got[k] = flat[PAD:-PAD].reshape(shape)
    if not check:
        return got, None, bad
    want = nf.fuse(depth, table, normal, bgr, tau, cos_min, unique)
    for k in NAMES:
        if bad is None and want[k] is not None and not pc.same(got[k], want[k]):
            bad = k
    return got, want, bad


def smooth_maps(rng, n, h, w, hole=0.1):
    """n noisy copies of one smooth depth surface (about 4 units away), with holes."""
    ys, xs = np.mgrid[0:h, 0:w]
    base = (4.0 + 0.01 * xs - 0.02 * ys + 0.5 * np.sin(xs / 7.0) * np.cos(ys / 5.0)).astype(F)
    out = np.empty((n, h, w), F)
    for i in range(n):
        out[i] = base * (1 + float(rng.choice([0.0, 0.002, 0.02])) * rng.standard_normal((h, w)))
        out[i][rng.random((h, w)) < hole] = 0
    return out


def unit_normals(rng, n, h, w, spread):
    v = np.array([0.2, -0.3, -1.0]) + spread * rng.standard_normal((n, h, w, 3))
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(F)


def random_table(rng, n, max_slots=8):
    """Near-identity motions with sub-pixel to few-pixel shifts between any two views -> int32 [n, 128]."""
    nbrs, mins, bcs, abs_ = [], [], [], []
    for i in range(n):
        k = int(rng.integers(0, min(max_slots, 8) + 1))
        row = [int(v) + (int(v) >= i) for v in rng.integers(0, n - 1, k)] if n > 1 else []      # any view but i; repeats may occur
        ab = np.tile(IDENTITY, (len(row), 1))
        ab[:, :9] += rng.normal(0, 1e-4, (len(row), 9)).astype(F)
        ab[:, 9:] = rng.normal(0, [2.0, 2.0, 0.02], (len(row), 3)).astype(F)
        nbrs.append(row); abs_.append(ab); mins.append(int(rng.integers(0, len(row) + 1)))
        bcs.append((IDENTITY + np.concatenate([rng.normal(0, 0.01, 9), rng.normal(0, 1.0, 3)])).astype(F))
    return nf.make_table(nbrs, mins, bcs, abs_)


def gen_case(rng):
    n = log_uniform_int(rng, 1, 4096 if rng.random() < 0.1 else 48)       # (the NumPy side loops over views x slots)
    slots = int(rng.integers(0, 9))
    w, h = frame_size(rng, 1, 32767, max(1, MAX_TERMS // (n * max(slots, 1))))
    tau = float(rng.choice([0.0, 0.001, 0.01, 0.1])); unique = int(rng.integers(0, 2))
    cos_min = float(rng.choice([-np.inf, -1.0, 0.0, COS30, 0.999, 1.0, np.inf]))
    depth = smooth_maps(rng, n, h, w)
    normal = unit_normals(rng, n, h, w, float(rng.choice([0.0, 0.05, 0.4]))) if rng.random() < 0.7 else None
    bgr = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8) if rng.random() < 0.7 else None
    table = random_table(rng, n, slots)
    quirk = int(rng.integers(0, 9)) if rng.random() < 0.25 else -1
    i = int(rng.integers(0, n))
    if quirk == 0:
        depth = pc.plant_specials(depth, rng)
    elif quirk == 1 and normal is not None:
        normal = pc.plant_specials(normal, rng, values=(np.nan, 0.0, np.inf))
    elif quirk == 2 and table[i, nf.W_NNBR] >= 2:
        s = nf.W_AB
        table[i, nf.W_NBR + 1] = table[i, nf.W_NBR]
        table[i, s + 12:s + 24] = table[i, s:s + 12]
    elif quirk == 3:
        for v in range(n):
            table[v, nf.W_NBR:nf.W_NBR + 8] = rng.choice([-1, n, v, -(1 << 31), (1 << 31) - 1, int(rng.integers(0, n))], 8)
            table[v, nf.W_NNBR] = int(rng.choice([9, 1000, -3, 8, (1 << 31) - 1]))
            table[v, nf.W_MIN] = int(rng.choice([-1, 0, 1, 9, 1 << 30]))
            table.view(F)[v, nf.W_AB:nf.W_AB + 96] = np.tile(IDENTITY, 8) + rng.normal(0, 1e-4, 96).astype(F)
    elif quirk == 4 and table[i, nf.W_NNBR] >= 1:
        f = table.view(F)
        f[i, nf.W_AB + 6:nf.W_AB + 9] = -f[i, nf.W_AB + 6:nf.W_AB + 9]
        f[i, nf.W_AB + 11] = F(rng.choice([-1.0, 4.0]))
    elif quirk == 5 and normal is not None:
        normal[1::2] = -normal[0]                               # odd views face away from the even ones: sums of zero length
        normal[0::2] = normal[0]
        cos_min = -np.inf
    elif quirk in (6, 7):                                       # whole-pixel motions, exact depths: tau = 0 keeps equal depths only
        depth[:] = F(4.0) if quirk == 6 else np.round(depth * 4) / 4
        f = table.view(F)
        for v in range(n):
            for s in range(8):
                a = IDENTITY.copy()
                a[9:11] = F(4.0) * rng.integers(-2, 3, 2).astype(F) * (F(1.0) if quirk == 6 else F(0.5))
                f[v, nf.W_AB + 12 * s:nf.W_AB + 12 * s + 12] = a
        tau = 0.0
    elif quirk == 8:
        depth[rng.integers(0, n)] = 0
        if rng.random() < 0.3:
            depth[:] = 0
    tag = (f"{n} views {w} x {h} slots <= {slots} tau {tau} cos_min {cos_min} unique {unique} normals {normal is not None} "
           f"colours {bgr is not None} quirk {quirk}")
    return tag, (depth, table, normal, bgr, tau, cos_min, unique)


def case(rng):
    tag, args = gen_case(rng)
    _, _, bad = fuse_both(*args)
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
            log(f"MISMATCH (seed {seed}, case seed {case_seed}; replay: fuzz_mvs_fuse.py 0 0 {case_seed}) {msg}")
    return count, bad, time.time() - t0


def main():
    import sfm_mvs_amd
    from sfm_mvs_amd import _lib
    budget = float(sys.argv[1]) if len(sys.argv) > 1 else 120.0
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    sfm_mvs_amd.lib()
    if len(sys.argv) > 3:                               # replay one case
        msg = case(np.random.default_rng(int(sys.argv[3])))
        print(f"fuzz_mvs_fuse replay {sys.argv[3]}: {msg or 'no mismatch'}")
        return 1 if msg else 0
    count, bad, dt = run(budget, seed, log=lambda m: print(m, flush=True))
    print(f"fuzz_mvs_fuse: seed {seed}, {count} cases, {bad} mismatches, {dt:.0f} s")
    print(f"sfm_build_id {_lib.build_id()}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
