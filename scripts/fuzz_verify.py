"""Randomised parity sweep of the VERIFY family on the GPU box: sfm_verify_survivors / _samples / _models / _score / _select and
verify.verify_pairs (through sfm_mvs_amd.verify, into sentinel-filled buffers where the extent matters) vs the restatement
tests/np_verify.py; every output word compared exactly (floats as integer views, a NaN equals a NaN).

  python scripts/fuzz_verify.py [seconds] [seed] [family:case_seed]

Families (one case = one random draw; sizes log-uniform from 0 up to a cap that keeps the host solvers of the NumPy side under a second):
  survivors   fuzz_tracks' random match stores (train indices from -1 to past the image, exact ties d0 == ratio * d1, inf, NaN, no
              second neighbour), nq below, at and above cap, pairs i == j and pairs that name images outside the range
  samples     survivor counts from 0 over 4, 5, 6 to 2^31 - 1, budgets 1..1024, random seeds
  models      random and planted five-tuples, slots of -1 and past m, survivors that name no node
  score       the restatement's models (some passed in twice: ties) over planted pairs, m around the LDS tile of 256
  select      the restatement's best keys, keys of 0 and keys that name no slot
  composed    verify.verify_pairs against the restated composition on planted multi-image scenes
One case in four carries a degeneracy: no points, every keypoint equal, collinear keypoints, NaN, inf and huge coordinates, cap = 0.
The script stops at the first mismatch, prints the family and the case seed that rebuilds the inputs without a GPU, exits non-zero, and
ends with one JSON line."""
import json
import os
import sys
import time

os.environ.setdefault("OMP_WAIT_POLICY", "passive")

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "scripts"))
import fuzz_tracks as ft
import np_verify as nv
from fuzz_tracks import SENTINEL, dev, log_uniform_from_zero

INT32_MAX = 2 ** 31 - 1


def same(name, got, want):
    """'' when got equals want word for word; a NaN equals a NaN."""
    import torch
    g = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    w = np.asarray(want)
    if g.shape != w.shape:
        return f"{name}: shape {g.shape} vs {w.shape}"
    if g.dtype.kind == "f" or w.dtype.kind == "f":
        g, w = g.astype(np.float64, copy=False), w.astype(np.float64, copy=False)
        eq = (g.view(np.int64) == w.view(np.int64)) | (np.isnan(g) & np.isnan(w))
    else:
        eq = g.astype(np.int64) == w.astype(np.int64) if g.dtype != np.uint64 and w.dtype != np.uint64 else g.astype(np.uint64) == w.astype(np.uint64)
    if not eq.all():
        return f"{name}: differs at {np.argwhere(~eq)[:3].tolist()} of {g.shape}"
    return ""


def first(*msgs):
    return next((m for m in msgs if m), "")


def flat_out(shape, dtype, pad=5):
    """A tensor of `shape` carved from a sentinel-filled buffer with `pad` words after it -> (tensor, check())."""
    import torch
    n = int(np.prod(shape))
    words = n * (torch.empty(0, dtype=dtype).element_size() // 4 if dtype != torch.uint8 else 1)
    if dtype == torch.uint8:
        buf = torch.full((n + pad,), 0x5A, dtype=torch.uint8, device="cuda")
        return buf[:n].view(shape), lambda: "" if bool((buf[n:] == 0x5A).all()) else "written past the end"
    buf = torch.full((words + pad,), SENTINEL, dtype=torch.int32, device="cuda")
    return buf[:words].view(dtype).view(shape), lambda: "" if bool((buf[words:] == SENTINEL).all()) else "written past the end"


# ---- scenes -------------------------------------------------------------------------------------------------------------------

def gen_scene(rng, max_pts=300, max_pairs=3):
    """A planted multi-image scene with wrong matches -> dict(store, nq, pairs, img_off, kp, K, ratio)."""
    from datagen import load_pose_csv, project, ring_cameras
    from scipy.spatial.transform import Rotation
    deg = int(rng.integers(7)) if rng.integers(4) == 0 else -1
    K, _ = load_pose_csv()
    n_img = int(rng.choice([2, 3, 5]))
    ring = ring_cameras(8)
    n_pts = 0 if deg == 0 else log_uniform_from_zero(rng, max_pts)
    X = rng.normal(size=(n_pts, 3))
    X = X / np.maximum(np.linalg.norm(X, axis=1, keepdims=True), 1.0) * rng.uniform(0.2, 1.0, (n_pts, 1))
    kps, where = [], []
    for i in range(n_img):
        P = K @ np.c_[Rotation.from_rotvec(ring[i, :3]).as_matrix(), ring[i, 3:]]
        x = project(P, X)[0] + rng.normal(0, 0.5, (n_pts, 2)) if n_pts else np.zeros((0, 2))
        nc = int(rng.integers(0, 20))
        x = np.vstack([x, rng.uniform([1, 1], [967, 647], (nc, 2))])
        order = rng.permutation(len(x))
        w = np.empty(len(x), np.int64)
        w[order] = np.arange(len(x))
        kps.append(x[order].astype(np.float32))
        where.append(w)                                             # where[i][point] = its keypoint in image i
    if deg == 1:
        kps = [np.full_like(k, 123.25) for k in kps]
    if deg == 2:
        kps = [np.stack([k[:, 0], 0.5 * k[:, 0] + 7], 1).astype(np.float32) for k in kps]
    if deg == 3:
        for k in kps:
            k[rng.random(len(k)) < 0.2] = np.nan
    if deg == 4:
        for k in kps:
            k[rng.random(len(k)) < 0.2] = rng.choice([np.inf, -np.inf, 3e38, 1e30])
    sizes = np.array([len(k) for k in kps])
    cap = 0 if deg == 5 else int(sizes.max() + rng.integers(-2, 3)) if sizes.max() > 2 else int(sizes.max())
    n_pairs = int(rng.integers(0 if deg == 6 else 1, max_pairs + 1))
    pairs = np.array([rng.choice(n_img, 2, replace=False) for _ in range(n_pairs)], np.int32).reshape(-1, 2)
    if n_pairs and rng.integers(4) == 0:
        pairs[rng.integers(n_pairs)] = rng.choice([[0, 0], [-1, 1], [1, n_img], [INT32_MAX, 0]])
    store = np.zeros((n_pairs, 2, cap, 2), np.int32)
    nq = np.zeros(n_pairs, np.int32)
    for p, (i, j) in enumerate(pairs):
        ii, jj = int(np.clip(i, 0, n_img - 1)), int(np.clip(j, 0, n_img - 1))
        nq[p] = min(sizes[ii], cap) if rng.integers(4) else rng.integers(-1, cap + 3)
        t = rng.integers(-1, sizes[jj] + 2, cap)
        pt = np.full(sizes[ii], -1)
        pt[where[ii][:n_pts]] = np.arange(n_pts)                    # the point keypoint q of image ii shows
        q = np.arange(min(cap, sizes[ii]))
        good = (pt[q] >= 0) & (rng.random(len(q)) < 0.8)
        t[q[good]] = where[jj][pt[q[good]]]
        store[p, 0, :, 0] = t
        store[p, 0, :, 1] = rng.integers(-1, sizes[jj] + 1, cap)
        d1 = rng.choice([1.0, 2.0, 3.5, 10.0, np.inf, np.nan], cap, p=[0.35, 0.25, 0.2, 0.14, 0.03, 0.03]).astype(np.float32)
        d0 = (d1 * rng.choice([0.25, 0.5, 0.7, 0.75, 1.0], cap, p=[0.5, 0.3, 0.05, 0.1, 0.05])).astype(np.float32)
        store[p, 1] = np.stack([d0, d1], -1).view(np.int32)
    return dict(store=store, nq=nq, pairs=pairs, img_off=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32),
                kp=np.concatenate(kps).astype(np.float32).reshape(-1, 2), K=K, ratio=float(rng.choice([0.7, 0.75, 0.5])))


def staged(case, budget, seed):
    """The restated stages of a scene."""
    return nv.verify_pairs(case["store"], case["nq"], case["pairs"], case["img_off"], case["kp"], case["K"], case["ratio"], budget=budget, seed=seed,
                           stages=True)


def device_inputs(case, st):
    return dict(surv=dev(st["surv"]), m=dev(st["m"]), pairs=dev(case["pairs"]), img_off=dev(case["img_off"]), xn=dev(st["xn"]))


# ---- families -----------------------------------------------------------------------------------------------------------------

def fuzz_survivors(rng):
    import torch
    from sfm_mvs_amd import verify
    store, nq, pair, img_off, ratio, _ = ft.gen_store(rng)
    want_s, want_m = nv.survivors(store, nq, pair, img_off, ratio)
    surv, chk_s = flat_out(want_s.shape, torch.int32)
    m, chk_m = flat_out(want_m.shape, torch.int32)
    verify.survivors(dev(store), dev(nq), dev(pair), dev(img_off), ratio, out=(surv, m))
    return first(same("surv", surv, want_s), same("m", m, want_m), chk_s(), chk_m())


def fuzz_samples(rng):
    import torch
    from sfm_mvs_amd import verify
    n_pairs = log_uniform_from_zero(rng, 12)
    H = max(1, log_uniform_from_zero(rng, 1024)) if rng.integers(4) else int(rng.choice([1, 64, 65, 1024]))
    H = min(H, max(1, 3000 // max(n_pairs, 1)))
    m = rng.choice([0, 4, 5, 6, 7, 255, 256, 257, 10000, INT32_MAX, -1], n_pairs).astype(np.int32)
    rnd = rng.random(n_pairs) < 0.3
    m[rnd] = np.exp(rng.uniform(0, np.log(2.0 ** 31 - 1), int(rnd.sum()))).astype(np.int32)
    seed = int(rng.integers(1 << 32))
    out, chk = flat_out((n_pairs, H, 5), torch.int32)
    verify.samples(dev(m), H, seed, out=out)
    return first(same("samp", out, nv.samples(m, H, seed)), chk())


def gen_models_case(rng):
    deg = int(rng.integers(5)) if rng.integers(4) == 0 else -1
    case = gen_scene(rng, max_pts=120, max_pairs=2)
    H = max(1, log_uniform_from_zero(rng, 96))
    xn = nv.normalise(case["kp"], case["K"])
    if len(xn):
        if deg == 0:
            xn[:] = xn[0]
        if deg == 1:
            xn[:, 1] = 2 * xn[:, 0] + 0.1
        if deg == 2:
            xn[rng.random(len(xn)) < 0.1] = np.nan
        if deg == 3:
            xn[rng.random(len(xn)) < 0.1] = 1e150
        if deg == 4:
            xn[rng.random(len(xn)) < 0.1] = np.inf
    surv, m = nv.survivors(case["store"], case["nq"], case["pairs"], case["img_off"], case["ratio"])
    samp = nv.samples(m, H, int(rng.integers(1 << 32)))
    bad = rng.random(samp.shape) < 0.02
    samp[bad] = rng.choice([-1, surv.shape[1], INT32_MAX], int(bad.sum()))
    if m.size and rng.integers(4) == 0:
        m = m.copy()
        m[rng.integers(len(m))] += rng.choice([-1, 1, 1000])
    return case, xn, surv, m, samp


def fuzz_models(rng):
    import torch
    from sfm_mvs_amd import verify
    case, xn, surv, m, samp = gen_models_case(rng)
    want_n, want_E = nv.models(samp, surv, m, case["pairs"], case["img_off"], xn)
    nm, chk_n = flat_out(want_n.shape, torch.int32)
    E, chk_E = flat_out(want_E.shape, torch.float64)
    verify.models(dev(samp), dev(surv), dev(m), dev(case["pairs"]), dev(case["img_off"]), dev(xn), out=(nm, E))
    return first(same("nmodels", nm, want_n), same("E", E, want_E), chk_n(), chk_E())


def fuzz_score(rng):
    import torch
    from sfm_mvs_amd import verify
    case = gen_scene(rng, max_pts=int(rng.choice([40, 250, 260, 600])), max_pairs=2)
    st = staged(case, max(1, log_uniform_from_zero(rng, 48)), int(rng.integers(1 << 32)))
    nm, E = st["nmodels"].copy(), st["E_all"].copy()
    if nm.size and rng.integers(2):                                  # one model under several slots: the smallest must win
        p = int(rng.integers(len(nm)))
        src = np.argwhere(nm[p] > 0)
        if len(src):
            E[p, :, 0] = E[p, src[0, 0], 0]
            nm[p] = np.maximum(nm[p], 1)
    if nm.size and rng.integers(4) == 0:
        nm[rng.integers(len(nm))] = rng.choice([0, -3, 11], nm.shape[1])
    thr2 = float(st["thr2"]) * float(rng.choice([1.0, 1.0, 100.0, 0.0, np.inf]))
    want_c, want_b = nv.score(E, nm, st["surv"], st["m"], case["pairs"], case["img_off"], st["xn"], thr2)
    d = device_inputs(case, st)
    counts, chk_c = flat_out(want_c.shape, torch.int32)
    got_c, got_b = verify.score(dev(E), dev(nm), d["surv"], d["m"], d["pairs"], d["img_off"], d["xn"], thr2, out=(counts, torch.empty(len(nm), dtype=torch.int64, device="cuda")))
    return first(same("counts", got_c, want_c), same("best", got_b.cpu().numpy().view(np.uint64), want_b), chk_c())


def fuzz_select(rng):
    import torch
    from sfm_mvs_amd import verify
    case = gen_scene(rng, max_pts=int(rng.choice([40, 250, 600])), max_pairs=2)
    st = staged(case, max(1, log_uniform_from_zero(rng, 32)), int(rng.integers(1 << 32)))
    best = st["best"].copy()
    if best.size and rng.integers(4) == 0:
        best[rng.integers(len(best))] = rng.choice(np.array([0, 1, (5 << 32) | 0xFFFFFFFF, (3 << 32) | 5], np.uint64))
    thr2 = float(st["thr2"]) * float(rng.choice([1.0, 1.0, 100.0, 1e6]))
    args = (st["E_all"], st["nmodels"], best, st["surv"], st["m"], case["pairs"], case["img_off"], st["xn"], thr2)
    want = nv.select(*args)
    d = device_inputs(case, st)
    n_pairs, cap = st["surv"].shape[:2]
    outs = [flat_out(s, t) for s, t in (((n_pairs, cap), torch.uint8), ((n_pairs, 9), torch.float64), ((n_pairs, 12), torch.float64), ((n_pairs, 8), torch.int32))]
    got = verify.select(dev(st["E_all"]), dev(st["nmodels"]), dev(best.view(np.int64)), d["surv"], d["m"], d["pairs"], d["img_off"], d["xn"], thr2,
                        out=tuple(o for o, _ in outs))
    return first(*[same(n, g, w) for n, g, w in zip(("keep", "E", "Rt", "info"), got, want)], *[c() for _, c in outs])


def fuzz_composed(rng):
    import torch
    from sfm_mvs_amd import verify
    case = gen_scene(rng, max_pts=300, max_pairs=3)
    H, seed = max(1, log_uniform_from_zero(rng, 64)), int(rng.integers(1 << 32))
    want = staged(case, H, seed)
    torch.cuda.synchronize()
    got = verify.verify_pairs(dev(case["store"]), dev(case["nq"]), dev(case["pairs"]), dev(case["img_off"]), dev(case["kp"]), case["K"], case["ratio"],
                              budget=H, seed=seed)
    return first(*[same(n, got[n], want[n]) for n in ("keep", "E", "Rt", "info")])


FAMILIES = [("survivors", fuzz_survivors, 3), ("samples", fuzz_samples, 2), ("models", fuzz_models, 2), ("score", fuzz_score, 2),
            ("select", fuzz_select, 2), ("composed", fuzz_composed, 2)]


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
            log(f"MISMATCH {name} (seed {seed}, case seed {case_seed}; replay: fuzz_verify.py 0 0 {name}:{case_seed}) {msg}")
    return counts, bad, time.time() - t0


def main():
    import sfm_mvs_amd
    from sfm_mvs_amd import _lib
    budget = float(sys.argv[1]) if len(sys.argv) > 1 else 90.0
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    sfm_mvs_amd.lib()
    if len(sys.argv) > 3:                               # replay one case
        name, case_seed = sys.argv[3].split(":")
        msg = {n: fn for n, fn, _ in FAMILIES}[name](np.random.default_rng(int(case_seed)))
        print(f"fuzz_verify replay {name}:{case_seed}: {msg or 'no mismatch'}")
        return 1 if msg else 0
    counts, bad, dt = run(budget, seed, log=lambda s: print(s, flush=True))
    print(f"fuzz_verify: seed {seed}, {sum(counts.values())} cases {counts}, {bad} mismatches, {dt:.0f} s")
    print(f"sfm_build_id {_lib.build_id()}")
    print(json.dumps(dict(tool="fuzz_verify", seed=seed, cases=sum(counts.values()), families=counts, mismatches=bad, seconds=round(dt, 1))))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
