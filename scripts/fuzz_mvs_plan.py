"""Randomised parity sweep of the MVS-PLAN family on the GPU box: sfm_view_pair_counts / sfm_view_depth_ranges / sfm_view_select and
mvs_plan.plan_views + host_plan (through sfm_mvs_amd.mvs_plan, into sentinel-padded buffers) vs the restatement tests/np_mvs_plan.py.
Every word is compared exactly (float outputs as integer views), every call is made twice and must repeat its bits, and nothing past a
stated size may be written.

  python scripts/fuzz_mvs_plan.py [seconds] [seed] [family:case_seed]

Families (one case = one random draw; sizes log-uniform from 0 up to a cap that keeps the NumPy side well under a second):
  pairs     cameras around the origin, points near it, tracks of random lengths over random cameras; a random cosine window; ncam on
            both sides of SFM_PLAN_LDS_CAMS
  ranges    the same problems through the camera-side CSR at random permille bounds
  select    random small-integer matrices (many exact ties), nsrc 1..8, a random min_good
  composed  plan_views + host_plan against the restatement's chain: neighbours and ranges
One case in four carries a degeneracy: no observation, NaN / infinite points, indices from {-1, ncam, INT32_MAX} in cam_idx, CSR offsets
outside 0..nobs, identical camera centres, cam_obs entries out of range or naming another camera, duplicated points (runs of equal
depths), a track naming one camera twice, a third row of P that makes the depths denormal, infinite, zero or negative.  The script
stops at the first mismatch, prints the family and the case seed that rebuilds the inputs without a GPU, and exits non-zero.
"""
import os
import sys
import time

os.environ.setdefault("OMP_WAIT_POLICY", "passive")

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "scripts"))
import np_mvs_plan as npl
from fuzz_tracks import SENTINEL, dev, log_uniform_from_zero

K = np.array([[900.0, 0, 480.0], [0, 900.0, 320.0], [0, 0, 1.0]])
INT32_MAX = 2 ** 31 - 1
LDS_CAMS = 96
MAX_OBS = 1 << 13
N_DEG = 9
PAD = 64                        # sentinel words behind every output


def random_P(rng, ncam):
    """[ncam, 3, 4] = K [R | t]: cameras at a distance of about 8 that look at the origin."""
    from mvs_scenes import look_at
    P = np.empty((ncam, 3, 4))
    for k in range(ncam):
        a = rng.uniform(0, 2 * np.pi)
        C = np.array([8 * np.cos(a), rng.uniform(-1, 1), 8 * np.sin(a)]) * rng.uniform(0.8, 1.3)
        R, t = look_at(C, np.zeros(3))
        P[k] = K @ np.c_[R, t]
    return P


def make_problem(rng, ncam, npt, lengths, deg=-1):
    """Point-major observations: track t is seen by lengths[t] distinct cameras (ascending) -> dict of the inputs and both CSRs."""
    P = random_P(rng, ncam)
    X = rng.normal(0, 0.6, (npt, 3))
    lengths = np.minimum(np.asarray(lengths, np.int64), ncam)
    if deg == 0:
        lengths = np.zeros(npt, np.int64)
    pt_idx = np.repeat(np.arange(npt), lengths).astype(np.int32)
    cam_idx = (np.concatenate([np.sort(rng.permutation(ncam)[:n]) for n in lengths]) if len(pt_idx) else np.zeros(0)).astype(np.int32)
    nobs = len(pt_idx)
    if deg == 1 and npt:
        hit = rng.random(npt) < 0.2
        X[hit, rng.integers(3, size=int(hit.sum()))] = rng.choice([np.nan, np.inf, -np.inf], int(hit.sum()))
    if deg == 2 and nobs:
        hit = rng.random(nobs) < 0.15
        cam_idx[hit] = rng.choice([-1, ncam, INT32_MAX], int(hit.sum()))
    if deg == 4 and ncam > 1:
        P[rng.random(ncam) < 0.5] = P[0]
    if deg == 6 and npt:
        X = X[rng.integers(max(1, npt // 8), size=npt)]                                             # runs of equal depths
    if deg == 7 and nobs > 1:
        hit = np.flatnonzero((rng.random(nobs) < 0.2) & (np.arange(nobs) > 0))
        same = pt_idx[hit] == pt_idx[hit - 1]
        cam_idx[hit[same]] = cam_idx[hit[same] - 1]
    if deg == 8:
        for k in np.flatnonzero(rng.random(ncam) < 0.6):
            P[k, 2] *= rng.choice([1e-42, 1e-39, 1e37, 1e39, -1.0, 0.0])
    track_off, _ = npl.csr(pt_idx, npt)
    cam_off, cam_obs = npl.csr(cam_idx, ncam)
    if deg == 3:
        for off in (track_off, cam_off):
            hit = rng.random(len(off)) < 0.2
            off[hit] = rng.choice([-5, nobs + 3, INT32_MAX, 0, nobs // 2], int(hit.sum()))
    if deg == 5 and nobs:
        hit = rng.random(nobs) < 0.2
        cam_obs[hit] = rng.choice([-1, nobs, INT32_MAX, int(rng.integers(nobs))], int(hit.sum()))
    return dict(ncam=ncam, npt=npt, P=P, X=np.ascontiguousarray(X), cam_idx=cam_idx, pt_idx=pt_idx, track_off=track_off, cam_off=cam_off,
                cam_obs=cam_obs, deg=deg)


def gen_problem(rng, max_obs=MAX_OBS, deg=None):
    if deg is None:
        deg = int(rng.integers(N_DEG)) if rng.integers(4) == 0 else -1
    ncam = int(rng.choice([1, 2, 3, int(rng.integers(4, 33)), int(rng.integers(33, LDS_CAMS + 1)), int(rng.integers(LDS_CAMS + 1, 160))],
                          p=[0.05, 0.1, 0.1, 0.4, 0.2, 0.15]))
    npt = log_uniform_from_zero(rng, 1 << 10)
    top = max(2, min(ncam, int(rng.choice([3, 8, 17, 64, 160]))))
    lengths = rng.integers(0 if rng.integers(4) == 0 else 2, top + 1, npt)
    while lengths.sum() > max_obs:
        lengths = lengths // 2
    return make_problem(rng, ncam, npt, lengths, deg)


def padded(n, dtype):
    """(flat int32 buffer of sentinels, the first n elements viewed as `dtype`)."""
    import torch
    k = torch.empty(0, dtype=dtype).element_size() // 4
    flat = torch.full((n * k + PAD,), SENTINEL, dtype=torch.int32, device="cuda")
    return flat, flat[:n * k].view(dtype)


def pad_clean(*flats):
    return all(bool((f[-PAD:] == SENTINEL).all()) for f in flats)


def device_plan(p):
    from sfm_mvs_amd import track_ba
    return track_ba.Plan(p["ncam"], p["npt"], dev(p["track_off"]), dev(p["cam_idx"]), dev(p["pt_idx"]), dev(p["cam_off"]), dev(p["cam_obs"]))


def same_words(got, want):
    got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    want = np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype.kind == "f":
        view = np.int32 if got.dtype == np.float32 else np.int64
        return bool(np.array_equal(got.view(view), want.view(view)) or np.array_equal(got, want, equal_nan=True))
    return bool(np.array_equal(got, want))


def check_pairs(p, cos_lo, cos_hi):
    """-> (message or '', device (shared, good), restated (shared, good))."""
    import torch
    from sfm_mvs_amd import mvs_plan
    pl, n = device_plan(p), p["ncam"]
    X, P = dev(p["X"]), dev(p["P"].reshape(n, 12))
    runs = []
    for _ in range(2):
        fs, s = padded(n * n, torch.int32)
        fg, g = padded(n * n, torch.int32)
        fc, c = padded(n * 3, torch.float64)
        mvs_plan.pair_counts(pl, X, P, cos_lo, cos_hi, out=(s.view(n, n), g.view(n, n), c.view(n, 3)))
        if not pad_clean(fs, fg, fc):
            return "pairs: wrote past a stated size", None, None
        runs.append((s.view(n, n).cpu().numpy(), g.view(n, n).cpu().numpy(), c.view(n, 3).cpu().numpy()))
    if not all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(*runs)):
        return "pairs: a second run gave other bits", None, None
    shared, good, C = runs[0]
    wC = npl.centres(p["P"])
    if not same_words(C, wC):
        return f"pairs: centres differ by {np.nanmax(np.abs(C - wC))}", None, None
    ws, wg = npl.pair_counts(p["track_off"], p["cam_idx"], p["X"], wC, n, cos_lo, cos_hi)
    if not np.array_equal(shared, ws):
        return f"pairs: shared differs in {int((shared != ws).sum())} cells (deg {p['deg']}, ncam {n})", None, None
    if not np.array_equal(good, wg):
        return f"pairs: good differs in {int((good != wg).sum())} cells (deg {p['deg']}, ncam {n})", None, None
    if not (np.array_equal(shared, shared.T) and np.array_equal(good, good.T) and not np.diag(shared).any() and not np.diag(good).any()):
        return "pairs: not symmetric with a zero diagonal", None, None
    return "", (shared, good), (ws, wg)


def check_ranges(p, lo_pm, hi_pm):
    import torch
    from sfm_mvs_amd import mvs_plan
    pl, n = device_plan(p), p["ncam"]
    X, P = dev(p["X"]), dev(p["P"].reshape(n, 12))
    runs = []
    for _ in range(2):
        fm, m = padded(n, torch.int32)
        fa, a = padded(n, torch.float32)
        fb, b = padded(n, torch.float32)
        mvs_plan.depth_ranges(pl, X, P, lo_pm, hi_pm, out=(m, a, b))
        if not pad_clean(fm, fa, fb):
            return "ranges: wrote past a stated size", None, None
        runs.append((m.cpu().numpy(), a.cpu().numpy().view(np.int32), b.cpu().numpy().view(np.int32)))
    if not all(np.array_equal(x, y) for x, y in zip(*runs)):
        return "ranges: a second run gave other bits", None, None
    want = npl.depth_ranges(p["cam_off"], p["cam_obs"], p["cam_idx"], p["pt_idx"], p["X"], p["P"], lo_pm, hi_pm)
    got = runs[0]
    for name, g, w in zip(("m", "z_lo", "z_hi"), got, (want[0], want[1].view(np.int32), want[2].view(np.int32))):
        if not np.array_equal(g, w):
            bad = np.flatnonzero(g != w)
            return f"ranges: {name} differs at cameras {bad[:5].tolist()} (got {g[bad[:5]].tolist()}, want {w[bad[:5]].tolist()}; deg {p['deg']})", None, None
    return "", got, want


def check_select(shared, good, nsrc, min_good):
    import torch
    from sfm_mvs_amd import mvs_plan
    n = len(good)
    s, g = dev(np.ascontiguousarray(shared, np.int32)), dev(np.ascontiguousarray(good, np.int32))
    fn, nbr = padded(n * nsrc, torch.int32)
    fk, cnt = padded(n, torch.int32)
    mvs_plan.select(s, g, nsrc, min_good, out=(nbr.view(n, nsrc), cnt))
    if not pad_clean(fn, fk):
        return "select: wrote past a stated size"
    wn, wk = npl.select(shared, good, nsrc, min_good)
    if not (np.array_equal(nbr.view(n, nsrc).cpu().numpy(), wn) and np.array_equal(cnt.cpu().numpy(), wk)):
        return f"select: differs (ncam {n}, nsrc {nsrc}, min_good {min_good})"
    return ""


def check_composed(p, nsrc, window, min_good, lo, hi):
    from sfm_mvs_amd import mvs_plan
    from sfm_mvs_amd._lib import SfmHipError
    pl, n = device_plan(p), p["ncam"]
    planned = mvs_plan.plan_views(pl, dev(p["X"]), dev(p["P"].reshape(n, 12)), nsrc, window[0], window[1], min_good, lo, hi)
    cos_lo, cos_hi = mvs_plan.cos_window(*window)
    ws, wg = npl.pair_counts(p["track_off"], p["cam_idx"], p["X"], npl.centres(p["P"]), n, cos_lo, cos_hi)
    wn, wk = npl.select(ws, wg, nsrc, min_good)
    wm, wa, wb = npl.depth_ranges(p["cam_off"], p["cam_obs"], p["cam_idx"], p["pt_idx"], p["X"], p["P"], int(round(10 * lo)), int(round(10 * hi)))
    want = npl.pooled_ranges(wm, wa, wb)
    try:
        hp = mvs_plan.host_plan(planned)
    except SfmHipError:
        return "" if want is None else "composed: host_plan raised although a view has 8 depths"
    if want is None:
        return "composed: host_plan did not raise although no view has 8 depths"
    if hp["neighbours"] != [[int(v) for v in wn[i, :wk[i]]] for i in range(n)]:
        return "composed: neighbours differ"
    if not np.array_equal(hp["ranges"].view(np.int64), want.view(np.int64)):
        return "composed: ranges differ"
    return "" if np.array_equal(hp["shared"], ws) and np.array_equal(hp["good"], wg) and np.array_equal(hp["m"], wm) else "composed: matrices differ"


def random_window(rng):
    lo = float(rng.choice([0.0, 1.0, 5.0, 20.0]))
    hi = float(rng.choice([30.0, 60.0, 120.0, 180.0]))
    return lo, hi


def fuzz_pairs(rng):
    from sfm_mvs_amd import mvs_plan
    p = gen_problem(rng)
    if rng.integers(8) == 0:
        return check_pairs(p, -1.0, 1.0)[0]
    return check_pairs(p, *mvs_plan.cos_window(*random_window(rng)))[0]


def fuzz_ranges(rng):
    p = gen_problem(rng)
    lo = int(rng.choice([0, 20, 500, 1000, int(rng.integers(1001))]))
    hi = int(rng.choice([lo, 980, 1000, int(rng.integers(lo, 1001))]))
    return check_ranges(p, lo, max(lo, hi))[0]


def fuzz_select(rng):
    n = max(1, log_uniform_from_zero(rng, 300))
    top = int(rng.choice([1, 3, 50, 100000]))
    shared = rng.integers(0, top + 1, (n, n)).astype(np.int32)
    good = np.minimum(shared, rng.integers(0, top + 1, (n, n))).astype(np.int32)
    if rng.integers(4) == 0:
        good[rng.random(n) < 0.5] = 0
    return check_select(shared, good, int(rng.integers(1, 9)), int(rng.choice([0, 1, 2, top, top + 1])))


def fuzz_composed(rng):
    p = gen_problem(rng, 1 << 11)
    return check_composed(p, int(rng.integers(1, 9)), random_window(rng), int(rng.choice([1, 2, 8])), float(rng.choice([0, 2, 10])),
                          float(rng.choice([90, 98, 100])))


FAMILIES = [("pairs", fuzz_pairs, 3), ("ranges", fuzz_ranges, 3), ("select", fuzz_select, 2), ("composed", fuzz_composed, 1)]


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
            log(f"MISMATCH {name} (seed {seed}, case seed {case_seed}; replay: fuzz_mvs_plan.py 0 0 {name}:{case_seed}) {msg}")
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
        print(f"fuzz_mvs_plan replay {name}:{case_seed}: {msg or 'no mismatch'}")
        return 1 if msg else 0
    counts, bad, dt = run(budget, seed, log=lambda s: print(s, flush=True))
    print(f"fuzz_mvs_plan: seed {seed}, {sum(counts.values())} cases {counts}, {bad} mismatches, {dt:.0f} s")
    print(f"sfm_build_id {_lib.build_id()}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
