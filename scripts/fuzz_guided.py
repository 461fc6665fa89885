"""Randomised parity sweep of the GUIDED family on the GPU box: sfm_guided_match / sfm_guided_mutual, guided.guided_pairs and
tracks.guided_keep (through sfm_mvs_amd.guided, into sentinel-filled buffers) vs the restatement tests/np_guided.py; every output word
compared exactly (floats as integer views).

  python scripts/fuzz_guided.py [seconds] [seed] [family:case_seed]

Families (one case = one random draw; sizes log-uniform from 0):
  match       two to four images of 0..600 keypoints with duplicate descriptor rows, one to four pairs, an essential matrix per pair; cap
              and the rev stride around the image sizes; thr2g = one pair's own float32 quotient (a quantile of its band values), the float
              below it, 0, -1 and +inf
  mutual      the restatement's store and rev with words replaced (neighbours of -1, past the stride, rev rows that name other queries)
  composed    guided.guided_pairs whole and in chunks of one and of three pairs against the restated composition, and tracks.guided_keep
              on a small scene with twins against the restated `guided_keep`
One case in four carries a degeneracy: NaN, inf and 1e30 descriptor values; E zero, NaN, 1e150; NaN keypoints; pairs (i, i) and out of
range; inactive pairs; no pairs; cap = 0.
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
import np_guided as ng
import np_verify as nv
from datagen import sift_like
from fuzz_tracks import dev, log_uniform_from_zero
from fuzz_verify import INT32_MAX, first, flat_out, same


def as_i64(keys):
    return np.ascontiguousarray(keys, np.uint64).view(np.int64)


def random_E(rng):
    from scipy.spatial.transform import Rotation
    t = rng.normal(size=3)
    t /= np.linalg.norm(t)
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    E = tx @ Rotation.from_rotvec(rng.normal(0, 0.3, 3)).as_matrix()
    return (E / np.linalg.norm(E)).reshape(9)


def gen_case(rng, max_pts=600, max_pairs=4):
    """-> dict(desc, xn, E, active, nq, pairs, img_off, cap, stride, thr2g)."""
    deg = int(rng.integers(9)) if rng.integers(4) == 0 else -1
    n_img = int(rng.integers(2, 5))
    sizes = np.array([log_uniform_from_zero(rng, max_pts) for _ in range(n_img)])
    if rng.integers(3) == 0:                                         # around the tile of 256 and the wave of 64
        sizes[:2] = rng.choice([63, 64, 65, 255, 256, 257], 2)
    n = int(sizes.sum())
    img_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    desc = sift_like(rng, n) if n else np.zeros((0, 128), np.float32)
    if n > 1:                                                        # duplicate rows inside and across images: ties of the keys
        k = int(rng.integers(0, n // 2 + 1))
        desc[rng.integers(n, size=k)] = desc[rng.integers(n, size=k)]
    xn = rng.uniform(-0.6, 0.6, (n, 2))
    n_pairs = 0 if deg == 0 else int(rng.integers(1, max_pairs + 1))
    pairs = np.array([rng.choice(n_img, 2, replace=False) for _ in range(n_pairs)], np.int32).reshape(-1, 2)
    E = np.array([random_E(rng) for _ in range(n_pairs)]).reshape(n_pairs, 9)
    active = (rng.random(n_pairs) < 0.9).astype(np.uint8)
    if n_pairs:
        p = int(rng.integers(n_pairs))
        if deg == 1:
            pairs[p] = rng.choice([[0, 0], [-1, 1], [1, n_img], [INT32_MAX, 0]])
        if deg == 2:
            E[p] = rng.choice([0.0, np.nan, 1e150, np.inf])
        if deg == 3:
            E[p, rng.integers(9)] = rng.choice([np.nan, 1e150, -1e150])
        if deg == 4:
            active[:] = 0
    if n:
        if deg == 5:
            desc[rng.random(n) < 0.2, rng.integers(128)] = rng.choice([np.nan, np.inf, 1e30, -1e30, 3e38])
        if deg == 6:
            xn[rng.random(n) < 0.1] = rng.choice([np.nan, np.inf, 1e150])
        if deg == 7:
            xn[:] = xn[0]
    big = int(sizes.max())
    cap = 0 if deg == 8 else max(0, big + int(rng.integers(-3, 4))) if rng.integers(3) else log_uniform_from_zero(rng, big + 5)
    stride = big if rng.integers(4) else max(0, big + int(rng.integers(-3, 4)))
    nq = np.array([min(sizes[int(np.clip(i, 0, n_img - 1))], cap) if rng.integers(4) else rng.integers(-1, cap + 3) for i, _ in pairs], np.int32).reshape(-1)
    thr2g = float(rng.choice([0.0, -1.0, np.inf, 1e-4]))
    if n_pairs and rng.integers(4):                                  # one pair's own value: a quantile of its band values, or the float below
        p = int(rng.integers(n_pairs))
        qb, nt, oa, ob = ng.extent(p, nq, pairs, img_off.astype(np.int64), n_img, cap, stride)
        if qb and nt:
            v = ng.quotient(E[p], xn[oa:oa + qb], xn[ob:ob + nt]).ravel()
            v = np.sort(v[~np.isnan(v)])
            if len(v):
                thr2g = float(v[int(rng.choice([0.0, 0.002, 0.01, 0.05, 0.5, 0.999]) * (len(v) - 1))])
                if rng.integers(3) == 0:
                    thr2g = float(np.nextafter(np.float32(thr2g), np.float32(-1)))
    return dict(desc=desc, xn=xn, E=E, active=active, nq=nq, pairs=pairs, img_off=img_off, cap=int(cap), stride=int(stride), thr2g=thr2g)


def match_both(c):
    """The device's store and rev beside the restatement's -> (mismatch message, store, rev)."""
    import torch
    from sfm_mvs_amd import guided
    want_s, want_r = ng.guided_match(c["desc"], c["xn"], c["E"], c["active"], c["nq"], c["pairs"], c["img_off"], c["cap"], c["thr2g"], c["stride"])
    store, chk_s = flat_out(want_s.shape, torch.int32)
    rev, chk_r = flat_out(want_r.shape, torch.int64)
    guided.guided_match(dev(c["desc"]), dev(c["xn"]), dev(c["E"]), dev(c["active"]), dev(c["nq"]), dev(c["pairs"]), dev(c["img_off"]), c["cap"],
                        c["thr2g"], out=store, rev=rev)
    return first(same("store_g", store, want_s), same("rev", rev.cpu().numpy().view(np.uint64), want_r), chk_s(), chk_r()), want_s, want_r


def mutual_both(store, rev, c):
    import torch
    from sfm_mvs_amd import guided
    want_k, want_i = ng.guided_mutual(store, rev, c["nq"], c["pairs"], c["img_off"])
    keep, chk_k = flat_out(want_k.shape, torch.uint8)
    info, chk_i = flat_out(want_i.shape, torch.int32)
    guided.guided_mutual(dev(store), dev(as_i64(rev)), dev(c["nq"]), dev(c["pairs"]), dev(c["img_off"]), out=(keep, info))
    return first(same("keep_g", keep, want_k), same("info_g", info, want_i), chk_k(), chk_i())


def fuzz_match(rng):
    c = gen_case(rng)
    msg, store, rev = match_both(c)
    return msg or mutual_both(store, rev, c)


def fuzz_mutual(rng):
    c = gen_case(rng, max_pts=300)
    store, rev = ng.guided_match(c["desc"], c["xn"], c["E"], c["active"], c["nq"], c["pairs"], c["img_off"], c["cap"], c["thr2g"], c["stride"])
    if store.size:
        bad = rng.random(store[:, 0].shape) < 0.1
        store[:, 0][bad] = rng.choice([-1, 0, c["stride"] - 1, c["stride"], c["stride"] + 7, INT32_MAX, -5], int(bad.sum()))
    if rev.size:
        bad = rng.random(rev.shape) < 0.2
        rev[bad] = (rng.integers(0, 1 << 31, int(bad.sum())).astype(np.uint64) << np.uint64(32)) | rng.integers(0, c["cap"] + 2, int(bad.sum())).astype(np.uint64)
    return mutual_both(store, rev, c)


def fuzz_composed(rng):
    import torch
    from sfm_mvs_amd import guided, tracks
    if rng.integers(3) == 0:                                         # guided_keep on a small scene with twins
        import guided_cases as gc
        sc = gc.twin_scene(int(rng.integers(2, 4)), int(rng.choice([40, 70, 130])), float(rng.choice([0.0, 0.5])), int(rng.integers(1 << 20)))
        store = gc.global_store(sc)
        kw = dict(budget=int(rng.choice([8, 32])), seed=int(rng.integers(1 << 32)))
        mult, mutual = float(rng.choice([1, 4, 30])), bool(rng.integers(2))
        want_s, want_k = ng.guided_keep(sc["desc"], store, sc["nq"], sc["pairs"], sc["img_off"], sc["kp"], sc["K"], guided_threshold=mult * 0.4,
                                        mutual=mutual, **kw)
        got_s, got_k = tracks.guided_keep([dev(d) for d in sc["descs"]], dev(store), sc["nq"], sc["pairs"], [dev(k) for k in sc["kps"]], sc["K"],
                                          guided_threshold=mult * 0.4, mutual=mutual, **kw)
        return first(same("store_g", got_s, want_s), same("keep", got_k, want_k))
    c = gen_case(rng, max_pts=300, max_pairs=5)
    n_pairs = len(c["pairs"])
    K = np.array([[800.0, 0, 480], [0, 810.0, 320], [0, 0, 1]])
    with np.errstate(all="ignore"):                                  # keypoints of 1e150 become inf in float32
        kp = (c["xn"] * [800.0, 810.0] + [480.0, 320.0]).astype(np.float32)
    info = np.zeros((n_pairs, 8), np.int32)
    info[:, 2] = rng.integers(0, 17, n_pairs)
    thr, mi, mutual = float(rng.choice([0.4, 1.6, 40.0])), int(rng.choice([0, 8, 12])), bool(rng.integers(2))
    big = int(np.diff(c["img_off"]).max())
    want = ng.guided_pairs(c["desc"], c["nq"], c["pairs"], c["img_off"], kp, K, c["E"], info, thr, mi, mutual, cap=c["cap"], max_size=big)
    chunk = {} if rng.integers(3) == 0 else dict(max_rev_bytes=int(rng.choice([1, 3 * 8 * max(big, 1)])))
    got = guided.guided_pairs(dev(c["desc"]), dev(c["nq"]), dev(c["pairs"]), dev(c["img_off"]), dev(kp), K, dev(c["E"]), dev(info), thr, mi, mutual,
                              cap=c["cap"], max_size=big, **chunk)
    if not mutual:
        return first(same("store", got["store"], want["store"]), "" if got["keep"] is None and got["info"] is None else "keep without mutual")
    return first(*[same(n, got[n], want[n]) for n in ("store", "keep", "info")])


FAMILIES = [("match", fuzz_match, 4), ("mutual", fuzz_mutual, 2), ("composed", fuzz_composed, 2)]


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
            log(f"MISMATCH {name} (seed {seed}, case seed {case_seed}; replay: fuzz_guided.py 0 0 {name}:{case_seed}) {msg}")
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
        print(f"fuzz_guided replay {name}:{case_seed}: {msg or 'no mismatch'}")
        return 1 if msg else 0
    counts, bad, dt = run(budget, seed, log=lambda s: print(s, flush=True))
    print(f"fuzz_guided: seed {seed}, {sum(counts.values())} cases {counts}, {bad} mismatches, {dt:.0f} s")
    print(f"sfm_build_id {_lib.build_id()}")
    print(json.dumps(dict(tool="fuzz_guided", seed=seed, cases=sum(counts.values()), families=counts, mismatches=bad, seconds=round(dt, 1))))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
