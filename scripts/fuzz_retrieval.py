"""Randomised parity sweep of the RETRIEVAL family on the GPU box: sfm_vlad_accumulate / _centres / _signature / _shortlist / _pairs and
retrieval.select_pairs (through sfm_mvs_amd.retrieval, into sentinel-filled buffers) vs the restatement tests/np_retrieval.py; every
output word compared exactly (floats as integer views).

  python scripts/fuzz_retrieval.py [seconds] [seed] [family:case_seed]

Families (one case = one random draw; sizes log-uniform from 0):
  accumulate  one to nine images of 0..700 keypoints (sizes around the wave, the block and the chunk of 1 024 mixed in), 1..256 centres
              some of which are descriptor rows and some equal, duplicate descriptor rows, scale 2^-3 .. 2^12 or one that makes the
              clamp bite
  centres     the restatement's sums of a single image with counts of 0 and 1 forced, then the update
  signature   random sums of every magnitude up to 2^62, ssr 0 and 1, qs of 1, 127, 254, 1000
  shortlist   random signatures with equal, opposite and all-zero rows, k of 1..64, min_sim of -inf, -1, 0, 1, +inf, a row's own k-th
              value and the float above it
  pairs       random neighbour lists with -1, out-of-range, self and repeated entries, union and mutual, cap_pairs of 0, count - 1, count
  composed    retrieval.select_pairs on a small corridor against the restated composition
One case in four carries a degeneracy: NaN, +-inf, 1e30 and denormal descriptor values, an all-zero descriptor set, one image that holds
every node, all centres equal, no keypoint at all.
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
import np_retrieval as nr
from datagen import sift_like
from fuzz_tracks import dev, gen_offsets, log_uniform_from_zero
from fuzz_verify import first, flat_out, same

EDGE_SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)
MAX_NORM2 = 256 * 128 * 127 * 127


def sig_out(shape):
    """An int8 tensor carved from sentinel bytes -> (tensor, check())."""
    import torch
    buf, chk = flat_out(shape, torch.uint8)
    return buf.view(torch.int8), chk


# ---- one entry point against the restatement: '' or the first mismatch ----------------------------------------------------------------

def accumulate_both(desc, centres, img_off, scale):
    import torch
    from sfm_mvs_amd import retrieval
    want = nr.accumulate(desc, centres, img_off, scale)
    outs = [flat_out(w.shape, t) for w, t in zip(want, (torch.int32, torch.int64, torch.int32))]
    retrieval.assign_accumulate(dev(desc), dev(centres), dev(np.asarray(img_off, np.int32)), scale, out=tuple(o for o, _ in outs))
    return first(*[same(n, o, w) for n, (o, _), w in zip(("assign", "acc", "count"), outs, want)], *[chk() for _, chk in outs]), want


def centres_both(centres, acc, count, scale):
    import torch
    from sfm_mvs_amd import retrieval
    want = nr.update_centres(centres, acc, count, scale)
    out, chk = flat_out(want.shape, torch.float32)
    retrieval.update_centres(dev(centres), dev(acc), dev(count), scale, out=out)
    return first(same("centres", out, want), chk()), want


def signature_both(acc, ssr, qs):
    import torch
    from sfm_mvs_amd import retrieval
    want = nr.signatures(acc, ssr, qs)
    sig, chk_s = sig_out(want[0].shape)
    norm2, chk_n = flat_out(want[1].shape, torch.int32)
    retrieval.signatures(dev(acc), ssr, qs, out=(sig, norm2))
    return first(same("sig", sig, want[0]), same("norm2", norm2, want[1]), chk_s(), chk_n()), want


def shortlist_both(sig, norm2, k, min_sim):
    import torch
    from sfm_mvs_amd import retrieval
    want = nr.shortlist(sig, norm2, k, -np.inf if min_sim is None else min_sim)
    nbr, chk_n = flat_out(want[0].shape, torch.int32)
    nbr_sim, chk_s = flat_out(want[1].shape, torch.float32)
    retrieval.shortlist(dev(sig), dev(norm2), k, min_sim, out=(nbr, nbr_sim))
    return first(same("nbr", nbr, want[0]), same("nbr_sim", nbr_sim, want[1]), chk_n(), chk_s()), want


def pairs_both(nbr, mutual, cap):
    """cap None: n_img * k."""
    import torch
    from sfm_mvs_amd import retrieval
    n_img, k = nbr.shape
    cap = n_img * k if cap is None else cap
    want, want_count = nr.pair_list(nbr, mutual, cap)
    buf = torch.full((cap, 2), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    count, chk = flat_out((2,), torch.int32)
    retrieval.pair_list(dev(nbr), mutual, cap, out=(buf, count))
    w = int(want_count[1])
    got = buf.cpu().numpy()
    return first(same("count", count, want_count), same("pairs", got[:w], want[:w]),
                 "" if (got[w:] == 0x5A5A5A5A).all() else "pairs: written at or past the counted rows", chk()), (want, want_count)


# ---- generators -----------------------------------------------------------------------------------------------------------------------

def gen_accumulate(rng, max_pts=700):
    deg = int(rng.integers(7)) if rng.integers(4) == 0 else -1
    n_img = int(rng.choice([1, 2, 3, 5, 9]))
    if rng.integers(3) == 0:
        sizes = rng.choice(EDGE_SIZES, n_img)
    else:
        sizes = np.array([log_uniform_from_zero(rng, max_pts) for _ in range(n_img)])
    if deg == 0:
        sizes[:] = 0
    n = int(sizes.sum())
    img_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    if deg == 1 and n_img > 1:                                       # one image holds every node
        img_off[1:-1] = rng.choice([0, n])
        img_off = np.sort(img_off)
    C = int(rng.choice([1, 2, 3, 16, 63, 64, 65, 255, 256])) if rng.integers(2) else int(rng.integers(1, 257))
    desc = sift_like(rng, n) if n else np.zeros((0, 128), np.float32)
    if n > 1:
        m = int(rng.integers(0, n // 2 + 1))
        desc[rng.integers(n, size=m)] = desc[rng.integers(n, size=m)]
    centres = sift_like(rng, C)
    if n:
        own = rng.random(C) < 0.5                                    # centres that ARE descriptor rows: distances of zero
        centres[own] = desc[rng.integers(n, size=int(own.sum()))]
    if C > 1:
        m = int(rng.integers(0, C // 2 + 1))
        centres[rng.integers(C, size=m)] = centres[rng.integers(C, size=m)]
    if rng.integers(4) == 0:
        centres += rng.normal(0, 0.37, centres.shape).astype(np.float32)          # terms off the integers
    if deg == 2:
        centres[:] = centres[0]
    if n:
        if deg == 3:
            desc[rng.random(n) < 0.2, rng.integers(128)] = rng.choice([np.nan, np.inf, -np.inf, 1e30, -1e30, 3e38])
        if deg == 4:
            desc[rng.random(n) < 0.3, rng.integers(128)] = rng.choice([1e-45, -1e-40, 1e-38])
        if deg == 5:
            desc[:] = 0
    if deg == 6:
        centres[rng.integers(C), rng.integers(128)] = rng.choice([np.nan, np.inf, 1e30])
    scale = float(rng.choice([2.0 ** -3, 1.0, 0.5, 4096.0, 3.7, 2.0 ** 24, 1e30]))
    if rng.integers(5) == 0:                                         # terms exactly at .5: half-even
        scale = 0.5
    return dict(desc=desc, centres=centres, img_off=img_off, scale=scale)


def fuzz_accumulate(rng):
    c = gen_accumulate(rng)
    return accumulate_both(c["desc"], c["centres"], c["img_off"], c["scale"])[0]


def fuzz_centres(rng):
    c = gen_accumulate(rng, max_pts=400)
    n = len(c["desc"])
    _, acc, count = nr.accumulate(c["desc"], c["centres"], np.array([0, n]), c["scale"])
    acc, count = acc[0].copy(), count[0].copy()
    C = len(count)
    for v in (0, 1):
        count[rng.integers(C)] = v
    if rng.integers(4) == 0:
        acc[rng.integers(C)] = rng.integers(-2 ** 62, 2 ** 62, 128)
    return centres_both(c["centres"], acc, count, c["scale"])[0]


def gen_acc(rng, n_img=None, C=None):
    n_img = int(rng.choice([1, 2, 3, 17, 64, 65])) if n_img is None else n_img
    C = int(rng.choice([1, 2, 16, 63, 64, 65, 256])) if C is None else C
    mag = rng.choice([1, 3, 2 ** 10, 2 ** 31, 2 ** 53, 2 ** 62])
    acc = rng.integers(-int(mag), int(mag) + 1, (n_img, C, 128), dtype=np.int64)
    sparse = rng.random((n_img, C)) < 0.3
    acc[sparse] = 0
    if rng.integers(3) == 0:
        acc[rng.random((n_img, C)) < 0.3] = rng.choice([1, -1, 2 ** 53 + 1, -(2 ** 53 + 1), 2 ** 62, -(2 ** 62)])
    return acc


def fuzz_signature(rng):
    return signature_both(gen_acc(rng), bool(rng.integers(2)), float(rng.choice([1.0, 127.0, 254.0, 1000.0, 126.5])))[0]


def gen_signatures(rng, n_img=None, C=None):
    n_img = int(rng.choice([1, 2, 3, 15, 16, 17, 63, 64, 65, 100])) if n_img is None else n_img
    C = int(rng.choice([1, 2, 3, 16, 64])) if C is None else C
    sig, norm2 = nr.signatures(gen_acc(rng, n_img, C), bool(rng.integers(2)), float(rng.choice([127.0, 254.0, 20.0])))
    if n_img > 1:
        m = int(rng.integers(0, n_img // 2 + 1))
        a, b = rng.integers(n_img, size=m), rng.integers(n_img, size=m)
        sig[a] = sig[b]                                              # equal rows: exact ties
        a, b = rng.integers(n_img, size=m // 2), rng.integers(n_img, size=m // 2)
        sig[a] = -sig[b]                                             # opposite rows: sim = -1
    norm2 = (sig.astype(np.int64) ** 2).sum(1).astype(np.int32)
    return sig, norm2


def fuzz_shortlist(rng):
    sig, norm2 = gen_signatures(rng)
    n_img = len(norm2)
    k = int(rng.choice([1, 2, max(n_img - 1, 1), min(n_img, 64), 64, int(rng.integers(1, 65))]))
    k = min(max(k, 1), 64)
    min_sim = rng.choice([None, -np.inf, -1.0, 0.0, 1.0, np.inf, 0.3])
    if rng.integers(3) == 0:                                         # a row's own k-th value, or the float above it
        _, sims = nr.shortlist(sig, norm2, k)
        v = sims[np.isfinite(sims)]
        if len(v):
            min_sim = float(rng.choice(v))
            if rng.integers(2):
                min_sim = float(np.nextafter(np.float32(min_sim), np.float32(2)))
    return shortlist_both(sig, norm2, k, None if min_sim is None else float(min_sim))[0]


def gen_nbr(rng):
    n_img = int(rng.choice([1, 2, 3, 31, 32, 33, 64, 65, 200])) if rng.integers(2) else log_uniform_from_zero(rng, 300) + 1
    k = int(rng.choice([1, 2, 8, 64])) if rng.integers(2) else int(rng.integers(1, 65))
    nbr = rng.integers(0, n_img, (n_img, k)).astype(np.int32)
    nbr[rng.random(nbr.shape) < rng.choice([0.0, 0.3, 0.9, 1.0])] = -1
    bad = rng.random(nbr.shape) < 0.05
    nbr[bad] = rng.choice([-7, n_img, n_img + 5, 2 ** 31 - 1], int(bad.sum()))
    if rng.integers(4) == 0:                                         # a star: everybody names image 0
        nbr[:, 0] = 0
    return nbr


def fuzz_pairs(rng):
    nbr = gen_nbr(rng)
    mutual = bool(rng.integers(2))
    total = int(nr.pair_list(nbr, mutual)[1][0])
    cap = rng.choice([None, 0, max(total - 1, 0), total, total + 3])
    return pairs_both(nbr, mutual, None if cap is None else int(cap))[0]


def fuzz_composed(rng):
    import retrieval_cases as rc
    from sfm_mvs_amd import retrieval
    n_img = int(rng.integers(2, 9))
    sc = rc.corridor_scene(n_img, int(rng.choice([20, 50])), int(rng.choice([5, 10])), int(rng.choice([0, 10])), int(rng.integers(1 << 20)))
    kw = dict(k=int(rng.integers(1, 6)), n_centres=int(rng.choice([1, 4, 16])), iters=int(rng.integers(0, 4)), seed=int(rng.integers(100)),
              ssr=bool(rng.integers(2)), mutual=bool(rng.integers(2)), min_sim=rng.choice([None, 0.0, 0.2]))
    want, st = nr.select_pairs(sc["descs"], **kw)
    got, dv = retrieval.select_pairs([dev(d) for d in sc["descs"]], **kw)
    return first("" if got == want else f"pairs: {got[:5]} vs {want[:5]}", *[same(n, dv[n], st[n]) for n in ("centres", "sig", "nbr", "nbr_sim")])


FAMILIES = [("accumulate", fuzz_accumulate, 4), ("centres", fuzz_centres, 1), ("signature", fuzz_signature, 2), ("shortlist", fuzz_shortlist, 3),
            ("pairs", fuzz_pairs, 2), ("composed", fuzz_composed, 1)]


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
            log(f"MISMATCH {name} (seed {seed}, case seed {case_seed}; replay: fuzz_retrieval.py 0 0 {name}:{case_seed}) {msg}")
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
        print(f"fuzz_retrieval replay {name}:{case_seed}: {msg or 'no mismatch'}")
        return 1 if msg else 0
    counts, bad, dt = run(budget, seed, log=lambda s: print(s, flush=True))
    print(f"fuzz_retrieval: seed {seed}, {sum(counts.values())} cases {counts}, {bad} mismatches, {dt:.0f} s")
    print(f"sfm_build_id {_lib.build_id()}")
    print(json.dumps(dict(tool="fuzz_retrieval", seed=seed, cases=sum(counts.values()), families=counts, mismatches=bad, seconds=round(dt, 1))))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
