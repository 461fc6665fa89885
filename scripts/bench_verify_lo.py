"""Times the local optimisation of the batched verification (VERIFY-LO, docs/tracks.md §12) on the workload of scripts/bench_verify.py
(64 images x 10 000 features, 2 016 pairs, default budget) and writes one JSON line (default: profiles/verify_lo_bench.json).

  python scripts/bench_verify_lo.py [--images 64] [--budget H] [--top T --rounds R] [--out PATH] [--once]

`verify_pairs` with lo=None, with the default lo and with the setting of --top / --rounds (default 8 x 4, the multiplier of the default in
every round) runs in alternating calls in one process, each by the wall clock around a synchronised call (the median and the minimum of
5 rounds after one warm-up of each).  The three new launches are timed with HIP events on one chunk's worth of all pairs (the median of 5
calls after 2 warm-ups).  --once runs verify_pairs with both lo settings once and leaves (for a kernel trace collected in a run of its own:
profiles/verify_lo_kernel_stats.csv)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "scripts"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--budget", type=int, default=None)
    ap.add_argument("--top", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_lo_bench.json"))
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    import torch
    from bench_tracks import timed
    from datagen import ring_scene
    from sfm_mvs_amd import _lib, sharded, tracks, verify
    dev = torch.device("cuda:0")
    H = verify.DEFAULT_BUDGET if args.budget is None else args.budget
    n_img, n_desc, n_scene = args.images, 10_000, 7_000
    K, P, image = ring_scene(n_img, n_desc, n_scene, seed=11)
    ims = [image(k) for k in range(n_img)]
    kps = [torch.from_numpy(im[0]).to(dev) for im in ims]
    des = [torch.from_numpy(im[1]).to(dev) for im in ims]
    pairs = sharded.all_pairs(n_img)
    store, nq = sharded.match_pairs_sharded(des, pairs, batch=8)
    store = store.contiguous()
    del des
    img_off, kp, nqd, prd, _, n = tracks._scene_tensors(nq, pairs, kps, None, dev)
    n_pairs, cap = int(store.shape[0]), int(store.shape[2])
    big = dict(top=args.top, rounds=args.rounds)
    settings = {"plain": None, "default": True, "big": big}

    def call(lo):
        return verify.verify_pairs(store, nqd, prd, img_off, kp, K, budget=H, lo=lo)

    outs = {name: call(lo) for name, lo in settings.items()}         # warm-up: allocations and module loading
    torch.cuda.synchronize()
    if args.once:
        print("bench_verify_lo: one pass of each setting done")
        return 0

    wall = {name: [] for name in settings}
    for _ in range(5):                                               # alternating calls, one process
        for name, lo in settings.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            call(lo)
            torch.cuda.synchronize(); wall[name].append(time.perf_counter() - t0)

    # the three launches on one chunk of pairs
    thr2 = verify.thr2_of(K)
    k = min(verify.pairs_per_chunk(H), n_pairs)
    xn = verify.normalise_keypoints(kp, K)
    surv, m = verify.survivors(store, nqd, prd, img_off)
    part = (surv[:k], m[:k], prd[:k], img_off, xn)
    nmodels, E = verify.models(verify.samples(m[:k], H), *part)
    counts, _ = verify.score(E, nmodels, *part, thr2)
    ms = {}
    for name, lo in (("default", True), ("big", big)):
        T, widen = verify.lo_settings(lo)
        wide2 = [verify.thr2_of(K, w * verify.DEFAULT_THRESHOLD) for w in widen]
        top = verify.top_models(counts, nmodels, T)
        cand = verify.local_optimise(E, top, *part, thr2, wide2)
        sel = verify.pick(top, *cand, H)
        ms[name] = {"pairs": k, "top": T, "rounds": len(widen),
                    "top_models": timed(lambda: verify.top_models(counts, nmodels, T, out=top), 2, 5),
                    "local_optimise": timed(lambda: verify.local_optimise(E, top, *part, thr2, wide2, out=cand), 2, 5),
                    "pick": timed(lambda: verify.pick(top, *cand, H, out=sel), 2, 5)}

    info = {name: o["info"].cpu().numpy() for name, o in outs.items()}
    lo_info = {name: outs[name]["lo_info"].cpu().numpy() for name in ("default", "big")}
    med = {name: float(np.median(w)) for name, w in wall.items()}
    res = {"workload": f"verify_pairs on the all-pairs ring scene: {n_img} images x {n_desc}, {n_pairs} pairs, cap {cap}, budget {H}",
           "settings": {"default": verify.DEFAULT_LO, "big": big},
           "verify_pairs_wall_s_median": med, "verify_pairs_wall_s_min": {name: float(min(w)) for name, w in wall.items()},
           "lo_over_plain": {name: med[name] / med["plain"] for name in ("default", "big")},
           "ms_median_min_one_chunk": ms,
           "workspace_bytes": {name: verify.workspace_bytes(n_pairs, cap, H, lo=lo) for name, lo in settings.items()},
           "sampson_inliers_total": {name: int(i[:, 2].sum()) for name, i in info.items()},
           "cheirality_inliers_total": {name: int(i[:, 3].sum()) for name, i in info.items()},
           "pairs_improved": {name: int((li[:, 1] > li[:, 0]).sum()) for name, li in lo_info.items()},
           "pairs_won_by_a_refit": {name: int((li[:, 3] >= 0).sum()) for name, li in lo_info.items()},
           "build_id_verify_lo": _lib.code_hashes_of_binary().get("verify_lo.hip"), "build_id_verify": _lib.code_hashes_of_binary().get("verify.hip")}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
