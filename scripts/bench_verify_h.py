"""Times the homography of the batched verification (VERIFY-H, docs/tracks.md §13) on the workload of scripts/bench_verify.py
(64 images x 10 000 features, 2 016 pairs, default budget) and writes one JSON line (default: profiles/verify_h_bench.json).

  python scripts/bench_verify_h.py [--images 64] [--budget H] [--out PATH] [--once]

`verify_pairs` with homography=None and with the default runs in alternating calls in one process, each by the wall clock around a
synchronised call (the median and the minimum of 5 rounds after one warm-up of each).  The three new launches are timed with HIP events
on one chunk's worth of all pairs (the median of 5 calls after 2 warm-ups), sfm_verify_score beside them.  --once runs verify_pairs with
both settings once and leaves (for a kernel trace collected in a run of its own: profiles/verify_h_kernel_stats.csv)."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_h_bench.json"))
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
    settings = {"plain": None, "homography": True}

    def call(h):
        return verify.verify_pairs(store, nqd, prd, img_off, kp, K, budget=H, homography=h)

    outs = {name: call(h) for name, h in settings.items()}           # warm-up: allocations and module loading
    torch.cuda.synchronize()
    if args.once:
        print("bench_verify_h: one pass of each setting done")
        return 0

    wall = {name: [] for name in settings}
    for _ in range(5):                                               # alternating calls, one process
        for name, h in settings.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            call(h)
            torch.cuda.synchronize(); wall[name].append(time.perf_counter() - t0)

    # the launches on one chunk of pairs
    hs = verify.homography_settings(True)
    thr2, thr2h = verify.thr2_of(K), verify.thr2_of(K, hs["threshold"])
    k = min(verify.pairs_per_chunk(H), n_pairs)
    xn = verify.normalise_keypoints(kp, K)
    surv, m = verify.survivors(store, nqd, prd, img_off)
    part = (surv[:k], m[:k], prd[:k], img_off, xn)
    samp = verify.samples(m[:k], H)
    nmodels, E = verify.models(samp, *part)
    e_out = verify.score(E, nmodels, *part, thr2)
    ok, Hm = verify.h_models(samp, *part)
    sc = verify.h_score(Hm, ok, *part, thr2h)
    sel = verify.h_select(Hm, ok, sc[1], *part, thr2h, hs["refit"])
    ms = {"pairs": k,
          "score": timed(lambda: verify.score(E, nmodels, *part, thr2, out=e_out), 2, 5),
          "h_models": timed(lambda: verify.h_models(samp, *part, out=(ok, Hm)), 2, 5),
          "h_score": timed(lambda: verify.h_score(Hm, ok, *part, thr2h, out=sc), 2, 5),
          "h_select": timed(lambda: verify.h_select(Hm, ok, sc[1], *part, thr2h, hs["refit"], out=sel), 2, 5)}
    mk = m[:k].to(torch.int64).clamp(0, cap)
    evals = {"score": int((nmodels.clamp(0, verify.SLOTS).sum(1, dtype=torch.int64) * mk).sum()), "h_score": int(((ok != 0).sum(1, dtype=torch.int64) * mk).sum())}
    rate = {name: evals[name] / (ms[name][0] * 1e-3) for name in evals}

    full = outs["homography"]
    config = full["config"].cpu().numpy()
    h_info = full["h_info"].cpu().numpy()
    med = {name: float(np.median(w)) for name, w in wall.items()}
    res = {"workload": f"verify_pairs on the all-pairs ring scene: {n_img} images x {n_desc}, {n_pairs} pairs, cap {cap}, budget {H}",
           "settings": verify.DEFAULT_HOMOGRAPHY,
           "verify_pairs_wall_s_median": med, "verify_pairs_wall_s_min": {name: float(min(w)) for name, w in wall.items()},
           "homography_over_plain": med["homography"] / med["plain"],
           "ms_median_min_one_chunk": ms, "evaluations_one_chunk": evals, "evaluations_per_s": rate,
           "workspace_bytes": {name: verify.workspace_bytes(n_pairs, cap, H, homography=h) for name, h in settings.items()},
           "config_counts": {name: int((config == w).sum()) for name, w in (("none", 0), ("general", 1), ("planar", 2), ("rotating", 3))},
           "h_inliers_total": int(h_info[:, 2].sum()), "pairs_won_by_the_refit": int((h_info[:, 5] == 0).sum()),
           "keep_E_Rt_info_unchanged": all(bool(torch.equal(outs["plain"][n_].view(torch.uint8), full[n_].view(torch.uint8))) for n_ in outs["plain"]),
           "build_id_verify_h": _lib.code_hashes_of_binary().get("verify_h.hip"), "build_id_verify": _lib.code_hashes_of_binary().get("verify.hip")}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
