"""Times the VERIFY family on the all-pairs scene of `bench.py --workload allpairs` (64 images x 10 000 features, 2 016 pairs) at the
default budget and writes one JSON line (default: profiles/verify_bench.json).

  python scripts/bench_verify.py [--images 64] [--budget H] [--subset 64] [--out PATH] [--once]

Each stage is timed with HIP events on the current stream (the median of 5 calls after 2 warm-ups), `verify_pairs` as a whole by the wall
clock around a synchronised call.  The per-pair path (`tracks.verify_keep` without `batched`) runs in the same process, in calls that
alternate with the batched one, on a fixed subset of pairs (every n_pairs / subset-th) and is reported as ms per pair.  `run_tracks`
runs on that subset with the `keep` of each path: tracks kept and tracks pure.  The scoring rate stands beside the float64 vector rate
of the chip (78.6 TFLOP/s with every operation a fused multiply-add; half of it for the separately rounded multiplies and adds the
specification asks for; 39 operations per Sampson evaluation, one of them a division).  --once runs verify_pairs once and leaves (for a
kernel trace collected in a run of its own)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "scripts"))

F64_VECTOR_OPS_PER_S = 78.6e12 / 2
SAMPSON_OPS = 39


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--budget", type=int, default=None)
    ap.add_argument("--subset", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_bench.json"))
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
    ids = [im[2] for im in ims]
    pairs = sharded.all_pairs(n_img)
    store, nq = sharded.match_pairs_sharded(des, pairs, batch=8)
    store = store.contiguous()
    del des
    img_off, kp, nqd, prd, _, n = tracks._scene_tensors(nq, pairs, kps, None, dev)
    n_pairs, cap = int(store.shape[0]), int(store.shape[2])

    out = verify.verify_pairs(store, nqd, prd, img_off, kp, K, budget=H)
    torch.cuda.synchronize()
    if args.once:
        print("bench_verify: one pass done")
        return 0

    thr2 = verify.thr2_of(K)
    xn = verify.normalise_keypoints(kp, K)
    surv, m = verify.survivors(store, nqd, prd, img_off)
    samp = verify.samples(m, H)
    nmodels, E = verify.models(samp, surv, m, prd, img_off, xn)
    counts, best = verify.score(E, nmodels, surv, m, prd, img_off, xn, thr2)
    sel = verify.select(E, nmodels, best, surv, m, prd, img_off, xn, thr2)
    ms = {"normalise": timed(lambda: verify.normalise_keypoints(kp, K, out=xn), 2, 5),
          "survivors": timed(lambda: verify.survivors(store, nqd, prd, img_off, out=(surv, m)), 2, 5),
          "samples": timed(lambda: verify.samples(m, H, out=samp), 2, 5),
          "models": timed(lambda: verify.models(samp, surv, m, prd, img_off, xn, out=(nmodels, E)), 1, 3),
          "score": timed(lambda: verify.score(E, nmodels, surv, m, prd, img_off, xn, thr2, out=(counts, best)), 1, 3),
          "select": timed(lambda: verify.select(E, nmodels, best, surv, m, prd, img_off, xn, thr2, out=sel), 2, 5)}
    info = out["info"].cpu().numpy()
    models_scored, survivors_total = int(info[:, 1].sum()), int(info[:, 0].sum())
    evals = int((info[:, 1].astype(np.int64) * info[:, 0].astype(np.int64)).sum())

    rows = list(range(0, n_pairs, max(n_pairs // args.subset, 1)))[:args.subset]
    idx = torch.tensor(rows, dtype=torch.long, device=dev)
    sub_store, sub_nq, sub_pairs = store[idx].contiguous(), [nq[r] for r in rows], [pairs[r] for r in rows]
    wall_b, wall_s = [], []
    for _ in range(3):                                             # alternating calls, one process
        torch.cuda.synchronize(); t0 = time.perf_counter()
        out = verify.verify_pairs(store, nqd, prd, img_off, kp, K, budget=H)
        torch.cuda.synchronize(); wall_b.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        keep_s = tracks.verify_keep(sub_store, sub_nq, sub_pairs, kps, K)
        torch.cuda.synchronize(); wall_s.append(time.perf_counter() - t0)
    keep_b = out["keep"][idx].contiguous()

    def tracks_of(keep):
        return len(tracks.run_tracks(sub_store, sub_nq, sub_pairs, kps, P, keep=keep, max_reproj=2.0)["track_len"])
    n_b, n_s, n_0 = tracks_of(keep_b), tracks_of(keep_s), tracks_of(None)

    def pure(keep):
        """Tracks over the subset's edges under `keep` whose nodes show one scene point and no clutter."""
        edges = tracks.match_edges(sub_store, nqd[idx].contiguous(), prd[idx].contiguous(), img_off, keep=keep)
        labels, _ = tracks.track_components(edges, n, rounds=64)
        node_track, track_off, obs_node, cnt = tracks.build_tracks(labels, img_off)
        c = cnt.cpu().numpy()
        T, nobs = int(c[0]), int(c[1])
        off_h, obs_h = track_off[:T + 1].cpu().numpy(), obs_node[:nobs].cpu().numpy()
        node_ids = np.concatenate(ids)
        tr = np.repeat(np.arange(T), np.diff(off_h))
        lo, hi = np.full(T, np.iinfo(np.int64).max), np.full(T, -2)
        np.minimum.at(lo, tr, node_ids[obs_h]); np.maximum.at(hi, tr, node_ids[obs_h])
        return T, int(((lo == hi) & (lo >= 0)).sum())
    built = {"batched": pure(keep_b), "per_pair": pure(keep_s), "unverified": pure(None)}

    ws = verify.workspace_bytes(n_pairs, cap, H)
    res = {"workload": f"verify on the all-pairs ring scene: {n_img} images x {n_desc}, {n_pairs} pairs, cap {cap}, budget {H}",
           "ms_median_min": ms, "verify_pairs_wall_s_median": float(np.median(wall_b)), "verify_pairs_wall_s_min": float(min(wall_b)),
           "workspace_bytes": ws, "models_bytes": n_pairs * H * 720, "survivors": survivors_total, "models_scored": models_scored,
           "sampson_evaluations": evals, "hypotheses_per_s": n_pairs * H / (ms["models"][0] * 1e-3),
           "sampson_evaluations_per_s": evals / (ms["score"][0] * 1e-3),
           "score_share_of_f64_vector_rate": evals * SAMPSON_OPS / (ms["score"][0] * 1e-3) / F64_VECTOR_OPS_PER_S,
           "status_counts": {"few_survivors": int((info[:, 7] & 1 != 0).sum()), "no_model": int((info[:, 7] & 2 != 0).sum()), "no_vote": int((info[:, 7] & 4 != 0).sum())},
           "pairs_beyond_budget_at_0.999": int((verify.confidence_iters(info) > H).sum()),
           "per_pair_subset": len(rows), "per_pair_ms_per_pair_median": float(np.median(wall_s)) / len(rows) * 1e3,
           "batched_ms_per_pair_median": float(np.median(wall_b)) / n_pairs * 1e3,
           "ratio_per_pair_over_batched": (float(np.median(wall_s)) / len(rows)) / (float(np.median(wall_b)) / n_pairs),
           "keep_on_subset": {"batched": int(keep_b.sum()), "per_pair": int(keep_s.sum())},
           "run_tracks_points_kept_at_2px_on_subset": {"batched": n_b, "per_pair": n_s, "unverified": n_0},
           "tracks_built_and_pure_on_subset": {k: {"tracks": v[0], "pure": v[1]} for k, v in built.items()},
           "build_id_verify": _lib.code_hashes_of_binary().get("verify.hip")}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
