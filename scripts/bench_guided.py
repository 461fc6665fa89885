"""Times guided matching (GUIDED, docs/tracks.md §14) on an all-pairs ring scene with twins (64 images x 10 000 features, 2 016 pairs) at
the default threshold (or --threshold) and writes one JSON line (default: profiles/guided_bench.json; profiles/guided_bench_0p8px.json is
the same run at --threshold 0.8).

  python scripts/bench_guided.py [--images 64] [--twins 0.25] [--threshold PX] [--out PATH] [--once] [--plain [--tree ROOT --label NAME]]

`guided_pairs` and `verify_pairs` run in alternating calls in one process, each by the wall clock around a synchronised call (the median
and the minimum of 5 rounds after one warm-up of each).  The match kernel is timed with HIP events over all pairs (the median of 5 calls
after 2 warm-ups) beside sfm_verify_score on one chunk; band tests per second beside Sampson evaluations per second.  Survivors, kept
matches and full-length tracks of `run_tracks` are counted for the plain path and for `guided_keep`.
--once runs verify_pairs and guided_pairs once, prints the two evaluation counts and leaves (for a kernel trace collected in a run of its
own: profiles/guided_kernel_stats.csv).
--plain times `verify_pairs` and `run_tracks` alone, with nothing of this family called, from the package under ROOT (this tree by
default): run alternately on two trees it shows that the existing paths take the time they took (profiles/guided_plain_ab.txt)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--twins", type=float, default=0.25)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guided_bench.json"))
    ap.add_argument("--threshold", type=float, default=None, help="the band in pixels (default: guided.DEFAULT_GUIDED_THRESHOLD)")
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--plain", action="store_true")
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--label", default="this tree")
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    sys.path.insert(0, os.path.join(ROOT, "scripts")); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, tree)
    import torch
    from sfm_mvs_amd import _lib, sharded, tracks, verify            # the package of `tree`, before anything else puts a root on the path
    import guided_cases as gc
    from bench_tracks import timed
    dev = torch.device("cuda:0")
    n_img, n_kp = args.images, 10_000
    sc = gc.twin_scene(n_img, n_kp, args.twins, 11, ring=n_img)
    kps = [torch.from_numpy(k).to(dev) for k in sc["kps"]]
    des = [torch.from_numpy(d).to(dev) for d in sc["descs"]]
    pairs = sharded.all_pairs(n_img)
    store, nq = sharded.match_pairs_sharded(des, pairs, batch=8)
    store = store.contiguous()
    img_off, kp, nqd, prd, _, n = tracks._scene_tensors(nq, pairs, kps, None, dev)
    n_pairs, cap = int(store.shape[0]), int(store.shape[2])
    K, P = sc["K"], sc["P"]

    def wall_of(fn, rounds=5):
        fn()
        out = []
        for _ in range(rounds):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(); out.append(time.perf_counter() - t0)
        return out

    if args.plain:
        first = verify.verify_pairs(store, nqd, prd, img_off, kp, K)
        w_v = wall_of(lambda: verify.verify_pairs(store, nqd, prd, img_off, kp, K))
        w_t = wall_of(lambda: tracks.run_tracks(store, nq, pairs, kps, P, keep=first["keep"]), 3)
        print(json.dumps({"tree": args.label, "images": n_img, "pairs": n_pairs, "verify_pairs_wall_s": [round(w, 4) for w in w_v],
                          "run_tracks_wall_s": [round(w, 4) for w in w_t], "build_id_verify": _lib.code_hashes_of_binary().get("verify.hip"),
                          "has_guided": "guided.hip" in _lib.code_hashes_of_binary()}))
        return 0

    from sfm_mvs_amd import guided
    desc = torch.cat(des).contiguous()
    thr_px = guided.DEFAULT_GUIDED_THRESHOLD if args.threshold is None else args.threshold
    kw = dict(cap=cap, max_size=n_kp, threshold=thr_px)
    first = verify.verify_pairs(store, nqd, prd, img_off, kp, K)     # warm-up: allocations and module loading
    g = guided.guided_pairs(desc, nqd, prd, img_off, kp, K, first["E"], first["info"], **kw)
    torch.cuda.synchronize()
    active = first["info"][:, 2] >= guided.DEFAULT_MIN_INLIERS
    sizes = torch.from_numpy(np.asarray(sc["sizes"], np.int64)).to(dev)
    band_tests = int((active.to(torch.int64) * nqd.to(torch.int64).clamp(0, cap) * sizes[prd[:, 1].long()]).sum())
    H = verify.DEFAULT_BUDGET
    k = min(verify.pairs_per_chunk(H), n_pairs)
    xn = verify.normalise_keypoints(kp, K)
    surv, m = verify.survivors(store, nqd, prd, img_off)
    part = (surv[:k], m[:k], prd[:k], img_off, xn)
    samp = verify.samples(m[:k], H)
    nmodels, E = verify.models(samp, *part)
    thr2 = verify.thr2_of(K)
    e_out = verify.score(E, nmodels, *part, thr2)
    sampson = int((nmodels.clamp(0, verify.SLOTS).sum(1, dtype=torch.int64) * m[:k].to(torch.int64).clamp(0, cap)).sum())
    if args.once:
        print(json.dumps({"once": True, "band_tests_guided_match_kernel": band_tests, "sampson_evaluations_score_kernel_one_chunk": sampson,
                          "score_kernel_launches": 1 + (n_pairs + k - 1) // k, "pairs_of_the_chunk": k}))
        return 0

    wall = {"verify_pairs": [], "guided_pairs": []}
    for _ in range(5):                                               # alternating calls, one process
        torch.cuda.synchronize(); t0 = time.perf_counter()
        verify.verify_pairs(store, nqd, prd, img_off, kp, K)
        torch.cuda.synchronize(); wall["verify_pairs"].append(time.perf_counter() - t0); t0 = time.perf_counter()
        guided.guided_pairs(desc, nqd, prd, img_off, kp, K, first["E"], first["info"], **kw)
        torch.cuda.synchronize(); wall["guided_pairs"].append(time.perf_counter() - t0)

    thr2g = verify.thr2_of(K, thr_px)
    act8 = active.to(torch.uint8)
    rev = torch.empty((n_pairs, n_kp), dtype=torch.int64, device=dev)
    out = torch.empty_like(g["store"])
    mk = (torch.empty_like(g["keep"]), torch.empty_like(g["info"]))
    ms = {"guided_match": timed(lambda: guided.guided_match(desc, xn, first["E"], act8, nqd, prd, img_off, cap, thr2g, out=out, rev=rev), 2, 5),
          "guided_mutual": timed(lambda: guided.guided_mutual(out, rev, nqd, prd, img_off, out=mk), 2, 5),
          "score_one_chunk": timed(lambda: verify.score(E, nmodels, *part, thr2, out=e_out), 2, 5)}
    assert torch.equal(out, g["store"])
    rate = {"band_tests_per_s": band_tests / (ms["guided_match"][0] * 1e-3), "sampson_evaluations_per_s": sampson / (ms["score_one_chunk"][0] * 1e-3)}

    # candidates per query on eight pairs, by torch operations on the band's words (float64, one operation a call)
    cands, queries = 0, 0
    for p in np.linspace(0, n_pairs - 1, 8).astype(int):
        if not bool(active[p]):
            continue
        i, j = pairs[p]
        Em = first["E"][p]
        x1, x2 = xn[int(img_off[i]):int(img_off[i + 1])], xn[int(img_off[j]):int(img_off[j + 1])]
        a1, b1, a2, b2 = x1[:, :1], x1[:, 1:], x2[:, 0][None], x2[:, 1][None]
        e0, e1, e2 = Em[0] * a1 + Em[1] * b1 + Em[2], Em[3] * a1 + Em[4] * b1 + Em[5], Em[6] * a1 + Em[7] * b1 + Em[8]
        f0, f1 = Em[0] * a2 + Em[3] * b2 + Em[6], Em[1] * a2 + Em[4] * b2 + Em[7]
        s = a2 * e0 + b2 * e1 + e2
        cands += int(((s * s / (((e0 * e0 + e1 * e1) + f0 * f0) + f1 * f1)).to(torch.float32) <= thr2g).sum())
        queries += len(x1)

    full = lambda res: int((res["track_len"] == n_img).sum())        # noqa: E731
    long_ = lambda res: int((res["track_len"] >= n_img // 2).sum())   # noqa: E731
    t_plain = tracks.run_tracks(store, nq, pairs, kps, P, keep=first["keep"])
    store_g, keep_g = tracks.guided_keep(des, store, nq, pairs, kps, K, guided_threshold=thr_px)
    t_guided = tracks.run_tracks(store_g, nq, pairs, kps, P, keep=keep_g)
    w_t = wall_of(lambda: tracks.run_tracks(store, nq, pairs, kps, P, keep=first["keep"]), 3)
    info_g = g["info"].cpu().numpy()
    med = {name: float(np.median(w)) for name, w in wall.items()}
    res = {"workload": f"guided_pairs on the all-pairs ring scene with twins: {n_img} images x {n_kp}, twin share {args.twins}, {n_pairs} pairs, cap {cap}",
           "threshold_px": thr_px, "min_inliers": guided.DEFAULT_MIN_INLIERS, "active_pairs": int(active.sum()),
           "wall_s_median": med, "wall_s_min": {name: float(min(w)) for name, w in wall.items()}, "guided_over_verify": med["guided_pairs"] / med["verify_pairs"],
           "run_tracks_plain_wall_s": [round(w, 4) for w in w_t],
           "ms_median_min": ms, "band_tests": band_tests, "sampson_evaluations_one_chunk": sampson, "rates": rate,
           "match_over_score_rate": rate["band_tests_per_s"] / rate["sampson_evaluations_per_s"],
           "candidates_per_query_eight_pairs": cands / max(queries, 1),
           "queries_in_range": int(info_g[:, 0].sum()), "queries_with_a_candidate": int(info_g[:, 1].sum()), "queries_with_two": int(info_g[:, 2].sum()),
           "queries_mutual": int(info_g[:, 3].sum()),
           "survivors": {"plain": int(m.sum()), "guided": int(verify.survivors(store_g, nqd, prd, img_off)[1].sum())},
           "kept": {"plain": int(first["keep"].sum()), "guided": int(keep_g.sum())},
           "tracks_full_length": {"plain": full(t_plain), "guided": full(t_guided)},
           "tracks_half_length_or_more": {"plain": long_(t_plain), "guided": long_(t_guided)},
           "tracks": {"plain": int(len(t_plain["track_len"])), "guided": int(len(t_guided["track_len"]))},
           "workspace_bytes": guided.workspace_bytes(n_pairs, n_kp),
           "build_id_guided": _lib.code_hashes_of_binary().get("guided.hip"), "build_id_verify": _lib.code_hashes_of_binary().get("verify.hip")}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
