"""Times the RETRIEVAL family (docs/retrieval.md §4) on two inputs and writes one JSON line (default: profiles/retrieval_bench.json):
  bench      the all-pairs bench scene of the verification and guided benchmarks: 64 images x 10 000 keypoints
  corridor   a corridor of 1 024 images x 2 000 keypoints (window 1 600, step 160, clutter 400)

  python scripts/bench_retrieval.py [--out PATH] [--once] [--only bench|corridor]

Every entry point by HIP events, the median (and minimum) of 10 calls after 3 warm-ups (docs/measurement.md), beside its floor: the
bytes it moves at the HBM rate (accumulate reads every descriptor row twice, and the floor counts both), for `accumulate` also 3 * 128 * C * N float32 vector operations at the packed vector rate, for
`shortlist` 2 * n_img^2 * C * 128 int8 operations at the dense i8 roof.  `select_pairs` and `train_vocabulary` by the wall clock around
a synchronised call (median of 5 after one warm-up).  The time of the steps the shortlist spares is the per-pair cost of
profiles/verify_bench.json and profiles/guided_bench.json (and 42 ms per 2 016 pairs of matching) times the pairs it removes.
--once runs every entry point once on the bench scene and leaves (for a kernel trace collected in a run of its own:
profiles/retrieval_kernel_stats.csv)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_BYTES_PER_S = 6.3e12                   # what a streaming kernel sustains here (scripts/bench_tracks.py)
F32_VECTOR_OPS_PER_S = 157.3e12 / 2        # packed float32 vector operations: half the FMA FLOP rate (benchlib/common.py)
I8_OPS_PER_S = 5000e12                     # the dense int8 roof of the README (benchlib/common.py)
MATCH_S_PER_PAIR = 0.042 / 2016            # README: 64 images, 2 016 pairs, 42 ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "retrieval_bench.json"))
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--only", default=None)
    ap.add_argument("--centres", type=int, default=64)
    ap.add_argument("--k", type=int, default=8)
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "scripts")); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, ROOT)
    import torch
    from sfm_mvs_amd import _lib, retrieval
    import guided_cases as gc
    import retrieval_cases as rc
    from bench_tracks import timed
    dev = torch.device("cuda:0")
    C, k = args.centres, args.k

    def per_pair(name, key):
        with open(os.path.join(ROOT, "profiles", name)) as f:
            return json.loads(f.readline())[key]
    verify_s = per_pair("verify_bench.json", "verify_pairs_wall_s_median") / 2016
    guided_s = per_pair("guided_bench.json", "wall_s_median")["guided_pairs"] / 2016

    def wall_of(fn, rounds=5):
        fn()
        out = []
        for _ in range(rounds):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(); out.append(time.perf_counter() - t0)
        return float(np.median(out)), float(min(out))

    def measure(name, descs, shared=None):
        sizes = [len(d) for d in descs]
        n_img, N = len(sizes), int(sum(sizes))
        des = [torch.from_numpy(d).to(dev) for d in descs]
        desc = torch.cat(des).contiguous()
        img_off = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)).to(dev)
        one = torch.tensor([0, N], dtype=torch.int32, device=dev)
        scale = retrieval.scale_of()
        centres = retrieval.train_vocabulary(desc, C, 8, 0, scale)
        acc_out = retrieval.assign_accumulate(desc, centres, img_off, scale)
        one_out = retrieval.assign_accumulate(desc, centres, one, scale)
        sig_out = retrieval.signatures(acc_out[1])
        ws = torch.empty(int(_lib.lib().sfm_vlad_shortlist_ws_bytes(n_img)), dtype=torch.uint8, device=dev)
        nbr_out = retrieval.shortlist(*sig_out, k, workspace=ws)
        pr_out = retrieval.pair_list(nbr_out[0])
        if args.once:
            retrieval.update_centres(centres, one_out[1], one_out[2], scale)
            torch.cuda.synchronize()
            return dict(input=name, images=n_img, nodes=N, selected=int(pr_out[1][0]))
        cen_out = torch.empty_like(centres)
        ms = {"accumulate": timed(lambda: retrieval.assign_accumulate(desc, centres, img_off, scale, out=acc_out)),
              "accumulate_one_image": timed(lambda: retrieval.assign_accumulate(desc, centres, one, scale, out=one_out)),
              "centres": timed(lambda: retrieval.update_centres(centres, one_out[1], one_out[2], scale, out=cen_out)),
              "signature": timed(lambda: retrieval.signatures(acc_out[1], out=sig_out)),
              "shortlist": timed(lambda: retrieval.shortlist(*sig_out, k, out=nbr_out, workspace=ws)),
              "pairs": timed(lambda: retrieval.pair_list(nbr_out[0], out=pr_out))}
        cells = n_img * C
        floor_ms = {"accumulate": (2 * N * 512 + 2 * N * 4 + cells * 128 * 8 * 2 + cells * 4 * 2) / HBM_BYTES_PER_S * 1e3,
                    "accumulate_vector_ops": 3 * 128 * C * N / F32_VECTOR_OPS_PER_S * 1e3,
                    "accumulate_one_image": (2 * N * 512 + 2 * N * 4) / HBM_BYTES_PER_S * 1e3,
                    "centres": C * 128 * (4 + 8 + 4) / HBM_BYTES_PER_S * 1e3,
                    "signature": cells * 128 * (8 + 1) / HBM_BYTES_PER_S * 1e3,
                    "shortlist": (cells * 128 + n_img * k * 8) / HBM_BYTES_PER_S * 1e3,
                    "shortlist_i8_ops": 2 * n_img * n_img * C * 128 / I8_OPS_PER_S * 1e3,
                    "pairs": (n_img * k * 4 + int(pr_out[1][0]) * 8) / HBM_BYTES_PER_S * 1e3}
        w_train = wall_of(lambda: retrieval.train_vocabulary(desc, C, 8, 0, scale), 3)
        w_sel = wall_of(lambda: retrieval.select_pairs(desc, img_off, k, centres=centres))
        w_sel_train = wall_of(lambda: retrieval.select_pairs(desc, img_off, k, n_centres=C), 3)
        pairs, _ = retrieval.select_pairs(desc, img_off, k, centres=centres)
        n_all = n_img * (n_img - 1) // 2
        removed = n_all - len(pairs)
        res = dict(input=name, images=n_img, nodes=N, centres=C, k=k, all_pairs=n_all, selected=len(pairs), kept_fraction=len(pairs) / n_all,
                   ms_median_min=ms, floor_ms=floor_ms,
                   share_of_floor={"accumulate_of_vector_rate": floor_ms["accumulate_vector_ops"] / ms["accumulate"][0],
                                   "accumulate_of_hbm": floor_ms["accumulate"] / ms["accumulate"][0],
                                   "signature_of_hbm": floor_ms["signature"] / ms["signature"][0],
                                   "shortlist_of_i8_roof": floor_ms["shortlist_i8_ops"] / ms["shortlist"][0],
                                   "shortlist_of_hbm": floor_ms["shortlist"] / ms["shortlist"][0]},
                   train_vocabulary_wall_s_median_min=w_train, select_pairs_wall_s_median_min=w_sel,
                   select_pairs_with_training_wall_s_median_min=w_sel_train,
                   shortlist_workspace_bytes=int(ws.numel()),
                   removed_pairs=removed, removed_pairs_cost_s=dict(matching=removed * MATCH_S_PER_PAIR, verify=removed * verify_s, guided=removed * guided_s))
        if shared is not None:
            res["truth"] = rc.measures(pairs, shared, k)
        return res

    out = {}
    if args.only in (None, "bench"):
        sc = gc.twin_scene(64, 10_000, 0.25, 11, ring=64)
        out["bench"] = measure("bench scene: 64 images x 10 000 keypoints", sc["descs"])
    if args.only in (None, "corridor") and not args.once:
        sc = rc.corridor_scene(1024, 1600, 160, 400, 0)
        order = sc["order"]
        shared = np.maximum(1600 - 160 * np.abs(order[:, None] - order[None, :]), 0)   # the windows' overlap; shared_points() would take minutes
        np.fill_diagonal(shared, 0)
        out["corridor"] = measure("corridor: 1 024 images x 2 000 keypoints", sc["descs"], shared)
    out["build_id_retrieval"] = _lib.code_hashes_of_binary().get("retrieval.hip")
    line = json.dumps(out)
    if not args.once:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
