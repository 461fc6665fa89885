"""Times the TRACKS family on the all-pairs scene of `bench.py --workload allpairs` (64 images x 10 000 features, 2 016 pairs,
N = 640 000 nodes, 20.16 M edge slots) and writes one JSON line (default: profiles/tracks_bench.json).

  python scripts/bench_tracks.py [--images 64] [--out PATH] [--once]

Each entry point is timed with HIP events on the current stream: the median of 10 calls after 3 warm-ups.  Beside each time stands
its byte floor (the words the call must read and write once, over 6.3 TB/s; the labelling's floor counts one pass over the edges and
two over the labels per executed round) and, for the labelling, the CPU time of scipy.sparse.csgraph.connected_components on the
same edges.  --once runs every entry point once and leaves (for a kernel trace collected in a run of its own)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_BYTES_PER_S = 6.3e12


def timed(fn, warm=3, reps=10):
    import torch
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracks_bench.json"))
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    import torch
    from datagen import ring_scene
    from sfm_mvs_amd import _lib, sharded, tracks
    dev = torch.device("cuda:0")
    n_img, n_desc, n_scene = args.images, 10_000, 7_000
    K, P, image = ring_scene(n_img, n_desc, n_scene, seed=11)
    ims = [image(k) for k in range(n_img)]
    kps = [torch.from_numpy(im[0]).to(dev) for im in ims]
    des = [torch.from_numpy(im[1]).to(dev) for im in ims]
    ids = np.concatenate([im[2] for im in ims])
    pairs = sharded.all_pairs(n_img)
    store, nq = sharded.match_pairs_sharded(des, pairs, batch=8)
    store = store.contiguous()
    del des
    img_off, kp, nqd, prd, Pd, n = tracks._scene_tensors(nq, pairs, kps, P, dev)
    n_pairs, cap = int(store.shape[0]), int(store.shape[2])
    ne = n_pairs * cap

    edges = tracks.match_edges(store, nqd, prd, img_off)
    labels, status = tracks.track_components(edges, n)
    node_track, track_off, obs_node, counts = tracks.build_tracks(labels, img_off)
    tri = tracks.triangulate_tracks(counts, track_off, obs_node, img_off, kp, Pd)
    torch.cuda.synchronize()
    if args.once:
        print("bench_tracks: one pass done")
        return 0
    st, ct = status.cpu().numpy(), counts.cpu().numpy()
    T, nobs = int(ct[0]), int(ct[1])
    rounds_run = int(st[1]) + 1

    t_edges = timed(lambda: tracks.match_edges(store, nqd, prd, img_off, out=edges))
    t_comp = timed(lambda: tracks.track_components(edges, n))
    t_build = timed(lambda: tracks.build_tracks(labels, img_off))
    t_tri = timed(lambda: tracks.triangulate_tracks(counts, track_off, obs_node, img_off, kp, Pd, out=tri))
    wall = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = tracks.run_tracks(store, nq, pairs, kps, P, max_reproj=2.0)
        wall.append(time.perf_counter() - t0)

    # lowering rounds over the pair lists the benchmarks drive: all pairs, the consecutive pairs alone, all pairs of the first 8 images
    rounds_table = {}
    for name, rows in (("all_pairs", list(range(n_pairs))), ("sequential_pairs", [p for p, (j, i) in enumerate(pairs) if i == j + 1]),
                       ("all_pairs_first_8_images", [p for p, (j, i) in enumerate(pairs) if i < 8])):
        idx = torch.tensor(rows, dtype=torch.long, device=dev)
        sub = tracks.match_edges(store[idx].contiguous(), nqd[idx].contiguous(), prd[idx].contiguous(), img_off)
        lab, stt = tracks.track_components(sub, n, rounds=64)
        cnt = tracks.build_tracks(lab, img_off)[3]
        rounds_table[name] = {"pairs": len(rows), "converged": int(stt[0]), "rounds_that_lowered_a_label": int(stt[1]),
                              "tracks": int(cnt[0]), "conflicting": int(cnt[3]), "longest": int(cnt[4])}

    e_host = edges.cpu().numpy()
    valid = e_host[e_host[:, 0] >= 0]
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    t0 = time.perf_counter()
    ncomp, _ = connected_components(coo_matrix((np.ones(len(valid), np.int8), (valid[:, 0], valid[:, 1])), shape=(n, n)), directed=False)
    t_scipy = time.perf_counter() - t0

    # purity against the planted ids, as the calibration tests measure it
    off_h, obs_h = track_off[:T + 1].cpu().numpy(), obs_node[:nobs].cpu().numpy()
    tr = np.repeat(np.arange(T), np.diff(off_h))
    lo, hi = np.full(T, np.iinfo(np.int64).max), np.full(T, -2)
    np.minimum.at(lo, tr, ids[obs_h]); np.maximum.at(hi, tr, ids[obs_h])
    floors = {"match_edges": (store.numel() * 4 + ne * 8 + ne // 8) / HBM_BYTES_PER_S * 1e3,
              "track_components": rounds_run * (ne * 8 + 2 * n * 4) / HBM_BYTES_PER_S * 1e3,
              "build_tracks": (n * 4 * 6) / HBM_BYTES_PER_S * 1e3,
              "triangulate_tracks": (nobs * (4 + 8 + 8) + T * (12 + 8 + 8)) / HBM_BYTES_PER_S * 1e3}
    res = {"workload": f"tracks on the all-pairs ring scene: {n_img} images x {n_desc}, {n_pairs} pairs, N = {n}, {ne} edge slots, {len(valid)} valid edges",
           "ms_median_min": {"match_edges": t_edges, "track_components": t_comp, "build_tracks": t_build, "triangulate_tracks": t_tri},
           "ms_byte_floor_at_6.3TBps": floors,
           "rounds_default": tracks.TRACK_ROUNDS, "rounds_that_lowered_a_label": int(st[1]), "converged": int(st[0]), "rounds_table": rounds_table,
           "scipy_connected_components_s": t_scipy, "scipy_components": int(ncomp),
           "counts": ct.tolist(), "length_histogram": np.bincount(np.diff(off_h), minlength=n_img + 1).tolist(),
           "pure_tracks": int(((lo == hi) & (lo >= 0)).sum()), "points_kept_at_2px": int(len(out["points"])),
           "run_tracks_wall_s_median": float(np.median(wall)), "run_tracks_wall_s_min": float(min(wall)),
           "build_id_tracks": _lib.code_hashes_of_binary().get("tracks.hip")}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
