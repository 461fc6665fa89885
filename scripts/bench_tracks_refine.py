"""Times the TRACKS-REFINE family on the bench scene of docs/tracks.md §5 (64 images x 10 000 features, 2 016 pairs, 7 000 tracks of 64
observations) and writes one JSON line (default: profiles/tracks_refine_bench.json).

  python scripts/bench_tracks_refine.py [--images 64] [--out PATH] [--once]

In one process: `triangulate_tracks` (the yardstick), `refine_tracks` at its defaults and `prune_tracks`, each with HIP events on the
current stream, the median of 10 calls after 3 warm-ups; refine also with one keypoint of a quarter of the tracks displaced by 20 to
100 px, and with iters = iters2 = 0 (the passes every call makes); the wall time of run_tracks with and without robust=True, the two
alternating, seven timed calls each after one untimed.
--once runs every entry point once and leaves (for a kernel trace collected in a run of its own)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bench_tracks import timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracks_refine_bench.json"))
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
    pairs = sharded.all_pairs(n_img)
    store, nq = sharded.match_pairs_sharded(des, pairs, batch=8)
    store = store.contiguous()
    del des
    img_off, kp, nqd, prd, Pd, n = tracks._scene_tensors(nq, pairs, kps, P, dev)
    edges = tracks.match_edges(store, nqd, prd, img_off)
    labels, status = tracks.track_components(edges, n)
    node_track, track_off, obs_node, counts = tracks.build_tracks(labels, img_off)
    del edges

    def chain(kp_, **kw):
        tri = tracks.triangulate_tracks(counts, track_off, obs_node, img_off, kp_, Pd)
        ref = tracks.refine_tracks(counts, track_off, obs_node, img_off, kp_, Pd, tri[0], tri[3], **kw)
        return tri, ref, tracks.prune_tracks(counts, track_off, obs_node, ref[0], ref[1], ref[4], ref[5], ref[6], ref[8], 2, 2.0)

    tri, ref, pruned = chain(kp)
    torch.cuda.synchronize()
    if args.once:
        print("bench_tracks_refine: one pass done")
        return 0
    ct = counts.cpu().numpy()
    T, nobs = int(ct[0]), int(ct[1])
    # one keypoint of a quarter of the tracks displaced by 20 to 100 px, the rule of the calibration
    rng = np.random.default_rng(7)
    off_h, obs_h = track_off[:T + 1].cpu().numpy().astype(np.int64), obs_node[:nobs].cpu().numpy()
    bad = np.flatnonzero(rng.random(T) < 0.25)
    rows = off_h[bad] + rng.integers(0, np.diff(off_h)[bad])
    mag, ang = rng.uniform(20.0, 100.0, len(bad)), rng.uniform(0.0, 2.0 * np.pi, len(bad))
    kp_h = kp.cpu().numpy()
    kp_h[obs_h[rows]] += np.stack([mag * np.cos(ang), mag * np.sin(ang)], 1).astype(np.float32)
    kp_bad = torch.from_numpy(kp_h).to(dev)
    tri_b, ref_b, pruned_b = chain(kp_bad)

    t_tri = timed(lambda: tracks.triangulate_tracks(counts, track_off, obs_node, img_off, kp, Pd, out=tri))
    t_ref = timed(lambda: tracks.refine_tracks(counts, track_off, obs_node, img_off, kp, Pd, tri[0], tri[3], out=ref))
    t_ref_b = timed(lambda: tracks.refine_tracks(counts, track_off, obs_node, img_off, kp_bad, Pd, tri_b[0], tri_b[3], out=ref_b))
    zero = chain(kp, iters=0, iters2=0)[1]
    t_ref_0 = timed(lambda: tracks.refine_tracks(counts, track_off, obs_node, img_off, kp, Pd, tri[0], tri[3], iters=0, iters2=0, out=zero))
    t_prune = timed(lambda: tracks.prune_tracks(counts, track_off, obs_node, ref_b[0], ref_b[1], ref_b[4], ref_b[5], ref_b[6], ref_b[8], 2, 2.0, out=pruned_b))
    # the two variants ALTERNATE after one untimed call of each (the first call of a process pays for the pinned host pool)
    variants = (("plain", dict()), ("robust", dict(robust=True)))
    wall, points = {name: [] for name, _ in variants}, {}
    for rep in range(8):
        for name, kw in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = tracks.run_tracks(store, nq, pairs, kps, P, max_reproj=2.0, **kw)
            if rep:
                wall[name].append(time.perf_counter() - t0)
            points[name] = int(len(out["points"]))
    walls = {name: {"wall_s_median": float(np.median(w)), "wall_s_min": float(min(w)), "wall_s_all": [round(v, 6) for v in w], "points": points[name]}
             for name, w in wall.items()}
    steps, steps_b = ref[7][:T].cpu().numpy(), ref_b[7][:T].cpu().numpy()
    c2, c2b = pruned[4].cpu().numpy(), pruned_b[4].cpu().numpy()
    res = {"workload": f"track refinement on the all-pairs ring scene: {n_img} images x {n_desc}, N = {n}, {T} tracks, {nobs} observations",
           "ms_median_min": {"triangulate_tracks": t_tri, "refine_tracks": t_ref, "refine_tracks_displaced": t_ref_b, "refine_tracks_no_attempt": t_ref_0,
                             "prune_tracks": t_prune},
           "refine_over_triangulate": t_ref[0] / t_tri[0], "refine_displaced_over_triangulate": t_ref_b[0] / t_tri[0],
           "prune_over_triangulate": t_prune[0] / t_tri[0],
           "accepted_steps_mean_max": [float(steps.mean()), int(steps.max())], "accepted_steps_displaced_mean_max": [float(steps_b.mean()), int(steps_b.max())],
           "counts2": c2.tolist(), "counts2_displaced": c2b.tolist(), "displaced_tracks": int(len(bad)), "run_tracks": walls,
           "build_id_tracks_refine": _lib.code_hashes_of_binary().get("tracks_refine.hip")}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
