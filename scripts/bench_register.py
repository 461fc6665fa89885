"""Times the TRACKS-REGISTER family on the bench scene of docs/tracks.md §5 (64 images x 10 000 features, 2 016 pairs, 7 000 tracks of 64
observations) and writes one JSON line (default: profiles/tracks_register_bench.json).

  python scripts/bench_register.py [--images 64] [--out PATH] [--once]

In one process, with half of the images registered: `restrict_tracks`, `adopt_points`, `view_scores` and `correspondences`, each with HIP
events on the current stream, the median of 10 calls after 3 warm-ups, beside its byte floor at 6.3 TB/s (every word the call must read
and write once) and beside the same step written with torch alone (bucketize, masks, nonzero, index_select), the two ALTERNATING call by
call, the yardstick's host waits counted under torch's sync debug mode.  Then `register_tracks` on the whole scene: the wall time, its
split into model rounds, PnP, bundle adjustment and the rest of the host, the host reads per registered image, the final median
camera-centre error against the planted cameras.
--once runs every entry point and one model round once and leaves (for a kernel trace collected in a run of its own)."""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "scripts"))

HBM_BYTES_PER_S = 6.3e12


def alternating(fn_a, fn_b, warm=3, reps=10):
    """(median, min) ms of fn_a and of fn_b by HIP events, the two alternating call by call."""
    import torch
    ms = ([], [])
    for rep in range(warm + reps):
        for k, fn in enumerate((fn_a, fn_b)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if rep >= warm:
                ms[k].append(a.elapsed_time(b))
    return [(float(np.median(m)), float(min(m))) for m in ms]


def host_waits(fn):
    import torch
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    return len([w for w in caught if "synchroniz" in str(w.message).lower()])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracks_register_bench.json"))
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    import torch
    from datagen import ring_scene
    from register_cases import FRAME, centre_errors
    from sfm_mvs_amd import _lib, register, sharded, tracks
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
    labels, _ = tracks.track_components(tracks.match_edges(store, nqd, prd, img_off), n)
    node_track, track_off, obs_node, counts = tracks.build_tracks(labels, img_off)
    reg_h = (np.arange(n_img) % 2 == 0).astype(np.uint8)                       # every other image registered
    reg = torch.from_numpy(reg_h).to(dev)
    P_half = torch.from_numpy(np.where(reg_h[:, None, None] != 0, P, 0.0).reshape(n_img, 12)).to(dev)
    target = 1                                                               # an unregistered image

    def model_round():
        r = register.restrict_tracks(counts, track_off, obs_node, img_off, reg)
        tri = tracks.triangulate_tracks(r[3], r[0], r[1], img_off, kp, P_half)
        rf = tracks.refine_tracks(r[3], r[0], r[1], img_off, kp, P_half, tri[0], tri[3])
        p = tracks.prune_tracks(r[3], r[0], r[1], rf[0], rf[1], rf[4], rf[5], rf[6], rf[8], 2, 2.0, 2.0)
        a = register.adopt_points(counts, track_off, obs_node, r, p)
        s = register.view_scores(counts, node_track, a[1], img_off, kp, FRAME, 8)
        return r, p, a, s

    r, p, a, s = model_round()
    c = register.correspondences(target, counts, node_track, a[1], a[0], img_off, kp, capacity=n_desc)
    torch.cuda.synchronize()
    if args.once:
        print("bench_register: one pass done")
        return 0
    ct, cr, cp = counts.cpu().numpy(), r[3].cpu().numpy(), p[4].cpu().numpy()
    T, nobs, Tr, nobs_r, Tp, nobs_p = int(ct[0]), int(ct[1]), int(cr[0]), int(cr[1]), int(cp[0]), int(cp[1])
    k = int(c[3].item())

    # ---- the same steps with torch alone: sizes known on the host (T, nobs), every data-dependent size costs a wait ----
    obs_track = torch.searchsorted(track_off[1:T + 1].contiguous(), torch.arange(nobs, dtype=torch.int32, device=dev), right=True)
    bounds = img_off[1:].contiguous()

    def torch_restrict():
        nodes = obs_node[:nobs]
        live = reg[torch.bucketize(nodes, bounds, right=True)] != 0
        n_live = torch.zeros(T, dtype=torch.int64, device=dev).index_add_(0, obs_track, live.long())
        kept = n_live >= 2
        src = torch.nonzero(kept).reshape(-1)
        obs2 = nodes[kept[obs_track] & live]
        off2 = torch.cumsum(n_live[src], 0)
        return src, obs2, off2

    def torch_adopt():
        t_p, n_p = (int(v) for v in p[4][:2].cpu())                          # the sizes live on the device
        src = r[2].index_select(0, p[3][:t_p].long()).long()
        has = torch.zeros(n // 2 + 1, dtype=torch.uint8, device=dev)
        has[src] = 1
        X_full = torch.full((n // 2 + 1, 3), float("nan"), dtype=torch.float32, device=dev)
        X_full[src] = p[2][:t_p]
        node_live = torch.zeros(n, dtype=torch.uint8, device=dev)
        node_live[p[1][:n_p].long()] = 1
        return X_full, has, node_live[obs_node[:nobs].long()]

    node_img = torch.bucketize(torch.arange(n, dtype=torch.int32, device=dev), bounds, right=True)

    def torch_scores():
        t = node_track.long()
        has = (t >= 0) & (a[1][t.clamp(min=0)] != 0)
        seen = torch.zeros(n_img, dtype=torch.int64, device=dev).index_add_(0, node_img, has.long())
        cx = (kp[:, 0] * (8.0 / FRAME[0])).clamp(0, 7).long()
        cy = (kp[:, 1] * (8.0 / FRAME[1])).clamp(0, 7).long()
        table = torch.zeros(n_img * 64, dtype=torch.int64, device=dev).index_add_(0, node_img * 64 + cy * 8 + cx, has.long())
        return seen, (table.view(n_img, 64) > 0).sum(1)

    def torch_corr():
        lo, hi = target * n_desc, (target + 1) * n_desc
        t = node_track[lo:hi].long()
        idx = torch.nonzero((t >= 0) & (a[1][t.clamp(min=0)] != 0)).reshape(-1)
        tt = t[idx]
        return a[0].index_select(0, tt), kp[lo:hi].index_select(0, idx), tt

    out_r, out_a, out_s = r, a, s
    pairs_of = {
        "restrict_tracks": (lambda: register.restrict_tracks(counts, track_off, obs_node, img_off, reg, out=out_r), torch_restrict,
                            4 * (T + 1) + 4 * nobs + n_img + 4 * (n_img + 1) + 4 * (Tr + 1) + 4 * nobs_r + 4 * Tr + 16),
        "adopt_points": (lambda: register.adopt_points(counts, track_off, obs_node, r, p, out=out_a), torch_adopt,
                         4 * Tp + 4 * Tr + 12 * Tp + 4 * (Tp + 1) + 4 * nobs_p + 4 * (T + 1) + 4 * nobs + 13 * T + nobs),
        "view_scores": (lambda: register.view_scores(counts, node_track, a[1], img_off, kp, FRAME, 8, out=out_s), torch_scores,
                        4 * n + T + 8 * n + 4 * (n_img + 1) + 16 * n_img),
        "correspondences": (lambda: register.correspondences(target, counts, node_track, a[1], a[0], img_off, kp, capacity=n_desc, out=c), torch_corr,
                            4 * n_desc + k * (1 + 12 + 8) + k * 24 + 4),
    }
    entry = {}
    for name, (hip_fn, torch_fn, nbytes) in pairs_of.items():
        (hm, hmin), (tm, tmin) = alternating(hip_fn, torch_fn)
        floor = nbytes / HBM_BYTES_PER_S * 1e3
        entry[name] = {"ms_median": hm, "ms_min": hmin, "bytes": int(nbytes), "byte_floor_ms": floor, "over_floor": hm / floor,
                       "torch_ms_median": tm, "torch_ms_min": tmin, "torch_over_hip": tm / hm, "hip_host_waits": host_waits(hip_fn),
                       "torch_host_waits": host_waits(torch_fn)}
    t_round = alternating(lambda: model_round(), lambda: None)[0]

    # ---- the loop: wall time and where it goes (every engine call below ends synchronised or with a host read of its own) ----
    class Timed(register._HipEngine):
        spent = {"tracks": 0.0, "rounds": 0.0, "pnp": 0.0, "ba": 0.0, "seed_solvers": 0.0}
        calls = {"rounds": 0, "pnp": 0, "ba": 0}

        def _t(self, key, fn, *a_, **kw):
            t0 = time.perf_counter()
            out = fn(*a_, **kw)
            self.spent[key] += time.perf_counter() - t0
            if key in self.calls:
                self.calls[key] += 1
            return out

        def tracks(self):
            return self._t("tracks", super().tracks)

        def round(self, *a_):
            return self._t("rounds", super().round, *a_)

        def pnp(self, *a_, **kw):
            return self._t("pnp", super().pnp, *a_, **kw)

        def bundle(self, *a_, **kw):
            return self._t("ba", super().bundle, *a_, **kw)

        def relative_pose(self, *a_):
            return self._t("seed_solvers", super().relative_pose, *a_)

    runs = []
    for rep in range(3):
        Timed.spent = {key: 0.0 for key in Timed.spent}
        Timed.calls = {key: 0 for key in Timed.calls}
        eng = Timed(store, nq, pairs, kps, K, FRAME, 0.70, None, 2, None, 1.0, 2.0, 2.0, 2.0, 10, 8)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = register.register_loop(eng, n_img, pairs, K)
        wall = time.perf_counter() - t0
        order = out["order"]
        runs.append({"wall_s": wall, **{f"{key}_s": v for key, v in Timed.spent.items()}, "host_rest_s": wall - sum(Timed.spent.values()),
                     **{f"{key}_calls": v for key, v in Timed.calls.items()}, "registered": int(out["registered"].sum()), "points": int(len(out["points"])),
                     "model_round_reads_per_registered_image": out["rounds"] / max(int(out["registered"].sum()), 1),
                     "median_centre_error": float(np.median(centre_errors(out["P"][order], P[order]))),
                     "ba_final_cost": float(out["ba_history"][-1][-1]), "ba_runs": len(out["ba_history"])})
    res = {"workload": f"incremental registration on the all-pairs ring scene: {n_img} images x {n_desc}, N = {n}, {T} tracks, {nobs} observations; "
                       f"entry points with every other image registered ({Tr} restricted tracks, {nobs_r} observations, {Tp} points, image {target}: {k} rows)",
           "entry_points": entry, "model_round_ms_median_min": t_round, "register_tracks": runs[1:], "register_tracks_first_call": runs[0],
           "build_id_tracks_register": _lib.code_hashes_of_binary().get("tracks_register.hip")}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
