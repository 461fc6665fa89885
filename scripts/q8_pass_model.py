"""CPU model of the quantised refine's two evaluation loops (refine_q8_body, csrc/knn.hip): how many records a query lists, how
many rows go on to the float32 stage, how often a query rescans, and how many PASSES a wave (four queries, 16 lanes each) runs —
with every query's own lanes walking its own list (trip count: the longest of the four lists) and with the four lists pooled over
the wave's lanes.  No GPU: numpy only.  usage: python scripts/q8_pass_model.py [nq = 1500] [nt = 10000] [seed = 0]

The model follows the kernel: one 8-bit grid per pair (lo, s from sixteen sampled rows per side), D = sum (k_q - k_t)^2, E =
||q - q^|| + max_t ||t - t^|| in units of s, records of eight ADJACENT train rows (rows 16 e + 8 h + r, r = 0 .. 7, of a 32-row tile),
per (substream, half-wave h) the three smallest record keys (key = (min D of the record - cq) >> 1), the selection bound U from the
second smallest key, R and Dlim by the kernel's float32 formulas, records listed up to Dlim, rows evaluated in float32 when
D <= Dlim, a substream certified when its third key's lower bound exceeds the second distance.  base = 0, cq = 0 (they cancel)."""
import sys
import numpy as np

nq = int(sys.argv[1]) if len(sys.argv) > 1 else 1500
nt = int(sys.argv[2]) if len(sys.argv) > 2 else 10000
seed = int(sys.argv[3]) if len(sys.argv) > 3 else 0
rng = np.random.default_rng(seed)
q, t = rng.random((nq, 128), dtype=np.float32), rng.random((nt, 128), dtype=np.float32)

f32 = np.float32
RHO, ETA = f32(4e-6), f32(1e-17)                                 # kQ8Rho, kQ8Eta
sample = np.concatenate([x[[(k * len(x)) >> 4 for k in range(16)]].ravel() for x in (q, t)])
lo, s = f32(sample.min()), f32((sample.max() - sample.min()) / 255.0)
quant = lambda x: np.clip(np.rint((x - lo) / s), 0, 255).astype(np.float32)
kq, kt = quant(q), quant(t)
qerr = np.linalg.norm(q - (lo + s * kq), axis=1).astype(np.float32)
terr = f32(np.linalg.norm(t - (lo + s * kt), axis=1).max())
mabs = max(abs(lo), abs(lo + f32(255) * s))
E = (qerr + terr) * f32(1 + 8e-6) + f32(24 * 5.9604645e-08) * mabs * f32(1 + 1e-6)
e_s = (E / s * f32(1 + 1e-6)).astype(np.float32)
eta_s = f32(ETA / s)

# exact integer D (every partial sum is an integer below 2^24: float32 BLAS is exact)
D = ((kq * kq).sum(1)[:, None] + (kt * kt).sum(1)[None, :] - 2.0 * (kq @ kt.T)).astype(np.int32)
tiles = (nt + 31) // 32
BIG = np.int32(1 << 30)
Dp = np.full((nq, tiles * 32), BIG, np.int32)
Dp[:, :nt] = D
# row of a tile = 16 e + 8 h + r: a record is (tile, e, h)
recmin = Dp.reshape(nq, tiles, 2, 2, 8).min(axis=4)               # [query, tile, e, h]
dist = lambda i, rows: np.sqrt(((q[i][None, :].astype(np.float64) - t[rows].astype(np.float64)) ** 2).sum(1))


def model(L):
    """Lists and certificates with substreams of L tiles.  Returns (records listed, float32 rows, open) per query."""
    nstr = (tiles + L - 1) // L
    pad = np.full((nq, nstr * L, 2, 2), BIG, np.int32)
    pad[:, :tiles] = recmin
    pairs = pad.reshape(nq, nstr, L, 2, 2).transpose(0, 1, 4, 2, 3).reshape(nq, nstr * 2, L * 2)   # [query, (stream, h), (tile, e)]
    tile_of = np.broadcast_to((np.arange(nstr)[:, None, None, None] * L + np.arange(L)[None, None, :, None]), (nstr, 2, L, 2)).reshape(nstr * 2, L * 2)
    e_of = np.broadcast_to(np.arange(2)[None, None, None, :], (nstr, 2, L, 2)).reshape(nstr * 2, L * 2)
    h_of = np.broadcast_to(np.arange(2)[None, :, None, None], (nstr, 2, L, 2)).reshape(nstr * 2, L * 2)
    top = np.argsort(pairs, axis=2, kind="stable")[:, :, :3]     # the three smallest record keys of every pair
    nrec, nrow, opened = np.zeros(nq, int), np.zeros(nq, int), np.zeros(nq, bool)
    for i in range(nq):
        keys = np.take_along_axis(pairs[i], top[i], axis=1)      # [pair, 3] min D of the kept records
        acc = keys >> 1
        flat = np.sort(acc[keys < BIG])
        e, dlim, al = e_s[i], np.iinfo(np.int32).max, None
        if len(flat) >= 2:
            U = f32(2 * int(flat[1]) + 1)
            R = (np.sqrt(U) * f32(1 + 2e-7) + e) * (f32(1) + RHO) + eta_s
            r = (R + eta_s) * (f32(1) + f32(2) * RHO) + e
            dl = r * r * f32(1 + 1e-6) + f32(2)
            if dl < 1.6e7:
                dlim = int(dl)
                al = max((dlim >> 1) + 1, int(flat[1]))
        listed = (keys < BIG) & ((acc <= al) if al is not None else True)
        nrec[i] = listed.sum()
        pi, ki = np.nonzero(listed)
        col = top[i][pi, ki]
        tl, ee, hh = tile_of[pi, col], e_of[pi, col], h_of[pi, col]
        rows = (tl[:, None] * 32 + 16 * ee[:, None] + 8 * hh[:, None] + np.arange(8)[None, :]).ravel()
        rows = rows[rows < nt]
        rows = rows[D[i, rows] <= dlim]
        nrow[i] = len(rows)
        d2 = np.sort(dist(i, rows))[1] if len(rows) >= 2 else np.inf
        k3 = keys[:, 2]
        full = k3 < BIG
        lowb = (np.sqrt((2 * (k3[full] >> 1)).astype(np.float32)) * f32(1 - 2e-7) - e) * (f32(1) - RHO) - eta_s
        opened[i] = bool((lowb <= f32(d2 / s) * f32(1 + 1e-6)).any())
    return nrec, nrow, opened


def passes(n, per_query, slots):
    """Wave passes over lists of n[query] entries: per_query entries of each of the four queries a pass (per-query lists) against `slots`
    entries of the pooled list a pass."""
    w = n[: len(n) // 4 * 4].reshape(-1, 4)
    own = -(-w.max(1) // per_query)
    pooled = -(-w.sum(1) // slots)
    return own.mean(), w.sum() / max((own * slots).sum(), 1), pooled.mean()


print(f"q8 pass model: {nq} queries x {nt} trains, uniform float32, seed {seed}; grid lo {lo:.6f} s {s:.6f}; e = E / s: mean {e_s.mean():.2f} max {e_s.max():.2f}")
rates = {}
for L in (128, 64, 32, 16):
    nrec, nrow, opened = model(L)
    rates[L] = 100.0 * opened.mean()
    if L == 32:
        print(f"substreams of 32 tiles (the kernel's): records listed per query {nrec.mean():.2f} (p95 {int(np.percentile(nrec, 95))}, max {nrec.max()}), "
              f"float32 rows per query {nrow.mean():.2f} (max {nrow.max()})")
        a, u, b = passes(nrec, 2, 8)
        print(f"integer rows (8 records a pass): passes per wave with per-query lists {a:.2f}, lane slots used {100 * u:.0f} %, pooled {b:.2f}")
        a, u, b = passes(nrow, 4, 16)
        print(f"float32 rows (16 rows a pass):   passes per wave with per-query lists {a:.2f}, lane slots used {100 * u:.0f} %, pooled {b:.2f}")
print("rescan rate at 128 / 64 / 32 / 16-tile substreams (% of queries): " + " / ".join(f"{rates[L]:.2f}" for L in (128, 64, 32, 16)))
