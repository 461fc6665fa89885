"""Integer NumPy restatement of the cost-volume aggregation (include/sfm_hip.h, "MVS-AGGREGATE"; docs/mvs.md §7), written from
the header: sfm_mvs_cost_shift, sfm_mvs_cost_aggregate, sfm_mvs_cost_depth.  Only the quantisation and the parabola are float32
(every constant a np.float32); the rest is int64 arithmetic, vectorised over the planes and one image axis and looping along
the paths.  The bit-for-bit checker of the three entry points and the CPU model of the stage (tests/test_mvs_aggregate_cpu.py).
Imports nothing of the product."""
import numpy as np

F = np.float32
QMAX = 2048
DIRECTIONS = [(1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, 1), (1, -1), (-1, -1)]


def quantise(c):
    """q(c) = !(c < 2) ? 2048 : c > 0 ? floorf(c*1024 + 0.5) : 0 (float32 product and sum) -> int64."""
    c = np.asarray(c, F)
    with np.errstate(invalid="ignore", over="ignore"):
        below = c < F(2)                                    # False for a NaN
        pos = c > F(0)
        r = np.floor(np.where(below & pos, c, F(0)) * F(1024) + F(0.5))
    return np.where(~below, QMAX, np.where(pos, r.astype(np.int64), 0)).astype(np.int64)


def min_filter(a, shift):
    """Minimum over the taps |dx|, |dy| <= shift that lie in the frame, per plane: a [nd, h, w] integers."""
    nd, h, w = a.shape
    out = a.copy()
    for dy in range(-shift, shift + 1):
        for dx in range(-shift, shift + 1):
            ys, ye = max(0, -dy), min(h, h - dy)            # destination rows y with 0 <= y + dy < h
            xs, xe = max(0, -dx), min(w, w - dx)
            if ys >= ye or xs >= xe:
                continue
            np.minimum(out[:, ys:ye, xs:xe], a[:, ys + dy:ye + dy, xs + dx:xe + dx], out=out[:, ys:ye, xs:xe])
    return out


def cost_shift(volume, shift):
    """sfm_mvs_cost_shift: float32 [nd, h, w] -> uint16 [nd, h, w]."""
    assert 0 <= shift <= 4
    return min_filter(quantise(volume), int(shift)).astype(np.uint16)


def _step(q, prev, p1, p2):
    """L(p, .) from L(p', .): q, prev [nd, n] int64."""
    m = prev.min(axis=0, keepdims=True)
    best = np.minimum(prev, m + p2)
    best[1:] = np.minimum(best[1:], prev[:-1] + p1)
    best[:-1] = np.minimum(best[:-1], prev[1:] + p1)
    return q + best - m


def path_costs(Q, dx, dy, p1, p2):
    """L_r of one direction: Q [nd, h, w] integers -> int64 [nd, h, w]."""
    Q = np.asarray(Q).astype(np.int64)
    nd, h, w = Q.shape
    L = np.empty_like(Q)
    if dy == 0:                                             # along a row: columns in the order of the path
        xs = range(w) if dx > 0 else range(w - 1, -1, -1)
        for n, x in enumerate(xs):
            L[:, :, x] = Q[:, :, x] if n == 0 else _step(Q[:, :, x], L[:, :, x - dx], p1, p2)
        return L
    ys = range(h) if dy > 0 else range(h - 1, -1, -1)
    for n, y in enumerate(ys):
        L[:, y, :] = Q[:, y, :]
        if n == 0:
            continue
        # the pixels x whose predecessor x - dx lies in the frame
        lo, hi = max(0, dx), min(w, w + dx)
        if lo < hi:
            L[:, y, lo:hi] = _step(Q[:, y, lo:hi], L[:, y - dy, lo - dx:hi - dx], p1, p2)
    return L


def cost_aggregate(Q, p1, p2, ndir):
    """sfm_mvs_cost_aggregate: uint16 [nd, h, w] -> uint16 [nd, h, w] (the sum modulo 65536)."""
    assert ndir in (4, 8) and 0 <= p1 <= p2 <= QMAX
    S = np.zeros(np.asarray(Q).shape, np.int64)
    for dx, dy in DIRECTIONS[:ndir]:
        S += path_costs(Q, dx, dy, int(p1), int(p2))
    return (S & 0xFFFF).astype(np.uint16)


def cost_depth(S, Q, invd, gate):
    """sfm_mvs_cost_depth -> (depth [h, w] f32, cost [h, w] f32, plane [h, w] int32)."""
    S = np.asarray(S).astype(np.int64)
    Q = np.asarray(Q).astype(np.int64)
    invd = np.asarray(invd, F)
    nd = S.shape[0]
    jstar = np.argmin(S, axis=0)                            # the first index of the minimum
    mid = (jstar > 0) & (jstar < nd - 1)
    jm, jp = np.clip(jstar - 1, 0, nd - 1), np.clip(jstar + 1, 0, nd - 1)
    a = np.take_along_axis(S, jm[None], 0)[0].astype(F)
    b = np.take_along_axis(S, jstar[None], 0)[0].astype(F)
    c = np.take_along_axis(S, jp[None], 0)[0].astype(F)
    den = (a + c) - F(2) * b
    ok = mid & (den > F(0))
    delta = np.where(ok, np.clip(F(0.5) * (a - c) / np.where(ok, den, F(1)), F(-0.5), F(0.5)), F(0)).astype(F)
    step = np.where(delta >= F(0), invd[jp] - invd[jstar], invd[jstar] - invd[jm]).astype(F)
    inv = np.where(mid, invd[jstar] + delta * step, invd[jstar]).astype(F)
    q = np.take_along_axis(Q, jstar[None], 0)[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        depth = np.where(q >= int(gate), F(0), F(1) / inv).astype(F)
    cost = (q.astype(F) / F(1024)).astype(F)
    return depth, cost, jstar.astype(np.int32)


def gate_of(cost_max):
    """q(cost_max): what the wrapper passes as `gate`."""
    return int(quantise(F(cost_max)))


def aggregate_depth(volume, invd, shift, p1, p2, ndir, cost_max):
    Q = cost_shift(volume, shift)
    S = cost_aggregate(Q, p1, p2, ndir)
    return cost_depth(S, Q, invd, gate_of(cost_max))
