"""Float32 NumPy restatement of the PatchMatch refinement (include/sfm_hip.h, "MVS-PATCHMATCH"; docs/mvs.md §9), written from the
header: every constant a np.float32 so that every operation is a correctly rounded float32 one, in the header's order.  A half-sweep
is one vectorised pass over the pixels of one colour (they read the other colour's planes only).  The checker of sfm_mvs_patchmatch
bit for bit and the CPU model of the algorithm (tests/test_mvs_patchmatch_cpu.py).  Imports nothing of the product."""
import numpy as np

import np_mvs
from np_mvs import F, HALF, ONE, TWO, ZERO

NEIGHBOURS = ((-1, 0), (1, 0), (0, -1), (0, 1), (-3, 0), (3, 0), (0, -3), (0, 3))
M32 = 0xFFFFFFFF


def hash_u(seed, pix, it, c):
    """U(pix, it, c) of the header for a uint32 array `pix` -> float32 in [-1, 1]."""
    pix = np.asarray(pix, np.uint32)
    k = np.uint32((int(it) * 0x85EBCA6B + int(c) * 0xC2B2AE35) & M32)
    x = np.uint32(int(seed) & M32) ^ (pix * np.uint32(0x9E3779B9) + k)
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x7FEB352D)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x846CA68B)
    x = x ^ (x >> np.uint32(16))
    return x.view(np.int32).astype(F) * F(2.0 ** -31)


class Frame:
    """What does not depend on the plane: I' of every frame, the reference moments, and where a cost other than 2 can arise."""

    def __init__(self, ref, srcs, mvs, radius, topk, var_min):
        self.h, self.w = ref.shape
        self.r, self.topk, self.var_min = int(radius), int(topk), F(var_min)
        self.n = F((2 * self.r + 1) ** 2)
        self.R = ref.astype(F) - F(128)
        self.I = [s.astype(F) - F(128) for s in srcs]
        self.mvs = np.asarray(mvs, F).reshape(len(srcs), 12)
        r, h, w = self.r, self.h, self.w
        self.ref_in = np.zeros((h, w), bool)
        self.ref_in[r:h - r, r:w - r] = True
        self.s_r = np.zeros((h, w), F)
        self.var_r = np.zeros((h, w), F)
        s_r = np_mvs.window_sum(self.R, r)
        s_rr = np_mvs.window_sum(self.R * self.R, r)
        self.s_r[r:h - r, r:w - r] = s_r
        self.var_r[r:h - r, r:w - r] = s_rr - (s_r * s_r) / self.n
        self.live = self.ref_in & ~(self.var_r < self.var_min)      # elsewhere C = 2 under every plane


def plane_cost(fr, ys, xs, q0, a, b):
    """C(x, y; q0, a, b) for the live pixels (ys, xs) -> float32 [N]."""
    r, w, h = fr.r, fr.w, fr.h
    d = 2 * r + 1
    off = np.arange(-r, r + 1)
    du, dv = off.astype(F)[None, :, None], off.astype(F)[:, None, None]          # [i (rows), j (columns), pixel]
    q = (q0[None, None, :] + a[None, None, :] * du) + b[None, None, :] * dv
    u = (xs[None, None, :] + off[None, :, None]).astype(F) + np.zeros((d, 1, 1), F)
    v = (ys[None, None, :] + off[:, None, None]).astype(F) + np.zeros((1, d, 1), F)
    Rw = fr.R[ys[None, None, :] + off[:, None, None], xs[None, None, :] + off[None, :, None]]
    s_r, var_r = fr.s_r[ys, xs], fr.var_r[ys, xs]
    costs = np.empty((len(fr.I), len(ys)), F)
    for s, (I, m) in enumerate(zip(fr.I, fr.mvs)):
        hh = [((m[3 * i] * u + m[3 * i + 1] * v) + m[3 * i + 2]) + m[9 + i] * q for i in range(3)]
        pos = hh[2] > ZERO
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            den = np.where(pos, hh[2], ONE)
            px, py = hh[0] / den, hh[1] / den
        valid = pos & (px >= ZERO) & (px <= F(w - 1)) & (py >= ZERO) & (py <= F(h - 1))
        px, py = np.where(valid, px, ZERO), np.where(valid, py, ZERO)
        x0 = np.minimum(np.floor(px).astype(np.int64), w - 2)
        y0 = np.minimum(np.floor(py).astype(np.int64), h - 2)
        ax, ay = px - x0.astype(F), py - y0.astype(F)
        val = (ONE - ay) * ((ONE - ax) * I[y0, x0] + ax * I[y0, x0 + 1]) + ay * ((ONE - ax) * I[y0 + 1, x0] + ax * I[y0 + 1, x0 + 1])
        val = np.where(valid, val, ZERO).astype(F)

        def wsum(t):                                            # row sums left to right, then the row sums top to bottom
            rows = t[:, 0]
            for j in range(1, d):
                rows = rows + t[:, j]
            tot = rows[0]
            for i in range(1, d):
                tot = tot + rows[i]
            return tot
        s_w, s_ww, s_rw = wsum(val), wsum(val * val), wsum(Rw * val)
        var_w = s_ww - (s_w * s_w) / fr.n
        ok = valid.all(axis=(0, 1)) & ~(var_w < fr.var_min)
        cov = s_rw - (s_r * s_w) / fr.n
        with np.errstate(divide="ignore", invalid="ignore"):
            c = ONE - cov / np.sqrt(np.where(ok, var_r * var_w, ONE))
        costs[s] = np.where(ok, np.clip(c, ZERO, TWO), TWO)
    costs.sort(axis=0)
    acc = costs[0].copy()
    for k in range(1, fr.topk):
        acc = acc + costs[k]
    return acc / F(fr.topk)


def init_state(fr, qmin, qmax, depth_init, seed):
    """-> state [h, w, 4] float32 (q0, 0, 0, cost)."""
    h, w = fr.h, fr.w
    qmin, qmax = F(qmin), F(qmax)
    pix = np.arange(h * w, dtype=np.uint32).reshape(h, w)
    q0 = qmin + (qmax - qmin) * (HALF * hash_u(seed, pix, 0, 0) + HALF)
    if depth_init is not None:
        d = np.asarray(depth_init, F)
        with np.errstate(divide="ignore", invalid="ignore"):
            qi = ONE / np.where(d > ZERO, d, ONE)
        q0 = np.where((d > ZERO) & (qi >= qmin) & (qi <= qmax), qi, q0)
    state = np.zeros((h, w, 4), F)
    state[..., 0] = q0
    state[..., 3] = TWO
    ys, xs = np.nonzero(fr.live)
    if len(ys):
        z = np.zeros(len(ys), F)
        state[ys, xs, 3] = plane_cost(fr, ys, xs, q0[ys, xs].astype(F), z, z)
    return state


def half_sweep(fr, state, colour, it, qmin, qmax, far, depth_step, slope_step, seed):
    """One half-sweep in place: the live pixels with (x + y) & 1 == colour."""
    qmin, qmax = F(qmin), F(qmax)
    gy, gx = np.mgrid[0:fr.h, 0:fr.w]
    ys, xs = np.nonzero(fr.live & (((gx + gy) & 1) == colour))
    if not len(ys):
        return state
    cur = state[ys, xs].copy()                                  # [N, 4]
    rr = F(fr.r)

    def consider(cq, ca, cb, present):
        with np.errstate(invalid="ignore", over="ignore"):
            adm = present & np.isfinite(cq) & np.isfinite(ca) & np.isfinite(cb) & (cq >= qmin) & (cq <= qmax) \
                & (rr * (np.abs(ca) + np.abs(cb)) <= HALF * cq)
        k = np.nonzero(adm)[0]
        if not len(k):
            return
        c = plane_cost(fr, ys[k], xs[k], cq[k], ca[k], cb[k])
        win = c < cur[k, 3]
        k, c = k[win], c[win]
        cur[k, 0], cur[k, 1], cur[k, 2], cur[k, 3] = cq[k], ca[k], cb[k], c

    everyone = np.ones(len(ys), bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for dx, dy in NEIGHBOURS[:8 if far else 4]:
            xn, yn = xs + dx, ys + dy
            inb = (xn >= 0) & (xn < fr.w) & (yn >= 0) & (yn < fr.h)
            nb = state[np.where(inb, yn, 0), np.where(inb, xn, 0)]
            consider((nb[:, 0] + nb[:, 1] * F(-dx)) + nb[:, 2] * F(-dy), nb[:, 1].copy(), nb[:, 2].copy(), inb)
        s = F(2.0 ** -int(it))
        ds, ss = F(depth_step) * s, F(slope_step) * s
        pix = (ys * fr.w + xs).astype(np.uint32)
        U = [None] + [hash_u(seed, pix, it, c) for c in range(1, 7)]
        consider(cur[:, 0] * (ONE + ds * U[1]), cur[:, 1].copy(), cur[:, 2].copy(), everyone)
        t = ss * cur[:, 0]
        consider(cur[:, 0].copy(), cur[:, 1] + t * U[2], cur[:, 2] + t * U[3], everyone)
        t = ss * cur[:, 0]
        consider(cur[:, 0] * (ONE + ds * U[4]), cur[:, 1] + t * U[5], cur[:, 2] + t * U[6], everyone)
    state[ys, xs] = cur
    return state


def finish(fr, state, cost_max, nmat=None):
    """-> (depth [h, w], cost [h, w], normal [h, w, 3] or None)."""
    q0, a, b, cost = (state[..., k] for k in range(4))
    with np.errstate(divide="ignore", invalid="ignore"):
        depth = np.where(fr.ref_in & (cost < F(cost_max)), ONE / q0, ZERO).astype(F)
    normal = None
    if nmat is not None:
        N = np.asarray(nmat, F).reshape(3, 3)
        gy, gx = np.mgrid[0:fr.h, 0:fr.w]
        C = (q0 - a * gx.astype(F)) - b * gy.astype(F)
        n = [(N[i, 0] * a + N[i, 1] * b) + N[i, 2] * C for i in range(3)]
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            length = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
            normal = np.stack([np.where(depth != ZERO, c / length, ZERO) for c in n], -1).astype(F)
    return depth, cost.copy(), normal


def patchmatch(ref, srcs, mvs, qmin, qmax, radius, topk, var_min, cost_max, depth_init=None, iters=2, far=1, depth_step=0.1, slope_step=0.0,
               seed=0, nmat=None, after=None):
    """sfm_mvs_patchmatch -> (state [h, w, 4], depth, cost, normal or None).  after(it, colour, state), if given, is called after every
    half-sweep (the tests read the intermediate states through it)."""
    fr = Frame(ref, srcs, mvs, radius, topk, var_min)
    state = init_state(fr, qmin, qmax, depth_init, seed)
    for it in range(int(iters)):
        for colour in (0, 1):
            half_sweep(fr, state, colour, it, qmin, qmax, far, depth_step, slope_step, seed)
            if after is not None:
                after(it, colour, state)
    return (state,) + finish(fr, state, cost_max, nmat)
