"""Float32 NumPy restatement of the plane-sweep MVS arithmetic (include/sfm_hip.h, "MVS"; docs/mvs.md §2), written from the
specification: vectorised over pixels, looping over planes, sources and window offsets in the specified order, every constant a
np.float32 so that every operation is a correctly rounded float32 one.  The checker of sfm_mvs_plane_sweep /
sfm_mvs_consistency bit for bit, and the CPU model of the algorithm (tests/test_mvs_cpu.py).  Imports nothing of the product."""
import numpy as np

F = np.float32
ONE, ZERO, TWO, HALF = F(1), F(0), F(2), F(0.5)


def _grid(w, h):
    ys, xs = np.mgrid[0:h, 0:w]
    return xs.astype(F), ys.astype(F)


def warp(src, mv, invd, w, h):
    """Warped source I' at every integer pixel of the reference frame for inverse depth `invd` -> (val [h, w] f32, valid bool)."""
    m = np.asarray(mv, F)
    fx, fy = _grid(w, h)
    a = [(m[3 * i] * fx + m[3 * i + 1] * fy) + m[3 * i + 2] for i in range(3)]
    hh = [a[i] + m[9 + i] * F(invd) for i in range(3)]
    pos = hh[2] > ZERO
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        den = np.where(pos, hh[2], ONE)
        px, py = hh[0] / den, hh[1] / den
    valid = pos & (px >= ZERO) & (px <= F(w - 1)) & (py >= ZERO) & (py <= F(h - 1))
    px, py = np.where(valid, px, ZERO), np.where(valid, py, ZERO)
    x0 = np.minimum(np.floor(px).astype(np.int64), w - 2)
    y0 = np.minimum(np.floor(py).astype(np.int64), h - 2)
    ax, ay = px - x0.astype(F), py - y0.astype(F)
    I = src.astype(F) - F(128)
    i00, i01, i10, i11 = I[y0, x0], I[y0, x0 + 1], I[y0 + 1, x0], I[y0 + 1, x0 + 1]
    val = (ONE - ay) * ((ONE - ax) * i00 + ax * i01) + ay * ((ONE - ax) * i10 + ax * i11)
    return np.where(valid, val, ZERO).astype(F), valid


def window_sum(img, r):
    """Window sum of img about every pixel whose window lies in the frame ([h-2r, w-2r]): row sums of 2r+1 terms left to right,
    then the row sums top to bottom."""
    h, w = img.shape
    d = 2 * r + 1
    tot = None
    for dy in range(d):
        row = img[dy:dy + h - 2 * r, 0:w - 2 * r].copy()
        for dx in range(1, d):
            row = row + img[dy:dy + h - 2 * r, dx:dx + w - 2 * r]
        tot = row if tot is None else tot + row
    return tot


def window_any(mask, r):
    h, w = mask.shape
    out = np.zeros((h - 2 * r, w - 2 * r), bool)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out |= mask[dy:dy + h - 2 * r, dx:dx + w - 2 * r]
    return out


def plane_sweep(ref, srcs, mvs, invd, radius, topk, var_min, cost_max):
    """sfm_mvs_plane_sweep: ref [h, w] uint8, srcs list of [h, w] uint8, mvs [nsrc, 12] f32, invd [ndepth] f32
    -> (depth [h, w] f32, cost [h, w] f32, plane [h, w] int32, volume [ndepth, h, w] f32)."""
    h, w = ref.shape
    r = int(radius)
    invd = np.asarray(invd, F)
    nd, ns = len(invd), len(srcs)
    var_min, cost_max = F(var_min), F(cost_max)
    n = F((2 * r + 1) ** 2)
    R = ref.astype(F) - F(128)
    ih, iw = h - 2 * r, w - 2 * r                  # interior: the pixels whose reference window lies in the frame
    s_r = window_sum(R, r)
    s_rr = window_sum(R * R, r)
    var_r = s_rr - (s_r * s_r) / n
    ref_ok = ~(var_r < var_min)
    vol_i = np.empty((nd, ih, iw), F)
    for j in range(nd):
        costs = np.empty((ns, ih, iw), F)
        for s in range(ns):
            W, valid = warp(srcs[s], mvs[s], invd[j], w, h)
            s_w = window_sum(W, r)
            s_ww = window_sum(W * W, r)
            s_rw = window_sum(R * W, r)
            bad = window_any(~valid, r)
            var_w = s_ww - (s_w * s_w) / n
            ok = ref_ok & ~bad & ~(var_w < var_min)
            cov = s_rw - (s_r * s_w) / n
            with np.errstate(divide="ignore", invalid="ignore"):
                c = ONE - cov / np.sqrt(np.where(ok, var_r * var_w, ONE))
            costs[s] = np.where(ok, np.clip(c, ZERO, TWO), TWO)
        costs.sort(axis=0)
        acc = costs[0].copy()
        for q in range(1, topk):
            acc = acc + costs[q]
        vol_i[j] = acc / F(topk)
    jstar = np.argmin(vol_i, axis=0)                 # first index of the minimum
    best = np.take_along_axis(vol_i, jstar[None], 0)[0]
    inv = invd[jstar]
    mid = (jstar > 0) & (jstar < nd - 1)
    jm, jp = np.clip(jstar - 1, 0, nd - 1), np.clip(jstar + 1, 0, nd - 1)
    cm1 = np.take_along_axis(vol_i, jm[None], 0)[0]
    cp1 = np.take_along_axis(vol_i, jp[None], 0)[0]
    den = (cm1 + cp1) - TWO * best
    with np.errstate(divide="ignore", invalid="ignore"):
        delta = np.where(mid & (den > ZERO), np.clip(HALF * (cm1 - cp1) / np.where(den > ZERO, den, ONE), F(-0.5), HALF), ZERO)
    step = np.where(delta >= ZERO, invd[jp] - invd[jstar], invd[jstar] - invd[jm])
    inv = np.where(mid, invd[jstar] + delta * step, inv)
    with np.errstate(divide="ignore"):
        d = ONE / inv
    d = np.where(best < cost_max, d, ZERO)
    # outside the interior every source is invalid: C_j = 2 for every j, j* = 0, depth 0
    depth = np.zeros((h, w), F)
    cost = np.full((h, w), TWO, F)
    plane = np.zeros((h, w), np.int32)
    volume = np.full((nd, h, w), TWO, F)
    depth[r:r + ih, r:r + iw] = d
    cost[r:r + ih, r:r + iw] = best
    plane[r:r + ih, r:r + iw] = jstar
    volume[:, r:r + ih, r:r + iw] = vol_i
    return depth, cost, plane, volume


def consistency(depth, nbr_depths, nbr_index, abs_, ref_index, bc, tau, min_consistent, unique):
    """sfm_mvs_consistency -> (mask [h, w] uint8, xyz [h, w, 3] f32)."""
    h, w = depth.shape
    fx, fy = _grid(w, h)
    d = depth.astype(F)
    tau = F(tau)
    has = d > ZERO
    count = np.zeros((h, w), np.int64)
    lower = np.zeros((h, w), bool)
    for v, (dv_map, a) in enumerate(zip(nbr_depths, abs_)):
        a = np.asarray(a, F)
        p = [d * ((a[3 * i] * fx + a[3 * i + 1] * fy) + a[3 * i + 2]) + a[9 + i] for i in range(3)]
        pos = p[2] > ZERO
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            den = np.where(pos, p[2], ONE)
            u = np.floor(p[0] / den + HALF)
            t = np.floor(p[1] / den + HALF)
        inb = pos & (u >= ZERO) & (u <= F(w - 1)) & (t >= ZERO) & (t <= F(h - 1))
        ui = np.where(inb, u, ZERO).astype(np.int64)
        ti = np.where(inb, t, ZERO).astype(np.int64)
        dv = dv_map.astype(F)[ti, ui]
        ok = has & inb & (dv > ZERO) & (np.abs(p[2] - dv) <= tau * dv)
        count += ok
        if nbr_index[v] < ref_index:
            lower |= ok
    keep = has & (count >= min_consistent) & ~(bool(unique) & lower)
    b = np.asarray(bc, F)
    xyz = np.stack([d * ((b[3 * i] * fx + b[3 * i + 1] * fy) + b[3 * i + 2]) + b[9 + i] for i in range(3)], -1)
    xyz = np.where(keep[..., None], xyz, ZERO).astype(F)
    return keep.astype(np.uint8), xyz
