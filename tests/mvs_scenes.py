"""Rendered multi-view scenes with ground-truth depth for the MVS tests: a few textured quads in front of a textured back wall,
seen by `n` planted cameras on a short horizontal arc.  Same method as datagen.gustav_views — exact ray / plane intersection per
pixel, the nearest hit wins, bilinear texture lookup — and the camera depth of the hit is its ray parameter (the direction
R^T K^-1 (x, y, 1) has camera z = 1).  Test-data generation: torch float64 on the CPU (or `device`)."""
import numpy as np


def look_at(C, target, up=(0.0, -1.0, 0.0)):
    """R, t of a camera at C looking at `target` (x right, y down, z forward)."""
    C, target = np.asarray(C, np.float64), np.asarray(target, np.float64)
    z = target - C
    z /= np.linalg.norm(z)
    x = np.cross(np.asarray(up, np.float64), z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    return R, -R @ C


def render_scene(n=5, w=160, h=120, seed=0, arc=0.3, tex=256, device="cpu"):
    """-> (images: list of (h, w, 3) uint8 BGR arrays, K (3x3), P [n, 3, 4] = K [R|t], depth: list of (h, w) float64 camera depth
    of the nearest hit (0 where nothing is hit))."""
    import torch
    from datagen import fast_texture
    dev = torch.device(device)
    rng = np.random.default_rng(seed)
    f = 0.9 * w
    K = np.array([[f, 0.0, (w - 1) / 2.0], [0.0, f, (h - 1) / 2.0], [0.0, 0.0, 1.0]])
    # quads: (centre, u axis, v axis, half size); the scene is centred on the origin, the cameras stand ~4 units away
    planes = []
    for q in range(3):
        o = np.array([rng.uniform(-0.8, 0.8), rng.uniform(-0.5, 0.5), rng.uniform(-0.8, 0.6)])
        nrm = np.array([rng.uniform(-0.4, 0.4), rng.uniform(-0.3, 0.3), -1.0])
        nrm /= np.linalg.norm(nrm)
        u = np.cross(nrm, [0.0, 1.0, 0.0])
        u /= np.linalg.norm(u)
        v = np.cross(nrm, u)
        planes.append((o, u, v, nrm, rng.uniform(0.5, 0.8)))
    planes.append((np.array([0.0, 0.0, 2.0]), np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0]), np.array([0.0, 0.0, -1.0]), 6.0))
    texs = torch.stack([fast_texture(tex, seed * 31 + p, dev) for p in range(len(planes))]).to(torch.float32)
    Kinv = np.linalg.inv(K)
    xs = torch.arange(w, dtype=torch.float64, device=dev)[None, :]
    ys = torch.arange(h, dtype=torch.float64, device=dev)[:, None]
    images, Ps, depths = [], [], []
    for k in range(n):
        a = arc * (k / max(n - 1, 1) - 0.5)
        C = np.array([4.0 * np.sin(a), 0.2 * np.sin(3.0 * a), -4.0 * np.cos(a)])
        R, t = look_at(C, np.zeros(3))
        Ps.append(K @ np.hstack([R, t[:, None]]))
        M = R.T @ Kinv
        best = torch.full((h, w), float("inf"), dtype=torch.float64, device=dev)
        ta = torch.zeros((h, w), dtype=torch.float64, device=dev)
        tb = torch.zeros((h, w), dtype=torch.float64, device=dev)
        ti = torch.zeros((h, w), dtype=torch.int64, device=dev)
        for pi, (o, u, v, nrm, half) in enumerate(planes):
            dn, du, dv = nrm @ M, u @ M, v @ M
            den = dn[0] * xs + dn[1] * ys + dn[2]
            s = float(nrm @ (o - C)) / torch.where(den.abs() < 1e-12, torch.full_like(den, 1e-12), den)
            aa = float((C - o) @ u) + s * (du[0] * xs + du[1] * ys + du[2])
            bb = float((C - o) @ v) + s * (dv[0] * xs + dv[1] * ys + dv[2])
            hit = (s > 0.05) & (aa.abs() < half) & (bb.abs() < half) & (s < best)
            best = torch.where(hit, s, best)
            sc = (tex - 1) / (2.0 * half)
            ta = torch.where(hit, (aa + half) * sc, ta)
            tb = torch.where(hit, (bb + half) * sc, tb)
            ti = torch.where(hit, torch.full_like(ti, pi), ti)
        x0 = torch.clamp(torch.floor(ta).long(), 0, tex - 2)
        y0 = torch.clamp(torch.floor(tb).long(), 0, tex - 2)
        fx, fy = torch.clamp(ta - x0, 0, 1).float(), torch.clamp(tb - y0, 0, 1).float()
        g = (texs[ti, y0, x0] * (1 - fx) * (1 - fy) + texs[ti, y0, x0 + 1] * fx * (1 - fy)
             + texs[ti, y0 + 1, x0] * (1 - fx) * fy + texs[ti, y0 + 1, x0 + 1] * fx * fy)
        g = torch.clamp(torch.round(g), 0, 255).to(torch.uint8).cpu().numpy()
        images.append(np.stack([g, g, g], -1))
        depths.append(torch.where(torch.isinf(best), torch.zeros_like(best), best).cpu().numpy())
    return images, K, np.stack(Ps), depths


def gray(bgr):
    """The frames are gray replicated in B, G and R: any of the channels is cv2.cvtColor's gray."""
    return np.ascontiguousarray(bgr[..., 0])


def scene_cloud(K, P, gt, step=7):
    """A sparse cloud of the scene in world units: every `step`-th ground-truth pixel of every view, back-projected."""
    pts = []
    for k in range(len(P)):
        Rt = np.linalg.solve(K, P[k])
        ys, xs = np.nonzero(gt[k][::step, ::step] > 0)
        ys, xs = ys * step, xs * step
        rays = np.linalg.solve(K, np.stack([xs, ys, np.ones_like(xs)]).astype(np.float64))
        pts.append((Rt[:, :3].T @ (rays * gt[k][ys, xs] - Rt[:, 3:])).T)
    return np.vstack(pts)


def surface_error(pts, K, P, gt):
    """Per world point: the smallest relative difference, over the views it projects into, between its camera depth and the
    ground-truth depth at its nearest pixel (inf where it lands on no rendered surface)."""
    h, w = gt[0].shape
    Xh = np.hstack([np.asarray(pts, np.float64), np.ones((len(pts), 1))]).T
    best = np.full(len(pts), np.inf)
    for k in range(len(P)):
        q = P[k] @ Xh
        with np.errstate(divide="ignore", invalid="ignore"):
            u = np.floor(q[0] / q[2] + 0.5)
            v = np.floor(q[1] / q[2] + 0.5)
        ok = (q[2] > 0) & (u >= 0) & (u <= w - 1) & (v >= 0) & (v <= h - 1)
        g = np.where(ok, gt[k][np.where(ok, v, 0).astype(int), np.where(ok, u, 0).astype(int)], 0.0)
        e = np.where(ok & (g > 0), np.abs(q[2] - g) / np.where(g > 0, g, 1.0), np.inf)
        best = np.minimum(best, e)
    return best
