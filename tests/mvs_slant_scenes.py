"""A rendered multi-view scene with slanted geometry for the PatchMatch tests (docs/mvs.md §9): one large textured plane tilted
`tilt_deg` (60-70) degrees from fronto-parallel — a floor that rises towards the back — and a fronto-parallel wall behind it, seen by
`n` planted cameras on mvs_scenes' arc.  Same method as mvs_scenes.render_scene (exact ray / plane intersection per pixel, the nearest
hit wins, bilinear texture lookup), with two more ground truths: the world normal of the hit, turned towards the camera, and which
plane was hit."""
import numpy as np

from mvs_scenes import look_at

FLOOR, WALL = 0, 1


def slant_planes(tilt_deg=65.0):
    """[(centre, u axis, v axis, normal, half size)]: the floor (index FLOOR), then the wall (index WALL)."""
    a = np.deg2rad(tilt_deg)
    nrm = np.array([0.0, -np.sin(a), -np.cos(a)])          # (0, 0, -1) is fronto-parallel; y points down, so the floor faces up
    u = np.array([1.0, 0.0, 0.0])
    v = np.cross(nrm, u)
    return [(np.array([0.0, 0.7, 0.0]), u, v, nrm, 5.0),
            (np.array([0.0, 0.0, 2.0]), np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0]), np.array([0.0, 0.0, -1.0]), 6.0)]


def render_slant_scene(n=5, w=160, h=120, seed=0, arc=0.3, tex=256, tilt_deg=65.0, device="cpu"):
    """-> (images: list of (h, w, 3) uint8 BGR, K (3x3), P [n, 3, 4], depth: list of (h, w) float64 camera depth (0 = no hit),
    normal: list of (h, w, 3) float64 unit world normals facing the camera (0 where nothing is hit), index: list of (h, w) int64
    FLOOR / WALL (-1 = no hit))."""
    import torch
    from datagen import fast_texture
    dev = torch.device(device)
    f = 0.9 * w
    K = np.array([[f, 0.0, (w - 1) / 2.0], [0.0, f, (h - 1) / 2.0], [0.0, 0.0, 1.0]])
    planes = slant_planes(tilt_deg)
    texs = torch.stack([fast_texture(tex, seed * 31 + 7 + p, dev) for p in range(len(planes))]).to(torch.float32)
    Kinv = np.linalg.inv(K)
    xs = torch.arange(w, dtype=torch.float64, device=dev)[None, :]
    ys = torch.arange(h, dtype=torch.float64, device=dev)[:, None]
    images, Ps, depths, normals, indices = [], [], [], [], []
    for k in range(n):
        a = arc * (k / max(n - 1, 1) - 0.5)
        C = np.array([4.0 * np.sin(a), 0.2 * np.sin(3.0 * a), -4.0 * np.cos(a)])
        R, t = look_at(C, np.zeros(3))
        Ps.append(K @ np.hstack([R, t[:, None]]))
        M = R.T @ Kinv
        best = torch.full((h, w), float("inf"), dtype=torch.float64, device=dev)
        ta = torch.zeros((h, w), dtype=torch.float64, device=dev)
        tb = torch.zeros((h, w), dtype=torch.float64, device=dev)
        ti = torch.full((h, w), -1, dtype=torch.int64, device=dev)
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
        tc = torch.clamp(ti, min=0)
        x0 = torch.clamp(torch.floor(ta).long(), 0, tex - 2)
        y0 = torch.clamp(torch.floor(tb).long(), 0, tex - 2)
        fx, fy = torch.clamp(ta - x0, 0, 1).float(), torch.clamp(tb - y0, 0, 1).float()
        g = (texs[tc, y0, x0] * (1 - fx) * (1 - fy) + texs[tc, y0, x0 + 1] * fx * (1 - fy)
             + texs[tc, y0 + 1, x0] * (1 - fx) * fy + texs[tc, y0 + 1, x0 + 1] * fx * fy)
        g = torch.where(ti >= 0, g, torch.zeros_like(g))
        g = torch.clamp(torch.round(g), 0, 255).to(torch.uint8).cpu().numpy()
        images.append(np.stack([g, g, g], -1))
        depths.append(torch.where(torch.isinf(best), torch.zeros_like(best), best).cpu().numpy())
        idx = ti.cpu().numpy()
        nm = np.zeros((h, w, 3))
        for pi, (o, _, _, nrm, _) in enumerate(planes):
            nm[idx == pi] = nrm if nrm @ (C - o) > 0 else -nrm
        normals.append(nm)
        indices.append(idx)
    return images, K, np.stack(Ps), depths, normals, indices
