"""Randomised parity sweep of the mesh texturing step on the GPU box: sfm_mesh_render_depth, sfm_mesh_face_views and
sfm_mesh_texture_fill (the C-ABI into sentinel-filled buffers) and mesh.texture_mesh vs the restatement tests/np_mesh_texture.py;
every output compared exactly (the depth maps and the scores as int32 views, every atlas byte), and the sentinel must survive at and
past the counted rows.

  python scripts/fuzz_mesh_texture.py [seconds] [seed] [family:case_seed]

Families (one case = one random draw; nv and nf log-uniform from 0 up to a cap that keeps the NumPy side near a second):
  soup      a face soup over the rows of a random walk (neighbouring ids are neighbouring points, so most triangles span a few
            pixels) plus up to 40 faces over arbitrary rows (large triangles: the wave-cooperative path), 1..5 views of 2..96 x
            2..96 pixels, random frames, 1..13 texels per leg, with or without vertex colours; the three calls chained
  views     the same mesh, but the depth map handed to sfm_mesh_face_views is random around the samples' own depths (exact ties
            included) and face_view handed to sfm_mesh_texture_fill is random in -2..n: each step against its own inputs
  composed  mesh.texture_mesh over host arrays against the restated chain
One case in three carries a degeneracy: nf = 0, nv = 0, a quarter of the indices from {-1, nv, INT32_MAX}, repeated indices and
duplicate faces, NaN / inf / 1e30 rows, rows behind and exactly on the camera plane (cameras K [I | t]: the depth is z itself),
a triangle over the whole frame and one over a pixel and a half, a mesh far larger than the frame; and one in three passes
device counts (smaller, equal, (0, 0), negative, too large).  Half of the cases look along +z from translated pinhole cameras,
half from cameras on an arc that look at the origin.
The script stops at the first mismatch, prints the family and the case seed that rebuilds the inputs without a GPU
(gen_case(np.random.default_rng(case_seed))), and exits non-zero.
"""
import os
import sys
import time

os.environ.setdefault("OMP_WAIT_POLICY", "passive")

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]
import np_mesh_texture as nt
from fuzz_mesh_clean import SENTINEL, bits, log_uniform_from_zero, up
from mvs_scenes import look_at

MAX_NV, MAX_NF = 1 << 16, 1 << 17
MAX_TEXELS = 1 << 20            # atlas texels the NumPy side fills per case
INT32_MAX = 2 ** 31 - 1
SENTINEL_BYTE = 0x5A


def raw_render(v, f, P, w, h, counts=None):
    """sfm_mesh_render_depth through the C-ABI into a sentinel-filled map -> (n, h, w) float32 host array."""
    import torch
    from sfm_mvs_amd import _lib
    L = _lib.lib()
    nv, nk, n = len(v), len(f), len(P)
    dv, df, dP = up(np.asarray(v, np.float32)), up(np.asarray(f, np.int32)), up(np.asarray(P, np.float32))
    dn = None if counts is None else torch.tensor([int(x) for x in counts], dtype=torch.int32, device="cuda")
    z = torch.full((n, h, w), SENTINEL, dtype=torch.int32, device="cuda")
    _lib.check(L.sfm_mesh_render_depth(_lib.ptr(dv) if nv else None, _lib.ptr(df) if nk else None, nv, nk, _lib.ptr(dn), _lib.ptr(dP), n, w, h,
                                       _lib.ptr(z), _lib.stream_ptr()), "sfm_mesh_render_depth")
    return z.cpu().numpy().view(np.float32)


def raw_views(v, f, P, zbuf, vis_tol, counts=None):
    """sfm_mesh_face_views into sentinel-filled rows -> (face_view int32 [nf_cap], face_score bits int32 [nf_cap])."""
    import torch
    from sfm_mvs_amd import _lib
    L = _lib.lib()
    nv, nk = len(v), len(f)
    n, h, w = zbuf.shape
    dv, df, dP, dz = up(np.asarray(v, np.float32)), up(np.asarray(f, np.int32)), up(np.asarray(P, np.float32)), up(np.asarray(zbuf, np.float32))
    dn = None if counts is None else torch.tensor([int(x) for x in counts], dtype=torch.int32, device="cuda")
    fv = torch.full((nk,), SENTINEL, dtype=torch.int32, device="cuda")
    fs = torch.full((nk,), SENTINEL, dtype=torch.int32, device="cuda")
    _lib.check(L.sfm_mesh_face_views(_lib.ptr(dv) if nv else None, _lib.ptr(df) if nk else None, nv, nk, _lib.ptr(dn), _lib.ptr(dP), n, w, h,
                                     _lib.ptr(dz), float(vis_tol), _lib.ptr(fv) if nk else None, _lib.ptr(fs) if nk else None, _lib.stream_ptr()),
               "sfm_mesh_face_views")
    return fv.cpu().numpy(), fs.cpu().numpy()


def raw_fill(v, c, f, P, frames, face_view, texels, counts=None):
    """sfm_mesh_texture_fill into a sentinel-filled atlas -> (side, side, 3) uint8 host array."""
    import torch
    from sfm_mvs_amd import _lib
    L = _lib.lib()
    nv, nk = len(v), len(f)
    n, h, w = frames.shape[:3]
    side, cols, _ = nt.layout(nk, texels)
    dv, df, dP, dfr = up(np.asarray(v, np.float32)), up(np.asarray(f, np.int32)), up(np.asarray(P, np.float32)), up(np.asarray(frames, np.uint8))
    dc = None if c is None or nv == 0 else up(np.asarray(c, np.float32))
    dfv = up(np.asarray(face_view, np.int32))
    dn = None if counts is None else torch.tensor([int(x) for x in counts], dtype=torch.int32, device="cuda")
    atlas = torch.full((side, side, 3), SENTINEL_BYTE, dtype=torch.uint8, device="cuda")
    _lib.check(L.sfm_mesh_texture_fill(_lib.ptr(dv) if nv else None, _lib.ptr(dc), _lib.ptr(df) if nk else None, nv, nk, _lib.ptr(dn), _lib.ptr(dP),
                                       _lib.ptr(dfr), n, w, h, _lib.ptr(dfv) if nk else None, int(texels), cols, side, _lib.ptr(atlas),
                                       _lib.stream_ptr()), "sfm_mesh_texture_fill")
    return atlas.cpu().numpy()


def compare_views(got, want, nk):
    fv, fs = got
    wv, ws = want
    k = len(wv)
    bad = []
    if not np.array_equal(fv[:k], wv):
        bad.append(f"face_view ({int((fv[:k] != wv).sum())} of {k} rows)")
    if not np.array_equal(fs[:k], bits(ws)):
        bad.append(f"face_score ({int((fs[:k] != bits(ws)).sum())} of {k} rows)")
    if not (np.all(fv[k:] == SENTINEL) and np.all(fs[k:] == SENTINEL)):
        bad.append("face_view or face_score written at or past the counted rows")
    return bad


def check_chain(v, c, f, P, frames, vis_tol, texels, counts=None):
    """The three calls chained, each output against the restatement -> (list of what differs, the restated (zbuf, view, score, atlas))."""
    n, h, w = frames.shape[:3]
    wz = nt.render_depth(v, f, P, w, h, counts)
    wv, ws = nt.face_views(v, f, P, wz, vis_tol, counts)
    full = np.full(len(f), -1, np.int32)
    full[:len(wv)] = wv
    wa = nt.texture_fill(v, c, f, P, frames, full, texels, counts)
    bad = []
    z = raw_render(v, f, P, w, h, counts)
    if not np.array_equal(bits(z), bits(wz)):
        bad.append(f"zbuf ({int((bits(z) != bits(wz)).sum())} of {wz.size} pixels)")
    bad += compare_views(raw_views(v, f, P, z, vis_tol, counts), (wv, ws), len(f))
    a = raw_fill(v, c, f, P, frames, full, texels, counts)
    if not np.array_equal(a, wa):
        bad.append(f"atlas ({int(np.any(a != wa, axis=2).sum())} of {wa.shape[0] * wa.shape[1]} texels)")
    return bad, (wz, wv, ws, wa)


def pinhole_views(rng, n, w, h):
    """K [I | t_k]: cameras that look along +z, shifted sideways; the depth of a point is its z."""
    fl = 0.9 * w
    K = np.array([[fl, 0.0, (w - 1) / 2.0], [0.0, fl * rng.uniform(0.8, 1.2), (h - 1) / 2.0], [0.0, 0.0, 1.0]])
    return np.stack([K @ np.hstack([np.eye(3), np.array([[rng.uniform(-0.5, 0.5)], [rng.uniform(-0.3, 0.3)], [4.0]])]) for _ in range(n)])


def arc_views(rng, n, w, h):
    fl = 0.9 * w
    K = np.array([[fl, 0.0, (w - 1) / 2.0], [0.0, fl, (h - 1) / 2.0], [0.0, 0.0, 1.0]])
    out = []
    for k in range(n):
        a = 0.6 * (k / max(n - 1, 1) - 0.5) + rng.uniform(-0.05, 0.05)
        R, t = look_at(np.array([4.0 * np.sin(a), 0.2 * np.sin(3.0 * a), -4.0 * np.cos(a)]), np.zeros(3))
        out.append(K @ np.hstack([R, t[:, None]]))
    return np.stack(out)


def rows_of(P):
    return np.ascontiguousarray(np.asarray(P, np.float64).reshape(-1, 12)).astype(np.float32)


def walk(rng, nv, step, reach):
    """nv rows of a random walk of `step` a move, folded back into the cube of half side `reach`."""
    if nv == 0:
        return np.zeros((0, 3), np.float32)
    p = np.cumsum(rng.standard_normal((nv, 3)) * step, axis=0) + rng.uniform(-0.5, 0.5, 3)
    p = np.abs((p + reach) % (4.0 * reach) - 2.0 * reach) - reach              # a triangle wave: reflection at the walls
    return p.astype(np.float32)


def walk_soup(rng, nv, nk, wild=40):
    """nk faces whose three indices lie within 4 of each other, `wild` of them over arbitrary rows instead."""
    if nv == 0 or nk == 0:
        return np.zeros((nk, 3), np.int32) if nv else rng.integers(-3, 4, (nk, 3)).astype(np.int32)
    base = rng.integers(0, nv, nk)
    f = np.clip(base[:, None] + rng.integers(-3, 4, (nk, 3)), 0, nv - 1)
    hit = rng.permutation(nk)[:min(wild, nk)]
    f[hit] = rng.integers(0, nv, (len(hit), 3))
    return np.ascontiguousarray(f, np.int32)


def gen_case(rng):
    """(tag, vertices, colours or None, faces, P float32 [n, 12], frames, vis_tol, texels, counts or None)."""
    nv, nk = log_uniform_from_zero(rng, MAX_NV), log_uniform_from_zero(rng, MAX_NF)
    quirk = int(rng.integers(0, 9)) if rng.random() < 1.0 / 3 else -1
    if quirk == 0:
        nk = 0
    elif quirk == 1:
        nv = 0
    n, w, h = int(rng.integers(1, 6)), int(rng.integers(2, 97)), int(rng.integers(2, 97))
    pin = bool(rng.random() < 0.5) or quirk == 5
    P = rows_of(pinhole_views(rng, n, w, h) if pin else arc_views(rng, n, w, h))
    step = float(np.exp(rng.uniform(np.log(0.01), np.log(0.5))))
    reach = float(rng.choice([0.5, 1.5, 3.0]))
    v = walk(rng, nv, step, reach)
    c = (rng.random((nv, 3)) * 255.0).astype(np.float32) if rng.random() < 0.6 else None
    f = walk_soup(rng, nv, nk, int(rng.integers(0, 41)))
    frames = rng.integers(0, 256, (n, h, w, 3)).astype(np.uint8)
    texels = int(rng.choice([1, 2, 3, 4, 8, 13]))
    while texels > 1 and nt.layout(nk, texels)[0] ** 2 > MAX_TEXELS:
        texels -= 1
    vis_tol = float(rng.choice([0.0, 0.0025, 0.02, 0.5]))
    tag = f"nv {nv} nf {nk} quirk {quirk} views {n} of {w} x {h} pinhole {pin} step {step:.3g} reach {reach} texels {texels} vis_tol {vis_tol} colours {c is not None}"
    if quirk == 2 and nk:                                     # a quarter of the indices name no vertex
        hit = rng.random((nk, 3)) < 0.25
        f[hit] = rng.choice(np.array([-1, nv, INT32_MAX], np.int64), int(hit.sum())).astype(np.int32)
    elif quirk == 3 and nk:                                   # duplicate faces, (a, a, b), (a, a, a)
        f[rng.random(nk) < 0.3] = f[0]
        k = rng.random(nk) < 0.3
        f[k, 1] = f[k, 0]
        k = rng.random(nk) < 0.2
        f[k, 2] = f[k, 0]
    elif quirk == 4 and nv:                                   # rows that are not finite or overflow
        hit = rng.random((nv, 3)) < 0.1
        v[hit] = rng.choice(np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 3e38], np.float32), int(hit.sum()))
    elif quirk == 5 and nv:                                   # behind and exactly on the camera plane (z + 4 = 0 in these cameras)
        hit = rng.random(nv) < 0.2
        v[hit, 2] = rng.choice(np.array([-4.0, -4.5, -3.9999998, -6.0], np.float32), int(hit.sum()))
    elif quirk == 6 and nv >= 6 and nk >= 2:                  # a triangle over the whole frame and one over a pixel and a half
        v[:3] = [[-40.0, -40.0, 1.0], [40.0, -40.0, 1.0], [0.0, 60.0, 1.0]]
        px = 4.0 / (0.9 * w)
        v[3:6] = np.array([[0.0, 0.0, 0.0], [1.5 * px, 0.0, 0.0], [0.0, 2.0 * px, 0.0]], np.float32)
        f[0], f[1] = (0, 1, 2) if rng.random() < 0.5 else (0, 2, 1), (3, 5, 4)
    elif quirk == 7 and nv:                                   # a mesh far larger than the frame
        v *= np.float32(30.0)
    elif quirk == 8 and nv:                                   # everything on a few pixels: ties of the minimum and of the scores
        v = (np.round(v * 4.0) / 4.0).astype(np.float32)
        P[1:] = P[0]
    counts = None
    if rng.random() < 1.0 / 3:
        counts = [(int(rng.integers(0, nv + 1)), int(rng.integers(0, nk + 1))), (nv, nk), (0, 0), (-1, int(rng.integers(0, nk + 1))),
                  (int(rng.integers(0, nv + 1)), -7), (nv + 1, nk + 1), (INT32_MAX, INT32_MAX)][int(rng.integers(0, 7))]
        tag += f" counts {counts}"
    return tag, v, c, f, P, frames, vis_tol, texels, counts


def case_soup(rng):
    tag, v, c, f, P, frames, vis_tol, texels, counts = gen_case(rng)
    bad, _ = check_chain(v, c, f, P, frames, vis_tol, texels, counts)
    return f"{tag}: {', '.join(bad)}" if bad else None


def case_views(rng):
    tag, v, c, f, P, frames, vis_tol, texels, counts = gen_case(rng)
    n, h, w = frames.shape[:3]
    # a depth map around the depths the samples have: the own map, scaled per pixel by 1 or by a factor near 1 / (1 + vis_tol)
    z = nt.render_depth(v, f, P, w, h, counts)
    tol1 = np.float32(np.float32(1.0) + np.float32(vis_tol))
    pick = rng.integers(0, 4, z.shape)
    with np.errstate(all="ignore"):
        z = np.where(pick == 0, z, np.where(pick == 1, z / tol1, np.where(pick == 2, np.nextafter(z / tol1, np.float32(0.0)), z * np.float32(0.9)))).astype(np.float32)
    bad = compare_views(raw_views(v, f, P, z, vis_tol, counts), nt.face_views(v, f, P, z, vis_tol, counts), len(f))
    fv = rng.integers(-2, n + 1, len(f)).astype(np.int32)
    a, wa = raw_fill(v, c, f, P, frames, fv, texels, counts), nt.texture_fill(v, c, f, P, frames, fv, texels, counts)
    if not np.array_equal(a, wa):
        bad.append(f"atlas ({int(np.any(a != wa, axis=2).sum())} texels)")
    return f"{tag}: {', '.join(bad)}" if bad else None


def case_composed(rng):
    from sfm_mvs_amd import mesh
    tag, v, c, f, P, frames, vis_tol, texels, _ = gen_case(rng)
    n, h, w = frames.shape[:3]
    out = mesh.texture_mesh(v, c, f, list(frames), np.eye(3), P.reshape(-1, 3, 4), texels, vis_tol)
    wz = nt.render_depth(v, f, P, w, h)
    wv, _ = nt.face_views(v, f, P, wz, vis_tol)
    wa = nt.texture_fill(v, c, f, P, frames, wv, texels)
    bad = []
    if not np.array_equal(out["face_view"], wv) or out["textured"] != int((wv >= 0).sum()):
        bad.append("face_view")
    if not np.array_equal(out["atlas"], wa):
        bad.append("atlas")
    if not np.array_equal(out["uv"], nt.uv_of(len(f), texels)):
        bad.append("uv")
    return f"{tag}: {', '.join(bad)}" if bad else None


FAMILIES = [("soup", case_soup, 5), ("views", case_views, 3), ("composed", case_composed, 2)]


def run(budget, seed, log=print):
    """Cases for `budget` seconds from `seed`; stops at the first mismatch -> (counts per family, mismatches, seconds)."""
    fns = {name: fn for name, fn, _ in FAMILIES}
    rng = np.random.default_rng(seed)
    weights = np.array([w for _, _, w in FAMILIES], float); weights /= weights.sum()
    t0 = time.time(); counts = {name: 0 for name, _, _ in FAMILIES}; bad = 0
    while time.time() - t0 < budget and not bad:
        name = FAMILIES[int(rng.choice(len(FAMILIES), p=weights))][0]
        case_seed = int(rng.integers(1 << 31))
        try:
            msg = fns[name](np.random.default_rng(case_seed))
        except Exception as e:  # noqa: BLE001
            msg = f"EXCEPTION {e!r}"[:300]
        counts[name] += 1
        if msg:
            bad += 1
            log(f"MISMATCH {name} (seed {seed}, case seed {case_seed}; replay: fuzz_mesh_texture.py 0 0 {name}:{case_seed}) {msg}")
    return counts, bad, time.time() - t0


def main():
    import sfm_mvs_amd
    from sfm_mvs_amd import _lib
    budget = float(sys.argv[1]) if len(sys.argv) > 1 else 120.0
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    sfm_mvs_amd.lib()
    if len(sys.argv) > 3:                               # replay one case
        name, case_seed = sys.argv[3].split(":")
        msg = {n: fn for n, fn, _ in FAMILIES}[name](np.random.default_rng(int(case_seed)))
        print(f"fuzz_mesh_texture replay {name}:{case_seed}: {msg or 'no mismatch'}")
        return 1 if msg else 0
    counts, bad, dt = run(budget, seed, log=lambda s: print(s, flush=True))
    print(f"fuzz_mesh_texture: seed {seed}, {sum(counts.values())} cases {counts}, {bad} mismatches, {dt:.0f} s")
    print(f"sfm_build_id {_lib.build_id()}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
