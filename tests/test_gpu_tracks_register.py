"""The TRACKS-REGISTER family on the device (sfm_track_restrict, sfm_track_adopt, sfm_track_view_scores, sfm_track_correspondences,
register.register_tracks): every output word equal to the restatement tests/np_tracks_register.py, float rows as integer views, NaN
equal to NaN; the loop against its CPU twin (include/sfm_hip.h, "TRACKS-REGISTER"; docs/tracks.md §10)."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

import np_tracks as nt  # noqa: E402
import np_tracks_register as ng  # noqa: E402
import fuzz_tracks as fz  # noqa: E402
import fuzz_tracks_register as fg  # noqa: E402
import register_cases as rc  # noqa: E402
from fuzz_tracks import dev  # noqa: E402

INT32_MAX = 2 ** 31 - 1
FUZZ_FLOOR = 8000              # a tenth of the cases the committed logs hold, rounded down to one figure (docs/tracks.md §10.6)
LDS_IMAGES = 256                # SFM_REGISTER_LDS_IMAGES: the last n_img whose scores are kept in LDS


def grid_table(rng, T, L, n_img, extra=3):
    """T tracks of exactly L observations over the first L of n_img images; every image holds T + extra keypoints (node = image * (T +
    extra) + track), the extra ones in no track."""
    m = T + extra
    n = n_img * m
    obs_node = (np.arange(L)[None, :] * m + np.arange(T)[:, None]).reshape(-1).astype(np.int32) if T else np.zeros(0, np.int32)
    node_track = np.full(n, -1, np.int32)
    node_track[obs_node] = np.repeat(np.arange(T), L)
    kp = np.stack([rng.uniform(-40, fg.FRAME[0] + 40, n), rng.uniform(-40, fg.FRAME[1] + 40, n)], 1).astype(np.float32)
    return dict(n=n, n_img=n_img, img_off=(np.arange(n_img + 1) * m).astype(np.int32), track_off=(L * np.arange(T + 1)).astype(np.int32),
                obs_node=obs_node, node_track=node_track, kp=kp, counts=np.array([T, L * T, 0, 0, 0, 0], np.int32), T=T, deg=-1)


def registered_sets(n_img):
    alt = (np.arange(n_img) % 2 == 0).astype(np.uint8)
    one = np.zeros(n_img, np.uint8)
    one[n_img // 2] = 1
    return dict(none=np.zeros(n_img, np.uint8), all=np.ones(n_img, np.uint8), one=one, alternating=alt)


@pytest.mark.gpu
@pytest.mark.parametrize("n_img", [1, 2, 3, 64, 65])
def test_every_count_length_and_registered_set(hip, n_img):
    """Track counts around a wave and a workgroup (and 1 025: five blocks, a scan over more than one entry), lengths 2, 3 and n_img, the
    registered set none / all / one / alternating, has_point none / all / random: all four entry points."""
    rng = np.random.default_rng(4000 + n_img)
    for T in (0, 1, 2, 3, 255, 256, 257, 1025):
        for L in sorted({2, 3, n_img}):
            t = grid_table(rng, T if 2 <= L <= n_img else 0, min(L, n_img), n_img)    # a track has two observations or more
            d = fg.device_table(t)
            for name, reg in registered_sets(n_img).items():
                for min_len in (2, max(L, 1)):
                    msg = fg.check_restrict(t, reg, min_len, d)
                    assert not msg, (T, L, name, min_len, msg)
                t["registered"] = reg
                msg = fg.check_adopt(*fg.gen_adopt(rng, t), d)
                assert not msg, (T, L, name, msg)
            cap = t["n"] // 2 + 1
            X_full = rng.normal(size=(cap, 3)).astype(np.float32)
            for has in (np.zeros(cap, np.uint8), np.ones(cap, np.uint8), (rng.random(cap) < 0.5).astype(np.uint8)):
                for grid in (1, 8):
                    msg = fg.check_scores(t, has, grid, d=d)
                    assert not msg, (T, L, grid, msg)
                msg = fg.check_corr(t, has, X_full, int(rng.integers(n_img)), d=d)
                assert not msg, (T, L, msg)


@pytest.mark.gpu
@pytest.mark.parametrize("n_img", [LDS_IMAGES, LDS_IMAGES + 1])
def test_scores_on_both_sides_of_the_lds_bound(hip, n_img):
    """256 images keep their counters and masks in LDS, 257 take the global atomics: the same words; 20 blocks of nodes, empty images."""
    rng = np.random.default_rng(4100 + n_img)
    for seed in range(4):
        t = fg.gen_table(np.random.default_rng([seed, n_img]), n_img=n_img, n=5000 + seed, deg=-1)
        for has in (t["has_point"], np.ones_like(t["has_point"]), np.zeros_like(t["has_point"])):
            for grid in (1, 8):
                msg = fg.check_scores(t, has, grid)
                assert not msg, (seed, grid, msg)
        assert ng.view_scores(t["counts"], t["node_track"], np.ones_like(t["has_point"]), t["img_off"], t["kp"], t["n"], *fg.FRAME, 8)[0].max() > 0
    t = grid_table(rng, 40, n_img, n_img, extra=0)                            # every image sees every track
    msg = fg.check_scores(t, np.ones(t["n"] // 2 + 1, np.uint8), 8)
    assert not msg, msg


@pytest.mark.gpu
def test_correspondences_of_images_of_every_size(hip):
    """Images of 0, 1, 255, 256 and 257 keypoints (and a last one of 300 that closes the tracks): ranks inside a block and across blocks."""
    rng = np.random.default_rng(4200)
    sizes = [0, 1, 255, 256, 257, 300]
    img_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    n = int(img_off[-1])
    o = img_off.tolist()
    tracks = [[o[2] + j, o[3] + j, o[4] + j, o[5] + j] for j in range(255)]      # every keypoint of images 1..4 lies in a track
    tracks += [[o[1], o[3] + 255, o[4] + 255, o[5] + 255], [o[4] + 256, o[5] + 256]]
    T = len(tracks)
    track_off = np.concatenate([[0], np.cumsum([len(t) for t in tracks])]).astype(np.int32)
    obs_node = np.array([u for t in tracks for u in t], np.int32)
    node_track = np.full(n, -1, np.int32)
    node_track[obs_node] = np.repeat(np.arange(T), np.diff(track_off))
    t = dict(n=n, n_img=len(sizes), img_off=img_off, track_off=track_off, obs_node=obs_node, node_track=node_track,
             kp=rng.uniform(0, 600, (n, 2)).astype(np.float32), counts=np.array([T, len(obs_node), 0, 0, 0, 0], np.int32), T=T, deg=-1)
    d = fg.device_table(t)
    cap = n // 2 + 1
    X_full = rng.normal(size=(cap, 3)).astype(np.float32)
    X_full[::7] = np.nan
    full = 0
    for has in (np.ones(cap, np.uint8), np.zeros(cap, np.uint8), (rng.random(cap) < 0.6).astype(np.uint8) * np.uint8(9)):
        for image in range(len(sizes)):
            k = len(ng.correspondences(image, t["counts"], node_track, has, X_full, img_off, t["kp"], n)[2])
            full = max(full, k)
            for capacity in {k, max(k - 1, 0), k + 5}:
                msg = fg.check_corr(t, has, X_full, image, capacity, d=d)
                assert not msg, (image, capacity, msg)
    assert full == 257                                                       # an image whose rows span two blocks


@pytest.mark.gpu
def test_nodes_outside_the_range_nan_keypoints_and_stray_track_indices(hip):
    """A quarter of the observations from {-1, N, INT32_MAX}; a quarter of node_track and a fifth of both track_src outside their tables;
    NaN, infinite and far keypoints: the generator's degeneracies one by one, every entry point."""
    for deg in (1, 2, 3, 4, 5):
        for seed in range(6):
            rng = np.random.default_rng([deg, seed])
            t = fg.gen_table(rng, deg=deg, n=int(rng.choice([300, 2000, 9000])))
            d = fg.device_table(t)
            msg = (fg.check_restrict(t, t["registered"], 2, d) or fg.check_adopt(*fg.gen_adopt(rng, t), d) or fg.check_scores(t, t["has_point"], 8, d=d)
                   or fg.check_scores(t, t["has_point"], 1, d=d)
                   or fg.check_corr(t, t["has_point"], rng.normal(size=(t["n"] // 2 + 1, 3)).astype(np.float32), int(rng.integers(t["n_img"])), d=d))
            assert not msg, (deg, seed, msg)
    # every keypoint of image 0 has a NaN coordinate: counted in seen, no bit set; infinite ones fall into the border cells
    t = grid_table(np.random.default_rng(5), 300, 4, 4)
    m = t["n"] // 4
    t["kp"][:m, 0] = np.nan
    t["kp"][m:2 * m:2] = (np.inf, -np.inf)
    has = np.ones(t["n"] // 2 + 1, np.uint8)
    for grid in (1, 8):
        msg = fg.check_scores(t, has, grid)
        assert not msg, (grid, msg)
    seen, cover, cells = ng.view_scores(t["counts"], t["node_track"], has, t["img_off"], t["kp"], t["n"], *fg.FRAME, 8)
    assert seen.tolist() == [300] * 4 and cover[0] == 0 and cells[0] == 0 and int(cover[1]) & (1 << 7) and cells.max() <= 64


def garbage(t, rng, unordered):
    """The table behind counts = (INT32_MAX, -7): every row of the capacity is a track.  unordered: the offsets past the true ones lie
    inside 0..N in no order (ranges that overlap) over random nodes, else offsets and nodes past the true ones hold the sentinel: row T runs
    from the true end to N over nodes outside the range, the rows behind it are empty."""
    n = t["n"]
    off = fg.padded(t["track_off"], n // 2 + 2)
    if unordered:
        off[t["T"] + 1:] = rng.integers(0, n + 1, n // 2 + 2 - t["T"] - 1)
    g = dict(t, counts=np.array([INT32_MAX, -7, 0, 0, 0, 0], np.int32), track_off=off, obs_node=fg.padded(t["obs_node"], n))
    if unordered:
        g["obs_node"][len(t["obs_node"]):] = rng.integers(0, n, n - len(t["obs_node"]))
    return g


@pytest.mark.gpu
def test_garbage_device_counts_are_clamped(hip):
    """counts = (INT32_MAX, -7): T becomes N / 2 + 1 and nobs N; offsets are clamped; the rows after the true tracks are empty."""
    rng = np.random.default_rng(4300)
    t = grid_table(rng, 300, 4, 6)
    g = garbage(t, rng, unordered=False)
    assert ng.clamped(g["counts"], g["n"]) == (g["n"] // 2 + 1, g["n"])
    d = fg.device_table(g)
    reg = np.array([1, 1, 0, 1, 1, 0], np.uint8)
    msg = fg.check_restrict(g, reg, 2, d)
    assert not msg, msg
    want = ng.restrict(g["counts"], g["track_off"], g["obs_node"], g["img_off"], reg, g["n"], 2)
    assert want[3].tolist() == [300, 900, 0, 300]
    g["registered"] = reg
    msg = fg.check_adopt(*fg.gen_adopt(rng, g), d) or fg.check_scores(g, np.ones(g["n"] // 2 + 1, np.uint8), 8, d=d)
    assert not msg, msg
    msg = fg.check_corr(g, np.ones(g["n"] // 2 + 1, np.uint8), rng.normal(size=(g["n"] // 2 + 1, 3)).astype(np.float32), 1, d=d)
    assert not msg, msg


def guarded(rows, dtype, width=None):
    """(whole, view): `rows` rows between two guards of 64 rows, every byte of it 0x5A."""
    shape = (rows + 128,) if width is None else (rows + 128, width)
    nbytes = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
    whole = torch.full((nbytes,), fg.BYTE, dtype=torch.uint8, device="cuda").view(dtype).view(shape)
    return whole, whole[64:64 + rows]


def guards_intact(whole, rows):
    b = whole.view(-1).view(torch.uint8).view(whole.shape[0], -1)
    return bool((b[:64] == fg.BYTE).all()) and bool((b[64 + rows:] == fg.BYTE).all())


@pytest.mark.gpu
def test_overlapping_ranges_stay_inside_the_buffers(hip):
    """counts = (INT32_MAX, -7) over offsets that lie inside 0..N in no order, garbage track_src and node_track: the words are unspecified
    (include/sfm_hip.h); nothing lands outside the arrays, the flags are flags and the counts lie inside their ranges."""
    from sfm_mvs_amd import register
    rng = np.random.default_rng(4400)
    t = grid_table(rng, 300, 8, 8, extra=2)
    g = garbage(t, rng, unordered=True)
    n, cap, n_img = g["n"], g["n"] // 2 + 1, 8
    lo, hi = ng.ranges(g["track_off"], cap, n)
    assert int((hi - lo).sum()) > 20 * n                                      # the ranges cover every row many times
    g["node_track"] = rng.integers(-3, cap + 3, n).astype(np.int32)
    d = fg.device_table(g)
    i32, f32, u8 = torch.int32, torch.float32, torch.uint8
    rb = [guarded(cap + 1, i32), guarded(n, i32), guarded(cap, i32), guarded(4, i32)]
    r = register.restrict_tracks(d["counts"], d["track_off"], d["obs_node"], d["img_off"], dev(np.ones(n_img, np.uint8)), 2, out=tuple(v for _, v in rb))
    src = dev(rng.integers(-3, cap + 3, cap).astype(np.int32))
    pruned = (dev(rng.integers(0, n + 1, cap + 1).astype(np.int32)), d["obs_node"], dev(rng.normal(size=(cap, 3)).astype(np.float32)), src,
              dev(np.array([INT32_MAX, -7, 0, 0], np.int32)))
    ab = [guarded(cap, f32, 3), guarded(cap, u8), guarded(n, u8)]
    a = register.adopt_points(d["counts"], d["track_off"], d["obs_node"], (r[0], r[1], src, r[3]), pruned, out=tuple(v for _, v in ab))
    sb = [guarded(n_img, i32), guarded(n_img, torch.int64), guarded(n_img, i32)]
    register.view_scores(d["counts"], d["node_track"], a[1], d["img_off"], d["kp"], fg.FRAME, 8, out=tuple(v for _, v in sb))
    cb = [guarded(50, f32, 3), guarded(50, f32, 2), guarded(50, i32), guarded(1, i32)]
    register.correspondences(3, d["counts"], d["node_track"], a[1], a[0], d["img_off"], d["kp"], 50, out=tuple(v for _, v in cb))
    torch.cuda.synchronize()
    for (whole, _), rows in zip(rb + ab + sb + cb, [cap + 1, n, cap, 4, cap, cap, n, n_img, n_img, n_img, 50, 50, 50, 1]):
        assert guards_intact(whole, rows), rows
    c2 = rb[3][1].tolist()
    assert 0 <= c2[0] <= cap and c2[2] >= 0 and set(a[1].unique().tolist()) <= {0, 1} and set(a[2].unique().tolist()) <= {0, 1}
    assert 0 <= int(sb[0][1].min()) and int(sb[0][1].sum()) <= n and 0 <= int(cb[3][1][0]) <= n


# ---- the chain and the wrappers ---------------------------------------------------------------------------------------------------

def ring_device(case):
    return (dev(case["store"]), dev(case["nq"]), dev(np.array(case["pairs"], np.int32)), dev(case["img_off"]), dev(case["kp"]),
            dev(case["P"].reshape(-1, 12)))


@pytest.mark.gpu
def test_the_chain_never_waits_and_feeds_pnp(hip):
    """match_edges -> components -> build -> restrict -> triangulate -> refine -> prune -> adopt -> scores -> correspondences under torch's
    sync debug mode "error"; with every image registered restrict returns the input table; every word equals the restated round; the
    correspondences of an image given to solve_pnp_ransac as they are recover its planted camera."""
    from sfm_mvs_amd import ransac, register, tracks
    case = rc.scene("ring")
    store, nq, pr, off, kp, P = ring_device(case)
    n = int(case["img_off"][-1])
    reg = np.ones(8, np.uint8)
    reg[6] = 0
    reg_all, reg_d = dev(np.ones(8, np.uint8)), dev(reg)
    P_host = case["P"].reshape(8, 12).copy()
    P_host[6] = 0.0
    P6 = dev(P_host)

    def chain():
        labels, _ = tracks.track_components(tracks.match_edges(store, nq, pr, off), n)
        node_track, track_off, obs_node, counts = tracks.build_tracks(labels, off)
        same = register.restrict_tracks(counts, track_off, obs_node, off, reg_all)
        r = register.restrict_tracks(counts, track_off, obs_node, off, reg_d)
        tri = tracks.triangulate_tracks(r[3], r[0], r[1], off, kp, P6)
        rf = tracks.refine_tracks(r[3], r[0], r[1], off, kp, P6, tri[0], tri[3])
        p = tracks.prune_tracks(r[3], r[0], r[1], rf[0], rf[1], rf[4], rf[5], rf[6], rf[8], 2, 2.0, 2.0)
        a = register.adopt_points(counts, track_off, obs_node, r, p)
        s = register.view_scores(counts, node_track, a[1], off, kp, rc.FRAME, 8)
        c = register.correspondences(6, counts, node_track, a[1], a[0], off, kp, capacity=400)
        return (node_track, track_off, obs_node, counts), same, r, p, a, s, c

    chain()                                                                  # warm: the workspaces
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        table, same, r, p, a, s, c = chain()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    base = nt.run(case["store"], case["nq"], case["pairs"], case["img_off"], case["kp"], case["P"])
    T, nobs = 400, 3200
    assert table[3].cpu().numpy()[:2].tolist() == [T, nobs]
    # every image registered: the words of the input table, the identity as track_src
    assert same[3].cpu().numpy().tolist() == [T, nobs, 0, 0] and torch.equal(same[0][:T + 1], table[1][:T + 1]) and torch.equal(same[1][:nobs], table[2][:nobs])
    assert same[2][:T].cpu().numpy().tolist() == list(range(T))
    t = dict(n=n, n_img=8, img_off=case["img_off"], track_off=base["track_off"], obs_node=base["obs_node"], node_track=base["node_track"], kp=case["kp"],
             counts=base["counts"], T=T, deg=-1)
    want = fg.restated_round(t, reg, P_host, max_cos=float(np.cos(np.deg2rad(2.0))))
    eq = lambda got, w, rows: np.array_equal(got[:rows].cpu().numpy().view(np.uint8).reshape(rows, -1), np.ascontiguousarray(w).view(np.uint8).reshape(rows, -1))  # noqa: E731
    Tr, nr_, Tp, np_ = (int(v) for v in (want[0][3][0], want[0][3][1], want[1][4][0], want[1][4][1]))
    assert (Tr, nr_, Tp) == (400, 2800, 400)
    assert eq(r[3], want[0][3], 4) and eq(r[0], want[0][0], Tr + 1) and eq(r[1], want[0][1], nr_) and eq(r[2], want[0][2], Tr)
    assert eq(p[4], want[1][4], 4) and eq(p[0], want[1][0], Tp + 1) and eq(p[1], want[1][1], np_) and eq(p[2], want[1][2], Tp) and eq(p[3], want[1][3], Tp)
    assert eq(a[0], want[2][0], T) and eq(a[1], want[2][1], T) and eq(a[2], want[2][2], nobs)
    assert eq(s[0], want[3][0], 8) and eq(s[1], want[3][1], 8) and eq(s[2], want[3][2], 8) and want[3][0].tolist() == [400] * 8
    wc = ng.correspondences(6, base["counts"], base["node_track"], want[2][1], want[2][0], case["img_off"], case["kp"], n)
    assert int(c[3][0]) == 400 == len(wc[2]) and eq(c[0], wc[0], 400) and eq(c[1], wc[1], 400) and eq(c[2], wc[2], 400)
    ok, rvec, tvec, inl = ransac.solve_pnp_ransac(c[0], c[1], case["K"])
    assert ok and len(inl) >= 380
    from sfm_mvs_amd import hostgeom
    P_got = case["K"] @ np.c_[hostgeom.rodrigues_vec2mat(rvec.reshape(3)), tvec.reshape(3)]
    centre = rc.centres_of(P_got[None])[0] - rc.centres_of(case["P"][6:7])[0]
    print(f"PnP on the correspondences of image 6: {len(inl)} inliers, centre {np.linalg.norm(centre):.5f} from the planted one (radius 8)")
    assert np.linalg.norm(centre) < 0.05                                     # 0.3 px noise at f = 900, depth 8: a centre within millimetres of 8 units


# ---- register_tracks end to end ---------------------------------------------------------------------------------------------------

def device_scene(name):
    from sfm_mvs_amd import sharded
    case = rc.scene(name)
    des = [torch.from_numpy(np.ascontiguousarray(d)).cuda() for d in case["des"]]
    store, nq = sharded.match_pairs_sharded(des, case["pairs"], batch=4)
    kps = [torch.from_numpy(np.ascontiguousarray(k, np.float32)).cuda() for k in case["kps"]]
    return case, store.contiguous(), nq, kps


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ring_permuted", "gustav_permuted", "ring_duplicate", "ring_clutter", "ring_corrupted"])
def test_register_tracks_end_to_end(hip, name):
    """match_pairs_sharded -> register_tracks against the CPU twin: the same seed candidates, order, registered set and per-step seen /
    cells (the RANSAC entry points are bit-identical to the oracle's and the kernels to the restatements, so both loops see the same
    numbers up to the bundle adjustment's float64 sums; no scene here sits on a tie those could break); the twin's assertions; the
    centre bar against the restatement's BA from the planted cameras; adjust_tracks takes the result."""
    from sfm_mvs_amd import register, tracks
    case, store, nq, kps = device_scene(name)
    assert np.array_equal(store.cpu().numpy(), case["store"])
    got = register.register_tracks(store, nq, case["pairs"], kps, case["K"], rc.FRAME)
    _, eng, want = rc.twin(name)
    order = got["order"]
    assert order.tolist() == want["order"].tolist() and got["registered"].tolist() == want["registered"].tolist()
    assert got["tries"].tolist() == want["tries"].tolist() and got["rounds"] == want["rounds"]
    assert [(s["pair"], s["shared"], s["points"]) for s in got["seeds"]] == [(s["pair"], s["shared"], s["points"]) for s in want["seeds"]]
    assert [(s["image"], s["seen"], s["cells"], s["accepted"]) for s in got["steps"]] == [(s["image"], s["seen"], s["cells"], s["accepted"]) for s in want["steps"]]
    assert got["seen"].tolist() == want["seen"].tolist() and got["cells"].tolist() == want["cells"].tolist()
    n, pure = rc.pure_tracks(case, got)
    med = float(np.median(rc.centre_errors(got["P"][order], case["P"][order])))
    ref, _ = rc.truth_start(case, got)
    print(f"{name}: order {order.tolist()}, {n} points ({pure} pure), {got['rounds']} rounds, BA costs {[round(h[-1], 4) for h in got['ba_history']]}; "
          f"median centre error {med:.7f} against {ref:.7f} (ratio {med / ref:.4f}, bar {rc.CENTRE_BAR})")
    assert n == len(got["points"]) > 0 and pure == n
    assert np.isfinite(got["P"][order]).all() and np.isnan(got["P"][~got["registered"]]).all()
    assert med <= rc.CENTRE_BAR * ref, (med, ref)
    if name == "ring_duplicate":
        assert got["seeds"][0]["pair"] == (0, 8) and got["seeds"][0]["points"] == 0 and got["registered"].all()
        clutter = case["ids"][eng.obs_node[eng.track_off[:-1]]] < 0
        assert not np.isin(np.flatnonzero(clutter), got["track_idx"]).any()   # no clutter track has a point
    if name == "ring_clutter":
        assert (~got["registered"]).nonzero()[0].tolist() == [rc.CLUTTER_IMAGE] and got["seen"][rc.CLUTTER_IMAGE] == 0
    else:
        assert got["registered"].all()
    if name in ("ring_permuted", "ring_clutter"):                            # scene 4: the NaN row of the image left out goes through as it is
        reg = got["registered"]
        P2, X2, info = tracks.adjust_tracks(got, got["P"], case["K"], huber=1.0, iters=3)
        assert P2.shape == got["P"].shape and X2.shape == got["points"].shape and np.isfinite(P2[reg]).all() and np.isnan(P2[~reg]).all()
        assert np.isfinite(X2).all() and np.isfinite(info["history"]).all() and info["history"][-1] <= info["history"][0]


@pytest.mark.gpu
def test_a_model_round_waits_for_the_host_once(hip):
    """One model round of the engine: ONE synchronising read (the head words) under torch's sync debug mode, none inside the library."""
    from sfm_mvs_amd import _lib, register
    case, store, nq, kps = device_scene("ring_permuted")
    eng = register._HipEngine(store, nq, case["pairs"], kps, case["K"], rc.FRAME, 0.70, None, 2, None, 1.0, 2.0, 2.0, 2.0, 10, 8)
    eng.tracks()
    reg = np.ones(8, np.uint8)
    reg[3] = 0
    P = case["P"].copy()
    P[3] = 0.0
    eng.round(reg, P)                                                        # warm: the pinned host pool, the workspaces
    torch.cuda.synchronize()
    lib0 = int(_lib.lib().sfm_host_sync_count())
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            model = eng.round(reg, P)
            X, uv = eng.correspondences(3, int(model["seen"][3]))
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    syncs = [str(w.message) for w in caught if "synchroniz" in str(w.message).lower()]
    assert len(syncs) == 1, syncs
    assert int(_lib.lib().sfm_host_sync_count()) == lib0
    assert model["points"] == 400 and model["seen"].tolist() == [400] * 8 and tuple(X.shape) == (400, 3) and tuple(uv.shape) == (400, 2)


@pytest.mark.gpu
def test_run_tracks_returns_what_it_returned(hip):
    from sfm_mvs_amd import tracks
    case, store, nq, kps = device_scene("ring")
    got = tracks.run_tracks(store, nq, case["pairs"], kps, case["P"], max_reproj=2.0)
    want = nt.run(case["store"], case["nq"], case["pairs"], case["img_off"], case["kp"], case["P"], max_reproj=2.0)
    for key in ("counts", "points", "obs", "cam_idx", "pt_idx", "track_len"):
        assert np.array_equal(np.ascontiguousarray(got[key]).view(np.uint8).ravel(), np.ascontiguousarray(want[key]).astype(got[key].dtype).view(np.uint8).ravel()), key
    assert sorted(got) == ["cam_idx", "counts", "obs", "points", "pt_idx", "status", "track_len"]


@pytest.mark.gpu
def test_a_short_fixed_seed_fuzz_run_finds_no_mismatch(hip):
    counts, bad, dt = fg.run(10.0, 6666)
    print(f"fuzz_tracks_register: seed 6666, {sum(counts.values())} cases {counts}, {bad} mismatches, {dt:.0f} s")
    assert bad == 0 and all(c > 0 for c in counts.values()), counts


@pytest.mark.gpu
def test_committed_fuzz_logs_are_clean_and_name_this_code(hip):
    """profiles/tracks_register_fuzz_seed*.log: no mismatch, and run on the code of csrc/tracks_register.hip and csrc/common.h that the
    loaded library was built from (scripts/knn_code_hash.py: comments and whitespace do not count)."""
    import glob
    import re
    from sfm_mvs_amd import _lib
    have = _lib.code_hashes_of_binary()
    logs = sorted(glob.glob(os.path.join(ROOT, "profiles", "tracks_register_fuzz_seed*.log")))
    assert len(logs) >= 2, logs
    total = 0
    for path in logs:
        text = open(path).read()
        m = re.search(r"fuzz_tracks_register: seed \d+, (\d+) cases .*?, (\d+) mismatches", text)
        assert m and int(m.group(2)) == 0, f"{path}: no clean summary line"
        ids = re.findall(r"sfm_build_id (knn\.hip:\S+(?: \S+:\S+)*)", text)
        assert ids, f"{path} does not name the build it ran on"
        logged = dict(tok.split(":", 1) for tok in ids[-1].split() if ":" in tok)
        for name in ("tracks_register.hip", "common.h"):
            assert logged.get(name) == have[name], f"{path} was produced by another csrc/{name} than the loaded binary's"
        total += int(m.group(1))
    assert total >= FUZZ_FLOOR, total
