"""sfm_mvs_patchmatch on the device (mvs.patchmatch_refine, run_mvs(refine=...)): state (as int32 views), depth, cost and normals equal to
the float32 restatement tests/np_mvs_patchmatch.py bit for bit — a NaN equals a NaN, as in tests/parity_cases.py — on every frame shape,
parameter and start the header admits, written into sentinel-padded buffers; no host wait; and the end-to-end maps held to the bars of
tests/golden/mvs_patchmatch_calibration.json (docs/mvs.md §9)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

import fuzz_mvs_patchmatch as fz  # noqa: E402
import mvs_patchmatch_cases as cases  # noqa: E402
import parity_cases as pc  # noqa: E402
from fuzz_mvs import IDENTITY  # noqa: E402
from test_mvs_patchmatch_cpu import bars, default_row, meets  # noqa: E402

F = np.float32
FUZZ_FLOOR = 1000            # a tenth of the 10768 cases the two committed logs hold, rounded down to one figure (docs/mvs.md §9)


def shifted(w, h, nsrc, seed):
    """A texture and `nsrc` copies shifted by whole pixels under near-identity matrices -> (ref, srcs, mv); planes 0.1 .. 0.5."""
    rng = np.random.default_rng(seed)
    pad = 3
    big = pc.texture(h + 2 * pad, w + 2 * pad, seed)
    ref = np.ascontiguousarray(big[pad:pad + h, pad:pad + w])
    srcs, mv = [], np.tile(IDENTITY, (nsrc, 1))
    for s in range(nsrc):
        sx, sy = (int(v) for v in rng.integers(-pad, pad + 1, 2))
        srcs.append(np.ascontiguousarray(big[pad - sy:pad - sy + h, pad - sx:pad - sx + w]))
        mv[s, 9:11] = np.array([sx, sy], F) / F(rng.uniform(0.15, 0.45))
        mv[s, :9] += rng.normal(0, 1e-4, 9).astype(F)
    return ref, srcs, np.ascontiguousarray(mv, F)


def crop_case(nsrc, w=40, h=33):
    """A crop of the rendered 9-view scene with its real matrices -> (ref, srcs, mv, qmin, qmax, slope_step, nmat, truth)."""
    from sfm_mvs_amd import mvs
    grays, K, P, gt, _ = pc.scene()
    g, Kc, Pc = pc.crop(grays, K, P, 50, 30, w, h)
    nb = mvs.neighbours(4, 9, nsrc)
    return (g[4], [g[v] for v in nb], mvs.sweep_matrices(Kc, Pc[4], Pc[nb]), float(F(1 / 9.0)), float(F(1 / 2.0)), 1.0 / Kc[0, 0],
            mvs.normal_matrix(Kc, Pc[4]), gt[4][30:30 + h, 50:50 + w].astype(F))


def agree(ref, srcs, mv, qmin=0.1, qmax=0.5, r=2, topk=1, var_min=50.0, cost_max=0.5, depth_init=None, iters=2, far=1, depth_step=0.1,
          slope_step=0.01, seed=0, nmat=None):
    want, bad = fz.patchmatch_both(ref, srcs, mv, qmin, qmax, r, topk, var_min, cost_max, depth_init, iters, far, depth_step, slope_step, seed, nmat)
    assert bad is None, bad
    return want


NMAT = np.array([0.9, 0.1, -0.2, -0.1, 0.8, 0.3, 0.2, -0.3, -1.0], F)


@pytest.mark.gpu
@pytest.mark.parametrize("r", [1, 4])
@pytest.mark.parametrize("shape", ["d x d", "d x 40", "15 x 15", "16 x 16", "17 x 33", "160 x 16", "4099 x d", "33 x 17"])
def test_parity_on_frame_shapes(hip, shape, r):
    """Tile edges of both kernels (16 and 32 wide), both row parities of the colouring, a single interior pixel, row or column."""
    d = 2 * r + 1
    w, h = (int(t) if t != "d" else d for t in shape.split(" x "))
    ref, srcs, mv = shifted(w, h, 2, 100 + w + r)
    start = np.random.default_rng(w * h).uniform(1.5, 12.0, (h, w)).astype(F)          # partly outside 2 .. 10
    state = agree(ref, srcs, mv, r=r, topk=2, depth_init=start, iters=2, far=1, seed=w + 7 * h, nmat=NMAT)[0]
    if w >= 15 and h >= 15:
        assert np.any(state[..., 1] != 0)                       # slanted planes were accepted: the case is no fixed point of the init


@pytest.mark.gpu
def test_a_frame_too_narrow_for_the_far_neighbours(hip):
    for w, h in ((3, 12), (12, 3), (5, 5)):
        ref, srcs, mv = shifted(w, h, 2, 7)
        agree(ref, srcs, mv, r=1, topk=1, iters=3, far=1, seed=3, nmat=NMAT)


@pytest.mark.gpu
@pytest.mark.parametrize("nsrc", [1, 8])
def test_parity_over_sources_topk_iterations_and_far(hip, nsrc):
    ref, srcs, mv, qmin, qmax, slope, nmat, truth = crop_case(nsrc, 28, 25)
    noisy = (truth * (1 + 0.03 * np.random.default_rng(1).standard_normal(truth.shape))).astype(F)
    for topk in sorted({1, min(2, nsrc), nsrc}):
        for iters, far in ((0, 1), (1, 0), (3, 1)):
            agree(ref, srcs, mv, qmin, qmax, r=2, topk=topk, depth_init=noisy, iters=iters, far=far, slope_step=slope, seed=11 * iters + far, nmat=nmat)


@pytest.mark.gpu
def test_parity_over_the_starts(hip):
    ref, srcs, mv, qmin, qmax, slope, nmat, truth = crop_case(3)
    rng = np.random.default_rng(2)
    outside = truth.copy()
    outside[::2] = F(1.2)                   # nearer than 1/qmax = 2
    outside[1::4] = F(40.0)                 # farther than 1/qmin = 9
    for start in (None, np.zeros_like(truth), pc.plant_specials(truth, rng, fraction=0.05), outside):
        st = agree(ref, srcs, mv, qmin, qmax, r=3, topk=2, depth_init=start, iters=1, slope_step=slope, seed=4, nmat=nmat)[0]
    assert np.all((st[..., 0] >= F(qmin)) & (st[..., 0] <= F(qmax) * F(1.000001)))
    none = agree(ref, srcs, mv, qmin, qmax, r=3, topk=2, depth_init=None, iters=0, seed=4)[0]
    zero = agree(ref, srcs, mv, qmin, qmax, r=3, topk=2, depth_init=np.zeros_like(truth), iters=0, seed=4)[0]
    assert pc.same(none, zero)                                  # no start and a start without a depth: every pixel hashed


@pytest.mark.gpu
def test_degenerate_inputs(hip):
    ref, srcs, mv, qmin, qmax, slope, nmat, truth = crop_case(2)
    flat = np.full(ref.shape, 128, np.uint8)
    for a, b in ((flat, srcs), (ref, [flat, flat]), (flat, [flat, flat])):
        state, depth, cost, normal = agree(a, b, mv, qmin, qmax, r=2, topk=2, cost_max=2.5, depth_init=truth, iters=2, slope_step=slope, seed=1, nmat=nmat)
        init = agree(a, b, mv, qmin, qmax, r=2, topk=2, cost_max=2.5, depth_init=truth, iters=0, slope_step=slope, seed=1)[0]
        assert np.all(cost == 2) and pc.same(state, init)       # nothing beats 2: the state is the init
    behind = -mv
    state, depth, cost, _ = agree(ref, srcs, behind, qmin, qmax, r=2, topk=1, depth_init=truth, iters=1, slope_step=slope, seed=1, nmat=nmat)
    assert np.all(cost == 2) and np.all(depth == 0)
    one_behind = mv.copy()
    one_behind[1] = -one_behind[1]
    agree(ref, srcs, one_behind, qmin, qmax, r=2, topk=2, depth_init=truth, iters=1, slope_step=slope, seed=1, nmat=nmat)
    for cost_max in (-1.0, 2.0, float("inf")):
        _, depth, cost, normal = agree(ref, srcs, mv, qmin, qmax, r=2, topk=2, cost_max=cost_max, depth_init=truth, iters=1, slope_step=slope, seed=1,
                                       nmat=nmat)
        interior = np.zeros(ref.shape, bool)
        interior[2:-2, 2:-2] = True
        if cost_max < 0:
            assert np.all(depth == 0) and np.all(normal == 0)
        elif cost_max == 2.0:
            assert np.array_equal(depth > 0, interior & (cost < 2))
        else:
            assert np.array_equal(depth > 0, interior)
    agree(ref, srcs, mv, qmin, qmin, r=2, topk=2, depth_init=truth, iters=2, slope_step=slope, seed=1, nmat=nmat)      # one admissible depth


@pytest.mark.gpu
def test_the_hash_wraps_on_the_device_as_in_the_restatement(hip):
    w, h = 4099, 7
    assert (w * h - 1) * 0x9E3779B9 >= 1 << 32 and 2 * 0x85EBCA6B >= 1 << 32 and 6 * 0xC2B2AE35 >= 1 << 32
    ref, srcs, mv = shifted(w, h, 1, 5)
    agree(ref, srcs, mv, r=3, topk=1, depth_init=None, iters=3, far=1, depth_step=0.2, seed=0xFFFFFFFF, nmat=NMAT)
    ref, srcs, mv = shifted(14, 11, 2, 6)
    agree(ref, srcs, mv, r=2, topk=2, depth_init=None, iters=16, far=1, depth_step=0.2, seed=0x80000000, nmat=NMAT)     # the last admitted iteration


@pytest.mark.gpu
def test_a_second_run_gives_the_same_bits_and_the_wrapper_is_the_raw_call(hip):
    from sfm_mvs_amd import mvs
    ref, srcs, mv, qmin, qmax, slope, nmat, truth = crop_case(4)
    K = np.array([[1 / slope, 0, 0], [0, 1 / slope, 0], [0, 0, 1.0]])
    args = (pc.up(ref), [pc.up(s) for s in srcs], mv, qmin, qmax)
    kw = dict(depth_init=pc.up(truth), K=K, P_ref=np.hstack([K, np.zeros((3, 1))]), radius=2, topk=2, var_min=50.0, cost_max=0.5, seed=77)
    a = mvs.patchmatch_refine(*args, **kw)
    b = mvs.patchmatch_refine(*args, **kw)
    assert all(pc.same(x, y) for x, y in zip(a, b))
    want = agree(ref, srcs, mv, qmin, qmax, r=2, topk=2, depth_init=truth, iters=mvs.PM_ITERS, far=int(mvs.PM_FAR), depth_step=mvs.PM_DEPTH_STEP,
                 slope_step=slope, seed=77, nmat=mvs.normal_matrix(K, kw["P_ref"]))
    depth, cost, normal, state = a
    assert pc.same(state, want[0]) and pc.same(depth, want[1]) and pc.same(cost, want[2]) and pc.same(normal, want[3])
    c = mvs.patchmatch_refine(*args, **dict(kw, normals=False, K=None, P_ref=None, slope_step=slope))
    assert c[2] is None and pc.same(c[3], state)                # the normals change no other output


@pytest.mark.gpu
def test_patchmatch_refine_never_waits_for_the_host(hip):
    from sfm_mvs_amd import _lib, mvs
    ref, srcs, mv, qmin, qmax, slope, nmat, truth = crop_case(4)
    K = np.array([[1 / slope, 0, 0], [0, 1 / slope, 0], [0, 0, 1.0]])
    args = (pc.up(ref), [pc.up(s) for s in srcs], mv, qmin, qmax, pc.up(truth), K, np.hstack([K, np.zeros((3, 1))]))
    mvs.patchmatch_refine(*args)
    torch.cuda.synchronize()
    lib0 = int(_lib.lib().sfm_host_sync_count())
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = mvs.patchmatch_refine(*args)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert int(_lib.lib().sfm_host_sync_count()) == lib0 and out[0].shape == ref.shape


def _scene_inputs(name):
    sc = cases.scene(name)
    return sc, np.hstack([sc["K"].ravel()] + [p.ravel() for p in sc["P"]])


@pytest.mark.gpu
def test_run_mvs_refine_waits_for_the_host_twice_and_none_is_the_plain_call(hip):
    import warnings
    from sfm_mvs_amd import _lib, mvs
    sc, posearr = _scene_inputs("quads")
    opts = dict(ndepth=16, refine=dict(iters=1))
    mvs.run_mvs(sc["images"], sc["K"], posearr, sc["cloud"], **opts)
    torch.cuda.synchronize()
    lib0 = int(_lib.lib().sfm_host_sync_count())
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            out = mvs.run_mvs(sc["images"], sc["K"], posearr, sc["cloud"], **opts)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    syncs = [str(w.message) for w in caught if "synchroniz" in str(w.message).lower()]
    assert len(syncs) == 2, syncs
    assert int(_lib.lib().sfm_host_sync_count()) == lib0
    m = len(out["points"])
    assert m > 0 and out["normals"].shape == (m, 3) and out["normals"].dtype == np.float64 and out["colors"].shape == (m, 3)
    assert np.allclose(np.linalg.norm(out["normals"], axis=1), 1.0, atol=1e-5)
    assert len(out["normal_maps"]) == 5 and all(n.shape == (cases.H, cases.W, 3) for n in out["normal_maps"])
    plain = mvs.run_mvs(sc["images"], sc["K"], posearr, sc["cloud"], ndepth=16)
    none = mvs.run_mvs(sc["images"], sc["K"], posearr, sc["cloud"], ndepth=16, refine=None)
    assert all(pc.same(a, b) for a, b in zip(plain["depths"], none["depths"])) and "normals" not in none and "normal_maps" not in none
    assert np.array_equal(plain["points"], none["points"]) and np.array_equal(plain["colors"], none["colors"])
    assert any(not pc.same(a, b) for a, b in zip(plain["depths"], out["depths"]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["quads", "slant"])
def test_run_mvs_refine_meets_the_calibration_bars(hip, name):
    """run_mvs(refine=True) at its defaults: the middle view's map and normals are the restatement's of the calibration (same sweep, same
    planes, seed 0), so they are held to the committed bars and to the two fixed conditions of docs/mvs.md §9."""
    from sfm_mvs_amd import mvs
    sc, posearr = _scene_inputs(name)
    out = mvs.run_mvs(sc["images"], sc["K"], posearr, sc["cloud"], refine=True)
    plain = mvs.run_mvs(sc["images"], sc["K"], posearr, sc["cloud"])
    assert pc.same(plain["depths"][cases.VIEW], cases.sweep_depth(name))
    doc = cases.golden()
    fig = cases.figures(name, out["depths"][cases.VIEW].cpu().numpy(), out["normal_maps"][cases.VIEW].cpu().numpy())
    print(name, fig)
    assert meets(fig, bars(default_row(doc, name, 0))), fig
    sweep_fig = cases.figures(name, plain["depths"][cases.VIEW].cpu().numpy())
    if name == "quads":
        assert fig["valid"] >= 0.95 and fig["within_1pct"] >= 0.85
    else:
        assert fig["floor_within_025pct"] > sweep_fig["floor_within_025pct"]
    assert len(out["points"]) > 5000 and out["normals"].shape == out["points"].shape


# ---- fuzzing ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_a_short_fixed_seed_fuzz_run(hip):
    count, bad, dt = fz.run(4.0, 20265, log=print)
    print(f"fuzz_mvs_patchmatch: {count} cases in {dt:.1f} s")
    assert bad == 0 and count >= 3


@pytest.mark.gpu
def test_committed_fuzz_logs_are_clean_and_of_this_code(hip):
    """profiles/mvs_patchmatch_fuzz_seed*.log: no mismatch, and run on the code of csrc/mvs_patchmatch.hip and csrc/common.h that the
    loaded library was built from (scripts/knn_code_hash.py: comments and whitespace do not count)."""
    import glob
    import re
    from sfm_mvs_amd import _lib
    have = _lib.code_hashes_of_binary()
    logs = sorted(glob.glob(os.path.join(ROOT, "profiles", "mvs_patchmatch_fuzz_seed*.log")))
    assert len(logs) >= 2, logs
    total = 0
    for path in logs:
        text = open(path).read()
        m = re.search(r"fuzz_mvs_patchmatch: seed \d+, (\d+) cases, (\d+) mismatches", text)
        assert m and int(m.group(2)) == 0, f"{path}: no clean summary line"
        ids = re.findall(r"sfm_build_id (knn\.hip:\S+(?: \S+:\S+)*)", text)
        assert ids, f"{path} does not name the build it ran on"
        logged = dict(tok.split(":", 1) for tok in ids[-1].split() if ":" in tok)
        for name in ("mvs_patchmatch.hip", "common.h"):
            assert logged.get(name) == have[name], f"{path} was produced by another csrc/{name} than the loaded binary's"
        total += int(m.group(1))
    assert total >= FUZZ_FLOOR, total
