"""csrc/triangulate.hip (sfm_triangulate_dlt, sfm_triangulate_matches_batch, sfm_recover_pose_score) and csrc/assoc.hip
(sfm_common_points, sfm_mask_indices, sfm_knn_merge_top2) on every launch path, against the float64 reference of
np_triangulate.py (LAPACK's SVD: independent of the Jacobi sweeps the kernels share with the C oracle), the oracle and NumPy.
The cases, the plan each lands on and the one assumption they make are in tri_cases.py; test_tri_cases_cpu.py proves the plans
and that the oracle alone holds the bars.  Every test prints its largest error in units of 2^-24 before it asserts."""
import ctypes

import numpy as np
import pytest
import torch

import np_triangulate as T
import tri_cases as C
from datagen import load_pose_csv

pytestmark = pytest.mark.gpu

REDO_MARK = 0x7FC0DEAD
MODES4 = (False, True, "fast", "guarded")


def bits(t):
    return t.view(torch.int32)


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------- triangulation below the list threshold
@pytest.mark.parametrize("n", C.SIZES_SMALL)
def test_small_sizes_on_every_layout_and_mode(hip, oracle, n):
    """Scan fix-up (no reject list), one point per lane: every size x layout x normalise_w, rows 4 (and 6 for the faithful
    forms).  All layouts give the same bits; guarded == faithful in every bit on every geometry; where the system has one
    null vector the faithful and fast forms are within the derived bars of the float64 reference and the faithful form is
    bit-identical to the oracle on >= 99 % of the points.
    Measured (units of 2^-24): faithful <= 2.14 normalised, 0.50 raw; "fast" <= 2.09.  Before triangulate_kernel sent its
    ill-conditioned lanes (16 sens > 2^-26 |w|) to the Jacobi sweeps, "fast" reached 27.74 on the baseline pair at n >= 2047."""
    worst =dict(normalised=0.0, raw=0.0, fast=0.0)
    for geometry in C.geometries_of(n):
        P1, P2, x1, x2 = C.pair(geometry, n)
        views = {name: C.layout_views(name, x1, x2, "cuda") for name in C.LAYOUTS}
        for name, packed in C.LAYOUTS.items():
            if n > 1:
                assert C.plan(n, *C.wrapper_strides(*views[name]))["packed"] == packed, name
        out = {}
        for rows, modes in ((4, MODES4), (6, (False, True))):
            for mode in modes:
                base = hip.triangulate(P1, P2, *views["transposed"], rows=rows, normalise_w=mode)
                assert tuple(base.shape) == (4, n)
                for name in C.LAYOUTS:
                    other = hip.triangulate(P1, P2, *views[name], rows=rows, normalise_w=mode)
                    assert torch.equal(bits(other), bits(base)), (geometry, rows, mode, name)
                out[rows, mode] = base
        assert torch.equal(bits(out[4, "guarded"]), bits(out[4, True])), geometry
        if not C.GEOMETRIES[geometry]:
            continue
        refs = {}
        for rows in (4, 6):
            unit, normalised, _ = refs[rows] = T.triangulate(P1, P2, x1, x2, rows)
            got, raw = out[rows, True].cpu().numpy(), out[rows, False].cpu().numpy()
            en, er = T.normalised_error(got, normalised).max(), T.raw_error(raw, unit).max()
            worst["normalised"], worst["raw"] = max(worst["normalised"], en), max(worst["raw"], er)
            print(f"n {n} {geometry} rows {rows}: normalised {en:.3f} raw {er:.3f}")
            assert en <= T.BAR_NORMALISED and er <= T.BAR_RAW, (geometry, rows, en, er)
            assert np.all(got[3] == 1.0)
            want = oracle.triangulate(P1, P2, x1.T, x2.T, rows=rows, normalise_w=True)
            want_raw = oracle.triangulate(P1, P2, x1.T, x2.T, rows=rows, normalise_w=False)
            assert np.allclose(got, want, rtol=1e-6, atol=1e-7) and np.allclose(np.abs(raw), np.abs(want_raw), rtol=1e-6, atol=1e-9)
            assert (got == want).all(0).mean() >= 0.99, (geometry, rows, (got == want).all(0).mean())
        ef = T.normalised_error(out[4, "fast"].cpu().numpy(), refs[4][1]).max()
        worst["fast"] = max(worst["fast"], ef)
        print(f"n {n} {geometry}: fast {ef:.3f}")
        assert ef <= T.BAR_NORMALISED, (geometry, ef)
    print(f"n {n}: worst {worst}")


# ---------------------------------------------------------------- the guard's empirical bound
@pytest.mark.parametrize("sigma", C.GUARD_SWEEP_SIGMAS)
def test_guard_holds_on_all_56_consecutive_pairs(hip, sigma):
    """kSensFactor = 16 is calibrated, not derived: every consecutive pose.csv pair at 4096 points, guarded == faithful."""
    bad = []
    for k in range(56):
        P1, P2, x1, x2 = C.guard_sweep_pair(k, sigma)
        a, b = cu(x1).t(), cu(x2).t()
        g = hip.triangulate(P1, P2, a, b, normalise_w="guarded")
        f = hip.triangulate(P1, P2, a, b, normalise_w=True)
        if not torch.equal(bits(g), bits(f)):
            idx = torch.nonzero((bits(g) != bits(f)).any(0)).flatten().cpu().tolist()
            bad.append((k, idx[:8], x1[idx[:8]].tolist(), x2[idx[:8]].tolist()))
    assert not bad, bad


# ---------------------------------------------------------------- list mode
def _guarded_equals_faithful(hip, P1, P2, x1, x2, planted=None):
    """x1, x2: (n, 2) device tensors.  Packed and strided readers; returns the faithful result."""
    n = x1.shape[0]
    keep = torch.ones(n, dtype=torch.bool, device=x1.device)
    if planted is not None and len(planted):
        keep[planted] = False
    faithful = None
    for name, (a, b) in (("packed", (x1.t(), x2.t())), ("strided", (x1.t().contiguous(), x2.t().contiguous()))):
        assert C.plan(n, *C.wrapper_strides(a, b))["packed"] == (name == "packed")
        g = hip.triangulate(P1, P2, a, b, normalise_w="guarded")
        f = hip.triangulate(P1, P2, a, b, normalise_w=True)
        assert torch.equal(bits(g)[:, keep], bits(f)[:, keep]), name
        if planted is not None and len(planted):
            assert not torch.isfinite(g[:, planted]).any() and not torch.isfinite(f[:, planted]).any(), name
            assert not (bits(g)[:, planted] == REDO_MARK).any(), name          # redone by the fix-up pass, not left marked
        assert faithful is None or torch.equal(bits(faithful), bits(f))
        faithful = f
    return faithful


@pytest.mark.parametrize("n", C.SIZES_LIST)
def test_list_sizes(hip, n):
    """n >= 2^18: the first pass keeps a compact reject list; at 393 217 a lane walks two points (the prefetch runs)."""
    assert C.plan(n)["list"]
    P1, P2, x1, x2 = C.device_pair(n, seed=n, device="cuda")
    f = _guarded_equals_faithful(hip, P1, P2, x1, x2)
    sel = cu(np.r_[0:2048, n - 2048:n])                                  # the float64 bar on both ends of the grid
    ref = T.triangulate(P1, P2, x1[sel].cpu().numpy(), x2[sel].cpu().numpy(), 4)[1]
    e = T.normalised_error(f[:, sel].cpu().numpy(), ref).max()
    print(f"n {n}: normalised {e:.3f}")
    assert e <= T.BAR_NORMALISED


@pytest.mark.parametrize("name", list(C.REJECT_CASES))
def test_reject_plans(hip, name):
    """list / global overflow / workgroup-queue overflow (the `total > kQ` branch and the `at < kQ` guard), by planted NaN."""
    n, which, geometry, want, why = C.REJECT_CASES[name]
    planted = C.planted_rejects(n, which)
    assert C.reject_plan(n, planted) == (want, why)
    P1, P2, x1, x2 = C.device_pair(n, seed=len(name), device="cuda", geometry=geometry)
    pl = cu(planted)
    x1[pl, 0] = float("nan")
    f = _guarded_equals_faithful(hip, P1, P2, x1, x2, pl)
    assert int(torch.isfinite(f).all(0).sum()) == n - len(planted)


def test_fixup_two_rounds(hip):
    """1024 * 20 480 + 4097 points, all rejected (identical cameras and rays): the scan pass's grid stride takes a second
    round.  Compared on the device."""
    n = C.FIXUP_TWO_ROUNDS_N
    assert C.plan(n)["rounds2"] == 2
    _, P = load_pose_csv()
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.rand((n, 2), dtype=torch.float32, device="cuda", generator=g) * torch.tensor([968.0, 648.0], device="cuda")
    a = x.t()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    ev[0].record()
    guarded = hip.triangulate(P[1], P[1], a, a, normalise_w="guarded")
    ev[1].record()
    faithful = hip.triangulate(P[1], P[1], a, a, normalise_w=True)
    ev[2].record()
    torch.cuda.synchronize()
    print(f"fixup_two_rounds: guarded {ev[0].elapsed_time(ev[1]):.1f} ms, faithful {ev[1].elapsed_time(ev[2]):.1f} ms")
    assert torch.equal(bits(guarded), bits(faithful))
    assert not (bits(guarded) == REDO_MARK).any()


# ---------------------------------------------------------------- sfm_triangulate_matches_batch
def _lowe(idx, dist, ratio):
    return np.flatnonzero((idx[:, 1] >= 0) & (dist[:, 0].astype(np.float64) < ratio * dist[:, 1].astype(np.float64)))


def _knn_block(idx, dist, cap):
    blk = np.full((2, cap, 2), -3, np.int32)
    blk[0, :len(idx)], blk[1, :len(idx)] = idx, dist.view(np.int32)
    return cu(blk)


def test_matches_batch_past_256_blocks(hip):
    """cap = nq = 257 * 1024 + 3: 258 workgroups, so the 256-strided prefix loop over block_count takes a second step for
    workgroups 256 and 257.  Survivors mostly in blocks 0, 255, 256 and 257."""
    _, P = load_pose_csv()
    rng = np.random.default_rng(8)
    nq = cap = 257 * 1024 + 3
    blk_of = np.arange(nq) // C.TM_CHUNK
    dense = np.isin(blk_of, (0, 255, 256, 257))
    passes = rng.random(nq) < np.where(dense, 0.4, 0.004)
    d1 = rng.uniform(50, 400, nq).astype(np.float32)
    d0 = (d1 * np.where(passes, rng.uniform(0.2, 0.65, nq), rng.uniform(0.75, 1.0, nq))).astype(np.float32)
    X = np.stack([rng.uniform(-6.3, 3.6, nq), rng.uniform(-2.6, 5.0, nq), rng.uniform(3.2, 13.0, nq), np.ones(nq)], 0)
    kps = []
    for Pm in (P[1], P[2]):
        x = Pm @ X
        kps.append(((x[:2] / x[2]).T + rng.normal(0, 0.3, (nq, 2))).astype(np.float32))
    perm = rng.permutation(nq).astype(np.int32)
    kp1 = np.empty_like(kps[1])
    kp1[perm] = kps[1]                                                   # query q matches train row perm[q]
    idx = np.stack([perm, rng.integers(0, nq, nq).astype(np.int32)], 1)
    idx[5, 1] = -1
    dist = np.stack([d0, d1], 1)
    surv = _lowe(idx, dist, 0.70)
    per_block = np.bincount(blk_of[surv], minlength=258)
    assert all(per_block[b] > 0 for b in (0, 255, 256, 257)) and per_block[257] <= 3
    out = torch.full((4 * cap + 1,), 7.0, dtype=torch.float32, device="cuda")
    pts, cnt = out[:4 * cap].view(4, cap), out[4 * cap:].view(torch.int32)
    dk0, dk1 = cu(kps[0]), cu(kp1)
    hip.triangulate_matches_batch([_knn_block(idx, dist, cap)], [nq], [dk0], [dk1], [P[1]], [P[2]], [pts], [cnt], ratio=0.70)
    m = len(surv)
    assert int(cnt.item()) == m
    assert float(pts[:, m:].abs().sum()) == 0.0
    want = hip.triangulate(P[1], P[2], dk0[cu(surv)].t(), dk1[cu(idx[surv, 0]).long()].t(), normalise_w=True)
    assert torch.equal(bits(pts[:, :m]), bits(want))                     # column order and every point, bit for bit
    e = T.normalised_error(want[:, :4096].cpu().numpy(), T.triangulate(P[1], P[2], kps[0][surv[:4096]], kp1[idx[surv[:4096], 0]], 4)[1]).max()
    print(f"matches_batch: normalised {e:.3f}")
    assert e <= T.BAR_NORMALISED


@pytest.mark.parametrize("cap", [1, 1023, 1024, 1025])
def test_matches_batch_at_the_chunk_edges(hip, cap):
    """Batch of 8 with pair sizes 0, 1 and cap around one workgroup's 1024 queries."""
    _, P = load_pose_csv()
    rng = np.random.default_rng(cap)
    sizes = [0, 1, cap, cap, 1, 0, cap, min(cap, 700)]
    nt = 1500
    out = torch.full((8, 4 * cap + 1), 7.0, dtype=torch.float32, device="cuda")
    pts = [out[b, :4 * cap].view(4, cap) for b in range(8)]
    cnt = [out[b, 4 * cap:].view(torch.int32) for b in range(8)]
    blocks, kp0s, kp1s, cases = [], [], [], []
    for b, nq in enumerate(sizes):
        idx = np.stack([rng.integers(0, nt, nq), rng.integers(0, nt, nq)], 1).astype(np.int32)
        d1 = rng.uniform(50, 400, nq).astype(np.float32)
        d0 = (d1 * rng.uniform(0.3, 1.0, nq)).astype(np.float32)
        if b == 3:
            d0[:] = 0.0                                                   # every query survives: a full block
        if b == 6:
            d0[:] = d1                                                    # none does
        dist = np.stack([d0, d1], 1)
        X = np.stack([rng.uniform(-6.3, 3.6, nt), rng.uniform(-2.6, 5.0, nt), rng.uniform(3.2, 13.0, nt), np.ones(nt)], 0)
        kp = []
        for Pm in (P[2 * b], P[2 * b + 1]):
            x = Pm @ X
            kp.append(((x[:2] / x[2]).T + rng.normal(0, 0.3, (nt, 2))).astype(np.float32))
        kp0 = kp[0][idx[:, 0]] if nq else np.zeros((1, 2), np.float32)    # query q looks at the point of its first neighbour
        blocks.append(_knn_block(idx, dist, cap)); kp0s.append(cu(kp0)); kp1s.append(cu(kp[1]))
        cases.append((idx, _lowe(idx, dist, 0.70)))
    hip.triangulate_matches_batch(blocks, sizes, kp0s, kp1s, [P[2 * b] for b in range(8)], [P[2 * b + 1] for b in range(8)], pts, cnt, ratio=0.70)
    assert len(cases[3][1]) == cap and len(cases[6][1]) == 0
    for b, (idx, surv) in enumerate(cases):
        m = len(surv)
        assert int(cnt[b].item()) == m, b
        assert float(pts[b][:, m:].abs().sum()) == 0.0, b
        if m:
            want = hip.triangulate(P[2 * b], P[2 * b + 1], kp0s[b][cu(surv)].t(), kp1s[b][cu(idx[surv, 0]).long()].t(), normalise_w=True)
            assert torch.equal(bits(pts[b][:, :m]), bits(want)), b


# ---------------------------------------------------------------- sfm_recover_pose_score, directly
@pytest.mark.parametrize("rows", [4, 6])
@pytest.mark.parametrize("n", C.POSE_N)
def test_recover_pose_score_direct(hip, oracle, n, rows):
    """Every candidate count, mask given and null, counts pre-filled with garbage: masks and counts equal the oracle's bit for
    bit and the float64 reference on the decidable points."""
    from sfm_mvs_amd import _lib
    lib = _lib.lib()
    cands, x1n, x2n = C.pose_case()[:3]
    d1, d2 = cu(x1n[:n].copy()), cu(x2n[:n].copy())
    for h in range(1, 5):
        Ph = np.ascontiguousarray(cands[:h], np.float64)
        want_counts, want_mask = oracle.recover_pose_score(Ph, x1n[:n], x2n[:n], C.POSE_DIST, rows)
        ref, decidable = T.cheirality(Ph, x1n[:n], x2n[:n], C.POSE_DIST, rows)
        assert (~decidable).sum() <= 1e-3 * decidable.size
        for with_mask in (True, False):
            counts = torch.full((4,), -12345, dtype=torch.int32, device="cuda")
            mask = torch.full((h, n), 77, dtype=torch.uint8, device="cuda") if with_mask else None
            _lib.check(lib.sfm_recover_pose_score(Ph.ctypes.data_as(ctypes.c_void_p), h, _lib.ptr(d1), _lib.ptr(d2), n, C.POSE_DIST, rows,
                                                  _lib.ptr(counts), _lib.ptr(mask), _lib.stream_ptr()), "sfm_recover_pose_score")
            got_counts = counts.cpu().numpy()
            assert np.array_equal(got_counts[:h], want_counts) and (got_counts[h:] == -12345).all(), (h, with_mask)
            if with_mask:
                got = mask.cpu().numpy()
                assert np.array_equal(got, want_mask), h
                assert np.array_equal((got > 0)[decidable], ref[decidable]), h
                assert np.array_equal(got_counts[:h], got.astype(np.int64).sum(1) // 255)


# ---------------------------------------------------------------- sfm_mask_indices
def test_mask_indices_past_256_blocks(hip):
    """n = 258 * 1024 + 5: 259 workgroups, the prefix loop of workgroups 257 and 258 takes a second step."""
    n = 258 * 1024 + 5
    rng = np.random.default_rng(12)
    first_256 = np.arange(n) < 256 * C.MASK_BLOCK
    masks = [rng.choice(np.array([0, 0, 1, 255, 7], np.uint8), n)]
    masks.append(np.where(first_256, 0, masks[0]).astype(np.uint8))       # blocks 0 .. 255 all zero, passes only after them
    masks.append(np.where(first_256, masks[0], 0).astype(np.uint8))       # ... and the reverse
    masks.append(np.ones(n, np.uint8))
    for k, m in enumerate(masks):
        d = cu(m)
        assert np.array_equal(hip.mask_indices(d).cpu().numpy(), np.flatnonzero(m == 1)), k
        assert np.array_equal(hip.mask_indices(d, nonzero=True).cpu().numpy(), np.flatnonzero(m > 0)), k
    assert len(np.flatnonzero(masks[1] == 1)) > 0 and np.flatnonzero(masks[1] > 0).min() >= 256 * C.MASK_BLOCK


# ---------------------------------------------------------------- sfm_common_points
def _common_points_case(n1, n2, rng):
    """pts2: distinct coordinates (x = 10 + j, y = 5000 + j) with duplicates of earlier rows, a 0.0 and NaN rows; pts1: the
    first 64 rows (one workgroup) copy rows of the FIRST tile of pts2, the others mix copies, x-only and y-only hits, -0.0,
    NaN, rows without a hit and rows with two hits in different lanes of the quad, in either tile."""
    j = np.arange(n2, dtype=np.float32)
    p2 = np.stack([10 + j, 5000 + j], 1).astype(np.float32)
    if n2 > 40:
        p2[30] = p2[12]                                                  # duplicates: the lower index answers
        p2[n2 - 1] = p2[n2 // 2]
        p2[20] = (0.0, 123456.0)
        p2[25] = (np.nan, np.nan)
        p2[26] = (np.nan, 654321.0)
    p1 = np.stack([-1000 - np.arange(n1, dtype=np.float32), -9000 - np.arange(n1, dtype=np.float32)], 1)     # no hit
    if n2 == 0:
        return p1, p2
    for i in range(n1):
        kind = i % 8 if i >= 64 else 0
        src = int(rng.integers(0, min(n2, C.ASSOC_TILE))) if i < 64 else int(rng.integers(0, n2))
        if i < 64 and src in (25, 26):
            src = 0                                                      # (the NaN rows: workgroup 0 must leave after the first tile)
        if kind == 0:
            p1[i] = p2[src]
        elif kind == 1:
            p1[i, 0] = p2[src, 0]                                        # x only
        elif kind == 2:
            p1[i, 1] = p2[src, 1]                                        # y only
        elif kind == 3:
            p1[i] = (np.nan, np.nan)                                     # never a hit
        elif kind == 4:
            other = int(rng.integers(0, n2))
            p1[i] = (p2[src, 0], p2[other, 1])                           # two hits: the lower index wins
        # 5, 6, 7: no hit — the workgroup scans to the end
    if n2 > 40 and n1 > 70:
        p1[65] = (-0.0, -77.0)                                           # -0.0 == 0.0: row 20
        p1[66] = (np.nan, 654321.0)                                      # NaN x never hits, y does: row 26
        p1[67] = (p2[9, 0], p2[7, 1])                                    # lanes 1 and 3 of the quad in the first tile: 7
    if n2 > 1031 and n1 > 70:
        p1[68] = (p2[1030, 0], p2[1027, 1])                              # first hit in the second tile, lanes 2 and 3: 1027
        p1[69] = (p2[1029, 0], p2[5, 1])                                 # hits in both tiles: 5
    return p1, p2


@pytest.mark.parametrize("n1", [0, 1, 63, 64, 65, 1023, 1024, 1025])
def test_common_points_edges(hip, oracle, n1):
    rng = np.random.default_rng(100 + n1)
    for n2 in (0, 1, 1023, 1024, 1025, 2049):
        p1, p2 = _common_points_case(n1, n2, rng)
        tag = np.stack([np.arange(n2), np.arange(n2)], 1).astype(np.float32)
        wi1, wi2, _, kept = oracle.common_points(p1, p2, tag)
        want_keep = np.zeros(n2, bool)
        want_keep[kept.reshape(-1, 2)[:, 0].astype(np.int64)] = True
        with np.errstate(invalid="ignore"):
            hit = (p1[:, None, 0] == p2[None, :, 0]) | (p1[:, None, 1] == p2[None, :, 1])      # NumPy's own statement of it
        rows = np.flatnonzero(hit.any(1))
        assert np.array_equal(wi1, rows) and np.array_equal(wi2, hit[rows].argmax(1) if n2 else rows)
        i1, i2, keep = hip.common_points(cu(p1).reshape(-1, 2), cu(p2).reshape(-1, 2))
        assert np.array_equal(i1.cpu().numpy(), wi1) and np.array_equal(i2.cpu().numpy(), wi2), (n1, n2)
        assert np.array_equal(keep.cpu().numpy()[:n2], want_keep), (n1, n2)
        if n1 > 70 and n2 > 1031:
            got = dict(zip(i1.cpu().tolist(), i2.cpu().tolist()))
            assert got[65] == 20 and got[66] == 26 and got[67] == 7 and got[68] == 1027 and got[69] == 5


# ---------------------------------------------------------------- sfm_knn_merge_top2
@pytest.mark.parametrize("S", [1, 2, 5])
@pytest.mark.parametrize("nq", [1, 255, 256, 257])
def test_knn_merge_on_synthetic_candidates(hip, nq, S):
    """Candidates written by hand (no KNN call): ties across shards with indices in descending shard order, a shard whose
    first slot is missing while its second is valid, queries with one neighbour and with none."""
    rng = np.random.default_rng(10 * nq + S)
    idx = np.empty((S, nq, 2), np.int32)
    for s in range(S):
        base = (S - 1 - s) * 1000                                         # later shards hold LOWER train indices
        a = rng.integers(0, 999, nq)
        idx[s, :, 0], idx[s, :, 1] = base + a, base + a + 1 + rng.integers(0, 999 - a)
    dist = rng.choice(np.array([0.0, 1.5, 1.5, 2.0, 7.25, 300.0], np.float32), (S, nq, 2))    # few values: ties everywhere
    for q in range(nq):
        kind = q % 6
        if kind == 1:
            idx[q % S, q, 0] = -1                                         # first slot missing, second valid
        elif kind == 2:
            dist[:, q, :] = 4.0                                           # all equal: the two lowest indices
        elif kind == 3:
            idx[:, q, :] = -1                                             # no neighbour at all
        elif kind == 4:
            idx[:, q, :] = -1
            idx[S - 1, q, 1] = 5                                          # one neighbour, in a second slot
    cand = np.stack([idx, dist.view(np.int32)], 1)                        # [S][2][nq][2]
    gi, gd = hip.knn_merge_top2(cu(cand))
    want_i = np.full((nq, 2), -1, np.int32)
    want_d = np.zeros((nq, 2), np.float32)
    for q in range(nq):
        ci, cd = idx[:, q, :].ravel(), dist[:, q, :].ravel()
        ok = ci >= 0
        order = np.lexsort((ci[ok], cd[ok]))[:2]                          # by distance, then index
        want_i[q, :len(order)], want_d[q, :len(order)] = ci[ok][order], cd[ok][order]
    assert np.array_equal(gi.cpu().numpy(), want_i)
    assert np.array_equal(gd.cpu().numpy().view(np.uint32), want_d.view(np.uint32))
