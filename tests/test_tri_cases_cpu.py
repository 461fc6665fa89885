"""CPU-only proofs behind test_gpu_tri_paths.py: every case of tri_cases.py lands on the launch plan claimed for it (by the plan
of sfm_triangulate_dlt restated there, whose constants are read back from the .hip text), and the C oracle — the same Jacobi
algorithm as the kernels — stays inside the derived bars of the float64 reference np_triangulate.py on the committed inputs, so
the bars stand on the reference and not on the kernel.  Measured here: normalised <= 2.14 (rows 6, baseline pair), raw <= 0.50
units of 2^-24."""
import numpy as np
import pytest

import np_triangulate as T
import tri_cases as C


def test_restated_constants_are_the_sources():
    src = C.source_constants()
    for k, v in src.items():
        assert getattr(C, k) == v, k
    assert C.fixup_chunk(1) == 2048 and C.fixup_chunk(512 * 2048) == 2048 and C.fixup_chunk(512 * 2048 + 1) == 4096
    assert C.fixup_chunk(10 ** 9) == 20480


def test_sizes_land_on_the_claimed_plans():
    for n in C.SIZES_SMALL:
        p = C.plan(n)
        assert not p["list"] and p["per_lane"] == 1 and p["chunk"] == 2048 and p["rounds2"] == 1, n
    assert C.plan(2047)["grid2"] == 1 and C.plan(2048)["grid2"] == 1 and C.plan(2049)["grid2"] == 2 and C.plan(4097)["grid2"] == 3
    assert C.plan(255)["grid1"] == 1 and C.plan(256)["grid1"] == 1 and C.plan(257)["grid1"] == 2
    assert C.plan(C.LIST_MIN - 1)["grid1"] == 1024 and C.plan(C.LIST_MIN - 1)["grid2"] == 128
    a, b, c = (C.plan(n) for n in C.SIZES_LIST)
    assert a["list"] and a["cap"] == 32768 and a["per_lane"] == 1 and a["grid1"] == 1024
    assert C.plan(C.SIZES_LIST[1] - 1)["per_lane"] == 1 and b["per_lane"] == 2 and b["grid1"] == 1536 and b["list"]
    assert c["list"] and c["cap"] == 50000 and c["per_lane"] == 2


@pytest.mark.parametrize("n", [1, 2, 65, 4097])
def test_layouts_land_on_the_claimed_reader(n):
    rng = np.random.default_rng(n)
    x1, x2 = rng.uniform(0, 900, (n, 2)).astype(np.float32), rng.uniform(0, 900, (n, 2)).astype(np.float32)
    for name, packed in C.LAYOUTS.items():
        a, b = C.layout_views(name, x1, x2)
        assert tuple(a.shape) == (2, n) and np.array_equal(a.numpy(), x1.T) and np.array_equal(b.numpy(), x2.T), name
        spt, sxy, al1, al2 = C.wrapper_strides(a, b)
        got = C.plan(n, spt, sxy, al1, al2)["packed"]
        if n == 1 and name == "mixed":
            assert got          # (strides of a one-column array are free: `contiguous()` keeps the transposed view's)
        elif n > 1:
            assert got == packed, (name, spt, sxy, al1, al2)
        if name == "offset4":
            assert (spt, sxy) == (2, 1) and al1 == 4 and al2 == 4
        if name == "mixed" and n > 1:
            assert (spt, sxy) == (1, n)
        if name == "wide":
            assert (spt, sxy) == (3, 1)


def test_reject_cases_land_on_the_claimed_plans():
    for name, (n, which, _, want, why) in C.REJECT_CASES.items():
        planted = C.planted_rejects(n, which)
        assert len(np.unique(planted)) == len(planted) and (len(planted) == 0 or (planted.min() >= 0 and planted.max() < n)), name
        assert C.reject_plan(n, planted) == (want, why), name
    n, which = C.REJECT_CASES["list_many"][:2]
    assert len(C.planted_rejects(n, which)) == n // 16
    n, which = C.REJECT_CASES["cap_overflow"][:2]
    assert len(C.planted_rejects(n, which)) == C.plan(n)["cap"] + 1                  # exceeds cap by its planted points alone
    n, which = C.REJECT_CASES["wg_overflow"][:2]
    planted = C.planted_rejects(n, which)
    assert n == 4 * 1536 * 256 + 256 and len(planted) == 1280 and C.plan(n)["per_lane"] == 5
    assert np.array_equal(planted, np.flatnonzero((np.arange(n) // 256) % 1536 == 0))
    per_wg = np.bincount(C.workgroup_of(planted, n), minlength=1536)
    assert per_wg[0] == 1280 > C.WG_QUEUE and per_wg[1:].sum() == 0
    assert len(planted) + int(np.ceil(C.NATURAL_REJECT_MAX * n)) < C.plan(n)["cap"] // 2      # total far below cap
    p = C.plan(C.FIXUP_TWO_ROUNDS_N)
    assert C.FIXUP_TWO_ROUNDS_N == 1024 * 20480 + 4097 and p["chunk"] == 20480 and p["grid2"] == 1024 and p["rounds2"] == 2
    assert p["list"] and C.FIXUP_TWO_ROUNDS_N // 1536 > C.WG_QUEUE         # all rejected: every workgroup's queue overflows
    assert C.plan(C.FIXUP_TWO_ROUNDS_N - 4097)["rounds2"] == 1


def test_block_sizes_pass_the_prefix_stride():
    assert -(-(257 * 1024 + 3) // C.TM_CHUNK) == 258 > C.PREFIX_STRIDE + 1
    assert -(-(258 * 1024 + 5) // C.MASK_BLOCK) == 259 > C.PREFIX_STRIDE + 1


@pytest.mark.parametrize("rows", [4, 6])
@pytest.mark.parametrize("geometry", [g for g, unique in C.GEOMETRIES.items() if unique])
def test_oracle_holds_the_bars_of_the_float64_reference(oracle, geometry, rows):
    n = C.POOL if (geometry == "gustav03" and rows == 4) else 4097
    P1, P2, x1, x2 = C.pair(geometry, n)
    unit, normalised, s = T.triangulate(P1, P2, x1, x2, rows)
    assert (s[:, 2] > s[:, 3]).all()                                    # one null vector
    en = T.normalised_error(oracle.triangulate(P1, P2, x1.T, x2.T, rows=rows, normalise_w=True), normalised)
    er = T.raw_error(oracle.triangulate(P1, P2, x1.T, x2.T, rows=rows, normalise_w=False), unit)
    print(f"{geometry} rows {rows} n {n}: normalised {en.max():.3f}, raw {er.max():.3f} (units of 2^-24)")
    assert en.max() <= T.BAR_NORMALISED and er.max() <= T.BAR_RAW
    for m in C.SIZES_SMALL:                                             # a prefix of the pool is the case of that size
        if m <= n:
            assert np.array_equal(C.pair(geometry, m)[2], x1[:m])


def test_same_camera_geometry_has_no_unique_null_vector():
    P1, P2, x1, x2 = C.pair("same", 4097)
    s = T.triangulate(P1, P2, x1, x2, 4)[2]
    assert np.array_equal(P1, P2) and np.array_equal(x1, x2) and (s[:, 2] < 1e-12 * s[:, 0]).all()


def test_pose_case_holds_every_kind_of_point():
    cands, x1n, x2n, kind, z1, z2 = C.pose_case()
    assert cands.shape == (4, 3, 4) and np.allclose(np.linalg.det(cands[:, :, :3]), 1.0)
    assert ((z1 > 0) & (z2 > 0))[kind <= 1].all() and (z1[kind == 2] < 0).all()
    assert (z1[kind == 3] > 0).all() and (z2[kind == 3] < 0).all() and (z1[kind == 4] > 1e3).all()
    near = kind == 1
    for z in (z1, z2):
        assert (z[near] < C.POSE_DIST).sum() > 20 and (z[near] > C.POSE_DIST).sum() > 20          # both sides of dist
    for n in C.POSE_N[2:]:
        assert len(np.unique(kind[:n])) == 5, n
    mask, _ = T.cheirality(cands, x1n, x2n, C.POSE_DIST, 4)
    assert all((mask[a] != mask[b]).any() for a in range(4) for b in range(a))                   # the four masks differ


@pytest.mark.parametrize("rows", [4, 6])
@pytest.mark.parametrize("n", C.POSE_N)
def test_oracle_cheirality_equals_the_float64_reference(oracle, n, rows):
    cands, x1n, x2n = C.pose_case()[:3]
    for h in range(1, 5):
        counts, mask = oracle.recover_pose_score(cands[:h], x1n[:n], x2n[:n], C.POSE_DIST, rows)
        want, decidable = T.cheirality(cands[:h], x1n[:n], x2n[:n], C.POSE_DIST, rows)
        assert (~decidable).sum() <= 1e-3 * decidable.size
        assert np.array_equal((mask > 0)[decidable], want[decidable]) and set(np.unique(mask)) <= {0, 255}
        assert np.array_equal(counts, (mask > 0).sum(1))
