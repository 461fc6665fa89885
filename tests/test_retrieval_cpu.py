"""The RETRIEVAL family without a GPU: the symbols and every argument error of the entry points and wrappers, the restatement
tests/np_retrieval.py on cases small enough to check by hand, and the calibration bars on the scenes of tests/retrieval_cases.py
(committed as tests/golden/retrieval_calibration.json; include/sfm_hip.h, "RETRIEVAL"; docs/retrieval.md)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import np_retrieval as nr  # noqa: E402
import retrieval_cases as rc  # noqa: E402

SYMBOLS = ("sfm_vlad_accumulate", "sfm_vlad_centres", "sfm_vlad_signature", "sfm_vlad_shortlist_ws_bytes", "sfm_vlad_shortlist",
           "sfm_vlad_pairs_ws_bytes", "sfm_vlad_pairs")


@pytest.fixture(scope="module")
def retrieval():
    import sfm_mvs_amd
    sfm_mvs_amd.lib()
    from sfm_mvs_amd import retrieval
    return retrieval


# ---- symbols and errors -----------------------------------------------------------------------------------------------------------

def test_the_symbols_are_declared_bound_and_documented_and_the_abi_is_still_3(retrieval):
    from sfm_mvs_amd import _lib
    header = open(os.path.join(ROOT, "include", "sfm_hip.h")).read()
    doc = open(os.path.join(ROOT, "docs", "retrieval.md")).read()
    for name in SYMBOLS:
        assert name + "(" in header and name in _lib.SIGNATURES and name in doc, name
        getattr(_lib.lib(), name)
    assert "RETRIEVAL" in header and _lib.lib().sfm_abi_version() == 3 and _lib.ABI_VERSION == 3
    assert "retrieval.hip" in _lib.code_hashes_of_binary()
    assert "retrieval.md" in open(os.path.join(ROOT, "DESIGN.md")).read() and "retrieval" in open(os.path.join(ROOT, "README.md")).read()


def test_argument_errors_of_the_entry_points_come_before_any_device_call(retrieval):
    from sfm_mvs_amd import _lib
    L = _lib.lib()
    p = np.zeros(16, np.int64).ctypes.data                           # 16-byte aligned, never dereferenced: every call below fails on its arguments
    assert p % 16 == 0
    nan, inf = float("nan"), float("inf")
    err = lambda rc_, text: rc_ == -1 and text in L.sfm_last_error()  # noqa: E731

    def acc(n=4, C=2, n_img=1, scale=1.0, desc=p, cen=p, off=p, out=p):
        return L.sfm_vlad_accumulate(desc, n, cen, C, off, n_img, scale, out, out, out, None)
    assert err(acc(n=-1), b"n_nodes") and err(acc(n=2 ** 31), b"n_nodes")
    assert err(acc(C=0), b"n_centres must be 1..256") and err(acc(C=257), b"n_centres must be 1..256")
    assert err(acc(n_img=0), b"n_img must be 1..65536") and err(acc(n_img=65537), b"n_img must be 1..65536")
    for bad in (nan, 0.0, -1.0, inf):
        assert err(acc(scale=bad), b"scale must be positive and finite"), bad
    assert err(acc(desc=p + 4), b"16-byte aligned") and err(acc(cen=p + 8), b"16-byte aligned")
    assert err(acc(desc=None), b"null pointer") and err(acc(cen=None), b"null pointer") and err(acc(off=None), b"null pointer") and err(acc(out=None), b"null pointer")

    def cen(C=2, scale=1.0, a=p, out=p):
        return L.sfm_vlad_centres(a, a, a, C, scale, out, None)
    assert err(cen(C=0), b"n_centres") and err(cen(C=257), b"n_centres") and err(cen(a=None), b"null pointer") and err(cen(out=None), b"null pointer")
    for bad in (nan, 0.0, -2.0, inf):
        assert err(cen(scale=bad), b"scale must be positive and finite"), bad

    def sig(n_img=1, C=2, qs=127.0, a=p, out=p):
        return L.sfm_vlad_signature(a, n_img, C, 0, qs, out, out, None)
    assert err(sig(n_img=0), b"n_img") and err(sig(n_img=-3), b"n_img") and err(sig(n_img=65537), b"n_img") and err(sig(C=0), b"n_centres") and err(sig(C=300), b"n_centres")
    for bad in (nan, 0.0, -127.0, inf):
        assert err(sig(qs=bad), b"qs must be positive and finite"), bad
    assert err(sig(a=None), b"null pointer") and err(sig(out=None), b"null pointer")

    def short(n_img=4, C=2, k=2, min_sim=0.0, ws=None, s=p, out=p, w=p):
        return L.sfm_vlad_shortlist(s, out, n_img, C, k, min_sim, out, out, w, n_img * n_img * 4 if ws is None else ws, None)
    assert err(short(n_img=0), b"n_img must be 1..16384") and err(short(n_img=16385), b"n_img must be 1..16384")
    assert err(short(C=0), b"n_centres") and err(short(C=257), b"n_centres") and err(short(k=0), b"k must be 1..64") and err(short(k=65), b"k must be 1..64")
    assert err(short(min_sim=nan), b"min_sim is NaN") and err(short(ws=63), b"the workspace holds 63 bytes, 64 are needed")
    assert err(short(s=p + 1), b"16-byte aligned") and err(short(s=None), b"null pointer") and err(short(out=None), b"null pointer") and err(short(w=None), b"null pointer")
    assert L.sfm_vlad_shortlist_ws_bytes(4) == 64 and L.sfm_vlad_shortlist_ws_bytes(16384) == 2 ** 30
    assert L.sfm_vlad_shortlist_ws_bytes(0) == 0 and L.sfm_vlad_shortlist_ws_bytes(-1) == 0 and L.sfm_vlad_shortlist_ws_bytes(16385) == 0

    def pairs(n_img=4, k=2, cap=8, ws=None, nbr=p, out=p, cnt=p, w=p):
        return L.sfm_vlad_pairs(nbr, n_img, k, 0, out, cap, cnt, w, 512 if ws is None else ws, None)
    assert err(pairs(n_img=0), b"n_img must be 1..16384") and err(pairs(n_img=16385, ws=2 ** 40), b"n_img must be 1..16384")
    assert err(pairs(k=0), b"k must be 1..64") and err(pairs(k=65), b"k must be 1..64") and err(pairs(cap=-1), b"cap_pairs") and err(pairs(cap=2 ** 31), b"cap_pairs")
    assert err(pairs(ws=511), b"the workspace holds 511 bytes, 512 are needed")
    assert err(pairs(nbr=None), b"null pointer") and err(pairs(out=None), b"null pointer") and err(pairs(cnt=None), b"null pointer") and err(pairs(w=None), b"null pointer")
    assert L.sfm_vlad_pairs_ws_bytes(4) == 512 and L.sfm_vlad_pairs_ws_bytes(0) == 0 and L.sfm_vlad_pairs_ws_bytes(16385) == 0
    assert L.sfm_vlad_pairs_ws_bytes(16384) == 16384 * 512 * 4 + 16384 * 4


def test_the_wrappers_reject_host_tensors_and_bad_settings(retrieval):
    from sfm_mvs_amd import tracks
    Err = retrieval.SfmHipError
    z = lambda shape, dt: torch.zeros(shape, dtype=dt)                # noqa: E731
    desc, cen, off = z((4, 128), torch.float32), z((2, 128), torch.float32), z(2, torch.int32)
    for call in (lambda: retrieval.assign_accumulate(desc, cen, off, 1.0),
                 lambda: retrieval.update_centres(cen, z((2, 128), torch.int64), z(2, torch.int32), 1.0),
                 lambda: retrieval.train_vocabulary(desc, 2),
                 lambda: retrieval.signatures(z((1, 2, 128), torch.int64)),
                 lambda: retrieval.shortlist(z((3, 256), torch.int8), z(3, torch.int32), 2),
                 lambda: retrieval.pair_list(z((3, 2), torch.int32)),
                 lambda: retrieval.select_pairs([desc, desc]),
                 lambda: tracks.retrieval_pairs([desc, desc], k=2)):
        with pytest.raises(Err, match="no CPU fallback"):
            call()
    with pytest.raises(Err, match="no image"):
        retrieval.select_pairs([])
    for bad in (0, 65, -1):
        with pytest.raises(Err, match="k must be 1..64"):
            retrieval._k(bad)
    for bad in (float("nan"), 0.0, -1.0, float("inf")):
        with pytest.raises(Err, match="positive and finite"):
            retrieval._positive(bad, "scale")
        with pytest.raises(Err, match="positive and finite"):
            retrieval.scale_of(bad)
    with pytest.raises(Err, match="centres"):
        retrieval.initial_rows(10, 257)
    with pytest.raises(Err, match="3 centres from 2 descriptors"):
        retrieval.initial_rows(2, 3)
    assert retrieval.scale_of(256.0) == 4096.0 == nr.scale_of(256.0) and retrieval.scale_of(1.0) == 2.0 ** 20 and retrieval.scale_of(200.0) == 4096.0
    assert retrieval.initial_rows(1000, 64, 3) == nr.initial_rows(1000, 64, 3) == sorted(set(retrieval.initial_rows(1000, 64, 3)))


# ---- the restatement on cases checked by hand ---------------------------------------------------------------------------------------

def rows(*firsts):
    """Descriptor rows that are zero but for their first entries."""
    out = np.zeros((len(firsts), 128), np.float32)
    for r, f in enumerate(firsts):
        f = np.atleast_1d(np.asarray(f, np.float32))
        out[r, :len(f)] = f
    return out


def test_two_centres_and_four_descriptors_by_hand():
    centres = rows([0, 0], [10, 0])
    desc = rows([1, 2], [9, -1], [2, 0], [12, 3])
    a, acc, count = nr.accumulate(desc, centres, [0, 4], 4.0)
    assert a.tolist() == [0, 1, 0, 1] and count.tolist() == [[2, 2]]
    assert acc[0, 0, :3].tolist() == [4 * (1 + 2), 4 * (2 + 0), 0] and acc[0, 1, :3].tolist() == [4 * (-1 + 2), 4 * (-1 + 3), 0]
    a, acc, count = nr.accumulate(desc, centres, [0, 1, 1, 4], 4.0)    # three images, the second empty
    assert count.tolist() == [[1, 0], [0, 0], [1, 2]] and acc[0, 0, :2].tolist() == [4, 8] and acc[2, 0, :2].tolist() == [8, 0] and not acc[1].any()
    new = nr.update_centres(centres, *[v[0] for v in nr.accumulate(desc, centres, [0, 4], 4.0)[1:]], 4.0)
    assert new[0, :2].tolist() == [1.5, 1.0] and new[1, :2].tolist() == [10.5, 1.0]                   # the means of the members


def test_ties_duplicate_centres_and_an_empty_centre_that_keeps_its_bits():
    centres = rows([0], [4], [4], [-0.0])
    centres[3, 5] = np.float32(1e-40)                                # a denormal and a negative zero: bits a recomputation would not keep
    desc = rows([2], [4], [5])
    a, acc, count = nr.accumulate(desc, centres, [0, 3], 1.0)
    assert a.tolist() == [0, 1, 1]                                   # equidistant from 0 and 1: the lower index; the duplicate 2 stays empty
    assert count.tolist() == [[1, 2, 0, 0]]
    new = nr.update_centres(centres, acc[0], count[0], 1.0)
    assert new[2].view(np.int32).tolist() == centres[2].view(np.int32).tolist() and new[3].view(np.int32).tolist() == centres[3].view(np.int32).tolist()
    assert new[1, 0] == 4.5 and new[0, 0] == 2.0


def test_terms_round_half_even_and_clamp_at_two_to_the_thirty():
    centres = rows([0])
    desc = rows([0.5, 1.5, 2.5, -0.5, -1.5, 1e15, -1e15, 1.25])
    _, acc, _ = nr.accumulate(desc, centres, [0, 1], 1.0)
    assert acc[0, 0, :8].tolist() == [0, 2, 2, 0, -2, 2 ** 30, -2 ** 30, 1]
    _, acc, _ = nr.accumulate(desc, centres, [0, 1], 2.0 ** 40)
    assert acc[0, 0, :8].tolist() == [2 ** 30, 2 ** 30, 2 ** 30, -2 ** 30, -2 ** 30, 2 ** 30, -2 ** 30, 2 ** 30]
    _, acc, _ = nr.accumulate(desc, centres, [0, 1], 3e38)           # r * scale overflows to +-inf: the clamp still holds
    assert acc[0, 0, 4:7].tolist() == [-2 ** 30, 2 ** 30, -2 ** 30]
    assert nr.terms(np.float32([0.5, 1.5, -2.5, 3e38]), np.float32([0, 0, 0, -3e38]), 1.0).tolist() == [0, 2, -2, 2 ** 30]


def test_nan_and_inf_rows_are_assigned_to_nobody_and_add_nothing():
    centres = rows([0], [8])
    desc = rows([1], [np.nan], [np.inf], [7], [-np.inf], [3e30])     # 3e30: the square overflows to +inf
    a, acc, count = nr.accumulate(desc, centres, [0, 6], 1.0)
    assert a.tolist() == [0, -1, -1, 1, -1, -1] and count.tolist() == [[1, 1]] and acc[0, :, 0].tolist() == [1, -1]
    bad = rows([np.nan], [8])                                        # a NaN centre is no candidate
    assert nr.assign(rows([1]), bad).tolist() == [1] and nr.assign(rows([1]), rows([np.nan])).tolist() == [-1]


def test_an_image_without_keypoints_has_a_zero_signature_and_no_neighbours():
    centres = rows([0], [8])
    desc = rows([1, 1], [7, 2], [1, 2], [7, 1])
    _, acc, _ = nr.accumulate(desc, centres, [0, 2, 2, 4], 16.0)
    sig, norm2 = nr.signatures(acc)
    assert norm2[1] == 0 and not sig[1].any() and norm2[0] > 0 and norm2[2] > 0
    nbr, sim = nr.shortlist(sig, norm2, 2)
    assert nbr.tolist() == [[2, -1], [-1, -1], [0, -1]] and np.isneginf(sim[1]).all() and np.isneginf(sim[:, 1]).all()
    assert nr.pair_list(nbr)[0].tolist() == [[0, 2]]


def test_signature_words_by_hand():
    acc = np.zeros((1, 2, 128), np.int64)
    acc[0, 0, :2] = [3, -4]
    sig, norm2 = nr.signatures(acc, qs=10.0)
    assert sig[0, :2].tolist() == [6, -8] and not sig[0, 128:].any() and norm2.tolist() == [100]
    sig, _ = nr.signatures(acc, ssr=True, qs=7.0)                    # sqrt 3 and -2 over sqrt 7: 4.58 and -5.29
    assert sig[0, :2].tolist() == [5, -5]
    sig, _ = nr.signatures(acc, qs=1000.0)                           # 600 and -800 clip
    assert sig[0, :2].tolist() == [127, -127]
    acc[0, 1, :] = 2 ** 62
    sig, norm2 = nr.signatures(acc)
    assert (sig[0, 128:] == 11).all() and norm2[0] == 76 * 76 + 102 * 102 + 128 * 121                  # 127 / sqrt(128) = 11.2


def test_identical_images_tie_to_the_smaller_index_and_opposite_ones_score_minus_one():
    rng = np.random.default_rng(1)
    sig = rng.integers(-100, 101, (4, 256)).astype(np.int8)
    sig[2] = sig[0]
    sig[3] = -sig[0]
    norm2 = (sig.astype(np.int64) ** 2).sum(1).astype(np.int32)
    nbr, sim = nr.shortlist(sig, norm2, 3)
    assert nbr[1, :2].tolist() == [0, 2] and sim[1, 0] == sim[1, 1]   # images 0 and 2 are equally similar to image 1: 0 first
    assert nbr[0, 0] == 2 and sim[0, 0] == 1.0 and nbr[0, 2] == 3 and sim[0, 2] == -1.0 and nbr[3].tolist() == [1, 0, 2]
    nbr, sim = nr.shortlist(sig, norm2, 3, min_sim=1.0)
    assert nbr[0].tolist() == [2, -1, -1] and nbr[1].tolist() == [-1, -1, -1]
    assert (nr.shortlist(sig, norm2, 3, min_sim=np.inf)[0] == -1).all()


def test_mutual_against_the_union_on_an_asymmetric_list():
    nbr = np.array([[1, 2], [0, -1], [3, -1], [2, 0], [4, 9]], np.int32)   # 0 names 2, 2 does not name 0; 4 names itself and nobody
    union, cu = nr.pair_list(nbr)
    both, cm = nr.pair_list(nbr, mutual=True)
    assert union.tolist() == [[0, 1], [0, 2], [0, 3], [2, 3]] and cu.tolist() == [4, 4]
    assert both.tolist() == [[0, 1], [2, 3]] and cm.tolist() == [2, 2]
    assert nr.pair_list(nbr, cap_pairs=3)[1].tolist() == [4, 3] and nr.pair_list(nbr, cap_pairs=0)[1].tolist() == [4, 0]


def test_k_of_everybody_selects_all_pairs_of_the_images_that_have_descriptors():
    sc = rc.corridor_scene(6, 30, 5, 5, 0)
    descs = list(sc["descs"])
    descs[3] = descs[3][:0]
    pairs, st = nr.select_pairs(descs, k=5, n_centres=4, iters=2)
    assert set(pairs) == set((a, b) for a, b in rc.all_pairs(6) if 3 not in (a, b)) and pairs == sorted(pairs)
    again, st2 = nr.select_pairs(descs, k=5, n_centres=4, iters=2)
    assert again == pairs and np.array_equal(st["centres"].view(np.int32), st2["centres"].view(np.int32))


# ---- calibration --------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def table():
    return rc.load_calibration()


@pytest.fixture(scope="module")
def corridor_default():
    """The corridor at the default setting, restated once: (pairs per k, stages, shared points)."""
    sc = rc.corridor_scene(seed=0, **rc.CORRIDOR)
    shared = rc.shared_points(sc["ids"])
    out, centres = {}, None
    for k in (4, 8):
        pairs, st = nr.select_pairs(sc["descs"], k=k, n_centres=rc.DEFAULT["n_centres"], ssr=rc.DEFAULT["ssr"], centres=centres)
        centres = st["centres"]
        out[k] = (pairs, st)
    return out, shared


@pytest.mark.parametrize("k", [4, 8])
def test_the_corridor_shortlist_stays_within_the_calibrated_bars(table, corridor_default, k):
    """The share of selected pairs without a common point at most the measured value + 0.02, the recall of the pairs within the k / 2
    nearest at least the measured value - 0.05; the margins absorb a change of seed, not of arithmetic."""
    (pairs, st), shared = corridor_default[0][k], corridor_default[1]
    m = rc.measures(pairs, shared, k)
    print(f"k = {k}: {m}")
    row = rc.row_of(table, scene="corridor", seed=0, k=k, **{n: rc.DEFAULT[n] for n in ("n_centres", "ssr")})
    assert m["wrong_share"] <= row["wrong_share"] + 0.02 and m["recall"] >= row["recall"] - 0.05
    assert m["selected"] == row["selected"] and m["kept_fraction"] < 0.2          # the same arithmetic gives the same list
    assert int((np.abs(st["sig"].astype(np.int32)) == 127).sum()) == row["clipped"] == 0
    for seed in (1, 2):                                              # the other seeds of the table lie inside the margins of seed 0
        other = rc.row_of(table, scene="corridor", seed=seed, k=k, **{n: rc.DEFAULT[n] for n in ("n_centres", "ssr")})
        assert other["wrong_share"] <= row["wrong_share"] + 0.02 and other["recall"] >= row["recall"] - 0.05


def test_the_similarity_falls_with_the_distance_along_the_corridor(corridor_default):
    (_, st), shared = corridor_default[0][8], corridor_default[1]
    _, sim = nr.similarities(st["sig"], st["norm2"])
    steps = np.array([np.mean(sim[shared == 600 - 60 * d]) for d in range(1, 10)])
    print("mean cosine by images apart:", np.round(steps, 3))
    assert (np.diff(steps) < 0).all() and steps[0] > 0.4 and np.mean(sim[(shared == 0) & ~np.eye(len(sim), dtype=bool)]) < steps[-1]


def test_the_cluster_scene_selects_no_pair_across_objects(table):
    cl = rc.cluster_scene(seed=0, **rc.CLUSTER)
    for k in (2, rc.CLUSTER["ring"] - 1):
        pairs, _ = nr.select_pairs(cl["descs"], k=k, n_centres=16)
        assert pairs and all(cl["obj"][a] == cl["obj"][b] for a, b in pairs)
        row = rc.row_of(table, scene="cluster", k=k)
        assert row["crossing"] == 0 and row["selected"] == len(pairs)
    assert len(pairs) == rc.CLUSTER["n_obj"] * rc.CLUSTER["ring"] * (rc.CLUSTER["ring"] - 1) // 2        # at ring - 1 every same-object pair


def test_the_shortlist_keeps_the_calibrated_fraction_of_the_all_pairs_tracks(table):
    from oracle import oracle as O
    O.lib()
    tc = rc.track_case()
    row = rc.row_of(table, scene="tracks")
    frac = tc["tracks_short"] / tc["tracks_all"]
    print(f"tracks: {tc['tracks_short']} of {tc['tracks_all']} from {len(tc['pairs'])} of 120 pairs")
    assert frac >= row["track_fraction"] - 0.05 and len(tc["pairs"]) == row["selected"] and tc["tracks_all"] == row["tracks_all"]
    m = rc.measures(tc["pairs"], rc.shared_points(tc["scene"]["ids"]), rc.TRACK_SETTING["k"])
    assert m["wrong_share"] <= row["wrong_share"] + 0.02 and m["recall"] >= row["recall"] - 0.05
