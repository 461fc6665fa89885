"""The TRACKS family without a GPU (include/sfm_hip.h, "TRACKS"; docs/tracks.md): the C-ABI declares, binds, documents and validates
the entry points; the restatement tests/np_tracks.py stands apart from the product, gives hand-checked results on small graphs,
stays within a recorded bound of np.linalg.eigh, and meets the calibration bars on the two planted scenes."""
import ast
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import np_tracks as nt  # noqa: E402

NEW_SYMBOLS = ("sfm_match_edges", "sfm_track_components_ws_bytes", "sfm_track_components", "sfm_track_build_ws_bytes", "sfm_track_build",
               "sfm_track_triangulate")

# Measured here (docs/tracks.md §4), each recorded with its margin.
# The restated Jacobi against np.linalg.eigh on the same M, over the 400 ring tracks, as points v[:3] / v[3] in float64 (the points lie
# within the unit ball; M's eigenvalues span up to 1.1e6): the largest difference of a coordinate is 1.263e-15.  The bound is 4 x that.
EIGH_BOUND = 5.1e-15
# N-view against first-two-view triangulation with the header's rows (not normalised), both by the restatement: median distance to the
# planted points 0.00135 against 0.00335 on ring_scene(8, 600, 400, seed=3): r = 0.404.  The bar is (1 + r) / 2 = 0.702.
RING_RATIO = 0.404
RING_BAR = (1.0 + RING_RATIO) / 2.0


def declared():
    from test_abi import declared_symbols
    return declared_symbols()


def test_header_declares_binds_and_documents_the_track_entry_points():
    from sfm_mvs_amd import _lib
    syms = declared()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    doc = open(os.path.join(ROOT, "docs", "tracks.md")).read()
    header = open(os.path.join(ROOT, "include", "sfm_hip.h")).read()
    assert "TRACKS" in header and "no word depends on" in header and "cyclic Jacobi" in header
    for s in NEW_SYMBOLS:
        assert s in syms and s in _lib.SIGNATURES and hasattr(handle, s), s
        assert s in doc, f"docs/tracks.md does not mention {s}"
    assert _lib.lib().sfm_abi_version() == 3 and _lib.ABI_VERSION == 3
    assert "tracks.hip" in _lib.code_hashes_of_binary()


def test_python_layer_exposes_the_entry_points():
    import inspect
    from sfm_mvs_amd import tracks
    for name in ("match_edges", "track_components", "build_tracks", "triangulate_tracks", "run_tracks", "verify_keep"):
        assert callable(getattr(tracks, name)), name
    sig = inspect.signature(tracks.run_tracks).parameters
    assert list(sig)[:5] == ["store", "n_query", "pairs", "keypoints", "P"]
    assert sig["ratio"].default == 0.70 and sig["keep"].default is None and sig["min_len"].default == 2
    assert sig["max_len"].default is None and sig["max_reproj"].default is None
    assert inspect.signature(tracks.track_components).parameters["rounds"].default == tracks.TRACK_ROUNDS
    assert 1 <= tracks.TRACK_ROUNDS <= 1024


def test_argument_errors_are_reported_before_the_device():
    """Every argument error of the header: SFM_ERR_ARG with its message, before any device call (the pointers are never read)."""
    from sfm_mvs_amd import _lib
    L = _lib.lib()
    fake = [ctypes.c_void_p(16 * (k + 1)) for k in range(12)]
    big = 1 << 31
    nan = float("nan")

    def edges(store=fake[0], n_pairs=10, cap=100, pair=fake[1], nq=fake[2], off=fake[3], n_img=5, ratio=0.7, keep=None, out=fake[4]):
        return L.sfm_match_edges(store, n_pairs, cap, pair, nq, off, n_img, ratio, keep, out, None)

    def comps(e=fake[0], n=100, ne=50, rounds=8, resume=0, labels=fake[1], status=fake[2], ws=fake[3], wsb=1 << 20):
        return L.sfm_track_components(e, n, ne, rounds, resume, labels, status, ws, wsb, None)

    def build(labels=fake[0], off=fake[1], n=100, n_img=5, lo=2, hi=big - 1, nt=fake[2], to=fake[3], on=fake[4], counts=fake[5], ws=fake[6], wsb=1 << 30):
        return L.sfm_track_build(labels, off, n, n_img, lo, hi, nt, to, on, counts, ws, wsb, None)

    def tri(counts=fake[0], to=fake[1], on=fake[2], off=fake[3], n_img=5, kp=fake[4], P=fake[5], n=100, X=fake[6], err=fake[7], depth=fake[8],
            flags=fake[9], worst=fake[10]):
        return L.sfm_track_triangulate(counts, to, on, off, n_img, kp, P, n, X, err, depth, flags, worst, None)

    cases = [
        (edges, dict(n_pairs=-1), b"n_pairs"), (edges, dict(cap=-1), b"cap"), (edges, dict(n_pairs=big), b"n_pairs"), (edges, dict(cap=big), b"cap"),
        (edges, dict(n_pairs=1 << 16, cap=1 << 15), b"edge slots"), (edges, dict(n_img=0), b"n_img"), (edges, dict(n_img=65537), b"n_img"),
        (edges, dict(ratio=nan), b"NaN"), (edges, dict(off=None), b"null"), (edges, dict(store=None), b"null"), (edges, dict(pair=None), b"null"),
        (edges, dict(nq=None), b"null"), (edges, dict(out=None), b"null"), (edges, dict(n_pairs=0, off=None), b"null"),
        (comps, dict(n=-1), b"n_nodes"), (comps, dict(ne=-1), b"ne"), (comps, dict(n=big), b"n_nodes"), (comps, dict(ne=big), b"ne"),
        (comps, dict(rounds=0), b"rounds"), (comps, dict(rounds=1025), b"rounds"), (comps, dict(status=None), b"null"),
        (comps, dict(ws=None), b"null"), (comps, dict(labels=None), b"null"), (comps, dict(e=None), b"null"), (comps, dict(wsb=16), b"workspace"),
        (build, dict(n=-1), b"n_nodes"), (build, dict(n=big), b"n_nodes"), (build, dict(n_img=0), b"n_img"), (build, dict(n_img=65537), b"n_img"),
        (build, dict(lo=1), b"min_len"), (build, dict(lo=5, hi=4), b"min_len"), (build, dict(hi=big), b"max_len"), (build, dict(lo=-3), b"min_len"),
        (build, dict(labels=None), b"null"), (build, dict(off=None), b"null"), (build, dict(nt=None), b"null"), (build, dict(to=None), b"null"),
        (build, dict(on=None), b"null"), (build, dict(counts=None), b"null"), (build, dict(ws=None), b"null"), (build, dict(wsb=64), b"workspace"),
        (build, dict(n=0, to=None), b"null"),
        (tri, dict(n=-1), b"n_nodes"), (tri, dict(n=big), b"n_nodes"), (tri, dict(n_img=0), b"n_img"), (tri, dict(n_img=65537), b"n_img"),
        (tri, dict(counts=None), b"null"), (tri, dict(to=None), b"null"), (tri, dict(on=None), b"null"), (tri, dict(off=None), b"null"),
        (tri, dict(kp=None), b"null"), (tri, dict(P=None), b"null"), (tri, dict(X=None), b"null"), (tri, dict(err=None), b"null"),
        (tri, dict(depth=None), b"null"), (tri, dict(flags=None), b"null"), (tri, dict(worst=None), b"null"),
    ]
    for call, kw, msg in cases:
        assert call(**kw) == -1, (call.__name__, kw)
        assert msg in L.sfm_last_error(), (call.__name__, kw, L.sfm_last_error())
    assert L.sfm_track_components_ws_bytes(-1, 0) == 0 and L.sfm_track_components_ws_bytes(0, big) == 0 and L.sfm_track_build_ws_bytes(big) == 0
    assert L.sfm_track_components_ws_bytes(10, 10) >= 4 * 1025 and L.sfm_track_build_ws_bytes(0) > 0
    assert L.sfm_track_build_ws_bytes(640000) >= 4 * 5 * 640000 + 12 * (1 << 21)


def test_the_restatement_does_not_import_the_product():
    tree = ast.parse(open(os.path.join(ROOT, "tests", "np_tracks.py")).read())
    for node in ast.walk(tree):
        names = [a.name for a in node.names] if isinstance(node, ast.Import) else [node.module or ""] if isinstance(node, ast.ImportFrom) else []
        assert not any(n.split(".")[0] in ("sfm_mvs_amd", "oracle") for n in names), names


# ---- hand-checked graphs ------------------------------------------------------------------------------------------------------

def tracks_of(edges, img_off, **kw):
    n = img_off[-1]
    labels = nt.components(np.array(edges, np.int32).reshape(-1, 2), n)
    node_track, track_off, obs_node, counts = nt.build(labels, img_off, **kw)
    return labels, node_track, [obs_node[track_off[t]:track_off[t + 1]].tolist() for t in range(len(track_off) - 1)], counts.tolist()


def test_two_tracks_and_a_lone_node():
    # images of 3, 3, 3 nodes: 0-2, 3-5, 6-8.  Track {1, 4, 8}, track {2, 3}; node 0 is alone, as are 5, 6, 7.
    labels, node_track, tracks, counts = tracks_of([[1, 4], [4, 8], [3, 2]], [0, 3, 6, 9])
    assert labels.tolist() == [0, 1, 2, 2, 1, 5, 6, 7, 1]
    assert tracks == [[1, 4, 8], [2, 3]] and node_track.tolist() == [-1, 0, 1, 1, 0, -1, -1, -1, 0]
    assert counts == [2, 5, 2, 0, 3, 4]


def test_conflicts_direct_and_through_a_chain():
    # a direct edge inside image 0 (nodes 0, 1), with a clean track {2, 4} beside it
    _, node_track, tracks, counts = tracks_of([[0, 1], [2, 4]], [0, 3, 6])
    assert tracks == [[2, 4]] and counts == [1, 2, 2, 1, 2, 2] and node_track.tolist() == [-1, -1, 0, -1, 1 - 1, -1]
    # a chain through three images that comes back to the first: 0 (img 0) - 3 (img 1) - 6 (img 2) - 1 (img 0)
    _, node_track, tracks, counts = tracks_of([[0, 3], [3, 6], [6, 1], [2, 5]], [0, 3, 6, 9])
    assert tracks == [[2, 5]] and counts == [1, 2, 2, 1, 2, 3] and node_track[[0, 1, 3, 6]].tolist() == [-1] * 4


def test_a_many_to_one_match_is_a_conflict():
    # two keypoints of image 0 both match keypoint 3 of image 1
    _, _, tracks, counts = tracks_of([[0, 3], [1, 3]], [0, 3, 6])
    assert tracks == [] and counts == [0, 0, 1, 1, 0, 3]


def test_length_bounds_at_the_boundary():
    off = [0, 2, 4, 6, 8]
    edges = [[0, 2], [1, 3], [3, 5], [1, 7]]                      # sizes 2 and 4
    for lo, hi, want in ((2, 4, [[0, 2], [1, 3, 5, 7]]), (3, 4, [[1, 3, 5, 7]]), (2, 3, [[0, 2]]), (2, 2, [[0, 2]]), (4, 4, [[1, 3, 5, 7]]),
                         (5, 9, []), (3, 3, [])):
        _, _, tracks, counts = tracks_of(edges, off, min_len=lo, max_len=hi)
        assert tracks == want and counts[2:4] == [2, 0] and counts[4] == max([len(t) for t in want], default=0) and counts[5] == 2


def test_empty_images_in_the_offsets():
    off = [0, 0, 2, 2, 2, 4, 4]                                    # images 0, 2, 3, 5 are empty; nodes 0, 1 in image 1; 2, 3 in image 4
    assert nt.image_of(off, [0, 1, 2, 3]).tolist() == [1, 1, 4, 4]
    _, _, tracks, counts = tracks_of([[0, 2], [1, 3]], off)
    assert tracks == [[0, 2], [1, 3]] and counts == [2, 4, 2, 0, 2, 0]
    _, _, tracks, counts = tracks_of([[0, 1], [2, 3]], off)        # both inside one image
    assert tracks == [] and counts == [0, 0, 2, 2, 0, 0]


def test_invalid_and_duplicate_edges_and_self_loops():
    big = 2 ** 31 - 1
    edges = [[0, 3], [3, 0], [0, 3], [1, 1], [-1, 2], [2, 6], [big, 4], [5, -1], [-1, -1], [4, 4], [2, 5]]
    labels, _, tracks, counts = tracks_of(edges, [0, 3, 6])
    assert labels.tolist() == [0, 1, 2, 0, 4, 2] and tracks == [[0, 3], [2, 5]] and counts == [2, 4, 2, 0, 2, 2]
    assert nt.components(np.zeros((0, 2), np.int32), 0).shape == (0,) and nt.build(np.zeros(0, np.int32), [0, 0])[3].tolist() == [0] * 6
    assert nt.is_valid_state([0, 1, 2, 0, 4, 2], labels) and nt.is_valid_state([0, 1, 2, 3, 4, 2], labels)
    assert not nt.is_valid_state([0, 1, 2, 1, 4, 2], labels) and not nt.is_valid_state([0, 1, 2, 0, 4, 5 + 1], labels)


def hand_store():
    """Two pairs over images of 4 and 3 keypoints -> (store, nq, pairs, img_off); see test_match_edges_by_hand."""
    inf = np.float32(np.inf)
    off = [0, 4, 7]                                                # image 0 has 4 keypoints, image 1 three
    d = lambda a, b: np.array([a, b], np.float32).view(np.int32)  # noqa: E731
    store = np.zeros((2, 2, 4, 2), np.int32)
    # pair 0 = (0, 1): q0 passes; q1 has d0 == 0.5 d1 exactly at ratio 0.5; q2 has no second neighbour; q3 is beyond nq
    store[0, 0] = [[2, 1], [0, 2], [1, -1], [2, 0]]
    store[0, 1] = [d(1.0, 4.0), d(2.0, 4.0), d(1.0, inf), d(1.0, 9.0)]
    # pair 1 = (1, 0): q0 passes to train 3; q1 names train 4 (outside image 0); q2 passes; slot 3 is beyond image 1's size
    store[1, 0] = [[3, 0], [4, 0], [0, 1], [0, 1]]
    store[1, 1] = [d(1.0, 4.0), d(1.0, 4.0), d(0.0, 1.0), d(0.0, 1.0)]
    return store, np.array([3, 4], np.int32), np.array([[0, 1], [1, 0]], np.int32), np.array(off, np.int32)


def test_match_edges_by_hand():
    store, _, _, off = hand_store()
    e = nt.match_edges(store, [3, 4], [[0, 1], [1, 0]], off, 0.5)
    assert e.tolist() == [[0, 6], [-1, -1], [-1, -1], [-1, -1], [4, 3], [-1, -1], [6, 0], [-1, -1]]
    keep = np.array([[0, 1, 1, 1], [1, 1, 0, 1]], np.uint8)
    e = nt.match_edges(store, [3, 4], [[0, 1], [1, 0]], off, 0.5, keep)
    assert e.tolist() == [[-1, -1]] * 4 + [[4, 3]] + [[-1, -1]] * 3
    assert nt.match_edges(store, [3, 4], [[0, 1], [1, 0]], off, np.nextafter(0.5, 1.0))[1].tolist() == [1, 4]


# ---- the planted scenes -------------------------------------------------------------------------------------------------------

def ring_points(n_scene, seed):
    """The scene points datagen.ring_scene draws first from its generator (it returns the cameras and the images only)."""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n_scene, 3))
    return X / np.maximum(np.linalg.norm(X, axis=1, keepdims=True), 1.0) * rng.uniform(0.2, 1.0, (n_scene, 1))


def store_of(des, pairs):
    """The match store of a pair list by the CPU oracle's exhaustive 2-NN."""
    from oracle import oracle as O
    cap = max(len(des[i]) for i, _ in pairs)
    store = np.zeros((len(pairs), 2, cap, 2), np.int32)
    for p, (i, j) in enumerate(pairs):
        idx, dist = O.knn2(des[i], des[j], nthreads=8)
        store[p, 0, :len(idx)] = idx
        store[p, 1, :len(idx)] = dist.view(np.int32)
    return store


@functools.lru_cache(maxsize=None)
def ring_case(n_img=8, n_desc=600, n_scene=400, seed=3):
    """-> dict(K, P, kps, des, ids, pairs, store, nq, img_off, kp, X): the all-pairs ring scene with its oracle match store."""
    from datagen import project, ring_scene
    K, P, image = ring_scene(n_img, n_desc, n_scene, seed=seed)
    ims = [image(k) for k in range(n_img)]
    kps, des, ids = [im[0] for im in ims], [im[1] for im in ims], [im[2] for im in ims]
    X = ring_points(n_scene, seed)
    x0, _ = project(P[0], X)
    seen = ids[0] >= 0
    assert np.abs(kps[0][seen] - x0[ids[0][seen]]).max() < 3.0          # the same points the scene projected (0.3 px noise)
    pairs = [(i, j) for i in range(n_img) for j in range(i + 1, n_img)]
    return finish_case(K, P, kps, des, ids, pairs, X)


@functools.lru_cache(maxsize=None)
def gustav_case(n_img=8, first=1500):
    from datagen import gustav_scene, sparse_points
    K, P, feats, ids = gustav_scene(n_img, seed=0, pix_noise=0.3)
    kps, des, ids = [f[0][:first] for f in feats], [f[1][:first] for f in feats], [np.asarray(i)[:first] for i in ids]
    pairs = [(i, j) for i in range(n_img) for j in range(i + 1, n_img)]
    return finish_case(K, np.asarray(P)[:n_img], kps, des, ids, pairs, sparse_points())


def finish_case(K, P, kps, des, ids, pairs, X):
    sizes = [len(k) for k in kps]
    return dict(K=K, P=np.asarray(P, np.float64), kps=kps, des=des, ids=np.concatenate(ids), pairs=pairs, store=store_of(des, pairs),
                nq=np.array([sizes[i] for i, _ in pairs], np.int32), img_off=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32),
                kp=np.concatenate(kps).astype(np.float32), X=X)


def purity(case, out):
    """(tracks, tracks that hold one scene-point id and no clutter, the id per track)."""
    tr = np.repeat(np.arange(len(out["track_off"]) - 1), np.diff(out["track_off"]))
    ids = case["ids"][out["obs_node"]]
    lo, hi = np.full(tr.max() + 1, np.iinfo(np.int64).max), np.full(tr.max() + 1, -2)
    np.minimum.at(lo, tr, ids)
    np.maximum.at(hi, tr, ids)
    return len(lo), int(((lo == hi) & (lo >= 0)).sum()), lo


def two_view(case, out):
    """The same tracks cut to their first two observations, triangulated by the same restatement."""
    off = out["track_off"].astype(np.int64)
    first = np.stack([out["obs_node"][off[:-1]], out["obs_node"][off[:-1] + 1]], 1).reshape(-1)
    return nt.triangulate(2 * np.arange(len(off)), first, case["img_off"], case["kp"], case["P"])[0]


def calibration(case):
    out = nt.run(case["store"], case["nq"], case["pairs"], case["img_off"], case["kp"], case["P"])
    n, pure, ids = purity(case, out)
    Xn, X2 = out["X"].astype(np.float64), two_view(case, out).astype(np.float64)
    truth = case["X"][ids]
    en, e2 = np.linalg.norm(Xn - truth, axis=1), np.linalg.norm(X2 - truth, axis=1)
    return out, n, pure, float(np.median(en)), float(np.median(e2))


def test_calibration_on_the_ring_scene():
    case = ring_case()
    out, n, pure, en, e2 = calibration(case)
    length = np.diff(out["track_off"])
    print(f"ring: {n} tracks, lengths {np.bincount(length).tolist()}, counts {out['counts'].tolist()}, pure {pure}; median error N-view {en:.5f} "
          f"two-view {e2:.5f} ratio {en / e2:.3f} (bar {RING_BAR:.3f})")
    assert n == 400 and np.all(length == 8) and out["counts"][3] == 0                      # every scene point, through all images, no conflict
    assert pure == n
    assert np.all(out["flags"] == 3)
    assert en <= RING_BAR * e2, (en, e2)


def test_calibration_on_the_gustav_scene():
    case = gustav_case()
    out, n, pure, en, e2 = calibration(case)
    length = np.diff(out["track_off"])
    print(f"gustav: {n} tracks, >= 3 views {int((length >= 3).sum())}, longest {length.max()}, counts {out['counts'].tolist()}, pure {pure}; "
          f"median error N-view {en:.5f} two-view {e2:.5f}")
    assert n > 2000 and pure == n and out["counts"][3] == 0
    assert length.max() == 8 and (length >= 3).sum() > 0.8 * n


def test_the_restated_jacobi_against_eigh():
    """v of the header's Jacobi against the eigenvector np.linalg.eigh gives for the same M, as points v[:3] / v[3] in float64."""
    case = ring_case()
    out = nt.run(case["store"], case["nq"], case["pairs"], case["img_off"], case["kp"], case["P"])
    M = nt.normal_matrices(out["track_off"], out["obs_node"], case["img_off"], case["kp"], case["P"], int(case["img_off"][-1]))
    v = nt.jacobi_smallest(M)
    w, U = np.linalg.eigh(M)
    u = U[:, :, 0]
    worst = float(np.abs(v[:, :3] / v[:, 3:] - u[:, :3] / u[:, 3:]).max())
    cond = float((w[:, 3] / np.abs(w[:, 0])).max())
    print(f"jacobi vs eigh over {len(M)} ring tracks: largest point difference {worst:.3e} (bound {EIGH_BOUND:.1e}), condition up to {cond:.2e}")
    assert len(M) == 400 and worst <= EIGH_BOUND
    # a diagonal M needs no rotation and returns the axis of its smallest entry; ties go to the lowest index
    assert nt.jacobi_smallest(np.diag([3.0, 1.0, 2.0, 1.0])[None])[0].tolist() == [0.0, 1.0, 0.0, 0.0]
