"""Guided matching (include/sfm_hip.h, "GUIDED"; docs/tracks.md §14): the 2-NN of every query among the train keypoints inside the
epipolar band of the essential matrix `verify.verify_pairs` left for its pair, as a second match store in the format of the global one.

`guided_match` and `guided_mutual` are the two launches; each takes and returns device tensors and never waits for the host.
`guided_pairs` composes them over chunks of pairs that share one `rev` buffer and returns the store `tracks.match_edges`,
`verify.survivors`, `verify.verify_pairs` and `tracks.run_tracks` take, with the mutual mask as their `keep`.  A query whose global
second neighbour was too close for the ratio test (repeated structure) gets a second chance among the few keypoints on its epipolar
line; a query the verification kept keeps its match (docs/tracks.md §14.2)."""
import numpy as np
import torch

from . import _lib
from ._lib import SfmHipError, check, on_device, ptr, require_cuda, stream_ptr
from .verify import DEFAULT_THRESHOLD, _i32, _n_img, _typed, _xn, normalise_keypoints, thr2_of

# docs/tracks.md §14.4: the rule "the smallest multiple of the verification threshold on the grid {1, 2, 4, 8} after which the correct
# matches of the final kept set grow by no more than one per cent in every scene class" does not settle inside the grid (the scenes of
# 50 keypoints an image still gain a third from x4 to x8, the two-view scenes of 500 gain 2.6 %), so the default is the grid's cap;
# min_inliers is the floor under which a pair's essential matrix is not trusted to guide (`verify.DEFAULT_HOMOGRAPHY["min_inliers"]`).
DEFAULT_GUIDED_THRESHOLD = 8 * DEFAULT_THRESHOLD
DEFAULT_MIN_INLIERS = 8
MAX_REV_BYTES = 256 << 20        # the rev buffer of `guided_pairs`: 3 355 pairs a chunk at 10 000 keypoints an image
DIM = 128
INT32_MAX = 2 ** 31 - 1


def _thr2g(thr2g):
    thr2g = float(thr2g)
    if thr2g != thr2g:
        raise SfmHipError("guided: thr2g is NaN")
    return thr2g


def _count(v, what):
    v = int(v)
    if not 0 <= v <= INT32_MAX:
        raise SfmHipError(f"guided: {what} must be 0..2^31-1 (got {v})")
    return v


def _pair_args(who, n_query, pairs, img_off):
    n_img = _n_img(img_off)
    require_cuda(n_query, pairs)
    if pairs.dtype != torch.int32 or pairs.dim() != 2 or pairs.shape[1] != 2 or not pairs.is_contiguous():
        raise SfmHipError(f"{who}: pairs must be a contiguous int32 [n_pairs, 2] device tensor")
    n_pairs = int(pairs.shape[0])
    _i32(n_query, "n_query", (n_pairs,))
    return n_img, n_pairs


def _rev(rev, n_pairs):
    require_cuda(rev)
    if rev.dtype != torch.int64 or rev.dim() != 2 or rev.shape[0] != n_pairs or not rev.is_contiguous():
        raise SfmHipError("guided: rev must be a contiguous int64 [n_pairs, stride] device tensor")
    stride = int(rev.shape[1])
    if n_pairs * stride > INT32_MAX:
        raise SfmHipError(f"guided: rev holds {n_pairs * stride} words, more than 2^31-1")
    return stride


def guided_match(desc, xn, E, active, n_query, pairs, img_off, cap, thr2g, out=None, rev=None):
    """sfm_guided_match: desc float32 [n_nodes, 128], xn float64 [n_nodes, 2] (`verify.normalise_keypoints`), E float64 [n_pairs, 9],
    active uint8 [n_pairs], n_query int32 [n_pairs], pairs int32 [n_pairs, 2], img_off int32 [n_img + 1]: device tensors.  thr2g:
    `verify.thr2_of(K, the guided threshold)`.  rev: int64 [n_pairs, stride] with stride >= the largest image (train keypoints past it
    are in no band; None: a row of n_nodes words a pair is allocated); it is cleared and filled with the uint64 keys (bits(d) << 32) | q
    of the best query of every train keypoint.
    Returns (store_g int32 [n_pairs, 2, cap, 2], rev).  No host wait."""
    n_img, n_pairs = _pair_args("guided_match", n_query, pairs, img_off)
    n_nodes, cap, thr2g = _xn(xn), _count(cap, "cap"), _thr2g(thr2g)
    _typed(desc, torch.float32, (n_nodes, DIM), "desc")
    _typed(E, torch.float64, (n_pairs, 9), "E")
    _typed(active, torch.uint8, (n_pairs,), "active")
    if n_pairs * cap > INT32_MAX:
        raise SfmHipError(f"guided_match: {n_pairs} pairs of {cap} queries exceed 2^31-1")
    dev = pairs.device
    if rev is None:                                                  # the sizes live on the device: no image is larger than all nodes
        if n_pairs * n_nodes > INT32_MAX:
            raise SfmHipError(f"guided_match: pass rev (int64 [n_pairs, the largest image]): {n_pairs} rows of all {n_nodes} nodes exceed 2^31-1")
        rev = torch.empty((n_pairs, n_nodes), dtype=torch.int64, device=dev)
    stride = _rev(rev, n_pairs)
    store = torch.empty((n_pairs, 2, cap, 2), dtype=torch.int32, device=dev) if out is None else _i32(out, "store_g", (n_pairs, 2, cap, 2))
    with on_device(dev):
        check(_lib.lib().sfm_guided_match(ptr(desc) if n_nodes else None, ptr(xn) if n_nodes else None, n_nodes, ptr(E) if n_pairs else None,
                                          ptr(active) if n_pairs else None, ptr(pairs) if n_pairs else None, ptr(n_query) if n_pairs else None,
                                          ptr(img_off), n_img, n_pairs, cap, thr2g, ptr(store) if n_pairs * cap else None,
                                          ptr(rev) if n_pairs * stride else None, n_pairs * stride * 8, stride, stream_ptr()), "sfm_guided_match")
    return store, rev


def guided_mutual(store_g, rev, n_query, pairs, img_off, out=None):
    """sfm_guided_mutual: (keep_g uint8 [n_pairs, cap]: 1 where the first neighbour of the query has the query as ITS best, info_g int32
    [n_pairs, 4]: queries in range, with >= 1 candidate, with >= 2, with keep_g set).  store_g, rev as `guided_match` leaves them.
    No host wait."""
    n_img, n_pairs = _pair_args("guided_mutual", n_query, pairs, img_off)
    require_cuda(store_g)
    if store_g.dtype != torch.int32 or store_g.dim() != 4 or tuple(store_g.shape[:2]) != (n_pairs, 2) or store_g.shape[3] != 2 or not store_g.is_contiguous():
        raise SfmHipError("guided_mutual: store_g must be a contiguous int32 [n_pairs, 2, cap, 2] device tensor")
    cap, stride, dev = int(store_g.shape[2]), _rev(rev, n_pairs), pairs.device
    if out is None:
        out = (torch.empty((n_pairs, cap), dtype=torch.uint8, device=dev), torch.empty((n_pairs, 4), dtype=torch.int32, device=dev))
    keep, info = _typed(out[0], torch.uint8, (n_pairs, cap), "keep_g"), _i32(out[1], "info_g", (n_pairs, 4))
    with on_device(dev):
        check(_lib.lib().sfm_guided_mutual(ptr(store_g) if n_pairs * cap else None, ptr(rev) if n_pairs * stride else None, n_pairs * stride * 8,
                                           stride, ptr(pairs) if n_pairs else None, ptr(n_query) if n_pairs else None, ptr(img_off), n_img, n_pairs,
                                           cap, ptr(keep) if n_pairs * cap else None, ptr(info) if n_pairs else None, stream_ptr()),
              "sfm_guided_mutual")
    return keep, info


def pairs_per_chunk(max_size, max_rev_bytes=MAX_REV_BYTES):
    """How many pairs `guided_pairs` matches at a time: their rev rows (8 bytes a train keypoint) fit `max_rev_bytes`."""
    return max(1, int(max_rev_bytes) // (8 * max(int(max_size), 1)))


def workspace_bytes(n_pairs, max_size, max_rev_bytes=MAX_REV_BYTES):
    """Bytes of the intermediate tensors `guided_pairs` allocates, without xn: the rev rows of one chunk and the active flags."""
    n_pairs, max_size = _count(n_pairs, "n_pairs"), _count(max_size, "max_size")
    step = min(pairs_per_chunk(max_size, max_rev_bytes), max(n_pairs, 1))
    return int(_lib.lib().sfm_guided_ws_bytes(step, max_size)) + n_pairs


def guided_pairs(desc, n_query, pairs, img_off, kp, K, E, info, threshold=DEFAULT_GUIDED_THRESHOLD, min_inliers=DEFAULT_MIN_INLIERS,
                 mutual=True, max_rev_bytes=MAX_REV_BYTES, cap=None, max_size=None):
    """All pairs guided by their essential matrices.  desc float32 [n_nodes, 128], n_query int32 [n_pairs], pairs int32 [n_pairs, 2],
    img_off int32 [n_img + 1], kp float32 [n_nodes, 2]: device tensors as `verify.verify_pairs` takes them; K: 3 x 3 on the host; E float64
    [n_pairs, 9] and info int32 [n_pairs, 8] as it returns them.  A pair is active when info[:, 2] >= min_inliers (a torch operation on the
    device).  threshold: the half-width of the band in pixels, as the verification's.  The pairs run in chunks of
    `pairs_per_chunk(max_size, max_rev_bytes)` that share one rev buffer; a word of the result does not depend on the chunking.
    cap (rows of the store) and max_size (the largest image) default to the largest image, read from img_off: ONE host wait; with both
    given there is none.  Returns dict(store= int32 [n_pairs, 2, cap, 2], keep= uint8 [n_pairs, cap] or None when mutual is False,
    info= int32 [n_pairs, 4] or None)."""
    n_img, n_pairs = _pair_args("guided_pairs", n_query, pairs, img_off)
    require_cuda(info)
    if info.dtype != torch.int32 or info.dim() != 2 or tuple(info.shape) != (n_pairs, 8) or not info.is_contiguous():
        raise SfmHipError("guided_pairs: info must be a contiguous int32 [n_pairs, 8] device tensor")
    if not float(threshold) > 0:
        raise SfmHipError(f"guided_pairs: the threshold must be positive (got {threshold!r})")
    if int(min_inliers) < 0 or int(max_rev_bytes) < 0:
        raise SfmHipError(f"guided_pairs: min_inliers and max_rev_bytes must not be negative (got {min_inliers!r}, {max_rev_bytes!r})")
    if cap is None or max_size is None:
        largest = int(np.diff(img_off.cpu().numpy().astype(np.int64)).max())                 # the one host wait
        cap = largest if cap is None else cap
        max_size = largest if max_size is None else max_size
    cap, max_size = _count(cap, "cap"), _count(max_size, "max_size")
    thr2g = thr2_of(K, threshold)
    xn = normalise_keypoints(kp, K)
    dev = pairs.device
    active = (info[:, 2] >= int(min_inliers)).to(torch.uint8)
    store = torch.empty((n_pairs, 2, cap, 2), dtype=torch.int32, device=dev)
    keep = torch.empty((n_pairs, cap), dtype=torch.uint8, device=dev) if mutual else None
    info_g = torch.empty((n_pairs, 4), dtype=torch.int32, device=dev) if mutual else None
    step = min(pairs_per_chunk(max_size, max_rev_bytes), max(n_pairs, 1))
    rev = torch.empty((step, max_size), dtype=torch.int64, device=dev)
    for a in range(0, n_pairs, step):
        b = min(a + step, n_pairs)
        guided_match(desc, xn, E[a:b], active[a:b], n_query[a:b], pairs[a:b], img_off, cap, thr2g, out=store[a:b], rev=rev[:b - a])
        if mutual:
            guided_mutual(store[a:b], rev[:b - a], n_query[a:b], pairs[a:b], img_off, out=(keep[a:b], info_g[a:b]))
    return dict(store=store, keep=keep, info=info_g)
