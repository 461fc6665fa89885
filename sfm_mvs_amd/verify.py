"""Geometric verification of all matched pairs at once (include/sfm_hip.h, "VERIFY"; docs/tracks.md §11).

`normalise_keypoints`, `survivors`, `samples`, `models`, `score` and `select` are the six launches; each takes and returns device
tensors and never waits for the host.  `verify_pairs` composes them and returns the `keep` mask `tracks.match_edges` takes, with every
pair's essential matrix, relative pose and eight words of bookkeeping; the last three launches run once per chunk of pairs, so the
models buffer is bounded (`MAX_MODELS_BYTES`).  A fixed budget of five-point hypotheses per pair, drawn by a
counter-based sampler, replaces the sequential RANSAC of `ransac.find_essential_mat`: the result is a function of the inputs and the
seed alone, and differs from the per-pair path's masks.

`top_models`, `local_optimise` and `pick` are the three launches of the local optimisation ("VERIFY-LO"; docs/tracks.md §12) that
`verify_pairs(lo=...)` puts between `score` and `select`: the best models of a pair refitted on their inliers and recounted.

`h_models`, `h_score` and `h_select` are the three launches of the homography ("VERIFY-H"; docs/tracks.md §13) that
`verify_pairs(homography=...)` runs after `select`: a second model per pair from the same survivors and samples, and with it `config`,
the word that tells a general pair from one that sees a plane or has no baseline (`pair_config`)."""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import SfmHipError, check, on_device, ptr, require_cuda, stream_ptr

MAX_BUDGET = 1024
# docs/tracks.md §11.4: the rule "the smallest budget past which neither the recall of planted inliers nor the share of planted outliers
# kept improves by more than a point at 30 % inliers" does not settle inside the admitted range (the recall still rises by 4 to 13 points
# from 512 to 1 024), so the default is the cap.
DEFAULT_BUDGET = 1024
DEFAULT_THRESHOLD = 0.4          # pixels, as HipVerifyEngine passes it to find_essential_mat
DEFAULT_SEED = 0
MAX_MODELS_BYTES = 256 << 20     # the models buffer of `verify_pairs`: 364 pairs a chunk at the default budget
SLOTS = 10                       # models per sample
FEW_SURVIVORS, NO_MODEL, NO_VOTE = 1, 2, 4
MAX_TOP, MAX_ROUNDS = 16, 8      # SFM_VERIFY_LO_MAX_TOP, SFM_VERIFY_LO_MAX_ROUNDS
# docs/tracks.md §12.4: the setting with the smallest top * rounds whose mean recall over the nine 30 % scenes is within a point of the
# best setting tried and whose share of planted outliers kept stays within a point of the plain path's on every (share, m) mean.
DEFAULT_LO = dict(top=1, rounds=1, widen=(3.0,))
CONFIG_NONE, CONFIG_GENERAL, CONFIG_PLANAR, CONFIG_ROTATING = 0, 1, 2, 3
H_MODEL_BYTES = 80               # a sample of `verify_pairs(homography=...)`: nine float64, its flag and its count
# docs/tracks.md §13.4: the threshold is the smallest of the grid at which keep_h recalls the planted inliers of the planar scenes no worse
# than keep recalls those of the general scenes; min_ratio and rot_spread are the geometric means of the two sides they separate.
DEFAULT_HOMOGRAPHY = dict(threshold=1.2, min_ratio=0.246, rot_spread=1.525, min_inliers=8, refit=1)


def _i32(t, what, shape):
    require_cuda(t)
    if t.dtype != torch.int32 or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
        raise SfmHipError(f"verify: {what} must be a contiguous int32 device tensor of shape {tuple(shape)}")
    return t


def _typed(t, dtype, shape, what):
    require_cuda(t)
    if t.dtype != dtype or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
        raise SfmHipError(f"verify: {what} must be a contiguous {dtype} device tensor of shape {tuple(shape)}")
    return t


def _K9(K):
    K = np.ascontiguousarray(np.asarray(K, np.float64).reshape(9))
    return K


def thr2_of(K, threshold=DEFAULT_THRESHOLD):
    """(float)(thr * thr) with thr = threshold / ((K[0] + K[4]) / 2), as sfm_find_essential_mat computes it."""
    K = _K9(K)
    thr = float(threshold) / ((K[0] + K[4]) / 2)
    return float(np.float32(thr * thr))


def _budget(budget):
    budget = int(budget)
    if not 1 <= budget <= MAX_BUDGET:
        raise SfmHipError(f"verify: the budget must be 1..{MAX_BUDGET} (got {budget})")
    return budget


def _n_img(img_off):
    require_cuda(img_off)
    if img_off.dtype != torch.int32 or img_off.dim() != 1 or img_off.numel() < 2 or not img_off.is_contiguous():
        raise SfmHipError("verify: img_off must be a contiguous int32 [n_img + 1] device tensor with n_img >= 1")
    return int(img_off.numel()) - 1


def _xn(xn):
    require_cuda(xn)
    if xn.dtype != torch.float64 or xn.dim() != 2 or xn.shape[1] != 2 or not xn.is_contiguous():
        raise SfmHipError("verify: xn must be a contiguous float64 [n_nodes, 2] device tensor")
    return int(xn.shape[0])


def _surv(surv):
    require_cuda(surv)
    if surv.dtype != torch.int32 or surv.dim() != 3 or surv.shape[2] != 2 or not surv.is_contiguous():
        raise SfmHipError("verify: surv must be a contiguous int32 [n_pairs, cap, 2] device tensor")
    return int(surv.shape[0]), int(surv.shape[1])


def normalise_keypoints(kp, K, out=None):
    """sfm_verify_normalise: kp float32 [n_nodes, 2] (all images concatenated) -> float64 [n_nodes, 2] K-normalised.  No host wait."""
    require_cuda(kp)
    if kp.dtype != torch.float32 or kp.dim() != 2 or kp.shape[1] != 2 or not kp.is_contiguous():
        raise SfmHipError("normalise_keypoints: kp must be a contiguous float32 [n_nodes, 2] device tensor")
    n = int(kp.shape[0])
    K = _K9(K)
    xn = torch.empty((n, 2), dtype=torch.float64, device=kp.device) if out is None else _typed(out, torch.float64, (n, 2), "xn")
    with on_device(kp.device):
        check(_lib.lib().sfm_verify_normalise(ptr(kp) if n else None, n, K.ctypes.data_as(ctypes.c_void_p), ptr(xn) if n else None, stream_ptr()),
              "sfm_verify_normalise")
    return xn


def survivors(store, n_query, pairs, img_off, ratio=0.70, out=None):
    """sfm_verify_survivors: the Lowe survivors of every pair of store (int32 [n_pairs, 2, cap, 2]) in ascending query order.
    Returns (surv int32 [n_pairs, cap, 2] = (q, t) then (-1, -1), m int32 [n_pairs]).  No host wait."""
    require_cuda(store)
    if store.dtype != torch.int32 or store.dim() != 4 or store.shape[1] != 2 or store.shape[3] != 2 or not store.is_contiguous():
        raise SfmHipError("survivors: store must be a contiguous int32 [n_pairs, 2, cap, 2] device tensor")
    n_pairs, cap, dev = int(store.shape[0]), int(store.shape[2]), store.device
    n_img = _n_img(img_off)
    _i32(n_query, "n_query", (n_pairs,))
    _i32(pairs, "pairs", (n_pairs, 2))
    if out is None:
        out = (torch.empty((n_pairs, cap, 2), dtype=torch.int32, device=dev), torch.empty(n_pairs, dtype=torch.int32, device=dev))
    surv, m = _i32(out[0], "surv", (n_pairs, cap, 2)), _i32(out[1], "m", (n_pairs,))
    ne = n_pairs * cap
    with on_device(dev):
        check(_lib.lib().sfm_verify_survivors(ptr(store) if ne else None, n_pairs, cap, ptr(pairs) if n_pairs else None,
                                              ptr(n_query) if n_pairs else None, ptr(img_off), n_img, float(ratio), ptr(surv) if ne else None,
                                              ptr(m) if n_pairs else None, stream_ptr()), "sfm_verify_survivors")
    return surv, m


def samples(m, budget=DEFAULT_BUDGET, seed=DEFAULT_SEED, out=None):
    """sfm_verify_samples: int32 [n_pairs, budget, 5] survivor indices, five times -1 where a sample could not be drawn.  No host wait."""
    require_cuda(m)
    if m.dtype != torch.int32 or m.dim() != 1 or not m.is_contiguous():
        raise SfmHipError("samples: m must be a contiguous int32 [n_pairs] device tensor")
    n_pairs, H = int(m.numel()), _budget(budget)
    samp = torch.empty((n_pairs, H, 5), dtype=torch.int32, device=m.device) if out is None else _i32(out, "samp", (n_pairs, H, 5))
    with on_device(m.device):
        check(_lib.lib().sfm_verify_samples(ptr(m) if n_pairs else None, n_pairs, H, int(seed) & 0xFFFFFFFF, ptr(samp) if n_pairs else None,
                                            stream_ptr()), "sfm_verify_samples")
    return samp


def models(samp, surv, m, pairs, img_off, xn, out=None):
    """sfm_verify_models: the five-point models of every sample, the bits `hostgeom.five_point` returns.
    Returns (nmodels int32 [n_pairs, H], E float64 [n_pairs, H, 10, 9], zero past nmodels).  No host wait."""
    n_pairs, cap = _surv(surv)
    n_img, n_nodes = _n_img(img_off), _xn(xn)
    require_cuda(samp)
    if samp.dtype != torch.int32 or samp.dim() != 3 or samp.shape[0] != n_pairs or samp.shape[2] != 5 or not samp.is_contiguous():
        raise SfmHipError("models: samp must be a contiguous int32 [n_pairs, H, 5] device tensor")
    H, dev = _budget(samp.shape[1]), surv.device
    _i32(m, "m", (n_pairs,))
    _i32(pairs, "pairs", (n_pairs, 2))
    if out is None:
        out = (torch.empty((n_pairs, H), dtype=torch.int32, device=dev), torch.empty((n_pairs, H, SLOTS, 9), dtype=torch.float64, device=dev))
    nmodels, E = _i32(out[0], "nmodels", (n_pairs, H)), _typed(out[1], torch.float64, (n_pairs, H, SLOTS, 9), "E")
    with on_device(dev):
        check(_lib.lib().sfm_verify_models(ptr(samp) if n_pairs else None, ptr(surv) if n_pairs * cap else None, ptr(m) if n_pairs else None,
                                           ptr(pairs) if n_pairs else None, ptr(img_off), n_img, ptr(xn) if n_nodes else None, n_nodes, n_pairs,
                                           cap, H, ptr(nmodels) if n_pairs else None, ptr(E) if n_pairs else None, stream_ptr()),
              "sfm_verify_models")
    return nmodels, E


def _scored(who, E, nmodels, surv, m, pairs, img_off, xn):
    n_pairs, cap = _surv(surv)
    n_img, n_nodes = _n_img(img_off), _xn(xn)
    require_cuda(E, nmodels)
    if nmodels.dtype != torch.int32 or nmodels.dim() != 2 or nmodels.shape[0] != n_pairs or not nmodels.is_contiguous():
        raise SfmHipError(f"{who}: nmodels must be a contiguous int32 [n_pairs, H] device tensor")
    H = _budget(nmodels.shape[1])
    _typed(E, torch.float64, (n_pairs, H, SLOTS, 9), "E")
    _i32(m, "m", (n_pairs,))
    _i32(pairs, "pairs", (n_pairs, 2))
    return n_pairs, cap, n_img, n_nodes, H


def score(E, nmodels, surv, m, pairs, img_off, xn, thr2, out=None):
    """sfm_verify_score: (counts int32 [n_pairs, H, 10], best int64 [n_pairs] holding the uint64 key
    (count << 32) | (0xFFFFFFFF - (10 s + j)) of the best model, 0 without one).  thr2: `thr2_of(K, threshold)`.  No host wait."""
    n_pairs, cap, n_img, n_nodes, H = _scored("score", E, nmodels, surv, m, pairs, img_off, xn)
    dev = surv.device
    if out is None:
        out = (torch.empty((n_pairs, H, SLOTS), dtype=torch.int32, device=dev), torch.empty(n_pairs, dtype=torch.int64, device=dev))
    counts, best = _i32(out[0], "counts", (n_pairs, H, SLOTS)), _typed(out[1], torch.int64, (n_pairs,), "best")
    with on_device(dev):
        check(_lib.lib().sfm_verify_score(ptr(E) if n_pairs else None, ptr(nmodels) if n_pairs else None, ptr(surv) if n_pairs * cap else None,
                                          ptr(m) if n_pairs else None, ptr(pairs) if n_pairs else None, ptr(img_off), n_img,
                                          ptr(xn) if n_nodes else None, n_nodes, n_pairs, cap, H, float(thr2), ptr(counts) if n_pairs else None,
                                          ptr(best) if n_pairs else None, stream_ptr()), "sfm_verify_score")
    return counts, best


def select(E, nmodels, best, surv, m, pairs, img_off, xn, thr2, out=None):
    """sfm_verify_select: (keep uint8 [n_pairs, cap], E float64 [n_pairs, 9], Rt float64 [n_pairs, 12], info int32 [n_pairs, 8]) of the
    best model of every pair.  No host wait."""
    n_pairs, cap, n_img, n_nodes, H = _scored("select", E, nmodels, surv, m, pairs, img_off, xn)
    dev = surv.device
    _typed(best, torch.int64, (n_pairs,), "best")
    if out is None:
        out = (torch.empty((n_pairs, cap), dtype=torch.uint8, device=dev), torch.empty((n_pairs, 9), dtype=torch.float64, device=dev),
               torch.empty((n_pairs, 12), dtype=torch.float64, device=dev), torch.empty((n_pairs, 8), dtype=torch.int32, device=dev))
    keep, Eb, Rt, info = out
    _typed(keep, torch.uint8, (n_pairs, cap), "keep")
    _typed(Eb, torch.float64, (n_pairs, 9), "E_out")
    _typed(Rt, torch.float64, (n_pairs, 12), "Rt")
    _i32(info, "info", (n_pairs, 8))
    with on_device(dev):
        check(_lib.lib().sfm_verify_select(ptr(E) if n_pairs else None, ptr(nmodels) if n_pairs else None, ptr(best) if n_pairs else None,
                                           ptr(surv) if n_pairs * cap else None, ptr(m) if n_pairs else None, ptr(pairs) if n_pairs else None,
                                           ptr(img_off), n_img, ptr(xn) if n_nodes else None, n_nodes, n_pairs, cap, H, float(thr2),
                                           ptr(keep) if n_pairs * cap else None, ptr(Eb) if n_pairs else None, ptr(Rt) if n_pairs else None,
                                           ptr(info) if n_pairs else None, stream_ptr()), "sfm_verify_select")
    return keep, Eb, Rt, info


def _top(top):
    top = int(top)
    if not 1 <= top <= MAX_TOP:
        raise SfmHipError(f"verify: top must be 1..{MAX_TOP} (got {top})")
    return top


def top_models(counts, nmodels, top, out=None):
    """sfm_verify_top: int64 [n_pairs, top] holding the uint64 keys of the `top` best models of every pair in descending order, then
    zeros; column 0 is `score`'s best.  counts int32 [n_pairs, H, 10], nmodels int32 [n_pairs, H].  No host wait."""
    require_cuda(counts, nmodels)
    if nmodels.dtype != torch.int32 or nmodels.dim() != 2 or not nmodels.is_contiguous():
        raise SfmHipError("top_models: nmodels must be a contiguous int32 [n_pairs, H] device tensor")
    n_pairs, H, T = int(nmodels.shape[0]), _budget(nmodels.shape[1]), _top(top)
    _i32(counts, "counts", (n_pairs, H, SLOTS))
    keys = torch.empty((n_pairs, T), dtype=torch.int64, device=nmodels.device) if out is None else _typed(out, torch.int64, (n_pairs, T), "top")
    with on_device(nmodels.device):
        check(_lib.lib().sfm_verify_top(ptr(counts) if n_pairs else None, ptr(nmodels) if n_pairs else None, n_pairs, H, T,
                                        ptr(keys) if n_pairs else None, stream_ptr()), "sfm_verify_top")
    return keys


def _wide2(wide2):
    w = np.ascontiguousarray(np.asarray(wide2, np.float32).reshape(-1))
    if len(w) > MAX_ROUNDS or np.isnan(w).any():
        raise SfmHipError(f"verify: wide2 must hold 0..{MAX_ROUNDS} squared thresholds, none a NaN (got {w.tolist()})")
    return w


def local_optimise(E, top, surv, m, pairs, img_off, xn, thr2, wide2, out=None):
    """sfm_verify_lo: every candidate of `top` (int64 [n_pairs, T], as `top_models` leaves it) refitted len(wide2) times on its inliers
    under the squared thresholds wide2 (floats on the host, `thr2_of(K, widen * threshold)`) and recounted at thr2.
    Returns (E_lo float64 [n_pairs, T, 9], n_lo int32 [n_pairs, T], round_lo int32 [n_pairs, T]): the best of each candidate and its
    refits, its inlier count, and the round that produced it (-1: the candidate itself).  No host wait."""
    n_pairs, cap = _surv(surv)
    n_img, n_nodes = _n_img(img_off), _xn(xn)
    require_cuda(E, top)
    if E.dtype != torch.float64 or E.dim() != 4 or E.shape[0] != n_pairs or tuple(E.shape[2:]) != (SLOTS, 9) or not E.is_contiguous():
        raise SfmHipError("local_optimise: E must be a contiguous float64 [n_pairs, H, 10, 9] device tensor")
    H, dev = _budget(E.shape[1]), surv.device
    if top.dtype != torch.int64 or top.dim() != 2 or top.shape[0] != n_pairs or not top.is_contiguous():
        raise SfmHipError("local_optimise: top must be a contiguous int64 [n_pairs, T] device tensor")
    T, w = _top(top.shape[1]), _wide2(wide2)
    _i32(m, "m", (n_pairs,))
    _i32(pairs, "pairs", (n_pairs, 2))
    if out is None:
        out = (torch.empty((n_pairs, T, 9), dtype=torch.float64, device=dev), torch.empty((n_pairs, T), dtype=torch.int32, device=dev),
               torch.empty((n_pairs, T), dtype=torch.int32, device=dev))
    E_lo, n_lo, round_lo = _typed(out[0], torch.float64, (n_pairs, T, 9), "E_lo"), _i32(out[1], "n_lo", (n_pairs, T)), _i32(out[2], "round_lo", (n_pairs, T))
    with on_device(dev):
        check(_lib.lib().sfm_verify_lo(ptr(E) if n_pairs else None, ptr(top) if n_pairs else None, T, ptr(surv) if n_pairs * cap else None,
                                       ptr(m) if n_pairs else None, ptr(pairs) if n_pairs else None, ptr(img_off), n_img,
                                       ptr(xn) if n_nodes else None, n_nodes, n_pairs, cap, H, float(thr2), len(w),
                                       w.ctypes.data_as(ctypes.c_void_p) if len(w) else None, ptr(E_lo) if n_pairs else None,
                                       ptr(n_lo) if n_pairs else None, ptr(round_lo) if n_pairs else None, stream_ptr()), "sfm_verify_lo")
    return E_lo, n_lo, round_lo


def pick(top, E_lo, n_lo, round_lo, budget, out=None):
    """sfm_verify_lo_pick: the candidate with the most inliers of every pair (the lowest on ties), as the one-sample models buffer
    `select` takes.  `budget`: the H of the models the keys of `top` index.  Returns (E_sel float64 [n_pairs, 1, 10, 9], nmodels_sel int32
    [n_pairs, 1], best_sel int64 [n_pairs], lo_info int32 [n_pairs, 8] = plain best count, LO count, winning candidate, its round, its
    origin sample and model, candidates that had a model, 0).  No host wait."""
    require_cuda(top, E_lo, n_lo, round_lo)
    if top.dtype != torch.int64 or top.dim() != 2 or not top.is_contiguous():
        raise SfmHipError("pick: top must be a contiguous int64 [n_pairs, T] device tensor")
    n_pairs, T, H, dev = int(top.shape[0]), _top(top.shape[1]), _budget(budget), top.device
    _typed(E_lo, torch.float64, (n_pairs, T, 9), "E_lo")
    _i32(n_lo, "n_lo", (n_pairs, T))
    _i32(round_lo, "round_lo", (n_pairs, T))
    if out is None:
        out = (torch.empty((n_pairs, 1, SLOTS, 9), dtype=torch.float64, device=dev), torch.empty((n_pairs, 1), dtype=torch.int32, device=dev),
               torch.empty(n_pairs, dtype=torch.int64, device=dev), torch.empty((n_pairs, 8), dtype=torch.int32, device=dev))
    E_sel, nm_sel, best_sel, lo_info = out
    _typed(E_sel, torch.float64, (n_pairs, 1, SLOTS, 9), "E_sel")
    _i32(nm_sel, "nmodels_sel", (n_pairs, 1))
    _typed(best_sel, torch.int64, (n_pairs,), "best_sel")
    _i32(lo_info, "lo_info", (n_pairs, 8))
    with on_device(dev):
        check(_lib.lib().sfm_verify_lo_pick(*(ptr(t) if n_pairs else None for t in (top, E_lo, n_lo, round_lo)), n_pairs, H, T,
                                            *(ptr(t) if n_pairs else None for t in (E_sel, nm_sel, best_sel, lo_info)), stream_ptr()),
              "sfm_verify_lo_pick")
    return E_sel, nm_sel, best_sel, lo_info


def _h_models_args(who, Hm, ok, surv, m, pairs, img_off, xn):
    n_pairs, cap = _surv(surv)
    n_img, n_nodes = _n_img(img_off), _xn(xn)
    require_cuda(Hm, ok)
    if ok.dtype != torch.int32 or ok.dim() != 2 or ok.shape[0] != n_pairs or not ok.is_contiguous():
        raise SfmHipError(f"{who}: ok must be a contiguous int32 [n_pairs, H] device tensor")
    H = _budget(ok.shape[1])
    _typed(Hm, torch.float64, (n_pairs, H, 9), "Hm")
    _i32(m, "m", (n_pairs,))
    _i32(pairs, "pairs", (n_pairs, 2))
    return n_pairs, cap, n_img, n_nodes, H


def _thr2h(thr2h):
    thr2h = float(thr2h)
    if thr2h != thr2h:
        raise SfmHipError("verify: thr2h is NaN")
    return thr2h


def h_models(samp, surv, m, pairs, img_off, xn, out=None):
    """sfm_verify_h_models: the four-point homography of the first four slots of every sample of `samples`, the bits
    `hostgeom.homography4` returns.  Returns (ok int32 [n_pairs, H], Hm float64 [n_pairs, H, 9], zero without a model).  No host wait."""
    n_pairs, cap = _surv(surv)
    n_img, n_nodes = _n_img(img_off), _xn(xn)
    require_cuda(samp)
    if samp.dtype != torch.int32 or samp.dim() != 3 or samp.shape[0] != n_pairs or samp.shape[2] != 5 or not samp.is_contiguous():
        raise SfmHipError("h_models: samp must be a contiguous int32 [n_pairs, H, 5] device tensor")
    H, dev = _budget(samp.shape[1]), surv.device
    _i32(m, "m", (n_pairs,))
    _i32(pairs, "pairs", (n_pairs, 2))
    if out is None:
        out = (torch.empty((n_pairs, H), dtype=torch.int32, device=dev), torch.empty((n_pairs, H, 9), dtype=torch.float64, device=dev))
    ok, Hm = _i32(out[0], "ok", (n_pairs, H)), _typed(out[1], torch.float64, (n_pairs, H, 9), "Hm")
    with on_device(dev):
        check(_lib.lib().sfm_verify_h_models(ptr(samp) if n_pairs else None, ptr(surv) if n_pairs * cap else None, ptr(m) if n_pairs else None,
                                             ptr(pairs) if n_pairs else None, ptr(img_off), n_img, ptr(xn) if n_nodes else None, n_nodes, n_pairs,
                                             cap, H, ptr(ok) if n_pairs else None, ptr(Hm) if n_pairs else None, stream_ptr()),
              "sfm_verify_h_models")
    return ok, Hm


def h_score(Hm, ok, surv, m, pairs, img_off, xn, thr2h, out=None):
    """sfm_verify_h_score: (counts int32 [n_pairs, H], best int64 [n_pairs] holding the uint64 key (count << 32) | (0xFFFFFFFF - s) of the
    best sample, 0 without one) under the transfer error of x1 -> x2.  thr2h: `thr2_of(K, the homography's threshold)`.  No host wait."""
    n_pairs, cap, n_img, n_nodes, H = _h_models_args("h_score", Hm, ok, surv, m, pairs, img_off, xn)
    thr2h, dev = _thr2h(thr2h), surv.device
    if out is None:
        out = (torch.empty((n_pairs, H), dtype=torch.int32, device=dev), torch.empty(n_pairs, dtype=torch.int64, device=dev))
    counts, best = _i32(out[0], "counts", (n_pairs, H)), _typed(out[1], torch.int64, (n_pairs,), "best")
    with on_device(dev):
        check(_lib.lib().sfm_verify_h_score(ptr(Hm) if n_pairs else None, ptr(ok) if n_pairs else None, ptr(surv) if n_pairs * cap else None,
                                            ptr(m) if n_pairs else None, ptr(pairs) if n_pairs else None, ptr(img_off), n_img,
                                            ptr(xn) if n_nodes else None, n_nodes, n_pairs, cap, H, thr2h, ptr(counts) if n_pairs else None,
                                            ptr(best) if n_pairs else None, stream_ptr()), "sfm_verify_h_score")
    return counts, best


def h_select(Hm, ok, best, surv, m, pairs, img_off, xn, thr2h, refit=1, out=None):
    """sfm_verify_h_select: (keep_h uint8 [n_pairs, cap], H float64 [n_pairs, 9] scaled to a middle singular value of 1, sv float64
    [n_pairs, 3] descending with sv[:, 1] = 1, h_info int32 [n_pairs, 8]) of the best sample of every pair, refitted once on its inliers
    when `refit` is 1 and kept only when that counts strictly more.  No host wait."""
    n_pairs, cap, n_img, n_nodes, H = _h_models_args("h_select", Hm, ok, surv, m, pairs, img_off, xn)
    thr2h, dev = _thr2h(thr2h), surv.device
    if refit not in (0, 1):
        raise SfmHipError(f"h_select: refit must be 0 or 1 (got {refit!r})")
    _typed(best, torch.int64, (n_pairs,), "best")
    if out is None:
        out = (torch.empty((n_pairs, cap), dtype=torch.uint8, device=dev), torch.empty((n_pairs, 9), dtype=torch.float64, device=dev),
               torch.empty((n_pairs, 3), dtype=torch.float64, device=dev), torch.empty((n_pairs, 8), dtype=torch.int32, device=dev))
    keep_h, Hb, sv, h_info = out
    _typed(keep_h, torch.uint8, (n_pairs, cap), "keep_h")
    _typed(Hb, torch.float64, (n_pairs, 9), "H_out")
    _typed(sv, torch.float64, (n_pairs, 3), "sv")
    _i32(h_info, "h_info", (n_pairs, 8))
    with on_device(dev):
        check(_lib.lib().sfm_verify_h_select(ptr(Hm) if n_pairs else None, ptr(ok) if n_pairs else None, ptr(best) if n_pairs else None,
                                             ptr(surv) if n_pairs * cap else None, ptr(m) if n_pairs else None, ptr(pairs) if n_pairs else None,
                                             ptr(img_off), n_img, ptr(xn) if n_nodes else None, n_nodes, n_pairs, cap, H, thr2h, int(refit),
                                             ptr(keep_h) if n_pairs * cap else None, ptr(Hb) if n_pairs else None, ptr(sv) if n_pairs else None,
                                             ptr(h_info) if n_pairs else None, stream_ptr()), "sfm_verify_h_select")
    return keep_h, Hb, sv, h_info


def homography_settings(homography):
    """`homography=True` or dict(threshold=, min_ratio=, rot_spread=, min_inliers=, refit=) -> the full dict, missing keys from
    `DEFAULT_HOMOGRAPHY`; None for homography=None."""
    if homography is None or homography is False:
        return None
    if homography is True:
        homography = {}
    if not isinstance(homography, dict) or set(homography) - set(DEFAULT_HOMOGRAPHY):
        raise SfmHipError(f"verify: homography must be None, True or a dict of {', '.join(DEFAULT_HOMOGRAPHY)} (got {homography!r})")
    s = dict(DEFAULT_HOMOGRAPHY, **homography)
    try:
        s = dict(threshold=float(s["threshold"]), min_ratio=float(s["min_ratio"]), rot_spread=float(s["rot_spread"]),
                 min_inliers=int(s["min_inliers"]), refit=int(s["refit"]))
    except (TypeError, ValueError) as e:
        raise SfmHipError(f"verify: homography settings must be numbers (got {homography!r})") from e
    if not s["threshold"] > 0 or not s["min_ratio"] >= 0 or not s["rot_spread"] >= 1 or s["min_inliers"] < 0 or s["refit"] not in (0, 1):
        raise SfmHipError(f"verify: homography needs threshold > 0, min_ratio >= 0, rot_spread >= 1, min_inliers >= 0 and refit 0 or 1 (got {s})")
    return s


def pair_config(info, h_info, h_sv, settings):
    """The two-view configuration word of every pair, int32 [n_pairs], by torch operations on the device (no host wait): NONE when the
    essential matrix has fewer than min_inliers Sampson inliers; otherwise GENERAL when the homography explains fewer than min_ratio of
    them; otherwise ROTATING when its singular values spread by no more than rot_spread, else PLANAR."""
    n_E, n_H = info[:, 2].to(torch.float64), h_info[:, 2].to(torch.float64)
    word = torch.where(h_sv[:, 0] / h_sv[:, 2] <= settings["rot_spread"], CONFIG_ROTATING, CONFIG_PLANAR)
    word = torch.where(n_H < settings["min_ratio"] * n_E, CONFIG_GENERAL, word)
    return torch.where(info[:, 2] < settings["min_inliers"], CONFIG_NONE, word).to(torch.int32)


def lo_settings(lo):
    """`lo=True` or dict(top=, rounds=, widen=) -> (top, widen tuple of `rounds` multipliers of the threshold); None for lo=None."""
    if lo is None or lo is False:
        return None
    if lo is True:
        lo = {}
    if not isinstance(lo, dict) or set(lo) - {"top", "rounds", "widen"}:
        raise SfmHipError(f"verify: lo must be None, True or a dict of top, rounds, widen (got {lo!r})")
    top = _top(lo.get("top", DEFAULT_LO["top"]))
    widen = lo.get("widen")
    if widen is None:                                               # the default's multiplier in every round
        widen = (DEFAULT_LO["widen"][0],) * int(lo.get("rounds", DEFAULT_LO["rounds"]))
    widen = tuple(float(w) for w in widen)
    rounds = lo.get("rounds", len(widen))
    if not 0 <= int(rounds) <= MAX_ROUNDS or len(widen) != int(rounds) or any(not w > 0 for w in widen):
        raise SfmHipError(f"verify: lo needs rounds in 0..{MAX_ROUNDS} and as many positive multipliers in widen (got rounds {rounds}, widen {widen})")
    return top, widen


def pairs_per_chunk(budget=DEFAULT_BUDGET, max_models_bytes=MAX_MODELS_BYTES):
    """How many pairs `verify_pairs` solves, scores and selects at a time: the models of a chunk (720 bytes a sample) fit `max_models_bytes`."""
    return max(1, int(max_models_bytes) // (_budget(budget) * SLOTS * 72))


def verify_pairs(store, n_query, pairs, img_off, kp, K, ratio=0.70, threshold=DEFAULT_THRESHOLD, budget=DEFAULT_BUDGET, seed=DEFAULT_SEED,
                 max_models_bytes=MAX_MODELS_BYTES, lo=None, homography=None):
    """All pairs in a fixed number of launches and no host wait.  store int32 [n_pairs, 2, cap, 2], n_query int32 [n_pairs], pairs int32
    [n_pairs, 2], img_off int32 [n_img + 1], kp float32 [n_nodes, 2]: device tensors, as `tracks.match_edges` takes them; K: 3 x 3 on the
    host.  Keypoints, survivors and samples are computed for all pairs at once (three launches); models, scores and the selection run over
    chunks of `pairs_per_chunk(budget, max_models_bytes)` pairs (three launches and two clears a chunk) that share one models buffer, so the
    workspace does not grow with the number of pairs beyond the survivors and samples.  A sample is a function of (seed, pair, sample), so
    the chunking does not change a word of the result.
    Returns a dict of device tensors: keep uint8 [n_pairs, cap] (what `match_edges(keep=...)` takes), E float64 [n_pairs, 9],
    Rt float64 [n_pairs, 12] (the relative pose [R | t], 3 x 4 row-major, |t| = 1), info int32 [n_pairs, 8] (survivors, models scored,
    Sampson inliers, cheirality inliers, best sample, best model, winning candidate, status bits).
    lo: None (the plain path, launch for launch), True (`DEFAULT_LO`) or dict(top=, rounds=, widen=): local optimisation (docs/tracks.md
    §12) of the `top` best models of every pair, `rounds` refits each on the inliers under widen[r] * threshold; three more launches a
    chunk between `score` and `select`, which then runs on the winner alone.  The Sampson inliers of a pair (info[:, 2]) are never fewer
    than without; best sample and best model name the five-point model the winner was refitted from; the dict gains lo_info int32
    [n_pairs, 8] (plain best count, LO count, winning candidate, its round or -1, origin sample, origin model, candidates, 0).
    homography: None (no further launch), True (`DEFAULT_HOMOGRAPHY`) or dict(threshold=, min_ratio=, rot_spread=, min_inliers=, refit=):
    a homography per pair beside the essential matrix (docs/tracks.md §13), from the same survivors and the first four slots of the same
    samples; three more launches a chunk after `select`, with or without `lo`.  keep, E, Rt and info stay the words they are without it;
    the dict gains H float64 [n_pairs, 9] (middle singular value 1), keep_h uint8 [n_pairs, cap], h_sv float64 [n_pairs, 3], h_info int32
    [n_pairs, 8] (survivors, samples with a model, inliers, the sample's inliers before the refit, best sample, 0 when the refit won else
    -1, 0, status bits) and config int32 [n_pairs] (`CONFIG_NONE`, `_GENERAL`, `_PLANAR`, `_ROTATING`; `pair_config`)."""
    settings = lo_settings(lo)
    hs = homography_settings(homography)
    thr2 = thr2_of(K, threshold)
    xn = normalise_keypoints(kp, K)
    surv, m = survivors(store, n_query, pairs, img_off, ratio)
    samp = samples(m, budget, seed)
    n_pairs, cap, H, dev = int(surv.shape[0]), int(surv.shape[1]), int(samp.shape[1]), surv.device
    keep = torch.empty((n_pairs, cap), dtype=torch.uint8, device=dev)
    Eb = torch.empty((n_pairs, 9), dtype=torch.float64, device=dev)
    Rt = torch.empty((n_pairs, 12), dtype=torch.float64, device=dev)
    info = torch.empty((n_pairs, 8), dtype=torch.int32, device=dev)
    step = min(pairs_per_chunk(H, max_models_bytes), max(n_pairs, 1))
    nmodels = torch.empty((step, H), dtype=torch.int32, device=dev)
    E = torch.empty((step, H, SLOTS, 9), dtype=torch.float64, device=dev)
    counts = torch.empty((step, H, SLOTS), dtype=torch.int32, device=dev)
    best = torch.empty(step, dtype=torch.int64, device=dev)
    if settings is not None:
        T, widen = settings
        wide2 = [thr2_of(K, w * float(threshold)) for w in widen]
        lo_info = torch.empty((n_pairs, 8), dtype=torch.int32, device=dev)
        top = torch.empty((step, T), dtype=torch.int64, device=dev)
        cand = (torch.empty((step, T, 9), dtype=torch.float64, device=dev), torch.empty((step, T), dtype=torch.int32, device=dev),
                torch.empty((step, T), dtype=torch.int32, device=dev))
        E_sel = torch.empty((step, 1, SLOTS, 9), dtype=torch.float64, device=dev)
        nm_sel = torch.empty((step, 1), dtype=torch.int32, device=dev)
        best_sel = torch.empty(step, dtype=torch.int64, device=dev)
    if hs is not None:
        thr2h = thr2_of(K, hs["threshold"])
        h_out = (torch.empty((n_pairs, cap), dtype=torch.uint8, device=dev), torch.empty((n_pairs, 9), dtype=torch.float64, device=dev),
                 torch.empty((n_pairs, 3), dtype=torch.float64, device=dev), torch.empty((n_pairs, 8), dtype=torch.int32, device=dev))
        ok_h = torch.empty((step, H), dtype=torch.int32, device=dev)
        Hm = torch.empty((step, H, 9), dtype=torch.float64, device=dev)
        counts_h = torch.empty((step, H), dtype=torch.int32, device=dev)
        best_h = torch.empty(step, dtype=torch.int64, device=dev)

    def homographies(a, b, part):
        k = b - a
        h_models(samp[a:b], *part, out=(ok_h[:k], Hm[:k]))
        h_score(Hm[:k], ok_h[:k], *part, thr2h, out=(counts_h[:k], best_h[:k]))
        h_select(Hm[:k], ok_h[:k], best_h[:k], *part, thr2h, hs["refit"], out=tuple(t[a:b] for t in h_out))

    for a in range(0, n_pairs, step):
        b = min(a + step, n_pairs)
        k = b - a
        part = (surv[a:b], m[a:b], pairs[a:b], img_off, xn)
        models(samp[a:b], *part, out=(nmodels[:k], E[:k]))
        score(E[:k], nmodels[:k], *part, thr2, out=(counts[:k], best[:k]))
        if settings is None:
            select(E[:k], nmodels[:k], best[:k], *part, thr2, out=(keep[a:b], Eb[a:b], Rt[a:b], info[a:b]))
            if hs is not None:
                homographies(a, b, part)
            continue
        top_models(counts[:k], nmodels[:k], T, out=top[:k])
        local_optimise(E[:k], top[:k], *part, thr2, wide2, out=tuple(t[:k] for t in cand))
        pick(top[:k], *(t[:k] for t in cand), H, out=(E_sel[:k], nm_sel[:k], best_sel[:k], lo_info[a:b]))
        select(E_sel[:k], nm_sel[:k], best_sel[:k], *part, thr2, out=(keep[a:b], Eb[a:b], Rt[a:b], info[a:b]))
        # `select` saw one sample of one model: models scored, best sample and best model keep their documented meaning
        info[a:b, 1] = nmodels[:k].clamp(0, SLOTS).sum(1, dtype=torch.int32)
        info[a:b, 4:6] = lo_info[a:b, 4:6]
        if hs is not None:
            homographies(a, b, part)
    out = dict(keep=keep, E=Eb, Rt=Rt, info=info)
    if settings is not None:
        out["lo_info"] = lo_info
    if hs is not None:
        out.update(keep_h=h_out[0], H=h_out[1], h_sv=h_out[2], h_info=h_out[3], config=pair_config(info, h_out[3], h_out[2], hs))
    return out


def workspace_bytes(n_pairs, cap, budget=DEFAULT_BUDGET, max_models_bytes=MAX_MODELS_BYTES, lo=None, homography=None):
    """Bytes of the intermediate tensors `verify_pairs` allocates, without xn: survivors and samples of all pairs, and the models, model
    counts, inlier counts and best keys of one chunk; with `lo`, the keys, models, counts and rounds of a chunk's candidates and its
    one-sample models buffer as well; with `homography`, the models, flags, counts (80 bytes a sample) and best keys of a chunk."""
    n_pairs, cap, H = int(n_pairs), int(cap), int(budget)
    step = min(pairs_per_chunk(H, max_models_bytes), max(n_pairs, 1))
    total = n_pairs * (cap * 8 + 4 + H * 20) + step * (H * (4 + SLOTS * 72 + SLOTS * 4) + 8)
    settings = lo_settings(lo)
    if settings is not None:
        total += step * (settings[0] * (8 + 72 + 4 + 4) + SLOTS * 72 + 4 + 8)
    if homography_settings(homography) is not None:
        total += step * (H * H_MODEL_BYTES + 8)
    return total


def confidence_iters(info, prob=0.999):
    """The iteration bound of sequential RANSAC (`ransac_update_num_iters`: log(1 - prob) / log(1 - w^5)) at the inlier ratio w each
    pair achieved (Sampson inliers / survivors): a pair whose bound exceeds the budget was not covered with confidence `prob`.
    info: the int32 [n_pairs, 8] of `verify_pairs` (a device tensor is downloaded: a host wait).  Returns float64 [n_pairs]; inf where
    no model was found, 0 where every survivor is an inlier."""
    info = info.cpu().numpy() if isinstance(info, torch.Tensor) else np.asarray(info)
    m, inl = info[:, 0].astype(np.float64), info[:, 2].astype(np.float64)
    w = np.divide(inl, m, out=np.zeros_like(m), where=m > 0)
    out = np.full(len(m), np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        denom = 1.0 - w ** 5
        num = np.log(max(1.0 - float(prob), np.finfo(np.float64).tiny))
        ok = (w > 0) & (denom >= np.finfo(np.float64).tiny)
        out[ok] = np.rint(num / np.log(denom[ok]))
        out[(w > 0) & ~ok] = 0.0
    return out
