"""Image retrieval (include/sfm_hip.h, "RETRIEVAL"; docs/retrieval.md): one VLAD signature per image and a shortlist of the pairs worth
matching, for collections without an order: what `match_pairs_sharded`, `verify_pairs`, `guided_pairs`, `match_edges` and `run_tracks`
take in place of `all_pairs`.

`assign_accumulate`, `update_centres`, `train_vocabulary`, `signatures`, `shortlist` and `pair_list` take and return device tensors and
never wait for the host.  `select_pairs` composes them and waits once, for the download of the pair list."""
import math

import numpy as np
import torch

from . import _lib
from ._lib import SfmHipError, check, on_device, ptr, require_cuda, stream_ptr
from .mvs import _upload

DIM = 128
MAX_CENTRES = 256
MAX_K = 64
MAX_IMAGES = 65536
MAX_SHORTLIST_IMAGES = 16384
DEFAULT_QS = 127.0
DEFAULT_VALUE_RANGE = 256.0
INT32_MAX = 2 ** 31 - 1


def scale_of(value_range=DEFAULT_VALUE_RANGE):
    """The fixed-point scale of the VLAD sums: the power of two with value_range * scale = 2^20 (value_range rounded up to a power of
    two), so a sum of 2^40 terms of full range still fits the int64 accumulator."""
    value_range = float(value_range)
    if not (0.0 < value_range < math.inf):
        raise SfmHipError(f"retrieval: value_range must be positive and finite (got {value_range!r})")
    return float(2.0 ** (20 - math.ceil(math.log2(value_range))))


def _positive(v, what):
    v = float(v)
    if not (0.0 < v < math.inf):
        raise SfmHipError(f"retrieval: {what} must be positive and finite (got {v!r})")
    return v


def _typed(t, dtype, shape, what):
    require_cuda(t)
    if t.dtype != dtype or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
        raise SfmHipError(f"retrieval: {what} must be a contiguous {dtype} device tensor of shape {tuple(shape)}")
    return t


def _desc(desc):
    require_cuda(desc)
    if desc.dtype != torch.float32 or desc.dim() != 2 or desc.shape[1] != DIM or not desc.is_contiguous():
        raise SfmHipError("retrieval: desc must be a contiguous float32 [n_nodes, 128] device tensor")
    if int(desc.shape[0]) > INT32_MAX:
        raise SfmHipError("retrieval: more than 2^31-1 nodes")
    return int(desc.shape[0])


def _centres(centres):
    require_cuda(centres)
    if centres.dtype != torch.float32 or centres.dim() != 2 or centres.shape[1] != DIM or not centres.is_contiguous():
        raise SfmHipError("retrieval: centres must be a contiguous float32 [C, 128] device tensor")
    C = int(centres.shape[0])
    if not 1 <= C <= MAX_CENTRES:
        raise SfmHipError(f"retrieval: 1..{MAX_CENTRES} centres (got {C})")
    return C


def _n_img(img_off, limit=MAX_IMAGES):
    require_cuda(img_off)
    if img_off.dtype != torch.int32 or img_off.dim() != 1 or img_off.numel() < 2 or not img_off.is_contiguous():
        raise SfmHipError("retrieval: img_off must be a contiguous int32 [n_img + 1] device tensor with n_img >= 1")
    n_img = int(img_off.numel()) - 1
    if n_img > limit:
        raise SfmHipError(f"retrieval: at most {limit} images (got {n_img})")
    return n_img


def _k(k):
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise SfmHipError(f"retrieval: k must be 1..{MAX_K} (got {k})")
    return k


def assign_accumulate(desc, centres, img_off, scale, out=None):
    """sfm_vlad_accumulate: desc float32 [n_nodes, 128], centres float32 [C, 128], img_off int32 [n_img + 1]: device tensors.
    Returns (assign int32 [n_nodes], acc int64 [n_img, C, 128], count int32 [n_img, C]).  No host wait."""
    n_nodes, C, n_img, scale = _desc(desc), _centres(centres), _n_img(img_off), _positive(scale, "scale")
    dev = desc.device
    if out is None:
        out = (torch.empty(n_nodes, dtype=torch.int32, device=dev), torch.empty((n_img, C, DIM), dtype=torch.int64, device=dev),
               torch.empty((n_img, C), dtype=torch.int32, device=dev))
    assign, acc, count = (_typed(out[0], torch.int32, (n_nodes,), "assign"), _typed(out[1], torch.int64, (n_img, C, DIM), "acc"),
                          _typed(out[2], torch.int32, (n_img, C), "count"))
    with on_device(dev):
        check(_lib.lib().sfm_vlad_accumulate(ptr(desc) if n_nodes else None, n_nodes, ptr(centres), C, ptr(img_off), n_img, scale,
                                             ptr(assign) if n_nodes else None, ptr(acc), ptr(count), stream_ptr()), "sfm_vlad_accumulate")
    return assign, acc, count


def update_centres(centres, acc, count, scale, out=None):
    """sfm_vlad_centres: one Lloyd update from `assign_accumulate(desc, centres, [0, N], scale)`; acc int64 [1, C, 128] or [C, 128],
    count int32 [1, C] or [C].  Returns the new centres (float32 [C, 128]).  No host wait."""
    C, scale = _centres(centres), _positive(scale, "scale")
    require_cuda(acc, count)
    if acc.dtype != torch.int64 or not acc.is_contiguous() or tuple(acc.shape) not in ((C, DIM), (1, C, DIM)):
        raise SfmHipError(f"retrieval: acc must be a contiguous int64 device tensor of shape ({C}, 128) or (1, {C}, 128)")
    if count.dtype != torch.int32 or not count.is_contiguous() or tuple(count.shape) not in ((C,), (1, C)):
        raise SfmHipError(f"retrieval: count must be a contiguous int32 device tensor of shape ({C},) or (1, {C})")
    out = torch.empty_like(centres) if out is None else _typed(out, torch.float32, (C, DIM), "centres_out")
    with on_device(centres.device):
        check(_lib.lib().sfm_vlad_centres(ptr(centres), ptr(acc), ptr(count), C, scale, ptr(out), stream_ptr()), "sfm_vlad_centres")
    return out


def initial_rows(n_nodes, n_centres, seed=0):
    """The rows the vocabulary starts from: the one host-side step of the training, and it reads nothing from the device."""
    n_nodes, n_centres = int(n_nodes), int(n_centres)
    if not 1 <= n_centres <= MAX_CENTRES:
        raise SfmHipError(f"retrieval: 1..{MAX_CENTRES} centres (got {n_centres})")
    if n_centres > n_nodes:
        raise SfmHipError(f"retrieval: {n_centres} centres from {n_nodes} descriptors")
    return sorted(int(r) for r in np.random.default_rng(seed).choice(n_nodes, n_centres, replace=False))


def train_vocabulary(desc, n_centres=64, iters=8, seed=0, scale=None):
    """`iters` Lloyd rounds (accumulate over all nodes as one image, then the update) from the rows `initial_rows` names.  desc float32
    [N, 128] on the device.  Returns centres float32 [C, 128].  No host wait; a second run gives the same bits."""
    n_nodes = _desc(desc)
    scale = scale_of() if scale is None else _positive(scale, "scale")
    rows = initial_rows(n_nodes, n_centres, seed)
    dev = desc.device
    centres = desc.index_select(0, _upload(np.asarray(rows, np.int64), dev)).contiguous()
    off = _upload(np.array([0, n_nodes], np.int32), dev)
    out = (torch.empty(n_nodes, dtype=torch.int32, device=dev), torch.empty((1, n_centres, DIM), dtype=torch.int64, device=dev),
           torch.empty((1, n_centres), dtype=torch.int32, device=dev))
    for _ in range(int(iters)):
        assign_accumulate(desc, centres, off, scale, out=out)
        centres = update_centres(centres, out[1], out[2], scale)
    return centres


def signatures(acc, ssr=False, qs=DEFAULT_QS, out=None):
    """sfm_vlad_signature: acc int64 [n_img, C, 128] -> (sig int8 [n_img, C * 128], norm2 int32 [n_img]).  No host wait."""
    require_cuda(acc)
    if acc.dtype != torch.int64 or acc.dim() != 3 or acc.shape[2] != DIM or not acc.is_contiguous():
        raise SfmHipError("retrieval: acc must be a contiguous int64 [n_img, C, 128] device tensor")
    n_img, C, qs = int(acc.shape[0]), int(acc.shape[1]), _positive(qs, "qs")
    if not 1 <= n_img <= MAX_IMAGES or not 1 <= C <= MAX_CENTRES:
        raise SfmHipError(f"retrieval: acc of {n_img} images and {C} centres")
    dev = acc.device
    if out is None:
        out = (torch.empty((n_img, C * DIM), dtype=torch.int8, device=dev), torch.empty(n_img, dtype=torch.int32, device=dev))
    sig, norm2 = _typed(out[0], torch.int8, (n_img, C * DIM), "sig"), _typed(out[1], torch.int32, (n_img,), "norm2")
    with on_device(dev):
        check(_lib.lib().sfm_vlad_signature(ptr(acc), n_img, C, int(bool(ssr)), qs, ptr(sig), ptr(norm2), stream_ptr()), "sfm_vlad_signature")
    return sig, norm2


def shortlist(sig, norm2, k=8, min_sim=None, out=None, workspace=None):
    """sfm_vlad_shortlist: sig int8 [n_img, C * 128], norm2 int32 [n_img] -> (nbr int32 [n_img, k], nbr_sim float32 [n_img, k]): the k
    most similar images of every image in descending similarity (ties to the smaller index), -1 / -inf where there are fewer; min_sim
    (None: -inf) is the least similarity admitted.  At most 16 384 images.  No host wait."""
    require_cuda(sig, norm2)
    if sig.dtype != torch.int8 or sig.dim() != 2 or sig.shape[1] % DIM or not sig.is_contiguous():
        raise SfmHipError("retrieval: sig must be a contiguous int8 [n_img, C * 128] device tensor")
    n_img, C, k = int(sig.shape[0]), int(sig.shape[1]) // DIM, _k(k)
    if not 1 <= n_img <= MAX_SHORTLIST_IMAGES or not 1 <= C <= MAX_CENTRES:
        raise SfmHipError(f"retrieval: shortlist of {n_img} images (1..{MAX_SHORTLIST_IMAGES}) and {C} centres (1..{MAX_CENTRES})")
    _typed(norm2, torch.int32, (n_img,), "norm2")
    min_sim = -math.inf if min_sim is None else float(min_sim)
    if min_sim != min_sim:
        raise SfmHipError("retrieval: min_sim is NaN")
    dev = sig.device
    need = int(_lib.lib().sfm_vlad_shortlist_ws_bytes(n_img))
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    require_cuda(workspace)
    if out is None:
        out = (torch.empty((n_img, k), dtype=torch.int32, device=dev), torch.empty((n_img, k), dtype=torch.float32, device=dev))
    nbr, nbr_sim = _typed(out[0], torch.int32, (n_img, k), "nbr"), _typed(out[1], torch.float32, (n_img, k), "nbr_sim")
    with on_device(dev):
        check(_lib.lib().sfm_vlad_shortlist(ptr(sig), ptr(norm2), n_img, C, k, min_sim, ptr(nbr), ptr(nbr_sim), ptr(workspace),
                                            workspace.numel() * workspace.element_size(), stream_ptr()), "sfm_vlad_shortlist")
    return nbr, nbr_sim


def pair_list(nbr, mutual=False, cap_pairs=None, out=None, workspace=None):
    """sfm_vlad_pairs: nbr int32 [n_img, k] -> (pairs int32 [cap_pairs, 2], count int32 [2] = (selected, written)): the pairs (a, b),
    a < b, of which one names the other (mutual: both), ascending; cap_pairs defaults to n_img * k, which always fits.  No host wait."""
    require_cuda(nbr)
    if nbr.dtype != torch.int32 or nbr.dim() != 2 or not nbr.is_contiguous():
        raise SfmHipError("retrieval: nbr must be a contiguous int32 [n_img, k] device tensor")
    n_img, k = int(nbr.shape[0]), _k(nbr.shape[1])
    if not 1 <= n_img <= MAX_SHORTLIST_IMAGES:
        raise SfmHipError(f"retrieval: pair list of {n_img} images (1..{MAX_SHORTLIST_IMAGES})")
    cap = n_img * k if cap_pairs is None else int(cap_pairs)
    if not 0 <= cap <= INT32_MAX:
        raise SfmHipError(f"retrieval: cap_pairs must be 0..2^31-1 (got {cap})")
    dev = nbr.device
    need = int(_lib.lib().sfm_vlad_pairs_ws_bytes(n_img))
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    require_cuda(workspace)
    if out is None:
        out = (torch.empty((cap, 2), dtype=torch.int32, device=dev), torch.empty(2, dtype=torch.int32, device=dev))
    pairs, count = _typed(out[0], torch.int32, (cap, 2), "pairs"), _typed(out[1], torch.int32, (2,), "count")
    with on_device(dev):
        check(_lib.lib().sfm_vlad_pairs(ptr(nbr), n_img, k, int(bool(mutual)), ptr(pairs) if cap else None, cap, ptr(count), ptr(workspace),
                                        workspace.numel() * workspace.element_size(), stream_ptr()), "sfm_vlad_pairs")
    return pairs, count


def select_pairs(descriptors_or_desc, img_off=None, k=8, centres=None, n_centres=64, iters=8, seed=0, ssr=False, mutual=False, min_sim=None,
                 value_range=DEFAULT_VALUE_RANGE):
    """The pairs worth matching.  descriptors_or_desc: a list over images of float32 [n_i, 128] device tensors (img_off None), or the
    concatenated float32 [n_nodes, 128] with img_off int32 [n_img + 1] on the device.  centres (float32 [C, 128]): a vocabulary trained
    before; None trains one of n_centres centres on these descriptors (`train_vocabulary(desc, n_centres, iters, seed)`).  Every image
    is paired with its k most similar images (mutual: only where both name each other; min_sim: the least similarity admitted).
    value_range: the width of the descriptor values (256 for SIFT bytes); it fixes the fixed-point scale (`scale_of`).
    Returns (list of (i, j) with i < j, ascending: what `match_pairs_sharded(descriptors, pairs)` takes,
             dict(centres=, sig=, nbr=, nbr_sim=) of device tensors).
    ONE host wait: the download of the count together with the n_img * k pair rows."""
    if img_off is None:
        descs = list(descriptors_or_desc)
        if not descs:
            raise SfmHipError("select_pairs: no image")
        require_cuda(*descs)
        if any(d.dim() != 2 or d.shape[1] != DIM for d in descs):
            raise SfmHipError("select_pairs: descriptors must be [n_i, 128]")
        dev = descs[0].device
        off = np.zeros(len(descs) + 1, np.int64)
        np.cumsum([int(d.shape[0]) for d in descs], out=off[1:])
        if off[-1] > INT32_MAX:
            raise SfmHipError(f"select_pairs: {int(off[-1])} nodes exceed 2^31-1")
        img_off = _upload(off.astype(np.int32), dev)
        desc = torch.cat([d.to(device=dev, dtype=torch.float32) for d in descs]).contiguous()
    else:
        desc = descriptors_or_desc
    n_nodes, n_img, k, scale = _desc(desc), _n_img(img_off, MAX_SHORTLIST_IMAGES), _k(k), scale_of(value_range)
    if centres is None:
        centres = train_vocabulary(desc, n_centres, iters, seed, scale)
    _, acc, _ = assign_accumulate(desc, centres, img_off, scale)
    sig, norm2 = signatures(acc, ssr)
    nbr, nbr_sim = shortlist(sig, norm2, k, min_sim)
    cap = n_img * k
    block = torch.empty((cap + 1, 2), dtype=torch.int32, device=desc.device)          # the count in front of the rows: one download
    pair_list(nbr, mutual, cap, out=(block[1:], block[0]))
    host = block.cpu().numpy()                                                         # the one host wait
    written = int(host[0, 1])
    return [(int(a), int(b)) for a, b in host[1:1 + written]], dict(centres=centres, sig=sig, nbr=nbr, nbr_sim=nbr_sim)
