"""NumPy restatement of the RETRIEVAL family, written from include/sfm_hip.h ("RETRIEVAL"), not from the kernels: every output word.
Float32 steps are NumPy float32 operations (one rounding each, no FMA), float64 steps float64; integer words are Python / int64."""
import numpy as np

DIM = 128
CLAMP = np.float32(2.0 ** 30)
NEG_INF_BITS = np.float32(-np.inf).view(np.int32)


def image_of(img_off, u):
    """The largest i < n_img with img_off[i] <= u (0 when there is none)."""
    n_img = len(img_off) - 1
    i = int(np.searchsorted(np.asarray(img_off[:n_img], np.int64), u, side="right")) - 1
    return max(i, 0)


def l2sqr(a, b):
    """The direct form: a [n, 128], b [128] float32 -> float32 [n], eight accumulators in the header's order."""
    a = np.asarray(a, np.float32).reshape(-1, DIM)
    b = np.asarray(b, np.float32).reshape(DIM)
    acc = np.zeros((a.shape[0], 8), np.float32)
    with np.errstate(all="ignore"):
        for k in range(16):
            t = a[:, 8 * k:8 * k + 8] - b[8 * k:8 * k + 8]
            acc = acc + t * t
        s = acc[:, :4] + acc[:, 4:]
        return ((s[:, 0] + s[:, 1]) + s[:, 2]) + s[:, 3]


def assign(desc, centres):
    """int32 [n_nodes]: the candidate with the smallest key (bits(d2) << 32) | c, -1 without a candidate."""
    desc = np.asarray(desc, np.float32).reshape(-1, DIM)
    centres = np.asarray(centres, np.float32).reshape(-1, DIM)
    best = np.full(len(desc), np.iinfo(np.uint64).max, np.uint64)
    for c in range(len(centres)):
        d2 = l2sqr(desc, centres[c])
        with np.errstate(invalid="ignore"):
            cand = d2 < np.inf                                   # neither NaN nor +inf
        key = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(c)
        best = np.where(cand & (key < best), key, best)
    out = (best & np.uint64(0xFFFFFFFF)).astype(np.int64)
    out[best == np.iinfo(np.uint64).max] = -1
    return out.astype(np.int32)


def terms(desc, centre_rows, scale):
    """int64 [n, 128]: t = (int64) rintf(fminf(fmaxf(r * scale, -2^30), 2^30)), r = desc - centre in float32."""
    with np.errstate(all="ignore"):
        r = np.asarray(desc, np.float32) - np.asarray(centre_rows, np.float32)
        v = r * np.float32(scale)
        v = np.fmin(np.fmax(v, -CLAMP), CLAMP)
        return np.rint(v).astype(np.int64)


def accumulate(desc, centres, img_off, scale):
    """-> (assign int32 [n_nodes], acc int64 [n_img, C, 128], count int32 [n_img, C])."""
    desc = np.asarray(desc, np.float32).reshape(-1, DIM)
    centres = np.asarray(centres, np.float32).reshape(-1, DIM)
    img_off = np.asarray(img_off, np.int64)
    n_img, C, n = len(img_off) - 1, len(centres), len(desc)
    a = assign(desc, centres)
    acc = np.zeros((n_img, C, DIM), np.int64)
    count = np.zeros((n_img, C), np.int32)
    if n:
        img = np.maximum(np.searchsorted(img_off[:n_img], np.arange(n), side="right") - 1, 0)
        ok = a >= 0
        t = terms(desc[ok], centres[a[ok]], scale)
        np.add.at(acc, (img[ok], a[ok]), t)
        np.add.at(count, (img[ok], a[ok]), 1)
    return a, acc, count


def update_centres(centres, acc, count, scale):
    """One Lloyd update from a single-image accumulate: acc [C, 128] (or [1, C, 128]), count [C]."""
    centres = np.asarray(centres, np.float32).reshape(-1, DIM)
    acc = np.asarray(acc, np.int64).reshape(-1, DIM)
    count = np.asarray(count, np.int32).reshape(-1)
    out = centres.copy()
    nz = count != 0
    den = count[nz].astype(np.float64) * np.float64(np.float32(scale))
    out[nz] = (centres[nz].astype(np.float64) + acc[nz].astype(np.float64) / den[:, None]).astype(np.float32)
    return out


def initial_rows(n, C, seed):
    return sorted(int(r) for r in np.random.default_rng(seed).choice(n, C, replace=False))


def train_vocabulary(desc, C, iters=8, seed=0, scale=4096.0):
    desc = np.asarray(desc, np.float32).reshape(-1, DIM)
    centres = desc[initial_rows(len(desc), C, seed)].copy()
    off = np.array([0, len(desc)], np.int64)
    for _ in range(iters):
        _, acc, count = accumulate(desc, centres, off, scale)
        centres = update_centres(centres, acc[0], count[0], scale)
    return centres


def signatures(acc, ssr=False, qs=127.0):
    """acc int64 [n_img, C, 128] -> (sig int8 [n_img, C * 128], norm2 int32 [n_img])."""
    acc = np.asarray(acc, np.int64)
    n_img, C = acc.shape[0], acc.shape[1]
    a = acc.astype(np.float64)
    if ssr:
        a = np.copysign(np.sqrt(np.abs(a)), a)
    sq = a * a
    n2 = np.zeros((n_img, C), np.float64)
    for k in range(DIM):                                         # left to right
        n2 = n2 + sq[:, :, k]
    ok = (n2 != 0) & np.isfinite(n2)
    with np.errstate(all="ignore"):
        v = np.rint(a / np.sqrt(n2)[:, :, None] * np.float64(qs))
        v = np.fmin(np.fmax(v, -127.0), 127.0)
    q = np.where(ok[:, :, None], v, 0.0).astype(np.int8)
    norm2 = (q.astype(np.int64) ** 2).sum((1, 2))
    assert (norm2 < 2 ** 31).all()
    return q.reshape(n_img, C * DIM), norm2.astype(np.int32)


def similarities(sig, norm2):
    """(S int64 [n, n] exact, sim float32 [n, n]; sim is only meaningful where both norms are non-zero)."""
    s = np.asarray(sig, np.int8).astype(np.int64)
    S = s @ s.T
    n = np.asarray(norm2, np.int32).astype(np.float64)
    with np.errstate(all="ignore"):
        sim = (S.astype(np.float64) / np.sqrt(n[:, None] * n[None, :])).astype(np.float32)
    return S, sim


def shortlist(sig, norm2, k, min_sim=-np.inf):
    """-> (nbr int32 [n, k], nbr_sim float32 [n, k]): descending sim, ties to the smaller j, -1 / -inf where missing."""
    norm2 = np.asarray(norm2, np.int32)
    n = len(norm2)
    _, sim = similarities(sig, norm2)
    nbr = np.full((n, k), -1, np.int32)
    nbr_sim = np.full((n, k), -np.inf, np.float32)
    for i in range(n):
        if norm2[i] == 0:
            continue
        cand = [j for j in range(n) if j != i and norm2[j] != 0 and sim[i, j] >= np.float32(min_sim)]
        cand.sort(key=lambda j: (-float(sim[i, j]), j))
        for s, j in enumerate(cand[:k]):
            nbr[i, s], nbr_sim[i, s] = j, sim[i, j]
    return nbr, nbr_sim


def pair_list(nbr, mutual=False, cap_pairs=None):
    """-> (pairs int32 [selected, 2] in ascending (a, b) order, count [2] = (selected, written))."""
    nbr = np.asarray(nbr, np.int32)
    n = nbr.shape[0]
    named = [set(int(j) for j in row if 0 <= j < n and j != i) for i, row in enumerate(nbr)]
    sel = []
    for a in range(n):
        for b in range(a + 1, n):
            fwd, back = b in named[a], a in named[b]
            if (fwd and back) if mutual else (fwd or back):
                sel.append((a, b))
    pairs = np.array(sel, np.int32).reshape(-1, 2)
    written = len(pairs) if cap_pairs is None else min(len(pairs), int(cap_pairs))
    return pairs, np.array([len(pairs), written], np.int32)


def scale_of(value_range):
    """The power of two with value_range * scale = 2^20 (value_range rounded up to a power of two)."""
    return float(2.0 ** (20 - int(np.ceil(np.log2(float(value_range))))))


def select_pairs(descs, k=8, centres=None, n_centres=64, iters=8, seed=0, ssr=False, mutual=False, min_sim=None, value_range=256.0, qs=127.0):
    """The composition `retrieval.select_pairs` runs.  descs: list of [n_i, 128].  -> (list of (i, j), dict of every stage)."""
    sizes = [len(d) for d in descs]
    img_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    desc = np.concatenate([np.asarray(d, np.float32).reshape(-1, DIM) for d in descs]) if descs else np.zeros((0, DIM), np.float32)
    scale = scale_of(value_range)
    if centres is None:
        centres = train_vocabulary(desc, n_centres, iters, seed, scale)
    a, acc, count = accumulate(desc, centres, img_off, scale)
    sig, norm2 = signatures(acc, ssr, qs)
    nbr, nbr_sim = shortlist(sig, norm2, k, -np.inf if min_sim is None else min_sim)
    pairs, cnt = pair_list(nbr, mutual, len(sizes) * k)
    return [(int(x), int(y)) for x, y in pairs[:cnt[1]]], dict(centres=centres, assign=a, acc=acc, count=count, sig=sig, norm2=norm2, nbr=nbr,
                                                                 nbr_sim=nbr_sim, pairs=pairs, pair_count=cnt)
