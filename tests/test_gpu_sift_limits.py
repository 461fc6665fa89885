"""SIFT on the MI355X at the limits its argument checks admit (tests/sift_cases.py; tests/test_sift_cases_cpu.py proves on the
oracle that the table reaches them): every blur launch path and tap count up to the 55-tap limit, 2 to 8 layers, frames from
8 x 8 and 8 x 300, list capacities between "everything overflows" and "plenty", the ordering pass on a frame whose keypoints sit
in three x ranges, multi-pass orientation windows, and the preprocessing calls' remaining entry-point cases.  Every comparison
is bit for bit against oracle.sift (int32 view of the keypoints, array_equal of the descriptors)."""
import ctypes

import numpy as np
import pytest
import torch

import sift_cases as sc

pytestmark = pytest.mark.gpu


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()              # (the table's frames are read only: upload a copy)


def _engine(w, h, nl=3, sigma=1.6, **kw):
    from sfm_mvs_amd import sift
    return sift.Sift(w, h, "cuda", n_octave_layers=nl, sigma=sigma, **kw)


def _run(g, nl=3, sigma=1.6, **kw):
    h, w = g.shape
    kp, des = _engine(w, h, nl, sigma, **kw).run(_dev(g))
    return kp.cpu().numpy(), des.cpu().numpy()


def _check_pair(oracle, size, params):
    g = sc.frame(*size)
    kpo, deso = sc.oracle_sift(oracle, size, g, *params)
    assert len(kpo) >= sc.KEYPOINT_FLOORS[size][params]
    kp, des = _run(g, *params)
    if len(kpo) == 0:
        assert kp.shape == (0, 8) and des.shape == (0, 128)
    assert _same(kp, kpo) and _same(des, deso), (size, params, len(kp), len(kpo))


@pytest.mark.parametrize("size", sc.SPREAD_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("params", sc.PARAM_SETS, ids=lambda p: f"nL{p[0]}-sigma{p[1]}")
def test_every_parameter_set_bit_exact(hip, oracle, size, params):
    """Blur launch paths by tap count: gauss_blur_kernel at 3 taps (R = 1: the base blur of sigma 1.0, and of 1.045 where the outer
    taps are large enough to move a pixel) and at 31, 33, 35, 39, 43,
    47 and 55 taps (the 62.8 KB LDS tile of the limit), every gauss_blur_fixed_kernel<N>, N = 5..27 (5 and 25 had never run),
    the pair launches at (3, 1.6); 2, 3 and 8 layers (11 blurs and `Taps taps[16]`); orientation windows of two to five
    1024-sample passes at sigma 2.4 and 3.4.  On a frame of 7 x 10 blur tiles (interior and border tiles) and on one just over a tile.  One tap off in
    any kernel, or a pass boundary that drops or repeats a sample, changes keypoints or descriptors."""
    _check_pair(oracle, size, params)


@pytest.mark.parametrize("size", sc.TINY_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("params", sc.WIDE_SETS, ids=lambda p: f"nL{p[0]}-sigma{p[1]}")
def test_wide_taps_on_planes_narrower_than_the_radius(hip, oracle, size, params):
    """Blur radius (27 at 55 taps) against octave planes of 16, 8 and 4 pixels: reflect101 wraps several periods in the tile
    load of both blur kernels, every tile is a border tile, a plane is one tile wide and nineteen high (8 x 300), and the
    octave count comes from the short side.  Where the oracle finds nothing the result is (0, 8) / (0, 128) and no error."""
    _check_pair(oracle, size, params)


@pytest.mark.parametrize("size", sc.FRAME_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("params", [sc.DEFAULT, (8, 1.0)], ids=lambda p: f"nL{p[0]}-sigma{p[1]}")
def test_every_frame_size_bit_exact(hip, oracle, size, params):
    """Frame sizes at, one below and one above the 64 x 32 blur tile and the 64 x 4 lane maps of the doubled base (32 x 16, 33 x
    17, 31 x 33, 64 x 32, 65 x 33), the smallest admitted frames (8 x 8, 9 x 8), the most elongated (8 x 300, 300 x 8, 11 x 257),
    odd sizes whose octaves halve with truncation: the pair launches (defaults) and the 3- to 9-tap chain of eleven blurs
    (8, 1.0), the extrema / gradient tile maps, the stride-2 read of the next octave."""
    _check_pair(oracle, size, params)


def test_tap_limit_is_55_and_an_error_leaves_nothing_behind(hip, oracle):
    """kMaxTaps: (3, 3.4) needs exactly 55 taps and runs; (3, 3.6) needs 57 and (1, 1.6) needs 91: both are refused with the
    library's error before anything is launched, and an engine of the same size built afterwards is exact."""
    from sfm_mvs_amd import SfmHipError
    size = (65, 33)
    g = sc.frame(*size)
    d = _dev(g)
    assert max(sc.tap_counts(oracle, 3, 3.4)) == 55
    _check_pair(oracle, size, (3, 3.4))
    for nl, sg in [(3, 3.6), (1, 1.6)]:
        assert max(sc.tap_counts(oracle, nl, sg)) > 55
        with pytest.raises(SfmHipError, match="filter taps"):
            _engine(size[0], size[1], nl, sg).run(d)
        _check_pair(oracle, size, (3, 3.4))
        _check_pair(oracle, size, sc.DEFAULT)


@pytest.mark.parametrize("k", [0, 1], ids=["160x120", "256x192"])
def test_capacity_exact_or_loud(hip, oracle, k):
    """List capacities: the raw-extrema, candidate and keypoint lists are 64 segments of cap / 64 slots (workgroup -> segment
    round robin), so one segment can overflow far below max_keypoints; a max_keypoints that is no multiple of 64 (100, 321, 1000)
    leaves slots no segment owns.  Whatever happens inside, Sift.run either raises or returns exactly the oracle's result — a
    segment that drops its last slot, or an overflow that is not reported, returns a short or different list here.  After a
    raise the same engine runs a flat frame (no keypoints, no error: the counters are cleared per launch) and a fresh engine of
    the default capacity is exact.  Beside the listed capacities every segment size 1..40 is run: one of them is the size at which
    the fullest keypoint segment is exactly full while nothing overflows, where a run must return and be complete.  Both outcomes must occur between the ends of the sweep: 64 raises, some value below 4 n
    raises, some value below 1 << 17 succeeds, 1 << 17 succeeds."""
    from sfm_mvs_amd import SfmHipError
    g = sc.capacity_frame(k)
    h, w = g.shape
    kpo, deso = sc.oracle_sift(oracle, ("capacity", k), g, *sc.DEFAULT)
    n = len(kpo)
    assert n == [556, 1201][k]
    d = _dev(g)
    flat = _dev(np.full((h, w), 93, np.uint8))
    raised = {}
    for cap in sc.CAPACITIES_FINE:
        eng = _engine(w, h, max_keypoints=cap)
        try:
            kp, des = eng.run(d)
            raised[cap] = False
        except SfmHipError:
            raised[cap] = True
        print(f"{w}x{h} ({n} keypoints) max_keypoints {cap}: {'raises' if raised[cap] else 'returns'}; counters {eng.count.tolist()}")
        if raised[cap]:
            kp0, des0 = eng.run(flat)
            assert kp0.shape == (0, 8) and des0.shape == (0, 128) and eng.count.tolist() == [0, 0, 0, 0], cap
            kp, des = _engine(w, h).run(d)
        assert _same(kp.cpu().numpy(), kpo) and _same(des.cpu().numpy(), deso), cap
    print(f"{w}x{h}: smallest succeeding max_keypoints {min(c for c, r in raised.items() if not r)}")
    assert raised[64] and not raised[1 << 17]
    assert any(r for c, r in raised.items() if c < 4 * n)
    assert any(not r for c, r in raised.items() if c < 1 << 17)


def test_column_frame_through_engine_and_pipeline(hip, oracle):
    """Ordering pass: bucket_scatter_kernel / bucket_rank_kernel assume about n / 256 keypoints per x range; here 228 keypoints
    fall into three ranges (152 in one, spread over the rows of a workgroup's LDS staging) and 152 share (x, y) with another, so
    the rank is decided by the size / angle / response / octave cascade and dedupe_kernel sees runs of equal (x, y).  Through Sift and
    through a SiftPipeline(depth=2) that takes the frame twice (two engines, two streams)."""
    from sfm_mvs_amd import sift
    g = sc.column_frame()
    h, w = g.shape
    kpo, deso = sc.oracle_sift(oracle, "column", g, *sc.DEFAULT)
    assert len(kpo) >= 200
    kp, des = _run(g)
    assert _same(kp, kpo) and _same(des, deso)
    pipe = sift.SiftPipeline(w, h, "cuda", depth=2)
    d = _dev(g)
    subs = [pipe.submit(d) for _ in range(2)]
    assert subs[0][2] is not subs[1][2]
    for _, st, eng in subs:
        st.synchronize()
        n = eng.check_capacity()
        assert _same(eng.keypoints[:n].cpu().numpy(), kpo) and _same(eng.descriptors[:n].cpu().numpy(), deso)


@pytest.mark.parametrize("size,params", [((200, 150), sc.DEFAULT), ((65, 33), (8, 1.0))], ids=["200x150", "65x33"])
def test_keypoints_without_descriptors(hip, oracle, size, params):
    """want_descriptors=False (a null descriptor pointer: the descriptor launches are skipped): the same keypoints bit for bit,
    `descriptors` is None, and the engine's descriptor buffer is not written."""
    g = sc.frame(*size)
    kpo, _ = sc.oracle_sift(oracle, size, g, *params)
    assert len(kpo) > 50
    eng = _engine(size[0], size[1], *params)
    eng.descriptors.fill_(-7.0)
    kp, des = eng.run(_dev(g), want_descriptors=False)
    assert des is None and _same(kp.cpu().numpy(), kpo)
    assert bool((eng.descriptors == -7.0).all())
    kp2, des2 = eng.run(_dev(g))
    assert _same(kp2.cpu().numpy(), kpo) and des2.shape == (len(kpo), 128)


@pytest.mark.parametrize("case", ["11_wide", "65x33", "unaligned_base"])
def test_strided_and_unaligned_input(hip, oracle, case):
    """upsample2_kernel reads the frame through (pointer, row stride): crops with odd offsets whose stride exceeds their width
    (an 11-wide and a 65 x 33 crop) and a crop whose first byte is not 4-byte aligned (big[3:, 1:] of a 70-wide frame), no copy."""
    if case == "11_wide":
        big, crop = sc.blocks(37, 263, 5), (slice(5, 262), slice(13, 24))
        params = (8, 1.0)
    elif case == "65x33":
        big, crop = sc.blocks(101, 47, 6), (slice(7, 40), slice(29, 94))
        params = sc.DEFAULT
    else:
        big, crop = sc.blocks(70, 45, 7), (slice(3, None), slice(1, None))
        params = (8, 1.0)
    want = np.ascontiguousarray(big[crop])
    kpo, deso = oracle.sift(want, n_octave_layers=params[0], sigma=params[1])
    assert len(kpo) > 30
    view = _dev(big)[crop]
    assert view.stride(0) > view.shape[1] and not view.is_contiguous()
    if case == "unaligned_base":
        assert view.data_ptr() % 4 != 0
    h, w = want.shape
    kp, des = _engine(w, h, *params).run(view)
    assert _same(kp.cpu().numpy(), kpo) and _same(des.cpu().numpy(), deso)


PRE_SHAPES = [(1, 1), (1, 9), (9, 1), (2, 2), (3, 2), (5, 257)]          # (h, w)


@pytest.mark.parametrize("ch", [2, 4])
def test_pyrdown_two_and_four_channels(hip, oracle, ch):
    """pyrdown_kernel's channel loop with 2 and 4 interleaved channels (1 and 3 are what the pipeline uses), on an odd frame of
    more than one workgroup and on the tiny shapes."""
    from sfm_mvs_amd import sift
    rng = np.random.default_rng(10 + ch)
    for h, w in [(37, 131)] + PRE_SHAPES:
        img = rng.integers(0, 256, (h, w, ch), dtype=np.uint8)
        got = sift.pyrdown(_dev(img)).cpu().numpy()
        assert got.shape == ((h + 1) // 2, (w + 1) // 2, ch) and np.array_equal(got, oracle.pyrdown(img))


@pytest.mark.parametrize("h,w", PRE_SHAPES)
def test_preprocessing_on_one_pixel_wide_and_high_frames(hip, oracle, h, w):
    """Frames one or two pixels wide or high: reflect101 with len 1 and 2 in pyrdown_kernel, partial lane maps in both kernels,
    257 columns = four workgroups and one lane."""
    from sfm_mvs_amd import sift
    rng = np.random.default_rng(100 * h + w)
    bgr = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    d = _dev(bgr)
    assert np.array_equal(sift.bgr2gray(d).cpu().numpy(), oracle.bgr2gray(bgr))
    assert np.array_equal(sift.pyrdown(d).cpu().numpy(), oracle.pyrdown(bgr))
    gray = np.ascontiguousarray(bgr[..., 2])
    assert np.array_equal(sift.pyrdown(_dev(gray)).cpu().numpy(), oracle.pyrdown(gray))


def test_bgr2gray_row_stride_through_the_c_abi(hip, oracle):
    """sfm_bgr2gray_u8 with a row stride of 3 w + 5 bytes (the Python wrapper always passes 3 w): rows start at odd addresses,
    and the five bytes of padding per row are not read into the result (two different paddings, one answer)."""
    from sfm_mvs_amd import _lib
    rng = np.random.default_rng(77)
    for h, w in [(37, 131), (5, 257), (9, 1)]:
        bgr = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        want = oracle.bgr2gray(bgr)
        stride = 3 * w + 5
        for pad in (0, 255):
            buf = np.full((h, stride), pad, np.uint8)
            buf[:, :3 * w] = bgr.reshape(h, 3 * w)
            src = _dev(buf)
            out = torch.full((h, w), 7, dtype=torch.uint8, device="cuda")
            _lib.check(_lib.lib().sfm_bgr2gray_u8(_lib.ptr(src), w, h, stride, _lib.ptr(out), _lib.stream_ptr()), "sfm_bgr2gray_u8")
            assert np.array_equal(out.cpu().numpy(), want), (h, w, pad)
    src = _dev(np.zeros((4, 3 * 8), np.uint8))
    out = torch.empty((4, 8), dtype=torch.uint8, device="cuda")
    assert _lib.lib().sfm_bgr2gray_u8(_lib.ptr(src), 8, 4, ctypes.c_int64(3 * 8 - 1), _lib.ptr(out), _lib.stream_ptr()) != 0   # stride < 3 w: refused
