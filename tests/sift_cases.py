"""Case table of the SIFT limit tests, shared by tests/test_sift_cases_cpu.py (which proves on the oracle alone that the table
reaches what it claims) and tests/test_gpu_sift_limits.py (which runs it on the HIP path).  Plain data and builders: nothing of
sfm_mvs_amd is imported here; functions that need the oracle take it as an argument."""
import functools

import numpy as np

from datagen import scene_image

# (n_octave_layers, sigma).  Their blur lengths n = lrint(8 s + 1) | 1 (base blur and every layer) together are every odd n of
# 3..27 (gauss_blur_kernel at R = 1, every gauss_blur_fixed_kernel<N>) and 31, 33, 35, 39, 43, 47, 55 (gauss_blur_kernel up to its
# documented limit); (3, 1.6) alone takes the two gauss_blur_pair_kernel launches.  test_sift_cases_cpu.py asserts the coverage.
# (3, 1.045) is there for the 3-tap kernel's OUTER taps: at sigma 1.0 the base blur is the floor sigma 0.1, whose taps (1.9e-22,
# 1, 1.9e-22) leave every pixel unchanged, so a kernel that fetched the wrong neighbour at R = 1 would still be exact; at 1.045 the
# base blur is sigma 0.303, still 3 taps, with outer taps of 0.0043 (a grey level).
PARAM_SETS = [(3, 1.0), (8, 1.0), (3, 1.4), (3, 1.6), (3, 2.4), (3, 3.4), (8, 1.6), (2, 2.0), (3, 1.045)]
EFFECTIVE_3_TAP_SET = (3, 1.045)
DEFAULT = (3, 1.6)
WIDE_SETS = [(3, 3.4), (8, 1.0), (2, 2.0)]            # the widest taps, the most layers, the fewest layers
MAX_TAPS = 55                                          # kMaxTaps of csrc/sift.hip
FIXED_TAPS = tuple(range(5, 28, 2))                    # tap counts with a gauss_blur_fixed_kernel<N>

# (w, h): at, one below and one above the 64 x 32 blur tile and the 64 x 4 lane maps of the DOUBLED base (32 x 16 doubles to one
# tile), the smallest admitted frame, planes narrower than a blur radius (8 x 300, 300 x 8), odd sizes whose octaves halve with
# truncation
FRAME_SIZES = [(8, 8), (9, 8), (8, 300), (300, 8), (11, 257), (24, 17), (31, 33), (32, 16), (33, 17), (64, 32), (65, 33), (200, 150)]
TINY_SIZES = [(8, 8), (9, 8), (24, 17), (40, 30), (8, 300)]
SPREAD_SIZES = [(200, 150), (65, 33)]

CAPACITY_FRAMES = [(160, 120, 0), (256, 192, 1)]       # scene_image(w, h, seed): 556 and 1 201 oracle keypoints
CAPACITIES = [64, 100, 321, 512, 640, 1000, 1024, 2048, 4096, 1 << 17]
# every segment size 1..40 as well: somewhere in between lies the capacity at which the fullest keypoint segment is EXACTLY full
# and nothing overflows (the run must return, complete); a coarse sweep steps over it
CAPACITIES_FINE = sorted(set(CAPACITIES) | {64 * s for s in range(1, 41)})

X_BUCKETS = 256                                        # kXBuckets
ORI_CHUNK = 1024                                       # kOriChunk: window samples per pass of orientation_kernel


def blocks(w, h, seed, side=4):
    """side x side blocks of random grey levels: corners and exact ties at any frame size (scene_image needs room for its
    shapes, white noise is blurred away on frames this small)."""
    rng = np.random.default_rng(seed)
    lv = rng.integers(0, 256, ((h + side - 1) // side, (w + side - 1) // side), dtype=np.uint8)
    return np.ascontiguousarray(np.kron(lv, np.ones((side, side), np.uint8))[:h, :w])


@functools.lru_cache(maxsize=None)
def frame(w, h):
    """The table's frame of that size (read only: the tests share it)."""
    g = scene_image(200, 150, 4) if (w, h) == (200, 150) else blocks(w, h, 1000 * w + h)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def column_frame():
    """512 x 400, grey 40, Gaussian blobs (sigma 2.5 px, amplitude 180) every 10 rows on column 256: every keypoint falls into
    two or three of the ordering pass's 256 x ranges, and blobs answer in several layers at the same (x, y)."""
    w, h = 512, 400
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.full((h, w), 40.0)
    for cy in range(10, h - 5, 10):
        img += 180.0 * np.exp(-((xx - 256) ** 2 + (yy - cy) ** 2) / (2 * 2.5 ** 2))
    g = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def capacity_frame(k):
    w, h, seed = CAPACITY_FRAMES[k]
    g = scene_image(w, h, seed)
    g.setflags(write=False)
    return g


def blur_sigmas(n_layers, sigma):
    """OpenCV's schedule: the base blur lifts the doubled frame's assumed blur of 1.0 to sigma (float32, floored at 0.1); layer i
    adds sqrt((sigma k^i)^2 - (sigma k^(i-1))^2), k = 2^(1/nL), for i = 1..nL+2."""
    sf = np.float32(sigma)
    sd = sf * sf - np.float32(1.0)
    out = [float(np.sqrt(max(sd, np.float32(0.01)), dtype=np.float32))]
    k = 2.0 ** (1.0 / n_layers)
    for i in range(1, n_layers + 3):
        sp = k ** (i - 1) * sigma
        out.append(float(np.sqrt((sp * k) ** 2 - sp * sp)))
    return out


def tap_counts(oracle, n_layers, sigma):
    """Kernel lengths of the base blur and of every layer, from the oracle's own kernel builder.  (Its buffer holds 128 taps;
    a blur beyond sigma 15 is far over the limit whatever its exact length.)"""
    return [999 if s > 15.0 else len(oracle.sift_gauss_kernel(s)) for s in blur_sigmas(n_layers, sigma)]


def gpu_pairs():
    """Every ((w, h), (nL, sigma)) the GPU tests run on the table's frames, in a fixed order, without repeats."""
    pairs = [(s, p) for s in SPREAD_SIZES for p in PARAM_SETS]
    pairs += [(s, p) for s in TINY_SIZES for p in WIDE_SETS]
    pairs += [(s, p) for s in FRAME_SIZES for p in (DEFAULT, (8, 1.0))]
    return list(dict.fromkeys(pairs))


# Floors of the ORACLE's keypoint count per (frame, parameter set): two thirds of what the oracle gives on the table's frames
# (its exact count below three), so that a GPU case cannot pass by comparing two empty lists.  0 marks the pairs where the
# oracle itself finds nothing (the plane is smaller than the detector's 5 px border at every octave the blur leaves contrast
# in): they pin "no keypoints, no error" and may be at most a quarter of the pairs.
KEYPOINT_FLOORS = {
    (200, 150): {(3, 1.0): 492, (8, 1.0): 766, (3, 1.4): 540, (3, 1.6): 548, (3, 2.4): 158, (3, 3.4): 31, (8, 1.6): 570, (2, 2.0): 244, (3, 1.045): 500},
    (65, 33): {(3, 1.0): 32, (8, 1.0): 248, (3, 1.4): 38, (3, 1.6): 34, (3, 2.4): 11, (3, 3.4): 6, (8, 1.6): 54, (2, 2.0): 30, (3, 1.045): 36},
    (8, 8): {(3, 3.4): 0, (8, 1.0): 1, (2, 2.0): 0, (3, 1.6): 0},
    (9, 8): {(3, 3.4): 0, (8, 1.0): 2, (2, 2.0): 0, (3, 1.6): 0},
    (24, 17): {(3, 3.4): 1, (8, 1.0): 27, (2, 2.0): 7, (3, 1.6): 2},
    (40, 30): {(3, 3.4): 0, (8, 1.0): 125, (2, 2.0): 13},
    (8, 300): {(3, 3.4): 0, (8, 1.0): 114, (2, 2.0): 0, (3, 1.6): 0},
    (300, 8): {(3, 1.6): 1, (8, 1.0): 119},
    (11, 257): {(3, 1.6): 13, (8, 1.0): 144},
    (31, 33): {(3, 1.6): 12, (8, 1.0): 81},
    (32, 16): {(3, 1.6): 4, (8, 1.0): 50},
    (33, 17): {(3, 1.6): 6, (8, 1.0): 44},
    (64, 32): {(3, 1.6): 22, (8, 1.0): 212},
}

_ORACLE = {}


def oracle_sift(oracle, g_key, g, n_layers, sigma):
    """oracle.sift once per (frame, parameter set), shared by the tests of a session; the arrays are read only."""
    key = (g_key, n_layers, sigma)
    if key not in _ORACLE:
        kp, des = oracle.sift(g, n_octave_layers=n_layers, sigma=sigma)
        kp.setflags(write=False)
        des.setflags(write=False)
        _ORACLE[key] = (kp, des)
    return _ORACLE[key]


def x_bucket(x, W0):
    """x_bucket of csrc/sift.hip: the ordering pass's range of a keypoint, from its x on the doubled base (float32 arithmetic)."""
    x = np.asarray(x, np.float32)
    s = np.float32(X_BUCKETS) / np.float32(W0)
    return np.clip((x * s).astype(np.int32), 0, X_BUCKETS - 1)


def orientation_radius(kp):
    """Radius of a keypoint's orientation window: round(4.5 * scl_octv), scl_octv = size / 2 / 2^octave (OpenCV's
    calcOrientationHist call), from the OUTPUT keypoints (size and the octave byte both refer to the undoubled frame)."""
    octave = (kp[:, 5].view(np.int32) & 255).astype(np.int32)
    octave = np.where(octave < 128, octave, octave - 256)
    scl = kp[:, 2].astype(np.float32) * np.float32(0.5) / np.exp2(octave).astype(np.float32)
    return np.rint(np.float32(4.5) * scl).astype(np.int32)
