"""Randomised SIFT parity sweep on the GPU box: HIP path vs the CPU oracle, bit for bit, over random frame sizes, contents,
detector parameters and list capacities — the whole box the library's argument checks admit (sides from 8, elongated frames,
1..8 layers, sigma 1.0..3.4).  A draw whose blurs need more than 55 taps must be REJECTED with the library's error (expected
from oracle.sift_gauss_kernel, not from the library); a draw whose lists overflow max_keypoints must raise (exact or loud);
both are counted apart from mismatches.  Usage: python scripts/fuzz_sift.py [seconds] [seed]"""
import os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from sfm_mvs_amd import SfmHipError, sift
from oracle import oracle as orc
import datagen

MAX_TAPS = 55


def max_taps(nl, sg):
    """Longest blur kernel of the schedule (base blur + nL + 2 layers), from the oracle's kernel builder (which holds 128 taps:
    a blur beyond sigma 15 is over the limit whatever its exact length)."""
    sf = np.float32(sg)
    sigmas = [float(np.sqrt(max(sf * sf - np.float32(1.0), np.float32(0.01)), dtype=np.float32))]
    k = 2.0 ** (1.0 / nl)
    for i in range(1, nl + 3):
        sp = k ** (i - 1) * sg
        sigmas.append(float(np.sqrt((sp * k) ** 2 - sp * sp)))
    return max(999 if s > 15.0 else len(orc.sift_gauss_kernel(s)) for s in sigmas)


def blocks(rng, w, h, side):
    return np.kron(rng.integers(0, 256, ((h + side - 1) // side, (w + side - 1) // side), dtype=np.uint8), np.ones((side, side), np.uint8))[:h, :w].copy()


budget = float(sys.argv[1]) if len(sys.argv) > 1 else 120.0
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
rng = np.random.default_rng(seed)
t0 = time.time(); cases = bad = kps = rejected = overflows = 0
while time.time() - t0 < budget:
    if rng.integers(0, 5) == 0:                                                                        # elongated: one side 8..16
        a, b = int(rng.integers(8, 17)), int(rng.integers(8, 401))
        w, h = (a, b) if rng.integers(0, 2) else (b, a)
    else:
        w, h = int(rng.integers(8, 520)), int(rng.integers(8, 420))
    kind = int(rng.integers(0, 6))
    s = int(rng.integers(0, 1 << 30))
    if min(w, h) < 24 and kind in (0, 3, 4): kind = 5                                                  # scene_image needs room for its shapes
    if kind == 0:   g = datagen.scene_image(w, h, s)
    elif kind == 1: g = rng.integers(0, 256, (h, w), dtype=np.uint8)                                   # white noise
    elif kind == 2: g = blocks(rng, w, h, 8)                                                           # blocks: exact ties
    elif kind == 3: g = np.rot90(datagen.scene_image(h, w, s)).copy()
    elif kind == 4: g = (datagen.scene_image(w, h, s) // 16 * 16).astype(np.uint8)                    # posterised: plateaus
    else:           g = blocks(rng, w, h, 4)                                                           # small blocks: keypoints on tiny frames
    nl = int(rng.integers(1, 9))
    ct = float(rng.choice([0.04, 0.04, 0.02, 0.08]))
    et = float(rng.choice([10.0, 10.0, 5.0, 20.0]))
    sg = float(rng.uniform(1.0, 3.4))
    cap = int(rng.choice([1 << 16, 4096, 1024]))
    reject = max_taps(nl, sg) > MAX_TAPS
    what = f"{w}x{h} kind {kind} seed {s} nL {nl} ct {ct} et {et} sigma {sg!r} cap {cap}"
    cases += 1
    try:
        eng = sift.Sift(w, h, "cuda", n_octave_layers=nl, contrast_threshold=ct, edge_threshold=et, sigma=sg, max_keypoints=cap)
        try:
            kp, des = eng.run(torch.as_tensor(g).cuda())
        except SfmHipError as e:
            if reject and "filter taps" in str(e): rejected += 1
            elif not reject and "more than max_keypoints" in str(e): overflows += 1                    # loud: allowed at any capacity
            else: bad += 1; print(f"MISMATCH case {cases}: {what}: unexpected error {str(e)[:160]}")
            continue
        if reject:
            bad += 1; print(f"MISMATCH case {cases}: {what}: needs {max_taps(nl, sg)} taps and was not rejected")
            continue
        kpo, deso = orc.sift(g, n_octave_layers=nl, contrast=ct, edge=et, sigma=sg)
        kp, des = kp.cpu().numpy(), des.cpu().numpy()
        kps += len(kpo)
        if not (kp.shape == kpo.shape and np.array_equal(kp.view(np.int32), kpo.view(np.int32)) and np.array_equal(des, deso)):
            bad += 1; print(f"MISMATCH case {cases}: {what}: oracle {len(kpo)} hip {len(kp)}")
    except Exception as e:                                                                             # noqa: BLE001
        bad += 1; print(f"MISMATCH case {cases}: {what}: EXC {repr(e)[:200]}")
from sfm_mvs_amd import _lib as _sfm_lib
print(f"fuzz_sift: {cases} cases, {kps} keypoints compared, {bad} mismatches, {rejected} rejected, {overflows} overflows, {time.time() - t0:.0f} s; build {_sfm_lib.build_id()}")
