"""Calibration of the retrieval bars on the CPU (docs/retrieval.md §5): the RESTATEMENT tests/np_retrieval.py over the grid of
tests/retrieval_cases.py (n_centres {16, 64} x ssr {0, 1} x k {4, 8, 16} on the corridor, the default setting on three seeds, the
cluster scene, the track scene) -> tests/golden/retrieval_calibration.json.  No GPU.

  python scripts/calibrate_retrieval.py [--check]       --check: recompute and compare with the committed file, write nothing"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import retrieval_cases as rc


def main():
    t0 = time.time()
    rows = rc.calibration()
    path = os.path.join(ROOT, "tests", "golden", rc.CALIBRATION_JSON)
    doc = dict(tool="calibrate_retrieval", corridor=rc.CORRIDOR, cluster=rc.CLUSTER, track_scene=rc.TRACK_SCENE, track_setting=rc.TRACK_SETTING,
               default=rc.DEFAULT, rows=rows)
    for r in rows:
        print(json.dumps(r))
    if "--check" in sys.argv[1:]:
        with open(path) as f:
            same = json.load(f)["rows"] == json.loads(json.dumps(rows))
        print(f"calibrate_retrieval: {'equal to' if same else 'DIFFERS from'} {path} ({time.time() - t0:.0f} s)")
        return 0 if same else 1
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"calibrate_retrieval: {len(rows)} rows -> {path} ({time.time() - t0:.0f} s)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
