"""Calibrates the defaults of `verify_pairs(homography=...)` on the CPU with the restatement tests/np_verify_h.py at the default budget
(docs/tracks.md §13.4): every planted scene of tests/verify_h_cases.py at every threshold of the grid, the rules of `chosen_defaults`.
  python scripts/calibrate_verify_h.py [--write]      --write: tests/golden/verify_h_calibration.json"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import verify_h_cases as hc  # noqa: E402


def main():
    rows = hc.calibration()
    thr, table = hc.chosen_threshold(rows)
    print("threshold: planar recall by keep_h / general recall by keep / planar outliers kept by keep_h, per (share, m)")
    for t, cells in table.items():
        print(f"  {t} px: " + "; ".join(f"({f}, {m}) {100 * a:.1f} / {100 * b:.1f} / {100 * c:.2f}" for f, m, a, b, c in cells))
    print("chosen threshold:", thr)
    if thr is None:
        return 1
    for what in ("ratio", "spread"):
        print(what, hc.separation(rows, thr, what))
    settings = hc.chosen_defaults(rows)
    print("defaults:", settings)
    print("misclassified at the defaults:", hc.misclassified(rows, settings))
    print(hc.format_table(rows, thr))
    if "--write" in sys.argv[1:]:
        from datagen import GOLDEN
        with open(os.path.join(GOLDEN, hc.CALIBRATION_JSON), "w") as f:
            json.dump(dict(budget=hc.BUDGET, thresholds=list(hc.THRESHOLDS), defaults=settings, rows=rows), f, indent=0)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
