"""Writes tests/golden/track_cal_calibration.json: what the restatement tests/np_track_cal.py reaches on the calibration scenes of
docs/tracks.md §15.4 with (f, k1) free, and what the fixed-K adjustment reaches from the same start.  No GPU.

  python scripts/calibrate_track_cal.py [--check]      (--check: print, do not write)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import track_cal_cases as cc  # noqa: E402


def main():
    out = dict(about="settings and the figures tests/np_track_cal.py reaches (scripts/calibrate_track_cal.py); bars are halfway between "
                     "'calibrated' and 'fixed'", planted=cc.PLANTED, nominal_f=cc.NOMINAL_F, free=list(cc.FREE), scenes={})
    for name in cc.SCENES:
        s = cc.scene(name)
        rec = dict(ncam=len(s["cams"]), npt=len(s["X"]), nobs=len(s["obs"]), huber=s["huber"], iters=s["iters"],
                   planted=dict(f=float(s["theta_true"][0]), k1=float(s["theta_true"][3]), k2=float(s["theta_true"][4])),
                   start_f=float(s["K"][0, 0]), calibrated=cc.run_scene(s, cc.host_adjust, cc.FREE), fixed=cc.run_scene(s, cc.host_adjust, 0))
        out["scenes"][name] = rec
        print(name, json.dumps(rec, indent=None))
    if "--check" not in sys.argv:
        with open(cc.FIXTURE, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
