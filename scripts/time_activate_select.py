"""Candidate selection of FullSystem::activatePointsMT, timed on ONE state (C3: 7 key frames, ~1700 seeds, several thousand candidates) for currentMinActDist 1 and 4:
the device selection alone (ldso_ba_select_candidates: upload, one kernel, download, one wait), the fused call (ldso_ba_select_activate_points: plus k_activate on
the selected list) and the reference's host loop through its compiled CoarseDistanceMap on one core of the same machine (adp_ref_select_candidates).
Median of `--reps` calls after `--warmup`, with the 10th / 90th percentile beside it; one JSON line per distance.
    python scripts/time_activate_select.py [--reps 50] [--warmup 5] [--per-frame 1200]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def stats(t):
    t = np.asarray(t) * 1e6
    return dict(median_us=round(float(np.median(t)), 1), p10_us=round(float(np.percentile(t, 10)), 1), p90_us=round(float(np.percentile(t, 90)), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50); ap.add_argument("--warmup", type=int, default=5); ap.add_argument("--per-frame", type=int, default=1200)
    a = ap.parse_args()
    from ldso_amd import binding
    import activation_select_common as asc
    win, (r,), _ = asc.make_state("C3", per_frame=a.per_frame)
    g = asc.gather(r)
    ba = binding.BA.from_window(win)
    args = (g["seeds"], g["cand"], g["my_type"], g["KRKi"], g["Kt"], g["flagged"])
    for d in (1.0, 4.0):
        ref = asc.ref_select(r, d)
        dec, sel = ba.select_candidates(*args, d)
        assert np.array_equal(dec, ref["decision"]) and np.array_equal(sel, ref["selected"]), "the legs disagree: nothing to time"
        legs = {}
        for name, call in (("device_select", lambda: ba.select_candidates(*args, d)), ("device_select_activate", lambda: ba.select_activate_points(*args, d))):
            t = []
            for i in range(a.warmup + a.reps):
                t0 = time.perf_counter(); call(); t.append(time.perf_counter() - t0)
            legs[name] = stats(t[a.warmup:])
        legs["reference_host_one_core"] = stats(asc.time_ref_select(r, d, a.warmup + a.reps)[a.warmup:])
        print(json.dumps(dict(currentMinActDist=d, seeds=len(g["seeds"]), candidates=len(g["cand"]), selected=len(sel), reps=a.reps, **legs)))
    ba.close(); r.close()


if __name__ == "__main__":
    main()
