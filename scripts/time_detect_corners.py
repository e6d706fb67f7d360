"""ldso_feat_detect (FeatureDetector::DetectCorners + the ImmaturePoint constructors on the device) timed at 640 x 480, n = 1500 wanted features, on the image
of tests/feature_detect_common.scene: a host clock around the call, which ends in its one stream synchronisation - median of `--reps` calls after `--warmup`,
with the 10th / 90th percentile; then, in calls of their own with the event brackets on, the split by kernel group.  One JSON line.  The result is checked
against the numpy restatement first.  The host side of the comparison is scripts/golden/make_ref_detect_corners.py --time (needs the LDSO sources).
    python scripts/time_detect_corners.py [--reps 50] [--warmup 10]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50); ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--width", type=int, default=640); ap.add_argument("--height", type=int, default=480); ap.add_argument("-n", type=int, default=1500)
    a = ap.parse_args()
    from ldso_amd import binding
    import feature_detect_common as fc
    w, h, n = a.width, a.height, a.n
    irr, dI = fc.scene(w, h)
    pyr = binding.Pyramid(w, h, 1).make_images(irr)
    det = binding.Features(w, h, binding.Features.grid(w, h, n)["capacity"], fc.golden()["pattern"])
    nf, nc = det.detect(pyr, n)
    F, _ = det.get()
    R = fc.detect(dI, n, None, fc.golden()["pattern"])
    W = R["features"]
    assert nf == len(W) and nc == R["n_corners"] and np.array_equal(F["u"], W["u"]) and np.array_equal(F["v"], W["v"]) \
        and np.array_equal(F["score"].view(np.uint32), W["score"].view(np.uint32)) and np.array_equal(F["is_corner"], W["is_corner"]), "device and restatement disagree: nothing to time"
    t = []
    for i in range(a.warmup + a.reps):
        t0 = time.perf_counter(); det.detect(pyr, n); t.append(time.perf_counter() - t0)
    t = np.asarray(t[a.warmup:]) * 1e6
    det.profile(True)
    split = []
    for i in range(a.reps):
        det.detect(pyr, n)
        split.append(det.profile(True))
    det.profile(False)
    split = np.median(np.asarray(split), axis=0)
    print(json.dumps(dict(w=w, h=h, n=n, features=nf, corners=nc, reps=a.reps, call_median_us=round(float(np.median(t)), 1), call_p10_us=round(float(np.percentile(t, 10)), 1),
                          call_p90_us=round(float(np.percentile(t, 90)), 1),
                          kernels_median_us=dict(cells=round(float(split[0]), 1), corners=round(float(split[1]), 1), angle_descriptor=round(float(split[2]), 1), records=round(float(split[3]), 1)))))
    det.close(); pyr.close()


if __name__ == "__main__":
    main()
