"""A camera frame's way into its device pyramid, timed at 640 x 480, 8-bit, 4 pyramid levels, in one process:
  (a) today's path: ldso_pyr_make_images from a HOST float irradiance image (4 bytes per pixel go up).  It presupposes the host undistortion
      (Undistort::undistort<T>), which is NOT part of this number: scripts/golden/make_ref_undistort.py --time measures that on the host (needs the LDSO sources).
  (b) ldso_undist_frame: the raw frame goes up (1 byte per pixel), photometric + geometric undistortion and the pyramid build run on the device.
Each number is a host clock around the call and a device synchronisation behind it, the two paths alternating call by call: median of `--reps` after
`--warmup`, with the 10th / 90th percentile.  Then, in calls of their own with the event brackets on, the split of (b): copy / undistortion kernel / pyramid.
The result of (b) is checked against the numpy restatement first.  One JSON line.
    python scripts/time_undistort.py [--reps 50] [--warmup 10]"""
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
    ap.add_argument("--width", type=int, default=640); ap.add_argument("--height", type=int, default=480); ap.add_argument("--levels", type=int, default=4)
    a = ap.parse_args()
    import torch
    from ldso_amd import binding
    import undistort_common as uc
    w, h = a.width, a.height
    rx, ry = uc.synthetic_tables(w, h, w, h)
    f8, _ = uc.textured_frames(w, h)
    G = uc.golden()["G256"]
    vig = (1.0 / np.random.default_rng(1).uniform(0.4, 1.0, (h, w))).astype(np.float32)
    U = binding.Undistorter(w, h, w, h)
    U.set_remap(rx, ry)
    U.set_photometric(G, vig, 2)
    pa, pb = binding.Pyramid(w, h, a.levels), binding.Pyramid(w, h, a.levels)
    irr = uc.undistort(f8, rx, ry, w, h, w, h, G, vig, uc.VIGNETTE)
    U.frame(f8, 1.0, 1.0, pyr=pb)
    pa.make_images(irr)
    assert np.array_equal(U.get(), irr) and all(pa.get_level(l).tobytes() == pb.get_level(l).tobytes() for l in range(a.levels)), "device and restatement disagree: nothing to time"
    sync = torch.cuda.synchronize
    ta, tb = [], []
    for i in range(a.warmup + a.reps):
        sync(); t0 = time.perf_counter(); pa.make_images(irr); sync(); ta.append(time.perf_counter() - t0)
        sync(); t0 = time.perf_counter(); U.frame(f8, 1.0, 1.0, pyr=pb); sync(); tb.append(time.perf_counter() - t0)
    ta, tb = np.asarray(ta[a.warmup:]) * 1e6, np.asarray(tb[a.warmup:]) * 1e6
    U.profile(True)
    split = []
    for i in range(a.reps):
        U.frame(f8, 1.0, 1.0, pyr=pb)
        split.append(U.profile(True))
    U.profile(False)
    split = np.median(np.asarray(split), axis=0)
    q = lambda t: dict(median_us=round(float(np.median(t)), 1), p10_us=round(float(np.percentile(t, 10)), 1), p90_us=round(float(np.percentile(t, 90)), 1))
    print(json.dumps(dict(w=w, h=h, levels=a.levels, reps=a.reps, a_make_images_from_host_float=q(ta), b_undist_frame_into_pyramid=q(tb),
                          b_split_median_us=dict(copy=round(float(split[0]), 1), undistort=round(float(split[1]), 1), pyramid=round(float(split[2]), 1)))))
    for x in (U, pa, pb):
        x.close()


if __name__ == "__main__":
    main()
