"""Time the first frame of the monocular initialiser on the MI355X at 640 x 480 with 4 levels, median of 50 calls (after 3), the two legs alternating:
  (a) ldso_init_set_first_frame from a resident pyramid: selection, records and makeNN by the library; its split from ldso_init_first_profile
      (level-0 maps, coarser-level maps, records, tree build on the host, searches, the existing schedule build with its uploads);
  (b) ldso_init_set_first with the finished records of (a) and the frame as a host image: what a caller paid before, EXCLUDING the selection and the
      k-d tree it had to run on the host first.
The yardstick for (a) is the reference's own setFirst on one core: scripts/golden/make_ref_init_first.py --time (same image, same size, sparsityFactor 5).

    python scripts/time_init_first.py [--reps 50]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    import feature_detect_common as fc
    from ldso_amd import binding
    w, h, L = 640, 480, 4
    K4 = (500.0, 500.0, 319.5, 239.5)
    img = np.clip(np.rint(fc.scene(w, h)[0]), 0, 255).astype(np.float32)
    rp = np.random.default_rng(3).integers(0, 256, w * h).astype(np.uint8)
    pyr = binding.Pyramid(w, h, L).make_images(img)
    sel = binding.PixelSelector(w, h, rp)
    ini, old = binding.Initializer(w, h, L), binding.Initializer(w, h, L)
    ini.first_profile(True)
    ta, tb, us = [], [], []
    for r in range(3 + a.reps):
        ini.sparsity = 5
        t0 = time.perf_counter()
        n = ini.set_first_frame(K4, pyr, sel)
        t1 = time.perf_counter()
        recs = [ini.points(l) for l in range(L)]
        t2 = time.perf_counter()
        old.set_first(K4, img, recs)
        t3 = time.perf_counter()
        if r >= 3:
            ta.append(t1 - t0); tb.append(t3 - t2); us.append(ini.first_profile(True).copy())
    us = np.median(np.array(us), 0)
    print(f"set_first_frame 640x480, 4 levels, scene: numPoints {n}, sparsity left {ini.sparsity}, median of {len(ta)}: {np.median(ta) * 1e6:.1f} us; "
          f"split: level-0 maps {us[0]:.1f}, coarser maps {us[1]:.1f}, records {us[2]:.1f}, tree build (host) {us[3]:.1f}, searches {us[4]:.1f}, "
          f"schedules + uploads + image copies {us[5]:.1f} us")
    print(f"set_first with finished records and a host image (no selection, no k-d tree): median {np.median(tb) * 1e6:.1f} us")
    for x in (ini, old, sel, pyr):
        x.close()


if __name__ == "__main__":
    main()
