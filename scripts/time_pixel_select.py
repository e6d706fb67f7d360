"""Time the device pixel selection on the MI355X: median of 50 calls (after 3) of ldso_pixsel_make_maps + ldso_pixsel_make_points at 640 x 480 with
setting_desiredImmatureDensity's default (1500), wall clock around both calls (their waits included), plus the kernels' split from ldso_pixsel_profile (median of
ten further calls bracketed with HIP events), for
  - the synthetic scene (8-bit valued), from potential 3;
  - an 8-bit image of axis-aligned step edges from potential 1: nearly every pot block that selects depends on its direction, the worst case for the
    sequential part of the scan.
The yardstick is the reference's own makeMaps on one core: scripts/golden/make_ref_pixel_select.py --time (same images, same density, same start potentials).

    python scripts/time_pixel_select.py [--reps 50]"""
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
    import pixel_select_common as pc
    from ldso_amd import binding
    w, h, density = 640, 480, 1500.0
    rp = np.random.default_rng(3).integers(0, 256, w * h).astype(np.uint8)
    for name, img, pot in (("scene", np.clip(np.rint(fc.scene(w, h)[0]), 0, 255), 3), ("step edges, potential 1", pc.steps_image(w, h), 1)):
        pyr = binding.Pyramid(w, h, 3).make_images(img.astype(np.float32))
        sel = binding.PixelSelector(w, h, rp)
        t, us = [], []
        for r in range(3 + a.reps + 10):
            sel.potential = pot
            sel.profile(r >= 3 + a.reps)          # the last ten calls with events: the split; the calls before without: the wall time
            t0 = time.perf_counter()
            n, counts, used = sel.make_maps(pyr, density)
            k = sel.make_points(pyr, 0)
            dt = time.perf_counter() - t0
            if r >= 3 + a.reps:
                us.append(sel.profile(True).copy())
            elif r >= 3:
                t.append(dt)
        us = np.median(np.array(us), 0)
        print(f"make_maps + make_points 640x480 density 1500, {name}: {n} pixels ({k} points), counts {counts}, potential {pot} -> {used}, "
              f"median of {len(t)}: {np.median(t) * 1e6:.1f} us; kernels: histogram {us[0]:.1f}, masks + scan {us[1]:.1f}, select {us[2]:.1f}, "
              f"thinning {us[3]:.1f}, records {us[4]:.1f} us")
        sel.close(); pyr.close()


if __name__ == "__main__":
    main()
