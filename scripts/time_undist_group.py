"""The raw frames of n sequences on their way into their device pyramids, timed on an MI355X at 640 x 480, 8-bit, 4 pyramid levels, n = 8 and n = 32 members with
distinct frames, all on one stream:
  (a) n sequential ldso_undist_frame(..., pyr_i): n copies, n undistortion launches, n x 2 x levels pyramid launches
  (b) ONE ldso_undist_group_frames into a pyramid group: one copy of the n raw frames, one undistortion launch, 2 x levels pyramid launches
  (c) ldso_pyr_group_make_images from n HOST float irradiance images (4 bytes per pixel go up): the grouped path without this entry.  It presupposes the host
      undistortion (Undistort::undistort<T>, about 2.2 ms per frame on one core), which is NOT part of this number.
The three legs alternate call by call on the same handles (the members of a group stay usable on their own), through the C entries with buffers allocated once; each
leg is a host clock around the call(s) and ONE stream synchronisation behind them.  The median of `--reps` rounds after `--warmup` is reported with the 10th / 90th
percentile, and whether the median of (b) lies below the 10th percentile of (a).  For (b) also the host time of the call itself (before the synchronisation) and,
from rounds of their own with the event brackets on, its three stages: copy / undistortion kernel / pyramid build.  The first round checks that the three legs
leave the same bytes in every pyramid level.  Nothing is asserted about time.  Each group size runs as a child process of its own under `timeout`; the second does
not start when the first failed.  One JSON line per group size.
    python scripts/time_undist_group.py [--reps 50] [--warmup 5] [--n 8|32]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
STEP_TIMEOUT_S = 280
W, H, LEVELS = 640, 480, 4


def stats(t):
    t = np.asarray(t) * 1e6
    return dict(median_us=round(float(np.median(t)), 1), p10_us=round(float(np.percentile(t, 10)), 1), p90_us=round(float(np.percentile(t, 90)), 1))


def run(a):
    n = a.n
    import torch
    import undistort_common as uc
    from ldso_amd import binding
    rx, ry = uc.synthetic_tables(W, H, W, H)
    G = uc.golden()["G256"]
    vig = (1.0 / np.random.default_rng(1).uniform(0.4, 1.0, (H, W))).astype(np.float32)
    frames = [uc.textured_frames(W, H, seed=100 + i)[0] for i in range(n)]
    irr = [uc.undistort(f, rx, ry, W, H, W, H, G, vig, uc.VIGNETTE) for f in frames]
    ts = torch.cuda.Stream(); torch.cuda.set_stream(ts)
    st = C.c_void_p(ts.cuda_stream)
    und, pyr = [], []
    for i in range(n):
        U = binding.Undistorter(W, H, W, H)
        U.set_stream(ts.cuda_stream)
        U.set_remap(rx, ry)
        U.set_photometric(G, vig, 2)
        und.append(U)
        pyr.append(binding.Pyramid(W, H, LEVELS))
    ug, pg = binding.UndistorterGroup(und), binding.PyramidGroup(pyr)
    L = ug.L
    p = binding._p
    raw_ptrs = (C.c_void_p * n)(*[f.ctypes.data for f in frames])
    irr_ptrs = (C.c_void_p * n)(*[x.ctypes.data for x in irr])
    bpp, expo, fac, eout = np.ones(n, np.int32), np.ones(n, np.float32), np.ones(n, np.float32), np.zeros(n, np.float32)

    def solo():
        for U, f, q in zip(und, frames, pyr):
            rc = L.ldso_undist_frame(U.h, p(f), C.c_int(1), C.c_float(1.0), C.c_float(1.0), q.h, None)
            if rc:
                return rc
        return 0

    def grouped():
        return L.ldso_undist_group_frames(ug.h, None, raw_ptrs, p(bpp), p(expo), p(fac), pg.h, p(eout))

    def from_host():
        return L.ldso_pyr_group_make_images(pg.h, None, irr_ptrs, st)

    def timed(call):
        """(seconds until the leg's synchronisation has returned, seconds the call(s) took on the host)"""
        t0 = time.perf_counter()
        rc = call()
        t1 = time.perf_counter()
        ts.synchronize()
        t2 = time.perf_counter()
        assert rc == 0, (rc, L.ldso_last_error().decode())
        return t2 - t0, t1 - t0

    def fetch_levels():
        return [q.get_level(l).tobytes() for q in pyr for l in range(LEVELS)]

    legs = (("a", solo), ("b", grouped), ("c", from_host))
    t = {k: [] for k, _ in legs}
    host_b = []
    want = None
    for it in range(a.warmup + a.reps):
        for k, call in legs:
            total, host = timed(call)
            t[k].append(total)
            if k == "b":
                host_b.append(host)
            if it == 0:
                got = fetch_levels()
                want = want or got
                assert got == want, "the legs disagree: nothing to time"
    L.ldso_undist_group_profile(ug.h, C.c_int(1), None)
    split = []
    us = np.zeros(3, np.float32)
    for it in range(a.reps):
        assert grouped() == 0
        assert L.ldso_undist_group_profile(ug.h, C.c_int(1), p(us)) == 0
        split.append(us.copy())
    L.ldso_undist_group_profile(ug.h, C.c_int(0), None)
    split = np.median(np.asarray(split), axis=0)
    sa, sb, sc = (stats(t[k][a.warmup:]) for k in "abc")
    print(json.dumps(dict(step="undist_group", n=n, shape="%d x %d, 8-bit, %d levels" % (W, H, LEVELS), reps=a.reps,
                          a_sequential_undist_frame=sa, b_undist_group_frames=sb, c_pyr_group_make_images_from_host_float_excluding_host_undistortion=sc,
                          b_host_time_of_the_call=stats(host_b[a.warmup:]),
                          b_split_median_us=dict(copy=round(float(split[0]), 1), undistort=round(float(split[1]), 1), pyramid=round(float(split[2]), 1)),
                          ratio_a_over_b=round(sa["median_us"] / sb["median_us"], 2), b_median_below_a_p10=bool(sb["median_us"] < sa["p10_us"]))), flush=True)
    ug.close()
    pg.close()
    for x in und + pyr:
        x.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50); ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--n", type=int, choices=(8, 32))
    a = ap.parse_args()
    if a.n:
        run(a)
        return 0
    for n in (8, 32):
        rc = subprocess.run(["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--n", str(n), "--reps", str(a.reps), "--warmup", str(a.warmup)]).returncode
        if rc != 0:
            print(f"n = {n} ended with status {rc}: stopping", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
