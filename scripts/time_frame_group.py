"""What the per-frame leg of many sequences costs around the grouped tracking step, timed on an MI355X with n = 8 and n = 32 sequences on different C3 scenes
(640 x 480, 4 pyramid levels, the scenes of tests/tracker_common.py with seeds 20260925 + i, 1000 fresh immature points on each of the 7 key frames = 7000 per
member), all on one stream:
  (a) n sequential ldso_pyr_make_images (2 x 4 launches each) against ONE ldso_pyr_group_make_images (2 x 4 launches for all), a stream synchronisation closing both legs
  (b) n sequential ldso_trace_on (an upload, a memset, a launch, a download and a wait each) against ONE ldso_trace_group_on
  (c) the whole frame leg: the build, ldso_tr_set_new_frame_pyramid and ldso_trace_set_frame_pyramid per member, ldso_tr_group_track, the trace - solo build and solo
      traces against the grouped ones, the tracking grouped in both legs
The two legs of a pair alternate call by call on the SAME handles (the members of a group stay usable on their own), through the C entries with buffers allocated
once.  A trace changes the records it works on, so every traced leg starts from the same records: they are set again, outside the clock, before each leg.  The median
of `--reps` calls after `--warmup` is reported with the 10th / 90th percentile, the ratio of the medians and whether the grouped median lies below the sequential
leg's 10th percentile - one JSON line per group size.  The first round checks that the legs agree byte for byte (every pyramid level, the records, the counts).
Nothing is asserted about time.  Each group size runs as a child process of its own under `timeout`; the second does not start when the first failed.
    python scripts/time_frame_group.py [--reps 50] [--warmup 5] [--n 8|32]"""
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
STEP_TIMEOUT_S = 560
SEED0 = 20260925
PER_FRAME = 1000


def stats(t):
    t = np.asarray(t) * 1e6
    return dict(median_us=round(float(np.median(t)), 1), p10_us=round(float(np.percentile(t, 10)), 1), p90_us=round(float(np.percentile(t, 90)), 1))


def timed(call):
    t0 = time.perf_counter()
    rc = call()
    dt = time.perf_counter() - t0
    assert rc == 0, rc
    return dt


def make_scene(seed):
    from tracker_common import tracker_scenario
    from ldso_amd import synth
    sc = tracker_scenario("C3", seed=seed)
    win = sc["win"]
    sc["immature"], _ = synth.make_immature_points(win, PER_FRAME)
    sc["trace_poses"] = synth.trace_poses(win, win.F)
    sc["color"] = np.ascontiguousarray(sc["new_pyr"][0][:, :, 0])
    return sc


def verdict(seq, grp):
    return dict(sequential=seq, grouped=grp, ratio=round(seq["median_us"] / grp["median_us"], 2), grouped_median_below_sequential_p10=bool(grp["median_us"] < seq["p10_us"]))


def run(a):
    n = a.n
    # the scenes first, on a few cores, before anything opens the device
    from concurrent.futures import ProcessPoolExecutor
    with ProcessPoolExecutor(max_workers=min(8, n)) as ex:
        scs = list(ex.map(make_scene, [SEED0 + i for i in range(n)]))
    import torch
    from ldso_amd import binding
    ts = torch.cuda.Stream(); torch.cuda.set_stream(ts)
    st = C.c_void_p(ts.cuda_stream)
    levels = scs[0]["levels"]
    trk, trc, pyr = [], [], []
    for sc in scs:
        win = sc["win"]
        g = binding.Tracker(win.w, win.h, levels, win.settings, win.calib)
        g.set_stream(ts.cuda_stream)
        g.set_ref(sc["ref_pyr"], sc["ref_aff"][0], sc["ref_aff"][1], 1.0, sc["pts"])
        trk.append(g)
        t = binding.Tracer(win.w, win.h, len(sc["immature"]))
        t.set_stream(ts.cuda_stream)
        trc.append(t)
        pyr.append(binding.Pyramid(win.w, win.h, levels))
    tg, cg, pg = binding.TrackerGroup(trk), binding.TracerGroup(trc), binding.PyramidGroup(pyr)
    L = tg.L
    p = binding._p

    colors = [sc["color"] for sc in scs]
    color_ptrs = (C.c_void_p * n)(*[c.ctypes.data for c in colors])
    poses = [[np.ascontiguousarray(x, np.float32) for x in sc["trace_poses"]] for sc in scs]
    pose_ptrs = [(C.c_void_p * n)(*[ps[q].ctypes.data for ps in poses]) for q in range(3)]
    nh = np.array([len(ps[0]) for ps in poses], np.int32)
    T0 = np.ascontiguousarray(np.tile(np.eye(4)[:3, :4], (n, 1, 1)))
    ab0 = np.ascontiguousarray(np.array([sc["new_aff"] for sc in scs], np.float32))
    co = np.full(n, levels - 1, np.int32)

    def sync():
        ts.synchronize()
        return 0

    def solo_build():
        for q, c in zip(pyr, colors):
            rc = L.ldso_pyr_make_images(q.h, p(c), st)
            if rc:
                return rc
        return 0

    def group_build():
        return L.ldso_pyr_group_make_images(pg.h, None, color_ptrs, st)

    def hand_over():
        for g, t, q in zip(trk, trc, pyr):
            rc = L.ldso_tr_set_new_frame_pyramid(g.h, q.h, C.c_float(1.0)) or L.ldso_trace_set_frame_pyramid(t.h, q.h)
            if rc:
                return rc
        return 0

    def solo_trace(counts):
        for i, t in enumerate(trc):
            rc = L.ldso_trace_on(t.h, C.c_int(int(nh[i])), p(poses[i][0]), p(poses[i][1]), p(poses[i][2]), p(counts[i]))
            if rc:
                return rc
        return 0

    def group_trace(counts):
        return L.ldso_trace_group_on(cg.h, None, p(nh), pose_ptrs[0], pose_ptrs[1], pose_ptrs[2], p(counts))

    def track(o):
        return L.ldso_tr_group_track(tg.h, None, p(o["T"]), p(o["ab"]), p(co), None, p(o["lr"]), p(o["fl"]), p(o["ok"]), p(o["it"]))

    def track_out():
        return dict(T=T0.copy(), ab=ab0.copy(), lr=np.zeros((n, 5)), fl=np.zeros((n, 3)), ok=np.zeros(n, np.int32), it=np.zeros(n, np.int32))

    def reset_records():
        for t, sc in zip(trc, scs):
            t.set_points(sc["immature"])

    def fetch_levels():
        return [q.get_level(l).tobytes() for q in pyr for l in range(levels)]

    def fetch_records():
        return [t.get_points().tobytes() for t in trc]

    # (a) the build
    t_solo, t_grp = [], []
    for it in range(a.warmup + a.reps):
        t_solo.append(timed(lambda: solo_build() or sync()))
        if it == 0:
            want = fetch_levels()
        t_grp.append(timed(lambda: group_build() or sync()))
        if it == 0:
            assert fetch_levels() == want, "the legs disagree: nothing to time"
    build = verdict(stats(t_solo[a.warmup:]), stats(t_grp[a.warmup:]))

    # (b) the trace, on the frames the last build left
    assert hand_over() == 0
    t_solo, t_grp = [], []
    for it in range(a.warmup + a.reps):
        cs, cgp = np.zeros((n, 6), np.int32), np.zeros((n, 6), np.int32)
        reset_records()
        t_solo.append(timed(lambda: solo_trace(cs)))
        if it == 0:
            want = fetch_records()
        reset_records()
        t_grp.append(timed(lambda: group_trace(cgp)))
        if it == 0:
            assert fetch_records() == want and np.array_equal(cs, cgp), "the legs disagree: nothing to time"
            counts0 = cs[0].tolist()
    trace = verdict(stats(t_solo[a.warmup:]), stats(t_grp[a.warmup:]))

    # (c) the whole frame leg
    t_solo, t_grp = [], []
    for it in range(a.warmup + a.reps):
        cs, cgp = np.zeros((n, 6), np.int32), np.zeros((n, 6), np.int32)
        so, go = track_out(), track_out()
        reset_records()
        t_solo.append(timed(lambda: solo_build() or hand_over() or track(so) or solo_trace(cs)))
        if it == 0:
            want = fetch_records()
        reset_records()
        t_grp.append(timed(lambda: group_build() or hand_over() or track(go) or group_trace(cgp)))
        if it == 0:
            assert so["ok"].all() and go["ok"].all(), "a track failed: nothing to time"
            assert fetch_records() == want and np.array_equal(cs, cgp) and np.abs(so["T"] - go["T"]).max() < 1e-4, "the legs disagree: nothing to time"
    frame = verdict(stats(t_solo[a.warmup:]), stats(t_grp[a.warmup:]))

    print(json.dumps(dict(step="frame_group", n=n, scene="C3 %d x %d, %d levels" % (scs[0]["win"].w, scs[0]["win"].h, levels), immature_per_member=len(scs[0]["immature"]),
                          trace_counts_member0=counts0, reps=a.reps, build=build, trace=trace, frame_leg=frame)), flush=True)
    for grp in (tg, cg, pg):
        grp.close()
    for h in trk + trc + pyr:
        h.close()


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
