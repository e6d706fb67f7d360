"""What the per-frame leg of many sequences costs, timed on an MI355X with n = 8 and n = 32 trackers on different C3 tracker scenarios (640 x 480, the scenes of
tests/tracker_common.py with seeds 20260925 + i), all on one stream:
  (a) n sequential ldso_tr_track calls (one per handle: k_tr_track<16>, an upload, a download and a wait each) against ONE ldso_tr_group_track on the same handles
      from the same guesses (the identity)
  (b) n sequential ldso_tr_track_new_coarse calls on the not-lost path (one try each) against ONE ldso_tr_group_track_new_coarse
The two legs of a step alternate call by call on the SAME handles (the members of the group stay usable on their own), through the C entries with buffers allocated
once; the median of `--reps` calls after `--warmup` is reported with the 10th / 90th percentile, the ratio of the medians, the cooperation width G of the grouped
launch and whether the grouped median lies below the sequential leg's 10th percentile - one JSON line per group size.  Every call ends in a stream synchronisation, so
the host clock around it is the call's time; `device_span_us` is the time between two events on the stream around the grouped call (upload, kernel and download).
The first round checks that the legs agree (byte for byte where the grouped launch runs the solo width 16, to 1e-4 in the pose otherwise).  Nothing is asserted about
time.  Each group size runs as a child process of its own under `timeout`; the second does not start when the first failed.
    python scripts/time_tracker_group.py [--reps 50] [--warmup 5] [--n 8|32]"""
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
    return tracker_scenario("C3", seed=seed)


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
    trk = []
    for sc in scs:
        win = sc["win"]
        g = binding.Tracker(win.w, win.h, sc["levels"], win.settings, win.calib)
        g.set_stream(ts.cuda_stream)
        g.set_ref(sc["ref_pyr"], sc["ref_aff"][0], sc["ref_aff"][1], 1.0, sc["pts"])
        g.set_new_frame(sc["new_pyr"], 1.0)
        trk.append(g)
    grp = binding.TrackerGroup(trk)
    L = grp.L
    p = binding._p
    G = grp.coop_width(n)
    levels = scs[0]["levels"]
    T0 = np.ascontiguousarray(np.tile(np.eye(4)[:3, :4], (n, 1, 1)))
    ab0 = np.ascontiguousarray(np.array([sc["new_aff"] for sc in scs], np.float32))
    co = np.full(n, levels - 1, np.int32)

    def out():
        return dict(T=T0.copy(), ab=ab0.copy(), lr=np.zeros((n, 5)), fl=np.zeros((n, 3)), ok=np.zeros(n, np.int32), it=np.zeros(n, np.int32))

    def solo_track(o):
        for i, g in enumerate(trk):
            rc = L.ldso_tr_track(g.h, p(o["T"][i]), p(o["ab"][i]), C.c_int(levels - 1), None, p(o["lr"][i]), p(o["fl"][i]), p(o["ok"][i:i + 1]), p(o["it"][i:i + 1]))
            if rc:
                return rc
        return 0

    def group_track(o):
        return L.ldso_tr_group_track(grp.h, None, p(o["T"]), p(o["ab"]), p(co), None, p(o["lr"]), p(o["fl"]), p(o["ok"]), p(o["it"]))

    t_solo, t_grp, t_dev = [], [], []
    ea, eb = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for it in range(a.warmup + a.reps):
        so, go = out(), out()
        t_solo.append(timed(lambda: solo_track(so)))
        ea.record(ts)
        t_grp.append(timed(lambda: group_track(go)))
        eb.record(ts); eb.synchronize()
        t_dev.append(ea.elapsed_time(eb) * 1e-3)
        if it == 0:
            assert so["ok"].all() and go["ok"].all(), "a track failed: nothing to time"
            if G == 16:
                assert all(so[k].tobytes() == go[k].tobytes() for k in so), "the legs disagree: nothing to time"
            else:
                assert np.abs(so["T"] - go["T"]).max() < 1e-4, "the legs disagree: nothing to time"
    track = verdict(stats(t_solo[a.warmup:]), stats(t_grp[a.warmup:]))
    track["grouped_device_span_us"] = stats(t_dev[a.warmup:])["median_us"]

    # FullSystem::trackNewCoarse, not lost: the hypothesis list of three consecutive poses, lastCoarseRMSE far above what try 0 achieves
    w2c = [sc["win"].truth["w2c"] for sc in scs]
    F = scs[0]["win"].F
    P3 = lambda k: np.ascontiguousarray(np.stack([m[k][:3, :4] for m in w2c]), np.float64)
    sprelast, slast, lastF = P3(F - 2), P3(F - 1), P3(F - 1)
    pv, thr = np.ones(n, np.int32), np.full(n, 1.5)

    def out2():
        return dict(rmse=np.full((n, 5), 100.0), res4=np.zeros((n, 4)), w2c=np.zeros((n, 3, 4)), aff=np.zeros((n, 2), np.float32), tries=np.zeros(n, np.int32), good=np.zeros(n, np.int32))

    def solo_new(o):
        for i, g in enumerate(trk):
            rc = L.ldso_tr_track_new_coarse(g.h, p(sprelast[i]), p(slast[i]), p(lastF[i]), C.c_int(1), p(ab0[i]), p(o["rmse"][i]), C.c_double(1.5), p(o["res4"][i]), p(o["w2c"][i]),
                                            p(o["aff"][i]), p(o["tries"][i:i + 1]), p(o["good"][i:i + 1]))
            if rc:
                return rc
        return 0

    def group_new(o):
        return L.ldso_tr_group_track_new_coarse(grp.h, None, p(sprelast), p(slast), p(lastF), p(pv), p(ab0), p(o["rmse"]), p(thr), p(o["res4"]), p(o["w2c"]), p(o["aff"]),
                                                p(o["tries"]), p(o["good"]))

    t_solo, t_grp = [], []
    for it in range(a.warmup + a.reps):
        so, go = out2(), out2()
        t_solo.append(timed(lambda: solo_new(so)))
        t_grp.append(timed(lambda: group_new(go)))
        if it == 0:
            if not ((so["tries"] == 1).all() and (go["tries"] == 1).all() and so["good"].all() and go["good"].all()):
                print("tries / good, sequential:", so["tries"].tolist(), so["good"].tolist(), "grouped:", go["tries"].tolist(), go["good"].tolist(), file=sys.stderr)
                raise AssertionError("not the not-lost path: nothing to time")
            if G == 16:
                assert all(so[k].tobytes() == go[k].tobytes() for k in so), "the legs disagree: nothing to time"
            else:
                assert np.abs(so["w2c"] - go["w2c"]).max() < 1e-4, "the legs disagree: nothing to time"
    new_coarse = verdict(stats(t_solo[a.warmup:]), stats(t_grp[a.warmup:]))
    pc_n = [int(x) for x in trk[0].last_track_evals()[1][:levels]]
    print(json.dumps(dict(step="tracker_group", n=n, G=G, scene="C3 %d x %d, %d levels" % (scs[0]["win"].w, scs[0]["win"].h, levels), pc_n_member0=pc_n, reps=a.reps,
                          track=track, track_new_coarse=new_coarse)), flush=True)
    grp.close()
    for g in trk:
        g.close()


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
