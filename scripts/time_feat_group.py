"""What the corner features of a key frame cost when many sequences make one in the same step (FullSystem::makeNewTraces, FullSystem.cc:1272-1325, for
setting_pointSelection == 1), timed on an MI355X at n = 8 and n = 32 sequences: 640 x 480, 1500 wanted features, every sequence a scene of its own
(synth.make_window, seeds 20261021 + i), the ORB pattern set.  Two legs, alternating call by call:
  (a) n sequential ldso_feat_detect + ldso_trace_append_points_device (per sequence: a memset, five launches, a download and a wait, then two copies and a wait);
  (b) ONE ldso_feat_group_detect with the tracers over a group of n twin detectors (one upload, six launches, one download, one wait).
The tracers of both legs are emptied before every call, outside the clock, so every call does the same work.  Through the C entries with buffers allocated once; the
median of `--reps` calls after `--warmup` is reported with the 10th / 90th percentile, one JSON line per n.  Every call ends in a stream synchronisation, so the host
clock around it is the call's time.  Behind the clock the per-stage split of the grouped call (ldso_feat_group_profile: cells + compaction, corners, angle +
descriptor, records, append; median of `--reps` profiled calls) and of one member's solo call (ldso_feat_profile) are taken, and the legs are compared once: counts,
features, records and the tracers byte for byte.  Nothing is asserted about time.  Each n runs as a child process of its own under `timeout`; the second does not
start when the first failed.
    python scripts/time_feat_group.py [--reps 50] [--warmup 5] [--batch 8|32]"""
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
W, H, WANTED, SEED0 = 640, 480, 1500, 20261021


def make_scene(seed):
    from ldso_amd import synth
    win = synth.make_window(F=2, P=50, w=W, h=H, fx=W * 0.6, seed=seed)
    return np.ascontiguousarray(win.images[0][0][..., 0], np.float32)


def stats(t):
    t = np.asarray(t) * 1e6
    return dict(median_us=round(float(np.median(t)), 1), p10_us=round(float(np.percentile(t, 10)), 1), p90_us=round(float(np.percentile(t, 90)), 1))


def timed(call):
    t0 = time.perf_counter()
    rc = call()
    dt = time.perf_counter() - t0
    assert rc == 0, rc
    return dt


def run(a):
    n = a.batch
    # the scenes first, on a few cores, before anything opens the device
    from concurrent.futures import ProcessPoolExecutor
    with ProcessPoolExecutor(max_workers=min(8, n)) as ex:
        scenes = list(ex.map(make_scene, [SEED0 + i for i in range(n)]))
    import torch
    import feature_detect_common as fc
    from ldso_amd import binding, synth
    ts = torch.cuda.Stream(); torch.cuda.set_stream(ts)
    cap = binding.Features.grid(W, H, WANTED)["capacity"]
    pattern = fc.golden()["pattern"]
    pyr = [binding.Pyramid(W, H, 1).make_images(s) for s in scenes]
    legs = []
    for _ in range(2):
        dets, trs = [], []
        for _i in range(n):
            d = binding.Features(W, H, cap, pattern); d.set_stream(ts.cuda_stream)
            t = binding.Tracer(W, H, cap); t.set_stream(ts.cuda_stream)
            dets.append(d); trs.append(t)
        legs.append((dets, trs))
    (solo, solo_tr), (grouped, group_tr) = legs
    grp = binding.FeaturesGroup(grouped)
    L = grp.L
    none = np.zeros(0, synth.IMMATURE_DTYPE)

    def empty(trs):
        for t in trs:
            t.set_points(none)

    cnt_solo = [C.c_int() for _ in range(n)]
    cor_solo = [C.c_int() for _ in range(n)]

    def sequential():
        for i in range(n):
            rc = L.ldso_feat_detect(solo[i].h, pyr[i].h, C.c_int(WANTED), C.c_int(i % 7), C.byref(cnt_solo[i]), C.byref(cor_solo[i]))
            if rc:
                return rc
            dev = C.c_void_p()
            L.ldso_feat_device(solo[i].h, None, C.byref(dev), None)
            rc = L.ldso_trace_append_points_device(solo_tr[i].h, cnt_solo[i], dev)
            if rc:
                return rc
        return 0

    P = (C.c_void_p * n)(*[p.h for p in pyr])
    T = (C.c_void_p * n)(*[t.h for t in group_tr])
    nf = np.full(n, WANTED, np.int32)
    host = (np.arange(n) % 7).astype(np.int32)
    cnt = np.zeros(n, np.int32); cor = np.zeros(n, np.int32); sta = np.zeros(n, np.int32)

    def one_group_call():
        return L.ldso_feat_group_detect(grp.h, None, P, binding._p(nf), binding._p(host), T, binding._p(cnt), binding._p(cor), binding._p(sta))

    t_solo, t_group = [], []
    for _ in range(a.warmup + a.reps):
        empty(solo_tr); empty(group_tr)
        t_solo.append(timed(sequential))
        t_group.append(timed(one_group_call))
    # the legs agree: counts, features, records, tracers
    for i in range(n):
        solo[i].n = cnt_solo[i].value; grouped[i].n = int(cnt[i]); solo_tr[i].n = cnt_solo[i].value; group_tr[i].n = int(cnt[i])
        same = cnt_solo[i].value == cnt[i] and cor_solo[i].value == cor[i] and all(x.tobytes() == y.tobytes() for x, y in zip(solo[i].get(), grouped[i].get()))
        same = same and solo_tr[i].get_points().tobytes() == group_tr[i].get_points().tobytes() and solo_tr[i].get_point_types().tobytes() == group_tr[i].get_point_types().tobytes()
        assert same and cnt[i] > 0, "the legs disagree: nothing to time"
    # the per-stage splits, behind the clock
    grp.profile(True)
    split = []
    for _ in range(a.reps):
        empty(group_tr)
        assert one_group_call() == 0
        split.append(grp.profile(True).copy())
    grp.profile(False)
    solo[0].profile(True)
    solo_split = []
    for _ in range(a.reps):
        solo[0].detect(pyr[0], WANTED, 0)
        solo_split.append(solo[0].profile(True).copy())
    stages = ("cells_compaction", "corners", "angle_descriptor", "records", "append")
    out = dict(step="feat_group", n=n, reps=a.reps, features_per_member=int(np.mean(cnt)), corners_per_member=int(np.mean(cor)),
               sequential=stats(t_solo[a.warmup:]), grouped=stats(t_group[a.warmup:]),
               grouped_split_us={k: round(float(v), 1) for k, v in zip(stages, np.median(np.array(split), axis=0))},
               solo_split_us={k: round(float(v), 1) for k, v in zip(stages[:4], np.median(np.array(solo_split), axis=0))})
    print(json.dumps(out), flush=True)
    grp.close()
    for x in solo + grouped + solo_tr + group_tr + pyr:
        x.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50); ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, choices=(8, 32))
    a = ap.parse_args()
    if a.batch:
        run(a)
        return 0
    for n in (8, 32):
        rc = subprocess.run(["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--batch", str(n), "--reps", str(a.reps), "--warmup", str(a.warmup)]).returncode
        if rc != 0:
            print(f"n = {n} ended with status {rc}: stopping", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
