"""What it costs to drop a marginalised frame's records from the immature sets of many sequences (FullSystem.cc:602-645), timed on an MI355X at n = 8 and n = 32
tracers, each holding the about 7200 traced candidates of a C3 window of its own (7 key frames, 640 x 480, seeds 20260925 + i, 1200 per key frame but the newest;
tests/batch_activate_common.py).  The host map removes the middle key frame and shifts the hosts behind it, so a sixth of every tracer's records leaves.  Two legs,
alternating call by call:
  (a) n sequential ldso_trace_compact calls with the host map (one per tracer: an upload, two launches, a 4-byte download and a wait each);
  (b) ONE ldso_trace_group_compact over a group of n twin tracers (one upload, two launches, one download, one wait).
Both sets of tracers are loaded again with the full records before every call, outside the clock, so every call does the same work.  Through the C entries with
buffers allocated once; the median of `--reps` calls after `--warmup` is reported with the 10th / 90th percentile, one JSON line per n.  Every call ends in a stream
synchronisation, so the host clock around it is the call's time.  After the clock has stopped the legs are compared once: counts, records and types byte for byte.
Nothing is asserted about time.  Each n runs as a child process of its own under `timeout`; the second does not start when the first failed.
    python scripts/time_trace_group_compact.py [--reps 50] [--warmup 5] [--batch 8|32]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
STEP_TIMEOUT_S = 560


def run(a):
    from time_batch_activate import make_c3, stats, timed, SEED0
    n = a.batch
    # the windows and their candidates first, on a few cores, before anything opens the device
    from concurrent.futures import ProcessPoolExecutor
    with ProcessPoolExecutor(max_workers=min(8, n)) as ex:
        made = list(ex.map(make_c3, [SEED0 + i for i in range(n)]))
    import torch
    from ldso_amd import binding
    ts = torch.cuda.Stream(); torch.cuda.set_stream(ts)
    F = made[0][0].F
    mid = F // 2
    hmap = np.array([f if f < mid else (-1 if f == mid else f - 1) for f in range(F)], np.int32)          # the middle host leaves, the ones behind it shift
    solo, grouped = [], []
    for w, j in made:
        for lst in (solo, grouped):
            t = binding.Tracer(w.w, w.h, len(j["cand"]))
            t.set_stream(ts.cuda_stream)
            lst.append(t)
    grp = binding.TracerGroup(grouped)
    L = grp.L

    def reload(trs):
        for t, (_, j) in zip(trs, made):
            t.set_points(j["cand"]); t.set_point_types(j["my_type"])

    left_solo = [C.c_int() for _ in range(n)]
    left_group = np.zeros(n, np.int32)
    nh = np.full(n, F, np.int32)
    PM = (C.c_void_p * n)(*[hmap.ctypes.data] * n)

    def sequential():
        for i, t in enumerate(solo):
            rc = L.ldso_trace_compact(t.h, None, C.c_int(F), binding._p(hmap), C.byref(left_solo[i]))
            if rc:
                return rc
        return 0

    t_solo, t_group = [], []
    for _ in range(a.warmup + a.reps):
        reload(solo); reload(grouped)
        t_solo.append(timed(sequential))
        t_group.append(timed(lambda: L.ldso_trace_group_compact(grp.h, None, None, binding._p(nh), PM, binding._p(left_group))))
    for i in range(n):
        solo[i].n = left_solo[i].value; grouped[i].n = int(left_group[i])
        same = solo[i].n == grouped[i].n and solo[i].get_points().tobytes() == grouped[i].get_points().tobytes() and solo[i].get_point_types().tobytes() == grouped[i].get_point_types().tobytes()
        assert same and 0 < solo[i].n < len(made[i][1]["cand"]), "the legs disagree: nothing to time"
    out = dict(step="trace_group_compact", n=n, reps=a.reps, records_per_tracer=len(made[0][1]["cand"]), left_per_tracer=int(np.mean(left_group)),
               sequential=stats(t_solo[a.warmup:]), grouped=stats(t_group[a.warmup:]))
    print(json.dumps(out), flush=True)
    grp.close()
    for t in solo + grouped:
        t.close()


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
