"""What the key-frame hand-over of the resident immature sets costs for a batch of windows, timed on an MI355X at B = 8 and B = 32 different C3 windows (7 key frames
x 2000 points, 640 x 480, seeds 20260925 + i), each with a tracer that holds about 7200 traced candidates of its own (1200 per key frame but the newest;
tests/batch_activate_common.py), at currentMinActDist 1 and 4.  Three legs, alternating call by call on the SAME handles (the members of the batch):
  (a) B sequential ldso_ba_select_activate_tracer calls with the compaction (one per handle: an upload, five launches, a download and a wait each);
  (b) ONE ldso_ba_batch_select_activate_points on the same jobs with explicit arrays (every candidate and seed crosses PCIe; no compaction);
  (c) ONE ldso_ba_batch_select_activate_tracers with the compaction of every window (one upload, four launches, one download, one wait).
(a) and (c) each have a tracer per window of their own; both are loaded again with the full candidate set before every call, outside the clock, so every call does
the same work.  Through the C entries with buffers allocated once; the median of `--reps` calls after `--warmup` is reported with the 10th / 90th percentile, one JSON
line per batch size.  Every call ends in a stream synchronisation, so the host clock around it is the call's time.  After the clock has stopped the legs are compared
once: decisions, selected lists and records byte for byte, the two sets of tracers byte for byte.  Nothing is asserted about time.  Each batch size runs as a child
process of its own under `timeout`; the second does not start when the first failed.
    python scripts/time_batch_activate_tracer.py [--reps 50] [--warmup 5] [--batch 8|32]"""
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
    B = a.batch
    # the windows and their candidates first, on a few cores, before anything opens the device
    from concurrent.futures import ProcessPoolExecutor
    with ProcessPoolExecutor(max_workers=min(8, B)) as ex:
        made = list(ex.map(make_c3, [SEED0 + i for i in range(B)]))
    import torch
    from ldso_amd import binding, synth
    import batch_activate_common as bac
    ts = torch.cuda.Stream(); torch.cuda.set_stream(ts)
    hs = [binding.BA.from_window(w, stream=ts.cuda_stream) for w, _ in made]
    b = binding.BABatch(hs)
    L = b.L
    n = [len(j["cand"]) for _, j in made]
    out = dict(step="batch_activate_tracer", B=B, window="C3 %d KF x %d pt" % (made[0][0].F, made[0][0].P), reps=a.reps, candidates_per_window=n[0],
               window_points_per_window=made[0][0].P)
    tr_solo = [binding.Tracer(w.w, w.h, len(j["cand"])) for w, j in made]
    tr_batch = [binding.Tracer(w.w, w.h, len(j["cand"])) for w, j in made]

    def reload(trs):
        for t, (_, j) in zip(trs, made):
            t.set_points(j["cand"]); t.set_point_types(j["my_type"])

    tail = (C.c_int(1), C.c_float(100.0), C.c_int(3))
    for dist in (1.0, 4.0):
        jobs = [bac.with_distance(j, dist) for _, j in made]
        J, keep = b._jobs(jobs, True)
        reload(tr_batch)
        JT, keepT = b._tracer_jobs([dict(tracer=t, KRKi=j["KRKi"], Kt=j["Kt"], flagged=j["flagged"], min_act_dist=dist, compact=True) for t, j in zip(tr_batch, jobs)])
        solo = [(np.zeros(k, np.int32), np.zeros(k, np.int32), C.c_int(), np.zeros(k, synth.ACTIVATION_DTYPE), C.c_int()) for k in n]
        pose = [(np.ascontiguousarray(j["KRKi"], np.float32), np.ascontiguousarray(j["Kt"], np.float32), np.ascontiguousarray(j["flagged"], np.int32)) for j in jobs]

        def sequential():
            for i, g in enumerate(hs):
                dec, sel, ns, rec, left = solo[i]
                K1, K2, fl = pose[i]
                rc = L.ldso_ba_select_activate_tracer(g.h, tr_solo[i].h, C.c_int(len(fl)), binding._p(K1), binding._p(K2), binding._p(fl), C.c_float(dist), C.c_float(3.0), *tail,
                                                      C.c_int(1), binding._p(dec), binding._p(sel), C.byref(ns), binding._p(rec), C.byref(left))
                if rc:
                    return rc
            return 0

        t_solo, t_arrays, t_tracers = [], [], []
        for _ in range(a.warmup + a.reps):
            reload(tr_solo); reload(tr_batch)
            t_solo.append(timed(sequential))
            t_arrays.append(timed(lambda: L.ldso_ba_batch_select_activate_points(b.h, J, C.c_float(3.0), *tail)))
            t_tracers.append(timed(lambda: L.ldso_ba_batch_select_activate_tracers(b.h, JT, C.c_float(3.0), *tail)))
        nsel, nleft = [], []
        for i in range(B):
            dec, sel, ns, rec, left = solo[i]
            for got_ns, got in ((J[i].n_selected, keep[i][6:9]), (JT[i].n_selected, keepT[i][4:7])):
                same = got_ns == ns.value and got[0].tobytes() == dec.tobytes() and got[1][:ns.value].tobytes() == sel[:ns.value].tobytes() and got[2][:ns.value].tobytes() == rec[:ns.value].tobytes()
                assert same and ns.value > 0, "the legs disagree: nothing to time"
            tr_solo[i].n = left.value; tr_batch[i].n = JT[i].n_left
            assert left.value == JT[i].n_left == int((dec == synth.ACT_KEEP).sum()) and tr_solo[i].get_points().tobytes() == tr_batch[i].get_points().tobytes() \
                and tr_solo[i].get_point_types().tobytes() == tr_batch[i].get_point_types().tobytes(), "the compacted tracers disagree: nothing to time"
            nsel.append(ns.value); nleft.append(left.value)
        out["dist_%g" % dist] = dict(sequential_tracer=stats(t_solo[a.warmup:]), batched_arrays=stats(t_arrays[a.warmup:]), batched_tracers=stats(t_tracers[a.warmup:]),
                                     selected_per_window=int(np.mean(nsel)), left_per_window=int(np.mean(nleft)))
    print(json.dumps(out), flush=True)
    b.close()
    for g in hs + tr_solo + tr_batch:
        g.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50); ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, choices=(8, 32))
    a = ap.parse_args()
    if a.batch:
        run(a)
        return 0
    for B in (8, 32):
        rc = subprocess.run(["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--batch", str(B), "--reps", str(a.reps), "--warmup", str(a.warmup)]).returncode
        if rc != 0:
            print(f"B = {B} ended with status {rc}: stopping", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
