"""What activatePointsMT costs for a batch of windows, timed on an MI355X at B = 8 and B = 32 different C3 windows (7 key frames x 2000 points, 640 x 480, seeds
20260925 + i), each with about 7200 traced candidates of its own (1200 per key frame but the newest; tests/batch_activate_common.py):
  (a) B sequential ldso_ba_select_activate_points calls (one per handle: upload, k_act_select, k_activate on the selected list, download and a wait each) against
      ONE ldso_ba_batch_select_activate_points, at currentMinActDist 1 and 4;
  (b) the selection alone: B sequential ldso_ba_select_candidates against ONE ldso_ba_batch_select_candidates - with (a) the split of the fused call into its two kernels;
  (c) B sequential ldso_ba_activate_points calls against ONE ldso_ba_batch_activate_points, about 2300 candidates per window.
The two legs of a step alternate call by call on the SAME handles (the members of the batch), through the C entries with buffers allocated once; the median of
`--reps` calls after `--warmup` is reported with the 10th / 90th percentile, one JSON line per batch size.  Every call ends in a stream synchronisation, so the host
clock around it is the call's time.  After the clock has stopped the legs are compared once: decisions, selected lists and records byte for byte.  Nothing is
asserted about time.  Each batch size runs as a child process of its own under `timeout`; the second does not start when the first failed.
    python scripts/time_batch_activate.py [--reps 50] [--warmup 5] [--batch 8|32]"""
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
PER_FRAME, PLAIN = 1200, 2300


def stats(t):
    t = np.asarray(t) * 1e6
    return dict(median_us=round(float(np.median(t)), 1), p10_us=round(float(np.percentile(t, 10)), 1), p90_us=round(float(np.percentile(t, 90)), 1))


def timed(call):
    t0 = time.perf_counter()
    rc = call()
    dt = time.perf_counter() - t0
    assert rc == 0, rc
    return dt


def make_c3(seed):
    from ldso_amd import synth
    import batch_activate_common as bac
    win = synth.make_config("C3", seed=seed)
    return win, bac.make_job(win, PER_FRAME, seed=seed % 1000)


def run(a):
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
    out = dict(step="batch_activate", B=B, window="C3 %d KF x %d pt" % (made[0][0].F, made[0][0].P), reps=a.reps, candidates_per_window=len(made[0][1]["cand"]),
               seeds_per_window=len(made[0][1]["seeds"]))

    for dist in (1.0, 4.0):
        jobs = [bac.with_distance(j, dist) for _, j in made]
        for fused in (True, False):
            J, keep = b._jobs(jobs, fused)
            solo = [(np.zeros(len(j["cand"]), np.int32), np.zeros(len(j["cand"]), np.int32), C.c_int(), np.zeros(len(j["cand"]) if fused else 0, synth.ACTIVATION_DTYPE)) for j in jobs]
            sargs = [hs[i]._select_args(*bac.solo_args(j), dist, 3.0) for i, j in enumerate(jobs)]
            tail = (C.c_int(1), C.c_float(100.0), C.c_int(3))

            def sequential():
                for i, g in enumerate(hs):
                    dec, sel, ns, rec = solo[i]
                    if fused:
                        rc = L.ldso_ba_select_activate_points(g.h, *sargs[i][1], *tail, binding._p(dec), binding._p(sel), C.byref(ns), binding._p(rec))
                    else:
                        rc = L.ldso_ba_select_candidates(g.h, *sargs[i][1], binding._p(dec), binding._p(sel), C.byref(ns))
                    if rc:
                        return rc
                return 0

            def batched():
                if fused:
                    return L.ldso_ba_batch_select_activate_points(b.h, J, C.c_float(3.0), *tail)
                return L.ldso_ba_batch_select_candidates(b.h, J, C.c_float(3.0))

            t_solo, t_batch = [], []
            for _ in range(a.warmup + a.reps):
                t_solo.append(timed(sequential))
                t_batch.append(timed(batched))
            nsel = []
            for i in range(B):
                dec, sel, ns, rec = solo[i]
                k = keep[i]
                same = J[i].n_selected == ns.value and k[6].tobytes() == dec.tobytes() and k[7][:ns.value].tobytes() == sel[:ns.value].tobytes()
                same = same and (not fused or k[8][:ns.value].tobytes() == rec[:ns.value].tobytes())
                assert same and ns.value > 0, "the legs disagree: nothing to time"
                nsel.append(ns.value)
            out["%s_dist_%g" % ("select_activate" if fused else "select", dist)] = dict(sequential=stats(t_solo[a.warmup:]), batched=stats(t_batch[a.warmup:]),
                                                                                        selected_per_window=int(np.mean(nsel)))

    pts = [np.ascontiguousarray(j["cand"][::3][:PLAIN]) for _, j in made]
    rs = [np.zeros(len(p), synth.ACTIVATION_DTYPE) for p in pts]
    rb = [np.zeros(len(p), synth.ACTIVATION_DTYPE) for p in pts]
    cnt = np.array([len(p) for p in pts], np.int32)
    PP = (C.c_void_p * B)(*[p.ctypes.data for p in pts]); PO = (C.c_void_p * B)(*[r.ctypes.data for r in rb])
    tail = (C.c_int(1), C.c_float(100.0), C.c_int(3))

    def sequential_plain():
        for i, g in enumerate(hs):
            rc = L.ldso_ba_activate_points(g.h, C.c_int(len(pts[i])), binding._p(pts[i]), *tail, binding._p(rs[i]))
            if rc:
                return rc
        return 0

    t_solo, t_batch = [], []
    for _ in range(a.warmup + a.reps):
        t_solo.append(timed(sequential_plain))
        t_batch.append(timed(lambda: L.ldso_ba_batch_activate_points(b.h, binding._p(cnt), PP, *tail, PO)))
    assert all(x.tobytes() == y.tobytes() and 0 < x["ok"].mean() < 1 for x, y in zip(rs, rb)), "the legs disagree: nothing to time"
    out["activate_points"] = dict(sequential=stats(t_solo[a.warmup:]), batched=stats(t_batch[a.warmup:]), candidates_per_window=int(cnt[0]))
    print(json.dumps(out), flush=True)
    b.close()
    for g in hs:
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
