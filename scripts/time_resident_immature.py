"""The immature set resident on the device, timed on an MI355X at C3 with 7200 traced candidates (the state of scripts/time_activate_select.py):
  (a) selection + activation: ldso_ba_select_activate_points with explicit host arrays (7200 records, their types and ~1700 seeds go up) against
      ldso_ba_select_activate_tracer (candidates where the tracer holds them, seeds from the resident window, the compaction by the decisions included)
  (b) the drop-in's GpuBackend::traceNewCoarse with residentImmature off (flatten, upload, trace, download, write back) against on (poses and trace only)
The two legs of a step alternate call by call; the median of `--reps` calls after `--warmup` is reported with the 10th / 90th percentile, one JSON line per step.
Every call ends in a stream synchronisation, so the host clock around it is the call's time.  Without arguments the two steps run one after the other, each as a
child process of its own under `timeout`; the second does not start when the first failed.
    python scripts/time_resident_immature.py [--reps 50] [--warmup 5] [--min-dist 1.0] [--step a|b]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
STEP_TIMEOUT_S = {"a": 420, "b": 420}
PER_FRAME = 1200          # x 6 host key frames of C3 = 7200 candidates


def stats(t):
    t = np.asarray(t) * 1e6
    return dict(median_us=round(float(np.median(t)), 1), p10_us=round(float(np.percentile(t, 10)), 1), p90_us=round(float(np.percentile(t, 90)), 1))


def timed(call):
    t0 = time.perf_counter()
    out = call()
    return time.perf_counter() - t0, out


def step_a(a):
    from ldso_amd import binding
    import activation_select_common as asc
    win, (r,), _ = asc.make_state("C3", per_frame=PER_FRAME)
    g = asc.gather(r)
    n = len(g["cand"])
    args = (g["seeds"], g["cand"], g["my_type"], g["KRKi"], g["Kt"], g["flagged"])
    ba = binding.BA.from_window(win)
    tr = binding.Tracer(win.w, win.h, n)
    t_exp, t_res = [], []
    for i in range(a.warmup + a.reps):
        tr.set_points(g["cand"]); tr.set_point_types(g["my_type"])          # the state the frames before the key frame left: not part of the call
        dt, (dec, sel, out) = timed(lambda: ba.select_activate_points(*args, a.min_dist))
        t_exp.append(dt)
        dt, (dec2, sel2, out2) = timed(lambda: ba.select_activate_tracer(tr, g["KRKi"], g["Kt"], g["flagged"], a.min_dist, compact=True))
        t_res.append(dt)
        assert np.array_equal(dec, dec2) and np.array_equal(sel, sel2) and out.tobytes() == out2.tobytes() and tr.n == int((dec == 0).sum()), "the legs disagree: nothing to time"
    print(json.dumps(dict(step="select_activate", currentMinActDist=a.min_dist, seeds=len(g["seeds"]), candidates=n, selected=len(sel), left_in_tracer=tr.n, reps=a.reps,
                          explicit_arrays=stats(t_exp[a.warmup:]), from_tracer_with_compaction=stats(t_res[a.warmup:]))), flush=True)
    ba.close(); tr.close(); r.close()


def step_b(a):
    import ctypes as C
    from oracle import pyref as pr
    import activation_select_common as asc
    win, (r_off, r_on), pts = asc.make_state("C3", per_frame=PER_FRAME, n_graphs=2)
    A_off = pr.GpuAdapter(max_frames=win.F + 1, max_points=win.P + 16)
    A_on = pr.GpuAdapter(max_frames=win.F + 1, max_points=win.P + 16)
    assert pr.adapter_lib().adp_set_resident_immature(A_on.h, C.c_int(1)) == 0
    t_off, t_on = [], []
    for i in range(a.warmup + a.reps):
        fidx = win.F + (i & 1)
        T = win.truth["w2c"][fidx]; aa, bb = float(win.truth["aff_a"][fidx]), float(win.truth["aff_b"][fidx])
        fh_off = r_off.fs_new_frame(win.images[fidx][0], T, aa, bb); fh_on = r_on.fs_new_frame(win.images[fidx][0], T, aa, bb)      # a new frame per call, as in a sequence
        dt, c_off = timed(lambda: A_off.trace_new_coarse(r_off, fh_off))
        t_off.append(dt)
        dt, c_on = timed(lambda: A_on.trace_new_coarse(r_on, fh_on))
        t_on.append(dt)
        assert np.array_equal(c_off, c_on), "the legs disagree: nothing to time"
    cnt = np.zeros(3, np.int32)
    pr.adapter_lib().adp_immature_reconcile_counts(A_on.h, cnt.ctypes.data_as(C.c_void_p))
    assert pr.adapter_lib().adp_sync_immature(A_on.h, r_on.fs_handle()) == 0
    assert r_on.fs_get_immature().tobytes() == r_off.fs_get_immature().tobytes(), "the legs disagree after the run"
    print(json.dumps(dict(step="adapter_trace_new_coarse", immature_points=len(pts), reps=a.reps, reconcile_unchanged_compacted_full=[int(x) for x in cnt],
                          resident_off=stats(t_off[a.warmup:]), resident_on=stats(t_on[a.warmup:]))), flush=True)
    A_off.close(); A_on.close(); r_off.close(); r_on.close()
    r_off.L.ref_fs_release_new_frames()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50); ap.add_argument("--warmup", type=int, default=5); ap.add_argument("--min-dist", type=float, default=1.0)
    ap.add_argument("--step", choices=("a", "b"))
    a = ap.parse_args()
    if a.step:
        {"a": step_a, "b": step_b}[a.step](a)
        return 0
    for s in ("a", "b"):
        rc = subprocess.run(["timeout", "-k", "10", str(STEP_TIMEOUT_S[s]), sys.executable, os.path.abspath(__file__), "--step", s, "--reps", str(a.reps), "--warmup", str(a.warmup),
                             "--min-dist", str(a.min_dist)]).returncode
        if rc != 0:
            print(f"step {s} ended with status {rc}: stopping", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
