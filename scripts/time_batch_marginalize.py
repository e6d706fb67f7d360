"""What the key frame costs behind a batched optimize(), timed on an MI355X at B = 8 and B = 32 different C3 windows (7 key frames x 2000 points, 640 x 480: the
windows of bench.py's batched line, seeds 20260925 + i, each with the synthetic prior), every seventh point flagged:
  (a) B sequential ldso_ba_marginalize_points calls (one per handle: four launches, two copies back and a wait each) against ONE ldso_ba_batch_marginalize_points
  (b) B sequential ldso_ba_marginalize_frame calls (frame 0) against ONE ldso_ba_batch_marginalize_frame
  (c) for scale: one ldso_ba_batch_optimize(6, forced) of the same batch
The two legs of a step alternate call by call on the SAME handles (the members of the batch; the solo entries work on them as on any handle), through the C entries
with buffers allocated once; the median of `--reps` calls after `--warmup` is reported with the 10th / 90th percentile, one JSON line per batch size.  Every call
ends in a stream synchronisation, so the host clock around it is the call's time.  The first round checks that the legs agree (the points: each leg adds onto the
prior the other left, so the increments are compared; the frames: byte for byte).  Nothing is asserted about time.  Each batch size runs as a child process of
its own under `timeout`; the second does not start when the first failed.
    python scripts/time_batch_marginalize.py [--reps 50] [--warmup 5] [--batch 8|32]"""
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


def make_c3(seed):
    from ldso_amd import synth
    return synth.add_synthetic_prior(synth.make_config("C3", seed=seed))


def run(a):
    B = a.batch
    # the windows first, on a few cores, before anything opens the device
    from concurrent.futures import ProcessPoolExecutor
    with ProcessPoolExecutor(max_workers=min(8, B)) as ex:
        wins = list(ex.map(make_c3, [SEED0 + i for i in range(B)]))
    import torch
    from ldso_amd import binding
    ts = torch.cuda.Stream(); torch.cuda.set_stream(ts)
    hs = []
    for w in wins:
        g = binding.BA.from_window(w, stream=ts.cuda_stream)
        g.collect_active(); g.linearize_all(False); g.apply_res()
        hs.append(g)
    b = binding.BABatch(hs)
    L = b.L
    n, nd = 8 * wins[0].F + 4, 8 * (wins[0].F - 1) + 4
    flags = [np.ascontiguousarray(np.arange(w.P) % 7 == 0, np.int32) for w in wins]
    PF = (C.c_void_p * B)(*[f.ctypes.data for f in flags])
    idx = np.zeros(B, np.int32)

    def buffers(k):
        H, v = [np.zeros((k, k)) for _ in range(B)], [np.zeros(k) for _ in range(B)]
        return H, v, (C.c_void_p * B)(*[x.ctypes.data for x in H]), (C.c_void_p * B)(*[x.ctypes.data for x in v])

    def solo_points(H, v):
        for i, g in enumerate(hs):
            rc = L.ldso_ba_marginalize_points(g.h, binding._p(flags[i]), binding._p(H[i]), binding._p(v[i]))
            if rc:
                return rc
        return 0

    def solo_frames(H, v):
        for i, g in enumerate(hs):
            rc = L.ldso_ba_marginalize_frame(g.h, C.c_int(0), binding._p(H[i]), binding._p(v[i]))
            if rc:
                return rc
        return 0

    Hs, vs, _, _ = buffers(n)
    Hb, vb, PHb, Pvb = buffers(n)
    t_solo, t_batch = [], []
    for it in range(a.warmup + a.reps):
        prev = [x.copy() for x in Hb] if it else [w.HM.copy() for w in wins]
        t_solo.append(timed(lambda: solo_points(Hs, vs)))
        t_batch.append(timed(lambda: L.ldso_ba_batch_marginalize_points(b.h, PF, PHb, Pvb)))
        if it == 0:          # the same increment from both legs (the prior they add onto differs by one increment: not bit for bit)
            for i in range(B):
                d1, d2 = Hs[i] - prev[i], Hb[i] - Hs[i]
                assert np.abs(d1).max() > 0 and np.abs(d2 - d1).max() <= 1e-9 * np.abs(d1).max(), "the legs disagree: nothing to time"
    points = dict(sequential=stats(t_solo[a.warmup:]), batched=stats(t_batch[a.warmup:]))

    Fs, fs, _, _ = buffers(nd)
    Fb, fb, PFb, Pfb = buffers(nd)
    t_solo, t_batch = [], []
    for it in range(a.warmup + a.reps):
        t_solo.append(timed(lambda: solo_frames(Fs, fs)))
        t_batch.append(timed(lambda: L.ldso_ba_batch_marginalize_frame(b.h, binding._p(idx), PFb, Pfb)))
        if it == 0:
            assert all(Fs[i].tobytes() == Fb[i].tobytes() and fs[i].tobytes() == fb[i].tobytes() and np.abs(Fs[i]).max() > 0 for i in range(B)), "the legs disagree: nothing to time"
    frames = dict(sequential=stats(t_solo[a.warmup:]), batched=stats(t_batch[a.warmup:]))

    rm, its, st = np.zeros(B, np.float32), np.zeros(B, np.int32), np.zeros(B, np.int32)
    def optimize():          # a non-finite verdict (LDSO_E_NONFINITE = -3) is a result, reported below; the call has done the same work
        rc = L.ldso_ba_batch_optimize(b.h, C.c_int(6), C.c_int(1), binding._p(rm), binding._p(its), binding._p(st))
        return 0 if rc == -3 else rc

    t_opt = [timed(optimize) for _ in range(a.warmup + a.reps)]
    print(json.dumps(dict(step="batch_marginalize", B=B, window="C3 %d KF x %d pt" % (wins[0].F, wins[0].P), flagged_per_window=int(flags[0].sum()), reps=a.reps,
                          marginalize_points=points, marginalize_frame=frames, batch_optimize_6_forced=stats(t_opt[a.warmup:]), windows_finite=int((st == 0).sum()))), flush=True)
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
