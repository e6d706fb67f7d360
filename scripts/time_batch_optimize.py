"""Wall time of ONE BABatch.optimize(6) (ldso_ba_batch_optimize) against B sequential BA.optimize(6) calls on twin handles, for B different C3 windows
(built as bench.py's batched line builds them).  Every repetition starts from the freshly uploaded windows (the upload and the forming of the batch are
outside the clock); median of the repetitions after one warm-up.  Prints one JSON line.  Run on the GPU box:
    python scripts/time_batch_optimize.py [--B 8 32] [--reps 7] [--iters 6]"""
import argparse
import json
import sys
import time

import numpy as np

sys.path.insert(0, '.')
import torch
from ldso_amd import synth, binding

ap = argparse.ArgumentParser()
ap.add_argument("--B", type=int, nargs="+", default=[8, 32])
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--iters", type=int, default=6)
args = ap.parse_args()
assert args.reps >= 5

ts = torch.cuda.Stream(); torch.cuda.set_stream(ts)
st = ts.cuda_stream
wins, batch, twins = [], [], []
out = {"workload": "B different C3 windows (seeds 20260925 + i, synthetic prior), un-forced optimize(%d)" % args.iters}
for B in sorted(args.B):
    while len(wins) < B:
        w = synth.add_synthetic_prior(synth.make_config("C3", seed=20260925 + len(wins)) if wins else synth.make_config("C3"))
        wins.append(w)
        batch.append(binding.BA.from_window(w, stream=st)); twins.append(binding.BA.from_window(w, stream=st))
    tb, tq, its_b, its_q = [], [], None, None
    for rep in range(args.reps + 1):          # rep 0 warms up (code objects, LDS attributes, allocations)
        for g, w in zip(batch[:B] + twins[:B], wins[:B] + wins[:B]):
            g.load_window(w)
        bt = binding.BABatch(batch[:B])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rm_b, its_b, status = bt.optimize(args.iters)
        t1 = time.perf_counter()
        bt.close()
        assert not status.any(), status
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        res = [g.optimize(args.iters) for g in twins[:B]]
        t3 = time.perf_counter()
        its_q = [r[1] for r in res]
        if rep > 0:
            tb.append(t1 - t0); tq.append(t3 - t2)
    b_ms, q_ms = float(np.median(tb)) * 1e3, float(np.median(tq)) * 1e3
    out["B%d" % B] = {"batch_ms": round(b_ms, 4), "sequential_ms": round(q_ms, 4), "sequential_over_batch": round(q_ms / b_ms, 3),
                      "iterations_batch": [int(i) for i in its_b], "iterations_sequential": [int(i) for i in its_q],
                      "rmse_max_rel_diff": float(max(abs(a - r[0]) / r[0] for a, r in zip(rm_b, res))), "repetitions": args.reps}
print(json.dumps(out))
