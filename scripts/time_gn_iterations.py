#!/usr/bin/env python3
"""Microseconds per forced Gauss-Newton iteration of one window (ldso_ba_enqueue_gn, the graph replay bench.py times), by K-splits per Schur tile:

    [LDSO_HIP_LIB=<variant>] python scripts/time_gn_iterations.py [config = C3] [K-splits, comma separated = 8] [rounds = 6] [iterations per round = 5000]

One handle per K-split value (ldso_ba_set_reduce_splits), the values alternating round by round; a round is iterations / 100 replays of a captured sequence of
100 iterations between two host clock readings, the second behind a stream synchronisation.  Prints every round and the range per value.  To compare builds of
the library, run one process per build and round, alternating (LDSO_HIP_LIB), with rounds = 1."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ldso_amd import synth, binding          # noqa: E402

cfg = sys.argv[1] if len(sys.argv) > 1 else "C3"
splits = [int(s) for s in (sys.argv[2] if len(sys.argv) > 2 else "8").split(",")]
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 6
iters = int(sys.argv[4]) if len(sys.argv) > 4 else 5000
SEQ = 100
win = synth.add_synthetic_prior(synth.make_config(cfg))
handles = {}
for ks in splits:
    g = binding.BA.from_window(win)
    g.set_reduce_splits(ks)
    g.collect_active(); g.linearize_all(False); g.apply_res()
    g.enqueue_gn(0, 2)
    for _ in range(3):
        g.enqueue_gn(2, SEQ)          # the first call captures, the others replay
    g.sync()
    handles[ks] = g
us = {ks: [] for ks in splits}
for r in range(rounds):
    for ks in splits:
        g = handles[ks]
        g.sync()
        t0 = time.perf_counter()
        for _ in range(iters // SEQ):
            g.enqueue_gn(2, SEQ)
        g.sync()
        us[ks].append((time.perf_counter() - t0) * 1e6 / (iters // SEQ * SEQ))
for ks in splits:
    g = handles[ks]
    g.get_arrival_words()          # raises on the non-finite status
    print(f"{cfg} {os.path.basename(binding.lib_path())} K-splits {ks:2d}: us per iteration, {rounds} alternating rounds of {iters}: " + " ".join(f"{v:.2f}" for v in us[ks]) +
          f"   range {min(us[ks]):.2f}-{max(us[ks]):.2f}")
