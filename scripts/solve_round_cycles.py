#!/usr/bin/env python3
"""Where the control workgroup of k_reduce_solve spends its time, as JSON (stamps build of the unit that holds k_reduce_solve: scripts/build_variant.sh stamps ba_solve.hip -DLDSO_STAMPS, then
LDSO_HIP_LIB=ldso_amd/libldso_hip_stamps.so python scripts/solve_round_cycles.py [config] [out.json]).  Medians over 12 launches of one iteration:
cycles per round of the 4-column LDL^T on wave 0 (solve_core's RCYC counters) and the split of the control step in us (100 MHz wall clock stamps)."""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ldso_amd import synth, binding          # noqa: E402

cfg = sys.argv[1] if len(sys.argv) > 1 else "C3"
win = synth.add_synthetic_prior(synth.make_config(cfg))
g = binding.BA.from_window(win)
g.collect_active(); g.linearize_all(False); g.apply_res()
g.enqueue_gn(0, 10); g.sync()
rounds = (win.F * 8 + 4 + 3) // 4
PH = ["panel_in_registers", "phase1_issued", "keeper_stores_and_operands", "matrix_cores_and_publish", "barrier"]
cyc, us = [], []
for rep in range(12):
    g.enqueue_gn(2, 1); g.sync()
    buf = np.zeros(64)
    g.L.ldso_ba_get_energy_log(g.h, buf.ctypes.data_as(C.c_void_p), C.c_int(64))
    t = lambda i: (buf[i] - buf[39]) / 100.0
    cyc.append([buf[53 + u] / rounds for u in range(5)])
    us.append([t(47), t(48) - t(47), t(41) - t(48), t(42) - t(41), t(43) - t(42), max(t(58), t(62), t(63)) - t(43)])
cyc, us = np.median(np.array(cyc), axis=0), np.median(np.array(us), axis=0)
res = {"config": cfg, "n": int(win.F * 8 + 4), "rounds": rounds, "library": os.path.basename(os.environ.get("LDSO_HIP_LIB", "libldso_hip.so")),
       "cycles_per_round_wave0": {k: round(float(v), 1) for k, v in zip(PH, cyc)}, "cycles_per_round_total": round(float(cyc.sum()), 1),
       "control_step_us": {k: round(float(v), 2) for k, v in zip(["staging_before_wait", "wait", "load_and_scale", "factorisation", "back_substitution", "tail_to_last_wave_at_barrier"], us)}}
print(json.dumps(res))
if len(sys.argv) > 2:
    json.dump(res, open(sys.argv[2], "w"), indent=1)
