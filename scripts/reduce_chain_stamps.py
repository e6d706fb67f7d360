#!/usr/bin/env python3
"""The reduce side of k_reduce_solve in front of the control step, from the device stamps (a -DLDSO_STAMPS build of the unit that holds the kernel:
scripts/build_variant.sh stamps ba_solve.hip -DLDSO_STAMPS, then LDSO_HIP_LIB=ldso_amd/libldso_hip_stamps.so):

    python scripts/reduce_chain_stamps.py [config = C3] [K-splits per Schur tile = the library's default] [iterations = 24]

Per forced iteration, microseconds (100 MHz wall clock):
  * what scripts/r4/last_reduce.py prints: which reduce workgroup signalled last (its index in reduce_body's numbering pairs | tiles | extras, and its kind),
    when it signalled and when it had started, when the control workgroup's wait was over, its loads done, its factorisation done - all after the START OF
    THE CONTROL WORKGROUP;
  * tile workgroup 0 (RSTAMP 25 / 26 / 27: operands there, tile computed, atomics issued), pair workgroup 0 (RSTAMP 23 / 20 / 21: partials loaded, slice sums
    in LDS, atomics issued) and the extras workgroup (RSTAMP 28) - after THEIR OWN start.
Then the medians and how often each kind of workgroup was the last signaller."""
import collections
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ldso_amd import synth, binding          # noqa: E402

cfg = sys.argv[1] if len(sys.argv) > 1 else "C3"
splits = int(sys.argv[2]) if len(sys.argv) > 2 else 0
iters = int(sys.argv[3]) if len(sys.argv) > 3 else 24
win = synth.add_synthetic_prior(synth.make_config(cfg))
g = binding.BA.from_window(win)
if splits:
    g.set_reduce_splits(splits)
ks = splits or 8
g.collect_active(); g.linearize_all(False); g.apply_res()
g.enqueue_gn(0, 10); g.sync()
F = win.F
n_pair = F * F * (2 if int(np.sum(win.residuals["is_linearized"])) > 0 else 1)
n_t = (8 * ((F + 7) // 8 * 8) + 8 + 15) // 16
n_tile = ks * n_t * (n_t + 1) // 2


def kind(bid):
    return "pair" if bid < n_pair else "tile" if bid < n_pair + n_tile else "extras"


print(f"{cfg}: F {F} P {win.P}, {ks} K-splits per tile: {n_pair} pair, {n_tile} tile workgroups, 1 extras; library {os.path.basename(binding.lib_path())}")
print("last bid kind | signals at, had started at, wait over, loads done, factor done (after the control workgroup's start) | tile 0: operands, tile, atomics | "
      "pair 0: partials, slice sums, atomics | extras done (after their own start)")
rows, kinds = [], collections.Counter()
for rep in range(iters):
    g.enqueue_gn(2, 1); g.sync()
    buf = np.zeros(64)
    g.L.ldso_ba_get_energy_log(g.h, buf.ctypes.data_as(C.c_void_p), C.c_int(64))
    t0 = buf[39]
    r = [(buf[29] - t0) / 100, (buf[31] - t0) / 100, (buf[48] - t0) / 100, (buf[41] - t0) / 100, (buf[42] - t0) / 100,
         buf[25] / 100, buf[26] / 100, buf[27] / 100, buf[23] / 100, buf[20] / 100, buf[21] / 100, buf[28] / 100]
    bid = int(buf[30])
    kinds[kind(bid)] += 1
    rows.append(r)
    print(f"{bid:4d} {kind(bid):6s} | " + " ".join(f"{v:6.2f}" for v in r[:5]) + " | " + " ".join(f"{v:5.2f}" for v in r[5:8]) + " | " +
          " ".join(f"{v:5.2f}" for v in r[8:11]) + f" | {r[11]:5.2f}")
med = np.median(np.array(rows), axis=0)
print("median      | " + " ".join(f"{v:6.2f}" for v in med[:5]) + " | " + " ".join(f"{v:5.2f}" for v in med[5:8]) + " | " + " ".join(f"{v:5.2f}" for v in med[8:11]) + f" | {med[11]:5.2f}")
print("last signaller:", ", ".join(f"{k} {v}/{iters}" for k, v in kinds.most_common()))
