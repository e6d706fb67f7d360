#!/usr/bin/env python3
"""The reduce side of k_reduce_solve in front of the control step, from the device stamps (a -DLDSO_STAMPS build of the unit that holds the kernel:
scripts/build_variant.sh stamps ba_solve.hip -DLDSO_STAMPS, then LDSO_HIP_LIB=ldso_amd/libldso_hip_stamps.so):

    python scripts/reduce_chain_stamps.py [config = C3] [K-splits per Schur tile = the library's default] [iterations = 24]

Per forced iteration, microseconds (100 MHz wall clock):
  * which reduce workgroup's arrival atomic returned last (its index in reduce_body's numbering pairs | tiles | extras, and its kind), when that was and when
    it had started, when the control workgroup's wait was over, its loads done, its factorisation done - all after the START OF THE CONTROL WORKGROUP;
  * tile workgroup 0 (RSTAMP 25 / 26 / 27: operands there, tile computed, atomics issued), pair workgroup 0 (RSTAMP 23 / 20 / 21: partials loaded, slice sums
    in LDS, atomics issued) and the extras workgroup (RSTAMP 28) - after THEIR OWN start;
  * the arrivals, from the record every reduce workgroup leaves (ldso_ba_get_reduce_stamps: started | data atomics acknowledged | arrival atomic returned):
    first and last "data acknowledged" (after the control workgroup's start) and their spread, the same for "arrived", the median gap between consecutive
    arrivals in nanoseconds (the clock ticks every 10 ns), and how long the last arrival came behind the last acknowledgement.
Then the medians and how often each kind of workgroup arrived last."""
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
total = n_pair + n_tile + 1


def kind(bid):
    return "pair" if bid < n_pair else "tile" if bid < n_pair + n_tile else "extras"


def bid_of(q):
    """dispatch index behind the control workgroups (tiles | pairs | extras) -> reduce_body's numbering (pairs | tiles | extras), as k_reduce_solve maps them"""
    return n_pair + q if q < n_tile else q - n_tile if q < n_tile + n_pair else q


def fmt(r):
    return (" ".join(f"{v:6.2f}" for v in r[:5]) + " | " + " ".join(f"{v:5.2f}" for v in r[5:8]) + " | " + " ".join(f"{v:5.2f}" for v in r[8:11]) + f" | {r[11]:5.2f} | " +
            " ".join(f"{v:5.2f}" for v in r[12:15]) + " | " + " ".join(f"{v:5.2f}" for v in r[15:18]) + f" | {r[18]:5.1f} | {r[19]:5.2f}")


print(f"{cfg}: F {F} P {win.P}, {ks} K-splits per tile: {n_pair} pair, {n_tile} tile workgroups, 1 extras; library {os.path.basename(binding.lib_path())}")
print("last bid kind | arrives at, had started at, wait over, loads done, factor done (after the control workgroup's start) | tile 0: operands, tile, atomics | "
      "pair 0: partials, slice sums, atomics | extras done (after their own start) | data acknowledged: first, last, spread | arrived: first, last, spread | "
      "median gap between arrivals, ns | last arrival behind last acknowledgement")
rows, kinds = [], collections.Counter()
for rep in range(iters):
    g.enqueue_gn(2, 1); g.sync()
    buf = np.zeros(64)
    g.L.ldso_ba_get_energy_log(g.h, buf.ctypes.data_as(C.c_void_p), C.c_int(64))
    rec = np.zeros(3 * total)
    got = g.L.ldso_ba_get_reduce_stamps(g.h, rec.ctypes.data_as(C.c_void_p), C.c_int(rec.size))
    assert got == rec.size, got
    t0 = buf[39]
    start, ack, arr = ((rec[k::3] - t0) / 100 for k in range(3))
    q_last = int(np.argmax(arr))
    bid = bid_of(q_last)
    gaps = np.diff(np.sort(arr)) * 1000
    r = [arr[q_last], start[q_last], (buf[48] - t0) / 100, (buf[41] - t0) / 100, (buf[42] - t0) / 100,
         buf[25] / 100, buf[26] / 100, buf[27] / 100, buf[23] / 100, buf[20] / 100, buf[21] / 100, buf[28] / 100,
         ack.min(), ack.max(), ack.max() - ack.min(), arr.min(), arr.max(), arr.max() - arr.min(), float(np.median(gaps)), arr.max() - ack.max()]
    kinds[kind(bid)] += 1
    rows.append(r)
    print(f"{bid:4d} {kind(bid):6s} | " + fmt(r))
print("median      | " + fmt(np.median(np.array(rows), axis=0)))
print("last to arrive:", ", ".join(f"{k} {v}/{iters}" for k, v in kinds.most_common()))
# the last iteration's arrivals one by one, in the order they returned: who, acknowledged, arrived (after the control workgroup's start)
order = np.argsort(arr)
print("last iteration, every 8th arrival in order (kind: acknowledged -> arrived): " +
      "  ".join(f"{kind(bid_of(int(q)))} {ack[q]:.2f}->{arr[q]:.2f}" for q in order[::8]))
