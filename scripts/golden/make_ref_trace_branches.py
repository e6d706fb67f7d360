"""Record tests/golden/ref_trace_branches.npz: the reference's own ImmaturePoint::traceOn (oracle/_ref/libldso_ref.so, `make -C oracle ref`, through
pyref.trace_on) on the calls of tests/trace_branch_common.py that are marked `golden` - the 85-step call, the 99-step call and the finite-interval call, each with
its second trace.  Records and counts only: the scene is regenerated from its seed.  Run from the repo root: python scripts/golden/make_ref_trace_branches.py"""
import os
import sys
sys.path.insert(0, '.'); sys.path.insert(0, 'tests')
import numpy as np
import trace_branch_common as tb
from oracle import pyref as pr

out = {}
for c in tb.scene()["calls"]:
    if not c["golden"]:
        continue
    for t, (counts, records) in enumerate(tb.run(c, pr.trace_on)):
        out[f"{c['name']}_counts{t}"] = counts
        out[f"{c['name']}_records{t}"] = np.frombuffer(records.tobytes(), dtype=np.uint8)
path = os.path.join('tests', 'golden', 'ref_trace_branches.npz')
np.savez_compressed(path, **out)
print('written', path, os.path.getsize(path), 'bytes', sorted(out))
