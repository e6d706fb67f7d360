#!/usr/bin/env python3
"""tests/golden/reduce_tiles_parent.npz: per case of tests/test_reduce_tiles_gpu.py what the library that is loaded gives - run it on an MI355X with the
library of the commit BEFORE the Schur tile workgroups loaded their matrix-core operands straight from G (the kernel that staged them in an LDS slab):
    LDSO_HIP_LIB=<that build of libldso_hip.so> python scripts/golden/make_reduce_tiles_parent.py
Per case: <name>__H, <name>__b (lower triangle of HFinal and bFinal of the first of 20 repetitions), <name>__spread (the largest entrywise difference among
the 20: the arrival order of the fp64 atomics), <name>__oracle_dev_H, <name>__oracle_dev_b (the largest deviation of any repetition from the oracle's system,
in the units of the test's oracle_deviation)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_reduce_tiles_gpu as t          # noqa: E402
from ldso_amd import binding          # noqa: E402

REPS = 20
print("library", binding.lib_path(), flush=True)
out = {}
for name, F, P, splits, shard in t.CASES:
    win, runs, whole = t.run_case(F, P, splits, shard, REPS)
    Hs, bs = np.stack([r[0] for r in runs]), np.stack([r[1] for r in runs])
    assert np.isfinite(Hs).all() and np.isfinite(bs).all(), name
    spread = max(float((Hs.max(0) - Hs.min(0)).max()), float((bs.max(0) - bs.min(0)).max()))
    Ho, bo = t.oracle_system(win)
    devs = [t.oracle_deviation(h, b, Ho, bo) for h, b in whole]
    dev_h, dev_b = max(d[0] for d in devs), max(d[1] for d in devs)
    print(f"{name}: n {Hs.shape[1]} spread {spread:.3e} (largest |H| {np.abs(Hs[0]).max():.3e}), against the oracle H {dev_h:.3e} b {dev_b:.3e}", flush=True)
    out.update({name + "__H": Hs[0], name + "__b": bs[0], name + "__spread": np.float64(spread), name + "__oracle_dev_H": np.float64(dev_h),
                name + "__oracle_dev_b": np.float64(dev_b)})
dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "reduce_tiles_parent.npz")
np.savez_compressed(dst, **out)
print("wrote", dst, os.path.getsize(dst), "bytes")
