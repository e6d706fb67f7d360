#!/usr/bin/env python3
"""tests/golden/solve64_parent.npz: the inputs of tests/test_solve64_operands_gpu.py and, per case, the x of the library that is loaded - run it on an MI355X with
the library of the commit BEFORE the register transpose of the matrix cores' operands (the kernel that transposed F and G through per-wave LDS copies):
    LDSO_HIP_LIB=<that build of libldso_hip.so> python scripts/golden/make_solve64_parent.py
Per case: <name>__H, <name>__b (the system), <name>__x (two runs of the library must agree to the bit: asserted), <name>__err_numpy (its relative error against
numpy's float64 solution of the same scaled system - the test allows the kernel under test 3 x that)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_solve64_operands_gpu as t          # noqa: E402

out = {}
for name, F, kind, iteration in t.CASES:
    H, b = t.make_system(name, F, kind)
    x, ref = t.run_case(F, H, b, iteration)
    x2, _ = t.run_case(F, H, b, iteration)
    assert np.array_equal(x, x2, equal_nan=True), (name, "two runs of the same library differ")
    assert np.isfinite(x).all(), name
    err = t.relerr(x, ref)
    print(name, "n", len(b), "iteration", iteration, "rel. error against numpy", err, "|x|", np.linalg.norm(x), flush=True)
    out.update({name + "__H": H, name + "__b": b, name + "__x": x, name + "__err_numpy": np.float64(err)})
dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "solve64_parent.npz")
np.savez_compressed(dst, **out)
print("wrote", dst, os.path.getsize(dst), "bytes")
