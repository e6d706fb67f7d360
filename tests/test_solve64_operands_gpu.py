"""The 64 x 64 LDL^T of solve_core<4> (n + 1 <= 64: windows of 2..7 key frames) on systems the test supplies: the matrix cores' operands are
formed in registers (a 4 x 4 transpose of 16-lane row groups), and the solution must stay bit for bit what the LDS-transposing kernel gave.

Each case drives the solve alone (the fused iteration adds with fp64 atomics in arrival order and is not reproducible to the bit): a small window,
ldso_ba_gn_reduce_local once so that the handle adopts the buffer, HFinal | bFinal overwritten with the case's system, ldso_ba_gn_solve_reduced,
x from ldso_ba_get_system.  Two yardsticks, neither of them the code under test:
  * tests/golden/solve64_parent.npz - inputs and the x of the kernel that transposed through LDS, recorded on an MI355X (scripts/golden/make_solve64_parent.py,
    which also shows two runs of that kernel equal): np.array_equal;
  * numpy's float64 solution of the same scaled system (with the gauge projection where the iteration has it on): relative error at most 3 x the
    recorded kernel's own error against numpy on the same case (stored in the golden file).
Cases: n = 20, 28, 36, 44, 60 (one to four tile rows live, the right-hand-side row n at different places inside its tile, at n = 60 all ten tiles), a zero
8 x 8 frame block at n = 60 (|d| <= TINY -> inv = 0), one negative diagonal entry at n = 28, and n = 60 with the orthogonalisation off (iteration 0) and on
(iteration 2)."""
import os

import numpy as np
import pytest

import solve_system_common as common
from solve_system_common import frame_rows, gauge_projector, hash_name, numpy_solution, relerr, scaled          # noqa: F401 (scripts/golden/make_solve64_parent.py reads them here)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "solve64_parent.npz")
# name, key frames, kind, iteration
CASES = [("spd_n20", 2, "spd", 0), ("spd_n28", 3, "spd", 0), ("spd_n36", 4, "spd", 0), ("spd_n44", 5, "spd", 0), ("spd_n60", 7, "spd", 0),
         ("spd_n60_ortho", 7, "spd", 2), ("zero_block_n60", 7, "zero_block", 0), ("indefinite_n28", 3, "indefinite", 0)]
ZERO_FRAME = 3          # zero_block: the key frame whose 8 rows and columns are zero
NEG_ENTRY = 13          # indefinite: the diagonal entry that is negative


def make_system(name, F, kind):
    """the case's system (tests/solve_system_common.py): zero_block zeroes key frame ZERO_FRAME, indefinite makes entry NEG_ENTRY negative"""
    return common.make_system(name, F, zero_ranges=(frame_rows(ZERO_FRAME),) if kind == "zero_block" else (), neg_index=NEG_ENTRY if kind == "indefinite" else None)


def run_case(F, H, b, iteration):
    """-> x of the library in use, and the numpy solution of the same case"""
    r = common.run_gn_case(F, H, b, iteration)
    return r["x"], numpy_solution(H, b, r["U"])


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.gpu
@pytest.mark.parametrize("name,F,kind,iteration", CASES, ids=[c[0] for c in CASES])
def test_solve64_matches_parent_bits_and_numpy(golden, name, F, kind, iteration):
    H, b = golden[name + "__H"], golden[name + "__b"]
    assert H.shape == (8 * F + 4, 8 * F + 4)
    x, ref = run_case(F, H, b, iteration)
    err, err_parent = relerr(x, ref), float(golden[name + "__err_numpy"])
    print(name, "rel. error against numpy", err, "recorded kernel", err_parent, "|x|", np.linalg.norm(x))
    assert np.isfinite(x).all() and np.linalg.norm(x) <= 1.001e-6
    if kind == "zero_block":
        assert not x[4 + 8 * ZERO_FRAME:12 + 8 * ZERO_FRAME].any()
    assert np.array_equal(x, golden[name + "__x"], equal_nan=True), "x differs from the LDS-transposing kernel's in at least one bit"
    assert err <= 3.0 * err_parent
