"""The 112- and 144-row LDL^T of solve_core<7> / <9> (ba_ldlt.h; n + 1 = 69 .. 133: windows of 8 .. 16 key frames, VALU) on systems the test supplies, against the long-double
solution of the same operation - the test the 64 x 64 variant has in tests/test_solve64_operands_gpu.py, for the code that is specific to the large variants: the
|d| <= TINY -> inv = 0 pivot, a negative pivot, the packed LIX storage of L, the two- and three-segment back substitution (lane l owns rows l, l + 64, l + 128; x_k is
broadcast across the 64 | 128 boundaries), the right-hand-side row n at row 4 or 12 of tiles 4 .. 8, the padding rows n + 1 .. M - 1, the gauge projection with up to
924 entries, and gn_tail without the single-wavefront split (F F > 64) and without the LDS adjoint copies (F > 8).

Both instantiations are driven (they are compiled differently: 272 / 275 against 280 VGPRs, see the NR loop of solve_core):
  * the fast path, k_gn_solve (GN = true, the lower triangle read from the accumulator): small window, ldso_ba_gn_reduce_local once, HFinal | bFinal overwritten,
    ldso_ba_gn_solve_reduced, x from ldso_ba_get_system; the fused step of gn_tail (state += -x, calibration += -x) must be bit-exact;
  * the step-wise kernel, k_solve (GN = false): ldso_ba_reduce_local, the three blocks of the reduce buffer overwritten so that k_gather assembles the case's system,
    ldso_ba_solve_reduced without the step; the references are built from HFinal | bFinal as read back (k_gather scales the diagonal by 1 + 1e-5).
Yardsticks (tests/solve_system_common.py; they are checked on their own, and shown to reject wrong variants, in tests/test_solve_large_cpu.py): x_hp, the kernel's
algorithm in long double, and e_model, the error a plain float64 LDL^T reaches when every pivot reciprocal is off by the 2.2e-15 documented above fast_rcp.  The
kernel may be 3 x e_model from x_hp - the margin the 64 x 64 test gives the same quantity, for a different but valid summation order and fma contraction; it is not
measured from the kernel.  The measured errors are kept (conftest.observe: solve_large_<case>, solve_large_step_<case>) and tabulated in DESIGN.md, section 5."""
import numpy as np
import pytest

import solve_system_common as common
from conftest import observe

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,F,iteration,zero_ranges,neg_index", common.LARGE_CASES, ids=[c[0] for c in common.LARGE_CASES])
def test_gn_solve_large_against_long_double(name, F, iteration, zero_ranges, neg_index):
    H, b = common.make_system(name, F, zero_ranges, neg_index)
    n = 8 * F + 4
    assert H.shape == (n, n) and 64 < n + 1 <= 144
    r = common.run_gn_case(F, H, b, iteration)
    x = r["x"]
    assert (r["U"] is not None) == (iteration >= 2)
    refs = common.Refs(name, H, b, r["U"])
    print(name, "n", n, "rel. error against long double", common.relerr(x, refs.x_hp), "e_model", refs.e_model, "numpy", common.relerr(refs.x_np, refs.x_hp),
          "plain float64 LDLT", common.relerr(refs.x_plain, refs.x_hp), "|x|", np.linalg.norm(x))
    common.check_solution(x, refs, zero_ranges, max_norm=1.001e-6, observe=(observe, "solve_large_" + name))
    # gn_tail: backupState + doStepFromBackup on the frames and the calibration, fused into the output pass - state = backup + (-x), bit for bit
    before, after = r["before"], r["after"]
    state0, state1 = np.asarray(before["frames"]["state"], np.float64), np.asarray(after["frames"]["state"], np.float64)
    assert np.array_equal(state1[:, :8], state0[:, :8] + (-x[4:].reshape(F, 8)))
    assert np.array_equal(state1[:, 8:], state0[:, 8:])
    assert np.array_equal(after["calib_value"], before["calib_value"] + (-x[:4]))
    assert np.array_equal(after["step"][:, :8], -x[4:].reshape(F, 8)) and np.array_equal(after["calib_step"], -x[:4])
    for lo, hi in zero_ranges:
        if lo >= 4:
            f = (lo - 4) // 8
            assert np.array_equal(state1[f], state0[f])          # a frame whose block was zeroed keeps its state
        else:
            assert np.array_equal(after["calib_value"], before["calib_value"])
    assert (state1[:, :8] != state0[:, :8]).any()


@pytest.mark.parametrize("name,F,iteration,zero_ranges,neg_index", common.STEP_CASES, ids=[c[0] for c in common.STEP_CASES])
def test_step_solve_large_against_long_double(name, F, iteration, zero_ranges, neg_index):
    H, b = common.make_system(name, F, zero_ranges, neg_index)
    n = 8 * F + 4
    r = common.run_step_case(F, H, b, iteration)
    HF, bF, x = r["HFinal"], r["bFinal"], r["x"]
    # the system the kernel solved is the case's: symmetric, zeroed rows and columns exactly zero, the diagonal (1 + 1e-5) x the case's up to the rounding of
    # (prior + (H - prior)), everything else the case's own numbers
    assert np.isfinite(HF).all() and np.isfinite(bF).all() and np.array_equal(HF, HF.T)
    for lo, hi in zero_ranges:
        assert not HF[lo:hi].any() and not HF[:, lo:hi].any() and not bF[lo:hi].any()
    off = ~np.eye(n, dtype=bool)
    assert np.array_equal(HF[off], H[off])
    assert np.allclose(np.diag(HF), np.diag(H) * (1.0 + 1e-5), rtol=0.0, atol=0.1)          # priors up to 1e14 on the diagonal: half an ulp of them is 0.008
    assert common.kept_condition(HF, zero_ranges) <= 1e4
    refs = common.Refs(name, HF, bF, r["U"])
    print(name, "n", n, "rel. error against long double", common.relerr(x, refs.x_hp), "e_model", refs.e_model, "numpy", common.relerr(refs.x_np, refs.x_hp),
          "plain float64 LDLT", common.relerr(refs.x_plain, refs.x_hp), "|x|", np.linalg.norm(x))
    assert common.relerr(refs.x_np, refs.x_hp) <= 1e-12 and common.relerr(refs.x_plain, refs.x_hp) <= 1e-12          # the references, on the system as read back
    common.check_solution(x, refs, zero_ranges, observe=(observe, "solve_large_step_" + name))
