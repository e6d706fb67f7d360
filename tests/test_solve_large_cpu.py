"""The yardsticks of tests/test_solve_large_gpu.py (tests/solve_system_common.py) must hold on their own, without a GPU: a reference that is wrong fails here.

Per case of the large solve: the condition number of the kept scaled block is at most 1e4; numpy's solution and the plain float64 LDL^T agree with the long-double
LDL^T (x_hp) to 1e-12 (measured: condition 246 .. 339, numpy 3.6e-16 .. 5.5e-15, plain LDL^T 9.5e-16 .. 7.8e-15, e_model 2.8e-15 .. 2.7e-14); e_model - the plain
float64 LDL^T with every pivot reciprocal off by the 2.2e-15 that fast_rcp documents - is at least the plain float64 LDL^T's own error (2.4 .. 5.7 x it; the draws are
seeded by the case's name.  The property is statistical: on the negative-pivot systems one component dominates x, the reciprocals matter little, and a seed can be
found at which e_model is 0.94 x the plain error - this assertion is what notices such a seed); zeroed ranges give exactly zero in every reference.
The yardstick on the one real kernel output the repository holds (tests/golden/solve64_parent.npz, the x of the 64 x 64 kernel recorded on an MI355X): within
e_model of x_hp on every case (measured 0.09 .. 0.40 of it; up to 2.3 x the plain float64 LDL^T's error, which is why that times 3 would be too close a bound).
Sensitivity: three deliberately wrong variants of the plain LDL^T - one column's update skipped, one reciprocal truncated to float32, the back substitution
taking x_k from the other 64-row segment - each go through the assertion the GPU tests make and miss 3 x e_model by orders of magnitude."""
import functools

import numpy as np
import pytest

import solve_system_common as common
import test_solve64_operands_gpu as t64

IDS = [c[0] for c in common.LARGE_CASES]


@functools.lru_cache(maxsize=None)
def large_case(name):
    """-> H, b, U, Refs of a case of the large solve, as the fast-path test builds them (U from the window's own nullspaces: the upload copies them)"""
    _, F, iteration, zero_ranges, neg_index = common.LARGE_BY_NAME[name]
    H, b = common.make_system(name, F, zero_ranges, neg_index)
    U = common.window_projector(common.window(F), iteration)
    return H, b, U, common.Refs(name, H, b, U)


@pytest.fixture(scope="module")
def golden():
    return np.load(t64.GOLDEN)


def test_long_double_is_wider_than_double():
    assert np.finfo(np.longdouble).eps <= 1.1e-19          # x_hp is a high-precision reference only where long double is the x87 format


@pytest.mark.parametrize("name", IDS)
def test_references_hold_on_their_own(name):
    _, F, iteration, zero_ranges, neg_index = common.LARGE_BY_NAME[name]
    H, b, U, refs = large_case(name)
    n = 8 * F + 4
    assert H.shape == (n, n) and np.array_equal(H, H.T) and (U is not None) == (iteration >= 2)
    cond = common.kept_condition(H, zero_ranges)
    e_np, e_plain = common.relerr(refs.x_np, refs.x_hp), common.relerr(refs.x_plain, refs.x_hp)
    print(name, "n", n, "condition", cond, "numpy", e_np, "plain float64 LDLT", e_plain, "e_model", refs.e_model, "draws", refs.draws)
    assert cond <= 1e4
    if neg_index is not None:
        assert H[neg_index, neg_index] == -5.0 and (np.delete(np.diag(H), neg_index) > 0).all()
    assert e_np <= 1e-12 and e_plain <= 1e-12
    assert refs.e_model >= e_plain
    assert abs(np.linalg.norm(refs.x_hp) - 1e-6) <= 1e-9 or U is not None          # b is scaled so that |x| = 1e-6 (the projection only shortens x)
    assert np.linalg.norm(refs.x_hp) <= 1.001e-6
    for lo, hi in zero_ranges:
        assert not H[lo:hi].any() and not H[:, lo:hi].any() and not b[lo:hi].any()
        for x in (refs.x_hp, refs.x_np, refs.x_plain):
            assert not x[lo:hi].any()
    for x in (refs.x_hp, refs.x_np, refs.x_plain):
        assert np.isfinite(x).all() and x.dtype == np.float64


@pytest.mark.parametrize("name,F,kind,iteration", t64.CASES, ids=[c[0] for c in t64.CASES])
def test_make_system_still_generates_the_golden_inputs(golden, name, F, kind, iteration):
    """the generalised make_system (index ranges to zero, index of the negative entry) gives the 64 x 64 cases the systems the golden file was recorded on"""
    H, b = t64.make_system(name, F, kind)
    assert np.array_equal(H, golden[name + "__H"]) and np.array_equal(b, golden[name + "__b"])


@pytest.mark.parametrize("name,F,kind,iteration", t64.CASES, ids=[c[0] for c in t64.CASES])
def test_yardstick_on_the_recorded_64x64_kernel(golden, name, F, kind, iteration):
    """the x that the 64 x 64 kernel gave on an MI355X is within e_model of x_hp: the yardstick, anchored to a known-good kernel"""
    H, b, x = golden[name + "__H"], golden[name + "__b"], golden[name + "__x"]
    U = common.window_projector(common.window(F), iteration)
    refs = common.Refs(name, H, b, U)
    zero = (common.frame_rows(t64.ZERO_FRAME),) if kind == "zero_block" else ()
    e_plain = common.relerr(refs.x_plain, refs.x_hp)
    err = common.check_solution(x, refs, zero, max_norm=1.001e-6, margin=1.0)
    print(name, "recorded kernel", err, "e_model", refs.e_model, "share", err / refs.e_model, "plain float64 LDLT", e_plain, "multiple", err / e_plain)
    assert common.relerr(refs.x_np, refs.x_hp) <= 1e-12 and e_plain <= 1e-12 and refs.e_model >= e_plain


WRONG = {"skip_column": lambda n: ("skip_column", n // 2), "rcp_f32": lambda n: ("rcp_f32", n // 2), "swap_segments": lambda n: ("swap_segments",)}


@pytest.mark.parametrize("fault", sorted(WRONG))
@pytest.mark.parametrize("name", ["spd_n68", "spd_n108", "spd_n132_ortho", "zero_frame15_n132", "indefinite_n116"])
def test_yardstick_rejects_wrong_variants(name, fault):
    """sensitivity, on the Python reference: a subtly wrong solve fails the assertion the GPU tests make, by orders of magnitude"""
    zero_ranges = common.LARGE_BY_NAME[name][3]
    H, b, U, refs = large_case(name)
    x = common.project(common.ldlt_plain(H, b, np.float64, fault=WRONG[fault](len(b))), U)
    err = common.relerr(x, refs.x_hp)
    print(name, fault, "error", err, "=", err / (common.MARGIN * refs.e_model), "x the bound")
    assert np.isfinite(x).all()          # wrong but finite: nothing else would notice
    assert err > 1e3 * common.MARGIN * refs.e_model
    with pytest.raises(AssertionError):
        common.check_solution(x, refs, zero_ranges)
    common.check_solution(refs.x_plain, refs, zero_ranges)          # and the right one passes it
