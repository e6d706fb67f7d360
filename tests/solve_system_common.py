"""Supplied-system tests of solve_core (ba_ldlt.h): case generation, references and harnesses shared by tests/test_solve64_operands_gpu.py (NB = 4, the 64 x 64
system on the matrix cores), tests/test_solve_large_cpu.py and tests/test_solve_large_gpu.py (NB = 7 / 9, the 112- and 144-row VALU variants).

References of one operation - x = S (S H S)^+ S b with S = (diag H + 10)^-1/2, rows / columns that are exactly zero give x = 0, then (iteration >= 2) x -= U U^T x
against the gauge directions - none of them the code under test:
  * numpy_solution      numpy's float64 LU of the kept scaled block;
  * ldlt_plain          the kernel's ALGORITHM written plainly (scaling, column-by-column unpivoted LDL^T with inv = 0 where |d| <= TINY, forward substitution as row n
                        of the augmented system, z = y / d, back substitution, unscale) in a dtype of the caller's choice;
  * x_hp                ldlt_plain in np.longdouble (eps 1.08e-19 on x86-64): the high-precision solution every error is measured against;
  * e_model             the largest error against x_hp over E_MODEL_DRAWS seeded draws of ldlt_plain(float64) with every pivot reciprocal off by a relative
                        RCP_REL = 2.2e-15 of random sign - the bound the comment above fast_rcp documents for the kernel's reciprocal (hardware estimate + one
                        Newton step).  This is what a correct float64 implementation with that reciprocal is expected to reach; the kernels get 3 x that (a different
                        but valid summation order, fma contraction): the margin tests/test_solve64_operands_gpu.py already gives the same quantity.
The harnesses need a GPU; everything else is numpy only."""
import functools

import numpy as np

TINY = 2.2250738585072014e-308          # solve_core: |d| <= TINY -> inv = 0
RCP_REL = 2.2e-15                       # fast_rcp (ba_ldlt.h): documented relative error of the pivot reciprocal
E_MODEL_DRAWS = 4
MARGIN = 3.0                            # the kernel against e_model


def frame_rows(f):
    """index range of key frame f's 8 unknowns (the 4 calibration unknowns come first)"""
    return (4 + 8 * f, 12 + 8 * f)


CALIB_ROWS = (0, 4)

# ---- the cases of the large solve: name, key frames, iteration (>= 2: orthogonalisation on), zeroed index ranges, index of the negative diagonal entry -------------------
# n + 1 = 69 .. 109 run solve_core<7> (M = 112), 117 .. 133 solve_core<9> (M = 144); the right-hand-side row n sits at row 4 or 12 of tiles 4 .. 8
def _case(kind, F, iteration=0, zero_ranges=(), neg_index=None):
    return ("%s_n%d" % (kind, 8 * F + 4) + ("_ortho" if iteration >= 2 else ""), F, iteration, tuple(zero_ranges), neg_index)          # named like the 64 x 64 cases


LARGE_CASES = (
    [_case("spd", F) for F in range(8, 17)]
    + [_case("spd", F, iteration=2) for F in (8, 13, 14, 16)]
    + [_case("zero_frame7", 8, zero_ranges=[frame_rows(7)]),            # rows 60..67: lanes 63 | 64 of the back substitution, tiles 3 | 4
       _case("zero_frame12", 13, zero_ranges=[frame_rows(12)]),         # rows 100..107: the last rows before the right-hand side under M = 112
       _case("zero_frame15", 16, zero_ranges=[frame_rows(15)]),         # rows 124..131: across the 127 | 128 segment boundary
       _case("zero_frame0", 16, zero_ranges=[frame_rows(0)]),           # rows 4..11: across the first and third panels
       _case("zero_calib", 12, zero_ranges=[CALIB_ROWS]),               # rows 0..3: the whole first pivot block has inv = 0
       _case("indefinite", 9, neg_index=65),                            # a negative pivot in the second 64-row segment
       _case("indefinite", 14, neg_index=113),
       _case("indefinite", 16, neg_index=129)])                         # ... in the third
LARGE_BY_NAME = {c[0]: c for c in LARGE_CASES}
assert len(LARGE_BY_NAME) == len(LARGE_CASES)
# the step-wise kernel (k_solve, GN = false) runs a subset of the same systems
STEP_CASES = [LARGE_BY_NAME[k] for k in ("spd_n68", "spd_n108", "spd_n116", "spd_n132", "spd_n108_ortho", "spd_n132_ortho", "zero_frame7_n68", "zero_frame15_n132", "indefinite_n116")]


def scaled(H):
    """the kernel's scaling: S = (diag + 10)^-1/2, S H S"""
    s = 1.0 / np.sqrt(np.diag(H) + 10.0)
    return s, H * s[:, None] * s[None, :]


def hash_name(name):
    return int.from_bytes(name.encode(), "little") % (2 ** 31 - 1)          # stable from run to run, unlike hash()


def keep_mask(n, zero_ranges):
    keep = np.ones(n, bool)
    for lo, hi in zero_ranges:
        keep[lo:hi] = False
    return keep


def kept_condition(H, zero_ranges=()):
    """condition number of the kept block of the scaled system"""
    keep = keep_mask(len(H), zero_ranges)
    return float(np.linalg.cond(scaled(H)[1][np.ix_(keep, keep)]))


def make_system(name, F, zero_ranges=(), neg_index=None):
    """seeded symmetric system of n = 8 F + 4 unknowns: condition number <= 1e4 after the kernel's scaling, b scaled so that |x| = 1e-6 (the call goes on
    to step and linearise: the window stays where it is to 1e-6).  zero_ranges: index ranges (lo, hi) whose rows and columns are zero; neg_index: the diagonal
    entry that is negative"""
    n = 8 * F + 4
    rng = np.random.default_rng(abs(hash_name(name)))
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    H = (Q * np.logspace(3.0, 5.5, n)) @ Q.T
    H = 0.5 * (H + H.T)
    keep = keep_mask(n, zero_ranges)
    H[~keep, :] = 0.0; H[:, ~keep] = 0.0
    if neg_index is not None:
        # the scaling takes the root of diag + 10: the negative entry is -5, its row and column shrunk to match (scaled, the row is what it was, its diagonal -1)
        j, w = neg_index, np.sqrt(5.0 / H[neg_index, neg_index])
        H[j, :] *= w; H[:, j] *= w
        H[j, j] = -5.0
    cond = kept_condition(H, zero_ranges)
    assert cond <= 1e4, (name, cond)
    b = rng.standard_normal(n)
    b[~keep] = 0.0
    x = np.zeros(n)
    x[keep] = np.linalg.solve(H[np.ix_(keep, keep)], b[keep])
    b *= 1e-6 / np.linalg.norm(x)
    return H, b


def gauge_projector(frames, delta):
    """U of x -= U U^T x (EnergyFunctional::orthogonalize): the 7 gauge directions with normalised columns, the left singular vectors above delta * largest"""
    F = len(frames)
    N = np.zeros((8 * F + 4, 7))
    for f in range(F):
        N[4 + 8 * f:4 + 8 * f + 6, :6] = np.asarray(frames["nullspaces_pose"][f]).reshape(6, 6)
        N[4 + 8 * f:4 + 8 * f + 6, 6] = frames["nullspaces_scale"][f]
        N[4 + 8 * f:4 + 8 * f + 3, :] *= 2.0                                          # SCALE_XI_TRANS_INVERSE
    N /= np.linalg.norm(N, axis=0)
    U, sv, _ = np.linalg.svd(N, full_matrices=False)
    return U[:, sv > delta * sv.max()]


def project(x, U):
    """the float64 projection every reference gets"""
    x = np.asarray(x, np.float64)
    return x if U is None else x - U @ (U.T @ x)


def numpy_solution(H, b, U=None):
    """float64 solution of the scaled system; rows / columns that are exactly zero give x = 0 (the kernel: inv = 0)"""
    keep = np.diag(H) != 0.0
    s, Hs = scaled(H)
    x = np.zeros(len(b))
    x[keep] = s[keep] * np.linalg.solve(Hs[np.ix_(keep, keep)], (s * b)[keep])
    if U is not None:
        x = x - U @ (U.T @ x)
    return x


def relerr(x, ref):
    return float(np.linalg.norm(x - ref) / np.linalg.norm(ref))


def ldlt_plain(H, b, dtype, rcp_rel=0.0, rng=None, fault=None):
    """solve_core's algorithm, plainly, in `dtype` -> x (unprojected, in `dtype`).  The augmented system [S H S ; (S b)^T] (row n, the right-hand side, unscaled: the
    forward substitution is part of the factorisation), column by column: d_k = A[k][k], inv_k = 1 / d_k or 0 where |d_k| <= TINY, L[i][k] = A[i][k] inv_k,
    A[i][j] -= L[i][k] A[j][k]; y = row n, z_i = y_i / d_i or 0; x_i = z_i - sum_{k > i} L[k][i] x_k; x *= S.
    rcp_rel > 0: every pivot reciprocal is multiplied by 1 + rcp_rel * s, s = +-1 drawn from rng.
    fault: a deliberately WRONG variant, for showing that the yardstick notices (tests/test_solve_large_cpu.py) - ("skip_column", k): column k's update of the rest
    is left out; ("rcp_f32", k): pivot k's reciprocal is truncated to float32; ("swap_segments",): the back substitution takes x_k from the other 64-row segment."""
    n = len(b)
    H = np.asarray(H, dtype); b = np.asarray(b, dtype)
    one, ten = dtype(1.0), dtype(10.0)
    s = one / np.sqrt(np.diag(H) + ten)
    A = np.empty((n + 1, n), dtype)
    A[:n] = H * s[:, None] * s[None, :]
    A[n] = s * b
    L = np.zeros((n + 1, n), dtype)
    d = np.zeros(n, dtype)
    for k in range(n):
        d[k] = A[k, k]
        inv = one / d[k] if abs(d[k]) > TINY else dtype(0.0)
        if rcp_rel > 0.0:
            inv = inv * (one + dtype(rcp_rel) * dtype(rng.choice((-1.0, 1.0))))
        if fault == ("rcp_f32", k):
            inv = dtype(np.float32(inv))
        L[k + 1:, k] = A[k + 1:, k] * inv
        if fault == ("skip_column", k):
            continue
        A[k + 1:, k + 1:] -= np.outer(L[k + 1:, k], A[k + 1:n, k])          # only the lower triangle and row n are read again
    y = A[n]
    x = np.zeros(n, dtype)
    live = np.abs(d) > TINY
    x[live] = y[live] / d[live]
    for k in range(n - 1, 0, -1):
        xk = x[k ^ 64] if fault == ("swap_segments",) and (k ^ 64) < n else x[k]
        x[:k] -= L[k, :k] * xk
    return x * s


class Refs:
    """the references of one case: x_hp, x_np (numpy_solution), x_plain (ldlt_plain in float64), e_model, all projected alike in float64"""

    def __init__(self, name, H, b, U=None):
        self.x_hp = project(ldlt_plain(H, b, np.longdouble), U)
        self.x_np = numpy_solution(H, b, U)
        self.x_plain = project(ldlt_plain(H, b, np.float64), U)
        self.draws = [relerr(project(ldlt_plain(H, b, np.float64, RCP_REL, np.random.default_rng([hash_name(name), k])), U), self.x_hp) for k in range(E_MODEL_DRAWS)]
        self.e_model = max(self.draws)


def check_solution(x, refs, zero_ranges=(), max_norm=None, observe=None, margin=MARGIN):
    """THE assertion on a solution of the code under test (or, on the CPU, of a deliberately wrong variant): finite, exactly zero on zeroed ranges, relative
    error against x_hp at most margin * e_model.  observe: (function, name) - tests/conftest.py's observe, which keeps the measured error -> the error"""
    x = np.asarray(x, np.float64)
    assert np.isfinite(x).all()
    if max_norm is not None:
        assert np.linalg.norm(x) <= max_norm, np.linalg.norm(x)
    for lo, hi in zero_ranges:
        assert not x[lo:hi].any(), (lo, hi, x[lo:hi])
    err = relerr(x, refs.x_hp)
    if observe is not None:
        observe[0](observe[1], err, margin * refs.e_model)
    assert err <= margin * refs.e_model, (err, refs.e_model, err / refs.e_model)
    return err


# ---- windows and harnesses ----------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def window(F):
    """the small window every supplied-system case of F key frames runs on (its residuals only make the scalar tail of the reduce buffers legitimate)"""
    from ldso_amd import synth
    return synth.make_window(F, P=64, w=320, h=240, fx=200.0)


def ortho_on(win, iteration):
    """default solverMode: LDSO_SOLVER_ORTHOGONALIZE_X_LATER"""
    assert int(win.settings["solverMode"]) & 2048 and not int(win.settings["solverMode"]) & 256
    return iteration >= 2


def window_projector(win, iteration, frames=None):
    """U of the case, from the nullspaces the handle holds (frames = get_frames()["frames"]) or, without a GPU, from the window's own: the upload copies them"""
    if not ortho_on(win, iteration):
        return None
    return gauge_projector(win.frames if frames is None else frames, float(win.settings["solverModeDelta"]))


def _prepared(F):
    import torch          # noqa: F401
    from ldso_amd import binding
    win = window(F)
    g = binding.BA.from_window(win)
    g.collect_active(); g.linearize_all(False); g.apply_res()
    return win, g


def run_gn_case(F, H, b, iteration):
    """the fast path (k_gn_solve, GN = true) on a supplied system: ldso_ba_gn_reduce_local once so that the handle adopts the buffer, HFinal | bFinal overwritten,
    ldso_ba_gn_solve_reduced -> dict(x, U, before, after): x from ldso_ba_get_system, get_frames() before and after the call"""
    import torch
    win, g = _prepared(F)
    n = 8 * F + 4
    buf = torch.zeros(g.gn_reduce_doubles(), dtype=torch.float64, device="cuda")
    g.gn_reduce_local(buf.data_ptr(), 1e-1); g.sync(); torch.cuda.synchronize()
    buf[:n * n + n].copy_(torch.from_numpy(np.concatenate([H.reshape(-1), b])))          # the scalar tail stays
    torch.cuda.synchronize()
    before = g.get_frames()
    U = window_projector(win, iteration, before["frames"])
    g.gn_solve_reduced(buf.data_ptr(), iteration, 1e-1); g.sync(); torch.cuda.synchronize()
    return dict(x=g.get_system()["x"].copy(), U=U, before=before, after=g.get_frames())


def run_step_case(F, H, b, iteration):
    """the step-wise kernel (k_solve, GN = false) on a supplied system: ldso_ba_reduce_local once (a legitimate scalar and candidate tail), the three (n^2 + n)
    blocks overwritten, ldso_ba_solve_reduced without the step.  k_gather (mode 2) assembles HFinal = (L + prior + A) with the diagonal times 1 + 1e-5
    (LDSO_SOLVER_FIX_LAMBDA) - Schur / (1 + 1e-5), bFinal = (L + prior delta_prior) + A - Schur: the A block is H | b MINUS the priors (a zeroed row cancels to
    exactly zero), L and Schur are zero -> dict(x, U, HFinal, bFinal): the system the kernel solved, as read back"""
    import torch
    win, g = _prepared(F)
    n = 8 * F + 4
    blk = n * n + n
    buf = torch.zeros(g.reduce_doubles(), dtype=torch.float64, device="cuda")
    g.reduce_local(buf.data_ptr()); g.sync(); torch.cuda.synchronize()
    fr = g.get_frames()
    assert np.array_equal(fr["calib_value"], win.calib["value_zero"])          # the calibration's prior term on b is initialCalibHessian * (value - value_zero) = 0
    prior = np.concatenate([np.full(4, float(np.float32(win.settings["initialCalibHessian"]))), np.asarray(win.frames["prior"], np.float64).reshape(-1)])
    delta_prior = np.concatenate([np.zeros(4), np.asarray(fr["frames"]["state"], np.float64)[:, :8].reshape(-1)])
    HA = H.copy()
    HA[np.diag_indices(n)] -= prior
    bA = b - prior * delta_prior
    buf[:3 * blk].copy_(torch.from_numpy(np.concatenate([HA.reshape(-1), bA, np.zeros(2 * blk)])))          # the scalar tail stays
    torch.cuda.synchronize()
    U = window_projector(win, iteration, fr["frames"])
    g.solve_reduced(buf.data_ptr(), iteration, 1e-1, do_step=False); g.sync(); torch.cuda.synchronize()
    s = g.get_system()
    return dict(x=s["x"].copy(), U=U, HFinal=s["HFinal"].copy(), bFinal=s["bFinal"].copy())
