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

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "solve64_parent.npz")
# name, key frames, kind, iteration
CASES = [("spd_n20", 2, "spd", 0), ("spd_n28", 3, "spd", 0), ("spd_n36", 4, "spd", 0), ("spd_n44", 5, "spd", 0), ("spd_n60", 7, "spd", 0),
         ("spd_n60_ortho", 7, "spd", 2), ("zero_block_n60", 7, "zero_block", 0), ("indefinite_n28", 3, "indefinite", 0)]
ZERO_FRAME = 3          # zero_block: the key frame whose 8 rows and columns are zero
NEG_ENTRY = 13          # indefinite: the diagonal entry that is negative


def scaled(H):
    """the kernel's scaling: S = (diag + 10)^-1/2, S H S"""
    s = 1.0 / np.sqrt(np.diag(H) + 10.0)
    return s, H * s[:, None] * s[None, :]


def make_system(name, F, kind):
    """seeded symmetric system of n = 8 F + 4 unknowns: condition number <= 1e4 after the kernel's scaling, b scaled so that |x| = 1e-6 (the call goes on
    to step and linearise: the window stays where it is to 1e-6)"""
    n = 8 * F + 4
    rng = np.random.default_rng(abs(hash_name(name)))
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    H = (Q * np.logspace(3.0, 5.5, n)) @ Q.T
    H = 0.5 * (H + H.T)
    keep = np.ones(n, bool)
    if kind == "zero_block":
        keep[4 + 8 * ZERO_FRAME:12 + 8 * ZERO_FRAME] = False
        H[~keep, :] = 0.0; H[:, ~keep] = 0.0
    if kind == "indefinite":
        # the scaling takes the root of diag + 10: the negative entry is -5, its row and column shrunk to match (scaled, the row is what it was, its diagonal -1)
        j, w = NEG_ENTRY, np.sqrt(5.0 / H[NEG_ENTRY, NEG_ENTRY])
        H[j, :] *= w; H[:, j] *= w
        H[j, j] = -5.0
    _, Hs = scaled(H)
    cond = np.linalg.cond(Hs[np.ix_(keep, keep)])
    assert cond <= 1e4, (name, cond)
    b = rng.standard_normal(n)
    b[~keep] = 0.0
    x = np.zeros(n)
    x[keep] = np.linalg.solve(H[np.ix_(keep, keep)], b[keep])
    b *= 1e-6 / np.linalg.norm(x)
    return H, b


def hash_name(name):
    return int.from_bytes(name.encode(), "little") % (2 ** 31 - 1)          # stable from run to run, unlike hash()


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


def run_case(F, H, b, iteration):
    """-> x of the library in use, and the numpy solution of the same case"""
    import torch
    from ldso_amd import synth, binding
    win = synth.make_window(F, P=64, w=320, h=240, fx=200.0)
    g = binding.BA.from_window(win)
    g.collect_active(); g.linearize_all(False); g.apply_res()
    n = 8 * F + 4
    buf = torch.zeros(g.gn_reduce_doubles(), dtype=torch.float64, device="cuda")
    g.gn_reduce_local(buf.data_ptr(), 1e-1); g.sync(); torch.cuda.synchronize()
    buf[:n * n + n].copy_(torch.from_numpy(np.concatenate([H.reshape(-1), b])))          # the scalar tail stays
    torch.cuda.synchronize()
    ortho = iteration >= 2          # default solverMode: LDSO_SOLVER_ORTHOGONALIZE_X_LATER
    assert int(win.settings["solverMode"]) & 2048 and not int(win.settings["solverMode"]) & 256
    U = gauge_projector(g.get_frames()["frames"], float(win.settings["solverModeDelta"])) if ortho else None
    g.gn_solve_reduced(buf.data_ptr(), iteration, 1e-1); g.sync(); torch.cuda.synchronize()
    return g.get_system()["x"].copy(), numpy_solution(H, b, U)


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
