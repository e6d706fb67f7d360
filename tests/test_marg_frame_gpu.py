"""ldso_ba_marginalize_frame (k_marg_frame, ldso_amd/csrc/ba_reduce.hip) at EVERY frame index of every frame-count boundary, against two references of
EnergyFunctional::marginalizeFrame (EnergyFunctional.cc:72-131): the oracle's restatement (oracle/backend.cc) and a long-double numpy restatement kept in
this file.  The reference's key-frame policy (FullSystem::flagFramesForMarginalization, FullSystem.cc:647-720) removes MIDDLE frames as its normal case:
the permutation that moves the frame's 8 rows / columns to the end (`perm()` of the kernel) does nothing at idx = F-1, shifts everything at idx = 0 and
splits the matrix anywhere else.

The prior of these tests has FULL rank.  synth.add_synthetic_prior is rank 6: a frame without a pose prior (every frame but frameID 0) then has a singular
8 x 8 block, its inverse is noise, and two correct implementations disagree by O(1).  The full-rank prior is HM + 0.1 s s^T o (B B^T / 3n) with B an n x 3n
standard normal and s = sqrt(|diag HM| + 1); the scaled eliminated block then has a condition number <= 39 at every index (asserted < 1e3 on the input).

The reference averages the eliminated block and its inverse with THEMSELVES (`hpi = 0.5f * (hpi + hpi)`, EnergyFunctional.cc:116,118 - a no-op), not with
their transposes.  On a symmetric prior the two are the same; on a prior asymmetric at 1e-6 they are 7e-7 .. 1.2e-5 apart in the resulting b_M (and 1e-11 ..
4e-10 in H_M), which is what the asymmetric half of the grid is for.  The kernel used the transposed average until this test existed."""
import copy

import numpy as np
import pytest

from conftest import rel, blockrel, observe
from ldso_amd import synth, binding
from oracle import pyoracle as po

FRAME_COUNTS = (2, 3, 5, 8, 9, 12, 16)          # minimum, odd small, the usual window, one slot group full, the second appears, C5's, LDSO_MAX_FRAMES
LD = np.longdouble


# ---- the long-double restatement of EnergyFunctional.cc:72-131 -----------------------------------------------------------------------------------------
def _inverse_ld(M):
    """Gauss-Jordan with partial pivoting in long double (numpy.linalg has no long-double inverse)"""
    k = M.shape[0]
    A = np.concatenate([M.astype(LD), np.eye(k, dtype=LD)], axis=1)
    for c in range(k):
        p = c + int(np.argmax(np.abs(A[c:, c])))
        if p != c:
            A[[c, p]] = A[[p, c]]
        A[c] = A[c] / A[c, c]
        for r in range(k):
            if r != c:
                A[r] = A[r] - A[r, c] * A[c]
    return A[:, k:]


def marginalize_frame_np(HM, bM, prior, delta_prior, idx):
    """-> (H_M, b_M of the window without frame idx as float64, the scaled 8 x 8 block that gets inverted)"""
    n = HM.shape[0]
    nd, io = n - 8, 4 + 8 * idx
    order = list(range(io)) + list(range(io + 8, n)) + list(range(io, io + 8))          # :81-100 the frame's rows / columns go to the end, the others keep their order
    H = np.asarray(HM, LD)[np.ix_(order, order)].copy()
    b = np.asarray(bM, LD)[order].copy()
    pr, dp = np.asarray(prior, LD), np.asarray(delta_prior, LD)
    H[np.arange(nd, n), np.arange(nd, n)] += pr                                            # :104-105
    b[nd:] += pr * dp
    S = np.sqrt(np.abs(np.diag(H)) + LD(10))                                                # :107-112
    Si = LD(1) / S
    Hs = Si[:, None] * H * Si[None, :]
    bs = Si * b
    hp = Hs[nd:, nd:].copy()                                                                # :115-118
    block = hp.astype(np.float64)
    hpi = LD(0.5) * (hp + hp)                                                               # sic: with itself, not with its transpose
    hpi = _inverse_ld(hpi)
    hpi = LD(0.5) * (hpi + hpi)
    bl = Hs[nd:, :nd].copy()                                                                # :121-123
    bli = bl.T @ hpi
    Hs[:nd, :nd] -= bli @ bl
    bs[:nd] -= bli @ bs[nd:]
    Hu = S[:, None] * Hs * S[None, :]                                                       # :126-127
    bu = S * bs
    Hn = LD(0.5) * (Hu[:nd, :nd] + Hu[:nd, :nd].T)                                          # :130-131
    return Hn.astype(np.float64), bu[:nd].astype(np.float64), block


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------------------------
_WINDOWS = {}


def _window(F):
    if F not in _WINDOWS:
        _WINDOWS[F] = synth.make_window(F=F, P=40 + 3 * F, w=256, h=192, fx=160.0, seed=300 + F)
        assert _WINDOWS[F].F == F
    return _WINDOWS[F]


def _full_rank_prior(win, asymmetric):
    w = synth.add_synthetic_prior(copy.deepcopy(win), seed=20 + win.F)
    rng = np.random.default_rng(7000 + win.F)
    n = w.HM.shape[0]
    B = rng.standard_normal((n, 3 * n))
    s = np.sqrt(np.abs(np.diag(w.HM)) + 1.0)
    HM = w.HM + 0.1 * np.outer(s, s) * (B @ B.T / (3 * n))
    if asymmetric:
        A = rng.standard_normal((n, n))
        HM = HM * (1.0 + 1e-6 * (A - A.T))
    return HM, w.bM.copy()


def _with_prior(win, HM, bM):
    w = copy.deepcopy(win)
    w.HM, w.bM = HM.copy(), bM.copy()
    return w


def _oracle(w, idx):
    o = po.OracleWindow(w)
    o.marginalize_frame(idx)
    H, b = o.get_prior()
    o.close()
    return H, b


def _numpy(w, idx):
    return marginalize_frame_np(w.HM, w.bM, w.frames["prior"][idx], w.frames["state"][idx, :8], idx)


def _index_class(F, idx):
    return "first" if idx == 0 else "last" if idx == F - 1 else "middle"


def _dist(Ha, ba, Hb, bb):
    return max(blockrel(Ha, Hb, 4), rel(ba, bb))


# ---- CPU: the two references agree, so a drifting helper cannot hide a kernel error ----------------------------------------------------------------------
@pytest.mark.parametrize("asymmetric", [False, True], ids=["symmetric", "asymmetric"])
@pytest.mark.parametrize("F", FRAME_COUNTS)
def test_numpy_restatement_equals_the_oracle(F, asymmetric):
    win = _window(F)
    w = _with_prior(win, *_full_rank_prior(win, asymmetric))
    worst = 0.0
    for idx in range(F):
        Hn, bn, block = _numpy(w, idx)
        assert np.linalg.cond(block) < 1e3, (F, idx, np.linalg.cond(block))                # on the input alone; observed <= 39
        Ho, bo = _oracle(w, idx)
        assert Ho.shape == Hn.shape == (8 * (F - 1) + 4,) * 2
        worst = max(worst, _dist(Ho, bo, Hn, bn))
    assert worst <= 1e-12, (F, worst)                                                        # observed <= 1.3e-14


def test_transposed_averaging_is_a_different_function_on_an_asymmetric_prior():
    """What the asymmetric half of the grid can see: 0.5 (hpi + hpi^T) in place of the reference's 0.5 (hpi + hpi) on a prior asymmetric at 1e-6 (a float64
    restatement of the OTHER formula, here only to show the distance).  b_M = b - bl^T hpi b_tail moves in first order of the asymmetry (measured 7e-7 ..
    1.2e-5 over the grid), decades above the 1e-9 limit of the device comparison; H_M, symmetrised at the end, only in second order (1e-11 .. 4e-10: the
    symmetric part of an inverse is the inverse of the symmetric part to first order).  Not at idx 0: frameID 0 carries the pose prior of 1e10 .. 1e14, its
    scaled block is the identity to 1e-7 and both formulas give the same inverse."""
    win = _window(5)
    w = _with_prior(win, *_full_rank_prior(win, True))
    for idx in range(1, 5):
        Hn, bn, _ = _numpy(w, idx)
        n = w.HM.shape[0]
        nd, io = n - 8, 4 + 8 * idx
        order = list(range(io)) + list(range(io + 8, n)) + list(range(io, io + 8))
        H = w.HM[np.ix_(order, order)].copy(); b = w.bM[order].copy()
        H[np.arange(nd, n), np.arange(nd, n)] += w.frames["prior"][idx]; b[nd:] += w.frames["prior"][idx] * w.frames["state"][idx, :8]
        S = np.sqrt(np.abs(np.diag(H)) + 10.0)
        Hs = H / np.outer(S, S); bs = b / S
        hp = Hs[nd:, nd:]
        hpi = np.linalg.inv(0.5 * (hp + hp.T)); hpi = 0.5 * (hpi + hpi.T)
        bt = (bs[:nd] - Hs[nd:, :nd].T @ hpi @ bs[nd:]) * S[:nd]
        assert rel(bt, bn) > 1e-7, (idx, rel(bt, bn))                                       # 100 x the device limit; first order of a 1e-6 asymmetry


# ---- GPU: the grid ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("asymmetric", [False, True], ids=["symmetric", "asymmetric"])
@pytest.mark.parametrize("F", FRAME_COUNTS)
def test_marginalize_frame_at_every_index(F, asymmetric):
    """device against the oracle and against the numpy restatement at every idx of range(F): the project's 1e-9 of marginalize_frame_same_input
    (tests/test_ba_gpu.py) - fp64 on all three sides.  Observed on MI355X: see the comments at the observe() calls.  With the transposed averaging the kernel
    had before, the asymmetric half fails at every F (b_M 1.1e-6 .. 9.6e-6 at idx 1); with a permutation that leaves the frame in place for idx > 0 both halves
    fail at every F >= 3 (2.5 .. 7.2)."""
    win = _window(F)
    HM, bM = _full_rank_prior(win, asymmetric)
    w = _with_prior(win, HM, bM)
    g = binding.BA.from_window(win)
    g.set_prior(HM, bM)
    state_before = g.get_residuals()["state_state"].copy()
    kind = "asym" if asymmetric else "sym"
    worst = {}
    for idx in range(F):
        Hn, bn, block = _numpy(w, idx)
        assert np.linalg.cond(block) < 1e3, (F, idx, np.linalg.cond(block))
        Ho, bo = _oracle(w, idx)
        assert _dist(Ho, bo, Hn, bn) <= 1e-12, ("the two references disagree", F, idx)
        Hg, bg = g.marginalize_frame(idx)
        assert Hg.shape == (8 * (F - 1) + 4,) * 2 and bg.shape == (8 * (F - 1) + 4,)
        assert np.isfinite(Hg).all() and np.isfinite(bg).all()
        assert np.abs(Hg - Hg.T).max() <= 1e-9 * np.abs(Hg).max(), (F, idx)
        c = _index_class(F, idx)
        # blockrel compares 4 x 4 block by 4 x 4 block, every block of the random prior has its own values: a remaining frame that ended up in another
        # frame's rows / columns (the order of the others must not change, EnergyFunctional.cc:133) is an O(1) distance here, not a small one
        dn, do = _dist(Hg, bg, Hn, bn), _dist(Hg, bg, Ho, bo)
        assert dn <= 1e-9 and do <= 1e-9, ("frame blocks out of order or wrong arithmetic: block-by-block distance to numpy / oracle", F, idx, dn, do)
        worst[c] = max(worst.get(c, (0.0, 0.0))[0], dn), max(worst.get(c, (0.0, 0.0))[1], do)
        H2, b2 = g.marginalize_frame(idx)                                                   # the call reads the handle's prior and writes scratch only
        assert H2.tobytes() == Hg.tobytes() and b2.tobytes() == bg.tobytes(), ("two consecutive calls differ", F, idx)
    for c, (dn, do) in worst.items():
        observe("marg_frame_%s_F%d_%s_vs_numpy" % (kind, F, c), dn, 1e-9)                  # observed on MI355X <= 1.5e-14 (symmetric and asymmetric, every F)
        observe("marg_frame_%s_F%d_%s_vs_oracle" % (kind, F, c), do, 1e-9)                 # observed on MI355X <= 1.3e-14: the distance of the oracle from the numpy restatement
    assert np.array_equal(g.get_residuals()["state_state"], state_before), "the applied window state is untouched"
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("F", FRAME_COUNTS)
def test_marginalize_frame_rejects_indices_outside_the_window(F):
    win = _window(F)
    g = binding.BA.from_window(win)
    g.set_prior(*_full_rank_prior(win, False))
    for idx in (-1, F):
        with pytest.raises(binding.LdsoError):
            g.marginalize_frame(idx)
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("F,idx", [(5, 2), (9, 0), (9, 8), (16, 7)])
def test_marginalize_frame_leaves_the_system_scratch_reusable(F, idx):
    """k_marg_frame works in B.sys, the buffer of the step-wise system: a solve_system(0) after the call gives the bytes of a twin handle that never
    marginalised"""
    win = _window(F)
    HM, bM = _full_rank_prior(win, False)
    hs = []
    for marg in (True, False):
        g = binding.BA.from_window(win)
        g.set_prior(HM, bM)
        g.collect_active(); g.linearize_all(False); g.apply_res(); g.backup_state()
        if marg:
            g.marginalize_frame(idx)
        g.solve_system(0)
        hs.append(g)
    sa, sb = hs[0].get_system(), hs[1].get_system()
    for k in ("HFinal", "bFinal", "x"):
        assert np.isfinite(sa[k]).all() and sa[k].tobytes() == sb[k].tobytes(), k
    for g in hs:
        g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("F,idx", [(5, 0), (5, 2), (9, 8)])
def test_marginalize_frame_without_a_prior_eliminates_a_zero_H_M(F, idx):
    """hasPrior false: the elimination of an all-zero H_M plus the frame's prior.  The frame gets the full pose prior of frameID 0 (synth.frame_prior) where
    it has none of its own: with zeros on the pose diagonal the 8 x 8 block is singular and there is nothing to compare."""
    w = copy.deepcopy(_window(F))
    w.frames["prior"][idx] = synth.frame_prior(0, w.settings)
    assert not np.any(w.HM) and not np.any(w.bM)
    g = binding.BA.from_window(w)
    Hg, bg = g.marginalize_frame(idx)
    Hn, bn, block = _numpy(w, idx)
    assert np.linalg.cond(block) < 1e3
    assert Hg.shape == Hn.shape and np.array_equal(Hg, Hn) and np.array_equal(bg, bn)      # zeros off the eliminated block: nothing to round
    assert not np.any(Hg) and not np.any(bg)
    # ... and the same after a prior was set and cleared again (the handle zeroes H_M itself)
    g.set_prior(*_full_rank_prior(w, False))
    assert np.any(g.marginalize_frame(idx)[0])
    g.set_prior(None, None)
    Hg, bg = g.marginalize_frame(idx)
    assert not np.any(Hg) and not np.any(bg)
    g.close()
