"""GPU parity tests of the windowed BA hot path: libldso_hip.so (through the C-ABI) against the oracle on the
same seeded windows.  Tolerances (north_star): 1e-4 relative on energies and Hessian entries (entry tolerance
relative to the 4x4 block maximum), bit-exact on residual states / indices."""
import copy

import numpy as np
import pytest

from conftest import rel, blockrel, observe, get_window
from ldso_amd import synth, binding
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

TOL = 1e-4


def stage_compare(win, check_J=True):
    o = po.OracleWindow(win)
    g = binding.BA.from_window(win)
    # setPrecalcValues
    assert rel(g.get_precalc(), o.get_precalc()) < 1e-6
    o.collect_active(); g.collect_active()
    g.set_debug_dump(True)
    Eo, Eg = o.linearize_all(False), g.linearize_all(False)
    assert abs(Eo - Eg) <= TOL * abs(Eo)
    ro, rg = o.get_residuals(), g.get_residuals()
    lin = win.residuals["is_linearized"].astype(bool)       # linearised residuals are not part of activeResiduals
    assert np.array_equal(ro["out"]["state_NewState"][~lin], rg["out"]["state_NewState"][~lin])            # bit-exact states
    assert rel(rg["out"]["state_NewEnergy"][~lin], ro["out"]["state_NewEnergy"][~lin]) < 2e-5
    assert rel(g.get_frames()["frames"]["frameEnergyTH"], o.get_frames()["frames"]["frameEnergyTH"]) < 1e-6
    if check_J:
        Jg = g.get_jacobians()
        ok = (ro["out"]["state_NewState"] != 1) & ~lin
        for k in ("resF", "Jpdxi", "Jpdc", "Jpdd", "JIdx", "JabF", "JIdx2", "JabJIdx", "Jab2"):
            assert rel(Jg[k][ok], ro["J"][k][ok]) < 1e-5, k
    g.set_debug_dump(False)
    o.apply_res(); g.apply_res()
    ro, rg = o.get_residuals(), g.get_residuals()
    assert np.array_equal(ro["is_active"], rg["is_active"]) and np.array_equal(ro["state_state"], rg["state_state"])
    act = ro["is_active"].astype(bool)
    assert rel(rg["out"]["JpJdF"][act], ro["out"]["JpJdF"][act]) < 1e-5
    assert rel(rg["out"]["centerProjectedTo"][act & ~lin], ro["out"]["centerProjectedTo"][act & ~lin]) < 1e-6
    # solveSystem
    o.backup_state(); g.backup_state()
    o.solve_system(0); g.solve_system(0)
    so, sg = o.get_system(), g.get_system()
    for k in ("HA", "HL", "Hsc", "HFinal"):
        assert rel(sg[k], so[k]) < TOL, k
        assert blockrel(sg[k], so[k], 4) < TOL, k
        assert np.abs(sg[k] - sg[k].T).max() <= 1e-7 * np.abs(sg[k]).max(), k
    for k in ("bA", "bL", "bsc", "bFinal"):
        assert rel(sg[k], so[k]) < TOL, k
    assert np.linalg.norm(sg["HFinal"] @ sg["x"] - sg["bFinal"]) / np.linalg.norm(sg["bFinal"]) < 1e-8     # backward error
    # x itself is only determined up to the weakly constrained gauge directions (cond ~1e5 after scaling: two fp64 solvers agree on it
    # to ~1e-3).  What must agree tightly: the GPU's x solves the ORACLE's system, reaches the oracle's model decrease, and lies within
    # 1e-5 of the oracle's x in the energy norm of that system
    Ho, bo, xo, xg = so["HFinal"], so["bFinal"], so["x"], sg["x"]
    assert np.linalg.norm(Ho @ xg - bo) / np.linalg.norm(bo) < 1e-6
    dec = lambda x: float(x @ bo - 0.5 * x @ Ho @ x)
    assert abs(dec(xg) - dec(xo)) <= 1e-9 * abs(dec(xo))
    d = xg - xo
    assert np.sqrt(abs(d @ Ho @ d)) <= 1e-5 * np.sqrt(abs(xo @ Ho @ xo))
    assert rel(sg["x"], so["x"]) < 5e-2                                                                       # gauge-limited (loose by nature)
    assert o.counts()[:2] == g.get_counts()
    pto, _ = o.get_points(); ptg = g.get_points()
    for k in ("HdiF", "bdSumF", "idepth_hessian", "Hdd_accAF", "bd_accAF", "Hcd_accAF", "Hdd_accLF", "bd_accLF", "Hcd_accLF"):
        assert rel(ptg[k], pto[k]) < 1e-5, k
    # doStepFromBackup + relinearise
    cbo, cbg = o.do_step(), g.do_step()
    assert cbo == cbg
    fo, fg = o.get_frames(), g.get_frames()
    assert rel(fg["step"], fo["step"]) < 5e-2                       # the frame part of -x: gauge-limited like x
    Eo, Eg = o.linearize_all(False), g.linearize_all(False)
    observe("stage_relinearise_energy", abs(Eo - Eg) / abs(Eo), TOL)          # two solvers, one step apart along the gauge: observed 9.5e-5 (round 4)
    # ... and without the solvers' drift: the oracle moved to the GPU's own stepped state re-linearises to the GPU's energy
    from test_fullsize_gpu import _transplant
    ot = po.OracleWindow(_transplant(win, g)); ot.collect_active(reset_oob=False)
    observe("stage_relinearise_energy_at_gpu_state", abs(ot.linearize_all(False) - Eg) / abs(Eg), 1e-6)
    return o, g


def _gauge_basis(frames):
    """The 7 gauge directions (6 pose + scale) in the 8-per-frame state, as FullSystem::getNullspaces assembles them (FullSystem.cc:1711-1760)."""
    N = np.zeros((8 * len(frames), 7))
    for f in range(len(frames)):
        N[8 * f:8 * f + 6, :6] = frames["nullspaces_pose"][f].reshape(6, 6)
        N[8 * f:8 * f + 6, 6] = frames["nullspaces_scale"][f]
        N[8 * f:8 * f + 3, :] *= 2.0                                                     # SCALE_XI_TRANS_INVERSE
    return N


def test_stagewise_tiny(tiny):
    stage_compare(tiny)


def test_stagewise_small(small):
    stage_compare(small)


def test_stagewise_mixed_linearized(small):
    """20..50 % of the residuals pre-linearised: exercises addPoint<1> (res_toZeroF + J*delta) and H_L."""
    w2 = po.make_mixed_window(small)
    assert 0 < w2.residuals["is_linearized"].sum() < w2.R
    o, g = stage_compare(w2, check_J=False)
    a, l = g.get_counts()
    assert a > 0 and l > 0


def test_optimize_small(small):
    o = po.OracleWindow(small); o.set_force_all_iterations(True)
    g = binding.BA.from_window(small)
    rmo = o.optimize(6)
    rmg, its = g.optimize(6, force_all=True)
    assert its == 6 and abs(rmo - rmg) <= TOL * rmo
    eo, eg = o.energy_log(), g.get_energy_log()
    assert len(eo) == len(eg) == 8
    observe("optimize6_energy_log", rel(eg, eo), TOL)      # observed 2.6e-5
    ro, rg = o.get_residuals(), g.get_residuals()
    assert np.array_equal(ro["state_state"], rg["state_state"]) and np.array_equal(ro["is_active"], rg["is_active"])
    assert np.array_equal(rg["to_remove"].astype(bool), ro["alive"] == 0)
    pto, _ = o.get_points(); ptg = g.get_points()
    assert np.array_equal(pto["numGoodResiduals"], ptg["numGoodResiduals"])
    assert rel(ptg["idepth"], pto["idepth"]) < 5e-3 and rel(ptg["maxRelBaseline"], pto["maxRelBaseline"]) < 1e-3
    fo, fg = o.get_frames(), g.get_frames()
    assert rel(fg["frames"]["worldToCam_evalPT"], fo["frames"]["worldToCam_evalPT"]) < 1e-3     # re-anchored newest frame
    assert np.array_equal(fg["frames"]["state_zero"][-1][:6], np.zeros(6))
    assert rel(fg["frames"]["nullspaces_pose"][-1], fo["frames"]["nullspaces_pose"][-1]) < 1e-3


def test_get_results_equals_the_three_getters(small):
    """ldso_ba_get_results (one synchronisation, the drop-in's write-back) against ldso_ba_get_residuals / _points / _frames: the same bytes - after an optimize()
    and with a linearisation pending (the "new" values then come from the other residual set)."""
    g = binding.BA.from_window(small)

    def same():
        r, p, f = g.get_residuals(), g.get_points(), g.get_frames()
        a = g.get_results()
        for k in ("out", "state_state", "is_active", "to_remove"):
            assert a["residuals"][k].tobytes() == r[k].tobytes(), k
        assert a["points"].tobytes() == p.tobytes()
        for k in ("frames", "step", "calib_value", "calib_step"):
            assert a["frames"][k].tobytes() == f[k].tobytes(), k

    g.optimize(3, force_all=True)
    same()
    g.linearize_all(False)                                  # pending: not applied
    same()


def test_optimize_canbreak_path(small):
    """un-forced optimize: the host reads `canbreak` every iteration like the reference loop (FullSystem.cc:829)."""
    o = po.OracleWindow(small)
    g = binding.BA.from_window(small)
    rmo = o.optimize(6)
    rmg, its = g.optimize(6, force_all=False)
    assert its == len(o.energy_log()) - 2
    observe("optimize_rmse", abs(rmo - rmg) / rmo, TOL)      # observed 7.5e-6


@pytest.mark.parametrize("F,P", [(12, 500), (3, 300), (2, 200)])
def test_optimize_canbreak_other_window_shapes(F, P):
    """The device-side loop end (host-mapped stop word) on the split-launch path (F = 12: k_reduce | k_gn_solve | k_linearize) and on the
    small windows whose iteration budget the reference changes (FullSystem.cc:729-731: F < 3 -> 20, F < 4 -> 15)."""
    win = synth.make_window(F=F, P=P, w=320, h=240, fx=200.0, seed=7 + F)
    o = po.OracleWindow(win)
    g = binding.BA.from_window(win)
    rmo = o.optimize(6)
    rmg, its = g.optimize(6, force_all=False)
    assert its == len(o.energy_log()) - 2
    observe("optimize_rmse", abs(rmo - rmg) / rmo, TOL)      # observed 7.5e-6
    observe("optimize_energy_log_b", rel(g.get_energy_log(), o.energy_log()), TOL)      # observed 4.3e-5
    # and once more on the same handle: the stop word is re-armed per call
    rmg2, its2 = g.optimize(6, force_all=False)
    assert its2 >= 1 and np.isfinite(rmg2)


def _optimize_compare(win, its=5, tol_e=TOL):          # observed <= 1.2e-5 (round 4)
    o = po.OracleWindow(win); o.set_force_all_iterations(True)
    g = binding.BA.from_window(win)
    rmo = o.optimize(its)
    rmg, n_its = g.optimize(its, force_all=True)
    assert n_its == its
    observe(f"optimize_compare_rmse_F{win.F}_P{win.P}", abs(rmo - rmg) / rmo, tol_e)
    eo, eg = o.energy_log(), g.get_energy_log()
    assert len(eo) == len(eg) == its + 2
    observe(f"optimize_compare_energy_log_F{win.F}_P{win.P}", rel(eg, eo), tol_e)
    ro, rg = o.get_residuals(), g.get_residuals()
    mism = (ro["state_state"] != rg["state_state"]).sum()
    assert mism <= 2e-3 * len(ro["state_state"])          # a few threshold-borderline residuals may flip after several GN steps
    fo, fg = o.get_frames(), g.get_frames()
    assert rel(fg["frames"]["state"], fo["frames"]["state"]) < 5e-3
    # off the gauge directions (6 pose + scale: the weakly constrained part of the system) the states agree an order of magnitude tighter
    xs_o, xs_g = fo["frames"]["state"][:-1, :8].reshape(-1), fg["frames"]["state"][:-1, :8].reshape(-1)      # the newest frame was re-anchored
    Q, _ = np.linalg.qr(_gauge_basis(fo["frames"][:-1]))
    d = xs_g - xs_o
    assert np.abs(d - Q @ (Q.T @ d)).max() < 5e-4 * np.abs(xs_o).max()
    return o, g


def test_optimize_mixed_linearized(small):
    """GN fast path (k_reduce atomics -> k_gn_solve -> fused k_linearize) with linearised residuals (H_L, b_L)."""
    w2 = po.make_mixed_window(small)
    # one iteration: with a third of the residuals frozen at a perturbed linearisation point the forced-accept GN sequence of this
    # synthetic window overshoots from the second step on (energy x15), and float-level differences (summation order) are
    # amplified beyond any fixed tolerance; the first step is what pins H_L / b_L on the fast path.
    _, g = _optimize_compare(w2, its=1)
    a, l = g.get_counts()
    assert a > 0 and l > 0


def test_optimize_convergent_mixed_window_five_iterations(small):
    """The H_L / b_L fast path over several iterations: a window whose linearised residuals were fixed at a CONVERGED state
    (po.make_convergent_mixed_window) - the forced-accept sequence stays put, so the per-iteration energies, the residual states and
    the frame states can be held to the same tolerances as a window without linearised residuals."""
    w2 = po.make_convergent_mixed_window(small)
    assert w2.residuals["is_linearized"].sum() > 100
    o, g = _optimize_compare(w2, its=5)
    a, l = g.get_counts()
    assert a > 0 and l > 0 and (a, l) == o.counts()[:2]
    eo = o.energy_log()
    assert eo[1:].max() < 1.05 * eo[0], "the window is meant to be convergent"


def test_optimize_with_marginalization_prior(small):
    """H_M / b_M present: bFinal picks up b_M + H_M delta every iteration (EnergyFunctional.cc:279).  The prior is a
    synthetic symmetric PSD matrix (both sides get the same one)."""
    w1 = synth.add_synthetic_prior(copy.deepcopy(small))
    assert np.abs(w1.HM).max() > 0 and np.abs(w1.bM).max() > 0
    _optimize_compare(w1)
    g = binding.BA.from_window(w1); o = po.OracleWindow(w1)
    o.collect_active(); g.collect_active(); o.linearize_all(False); g.linearize_all(False)
    o.apply_res(); g.apply_res(); o.backup_state(); g.backup_state(); o.solve_system(0); g.solve_system(0)
    so, sg = o.get_system(), g.get_system()
    assert blockrel(sg["HFinal"], so["HFinal"], 4) < TOL and rel(sg["bFinal"], so["bFinal"]) < TOL


def test_optimize_12_frames():
    """F = 12 > 8: two slot groups per point (NSG = 2), FS = 16, 9x9 Schur tiles, 7x16 padded LDL^T."""
    win = synth.make_window(F=12, P=500, w=320, h=240, fx=200.0, seed=5)
    assert win.F == 12
    o = po.OracleWindow(win); g = binding.BA.from_window(win)
    o.collect_active(); g.collect_active()
    Eo, Eg = o.linearize_all(False), g.linearize_all(False)
    assert abs(Eo - Eg) <= TOL * Eo
    assert np.array_equal(o.get_residuals(False)["out"]["state_NewState"], g.get_residuals()["out"]["state_NewState"])
    o.apply_res(); g.apply_res(); o.backup_state(); g.backup_state(); o.solve_system(0); g.solve_system(0)
    so, sg = o.get_system(), g.get_system()
    for k in ("HA", "Hsc", "HFinal"):
        assert blockrel(sg[k], so[k], 4) < TOL, k
    assert np.linalg.norm(sg["HFinal"] @ sg["x"] - sg["bFinal"]) / np.linalg.norm(sg["bFinal"]) < 1e-8
    _optimize_compare(win, its=4)


@pytest.mark.parametrize("with_prior", [False, True])
def test_marginalize_points(small, with_prior):
    _marginalize_points(small, with_prior, 0)


@pytest.mark.parametrize("marg", [2, -2], ids=["2", "F-2"])
@pytest.mark.parametrize("with_prior", [False, True])
def test_marginalize_points_of_a_middle_frame(small, with_prior, marg):
    _marginalize_points(small, with_prior, marg)


def _marginalize_points(small, with_prior, marg):
    """a11: marginalizePointsF on the device (mode-2 accumulate of the flagged points incl. the re-linearise + fixLinearizationF
    pass of flagPointsForRemoval) against the oracle's flagPointsForRemoval + marginalizePointsF: the new H_M / b_M.  Then marginalizeFrame of
    the flagged frame `marg` (negative: counted from the newest) - the oldest, a middle one, the last but one (FullSystem::flagFramesForMarginalization,
    FullSystem.cc:647-720, picks middle frames as its normal case)."""
    win = synth.add_synthetic_prior(copy.deepcopy(small)) if with_prior else small
    idx = marg if marg >= 0 else win.F + marg
    assert 0 <= idx < win.F
    o = po.OracleWindow(win); o.set_force_all_iterations(True)
    o.optimize(3)
    # the device handle starts from the oracle's post-optimize state (identical applied state on both sides)
    ex, fo = o.export_window(), o.get_frames()
    assert ex["F"] == win.F and len(ex["points"]) == win.P and np.array_equal(ex["orig_point"], np.arange(win.P))
    w2 = copy.deepcopy(win)
    w2.points, w2.residuals, w2.lin_J, w2.lin_res_toZeroF = ex["points"], ex["residuals"], ex["lin_J"], ex["lin_res_toZeroF"]
    w2.frames = fo["frames"]
    w2.calib = w2.calib.copy(); w2.calib["value"] = fo["calib_value"]
    g = binding.BA.from_window(w2)
    o.flag_frame(idx)
    o.flag_points_for_removal()
    _, status = o.get_points()
    flags = (status == 3).astype(np.int32)                  # PS_MARGINALIZED
    assert 0 < flags.sum() < win.P
    o.drop_points()
    o.marginalize_points()
    HMo, bMo = o.get_prior()
    HMg, bMg = g.marginalize_points(flags)
    assert np.abs(HMo).max() > 0
    assert blockrel(HMg, HMo, 4) < TOL and rel(HMg, HMo) < TOL
    assert rel(bMg, bMo) < TOL
    assert np.abs(HMg - HMg.T).max() <= 1e-6 * np.abs(HMg).max()
    # the applied window state is untouched by the call
    rg = g.get_residuals()
    assert np.array_equal(rg["state_state"], ex["residuals"]["state_state"])
    # marginalizeFrame on the resulting prior (the flagged frame)
    o.marginalize_frame(idx)
    HM2o, bM2o = o.get_prior()
    HM2g, bM2g = g.marginalize_frame(idx)
    assert HM2g.shape == HM2o.shape == (8 * (win.F - 1) + 4,) * 2
    # marginalizeFrame is fp64 on both sides: what separates HM2g from HM2o is the fp32 difference of their inputs (HMg vs HMo, within TOL above) pushed through the
    # inverse of the frame's 8 x 8 block - measured apart (tests/test_fullsize_gpu.py::test_c5_end_to_end has the same three steps at C5):
    g.set_prior(HMo, bMo)                                   # (i) the device on the oracle's prior = the oracle's result
    HM2i, bM2i = g.marginalize_frame(idx)
    observe("marginalize_frame_same_input", max(blockrel(HM2i, HM2o, 4), rel(bM2i, bM2o)), 1e-9)
    w2b = copy.deepcopy(w2); w2b.HM, w2b.bM = HMg, bMg      # (ii) the oracle on the device's prior = the device's result
    ob = po.OracleWindow(w2b); ob.marginalize_frame(idx)
    HM2b, bM2b = ob.get_prior(); ob.close()
    observe("marginalize_frame_device_input", max(blockrel(HM2g, HM2b, 4), rel(bM2g, bM2b)), 1e-9)
    sens_H, sens_b = blockrel(HM2b, HM2o, 4), rel(bM2b, bM2o)          # (iii) the chained difference = the oracle's own sensitivity to the input difference
    assert blockrel(HM2g, HM2o, 4) <= 1.01 * sens_H + 1e-8 and rel(bM2g, bM2o) <= 1.01 * sens_b + 1e-8, (blockrel(HM2g, HM2o, 4), sens_H, rel(bM2g, bM2o), sens_b)
    assert np.abs(HM2g - HM2g.T).max() <= 1e-9 * np.abs(HM2g).max()


@pytest.mark.parametrize("F,P", [(2, 37), (3, 50), (7, 113), (8, 130), (9, 131), (13, 101), (14, 103), (16, 97)])
def test_window_shape_boundaries(F, P):
    """Frame counts at the layout boundaries (F = 2 minimum, F = 8 fills one slot group exactly, F = 9 needs the second one, F = 16
    = LDSO_MAX_FRAMES with the 144-padded LDL^T; F = 7 | 8 and F = 13 | 14 are the two sides of each switch of the factorisation, and with it of the
    solve kernels' LDS layout: n + 1 = 61 | 69 around 64, 109 | 117 around 112) and point counts that are not multiples of the chunk size: one stage-wise pass
    and two fast-path iterations against the oracle."""
    win = synth.make_window(F=F, P=P, w=256, h=192, fx=160.0, seed=100 + F)
    o = po.OracleWindow(win); g = binding.BA.from_window(win)
    o.collect_active(); g.collect_active()
    Eo, Eg = o.linearize_all(False), g.linearize_all(False)
    assert abs(Eo - Eg) <= TOL * Eo
    assert np.array_equal(o.get_residuals(False)["out"]["state_NewState"], g.get_residuals()["out"]["state_NewState"])
    o.apply_res(); g.apply_res(); o.backup_state(); g.backup_state(); o.solve_system(0); g.solve_system(0)
    so, sg = o.get_system(), g.get_system()
    for k in ("HA", "Hsc", "HFinal"):
        assert blockrel(sg[k], so[k], 4) < TOL, k
    assert np.linalg.norm(sg["HFinal"] @ sg["x"] - sg["bFinal"]) / np.linalg.norm(sg["bFinal"]) < 1e-8
    o2 = po.OracleWindow(win); o2.set_force_all_iterations(True)
    g2 = binding.BA.from_window(win)
    rmo = o2.optimize(2); rmg, its = g2.optimize(2, force_all=True)
    tol = 5e-3 if F == 2 else 5 * TOL          # two frames: the gauge (scale) is barely constrained, the solvers agree less
    assert its == 2 and abs(rmo - rmg) <= tol * rmo
    assert rel(g2.get_energy_log(), o2.energy_log()) < tol


@pytest.mark.parametrize("F,P,per_wave", [(5, 2600, "2 points in four wavefronts, 1 in the others"), (7, 5700, "3 points per wavefront, ragged last chunk"), (8, 9000, "4-5 points per wavefront")])
def test_pipelined_point_loop_of_the_single_window_kernel(F, P, per_wave):
    """k_linearize_one<1> above 8 points per chunk: the software pipeline with the point's records parked in LDS and the first point peeled off the loop (round 6) - chunk
    sizes that leave the wavefronts of a workgroup with DIFFERENT numbers of points (a wavefront with one point runs the peeled iteration only).  One stage-wise pass and
    three fast-path iterations against the oracle: energies 1e-4, residual states bit for bit.  (Round 6: a bit-cast on a vector element made this loop read every residual's
    is-linearised flag as its index - energies 0; the full-size C4 test was the only one with more than 8 points per chunk.)"""
    win = synth.make_window(F=F, P=P, w=320, h=240, fx=200.0, seed=600 + F)
    o = po.OracleWindow(win); g = binding.BA.from_window(win)
    cuts = np.asarray(g.get_chunk_cuts())
    sizes = np.diff(np.concatenate([[0], cuts]))
    assert sizes.max() > 8, (per_wave, sizes.max())
    o.collect_active(); g.collect_active()
    Eo, Eg = o.linearize_all(False), g.linearize_all(False)
    assert abs(Eo - Eg) <= TOL * Eo
    assert np.array_equal(o.get_residuals(False)["out"]["state_NewState"], g.get_residuals()["out"]["state_NewState"])
    o.close(); g.close()
    o2 = po.OracleWindow(win); o2.set_force_all_iterations(True)
    g2 = binding.BA.from_window(win)
    rmo = o2.optimize(3); rmg, its = g2.optimize(3, force_all=True)
    assert its == 3 and abs(rmo - rmg) <= 5 * TOL * rmo
    assert rel(g2.get_energy_log(), o2.energy_log()) < 5 * TOL
    o2.close(); g2.close()


@pytest.mark.parametrize("name", ["C3", "C4"])
def test_full_size_parity_and_properties(name):
    """BASELINE configs at full size: one stage-wise pass against the oracle plus size-independent properties."""
    win = get_window(name)
    o = po.OracleWindow(win); g = binding.BA.from_window(win)
    o.collect_active(); g.collect_active()
    Eo, Eg = o.linearize_all(False), g.linearize_all(False)
    assert abs(Eo - Eg) <= TOL * Eo
    assert np.array_equal(o.get_residuals(False)["out"]["state_NewState"], g.get_residuals()["out"]["state_NewState"])
    o.apply_res(); g.apply_res(); o.backup_state(); g.backup_state(); o.solve_system(0); g.solve_system(0)
    so, sg = o.get_system(), g.get_system()
    for k in ("HA", "Hsc"):
        assert blockrel(sg[k], so[k], 4) < TOL, k
        # symmetry + positive semi-definiteness of the accumulated blocks
        assert np.abs(sg[k] - sg[k].T).max() <= 1e-7 * np.abs(sg[k]).max()
        assert np.linalg.eigvalsh(0.5 * (sg[k] + sg[k].T)).min() > -1e-6 * np.abs(sg[k]).max()
    # H_A - H_sc (the reduced camera system) must be PSD as a Schur complement
    red = sg["HA"] - sg["Hsc"]
    assert np.linalg.eigvalsh(0.5 * (red + red.T)).min() > -1e-6 * np.abs(red).max()


def test_shard_and_sum_invariance(small):
    """points sharded over two 'ranks' on one GPU: the summed reduce buffers equal the unsharded one (the
    multi-GPU all-reduce is a plain sum of these buffers)."""
    import torch
    ts = torch.cuda.Stream(); torch.cuda.set_stream(ts)          # one non-default stream for torch and the handles
    g = binding.BA.from_window(small)
    g.collect_active(); g.linearize_all(False); g.apply_res()
    nd = g.reduce_doubles()
    full = torch.zeros(nd, dtype=torch.float64, device="cuda")
    g.set_stream(torch.cuda.current_stream().cuda_stream)
    g.reduce_local(full.data_ptr()); torch.cuda.synchronize()
    parts = []
    half = small.P // 2
    for (a, b) in ((0, half), (half, small.P)):
        gi = binding.BA.from_window(small)
        gi.set_stream(torch.cuda.current_stream().cuda_stream)
        gi.set_shard(a, b)
        gi.collect_active(); gi.linearize_all(False); gi.apply_res()
        buf = torch.zeros(nd, dtype=torch.float64, device="cuda")
        gi.reduce_local(buf.data_ptr()); torch.cuda.synchronize()
        parts.append(buf)
    s = (parts[0] + parts[1]).cpu().numpy()
    f = full.cpu().numpy()
    n = 8 * small.F + 4
    blk = n * n + n
    assert blockrel(s[:n * n].reshape(n, n), f[:n * n].reshape(n, n), 4) < 1e-5          # H_A
    assert blockrel(s[2 * blk:2 * blk + n * n].reshape(n, n), f[2 * blk:2 * blk + n * n].reshape(n, n), 4) < 1e-5   # H_sc
    assert rel(s[3 * blk:3 * blk + 3], f[3 * blk:3 * blk + 3]) < 1e-9                     # energy, counters
    assert np.array_equal(s[3 * blk + 8:], f[3 * blk + 8:])                               # energy candidates: exact


@pytest.mark.parametrize("with_prior", [False, True])
def test_two_rank_fast_path_equals_single_gpu(small, with_prior):
    """Multi-GPU fast path on one GPU: two handles own the two halves of the points; per iteration their accumulator buffers are
    summed (what the RCCL all-reduce does) and both run the replicated solve.  After 4 iterations every 'rank' holds the state of
    the unsharded 3-launch path."""
    import torch
    win = synth.add_synthetic_prior(copy.deepcopy(small)) if with_prior else small
    ts = torch.cuda.Stream(); torch.cuda.set_stream(ts)          # one non-default stream for torch and the handles
    st = ts.cuda_stream
    ref = binding.BA.from_window(win, stream=st)
    ref.collect_active(); ref.linearize_all(False); ref.apply_res()
    ref.enqueue_gn(0, 4); ref.sync()
    half = win.P // 2
    ranks, bufs = [], []
    for (a, b) in ((0, half), (half, win.P)):
        g = binding.BA.from_window(win, stream=st)
        g.set_shard(a, b)
        g.collect_active(); g.linearize_all(False); g.apply_res()
        ranks.append(g); bufs.append(torch.zeros(g.gn_reduce_doubles(), dtype=torch.float64, device="cuda"))
    for it in range(4):
        for g, b in zip(ranks, bufs):
            g.gn_reduce_local(b.data_ptr(), 1e-1)
        tot = bufs[0] + bufs[1]
        for g, b in zip(ranks, bufs):
            b.copy_(tot)
            g.gn_solve_reduced(b.data_ptr(), it, 1e-1)
    torch.cuda.synchronize()
    # Tolerances: the fp32 partial sums (chunk / K-split boundaries differ between the sharded and the unsharded run) perturb the
    # reduced system at 1e-7, the gauge-ill-conditioned solve amplifies that to ~2e-3 in the state (same band as GPU vs oracle);
    # the energy of the next linearizeAll is insensitive to it.
    fr = ref.get_frames()
    for g in ranks:
        fg = g.get_frames()
        assert rel(fg["frames"]["state"], fr["frames"]["state"]) < 5e-3
        assert rel(fg["frames"]["frameEnergyTH"], fr["frames"]["frameEnergyTH"]) < 1e-3
    idr = ref.get_points()["idepth"]
    assert rel(ranks[0].get_points()["idepth"][:half], idr[:half]) < 5e-3 and rel(ranks[1].get_points()["idepth"][half:], idr[half:]) < 5e-3
    rb = torch.zeros(ref.gn_reduce_doubles(), dtype=torch.float64, device="cuda")
    ref.gn_reduce_local(rb.data_ptr(), 1e-1)
    for g, b in zip(ranks, bufs):
        g.gn_reduce_local(b.data_ptr(), 1e-1)
    torch.cuda.synchronize()
    n = 8 * win.F + 4
    blk = n * n + n
    tot, r = (bufs[0] + bufs[1]).cpu().numpy(), rb.cpu().numpy()
    assert abs(tot[blk] - r[blk]) <= 1e-4 * r[blk]                                   # energy after 4 iterations
    assert (tot[blk + 8:] > 0).sum() == (r[blk + 8:] > 0).sum()                      # same set size of newest-frame candidates
    assert blockrel(np.tril(tot[:n * n].reshape(n, n)), np.tril(r[:n * n].reshape(n, n)), 4) < 5e-3


@pytest.mark.parametrize("name", ["small", "C3"])
def test_fused_launch_stress(name):
    """the fused k_reduce_solve launch hands HFinal / bFinal from the reduce workgroups to the control workgroup inside
    one launch (device counter).  Many optimize() calls, alternating forced / un-forced: every fused run must reproduce the split
    schedule (k_reduce -> k_gn_solve as two launches, ordered by the kernel boundary) — a lost signal or a stale read shows up as
    a different energy log.  The fp64 atomics only reorder sums, hence 1e-12 instead of bit equality."""
    win = synth.add_synthetic_prior(copy.deepcopy(get_window(name)))
    ref = {}
    for force in (True, False):
        g = binding.BA.from_window(win)
        g.set_debug_split_launch(True)
        rm, its = g.optimize(6, force_all=force)
        ref[force] = (np.array(g.get_energy_log()), g.get_frames()["frames"]["state"].copy(), its)
    g = binding.BA.from_window(win)
    for r in range(40):
        force = (r % 2 == 0)
        g.load_window(win)
        rm, its = g.optimize(6, force_all=force)
        el, st = np.array(g.get_energy_log()), g.get_frames()["frames"]["state"]
        assert its == ref[force][2], (r, its)
        assert rel(el, ref[force][0]) < 1e-12, (r, el, ref[force][0])
        assert np.abs(st - ref[force][1]).max() < 1e-9, r


def test_sharded_handle_rejects_single_gpu_entry_points(small):
    """a handle that owns only a shard of the points must not run the unsharded solve silently."""
    g = binding.BA.from_window(small)
    g.set_shard(0, small.P // 2)
    g.collect_active(); g.linearize_all(False); g.apply_res()
    for call in (lambda: g.optimize(2, force_all=True), lambda: g.enqueue_gn(0, 1), lambda: g.solve_system(0)):
        with pytest.raises(binding.LdsoError) as e:
            call()
        assert e.value.code == -1 or "sharded" in str(e.value)
    g.set_shard(0, small.P)
    g.solve_system(0)


def test_prior_survives_set_frames(small):
    """ldso_ba_set_prior before ldso_ba_set_frames must not lose the prior (set_window resets it, set_frames does not)."""
    w1 = synth.add_synthetic_prior(copy.deepcopy(small))
    a = binding.BA.from_window(w1)
    b = binding.BA(w1.w, w1.h, w1.F, w1.P)
    b.set_settings(w1.settings)
    for f in range(w1.F):
        b.set_image(f, w1.images[f][0])
    b.set_window(np.arange(w1.F), w1.points, w1.residuals, w1.lin_J, w1.lin_res_toZeroF)
    b.set_prior(w1.HM, w1.bM)
    b.set_frames(w1.frames, w1.calib)
    ra, _ = a.optimize(3, force_all=True); rb, _ = b.optimize(3, force_all=True)
    assert ra == rb and rel(b.get_energy_log(), a.get_energy_log()) < 1e-12
    c = binding.BA.from_window(small)
    rc, _ = c.optimize(3, force_all=True)
    assert rc != ra                                                # the prior matters on this window


def test_large_batch_is_rechunked_and_equals_solo_runs_under_the_same_chunking():
    """A batch big enough to fill the chip several times over (12 windows x 1600 points): ldso_ba_batch_create gives its windows fatter
    workgroups (several points per wavefront); a handle run alone with the SAME chunking (ldso_ba_set_chunk_points) ends in the same state
    to the last bits the fp64 atomics allow - the chunking decides only where the fp32 partial sums of the top Hessian are cut."""
    import torch
    ts = torch.cuda.Stream(); torch.cuda.set_stream(ts)
    st = ts.cuda_stream
    wins = [synth.add_synthetic_prior(synth.make_window(F=7, P=1750, w=320, h=240, fx=200.0, seed=60 + i)) for i in range(12)]
    batch = []
    for w in wins:
        g = binding.BA.from_window(w, stream=st); g.collect_active(); g.linearize_all(False); g.apply_res(); batch.append(g)
    b = binding.BABatch(batch)
    ch = b.chunk_points()
    assert ch >= 16, ch                                          # (the average: since round 6 the batch cuts its windows unevenly, one equal workload per workgroup)
    cuts = [g.get_chunk_cuts() for g in batch]
    assert all(c[-1] == 1750 and np.all(np.diff(c) > 0) for c in cuts)
    assert len(set(len(c) for c in cuts)) > 1 or len(set(tuple(c) for c in cuts)) > 1, "windows at different places of the launch are cut differently"
    b.enqueue_gn(0, 4); b.sync(); torch.cuda.synchronize()
    for i in (0, 5, 11):
        g = binding.BA.from_window(wins[i], stream=st); g.set_chunk_cuts(cuts[i]); g.set_reduce_splits(b.reduce_splits())
        assert np.array_equal(g.get_chunk_cuts(), cuts[i])
        g.collect_active(); g.linearize_all(False); g.apply_res()
        g.set_debug_split_launch(True); g.enqueue_gn(0, 4); g.sync(); torch.cuda.synchronize()
        fs, fb = g.get_frames(), batch[i].get_frames()
        assert np.abs(fb["frames"]["state"] - fs["frames"]["state"]).max() <= 1e-9 * np.abs(fs["frames"]["state"]).max()
        assert np.array_equal(fb["frames"]["frameEnergyTH"], fs["frames"]["frameEnergyTH"])
        rs, rb = g.get_residuals(), batch[i].get_residuals()
        assert np.array_equal(rs["state_state"], rb["state_state"]) and rel(rb["out"]["state_NewEnergy"], rs["out"]["state_NewEnergy"]) < 1e-5
        # and against the oracle (default chunking is irrelevant there): energies 1e-4
        if i == 0:
            o = po.OracleWindow(wins[i]); o.collect_active(); o.linearize_all(False); o.apply_res()
            for it in range(4):
                o.backup_state(); o.solve_system(it); o.do_step(); o.linearize_all(False); o.apply_res()
            Eo = o.get_residuals(False)["out"]["state_NewEnergy"].astype(np.float64).sum()
            Eg = rb["out"]["state_NewEnergy"].astype(np.float64).sum()
            assert abs(Eg - Eo) <= 1e-4 * Eo
        g.close()
    b.close()
    assert batch[0].get_chunk_points() == (0, batch[0].get_chunk_points()[1])          # back to the single-window chunking
    for g in batch:
        g.close()


def test_batched_windows_equal_individual_runs():
    """ldso_ba_batch_*: six independent windows (different scenes, point counts and frame counts <= 8, one with a prior; the window of 8 key frames sizes the
    control step's LDS for the whole batch and lays itself out for the 112 x 112 factorisation, the others for the 64 x 64 one) iterated by
    three launches per iteration for the whole batch; every window must end where its own ldso_ba_enqueue_gn (split schedule) ends."""
    import torch
    ts = torch.cuda.Stream(); torch.cuda.set_stream(ts)
    st = ts.cuda_stream
    wins = [synth.make_window(F=5, P=400, w=320, h=240, fx=200.0, seed=31), synth.make_window(F=5, P=333, w=320, h=240, fx=200.0, seed=32),
            synth.make_window(F=7, P=500, w=320, h=240, fx=200.0, seed=33), synth.make_window(F=4, P=150, w=256, h=192, fx=160.0, seed=34),
            synth.add_synthetic_prior(synth.make_window(F=6, P=420, w=320, h=240, fx=200.0, seed=35)), synth.make_window(F=8, P=260, w=320, h=240, fx=200.0, seed=37)]
    solo, batch = [], []
    for w in wins:
        for lst in (solo, batch):
            g = binding.BA.from_window(w, stream=st)
            g.collect_active(); g.linearize_all(False); g.apply_res()
            lst.append(g)
    b = binding.BABatch(batch)
    for g in solo:
        g.set_debug_split_launch(True)
        g.set_reduce_splits(b.reduce_splits())          # the fp32 partial tiles of the Schur complement are formed per K-split: a batch of >= 4 windows uses 4, a lone window 8
        g.enqueue_gn(0, 5)
    b.enqueue_gn(0, 3); b.enqueue_gn(3, 2)
    b.sync(); torch.cuda.synchronize()
    for w, gs, gb in zip(wins, solo, batch):
        fs, fb = gs.get_frames(), gb.get_frames()
        assert np.abs(fb["frames"]["state"] - fs["frames"]["state"]).max() <= 1e-9 * np.abs(fs["frames"]["state"]).max()
        assert np.array_equal(fb["frames"]["frameEnergyTH"], fs["frames"]["frameEnergyTH"])
        ps, pb = gs.get_points(), gb.get_points()
        assert rel(pb["idepth"], ps["idepth"]) < 1e-6 and rel(pb["HdiF"], ps["HdiF"]) < 1e-5
        rs, rb = gs.get_residuals(), gb.get_residuals()
        assert np.array_equal(rs["state_state"], rb["state_state"]) and rel(rb["out"]["state_NewEnergy"], rs["out"]["state_NewEnergy"]) < 1e-5
    # and against the oracle: the batch is the reference's loop on every window
    for w, gb in zip(wins[:2], batch[:2]):
        o = po.OracleWindow(w)
        o.collect_active(); o.linearize_all(False); o.apply_res()
        E = 0.0
        for it in range(5):
            o.backup_state(); o.solve_system(it); o.do_step(); E = o.linearize_all(False); o.apply_res()
        Eg = gb.get_residuals()["out"]["state_NewEnergy"].astype(np.float64)
        ro = o.get_residuals(False)
        Eo = ro["out"]["state_NewEnergy"].astype(np.float64)
        assert abs(Eg.sum() - Eo.sum()) <= 1e-4 * Eo.sum()
    b.close()


def test_lm_energies_and_rejection_path(small):
    """setting_forceAceptStep = false (FullSystem.cc:805-826): calcMEnergyF / calcLEnergyF_MT on the device, and ldso_ba_optimize
    accepting / rejecting steps like the oracle's loop.  The window (a third of the residuals frozen at a perturbed linearisation
    point + a marginalisation prior) makes the second Gauss-Newton step overshoot, so steps ARE rejected."""
    w = po.make_mixed_window(synth.add_synthetic_prior(copy.deepcopy(small)))
    o, g = po.OracleWindow(w), binding.BA.from_window(w)
    (mo, lo), (mg, lg) = o.calc_lm_energies(), g.calc_lm_energies()
    assert abs(mg - mo) <= 1e-9 * abs(mo) and abs(lg - lo) <= 1e-5 * abs(lo) and lo > 0 and mo != 0
    w.settings = w.settings.copy(); w.settings["forceAcceptStep"] = 0
    o = po.OracleWindow(w); o.set_force_all_iterations(True)
    g = binding.BA.from_window(w)
    rmo = o.optimize(6); rmg, its = g.optimize(6, force_all=True)
    eo, eg = o.energy_log(), g.get_energy_log()
    assert its == 6 and len(eo) == len(eg) == 8
    assert eo[2] > 2 * eo[1]                                                     # the overshooting step ...
    assert abs(eo[-1] - eo[1]) <= 1e-9 * eo[1]                                   # ... was rejected: the window ends at the last accepted state
    assert np.all(np.abs(eg - eo) <= 5e-4 * np.abs(eo)), (eo, eg)
    assert abs(rmg - rmo) <= 5e-4 * rmo
    ro, rg = o.get_residuals(False), g.get_residuals()
    assert (ro["state_state"] != rg["state_state"]).sum() <= 2e-3 * w.R
    fo, fg = o.get_frames(), g.get_frames()
    assert rel(fg["frames"]["state"], fo["frames"]["state"]) < 5e-3


def test_enqueue_gn_rccl_with_a_one_rank_communicator(small):
    """The C / C++ entry of the sharded iteration (ncclAllReduce inside, no torch.distributed): with a one-rank RCCL communicator it
    must reproduce the single-GPU fast path.  (RCCL refuses two ranks on one device, so more ranks need more GPUs.)"""
    import ctypes as C
    import os
    import torch
    rccl = C.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so"), mode=C.RTLD_GLOBAL)

    class UID(C.Structure):
        _fields_ = [("b", C.c_char * 128)]
    uid = UID()
    assert rccl.ncclGetUniqueId(C.byref(uid)) == 0
    comm = C.c_void_p()
    rccl.ncclCommInitRank.argtypes = [C.POINTER(C.c_void_p), C.c_int, UID, C.c_int]
    torch.cuda.set_device(0)
    assert rccl.ncclCommInitRank(C.byref(comm), 1, uid, 0) == 0
    try:
        win = synth.add_synthetic_prior(copy.deepcopy(small))
        a = binding.BA.from_window(win); b = binding.BA.from_window(win)
        for g in (a, b):
            g.collect_active(); g.linearize_all(False); g.apply_res()
        a.enqueue_gn(0, 4); a.sync()
        b.enqueue_gn_rccl(comm.value, 0, 4); b.sync()
        fa, fb = a.get_frames(), b.get_frames()
        assert rel(fb["frames"]["state"], fa["frames"]["state"]) < 5e-3          # same band as the two-handle test (different partial-sum boundaries)
        assert rel(fb["frames"]["frameEnergyTH"], fa["frames"]["frameEnergyTH"]) < 1e-3
        assert rel(b.get_points()["idepth"], a.get_points()["idepth"]) < 5e-3
        ea = a.get_residuals()["out"]["state_NewEnergy"].astype(np.float64).sum(); eb = b.get_residuals()["out"]["state_NewEnergy"].astype(np.float64).sum()
        assert abs(ea - eb) <= 1e-4 * ea
    finally:
        rccl.ncclCommDestroy.argtypes = [C.c_void_p]
        rccl.ncclCommDestroy(comm)


def test_edge_points_without_residuals_and_oob(tiny):
    """points with no residuals, OOB residuals (point projected outside the image) and an all-OUTLIER point."""
    w2 = copy.deepcopy(tiny)
    # point 0: move to the image corner so its residuals go OOB; point 1: absurd idepth -> OOB/outliers
    w2.points["u"][0] = 3.0; w2.points["v"][0] = 3.0
    w2.points["idepth"][1] = 50.0; w2.points["idepth_zero"][1] = 50.0
    # point 2: corrupt colours -> OUTLIER
    w2.points["color"][2] += 100.0
    o = po.OracleWindow(w2); g = binding.BA.from_window(w2)
    o.collect_active(); g.collect_active()
    Eo, Eg = o.linearize_all(False), g.linearize_all(False)
    ro, rg = o.get_residuals(False), g.get_residuals()
    assert np.array_equal(ro["out"]["state_NewState"], rg["out"]["state_NewState"])
    assert (rg["out"]["state_NewState"] == 1).sum() > 0 and (rg["out"]["state_NewState"] == 2).sum() > 0
    assert abs(Eo - Eg) <= TOL * Eo
    o.apply_res(); g.apply_res(); o.backup_state(); g.backup_state(); o.solve_system(0); g.solve_system(0)
    pto, _ = o.get_points(); ptg = g.get_points()
    assert rel(ptg["HdiF"], pto["HdiF"]) < 1e-5 and rel(ptg["step"], pto["step"]) < 5e-2
    assert ptg["HdiF"][0] == 0 and ptg["step"][0] == 0          # no good residual -> zeroed (AccumulatedSCHessian.cc:16-22)


def test_invalid_arguments_fail_loudly(tiny):
    with pytest.raises(binding.LdsoError):
        binding.BA(64, 64, 32, 10)                              # more frames than LDSO_MAX_FRAMES
    g = binding.BA(tiny.w, tiny.h, tiny.F, tiny.P)
    with pytest.raises(binding.LdsoError):
        g.linearize_all(False)                                  # no window yet
    g.set_settings(tiny.settings)
    for f in range(tiny.F):
        g.set_image(f, tiny.images[f][0])
    bad = tiny.residuals.copy(); bad["target"][0] = bad["host"][0]
    with pytest.raises(binding.LdsoError):
        g.set_window(np.arange(tiny.F), tiny.points, bad)
    s = tiny.settings.copy(); s["solverMode"] = 1
    with pytest.raises(binding.LdsoError) as e:
        g.set_settings(s)
    assert e.value.code == -4
