"""GPU parity of point activation (ldso_ba_activate_points: FullSystem::optimizeImmaturePoint / ImmaturePoint::linearizeResidual)
against the oracle restatement on the same inputs: inverse depth, energy, Hdd, bd bit for bit, verdict and per-target residual
states exact; plus the purpose of the function - the activated inverse depths are close to the scene's.  Windows of 9, 12 and 16 key frames run k_activate<2>
(second slot group: hosts and targets of index 8 and above); what those inputs reach is asserted from the oracle's per-point counts (orc_activate_points_diag)."""
import numpy as np
import pytest

from ldso_amd import synth, binding
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu


def _traced_points(win, per_frame):
    """immature points of the window's key frames, traced (oracle) against the two extra frames so that they carry intervals"""
    pts, true_id = synth.make_immature_points(win, per_frame)
    F = win.F
    for fidx in (F, F + 1):
        KRKi, Kt, aff = synth.trace_poses(win, fidx)
        po.trace_on(pts, win.images[fidx][0], KRKi, Kt, aff)
    keep = np.isfinite(pts["idepth_max"]) & (pts["lastTraceStatus"] != 1)
    return pts[keep].copy(), true_id[keep]


def _K4(win):
    return np.asarray([np.float32(50.0 * v) for v in win.calib["value"]], np.float32)


def _assert_same(out, ref):
    """verdict, residual states, counts exact; inverse depth, energy, Hdd, bd by bit pattern"""
    for k in ("ok", "res_state", "numGoodRes", "iterations"):
        bad = np.nonzero((out[k] != ref[k]).reshape(len(out), -1).any(1))[0]
        assert len(bad) == 0, (k, bad[:8], out[k][bad[:4]], ref[k][bad[:4]])
    for k in ("idepth", "energy", "Hdd", "bd"):
        bad = np.nonzero(out[k].view(np.uint32) != ref[k].view(np.uint32))[0]
        assert len(bad) == 0, (k, bad[:8], out[k][bad[:4]], ref[k][bad[:4]])


@pytest.mark.parametrize("name,per_frame,F", [
    pytest.param("small", 120, None, id="small-120"), pytest.param("C3", 200, None, id="C3-200"),
    pytest.param("small", 60, 9, id="small-60-F9"), pytest.param("small", 60, 12, id="small-60-F12"), pytest.param("small", 60, 16, id="small-60-F16")])
def test_activation_matches_oracle(name, per_frame, F):
    win = synth.make_config(name, extra_frames=2) if F is None else synth.make_config(name, extra_frames=2, F=F)
    pts, true_id = _traced_points(win, per_frame)
    assert len(pts) > 50
    g = binding.BA.from_window(win)
    pairs = g.get_pair_rt()
    F = win.F
    ref, diag = po.activate_points(pts, [win.images[f][0] for f in range(F)], _K4(win), pairs, win.w, win.h, diag=True)
    if F > 8:                                            # what the second slot group gets to do
        assert (pts["host"] >= 8).sum() >= 30
        assert (ref["res_state"][:, 8:F] == 0).sum() >= 30
        assert (diag[:, po.AD_MID_PATTERN] > 0).sum() >= 3          # residuals that left mid-pattern: Hdd / bd keep their partial sums
    assert (ref["res_state"][:, F:] == -1).all()
    out = g.activate_points(pts)
    _assert_same(out, ref)
    ok = out["ok"] == 1
    assert ok.mean() > 0.5
    relerr = np.abs(out["idepth"][ok] - true_id[ok]) / true_id[ok]
    assert np.median(relerr) < 0.05                      # activation lands on the scene's inverse depth


def _loop_only_failure(pts, images, K4, pairs, w, h):
    """a record whose first pass has Hdd >= 100 while the first Gauss-Newton pass has newHdd < 100 (FullSystem.cc:945-947): Hdd is a sum over the residuals that are
    not OOB, so it drops where a residual left the image in the first pass.  Weights scale Hdd by their square and leave the step alone: scale the weights of the
    candidate with the largest drop so that 100 falls between the two."""
    first = po.activate_points(pts, images, K4, pairs, w, h, gn_iterations=0)
    one = po.activate_points(pts, images, K4, pairs, w, h, gn_iterations=1, min_idepth_hessian=0.0)
    moved = (one["iterations"] == 1) & (one["idepth"] != first["idepth"]) & (first["Hdd"] > 0) & (one["Hdd"] > 0) & np.isfinite(first["energy"])
    ratio = np.where(moved, one["Hdd"] / np.maximum(first["Hdd"], 1e-30), np.inf)
    i = int(np.argmin(ratio))
    assert ratio[i] < 0.98, ratio[i]
    p = pts[i:i + 1].copy()
    p["weights"] *= np.float32(np.sqrt(100.0 / np.sqrt(float(first["Hdd"][i]) * float(one["Hdd"][i]))))
    return p


def test_activation_edge_cases():
    win = synth.make_config("small", extra_frames=2)
    pts, _ = _traced_points(win, 40)
    # a NaN patch in target 1: some projected patterns meet it at their first pixel, some later (isfinite(hit) at k == 0 and at k > 0)
    win.images[1][0][100:150, 120:200, 0] = np.nan
    g = binding.BA.from_window(win)
    pairs = g.get_pair_rt()
    K4 = _K4(win)
    images = [win.images[f][0] for f in range(win.F)]
    special = _loop_only_failure(pts, images, K4, pairs, win.w, win.h)
    pts = np.concatenate([pts[:24], pts[pts["host"] != 1][24:64], special])
    pts["idepth_min"][0] = np.nan                        # non-finite start: rejected
    pts["idepth_min"][1] = 50.0; pts["idepth_max"][1] = 60.0     # absurdly close: projections leave the images (OOB residuals)
    pts["u"][2] = 2.0; pts["v"][2] = 2.0                 # pattern leaves the image in the targets
    pts["energyTH"][3] = 1e-9                            # OUTLIER already at slack 1000
    ref, diag = po.activate_points(pts, images, K4, pairs, win.w, win.h, diag=True)
    assert (diag[:, po.AD_NONFINITE_FIRST] > 0).sum() >= 1 and (diag[:, po.AD_NONFINITE_LATER] > 0).sum() >= 1
    assert diag[3, po.AD_FIRST_PASS_OUTLIER] > 0
    # the last record fails at :945-947 and nowhere else: one iteration, residuals in, finite state, Hdd of the first pass still above the threshold
    assert ref["ok"][-1] == 0 and ref["iterations"][-1] == 1 and ref["numGoodRes"][-1] >= 1 and np.isfinite(ref["idepth"][-1]) and np.isfinite(ref["energy"][-1])
    assert ref["Hdd"][-1] >= 100.0
    out = g.activate_points(pts)
    _assert_same(out, ref)
    assert out["ok"][0] == 0
    assert len(g.activate_points(pts[:0])) == 0
