"""What tests/test_batch_update_window_gpu.py builds its windows from: the scenario of tests/test_resident_gpu.py::_scenario (old window -> optimize -> the reference's
edits on the host objects -> the delta of ldso_ba_update_window plus the window `w1` a fresh upload of the same objects would load), restated in two steps because here
the optimize() in the middle is the BATCH's: start() / load() give the old window on a handle, edit() reads that handle after the optimize and returns the delta.

One delta is applied to two sets of handles (set X through ldso_ba_batch_update_windows, set Y through the single-window entries): it names indices and brings fresh
records from the synthetic scene, and the frames / prior that follow come from `w1`, so the two sets receive the same host bytes."""
import copy
import functools

import numpy as np

from ldso_amd import synth, binding
from test_resident_gpu import _sub

KINDS = {
    "steady": (7, [0, 1, 2, 3, 4, 5], [1, 2, 3, 4, 5, 6]),          # makeKeyFrame's steady state: the oldest frame leaves, a new one arrives
    "points-only": (7, [0, 1, 2, 3, 4, 5], [0, 1, 2, 3, 4, 5]),     # nothing but point / residual edits
    "middle": (7, [0, 1, 2, 3, 4], [0, 1, 3, 4, 5, 6]),             # a middle frame leaves, two arrive
    "grow-to-9": (10, [0, 1, 2, 3, 4, 5, 6, 7], [1, 2, 3, 4, 5, 6, 7, 8, 9]),      # 8 -> 9 frames: the slot table would widen (FS 8 -> 16)
}


@functools.lru_cache(maxsize=None)
def scene(F_big, P):
    """the synthetic scene all windows of one size are cut from (read-only: every user copies what it edits)"""
    return synth.make_config("small", F=F_big, P=P)


def start(kind, P, seed):
    """the old window of a scenario: which points of the scene it holds depends on the seed"""
    F_big, old_frames, new_frames = KINDS[kind]
    rng = np.random.default_rng(seed)
    big = scene(F_big, P)
    old_pts = np.nonzero(np.isin(big.points["host"], old_frames) & (rng.random(big.P) < 0.85))[0]
    w0, _, _ = _sub(big, old_frames, old_pts)
    synth.add_synthetic_prior(w0, seed=3)
    return dict(kind=kind, seed=seed, big=big, old_frames=old_frames, new_frames=new_frames, old_pts=old_pts, w0=w0)


def load(st, stream):
    """a handle that holds the scenario's old window, frames and prior (image slot = frame index in the scene)"""
    big, w0 = st["big"], st["w0"]
    A = binding.BA(big.w, big.h, max_frames=big.F, max_points=big.P, stream=stream)
    A.set_settings(big.settings)
    for f in range(big.F):
        A.set_image(f, big.images[f][0])
    A.set_window(st["old_frames"], w0.points, w0.residuals)
    A.set_frames(w0.frames, w0.calib)
    A.set_prior(w0.HM, w0.bM)
    return A


def edit(st, A, keep=0.9):
    """The host objects after the write-back of handle A's optimize(), the reference's edits, the delta: tests/test_resident_gpu.py::_scenario from its get_points() on.
    keep = the share of the old points (of frames that stay) that survive.  -> dict with `job` (the arguments of BA.update_window), `w1`, `mrb`, `ngr`."""
    big, old_frames, new_frames, old_pts, w0 = st["big"], st["old_frames"], st["new_frames"], st["old_pts"], st["w0"]
    rng = np.random.default_rng(1000 + st["seed"])
    pa, ra, fa = A.get_points(), A.get_residuals(), A.get_frames()
    big2 = copy.copy(big)
    big2.points, big2.frames, big2.calib, big2.residuals = big.points.copy(), big.frames.copy(), big.calib.copy(), big.residuals.copy()
    big2.points["idepth"][old_pts] = pa["idepth"]; big2.points["idepth_zero"][old_pts] = pa["idepth"]
    big2.frames[old_frames] = fa["frames"]
    big2.calib["value"] = fa["calib_value"]
    rb = big.residuals
    in_old = np.isin(rb["point"], old_pts) & np.isin(rb["target"], old_frames)
    idx_old = np.nonzero(in_old)[0]
    idx_old = idx_old[np.lexsort((rb["target"][idx_old], rb["point"][idx_old]))]          # = the flat order of w0
    assert len(idx_old) == w0.R
    big2.residuals["state_state"][idx_old] = ra["state_state"]; big2.residuals["is_active"][idx_old] = ra["is_active"]
    big2.residuals["state_energy"][idx_old] = ra["out"]["state_NewEnergy"]; big2.residuals["is_new"][idx_old] = 1
    dropped_res = np.zeros(big.R, bool)
    dropped_res[idx_old] = (ra["to_remove"] != 0) | (rng.random(w0.R) < 0.03)                # linearizeAll(true)'s toRemove + a few more dropResidual calls
    gone_frames = [f for f in old_frames if f not in new_frames]
    added_frames = [f for f in new_frames if f not in old_frames]
    survive = old_pts[~np.isin(big.points["host"][old_pts], gone_frames) & (rng.random(len(old_pts)) < keep)]
    fresh = np.nonzero(~np.isin(np.arange(big.P), old_pts) & np.isin(big.points["host"], [f for f in new_frames if f not in added_frames]))[0]
    new_res = np.isin(rb["point"], survive) & np.isin(rb["target"], added_frames)            # insertResidual: IN, energy 0, not active, isNew
    big2.residuals["state_state"][new_res] = 0; big2.residuals["is_active"][new_res] = 0; big2.residuals["state_energy"][new_res] = 0; big2.residuals["is_new"][new_res] = 1
    big2.residuals["is_new"][np.isin(rb["point"], fresh)] = 1
    new_pts = np.sort(np.concatenate([survive, fresh]))                                   # host-major order of the scene = makeIDX order
    big2.residuals = big2.residuals[~dropped_res]
    w1, _, _ = _sub(big2, new_frames, new_pts)
    synth.add_synthetic_prior(w1, seed=4)
    mrb = np.zeros(big.P, np.float32); ngr = np.zeros(big.P, np.int32)
    mrb[old_pts] = pa["maxRelBaseline"]; ngr[old_pts] = pa["numGoodResiduals"]
    frame_from = np.array([old_frames.index(f) if f in old_frames else -1 for f in new_frames], np.int32)
    old_row = -np.ones(big.P, np.int64); old_row[old_pts] = np.arange(len(old_pts))
    point_from = old_row[new_pts].astype(np.int32)
    is_fresh = point_from < 0
    point_from[is_fresh] = -1 - np.arange(is_fresh.sum())
    res_mask = np.zeros(len(new_pts), np.uint32)
    np.bitwise_or.at(res_mask, w1.residuals["point"], (1 << w1.residuals["target"]).astype(np.uint32))
    fresh_rows = np.nonzero(is_fresh)[0]
    fresh_res = w1.residuals[np.isin(w1.residuals["point"], fresh_rows)].copy()
    remap = -np.ones(len(new_pts), np.int64); remap[fresh_rows] = np.arange(len(fresh_rows))
    fresh_res["point"] = remap[fresh_res["point"]]
    job = (np.asarray(new_frames, np.int32), frame_from, point_from, res_mask, w1.points[fresh_rows], fresh_res, mrb[new_pts][fresh_rows], ngr[new_pts][fresh_rows])
    return dict(job=job, w1=w1, n_survive=len(survive), n_fresh=len(fresh), n_dropped=int(dropped_res.sum()))


def edit_again(sc, A, flags, seed):
    """A second, points-only edit of the window `sc` left on handle A (after another optimize() and the marginalisation of the points in `flags`): the marginalised
    points and a tenth of the others leave, linearizeAll(true)'s toRemove and a few more residuals are dropped, the frames stay.  -> (job, frames, calib, (HM, bM))"""
    w1 = sc["w1"]
    rng = np.random.default_rng(2000 + seed)
    ra, fa = A.get_residuals(), A.get_frames()
    assert len(ra["to_remove"]) == w1.R and len(flags) == w1.P
    stay = np.nonzero((np.asarray(flags) == 0) & (rng.random(w1.P) > 0.1))[0]
    res_keep = (ra["to_remove"] == 0) & (rng.random(w1.R) > 0.03)
    res_mask = np.zeros(w1.P, np.uint32)
    r = w1.residuals[res_keep]
    np.bitwise_or.at(res_mask, r["point"], (1 << r["target"]).astype(np.uint32))
    job = (sc["job"][0], np.arange(w1.F, dtype=np.int32), stay.astype(np.int32), res_mask[stay])
    calib = w1.calib.copy(); calib["value"] = fa["calib_value"]
    n = 8 * w1.F + 4
    g = np.random.default_rng(3000 + seed)
    M = g.standard_normal((n, n)) * 1e-2
    return job, fa["frames"].copy(), calib, (M @ M.T, g.standard_normal(n) * 1e-2)
