"""Inputs of tests/test_batch_activate_gpu.py and scripts/time_batch_activate.py: what FullSystem::activatePointsMT (FullSystem.cc:1052-1189) reads for one window,
built in numpy from a synthetic window, so that nothing depends on the reference libraries.  The newest key frame of the window (index F - 1) plays the newest
frame of the selection: the candidates are fresh immature points on the other key frames, traced on the CPU (oracle.pyoracle.trace_on) against the window's own
last two key frames so that they carry depth intervals and statuses, then given every branch of the candidate rule (activation_select_common.add_branch_cases);
the seeds are the window's points that the newest frame does not host; KRKi / Kt are the ground-truth poses host -> newest frame at pyramid level 1."""
import numpy as np

from ldso_amd import synth
from oracle import pyoracle as po
import activation_select_common as asc

KEEP, DROP, SELECTED = synth.ACT_KEEP, synth.ACT_DROP, synth.ACT_SELECTED
JOB_KEYS = ("seeds", "cand", "my_type", "KRKi", "Kt", "flagged")


def level1_poses(win):
    """K[1] * R * Ki[0] and K[1] * t of every key frame towards the newest one (FullSystem.cc:1093-1094): synth.trace_poses scaled to pyramid level 1"""
    KRKi0, Kt0, _ = synth.trace_poses(win, win.F - 1)
    S = np.array([[0.5, 0, -0.25], [0, 0.5, -0.25], [0, 0, 1]], np.float32)          # K[1] = S K[0]: fx / 2, (cx + 0.5) / 2 - 0.5
    KRKi = np.stack([(S @ k.reshape(3, 3)).ravel() for k in KRKi0]).astype(np.float32)
    Kt = np.stack([S @ t for t in Kt0]).astype(np.float32)
    return KRKi, Kt


def window_seeds(win):
    """the points the newest frame does not host, at their current inverse depth (CoarseTracker.cc:706-709), hosts in window order"""
    p = win.points[win.points["host"] != win.F - 1]
    sd = np.zeros(len(p), synth.ACT_SEED_DTYPE)
    sd["u"], sd["v"], sd["idepth_scaled"], sd["host"] = p["u"], p["v"], p["idepth"], p["host"]
    return sd


def traced_candidates(win, per_frame, seed=7):
    """per_frame immature points on every key frame but the newest, traced into the last two key frames (each point into those that are not its host)"""
    F = win.F
    pts, _ = synth.make_immature_points(win, per_frame, seed=seed, frames=range(F - 1))
    for target in ([F - 2] if F >= 3 else []) + [F - 1]:
        KRKi, Kt, aff = synth.trace_poses(win, target)
        m = pts["host"] != target
        sub = np.ascontiguousarray(pts[m])
        po.trace_on(sub, win.images[target][0], KRKi, Kt, aff)
        pts[m] = sub
    return pts


def make_job(win, per_frame, seed=7, types_seed=3, flag_frame=None):
    """-> dict(seeds, cand, my_type, KRKi, Kt, flagged): the arrays ldso_ba_select_candidates takes, my_type mixed over 1 / 2 / 4, one host flagged"""
    rng = np.random.default_rng(types_seed)
    cand = traced_candidates(win, per_frame, seed=seed)
    asc.add_branch_cases(cand, rng)
    types = rng.choice(np.array([1.0, 2.0, 4.0], np.float32), len(cand), p=(0.5, 0.3, 0.2))
    KRKi, Kt = level1_poses(win)
    flagged = np.zeros(win.F, np.int32)
    flagged[min(1, win.F - 2) if flag_frame is None else flag_frame] = 1
    return dict(seeds=window_seeds(win), cand=cand, my_type=types, KRKi=KRKi, Kt=Kt, flagged=flagged)


def with_distance(job, min_act_dist, **over):
    j = dict(job, min_act_dist=float(min_act_dist))
    j.update(over)
    return j


def solo_args(job):
    return tuple(job[k] for k in JOB_KEYS)


def order_dependent(job, decision, map_before, min_dist):
    """candidates that pass the distance test against the map BEFORE the loop and are still kept: rejected at their turn by a candidate accepted before them
    (tests/test_activate_select_gpu.py::_order_dependent)"""
    c = job["cand"]
    keep = np.nonzero(decision == KEEP)[0]
    K = job["KRKi"][c["host"][keep]]; T = job["Kt"][c["host"][keep]]
    h1, w1 = map_before.shape
    with np.errstate(all="ignore"):
        d = np.float32(0.5) * (c["idepth_max"][keep] + c["idepth_min"][keep])
        p = [((K[:, 3 * i] * c["u"][keep] + K[:, 3 * i + 1] * c["v"][keep]) + K[:, 3 * i + 2]) + T[:, i] * d for i in range(3)]
        u = (p[0] / p[2] + np.float32(0.5)); v = (p[1] / p[2] + np.float32(0.5))
        el = np.isfinite(u) & np.isfinite(v) & (u >= 1) & (v >= 1) & (u < w1) & (v < h1)
    el &= asc.eligible_in_bounds(job, (h1, w1))[keep]
    ui, vi = u[el].astype(np.int64), v[el].astype(np.int64)
    dist = map_before[vi, ui] + (p[0][el] - np.floor(p[0][el]))
    return int((dist >= np.float32(min_dist) * job["my_type"][keep][el]).sum())


def input_conditions(job, min_act_dist, decision, selected, records, shape):
    """the conditions that keep a comparison from passing on empty work, for a window with min_act_dist > 0 -> the figures, asserted"""
    el = int(asc.eligible_in_bounds(job, shape).sum())
    share = len(selected) / max(el, 1)
    drops = int((decision == DROP).sum())
    ok = float(records["ok"].mean()) if records is not None and len(records) else None
    fig = dict(candidates=len(job["cand"]), eligible=el, selected=len(selected), share=round(share, 3), dropped=drops, ok=ok)
    assert len(selected) >= 30, fig
    assert 0.10 <= share <= 0.90, fig
    assert drops >= 5, fig
    if records is not None:
        assert 0.0 < ok < 1.0, fig
    return fig
