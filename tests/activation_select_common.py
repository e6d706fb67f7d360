"""Candidate selection of FullSystem::activatePointsMT (FullSystem.cc:1052-1189) for tests/test_activate_select_*.py and scripts/time_activate_select.py:
ctypes bindings of the harness entries adapter/adapter_capi.cc adds for it (through oracle.pyref.adapter_lib()), and the states the tests run at - a window
of reference objects whose last key frame plays the newest frame, traced immature points on the others, every branch of the candidate rule present."""
import ctypes as C

import numpy as np

from ldso_amd import synth
from oracle import pyoracle as po, pyref as pr

KEEP, DROP, SELECTED = synth.ACT_KEEP, synth.ACT_DROP, synth.ACT_SELECTED
MIN_TRACE_QUALITY = 3.0            # setting_minTraceQuality (Setting.cc:51)
DEFAULT_DENSITY = 2000.0           # setting_desiredPointDensity (Setting.cc:30)


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def adp():
    A = pr.adapter_lib()
    A.adp_set_desired_point_density.restype = C.c_float
    A.adp_get_min_act_dist.restype = C.c_float
    return A


def _chk(rc):
    if rc < 0:
        raise RuntimeError(adp().adp_last_error().decode())
    return rc


def set_distance_map(on: bool):
    """adp_make_keyframe: FullSystem::activatePointsMT with distance map and controller (GpuBackend::activatePointsMT with an adapter) instead of the restated rule"""
    adp().adp_set_distance_map(C.c_int(1 if on else 0))


def min_act_dist_trace():
    """fs.currentMinActDist after every key frame adp_make_keyframe ran since set_distance_map"""
    out = np.zeros(256, np.float32)
    n = adp().adp_min_act_dist_trace(C.c_int(len(out)), _p(out))
    return out[:n].copy()


def set_all_point_status(r, status: int) -> int:
    """Point::status of every point of the graph (Point.h: 0 ACTIVE, 1 OUTLIER, ...)"""
    return int(adp().adp_set_all_point_status(r.fs_handle(), C.c_int(status)))


def set_desired_point_density(v: float) -> float:
    """-> the value it replaces"""
    return float(adp().adp_set_desired_point_density(C.c_float(v)))


def min_act_dist(r) -> float:
    return float(adp().adp_get_min_act_dist(r.fs_handle()))


def set_min_act_dist(r, v: float):
    adp().adp_set_min_act_dist(r.fs_handle(), C.c_float(v))


def ef_npoints(r) -> int:
    return int(adp().adp_ef_npoints(r.fs_handle()))


def set_immature_types(r, types):
    t = np.ascontiguousarray(types, np.float32)
    n = adp().adp_set_immature_types(r.fs_handle(), C.c_int(len(t)), _p(t))
    assert n == len(t), (n, len(t))


def feature_statuses(r):
    fs = r.fs_handle()
    n = adp().adp_feature_statuses(fs, C.c_int(0), None)
    out = np.zeros(n, np.int32)
    adp().adp_feature_statuses(fs, C.c_int(n), _p(out))
    return out


def map_shape(r):
    return (r.win.h >> 1, r.win.w >> 1)


def ref_distance_map(r):
    out = np.zeros(map_shape(r), np.float32)
    assert adp().adp_get_ref_distance_map(r.fs_handle(), _p(out)) == out.size
    return out


def ref_activate_points_mt(r):
    """the reference's own FullSystem::activatePointsMT()"""
    _chk(adp().adp_ref_activate_points_mt(r.fs_handle()))
    r.L.ref_fs_sync_back(r.h)


def adapter_activate_points_mt(adapter, r):
    """GpuBackend::activatePointsMT(fs) -> (candidates, selected, activated)"""
    c = np.zeros(3, np.int32)
    if adp().adp_activate_points_mt(adapter.h, r.fs_handle(), _p(c)) != 0:
        raise RuntimeError(adp().adp_last_error().decode())
    r.L.ref_fs_sync_back(r.h)
    return tuple(int(x) for x in c)


def ref_select(r, current_min_act_dist: float):
    """the selection loop through the reference's compiled CoarseDistanceMap members; the graph keeps its statuses"""
    fs = r.fs_handle()
    n = _chk(adp().adp_ref_select_candidates(fs, C.c_float(current_min_act_dist), C.c_int(0), None, None, None, None, None))
    dec = np.zeros(n, np.int32); sel = np.zeros(max(n, 1), np.int32); ns = C.c_int()
    before = np.zeros(map_shape(r), np.float32); after = np.zeros(map_shape(r), np.float32)
    assert _chk(adp().adp_ref_select_candidates(fs, C.c_float(current_min_act_dist), C.c_int(n), _p(dec), _p(sel), C.byref(ns), _p(before), _p(after))) == n
    return dict(decision=dec, selected=sel[:ns.value].copy(), map_before=before, map_after=after)


def ref_apply_selection(r, decision, selected):
    """statuses of the deleted candidates, the reference's activatePointsMT_Reductor on the selected ones, the hand-over of FullSystem.cc:1166-1188"""
    d = np.ascontiguousarray(decision, np.int32); s = np.ascontiguousarray(selected, np.int32)
    if adp().adp_ref_apply_selection(r.fs_handle(), C.c_int(len(d)), _p(d), C.c_int(len(s)), _p(s)) != 0:
        raise RuntimeError(adp().adp_last_error().decode())
    r.L.ref_fs_sync_back(r.h)


def time_ref_select(r, current_min_act_dist: float, reps: int):
    """seconds per selection on one core, [reps]"""
    out = np.zeros(reps)
    _chk(adp().adp_time_ref_select_candidates(r.fs_handle(), C.c_float(current_min_act_dist), C.c_int(reps), _p(out)))
    return out


def gather(r):
    """the common state for the device leg: what the selection reads from the graph, as the arrays ldso_ba_select_candidates takes"""
    fs = r.fs_handle()
    cnt = np.zeros(3, np.int32)
    assert adp().adp_gather_selection(fs, _p(cnt), None, None, None, None, None, None) == 0, adp().adp_last_error()
    ns, n, nh = (int(x) for x in cnt)
    seeds = np.zeros(ns, synth.ACT_SEED_DTYPE); cand = np.zeros(n, synth.IMMATURE_DTYPE); mt = np.zeros(n, np.float32)
    KRKi = np.zeros((nh, 9), np.float32); Kt = np.zeros((nh, 3), np.float32); fl = np.zeros(nh, np.int32)
    assert adp().adp_gather_selection(fs, _p(cnt), _p(seeds), _p(cand), _p(mt), _p(KRKi), _p(Kt), _p(fl)) == 0
    return dict(seeds=seeds, cand=cand, my_type=mt, KRKi=KRKi, Kt=Kt, flagged=fl)


def eligible_in_bounds(g, shape):
    """candidates that reach the distance test: canActivate and projected into the map (numpy restatement, used for the conditions on the inputs only)"""
    c = g["cand"]
    st = c["lastTraceStatus"]
    with np.errstate(invalid="ignore"):
        can = np.isfinite(c["idepth_max"]) & (st != 2) & np.isin(st, (0, 3, 4, 1)) & (c["lastTracePixelInterval"] < 8) & (c["quality"] > MIN_TRACE_QUALITY) \
            & ((c["idepth_max"] + c["idepth_min"]) > 0)
        K = g["KRKi"][c["host"]]; T = g["Kt"][c["host"]]
        d = np.float32(0.5) * (c["idepth_max"] + c["idepth_min"])
        p = [K[:, 3 * i] * c["u"] + K[:, 3 * i + 1] * c["v"] + K[:, 3 * i + 2] + T[:, i] * d for i in range(3)]
        u = p[0] / p[2] + 0.5; v = p[1] / p[2] + 0.5
        inb = (u >= 1) & (v >= 1) & (u < shape[1]) & (v < shape[0])
    return can & inb


def traced_immature(win, per_frame, seed=7, extra=(0, 1)):
    """immature points on the window's key frames, traced (oracle) into the extra frames so that they carry depth intervals and statuses"""
    pts, _ = synth.make_immature_points(win, per_frame, seed=seed)
    for e in extra:
        KRKi, Kt, aff = synth.trace_poses(win, win.F + e)
        po.trace_on(pts, win.images[win.F + e][0], KRKi, Kt, aff)
    return pts


def add_branch_cases(pts, rng, frac=0.04):
    """every branch of FullSystem.cc:1105-1148 on a share of the records: never traced, OUTLIER, OOB, interval >= 8, low quality, idepth_min + idepth_max <= 0,
    projection out of bounds (a depth interval far in front of the camera)"""
    n = len(pts)
    k = max(3, int(frac * n))
    idx = rng.permutation(n)[:7 * k].reshape(7, k)
    pts["idepth_max"][idx[0]] = np.nan
    pts["lastTraceStatus"][idx[1]] = 2
    pts["lastTraceStatus"][idx[2]] = 1
    pts["lastTracePixelInterval"][idx[3]] = 8.0
    pts["quality"][idx[4]] = 3.0
    pts["idepth_min"][idx[5]] = -1.0; pts["idepth_max"][idx[5]] = 1.0
    pts["idepth_min"][idx[6]] = 40.0; pts["idepth_max"][idx[6]] = 60.0
    half = idx[2][: k // 2]                                    # OOB that cannot activate either
    pts["lastTracePixelInterval"][half] = 9.0
    # ... and candidates the selection takes but optimizeImmaturePoint rejects (zero weights: Hdd = 0 < setting_minIdepthH_act, FullSystem.cc:924-926)
    pts["weights"][np.random.default_rng(99).permutation(n)[:k]] = 0.0
    return pts


def make_state(name="C3", per_frame=1200, seed=7, types_seed=3, flag_frame=1, branch_cases=True, n_graphs=1, type_p=(0.5, 0.3, 0.2), **over):
    """-> (win, [RefWindow] * n_graphs, immature records): identical object graphs of the window `name` (its last key frame is the newest frame of the selection)
    with traced immature points of mixed my_type on every key frame; frame `flag_frame` flaggedForMarginalization."""
    win = synth.make_config(name, extra_frames=2 if per_frame else 0, **over)
    rng = np.random.default_rng(types_seed)
    pts = traced_immature(win, per_frame, seed=seed) if per_frame else np.zeros(0, synth.IMMATURE_DTYPE)
    if branch_cases and per_frame:
        add_branch_cases(pts, rng)
    types = rng.choice(np.array([1.0, 2.0, 4.0], np.float32), len(pts), p=type_p)
    graphs = []
    for _ in range(n_graphs):
        r = pr.RefWindow(win)
        r.fs_attach()
        if len(pts):
            r.fs_add_immature(pts)
            set_immature_types(r, types)
        if flag_frame is not None:
            r.fs_flag_frame(flag_frame)
        graphs.append(r)
    return win, graphs, pts
