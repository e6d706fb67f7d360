"""GpuBackend::residentImmature (adapter/ldso_gpu_adapter.h): the drop-in with the immature set resident on the device against the same drop-in with the mode
off, on two identical reference object graphs driven through the same schedule.  Both legs run the same kernels on the same values - one moves the records
across PCIe and through the objects at every stage, the other does not - so everything compared is exactly equal."""
import ctypes as C

import numpy as np
import pytest

from ldso_amd import synth
from oracle import pyref as pr

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not (pr.available() and pr.adapter_available()), reason="oracle/_ref/libldso_ref.so / adapter/_build/libldso_adapter_test.so not built")]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _set_resident(adapter, on):
    assert pr.adapter_lib().adp_set_resident_immature(adapter.h, C.c_int(1 if on else 0)) == 0


def _sync(adapter, r):
    A = pr.adapter_lib()
    if A.adp_sync_immature(adapter.h, r.fs_handle()) != 0:
        raise RuntimeError(A.adp_last_error().decode())


def _counts(adapter):
    """reconcile steps so far: (rows unchanged, one compaction, full upload)"""
    out = np.zeros(3, np.int32)
    assert pr.adapter_lib().adp_immature_reconcile_counts(adapter.h, _p(out)) == 0
    return tuple(int(x) for x in out)


def _trace(adapter, r, win, fidx):
    T = win.truth["w2c"][fidx]
    return adapter.trace_new_coarse(r, r.fs_new_frame(win.images[fidx][0], T, float(win.truth["aff_a"][fidx]), float(win.truth["aff_b"][fidx])))


def _assert_graphs_equal(r_off, r_on, what):
    import activation_select_common as asc
    assert np.array_equal(asc.feature_statuses(r_off), asc.feature_statuses(r_on)), what
    ga, gb = pr.graph_summary(r_off), pr.graph_summary(r_on)
    for k in ("points", "immature", "residuals", "host", "uv", "idepth"):
        assert np.array_equal(ga[k], gb[k]), (what, k)
    ca, cb = asc.gather(r_off), asc.gather(r_on)
    assert len(ca["cand"]) == len(cb["cand"]) and ca["cand"].tobytes() == cb["cand"].tobytes(), what
    assert np.array_equal(ca["my_type"], cb["my_type"]), what
    assert np.float32(asc.min_act_dist(r_off)) == np.float32(asc.min_act_dist(r_on)), what
    return ga, ca


def _pair(win):
    A_off = pr.GpuAdapter(max_frames=win.F + 1, max_points=win.P + 2048)
    A_on = pr.GpuAdapter(max_frames=win.F + 1, max_points=win.P + 2048)
    _set_resident(A_on, True)
    return A_off, A_on


def test_resident_cycle_equals_the_transferring_cycle():
    """trace, trace, activatePointsMT, marginalise the flagged frame, trace, sync: the graphs end exactly equal, and the resident leg uploaded the records once"""
    import activation_select_common as asc
    win, (r_off, r_on), pts = asc.make_state("small", per_frame=400, P=150, n_graphs=2)
    F = win.F
    A_off, A_on = _pair(win)
    legs = ((A_off, r_off), (A_on, r_on))
    before = r_on.fs_get_immature()
    assert len(before) == len(pts) and before.tobytes() == r_off.fs_get_immature().tobytes()
    # 1. two frames traced
    for fidx in (F, F + 1):
        c = [_trace(A, r, win, fidx) for A, r in legs]
        assert np.array_equal(c[0], c[1]) and c[0].sum() == len(pts)
    assert _counts(A_on) == (1, 0, 1), "the first trace uploads the set, the second finds it where it is"
    assert _counts(A_off) == (0, 0, 0)
    # the objects of the resident leg were not written: they still hold what the state was built with, the other leg's moved on
    stale, fresh = r_on.fs_get_immature(), r_off.fs_get_immature()
    assert stale.tobytes() == before.tobytes() and fresh.tobytes() != before.tobytes()
    # 2. activatePointsMT
    s = [asc.adapter_activate_points_mt(A, r) for A, r in legs]
    assert s[0] == s[1] and s[0][1] > 100 and 0 < s[0][2] < s[0][1], s
    assert _counts(A_on) == (2, 0, 1), "the activation read the tracer's rows: no record went up"
    # 3. the flagged frame leaves the window (its immature points with it, the hosts behind it shift)
    for _, r in legs:
        r.fs_marginalize_frame(1)
    # 4. trace again
    c = [_trace(A, r, win, F) for A, r in legs]
    assert np.array_equal(c[0], c[1]) and 0 < c[0].sum() < len(pts)
    assert _counts(A_on) == (2, 1, 1), "the rows of the marginalised frame left by one compaction, the host indices were remapped"
    # 5. the device state into the objects
    _sync(A_on, r_on)
    g, cand = _assert_graphs_equal(r_off, r_on, "after the cycle")
    assert g["F"] == F - 1 and g["points"].sum() > 100 and len(cand["cand"]) > 100
    left = r_on.fs_get_immature()
    assert left.tobytes() == r_off.fs_get_immature().tobytes() and 0 < len(left) < len(pts)
    assert len(np.unique(left["lastTraceStatus"])) >= 3
    for A, r in legs:
        A.close(); r.close()
    r_off.L.ref_fs_release_new_frames()


def test_host_created_points_take_the_full_upload():
    """points the host creates between two traces (the device has not seen them) send the reconcile down its third branch: the device state is written into the
    objects that are still there, everything goes up again, and the two legs still end equal"""
    import activation_select_common as asc
    win, (r_off, r_on), pts = asc.make_state("small", per_frame=200, P=150, n_graphs=2)
    F = win.F
    A_off, A_on = _pair(win)
    legs = ((A_off, r_off), (A_on, r_on))
    for A, r in legs:
        _trace(A, r, win, F)
    more, _ = synth.make_immature_points(win, 30, seed=23, frames=list(range(F - 1)))
    for _, r in legs:
        r.fs_add_immature(more)
    c = [_trace(A, r, win, F + 1) for A, r in legs]
    assert np.array_equal(c[0], c[1]) and c[0].sum() == len(pts) + len(more)
    assert _counts(A_on) == (0, 0, 2)
    _sync(A_on, r_on)
    _assert_graphs_equal(r_off, r_on, "after the full upload")
    s = [asc.adapter_activate_points_mt(A, r) for A, r in legs]
    assert s[0] == s[1] and s[0][1] > 50
    _sync(A_on, r_on)
    _assert_graphs_equal(r_off, r_on, "after the activation")
    assert _counts(A_on) == (1, 0, 2)
    for A, r in legs:
        A.close(); r.close()
    r_off.L.ref_fs_release_new_frames()


def _make_new_traces(adapter, r, fh, n, cap=2048):
    """GpuBackend::makeNewTraces through adp_make_new_traces -> (the features' immature records, counts: detected, corners, dropped, kept)"""
    import feature_detect_common as fc
    pat = np.ascontiguousarray(fc.golden()["pattern"], np.int32)
    feat, desc, imm, counts = np.zeros((cap, 5), np.float32), np.zeros((cap, 32), np.uint8), np.zeros(cap, synth.IMMATURE_DTYPE), np.zeros(4, np.int32)
    adapter._chk(adapter.A.adp_make_new_traces(adapter.h, r.fs_handle(), fh, _p(pat), C.c_int(n), None, C.c_int(cap), _p(feat), _p(desc), _p(imm), _p(counts)))
    return imm[:int(counts[3])].copy(), counts


def test_make_new_traces_appends_on_the_device():
    """makeNewTraces in resident mode: the fresh records go behind the tracer's rows device to device, the features it drops (non-finite energyTH: a NaN pixel
    under the pattern) leave by one compaction mask, and the host objects are what the transferring leg builds.  The frame is not a key frame of the window here,
    so its rows leave again at the next reconcile - by the compaction branch, not by an upload."""
    import activation_select_common as asc
    import feature_detect_common as fc
    win, (r_off, r_on), pts = asc.make_state("small", per_frame=100, P=150, n_graphs=2)
    F = win.F
    A_off, A_on = _pair(win)
    legs = ((A_off, r_off), (A_on, r_on))
    for A, r in legs:
        _trace(A, r, win, F)
    clean = np.ascontiguousarray(win.images[F + 1][0], np.float32)
    W0 = fc.detect(clean, 300, None, fc.golden()["pattern"])["features"]
    irr = clean[..., 0].copy()
    irr[int(W0["v"][40]), int(W0["u"][40])] = np.nan
    dI = synth.make_images(irr, 1)[0]
    T = win.truth["w2c"][F + 1]
    out = [_make_new_traces(A, r, r.fs_new_frame(dI, T, 0.0, 0.0), 300) for A, r in legs]
    assert np.array_equal(out[0][1], out[1][1]) and out[0][0].tobytes() == out[1][0].tobytes()
    assert out[0][1][2] > 0 and out[0][1][3] > 100, "features were dropped and features were kept"
    assert _counts(A_on) == (1, 0, 1)
    c = [_trace(A, r, win, F + 1) for A, r in legs]
    assert np.array_equal(c[0], c[1]) and c[0].sum() == len(pts)
    assert _counts(A_on) == (1, 1, 1)
    _sync(A_on, r_on)
    _assert_graphs_equal(r_off, r_on, "after makeNewTraces and a trace")
    for A, r in legs:
        A.close(); r.close()
    r_off.L.ref_fs_release_new_frames()


def _make_new_traces_window(adapter, r, frame_idx, n):
    """GpuBackend::makeNewTraces on a key frame of the window, behind the features it has -> counts: detected, corners, dropped, features of the frame"""
    import feature_detect_common as fc
    pat = np.ascontiguousarray(fc.golden()["pattern"], np.int32)
    counts = np.zeros(4, np.int32)
    adapter._chk(adapter.A.adp_make_new_traces_window(adapter.h, r.fs_handle(), C.c_int(frame_idx), _p(pat), C.c_int(n), _p(counts)))
    return counts


@pytest.mark.parametrize("min_capacity", [None, 64], ids=["roomy", "grows"])
def test_detection_to_activation_without_an_upload(min_capacity):
    """makeNewTraces, trace, activatePointsMT, makeNewTraces, trace, sync with the new points on the newest key frame of the window: the resident leg ends equal to
    the transferring one.  With room in the tracer the set goes up once (the state's host-built points, at the first call) and never again: the fresh records are
    appended device to device and traced where they lie.  With a tracer made too small for the first batch (700 wanted on 500 rows of 1000) the backend brings the
    device state home, makes a larger tracer and uploads once more - and appends the second batch."""
    import activation_select_common as asc
    win, (r_off, r_on), pts = asc.make_state("small", per_frame=100, P=150, n_graphs=2)
    F = win.F
    A_off, A_on = _pair(win)
    if min_capacity is not None:
        assert pr.adapter_lib().adp_set_tracer_min_capacity(A_on.h, C.c_int(min_capacity)) == 0
    legs = ((A_off, r_off), (A_on, r_on))
    n_imm = len(pts)
    grown = min_capacity is not None
    expect = []                                   # reconcile counters of the resident leg after every step
    # makeNewTraces: the reconcile at its head uploads the state's points (the tracer is made here), the fresh ones follow on the device
    m = [_make_new_traces_window(A, r, F - 1, 700) for A, r in legs]
    assert np.array_equal(m[0], m[1]) and m[0][0] > 500 and m[0][2] == 0
    n_imm += int(m[0][0])
    assert n_imm > 2 * len(pts), "the first batch outgrows a tracer made for twice the state's points"
    assert _counts(A_on) == (0, 0, 1)
    c = [_trace(A, r, win, F) for A, r in legs]
    assert np.array_equal(c[0], c[1]) and c[0].sum() == n_imm
    assert _counts(A_on) == ((0, 0, 2) if grown else (1, 0, 1))
    s = [asc.adapter_activate_points_mt(A, r) for A, r in legs]
    assert s[0] == s[1] and s[0][1] > 30 and s[0][0] == len(pts) - 100, "the newest frame's points, old and fresh, are no candidates"
    m = [_make_new_traces_window(A, r, F - 1, 300) for A, r in legs]
    assert np.array_equal(m[0], m[1]) and m[0][0] > 100
    c = [_trace(A, r, win, F + 1) for A, r in legs]
    assert np.array_equal(c[0], c[1]) and c[0].sum() > n_imm - s[0][0]
    assert _counts(A_on) == ((3, 0, 2) if grown else (4, 0, 1)), "no upload after the first" + (" but the one the growth costs" if grown else "")
    _sync(A_on, r_on)
    _assert_graphs_equal(r_off, r_on, "after two rounds of new traces")
    a, b = r_off.fs_get_immature(), r_on.fs_get_immature()
    assert a.tobytes() == b.tobytes() and (a["host"] == F - 1).sum() > 700 and (a["lastTraceStatus"][a["host"] == F - 1] != 5).all(), "the fresh points were traced"
    for A, r in legs:
        A.close(); r.close()
    r_off.L.ref_fs_release_new_frames()
