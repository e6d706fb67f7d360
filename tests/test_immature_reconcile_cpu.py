"""The decision GpuBackend::reconcileImmature takes at the head of traceNewCoarse, activatePointsMT and makeNewTraces (adapter/adapter_internal.h:
adp::planReconcile, through adp_reconcile_plan of adapter/adapter_capi.cc) as a function of plain data, without a GPU: the tracer's rows against the graph's
current list of immature points, each a (point id, host index) pair.  The outcome, the keep mask and the WHOLE host map are asserted."""
import ctypes as C

import numpy as np
import pytest

from ldso_amd import binding

SAME, COMPACT, REUPLOAD = 0, 1, 2
MF = binding.MAX_FRAMES
A, B, C_, D = 11, 12, 13, 14
UNTOUCHED = -7


def _plan(rows, cur, tracer=True):
    from oracle import pyref as pr
    if not (pr.available() and pr.adapter_available()):
        pytest.skip("oracle/_ref/libldso_ref.so / adapter/_build/libldso_adapter_test.so not built")
    lib = pr.adapter_lib()
    r = np.asarray(rows, np.int32).reshape(-1, 2); c = np.asarray(cur, np.int32).reshape(-1, 2)
    rid, rhost = np.ascontiguousarray(r[:, 0]), np.ascontiguousarray(r[:, 1])
    cid, chost = np.ascontiguousarray(c[:, 0]), np.ascontiguousarray(c[:, 1])
    keep = np.full(max(len(r), 1), 255, np.uint8); host_map = np.full(MF, UNTOUCHED, np.int32)
    out = lib.adp_reconcile_plan(C.c_int(len(r)), binding._p(rid), binding._p(rhost), C.c_int(len(c)), binding._p(cid), binding._p(chost), C.c_int(1 if tracer else 0),
                                 binding._p(keep), binding._p(host_map))
    return out, keep[:len(r)].tolist(), host_map.tolist()


def _map(**pairs):
    m = [-1] * MF
    for old, new in pairs.items():
        m[int(old[1:])] = new
    return m


ROWS3 = [(A, 0), (B, 0), (C_, 1)]

COMPACT_CASES = [
    # rows, current, keep, host map
    pytest.param(ROWS3, [(A, 0), (C_, 1)], [1, 0, 1], _map(h0=0, h1=1), id="2-a-point-released"),
    pytest.param([(A, 1), (B, 2)], [(A, 0), (B, 1)], [1, 1], _map(h1=0, h2=1), id="3-a-frame-in-front-left"),
    pytest.param([(A, 0), (B, 0)], [], [0, 0], _map(), id="10-current-list-empty"),
]

REUPLOAD_CASES = [
    pytest.param([(A, 1), (B, 1)], [(A, 0), (B, 2)], True, id="4-one-old-host-to-two-new-ones"),
    pytest.param([(A, 0), (B, 0)], [(B, 0), (A, 0)], True, id="5-order-changed"),
    pytest.param([(A, 0), (B, 0)], [(A, 0), (D, 0)], True, id="6-a-point-the-device-has-not-seen"),
    pytest.param([(A, 0), (B, 0)], [(A, 0), (B, 0), (C_, 0)], True, id="7-longer-than-the-rows"),
    pytest.param([(A, MF)], [(A, 0)], True, id="8-old-host-index-outside-the-map"),
    pytest.param(ROWS3, ROWS3, False, id="9-no-tracer"),
]


def test_same_list_is_same():
    """case 1: nothing is uploaded; mask and map are not written"""
    out, keep, host_map = _plan(ROWS3, ROWS3)
    assert out == SAME
    assert keep == [255] * 3 and host_map == [UNTOUCHED] * MF


@pytest.mark.parametrize("rows,cur,want_keep,want_map", COMPACT_CASES)
def test_ordered_subsequence_compacts(rows, cur, want_keep, want_map):
    out, keep, host_map = _plan(rows, cur)
    assert out == COMPACT
    assert keep == want_keep
    assert host_map == want_map


@pytest.mark.parametrize("rows,cur,tracer", REUPLOAD_CASES)
def test_anything_else_uploads_anew(rows, cur, tracer):
    out, keep, host_map = _plan(rows, cur, tracer)
    assert out == REUPLOAD
    assert keep == [255] * len(rows) and host_map == [UNTOUCHED] * MF, "mask and map are written for a compaction only"


def test_null_outputs_are_refused():
    from oracle import pyref as pr
    if not (pr.available() and pr.adapter_available()):
        pytest.skip("oracle/_ref/libldso_ref.so / adapter/_build/libldso_adapter_test.so not built")
    one = np.zeros(1, np.int32)
    assert pr.adapter_lib().adp_reconcile_plan(C.c_int(1), binding._p(one), binding._p(one), C.c_int(1), binding._p(one), binding._p(one), C.c_int(1), None, None) == -1
