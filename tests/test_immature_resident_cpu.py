"""The entry points of the resident immature set without a GPU: null or invalid arguments are refused with LDSO_E_INVALID before anything touches a device,
and where no device is visible a backend cannot exist.  That every declared symbol is exported is tests/test_abi.py's business."""
import ctypes as C

import numpy as np
import pytest

from ldso_amd import binding

E_INVALID = -1


def _null():
    return C.c_void_p(None)


def test_tracer_entries_refuse_null_arguments():
    L = binding.lib()
    buf = np.zeros(4, np.float32)
    n = C.c_int(-7)
    assert L.ldso_trace_set_point_types(_null(), binding._p(buf)) == E_INVALID
    assert L.ldso_trace_get_point_types(_null(), binding._p(buf)) == E_INVALID
    assert L.ldso_trace_compact(_null(), None, C.c_int(4), None, C.byref(n)) == E_INVALID
    assert n.value == -7, "a refused call writes nothing"
    assert b"ldso_trace_compact" in L.ldso_last_error()


def test_select_activate_tracer_refuses_null_handles():
    L = binding.lib()
    K = np.zeros((4, 9), np.float32); t = np.zeros((4, 3), np.float32); fl = np.zeros(4, np.int32)
    ns, left = C.c_int(-7), C.c_int(-7)
    rc = L.ldso_ba_select_activate_tracer(_null(), _null(), C.c_int(4), binding._p(K), binding._p(t), binding._p(fl), C.c_float(1.0), C.c_float(3.0), C.c_int(1), C.c_float(100.0),
                                          C.c_int(3), C.c_int(1), None, None, C.byref(ns), None, C.byref(left))
    assert rc == E_INVALID and ns.value == -7 and left.value == -7
    assert b"ldso_ba_select_activate_tracer" in L.ldso_last_error()


def test_adapter_entries_refuse_null_backend():
    """adp_set_resident_immature / adp_sync_immature / adp_immature_reconcile_counts (adapter/adapter_capi.cc) with no backend: LDSO_E_INVALID, nothing written"""
    from oracle import pyref as pr
    if not (pr.available() and pr.adapter_available()):
        pytest.skip("oracle/_ref/libldso_ref.so / adapter/_build/libldso_adapter_test.so not built")
    A = pr.adapter_lib()
    out = np.full(3, -7, np.int32)
    assert A.adp_set_resident_immature(_null(), C.c_int(1)) == E_INVALID
    assert A.adp_sync_immature(_null(), _null()) == E_INVALID
    assert A.adp_immature_reconcile_counts(_null(), binding._p(out)) == E_INVALID and (out == -7).all()
    assert A.adp_set_tracer_min_capacity(_null(), C.c_int(64)) == E_INVALID
    assert A.adp_make_new_traces_window(_null(), _null(), C.c_int(0), None, C.c_int(100), binding._p(out)) == E_INVALID and (out == -7).all()
    if binding.lib().ldso_device_count() == 0:
        assert not A.adp_create(C.c_int(0), C.c_int(8), C.c_int(64)), "no backend without a device"
