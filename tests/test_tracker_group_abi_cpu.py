"""ldso_tr_group_* and ldso_tr_coop_width (include/ldso_hip.h) without a device: the entries are exported by the built library and declared in the header, refuse a
NULL group / an empty tracker list before they touch the runtime, the binding offers them, and the launch-shape rule of a track (how many workgroups share each of
`count` concurrent tracks) is the chain the tracker has always used, with every cooperative shape resident on the device it was asked for."""
import ctypes as C
import os
import re

import pytest

from ldso_amd import binding

LDSO_OK, LDSO_E_INVALID = 0, -1
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "ldso_hip.h")
ENTRIES = ("ldso_tr_group_create", "ldso_tr_group_destroy", "ldso_tr_group_coop_width", "ldso_tr_group_track", "ldso_tr_group_track_new_coarse", "ldso_tr_coop_width")


@pytest.mark.parametrize("entry", ENTRIES)
def test_entry_is_exported_and_declared(entry):
    assert hasattr(binding.lib(), entry)
    assert re.search(r"\bint\s+%s\s*\(" % entry, open(HEADER).read())


@pytest.mark.parametrize("entry,nargs", [("ldso_tr_group_track", 10), ("ldso_tr_group_track_new_coarse", 14)])
def test_null_group_is_refused_with_a_message(entry, nargs):
    L = binding.lib()
    f = getattr(L, entry)
    f.restype = C.c_int
    f.argtypes = [C.c_void_p] * nargs
    assert f(*([None] * nargs)) == LDSO_E_INVALID
    assert entry in L.ldso_last_error().decode()


def test_empty_tracker_list_is_refused_with_a_message():
    L = binding.lib()
    out = C.c_void_p()
    L.ldso_tr_group_create.restype = C.c_int
    assert L.ldso_tr_group_create(None, C.c_int(0), C.byref(out)) == LDSO_E_INVALID
    assert "ldso_tr_group_create" in L.ldso_last_error().decode()
    assert not out.value


@pytest.mark.parametrize("method", ("track", "track_new_coarse", "coop_width", "close"))
def test_binding_offers_the_method(method):
    assert callable(getattr(binding.TrackerGroup, method, None))


def chain(nhyp, numCU):
    """the rule as ldso_tr_track_batch has always spelled it"""
    return 16 if nhyp * 16 <= numCU else 12 if nhyp * 12 <= numCU else 8 if nhyp * 8 <= numCU else 4 if nhyp * 4 <= numCU else 1


@pytest.mark.parametrize("num_cu", (64, 256, 304))
def test_coop_width_is_the_trackers_chain_and_stays_resident(num_cu, monkeypatch):
    monkeypatch.delenv("LDSO_TR_NO_COOP", raising=False)
    L = binding.lib()
    for count in range(1, 129):
        G = C.c_int(-1)
        assert L.ldso_tr_coop_width(C.c_int(count), C.c_int(num_cu), C.byref(G)) == LDSO_OK
        assert G.value in (16, 12, 8, 4, 1), (count, num_cu, G.value)
        assert G.value == 1 or count * G.value <= num_cu, (count, num_cu, G.value)
        assert G.value == chain(count, num_cu), (count, num_cu, G.value)
        assert binding.coop_width(count, num_cu) == G.value


def test_coop_width_refuses_bad_arguments():
    L = binding.lib()
    G = C.c_int(-1)
    assert L.ldso_tr_coop_width(C.c_int(0), C.c_int(256), C.byref(G)) == LDSO_E_INVALID
    assert L.ldso_tr_coop_width(C.c_int(1), C.c_int(256), None) == LDSO_E_INVALID
    assert "ldso_tr_coop_width" in L.ldso_last_error().decode()
