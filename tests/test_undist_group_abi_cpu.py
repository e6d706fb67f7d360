"""ldso_undist_group_* (include/ldso_hip.h) without a device: the entries are exported by the built library and declared in the header, refuse a NULL group / an
empty or oversized member list before they touch the runtime, and the binding offers them."""
import ctypes as C
import os
import re

import pytest

from ldso_amd import binding

LDSO_OK, LDSO_E_INVALID = 0, -1
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "ldso_hip.h")
ENTRIES = ("ldso_undist_group_create", "ldso_undist_group_destroy", "ldso_undist_group_frames", "ldso_undist_group_profile")


@pytest.mark.parametrize("entry", ENTRIES)
def test_entry_is_exported_and_declared(entry):
    assert hasattr(binding.lib(), entry)
    assert re.search(r"\bint\s+%s\s*\(" % entry, open(HEADER).read())


def test_header_names_the_reference_lines():
    """in the comment right above the group's typedef"""
    text = open(HEADER).read()
    end = text.index("typedef struct ldso_undist_group ")
    comment = text[text.rindex("/*", 0, end):end]
    assert "Undistort.cc:357-457" in comment


@pytest.mark.parametrize("entry,nargs", [("ldso_undist_group_frames", 8), ("ldso_undist_group_profile", 3)])
def test_null_group_is_refused_with_a_message(entry, nargs):
    L = binding.lib()
    f = getattr(L, entry)
    f.restype = C.c_int
    f.argtypes = [C.c_void_p] * nargs
    assert f(*([None] * nargs)) == LDSO_E_INVALID
    assert entry in L.ldso_last_error().decode()


def test_create_refuses_bad_member_lists():
    L = binding.lib()
    entry = "ldso_undist_group_create"
    f = getattr(L, entry)
    f.restype = C.c_int
    out = C.c_void_p()
    assert f(None, C.c_int(0), C.byref(out)) == LDSO_E_INVALID
    assert entry in L.ldso_last_error().decode()
    assert not out.value
    empty = (C.c_void_p * 1)()
    assert f(empty, C.c_int(0), C.byref(out)) == LDSO_E_INVALID and not out.value
    assert f(empty, C.c_int(1), C.byref(out)) == LDSO_E_INVALID and not out.value          # a NULL member
    assert entry in L.ldso_last_error().decode()
    assert f(empty, C.c_int(129), C.byref(out)) == LDSO_E_INVALID and not out.value
    assert f(empty, C.c_int(1), None) == LDSO_E_INVALID


def test_group_destroy_of_null_is_a_no_op():
    assert binding.lib().ldso_undist_group_destroy(None) == LDSO_OK


@pytest.mark.parametrize("method", ("frames", "profile", "close"))
def test_binding_offers_the_method(method):
    assert callable(getattr(getattr(binding, "UndistorterGroup", None), method, None))
