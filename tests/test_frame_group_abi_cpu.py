"""ldso_trace_group_*, ldso_pyr_group_*, ldso_trace_set_stream and ldso_trace_group_member_of (include/ldso_hip.h) without a device: the entries are exported by the
built library and declared in the header, refuse a NULL group / an empty member list before they touch the runtime, the binding offers them, and the member-lookup
rule of a grouped launch (which job owns wavefront `wave` under the prefix `first`) holds for every count vector of length 1..5 with entries 0..5."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

from ldso_amd import binding

LDSO_OK, LDSO_E_INVALID = 0, -1
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "ldso_hip.h")
ENTRIES = ("ldso_trace_set_stream", "ldso_trace_group_member_of", "ldso_trace_group_create", "ldso_trace_group_destroy", "ldso_trace_group_on",
           "ldso_pyr_group_create", "ldso_pyr_group_destroy", "ldso_pyr_group_make_images", "ldso_pyr_group_make_images_device")


@pytest.mark.parametrize("entry", ENTRIES)
def test_entry_is_exported_and_declared(entry):
    assert hasattr(binding.lib(), entry)
    assert re.search(r"\bint\s+%s\s*\(" % entry, open(HEADER).read())


def test_header_names_the_reference_lines():
    """in the comment right above each group's typedef"""
    text = open(HEADER).read()
    for typedef, lines in (("typedef struct ldso_trace_group ", ("FullSystem.cc:1012-1050", "ImmaturePoint.cc:47-310")), ("typedef struct ldso_pyr_group ", ("FrameHessian.cc:44-113",))):
        end = text.index(typedef)
        comment = text[text.rindex("/*", 0, end):end]
        for ref in lines:
            assert ref in comment, (typedef, ref)


@pytest.mark.parametrize("entry,nargs", [("ldso_trace_group_on", 7), ("ldso_pyr_group_make_images", 4), ("ldso_pyr_group_make_images_device", 4), ("ldso_trace_set_stream", 2)])
def test_null_handle_is_refused_with_a_message(entry, nargs):
    L = binding.lib()
    f = getattr(L, entry)
    f.restype = C.c_int
    f.argtypes = [C.c_void_p] * nargs
    assert f(*([None] * nargs)) == LDSO_E_INVALID
    assert entry in L.ldso_last_error().decode()


@pytest.mark.parametrize("entry", ("ldso_trace_group_create", "ldso_pyr_group_create"))
def test_empty_member_list_is_refused_with_a_message(entry):
    L = binding.lib()
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


def test_group_destroy_of_null_is_a_no_op():
    L = binding.lib()
    assert L.ldso_trace_group_destroy(None) == LDSO_OK and L.ldso_pyr_group_destroy(None) == LDSO_OK


@pytest.mark.parametrize("cls,method", [("Tracer", "set_stream"), ("TracerGroup", "trace_on"), ("TracerGroup", "close"), ("PyramidGroup", "make_images"),
                                        ("PyramidGroup", "make_images_device"), ("PyramidGroup", "close")])
def test_binding_offers_the_method(cls, method):
    assert callable(getattr(getattr(binding, cls, None), method, None))


def member_of(first, wave):
    L = binding.lib()
    job = C.c_int(-7)
    rc = L.ldso_trace_group_member_of(binding._p(first), C.c_int(len(first) - 1), C.c_int(wave), C.byref(job))
    return rc, job.value


@pytest.mark.parametrize("length", (1, 2, 3, 4, 5))
def test_member_lookup_is_exhaustively_right(length):
    """every wave index in [0, total) maps to the member whose range holds it (members without points are skipped wherever they stand); outside it is refused"""
    for counts in itertools.product(range(6), repeat=length):
        first = np.zeros(length + 1, np.int32)
        first[1:] = np.cumsum(counts)
        total = int(first[-1])
        owner = [j for j, c in enumerate(counts) for _ in range(c)]
        for wave in range(total):
            rc, job = member_of(first, wave)
            assert rc == LDSO_OK and job == owner[wave], (counts, wave, job)
            assert first[job] <= wave < first[job + 1]
        for wave in (total, total + 1, -1):
            rc, job = member_of(first, wave)
            assert rc == LDSO_E_INVALID and job == -7, (counts, wave)


def test_member_lookup_refuses_bad_arguments():
    L = binding.lib()
    job = C.c_int()
    first = np.array([0, 2, 1], np.int32)          # decreasing
    assert L.ldso_trace_group_member_of(binding._p(first), C.c_int(2), C.c_int(0), C.byref(job)) == LDSO_E_INVALID
    assert "ldso_trace_group_member_of" in L.ldso_last_error().decode()
    ok = np.array([0, 2, 3], np.int32)
    assert L.ldso_trace_group_member_of(None, C.c_int(2), C.c_int(0), C.byref(job)) == LDSO_E_INVALID
    assert L.ldso_trace_group_member_of(binding._p(ok), C.c_int(2), C.c_int(0), None) == LDSO_E_INVALID
    assert L.ldso_trace_group_member_of(binding._p(ok), C.c_int(0), C.c_int(0), C.byref(job)) == LDSO_E_INVALID
