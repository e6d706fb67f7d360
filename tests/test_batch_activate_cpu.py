"""ldso_ba_batch_activate_points / ldso_ba_batch_select_candidates / ldso_ba_batch_select_activate_points (include/ldso_hip.h) without a device: the entries are
exported, refuse a NULL batch before they touch the runtime, and the binding offers them."""
import ctypes as C

import pytest

from ldso_amd import binding

LDSO_E_INVALID = -1
# entry -> the arguments behind the batch
ENTRIES = {
    "ldso_ba_batch_activate_points": (None, None, C.c_int(1), C.c_float(100.0), C.c_int(3), None),
    "ldso_ba_batch_select_candidates": (None, C.c_float(3.0)),
    "ldso_ba_batch_select_activate_points": (None, C.c_float(3.0), C.c_int(1), C.c_float(100.0), C.c_int(3)),
}


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_entry_is_exported(entry):
    assert hasattr(binding.lib(), entry)


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_null_batch_is_refused_with_a_message(entry):
    L = binding.lib()
    f = getattr(L, entry)
    f.restype = C.c_int
    rc = f(None, *ENTRIES[entry])
    assert rc == LDSO_E_INVALID
    assert entry in L.ldso_last_error().decode()


@pytest.mark.parametrize("method", ("activate_points", "select_candidates", "select_activate_points"))
def test_binding_offers_the_method(method):
    assert callable(getattr(binding.BABatch, method, None))


def test_job_record_matches_the_header():
    """ldso_act_job_t on a 64-bit host: 4 ints, a float and 9 pointers with their padding"""
    assert C.sizeof(binding.ActJob) == 112
    assert binding.ActJob.n_hosts.offset == 40 and binding.ActJob.currentMinActDist.offset == 72 and binding.ActJob.n_selected.offset == 96 and binding.ActJob.out.offset == 104
