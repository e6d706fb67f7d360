"""ldso_ba_batch_marginalize_points / ldso_ba_batch_marginalize_frame (include/ldso_hip.h) without a device: the entries are exported, refuse a NULL batch before
they touch the runtime, and the binding offers them."""
import ctypes as C

import pytest

from ldso_amd import binding

LDSO_E_INVALID = -1
ENTRIES = ("ldso_ba_batch_marginalize_points", "ldso_ba_batch_marginalize_frame")


@pytest.mark.parametrize("entry", ENTRIES)
def test_entry_is_exported(entry):
    assert hasattr(binding.lib(), entry)


@pytest.mark.parametrize("entry", ENTRIES)
def test_null_batch_is_refused_with_a_message(entry):
    L = binding.lib()
    f = getattr(L, entry)
    f.restype = C.c_int
    rc = f(None, None, None, None)
    assert rc == LDSO_E_INVALID
    assert entry in L.ldso_last_error().decode()


@pytest.mark.parametrize("method", ("marginalize_points", "marginalize_frame"))
def test_binding_offers_the_method(method):
    assert callable(getattr(binding.BABatch, method, None))
