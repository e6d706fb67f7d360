"""ldso_ba_batch_optimize (include/ldso_hip.h) without a device: the entry is exported, refuses a NULL batch before it touches the runtime, and the binding offers it."""
import ctypes as C

from ldso_amd import binding

LDSO_E_INVALID = -1


def test_entry_is_exported():
    assert hasattr(binding.lib(), "ldso_ba_batch_optimize")


def test_null_batch_is_refused_with_a_message():
    L = binding.lib()
    L.ldso_ba_batch_optimize.restype = C.c_int
    rc = L.ldso_ba_batch_optimize(None, C.c_int(6), C.c_int(0), None, None, None)
    assert rc == LDSO_E_INVALID
    assert "ldso_ba_batch_optimize" in L.ldso_last_error().decode()


def test_binding_offers_optimize():
    assert callable(getattr(binding.BABatch, "optimize", None))
