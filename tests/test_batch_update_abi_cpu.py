"""ldso_ba_batch_update_windows / ldso_ba_batch_set_frames (include/ldso_hip.h) without a device: the entries are exported by the built library and declared in the
header, refuse a NULL batch before they touch the runtime, the binding offers them, and its job records have the layout of the C structs (the library pins the same
sizes with a static_assert beside the entries, csrc/ba_window.hip)."""
import ctypes as C
import os
import re

import pytest

from ldso_amd import binding

LDSO_E_INVALID = -1
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "ldso_hip.h")
ENTRIES = ("ldso_ba_batch_update_windows", "ldso_ba_batch_set_frames")


@pytest.mark.parametrize("entry", ENTRIES + ("ldso_ba_batch_balanced", "ldso_ba_get_prior"))
def test_entry_is_exported_and_declared(entry):
    assert hasattr(binding.lib(), entry)
    assert re.search(r"\bint\s+%s\s*\(" % entry, open(HEADER).read())


@pytest.mark.parametrize("entry", ENTRIES)
def test_null_batch_is_refused_with_a_message(entry):
    L = binding.lib()
    f = getattr(L, entry)
    f.restype = C.c_int
    assert f(None, None) == LDSO_E_INVALID
    assert entry in L.ldso_last_error().decode()


@pytest.mark.parametrize("method", ("update_windows", "set_frames", "balanced"))
def test_binding_offers_the_method(method):
    assert callable(getattr(binding.BABatch, method, None))


def c_struct_fields(name):
    """(type, field) pairs of `typedef struct { ... } name;` in the header, in order"""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*%s\s*;" % name, src).group(1)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        first, *rest = [d.strip() for d in decl.split(",")]
        m = re.match(r"(.*?)(\**)\s*(\w+)$", first)
        base = m.group(1).strip()
        out.append((base + m.group(2), m.group(3)))
        for r in rest:
            m2 = re.match(r"(\**)\s*(\w+)$", r)
            out.append((base + m2.group(1), m2.group(2)))
    return out


@pytest.mark.parametrize("cname,record,size", [("ldso_win_job_t", binding.WinJob, 96), ("ldso_frames_job_t", binding.FramesJob, 32)])
def test_job_record_matches_the_header(cname, record, size):
    """field for field: the same names in the same order, an int where the header has an int and a pointer where it has one; sizeof on a 64-bit host"""
    fields = c_struct_fields(cname)
    assert [f for _, f in fields] == [f for f, _ in record._fields_]
    for (ctype_c, fname), (_, ctype_py) in zip(fields, record._fields_):
        assert (ctype_py is C.c_void_p) == ctype_c.endswith("*"), fname
        assert (ctype_py is C.c_int) == (ctype_c == "int"), fname
    assert C.sizeof(record) == size
    if record is binding.WinJob:
        assert record.P.offset == 24 and record.n_fresh.offset == 48 and record.n_fresh_res.offset == 64 and record.fresh_ngr.offset == 88
    else:
        assert record.HM.offset == 16 and record.bM.offset == 24
