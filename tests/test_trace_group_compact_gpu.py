"""ldso_trace_group_compact: ldso_trace_compact of many tracers in two launches (k_compact_count_group / k_compact_move_group, ldso_amd/csrc/trace.hip).  Every
active member's records, types and count are those of a twin tracer's own ldso_trace_compact from the same input, byte for byte: the grouped kernels run the device
functions of the solo kernels on the same bytes, so no tolerance applies.  Seven members with 0, 1, 64, 255, 257, 1025 and 4097 records (below, at and above the
wavefront and the 256-record workgroup; 17 workgroups of one member beside single ones; a member without records, which has no workgroup), built as
tests/test_immature_resident_gpu.py builds its records: hosts mixed, every record recognisable.  The masks of that file cycle over the members, so one call mixes
keep bytes, host maps, both and neither."""
import numpy as np
import pytest

from ldso_amd import binding
from test_immature_resident_gpu import _base, _records, _masks, _expected
from test_trace_group_gpu import stream

pytestmark = pytest.mark.gpu

COUNTS = (0, 1, 64, 255, 257, 1025, 4097)
MAX_POINTS = (16, 1, 100, 300, 1000, 2048, 4097)          # every member its own capacity (>= its count): the workgroup counts of each lie in its own tracer
INACTIVE = 4
N_MASKS = 9


def members(st):
    """-> (tracers on the stream, their twins on streams of their own, the records and types they hold)"""
    win, _, _ = _base()
    trk, twin, data = [], [], []
    for n, cap in zip(COUNTS, MAX_POINTS):
        pts, types = _records(n)
        pair = []
        for s in (st, None):
            t = binding.Tracer(win.w, win.h, cap)
            if s is not None:
                t.set_stream(s)
            t.set_points(pts); t.set_point_types(types)
            pair.append(t)
        trk.append(pair[0]); twin.append(pair[1]); data.append((pts, types))
    return trk, twin, data


def state(t):
    return t.n, t.get_points().tobytes(), t.get_point_types().tobytes()


def masks_for(trk, F, shift, rng):
    """member i gets mask (i + shift) mod 9 of _masks for its current count -> (names, keeps, maps)"""
    names, keeps, maps = [], [], []
    for i, t in enumerate(trk):
        name, keep, hmap = _masks(t.n, F, rng)[(i + shift) % N_MASKS]
        names.append(name); keeps.append(keep); maps.append(hmap)
    return names, keeps, maps


def close_all(grp, *lists):
    grp.close()
    for l in lists:
        for t in l:
            t.close()


def test_group_equals_solo_compactions_with_mixed_masks_and_an_inactive_member():
    st = stream()
    F = _base()[0].F
    trk, twin, data = members(st)
    grp = binding.TracerGroup(trk)
    active = [i != INACTIVE for i in range(len(trk))]
    rng = np.random.default_rng(5)
    seen = set()
    for rnd, shift in enumerate((0, 2, 1)):          # members 5 and 6, the large ones: alternating / random, then host-map / mask+map, then random / host-map; the second and third call work on the already compacted group: the members' buffers really swapped
        names, keeps, maps = masks_for(trk, F, shift, rng)
        before = state(trk[INACTIVE])
        left = grp.compact(keeps, maps, n_hosts=[F] * len(trk), active=active)
        for i, t in enumerate(trk):
            if i == INACTIVE:
                assert state(t) == before and left[i] == before[0], "the inactive member is untouched"
                continue
            had = twin[i].n
            want_n = twin[i].compact(keeps[i], maps[i], n_hosts=F)
            assert left[i] == want_n == t.n, (rnd, i, names[i], left[i], want_n)
            assert state(t) == state(twin[i]), (rnd, i, names[i])
            seen.add((names[i], had > 0, 0 < want_n < had))
    assert trk[INACTIVE].n == COUNTS[INACTIVE]
    # the calls did work of every kind: a mask, a map and both each removed a part of a non-empty member's records
    for name in ("alternating", "random", "host-map", "mask+map"):
        assert (name, True, True) in seen, (name, sorted(seen))
    close_all(grp, trk, twin)


def test_first_call_equals_the_numpy_restatement():
    st = stream()
    F = _base()[0].F
    trk, twin, data = members(st)
    grp = binding.TracerGroup(trk)
    keeps, maps, names = [], [], []
    for i, (pts, types) in enumerate(data):
        name, keep, hmap = _masks(len(pts), F, np.random.default_rng(20 + i))[(i + 5) % N_MASKS]
        names.append(name); keeps.append(keep); maps.append(hmap)
    assert {"host-map", "mask+map", "random"} <= set(names)
    left = grp.compact(keeps, maps, n_hosts=[F] * len(trk))
    for i, (pts, types) in enumerate(data):
        want, want_t = _expected(pts, types, keeps[i], maps[i], F)
        assert left[i] == len(want) == trk[i].n, (i, names[i])
        assert trk[i].get_points().tobytes() == want.tobytes() and np.array_equal(trk[i].get_point_types(), want_t), (i, names[i])
    # keeps and maps left out altogether: everything whose host is a frame stays
    before = [state(t) for t in trk]
    left = grp.compact(n_hosts=[F] * len(trk))
    assert [state(t) for t in trk] == before and list(left) == [b[0] for b in before]
    close_all(grp, trk, twin)


def test_every_member_empty():
    st = stream()
    win, _, _ = _base()
    trk = []
    for cap in (1, 300, 5000):
        t = binding.Tracer(win.w, win.h, cap)
        t.set_stream(st)
        trk.append(t)
    grp = binding.TracerGroup(trk)
    left = np.full(3, -7, np.int32)
    nh = np.full(3, win.F, np.int32)
    assert grp.L.ldso_trace_group_compact(grp.h, None, None, binding._p(nh), None, binding._p(left)) == 0
    assert list(left) == [0, 0, 0] and all(t.n == 0 for t in trk)
    # ... and with one of them inactive its row of n_out is left alone
    left[:] = -7
    act = np.array([1, 0, 1], np.uint8)
    assert grp.L.ldso_trace_group_compact(grp.h, binding._p(act), None, binding._p(nh), None, binding._p(left)) == 0
    assert list(left) == [0, -7, 0]
    close_all(grp, trk)


def test_refusals_leave_every_member_as_it_was():
    st = stream()
    F = _base()[0].F
    trk, twin, data = members(st)
    grp = binding.TracerGroup(trk)
    before = [state(t) for t in trk]
    n = len(trk)
    rng = np.random.default_rng(9)
    _, keeps, maps = masks_for(trk, F, 6, rng)

    def refused(call, *words):
        with pytest.raises(binding.LdsoError) as e:
            call()
        assert e.value.code == binding.E_INVALID and "ldso_trace_group_compact" in str(e.value), str(e.value)
        for w in words:
            assert w in str(e.value), (w, str(e.value))
        assert [state(t) for t in trk] == before, words

    for bad in (0, binding.MAX_FRAMES + 1, -1):
        nh = [F] * n; nh[5] = bad
        refused(lambda: grp.compact(keeps, maps, n_hosts=nh), "member 5", "n_hosts")
    far = [None] * n
    far[2] = np.arange(F, dtype=np.int32); far[2][F - 1] = binding.MAX_FRAMES
    refused(lambda: grp.compact(keeps, far, n_hosts=[F] * n), "member 2", "LDSO_MAX_FRAMES")
    # an inactive member's arguments are not looked at
    nh = [F] * n; nh[INACTIVE] = 0
    active = [i != INACTIVE for i in range(n)]
    none_kept = [np.zeros(t.n, np.uint8) for t in trk]
    left = grp.compact(none_kept, None, n_hosts=nh, active=active)
    assert [int(x) for x in left] == [0 if i != INACTIVE else COUNTS[INACTIVE] for i in range(n)]
    before = [state(t) for t in trk]
    assert before[INACTIVE][0] == COUNTS[INACTIVE]
    # a member moved to another stream: the group refuses until it is back
    trk[INACTIVE].set_stream(None)
    refused(lambda: grp.compact(n_hosts=[F] * n), "stream")
    refused(lambda: grp.compact(n_hosts=[F] * n, active=active), "stream")          # ... also while that member sits out
    trk[INACTIVE].set_stream(st)
    # no active member, a null n_hosts
    refused(lambda: grp.compact(n_hosts=[F] * n, active=[False] * n), "no active member")
    assert grp.L.ldso_trace_group_compact(grp.h, None, None, None, None, None) == binding.E_INVALID
    assert [state(t) for t in trk] == before
    left = grp.compact(n_hosts=[F] * n)
    assert int(left[INACTIVE]) == COUNTS[INACTIVE] and [state(t) for t in trk] == before
    close_all(grp, trk, twin)
