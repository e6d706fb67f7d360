"""ldso_trace_group_on: the traces of several tracers in one launch (k_trace_group).  A member's records and counts are those of its own ldso_trace_on from the same
input, byte for byte: the grouped kernel runs the same body (trace_point), one wavefront per point, the points of all members packed wavefront by wavefront - so a
workgroup of four wavefronts may serve two or more members, and members without points stand between them.  The members:
  "small"    the synthetic window of synth.make_config("small"), 320 x 240, 150 fresh points per key frame, default settings
  "inf99"    tests/trace_branch_common.py: the second pass of the search, the clamp at 99 steps, a non-default maxPixSearch; traced twice
  "step05"   a non-default step size on the finite intervals
  "gradnan"  its own image (NaN gradients)
  "single"   one point
  "empty"    a tracer without points
The scene members are also held against trace_branch_common.oracle(name).  All group calls run on one torch stream."""
import ctypes as C
import functools

import numpy as np
import pytest

import trace_branch_common as tb
from ldso_amd import binding, synth
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu
LDSO_OK, LDSO_E_INVALID = 0, -1
SCENE_MEMBERS = ("inf99", "step05", "gradnan", "single")


def stream():
    import torch
    ts = torch.cuda.Stream(); torch.cuda.set_stream(ts)
    return ts.cuda_stream


@functools.lru_cache(maxsize=None)
def small():
    """dict: w, h, pts, frame (level-0 image), color, poses, settings, want = [(counts, records)] of the oracle (read-only)"""
    win = synth.make_config("small", extra_frames=1)
    pts, _ = synth.make_immature_points(win, 150)
    poses = synth.trace_poses(win, win.F)
    frame = win.images[win.F][0]
    ref = pts.copy()
    counts = po.trace_on(ref, frame, *poses)
    return dict(name="small", w=win.w, h=win.h, pts=pts, frame=frame, color=np.ascontiguousarray(frame[:, :, 0]), poses=poses, settings=None,
                want=[(np.asarray(counts).copy(), ref)])


def scene_member(name, pts=None):
    sc = tb.scene()
    call = tb.get_call(name)
    return dict(name=name, w=sc["w"], h=sc["h"], pts=call["pts"] if pts is None else pts, frame=sc[call["image"]], color=sc["color"], poses=sc["hosts"],
                settings=call["settings"], want=tb.oracle(name) if pts is None else None)


def empty_member():
    sc = tb.scene()
    return dict(name="empty", w=sc["w"], h=sc["h"], pts=np.zeros(0, synth.IMMATURE_DTYPE), frame=sc["dI"], color=sc["color"], poses=sc["hosts"], settings=None, want=None)


def mixed_members():
    return [small()] + [scene_member(k) for k in SCENE_MEMBERS] + [empty_member()]


def make_tracer(m, st, frame=True):
    g = binding.Tracer(m["w"], m["h"], max(len(m["pts"]), 1), settings=m["settings"])
    if st is not None:
        g.set_stream(st)
    g.set_points(m["pts"])
    if frame:
        g.set_frame(m["frame"])
    return g


def solo(m, traces=1):
    """the member alone, on a tracer and a stream of its own -> [(counts, records)] per trace"""
    g = make_tracer(m, None)
    out = []
    for _ in range(traces):
        c = g.trace_on(*m["poses"])
        out.append((np.asarray(c).copy(), g.get_points()))
    g.close()
    return out


def close_all(grp, trk):
    grp.close()
    for g in trk:
        g.close()


def assert_member(tag, counts, records, want):
    assert np.array_equal(counts, want[0]), (tag, counts, want[0])
    assert records.tobytes() == want[1].tobytes(), tag


def test_mixed_group_equals_solo_traces_and_the_oracle_over_two_frames():
    st = stream()
    ms = mixed_members()
    trk = [make_tracer(m, st) for m in ms]
    grp = binding.TracerGroup(trk)
    alone = [solo(m, 2) for m in ms]
    for t in range(2):                                   # the second frame starts from the intervals the first one left
        counts = grp.trace_on([m["poses"] for m in ms])
        assert counts.shape == (len(ms), 6)
        for i, m in enumerate(ms):
            rec = trk[i].get_points()
            assert_member((m["name"], t, "solo"), counts[i], rec, alone[i][t])
            if m["want"] is not None and t < len(m["want"]):
                assert_member((m["name"], t, "oracle"), counts[i], rec, m["want"][t])
        assert counts[-1].sum() == 0 and counts[:-1].sum() > 0
    assert len(tb.oracle("inf99")) == 2                  # the scene's own second trace was among them
    close_all(grp, trk)


def test_workgroups_that_straddle_members():
    """counts (1, 0, 3, 0, 5, 4) cut from the `finite` records: 13 wavefronts in 4 workgroups.  Workgroup 0 holds members 0 and 2 with the empty member 1 between
    them, workgroup 2 the end of member 4 and the start of member 5; workgroup 1 lies inside member 4, behind the empty member 3"""
    st = stream()
    sizes = (1, 0, 3, 0, 5, 4)
    fin = tb.get_call("finite")["pts"]
    cuts = np.concatenate([[0], np.cumsum(sizes)])
    ms = [scene_member("finite", pts=fin[cuts[j]:cuts[j + 1]].copy()) for j in range(len(sizes))]
    first = cuts
    owners = [sorted({int(np.searchsorted(first, w, side="right")) - 1 for w in range(4 * wg, min(4 * wg + 4, 13))}) for wg in range(4)]
    assert owners == [[0, 2], [4], [4, 5], [5]], owners
    trk = [make_tracer(m, st) for m in ms]
    grp = binding.TracerGroup(trk)
    counts = grp.trace_on([m["poses"] for m in ms])
    want_c, want_r = tb.oracle("finite")[0]
    for j, m in enumerate(ms):
        rec = trk[j].get_points()
        assert_member((j, "solo"), counts[j], rec, solo(m)[0])
        assert rec.tobytes() == want_r[cuts[j]:cuts[j + 1]].tobytes(), j
    assert counts.sum() == sum(0 <= h < tb.N_HOSTS for h in fin["host"][:13])          # a record whose host is no frame is not traced and not counted
    close_all(grp, trk)


def raw_group_on(grp, ms, active, counts):
    """ldso_trace_group_on through the C entry with the caller's count array"""
    n = len(ms)
    keep = [[np.ascontiguousarray(a, np.float32) for a in m["poses"]] for m in ms]
    ptrs = [(C.c_void_p * n)(*[k[q].ctypes.data for k in keep]) for q in range(3)]
    nh = np.array([len(k[0]) for k in keep], np.int32)
    act = None if active is None else np.ascontiguousarray(active, np.uint8)
    return grp.L.ldso_trace_group_on(grp.h, binding._p(act), binding._p(nh), ptrs[0], ptrs[1], ptrs[2], binding._p(counts))


def test_active_mask_and_solo_calls_between_group_calls():
    st = stream()
    ms = mixed_members()
    trk = [make_tracer(m, st) for m in ms]
    grp = binding.TracerGroup(trk)
    active = np.array([1, 0, 1, 0, 1, 1], np.uint8)          # inf99 and gradnan sit out
    counts = np.full((len(ms), 6), -5, np.int32)
    assert raw_group_on(grp, ms, active, counts) == LDSO_OK
    for i, m in enumerate(ms):
        rec = trk[i].get_points()
        if active[i]:
            assert_member((m["name"], "active"), counts[i], rec, solo(m)[0])
        else:
            assert (counts[i] == -5).all(), m["name"]
            assert rec.tobytes() == m["pts"].tobytes(), m["name"]
    # a member on its own between two group calls
    c = trk[1].trace_on(*ms[1]["poses"])
    assert_member("inf99 solo between", np.asarray(c), trk[1].get_points(), tb.oracle("inf99")[0])
    # ... and the group goes on from there: inf99 gets its second trace, gradnan its first
    counts = np.full((len(ms), 6), -5, np.int32)
    assert raw_group_on(grp, ms, np.array([0, 1, 0, 1, 0, 0], np.uint8), counts) == LDSO_OK
    assert_member("inf99 second", counts[1], trk[1].get_points(), tb.oracle("inf99")[1])
    assert_member("gradnan first", counts[3], trk[3].get_points(), tb.oracle("gradnan")[0])
    assert (counts[[0, 2, 4, 5]] == -5).all()
    close_all(grp, trk)


def test_frames_built_by_the_pyramid_group():
    """the frames handed in through PyramidGroup.make_images + set_frame_pyramid: the bytes of set_frame_raw on a tracer alone"""
    st = stream()
    ms = [small(), scene_member("inf99"), scene_member("single")]
    trk = [make_tracer(m, st, frame=False) for m in ms]
    pyr = [binding.Pyramid(m["w"], m["h"], lv) for m, lv in zip(ms, (3, 1, 2))]
    pg = binding.PyramidGroup(pyr)
    pg.make_images([m["color"] for m in ms], stream=st)
    for g, p in zip(trk, pyr):
        g.set_frame_pyramid(p)
    grp = binding.TracerGroup(trk)
    counts = grp.trace_on([m["poses"] for m in ms])
    for i, m in enumerate(ms):
        g = binding.Tracer(m["w"], m["h"], len(m["pts"]), settings=m["settings"])
        g.set_points(m["pts"]); g.set_frame_raw(m["color"])
        c = g.trace_on(*m["poses"])
        assert_member((m["name"], "raw"), counts[i], trk[i].get_points(), (np.asarray(c), g.get_points()))
        g.close()
    assert_member("inf99 oracle", counts[1], trk[1].get_points(), tb.oracle("inf99")[0])
    close_all(grp, trk)
    pg.close()
    for p in pyr:
        p.close()


def test_refusals_launch_nothing():
    st = stream()
    ms = [small(), scene_member("single"), scene_member("step05")]
    trk = [make_tracer(m, st) for m in ms]
    poses = [m["poses"] for m in ms]
    L = binding.lib()

    def untouched():
        for g, m in zip(trk, ms):
            assert g.get_points().tobytes() == m["pts"].tobytes(), m["name"]

    def refused(call, *words):
        with pytest.raises(binding.LdsoError) as e:
            call()
        assert e.value.code == LDSO_E_INVALID
        for w in words:
            assert w in str(e.value), (w, str(e.value))
        untouched()

    # members on different streams cannot form a group
    loner = make_tracer(ms[1], None)
    refused(lambda: binding.TracerGroup([trk[0], loner]), "ldso_trace_group_create", "stream")
    grp = binding.TracerGroup(trk)
    # a tracer in a second group
    refused(lambda: binding.TracerGroup([trk[1]]), "ldso_trace_group_create", "at most one group")
    # n_hosts of 0
    none = (np.zeros((0, 9), np.float32), np.zeros((0, 3), np.float32), np.zeros((0, 2), np.float32))
    refused(lambda: grp.trace_on([poses[0], none, poses[2]]), "ldso_trace_group_on", "member 1", "n_hosts")
    # ldso_trace_destroy of a member while the group lives
    assert L.ldso_trace_destroy(trk[2].h) == LDSO_E_INVALID and "ldso_trace_destroy" in L.ldso_last_error().decode()
    untouched()
    # a frame not set again after set_stream: the tracer holds none
    trk[2].set_stream(st)
    refused(lambda: grp.trace_on(poses), "ldso_trace_group_on", "member 2", "frame")
    refused(lambda: trk[2].trace_on(*poses[2]), "ldso_trace_on")
    trk[2].set_frame(ms[2]["frame"])
    # a member moved to another stream after the group was made
    trk[1].set_stream(None); trk[1].set_frame(ms[1]["frame"])
    refused(lambda: grp.trace_on(poses), "ldso_trace_group_on", "stream")
    trk[1].set_stream(st)
    # a member without a frame (not set again after the move back)
    refused(lambda: grp.trace_on(poses), "ldso_trace_group_on", "member 1", "frame")
    trk[1].set_frame(ms[1]["frame"])
    # and with everything in place the same group works
    counts = grp.trace_on(poses)
    for i, m in enumerate(ms):
        assert_member((m["name"], "after refusals"), counts[i], trk[i].get_points(), solo(m)[0])
    grp.close()
    assert L.ldso_trace_destroy(trk[2].h) == LDSO_OK          # free once the group is gone
    trk[2].h = None
    for g in trk[:2] + [loner]:
        g.close()
