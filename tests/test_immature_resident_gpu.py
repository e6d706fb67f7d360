"""The immature set resident on the device from detection through activation: the tracer owns the records and their my_type (ldso_amd/csrc/trace.hip:
ldso_trace_set_point_types / ldso_trace_compact), the selection reads candidates from the tracer and seeds from the resident window
(ldso_ba_select_activate_tracer, ldso_amd/csrc/act_select.hip).  Every comparison is device path against device path (or a numpy restatement of a pure data
movement) on identical inputs: equality means bytes or np.array_equal."""
import numpy as np
import pytest

from ldso_amd import binding, synth
from oracle import pyref as pr

pytestmark = pytest.mark.gpu
needs_ref = pytest.mark.skipif(not (pr.available() and pr.adapter_available()), reason="oracle/_ref/libldso_ref.so / adapter/_build/libldso_adapter_test.so not built")

KEEP, DROP, SELECTED = synth.ACT_KEEP, synth.ACT_DROP, synth.ACT_SELECTED
COMPACT_SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 1025, 4097)      # around the wavefront (64) and the workgroup (256) of the compaction, several workgroups
_BASE = {}


def _base():
    """the window "small" with one extra frame, 60 fresh immature points per key frame, traced once (oracle) so that the records differ in every field"""
    if not _BASE:
        from oracle import pyoracle as po
        win = synth.make_config("small", extra_frames=1)
        pts, _ = synth.make_immature_points(win, 60)
        KRKi, Kt, aff = synth.trace_poses(win, win.F)
        po.trace_on(pts, win.images[win.F][0], KRKi, Kt, aff)
        _BASE.update(win=win, pts=pts, poses=(KRKi, Kt, aff))
    return _BASE["win"], _BASE["pts"], _BASE["poses"]


def _records(n):
    """n records: the base set truncated or tiled, hosts still mixed, every record recognisable by its index"""
    win, pts, _ = _base()
    perm = np.random.default_rng(1).permutation(len(pts))           # hosts mixed along the array, so that a host map removes records everywhere
    out = np.resize(pts[perm], n).copy()
    out["lastTracePixelInterval"] = np.arange(n, dtype=np.float32)
    types = (1.0 + 0.25 * np.arange(n)).astype(np.float32)
    return out, types


def _expected(pts, types, keep, hmap, n_hosts):
    """ldso_trace_compact restated: pts[keep & (map[host] >= 0)] with remapped hosts, stable"""
    k = np.ones(len(pts), bool) if keep is None else np.asarray(keep) != 0
    host = pts["host"]
    ok = (host >= 0) & (host < n_hosts)
    m = np.arange(n_hosts, dtype=np.int32) if hmap is None else np.asarray(hmap, np.int32)
    stay = k & ok
    stay[ok] &= m[host[ok]] >= 0
    out = pts[stay].copy()
    out["host"] = m[out["host"]]
    return out, types[stay].copy()


def _masks(n, F, rng):
    first = np.zeros(n, np.uint8); first[:1] = 1
    last = np.zeros(n, np.uint8); last[n - 1:] = 1
    alt = (np.arange(n) % 2 == 0).astype(np.uint8)
    rnd = (rng.random(n) < 0.5).astype(np.uint8)
    mid = F // 2
    hmap = np.array([f if f < mid else (-1 if f == mid else f - 1) for f in range(F)], np.int32)      # the middle host leaves, the ones behind it shift
    return [("all", None, None), ("all-ones", np.ones(n, np.uint8), None), ("none", np.zeros(n, np.uint8), None), ("first", first, None), ("last", last, None),
            ("alternating", alt, None), ("random", rnd, None), ("host-map", None, hmap), ("mask+map", rnd, hmap)]


@pytest.mark.parametrize("n", COMPACT_SIZES)
def test_compaction_equals_numpy_restatement(n):
    win, _, (KRKi, Kt, aff) = _base()
    F = win.F
    pts, types = _records(n)
    rng = np.random.default_rng(100 + n)
    tr = binding.Tracer(win.w, win.h, max(n, 1))
    for name, keep, hmap in _masks(n, F, rng):
        tr.set_points(pts)
        assert np.array_equal(tr.get_point_types(), np.ones(n, np.float32)), "set_points resets my_type to 1"
        tr.set_point_types(types)
        want, want_t = _expected(pts, types, keep, hmap, F)
        left = tr.compact(keep, hmap, n_hosts=F)
        assert left == len(want) == tr.n, (name, left, len(want))
        got = tr.get_points()
        assert got.tobytes() == want.tobytes(), (name, n)
        assert np.array_equal(tr.get_point_types(), want_t), (name, n)
        # a second compaction on the result: the two buffers really swapped
        keep2 = (np.arange(len(want)) % 3 != 1).astype(np.uint8)
        want2, want2_t = _expected(want, want_t, keep2, None, F)
        assert tr.compact(keep2, None, n_hosts=F) == len(want2)
        assert tr.get_points().tobytes() == want2.tobytes(), (name, n, "second")
        assert np.array_equal(tr.get_point_types(), want2_t), (name, n, "second")
    # trace_on after a compaction = set_points of the expected array + trace_on (the poses follow the host map)
    name, keep, hmap = _masks(n, F, rng)[-1]
    want, want_t = _expected(pts, types, keep, hmap, F)
    inv = [int(np.nonzero(hmap == f)[0][0]) for f in range(F - 1)]
    poses = (KRKi[inv], Kt[inv], aff[inv])
    tr.set_points(pts); tr.set_point_types(types); tr.compact(keep, hmap, n_hosts=F)
    tr.set_frame(win.images[F][0])
    ca = tr.trace_on(*poses)
    ref = binding.Tracer(win.w, win.h, max(n, 1))
    ref.set_points(want); ref.set_point_types(want_t); ref.set_frame(win.images[F][0])
    cb = ref.trace_on(*poses)
    assert np.array_equal(ca, cb) and tr.get_points().tobytes() == ref.get_points().tobytes()
    assert np.array_equal(tr.get_point_types(), want_t)
    if n >= 255:
        assert ca[:5].sum() > 0 and len(np.unique(ref.get_points()["lastTraceStatus"])) > 1, "the trace did something"
    tr.close(); ref.close()


def test_compaction_drops_records_with_a_host_outside_the_window():
    """a host outside [0, n_hosts) is dropped, not dereferenced - with and without a host map"""
    win, _, _ = _base()
    F = win.F
    pts, types = _records(300)
    pts["host"][::7] = -1; pts["host"][3::11] = F; pts["host"][5::13] = 1 << 20; pts["host"][6::17] = -(1 << 30)
    hmap = np.arange(F, dtype=np.int32)[::-1].copy()                 # a permutation: every host in range stays
    tr = binding.Tracer(win.w, win.h, 300)
    for hm in (None, hmap):
        tr.set_points(pts); tr.set_point_types(types)
        want, want_t = _expected(pts, types, None, hm, F)
        assert 100 < len(want) < 300
        assert tr.compact(None, hm, n_hosts=F) == len(want)
        assert tr.get_points().tobytes() == want.tobytes() and np.array_equal(tr.get_point_types(), want_t)
    tr.close()


def test_append_points_device_sets_type_one():
    """ldso_trace_append_points_device: the appended records get my_type 1 (FullSystem.cc:1281), the resident ones keep theirs"""
    win, _, _ = _base()
    pts, types = _records(100)
    pyr = binding.Pyramid(win.w, win.h, 1)
    pyr.make_images(np.ascontiguousarray(win.images[0][0][:, :, 0]))
    feat = binding.Features(win.w, win.h, 4096)
    n_new = feat.detect(pyr, 200, host_index=2)[0]
    fresh = feat.get()[1]
    assert n_new > 20 and len(fresh) == n_new
    tr = binding.Tracer(win.w, win.h, 100 + n_new)
    tr.set_points(pts); tr.set_point_types(types)
    tr.append_points_device(n_new, feat.device_ptrs()[1])
    assert tr.n == 100 + n_new
    assert np.array_equal(tr.get_point_types(), np.concatenate([types, np.ones(n_new, np.float32)]))
    assert tr.get_points().tobytes() == np.concatenate([pts, fresh]).tobytes()
    tr.close(); feat.close(); pyr.close()


# ---- selection from the tracer ---------------------------------------------------------------------------------------------------------------------------
_SEL = {}
N_EXTRA = 50


def _sel_state():
    import activation_select_common as asc
    if not _SEL:
        win, (r,), _ = asc.make_state("small", per_frame=1000, P=150)
        g = asc.gather(r)
        F = win.F
        # 50 records hosted by the newest frame, made to look like candidates the rules would select or delete
        extra, _ = synth.make_immature_points(win, N_EXTRA, seed=11, frames=[F - 1])
        extra["idepth_min"] = 0.5; extra["idepth_max"] = 1.5; extra["lastTraceStatus"] = 0; extra["lastTracePixelInterval"] = 1.0
        extra["lastTraceStatus"][::5] = 2; extra["idepth_max"][1::5] = np.nan
        _SEL.update(win=win, r=r, g=g, extra=extra)
    return _SEL["win"], _SEL["g"], _SEL["extra"]


def _loaded_tracer(win, g, extra):
    tr = binding.Tracer(win.w, win.h, len(g["cand"]) + len(extra))
    allp = np.concatenate([g["cand"], extra]); allt = np.concatenate([g["my_type"], np.full(len(extra), 2.0, np.float32)])
    tr.set_points(allp); tr.set_point_types(allt)
    return tr, allp, allt


@needs_ref
def test_window_points_are_the_gathered_seeds():
    """what the seed loop reads from the resident window (every point with host != F - 1: u, v, idepth) is what gatherSelection reads from the object graph"""
    win, g, _ = _sel_state()
    p = win.points[win.points["host"] != win.F - 1]
    a = np.stack([p["u"], p["v"], p["idepth"], p["host"].astype(np.float32)], 1)
    s = g["seeds"]
    b = np.stack([s["u"], s["v"], s["idepth_scaled"], s["host"].astype(np.float32)], 1)
    assert len(a) == len(b) > 20
    assert np.array_equal(a[np.lexsort(a.T)], b[np.lexsort(b.T)])


@needs_ref
@pytest.mark.parametrize("min_dist", (1.0, 4.0))
def test_selection_from_the_tracer_equals_explicit_arrays(min_dist):
    win, g, extra = _sel_state()
    n = len(g["cand"])
    ba2 = binding.BA.from_window(win)
    dec2, sel2, out2 = ba2.select_activate_points(g["seeds"], g["cand"], g["my_type"], g["KRKi"], g["Kt"], g["flagged"], min_dist)
    map2 = ba2.get_distance_map()
    ba2.close()
    # the guard of tests/test_activate_select_gpu.py: a real selection, decisions of all three kinds
    assert len(sel2) > 100 and (dec2 == KEEP).sum() > 10 and (dec2 == DROP).sum() > 10 and (dec2 == SELECTED).sum() == len(sel2)
    tr, allp, allt = _loaded_tracer(win, g, extra)
    ba = binding.BA.from_window(win)
    for compact in (False, True):
        dec, sel, out = ba.select_activate_tracer(tr, g["KRKi"], g["Kt"], g["flagged"], min_dist, compact=compact)
        assert len(dec) == n + N_EXTRA
        assert np.array_equal(dec[:n], dec2), int((dec[:n] != dec2).sum())
        assert (dec[n:] == KEEP).all(), "a record hosted by the newest frame is no candidate"
        assert np.array_equal(sel, sel2)
        assert out.tobytes() == out2.tobytes()
        assert np.array_equal(ba.get_distance_map(), map2)
        if not compact:
            assert tr.n == n + N_EXTRA and tr.get_points().tobytes() == allp.tobytes() and np.array_equal(tr.get_point_types(), allt)
    stay = np.concatenate([dec2 == KEEP, np.ones(N_EXTRA, bool)])
    assert tr.n == stay.sum()
    assert tr.get_points().tobytes() == allp[stay].tobytes()
    assert np.array_equal(tr.get_point_types(), allt[stay])
    ba.close(); tr.close()


@needs_ref
def test_seeds_follow_the_device_state():
    """after optimize() the inverse depths of the resident window have moved: the tracer call seeds the map from them"""
    win, g, extra = _sel_state()
    ba = binding.BA.from_window(win)
    ba.optimize(3, force_all=True)
    idepth = ba.get_points()["idepth"]
    old = win.points["host"] != win.F - 1
    assert (idepth[old] != win.points["idepth"][old]).mean() > 0.5, "the inverse depths moved"
    seeds = np.zeros(int(old.sum()), synth.ACT_SEED_DTYPE)
    seeds["u"] = win.points["u"][old]; seeds["v"] = win.points["v"][old]; seeds["idepth_scaled"] = idepth[old]; seeds["host"] = win.points["host"][old]
    dec2, sel2, out2 = ba.select_activate_points(seeds, g["cand"], g["my_type"], g["KRKi"], g["Kt"], g["flagged"], 1.0)
    map2 = ba.get_distance_map()
    tr, _, _ = _loaded_tracer(win, g, extra)
    dec, sel, out = ba.select_activate_tracer(tr, g["KRKi"], g["Kt"], g["flagged"], 1.0, compact=False)
    n = len(g["cand"])
    assert len(sel2) > 100
    assert np.array_equal(dec[:n], dec2) and np.array_equal(sel, sel2) and out.tobytes() == out2.tobytes()
    assert np.array_equal(ba.get_distance_map(), map2)
    ba.close(); tr.close()


@needs_ref
def test_precondition_errors_leave_the_tracer_alone():
    win, g, extra = _sel_state()
    tr, allp, allt = _loaded_tracer(win, g, extra)
    ba = binding.BA.from_window(win)
    with pytest.raises(binding.LdsoError) as e:
        ba.select_activate_tracer(tr, g["KRKi"][:-1], g["Kt"][:-1], g["flagged"][:-1], 1.0)       # n_hosts != F
    assert e.value.code == binding.E_INVALID
    with pytest.raises(binding.LdsoError):
        ba.get_distance_map()                                                                     # no selection ever ran on this handle: nothing was launched
    assert tr.n == len(allp) and tr.get_points().tobytes() == allp.tobytes()
    ba.set_shard(0, win.P // 2)
    with pytest.raises(binding.LdsoError) as e:
        ba.select_activate_tracer(tr, g["KRKi"], g["Kt"], g["flagged"], 1.0)                      # a sharded handle
    assert e.value.code == binding.E_INVALID
    with pytest.raises(binding.LdsoError):
        ba.get_distance_map()                                                                     # no selection ever ran on this handle: nothing was launched
    assert tr.n == len(allp) and tr.get_points().tobytes() == allp.tobytes() and np.array_equal(tr.get_point_types(), allt)
    ba.close(); tr.close()
