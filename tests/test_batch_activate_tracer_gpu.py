"""ldso_ba_batch_select_activate_tracers: FullSystem::activatePointsMT (FullSystem.cc:1052-1189) for a whole batch of windows with every window's immature set where
it lives - the candidates are a tracer's resident records and types, the seeds the points of the resident window, and what the loop did not KEEP leaves the tracer in
the same enqueue.  The standard is equality with ldso_ba_select_activate_tracer run on the SAME member handle with a twin tracer that holds the same bytes:
decisions, selected lists and activation records byte for byte, distance maps with np.array_equal, the tracers' records, types and counts byte for byte - the
batched kernels call the device functions of the single-window kernels on the same bytes, so no tolerance applies.  Windows and jobs are those of
tests/test_batch_activate_gpu.py (mixed_windows(), batch_activate_common.make_job, PER_FRAME, MIN_DISTS: numpy and the CPU oracle only, no reference library);
every tracer holds the job's candidates and, behind them, 50 records hosted by the newest frame that look selectable but are no candidates (FullSystem.cc:1089)."""
import ctypes as C
import functools

import numpy as np
import pytest

from ldso_amd import synth, binding
import batch_activate_common as bac
from test_batch_optimize_gpu import mixed_windows, stream, make_batch
from test_batch_activate_gpu import base_jobs, map_before, MIN_DISTS, BIG_PER_FRAME, BIG_MIN_DIST

pytestmark = pytest.mark.gpu

KEEP, DROP, SELECTED = synth.ACT_KEEP, synth.ACT_DROP, synth.ACT_SELECTED
N_EXTRA = 50
EMPTY, NO_TRACER = 0, 5                                                  # window 0: a tracer without records (the map only), window 5 takes no part
COMPACT = (True, True, False, True, False, True, True)                  # per window of mixed_windows()
SENTINEL = -7


def newest_frame_records(win, seed=11):
    """50 records hosted by the newest frame, made to look like candidates the rules would select or delete (tests/test_immature_resident_gpu.py::_sel_state)"""
    extra, _ = synth.make_immature_points(win, N_EXTRA, seed=seed, frames=[win.F - 1])
    extra["idepth_min"] = 0.5; extra["idepth_max"] = 1.5; extra["lastTraceStatus"] = 0; extra["lastTracePixelInterval"] = 1.0
    extra["lastTraceStatus"][::5] = 2; extra["idepth_max"][1::5] = np.nan
    return extra


def resident_set(win, job):
    """what a window's tracer holds: (records, types)"""
    extra = newest_frame_records(win)
    return np.concatenate([job["cand"], extra]), np.concatenate([job["my_type"], np.full(N_EXTRA, 2.0, np.float32)])


@functools.lru_cache(maxsize=None)
def mixed_sets():
    """per window of mixed_windows() its job at MIN_DISTS and its tracer's (records, types); computed once and never written to"""
    jobs = [bac.with_distance(j, d) for j, d in zip(base_jobs(), MIN_DISTS)]
    sets = [resident_set(w, j) for w, j in zip(mixed_windows(), jobs)]
    sets[EMPTY] = (sets[EMPTY][0][:0], sets[EMPTY][1][:0])
    jobs[EMPTY] = dict(jobs[EMPTY], cand=jobs[EMPTY]["cand"][:0], my_type=jobs[EMPTY]["my_type"][:0])
    return tuple(jobs), tuple(sets)


@functools.lru_cache(maxsize=None)
def big_job():
    win = synth.make_config("tiny", w=1280, h=512, fx=500.0)
    return win, bac.with_distance(bac.make_job(win, BIG_PER_FRAME, seed=50), BIG_MIN_DIST)


def load(win, recs, types):
    t = binding.Tracer(win.w, win.h, max(len(recs), 1))
    t.set_points(recs); t.set_point_types(types)
    return t


def pair(win, recs_types):
    """the tracer of the batched call and its twin for the single-window leg"""
    return load(win, *recs_types), load(win, *recs_types)


def state(t):
    return t.n, t.get_points().tobytes(), t.get_point_types().tobytes()


def tracer_job(t, job, compact):
    return dict(tracer=t, KRKi=job["KRKi"], Kt=job["Kt"], flagged=job["flagged"], min_act_dist=job["min_act_dist"], compact=compact)


def run_and_check(batch, b, jobs, pairs, compacts):
    """one batched call on the first tracer of every pair, then the single-window entry with the twin on the member handle; every output compared
    -> {window: (decision, selected, records, map)} of the single-window leg"""
    tj = [None if p is None else tracer_job(p[0], jobs[i], compacts[i]) for i, p in enumerate(pairs)]
    before = [None if p is None else state(p[0]) for p in pairs]
    out = b.select_activate_tracers(tj)
    solo = {}
    for i, (g, p) in enumerate(zip(batch, pairs)):
        if p is None:
            assert out[i] is None
            continue
        job, tw = jobs[i], p[1]
        n = tw.n
        assert n == before[i][0] == len(out[i][0])
        got_map = g.get_distance_map()
        want = g.select_activate_tracer(tw, job["KRKi"], job["Kt"], job["flagged"], job["min_act_dist"], compact=compacts[i])
        want_map = g.get_distance_map()
        for k, (a, c) in enumerate(zip(out[i], want)):
            assert a.dtype == c.dtype and a.shape == c.shape and a.tobytes() == c.tobytes(), (i, k, a.shape, c.shape)
        assert np.array_equal(got_map, want_map), (i, int((got_map != want_map).sum()))
        dec = want[0]
        if n:
            assert (dec[n - N_EXTRA:] == KEEP).all(), "a record hosted by the newest frame is no candidate"
            assert (want[1] < n - N_EXTRA).all()
        if compacts[i]:
            assert p[0].n == int((dec == KEEP).sum()), i
            assert state(p[0]) == state(tw), i
        else:
            assert state(p[0]) == before[i] and state(tw) == before[i], i
        solo[i] = (dec, want[1], want[2], want_map)
    return solo


def guards(batch, jobs, solo):
    """the input conditions, on the single-window leg: a real selection in every window with currentMinActDist > 0 -> the order-dependent candidates of the batch"""
    od = 0
    for i, (dec, sel, rec, got_map) in solo.items():
        job = jobs[i]
        if len(job["cand"]) == 0:
            assert len(dec) == 0 and len(sel) == 0 and (got_map == 0).sum() > 20, i          # the map alone, and it holds the seeds
            continue
        if job["min_act_dist"] > 0:
            nc = len(job["cand"])
            fig = bac.input_conditions(job, job["min_act_dist"], dec[:nc], sel, rec, got_map.shape)
            fig["order_dependent"] = bac.order_dependent(job, dec[:nc], map_before(batch[i], job), job["min_act_dist"])
            od += fig["order_dependent"]
            print("window", i, "min_act_dist", job["min_act_dist"], fig)
    return od


def close_all(b, batch, pairs):
    b.close()
    for g in batch:
        g.close()
    for p in pairs:
        if p is not None:
            for t in p:
                t.close()


def test_batched_equals_solo_before_and_after_an_optimize():
    st = stream()
    wins = mixed_windows()
    batch, b = make_batch(wins, st)
    jobs, sets = mixed_sets()
    assert len(sets[EMPTY][0]) == 0 and len(set(COMPACT)) == 2
    # the window that takes no part keeps the map an earlier single-window selection left on it
    lone = load(wins[NO_TRACER], *sets[NO_TRACER])
    batch[NO_TRACER].select_activate_tracer(lone, jobs[NO_TRACER]["KRKi"], jobs[NO_TRACER]["Kt"], jobs[NO_TRACER]["flagged"], 2.0, compact=False)
    earlier = batch[NO_TRACER].get_distance_map()
    assert (earlier == 0).sum() > 20
    pairs = [None if i == NO_TRACER else pair(w, sets[i]) for i, w in enumerate(wins)]
    first = run_and_check(batch, b, jobs, pairs, COMPACT)
    assert np.array_equal(batch[NO_TRACER].get_distance_map(), earlier)
    assert pairs[EMPTY][0].n == 0
    # before any optimize() the window's own points are the explicit seeds of window_seeds: the conditions of tests/test_batch_activate_gpu.py apply
    od = guards(batch, jobs, first)
    assert od >= 1, "a candidate that passes against the initial map is rejected at its turn: the order matters somewhere in this batch"
    _, its, status = b.optimize(6)
    assert np.all(status == 0) and len(set((its & 1).tolist())) == 2, its          # the windows sit at both ping-pong parities
    fresh = [None if i == NO_TRACER else pair(w, sets[i]) for i, w in enumerate(wins)]
    second = run_and_check(batch, b, jobs, fresh, COMPACT)
    moved = [i for i in first if not np.array_equal(first[i][3], second[i][3])]
    print("windows whose map moved with the inverse depths:", moved)
    assert moved, "the seeds follow the device state: an optimize() in between changes at least one window's map"
    lone.close()
    close_all(b, batch, pairs + fresh)


def test_both_map_placements_in_one_batch():
    """1280 x 512: the 640 x 256 map does not fit into LDS beside the frontier lists and stays in global memory; 320 x 240 beside it in LDS"""
    st = stream()
    big, bj = big_job()
    wins = [big, mixed_windows()[0]]
    jobs = [bj, bac.with_distance(base_jobs()[0], 1.0)]
    batch, b = make_batch(wins, st)
    pairs = [pair(w, resident_set(w, j)) for w, j in zip(wins, jobs)]
    solo = run_and_check(batch, b, jobs, pairs, (True, False))
    assert solo[0][3].shape == (256, 640) and solo[1][3].shape == (120, 160)
    guards(batch, jobs, solo)
    close_all(b, batch, pairs)


def test_twice_on_the_same_batch():
    """the second call sees the compacted tracers: the counts shrink, the arenas of the first call are reused"""
    st = stream()
    wins = mixed_windows()[:3]
    jobs = [bac.with_distance(j, d) for j, d in zip(base_jobs()[:3], (1.0, 2.0, 1.0))]
    batch, b = make_batch(wins, st)
    pairs = [pair(w, resident_set(w, j)) for w, j in zip(wins, jobs)]
    n0 = [p[0].n for p in pairs]
    run_and_check(batch, b, jobs, pairs, (True,) * 3)
    n1 = [p[0].n for p in pairs]
    assert all(N_EXTRA < a < c for a, c in zip(n1, n0)), (n0, n1)
    second = run_and_check(batch, b, jobs, pairs, (True,) * 3)
    n2 = [p[0].n for p in pairs]
    assert all(len(second[i][0]) == n1[i] and N_EXTRA <= n2[i] <= n1[i] for i in range(3)), (n1, n2)
    close_all(b, batch, pairs)


def test_refusals():
    """each case returns LDSO_E_INVALID: the outputs handed in keep their sentinel, the tracers their bytes, and no member has a map (nothing was enqueued)"""
    st = stream()
    wins = mixed_windows()[:3]
    jobs = [bac.with_distance(j, 1.0) for j in base_jobs()[:3]]
    batch, b = make_batch(wins, st)
    trk = [load(w, *resident_set(w, j)) for w, j in zip(wins, jobs)]
    before = [state(t) for t in trk]
    good = [tracer_job(t, j, True) for t, j in zip(trk, jobs)]
    tail = (C.c_float(3.0), C.c_int(1), C.c_float(100.0), C.c_int(3))
    entry = b.L.ldso_ba_batch_select_activate_tracers

    def refused(name, tjobs, *words, mutate=None, args=tail):
        J, keep = b._tracer_jobs(tjobs)
        for j, k in zip(J, keep):
            k[4].fill(SENTINEL); k[5].fill(SENTINEL); k[6].view(np.int32).fill(SENTINEL)
            j.n_selected = SENTINEL; j.n_left = SENTINEL
        if mutate:
            mutate(J)
        assert entry(b.h, J, *args) == binding.E_INVALID, name
        msg = b.L.ldso_last_error().decode()
        assert "ldso_ba_batch_select_activate_tracers" in msg, (name, msg)
        for w in words:
            assert w in msg, (name, w, msg)
        for j, k in zip(J, keep):
            assert j.n_selected == SENTINEL and j.n_left == SENTINEL and np.all(k[4] == SENTINEL) and np.all(k[5] == SENTINEL) and np.all(k[6].view(np.int32) == SENTINEL), name
        assert [state(t) for t in trk] == before, name
        for g in batch:
            with pytest.raises(binding.LdsoError):
                g.get_distance_map()          # no selection ever ran on this handle: nothing was launched

    F1 = wins[1].F
    short = dict(good[1], KRKi=jobs[1]["KRKi"][:F1 - 1], Kt=jobs[1]["Kt"][:F1 - 1], flagged=jobs[1]["flagged"][:F1 - 1])
    refused("n_hosts != F", [good[0], short, good[2]], "per frame")
    refused("no KRKi", [good[0], good[1], dict(good[2], KRKi=None)], "KRKi")
    refused("no Kt", [dict(good[0], Kt=None), good[1], good[2]], "KRKi")
    refused("the same tracer twice", [good[0], good[1], dict(good[2], tracer=trk[0])], "window 2", "same tracer")

    def without(field):
        def m(J):
            setattr(J[1], field, None)
        return m
    for field in ("decision_out", "selected_out", "out"):
        refused("no " + field, good, "outputs", mutate=without(field))
    refused("gn_iterations < 0", good, "bad arguments", args=(C.c_float(3.0), C.c_int(1), C.c_float(100.0), C.c_int(-1)))
    import torch
    if torch.cuda.device_count() >= 2:
        far = binding.Tracer(wins[1].w, wins[1].h, 8, device=1)
        refused("another device", [good[0], dict(good[1], tracer=far), good[2]], "window 1", "different devices")
        far.close()
    # null jobs
    assert entry(b.h, None, *tail) == binding.E_INVALID and "null jobs" in b.L.ldso_last_error().decode()
    # a sharded member
    batch[2].set_shard(0, wins[2].P // 2)
    refused("sharded", good, "sharded")
    # the binding raises the same refusals
    with pytest.raises(binding.LdsoError) as e:
        b.select_activate_tracers(good)
    assert e.value.code == binding.E_INVALID and "sharded" in str(e.value)
    b.close()
    with pytest.raises(binding.LdsoError) as e:
        b.select_activate_tracers(good)
    assert e.value.code == binding.E_INVALID and "null batch" in str(e.value)
    assert [state(t) for t in trk] == before
    # windows of more than 8 key frames: refused like the other batched entries, with the single-window entry to use instead
    wins9 = [synth.make_window(F=9, P=100, w=256, h=192, fx=160.0, seed=40 + i) for i in range(2)]
    batch9, b9 = make_batch(wins9, st)
    with pytest.raises(binding.LdsoError) as e:
        b9.select_activate_tracers([dict(good[0], KRKi=np.zeros((9, 9)), Kt=np.zeros((9, 3)), flagged=np.zeros(9)), None])
    assert e.value.code == binding.E_INVALID and "F <= 8" in str(e.value) and "ldso_ba_select_activate_tracer" in str(e.value)
    assert [state(t) for t in trk] == before
    b9.close()
    for g in batch + batch9:
        g.close()
    for t in trk:
        t.close()
