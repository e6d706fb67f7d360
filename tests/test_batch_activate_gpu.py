"""ldso_ba_batch_activate_points / ldso_ba_batch_select_candidates / ldso_ba_batch_select_activate_points: FullSystem::activatePointsMT (FullSystem.cc:1052-1189) for
a whole batch of windows.  The standard throughout is equality with the single-window entry run on the SAME handle (the member of the batch: the same device
state): activation records, decisions and selected lists byte for byte, distance maps with np.array_equal - the batched kernels call the device functions of the
single-window kernels on the same bytes, so no tolerance applies.  The windows are mixed_windows() of test_batch_optimize_gpu.py (F = 2..7, 320 x 240 and
256 x 192, one prior); the candidates are traced on the CPU against the window's own last two key frames (batch_activate_common.py: numpy only, nothing here
needs the reference libraries); all handles sit on one torch stream."""
import ctypes as C
import functools

import numpy as np
import pytest

from ldso_amd import synth, binding
import batch_activate_common as bac
from test_batch_optimize_gpu import mixed_windows, stream, make_batch

pytestmark = pytest.mark.gpu

# candidates per key frame, per window of mixed_windows(): dense enough that currentMinActDist = 0.5 rejects more than a tenth of those that reach the distance
# test (window 1), sparse enough that 4.0 selects more than a tenth (window 4); the shares observed on an MI355X are printed by check_mix
PER_FRAME = (300, 1000, 300, 300, 200, 600, 600)
BIG_PER_FRAME, BIG_MIN_DIST = 1500, 4.0                     # the 1280 x 512 window: enough candidates on 640 x 256 cells that the distance test rejects a share of them
MIN_DISTS = (0.0, 0.5, 1.0, 2.0, 4.0, 1.0, 1.0)          # per window of mixed_windows()
NO_CANDIDATES, NO_JOB, NO_SEEDS = 0, 5, 6                   # window 0 builds its map only (n = 0), window 5 takes no part, window 6 has no seed


@functools.lru_cache(maxsize=None)
def base_jobs():
    """one job per window of mixed_windows(), computed once and never written to"""
    return tuple(bac.make_job(w, PER_FRAME[i], seed=40 + i) for i, w in enumerate(mixed_windows()))


def mixed_jobs():
    jobs = [bac.with_distance(j, d) for j, d in zip(base_jobs(), MIN_DISTS)]
    j = jobs[NO_CANDIDATES]
    jobs[NO_CANDIDATES] = dict(j, cand=j["cand"][:0], my_type=j["my_type"][:0])
    jobs[NO_SEEDS] = dict(jobs[NO_SEEDS], seeds=jobs[NO_SEEDS]["seeds"][:0])
    jobs[NO_JOB] = None
    return jobs


def solo_select(member, job):
    dec, sel = member.select_candidates(*bac.solo_args(job), job["min_act_dist"])
    return dec, sel, member.get_distance_map()


def solo_fused(member, job):
    dec, sel, rec = member.select_activate_points(*bac.solo_args(job), job["min_act_dist"])
    return dec, sel, rec, member.get_distance_map()


def map_before(member, job):
    """the map of makeDistanceMap alone: a selection without candidates"""
    member.select_candidates(job["seeds"], job["cand"][:0], job["my_type"][:0], job["KRKi"], job["Kt"], job["flagged"], 1.0)
    return member.get_distance_map()


def assert_window_equal(i, got, got_map, want, want_map):
    assert len(got) == len(want), i
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (i, k, a.shape, b.shape)
    assert np.array_equal(got_map, want_map), (i, int((got_map != want_map).sum()))


def check_mix(batch, jobs, out, fused):
    """every participating window of `out` against the single-window entry on its member; the input conditions on the single-window leg -> records per window"""
    od, recs = 0, {}
    for i, (g, job) in enumerate(zip(batch, jobs)):
        if job is None:
            assert out[i] is None
            continue
        got_map = g.get_distance_map()
        want = solo_fused(g, job) if fused else solo_select(g, job)
        assert_window_equal(i, out[i], got_map, want[:-1], want[-1])
        dec, sel = want[0], want[1]
        if fused:
            # the identity test_fused_selection_and_activation asserts for the single-window entry
            assert out[i][2].tobytes() == g.activate_points(job["cand"][sel]).tobytes() if len(sel) else len(out[i][2]) == 0, i
            recs[i] = out[i][2]
        if len(job["cand"]) == 0:
            assert len(dec) == 0 and len(sel) == 0 and (got_map == 0).sum() > 20, i          # the map alone, and it holds the seeds
            continue
        if job["min_act_dist"] > 0:
            fig = bac.input_conditions(job, job["min_act_dist"], dec, sel, want[2] if fused else None, got_map.shape)
            before = map_before(g, job)
            fig["order_dependent"] = bac.order_dependent(job, dec, before, job["min_act_dist"])
            od += fig["order_dependent"]
            print("window", i, "min_act_dist", job["min_act_dist"], fig)
        if len(job["seeds"]) == 0:
            assert (got_map == 0).sum() == len(sel), i          # nothing on the map but the accepted candidates
    assert od >= 1, "a candidate that passes against the initial map is rejected at its turn: the order matters somewhere in this batch"
    return recs


def test_plain_activation_ragged():
    """1, 3, none, 5, 257, 64 and 130 candidates: workgroups of four wavefronts straddle the window boundaries, one window takes no part"""
    st = stream()
    wins = mixed_windows()
    batch, b = make_batch(wins, st)
    counts = [1, 3, None, 5, 257, 64, 130]
    pts = []
    for job, n in zip(base_jobs(), counts):
        c = job["cand"]
        pts.append(None if n is None else np.ascontiguousarray(c[:: len(c) // n][:n]))
    out = b.activate_points(pts)
    oks = []
    for i, g in enumerate(batch):
        if counts[i] is None:
            assert out[i] is None
            continue
        assert len(pts[i]) == counts[i] and len(out[i]) == counts[i]
        want = g.activate_points(pts[i])
        assert out[i].tobytes() == want.tobytes(), (i, int((out[i]["ok"] != want["ok"]).sum()))
        oks.append(want["ok"])
    ok = np.concatenate(oks)
    assert 0.0 < ok.mean() < 1.0, ok.mean()
    # an empty array is no part either, and a batch without any part is no call
    assert b.activate_points([None] * 3 + [pts[3][:0]] + [None] * 3) == [None] * 7
    b.close()


def test_selection_at_mixed_settings():
    """currentMinActDist 0 .. 4 side by side, a window without candidates (the map only), one without seeds, one without a job - which keeps the map an earlier
    single-window selection left on it"""
    st = stream()
    batch, b = make_batch(mixed_windows(), st)
    jobs = mixed_jobs()
    earlier = solo_select(batch[NO_JOB], bac.with_distance(base_jobs()[NO_JOB], 2.0))[2]
    assert (earlier == 0).sum() > 20
    out = b.select_candidates(jobs)
    assert np.array_equal(batch[NO_JOB].get_distance_map(), earlier)
    check_mix(batch, jobs, out, fused=False)
    b.close()


def test_fused_selection_and_activation_before_and_after_an_optimize():
    st = stream()
    batch, b = make_batch(mixed_windows(), st)
    jobs = mixed_jobs()
    first = check_mix(batch, jobs, b.select_activate_points(jobs), fused=True)
    _, its, status = b.optimize(6)
    assert np.all(status == 0) and len(set((its & 1).tolist())) == 2, its          # the windows sit at both ping-pong parities
    second = check_mix(batch, jobs, b.select_activate_points(jobs), fused=True)
    changed = [i for i in first if len(first[i]) and first[i].tobytes() != second[i].tobytes()]
    print("windows whose records moved with the poses:", changed)
    assert changed, "the call reads the current poses: an optimize() in between changes at least one window's records"
    b.close()


def test_both_map_placements_in_one_batch():
    """1280 x 512: the 640 x 256 map (163 840 B) does not fit into LDS beside the frontier lists and stays in global memory; 320 x 240 beside it in LDS.
    ldso_ba_batch_create accepts the pair (same stream, settings and slot-table width)."""
    st = stream()
    wins = (synth.make_config("tiny", w=1280, h=512, fx=500.0), mixed_windows()[0])
    batch, b = make_batch(list(wins), st)
    jobs = [bac.with_distance(bac.make_job(wins[0], BIG_PER_FRAME, seed=50), BIG_MIN_DIST), bac.with_distance(base_jobs()[0], 1.0)]
    out = b.select_activate_points(jobs)
    assert batch[0].get_distance_map().shape == (256, 640) and batch[1].get_distance_map().shape == (120, 160)
    check_mix(batch, jobs, out, fused=True)
    out = b.select_candidates(jobs)
    check_mix(batch, jobs, out, fused=False)
    b.close()


def test_twice_on_the_same_batch_with_growing_counts():
    """the second call brings more candidates than the first: the staging arena grows between them; the batched marginalisation that shares the arena still
    equals its twin afterwards"""
    from test_batch_marginalize_gpu import applied_batch, twin, every7, same_prior
    st = stream()
    wins = mixed_windows()[:3]
    batch, b = applied_batch(wins, st)
    full = [bac.with_distance(j, d) for j, d in zip(base_jobs()[:3], (1.0, 2.0, 1.0))]
    small = [dict(j, cand=j["cand"][::2].copy(), my_type=j["my_type"][::2].copy()) for j in full]
    assert all(len(f["cand"]) == 2 * len(s["cand"]) for s, f in zip(small, full))
    for jobs in (small, full):
        out = b.select_activate_points(jobs)
        for i, (g, job) in enumerate(zip(batch, jobs)):
            got_map = g.get_distance_map()
            want = solo_fused(g, job)
            assert_window_equal(i, out[i], got_map, want[:-1], want[-1])
            print("window", i, bac.input_conditions(job, job["min_act_dist"], want[0], want[1], want[2], got_map.shape))
        plain = b.activate_points([j["cand"] for j in jobs])
        for i, (g, job) in enumerate(zip(batch, jobs)):
            assert plain[i].tobytes() == g.activate_points(job["cand"]).tobytes(), i
    flags = [every7(w) for w in wins]
    marg = b.marginalize_points(flags)
    for i, w in enumerate(wins):
        g = twin(w, b, batch[i], st)
        same_prior("batch_activate_then_marg_points_w%d" % i, marg[i], g.marginalize_points(flags[i]))
        g.close()
    b.close()


def test_counts_at_which_a_regions_rounding_changes():
    """1, 3, 4 and 5 candidates (4 n bytes cross a 16-byte boundary between 4 and 5) with no seed and with one, on two 320 x 240 `tiny` windows: each count once as
    the first window of the batched fused call, whose size moves the second window's regions, and once as the second.  The batch against the single-window entry on
    its member, and the single-window entry against ldso_ba_activate_points on the candidates it selected.  The candidates are ones that reach the distance test, so
    every call selects."""
    import activation_select_common as asc
    st = stream()
    wins = [synth.make_config("tiny", w=320, h=240, fx=200.0, seed=71 + i) for i in range(2)]
    batch, b = make_batch(wins, st)
    pool = []
    for i, w in enumerate(wins):
        j = bac.with_distance(bac.make_job(w, 40, seed=75 + i), 1.0)
        el = np.nonzero(asc.eligible_in_bounds(j, (120, 160)))[0]
        assert len(el) >= 5
        pool.append(dict(j, cand=np.ascontiguousarray(j["cand"][el]), my_type=np.ascontiguousarray(j["my_type"][el])))
    for n_seeds in (0, 1):
        for counts in ((1, 3), (3, 4), (4, 5), (5, 1)):
            jobs = [dict(j, cand=j["cand"][:n].copy(), my_type=j["my_type"][:n].copy(), seeds=j["seeds"][:n_seeds].copy()) for j, n in zip(pool, counts)]
            out = b.select_activate_points(jobs)
            for i, (g, job) in enumerate(zip(batch, jobs)):
                got_map = g.get_distance_map()
                want = solo_fused(g, job)
                assert_window_equal((n_seeds, counts, i), out[i], got_map, want[:-1], want[-1])
                dec, sel, rec = want[:3]
                assert len(dec) == counts[i] and 1 <= len(sel) <= counts[i] and len(rec) == len(sel), (n_seeds, counts, i)
                assert rec.tobytes() == g.activate_points(job["cand"][sel]).tobytes(), (n_seeds, counts, i)
                assert (got_map == 0).sum() >= len(sel)
    b.close()


SENTINEL = -7


def test_refusals():
    """each case raises LdsoError (LDSO_E_INVALID) through the binding; through the C entry the outputs handed in keep their sentinel; the members' maps stay"""
    st = stream()
    wins = mixed_windows()[:3]
    batch, b = make_batch(wins, st)
    good = [bac.with_distance(j, 1.0) for j in base_jobs()[:3]]
    maps = [solo_select(g, j)[2] for g, j in zip(batch, good)]
    F1 = wins[1].F
    outside = good[1]["cand"].copy(); outside["host"][5] = F1
    cases = {
        "n_hosts != F": ([good[0], dict(good[1], KRKi=good[1]["KRKi"][:F1 - 1], Kt=good[1]["Kt"][:F1 - 1], flagged=good[1]["flagged"][:F1 - 1]), good[2]], ("select_activate_points",)),
        "host outside": ([good[0], dict(good[1], cand=outside), good[2]], ("select_candidates", "select_activate_points")),
        "no KRKi": ([good[0], good[1], dict(good[2], KRKi=None)], ("select_candidates", "select_activate_points")),
    }
    for name, (jobs, methods) in cases.items():
        for method in methods:
            fused = method == "select_activate_points"
            with pytest.raises(binding.LdsoError) as e:
                getattr(b, method)(jobs)
            assert e.value.code == binding.E_INVALID and "ldso_ba_batch_" + method in str(e.value), (name, str(e.value))
            J, keep = b._jobs(jobs, fused)
            for k in keep:
                k[6].fill(SENTINEL); k[7].fill(SENTINEL)
                if fused:
                    k[8].view(np.int32).fill(SENTINEL)
            for j in J:
                j.n_selected = SENTINEL
            args = (C.c_float(3.0), C.c_int(1), C.c_float(100.0), C.c_int(3)) if fused else (C.c_float(3.0),)
            assert getattr(b.L, "ldso_ba_batch_" + method)(b.h, J, *args) == binding.E_INVALID, name
            for j, k in zip(J, keep):
                assert j.n_selected == SENTINEL and np.all(k[6] == SENTINEL) and np.all(k[7] == SENTINEL) and (not fused or np.all(k[8].view(np.int32) == SENTINEL)), name
            for g, m in zip(batch, maps):
                assert np.array_equal(g.get_distance_map(), m), name
    # the plain entry: a window that takes part without its output array
    pts = [np.ascontiguousarray(j["cand"][:8]) for j in good]
    rec = [np.full(8, SENTINEL, np.int32).repeat(synth.ACTIVATION_DTYPE.itemsize // 4) for _ in pts]
    cnt = np.array([8, 8, 8], np.int32)
    PP = (C.c_void_p * 3)(*[p.ctypes.data for p in pts]); PO = (C.c_void_p * 3)(rec[0].ctypes.data, None, rec[2].ctypes.data)
    assert b.L.ldso_ba_batch_activate_points(b.h, binding._p(cnt), PP, C.c_int(1), C.c_float(100.0), C.c_int(3), PO) == binding.E_INVALID
    assert "ldso_ba_batch_activate_points" in b.L.ldso_last_error().decode() and all(np.all(r == SENTINEL) for r in rec)
    # a None batch
    b.close()
    for call in (lambda: b.select_candidates(good), lambda: b.select_activate_points(good), lambda: b.activate_points(pts)):
        with pytest.raises(binding.LdsoError) as e:
            call()
        assert e.value.code == binding.E_INVALID and "null batch" in str(e.value)
    for g, m in zip(batch, maps):
        assert np.array_equal(g.get_distance_map(), m)
    # windows of more than 8 key frames: refused like ldso_ba_batch_optimize, with the single-window entry to use instead
    wins9 = [synth.make_window(F=9, P=100, w=256, h=192, fx=160.0, seed=40 + i) for i in range(2)]
    batch9, b9 = make_batch(wins9, st)
    with pytest.raises(binding.LdsoError) as e:
        b9.activate_points([pts[0], None])
    assert e.value.code == binding.E_INVALID and "F <= 8" in str(e.value) and "ldso_ba_activate_points" in str(e.value)
    with pytest.raises(binding.LdsoError) as e:
        b9.select_activate_points([good[0], None])
    assert e.value.code == binding.E_INVALID and "F <= 8" in str(e.value) and "ldso_ba_select_activate_points" in str(e.value)
    b9.close()
