"""ldso_ba_batch_marginalize_points / ldso_ba_batch_marginalize_frame: the two steps FullSystem::makeKeyFrame runs behind optimize() (marginalizePointsF with the
re-linearise + fix pass of flagPointsForRemoval, FullSystem.cc:527; marginalizeFrame, :574-583) for a whole batch of windows.  Every window that takes part must
end where the single-window entry leaves its twin handle ("solo": split launches, the batch's K-splits, and ALWAYS the batch's chunk cuts - the per-chunk partial
sums are fp32, another cut is another rounding): H_M / b_M of the points within 1e-9 of their maximum (the bound test_batch_optimize_gpu.py asserts for the same
quantity), the frames byte for byte (the same device function on the same bytes, no atomics).  The windows are mixed_windows() of test_batch_optimize_gpu.py
(F = 2..7, P = 120..500: different n = 8F+4 side by side, a window with and without a prior, re-cut chunks); all tests run on one torch stream."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import rel, blockrel, observe
from ldso_amd import synth, binding
from oracle import pyoracle as po
from test_batch_optimize_gpu import mixed_windows, stream, make_batch, make_solo
from test_marg_frame_gpu import _full_rank_prior

pytestmark = pytest.mark.gpu
TOL = 1e-4           # tests/test_ba_gpu.py: the device against the oracle
SAME = 1e-9          # batch against solo


def assert_equal(gs, gb, tag):
    """the bounds of tests/test_batch_optimize_gpu.py::assert_equal"""
    fs, fb = gs.get_frames(), gb.get_frames()
    assert np.abs(fb["frames"]["state"] - fs["frames"]["state"]).max() <= 1e-9 * np.abs(fs["frames"]["state"]).max(), tag
    assert np.array_equal(fb["frames"]["frameEnergyTH"], fs["frames"]["frameEnergyTH"]), tag
    ps, pb = gs.get_points(), gb.get_points()
    assert rel(pb["idepth"], ps["idepth"]) < 1e-6 and rel(pb["HdiF"], ps["HdiF"]) < 1e-5, tag
    rs, rb = gs.get_residuals(), gb.get_residuals()
    for k in ("state_state", "is_active", "to_remove"):
        assert np.array_equal(rs[k], rb[k]), (tag, k)
    assert rel(rb["out"]["state_NewEnergy"], rs["out"]["state_NewEnergy"]) < 1e-5, tag
    es, eb = gs.get_energy_log(), gb.get_energy_log()
    assert len(es) == len(eb) and rel(eb, es) < 1e-5, (tag, es, eb)


def applied(g):
    g.linearize_all()
    g.apply_res()
    return g


def applied_batch(wins, st):
    """members from BA.from_window + linearize_all + apply_res, then the batch (which may re-cut their chunks)"""
    hs = [applied(binding.BA.from_window(w, stream=st)) for w in wins]
    return hs, binding.BABatch(hs)


def twin(w, b, member, st):
    """the solo twin of a batch member at the applied state: the batch's K-splits and the member's chunk cuts"""
    g = make_solo(w, b, st, member.get_chunk_cuts())
    assert np.array_equal(g.get_chunk_cuts(), member.get_chunk_cuts())
    return applied(g)


def every7(w):
    return (np.arange(w.P) % 7 == 0).astype(np.int32)


def same_prior(name, got, want):
    (Hb, bb), (Hs, bs) = got, want
    assert Hb.shape == Hs.shape and bb.shape == bs.shape, name
    d = max(rel(Hb, Hs), rel(bb, bs)) if np.abs(Hs).max() > 0 else float(max(np.abs(Hb).max(), np.abs(bb).max()))
    print(name, "distance", d)
    observe(name, d, SAME)


def test_points_from_an_identical_applied_state():
    """flags: every seventh point (windows 0, 2, 5, 6), all points (1), no point (3: no prior, the result is zeros), None (4: the window with the prior)"""
    st = stream()
    wins = mixed_windows()
    batch, b = applied_batch(wins, st)
    flags = [every7(w) for w in wins]
    flags[1] = np.ones(wins[1].P, np.int32)
    flags[3] = np.zeros(wins[3].P, np.int32)
    flags[4] = None
    before = [g.get_residuals()["state_state"].copy() for g in batch]
    out = b.marginalize_points(flags)
    assert out[4] is None and all(o is not None for i, o in enumerate(out) if i != 4)
    for i, w in enumerate(wins):
        assert np.array_equal(batch[i].get_residuals()["state_state"], before[i]), i
        g = twin(w, b, batch[i], st)
        if flags[i] is None:
            # the window that took no part: its prior, read through the solo entry with no point flagged on both sides, is the one it was loaded with
            zero = np.zeros(w.P, np.int32)
            (Hb, bb), (Hs, bs) = batch[i].marginalize_points(zero), g.marginalize_points(zero)
            assert Hb.tobytes() == Hs.tobytes() and bb.tobytes() == bs.tobytes()
            assert np.array_equal(Hb, w.HM) and np.array_equal(bb, w.bM) and np.abs(w.HM).max() > 0
        else:
            n = 8 * w.F + 4
            assert out[i][0].shape == (n, n) and out[i][1].shape == (n,)
            want = g.marginalize_points(flags[i])
            same_prior("batch_marg_points_w%d" % i, out[i], want)
            assert (np.abs(want[0]).max() > 0) == (flags[i].sum() > 0), i
            if flags[i].sum() == 0:
                assert not out[i][0].any() and not out[i][1].any()
        g.close()
    b.close()


def test_points_after_a_batched_optimize():
    """The windows sit at different ping-pong parities; the twin runs its own optimize(6), so this crosses two optimisers whose states agree to 1e-9
    (observed on an MI355X: 5e-16 .. 8.1e-15 over the six windows)."""
    st = stream()
    wins = mixed_windows()[:6]
    batch, b = make_batch(wins, st)
    _, its, _ = b.optimize(6)
    assert len(set((its & 1).tolist())) == 2, its
    flags = [every7(w) for w in wins]
    out = b.marginalize_points(flags)
    for i, w in enumerate(wins):
        g = make_solo(w, b, st, batch[i].get_chunk_cuts())
        _, ns = g.optimize(6)
        assert ns == its[i]
        same_prior("batch_marg_points_after_optimize_w%d" % i, out[i], g.marginalize_points(flags[i]))
        g.close()
    b.close()


def test_points_twice_on_the_same_batch():
    """the second call adds onto the prior the first one left (window 4 brought one along)"""
    st = stream()
    wins = mixed_windows()
    batch, b = applied_batch(wins, st)
    f1 = [every7(w) for w in wins]
    f2 = [(np.arange(w.P) % 5 == 1).astype(np.int32) for w in wins]
    first = b.marginalize_points(f1)
    second = b.marginalize_points(f2)
    for i, w in enumerate(wins):
        g = twin(w, b, batch[i], st)
        s1 = g.marginalize_points(f1[i])
        s2 = g.marginalize_points(f2[i])
        same_prior("batch_marg_points_twice_first_w%d" % i, first[i], s1)
        same_prior("batch_marg_points_twice_second_w%d" % i, second[i], s2)
        assert rel(second[i][0], first[i][0]) > 1e-6, i          # ... and it did add something
        g.close()
    b.close()


def test_the_new_prior_reaches_the_iteration_kernels():
    """windows without a prior: batched marginalize_points, then batched optimize(6), against the same two steps on the twins"""
    st = stream()
    wins = [w for w in mixed_windows() if not np.any(w.HM)]
    assert len(wins) == 6
    batch, b = applied_batch(wins, st)
    flags = [every7(w) for w in wins]
    out = b.marginalize_points(flags)
    assert all(np.abs(o[0]).max() > 0 for o in out)
    rm, its, status = b.optimize(6)
    assert np.all(status == 0)
    for i, w in enumerate(wins):
        g = twin(w, b, batch[i], st)
        g.marginalize_points(flags[i])
        rs, ns = g.optimize(6)
        assert ns == its[i] and abs(rm[i] - rs) <= 1e-5 * rs, (i, ns, its[i], rs, rm[i])
        assert_equal(g, batch[i], i)
        g.close()
    b.close()


def test_points_with_balanced_chunking():
    """the eight windows of test_balanced_chunking: the batch re-cuts them and its launches walk wgStart"""
    st = stream()
    wins = [synth.add_synthetic_prior(synth.make_window(F=7, P=1750, w=320, h=240, fx=200.0, seed=60 + i)) for i in range(8)]
    batch, b = applied_batch(wins, st)
    assert b.chunk_points() >= 16, b.chunk_points()
    flags = [every7(w) for w in wins]
    out = b.marginalize_points(flags)
    for i in (0, 2, 7):
        g = twin(wins[i], b, batch[i], st)
        same_prior("batch_marg_points_balanced_w%d" % i, out[i], g.marginalize_points(flags[i]))
        g.close()
    b.close()


@functools.lru_cache(maxsize=None)
def oracle_cases():
    """three windows of different F at the oracle's post-optimize(3) state (the recipe of tests/test_ba_gpu.py::_marginalize_points): the window to load, the flags
    of flagPointsForRemoval after flagging a frame (the oldest, a middle one, the last but one), the oracle's H_M / b_M after marginalizePointsF.  The F = 5, 7 and 6
    windows (the last with a prior): in the 256 x 192 windows of mixed_windows() flagPointsForRemoval drops points and marginalises none."""
    cases = []
    for win, idx in ((mixed_windows()[0], 0), (mixed_windows()[2], 2), (mixed_windows()[4], 4)):
        o = po.OracleWindow(win); o.set_force_all_iterations(True)
        o.optimize(3)
        ex, fo = o.export_window(), o.get_frames()
        assert ex["F"] == win.F and len(ex["points"]) == win.P and np.array_equal(ex["orig_point"], np.arange(win.P))
        w2 = copy.deepcopy(win)
        w2.points, w2.residuals, w2.lin_J, w2.lin_res_toZeroF = ex["points"], ex["residuals"], ex["lin_J"], ex["lin_res_toZeroF"]
        w2.frames = fo["frames"]
        w2.calib = w2.calib.copy(); w2.calib["value"] = fo["calib_value"]
        o.flag_frame(idx)
        o.flag_points_for_removal()
        _, status = o.get_points()
        flags = (status == 3).astype(np.int32)                  # PS_MARGINALIZED
        o.drop_points()
        o.marginalize_points()
        HMo, bMo = o.get_prior()
        o.close()
        cases.append((w2, flags, HMo, bMo, ex["residuals"]["state_state"].copy()))
    return tuple(cases)


def test_points_against_the_oracle():
    st = stream()
    cases = oracle_cases()
    assert len({c[0].F for c in cases}) == 3
    for w2, flags, _, _, _ in cases:
        assert 0 < flags.sum() < w2.P, (w2.F, flags.sum())
    batch, b = make_batch([c[0] for c in cases], st)
    out = b.marginalize_points([c[1] for c in cases])
    for i, (w2, flags, HMo, bMo, state) in enumerate(cases):
        HMg, bMg = out[i]
        assert np.abs(HMo).max() > 0
        assert blockrel(HMg, HMo, 4) < TOL and rel(HMg, HMo) < TOL, (i, blockrel(HMg, HMo, 4), rel(HMg, HMo))
        assert rel(bMg, bMo) < TOL, (i, rel(bMg, bMo))
        assert np.abs(HMg - HMg.T).max() <= 1e-6 * np.abs(HMg).max()
        assert np.array_equal(batch[i].get_residuals()["state_state"], state)
    b.close()


FRAME_IDX = (0, 2, 5, -1, 3, 1, 0)          # per window of mixed_windows() (F = 5, 5, 7, 4, 6, 3, 2): first, middle, F-2, none, middle, F-2 (a middle one), F-2 (the first)


def with_full_rank_priors(wins, handles):
    """every window an explicit full-rank prior (tests/test_marg_frame_gpu.py: behind the rank-6 synthetic prior every index but 0 eliminates a singular block)"""
    priors = [_full_rank_prior(w, False) for w in wins]
    for g, (HM, bM) in zip(handles, priors):
        g.set_prior(HM, bM)
    return priors


def test_frames():
    st = stream()
    wins = mixed_windows()
    batch, b = make_batch(wins, st)
    priors = with_full_rank_priors(wins, batch)
    out = b.marginalize_frame(list(FRAME_IDX))
    again = b.marginalize_frame([None if k < 0 else k for k in FRAME_IDX])
    for i, w in enumerate(wins):
        if FRAME_IDX[i] < 0:
            assert out[i] is None and again[i] is None
            continue
        nd = 8 * (w.F - 1) + 4
        assert out[i][0].shape == (nd, nd) and out[i][1].shape == (nd,)
        g = make_solo(w, b, st, batch[i].get_chunk_cuts())
        g.set_prior(*priors[i])
        Hs, bs = g.marginalize_frame(FRAME_IDX[i])
        assert np.abs(Hs).max() > 0 and np.all(np.isfinite(Hs)) and np.all(np.isfinite(bs))
        assert out[i][0].tobytes() == Hs.tobytes() and out[i][1].tobytes() == bs.tobytes(), (i, rel(out[i][0], Hs), rel(out[i][1], bs))
        assert again[i][0].tobytes() == Hs.tobytes() and again[i][1].tobytes() == bs.tobytes(), i
        g.close()
    # the output buffers of a window that takes no part are not written (the C entry, with buffers behind every slot)
    n = len(wins)
    bufs = [(np.full((8 * (w.F - 1) + 4,) * 2, 7.25), np.full(8 * (w.F - 1) + 4, -3.5)) for w in wins]
    PH = (C.c_void_p * n)(*[h.ctypes.data for h, _ in bufs])
    Pb = (C.c_void_p * n)(*[v.ctypes.data for _, v in bufs])
    idx = np.array(FRAME_IDX, np.int32)
    assert b.L.ldso_ba_batch_marginalize_frame(b.h, binding._p(idx), PH, Pb) == 0
    for i in range(n):
        if FRAME_IDX[i] < 0:
            assert np.all(bufs[i][0] == 7.25) and np.all(bufs[i][1] == -3.5)
        else:
            assert bufs[i][0].tobytes() == out[i][0].tobytes() and bufs[i][1].tobytes() == out[i][1].tobytes()
    b.close()


def test_the_chain_points_then_frames():
    """the frame kernel reads the prior the points kernels left on the device: twin i gets the batch's own (HM_i, bM_i) through set_prior"""
    st = stream()
    wins = mixed_windows()
    batch, b = applied_batch(wins, st)
    with_full_rank_priors(wins, batch)
    pts = b.marginalize_points([every7(w) for w in wins])
    idx = [k if k >= 0 else 1 for k in FRAME_IDX]
    out = b.marginalize_frame(idx)
    for i, w in enumerate(wins):
        g = make_solo(w, b, st, batch[i].get_chunk_cuts())
        g.set_prior(*pts[i])
        Hs, bs = g.marginalize_frame(idx[i])
        assert np.abs(Hs).max() > 0
        assert out[i][0].tobytes() == Hs.tobytes() and out[i][1].tobytes() == bs.tobytes(), (i, rel(out[i][0], Hs), rel(out[i][1], bs))
        g.close()
    b.close()


def test_refusals():
    st = stream()
    # windows of more than 8 key frames: both entries, the wording of ldso_ba_batch_optimize
    wins = [synth.make_window(F=9, P=100, w=256, h=192, fx=160.0, seed=40 + i) for i in range(2)]
    batch, b = make_batch(wins, st)
    with pytest.raises(binding.LdsoError) as e:
        b.marginalize_points([every7(w) for w in wins])
    assert e.value.code == -1 and "F <= 8" in str(e.value) and "ldso_ba_batch_marginalize_points" in str(e.value)
    with pytest.raises(binding.LdsoError) as e:
        b.marginalize_frame([0, 0])
    assert e.value.code == -1 and "F <= 8" in str(e.value) and "ldso_ba_batch_marginalize_frame" in str(e.value)
    b.close()
    wins = mixed_windows()[:3]
    batch, b = make_batch(wins, st)
    # a frame index that is no key frame of its window
    with pytest.raises(binding.LdsoError) as e:
        b.marginalize_frame([0, wins[1].F, 0])
    assert e.value.code == -1 and "ldso_ba_batch_marginalize_frame" in str(e.value)
    # NULL flags / frame_idx
    for entry in ("ldso_ba_batch_marginalize_points", "ldso_ba_batch_marginalize_frame"):
        assert getattr(b.L, entry)(b.h, None, None, None) == -1 and entry in b.L.ldso_last_error().decode()
    # a pending linearizeAll result (linearize_all without apply_res)
    batch[1].linearize_all()
    with pytest.raises(binding.LdsoError) as e:
        b.marginalize_points([every7(w) for w in wins])
    assert e.value.code == -1 and "pending" in str(e.value) and "ldso_ba_batch_marginalize_points" in str(e.value)
    with pytest.raises(binding.LdsoError) as e:
        b.marginalize_frame([0, 0, 0])
    assert e.value.code == -1 and "pending" in str(e.value)
    # ... which does not concern a window that takes no part
    batch[1].apply_res()
    assert b.marginalize_points([None, None, None]) == [None, None, None]
    b.close()
