"""ldso_ba_batch_optimize: FullSystem::optimize() on a batch of windows.  Every window of the batch must end where ldso_ba_optimize leaves its twin handle
("solo": split launches, the batch's K-splits and - where the batch re-cut them - its chunks), with the bounds the batch tests of test_ba_gpu.py use:
frame state 1e-9 of its maximum, frameEnergyTH / residual states / activity / removal flags equal, idepth 1e-6, HdiF 1e-5, residual energies, energy log and
rmse 1e-5 relative, identical iteration counts.  All tests run on one torch stream."""
import functools

import numpy as np
import pytest

from conftest import rel
from ldso_amd import synth, binding
from oracle import pyoracle as po
from test_ref_pin import nonfinite_windows

pytestmark = pytest.mark.gpu
LDSO_OK, LDSO_E_NONFINITE = 0, -3


@functools.lru_cache(maxsize=None)
def mixed_windows():
    """different scenes, point and frame counts, one prior; the last two run to the cap of 15 (F < 4), the F = 2 window never reaches canbreak"""
    return (synth.make_window(F=5, P=400, w=320, h=240, fx=200.0, seed=31), synth.make_window(F=5, P=333, w=320, h=240, fx=200.0, seed=32),
            synth.make_window(F=7, P=500, w=320, h=240, fx=200.0, seed=33), synth.make_window(F=4, P=150, w=256, h=192, fx=160.0, seed=34),
            synth.add_synthetic_prior(synth.make_window(F=6, P=420, w=320, h=240, fx=200.0, seed=35)),
            synth.make_window(F=3, P=200, w=256, h=192, fx=160.0, seed=36), synth.make_window(F=2, P=120, w=256, h=192, fx=160.0, seed=38))


@functools.lru_cache(maxsize=None)
def oracle_mixed():
    """the CPU oracle's un-forced optimize(6) on mixed_windows(): (iterations, rmse) per window"""
    out = []
    for w in mixed_windows():
        o = po.OracleWindow(w)
        rm = o.optimize(6)
        out.append((len(o.energy_log()) - 2, rm))
    return tuple(out)


def stream():
    import torch
    ts = torch.cuda.Stream(); torch.cuda.set_stream(ts)
    return ts.cuda_stream


def make_batch(wins, st):
    hs = [binding.BA.from_window(w, stream=st) for w in wins]
    return hs, binding.BABatch(hs)


def make_solo(w, b, st, cuts=None):
    g = binding.BA.from_window(w, stream=st)
    if cuts is not None:
        g.set_chunk_cuts(cuts)
    g.set_debug_split_launch(True)
    g.set_reduce_splits(b.reduce_splits())
    return g


def assert_equal(gs, gb, tag):
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


def test_mixed_batch_with_different_stop_iterations():
    """Seven windows that stop after 5, 4, 4, 4, 3, 4 and 15 iterations (the oracle's counts): both parities in each half of the batch, two windows with a cap
    of their own, windows idling through up to 12 launches that are no-ops for them."""
    st = stream()
    wins = mixed_windows()
    batch, b = make_batch(wins, st)
    rm, its, status = b.optimize(6)
    print("iterations", its.tolist(), "rmse", rm.tolist())
    assert np.all(status == LDSO_OK)
    want = [o[0] for o in oracle_mixed()]
    assert its.tolist() == want, (its.tolist(), want)
    assert len(set(its.tolist())) > 1
    for i, w in enumerate(wins):
        g = make_solo(w, b, st)
        rs, ns = g.optimize(6)
        assert ns == its[i] and abs(rm[i] - rs) <= 1e-5 * rs, (i, ns, its[i], rs, rm[i])
        assert_equal(g, batch[i], i)
        assert len(batch[i].get_energy_log()) == its[i] + 2
        assert abs(rm[i] - oracle_mixed()[i][1]) <= 1e-4 * oracle_mixed()[i][1], (i, rm[i], oracle_mixed()[i][1])
        g.close()
    b.close()


def test_twice_on_the_same_batch():
    """the second call starts from windows at different ping-pong parities"""
    st = stream()
    wins = mixed_windows()[:6]
    batch, b = make_batch(wins, st)
    _, its1, _ = b.optimize(6)
    assert len(set((its1 & 1).tolist())) == 2, its1          # ... which this batch really has
    rm, its, status = b.optimize(6)
    assert np.all(status == LDSO_OK)
    for i, w in enumerate(wins):
        g = make_solo(w, b, st)
        g.optimize(6)
        rs, ns = g.optimize(6)
        assert ns == its[i] and abs(rm[i] - rs) <= 1e-5 * rs, (i, ns, its[i], rs, rm[i])
        assert_equal(g, batch[i], i)
        g.close()
    b.close()


def test_forced_iterations():
    st = stream()
    wins = mixed_windows()[:5]
    batch, b = make_batch(wins, st)
    rm, its, status = b.optimize(4, force_all=True)
    assert its.tolist() == [4] * 5 and np.all(status == LDSO_OK)
    for i, w in enumerate(wins):
        g = make_solo(w, b, st)
        rs, ns = g.optimize(4, force_all=True)
        assert ns == 4 and abs(rm[i] - rs) <= 1e-5 * rs
        assert_equal(g, batch[i], i)
        assert len(batch[i].get_energy_log()) == 6
        g.close()
    b.close()


def test_balanced_chunking():
    """a batch that ldso_ba_batch_create cuts unevenly (one workload per workgroup): the solo twins get the batch's cuts.  The oracle stops these windows
    after 4, 4, 3, 4, 3, 3, 3 and 4 iterations."""
    st = stream()
    wins = [synth.add_synthetic_prior(synth.make_window(F=7, P=1750, w=320, h=240, fx=200.0, seed=60 + i)) for i in range(8)]
    batch, b = make_batch(wins, st)
    assert b.chunk_points() >= 16, b.chunk_points()
    cuts = [g.get_chunk_cuts() for g in batch]
    rm, its, status = b.optimize(6)
    print("iterations", its.tolist())
    assert np.all(status == LDSO_OK)
    for i in (0, 2, 7):
        g = make_solo(wins[i], b, st, cuts[i])
        assert np.array_equal(g.get_chunk_cuts(), cuts[i])
        rs, ns = g.optimize(6)
        assert ns == its[i] and abs(rm[i] - rs) <= 1e-5 * rs, (i, ns, its[i], rs, rm[i])
        assert_equal(g, batch[i], i)
        g.close()
    b.close()


def test_one_nonfinite_window_does_not_touch_the_others(small):
    st = stream()
    wins = [mixed_windows()[0], nonfinite_windows(small)["nan_gradient"], mixed_windows()[2], mixed_windows()[3]]
    batch, b = make_batch(wins, st)
    n = len(wins)
    rm, it, status = np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    code = b.L.ldso_ba_batch_optimize(b.h, 6, 0, binding._p(rm), binding._p(it), binding._p(status))
    assert code == LDSO_E_NONFINITE
    assert status.tolist() == [LDSO_OK, LDSO_E_NONFINITE, LDSO_OK, LDSO_OK]
    for i in (0, 2, 3):          # the healthy windows are where a lone optimize(6) leaves them
        g = make_solo(wins[i], b, st)
        rs, ns = g.optimize(6)
        assert ns == it[i] and abs(rm[i] - rs) <= 1e-5 * rs, (i, ns, it[i], rs, rm[i])
        assert_equal(g, batch[i], i)
        g.close()
    _, _, status2 = b.optimize(6)          # the binding reports the verdict per window and does not raise on it
    assert status2.tolist() == [LDSO_OK, LDSO_E_NONFINITE, LDSO_OK, LDSO_OK]
    b.close()


def test_handles_are_usable_afterwards():
    st = stream()
    wins = mixed_windows()[:4]
    batch, b = make_batch(wins, st)
    rm, its, _ = b.optimize(6)
    solo = make_solo(wins[0], b, st)
    solo.optimize(6)
    b.close()
    res = batch[0].get_results()
    assert np.array_equal(res["residuals"]["state_state"], solo.get_residuals()["state_state"])
    assert np.array_equal(res["frames"]["frames"]["state"], batch[0].get_frames()["frames"]["state"])
    flags = (np.arange(wins[0].P) % 7 == 0).astype(np.int32)
    (Hs, bs), (Hb, bb) = solo.marginalize_points(flags), batch[0].marginalize_points(flags)
    assert np.abs(Hs).max() > 0 and rel(Hb, Hs) <= 1e-9 and rel(bb, bs) <= 1e-9
    solo.close()


def test_refusals():
    st = stream()
    # a window with a single key frame never becomes resident (ldso_ba_set_window wants two), so no batch can contain one: the refusal comes from there,
    # and the F >= 2 test of ldso_ba_batch_optimize itself cannot be reached through the interface
    with pytest.raises(binding.LdsoError) as e:
        binding.BA.from_window(synth.make_window(F=1, P=50, w=256, h=192, fx=160.0, seed=39), stream=st)
    assert e.value.code == -1 and "ldso_ba_set_window" in str(e.value)
    # windows of more than 8 key frames
    wins = [synth.make_window(F=9, P=100, w=256, h=192, fx=160.0, seed=40 + i) for i in range(2)]
    batch, b = make_batch(wins, st)
    with pytest.raises(binding.LdsoError) as e:
        b.optimize(6)
    assert e.value.code == -1 and "F <= 8" in str(e.value)
    b.close()
    # ldso_ba_batch_enqueue_gn keeps its condition: after optimize() the windows sit at different parities
    batch, b = make_batch(mixed_windows()[:4], st)
    _, its, _ = b.optimize(6)
    assert len(set((its & 1).tolist())) == 2, its
    with pytest.raises(binding.LdsoError) as e:
        b.enqueue_gn(0, 1)
    assert "same stage" in str(e.value)
    b.close()
