"""The hand-over inside k_reduce_solve: the reduce workgroups arrive on several words (ba_dev.h: arrive_shard) and the first wavefront of the control
workgroup waits on every word for its share of the arrivers (arrive_target), re-arms the words and only then loads the system.  A share that is too small
lets the control workgroup read a system that is still being summed, one that is too large ends its bounded poll in the non-finite status; a word that is
not re-armed breaks the next launch.

Every case: a 320 x 240 window with the synthetic prior.  Every test also reads the arrival words back (all zero between launches) through
ldso_ba_get_arrival_words, which reports the non-finite status - where a poll that ran out ends - as an error.

One fused iteration against the split launch (ldso_ba_set_debug_split_launch: k_reduce, then k_gn_solve behind a kernel boundary - the same reduce_body and
the same solve, no hand-over): fresh handles, collect_active -> linearize_all -> apply_res -> enqueue_gn(0, 1), x from ldso_ba_get_system.  Ten split-launch
repetitions give `spread`, the largest entrywise difference of x among them (the arrival order of the fp64 atomics); the fused x may differ from the first of
them by 4 x spread - two runs' worth of atomic order, doubled for the small sample (the rule of tests/test_reduce_tiles_gpu.py).
Arrivers = F^2 (1 + hasL) + 15 ks + 1:
  F2 P6 ks1    20   the smallest fused grid, words with 1 and 2 arrivers, K-splits without rows      F2 P64 ks3     50
  F7 P64 ks8   170  the count of the 7-frame benchmark window, no multiple of the word count        F5 P400 ks12   206
  F8 P64 ks8 mixed  249  linearised residuals: pair workgroups doubled, the largest launch that still fuses      F8 P64 ks8   185
"""
import functools

import numpy as np
import pytest

from conftest import observe, rel
from ldso_amd import binding, synth

pytestmark = pytest.mark.gpu

TOL = 1e-4          # the project's tolerance against the oracle (energies)
# name, F, P, K-splits per tile, linearised residuals, arrivers
CASES = [
    ("F2_P6_ks1", 2, 6, 1, False, 20),
    ("F2_P64_ks3", 2, 64, 3, False, 50),
    ("F7_P64_ks8", 7, 64, 8, False, 170),
    ("F5_P400_ks12", 5, 400, 12, False, 206),
    ("F8_P64_ks8_mixed", 8, 64, 8, True, 249),
    ("F8_P64_ks8", 8, 64, 8, False, 185),
]


@functools.lru_cache(maxsize=None)
def make_win(F, P, mixed=False):
    win = synth.add_synthetic_prior(synth.make_config("small", F=F, P=P))
    if mixed:
        from oracle import pyoracle as po
        win = po.make_mixed_window(win)
    return win


def words_clean(g):
    """the arrival words behind a synchronisation: re-armed, and the bounded poll never ran out (get_arrival_words raises on the non-finite status)"""
    w = g.get_arrival_words()
    assert len(w) == len(binding.arrival_targets(0)) and not w.any(), w


def one_iteration(win, splits, split_launch):
    g = binding.BA.from_window(win)
    g.set_reduce_splits(splits)
    g.set_debug_split_launch(split_launch)
    g.collect_active(); g.linearize_all(False); g.apply_res()
    g.enqueue_gn(0, 1); g.sync()
    x = g.get_system()["x"].copy()
    words_clean(g)
    g.close()
    return x


@pytest.mark.parametrize("name,F,P,splits,mixed,arrivers", CASES, ids=[c[0] for c in CASES])
def test_fused_iteration_against_the_split_launch(name, F, P, splits, mixed, arrivers):
    win = make_win(F, P, mixed)
    has_l = int(np.sum(win.residuals["is_linearized"])) > 0
    assert has_l == mixed and F * F * (2 if has_l else 1) + 15 * splits + 1 == arrivers
    assert int(binding.arrival_targets(arrivers).sum()) == arrivers
    ref = [one_iteration(win, splits, True) for _ in range(10)]
    spread = max(float(np.abs(a - b).max()) for a in ref for b in ref)
    x = one_iteration(win, splits, False)
    assert np.isfinite(x).all() and np.abs(x).max() > 0
    diff = float(np.abs(x - ref[0]).max())
    print(f"{name}: fused against the first split launch {diff:.3e}, spread of ten split launches {spread:.3e} (allowed {4 * spread:.3e}), |x| max {np.abs(x).max():.3e}")
    observe(f"reduce_arrival_spread_{name}", spread, np.inf)
    observe(f"reduce_arrival_fused_vs_split_{name}", diff, 4 * spread)


def test_rearm_and_graph_replay():
    """One handle, forced iterations 0..1, then twice iterations 2..41: the second call replays the graph the first one captured, so 82 launches run on words
    nobody cleared in between but the control workgroup.  The energy the handle reports for the state it ends in (k_reduce alone, as bench.py's parity check
    reads it) against the oracle's evaluation of that state."""
    import torch
    from oracle import pyoracle as po
    from test_fullsize_gpu import _transplant
    win = make_win(7, 64)
    g = binding.BA.from_window(win)
    g.collect_active(); g.linearize_all(False); g.apply_res()
    g.enqueue_gn(0, 2)
    g.enqueue_gn(2, 40)
    g.enqueue_gn(2, 40)
    g.sync()
    words_clean(g)
    n = 8 * win.F + 4
    buf = torch.zeros(g.gn_reduce_doubles(), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    g.gn_reduce_local(buf.data_ptr(), 1e-1); g.sync(); torch.cuda.synchronize()
    e_gpu = float(buf[n * n + n].item())
    fr = g.get_frames()
    assert np.isfinite(fr["frames"]["state"]).all() and np.isfinite(fr["calib_value"]).all() and np.isfinite(g.get_points()["idepth"]).all()
    o = po.OracleWindow(_transplant(win, g)); o.collect_active(reset_oob=False)
    e_orc = o.linearize_all(False); o.close()
    g.close()
    observe("reduce_arrival_graph_replay_energy", abs(e_gpu - e_orc) / abs(e_orc), TOL)


def test_skipped_iterations_leave_the_words_alone():
    """Un-forced optimize(6): the device decides where the loop ends, and the launches of the later iterations return at their first instruction - on both sides
    of the hand-over, so nobody arrives and nobody waits.  Then the same once more on the same handle.  Energy logs against the oracle's, which runs the same
    two calls."""
    from oracle import pyoracle as po
    win = make_win(5, 400)
    o = po.OracleWindow(win)
    g = binding.BA.from_window(win)
    for call in range(2):
        o.optimize(6)
        _, its = g.optimize(6, force_all=False)
        eo, eg = np.array(o.energy_log()), np.array(g.get_energy_log())
        print(f"call {call}: {its} iterations, energy log against the oracle {rel(eg, eo) if len(eg) == len(eo) else float('nan'):.3e}")
        assert its == len(eo) - 2 and len(eg) == len(eo)
        if call == 0:
            assert its < 6, "no iteration was skipped: the case does not reach what it is for"
        observe(f"reduce_arrival_skipped_energy_log_{call}", rel(eg, eo), TOL)
        words_clean(g)
    o.close(); g.close()
