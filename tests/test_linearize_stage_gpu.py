"""linearize_body (ldso_amd/csrc/ba_linearize_body.h) entry by entry against the float64 reference of tests/linearize_stage_common.py, in units of eps32 x the sum of
the |addends| of every entry, through every route that reaches a different instantiation.  The bound per quantity is max(FLOOR_UNITS, ORACLE_FACTOR x yardstick), the
yardstick being the oracle's own distance from the reference (tests/test_linearize_stage_cpu.py); decisions outside the guards are compared bit for bit.

Routes, and why each reaches the kernel it is named for (launch_linearize, ba_optimize.hip; ba_launch_linearize_one / ba_launch_linearize, ba_linearize.hip):
  plain   collect_active -> linearize_all(False) -> apply_res.  launch_linearize takes ba_launch_linearize_one when the pass does not fix, the window has no linearised
          residuals, the chunks are regular (linHeadOk: every host cut into pieces of CH points - asserted here by rebuilding the cuts from the hosts' point counts)
          and no Jacobian dump is set: k_linearize_one<1> for F <= 8, <2, true> (pair mode) for F = 9..12, <2> for F = 13..16.  Chunks of at most 4 points give a
          wavefront at most one point (the peeled first iteration alone); set_chunk_points(12 | 20 | 36) gives 9..16, 17..24 and more than 32 points per chunk, the
          pipelined point loop, with a ragged last chunk of one or two points per host.
  dump    the same pass under set_debug_dump(True): B.dumpJ != nullptr sends launch_linearize to the argument-based k_linearize, and get_jacobians() returns what it
          wrote - resF, JIdx, JabF, Jpdxi, Jpdc, Jpdd, JIdx2, JabJIdx, Jab2 are held entry by entry.
  mixed   a window with linearised residuals (get_counts() shows them): H->hasL sends both passes to k_linearize<.., HAS_L = true, ..>; the *_accLF triple, HL and bL
          are held too.
  fused   enqueue_gn(0, 1): one iteration on the plain path (iters < 2: no graph) = k_reduce -> k_gn_solve -> the linearisation with stepMode = 1, the point step
          fused in front of every point.  Frames, calibration, inverse depths and get_precalc() are fetched AFTER the step and the reference is evaluated there
          (doStepFromBackup moves idepth_zero with idepth); the new set's per-residual outputs and per-point accumulators are held, then HFinal | bFinal of one
          gn_reduce_local on it.  (HdiF / bdSumF / idepth_hessian are those of the solve BEFORE the step by then: they are held on the plain route.)
  batch   BABatch of three handles (F = 3, 5, 8, the batch's own chunking, printed) through BABatch.enqueue_gn(0, 1): k_linearize_batch<1>, held like `fused`.
Both system forms are held on the plain and dump routes: HA, bA, Hsc, bsc (HL, bL) as get_system() returns them after solve_system(0), and the lower triangle of
HFinal | bFinal of one gn_reduce_local into a zeroed buffer.

Left out on purpose: the fixing pass and the marginalisation accumulate (FIX, MARG) - their outputs cannot be fetched on their own and are covered against the oracle
in test_ba_gpu.py and test_marg_frame_gpu.py; windows of 9..16 key frames in a batch, which are kept out of batches; non-finite inputs (tests/test_nonfinite_gpu.py).

Every test prints its worst units per quantity and its adoption count, and records them through conftest.observe."""
import numpy as np
import pytest

from conftest import observe
from ldso_amd import binding
import linearize_stage_common as common

pytestmark = pytest.mark.gpu

IDS = list(common.CASES)


def _stream():
    import torch
    ts = torch.cuda.Stream(); torch.cuda.set_stream(ts)          # one non-default stream for torch and the handles
    return ts


def _handle(name, st):
    """the case's window on a handle with the chunking the case is named for; asserts the chunk sizes, and that they are the regular cut of every host"""
    win = common.case_window(name)
    F, _, _, ch, shows, _ = common.CASES[name]
    g = binding.BA.from_window(win, stream=st.cuda_stream)
    if ch:
        g.set_chunk_points(ch)
    sizes = common.chunk_sizes(g.get_chunk_cuts())
    assert shows(sizes), (name, sizes)
    per_host = np.bincount(win.points["host"], minlength=win.F)
    CH = ch or 4
    regular = [c for n in per_host for c in [CH] * (n // CH) + ([n % CH] if n % CH else [])]
    assert list(sizes) == regular, (name, "the chunks are not the regular cut k_linearize_one reads in closed form", sizes, regular)
    assert g.F == F == win.F
    return win, g


def _hold(route, name, got, ref, point_solve=True):
    un = common.check(got, ref, f"{route} {name}", point_solve)
    bd = common.bounds()
    for q, v in un.items():
        observe(f"linearize_stage/{route}/{name}/{q}", v, bd[q])
    return un


def _final(g, n):
    """HFinal | bFinal of one gn_reduce_local into a zeroed buffer -> the buffer (the handle's accumulator points into it from now on: keep it until the handle is
    closed) and (H [n, n], b [n])"""
    import torch
    buf = torch.zeros(g.gn_reduce_doubles(), dtype=torch.float64, device="cuda")
    g.gn_reduce_local(buf.data_ptr(), 1e-1)
    g.sync(); torch.cuda.synchronize()
    a = buf.cpu().numpy()
    return buf, (a[:n * n].reshape(n, n).copy(), a[n * n:n * n + n].copy())


def _pass(name, dump):
    st = _stream()
    win, g = _handle(name, st)
    inp = common.make_inputs(win, g.get_precalc())
    g.collect_active()
    g.set_debug_dump(dump)
    g.linearize_all(False)
    J = g.get_jacobians() if dump else None
    g.set_debug_dump(False)
    g.apply_res()
    out = g.get_residuals()["out"]
    g.backup_state(); g.solve_system(0)
    sysd, pts = g.get_system(), g.get_points()
    a, l = g.get_counts()
    assert (l > 0) == bool(win.residuals["is_linearized"].any()), (name, a, l)
    buf, final = _final(g, 8 * win.F + 4)
    got = common.got_of(out, J, pts, sysd, final)
    ref = common.reference(inp, got)
    assert ref.has_L == (l > 0)
    _hold("dump" if dump else "plain", name, got, ref)
    g.close()


@pytest.mark.parametrize("name", IDS)
def test_plain_pass(name):
    _pass(name, False)


@pytest.mark.parametrize("name", IDS)
def test_debug_dump_pass(name):
    _pass(name, True)


def _after_step(route, name, win, g, before):
    """hold the set a fused step left on handle g to the reference evaluated at the state fetched after the step"""
    fr, pts, after = g.get_frames(), g.get_points(), g.get_residuals()
    assert np.abs(fr["frames"]["state"] - win.frames["state"]).max() > 0 and (pts["idepth"] != win.points["idepth"]).any(), "the step moved nothing"
    inp = common.make_inputs(win, g.get_precalc(), frames=fr["frames"], calib_value=fr["calib_value"], idepth=pts["idepth"], idepth_zero=pts["idepth"],
                             state=before["state_state"], active=before["is_active"])
    buf, final = _final(g, 8 * win.F + 4)
    got = common.got_of(after["out"], None, pts, None, final)
    ref = common.reference(inp, got)
    _hold(route, name, got, ref, point_solve=False)
    return buf


@pytest.mark.parametrize("name", IDS)
def test_fused_point_step(name):
    st = _stream()
    win, g = _handle(name, st)
    g.collect_active(); g.linearize_all(False); g.apply_res()
    before = g.get_residuals()
    g.enqueue_gn(0, 1); g.sync()
    buf = _after_step("fused", name, win, g, before)
    g.close()


BATCH = ("F3", "F5_default", "F8")


def test_batched_fused_step():
    st = _stream()
    wins, hs, before = [], [], []
    for name in BATCH:
        win = common.case_window(name)
        g = binding.BA.from_window(win, stream=st.cuda_stream)
        g.collect_active(); g.linearize_all(False); g.apply_res()
        wins.append(win); hs.append(g); before.append(g.get_residuals())
    assert [g.F for g in hs] == [3, 5, 8]
    b = binding.BABatch(hs)
    print("batch chunking", b.chunk_points(), [list(common.chunk_sizes(g.get_chunk_cuts())) for g in hs])
    b.enqueue_gn(0, 1); b.sync()
    bufs = [_after_step("batch", name, win, g, r0) for name, win, g, r0 in zip(BATCH, wins, hs, before)]
    b.close()
    for g in hs:
        g.close()
