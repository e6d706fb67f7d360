"""ldso_ba_batch_update_windows / ldso_ba_batch_set_frames (include/ldso_hip.h): every window of a batch becomes its next one in one call, and the batch re-cuts itself.

Every test runs two sets of handles from the same start (tests/batch_update_common.py; windows of different seeds and edit kinds - "steady", "points-only", "middle" -
so that F, P, R and the number of fresh points differ inside one batch):
  set X   BABatch -> optimize(3, force_all) -> batch.update_windows -> batch.set_frames
  set Y   the yardstick, on the entries that were there before: the same start -> batch closed -> per handle update_window, set_frames, set_prior -> a new BABatch
The deltas are derived once, from X's state after the optimize, and applied to both.  Per handle X and Y must then be the same bytes - dimensions, residual states /
activity / energies, every point field, the frames with their precalc values, the chunk cuts (= the re-balance is the one ldso_ba_batch_create makes) - and the
optimize() that follows must agree within 1e-5 relative (the limit tests/test_batch_optimize_gpu.py uses between two device paths) with equal iteration counts and
residual states.  The chunk policy's threshold is total points / (CUs * 8 wavefronts): below 2 regular chunks, from 2 on balanced cuts."""
import numpy as np
import pytest

from conftest import rel
from ldso_amd import binding
import batch_update_common as bu

pytestmark = pytest.mark.gpu
LD_WAVES = 8
KIND_ORDER = ("steady", "points-only", "middle")


def stream():
    import torch
    ts = torch.cuda.Stream(); torch.cuda.set_stream(ts)
    return ts.cuda_stream


def ppw(handles):
    """points per wavefront slot of the chip, as the chunk policy counts them (the CU count read as the library reads it)"""
    import torch
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    return sum(h.P for h in handles) // (cu * LD_WAVES)


def specs(B, P):
    return [(KIND_ORDER[i % 3], P, 11 + i) for i in range(B)]


def begin(sp, st):
    """the common start of both sets: handles with their old windows in a batch that has run optimize(3)"""
    sts = [bu.start(*s) for s in sp]
    hs = [bu.load(s, st) for s in sts]
    bt = binding.BABatch(hs)
    bt.optimize(3, force_all=True)
    return sts, hs, bt


def frames_args(scs, sit_out=()):
    fr = [None if i in sit_out else sc["w1"].frames for i, sc in enumerate(scs)]
    return fr, [sc["w1"].calib for sc in scs], [(sc["w1"].HM, sc["w1"].bM) for sc in scs]


def apply_x(bt, scs, sit_out=()):
    bt.update_windows([None if i in sit_out else sc["job"] for i, sc in enumerate(scs)])
    bt.set_frames(*frames_args(scs, sit_out))


def apply_y(bt, hs, scs, sit_out=()):
    bt.close()
    for i, (h, sc) in enumerate(zip(hs, scs)):
        if i in sit_out:
            continue
        h.update_window(*sc["job"])
        h.set_frames(sc["w1"].frames, sc["w1"].calib); h.set_prior(sc["w1"].HM, sc["w1"].bM)
    return binding.BABatch(hs)


def same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.tobytes() == b.tobytes(), f"{what}: {int((a != b).sum()) if a.shape == b.shape and a.dtype.names is None else 'shape / records'} differ"


def window_bytes(h):
    """what the tests compare of a handle, as named arrays"""
    r, p, f = h.get_residuals(), h.get_points(), h.get_frames()
    out = {"dims": np.array([h.F, h.P, h.R]), "res.state_state": r["state_state"], "res.is_active": r["is_active"], "res.state_NewEnergy": r["out"]["state_NewEnergy"],
           "cuts": h.get_chunk_cuts(), "precalc": h.get_precalc()}
    for k in p.dtype.names:
        out["point." + k] = p[k]
    for k, v in f.items():
        out["frames." + k] = v
    return out


def assert_same_window(hx, hy, tag, skip=()):
    bx, by = window_bytes(hx), window_bytes(hy)
    for k in bx:
        if not k.startswith(skip or "\0"):
            same(bx[k], by[k], f"{tag}: {k}")


def assert_same_optimize(bx, hsx, by, hsy, tag):
    rx, ix, sx = bx.optimize(4, force_all=True); ry, iy, sy = by.optimize(4, force_all=True)
    assert np.array_equal(ix, iy) and np.array_equal(sx, sy), (tag, ix, iy)
    assert rel(rx, ry) < 1e-5, (tag, rx, ry)
    for i, (hx, hy) in enumerate(zip(hsx, hsy)):
        ex, ey = hx.get_energy_log(), hy.get_energy_log()
        print(tag, "window", i, "energy log", ex.tolist(), "rel", rel(ex, ey))
        assert len(ex) == len(ey) and rel(ex, ey) < 1e-5, (tag, i, ex, ey)
        same(hx.get_residuals()["state_state"], hy.get_residuals()["state_state"], f"{tag}: window {i} state_state after optimize")


def run_pair(B, P, keep=0.9, sit_out=()):
    st = stream()
    sp = specs(B, P)
    sts, hx, bx = begin(sp, st)
    _, hy, by = begin(sp, st)
    scs = [bu.edit(s, h, keep) for s, h in zip(sts, hx)]
    return sts, scs, hx, bx, hy, by


def close_all(*things):
    for t in things:
        for x in (t if isinstance(t, (list, tuple)) else [t]):
            x.close()


def test_update_equals_single_window_path_regular_chunks():
    sts, scs, hx, bx, hy, by = run_pair(2, 600)
    assert ppw(hx) < 2 and not bx.balanced()
    apply_x(bx, scs); by = apply_y(by, hy, scs)
    assert ppw(hx) < 2 and not bx.balanced() and not by.balanced() and bx.chunk_points() == by.chunk_points() == 0          # regular mode, single-window chunks kept
    assert len({(h.F, h.P, h.R) for h in hx}) == 2
    for i, (x, y, sc) in enumerate(zip(hx, hy, scs)):
        assert sc["n_survive"] > 100 and sc["n_fresh"] > 20 and sc["n_dropped"] > 5
        assert (x.F, x.P, x.R) == (sc["w1"].F, sc["w1"].P, sc["w1"].R)
        assert_same_window(x, y, f"window {i}")
        same(x.get_residuals()["state_state"], sc["w1"].residuals["state_state"], f"window {i}: state_state against the host objects")
        assert x.get_prior()[2] and y.get_prior()[2]
        same(x.get_prior()[0], y.get_prior()[0], f"window {i}: prior")
    assert_same_optimize(bx, hx, by, hy, "regular")
    close_all(bx, by, hx, hy)


def test_update_rebalances_like_batch_create():
    """six windows, two halves of three (n0 < n), balanced before and after the edit: the cuts of every window and the two-half launches are those of a fresh batch"""
    sts, scs, hx, bx, hy, by = run_pair(6, 1400)
    assert ppw(hx) >= 2 and bx.balanced()
    before = [h.get_chunk_cuts() for h in hx]
    apply_x(bx, scs); by = apply_y(by, hy, scs)
    assert ppw(hx) >= 2 and bx.balanced() and by.balanced() and bx.chunk_points() == by.chunk_points() > 0
    assert len({(h.F, h.P) for h in hx}) >= 3
    for i, (x, y, sc) in enumerate(zip(hx, hy, scs)):
        assert_same_window(x, y, f"window {i}")
        same(x.get_residuals()["state_state"], sc["w1"].residuals["state_state"], f"window {i}: state_state against the host objects")
        assert len(before[i]) != len(x.get_chunk_cuts()) or not np.array_equal(before[i], x.get_chunk_cuts())
    assert_same_optimize(bx, hx, by, hy, "balanced")
    close_all(bx, by, hx, hy)


def test_update_changes_the_chunk_mode_with_the_totals():
    """the edit removes so many points that the total drops below the balanced threshold: the batch ends in the regular mode with the cuts a fresh batch has"""
    sts, scs, hx, bx, hy, by = run_pair(6, 1400, keep=0.3)
    assert ppw(hx) >= 2 and bx.balanced()
    apply_x(bx, scs); by = apply_y(by, hy, scs)
    assert ppw(hx) < 2 and not bx.balanced() and not by.balanced() and bx.chunk_points() == by.chunk_points()
    for i, (x, y) in enumerate(zip(hx, hy)):
        assert_same_window(x, y, f"window {i}")
    assert_same_optimize(bx, hx, by, hy, "mode change")
    close_all(bx, by, hx, hy)


def test_a_window_that_sits_out_keeps_its_bytes_and_its_applied_state():
    sts, scs, hx, bx, hy, by = run_pair(3, 600)
    was = window_bytes(hx[1])
    prior_was = hx[1].get_prior()
    apply_x(bx, scs, sit_out=(1,)); by = apply_y(by, hy, scs, sit_out=(1,))
    now = window_bytes(hx[1])
    for k in was:
        if k != "cuts":          # it is re-cut with the others: the cost of sitting out
            same(now[k], was[k], "the window that sat out: " + k)
    same(hx[1].get_prior()[0], prior_was[0], "the window that sat out: prior")
    same(hx[1].get_chunk_cuts(), hy[1].get_chunk_cuts(), "the window that sat out: cuts")
    for i in (0, 2):
        assert_same_window(hx[i], hy[i], f"window {i}")
        same(hx[i].get_residuals()["state_state"], scs[i]["w1"].residuals["state_state"], f"window {i}: state_state against the host objects")
    assert len({(h.F, h.P, h.R) for h in hx}) == 3
    assert_same_optimize(bx, hx, by, hy, "sit-out")          # window 1 still holds an applied state: it runs like its twin that was only re-batched
    close_all(bx, by, hx, hy)


def test_second_round_on_the_same_batch():
    """the key-frame loop: update -> set_frames -> optimize -> marginalize_points -> update again, the batch never destroyed"""
    sts, scs, hx, bx, hy, by = run_pair(6, 1400)
    apply_x(bx, scs); by = apply_y(by, hy, scs)
    assert bx.balanced()
    bx.optimize(3, force_all=True); by.optimize(3, force_all=True)
    flags = [(np.arange(h.P) % 7 == 0).astype(np.int32) for h in hx]
    mx, my = bx.marginalize_points(flags), by.marginalize_points(flags)
    for a, b in zip(mx, my):
        assert rel(a[0], b[0]) < 1e-5
    second = [bu.edit_again(sc, h, fl, i) for i, (sc, h, fl) in enumerate(zip(scs, hx, flags))]
    jobs = [s[0] for s in second]
    fr, cal, pri = [s[1] for s in second], [s[2] for s in second], [s[3] for s in second]
    bx.update_windows(jobs); bx.set_frames(fr, cal, pri)
    by.close()
    for h, j, f, c, p in zip(hy, jobs, fr, cal, pri):
        h.update_window(*j); h.set_frames(f, c); h.set_prior(*p)
    by = binding.BABatch(hy)
    assert bx.balanced() == by.balanced() and bx.chunk_points() == by.chunk_points()
    for i, (x, y) in enumerate(zip(hx, hy)):
        assert x.P < scs[i]["w1"].P
        assert_same_window(x, y, f"second round, window {i}")
        same(x.get_prior()[0], y.get_prior()[0], f"second round, window {i}: prior")
    assert_same_optimize(bx, hx, by, hy, "second round")
    close_all(bx, by, hx, hy)


def test_refusal_is_all_or_nothing():
    sts, scs, hx, bx, hy, by = run_pair(3, 600)
    was = [window_bytes(h) for h in hx]
    good = scs[2]["job"]

    def bad(i, v):
        a = list(good); a[i] = v
        with pytest.raises(binding.LdsoError):
            bx.update_windows([scs[0]["job"], scs[1]["job"], tuple(a)])

    # the bad deltas of tests/test_resident_gpu.py::test_update_window_rejects_bad_deltas, in window 2 only
    ff = good[1].copy(); ff[0], ff[1] = ff[1], ff[0]; bad(1, ff)                                                     # surviving frames out of order
    pf = good[2].copy(); keep = np.nonzero(pf >= 0)[0]; pf[keep[0]], pf[keep[1]] = pf[keep[1]], pf[keep[0]]; bad(2, pf)      # surviving points out of order
    mk = good[3].copy(); mk[0] |= np.uint32(1 << 20); bad(3, mk)                                                     # a residual to a frame outside the window
    bad(5, good[5][:-1])                                                                                              # a fresh residual short
    with pytest.raises(binding.LdsoError):
        bx.update_windows([None, None, None])                                                                        # nobody takes part
    for i, h in enumerate(hx):
        now = window_bytes(h)
        for k in was[i]:
            same(now[k], was[i][k], f"after the refusals, window {i}: {k}")
    assert_same_optimize(bx, hx, by, hy, "after the refusals")          # the batch still runs, like its untouched twin
    close_all(bx, by, hx, hy)


def test_a_ninth_frame_is_refused_in_a_batch_of_eight_slot_tables():
    st = stream()
    sts = [bu.start("grow-to-9", 600, 21 + i) for i in range(2)]
    hs = [bu.load(s, st) for s in sts]
    bt = binding.BABatch(hs)
    bt.optimize(3, force_all=True)
    scs = [bu.edit(s, h) for s, h in zip(sts, hs)]
    assert scs[0]["w1"].F == 9
    was = [window_bytes(h) for h in hs]
    with pytest.raises(binding.LdsoError, match="slot-table width"):
        bt.update_windows([sc["job"] for sc in scs])
    for i, h in enumerate(hs):
        now = window_bytes(h)
        for k in was[i]:
            same(now[k], was[i][k], f"after the refusal, window {i}: {k}")
    hs[0].update_window(*scs[0]["job"])          # the same delta is a valid one for the handle alone
    assert hs[0].F == 9
    close_all(bt, hs)


def test_set_frames_alone():
    """batch.set_frames on a batch at rest: a prior for window 0, none for window 2, window 1 sits out"""
    sts, scs, hx, bx, hy, by = run_pair(3, 600)
    fr = [h.get_frames() for h in hx]
    frames = [f["frames"].copy() for f in fr]
    calibs = []
    for s, f in zip(sts, fr):
        c = s["w0"].calib.copy(); c["value"] = f["calib_value"]; calibs.append(c)
    for f in frames:
        f["state"][:, :6] *= 0.5          # not the state the handles hold: the adjoints and the precalc values move
    g = np.random.default_rng(7)
    n = 8 * hx[0].F + 4
    M = g.standard_normal((n, n)) * 1e-2
    HM, bM = M @ M.T, g.standard_normal(n) * 1e-2
    was_f, was_p = hx[1].get_frames(), hx[1].get_prior()
    bx.set_frames([frames[0], None, frames[2]], calibs, [(HM, bM), None, None])
    hy[0].set_frames(frames[0], calibs[0]); hy[0].set_prior(HM, bM)
    hy[2].set_frames(frames[2], calibs[2]); hy[2].set_prior(None, None)
    for i in (0, 2):
        fx, fy = hx[i].get_frames(), hy[i].get_frames()
        for k in fx:
            same(fx[k], fy[k], f"window {i}: frames.{k}")
        px, py = hx[i].get_prior(), hy[i].get_prior()
        same(px[0], py[0], f"window {i}: HM"); same(px[1], py[1], f"window {i}: bM")
        assert px[2] == py[2] == (i == 0)
        same(hx[i].get_precalc(), hy[i].get_precalc(), f"window {i}: precalc")
    same(hx[0].get_prior()[0], HM, "window 0: HM as given"); assert not hx[2].get_prior()[0].any()
    now_f, now_p = hx[1].get_frames(), hx[1].get_prior()
    for k in was_f:
        same(now_f[k], was_f[k], "the window that sat out: frames." + k)
    same(now_p[0], was_p[0], "the window that sat out: HM"); assert now_p[2] == was_p[2]
    close_all(bx, by, hx, hy)
