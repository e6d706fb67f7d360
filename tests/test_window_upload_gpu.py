"""The three routes of a window onto a handle (ldso_ba_set_window, ldso_ba_update_window, ldso_ba_batch_update_windows) share one description of the window's image
(stage_image), one derivation of the dimensions (adopt_dims) and one way to grow a staging arena (grow_arena, csrc/hip_host.h).  What those shared pieces could break
and tests/test_resident_gpu.py / test_batch_update_window_gpu.py do not reach: a handle after a REFUSED upload, the handle's arena growing and being reused across
windows of different sizes and kinds, the batch's arena growing between two key-frame steps of one batch.

"The same bytes" throughout: get_points, get_residuals, get_frames and, after one stage-wise pass (collect_active, linearize_all(False), apply_res, backup_state,
solve_system(0)), get_residuals, get_points and get_system once more, compared with tobytes() (test_resident_gpu._same).  The pass writes to the handle, so the bytes
of a reference handle are taken once and kept."""
import copy

import numpy as np
import pytest

from ldso_amd import synth, binding
from oracle import pyoracle as po
from test_resident_gpu import _scenario, _same, _sub, _load_fresh
import batch_update_common as bu

pytestmark = pytest.mark.gpu


def _as_loaded(h):
    """what the getters say about the window before anything runs (reads only)"""
    out = {"dims": np.array([h.F, h.P, h.R])}
    r, p, f = h.get_residuals(), h.get_points(), h.get_frames()
    for k in ("state_state", "is_active", "to_remove"):
        out["loaded res." + k] = r[k]
    for k in r["out"].dtype.names:
        out["loaded res.out." + k] = r["out"][k]
    for k in p.dtype.names:
        out["loaded point." + k] = p[k]
    for k, v in f.items():
        out["loaded frames." + k] = v
    return out


def _bytes(h):
    """the same bytes (module docstring); leaves the handle with an applied linearisation"""
    out = _as_loaded(h)
    h.collect_active()
    out["energy"] = np.array([h.linearize_all(False)])
    assert np.isfinite(out["energy"][0])
    h.apply_res(); h.backup_state(); h.solve_system(0)
    r, p, s = h.get_residuals(), h.get_points(), h.get_system()
    for k in r["out"].dtype.names:
        out["res.out." + k] = r["out"][k]
    for k in p.dtype.names:
        out["point." + k] = p[k]
    for k, v in s.items():
        out["system." + k] = v
    return out


def _assert_same(got, want, tag):
    assert got.keys() == want.keys()
    for k in want:
        _same(got[k], want[k], f"{tag}: {k}")


def _handle(win, max_frames, max_points):
    h = binding.BA(win.w, win.h, max_frames=max_frames, max_points=max_points)
    h.set_settings(win.settings)
    return h


def _upload(h, win, prior_first=None):
    """the calls of BA.load_window; prior_first = (HM, bM): a ldso_ba_set_prior on the RESIDENT window directly in front of the ldso_ba_set_window, nothing in between
    that waits for the stream - its copy out of the staging arena may still be in flight when the upload wants the arena (stageBusy)"""
    for f in range(win.F):
        h.set_image(f, win.images[f][0])
    if prior_first is not None:
        h.set_prior(*prior_first)
    h.set_window(np.arange(win.F), win.points, win.residuals, win.lin_J, win.lin_res_toZeroF)
    h.set_frames(win.frames, win.calib)
    if np.any(win.HM) or np.any(win.bM):
        h.set_prior(win.HM, win.bM)


def test_refused_set_window_then_reuse():
    """ldso_ba_set_window adopts the new dimensions before it has looked at the records: a refusal leaves the handle WITHOUT a window (WinGuard), whatever it had
    adopted and staged by then, and the next valid upload is the one a fresh handle gets."""
    win = synth.make_config("small", F=5, P=200)
    F, P = win.F, win.P
    fresh = _handle(win, F + 1, P)
    _upload(fresh, win)
    want = _bytes(fresh)
    fresh.close()
    h = _handle(win, F + 1, P)          # slot F never receives an image
    _upload(h, win)
    slots = np.arange(F)
    to_host = win.residuals.copy(); to_host["target"][3] = to_host["host"][3]
    bad_host = win.points.copy(); bad_host["host"][P // 2] = F
    no_image = slots.copy(); no_image[-1] = F
    mask = np.zeros(P, np.uint32)
    np.bitwise_or.at(mask, win.residuals["point"], (1 << win.residuals["target"]).astype(np.uint32))
    for name, args in (("a residual whose target is its host", (slots, win.points, to_host)), ("a point host out of range", (slots, bad_host, win.residuals)),
                       ("an image slot that was never set", (no_image, win.points, win.residuals))):
        h.optimize(2, force_all=True)          # a resident, optimised window
        with pytest.raises(binding.LdsoError):
            h.set_window(*args)
        with pytest.raises(binding.LdsoError, match="no window"):
            h.linearize_all(False)
        with pytest.raises(binding.LdsoError, match="no resident window"):
            h.update_window(slots, slots, np.arange(P), mask)
        h.set_window(slots, win.points, win.residuals)
        h.set_frames(win.frames, win.calib)
        _assert_same(_bytes(h), want, "after " + name)
    h.close()


def test_refused_update_window_leaves_the_resident_window():
    """A delta that fails its validation is refused before anything is written.  The before / after comparison uses the getters alone (the stage-wise pass would itself
    change the window); the valid delta that follows gives the bytes of the fresh upload, the pass included."""
    sc = _scenario(7, [0, 1, 2, 3, 4, 5], [1, 2, 3, 4, 5, 6], P=300)
    A, w1 = sc["A"], sc["w1"]
    args = [sc["new_frames"], sc["frame_from"], sc["point_from"], sc["res_mask"], sc["fresh_pts"], sc["fresh_res"], sc["mrb"][sc["fresh_rows"]], sc["ngr"][sc["fresh_rows"]]]
    was = _as_loaded(A)
    bad = list(args); bad[3] = sc["res_mask"].copy(); bad[3][0] |= np.uint32(1 << 20)          # a residual to a frame outside the window
    with pytest.raises(binding.LdsoError):
        A.update_window(*bad)
    _assert_same(_as_loaded(A), was, "after the refusal")
    A.update_window(*args)
    A.set_frames(w1.frames, w1.calib); A.set_prior(w1.HM, w1.bM)
    Bh = _load_fresh(sc)
    _assert_same(_bytes(A), _bytes(Bh), "the valid delta against the fresh upload")
    A.close(); Bh.close()


def test_handle_arena_grows_and_is_reused():
    """One handle made for 9 frames x 300 points takes four windows in turn; after each it holds the bytes of a fresh handle that only ever saw that window.
      3 x 37    the first arena; an odd P, so every part of the image ends off a 16-byte boundary and needs its padding
      9 x 300   two slot groups (FS = 16) and eight times the points: the arena of the first window (its need + a quarter) is too small and is replaced
      3 x 37    again, directly behind a ldso_ba_set_prior whose copy out of the arena nobody has waited for: the upload waits before it reuses the (large) arena
      9 x 300   with 20 .. 50 % of the residuals linearised (tests/test_ba_gpu.py::test_stagewise_mixed_linearized): the Jlin / res_toZeroF parts behind the image"""
    little, big = synth.make_config("small", F=3, P=37), synth.make_config("small", F=9, P=300)
    mixed = po.make_mixed_window(big)
    assert 0 < mixed.residuals["is_linearized"].sum() < mixed.R
    want = {}
    for name, win in (("little", little), ("big", big), ("mixed", mixed)):
        g = _handle(win, 9, 300)
        _upload(g, win)
        want[name] = _bytes(g)
        g.close()
    n = 8 * big.F + 4
    rng = np.random.default_rng(9)
    M = rng.standard_normal((n, n))
    h = _handle(big, 9, 300)
    _upload(h, little)
    _assert_same(_bytes(h), want["little"], "3 x 37 into a new arena")
    _upload(h, big)
    _assert_same(_bytes(h), want["big"], "9 x 300, the arena grows")
    _upload(h, little, prior_first=(M @ M.T, rng.standard_normal(n)))
    _assert_same(_bytes(h), want["little"], "3 x 37 behind a set_prior in flight")
    _upload(h, mixed)
    _assert_same(_bytes(h), want["mixed"], "9 x 300 with linearised residuals")
    assert h.get_counts()[1] > 0
    h.close()


def _sparse_start(kind, P, seed, share):
    """batch_update_common.start with a chosen share of the scene's points in the old window: the edit then brings more fresh points than the window had"""
    F_big, old_frames, new_frames = bu.KINDS[kind]
    rng = np.random.default_rng(seed)
    big = bu.scene(F_big, P)
    old_pts = np.nonzero(np.isin(big.points["host"], old_frames) & (rng.random(big.P) < share))[0]
    w0, _, _ = _sub(big, old_frames, old_pts)
    synth.add_synthetic_prior(w0, seed=3)
    return dict(kind=kind, seed=seed, big=big, old_frames=old_frames, new_frames=new_frames, old_pts=old_pts, w0=w0)


def test_batch_arena_grows_between_key_frame_steps():
    """One batch of two windows of about 100 points runs ldso_ba_batch_marginalize_points (the arena's first size: two window records, 800 bytes of flags, two priors of
    52 x 52 doubles - some 45 KB, half as much again allocated), then ldso_ba_batch_update_windows to about 300 points (two images of 300 x 8 slot records of 64 bytes and
    as many table entries: over 400 KB, the arena is replaced), then ldso_ba_batch_activate_points in the arena as grown.  Every result against the single-window entry
    on a twin handle that went through the same steps, as tests/test_batch_marginalize_gpu.py (1e-9 between a batched and a solo prior), test_batch_update_window_gpu.py
    (the same bytes) and test_batch_activate_gpu.py (the same bytes) compare them."""
    import batch_activate_common as bac
    from test_batch_marginalize_gpu import same_prior
    from test_batch_update_window_gpu import stream, apply_x, apply_y, assert_same_window, close_all
    st = stream()
    sp = [("points-only", 400, 61, 0.3), ("steady", 400, 62, 0.3)]
    sts = [_sparse_start(*s) for s in sp]
    hx = [bu.load(s, st) for s in sts]; bx = binding.BABatch(hx); bx.optimize(3, force_all=True)
    hy = [bu.load(s, st) for s in sts]; by = binding.BABatch(hy); by.optimize(3, force_all=True)
    assert all(80 <= h.P <= 130 for h in hx)
    flags = [(np.arange(h.P) % 7 == 0).astype(np.int32) for h in hx]
    mx = bx.marginalize_points(flags)
    for i, h in enumerate(hy):
        same_prior("window_upload_batch_marg_w%d" % i, mx[i], h.marginalize_points(flags[i]))
    scs = [bu.edit(s, h) for s, h in zip(sts, hx)]
    apply_x(bx, scs); by = apply_y(by, hy, scs)
    for i, (x, y, sc) in enumerate(zip(hx, hy, scs)):
        assert x.P >= 2.4 * len(sts[i]["old_pts"]) and 240 <= x.P <= 360, (x.P, len(sts[i]["old_pts"]))
        assert (x.F, x.P, x.R) == (sc["w1"].F, sc["w1"].P, sc["w1"].R)
        assert_same_window(x, y, f"window {i}")
        _same(x.get_residuals()["state_state"], sc["w1"].residuals["state_state"], f"window {i}: state_state against the host objects")
    cands = []
    for i, (s, sc) in enumerate(zip(sts, scs)):          # candidates traced in the new window: it is cut from the scene, whose true poses it takes along
        tr, nf = s["big"].truth, s["new_frames"]
        w1 = copy.copy(sc["w1"]); w1.truth = dict(w2c=tr["w2c"][nf], aff_a=np.asarray(tr["aff_a"])[nf], aff_b=np.asarray(tr["aff_b"])[nf], depths=None)
        cands.append(np.ascontiguousarray(bac.make_job(w1, 30, seed=70 + i)["cand"]))
    out = bx.activate_points(cands)
    for i, (y, c) in enumerate(zip(hy, cands)):
        want = y.activate_points(c)
        assert len(c) > 100 and out[i].tobytes() == want.tobytes(), (i, int((out[i]["ok"] != want["ok"]).sum()))
        assert 0 < want["ok"].sum()
    close_all(bx, by, hx, hy)
