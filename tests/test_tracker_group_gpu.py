"""ldso_tr_group_track / ldso_tr_group_track_new_coarse: the tracks of several trackers in one launch (k_tr_track_group).  A member's result is its own
ldso_tr_track / ldso_tr_track_new_coarse from the same inputs, byte for byte: the grouped kernel runs the same body, every job with its own parameters, record and
hand-over slot.  Three scenes (tracker_common.tracker_scenario; reference points per level checked on the CPU oracle):
  "tiny"   160 x 128, pc_n 313 / 304 / 265: every level below TR_COOP_MIN = 512, the leader works alone, the result does not depend on G
  "tinyP"  the same with P = 700, 3032 / 2098 / 843: level 2 engages ceil(843 / 64) = 14 of a job's 16 workgroups
  "small"  320 x 240, 1970 / 1842 / 1550: every level shared by all G
A solo track runs G = 16; three jobs do where 3 * 16 <= CUs.  Where the getter says otherwise, the members whose sums depend on G are compared against hypothesis 0
of Tracker.track_batch with as many copies of the guess as the group has jobs (the same launch-shape rule, hence the same G).  All tests run on one torch stream."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import rel
from tracker_common import tracker_scenario
from ldso_amd import synth, binding
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu
LDSO_E_INVALID = -1
KEYS = ("tiny", "tinyP", "small")
G_FREE = ("tiny",)          # scenes whose result does not depend on the cooperation width


@functools.lru_cache(maxsize=None)
def scene(key, seed=20260925):
    return tracker_scenario("tiny", P=700, seed=seed) if key == "tinyP" else tracker_scenario(key, seed=seed)


def stream():
    import torch
    ts = torch.cuda.Stream(); torch.cuda.set_stream(ts)
    return ts.cuda_stream


def make_tracker(sc, st, pts=None):
    win = sc["win"]
    g = binding.Tracker(win.w, win.h, sc["levels"], win.settings, win.calib)
    if st is not None:
        g.set_stream(st)
    g.set_ref(sc["ref_pyr"], sc["ref_aff"][0], sc["ref_aff"][1], 1.0, sc["pts"] if pts is None else pts)
    g.set_new_frame(sc["new_pyr"], 1.0)
    return g


def make_oracle(sc):
    win = sc["win"]
    o = po.OracleTracker(win.w, win.h, sc["levels"], win.settings, win.calib)
    o.set_ref(sc["ref_pyr"], sc["ref_aff"][0], sc["ref_aff"][1], 1.0, sc["pts"])
    o.set_new_frame(sc["new_pyr"], 1.0)
    return o


@functools.lru_cache(maxsize=None)
def oracle_for(key):
    return make_oracle(scene(key))


PERTURBED = synth.se3_exp([0.01, 0, 0, 0, 0.002, 0])


def guess_of(key):
    """test 1: identity for the member that is also held against the oracle (as test_track_matches_oracle does), the true motion, a perturbed guess"""
    return {"small": np.eye(4), "tinyP": scene("tinyP")["T_true"], "tiny": PERTURBED}[key]


def solo_reference(trk, key, T, a, b, coarsest, n_jobs, width, min_res=None):
    """what the member alone gives under the cooperation width the group launch runs with"""
    if width == 16 or key in G_FREE:
        return trk.track(T, a, b, coarsest, min_res)
    r = trk.track_batch([T] * n_jobs, [(a, b)] * n_jobs, coarsest, min_res)
    return {k: v[0] for k, v in r.items()}


def assert_same_track(rg, rs, tag):
    assert np.array_equal(rg["T"], rs["T"]), tag
    assert np.float32(rg["a"]) == np.float32(rs["a"]) and np.float32(rg["b"]) == np.float32(rs["b"]), tag
    assert np.array_equal(rg["lastResiduals"], rs["lastResiduals"], equal_nan=True), tag
    assert np.array_equal(rg["flow"], rs["flow"], equal_nan=True), tag
    assert bool(rg["ok"]) == bool(rs["ok"]) and int(rg["iterations"]) == int(rs["iterations"]), tag


def mixed_group(st):
    """the three scenes as one group, with what test 1 feeds them"""
    scs = [scene(k) for k in KEYS]
    trk = [make_tracker(sc, st) for sc in scs]
    Ts = [guess_of(k) for k in KEYS]
    affs = [sc["new_aff"] for sc in scs]
    coarsest = [sc["levels"] - 1 for sc in scs]
    return scs, trk, Ts, affs, coarsest


def test_mixed_group_equals_solo_tracks_and_the_oracle():
    st = stream()
    scs, trk, Ts, affs, coarsest = mixed_group(st)
    grp = binding.TrackerGroup(trk)
    try:
        W = grp.coop_width(3)
        solo = [solo_reference(trk[i], KEYS[i], Ts[i], affs[i][0], affs[i][1], coarsest[i], 3, W) for i in range(3)]
        out = grp.track(Ts, affs, coarsest)
        for i in range(3):
            assert out[i]["ok"], KEYS[i]
            assert_same_track(out[i], solo[i], KEYS[i])
        # the bounds of test_track_matches_oracle on the "small" member
        i = KEYS.index("small")
        sc, rg = scs[i], out[i]
        ro = oracle_for("small").track(Ts[i], affs[i][0], affs[i][1], coarsest[i])
        assert ro["ok"]
        To, Tg = np.eye(4), np.eye(4)
        To[:3, :4] = ro["T"]; Tg[:3, :4] = rg["T"]
        d = np.linalg.norm(synth.se3_log(Tg @ np.linalg.inv(To)))
        m = np.linalg.norm(synth.se3_log(To))
        print("small member vs oracle: d / m =", d / m, "iterations", rg["iterations"], ro["iterations"])
        assert d < 1e-4 * m + 1e-6
        assert abs(rg["iterations"] - ro["iterations"]) <= 1
        assert rel(rg["lastResiduals"][:sc["levels"]], ro["lastResiduals"][:sc["levels"]]) < 1e-4
        err = np.linalg.norm(synth.se3_log(Tg @ np.linalg.inv(sc["T_true"])))
        assert err < 0.25 * np.linalg.norm(synth.se3_log(sc["T_true"]))
    finally:
        grp.close()


def test_another_width_equals_track_batch_and_agrees_with_solo_and_oracle():
    """n members (17 on a 256-CU card) so that the launch-shape rule leaves G = 16: member i = hypothesis 0 of track_batch on its own handle with n copies of its
    guess, byte for byte; its G = 16 solo track and the oracle within the 1e-4 of test_cooperative_group_sizes_agree; the "tiny" members' solo track byte for byte."""
    st = stream()
    probe = make_tracker(scene("tiny"), st)
    pg = binding.TrackerGroup([probe])
    n = next((k for k in range(1, 129) if pg.coop_width(k) != 16), None)
    pg.close()
    if n is None:
        pytest.skip("every job count up to 128 runs G = 16 on this device: no other width to reach")
    keys = [KEYS[i % 3] for i in range(n)]
    scs = [scene(k) for k in keys]
    trk = [probe] + [make_tracker(scs[i], st) for i in range(1, n)]
    rng = np.random.default_rng(n)
    # drawn as in test_cooperative_group_sizes_agree (640 x 480), scaled to the same displacement in pixels on the smaller scenes
    Ts = [synth.se3_exp(np.concatenate([rng.normal(0, 2e-3, 3), rng.normal(0, 5e-4, 3)]) * (640.0 / sc["win"].w)) for sc in scs]
    affs = [sc["new_aff"] for sc in scs]
    coarsest = [sc["levels"] - 1 for sc in scs]
    grp = binding.TrackerGroup(trk)
    try:
        W = grp.coop_width(n)
        assert W != 16
        out = grp.track(Ts, affs, coarsest)
        for i in range(n):
            tag = (i, keys[i], W)
            a, b = affs[i]
            rb = trk[i].track_batch([Ts[i]] * n, [(a, b)] * n, coarsest[i])
            assert_same_track(out[i], {k: v[0] for k, v in rb.items()}, tag)
            single = trk[i].track(Ts[i], a, b, coarsest[i])                      # G = 16
            ro = oracle_for(keys[i]).track(Ts[i], a, b, coarsest[i])
            assert out[i]["ok"] and single["ok"] and ro["ok"], tag
            print(tag, "vs solo", np.abs(out[i]["T"] - single["T"]).max(), "vs oracle", np.abs(out[i]["T"] - ro["T"]).max(), "iterations", out[i]["iterations"], ro["iterations"])
            assert np.abs(out[i]["T"] - single["T"]).max() < 1e-4, tag
            assert np.abs(out[i]["T"] - ro["T"]).max() < 1e-4, tag
            assert abs(out[i]["iterations"] - ro["iterations"]) <= 2, tag
            if keys[i] in G_FREE:
                assert_same_track(out[i], single, tag)
    finally:
        grp.close()


def test_per_member_arguments():
    """one member aborts on its minRes while its neighbours finish; coarsestLvl differs between members; a reference of two points and one of a single point behave
    as in test_lm_solve_unpivoted_in_registers_and_pivoted_when_rank_deficient: ok, iterations and the count of pivoted solves of the solo track"""
    st = stream()
    small, tiny, tinyP = scene("small"), scene("tiny"), scene("tinyP")
    pts = np.array(small["pts"], np.float32)
    few = [pts[np.linspace(0, len(pts) - 1, k).astype(int)] for k in (2, 1)]
    keys = ["small", "tiny", "tinyP", "small", "small"]
    scs = [small, tiny, tinyP, small, small]
    trk = [make_tracker(small, st), make_tracker(tiny, st), make_tracker(tinyP, st), make_tracker(small, st, few[0]), make_tracker(small, st, few[1])]
    n = len(trk)
    Ts = [np.eye(4)] * n
    affs = [sc["new_aff"] for sc in scs]
    coarsest = [small["levels"] - 1, tiny["levels"] - 2, tinyP["levels"] - 1, small["levels"] - 1, small["levels"] - 1]
    min_res = np.full((n, 5), np.nan)
    min_res[0] = 1e-3
    grp = binding.TrackerGroup(trk)
    try:
        W = grp.coop_width(n)
        solo, piv, evals = [], [], []
        for i in range(n):
            solo.append(solo_reference(trk[i], keys[i], Ts[i], affs[i][0], affs[i][1], coarsest[i], n, W, min_res[i]))
            piv.append(trk[i].last_track_pivoted_solves()); evals.append(trk[i].last_track_evals()[0].copy())
        out = grp.track(Ts, affs, coarsest, min_res)
        assert not out[0]["ok"] and out[1]["ok"] and out[2]["ok"]
        for i in range(3):
            assert_same_track(out[i], solo[i], i)
        assert np.isnan(out[1]["lastResiduals"][coarsest[1] + 1])          # the level above its coarsestLvl was never visited
        assert not np.isnan(out[2]["lastResiduals"][coarsest[2]])
        for i in (3, 4):
            assert bool(out[i]["ok"]) == bool(solo[i]["ok"]) and out[i]["iterations"] == solo[i]["iterations"], i
        for i in range(n):
            if W == 16 or keys[i] in G_FREE:
                assert trk[i].last_track_pivoted_solves() == piv[i], i
                assert np.array_equal(trk[i].last_track_evals()[0], evals[i]), i
            else:                # the solo reference was a batch of n copies: its count of pivoted solves sums over all of them
                assert trk[i].last_track_pivoted_solves() * n == piv[i], i
    finally:
        grp.close()


def raw_track(grp, active, Ts, affs, coarsest, sentinel):
    """ldso_tr_group_track itself, on arrays whose rows hold `sentinel` wherever the library has not written"""
    n = len(grp.trackers)
    T = np.full((n, 3, 4), float(sentinel)); ab = np.full((n, 2), sentinel, np.float32)
    for i in range(n):
        if active[i]:
            T[i] = np.asarray(Ts[i], np.float64)[:3, :4]; ab[i] = affs[i]
    co = np.ascontiguousarray(coarsest, np.int32)
    lr = np.full((n, 5), float(sentinel)); fl = np.full((n, 3), float(sentinel)); ok = np.full(n, sentinel, np.int32); it = np.full(n, sentinel, np.int32)
    act = np.ascontiguousarray(active, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = grp.L.ldso_tr_group_track(grp.h, p(act), p(T), p(ab), p(co), None, p(lr), p(fl), p(ok), p(it))
    assert rc == 0, grp.L.ldso_last_error()
    return dict(T=T, ab=ab, lastResiduals=lr, flow=fl, ok=ok, iterations=it)


def test_active_members_only_and_a_member_with_new_frames():
    st = stream()
    scs, trk, Ts, affs, coarsest = mixed_group(st)
    grp = binding.TrackerGroup(trk)
    try:
        full = grp.track(Ts, affs, coarsest)
        active = [1, 0, 1]
        W = grp.coop_width(2)
        r = raw_track(grp, active, Ts, affs, coarsest, -7)
        for i in range(3):
            if not active[i]:
                assert (r["T"][i] == -7).all() and (r["ab"][i] == -7).all() and (r["lastResiduals"][i] == -7).all() and (r["flow"][i] == -7).all()
                assert r["ok"][i] == -7 and r["iterations"][i] == -7
                continue
            got = dict(T=r["T"][i], a=r["ab"][i, 0], b=r["ab"][i, 1], lastResiduals=r["lastResiduals"][i], flow=r["flow"][i], ok=r["ok"][i], iterations=r["iterations"][i])
            if W == grp.coop_width(3) or KEYS[i] in G_FREE:
                assert_same_track(got, full[i], KEYS[i])          # = test 1
            assert_same_track(got, solo_reference(trk[i], KEYS[i], Ts[i], affs[i][0], affs[i][1], coarsest[i], 2, W), KEYS[i])
        assert grp.track(Ts, affs, coarsest, active=active)[1] is None
        # member 0 gets another reference and another new frame between two group calls
        i = KEYS.index("tiny")
        other = scene("tiny", seed=7)
        trk[i].set_ref(other["ref_pyr"], other["ref_aff"][0], other["ref_aff"][1], 1.0, other["pts"])
        trk[i].set_new_frame(other["new_pyr"], 1.0)
        affs2 = list(affs); affs2[i] = other["new_aff"]
        again = grp.track(Ts, affs2, coarsest)
        assert_same_track(again[i], trk[i].track(Ts[i], affs2[i][0], affs2[i][1], coarsest[i]), "re-referenced")
        assert not np.array_equal(again[i]["T"], full[i]["T"])
        for k in range(3):
            if k != i:
                assert_same_track(again[k], full[k], KEYS[k])
    finally:
        grp.close()


def new_coarse_inputs(sc, lost):
    """the set-ups of test_track_new_coarse_matches_oracle"""
    w = sc["win"]; F = w.F
    w2c = w.truth["w2c"]
    lastF, slast, sprelast = w2c[F - 1], w2c[F - 1], w2c[F - 2]
    if lost:
        ang = 0.06
        Rz = np.array([[np.cos(ang), -np.sin(ang), 0, 0], [np.sin(ang), np.cos(ang), 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
        sprelast = Rz @ slast
    return sprelast, slast, lastF, (np.array([0.05] * 5) if lost else np.array([100.0] * 5))


def assert_same_new_coarse(a, b, tag):
    for k in ("result", "w2c", "aff", "lastCoarseRMSE"):
        assert np.array_equal(a[k], b[k], equal_nan=True), (tag, k)
    assert a["tries"] == b["tries"] and a["good"] == b["good"], tag


def test_track_new_coarse_equals_solo_and_the_oracle():
    """three members, the "small" one lost (83 tries: the second launch), two not (one try each); every output = the member's own ldso_tr_track_new_coarse, and the
    oracle's within the bounds of test_track_new_coarse_matches_oracle.  Then a member whose poses are not valid: the identity alone, one try."""
    st = stream()
    scs = [scene(k) for k in KEYS]
    trk = [make_tracker(sc, st) for sc in scs]
    lost = [k == "small" for k in KEYS]
    ins = [new_coarse_inputs(sc, l) for sc, l in zip(scs, lost)]
    affs = [sc["new_aff"] for sc in scs]
    grp = binding.TrackerGroup(trk)
    try:
        W = grp.coop_width(3)
        solo = [trk[i].track_new_coarse(ins[i][0], ins[i][1], ins[i][2], affs[i], ins[i][3]) for i in range(3)]
        out = grp.track_new_coarse([x[0] for x in ins], [x[1] for x in ins], [x[2] for x in ins], affs, [x[3] for x in ins])
        for i in range(3):
            tag = KEYS[i]
            b = out[i]
            assert b["good"] == 1 and b["tries"] == (83 if lost[i] else 1), tag
            if W == 16 or KEYS[i] in G_FREE:          # try 0 of the solo call runs G = 16
                assert_same_new_coarse(b, solo[i], tag)
            a = oracle_for(KEYS[i]).track_new_coarse(ins[i][0], ins[i][1], ins[i][2], affs[i], ins[i][3])
            for b_ in (b, solo[i]):
                assert a["good"] == b_["good"] and a["tries"] == b_["tries"], tag
                assert np.abs(a["w2c"] - b_["w2c"]).max() < 1e-4, tag
                assert np.abs(a["aff"] - b_["aff"]).max() < 1e-3 * max(1.0, np.abs(a["aff"]).max()), tag
                fin = np.isfinite(a["lastCoarseRMSE"])
                assert np.array_equal(fin, np.isfinite(b_["lastCoarseRMSE"])), tag
                assert np.abs(a["lastCoarseRMSE"][fin] - b_["lastCoarseRMSE"][fin]).max() <= 1e-3 * np.abs(a["lastCoarseRMSE"][fin]).max(), tag
                assert np.abs(a["result"] - b_["result"]).max() <= 1e-3 * max(1.0, np.abs(a["result"]).max()), tag
        i = KEYS.index("tiny")
        s1 = trk[i].track_new_coarse(ins[i][0], ins[i][1], ins[i][2], affs[i], ins[i][3], poses_valid=False)
        pv = [True] * 3; pv[i] = False
        g1 = grp.track_new_coarse([x[0] for x in ins], [x[1] for x in ins], [x[2] for x in ins], affs, [x[3] for x in ins], poses_valid=pv, active=[k == i for k in range(3)])
        assert g1[i]["tries"] == 1 and [k for k in range(3) if g1[k] is not None] == [i]
        assert_same_new_coarse(g1[i], s1, "poses not valid")
    finally:
        grp.close()


def test_refusals_leave_group_and_members_usable():
    st = stream()
    scs, trk, Ts, affs, coarsest = mixed_group(st)
    grp = binding.TrackerGroup(trk)
    try:
        first = grp.track(Ts, affs, coarsest)

        def still_works():
            again = grp.track(Ts, affs, coarsest)
            for i in range(3):
                assert_same_track(again[i], first[i], KEYS[i])

        loner = make_tracker(scene("tiny"), None)                 # on its own stream
        free = make_tracker(scene("tiny"), st)
        for bad in ([free, loner], [free, free], [free, trk[0]]):
            with pytest.raises(binding.LdsoError) as e:
                binding.TrackerGroup(bad)
            assert e.value.code == LDSO_E_INVALID and "ldso_tr_group_create" in str(e.value)
            still_works()
        binding.TrackerGroup([free]).close()                      # none of the refusals has claimed it
        # a member moved to another stream after the group was made
        trk[1].set_stream(None)
        with pytest.raises(binding.LdsoError) as e:
            grp.track(Ts, affs, coarsest)
        assert e.value.code == LDSO_E_INVALID
        trk[1].set_stream(st)
        still_works()
        bad_lvl = list(coarsest); bad_lvl[2] = scs[2]["levels"]
        with pytest.raises(binding.LdsoError) as e:
            grp.track(Ts, affs, bad_lvl)
        assert e.value.code == LDSO_E_INVALID and "coarsestLvl" in str(e.value)
        with pytest.raises(binding.LdsoError) as e:
            grp.track(Ts, affs, coarsest, active=[0, 0, 0])
        assert e.value.code == LDSO_E_INVALID
        still_works()
        with pytest.raises(binding.LdsoError) as e:
            trk[0].close()
        assert e.value.code == LDSO_E_INVALID and "ldso_tr_destroy" in str(e.value) and trk[0].h
        W = grp.coop_width(3)
        if W == 16 or KEYS[0] in G_FREE:
            assert_same_track(trk[0].track(Ts[0], affs[0][0], affs[0][1], coarsest[0]), first[0], "member after a refused destroy")
        still_works()
    finally:
        grp.close()
    trk[0].close()                                                # the group is gone: the member may go too
    assert not trk[0].h


def test_consecutive_group_calls_repeat_byte_for_byte():
    """the group's hand-over records and sequence counter carry over from launch to launch: three calls in a row, identical results"""
    st = stream()
    scs, trk, Ts, affs, coarsest = mixed_group(st)
    grp = binding.TrackerGroup(trk)
    try:
        runs = [grp.track(Ts, affs, coarsest) for _ in range(3)]
        for r in runs[1:]:
            for i in range(3):
                assert_same_track(r[i], runs[0][i], KEYS[i])
    finally:
        grp.close()
