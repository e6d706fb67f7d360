"""k_ini_eval (ldso_amd/csrc/initializer.hip) entry by entry against the float64 reference of tests/init_stage_common.py, whose own soundness is the subject of
tests/test_init_stage_cpu.py.  RUN THIS FILE AFTER EVERY CHANGE TO k_ini_eval.

The stage (ldso_init_calc_res_and_gs): 1 .. 16385 points on level 0 of a 192 x 144 two-level handle - one partial group, one block, the second trip of the
grid-stride loop from the 8193rd point on with a ragged last group (8193, 8225), a third trip (16385) - each at a large translation (alphaOpt = 0), a small one
(alphaOpt = 150^2) and t = 0, snapped and not; level 1 after level 0 on the same handle (stale partial rows); exactly one good point at every lane group of a
block and in the blocks of the second trip; NaN / +Inf pixels in either frame.  Asserted: isGood_new equal; carried energies byte-equal; maxstep exactly 1e10 where
no pattern pixel was visited and +inf at t = 0, the partial minimum of a point that is not good-new equal to the oracle's bit for bit; res[1], res[2],
ec[2] exact; every entry of H, b, Hsc, bsc, E, ec[0..1] and per point energy_new, lastHessian_new, maxstep and the ten Jb entries within max(4 * u_oracle, 16) * eps32 * S of the float64 value, u_oracle being the error of oracle/initializer.cc
on the same case and quantity in the same units.
doStep / applyStep / resetPoints' per-point part (ldso_init_debug_eval_step) at 8225 and 33 points: applyStep's copies and resetPoints' writes byte-equal,
idepth_new exactly at 1e-3 / 50 where the clamp acts, elsewhere within 8 * eps32 * (|idepth| + sum |terms of the step|); then the sums of the same launch as above.
The step's inputs (tiny and infinite maxstep, inverse depths next to both clamps) are set AFTER the evaluation that provides Jb: an evaluation rewrites maxstep.

Measured on an MI355X, the kernel's worst units over the 102 stage cases: H 233, b 61, Hsc 182, bsc 95, E 1.2, ec0 2.3, ec1 1.7, energy_new 3.6, lastHessian_new 0.19, maxstep 5.7, Jb 7.3
(the large ones on the cases where one point or 33 make the sum; the oracle shows the same there); on the random cases with n >= 8191: H 32, b 0.38, Hsc 81, bsc 19, E 0.09, ec0 0.71, ec1 0.92;
the sums behind a step: H 32, Hsc 20, others below 7.  Everywhere at most 0.36 of the bound.  idepth_new behind doStep: at most 1.5 units (bound 8)."""
import functools

import numpy as np
import pytest

import init_stage_common as common
from test_init_stage_cpu import INC, LAMBDA, STEP_MODES, step_inputs

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def device_handle(n0, nonfinite=False):
    from ldso_amd import binding
    seq, _, _ = common.sequence()
    first, new = (common.nonfinite_frames()[:2]) if nonfinite else (seq["first"], seq["frames"][1])
    g = binding.Initializer(common.W0, common.H0, common.LEVELS)
    g.set_first(seq["K4"], first, common.base_points(n0))
    g.set_new_frame(new, 1.0)
    return g


def _stage(name):
    c = common.case(name)
    u_oracle, got_oracle = common.oracle_units(name)
    got = common.run_impl(device_handle(c.n0, c.what == "nonfinite"), c)
    un = common.check_stage(got, c.ref, u_oracle, name)
    # the partial minimum of a point that is not good-new: the float64 value within the bound (above), and the float32 oracle's very bits (except at t = 0, where the
    # oracle keeps 1e10: tests/test_init_stage_cpu.py)
    part = ~c.ref.isGood_new & np.isfinite(c.ref.maxstep)
    assert np.array_equal(got["pts"]["maxstep"][part], got_oracle["pts"]["maxstep"][part]), name
    return c, got, un


@pytest.mark.parametrize("name", sorted(n for n, v in common.CASES.items() if v[4] == "random" and v[1] == 0))
def test_stage_point_counts(name):
    _stage(name)


def test_stage_level1_holds_nothing_of_a_large_level0():
    """16385 points fill the partial rows of all 256 blocks; the 391 points of level 1 use 13 of them right after"""
    _stage("n16385_large_t_s1")
    for name in ("n16385_level1_large_t_s1", "n16385_level1_small_t_s0"):
        c, got, _ = _stage(name)
        assert c.lvl == 1 and len(c.pts) == 391


@pytest.mark.parametrize("index", common.ONE_HOT)
def test_stage_one_good_point(index):
    """every sum is that one point's contribution, E its energy plus the carried energy[0] of all the others: a dropped lane group or partial row is a zero"""
    c, got, _ = _stage(f"n8225_one_hot_{index}")
    assert c.ref.isGood_new[index] and c.ref.isGood_new.sum() == 1
    assert np.all(got["H"][np.abs(c.ref.sums["H"][0]) > 0] != 0) and np.all(got["Hsc"][np.abs(c.ref.sums["Hsc"][0]) > 0] != 0)


@pytest.mark.parametrize("kind", sorted(common.POSES))
def test_stage_nonfinite_taps(kind):
    c, got, _ = _stage(f"n8225_nonfinite_{kind}")
    r = c.ref
    good = c.pts["isGood"] != 0
    assert (good & (r.first_bad == 0)).any() and np.all(got["pts"]["maxstep"][good & (r.first_bad == 0)] == np.float32(1e10))
    hit = good & (r.first_bad < 8) & (r.margins.px > 1.0) & (r.margins.depth > 0.5)          # bad through a non-finite tap, not through the border
    assert hit.sum() >= 3 and not got["pts"]["isGood_new"][hit].any()


@pytest.mark.parametrize("mode,pending", STEP_MODES)
@pytest.mark.parametrize("n0", (8225, 33))
def test_step(n0, mode, pending):
    name = f"n{n0}_large_t_s1"
    c = common.case(name)
    g, o = device_handle(n0), common.oracle_handle(n0)
    first = common.run_impl(g, c)                                   # provides Jb, energy_new, isGood_new, lastHessian_new
    q = step_inputs(first["pts"], first["jb"], 11 + n0)
    if not pending:                                                 # as an applied step leaves it: a good point has a Jb row (rows of points that are not good-new are not written)
        q["isGood"] &= q["isGood_new"]
    args = (c.K4, c.lvl, c.first, c.cur)

    def after(q):
        sr = common.step_ref(q, first["jb"], mode, pending, INC, LAMBDA)
        r = sr.pts.copy()
        r["idepth_new"] = sr.idn
        return sr, r

    # decisions of the evaluation behind the step must not sit on a threshold either: the same guards, at the inverse depths the step will give
    sr, r = after(q)
    m = common.stage_ref(*args, r, c.T, c.a, c.b, c.snapped).margins
    under = (r["isGood"] != 0) & ((m.px < common.GUARD_PX) | (m.depth < common.GUARD_PX) | (m.energy < common.GUARD_REL))
    assert under.mean() <= 0.01
    q["isGood"][under] = 0
    sr, r = after(q)
    assert (sr.clamp_lo.any() and sr.clamp_hi.any()) or mode == 0
    g.set_points(c.lvl, q)
    H, b, Hsc, bsc, res, ec = g.eval_step(c.lvl, mode, pending, INC, LAMBDA, c.T, c.a, c.b)
    p = g.points(c.lvl)
    common.check_step(p, sr, f"{name} mode {mode} pending {pending}")
    # the sums of the same launch, at the inverse depths the device has taken
    r["idepth_new"] = p["idepth_new"]
    ref = common.stage_ref(*args, r, c.T, c.a, c.b, c.snapped)
    cr = common.types.SimpleNamespace(lvl=c.lvl, pts=r, T=c.T, a=c.a, b=c.b, snapped=c.snapped)
    u_oracle = common.measure(common.run_impl(o, cr), ref, cap_maxstep=True)
    got = dict(H=H, b=b, Hsc=Hsc, bsc=bsc, res=res, ec=ec, pts=p, jb=g.jb(c.lvl))
    common.check_stage(got, ref, u_oracle, f"{name} mode {mode} pending {pending} sums")


def test_track_frame_after_a_debug_step_needs_no_care():
    """INI_BEGIN resets what ldso_init_debug_eval_step leaves in the control record: with the points put back, trackFrame gives what an untouched handle gives"""
    from ldso_amd import binding
    seq, _, _ = common.sequence()
    pts = common.base_points(33)
    hs = []
    for touched in (True, False):
        g = binding.Initializer(common.W0, common.H0, common.LEVELS)
        g.set_first(seq["K4"], seq["first"], pts)
        g.set_new_frame(seq["frames"][1], 1.0)
        if touched:
            c = common.case("n33_large_t_s1")
            g.calc_res_and_gs(0, c.T, c.a, c.b)
            g.eval_step(0, 1, 1, INC, LAMBDA, c.T, c.a, c.b)
            for lvl in range(common.LEVELS):
                g.set_points(lvl, pts[lvl])
        hs.append(g)
    for k in range(2):
        a, b = (h.track_frame(seq["frames"][k], 1.0) for h in hs)
        assert a.tobytes() == b.tobytes(), k
        for lvl in range(common.LEVELS):
            assert hs[0].points(lvl).tobytes() == hs[1].points(lvl).tobytes(), (k, lvl)
    for h in hs:
        h.close()
