"""The yardstick of tests/test_init_stage_gpu.py (tests/init_stage_common.py) must hold on its own, without a GPU: a reference that is wrong fails here.

Per case of the GPU file the float64 reference is compared with the float32 restatement of CoarseInitializer (oracle/initializer.cc): every decision (isGood_new)
equal, carried energies and the exactly prescribed maxstep values byte-equal, res[1], res[2], ec[2] exact, and the oracle's error per quantity printed in units of
eps32 * S (S = sum of the |addends| of the entry; for the quantities of one point S is built from the sizes of what its image taps are made of).  Measured over
all 111 cases, the oracle's worst per quantity: H 233, b 43, Hsc 165, bsc 26, E 6.7, ec0 6.1, ec1 15.9, energy_new 3.6, lastHessian_new 0.19, maxstep 5.7, Jb 7.3
(the large values come from the cases with one good point and from n <= 33, where nothing averages); on the random cases with n >= 8191: H 31, b 0.42, Hsc 82,
bsc 20, E 1.0.  A point dropped from 16385 moves the sums by about a thousand units, so 4 x the oracle's units stays well below one dropped point there (asserted:
at most 250).
The case builder's guards (1e-2 px, 1e-2 of the depth, 1e-3 relative of the outlier threshold) remove at most 1 % of a case's points.
Coverage is asserted, not assumed: both alpha branches and t = 0, a good point whose first bad pattern pixel is k for every k = 0 .. 7, outlier rejections,
new_idepth <= 0, residuals on both sides of the Huber threshold.
Sensitivity: deliberately wrong variants of the reference - one point dropped, a partial row of two points dropped, pattern pixel 7 dropped, the alpha branch
swapped, the square root of the Huber weight omitted, rv * w instead of rv * rv * w on the Schur diagonal, doStep without its maxstep clamp, applyStep without
lastHessian - each fail the assertion the GPU tests make; the unmodified reference passes it.

One difference between the oracle and the kernel is known and harmless: the reference implementation takes the minimum into a maxstep that starts at 1e10, the
kernel takes it over the visited pattern pixels alone, so at t = 0 (1 / sqrt(0)) the oracle keeps 1e10 where the kernel stores +inf.  doStep caps 0.25 * maxstep at
1e10 and the inverse depth is clamped to [1e-3, 50] behind it, so no result depends on it.  The oracle is measured with the minimum capped at 1e10."""
import numpy as np
import pytest

import init_stage_common as common

ORACLE_CAP = 500.0          # units; the worst the oracle shows on any case and quantity is recorded above: half of this

IDS = sorted(common.CASES)


@pytest.mark.parametrize("name", IDS)
def test_reference_against_oracle(name):
    c = common.case(name)
    un, got = common.oracle_units(name)          # asserts the decisions and everything exact
    print(name, "oracle units", {q: round(un[q], 2) for q in common.QUANTITIES}, "guarded", c.removed, "good-new", int(c.ref.isGood_new.sum()))
    assert c.removed <= 0.01
    assert all(np.isfinite(un[q]) for q in common.QUANTITIES)
    assert all(un[q] <= ORACLE_CAP for q in common.QUANTITIES), "the oracle is further from the float64 reference than float32 arithmetic explains"
    if c.n0 >= 8191 and c.what == "random" and c.lvl == 0:
        assert max(un[q] for q in ("H", "b", "Hsc", "bsc", "E")) <= 250.0          # 4 x this is the GPU bound; one dropped point of 16385 makes about 1000
    common.check_stage(got, c.ref, un, name, cap_maxstep=True)     # the oracle passes the GPU assertion with its own units as u_oracle (by construction; exercises the path)


def test_cases_cover_the_branches():
    first_bad = np.zeros(9, int)
    outliers = nonpos = below = above = 0
    alpha = set()
    for name in IDS:
        c = common.case(name)
        r = c.ref
        alpha.add((r.alphaOpt, bool(r.t_is_zero)))
        first_bad += np.bincount(r.first_bad[c.pts["isGood"] != 0], minlength=9)
        outliers += int(r.outlier.sum()); nonpos += int(r.new_idepth_nonpositive.sum())
        res = np.abs(r.residual[np.isfinite(r.residual)])
        below += int((res < common.HUBER).sum()); above += int((res >= common.HUBER).sum())
    print("first bad pattern pixel of good points", first_bad, "outliers", outliers, "new_idepth <= 0", nonpos, "residuals below / above huberTH", below, above)
    assert alpha == {(0.0, False), (common.ALPHA_W, False), (common.ALPHA_W, True)}
    assert (first_bad > 0).all()
    assert outliers > 0 and nonpos > 0
    assert below >= 0.1 * (below + above) and above >= 0.1 * (below + above)


def test_nonfinite_pixels_sit_under_known_points():
    """the NaN / +Inf pixels make known points bad at a known pattern pixel: the nearest point of the level whose pattern pixel 0 (new frame, +Inf) or 4 (NaN) taps
    the pixel and none of the earlier ones does"""
    c = common.case("n8225_nonfinite_large_t")
    r = c.ref
    good = c.pts["isGood"] != 0
    assert (good & (r.first_bad == 0) & (r.maxstep == 1e10)).any()
    hit_by_nan = good & (r.first_bad < 8) & (r.margins.px > 1.0) & (r.margins.depth > 0.5) & ~r.new_idepth_nonpositive          # bad, and not through the border
    assert hit_by_nan.sum() >= 3 and len(set(r.first_bad[hit_by_nan])) >= 4
    assert not r.isGood_new[hit_by_nan].any()
    for nm in common.SUMS:
        assert np.isfinite(r.sums[nm][0]).all()


SENSITIVITY_CASES = ["n33_large_t_s1", "n8225_small_t_s0", "n16385_large_t_s1", "n16385_small_t_s1"]


def _variant(c, fault):
    return common.stage_ref(c.K4, c.lvl, c.first, c.cur, c.pts, c.T, c.a, c.b, c.snapped, fault=fault)


def _faults(c):
    gn = np.nonzero(c.ref.isGood_new)[0]
    one = int(gn[len(gn) // 2])
    even = gn[(gn % 2 == 0) & (gn + 1 < len(c.pts))]
    row = int(even[np.argmax(c.ref.isGood_new[even + 1])])          # an even index whose neighbour is good-new too: 16 lanes of the kernel
    return {"one_point": ("drop_points", (one,)), "partial_row": ("drop_points", (row, row + 1)), "pixel7": "drop_pixel7", "alpha": "swap_alpha",
            "huber_sqrt": "no_sqrt_huber", "schur_diagonal": "sc_diag"}


@pytest.mark.parametrize("fault", ["one_point", "partial_row", "pixel7", "alpha", "huber_sqrt", "schur_diagonal"])
def test_yardstick_rejects_wrong_stage(fault):
    """every wrong variant fails the GPU assertion on at least one case - here: on every case that has more than a handful of points"""
    for name in SENSITIVITY_CASES:
        c = common.case(name)
        un, got = common.oracle_units(name)
        common.check_stage(common.as_got(c.ref), c.ref, un, name + " unmodified")
        bad = common.as_got(_variant(c, _faults(c)[fault]))
        if fault in ("one_point", "partial_row"):
            bad["pts"], bad["jb"] = common.as_got(c.ref)["pts"], common.as_got(c.ref)["jb"]          # the records are right: only the sums miss the points
            bad["ec"][2] = np.float32(c.ref.ec2)
        with pytest.raises(AssertionError):
            common.check_stage(bad, c.ref, un, name + " " + fault)


INC = np.array([0.011, -0.007, 0.013, -0.004, 0.006, 0.009, 0.02, -0.5], np.float32)
LAMBDA = 0.1
STEP_MODES = ((1, 1), (1, 0), (0, 1))


def step_inputs(pts, jb, seed):
    """the records of a step test: what an evaluation left, with maxstep tiny / +inf and inverse depths within a step of the end of [1e-3, 50] the step goes to"""
    rng = np.random.default_rng(seed)
    q = pts.copy()
    n = len(q)
    kind = np.arange(n) % 8                                                 # 0, 7: as it is, 1: tiny maxstep, 2: +inf, 3 .. 6: next to the clamp; all there from 8 points on
    down = (jb[:, 8].astype(np.float64) + jb[:, :8].astype(np.float64) @ INC.astype(np.float64)) * jb[:, 9] > 0          # the step is -b * Jb[9] / (1 + lambda)
    near = (kind >= 3) & (kind <= 6)
    q["maxstep"] = np.where(kind == 1, 1e-6, np.where(kind == 2, np.inf, np.where(near, 1e3, q["maxstep"]))).astype(np.float32)
    for f in ("idepth", "idepth_new"):
        q[f] = np.where(near & down, np.float32(1e-3) * (1 + rng.uniform(0, 0.5, n)), np.where(near & ~down, 50.0 - rng.uniform(0, 1e-3, n), q[f])).astype(np.float32)
    return q


@pytest.mark.parametrize("fault", ["no_maxstep_clamp", "no_lastHessian"])
def test_yardstick_rejects_wrong_step(fault):
    name = "n8225_large_t_s1"
    _, got = common.oracle_units(name)
    q = step_inputs(got["pts"], got["jb"], 5)
    good = common.step_ref(q, got["jb"], 1, 1, INC, LAMBDA)
    assert good.clamp_lo.any() and good.clamp_hi.any() and (q["maxstep"][good.good] == np.inf).any()
    g = good.pts.copy(); g["idepth_new"] = good.idn
    common.check_step(g, good, "unmodified")
    wrong = common.step_ref(q, got["jb"], 1, 1, INC, LAMBDA, fault=fault)
    w = wrong.pts.copy(); w["idepth_new"] = wrong.idn
    with pytest.raises(AssertionError):
        common.check_step(w, good, fault)
