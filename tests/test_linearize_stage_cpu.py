"""The yardstick of tests/test_linearize_stage_gpu.py (tests/linearize_stage_common.py) must hold on its own, without a GPU: a reference that is wrong fails here.

(a) The oracle (oracle/backend.cc, the float32 restatement of the reference project) runs one plain pass and solveSystemF(0) on every case and is measured against the
    float64 reference, per quantity, in units of eps32 * S.  It stays within the recorded table YARDSTICK (so the table cannot go stale), and over all cases it comes
    within a factor of two of every entry (so the table is not slack either).  The kernel's bound, max(FLOOR_UNITS, ORACLE_FACTOR x yardstick), is never taken from the
    kernel under test.
(b) Every deliberately wrong variant of the reference (FAULTS) puts the oracle over the kernel's bound on at least one quantity of at least one case, or makes a decision
    outside the guards differ.
(c) The decisions the reference adopts from the oracle (margins under the guard) stay under ADOPT_CAP of a case's residuals.
(d) On the `tiny` window the reference agrees with oracle/spec_np.py (linearize_np, explicit_system) to the tolerances tests/test_oracle_spec.py uses."""
import numpy as np
import pytest

from conftest import rel, blockrel
import linearize_stage_common as common
from oracle import pyoracle as po, spec_np as sp

IDS = list(common.CASES)


@pytest.mark.parametrize("name", IDS)
def test_oracle_within_yardstick(name):
    inp, got = common.oracle_run(name)
    ref = common.oracle_reference(name)
    un = common.measure(got, ref)
    print(name, "oracle units", {q: round(v, 2) for q, v in un.items()}, "adopted", ref.n_adopted, "of", int(ref.want.sum()))
    over = {q: (v, common.YARDSTICK[q]) for q, v in un.items() if not v <= common.YARDSTICK[q]}
    assert not over, (name, "the oracle is outside its recorded yardstick", over)
    assert ref.n_adopted <= common.ADOPT_CAP * int(ref.want.sum()), (name, ref.n_adopted, int(ref.want.sum()))          # (c)
    common.check(got, ref, name)                                       # the oracle passes the GPU assertion (exercises the path)


def test_yardstick_table_is_reached():
    worst = {}
    for name in IDS:
        _, got = common.oracle_run(name)
        for q, v in common.measure(got, common.oracle_reference(name)).items():
            worst[q] = max(worst.get(q, 0.0), v)
    assert set(worst) == set(common.QUANTITIES)
    slack = {q: (worst[q], common.YARDSTICK[q]) for q in worst if worst[q] < 0.5 * common.YARDSTICK[q]}
    assert not slack, ("YARDSTICK entries more than twice what the oracle shows", slack)


def test_cases_cover_the_branches():
    """what the cases are named for that shows without a GPU: residual states of all three kinds, both Huber branches, points without / with one / with all residuals,
    an empty host, linearised residuals"""
    st = np.zeros(3, int)
    inside = total = 0
    for name in IDS:
        ref = common.oracle_reference(name)
        st += np.bincount(ref.state[ref.want], minlength=3)[:3]
        inside += int(ref.huber_inside.sum()); total += int(ref.huber_used.sum())
    assert (st > 0).all(), st
    assert 0.02 * total < total - inside < 0.5 * total
    w = common.case_window("F5_residual_counts")
    cnt = w.points["res_count"]
    assert (cnt == 0).any() and (cnt == 1).any() and (cnt == w.F - 1).any()
    w = common.case_window("F6_empty_host")
    assert not (w.points["host"] == 3).any() and (w.points["host"] == 2).any() and (w.points["host"] == 4).any()
    assert common.oracle_reference("F5_mixed").has_L and common.oracle_reference("F5_mixed").actL.sum() > 20
    for name in IDS:                                                     # idepth != idepth_zero: the FEJ point of the geometry differs from the current state
        w = common.case_window(name)
        assert (w.points["idepth"] != w.points["idepth_zero"]).mean() > 0.9
        assert np.abs(w.frames["state"] - w.frames["state_zero"]).max() > 0 or w.F == 2


SENSITIVITY_CASES = ("F5_chunk12", "F2", "F9_pair", "F5_mixed", "F5_residual_counts")


@pytest.mark.parametrize("fault", common.FAULTS)
def test_yardstick_rejects_wrong_reference(fault):
    bd = common.bounds()
    fired = []
    for name in SENSITIVITY_CASES:
        _, got = common.oracle_run(name)
        ref = common.oracle_reference(name, fault)
        try:
            un = common.measure(got, ref)
        except AssertionError:
            fired.append((name, "state_NewState"))
            continue
        fired += [(name, q) for q, v in un.items() if v > bd[q]]
    print(fault, "fires on", fired)
    assert fired, (fault, "the oracle passes against this wrong reference on every quantity of", SENSITIVITY_CASES)
    # ... and on what a pass WITHOUT the Jacobian dump and without the separate system shows (the fused step's view): per residual, per point, HFinal | bFinal
    plain = set(common.PER_RES + common.PER_POINT_ACC + common.FINAL + ("state_NewState",))
    assert any(q in plain for _, q in fired), (fault, "fires only on dumped Jacobians or on the separate system", fired)


def test_reference_agrees_with_spec_np(tiny):
    o = po.OracleWindow(tiny)
    inp = common.make_inputs(tiny, o.get_precalc())
    o.close()
    ref = common.reference(inp)
    Jn = sp.linearize_np(tiny)
    act = ref.actA
    assert act.sum() > 0.9 * tiny.R
    for k, tol in [("Jpdxi", 1e-5), ("Jpdc", 1e-4), ("Jpdd", 1e-5), ("JIdx", 1e-4), ("JabF", 1e-5), ("resF", 5e-4)]:
        assert rel(ref.per_res[k].v[act], Jn[k][act]) < tol, k
    assert rel(ref.per_res["energyWO"].v[act], Jn["energy"][act]) < 5e-4
    assert rel(ref.per_res["centerProjectedTo"].v[act], Jn["center"][act]) < 1e-5
    assert not (Jn["oob"] & act).any()
    adH, adT = sp.adjoints_np(tiny.frames)
    mine = common.adjoints(tiny.frames)
    assert rel(mine[0], adH) < 1e-6 and rel(mine[1], adT) < 1e-6
    J = {k: ref.per_res[k].v for k in ("resF", "Jpdxi", "Jpdc", "Jpdd", "JIdx", "JabF")}
    ex = sp.explicit_system(tiny, J, act, adH, adT)
    s = ref.system
    assert rel(s["HA"].v, ex["Hcc"]) < 1e-6 and blockrel(s["HA"].v, ex["Hcc"]) < 1e-5
    assert rel(s["bA"].v, ex["bc"]) < 1e-6
    Hpp = np.maximum(ex["Hpp"], 1e-10)
    assert rel(s["Hsc"].v, (ex["Hcp"] / Hpp[None, :]) @ ex["Hcp"].T) < 1e-6 and rel(s["bsc"].v, (ex["Hcp"] / Hpp[None, :]) @ ex["bp"]) < 1e-6
    assert rel(ref.per_point["Hdd_accAF"].v, ex["Hpp"]) < 1e-6 and rel(ref.per_point["bd_accAF"].v, ex["bp"]) < 1e-6
