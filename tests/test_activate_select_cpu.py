"""Candidate selection of FullSystem::activatePointsMT without a GPU: the host-only density controller (ldso_act_update_min_dist) against the reference's own
member, and the test harness's selection loop (adp_ref_select_candidates + the host activation) against the same member - which pins the yardstick that
tests/test_activate_select_gpu.py compares the device with."""
import numpy as np
import pytest

from ldso_amd import binding, synth
from oracle import pyref as pr

pytestmark = pytest.mark.skipif(not (pr.available() and pr.adapter_available()), reason="oracle/_ref/libldso_ref.so / adapter/_build/libldso_adapter_test.so not built")

THRESHOLDS = (0.66, 0.8, 0.9, 1.0, 1.15, 1.3, 1.5)


def test_density_controller_equals_reference_member():
    """FullSystem.cc:1054-1073 on a graph without immature points, where activatePointsMT() does nothing but move currentMinActDist (and rebuild the map):
    nPoints / desiredDensity on, just below and just above every threshold of the ladder, far below and far above, from start values that reach both clamps."""
    import activation_select_common as asc
    win = synth.make_config("tiny")
    r = pr.RefWindow(win)
    r.fs_attach()
    n = asc.ef_npoints(r)
    assert n == win.P > 0
    ratios = [0.1, 0.5, 2.0, 10.0]
    for t in THRESHOLDS:
        ratios += [t, t * (1 - 1e-3), t * (1 + 1e-3), t * (1 - 3e-2), t * (1 + 3e-2)]
    densities = sorted({float(np.float32(n / q)) for q in ratios} | {float(n)})
    starts = (0.0, 0.05, 0.3, 0.75, 1.0, 2.0, 3.15, 3.7, 3.95, 4.0)
    old = asc.set_desired_point_density(asc.DEFAULT_DENSITY)
    moved = set()
    try:
        for d in densities:
            asc.set_desired_point_density(d)
            for s in starts:
                asc.set_min_act_dist(r, s)
                asc.ref_activate_points_mt(r)
                want = np.float32(asc.min_act_dist(r))
                got = np.float32(binding.act_update_min_dist(s, n, d))
                assert np.array_equal(got, want), (d, s, got, want)
                moved.add(round(float(want) - s, 3))
    finally:
        asc.set_desired_point_density(old)
        r.close()
    # every rung of the ladder was taken somewhere: the sums the thresholds produce away from the clamps
    assert {-1.3, -0.5, -0.2, -0.1, 0.0, 0.1, 0.3, 0.8, 1.6} <= moved, sorted(moved)


def test_harness_selection_loop_equals_reference_member():
    """adp_ref_select_candidates (the loop of FullSystem.cc:1088-1152 through the compiled CoarseDistanceMap) + the controller + the reference's
    activatePointsMT_Reductor and hand-over, against fs.activatePointsMT() itself on an identical graph: every Feature::status, the points per frame,
    currentMinActDist and the final distance map."""
    import activation_select_common as asc
    win, (r_loop, r_mem), pts = asc.make_state("small", per_frame=300, P=150, n_graphs=2)
    old = asc.set_desired_point_density(asc.DEFAULT_DENSITY)
    try:
        for step, density in enumerate((60.0, 2000.0)):          # far too many points: the distance grows; far too few: it shrinks
            asc.set_desired_point_density(density)
            before = asc.feature_statuses(r_mem)
            assert np.array_equal(before, asc.feature_statuses(r_loop))
            asc.ref_activate_points_mt(r_mem)
            cur = binding.act_update_min_dist(asc.min_act_dist(r_loop), asc.ef_npoints(r_loop), density)
            asc.set_min_act_dist(r_loop, cur)
            s = asc.ref_select(r_loop, cur)
            asc.ref_apply_selection(r_loop, s["decision"], s["selected"])
            assert np.float32(asc.min_act_dist(r_mem)) == np.float32(cur) and cur != 2.0
            st_mem, st_loop = asc.feature_statuses(r_mem), asc.feature_statuses(r_loop)
            assert np.array_equal(st_mem, st_loop)
            assert (st_mem != before).sum() > 50, "the step activated and deleted points"
            assert len(s["selected"]) > 20 and (s["decision"] == asc.KEEP).sum() > 20
            assert step > 0 or (s["decision"] == asc.DROP).sum() > 20          # the second step finds the deletable ones gone
            ga, gb = pr.graph_summary(r_mem), pr.graph_summary(r_loop)
            assert np.array_equal(ga["points"], gb["points"]) and np.array_equal(ga["immature"], gb["immature"]) and np.array_equal(ga["residuals"], gb["residuals"])
            assert np.array_equal(ga["idepth"], gb["idepth"])
            assert asc.ef_npoints(r_mem) == asc.ef_npoints(r_loop)
            assert np.array_equal(asc.ref_distance_map(r_mem), s["map_after"])
    finally:
        asc.set_desired_point_density(old)
        r_loop.close(); r_mem.close()
