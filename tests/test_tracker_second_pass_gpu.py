"""The second pass of tr_eval (more than TR_U = 4 points per lane of a workgroup's share) with a last wavefront that is only partly inside the share.  A cooperative
track reaches it at G <= 8 on a 640 x 480 level (9 - 10 thousand reference points: shares above 1024 points); whether a wavefront ends partly inside depends on the
point count, so the scene is one on which it does (C3, seed 20260925 + 20: found by the grouped tracking of 32 sequences, whose width is 8).  The matrix instructions
take the operands of all 64 lanes whatever the execution mask: every lane of a wavefront has to stay in the loop and stage zeros past the end of the share.  Before
that, lanes that had left the loop fed stale registers into the sums: lastResiduals[0] came out as 0.66 (G = 8) or NaN (G = 4, and G = 8 of the grouped kernel) where
every other width and the oracle have 2.09, the affine pair on another optimum.
Bounds: widths differ only in how the float sums are grouped - the pose to the 1e-4 of test_cooperative_group_sizes_agree, lastResiduals to the 1e-3 relative that
test_track_new_coarse_matches_oracle allows achievedRes, both against the oracle."""
import functools

import numpy as np
import pytest

from tracker_common import tracker_scenario
from ldso_amd import binding
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def scene_and_oracle_track():
    sc = tracker_scenario("C3", seed=20260925 + 20)
    win = sc["win"]
    o = po.OracleTracker(win.w, win.h, sc["levels"], win.settings, win.calib)
    o.set_ref(sc["ref_pyr"], sc["ref_aff"][0], sc["ref_aff"][1], 1.0, sc["pts"])
    o.set_new_frame(sc["new_pyr"], 1.0)
    w2c = win.truth["w2c"]
    T0 = np.eye(4)
    T0[:3, :4] = o.motion_hypotheses(w2c[win.F - 2], w2c[win.F - 1], w2c[win.F - 1])[0]          # try 0 of trackNewCoarse: constant motion
    ro = o.track(T0, sc["new_aff"][0], sc["new_aff"][1], sc["levels"] - 1)
    assert ro["ok"]
    return sc, T0, ro


def make_tracker(sc, st=None):
    win = sc["win"]
    g = binding.Tracker(win.w, win.h, sc["levels"], win.settings, win.calib)
    if st is not None:
        g.set_stream(st)
    g.set_ref(sc["ref_pyr"], sc["ref_aff"][0], sc["ref_aff"][1], 1.0, sc["pts"])
    g.set_new_frame(sc["new_pyr"], 1.0)
    return g


def assert_meets_oracle(r, ro, L, tag):
    print(tag, "lastResiduals", r["lastResiduals"][:L], "oracle", ro["lastResiduals"][:L], "pose", np.abs(r["T"] - ro["T"]).max())
    assert r["ok"], tag
    assert np.isfinite(r["lastResiduals"][:L]).all(), tag
    assert np.abs(r["lastResiduals"][:L] - ro["lastResiduals"][:L]).max() <= 1e-3 * np.abs(ro["lastResiduals"][:L]).max(), tag
    assert np.abs(r["T"] - ro["T"]).max() < 1e-4, tag


@pytest.mark.parametrize("nhyp", [1, 22, 33, 70])
def test_every_width_meets_the_oracle_with_a_partly_filled_last_wavefront(nhyp):
    """G = 16 / 8 / 4 / 1 on a 256-CU card"""
    sc, T0, ro = scene_and_oracle_track()
    g = make_tracker(sc)
    a, b = sc["new_aff"]
    L = sc["levels"]
    rb = g.track_batch([T0] * nhyp, [(a, b)] * nhyp, L - 1)
    for i in (0, nhyp - 1):
        assert_meets_oracle({k: v[i] for k, v in rb.items()}, ro, L, (nhyp, i))


def test_group_of_32_equals_track_batch_of_32():
    """the grouped kernel at the width of 32 jobs, on shares that need the second pass: member i = hypothesis 0 of the member's own batch of 32, byte for byte"""
    import torch
    ts = torch.cuda.Stream(); torch.cuda.set_stream(ts)
    sc, T0, ro = scene_and_oracle_track()
    n = 32
    trk = [make_tracker(sc, ts.cuda_stream) for _ in range(n)]
    a, b = sc["new_aff"]
    L = sc["levels"]
    grp = binding.TrackerGroup(trk)
    try:
        out = grp.track([T0] * n, [(a, b)] * n, [L - 1] * n)
        rb = trk[0].track_batch([T0] * n, [(a, b)] * n, L - 1)
        for i in (0, n // 2, n - 1):
            assert_meets_oracle(out[i], ro, L, ("group", i))
            assert np.array_equal(out[i]["T"], rb["T"][0]) and out[i]["a"] == rb["a"][0] and out[i]["b"] == rb["b"][0], i
            assert np.array_equal(out[i]["lastResiduals"], rb["lastResiduals"][0], equal_nan=True) and out[i]["iterations"] == rb["iterations"][0], i
    finally:
        grp.close()
