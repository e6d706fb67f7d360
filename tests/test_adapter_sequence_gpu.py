"""The drop-in END TO END: eight consecutive key frames in FullSystem::makeKeyFrame's order (FullSystem.cc:410-640) on two reference object graphs of
the same synthetic scene - the reference's own members on one (traceNewCoarse, optimizeImmaturePoint loop, optimize), ldso::GpuBackend on the other -
with everything around them (insertFrame, new residuals, removeOutliers, flagPointsForRemoval, dropPointsF, marginalizePointsF, marginalizeFrame) the
reference's host code on both.  The window grows from 5 to 6 key frames, then slides: image slots are recycled, the prior H_M / b_M is re-uploaded
after every marginalisation, lastResiduals / maxRelBaseline / numGoodResiduals travel through six optimize() calls.  Compared after EVERY key frame:
the key-frame set (ids) and per-frame point / residual / immature counts, the trajectory (camToWorld), the affine parameters, the prior, the
inverse depths - maxima and medians."""
import numpy as np
import pytest

from conftest import observe
from ldso_amd import synth
from oracle import pyref as pr

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not (pr.available() and pr.adapter_available()), reason="oracle/_ref/libldso_ref.so / adapter/_build/libldso_adapter_test.so not built")]

K = 8


def _rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


@pytest.mark.parametrize("policy,device_marg", [("oldest", False), ("oldest", True), ("rotate", False), ("rotate", True), ("middle", True), ("two", True)],
                         ids=["False", "True", "rotate-False", "rotate-True", "middle-True", "two-True"])
def test_eight_key_frames_through_the_adapter_follow_the_reference(policy, device_marg):
    """device_marg: the point marginalisation after optimize() through GpuBackend::flagPointsForRemoval + marginalizePoints (the policy on the host, the
    re-linearise / fix / accumulate pass of FullSystem.cc:1241-1250 + EnergyFunctional.cc:165-222 as ldso_ba_marginalize_points on the resident window)
    and the frame marginalisation through GpuBackend::marginalizeFrame (ldso_ba_marginalize_frame) instead of the reference's host members on what the
    adapter wrote back.  policy: which frames leave (adapter_sequence_common.frames_to_marginalize) - the oldest, or middle ones as the reference's own
    flagFramesForMarginalization picks them (FullSystem.cc:647-720), or two in one key frame."""
    from adapter_sequence_common import run_sequence, reference_yardstick, sequence_distance, QUANTITIES
    win = synth.make_config("small", extra_frames=K)
    r_ref, log_ref = run_sequence(win, K, marg_policy=policy)
    A = pr.GpuAdapter(max_frames=8, max_points=4000)
    pr.set_device_marginalisation(device_marg)
    try:
        r_adp, log_adp = run_sequence(win, K, adapter=A, marg_policy=policy)
    finally:
        pr.set_device_marginalisation(False)
    assert len(log_ref) == len(log_adp) == K
    # Which half ran where: without these counters a device_marg run whose every marginalizeFrame fell back to the host member would compare the
    # reference with itself for the frame half
    n_marg = sum(rec["marginalised"] for rec in log_adp)
    kf_marg = sum(rec["marginalised"] > 0 for rec in log_adp)
    on_device, on_host = A.marg_frame_counts()
    assert n_marg == sum(rec["marginalised"] for rec in log_ref) == 7 and kf_marg == (4 if policy == "two" else 7)
    if not device_marg:
        assert (on_device, on_host) == (0, 0), "the reference's host member, not through GpuBackend at all"
    elif policy != "two":
        assert on_host == 0 and on_device == n_marg, (policy, on_device, on_host)
    else:
        # the second frame of one key frame falls back to the host: GpuBackend::marginalizeFrame wants the window of optimize() resident, and after the
        # first removal its row bookkeeping (rowFrames_) still has the old length.  Observed: 4 on the device (one per key frame that marginalises), 3 on the host
        assert on_device + on_host == n_marg and on_device >= kf_marg, (on_device, on_host)
        print("policy two: marginalizeFrame on the device", on_device, "on the host", on_host)
    # FrameHessian::dIp on the device: ONE pyramid per frame seen (the 5 frames of the initial window + the 8 new key frames), shared by the tracer, the
    # BA image slot and - in a full system - the coarse trackers; built from 4 bytes per pixel
    assert A.pyramids_built() == win.F + K, A.pyramids_built()
    # The two graphs run DIFFERENT arithmetic for three stages (the device's summation orders): their states agree to ~1e-6 after one stage, and a
    # sliding-window system amplifies that through threshold decisions (an immature point on one side of `interval < 8`, a residual on one side of its
    # outlier energy, a point on one side of the inlier count).  HOW FAR two correct implementations drift apart over these eight key frames is measured on
    # the reference itself (adapter_sequence_common.reference_yardstick: the pin build against its own 6-worker IndexThreadReduce, whose float sums change
    # from run to run, and against the -O3 build of the same translation units); the drop-in may be at most K_YARD x as far from the reference as the
    # reference is from itself, per quantity.  No limit below is derived from the product's own output.
    K_YARD = 3.0
    # the policy's OWN yardstick.  The count-valued quantities (counts, residual_counts, unmatched_points) are 0, 1 or 5 between any two runs of the reference
    # (CPU, three pairs per policy: counts 0-3, residual_counts 0-10, unmatched_points 0-5), and the largest of three pairs is often 0 - a limit of 3 x 0 that
    # no second implementation can meet.  The new policies therefore take six six-thread runs of the reference instead of two: more samples of the
    # reference's own spread, on the CPU only; K_YARD and the `oldest` yardstick stay as they were.
    yard, per = reference_yardstick("small", K, log_ref=log_ref, mt_runs=2 if policy == "oldest" else 6, marg_policy=policy)
    worst, same = sequence_distance(log_ref, log_adp)
    assert same, "same key frames in the window after every key frame, >= 97 % of the points held by both graphs"
    tag = ("sequence_dm_" if device_marg else "sequence_") + ("" if policy == "oldest" else policy + "_")
    print("adapter sequence (policy %s, device marginalisation: %s), worst over" % (policy, device_marg), K, "key frames:", {k: float("%.3g" % v) for k, v in worst.items()},
          "| reference vs reference:", {k: float("%.3g" % v) for k, v in yard.items()})
    # Observed on MI355X (worst over the eight key frames | the policy's yardstick, before x 3):
    #   oldest, host marg    rmse 2.4e-3 | 1.9e-3, pose 9.9e-5 | 2.0e-4, HM 3.7e-5 | 1.3e-3, bM 1.4e-2 | 2.0e-2, idepth_max 1.3e-3 | 1.2e-3, counts 2 | 1, unmatched 4 | 5
    #   oldest, device marg  rmse 1.2e-6, pose 5.0e-6, HM 6.4e-4, bM 9.0e-3, idepth_max 9.3e-5, counts 1, unmatched 0 (same yardstick)
    #   rotate, host / device marg  rmse 1.4e-6 / 9.7e-7 | 1.4e-3, pose 4.6e-6 / 2.7e-6 | 1.8e-4, HM 5.6e-6 | 3.5e-3, bM 7.6e-4 / 7.8e-4 | 2.9e-3, counts 0 | 2, unmatched 0 | 5
    #   middle, device marg  rmse 1.1e-6 | 1.0e-3, pose 3.3e-6 | 1.2e-4, HM 5.6e-6 | 2.5e-3, bM 4.2e-4 | 3.5e-3, counts 0 | 3, unmatched 0 | 5
    #   two, device marg     rmse 3.7e-4 | 3.7e-4, pose 2.4e-5 | 3.2e-5, HM 1.3e-5 | 9.6e-4, bM 3.3e-3 | 1.6e-2, counts 1 | 1, residual_counts 5 | 5, unmatched 1 | 1
    for q in QUANTITIES:
        observe(tag + q, worst[q], K_YARD * yard[q])
    A.close()


def test_resident_window_sequence_equals_full_uploads():
    _resident_window_sequence_equals_full_uploads("oldest")


@pytest.mark.parametrize("policy", ["rotate", "two"])
def test_resident_window_sequence_equals_full_uploads_by_policy(policy):
    _resident_window_sequence_equals_full_uploads(policy)


def _resident_window_sequence_equals_full_uploads(policy):
    """The same eight key frames through two GpuBackends: one keeps the window resident between optimize() calls and sends deltas (ldso_ba_update_window: frames
    that left / arrived, surviving points, one bit per residual, the records of the activated points), the other flattens and uploads the whole window every
    time.  Both describe the same window to the same kernels: key-frame sets, point / residual counts and ids identical after every key frame, every float the
    drop-in writes back within the run-to-run reproducibility of the fused fast path (fp64 atomics, 1e-12 per iteration).  policy: which frames
    leave (adapter_sequence_common.frames_to_marginalize) - a middle frame's removal has to go over as a delta like the oldest one's."""
    from adapter_sequence_common import run_sequence
    win = synth.make_config("small", extra_frames=K)
    out = []
    for resident in (True, False):
        A = pr.GpuAdapter(max_frames=8, max_points=4000)
        A.set_resident_window(resident)
        pr.set_device_marginalisation(True)
        try:
            r, log = run_sequence(win, K, adapter=A, marg_policy=policy)
        finally:
            pr.set_device_marginalisation(False)
        d, f = A.upload_counts()
        out.append((log, d, f))
        A.close()
    (la, da, fa), (lb, db, fb) = out
    assert db == 0 and fb == 2 * K, "without the resident window every upload is a full one (activatePoints + optimize per key frame)"
    print("policy", policy, "resident handle: delta uploads", da, "fresh uploads", fa)
    assert da + fa == 2 * K
    if policy in ("oldest", "rotate"):
        assert fa == 1 and da == 2 * K - 1, (da, fa)      # only the very first window of the handle is flattened: a middle frame's removal goes over as a delta too
    else:
        # two frames leaving in one key frame (the second through the host member, see the counters of the test above) still go over as ONE delta: observed 15 / 1
        assert fa == 1 and da == 2 * K - 1, (da, fa)
    worst = 0.0
    for a, b in zip(la, lb):
        sa, sb = a["summary"], b["summary"]
        assert not a["lost"] and not b["lost"]
        for k in ("candidates", "activated", "new_residuals", "points"):
            assert a[k] == b[k], (a["k"], k, a[k], b[k])
        assert sa["F"] == sb["F"] and np.array_equal(sa["ids"], sb["ids"])
        for k in ("points", "residuals", "immature", "host"):
            assert np.array_equal(sa[k], sb[k]), (a["k"], k)
        assert np.array_equal(sa["uv"], sb["uv"])
        worst = max(worst, abs(a["rmse"] - b["rmse"]) / b["rmse"], *[_rel(sa[k], sb[k]) for k in ("c2w", "aff", "idepth", "HM", "bM")])
    observe("resident_vs_full_upload_sequence_floats" + ("" if policy == "oldest" else "_" + policy), worst, 1e-9)          # observed 8.2e-14 (oldest), 2.3e-13 (rotate), 2.4e-13 (two): two runs of the fused fast path (fp64 atomics) differ by ~1e-12 per iteration
