"""GpuBackend::makeNewTraces (adapter/ldso_gpu_adapter.cc) on a reference object graph, through adapter_capi.cc's adp_make_new_traces: frame->features after the
call against the numpy restatement of FeatureDetector::DetectCorners + the ImmaturePoint constructor (tests/feature_detect_common.py)."""
import ctypes as C

import numpy as np
import pytest

import feature_detect_common as fc
from ldso_amd import synth
from oracle import pyref as pr

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not (pr.available() and pr.adapter_available()), reason="oracle/_ref/libldso_ref.so / adapter/_build/libldso_adapter_test.so not built")]


def make_new_traces(A, r, fh, n, cap=1024):
    r.fs_attach()
    fs = C.c_void_p(r.L.ref_fs_handle(r.h))
    pat = np.ascontiguousarray(fc.golden()["pattern"], np.int32)
    feat, desc, imm, counts = np.zeros((cap, 5), np.float32), np.zeros((cap, 32), np.uint8), np.zeros(cap, synth.IMMATURE_DTYPE), np.zeros(4, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    A._chk(A.A.adp_make_new_traces(A.h, fs, fh, p(pat), C.c_int(n), None, C.c_int(cap), p(feat), p(desc), p(imm), p(counts)))
    k = int(counts[3])
    return feat[:k], desc[:k], imm[:k], counts


def test_adapter_make_new_traces_fills_frame_features():
    win = synth.make_config("tiny", extra_frames=1)
    n = 700
    r = pr.RefWindow(win)
    A = pr.GpuAdapter(max_frames=win.F + 1, max_points=win.P + 16)
    clean = np.ascontiguousarray(win.images[win.F][0], np.float32)
    W0 = fc.detect(clean, n, None, fc.golden()["pattern"])["features"]
    bad_irr = clean[..., 0].copy()
    bad_irr[int(W0["v"][40]), int(W0["u"][40])] = np.nan          # on a feature: whatever is picked around it samples the NaN with one of its pattern taps
    T = win.truth["w2c"][win.F]
    for dI in (clean, synth.make_images(bad_irr, 1)[0]):
        R = fc.detect(dI, n, None, fc.golden()["pattern"])
        W, Q = R["features"], fc.immature(dI, R["features"], host=-1)
        keep = np.isfinite(Q["energyTH"])
        feat, desc, imm, counts = make_new_traces(A, r, r.fs_new_frame(dI, T, 0.0, 0.0), n)
        assert counts[0] == len(W) and counts[1] == R["n_corners"] and counts[2] == (~keep).sum() and counts[3] == keep.sum() == len(feat)
        assert (dI is clean) == bool(keep.all())
        W, Q, U = W[keep], Q[keep], R["unsafe"][keep]
        assert np.array_equal(feat[:, 0], W["u"]) and np.array_equal(feat[:, 1], W["v"]) and np.array_equal(feat[:, 2].view(np.uint32), W["score"].view(np.uint32))
        assert np.array_equal(feat[:, 3] != 0, W["is_corner"] != 0)
        fin = np.isfinite(W["angle"])          # a corner whose moment patch holds the NaN pixel has a NaN angle on both sides
        assert np.array_equal(np.isfinite(feat[:, 4]), fin) and (dI is clean) == bool(fin.all())
        d = np.abs(feat[fin, 4].astype(np.float64) - W["angle"][fin])
        assert np.minimum(d, 2 * np.pi - d).max() <= 2e-6
        diff = np.unpackbits(desc ^ W["descriptor"], axis=1, bitorder="little").astype(bool)
        assert not (diff & ~U).any() and desc[W["is_corner"] == 1].any()
        assert imm.tobytes() == Q.tobytes()
    A.close()
    r.L.ref_fs_release_new_frames()
