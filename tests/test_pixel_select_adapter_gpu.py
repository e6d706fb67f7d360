"""GpuBackend::makeNewTraces for setting_pointSelection == 0 (adapter/ldso_gpu_adapter.cc) against the reference's own FullSystem::makeNewTraces, on two
reference object graphs of one scene, through adapter_capi.cc's adp_make_new_traces_pixsel: three key frames whose densities take both recursion branches of
PixelSelector::makeMaps.  frame->features, every ImmaturePoint field its constructor sets and pixelSelector->currentPotential are exactly equal after every frame."""
import ctypes as C

import numpy as np
import pytest

import feature_detect_common as fc
from ldso_amd import synth
from oracle import pyref as pr

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not (pr.available() and pr.adapter_available()), reason="oracle/_ref/libldso_ref.so / adapter/_build/libldso_adapter_test.so not built")]


# ImmaturePoint.h:120-121 declares lastTraceUV and lastTracePixelInterval without an initialiser and the constructor does not set them (traceOn writes both before
# anything reads them): the reference's objects hold whatever the allocation held.  The device record has -1 / 0 there, as ldso_feat_detect's.
CONSTRUCTED = ("u", "v", "color", "weights", "gradH", "energyTH", "idepth_min", "idepth_max", "quality", "lastTraceStatus", "host")


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def pixsel(A, backend, r, fh, density, potential, cap=8192):
    """adp_make_new_traces_pixsel; backend None: the reference's member -> (uv, immature records, my_type, counts, potential left)"""
    uv, imm, typ, counts = np.zeros((cap, 2), np.float32), np.zeros(cap, synth.IMMATURE_DTYPE), np.zeros(cap, np.float32), np.zeros(4, np.int32)
    pot = C.c_int(potential)
    rc = A.adp_make_new_traces_pixsel(backend, r.fs_handle(), fh, C.c_float(density), None, C.byref(pot), C.c_int(cap), _p(uv), _p(imm), _p(typ), _p(counts))
    if rc != 0:
        raise RuntimeError(A.adp_last_error().decode())
    k = int(counts[3])
    assert k <= cap
    return uv[:k].copy(), imm[:k].copy(), typ[:k].copy(), counts, pot.value


def settings(A):
    a, b, c = C.c_int(), C.c_float(), C.c_int()
    assert A.adp_point_selection_settings(C.byref(a), C.byref(b), C.byref(c)) == 0
    return a.value, b.value, c.value


@pytest.mark.parametrize("resident", [True, False], ids=["resident", "transferring"])
def test_make_new_traces_equals_the_reference(resident):
    win = synth.make_config("tiny", extra_frames=3)          # 160 x 128: three pyramid levels, multiples of 32
    r_ref, r_gpu = pr.RefWindow(win), pr.RefWindow(win)
    A = pr.adapter_lib()
    B = pr.GpuAdapter(max_frames=win.F + 1, max_points=win.P + 8192)
    assert A.adp_set_resident_immature(B.h, C.c_int(1 if resident else 0)) == 0
    before = settings(A)
    pots, seen = [3, 3], []
    for k, density in enumerate((700.0, 40.0, 6000.0)):
        irr = np.clip(np.rint(win.images[win.F + k][0][..., 0]), 0, 255).astype(np.float32)
        dI = synth.make_images(irr, 1)[0]
        T = win.truth["w2c"][win.F + k]
        ref = pixsel(A, None, r_ref, r_ref.fs_new_frame(dI, T, 0.0, 0.0), density, pots[0])
        gpu = pixsel(A, B.h, r_gpu, r_gpu.fs_new_frame(dI, T, 0.0, 0.0), density, pots[1])
        print("frame", k, "density", density, "points", len(ref[0]), len(gpu[0]), "potential", pots, "->", ref[4], gpu[4], "types", np.unique(ref[2]))
        assert len(ref[0]) == len(gpu[0]) and np.array_equal(ref[0], gpu[0])                       # frame->features: count, u, v
        for f in CONSTRUCTED:                                                                      # every ImmaturePoint: what its constructor sets, bit for bit
            assert ref[1][f].tobytes() == gpu[1][f].tobytes(), f
        assert np.all(gpu[1]["lastTraceUV"] == -1) and np.all(gpu[1]["lastTracePixelInterval"] == 0) and np.array_equal(ref[2], gpu[2])          # my_type
        assert ref[4] == gpu[4] and ref[3][3] == gpu[3][3] == gpu[3][0] - gpu[3][2]                # currentPotential; nothing dropped that the reference kept
        assert settings(A) == before                                                               # the process-wide settings are back
        seen.append((pots[0], ref[4], len(ref[0])))
        pots = [ref[4], gpu[4]]
    # the three calls: one that keeps the potential's order of magnitude, one that recurses to a larger potential, one that recurses to a smaller one
    assert seen[0][2] > 300 and seen[1][1] > seen[1][0] + 3 and seen[2][1] < seen[2][0] - 3, seen
    # the corner entry of the same process still gives the restatement's result
    n = 700
    clean = np.ascontiguousarray(win.images[win.F][0], np.float32)
    W = fc.detect(clean, n, None, fc.golden()["pattern"])["features"]
    pat = np.ascontiguousarray(fc.golden()["pattern"], np.int32)
    cap = 1024
    feat, desc, imm, counts = np.zeros((cap, 5), np.float32), np.zeros((cap, 32), np.uint8), np.zeros(cap, synth.IMMATURE_DTYPE), np.zeros(4, np.int32)
    B._chk(A.adp_make_new_traces(B.h, r_gpu.fs_handle(), r_gpu.fs_new_frame(clean, win.truth["w2c"][win.F], 0.0, 0.0), _p(pat), C.c_int(n), None, C.c_int(cap), _p(feat), _p(desc),
                                 _p(imm), _p(counts)))
    assert counts[0] == counts[3] == len(W) and np.array_equal(feat[:len(W), 0], W["u"]) and np.array_equal(feat[:len(W), 1], W["v"])
    assert imm[:len(W)].tobytes() == fc.immature(clean, W, host=-1).tobytes()
    B.close(); r_ref.close(); r_gpu.close()
    r_ref.L.ref_fs_release_new_frames()
