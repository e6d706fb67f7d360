"""GpuBackend::setUndistortion / undistortFrame (adapter/ldso_gpu_adapter.cc) through adapter_capi.cc: the pyramid a raw frame leaves under its Frame::id
is the one pyramidOf builds from the same irradiance uploaded from the host, and the consumers of that frame find it instead of building another."""
import ctypes as C

import numpy as np
import pytest

import undistort_common as uc
from ldso_amd import synth
from oracle import pyoracle as po
from oracle import pyref as pr

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not (pr.available() and pr.adapter_available()), reason="oracle/_ref/libldso_ref.so / adapter/_build/libldso_adapter_test.so not built")]


def p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def undistort_frame(A, frame_id, raw, exposure, factor, host=None):
    e = C.c_float()
    A._chk(A.A.adp_undistort_frame(A.h, C.c_long(frame_id), p(raw), C.c_int(raw.dtype.itemsize), C.c_float(exposure), C.c_float(factor), p(host), C.byref(e)))
    return e.value


def pyramid(A, fh, w, h, levels):
    out = [np.zeros((h >> l, w >> l, 3), np.float32) for l in range(levels)]
    for l in range(levels):
        A._chk(A.A.adp_get_pyramid_level(A.h, fh, C.c_int(l), p(out[l])))
    return out


def test_undistorted_frame_is_registered_for_its_consumers():
    win = synth.make_config("tiny", extra_frames=1)
    h, w = win.images[0][0].shape[:2]
    w_org, h_org = w + 17, h + 9
    rx, ry = uc.synthetic_tables(w_org, h_org, w, h, seed=11)
    f8, f16 = uc.textured_frames(w_org, h_org, seed=12)
    g = uc.golden()
    vig = (1.0 / np.random.default_rng(13).uniform(0.4, 1.0, (h_org, w_org))).astype(np.float32)
    pts, _ = synth.make_immature_points(win, 40)
    T = win.truth["w2c"][win.F]
    ra, rb = pr.RefWindow(win), pr.RefWindow(win)                          # they set the globals (wG, hG, pyrLevelsUsed) the backends read
    A = pr.GpuAdapter(max_frames=win.F + 1, max_points=win.P + 16)          # undistorts on the device
    B = pr.GpuAdapter(max_frames=win.F + 1, max_points=win.P + 16)          # gets the same irradiance as a host image
    A.A.adp_frame_id.restype = C.c_long
    levels = A.A.adp_pyr_levels_used()
    for r in (ra, rb):
        r.fs_attach(); r.fs_add_immature(pts)
    A._chk(A.A.adp_set_undistortion(A.h, C.c_int(w_org), C.c_int(h_org), p(rx), p(ry), p(g["G256"]), C.c_int(256), p(vig), C.c_int(2), C.c_int(0)))
    for raw, exposure, factor, mode in ((f8, 0.5, 1.0, uc.VIGNETTE), (f16, 0.0, 1.0 / 256, uc.PLAIN)):
        irr = uc.undistort(raw, rx, ry, w_org, h_org, w, h, g["G256"], vig, mode, factor)
        dI = po.make_images(irr, 1)[0]
        fha, fhb = ra.fs_new_frame(dI, T, 0.0, 0.0), rb.fs_new_frame(dI, T, 0.0, 0.0)
        ida = A.A.adp_frame_id(fha)
        built = A.pyramids_built()
        host = np.zeros((h, w), np.float32) if raw is f8 else None          # the host copy only when asked for
        assert undistort_frame(A, ida, raw, exposure, factor, host) == 1.0   # setting_useExposure off
        assert host is None or host.tobytes() == irr.tobytes()
        assert A.pyramids_built() == built + 1
        # a consumer of that frame finds the pyramid: none is built from fh->dIp[0]
        counts_a = A.trace_new_coarse(ra, fha)
        got = pyramid(A, fha, w, h, levels)
        assert A.pyramids_built() == built + 1
        # the host path on the other backend builds one, from the same irradiance: the same pyramid and the same trace
        built_b = B.pyramids_built()
        counts_b = B.trace_new_coarse(rb, fhb)
        ref = pyramid(B, fhb, w, h, levels)
        assert B.pyramids_built() == built_b + 1
        want = po.make_images(irr, levels)
        for l in range(levels):
            assert got[l].tobytes() == ref[l].tobytes() == want[l].tobytes(), l
        assert np.array_equal(counts_a, counts_b) and counts_a.sum() == len(pts)
        assert ra.fs_get_immature().tobytes() == rb.fs_get_immature().tobytes()
    A.close(); B.close()
    ra.L.ref_fs_release_new_frames()
