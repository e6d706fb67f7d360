"""GpuBackend::undistortFrame under the reference's threading: the tracking thread undistorts a frame and then asks for its pyramid (pyramidOf, what
trackNewCoarse does first), while the mapping thread's optimize() runs releasePyramids().  The frame is in no window yet and no consumer holds its pyramid,
so a release that falls between the two calls must leave it alone: the pyramid the consumer gets is the undistorted one, never one rebuilt from
fh->dIp[0] - which these frames fill with another image, so that a rebuild shows."""
import ctypes as C
import threading

import numpy as np
import pytest

import undistort_common as uc
from ldso_amd import synth
from oracle import pyoracle as po
from oracle import pyref as pr
from test_undistort_adapter_gpu import p, undistort_frame

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not (pr.available() and pr.adapter_available()), reason="oracle/_ref/libldso_ref.so / adapter/_build/libldso_adapter_test.so not built")]

N_FRAMES = 24


def level0(A, fh, w, h):
    out = np.zeros((h, w, 3), np.float32)
    A._chk(A.A.adp_get_pyramid_level(A.h, fh, C.c_int(0), p(out)))
    return out


def test_release_between_undistort_and_first_consumer_keeps_the_pyramid():
    win = synth.make_config("tiny", extra_frames=1)
    h, w = win.images[0][0].shape[:2]
    w_org, h_org = w + 17, h + 9
    rx, ry = uc.synthetic_tables(w_org, h_org, w, h, seed=21)
    f8, _ = uc.textured_frames(w_org, h_org, seed=22)
    irr = uc.undistort(f8, rx, ry, w_org, h_org, w, h, factor=0.5)
    want = po.make_images(irr, 1)[0]
    other = po.make_images(np.full((h, w), 7.0, np.float32), 1)[0]          # what fh->dIp[0] holds: a rebuild from it is not `want`
    r_map, r_frames = pr.RefWindow(win), pr.RefWindow(win)                   # the mapper's window; the graph the new frames hang on
    A = pr.GpuAdapter(max_frames=win.F + 1, max_points=win.P + 16)
    A.A.adp_frame_id.restype = C.c_long
    A._chk(A.A.adp_set_undistortion(A.h, C.c_int(w_org), C.c_int(h_org), p(rx), p(ry), None, C.c_int(0), None, C.c_int(2), C.c_int(1)))
    T = win.truth["w2c"][win.F]
    fhs = [r_frames.fs_new_frame(other, T, 0.0, 0.0) for _ in range(N_FRAMES + 1)]
    ids = [A.A.adp_frame_id(fh) for fh in fhs]
    assert len(set(ids)) == len(ids)

    # in sequence: undistort, a whole optimize() of the mapper (it ends in releasePyramids), then the consumer
    undistort_frame(A, ids[0], f8, 1.0, 0.5)
    built = A.pyramids_built()
    A.optimize(r_map, 1)
    built_by_window = A.pyramids_built() - built          # the window's own frames, first call
    assert level0(A, fhs[0], w, h).tobytes() == want.tobytes()
    assert A.pyramids_built() == built + built_by_window

    # two threads: the tracking side undistorts and consumes frame after frame, the mapper optimises (and releases) beside it until that is done
    out = {"err": [], "wrong": [], "rounds": 0}
    done = threading.Event()

    def tracker():
        try:
            for fh, fid in zip(fhs[1:], ids[1:]):
                undistort_frame(A, fid, f8, 1.0, 0.5)
                if level0(A, fh, w, h).tobytes() != want.tobytes():
                    out["wrong"].append(fid)
        except BaseException as e:                      # noqa: B036 - reported by the main thread
            out["err"].append(("tracker", repr(e)))
        finally:
            done.set()

    def mapper():
        try:
            while not done.is_set() or out["rounds"] < 3:
                A.optimize(r_map, 1)
                out["rounds"] += 1
        except BaseException as e:                      # noqa: B036
            out["err"].append(("mapper", repr(e)))

    tb, ta = threading.Thread(target=tracker), threading.Thread(target=mapper)
    ta.start(); tb.start(); tb.join(120); ta.join(120)
    assert not ta.is_alive() and not tb.is_alive(), "a thread hangs"
    assert not out["err"], out["err"]
    assert not out["wrong"], ("frames whose pyramid was rebuilt from fh->dIp[0]", out["wrong"])
    assert out["rounds"] >= 3
    # every frame's pyramid was built once, by undistortFrame
    assert A.pyramids_built() == built + built_by_window + N_FRAMES
    A.close()
    r_map.L.ref_fs_release_new_frames()
