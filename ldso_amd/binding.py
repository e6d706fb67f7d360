"""ctypes binding of libldso_hip.so — the product path.  Every call goes through the C-ABI declared in
include/ldso_hip.h; there is NO CPU fallback: if the HIP library is missing or no GPU is visible the
constructors raise."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import synth

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


E_NONFINITE = -3          # LDSO_E_NONFINITE (ldso_hip.h)
E_INVALID = -1            # LDSO_E_INVALID
E_UNSUPPORTED = -4        # LDSO_E_UNSUPPORTED
MAX_FRAMES = 16           # LDSO_MAX_FRAMES (ldso_window.h)


class LdsoError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"ldso_hip error {code}: {msg}")
        self.code = code


def lib_path() -> str:
    # LDSO_HIP_LIB: an alternative build of the same library (kernel experiments: scripts/build_variant.sh), never a CPU substitute
    return os.environ.get("LDSO_HIP_LIB") or os.path.join(_HERE, "libldso_hip.so")


def lib():
    global _LIB
    if _LIB is None:
        p = lib_path()
        if not os.path.exists(p):
            raise RuntimeError(f"{p} is missing: build it with `python -m ldso_amd.build` (hipcc, gfx950). There is no CPU fallback.")
        # PyTorch-ROCm wheels bundle their own libamdhip64/libhsa-runtime64 (same SONAMEs as /opt/rocm).  Two HIP
        # runtimes in one process cannot both own the GPU, so when torch is part of the process (streams, RCCL) it
        # must be loaded first; libldso_hip.so then binds to the runtime that is already resident.
        try:
            import torch  # noqa: F401
        except Exception:
            pass
        L = C.CDLL(p)
        L.ldso_last_error.restype = C.c_char_p
        L.ldso_ba_reduce_doubles.restype = C.c_size_t
        L.ldso_ba_gn_reduce_doubles.restype = C.c_size_t
        _LIB = L
    return _LIB


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _chk(code):
    if code != 0:
        raise LdsoError(code, lib().ldso_last_error().decode())


def default_settings() -> np.ndarray:
    s = np.zeros((), synth.SETTINGS_DTYPE)
    _chk(lib().ldso_settings_default(_p(s)))
    return s


def arrival_targets(total) -> np.ndarray:
    """how many of `total` reduce workgroups of a fused reduce + control-step launch arrive on each arrival word (ldso_ba_arrival_targets)"""
    t = np.full(64, -1, np.int32)
    n = lib().ldso_ba_arrival_targets(C.c_int(int(total)), _p(t))
    if n < 0:
        _chk(n)
    return t[:n].copy()


def arrival_shard(q) -> int:
    """the arrival word of reduce workgroup q (dispatch index behind the control workgroups; ldso_ba_arrival_shard)"""
    s = lib().ldso_ba_arrival_shard(C.c_int(int(q)))
    if s < 0:
        _chk(s)
    return s


def act_update_min_dist(current, n_points, desired_density) -> float:
    """the density controller of FullSystem::activatePointsMT (FullSystem.cc:1054-1073) on currentMinActDist"""
    out = C.c_float()
    _chk(lib().ldso_act_update_min_dist(C.c_float(current), C.c_int(n_points), C.c_float(desired_density), C.byref(out)))
    return out.value


class Pyramid:
    """FrameHessian::dIp of one frame resident in HBM (ldso_pyramid_t), shared zero-copy by Tracker / Tracer / BA."""

    def __init__(self, w, h, levels, device=0):
        self.L = lib()
        self.h = C.c_void_p()
        _chk(self.L.ldso_pyr_create(C.c_int(device), C.c_int(w), C.c_int(h), C.c_int(levels), C.byref(self.h)))
        self.w, self.hh, self.levels = w, h, levels

    def close(self):
        if self.h:
            self.L.ldso_pyr_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def make_images(self, irradiance, stream=None):
        a = np.ascontiguousarray(irradiance, np.float32)
        assert a.size == self.w * self.hh
        _chk(self.L.ldso_pyr_make_images(self.h, _p(a), C.c_void_p(stream)))
        return self

    def level_ptr(self, lvl):
        ptr, wl, hl = C.c_void_p(), C.c_int(), C.c_int()
        _chk(self.L.ldso_pyr_level(self.h, C.c_int(lvl), C.byref(ptr), C.byref(wl), C.byref(hl)))
        return ptr.value, wl.value, hl.value

    def get_level(self, lvl):
        out = np.zeros((self.hh >> lvl, self.w >> lvl, 3), np.float32)
        _chk(self.L.ldso_pyr_get_level(self.h, C.c_int(lvl), _p(out)))
        return out


class Features:
    """Corner features and immature points of a new key frame (ldso_features_t): FeatureDetector::DetectCorners + the ImmaturePoint constructors."""

    def __init__(self, w, h, max_features, orb_pattern=None, device=0):
        self.L = lib()
        self.h = C.c_void_p()
        pat = None if orb_pattern is None else np.ascontiguousarray(orb_pattern, np.int32)
        assert pat is None or pat.size == 1024
        _chk(self.L.ldso_feat_create(C.c_int(device), C.c_int(w), C.c_int(h), C.c_int(max_features), _p(pat), C.byref(self.h)))
        self.w, self.hh, self.n, self.n_corners = w, h, 0, 0

    def close(self):
        if self.h:
            self.L.ldso_feat_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def grid(w, h, n):
        """the grid rule of FeatureDetector.cc:37-42 (host only)"""
        v = [C.c_int() for _ in range(6)]
        _chk(lib().ldso_feat_grid(C.c_int(w), C.c_int(h), C.c_int(n), *[C.byref(x) for x in v]))
        return dict(zip(("gridsize", "gridX", "gridY", "skip", "per_cell", "capacity"), (x.value for x in v)))

    def set_stream(self, stream_ptr):
        _chk(self.L.ldso_feat_set_stream(self.h, C.c_void_p(stream_ptr)))

    def set_response(self, B):
        b = None if B is None else np.ascontiguousarray(B, np.float32)
        assert b is None or b.size == 256
        _chk(self.L.ldso_feat_set_response(self.h, _p(b)))

    def detect(self, pyr: "Pyramid", n_features, host_index=0):
        """(features, corners) found; raises LdsoError (code E_NONFINITE: the results can still be fetched)"""
        n, nc = C.c_int(), C.c_int()
        code = self.L.ldso_feat_detect(self.h, pyr.h, C.c_int(n_features), C.c_int(host_index), C.byref(n), C.byref(nc))
        if code in (0, E_NONFINITE):
            self.n, self.n_corners = n.value, nc.value
        _chk(code)
        return self.n, self.n_corners

    def get(self):
        f = np.zeros(self.n, synth.FEATURE_DTYPE)
        q = np.zeros(self.n, synth.IMMATURE_DTYPE)
        _chk(self.L.ldso_feat_get(self.h, _p(f), _p(q)))
        return f, q

    def device_ptrs(self):
        a, b, n = C.c_void_p(), C.c_void_p(), C.c_int()
        _chk(self.L.ldso_feat_device(self.h, C.byref(a), C.byref(b), C.byref(n)))
        return a.value, b.value, n.value

    def profile(self, enable=True):
        us = np.zeros(4, np.float32)
        _chk(self.L.ldso_feat_profile(self.h, C.c_int(1 if enable else 0), _p(us)))
        return us


class PixelSelector:
    """DSO's gradient pixels of a new key frame (ldso_pixsel_t): PixelSelector::makeMaps + the raster scan and ImmaturePoint constructors of makeNewTraces."""

    def __init__(self, w, h, random_pattern, device=0):
        self.L = lib()
        self.h = C.c_void_p()
        rp = np.ascontiguousarray(random_pattern, np.uint8)
        assert rp.size == w * h
        _chk(self.L.ldso_pixsel_create(C.c_int(device), C.c_int(w), C.c_int(h), _p(rp), C.byref(self.h)))
        self.w, self.hh, self.n = w, h, 0

    def close(self):
        if self.h:
            self.L.ldso_pixsel_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def supported(w, h):
        """host only: the return code of ldso_pixsel_supported (0, or E_UNSUPPORTED for sizes that are no multiples of 32)"""
        return lib().ldso_pixsel_supported(C.c_int(w), C.c_int(h))

    @staticmethod
    def plan(counts, density, potential, recursions_left):
        """host only: (action, new_potential, char_th) of makeMaps :125-153"""
        c = np.ascontiguousarray(counts, np.int32)
        v = [C.c_int() for _ in range(3)]
        _chk(lib().ldso_pixsel_plan(_p(c), C.c_float(density), C.c_int(potential), C.c_int(recursions_left), *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def set_stream(self, stream_ptr):
        _chk(self.L.ldso_pixsel_set_stream(self.h, C.c_void_p(stream_ptr)))

    def set_response(self, B):
        b = None if B is None else np.ascontiguousarray(B, np.float32)
        assert b is None or b.size == 256
        _chk(self.L.ldso_pixsel_set_response(self.h, _p(b)))

    def set_settings(self, min_grad_hist_cut=0.5, min_grad_hist_add=7.0, grad_downweight_per_level=0.75, select_direction_distribution=True):
        _chk(self.L.ldso_pixsel_set_settings(self.h, C.c_float(min_grad_hist_cut), C.c_float(min_grad_hist_add), C.c_float(grad_downweight_per_level),
                                             C.c_int(1 if select_direction_distribution else 0)))

    @property
    def potential(self):
        v = C.c_int()
        _chk(self.L.ldso_pixsel_get_potential(self.h, C.byref(v)))
        return v.value

    @potential.setter
    def potential(self, value):
        _chk(self.L.ldso_pixsel_set_potential(self.h, C.c_int(value)))

    def make_maps(self, pyr: "Pyramid", density, recursions_left=1, th_factor=1.0):
        """(return value of makeMaps, (n2, n3, n4), potential used); raises LdsoError (E_NONFINITE: the results can still be fetched)"""
        n, used = C.c_int(), C.c_int()
        counts = np.zeros(3, np.int32)
        _chk(self.L.ldso_pixsel_make_maps(self.h, pyr.h, C.c_float(density), C.c_int(recursions_left), C.c_float(th_factor), C.byref(n), _p(counts), C.byref(used)))
        return n.value, tuple(int(c) for c in counts), used.value

    def get_map(self):
        m = np.zeros((self.hh, self.w), np.float32)
        _chk(self.L.ldso_pixsel_get_map(self.h, _p(m)))
        return m

    def get_thresholds(self):
        a, b = np.zeros((self.hh // 32, self.w // 32), np.float32), np.zeros((self.hh // 32, self.w // 32), np.float32)
        _chk(self.L.ldso_pixsel_get_thresholds(self.h, _p(a), _p(b)))
        return a, b

    def make_points(self, pyr: "Pyramid", host_index=0):
        n = C.c_int()
        code = self.L.ldso_pixsel_make_points(self.h, pyr.h, C.c_int(host_index), C.byref(n))
        if code in (0, E_NONFINITE):
            self.n = n.value
        _chk(code)
        return self.n

    def get_points(self):
        q, t = np.zeros(self.n, synth.IMMATURE_DTYPE), np.zeros(self.n, np.float32)
        _chk(self.L.ldso_pixsel_get_points(self.h, _p(q), _p(t)))
        return q, t

    def device_ptrs(self):
        a, b, n = C.c_void_p(), C.c_void_p(), C.c_int()
        _chk(self.L.ldso_pixsel_device(self.h, C.byref(a), C.byref(b), C.byref(n)))
        return a.value, b.value, n.value

    def profile(self, enable=True):
        us = np.zeros(5, np.float32)
        _chk(self.L.ldso_pixsel_profile(self.h, C.c_int(1 if enable else 0), _p(us)))
        return us


class Undistorter:
    """Undistort::undistort<T> on the device (ldso_undistorter_t): raw 8- / 16-bit frame in, irradiance into a Pyramid (or the handle's own buffer)."""

    def __init__(self, w_org, h_org, w, h, device=0):
        self.L = lib()
        self.h = C.c_void_p()
        _chk(self.L.ldso_undist_create(C.c_int(device), C.c_int(w_org), C.c_int(h_org), C.c_int(w), C.c_int(h), C.byref(self.h)))
        self.w_org, self.h_org, self.w, self.hh = w_org, h_org, w, h

    def close(self):
        if self.h:
            self.L.ldso_undist_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_ptr):
        _chk(self.L.ldso_undist_set_stream(self.h, C.c_void_p(stream_ptr)))

    def set_remap(self, remap_x, remap_y):
        """both None: passthrough"""
        x = None if remap_x is None else np.ascontiguousarray(remap_x, np.float32)
        y = None if remap_y is None else np.ascontiguousarray(remap_y, np.float32)
        assert all(a is None or a.size == self.w * self.hh for a in (x, y))
        _chk(self.L.ldso_undist_set_remap(self.h, _p(x), _p(y)))

    def set_photometric(self, G, vignette_inv, photometric_calibration=2, use_exposure=True):
        """G None: no valid calibration"""
        g = None if G is None else np.ascontiguousarray(G, np.float32)
        v = None if vignette_inv is None else np.ascontiguousarray(vignette_inv, np.float32)
        assert v is None or v.size == self.w_org * self.h_org
        _chk(self.L.ldso_undist_set_photometric(self.h, _p(g), C.c_int(0 if g is None else g.size), _p(v), C.c_int(photometric_calibration), C.c_int(1 if use_exposure else 0)))

    def frame(self, raw, exposure=1.0, factor=1.0, pyr: "Pyramid" = None):
        """raw: uint8 or uint16 image of the original size -> the exposure the reference would return"""
        r = np.ascontiguousarray(raw)
        assert r.dtype in (np.uint8, np.uint16) and r.size == self.w_org * self.h_org
        e = C.c_float()
        _chk(self.L.ldso_undist_frame(self.h, _p(r), C.c_int(r.dtype.itemsize), C.c_float(exposure), C.c_float(factor), pyr.h if pyr is not None else None, C.byref(e)))
        return e.value

    def get(self):
        out = np.zeros((self.hh, self.w), np.float32)
        _chk(self.L.ldso_undist_get(self.h, _p(out)))
        return out

    def device_ptr(self):
        p = C.c_void_p()
        _chk(self.L.ldso_undist_device(self.h, C.byref(p)))
        return p.value

    def profile(self, enable=True):
        """microseconds of the last profiled frame: copy, undistortion kernel, pyramid build"""
        us = np.zeros(3, np.float32)
        _chk(self.L.ldso_undist_profile(self.h, C.c_int(1 if enable else 0), _p(us)))
        return us


class BA:
    """Windowed bundle adjustment handle (EnergyFunctional + FullSystem::optimize slice) on one GPU."""

    def __init__(self, w, h, max_frames, max_points, device=0, stream=None):
        self.L = lib()
        self.h = C.c_void_p()
        _chk(self.L.ldso_ba_create(C.c_int(device), C.c_int(w), C.c_int(h), C.c_int(max_frames), C.c_int(max_points), C.byref(self.h)))
        self.w, self.hh = w, h
        self.F = self.P = self.R = 0
        if stream is not None:
            self.set_stream(stream)

    @classmethod
    def from_window(cls, win: synth.Window, device=0, stream=None, max_frames=None, max_points=None):
        ba = cls(win.w, win.h, max_frames or max(win.F, 2), max_points or win.P, device=device, stream=stream)
        ba.load_window(win)
        return ba

    def close(self):
        if self.h:
            self.L.ldso_ba_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_ptr: int):
        """Run the handle on a caller's HIP stream.  The legacy default stream (handle 0, what torch.cuda.current_stream() is
        unless a torch.cuda.Stream was made current) cannot be passed through the C-ABI (NULL = "own stream") and would not
        order against the handle's own non-blocking stream: refuse it instead of racing silently."""
        if not stream_ptr:
            raise ValueError("pass a non-default HIP stream (e.g. s = torch.cuda.Stream(); torch.cuda.set_stream(s); s.cuda_stream)")
        _chk(self.L.ldso_ba_set_stream(self.h, C.c_void_p(stream_ptr)))

    def set_settings(self, s):
        s = np.ascontiguousarray(s)
        _chk(self.L.ldso_ba_set_settings(self.h, _p(s)))

    def set_image(self, slot, dI0):
        a = np.ascontiguousarray(dI0, np.float32)
        _chk(self.L.ldso_ba_set_image(self.h, C.c_int(slot), _p(a)))

    def set_image_raw(self, slot, irradiance):
        a = np.ascontiguousarray(irradiance, np.float32)
        _chk(self.L.ldso_ba_set_image_raw(self.h, C.c_int(slot), _p(a)))

    def set_image_pyramid(self, slot, pyr: "Pyramid"):
        _chk(self.L.ldso_ba_set_image_pyramid(self.h, C.c_int(slot), pyr.h))
        self._pyramids = getattr(self, "_pyramids", {}); self._pyramids[slot] = pyr          # keep it alive while the slot refers to it

    def get_image(self, slot):
        out = np.zeros((self.hh, self.w, 3), np.float32)
        _chk(self.L.ldso_ba_get_image(self.h, C.c_int(slot), _p(out)))
        return out

    def set_window(self, image_slots, points, residuals, lin_J=None, lin_rtz=None):
        sl = np.ascontiguousarray(image_slots, np.int32)
        pts = np.ascontiguousarray(points)
        res = np.ascontiguousarray(residuals)
        J = np.ascontiguousarray(lin_J) if lin_J is not None else None
        rt = np.ascontiguousarray(lin_rtz, np.float32) if lin_rtz is not None else None
        self.F, self.P, self.R = len(sl), len(pts), len(res)
        _chk(self.L.ldso_ba_set_window(self.h, C.c_int(self.F), _p(sl), C.c_int(self.P), _p(pts), C.c_int(self.R), _p(res), _p(J), _p(rt)))

    def set_point_stats(self, max_rel_baseline, num_good_residuals):
        a = np.ascontiguousarray(max_rel_baseline, np.float32); b = np.ascontiguousarray(num_good_residuals, np.int32)
        assert len(a) == len(b) == self.P
        _chk(self.L.ldso_ba_set_point_stats(self.h, _p(a), _p(b)))

    def update_window(self, image_slots, frame_from, point_from, res_mask, fresh=None, fresh_res=None, fresh_mrb=None, fresh_ngr=None):
        """ldso_ba_update_window: the next window as a delta against the resident one (include/ldso_hip.h)."""
        sl = np.ascontiguousarray(image_slots, np.int32); ff = np.ascontiguousarray(frame_from, np.int32)
        pf = np.ascontiguousarray(point_from, np.int32); mk = np.ascontiguousarray(res_mask, np.uint32)
        assert len(sl) == len(ff) and len(pf) == len(mk)
        nf = 0 if fresh is None else len(fresh); nr = 0 if fresh_res is None else len(fresh_res)
        fp = np.ascontiguousarray(fresh) if nf else None; fr = np.ascontiguousarray(fresh_res) if nr else None
        fm = np.ascontiguousarray(fresh_mrb, np.float32) if nf else None; fg = np.ascontiguousarray(fresh_ngr, np.int32) if nf else None
        _chk(self.L.ldso_ba_update_window(self.h, C.c_int(len(sl)), _p(sl), _p(ff), C.c_int(len(pf)), _p(pf), _p(mk), C.c_int(nf), _p(fp), C.c_int(nr), _p(fr), _p(fm), _p(fg)))
        self._sync_dims()

    # ---- the same delta call by call (ldso_ba_window_begin .. ldso_ba_window_commit) ----
    def window_begin(self):
        _chk(self.L.ldso_ba_window_begin(self.h))

    def remove_frame(self, frame_idx):
        _chk(self.L.ldso_ba_remove_frame(self.h, C.c_int(frame_idx)))

    def insert_frame(self, image_slot) -> int:
        fid = C.c_int()
        _chk(self.L.ldso_ba_insert_frame(self.h, C.c_int(image_slot), C.byref(fid)))
        return fid.value

    def remove_points(self, rows):
        a = np.ascontiguousarray(rows, np.int32)
        _chk(self.L.ldso_ba_remove_points(self.h, C.c_int(len(a)), _p(a)))

    def drop_residuals(self, rows, targets):
        a = np.ascontiguousarray(rows, np.int32); b = np.ascontiguousarray(targets, np.int32)
        _chk(self.L.ldso_ba_drop_residuals(self.h, C.c_int(len(a)), _p(a), _p(b)))

    def add_residuals(self, rows, targets):
        a = np.ascontiguousarray(rows, np.int32); b = np.ascontiguousarray(targets, np.int32)
        _chk(self.L.ldso_ba_add_residuals(self.h, C.c_int(len(a)), _p(a), _p(b)))

    def add_points(self, points, before_row, residuals, mrb=None, ngr=None):
        pts = np.ascontiguousarray(points); br = np.ascontiguousarray(before_row, np.int32); res = np.ascontiguousarray(residuals)
        m = np.ascontiguousarray(mrb, np.float32) if mrb is not None else None; g = np.ascontiguousarray(ngr, np.int32) if ngr is not None else None
        _chk(self.L.ldso_ba_add_points(self.h, C.c_int(len(pts)), _p(pts), _p(br), C.c_int(len(res)), _p(res), _p(m), _p(g)))

    def _sync_dims(self):
        """F / P / R as the HANDLE holds them (the getters size their numpy buffers from these: never from what a caller says)"""
        F, P, R = C.c_int(), C.c_int(), C.c_int()
        _chk(self.L.ldso_ba_get_dims(self.h, C.byref(F), C.byref(P), C.byref(R)))
        self.F, self.P, self.R = F.value, P.value, R.value

    def window_commit(self, F=None, P=None, R=None):
        _chk(self.L.ldso_ba_window_commit(self.h))
        self._sync_dims()
        assert (F is None or F == self.F) and (P is None or P == self.P) and (R is None or R == self.R), ((F, P, R), (self.F, self.P, self.R))

    def set_frames(self, frames, calib):
        fr = np.ascontiguousarray(frames)
        c = np.ascontiguousarray(calib)
        _chk(self.L.ldso_ba_set_frames(self.h, _p(fr), _p(c)))

    def set_prior(self, HM, bM):
        HM = np.ascontiguousarray(HM, np.float64) if HM is not None else None
        bM = np.ascontiguousarray(bM, np.float64) if bM is not None else None
        _chk(self.L.ldso_ba_set_prior(self.h, _p(HM), _p(bM)))

    def get_prior(self):
        """the marginalisation prior as the device holds it (ldso_ba_get_prior) -> (HM, bM, has_prior)"""
        n = 8 * self.F + 4
        HM, bM, has = np.zeros((n, n)), np.zeros(n), C.c_int()
        _chk(self.L.ldso_ba_get_prior(self.h, _p(HM), _p(bM), C.byref(has)))
        return HM, bM, bool(has.value)

    def load_window(self, win: synth.Window):
        self.set_settings(win.settings)
        for f in range(win.F):
            self.set_image(f, win.images[f][0])
        self.set_window(np.arange(win.F), win.points, win.residuals, win.lin_J, win.lin_res_toZeroF)
        self.set_frames(win.frames, win.calib)
        if np.any(win.HM) or np.any(win.bM):
            self.set_prior(win.HM, win.bM)

    def set_shard(self, begin, end):
        _chk(self.L.ldso_ba_set_shard(self.h, C.c_int(begin), C.c_int(end)))

    # ---- one-shot peer-write all-reduce (ldso_ba_enqueue_gn_p2p) ----
    def p2p_window_alloc(self, n_ranks, with_ipc_handle=False):
        w = C.c_void_p(); hnd = C.create_string_buffer(64) if with_ipc_handle else None
        _chk(self.L.ldso_ba_p2p_window_alloc(self.h, C.c_int(n_ranks), C.byref(w), hnd))
        return (w.value, hnd.raw) if with_ipc_handle else w.value

    def p2p_window_open(self, ipc_handle: bytes):
        w = C.c_void_p()
        _chk(self.L.ldso_ba_p2p_window_open(self.h, C.c_char_p(ipc_handle), C.byref(w)))
        return w.value

    def p2p_window_close(self, window, opened_from_handle=False):
        _chk(self.L.ldso_ba_p2p_window_close(self.h, C.c_void_p(window), C.c_int(1 if opened_from_handle else 0)))

    def enqueue_gn_p2p(self, rank, n_ranks, windows, first_iteration, iters):
        arr = (C.c_void_p * n_ranks)(*windows)
        _chk(self.L.ldso_ba_enqueue_gn_p2p(self.h, C.c_int(rank), C.c_int(n_ranks), arr, C.c_int(first_iteration), C.c_int(iters)))

    def p2p_check(self):
        _chk(self.L.ldso_ba_p2p_check(self.h))

    def set_chunk_points(self, n):
        _chk(self.L.ldso_ba_set_chunk_points(self.h, C.c_int(n)))

    def set_reduce_splits(self, splits):
        """K-splits per Schur tile of this handle's GN fast path (8; a batch of >= 4 windows uses 4: BABatch.reduce_splits())"""
        _chk(self.L.ldso_ba_set_reduce_splits(self.h, C.c_int(int(splits))))

    def get_chunk_cuts(self):
        """ends of the chunks in force (one past the last point of every chunk)"""
        n = C.c_int()
        _chk(self.L.ldso_ba_get_chunk_cuts(self.h, None, C.c_int(0), C.byref(n)))
        ends = np.zeros(n.value, np.int32)
        _chk(self.L.ldso_ba_get_chunk_cuts(self.h, _p(ends), C.c_int(len(ends)), C.byref(n)))
        return ends

    def set_chunk_cuts(self, ends):
        ends = np.ascontiguousarray(ends, np.int32)
        _chk(self.L.ldso_ba_set_chunk_cuts(self.h, _p(ends) if len(ends) else None, C.c_int(len(ends))))

    def get_chunk_points(self):
        n, w = C.c_int(), C.c_int()
        _chk(self.L.ldso_ba_get_chunk_points(self.h, C.byref(n), C.byref(w)))
        return n.value, w.value

    def reduce_doubles(self) -> int:
        return int(self.L.ldso_ba_reduce_doubles(self.h))

    # --- optimisation slice --------------------------------------------------------------------------
    def collect_active(self):
        _chk(self.L.ldso_ba_collect_active(self.h))

    def linearize_all(self, fix=False) -> float:
        e = C.c_double()
        _chk(self.L.ldso_ba_linearize_all(self.h, C.c_int(1 if fix else 0), C.byref(e)))
        return e.value

    def apply_res(self):
        _chk(self.L.ldso_ba_apply_res(self.h))

    def backup_state(self):
        _chk(self.L.ldso_ba_backup_state(self.h))

    def solve_system(self, iteration, lam=1e-1):
        _chk(self.L.ldso_ba_solve_system(self.h, C.c_int(iteration), C.c_double(lam)))

    def do_step(self) -> bool:
        cb = C.c_int()
        _chk(self.L.ldso_ba_do_step(self.h, C.byref(cb)))
        return bool(cb.value)

    def load_state_backup(self):
        _chk(self.L.ldso_ba_load_state_backup(self.h))

    def optimize(self, niters, force_all=False):
        rm = C.c_float()
        it = C.c_int()
        _chk(self.L.ldso_ba_optimize(self.h, C.c_int(niters), C.c_int(1 if force_all else 0), C.byref(rm), C.byref(it)))
        return rm.value, it.value

    def calc_lm_energies(self):
        m, l = C.c_double(), C.c_double()
        _chk(self.L.ldso_ba_calc_lm_energies(self.h, C.byref(m), C.byref(l)))
        return m.value, l.value

    def marginalize_points(self, flags):
        """EnergyFunctional::marginalizePointsF for the flagged points -> (HM, bM)"""
        flags = np.ascontiguousarray(flags, np.int32)
        assert len(flags) == self.P
        n = 8 * self.F + 4
        HM = np.zeros((n, n)); bM = np.zeros(n)
        _chk(self.L.ldso_ba_marginalize_points(self.h, _p(flags), _p(HM), _p(bM)))
        return HM, bM

    def marginalize_frame(self, idx):
        """EnergyFunctional::marginalizeFrame on the device prior -> (HM, bM) of the window without frame idx"""
        n = 8 * (self.F - 1) + 4
        HM = np.zeros((n, n)); bM = np.zeros(n)
        _chk(self.L.ldso_ba_marginalize_frame(self.h, C.c_int(idx), _p(HM), _p(bM)))
        return HM, bM

    def time_linearize(self, reps=50):
        us = C.c_double()
        _chk(self.L.ldso_ba_time_linearize(self.h, C.c_int(reps), C.byref(us)))
        return us.value

    def get_pair_rt(self):
        out = np.zeros((self.F * self.F, 14), np.float32)
        _chk(self.L.ldso_ba_get_pair_rt(self.h, _p(out)))
        return out

    def activate_points(self, pts, min_obs=1, min_idepth_hessian=100.0, gn_iterations=3):
        """FullSystem::optimizeImmaturePoint for a batch of immature points against the resident window"""
        a = np.ascontiguousarray(pts)
        assert a.dtype == synth.IMMATURE_DTYPE
        out = np.zeros(len(a), synth.ACTIVATION_DTYPE)
        _chk(self.L.ldso_ba_activate_points(self.h, C.c_int(len(a)), _p(a), C.c_int(min_obs), C.c_float(min_idepth_hessian), C.c_int(gn_iterations), _p(out)))
        return out

    def _select_args(self, seeds, pts, my_type, KRKi, Kt, host_flagged, min_act_dist, min_trace_quality):
        sd = np.ascontiguousarray(seeds); a = np.ascontiguousarray(pts)
        assert sd.dtype == synth.ACT_SEED_DTYPE and a.dtype == synth.IMMATURE_DTYPE
        mt = np.ascontiguousarray(my_type, np.float32); K1 = np.ascontiguousarray(KRKi, np.float32).reshape(-1, 9); K2 = np.ascontiguousarray(Kt, np.float32).reshape(-1, 3)
        fl = np.ascontiguousarray(host_flagged, np.int32)
        assert len(mt) == len(a) and len(K1) == len(K2) == len(fl)
        keep = (sd, a, mt, K1, K2, fl)
        return keep, (C.c_int(len(sd)), _p(sd), C.c_int(len(a)), _p(a), _p(mt), C.c_int(len(fl)), _p(K1), _p(K2), _p(fl), C.c_float(min_act_dist), C.c_float(min_trace_quality))

    def select_candidates(self, seeds, pts, my_type, KRKi, Kt, host_flagged, min_act_dist, min_trace_quality=3.0):
        """distance map + candidate selection of FullSystem::activatePointsMT -> (decision [n] LDSO_ACT_*, selected indices in order)"""
        keep, args = self._select_args(seeds, pts, my_type, KRKi, Kt, host_flagged, min_act_dist, min_trace_quality)
        n = len(keep[1])
        dec = np.zeros(n, np.int32); sel = np.zeros(n, np.int32); ns = C.c_int()
        _chk(self.L.ldso_ba_select_candidates(self.h, *args, _p(dec), _p(sel), C.byref(ns)))
        return dec, sel[:ns.value].copy()

    def select_activate_points(self, seeds, pts, my_type, KRKi, Kt, host_flagged, min_act_dist, min_trace_quality=3.0, min_obs=1, min_idepth_hessian=100.0, gn_iterations=3):
        """the selection and ldso_ba_activate_points on the selected list in one enqueue -> (decision, selected, activation records of the selected)"""
        keep, args = self._select_args(seeds, pts, my_type, KRKi, Kt, host_flagged, min_act_dist, min_trace_quality)
        n = len(keep[1])
        dec = np.zeros(n, np.int32); sel = np.zeros(n, np.int32); ns = C.c_int(); out = np.zeros(n, synth.ACTIVATION_DTYPE)
        _chk(self.L.ldso_ba_select_activate_points(self.h, *args, C.c_int(min_obs), C.c_float(min_idepth_hessian), C.c_int(gn_iterations), _p(dec), _p(sel), C.byref(ns), _p(out)))
        return dec, sel[:ns.value].copy(), out[:ns.value].copy()

    def select_activate_tracer(self, tracer: "Tracer", KRKi, Kt, host_flagged, min_act_dist, min_trace_quality=3.0, min_obs=1, min_idepth_hessian=100.0, gn_iterations=3, compact=True):
        """select_activate_points with the tracer's resident records and types as candidates and the resident window's points as seeds; compact: whatever the loop
        did not KEEP leaves the tracer's set -> (decision, selected, activation records of the selected)"""
        K1 = np.ascontiguousarray(KRKi, np.float32).reshape(-1, 9); K2 = np.ascontiguousarray(Kt, np.float32).reshape(-1, 3); fl = np.ascontiguousarray(host_flagged, np.int32)
        assert len(K1) == len(K2) == len(fl)
        n = tracer.n
        dec = np.zeros(n, np.int32); sel = np.zeros(n, np.int32); ns = C.c_int(); left = C.c_int(n); out = np.zeros(n, synth.ACTIVATION_DTYPE)
        _chk(self.L.ldso_ba_select_activate_tracer(self.h, tracer.h, C.c_int(len(fl)), _p(K1), _p(K2), _p(fl), C.c_float(min_act_dist), C.c_float(min_trace_quality), C.c_int(min_obs),
                                                   C.c_float(min_idepth_hessian), C.c_int(gn_iterations), C.c_int(1 if compact else 0), _p(dec), _p(sel), C.byref(ns), _p(out), C.byref(left)))
        tracer.n = left.value
        return dec, sel[:ns.value].copy(), out[:ns.value].copy()

    def get_distance_map(self):
        """CoarseDistanceMap::fwdWarpedIDDistFinal as the last selection left it: [h >> 1, w >> 1] floats, 0..39 and 1000"""
        out = np.zeros((self.hh >> 1, self.w >> 1), np.float32)
        _chk(self.L.ldso_ba_get_distance_map(self.h, _p(out)))
        return out

    def enqueue_gn(self, first_iteration, iters):
        _chk(self.L.ldso_ba_enqueue_gn(self.h, C.c_int(first_iteration), C.c_int(iters)))

    def sync(self):
        _chk(self.L.ldso_ba_sync(self.h))

    def gn_reduce_doubles(self):
        return int(self.L.ldso_ba_gn_reduce_doubles(self.h))

    def gn_reduce_local(self, buf_ptr: int, lam=1e-1):
        _chk(self.L.ldso_ba_gn_reduce_local(self.h, C.c_void_p(buf_ptr), C.c_double(lam)))

    def gn_solve_reduced(self, buf_ptr: int, iteration, lam=1e-1):
        _chk(self.L.ldso_ba_gn_solve_reduced(self.h, C.c_void_p(buf_ptr), C.c_int(iteration), C.c_double(lam)))

    def enqueue_gn_rccl(self, comm_ptr: int, first_iteration, iters):
        _chk(self.L.ldso_ba_enqueue_gn_rccl(self.h, C.c_void_p(comm_ptr), C.c_int(first_iteration), C.c_int(iters)))

    def reduce_local(self, buf_ptr: int):
        _chk(self.L.ldso_ba_reduce_local(self.h, C.c_void_p(buf_ptr)))

    def solve_reduced(self, buf_ptr: int, iteration, lam=1e-1, do_step=True):
        _chk(self.L.ldso_ba_solve_reduced(self.h, C.c_void_p(buf_ptr), C.c_int(iteration), C.c_double(lam), C.c_int(1 if do_step else 0)))

    # --- results ----------------------------------------------------------------------------------------
    def get_residuals(self):
        out = np.zeros(self.R, synth.RES_OUT_DTYPE)
        st = np.zeros(self.R, np.int32)
        act = np.zeros(self.R, np.int32)
        rem = np.zeros(self.R, np.int32)
        _chk(self.L.ldso_ba_get_residuals(self.h, _p(out), _p(st), _p(act), _p(rem)))
        return dict(out=out, state_state=st, is_active=act, to_remove=rem)

    def get_points(self):
        out = np.zeros(self.P, synth.POINT_OUT_DTYPE)
        _chk(self.L.ldso_ba_get_points(self.h, _p(out)))
        return out

    def get_frames(self):
        fr = np.zeros(self.F, synth.FRAME_DTYPE)
        step = np.zeros((self.F, 10))
        cv, cs = np.zeros(4), np.zeros(4)
        pre = np.zeros((self.F, 12))
        _chk(self.L.ldso_ba_get_frames(self.h, _p(fr), _p(step), _p(cv), _p(cs), _p(pre)))
        return dict(frames=fr, step=step, calib_value=cv, calib_step=cs, pre_worldToCam=pre)

    def get_results(self):
        """ldso_ba_get_results: residuals + points + frames behind one synchronisation; the same records as the three getters."""
        out = np.zeros(self.R, synth.RES_OUT_DTYPE); st = np.zeros(self.R, np.int32); act = np.zeros(self.R, np.int32); rem = np.zeros(self.R, np.int32)
        pts = np.zeros(self.P, synth.POINT_OUT_DTYPE)
        fr = np.zeros(self.F, synth.FRAME_DTYPE); step = np.zeros((self.F, 10)); cv, cs = np.zeros(4), np.zeros(4)
        _chk(self.L.ldso_ba_get_results(self.h, _p(out), _p(st), _p(act), _p(rem), _p(pts), _p(fr), _p(step), _p(cv), _p(cs)))
        return dict(residuals=dict(out=out, state_state=st, is_active=act, to_remove=rem), points=pts, frames=dict(frames=fr, step=step, calib_value=cv, calib_step=cs))

    def get_system(self):
        n = 8 * self.F + 4
        d = {k: np.zeros((n, n)) for k in ("HA", "HL", "Hsc", "HFinal")}
        d.update({k: np.zeros(n) for k in ("bA", "bL", "bsc", "bFinal", "x")})
        _chk(self.L.ldso_ba_get_system(self.h, _p(d["HA"]), _p(d["bA"]), _p(d["HL"]), _p(d["bL"]), _p(d["Hsc"]), _p(d["bsc"]),
                                       _p(d["HFinal"]), _p(d["bFinal"]), _p(d["x"])))
        return d

    def get_jacobians(self, ids=None):
        ids = np.arange(self.R, dtype=np.int32) if ids is None else np.ascontiguousarray(ids, np.int32)
        out = np.zeros(len(ids), synth.RAWJAC_DTYPE)
        _chk(self.L.ldso_ba_get_jacobians(self.h, _p(ids), C.c_int(len(ids)), _p(out)))
        return out

    def set_debug_dump(self, enable=True):
        _chk(self.L.ldso_ba_set_debug_dump(self.h, C.c_int(1 if enable else 0)))

    def set_debug_split_launch(self, enable=True):
        _chk(self.L.ldso_ba_set_debug_split_launch(self.h, C.c_int(1 if enable else 0)))

    def get_arrival_words(self):
        """the arrival words of the fused reduce + control-step launch behind a synchronisation (all zero between launches); raises LdsoError (E_NONFINITE)
        when the non-finite status of the iteration is set - also the end of a control-workgroup wait that ran out of polls"""
        words = np.full(64, -1, np.int32)
        n = self.L.ldso_ba_get_arrival_words(self.h, _p(words))
        if n < 0:
            _chk(n)
        return words[:n].copy()

    def get_precalc(self):
        out = np.zeros((self.F, self.F, 27), np.float32)
        _chk(self.L.ldso_ba_get_precalc(self.h, _p(out)))
        return out

    def get_counts(self):
        a, l = C.c_int(), C.c_int()
        _chk(self.L.ldso_ba_get_counts(self.h, C.byref(a), C.byref(l)))
        return a.value, l.value

    def get_energy_log(self):
        buf = np.zeros(64)
        n = self.L.ldso_ba_get_energy_log(self.h, _p(buf), C.c_int(64))
        self._dbg = buf[40:56].copy()
        return buf[:n].copy()

    def profile(self, enable=True):
        _chk(self.L.ldso_ba_profile(self.h, C.c_int(1 if enable else 0)))

    def kernel_time_ms(self, which):
        ms = C.c_double()
        n = C.c_int()
        _chk(self.L.ldso_ba_kernel_time_ms(self.h, C.c_int(which), C.byref(ms), C.byref(n)))
        return ms.value, n.value


class ActJob(C.Structure):
    """ldso_act_job_t (ldso_hip.h): one window's share of a batched selection"""
    _fields_ = [("n_seeds", C.c_int), ("seeds", C.c_void_p), ("n", C.c_int), ("points", C.c_void_p), ("my_type", C.c_void_p), ("n_hosts", C.c_int), ("KRKi", C.c_void_p),
                ("Kt", C.c_void_p), ("host_flagged", C.c_void_p), ("currentMinActDist", C.c_float), ("decision_out", C.c_void_p), ("selected_out", C.c_void_p),
                ("n_selected", C.c_int), ("out", C.c_void_p)]


class ActTracerJob(C.Structure):
    """ldso_act_tracer_job_t (ldso_hip.h): one window's share of ldso_ba_batch_select_activate_tracers"""
    _fields_ = [("tracer", C.c_void_p), ("n_hosts", C.c_int), ("KRKi", C.c_void_p), ("Kt", C.c_void_p), ("host_flagged", C.c_void_p), ("currentMinActDist", C.c_float),
                ("compact", C.c_int), ("decision_out", C.c_void_p), ("selected_out", C.c_void_p), ("n_selected", C.c_int), ("out", C.c_void_p), ("n_left", C.c_int)]


class WinJob(C.Structure):
    """ldso_win_job_t (ldso_hip.h): one window's share of ldso_ba_batch_update_windows = the arguments of ldso_ba_update_window"""
    _fields_ = [("F", C.c_int), ("image_slot", C.c_void_p), ("frame_from", C.c_void_p), ("P", C.c_int), ("point_from", C.c_void_p), ("res_mask", C.c_void_p),
                ("n_fresh", C.c_int), ("fresh", C.c_void_p), ("n_fresh_res", C.c_int), ("fresh_res", C.c_void_p), ("fresh_mrb", C.c_void_p), ("fresh_ngr", C.c_void_p)]


class FramesJob(C.Structure):
    """ldso_frames_job_t (ldso_hip.h): one window's share of ldso_ba_batch_set_frames"""
    _fields_ = [("frames", C.c_void_p), ("calib", C.c_void_p), ("HM", C.c_void_p), ("bM", C.c_void_p)]


class BABatch:
    """ldso_ba_batch_*: the GN iteration of several independent windows per launch."""

    def __init__(self, handles):
        self.L = lib()
        self.handles = list(handles)
        arr = (C.c_void_p * len(self.handles))(*[h.h for h in self.handles])
        self.h = C.c_void_p()
        _chk(self.L.ldso_ba_batch_create(arr, C.c_int(len(self.handles)), C.byref(self.h)))

    def enqueue_gn(self, first_iteration, iters):
        _chk(self.L.ldso_ba_batch_enqueue_gn(self.h, C.c_int(first_iteration), C.c_int(iters)))

    def optimize(self, niters, force_all=False):
        """FullSystem::optimize(niters) on every window of the batch (ldso_ba_batch_optimize) -> (rmse[n], iterations[n], status[n]).
        A non-finite window is reported in status (LDSO_E_NONFINITE = -3), not raised: the other windows' results stay readable."""
        n = len(self.handles)
        rm, it, st = np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(n, np.int32)
        code = self.L.ldso_ba_batch_optimize(self.h, C.c_int(niters), C.c_int(1 if force_all else 0), _p(rm), _p(it), _p(st))
        if code != E_NONFINITE:
            _chk(code)
        return rm, it, st

    def _marg_out(self, sizes):
        """per window (HM, bM) of the given side, or None, and the two pointer arrays the C entries take"""
        n = len(self.handles)
        out = [None if k is None else (np.zeros((k, k)), np.zeros(k)) for k in sizes]
        PH, Pb = (C.c_void_p * n)(), (C.c_void_p * n)()
        for i, o in enumerate(out):
            if o is not None:
                PH[i], Pb[i] = o[0].ctypes.data, o[1].ctypes.data
        return out, PH, Pb

    def marginalize_points(self, flags_list):
        """EnergyFunctional::marginalizePointsF for every window of the batch (ldso_ba_batch_marginalize_points): flags_list[i] = the P_i flags of window i,
        or None for a window that takes no part -> [(HM, bM) or None]"""
        n = len(self.handles)
        assert len(flags_list) == n
        fl = [None if f is None else np.ascontiguousarray(f, np.int32) for f in flags_list]
        for f, h in zip(fl, self.handles):
            assert f is None or len(f) == h.P
        out, PH, Pb = self._marg_out([None if f is None else 8 * h.F + 4 for f, h in zip(fl, self.handles)])
        PF = (C.c_void_p * n)()
        for i, f in enumerate(fl):
            if f is not None:
                PF[i] = f.ctypes.data
        _chk(self.L.ldso_ba_batch_marginalize_points(self.h, PF, PH, Pb))
        return out

    def marginalize_frame(self, idx_list):
        """EnergyFunctional::marginalizeFrame on the device prior of every window of the batch (ldso_ba_batch_marginalize_frame): idx_list[i] = the frame of
        window i, or None / -1 for a window that takes no part -> [(HM, bM) of the window without that frame, or None]"""
        n = len(self.handles)
        assert len(idx_list) == n
        idx = np.array([-1 if k is None or k < 0 else int(k) for k in idx_list], np.int32)
        out, PH, Pb = self._marg_out([None if k < 0 else 8 * (h.F - 1) + 4 for k, h in zip(idx, self.handles)])
        _chk(self.L.ldso_ba_batch_marginalize_frame(self.h, _p(idx), PH, Pb))
        return out

    def activate_points(self, pts_list, min_obs=1, min_idepth_hessian=100.0, gn_iterations=3):
        """FullSystem::optimizeImmaturePoint against every window of the batch (ldso_ba_batch_activate_points): pts_list[i] = the immature records for window i, or
        None / an empty array for a window that takes no part -> [activation records or None]"""
        n = len(self.handles)
        assert len(pts_list) == n
        pts = [None if a is None or len(a) == 0 else np.ascontiguousarray(a) for a in pts_list]
        out = [None if a is None else np.zeros(len(a), synth.ACTIVATION_DTYPE) for a in pts]
        cnt = np.array([0 if a is None else len(a) for a in pts], np.int32)
        PP, PO = (C.c_void_p * n)(), (C.c_void_p * n)()
        for i, a in enumerate(pts):
            if a is not None:
                assert a.dtype == synth.IMMATURE_DTYPE
                PP[i], PO[i] = a.ctypes.data, out[i].ctypes.data
        _chk(self.L.ldso_ba_batch_activate_points(self.h, _p(cnt), PP, C.c_int(min_obs), C.c_float(min_idepth_hessian), C.c_int(gn_iterations), PO))
        return out

    def _jobs(self, jobs, with_records):
        """the ldso_act_job_t array of a batched selection and the arrays it points into; jobs[i]: a dict with the keys seeds, cand, my_type, KRKi, Kt, flagged,
        min_act_dist, or None for a window that takes no part"""
        n = len(self.handles)
        assert len(jobs) == n
        J = (ActJob * n)()
        keep = []
        for i, job in enumerate(jobs):
            if job is None:
                keep.append(None)
                continue
            sd = np.ascontiguousarray(job["seeds"]); a = np.ascontiguousarray(job["cand"])
            assert sd.dtype == synth.ACT_SEED_DTYPE and a.dtype == synth.IMMATURE_DTYPE
            mt = np.ascontiguousarray(job["my_type"], np.float32)
            K1 = None if job.get("KRKi") is None else np.ascontiguousarray(job["KRKi"], np.float32).reshape(-1, 9)
            K2 = None if job.get("Kt") is None else np.ascontiguousarray(job["Kt"], np.float32).reshape(-1, 3)
            fl = np.ascontiguousarray(job["flagged"], np.int32)
            assert len(mt) == len(a)
            dec = np.zeros(len(a), np.int32); sel = np.zeros(len(a), np.int32); rec = np.zeros(len(a), synth.ACTIVATION_DTYPE) if with_records else None
            keep.append((sd, a, mt, K1, K2, fl, dec, sel, rec))
            j = J[i]
            j.n_seeds, j.seeds, j.n, j.points, j.my_type = len(sd), sd.ctypes.data, len(a), a.ctypes.data, mt.ctypes.data
            j.n_hosts, j.KRKi, j.Kt, j.host_flagged = len(fl), (None if K1 is None else K1.ctypes.data), (None if K2 is None else K2.ctypes.data), fl.ctypes.data
            j.currentMinActDist = float(job["min_act_dist"])
            j.decision_out, j.selected_out, j.out = dec.ctypes.data, sel.ctypes.data, (rec.ctypes.data if with_records else None)
        return J, keep

    def select_candidates(self, jobs, min_trace_quality=3.0):
        """distance map + candidate selection of FullSystem::activatePointsMT for every window of the batch (ldso_ba_batch_select_candidates)
        -> [(decision, selected) or None]; BA.get_distance_map() of a member returns the map the call left for it"""
        J, keep = self._jobs(jobs, False)
        _chk(self.L.ldso_ba_batch_select_candidates(self.h, J, C.c_float(min_trace_quality)))
        return [None if k is None else (k[6], k[7][:J[i].n_selected].copy()) for i, k in enumerate(keep)]

    def select_activate_points(self, jobs, min_trace_quality=3.0, min_obs=1, min_idepth_hessian=100.0, gn_iterations=3):
        """the selection and the activation of the selected candidates for every window of the batch in one enqueue (ldso_ba_batch_select_activate_points)
        -> [(decision, selected, activation records of the selected) or None]"""
        J, keep = self._jobs(jobs, True)
        _chk(self.L.ldso_ba_batch_select_activate_points(self.h, J, C.c_float(min_trace_quality), C.c_int(min_obs), C.c_float(min_idepth_hessian), C.c_int(gn_iterations)))
        return [None if k is None else (k[6], k[7][:J[i].n_selected].copy(), k[8][:J[i].n_selected].copy()) for i, k in enumerate(keep)]

    def _tracer_jobs(self, jobs):
        """the ldso_act_tracer_job_t array of select_activate_tracers and the arrays it points into (per window: tracer, KRKi, Kt, flagged, decision, selected,
        records, or None)"""
        n = len(self.handles)
        assert len(jobs) == n
        J = (ActTracerJob * n)()
        keep = []
        for i, job in enumerate(jobs):
            if job is None:
                keep.append(None)
                continue
            T = job["tracer"]
            K1 = None if job.get("KRKi") is None else np.ascontiguousarray(job["KRKi"], np.float32).reshape(-1, 9)
            K2 = None if job.get("Kt") is None else np.ascontiguousarray(job["Kt"], np.float32).reshape(-1, 3)
            fl = np.ascontiguousarray(job["flagged"], np.int32)
            dec = np.zeros(T.n, np.int32); sel = np.zeros(T.n, np.int32); rec = np.zeros(T.n, synth.ACTIVATION_DTYPE)
            keep.append((T, K1, K2, fl, dec, sel, rec))
            j = J[i]
            j.tracer, j.n_hosts, j.KRKi, j.Kt, j.host_flagged = T.h, len(fl), (None if K1 is None else K1.ctypes.data), (None if K2 is None else K2.ctypes.data), fl.ctypes.data
            j.currentMinActDist, j.compact = float(job["min_act_dist"]), 1 if job.get("compact", True) else 0
            j.decision_out, j.selected_out, j.out, j.n_left = dec.ctypes.data, sel.ctypes.data, rec.ctypes.data, T.n
        return J, keep

    def select_activate_tracers(self, jobs, min_trace_quality=3.0, min_obs=1, min_idepth_hessian=100.0, gn_iterations=3):
        """BA.select_activate_tracer for every window of the batch in one enqueue (ldso_ba_batch_select_activate_tracers).  jobs[i]: a dict with the keys tracer (a Tracer),
        KRKi, Kt, flagged, min_act_dist and optionally compact (default True), or None for a window that takes no part -> [(decision, selected, activation records of
        the selected) or None]; the tracers' counts are refreshed"""
        J, keep = self._tracer_jobs(jobs)
        _chk(self.L.ldso_ba_batch_select_activate_tracers(self.h, J, C.c_float(min_trace_quality), C.c_int(min_obs), C.c_float(min_idepth_hessian), C.c_int(gn_iterations)))
        out = []
        for i, k in enumerate(keep):
            if k is None:
                out.append(None)
                continue
            k[0].n = J[i].n_left
            out.append((k[4], k[5][:J[i].n_selected].copy(), k[6][:J[i].n_selected].copy()))
        return out

    def update_windows(self, jobs):
        """ldso_ba_batch_update_windows: every window of the batch becomes its next one in one call.  jobs[i]: the arguments of BA.update_window as a tuple / list
        (image_slots, frame_from, point_from, res_mask[, fresh, fresh_res, fresh_mrb, fresh_ngr]) or a dict with those names, or None for a window that sits out
        (a tuple whose frame_from is None sits out too).  The handles' F / P / R are refreshed afterwards, as BA.update_window does."""
        n = len(self.handles)
        assert len(jobs) == n
        names = ("image_slots", "frame_from", "point_from", "res_mask", "fresh", "fresh_res", "fresh_mrb", "fresh_ngr")
        J = (WinJob * n)()
        keep = []
        for i, job in enumerate(jobs):
            if job is None:
                continue
            a = [job.get(k) for k in names] if isinstance(job, dict) else (list(job) + [None] * 8)[:8]
            if a[1] is None:
                continue
            sl = np.ascontiguousarray(a[0], np.int32); ff = np.ascontiguousarray(a[1], np.int32)
            pf = np.ascontiguousarray(a[2], np.int32); mk = np.ascontiguousarray(a[3], np.uint32)
            assert len(sl) == len(ff) and len(pf) == len(mk)
            nf = 0 if a[4] is None else len(a[4]); nr = 0 if a[5] is None else len(a[5])
            fp = np.ascontiguousarray(a[4]) if nf else None; fr = np.ascontiguousarray(a[5]) if nr else None
            fm = np.ascontiguousarray(a[6], np.float32) if nf else None; fg = np.ascontiguousarray(a[7], np.int32) if nf else None
            keep.append((sl, ff, pf, mk, fp, fr, fm, fg))
            j = J[i]
            j.F, j.image_slot, j.frame_from, j.P, j.point_from, j.res_mask = len(sl), sl.ctypes.data, ff.ctypes.data, len(pf), pf.ctypes.data, mk.ctypes.data
            j.n_fresh, j.fresh, j.n_fresh_res, j.fresh_res = nf, (fp.ctypes.data if nf else None), nr, (fr.ctypes.data if nr else None)
            j.fresh_mrb, j.fresh_ngr = (fm.ctypes.data if nf else None), (fg.ctypes.data if nf else None)
        try:
            _chk(self.L.ldso_ba_batch_update_windows(self.h, J))
        finally:
            for h in self.handles:
                h._sync_dims()

    def set_frames(self, frames_list, calib_list, priors=None):
        """ldso_ba_batch_set_frames: BA.set_frames(frames, calib) followed by BA.set_prior(HM, bM) on every window with frames_list[i] not None; priors[i] = (HM, bM),
        either may be None (zero), or None for a zero prior; priors=None: zero priors everywhere."""
        n = len(self.handles)
        assert len(frames_list) == n and len(calib_list) == n and (priors is None or len(priors) == n)
        J = (FramesJob * n)()
        keep = []
        for i, fr in enumerate(frames_list):
            if fr is None:
                continue
            fr = np.ascontiguousarray(fr); c = np.ascontiguousarray(calib_list[i])
            assert len(fr) == self.handles[i].F
            HM, bM = (None, None) if priors is None or priors[i] is None else priors[i]
            HM = np.ascontiguousarray(HM, np.float64) if HM is not None else None
            bM = np.ascontiguousarray(bM, np.float64) if bM is not None else None
            k = 8 * self.handles[i].F + 4
            assert (HM is None or HM.size == k * k) and (bM is None or bM.size == k)
            keep.append((fr, c, HM, bM))
            J[i].frames, J[i].calib = fr.ctypes.data, c.ctypes.data
            J[i].HM, J[i].bM = (None if HM is None else HM.ctypes.data), (None if bM is None else bM.ctypes.data)
        _chk(self.L.ldso_ba_batch_set_frames(self.h, J))

    def balanced(self):
        """True: the batch runs balanced cuts (ldso_ba_batch_balanced), False: regular chunks of chunk_points() points"""
        b = C.c_int()
        _chk(self.L.ldso_ba_batch_balanced(self.h, C.byref(b)))
        return bool(b.value)

    def sync(self):
        self.handles[0].sync()

    def time_linearize(self, reps=50):
        us = C.c_double()
        _chk(self.L.ldso_ba_batch_time_linearize(self.h, C.c_int(reps), C.byref(us)))
        return us.value

    def reduce_splits(self):
        """K-splits per Schur tile the batch reduces its windows with (BA.set_reduce_splits gives a lone handle the same arithmetic)"""
        n = C.c_int(0)
        _chk(self.L.ldso_ba_batch_reduce_splits(self.h, C.byref(n)))
        return int(n.value)

    def chunk_points(self):
        n = C.c_int()
        _chk(self.L.ldso_ba_batch_chunk_points(self.h, C.byref(n)))
        return n.value

    def close(self):
        if self.h:
            self.L.ldso_ba_batch_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Tracker:
    """CoarseTracker handle (src/frontend/CoarseTracker.cc) on one GPU."""

    def __init__(self, w, h, levels, settings, calib, device=0):
        self.L = lib()
        self.h = C.c_void_p()
        _chk(self.L.ldso_tr_create(C.c_int(device), C.c_int(w), C.c_int(h), C.c_int(levels), C.byref(self.h)))
        self.w, self.hh, self.levels = w, h, levels
        s = np.ascontiguousarray(settings)
        _chk(self.L.ldso_tr_set_settings(self.h, _p(s)))
        c = np.ascontiguousarray(calib)
        _chk(self.L.ldso_tr_make_k(self.h, _p(c)))

    def close(self):
        if self.h:
            _chk(self.L.ldso_tr_destroy(self.h))          # refused while the tracker is a member of a live TrackerGroup: the handle stays
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_ptr):
        """the caller's HIP stream (an integer handle) instead of the tracker's own; None / 0: an own one again"""
        _chk(self.L.ldso_tr_set_stream(self.h, C.c_void_p(stream_ptr or None)))

    def _pyr(self, pyr):
        keep = [np.ascontiguousarray(pyr[l], np.float32) for l in range(self.levels)]
        arr = (C.c_void_p * self.levels)(*[a.ctypes.data for a in keep])
        return arr, keep

    def set_ref(self, pyr, a, b, exposure, pts):
        arr, keep = self._pyr(pyr)
        pts = np.ascontiguousarray(pts, np.float32)
        _chk(self.L.ldso_tr_set_ref(self.h, arr, C.c_float(a), C.c_float(b), C.c_float(exposure), _p(pts), C.c_int(len(pts))))

    def set_new_frame(self, pyr, exposure=1.0):
        arr, keep = self._pyr(pyr)
        _chk(self.L.ldso_tr_set_new_frame(self.h, arr, C.c_float(exposure)))

    def set_new_frame_image(self, irradiance, exposure=1.0):
        a = np.ascontiguousarray(irradiance, np.float32)
        _chk(self.L.ldso_tr_set_new_frame_image(self.h, _p(a), C.c_float(exposure)))

    def set_new_frame_pyramid(self, pyr: "Pyramid", exposure=1.0):
        _chk(self.L.ldso_tr_set_new_frame_pyramid(self.h, pyr.h, C.c_float(exposure)))
        self._new_pyr = pyr

    def set_ref_pyramid(self, pyr: "Pyramid", a, b, exposure, pts):
        pts = np.ascontiguousarray(pts, np.float32)
        _chk(self.L.ldso_tr_set_ref_pyramid(self.h, pyr.h, C.c_float(a), C.c_float(b), C.c_float(exposure), _p(pts), C.c_int(len(pts))))
        self._ref_pyr = pyr

    def get_new_frame_level(self, lvl):
        out = np.zeros((self.hh >> lvl, self.w >> lvl, 3), np.float32)
        _chk(self.L.ldso_tr_get_new_frame_level(self.h, C.c_int(lvl), _p(out)))
        return out

    def motion_hypotheses(self, sprelast, slast, lastF, poses_valid=True):
        P = [np.ascontiguousarray(np.asarray(m, np.float64)[:3, :4]) for m in (sprelast, slast, lastF)]
        out = np.zeros((83, 3, 4)); n = C.c_int()
        _chk(self.L.ldso_tr_motion_hypotheses(_p(P[0]), _p(P[1]), _p(P[2]), C.c_int(1 if poses_valid else 0), _p(out), C.byref(n)))
        return out[: n.value]

    def track_new_coarse(self, sprelast, slast, lastF, aff_last, last_rmse, retrack_threshold=1.5, poses_valid=True):
        """ldso_tr_track_new_coarse: FullSystem::trackNewCoarse (FullSystem.cc:179-386); poses are worldToCam 4x4 / 3x4"""
        P = [np.ascontiguousarray(np.asarray(m, np.float64)[:3, :4]) for m in (sprelast, slast, lastF)]
        aff = np.asarray(aff_last, np.float32); rmse = np.ascontiguousarray(last_rmse, np.float64).copy()
        res4 = np.zeros(4); w2c = np.zeros((3, 4)); aff_out = np.zeros(2, np.float32); tries, good = C.c_int(-1), C.c_int(-1)
        _chk(self.L.ldso_tr_track_new_coarse(self.h, _p(P[0]), _p(P[1]), _p(P[2]), C.c_int(1 if poses_valid else 0), _p(aff), _p(rmse), C.c_double(retrack_threshold),
                                             _p(res4), _p(w2c), _p(aff_out), C.byref(tries), C.byref(good)))
        return dict(result=res4, w2c=w2c, aff=aff_out, lastCoarseRMSE=rmse, tries=tries.value, good=good.value)

    def select_hypothesis(self, batch, coarsest, last_coarse_rmse0=float("nan"), retrack_threshold=1.5):
        lr = np.ascontiguousarray(batch["lastResiduals"], np.float64)
        ok = np.ascontiguousarray(batch["ok"], np.int32)
        best, tries = C.c_int(), C.c_int()
        ach = np.zeros(5)
        _chk(self.L.ldso_tr_select_hypothesis(C.c_int(len(ok)), C.c_int(coarsest), _p(lr), _p(ok), C.c_double(last_coarse_rmse0), C.c_double(retrack_threshold),
                                              C.byref(best), C.byref(tries), _p(ach)))
        return best.value, tries.value, ach

    def pc(self, lvl):
        n = C.c_int()
        _chk(self.L.ldso_tr_get_pc(self.h, C.c_int(lvl), None, None, None, None, C.byref(n)))
        u, v, d, c = (np.zeros(n.value, np.float32) for _ in range(4))
        _chk(self.L.ldso_tr_get_pc(self.h, C.c_int(lvl), _p(u), _p(v), _p(d), _p(c), C.byref(n)))
        return u, v, d, c

    def calc_res(self, lvl, T, a, b, cutoff):
        T = np.ascontiguousarray(T[:3, :4], np.float64)
        rs = np.zeros(6)
        n = C.c_int()
        _chk(self.L.ldso_tr_calc_res(self.h, C.c_int(lvl), _p(T), C.c_float(a), C.c_float(b), C.c_float(cutoff), _p(rs), C.byref(n)))
        return rs, n.value

    def calc_gs(self, lvl, T, a, b):
        T = np.ascontiguousarray(T[:3, :4], np.float64)
        H = np.zeros((8, 8))
        bb = np.zeros(8)
        _chk(self.L.ldso_tr_calc_gs(self.h, C.c_int(lvl), _p(T), C.c_float(a), C.c_float(b), _p(H), _p(bb)))
        return H, bb

    def track(self, T, a, b, coarsest, min_res=None):
        r = self.track_batch([T], [(a, b)], coarsest, min_res)
        return {k: (v[0] if isinstance(v, (list, np.ndarray)) else v) for k, v in r.items()}

    def last_track_pivoted_solves(self):
        """LM solves of the last track call that fell back to the pivoted LDL^T (ill-conditioned 8 x 8 system)"""
        n = C.c_int(0)
        _chk(self.L.ldso_tr_last_track_pivoted_solves(self.h, C.byref(n)))
        return int(n.value)

    def last_track_evals(self):
        """(evals[5], pc_n[5]) of the last track: calcRes evaluations and reference points per pyramid level"""
        ev = np.zeros(5, np.int32); pc = np.zeros(5, np.int32)
        _chk(self.L.ldso_tr_last_track_evals(self.h, _p(ev), _p(pc)))
        return ev, pc

    def track_batch(self, Ts, affs, coarsest, min_res=None):
        n = len(Ts)
        T = np.ascontiguousarray(np.stack([np.asarray(t)[:3, :4] for t in Ts]), np.float64).copy()
        ab = np.ascontiguousarray(np.asarray(affs, np.float32).reshape(n, 2)).copy()
        mr = np.full(5, np.nan) if min_res is None else np.asarray(min_res, np.float64)
        lr = np.zeros((n, 5))
        fl = np.zeros((n, 3))
        ok = np.zeros(n, np.int32)
        it = np.zeros(n, np.int32)
        _chk(self.L.ldso_tr_track_batch(self.h, C.c_int(n), _p(T), _p(ab), C.c_int(coarsest), _p(mr), _p(lr), _p(fl), _p(ok), _p(it)))
        return dict(ok=ok.astype(bool), T=T, a=ab[:, 0].copy(), b=ab[:, 1].copy(), lastResiduals=lr, flow=fl, iterations=it)


def coop_width(count, num_cu) -> int:
    """ldso_tr_coop_width: workgroups that share each of `count` concurrent tracks on a device with num_cu CUs"""
    G = C.c_int()
    _chk(lib().ldso_tr_coop_width(C.c_int(count), C.c_int(num_cu), C.byref(G)))
    return G.value


def _active_mask(active, n):
    """an active mask as the group entries take it: (None, all indices) or (n bytes, the indices set)"""
    if active is None:
        return None, list(range(n))
    act = np.ascontiguousarray(np.asarray(active).astype(bool), np.uint8)
    assert act.shape == (n,)
    return act, [i for i in range(n) if act[i]]


class _Group:
    """what the groups share: the members are kept alive (the group dereferences them), the handle comes from the entry named by _create and goes back
    through the one named by _destroy - unchecked, unlike a member's close: a group's destroy has nothing that refuses it"""
    _create = _destroy = None

    def __init__(self, members):
        self.L = lib()
        self.members = list(members)
        arr = (C.c_void_p * len(self.members))(*[m.h for m in self.members])
        self.h = C.c_void_p()
        _chk(getattr(self.L, self._create)(arr, C.c_int(len(self.members)), C.byref(self.h)))

    def close(self):
        if self.h:
            getattr(self.L, self._destroy)(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class TrackerGroup(_Group):
    """ldso_tr_group_*: the tracks of several trackers (independent sequences on one device and one stream) in one launch.  Arguments and results are per member,
    in the order of `trackers`; the members stay usable on their own between group calls."""

    _create, _destroy = "ldso_tr_group_create", "ldso_tr_group_destroy"

    def __init__(self, trackers):
        super().__init__(trackers)
        self.trackers = self.members

    def coop_width(self, n_jobs) -> int:
        G = C.c_int()
        _chk(self.L.ldso_tr_group_coop_width(self.h, C.c_int(n_jobs), C.byref(G)))
        return G.value

    def track(self, Ts, affs, coarsest, min_res=None, active=None):
        """ldso_tr_group_track -> per member the dict of Tracker.track (None for an inactive member).  Ts: n poses (4x4 or 3x4), affs: n (a, b) pairs, coarsest: n levels
        (or one for all), min_res: None, one row of 5 for all, or n rows (a row of NaN never aborts)."""
        n = len(self.trackers)
        T = np.ascontiguousarray(np.stack([np.asarray(t, np.float64)[:3, :4] for t in Ts]), np.float64).copy()
        ab = np.ascontiguousarray(np.asarray(affs, np.float32).reshape(n, 2)).copy()
        co = np.ascontiguousarray(np.broadcast_to(np.asarray(coarsest, np.int32), (n,)), np.int32)
        mr = None if min_res is None else np.ascontiguousarray(np.broadcast_to(np.asarray(min_res, np.float64), (n, 5)), np.float64)
        lr = np.zeros((n, 5)); fl = np.zeros((n, 3)); ok = np.zeros(n, np.int32); it = np.zeros(n, np.int32)
        act, idx = _active_mask(active, n)
        _chk(self.L.ldso_tr_group_track(self.h, _p(act), _p(T), _p(ab), _p(co), _p(mr), _p(lr), _p(fl), _p(ok), _p(it)))
        out = [None] * n
        for i in idx:
            out[i] = dict(ok=bool(ok[i]), T=T[i].copy(), a=ab[i, 0], b=ab[i, 1], lastResiduals=lr[i].copy(), flow=fl[i].copy(), iterations=it[i])
        return out

    def track_new_coarse(self, sprelast, slast, lastF, aff_last, last_rmse, retrack_threshold=1.5, poses_valid=True, active=None):
        """ldso_tr_group_track_new_coarse -> per member the dict of Tracker.track_new_coarse (None for an inactive member).  sprelast / slast / lastF: n worldToCam poses
        each, aff_last: n pairs, last_rmse: n rows of 5; retrack_threshold and poses_valid: one value for all or n."""
        n = len(self.trackers)
        P = [np.ascontiguousarray(np.stack([np.asarray(m, np.float64)[:3, :4] for m in ms]), np.float64) for ms in (sprelast, slast, lastF)]
        aff = np.ascontiguousarray(np.asarray(aff_last, np.float32).reshape(n, 2))
        rmse = np.ascontiguousarray(np.asarray(last_rmse, np.float64).reshape(n, 5)).copy()
        thr = np.ascontiguousarray(np.broadcast_to(np.asarray(retrack_threshold, np.float64), (n,)), np.float64)
        pv = np.ascontiguousarray(np.broadcast_to(np.asarray(poses_valid).astype(np.int32), (n,)), np.int32)
        res4 = np.zeros((n, 4)); w2c = np.zeros((n, 3, 4)); aff_out = np.zeros((n, 2), np.float32)
        tries = np.full(n, -1, np.int32); good = np.full(n, -1, np.int32)
        act, idx = _active_mask(active, n)
        _chk(self.L.ldso_tr_group_track_new_coarse(self.h, _p(act), _p(P[0]), _p(P[1]), _p(P[2]), _p(pv), _p(aff), _p(rmse), _p(thr), _p(res4), _p(w2c), _p(aff_out),
                                                   _p(tries), _p(good)))
        out = [None] * n
        for i in idx:
            out[i] = dict(result=res4[i].copy(), w2c=w2c[i].copy(), aff=aff_out[i].copy(), lastCoarseRMSE=rmse[i].copy(), tries=int(tries[i]), good=int(good[i]))
        return out


class Tracer:
    """Immature-point tracing handle: FullSystem::traceNewCoarse / ImmaturePoint::traceOn on one GPU."""

    def __init__(self, w, h, max_points, settings=None, device=0):
        self.L = lib()
        self.h = C.c_void_p()
        _chk(self.L.ldso_trace_create(C.c_int(device), C.c_int(w), C.c_int(h), C.c_int(max_points), C.byref(self.h)))
        self.w, self.hh, self.n = w, h, 0
        if settings is not None:
            s = np.ascontiguousarray(settings)
            _chk(self.L.ldso_trace_set_settings(self.h, _p(s)))

    def close(self):
        if self.h:
            self.L.ldso_trace_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_points(self, pts):
        a = np.ascontiguousarray(pts)
        assert a.dtype == synth.IMMATURE_DTYPE
        _chk(self.L.ldso_trace_set_points(self.h, C.c_int(len(a)), _p(a)))
        self.n = len(a)

    def get_points(self):
        out = np.zeros(self.n, synth.IMMATURE_DTYPE)
        _chk(self.L.ldso_trace_get_points(self.h, _p(out)))
        return out

    def set_point_types(self, my_type):
        """ImmaturePoint::my_type of the current records (set_points resets them to 1)"""
        t = np.ascontiguousarray(my_type, np.float32)
        assert len(t) == self.n
        _chk(self.L.ldso_trace_set_point_types(self.h, _p(t)))

    def get_point_types(self):
        out = np.zeros(self.n, np.float32)
        _chk(self.L.ldso_trace_get_point_types(self.h, _p(out)))
        return out

    def compact(self, keep=None, host_map=None, n_hosts=None):
        """stable compaction on the device: record i stays iff keep[i] and host_map[host] >= 0, and gets host = host_map[host] -> the new count.
        n_hosts: the frames a host may name (default: len(host_map), else the library's capacity)"""
        k = None if keep is None else np.ascontiguousarray(np.asarray(keep) != 0, np.uint8)
        m = None if host_map is None else np.ascontiguousarray(host_map, np.int32)
        assert k is None or len(k) == self.n
        nh = n_hosts if n_hosts is not None else (len(m) if m is not None else MAX_FRAMES)
        left = C.c_int()
        _chk(self.L.ldso_trace_compact(self.h, _p(k), C.c_int(nh), _p(m), C.byref(left)))
        self.n = left.value
        return self.n

    def append_points_device(self, n, immature_dev_ptr):
        """n immature records in device memory (Features.device_ptrs) behind the current points, device to device"""
        _chk(self.L.ldso_trace_append_points_device(self.h, C.c_int(n), C.c_void_p(immature_dev_ptr)))
        self.n += n

    def set_tail_types_device(self, n, type_dev_ptr):
        """my_type of the last n records from n floats in device memory (PixelSelector.device_ptrs)"""
        _chk(self.L.ldso_trace_set_tail_types_device(self.h, C.c_int(n), C.c_void_p(type_dev_ptr)))

    def set_frame(self, dI_level0):
        a = np.ascontiguousarray(dI_level0, np.float32)
        _chk(self.L.ldso_trace_set_frame(self.h, _p(a)))

    def set_frame_raw(self, irradiance):
        a = np.ascontiguousarray(irradiance, np.float32)
        _chk(self.L.ldso_trace_set_frame_raw(self.h, _p(a)))

    def set_frame_pyramid(self, pyr: "Pyramid"):
        _chk(self.L.ldso_trace_set_frame_pyramid(self.h, pyr.h))
        self._pyr = pyr

    def trace_on(self, KRKi, Kt, aff):
        K1 = np.ascontiguousarray(KRKi, np.float32); K2 = np.ascontiguousarray(Kt, np.float32); A = np.ascontiguousarray(aff, np.float32)
        counts = np.zeros(6, np.int32)
        _chk(self.L.ldso_trace_on(self.h, C.c_int(len(K1)), _p(K1), _p(K2), _p(A), _p(counts)))
        return counts

    def set_stream(self, stream_ptr):
        """the caller's stream (None: an own one again); the tracer holds no frame afterwards: set it again"""
        _chk(self.L.ldso_trace_set_stream(self.h, C.c_void_p(stream_ptr)))


class TracerGroup(_Group):
    """ldso_trace_group_*: the traces of several tracers (independent sequences on one device and one stream) in one launch.  Arguments and results are per member,
    in the order of `tracers`; the members stay usable on their own between group calls."""

    _create, _destroy = "ldso_trace_group_create", "ldso_trace_group_destroy"

    def __init__(self, tracers):
        super().__init__(tracers)
        self.tracers = self.members

    def trace_on(self, poses, active=None):
        """ldso_trace_group_on -> counts (n, 6) int32; rows of inactive members stay zero.  poses: one (KRKi, Kt, aff) triple per member (None for an inactive one)."""
        n = len(self.tracers)
        assert len(poses) == n
        act, idx = _active_mask(active, n)
        keep = []
        ptrs = [(C.c_void_p * n)() for _ in range(3)]
        nh = np.zeros(n, np.int32)
        for i in idx:
            K = [np.ascontiguousarray(a, np.float32) for a in poses[i]]
            nh[i] = len(K[0])
            assert K[0].size == 9 * nh[i] and K[1].size == 3 * nh[i] and K[2].size == 2 * nh[i]
            keep.append(K)
            for q in range(3):
                ptrs[q][i] = K[q].ctypes.data
        counts = np.zeros((n, 6), np.int32)
        _chk(self.L.ldso_trace_group_on(self.h, _p(act), _p(nh), ptrs[0], ptrs[1], ptrs[2], _p(counts)))
        return counts


    def compact(self, keeps=None, host_maps=None, n_hosts=None, active=None):
        """ldso_trace_group_compact: Tracer.compact of every active member in one call -> the members' new counts (n) int32; rows of inactive members hold their
        unchanged counts.  keeps / host_maps: per member the arguments of Tracer.compact (None, or a None entry: all kept / the identity); n_hosts: per member, default as
        Tracer.compact"""
        n = len(self.tracers)
        act, idx = _active_mask(active, n)
        hold = []
        PK, PM = (C.c_void_p * n)(), (C.c_void_p * n)()
        nh = np.zeros(n, np.int32)
        for i in idx:
            k = None if keeps is None or keeps[i] is None else np.ascontiguousarray(np.asarray(keeps[i]) != 0, np.uint8)
            m = None if host_maps is None or host_maps[i] is None else np.ascontiguousarray(host_maps[i], np.int32)
            assert k is None or len(k) == self.tracers[i].n
            nh[i] = n_hosts[i] if n_hosts is not None and n_hosts[i] is not None else (len(m) if m is not None else MAX_FRAMES)
            hold.append((k, m))
            if k is not None and len(k):
                PK[i] = k.ctypes.data
            if m is not None:
                PM[i] = m.ctypes.data
        left = np.array([t.n for t in self.tracers], np.int32)
        _chk(self.L.ldso_trace_group_compact(self.h, _p(act), PK, _p(nh), PM, _p(left)))
        for i in idx:
            self.tracers[i].n = int(left[i])
        return left


class PyramidGroup(_Group):
    """ldso_pyr_group_*: FrameHessian::makeImages of several pyramids (one device; sizes and level counts are free) in at most 2 x Lmax launches per call."""

    _create, _destroy = "ldso_pyr_group_create", "ldso_pyr_group_destroy"

    def __init__(self, pyramids):
        super().__init__(pyramids)
        self.pyramids = self.members

    def make_images(self, images, stream=None, active=None):
        """ldso_pyr_group_make_images: images = one irradiance array per member (None for an inactive one), enqueued on `stream`; like Pyramid.make_images it does not wait.
        The converted arrays are kept until the next call: the copies read them on the stream."""
        n = len(self.pyramids)
        assert len(images) == n
        act, idx = _active_mask(active, n)
        ptrs = (C.c_void_p * n)()
        keep = []
        for i in idx:
            a = np.ascontiguousarray(images[i], np.float32)
            assert a.size == self.pyramids[i].w * self.pyramids[i].hh
            keep.append(a)
            ptrs[i] = a.ctypes.data
        _chk(self.L.ldso_pyr_group_make_images(self.h, _p(act), ptrs, C.c_void_p(stream)))
        self._images = keep
        return self

    def make_images_device(self, image_ptrs, stream=None, active=None):
        """ldso_pyr_group_make_images_device: one device pointer per member (None / 0 for an inactive one)"""
        n = len(self.pyramids)
        assert len(image_ptrs) == n
        act, idx = _active_mask(active, n)
        ptrs = (C.c_void_p * n)()
        for i in idx:
            ptrs[i] = image_ptrs[i]
        _chk(self.L.ldso_pyr_group_make_images_device(self.h, _p(act), ptrs, C.c_void_p(stream)))
        return self


class UndistorterGroup(_Group):
    """ldso_undist_group_*: the raw frames of several undistorters (independent sequences on one device and one stream) in one copy and one launch, optionally
    straight into a PyramidGroup of as many members.  Arguments and results are per member, in the order of `undistorters`."""

    _create, _destroy = "ldso_undist_group_create", "ldso_undist_group_destroy"

    def __init__(self, undistorters):
        super().__init__(undistorters)
        self.undistorters = self.members

    def frames(self, raws, exposures, factors=None, pyr_group: "PyramidGroup" = None, active=None):
        """ldso_undist_group_frames: raws = one uint8 or uint16 image of the original size per member (None for an inactive one) -> float32 (n,) of the exposures
        the reference would return, NaN for inactive members.  The frames are staged before the call returns; it does not wait for the device."""
        n = len(self.undistorters)
        assert len(raws) == n and len(exposures) == n and (factors is None or len(factors) == n)
        act, idx = _active_mask(active, n)
        ptrs = (C.c_void_p * n)()
        bpp = np.zeros(n, np.int32)
        keep = []
        for i in idx:
            if raws[i] is None:          # refused by the library, with the member's index
                continue
            r = np.ascontiguousarray(raws[i])
            assert r.dtype in (np.uint8, np.uint16) and r.size == self.undistorters[i].w_org * self.undistorters[i].h_org
            keep.append(r)
            ptrs[i] = r.ctypes.data
            bpp[i] = r.dtype.itemsize
        e = np.ascontiguousarray(exposures, np.float32)
        f = np.ones(n, np.float32) if factors is None else np.ascontiguousarray(factors, np.float32)
        out = np.full(n, np.nan, np.float32)
        _chk(self.L.ldso_undist_group_frames(self.h, _p(act), ptrs, _p(bpp), _p(e), _p(f), pyr_group.h if pyr_group is not None else None, _p(out)))
        return out

    def profile(self, enable=True):
        """microseconds of the last profiled call: the one copy, the undistortion kernel, the grouped pyramid build"""
        us = np.zeros(3, np.float32)
        _chk(self.L.ldso_undist_group_profile(self.h, C.c_int(1 if enable else 0), _p(us)))
        return us


class FeaturesGroup(_Group):
    """ldso_feat_group_*: the corner features and immature points of the key frames of several detectors (independent sequences on one device and one stream) in
    five launches, six when the records are appended to the sequences' tracers.  Arguments and results are per member, in the order of `detectors`; the members stay
    usable on their own between group calls."""

    _create, _destroy = "ldso_feat_group_create", "ldso_feat_group_destroy"

    def __init__(self, detectors):
        super().__init__(detectors)
        self.detectors = self.members

    def detect(self, pyramids, n_features, host_indices=None, tracers=None, active=None):
        """ldso_feat_group_detect -> (n, n_corners, status) int32 arrays of one entry per member; entries of inactive members are -1.  pyramids: one Pyramid per
        member (None for an inactive one), n_features: n values or one for all, tracers: None or one Tracer / None per member.  Raises LdsoError; with the code
        E_NONFINITE the results are there all the same: Features.n / n_corners, Tracer.n and `last` = the three arrays."""
        n = len(self.detectors)
        assert len(pyramids) == n and (tracers is None or len(tracers) == n)
        act, idx = _active_mask(active, n)
        P = (C.c_void_p * n)()
        for i in idx:
            if pyramids[i] is not None:          # a missing one is refused by the library, with the member's index
                P[i] = pyramids[i].h
        T = None
        if tracers is not None:
            T = (C.c_void_p * n)()
            for i in idx:
                if tracers[i] is not None:
                    T[i] = tracers[i].h
        nf = np.ascontiguousarray(np.broadcast_to(np.asarray(n_features, np.int32), (n,)), np.int32)
        hi = np.ascontiguousarray(np.broadcast_to(np.asarray(0 if host_indices is None else host_indices, np.int32), (n,)), np.int32)
        cnt = np.full(n, -1, np.int32); cor = np.full(n, -1, np.int32); sta = np.full(n, -1, np.int32)
        code = self.L.ldso_feat_group_detect(self.h, _p(act), P, _p(nf), _p(hi), T, _p(cnt), _p(cor), _p(sta))
        if code in (0, E_NONFINITE):
            for i in idx:
                self.detectors[i].n, self.detectors[i].n_corners = int(cnt[i]), int(cor[i])
                if tracers is not None and tracers[i] is not None:
                    tracers[i].n += int(cnt[i])
        self.last = (cnt, cor, sta)
        _chk(code)
        return cnt, cor, sta

    def get(self, active=None):
        """ldso_feat_group_get -> per member (features, immature records) of its last detection, None for an inactive member"""
        n = len(self.detectors)
        act, idx = _active_mask(active, n)
        PF, PQ = (C.c_void_p * n)(), (C.c_void_p * n)()
        out = [None] * n
        for i in idx:
            f = np.zeros(self.detectors[i].n, synth.FEATURE_DTYPE)
            q = np.zeros(self.detectors[i].n, synth.IMMATURE_DTYPE)
            out[i] = (f, q)
            if len(f):
                PF[i] = f.ctypes.data; PQ[i] = q.ctypes.data
        _chk(self.L.ldso_feat_group_get(self.h, _p(act), PF, PQ))
        return out

    def profile(self, enable=True):
        """microseconds of the last profiled call: cells + compaction, corners, angle + descriptor, records, append"""
        us = np.zeros(5, np.float32)
        _chk(self.L.ldso_feat_group_profile(self.h, C.c_int(1 if enable else 0), _p(us)))
        return us


class Initializer:
    """Monocular initialiser handle: CoarseInitializer::setFirst / trackFrame on one GPU (include/ldso_hip.h)."""

    def __init__(self, w, h, levels, device=0, stream=None):
        self.L = lib()
        self.h = C.c_void_p()
        _chk(self.L.ldso_init_create(C.c_int(device), C.c_int(w), C.c_int(h), C.c_int(levels), C.byref(self.h)))
        self.w, self.hh, self.levels = w, h, levels
        self.n = [0] * levels
        if stream is not None:
            self.set_stream(stream)

    def close(self):
        if self.h:
            self.L.ldso_init_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_handle):
        if not stream_handle:
            raise ValueError("pass a non-default HIP stream handle (0 is the legacy default stream)")
        _chk(self.L.ldso_init_set_stream(self.h, C.c_void_p(stream_handle)))

    def set_first(self, K4, irradiance, points, exposure=1.0, huberTH=9.0, fixAffine=True):
        """K4 = (fxl, fyl, cxl, cyl) of level 0; irradiance float32 [h,w]; points: one INIT_POINT_DTYPE array per level."""
        k = np.ascontiguousarray(K4, np.float32)
        img = np.ascontiguousarray(irradiance, np.float32)
        assert img.shape == (self.hh, self.w) and len(points) == self.levels
        pts = [np.ascontiguousarray(p, dtype=synth.INIT_POINT_DTYPE) for p in points]
        pp = (C.c_void_p * self.levels)(*[p.ctypes.data for p in pts])
        n = np.array([len(p) for p in pts], dtype=np.int32)
        _chk(self.L.ldso_init_set_first(self.h, _p(k), _p(img), C.c_float(exposure), pp, _p(n), C.c_float(huberTH), C.c_int(1 if fixAffine else 0)))
        self.n = [int(x) for x in n]

    def set_schedule(self, first_steps=0, prepare_on_grid=True):
        """Launch schedule of track_frame (ldso_init_set_schedule): the results do not depend on it."""
        _chk(self.L.ldso_init_set_schedule(self.h, C.c_int(first_steps), C.c_int(1 if prepare_on_grid else 0)))

    def set_new_frame(self, irradiance, exposure=1.0):
        img = np.ascontiguousarray(irradiance, np.float32)
        assert img.shape == (self.hh, self.w)
        _chk(self.L.ldso_init_set_new_frame(self.h, _p(img), C.c_float(exposure)))

    def track_frame(self, irradiance=None, exposure=1.0):
        """trackFrame; irradiance None: the frame given to set_new_frame.  Returns the INIT_STATE_DTYPE record."""
        st = np.zeros((), synth.INIT_STATE_DTYPE)
        img = None
        if irradiance is not None:
            img = np.ascontiguousarray(irradiance, np.float32)
            assert img.shape == (self.hh, self.w)
        _chk(self.L.ldso_init_track_frame(self.h, _p(img), C.c_float(exposure), _p(st)))
        return st

    def state(self):
        st = np.zeros((), synth.INIT_STATE_DTYPE)
        _chk(self.L.ldso_init_get_state(self.h, _p(st)))
        return st

    def set_state(self, st):
        st = np.ascontiguousarray(st, dtype=synth.INIT_STATE_DTYPE)
        _chk(self.L.ldso_init_set_state(self.h, _p(st)))

    def points(self, lvl):
        out = np.zeros(self.n[lvl], synth.INIT_POINT_DTYPE)
        _chk(self.L.ldso_init_get_points(self.h, C.c_int(lvl), _p(out)))
        return out

    def set_points(self, lvl, pts):
        pts = np.ascontiguousarray(pts, dtype=synth.INIT_POINT_DTYPE)
        assert len(pts) == self.n[lvl]
        _chk(self.L.ldso_init_set_points(self.h, C.c_int(lvl), _p(pts)))

    def calc_res_and_gs(self, lvl, T, a, b):
        T = np.ascontiguousarray(np.asarray(T, dtype=np.float64)[:3, :4])
        H = np.zeros((8, 8), np.float32); bo = np.zeros(8, np.float32); Hsc = np.zeros((8, 8), np.float32); bsc = np.zeros(8, np.float32)
        res = np.zeros(3, np.float32); ec = np.zeros(3, np.float32)
        _chk(self.L.ldso_init_calc_res_and_gs(self.h, C.c_int(lvl), _p(T), C.c_double(a), C.c_double(b), _p(H), _p(bo), _p(Hsc), _p(bsc), _p(res), _p(ec)))
        return H, bo, Hsc, bsc, res, ec

    def jb(self, lvl):
        """JbBuffer_new [n, 10] of the last evaluation of the level (ldso_init_debug_get_jb); rows of points that are not good after it are not written"""
        out = np.zeros((self.n[lvl], 10), np.float32)
        _chk(self.L.ldso_init_debug_get_jb(self.h, C.c_int(lvl), _p(out)))
        return out

    def eval_step(self, lvl, mode, apply_pending, inc, lam, T, a, b):
        """One evaluation as trackFrame runs it (ldso_init_debug_eval_step): applyStep if apply_pending, resetPoints' per-point part (mode 0) or doStep
        (mode 1) with inc and lambda, then calcResAndGS and calcEC.  Returns what calc_res_and_gs returns."""
        T = np.ascontiguousarray(np.asarray(T, dtype=np.float64)[:3, :4])
        inc = np.ascontiguousarray(inc, np.float32)
        assert inc.shape == (8,)
        H = np.zeros((8, 8), np.float32); bo = np.zeros(8, np.float32); Hsc = np.zeros((8, 8), np.float32); bsc = np.zeros(8, np.float32)
        res = np.zeros(3, np.float32); ec = np.zeros(3, np.float32)
        _chk(self.L.ldso_init_debug_eval_step(self.h, C.c_int(lvl), C.c_int(mode), C.c_int(1 if apply_pending else 0), _p(inc), C.c_float(lam), _p(T),
                                              C.c_double(a), C.c_double(b), _p(H), _p(bo), _p(Hsc), _p(bsc), _p(res), _p(ec)))
        return H, bo, Hsc, bsc, res, ec

    # ---- setFirst from a resident pyramid (ldso_amd/csrc/init_first.hip) --------------------------------------------------------------------------
    @property
    def sparsity(self):
        """sparsityFactor of makePixelStatus: state of the handle, 5 at creation, carried from level to level and from one first frame to the next"""
        v = C.c_int()
        _chk(self.L.ldso_init_get_sparsity(self.h, C.byref(v)))
        return v.value

    @sparsity.setter
    def sparsity(self, value):
        _chk(self.L.ldso_init_set_sparsity(self.h, C.c_int(value)))

    def pixel_status(self, pyr: "Pyramid", lvl, desired_density, recs_left=5, th_fac=1.0):
        """makePixelStatus on level lvl >= 1 -> (return value, gridMaxSelection passes); raises LdsoError (E_NONFINITE: the map can still be fetched)"""
        n, passes = C.c_int(), C.c_int()
        self._status_shape = (self.hh >> lvl, self.w >> lvl)
        _chk(self.L.ldso_init_pixel_status(self.h, pyr.h, C.c_int(lvl), C.c_float(desired_density), C.c_int(recs_left), C.c_float(th_fac), C.byref(n), C.byref(passes)))
        return n.value, passes.value

    def status_map(self):
        """the byte map of the last pixel-status pass, uint8 [h >> lvl, w >> lvl]"""
        out = np.zeros(self._status_shape, np.uint8)
        _chk(self.L.ldso_init_get_status_map(self.h, _p(out), None))
        return out

    def make_nn(self, uv):
        """the searches of makeNN for one float32 [n, 2] position array per level -> per level (nb_idx [n, 10], nb_dist, parent_idx [n], parent_dist); squared distances"""
        uv = [np.ascontiguousarray(a, np.float32).reshape(-1, 2) for a in uv]
        L = len(uv)
        n = np.array([len(a) for a in uv], np.int32)
        out = [(np.zeros((len(a), 10), np.int32), np.zeros((len(a), 10), np.float32), np.zeros(len(a), np.int32), np.zeros(len(a), np.float32)) for a in uv]
        arr = lambda xs: (C.c_void_p * L)(*[x.ctypes.data for x in xs])
        _chk(self.L.ldso_init_make_nn(self.h, C.c_int(L), arr(uv), _p(n), arr([o[0] for o in out]), arr([o[1] for o in out]), arr([o[2] for o in out]),
                                      arr([o[3] for o in out])))
        return out

    def set_first_frame(self, K4, pyr: "Pyramid", pixsel: "PixelSelector", exposure=1.0, huberTH=9.0, fixAffine=True):
        """setFirst on the frame the pyramid holds: selection, records and neighbours on the device.  Returns numPoints per level."""
        k = np.ascontiguousarray(K4, np.float32)
        n = np.zeros(self.levels, np.int32)
        self.n = [0] * self.levels
        _chk(self.L.ldso_init_set_first_frame(self.h, _p(k), pyr.h, C.c_float(exposure), pixsel.h, C.c_float(huberTH), C.c_int(1 if fixAffine else 0), _p(n)))
        self.n = [int(x) for x in n]
        self._status_shape = (self.hh >> (self.levels - 1), self.w >> (self.levels - 1))          # the last pixel-status pass ran on the coarsest level
        return self.n

    def first_profile(self, enable=True):
        """microseconds of the last profiled set_first_frame: level-0 maps, coarser maps, records, tree build (host), searches, schedules + uploads"""
        us = np.zeros(6, np.float32)
        _chk(self.L.ldso_init_first_profile(self.h, C.c_int(1 if enable else 0), _p(us)))
        return us


# ---- host-only entries of the initialiser's first frame (no device) ------------------------------------------------------------------------------
NN_NODE_DTYPE = np.dtype([("child1", np.int32), ("child2", np.int32), ("left_or_feat", np.int32), ("right", np.int32), ("divlow", np.float32), ("divhigh", np.float32)])


def init_pixel_status_plan(n_good, desired, sparsity, recs_left, th_fac):
    """(action, new_sparsity, new_th_fac) of makePixelStatus behind one gridMaxSelection pass"""
    a, s, t = C.c_int(), C.c_int(), C.c_float()
    _chk(lib().ldso_init_pixel_status_plan(C.c_int(n_good), C.c_float(desired), C.c_int(sparsity), C.c_int(recs_left), C.c_float(th_fac), C.byref(a), C.byref(s), C.byref(t)))
    return a.value, s.value, t.value


class NNTree:
    """nanoflann's k-d tree over float32 [n, 2] positions, built and searched on the host (ldso_init_nn_*)"""

    def __init__(self, uv):
        self.L = lib()
        self.h = C.c_void_p()
        uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
        _chk(self.L.ldso_init_nn_build(C.c_int(len(uv)), _p(uv), C.byref(self.h)))
        n, nn, d = C.c_int(), C.c_int(), C.c_int()
        self.root_box = np.zeros(4, np.float32)
        _chk(self.L.ldso_init_nn_info(self.h, C.byref(n), C.byref(nn), C.byref(d), _p(self.root_box)))
        self.n, self.n_nodes, self.depth = n.value, nn.value, d.value

    def close(self):
        if self.h:
            self.L.ldso_init_nn_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def arrays(self):
        """(nodes as NN_NODE_DTYPE in allocation order, vind)"""
        nodes, vind = np.zeros(self.n_nodes, NN_NODE_DTYPE), np.zeros(self.n, np.int32)
        _chk(self.L.ldso_init_nn_get(self.h, _p(nodes), _p(vind)))
        return nodes, vind

    def search(self, query_uv, k=10):
        q = np.ascontiguousarray(query_uv, np.float32).reshape(-1, 2)
        idx, dist = np.zeros((len(q), k), np.int32), np.zeros((len(q), k), np.float32)
        _chk(self.L.ldso_init_nn_search_host(self.h, C.c_int(len(q)), _p(q), C.c_int(k), _p(idx), _p(dist)))
        return idx, dist
