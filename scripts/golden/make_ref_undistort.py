"""Record tests/golden/ref_undistort.npz from the LDSO sources' own Undistort::undistort<T> and PhotometricUndistorter.

    python scripts/golden/make_ref_undistort.py --ref <LDSO source tree> [--time]

Undistort.cc is compiled unmodified, outside this repository (a temporary directory), against the header stand-ins of oracle/ref_shim, and linked with
scripts/golden/undistort_driver.cc (which stands in for the two IOWrap image readers and reads the tables the constructors leave) and the settings globals
of Setting.o that `make -C oracle ref` left in oracle/_ref.  Same flags as the pin library: -O2 -msse4.2 -ffp-contract=off -DNDEBUG.  The calibration and
response text files are written into the temporary directory; the vignette image is handed over in memory.
--time: undistort<unsigned char> at 640 x 480 (RadTan, crop, photometric mode 2), built -O3, median of 50 calls on one core of this host."""
import argparse
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HERE = os.path.dirname(os.path.abspath(__file__))

RADTAN = "RadTan 0.55 0.73 0.49 0.52 -0.28 0.07 0.0002 0.00002"
CASES = {          # camera line, rectification line, output size (the raw frame is 120 x 90 everywhere)
    "A": (RADTAN, "crop", (104, 72)),
    "B": (RADTAN, "0.36 0.52 0.5 0.5 0", (104, 72)),
    "C": ("Pinhole 0.55 0.73 0.49 0.52 0", "none", (120, 90)),
}


def build(ref, tmp, opt):
    inc = ["-I", os.path.join(ROOT, "oracle", "ref_shim"), "-I", os.path.join(ref, "include"), "-I", os.path.join(ref, "thirdparty")]
    flags = ["-std=c++17", "-DNDEBUG", "-fPIC", "-pthread", "-w", *opt]
    und, drv, so = os.path.join(tmp, "Undistort.o"), os.path.join(tmp, "driver.o"), os.path.join(tmp, "libundistort.so")
    subprocess.run(["g++", *flags, *inc, "-c", os.path.join(ref, "src", "frontend", "Undistort.cc"), "-o", und], check=True)
    subprocess.run(["g++", *flags, *inc, "-c", os.path.join(HERE, "undistort_driver.cc"), "-o", drv], check=True)
    setting = os.path.join(ROOT, "oracle", "_ref", "Setting.o")
    assert os.path.exists(setting), "run `make -C oracle ref` first"
    subprocess.run(["g++", "-shared", "-pthread", "-Wl,--no-undefined", "-o", so, drv, und, setting], check=True)
    L = C.CDLL(so)
    L.ud_create.restype = C.c_void_p
    L.ud_run.restype = C.c_float
    L.ud_time.restype = C.c_double
    return L


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def response(depth):
    """a strictly increasing, bent response of whole numbers from 0 to 255 * 2^k in three straight pieces of slope 1, 2 and 4: the constructor's
    normalisation to 0..255 (:94-97) then leaves multiples of 2^-k in regular steps, which keeps the 65536-entry table small in the compressed fixture"""
    n1, n2 = (90, 120) if depth == 256 else (30510, 20025)          # steps of slope 1 and of slope 2; the rest has slope 4
    steps = np.concatenate([np.full(n1, 1.0), np.full(n2, 2.0), np.full(depth - 1 - n1 - n2, 4.0)])
    g = np.concatenate([[0.0], np.cumsum(steps)])
    assert g[-1] == 255 * (2 if depth == 256 else 512) and len(g) == depth
    return g


def vignette(w, h):
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    r2 = ((x - 0.47 * w) / w) ** 2 + ((y - 0.52 * h) / h) ** 2
    v = np.rint(65535 * (1 - 0.9 * r2)).astype(np.uint16)
    v[h // 3, w // 4] = 0          # one inverse entry is infinite
    return v


def make(L, tmp, camera, rect, size_org, size, depth):
    calib, gamma = os.path.join(tmp, "camera.txt"), os.path.join(tmp, f"pcalib{depth}.txt")
    with open(calib, "w") as f:
        f.write(f"{camera}\n{size_org[0]} {size_org[1]}\n{rect}\n{size[0]} {size[1]}\n")
    with open(gamma, "w") as f:
        f.write(" ".join(repr(float(v)) for v in response(depth)) + "\n")
    v = vignette(*size_org)
    L.ud_set_vignette(C.c_int(size_org[0]), C.c_int(size_org[1]), p(v))
    u = C.c_void_p(L.ud_create(calib.encode(), gamma.encode(), b"vignette.png"))
    assert u
    info = np.zeros(7, np.int32)
    L.ud_info(u, p(info))
    assert tuple(info[:4]) == (*size, *size_org) and info[5] == depth and info[6] == 1, info
    return u, info


def tables(L, u, info):
    w, h, w_org, h_org, _, depth, _ = (int(v) for v in info)
    rx, ry, G, vig = np.zeros(w * h, np.float32), np.zeros(w * h, np.float32), np.zeros(depth, np.float32), np.zeros(w_org * h_org, np.float32)
    L.ud_tables(u, p(rx), p(ry), p(G), p(vig))
    return rx.reshape(h, w), ry.reshape(h, w), G, vig.reshape(h_org, w_org)


def run(L, u, info, raw, exposure, factor, mode, use_exposure=True):
    out = np.zeros((int(info[1]), int(info[0])), np.float32)
    r = np.ascontiguousarray(raw)
    e = L.ud_run(u, p(r), C.c_int(r.dtype.itemsize), C.c_float(exposure), C.c_float(factor), C.c_int(mode), C.c_int(1 if use_exposure else 0), p(out))
    return out, e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True)
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "ref_undistort.npz"))
    a = ap.parse_args()
    import undistort_common as uc
    with tempfile.TemporaryDirectory() as tmp:
        if a.time:
            L = build(a.ref, tmp, ["-O3"])
            u, info = make(L, tmp, RADTAN, "crop", (640, 480), (640, 480), 256)
            f8, _ = uc.textured_frames(640, 480)
            ms = L.ud_time(u, p(f8), C.c_int(50))
            print(f"undistort<unsigned char> 640x480 (RadTan, crop, photometric mode 2): median of 50: {ms * 1e3:.1f} us")
            return
        L = build(a.ref, tmp, ["-O2", "-msse4.2", "-ffp-contract=off"])
        size_org = (120, 90)
        f8, f16 = uc.textured_frames(*size_org)
        rec = dict(raw8=f8, raw16=f16)
        for c, (camera, rect, size) in CASES.items():
            u8, i8 = make(L, tmp, camera, rect, size_org, size, 256)
            u16, i16 = make(L, tmp, camera, rect, size_org, size, 65536)
            rx, ry, G8, vig = tables(L, u8, i8)
            rx2, ry2, G16, vig2 = tables(L, u16, i16)
            assert np.array_equal(rx, rx2) and np.array_equal(ry, ry2) and np.array_equal(vig, vig2) and np.isinf(vig).sum() == 1
            k = uc.classify(rx, ry, *size_org)
            assert k["overread"] == 0, (c, k)          # nothing the reference reads for this fixture lies outside its source image
            print(f"case {c}: {size_org} -> {size}, passthrough {int(i8[4])}, tables: {k}")
            # the 65536 floats go in as their first differences (three distinct values in long runs; as a ramp of floats they would be a sixth of the file):
            # every entry is a multiple of 2^-9 below 2^8, so the running sum in double is exact and undistort_common.golden() gets the table back bit for bit
            dG = np.diff(G16.astype(np.float64)).astype(np.float32)
            assert np.array_equal(np.concatenate([[G16[0]], G16[0] + np.cumsum(dG.astype(np.float64))]).astype(np.float32), G16)
            for key, val in (("G256", G8), ("G65536_first", G16[:1].copy()), ("G65536_diff", dG), ("vignetteMapInv", vig)):
                assert key not in rec or np.array_equal(rec[key], val, equal_nan=True)          # the same camera-independent tables in every case
                rec[key] = val
            rec[c + "_dims"] = np.array([*size_org, *size, int(i8[4])], np.int32)
            if not i8[4]:          # a passthrough case never reads its tables: only what the reference's loop would have made of them is kept
                rec[c + "_remapX"], rec[c + "_remapY"] = rx, ry
            rec[c + "_table_classes"] = np.array([k["invalid"], k["zeroed"], k["overread"]], np.int32)
            rec[c + "_u8_m2"], e_on = run(L, u8, i8, f8, uc.EXPOSURE, 1.0, 2)
            rec[c + "_u8_m1"], _ = run(L, u8, i8, f8, uc.EXPOSURE, 1.0, 1)
            rec[c + "_u8_m0"], _ = run(L, u8, i8, f8, uc.EXPOSURE, 1.0, 0)
            rec[c + "_u8_e0"], e_zero = run(L, u8, i8, f8, 0.0, 0.7, 2)          # exposure <= 0: the plain path, with a factor that shows
            rec[c + "_u16_m2"], _ = run(L, u16, i16, f16, uc.EXPOSURE, 1.0, 2)
            # the other two paths on the 16-bit frame: every uc.SAMPLE_ROWS-th row of the reference's output (whole images would take the file past the size
            # of the largest fixture; a row holds every column, and in case B rows of both branches are among them)
            rec[c + "_u16_m1_rows"] = run(L, u16, i16, f16, uc.EXPOSURE, 1.0, 1)[0][::uc.SAMPLE_ROWS].copy()
            rec[c + "_u16_e0_rows"] = run(L, u16, i16, f16, 0.0, 1.0 / 256, 2)[0][::uc.SAMPLE_ROWS].copy()
            _, e_off = run(L, u8, i8, f8, uc.EXPOSURE, 1.0, 2, use_exposure=False)
            rec[c + "_exposure"] = np.array([e_on, e_zero, e_off], np.float32)          # useExposure on, on with exposure 0, off
            L.ud_destroy(u8); L.ud_destroy(u16)
        np.savez_compressed(a.out, **rec)
        size = os.path.getsize(a.out)
        gold = os.path.dirname(a.out)
        largest = max(os.path.getsize(os.path.join(gold, f)) for f in os.listdir(gold) if os.path.join(gold, f) != a.out)
        print(f"{a.out}: {size} bytes (largest other fixture: {largest})")
        assert size < largest


if __name__ == "__main__":
    main()
