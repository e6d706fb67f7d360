"""Record tests/golden/ref_detect_corners.npz from the LDSO sources' own FeatureDetector::DetectCorners and ImmaturePoint constructor.

    python scripts/golden/make_ref_detect_corners.py --ref <LDSO source tree> [--time]

FeatureDetector.cc is compiled unmodified, outside this repository (a temporary directory), against the header stand-ins of oracle/ref_shim with
scripts/golden/opencv_standins.h force-included, and linked with scripts/golden/detect_corners_driver.cc and the objects `make -C oracle ref` left in
oracle/_ref (FeatureDetector.o goes first; --allow-multiple-definition lets it win over the stubs of ref_stubs.o).  Same flags as the pin library:
-O2 -msse4.2 -ffp-contract=off.  --time: DetectCorners at 640 x 480, n = 1500, built -O3, median of 50 calls on this host."""
import argparse
import ctypes as C
import glob
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HERE = os.path.dirname(os.path.abspath(__file__))


def build(ref, tmp, opt):
    inc = ["-I", os.path.join(ROOT, "oracle", "ref_shim"), "-I", os.path.join(ref, "include"), "-I", os.path.join(ref, "thirdparty")]
    flags = ["-std=c++17", "-DNDEBUG", "-fPIC", "-pthread", "-w", *opt]
    fd, drv, so = os.path.join(tmp, "FeatureDetector.o"), os.path.join(tmp, "driver.o"), os.path.join(tmp, "libdetect.so")
    subprocess.run(["g++", *flags, "-include", os.path.join(HERE, "opencv_standins.h"), *inc, "-c", os.path.join(ref, "src", "frontend", "FeatureDetector.cc"), "-o", fd], check=True)
    subprocess.run(["g++", *flags, *inc, "-c", os.path.join(HERE, "detect_corners_driver.cc"), "-o", drv], check=True)
    objs = [o for o in sorted(glob.glob(os.path.join(ROOT, "oracle", "_ref", "*.o"))) if not o.endswith("ref_driver.o")]
    assert objs, "run `make -C oracle ref` first"
    subprocess.run(["g++", "-shared", "-pthread", "-Wl,--allow-multiple-definition", "-o", so, drv, fd, *objs], check=True)
    return C.CDLL(so)


def run(L, color, B, n, reps=0):
    h, w = color.shape
    cap = 4 * n + 64
    feat, desc, imm = np.zeros((cap, 6), np.float32), np.zeros((cap, 32), np.uint8), np.zeros((cap, 21), np.float32)
    nc, ms = C.c_int(), C.c_double()
    c = np.ascontiguousarray(color, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    L.gd_detect.restype = C.c_int
    k = L.gd_detect(C.c_int(w), C.c_int(h), p(c), p(B) if B is not None else None, C.c_int(n), C.c_int(cap), p(feat), p(desc), p(imm), C.byref(nc), C.c_int(reps), C.byref(ms))
    return feat[:k], desc[:k], imm[:k], nc.value, ms.value


def edge_patch(img):
    """A 40 x 40 patch of the scene replaced by a soft straight edge whose contrast grows with y: the candidates of the cells inside it have a smaller
    eigenvalue near zero, so the fixture holds features at or below scoreTH (the scene's own texture has none at this size)."""
    img = img.copy()
    prof = np.ones(40)
    prof[:19] = 0; prof[19] = 0.12; prof[20] = 0.5; prof[21] = 0.92
    for y in range(50, 90):
        img[y, 70:110] = 60 + prof * (100 + 2.0 * (y - 50))
    return img


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True)
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "ref_detect_corners.npz"))
    a = ap.parse_args()
    import feature_detect_common as fc
    with tempfile.TemporaryDirectory() as tmp:
        if a.time:
            L = build(a.ref, tmp, ["-O3", "-march=x86-64-v3"])
            irr, _ = fc.scene(640, 480)
            f, _, _, nc, ms = run(L, irr, None, 1500, reps=50)
            print(f"DetectCorners 640x480 n=1500: {len(f)} features, {nc} corners, median of 50: {ms * 1e3:.1f} us")
            return
        L = build(a.ref, tmp, ["-O2", "-msse4.2", "-ffp-contract=off"])
        pattern = np.zeros(1024, np.int32)
        L.gd_pattern(pattern.ctypes.data_as(C.c_void_p))
        irr, _ = fc.scene(192, 144)
        image = np.clip(np.rint(edge_patch(irr)), 0, 255).astype(np.uint8)
        B = fc.bent_response()
        n = 300
        f, d, q, nc, _ = run(L, image.astype(np.float32), B, n)
        np.savez_compressed(a.out, image=image, B=B, n=np.int32(n), pattern=pattern, u=f[:, 0].copy(), v=f[:, 1].copy(), score=f[:, 2].copy(),
                            is_corner=f[:, 3].astype(np.uint8), angle=f[:, 4].copy(), descriptor=d, n_corners=np.int32(nc),
                            color=q[:, 0:8].copy(), weights=q[:, 8:16].copy(), gradH=q[:, 16:20].copy(), energyTH=q[:, 20].copy())
        print(f"{a.out}: {len(f)} features, {nc} corners, {os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()
