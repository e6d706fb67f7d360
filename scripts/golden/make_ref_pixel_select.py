"""Record tests/golden/ref_pixel_select.npz, or with --large tests/golden/ref_pixel_select_large.npz (the 384 x 320 cases, the other file is left alone), from
the LDSO sources' own FrameHessian::makeImages, PixelSelector and ImmaturePoint constructor.

    make -C oracle ref REF=<LDSO source tree>
    python scripts/golden/make_ref_pixel_select.py --ref <LDSO source tree> [--large | --time]

scripts/golden/pixel_select_driver.cc is compiled against the header stand-ins of oracle/ref_shim and linked with the objects `make -C oracle ref` left in
oracle/_ref (PixelSelector2.o, FrameHessian.o, ImmaturePoint.o ... are among them), in a temporary directory.  Same flags as the pin library: -O2 -msse4.2
-ffp-contract=off.  The layout of the file and the property each case must show: tests/pixel_select_common.py; the properties are asserted here while
recording and again by the tests.  The potential a call used is not visible from outside makeMaps: it is the one potential p for which the reference's own
makeMaps(recursionsLeft = 0) from p reproduces the call's map, return value and potential left (asserted to be unique where the call recursed).
--time: makeMaps at 640 x 480 with setting_desiredImmatureDensity's default (1500), the sources rebuilt -O3, median of 50 calls on one core."""
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
REF_TUS = ("src/frontend/PixelSelector2.cc", "src/internal/FrameHessian.cc", "src/internal/ImmaturePoint.cc", "src/internal/GlobalCalib.cc")
f32 = np.float32


def build(ref, tmp, opt=None):
    inc = ["-I", os.path.join(ROOT, "oracle", "ref_shim"), "-I", os.path.join(ref, "include"), "-I", os.path.join(ref, "thirdparty")]
    flags = ["-std=c++17", "-DNDEBUG", "-fPIC", "-pthread", "-w", *(opt or ["-O2", "-msse4.2", "-ffp-contract=off"])]
    drv, so = os.path.join(tmp, "driver.o"), os.path.join(tmp, "libpixsel.so")
    subprocess.run(["g++", *flags, *inc, "-c", os.path.join(HERE, "pixel_select_driver.cc"), "-o", drv], check=True)
    first = []
    if opt:          # --time: the translation units makeMaps runs through at the reference's own optimisation level, ahead of the pin objects
        for tu in REF_TUS:
            o = os.path.join(tmp, os.path.basename(tu)[:-3] + ".o")
            subprocess.run(["g++", *flags, *inc, "-c", os.path.join(ref, tu), "-o", o], check=True)
            first.append(o)
    objs = [o for o in sorted(glob.glob(os.path.join(ROOT, "oracle", "_ref", "*.o"))) if not o.endswith("ref_driver.o")]
    assert objs, "run `make -C oracle ref` first"
    subprocess.run(["g++", "-shared", "-pthread", "-Wl,--allow-multiple-definition", "-o", so, drv, *first, *objs], check=True)
    L = C.CDLL(so)
    for n in ("ps_frame", "ps_selector"):
        getattr(L, n).restype = C.c_void_p
    L.ps_time.restype = C.c_double
    return L


def p(a):
    return a.ctypes.data_as(C.c_void_p)


class Ref:
    def __init__(self, L, w, h):
        self.L, self.w, self.h = L, w, h
        L.ps_init(C.c_int(w), C.c_int(h))

    def frame(self, img_u8, B=None):
        c = np.ascontiguousarray(img_u8, f32)
        assert c.shape == (self.h, self.w)
        return C.c_void_p(self.L.ps_frame(p(c), p(B) if B is not None else None))

    def selector(self):
        return C.c_void_p(self.L.ps_selector())

    def pattern(self, s):
        out = np.zeros(self.w * self.h, np.uint8)
        self.L.ps_pattern(s, p(out))
        return out

    def make_maps(self, s, f, density, rec, thf):
        m = np.zeros((self.h, self.w), f32)
        ret = self.L.ps_make_maps(s, f, p(m), C.c_float(density), C.c_int(rec), C.c_float(thf))
        return ret, m, self.L.ps_get_potential(s)

    def select(self, s, f, pot, thf):
        m, c = np.zeros((self.h, self.w), f32), np.zeros(3, np.int32)
        self.L.ps_select(s, f, p(m), C.c_int(pot), C.c_float(thf), p(c))
        return m, c

    def call(self, s, f, density, rec, thf):
        """one makeMaps on selector s -> dict(map, out = [ret, n2, n3, n4, used, left], ths, thsS, before = the last select pass's map)"""
        pot0 = self.L.ps_get_potential(s)
        ret, m, left = self.make_maps(s, f, density, rec, thf)
        match = []
        for q in ([pot0] if rec == 0 else range(1, 65)):
            t = self.selector()
            self.L.ps_set_potential(t, C.c_int(q))
            r2, m2, l2 = self.make_maps(t, f, density, 0, thf)
            if r2 == ret and l2 == left and np.array_equal(m, m2):
                match.append(q)
            self.L.ps_selector_free(t)
        assert match, "no potential reproduces the call"
        used = pot0 if pot0 in match else match[0]
        assert used == pot0 or len(match) == 1, match
        before, cnt = self.select(s, f, used, thf)
        n32 = (self.w // 32) * (self.h // 32)
        ths, thsS = np.zeros(n32, f32), np.zeros(n32, f32)
        self.L.ps_thresholds(s, p(ths), p(thsS))
        return dict(map=m, out=np.array([ret, *cnt, used, left], np.int32), ths=ths, thsS=thsS, before=before, ambiguous=len(match) > 1)

    def points(self, f, m):
        cap = int((m != 0).sum()) + 1
        imm, typ = np.zeros((cap, 23), f32), np.zeros(cap, f32)
        k = self.L.ps_points(f, p(np.ascontiguousarray(m, f32)), C.c_int(cap), p(imm), p(typ))
        assert k >= 0
        return imm[:k].copy(), typ[:k].copy()


def density_for(R, f, pot, thf, lo, hi):
    """a density whose quotia at potential `pot` lies in [lo, hi): the middle of the interval"""
    s = R.selector()
    _, c = R.select(s, f, pot, thf)
    R.L.ps_selector_free(s)
    return float(f32(0.5 * (lo + hi) * int(c.sum())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True)
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--large", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import feature_detect_common as fc
    import pixel_select_common as pc
    with tempfile.TemporaryDirectory() as tmp:
        if a.time:
            L = build(a.ref, tmp, ["-O3", "-march=x86-64-v3"])
            R = Ref(L, 640, 480)
            for name, img, pot in (("scene", np.clip(np.rint(fc.scene(640, 480)[0]), 0, 255), 3), ("step edges, potential 1", pc.steps_image(640, 480), 1)):
                f, s = R.frame(img), R.selector()
                m = np.zeros((480, 640), f32)
                ms = L.ps_time(s, f, p(m), C.c_float(1500.0), C.c_int(pot), C.c_int(50))
                print(f"makeMaps 640x480 density 1500, {name}: {int((m != 0).sum())} pixels, median of 50: {ms * 1e3:.1f} us")
            return
        L = build(a.ref, tmp)
        out = {}
        B = fc.bent_response()
        out["B"] = B

        def record(R, name, calls, settings=pc.DEFAULT_SETTINGS, large=False, before=None):
            """calls: list of (image name, potential to set or 0, density or (pot, lo, hi) for density_for, recursions_left, th_factor, response)
            large: the layout and the properties of pc.LARGE_CASES (one call each); before: the unthinned map of the same select pass -> returns the call's map"""
            L.ps_settings(p(np.array(settings, f32)))
            s = R.selector()
            out[f"pattern/{R.w}x{R.h}"] = R.pattern(s)
            done = []
            for j, (img, pot0, dens, rec, thf, resp) in enumerate(calls):
                out["crc/" + img if large else "img/" + img] = pc.crc(pc.image(img)) if large else pc.image(img)
                f = R.frame(pc.image(img), B if resp else None)
                if pot0:
                    L.ps_set_potential(s, C.c_int(pot0))
                start = L.ps_get_potential(s)
                if isinstance(dens, tuple):
                    dens = density_for(R, f, start, thf, *dens)
                r = R.call(s, f, dens, rec, thf)
                imm, typ = R.points(f, r["map"])
                k = f"{name}/{j}/"
                out[k + "image"] = np.array(img); out[k + "args"] = np.array([dens, thf], f32); out[k + "iargs"] = np.array([pot0, rec, int(resp)], np.int32)
                out[k + "map"] = r["map"].astype(np.uint8); out[k + "out"] = r["out"]; out[k + "ths"] = r["ths"]; out[k + "thsS"] = r["thsS"]
                out[k + "uv"] = imm[:, :2].astype(np.uint16 if large else np.uint8); out[k + "type"] = typ.astype(np.uint8)
                assert np.array_equal(out[k + "uv"].astype(f32), imm[:, :2]) and np.array_equal(out[k + "type"].astype(f32), typ)
                if name in pc.RECORD_CASES + pc.LARGE_RECORD_CASES:          # the constructor's fields: kept for a few cases, the file stays small
                    out[k + "imm"] = imm
                elif large:          # every 101st record: ranks above 65 536 are among them
                    out[k + "imm_every101"] = imm[::101]
                    assert np.isfinite(imm).all()
                assert np.array_equal(out[k + "map"].astype(f32), r["map"]) and set(np.unique(out[k + "map"])) <= {0, 1, 2, 4}
                done.append(dict(out=r["out"], pot0=start, density=dens, rec=rec, thsS=r["thsS"]))
                print(name, j, "density", dens, "out", r["out"], "points", len(imm), "quotia", pc.quotia(dens, r["out"][1:4]))
            out[f"{name}/settings"] = np.array(settings, f32)
            if large:
                if before is not None:
                    assert np.array_equal(r["before"], before)
                pc.check_large_property(name, r["out"], start, dens, r["map"], before, r["thsS"])
                L.ps_selector_free(s)
                return r["map"]
            npass = pc.passing_level0(pc.image(calls[0][0]), done[0]["thsS"]) if name == "steps" else None
            pc.check_property(name, done, npass)
            L.ps_selector_free(s)

        if a.large:
            path = a.out or pc.GOLDEN_LARGE
            R = Ref(L, pc.LARGE_W, pc.LARGE_H)
            record(R, "large_stripes_p1", [("stripes", 1, 1e6, 0, 1.0, False)], large=True)
            unthinned = record(R, "large_mixed_p1", [("stripes_noise", 1, 1e6, 0, 1.0, False)], large=True)
            record(R, "large_mixed_thinned", [("stripes_noise", 1, (0.5, 0.6), 0, 1.0, False)], large=True, before=unthinned)
            record(R, "large_natural", [("large_scene", 3, (1.0, 1.2), 1, 1.0, False)], large=True)
            record(R, "large_recurse", [("large_scene", 3, (1.6, 2.0), 2, 1.0, False)], large=True)
            del out["B"]
            for k in out:          # the records column by column on disk (same shape and type when loaded): a column of positions or colours compresses, a row does not
                if k.endswith(("/uv", "/imm", "/imm_every101")):
                    out[k] = np.asfortranarray(out[k])
            assert set(pc.LARGE_CASES) == {k.split("/")[0] for k in out if k.endswith("/settings")} and {k[4:] for k in out if k.startswith("crc/")} == set(pc.LARGE_IMAGES)
            np.savez_compressed(path, **out)
            print(f"{path}: {os.path.getsize(path)} bytes")
            # the pattern (random bytes: 120 KB) and the 23 constructor fields of large_natural's 6163 records (206 KB) do not compress further
            assert os.path.getsize(path) < 600 * 1024
            return
        a.out = a.out or pc.GOLDEN
        R = Ref(L, 160, 96)
        record(R, "natural", [("scene", 3, (1.0, 1.2), 1, 1.0, False)])
        record(R, "recurse_smaller", [("scene", 3, (1.6, 2.0), 1, 1.0, False)])
        record(R, "recurse_larger", [("scene", 3, (0.03, 0.05), 1, 1.0, False)])
        record(R, "thinning", [("scene", 3, (0.5, 0.6), 1, 1.0, False)])
        record(R, "th_factor2", [("scene", 3, (1.0, 1.2), 1, 2.0, False)])
        record(R, "response", [("scene", 3, (1.0, 1.2), 1, 1.0, True)])
        record(R, "no_direction", [("scene", 3, (1.0, 1.2), 1, 1.0, False)], settings=(0.5, 7.0, 0.75, 0.0))
        record(R, "carried", [("scene", 3, 300.0, 1, 1.0, False), ("scene_flip", 0, 60.0, 1, 1.0, False), ("scene_mirror", 0, 3000.0, 2, 1.0, False)])
        # the decisions of makeMaps on a grid of counts, densities and potentials (tests/test_pixel_select_cpu.py): observed from outside, never restated
        rows_i, rows_d, rows_o = [], [], []
        L.ps_settings(p(np.array(pc.DEFAULT_SETTINGS, f32)))
        for img in ("scene", "flat"):
            out["img/" + img] = pc.image(img)
            f = R.frame(pc.image(img))
            rp = out["pattern/160x96"]
            for pot in (1, 2, 3, 6):
                s = R.selector()
                _, c = R.select(s, f, pot, 1.0)
                L.ps_selector_free(s)
                have = int(c.sum())
                dens = [100.0] if have == 0 else []
                for q in (0.1, 0.25, 0.5, 0.95, 1.0, 1.25, 2.0, 6.0):
                    if have:
                        d = f32(q * have)
                        dens += [float(np.nextafter(d, f32(0))), float(d), float(np.nextafter(d, f32(1e9)))] if q in (0.25, 0.95, 1.25) else [float(d)]
                for d in dens:
                    for rec in (0, 1):
                        s = R.selector()
                        L.ps_set_potential(s, C.c_int(pot))
                        r = R.call(s, f, d, rec, 1.0)
                        L.ps_selector_free(s)
                        ret, used, left = int(r["out"][0]), int(r["out"][4]), int(r["out"][5])
                        if rec and r["ambiguous"]:          # an empty map from several potentials: whether the call recursed cannot be seen, where it ended can
                            assert have == 0
                            rows_o.append([-1, left, ret, -1, -1])
                        elif used != pot:          # the call recursed: what is pinned is the potential of the second pass
                            rows_o.append([1, used, -1, -1, -1])
                        else:
                            sel = np.flatnonzero(r["before"].ravel() != 0)
                            kept = r["map"].ravel()[sel] != 0
                            v = rp[:len(sel)].astype(np.int64)
                            lo = int(v[kept].max()) if kept.any() else -1
                            hi = int(v[~kept].min()) - 1 if (~kept).any() else 255
                            rows_o.append([0, left, ret, lo, hi])
                        rows_i.append([*c, pot, rec]); rows_d.append(d)
        out["plan_in"], out["plan_density"], out["plan_out"] = np.array(rows_i, np.int32), np.array(rows_d, f32), np.array(rows_o, np.int32)
        print("plan rows", len(rows_i), "recursing", int(np.sum(out["plan_out"][:, 0] == 1)))
        R = Ref(L, 96, 64)
        record(R, "clipped5", [("small", 5, 100.0, 0, 1.0, False)])
        record(R, "clipped7", [("small", 7, 60.0, 0, 1.0, False)])
        record(R, "steps", [("steps", 1, 400.0, 0, 1.0, False)])
        assert set(pc.CASES) == {k.split("/")[0] for k in out if k.endswith("/settings")}
        np.savez_compressed(a.out, **out)
        print(f"{a.out}: {os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()
