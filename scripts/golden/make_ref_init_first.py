"""Record tests/golden/ref_init_first.npz, or with --large tests/golden/ref_init_first_large.npz (setFirst on the 384 x 320 frame, the other file is left alone),
from the LDSO sources' own CoarseInitializer::setFirst, makePixelStatus and CoarseInitializer::makeNN.

    make -C oracle ref REF=<LDSO source tree>
    python scripts/golden/make_ref_init_first.py --ref <LDSO source tree> [--large | --time]

scripts/golden/init_first_driver.cc is compiled against the header stand-ins of oracle/ref_shim and linked with the objects `make -C oracle ref` left in
oracle/_ref (CoarseInitializer.o, PixelSelector2.o, FrameHessian.o ... are among them), in a temporary directory.  Same flags as the pin library: -O2 -msse4.2
-ffp-contract=off.  The layout of the file and the property each case must show: tests/init_first_common.py; the properties are asserted here while recording
and again by the tests.  Two things are not visible from outside makePixelStatus and are observed instead:
  - the number of gridMaxSelection passes of a call = 1 + the number of r in 1..recsLeft at which the call with recsLeft = r differs from the one with r - 1
    (asserted: once two consecutive ones agree, all later ones do);
  - whether a call recursed behind its first pass (the plan rows): yes when the call differs from the same call with recsLeft = 0; no when it does not AND the
    second pass it would have run (run separately, for both values THFac can take) gives something else; otherwise -1, not visible.
--time: setFirst at 640 x 480 with 4 levels, the sources of the frontend rebuilt -O3, median of 50 calls on one core, sparsityFactor 5 before each."""
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
REF_TUS = ("src/frontend/CoarseInitializer.cc", "src/frontend/PixelSelector2.cc", "src/internal/FrameHessian.cc", "src/internal/GlobalCalib.cc")
f32 = np.float32


def build(ref, tmp, opt=None):
    inc = ["-I", os.path.join(ROOT, "oracle", "ref_shim"), "-I", os.path.join(ref, "include"), "-I", os.path.join(ref, "thirdparty")]
    flags = ["-std=c++17", "-DNDEBUG", "-fPIC", "-pthread", "-w", *(opt or ["-O2", "-msse4.2", "-ffp-contract=off"])]
    drv, so = os.path.join(tmp, "driver.o"), os.path.join(tmp, "libinitfirst.so")
    subprocess.run(["g++", *flags, *inc, "-c", os.path.join(HERE, "init_first_driver.cc"), "-o", drv], check=True)
    first = []
    if opt:          # --time: the translation units setFirst runs through at the reference's own optimisation level, ahead of the pin objects
        for tu in REF_TUS:
            o = os.path.join(tmp, os.path.basename(tu)[:-3] + ".o")
            subprocess.run(["g++", *flags, *inc, "-c", os.path.join(ref, tu), "-o", o], check=True)
            first.append(o)
    objs = [o for o in sorted(glob.glob(os.path.join(ROOT, "oracle", "_ref", "*.o"))) if not o.endswith("ref_driver.o")]
    assert objs, "run `make -C oracle ref` first"
    subprocess.run(["g++", "-shared", "-pthread", "-Wl,--allow-multiple-definition", "-o", so, drv, *first, *objs], check=True)
    L = C.CDLL(so)
    for n in ("if_frame", "if_initializer"):
        getattr(L, n).restype = C.c_void_p
    L.if_time_set_first.restype = C.c_double
    return L


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def ptrs(xs):
    return (C.c_void_p * len(xs))(*[x.ctypes.data for x in xs])


class Ref:
    def __init__(self, L, w, h, levels, k4):
        self.L, self.w, self.h, self.levels = L, w, h, levels
        self.k4 = np.array(k4, f32)
        L.if_init(C.c_int(w), C.c_int(h), C.c_int(levels))

    def frame(self, img):
        c = np.ascontiguousarray(img, f32)
        assert c.shape == (self.h, self.w)
        return C.c_void_p(self.L.if_frame(p(c), p(self.k4)))

    def status(self, f, lvl, sparsity, desired, rec, thf):
        """one makePixelStatus from `sparsity` -> (return value, map, sparsity after)"""
        m = np.zeros((self.h >> lvl, self.w >> lvl), np.uint8)
        self.L.if_set_sparsity(C.c_int(sparsity))
        r = self.L.if_pixel_status(f, C.c_int(lvl), C.c_float(desired), C.c_int(rec), C.c_float(thf), p(m))
        return r, m, self.L.if_get_sparsity()

    def status_passes(self, f, lvl, sparsity, desired, rec, thf):
        """the call and its number of passes, observed as the docstring says"""
        runs = [self.status(f, lvl, sparsity, desired, r, thf) for r in range(rec + 1)]
        same = [a[0] == b[0] and a[2] == b[2] and np.array_equal(a[1], b[1]) for a, b in zip(runs, runs[1:])]
        passes = 1 + sum(not s for s in same)
        assert all(same[i + 1] for i in range(len(same) - 1) if same[i]), same
        return runs[-1], passes

    def set_first(self, f):
        c = C.c_void_p(self.L.if_initializer())
        n = np.zeros(self.levels, np.int32)
        self.L.if_set_first(c, f, p(n))
        lv = []
        for l in range(self.levels):
            k = int(n[l])
            fields, good, nb, nbd, par, pard = np.zeros((k, 10), f32), np.zeros(k, np.int32), np.zeros((k, 10), np.int32), np.zeros((k, 10), f32), np.zeros(k, np.int32), np.zeros(k, f32)
            self.L.if_points(c, C.c_int(l), p(fields), p(good), p(nb), p(nbd), p(par), p(pard))
            lv.append(dict(fields=fields, good=good, nb=nb, nbd=nbd, par=par, pard=pard))
        self.L.if_initializer_free(c)
        return n, lv

    def make_nn(self, uv):
        L = len(uv)
        n = np.array([len(a) for a in uv], np.int32)
        nb, nbd = [np.zeros((len(a), 10), np.int32) for a in uv], [np.zeros((len(a), 10), f32) for a in uv]
        par, pard = [np.zeros(len(a), np.int32) for a in uv], [np.zeros(len(a), f32) for a in uv]
        self.L.if_make_nn(C.c_int(L), ptrs(uv), p(n), ptrs(nb), ptrs(nbd), ptrs(par), ptrs(pard))
        return nb, nbd, par, pard

    def distances(self, uv, q, k):
        idx, d = np.zeros((len(q), k), np.int32), np.zeros((len(q), k), f32)
        q = np.ascontiguousarray(q, f32)
        self.L.if_nn_distances(C.c_int(len(uv)), p(uv), C.c_int(len(q)), p(q), C.c_int(k), p(idx), p(d))
        return idx, d


def record_nn(R, ic, uv, key, out):
    """makeNN on the levels uv (float32 [n, 2] each): indices from makeNN itself, squared distances from the same tree type asked again (asserted: same indices)"""
    uv = [np.ascontiguousarray(a, f32) for a in uv]
    nb, nbd, par, pard = R.make_nn(uv)
    res = []
    for l, a in enumerate(uv):
        i10, d10 = R.distances(a, a, 10)
        assert np.array_equal(i10, nb[l]), (key, l)
        if l + 1 < len(uv):
            i1, d1 = R.distances(uv[l + 1], ic.parent_query(a), 1)
            assert np.array_equal(i1[:, 0], par[l]), (key, l)
            d1 = d1[:, 0]
        else:
            assert np.all(par[l] == -1) and np.all(pard[l] == -1)
            d1 = np.full(len(a), -1, f32)
        assert nb[l].max() < 32768 and par[l].max() < 32768
        out[f"{key}/{l}/nb"] = nb[l].astype(np.int16); out[f"{key}/{l}/par"] = par[l].astype(np.int16)
        out[f"{key}/{l}/d10"] = d10; out[f"{key}/{l}/d1"] = d1
        res.append(dict(nb=nb[l], nbd=nbd[l], par=par[l], pard=pard[l], d10=d10, d1=d1))
    return res


def binding_depth(uv):
    """depth of our own k-d tree over uv (the reference's tree does not say its depth)"""
    from ldso_amd import binding
    t = binding.NNTree(uv)
    d = t.depth
    t.close()
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True)
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--large", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import feature_detect_common as fc
    import init_first_common as ic
    from ldso_amd import synth
    with tempfile.TemporaryDirectory() as tmp:
        if a.time:
            L = build(a.ref, tmp, ["-O3", "-march=x86-64-v3"])
            R = Ref(L, 640, 480, 4, (500.0, 500.0, 319.5, 239.5))
            f = R.frame(np.clip(np.rint(fc.scene(640, 480)[0]), 0, 255))
            c = C.c_void_p(L.if_initializer())
            ms = L.if_time_set_first(c, f, C.c_int(5), C.c_int(50))
            n = np.zeros(4, np.int32)
            L.if_set_sparsity(C.c_int(5)); L.if_set_first(c, f, p(n))
            print(f"setFirst 640x480, 4 levels, scene: numPoints {n.tolist()}, median of 50: {ms * 1e3:.1f} us")
            return
        L = build(a.ref, tmp)
        out = {}
        # ---- setFirst on the frames, in one process: the sparsityFactor is carried ------------------------------------------------------------------
        L.if_set_sparsity(C.c_int(5))
        for name, levels in (ic.FRAMES_LARGE if a.large else ic.FRAMES):
            img = ic.image(name)
            h, w = img.shape
            R = Ref(L, w, h, levels, ic.K4[w])
            f = R.frame(img)
            s0 = L.if_get_sparsity()
            n, lv = R.set_first(f)
            s1 = L.if_get_sparsity()
            k = f"first/{name}/"
            out[k + "meta"] = np.array([w, h, levels, s0, s1], np.int32); out[k + "n"] = n
            const = None
            for l, r in enumerate(lv):
                fl = r["fields"]
                xy = np.floor(fl[:, :2]).astype(np.uint16 if a.large else np.uint8)
                assert np.array_equal(ic.pos(xy), fl[:, :2]) and n[l] >= 10
                c8 = np.array([*fl[0, 2:8], fl[0, 9], r["good"][0]], f32)
                assert np.all(fl[:, 2:8] == fl[0, 2:8]) and np.all(fl[:, 9] == fl[0, 9]) and np.all(r["good"] == 1) and (const is None or np.array_equal(const, c8))
                const = c8
                out[f"{k}{l}/xy"] = xy; out[f"{k}{l}/type"] = fl[:, 8].astype(np.uint8)
                assert np.array_equal(out[f"{k}{l}/type"].astype(f32), fl[:, 8])
                out[f"{k}{l}/nbd"] = r["nbd"]; out[f"{k}{l}/pard"] = r["pard"]
            out[k + "const"] = const
            res = record_nn(R, ic, [r["fields"][:, :2] for r in lv], k[:-1], out)
            for l, r in enumerate(lv):          # makeNN on the positions alone gives what setFirst's own makeNN gave
                assert np.array_equal(res[l]["nb"], r["nb"]) and np.array_equal(res[l]["par"], r["par"]) and np.array_equal(res[l]["nbd"], r["nbd"]) and np.array_equal(res[l]["pard"], r["pard"])
            print("setFirst", name, "numPoints", n.tolist(), "sparsity", s0, "->", s1)
            L.if_frame_free(f)
        if a.large:
            path = a.out or ic.GOLDEN_LARGE
            depth = binding_depth(ic.pos(out["first/large_scene/0/xy"]))
            print("depth of the level-0 tree:", depth)
            assert depth >= ic.LARGE_MIN_DEPTH
            np.savez_compressed(path, **out)
            print(f"{path}: {os.path.getsize(path)} bytes")
            assert os.path.getsize(path) <= 600 * 1024
            return
        a.out = a.out or ic.GOLDEN
        assert int(out["first/scene/meta"][4]) != 5, "the first frame must move the sparsity, or the second one covers no carried value"
        # ---- makePixelStatus cases -----------------------------------------------------------------------------------------------------------------
        found = {}
        for case, name, lvl, sp, rec, thf, dens in ic.STATUS_CASES:
            img = ic.image(name)
            h, w = img.shape
            R = Ref(L, w, h, ic.levels_of(name), ic.K4[w])
            f = R.frame(img)
            if dens == "search":
                cands = [float(f32(d)) for d in (5, 10, 20, 40, 80, 150, 300, 600, 1200, 2400, 4800)]
                want = (lambda ps: ps >= 3) if case == "two_recursions" else (lambda ps: ps >= 2)
                dens = next(d for d in cands if want(R.status_passes(f, lvl, sp, d, 5, thf)[1]) and (case != "two_recursions" or R.status_passes(f, lvl, sp, d, 1, thf)[1] == 2))
                found[case] = dens
            elif isinstance(dens, str):
                dens = found["two_recursions"]
            (ret, m, left), passes = R.status_passes(f, lvl, sp, dens, rec, thf)
            natural = R.status_passes(f, lvl, sp, dens, 5, thf)[1]
            o = np.array([ret, passes, left], np.int32)
            ic.check_status_property(case, w >> lvl, h >> lvl, sp, o, rec, natural)
            if case == "steps_ties":
                assert ic.block_has_tie(synth.make_images(img, lvl + 1)[lvl], sp, thf)
            if case == "th_half":          # nothing passes THFac = 1 at any block size, so what was selected came through THFac = 0.5
                assert all(R.status(f, lvl, q, dens, 0, 1.0)[0] == 0 for q in (1, 2, 5)) and ret > 0
            k = f"status/{case}/"
            out[k + "image"] = np.array(name); out[k + "args"] = np.array([dens, thf], f32); out[k + "iargs"] = np.array([lvl, sp, rec], np.int32)
            out[k + "out"] = o; out[k + "map"] = np.packbits(m)
            assert ret == int(m.sum())
            print("status", case, "density", dens, "out", o.tolist(), "natural passes", natural)
            L.if_frame_free(f)
        # ---- the decisions of makePixelStatus on a grid, observed from outside ------------------------------------------------------------------------
        rows_i, rows_f, rows_o = [], [], []
        for name, lvl in (("scene", 1), ("scene", 2), ("ramp", 1), ("flat", 1)):
            img = ic.image(name)
            h, w = img.shape
            R = Ref(L, w, h, 4, ic.K4[w])
            f = R.frame(img)
            for sp in (1, 2, 5, 12):
                for thf in (1.0, 0.5):
                    have = R.status(f, lvl, sp, 100.0, 0, thf)[0]
                    dens = [100.0] if have == 0 else []
                    if have:
                        for q in (0.1, 0.5, 0.8, 1.0, 1.25, 2.0, 6.0):          # quotia = have / desired
                            d = f32(have / q)
                            dens += [float(np.nextafter(d, f32(0))), float(d), float(np.nextafter(d, f32(1e9)))] if q in (0.8, 1.25) else [float(d)]
                    for d in dens:
                        first = R.status(f, lvl, sp, d, 0, thf)
                        for rec in (0, 1, 5):
                            if rec == 0:
                                act = 0
                            else:
                                r = R.status(f, lvl, sp, d, rec, thf)
                                differs = not (r[0] == first[0] and r[2] == first[2] and np.array_equal(r[1], first[1]))
                                if differs:
                                    act = 1
                                else:          # no recursion is proven when the pass it would have run leaves something else behind
                                    second = [R.status(f, lvl, first[2], d, 0, t) for t in {thf, 0.5}]
                                    act = 0 if all(not (s[0] == first[0] and s[2] == first[2] and np.array_equal(s[1], first[1])) for s in second) else -1
                            rows_i.append([first[0], sp, rec]); rows_f.append([d, thf]); rows_o.append([act, first[2]])
            L.if_frame_free(f)
        out["plan_in"], out["plan_f"], out["plan_out"] = np.array(rows_i, np.int32), np.array(rows_f, f32), np.array(rows_o, np.int32)
        po, pi = out["plan_out"], out["plan_in"]
        print("plan rows", len(po), "recursing", int((po[:, 0] == 1).sum()), "staying", int((po[:, 0] == 0).sum()), "not visible", int((po[:, 0] == -1).sum()))
        assert (pi[:, 0] == 0).any() and ((po[:, 0] == 1) & (pi[:, 1] == 1) & (po[:, 1] == 1)).any(), "a count of 0 and the THFac = 0.5 branch must be among the rows"
        assert ((po[:, 0] == 0) & (pi[:, 2] > 0) & (po[:, 1] != pi[:, 1])).any() and (po[:, 0] == 1).any(), "both sides of the 0.8 boundaries must be visible"
        # ---- makeNN on synthetic position sets -----------------------------------------------------------------------------------------------------------
        R = Ref(L, 160, 96, 4, ic.K4[160])
        differs_from_tidy = 0
        for name in ic.NN_SETS:
            xy = ic.nn_set(name)
            uv = [ic.pos(q) for q in xy]
            out[f"nn/{name}/levels"] = np.array(len(xy), np.int32)
            for l, q in enumerate(xy):
                out[f"nn/{name}/{l}/xy"] = q
            res = record_nn(R, ic, uv, f"nn/{name}", out)
            for l, r in enumerate(res):
                if len(uv[l]) > 10:
                    ti, td = ic.tidy_order(uv[l])
                    assert np.array_equal(td[:, :10], r["d10"]), name          # the same distances in any case
                    differs_from_tidy += int((ti[:, :10] != r["nb"]).any(1).sum())
                    if name == "grid" and l == 0:
                        share = ic.tie_share(td[:, 9], td[:, 10])
                        print("grid: rows tied at the 10th distance", share)
                        assert share >= 0.5
            print("nn", name, [len(q) for q in xy])
        print("rows that differ from the (distance, index) order:", differs_from_tidy)
        assert differs_from_tidy > 0
        np.savez_compressed(a.out, **out)
        print(f"{a.out}: {os.path.getsize(a.out)} bytes")
        assert os.path.getsize(a.out) <= 550 * 1024


if __name__ == "__main__":
    main()
