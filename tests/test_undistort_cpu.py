"""The device undistorter without a device: the numpy restatement (tests/undistort_common.py) against the outputs recorded from the reference's own
Undistort::undistort<T> (tests/golden/ref_undistort.npz), the properties of the recorded tables, and ldso_amd/csrc/undistort_px.h - the one pixel
function the kernel of undistort.hip runs - compiled with g++ into a stand-alone program under AddressSanitizer / UBSan on heap buffers of exactly
wOrg * hOrg elements: the fixture outputs bit for bit, zeros for table entries whose taps leave the image, and no read outside the raw frame."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import undistort_common as uc
from ldso_amd import binding, build as ldso_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (key of the recorded output, raw frame, response, photometricCalibration, exposure, factor)
RUNS = (("u8_m2", "raw8", "G256", 2, uc.EXPOSURE, 1.0), ("u8_m1", "raw8", "G256", 1, uc.EXPOSURE, 1.0), ("u8_m0", "raw8", "G256", 0, uc.EXPOSURE, 1.0),
        ("u8_e0", "raw8", "G256", 2, 0.0, 0.7), ("u16_m2", "raw16", "G65536", 2, uc.EXPOSURE, 1.0))
# the same for the outputs of which the fixture holds every uc.SAMPLE_ROWS-th row
RUNS_ROWS = (("u16_m1_rows", "raw16", "G65536", 1, uc.EXPOSURE, 1.0), ("u16_e0_rows", "raw16", "G65536", 2, 0.0, 1.0 / 256))


def same_bits(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("c", uc.CASES)
def test_restatement_equals_the_recorded_reference_outputs(c):
    g = uc.golden()
    w_org, h_org, w, h, rx, ry = uc.case(c)
    for key, raw, G, pc, exposure, factor in RUNS + RUNS_ROWS:
        mode = uc.mode_of(g[G], exposure, pc)
        out = uc.undistort(g[raw], rx, ry, w_org, h_org, w, h, g[G], g["vignetteMapInv"], mode, factor)
        if key.endswith("_rows"):
            out = out[::uc.SAMPLE_ROWS]
        ref = g[f"{c}_{key}"]
        assert out.shape == ref.shape and same_bits(out, ref), (c, key, int((out != ref).sum()))
    assert np.isinf(g["vignetteMapInv"]).sum() == 1          # the pixel whose vignette is 0: multiplied in as infinity
    assert not np.isfinite(g[c + "_u8_m2"]).all() and np.isfinite(g[c + "_u8_m1"]).all()
    assert tuple(g[c + "_exposure"]) == (np.float32(uc.EXPOSURE), 0.0, 1.0)          # useExposure on; on with exposure 0; off


def test_recorded_tables_never_over_read_and_case_b_exercises_both_branches():
    g = uc.golden()
    for c in uc.CASES:
        w_org, h_org, w, h, rx, ry = uc.case(c)
        invalid, zeroed, over = (int(v) for v in g[c + "_table_classes"])
        assert over == 0
        if rx is None:
            assert c == "C" and zeroed == 120          # what the reference's loop would zero if a passthrough read its tables
            continue
        k = uc.classify(rx, ry, w_org, h_org)
        assert (k["invalid"], k["zeroed"], k["overread"]) == (invalid, zeroed, 0)
        ok, _, _ = uc.taps_inside(rx, ry, w_org, h_org)
        assert (~ok).sum() == invalid + zeroed          # without an over-reading entry the device's rule and the reference's zero the same pixels
    rx, ry = g["B_remapX"], g["B_remapY"]
    ok, _, _ = uc.taps_inside(rx, ry, 120, 90)
    assert 0.05 < (~ok).mean() < 0.50
    assert uc.classify(g["A_remapX"], g["A_remapY"], 120, 90) == dict(invalid=0, zeroed=0, overread=0)


def test_helpers_tell_the_over_reading_entry_from_the_zeroed_ones():
    """a check of tests/undistort_common.py itself (classify / taps_inside are what the other tests lean on), not of the product: undistort_px.h is
    covered by the sanitizer program below"""
    # the entry the issue measured (xxi == 0, yyi == hOrg - 1) passes the reference's range check and reads one row past the image
    k = uc.classify(np.float32([0.5]), np.float32([89.0]), 120, 90)
    assert k == dict(invalid=0, zeroed=0, overread=1)
    ax, ay = uc.adversarial_entries(120, 90)
    ok, _, _ = uc.taps_inside(ax, ay, 120, 90)
    assert not ok.any()
    f8, _ = uc.textured_frames(120, 90)
    assert not uc.undistort(f8, ax, ay, 120, 90, len(ax), 1).any()


PROGRAM = r'''
// one line of the job file per run: wOrg hOrg n bpp mode factor passthrough GDepth raw G vig remapX remapY expected ("-" = none)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "undistort_px.h"

template <class T> static T *load(const char *path, size_t n) {          // a heap block of exactly n elements
    if (!strcmp(path, "-")) return nullptr;
    T *p = new T[n];
    FILE *f = fopen(path, "rb");
    if (!f || fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "short file %s\n", path); exit(2); }
    fclose(f);
    return p;
}

int main(int argc, char **argv) {
    FILE *jobs = fopen(argv[1], "r");
    if (!jobs) return 2;
    int wOrg, hOrg, n, bpp, mode, pass, GDepth, bad = 0, runs = 0;
    float factor;
    char raw[512], G[512], vig[512], rx[512], ry[512], ex[512];
    while (fscanf(jobs, "%d %d %d %d %d %f %d %d %511s %511s %511s %511s %511s %511s", &wOrg, &hOrg, &n, &bpp, &mode, &factor, &pass, &GDepth, raw, G, vig, rx, ry, ex) == 14) {
        const size_t nOrg = (size_t) wOrg * hOrg;
        unsigned char *r = load<unsigned char>(raw, nOrg * bpp);
        float *g = load<float>(G, GDepth), *v = load<float>(vig, nOrg), *x = load<float>(rx, n), *y = load<float>(ry, n), *e = load<float>(ex, n);
        int miss = 0;
        for (int i = 0; i < n; i++) {
            const float o = pass ? undist_photo(r, bpp, i, g, v, mode, factor) : undist_px(r, bpp, g, v, mode, factor, x[i], y[i], wOrg, hOrg);
            if (memcmp(&o, e + i, 4) != 0 && !(std::isnan(o) && std::isnan(e[i]))) miss++;
        }
        printf("run %d: %d pixels, %d differ\n", runs++, n, miss);
        bad += miss;
        delete[] r; delete[] g; delete[] v; delete[] x; delete[] y; delete[] e;
    }
    printf("runs %d bad %d\n", runs, bad);
    return bad ? 1 : 0;
}
'''


def test_pixel_function_under_sanitizers_reproduces_the_fixture_and_never_leaves_the_frame():
    g = uc.golden()
    d = tempfile.mkdtemp(prefix="undist_px_")
    src, exe = os.path.join(d, "px.cc"), os.path.join(d, "px")
    open(src, "w").write(PROGRAM)
    san = ["-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all"]
    probe = subprocess.run(["g++", *san, "-x", "c++", "-", "-o", os.path.join(d, "probe")], input="int main() { return 0; }\n", capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("the sanitizer runtime cannot be linked here: " + probe.stderr[-300:])
    subprocess.run(["g++", "-O1", "-g", "-ffp-contract=off", *san, "-I", os.path.join(ROOT, "ldso_amd", "csrc"), src, "-o", exe], check=True)

    def put(name, a):
        if a is None:
            return "-"
        p = os.path.join(d, name)
        np.ascontiguousarray(a).tofile(p)
        return p

    jobs, expected_runs = [], 0
    vig = put("vig", g["vignetteMapInv"])
    for c in uc.CASES:
        w_org, h_org, w, h, rx, ry = uc.case(c)
        for key, raw, G, pc, exposure, factor in RUNS:
            mode = uc.mode_of(g[G], exposure, pc)
            # the plain path gets no tables at all: it must not touch them
            jobs.append(f"{w_org} {h_org} {w * h} {g[raw].dtype.itemsize} {mode} {factor!r} {int(rx is None)} {len(g[G])} {put(raw, g[raw])} "
                        f"{put(G, g[G]) if mode else '-'} {vig if mode == 2 else '-'} {put(c + 'rx', rx)} {put(c + 'ry', ry)} {put(c + key, g[c + '_' + key])}")
            expected_runs += 1
        for key, raw, G, pc, exposure, factor in RUNS_ROWS:
            if rx is None:
                continue
            mode = uc.mode_of(g[G], exposure, pc)
            sx, sy = rx[::uc.SAMPLE_ROWS], ry[::uc.SAMPLE_ROWS]
            jobs.append(f"{w_org} {h_org} {sx.size} 2 {mode} {factor!r} 0 {len(g[G])} {put(raw, g[raw])} {put(G, g[G]) if mode else '-'} - "
                        f"{put(c + 'sx', sx)} {put(c + 'sy', sy)} {put(c + key, g[c + '_' + key])}")
            expected_runs += 1
    # adversarial entries on the 8- and the 16-bit frame, every path: 0, and nothing outside the wOrg * hOrg block is read
    ax, ay = uc.adversarial_entries(120, 90)
    zeros = put("zeros", np.zeros(len(ax), np.float32))
    for raw, G in (("raw8", "G256"), ("raw16", "G65536")):
        for mode in (0, 1, 2):
            jobs.append(f"120 90 {len(ax)} {g[raw].dtype.itemsize} {mode} 1.0 0 {len(g[G])} {put(raw, g[raw])} {put(G, g[G]) if mode else '-'} {vig if mode == 2 else '-'} "
                        f"{put('ax', ax)} {put('ay', ay)} {zeros}")
            expected_runs += 1
    # a synthetic table that keeps rows beyond hOrg - 1 (the reference's validity rule), against the restatement
    rx, ry = uc.synthetic_tables(67, 53, 33, 29)
    f8, _ = uc.textured_frames(67, 53)
    assert 0 < (~uc.taps_inside(rx, ry, 67, 53)[0]).sum() < rx.size
    jobs.append(f"67 53 {rx.size} 1 0 0.5 0 0 {put('s8', f8)} - - {put('srx', rx)} {put('sry', ry)} {put('sexp', uc.undistort(f8, rx, ry, 67, 53, 33, 29, factor=0.5))}")
    expected_runs += 1
    jobfile = os.path.join(d, "jobs.txt")
    open(jobfile, "w").write("\n".join(jobs) + "\n")
    r = subprocess.run([exe, jobfile], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert f"runs {expected_runs} bad 0" in r.stdout, r.stdout[-2000:]


def test_create_without_a_device_reports_nodevice():
    if not os.path.exists(binding.lib_path()):
        ldso_build.build()
    if binding.lib().ldso_device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(binding.LdsoError) as e:
        binding.Undistorter(120, 90, 104, 72)
    assert e.value.code == -5
