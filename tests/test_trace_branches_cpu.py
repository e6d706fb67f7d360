"""What the branch scene of tests/trace_branch_common.py reaches, asserted from the oracle's own per-point diagnostics (orc_trace_on_diag: the same function
body as orc_trace_on), so that tests/test_trace_branches_gpu.py does not claim coverage it does not have; and, where oracle/_ref is built, the oracle against the
reference's own ImmaturePoint::traceOn on every call of the scene, byte for byte.  No GPU."""
import numpy as np
import pytest

import trace_branch_common as tb
from oracle import pyoracle as po, pyref as pr

BITS = po.TD_BITS


@pytest.fixture(scope="module")
def diags():
    """per call: list (one entry per trace) of (counts, records, diag, status before the trace)"""
    sc = tb.scene()
    KRKi, Kt, aff = sc["hosts"]
    out = {}
    for c in sc["calls"]:
        pts = c["pts"].copy()
        plain = tb.oracle(c["name"])
        rows = []
        for t in range(2 if c["second"] else 1):
            before = pts["lastTraceStatus"].copy()
            counts, diag = po.trace_on_diag(pts, sc[c["image"]], KRKi, Kt, aff, c["settings"])
            # the diagnostics entry writes the records and counts of orc_trace_on
            assert np.array_equal(counts, plain[t][0]) and pts.tobytes() == plain[t][1].tobytes(), (c["name"], t)
            rows.append((counts, pts.copy(), diag, before))
        out[c["name"]] = rows
    return out


def _all(diags):
    return np.concatenate([d for rows in diags.values() for _, _, d, _ in rows])


def test_searches_stay_inside_the_image_and_find_a_step(diags):
    """every 2 x 2 tap of every call lies inside the image with a pixel to spare (the device reads the same addresses), and every point that reached the search has a
    best step: bestIdx < 0 (refinement around (0, 0), guarded in the oracle and the kernel) is not part of these calls"""
    for name, rows in diags.items():
        for _, _, d, _ in rows:
            searched = d[:, po.TD_NUMSTEPS] > 0
            assert searched.any() or name == "single"
            assert (d[searched, po.TD_MARGIN] >= 1).all(), (name, d[searched, po.TD_MARGIN].min())
            assert (d[searched, po.TD_BESTIDX] >= 0).all(), name
            assert (d[~searched, po.TD_BESTIDX] == 0).all()


def test_second_pass_is_reached(diags):
    """best steps in the second pass, right behind its start and at its end; step counts 64, 65, the clamp at 99, and all 33 step counts in 66..98"""
    d = _all(diags)
    best = d[d[:, po.TD_NUMSTEPS] > 0, po.TD_BESTIDX]
    assert (best >= 64).sum() >= 20
    assert ((best >= 64) & (best <= 66)).sum() >= 5
    assert (best >= 96).sum() >= 5
    steps = set(d[:, po.TD_NUMSTEPS].tolist())
    assert {64, 65, 99} <= steps
    assert set(range(66, 99)) <= steps
    first = diags["finite"][0][2][:, po.TD_NUMSTEPS]
    assert len(set(first.tolist()) & set(range(3, 100))) >= 90          # one call with (nearly) every step count


def test_tied_best_energies(diags):
    d = _all(diags)
    tied = d[:, po.TD_TIES] >= 2
    assert tied.sum() >= 20
    assert (tied & (d[:, po.TD_TIE_LO] < 64) & (d[:, po.TD_TIE_HI] >= 64)).sum() >= 5


def test_both_forms_of_the_new_interval(diags):
    good = ydom = 0
    for rows in diags.values():
        for _, pts, d, _ in rows:
            g = (pts["lastTraceStatus"] == 0) & (d[:, po.TD_NUMSTEPS] > 0)
            good += g.sum(); ydom += (g & ((d[:, po.TD_MASK] & BITS["y_dominant"]) != 0)).sum()
    assert good > 200 and 0.3 <= ydom / good <= 0.7, (ydom, good)


def test_every_branch_bit_is_set(diags):
    """every branch of the mask at least 3 times.  Non-finite dx is reached by design in the call "slack0" (trace_slackInterval = 0 lets an interval of width zero
    through: dist = 0, dx = 0 / 0), and the oracle does reach it there, so it is required like the others.  step_nonfinite needs a non-finite image GRADIENT, which
    makeImages never produces: the call "gradnan" passes one through the plain frame entry."""
    m = _all(diags)[:, po.TD_MASK]
    counts = {name: int(((m & bit) != 0).sum()) for name, bit in BITS.items()}
    assert all(v >= 3 for v in counts.values()), counts
    slack0 = diags["slack0"][0][2][:, po.TD_MASK]
    assert ((slack0 & BITS["dx_nonfinite"]) != 0).sum() >= 3
    assert ((_all({k: v for k, v in diags.items() if k != "slack0"})[:, po.TD_MASK] & BITS["dx_nonfinite"]) != 0).sum() == 0


def test_every_status_occurs_and_outlier_twice_is_oob(diags):
    seen = set()
    twice = 0
    for name, rows in diags.items():
        for _, pts, d, before in rows:
            seen |= set(pts["lastTraceStatus"].tolist())
            twice += ((before == 2) & (pts["lastTraceStatus"] == 1) & (d[:, po.TD_NUMSTEPS] > 0)).sum()
    assert {0, 1, 2, 3, 4} <= seen
    assert twice >= 3
    # a host outside [0, n_hosts) leaves the record alone
    c = tb.get_call("inf85")
    bad = (c["pts"]["host"] < 0) | (c["pts"]["host"] >= tb.N_HOSTS)
    assert bad.sum() >= 3 and diags["inf85"][1][1][bad].tobytes() == c["pts"][bad].tobytes()


def test_settings_change_the_result(diags):
    """each non-default setting is visible in the oracle's records, so a kernel that ignored it could not match"""
    base = diags["finite"][0][1]
    for name in ("gn0", "radius0", "radius120", "step05", "step2", "slack0"):
        assert diags[name][0][1].tobytes() != base.tobytes(), name
    assert (diags["gn0"][0][2][:, po.TD_GNITS] == 0).all() and (diags["finite"][0][2][:, po.TD_GNITS] > 0).any()


@pytest.mark.skipif(not pr.available(), reason="oracle/_ref/libldso_ref.so missing and /root/reference not present to build it")
@pytest.mark.parametrize("name", tb.call_names())
def test_oracle_matches_reference_on_every_call(name):
    ref = tb.run(tb.get_call(name), pr.trace_on)
    for (co, po_pts), (cr, pr_pts) in zip(tb.oracle(name), ref):
        assert np.array_equal(co, cr), (co, cr)
        assert po_pts.tobytes() == pr_pts.tobytes()


# A stand-alone program around orc_trace_on for one point whose colour is NaN: every search energy is NaN, no step is valid, and the reference's refinement would
# sample around (0, 0) - pattern pixel (0, -2) lies two rows, (-2, 0) six floats in front of the image.  The image is a heap block of exactly w * h * 3 floats, so AddressSanitizer sees
# any read outside it.  Prints the status after a first trace and after a second (previous status OUTLIER).
GUARD_PROGRAM = r'''
#include <cmath>
#include <cstdio>
#include <cstring>
#include "ldso_window.h"
extern "C" void orc_trace_settings_default(ldso_trace_settings_t *s);
extern "C" void orc_trace_on(int n, ldso_immature_t *pts, const float *dI, int w, int h, int n_hosts, const float *KRKi, const float *Kt, const float *aff,
                             const ldso_trace_settings_t *s, int *counts);
int main() {
    const int w = 640, h = 480;
    float *img = new float[(size_t) w * h * 3];
    for (int y = 0; y < h; y++) for (int x = 0; x < w; x++) { float *p = img + 3 * (x + y * w); p[0] = 100 + 50 * sinf(0.3f * x) * cosf(0.2f * y); p[1] = 1; p[2] = -1; }
    ldso_immature_t p;
    memset(&p, 0, sizeof(p));
    p.u = 300; p.v = 200; p.energyTH = 1152; p.idepth_min = 0; p.idepth_max = NAN; p.quality = 10000; p.lastTraceStatus = LDSO_IPS_UNINITIALIZED; p.host = 0;
    for (int k = 0; k < 8; k++) { p.color[k] = 100; p.weights[k] = 1; }
    p.color[3] = NAN;
    p.gradH[0] = p.gradH[3] = 10;
    const float KRKi[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, Kt[3] = {100, 0, 0}, aff[2] = {1, 0};
    ldso_trace_settings_t s;
    orc_trace_settings_default(&s);
    int counts[6];
    orc_trace_on(1, &p, img, w, h, 1, KRKi, Kt, aff, &s, counts);
    printf("%d %g ", p.lastTraceStatus, p.quality);
    orc_trace_on(1, &p, img, w, h, 1, KRKi, Kt, aff, &s, counts);
    printf("%d %g\n", p.lastTraceStatus, p.quality);
    delete[] img;
    return 0;
}
'''


def test_no_valid_step_reads_nothing_under_address_sanitizer():
    """oracle/trace.cc compiled with -fsanitize=address into a stand-alone program: with no valid search step the refinement reads nothing (before the guard
    AddressSanitizer stops the same program at a read in front of the image: interp33 from the refinement loop, pattern pixel (0, -2) two rows ahead of the block), and
    the point is OUTLIER, then OOB, with quality 1e10 / 1e10"""
    import os
    import subprocess
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d = tempfile.mkdtemp(prefix="trace_guard_")
    src, exe = os.path.join(d, "guard.cc"), os.path.join(d, "guard")
    open(src, "w").write(GUARD_PROGRAM)
    san = ["-fsanitize=address", "-fno-sanitize-recover=all"]
    probe = subprocess.run(["g++", *san, "-x", "c++", "-", "-o", os.path.join(d, "probe")], input="int main() { return 0; }\n", capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("the sanitizer runtime cannot be linked here: " + probe.stderr[-300:])
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", *san, "-I", os.path.join(root, "include"), src, os.path.join(root, "oracle", "trace.cc"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})
    assert r.returncode == 0 and "AddressSanitizer" not in r.stderr, r.stderr[-2000:]
    assert r.stdout.split() == ["2", "1", "1", "1"], r.stdout
