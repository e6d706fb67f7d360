"""ldso_feat_group_* (include/ldso_hip.h) without a device: the five entries are exported by the built library and declared in the header, refuse a NULL group /
NULL members before they touch the runtime, and the binding offers them.  feat_group_layout of ldso_amd/csrc/group_stage.h - where the job table, the four prefix
tables and the control rows of a grouped detection lie in the group's arena - is compiled with g++ into a stand-alone program under AddressSanitizer / UBSan:
every arena is a heap block of exactly the size the layout reports and every region is filled at its offset, so a region that reaches past its arena ends the
program.  The four prefix tables (cells, compaction, corners and records, angle + descriptor) are built with group_prefix from grids that include empty ones and
searched with group_member_of for every unit."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest

from ldso_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ldso_hip.h")
LDSO_OK, LDSO_E_INVALID = 0, -1
ENTRIES = ("ldso_feat_group_create", "ldso_feat_group_destroy", "ldso_feat_group_detect", "ldso_feat_group_get", "ldso_feat_group_profile")

PROGRAM = r'''
#include <cstdio>
#include <cstdlib>
#include "group_stage.h"

void ldso_set_error(const std::string &) {}

static int g_bad = 0, g_calls = 0;
#define EXPECT(c) do { if (!(c)) { g_bad++; if (g_bad < 20) printf("line %d: %s\n", __LINE__, #c); } } while (0)

struct Region { size_t at, bytes; };

constexpr size_t FEATJOB = 128;          // sizeof(FeatArgs): ten pointers, the grid's eight words and three ints with their padding (features.hip)

// one job's grid: cells and picks per cell (0 cells: a grid the image has no room for)
struct Job { int cells, perCell; };
static int cap(const Job &j) { return j.cells * j.perCell; }

static void one(const std::vector<Job> &jobs) {
    g_calls++;
    const size_t nj = jobs.size();
    const FeatGroupLayout L = feat_group_layout(nj, FEATJOB);
    EXPECT(L.jobs == 0 && L.downBytes == nj * 8 * 4 && L.total == L.down + L.downBytes);
    const std::vector<Region> R = {{L.jobs, nj * FEATJOB}, {L.firstCells, (nj + 1) * 4}, {L.firstCompact, (nj + 1) * 4}, {L.firstCorners, (nj + 1) * 4},
                                   {L.firstDescribe, (nj + 1) * 4}, {L.down, L.downBytes}};
    unsigned char *blk = (unsigned char *) malloc(L.total);          // exactly `total` bytes
    for (size_t a = 0; a < R.size(); a++) {
        EXPECT(R[a].at % 16 == 0 && R[a].at + R[a].bytes <= L.total);
        memset(blk + R[a].at, (int) a + 1, R[a].bytes);          // past the block: the sanitizer ends the program
    }
    for (size_t a = 0; a < R.size(); a++) {
        for (size_t b = a + 1; b < R.size(); b++) EXPECT(R[a].at + R[a].bytes <= R[b].at || R[b].at + R[b].bytes <= R[a].at);
        bool kept = true;                                          // no later region wrote into this one
        for (size_t i = 0; i < R[a].bytes; i++) kept = kept && blk[R[a].at + i] == (unsigned char) (a + 1);
        EXPECT(kept);
    }
    EXPECT(L.down % 16 == 0 && L.down + L.downBytes <= L.total);          // the download region lies inside the block
    // the four prefix tables, written where the layout puts them, then searched for every unit
    const int n = (int) nj;
    const size_t at[4] = {L.firstCells, L.firstCompact, L.firstCorners, L.firstDescribe};
    for (int t = 0; t < 4; t++) {
        const auto units = [&](int j) {
            const Job &J = jobs[(size_t) j];
            return t == 0 ? J.cells : t == 1 ? (J.cells > 0 ? 1 : 0) : t == 2 ? (cap(J) + 255) / 256 : (cap(J) + 3) / 4;
        };
        int *first = (int *) (blk + at[t]);
        const int total = group_prefix(n, first, units);
        EXPECT(first[0] == 0 && first[n] == total);
        int u = 0;
        for (int j = 0; j < n; j++) {
            EXPECT(first[j] == u && first[j + 1] - first[j] == units(j));
            for (int k = 0; k < units(j); k++, u++) {
                const int m = group_member_of(first, n, u);          // never a job without units, wherever it stands
                EXPECT(m == j && u - first[m] == k);
            }
            if (t == 2 && cap(jobs[(size_t) j]) > 0) EXPECT((units(j) - 1) * 256 < cap(jobs[(size_t) j]) && units(j) * 256 >= cap(jobs[(size_t) j]));
            if (t == 3 && cap(jobs[(size_t) j]) > 0) EXPECT((units(j) - 1) * 4 < cap(jobs[(size_t) j]) && units(j) * 4 >= cap(jobs[(size_t) j]));
        }
        EXPECT(u == total);
    }
    free(blk);
}

int main() {
    // the grids of the GPU test and of 640 x 480 with 1500 wanted features, a grid without cells, one cell, capacities around 256 and 4
    const Job pool[] = {{88, 2}, {12, 2}, {228, 1}, {1218, 2}, {0, 1}, {1160, 2}, {1, 1}, {0, 3}, {256, 1}, {257, 1}, {3, 1}, {5, 1}, {128, 2}};
    for (size_t nj : {1, 2, 7, 128}) for (size_t shift = 0; shift < 13; shift++) {
        std::vector<Job> jobs(nj);
        for (size_t j = 0; j < nj; j++) jobs[j] = pool[(j * 5 + shift) % 13];
        one(jobs);
    }
    one({{0, 1}});                                    // nothing to launch at all
    one({{0, 1}, {0, 2}, {7, 1}, {0, 1}, {0, 1}});     // empty jobs at both ends
    std::vector<Job> many(128);
    for (int j = 0; j < 128; j++) many[(size_t) j] = j % 3 == 0 || j == 127 ? Job{0, 1} : Job{10 * j + 1, 1 + j % 2};
    one(many);
    printf("calls %d bad %d\n", g_calls, g_bad);
    return g_bad ? 1 : 0;
}
'''


@pytest.mark.parametrize("entry", ENTRIES)
def test_entry_is_exported_and_declared(entry):
    assert hasattr(binding.lib(), entry)
    assert re.search(r"\bint\s+%s\s*\(" % entry, open(HEADER).read())


def test_header_names_the_reference_lines_and_the_stricter_room_rule():
    """in the comment right above the group's typedef, and in the one above ldso_feat_group_detect"""
    text = open(HEADER).read()
    end = text.index("typedef struct ldso_feat_group ")
    comment = text[text.rindex("/*", 0, end):end]
    assert "FullSystem.cc:1272-1325" in comment and "FeatureDetector.cc:34-130" in comment
    first = text.index("int ldso_feat_group_detect(")
    comment = text[text.rindex("/*", 0, first):first]
    assert "stricter" in comment and "max_points" in comment


@pytest.mark.parametrize("entry,nargs", [("ldso_feat_group_detect", 9), ("ldso_feat_group_get", 4), ("ldso_feat_group_profile", 3)])
def test_null_group_is_refused_with_a_message(entry, nargs):
    L = binding.lib()
    f = getattr(L, entry)
    f.restype = C.c_int
    f.argtypes = [C.c_void_p] * nargs
    assert f(*([None] * nargs)) == LDSO_E_INVALID
    assert entry in L.ldso_last_error().decode()


def test_create_refuses_bad_member_lists():
    L = binding.lib()
    entry = "ldso_feat_group_create"
    f = getattr(L, entry)
    f.restype = C.c_int
    out = C.c_void_p()
    assert f(None, C.c_int(1), C.byref(out)) == LDSO_E_INVALID          # NULL members
    assert entry in L.ldso_last_error().decode()
    assert not out.value
    empty = (C.c_void_p * 1)()
    assert f(empty, C.c_int(0), C.byref(out)) == LDSO_E_INVALID and not out.value
    assert f(empty, C.c_int(1), C.byref(out)) == LDSO_E_INVALID and not out.value          # a NULL member
    assert entry in L.ldso_last_error().decode() and "detector" in L.ldso_last_error().decode()
    assert f(empty, C.c_int(129), C.byref(out)) == LDSO_E_INVALID and not out.value
    assert f(empty, C.c_int(1), None) == LDSO_E_INVALID


def test_group_destroy_of_null_is_a_no_op():
    assert binding.lib().ldso_feat_group_destroy(None) == LDSO_OK


@pytest.mark.parametrize("method", ("detect", "get", "profile", "close"))
def test_binding_offers_the_method(method):
    assert callable(getattr(getattr(binding, "FeaturesGroup", None), method, None))


def test_layout_and_prefix_tables_under_sanitizers():
    d = tempfile.mkdtemp(prefix="feat_stage_")
    src, exe = os.path.join(d, "stage.cc"), os.path.join(d, "stage")
    open(src, "w").write(PROGRAM)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = subprocess.run(["g++", *san, "-x", "c++", "-", "-o", os.path.join(d, "probe")], input="int main() { return 0; }\n", capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("the sanitizer runtime cannot be linked here: " + probe.stderr[-300:])
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *san, "-I", os.path.join(ROOT, "ldso_amd", "csrc"), src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    m = re.search(r"calls (\d+) bad 0\n", r.stdout)
    assert m, r.stdout[-2000:]
    assert int(m.group(1)) > 50          # an empty run cannot pass
