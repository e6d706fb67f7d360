"""ldso_trace_group_compact and ldso_ba_batch_select_activate_tracers (include/ldso_hip.h) without a device.  compact_group_layout of ldso_amd/csrc/group_stage.h - where
the job table, the prefix table, the host maps, every job's keep bytes and the counts of a grouped compaction lie in the group's arena - is compiled with g++ into a
stand-alone program under AddressSanitizer / UBSan: every arena is a heap block of exactly the size the layout reports and every region is filled at its offset, so a
region that reaches past its arena ends the program.  The prefix table of the two grouped kernels (a workgroup per 256 records) is searched for every workgroup.
Both entries are exported, refuse a NULL group / batch before they touch the runtime, and the binding offers them with a job record of the header's size."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest

from ldso_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDSO_E_INVALID = -1

PROGRAM = r'''
#include <cstdio>
#include <cstdlib>
#include "group_stage.h"

void ldso_set_error(const std::string &) {}

static int g_bad = 0, g_calls = 0;
#define EXPECT(c) do { if (!(c)) { g_bad++; if (g_bad < 20) printf("line %d: %s\n", __LINE__, #c); } } while (0)

struct Region { size_t at, bytes, align; };

static void check_arena(const std::vector<Region> &R, size_t total, size_t downAt, size_t downBytes) {
    g_calls++;
    unsigned char *blk = (unsigned char *) malloc(total);
    for (size_t a = 0; a < R.size(); a++) {
        EXPECT(R[a].at % R[a].align == 0 && R[a].at + R[a].bytes <= total);
        memset(blk + R[a].at, (int) (a % 251) + 1, R[a].bytes);          // past the block: the sanitizer ends the program
    }
    for (size_t a = 0; a < R.size(); a++) {
        for (size_t b = a + 1; b < R.size(); b++) if (R[a].bytes && R[b].bytes) EXPECT(R[a].at + R[a].bytes <= R[b].at || R[b].at + R[b].bytes <= R[a].at);
        bool kept = true;                                                                                             // no later region wrote into this one
        for (size_t i = 0; i < R[a].bytes; i++) kept = kept && blk[R[a].at + i] == (unsigned char) ((a % 251) + 1);
        EXPECT(kept);
    }
    EXPECT(downAt + downBytes <= total && downAt % 16 == 0);
    free(blk);
}

constexpr size_t COMPACTJOB = 96;          // sizeof(CompactArgs): nine pointers and three ints with their padding (trace.h)

// keep bytes per job: the record counts of the GPU test and friends, cycled; mode 1: nobody uploads keep bytes; mode 2: every other job
static void layouts() {
    const size_t counts[] = {0, 1, 64, 255, 257, 1025, 4097, 7200, 15, 16, 17};
    for (size_t nj : {1, 2, 7, 128}) for (int mode = 0; mode < 3; mode++) for (size_t shift = 0; shift < 3; shift++) {
        std::vector<size_t> kb(nj);
        for (size_t j = 0; j < nj; j++) kb[j] = mode == 1 || (mode == 2 && j % 2) ? 0 : counts[(j + shift) % 11];
        const CompactGroupLayout L = compact_group_layout(nj, COMPACTJOB, (size_t) LDSO_MAX_FRAMES, [&](size_t j) { return kb[j]; });
        EXPECT(L.jobs == 0 && L.keep.size() == nj && L.downBytes == nj * 4 && L.total == L.down + L.downBytes);
        EXPECT(L.maps % 16 == 0 && L.maps >= L.first + (nj + 1) * 4);
        std::vector<Region> R = {{L.jobs, nj * COMPACTJOB, 16}, {L.first, (nj + 1) * 4, 16}, {L.down, nj * 4, 16}};
        for (size_t j = 0; j < nj; j++) R.push_back({L.keep[j], kb[j], 16});
        for (size_t j = 0; j < nj; j++) R.push_back({L.maps + j * LDSO_MAX_FRAMES * 4, (size_t) LDSO_MAX_FRAMES * 4, 4});          // a job's own map inside the map region
        check_arena(R, L.total, L.down, L.downBytes);
    }
}

// the prefix table of the grouped compaction kernels: ceil(n / 256) workgroups per job, every workgroup finds its job, its block and the job's block count
static void prefix_tables() {
    const std::vector<std::vector<int>> cases = {
        {1}, {256}, {257}, {0, 5}, {5, 0}, {0, 0, 300, 0, 0}, {0, 1, 64, 255, 257, 1025, 4097}, {4097, 0, 0, 1, 0, 256, 0}, {0, 0, 0, 1}, {7200, 0, 7200, 0, 7200},
    };
    for (const std::vector<int> &n : cases) {
        g_calls++;
        const int nj = (int) n.size();
        int *first = (int *) malloc((size_t) (nj + 1) * sizeof(int));          // exactly nJobs + 1 entries
        const int total = group_prefix(nj, first, [&](int j) { return (n[(size_t) j] + 255) / 256; });
        EXPECT(first[0] == 0 && first[nj] == total && total > 0);
        int u = 0;
        for (int j = 0; j < nj; j++) {
            const int blocks = (n[(size_t) j] + 255) / 256;
            EXPECT(first[j] == u && first[j + 1] - first[j] == blocks);
            EXPECT((n[(size_t) j] == 0) == (blocks == 0));
            for (int k = 0; k < blocks; k++, u++) {
                const int m = group_member_of(first, nj, u);          // never an empty job, wherever it stands
                EXPECT(m == j && u - first[m] == k && first[m + 1] - first[m] == blocks);
                EXPECT(k * 256 < n[(size_t) j] && (k + 1 < blocks || (k + 1) * 256 >= n[(size_t) j]));          // the blocks cover the records, none is idle
            }
        }
        EXPECT(u == total);
        free(first);
    }
    // 128 jobs, every third one empty, empty ones at both ends
    g_calls++;
    std::vector<int> n(128);
    for (int j = 0; j < 128; j++) n[(size_t) j] = j % 3 == 0 || j == 127 ? 0 : 100 * j + 1;
    std::vector<int> first(129);
    const int total = group_prefix(128, first.data(), [&](int j) { return (n[(size_t) j] + 255) / 256; });
    for (int u = 0; u < total; u++) {
        const int m = group_member_of(first.data(), 128, u);
        EXPECT(n[(size_t) m] > 0 && first[(size_t) m] <= u && u < first[(size_t) m + 1]);
    }
}

int main() {
    layouts();
    prefix_tables();
    printf("calls %d bad %d\n", g_calls, g_bad);
    return g_bad ? 1 : 0;
}
'''

SIZES = r'''
#include <stdio.h>
#include <stddef.h>
#include "ldso_hip.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(ldso_act_tracer_job_t), offsetof(ldso_act_tracer_job_t, n_hosts), offsetof(ldso_act_tracer_job_t, currentMinActDist),
           offsetof(ldso_act_tracer_job_t, compact), offsetof(ldso_act_tracer_job_t, decision_out), offsetof(ldso_act_tracer_job_t, n_selected), offsetof(ldso_act_tracer_job_t, out),
           offsetof(ldso_act_tracer_job_t, n_left));
    return 0;
}
'''


def test_compaction_layout_and_prefix_table_under_sanitizers():
    d = tempfile.mkdtemp(prefix="compact_stage_")
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
    assert int(m.group(1)) > 40          # an empty run cannot pass


ENTRIES = {
    "ldso_trace_group_compact": (None, None, None, None, None),
    "ldso_ba_batch_select_activate_tracers": (None, C.c_float(3.0), C.c_int(1), C.c_float(100.0), C.c_int(3)),
}


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_entry_is_exported(entry):
    assert hasattr(binding.lib(), entry)


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_null_handle_is_refused_with_a_message(entry):
    L = binding.lib()
    f = getattr(L, entry)
    f.restype = C.c_int
    assert f(None, *ENTRIES[entry]) == LDSO_E_INVALID
    assert entry in L.ldso_last_error().decode()


def test_header_declares_both_entries_with_their_reference_lines():
    text = open(os.path.join(ROOT, "include", "ldso_hip.h")).read()
    for entry in ENTRIES:
        first = text.index(entry)          # the comment that introduces the entry names it first
        comment = text[text.rindex("/*", 0, first):text.index("*/", first)]
        assert "int " + entry + "(" in text[first:]
        assert "FullSystem.cc:1052-1189" in comment and ":602-645" in comment, entry


def test_tracer_job_record_matches_the_header():
    """the ctypes mirror of ldso_act_tracer_job_t against the header as a C compiler lays it out"""
    d = tempfile.mkdtemp(prefix="tracer_job_")
    src, exe = os.path.join(d, "sizes.c"), os.path.join(d, "sizes")
    open(src, "w").write(SIZES)
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
    want = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    J = binding.ActTracerJob
    assert [C.sizeof(J), J.n_hosts.offset, J.currentMinActDist.offset, J.compact.offset, J.decision_out.offset, J.n_selected.offset, J.out.offset, J.n_left.offset] == want
    assert want[0] == 88


@pytest.mark.parametrize("owner,method", ((binding.TracerGroup, "compact"), (binding.BABatch, "select_activate_tracers")))
def test_binding_offers_the_method(owner, method):
    assert callable(getattr(owner, method, None))
