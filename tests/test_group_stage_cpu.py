"""What the grouped calls share without a device: ldso_amd/csrc/group_stage.h - who may be a member of a group, the active list of a call, the prefix table that
group_member_of searches and the layouts of the four staging arenas - compiled with g++ into a stand-alone program under AddressSanitizer / UBSan.  Every arena is
a heap block of exactly the size its layout reports and every region is filled at its offset, so a region that reaches past its arena ends the program."""
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r'''
#include <cstdio>
#include <cstdlib>
#include "group_stage.h"

static std::string g_err;
void ldso_set_error(const std::string &s) { g_err = s; }

static int g_bad = 0, g_calls = 0, g_refusals = 0;
#define EXPECT(c) do { if (!(c)) { g_bad++; if (g_bad < 20) printf("line %d: %s\n", __LINE__, #c); } } while (0)

// ---- membership ----
struct Fake { int device = 0; void *stream = nullptr; const void *inGroup = nullptr; };
struct Bare { int device = 0; const void *inGroup = nullptr; };          // no stream at all: a pyramid
template <class M> struct GroupOf { std::vector<M *> m; };

static const GroupRule WITH_STREAM = {"a widget", "ldso_widget_set_stream", GROUP_MAX_MEMBERS}, DEVICE_ONLY = {"an owl", nullptr, GROUP_MAX_MEMBERS};
static char g_out;          // stands for the create entry's `out`

template <class M> static bool untouched(const std::vector<M> &pool, const std::vector<const void *> &was) {
    for (size_t i = 0; i < pool.size(); i++) if (pool[i].inGroup != was[i]) return false;
    return true;
}

template <class M> static void admitted(std::vector<M> &pool, std::vector<M *> list, const GroupRule &R) {
    g_calls++;
    g_err = "unset";
    EXPECT(group_admit(list.data(), (int) list.size(), &g_out, "entry", R) == LDSO_OK && g_err == "unset");
    for (const M &x : pool) EXPECT(x.inGroup == nullptr);          // admission writes nothing
}

template <class M> static void refused(std::vector<M> &pool, M *const *list, int n, const void *out, const GroupRule &R, const std::string &text) {
    g_refusals++;
    std::vector<const void *> was;
    for (const M &x : pool) was.push_back(x.inGroup);
    g_err = "unset";
    EXPECT(group_admit(list, n, out, "entry", R) == LDSO_E_INVALID);
    if (g_err != "entry: " + text) { g_bad++; printf("refusal text: got '%s', want 'entry: %s'\n", g_err.c_str(), text.c_str()); }
    EXPECT(untouched(pool, was));
}

static void membership() {
    int streamA, streamB, someGroup;
    std::vector<Fake> pool(129);
    for (Fake &f : pool) { f.device = 2; f.stream = &streamA; }
    auto list = [&](int n) { std::vector<Fake *> v; for (int i = 0; i < n; i++) v.push_back(&pool[(size_t) i]); return v; };
    const std::string bad = "bad arguments (1 <= n <= 128 widgets)", share = "the members of a group share one device and one stream (ldso_widget_set_stream)";
    for (int n : {1, 2, 5, 128}) admitted(pool, list(n), WITH_STREAM);
    for (int n : {1, 128}) admitted(pool, list(n), DEVICE_ONLY);
    std::vector<Fake *> v = list(129);
    refused(pool, v.data(), 0, &g_out, WITH_STREAM, bad);
    refused(pool, v.data(), 129, &g_out, WITH_STREAM, bad);
    refused(pool, v.data(), -1, &g_out, WITH_STREAM, bad);
    refused(pool, (Fake *const *) nullptr, 3, &g_out, WITH_STREAM, bad);
    refused(pool, v.data(), 3, nullptr, WITH_STREAM, bad);
    refused(pool, v.data(), 129, &g_out, DEVICE_ONLY, "bad arguments (1 <= n <= 128 owls)");
    const GroupRule few = {"a tracker", "ldso_tr_set_stream", 4};          // the bound is the rule's
    refused(pool, v.data(), 5, &g_out, few, "bad arguments (1 <= n <= 4 trackers)");
    admitted(pool, list(4), few);
    for (int n : {1, 7, 128}) for (int at : {0, n - 1}) {
        v = list(n); v[(size_t) at] = nullptr;
        refused(pool, v.data(), n, &g_out, WITH_STREAM, "null widget");
        refused(pool, v.data(), n, &g_out, DEVICE_ONLY, "null owl");
    }
    for (int n : {2, 7, 128}) for (int at : {1, n - 1}) {
        v = list(n); v[(size_t) at] = v[0];
        refused(pool, v.data(), n, &g_out, WITH_STREAM, "the same widget twice");
        refused(pool, v.data(), n, &g_out, DEVICE_ONLY, "the same owl twice");
    }
    for (int n : {1, 7, 128}) for (int at : {0, n - 1}) {
        v = list(n);
        pool[(size_t) at].inGroup = &someGroup;
        refused(pool, v.data(), n, &g_out, WITH_STREAM, "a widget belongs to at most one group at a time");
        refused(pool, v.data(), n, &g_out, DEVICE_ONLY, "an owl belongs to at most one group at a time");
        pool[(size_t) at].inGroup = nullptr;
    }
    for (int n : {2, 7, 128}) for (int at : {0, 1, n - 1}) {
        v = list(n);
        pool[(size_t) at].device = 3;
        refused(pool, v.data(), n, &g_out, WITH_STREAM, share);
        refused(pool, v.data(), n, &g_out, DEVICE_ONLY, "the members of a group share one device");
        pool[(size_t) at].device = 2;
        pool[(size_t) at].stream = at % 2 ? (void *) &streamB : nullptr;          // another stream, and none
        refused(pool, v.data(), n, &g_out, WITH_STREAM, share);
        admitted(pool, v, DEVICE_ONLY);                                            // the same pair under the device-only rule
        // the per-call form of the same check
        g_refusals++; g_err = "unset";
        EXPECT(group_check(v.data(), v.size(), "call", WITH_STREAM) == LDSO_E_INVALID && g_err == "call: " + share);
        g_calls++; g_err = "unset";
        EXPECT(group_check(v.data(), v.size(), "call", DEVICE_ONLY) == LDSO_OK && g_err == "unset");
        pool[(size_t) at].stream = &streamA;
        g_calls++;
        EXPECT(group_check(v.data(), v.size(), "call", WITH_STREAM) == LDSO_OK && g_err == "unset");
    }
    // a member type without a stream
    std::vector<Bare> bare(3);
    std::vector<Bare *> bv = {&bare[0], &bare[1], &bare[2]};
    admitted(bare, bv, DEVICE_ONLY);
    bare[2].device = 1;
    refused(bare, bv.data(), 3, &g_out, DEVICE_ONLY, "the members of a group share one device");
    bare[2].device = 0;
    // the texts of the four create entries, word for word
    const struct { GroupRule R; const char *who, *bad, *null, *one, *twice; } real[] = {
        {{"a tracker", "ldso_tr_set_stream", 128}, "ldso_tr_group_create", "bad arguments (1 <= n <= 128 trackers)", "null tracker", "a tracker belongs to at most one group at a time", "the same tracker twice"},
        {{"a tracer", "ldso_trace_set_stream", 128}, "ldso_trace_group_create", "bad arguments (1 <= n <= 128 tracers)", "null tracer", "a tracer belongs to at most one group at a time", "the same tracer twice"},
        {{"a pyramid", nullptr, 128}, "ldso_pyr_group_create", "bad arguments (1 <= n <= 128 pyramids)", "null pyramid", "a pyramid belongs to at most one group at a time", "the same pyramid twice"},
        {{"an undistorter", "ldso_undist_set_stream", 128}, "ldso_undist_group_create", "bad arguments (1 <= n <= 128 undistorters)", "null undistorter", "an undistorter belongs to at most one group at a time", "the same undistorter twice"},
    };
    for (const auto &e : real) {
        const std::string w = std::string(e.who) + ": ";
        v = list(3);
        g_refusals += 5;
        EXPECT(group_admit(v.data(), 0, &g_out, e.who, e.R) == LDSO_E_INVALID && g_err == w + e.bad);
        v[1] = nullptr; EXPECT(group_admit(v.data(), 3, &g_out, e.who, e.R) == LDSO_E_INVALID && g_err == w + e.null);
        v[1] = v[0]; EXPECT(group_admit(v.data(), 3, &g_out, e.who, e.R) == LDSO_E_INVALID && g_err == w + e.twice);
        v = list(3); pool[2].inGroup = &someGroup; EXPECT(group_admit(v.data(), 3, &g_out, e.who, e.R) == LDSO_E_INVALID && g_err == w + e.one);
        pool[2].inGroup = nullptr; pool[1].device = 0;
        EXPECT(group_admit(v.data(), 3, &g_out, e.who, e.R) == LDSO_E_INVALID &&
               g_err == w + "the members of a group share one device" + (e.R.setStream ? std::string(" and one stream (") + e.R.setStream + ")" : std::string()));
        pool[1].device = 2;
    }
    // join and leave
    GroupOf<Fake> g, h;
    g.m = list(128);
    g_calls += 2;
    group_join(&g);
    for (int i = 0; i < 129; i++) EXPECT(pool[(size_t) i].inGroup == (i < 128 ? &g : nullptr));
    v = {&pool[128], &pool[5]};
    refused(pool, v.data(), 2, &g_out, WITH_STREAM, "a widget belongs to at most one group at a time");
    group_leave(&g);
    for (const Fake &f : pool) EXPECT(f.inGroup == nullptr);
    // a member that has joined another group since is not cleared
    group_join(&g);
    h.m = {&pool[0], &pool[127]};
    group_join(&h);
    g_calls += 2;
    group_leave(&g);
    for (int i = 0; i < 128; i++) EXPECT(pool[(size_t) i].inGroup == (i == 0 || i == 127 ? &h : nullptr));
    group_leave(&h);
    for (const Fake &f : pool) EXPECT(f.inGroup == nullptr);
}

// ---- the active list ----
static void active_list() {
    for (int n : {1, 2, 7, 128}) {
        std::vector<uint8_t> ones((size_t) n, 1), zeros((size_t) n, 0), firstOnly(zeros), lastOnly(zeros), odd(zeros);
        firstOnly[0] = 1; lastOnly[(size_t) n - 1] = 2;          // any non-zero byte
        for (int i = 1; i < n; i += 2) odd[(size_t) i] = 1;
        std::vector<int> members = {-5}, visits;
        auto fine = [&](int i) -> const char * { visits.push_back(i); return nullptr; };
        auto run = [&](const uint8_t *act) { g_calls++; g_err = "unset"; visits.clear(); return group_active(n, act, "entry", members, fine); };
        std::vector<int> all;
        for (int i = 0; i < n; i++) all.push_back(i);
        EXPECT(run(nullptr) == LDSO_OK && members == all && visits == all && g_err == "unset");
        EXPECT(run(ones.data()) == LDSO_OK && members == all && visits == all);
        EXPECT(run(firstOnly.data()) == LDSO_OK && members == std::vector<int>{0} && visits == members);
        EXPECT(run(lastOnly.data()) == LDSO_OK && members == std::vector<int>{n - 1} && visits == members);
        if (n > 1) { EXPECT(run(odd.data()) == LDSO_OK && (int) members.size() == n / 2 && members[0] == 1 && visits == members); }
        g_refusals++;
        EXPECT(run(zeros.data()) == LDSO_E_INVALID && g_err == "entry: no active member" && visits.empty());
        // a member the call refuses: its index in the text, and nobody behind it is looked at
        for (int at : {0, n - 1}) for (const uint8_t *act : {(const uint8_t *) nullptr, (const uint8_t *) ones.data()}) {
            g_refusals++;
            visits.clear();
            const int r = group_active(n, act, "entry", members, [&](int i) -> const char * { visits.push_back(i); return i == at ? "no frame" : nullptr; });
            EXPECT(r == LDSO_E_INVALID && g_err == "entry: member " + std::to_string(at) + ": no frame");
            EXPECT((int) visits.size() == at + 1 && visits.back() == at);
        }
        // ... unless it is inactive
        g_calls++;
        visits.clear();
        EXPECT(group_active(n, n > 1 ? lastOnly.data() : ones.data(), "entry", members, [&](int i) -> const char * { visits.push_back(i); return i == 0 && n > 1 ? "no frame" : nullptr; }) == LDSO_OK);
        EXPECT(visits == std::vector<int>{n - 1});
    }
}

// ---- the prefix table against group_member_of: every unit-count vector of length 1..5 with entries 0..5 that has a unit ----
static void prefix_tables() {
    for (int len = 1; len <= 5; len++) {
        int total = 1;
        for (int k = 0; k < len; k++) total *= 6;
        for (int code = 0; code < total; code++) {
            int units[5], c = code, sum = 0;
            for (int k = 0; k < len; k++) { units[k] = c % 6; c /= 6; sum += units[k]; }
            if (!sum) continue;
            g_calls++;
            int *first = (int *) malloc((size_t) (len + 1) * sizeof(int));          // exactly nJobs + 1 entries
            EXPECT(group_prefix(len, first, [&](int j) { return units[j]; }) == sum);
            EXPECT(first[0] == 0 && first[len] == sum);
            int u = 0;
            for (int j = 0; j < len; j++) {
                EXPECT(first[j] == u && first[j + 1] - first[j] == units[j]);
                for (int k = 0; k < units[j]; k++, u++) EXPECT(group_member_of(first, len, u) == j);          // the job whose range holds it: never an empty one
            }
            free(first);
        }
    }
}

// ---- the layouts ----
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
    EXPECT(downAt + downBytes <= total);
    free(blk);
}

// the row sizes the .hip files static_assert (tracker_group.hip, trace_group.hip, images.hip, undistort.hip)
constexpr size_t TRPARAMS = 904, TRJOB = 24, TRHYP = 344, TRACEJOB = 112, IMGJOB = 40, UNDISTJOB = 80;

static void layouts() {
    const size_t tr[][2] = {{1, 1}, {1, 83}, {3, 5}, {128, 128}, {2, 166}};
    for (const auto &c : tr) {
        const size_t np = c[0], nj = c[1];
        const TrGroupLayout L = tr_group_layout(np, nj, TRPARAMS, TRJOB, TRHYP);
        EXPECT(L.params == 0 && L.downBytes == nj * TRHYP && L.total == L.down + L.downBytes);
        check_arena({{L.params, np * TRPARAMS, 16}, {L.jobs, nj * TRJOB, 16}, {L.down, nj * TRHYP, 16}}, L.total, L.down, L.downBytes);
    }
    EXPECT(LDSO_MAX_FRAMES == 16);
    for (size_t nj : {1, 2, 7, 128}) for (int mode = 0; mode < 3; mode++) {          // hosts per member: 1, 2, ... cycling through 1..16; all 1; all at the maximum
        std::vector<Region> R;
        size_t poseFloats = 0;
        std::vector<size_t> nh(nj);
        for (size_t j = 0; j < nj; j++) { nh[j] = mode == 0 ? j % LDSO_MAX_FRAMES + 1 : mode == 1 ? 1 : LDSO_MAX_FRAMES; poseFloats += nh[j] * 14; }
        const TraceGroupLayout L = trace_group_layout(poseFloats, nj, TRACEJOB);
        size_t po = 0;
        for (size_t j = 0; j < nj; j++) { R.push_back({L.poses + po * 4, nh[j] * 14 * 4, 4}); po += nh[j] * 14; }          // the members' pose blocks are packed: floats
        EXPECT(L.poses == 0 && L.downBytes == nj * 32 && L.total == L.down + L.downBytes);
        EXPECT(po == poseFloats && L.poses + po * 4 <= L.jobs);
        R.push_back({L.jobs, nj * TRACEJOB, 16}); R.push_back({L.first, (nj + 1) * 4, 16}); R.push_back({L.down, nj * 32, 16});
        check_arena(R, L.total, L.down, L.downBytes);
    }
    EXPECT(LDSO_PYR_LEVELS == 6);
    const std::vector<std::vector<int>> pyr = {{1}, {4, 2, 1}, {6, 6}, std::vector<int>(128, 4)};
    for (const std::vector<int> &levels : pyr) {
        const int Lmax = *std::max_element(levels.begin(), levels.end());
        auto at = [&](int l) { int nl = 0; for (int v : levels) nl += v > l; return nl; };
        const PyrGroupLayout P = pyr_group_layout(Lmax, IMGJOB, at);
        EXPECT((int) P.level.size() == Lmax);
        std::vector<Region> R;
        for (int l = 0; l < Lmax; l++) {
            const PyrLevelLayout &L = P.level[(size_t) l];
            EXPECT(L.nl == at(l) && L.nl >= 1);
            R.push_back({L.jobs, (size_t) L.nl * IMGJOB, 16}); R.push_back({L.firstI, (size_t) (L.nl + 1) * 4, 4}); R.push_back({L.firstG, (size_t) (L.nl + 1) * 4, 4});
        }
        check_arena(R, P.total, 0, 0);
    }
    const size_t tiny[] = {1 * 1 * 1, 5 * 3 * 1, 5 * 3 * 2}, vga = 640 * 480 * 1;
    std::vector<std::vector<size_t>> und = {{1}, {15}, {30}, {vga}, {1, vga, 15, 30, vga, 1}, {vga, 30}};
    und.push_back({});
    for (size_t j = 0; j < 128; j++) und.back().push_back(j % 5 == 4 ? vga : tiny[j % 3]);
    for (const std::vector<size_t> &bytes : und) {
        const size_t nj = bytes.size();
        const UndistGroupLayout L = undist_group_layout(nj, UNDISTJOB, [&](size_t j) { return bytes[j]; });
        EXPECT(L.jobs == 0 && L.frame.size() == nj && L.total % 64 == 0);
        std::vector<Region> R = {{L.jobs, nj * UNDISTJOB, 16}, {L.first, (nj + 1) * 4, 4}};
        for (size_t j = 0; j < nj; j++) R.push_back({L.frame[j], bytes[j], 64});
        check_arena(R, L.total, 0, 0);
    }
    // the one rounding helper
    g_calls++;
    for (size_t a : {1, 4, 16, 64}) for (size_t x = 0; x < 200; x++) { const size_t r = align_up(x, a); EXPECT(r % a == 0 && r >= x && r < x + a); }
}

int main() {
    membership();
    active_list();
    prefix_tables();
    layouts();
    printf("calls %d refusals %d bad %d\n", g_calls, g_refusals, g_bad);
    return g_bad ? 1 : 0;
}
'''


def test_membership_active_list_prefix_table_and_layouts_under_sanitizers():
    d = tempfile.mkdtemp(prefix="group_stage_")
    src, exe = os.path.join(d, "stage.cc"), os.path.join(d, "stage")
    open(src, "w").write(PROGRAM)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = subprocess.run(["g++", *san, "-x", "c++", "-", "-o", os.path.join(d, "probe")], input="int main() { return 0; }\n", capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("the sanitizer runtime cannot be linked here: " + probe.stderr[-300:])
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *san, "-I", os.path.join(ROOT, "ldso_amd", "csrc"), src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    m = re.search(r"calls (\d+) refusals (\d+) bad 0\n", r.stdout)
    assert m, r.stdout[-2000:]
    assert int(m.group(1)) > 0 and int(m.group(2)) > 0          # an empty run cannot pass
