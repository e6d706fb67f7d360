"""The staging of point activation without a device: ldso_amd/csrc/act_stage.h - the job view, its checks, the arena layout, pack and unpack that the single-window
and the batched activation entries of act_select.hip share - compiled with g++ into a stand-alone program under AddressSanitizer / UBSan.  Every arena is a heap
block of exactly the size the layout reports, so a region that reaches past its arena, or a copy sized by an unclamped n_selected, ends the program."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r'''
#include <cstdio>
#include <cstdlib>
#include "act_stage.h"

static std::string g_err;
void ldso_set_error(const std::string &s) { g_err = s; }

static int g_bad = 0, g_calls = 0, g_refusals = 0;
#define EXPECT(c) do { if (!(c)) { g_bad++; if (g_bad < 20) printf("line %d: %s\n", __LINE__, #c); } } while (0)

constexpr unsigned char UP_FILL = 0xA5, DOWN_FILL = 0x5A;
constexpr int32_t SENTINEL = -77;

template <class T> static T *heap(size_t n, unsigned seed) {          // exactly n elements of recognisable bytes (null for none)
    if (!n) return nullptr;
    T *p = (T *) malloc(n * sizeof(T));
    for (size_t i = 0; i < n * sizeof(T); i++) ((unsigned char *) p)[i] = (unsigned char) (seed * 31 + i * 7 + (i >> 8));
    return p;
}

struct Win {          // one window's inputs and outputs, each on the heap at its exact size
    ldso_act_job_t j;
    bool resident = false, part = true;
    int w = 0, h = 0;
    void make(int n, int nSeeds, int nHosts, bool res, int w_, int h_, unsigned seed) {
        resident = res; w = w_; h = h_;
        memset(&j, 0, sizeof(j));
        j.n = n; j.n_seeds = res ? 0 : nSeeds; j.n_hosts = nHosts; j.currentMinActDist = 1.5f;
        ldso_immature_t *p = res ? nullptr : heap<ldso_immature_t>((size_t) n, seed + 1);
        for (int i = 0; p && i < n; i++) p[i].host = i % nHosts;
        ldso_act_seed_t *s = heap<ldso_act_seed_t>((size_t) j.n_seeds, seed + 2);
        for (int i = 0; i < j.n_seeds; i++) s[i].host = (i * 5) % nHosts;
        j.points = p; j.seeds = s; j.my_type = res ? nullptr : heap<float>((size_t) n, seed + 3);
        j.KRKi = heap<float>((size_t) nHosts * 9, seed + 4); j.Kt = heap<float>((size_t) nHosts * 3, seed + 5); j.host_flagged = heap<int32_t>((size_t) nHosts, seed + 6);
        j.decision_out = heap<int32_t>((size_t) n, 0); j.selected_out = heap<int32_t>((size_t) n, 0); j.out = heap<ldso_activation_t>((size_t) n, 0);
        reset_outputs();
    }
    void reset_outputs() {
        for (int i = 0; i < j.n; i++) { j.decision_out[i] = SENTINEL; j.selected_out[i] = SENTINEL; for (size_t k = 0; k < sizeof(ldso_activation_t) / 4; k++) ((int32_t *) (j.out + i))[k] = SENTINEL; }
        j.n_selected = SENTINEL;
    }
    bool outputs_untouched(int fromSel = 0, int fromOut = 0, bool decisionToo = true) const {          // the selected list from entry fromSel on, the records from fromOut on
        for (int i = 0; i < j.n; i++) {
            if (decisionToo && j.decision_out[i] != SENTINEL) return false;
            if (i >= fromSel && j.selected_out[i] != SENTINEL) return false;
            for (size_t k = 0; i >= fromOut && k < sizeof(ldso_activation_t) / 4; k++) if (((const int32_t *) (j.out + i))[k] != SENTINEL) return false;
        }
        return true;
    }
    ActJob job(bool records, bool flat) const {
        ActJob J = flat ? act_job(j.n_seeds, j.seeds, j.n, j.points, j.my_type, j.n_hosts, j.KRKi, j.Kt, j.host_flagged, j.currentMinActDist, w, h, records, j.decision_out, j.selected_out, j.out)
                        : act_job(j, w, h, records);
        J.resident = resident;
        return J;
    }
    void release() {
        free((void *) j.points); free((void *) j.seeds); free((void *) j.my_type); free((void *) j.KRKi); free((void *) j.Kt); free((void *) j.host_flagged);
        free(j.decision_out); free(j.selected_out); free(j.out);
    }
};

struct Span { int arena; size_t at, bytes; const void *src; };          // arena 0 = upload, 1 = download, 2 = scratch

// the regions of one job with the sizes the kernels use (act_select.hip: SelArgs), counted here from the counts alone
static void spans_of(const ActJob &J, const ActRegions &R, std::vector<Span> &S) {
    const size_t n = (size_t) J.n, nUp = J.resident ? 0 : n, nh = (size_t) J.nHosts;
    S.push_back({0, R.pts, nUp * 128, J.points}); S.push_back({0, R.seeds, (size_t) J.nSeeds * 16, J.seeds}); S.push_back({0, R.type, nUp * 4, J.myType});
    S.push_back({0, R.KRKi, nh * 36, J.KRKi}); S.push_back({0, R.Kt, nh * 12, J.Kt}); S.push_back({0, R.flag, nh * 4, J.flagged});
    S.push_back({1, R.nSel, 16, nullptr}); S.push_back({1, R.dec, n * 4, nullptr}); S.push_back({1, R.sel, n * 4, nullptr}); S.push_back({1, R.act, J.records ? n * 96 : 0, nullptr});
    S.push_back({2, R.cell, n * 4, nullptr}); S.push_back({2, R.frac, n * 4, nullptr}); S.push_back({2, R.thr, n * 4, nullptr});
}

// One call over `wins` (one window: a single-window entry; several: a batch, its bases threaded through the windows that take part): layout, pack, and for each planted
// n_selected an unpack.  plant(J) -> the value written where the device leaves its count.
static void run_call(std::vector<Win> &wins, bool records, bool flat) {
    g_calls++;
    std::vector<ActJob> jobs; std::vector<ActRegions> regs; std::vector<int> who;
    std::vector<Span> S;
    ActBases at;
    for (size_t i = 0; i < wins.size(); i++) {
        if (!wins[i].part) continue;
        ActJob J = wins[i].job(records, flat);
        g_err = "unset";
        EXPECT(act_job_check(J, "entry", flat ? ACT_MISSING_SOLO : ACT_MISSING_BATCH) == LDSO_OK && g_err == "unset");
        const ActBases before = at;
        const ActRegions R = act_layout(J, at);
        EXPECT(R.pts == before.up && R.nSel == before.down && R.cell == before.scratch);
        EXPECT(R.mapBytes % 16 == 0 && R.mapBytes >= (size_t) (wins[i].w >> 1) * (wins[i].h >> 1) && R.mapBytes < (size_t) (wins[i].w >> 1) * (wins[i].h >> 1) + 16);
        spans_of(J, R, S);
        jobs.push_back(J); regs.push_back(R); who.push_back((int) i);
    }
    const size_t tot[3] = {at.up, at.down, at.scratch};
    for (size_t a = 0; a < S.size(); a++) {
        EXPECT(S[a].at % 16 == 0 && S[a].at + S[a].bytes <= tot[S[a].arena]);
        for (size_t b = a + 1; b < S.size(); b++)
            if (S[a].arena == S[b].arena && S[a].bytes && S[b].bytes) EXPECT(S[a].at + S[a].bytes <= S[b].at || S[b].at + S[b].bytes <= S[a].at);
    }
    EXPECT(at.up % 16 == 0 && at.down % 16 == 0 && at.scratch % 16 == 0);
    // pack: the regions hold the inputs, every other byte of the arena is untouched
    unsigned char *up = (unsigned char *) malloc(at.up ? at.up : 1);
    std::vector<char> covered(at.up, 0);
    memset(up, UP_FILL, at.up);
    for (size_t k = 0; k < jobs.size(); k++) act_pack(jobs[k], regs[k], (char *) up);
    for (const Span &s : S) {
        if (s.arena != 0 || !s.bytes) continue;
        EXPECT(memcmp(up + s.at, s.src, s.bytes) == 0);
        for (size_t i = 0; i < s.bytes; i++) covered[s.at + i] = 1;
    }
    size_t stray = 0;
    for (size_t i = 0; i < at.up; i++) if (!covered[i] && up[i] != UP_FILL) stray++;
    EXPECT(stray == 0);
    free(up);
    // unpack: what was planted comes out, with the count kept in [0, n]
    for (int plant = 0; plant < 4; plant++) {
        unsigned char *down = (unsigned char *) malloc(at.down ? at.down : 1);
        memset(down, DOWN_FILL, at.down);
        std::vector<int32_t> planted;
        for (size_t k = 0; k < jobs.size(); k++) {
            const ActJob &J = jobs[k];
            const int32_t ns = plant == 0 ? -1 : plant == 1 ? J.n + 1 : plant == 2 ? J.n / 2 : J.n;
            planted.push_back(ns);
            memcpy(down + regs[k].nSel, &ns, 4);
            for (int i = 0; i < J.n; i++) {
                const int32_t dv = 1000 * (int) k + i, sv = J.n - 1 - i;
                memcpy(down + regs[k].dec + 4 * (size_t) i, &dv, 4); memcpy(down + regs[k].sel + 4 * (size_t) i, &sv, 4);
                if (J.records) memset(down + regs[k].act + 96 * (size_t) i, (i * 3 + (int) k) & 0x7f, 96);
            }
        }
        for (size_t k = 0; k < jobs.size(); k++) {
            const ActJob &J = jobs[k];
            Win &W = wins[(size_t) who[k]];
            W.reset_outputs();
            const int ns = act_unpack(J, regs[k], (const char *) down);
            EXPECT(ns == std::min(std::max(planted[k], 0), J.n));
            for (int i = 0; i < J.n; i++) {
                EXPECT(W.j.decision_out[i] == 1000 * (int) k + i);
                if (i < ns) EXPECT(W.j.selected_out[i] == J.n - 1 - i);
                for (size_t b = 0; J.records && i < ns && b < 96; b++) EXPECT(((const unsigned char *) (W.j.out + i))[b] == (unsigned char) ((i * 3 + (int) k) & 0x7f));
            }
            EXPECT(W.outputs_untouched(ns, J.records ? ns : 0, false));                   // nothing behind the count, and no record where none is wanted
        }
        for (size_t i = 0; i < wins.size(); i++) if (!wins[i].part) EXPECT(wins[i].outputs_untouched() && wins[i].j.n_selected == SENTINEL);
        free(down);
    }
}

static void refused(const Win &W, ActJob J, bool flat, const std::string &text) {
    g_refusals++;
    g_err = "unset";
    const int r = act_job_check(J, "entry", flat ? ACT_MISSING_SOLO : ACT_MISSING_BATCH);
    EXPECT(r == LDSO_E_INVALID);
    if (g_err != "entry: " + text) { g_bad++; printf("refusal text: got '%s', want 'entry: %s'\n", g_err.c_str(), text.c_str()); }
    EXPECT(W.outputs_untouched());
}

int main() {
    const int ns[] = {0, 1, 3, 4, 5, 257}, seeds[] = {0, 1, 7}, hosts[] = {1, 2, 16};
    unsigned seed = 1;
    for (int n : ns) for (int s : seeds) for (int h : hosts) for (int records = 0; records < 2; records++) for (int resident = 0; resident < 2; resident++) {
        std::vector<Win> one(1);
        one[0].make(n, s, h, resident != 0, 320, 240, seed++);
        run_call(one, records != 0, true);
        one[0].release();
    }
    // a batch of three: candidates and seeds, the map only (n = 0), and one that takes no part (n_hosts = 0) between them; then with other counts and image sizes
    for (int records = 0; records < 2; records++) for (int round = 0; round < 2; round++) {
        std::vector<Win> three(3);
        three[0].make(round ? 257 : 5, 7, round ? 16 : 2, false, 320, 240, seed++);
        three[1].make(3, 1, 2, false, 256, 192, seed++); three[1].j.n_hosts = 0; three[1].part = false;
        three[2].make(0, round ? 0 : 7, 3, false, 1280, 512, seed++);
        if (round) std::swap(three[1], three[2]);
        run_call(three, records != 0, false);
        for (Win &W : three) W.release();
    }
    // refusals, with the texts of the entries
    const std::string solo = ACT_MISSING_SOLO, batch = ACT_MISSING_BATCH;
    EXPECT(solo == "bad arguments" && batch == "a window that takes part needs its arrays (seeds, points, my_type, KRKi, Kt, host_flagged and the outputs)");
    for (int flat = 0; flat < 2; flat++) {
        const std::string missing = flat ? solo : batch;
        Win W;
        W.make(5, 7, 2, false, 320, 240, seed++);
        const ActJob good = W.job(true, flat != 0);
        EXPECT(act_job_check(good, "entry", missing.c_str()) == LDSO_OK);
        ldso_immature_t *p = (ldso_immature_t *) W.j.points; ldso_act_seed_t *s = (ldso_act_seed_t *) W.j.seeds;
        p[4].host = 2; refused(W, good, flat, "a candidate's host is not a frame of the window"); p[4].host = -1; refused(W, good, flat, "a candidate's host is not a frame of the window"); p[4].host = 0;
        s[6].host = 2; refused(W, good, flat, "a seed's host is not a frame of the window"); s[6].host = -1; refused(W, good, flat, "a seed's host is not a frame of the window"); s[6].host = 0;
        p[0].host = 7; s[0].host = 7; refused(W, good, flat, "a candidate's host is not a frame of the window"); p[0].host = 0; s[0].host = 0;          // the candidates come first
        ActJob J = good; J.nHosts = 0; refused(W, J, flat, missing);
        J = good; J.nHosts = LDSO_MAX_FRAMES + 1; refused(W, J, flat, missing);
        EXPECT(LDSO_MAX_FRAMES == 16);
        J = good; J.n = -1; refused(W, J, flat, missing);
        J = good; J.nSeeds = -1; refused(W, J, flat, missing);
        J = good; J.points = nullptr; refused(W, J, flat, missing);
        J = good; J.myType = nullptr; refused(W, J, flat, missing);
        J = good; J.seeds = nullptr; refused(W, J, flat, missing);
        J = good; J.KRKi = nullptr; refused(W, J, flat, missing);
        J = good; J.Kt = nullptr; refused(W, J, flat, missing);
        J = good; J.flagged = nullptr; refused(W, J, flat, missing);
        J = good; J.decisionOut = nullptr; refused(W, J, flat, missing);
        J = good; J.selectedOut = nullptr; refused(W, J, flat, missing);
        J = good; J.out = nullptr; refused(W, J, flat, missing);
        J = good; J.w1 = 2; refused(W, J, flat, "image size out of range");
        J = good; J.h1 = 65536; refused(W, J, flat, "image size out of range");
        // null arrays are no fault where nothing is read from them: no count, no records, candidates that lie on the device
        J = good; J.n = 0; J.points = nullptr; J.myType = nullptr; J.decisionOut = nullptr; J.selectedOut = nullptr; J.out = nullptr; J.nSeeds = 0; J.seeds = nullptr;
        EXPECT(act_job_check(J, "entry", missing.c_str()) == LDSO_OK);
        J = good; J.records = false; J.selectedOut = nullptr; J.out = nullptr;
        EXPECT(act_job_check(J, "entry", missing.c_str()) == LDSO_OK);
        J = good; J.resident = true; J.points = nullptr; J.myType = nullptr; J.nSeeds = 0; J.seeds = nullptr;
        EXPECT(act_job_check(J, "entry", missing.c_str()) == LDSO_OK);
        W.release();
    }
    printf("calls %d refusals %d bad %d\n", g_calls, g_refusals, g_bad);
    return g_bad ? 1 : 0;
}
'''


def test_layout_pack_unpack_and_checks_under_sanitizers():
    d = tempfile.mkdtemp(prefix="act_stage_")
    src, exe = os.path.join(d, "stage.cc"), os.path.join(d, "stage")
    open(src, "w").write(PROGRAM)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = subprocess.run(["g++", *san, "-x", "c++", "-", "-o", os.path.join(d, "probe")], input="int main() { return 0; }\n", capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("the sanitizer runtime cannot be linked here: " + probe.stderr[-300:])
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *san, "-I", os.path.join(ROOT, "ldso_amd", "csrc"), src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    # 6 x 3 x 3 x 2 x 2 single-window calls and 4 batches; 5 hosts out of range, 13 missing or out-of-range arguments, 2 image sizes for each of the two kinds of entry
    assert "calls 220 refusals 40 bad 0" in r.stdout, r.stdout[-2000:]
