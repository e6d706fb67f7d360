// act_stage.h — the staging of one window's candidate selection (act_select.hip) as far as it can be said without a device: a view of the job, its checks, where its
// inputs, results and scratch lie in the call's arenas, and the host side of the two copies.  The single-window entries and the batched ones share every line of it.
// No HIP header: it compiles with a plain C++ compiler (tests/test_activation_stage_cpu.py runs it under the sanitizers).
#pragma once
#include "group_stage.h"          // align_up

inline size_t up16(size_t x) { return align_up(x, 16); }

// One window's job.  resident: the candidates are a tracer's records where they lie on the device and the seeds the points of the resident window - nothing of either
// is uploaded, `points` / `myType` / `seeds` stay null.  records: the activation follows, its records come down behind the selected list.
struct ActJob {
    int nSeeds = 0; const ldso_act_seed_t *seeds = nullptr;
    int n = 0; const ldso_immature_t *points = nullptr; const float *myType = nullptr;
    bool resident = false;
    int nHosts = 0; const float *KRKi = nullptr, *Kt = nullptr; const int32_t *flagged = nullptr;
    float minDist = 0;
    int w1 = 0, h1 = 0;                                          // the distance map: level 1 of the window's image size
    bool records = false;
    int32_t *decisionOut = nullptr, *selectedOut = nullptr; ldso_activation_t *out = nullptr;
};

// from the flat arguments of the single-window entries, and from a window's share of a batched call
inline ActJob act_job(int n_seeds, const ldso_act_seed_t *seeds, int n, const ldso_immature_t *points, const float *my_type, int n_hosts, const float *KRKi, const float *Kt,
                      const int32_t *host_flagged, float currentMinActDist, int w, int h, bool records, int32_t *decision_out, int32_t *selected_out, ldso_activation_t *out) {
    ActJob J;
    J.nSeeds = n_seeds; J.seeds = seeds; J.n = n; J.points = points; J.myType = my_type; J.nHosts = n_hosts; J.KRKi = KRKi; J.Kt = Kt; J.flagged = host_flagged;
    J.minDist = currentMinActDist; J.w1 = w >> 1; J.h1 = h >> 1; J.records = records; J.decisionOut = decision_out; J.selectedOut = selected_out; J.out = out;
    return J;
}
inline ActJob act_job(const ldso_act_job_t &j, int w, int h, bool records) {
    return act_job(j.n_seeds, j.seeds, j.n, j.points, j.my_type, j.n_hosts, j.KRKi, j.Kt, j.host_flagged, j.currentMinActDist, w, h, records, j.decision_out, j.selected_out, j.out);
}

// what an entry says of a job without its arrays: a single-window one, a batched one
constexpr const char *ACT_MISSING_SOLO = "bad arguments";
constexpr const char *ACT_MISSING_BATCH = "a window that takes part needs its arrays (seeds, points, my_type, KRKi, Kt, host_flagged and the outputs)";
constexpr const char *ACT_MISSING_TRACERS = "a window that takes part needs KRKi, Kt, host_flagged and, where its tracer holds records, the outputs";

// The checks of one job; `who` names the entry.  Device data cannot be range-checked here: the kernel drops a candidate and skips a seed whose host is not a frame of the window.
inline int act_job_check(const ActJob &J, const std::string &who, const char *missing) {
    REQ(J.nSeeds >= 0 && J.n >= 0 && J.nHosts >= 1 && J.nHosts <= LDSO_MAX_FRAMES && J.KRKi && J.Kt && J.flagged && (J.nSeeds == 0 || J.seeds)
        && (J.n == 0 || ((J.resident || (J.points && J.myType)) && J.decisionOut && (!J.records || (J.selectedOut && J.out)))), who + ": " + missing);
    REQ(J.w1 >= 3 && J.h1 >= 3 && J.w1 < 65536 && J.h1 < 65536, who + ": image size out of range");
    for (int i = 0; !J.resident && i < J.n; i++) REQ(J.points[i].host >= 0 && J.points[i].host < J.nHosts, who + ": a candidate's host is not a frame of the window");
    for (int i = 0; i < J.nSeeds; i++) REQ(J.seeds[i].host >= 0 && J.seeds[i].host < J.nHosts, who + ": a seed's host is not a frame of the window");
    return LDSO_OK;
}

// The layout.  A call has three arenas: what goes up in one copy, what comes down in one copy, and scratch that never leaves the device.  A job's regions are byte
// offsets into them, every one a multiple of 16 where the bases are:
//   upload    [points n x 128 | seeds n_seeds x 16 | my_type | KRKi n_hosts x 9 | Kt n_hosts x 3 | flagged n_hosts]      (points and my_type: none when resident)
//   download  [n_selected, 16 bytes | decision n | selected n | activation records n x 96, where wanted]
//   scratch   [cell n | frac n | thr n]                                                                                  (the pending candidates of the greedy pass)
// A single-window call starts the bases at zero; a batch threads them through its participating windows.  mapBytes: the room of the job's distance map, which the
// caller places (behind the scratch; in the member's own arena).
struct ActBases { size_t up = 0, down = 0, scratch = 0; };
struct ActRegions { size_t pts, seeds, type, KRKi, Kt, flag, nSel, dec, sel, act, cell, frac, thr, mapBytes; };

inline ActRegions act_layout(const ActJob &J, ActBases &at) {
    const size_t nn = (size_t) J.n, nUp = J.resident ? 0 : nn, idx = up16(nn * 4), nh = (size_t) J.nHosts;
    ActRegions R;
    R.pts = at.up; R.seeds = R.pts + nUp * sizeof(ldso_immature_t); R.type = R.seeds + up16((size_t) J.nSeeds * sizeof(ldso_act_seed_t)); R.KRKi = R.type + up16(nUp * 4);
    R.Kt = R.KRKi + up16(nh * 36); R.flag = R.Kt + up16(nh * 12); at.up = R.flag + up16(nh * 4);
    R.nSel = at.down; R.dec = R.nSel + 16; R.sel = R.dec + idx; R.act = R.sel + idx; at.down = R.act + (J.records ? nn * sizeof(ldso_activation_t) : 0);
    R.cell = at.scratch; R.frac = R.cell + idx; R.thr = R.frac + idx; at.scratch = R.thr + idx;
    R.mapBytes = up16((size_t) J.w1 * J.h1);
    return R;
}

// The tables of a batched call, in front of the windows' uploads: [nPart selection rows | nAct activation rows | nAct + 1 wavefront offsets | nCmp compaction rows |
// nCmp + 1 workgroup prefixes, where nCmp > 0], every region 16-byte aligned; `in` = where the first window's upload begins.  A call that compacts (the resident
// tracers of ldso_ba_batch_select_activate_tracers) gets its nCmp counts back behind the windows' downloads: act_batch_counts.
struct ActBatchTables { size_t sel, act, wave, cmp, first, in; };
inline ActBatchTables act_batch_tables(size_t nPart, size_t nAct, size_t nCmp, size_t selBytes, size_t actBytes, size_t cmpBytes) {
    ActBatchTables T;
    T.sel = 0; T.act = T.sel + up16(nPart * selBytes); T.wave = T.act + up16(nAct * actBytes); T.cmp = T.wave + up16((nAct + 1) * 4); T.first = T.cmp + up16(nCmp * cmpBytes);
    T.in = T.first + (nCmp ? up16((nCmp + 1) * 4) : 0);
    return T;
}
inline size_t act_batch_counts(size_t nCmp) { return up16(nCmp * 4); }

// the job's inputs into the host copy of the upload arena; the bytes between the regions are left as they are
inline void act_pack(const ActJob &J, const ActRegions &R, char *up) {
    if (J.n && !J.resident) { memcpy(up + R.pts, J.points, (size_t) J.n * sizeof(ldso_immature_t)); memcpy(up + R.type, J.myType, (size_t) J.n * 4); }
    if (J.nSeeds) memcpy(up + R.seeds, J.seeds, (size_t) J.nSeeds * sizeof(ldso_act_seed_t));
    memcpy(up + R.KRKi, J.KRKi, (size_t) J.nHosts * 36); memcpy(up + R.Kt, J.Kt, (size_t) J.nHosts * 12); memcpy(up + R.flag, J.flagged, (size_t) J.nHosts * 4);
}

// the job's results out of the host copy of the download arena -> the number of selected candidates, which sizes two of the copies and is the device's word: kept in [0, n]
inline int act_unpack(const ActJob &J, const ActRegions &R, const char *down) {
    int32_t ns;
    memcpy(&ns, down + R.nSel, 4);
    ns = std::min(std::max(ns, 0), J.n);
    if (J.n) memcpy(J.decisionOut, down + R.dec, (size_t) J.n * 4);
    if (J.selectedOut && ns > 0) memcpy(J.selectedOut, down + R.sel, (size_t) ns * 4);
    if (J.records && ns > 0) memcpy(J.out, down + R.act, (size_t) ns * sizeof(ldso_activation_t));
    return ns;
}
