// trace_group.hip — ldso_trace_group_* (include/ldso_hip.h): FullSystem::traceNewCoarse (reference src/frontend/FullSystem.cc:1012-1050) = ImmaturePoint::traceOn
// (src/internal/ImmaturePoint.cc:47-310) of several tracers (independent sequences on one card) in one launch.  One ldso_trace_on is a pose upload, a memset, a
// launch, a download and a wait; k_trace_group (trace.hip) runs the same body for the points of all members, one wavefront per point, packed wave-granular.  The
// members stay ordinary tracers; the group reads their current records, frame and settings at every call and owns only the staging arena of its launch.
// ldso_trace_group_compact is ldso_trace_compact of the members (the records of a marginalised frame leave every sequence's set, FullSystem.cc:602-645) in two launches.
#include "trace.h"
#include "group_member.h"

namespace {

constexpr GroupRule RULE = {"a tracer", "ldso_trace_set_stream", GROUP_MAX_MEMBERS};
static_assert(sizeof(TraceJob) == 112, "the row of trace_group_layout as tests/test_group_stage_cpu.py sizes it");
static_assert(sizeof(CompactArgs) == 96, "the row of compact_group_layout as tests/test_compact_group_stage_cpu.py sizes it");

}  // namespace

extern "C" {

// the member-lookup rule of the grouped launches (group_member.h) as a checked host function
int ldso_trace_group_member_of(const int *first, int n_jobs, int wave, int *job_out) {
    REQ(first && job_out && n_jobs >= 1, "ldso_trace_group_member_of: bad arguments");
    REQ(first[0] == 0, "ldso_trace_group_member_of: first[0] must be 0");
    for (int j = 0; j < n_jobs; j++) REQ(first[j + 1] >= first[j], "ldso_trace_group_member_of: first must not decrease");
    REQ(wave >= 0 && wave < first[n_jobs], "ldso_trace_group_member_of: wave outside [0, first[n_jobs])");
    *job_out = group_member_of(first, n_jobs, wave);
    return LDSO_OK;
}

int ldso_trace_group_create(ldso_tracer_t *const *tracers, int n, ldso_trace_group_t **out) {
    RUN(group_admit(tracers, n, out, "ldso_trace_group_create", RULE));
    CHK(hipSetDevice(tracers[0]->device));
    ldso_trace_group *g = new ldso_trace_group();
    g->device = tracers[0]->device;
    RUN(finish_create(LDSO_OK, g, out, ldso_trace_group_destroy));          // nothing of its own that could fail: the arena comes with the first call
    g->m.assign(tracers, tracers + n);
    group_join(g);
    return LDSO_OK;
}

int ldso_trace_group_destroy(ldso_trace_group_t *g) {
    if (!g) return LDSO_OK;
    hipSetDevice(g->device);
    if (g->arena.h_stage && !g->m.empty()) hipStreamSynchronize(g->m[0]->stream);
    group_leave(g);
    group_arena_free(g->arena);
    delete g;
    return LDSO_OK;
}

// ldso_trace_on of every active member: ONE upload of [pose blocks | TraceJob table | first | zeroed count rows], one launch, ONE download of the count rows, one wait
int ldso_trace_group_on(ldso_trace_group_t *g, const uint8_t *active, const int *n_hosts, const float *const *KRKi, const float *const *Kt, const float *const *aff, int *counts_out) {
    REQ(g && n_hosts && KRKi && Kt && aff, "ldso_trace_group_on: null argument");
    RUN(group_check(g->m.data(), g->m.size(), "ldso_trace_group_on", RULE));
    std::vector<int> members;
    RUN(group_active((int) g->m.size(), active, "ldso_trace_group_on", members, [&](int i) -> const char * {
        if (!(n_hosts[i] >= 1 && n_hosts[i] <= LDSO_MAX_FRAMES)) return "n_hosts outside 1..LDSO_MAX_FRAMES";
        if (!(KRKi[i] && Kt[i] && aff[i])) return "null pose array";
        return g->m[(size_t) i]->haveFrame ? nullptr : "set the new frame first";
    }));
    size_t poseFloats = 0;
    for (int i : members) poseFloats += (size_t) n_hosts[i] * 14;
    CHK(hipSetDevice(g->device));
    const size_t nj = members.size();
    const TraceGroupLayout L = trace_group_layout(poseFloats, nj, sizeof(TraceJob));
    hipStream_t st = g->m[0]->stream;
    RUN(group_arena_grow(g->arena, L.total, st));
    char *const h_stage = g->arena.h_stage, *const d_stage = g->arena.d_stage;
    float *hPose = (float *) (h_stage + L.poses);
    TraceJob *hJ = (TraceJob *) (h_stage + L.jobs);
    int *hF = (int *) (h_stage + L.first), *hC = (int *) (h_stage + L.down);
    size_t po = 0;
    for (size_t j = 0; j < nj; j++) {
        const int i = members[j], nh = n_hosts[i];
        const ldso_tracer *T = g->m[(size_t) i];
        memcpy(hPose + po, KRKi[i], (size_t) nh * 9 * 4);
        memcpy(hPose + po + nh * 9, Kt[i], (size_t) nh * 3 * 4);
        memcpy(hPose + po + nh * 12, aff[i], (size_t) nh * 2 * 4);
        const float *dPose = (const float *) (d_stage + L.poses) + po;
        TraceJob &A = hJ[j];
        memset(&A, 0, sizeof(A));
        A.pts = T->d_pts; A.n = T->n; A.img = T->img; A.w = T->w; A.h = T->h;
        A.KRKi = dPose; A.Kt = dPose + nh * 9; A.aff = dPose + nh * 12; A.nHosts = nh;
        A.s = T->settings; A.counts = (int *) (d_stage + L.down) + 8 * j;
        po += (size_t) nh * 14;
    }
    const int waves = group_prefix((int) nj, hF, [&](int j) { return g->m[(size_t) members[(size_t) j]]->n; });          // one wavefront per point; a member without points is skipped
    memset(hC, 0, L.downBytes);
    CHK(hipMemcpyAsync(d_stage, h_stage, L.total, hipMemcpyHostToDevice, st));
    if (waves > 0) CHK(trace_launch_group((const TraceJob *) (d_stage + L.jobs), (const int *) (d_stage + L.first), (int) nj, waves, st));
    CHK(hipMemcpyAsync(hC, d_stage + L.down, L.downBytes, hipMemcpyDeviceToHost, st));
    CHK(hipStreamSynchronize(st));
    if (counts_out) for (size_t j = 0; j < nj; j++) for (int k = 0; k < 6; k++) counts_out[6 * members[j] + k] = hC[8 * j + k];
    return LDSO_OK;
}

// ldso_trace_compact of every active member (what leaves the immature sets when a frame is marginalised, FullSystem.cc:602-645, or host code released points,
// :1105-1188): ONE upload of [CompactArgs table | first | host maps | keep bytes | zeroed counts] (compact_group_layout), two launches (k_compact_count_group,
// k_compact_move_group: trace.hip), ONE download of the counts, one wait; the members' host state changes behind the wait only
int ldso_trace_group_compact(ldso_trace_group_t *g, const uint8_t *active, const uint8_t *const *keep, const int *n_hosts, const int32_t *const *host_map, int *n_out) {
    REQ(g && n_hosts, "ldso_trace_group_compact: null argument");
    RUN(group_check(g->m.data(), g->m.size(), "ldso_trace_group_compact", RULE));
    std::vector<int> members;
    RUN(group_active((int) g->m.size(), active, "ldso_trace_group_compact", members, [&](int i) -> const char * {
        if (!(n_hosts[i] >= 1 && n_hosts[i] <= LDSO_MAX_FRAMES)) return "n_hosts outside 1..LDSO_MAX_FRAMES";
        for (int f = 0; host_map && host_map[i] && f < n_hosts[i]; f++) if (host_map[i][f] >= LDSO_MAX_FRAMES) return "a host maps beyond LDSO_MAX_FRAMES";
        return nullptr;
    }));
    CHK(hipSetDevice(g->device));
    const size_t nj = members.size();
    const auto keepOf = [&](size_t j) -> const uint8_t * { return keep && g->m[(size_t) members[j]]->n > 0 ? keep[members[j]] : nullptr; };
    const CompactGroupLayout L = compact_group_layout(nj, sizeof(CompactArgs), (size_t) LDSO_MAX_FRAMES, [&](size_t j) { return keepOf(j) ? (size_t) g->m[(size_t) members[j]]->n : (size_t) 0; });
    hipStream_t st = g->m[0]->stream;
    RUN(group_arena_grow(g->arena, L.total, st));
    char *const h_stage = g->arena.h_stage, *const d_stage = g->arena.d_stage;
    CompactArgs *hJ = (CompactArgs *) (h_stage + L.jobs);
    int *hF = (int *) (h_stage + L.first), *hC = (int *) (h_stage + L.down);
    int32_t *hMap = (int32_t *) (h_stage + L.maps);
    memset(hMap, 0, nj * LDSO_MAX_FRAMES * 4);
    for (size_t j = 0; j < nj; j++) {
        const int i = members[j];
        const ldso_tracer *T = g->m[(size_t) i];
        const int32_t *map = host_map ? host_map[i] : nullptr;
        if (map) memcpy(hMap + j * LDSO_MAX_FRAMES, map, (size_t) n_hosts[i] * 4);
        if (keepOf(j)) memcpy(h_stage + L.keep[j], keepOf(j), (size_t) T->n);
        hJ[j] = trace_compact_job(T, keepOf(j) ? (const unsigned char *) (d_stage + L.keep[j]) : nullptr, nullptr, 0, n_hosts[i],
                                  map ? (const int32_t *) (d_stage + L.maps) + j * LDSO_MAX_FRAMES : nullptr, (int32_t *) (d_stage + L.down) + j);
    }
    const int blocks = group_prefix((int) nj, hF, [&](int j) { return compact_blocks(g->m[(size_t) members[(size_t) j]]->n); });          // a member without records is skipped
    memset(hC, 0, L.downBytes);
    CHK(hipMemcpyAsync(d_stage, h_stage, L.total, hipMemcpyHostToDevice, st));
    if (blocks > 0) CHK(trace_launch_compact_group((const CompactArgs *) (d_stage + L.jobs), (const int *) (d_stage + L.first), (int) nj, blocks, st));
    CHK(hipMemcpyAsync(hC, d_stage + L.down, L.downBytes, hipMemcpyDeviceToHost, st));
    CHK(hipStreamSynchronize(st));
    for (size_t j = 0; j < nj; j++) {
        ldso_tracer *T = g->m[(size_t) members[j]];
        if (T->n > 0) trace_compact_finish_group(T, hC[j]);
        if (n_out) n_out[members[j]] = T->n;
    }
    return LDSO_OK;
}

}  // extern "C"
