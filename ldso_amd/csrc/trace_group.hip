// trace_group.hip — ldso_trace_group_* (include/ldso_hip.h): FullSystem::traceNewCoarse (reference src/frontend/FullSystem.cc:1012-1050) = ImmaturePoint::traceOn
// (src/internal/ImmaturePoint.cc:47-310) of several tracers (independent sequences on one card) in one launch.  One ldso_trace_on is a pose upload, a memset, a
// launch, a download and a wait; k_trace_group (trace.hip) runs the same body for the points of all members, one wavefront per point, packed wave-granular.  The
// members stay ordinary tracers; the group reads their current records, frame and settings at every call and owns only the staging arena of its launch.
#include "ba_host.h"
#include "group_member.h"

namespace {

inline size_t up16(size_t x) { return (x + 15) & ~(size_t) 15; }

// what every call checks of its group before anything is enqueued: the members still share the stream the group was made on
int group_check(const ldso_trace_group *g, const char *who) {
    for (const ldso_tracer *T : g->m) REQ(T->stream == g->m[0]->stream && T->device == g->device, std::string(who) + ": the members of a group share one device and one stream (ldso_trace_set_stream)");
    return LDSO_OK;
}

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
    REQ(tracers && out && n >= 1 && n <= 128, "ldso_trace_group_create: bad arguments (1 <= n <= 128 tracers)");
    for (int i = 0; i < n; i++) {
        REQ(tracers[i], "ldso_trace_group_create: null tracer");
        REQ(tracers[i]->inGroup == nullptr, "ldso_trace_group_create: a tracer belongs to at most one group at a time");
        for (int k = 0; k < i; k++) REQ(tracers[k] != tracers[i], "ldso_trace_group_create: the same tracer twice");
        REQ(tracers[i]->device == tracers[0]->device && tracers[i]->stream == tracers[0]->stream,
            "ldso_trace_group_create: the members of a group share one device and one stream (ldso_trace_set_stream)");
    }
    ldso_trace_group *g = new ldso_trace_group();
    g->device = tracers[0]->device;
    g->m.assign(tracers, tracers + n);
    for (ldso_tracer *T : g->m) T->inGroup = g;
    *out = g;
    return LDSO_OK;
}

int ldso_trace_group_destroy(ldso_trace_group_t *g) {
    if (!g) return LDSO_OK;
    hipSetDevice(g->device);
    if (g->h_stage && !g->m.empty()) hipStreamSynchronize(g->m[0]->stream);
    for (ldso_tracer *T : g->m) if (T->inGroup == g) T->inGroup = nullptr;
    if (g->h_stage) hipHostFree(g->h_stage);
    if (g->d_stage) hipFree(g->d_stage);
    delete g;
    return LDSO_OK;
}

// ldso_trace_on of every active member: ONE upload of [pose blocks | TraceJob table | first | zeroed count rows], one launch, ONE download of the count rows, one wait
int ldso_trace_group_on(ldso_trace_group_t *g, const uint8_t *active, const int *n_hosts, const float *const *KRKi, const float *const *Kt, const float *const *aff, int *counts_out) {
    REQ(g && n_hosts && KRKi && Kt && aff, "ldso_trace_group_on: null argument");
    RUN(group_check(g, "ldso_trace_group_on"));
    const int n = (int) g->m.size();
    std::vector<int> members;
    size_t poseFloats = 0;
    for (int i = 0; i < n; i++) {
        if (active && !active[i]) continue;
        const std::string who = "ldso_trace_group_on: member " + std::to_string(i);
        REQ(n_hosts[i] >= 1 && n_hosts[i] <= LDSO_MAX_FRAMES, who + ": n_hosts outside 1..LDSO_MAX_FRAMES");
        REQ(KRKi[i] && Kt[i] && aff[i], who + ": null pose array");
        REQ(g->m[(size_t) i]->haveFrame, who + ": set the new frame first");
        members.push_back(i);
        poseFloats += (size_t) n_hosts[i] * 14;
    }
    REQ(!members.empty(), "ldso_trace_group_on: no active member");
    CHK(hipSetDevice(g->device));
    const size_t nj = members.size();
    const size_t offJ = up16(poseFloats * 4), offF = up16(offJ + nj * sizeof(TraceJob)), offC = up16(offF + (nj + 1) * 4), total = offC + nj * 8 * 4;
    hipStream_t st = g->m[0]->stream;
    RUN(grow_arena(g->h_stage, g->d_stage, g->stageCap, total, 2, st));
    float *hPose = (float *) g->h_stage;
    TraceJob *hJ = (TraceJob *) (g->h_stage + offJ);
    int *hF = (int *) (g->h_stage + offF), *hC = (int *) (g->h_stage + offC);
    size_t po = 0;
    int waves = 0;
    for (size_t j = 0; j < nj; j++) {
        const int i = members[j], nh = n_hosts[i];
        const ldso_tracer *T = g->m[(size_t) i];
        memcpy(hPose + po, KRKi[i], (size_t) nh * 9 * 4);
        memcpy(hPose + po + nh * 9, Kt[i], (size_t) nh * 3 * 4);
        memcpy(hPose + po + nh * 12, aff[i], (size_t) nh * 2 * 4);
        const float *dPose = (const float *) g->d_stage + po;
        TraceJob &A = hJ[j];
        memset(&A, 0, sizeof(A));
        A.pts = T->d_pts; A.n = T->n; A.img = T->img; A.w = T->w; A.h = T->h;
        A.KRKi = dPose; A.Kt = dPose + nh * 9; A.aff = dPose + nh * 12; A.nHosts = nh;
        A.s = T->settings; A.counts = (int *) (g->d_stage + offC) + 8 * j;
        hF[j] = waves;                       // one wavefront per point; a member without points: first[j] == first[j + 1]
        waves += T->n;
        po += (size_t) nh * 14;
    }
    hF[nj] = waves;
    memset(hC, 0, nj * 8 * 4);
    CHK(hipMemcpyAsync(g->d_stage, g->h_stage, total, hipMemcpyHostToDevice, st));
    if (waves > 0) CHK(trace_launch_group((const TraceJob *) (g->d_stage + offJ), (const int *) (g->d_stage + offF), (int) nj, waves, st));
    CHK(hipMemcpyAsync(hC, g->d_stage + offC, nj * 8 * 4, hipMemcpyDeviceToHost, st));
    CHK(hipStreamSynchronize(st));
    if (counts_out) for (size_t j = 0; j < nj; j++) for (int k = 0; k < 6; k++) counts_out[6 * members[j] + k] = hC[8 * j + k];
    return LDSO_OK;
}

}  // extern "C"
