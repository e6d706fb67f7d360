// tracker_group.hip — ldso_tr_group_* (include/ldso_hip.h): the tracks of several trackers (independent sequences on one card) in one launch.  A sequence meets
// CoarseTracker::trackNewestCoarse on every frame; one track alone is latency bound and uses 16 of the CUs (k_tr_track<16>), so the tracks of a group run side by side:
// k_tr_track_group (tracker.hip) gives every job its own TrParams, record and hand-over slot.  The members stay ordinary trackers; the group reads their current
// parameters at every call and owns what a launch needs beyond them: the staging arena, the hand-over records and their sequence counter.
#include "tracker.h"

namespace {

struct GroupJobIn { int p; const double *T; float a, b; int coarsest; const double *minRes; };      // p: index into the call's list of members that take part

constexpr GroupRule RULE = {"a tracker", "ldso_tr_set_stream", TR_COOP_SLOTS};          // a hand-over slot per job: the bound is the slots'
static_assert(sizeof(TrParams) == 904 && sizeof(TrJob) == 24 && sizeof(TrHyp) == 344, "the rows of tr_group_layout as tests/test_group_stage_cpu.py sizes them");

// One launch for `jobs` (the jobs of a member are contiguous, in the order of `members`): ONE upload of [TrParams of the members | TrJob table | TrHyp records], the
// kernel, ONE download of the records, one wait.  `out` = the records on the host (the group's pinned arena: valid until the next launch).  Every member's lastEvals /
// lastPivotedSolves are written as ldso_tr_track_batch writes them for the same tries.
int group_launch(ldso_tr_group *g, const std::vector<int> &members, const std::vector<GroupJobIn> &jobs, TrHyp *&out) {
    const size_t np = members.size(), nj = jobs.size();
    const TrGroupLayout L = tr_group_layout(np, nj, sizeof(TrParams), sizeof(TrJob), sizeof(TrHyp));
    hipStream_t st = g->m[0]->stream;
    RUN(group_arena_grow(g->arena, L.total, st));
    char *const h_stage = g->arena.h_stage, *const d_stage = g->arena.d_stage;
    const int G = tr_coop_width((int) nj, g->numCU);          // G > 1 only for nj <= TR_COOP_SLOTS: job j's hand-over record is d_coop[j]
    TrParams *hP = (TrParams *) (h_stage + L.params);
    TrJob *hJ = (TrJob *) (h_stage + L.jobs);
    TrHyp *hH = (TrHyp *) (h_stage + L.down);
    for (size_t i = 0; i < np; i++) hP[i] = g->m[(size_t) members[i]]->P;
    for (size_t j = 0; j < nj; j++) {
        const GroupJobIn &in = jobs[j];
        TrHyp &hy = hH[j];
        memset(&hy, 0, sizeof(TrHyp));
        memcpy(hy.T, in.T, 96);
        hy.a = in.a; hy.b = in.b; hy.coarsestLvl = in.coarsest;
        for (int k = 0; k < 5; k++) hy.minRes[k] = in.minRes ? in.minRes[k] : NAN;
        hJ[j].P = (const TrParams *) (d_stage + L.params) + in.p;
        hJ[j].hyp = (TrHyp *) (d_stage + L.down) + j;
        hJ[j].coop = G > 1 ? g->d_coop + j : nullptr;
    }
    CHK(hipMemcpyAsync(d_stage, h_stage, L.total, hipMemcpyHostToDevice, st));
    const TrJob *dJ = (const TrJob *) (d_stage + L.jobs);
    if (G > 1) {
        std::unique_lock<std::mutex> lk;
        RUN(tr_coop_begin(g->device, st, g->d_coop, g->coopSeq, lk));
        CHK(tr_launch_track_group(G, (int) nj, dJ, g->coopSeq, st));
        RUN(tr_coop_end(g->device, st, g->coopSeq));
    } else {
        CHK(tr_launch_track_group(1, (int) nj, dJ, 0, st));
    }
    CHK(hipMemcpyAsync(hH, d_stage + L.down, L.downBytes, hipMemcpyDeviceToHost, st));
    CHK(hipStreamSynchronize(st));
    for (size_t j = 0; j < nj; j++) if (hH[j].ok == -2) {
        ldso_set_error("ldso_tr_track: the cooperating workgroups of a hypothesis did not become co-resident (device shared with another process or CU-masked?); set LDSO_TR_NO_COOP=1");
        return LDSO_E_HIP;
    }
    for (size_t j = 0; j < nj; j++) {
        ldso_tracker *H = g->m[(size_t) members[(size_t) jobs[j].p]];
        if (j == 0 || jobs[j - 1].p != jobs[j].p) { memcpy(H->lastEvals, hH[j].evals, sizeof(H->lastEvals)); H->lastPivotedSolves = 0; }
        H->lastPivotedSolves += hH[j].pivotedSolves;
    }
    out = hH;
    return LDSO_OK;
}

}  // namespace

extern "C" {

int ldso_tr_group_create(ldso_tracker_t *const *trackers, int n, ldso_tr_group_t **out) {
    RUN(group_admit(trackers, n, out, "ldso_tr_group_create", RULE));
    CHK(hipSetDevice(trackers[0]->device));
    ldso_tr_group *g = new ldso_tr_group();
    g->device = trackers[0]->device; g->numCU = trackers[0]->numCU;
    auto body = [&]() -> int {
        CHK(hipMalloc((void **) &g->d_coop, TR_COOP_SLOTS * sizeof(TrCoop)));
        return zero_fill(g->d_coop, TR_COOP_SLOTS * sizeof(TrCoop));
    };
    RUN(finish_create(body(), g, out, ldso_tr_group_destroy));
    g->m.assign(trackers, trackers + n);
    group_join(g);
    return LDSO_OK;
}

int ldso_tr_group_destroy(ldso_tr_group_t *g) {
    if (!g) return LDSO_OK;
    hipSetDevice(g->device);
    if (!g->m.empty()) hipStreamSynchronize(g->m[0]->stream);
    group_leave(g);
    if (g->d_coop) hipFree(g->d_coop);
    group_arena_free(g->arena);
    delete g;
    return LDSO_OK;
}

int ldso_tr_group_coop_width(ldso_tr_group_t *g, int n_jobs, int *G) {
    REQ(g && G && n_jobs >= 1, "ldso_tr_group_coop_width: bad arguments");
    *G = tr_coop_width(n_jobs, g->numCU);
    return LDSO_OK;
}

// CoarseTracker::trackNewestCoarse (CoarseTracker.cc:61-217) of every active member: ldso_tr_track per member, one launch for all of them
int ldso_tr_group_track(ldso_tr_group_t *g, const uint8_t *active, double *T_inout, float *aff_inout, const int *coarsestLvl, const double *minRes, double *lastResiduals,
                        double *flow, int *ok, int *iterations) {
    REQ(g && T_inout && aff_inout && coarsestLvl, "ldso_tr_group_track: null argument");
    RUN(group_check(g->m.data(), g->m.size(), "ldso_tr_group_track", RULE));
    std::vector<int> members;
    RUN(group_active((int) g->m.size(), active, "ldso_tr_group_track", members, [&](int i) -> const char * {
        return coarsestLvl[i] >= 0 && coarsestLvl[i] < 5 && coarsestLvl[i] < g->m[(size_t) i]->levels ? nullptr : "coarsestLvl outside a member's pyramid levels";
    }));
    std::vector<GroupJobIn> jobs;
    for (size_t k = 0; k < members.size(); k++) {
        const int i = members[k];
        jobs.push_back({(int) k, T_inout + 12 * i, aff_inout[2 * i], aff_inout[2 * i + 1], coarsestLvl[i], minRes ? minRes + 5 * i : nullptr});
    }
    CHK(hipSetDevice(g->device));
    TrHyp *hy = nullptr;
    RUN(group_launch(g, members, jobs, hy));
    for (size_t j = 0; j < members.size(); j++) {
        const int i = members[j];
        memcpy(T_inout + 12 * i, hy[j].T, 96);
        aff_inout[2 * i] = hy[j].a; aff_inout[2 * i + 1] = hy[j].b;
        if (lastResiduals) memcpy(lastResiduals + 5 * i, hy[j].lastResiduals, 40);
        if (flow) memcpy(flow + 3 * i, hy[j].flow, 24);
        if (ok) ok[i] = hy[j].ok;
        if (iterations) iterations[i] = hy[j].iterations;
    }
    return LDSO_OK;
}

// Vec4 FullSystem::trackNewCoarse (FullSystem.cc:179-386) of every active member (ldso_tr_track_new_coarse per member) in two launches for the whole group: try 0 of
// every member, then the remaining tries of all members whose loop goes on (:355 not met), concatenated.
int ldso_tr_group_track_new_coarse(ldso_tr_group_t *g, const uint8_t *active, const double *sprelast, const double *slast, const double *lastF, const int *poses_valid,
                                   const float *aff_last, double *lastCoarseRMSE, const double *reTrackThreshold, double *result4, double *new_w2c, float *aff_out,
                                   int *tries_consumed, int *good) {
    REQ(g && sprelast && slast && lastF && poses_valid && aff_last && lastCoarseRMSE && reTrackThreshold && result4 && new_w2c && aff_out,
        "ldso_tr_group_track_new_coarse: null argument");
    RUN(group_check(g->m.data(), g->m.size(), "ldso_tr_group_track_new_coarse", RULE));
    std::vector<int> members;
    RUN(group_active((int) g->m.size(), active, "ldso_tr_group_track_new_coarse", members, [&](int i) -> const char * {
        return g->m[(size_t) i]->levels <= 5 ? nullptr : "a member has more than five pyramid levels";
    }));
    CHK(hipSetDevice(g->device));
    std::vector<TrNewCoarse> S(members.size());
    std::vector<GroupJobIn> jobs;
    for (size_t k = 0; k < members.size(); k++) {
        const int i = members[k];
        RUN(tr_new_coarse_before(S[k], g->m[(size_t) i]->levels, sprelast + 12 * i, slast + 12 * i, lastF + 12 * i, poses_valid[i], aff_last + 2 * i));
        jobs.push_back({(int) k, S[k].T.data(), S[k].aff[0], S[k].aff[1], S[k].coarsest, nullptr});
    }
    // a launch's records back into the members' try lists: job j is try `first + (j - the member's first job)` of member jobs[j].p of `who`
    auto take = [&](const std::vector<GroupJobIn> &js, const std::vector<size_t> &who, const TrHyp *hy, int first) {
        int t = first;
        for (size_t j = 0; j < js.size(); j++) {
            t = (j == 0 || js[j - 1].p != js[j].p) ? first : t + 1;
            TrNewCoarse &s = S[who[(size_t) js[j].p]];
            memcpy(s.T.data() + 12 * t, hy[j].T, 96);
            s.aff[2 * t] = hy[j].a; s.aff[2 * t + 1] = hy[j].b;
            memcpy(s.lr.data() + 5 * t, hy[j].lastResiduals, 40);
            memcpy(s.flow.data() + 3 * t, hy[j].flow, 24);
            s.ok[(size_t) t] = hy[j].ok;
        }
    };
    TrHyp *hy = nullptr;
    std::vector<size_t> all(members.size());
    for (size_t k = 0; k < all.size(); k++) all[k] = k;
    RUN(group_launch(g, members, jobs, hy));
    take(jobs, all, hy, 0);
    std::vector<int> restMembers;
    std::vector<size_t> restWho;
    jobs.clear();
    for (size_t k = 0; k < members.size(); k++) {
        const int i = members[k];
        RUN(tr_new_coarse_between(S[k], lastCoarseRMSE + 5 * i, reTrackThreshold[i]));
        if (S[k].done || S[k].n <= 1) continue;
        for (int t = 1; t < S[k].n; t++) jobs.push_back({(int) restMembers.size(), S[k].T.data() + 12 * t, S[k].aff[2 * t], S[k].aff[2 * t + 1], S[k].coarsest, nullptr});
        restMembers.push_back(i); restWho.push_back(k);
    }
    if (!jobs.empty()) {
        RUN(group_launch(g, restMembers, jobs, hy));
        take(jobs, restWho, hy, 1);
    }
    for (size_t k = 0; k < members.size(); k++) {
        const int i = members[k];
        const bool rest = !S[k].done && S[k].n > 1;
        RUN(tr_new_coarse_after(S[k], rest, lastF + 12 * i, aff_last + 2 * i, lastCoarseRMSE + 5 * i, reTrackThreshold[i], result4 + 4 * i, new_w2c + 12 * i, aff_out + 2 * i,
                                tries_consumed ? tries_consumed + i : nullptr, good ? good + i : nullptr));
    }
    return LDSO_OK;
}

}  // extern "C"
