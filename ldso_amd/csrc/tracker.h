// tracker.h — what the translation units of the coarse tracker share: the records the kernels read, the handle, and the launchers that cross files
// (tracker.hip: the kernels of the LM loop; tracker_ref.hip: the reference point cloud; tracker_api.hip: handle and ldso_tr_*; tracker_hyp.cpp: host-only hypotheses).
#pragma once
#include <cstdlib>
#include <mutex>
#include <vector>
#include "hip_host.h"

#define TR_NT 256          // 4 wavefronts, one per SIMD: 512 registers (VGPR + AGPR) per lane - tr_eval keeps 4 points per lane in flight without scratch spills
#define TR_MAXL LDSO_PYR_LEVELS
#define TR_NACC 52         // sums of one evaluation (see tr_eval)
#define TR_GMAX 16         // most workgroups that share one hypothesis
#define TR_COOP_SLOTS 128  // = the maximum number of hypotheses of ldso_tr_track_batch: coop[] is indexed by hypothesis
#ifdef LDSO_STAMPS
#define LD_STAMP_ON_TR 1
#else
#define LD_STAMP_ON_TR 0
#endif

struct TrLevel {
    int w, h, n;
    float fx, fy, cx, cy;
    float Ki[9];
    const float *newImg;      // Vec3f AoS of the frame being tracked
    const float *refImg;      // Vec3f AoS of the reference keyframe
    float *pc_u, *pc_v, *pc_idepth, *pc_color;
    float *idepth, *wsum, *wsum_bak;
    int *blockCnt;            // compaction scratch
};

struct TrParams {
    TrLevel lv[TR_MAXL];
    int levels;
    float ref_a, ref_b, ref_exposure, new_exposure;
    float huberTH, coarseCutoffTH, affineOptModeA, affineOptModeB;
};

struct TrHyp {                 // one motion hypothesis in / result out
    double T[12];
    float a, b;
    int coarsestLvl;
    double minRes[5];
    double lastResiduals[5];
    double flow[3];
    int ok, iterations;
    int evals[5], pivotedSolves;          // calcRes evaluations per pyramid level (algorithmic bytes of a track = sum evals[l] * pc_n[l] * 64 B); LM solves that fell back to the pivoted factorisation
    double dbg[12];             // LDSO_STAMPS builds: time in tr_eval / serial LM sections / evals count
};

struct TrCoop {
    // every 64-bit word carries (payload << 32 | sequence number): a word is valid by itself, no fence / second round trip needed
    unsigned long long cmd[16];                          // R (9), t (3) as float, affine a, b, cut-off, level (-1: the track is over)
    unsigned long long part[TR_GMAX][TR_NACC][2];        // a helper's partial sums: low / high half of the double
};

struct TrJob {                 // one track of a grouped launch (k_tr_track_group): the member's parameters, the record of the try, its hand-over slot - all device memory
    const TrParams *P;
    TrHyp *hyp;
    TrCoop *coop;
};

// The launch shape of a track: G workgroups share each of `count` hypotheses / jobs on the large levels, as many as keep all count * G workgroups resident
// (one 256-thread workgroup per CU); many jobs fill the chip by themselves (G = 1, no hand-over and no residency condition).  More jobs than hand-over slots, or
// LDSO_TR_NO_COOP set in the environment (a device shared with another process or CU-masked, where co-residency cannot be promised): 1.
inline int tr_coop_width(int count, int numCU) {
    if (count > TR_COOP_SLOTS || getenv("LDSO_TR_NO_COOP")) return 1;
    return count * 16 <= numCU ? 16 : count * 12 <= numCU ? 12 : count * 8 <= numCU ? 8 : count * 4 <= numCU ? 4 : 1;
}

struct ldso_tracker {
    int device = 0, w = 0, h = 0, levels = 0;
    hipStream_t stream = nullptr;
    bool ownStream = false;
    ldso_settings_t settings;
    TrParams P;
    std::vector<void *> allocs;
    float *d_newImg[TR_MAXL] = {nullptr}, *d_refImg[TR_MAXL] = {nullptr};
    float *d_pts = nullptr;
    int *d_next = nullptr;            // per-point list links of the level-0 scatter
    float *d_color = nullptr;          // level-0 irradiance staging of ldso_tr_set_new_frame_image
    int ptsCap = 0;
    int *d_total = nullptr;
    double *d_T = nullptr, *d_acc = nullptr;
    TrHyp *d_hyp = nullptr, *h_hyp = nullptr;      // device records, pinned staging copy (no pageable-memory detour on the per-track round trip)
    TrParams *d_P = nullptr, *h_P = nullptr, Pdev;   // device copy of P (what the kernels read), pinned staging buffer, what the device copy holds
    TrCoop *d_coop = nullptr;         // cooperative evaluation: one record per hypothesis
    int numCU = 256, coopSeq = 1;     // sequence numbers already used by earlier launches on d_coop
    double lastAcc[TR_NACC];
    bool haveAcc = false;
    int lastEvals[5] = {0, 0, 0, 0, 0};      // of hypothesis 0 of the last track call
    int lastPivotedSolves = 0;               // LM solves of the last track call (all hypotheses) that fell back to the pivoted factorisation (ldlt8_lane)
    const void *inGroup = nullptr;           // the ldso_tr_group this tracker belongs to (at most one; ldso_tr_destroy refuses while set: the group dereferences its members)
};

// a group of trackers whose tracks share launches (tracker_group.hip)
struct ldso_tr_group {
    std::vector<ldso_tracker *> m;
    int device = 0, numCU = 256;
    TrCoop *d_coop = nullptr;         // [TR_COOP_SLOTS] hand-over records, indexed by the job of a launch
    int coopSeq = 1;                  // sequence numbers already used by earlier launches on d_coop
    GroupArena arena;                 // tr_group_layout
};

#pragma GCC visibility push(hidden)
// tracker_ref.hip: makeCoarseDepthL0 from n points (u, v, idepth, weight input) against the reference images already in H->P; ends synchronised
int tr_set_ref_common(ldso_tracker *H, float ref_a, float ref_b, float ref_exposure, const float *pts, int n);
// tracker.hip: the launches of its kernels.  G workgroups per hypothesis (16, 12, 8, 4: cooperative, all nhyp * G workgroups must be resident; 1: coop unused)
hipError_t tr_launch_track(int G, int nhyp, const TrParams *d_P, TrHyp *d_hyp, TrCoop *d_coop, int seq0, hipStream_t st);
// the same for the jobs of a group of trackers: job j = workgroups [j * G, (j + 1) * G), its hand-over slot is jobs[j].coop
hipError_t tr_launch_track_group(int G, int njobs, const TrJob *d_jobs, int seq0, hipStream_t st);
hipError_t tr_launch_calc(const TrParams *d_P, int lvl, const double *d_T, float a, float b, float cutoffTH, double *d_acc, hipStream_t st);
hipError_t tr_launch_solve8(const double *d_H, const double *d_b, double diagScale, double *d_x, int *d_pivoted);
// tracker_api.hip: a cooperative launch (G > 1) on `st`.  tr_coop_begin takes the process-wide lock into `lk`, orders the stream behind the last cooperative launch
// on the device and clears the records when the sequence numbers run out; the caller launches with seq0 = coopSeq, then tr_coop_end advances the counter and records
// the launch for the next one.  The lock is held from begin to end.
int tr_coop_begin(int device, hipStream_t st, TrCoop *d_coop, int &coopSeq, std::unique_lock<std::mutex> &lk);
int tr_coop_end(int device, hipStream_t st, int &coopSeq);
// tracker_api.hip: FullSystem::trackNewCoarse around its tracks, shared by ldso_tr_track_new_coarse and ldso_tr_group_track_new_coarse
struct TrNewCoarse {
    std::vector<double> T, T0, lr, flow;      // 83 tries: guess / result pose, the untouched guesses, lastResiduals, flow indicators
    std::vector<float> aff;
    std::vector<int> ok;
    int n = 0, coarsest = 0, best = -1, used = 0;
    double achieved[5];
    bool done = false;
};
int tr_new_coarse_before(TrNewCoarse &S, int levels, const double sprelast[12], const double slast[12], const double lastF[12], int poses_valid, const float aff_last[2]);
int tr_new_coarse_between(TrNewCoarse &S, const double lastCoarseRMSE[5], double reTrackThreshold);          // after try 0: S.done, or the remaining tries go on
int tr_new_coarse_after(TrNewCoarse &S, bool ranRest, const double lastF[12], const float aff_last[2], double lastCoarseRMSE[5], double reTrackThreshold,
                        double result4[4], double new_w2c[12], float aff_out[2], int *tries_consumed, int *good);
#if LD_STAMP_ON_TR
void tr_fetch_phase_stamps(long long ph[5][8]);          // reads and clears the per-level phase times of tr_eval
#endif
#pragma GCC visibility pop
