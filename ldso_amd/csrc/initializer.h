// initializer.h — what the translation units of the monocular initialiser share: the records the kernels read, the handle, and the launchers that cross files
// (initializer.hip: the kernels; initializer_api.hip: handle, ldso_init_*, point record conversion; initializer_sched.cpp: the host-only optReg sweep schedule).
#pragma once
#include "hip_host.h"

#define INI_MAXL 5            // maxIterations[] has five entries (CoarseInitializer.cc:43)
#define INI_NT 256            // threads of an eval block: 32 points x 8 pattern pixels
#define INI_MAXBLK 256        // eval blocks (= partial rows) per launch
#define INI_NPART 128         // floats per partial row
#define INI_CT 1024           // threads of the control block (its per-point passes are latency bound: many loads in flight)
#define INI_NB 12             // neighbour row pitch (10 used)
// partial row layout
#define PR_SC 45              // 8 x 9 Schur block
#define PR_SC88 117
#define PR_E 118
#define PR_ECO 119
#define PR_ECN 120
#define PR_ECC 121
#define PR_N 122
#define INI_LDS_EXTRA 3       // slots behind the n keys of the control block's LDS array (see the sweeps)
#define INI_SWPAD 16          // unconditional prefetch: the schedule arrays carry INI_SWPAD passes of padding (idle lanes) behind the last pass
#define INI_PT 256            // threads of a k_ini_prep block
#define INI_BEGIN 0           // phases of k_ini_ctl
#define INI_STEP 1
#define INI_STAGE 2

struct IniLevel {
    int n, w, h, nPass;
    float fx, fy, cx, cy;
    double Ki[9];
    const float *first, *cur;           // dIp[lvl] of the first and of the new frame
    float *u, *v, *idepth, *idepth_new, *iR, *iRSumNum, *lastHessian, *lastHessian_new, *maxstep, *energy0, *energy1, *energy_new0, *energy_new1, *outlierTH;
    int *isGood, *isGood_new, *parent, *nb;
    float *jb[2];                       // [n][10]
    // resetPoints sweep (top level only; one lane per point):
    const int *sched;                   // [nPass][64] point index or -1
    const int *schedOff;                // [nPass][64] LDS byte offset of the point's key (dummy slot n*4 for idle lanes)
    const int *schedNb;                 // [nPass][64][INI_NB] LDS byte offsets of the neighbours' keys in schedule order (dummy slot: none)
    // optReg sweep (two lanes per point): schedule of passes of <= 32 points and the per-lane inputs ini_prep writes before every sweep
    int nPass2;
    int nIdle;
    const int *slotOf;                  // [n] place of the point in the schedule: pass * 32 + position
    const int *idleSlot;                // [nIdle] places (of nPass2 + INI_SWPAD passes) that hold no point
    int4 *swRec;                        // [nPass2 + INI_SWPAD][64][2]: see SwRec
    const int *childOff, *childIdx;     // children (points of level - 1) of every point of this level, ascending
};

struct IniCtl {
    double Tcur[12], Tnew[12];
    float aCur, bCur, aNew, bNew;
    float inc[8];
    float lambda;
    float H[64], b[8], Hsc[64], bsc[8], resOld[3];
    float Hn[64], bn[8], Hscn[64], bscn[8], resNew[3], ec[3];
    int lvl, mode, iteration, fails, done, snapped, snappedAt, frameID, jbSel, applyPending, evals, ready;
    int idleWritten;                    // the records of the schedule places that hold no point are written (ini_prep_idle)
    int ldsBase;                        // LDS address of the control block's key array (the sweep records hold LDS addresses)
    int sweepDue, upGoing;              // level + 1 whose optReg sweep (view: good points, applied depths) is the next control step's; in the propagateUp chain
    int steps;                          // control steps of this frame so far (INI_STEP launches that did something)
    int prepReady;                      // k_ini_prep has written the records of the level for the step this evaluation tried; consumed by the control step
    long long dbgSweepTicks, dbgSweepPasses, dbgCtlTicks, dbgSweeps, dbgPrepTicks, dbgFrontTicks, dbgTailTicks, dbgSpare;     // LDSO_STAMPS builds only (100 MHz wall clock)
};

struct IniParams {
    IniLevel L[INI_MAXL];
    int levels, fixAffine;
    float huberTH, firstExposure, newExposure;
    IniCtl *ctl;
    float *part;                        // [INI_MAXBLK][INI_NPART]
};

struct ldso_initializer {
    int device = 0, w = 0, h = 0, levels = 0;
    hipStream_t stream = nullptr;
    bool ownStream = false;
    IniParams P;
    std::vector<void *> allocs, levelAllocs;
    float *d_first[INI_MAXL] = {nullptr}, *d_new[INI_MAXL] = {nullptr};
    float *d_color = nullptr;
    int n[INI_MAXL] = {0};
    size_t ldsBytes = 0;
    int prepBlocks = 1;                 // k_ini_prep: one thread per point of the largest level
    int lastSteps = 0, stepsTaken = 0;  // control steps of the previous frame / of the frame just read back (get_state)
    int firstSteps = 0;                 // ldso_init_set_schedule: control steps of the first batch (0 = by the previous frame)
    bool prepareOnGrid = true;          // ldso_init_set_schedule: k_ini_prep launches (false: the control block prepares every sweep)
    bool frameDone = false;
    bool snappedAtFrameStart = false;   // host copy of the state's snapped (get_state / set_state / set_first): before the snap optReg does not sweep and the
                                        // k_ini_prep launches would be empty (the frame that snaps prepares its sweeps in the control block)
    bool haveFirst = false, haveNew = false;
    // setFirst from a pyramid (init_first.hip): sparsityFactor, the byte map of makePixelStatus with its counters, the records and positions of every level
    int sparsity = 5;                   // Setting.cc:126
    std::vector<void *> firstAllocs;    // freed by destroy
    unsigned char *d_status = nullptr;  // (w / 2) * (h / 2) bytes
    int statusLvl = 0;                  // the level the map was last written for
    int *d_fctl = nullptr, *d_rowCount = nullptr, *d_rowStart = nullptr;
    ldso_init_point_t *d_rec[INI_MAXL] = {nullptr};
    float *d_uv[INI_MAXL] = {nullptr};
    int recCap[INI_MAXL] = {0};
    std::vector<ldso_init_point_t> firstRec[INI_MAXL];      // the records as set_first_frame built them (weights and my_type are not part of the SoA)
    bool profileFirst = false;
    float usFirst[6] = {0, 0, 0, 0, 0, 0};
};

#pragma GCC visibility push(hidden)
// initializer.hip: the launches of its kernels (the control block takes ldsBytes of dynamic LDS, which ini_ctl_reserve_lds has to allow first)
hipError_t ini_ctl_reserve_lds(size_t ldsBytes);
void ini_launch_eval(const IniParams &P, int stage, hipStream_t st);
void ini_launch_prep(const IniParams &P, int blocks, hipStream_t st);
void ini_launch_ctl(const IniParams &P, int phase, size_t ldsBytes, hipStream_t st);
// initializer_api.hip: ldso_init_set_first without its image build - levels, schedules, records and the state of setFirst (the caller fills d_first and sets haveFirst)
int ini_set_first_records(ldso_initializer *H, const float calib[4], float ab_exposure, const ldso_init_point_t *const *points, const int *n_points, float huberTH, int fixAffine);
// pixel_select.hip: the byte map (0 / 1 / 2 / 4) of the selector's last make_maps, its size and stream
const unsigned char *pix_map_device(const struct ldso_pixsel *P, int *w, int *h, int *device);
#pragma GCC visibility pop
