// ba_host.h — what the host-side translation units of the bundle adjustment share (the ba_*.hip units and act_select.hip, which also compacts tracers): the
// launcher prototypes of its kernel files, the handle and the batch, and the host helpers of the BA that cross files (hidden: none of them is part of the
// library's interface).  What every host-side unit shares is hip_host.h; a stage unit includes that, never this file.
#pragma once
#include "hip_host.h"           // CHK, launch_lds, the create / allocation / stream / arena helpers
#include "trace.h"              // ldso_tracer, CompactArgs, trace_compact_* (act_select.hip)
#include "ba_dev.h"
#include "ba_solve.h"

// k_activate's view of a call (ba_activate.hip), and one window's share of a batched one (k_activate_batch): `item` = the window's BatchItem in ldso_ba_batch::d_items
struct ActArgs {
    const ldso_immature_t *pts;
    ldso_activation_t *out;
    int n, minObs, GNIts;
    float minIdepthH_act;
    const int32_t *sel;      // non-null: wavefront i works on pts[sel[i]] for i < *nSel (the list act_select.hip left on the device), out[i] is its record
    const int32_t *nSel;
};
struct ActWin { ActArgs A; int32_t item, pad_[3]; };
// one window's activation: n wavefronts over d_pts -> d_out, or over the list d_sel of length *d_nSel (both null: every point); every byte set, the records cross PCIe in tables
inline ActWin act_win(const ldso_immature_t *d_pts, ldso_activation_t *d_out, int n, int minObs, float minIdepthH_act, int GNIts, const int32_t *d_sel, const int32_t *d_nSel, int item) {
    ActWin T;
    memset(&T, 0, sizeof(T));
    T.A.pts = d_pts; T.A.out = d_out; T.A.n = n; T.A.minObs = minObs; T.A.GNIts = GNIts; T.A.minIdepthH_act = minIdepthH_act; T.A.sel = d_sel; T.A.nSel = d_nSel; T.item = item;
    return T;
}

// the launchers, defined beside their kernels (ba_linearize / ba_linearize_batch / ba_reduce / ba_solve / ba_solve_batch / ba_step / ba_activate .hip)
hipError_t ba_launch_linearize(const BaPtrs &B, const BaDims &D, const ResSet &cur, const ResSet &nxt, const ldso_settings_t &S, bool hasL, bool fix, int stepMode, const GnInit &gi, hipStream_t st);
hipError_t ba_launch_reduce(const BaPtrs &B, const BaDims &D, const ResSet &S, const ChunkStarts &chunkStart, bool hasL, int GSP, int atomicMode, bool hasPrior, float calibPrior, double l1, double il, int itCheck, hipStream_t st);
hipError_t ba_launch_gather(const BaPtrs &B, const BaDims &D, const ResSet &S, bool hasL, bool hasPrior, int GSP, double lambda, const ldso_settings_t &St, int mode, double *rbuf, hipStream_t st);
hipError_t ba_launch_solve(const BaPtrs &B, const BaDims &D, const ResSet &S, const ldso_settings_t &St, const SolveArgs &A, hipStream_t st);
hipError_t ba_launch_point_step(const BaPtrs &B, const BaDims &D, const ResSet &S, int mode, hipStream_t st);
hipError_t ba_launch_linearize_one(const BaPtrs &B, const BaDims &D, const ResSet &cur, const ResSet &nxt, const ldso_settings_t &S, int stepMode, const GnInit &gi, const LinHead &hd, hipStream_t st);
hipError_t ba_launch_linearize_marg(const BaPtrs &B, const BaDims &D, const ResSet &cur, const ResSet &nxt, const ldso_settings_t &S, const int32_t *margFlags, hipStream_t st);
hipError_t ba_launch_marg_frame(const BaPtrs &B, const BaDims &D, int idx, double *work, double *outH, double *outb, hipStream_t st);
hipError_t ba_launch_acc_init(const BaPtrs &B, const BaDims &D, const GnInit &gi, hipStream_t st);
hipError_t ba_launch_gn_export(const BaPtrs &B, const BaDims &D, const ResSet &S, double *tail, hipStream_t st);
hipError_t ba_launch_activate(const BaPtrs &B, const BaDims &D, const ldso_settings_t &S, const ActArgs &A, hipStream_t st);
hipError_t ba_launch_activate_batch(const BatchItem *d_items, const ActWin *d_tab, const int32_t *d_waveOff, int nTab, int totalWaves, int nsg, const ldso_settings_t &S, hipStream_t st);
hipError_t ba_launch_linearize_batch(const BatchItem *d_items, const BatchBlock *d_blocks, int totalChunks, const int32_t *d_wgStart, int nWG, int FS, int cur, const ldso_settings_t &S, int stepMode, float calibPrior, hipStream_t st, int itCheck = -1);
hipError_t ba_launch_reduce_batch(const BatchItem *d_items, int nWin, int totalBlocks, int cur, float calibPrior, double l1, double il, hipStream_t st, int itCheck = -1);
hipError_t ba_launch_gn_solve_batch(const BatchItem *d_items, int nWin, const BaDims &Dmax, int cur, const ldso_settings_t &St, int iteration, double lambda, hipStream_t st, int logIdx = -1, int itCheck = -1);
// ldso_ba_batch_optimize: energy log / LD_SC_STOP reset, the batched tail (k_solve_batch: phase 0 on the applied set, phase 1 on the fixed one), the fixing linearisation
hipError_t ba_launch_batch_begin(const BatchItem *d_items, int nWin, int mnumOptIts, int forceAll, hipStream_t st);
hipError_t ba_launch_solve_batch(const BatchItem *d_items, int nWin, const BaDims &Dmax, const ldso_settings_t &St, unsigned flags, int phase, double *d_scalarsOut, hipStream_t st);
hipError_t ba_launch_linearize_batch_fix(const BatchItem *d_items, const BatchBlock *d_blocks, int totalChunks, const int32_t *d_wgStart, int nWG, const ldso_settings_t &S, float calibPrior, hipStream_t st);
// ldso_ba_batch_marginalize_points / _frame: the MARG linearisation, the non-atomic reduce and the fused gather + prior update of every window that takes part; k_marg_frame per window
hipError_t ba_launch_linearize_batch_marg(const BatchItem *d_items, const BatchBlock *d_blocks, int totalChunks, const int32_t *d_wgStart, int nWG, const MargWin *d_mw, const int32_t *d_flags, const ldso_settings_t &S, hipStream_t st);
hipError_t ba_launch_reduce_batch_marg(const BatchItem *d_items, const MargWin *d_mw, int nWin, int totalBlocks, int maxGSP, hipStream_t st);
hipError_t ba_launch_marg_gather_update_batch(const BatchItem *d_items, const MargWin *d_mw, int nWin, int maxN, double w, double *d_out, hipStream_t st);
hipError_t ba_launch_marg_frame_batch(const BatchItem *d_items, int nWin, const MargWin *d_mw, double *d_out, hipStream_t st);
hipError_t ba_launch_lm_energies(const BaPtrs &B, const BaDims &D, const ResSet &S, float calibPrior, bool hasPrior, hipStream_t st);
hipError_t ba_launch_marg_update(const BaPtrs &B, const BaDims &D, double w, hipStream_t st);
hipError_t ba_launch_gn_solve(const BaPtrs &B, const BaDims &D, const ResSet &S, const ldso_settings_t &St, const SolveArgs &A, hipStream_t st);
hipError_t ba_launch_reduce_solve(const BaPtrs &B, const BaDims &D, const ResSet &S, const ldso_settings_t &St, const SolveArgs &A, const ChunkStarts &chunkStart, int atomicMode, float calibPrior, double l1, double il, hipStream_t st);

struct Timer { hipEvent_t a, b; int which; };
struct ldso_ba {
    int device = 0, w = 0, h = 0, maxF = 0, maxP = 0, FSmax = 0, maxChunks = 0, numCU = 256;
    hipStream_t stream = nullptr;
    bool ownStream = false;
    ldso_settings_t settings;
    BaDims D;
    BaPtrs B;
    ResSet sets[2];
    int cur = 0;
    bool pendingApply = false;
    bool hasL = false;
    bool hasPrior = false;
    int GSP = 0;
    int R = 0;
    float *imgSlots[LD_MAXF] = {nullptr};
    bool imgOwned[LD_MAXF] = {false};
    int32_t *d_chunkStart = nullptr;
    int *d_waitCtr = nullptr;          // k_reduce_solve: the arrival words of the reduce workgroups, LD_ARRIVE_BYTES (ba_dev.h; zero between launches)
    int32_t *d_margFlags = nullptr;
    float *d_color = nullptr;          // irradiance staging of ldso_ba_set_image_raw
    void *d_act = nullptr;             // staging of ldso_ba_activate_points: n immature records + n results
    int actCap = 0;
    void *d_sel = nullptr;             // device arena of ldso_ba_select_candidates / ldso_ba_select_activate_points (act_select.hip: inputs, results, scratch, the distance map)
    size_t selCap = 0, selMapOffset = 0;
    int selW1 = 0, selH1 = 0;          // size of the distance map the last selection left in d_sel (0: none yet)
    int selLdsLimit = -1, selLdsSet = 0; // dynamic LDS the selection kernel may have on this device (-1: not asked yet), and what its attribute was last raised to
    std::vector<char> selHost;         // host staging of the same calls (one upload, one download)
    double *ownAcc = nullptr;          // the handle's own HFinal/bFinal accumulator (B.acc may point at a caller's all-reduce buffer)
    ChunkStarts chunkStarts;
    ldso_rawjac_t *d_dumpJ = nullptr;
    std::vector<int32_t> flat2slot;
    std::vector<int32_t> imageSlot;
    std::vector<void *> allocs;
    // host staging of the window (for shard rebuilds)
    std::vector<int32_t> h_phost;
    // window upload: ONE pinned staging arena -> ONE device arena -> one scatter kernel (k_win_scatter) instead of ~25 copies + ~20 fills
    // the window's descriptors in device memory (one BatchItem): the plain linearisation of the GN iteration reads them from there - passed
    // as kernel arguments, the ~150 pointers outgrow the scalar registers (400 SGPR spill moves in the kernel)
    BatchItem *d_item = nullptr, *h_item = nullptr;
    BatchBlock *d_blocks = nullptr;    // [maxChunks] the window's chunks as k_linearize_batch reads them (window index 0)
    std::vector<BatchBlock> h_blocks;
    bool appliedValid = false;         // the applied residual set holds a linearisation of the resident window (its per-chunk partials feed the next reduce)
    LinHead linHead;                   // chunk geometry of the current window by value (k_linearize_one)
    int reduceSplits = LD_SCT_KS;      // K-splits per 16 x 16 Schur tile (BaDims::ks; ldso_ba_set_reduce_splits)
    bool linHeadOk = false;            // the chunks are regular (every host cut into CH-point pieces): true for everything build_chunks produces
    const void *inBatch = nullptr;     // the ldso_ba_batch this handle belongs to (at most one; it must outlive the batch: ldso_ba_destroy refuses while set)
    int chunkPoints = 0;               // points per workgroup of k_linearize: 0 = as few as keep the grid within one wave of workgroups (one window alone on the chip)
    std::vector<int32_t> chunkCuts;    // explicit chunk ends (ldso_ba_set_chunk_cuts / ldso_ba_batch_create: uneven chunks, one workload per workgroup); empty: regular chunks of chunkPoints
    BatchItem itemShadow;
    bool itemValid = false;
    int *h_stop = nullptr, *d_stop = nullptr;      // host-mapped word (and its device address): which iteration ended an un-forced optimize() loop
    char *h_down = nullptr;             // pinned arena of the fetch functions (ldso_ba_get_residuals / _points / _frames): device -> pinned host at link speed, one wait
    size_t downCap = 0;
    bool stageBusy = false;            // an asynchronous copy out of h_stage may still be in flight (ldso_ba_set_prior): the next user of the arena waits first
    // an edit of the resident window being recorded (ldso_ba_window_begin .. ldso_ba_window_commit): frames and residual targets are named by their index in the
    // RESIDENT window (inserted frames: oF, oF + 1, ...), points by their resident row
    struct NewPoint { ldso_point_t p; int before; std::vector<ldso_residual_t> res; float mrb; int32_t ngr; };
    struct WindowEdit {
        bool active = false;
        int oF = 0, oP = 0;
        std::vector<char> frameGone, rowGone;
        std::vector<int32_t> insertedSlots;
        std::vector<uint32_t> mask;          // per resident row, bit = edit-time frame id
        std::vector<NewPoint> fresh;
    } edit;
    char *h_stage = nullptr, *d_stage = nullptr;
    size_t stageCap = 0;
    // profiling
    bool profile = false;
    std::vector<Timer> timers;
    double tsum[5] = {0, 0, 0, 0, 0};
    int tcnt[5] = {0, 0, 0, 0, 0};
    int lastIterations = 0;
    bool noFusedLaunch = false;        // debug: k_reduce and k_gn_solve as two launches even where the fused k_reduce_solve applies
    // ldso_ba_enqueue_gn replays a cached HIP graph when the same launch sequence was enqueued before: the key is EVERYTHING the launches take as
    // arguments (pointer tables, dimensions, both residual sets, settings, chunk geometry, flags, stream, first iteration, count, parity of the sets),
    // byte for byte (round 6: the 64-bit hash of those bytes only pre-selects - a collision must not replay another window's launches)
    struct GnGraph { unsigned long long sig; std::vector<unsigned char> key; hipGraphExec_t exec; hipGraph_t graph; };
    std::vector<GnGraph> gnGraphs;
    std::vector<unsigned char> gnKeyScratch;      // the key of the current call (kept to avoid an allocation per enqueue)
    bool gnUseGraphs = true;
    double *distBuf = nullptr;         // ldso_ba_enqueue_gn_rccl / _p2p: all-reduce buffer [HFinal | bFinal | scalars | candidates]
    unsigned p2pSeq = 0;               // ldso_ba_enqueue_gn_p2p: exchanges done (the tag of the hand-over words)
    int *d_p2pErr = nullptr;           // set by k_p2p_sum when a peer's words did not arrive in time
    double neverStop = 1e300;          // source of the LD_SC_STOP reset (outlives the asynchronous copy)
};

#define REQ_UNSHARDED(name) REQ(H->D.pBegin == 0 && H->D.pEnd == H->D.P, name ": not available on a sharded handle (ldso_ba_set_shard): " \
                                    "use ldso_ba_gn_reduce_local / ldso_ba_gn_solve_reduced or ldso_ba_reduce_local / ldso_ba_solve_reduced around the all-reduce")

// a batch of windows (ba_batch.hip)
struct ldso_ba_batch {
    std::vector<ldso_ba *> h;
    BatchItem *d_items = nullptr;      // [n] numbered over the whole batch, then [n] numbered per half (see ldso_ba_batch_enqueue_gn)
    std::vector<BatchItem> items;
    BatchBlock *d_blocks = nullptr;    // [totalChunks] workgroups of the whole batch, then [halfChunks[0]] + [halfChunks[1]] per half
    std::vector<BatchBlock> blocks;
    size_t blocksCap = 0;
    int chunkPoints = 0;               // the chunking ldso_ba_batch_create gave its windows
    int totalChunks = 0, totalReduce = 0, FS = 0, cur = 0;
    int n0 = 0;                        // windows in the first half (= all of them for batches under 4 windows)
    int ks = LD_SCT_KS;                // K-splits per Schur tile of the batched reduction (ldso_ba_batch_create: 4 from 4 windows on)
    int halfChunks[2] = {0, 0}, halfReduce[2] = {0, 0};
    // Balanced launches (round 6): workgroup w of a batched k_linearize works through the blocks [wgStart[w], wgStart[w + 1]) of its launch's table, cut by
    // ldso_ba_batch_create so that every workgroup carries the same load.  wg[0] = the whole batch, wg[1] / wg[2] = the halves; empty: one block per workgroup
    std::vector<int32_t> wg[3];
    int32_t *d_wg = nullptr; size_t wgCap = 0;
    std::vector<int32_t> wgHost;       // what d_wg holds (kept: the copy is asynchronous)
    int nWG[3] = {0, 0, 0}; size_t wgOff[3] = {0, 0, 0};
    bool balanced = false;
    hipStream_t aux = nullptr;         // second stream: the two halves run half an iteration apart
    hipEvent_t ev0 = nullptr, ev1 = nullptr, evEnd = nullptr;
    BaDims Dmax;
    double *d_scalars = nullptr, *h_scalars = nullptr;      // [n][16]: every window's scalars after ldso_ba_batch_optimize (device block, pinned host copy)
    // The staging arena of the batched key-frame steps (batch_stage): one pinned arena and its device twin, grown on demand (grow_arena).  ldso_ba_batch_marginalize_points /
    // _frame: [n MargWin | the flags of all windows | pad to 8] go up in one copy, [the windows' (H_M | b_M) in doubles] come down in one; the batched activation
    // entries (act_select.hip): [tables | every window's inputs] up, [every window's results] down, the selection's scratch behind them on the device; the batched
    // window update and ldso_ba_batch_set_frames (ba_window.hip): [transfer table | tables | every window's delta or records] up, the images behind them on the device
    char *h_stage = nullptr, *d_stage = nullptr;
    size_t stageCap = 0;
    int selLdsLimit = -1, selLdsSet = 0; // dynamic LDS k_act_select_batch may have on this device (-1: not asked yet), and what its attribute was last raised to
    bool lost = false;                 // a ldso_ba_batch_update_windows failed behind its validation: members hold no window, batch_refresh refuses, ldso_ba_batch_destroy cleans up
};

// A call that replaces the window of a handle and fails half way (bad indices, allocation) must not leave the dimensions of the NEW window over the data of the
// old one: the handle then holds no window (every entry point that needs one says so).  ldso_ba_set_window, ldso_ba_update_window, ldso_ba_batch_update_windows.
struct WinGuard {
    ldso_ba *H; bool ok;
    ~WinGuard() { if (!ok) { H->D.P = 0; H->D.R = 0; H->R = 0; H->appliedValid = false; H->itemValid = false; } }
};

// The chunking of a batch as its policy decides it (ba_batch.hip: batch_chunk_policy; ldso_ba_batch_create and ldso_ba_batch_update_windows): balanced cuts per window
// and the workgroup tables of the three launches (whole batch | half A | half B), or regular chunks of CH points (0: the single-window chunking is the right one).
struct BatchCuts {
    bool balanced = false;
    int CH = 0;
    std::vector<std::vector<int32_t>> cuts;
    std::vector<int32_t> wg[3];
};

#pragma GCC visibility push(hidden)
// ba_batch.hip: the windows' descriptors as they are now into ldso_ba_batch::d_items; the batch's staging arena with room for `up` + `down` bytes
int batch_refresh(ldso_ba_batch *Bt);
int batch_stage(ldso_ba_batch *Bt, size_t up, size_t down);
int build_chunks(ldso_ba *H);          // ba_window.hip
int rechunk(ldso_ba *H);
// ba_batch.hip: the chunk policy of a batch from the windows' point counts and host runs (host logic; nothing is applied), how one window takes its share of it
// (`cut` = rechunk for a window with a resident applied state, a host-only plan inside ldso_ba_batch_update_windows; `always`: cut even where the policy leaves the
// single-window chunking alone), and the points per workgroup the batch reports once its windows are cut
void batch_chunk_policy(ldso_ba *const *handles, int n, BatchCuts &C);
template <class Cut> int batch_cut_window(ldso_ba *H, int i, const BatchCuts &C, bool always, Cut cut) {
    if (C.balanced) { H->chunkCuts = C.cuts[(size_t) i]; return cut(H); }
    if (C.CH > 0 && H->chunkPoints == 0 && H->chunkCuts.empty()) {
        H->chunkPoints = C.CH;
        const int r_ = cut(H);
        H->chunkPoints = 0;                                         // the policy stays "automatic": the next ldso_ba_set_window re-chunks for a single window
        return r_;
    }
    return always ? cut(H) : LDSO_OK;                               // CH == 0: the single-window chunking already is the right one
}
int batch_chunk_points(ldso_ba *const *handles, int n, const BatchCuts &C);
// ba_api.hip: the device records of ldso_ba_set_frames for the resident window of H (df: F entries)
void fill_dev_frames(const ldso_ba *H, const ldso_frame_t *fr, const ldso_calib_t *calib, DevFrame *df, DevCalib *dc);
// ba_optimize.hip: the launch helpers (with optional HIP-event timing) and what every caller of a launcher fills in the same way
void t_begin(ldso_ba *H, int which);
void t_end(ldso_ba *H);
int launch_linearize(ldso_ba *H, bool fix, int stepMode = 0, int itCheck = -1);
int launch_reduce(ldso_ba *H, const ResSet &S, bool atomicMode = false, double lambda = 0.0, int itCheck = -1);
int launch_gather(ldso_ba *H, const ResSet &S, double lambda, int mode, double *rbuf);
int launch_solve(ldso_ba *H, const ResSet &S, unsigned flags, int iteration = 0, double lambda = 0, int logIdx = -1, double *rout = nullptr, const double *rin = nullptr);
int launch_pstep(ldso_ba *H, const ResSet &S, int mode);
int refresh_item(ldso_ba *H);
// the descriptors of H's window as the kernels read them: `ks` K-splits per Schur tile; the residual sets as the handle numbers them, or (`relative`, the batch's
// order) set[0] = the applied one; linBlock0 / redBlock0 stay 0 (batch_refresh adds the offsets it computes)
void fill_item(BatchItem &it, const ldso_ba *H, int ks, bool relative, int outSlot);
int read_scalars(ldso_ba *H, double *sc);
SolveArgs solve_args(const ldso_ba *H, unsigned flags);
struct Damping { double lam, l1, il; };
Damping damping(const ldso_settings_t &St, double lambda);
GnInit gn_init(const ldso_ba *H, int itCheck);
int lend_acc(ldso_ba *H, double *buf);
#pragma GCC visibility pop
