// ba_optimize.hip — kernel sequencing of one window: the launch helpers, the step-wise LM entries, the GN iteration with its HIP-graph cache,
// ldso_ba_optimize, both marginalisations.  (Point activation, ldso_ba_activate_points, lies beside the other activation entries in act_select.hip.)
//
// Kernel sequences:
//   fast path (ldso_ba_optimize, ldso_ba_enqueue_gn):  k_reduce(atomic) -> k_gn_solve -> k_linearize(point step fused)   per iteration
//   multi-GPU fast path:  k_reduce(atomic into the caller's all-reduce buffer) -> k_gn_export -> [all-reduce] -> k_gn_solve -> k_linearize
//   step-wise entry points (solve_system, do_step, ...):  k_reduce -> k_gather -> k_solve(flags) -> k_point_step -> k_linearize
//   marginalisation:  k_linearize<MARG> -> k_reduce -> k_gather -> k_marg_update;  k_marg_frame
#include "ba_host.h"

// ---- launch helpers with optional HIP-event timing ----
void t_begin(ldso_ba *H, int which) {
    if (!H->profile) return;
    Timer t; t.which = which;
    hipEventCreate(&t.a); hipEventCreate(&t.b);
    hipEventRecord(t.a, H->stream);
    H->timers.push_back(t);
}
void t_end(ldso_ba *H) { if (H->profile) hipEventRecord(H->timers.back().b, H->stream); }

int launch_solve(ldso_ba *H, const ResSet &S, unsigned flags, int iteration, double lambda, int logIdx, double *rout, const double *rin) {
    SolveArgs A = solve_args(H, flags);
    A.iteration = iteration; A.lambda = lambda; A.logIdx = logIdx; A.reduceOut = rout; A.reduceIn = rin;
    t_begin(H, 2);
    CHK(ba_launch_solve(H->B, H->D, S, H->settings, A, H->stream));
    t_end(H);
    return LDSO_OK;
}
// the handle's BatchItem in device memory, uploaded when it changed (window, image slots, accumulator lent to an all-reduce buffer, prior)
void fill_item(BatchItem &it, const ldso_ba *H, int ks, bool relative, int outSlot) {
    const int applied = relative ? H->cur : 0;
    memset(&it, 0, sizeof(it));
    it.B = H->B; it.D = H->D; it.D.ks = ks; it.set[0] = H->sets[applied]; it.set[1] = H->sets[applied ^ 1]; it.cs = H->chunkStarts;
    it.hasPrior = H->hasPrior ? 1 : 0; it.GSP = H->GSP; it.outSlot = (int32_t) outSlot;
}
int refresh_item(ldso_ba *H) {
    BatchItem it;
    fill_item(it, H, H->D.ks, false, 0);
    if (H->itemValid && memcmp(&it, &H->itemShadow, sizeof(it)) == 0) return LDSO_OK;
    CHK(hipStreamSynchronize(H->stream));            // the pinned copy may still be in flight (rare: the descriptors change per key frame)
    memcpy(H->h_item, &it, sizeof(it));
    CHK(hipMemcpyAsync(H->d_item, H->h_item, sizeof(it), hipMemcpyHostToDevice, H->stream));
    H->itemShadow = it; H->itemValid = true;
    return LDSO_OK;
}

int launch_linearize(ldso_ba *H, bool fix, int stepMode, int itCheck) {
    t_begin(H, 0);
    const GnInit gi = gn_init(H, itCheck);
    if (!fix && !H->hasL && gi.enable == 1 && H->linHeadOk && H->B.dumpJ == nullptr) {          // (the Jacobian dump of ldso_ba_set_debug_dump: the argument-based kernel)
        // the plain linearisation (GN iterations) of one window, one or two slot groups: descriptor and chunk geometry in the kernel arguments (k_linearize_one;
        // until round 3 k_linearize_batch with one window for F <= 8 and the argument-based kernel for F > 8)
        CHK(ba_launch_linearize_one(H->B, H->D, H->sets[H->cur], H->sets[H->cur ^ 1], H->settings, stepMode, gi, H->linHead, H->stream));
    } else          // fixing pass, linearised residuals, shards of a multi-GPU window: the argument-based kernels
    CHK(ba_launch_linearize(H->B, H->D, H->sets[H->cur], H->sets[H->cur ^ 1], H->settings, H->hasL, fix, stepMode, gi, H->stream));
    t_end(H);
    if (H->profile) { t_begin(H, 4); t_end(H); }      // empty event pair: calibrates the event overhead (which = 4)
    return LDSO_OK;
}
int launch_reduce(ldso_ba *H, const ResSet &S, bool atomicMode, double lambda, int itCheck) {
    t_begin(H, 1);
    const Damping d = damping(H->settings, lambda);
    CHK(ba_launch_reduce(H->B, H->D, S, H->chunkStarts, H->hasL, H->GSP, atomicMode ? ((H->D.pBegin > 0) ? 2 : 1) : 0, H->hasPrior, H->settings.initialCalibHessian, d.l1, d.il, itCheck, H->stream));
    t_end(H);
    return LDSO_OK;
}
int launch_gather(ldso_ba *H, const ResSet &S, double lambda, int mode, double *rbuf) {
    t_begin(H, 1);
    CHK(ba_launch_gather(H->B, H->D, S, H->hasL, H->hasPrior, H->GSP, lambda, H->settings, mode, rbuf, H->stream));
    t_end(H);
    return LDSO_OK;
}
int launch_pstep(ldso_ba *H, const ResSet &S, int mode) {
    t_begin(H, 3);
    CHK(ba_launch_point_step(H->B, H->D, S, mode, H->stream));
    t_end(H);
    return LDSO_OK;
}

int read_scalars(ldso_ba *H, double *sc) {
    CHK(hipMemcpyAsync(sc, H->B.scalars, 16 * sizeof(double), hipMemcpyDeviceToHost, H->stream));
    CHK(hipStreamSynchronize(H->stream));
    return LDSO_OK;
}
SolveArgs solve_args(const ldso_ba *H, unsigned flags) {          // what every launch of this handle passes; the rest stays neutral (ba_solve.h) until a caller sets it
    SolveArgs A;
    A.flags = flags; A.hasL = H->hasL ? 1 : 0; A.hasPrior = H->hasPrior ? 1 : 0; A.GSP = H->GSP;
    return A;
}
// the damping of a reduction from the settings and the nominal lambda; `il` is rounded through float (the results are bit-reproducible only with this expression)
Damping damping(const ldso_settings_t &St, double lam) {
    if (St.solverMode & LDSO_SOLVER_USE_GN) lam = 0;
    if (St.solverMode & LDSO_SOLVER_FIX_LAMBDA) lam = 1e-5;
    return Damping{lam, 1 + lam, (double) (1.0f / (1 + lam))};
}
// what k_linearize / k_acc_init need to initialise B.acc.  enable = 2 on a shard that does not start at point 0; enqueue_iteration used to write 1
// here: both its callers have passed REQ_UNSHARDED (pBegin == 0), where the two forms are the same value.
GnInit gn_init(const ldso_ba *H, int itCheck) {
    GnInit gi; gi.enable = (H->D.pBegin > 0) ? 2 : 1; gi.hasPrior = H->hasPrior ? 1 : 0; gi.calibPrior = H->settings.initialCalibHessian; gi.itCheck = itCheck;
    return gi;
}
// the accumulator moves to `buf` (a caller's all-reduce buffer, or back to the handle's own): re-point it and give it what the last k_linearize put into the old one
int lend_acc(ldso_ba *H, double *buf) {
    if (H->B.acc == buf) return LDSO_OK;
    H->B.acc = buf;
    CHK(ba_launch_acc_init(H->B, H->D, gn_init(H, -1), H->stream));
    return LDSO_OK;
}

extern "C" {

// ---------------------------------------------------------------------------------------------------------
// the optimisation slice
// ---------------------------------------------------------------------------------------------------------
// Average duration of the dominant kernel for bench.py's roofline: `reps` back-to-back launches of k_linearize on the applied
// state (read set -> scratch set, no point step, nothing applied: idempotent) between ONE pair of HIP events on the handle's
// stream, so the event overhead is amortised over the launches; includes the ~1.5 us dependent-launch boundary per launch.
int ldso_ba_time_linearize(ldso_ba_t *H, int reps, double *avg_us) {
    REQ(H && H->D.P > 0 && reps > 0 && avg_us, "bad arguments");
    CHK(hipSetDevice(H->device));
    REQ(!H->pendingApply, "ldso_ba_time_linearize: a linearizeAll result is pending");
    const bool prof = H->profile;
    H->profile = false;
    const int rc = time_launches(H->stream, reps, avg_us, [H] { return launch_linearize(H, false, 0); });
    H->profile = prof;
    return rc;
}

int ldso_ba_collect_active(ldso_ba_t *H) {
    REQ(H && H->D.P > 0, "no window");
    CHK(hipSetDevice(H->device));
    H->pendingApply = false;
    return launch_solve(H, H->sets[H->cur], SK_COLLECT);
}

int ldso_ba_linearize_all(ldso_ba_t *H, int fix, double *energy_out) {
    REQ(H && H->D.P > 0, "no window");
    CHK(hipSetDevice(H->device));
    RUN(launch_linearize(H, fix != 0));
    RUN(launch_solve(H, H->sets[H->cur ^ 1], SK_POST | SK_THRESH));
    H->pendingApply = true;
    if (fix) { H->cur ^= 1; H->pendingApply = false; H->appliedValid = true; }     // applyRes happens inside the reductor when fixing
    double sc[16];
    RUN(read_scalars(H, sc));
    if (energy_out) *energy_out = sc[0];
    if (!std::isfinite(sc[0])) return LDSO_E_NONFINITE;
    return LDSO_OK;
}

int ldso_ba_apply_res(ldso_ba_t *H) {
    REQ(H, "null handle");
    if (H->pendingApply) { H->cur ^= 1; H->pendingApply = false; H->appliedValid = true; }
    return LDSO_OK;
}

int ldso_ba_backup_state(ldso_ba_t *H) {
    REQ(H && H->D.P > 0, "no window");
    CHK(hipSetDevice(H->device));
    RUN(launch_solve(H, H->sets[H->cur], SK_BACKUP));
    RUN(launch_pstep(H, H->sets[H->cur], PS_BACKUP));
    return LDSO_OK;
}

int ldso_ba_solve_system(ldso_ba_t *H, int iteration, double lambda) {
    REQ(H && H->D.P > 0, "no window");
    REQ_UNSHARDED("ldso_ba_solve_system");
    CHK(hipSetDevice(H->device));
    const ResSet &S = H->sets[H->cur];
    RUN(launch_reduce(H, S));
    RUN(launch_gather(H, S, lambda, 0, nullptr));
    RUN(launch_solve(H, S, SK_SOLVE, iteration, lambda));
    RUN(launch_pstep(H, S, PS_RESUB));
    double sc[16];
    RUN(read_scalars(H, sc));
    if (sc[4] != 0.0) return LDSO_E_NONFINITE;
    return LDSO_OK;
}

int ldso_ba_do_step(ldso_ba_t *H, int *canbreak) {
    REQ(H && H->D.P > 0, "no window");
    CHK(hipSetDevice(H->device));
    RUN(launch_solve(H, H->sets[H->cur], SK_STEP | SK_PRECALC));
    RUN(launch_pstep(H, H->sets[H->cur], PS_STEP));
    double sc[16];
    RUN(read_scalars(H, sc));
    if (canbreak) *canbreak = sc[3] != 0.0;
    return LDSO_OK;
}

int ldso_ba_load_state_backup(ldso_ba_t *H) {
    REQ(H && H->D.P > 0, "no window");
    CHK(hipSetDevice(H->device));
    RUN(launch_solve(H, H->sets[H->cur], SK_LOADBK | SK_PRECALC));
    RUN(launch_pstep(H, H->sets[H->cur], PS_LOAD));
    H->pendingApply = false;
    return LDSO_OK;
}

// one GN iteration = solveSystem + doStepFromBackup + linearizeAll(false) + applyRes: 4 launches (k_reduce, k_gather,
// k_gn_solve, k_linearize with the point step fused in), no host sync
static int enqueue_iteration(ldso_ba *H, int iteration, double lambda, int logIdx, int itCheck = -1, int lastIt = -1) {
    const ResSet &S = H->sets[H->cur];
    RUN(lend_acc(H, H->ownAcc));      // the accumulator was lent to an all-reduce buffer: take it back (and re-initialise)
    SolveArgs A = solve_args(H, 0);
    A.iteration = iteration; A.lambda = lambda; A.logIdx = logIdx; A.itCheck = itCheck; A.hostStop = (itCheck >= 0) ? H->d_stop : nullptr; A.lastIt = lastIt;
    if (reduce_grid(H->D.F, H->hasL, H->D.ks, H->GSP).total + LD_FUSED_CTL <= H->numCU && !H->noFusedLaunch) {
        // k_reduce (fp64 atomics straight into B.acc, no k_gather on this path) and the control step in ONE launch: the control
        // workgroup waits on a device counter for the reduce workgroups (k_reduce_solve, ba_solve.hip).  Only while every workgroup
        // of the launch gets its own CU (F <= 8; from F = 9 the Schur part alone has 180 workgroups): the fused kernel's LDS footprint allows one workgroup per CU.
        A.waitCtr = H->d_waitCtr;
        const Damping d = damping(H->settings, lambda);
        t_begin(H, 2);
        CHK(ba_launch_reduce_solve(H->B, H->D, S, H->settings, A, H->chunkStarts, (H->D.pBegin > 0) ? 2 : 1, H->settings.initialCalibHessian, d.l1, d.il, H->stream));
        t_end(H);
    } else {
        RUN(launch_reduce(H, S, true, lambda, itCheck));
        t_begin(H, 2);
        CHK(ba_launch_gn_solve(H->B, H->D, S, H->settings, A, H->stream));
        t_end(H);
    }
    RUN(launch_linearize(H, false, 1, itCheck));
    H->cur ^= 1; H->appliedValid = true;      // forceAcceptStep: applyRes
    return LDSO_OK;
}

static unsigned long long fnv1a(unsigned long long h, const void *p, size_t n) {
    const unsigned char *b = (const unsigned char *) p;
    for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 1099511628211ull; }
    return h;
}
// everything the launches of `iters` forced iterations take as arguments, as bytes (the cache key) ...
static void gn_key(const ldso_ba *H, int first_iteration, int iters, std::vector<unsigned char> &key) {
    key.clear();
    auto put = [&key](const void *p, size_t n) { const unsigned char *b = (const unsigned char *) p; key.insert(key.end(), b, b + n); };
    put(&H->B, sizeof(H->B)); put(&H->D, sizeof(H->D)); put(H->sets, sizeof(H->sets)); put(&H->settings, sizeof(H->settings));
    put(&H->chunkStarts, sizeof(H->chunkStarts)); put(&H->linHead, sizeof(H->linHead));
    const long long misc[12] = {first_iteration, iters, H->cur, H->hasL, H->hasPrior, H->GSP, H->linHeadOk, H->noFusedLaunch, H->numCU, (long long) (size_t) H->stream, (long long) (size_t) H->ownAcc,
                                (long long) (size_t) H->d_waitCtr};
    put(misc, sizeof(misc));
}
// ... and their 64-bit hash (pre-selection only: a hit is confirmed on the bytes)
static unsigned long long gn_signature(const std::vector<unsigned char> &key) { return fnv1a(1469598103934665603ull, key.data(), key.size()); }
static int enqueue_gn_plain(ldso_ba *H, int first_iteration, int iters) {
    CHK(hipMemsetAsync(H->d_waitCtr, 0, LD_ARRIVE_BYTES, H->stream));      // an aborted launch must not leave an arrival word armed
    for (int i = 0; i < iters; i++) RUN(enqueue_iteration(H, first_iteration + i, 1e-1, -1));
    return LDSO_OK;
}
// The iterations are 2-3 dependent launches each, the host runs far ahead of the device, and what is left to remove on the device side is the per-packet work of the
// command processor: the same sequence captured ONCE into a HIP graph and replayed is 35.55 against 36.04 us per iteration at C3 (scripts/r5/graph_gn.py).  The
// graph is keyed by a hash of every launch argument (gn_signature): anything that changes what the kernels are handed - a new window, other settings, a prior,
// another stream, another iteration index (the orthogonalisation starts at iteration 2) - captures anew; profiling runs (per-kernel events) and callers that are
// capturing themselves take the plain path.  LDSO_GN_GRAPHS=0 turns it off.
int ldso_ba_enqueue_gn(ldso_ba_t *H, int first_iteration, int iters) {
    REQ(H && H->D.P > 0 && iters >= 0, "bad arguments");
    REQ_UNSHARDED("ldso_ba_enqueue_gn");
    CHK(hipSetDevice(H->device));
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (!H->gnUseGraphs || H->profile || iters < 2 || H->B.acc != H->ownAcc || hipStreamIsCapturing(H->stream, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone)
        return enqueue_gn_plain(H, first_iteration, iters);
    std::vector<unsigned char> &key = H->gnKeyScratch;
    gn_key(H, first_iteration, iters, key);
    const unsigned long long sig = gn_signature(key);
    for (ldso_ba::GnGraph &g : H->gnGraphs)
        if (g.sig == sig && g.key == key) {
            CHK(hipGraphLaunch(g.exec, H->stream));
            if (iters & 1) H->cur ^= 1;          // what the captured enqueue did to the handle's host state: the sets swap once per iteration
            H->appliedValid = true;
            return LDSO_OK;
        }
    // capture; the handle's host state advances as in a plain enqueue, the device work happens at the launch below
    const int cur0 = H->cur;
    hipGraph_t graph = nullptr;
    if (hipStreamBeginCapture(H->stream, hipStreamCaptureModeThreadLocal) != hipSuccess) { (void) hipGetLastError(); return enqueue_gn_plain(H, first_iteration, iters); }
    const int rc = enqueue_gn_plain(H, first_iteration, iters);
    const hipError_t ec = hipStreamEndCapture(H->stream, &graph);
    hipGraphExec_t exec = nullptr;
    if (rc != LDSO_OK || ec != hipSuccess || graph == nullptr || hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) != hipSuccess) {
        (void) hipGetLastError();
        if (graph) hipGraphDestroy(graph);
        H->cur = cur0;                            // nothing ran: enqueue for real
        H->gnUseGraphs = false;                   // this runtime / stream does not capture the sequence: do not try again
        return enqueue_gn_plain(H, first_iteration, iters);
    }
    if (H->gnGraphs.size() >= 4) { hipGraphExecDestroy(H->gnGraphs.front().exec); hipGraphDestroy(H->gnGraphs.front().graph); H->gnGraphs.erase(H->gnGraphs.begin()); }
    H->gnGraphs.push_back(ldso_ba::GnGraph{sig, key, exec, graph});
    CHK(hipGraphLaunch(exec, H->stream));
    return LDSO_OK;
}

// EnergyFunctional::calcMEnergyF / calcLEnergyF_MT (EnergyFunctional.cc:353-378, 627-682) at the current state: the two extra
// terms of the LM accept test (FullSystem.cc:805-826).  (With setting_forceAceptStep the reference skips them, FullSystem.cc:1694-1704.)
int ldso_ba_calc_lm_energies(ldso_ba_t *H, double *energy_M, double *energy_L) {
    REQ(H && H->D.P > 0, "no window");
    CHK(hipSetDevice(H->device));
    CHK(ba_launch_lm_energies(H->B, H->D, H->sets[H->cur], H->settings.initialCalibHessian, H->hasPrior, H->stream));
    double sc[16];
    RUN(read_scalars(H, sc));
    if (energy_M) *energy_M = sc[12];
    if (energy_L) *energy_L = sc[13];
    return LDSO_OK;
}

// FullSystem::optimize with setting_forceAceptStep = false (FullSystem.cc:777-831): every iteration is accepted or rejected on
// E_P + E_L + E_M; a rejected step restores the backup (loadSateBackup), re-linearises and multiplies lambda by 100.  One host
// round trip per stage - this is not the default schedule of the reference (Setting.cc:73) and not the timed path.
static int optimize_lm(ldso_ba *H, int mnumOptIts, int force_all, float *rmse_out, int *iters_out) {
    mnumOptIts = optimize_iteration_cap(H->D.F, mnumOptIts, force_all);
    REQ(mnumOptIts + 2 < 64, "too many iterations");
    std::vector<double> elog;
    RUN(ldso_ba_collect_active(H));
    double lastE = 0, lastL = 0, lastM = 0;
    RUN(ldso_ba_linearize_all(H, 0, &lastE));
    RUN(ldso_ba_calc_lm_energies(H, &lastM, &lastL));
    elog.push_back(lastE);
    RUN(ldso_ba_apply_res(H));
    double lambda = 1e-1;
    int done = 0;
    for (int it = 0; it < mnumOptIts; it++) {
        RUN(ldso_ba_backup_state(H));
        RUN(ldso_ba_solve_system(H, it, lambda));
        int canbreak = 0;
        RUN(ldso_ba_do_step(H, &canbreak));
        double newE = 0, newL = 0, newM = 0;
        RUN(ldso_ba_linearize_all(H, 0, &newE));
        RUN(ldso_ba_calc_lm_energies(H, &newM, &newL));
        elog.push_back(newE);
        done = it + 1;
        if (newE + newL + newM < lastE + lastL + lastM) {
            RUN(ldso_ba_apply_res(H));
            lastE = newE; lastL = newL; lastM = newM;
            lambda *= 0.25;
        } else {
            RUN(ldso_ba_load_state_backup(H));
            RUN(ldso_ba_linearize_all(H, 0, &lastE));
            H->pendingApply = false;                 // the re-linearisation at the restored state is not applied (FullSystem.cc:821-826)
            RUN(ldso_ba_calc_lm_energies(H, &lastM, &lastL));
            lambda *= 1e2;
        }
        if (canbreak && it >= H->settings.minOptIterations && !force_all) break;
    }
    RUN(launch_solve(H, H->sets[H->cur], SK_REANCHOR | SK_ADJ | SK_NONULLSPACE | SK_PRECALC));
    double Efix = 0;
    RUN(ldso_ba_linearize_all(H, 1, &Efix));
    elog.push_back(Efix);
    CHK(hipMemsetAsync(H->B.energyLog, 0, 64 * 8, H->stream));
    CHK(hipMemcpyAsync(H->B.energyLog, elog.data(), elog.size() * sizeof(double), hipMemcpyHostToDevice, H->stream));
    double sc[16];
    RUN(read_scalars(H, sc));
    H->lastIterations = (int) elog.size() - 2;
    if (iters_out) *iters_out = done;
    if (rmse_out) *rmse_out = sqrtf((float) (sc[0] / (8 * sc[9])));
    if (!std::isfinite(sc[0]) || sc[4] != 0.0) return LDSO_E_NONFINITE;
    return LDSO_OK;
}

int ldso_ba_optimize(ldso_ba_t *H, int mnumOptIts, int force_all, float *rmse_out, int *iters_out) {
    REQ(H && H->D.P > 0, "no window");
    REQ_UNSHARDED("ldso_ba_optimize");
    CHK(hipSetDevice(H->device));
    CHK(hipMemsetAsync(H->d_waitCtr, 0, LD_ARRIVE_BYTES, H->stream));      // an aborted launch must not leave an arrival word armed
    if (!H->settings.forceAcceptStep) return optimize_lm(H, mnumOptIts, force_all, rmse_out, iters_out);
    const int F = H->D.F;
    if (F < 2) { if (rmse_out) *rmse_out = 0; return LDSO_OK; }
    mnumOptIts = optimize_iteration_cap(F, mnumOptIts, force_all);
    REQ(mnumOptIts + 2 < 64, "too many iterations");
    CHK(hipMemsetAsync(H->B.energyLog, 0, 64 * 8, H->stream));
    H->pendingApply = false;
    RUN(launch_linearize(H, false, 2));            // stepMode bit 1: resetOOB of the optimize() preamble fused into the first linearizeAll
    H->cur ^= 1; H->appliedValid = true;           // applyRes
    int done = 0;
    double lambda = 1e-1;
    {   // no iteration has asked to stop yet
        CHK(hipMemcpyAsync(H->B.scalars + LD_SC_STOP, &H->neverStop, sizeof(double), hipMemcpyHostToDevice, H->stream));
    }
    volatile int *stopWord = H->h_stop;
    *stopWord = -1;
    for (int it = 0; it < mnumOptIts; it++) {
        // un-forced: the device decides (canbreak && it >= minOptIterations, FullSystem.cc:829); later iterations become no-ops
        RUN(enqueue_iteration(H, it, lambda, it, force_all ? -1 : it, mnumOptIts - 1));    // POST/THRESH/LOG of the previous linearize ride along
        lambda *= 0.25;
    }
    done = mnumOptIts;
    if (!force_all && mnumOptIts > 0) {
        // The control step of the iteration that ends the loop writes its index into a host-mapped word: the host learns `done` while the
        // GPU is still busy and enqueues the tail right behind the iterations that turned into no-ops (no stream synchronisation, which
        // cost a 40 us bubble).  The stream is polled as well so that a failed launch cannot hang the caller.
        int spins = 0;
        while (*stopWord < 0) {
            if ((++spins & 0x3FF) == 0) {
                const hipError_t q = hipStreamQuery(H->stream);
                if (q == hipSuccess) break;                         // everything ran: the word is final (or the loop never reported)
                if (q != hipErrorNotReady) CHK(q);
            }
        }
        int stopIt = *stopWord;
        if (stopIt < 0) {                                           // not reported (cannot happen on a healthy run): fall back to the device scalar
            double sc[16];
            RUN(read_scalars(H, sc));
            stopIt = (sc[LD_SC_STOP] < (double) mnumOptIts) ? (int) sc[LD_SC_STOP] : mnumOptIts - 1;
        }
        done = stopIt + 1;
        if ((mnumOptIts - done) & 1) H->cur ^= 1;   // the skipped iterations never wrote / applied a residual set
    }
    // tail: statistics of the last linearize, re-anchor the newest frame, adjoints, precalc, linearizeAll(true)
    RUN(launch_solve(H, H->sets[H->cur], SK_POST | SK_THRESH | SK_LOG | SK_REANCHOR | SK_ADJ | SK_NONULLSPACE | SK_PRECALC, 0, 0, done));
    RUN(launch_linearize(H, true));
    H->cur ^= 1;
    RUN(launch_solve(H, H->sets[H->cur], SK_POST | SK_THRESH | SK_LOG, 0, 0, done + 1));
    double sc[16];
    RUN(read_scalars(H, sc));
    H->lastIterations = done;
    if (iters_out) *iters_out = done;
    if (rmse_out) *rmse_out = sqrtf((float) (sc[0] / (8 * sc[9])));
    if (!std::isfinite(sc[0]) || sc[4] != 0.0) return LDSO_E_NONFINITE;
    return LDSO_OK;
}

// EnergyFunctional::marginalizePointsF (EnergyFunctional.cc:165-222) for the points with flags[p] != 0, including the
// re-linearise + fixLinearizationF pass FullSystem::flagPointsForRemoval ran on them (FullSystem.cc:1241-1250).
// The applied state of the window is not changed; the caller removes the points (next ldso_ba_set_window).
int ldso_ba_marginalize_points(ldso_ba_t *H, const int32_t *flags, double *HM_out, double *bM_out) {
    REQ(H && flags && H->D.P > 0, "ldso_ba_marginalize_points: bad arguments");
    CHK(hipSetDevice(H->device));
    REQ(!H->pendingApply, "ldso_ba_marginalize_points: a linearizeAll result is pending (apply or discard it first)");
    REQ(H->D.pBegin == 0 && H->D.pEnd == H->D.P, "ldso_ba_marginalize_points: not available on a sharded handle");
    const size_t n = H->D.n;
    if (!H->hasPrior) { CHK(hipMemsetAsync(H->B.HM, 0, n * n * 8, H->stream)); CHK(hipMemsetAsync(H->B.bM, 0, n * 8, H->stream)); }
    CHK(hipMemcpyAsync(H->d_margFlags, flags, (size_t) H->D.P * 4, hipMemcpyHostToDevice, H->stream));
    const ResSet &scratch = H->sets[H->cur ^ 1];
    CHK(ba_launch_linearize_marg(H->B, H->D, H->sets[H->cur], scratch, H->settings, H->d_margFlags, H->stream));
    CHK(ba_launch_reduce(H->B, H->D, scratch, H->chunkStarts, /*hasL*/ false, H->GSP, 0, false, 0.0f, 1.0, 1.0, -1, H->stream));
    CHK(ba_launch_gather(H->B, H->D, scratch, /*hasL*/ false, /*hasPrior*/ false, H->GSP, 0.0, H->settings, 0, nullptr, H->stream));
    CHK(ba_launch_marg_update(H->B, H->D, (double) H->settings.margWeightFac, H->stream));
    H->hasPrior = true;
    if (HM_out) CHK(hipMemcpyAsync(HM_out, H->B.HM, n * n * 8, hipMemcpyDeviceToHost, H->stream));
    if (bM_out) CHK(hipMemcpyAsync(bM_out, H->B.bM, n * 8, hipMemcpyDeviceToHost, H->stream));
    CHK(hipStreamSynchronize(H->stream));
    return LDSO_OK;
}

// EnergyFunctional::marginalizeFrame (EnergyFunctional.cc:72-151) applied to the device prior: returns the prior of the
// window without frame `frame_idx` ((8(F-1)+4)^2 row-major, 8(F-1)+4).  The handle keeps its window; the caller rebuilds
// it without the frame (ldso_ba_set_window / ldso_ba_set_prior with the returned matrices).
int ldso_ba_marginalize_frame(ldso_ba_t *H, int frame_idx, double *HM_out, double *bM_out) {
    REQ(H && HM_out && bM_out && H->D.F >= 2 && frame_idx >= 0 && frame_idx < H->D.F, "ldso_ba_marginalize_frame: bad arguments");
    CHK(hipSetDevice(H->device));
    const size_t n = H->D.n, nd = n - 8;
    if (!H->hasPrior) { CHK(hipMemsetAsync(H->B.HM, 0, n * n * 8, H->stream)); CHK(hipMemsetAsync(H->B.bM, 0, n * 8, H->stream)); }
    // scratch: B.sys holds 4 (n^2 + n) doubles: work = first n^2 + n, output after it
    double *work = H->B.sys, *oH = work + n * n + n, *ob = oH + nd * nd;
    CHK(ba_launch_marg_frame(H->B, H->D, frame_idx, work, oH, ob, H->stream));
    CHK(hipMemcpyAsync(HM_out, oH, nd * nd * 8, hipMemcpyDeviceToHost, H->stream));
    CHK(hipMemcpyAsync(bM_out, ob, nd * 8, hipMemcpyDeviceToHost, H->stream));
    CHK(hipStreamSynchronize(H->stream));
    return LDSO_OK;
}
}  // extern "C"
