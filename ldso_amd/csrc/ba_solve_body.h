// ba_solve_body.h — the bodies of the control kernels (gfx950): what composes the statistics (ba_stats.h), the frame records (ba_frames_dev.h) and the solver
// (ba_ldlt.h) into the control step, shared by the single-window kernels (ba_solve.hip) and the batched ones (ba_solve_batch.hip).
//   gn_solve_body  the forced-accept fast path: role 0 solve_core (+ backupState, doStepFromBackup, canbreak, setPrecalcValues) on an LDS mirror of
//                  the frames; role 1 statistics of the previous linearizeAll (energy sums, setNewFrameEnergyTH, energy log).
//   solve_body     flag-selected pieces for the step-wise C entry points (LM rejection, debugging, old multi-GPU path):
//     SK_POST     FullSystem::linearizeAll tail: energy sum (FullSystem.cc:1762-1793);  SK_THRESH: setNewFrameEnergyTH
//     SK_ADJ      EnergyFunctional::setAdjointsF (EnergyFunctional.cc:431-489) + gauge nullspace basis
//                 for orthogonalize (EnergyFunctional.cc:685-717, FullSystem.cc:1711-1760)
//     SK_SOLVE    EnergyFunctional::solveSystemF after the assembly (EnergyFunctional.cc:293-351, default solver mode) and the
//                 frame part of resubstituteF_MT (:491-516); HFinal / bFinal come from k_gather (ba_reduce.hip)
//     SK_BACKUP   FullSystem::backupState (FullSystem.cc:1625-1673)
//     SK_STEP     FullSystem::doStepFromBackup frame/calib part + canbreak (FullSystem.cc:1546-1623)
//     SK_LOADBK   FullSystem::loadSateBackup frame/calib part (FullSystem.cc:1675-1692)
//     SK_PRECALC  FullSystem::setPrecalcValues: FrameFramePrecalc::Set for F^2 pairs + setDeltaF
//                 (FullSystem.cc:1423-1431, FrameFramePrecalc.cc:6-35, EnergyFunctional.cc:403-429)
//     SK_REANCHOR end of optimize(): newest frame setEvalPT(PRE_worldToCam, newStateZero) (FullSystem.cc:833-841)
//     SK_COLLECT / SK_LOG / SK_EXPORT / SK_FROMREDUCED: optimize() preamble, energy log, multi-GPU scalar exchange
#pragma once
#include <stddef.h>          // offsetof
#include <hip/hip_runtime.h>
#include "ba_dev.h"
#include "ba_solve.h"          // SolveArgs, SK_*
#include "lie_dev.h"
#include "ba_stats.h"          // NT
#include "ba_frames_dev.h"
#include "ba_ldlt.h"

// ---------------------------------------------------------------------------------------------------------
// The control kernel's body, shared by k_solve (one window: everything in the kernel arguments) and k_solve_batch (the tail of a batched optimize(): the
// descriptors live in device memory).  nRoles == 2: the statistics (role 1) run next to the control part (role 0), one workgroup each.
static __device__ __forceinline__ void solve_body(const BaPtrs &B, const BaDims &D, const ResSet &S, const ldso_settings_t &St, const SolveArgs &A, const int nRoles, const int role) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int tid = threadIdx.x, F = D.F, n = D.n;
    const SolveLds lds = solve_lds(n);
    double *const top = sm + core_lds_end(LD_SOLVE_NB(n), n), *sW = top + lds.sW;
    // two workgroups (solve_roles): the statistics of the last linearizeAll (POST / THRESH / LOG) run next to the control part;
    // they touch disjoint data (frameEnergyTH is only written by the statistics and only read by k_linearize)
    unsigned fl = A.flags;
    if (nRoles == 2) fl &= (role == 1) ? (unsigned) SK_STATS : ~(unsigned) SK_STATS;

    if (fl & SK_COLLECT) {
        // FullSystem::optimize preamble: resetOOB on every non-linearised residual (FullSystem.cc:744-748)
        for (int i = tid; i < D.P * D.FS; i += NT)
            if (B.rtab[i].rflat >= 0 && !B.rtab[i].rlin) { S.slot[i].e[LD_SM_STATE].m.i = 0; S.slot[i].e[LD_SM_ENERGY].m.f = 0.0f; }
        __syncthreads();
    }
    if (fl & SK_POST) post_sums(B, D, S, sW);

    if (fl & SK_REANCHOR) {
        // FrameHessian::setEvalPT + setStateZero of the newest frame (FrameHessian.cc:12-42).  The numeric nullspaces are 14 independent
        // exp / mul / mul / log chains (6 directions x +-eps, scale up / down): one lane each - the same operations as ld::frame_nullspaces
        // (bit-identical), a fourteenth of its latency (it was 30 us of the 39 us tail on one lane)
        DevFrame &f = B.frames[F - 1];
        double *sLp = sW;                  // [14][6] logs
        double *sEv = top + lds.sEv;             // the new evalPT
        if (tid < 12) sEv[tid] = f.PRE_w2c[tid];
        __syncthreads();
        if (tid < 14) {
            double Ti[12], Am[12], Bm[12], lg[6];
            ld::se3_inv(sEv, Ti);
            if (tid < 12) {
                double eps[6] = {0, 0, 0, 0, 0, 0}, E[12];
                const double e_ = (tid & 1) ? -1e-3 : 1e-3;
#pragma unroll
                for (int q = 0; q < 6; q++) eps[q] = (q == (tid >> 1)) ? e_ : 0.0;
                ld::se3_exp(eps, E); ld::se3_mul(sEv, E, Am); ld::se3_mul(Am, Ti, Bm); ld::se3_log(Bm, lg);
            } else {
                double Tp[12];
                for (int i = 0; i < 12; i++) Tp[i] = sEv[i];
                if (tid == 12) { for (int i = 0; i < 3; i++) Tp[i * 4 + 3] *= 1.00001; } else { for (int i = 0; i < 3; i++) Tp[i * 4 + 3] /= 1.00001; }
                ld::se3_mul(Tp, Ti, Am); ld::se3_log(Am, lg);
            }
#pragma unroll
            for (int r = 0; r < 6; r++) sLp[tid * 6 + r] = lg[r];
        }
        __syncthreads();
        if (tid < 36) { const int r = tid / 6, i = tid % 6; f.ns_pose[r * 6 + i] = (sLp[(2 * i) * 6 + r] - sLp[(2 * i + 1) * 6 + r]) / 2e-3; }
        else if (tid < 42) { const int r = tid - 36; f.ns_scale[r] = (sLp[12 * 6 + r] - sLp[13 * 6 + r]) / 2e-3; }
        else if (tid < 54) f.evalPT[tid - 42] = sEv[tid - 42];
        else if (tid == 54) {
            const double a = f.state[6], b = f.state[7];
            for (int i = 0; i < 10; i++) { f.state[i] = 0; f.state_zero[i] = 0; }
            f.state[6] = a; f.state[7] = b; f.state_zero[6] = a; f.state_zero[7] = b;
            for (int i = 0; i < 8; i++) f.ns_affine[i] = 0;
            f.ns_affine[0] = 1;
            f.ns_affine[3] = (double) (expf((float) (a * 10.0)) * f.ab_exposure);
        }
        __syncthreads();
    }
    if (fl & SK_ADJ) set_adjoints(B, D, St, sW, !(fl & SK_NONULLSPACE), sm);

    if (fl & SK_EXPORT) {
        // multi-GPU: rank-local scalar sums ride in the all-reduce buffer
        double na = 0, nl = 0;
        for (int c = tid; c < D.nChunks; c += NT) { na += S.chunkCnt[c * 2]; nl += S.chunkCnt[c * 2 + 1]; }
        na = wave_sum(na); nl = wave_sum(nl);
        if ((tid & 63) == 0) { sW[tid >> 6] = na; sW[4 + (tid >> 6)] = nl; }
        __syncthreads();
        if (tid == 0) { double *sc = A.reduceOut + 3 * (n * n + n); sc[0] = B.scalars[0]; sc[1] = B.scalars[1]; sc[2] = B.scalars[2]; sc[3] = B.scalars[6]; sc[4] = B.scalars[7];
                        sc[5] = sW[0] + sW[1] + sW[2] + sW[3]; sc[6] = sW[4] + sW[5] + sW[6] + sW[7]; sc[7] = 0; }
        __syncthreads();
    }
    if (fl & SK_FROMREDUCED) {
        const double *sc = A.reduceIn + 3 * (n * n + n);
        if (tid == 0) { B.scalars[0] = sc[0]; B.scalars[1] = sc[1]; B.scalars[2] = sc[2]; B.scalars[6] = sc[3]; B.scalars[7] = sc[4]; B.scalars[9] = sc[5]; B.scalars[10] = sc[6]; }
        __syncthreads();
    }
    if (fl & SK_THRESH) post_thresh(B, D, S, St, (fl & SK_FROMREDUCED) ? (A.reduceIn + 3 * (n * n + n) + 8) : nullptr, (int *) sm);
    if (fl & SK_LOG) { if (tid == 0 && A.logIdx >= 0 && A.logIdx < 64) B.energyLog[A.logIdx] = B.scalars[0]; __syncthreads(); }

    if (fl & SK_SOLVE) {
        // HFinal / bFinal were assembled by k_gather (ba_reduce.hip)
        if (!(fl & SK_FROMREDUCED)) res_counts(B, D, S, sW);
        SolveIO io;
        io.fr = B.frames; io.cal = B.calib; io.adH = B.adHostF; io.adT = B.adTargetF; io.adPitch = 64; io.ldsAd = nullptr; io.sRed = sW; io.sumNID = 0; io.lambda = A.lambda; io.hasPrior = A.hasPrior; io.redScalars = nullptr;
        solve_core_dispatch<false>(B, D, S, St, A.iteration, sm, io);
    }
    if (fl & SK_BACKUP) frames_backup(B.frames, B.calib, F);
    if (fl & SK_STEP) frames_step(B, St, B.frames, B.calib, F, (float) B.scalars[6] / (float) B.scalars[7], sW);
    if (fl & SK_LOADBK) {
        if (tid < F) for (int i = 0; i < 10; i++) B.frames[tid].state[i] = B.frames[tid].state_backup[i];
        if (tid == 0) for (int i = 0; i < 4; i++) B.calib->value[i] = B.calib->value_backup[i];
        __syncthreads();
    }
    if (fl & SK_PRECALC) set_precalc(B, D, B.frames, B.calib, B.adHostF, B.adTargetF);
}

// ---------------------------------------------------------------------------------------------------------
// gn_tail - everything of the control step behind the back substitution: x, xAd, backupState + doStepFromBackup (frames, calibration), canbreak,
// setPrecalcValues (frame poses, pair records, adHTdeltaF).  One workgroup on the critical path of the iteration, so it is laid out by WAVEFRONT around the
// one chain that is long:  new states -> frame poses (a lane per frame, a few hundred dependent fp64 instructions) -> pair records (a lane per pair).
// Wave 0 runs that chain and nothing else: it forms the new states in registers, touches no memory another wave writes, and (windows of up to 8 frames:
// all pairs fit its lanes) needs no workgroup barrier between the poses and the pair records.  Waves 1..3 do the wide work beside it: float copies of x
// and of the new deltas (private to each wave), per item (pair, column) xAd AND adHTdeltaF in one pass over the adjoint columns (the same loads; waves 1
// and 2), the calibration (its step, the derived floats, K^-1: one lane, handed to wave 0 through a flag), the remainder of the items and canbreak (wave 3),
// the frames' step / state_backup (wave 2).  The OLD states stay in the working copies - every
// wave reads them - and the new ones reach memory through delta_prior (see the end).  One workgroup barrier, at the end.
// Device stamps, C3, us after the back substitution - before: outputs 1.2, poses 2.0 - 2.8, pair records 1.0, adHTdeltaF 0.85 = 5.6 (the poses stored through
// LDS between dependent products, canbreak walked four divergent branches with LDS round trips inside, and every wave walked every phase); now: see DESIGN 5.
// ---------------------------------------------------------------------------------------------------------
static_assert(NT == 256, "gn_tail is laid out for exactly four wavefronts: wave 0 waits for a flag that wave 3 sets");
static_assert(LD_TAIL_KI + 9 <= LD_TAIL_FLAG && (LD_TAIL_FLAG + 1) * 4 <= (LD_SW_DOUBLES - LD_SW_RED) * 8, "gn_tail's floats must fit the scratch behind io.sRed");
static __device__ __forceinline__ void gn_tail(const BaPtrs &B, const BaDims &D, DevFrame *fr, DevCalib *cal, const SolveIO &io, const ldso_settings_t &St, float *cbF,
                                               int cbIter, int *hostStop, int lastIt) {
    const int tid = threadIdx.x, F = D.F, n = D.n, wave = tid >> 6, lane = tid & 63;
    constexpr int W2 = 128;          // waves 1 and 2 walk the items; wave 3 takes what is left of them, and canbreak
    const double *sx = io.sx;
    DevCalib &C = *cal;
    float *sKi = cbF + LD_TAIL_KI;          // 9 floats of the scratch behind the canbreak sums
    int *sFlag = (int *) (cbF + LD_TAIL_FLAG);          // cleared by the caller before the solve
    const bool split = F * F <= 64;          // one wavefront holds all pairs
    const int items = F * F * 8, nMain = (items / W2) * W2;
    float *xf = io.sTail + (wave > 0 ? wave - 1 : 0) * 2 * LD_XFP, *df = xf + LD_XFP;
    const float *adH = io.adH, *adT = io.adT;
    const int adPitch = io.adPitch;
    // xAd[i] = x_h^T adHostF[:, c] + x_t^T adTargetF[:, c] (EnergyFunctional.cc:491-516), adHTdeltaF likewise from the deltas (:403-414)
    auto item = [&](int i) {
        const int c = i & 7, pr = i >> 3, h = pr / F, t = pr % F;
        const int sl = (adPitch == 64) ? h + F * t : pr;          // the LDS copies are ordered by pr = h F + t
        const float *AH = adH + (size_t) sl * adPitch, *AT = adT + (size_t) sl * adPitch;
        float ah[8], at[8];
#pragma unroll
        for (int k = 0; k < 8; k++) { ah[k] = AH[k * 8 + c]; at[k] = AT[k * 8 + c]; }
        const float4 xh0 = *(const float4 *) (xf + 4 + 8 * h), xh1 = *(const float4 *) (xf + 8 + 8 * h), xt0 = *(const float4 *) (xf + 4 + 8 * t), xt1 = *(const float4 *) (xf + 8 + 8 * t);
        const float4 dh0 = *(const float4 *) (df + 4 + 8 * h), dh1 = *(const float4 *) (df + 8 + 8 * h), dt0 = *(const float4 *) (df + 4 + 8 * t), dt1 = *(const float4 *) (df + 8 + 8 * t);
        const float xh[8] = {xh0.x, xh0.y, xh0.z, xh0.w, xh1.x, xh1.y, xh1.z, xh1.w}, xt[8] = {xt0.x, xt0.y, xt0.z, xt0.w, xt1.x, xt1.y, xt1.z, xt1.w};
        const float dh[8] = {dh0.x, dh0.y, dh0.z, dh0.w, dh1.x, dh1.y, dh1.z, dh1.w}, dt[8] = {dt0.x, dt0.y, dt0.z, dt0.w, dt1.x, dt1.y, dt1.z, dt1.w};
        float s1 = 0, s2 = 0, d1 = 0, d2 = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) { s1 += xh[k] * ah[k]; d1 += dh[k] * ah[k]; }
#pragma unroll
        for (int k = 0; k < 8; k++) { s2 += xt[k] * at[k]; d2 += dt[k] * at[k]; }
        B.xAd[i] = s1 + s2;
        B.pairs[pr].dp[c] = d1 + d2;
    };
    if (wave == 0) {
        if (lane < F) {
            double st[8];
#pragma unroll
            for (int a = 0; a < 8; a++) st[a] = fr[lane].state[a] + (-sx[4 + 8 * lane + a]);          // doStepFromBackup: state = backup + step, step = -x
            frame_pose(fr[lane], st);
        }
        if (LD_STAMP_ON && tid == 0) B.energyLog[59] = (double) wall_clock64();          // frame poses done
        if (split) {
            // poses, calibration floats and pair records all belong to this wave: no workgroup barrier between them
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            // wave 3: calibration floats, K^-1 (long done).  Bounded like the p2p polls: a flag that never comes (a launch shape this was not written for) ends
            // in the non-finite status of the iteration (scalars[4]) instead of a hung kernel
            int spins = 0;
            while (__hip_atomic_load(sFlag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) == 0 && ++spins < (1 << 22)) __builtin_amdgcn_s_sleep(1);
            if (spins >= (1 << 22) && lane == 0) B.scalars[4] = 1.0;
            if (lane < F * F) pair_record<false>(B, fr, C, F, lane, sKi);
        }
        if (LD_STAMP_ON && tid == 0) B.energyLog[62] = (double) wall_clock64();          // wave 0 at the barrier
    } else {
        bool bad = false;
        for (int i = lane; i < n; i += 64) {
            const double x = sx[i];
            double d = 0.0;
            if (i >= 4) {
                const int f = (i - 4) >> 3, a = (i - 4) & 7;
                const double bk = fr[f].state[a];
                d = (bk + (-x)) - fr[f].state_zero[a];
                if (wave == 2) { fr[f].step[a] = -x; fr[f].state_backup[a] = bk; }          // backupState, the step: written only, by nobody else
            }
            xf[i] = (float) x; df[i] = (float) d;
            if (wave == 1) { B.x[i] = x; if (!isfinite(x)) bad = true; }
        }
        if (wave == 2 && lane < 2 * F) { const int f = lane >> 1, a = 8 + (lane & 1); fr[f].step[a] = 0.0; fr[f].state_backup[a] = fr[f].state[a]; }
        if (bad) B.scalars[4] = 1.0;
        // the copies are private to the wave; LDS executes a wavefront's accesses in order
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (wave < 3) for (int i = tid - 64; i < nMain; i += W2) item(i);
        if (wave == 3) {
            // the calibration: backupState + doStepFromBackup, the derived floats, K^-1 for the pair records - one lane, off wave 0's chain (a branch of
            // its own there ran behind the poses: +0.25 us); handed to wave 0 through a flag in LDS (a wavefront's LDS accesses complete in order)
            if (lane == 63) {
                double v[4];
#pragma unroll
                for (int a = 0; a < 4; a++) {
                    const double stp = -sx[a], bk = C.value[a];
                    v[a] = bk + stp * (double) 1.0f;
                    C.step[a] = stp; C.value_backup[a] = bk; C.value[a] = v[a]; B.xc[a] = (float) sx[a];
                }
                calib_derived(C, v);
                float Ki[9];
                k_inverse((float) (50.0 * v[0]), (float) (50.0 * v[1]), (float) (50.0 * v[2]), (float) (50.0 * v[3]), Ki);          // = C.sf
                for (int q = 0; q < 9; q++) sKi[q] = Ki[q];
                __hip_atomic_store(sFlag, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
            for (int i = nMain + lane; i < items; i += 64) item(i);
            // canbreak (FullSystem.cc:1604-1622): the four sums, their square roots and comparisons on four lanes side by side, the conjunction by ballot
            // (one lane walking sqrt -> compare -> branch four times in a row, behind a round trip through LDS, took as long as the sums)
            bool ok = true;
            if (lane < 4) {
                float v = sqrtf(canbreak_partial_x(sx, F, lane));
                if (lane == 2) v = v * io.sumNID;
                ok = v < ((lane == 0) ? 0.0005 : 0.00005) * St.thOptIterations;
            }
            const bool cb = (__ballot(ok) & 0xFull) == 0xFull;
            if (lane == 0) {
                B.scalars[3] = cb ? 1.0 : 0.0;
                // un-forced optimize(): end the loop after this iteration (FullSystem.cc:829)
                if (cbIter >= 0 && cb && cbIter >= St.minOptIterations && (double) cbIter < B.scalars[LD_SC_STOP]) B.scalars[LD_SC_STOP] = (double) cbIter;
                // tell the host at once which iteration ended the loop (it then enqueues the tail behind the iterations that turn into no-ops
                // instead of synchronising with the stream first); iterations after the stop return at their first instruction and never get here
                if (hostStop != nullptr && cbIter >= 0 && (B.scalars[LD_SC_STOP] == (double) cbIter || cbIter == lastIt))
                    __hip_atomic_store(hostStop, cbIter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
            if (LD_STAMP_ON && lane == 0) B.energyLog[63] = (double) wall_clock64();          // wave 3 at the barrier
        }
        if (LD_STAMP_ON && tid == 64) B.energyLog[58] = (double) wall_clock64();          // wave 1 at the barrier
    }
    if (!split) {
        __syncthreads();
        for (int i = tid; i < F * F; i += NT) pair_record<false>(B, fr, C, F, i, sKi);
    }
    // The frames' NEW states are in delta_prior (= state, setPrecalcValues); the state fields of the working copies still hold the old ones - they were
    // read by every wave up to here.  The caller's write-back of the copies takes state[0..7] from delta_prior (gn_solve_body).
    __syncthreads();
}

template <bool WAIT>
static __device__ __forceinline__ void gn_solve_body(const BaPtrs &B, const BaDims &D, const ResSet &S, const ldso_settings_t &St, const SolveArgs &A, const int role) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int tid = threadIdx.x, F = D.F, n = D.n;
    char *const top = (char *) (sm + core_lds_end(LD_SOLVE_NB(n), n));
    if (LD_ITER_SKIPPED(B, A.itCheck)) return;
    const long long t0_ = wall_clock64();
#define GSTAMP(i) do { if (LD_STAMP_ON && tid == 0) B.energyLog[40 + (i)] = (double) (wall_clock64() - t0_); } while (0)
    if (role == 1) {
        constexpr GnStatsLds lds = gn_stats_lds();
        double *sW1 = (double *) ((char *) sm + lds.sW);
        int *sTh = (int *) ((char *) sm + lds.sTh);
        if (A.reduceIn != nullptr) {
            // multi-GPU: the sums over all ranks arrive in the all-reduce buffer (k_gn_export layout), the candidates behind them
            const double *sc = A.reduceIn;
            if (tid == 0) { B.scalars[0] = sc[0]; B.scalars[1] = sc[1]; B.scalars[2] = sc[2]; B.scalars[6] = sc[3]; B.scalars[7] = sc[4]; B.scalars[9] = sc[5]; B.scalars[10] = sc[6]; }
            __syncthreads();
            post_thresh(B, D, S, St, A.reduceIn + 8, sTh);
        } else {
            post_sums(B, D, S, sW1);
            GSTAMP(10);
            res_counts(B, D, S, sW1);
            GSTAMP(11);
            post_thresh(B, D, S, St, nullptr, sTh);
            GSTAMP(12);
        }
        if (tid == 0 && A.logIdx >= 0 && A.logIdx < 64) B.energyLog[A.logIdx] = B.scalars[0];
        return;
    }
    const GnLds lds = gn_lds(F);
    double *sW = (double *) (top + lds.sW);
    DevFrame *sFr = (DevFrame *) (top + lds.sFr);
    DevCalib *sCal = (DevCalib *) (top + lds.sCal);
    if (LD_STAMP_ON && tid == 0) B.energyLog[39] = (double) t0_;
    SolveIO io;
    io.fr = sFr; io.cal = sCal; io.adH = B.adHostF; io.adT = B.adTargetF; io.adPitch = 64; io.sRed = sW; io.sumNID = 0; io.lambda = A.lambda; io.hasPrior = A.hasPrior; io.redScalars = A.reduceIn; io.waitCtr = A.waitCtr; io.waitTarget = A.waitTarget;
    io.ldsAd = gn_mirrors_adjoints(F) ? (float *) (sCal + 1) : nullptr;
    if (tid == 0) *(int *) ((float *) (sW + LD_SW_RED) + LD_TAIL_FLAG) = 0;          // gn_tail's hand-over flag (the solve's barriers publish it)
    solve_core_dispatch<true, WAIT>(B, D, S, St, A.iteration, sm, io);      // + mirrors
    GSTAMP(4);
    GSTAMP(5);
    gn_tail(B, D, sFr, sCal, io, St, (float *) (sW + LD_SW_RED), A.itCheck, A.hostStop, A.lastIt);      // x, xAd, backupState + doStepFromBackup + canbreak, setPrecalcValues
    GSTAMP(6);
    // write the mirrors back (all but frameEnergyTH, which block 1 owns)
    {
        unsigned *gF = (unsigned *) B.frames; const unsigned *lF = (const unsigned *) sFr;
        const int W = (int) (sizeof(DevFrame) / 4), skip = (int) (offsetof(DevFrame, frameEnergyTH) / 4);
        const int s0 = (int) (offsetof(DevFrame, state) / 4), dp0 = (int) (offsetof(DevFrame, delta_prior) / 4);
        for (int i = tid; i < F * W; i += NT) {
            const int w = i % W;
            if (w != skip) gF[i] = lF[(w >= s0 && w < s0 + 16) ? i - s0 + dp0 : i];          // doStepFromBackup: state[0..7] = the new states (gn_tail)
        }
        unsigned *gC = (unsigned *) B.calib; const unsigned *lC = (const unsigned *) sCal;
        for (int i = tid; i < (int) (sizeof(DevCalib) / 4); i += NT) gC[i] = lC[i];
    }
}
#undef GSTAMP
