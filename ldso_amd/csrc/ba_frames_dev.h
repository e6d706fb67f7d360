// ba_frames_dev.h — the frame, calibration and pair records of the control step as device functions (gfx950), shared by the step-wise body (solve_body) and the
// Gauss-Newton tail (gn_tail) of ba_solve_body.h: set_adjoints (SK_ADJ), frames_backup / frames_step (SK_BACKUP / SK_STEP), set_precalc (SK_PRECALC) and the pieces
// gn_tail lays out by wavefront (frame_pose, calib_derived, pair_record, canbreak_*).  The reference's lines are listed with the SK_ flags in ba_solve_body.h.
#pragma once
#include <hip/hip_runtime.h>
#include "ba_dev.h"
#include "lie_dev.h"
#include "ba_stats.h"          // NT, wave_sum_dpp

static __device__ void frame_nullspaces(DevFrame &f) { ld::frame_nullspaces(f.evalPT, f.state_zero[6], f.ab_exposure, f.ns_pose, f.ns_scale, f.ns_affine); }

// setAdjointsF + nullspace basis U (n x 7, columns with dropped singular values zeroed)
static __device__ __forceinline__ void set_adjoints(const BaPtrs &B, const BaDims &D, const ldso_settings_t &St, double *sW /*LDS scratch >= 7*n + 64 doubles*/, bool withNullspace,
                                    double *sBig /*LDS >= 37 * F * F doubles (the solve-core region, idle here)*/) {
    const int tid = threadIdx.x, F = D.F, n = D.n;
    // (1) one lane per pair: Adj(T_t T_h^-1) at the evaluation points and the affine factor -> LDS
    for (int i = tid; i < F * F; i += NT) {
        int h = i % F, t = i / F;      // slot h + t*F
        const DevFrame &fh = B.frames[h], &ft = B.frames[t];
        double Ti[12], T[12], Adj[36];
        ld::se3_inv(fh.evalPT, Ti);
        ld::se3_mul(ft.evalPT, Ti, T);
        ld::se3_adj(T, Adj);
        float a, b;
        aff_from_to(fh.ab_exposure, ft.ab_exposure, (float) (fh.state_zero[6] * 10.0), (float) (fh.state_zero[7] * 1000.0),
                    (float) (ft.state_zero[6] * 10.0), (float) (ft.state_zero[7] * 1000.0), a, b);
#pragma unroll
        for (int e = 0; e < 36; e++) sBig[i * 37 + e] = Adj[e];
        sBig[i * 37 + 36] = (double) a;
    }
    __syncthreads();
    // (2) one thread per entry of the two 8x8 adjoints (EnergyFunctional.cc:431-489), coalesced stores of the four tables
    for (int idx = tid; idx < F * F * 64; idx += NT) {
        const int i = idx >> 6, e = idx & 63, r = e >> 3, c = e & 7;
        const double *Adj = sBig + i * 37;
        const double a = Adj[36];
        double AH = (r == c) ? 1.0 : 0.0, AT = AH;
        if (r < 6 && c < 6) AH = -Adj[c * 6 + r];
        if (e == 6 * 8 + 6) { AT = -a; AH = a; }
        if (e == 7 * 8 + 7) { AT = -1.0; AH = a; }
        const double rs = (r < 3) ? 0.5 : (r < 6) ? 1.0 : (r == 6) ? 10.0 : 1000.0;
        AH *= rs; AT *= rs;
        B.adHost[idx] = AH; B.adTarget[idx] = AT;
        B.adHostF[idx] = (float) AH; B.adTargetF[idx] = (float) AT;
    }
    if (!withNullspace) { __syncthreads(); return; }
    // ---- N = [6 pose | 1 scale] nullspaces, columns normalised (FullSystem.cc:1711-1760, EF.cc:691-694) -----
    double *N = sW;               // column-major n x 7
    for (int i = tid; i < n * 7; i += NT) {
        int c = i / n, r = i % n;
        double v = 0;
        if (r >= 4) {
            int f = (r - 4) / 8, o = (r - 4) % 8;
            if (o < 6) {
                v = (c < 6) ? B.frames[f].ns_pose[o * 6 + c] : B.frames[f].ns_scale[o];
                v *= (o < 3) ? (double) (1.0f / 0.5f) : (double) (1.0f / 1.0f);
            }
        }
        N[c * n + r] = v;
    }
    __syncthreads();
    if (tid < 64) {
        // one wave: normalise, then one-sided Jacobi (Hestenes) on the 7 columns
        const int lane = tid;
        for (int c = 0; c < 7; c++) {
            double s = 0;
            for (int r = lane; r < n; r += 64) s += N[c * n + r] * N[c * n + r];
            s = sqrt(wave_sum_dpp(s));
            for (int r = lane; r < n; r += 64) N[c * n + r] /= s;
        }
        for (int sweep = 0; sweep < 30; sweep++) {
            double off = 0;
            for (int p = 0; p < 6; p++)
                for (int q = p + 1; q < 7; q++) {
                    double al = 0, be = 0, ga = 0;
                    for (int r = lane; r < n; r += 64) { double a = N[p * n + r], b = N[q * n + r]; al += a * a; be += b * b; ga += a * b; }
                    al = wave_sum_dpp(al); be = wave_sum_dpp(be); ga = wave_sum_dpp(ga);
                    if (ga == 0) continue;
                    off = fmax(off, fabs(ga) / sqrt(al * be + 1e-300));
                    double zeta = (be - al) / (2 * ga);
                    double tt = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1 + zeta * zeta));
                    double cs = 1 / sqrt(1 + tt * tt), sn = cs * tt;
                    for (int r = lane; r < n; r += 64) { double a = N[p * n + r], b = N[q * n + r]; N[p * n + r] = cs * a - sn * b; N[q * n + r] = sn * a + cs * b; }
                }
            if (off < 1e-15) break;
        }
        double sv[7], maxSv = 0;
        for (int c = 0; c < 7; c++) {
            double s = 0;
            for (int r = lane; r < n; r += 64) s += N[c * n + r] * N[c * n + r];
            sv[c] = sqrt(wave_sum_dpp(s));
            maxSv = fmax(maxSv, sv[c]);
        }
        for (int c = 0; c < 7; c++) {
            bool keep = sv[c] > St.solverModeDelta * maxSv;
            for (int r = lane; r < n; r += 64) B.nsProj[c * n + r] = keep ? N[c * n + r] / sv[c] : 0.0;
        }
    }
    __syncthreads();
}

// canbreak of doStepFromBackup (FullSystem.cc:1604-1622) in two parts so that it can overlap setPrecalcValues: the four
// sums are accumulated by lanes of waves 1..3 (wave 0 is busy with the frame exponentials), the decision is taken by one
// thread after the next block barrier.
static __device__ __forceinline__ void canbreak_partial(const DevFrame *fr, int F, float *sF /*4 floats of LDS*/) {
    const int tid = threadIdx.x;
    const int which = (tid == 64) ? 0 : (tid == 65) ? 1 : (tid == 128) ? 2 : (tid == 192) ? 3 : -1;
    if (which < 0) return;
    float acc = 0;
    for (int f = 0; f < F; f++) {
        const double *s = fr[f].step;
        if (which == 0) acc += s[6] * s[6];
        else if (which == 1) acc += s[7] * s[7];
        else if (which == 2) acc += s[0] * s[0] + s[1] * s[1] + s[2] * s[2];
        else acc += s[3] * s[3] + s[4] * s[4] + s[5] * s[5];
    }
    acc /= F;
    sF[which] = acc;
}
// the same four sums from the solution vector x (step = -x: the squares are the same numbers), by lanes 0..3 of the calling wavefront.  No branch on
// `which` around the loads: four lanes taking four different branches, each with its own LDS round trips inside the loop over the frames, took 2.8 us
static __device__ __forceinline__ float canbreak_partial_x(const double *x, int F, int which) {
    const int base = (which == 0) ? 6 : (which == 1) ? 7 : (which == 2) ? 0 : 3;
    const bool three = which >= 2;
    const int o1 = three ? base + 1 : base, o2 = three ? base + 2 : base;
    float acc = 0;
    for (int f0 = 0; f0 < F; f0 += 8) {
        double a[8], b[8], c[8];
#pragma unroll
        for (int u = 0; u < 8; u++) { const double *s = x + 4 + 8 * min(f0 + u, F - 1); a[u] = s[base]; b[u] = s[o1]; c[u] = s[o2]; }
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const double v1 = a[u] * a[u], v3 = a[u] * a[u] + b[u] * b[u] + c[u] * c[u];
            if (f0 + u < F) acc += three ? v3 : v1;
        }
    }
    acc /= F;
    return acc;
}
static __device__ __forceinline__ void canbreak_final(const BaPtrs &B, const ldso_settings_t &St, const float *sF, float sumNID) {
    const float sumA = sF[0], sumB = sF[1], sumT = sF[2], sumR = sF[3];
    bool cb = sqrtf(sumA) < 0.0005 * St.thOptIterations && sqrtf(sumB) < 0.00005 * St.thOptIterations &&
              sqrtf(sumR) < 0.00005 * St.thOptIterations && sqrtf(sumT) * sumNID < 0.00005 * St.thOptIterations;
    B.scalars[3] = cb ? 1.0 : 0.0;
}

// ---- pieces of setPrecalcValues shared by the step-wise path (set_precalc) and the GN tail (gn_tail) ----
// one frame: PRE_worldToCam = exp(state) evalPT, its inverse, the deltas, from the state st[8] the caller holds in registers.  Everything is computed in
// registers and stored afterwards - written straight into the frame, every store would force the loads that follow it to wait for it
static __device__ __forceinline__ void frame_pose(DevFrame &f, const double *st) {
    double sz[8], ev[12];
#pragma unroll
    for (int i = 0; i < 8; i++) sz[i] = f.state_zero[i];
#pragma unroll
    for (int i = 0; i < 12; i++) ev[i] = f.evalPT[i];
    const double ss[6] = {0.5 * st[0], 0.5 * st[1], 0.5 * st[2], 1.0 * st[3], 1.0 * st[4], 1.0 * st[5]};
    double E[12], P[12], Pi[12];
    ld::se3_exp(ss, E);
    ld::se3_mul(E, ev, P);
    ld::se3_inv(P, Pi);
#pragma unroll
    for (int i = 0; i < 12; i++) { f.PRE_w2c[i] = P[i]; f.PRE_c2w[i] = Pi[i]; }
#pragma unroll
    for (int i = 0; i < 8; i++) { f.delta[i] = st[i] - sz[i]; f.delta_prior[i] = st[i]; }
}
// CalibHessian::setValue derived floats (CalibHessian.h:71-85) from the calibration value v[4]
static __device__ __forceinline__ void calib_derived(DevCalib &C, const double *v) {
    float sf[4], dl[4];
    for (int i = 0; i < 4; i++) { sf[i] = (float) (50.0 * v[i]); dl[i] = (float) (v[i] - C.value_zero[i]); }
    for (int i = 0; i < 4; i++) { C.sf[i] = sf[i]; C.cDeltaF[i] = dl[i]; }
    C.si[0] = 1.0f / sf[0]; C.si[1] = 1.0f / sf[1]; C.si[2] = -sf[2] / sf[0]; C.si[3] = -sf[3] / sf[1];
}
// one pair record.  The affine parameters come from delta_prior (= state, written by frame_pose): inside gn_tail the states themselves are being
// stored by other wavefronts while this runs.  FULL = false (inside a GN iteration): the linearisation-point part of a pair (R0, t0, b0: functions of
// evalPT and state_zero only) is left untouched.
// K^-1 by Eigen's 3x3 cofactor inverse (float)
static __device__ __forceinline__ void k_inverse(float fx, float fy, float cx, float cy, float *Ki) {
    const float K[9] = {fx, 0, cx, 0, fy, cy, 0, 0, 1};
    auto cof = [&](int a, int b) { int a1 = (a + 1) % 3, a2 = (a + 2) % 3, b1 = (b + 1) % 3, b2 = (b + 2) % 3; return K[a1 * 3 + b1] * K[a2 * 3 + b2] - K[a1 * 3 + b2] * K[a2 * 3 + b1]; };
    float k0 = cof(0, 0), k1 = cof(1, 0), k2 = cof(2, 0);
    float det = (k0 * K[0] + k1 * K[3]) + k2 * K[6];
    float invdet = 1.0f / det;
    Ki[0] = k0 * invdet; Ki[1] = k1 * invdet; Ki[2] = k2 * invdet;
    Ki[3] = cof(0, 1) * invdet; Ki[4] = cof(1, 1) * invdet; Ki[5] = cof(2, 1) * invdet;
    Ki[6] = cof(0, 2) * invdet; Ki[7] = cof(1, 2) * invdet; Ki[8] = cof(2, 2) * invdet;
}
// KiShared: K^-1 of the current calibration where the caller has it (gn_tail: computed once beside the frame poses), or nullptr
template <bool FULL>
static __device__ __forceinline__ void pair_record(const BaPtrs &B, const DevFrame *fr, const DevCalib &C, int F, int i, const float *KiShared = nullptr) {
    const int h = i / F, t = i % F;
    const DevFrame &fh = fr[h], &ft = fr[t];
    DevPair &o = B.pairs[i];
    // every operand into registers before the first store of the record
    double Tw[12], Hc[12], T[12];
#pragma unroll
    for (int q = 0; q < 12; q++) { Tw[q] = ft.PRE_w2c[q]; Hc[q] = fh.PRE_c2w[q]; }
    const float expH = fh.ab_exposure, expT = ft.ab_exposure;
    const float aH = (float) (10.0f * fh.delta_prior[6]), bH = (float) (1000.0f * fh.delta_prior[7]), aT = (float) (10.0f * ft.delta_prior[6]), bT = (float) (1000.0f * ft.delta_prior[7]);
    const float fx = C.sf[0], fy = C.sf[1], cx = C.sf[2], cy = C.sf[3];
    ld::se3_mul(Tw, Hc, T);
    float R[9], tt[3];
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) R[r * 3 + c] = (float) T[r * 4 + c]; tt[r] = (float) T[r * 4 + 3]; }
    // PRE_RTll / PRE_tTll for point activation: only where the host can call it (after set_frames / optimize), not inside GN iterations
    if (FULL) { float *rt = B.pairRt + (size_t) i * 12; for (int q = 0; q < 9; q++) rt[q] = R[q]; for (int q = 0; q < 3; q++) rt[9 + q] = tt[q]; }
    if (FULL) {
        double Ti[12], T0[12];
        ld::se3_inv(fh.evalPT, Ti);
        ld::se3_mul(ft.evalPT, Ti, T0);
        for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) o.R0[r * 3 + c] = (float) T0[r * 4 + c]; o.t0[r] = (float) T0[r * 4 + 3]; }
        o.b0 = (float) (fh.state_zero[7] * 1000.0);
        o.thMax = fmaxf(fh.frameEnergyTH, ft.frameEnergyTH);
    }
    const float K[9] = {fx, 0, cx, 0, fy, cy, 0, 0, 1};
    float Ki[9];
    if (KiShared != nullptr) { for (int q = 0; q < 9; q++) Ki[q] = KiShared[q]; }
    else k_inverse(fx, fy, cx, cy, Ki);
    float KR[9], KRKi[9], Kt[3];
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) KR[r * 3 + c] = (K[r * 3 + 0] * R[0 * 3 + c] + K[r * 3 + 1] * R[1 * 3 + c]) + K[r * 3 + 2] * R[2 * 3 + c];
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) KRKi[r * 3 + c] = (KR[r * 3 + 0] * Ki[0 * 3 + c] + KR[r * 3 + 1] * Ki[1 * 3 + c]) + KR[r * 3 + 2] * Ki[2 * 3 + c];
    for (int r = 0; r < 3; r++) Kt[r] = (K[r * 3 + 0] * tt[0] + K[r * 3 + 1] * tt[1]) + K[r * 3 + 2] * tt[2];
    float a0_, b0_;
    aff_from_to(expH, expT, aH, bH, aT, bT, a0_, b0_);
    for (int q = 0; q < 9; q++) o.KRKi[q] = KRKi[q];
    for (int q = 0; q < 3; q++) o.Kt[q] = Kt[q];
    o.aff[0] = a0_; o.aff[1] = b0_;
}

// setPrecalcValues of the step-wise path and of the host entry points: frames' PRE poses, pair precalc (with the linearisation-point part), deltas
static __device__ __forceinline__ void set_precalc(const BaPtrs &B, const BaDims &D, DevFrame *fr, DevCalib *cal, const float *adH, const float *adT) {
    const int tid = threadIdx.x, F = D.F;
    DevCalib &C = *cal;
    if (tid < F) {
        double st[8];
        for (int i = 0; i < 8; i++) st[i] = fr[tid].state[i];
        frame_pose(fr[tid], st);
    }
    if (tid == 64) {
        double v[4];
        for (int i = 0; i < 4; i++) v[i] = C.value[i];
        calib_derived(C, v);
    }
    __syncthreads();
    for (int i = tid; i < F * F; i += NT) pair_record<true>(B, fr, C, F, i);
    // adHTdeltaF[h + t*F] = delta_h^T adHostF + delta_t^T adTargetF  (EnergyFunctional.cc:403-414), one thread per component; the frames' delta is
    // state - state_zero in double, stored exactly: converting it is converting the difference
    for (int i = tid; i < F * F * 8; i += NT) {
        const int c = i & 7, pr = i >> 3, h = pr / F, t = pr % F;
        const DevFrame &fh = fr[h], &ft = fr[t];
        const float *AH = adH + (size_t) (h + t * F) * 64, *AT = adT + (size_t) (h + t * F) * 64;
        float s1 = 0, s2 = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) s1 += (float) fh.delta[k] * AH[k * 8 + c];
#pragma unroll
        for (int k = 0; k < 8; k++) s2 += (float) ft.delta[k] * AT[k * 8 + c];
        B.pairs[pr].dp[c] = s1 + s2;
    }
    __syncthreads();
}

// frame / calibration part of backupState, doStepFromBackup (+ canbreak), loadSateBackup on the working copies
static __device__ void frames_backup(DevFrame *fr, DevCalib *cal, int F) {
    const int tid = threadIdx.x;
    if (tid < F) for (int i = 0; i < 10; i++) fr[tid].state_backup[i] = fr[tid].state[i];
    if (tid == 0) for (int i = 0; i < 4; i++) cal->value_backup[i] = cal->value[i];
    __syncthreads();
}
static __device__ __forceinline__ void frames_step(const BaPtrs &B, const ldso_settings_t &St, DevFrame *fr, DevCalib *cal, int F, float sumNID, double *sRed) {
    const int tid = threadIdx.x;
    if (tid < F) for (int i = 0; i < 10; i++) fr[tid].state[i] = fr[tid].state_backup[i] + fr[tid].step[i];
    if (tid == 0) for (int i = 0; i < 4; i++) cal->value[i] = cal->value_backup[i] + cal->step[i] * (double) 1.0f;
    canbreak_partial(fr, F, (float *) (sRed + 8));
    __syncthreads();
    if (tid == 0) canbreak_final(B, St, (const float *) (sRed + 8), sumNID);
    __syncthreads();
}
