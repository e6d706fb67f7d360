// ba_step.hip — the kernels of a Gauss-Newton iteration's control side that never touch the solver (gfx950): the point part of the step (k_point_step), the
// two energies of the LM accept test (k_lm_energies) and the multi-GPU export of the statistics (k_gn_export).  The control kernels are ba_solve.hip.
#include <hip/hip_runtime.h>
#include "ba_host.h"
#include "ba_stats.h"

// ---------------------------------------------------------------------------------------------------------
// k_gn_export (multi-GPU fast path): rank-local scalar sums and newest-frame energy candidates into the tail of the all-reduce
// buffer  [HFinal lower | bFinal | 8 scalars | P candidates (value+1, 0 = none)]  whose head k_reduce accumulated (B.acc).
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void k_gn_export(BaPtrs B, BaDims D, ResSet S, double *tail) {
    __shared__ double sW[16];
    const int tid = threadIdx.x;
    if (blockIdx.x == 0) {
        post_sums(B, D, S, sW);
        res_counts(B, D, S, sW);
        if (tid == 0) { tail[0] = B.scalars[0]; tail[1] = B.scalars[1]; tail[2] = B.scalars[2]; tail[3] = B.scalars[6]; tail[4] = B.scalars[7];
                        tail[5] = B.scalars[9]; tail[6] = B.scalars[10]; tail[7] = 0; }
        return;
    }
    const int i = (blockIdx.x - 1) * NT + tid;
    if (i < D.P) {
        double v = 0.0;
        if (i >= D.pBegin && i < D.pEnd) { const float c = S.candE[i]; if (c >= 0.0f) v = (double) c + 1.0; }
        tail[8 + i] = v;
    }
}

hipError_t ba_launch_gn_export(const BaPtrs &B, const BaDims &D, const ResSet &S, double *tail, hipStream_t st) {
    hipLaunchKernelGGL(k_gn_export, dim3(1 + (D.P + NT - 1) / NT), dim3(NT), 0, st, B, D, S, tail);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------
// point part of resubstituteFPt + doStepFromBackup / backupState / loadSateBackup
//   (EnergyFunctional.cc:518-547, FullSystem.cc:1585-1602)
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_point_step(BaPtrs B, BaDims D, ResSet S, int mode) {
    const int p = D.pBegin + blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= D.pEnd) return;
    PtGeo &Gp = B.pgeo[p];
    if (mode & PS_LOAD) { float b = Gp.idepth_backup; Gp.idepth = b; Gp.idepth_zero = b; return; }   // loadSateBackup
    const int F = D.F, FS = D.FS, h = B.phost[p];
    float step = Gp.step;
    PtRec &R = S.pt[p];
    if (mode & PS_RESUB) { Gp.lastHdiF = R.HdiF; Gp.lastBdSumF = R.bdSumF; Gp.lastIdH = R.idH; }      // what this solve's accumulateSCF_MT left in the point
    if ((mode & PS_RESUB) && R.nActive <= 0) { step = 0.0f; R.maxRelBS = 0.0f; }      // AccumulatedSCHessian.cc:14-21 (zeroed by the solve)
    if ((mode & PS_RESUB) && R.nActive > 0) {
        float b = R.bdSumF;
        float dot = 0;
        for (int i = 0; i < 4; i++) dot += B.xc[i] * (R.HcdA[i] + R.HcdL[i]);
        b -= dot;
        bool finite = true;
        for (int t = 0; t < F; t++) {
            int slot = p * FS + t;
            const SlotRec &sr = S.slot[slot];
            if (B.rtab[slot].rflat < 0 || !sr.e[LD_SM_ACTIVE].m.i) continue;
            const float *xa = B.xAd + (size_t) (h * F + t) * 8;
            float s = 0;
            for (int i = 0; i < 8; i++) s += xa[i] * sr.e[i].jp;
            b -= s;
        }
        if (!isfinite(b)) finite = false;
        if (finite) step = -b * R.HdiF; else { step = Gp.step; B.scalars[4] = 1.0; }
    }
    Gp.step = step;
    if (mode & PS_BACKUP) Gp.idepth_backup = Gp.idepth;
    if (mode & PS_STEP) {     // doStepFromBackup (stepfacD = 1)
        float ni = Gp.idepth_backup + 1.0f * step;
        Gp.idepth = ni;
        Gp.idepth_zero = ni;
    }
}

// ---------------------------------------------------------------------------------------------------------
// k_lm_energies — the two energies of the LM accept test (FullSystem.cc:805-826):
//   scalars[12] = EnergyFunctional::calcMEnergyF (EnergyFunctional.cc:353-359):  delta^T (2 b_M + H_M delta)
//   scalars[13] = EnergyFunctional::calcLEnergyF_MT (:361-378, calcLEnergyPt :627-682): prior terms of frames / calibration /
//                 points + the linearised residuals' (2 res_toZeroF + J delta) . J delta
// One workgroup; sums in double (the reference accumulates the point part in float Accumulator11: same value to ~1e-6).
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_lm_energies(BaPtrs B, BaDims D, ResSet S, float calibPrior, int hasPrior) {
    __shared__ double sDelta[8 * LD_MAXF + 4];
    __shared__ double sRed[8];
    const int tid = threadIdx.x, F = D.F, n = D.n;
    for (int i = tid; i < n; i += 256) sDelta[i] = (i < 4) ? (double) B.calib->cDeltaF[i] : B.frames[(i - 4) >> 3].delta[(i - 4) & 7];
    __syncthreads();
    // ---- M energy ----
    double em = 0.0;
    if (hasPrior) for (int i = tid; i < n; i += 256) {
        double hd = 0.0;
        for (int j = 0; j < n; j++) hd += B.HM[(size_t) i * n + j] * sDelta[j];
        em += sDelta[i] * (2.0 * B.bM[i] + hd);
    }
    // ---- L energy: frame and calibration priors ----
    double el = 0.0;
    for (int i = tid; i < F * 8; i += 256) { const DevFrame &f = B.frames[i >> 3]; const double dp = f.delta_prior[i & 7]; el += dp * f.prior[i & 7] * dp; }
    if (tid < 4) { const float c = B.calib->cDeltaF[tid]; el += (double) (c * calibPrior * c); }
    // ---- L energy: points ----
    const float cD0 = B.calib->cDeltaF[0], cD1 = B.calib->cDeltaF[1], cD2 = B.calib->cDeltaF[2], cD3 = B.calib->cDeltaF[3];
    for (int p = D.pBegin + tid; p < D.pEnd; p += 256) {
        const float dd = B.pgeo[p].idepth - B.pgeo[p].idepth_zero;
        const int h = B.phost[p];
        double e = 0.0;
        for (int t = 0; t < F; t++) {
            const int slot = p * D.FS + t;
            const SlotTab tb = B.rtab[slot];
            if (tb.rflat < 0 || !tb.rlin || !S.slot[slot].e[LD_SM_ACTIVE].m.i) continue;
            const ldso_rawjac_t &J = B.Jlin[tb.rlidx];
            const float *rtz = B.rtz + (size_t) tb.rlidx * 8;
            const float *dp = B.pairs[h * F + t].dp;
            float jx = 0, jy = 0;
            for (int i = 0; i < 6; i++) { jx += J.Jpdxi[0][i] * dp[i]; jy += J.Jpdxi[1][i] * dp[i]; }
            jx = jx + (((J.Jpdc[0][0] * cD0 + J.Jpdc[0][1] * cD1) + J.Jpdc[0][2] * cD2) + J.Jpdc[0][3] * cD3) + J.Jpdd[0] * dd;
            jy = jy + (((J.Jpdc[1][0] * cD0 + J.Jpdc[1][1] * cD1) + J.Jpdc[1][2] * cD2) + J.Jpdc[1][3] * cD3) + J.Jpdd[1] * dd;
            for (int i = 0; i < 8; i++) {
                const float Jd = ((J.JIdx[0][i] * jx + J.JIdx[1][i] * jy) + J.JabF[0][i] * dp[6]) + J.JabF[1][i] * dp[7];
                e += (double) (Jd * ((rtz[i] + rtz[i]) + Jd));
            }
        }
        e += (double) (dd * dd * B.pgeo[p].priorF);
        el += e;
    }
    em = wave_sum(em); el = wave_sum(el);
    if ((tid & 63) == 0) { sRed[tid >> 6] = em; sRed[4 + (tid >> 6)] = el; }
    __syncthreads();
    if (tid == 0) { B.scalars[12] = sRed[0] + sRed[1] + sRed[2] + sRed[3]; B.scalars[13] = sRed[4] + sRed[5] + sRed[6] + sRed[7]; }
}

hipError_t ba_launch_lm_energies(const BaPtrs &B, const BaDims &D, const ResSet &S, float calibPrior, bool hasPrior, hipStream_t st) {
    hipLaunchKernelGGL(k_lm_energies, dim3(1), dim3(256), 0, st, B, D, S, calibPrior, hasPrior ? 1 : 0);
    return hipGetLastError();
}

hipError_t ba_launch_point_step(const BaPtrs &B, const BaDims &D, const ResSet &S, int mode, hipStream_t st) {
    int np = D.pEnd - D.pBegin;
    if (np <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_point_step, dim3((np + 255) / 256), dim3(256), 0, st, B, D, S, mode);
    return hipGetLastError();
}
