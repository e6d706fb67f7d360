// ba_stats.h — the statistics of a linearizeAll as device functions (gfx950): sums over the wavefront, the energy sum and the counters of the residual chunks
// (FullSystem::linearizeAll tail, FullSystem.cc:1762-1793) and setNewFrameEnergyTH.  Shared by the control kernels (ba_solve.hip, ba_solve_batch.hip: role 1 of
// solve_body / gn_solve_body) and by k_gn_export (ba_step.hip).  All sums are fp64 like the reference.
#pragma once
#include <hip/hip_runtime.h>
#include "ba_dev.h"

// Seen outside, on purpose: the workgroup size of every kernel that calls into this header, ba_frames_dev.h, ba_ldlt.h or ba_solve_body.h - their loops stride by it and
// the kernels launch with it.  ba_reduce_body.h names a template parameter NT: a unit that needs both includes that header first.
#define NT 256
#define TH_CAP 8192      // candidate energies staged in LDS up to this many points
#define LD_THRESH_DOUBLES ((256 + 8 + TH_CAP) / 2)      // LDS of the threshold pass (post_thresh), in doubles

static __device__ __forceinline__ double wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// the same sum over the 64 lanes through DPP row operations + four v_readlane (a dependent ds_bpermute costs 30 ns, a DPP step 7 ns):
// for the serial chains that are made of wave sums (the one-sided Jacobi of the nullspace basis)
template <int CTRL> static __device__ __forceinline__ double dpp_f64(double v) {
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned) __builtin_amdgcn_update_dpp(0, (int) (u & 0xFFFFFFFFu), CTRL, 0xF, 0xF, true);
    const unsigned hi = (unsigned) __builtin_amdgcn_update_dpp(0, (int) (u >> 32), CTRL, 0xF, 0xF, true);
    return __builtin_bit_cast(double, ((unsigned long long) hi << 32) | lo);
}
static __device__ __forceinline__ double readlane_d(double v, int lane) {
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned) __builtin_amdgcn_readlane((int) (u & 0xFFFFFFFFu), lane), hi = (unsigned) __builtin_amdgcn_readlane((int) (u >> 32), lane);
    return __builtin_bit_cast(double, ((unsigned long long) hi << 32) | lo);
}
static __device__ __forceinline__ double wave_sum_dpp(double v) {
    v += dpp_f64<0xB1>(v);       // quad_perm [1,0,3,2]
    v += dpp_f64<0x4E>(v);       // quad_perm [2,3,0,1]
    v += dpp_f64<0x141>(v);      // row_half_mirror
    v += dpp_f64<0x140>(v);      // row_mirror: every lane holds the sum of its 16-lane row
    return (readlane_d(v, 0) + readlane_d(v, 16)) + (readlane_d(v, 32) + readlane_d(v, 48));
}

// ---------------------------------------------------------------------------------------------------------
// setNewFrameEnergyTH: k-th smallest of the newest frame's residual energies by a 4-pass radix select
// ---------------------------------------------------------------------------------------------------------
static __device__ __forceinline__ void post_sums(const BaPtrs &B, const BaDims &D, const ResSet &S, double *sD /*8 doubles*/) {
    const int tid = threadIdx.x;
    // ---- energy sum + counters over the chunks, fixed order -----------------------------------------------
    {
        double e = 0; double na = 0, nl = 0, ns = 0, nc = 0;
        for (int c = tid; c < D.nChunks; c += NT) {
            e += S.chunkEnergy[c]; na += S.chunkCnt[c * 2]; nl += S.chunkCnt[c * 2 + 1];
            ns += (double) S.chunkNID[c * 2]; nc += (double) S.chunkNID[c * 2 + 1];
        }
        e = wave_sum(e); na = wave_sum(na); nl = wave_sum(nl); ns = wave_sum(ns); nc = wave_sum(nc);
        if ((tid & 63) == 0) { sD[(tid >> 6)] = e; sD[4 + (tid >> 6)] = na; }
        __syncthreads();
        if (tid == 0) { B.scalars[0] = sD[0] + sD[1] + sD[2] + sD[3]; B.scalars[1] = sD[4] + sD[5] + sD[6] + sD[7]; }
        __syncthreads();
        if ((tid & 63) == 0) { sD[(tid >> 6)] = nl; sD[4 + (tid >> 6)] = ns; }
        __syncthreads();
        if (tid == 0) { B.scalars[2] = sD[0] + sD[1] + sD[2] + sD[3]; B.scalars[6] = sD[4] + sD[5] + sD[6] + sD[7]; }
        __syncthreads();
        if ((tid & 63) == 0) sD[(tid >> 6)] = nc;
        __syncthreads();
        if (tid == 0) B.scalars[7] = sD[0] + sD[1] + sD[2] + sD[3];
        __syncthreads();
    }
}

// resInA / resInL of the accumulate that produced this set (EnergyFunctional.cc:558,573)
static __device__ __forceinline__ void res_counts(const BaPtrs &B, const BaDims &D, const ResSet &S, double *sD /*8 doubles*/) {
    const int tid = threadIdx.x;
    double na = 0, nl = 0;
    for (int c = tid; c < D.nChunks; c += NT) { na += S.chunkCnt[c * 2]; nl += S.chunkCnt[c * 2 + 1]; }
    na = wave_sum(na); nl = wave_sum(nl);
    if ((tid & 63) == 0) { sD[tid >> 6] = na; sD[4 + (tid >> 6)] = nl; }
    __syncthreads();
    if (tid == 0) { B.scalars[9] = sD[0] + sD[1] + sD[2] + sD[3]; B.scalars[10] = sD[4] + sD[5] + sD[6] + sD[7]; }
    __syncthreads();
}

// candidates: active-set residuals targeting the newest frame with state_NewEnergyWithOutlier >= 0,
// written compactly by the linearize kernel (S.candE[p], -1 = no candidate).
// extE (multi-GPU): all-reduced array of P doubles holding value+1 for candidates and 0 otherwise.
static __device__ __forceinline__ void post_thresh(const BaPtrs &B, const BaDims &D, const ResSet &S, const ldso_settings_t &St,
                                   const double *extE, int *sTh /*LDS, LD_THRESH_DOUBLES*/) {
    int *sHist = sTh, *sI = sHist + 256;          // histogram [256] | counters [8] | staged candidates [TH_CAP] float
    float *sVal = (float *) (sI + 8);
    const int tid = threadIdx.x;
    const int F = D.F;
    const int tN = F - 1;
    const int nItems = D.P;
    const bool inLds = nItems <= TH_CAP;
    // stage the candidate values (negative = not a candidate)
    for (int i0 = tid; i0 < nItems; i0 += NT * 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            int i = i0 + u * NT;
            v[u] = -1.0f;
            if (i < nItems) {
                if (extE != nullptr) { double d = extE[i]; v[u] = (d > 0.0) ? (float) (d - 1.0) : -1.0f; }
                else if (i >= D.pBegin && i < D.pEnd) v[u] = S.candE[i];
            }
        }
        if (inLds) {
#pragma unroll
            for (int u = 0; u < 8; u++) { int i = i0 + u * NT; if (i < nItems) sVal[i] = v[u]; }
        }
    }
    __syncthreads();
    auto value = [&](int i) -> float {
        if (inLds) return sVal[i];
        if (extE != nullptr) { double d = extE[i]; return (d > 0.0) ? (float) (d - 1.0) : -1.0f; }
        return (i >= D.pBegin && i < D.pEnd) ? S.candE[i] : -1.0f;
    };
    int cnt = 0;
    for (int i = tid; i < nItems; i += NT) if (value(i) >= 0.0f) cnt++;
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if ((tid & 63) == 0) sI[tid >> 6] = cnt;
    __syncthreads();
    const int total = sI[0] + sI[1] + sI[2] + sI[3];
    __syncthreads();
    DevFrame &nf = B.frames[tN];
    if (total == 0) {
        if (tid == 0) nf.frameEnergyTH = 12 * 12 * 8;
        __syncthreads();
    } else {
        int kth = (int) (St.frameEnergyTHN * (float) total);
        unsigned prefix = 0, mask = 0;
        for (int pass = 3; pass >= 0; pass--) {
            sHist[tid] = 0;
            __syncthreads();
            const int shift = pass * 8;
            for (int i = tid; i < nItems; i += NT) {
                float v = value(i);
                if (v >= 0.0f) {
                    unsigned u = __float_as_uint(v);
                    if ((u & mask) == prefix) atomicAdd(&sHist[(u >> shift) & 0xFF], 1);
                }
            }
            __syncthreads();
            {
                const int c = sHist[tid];
                int inc = c;
                for (int o = 1; o < 64; o <<= 1) { int v = __shfl_up(inc, o, 64); if ((tid & 63) >= o) inc += v; }
                if ((tid & 63) == 63) sI[tid >> 6] = inc;
                __syncthreads();
                int base = 0;
                for (int wv = 0; wv < (tid >> 6); wv++) base += sI[wv];
                inc += base;
                const int exc = inc - c;
                __syncthreads();
                if (c > 0 && exc <= kth && kth < inc) { sI[4] = tid; sI[5] = kth - exc; }
            }
            __syncthreads();
            prefix |= ((unsigned) sI[4]) << shift;
            mask |= 0xFFu << shift;
            kth = sI[5];
            __syncthreads();
        }
        if (tid == 0) {
            float nthElement = sqrtf(__uint_as_float(prefix));
            float th = nthElement * St.frameEnergyTHFacMedian;
            th = 26.0f * St.frameEnergyTHConstWeight + th * (1 - St.frameEnergyTHConstWeight);
            th = th * th;
            th *= St.overallEnergyTHWeight * St.overallEnergyTHWeight;
            nf.frameEnergyTH = th;
        }
        __syncthreads();
    }
    // refresh thMax of the pairs (the next linearize reads it)
    for (int i = tid; i < F * F; i += NT) {
        int h = i / F, t = i % F;
        B.pairs[i].thMax = fmaxf(B.frames[h].frameEnergyTH, B.frames[t].frameEnergyTH);
    }
    __syncthreads();
}
