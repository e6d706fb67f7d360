// trace.hip — immature-point tracing on the device (gfx950): FullSystem::traceNewCoarse (reference
// src/frontend/FullSystem.cc:1012-1050) = ImmaturePoint::traceOn (src/internal/ImmaturePoint.cc:47-310) for every immature point
// of the window against a new frame, ONE launch.
//
// Mapping: one wavefront per immature point.  The discrete epipolar search is the parallel part: lane l evaluates the 8-pattern
// Huber energy at search steps l and l+64 (numSteps <= 99) - the position of step i is reached with i sequential float additions
// exactly like the reference's `ptx += dx` loop, the 8 pattern terms are summed in pattern order, so every energy is bit-identical
// to the CPU path; the best step (first minimum) and the second-best outside the +-radius window are wave reductions.  The
// short Gauss-Newton refinement (<= 3 iterations of 8 samples) and the scalar bookkeeping run uniformly in all lanes.
// Memory: per point 128 B record in / out + 4-byte taps of the level-0 image along the epipolar line (L2 resident).
#include "trace.h"
#include "lane.h"
#include "group_member.h"

// getInterpolatedElement31 (GlobalFuncs.h:146-159)
static __device__ __forceinline__ float interp31(const float *img, float x, float y, int w) {
    const int ix = (int) x, iy = (int) y;
    const float dx = x - ix, dy = y - iy, dxdy = dx * dy;
    const float *bp = img + 3 * (ix + iy * w);
    return dxdy * bp[3 + 3 * w] + (dy - dxdy) * bp[3 * w] + (dx - dxdy) * bp[3] + (1 - dx - dy + dxdy) * bp[0];
}

// A NaN that an invalid operation (0 / 0, Inf / Inf, Inf - Inf) produces is, in the reference's records, the x86 default NaN 0xFFC00000 (sign bit set), and SSE
// hands it on unchanged; the same operation on the device yields 0x7FC00000.  The three values a point's record can hold such a NaN in - quality and the two ends
// of the new interval - take the reference's bits through this, so that records compare byte for byte.
static __device__ __forceinline__ float x86_default_nan(float x) { return x != x ? __builtin_bit_cast(float, 0xFFC00000u) : x; }

static __device__ __forceinline__ void trace_fail(ldso_immature_t *p, int lane, int status, int *counts) {
    if (lane == 0) { p->lastTraceUV[0] = -1; p->lastTraceUV[1] = -1; p->lastTracePixelInterval = 0; p->lastTraceStatus = status; atomicAdd(&counts[status], 1); }
}

// ImmaturePoint::traceOn of point i of one job by one wavefront (`lane` = its lane; i is wave-uniform).  No LDS and no barrier: the wavefronts of a workgroup are
// independent, which is what lets k_trace_group put wavefronts of different jobs into one workgroup.
static __device__ __forceinline__ void trace_point(const TraceJob &A, int i, int lane) {
    if (i >= A.n) return;
    ldso_immature_t *P = A.pts + i;
    const int hst = P->host;
    if (hst < 0 || hst >= A.nHosts) return;
    const ldso_trace_settings_t &S = A.s;
    const int w = A.w, h = A.h;
    const int prevStatus = P->lastTraceStatus;
    if (prevStatus == LDSO_IPS_OOB) { if (lane == 0) atomicAdd(&A.counts[LDSO_IPS_OOB], 1); return; }     // :53
    const float *KRKi = A.KRKi + 9 * hst, *Kt = A.Kt + 3 * hst, *aff = A.aff + 2 * hst;
    const float pu = P->u, pv = P->v, idmin = P->idepth_min, idmax = P->idepth_max;
    const float maxPixSearch = (w + h) * S.maxPixSearch;
    // ---- project idepth_min / idepth_max (:59-124) ----
    const float pr0 = (KRKi[0] * pu + KRKi[1] * pv) + KRKi[2] * 1.0f, pr1 = (KRKi[3] * pu + KRKi[4] * pv) + KRKi[5] * 1.0f,
                pr2 = (KRKi[6] * pu + KRKi[7] * pv) + KRKi[8] * 1.0f;
    const float m0 = pr0 + Kt[0] * idmin, m1 = pr1 + Kt[1] * idmin, m2 = pr2 + Kt[2] * idmin;
    const float uMin = m0 / m2, vMin = m1 / m2;
    if (!(uMin > 4 && vMin > 4 && uMin < w - 5 && vMin < h - 5)) { trace_fail(P, lane, LDSO_IPS_OOB, A.counts); return; }
    float dist, uMax, vMax;
    const bool finiteMax = isfinite(idmax);
    if (finiteMax) {
        const float x0 = pr0 + Kt[0] * idmax, x1 = pr1 + Kt[1] * idmax, x2 = pr2 + Kt[2] * idmax;
        uMax = x0 / x2; vMax = x1 / x2;
        if (!(uMax > 4 && vMax > 4 && uMax < w - 5 && vMax < h - 5)) { trace_fail(P, lane, LDSO_IPS_OOB, A.counts); return; }
        dist = (uMin - uMax) * (uMin - uMax) + (vMin - vMax) * (vMin - vMax);
        dist = sqrtf(dist);
        if (dist < S.trace_slackInterval) {                                                          // :91-96
            if (lane == 0) { P->lastTraceUV[0] = (uMax + uMin) * 0.5f; P->lastTraceUV[1] = (vMax + vMin) * 0.5f; P->lastTracePixelInterval = dist;
                             P->lastTraceStatus = LDSO_IPS_SKIPPED; atomicAdd(&A.counts[LDSO_IPS_SKIPPED], 1); }
            return;
        }
    } else {
        dist = maxPixSearch;
        const float q0 = pr0 + Kt[0] * 0.01f, q1 = pr1 + Kt[1] * 0.01f, q2 = pr2 + Kt[2] * 0.01f;
        uMax = q0 / q2; vMax = q1 / q2;
        const float ddx = uMax - uMin, ddy = vMax - vMin;
        const float d = 1.0f / sqrtf(ddx * ddx + ddy * ddy);
        uMax = uMin + dist * ddx * d; vMax = vMin + dist * ddy * d;
        if (!(uMax > 4 && vMax > 4 && uMax < w - 5 && vMax < h - 5)) { trace_fail(P, lane, LDSO_IPS_OOB, A.counts); return; }
    }
    if (!(idmin < 0 || (m2 > 0.75f && m2 < 1.5f))) { trace_fail(P, lane, LDSO_IPS_OOB, A.counts); return; }      // :127-131
    // ---- error bound in pixels (:134-147) ----
    float dx = S.trace_stepsize * (uMax - uMin), dy = S.trace_stepsize * (vMax - vMin);
    const float g0 = P->gradH[0], g1 = P->gradH[1], g2 = P->gradH[2], g3 = P->gradH[3];
    const float a = (dx * g0 + dy * g2) * dx + (dx * g1 + dy * g3) * dy;
    const float b = (dy * g0 + -dx * g2) * dy + (dy * g1 + -dx * g3) * -dx;
    float errorInPixel = 0.2f + 0.2f * (a + b) / a;
    // a NaN handed in through gradH reaches errorInPixel with its own bits, quieted (SSE returns the NaN operand; g0, g2, g1, g3 is the order they enter `a`);
    // any other NaN here is 0 / 0 where gradH is zero along the line
    if (errorInPixel != errorInPixel) {
        const float gn = g0 != g0 ? g0 : g2 != g2 ? g2 : g1 != g1 ? g1 : g3;
        errorInPixel = gn != gn ? __builtin_bit_cast(float, __builtin_bit_cast(unsigned, gn) | 0x00400000u) : x86_default_nan(errorInPixel);
    }
    if (errorInPixel * S.trace_minImprovementFactor > dist && finiteMax) {
        if (lane == 0) { P->lastTraceUV[0] = (uMax + uMin) * 0.5f; P->lastTraceUV[1] = (vMax + vMin) * 0.5f; P->lastTracePixelInterval = dist;
                         P->lastTraceStatus = LDSO_IPS_BADCONDITION; atomicAdd(&A.counts[LDSO_IPS_BADCONDITION], 1); }
        return;
    }
    if (errorInPixel > 10) errorInPixel = 10;
    // ---- discrete search (:150-205), lanes = steps ----
    dx /= dist; dy /= dist;
    if (dist > maxPixSearch) { uMax = uMin + maxPixSearch * dx; vMax = vMin + maxPixSearch * dy; dist = maxPixSearch; }
    int numSteps = (int) (1.9999f + dist / S.trace_stepsize);
    const float randShift = uMin * 1000 - floorf(uMin * 1000);
    const float ptx0 = uMin - randShift * dx, pty0 = vMin - randShift * dy;
    float rx[8], ry[8], col[8];
    {
        const int ox[8] = {0, -1, 1, -2, 0, 2, -1, 0}, oy[8] = {-2, -1, -1, 0, 0, 0, 1, 2};           // staticPattern[8], Setting.cc:221
#pragma unroll
        for (int k = 0; k < 8; k++) { rx[k] = KRKi[0] * ox[k] + KRKi[1] * oy[k]; ry[k] = KRKi[3] * ox[k] + KRKi[4] * oy[k]; col[k] = P->color[k]; }
    }
    if (!isfinite(dx) || !isfinite(dy)) { trace_fail(P, lane, LDSO_IPS_OOB, A.counts); return; }
    if (numSteps >= 100) numSteps = 99;
    const float aff0 = aff[0], aff1 = aff[1];
    float e[2], px[2], py[2];
    {
        // position of step `lane`, then 64 more additions for step lane + 64 (sequential float accumulation as in the reference loop)
        float x = ptx0, y = pty0;
        for (int j = 0; j < 63; j++) if (j < lane) { x += dx; y += dy; }
        px[0] = x; py[0] = y;
        for (int j = 0; j < 64; j++) { x += dx; y += dy; }
        px[1] = x; py[1] = y;
    }
#pragma unroll
    for (int pass = 0; pass < 2; pass++) {
        const int si = lane + 64 * pass;
        float energy = 0;
        if (si < numSteps) {
            float hit[8];
#pragma unroll
            for (int k = 0; k < 8; k++) hit[k] = interp31(A.img, px[pass] + rx[k], py[pass] + ry[k], w);
#pragma unroll
            for (int k = 0; k < 8; k++) {
                if (!isfinite(hit[k])) { energy += 1e5f; continue; }
                const float r = hit[k] - (float) (aff0 * col[k] + aff1);
                const float hw = fabsf(r) < S.huberTH ? 1 : S.huberTH / fabsf(r);
                energy += hw * r * r * (2 - hw);
            }
        }
        e[pass] = energy;
    }
    // best step: first minimum below 1e10 (strict < in index order)
    float bE; int bI;
    {
        const bool v0 = lane < numSteps && e[0] < 1e10f, v1 = lane + 64 < numSteps && e[1] < 1e10f;
        bE = v0 ? e[0] : 3e38f; bI = v0 ? lane : 1 << 20;
        if (v1 && e[1] < bE) { bE = e[1]; bI = lane + 64; }
        for (int o = 32; o > 0; o >>= 1) {
            const float e2 = __shfl_xor(bE, o, 64); const int i2 = __shfl_xor(bI, o, 64);
            if (e2 < bE || (e2 == bE && i2 < bI)) { bE = e2; bI = i2; }
        }
    }
    float bestU = 0, bestV = 0, bestEnergy = 1e10f;
    int bestIdx = -1;
    if (bI < (1 << 20)) {
        bestIdx = bI; bestEnergy = bE;
        const float sx = (bI >= 64) ? px[1] : px[0], sy = (bI >= 64) ? py[1] : py[0];
        bestU = __shfl(sx, bI & 63, 64); bestV = __shfl(sy, bI & 63, 64);
    }
    float secondBest = 1e10f;                                                                        // :208-215
    {
        float sb = 1e10f;
#pragma unroll
        for (int pass = 0; pass < 2; pass++) {
            const int si = lane + 64 * pass;
            if (si < numSteps && (si < bestIdx - S.minTraceTestRadius || si > bestIdx + S.minTraceTestRadius) && e[pass] < sb) sb = e[pass];
        }
        for (int o = 32; o > 0; o >>= 1) sb = fminf(sb, __shfl_xor(sb, o, 64));
        secondBest = sb;
    }
    float quality = P->quality;
    const float newQuality = x86_default_nan(secondBest / bestEnergy);      // neither operand is ever NaN: 0 / 0 where every step matches exactly
    if (newQuality < quality || numSteps > 10) quality = newQuality;
    // ---- Gauss-Newton refinement along the line (:218-268), uniform in all lanes ----
    float uBak = bestU, vBak = bestV, gnstepsize = 1, stepBack = 0;
    if (S.trace_GNIterations > 0) bestEnergy = 1e5f;
    float wgt[8];
#pragma unroll
    for (int k = 0; k < 8; k++) wgt[k] = P->weights[k];
    for (int it = 0; it < S.trace_GNIterations && bestIdx >= 0; it++) {
        float H = 1, bb = 0, energy = 0;
        float h0[8], h1[8], h2[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const float x = bestU + rx[k], y = bestV + ry[k];
            const int ix = (int) x, iy = (int) y;
            const float fx = x - ix, fy = y - iy, fxy = fx * fy;
            const float *bp = A.img + 3 * (ix + iy * w);
            const float w11 = fxy, w01 = fy - fxy, w10 = fx - fxy, w00 = 1 - fx - fy + fxy;
            h0[k] = w11 * bp[3 + 3 * w] + w01 * bp[3 * w] + w10 * bp[3] + w00 * bp[0];
            h1[k] = w11 * bp[4 + 3 * w] + w01 * bp[3 * w + 1] + w10 * bp[4] + w00 * bp[1];
            h2[k] = w11 * bp[5 + 3 * w] + w01 * bp[3 * w + 2] + w10 * bp[5] + w00 * bp[2];
        }
#pragma unroll
        for (int k = 0; k < 8; k++) {
            if (!isfinite(h0[k])) { energy += 1e5f; continue; }
            const float r = h0[k] - (aff0 * col[k] + aff1);
            const float dResdDist = dx * h1[k] + dy * h2[k];
            const float hw = fabsf(r) < S.huberTH ? 1 : S.huberTH / fabsf(r);
            H += hw * dResdDist * dResdDist;
            bb += hw * r * dResdDist;
            energy += wgt[k] * wgt[k] * hw * r * r * (2 - hw);
        }
        if (energy > bestEnergy) {
            stepBack *= 0.5f;
            bestU = uBak + stepBack * dx; bestV = vBak + stepBack * dy;
        } else {
            float step = -gnstepsize * bb / H;
            if (step < -0.5f) step = -0.5f; else if (step > 0.5f) step = 0.5f;
            if (!isfinite(step)) step = 0;
            uBak = bestU; vBak = bestV; stepBack = step;
            bestU += step * dx; bestV += step * dy;
            bestEnergy = energy;
        }
        if (fabsf(stepBack) < S.trace_GNThreshold) break;
    }
    if (lane == 0) P->quality = quality;
    // ---- energy-based outlier (:271-278) ----
    // bestIdx < 0 (no step below 1e10: a non-finite colour or affine value makes every energy NaN): the loop above read nothing, and the point ends here whatever
    // energyTH is - the reference samples around (0, 0), in front of the image, and ends here too unless that memory happens to match (tracer)
    if (bestIdx < 0 || !(bestEnergy < P->energyTH * S.trace_extraSlackOnTH)) {
        trace_fail(P, lane, prevStatus == LDSO_IPS_OUTLIER ? LDSO_IPS_OOB : LDSO_IPS_OUTLIER, A.counts);
        return;
    }
    // ---- new interval (:281-300) ----
    float nmin, nmax;
    if (dx * dx > dy * dy) {
        nmin = (pr2 * (bestU - errorInPixel * dx) - pr0) / (Kt[0] - Kt[2] * (bestU - errorInPixel * dx));
        nmax = (pr2 * (bestU + errorInPixel * dx) - pr0) / (Kt[0] - Kt[2] * (bestU + errorInPixel * dx));
    } else {
        nmin = (pr2 * (bestV - errorInPixel * dy) - pr1) / (Kt[1] - Kt[2] * (bestV - errorInPixel * dy));
        nmax = (pr2 * (bestV + errorInPixel * dy) - pr1) / (Kt[1] - Kt[2] * (bestV + errorInPixel * dy));
    }
    if (nmin > nmax) { const float t = nmin; nmin = nmax; nmax = t; }
    // a NaN errorInPixel passes through every operation above as it is; any other NaN here was made by an invalid operation
    if (errorInPixel != errorInPixel) { nmin = errorInPixel; nmax = errorInPixel; } else { nmin = x86_default_nan(nmin); nmax = x86_default_nan(nmax); }
    if (lane == 0) { P->idepth_min = nmin; P->idepth_max = nmax; }
    if (!isfinite(nmin) || !isfinite(nmax) || (nmax < 0)) { trace_fail(P, lane, LDSO_IPS_OUTLIER, A.counts); return; }
    if (lane == 0) {
        P->lastTracePixelInterval = 2 * errorInPixel;
        P->lastTraceUV[0] = bestU; P->lastTraceUV[1] = bestV;
        P->lastTraceStatus = LDSO_IPS_GOOD;
        atomicAdd(&A.counts[LDSO_IPS_GOOD], 1);
    }
}

__global__ __launch_bounds__(256) void k_trace_on(TraceJob A) {
    const int lane = threadIdx.x & 63;
    const int i = __builtin_amdgcn_readfirstlane((int) ((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    trace_point(A, i, lane);
}

// a row of the job table as the kernel reads it: TraceJob with its pointers typed as device memory (group_member.h: LD_GLOBAL)
struct TraceJobDev {
    LD_GLOBAL ldso_immature_t *pts;
    int n;
    LD_GLOBAL const float *img;
    int w, h;
    LD_GLOBAL const float *KRKi, *Kt, *aff;
    int nHosts;
    ldso_trace_settings_t s;
    LD_GLOBAL int *counts;
};
static_assert(sizeof(TraceJobDev) == sizeof(TraceJob) && offsetof(TraceJobDev, counts) == offsetof(TraceJob, counts) && offsetof(TraceJobDev, s) == offsetof(TraceJob, s) &&
              offsetof(TraceJobDev, aff) == offsetof(TraceJob, aff), "TraceJobDev is TraceJob");

// The traces of a group of tracers in one launch (ldso_trace_group_*, trace_group.hip): one wavefront per point, the points of all jobs packed wave-granular, so a
// workgroup may hold wavefronts of several jobs (trace_point has no LDS and no barrier).  first[j] = the wavefronts in front of job j, first[nJobs] = all of them; the
// wavefront finds its job with group_member_of.  Wave index and job index are wave-uniform (readfirstlane), and the job is copied before the first store of the
// kernel: its pointers and settings are fetched with scalar loads and stay in scalar registers, as the by-value argument of k_trace_on does.
__global__ __launch_bounds__(256) void k_trace_group(const TraceJob *__restrict__ jobs, const int *__restrict__ first, int nJobs) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int) ((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    if (wave >= first[nJobs]) return;
    const int j = __builtin_amdgcn_readfirstlane(group_member_of(first, nJobs, wave));
    const int i = __builtin_amdgcn_readfirstlane(wave - first[j]);
    const TraceJobDev D = ((const TraceJobDev *) jobs)[j];
    TraceJob A;
    A.pts = (ldso_immature_t *) D.pts; A.n = D.n; A.img = (const float *) D.img; A.w = D.w; A.h = D.h;
    A.KRKi = (const float *) D.KRKi; A.Kt = (const float *) D.Kt; A.aff = (const float *) D.aff; A.nHosts = D.nHosts; A.s = D.s; A.counts = (int *) D.counts;
    trace_point(A, i, lane);
}

hipError_t trace_launch_group(const TraceJob *d_jobs, const int *d_first, int nJobs, int totalWaves, hipStream_t st) {
    hipLaunchKernelGGL(k_trace_group, dim3((totalWaves + 3) / 4), dim3(256), 0, st, d_jobs, d_first, nJobs);
    return hipGetLastError();
}


// ---------------------------------------------------------------------------------------------------------
// Stable compaction of the resident set (what leaves it: points the selection dropped or activated, FullSystem.cc:1105-1188; points of a marginalised host
// frame, FullSystem.cc:602-645).  Record i survives iff its keep flag is set and its host maps to a frame of the new window; survivors keep their relative order
// (the reference's iteration order, FullSystem.cc:1088-1098: the greedy selection depends on it) and move OUT OF PLACE into the tracer's second buffer.
//   k_compact_count  one flag per record, one count per workgroup of 256 records
//   k_compact_move   every workgroup sums the counts in front of it (<= max_points / 256 words), ranks its own records, then moves them: 8 lanes x 16 B per
//                    128-byte record, the lane that holds `host` rewrites it
// CompactArgs (trace.h) is one compaction; the bodies are device functions of (job, block, blocks of the job), shared with the grouped kernels below.
// ---------------------------------------------------------------------------------------------------------
// the body of k_compact_count for workgroup `block` of the nBlocks that serve A
static __device__ __forceinline__ void compact_count(const CompactArgs &A, int block, int nBlocks) {
    __shared__ int s_cnt[CMP_THREADS / 64];
    (void) nBlocks;
    const int i = block * CMP_THREADS + threadIdx.x;
    bool keep = false;
    if (i < A.n) {
        const int host = A.src[i].host;
        keep = A.keep8 ? A.keep8[i] != 0 : A.keep32 ? A.keep32[i] == A.keepValue : true;
        keep = keep && host >= 0 && host < A.nHosts && (!A.hostMap || A.hostMap[host] >= 0);       // a host outside the window: dropped, not dereferenced
        A.flag[i] = keep ? 1 : 0;
    }
    const int c = __popcll(__ballot(keep));
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) A.blockCount[block] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

// the body of k_compact_move for workgroup `block` of the nBlocks that serve A
static __device__ __forceinline__ void compact_move(const CompactArgs &A, int block, int nBlocks) {
    __shared__ int s_part[2][CMP_THREADS / 64], s_wave[CMP_THREADS / 64], s_dest[CMP_THREADS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // the workgroups in front of this one, and all of them
    int before = 0, total = 0;
    for (int j = tid; j < nBlocks; j += CMP_THREADS) { const int c = A.blockCount[j]; total += c; if (j < block) before += c; }
    before = wave_sum(before); total = wave_sum(total);
    const int i = block * CMP_THREADS + tid;
    const bool keep = i < A.n && A.flag[i] != 0;
    const unsigned long long bm = __ballot(keep);
    if (lane == 0) { s_part[0][wave] = before; s_part[1][wave] = total; s_wave[wave] = __popcll(bm); }
    __syncthreads();
    before = s_part[0][0] + s_part[0][1] + s_part[0][2] + s_part[0][3];
    total = s_part[1][0] + s_part[1][1] + s_part[1][2] + s_part[1][3];
    if (block == 0 && tid == 0) *A.nOut = total;
    int rank = before + __popcll(bm & ((1ull << lane) - 1ull));
    for (int wv = 0; wv < wave; wv++) rank += s_wave[wv];
    s_dest[tid] = keep ? rank : -1;
    if (keep) A.dstType[rank] = A.srcType[i];
    __syncthreads();
    const int part = tid & 7;
    static_assert(sizeof(ldso_immature_t) == 128 && offsetof(ldso_immature_t, host) == 120, "a record is eight 16-byte parts, host is dword 2 of the last");
    for (int r = tid >> 3; r < CMP_THREADS; r += CMP_THREADS / 8) {
        const int d = s_dest[r];
        if (d < 0) continue;                       // covers r beyond n: s_dest is -1 there
        uint4 q = ((const uint4 *) (A.src + block * CMP_THREADS + r))[part];
        if (part == 7 && A.hostMap) q.z = (unsigned) A.hostMap[(int) q.z];            // the count pass kept only hosts in [0, nHosts)
        ((uint4 *) (A.dst + d))[part] = q;
    }
}

__global__ __launch_bounds__(CMP_THREADS) void k_compact_count(CompactArgs A) { compact_count(A, (int) blockIdx.x, (int) gridDim.x); }
__global__ __launch_bounds__(CMP_THREADS) void k_compact_move(CompactArgs A) { compact_move(A, (int) blockIdx.x, (int) gridDim.x); }

// a row of the compaction table as the kernels read it: CompactArgs with its pointers typed as device memory (group_member.h: LD_GLOBAL)
struct CompactArgsDev {
    LD_GLOBAL const ldso_immature_t *src; LD_GLOBAL ldso_immature_t *dst;
    LD_GLOBAL const float *srcType; LD_GLOBAL float *dstType;
    int n, nHosts;
    LD_GLOBAL const unsigned char *keep8;
    LD_GLOBAL const int32_t *keep32;
    int keepValue;
    LD_GLOBAL const int32_t *hostMap;
    LD_GLOBAL unsigned char *flag;
    LD_GLOBAL int32_t *blockCount;
    LD_GLOBAL int32_t *nOut;
};
static_assert(sizeof(CompactArgsDev) == sizeof(CompactArgs) && offsetof(CompactArgsDev, n) == offsetof(CompactArgs, n) && offsetof(CompactArgsDev, keep8) == offsetof(CompactArgs, keep8) &&
              offsetof(CompactArgsDev, keepValue) == offsetof(CompactArgs, keepValue) && offsetof(CompactArgsDev, nOut) == offsetof(CompactArgs, nOut), "CompactArgsDev is CompactArgs");

// The compactions of many tracers in two launches (ldso_trace_group_compact, trace_group.hip; ldso_ba_batch_select_activate_tracers, act_select.hip): first[j] = the
// workgroups in front of job j, first[nJobs] = the grid.  Workgroup u serves the job group_member_of finds as that job's block u - first[j] of first[j + 1] - first[j]:
// the same body on the same bytes as the job's own k_compact_count / k_compact_move.  A job without records has no workgroup.  Job index and block are uniform
// (blockIdx), and the row is copied before the first store of the kernel, so its pointers stay in scalar registers.
static __device__ __forceinline__ CompactArgs compact_job_of(const CompactArgs *jobs, const int *first, int nJobs, int &block, int &nBlocks) {
    const int u = (int) blockIdx.x;
    const int j = group_member_of(first, nJobs, u);
    const int f0 = first[j];
    block = u - f0; nBlocks = first[j + 1] - f0;
    const CompactArgsDev D = ((const CompactArgsDev *) jobs)[j];
    CompactArgs A;
    A.src = (const ldso_immature_t *) D.src; A.dst = (ldso_immature_t *) D.dst; A.srcType = (const float *) D.srcType; A.dstType = (float *) D.dstType; A.n = D.n; A.nHosts = D.nHosts;
    A.keep8 = (const unsigned char *) D.keep8; A.keep32 = (const int32_t *) D.keep32; A.keepValue = D.keepValue; A.hostMap = (const int32_t *) D.hostMap;
    A.flag = (unsigned char *) D.flag; A.blockCount = (int32_t *) D.blockCount; A.nOut = (int32_t *) D.nOut;
    return A;
}

__global__ __launch_bounds__(CMP_THREADS) void k_compact_count_group(const CompactArgs *__restrict__ jobs, const int *__restrict__ first, int nJobs) {
    int block, nBlocks;
    const CompactArgs A = compact_job_of(jobs, first, nJobs, block, nBlocks);
    compact_count(A, block, nBlocks);
}

__global__ __launch_bounds__(CMP_THREADS) void k_compact_move_group(const CompactArgs *__restrict__ jobs, const int *__restrict__ first, int nJobs) {
    int block, nBlocks;
    const CompactArgs A = compact_job_of(jobs, first, nJobs, block, nBlocks);
    compact_move(A, block, nBlocks);
}

hipError_t trace_launch_compact_group(const CompactArgs *d_jobs, const int *d_first, int nJobs, int totalBlocks, hipStream_t st) {
    hipLaunchKernelGGL(k_compact_count_group, dim3(totalBlocks), dim3(CMP_THREADS), 0, st, d_jobs, d_first, nJobs);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_compact_move_group, dim3(totalBlocks), dim3(CMP_THREADS), 0, st, d_jobs, d_first, nJobs);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------

static constexpr int TYPE_ONE = 0x3f800000;      // 1.0f as the word hipMemsetD32Async writes

// The compaction on stream `st` (the tracer's own, or the stream of the BA handle whose selection produced keep32: the tracer is idle then).  The host map, when
// there is one, lies in d_cmp already.  Nothing of the tracer's host state changes until trace_compact_finish, which the caller runs behind its synchronisation.
CompactArgs trace_compact_job(const ldso_tracer *T, const unsigned char *d_keep8, const int32_t *d_keep32, int keepValue, int n_hosts, const int32_t *d_hostMap, int32_t *d_nOut) {
    CompactArgs A;
    memset(&A, 0, sizeof(A));          // a row of a table crosses PCIe: every byte set
    A.src = T->d_pts; A.dst = T->d_alt; A.srcType = T->d_type; A.dstType = T->d_typeAlt; A.n = T->n; A.nHosts = n_hosts;
    A.keep8 = d_keep8; A.keep32 = d_keep32; A.keepValue = keepValue; A.hostMap = d_hostMap;
    A.flag = T->d_flag; A.nOut = d_nOut; A.blockCount = T->d_cmp + LDSO_MAX_FRAMES + 4;
    return A;
}

int trace_compact_enqueue(ldso_tracer *T, const unsigned char *d_keep8, const int32_t *d_keep32, int keepValue, int n_hosts, bool haveMap, hipStream_t st) {
    T->nAfterCompact = T->n;
    if (T->n <= 0) return LDSO_OK;
    const CompactArgs A = trace_compact_job(T, d_keep8, d_keep32, keepValue, n_hosts, haveMap ? T->d_cmp : nullptr, T->d_cmp + LDSO_MAX_FRAMES);
    const int blocks = compact_blocks(T->n);
    hipLaunchKernelGGL(k_compact_count, dim3(blocks), dim3(CMP_THREADS), 0, st, A);
    CHK(hipGetLastError());
    hipLaunchKernelGGL(k_compact_move, dim3(blocks), dim3(CMP_THREADS), 0, st, A);
    CHK(hipGetLastError());
    CHK(hipMemcpyAsync(&T->nAfterCompact, A.nOut, 4, hipMemcpyDeviceToHost, st));
    return LDSO_OK;
}

void trace_compact_finish(ldso_tracer *T) {
    if (T->n <= 0) return;
    std::swap(T->d_pts, T->d_alt); std::swap(T->d_type, T->d_typeAlt);
    T->n = std::min(std::max(T->nAfterCompact, 0), T->n);
}

void trace_compact_finish_group(ldso_tracer *T, int nOut) { T->nAfterCompact = nOut; trace_compact_finish(T); }

extern "C" {

int ldso_trace_settings_default(ldso_trace_settings_t *s) {
    if (!s) return LDSO_E_INVALID;
    memset(s, 0, sizeof(*s));
    s->maxPixSearch = 0.027f; s->trace_stepsize = 1.0f; s->trace_GNThreshold = 0.1f; s->trace_extraSlackOnTH = 1.2f;
    s->trace_slackInterval = 1.5f; s->trace_minImprovementFactor = 2; s->huberTH = 9; s->trace_GNIterations = 3; s->minTraceTestRadius = 2;
    return LDSO_OK;
}

static int trace_create_body(ldso_tracer *T, int device, int w, int h, int max_points) {
    T->device = device; T->w = w; T->h = h; T->maxPoints = max_points;
    ldso_trace_settings_default(&T->settings);
    CHK(hipStreamCreateWithFlags(&T->stream, hipStreamNonBlocking));
    T->ownStream = true;
    CHK(hipMalloc(&T->d_pts, (size_t) max_points * sizeof(ldso_immature_t))); CHK(hipMalloc(&T->d_alt, (size_t) max_points * sizeof(ldso_immature_t)));
    CHK(hipMalloc(&T->d_type, (size_t) max_points * 4)); CHK(hipMalloc(&T->d_typeAlt, (size_t) max_points * 4));
    CHK(hipMalloc(&T->d_keep, (size_t) max_points)); CHK(hipMalloc(&T->d_flag, (size_t) max_points));
    CHK(hipMalloc(&T->d_cmp, (size_t) (LDSO_MAX_FRAMES + 4 + (max_points + CMP_THREADS - 1) / CMP_THREADS) * 4));
    CHK(hipMalloc(&T->d_img, (size_t) w * h * 12));
    CHK(hipMalloc(&T->d_color, (size_t) w * h * 4));
    CHK(hipMalloc(&T->d_pose, (size_t) LDSO_MAX_FRAMES * 14 * 4));
    CHK(hipMalloc(&T->d_counts, 8 * 4));
    return LDSO_OK;
}

int ldso_trace_create(int device, int w, int h, int max_points, ldso_tracer_t **out) {
    REQ(out && w > 16 && h > 16 && max_points > 0, "ldso_trace_create: bad arguments");
    RUN(open_device(device, "ldso_trace_create"));
    ldso_tracer *T = new ldso_tracer();
    return finish_create(trace_create_body(T, device, w, h, max_points), T, out, ldso_trace_destroy);      // nothing of a half-built handle leaks
}

int ldso_trace_destroy(ldso_tracer_t *T) {
    if (!T) return LDSO_OK;
    REQ(T->inGroup == nullptr, "ldso_trace_destroy: the tracer is a member of a live group (ldso_trace_group_destroy first: the group dereferences its members)");
    hipSetDevice(T->device);
    hipDeviceSynchronize();
    hipFree(T->d_pts); hipFree(T->d_alt); hipFree(T->d_type); hipFree(T->d_typeAlt); hipFree(T->d_keep); hipFree(T->d_flag); hipFree(T->d_cmp); hipFree(T->d_img); hipFree(T->d_color); hipFree(T->d_pose); hipFree(T->d_counts);
    if (T->stream && T->ownStream) hipStreamDestroy(T->stream);
    delete T;
    return LDSO_OK;
}

// The caller's stream instead of the tracer's own (NULL: an own one again).  The wait that ldso_trace_set_frame_pyramid queued for the frame's build stands on the
// OLD stream, so the tracer holds no frame afterwards: set it again.
int ldso_trace_set_stream(ldso_tracer_t *T, void *s) {
    REQ(T, "ldso_trace_set_stream: null handle");
    CHK(hipSetDevice(T->device));
    RUN(swap_stream(T->stream, T->ownStream, s));
    T->haveFrame = false;
    return LDSO_OK;
}

int ldso_trace_set_settings(ldso_tracer_t *T, const ldso_trace_settings_t *s) {
    REQ(T && s, "null argument");
    REQ(s->trace_GNIterations >= 0 && s->trace_stepsize > 0 && s->minTraceTestRadius >= 0, "ldso_trace_set_settings: bad values");
    T->settings = *s;
    return LDSO_OK;
}

int ldso_trace_set_points(ldso_tracer_t *T, int n, const ldso_immature_t *pts) {
    REQ(T && n >= 0 && n <= T->maxPoints && (n == 0 || pts), "ldso_trace_set_points: bad arguments");
    CHK(hipSetDevice(T->device));
    if (n) CHK(hipMemcpyAsync(T->d_pts, pts, (size_t) n * sizeof(ldso_immature_t), hipMemcpyHostToDevice, T->stream));
    if (n) CHK(hipMemsetD32Async((hipDeviceptr_t) T->d_type, TYPE_ONE, (size_t) n, T->stream));
    CHK(hipStreamSynchronize(T->stream));
    T->n = n;
    return LDSO_OK;
}

int ldso_trace_set_point_types(ldso_tracer_t *T, const float *my_type) {
    REQ(T && (T->n == 0 || my_type), "ldso_trace_set_point_types: bad arguments");
    CHK(hipSetDevice(T->device));
    if (T->n) CHK(hipMemcpyAsync(T->d_type, my_type, (size_t) T->n * 4, hipMemcpyHostToDevice, T->stream));
    CHK(hipStreamSynchronize(T->stream));
    return LDSO_OK;
}

int ldso_trace_get_point_types(ldso_tracer_t *T, float *out) {
    REQ(T && (T->n == 0 || out), "ldso_trace_get_point_types: bad arguments");
    CHK(hipSetDevice(T->device));
    if (T->n) CHK(hipMemcpyAsync(out, T->d_type, (size_t) T->n * 4, hipMemcpyDeviceToHost, T->stream));
    CHK(hipStreamSynchronize(T->stream));
    return LDSO_OK;
}

int ldso_trace_compact(ldso_tracer_t *T, const uint8_t *keep, int n_hosts, const int32_t *host_map, int *n_out) {
    REQ(T && n_hosts >= 1 && n_hosts <= LDSO_MAX_FRAMES, "ldso_trace_compact: bad arguments");
    for (int f = 0; host_map && f < n_hosts; f++) REQ(host_map[f] < LDSO_MAX_FRAMES, "ldso_trace_compact: a host maps beyond LDSO_MAX_FRAMES");
    CHK(hipSetDevice(T->device));
    if (T->n > 0) {
        if (keep) CHK(hipMemcpyAsync(T->d_keep, keep, (size_t) T->n, hipMemcpyHostToDevice, T->stream));
        if (host_map) CHK(hipMemcpyAsync(T->d_cmp, host_map, (size_t) n_hosts * 4, hipMemcpyHostToDevice, T->stream));
        RUN(trace_compact_enqueue(T, keep ? T->d_keep : nullptr, nullptr, 0, n_hosts, host_map != nullptr, T->stream));
        CHK(hipStreamSynchronize(T->stream));          // the call's one synchronisation: the count is behind it
        trace_compact_finish(T);
    }
    if (n_out) *n_out = T->n;
    return LDSO_OK;
}

// fresh immature points straight from the device (ldso_feat_device): appended behind the resident ones, stream-ordered behind the caller's work on `immature_dev`
// only through the synchronisation its producer ended with (ldso_feat_detect synchronises before it returns)
int ldso_trace_append_points_device(ldso_tracer_t *T, int n, const void *immature_dev) {
    REQ(T && n >= 0 && (n == 0 || immature_dev), "ldso_trace_append_points_device: bad arguments");
    REQ(n <= T->maxPoints - T->n, "ldso_trace_append_points_device: more points than max_points");
    CHK(hipSetDevice(T->device));
    if (n) CHK(hipMemcpyAsync(T->d_pts + T->n, immature_dev, (size_t) n * sizeof(ldso_immature_t), hipMemcpyDeviceToDevice, T->stream));
    if (n) CHK(hipMemsetD32Async((hipDeviceptr_t) (T->d_type + T->n), TYPE_ONE, (size_t) n, T->stream));      // my_type = 1 (FullSystem.cc:1281)
    CHK(hipStreamSynchronize(T->stream));
    T->n += n;
    return LDSO_OK;
}

// my_type of the last n records from device memory (ldso_pixsel_device): the points of setting_pointSelection == 0 carry their map value (FullSystem.cc:1297)
int ldso_trace_set_tail_types_device(ldso_tracer_t *T, int n, const void *type_dev) {
    REQ(T && n >= 0 && n <= T->n && (n == 0 || type_dev), "ldso_trace_set_tail_types_device: bad arguments");
    CHK(hipSetDevice(T->device));
    if (n) CHK(hipMemcpyAsync(T->d_type + (T->n - n), type_dev, (size_t) n * sizeof(float), hipMemcpyDeviceToDevice, T->stream));
    CHK(hipStreamSynchronize(T->stream));
    return LDSO_OK;
}

int ldso_trace_get_points(ldso_tracer_t *T, ldso_immature_t *out) {
    REQ(T && (T->n == 0 || out), "ldso_trace_get_points: bad arguments");
    CHK(hipSetDevice(T->device));
    if (T->n) CHK(hipMemcpyAsync(out, T->d_pts, (size_t) T->n * sizeof(ldso_immature_t), hipMemcpyDeviceToHost, T->stream));
    CHK(hipStreamSynchronize(T->stream));
    return LDSO_OK;
}

int ldso_trace_set_frame(ldso_tracer_t *T, const float *dI) {
    REQ(T && dI, "ldso_trace_set_frame: bad arguments");
    CHK(hipSetDevice(T->device));
    CHK(hipMemcpyAsync(T->d_img, dI, (size_t) T->w * T->h * 12, hipMemcpyHostToDevice, T->stream));
    CHK(hipStreamSynchronize(T->stream));
    T->haveFrame = true; T->img = T->d_img;
    return LDSO_OK;
}

int ldso_trace_set_frame_raw(ldso_tracer_t *T, const float *irradiance) {
    REQ(T && irradiance, "ldso_trace_set_frame_raw: bad arguments");
    CHK(hipSetDevice(T->device));
    float *lv[1] = {T->d_img};
    RUN(raw_to_images(T->d_color, irradiance, T->w, T->h, 1, lv, T->stream));
    CHK(hipStreamSynchronize(T->stream));
    T->haveFrame = true; T->img = T->d_img;
    return LDSO_OK;
}

// the new frame as a resident ldso_pyramid_t (zero-copy: ImmaturePoint::traceOn samples frame->dI = level 0)
int ldso_trace_set_frame_pyramid(ldso_tracer_t *T, ldso_pyramid_t *pyr) {
    REQ(T && pyr, "ldso_trace_set_frame_pyramid: bad arguments");
    RUN(pyramid_wait(pyr, T->device, T->w, T->h, 1, T->stream, "ldso_trace_set_frame_pyramid", "the tracer (device, size)"));
    T->haveFrame = true; T->img = pyr->lv[0];
    return LDSO_OK;
}

int ldso_trace_on(ldso_tracer_t *T, int n_hosts, const float *KRKi, const float *Kt, const float *aff, int *counts_out) {
    REQ(T && n_hosts > 0 && n_hosts <= LDSO_MAX_FRAMES && KRKi && Kt && aff, "ldso_trace_on: bad arguments");
    REQ(T->haveFrame, "ldso_trace_on: set the new frame first");
    CHK(hipSetDevice(T->device));
    std::vector<float> pose((size_t) n_hosts * 14);
    memcpy(pose.data(), KRKi, (size_t) n_hosts * 9 * 4);
    memcpy(pose.data() + n_hosts * 9, Kt, (size_t) n_hosts * 3 * 4);
    memcpy(pose.data() + n_hosts * 12, aff, (size_t) n_hosts * 2 * 4);
    CHK(hipMemcpyAsync(T->d_pose, pose.data(), pose.size() * 4, hipMemcpyHostToDevice, T->stream));
    CHK(hipMemsetAsync(T->d_counts, 0, 8 * 4, T->stream));
    if (T->n > 0) {
        TraceJob A;
        A.pts = T->d_pts; A.n = T->n; A.img = T->img; A.w = T->w; A.h = T->h;
        A.KRKi = T->d_pose; A.Kt = T->d_pose + n_hosts * 9; A.aff = T->d_pose + n_hosts * 12; A.nHosts = n_hosts;
        A.s = T->settings; A.counts = T->d_counts;
        const int waves = T->n, blocks = (waves + 3) / 4;
        hipLaunchKernelGGL(k_trace_on, dim3(blocks), dim3(256), 0, T->stream, A);
        CHK(hipGetLastError());
    }
    int c[8] = {0};
    CHK(hipMemcpyAsync(c, T->d_counts, 8 * 4, hipMemcpyDeviceToHost, T->stream));
    CHK(hipStreamSynchronize(T->stream));
    if (counts_out) for (int i = 0; i < 6; i++) counts_out[i] = c[i];
    return LDSO_OK;
}

}  // extern "C"
