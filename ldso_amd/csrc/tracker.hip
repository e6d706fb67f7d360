// tracker.hip — CoarseTracker direct image alignment on gfx950 (reference src/frontend/CoarseTracker.cc): the kernels of the LM loop.
//
//   calcRes + calcGSSSE   CoarseTracker.cc:440-632   tr_eval(): ONE fused pass — projection, bilinear Vec3f gather,
//                                                    Huber, energy, flow indicators and the 9x9 weighted outer
//                                                    product; the warped buffers are never materialised
//   trackNewestCoarse     CoarseTracker.cc:61-217    k_tr_track: the whole coarse-to-fine LM loop runs inside one
//                                                    persistent workgroup per motion hypothesis (no host sync, no
//                                                    launch per iteration); the 8x8 LDLT, SE3::exp and the
//                                                    accept/reject logic run on the device in fp64.
// The per-level point clouds are tiny (10^3..10^4 points): the path is latency bound, so the design minimises
// dependent launches, and batches hypotheses across workgroups (FullSystem::trackNewCoarse tries up to 83).
// makeCoarseDepthL0 is tracker_ref.hip, makeK and the rest of the host side tracker_api.hip; tr_eval, the solvers and the three kernels stay in
// ONE file: they share inlined device functions, the out-of-line solvers and the TR_QROW / TR_QCOL tables.
#include "tracker.h"
#include "lie_dev.h"

// ---------------------------------------------------------------------------------------------------------
// fused calcRes + calcGSSSE over one level by one workgroup; results in LDS `out` (doubles):
//   [0] E  [1] numTermsInE  [2] sumSquaredShiftT  [3] sumSquaredShiftRT  [4] sumSquaredShiftNum  [5] numSaturated
//   [6] numTermsInWarped   [7..51] 45 upper-triangular entries of sum w J J^T (9x9)
// ---------------------------------------------------------------------------------------------------------
#define TR_U 4            // points per thread and pass of tr_eval

// A workgroup's share of a level: nAct workgroups split the n points into contiguous chunks (multiples of 64); a workgroup
// works with only as many wavefronts as its share needs (TR_U points per lane), so the small levels pay the 52-value reduction
// on few wavefronts.  The points of the first pass stay in registers across the evaluations of a level (they do not depend on the
// candidate pose): an evaluation then costs ONE memory latency (the tap gather) instead of two.
struct TrPts { float id[TR_U], x[TR_U], y[TR_U], col[TR_U]; int lvl; };
// LDS scratch of tr_eval: per wavefront the staged vectors U | V ([16][TR_UVP] floats each), then one 16x16 result per wavefront
#define TR_UVP 68                                   // row pitch: lane l of an MFMA reads bank 4 (l & 15) + (l >> 4) (+ 4 m): conflict-free
#define TR_LDS_FLOATS ((TR_NT / 64) * (2 * 16 * TR_UVP + 256))
// accumulator q of the 52 sums <-> entry (row, col) of M = sum_p u_p v_p^T (see tr_eval): q < 7: (9 + q, 9); then the upper triangle of the 9x9
static __device__ const unsigned char TR_QROW[TR_NACC] = {9, 10, 11, 12, 13, 14, 15, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 3, 3, 3, 3, 3, 3, 4, 4, 4, 4, 4, 5, 5, 5, 5, 6, 6, 6, 7, 7, 8};
static __device__ const unsigned char TR_QCOL[TR_NACC] = {9, 9, 9, 9, 9, 9, 9, 0, 1, 2, 3, 4, 5, 6, 7, 8, 1, 2, 3, 4, 5, 6, 7, 8, 2, 3, 4, 5, 6, 7, 8, 3, 4, 5, 6, 7, 8, 4, 5, 6, 7, 8, 5, 6, 7, 8, 6, 7, 8, 7, 8, 8};
typedef float __attribute__((ext_vector_type(4))) tr_f4;
// pointers read from TrParams are generic to the compiler (flat loads); they all point to device memory
typedef const __attribute__((address_space(1))) float *tr_gptr;

#if LD_STAMP_ON_TR
__device__ long long g_trPh[5][8];      // debug: per level, time in the phases of tr_eval (wave 0 of workgroup 0), and the evaluation count
#define TPH(k) do { if (threadIdx.x == 0 && blockIdx.x == 0) { long long n_ = wall_clock64(); g_trPh[lvl][k] += n_ - tph_; tph_ = n_; } } while (0)
#else
#define TPH(k) do { } while (0)
#endif
__device__ __forceinline__ void tr_eval(const TrParams &P, int lvl, const float *Rt /*LDS: R row major (9), t (3)*/, float aff_a, float aff_b, float cutoffTH,
                        double *out /*LDS TR_NACC*/, float *red /*LDS TR_LDS_FLOATS*/, int g, int nAct, TrPts &pc) {
    const TrLevel &L = P.lv[lvl];
#if LD_STAMP_ON_TR
    long long tph_ = wall_clock64();
#endif
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nW = blockDim.x >> 6;
    const int wl = L.w, hl = L.h;
    const float fxl = L.fx, fyl = L.fy, cxl = L.cx, cyl = L.cy;
    const tr_gptr gImg = (tr_gptr) L.newImg, gId = (tr_gptr) L.pc_idepth, gU = (tr_gptr) L.pc_u, gV = (tr_gptr) L.pc_v, gCol = (tr_gptr) L.pc_color;
    const int share = (((L.n + nAct - 1) / nAct) + 63) & ~63;
    const int lo = g * share, hi = min(L.n, lo + share);
    // latency first: the share is spread over all wavefronts (one per SIMD) before a lane takes a second point
    const int nWact = max(1, min(nW, (hi - lo + 63) / 64)), nth = nWact * 64;
    const int nU = min(TR_U, max(1, (hi - lo + nth - 1) / nth));          // points per lane in the first pass (uniform)
    // RKi = R.cast<float>() * Ki ; t.cast<float>()
    float RKi[9], t[3];
    for (int r = 0; r < 3; r++) t[r] = Rt[9 + r];
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) RKi[r * 3 + c] = (Rt[r * 3 + 0] * L.Ki[0 * 3 + c] + Rt[r * 3 + 1] * L.Ki[1 * 3 + c]) + Rt[r * 3 + 2] * L.Ki[2 * 3 + c];
    float affA, affB;
    aff_from_to(P.ref_exposure, P.new_exposure, P.ref_a, P.ref_b, aff_a, aff_b, affA, affB);
    const float maxEnergy = 2 * P.huberTH * cutoffTH - P.huberTH * P.huberTH;
    const float b0 = P.ref_b;

    // The 52 sums are entries of ONE matrix M = sum_p u_p v_p^T with u = [hw J (9) | E, terms, 3 flow sums, saturated, warped] and
    // v = [J (9) | 1 | 0 ...]: the fp32 matrix cores do the 45 products per point AND the reduction over the points
    // (v_mfma_f32_16x16x4_f32: 4 points per instruction) - no per-lane accumulators, no 52-value cross-lane reduction.  Every lane
    // stages its point's u, v in the wave's LDS scratch ([component][point], conflict-free pitch) and reads them back as operands
    // (same wave: no barrier); M accumulates in 2 x 4 registers per lane.
    float *sU = red + wave * (2 * 16 * TR_UVP), *sV = sU + 16 * TR_UVP;
    tr_f4 Dm0 = {0.f, 0.f, 0.f, 0.f}, Dm1 = {0.f, 0.f, 0.f, 0.f};
    if (tid < nth) {
#pragma unroll
        for (int c = 10; c < 16; c++) sV[c * TR_UVP + lane] = 0.f;            // components 10..15 of v stay zero
    }
    TPH(0);

    // one pass: TR_U points per lane; all 12-float tap gathers of a pass are issued together
    auto pass = [&](const float (&id)[TR_U], const float (&x)[TR_U], const float (&y)[TR_U], const float (&col)[TR_U], int ib, int nu) {
        float uu[TR_U], vv[TR_U], Ku[TR_U], Kv[TR_U], nid[TR_U], tap[TR_U][12];
        bool ok[TR_U], in[TR_U];
#pragma unroll
        for (int u_ = 0; u_ < TR_U; u_++) {
            if (u_ >= nu) { ok[u_] = false; in[u_] = false; continue; }          // uniform
            in[u_] = ib + u_ * nth < hi;
            float p0 = ((RKi[0] * x[u_] + RKi[1] * y[u_]) + RKi[2] * 1.0f) + t[0] * id[u_];
            float p1 = ((RKi[3] * x[u_] + RKi[4] * y[u_]) + RKi[5] * 1.0f) + t[1] * id[u_];
            float p2 = ((RKi[6] * x[u_] + RKi[7] * y[u_]) + RKi[8] * 1.0f) + t[2] * id[u_];
            uu[u_] = p0 / p2; vv[u_] = p1 / p2;
            Ku[u_] = fxl * uu[u_] + cxl; Kv[u_] = fyl * vv[u_] + cyl;
            nid[u_] = id[u_] / p2;
            ok[u_] = in[u_] && (Ku[u_] > 2 && Kv[u_] > 2 && Ku[u_] < wl - 3 && Kv[u_] < hl - 3 && nid[u_] > 0);
            const int ix = ok[u_] ? (int) Ku[u_] : 0, iy = ok[u_] ? (int) Kv[u_] : 0;
            const tr_gptr bp = gImg + 3 * (ix + iy * wl);
            const tr_gptr bq = bp + 3 * wl;
#pragma unroll
            for (int c = 0; c < 6; c++) { tap[u_][c] = bp[c]; tap[u_][6 + c] = bq[c]; }
        }
#pragma unroll
        for (int u_ = 0; u_ < TR_U; u_++) {
            if (u_ >= nu) break;                                                   // uniform
            const int i = ib + u_ * nth;
            float uv[16], vj[9];
#pragma unroll
            for (int c = 0; c < 16; c++) uv[c] = 0.f;
#pragma unroll
            for (int c = 0; c < 9; c++) vj[c] = 0.f;
            if (in[u_] && lvl == 0 && i % 32 == 0) {
                const float *Ki = L.Ki;
                const float xx = x[u_], yy = y[u_], idd = id[u_];
                float k0 = (Ki[0] * xx + Ki[1] * yy) + Ki[2] * 1.0f, k1 = (Ki[3] * xx + Ki[4] * yy) + Ki[5] * 1.0f, k2 = (Ki[6] * xx + Ki[7] * yy) + Ki[8] * 1.0f;
                float a0 = k0 + t[0] * idd, a1 = k1 + t[1] * idd, a2 = k2 + t[2] * idd;
                float KuT = fxl * (a0 / a2) + cxl, KvT = fyl * (a1 / a2) + cyl;
                float c0 = k0 - t[0] * idd, c1 = k1 - t[1] * idd, c2 = k2 - t[2] * idd;
                float KuT2 = fxl * (c0 / c2) + cxl, KvT2 = fyl * (c1 / c2) + cyl;
                float r0 = (((RKi[0] * xx + RKi[1] * yy) + RKi[2] * 1.0f)) - t[0] * idd, r1 = (((RKi[3] * xx + RKi[4] * yy) + RKi[5] * 1.0f)) - t[1] * idd,
                      r2 = (((RKi[6] * xx + RKi[7] * yy) + RKi[8] * 1.0f)) - t[2] * idd;
                float Ku3 = fxl * (r0 / r2) + cxl, Kv3 = fyl * (r1 / r2) + cyl;
                uv[11] = ((KuT - xx) * (KuT - xx) + (KvT - yy) * (KvT - yy)) + ((KuT2 - xx) * (KuT2 - xx) + (KvT2 - yy) * (KvT2 - yy));
                uv[12] = ((Ku[u_] - xx) * (Ku[u_] - xx) + (Kv[u_] - yy) * (Kv[u_] - yy)) + ((Ku3 - xx) * (Ku3 - xx) + (Kv3 - yy) * (Kv3 - yy));
                uv[13] = 2;
            }
            if (ok[u_]) {
                const float refColor = col[u_], u = uu[u_], v = vv[u_], new_idepth = nid[u_];
                const int ix = (int) Ku[u_], iy = (int) Kv[u_];
                float dx = Ku[u_] - ix, dy = Kv[u_] - iy, dxdy = dx * dy;
                float w11 = dxdy, w01 = dy - dxdy, w10 = dx - dxdy, w00 = 1 - dx - dy + dxdy;
                const float *tp = tap[u_];
                float h0 = ((w11 * tp[9] + w01 * tp[6]) + w10 * tp[3]) + w00 * tp[0];
                float h1 = ((w11 * tp[10] + w01 * tp[7]) + w10 * tp[4]) + w00 * tp[1];
                float h2 = ((w11 * tp[11] + w01 * tp[8]) + w10 * tp[5]) + w00 * tp[2];
                if (isfinite(h0)) {
                    float residual = h0 - (float) (affA * refColor + affB);
                    float hw = fabsf(residual) < P.huberTH ? 1 : P.huberTH / fabsf(residual);
                    uv[10] = 1;
                    if (fabsf(residual) > cutoffTH) {
                        uv[9] = maxEnergy; uv[14] = 1;
                    } else {
                        uv[9] = hw * residual * residual * (2 - hw); uv[15] = 1;
                        // calcGSSSE row (CoarseTracker.cc:592-615)
                        float ddx = h1 * fxl, ddy = h2 * fyl;
                        vj[0] = new_idepth * ddx;
                        vj[1] = new_idepth * ddy;
                        vj[2] = 0 - new_idepth * (u * ddx + v * ddy);
                        vj[3] = 0 - ((u * v) * ddx + ddy * (1 + v * v));
                        vj[4] = (u * v) * ddy + ddx * (1 + u * u);
                        vj[5] = u * ddy - v * ddx;
                        vj[6] = affA * (b0 - refColor);
                        vj[7] = -1;
                        vj[8] = residual;
#pragma unroll
                        for (int r = 0; r < 9; r++) uv[r] = vj[r] * hw;
                    }
                }
            }
            // stage (all lanes of the wave: a lane without a valid point contributes u = 0), then 16 MFMAs over the 64 points
#pragma unroll
            for (int c = 0; c < 16; c++) sU[c * TR_UVP + lane] = uv[c];
#pragma unroll
            for (int c = 0; c < 9; c++) sV[c * TR_UVP + lane] = vj[c];
            sV[9 * TR_UVP + lane] = 1.f;
#pragma unroll
            for (int m = 0; m < 16; m += 2) {
                const int o0 = (lane & 15) * TR_UVP + 4 * m + (lane >> 4);
                Dm0 = __builtin_amdgcn_mfma_f32_16x16x4f32(sU[o0], sV[o0], Dm0, 0, 0, 0);
                Dm1 = __builtin_amdgcn_mfma_f32_16x16x4f32(sU[o0 + 4], sV[o0 + 4], Dm1, 0, 0, 0);
            }
        }
    };

    if (tid < nth) {
        if (pc.lvl != lvl) {                     // uniform: first evaluation of this level
#pragma unroll
            for (int u_ = 0; u_ < TR_U; u_++) {
                const int i = lo + tid + u_ * nth;
                const int ic = i < hi ? i : 0;
                pc.id[u_] = gId[ic]; pc.x[u_] = gU[ic]; pc.y[u_] = gV[ic]; pc.col[u_] = gCol[ic];
            }
        }
        pass(pc.id, pc.x, pc.y, pc.col, lo + tid, nU);
        // the trip count is the WAVE's (its first lane decides): the matrix instructions of pass() take the operands of all 64 lanes whatever the execution mask, so a
        // lane that left the loop early would feed them whatever its operand registers hold; a lane past `hi` stages zeros like the lanes past `hi` of the first pass
        for (int ib = lo + tid + nth * TR_U; ib - lane < hi; ib += nth * TR_U) {
            float id[TR_U], x[TR_U], y[TR_U], col[TR_U];
#pragma unroll
            for (int u_ = 0; u_ < TR_U; u_++) {
                const int i = ib + u_ * nth;
                const int ic = i < hi ? i : 0;
                id[u_] = gId[ic]; x[u_] = gU[ic]; y[u_] = gV[ic]; col[u_] = gCol[ic];
            }
            pass(id, x, y, col, ib, TR_U);
        }
    }
    pc.lvl = lvl;
    TPH(1);
    // one 16x16 result per wavefront: lane l, register r holds M[(l >> 4) * 4 + r][l & 15]
    float *sM = red + (TR_NT / 64) * (2 * 16 * TR_UVP);
    if (wave < nWact) {
        const tr_f4 Dm = Dm0 + Dm1;
#pragma unroll
        for (int r = 0; r < 4; r++) sM[wave * 256 + ((lane >> 4) * 4 + r) * 16 + (lane & 15)] = Dm[r];
    }
    TPH(2);
    __syncthreads();
    TPH(3);
    if (tid < TR_NACC) {
        const int o = TR_QROW[tid] * 16 + TR_QCOL[tid];
        float rv[TR_NT / 64];
#pragma unroll
        for (int w_ = 0; w_ < TR_NT / 64; w_++) rv[w_] = (w_ < nWact) ? sM[w_ * 256 + o] : 0.f;
        double s = 0;
#pragma unroll
        for (int w_ = 0; w_ < TR_NT / 64; w_++) if (w_ < nWact) s += (double) rv[w_];
        out[tid] = s;
    }
    __syncthreads();
    TPH(4);
#if LD_STAMP_ON_TR
    if (threadIdx.x == 0 && blockIdx.x == 0) g_trPh[lvl][7]++;
#endif
}

// H (8x8), b (8) from the accumulated sums: divide by the padded n, apply the reference's scale swap.
// One thread per entry (threads 0..71 of the block): no local arrays (they would live in scratch memory).
__device__ __forceinline__ void tr_hb(const double *acc, double *H, double *b) {
    const int tid = threadIdx.x;
    if (tid >= 72) return;
    const int r = (tid < 64) ? (tid >> 3) : (tid - 64), c = (tid < 64) ? (tid & 7) : 8;
    const int nw = (int) acc[6];
    const int npad = (nw + 3) / 4 * 4;
    const double inv = (double) (1.0f / (float) npad);
    // cols 0-2 x SCALE_XI_ROT, 3-5 x SCALE_XI_TRANS (sic)
    auto cs = [](int q) -> double { return (q < 3) ? 1.0 : (q < 6) ? 0.5 : (q == 6) ? 10.0 : 1000.0; };
    const int lo = min(r, c), hi = max(r, c);
    const double m = (double) (float) acc[7 + lo * 9 - (lo * (lo - 1)) / 2 + (hi - lo)];
    if (c < 8) H[r * 8 + c] = m * inv * cs(r) * cs(c);
    else b[r] = m * inv * cs(r);
}

// Eigen-style pivoted LDLT solve of an n x n (n <= 8) system, single thread
__device__ void small_ldlt_solve(const double *Ain, const double *rhs, double *x, int n) {
    double A[64];
    int tr[8];
    for (int i = 0; i < n * n; i++) A[i] = Ain[i];
    for (int k = 0; k < n; k++) {
        int idx = k; double best = fabs(A[k * n + k]);
        for (int i = k + 1; i < n; i++) if (fabs(A[i * n + i]) > best) { best = fabs(A[i * n + i]); idx = i; }
        tr[k] = idx;
        if (idx != k) {
            for (int j = 0; j < k; j++) { double a = A[k * n + j]; A[k * n + j] = A[idx * n + j]; A[idx * n + j] = a; }
            for (int j = idx + 1; j < n; j++) { double a = A[j * n + k]; A[j * n + k] = A[j * n + idx]; A[j * n + idx] = a; }
            { double a = A[k * n + k]; A[k * n + k] = A[idx * n + idx]; A[idx * n + idx] = a; }
            for (int j = k + 1; j < idx; j++) { double a = A[j * n + k]; A[j * n + k] = A[idx * n + j]; A[idx * n + j] = a; }
        }
        double temp[8];
        for (int j = 0; j < k; j++) temp[j] = A[j * n + j] * A[k * n + j];
        double s = 0;
        for (int j = 0; j < k; j++) s += A[k * n + j] * temp[j];
        A[k * n + k] -= s;
        for (int i = k + 1; i < n; i++) { double tt = 0; for (int j = 0; j < k; j++) tt += A[i * n + j] * temp[j]; A[i * n + k] -= tt; }
        double akk = A[k * n + k];
        if (fabs(akk) > 0.0) for (int i = k + 1; i < n; i++) A[i * n + k] /= akk;
    }
    for (int i = 0; i < n; i++) x[i] = rhs[i];
    for (int k = 0; k < n; k++) if (tr[k] != k) { double a = x[k]; x[k] = x[tr[k]]; x[tr[k]] = a; }
    for (int i = 0; i < n; i++) { double s = x[i]; for (int j = 0; j < i; j++) s -= A[i * n + j] * x[j]; x[i] = s; }
    for (int i = 0; i < n; i++) x[i] = (fabs(A[i * n + i]) > 2.2250738585072014e-308) ? x[i] / A[i * n + i] : 0.0;
    for (int i = n - 1; i >= 0; i--) { double s = x[i]; for (int j = i + 1; j < n; j++) s -= A[j * n + i] * x[j]; x[i] = s; }
    for (int k = n - 1; k >= 0; k--) if (tr[k] != k) { double a = x[k]; x[k] = x[tr[k]]; x[tr[k]] = a; }
}

// H (1 + lambda on the diagonal) x = rhsSign rhs, 8 x 8, by ONE lane with everything in registers: unpivoted LDL^T (the matrix is symmetric positive definite
// after the scaling, so Eigen's diagonal pivoting - which the reference runs, CoarseTracker.cc:120-128 - gives the same solution up to rounding; zero pivots
// as there: the column stays as it is, the component is dropped by D^+), one reciprocal per column (v_rcp_f64 + two Newton steps: 1.1e-16) instead of the
// ~12-instruction IEEE division sequence, the solution scaled by the same reciprocals.  On the critical path of every LM iteration: until round 4 a
// wavefront ran Eigen's pivoted factorisation lane-parallel (pivot search by DPP maxima + ballot, rows and columns exchanged by ds_bpermute: eight rounds of
// ~250 ns, 2.1 us per solve); one lane's ~250 fp64 instructions take 1.0 us (round 5, A/B on one box: kernel 311 -> 2xx us per track, same 28 iterations).
__device__ __forceinline__ double tr_rcp(double d) {
    double r = __builtin_amdgcn_rcp(d);
    r = __builtin_fma(__builtin_fma(-d, r, 1.0), r, r);
    r = __builtin_fma(__builtin_fma(-d, r, 1.0), r, r);
    return r;
}
// Returns false when a pivot has lost six digits against the diagonal entry it started from (|d_k| < 1e-6 |H_kk|: column k is, to float precision, a combination of the
// columns in front of it - a rank-deficient system: fewer than eight reference points on a level; the entries of H are float sums, so "zero" pivots come out at ~1e-7):
// Eigen's diagonal pivoting defers such a pivot to the end, where the unpivoted elimination inverts it early - the caller then runs the pivoted factorisation
// (tr_solve_pivoted8, the reference's algorithm) instead.
__device__ __forceinline__ bool ldlt8_lane(const double *H /*LDS 64, row major*/, const double *rhs /*LDS 8*/, double rhsSign, double diagScale, double *x /*8 registers*/) {
    double A[8][8], y[8], inv[8];
    bool wellConditioned = true;
#pragma unroll
    for (int i = 0; i < 8; i++) {
#pragma unroll
        for (int j = 0; j <= i; j++) A[i][j] = H[i * 8 + j];
        y[i] = rhsSign * rhs[i];
    }
#pragma unroll
    for (int i = 0; i < 8; i++) A[i][i] *= diagScale;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const double d = A[k][k];
        wellConditioned = wellConditioned && (fabs(d) >= 1e-6 * fabs(H[k * 8 + k] * diagScale));          // (the entry it started from: re-read, not kept in a register)
        const bool valid = fabs(d) > 2.2250738585072014e-308;
        inv[k] = valid ? tr_rcp(d) : 0.0;
        const double sc = valid ? inv[k] : 1.0;
#pragma unroll
        for (int j = k + 1; j < 8; j++) {
            const double L = A[j][k] * sc;          // L[j][k] (zero pivot: the column as it is)
            if (valid) {
#pragma unroll
                for (int i = j; i < 8; i++) A[i][j] = __builtin_fma(-A[i][k], L, A[i][j]);
            }
            y[j] = __builtin_fma(-y[k], L, y[j]);
            A[j][k] = L;
        }
    }
#pragma unroll
    for (int j = 0; j < 8; j++) x[j] = y[j] * inv[j];
#pragma unroll
    for (int c = 7; c >= 1; c--)
#pragma unroll
        for (int r = 0; r < c; r++) x[r] = __builtin_fma(-A[c][r], x[c], x[r]);
    return wellConditioned;
}

__device__ __forceinline__ void tr_vec6(const double *acc, double *rs) {
    const double a0 = acc[0], a1 = acc[1], a2 = acc[2], a3 = acc[3], a4 = acc[4], a5 = acc[5];          // all loads in front of the first store (both may be LDS)
    rs[0] = (double) (float) a0;
    rs[1] = (double) (int) a1;
    rs[2] = (double) ((float) a2 / ((float) a4 + 0.1f));
    rs[3] = 0;
    rs[4] = (double) ((float) a3 / ((float) a4 + 0.1f));
    rs[5] = (double) ((float) (int) a5 / (float) (int) a1);
}

// The 8 x 8 LM system by the reference's own algorithm (Eigen's diagonally pivoted LDL^T, CoarseTracker.cc:120-128): the fallback of ldlt8_lane for ill-conditioned
// systems.  Rare, single thread, out of line (its arrays live in scratch memory).
__device__ __attribute__((noinline)) void tr_solve_pivoted8(const double *sH, const double *sB, double rhsSign, double diagScale, double *sInc) {
    double Hl[64], nb[8], xs[8];
    for (int i = 0; i < 64; i++) Hl[i] = sH[i];
    for (int i = 0; i < 8; i++) { Hl[i * 8 + i] *= diagScale; nb[i] = rhsSign * sB[i]; }
    small_ldlt_solve(Hl, nb, xs, 8);
    for (int i = 0; i < 8; i++) sInc[i] = xs[i];
}

// The step when an affine parameter is fixed (setting_affineOptModeA/B < 0; CoarseTracker.cc:129-166): rare, single thread, kept out
// of line so that its 8x8 temporaries (scratch memory) stay out of the tracking kernel's register allocation.
__device__ __attribute__((noinline)) void tr_solve_fixed_affine(const double *sH, const double *sB, const double *sNb, float lambda, bool fixA, bool fixB, double *sInc) {
    double Hl[64], inc[8];
    for (int i = 0; i < 64; i++) Hl[i] = sH[i];
    for (int i = 0; i < 8; i++) { Hl[i * 8 + i] *= (1 + lambda); inc[i] = 0; }
    if (fixA && fixB) {
        double H6[36], x6[6];
        for (int i = 0; i < 6; i++) for (int j = 0; j < 6; j++) H6[i * 6 + j] = Hl[i * 8 + j];
        small_ldlt_solve(H6, sNb, x6, 6);
        for (int i = 0; i < 6; i++) inc[i] = x6[i];
    } else if (fixB) {
        double H7[49], x7[7];
        for (int i = 0; i < 7; i++) for (int j = 0; j < 7; j++) H7[i * 7 + j] = Hl[i * 8 + j];
        small_ldlt_solve(H7, sNb, x7, 7);
        for (int i = 0; i < 7; i++) inc[i] = x7[i];
    } else {
        double bs[8], H7[49], x7[7], nb7[7];
        for (int i = 0; i < 8; i++) bs[i] = sB[i];
        for (int i = 0; i < 8; i++) Hl[i * 8 + 6] = Hl[i * 8 + 7];
        for (int j = 0; j < 8; j++) Hl[6 * 8 + j] = Hl[7 * 8 + j];
        bs[6] = bs[7];
        for (int i = 0; i < 7; i++) { nb7[i] = -bs[i]; for (int j = 0; j < 7; j++) H7[i * 7 + j] = Hl[i * 8 + j]; }
        small_ldlt_solve(H7, nb7, x7, 7);
        for (int i = 0; i < 6; i++) inc[i] = x7[i];
        inc[7] = x7[6];
    }
    for (int i = 0; i < 8; i++) sInc[i] = inc[i];
}

// ---------------------------------------------------------------------------------------------------------
// Cooperative evaluation: G workgroups share ONE hypothesis.  Workgroup 0 of the group runs the LM loop (it is the only one that
// decides anything); for every calcRes / calcGSSSE evaluation it publishes the candidate (pose, affine, level, cut-off) in device
// memory under a new sequence number, every workgroup of the group evaluates a contiguous 1/nAct share of the level's points
// (nAct grows with the level size: the coarse levels stay on the leader alone), the helpers store their 52 partial sums, the
// leader adds them in workgroup order (deterministic).  The hand-over is made of self-validating 64-bit words (payload | sequence
// number) written and read with device-scope relaxed atomics (performed at the memory side, visible across the XCDs' L2s): one
// memory round trip per direction, no fences, no counters.  All workgroups of a launch must be resident (the host bounds
// nhyp * G by the CU count); sequence numbers grow over the launches of a handle, so nothing has to be cleared in between.
// ---------------------------------------------------------------------------------------------------------
#define TR_COOP_MIN 512        // smaller levels stay on the leader: less than the ~1.4 us of a hand-over to win
#define TR_COOP_PER 64         // finest share: one wavefront with one point per lane
#define TR_SPIN_LIMIT 500000000ll   // bail-out of the hand-over polls: 5 s of the 100 MHz wall clock (a track takes < 1 ms)
__device__ __forceinline__ unsigned long long tr_ld(const unsigned long long *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void tr_st(unsigned long long *p, unsigned long long v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int tr_nact(int n, int G) { return (G == 1 || n < TR_COOP_MIN) ? 1 : min(G, (n + TR_COOP_PER - 1) / TR_COOP_PER); }

// leader side of one evaluation (all threads of the leader workgroup)
template <int G>
__device__ __forceinline__ void tr_eval_lead(const TrParams &P, int lvl, const double *T, float a, float b, float cutoff, double *sAcc, float *sRed, float *sRt,
                                             TrCoop *co, int &seq, TrPts &pc, int *sAbort) {
    const int tid = threadIdx.x, nAct = tr_nact(P.lv[lvl].n, G);
    if (tid < 12) sRt[tid] = (float) T[tid < 9 ? (tid / 3) * 4 + tid % 3 : (tid - 9) * 4 + 3];
    __syncthreads();
    if (G > 1 && nAct > 1) {
        ++seq;
        if (tid < 16) {
            const unsigned pl = tid < 12 ? __builtin_bit_cast(unsigned, sRt[tid]) : tid == 12 ? __builtin_bit_cast(unsigned, a) : tid == 13 ? __builtin_bit_cast(unsigned, b)
                              : tid == 14 ? __builtin_bit_cast(unsigned, cutoff) : (unsigned) lvl;
            tr_st(&co->cmd[tid], ((unsigned long long) pl << 32) | (unsigned) seq);
        }
    }
    tr_eval(P, lvl, sRt, a, b, cutoff, sAcc, sRed, 0, nAct, pc);
    if (G > 1 && nAct > 1) {
        if (tid < TR_NACC) {
            // all helpers' words are requested together (one memory round trip once they are there), added in workgroup order
            unsigned long long w0[G > 1 ? G - 1 : 1], w1[G > 1 ? G - 1 : 1];
            bool ok;
            unsigned spins = 0; long long t0 = 0;
            do {
                ok = true;
#pragma unroll
                for (int g = 1; g < G; g++) if (g < nAct) {
                    w0[g - 1] = tr_ld(&co->part[g][tid][0]); w1[g - 1] = tr_ld(&co->part[g][tid][1]);
                }
#pragma unroll
                for (int g = 1; g < G; g++) if (g < nAct) ok = ok && ((unsigned) w0[g - 1] == (unsigned) seq) && ((unsigned) w1[g - 1] == (unsigned) seq);
                // a helper workgroup that never becomes resident (CUs held by another process / a masked device) must not hang the
                // stream: give up after TR_SPIN_LIMIT, the track then reports an error instead of a pose
                if (!ok && (++spins & 1023u) == 0) { const long long now = wall_clock64(); if (t0 == 0) t0 = now; else if (now - t0 > TR_SPIN_LIMIT) { *sAbort = 1; break; } }
            } while (!ok);
            double s_ = sAcc[tid];
#pragma unroll
            for (int g = 1; g < G; g++) if (g < nAct) s_ += __builtin_bit_cast(double, (w1[g - 1] & 0xFFFFFFFF00000000ull) | (w0[g - 1] >> 32));
            sAcc[tid] = s_;
        }
        __syncthreads();
    }
}

// helper workgroups: evaluate shares until the leader says the track is over
template <int G>
__device__ void tr_helper_loop(const TrParams &P, TrCoop *co, int g, int seq, double *sAcc, float *sRed, float *sRt, float *sF, int *sI) {
    const int tid = threadIdx.x;
    TrPts pc; pc.lvl = -1;
    for (;;) {
        if (tid < 64) {
            // the 16 command words are read by one instruction; they belong to one command when their sequence numbers agree (a
            // command this workgroup takes part in is stable until it has answered; torn reads only happen on commands it sits out)
            unsigned long long w; unsigned tag, t0; bool ok;
            unsigned spins = 0; long long c0 = 0; bool dead = false;
            do {
                w = tr_ld(&co->cmd[tid & 15]); tag = (unsigned) w;
                t0 = (unsigned) __builtin_amdgcn_readfirstlane((int) tag);
                ok = (__builtin_amdgcn_ballot_w64(tag != t0) == 0ull) && ((int) (t0 - (unsigned) seq) > 0);
                if (!ok) {
                    __builtin_amdgcn_s_sleep(1);
                    if ((++spins & 1023u) == 0) { const long long now = wall_clock64(); if (c0 == 0) c0 = now; else if (now - c0 > 2 * TR_SPIN_LIMIT) { dead = true; break; } }   // wave-uniform: the leader is gone
                }
            } while (!ok);
            const unsigned pl = (unsigned) (w >> 32);
            if (tid < 12) sRt[tid] = __builtin_bit_cast(float, pl);
            else if (tid < 15) sF[tid - 12] = __builtin_bit_cast(float, pl);
            else if (tid == 15) { sI[0] = dead ? -1 : (int) pl; sI[1] = (int) t0; }
        }
        __syncthreads();
        const int lvl = sI[0];
        seq = sI[1];
        if (lvl < 0) return;
        const int nAct = tr_nact(P.lv[lvl].n, G);
        if (g < nAct) {
            tr_eval(P, lvl, sRt, sF[0], sF[1], sF[2], sAcc, sRed, g, nAct, pc);
            if (tid < TR_NACC) {
                const unsigned long long u = __builtin_bit_cast(unsigned long long, sAcc[tid]);
                tr_st(&co->part[g][tid][0], (u << 32) | (unsigned) seq);
                tr_st(&co->part[g][tid][1], (u & 0xFFFFFFFF00000000ull) | (unsigned) seq);
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------
// trackNewestCoarse: G workgroups per hypothesis (G = 1: one workgroup runs everything)
// ---------------------------------------------------------------------------------------------------------
// The track of one hypothesis `hy` under the parameters P by the G workgroups that share the hand-over record `co` (nullptr for G = 1); this workgroup is
// number g of them (0: the leader).  Inlined into its kernels: k_tr_track (one TrParams for the whole grid) and k_tr_track_group (one job per G workgroups).
// P carries no __restrict__ here: on the inlined body it lets the compiler hoist loads of P over the whole LM loop (+28..+78 registers per lane, spills in the group kernel).
template <int G>
__device__ __forceinline__ void tr_track_body(const TrParams &P, TrHyp &hy, TrCoop *co, int g, int seq0) {
    __shared__ double sAcc[TR_NACC];
    __shared__ __attribute__((aligned(16))) float sRed[TR_LDS_FLOATS];
    __shared__ float sRt[12];
    __shared__ double sT[12], sTnew[12];
    __shared__ float sAff[2], sAffNew[2];
    __shared__ double sH[64], sB[8], sNb[8], sInc[8], sResOld[6];
    __shared__ int sCtl[5];          // 0: continue LM loop, 1: accept, 2: abort (return false), 3: iterations, 4: hand-over timed out (error)
#if LD_STAMP_ON_TR
    // debug builds: device timing of tr_eval per level (dynamically indexed -> scratch memory: never in a product build)
    long long tEval = 0, tS1 = 0, tS2 = 0, tS3 = 0, tQ = 0, tTot0 = wall_clock64(), tLv[5] = {0, 0, 0, 0, 0}; int nEval = 0, nLv[5] = {0, 0, 0, 0, 0};
#define TEV(call) do { long long t_ = wall_clock64(); call; t_ = wall_clock64() - t_; tEval += t_; nEval++; if (lvl < 5) { tLv[lvl] += t_; nLv[lvl]++; } if (threadIdx.x == 0) sEv[lvl]++; } while (0)
#else
#define TEV(call) do { call; if (threadIdx.x == 0) sEv[lvl]++; } while (0)
#endif
    __shared__ float sLambda, sCutRep;
    __shared__ int sEv[5];
    __shared__ float sCoF[4];
    if (threadIdx.x < 5) sEv[threadIdx.x] = 0;
    const int tid = threadIdx.x;
    int coSeq = seq0;
    if (G > 1 && g != 0) { tr_helper_loop<G>(P, co, g, seq0, sAcc, sRed, sRt, sCoF, sCtl); return; }
    TrPts pc; pc.lvl = -1;
    if (tid < 12) sT[tid] = hy.T[tid];
    if (tid == 0) { sAff[0] = hy.a; sAff[1] = hy.b; sCtl[3] = 0; sCtl[2] = 0; sCtl[4] = 0; for (int i = 0; i < 5; i++) hy.lastResiduals[i] = NAN; for (int i = 0; i < 3; i++) hy.flow[i] = 1000; }
    __syncthreads();
    const int maxIterations[5] = {10, 20, 50, 50, 50};
    const float lambdaExtrapolationLimit = 0.001f;
    bool haveRepeated = false;

    for (int lvl = hy.coarsestLvl; lvl >= 0; lvl--) {
        float levelCutoffRepeat = 1;
        TEV(tr_eval_lead<G>(P, lvl, sT, sAff[0], sAff[1], P.coarseCutoffTH * levelCutoffRepeat, sAcc, sRed, sRt, co, coSeq, pc, &sCtl[4]););
        if (tid == 0) tr_vec6(sAcc, sResOld);
        __syncthreads();
        while (sResOld[5] > 0.6 && levelCutoffRepeat < 50 && !sCtl[4]) {
            levelCutoffRepeat *= 2;
            TEV(tr_eval_lead<G>(P, lvl, sT, sAff[0], sAff[1], P.coarseCutoffTH * levelCutoffRepeat, sAcc, sRed, sRt, co, coSeq, pc, &sCtl[4]););
            if (tid == 0) tr_vec6(sAcc, sResOld);
            __syncthreads();
        }
        tr_hb(sAcc, sH, sB);
        if (tid == 0) sLambda = 0.01f;
        __syncthreads();

        for (int iteration = 0; iteration < maxIterations[lvl]; iteration++) {
            // the accepted energy ratio, read HERE: thread 0 overwrites sResOld in the accept block below while other wavefronts may still
            // be deciding; the closing barrier of the previous iteration orders this read behind that write, the barrier after the step
            // orders it in front of the next one
            const double oldRatio = sResOld[0] / sResOld[1];
            // H (1 + lambda on the diagonal) x = -b (CoarseTracker.cc:120-128)
#if LD_STAMP_ON_TR
            tQ = wall_clock64();
#endif
            // lane 0 alone: the solve (right-hand side -b, ldlt8_lane), then the step from the increment it has just stored
            if (tid == 0) {
                double xs[8];
                const bool wellConditioned = ldlt8_lane(sH, sB, -1.0, (double) (1 + sLambda), xs);
                for (int i = 0; i < 8; i++) sInc[i] = xs[i];
                if (!wellConditioned) { tr_solve_pivoted8(sH, sB, -1.0, (double) (1 + sLambda), sInc); hy.pivotedSolves++; }
            }
#if LD_STAMP_ON_TR
            tS1 += wall_clock64() - tQ; tQ = wall_clock64();
#endif
            if (tid == 0) {
                sCtl[3]++;
                const float lambda = sLambda;
                double inc[8];
                const bool fixA = P.affineOptModeA < 0, fixB = P.affineOptModeB < 0;
                if (fixA || fixB) { for (int i = 0; i < 8; i++) sNb[i] = -sB[i]; tr_solve_fixed_affine(sH, sB, sNb, lambda, fixA, fixB, sInc); }
                for (int i = 0; i < 8; i++) inc[i] = sInc[i];
                float extrapFac = 1;
                if (lambda < lambdaExtrapolationLimit) extrapFac = sqrtf((float) sqrt((double) (lambdaExtrapolationLimit / lambda)));
                double incScaled[8], nrm = 0, sum = 0;
                const double sc[8] = {1.0, 1.0, 1.0, 0.5, 0.5, 0.5, 10.0, 1000.0};
                for (int i = 0; i < 8; i++) { inc[i] *= extrapFac; nrm += inc[i] * inc[i]; incScaled[i] = inc[i] * sc[i]; sum += incScaled[i]; }
                if (!isfinite(sum)) for (int i = 0; i < 8; i++) incScaled[i] = 0;
                // operands into registers first, results stored at the end: a product written straight into LDS orders every load behind each of its
                // stores (same type, possibly the same memory) - twelve dependent LDS round trips for one 3 x 4 product on the LM loop's critical lane
                double E[12], Told[12], Tn[12];
#pragma unroll
                for (int i = 0; i < 12; i++) Told[i] = sT[i];
                const float a0 = sAff[0], b0 = sAff[1];
                ld::se3_exp(incScaled, E);
                ld::se3_mul(E, Told, Tn);
                float an = a0, bn = b0;
                an += incScaled[6]; bn += incScaled[7];
#pragma unroll
                for (int i = 0; i < 12; i++) sTnew[i] = Tn[i];
                sAffNew[0] = an; sAffNew[1] = bn;
                sCtl[0] = (sqrt(nrm) > 1e-3) ? 1 : 0;          // continue after this iteration?
            }
            __syncthreads();
#if LD_STAMP_ON_TR
            tS2 += wall_clock64() - tQ;
#endif
            TEV(tr_eval_lead<G>(P, lvl, sTnew, sAffNew[0], sAffNew[1], P.coarseCutoffTH * levelCutoffRepeat, sAcc, sRed, sRt, co, coSeq, pc, &sCtl[4]););
#if LD_STAMP_ON_TR
            tQ = wall_clock64();
#endif
            if (sCtl[4]) break;
            // accept? (CoarseTracker.cc:168-170) - every thread takes the decision itself from the sums the evaluation left in LDS
            // (the two operands of tr_vec6's entries 0 and 1), instead of one thread publishing it behind a barrier
            const bool accept = (((double) (float) sAcc[0]) / ((double) (int) sAcc[1])) < oldRatio;
            if (accept) tr_hb(sAcc, sH, sB);
            if (tid == 0) {
                if (accept) {
                    // every load in front of the first store (see the step above)
                    double acc6[6], rn[6], Tn[12];
#pragma unroll
                    for (int i = 0; i < 6; i++) acc6[i] = sAcc[i];
#pragma unroll
                    for (int i = 0; i < 12; i++) Tn[i] = sTnew[i];
                    const float an = sAffNew[0], bn = sAffNew[1], lam = sLambda;
                    tr_vec6(acc6, rn);
#pragma unroll
                    for (int i = 0; i < 6; i++) sResOld[i] = rn[i];
                    sAff[0] = an; sAff[1] = bn;
#pragma unroll
                    for (int i = 0; i < 12; i++) sT[i] = Tn[i];
                    sLambda = lam * 0.5f;
                } else {
                    float lam = sLambda * 4;
                    if (lam < lambdaExtrapolationLimit) lam = lambdaExtrapolationLimit;
                    sLambda = lam;
                }
            }
            __syncthreads();
#if LD_STAMP_ON_TR
            tS3 += wall_clock64() - tQ;
#endif
            if (!sCtl[0]) break;
        }
        if (tid == 0) {
            float lr = sqrtf((float) (sResOld[0] / sResOld[1]));
            hy.lastResiduals[lvl] = lr;
            for (int i = 0; i < 3; i++) hy.flow[i] = sResOld[2 + i];
            if (lr > 1.5 * hy.minRes[lvl]) sCtl[2] = 1;
        }
        __syncthreads();
        if (sCtl[2] || sCtl[4]) break;
        if (levelCutoffRepeat > 1 && !haveRepeated) { lvl++; haveRepeated = true; }
    }
#if LD_STAMP_ON_TR
    if (tid == 0) { hy.dbg[0] = (double) tEval; hy.dbg[1] = (double) (wall_clock64() - tTot0); hy.dbg[2] = nEval; for (int q = 0; q < 5; q++) hy.dbg[3 + q] = nLv[q] ? (double) tLv[q] / nLv[q] : 0.0; hy.dbg[8] = (double) tS1; hy.dbg[9] = (double) tS2; hy.dbg[10] = (double) tS3; }
#endif
    if (G > 1) {      // release the helper workgroups
        ++coSeq;
        if (tid < 16) tr_st(&co->cmd[tid], ((unsigned long long) 0xFFFFFFFFu << 32) | (unsigned) coSeq);
    }
    if (tid == 0) {
        hy.iterations = sCtl[3];
        for (int q = 0; q < 5; q++) hy.evals[q] = sEv[q];
        if (sCtl[4]) { hy.ok = -2; }      // the host turns this into LDSO_E_HIP
        else if (sCtl[2]) { hy.ok = 0; }
        else {
            for (int i = 0; i < 12; i++) hy.T[i] = sT[i];
            float a = sAff[0], b = sAff[1];
            bool ok = true;
            if ((P.affineOptModeA != 0 && (fabsf(a) > 1.2)) || (P.affineOptModeB != 0 && (fabsf(b) > 200))) ok = false;
            float ra, rb;
            aff_from_to(P.ref_exposure, P.new_exposure, P.ref_a, P.ref_b, a, b, ra, rb);
            if ((P.affineOptModeA == 0 && (fabsf(logf(ra)) > 1.5)) || (P.affineOptModeB == 0 && (fabsf(rb) > 200))) ok = false;
            if (ok) { if (P.affineOptModeA < 0) a = 0; if (P.affineOptModeB < 0) b = 0; }
            hy.a = a; hy.b = b;
            hy.ok = ok ? 1 : 0;
        }
    }
}

template <int G>
__global__ __launch_bounds__(TR_NT) void k_tr_track(const TrParams *__restrict__ Pp, TrHyp *hyps, TrCoop *coop, int seq0) {
    // *Pp: device memory, not a by-value argument: a dynamically indexed kernel argument would be copied to scratch memory
    tr_track_body<G>(*Pp, hyps[blockIdx.x / G], (G > 1) ? coop + blockIdx.x / G : nullptr, (int) (blockIdx.x % G), seq0);
}

// The tracks of a group of trackers in one launch (ldso_tr_group_*, tracker_group.hip): workgroup b serves job b / G in role b % G.  The job index is wave-uniform
// (readfirstlane), so the job's three pointers are fetched with scalar loads and stay in scalar registers; every job brings its own TrParams (device memory, as above),
// its own record and its own hand-over slot - the jobs of a launch share nothing but the sequence number seq0.
template <int G>
__global__ __launch_bounds__(TR_NT) void k_tr_track_group(const TrJob *__restrict__ jobs, int seq0) {
    const int j = __builtin_amdgcn_readfirstlane((int) (blockIdx.x / G));
    const TrJob &J = jobs[j];
    tr_track_body<G>(*J.P, *J.hyp, (G > 1) ? J.coop : nullptr, (int) (blockIdx.x % G), seq0);
}

// stand-alone calcRes / calcGSSSE for the step-wise API (one workgroup)
__global__ __launch_bounds__(TR_NT) void k_tr_calc(const TrParams *__restrict__ Pp, int lvl, const double *Tdev, float a, float b, float cutoffTH, double *outAcc) {
    const TrParams &P = *Pp;
    __shared__ double sAcc[TR_NACC];
    __shared__ __attribute__((aligned(16))) float sRed[TR_LDS_FLOATS];
    __shared__ float sRt[12];
    const int tid = threadIdx.x;
    if (tid < 12) sRt[tid] = (float) Tdev[tid < 9 ? (tid / 3) * 4 + tid % 3 : (tid - 9) * 4 + 3];
    __syncthreads();
    TrPts pc; pc.lvl = -1;
    tr_eval(P, lvl, sRt, a, b, cutoffTH, sAcc, sRed, 0, 1, pc);
    if (threadIdx.x < TR_NACC) outAcc[threadIdx.x] = sAcc[threadIdx.x];
}

// The LM solve of k_tr_track on its own (debug / test entry): H (1 + lambda on the diagonal = diag_scale) x = -b by one lane, exactly the code path of the kernel -
// the unpivoted register factorisation and, when it reports a rank-deficient system, the pivoted one.
extern "C" __global__ void k_tr_solve8(const double *H, const double *b, double diagScale, double *x, int *pivoted) {
    __shared__ double sH[64], sB[8], sInc[8];
    if (threadIdx.x < 64) sH[threadIdx.x] = H[threadIdx.x];
    if (threadIdx.x < 8) sB[threadIdx.x] = b[threadIdx.x];
    __syncthreads();
    if (threadIdx.x == 0) {
        double xs[8];
        const bool wellConditioned = ldlt8_lane(sH, sB, -1.0, diagScale, xs);
        for (int i = 0; i < 8; i++) sInc[i] = xs[i];
        if (!wellConditioned) tr_solve_pivoted8(sH, sB, -1.0, diagScale, sInc);
        *pivoted = wellConditioned ? 0 : 1;
        for (int i = 0; i < 8; i++) x[i] = sInc[i];
    }
}
// the launches (the host side is tracker_api.hip)
hipError_t tr_launch_track(int G, int nhyp, const TrParams *d_P, TrHyp *d_hyp, TrCoop *d_coop, int seq0, hipStream_t st) {
    if (G == 16) hipLaunchKernelGGL(k_tr_track<16>, dim3(nhyp * 16), dim3(TR_NT), 0, st, d_P, d_hyp, d_coop, seq0);
    else if (G == 12) hipLaunchKernelGGL(k_tr_track<12>, dim3(nhyp * 12), dim3(TR_NT), 0, st, d_P, d_hyp, d_coop, seq0);
    else if (G == 8) hipLaunchKernelGGL(k_tr_track<8>, dim3(nhyp * 8), dim3(TR_NT), 0, st, d_P, d_hyp, d_coop, seq0);
    else if (G == 4) hipLaunchKernelGGL(k_tr_track<4>, dim3(nhyp * 4), dim3(TR_NT), 0, st, d_P, d_hyp, d_coop, seq0);
    else hipLaunchKernelGGL(k_tr_track<1>, dim3(nhyp), dim3(TR_NT), 0, st, d_P, d_hyp, (TrCoop *) nullptr, 0);
    return hipGetLastError();
}
hipError_t tr_launch_track_group(int G, int njobs, const TrJob *d_jobs, int seq0, hipStream_t st) {
    if (G == 16) hipLaunchKernelGGL(k_tr_track_group<16>, dim3(njobs * 16), dim3(TR_NT), 0, st, d_jobs, seq0);
    else if (G == 12) hipLaunchKernelGGL(k_tr_track_group<12>, dim3(njobs * 12), dim3(TR_NT), 0, st, d_jobs, seq0);
    else if (G == 8) hipLaunchKernelGGL(k_tr_track_group<8>, dim3(njobs * 8), dim3(TR_NT), 0, st, d_jobs, seq0);
    else if (G == 4) hipLaunchKernelGGL(k_tr_track_group<4>, dim3(njobs * 4), dim3(TR_NT), 0, st, d_jobs, seq0);
    else hipLaunchKernelGGL(k_tr_track_group<1>, dim3(njobs), dim3(TR_NT), 0, st, d_jobs, 0);
    return hipGetLastError();
}
hipError_t tr_launch_calc(const TrParams *d_P, int lvl, const double *d_T, float a, float b, float cutoffTH, double *d_acc, hipStream_t st) {
    hipLaunchKernelGGL(k_tr_calc, dim3(1), dim3(TR_NT), 0, st, d_P, lvl, d_T, a, b, cutoffTH, d_acc);
    return hipGetLastError();
}
hipError_t tr_launch_solve8(const double *d_H, const double *d_b, double diagScale, double *d_x, int *d_pivoted) {
    hipLaunchKernelGGL(k_tr_solve8, dim3(1), dim3(64), 0, 0, d_H, d_b, diagScale, d_x, d_pivoted);
    return hipGetLastError();
}
#if LD_STAMP_ON_TR
void tr_fetch_phase_stamps(long long ph[5][8]) { const long long z[5][8] = {}; hipMemcpyFromSymbol(ph, HIP_SYMBOL(g_trPh), sizeof(z)); hipMemcpyToSymbol(HIP_SYMBOL(g_trPh), z, sizeof(z)); }
#endif
