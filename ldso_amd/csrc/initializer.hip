// initializer.hip — the monocular initialiser CoarseInitializer (reference src/frontend/CoarseInitializer.cc) for gfx950.
//
// One trackFrame (:40-178) is a Levenberg-Marquardt loop per pyramid level over (pose, affine, one inverse depth per point)
// with the depths eliminated point-wise (JbBuffer, :287-297,:363-386).  Device design:
//   k_ini_eval   grid kernel, 8 lanes per point (one lane per pattern pixel, as the BA linearise kernel): the lazily applied
//                applyStep (:673-687) of the previously accepted step, resetPoints' per-point part (:625-626) on the first
//                evaluation of a level, doStep (:645-671), then calcResAndGS (:181-405) and the calcEC sums (:412-428).
//                Per-lane fp32 accumulators (45 entries of the 9x9 Hessian, 8x9+1 of the Schur block), one partial row per block.
//   k_ini_ctl    ONE workgroup: sums the partial rows in double, takes the accept/reject decision of :120-146, keeps the LM
//                state (lambda, fails, iteration, level) in device memory, solves the damped 6x6 / 8x8 system with a
//                lane-parallel pivoted LDL^T, and runs everything that is sequential in the reference: optReg (:430-459),
//                propagateDown/Up (:462-522) and the neighbour average of resetPoints (:629-641).
//   k_ini_prep   grid kernel between the two: the per-lane inputs of the optReg sweep that follows if the step is accepted.
// The host enqueues BEGIN + the maximal number of (eval, prep, ctl) triples once; finished levels / a finished frame make the
// remaining launches return at once (device-side `done`), so there is no host round trip inside trackFrame.
//
// optReg and the resetPoints average update points IN PLACE in index order, reading neighbours that may already have been
// updated.  That order is kept exactly: the host builds, per level, a schedule of passes such that every neighbour with a
// lower index sits in an earlier pass and every reader with a lower index in an earlier-or-equal pass; one wavefront executes
// the passes with the working values in LDS (reads before writes within a pass by lock-step execution).  The dependency
// depth of that order (a diagonal front through the raster: 200-590 passes per level at 640 x 480, 20-40 points wide) is what
// a sweep costs, so a pass is made as short as it can be: optReg with two lanes per point and a fixed selection instead of a
// count-dependent one (ini_sw2_point: 28 instructions, 0.11 us per pass; round 4: one lane, a 10-key sorting network, 0.38 us).
#include "initializer.h"
#include "lie_dev.h"
#include "lane.h"

__device__ __forceinline__ float dpp_row_mirror(float x) { return dpp_mov<0x140>(x); }        // lane i <-> 15-i within each 16-lane row
__device__ __forceinline__ float min8(float x) { x = fminf(x, dpp_quad_xor1(x)); x = fminf(x, dpp_quad_xor2(x)); x = fminf(x, dpp_half_mirror(x)); return x; }
__device__ __forceinline__ float sum16(float x) { x = sum8(x); x += dpp_row_mirror(x); return x; }

__device__ __forceinline__ int ini_nblocks(int n, int gridCap) { const int nb = (n + 31) / 32; return nb < gridCap ? (nb < 1 ? 1 : nb) : gridCap; }

// ---------------------------------------------------------------------------------------------------------
// eval: (lazy applyStep) + (resetPoints | doStep) + calcResAndGS + calcEC sums
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(INI_NT) void k_ini_eval(IniParams P, int stage) {
    const IniCtl *ctl = P.ctl;
    if (!stage && (ctl->done || ctl->sweepDue)) return;         // frame finished / a level transition's control step comes first
    const int lvl = ctl->lvl;
    const IniLevel &L = P.L[lvl];
    const int n = L.n;
    const int nblk = ini_nblocks(n, INI_MAXBLK);
    if ((int) blockIdx.x >= nblk) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, k = tid & 7;
    __shared__ float sRow[16][52];
    __shared__ float sSC[16][8][10];

    // ---- uniform prologue ----
    const int mode = stage ? 2 : ctl->mode, pend = stage ? 0 : ctl->applyPending, jbSel = ctl->jbSel, snapped = ctl->snapped;
    const float lambda = ctl->lambda;
    float inc[8];
#pragma unroll
    for (int i = 0; i < 8; i++) inc[i] = ctl->inc[i];
    double T[12];
#pragma unroll
    for (int i = 0; i < 12; i++) T[i] = ctl->Tnew[i];
    float RKi[9], t[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) RKi[r * 3 + c] = (float) (T[r * 4 + 0] * L.Ki[0 * 3 + c] + T[r * 4 + 1] * L.Ki[1 * 3 + c] + T[r * 4 + 2] * L.Ki[2 * 3 + c]);
        t[r] = (float) T[r * 4 + 3];
    }
    const float affA = expf(ctl->aNew), affB = ctl->bNew;
    const float fxl = L.fx, fyl = L.fy, cxl = L.cx, cyl = L.cy;
    const int wl = L.w, hl = L.h;
    const float alphaK = 2.5f * 2.5f, alphaW = 150.0f * 150.0f, couplingWeight = 1.0f;
    float alphaOpt;
    {
        const double tsq = T[3] * T[3] + T[7] * T[7] + T[11] * T[11];
        const float alphaEnergy = (float) ((double) alphaW * (0.0 + tsq * (double) n));
        alphaOpt = (alphaEnergy > alphaK * (float) n) ? 0.0f : alphaW;
    }
    const float huberTH = P.huberTH;
    const int pdx = (k == 0) ? 0 : (k == 1) ? -1 : (k == 2) ? 1 : (k == 3) ? -2 : (k == 4) ? 0 : (k == 5) ? 2 : (k == 6) ? -1 : 0;
    const int pdy = (k == 0) ? -2 : (k == 1) ? -1 : (k == 2) ? -1 : (k == 3) ? 0 : (k == 4) ? 0 : (k == 5) ? 0 : (k == 6) ? 1 : 2;
    const float *jbOld = L.jb[jbSel];
    float *jbNew = L.jb[jbSel ^ 1];

    float acc[45];
#pragma unroll
    for (int i = 0; i < 45; i++) acc[i] = 0.0f;
    float accSC[10];
#pragma unroll
    for (int i = 0; i < 10; i++) accSC[i] = 0.0f;
    float accE = 0.0f, accEO = 0.0f, accEN = 0.0f, accEC = 0.0f;

    for (int i = blockIdx.x * 32 + (tid >> 3); i < ((n + 31) & ~31); i += nblk * 32) {
        const bool valid = i < n;
        const int ii = valid ? i : n - 1;
        float pu = L.u[ii], pv = L.v[ii], idp = L.idepth[ii], idn = L.idepth_new[ii], iR = L.iR[ii];
        int good = L.isGood[ii];
        float e0 = L.energy0[ii], e1 = L.energy1[ii];
        const float oTH = L.outlierTH[ii];
        if (mode != 2) {
            if (pend) {                                   // applyStep of the accepted evaluation (:673-687), this point's share
                if (!good) { idp = iR; idn = iR; if (valid && k == 0) L.idepth[ii] = idp; }
                else {
                    e0 = L.energy_new0[ii]; e1 = L.energy_new1[ii]; good = L.isGood_new[ii]; idp = idn;
                    if (valid && k == 0) {
                        L.energy0[ii] = e0; L.energy1[ii] = e1; L.isGood[ii] = good; L.idepth[ii] = idp;
                        L.lastHessian[ii] = L.lastHessian_new[ii];
                    }
                }
            }
            if (mode == 0) { e0 = 0.0f; e1 = 0.0f; idn = idp; if (valid && k == 0) { L.energy0[ii] = 0.0f; L.energy1[ii] = 0.0f; } }   // resetPoints :625-626
            else if (good) {                              // doStep (:645-671)
                const float *J = jbOld + (size_t) ii * 10;
                float p4[4];
#pragma unroll
                for (int q = 0; q < 4; q++) p4[q] = J[q] * inc[q] + J[q + 4] * inc[q + 4];
                const float b = J[8] + ((p4[0] + p4[2]) + (p4[1] + p4[3]));
                float step = -b * J[9] / (1 + lambda);
                float maxstep = 0.25f * L.maxstep[ii];
                if (maxstep > 1e10f) maxstep = 1e10f;
                if (step > maxstep) step = maxstep;
                if (step < -maxstep) step = -maxstep;
                float newIdepth = idp + step;
                if (newIdepth < 1e-3f) newIdepth = 1e-3f;
                if (newIdepth > 50.0f) newIdepth = 50.0f;
                idn = newIdepth;
            }
        }
        // ---- calcResAndGS for this point (:206-334) ----
        bool bad = true;
        float dp[9], dd = 0.0f, e = 0.0f, ms = 1e10f;
#pragma unroll
        for (int q = 0; q < 9; q++) dp[q] = 0.0f;
        if (valid && good) {
            const float px = pu + (float) pdx, py = pv + (float) pdy;
            const float pt0 = ((RKi[0] * px + RKi[1] * py) + RKi[2] * 1.0f) + t[0] * idn;
            const float pt1 = ((RKi[3] * px + RKi[4] * py) + RKi[5] * 1.0f) + t[1] * idn;
            const float pt2 = ((RKi[6] * px + RKi[7] * py) + RKi[8] * 1.0f) + t[2] * idn;
            const float uu = pt0 / pt2, vv = pt1 / pt2;
            const float Ku = fxl * uu + cxl, Kv = fyl * vv + cyl;
            const float new_idepth = idn / pt2;
            if (Ku > 1 && Kv > 1 && Ku < wl - 2 && Kv < hl - 2 && new_idepth > 0) {
                float hit[3], rlR;
                {
                    const int ix = (int) Ku, iy = (int) Kv;
                    const float dx = Ku - ix, dy = Kv - iy, dxdy = dx * dy;
                    const float *bp = L.cur + 3 * ((size_t) ix + (size_t) iy * wl);
#pragma unroll
                    for (int c = 0; c < 3; c++)
                        hit[c] = dxdy * bp[3 + 3 * wl + c] + (dy - dxdy) * bp[3 * wl + c] + (dx - dxdy) * bp[3 + c] + (1 - dx - dy + dxdy) * bp[c];
                }
                {
                    const int ix = (int) px, iy = (int) py;
                    const float dx = px - ix, dy = py - iy, dxdy = dx * dy;
                    const float *bp = L.first + 3 * ((size_t) ix + (size_t) iy * wl);
                    rlR = dxdy * bp[3 + 3 * wl] + (dy - dxdy) * bp[3 * wl] + (dx - dxdy) * bp[3] + (1 - dx - dy + dxdy) * bp[0];
                }
                if (isfinite(rlR) && isfinite(hit[0])) {
                    bad = false;
                    const float residual = hit[0] - affA * rlR - affB;
                    float hw = fabsf(residual) < huberTH ? 1 : huberTH / fabsf(residual);
                    e = hw * residual * residual * (2 - hw);
                    const float dxdd = (t[0] - t[2] * uu) / pt2;
                    const float dydd = (t[1] - t[2] * vv) / pt2;
                    if (hw < 1) hw = sqrtf(hw);
                    const float dxI = hw * hit[1] * fxl, dyI = hw * hit[2] * fyl;
                    dp[0] = new_idepth * dxI;
                    dp[1] = new_idepth * dyI;
                    dp[2] = -new_idepth * (uu * dxI + vv * dyI);
                    dp[3] = -uu * vv * dxI - (1 + vv * vv) * dyI;
                    dp[4] = (1 + uu * uu) * dxI + uu * vv * dyI;
                    dp[5] = -vv * dxI + uu * dyI;
                    dp[6] = -hw * affA * rlR;
                    dp[7] = -hw * 1;
                    dd = dxI * dxdd + dyI * dydd;
                    dp[8] = hw * residual;
                    const float nx = dxdd * fxl, ny = dydd * fyl;
                    ms = 1.0f / sqrtf(nx * nx + ny * ny);
                }
            }
        }
        // first bad pattern pixel of the 8-lane group: the reference breaks there (:245-259), pixels before it have updated maxstep
        const unsigned long long bm = __ballot(bad);
        const unsigned grp = (unsigned) (bm >> (lane & ~7)) & 0xFFu;
        const int firstBad = grp ? (__ffs(grp) - 1) : 8;
        const float maxstepNew = min8((k < firstBad) ? ms : 1e10f);
        const float energy = sum8(e);
        const bool goodNew = valid && good && firstBad == 8 && !(energy > oTH * 20);
        float Jb[10];
#pragma unroll
        for (int q = 0; q < 9; q++) Jb[q] = sum8(dp[q] * dd);
        Jb[9] = sum8(dd * dd);
        float en0, en1;
        if (goodNew) {
#pragma unroll
            for (int r = 0; r < 9; r++)
#pragma unroll
                for (int c = r; c < 9; c++) acc[r * 9 - (r * (r - 1)) / 2 + (c - r)] += dp[r] * dp[c];
            en0 = energy;
            en1 = (idn - 1) * (idn - 1);
            const float lastHn = Jb[9];
            Jb[8] += alphaOpt * (idn - 1);
            Jb[9] += alphaOpt;
            if (alphaOpt == 0) { Jb[8] += couplingWeight * (idn - iR); Jb[9] += couplingWeight; }
            Jb[9] = 1 / (1 + Jb[9]);
            const float w = Jb[9];
            // Schur block row k (updateSingleWeighted, MatrixAccumulators.h:1489-1614): diagonal J_r*J_r*w, off-diagonal J_c*(J_r*w)
            const float rv = (k == 0) ? Jb[0] : (k == 1) ? Jb[1] : (k == 2) ? Jb[2] : (k == 3) ? Jb[3] : (k == 4) ? Jb[4] : (k == 5) ? Jb[5] : (k == 6) ? Jb[6] : Jb[7];
            const float rw = rv * w;
#pragma unroll
            for (int q = 0; q < 9; q++) accSC[q] += (q == k) ? (rv * rv * w) : (Jb[q] * rw);
            if (k == 0) {
                accSC[9] += Jb[8] * Jb[8] * w;
                accE += energy;
                if (snapped) { const float ro = idp - iR, rn = idn - iR; accEO += ro * ro; accEN += rn * rn; accEC += 1.0f; }
                L.lastHessian_new[ii] = lastHn;
            }
            float *Jo = jbNew + (size_t) ii * 10;
            Jo[k] = rv;
            if (k < 2) Jo[8 + k] = (k == 0) ? Jb[8] : Jb[9];
        } else {
            en0 = e0; en1 = e1;                            // energy_new = energy (:213, :303)
            if (valid && k == 0) accE += e0;
        }
        if (valid && k == 0) {
            L.idepth_new[ii] = idn;
            L.isGood_new[ii] = goodNew ? 1 : 0;
            L.energy_new0[ii] = en0; L.energy_new1[ii] = en1;
            L.maxstep[ii] = maxstepNew;
        }
    }

    // ---- block reduction -> one partial row ----
#pragma unroll
    for (int i = 0; i < 45; i++) acc[i] = sum16(acc[i]);
    accE = sum16(accE); accEO = sum16(accEO); accEN = sum16(accEN); accEC = sum16(accEC);
#pragma unroll
    for (int q = 0; q < 10; q++) accSC[q] += dpp_row_ror8(accSC[q]);
    const int row = wave * 4 + (lane >> 4);
    if ((lane & 15) == 0) {
#pragma unroll
        for (int i = 0; i < 45; i++) sRow[row][i] = acc[i];
        sRow[row][45] = accE; sRow[row][46] = accEO; sRow[row][47] = accEN; sRow[row][48] = accEC;
    }
    if ((lane & 15) < 8) {
#pragma unroll
        for (int q = 0; q < 10; q++) sSC[row][lane & 7][q] = accSC[q];
    }
    __syncthreads();
    float *out = P.part + (size_t) blockIdx.x * INI_NPART;
    if (tid < 49) {
        float s = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; r++) s += sRow[r][tid];
        out[tid < 45 ? tid : (PR_E + tid - 45)] = s;
    } else if (tid >= 64 && tid < 64 + 80) {
        const int kk = (tid - 64) / 10, q = (tid - 64) % 10;
        float s = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; r++) s += sSC[r][kk][q];
        if (q < 9) out[PR_SC + kk * 9 + q] = s;
        else if (kk == 0) out[PR_SC88] = s;
    }
}

// ---------------------------------------------------------------------------------------------------------
// control block
// ---------------------------------------------------------------------------------------------------------
// Eigen-style pivoted LDL^T solve (float) of the leading nn x nn block by one wavefront, lane i*8+j holds A[i][j]; x by lanes 0..7
__device__ void ini_ldlt_wave(float a, float rhsLane, int nn, float *x /*LDS 8*/) {
    const int lane = threadIdx.x & 63, i = lane >> 3, j = lane & 7;
    if (i >= nn || j >= nn) a = 0.0f;
    int tr[8];
#pragma unroll
    for (int kk = 0; kk < 8; kk++) {
        tr[kk] = kk;
        if (kk < nn) {
            int idx = kk;
            float best = fabsf(lane_read(a, kk * 9));
#pragma unroll
            for (int q = kk + 1; q < 8; q++) { const float d = fabsf(lane_read(a, q * 9)); if (q < nn && d > best) { best = d; idx = q; } }
            tr[kk] = idx;
            if (idx != kk) {
                const int si = (i == kk) ? idx : (i == idx) ? kk : i, sj = (j == kk) ? idx : (j == idx) ? kk : j;
                a = lane_shfl(a, si * 8 + sj);
            }
            const float d = lane_read(a, kk * 9);
            const float ci = lane_shfl(a, i * 8 + kk), cj = lane_shfl(a, j * 8 + kk);
            if (fabsf(d) > 0.0f) {
                if (i > kk && j > kk) a -= ci * (cj / d);
                else if (j == kk && i > kk) a = ci / d;
                else if (i == kk && j > kk) a = cj / d;
            }
        }
    }
    float xr = (lane < nn) ? rhsLane : 0.0f;
#pragma unroll
    for (int kk = 0; kk < 8; kk++) { const int t_ = tr[kk]; if (t_ != kk) { const int src = (lane == kk) ? t_ : (lane == t_) ? kk : lane; xr = lane_shfl(xr, src & 63); } }
#pragma unroll
    for (int c = 0; c < 7; c++) { const float xc = lane_read(xr, c); const float l = lane_shfl(a, (lane & 7) * 8 + c); if (lane < 8 && lane > c) xr -= l * xc; }
    { const float dr = lane_shfl(a, (lane & 7) * 9); xr = (fabsf(dr) > 1.17549435e-38f) ? xr / dr : 0.0f; }
#pragma unroll
    for (int c = 7; c >= 1; c--) { const float xc = lane_read(xr, c); const float l = lane_shfl(a, c * 8 + (lane & 7)); if (lane < c) xr -= l * xc; }
#pragma unroll
    for (int kk = 7; kk >= 0; kk--) { const int t_ = tr[kk]; if (t_ != kk) { const int src = (lane == kk) ? t_ : (lane == t_) ? kk : lane; xr = lane_shfl(xr, src & 63); } }
    if (lane < 8) x[lane] = (lane < nn) ? xr : 0.0f;
}

// The in-place sequential sweeps (see file header).  sIR[j] = key of iR of point j if it is good, INI_NOKEY otherwise; filled by the caller.
// Behind the keys: sIR[n] = INI_NOKEY (dummy of absent / not-good neighbours and of idle lanes), sIR[n + 1] = INI_MINKEY, sIR[n + 2] = a slot nobody reads.
// Order-preserving integer key of a (non-NaN) float: integer min/max need no NaN canonicalisation.  INI_NOKEY = point not good.
#define INI_NOKEY 0x7fffffff
#define INI_MINKEY ((int) 0x80000000)
__device__ __forceinline__ int ini_key(float f) { const int b = __builtin_bit_cast(int, f); return b ^ ((b >> 31) & 0x7fffffff); }
__device__ __forceinline__ float ini_unkey(int k) { return __builtin_bit_cast(float, k ^ ((k >> 31) & 0x7fffffff)); }

// ---- resetPoints' neighbour average (:629-641), one lane per point: a point that gets an average BECOMES good for the points behind it, and the float sum runs in
// neighbour order - nothing of it can be prepared or split.  Top level only, once per frame.
// Sweep inputs of one scheduled point: LDS BYTE offsets of its own key and of its 10 neighbours' keys (an absent neighbour and an
// idle lane point at the dummy slot sK[n], which always holds INI_NOKEY - no clamps or selects in the loop).
struct SwIn { int self; int4 a, b, c; };
__device__ __forceinline__ SwIn ini_sw_load(const IniLevel &L, int p, int lane) {
    SwIn r;
    const size_t q = (size_t) p * 64 + lane;
    r.self = L.schedOff[q];
    const int4 *row = (const int4 *) (L.schedNb + q * INI_NB);
    r.a = row[0]; r.b = row[1]; r.c = row[2];
    return r;
}
__device__ __forceinline__ void ini_sw_point(const SwIn &r, int *sK, int dummyOff) {
    char *base = (char *) sK;
#define GK(off) (*(const int *) (base + (off)))
    int v[10] = {GK(r.a.x), GK(r.a.y), GK(r.a.z), GK(r.a.w), GK(r.b.x), GK(r.b.y), GK(r.b.z), GK(r.b.w), GK(r.c.x), GK(r.c.y)};
    const int self = GK(r.self);
#undef GK
    float snd = 0, sn = 0;
#pragma unroll
    for (int q = 0; q < 10; q++) if (v[q] != INI_NOKEY) { snd += ini_unkey(v[q]); sn += 1; }
    if (r.self != dummyOff && self == INI_NOKEY && sn > 0) *(int *) (base + r.self) = ini_key(snd / sn);
}
// Executed by wave 0.  The pass inputs are stored in schedule order, so every pass needs one level of coalesced global loads,
// issued four passes ahead; the dependent chain of a pass is LDS gather -> sum -> LDS write.
__device__ void ini_sweep_reset(const IniLevel &L, int *sIR) {
    if (threadIdx.x >= 64) return;
    const int lane = threadIdx.x;
    if (L.nPass == 0) return;
    const int dummyOff = L.n * 4;
    SwIn r0 = ini_sw_load(L, 0, lane), r1 = ini_sw_load(L, 1, lane), r2 = ini_sw_load(L, 2, lane), r3 = ini_sw_load(L, 3, lane);
    for (int p = 0; p < L.nPass; p += 4) {
        ini_sw_point(r0, sIR, dummyOff); r0 = ini_sw_load(L, p + 4, lane);
        ini_sw_point(r1, sIR, dummyOff); r1 = ini_sw_load(L, p + 5, lane);
        ini_sw_point(r2, sIR, dummyOff); r2 = ini_sw_load(L, p + 6, lane);
        ini_sw_point(r3, sIR, dummyOff); r3 = ini_sw_load(L, p + 7, lane);
    }
}

// ---- optReg (:430-459), TWO lanes per point.  Which points are good does not change during the sweep, so everything but the median itself is prepared in parallel
// (ini_prep) right before it: the reference takes nth_element(nnn / 2) of the nnn good neighbours' iR.  Of the 10 - nnn others, 5 - nnn / 2 are pointed at a slot
// holding the smallest key and the rest at one holding the largest: the wanted value is then ALWAYS the 6th smallest of ten keys - a fixed selection, no count,
// no select chain.  Lane 2p sorts neighbours 0-4 of its point, lane 2p + 1 neighbours 5-9 (3-input min / med / max: 15 instructions); with a_1 <= .. <= a_5 and
// b_1 <= .. <= b_5 the 6th smallest of the union is min_i max(a_i, b_(6-i)): five maxima against the partner lane's registers (DPP) and two 3-input minima.
// A point that is not written (not good, or nnn <= 2) has its result directed at a slot nobody reads; so have the odd lanes and the idle ones.
// Per lane: a = {LDS addresses of keys 0..3 of its half}, b = {the 5th, LDS address the result goes to, idepth (float bits), -}; addresses, not offsets into
// the key array: a ds_read takes them as they are
struct SwRec { int4 a, b; };
typedef __attribute__((address_space(3))) int ini_lds_int;
__device__ __forceinline__ SwRec ini_sw2_load(const IniLevel &L, int p, int lane) {
    const int4 *r = L.swRec + ((size_t) p * 64 + lane) * 2;
    SwRec o; o.a = r[0]; o.b = r[1];
    return o;
}
__device__ __forceinline__ int ini_min3(int a, int b, int c) { int r; asm("v_min3_i32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }
__device__ __forceinline__ int ini_med3(int a, int b, int c) { int r; asm("v_med3_i32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }
__device__ __forceinline__ int ini_max3(int a, int b, int c) { int r; asm("v_max3_i32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }
__device__ __forceinline__ int ini_pair(int x) { return dpp_mov<0xB1>(x); }      // the other lane of the pair
__device__ __forceinline__ void ini_sw2_point(const SwRec &r) {
    const float regWeight = 0.8f;
#define GK(adr) (*(const ini_lds_int *) (unsigned long long) (unsigned) (adr))
    const int v0 = GK(r.a.x), v1 = GK(r.a.y), v2 = GK(r.a.z), v3 = GK(r.a.w), v4 = GK(r.b.x);
#undef GK
    // sort five: s = sorted (v0, v1, v2), t = sorted (v3, v4), merged rank k = min over i + j = k of max(s_i, t_j)
    const int s1 = ini_min3(v0, v1, v2), s2 = ini_med3(v0, v1, v2), s3 = ini_max3(v0, v1, v2);
    const int t1 = min(v3, v4), t2 = max(v3, v4);
    const int m1 = min(s1, t1);
    const int m2 = ini_min3(s2, max(s1, t1), t2);
    const int m3 = ini_min3(s3, max(s2, t1), max(s1, t2));
    const int m4 = min(max(s3, t1), max(s2, t2));
    const int m5 = max(s3, t2);
    // 6th smallest of the pair's ten
    const int x1 = max(m1, ini_pair(m5)), x2 = max(m2, ini_pair(m4)), x3 = max(m3, ini_pair(m3)), x4 = max(m4, ini_pair(m2)), x5 = max(m5, ini_pair(m1));
    const int mk = ini_min3(ini_min3(x1, x2, x3), x4, x5);
    *(ini_lds_int *) (unsigned long long) (unsigned) r.b.y = ini_key((1 - regWeight) * __builtin_bit_cast(float, r.b.z) + regWeight * ini_unkey(mk));
}
// Wavefront 0 sweeps, with the inputs of INI_SW_DEPTH passes in flight.  remote: the records were written by other compute units (k_ini_prep) and lie in
// memory, not in this XCD's L2 - the other wavefronts of the block pull them in, in sweep order, ahead of wavefront 0 (one dword per 128-byte line).
#define INI_SW_DEPTH 8
__device__ void ini_sweep_reg(const IniLevel &L, int *sIR, bool remote) {
    if (L.nPass2 == 0) return;
    if (threadIdx.x >= 64) {
        if (!remote) return;
        const int *rec = (const int *) L.swRec;
        const int nLines = (L.nPass2 + INI_SWPAD) * 16;                  // 64 lanes x 32 bytes per pass
        int acc = 0;
        for (int l = threadIdx.x - 64; l < nLines; l += blockDim.x - 64) acc ^= rec[(size_t) l * 32];
        asm volatile("" :: "v"(acc));
        return;
    }
    const int lane = threadIdx.x;
    SwRec r[INI_SW_DEPTH];
#pragma unroll
    for (int u = 0; u < INI_SW_DEPTH; u++) r[u] = ini_sw2_load(L, u, lane);
    for (int p = 0; p < L.nPass2; p += INI_SW_DEPTH) {
#pragma unroll
        for (int u = 0; u < INI_SW_DEPTH; u++) { ini_sw2_point(r[u]); r[u] = ini_sw2_load(L, p + INI_SW_DEPTH + u, lane); }
    }
}

__device__ void ini_fill(const IniLevel &L, int *sIR, int pending) {
    const int nt = blockDim.x;
    if (threadIdx.x == 0) { sIR[L.n] = INI_NOKEY; sIR[L.n + 1] = INI_MINKEY; sIR[L.n + 2] = INI_NOKEY; }
    for (int j0 = threadIdx.x; j0 < L.n; j0 += 4 * nt) {
        int g[4], gn[4]; float r[4];
#pragma unroll
        for (int u = 0; u < 4; u++) { const int j = j0 + u * nt; const bool in = j < L.n; g[u] = in ? L.isGood[j] : 0; gn[u] = (in && pending) ? L.isGood_new[j] : 1; r[u] = in ? L.iR[j] : 0.0f; }
#pragma unroll
        for (int u = 0; u < 4; u++) { const int j = j0 + u * nt; if (j < L.n) sIR[j] = (g[u] && gn[u]) ? ini_key(r[u]) : INI_NOKEY; }
    }
}
// The inputs of an optReg sweep of one point (its record pair goes to the point's place in the schedule).  good(j): point j is good in the view the sweep works on.
template <class Good>
__device__ __forceinline__ void ini_prep_point(const IniLevel &L, int i, int place, const int4 &na, const int4 &nb_, const int4 &nc, float id, int base, Good good) {
    const int offMax = base + L.n * 4, offMin = offMax + 4, offNone = offMax + 8;
    const int j[10] = {na.x, na.y, na.z, na.w, nb_.x, nb_.y, nb_.z, nb_.w, nc.x, nc.y};
    int off[10], nnn = 0;
#pragma unroll
    for (int e = 0; e < 10; e++) { const bool g = j[e] >= 0 && good(max(j[e], 0)); off[e] = g ? base + j[e] * 4 : -1; nnn += g ? 1 : 0; }
    int low = 5 - (nnn >> 1);
#pragma unroll
    for (int e = 0; e < 10; e++) if (off[e] < 0) { off[e] = (low > 0) ? offMin : offMax; low--; }
    const int selfOff = (good(i) && nnn > 2) ? base + i * 4 : offNone;
    const int idb = __builtin_bit_cast(int, id);
    int4 *dst = L.swRec + (size_t) place * 4;                           // two lanes x two int4
    dst[0] = make_int4(off[0], off[1], off[2], off[3]); dst[1] = make_int4(off[4], selfOff, idb, 0);
    dst[2] = make_int4(off[5], off[6], off[7], off[8]); dst[3] = make_int4(off[9], offNone, idb, 0);
}
// ... by the control block itself (sIR holds the keys): 2.4 MB through ONE compute unit at the two big levels, ~50 us.  Only where the sweep follows a change of
// the level made by the control step (propagateDown / propagateUp, a step that snaps); the sweep behind an accepted step is prepared by k_ini_prep.
__device__ void ini_prep(const IniLevel &L, const int *sIR, const float *idv) {
    const int nt = blockDim.x;
    const int base = (int) (unsigned long long) (const ini_lds_int *) sIR;
    for (int j0 = threadIdx.x; j0 < L.n; j0 += 4 * nt) {
        int q[4]; int4 na[4], nb_[4], nc[4]; float id[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int i = min(j0 + u * nt, L.n - 1);
            const int4 *row = (const int4 *) (L.nb + (size_t) i * INI_NB);
            q[u] = L.slotOf[i]; na[u] = row[0]; nb_[u] = row[1]; nc[u] = row[2]; id[u] = idv[i];
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int i = j0 + u * nt;
            if (i < L.n) ini_prep_point(L, i, q[u], na[u], nb_[u], nc[u], id[u], base, [&](int j) { return sIR[j] != INI_NOKEY; });
        }
    }
}
// the schedule places no point has: once per handle (BEGIN), every level
__device__ void ini_prep_idle(const IniLevel &L, const int *sIR) {
    const int base = (int) (unsigned long long) (const ini_lds_int *) sIR;
    const int offMax = base + L.n * 4, offNone = offMax + 8;
    const int4 i1 = make_int4(offMax, offMax, offMax, offMax), i2 = make_int4(offMax, offNone, 0, 0);
    for (int k = threadIdx.x; k < L.nIdle; k += blockDim.x) { int4 *dst = L.swRec + (size_t) L.idleSlot[k] * 4; dst[0] = i1; dst[1] = i2; dst[2] = i1; dst[3] = i2; }
}

// optReg(lvl) (:430-459).  pending: an accepted step has not been applied to the arrays yet (lazy applyStep) - use its view.
__device__ void ini_opt_reg(const IniLevel &L, int *sIR, int snapped, int pending, bool prepared, IniCtl *ctl) {
    if (!snapped) { for (int j = threadIdx.x; j < L.n; j += blockDim.x) L.iR[j] = 1.0f; __syncthreads(); return; }
#ifdef LDSO_STAMPS
    const long long tp_ = wall_clock64();
#endif
    ini_fill(L, sIR, pending);
    __syncthreads();
    const bool remote = prepared && ctl->prepReady;                                                 // k_ini_prep has written them (for this very sweep: prepared)
    if (!remote) ini_prep(L, sIR, pending ? L.idepth_new : L.idepth);
    __syncthreads();
#ifdef LDSO_STAMPS
    const long long t0_ = wall_clock64();
#endif
    ini_sweep_reg(L, sIR, remote);
#ifdef LDSO_STAMPS
    if (threadIdx.x == 0) { const long long t1_ = wall_clock64(); ctl->dbgSweepTicks += t1_ - t0_; ctl->dbgPrepTicks += t0_ - tp_; ctl->dbgSweepPasses += L.nPass2; ctl->dbgSweeps++; }
#endif
    __syncthreads();
    for (int j = threadIdx.x; j < L.n; j += blockDim.x) { const int kk = sIR[j]; if (kk != INI_NOKEY) L.iR[j] = ini_unkey(kk); }
    __syncthreads();
}

__device__ void ini_flush_apply(const IniLevel &L) {   // applyStep (:673-687) for every point of the level
    const int nt = blockDim.x;
    for (int j0 = threadIdx.x; j0 < L.n; j0 += 4 * nt) {
        int g[4], gn[4]; float r[4], e0[4], e1[4], idn[4], lh[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int j = min(j0 + u * nt, L.n - 1);
            g[u] = L.isGood[j]; gn[u] = L.isGood_new[j]; r[u] = L.iR[j]; e0[u] = L.energy_new0[j]; e1[u] = L.energy_new1[j]; idn[u] = L.idepth_new[j]; lh[u] = L.lastHessian_new[j];
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int j = j0 + u * nt;
            if (j >= L.n) continue;
            if (!g[u]) { L.idepth[j] = r[u]; L.idepth_new[j] = r[u]; continue; }
            L.energy0[j] = e0[u]; L.energy1[j] = e1[u]; L.isGood[j] = gn[u]; L.idepth[j] = idn[u]; L.lastHessian[j] = lh[u];
        }
    }
    __syncthreads();
}

// propagateDown(lvl) (:498-522) into level lvl - 1
__device__ void ini_propagate_down(const IniParams &P, int lvl) {
    const IniLevel &L = P.L[lvl];
    const int tid = threadIdx.x;
    const IniLevel &F = P.L[lvl - 1];
    const int nt = blockDim.x;
    for (int j0 = tid; j0 < F.n; j0 += 4 * nt) {
        int pa[4], pg[4], fg[4]; float plh[4], pir[4], fir[4], flh[4];
#pragma unroll
        for (int u = 0; u < 4; u++) { const int j = min(j0 + u * nt, F.n - 1); pa[u] = F.parent[j]; fg[u] = F.isGood[j]; fir[u] = F.iR[j]; flh[u] = F.lastHessian[j]; }
#pragma unroll
        for (int u = 0; u < 4; u++) { pg[u] = L.isGood[pa[u]]; plh[u] = L.lastHessian[pa[u]]; pir[u] = L.iR[pa[u]]; }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int j = j0 + u * nt;
            if (j >= F.n) continue;
            if (!pg[u] || plh[u] < 0.1f) continue;
            if (!fg[u]) {
                const float r = pir[u];
                F.iR[j] = r; F.idepth[j] = r; F.idepth_new[j] = r; F.isGood[j] = 1; F.lastHessian[j] = 0;
            } else {
                const float newiR = (fir[u] * flh[u] * 2 + pir[u] * plh[u]) / (flh[u] * 2 + plh[u]);
                F.iR[j] = newiR; F.idepth[j] = newiR; F.idepth_new[j] = newiR;
            }
        }
    }
}
// propagateUp(s) (:462-496) into level s + 1
__device__ void ini_propagate_up(const IniParams &P, int s) {
    const IniLevel &S = P.L[s], &D = P.L[s + 1];
    for (int p = threadIdx.x; p < D.n; p += blockDim.x) {
        float a = 0, sum = 0;
        for (int q = D.childOff[p]; q < D.childOff[p + 1]; q++) {
            const int c = D.childIdx[q];
            if (!S.isGood[c]) continue;
            a += S.iR[c] * S.lastHessian[c];
            sum += S.lastHessian[c];
        }
        D.iRSumNum[p] = sum;
        if (sum > 0) { const float r = a / sum; D.iR[p] = r; D.idepth[p] = r; D.isGood[p] = 1; }
        else D.iR[p] = a;
    }
}
// the end of trackFrame (:165-177), one lane
__device__ __forceinline__ void ini_frame_end(IniCtl *ctl) {
    ctl->frameID++;
    if (!ctl->snapped) ctl->snappedAt = 0;
    if (ctl->snapped && ctl->snappedAt == 0) ctl->snappedAt = ctl->frameID;
    ctl->ready = ctl->snapped && ctl->frameID > ctl->snappedAt + 5;
    ctl->done = 1;
}

// The control step proper.  ctl is the block's LDS copy of the control record (k_ini_ctl): the decision, the bookkeeping and the pose update are one lane's
// chains of dependent reads and writes of it.
__device__ __forceinline__ void ini_ctl_body(const IniParams &P, int phase, IniCtl *ctl, int *sIR) {
    __shared__ double sSum[INI_NPART];
    __shared__ double sPart[INI_CT / 128][128];
    __shared__ float sX[8];
    __shared__ int sFlag[4];
    const int tid = threadIdx.x;
    const int top = P.levels - 1;

    if (phase == INI_BEGIN) {                                   // trackFrame :42-69 + resetPoints' neighbour average at the top level
        const int snapped = ctl->snapped;
        if (!snapped) {
            for (int l = 0; l < P.levels; l++) {
                const IniLevel &L = P.L[l];
                for (int j = tid; j < L.n; j += blockDim.x) { L.iR[j] = 1.0f; L.idepth_new[j] = 1.0f; L.lastHessian[j] = 0.0f; }
            }
        }
        if (tid == 0) {
            if (!snapped) { ctl->Tcur[3] = 0; ctl->Tcur[7] = 0; ctl->Tcur[11] = 0; }
            if (P.firstExposure > 0 && P.newExposure > 0) { ctl->aCur = logf(P.newExposure / P.firstExposure); ctl->bCur = 0; }
            for (int q = 0; q < 12; q++) ctl->Tnew[q] = ctl->Tcur[q];
            ctl->aNew = ctl->aCur; ctl->bNew = ctl->bCur;
            ctl->lvl = top; ctl->mode = 0; ctl->done = 0; ctl->evals = 0; ctl->applyPending = 0; ctl->iteration = 0; ctl->fails = 0; ctl->lambda = 0.1f;
            for (int q = 0; q < 8; q++) ctl->inc[q] = 0;
        }
        if (!ctl->idleWritten) for (int l = 0; l < P.levels; l++) ini_prep_idle(P.L[l], sIR);
        __syncthreads();
        if (tid == 0) { ctl->idleWritten = 1; ctl->ldsBase = (int) (unsigned long long) (const ini_lds_int *) sIR; ctl->prepReady = 0; ctl->steps = 0; ctl->sweepDue = 0; ctl->upGoing = 0; }
        const IniLevel &L = P.L[top];
        ini_fill(L, sIR, 0);
        __syncthreads();
        ini_sweep_reset(L, sIR);
        __syncthreads();
        for (int j = tid; j < L.n; j += blockDim.x) {
            const int kk = sIR[j];
            if (!L.isGood[j] && kk != INI_NOKEY) { const float v = ini_unkey(kk); L.isGood[j] = 1; L.iR[j] = v; L.idepth[j] = v; L.idepth_new[j] = v; }
        }
        return;
    }

#ifdef LDSO_STAMPS
    const long long tk0_ = wall_clock64();
#endif
    if (phase == INI_STEP && ctl->sweepDue) {                   // a level transition of a snapped frame: the sweep behind propagateDown / propagateUp, then what follows it
        const int sl = ctl->sweepDue - 1, up = ctl->upGoing;
        ini_opt_reg(P.L[sl], sIR, 1, 0, true, ctl);
        if (up && sl + 1 < P.levels) {
            ini_propagate_up(P, sl);
            __syncthreads();
            if (tid == 0) ctl->sweepDue = sl + 2;
        } else if (tid == 0) {
            ctl->sweepDue = 0;
            if (up) { ctl->upGoing = 0; ini_frame_end(ctl); }
        }
        return;
    }
    const int lvl = ctl->lvl;
    const IniLevel &L = P.L[lvl];
    const int n = L.n;
    // ---- sum the partial rows ----
    {
        const int nblk = ini_nblocks(n, INI_MAXBLK);
        const int c = tid & 127, part = tid >> 7;              // 8 row slices
        double s = 0.0;
        if (c < PR_N) {
#pragma unroll 8
            for (int r = part; r < nblk; r += INI_CT / 128) s += (double) P.part[(size_t) r * INI_NPART + c];
        }
        sPart[part][c] = s;
        __syncthreads();
        if (tid < 128) { double a = 0.0; for (int q = 0; q < INI_CT / 128; q++) a += sPart[q][tid]; sSum[tid] = a; }
        __syncthreads();
    }
    const float alphaK = 2.5f * 2.5f, alphaW = 150.0f * 150.0f;
    if (tid < 64) {                                             // H_new, Hsc_new (:389-401)
        const int r = tid >> 3, c = tid & 7, lo = min(r, c), hi = max(r, c);
        ctl->Hn[tid] = (float) sSum[lo * 9 - (lo * (lo - 1)) / 2 + (hi - lo)];
        ctl->Hscn[tid] = (float) sSum[PR_SC + lo * 9 + hi];
    } else if (tid < 72) {
        const int r = tid - 64;
        ctl->bn[r] = (float) sSum[r * 9 - (r * (r - 1)) / 2 + (8 - r)];
        ctl->bscn[r] = (float) sSum[PR_SC + r * 9 + 8];
    }
    __syncthreads();
    if (tid == 0) {
        const double *T = ctl->Tnew;
        const double tsq = T[3] * T[3] + T[7] * T[7] + T[11] * T[11];
        float alphaEnergy = (float) ((double) alphaW * (0.0 + tsq * (double) n));
        float alphaOpt;
        if (alphaEnergy > alphaK * (float) n) { alphaOpt = 0; alphaEnergy = alphaK * (float) n; } else alphaOpt = alphaW;
        ctl->Hn[0] += alphaOpt * n; ctl->Hn[9] += alphaOpt * n; ctl->Hn[18] += alphaOpt * n;
        double lg[6];
        ld::se3_log(T, lg);
        for (int q = 0; q < 3; q++) ctl->bn[q] += (float) lg[q] * alphaOpt * n;
        ctl->resNew[0] = (float) sSum[PR_E]; ctl->resNew[1] = alphaEnergy; ctl->resNew[2] = (float) (2 * n);
        if (ctl->snapped) { ctl->ec[0] = 1.0f * (float) sSum[PR_ECO]; ctl->ec[1] = 1.0f * (float) sSum[PR_ECN]; ctl->ec[2] = (float) sSum[PR_ECC]; }
        else { ctl->ec[0] = 0; ctl->ec[1] = 0; ctl->ec[2] = (float) n; }
    }
    __syncthreads();
    if (phase == INI_STAGE) return;

    // ---- the decision of :120-158 ----
    if (tid == 0) {
        const int maxIterations[5] = {5, 5, 10, 30, 50};
        int accept, quit = 0, doOpt = 0;
        ctl->evals++;
        if (ctl->mode == 0) {                                   // first evaluation of the level (:81-88)
            accept = 1;
            ctl->lambda = 0.1f; ctl->fails = 0; ctl->iteration = 0; ctl->mode = 1;
        } else {
            const float eTotalNew = (ctl->resNew[0] + ctl->resNew[1] + ctl->ec[1]);
            const float eTotalOld = (ctl->resOld[0] + ctl->resOld[1] + ctl->ec[0]);
            accept = eTotalOld > eTotalNew;
            if (accept) {
                if (ctl->resNew[1] == alphaK * (float) n) ctl->snapped = 1;
                for (int q = 0; q < 12; q++) ctl->Tcur[q] = ctl->Tnew[q];
                ctl->aCur = ctl->aNew; ctl->bCur = ctl->bNew;
                doOpt = 1;
                ctl->lambda *= 0.5f; ctl->fails = 0;
                if (ctl->lambda < 0.0001f) ctl->lambda = 0.0001f;
            } else {
                ctl->fails++;
                ctl->lambda *= 4;
                if (ctl->lambda > 10000) ctl->lambda = 10000;
            }
            float nrm = 0;
            for (int q = 0; q < 8; q++) nrm += ctl->inc[q] * ctl->inc[q];
            nrm = sqrtf(nrm);
            if (!(nrm > 1e-4f) || ctl->iteration >= maxIterations[lvl] || ctl->fails >= 2) quit = 1;
            else ctl->iteration++;
        }
        if (accept) {
            for (int q = 0; q < 64; q++) { ctl->H[q] = ctl->Hn[q]; ctl->Hsc[q] = ctl->Hscn[q]; }
            for (int q = 0; q < 8; q++) { ctl->b[q] = ctl->bn[q]; ctl->bsc[q] = ctl->bscn[q]; }
            for (int q = 0; q < 3; q++) ctl->resOld[q] = ctl->resNew[q];
            ctl->applyPending = 1; ctl->jbSel ^= 1;
        } else ctl->applyPending = 0;
        sFlag[0] = accept; sFlag[1] = quit; sFlag[2] = doOpt; sFlag[3] = ctl->snapped;
    }
    __syncthreads();
    const int accept = sFlag[0], quit = sFlag[1], doOpt = sFlag[2], snapped = sFlag[3];
#ifdef LDSO_STAMPS
    if (tid == 0) ctl->dbgFrontTicks += wall_clock64() - tk0_;
#endif
    if (doOpt) ini_opt_reg(L, sIR, snapped, 1, true, ctl);                 // applyStep (pending) + optReg (:137-138)

    if (quit) {
        if (accept) ini_flush_apply(L);
        if (tid == 0) ctl->applyPending = 0;
        // Once snapped, the optReg sweep that follows a propagation is the next control step's (ini_transition_step): k_ini_prep prepares it in between, on the
        // whole chip, instead of this block streaming the level's records through one compute unit (~50 us at the big levels)
        if (lvl > 0) {
            ini_propagate_down(P, lvl);
            __syncthreads();
            if (snapped) { if (tid == 0) ctl->sweepDue = lvl; }          // level lvl - 1, stored + 1
            else ini_opt_reg(P.L[lvl - 1], sIR, 0, 0, false, ctl);
            if (tid == 0) {
                ctl->lvl = lvl - 1; ctl->mode = 0;
                for (int q = 0; q < 12; q++) ctl->Tnew[q] = ctl->Tcur[q];
                ctl->aNew = ctl->aCur; ctl->bNew = ctl->bCur;
            }
        } else if (snapped && P.levels > 1) {                   // :165-177, continued by the transition steps
            ini_propagate_up(P, 0);
            __syncthreads();
            if (tid == 0) { ctl->sweepDue = 2; ctl->upGoing = 1; }
        } else {
            for (int s = 0; s + 1 < P.levels; s++) {
                ini_propagate_up(P, s);
                __syncthreads();
                ini_opt_reg(P.L[s + 1], sIR, snapped, 0, false, ctl);
            }
            if (tid == 0) ini_frame_end(ctl);
        }
        return;
    }

    // ---- next increment (:90-111) ----
#ifdef LDSO_STAMPS
    const long long tt0_ = wall_clock64();
#endif
    if (tid < 64) {
        const int i = tid >> 3, j = tid & 7;
        const float lambda = ctl->lambda;
        const float wMi = (i < 3) ? 1.0f : (i < 6) ? 0.5f : (i == 6) ? 10.0f : 1000.0f, wMj = (j < 3) ? 1.0f : (j < 6) ? 0.5f : (j == 6) ? 10.0f : 1000.0f;
        float Hl = ctl->H[tid];
        if (i == j) Hl *= (1 + lambda);
        Hl -= ctl->Hsc[tid] * (1 / (1 + lambda));
        const float sc = (0.01f / (L.w * L.h));
        Hl = ((wMi * Hl) * wMj) * sc;
        float bl = 0.0f;
        if (tid < 8) {
            const float wMr = (tid < 3) ? 1.0f : (tid < 6) ? 0.5f : (tid == 6) ? 10.0f : 1000.0f;
            bl = ctl->b[tid] - ctl->bsc[tid] * (1 / (1 + lambda));
            bl = (wMr * bl) * sc;
        }
        ini_ldlt_wave(Hl, bl, P.fixAffine ? 6 : 8, sX);
    }
    __syncthreads();
    if (tid == 0) {
        double xi[6], E[12], Tn[12];
        for (int q = 0; q < 8; q++) {
            const float wMr = (q < 3) ? 1.0f : (q < 6) ? 0.5f : (q == 6) ? 10.0f : 1000.0f;
            ctl->inc[q] = (P.fixAffine && q >= 6) ? 0.0f : -(wMr * sX[q]);
        }
        for (int q = 0; q < 6; q++) xi[q] = (double) ctl->inc[q];
        ld::se3_exp(xi, E);
        ld::se3_mul(E, ctl->Tcur, Tn);
        for (int q = 0; q < 12; q++) ctl->Tnew[q] = Tn[q];
        ctl->aNew = ctl->aCur + ctl->inc[6];
        ctl->bNew = ctl->bCur + ctl->inc[7];
#ifdef LDSO_STAMPS
        ctl->dbgTailTicks += wall_clock64() - tt0_;
#endif
    }
}

__global__ __launch_bounds__(INI_CT) void k_ini_ctl(IniParams P, int phase) {
    extern __shared__ int sIR[];
    __shared__ IniCtl sCtl;
    static_assert(sizeof(IniCtl) % 4 == 0, "IniCtl is copied in dwords");
    if (phase == INI_STEP && P.ctl->done) return;           // the frame is finished: the rest of the enqueued launches return at once
#ifdef LDSO_STAMPS
    const long long tk0_ = wall_clock64();
#endif
    for (int q = threadIdx.x; q < (int) (sizeof(IniCtl) / 4); q += blockDim.x) ((int *) &sCtl)[q] = ((const int *) P.ctl)[q];
    __syncthreads();
    ini_ctl_body(P, phase, &sCtl, sIR);
    __syncthreads();
    if (threadIdx.x == 0) {
        sCtl.prepReady = 0;
        if (phase == INI_STEP) sCtl.steps++;
#ifdef LDSO_STAMPS
        if (phase != INI_BEGIN) sCtl.dbgCtlTicks += wall_clock64() - tk0_;
#endif
    }
    __syncthreads();
    for (int q = threadIdx.x; q < (int) (sizeof(IniCtl) / 4); q += blockDim.x) ((int *) P.ctl)[q] = ((const int *) &sCtl)[q];
}

// The sweep inputs of the step an evaluation has just tried, by the whole chip instead of the control block (launched between k_ini_eval and k_ini_ctl): if the
// control step accepts it, optReg (:137-138) sweeps the level in the view "good and still good after the step" with the new inverse depths - both final when
// k_ini_eval ends.  Wasted when the step is rejected (a few us beside the evaluation).
__global__ __launch_bounds__(INI_PT) void k_ini_prep(IniParams P) {
    const IniCtl *ctl = P.ctl;
    // nothing to prepare: frame finished; optReg only resets iR before the snap (a step that snaps is prepared by the control step itself)
    if (ctl->done || !ctl->snapped) return;
    const int due = ctl->sweepDue;
    if (!due && ctl->mode == 0) return;                         // first evaluation of a level: no step to accept
    // the sweep behind a propagation (level due - 1: good points, applied depths) or the one behind the step just evaluated (good and still good, new depths)
    const IniLevel &L = P.L[due ? due - 1 : ctl->lvl];
    const float *idv = due ? L.idepth : L.idepth_new;
    const int base = ctl->ldsBase;
    for (int i = blockIdx.x * INI_PT + threadIdx.x; i < L.n; i += gridDim.x * INI_PT) {
        const int4 *row = (const int4 *) (L.nb + (size_t) i * INI_NB);
        const int4 na = row[0], nb_ = row[1], nc = row[2];
        if (due) ini_prep_point(L, i, L.slotOf[i], na, nb_, nc, idv[i], base, [&](int j) { return L.isGood[j] != 0; });
        else ini_prep_point(L, i, L.slotOf[i], na, nb_, nc, idv[i], base, [&](int j) { return L.isGood[j] && L.isGood_new[j]; });
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) P.ctl->prepReady = 1;
}

// the launches (the host side is initializer_api.hip)
hipError_t ini_ctl_reserve_lds(size_t ldsBytes) { return hipFuncSetAttribute((const void *) k_ini_ctl, hipFuncAttributeMaxDynamicSharedMemorySize, (int) ldsBytes); }
void ini_launch_eval(const IniParams &P, int stage, hipStream_t st) { hipLaunchKernelGGL(k_ini_eval, dim3(INI_MAXBLK), dim3(INI_NT), 0, st, P, stage); }
void ini_launch_prep(const IniParams &P, int blocks, hipStream_t st) { hipLaunchKernelGGL(k_ini_prep, dim3(blocks), dim3(INI_PT), 0, st, P); }
void ini_launch_ctl(const IniParams &P, int phase, size_t ldsBytes, hipStream_t st) { hipLaunchKernelGGL(k_ini_ctl, dim3(1), dim3(INI_CT), ldsBytes, st, P, phase); }
