// ba_ldlt.h — the LDL^T solver of the control step as a device function (gfx950), with everything that sizes or addresses its LDS.
// All dense math is fp64 like the reference.  The factorisation is an unpivoted LDL^T of the (diag+10)^-1/2-scaled system (SPD
// after the scaling; Eigen's LDLT pivots on the diagonal and gives the same solution up to rounding), see solve_core.
#pragma once
#include <hip/hip_runtime.h>
#include "ba_dev.h"
#include "ba_stats.h"          // NT, readlane_d, LD_THRESH_DOUBLES

// ---------------------------------------------------------------------------------------------------------
// solve_core — EnergyFunctional::solveSystemF after the assembly (EnergyFunctional.cc:293-351): scale by
// (diag+10)^-1/2, LDL^T, back substitution, unscale, orthogonalise against the gauge nullspaces, then the frame /
// calibration part of resubstituteF_MT (:491-516).
//
// The matrix is symmetric positive (semi-)definite after the scaling, so the factorisation runs WITHOUT pivoting
// (Eigen's LDLT pivots on the diagonal; for SPD input both give the same solution up to rounding).  Zero pivots
// (all-zero row/column of a PSD matrix) are skipped, like Eigen's D^+ pseudo-inverse.
//
// Layout: the (n+1)x(n+1) augmented system (row n = right-hand side, so the forward substitution is part of the
// factorisation) is padded to M = 16*NB and its lower triangle lives in REGISTERS: thread (ty,tx) of the 16x16
// block owns element (ty+16a, tx+16b) of every tile a >= b.  C (= 4) columns are eliminated per round:
//   phase 1: one thread per row replays the four scalar elimination steps on its 4 panel entries (private copy of
//            the 4x4 pivot block) -> multipliers F[i][q] = L[i][k+q] and pivot-row values G[j][q] into LDS;
//   phase 2: every thread applies the rank-4 update v -= sum_q F[i][q] G[j][q] to its register tiles and the
//            owners of the next four columns publish them as the next panel.
// Two barriers per round, no global or matrix LDS traffic inside the loop.  Every global read of the solve is
// issued in the prologue (one latency level).
// ---------------------------------------------------------------------------------------------------------
// reciprocal: hardware estimate (v_rcp_f64, ~2^-24) + ONE Newton step -> relative error <= 2.2e-15 (measured on gfx950 over
// 2^20 samples spanning 26 decades; a second step reaches 1.1e-16).  The pivot reciprocals sit on the serial critical path of the
// factorisation (fp64 VALU results have a ~30-cycle dependent-issue latency), and a 2e-15 perturbation of a multiplier is far
// below the conditioning of the system.
static __device__ __forceinline__ double fast_rcp(double d) {
    double r = __builtin_amdgcn_rcp(d);
    return __builtin_fma(__builtin_fma(-d, r, 1.0), r, r);
}

// reciprocal square root: hardware estimate (v_rsq_f64) + one Newton step (relative error <= 4.2e-15; only used as a scaling)
static __device__ __forceinline__ double fast_rsqrt(double d) {
    double r = __builtin_amdgcn_rsq(d);
    double e = __builtin_fma(-(d * r), r, 1.0);
    return __builtin_fma(0.5 * r, e, r);
}
static __device__ __forceinline__ double2 ld2(const double *p) { return *(const double2 *) p; }
static __device__ __forceinline__ void st2(double *p, double a, double b) { *(double2 *) p = make_double2(a, b); }

// Storage of L for the back substitution: L[i][c] (i > c) at sL[LIX(i, c)].
//   NB == 4: zero-initialised square [c][i] with row pitch M+2, so that lane c reads its whole column with 16-byte loads;
//   NB  > 4: packed columns (column c holds rows c..M-1).
#define LIX(i, c) ((NB == 4) ? ((c) * (M + 2) + (i)) : ((c) * M - (((c) * ((c) -1)) >> 1) + ((i) - (c))))

// GN = true (k_gn_solve): the prologue also mirrors the frames / calibration (and, when they fit, the float
// adjoints) into LDS and reduces sumNID, so that the whole control step has ONE global-load latency level; the
// frame / calibration part of backupState + doStepFromBackup is fused into the output pass.
// LDS copies of the float adjoints: 72 floats per 8 x 8 matrix.  At 64 the column reads of xAd / adHTdeltaF (lane = (pair, column), one row per instruction) put the
// eight pairs of a wavefront on the same eight banks - an 8-way conflict on each of the 32 reads of an item.  The copies are ordered by pr = h F + t (the order the
// items walk them in; the global tables are indexed h + F t), so that eight consecutive items always read eight different bank groups
#define LD_AD_LDS_PITCH 72
struct SolveIO {
    DevFrame *fr;          // working copy of the frames (global, or the LDS mirror)
    DevCalib *cal;
    const float *adH, *adT;  // float adjoints [F*F][adPitch] (global: 64, or the LDS copies: LD_AD_LDS_PITCH)
    int adPitch;
    float *ldsAd;          // LDS room for both adjoint tables (GN, may be null)
    double *sRed;          // 16 doubles of LDS scratch
    float sumNID;          // out (GN)
    double lambda;         // GN: LM lambda as passed to solveSystem
    int hasPrior;          // GN: HM / bM present
    const double *redScalars;  // GN, multi-GPU: all-reduced scalar sums (see k_gn_export), nullptr on one GPU
    const double *sx;          // out (GN): the solution in LDS (steps are its negative)
    float *sTail;              // out (GN): LDS scratch for gn_tail, 3 x 2 x LD_XFP floats (the panel buffers, free after the factorisation)
    int *waitCtr;              // GN, fused kernel: HFinal / bFinal are complete when the arrival words (ba_dev.h: arrive_shard) hold waitTarget arrivals in all,
    int waitTarget;            //                   every word its arrive_target
};

// ---------------------------------------------------------------------------------------------------------
// The dynamic LDS of the solve kernels, described once per body - core_lds (solve_core), solve_lds (solve_body), gn_lds (gn_solve_body): the kernels take their region
// pointers from these descriptions, the launchers the byte count.  The byte counts are what the residency of these kernels was tuned at (k_reduce_solve: one workgroup
// per CU): room that no region explains stays, as named slack.
// Which factorisation for n unknowns (row n of the augmented system is the right-hand side): n + 1 <= 64 -> NB = 4 blocks of 16 rows (on the matrix cores),
// n + 1 <= 112 -> 7, else 9 (the VALU variants)
// (LD_SOLVE_BY_N is seen outside this header, on purpose: LD_SOLVE_NB expands to it where the bodies and the launchers use it)
#define LD_SOLVE_BY_N(n, for4, for7, for9) (((n) + 1 <= 64) ? for4 : ((n) + 1 <= 112) ? for7 : for9)
#define LD_SOLVE_NB(n) LD_SOLVE_BY_N(n, 4, 7, 9)
#define LD_C7 4          // columns per round of the 112 x 112 factorisation (VALU variant)
static __host__ __device__ constexpr int solve_cols(int NB) { return (NB == 7) ? LD_C7 : 4; }          // columns per round of solve_core<NB>
#define LD_XFP (8 * LD_MAXF + 8)          // gn_tail: floats of one copy of x (or of the new deltas)
// solve_core, offsets in doubles from the base.  sTail aliases the panel buffers (free after the factorisation): gn_tail's float copies of x and of the deltas,
// 3 x 2 x LD_XFP floats.  slack: the launchers count 14 M doubles (NB == 4) or 30 M (three panels of up to 8 columns at pitch 10) for sFp .. sPn and
// 16 more behind sNs; the panels take 12 M (NB == 4: two buffers, the matrix cores' operands stay in registers) and 3 CP M, no region uses the difference
static __host__ __device__ constexpr size_t core_lds_end(int NB, int n) {          // CoreLds::end by itself, for the bodies: they lay their regions out behind it at run time
    size_t M = 16 * NB;
    size_t L = (NB == 4) ? M * (M + 2) : M * (M + 1) / 2;
    return L + 2 * (M + 8) /*D,Y*/ + ((NB == 4) ? 14 : 30) * M /*F,G,panel + slack*/ + 2 * M /*scale,x*/ + 7 * (size_t) n + 16;
}
struct CoreLds { size_t sL, sD, sY, sFp, sGp, sPn, sSc, sx, sNs, sTail, slack, end; };
static __host__ __device__ constexpr CoreLds core_lds(int NB, int n) {
    const size_t M = 16 * NB, CP = solve_cols(NB) + 2;          // CP: row pitch of the panel buffers (see solve_core)
    CoreLds o{};
    o.sL = 0;                                                       // L (see LIX): NB == 4 the zero-initialised square [M][M + 2], NB > 4 packed columns
    o.sD = o.sL + ((NB == 4) ? M * (M + 2) : M * (M + 1) / 2);      // [M + 8]
    o.sY = o.sD + M + 8;                                            // [M + 8]
    o.sFp = o.sTail = o.sY + M + 8;                                 // [M][CP]        (NB == 4: panel buffer A)
    o.sGp = o.sFp + CP * M;                                         // [M][CP]        (NB == 4: panel buffer B)
    o.sPn = o.sGp + CP * M;                                         // [M][CP]        (NB == 4: empty, the two buffers above alternate)
    o.sSc = o.sPn + ((NB == 4) ? 0 : CP * M);                       // [M]
    o.sx = o.sSc + M;                                               // [M]
    o.sNs = o.sx + M;                                               // [7][n], the last region
    o.end = core_lds_end(NB, n);
    o.slack = o.end - (o.sNs + 7 * (size_t) n);
    return o;
}
#define LD_LDS_SLACK 64          // slack: BYTES the launchers have always added behind the last region

// Both bodies lay their own regions out behind the core: their offsets count from core_lds_end, which is all of the layout that depends on n at run time.
// solve_body, offsets in doubles:  core | sW.  sW, 7 n + 64 doubles: the nullspace basis [7][n] of set_adjoints; the re-anchor's logs [14][6] and, at sEv, the new
// evalPT [12]; the partial sums of post_sums / res_counts [8] and io.sRed [16].  Aliases from the base, over the core (both are over when solve_core starts): the
// threshold pass (post_thresh, LD_THRESH_DOUBLES) and set_adjoints' staging of 37 doubles per pair.
struct SolveLds { size_t sW, sEv, end; };
static __host__ __device__ constexpr SolveLds solve_lds(int n) {
    SolveLds o{};
    o.sW = 0;
    o.sEv = o.sW + 96;
    o.end = o.sW + 7 * (size_t) n + 64;
    return o;
}
static __host__ __device__ constexpr size_t solve_lds_bytes(int n) { return (core_lds_end(LD_SOLVE_NB(n), n) + solve_lds(n).end) * sizeof(double) + LD_LDS_SLACK; }

// gn_solve_body, offsets in BYTES (the regions are of unlike type).  Role 0 (control step):  core | sW | sFr | sCal | ldsAd.  sW, LD_SW_DOUBLES doubles: [0, LD_SW_RED)
// are io.sRed (solve_core's partial sums of sumNID - the only part of it the solve may touch), the floats behind them belong to gn_tail: canbreak sums 0..3, K^-1 from
// LD_TAIL_KI, the calibration hand-over flag at LD_TAIL_FLAG.  sFr [F] DevFrame and sCal are the mirrors, ldsAd both float adjoint tables, gn_ad_floats each (windows of
// up to 8 key frames: F * F * 16 <= 1024 float4 per table, solve_core's prologue); gn_lds_end adds them, so that the kernel, which needs no end, does not evaluate it.
// The kernel reaches ldsAd as sCal + 1 (lds_layouts_ok: the same place): behind a constant step the pointer is known not to be null, which solve_core tests.
// Role 1 (statistics) never runs solve_core; its offsets (gn_stats_lds) count from the base:  sW [LD_SW_DOUBLES] | sTh, the threshold pass.
#define LD_SW_DOUBLES 64
#define LD_SW_RED 8
#define LD_TAIL_KI 8
#define LD_TAIL_FLAG 20          // float index behind cbF of the calibration hand-over flag
static __host__ __device__ constexpr bool gn_mirrors_adjoints(int F) { return F <= 8; }
static __host__ __device__ constexpr int gn_ad_floats(int F) { return F * F * LD_AD_LDS_PITCH; }          // one adjoint table in LDS
struct GnLds { size_t sW, sFr, sCal, ldsAd; };
static __host__ __device__ constexpr GnLds gn_lds(int F) {
    GnLds o{};
    o.sW = 0;
    o.sFr = o.sW + LD_SW_DOUBLES * sizeof(double);
    o.sCal = o.sFr + F * sizeof(DevFrame);
    o.ldsAd = o.sCal + sizeof(DevCalib);
    return o;
}
static __host__ __device__ constexpr size_t gn_lds_end(int F) { return gn_lds(F).ldsAd + (gn_mirrors_adjoints(F) ? 2 * gn_ad_floats(F) * sizeof(float) : 0); }
struct GnStatsLds { size_t sW, sTh, end; };
static __host__ __device__ constexpr GnStatsLds gn_stats_lds() {
    GnStatsLds o{};
    o.sW = 0;
    o.sTh = o.sW + LD_SW_DOUBLES * sizeof(double);
    o.end = o.sTh + LD_THRESH_DOUBLES * sizeof(double);
    return o;
}
static __host__ __device__ constexpr size_t gn_lds_bytes(int F, int n) {
    const size_t role0 = core_lds_end(LD_SOLVE_NB(n), n) * sizeof(double) + gn_lds_end(F), role1 = gn_stats_lds().end;
    return (role0 > role1 ? role0 : role1) + LD_LDS_SLACK;
}

// What the code around the layouts relies on, for every window size (n = 8 F + 4): regions of unlike type are cast onto each other and read with 16-byte accesses
// (ld2 / st2, the float4 of the adjoint copies and of gn_tail), so every offset is a multiple of 16 bytes; the aliases fit what they lie over; and, since a batched
// launch is sized by the window with the most key frames (Dmax) while each window lays itself out by its own F, the byte count does not decrease with F among the
// windows one batch can hold - 1..8 or 9..LD_MAXF key frames (one slot-table width, ldso_ba_batch_create).  From F = 8 to 9 gn_lds_bytes does decrease, 132512 to
// 97312: the adjoint copies (36864 bytes) end there.
static constexpr bool lds_layouts_ok() {
    size_t solvePrev = 0, gnPrev = 0;
    for (int F = 1; F <= LD_MAXF; F++) {
        const int n = 8 * F + 4;
        const CoreLds c = core_lds(LD_SOLVE_NB(n), n);
        const SolveLds s = solve_lds(n);
        const GnLds g = gn_lds(F);
        if ((c.sD | c.sY | c.sFp | c.sGp | c.sPn | c.sSc | c.sx | c.sNs | c.end | s.sW | s.sEv) % 2 != 0 || (g.sW | g.sFr | g.sCal | g.ldsAd | gn_stats_lds().sTh) % 16 != 0 || LD_XFP % 4 != 0 || g.ldsAd != g.sCal + sizeof(DevCalib)) return false;
        if (c.sTail * sizeof(double) + 3 * 2 * LD_XFP * sizeof(float) > c.sSc * sizeof(double)) return false;
        if (LD_THRESH_DOUBLES > c.end || 37 * (size_t) F * F > c.end || s.sEv + 12 > s.end || s.sW + 14 * 6 > s.sEv) return false;
        if (solve_lds_bytes(n) < solvePrev || (F != 9 && gn_lds_bytes(F, n) < gnPrev)) return false;
        solvePrev = solve_lds_bytes(n); gnPrev = gn_lds_bytes(F, n);
    }
    return true;
}
static_assert(lds_layouts_ok(), "solve kernels: an offset lost its alignment, an alias outgrew what it lies over, or a smaller window needs more LDS than a larger one");
typedef double __attribute__((ext_vector_type(4))) ld_d4;

// 4 x 4 transpose of (16-lane row group R = lane >> 4) x (register index q) over four doubles per lane, in registers: afterwards t[q] of lane (R, c) is what t[R] of
// lane (q, c) was.  Per dword plane, v_permlane32_swap on the register pairs (0,2), (1,3) exchanges the off-diagonal 2 x 2 blocks (lanes 32..63 of vdst <-> lanes 0..31
// of src), then v_permlane16_swap on (0,1), (2,3) transposes inside every block (odd row groups of vdst <-> even row groups of src): 16 swaps, no LDS, no wait.
// vdst is the LOWER register of each pair; the other way round yields a wrong but finite matrix (NEXT.md, section 6).
static __device__ __forceinline__ void transpose_rowgroups(double (&t)[4]) {
    unsigned w[2][4];
#pragma unroll
    for (int q = 0; q < 4; q++) { w[0][q] = (unsigned) __double2loint(t[q]); w[1][q] = (unsigned) __double2hiint(t[q]); }
#pragma unroll
    for (int p = 0; p < 2; p++) {
#pragma unroll
        for (int q = 0; q < 2; q++) { const auto r = __builtin_amdgcn_permlane32_swap(w[p][q], w[p][q + 2], false, false); w[p][q] = r[0]; w[p][q + 2] = r[1]; }
#pragma unroll
        for (int q = 0; q < 4; q += 2) { const auto r = __builtin_amdgcn_permlane16_swap(w[p][q], w[p][q + 1], false, false); w[p][q] = r[0]; w[p][q + 1] = r[1]; }
    }
#pragma unroll
    for (int q = 0; q < 4; q++) t[q] = __hiloint2double((int) w[1][q], (int) w[0][q]);
}

template <int NB, int C, bool GN, bool WAIT = false, bool MF = false>
static __device__ __forceinline__ void solve_core(const BaPtrs &B, const BaDims &D, const ResSet &S, const ldso_settings_t &St, int iteration, double *sm, SolveIO &io) {
    constexpr int M = 16 * NB;
    constexpr int CP = C + 2;      // row pitch of the panel buffers: 16-byte aligned rows, conflict-free 16-byte accesses at stride CP
    constexpr int NTILE = NB * (NB + 1) / 2;
    static_assert(MF == (NB == 4) && C == solve_cols(NB), "core_lds lays the panel buffers out for this variant");
    constexpr CoreLds lds = core_lds(NB, 0);          // n moves the end alone
    constexpr int LSZ = (int) (lds.sD - lds.sL);
    const double TINY = 2.2250738585072014e-308;
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15, F = D.F, n = D.n;
    double *sL = sm + lds.sL, *sD = sm + lds.sD, *sY = sm + lds.sY, *sFp = sm + lds.sFp, *sGp = sm + lds.sGp, *sPn = sm + lds.sPn, *sSc = sm + lds.sSc, *sx = sm + lds.sx, *sNs = sm + lds.sNs;
    const double *HF = B.sys + 3 * (n * n + n), *bF = HF + n * n;      // assembled by k_gather (step-wise path)
    const bool ortho = (St.solverMode & LDSO_SOLVER_ORTHOGONALIZE_X) || (iteration >= 2 && (St.solverMode & LDSO_SOLVER_ORTHOGONALIZE_X_LATER));

    // ---------------- prologue: every global load of the control step, issued back to back ----------------
    // GN: HFinal / bFinal (lower triangle) come straight from the accumulator k_reduce added into (B.acc)
    double v[NTILE], dI[NB], dJ[NB], dS = 0.0;
    // MF (NB == 4): the trailing update runs on the fp64 matrix cores (v_mfma_f64_16x16x4_f64).  The ten 16x16 tiles of the lower
    // triangle live in MFMA accumulator layout, three slots per wavefront: lane l, register r of a slot <-> element
    // (16 ta + (l >> 4) + 4 r, 16 tb + (l & 15)) of tile (ta, tb); wave w holds (w,0) | (w+1,w... see the packed tables) - 15 = no tile.
    static_assert(!MF || (NB == 4 && C == 4), "the MFMA variant is written for the 64x64 system, 4 columns per round");
    const int lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    constexpr int NS = MF ? 3 : 1;          // tile slots per wavefront
    int mta[NS], mtb[NS];
    if constexpr (MF) {
        mta[0] = (0x3210 >> (4 * wv)) & 15; mta[1] = (0xF321 >> (4 * wv)) & 15; mta[2] = (0xF332 >> (4 * wv)) & 15;
        mtb[0] = 0; mtb[1] = (0xF111 >> (4 * wv)) & 15; mtb[2] = (0xF322 >> (4 * wv)) & 15;
    } else { mta[0] = 15; mtb[0] = 0; }
    ld_d4 Dv[NS];
    if (GN) { HF = B.acc; bF = HF + (size_t) n * n; }
// branch-free (clamped offsets, masked values): bFinal follows HFinal in memory, so row n of the augmented system is HF[n*n + j].
// Straight-line code matters here: in the fused kernel these loads are the first instructions after the wait (cold instruction cache).
#define LD_LOAD_H() do { \
        const int nn_ = n * n + n - 1; \
_Pragma("unroll") \
        for (int a = 0; a < NB; a++) { \
            const int i = ty + 16 * a, j = tx + 16 * a; \
            const double vi = HF[min(i * n + i, nn_)], vj = HF[min(j * n + j, nn_)]; \
            dI[a] = (i < n) ? vi : 0.0; \
            dJ[a] = (j < n) ? vj : 0.0; \
        } \
_Pragma("unroll") \
        for (int a = 0; a < NB; a++) \
_Pragma("unroll") \
            for (int b = 0; b <= a; b++) { \
                const int i = ty + 16 * a, j = tx + 16 * b; \
                const double q = HF[min(i * n + j, nn_)]; \
                v[a * (a + 1) / 2 + b] = (j < n && (!GN || j <= i) && i <= n) ? q : 0.0; \
            } \
        { const double q = HF[min(tid * n + tid, nn_)]; dS = (tid < n) ? q : 0.0; } \
    } while (0)
#define LD_LOAD_H_MF() do { \
        const int nn_ = n * n + n - 1; \
_Pragma("unroll") \
        for (int s_ = 0; s_ < NS; s_++) \
_Pragma("unroll") \
            for (int r = 0; r < 4; r++) { \
                const int i = 16 * mta[s_] + (lane >> 4) + 4 * r, j = 16 * mtb[s_] + (lane & 15); \
                const double q = HF[min(i * n + j, nn_)]; \
                Dv[s_][r] = (mta[s_] < NB && j < n && (!GN || j <= i) && i <= n) ? q : 0.0; \
            } \
        { const double q = HF[min(tid * n + tid, nn_)]; dS = (tid < n) ? q : 0.0; } \
    } while (0)
    // fused kernel (io.waitCtr): the system is still being accumulated by the reduce workgroups of this launch - everything that does
    // not depend on it is loaded and staged first, the system after the wait below
    constexpr bool waitH = GN && WAIT;
    if constexpr (!waitH) { if constexpr (MF) { LD_LOAD_H_MF(); } else { LD_LOAD_H(); } }
    double nsv[4];
    if (ortho) {
#pragma unroll
        for (int u = 0; u < 4; u++) { const int i = tid + u * NT; nsv[u] = (i < 7 * n) ? B.nsProj[i] : 0.0; }      // 7n <= 924
    }
    if (GN) {
        constexpr int FW = (int) (sizeof(DevFrame) / 4), CW = (int) (sizeof(DevCalib) / 4), MW = (LD_MAXF * FW + NT - 1) / NT;
        unsigned mw[MW];
        const unsigned *gF = (const unsigned *) B.frames;
#pragma unroll
        for (int u = 0; u < MW; u++) { const int i = tid + u * NT; mw[u] = (i < F * FW) ? gF[i] : 0u; }
        const unsigned cw = (tid < CW) ? ((const unsigned *) B.calib)[tid] : 0u;
        float4 ah[4], at[4];
        if (io.ldsAd != nullptr) {      // F <= 8: F*F*16 <= 1024 float4 per table
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int i = tid + u * NT;
                ah[u] = (i < F * F * 16) ? ((const float4 *) B.adHostF)[i] : make_float4(0, 0, 0, 0);
                at[u] = (i < F * F * 16) ? ((const float4 *) B.adTargetF)[i] : make_float4(0, 0, 0, 0);
            }
        }
        double ns = 0, nc = 0;      // sumNID of doStepFromBackup, same summation order as post_sums
        for (int c = tid; c < D.nChunks; c += NT) { ns += (double) S.chunkNID[c * 2]; nc += (double) S.chunkNID[c * 2 + 1]; }
        // ---- consume ----
        unsigned *lF = (unsigned *) io.fr;
#pragma unroll
        for (int u = 0; u < MW; u++) { const int i = tid + u * NT; if (i < F * FW) lF[i] = mw[u]; }
        if (tid < CW) ((unsigned *) io.cal)[tid] = cw;
        if (io.ldsAd != nullptr) {
            float4 *lh = (float4 *) io.ldsAd, *lt = (float4 *) (io.ldsAd + gn_ad_floats(F));
#pragma unroll
            for (int u = 0; u < 4; u++) { const int i = tid + u * NT, sl = i >> 4, j = ((sl % F) * F + sl / F) * (LD_AD_LDS_PITCH / 4) + (i & 15); if (i < F * F * 16) { lh[j] = ah[u]; lt[j] = at[u]; } }
            io.adH = io.ldsAd; io.adT = io.ldsAd + gn_ad_floats(F); io.adPitch = LD_AD_LDS_PITCH;
        }
        for (int o = 32; o > 0; o >>= 1) { double a_ = __shfl_xor(ns, o, 64), b_ = __shfl_xor(nc, o, 64); ns += a_; nc += b_; }
        if ((tid & 63) == 0) { io.sRed[tid >> 6] = ns; io.sRed[4 + (tid >> 6)] = nc; }
    }
    if (ortho) {
#pragma unroll
        for (int u = 0; u < 4; u++) { const int i = tid + u * NT; if (i < 7 * n) sNs[i] = nsv[u]; }
    }
    if (NB == 4) {      // zero the square L buffer
        for (int i = tid; i < LSZ / 2; i += NT) st2(&sL[2 * i], 0.0, 0.0);
    }
    if constexpr (waitH) {
        if (LD_STAMP_ON && tid == 0) B.energyLog[47] = (double) wall_clock64();
        if (wv == 0) {
            // the producers arrive on LD_ARRIVE_SHARDS words (ba_dev.h: arrive_shard): lane s polls word s until its share of the launch's arrivers is there.
            // Bounded like gn_tail's flag wait: a target that is never met ends in the non-finite status of the iteration instead of a hung kernel
            const bool mine = lane < LD_ARRIVE_SHARDS;
            int *const word = io.waitCtr + (mine ? lane : 0) * LD_ARRIVE_STRIDE;
            const int target = mine ? arrive_target(lane, io.waitTarget) : 0;
            int spins = 0;
            while (__builtin_amdgcn_ballot_w64(target > 0 && __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) != 0 && ++spins < (1 << 22))
                __builtin_amdgcn_s_sleep(1);
            if (spins >= (1 << 22) && lane == 0) B.scalars[4] = 1.0;
            if (mine) __hip_atomic_store(word, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // every producer has arrived: re-arm for the next launch
        }
        __syncthreads();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        if (LD_STAMP_ON && tid == 0) B.energyLog[48] = (double) wall_clock64();
        if constexpr (MF) { LD_LOAD_H_MF(); } else { LD_LOAD_H(); }
    }
    if (tid < M) sSc[tid] = fast_rsqrt(dS + 10.0);
    if constexpr (MF) {
        __syncthreads();
#pragma unroll
        for (int s_ = 0; s_ < NS; s_++) {
            const double sj = sSc[min(16 * mtb[s_] + (lane & 15), M - 1)];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int i = 16 * mta[s_] + (lane >> 4) + 4 * r;
                const double si = (i == n) ? 1.0 : sSc[min(i, M - 1)];
                Dv[s_][r] = si * Dv[s_][r] * sj;
            }
        }
        // first panel (columns 0..3): the tiles of tile column 0 (slot 0 of every wave)
#pragma unroll
        for (int s_ = 0; s_ < NS; s_++) {
            if (mta[s_] >= NB || mtb[s_] != 0) continue;          // uniform per wave
            if ((lane & 15) < C) {
#pragma unroll
                for (int r = 0; r < 4; r++) sFp[(16 * mta[s_] + (lane >> 4) + 4 * r) * CP + (lane & 15)] = Dv[s_][r];
            }
        }
    } else {
        double sI[NB], sJ[NB];
#pragma unroll
        for (int a = 0; a < NB; a++) { sI[a] = (ty + 16 * a == n) ? 1.0 : fast_rsqrt(dI[a] + 10.0); sJ[a] = fast_rsqrt(dJ[a] + 10.0); }
#pragma unroll
        for (int a = 0; a < NB; a++)
#pragma unroll
            for (int b = 0; b <= a; b++) v[a * (a + 1) / 2 + b] = sI[a] * v[a * (a + 1) / 2 + b] * sJ[b];
    }
    // first panel (columns 0..C-1)
    if (!MF && tx < C) {
#pragma unroll
        for (int a = 0; a < NB; a++) sPn[(ty + 16 * a) * CP + tx] = v[a * (a + 1) / 2];
    }
    __syncthreads();
    if (LD_STAMP_ON && GN && tid == 0) B.energyLog[41] = (double) wall_clock64();
    if (GN) io.sumNID = (io.redScalars != nullptr) ? (float) io.redScalars[3] / (float) io.redScalars[4]
                                                   : (float) (io.sRed[0] + io.sRed[1] + io.sRed[2] + io.sRed[3]) / (float) (io.sRed[4] + io.sRed[5] + io.sRed[6] + io.sRed[7]);

#if LD_STAMP_ON
    long long rc_[6] = {0, 0, 0, 0, 0, 0}, rt_ = 0;
#define RCYC(i, WAITLDS) do { if (WAITLDS) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); const long long now_ = (long long) __builtin_readcyclecounter(); \
        rc_[i] += now_ - rt_; rt_ = now_; } while (0)
    rt_ = (long long) __builtin_readcyclecounter();
#else
#define RCYC(i, WAITLDS) do { } while (0)
#endif
#pragma nounroll
    for (int k = 0; k < n; k += C) {
        // ---------------- phase 1: LDL^T of the CxC pivot block (replicated in every lane) + this row's multipliers -------
        // c[r][q] (r >= q) = column q of the block after the eliminations 0..q-1 (unscaled), d_q = c[q][q], inv_q = 1/d_q;
        // g_q = A[i][k+q] after the eliminations 0..q-1, f_q = g_q / d_q = L[i][k+q].  Every update is written as
        // x -= (product of already known values) * inv_q, so that pivot d_{q+1} is ONE fma behind the reciprocal of d_q.
        // MF: every wavefront replays phase 1 for all 64 rows (lane = row) - the four copies run side by side on the four SIMDs and
        // spare the hand-over of F / G through a workgroup barrier; the panel buffers alternate (one barrier per round)
        double Ta[4], Tb[4];          // MF: the matrix cores' operands of this round (see phase 2)
        if (MF || tid < M) {
            const double *sPr = MF ? (((k >> 2) & 1) ? sGp : sFp) : sPn;
            double c[C][C], inv[C];
#pragma unroll
            for (int r = 0; r < C; r++)
#pragma unroll
                for (int q2 = 0; q2 <= r; q2 += 2) {
                    const double2 w = ld2(&sPr[(k + r) * CP + q2]);
                    c[r][q2] = w.x; if (q2 + 1 < C) c[r][q2 + 1] = w.y;
                }
            // this lane's row of the panel (the row of the thread / of the lane).  The single-pass loops over rr stay: written without them, the compiler
            // allocates k_solve and k_gn_solve differently (272 / 275 instead of 280 VGPRs, different code)
            constexpr int NR = 1;
            double g[NR][C], f[NR][C];
#pragma unroll
            for (int rr = 0; rr < NR; rr++) {
                const int i = MF ? lane + 64 * rr : tid;
#pragma unroll
                for (int q2 = 0; q2 < C; q2 += 2) { const double2 w = ld2(&sPr[i * CP + q2]); g[rr][q2] = w.x; g[rr][q2 + 1] = w.y; }
            }
            RCYC(0, true);          // panel in registers
            // l_r = c[r][q] / d_q once per pivot, every update ONE fma on it, this row's g decoupled from f: 38 fp64 instructions per round.  (Until round 4
            // every update was written as x -= (product of known values) * inv_q, which puts pivot d_{q+1} one fma behind the reciprocal of d_q but takes
            // 48 instructions: 25.4 -> 25.7 k GN iterations/s at C3 for the short form, same box - the round is bound by issue, not by the pivot chain.)
#pragma unroll
            for (int q = 0; q < C; q++) {
                const double d = c[q][q];
                inv[q] = (fabs(d) > TINY) ? fast_rcp(d) : 0.0;
                double l_[C];
#pragma unroll
                for (int r = q + 1; r < C; r++) l_[r] = c[r][q] * inv[q];
#pragma unroll
                for (int r = q + 1; r < C; r++) {
#pragma unroll
                    for (int s_ = q + 1; s_ <= r; s_++) c[r][s_] = __builtin_fma(-l_[r], c[s_][q], c[r][s_]);
#pragma unroll
                    for (int rr = 0; rr < NR; rr++) g[rr][r] = __builtin_fma(-g[rr][q], l_[r], g[rr][r]);
                }
            }
#pragma unroll
            for (int rr = 0; rr < NR; rr++)
#pragma unroll
                for (int q = 0; q < C; q++) f[rr][q] = g[rr][q] * inv[q];
#if LD_STAMP_ON
            asm volatile("" :: "v"(f[0][C - 1]), "v"(g[0][C - 1]));
#endif
            RCYC(1, false);         // 4 x 4 block and this row's multipliers issued
#pragma unroll
            for (int rr = 0; rr < NR; rr++) {
                const int i = MF ? lane + 64 * rr : tid;
                const bool below = (i >= k + C);
                const bool rowOn = below && (i <= n), colOn = below && (i < n);
                if constexpr (MF) {
                    // the masked -F and G of this lane's row, transposed in registers into MFMA operand order: afterwards Ta[t] / Tb[t] of lane l are
                    // -F / G [16 t + (l & 15)][l >> 4], the A / B operand of every tile in tile row / tile column t
#pragma unroll
                    for (int q = 0; q < C; q++) { Ta[q] = -(rowOn ? f[rr][q] : 0.0); Tb[q] = colOn ? g[rr][q] : 0.0; }
                    transpose_rowgroups(Ta); transpose_rowgroups(Tb);
                } else {
#pragma unroll
                    for (int q2 = 0; q2 < C; q2 += 2) {
                        st2(&sFp[i * CP + q2], rowOn ? f[rr][q2] : 0.0, rowOn ? f[rr][q2 + 1] : 0.0);
                        st2(&sGp[i * CP + q2], colOn ? g[rr][q2] : 0.0, colOn ? g[rr][q2 + 1] : 0.0);
                    }
                }
                // L, y, D are stored once (MF: by wave 3 - it holds ONE tile, wave 0 holds three for the longest and is the wave the round's barrier waits for:
                // 36.9 -> 35.6 us per iteration at C3, A/B x 3 on one box, profiles/r05_call0_solve_variants.log; skipping phase 1 in waves without a live tile was slower)
                const bool keeper = !MF || wv == 3;
                if (keeper && i > k && i < n) {       // L[i][k+q] for the rows of the pivot block (q < i-k) and all rows below it
#pragma unroll
                    for (int q = 0; q < C; q++) if (i > k + q) sL[LIX(i, k + q)] = f[rr][q];
                }
                if (keeper && i == n) {               // forward-substituted rhs (k + C <= n + C - 1 < M + C: sY has C spare entries)
#pragma unroll
                    for (int q2 = 0; q2 < C; q2 += 2) st2(&sY[k + q2], g[rr][q2], g[rr][q2 + 1]);
                }
                if (keeper && i == k) {
#pragma unroll
                    for (int q2 = 0; q2 < C; q2 += 2) st2(&sD[k + q2], c[q2][q2], c[q2 + 1][q2 + 1]);
                }
            }
        }
        if constexpr (MF) {
            // ---------------- phase 2 on the matrix cores: one v_mfma_f64_16x16x4_f64 per live tile (D -= F_rows G_cols^T) -------------
            // A operand: lane l supplies -F[16 ta + (l & 15)][l >> 4], B operand: G[16 tb + (l & 15)][l >> 4] - Ta[ta] and Tb[tb], which phase 1 left in
            // this wave's registers (no LDS copy, no wait between phase 1 and the matrix cores).  Tile columns left of the next panel are finished.
            RCYC(2, true);          // L, y, D stored, operands transposed
            const int bDone = (k + C) >> 4, c0 = (k + C) & 15;
            double *sPw = ((k >> 2) & 1) ? sFp : sGp;
            // Ta[mta[s]] / Tb[mtb[s]] by wave-uniform selects, written out by what the tile tables hold: mta = wv | wv + 1 | min(wv + 2, 3), mtb = 0 | 1 | 2, 2, 3
            // (14 v_cndmask a round; one case per wave with constant indices moved the accumulators between the cases and took 9 more registers)
            const double aop[NS] = {(wv == 0) ? Ta[0] : (wv == 1) ? Ta[1] : (wv == 2) ? Ta[2] : Ta[3], (wv == 0) ? Ta[1] : (wv == 1) ? Ta[2] : Ta[3], (wv == 0) ? Ta[2] : Ta[3]};
            const double bop[NS] = {Tb[0], Tb[1], (wv == 2) ? Tb[3] : Tb[2]};
#pragma unroll
            for (int s_ = 0; s_ < NS; s_++) {
                if (mta[s_] >= NB || mtb[s_] < bDone) continue;          // uniform per wave
                Dv[s_] = __builtin_amdgcn_mfma_f64_16x16x4f64(aop[s_], bop[s_], Dv[s_], 0, 0, 0);
                // owners of columns k+C .. k+2C-1 publish them as the next panel
                if (mtb[s_] == bDone && (lane & 15) >= c0 && (lane & 15) < c0 + C) {
#pragma unroll
                    for (int r = 0; r < 4; r++) sPw[(16 * mta[s_] + (lane >> 4) + 4 * r) * CP + (lane & 15) - c0] = Dv[s_][r];
                }
            }
            RCYC(3, true);          // operands selected, matrix cores, next panel published
            __syncthreads();
            RCYC(4, false);         // barrier
            continue;
        }
        __syncthreads();
        // ---------------- phase 2 (branch free: finished columns have G = 0, finished rows F = 0) ----------------
        const int a0 = (k + C) >> 4, c0 = (k + C) & 15;
        double fi[NB][C], gj[NB][C];
#pragma unroll
        for (int a = 0; a < NB; a++) {
#pragma unroll
            for (int q2 = 0; q2 < C; q2 += 2) {
                const double2 f0 = ld2(&sFp[(ty + 16 * a) * CP + q2]), g0 = ld2(&sGp[(tx + 16 * a) * CP + q2]);
                fi[a][q2] = f0.x; fi[a][q2 + 1] = f0.y; gj[a][q2] = g0.x; gj[a][q2 + 1] = g0.y;
            }
        }
        // (tile columns left of the next panel are finished, their G is zero; skipping them is slower: the round is a latency chain, not fma issue)
#pragma unroll
        for (int b = 0; b < NB; b++) {
#pragma unroll
            for (int a = b; a < NB; a++) {
                double w = v[a * (a + 1) / 2 + b];
#pragma unroll
                for (int q = 0; q < C; q++) w = __builtin_fma(-fi[a][q], gj[b][q], w);
                v[a * (a + 1) / 2 + b] = w;
            }
        }
        // owners of columns k+C .. k+2C-1 publish them as the next panel
        const bool pub = (tx >= c0) && (tx < c0 + C);
#pragma unroll
        for (int a = 0; a < NB; a++) {
            double w = v[a * (a + 1) / 2];
#pragma unroll
            for (int b = 1; b <= a; b++) w = (a0 == b) ? v[a * (a + 1) / 2 + b] : w;
            if (pub && a >= a0) sPn[(ty + 16 * a) * CP + (tx - c0)] = w;
        }
        __syncthreads();
    }
    if (LD_STAMP_ON && GN && tid == 0) B.energyLog[42] = (double) wall_clock64();
#if LD_STAMP_ON
    if (GN && MF && tid == 0) for (int u = 0; u < 5; u++) B.energyLog[53 + u] = (double) rc_[u];
#endif

    // ---------------- back substitution by wave 0: x = L^-T D^+ y ----------------
    if (tid < 64) {
        const int lane = tid;
        if (NB == 4) {
            // lane i owns x_i and column i of L in registers (zero outside the strict lower triangle); x_k is broadcast
            // with v_readlane
            double row[64];
#pragma unroll
            for (int kk = 0; kk < 64; kk += 2) { const double2 q = ld2(&sL[lane * (M + 2) + kk]); row[kk] = q.x; row[kk + 1] = q.y; }
            const double d = sD[lane], z = sY[lane];
            double xi = (lane < n && fabs(d) > TINY) ? z * fast_rcp(d) : 0.0;
            // (tried, round 4: 16-lane blocks, x_k to the lanes of its row by DPP row_newbcast - 2 moves + 1 fma per column, no v_readlane - and the 16
            // finished values of a block to the lanes below through LDS: bitwise the same x, 2.04 against 1.78 us.  A column is one broadcast + one fp64 fma
            // on the dependent chain either way, ~50 cycles; the DPP moves wait for the fma like the readlanes do, and the LDS hand-overs come on top.)
#pragma unroll
            for (int kk = 63; kk >= 1; kk--) { double xk = readlane_d(xi, kk); xi = __builtin_fma(-row[kk], xk, xi); }
            if (lane < n) sx[lane] = xi * sSc[lane];
        } else {
            // lane l owns x_i for i = l, l + 64, (l + 128) in registers; x_k is broadcast with v_readlane (no LDS round trip and no
            // wave barrier per column: the column-oriented LDS version took 15 us at n = 100); the L entries do not depend on x and
            // are loaded ahead of the dependent chain (the loop carries no LDS store)
            constexpr int NSEG = (M + 63) / 64;
            double xr[NSEG];
#pragma unroll
            for (int sg = 0; sg < NSEG; sg++) {
                const int i = lane + 64 * sg;
                const double d = sD[min(i, M - 1)];
                xr[sg] = (i < n && fabs(d) > TINY) ? sY[min(i, M - 1)] / d : 0.0;
            }
            // (round 6, measured and not kept: the L entries fetched in blocks of 16 rows one block ahead of the chain, 32 + 32 doubles in registers - k_gn_solve at C5
            // 61.2 -> 67.8 us; 8 columns per round in the factorisation, LD_C7 = 8: - 1 us)
#pragma unroll 4
            for (int kk = n - 1; kk > 0; kk--) {           // x_i -= L[k][i] x_k for i < k
                double lk[NSEG];
#pragma unroll
                for (int sg = 0; sg < NSEG; sg++) { const int i = lane + 64 * sg; lk[sg] = (i < kk) ? sL[LIX(kk, min(i, kk))] : 0.0; }
                double xk = 0.0;
#pragma unroll
                for (int sg = 0; sg < NSEG; sg++) if ((kk >> 6) == sg) xk = readlane_d(xr[sg], kk & 63);      // uniform
#pragma unroll
                for (int sg = 0; sg < NSEG; sg++) xr[sg] = __builtin_fma(-lk[sg], xk, xr[sg]);
            }
#pragma unroll
            for (int sg = 0; sg < NSEG; sg++) { const int i = lane + 64 * sg; if (i < n) sx[i] = xr[sg] * sSc[i]; }
        }
        // orthogonalize x against the gauge nullspaces (x -= U U^T x): 8 lanes per nullspace vector
        if (ortho) {
            __builtin_amdgcn_wave_barrier();
            const int kk = lane >> 3, j = lane & 7;
            double c = 0;
            if (kk < 7) for (int r = j; r < n; r += 8) c = __builtin_fma(sNs[kk * n + r], sx[r], c);
            c += __shfl_xor(c, 1, 64); c += __shfl_xor(c, 2, 64); c += __shfl_xor(c, 4, 64);
            double cc[7];
#pragma unroll
            for (int q = 0; q < 7; q++) cc[q] = readlane_d(c, q * 8);
            for (int r = lane; r < n; r += 64) {
                double s_ = 0;
#pragma unroll
                for (int q = 0; q < 7; q++) s_ = __builtin_fma(sNs[q * n + r], cc[q], s_);
                sx[r] -= s_;
            }
        }
    }
    __syncthreads();
    if (LD_STAMP_ON && GN && tid == 0) B.energyLog[43] = (double) wall_clock64();
    // ---------------- outputs: x, steps, xAd ----------------
    DevFrame *fr = io.fr;
    io.sx = sx;
    auto x_ad = [&](int i) {
        int c = i & 7, pr = i >> 3, h = pr / F, t = pr % F;
        const int sl = (io.adPitch == 64) ? h + F * t : pr;          // the LDS copies are ordered by pr = h F + t
        const float *AH = io.adH + (size_t) sl * io.adPitch, *AT = io.adT + (size_t) sl * io.adPitch;
        float ah[8], at[8];
#pragma unroll
        for (int kk = 0; kk < 8; kk++) { ah[kk] = AH[kk * 8 + c]; at[kk] = AT[kk * 8 + c]; }
        float s1 = 0, s2 = 0;
#pragma unroll
        for (int kk = 0; kk < 8; kk++) s1 += (float) sx[4 + 8 * h + kk] * ah[kk];
#pragma unroll
        for (int kk = 0; kk < 8; kk++) s2 += (float) sx[4 + 8 * t + kk] * at[kk];
        B.xAd[i] = s1 + s2;
    };
    if constexpr (GN) { io.sTail = (float *) (sm + lds.sTail); return; }          // the panel buffers are free now; gn_tail does the rest
    bool bad = false;
    for (int i = tid; i < n; i += NT) { B.x[i] = sx[i]; if (!isfinite(sx[i])) bad = true; }
    if (bad) B.scalars[4] = 1.0;
    if (tid < 4) {
        const double st = -sx[tid];
        io.cal->step[tid] = st; B.xc[tid] = (float) sx[tid];
    }
    for (int i = tid; i < F * 10; i += NT) {
        int f = i / 10, a = i % 10;
        const double st = (a < 8) ? -sx[4 + 8 * f + a] : 0.0;
        fr[f].step[a] = st;
    }
    for (int i = tid; i < F * F * 8; i += NT) x_ad(i);
    __syncthreads();
}

template <bool GN, bool WAIT = false>
static __device__ __forceinline__ void solve_core_dispatch(const BaPtrs &B, const BaDims &D, const ResSet &S, const ldso_settings_t &St, int iteration, double *sm, SolveIO &io) {
    LD_SOLVE_BY_N(D.n, (solve_core<4, solve_cols(4), GN, WAIT, true>(B, D, S, St, iteration, sm, io)), (solve_core<7, solve_cols(7), GN, WAIT>(B, D, S, St, iteration, sm, io)),
                  (solve_core<9, solve_cols(9), GN, WAIT>(B, D, S, St, iteration, sm, io)));
}

// solve_core's own macros end here
#undef LIX
#undef LD_LOAD_H
#undef LD_LOAD_H_MF
#undef RCYC
