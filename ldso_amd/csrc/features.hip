// features.hip — corner features of a new key frame on the device (gfx950): FeatureDetector::DetectCorners (reference
// src/frontend/FeatureDetector.cc:34-130 with ShiTomasiScore / IC_Angle of include/frontend/FeatureDetector.h:49-114 and ComputeDescriptor :132-189)
// and the ImmaturePoint constructor (src/internal/ImmaturePoint.cc:14-38) for every feature - what FullSystem::makeNewTraces (FullSystem.cc:1272-1325)
// does for setting_pointSelection == 1.  Input: level 0 of a resident ldso_pyramid_t, 12-byte pixels (I, dx, dy).
//
//   k_feat_cells     one workgroup per grid cell: the (dx, dy) patch of (gridsize + 8)^2 pixels is staged in LDS once, absSquaredGrad is computed on the fly,
//                    cell maximum -> gradTH -> candidates; every candidate's 64 Shi-Tomasi taps are summed by ONE lane in the reference's order (three float
//                    accumulators); the k best by (score descending, idx ascending) go to the cell's slots; the global maximum score over ALL
//                    candidates is an integer atomicMax on the bits of max(s, 0) (exact, order-independent)
//   k_feat_compact   one workgroup: prefix sum over the cells' counts (segment_scan256; cells gx-major, gy inner = the reference's loop order), features to their final
//                    places, corner candidates score > float(0.01 * double(maxScore))
//   k_feat_corners   the all-pairs suppression :107-118 through LDS tiles; it never rereads isCorner, so it is a pure function of (u, v, score, index)
//   k_feat_describe  one wavefront per corner: the 31 x 31 intensity patch staged in LDS, lane 0 accumulates the moments in the reference's order,
//                    atan2f; then 4 x 64 descriptor bits, one per lane, collected with a ballot
//   k_feat_records   one lane per feature: the 8 pattern taps of the ImmaturePoint constructor (getInterpolatedElement33BiLin, GlobalFuncs.h:186-207)
//   k_feat_*_group   the same five bodies for the jobs of a group of detectors (ldso_feat_group_*, at the end of this file), and k_feat_append_group: the fresh
//                    records behind those of each job's tracer
//
// Every float expression keeps the reference's operand order and width (the library is built with -ffp-contract=off).  Where the reference would read
// outside the image (descriptor / moment taps of a feature near the right or bottom border, possible at gridsize 16..18 and from 31 on; it has no check) a tap reads 0 here, and
// an immature record whose taps leave the image gets a NaN colour and energyTH = NaN.  Rows 0 and h-1 have zero gradients (images.hip).
#include "trace.h"
#include "immature_record.h"
#include "lane.h"
#include "select_dev.h"

#define FEAT_HP 15                      // HALF_PATCH_SIZE, FeatureDetector.h:20
#define FEAT_MAX_GRID 64                // largest gridsize the cell kernel stages in LDS

struct FeatGrid { int gridsize, gridX, gridY, skip, perCell, nx, ny; float nfeatInGrid; };

// FeatureDetector.cc:37-42 - the one definition host and device read
static __host__ __device__ inline FeatGrid feat_grid(int w, int h, int n) {
    FeatGrid G;
    G.gridsize = (int) (sqrtf((float) (w * h / n)) + 0.5);
    G.gridX = w / G.gridsize + 1; G.gridY = h / G.gridsize + 1;
    G.nfeatInGrid = (float) n / (w * h) * (G.gridsize * G.gridsize);
    G.skip = (FEAT_HP * 2 / G.gridsize) + 1;
    int k = 0;                          // `picked++; if (picked > nfeatInGrid) break` (:88-91)
    do k++; while (!((float) k > G.nfeatInGrid));
    G.perCell = k;
    G.nx = G.gridX - 2 * G.skip > 0 ? G.gridX - 2 * G.skip : 0;
    G.ny = G.gridY - 2 * G.skip > 0 ? G.gridY - 2 * G.skip : 0;
    return G;
}

struct FeatArgs {
    const float *img; int w, h;
    FeatGrid G;
    const float *B;                     // 256-entry response table or null
    const int32_t *pattern;             // 1024-entry ORB pattern or null
    ldso_feature_t *cellFeat; int32_t *cellCount;
    ldso_feature_t *feat; ldso_immature_t *imm;
    int32_t *ctl;                       // [0] bits of maxScore, [1] flags, [2] n features, [3] n corners
    ldso_immature_t *appendPts;         // grouped call with a tracer: where its next record goes (d_pts + n) and that record's my_type, else null
    float *appendType;
    int hostIndex;
};

// orderable key of a candidate's score: larger score = larger key, NaN below every number, 0 = no candidate
static __device__ __forceinline__ unsigned feat_key(float s) {
    if (s != s) return 1u;
    if (s == 0.0f) s = 0.0f;            // -0 == +0
    const unsigned u = (unsigned) __float_as_int(s);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// The bodies of the five kernels as device functions of (job, unit): the solo kernel runs them on its by-value argument and blockIdx, the grouped twin
// (k_feat_*_group, below) on a row of the group's job table and the unit group_member_of finds: the same code on the same bytes.
// the body of k_feat_cells for grid cell `cell` of A (dynamic LDS: (16 + 2 P^2 + 2 g^2) floats, carved by the job's own gridsize)
static __device__ __forceinline__ void feat_cells(const FeatArgs &A, int cell) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int g = A.G.gridsize, P = g + 8, w = A.w, h = A.h, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned long long *red = (unsigned long long *) lds;          // [8] cross-wave scratch
    float *pdx = lds + 16, *pdy = pdx + P * P, *sc = pdy + P * P;
    unsigned *key = (unsigned *) (sc + g * g);
    const int gx = A.G.skip + cell / A.G.ny, gy = A.G.skip + cell % A.G.ny;
    const int x0 = gx * g, y0 = gy * g;
    bool bad = false;
    for (int p = tid; p < P * P; p += 256) {
        const int x = x0 - 4 + p % P, y = y0 - 4 + p / P;
        float dx = 0, dy = 0;
        if (x >= 0 && x < w && y >= 0 && y < h) { const float *px = A.img + 3 * ((size_t) y * w + x); dx = px[1]; dy = px[2]; }
        if (!isfinite(dx) || !isfinite(dy)) bad = true;
        pdx[p] = dx; pdy[p] = dy;
    }
    __syncthreads();
    // absSquaredGrad and the cell's maximum (:50-55)
    float m = 0;
    for (int p = tid; p < g * g; p += 256) {
        const int x = p % g, y = p / g, q = (y + 4) * P + x + 4;
        const float I = A.img[3 * ((size_t) (y0 + y) * w + x0 + x)];          // the cell lies inside the image (gx < gridX - skip, skip >= 1)
        const float d = abs_sq_grad(I, pdx[q], pdy[q], A.B, bad);
        sc[p] = d;
        if (d > m) m = d;
    }
    m = wave_max(m);
    if (lane == 0) ((float *) red)[wave] = m;
    __syncthreads();
    m = ((float *) red)[0];
    for (int i = 1; i < 4; i++) { const float x = ((float *) red)[i]; if (x > m) m = x; }
    __syncthreads();
    const float gradTH = (0.5f * m) > 5 ? 0.5f * m : 5;           // :59
    // candidates and their Shi-Tomasi scores (:62-76, FeatureDetector.h:49-82)
    float smax = 0;
    for (int p = tid; p < g * g; p += 256) {
        unsigned k = 0;
        if (sc[p] > gradTH) {
            const int x = p % g, y = p / g, u = x0 + x, v = y0 + y;
            float s = 0.0f;
            if (!(u - 4 < 1 || u + 4 >= w - 1 || v - 4 < 1 || v + 4 >= h - 1)) {
                float dXX = 0.0f, dYY = 0.0f, dXY = 0.0f;
                for (int yy = 0; yy < 8; yy++) {
                    const float *rx = pdx + (y + yy) * P + x, *ry = pdy + (y + yy) * P + x;
#pragma unroll
                    for (int xx = 0; xx < 8; xx++) {
                        const float dx = rx[xx], dy = ry[xx];
                        dXX += dx * dx; dYY += dy * dy; dXY += dx * dy;
                    }
                }
                dXX = (float) (dXX / (2.0 * 64)); dYY = (float) (dYY / (2.0 * 64)); dXY = (float) (dXY / (2.0 * 64));
                // float arithmetic as the expression is typed; the square root resolves to the float overload
                s = (float) (0.5 * (dXX + dYY - sqrtf((dXX + dYY) * (dXX + dYY) - 4 * (dXX * dYY - dXY * dXY))));
            }
            if (!isfinite(s)) bad = true;
            if (s > smax) smax = s;
            sc[p] = s;
            k = feat_key(s);
        }
        key[p] = k;
    }
    smax = wave_max(smax);
    if (lane == 0 && smax > 0) atomicMax(&A.ctl[0], __float_as_int(smax));
    report_nonfinite(bad, &A.ctl[1]);
    __syncthreads();
    // the k best: score descending, equal scores lower idx first (:78-92)
    int picked = 0;
    for (int r = 0; r < A.G.perCell; r++) {
        unsigned long long best = 0;
        for (int p = tid; p < g * g; p += 256) {
            const unsigned long long c = argmax_key(key[p], p);
            if (key[p] && c > best) best = c;
        }
        best = wave_max(best);
        if (lane == 0) red[wave] = best;
        __syncthreads();
        best = red[0];
        for (int i = 1; i < 4; i++) if (red[i] > best) best = red[i];
        __syncthreads();
        if (best == 0) break;
        const int idx = argmax_index(best);
        if (tid == 0) {
            ldso_feature_t f;
            memset(&f, 0, sizeof(f));
            f.u = (float) (x0 + idx % g); f.v = (float) (y0 + idx / g); f.score = sc[idx]; f.cell = gx * A.G.gridY + gy;
            A.cellFeat[(size_t) cell * A.G.perCell + r] = f;
            key[idx] = 0;
        }
        picked++;
        __syncthreads();
    }
    if (tid == 0) A.cellCount[cell] = picked;
}
__global__ __launch_bounds__(256) void k_feat_cells(FeatArgs A) { feat_cells(A, (int) blockIdx.x); }

// one workgroup of 256: exclusive prefix sum of the cells' counts, features to their places in the reference's order
static __device__ __forceinline__ void feat_compact(const FeatArgs &A, int nCells) {
    __shared__ int part[256];
    const Segment s = segment_scan256(A.cellCount, nCells, part, &A.ctl[2]);
    const float maxScore = __int_as_float(A.ctl[0]);
    const float scoreTH = (float) (0.01 * (double) maxScore);     // :98
    int off = s.off;
    for (int c = s.b; c < s.e; c++) {
        const int n = A.cellCount[c];
        for (int r = 0; r < n; r++) {
            ldso_feature_t f = A.cellFeat[(size_t) c * A.G.perCell + r];
            f.is_corner = f.score > scoreTH ? 1 : 0;               // candidate (:100-105); k_feat_corners decides
            A.feat[off + r] = f;
        }
        off += n;
    }
}
__global__ __launch_bounds__(256) void k_feat_compact(FeatArgs A, int nCells) { feat_compact(A, nCells); }

// :107-118 - feature i stays a corner unless a candidate j within 5 pixels has a larger score, or an equal one and j > i
// ... for workgroup `block` of A (256 features each)
static __device__ __forceinline__ void feat_corners(const FeatArgs &A, int block) {
    __shared__ float tu[256], tv[256], ts[256];
    __shared__ int tc[256];
    const int n = A.ctl[2], i = block * 256 + threadIdx.x;
    if (block * 256 >= n) return;
    float u = 0, v = 0, s = 0; int cand = 0;
    if (i < n) { u = A.feat[i].u; v = A.feat[i].v; s = A.feat[i].score; cand = A.feat[i].is_corner; }
    bool lost = false;
    for (int t = 0; t < n; t += 256) {
        const int j = t + threadIdx.x;
        __syncthreads();
        if (j < n) { tu[threadIdx.x] = A.feat[j].u; tv[threadIdx.x] = A.feat[j].v; ts[threadIdx.x] = A.feat[j].score; tc[threadIdx.x] = A.feat[j].is_corner; }
        else tc[threadIdx.x] = 0;
        __syncthreads();
        if (cand) for (int k = 0; k < 256; k++) {
            const int jj = t + k;
            if (!tc[k] || jj == i) continue;
            const int du = (int) u - (int) tu[k], dv = (int) v - (int) tv[k];
            if (du * du + dv * dv < 25 && (ts[k] > s || (ts[k] == s && jj > i))) lost = true;
        }
    }
    __syncthreads();          // every thread has read the candidates' flags of the last tile before any is_corner is overwritten ...
    // ... but other workgroups may still be reading them: the final flag goes to bit 1, k_feat_describe folds it down
    if (i < n) { const int keep = cand && !lost; A.feat[i].is_corner = cand | (keep ? 2 : 0); if (keep) atomicAdd(&A.ctl[3], 1); }
}
__global__ __launch_bounds__(256) void k_feat_corners(FeatArgs A) { feat_corners(A, (int) blockIdx.x); }

// one wavefront per feature: IC_Angle (FeatureDetector.h:91-114) and ComputeDescriptor (FeatureDetector.cc:132-189) of the corners
struct FeatUmax { int v[FEAT_HP + 1]; };
// ... for workgroup `block` of A (4 features each)
static __device__ __forceinline__ void feat_describe(const FeatArgs &A, int block, FeatUmax U) {
    __shared__ float patchAll[4][31 * 31];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = block * 4 + wave, n = A.ctl[2];
    if (i >= n) return;
    ldso_feature_t *F = A.feat + i;
    const int flags = F->is_corner;
    if (lane == 0) F->is_corner = (flags & 2) ? 1 : 0;
    if (!(flags & 2)) return;
    const int w = A.w, h = A.h, cu = (int) F->u, cv = (int) F->v;
    float *patch = patchAll[wave];
    bool bad = false;
    for (int p = lane; p < 31 * 31; p += 64) {
        const int x = cu - FEAT_HP + p % 31, y = cv - FEAT_HP + p / 31;
        float I = 0;
        if (x >= 0 && x < w && y >= 0 && y < h) I = A.img[3 * ((size_t) y * w + x)];
        if (!isfinite(I)) bad = true;
        patch[p] = I;
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    float angle = 0;
    if (lane == 0) {
        const float *center = patch + FEAT_HP * 31 + FEAT_HP;
        float m_01 = 0, m_10 = 0;
        for (int u = -FEAT_HP; u <= FEAT_HP; ++u) m_10 += u * center[u];
        for (int v = 1; v <= FEAT_HP; ++v) {
            float v_sum = 0;
            const int d = U.v[v];
            for (int u = -d; u <= d; ++u) {
                const float val_plus = center[u + v * 31], val_minus = center[u - v * 31];
                v_sum += (val_plus - val_minus);
                m_10 += u * (val_plus + val_minus);
            }
            m_01 += v * v_sum;
        }
        angle = atan2f(m_01, m_10);
        F->angle = angle;
    }
    angle = __shfl(angle, 0, 64);
    report_nonfinite(bad || !isfinite(angle), &A.ctl[1]);
    if (!A.pattern) return;
    const float factorPI = (float) (3.1415926535897932384626433832795 / 180.f);
    const float ang = angle * factorPI;                            // the reference converts the radian value once more (:136): followed
    const float a = cosf(ang), b = sinf(ang);
    unsigned long long *out = (unsigned long long *) F->descriptor;
    for (int pass = 0; pass < 4; pass++) {
        const int32_t *pt = A.pattern + 4 * (pass * 64 + lane);
        int t[2];
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const int p0 = pt[2 * k], p1 = pt[2 * k + 1];
            const int y = cv + (int) (p0 * b + p1 * a), x = cu + (int) (p0 * a - p1 * b);
            float I = 0;
            if (x >= 0 && x < w && y >= 0 && y < h) I = A.img[3 * ((size_t) y * w + x)];
            t[k] = isfinite(I) ? (int) I : 0;
        }
        const unsigned long long bits = __ballot(t[0] < t[1]);
        if (lane == 0) out[pass] = bits;
    }
}
__global__ __launch_bounds__(256) void k_feat_describe(FeatArgs A, FeatUmax U) { feat_describe(A, (int) blockIdx.x, U); }

// ImmaturePoint::ImmaturePoint (ImmaturePoint.cc:14-38), type 1: immature_record.h
static __device__ __forceinline__ void feat_records(const FeatArgs &A, int block) {
    const int i = block * 256 + threadIdx.x, n = A.ctl[2];
    if (i >= n) return;
    bool bad = false;
    A.imm[i] = imm_record(A.img, A.feat[i].u, A.feat[i].v, A.w, A.h, A.hostIndex, bad);
    if (bad) atomicOr(&A.ctl[1], SEL_FLAG_NONFINITE);
}
__global__ __launch_bounds__(256) void k_feat_records(FeatArgs A) { feat_records(A, (int) blockIdx.x); }

// ---------------------------------------------------------------------------------------------------------
// The detections of a group of detectors (ldso_feat_group_*, below) in five launches: a launch runs one of the bodies above for the units of all jobs.
// first[j] = the units in front of job j, first[nJobs] = the grid; units per job: cells nx * ny workgroups, compaction 1 (0 for a grid without cells), corners
// and records ceil(capacity / 256), angle + descriptor ceil(capacity / 4).  Workgroup u serves the job group_member_of finds as that job's unit u - first[j]:
// the same body on the same bytes as the job's own solo kernel.  Job index and unit are uniform (blockIdx), and the row is copied before the first store of
// the kernel, so its pointers stay in scalar registers.
// ---------------------------------------------------------------------------------------------------------
// a row of the job table as the kernels read it: FeatArgs with its pointers typed as device memory (group_member.h: LD_GLOBAL)
struct FeatArgsDev {
    LD_GLOBAL const float *img; int w, h;
    FeatGrid G;
    LD_GLOBAL const float *B;
    LD_GLOBAL const int32_t *pattern;
    LD_GLOBAL ldso_feature_t *cellFeat; LD_GLOBAL int32_t *cellCount;
    LD_GLOBAL ldso_feature_t *feat; LD_GLOBAL ldso_immature_t *imm;
    LD_GLOBAL int32_t *ctl;
    LD_GLOBAL ldso_immature_t *appendPts;
    LD_GLOBAL float *appendType;
    int hostIndex;
};
static_assert(sizeof(FeatArgsDev) == sizeof(FeatArgs) && offsetof(FeatArgsDev, G) == offsetof(FeatArgs, G) && offsetof(FeatArgsDev, B) == offsetof(FeatArgs, B) &&
              offsetof(FeatArgsDev, ctl) == offsetof(FeatArgs, ctl) && offsetof(FeatArgsDev, hostIndex) == offsetof(FeatArgs, hostIndex), "FeatArgsDev is FeatArgs");
static_assert(sizeof(FeatArgs) == 128, "the row of feat_group_layout as tests/test_feat_group_abi_cpu.py sizes it");

static __device__ __forceinline__ FeatArgs feat_job_of(const FeatArgs *jobs, const int *first, int nJobs, int &unit) {
    const int u = (int) blockIdx.x;
    const int j = group_member_of(first, nJobs, u);
    unit = u - first[j];
    const FeatArgsDev D = ((const FeatArgsDev *) jobs)[j];
    FeatArgs A;
    A.img = (const float *) D.img; A.w = D.w; A.h = D.h; A.G = D.G; A.B = (const float *) D.B; A.pattern = (const int32_t *) D.pattern;
    A.cellFeat = (ldso_feature_t *) D.cellFeat; A.cellCount = (int32_t *) D.cellCount; A.feat = (ldso_feature_t *) D.feat; A.imm = (ldso_immature_t *) D.imm;
    A.ctl = (int32_t *) D.ctl; A.appendPts = (ldso_immature_t *) D.appendPts; A.appendType = (float *) D.appendType; A.hostIndex = D.hostIndex;
    return A;
}

__global__ __launch_bounds__(256) void k_feat_cells_group(const FeatArgs *__restrict__ jobs, const int *__restrict__ first, int nJobs) {
    int unit;
    const FeatArgs A = feat_job_of(jobs, first, nJobs, unit);
    feat_cells(A, unit);
}
__global__ __launch_bounds__(256) void k_feat_compact_group(const FeatArgs *__restrict__ jobs, const int *__restrict__ first, int nJobs) {
    int unit;
    const FeatArgs A = feat_job_of(jobs, first, nJobs, unit);
    feat_compact(A, A.G.nx * A.G.ny);
}
__global__ __launch_bounds__(256) void k_feat_corners_group(const FeatArgs *__restrict__ jobs, const int *__restrict__ first, int nJobs) {
    int unit;
    const FeatArgs A = feat_job_of(jobs, first, nJobs, unit);
    feat_corners(A, unit);
}
__global__ __launch_bounds__(256) void k_feat_describe_group(const FeatArgs *__restrict__ jobs, const int *__restrict__ first, int nJobs, FeatUmax U) {
    int unit;
    const FeatArgs A = feat_job_of(jobs, first, nJobs, unit);
    feat_describe(A, unit, U);
}
__global__ __launch_bounds__(256) void k_feat_records_group(const FeatArgs *__restrict__ jobs, const int *__restrict__ first, int nJobs) {
    int unit;
    const FeatArgs A = feat_job_of(jobs, first, nJobs, unit);
    feat_records(A, unit);
}
// ldso_trace_append_points_device of every job with a tracer, over the prefix table of the records launch: workgroup `unit` copies the job's records
// [256 unit, 256 unit + 256) below its count behind the tracer's own, 8 lanes x 16 B per 128-byte record, and writes their my_type = 1 (FullSystem.cc:1281)
__global__ __launch_bounds__(256) void k_feat_append_group(const FeatArgs *__restrict__ jobs, const int *__restrict__ first, int nJobs) {
    int unit;
    const FeatArgs A = feat_job_of(jobs, first, nJobs, unit);
    if (!A.appendPts) return;
    static_assert(sizeof(ldso_immature_t) == 128, "a record is eight 16-byte parts");
    const int n = A.ctl[2], tid = threadIdx.x, part = tid & 7;
    for (int r = unit * 256 + (tid >> 3); r < min(n, unit * 256 + 256); r += 32) ((uint4 *) (A.appendPts + r))[part] = ((const uint4 *) (A.imm + r))[part];
    const int i = unit * 256 + tid;
    if (i < n) A.appendType[i] = 1.0f;
}

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
struct ldso_features {
    int device = 0, w = 0, h = 0, maxFeat = 0, n = 0, nCorners = 0;
    hipStream_t stream = nullptr;
    bool ownStream = false, hasPattern = false, hasB = false;
    const void *inGroup = nullptr;      // the ldso_feat_group this detector belongs to (at most one; ldso_feat_destroy refuses while set: the group dereferences its members)
    int32_t *d_pattern = nullptr, *d_cellCount = nullptr, *d_ctl = nullptr;
    float *d_B = nullptr;
    ldso_feature_t *d_cellFeat = nullptr, *d_feat = nullptr;
    ldso_immature_t *d_imm = nullptr;
    FeatUmax umax;
    StageClock<4> clock;                // cells + compaction, corners, angle + descriptor, records
};

// FeatureDetector::FeatureDetector (FeatureDetector.cc:10-28); cvFloor / cvCeil / cvRound = floor / ceil / round-half-even of a double
static FeatUmax feat_umax() {
    FeatUmax U;
    int v, v0;
    const int vmax = (int) std::floor(FEAT_HP * sqrt(2.f) / 2 + 1), vmin = (int) std::ceil(FEAT_HP * sqrt(2.f) / 2);
    const double hp2 = FEAT_HP * FEAT_HP;
    for (v = 0; v <= FEAT_HP; ++v) U.v[v] = 0;
    for (v = 0; v <= vmax; ++v) U.v[v] = (int) std::nearbyint(sqrt(hp2 - v * v));
    for (v = FEAT_HP, v0 = 0; v >= vmin; --v) {
        while (U.v[v0] == U.v[v0 + 1]) ++v0;
        U.v[v] = v0;
        ++v0;
    }
    return U;
}

// one detection as the kernels read it: the detector's own buffers, level 0 of the pyramid, the control words at `ctl` (the detector's, or its row of a group's block); every byte set
static FeatArgs feat_args(const ldso_features *F, const ldso_pyramid *pyr, const FeatGrid &G, int host_index, int32_t *ctl) {
    FeatArgs A;
    memset(&A, 0, sizeof(A));
    A.img = pyr->lv[0]; A.w = F->w; A.h = F->h; A.G = G; A.B = F->hasB ? F->d_B : nullptr; A.pattern = F->hasPattern ? F->d_pattern : nullptr;
    A.cellFeat = F->d_cellFeat; A.cellCount = F->d_cellCount; A.feat = F->d_feat; A.imm = F->d_imm; A.ctl = ctl; A.hostIndex = host_index;
    return A;
}
// the dynamic LDS of k_feat_cells for a grid
static size_t feat_cells_lds(const FeatGrid &G) { const int P = G.gridsize + 8; return (size_t) (16 + 2 * P * P + 2 * G.gridsize * G.gridsize) * 4; }

extern "C" {

int ldso_feat_grid(int w, int h, int n, int *gridsize, int *gridX, int *gridY, int *skip, int *per_cell, int *capacity) {
    REQ(w > 0 && h > 0 && n > 0 && (long long) w * h < (1ll << 30) && n <= w * h, "ldso_feat_grid: bad arguments (0 < n <= w * h)");
    const FeatGrid G = feat_grid(w, h, n);
    if (gridsize) *gridsize = G.gridsize;
    if (gridX) *gridX = G.gridX;
    if (gridY) *gridY = G.gridY;
    if (skip) *skip = G.skip;
    if (per_cell) *per_cell = G.perCell;
    if (capacity) *capacity = G.nx * G.ny * G.perCell;
    return LDSO_OK;
}

int ldso_feat_destroy(ldso_features_t *F) {
    if (!F) return LDSO_OK;
    REQ(F->inGroup == nullptr, "ldso_feat_destroy: the detector is a member of a live group (ldso_feat_group_destroy first: the group dereferences its members)");
    hipSetDevice(F->device);
    hipDeviceSynchronize();
    hipFree(F->d_pattern); hipFree(F->d_cellCount); hipFree(F->d_ctl); hipFree(F->d_B); hipFree(F->d_cellFeat); hipFree(F->d_feat); hipFree(F->d_imm);
    F->clock.destroy();
    if (F->ownStream && F->stream) hipStreamDestroy(F->stream);
    delete F;
    return LDSO_OK;
}

int ldso_feat_create(int device, int w, int h, int max_features, const int32_t *orb_pattern, ldso_features_t **out) {
    REQ(out && w > 16 && h > 16 && max_features > 0 && (long long) w * h < (1ll << 30), "ldso_feat_create: bad arguments");
    RUN(open_device(device, "ldso_feat_create"));
    ldso_features *F = new ldso_features();
    F->device = device; F->w = w; F->h = h; F->maxFeat = max_features; F->umax = feat_umax();
    const size_t m = (size_t) max_features;
    bool ok = hipStreamCreateWithFlags(&F->stream, hipStreamNonBlocking) == hipSuccess;
    F->ownStream = ok;
    ok = ok && hipMalloc(&F->d_pattern, 1024 * 4) == hipSuccess && hipMalloc(&F->d_B, 256 * 4) == hipSuccess && hipMalloc(&F->d_ctl, 8 * 4) == hipSuccess
         && hipMalloc(&F->d_cellCount, m * 4) == hipSuccess && hipMalloc(&F->d_cellFeat, m * sizeof(ldso_feature_t)) == hipSuccess
         && hipMalloc(&F->d_feat, m * sizeof(ldso_feature_t)) == hipSuccess && hipMalloc(&F->d_imm, m * sizeof(ldso_immature_t)) == hipSuccess;
    ok = ok && F->clock.create() == LDSO_OK;
    if (ok && orb_pattern) { ok = hipMemcpy(F->d_pattern, orb_pattern, 1024 * 4, hipMemcpyHostToDevice) == hipSuccess; F->hasPattern = true; }
    if (!ok) { ldso_feat_destroy(F); ldso_set_error("ldso_feat_create: out of device memory"); return LDSO_E_HIP; }
    *out = F;
    return LDSO_OK;
}

int ldso_feat_set_stream(ldso_features_t *F, void *s) {
    REQ(F, "ldso_feat_set_stream: null handle");
    return swap_stream(F->stream, F->ownStream, s);
}

int ldso_feat_set_response(ldso_features_t *F, const float *B) {
    REQ(F, "ldso_feat_set_response: null handle");
    CHK(hipSetDevice(F->device));
    if (B) { CHK(hipMemcpyAsync(F->d_B, B, 256 * 4, hipMemcpyHostToDevice, F->stream)); CHK(hipStreamSynchronize(F->stream)); }
    F->hasB = B != nullptr;
    return LDSO_OK;
}

int ldso_feat_profile(ldso_features_t *F, int enable, float us_out[4]) {
    REQ(F, "ldso_feat_profile: null handle");
    return F->clock.report(F->device, enable, us_out);
}

int ldso_feat_detect(ldso_features_t *F, ldso_pyramid_t *pyr, int n_features, int host_index, int *n_features_out, int *n_corners_out) {
    REQ(F && pyr, "ldso_feat_detect: null argument");
    REQ(n_features > 0 && n_features <= F->w * F->h, "ldso_feat_detect: n_features out of range");
    const FeatGrid G = feat_grid(F->w, F->h, n_features);
    const int nCells = G.nx * G.ny;
    REQ(nCells * G.perCell <= F->maxFeat, "ldso_feat_detect: the grid's capacity (ldso_feat_grid) exceeds max_features");
    if (G.gridsize > FEAT_MAX_GRID) { ldso_set_error("ldso_feat_detect: gridsize above 64 (too few features for this image size)"); return LDSO_E_UNSUPPORTED; }
    hipStream_t st = F->stream;
    RUN(pyramid_wait(pyr, F->device, F->w, F->h, 1, st, "ldso_feat_detect", "the detector (device, size)"));
    CHK(hipMemsetAsync(F->d_ctl, 0, 8 * 4, st));
    const FeatArgs A = feat_args(F, pyr, G, host_index, F->d_ctl);
    StageClock<4> &clk = F->clock.begin();
    RUN(clk.mark(0, st));
    if (nCells > 0) {
        CHK(launch_lds(k_feat_cells, dim3(nCells), dim3(256), feat_cells_lds(G), st, A));
        hipLaunchKernelGGL(k_feat_compact, dim3(1), dim3(256), 0, st, A, nCells);
        CHK(hipGetLastError());
    }
    RUN(clk.mark(1, st));
    // the launches below are sized for the capacity; the kernels read the count from the device
    const int cap = nCells * G.perCell;
    if (cap > 0) {
        hipLaunchKernelGGL(k_feat_corners, dim3((cap + 255) / 256), dim3(256), 0, st, A);
        CHK(hipGetLastError());
        RUN(clk.mark(2, st));
        hipLaunchKernelGGL(k_feat_describe, dim3((cap + 3) / 4), dim3(256), 0, st, A, F->umax);
        CHK(hipGetLastError());
        RUN(clk.mark(3, st));
        hipLaunchKernelGGL(k_feat_records, dim3((cap + 255) / 256), dim3(256), 0, st, A);
        CHK(hipGetLastError());
    } else { RUN(clk.mark(2, st)); RUN(clk.mark(3, st)); }
    RUN(clk.mark(4, st));
    int ctl[8] = {0};
    CHK(hipMemcpyAsync(ctl, F->d_ctl, 8 * 4, hipMemcpyDeviceToHost, st));
    CHK(hipStreamSynchronize(st));
    RUN(clk.read());
    F->n = ctl[2]; F->nCorners = ctl[3];
    if (n_features_out) *n_features_out = F->n;
    if (n_corners_out) *n_corners_out = F->nCorners;
    if (ctl[1] & SEL_FLAG_NONFINITE) { ldso_set_error("ldso_feat_detect: non-finite pixel, score, angle or colour"); return LDSO_E_NONFINITE; }
    return LDSO_OK;
}

int ldso_feat_get(ldso_features_t *F, ldso_feature_t *out, ldso_immature_t *imm_out) {
    REQ(F && (F->n == 0 || out), "ldso_feat_get: bad arguments");
    CHK(hipSetDevice(F->device));
    if (F->n) {
        CHK(hipMemcpyAsync(out, F->d_feat, (size_t) F->n * sizeof(ldso_feature_t), hipMemcpyDeviceToHost, F->stream));
        if (imm_out) CHK(hipMemcpyAsync(imm_out, F->d_imm, (size_t) F->n * sizeof(ldso_immature_t), hipMemcpyDeviceToHost, F->stream));
    }
    CHK(hipStreamSynchronize(F->stream));
    return LDSO_OK;
}

int ldso_feat_device(ldso_features_t *F, const void **features_dev, const void **immature_dev, int *n) {
    REQ(F, "ldso_feat_device: null handle");
    if (features_dev) *features_dev = F->d_feat;
    if (immature_dev) *immature_dev = F->d_imm;
    if (n) *n = F->n;
    return LDSO_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------
// ldso_feat_group_* (include/ldso_hip.h): FullSystem::makeNewTraces (FullSystem.cc:1272-1325, setting_pointSelection == 1) of several detectors (independent
// sequences on one card) in five launches, six with the append.  The members stay ordinary detectors and keep their own buffers; the group owns the staging
// arena of its launches (feat_group_layout, group_stage.h), the control rows in it, and its profiling events.
// ---------------------------------------------------------------------------------------------------------
struct ldso_feat_group {
    std::vector<ldso_features *> m;
    int device = 0;
    GroupArena arena;
    FeatUmax umax;
    StageClock<5> clock;                // the four stages of a detector, then the append
};

namespace {

constexpr GroupRule FEAT_RULE = {"a detector", "ldso_feat_set_stream", GROUP_MAX_MEMBERS};

template <class Kernel, class... Args>
hipError_t feat_launch_group(Kernel kernel, int units, hipStream_t st, const Args &... args) {
    if (units <= 0) return hipSuccess;
    hipLaunchKernelGGL(kernel, dim3(units), dim3(256), 0, st, args...);
    return hipGetLastError();
}

}  // namespace

extern "C" {

int ldso_feat_group_destroy(ldso_feat_group_t *g) {
    if (!g) return LDSO_OK;
    hipSetDevice(g->device);
    if (g->arena.h_stage && !g->m.empty()) hipStreamSynchronize(g->m[0]->stream);
    group_leave(g);
    group_arena_free(g->arena);
    g->clock.destroy();
    delete g;
    return LDSO_OK;
}

int ldso_feat_group_create(ldso_features_t *const *members, int n, ldso_feat_group_t **out) {
    RUN(group_admit(members, n, out, "ldso_feat_group_create", FEAT_RULE));
    CHK(hipSetDevice(members[0]->device));
    ldso_feat_group *g = new ldso_feat_group();
    g->device = members[0]->device; g->umax = feat_umax();
    const bool ok = g->clock.create() == LDSO_OK;
    if (!ok) ldso_set_error("ldso_feat_group_create: hipEventCreate failed");
    RUN(finish_create(ok ? LDSO_OK : LDSO_E_HIP, g, out, ldso_feat_group_destroy));          // the arena comes with the first call
    g->m.assign(members, members + n);
    group_join(g);
    return LDSO_OK;
}

int ldso_feat_group_profile(ldso_feat_group_t *g, int enable, float us_out[5]) {
    REQ(g, "ldso_feat_group_profile: null group");
    return g->clock.report(g->device, enable, us_out);
}

// ldso_feat_detect (+ ldso_trace_append_points_device) of every active member: ONE upload of [FeatArgs table | four prefix tables | zeroed control rows], five or
// six launches, ONE download of the control rows, one wait; the members' and tracers' host state changes behind the wait only
int ldso_feat_group_detect(ldso_feat_group_t *g, const uint8_t *active, ldso_pyramid_t *const *pyr, const int *n_features, const int *host_index, ldso_tracer_t *const *tracers,
                           int *n_features_out, int *n_corners_out, int *status_out) {
    const char *who = "ldso_feat_group_detect";
    REQ(g && pyr && n_features && host_index, "ldso_feat_group_detect: null argument");
    RUN(group_check(g->m.data(), g->m.size(), who, FEAT_RULE));
    const int n = (int) g->m.size();
    std::vector<FeatGrid> grid((size_t) n);
    std::vector<int> members;
    int unsupported = -1;
    RUN(group_active(n, active, who, members, [&](int i) -> const char * {
        const ldso_features *F = g->m[(size_t) i];
        if (!pyr[i]) return "null pyramid";
        if (!(n_features[i] > 0 && n_features[i] <= F->w * F->h)) return "n_features out of range";
        const FeatGrid G = feat_grid(F->w, F->h, n_features[i]);
        grid[(size_t) i] = G;
        const int cap = G.nx * G.ny * G.perCell;
        if (cap > F->maxFeat) return "the grid's capacity (ldso_feat_grid) exceeds max_features";
        if (G.gridsize > FEAT_MAX_GRID && unsupported < 0) unsupported = i;
        const ldso_pyramid *P = pyr[i];
        if (!(P->built && P->device == F->device && P->w == F->w && P->h == F->h && P->levels >= 1)) return "the pyramid does not match the detector (device, size) or holds no image";
        const ldso_tracer *T = tracers ? tracers[i] : nullptr;
        if (T) {
            if (T->device != g->device || (const void *) T->stream != (const void *) g->m[0]->stream) return "the tracer is not on the group's device and stream (ldso_trace_set_stream)";
            if (T->maxPoints - T->n < cap) return "the tracer has no room for the grid's capacity (max_points - n >= the capacity of ldso_feat_grid)";
            for (int k : members) if (tracers[k] == T) return "the same tracer as an earlier member";
        }
        return nullptr;
    }));
    if (unsupported >= 0) {
        ldso_set_error(std::string(who) + ": member " + std::to_string(unsupported) + ": gridsize above 64 (too few features for this image size)");
        return LDSO_E_UNSUPPORTED;
    }
    CHK(hipSetDevice(g->device));
    hipStream_t st = g->m[0]->stream;
    const size_t nj = members.size();
    const FeatGroupLayout L = feat_group_layout(nj, sizeof(FeatArgs));
    RUN(group_arena_grow(g->arena, L.total, st));
    for (int i : members) RUN(pyramid_wait(pyr[i], g->device, g->m[(size_t) i]->w, g->m[(size_t) i]->h, 1, st, who, "the detector (device, size)"));
    char *const h_stage = g->arena.h_stage, *const d_stage = g->arena.d_stage;
    FeatArgs *hJ = (FeatArgs *) (h_stage + L.jobs);
    int *hC = (int *) (h_stage + L.down);
    size_t ldsBytes = 0;
    bool append = false;
    for (size_t j = 0; j < nj; j++) {
        const int i = members[j];
        const ldso_features *F = g->m[(size_t) i];
        const FeatGrid &G = grid[(size_t) i];
        hJ[j] = feat_args(F, pyr[i], G, host_index[i], (int32_t *) (d_stage + L.down) + 8 * j);
        if (tracers && tracers[i]) { hJ[j].appendPts = tracers[i]->d_pts + tracers[i]->n; hJ[j].appendType = tracers[i]->d_type + tracers[i]->n; append = true; }
        if (G.nx * G.ny > 0) ldsBytes = std::max(ldsBytes, feat_cells_lds(G));
    }
    const auto gridOf = [&](int j) -> const FeatGrid & { return grid[(size_t) members[(size_t) j]]; };
    const auto capOf = [&](int j) { return gridOf(j).nx * gridOf(j).ny * gridOf(j).perCell; };
    const int uCells = group_prefix((int) nj, (int *) (h_stage + L.firstCells), [&](int j) { return gridOf(j).nx * gridOf(j).ny; });
    const int uCompact = group_prefix((int) nj, (int *) (h_stage + L.firstCompact), [&](int j) { return gridOf(j).nx * gridOf(j).ny > 0 ? 1 : 0; });
    const int uCorners = group_prefix((int) nj, (int *) (h_stage + L.firstCorners), [&](int j) { return (capOf(j) + 255) / 256; });
    const int uDescribe = group_prefix((int) nj, (int *) (h_stage + L.firstDescribe), [&](int j) { return (capOf(j) + 3) / 4; });
    memset(hC, 0, L.downBytes);
    CHK(hipMemcpyAsync(d_stage, h_stage, L.total, hipMemcpyHostToDevice, st));
    const FeatArgs *dJ = (const FeatArgs *) (d_stage + L.jobs);
    const int *dCells = (const int *) (d_stage + L.firstCells), *dCompact = (const int *) (d_stage + L.firstCompact), *dCorners = (const int *) (d_stage + L.firstCorners),
              *dDescribe = (const int *) (d_stage + L.firstDescribe);
    StageClock<5> &clk = g->clock.begin();
    const int J = (int) nj;
    RUN(clk.mark(0, st));
    if (uCells > 0) CHK(launch_lds(k_feat_cells_group, dim3(uCells), dim3(256), ldsBytes, st, dJ, dCells, J));
    CHK(feat_launch_group(k_feat_compact_group, uCompact, st, dJ, dCompact, J));
    RUN(clk.mark(1, st));
    // the launches below are sized for the capacities; the kernels read the counts from the device
    CHK(feat_launch_group(k_feat_corners_group, uCorners, st, dJ, dCorners, J));
    RUN(clk.mark(2, st));
    CHK(feat_launch_group(k_feat_describe_group, uDescribe, st, dJ, dDescribe, J, g->umax));
    RUN(clk.mark(3, st));
    CHK(feat_launch_group(k_feat_records_group, uCorners, st, dJ, dCorners, J));
    RUN(clk.mark(4, st));
    if (append) CHK(feat_launch_group(k_feat_append_group, uCorners, st, dJ, dCorners, J));
    RUN(clk.mark(5, st));
    CHK(hipMemcpyAsync(hC, d_stage + L.down, L.downBytes, hipMemcpyDeviceToHost, st));
    CHK(hipStreamSynchronize(st));
    RUN(clk.read());
    int firstBad = -1;
    for (size_t j = 0; j < nj; j++) {
        const int i = members[j], *ctl = hC + 8 * j;
        ldso_features *F = g->m[(size_t) i];
        F->n = ctl[2]; F->nCorners = ctl[3];
        if (tracers && tracers[i]) tracers[i]->n += ctl[2];
        const bool bad = (ctl[1] & SEL_FLAG_NONFINITE) != 0;
        if (bad && firstBad < 0) firstBad = i;
        if (n_features_out) n_features_out[i] = ctl[2];
        if (n_corners_out) n_corners_out[i] = ctl[3];
        if (status_out) status_out[i] = bad ? LDSO_E_NONFINITE : LDSO_OK;
    }
    if (firstBad >= 0) {
        ldso_set_error(std::string(who) + ": member " + std::to_string(firstBad) + ": non-finite pixel, score, angle or colour");
        return LDSO_E_NONFINITE;
    }
    return LDSO_OK;
}

// ldso_feat_get of every active member: exactly-sized copies on the group's stream, one wait
int ldso_feat_group_get(ldso_feat_group_t *g, const uint8_t *active, ldso_feature_t *const *features_out, ldso_immature_t *const *immature_out) {
    const char *who = "ldso_feat_group_get";
    REQ(g, "ldso_feat_group_get: null group");
    RUN(group_check(g->m.data(), g->m.size(), who, FEAT_RULE));
    std::vector<int> members;
    RUN(group_active((int) g->m.size(), active, who, members, [&](int) -> const char * { return nullptr; }));
    CHK(hipSetDevice(g->device));
    hipStream_t st = g->m[0]->stream;
    for (int i : members) {
        const ldso_features *F = g->m[(size_t) i];
        if (F->n == 0) continue;
        if (features_out && features_out[i]) CHK(hipMemcpyAsync(features_out[i], F->d_feat, (size_t) F->n * sizeof(ldso_feature_t), hipMemcpyDeviceToHost, st));
        if (immature_out && immature_out[i]) CHK(hipMemcpyAsync(immature_out[i], F->d_imm, (size_t) F->n * sizeof(ldso_immature_t), hipMemcpyDeviceToHost, st));
    }
    CHK(hipStreamSynchronize(st));
    return LDSO_OK;
}

}  // extern "C"
