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
//
// Every float expression keeps the reference's operand order and width (the library is built with -ffp-contract=off).  Where the reference would read
// outside the image (descriptor / moment taps of a feature near the right or bottom border, possible at gridsize 16..18 and from 31 on; it has no check) a tap reads 0 here, and
// an immature record whose taps leave the image gets a NaN colour and energyTH = NaN.  Rows 0 and h-1 have zero gradients (images.hip).
#include "ba_host.h"
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
    int hostIndex;
};

// orderable key of a candidate's score: larger score = larger key, NaN below every number, 0 = no candidate
static __device__ __forceinline__ unsigned feat_key(float s) {
    if (s != s) return 1u;
    if (s == 0.0f) s = 0.0f;            // -0 == +0
    const unsigned u = (unsigned) __float_as_int(s);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(256) void k_feat_cells(FeatArgs A) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int g = A.G.gridsize, P = g + 8, w = A.w, h = A.h, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned long long *red = (unsigned long long *) lds;          // [8] cross-wave scratch
    float *pdx = lds + 16, *pdy = pdx + P * P, *sc = pdy + P * P;
    unsigned *key = (unsigned *) (sc + g * g);
    const int cell = blockIdx.x, gx = A.G.skip + cell / A.G.ny, gy = A.G.skip + cell % A.G.ny;
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

// one workgroup of 256: exclusive prefix sum of the cells' counts, features to their places in the reference's order
__global__ __launch_bounds__(256) void k_feat_compact(FeatArgs A, int nCells) {
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

// :107-118 - feature i stays a corner unless a candidate j within 5 pixels has a larger score, or an equal one and j > i
__global__ __launch_bounds__(256) void k_feat_corners(FeatArgs A) {
    __shared__ float tu[256], tv[256], ts[256];
    __shared__ int tc[256];
    const int n = A.ctl[2], i = blockIdx.x * 256 + threadIdx.x;
    if (blockIdx.x * 256 >= n) return;
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

// one wavefront per feature: IC_Angle (FeatureDetector.h:91-114) and ComputeDescriptor (FeatureDetector.cc:132-189) of the corners
struct FeatUmax { int v[FEAT_HP + 1]; };
__global__ __launch_bounds__(256) void k_feat_describe(FeatArgs A, FeatUmax U) {
    __shared__ float patchAll[4][31 * 31];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x * 4 + wave, n = A.ctl[2];
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

// ImmaturePoint::ImmaturePoint (ImmaturePoint.cc:14-38), type 1: immature_record.h
__global__ __launch_bounds__(256) void k_feat_records(FeatArgs A) {
    const int i = blockIdx.x * 256 + threadIdx.x, n = A.ctl[2];
    if (i >= n) return;
    bool bad = false;
    A.imm[i] = imm_record(A.img, A.feat[i].u, A.feat[i].v, A.w, A.h, A.hostIndex, bad);
    if (bad) atomicOr(&A.ctl[1], SEL_FLAG_NONFINITE);
}

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
struct ldso_features {
    int device = 0, w = 0, h = 0, maxFeat = 0, n = 0, nCorners = 0;
    hipStream_t stream = nullptr;
    bool ownStream = false, hasPattern = false, hasB = false, profile = false;
    int32_t *d_pattern = nullptr, *d_cellCount = nullptr, *d_ctl = nullptr;
    float *d_B = nullptr;
    ldso_feature_t *d_cellFeat = nullptr, *d_feat = nullptr;
    ldso_immature_t *d_imm = nullptr;
    FeatUmax umax;
    hipEvent_t ev[5] = {};
    float us[4] = {0, 0, 0, 0};
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
    hipSetDevice(F->device);
    hipDeviceSynchronize();
    hipFree(F->d_pattern); hipFree(F->d_cellCount); hipFree(F->d_ctl); hipFree(F->d_B); hipFree(F->d_cellFeat); hipFree(F->d_feat); hipFree(F->d_imm);
    for (hipEvent_t e : F->ev) if (e) hipEventDestroy(e);
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
    for (hipEvent_t &e : F->ev) ok = ok && hipEventCreate(&e) == hipSuccess;
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
    F->profile = enable != 0;
    if (us_out) for (int i = 0; i < 4; i++) us_out[i] = F->us[i];
    return LDSO_OK;
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
    FeatArgs A;
    A.img = pyr->lv[0]; A.w = F->w; A.h = F->h; A.G = G; A.B = F->hasB ? F->d_B : nullptr; A.pattern = F->hasPattern ? F->d_pattern : nullptr;
    A.cellFeat = F->d_cellFeat; A.cellCount = F->d_cellCount; A.feat = F->d_feat; A.imm = F->d_imm; A.ctl = F->d_ctl; A.hostIndex = host_index;
    const bool prof = F->profile;
    if (prof) CHK(hipEventRecord(F->ev[0], st));
    if (nCells > 0) {
        const int P = G.gridsize + 8;
        const size_t ldsBytes = (size_t) (16 + 2 * P * P + 2 * G.gridsize * G.gridsize) * 4;
        CHK(launch_lds(k_feat_cells, dim3(nCells), dim3(256), ldsBytes, st, A));
        hipLaunchKernelGGL(k_feat_compact, dim3(1), dim3(256), 0, st, A, nCells);
        CHK(hipGetLastError());
    }
    if (prof) CHK(hipEventRecord(F->ev[1], st));
    // the launches below are sized for the capacity; the kernels read the count from the device
    const int cap = nCells * G.perCell;
    if (cap > 0) {
        hipLaunchKernelGGL(k_feat_corners, dim3((cap + 255) / 256), dim3(256), 0, st, A);
        CHK(hipGetLastError());
        if (prof) CHK(hipEventRecord(F->ev[2], st));
        hipLaunchKernelGGL(k_feat_describe, dim3((cap + 3) / 4), dim3(256), 0, st, A, F->umax);
        CHK(hipGetLastError());
        if (prof) CHK(hipEventRecord(F->ev[3], st));
        hipLaunchKernelGGL(k_feat_records, dim3((cap + 255) / 256), dim3(256), 0, st, A);
        CHK(hipGetLastError());
    } else if (prof) { CHK(hipEventRecord(F->ev[2], st)); CHK(hipEventRecord(F->ev[3], st)); }
    if (prof) CHK(hipEventRecord(F->ev[4], st));
    int ctl[8] = {0};
    CHK(hipMemcpyAsync(ctl, F->d_ctl, 8 * 4, hipMemcpyDeviceToHost, st));
    CHK(hipStreamSynchronize(st));
    if (prof) for (int i = 0; i < 4; i++) { float ms = 0; CHK(hipEventElapsedTime(&ms, F->ev[i], F->ev[i + 1])); F->us[i] = ms * 1e3f; }
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
