// init_first.hip — CoarseInitializer::setFirst from a resident pyramid (include/ldso_hip.h, "setFirst from a resident pyramid"): makePixelStatus for the
// levels >= 1 (k_ini_gridmax + the host recursion), the Pnt records of every level (k_ini_rows / k_ini_rowscan / k_ini_records), the searches of makeNN over
// the host-built k-d trees (k_ini_nn; the search itself is nn_search.h, the build init_nn_tree.cpp), and ldso_init_set_first_frame, which strings them together
// and hands the finished records to the code behind ldso_init_set_first (initializer_api.hip).
#include <chrono>
#include "initializer.h"
#include "pyramid.h"
#include "nn_search.h"

#define FC_COUNT 0            // d_fctl: pixels set by the gridMaxSelection pass
#define FC_FLAGS 1            // bit 0: a non-finite gradient was read
#define FC_TOTAL 2            // records of the scanned rectangle
#define NN_MAX_DEPTH 64       // 64 lanes x 64 entries x 16 bytes = 64 KB of LDS
#define INI_MAX_POINTS 36000  // ldso_init_set_first's limit per level

// ---------------------------------------------------------------------------------------------------------
// gridMaxSelection (PixelSelector2.h:63-225; the templated variants and the generic one are the same arithmetic): G = 1, 4, 16 or 64 lanes per pot x pot block.
// The reference scans a block with dx in the outer loop and dy in the inner one and keeps the FIRST strict maximum, so among equal values the smallest
// c = dx * pot + dy wins.  A lane walks its cells in ascending c (first strict maximum again); across the lanes the maximum of (value bits, ~c) picks the
// largest value and, among equals, the smallest c.  A value has to exceed the initial best of 0, and a NaN never does.
// ---------------------------------------------------------------------------------------------------------
static __device__ __forceinline__ unsigned long long gm_key(float v, int c) { return ((unsigned long long) (unsigned) __float_as_int(v) << 32) | (unsigned) (0x7fffffff - c); }

__global__ __launch_bounds__(256) void k_ini_gridmax(const float *__restrict__ img, unsigned char *__restrict__ map, int w, int h, int pot, int nbx, int nby, int G, float THFac,
                                                     int *__restrict__ ctl) {
    const long long gid = (long long) blockIdx.x * 256 + threadIdx.x;
    const int sub = (int) (gid % G);
    const long long blk = gid / G;
    const bool live = blk < (long long) nbx * nby;
    const float TH = THFac * 10.0f * 0.75f, TH2 = TH * TH;
    unsigned long long k0 = 0, k1 = 0, k2 = 0, k3 = 0;
    bool bad = false;
    int x0 = 0, y0 = 0;
    if (live) {
        x0 = 1 + (int) (blk % nbx) * pot; y0 = 1 + (int) (blk / nbx) * pot;          // x0 + pot - 1 <= w - 2, y0 + pot - 1 <= h - 2: nbx = (w - 2) / pot
        float b0 = 0, b1 = 0, b2 = 0, b3 = 0;
        for (int c = sub; c < pot * pot; c += G) {
            const int dx = c / pot, dy = c - dx * pot;
            const size_t i = ((size_t) (y0 + dy) * w + (x0 + dx)) * 3;
            const float gx = img[i + 1], gy = img[i + 2];
            bad = bad || !isfinite(gx) || !isfinite(gy);
            const float sqgd = gx * gx + gy * gy;
            if (sqgd > TH2) {
                const float agx = fabsf(gx), agy = fabsf(gy), gxpy = fabsf(gx - gy), gxmy = fabsf(gx + gy);
                if (agx > b0) { b0 = agx; k0 = gm_key(agx, c); }
                if (agy > b1) { b1 = agy; k1 = gm_key(agy, c); }
                if (gxpy > b2) { b2 = gxpy; k2 = gm_key(gxpy, c); }
                if (gxmy > b3) { b3 = gxmy; k3 = gm_key(gxmy, c); }
            }
        }
    }
    for (int o = G >> 1; o > 0; o >>= 1) {          // G divides 64: the butterfly stays inside the block's lanes
        k0 = max(k0, (unsigned long long) __shfl_xor((long long) k0, o, 64)); k1 = max(k1, (unsigned long long) __shfl_xor((long long) k1, o, 64));
        k2 = max(k2, (unsigned long long) __shfl_xor((long long) k2, o, 64)); k3 = max(k3, (unsigned long long) __shfl_xor((long long) k3, o, 64));
    }
    int set = 0;
    if (live && sub == 0) {
        const int c0 = k0 ? 0x7fffffff - (int) (unsigned) k0 : -1, c1 = k1 ? 0x7fffffff - (int) (unsigned) k1 : -1;
        const int c2 = k2 ? 0x7fffffff - (int) (unsigned) k2 : -1, c3 = k3 ? 0x7fffffff - (int) (unsigned) k3 : -1;
        const int cs[4] = {c0, c1, c2, c3};
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int c = cs[q];
            if (c < 0) continue;
            bool seen = false;
#pragma unroll
            for (int r = 0; r < q; r++) seen = seen || cs[r] == c;
            if (seen) continue;
            const int dx = c / pot, dy = c - dx * pot;
            map[(size_t) (y0 + dy) * w + (x0 + dx)] = 1;
            set++;
        }
    }
    for (int o = 32; o > 0; o >>= 1) set += __shfl_xor(set, o, 64);
    const int lane = threadIdx.x & 63;
    if (lane == 0 && set) atomicAdd(&ctl[FC_COUNT], set);
    if (__any(bad) && lane == 0) atomicOr(&ctl[FC_FLAGS], 1);
}

// ---------------------------------------------------------------------------------------------------------
// the records (:567-603): set pixels per row of the scanned rectangle, their prefix sum, one record per set pixel in raster order
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ini_rows(const unsigned char *__restrict__ map, int w, int h, int x0, int x1, int y0, int y1, int *__restrict__ rowCount) {
    const int lane = threadIdx.x & 63, y = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (y >= h) return;
    int c = 0;
    if (y >= y0 && y < y1) for (int x = x0 + lane; x < x1; x += 64) c += map[(size_t) y * w + x] != 0;
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if (lane == 0) rowCount[y] = c;
}

__global__ __launch_bounds__(256) void k_ini_rowscan(const int *__restrict__ rowCount, int *__restrict__ rowStart, int h, int *__restrict__ ctl) {
    __shared__ int part[256];
    const int tid = threadIdx.x, per = (h + 255) / 256, b = min(tid * per, h), e = min(b + per, h);
    int s = 0;
    for (int y = b; y < e; y++) s += rowCount[y];
    part[tid] = s;
    __syncthreads();
    if (tid == 0) { int a = 0; for (int i = 0; i < 256; i++) { const int t = part[i]; part[i] = a; a += t; } ctl[FC_TOTAL] = a; }
    __syncthreads();
    int off = part[tid];
    for (int y = b; y < e; y++) { rowStart[y] = off; off += rowCount[y]; }
}

__global__ __launch_bounds__(256) void k_ini_records(const unsigned char *__restrict__ map, int w, int x0, int x1, int y0, int y1, const int *__restrict__ rowStart, int typeFromMap,
                                                     ldso_init_point_t *__restrict__ rec, float *__restrict__ uv, int cap) {
    const int lane = threadIdx.x & 63, y = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (y < y0 || y >= y1) return;
    int base = rowStart[y];
    for (int xb = x0; xb < x1; xb += 64) {
        const int x = xb + lane;
        const int v = x < x1 ? map[(size_t) y * w + x] : 0;
        const unsigned long long bal = __ballot(v != 0);
        const int r = base + __popcll(bal & ((1ull << lane) - 1));
        if (v != 0 && r < cap) {
            ldso_init_point_t p;
            p.u = (float) (x + 0.1); p.v = (float) (y + 0.1);          // int + double, then rounded to float (:578-579)
            p.idepth = 1.0f; p.iR = 1.0f; p.isGood = 1;
            p.energy[0] = p.energy[1] = 0.0f; p.lastHessian = 0.0f; p.lastHessian_new = 0.0f;
            p.my_type = typeFromMap ? (float) v : 1.0f;
            p.outlierTH = 8 * (12.0f * 12.0f);                         // patternNum * setting_outlierTH (Settings.h: 8; Setting.cc: 12 * 12)
            p.parent = -1; p.parentDist = -1.0f;
#pragma unroll
            for (int q = 0; q < 10; q++) { p.neighbours[q] = -1; p.neighboursDist[q] = 0.0f; }
            LDSO_INIT_POINT_FILL_UNSET(p);
            rec[r] = p;
            uv[2 * r] = p.u; uv[2 * r + 1] = p.v;
        }
        base += __popcll(bal);
    }
}

// ---------------------------------------------------------------------------------------------------------
// makeNN :736-777: one lane per point - the 10 nearest on the point's own level, then the nearest on level + 1 to the halved position.  The result sets are
// registers, the traversal stacks lie interleaved in LDS (entry e of lane t at e * 64 + t).
// ---------------------------------------------------------------------------------------------------------
struct NnTreeDev { const ldso_nn_node_t *nodes; const int *vind; const float *uv; float root[4]; };

__global__ __launch_bounds__(64) void k_ini_nn(NnTreeDev T, NnTreeDev Up, int hasUp, int n, ldso_init_point_t *__restrict__ rec, int32_t *__restrict__ nbIdx, float *__restrict__ nbDist,
                                               int32_t *__restrict__ parIdx, float *__restrict__ parDist) {
    extern __shared__ NnEntry nn_stack[];
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const NnStack st{nn_stack + threadIdx.x, 64};
    const float qx = T.uv[2 * i], qy = T.uv[2 * i + 1];
    NnSet<NN_K> R;
    nn_search<NN_K>(T.nodes, T.vind, T.uv, T.root, qx, qy, st, R);
    int par = -1; float pd = -1.0f;
    if (hasUp) {
        NnSet<1> P;
        nn_search<1>(Up.nodes, Up.vind, Up.uv, Up.root, qx * 0.5f - 0.25f, qy * 0.5f - 0.25f, st, P);
        par = P.i[0]; pd = P.d[0];
    }
    if (nbIdx) {
#pragma unroll
        for (int k = 0; k < NN_K; k++) { nbIdx[(size_t) i * NN_K + k] = R.i[k]; nbDist[(size_t) i * NN_K + k] = R.d[k]; }
    }
    if (parIdx) { parIdx[i] = par; parDist[i] = pd; }
    if (rec) {
        const float NNDistFactor = 0.05f;
        float df[NN_K], sumDF = 0.0f;
#pragma unroll
        for (int k = 0; k < NN_K; k++) { df[k] = expf(-R.d[k] * NNDistFactor); sumDF += df[k]; }
        const float s = 10 / sumDF;                                    // the quotient first (:761)
        ldso_init_point_t *p = rec + i;
#pragma unroll
        for (int k = 0; k < NN_K; k++) { p->neighbours[k] = R.i[k]; p->neighboursDist[k] = df[k] * s; }
        p->parent = par;
        p->parentDist = hasUp ? expf(-pd * NNDistFactor) : -1.0f;
    }
}

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
static int first_buffers(ldso_initializer *H) {
    if (H->d_status) return LDSO_OK;
    DALLOC(H->firstAllocs, H->d_fctl, 4);
    DALLOC(H->firstAllocs, H->d_rowCount, (size_t) H->h);
    DALLOC(H->firstAllocs, H->d_rowStart, (size_t) H->h);
    DALLOC(H->firstAllocs, H->d_status, (size_t) (H->w >> 1) * (H->h >> 1));
    return LDSO_OK;
}

// the records and positions of level l hold at least n entries
static int first_reserve(ldso_initializer *H, int l, int n) {
    if (n <= H->recCap[l]) return LDSO_OK;
    const int cap = std::max(n, 1024);
    H->recCap[l] = 0;          // the old buffers stay in firstAllocs until destroy: a level grows a few times in a handle's life
    DALLOC(H->firstAllocs, H->d_rec[l], (size_t) cap);
    DALLOC(H->firstAllocs, H->d_uv[l], (size_t) cap * 2);
    H->recCap[l] = cap;
    return LDSO_OK;
}

// makePixelStatus on `img` (wl x hl pixels of (I, dx, dy)) into d_status; the stream waits once per pass for the count
static int pixel_status(ldso_initializer *H, const float *img, int wl, int hl, float desired, int recsLeft, float thFac, int *nOut, int *passesOut, int *flagsOut) {
    hipStream_t st = H->stream;
    int passes = 0, n = 0, flags = 0;
    for (;;) {
        if (H->sparsity < 1) H->sparsity = 1;                          // :230
        const int pot = H->sparsity;
        const int nbx = wl - 2 >= pot ? (wl - 2) / pot : 0, nby = hl - 2 >= pot ? (hl - 2) / pot : 0;          // blocks at 1 + i * pot < wl - pot
        const int G = pot <= 1 ? 1 : pot == 2 ? 4 : pot <= 4 ? 16 : 64;
        CHK(hipMemsetAsync(H->d_fctl, 0, 4 * sizeof(int), st));
        CHK(hipMemsetAsync(H->d_status, 0, (size_t) wl * hl, st));
        const long long lanes = (long long) nbx * nby * G;
        if (lanes > 0) {
            hipLaunchKernelGGL(k_ini_gridmax, dim3((unsigned) ((lanes + 255) / 256)), dim3(256), 0, st, img, H->d_status, wl, hl, pot, nbx, nby, G, thFac, H->d_fctl);
            CHK(hipGetLastError());
        }
        int ctl[4] = {0, 0, 0, 0};
        CHK(hipMemcpyAsync(ctl, H->d_fctl, sizeof(ctl), hipMemcpyDeviceToHost, st));
        CHK(hipStreamSynchronize(st));
        passes++; n = ctl[FC_COUNT]; flags |= ctl[FC_FLAGS];
        int act = 0, newSparsity = pot; float newTh = thFac;
        RUN(ldso_init_pixel_status_plan(n, desired, pot, recsLeft, thFac, &act, &newSparsity, &newTh));
        H->sparsity = newSparsity;
        if (!act) break;
        recsLeft--; thFac = newTh;
    }
    if (nOut) *nOut = n;
    if (passesOut) *passesOut = passes;
    if (flagsOut) *flagsOut = flags;
    return LDSO_OK;
}

// the raster scan of `map` (wl x hl bytes) into the records of level l; *nOut = numPoints[l]
static int make_records(ldso_initializer *H, int l, const unsigned char *map, int wl, int hl, int typeFromMap, int *nOut) {
    hipStream_t st = H->stream;
    const int x0 = 3, x1 = wl - 4, y0 = 3, y1 = hl - 4;          // patternPadding + 1 <= x < wl - patternPadding - 2 (patternPadding = 2, Settings.h:164)
    CHK(hipMemsetAsync(H->d_fctl, 0, 4 * sizeof(int), st));
    hipLaunchKernelGGL(k_ini_rows, dim3((hl + 3) / 4), dim3(256), 0, st, map, wl, hl, x0, x1, y0, y1, H->d_rowCount);
    hipLaunchKernelGGL(k_ini_rowscan, dim3(1), dim3(256), 0, st, H->d_rowCount, H->d_rowStart, hl, H->d_fctl);
    CHK(hipGetLastError());
    int ctl[4] = {0, 0, 0, 0};
    CHK(hipMemcpyAsync(ctl, H->d_fctl, sizeof(ctl), hipMemcpyDeviceToHost, st));
    CHK(hipStreamSynchronize(st));
    const int n = ctl[FC_TOTAL];
    *nOut = n;
    if (n > INI_MAX_POINTS || n == 0) return LDSO_OK;                  // the caller refuses both
    RUN(first_reserve(H, l, n));
    hipLaunchKernelGGL(k_ini_records, dim3((hl + 3) / 4), dim3(256), 0, st, map, wl, x0, x1, y0, y1, H->d_rowStart, typeFromMap, H->d_rec[l], H->d_uv[l], H->recCap[l]);
    CHK(hipGetLastError());
    return LDSO_OK;
}

// One tree per level from the positions on the host, uploaded; then one search launch per level.  Everything that can refuse does so before the first launch.
struct NnLevels {
    ldso_nn_tree_t *tree[INI_MAXL] = {nullptr};
    std::vector<void *> dev;
    ~NnLevels() { for (auto *t : tree) ldso_init_nn_free(t); for (void *p : dev) (void) hipFree(p); }
};

static int nn_run(ldso_initializer *H, int levels, const std::vector<float> *uvHost, float *const *d_uv, const int *n, ldso_init_point_t *const *rec,
                  int32_t *const *d_nbIdx, float *const *d_nbDist, int32_t *const *d_parIdx, float *const *d_parDist, float *usBuild) {
    hipStream_t st = H->stream;
    NnLevels N;
    NnTreeDev T[INI_MAXL];
    int depth = 1;
    const auto t0 = std::chrono::steady_clock::now();
    for (int l = 0; l < levels; l++) {
        RUN(ldso_init_nn_build(n[l], uvHost[l].data(), &N.tree[l]));
        int nn = 0, d = 0;
        RUN(ldso_init_nn_info(N.tree[l], nullptr, &nn, &d, T[l].root));
        depth = std::max(depth, d);
        if (d > NN_MAX_DEPTH) { ldso_set_error("makeNN: the k-d tree is deeper than the 64 stack entries a lane has"); return LDSO_E_UNSUPPORTED; }
    }
    if (usBuild) *usBuild = std::chrono::duration<float, std::micro>(std::chrono::steady_clock::now() - t0).count();
    for (int l = 0; l < levels; l++) {
        int nn = 0;
        RUN(ldso_init_nn_info(N.tree[l], nullptr, &nn, nullptr, nullptr));
        std::vector<ldso_nn_node_t> nodes(nn);
        std::vector<int32_t> vind(n[l]);
        RUN(ldso_init_nn_get(N.tree[l], nodes.data(), vind.data()));
        ldso_nn_node_t *dn = nullptr; int *dv = nullptr;
        CHK(hipMalloc(&dn, nodes.size() * sizeof(ldso_nn_node_t))); N.dev.push_back(dn);
        CHK(hipMalloc(&dv, vind.size() * sizeof(int))); N.dev.push_back(dv);
        CHK(hipMemcpyAsync(dn, nodes.data(), nodes.size() * sizeof(ldso_nn_node_t), hipMemcpyHostToDevice, st));
        CHK(hipMemcpyAsync(dv, vind.data(), vind.size() * sizeof(int), hipMemcpyHostToDevice, st));
        CHK(hipStreamSynchronize(st));                                 // the host vectors go out of scope
        T[l].nodes = dn; T[l].vind = dv; T[l].uv = d_uv[l];
    }
    const size_t lds = (size_t) depth * 64 * sizeof(NnEntry);
    for (int l = 0; l < levels; l++) {
        const int up = l + 1 < levels;
        CHK(launch_lds(k_ini_nn, dim3((n[l] + 63) / 64), dim3(64), lds, st, T[l], T[up ? l + 1 : l], up, n[l], rec ? rec[l] : nullptr, d_nbIdx ? d_nbIdx[l] : nullptr,
                       d_nbDist ? d_nbDist[l] : nullptr, d_parIdx ? d_parIdx[l] : nullptr, d_parDist ? d_parDist[l] : nullptr));
    }
    CHK(hipStreamSynchronize(st));                                     // the trees' device copies are freed on return
    return LDSO_OK;
}

extern "C" {

int ldso_init_set_sparsity(ldso_initializer_t *H, int sparsity) {
    REQ(H && sparsity >= 1 && sparsity < (1 << 20), "ldso_init_set_sparsity: bad argument (sparsity >= 1)");
    H->sparsity = sparsity;
    return LDSO_OK;
}

int ldso_init_get_sparsity(ldso_initializer_t *H, int *sparsity) {
    REQ(H && sparsity, "ldso_init_get_sparsity: null argument");
    *sparsity = H->sparsity;
    return LDSO_OK;
}

int ldso_init_pixel_status(ldso_initializer_t *H, ldso_pyramid_t *pyr, int lvl, float desired_density, int recs_left, float th_fac, int *n_out, int *passes_out) {
    REQ(H && pyr, "ldso_init_pixel_status: null argument");
    REQ(lvl >= 1 && lvl < pyr->levels && (H->w >> lvl) >= 3 && (H->h >> lvl) >= 3, "ldso_init_pixel_status: level out of range (1 .. the pyramid's last)");
    REQ(desired_density > 0 && std::isfinite(desired_density) && std::isfinite(th_fac) && recs_left >= 0, "ldso_init_pixel_status: bad arguments (density > 0, recs_left >= 0)");
    RUN(pyramid_wait(pyr, H->device, H->w, H->h, lvl + 1, H->stream, "ldso_init_pixel_status", "the initialiser (device, size, levels)"));
    RUN(first_buffers(H));
    int flags = 0;
    H->statusLvl = lvl;
    RUN(pixel_status(H, pyr->lv[lvl], H->w >> lvl, H->h >> lvl, desired_density, recs_left, th_fac, n_out, passes_out, &flags));
    if (flags & 1) { ldso_set_error("ldso_init_pixel_status: non-finite gradient"); return LDSO_E_NONFINITE; }
    return LDSO_OK;
}

int ldso_init_get_status_map(ldso_initializer_t *H, unsigned char *map_out, int *lvl_out) {
    REQ(H && map_out && H->d_status && H->statusLvl >= 1, "ldso_init_get_status_map: no pixel-status pass has run");
    CHK(hipSetDevice(H->device));
    CHK(hipMemcpyAsync(map_out, H->d_status, (size_t) (H->w >> H->statusLvl) * (H->h >> H->statusLvl), hipMemcpyDeviceToHost, H->stream));
    CHK(hipStreamSynchronize(H->stream));
    if (lvl_out) *lvl_out = H->statusLvl;
    return LDSO_OK;
}

int ldso_init_make_nn(ldso_initializer_t *H, int n_levels, const float *const *uv, const int *n, int32_t *const *nb_idx_out, float *const *nb_dist_out,
                      int32_t *const *parent_idx_out, float *const *parent_dist_out) {
    REQ(H && uv && n && n_levels >= 1 && n_levels <= INI_MAXL, "ldso_init_make_nn: bad arguments (1 .. 5 levels)");
    for (int l = 0; l < n_levels; l++) {
        REQ(uv[l] && n[l] <= (1 << 24), "ldso_init_make_nn: null or oversized level");
        if (n[l] < NN_K) { ldso_set_error("ldso_init_make_nn: a level with fewer than 10 points"); return LDSO_E_UNSUPPORTED; }
    }
    CHK(hipSetDevice(H->device));
    hipStream_t st = H->stream;
    std::vector<float> uvHost[INI_MAXL];
    std::vector<void *> tmp;
    struct Free { std::vector<void *> &v; ~Free() { for (void *p : v) (void) hipFree(p); } } guard{tmp};
    float *d_uv[INI_MAXL]; int32_t *d_ni[INI_MAXL], *d_pi[INI_MAXL]; float *d_nd[INI_MAXL], *d_pd[INI_MAXL];
    for (int l = 0; l < n_levels; l++) {
        uvHost[l].assign(uv[l], uv[l] + (size_t) n[l] * 2);
        CHK(hipMalloc(&d_uv[l], (size_t) n[l] * 8)); tmp.push_back(d_uv[l]);
        CHK(hipMalloc(&d_ni[l], (size_t) n[l] * NN_K * 4)); tmp.push_back(d_ni[l]);
        CHK(hipMalloc(&d_nd[l], (size_t) n[l] * NN_K * 4)); tmp.push_back(d_nd[l]);
        CHK(hipMalloc(&d_pi[l], (size_t) n[l] * 4)); tmp.push_back(d_pi[l]);
        CHK(hipMalloc(&d_pd[l], (size_t) n[l] * 4)); tmp.push_back(d_pd[l]);
        CHK(hipMemcpyAsync(d_uv[l], uvHost[l].data(), (size_t) n[l] * 8, hipMemcpyHostToDevice, st));
    }
    RUN(nn_run(H, n_levels, uvHost, d_uv, n, nullptr, d_ni, d_nd, d_pi, d_pd, nullptr));
    for (int l = 0; l < n_levels; l++) {
        if (nb_idx_out && nb_idx_out[l]) CHK(hipMemcpyAsync(nb_idx_out[l], d_ni[l], (size_t) n[l] * NN_K * 4, hipMemcpyDeviceToHost, st));
        if (nb_dist_out && nb_dist_out[l]) CHK(hipMemcpyAsync(nb_dist_out[l], d_nd[l], (size_t) n[l] * NN_K * 4, hipMemcpyDeviceToHost, st));
        if (parent_idx_out && parent_idx_out[l]) CHK(hipMemcpyAsync(parent_idx_out[l], d_pi[l], (size_t) n[l] * 4, hipMemcpyDeviceToHost, st));
        if (parent_dist_out && parent_dist_out[l]) CHK(hipMemcpyAsync(parent_dist_out[l], d_pd[l], (size_t) n[l] * 4, hipMemcpyDeviceToHost, st));
    }
    CHK(hipStreamSynchronize(st));
    return LDSO_OK;
}

int ldso_init_first_profile(ldso_initializer_t *H, int enable, float us_out[6]) {
    REQ(H, "ldso_init_first_profile: null handle");
    H->profileFirst = enable != 0;
    if (us_out) for (int i = 0; i < 6; i++) us_out[i] = H->usFirst[i];
    return LDSO_OK;
}

int ldso_init_set_first_frame(ldso_initializer_t *H, const float calib[4], ldso_pyramid_t *pyr, float ab_exposure, ldso_pixsel_t *pixsel, float huberTH, int fixAffine,
                              int n_points_out[]) {
    REQ(H && calib && pyr && pixsel, "ldso_init_set_first_frame: null argument");
    if (H->levels > 5) { ldso_set_error("ldso_init_set_first_frame: more than 5 levels (the reference's densities[] has five entries)"); return LDSO_E_UNSUPPORTED; }
    hipStream_t st = H->stream;
    int pw = 0, ph = 0, pdev = 0;
    const unsigned char *map0 = pix_map_device(pixsel, &pw, &ph, &pdev);
    REQ(pw == H->w && ph == H->h && pdev == H->device, "ldso_init_set_first_frame: the selector does not match the initialiser (device, size)");
    RUN(pyramid_wait(pyr, H->device, H->w, H->h, std::max(H->levels, 3), st, "ldso_init_set_first_frame", "the initialiser (device, size, levels)"));
    RUN(first_buffers(H));
    H->haveFirst = false; H->haveNew = false;
    typedef std::chrono::steady_clock clk;
    auto us = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<float, std::micro>(b - a).count(); };
    const auto tStart = clk::now();
    // level 0 (:559-562): sel.currentPotential = 3; makeMaps(firstFrame, statusMap, densities[0] * w[0] * h[0], 1, false, 2)
    const float densities[] = {0.03, 0.05, 0.15, 0.5, 1};
    RUN(ldso_pixsel_set_potential(pixsel, 3));
    RUN(ldso_pixsel_make_maps(pixsel, pyr, densities[0] * H->w * H->h, 1, 2.0f, nullptr, nullptr, nullptr));          // waits for its stream: the map is complete
    const auto tMaps0 = clk::now();
    float usMaps = 0, usRec = 0;
    int n[INI_MAXL] = {0};
    bool nonfinite = false;
    for (int l = 0; l < H->levels; l++) {
        const int wl = H->w >> l, hl = H->h >> l;
        const auto a = clk::now();
        if (l > 0) {
            int flags = 0;
            H->statusLvl = l;
            RUN(pixel_status(H, pyr->lv[l], wl, hl, densities[l] * H->w * H->h, 5, 1.0f, nullptr, nullptr, &flags));
            nonfinite = nonfinite || (flags & 1);
        }
        const auto b = clk::now();
        RUN(make_records(H, l, l ? H->d_status : map0, wl, hl, l == 0, &n[l]));
        CHK(hipStreamSynchronize(st));
        usMaps += us(a, b); usRec += us(b, clk::now());
    }
    if (nonfinite) { ldso_set_error("ldso_init_set_first_frame: non-finite gradient"); return LDSO_E_NONFINITE; }
    for (int l = 0; l < H->levels; l++) {
        REQ(n[l] <= INI_MAX_POINTS, "ldso_init_set_first_frame: more than 36000 points on one level (LDS working set of the sweeps)");
        if (n[l] < NN_K) { ldso_set_error("ldso_init_set_first_frame: a level with fewer than 10 records (makeNN needs 10 neighbours)"); return LDSO_E_UNSUPPORTED; }
    }
    // makeNN: positions down, trees up, one search launch per level
    std::vector<float> uvHost[INI_MAXL];
    for (int l = 0; l < H->levels; l++) {
        uvHost[l].resize((size_t) n[l] * 2);
        CHK(hipMemcpyAsync(uvHost[l].data(), H->d_uv[l], (size_t) n[l] * 8, hipMemcpyDeviceToHost, st));
    }
    CHK(hipStreamSynchronize(st));
    const auto tNn = clk::now();
    float usBuild = 0;
    RUN(nn_run(H, H->levels, uvHost, H->d_uv, n, H->d_rec, nullptr, nullptr, nullptr, nullptr, &usBuild));
    const auto tSearch = clk::now();
    // what ldso_init_set_first does with finished records; its schedules are host work on the neighbour lists
    std::vector<ldso_init_point_t> rec[INI_MAXL];
    const ldso_init_point_t *ptr[INI_MAXL] = {nullptr};
    for (int l = 0; l < H->levels; l++) {
        rec[l].resize(n[l]);
        CHK(hipMemcpyAsync(rec[l].data(), H->d_rec[l], (size_t) n[l] * sizeof(ldso_init_point_t), hipMemcpyDeviceToHost, st));
        ptr[l] = rec[l].data();
    }
    CHK(hipStreamSynchronize(st));
    RUN(ini_set_first_records(H, calib, ab_exposure, ptr, n, huberTH, fixAffine));
    for (int l = 0; l < H->levels; l++) {
        CHK(hipMemcpyAsync(H->d_first[l], pyr->lv[l], (size_t) (H->w >> l) * (H->h >> l) * 3 * sizeof(float), hipMemcpyDeviceToDevice, st));
        H->firstRec[l].swap(rec[l]);
    }
    CHK(hipStreamSynchronize(st));
    H->haveFirst = true;
    if (H->profileFirst) {
        H->usFirst[0] = us(tStart, tMaps0); H->usFirst[1] = usMaps; H->usFirst[2] = usRec; H->usFirst[3] = usBuild;
        H->usFirst[4] = us(tNn, tSearch) - usBuild; H->usFirst[5] = us(tSearch, clk::now());
    }
    if (n_points_out) for (int l = 0; l < H->levels; l++) n_points_out[l] = n[l];
    return LDSO_OK;
}

}  // extern "C"
