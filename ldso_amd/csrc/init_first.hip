// init_first.hip — CoarseInitializer::setFirst from a resident pyramid (include/ldso_hip.h, "setFirst from a resident pyramid"): makePixelStatus for the
// levels >= 1 (k_ini_gridmax + the host recursion), the Pnt records of every level (the raster scan of raster_scan.h + k_ini_records), the searches of makeNN over
// the host-built k-d trees (k_ini_nn; the search itself is nn_search.h, the build init_nn_tree.cpp), and ldso_init_set_first_frame, which strings them together
// and hands the finished records to the code behind ldso_init_set_first (initializer_api.hip).
#include <chrono>
#include "initializer.h"
#include "pyramid.h"
#include "nn_search.h"
#include "raster_scan.h"

#define FC_COUNT 0            // d_fctl: pixels set by the gridMaxSelection pass
#define FC_FLAGS 1            // SEL_FLAG_NONFINITE: a non-finite gradient was read
#define FC_TOTAL 2            // records of the scanned rectangle
#define NN_MAX_DEPTH 64       // 64 lanes x 64 entries x 16 bytes = 64 KB of LDS
#define INI_MAX_POINTS 36000  // ldso_init_set_first's limit per level

// ---------------------------------------------------------------------------------------------------------
// gridMaxSelection (PixelSelector2.h:63-225; the templated variants and the generic one are the same arithmetic): G = lanes_per_block(pot) lanes per pot x pot block.
// The reference scans a block with dx in the outer loop and dy in the inner one and keeps the FIRST strict maximum, so among equal values the smallest
// c = dx * pot + dy wins.  A lane walks its cells in ascending c (first strict maximum again); across the lanes the maximum of argmax_key(value, c) picks the
// largest value and, among equals, the smallest c.  A value has to exceed the initial best of 0, and a NaN never does.
// ---------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_ini_gridmax(const float *__restrict__ img, unsigned char *__restrict__ map, int w, int h, int pot, int nbx, int nby, int G, float THFac,
                                                     int *__restrict__ ctl) {
    const long long gid = (long long) blockIdx.x * 256 + threadIdx.x;
    const int sub = (int) (gid % G);
    const long long blk = gid / G;
    const bool live = blk < (long long) nbx * nby;
    const float TH = THFac * 10.0f * 0.75f, TH2 = TH * TH;
    unsigned long long k[4] = {0, 0, 0, 0};          // the best of |gx|, |gy|, |gx - gy|, |gx + gy|
    bool bad = false;
    int x0 = 0, y0 = 0;
    if (live) {
        x0 = 1 + (int) (blk % nbx) * pot; y0 = 1 + (int) (blk / nbx) * pot;          // x0 + pot - 1 <= w - 2, y0 + pot - 1 <= h - 2: nbx = (w - 2) / pot
        float best[4] = {0, 0, 0, 0};
        for (int c = sub; c < pot * pot; c += G) {
            const int dx = c / pot, dy = c - dx * pot;
            const size_t i = ((size_t) (y0 + dy) * w + (x0 + dx)) * 3;
            const float gx = img[i + 1], gy = img[i + 2];
            bad = bad || !isfinite(gx) || !isfinite(gy);
            const float sqgd = gx * gx + gy * gy;
            if (sqgd > TH2) {
                const float a[4] = {fabsf(gx), fabsf(gy), fabsf(gx - gy), fabsf(gx + gy)};
#pragma unroll
                for (int q = 0; q < 4; q++) if (a[q] > best[q]) { best[q] = a[q]; k[q] = argmax_key(a[q], c); }
            }
        }
    }
    for (int o = G >> 1; o > 0; o >>= 1) {          // G divides 64: the butterfly stays inside the block's lanes
#pragma unroll
        for (int q = 0; q < 4; q++) k[q] = max(k[q], (unsigned long long) __shfl_xor((long long) k[q], o, 64));
    }
    int set = 0;
    if (live && sub == 0) {
        int cs[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int c = cs[q] = k[q] ? argmax_index(k[q]) : -1;
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
    set = wave_sum(set);
    if ((threadIdx.x & 63) == 0 && set) atomicAdd(&ctl[FC_COUNT], set);
    report_nonfinite(bad, &ctl[FC_FLAGS]);
}

// ---------------------------------------------------------------------------------------------------------
// the records (:567-603): one record per set pixel of the scanned rectangle in raster order
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ini_records(const unsigned char *__restrict__ map, int w, ScanRect r, const int *__restrict__ rowStart, int typeFromMap,
                                                     ldso_init_point_t *__restrict__ rec, float *__restrict__ uv, int cap) {
    const int y = raster_row();
    if (y < r.y0 || y >= r.y1) return;
    raster_walk(map, w, r.x0, r.x1, y, rowStart, [&](int x, int v, int rank) {
        if (rank >= cap) return;
        ldso_init_point_t p;
        p.u = (float) (x + 0.1); p.v = (float) (y + 0.1);              // int + double, then rounded to float (:578-579)
        p.idepth = 1.0f; p.iR = 1.0f; p.isGood = 1;
        p.energy[0] = p.energy[1] = 0.0f; p.lastHessian = 0.0f; p.lastHessian_new = 0.0f;
        p.my_type = typeFromMap ? (float) v : 1.0f;
        p.outlierTH = 8 * (12.0f * 12.0f);                             // patternNum * setting_outlierTH (Settings.h: 8; Setting.cc: 12 * 12)
        p.parent = -1; p.parentDist = -1.0f;
#pragma unroll
        for (int q = 0; q < 10; q++) { p.neighbours[q] = -1; p.neighboursDist[q] = 0.0f; }
        LDSO_INIT_POINT_FILL_UNSET(p);
        rec[rank] = p;
        uv[2 * rank] = p.u; uv[2 * rank + 1] = p.v;
    });
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
        const int G = lanes_per_block(pot);
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
    const ScanRect r = scan_rect(wl, hl);
    int n = 0;
    CHK(hipMemsetAsync(H->d_fctl, 0, 4 * sizeof(int), st));
    RUN(raster_count(map, wl, hl, r, H->d_rowCount, H->d_rowStart, H->d_fctl + FC_TOTAL, st, &n));
    *nOut = n;
    if (n > INI_MAX_POINTS || n == 0) return LDSO_OK;                  // the caller refuses both
    RUN(first_reserve(H, l, n));
    hipLaunchKernelGGL(k_ini_records, raster_grid(hl), dim3(256), 0, st, map, wl, r, H->d_rowStart, typeFromMap, H->d_rec[l], H->d_uv[l], H->recCap[l]);
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
    if (flags & SEL_FLAG_NONFINITE) { ldso_set_error("ldso_init_pixel_status: non-finite gradient"); return LDSO_E_NONFINITE; }
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
            nonfinite = nonfinite || (flags & SEL_FLAG_NONFINITE);
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
