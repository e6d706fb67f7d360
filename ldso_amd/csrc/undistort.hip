// undistort.hip — Undistort::undistort<T> on the device (gfx950; reference src/frontend/Undistort.cc:357-457): the raw 8- or 16-bit camera frame goes up
// (1 or 2 bytes per pixel instead of the 4 of the float irradiance), PhotometricUndistorter::processFrame (:189-227) and the bilinear remap (:390-443) run as
// ONE kernel that writes the irradiance straight into a frame's pyramid staging (ldso_pyramid_t::d_color), and FrameHessian::makeImages (images.hip) follows
// on the same stream.  The irradiance never exists on the host as floats unless the caller asks for it (ldso_undist_get).
//
//   k_undist_frame   one lane per output pixel: its remap entry, four taps of the raw frame (a gather: about 32 bytes per pixel from tables that are L2
//                    resident), the pixel rule of undistort_px.h.  The 256-entry response G is staged in LDS for 8-bit frames; the 65536-entry one of
//                    16-bit frames is read from global memory.  Passthrough (rectification "none", :450-452): the photometric output of pixel idx.
//   k_undist_group   the same per-pixel work (undist_workgroup, defined once) for the frames of a group of undistorters: a job table, one launch
//                    (ldso_undist_group_*: the raw frames of many sequences in one copy).
//
// The result is bit for bit what the reference returns (float arithmetic in its operand order, -ffp-contract=off), with the one deliberate difference that
// undistort_px.h states: a pixel whose four taps are not all inside the source image is 0 and nothing outside the raw buffer is read, where the reference
// over-reads one row for the table entry xxi == 0 && yyi == hOrg - 1.  benchmark_varNoise / benchmark_varBlurNoise (:376-413, :468-555) are out of scope.
#include "hip_host.h"
#include "group_member.h"
#include "undistort_px.h"

struct UndistArgs {
    const void *raw;                    // wOrg * hOrg pixels of BPP bytes
    const float *G, *vig;               // response (256 / 65536 entries), vignetteMapInv (wOrg * hOrg); read on the calibrated paths only
    const float *remapX, *remapY;       // w * h each, or both null: passthrough
    float *out;                         // w * h
    int w, h, wOrg, hOrg, mode;
    float factor;
};

// Workgroup `wg` (256 lanes) of one frame: the stage of the response, the bounds test, the pixel rule.  Gs: 256 floats of LDS (BPP 1; unused for BPP 2).
// The one definition of the per-pixel work: k_undist_frame and k_undist_group both call it.
template <int BPP>
__device__ __forceinline__ void undist_workgroup(const UndistArgs &A, int wg, float *Gs) {
    const float *G = A.G;
    if (BPP == 1 && A.mode != UNDIST_PLAIN) {          // block-uniform
        Gs[threadIdx.x] = A.G[threadIdx.x];
        __syncthreads();
        G = Gs;
    }
    const int idx = wg * 256 + threadIdx.x;
    if (idx >= A.w * A.h) return;
    float v;
    if (A.remapX == nullptr) v = undist_photo(A.raw, BPP, idx, G, A.vig, A.mode, A.factor);
    else v = undist_px(A.raw, BPP, G, A.vig, A.mode, A.factor, A.remapX[idx], A.remapY[idx], A.wOrg, A.hOrg);
    A.out[idx] = v;
}

template <int BPP>
__global__ __launch_bounds__(256) void k_undist_frame(UndistArgs A) {
    __shared__ float Gs[BPP == 1 ? 256 : 1];
    undist_workgroup<BPP>(A, (int) blockIdx.x, Gs);
}

// The frames of a group of undistorters in one launch (ldso_undist_group_*): job j is one active member's frame, a workgroup belongs to one job - wgFirst[j]
// workgroups lie in front of job j, wgFirst[nJobs] is the grid (group_member_of).  bpp and mode are the job's, hence uniform per workgroup: an 8-bit job on a
// calibrated path stages its response in LDS, a 16-bit one reads it from global memory, exactly as k_undist_frame<1> / <2> do.
struct UndistJob {          // one row of the job table: UndistArgs and the pixel width; every pointer a device pointer, `raw` inside the group's device arena
    const void *raw;
    const float *G, *vig, *remapX, *remapY;
    float *out;
    int w, h, wOrg, hOrg, mode, bpp;
    float factor;
    int pad_;
};
// a row as the kernel reads it: UndistJob with its pointers typed as device memory (group_member.h: LD_GLOBAL)
struct UndistJobDev {
    LD_GLOBAL const void *raw;
    LD_GLOBAL const float *G, *vig, *remapX, *remapY;
    LD_GLOBAL float *out;
    int w, h, wOrg, hOrg, mode, bpp;
    float factor;
    int pad_;
};
static_assert(sizeof(UndistJobDev) == sizeof(UndistJob) && sizeof(UndistJob) % 16 == 0 && offsetof(UndistJobDev, out) == offsetof(UndistJob, out) &&
              offsetof(UndistJobDev, factor) == offsetof(UndistJob, factor), "UndistJobDev is UndistJob");

__global__ __launch_bounds__(256) void k_undist_group(const UndistJob *__restrict__ jobs, const int *__restrict__ wgFirst, int nJobs) {
    __shared__ float Gs[256];
    const int j = group_member_of(wgFirst, nJobs, (int) blockIdx.x);
    const UndistJobDev D = ((const UndistJobDev *) jobs)[j];
    UndistArgs A;
    A.raw = (const void *) D.raw; A.G = (const float *) D.G; A.vig = (const float *) D.vig; A.remapX = (const float *) D.remapX; A.remapY = (const float *) D.remapY;
    A.out = (float *) D.out; A.w = D.w; A.h = D.h; A.wOrg = D.wOrg; A.hOrg = D.hOrg; A.mode = D.mode; A.factor = D.factor;
    const int wg = (int) blockIdx.x - wgFirst[j];
    if (D.bpp == 1) undist_workgroup<1>(A, wg, Gs);
    else undist_workgroup<2>(A, wg, Gs);
}

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
struct ldso_undistorter {
    int device = 0, w = 0, h = 0, wOrg = 0, hOrg = 0;
    hipStream_t stream = nullptr;
    bool ownStream = false, hasRemap = false, remapSet = false, hasG = false, useExposure = true;
    int GDepth = 0, photometricCalibration = 2;
    float *d_remap = nullptr;           // remapX, then remapY
    float *d_G = nullptr, *d_vig = nullptr, *d_out = nullptr;
    void *d_raw = nullptr;
    void *h_raw[2] = {nullptr, nullptr};          // pinned staging of the raw frame, used alternately: a frame can be staged while the previous one's copy is in flight
    hipEvent_t copied[2] = {};                    // ... recorded behind the copy out of each
    int turn = 0;
    const float *last = nullptr;        // where the last frame's irradiance lies (a pyramid's d_color or d_out)
    hipEvent_t done = nullptr;          // recorded behind the last frame's kernel
    StageClock<3> clock;                // copy, undistortion kernel, pyramid build; a frame does not wait: ldso_undist_profile settles it
    const void *inGroup = nullptr;      // the ldso_undist_group this undistorter belongs to (at most one; ldso_undist_destroy refuses while set: the group dereferences its members)
};

// a group of undistorters whose frames share one copy and one launch
struct ldso_undist_group {
    std::vector<ldso_undistorter *> m;
    int device = 0;
    AsyncArena arena;                   // undist_group_layout
    StageClock<3> clock;                // the one copy, the undistortion kernel, the grouped pyramid build; settled by ldso_undist_group_profile
};

namespace {

// PhotometricUndistorter::processFrame for one frame of U: the path it takes (:197-198) and ImageAndExposure::exposure_time (:203, :220, :224-225)
struct FrameRule { int mode; float exposureOut; };
FrameRule frame_rule(const ldso_undistorter *U, float exposure) {
    int mode = UNDIST_PLAIN;
    if (U->hasG && exposure > 0 && U->photometricCalibration != 0) mode = U->photometricCalibration == 2 ? UNDIST_VIGNETTE : UNDIST_RESPONSE;
    return {mode, U->useExposure ? exposure : 1.0f};
}

// the kernel's view of one frame of U: `raw` in device memory, the irradiance into `out`
UndistArgs frame_args(const ldso_undistorter *U, const void *d_raw, float *out, int mode, float factor) {
    UndistArgs A;
    const size_t n = (size_t) U->w * U->h;
    A.raw = d_raw; A.G = U->d_G; A.vig = U->d_vig;
    A.remapX = U->hasRemap ? U->d_remap : nullptr; A.remapY = U->hasRemap ? U->d_remap + n : nullptr;
    A.out = out;
    A.w = U->w; A.h = U->h; A.wOrg = U->wOrg; A.hOrg = U->hOrg; A.mode = mode; A.factor = factor;
    return A;
}

constexpr GroupRule GROUP_RULE = {"an undistorter", "ldso_undist_set_stream", GROUP_MAX_MEMBERS};
static_assert(sizeof(UndistJob) == 80, "the row of undist_group_layout as tests/test_group_stage_cpu.py sizes it");

}  // namespace

extern "C" {

int ldso_undist_destroy(ldso_undistorter_t *U) {
    if (!U) return LDSO_OK;
    REQ(U->inGroup == nullptr, "ldso_undist_destroy: the undistorter is a member of a live group (ldso_undist_group_destroy first: the group dereferences its members)");
    hipSetDevice(U->device);
    hipDeviceSynchronize();
    hipFree(U->d_remap); hipFree(U->d_G); hipFree(U->d_vig); hipFree(U->d_out); hipFree(U->d_raw);
    for (void *p : U->h_raw) if (p) hipHostFree(p);
    for (hipEvent_t e : U->copied) if (e) hipEventDestroy(e);
    U->clock.destroy();
    if (U->done) hipEventDestroy(U->done);
    if (U->ownStream && U->stream) hipStreamDestroy(U->stream);
    delete U;
    return LDSO_OK;
}

int ldso_undist_create(int device, int wOrg, int hOrg, int w, int h, ldso_undistorter_t **out) {
    REQ(out && wOrg > 1 && hOrg > 1 && w > 0 && h > 0 && (long long) wOrg * hOrg < (1ll << 30) && (long long) w * h < (1ll << 30), "ldso_undist_create: bad arguments");
    RUN(open_device(device, "ldso_undist_create"));
    ldso_undistorter *U = new ldso_undistorter();
    U->device = device; U->w = w; U->h = h; U->wOrg = wOrg; U->hOrg = hOrg;
    const size_t n = (size_t) w * h, nOrg = (size_t) wOrg * hOrg;
    bool ok = hipStreamCreateWithFlags(&U->stream, hipStreamNonBlocking) == hipSuccess;
    U->ownStream = ok;
    ok = ok && hipMalloc(&U->d_remap, 2 * n * 4) == hipSuccess && hipMalloc(&U->d_G, 65536 * 4) == hipSuccess && hipMalloc(&U->d_vig, nOrg * 4) == hipSuccess
         && hipMalloc(&U->d_out, n * 4) == hipSuccess && hipMalloc(&U->d_raw, nOrg * 2) == hipSuccess;
    for (void *&p : U->h_raw) ok = ok && hipHostMalloc(&p, nOrg * 2, hipHostMallocDefault) == hipSuccess;
    for (hipEvent_t &e : U->copied) ok = ok && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
    ok = ok && U->clock.create() == LDSO_OK;
    ok = ok && hipEventCreateWithFlags(&U->done, hipEventDisableTiming) == hipSuccess;
    if (!ok) { ldso_undist_destroy(U); ldso_set_error("ldso_undist_create: out of device or pinned memory"); return LDSO_E_HIP; }
    *out = U;
    return LDSO_OK;
}

int ldso_undist_set_stream(ldso_undistorter_t *U, void *s) {
    REQ(U, "ldso_undist_set_stream: null handle");
    return swap_stream(U->stream, U->ownStream, s);
}

int ldso_undist_set_remap(ldso_undistorter_t *U, const float *remapX, const float *remapY) {
    REQ(U && (remapX == nullptr) == (remapY == nullptr), "ldso_undist_set_remap: null handle, or only one of the two tables");
    if (!remapX) {
        REQ(U->w == U->wOrg && U->h == U->hOrg, "ldso_undist_set_remap: passthrough needs w == wOrg && h == hOrg");
        U->hasRemap = false; U->remapSet = true;
        return LDSO_OK;
    }
    const size_t n = (size_t) U->w * U->h;
    for (size_t i = 0; i < n; i++) REQ(std::isfinite(remapX[i]) && std::isfinite(remapY[i]), "ldso_undist_set_remap: non-finite table entry");
    CHK(hipSetDevice(U->device));
    CHK(hipMemcpyAsync(U->d_remap, remapX, n * 4, hipMemcpyHostToDevice, U->stream));
    CHK(hipMemcpyAsync(U->d_remap + n, remapY, n * 4, hipMemcpyHostToDevice, U->stream));
    CHK(hipStreamSynchronize(U->stream));
    U->hasRemap = true; U->remapSet = true;
    return LDSO_OK;
}

int ldso_undist_set_photometric(ldso_undistorter_t *U, const float *G, int GDepth, const float *vignetteMapInv, int photometricCalibration, int useExposure) {
    REQ(U && photometricCalibration >= 0 && photometricCalibration <= 2, "ldso_undist_set_photometric: null handle or setting_photometricCalibration outside 0..2");
    REQ(!G || (GDepth >= 256 && GDepth <= 65536), "ldso_undist_set_photometric: GDepth outside 256..65536");
    REQ(!G || photometricCalibration != 2 || vignetteMapInv, "ldso_undist_set_photometric: mode 2 needs vignetteMapInv");
    CHK(hipSetDevice(U->device));
    if (G) CHK(hipMemcpyAsync(U->d_G, G, (size_t) GDepth * 4, hipMemcpyHostToDevice, U->stream));
    if (G && vignetteMapInv) CHK(hipMemcpyAsync(U->d_vig, vignetteMapInv, (size_t) U->wOrg * U->hOrg * 4, hipMemcpyHostToDevice, U->stream));
    CHK(hipStreamSynchronize(U->stream));
    U->hasG = G != nullptr; U->GDepth = G ? GDepth : 0;
    U->photometricCalibration = photometricCalibration; U->useExposure = useExposure != 0;
    return LDSO_OK;
}

int ldso_undist_profile(ldso_undistorter_t *U, int enable, float us_out[3]) {
    REQ(U, "ldso_undist_profile: null handle");
    return U->clock.report(U->device, enable, us_out);
}

int ldso_undist_frame(ldso_undistorter_t *U, const void *raw, int bytes_per_pixel, float exposure, float factor, ldso_pyramid_t *pyr, float *exposure_out) {
    REQ(U && raw && (bytes_per_pixel == 1 || bytes_per_pixel == 2), "ldso_undist_frame: bad arguments (bytes_per_pixel is 1 or 2)");
    REQ(U->remapSet, "ldso_undist_frame: ldso_undist_set_remap has not been called");
    REQ(!pyr || (pyr->device == U->device && pyr->w == U->w && pyr->h == U->h), "ldso_undist_frame: pyramid does not match the undistorter (device, size)");
    const FrameRule rule = frame_rule(U, exposure);
    const int mode = rule.mode;
    REQ(mode == UNDIST_PLAIN || bytes_per_pixel == 1 || U->GDepth >= 65536, "ldso_undist_frame: a 16-bit frame needs a response of 65536 entries");
    CHK(hipSetDevice(U->device));
    hipStream_t st = U->stream;
    const size_t bytes = (size_t) U->wOrg * U->hOrg * bytes_per_pixel;
    const int t = U->turn;
    U->turn ^= 1;
    CHK(hipEventSynchronize(U->copied[t]));          // the copy of the frame before last out of this staging buffer: long done
    memcpy(U->h_raw[t], raw, bytes);
    StageClock<3> &clk = U->clock.begin();
    RUN(clk.mark(0, st));
    CHK(hipMemcpyAsync(U->d_raw, U->h_raw[t], bytes, hipMemcpyHostToDevice, st));
    CHK(hipEventRecord(U->copied[t], st));
    RUN(clk.mark(1, st));
    const UndistArgs A = frame_args(U, U->d_raw, pyr ? pyr->d_color : U->d_out, mode, factor);
    const size_t n = (size_t) U->w * U->h;
    const dim3 grid((unsigned) ((n + 255) / 256));
    if (bytes_per_pixel == 1) hipLaunchKernelGGL(k_undist_frame<1>, grid, dim3(256), 0, st, A);
    else hipLaunchKernelGGL(k_undist_frame<2>, grid, dim3(256), 0, st, A);
    CHK(hipGetLastError());
    CHK(hipEventRecord(U->done, st));
    RUN(clk.mark(2, st));
    U->last = A.out;
    if (pyr) {
        CHK(img_launch_make_images(pyr->d_color, pyr->w, pyr->h, pyr->levels, pyr->lv, st));
        CHK(hipEventRecord(pyr->ready, st));
        pyr->built = true;
    }
    RUN(clk.mark(3, st)); clk.defer();
    if (exposure_out) *exposure_out = rule.exposureOut;
    return LDSO_OK;
}

int ldso_undist_get(ldso_undistorter_t *U, float *irradiance_out) {
    REQ(U && irradiance_out && U->last, "ldso_undist_get: bad arguments (or no frame yet)");
    CHK(hipSetDevice(U->device));
    CHK(hipEventSynchronize(U->done));
    CHK(hipMemcpy(irradiance_out, U->last, (size_t) U->w * U->h * 4, hipMemcpyDeviceToHost));
    return LDSO_OK;
}

int ldso_undist_device(ldso_undistorter_t *U, const void **dev_ptr) {
    REQ(U && dev_ptr, "ldso_undist_device: bad arguments");
    *dev_ptr = U->last;
    return LDSO_OK;
}

// ---------------------------------------------------------------------------------------------------------
// ldso_undist_group_*: Undistort::undistort<T> (Undistort.cc:357-457) of the raw frames of several sequences.  One ldso_undist_frame is a copy, a launch and - into
// a pyramid - 2 x levels more; the group stages every active member's raw frame and the job table into one pinned arena, moves it in one copy, undistorts in one
// launch (k_undist_group) and hands the members' pyramids to the grouped build (pyr_group_build, images.hip): 1 + 2 x Lmax launches and one copy whatever n.
// ---------------------------------------------------------------------------------------------------------

int ldso_undist_group_destroy(ldso_undist_group_t *g) {
    if (!g) return LDSO_OK;
    hipSetDevice(g->device);
    group_leave(g);
    async_arena_release(g->arena);          // waits for the last call's kernel
    g->clock.destroy();
    delete g;
    return LDSO_OK;
}

int ldso_undist_group_create(ldso_undistorter_t *const *u, int n, ldso_undist_group_t **out) {
    RUN(group_admit(u, n, out, "ldso_undist_group_create", GROUP_RULE));
    CHK(hipSetDevice(u[0]->device));
    ldso_undist_group *g = new ldso_undist_group();
    g->device = u[0]->device;
    auto body = [&]() -> int {
        RUN(async_arena_create(g->arena));
        return g->clock.create();
    };
    RUN(finish_create(body(), g, out, ldso_undist_group_destroy));
    g->m.assign(u, u + n);
    group_join(g);
    return LDSO_OK;
}

int ldso_undist_group_profile(ldso_undist_group_t *g, int enable, float us_out[3]) {
    REQ(g, "ldso_undist_group_profile: null group");
    return g->clock.report(g->device, enable, us_out);
}

int ldso_undist_group_frames(ldso_undist_group_t *g, const uint8_t *active, const void *const *raw, const int *bytes_per_pixel, const float *exposure, const float *factor,
                             ldso_pyr_group_t *pg, float *exposure_out) {
    static const char who[] = "ldso_undist_group_frames";
    REQ(g && raw && bytes_per_pixel && exposure && factor, std::string(who) + ": null argument");
    RUN(group_check(g->m.data(), g->m.size(), who, GROUP_RULE));
    const int n = (int) g->m.size();
    REQ(!pg || ((int) pg->m.size() == n && pg->device == g->device), std::string(who) + ": the pyramid group does not match the undistorter group (device, number of members)");
    // every refusal comes before anything is staged or enqueued
    std::vector<int> members;
    RUN(group_active(n, active, who, members, [&](int i) -> const char * {
        const ldso_undistorter *U = g->m[(size_t) i];
        if (!raw[i]) return "null raw frame";
        if (bytes_per_pixel[i] != 1 && bytes_per_pixel[i] != 2) return "bytes_per_pixel is 1 or 2";
        if (!U->remapSet) return "ldso_undist_set_remap has not been called";
        const FrameRule rule = frame_rule(U, exposure[i]);
        if (!(rule.mode == UNDIST_PLAIN || bytes_per_pixel[i] == 1 || U->GDepth >= 65536)) return "a 16-bit frame needs a response of 65536 entries";
        if (pg && !(pg->m[(size_t) i]->w == U->w && pg->m[(size_t) i]->h == U->h)) return "pyramid does not match the undistorter (size)";
        return nullptr;
    }));
    const size_t nj = members.size();
    auto frame_bytes = [&](size_t j) { const int i = members[j]; return (size_t) g->m[(size_t) i]->wOrg * g->m[(size_t) i]->hOrg * bytes_per_pixel[i]; };
    const UndistGroupLayout L = undist_group_layout(nj, sizeof(UndistJob), frame_bytes);
    CHK(hipSetDevice(g->device));
    hipStream_t st = g->m[0]->stream;
    RUN(async_arena_acquire(g->arena, L.total, st));
    char *const h_stage = g->arena.h_stage, *const d_stage = g->arena.d_stage;
    UndistJob *hJ = (UndistJob *) (h_stage + L.jobs);
    std::vector<FrameRule> rule(nj);
    for (size_t j = 0; j < nj; j++) {
        const int i = members[j];
        const ldso_undistorter *U = g->m[(size_t) i];
        rule[j] = frame_rule(U, exposure[i]);
        memcpy(h_stage + L.frame[j], raw[i], frame_bytes(j));
        const UndistArgs A = frame_args(U, d_stage + L.frame[j], pg ? pg->m[(size_t) i]->d_color : U->d_out, rule[j].mode, factor[i]);
        UndistJob &J = hJ[j];
        J.raw = A.raw; J.G = A.G; J.vig = A.vig; J.remapX = A.remapX; J.remapY = A.remapY; J.out = A.out;
        J.w = A.w; J.h = A.h; J.wOrg = A.wOrg; J.hOrg = A.hOrg; J.mode = A.mode; J.bpp = bytes_per_pixel[i]; J.factor = A.factor; J.pad_ = 0;
    }
    const int wgs = group_prefix((int) nj, (int *) (h_stage + L.first), [&](int j) { return (int) (((size_t) hJ[j].w * hJ[j].h + 255) / 256); });          // 256 pixels per workgroup
    StageClock<3> &clk = g->clock.begin();
    RUN(clk.mark(0, st));
    CHK(hipMemcpyAsync(d_stage, h_stage, L.total, hipMemcpyHostToDevice, st));
    RUN(async_arena_mark_uploaded(g->arena, st));
    RUN(clk.mark(1, st));
    hipLaunchKernelGGL(k_undist_group, dim3((unsigned) wgs), dim3(256), 0, st, (const UndistJob *) (d_stage + L.jobs), (const int *) (d_stage + L.first), (int) nj);
    CHK(hipGetLastError());
    RUN(async_arena_mark_done(g->arena, st));
    RUN(clk.mark(2, st));
    for (size_t j = 0; j < nj; j++) {
        ldso_undistorter *U = g->m[(size_t) members[j]];
        U->last = hJ[j].out;
        CHK(hipEventRecord(U->done, st));
    }
    if (pg) {
        std::vector<const float *> src;
        for (int i : members) src.push_back(pg->m[(size_t) i]->d_color);
        RUN(pyr_group_build(pg, members, src, st));
    }
    RUN(clk.mark(3, st)); clk.defer();
    if (exposure_out) for (size_t j = 0; j < nj; j++) exposure_out[members[j]] = rule[j].exposureOut;
    return LDSO_OK;
}

}  // extern "C"
