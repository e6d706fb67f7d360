// images.hip — FrameHessian::makeImages on the device (reference src/internal/FrameHessian.cc:44-113): from the level-0
// irradiance image build the pyramid of 12-byte AoS pixels (I, dx, dy) that the bundle adjustment (level 0) and the coarse
// tracker (all levels) sample.  Level l >= 1 is the 2x2 MEAN of level l-1 (:72-78); gradients are central differences over
// the flat index range [w, w(h-1)) including the row wrap at x = 0 / w-1 (:81-89); rows 0 and h-1 keep zero gradients (the
// reference leaves them uninitialised and never samples them).  Pure streaming: 4 B in / 12 B out per pixel at level 0.
// absSquaredGrad (pixel selector only) is not produced.
#include "hip_host.h"
#include "group_member.h"

// channel 0 of a level (copy of the input or 2x2 mean of the level below), gradients zeroed
__global__ __launch_bounds__(256) void k_img_intensity(const float *__restrict__ color, const float *__restrict__ below, float *__restrict__ dI, int wl, int hl, int wlm1) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= wl * hl) return;
    float v;
    if (below == nullptr) v = color[i];
    else {
        const int x = i % wl, y = i / wl;
        const float *p = below + 3 * (size_t) (2 * x + 2 * y * wlm1);
        v = 0.25f * (((p[0] + p[3]) + p[3 * wlm1]) + p[3 * wlm1 + 3]);
    }
    dI[3 * (size_t) i] = v; dI[3 * (size_t) i + 1] = 0.0f; dI[3 * (size_t) i + 2] = 0.0f;
}

__global__ __launch_bounds__(256) void k_img_gradient(float *__restrict__ dI, int wl, int hl) {
    const int idx = wl + blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= wl * (hl - 1)) return;
    float dx = 0.5f * (dI[3 * (size_t) (idx + 1)] - dI[3 * (size_t) (idx - 1)]);
    float dy = 0.5f * (dI[3 * (size_t) (idx + wl)] - dI[3 * (size_t) (idx - wl)]);
    if (!(fabsf(dx) <= 255.0f)) dx = 0;        // NaN or |.| > 255 (FrameHessian.cc:86-87)
    if (!(fabsf(dy) <= 255.0f)) dy = 0;
    dI[3 * (size_t) idx + 1] = dx;
    dI[3 * (size_t) idx + 2] = dy;
}

// The same two kernels for one level of a group of pyramids (ldso_pyr_group_*): job j is one member that has this level, a workgroup belongs to one job -
// wgFirst[j] workgroups lie in front of job j, wgFirst[nJobs] is the grid (group_member_of: a member whose level needs no workgroups is skipped).  Inside its job a
// lane computes what the solo kernel computes for the same pixel, operation for operation.
struct ImgJob {          // the pointers are typed as device memory (group_member.h: LD_GLOBAL)
    LD_GLOBAL const float *color;     // level 0: the irradiance
    LD_GLOBAL const float *below;     // level l >= 1: level l - 1 of the same member (color is null then)
    LD_GLOBAL float *dI;
    int wl, hl, wlm1, pad_;
};

__global__ __launch_bounds__(256) void k_img_intensity_group(const ImgJob *__restrict__ jobs, const int *__restrict__ wgFirst, int nJobs) {
    const int j = group_member_of(wgFirst, nJobs, (int) blockIdx.x);
    const ImgJob J = jobs[j];
    const int wl = J.wl, hl = J.hl, wlm1 = J.wlm1;
    const int i = ((int) blockIdx.x - wgFirst[j]) * blockDim.x + threadIdx.x;
    if (i >= wl * hl) return;
    float v;
    if (J.below == nullptr) v = J.color[i];
    else {
        const int x = i % wl, y = i / wl;
        const float *p = (const float *) J.below + 3 * (size_t) (2 * x + 2 * y * wlm1);
        v = 0.25f * (((p[0] + p[3]) + p[3 * wlm1]) + p[3 * wlm1 + 3]);
    }
    float *dI = (float *) J.dI;
    dI[3 * (size_t) i] = v; dI[3 * (size_t) i + 1] = 0.0f; dI[3 * (size_t) i + 2] = 0.0f;
}

__global__ __launch_bounds__(256) void k_img_gradient_group(const ImgJob *__restrict__ jobs, const int *__restrict__ wgFirst, int nJobs) {
    const int j = group_member_of(wgFirst, nJobs, (int) blockIdx.x);
    const ImgJob J = jobs[j];
    const int wl = J.wl, hl = J.hl;
    float *dI = (float *) J.dI;
    const int idx = wl + ((int) blockIdx.x - wgFirst[j]) * blockDim.x + threadIdx.x;
    if (idx >= wl * (hl - 1)) return;
    float dx = 0.5f * (dI[3 * (size_t) (idx + 1)] - dI[3 * (size_t) (idx - 1)]);
    float dy = 0.5f * (dI[3 * (size_t) (idx + wl)] - dI[3 * (size_t) (idx - wl)]);
    if (!(fabsf(dx) <= 255.0f)) dx = 0;        // NaN or |.| > 255 (FrameHessian.cc:86-87)
    if (!(fabsf(dy) <= 255.0f)) dy = 0;
    dI[3 * (size_t) idx + 1] = dx;
    dI[3 * (size_t) idx + 2] = dy;
}

// d_color: w*h floats on the device; d_levels[l]: (w>>l)*(h>>l)*3 floats on the device
extern "C" hipError_t img_launch_make_images(const float *d_color, int w, int h, int levels, float *const *d_levels, hipStream_t st) {
    for (int l = 0; l < levels; l++) {
        const int wl = w >> l, hl = h >> l, n = wl * hl;
        hipLaunchKernelGGL(k_img_intensity, dim3((n + 255) / 256), dim3(256), 0, st, l == 0 ? d_color : nullptr, l == 0 ? nullptr : d_levels[l - 1], d_levels[l], wl, hl, w >> (l > 0 ? l - 1 : 0));
        const int m = wl * (hl - 2);
        if (m > 0) hipLaunchKernelGGL(k_img_gradient, dim3((m + 255) / 256), dim3(256), 0, st, d_levels[l], wl, hl);
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------
// ldso_pyramid_t: FrameHessian::dIp of one frame, resident in HBM and shared by pointer - what the reference does on the host
// (CoarseTracker::setCoarseTrackingRef / trackNewestCoarse read fh->dIp[lvl], ImmaturePoint::traceOn and
// PointFrameResidual::linearize read fh->dI = dIp[0]).  One 4-byte-per-pixel upload per frame, every consumer zero-copy.
// ---------------------------------------------------------------------------------------------------------

extern "C" {

int ldso_pyr_create(int device, int w, int h, int levels, ldso_pyramid_t **out) {
    REQ(out && w > 16 && h > 16 && levels >= 1 && levels <= LDSO_PYR_LEVELS && (w >> (levels - 1)) > 2 && (h >> (levels - 1)) > 2, "ldso_pyr_create: bad arguments");
    RUN(open_device(device, "ldso_pyr_create"));
    ldso_pyramid *P = new ldso_pyramid();
    P->device = device; P->w = w; P->h = h; P->levels = levels;
    size_t total = 0;
    for (int l = 0; l < levels; l++) total += (size_t) (w >> l) * (h >> l) * 3;
    // ONE allocation for all levels (each level 16-byte aligned) + the raw image
    size_t off = 0, offs[LDSO_PYR_LEVELS];
    for (int l = 0; l < levels; l++) { offs[l] = off; off += (((size_t) (w >> l) * (h >> l) * 3) + 3) & ~(size_t) 3; }
    if (hipMalloc((void **) &P->base, (off + (size_t) w * h) * sizeof(float)) != hipSuccess) { delete P; ldso_set_error("ldso_pyr_create: out of device memory"); return LDSO_E_HIP; }
    for (int l = 0; l < levels; l++) P->lv[l] = P->base + offs[l];
    P->d_color = P->base + off;
    if (hipEventCreateWithFlags(&P->ready, hipEventDisableTiming) != hipSuccess) { hipFree(P->base); delete P; ldso_set_error("ldso_pyr_create: hipEventCreate failed"); return LDSO_E_HIP; }
    *out = P;
    return LDSO_OK;
}

int ldso_pyr_destroy(ldso_pyramid_t *P) {
    if (!P) return LDSO_OK;
    REQ(P->inGroup == nullptr, "ldso_pyr_destroy: the pyramid is a member of a live group (ldso_pyr_group_destroy first: the group dereferences its members)");
    hipSetDevice(P->device);
    hipDeviceSynchronize();          // consumers may still be reading the levels
    if (P->ready) hipEventDestroy(P->ready);
    hipFree(P->base);
    delete P;
    return LDSO_OK;
}

// FrameHessian::makeImages (FrameHessian.cc:44-113) from a device-resident irradiance image: enqueued on `hip_stream`, consumers wait
// on the pyramid's event (no host synchronisation).
int ldso_pyr_make_images_device(ldso_pyramid_t *P, const void *irradiance_dev, void *hip_stream) {
    REQ(P && irradiance_dev, "ldso_pyr_make_images_device: bad arguments");
    CHK(hipSetDevice(P->device));
    hipStream_t st = (hipStream_t) hip_stream;
    CHK(img_launch_make_images((const float *) irradiance_dev, P->w, P->h, P->levels, P->lv, st));
    CHK(hipEventRecord(P->ready, st));
    P->built = true;
    return LDSO_OK;
}

// the same from a host image (w*h floats): 4 bytes per pixel cross PCIe, once per frame
int ldso_pyr_make_images(ldso_pyramid_t *P, const float *irradiance, void *hip_stream) {
    REQ(P && irradiance, "ldso_pyr_make_images: bad arguments");
    CHK(hipSetDevice(P->device));
    hipStream_t st = (hipStream_t) hip_stream;
    CHK(hipMemcpyAsync(P->d_color, irradiance, (size_t) P->w * P->h * sizeof(float), hipMemcpyHostToDevice, st));
    return ldso_pyr_make_images_device(P, P->d_color, hip_stream);
}

// ---------------------------------------------------------------------------------------------------------
// ldso_pyr_group_*: FrameHessian::makeImages (FrameHessian.cc:44-113) of the new frames of several sequences.  One ldso_pyr_make_images is 2 x levels small
// launches; the group builds level l of every active member that has one in two launches (intensity, gradient), 2 x Lmax per call whatever n, with the job tables
// of all levels in one upload.
// ---------------------------------------------------------------------------------------------------------

static constexpr GroupRule PYR_RULE = {"a pyramid", nullptr, GROUP_MAX_MEMBERS};          // no stream of their own: it is an argument of each call
static_assert(sizeof(ImgJob) == 40, "the row of pyr_group_layout as tests/test_group_stage_cpu.py sizes it");

int ldso_pyr_group_create(ldso_pyramid_t *const *pyramids, int n, ldso_pyr_group_t **out) {
    RUN(group_admit(pyramids, n, out, "ldso_pyr_group_create", PYR_RULE));
    CHK(hipSetDevice(pyramids[0]->device));
    ldso_pyr_group *g = new ldso_pyr_group();
    g->device = pyramids[0]->device;
    RUN(finish_create(async_arena_create(g->arena), g, out, ldso_pyr_group_destroy));
    g->m.assign(pyramids, pyramids + n);
    group_join(g);
    return LDSO_OK;
}

int ldso_pyr_group_destroy(ldso_pyr_group_t *g) {
    if (!g) return LDSO_OK;
    hipSetDevice(g->device);
    group_leave(g);
    async_arena_release(g->arena);          // waits for the last call's kernels
    delete g;
    return LDSO_OK;
}

// the build of every active member from src[i] (device memory: the member's own d_color behind an upload or behind ldso_undist_group_frames' kernel, or the
// caller's image); declared in hip_host.h
extern "C++" int pyr_group_build(ldso_pyr_group *g, const std::vector<int> &members, const std::vector<const float *> &src, hipStream_t st) {
    const size_t nm = members.size();
    int Lmax = 0;
    for (int i : members) Lmax = std::max(Lmax, g->m[(size_t) i]->levels);
    const PyrGroupLayout plan = pyr_group_layout(Lmax, sizeof(ImgJob), [&](int l) { int nl = 0; for (int i : members) nl += g->m[(size_t) i]->levels > l; return nl; });
    RUN(async_arena_acquire(g->arena, plan.total, st));
    char *const h_stage = g->arena.h_stage, *const d_stage = g->arena.d_stage;
    int gridI[LDSO_PYR_LEVELS], gridG[LDSO_PYR_LEVELS];
    for (int l = 0; l < Lmax; l++) {
        const PyrLevelLayout &L = plan.level[(size_t) l];
        ImgJob *hJ = (ImgJob *) (h_stage + L.jobs);
        int j = 0;
        for (size_t k = 0; k < nm; k++) {
            const ldso_pyramid *P = g->m[(size_t) members[k]];
            if (P->levels <= l) continue;
            const int wl = P->w >> l, hl = P->h >> l;
            ImgJob &J = hJ[j++];
            J.color = (LD_GLOBAL const float *) (l == 0 ? src[k] : nullptr); J.below = (LD_GLOBAL const float *) (l == 0 ? nullptr : P->lv[l - 1]); J.dI = (LD_GLOBAL float *) P->lv[l];
            J.wl = wl; J.hl = hl; J.wlm1 = P->w >> (l > 0 ? l - 1 : 0); J.pad_ = 0;
        }
        // the workgroups of the two launches: 256 pixels each; the gradient has the rows 1 .. hl - 2
        gridI[l] = group_prefix(L.nl, (int *) (h_stage + L.firstI), [&](int q) { return (hJ[q].wl * hJ[q].hl + 255) / 256; });
        gridG[l] = group_prefix(L.nl, (int *) (h_stage + L.firstG), [&](int q) { const int nGrad = hJ[q].wl * (hJ[q].hl - 2); return nGrad > 0 ? (nGrad + 255) / 256 : 0; });
    }
    CHK(hipMemcpyAsync(d_stage, h_stage, plan.total, hipMemcpyHostToDevice, st));
    RUN(async_arena_mark_uploaded(g->arena, st));
    for (int l = 0; l < Lmax; l++) {
        const PyrLevelLayout &L = plan.level[(size_t) l];
        const ImgJob *dJ = (const ImgJob *) (d_stage + L.jobs);
        hipLaunchKernelGGL(k_img_intensity_group, dim3(gridI[l]), dim3(256), 0, st, dJ, (const int *) (d_stage + L.firstI), L.nl);
        if (gridG[l] > 0) hipLaunchKernelGGL(k_img_gradient_group, dim3(gridG[l]), dim3(256), 0, st, dJ, (const int *) (d_stage + L.firstG), L.nl);
    }
    CHK(hipGetLastError());
    RUN(async_arena_mark_done(g->arena, st));
    for (int i : members) { ldso_pyramid *P = g->m[(size_t) i]; CHK(hipEventRecord(P->ready, st)); P->built = true; }
    return LDSO_OK;
}

static int pyr_group_members(ldso_pyr_group *g, const uint8_t *active, const void *const *images, const char *who, std::vector<int> &members) {
    REQ(g && images, std::string(who) + ": null argument");
    return group_active((int) g->m.size(), active, who, members, [&](int i) { return images[i] ? nullptr : "null image"; });
}

int ldso_pyr_group_make_images_device(ldso_pyr_group_t *g, const uint8_t *active, const void *const *irradiance_dev, void *hip_stream) {
    std::vector<int> members;
    RUN(pyr_group_members(g, active, irradiance_dev, "ldso_pyr_group_make_images_device", members));
    CHK(hipSetDevice(g->device));
    std::vector<const float *> src;
    for (int i : members) src.push_back((const float *) irradiance_dev[i]);
    return pyr_group_build(g, members, src, (hipStream_t) hip_stream);
}

// from host images: every image goes straight into its pyramid's own d_color on the stream (the bytes dominate: no second staging copy on the host)
int ldso_pyr_group_make_images(ldso_pyr_group_t *g, const uint8_t *active, const float *const *irradiance, void *hip_stream) {
    std::vector<int> members;
    RUN(pyr_group_members(g, active, (const void *const *) irradiance, "ldso_pyr_group_make_images", members));
    CHK(hipSetDevice(g->device));
    hipStream_t st = (hipStream_t) hip_stream;
    std::vector<const float *> src;
    for (int i : members) {
        ldso_pyramid *P = g->m[(size_t) i];
        CHK(hipMemcpyAsync(P->d_color, irradiance[i], (size_t) P->w * P->h * sizeof(float), hipMemcpyHostToDevice, st));
        src.push_back(P->d_color);
    }
    return pyr_group_build(g, members, src, st);
}

int ldso_pyr_level(ldso_pyramid_t *P, int lvl, const void **dev_ptr, int *wl, int *hl) {
    REQ(P && lvl >= 0 && lvl < P->levels, "ldso_pyr_level: bad arguments");
    if (dev_ptr) *dev_ptr = P->lv[lvl];
    if (wl) *wl = P->w >> lvl;
    if (hl) *hl = P->h >> lvl;
    return LDSO_OK;
}

int ldso_pyr_get_level(ldso_pyramid_t *P, int lvl, float *out) {
    REQ(P && out && lvl >= 0 && lvl < P->levels && P->built, "ldso_pyr_get_level: bad arguments (or no image yet)");
    CHK(hipSetDevice(P->device));
    CHK(hipEventSynchronize(P->ready));
    CHK(hipMemcpy(out, P->lv[lvl], (size_t) (P->w >> lvl) * (P->h >> lvl) * 3 * sizeof(float), hipMemcpyDeviceToHost));
    return LDSO_OK;
}

}  // extern "C"
