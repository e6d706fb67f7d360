// hip_host.h — what every host-side translation unit that talks to HIP shares, in this order: the error check of a HIP call, the launch with dynamic LDS, the
// staging arenas of the grouped calls and the pyramid group (its build crosses into undistort.hip) as types; then, hidden (none is part of the library's
// interface), the head and tail of a create function, zeroed allocations, the stream swap, the growth of an arena and the arenas' functions, the hand-over of a
// pyramid, the timing of repeated launches, and the clock of a staged timing split.  Nothing of the bundle adjustment or the tracer: those are ba_host.h and
// trace.h, which include this file.  A next stage includes this header; a next staged split uses StageClock.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdio>
#include "host_only.h"          // ldso_set_error, REQ, RUN
#include "group_stage.h"        // align_up; membership, active list, prefix table and arena layouts of the grouped calls
#include "pyramid.h"

#define CHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { ldso_set_error(std::string(#call) + ": " + hipGetErrorString(e_)); return LDSO_E_HIP; } } while (0)

// A launch with dynamic LDS: above 48 KB the kernel's limit is raised first; the status of that call is no reason to skip the launch, whose own error the caller sees
template <class Kernel, class... Args>
hipError_t launch_lds(Kernel kernel, dim3 grid, dim3 block, size_t ldsBytes, hipStream_t st, const Args &... args) {
    if (ldsBytes > 48 * 1024) (void) hipFuncSetAttribute((const void *) kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) ldsBytes);
    hipLaunchKernelGGL(kernel, grid, block, ldsBytes, st, args...);
    return hipGetLastError();
}

// The staging arena of a grouped call (group_stage.h: the layouts): one pinned arena and its device twin, grown on demand.  The tracker and tracer groups end every
// call with a host wait, so the next call finds both sides free.
struct GroupArena { char *h_stage = nullptr, *d_stage = nullptr; size_t stageCap = 0; };
// The same for a group whose calls do NOT wait on the host (pyramid and undistorter groups).  The pinned side is free once the last upload has been read: `uploaded`,
// recorded behind the copy, guards it against the next call's writes.  The device side is free once the last call's kernels are through: in stream order on the
// same stream, behind `done` (recorded behind the last launch) on another.  A replacement of the pair waits for `done` on the host.
struct AsyncArena : GroupArena {
    hipEvent_t uploaded = nullptr, done = nullptr;
    hipStream_t lastStream = nullptr;
    bool used = false;
};

// a group of pyramids whose builds share launches (images.hip)
struct ldso_pyr_group {
    std::vector<ldso_pyramid *> m;
    int device = 0;
    AsyncArena arena;
};

#pragma GCC visibility push(hidden)
// The head of a create function: a device must be visible, `device` must name one, and it becomes the current one.
inline int open_device(int device, const char *who) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { ldso_set_error("no HIP device visible"); return LDSO_E_NODEVICE; }
    REQ(device >= 0 && device < ndev, std::string(who) + ": device index out of range");
    CHK(hipSetDevice(device));
    return LDSO_OK;
}
// The tail of a create function whose body may fail half-way: the handle's own destroy frees whatever a half-built handle holds, the error text of the failure is kept.
template <class Handle, class Destroy> int finish_create(int r, Handle *H, Handle **out, Destroy destroy) {
    if (r != LDSO_OK) { const std::string keep = ldso_last_error(); destroy(H); ldso_set_error(keep); return r; }
    *out = H; return LDSO_OK;
}
// Zero-fill of fresh device memory, waited for: hipMemset on device memory is asynchronous (legacy null stream) and the handles work on NON-BLOCKING streams,
// which do not order themselves behind it: without the wait a zero-fill that is still queued (the null stream busy with another library's work, e.g. torch's)
// could land on top of data the handle's first uploads / kernels have already written
inline int zero_fill(void *p, size_t bytes) { CHK(hipMemset(p, 0, bytes)); CHK(hipStreamSynchronize(nullptr)); return LDSO_OK; }
// n zeroed elements of device memory, recorded in `allocs` (what the handle's destroy frees)
template <class T> int dalloc(std::vector<void *> &allocs, T **p, size_t n) {
    const size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
    CHK(hipMalloc((void **) p, bytes));
    allocs.push_back(*p);
    return zero_fill(*p, bytes);
}
#define DALLOC(allocs, ptr, n) RUN(dalloc(allocs, &(ptr), (n)))
// *_set_stream: the caller's stream `s` instead of the handle's own non-blocking one (which is drained and destroyed), or, with s == nullptr, an own one again
inline int swap_stream(hipStream_t &stream, bool &ownStream, void *s) {
    if (ownStream && stream) { hipStreamSynchronize(stream); if (s) { hipStreamDestroy(stream); ownStream = false; } }
    if (s) { stream = (hipStream_t) s; ownStream = false; }
    else if (!ownStream) { CHK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking)); ownStream = true; }
    return LDSO_OK;
}
// A pinned arena and its device twin (the handle's h_stage / d_stage, the batch's) with room for `need` bytes.  A pair that is too small is replaced by one of
// need + need / slackDiv bytes once `st`, the stream whose work may still read the old pair, has drained.
inline int grow_arena(char *&h, char *&d, size_t &cap, size_t need, size_t slackDiv, hipStream_t st) {
    if (need <= cap) return LDSO_OK;
    CHK(hipStreamSynchronize(st));
    if (h) (void) hipHostFree(h);
    if (d) (void) hipFree(d);
    h = nullptr; d = nullptr; cap = 0;
    const size_t room = need + need / slackDiv;
    CHK(hipHostMalloc((void **) &h, room));
    CHK(hipMalloc((void **) &d, room));
    cap = room;
    return LDSO_OK;
}
// the arena of a group with room for `need` bytes; `st` = the stream of the group's calls
inline int group_arena_grow(GroupArena &A, size_t need, hipStream_t st) { return grow_arena(A.h_stage, A.d_stage, A.stageCap, need, 2, st); }
inline void group_arena_free(GroupArena &A) {          // at destroy
    if (A.h_stage) (void) hipHostFree(A.h_stage);
    if (A.d_stage) (void) hipFree(A.d_stage);
}
inline int async_arena_create(AsyncArena &A) {
    CHK(hipEventCreateWithFlags(&A.uploaded, hipEventDisableTiming));
    CHK(hipEventCreateWithFlags(&A.done, hipEventDisableTiming));
    return LDSO_OK;
}
// both sides of the arena free for a call of `total` bytes on `st` (the rule beside AsyncArena), and large enough
inline int async_arena_acquire(AsyncArena &A, size_t total, hipStream_t st) {
    if (A.used) CHK(hipEventSynchronize(A.uploaded));
    if (A.used && (total > A.stageCap || st != A.lastStream)) CHK(hipStreamWaitEvent(st, A.done, 0));
    if (A.used && total > A.stageCap) CHK(hipEventSynchronize(A.done));
    return group_arena_grow(A, total, st);
}
inline int async_arena_mark_uploaded(AsyncArena &A, hipStream_t st) { CHK(hipEventRecord(A.uploaded, st)); return LDSO_OK; }          // behind the call's one copy
inline int async_arena_mark_done(AsyncArena &A, hipStream_t st) {          // behind the last launch that reads the device side
    CHK(hipEventRecord(A.done, st));
    A.used = true; A.lastStream = st;
    return LDSO_OK;
}
inline void async_arena_release(AsyncArena &A) {          // at destroy
    if (A.used) (void) hipEventSynchronize(A.done);          // the last call's kernels read the device side
    if (A.uploaded) (void) hipEventDestroy(A.uploaded);
    if (A.done) (void) hipEventDestroy(A.done);
    group_arena_free(A);
}
// A resident pyramid handed to a consumer `what` (named in the message): it holds an image and matches in device, size and levels; then `st` waits for its build.
inline int pyramid_wait(const ldso_pyramid *pyr, int device, int w, int h, int minLevels, hipStream_t st, const char *who, const char *what) {
    REQ(pyr->built && pyr->device == device && pyr->w == w && pyr->h == h && pyr->levels >= minLevels, std::string(who) + ": pyramid does not match " + what + " or holds no image");
    CHK(hipSetDevice(device));
    CHK(hipStreamWaitEvent(st, pyr->ready, 0));
    return LDSO_OK;
}
// Raw level-0 irradiance on the host (w * h floats) -> `levels` images (images.hip): staging buffer on first use, upload, kernels, all on `st`; the caller waits or not.
inline int raw_to_images(float *&d_color, const float *irradiance, int w, int h, int levels, float *const *d_levels, hipStream_t st) {
    if (!d_color) CHK(hipMalloc(&d_color, (size_t) w * h * sizeof(float)));
    CHK(hipMemcpyAsync(d_color, irradiance, (size_t) w * h * sizeof(float), hipMemcpyHostToDevice, st));
    CHK(img_launch_make_images(d_color, w, h, levels, d_levels, st));
    return LDSO_OK;
}

// images.hip: the grouped FrameHessian::makeImages of the members `members` of g (indices into g->m) from src[k] = the level-0 irradiance of members[k] in device
// memory, enqueued on `st` without a host wait; records the members' `ready` events and `built` flags (ldso_pyr_group_make_images*, ldso_undist_group_frames)
int pyr_group_build(ldso_pyr_group *g, const std::vector<int> &members, const std::vector<const float *> &src, hipStream_t st);
// one warm launch, then `reps` launches between ONE pair of HIP events on `st` (the event overhead is amortised over them): microseconds per launch
template <class Launch> int time_launches(hipStream_t st, int reps, double *avg_us, Launch launch) {
    hipEvent_t a, b;
    CHK(hipEventCreate(&a)); CHK(hipEventCreate(&b));
    RUN(launch());          // warm
    CHK(hipEventRecord(a, st));
    for (int i = 0; i < reps; i++) RUN(launch());
    CHK(hipEventRecord(b, st));
    CHK(hipEventSynchronize(b));
    float ms = 0;
    CHK(hipEventElapsedTime(&ms, a, b));
    (void) hipEventDestroy(a); (void) hipEventDestroy(b);
    *avg_us = (double) ms * 1e3 / reps;
    return LDSO_OK;
}

// The clock of a call that is timed stage by stage (ldso_feat_*, ldso_pixsel_*, ldso_undist_* and their groups): N stages between N + 1 boundaries, each an event
// recorded where the boundary lies in the stream order, in profiled calls only.  The handle's *_profile entry sets the switch; a call samples it once (begin),
// so every mark of an unprofiled call is one untaken branch, and mark / lap / read / set / defer of such a call do nothing.  A call that marks without its own
// begin is a bug: it would run on what the call before sampled.  The stored values are the last measurement: zeros before the first, untouched by unprofiled calls.
template <int N> class StageClock {
    bool on = false, live = false, pending = false;          // the switch; this call is profiled; a profiled call's events are recorded but not read yet
    hipEvent_t ev[N + 1] = {};
    float us[N] = {};
    // microseconds between the boundaries k and k + 1, both reached (the caller has waited for the stream or for the later event)
    int elapsed(int k, float &out) const { float ms = 0; CHK(hipEventElapsedTime(&ms, ev[k], ev[k + 1])); out = ms * 1e3f; return LDSO_OK; }
public:
    int create() { for (hipEvent_t &e : ev) CHK(hipEventCreate(&e)); return LDSO_OK; }          // a failure leaves the rest null: destroy copes with a half-made clock
    void destroy() { for (hipEvent_t e : ev) if (e) (void) hipEventDestroy(e); }
    StageClock &begin() { live = on; return *this; }          // the head of every call that marks
    int mark(int k, hipStream_t st) { if (live) CHK(hipEventRecord(ev[k], st)); return LDSO_OK; }          // boundary k
    int lap(int k, float &out) const { return live ? elapsed(k, out) : LDSO_OK; }          // stage k of this call into `out` (a call that sums a stage over several rounds)
    void set(int k, float v) { if (live) us[k] = v; }                                     // ... and what it summed as the stored value
    int read(int k) { return lap(k, us[k]); }                                             // stage k of this call as the stored value
    int read() { for (int k = 0; k < N; k++) RUN(read(k)); return LDSO_OK; }          // all stages, behind the call's wait
    void defer() { if (live) pending = true; }          // a call that does not wait: the next settle reads its stages
    int settle(int device) {
        if (!pending) return LDSO_OK;
        CHK(hipSetDevice(device)); CHK(hipEventSynchronize(ev[N]));
        for (int k = 0; k < N; k++) RUN(elapsed(k, us[k]));
        pending = false; return LDSO_OK;
    }
    // the body of a *_profile entry: a pending measurement is waited for and read, the switch is set, the last measurement goes out
    int report(int device, int enable, float *us_out) {
        RUN(settle(device));
        on = enable != 0;
        if (us_out) for (int k = 0; k < N; k++) us_out[k] = us[k];
        return LDSO_OK;
    }
};
#pragma GCC visibility pop
