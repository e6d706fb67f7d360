// undistort.hip — Undistort::undistort<T> on the device (gfx950; reference src/frontend/Undistort.cc:357-457): the raw 8- or 16-bit camera frame goes up
// (1 or 2 bytes per pixel instead of the 4 of the float irradiance), PhotometricUndistorter::processFrame (:189-227) and the bilinear remap (:390-443) run as
// ONE kernel that writes the irradiance straight into a frame's pyramid staging (ldso_pyramid_t::d_color), and FrameHessian::makeImages (images.hip) follows
// on the same stream.  The irradiance never exists on the host as floats unless the caller asks for it (ldso_undist_get).
//
//   k_undist_frame   one lane per output pixel: its remap entry, four taps of the raw frame (a gather: about 32 bytes per pixel from tables that are L2
//                    resident), the pixel rule of undistort_px.h.  The 256-entry response G is staged in LDS for 8-bit frames; the 65536-entry one of
//                    16-bit frames is read from global memory.  Passthrough (rectification "none", :450-452): the photometric output of pixel idx.
//
// The result is bit for bit what the reference returns (float arithmetic in its operand order, -ffp-contract=off), with the one deliberate difference that
// undistort_px.h states: a pixel whose four taps are not all inside the source image is 0 and nothing outside the raw buffer is read, where the reference
// over-reads one row for the table entry xxi == 0 && yyi == hOrg - 1.  benchmark_varNoise / benchmark_varBlurNoise (:376-413, :468-555) are out of scope.
#include "ba_host.h"
#include "undistort_px.h"

struct UndistArgs {
    const void *raw;                    // wOrg * hOrg pixels of BPP bytes
    const float *G, *vig;               // response (256 / 65536 entries), vignetteMapInv (wOrg * hOrg); read on the calibrated paths only
    const float *remapX, *remapY;       // w * h each, or both null: passthrough
    float *out;                         // w * h
    int w, h, wOrg, hOrg, mode;
    float factor;
};

template <int BPP>
__global__ __launch_bounds__(256) void k_undist_frame(UndistArgs A) {
    __shared__ float Gs[BPP == 1 ? 256 : 1];
    const float *G = A.G;
    if (BPP == 1 && A.mode != UNDIST_PLAIN) {          // block-uniform
        Gs[threadIdx.x] = A.G[threadIdx.x];
        __syncthreads();
        G = Gs;
    }
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= A.w * A.h) return;
    float v;
    if (A.remapX == nullptr) v = undist_photo(A.raw, BPP, idx, G, A.vig, A.mode, A.factor);
    else v = undist_px(A.raw, BPP, G, A.vig, A.mode, A.factor, A.remapX[idx], A.remapY[idx], A.wOrg, A.hOrg);
    A.out[idx] = v;
}

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
struct ldso_undistorter {
    int device = 0, w = 0, h = 0, wOrg = 0, hOrg = 0;
    hipStream_t stream = nullptr;
    bool ownStream = false, hasRemap = false, remapSet = false, hasG = false, useExposure = true, profile = false, profPending = false;
    int GDepth = 0, photometricCalibration = 2;
    float *d_remap = nullptr;           // remapX, then remapY
    float *d_G = nullptr, *d_vig = nullptr, *d_out = nullptr;
    void *d_raw = nullptr;
    void *h_raw[2] = {nullptr, nullptr};          // pinned staging of the raw frame, used alternately: a frame can be staged while the previous one's copy is in flight
    hipEvent_t copied[2] = {};                    // ... recorded behind the copy out of each
    int turn = 0;
    const float *last = nullptr;        // where the last frame's irradiance lies (a pyramid's d_color or d_out)
    hipEvent_t done = nullptr;          // recorded behind the last frame's kernel
    hipEvent_t ev[4] = {};
    float us[3] = {0, 0, 0};
};

extern "C" {

int ldso_undist_destroy(ldso_undistorter_t *U) {
    if (!U) return LDSO_OK;
    hipSetDevice(U->device);
    hipDeviceSynchronize();
    hipFree(U->d_remap); hipFree(U->d_G); hipFree(U->d_vig); hipFree(U->d_out); hipFree(U->d_raw);
    for (void *p : U->h_raw) if (p) hipHostFree(p);
    for (hipEvent_t e : U->copied) if (e) hipEventDestroy(e);
    for (hipEvent_t e : U->ev) if (e) hipEventDestroy(e);
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
    for (hipEvent_t &e : U->ev) ok = ok && hipEventCreate(&e) == hipSuccess;
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
    if (U->profPending) {
        CHK(hipSetDevice(U->device));
        CHK(hipEventSynchronize(U->ev[3]));
        for (int i = 0; i < 3; i++) { float ms = 0; CHK(hipEventElapsedTime(&ms, U->ev[i], U->ev[i + 1])); U->us[i] = ms * 1e3f; }
        U->profPending = false;
    }
    U->profile = enable != 0;
    if (us_out) for (int i = 0; i < 3; i++) us_out[i] = U->us[i];
    return LDSO_OK;
}

int ldso_undist_frame(ldso_undistorter_t *U, const void *raw, int bytes_per_pixel, float exposure, float factor, ldso_pyramid_t *pyr, float *exposure_out) {
    REQ(U && raw && (bytes_per_pixel == 1 || bytes_per_pixel == 2), "ldso_undist_frame: bad arguments (bytes_per_pixel is 1 or 2)");
    REQ(U->remapSet, "ldso_undist_frame: ldso_undist_set_remap has not been called");
    REQ(!pyr || (pyr->device == U->device && pyr->w == U->w && pyr->h == U->h), "ldso_undist_frame: pyramid does not match the undistorter (device, size)");
    // PhotometricUndistorter::processFrame :197-198
    int mode = UNDIST_PLAIN;
    if (U->hasG && exposure > 0 && U->photometricCalibration != 0) mode = U->photometricCalibration == 2 ? UNDIST_VIGNETTE : UNDIST_RESPONSE;
    REQ(mode == UNDIST_PLAIN || bytes_per_pixel == 1 || U->GDepth >= 65536, "ldso_undist_frame: a 16-bit frame needs a response of 65536 entries");
    CHK(hipSetDevice(U->device));
    hipStream_t st = U->stream;
    const size_t bytes = (size_t) U->wOrg * U->hOrg * bytes_per_pixel;
    const int t = U->turn;
    U->turn ^= 1;
    CHK(hipEventSynchronize(U->copied[t]));          // the copy of the frame before last out of this staging buffer: long done
    memcpy(U->h_raw[t], raw, bytes);
    const bool prof = U->profile;
    if (prof) CHK(hipEventRecord(U->ev[0], st));
    CHK(hipMemcpyAsync(U->d_raw, U->h_raw[t], bytes, hipMemcpyHostToDevice, st));
    CHK(hipEventRecord(U->copied[t], st));
    if (prof) CHK(hipEventRecord(U->ev[1], st));
    UndistArgs A;
    const size_t n = (size_t) U->w * U->h;
    A.raw = U->d_raw; A.G = U->d_G; A.vig = U->d_vig;
    A.remapX = U->hasRemap ? U->d_remap : nullptr; A.remapY = U->hasRemap ? U->d_remap + n : nullptr;
    A.out = pyr ? pyr->d_color : U->d_out;
    A.w = U->w; A.h = U->h; A.wOrg = U->wOrg; A.hOrg = U->hOrg; A.mode = mode; A.factor = factor;
    const dim3 grid((unsigned) ((n + 255) / 256));
    if (bytes_per_pixel == 1) hipLaunchKernelGGL(k_undist_frame<1>, grid, dim3(256), 0, st, A);
    else hipLaunchKernelGGL(k_undist_frame<2>, grid, dim3(256), 0, st, A);
    CHK(hipGetLastError());
    CHK(hipEventRecord(U->done, st));
    if (prof) CHK(hipEventRecord(U->ev[2], st));
    U->last = A.out;
    if (pyr) {
        CHK(img_launch_make_images(pyr->d_color, pyr->w, pyr->h, pyr->levels, pyr->lv, st));
        CHK(hipEventRecord(pyr->ready, st));
        pyr->built = true;
    }
    if (prof) { CHK(hipEventRecord(U->ev[3], st)); U->profPending = true; }
    if (exposure_out) *exposure_out = U->useExposure ? exposure : 1.0f;          // :203, :220, :224-225
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

}  // extern "C"
