// ba_api.hip — C-ABI (include/ldso_hip.h) of the windowed bundle adjustment: the handle and its device memory, images, frames and prior,
// fetchers, debug getters.  The window (upload, edits, chunks) is ba_window.hip, the kernel sequencing ba_optimize.hip, batches ba_batch.hip,
// the multi-GPU paths ba_dist.hip; what they share is ba_host.h.
#include "ba_host.h"
#include "lie_dev.h"

static thread_local std::string g_err;
void ldso_set_error(const std::string &s) { g_err = s; }

// the device records of the frames and the calibration as ldso_ba_set_frames / ldso_ba_batch_set_frames upload them
void fill_dev_frames(const ldso_ba *H, const ldso_frame_t *fr, const ldso_calib_t *calib, DevFrame *df, DevCalib *dc) {
    const int F = H->D.F;
    for (int f = 0; f < F; f++) {
        DevFrame &d = df[f];
        memset(&d, 0, sizeof(d));
        memcpy(d.evalPT, fr[f].worldToCam_evalPT, sizeof(d.evalPT));
        memcpy(d.state, fr[f].state, sizeof(d.state)); memcpy(d.state_zero, fr[f].state_zero, sizeof(d.state_zero));
        memcpy(d.state_backup, fr[f].state, sizeof(d.state));
        memcpy(d.prior, fr[f].prior, sizeof(d.prior));
        memcpy(d.ns_pose, fr[f].nullspaces_pose, sizeof(d.ns_pose)); memcpy(d.ns_scale, fr[f].nullspaces_scale, sizeof(d.ns_scale));
        memcpy(d.ns_affine, fr[f].nullspaces_affine, sizeof(d.ns_affine));
        d.ab_exposure = fr[f].ab_exposure; d.frameEnergyTH = fr[f].frameEnergyTH; d.frameID = fr[f].frameID; d.imgSlot = H->imageSlot[f];
    }
    memset(dc, 0, sizeof(*dc));
    for (int i = 0; i < 4; i++) { dc->value[i] = calib->value[i]; dc->value_zero[i] = calib->value_zero[i]; dc->value_backup[i] = calib->value[i]; }
}

extern "C" {

int ldso_version(void) { return 100; }
const char *ldso_last_error(void) { return g_err.c_str(); }
int ldso_device_count(void) { int n = 0; if (hipGetDeviceCount(&n) != hipSuccess) return 0; return n; }

int ldso_settings_default(ldso_settings_t *s) {
    if (!s) return LDSO_E_INVALID;
    memset(s, 0, sizeof(*s));
    s->huberTH = 9; s->outlierTHSumComponent = 50 * 50; s->affineOptModeA = 1e12f; s->affineOptModeB = 1e8f;
    s->frameEnergyTHN = 0.7f; s->frameEnergyTHFacMedian = 1.5f; s->frameEnergyTHConstWeight = 0.5f; s->overallEnergyTHWeight = 1;
    s->initialCalibHessian = 5e9f; s->margWeightFac = 0.5f * 0.5f; s->idepthFixPriorMargFac = 600 * 600; s->thOptIterations = 1.2f;
    s->coarseCutoffTH = 20; s->minOptIterations = 1; s->solverMode = LDSO_SOLVER_FIX_LAMBDA | LDSO_SOLVER_ORTHOGONALIZE_X_LATER;
    s->forceAcceptStep = 1; s->solverModeDelta = 0.00001;
    return LDSO_OK;
}

int ldso_pyr_levels_used(int w, int h) {
    int wl = w, hl = h, lv = 1;
    while (wl % 2 == 0 && hl % 2 == 0 && wl * hl > 5000 && lv < LDSO_PYR_LEVELS) { wl /= 2; hl /= 2; lv++; }
    return lv;
}

int ldso_frame_set_evalPT(ldso_frame_t *f, const double worldToCam[12], const double state[10]) {
    if (!f || !worldToCam || !state) return LDSO_E_INVALID;
    memcpy(f->worldToCam_evalPT, worldToCam, 12 * sizeof(double));
    memcpy(f->state, state, 10 * sizeof(double));
    memcpy(f->state_zero, state, 10 * sizeof(double));
    ld::frame_nullspaces(f->worldToCam_evalPT, f->state_zero[6], f->ab_exposure, f->nullspaces_pose, f->nullspaces_scale, f->nullspaces_affine);
    return LDSO_OK;
}

int ldso_frame_set_prior(ldso_frame_t *f, const ldso_settings_t *s) {
    if (!f || !s) return LDSO_E_INVALID;
    for (int i = 0; i < 8; i++) f->prior[i] = 0;
    // Setting.cc:18-21: `float` globals in the reference - the double prior vector receives the float values (1e11f = 99999997952, 1e14f = 100000000376832)
    const double initialRotPrior = (double) 1e11f, initialTransPrior = (double) 1e10f, initialAffBPrior = (double) 1e14f, initialAffAPrior = (double) 1e14f;
    if (f->frameID == 0) {
        for (int i = 0; i < 3; i++) { f->prior[i] = initialTransPrior; f->prior[3 + i] = initialRotPrior; }
        if (s->solverMode & LDSO_SOLVER_REMOVE_POSEPRIOR) for (int i = 0; i < 6; i++) f->prior[i] = 0;
        f->prior[6] = initialAffAPrior; f->prior[7] = initialAffBPrior;
    } else {
        f->prior[6] = (s->affineOptModeA < 0) ? initialAffAPrior : (double) s->affineOptModeA;
        f->prior[7] = (s->affineOptModeB < 0) ? initialAffBPrior : (double) s->affineOptModeB;
    }
    return LDSO_OK;
}

// ---------------------------------------------------------------------------------------------------------
}  // extern "C"
// the fetch functions read the device tables through ONE pinned arena: reserve what the call needs (growth invalidates nothing: it happens before
// the first copy is enqueued), enqueue the copies back to back, wait once, read in place.  (std::vector destinations are pageable memory: the
// runtime stages them in small pieces - ldso_ba_get_residuals of a C3 window took 0.35 ms for 1 MB.)
static int down_reserve(ldso_ba *H, size_t bytes) {
    if (bytes <= H->downCap) return LDSO_OK;
    CHK(hipStreamSynchronize(H->stream));
    if (H->h_down) (void) hipHostFree(H->h_down);
    H->h_down = nullptr; H->downCap = 0;
    const size_t cap = bytes + bytes / 2 + 4096;
    CHK(hipHostMalloc((void **) &H->h_down, cap));
    H->downCap = cap;
    return LDSO_OK;
}
template <class T> static const T *down_put(ldso_ba *H, size_t &used, const T *src, size_t n, int &rc) {
    const size_t bytes = (n * sizeof(T) + 63) & ~(size_t) 63;
    const T *p = reinterpret_cast<const T *>(H->h_down + used);
    if (rc == LDSO_OK && n) { if (hipMemcpyAsync(H->h_down + used, src, n * sizeof(T), hipMemcpyDeviceToHost, H->stream) != hipSuccess) { ldso_set_error("hipMemcpyAsync (fetch) failed"); rc = LDSO_E_HIP; } }
    used += bytes;
    return p;
}

template <class T> static int d2h(ldso_ba *H, std::vector<T> &dst, const T *src, size_t n) {
    dst.resize(n);
    if (n == 0) return LDSO_OK;
    CHK(hipMemcpyAsync(dst.data(), src, n * sizeof(T), hipMemcpyDeviceToHost, H->stream));
    return LDSO_OK;
}
extern "C" {

static int alloc_set(ldso_ba *H, ResSet &S) {
    const size_t P = H->maxP, FS = H->FSmax, PS = P * FS, C = H->maxChunks;
    DALLOC(H->allocs, S.slot, PS); DALLOC(H->allocs, S.pt, P); DALLOC(H->allocs, S.acc, P); DALLOC(H->allocs, S.candE, P);
    DALLOC(H->allocs, S.G, P * (8 * FS + LD_GEXTRA)); DALLOC(H->allocs, S.topA, C * FS * LD_TOPN); DALLOC(H->allocs, S.topL, C * FS * LD_TOPN);
    DALLOC(H->allocs, S.chunkEnergy, C); DALLOC(H->allocs, S.chunkCnt, C * 2); DALLOC(H->allocs, S.chunkNID, C * 2);
    return LDSO_OK;
}

static int create_body(ldso_ba *H, int device, int w, int h, int max_frames, int max_points) {
    H->device = device; H->w = w; H->h = h; H->maxF = max_frames; H->maxP = max_points;
    H->FSmax = (max_frames + 7) / 8 * 8;
    H->maxChunks = max_points / 4 + max_frames + 4;
    { hipDeviceProp_t pr; if (hipGetDeviceProperties(&pr, device) == hipSuccess && pr.multiProcessorCount > 0) H->numCU = pr.multiProcessorCount; }
    ldso_settings_default(&H->settings);
    CHK(hipStreamCreateWithFlags(&H->stream, hipStreamNonBlocking));
    H->ownStream = true;
    CHK(hipHostMalloc((void **) &H->h_item, sizeof(BatchItem)));
    { void *q_ = nullptr; CHK(hipMalloc(&q_, sizeof(BatchItem))); H->d_item = (BatchItem *) q_; }
    { void *q_ = nullptr; CHK(hipMalloc(&q_, (size_t) H->maxChunks * sizeof(BatchBlock))); H->d_blocks = (BatchBlock *) q_; }
    CHK(hipHostMalloc((void **) &H->h_stop, 4 * sizeof(int), hipHostMallocMapped));
    CHK(hipHostGetDevicePointer((void **) &H->d_stop, H->h_stop, 0));
    memset(&H->B, 0, sizeof(H->B));
    memset(&H->D, 0, sizeof(H->D));
    BaPtrs &B = H->B;
    const size_t F = max_frames, P = max_points, FS = H->FSmax, nmax = 8 * F + 4;
    DALLOC(H->allocs, B.frames, F); DALLOC(H->allocs, B.calib, 1); DALLOC(H->allocs, B.pairs, F * F); DALLOC(H->allocs, B.pairRt, F * F * 12);
    DALLOC(H->allocs, B.adHost, F * F * 64); DALLOC(H->allocs, B.adTarget, F * F * 64); DALLOC(H->allocs, B.adHostF, F * F * 64); DALLOC(H->allocs, B.adTargetF, F * F * 64);
    DALLOC(H->allocs, B.nsProj, nmax * 7); DALLOC(H->allocs, B.HM, nmax * nmax); DALLOC(H->allocs, B.bM, nmax);
    DALLOC(H->allocs, B.pgeo, P); DALLOC(H->allocs, B.pcw, P * 8); DALLOC(H->allocs, B.phost, P);
    DALLOC(H->allocs, B.rtab, P * FS);
    DALLOC(H->allocs, B.Jlin, P * FS); DALLOC(H->allocs, B.rtz, P * FS * 8);
    DALLOC(H->allocs, B.chunk_p0, H->maxChunks); DALLOC(H->allocs, B.chunk_n, H->maxChunks); DALLOC(H->allocs, B.chunk_host, H->maxChunks);
    DALLOC(H->allocs, H->d_chunkStart, F + 2);
    DALLOC(H->allocs, H->d_waitCtr, LD_ARRIVE_SHARDS * LD_ARRIVE_STRIDE);          // hipMalloc aligns to 256 bytes and more: every arrival word on a line of its own
    DALLOC(H->allocs, H->d_margFlags, P);
    DALLOC(H->allocs, B.pairC, 2 * F * F * LD_PAIRC);
    const size_t GSPmax = (8 * FS + LD_GEXTRA + 15) / 16 * 16;
    DALLOC(H->allocs, B.scPart, (size_t) LD_SC_SPLITS * GSPmax * GSPmax);
    DALLOC(H->allocs, B.sys, 4 * (nmax * nmax + nmax));
    DALLOC(H->allocs, B.acc, nmax * nmax + nmax); H->ownAcc = B.acc;
    DALLOC(H->allocs, B.x, nmax); DALLOC(H->allocs, B.xAd, F * F * 8); DALLOC(H->allocs, B.xc, 4); DALLOC(H->allocs, B.scalars, 16); DALLOC(H->allocs, B.energyLog, 64);
    DALLOC(H->allocs, H->d_dumpJ, P * FS);
    B.dumpJ = nullptr;
    int r;
    if ((r = alloc_set(H, H->sets[0])) != LDSO_OK) return r;
    if ((r = alloc_set(H, H->sets[1])) != LDSO_OK) return r;
    return LDSO_OK;
}

int ldso_ba_create(int device, int w, int h, int max_frames, int max_points, ldso_ba_t **out) {
    REQ(out && w > 8 && h > 8 && max_frames >= 2 && max_frames <= LD_MAXF && max_points > 0, "ldso_ba_create: bad arguments");
    *out = nullptr;
    RUN(open_device(device, "ldso_ba_create"));
    ldso_ba *H = new ldso_ba();
    { const char *e = getenv("LDSO_GN_GRAPHS"); if (e && e[0] == '0') H->gnUseGraphs = false; }
    return finish_create(create_body(H, device, w, h, max_frames, max_points), H, out, ldso_ba_destroy);      // nothing of a half-built handle leaks
}

int ldso_ba_destroy(ldso_ba_t *H) {
    if (!H) return LDSO_OK;
    REQ(H->inBatch == nullptr, "ldso_ba_destroy: the handle is part of a live batch (ldso_ba_batch_destroy first: the batch dereferences its handles)");
    hipSetDevice(H->device);
    hipDeviceSynchronize();
    for (void *p : H->allocs) hipFree(p);
    for (int i = 0; i < LD_MAXF; i++) if (H->imgOwned[i] && H->imgSlots[i]) hipFree(H->imgSlots[i]);
    if (H->d_color) hipFree(H->d_color);
    if (H->h_item) hipHostFree(H->h_item);
    if (H->d_item) hipFree(H->d_item);
    if (H->d_blocks) hipFree(H->d_blocks);
    if (H->h_stop) hipHostFree(H->h_stop);
    if (H->h_down) hipHostFree(H->h_down);
    if (H->h_stage) hipHostFree(H->h_stage);
    if (H->d_stage) hipFree(H->d_stage);
    if (H->d_act) hipFree(H->d_act);
    if (H->d_sel) hipFree(H->d_sel);
    if (H->distBuf) hipFree(H->distBuf);
    if (H->d_p2pErr) hipFree(H->d_p2pErr);
    for (auto &t : H->timers) { hipEventDestroy(t.a); hipEventDestroy(t.b); }
    for (ldso_ba::GnGraph &g : H->gnGraphs) { hipGraphExecDestroy(g.exec); hipGraphDestroy(g.graph); }
    if (H->ownStream && H->stream) hipStreamDestroy(H->stream);
    delete H;
    return LDSO_OK;
}

int ldso_ba_set_stream(ldso_ba_t *H, void *s) {
    REQ(H, "null handle");
    CHK(hipSetDevice(H->device));
    // work of this handle that is still in flight on the OLD stream is not ordered against the new one: wait for it here - in particular a staged copy out of the
    // pinned arena (stageBusy, ldso_ba_set_prior), whose later "wait for H->stream" would otherwise wait on the wrong stream
    if (H->stream && (H->ownStream || H->stageBusy)) { CHK(hipStreamSynchronize(H->stream)); H->stageBusy = false; }
    return swap_stream(H->stream, H->ownStream, s);
}

int ldso_ba_set_settings(ldso_ba_t *H, const ldso_settings_t *s) {
    REQ(H && s, "null argument");
    if (s->solverMode & (LDSO_SOLVER_SVD | LDSO_SOLVER_ORTHOGONALIZE_SYSTEM | LDSO_SOLVER_ORTHOGONALIZE_POINTMARG | LDSO_SOLVER_ORTHOGONALIZE_FULL |
                         LDSO_SOLVER_MOMENTUM | LDSO_SOLVER_STEPMOMENTUM)) {
        ldso_set_error("solverMode bits SVD/ORTHOGONALIZE_SYSTEM/_POINTMARG/_FULL/MOMENTUM/STEPMOMENTUM are not provided by the device path");
        return LDSO_E_UNSUPPORTED;
    }
    H->settings = *s;
    return LDSO_OK;
}

// a slot changed its buffer: the resident window keeps reading the slot, so its image pointers follow
static void rebind_slot(ldso_ba *H, int slot) {
    for (int f = 0; f < H->D.F && f < (int) H->imageSlot.size(); f++) if (H->imageSlot[f] == slot) H->B.img[f] = H->imgSlots[slot];
}

int ldso_ba_set_image(ldso_ba_t *H, int slot, const float *src) {
    REQ(H && src && slot >= 0 && slot < H->maxF, "ldso_ba_set_image: bad arguments");
    CHK(hipSetDevice(H->device));
    size_t bytes = (size_t) H->w * H->h * 3 * sizeof(float);
    if (!H->imgOwned[slot]) { void *p; CHK(hipMalloc(&p, bytes)); H->imgSlots[slot] = (float *) p; H->imgOwned[slot] = true; rebind_slot(H, slot); }
    CHK(hipMemcpyAsync(H->imgSlots[slot], src, bytes, hipMemcpyHostToDevice, H->stream));
    CHK(hipStreamSynchronize(H->stream));
    return LDSO_OK;
}

// level-0 image of a key frame from its raw irradiance: FrameHessian::makeImages level 0 (FrameHessian.cc:44-113) on the device
int ldso_ba_set_image_raw(ldso_ba_t *H, int slot, const float *irradiance) {
    REQ(H && irradiance && slot >= 0 && slot < H->maxF, "ldso_ba_set_image_raw: bad arguments");
    CHK(hipSetDevice(H->device));
    const size_t n = (size_t) H->w * H->h;
    if (!H->imgOwned[slot]) { void *q; CHK(hipMalloc(&q, n * 12)); H->imgSlots[slot] = (float *) q; H->imgOwned[slot] = true; rebind_slot(H, slot); }
    float *lv[1] = {H->imgSlots[slot]};
    RUN(raw_to_images(H->d_color, irradiance, H->w, H->h, 1, lv, H->stream));
    CHK(hipStreamSynchronize(H->stream));
    return LDSO_OK;
}

// debug / test fetch of a key-frame image slot (w*h*3 floats)
int ldso_ba_get_image(ldso_ba_t *H, int slot, float *out) {
    REQ(H && out && slot >= 0 && slot < H->maxF && H->imgSlots[slot], "ldso_ba_get_image: bad arguments");
    CHK(hipSetDevice(H->device));
    CHK(hipMemcpyAsync(out, H->imgSlots[slot], (size_t) H->w * H->h * 12, hipMemcpyDeviceToHost, H->stream));
    CHK(hipStreamSynchronize(H->stream));
    return LDSO_OK;
}

int ldso_ba_set_image_device(ldso_ba_t *H, int slot, const void *dev) {
    REQ(H && dev && slot >= 0 && slot < H->maxF, "ldso_ba_set_image_device: bad arguments");
    CHK(hipSetDevice(H->device));
    float *old = H->imgSlots[slot];
    if (H->imgOwned[slot] && old) {
        CHK(hipStreamSynchronize(H->stream));      // a kernel of the resident window may still be reading the slot
        hipFree(old); H->imgOwned[slot] = false;
    }
    H->imgSlots[slot] = (float *) dev;
    rebind_slot(H, slot);          // (no dangling B.img)
    return LDSO_OK;
}

// image slot from a resident ldso_pyramid_t (level 0 = FrameHessian::dI): zero-copy, ordered after the pyramid's build on this stream
int ldso_ba_set_image_pyramid(ldso_ba_t *H, int slot, ldso_pyramid_t *pyr) {
    REQ(H && pyr && slot >= 0 && slot < H->maxF, "ldso_ba_set_image_pyramid: bad arguments");
    RUN(pyramid_wait(pyr, H->device, H->w, H->h, 1, H->stream, "ldso_ba_set_image_pyramid", "the handle (device, size)"));
    return ldso_ba_set_image_device(H, slot, pyr->lv[0]);
}

int ldso_ba_get_dims(ldso_ba_t *H, int *F, int *P, int *R) {
    REQ(H, "ldso_ba_get_dims: null handle");
    if (F) *F = H->D.F;
    if (P) *P = H->D.P;
    if (R) *R = H->R;
    return LDSO_OK;
}

int ldso_ba_set_frames(ldso_ba_t *H, const ldso_frame_t *fr, const ldso_calib_t *calib) {
    REQ(H && fr && calib && H->D.F > 0, "ldso_ba_set_frames: set the window first");
    CHK(hipSetDevice(H->device));
    const int F = H->D.F;
    std::vector<DevFrame> df(F);
    DevCalib dc;
    fill_dev_frames(H, fr, calib, df.data(), &dc);
    CHK(hipMemcpyAsync(H->B.frames, df.data(), F * sizeof(DevFrame), hipMemcpyHostToDevice, H->stream));
    CHK(hipMemcpyAsync(H->B.calib, &dc, sizeof(dc), hipMemcpyHostToDevice, H->stream));
    CHK(hipStreamSynchronize(H->stream));
    // first precalc needs valid calib floats for the adjoint-independent parts; adjoints, then precalc
    return launch_solve(H, H->sets[H->cur], SK_ADJ | SK_PRECALC);
}

int ldso_ba_set_prior(ldso_ba_t *H, const double *HM, const double *bM) {
    REQ(H && H->D.n > 0, "ldso_ba_set_prior: set the window first");
    CHK(hipSetDevice(H->device));
    size_t n = H->D.n;
    H->hasPrior = (HM != nullptr) || (bM != nullptr);
    // through the pinned staging arena of ldso_ba_set_window (free: that call ends synchronised) when it is there - two copies from pageable memory + a wait
    // took 0.13 ms for 29 KB; no wait at the end: the arena is not reused before the next ldso_ba_set_window / set_point_stats, which synchronise first
    const size_t bytesH = n * n * 8, bytesB = n * 8;
    if (H->h_stage && H->stageCap >= bytesH + bytesB + 64) {
        if (H->stageBusy) { CHK(hipStreamSynchronize(H->stream)); H->stageBusy = false; }          // a previous ldso_ba_set_prior's copy
        if (HM) { memcpy(H->h_stage, HM, bytesH); CHK(hipMemcpyAsync(H->B.HM, H->h_stage, bytesH, hipMemcpyHostToDevice, H->stream)); } else CHK(hipMemsetAsync(H->B.HM, 0, bytesH, H->stream));
        if (bM) { memcpy(H->h_stage + bytesH, bM, bytesB); CHK(hipMemcpyAsync(H->B.bM, H->h_stage + bytesH, bytesB, hipMemcpyHostToDevice, H->stream)); } else CHK(hipMemsetAsync(H->B.bM, 0, bytesB, H->stream));
        H->stageBusy = true;
        return LDSO_OK;
    }
    if (HM) CHK(hipMemcpyAsync(H->B.HM, HM, bytesH, hipMemcpyHostToDevice, H->stream)); else CHK(hipMemsetAsync(H->B.HM, 0, bytesH, H->stream));
    if (bM) CHK(hipMemcpyAsync(H->B.bM, bM, bytesB, hipMemcpyHostToDevice, H->stream)); else CHK(hipMemsetAsync(H->B.bM, 0, bytesB, H->stream));
    CHK(hipStreamSynchronize(H->stream));
    return LDSO_OK;
}

int ldso_ba_get_prior(ldso_ba_t *H, double *HM, double *bM, int *has_prior) {
    REQ(H && H->D.P > 0 && H->D.n > 0, "ldso_ba_get_prior: set the window first");
    CHK(hipSetDevice(H->device));
    const size_t n = H->D.n;
    if (HM) CHK(hipMemcpyAsync(HM, H->B.HM, n * n * 8, hipMemcpyDeviceToHost, H->stream));
    if (bM) CHK(hipMemcpyAsync(bM, H->B.bM, n * 8, hipMemcpyDeviceToHost, H->stream));
    CHK(hipStreamSynchronize(H->stream));
    if (has_prior) *has_prior = H->hasPrior ? 1 : 0;
    return LDSO_OK;
}

int ldso_ba_profile(ldso_ba_t *H, int enable) {
    REQ(H, "null handle");
    H->profile = enable != 0;
    for (auto &t : H->timers) { hipEventDestroy(t.a); hipEventDestroy(t.b); }
    H->timers.clear();
    for (int i = 0; i < 5; i++) { H->tsum[i] = 0; H->tcnt[i] = 0; }
    return LDSO_OK;
}

int ldso_ba_kernel_time_ms(ldso_ba_t *H, int which, double *avg_ms, int *launches) {
    REQ(H && which >= 0 && which < 5, "bad arguments");
    CHK(hipStreamSynchronize(H->stream));
    for (auto &t : H->timers) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, t.a, t.b) == hipSuccess) { H->tsum[t.which] += ms; H->tcnt[t.which]++; }
        hipEventDestroy(t.a); hipEventDestroy(t.b);
    }
    H->timers.clear();
    if (avg_ms) *avg_ms = H->tcnt[which] ? H->tsum[which] / H->tcnt[which] : 0.0;
    if (launches) *launches = H->tcnt[which];
    return LDSO_OK;
}

int ldso_ba_sync(ldso_ba_t *H) {
    REQ(H, "null handle");
    CHK(hipStreamSynchronize(H->stream));
    return LDSO_OK;
}

// ---------------------------------------------------------------------------------------------------------
// fetchers
// ---------------------------------------------------------------------------------------------------------
#define D2H(vec, src, n) do { int r_ = d2h(H, (vec), (src), (n)); if (r_ != LDSO_OK) return r_; } while (0)
// The three result getters share their halves: enqueue the copies into the pinned download arena (fetch_*_put), ONE stream synchronisation, unpack (fetch_*_unpack).
// ldso_ba_get_results does all three behind a single synchronisation (the drop-in's write-back: two round trips of ~20 us fewer per optimize()).
struct FetchRes { const SlotRec *rn, *rc; };
struct FetchPts { const PtGeo *geo; const PtRec *pt; const PtAcc *acc; };
struct FetchFrm { const DevFrame *df; const DevCalib *dc; };
static size_t fetch_res_bytes(const ldso_ba *H) { return 2 * ((size_t) H->D.P * H->D.FS * sizeof(SlotRec) + 64); }
static size_t fetch_pts_bytes(const ldso_ba *H) { return (size_t) H->D.P * (sizeof(PtGeo) + sizeof(PtRec) + sizeof(PtAcc)) + 3 * 64; }
static size_t fetch_frm_bytes(const ldso_ba *H) { return (size_t) H->D.F * sizeof(DevFrame) + sizeof(DevCalib) + 2 * 64; }
static FetchRes fetch_res_put(ldso_ba *H, size_t &used, int &rc) {
    const size_t PS = (size_t) H->D.P * H->D.FS;
    // "new" values come from the set written by the last linearize, applied values from the current set
    const ResSet &Sn = H->pendingApply ? H->sets[H->cur ^ 1] : H->sets[H->cur];
    const ResSet &Sc = H->sets[H->cur];
    FetchRes f;
    f.rn = down_put(H, used, Sn.slot, PS, rc);
    f.rc = (&Sn != &Sc) ? down_put(H, used, Sc.slot, PS, rc) : f.rn;
    return f;
}
static void fetch_res_unpack(const ldso_ba *H, const FetchRes &f, ldso_res_out_t *out, int32_t *state_state, int32_t *is_active, int32_t *to_remove) {
    for (int i = 0; i < H->R; i++) {
        size_t s = H->flat2slot[i];
        const SlotRec &n_ = f.rn[s], &c_ = f.rc[s];
        if (out) {
            ldso_res_out_t &o = out[i];
            o.state_NewEnergy = n_.e[LD_SM_ENERGY].m.f; o.state_NewEnergyWithOutlier = n_.e[LD_SM_EWO].m.f; o.state_NewState = n_.e[LD_SM_STATE].m.i;
            for (int k = 0; k < 3; k++) o.centerProjectedTo[k] = n_.e[LD_SM_CEN0 + k].m.f;
            for (int k = 0; k < 8; k++) o.JpJdF[k] = n_.e[k].jp;
        }
        if (state_state) state_state[i] = c_.e[LD_SM_STATE].m.i;
        if (is_active) is_active[i] = c_.e[LD_SM_ACTIVE].m.i;
        if (to_remove) to_remove[i] = n_.e[LD_SM_REMOVE].m.i;
    }
}
static FetchPts fetch_pts_put(ldso_ba *H, size_t &used, int &rc) {
    const size_t P = H->D.P;
    const ResSet &S = H->sets[H->cur];
    FetchPts f;
    f.geo = down_put(H, used, H->B.pgeo, P, rc);
    f.pt = down_put(H, used, S.pt, P, rc);
    f.acc = down_put(H, used, S.acc, P, rc);
    return f;
}
static void fetch_pts_unpack(const ldso_ba *H, const FetchPts &f, ldso_point_out_t *out) {
    const PtGeo *geo = f.geo; const PtRec *pt = f.pt; const PtAcc *acc = f.acc;
    for (size_t i = 0; i < (size_t) H->D.P; i++) {
        ldso_point_out_t &o = out[i];
        o.step = geo[i].step; o.HdiF = geo[i].lastHdiF; o.bdSumF = geo[i].lastBdSumF; o.idepth_hessian = geo[i].lastIdH; o.Hdd_accAF = acc[i].HddA; o.bd_accAF = acc[i].bdA;
        o.Hdd_accLF = acc[i].HddL; o.bd_accLF = acc[i].bdL;
        for (int k = 0; k < 4; k++) { o.Hcd_accAF[k] = pt[i].HcdA[k]; o.Hcd_accLF[k] = pt[i].HcdL[k]; }
        o.idepth = geo[i].idepth; o.maxRelBaseline = pt[i].maxRelBS; o.numGoodResiduals = pt[i].numGood;
    }
}
static FetchFrm fetch_frm_put(ldso_ba *H, size_t &used, int &rc) {
    FetchFrm f;
    f.df = down_put(H, used, H->B.frames, (size_t) H->D.F, rc);
    f.dc = down_put(H, used, H->B.calib, (size_t) 1, rc);
    return f;
}
static void fetch_frm_unpack(const ldso_ba *H, const FetchFrm &f, ldso_frame_t *fr, double *step, double *cv, double *cs, double *pre) {
    const DevFrame *df = f.df;
    const DevCalib &dc = *f.dc;
    for (int q = 0; q < H->D.F; q++) {
        if (fr) {
            ldso_frame_t &o = fr[q];
            memcpy(o.worldToCam_evalPT, df[q].evalPT, sizeof(o.worldToCam_evalPT));
            memcpy(o.state, df[q].state, sizeof(o.state)); memcpy(o.state_zero, df[q].state_zero, sizeof(o.state_zero));
            memcpy(o.prior, df[q].prior, sizeof(o.prior));
            memcpy(o.nullspaces_pose, df[q].ns_pose, sizeof(o.nullspaces_pose)); memcpy(o.nullspaces_scale, df[q].ns_scale, sizeof(o.nullspaces_scale));
            memcpy(o.nullspaces_affine, df[q].ns_affine, sizeof(o.nullspaces_affine));
            o.ab_exposure = df[q].ab_exposure; o.frameEnergyTH = df[q].frameEnergyTH; o.frameID = df[q].frameID; o.pad_ = 0;
        }
        if (step) memcpy(step + q * 10, df[q].step, 10 * sizeof(double));
        if (pre) memcpy(pre + q * 12, df[q].PRE_w2c, 12 * sizeof(double));
    }
    if (cv) memcpy(cv, dc.value, 4 * sizeof(double));
    if (cs) memcpy(cs, dc.step, 4 * sizeof(double));
}

int ldso_ba_get_residuals(ldso_ba_t *H, ldso_res_out_t *out, int32_t *state_state, int32_t *is_active, int32_t *to_remove) {
    REQ(H && H->D.P > 0, "no window");
    CHK(hipSetDevice(H->device));
    RUN(down_reserve(H, fetch_res_bytes(H)));
    size_t used = 0; int rcD = LDSO_OK;
    const FetchRes f = fetch_res_put(H, used, rcD);
    if (rcD != LDSO_OK) return rcD;
    CHK(hipStreamSynchronize(H->stream));
    fetch_res_unpack(H, f, out, state_state, is_active, to_remove);
    return LDSO_OK;
}

int ldso_ba_get_points(ldso_ba_t *H, ldso_point_out_t *out) {
    REQ(H && out && H->D.P > 0, "bad arguments");
    CHK(hipSetDevice(H->device));
    RUN(down_reserve(H, fetch_pts_bytes(H)));
    size_t used = 0; int rcD = LDSO_OK;
    const FetchPts f = fetch_pts_put(H, used, rcD);
    if (rcD != LDSO_OK) return rcD;
    CHK(hipStreamSynchronize(H->stream));
    fetch_pts_unpack(H, f, out);
    return LDSO_OK;
}

int ldso_ba_get_frames(ldso_ba_t *H, ldso_frame_t *fr, double *step, double *cv, double *cs, double *pre) {
    REQ(H && H->D.F > 0, "no window");
    CHK(hipSetDevice(H->device));
    RUN(down_reserve(H, fetch_frm_bytes(H)));
    size_t used = 0; int rcD = LDSO_OK;
    const FetchFrm f = fetch_frm_put(H, used, rcD);
    if (rcD != LDSO_OK) return rcD;
    CHK(hipStreamSynchronize(H->stream));
    fetch_frm_unpack(H, f, fr, step, cv, cs, pre);
    return LDSO_OK;
}

int ldso_ba_get_results(ldso_ba_t *H, ldso_res_out_t *res, int32_t *state_state, int32_t *is_active, int32_t *to_remove, ldso_point_out_t *points,
                        ldso_frame_t *frames, double *step, double *calib_value, double *calib_step) {
    REQ(H && H->D.P > 0 && H->D.F > 0 && points, "ldso_ba_get_results: bad arguments");
    CHK(hipSetDevice(H->device));
    RUN(down_reserve(H, fetch_res_bytes(H) + fetch_pts_bytes(H) + fetch_frm_bytes(H)));
    size_t used = 0; int rcD = LDSO_OK;
    // the small blocks first: their unpacking could start while the residual records are still on their way (it does not: one synchronisation keeps the call simple)
    const FetchFrm ff = fetch_frm_put(H, used, rcD);
    const FetchPts fp = fetch_pts_put(H, used, rcD);
    const FetchRes fr_ = fetch_res_put(H, used, rcD);
    if (rcD != LDSO_OK) return rcD;
    CHK(hipStreamSynchronize(H->stream));
    fetch_frm_unpack(H, ff, frames, step, calib_value, calib_step, nullptr);
    fetch_pts_unpack(H, fp, points);
    fetch_res_unpack(H, fr_, res, state_state, is_active, to_remove);
    return LDSO_OK;
}

int ldso_ba_get_system(ldso_ba_t *H, double *HA, double *bA, double *HL, double *bL, double *Hsc, double *bsc, double *HF, double *bF, double *x) {
    REQ(H && H->D.n > 0, "no window");
    CHK(hipSetDevice(H->device));
    const size_t n = H->D.n, blk = n * n + n;
    std::vector<double> sys, xx;
    D2H(sys, H->B.sys, 4 * blk); D2H(xx, H->B.x, n);
    CHK(hipStreamSynchronize(H->stream));
    double *Hs[4] = {HA, HL, Hsc, HF}, *bs[4] = {bA, bL, bsc, bF};
    for (int m = 0; m < 4; m++) {
        if (Hs[m]) memcpy(Hs[m], sys.data() + m * blk, n * n * 8);
        if (bs[m]) memcpy(bs[m], sys.data() + m * blk + n * n, n * 8);
    }
    if (x) memcpy(x, xx.data(), n * 8);
    return LDSO_OK;
}

int ldso_ba_set_debug_split_launch(ldso_ba_t *H, int enable) {
    REQ(H, "null handle");
    H->noFusedLaunch = enable != 0;
    return LDSO_OK;
}

int ldso_ba_set_debug_dump(ldso_ba_t *H, int enable) {
    REQ(H, "null handle");
    H->B.dumpJ = enable ? H->d_dumpJ : nullptr;
    return LDSO_OK;
}

int ldso_ba_get_jacobians(ldso_ba_t *H, const int32_t *ids, int n, ldso_rawjac_t *out) {
    REQ(H && ids && out && n >= 0 && H->D.P > 0, "bad arguments");
    CHK(hipSetDevice(H->device));
    std::vector<ldso_rawjac_t> all;
    if (H->B.dumpJ == nullptr) {
        // recompute on demand: run the linearize kernel at the current state with the J dump enabled, into the
        // spare set; neither the applied set nor the frame-energy thresholds are touched.
        REQ(!H->pendingApply, "ldso_ba_get_jacobians: a linearisation is pending (call ldso_ba_apply_res first, or enable ldso_ba_set_debug_dump)");
        BaPtrs Bd = H->B;
        Bd.dumpJ = H->d_dumpJ;
        CHK(ba_launch_linearize(Bd, H->D, H->sets[H->cur], H->sets[H->cur ^ 1], H->settings, H->hasL, false, 0, GnInit{0, 0, 0.0f, -1}, H->stream));
    }
    D2H(all, H->d_dumpJ, (size_t) H->R);
    CHK(hipStreamSynchronize(H->stream));
    for (int i = 0; i < n; i++) { REQ(ids[i] >= 0 && ids[i] < H->R, "residual id out of range"); out[i] = all[ids[i]]; }
    return LDSO_OK;
}

int ldso_ba_get_precalc(ldso_ba_t *H, float *out) {
    REQ(H && out && H->D.F > 0, "bad arguments");
    CHK(hipSetDevice(H->device));
    const int F = H->D.F;
    std::vector<DevPair> dp;
    D2H(dp, H->B.pairs, (size_t) F * F);
    CHK(hipStreamSynchronize(H->stream));
    for (int i = 0; i < F * F; i++) {
        float *o = out + i * 27;
        memcpy(o, dp[i].KRKi, 36); memcpy(o + 9, dp[i].Kt, 12); memcpy(o + 12, dp[i].R0, 36); memcpy(o + 21, dp[i].t0, 12);
        o[24] = dp[i].aff[0]; o[25] = dp[i].aff[1]; o[26] = dp[i].b0;
    }
    return LDSO_OK;
}

// [h*F+t][14]: PRE_RTll 9, PRE_tTll 3 (current state), PRE_aff_mode 2 - what point activation reads (debug / test fetch)
int ldso_ba_get_pair_rt(ldso_ba_t *H, float *out) {
    REQ(H && out && H->D.F > 0, "bad arguments");
    CHK(hipSetDevice(H->device));
    const int F = H->D.F;
    std::vector<DevPair> dp;
    std::vector<float> rt;
    D2H(dp, H->B.pairs, (size_t) F * F);
    D2H(rt, H->B.pairRt, (size_t) F * F * 12);
    CHK(hipStreamSynchronize(H->stream));
    for (int i = 0; i < F * F; i++) { memcpy(out + i * 14, rt.data() + i * 12, 48); out[i * 14 + 12] = dp[i].aff[0]; out[i * 14 + 13] = dp[i].aff[1]; }
    return LDSO_OK;
}

int ldso_ba_get_counts(ldso_ba_t *H, int *a, int *l) {
    REQ(H, "null handle");
    double sc[16];
    RUN(read_scalars(H, sc));
    if (a) *a = (int) sc[9];
    if (l) *l = (int) sc[10];
    return LDSO_OK;
}

int ldso_ba_get_energy_log(ldso_ba_t *H, double *out, int cap) {
    REQ(H && out, "bad arguments");
    std::vector<double> e;
    D2H(e, H->B.energyLog, (size_t) 64);
    CHK(hipStreamSynchronize(H->stream));
    int n = H->lastIterations + 2;
    if (cap >= 64) { for (int i = 0; i < 64; i++) out[i] = e[i]; return n; }
    for (int i = 0; i < std::min(n, cap); i++) out[i] = e[i];
    return n;
}

// the share of `total` arrivers on every arrival word of k_reduce_solve, by the functions the kernel compiles (ba_dev.h) - host logic without a device
int ldso_ba_arrival_targets(int total, int *targets) {
    REQ(total >= 0 && targets, "ldso_ba_arrival_targets: bad arguments");
    for (int s = 0; s < LD_ARRIVE_SHARDS; s++) targets[s] = arrive_target(s, total);
    return LD_ARRIVE_SHARDS;
}
int ldso_ba_arrival_shard(int q) { return (q >= 0) ? arrive_shard(q) : LDSO_E_INVALID; }

int ldso_ba_get_arrival_words(ldso_ba_t *H, int *words) {
    REQ(H && words, "ldso_ba_get_arrival_words: bad arguments");
    std::vector<int> w;
    D2H(w, H->d_waitCtr, (size_t) LD_ARRIVE_SHARDS * LD_ARRIVE_STRIDE);
    double sc[16];
    RUN(read_scalars(H, sc));          // synchronises the stream
    for (int s = 0; s < LD_ARRIVE_SHARDS; s++) words[s] = w[(size_t) s * LD_ARRIVE_STRIDE];
    if (sc[4] != 0.0) return LDSO_E_NONFINITE;
    return LD_ARRIVE_SHARDS;
}

int ldso_ba_get_reduce_stamps(ldso_ba_t *H, double *out, int cap) {
    REQ(H && out && cap >= 0, "bad arguments");
    const int n = std::min(cap, 2 * H->maxF * H->maxF * LD_PAIRC);
    std::vector<double> e;
    D2H(e, H->B.pairC, (size_t) n);
    CHK(hipStreamSynchronize(H->stream));
    for (int i = 0; i < n; i++) out[i] = e[i];
    return n;
}

}  // extern "C"
