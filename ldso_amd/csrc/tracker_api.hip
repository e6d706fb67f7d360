// tracker_api.hip — the handle of the coarse tracker and the ldso_tr_* functions (include/ldso_hip.h): reference and new frame, the step-wise calcRes / calcGSSSE,
// the batched track and FullSystem::trackNewCoarse on top of it.  The kernels are tracker.hip and tracker_ref.hip, what the files share is tracker.h.
#include <mutex>
#include <cstdlib>
#include "tracker.h"
#include "lie_dev.h"

// the kernels read TrParams from device memory: upload it when the host copy changed (stream ordered; the callers synchronise the
// stream before they return, so the pinned staging buffer is free again)
static int tr_sync_params(ldso_tracker *H) {
    if (memcmp(&H->P, &H->Pdev, sizeof(TrParams)) == 0) return LDSO_OK;
    CHK(hipStreamSynchronize(H->stream));
    memcpy(H->h_P, &H->P, sizeof(TrParams));
    CHK(hipMemcpyAsync(H->d_P, H->h_P, sizeof(TrParams), hipMemcpyHostToDevice, H->stream));
    H->Pdev = H->P;
    return LDSO_OK;
}

// a pyramid on the host (Vec3f AoS per level) into the handle's own level buffers, enqueued on the handle's stream
static int tr_upload_levels(ldso_tracker *H, const float *const *src, float *const *dst, const char *who) {
    for (int l = 0; l < H->levels; l++) {
        REQ(src[l], std::string(who) + ": missing pyramid level");
        CHK(hipMemcpyAsync(dst[l], src[l], (size_t) H->P.lv[l].w * H->P.lv[l].h * 3 * sizeof(float), hipMemcpyHostToDevice, H->stream));
    }
    return LDSO_OK;
}

// Cooperative launches (G > 1) spin-wait across workgroups: forward progress needs every workgroup of the launch resident.  One launch
// alone is (nhyp * G <= #CUs, one 256-thread workgroup per CU whatever else runs: other kernels finish and free their CUs); two such
// launches from different handles could each hold CUs with spinning leaders while the other's helpers wait for a CU.  Within a process
// they are therefore chained per device through an event; across processes (or under a CU mask) the bounded spins of the kernel turn a
// would-be hang into LDSO_E_HIP.
static std::mutex g_coopMutex;
static hipEvent_t g_coopLast[64] = {nullptr};
int tr_coop_begin(int device, hipStream_t st, TrCoop *d_coop, int &coopSeq, std::unique_lock<std::mutex> &lk) {
    lk = std::unique_lock<std::mutex>(g_coopMutex);
    if (device >= 0 && device < 64) {
        hipEvent_t &e = g_coopLast[device];
        if (!e) CHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        else CHK(hipStreamWaitEvent(st, e, 0));
    }
    if (coopSeq > (1 << 30)) { CHK(hipMemsetAsync(d_coop, 0, TR_COOP_SLOTS * sizeof(TrCoop), st)); coopSeq = 1; }
    return LDSO_OK;
}
int tr_coop_end(int device, hipStream_t st, int &coopSeq) {
    coopSeq += 1024;           // more than the evaluations of one track (5 levels x (50 iterations + 7 cut-off repeats) + 1)
    if (device >= 0 && device < 64) CHK(hipEventRecord(g_coopLast[device], st));
    return LDSO_OK;
}

// FullSystem::trackNewCoarse (FullSystem.cc:179-386) around its tracks, in three pieces (ldso_tr_track_new_coarse runs them on one tracker, ldso_tr_group_track_new_coarse
// on every member of a group).  Before: the hypothesis list (:189-309), every try starts from the last frame's affine pair.
int tr_new_coarse_before(TrNewCoarse &S, int levels, const double sprelast[12], const double slast[12], const double lastF[12], int poses_valid, const float aff_last[2]) {
    S.T0.assign(83 * 12, 0.0); S.lr.assign(83 * 5, 0.0); S.flow.assign(83 * 3, 0.0); S.aff.assign(83 * 2, 0.f); S.ok.assign(83, 0);
    S.n = 0;
    RUN(ldso_tr_motion_hypotheses(sprelast, slast, lastF, poses_valid, S.T0.data(), &S.n));
    S.T = S.T0;
    for (int i = 0; i < S.n; i++) { S.aff[2 * i] = aff_last[0]; S.aff[2 * i + 1] = aff_last[1]; }
    S.coarsest = levels - 1;
    S.best = -1; S.used = 0; S.done = false;
    return LDSO_OK;
}
// Between: try 0 has run alone; the loop ends there when it is good enough (:355), else ALL remaining tries run (S.done stays false and S.n > 1)
int tr_new_coarse_between(TrNewCoarse &S, const double lastCoarseRMSE[5], double reTrackThreshold) {
    RUN(ldso_tr_select_hypothesis(1, S.coarsest, S.lr.data(), S.ok.data(), lastCoarseRMSE[0], reTrackThreshold, &S.best, &S.used, S.achieved));
    S.done = S.best == 0 && S.achieved[0] < lastCoarseRMSE[0] * reTrackThreshold;
    return LDSO_OK;
}
// After: with the remaining tries run (ranRest), the sequential accept / abort / early-exit decisions replayed on all of them; then the hand-over (:359-378)
int tr_new_coarse_after(TrNewCoarse &S, bool ranRest, const double lastF[12], const float aff_last[2], double lastCoarseRMSE[5], double reTrackThreshold,
                        double result4[4], double new_w2c[12], float aff_out[2], int *tries_consumed, int *good) {
    if (ranRest) RUN(ldso_tr_select_hypothesis(S.n, S.coarsest, S.lr.data(), S.ok.data(), lastCoarseRMSE[0], reTrackThreshold, &S.best, &S.used, S.achieved));
    double lastF_2_fh[12];
    if (S.best >= 0) {
        memcpy(lastF_2_fh, S.T.data() + 12 * S.best, 96);
        aff_out[0] = S.aff[2 * S.best]; aff_out[1] = S.aff[2 * S.best + 1];
        for (int i = 0; i < 3; i++) result4[1 + i] = S.flow[3 * S.best + i];
    } else {
        memcpy(lastF_2_fh, S.T0.data(), 96);
        aff_out[0] = aff_last[0]; aff_out[1] = aff_last[1];
        result4[1] = result4[2] = result4[3] = 0;
    }
    result4[0] = S.achieved[0];
    for (int l = 0; l < 5; l++) lastCoarseRMSE[l] = S.achieved[l];
    // camToWorld = lastF^-1 * lastF_2_fh^-1, the frame's pose is its inverse (:376-377) = lastF_2_fh * lastF
    ld::se3_mul(lastF_2_fh, lastF, new_w2c);
    if (tries_consumed) *tries_consumed = S.used;
    if (good) *good = S.best >= 0 ? 1 : 0;
    return LDSO_OK;
}

extern "C" {

static int tr_create_body(ldso_tracker *H, int device, int w, int h, int levels) {
    H->device = device; H->w = w; H->h = h; H->levels = levels;
    ldso_settings_default(&H->settings);
    CHK(hipStreamCreateWithFlags(&H->stream, hipStreamNonBlocking));
    H->ownStream = true;
    memset(&H->P, 0, sizeof(H->P));
    H->P.levels = levels;
    for (int l = 0; l < levels; l++) {
        TrLevel &L = H->P.lv[l];
        L.w = w >> l; L.h = h >> l; L.n = 0;
        size_t n = (size_t) L.w * L.h;
        DALLOC(H->allocs, H->d_newImg[l], n * 3); DALLOC(H->allocs, H->d_refImg[l], n * 3);
        L.newImg = H->d_newImg[l]; L.refImg = H->d_refImg[l];
        DALLOC(H->allocs, L.pc_u, n); DALLOC(H->allocs, L.pc_v, n); DALLOC(H->allocs, L.pc_idepth, n); DALLOC(H->allocs, L.pc_color, n);
        // 64 floats of zeroed padding on both sides: the reference's dilation reads one element before / after
        // the image (CoarseTracker.cc:331-345, index i-1-w at i==w) out of its over-allocated buffers
        DALLOC(H->allocs, L.idepth, n + 128); DALLOC(H->allocs, L.wsum, n + 128); DALLOC(H->allocs, L.wsum_bak, n + 128);
        L.idepth += 64; L.wsum += 64; L.wsum_bak += 64;
        DALLOC(H->allocs, L.blockCnt, n / 256 + 2);
    }
    DALLOC(H->allocs, H->d_total, TR_MAXL); DALLOC(H->allocs, H->d_T, 12); DALLOC(H->allocs, H->d_acc, TR_NACC); DALLOC(H->allocs, H->d_hyp, 128); DALLOC(H->allocs, H->d_coop, TR_COOP_SLOTS); DALLOC(H->allocs, H->d_P, 1);
    CHK(hipHostMalloc((void **) &H->h_P, sizeof(TrParams)));
    CHK(hipHostMalloc((void **) &H->h_hyp, 128 * sizeof(TrHyp)));
    memset(&H->Pdev, 0xFF, sizeof(TrParams));
    { hipDeviceProp_t pr; if (hipGetDeviceProperties(&pr, device) == hipSuccess && pr.multiProcessorCount > 0) H->numCU = pr.multiProcessorCount; }
    return LDSO_OK;
}

int ldso_tr_create(int device, int w, int h, int levels, ldso_tracker_t **out) {
    REQ(out && w > 16 && h > 16 && levels >= 1 && levels <= TR_MAXL && (w >> (levels - 1)) >= 8, "ldso_tr_create: bad arguments");
    RUN(open_device(device, "ldso_tr_create"));
    ldso_tracker *H = new ldso_tracker();
    return finish_create(tr_create_body(H, device, w, h, levels), H, out, ldso_tr_destroy);      // nothing of a half-built handle leaks
}

int ldso_tr_destroy(ldso_tracker_t *H) {
    if (!H) return LDSO_OK;
    REQ(H->inGroup == nullptr, "ldso_tr_destroy: the tracker is a member of a live group (ldso_tr_group_destroy first: the group dereferences its members)");
    hipSetDevice(H->device);
    hipDeviceSynchronize();
    for (void *p : H->allocs) hipFree(p);
    if (H->d_pts) hipFree(H->d_pts);
    if (H->d_next) hipFree(H->d_next);
    if (H->d_color) hipFree(H->d_color);
    if (H->h_P) hipHostFree(H->h_P);
    if (H->h_hyp) hipHostFree(H->h_hyp);
    if (H->ownStream && H->stream) hipStreamDestroy(H->stream);
    delete H;
    return LDSO_OK;
}

int ldso_tr_set_stream(ldso_tracker_t *H, void *s) {
    REQ(H, "null handle");
    return swap_stream(H->stream, H->ownStream, s);
}

int ldso_tr_set_settings(ldso_tracker_t *H, const ldso_settings_t *s) {
    REQ(H && s, "null argument");
    H->settings = *s;
    H->P.huberTH = s->huberTH; H->P.coarseCutoffTH = s->coarseCutoffTH; H->P.affineOptModeA = s->affineOptModeA; H->P.affineOptModeB = s->affineOptModeB;
    return LDSO_OK;
}

// CoarseTracker::makeK, float arithmetic as the reference (CoarseTracker.cc:219-246)
int ldso_tr_make_k(ldso_tracker_t *H, const ldso_calib_t *calib) {
    REQ(H && calib, "null argument");
    ldso_tr_set_settings(H, &H->settings);
    float fx[TR_MAXL], fy[TR_MAXL], cx[TR_MAXL], cy[TR_MAXL];
    fx[0] = (float) (50.0 * calib->value[0]); fy[0] = (float) (50.0 * calib->value[1]); cx[0] = (float) (50.0 * calib->value[2]); cy[0] = (float) (50.0 * calib->value[3]);
    for (int l = 1; l < H->levels; l++) {
        fx[l] = (float) (fx[l - 1] * 0.5); fy[l] = (float) (fy[l - 1] * 0.5);
        cx[l] = (float) ((cx[0] + 0.5) / ((int) 1 << l) - 0.5); cy[l] = (float) ((cy[0] + 0.5) / ((int) 1 << l) - 0.5);
    }
    for (int l = 0; l < H->levels; l++) {
        TrLevel &L = H->P.lv[l];
        L.fx = fx[l]; L.fy = fy[l]; L.cx = cx[l]; L.cy = cy[l];
        float K[9] = {fx[l], 0, cx[l], 0, fy[l], cy[l], 0, 0, 1};
        auto cof = [&](int a, int b) { int a1 = (a + 1) % 3, a2 = (a + 2) % 3, b1 = (b + 1) % 3, b2 = (b + 2) % 3; return K[a1 * 3 + b1] * K[a2 * 3 + b2] - K[a1 * 3 + b2] * K[a2 * 3 + b1]; };
        float k0 = cof(0, 0), k1 = cof(1, 0), k2 = cof(2, 0);
        float det = (k0 * K[0] + k1 * K[3]) + k2 * K[6];
        float invdet = 1.0f / det;
        L.Ki[0] = k0 * invdet; L.Ki[1] = k1 * invdet; L.Ki[2] = k2 * invdet;
        L.Ki[3] = cof(0, 1) * invdet; L.Ki[4] = cof(1, 1) * invdet; L.Ki[5] = cof(2, 1) * invdet;
        L.Ki[6] = cof(0, 2) * invdet; L.Ki[7] = cof(1, 2) * invdet; L.Ki[8] = cof(2, 2) * invdet;
    }
    return LDSO_OK;
}

int ldso_tr_set_ref(ldso_tracker_t *H, const float *const *ref_dIp, float ref_a, float ref_b, float ref_exposure, const float *pts, int n) {
    REQ(H && ref_dIp && (pts || n == 0) && n >= 0, "ldso_tr_set_ref: bad arguments");
    CHK(hipSetDevice(H->device));
    RUN(tr_upload_levels(H, ref_dIp, H->d_refImg, "ldso_tr_set_ref"));
    for (int l = 0; l < H->levels; l++) H->P.lv[l].refImg = H->d_refImg[l];
    return tr_set_ref_common(H, ref_a, ref_b, ref_exposure, pts, n);
}

// the reference keyframe's pyramid already resident (ldso_pyramid_t, zero-copy: the tracker reads the pyramid's levels until the next
// ldso_tr_set_ref*; the caller keeps the pyramid alive that long)
int ldso_tr_set_ref_pyramid(ldso_tracker_t *H, ldso_pyramid_t *pyr, float ref_a, float ref_b, float ref_exposure, const float *pts, int n) {
    REQ(H && pyr && (pts || n == 0) && n >= 0, "ldso_tr_set_ref_pyramid: bad arguments");
    RUN(pyramid_wait(pyr, H->device, H->w, H->h, H->levels, H->stream, "ldso_tr_set_ref_pyramid", "the tracker (device, size, levels)"));
    for (int l = 0; l < H->levels; l++) H->P.lv[l].refImg = pyr->lv[l];
    return tr_set_ref_common(H, ref_a, ref_b, ref_exposure, pts, n);
}

int ldso_tr_set_new_frame(ldso_tracker_t *H, const float *const *new_dIp, float exposure) {
    REQ(H && new_dIp, "ldso_tr_set_new_frame: bad arguments");
    CHK(hipSetDevice(H->device));
    RUN(tr_upload_levels(H, new_dIp, H->d_newImg, "ldso_tr_set_new_frame"));
    for (int l = 0; l < H->levels; l++) H->P.lv[l].newImg = H->d_newImg[l];
    H->P.new_exposure = exposure;
    CHK(hipStreamSynchronize(H->stream));
    return LDSO_OK;
}

// CoarseTracker's new frame from the raw level-0 irradiance: FrameHessian::makeImages runs on the device (images.hip), one
// w*h float upload instead of the 12-byte AoS pyramid
int ldso_tr_set_new_frame_image(ldso_tracker_t *H, const float *irradiance, float exposure) {
    REQ(H && irradiance, "ldso_tr_set_new_frame_image: bad arguments");
    CHK(hipSetDevice(H->device));
    RUN(raw_to_images(H->d_color, irradiance, H->w, H->h, H->levels, H->d_newImg, H->stream));
    for (int l = 0; l < H->levels; l++) H->P.lv[l].newImg = H->d_newImg[l];
    H->P.new_exposure = exposure;
    CHK(hipStreamSynchronize(H->stream));
    return LDSO_OK;
}

// the frame to be tracked as a resident ldso_pyramid_t (zero-copy; stream-ordered after the pyramid's build, no host synchronisation)
int ldso_tr_set_new_frame_pyramid(ldso_tracker_t *H, ldso_pyramid_t *pyr, float exposure) {
    REQ(H && pyr, "ldso_tr_set_new_frame_pyramid: bad arguments");
    RUN(pyramid_wait(pyr, H->device, H->w, H->h, H->levels, H->stream, "ldso_tr_set_new_frame_pyramid", "the tracker (device, size, levels)"));
    for (int l = 0; l < H->levels; l++) H->P.lv[l].newImg = pyr->lv[l];
    H->P.new_exposure = exposure;
    return LDSO_OK;
}

// debug / test fetch of a level of the new frame's pyramid ((w>>lvl)*(h>>lvl)*3 floats)
int ldso_tr_get_new_frame_level(ldso_tracker_t *H, int lvl, float *out) {
    REQ(H && out && lvl >= 0 && lvl < H->levels, "ldso_tr_get_new_frame_level: bad arguments");
    CHK(hipSetDevice(H->device));
    CHK(hipMemcpyAsync(out, H->P.lv[lvl].newImg, (size_t) H->P.lv[lvl].w * H->P.lv[lvl].h * 3 * sizeof(float), hipMemcpyDeviceToHost, H->stream));
    CHK(hipStreamSynchronize(H->stream));
    return LDSO_OK;
}

static int tr_calc(ldso_tracker *H, int lvl, const double *T, float a, float b, float cutoff) {
    CHK(hipMemcpyAsync(H->d_T, T, 12 * 8, hipMemcpyHostToDevice, H->stream));
    RUN(tr_sync_params(H));
    CHK(tr_launch_calc(H->d_P, lvl, H->d_T, a, b, cutoff, H->d_acc, H->stream));
    CHK(hipMemcpyAsync(H->lastAcc, H->d_acc, TR_NACC * 8, hipMemcpyDeviceToHost, H->stream));
    CHK(hipStreamSynchronize(H->stream));
    H->haveAcc = true;
    return LDSO_OK;
}

int ldso_tr_calc_res(ldso_tracker_t *H, int lvl, const double T[12], float a, float b, float cutoffTH, double rs[6], int *n_warped) {
    REQ(H && T && rs && lvl >= 0 && lvl < H->levels, "ldso_tr_calc_res: bad arguments");
    CHK(hipSetDevice(H->device));
    int r = tr_calc(H, lvl, T, a, b, cutoffTH);
    if (r != LDSO_OK) return r;
    const double *acc = H->lastAcc;
    rs[0] = (double) (float) acc[0]; rs[1] = (double) (int) acc[1];
    rs[2] = (double) ((float) acc[2] / ((float) acc[4] + 0.1f)); rs[3] = 0; rs[4] = (double) ((float) acc[3] / ((float) acc[4] + 0.1f));
    rs[5] = (double) ((float) (int) acc[5] / (float) (int) acc[1]);
    if (n_warped) *n_warped = ((int) acc[6] + 3) / 4 * 4;
    return LDSO_OK;
}

int ldso_tr_calc_gs(ldso_tracker_t *H, int lvl, const double T[12], float a, float b, double Hout[64], double bout[8]) {
    REQ(H && T && Hout && bout && lvl >= 0 && lvl < H->levels, "ldso_tr_calc_gs: bad arguments");
    REQ(H->haveAcc, "ldso_tr_calc_gs: call ldso_tr_calc_res first (the reference reuses the warped buffers of the last calcRes)");
    const double *acc = H->lastAcc;
    int nw = (int) acc[6];
    int npad = (nw + 3) / 4 * 4;
    double inv = (double) (1.0f / (float) npad);
    const double cs[8] = {1.0, 1.0, 1.0, 0.5, 0.5, 0.5, 10.0, 1000.0};
    double M[81];
    int q = 7;
    for (int r = 0; r < 9; r++) for (int c = r; c < 9; c++) { double v = (double) (float) acc[q++]; M[r * 9 + c] = v; M[c * 9 + r] = v; }
    for (int r = 0; r < 8; r++) { for (int c = 0; c < 8; c++) Hout[r * 8 + c] = M[r * 9 + c] * inv * cs[r] * cs[c]; bout[r] = M[r * 9 + 8] * inv * cs[r]; }
    return LDSO_OK;
}

int ldso_tr_track_batch(ldso_tracker_t *H, int nhyp, double *T_inout /*nhyp*12*/, float *aff_inout /*nhyp*2*/, int coarsestLvl, const double minRes[5],
                        double *lastResiduals /*nhyp*5*/, double *flow /*nhyp*3*/, int *ok /*nhyp*/, int *iterations /*nhyp*/) {
    REQ(H && nhyp >= 1 && nhyp <= 128 && T_inout && aff_inout && coarsestLvl >= 0 && coarsestLvl < 5 && coarsestLvl < H->levels, "ldso_tr_track: bad arguments");
    CHK(hipSetDevice(H->device));
    TrHyp *hy = H->h_hyp;             // the stream is synchronised before this function returns: the buffer is free again
    for (int i = 0; i < nhyp; i++) {
        memset(&hy[i], 0, sizeof(TrHyp));
        memcpy(hy[i].T, T_inout + i * 12, 96);
        hy[i].a = aff_inout[2 * i]; hy[i].b = aff_inout[2 * i + 1]; hy[i].coarsestLvl = coarsestLvl;
        for (int k = 0; k < 5; k++) hy[i].minRes[k] = minRes ? minRes[k] : NAN;
    }
    CHK(hipMemcpyAsync(H->d_hyp, hy, nhyp * sizeof(TrHyp), hipMemcpyHostToDevice, H->stream));
    // few hypotheses: TR_GMAX workgroups share each of them on the large levels (all workgroups resident: nhyp * G <= CUs);
    // many hypotheses fill the chip by themselves
    RUN(tr_sync_params(H));
    const int G = tr_coop_width(nhyp, H->numCU);
    if (G > 1) {
        std::unique_lock<std::mutex> lk;
        RUN(tr_coop_begin(H->device, H->stream, H->d_coop, H->coopSeq, lk));
        CHK(tr_launch_track(G, nhyp, H->d_P, H->d_hyp, H->d_coop, H->coopSeq, H->stream));
        RUN(tr_coop_end(H->device, H->stream, H->coopSeq));
    } else {
        CHK(tr_launch_track(1, nhyp, H->d_P, H->d_hyp, nullptr, 0, H->stream));
    }
    CHK(hipMemcpyAsync(hy, H->d_hyp, nhyp * sizeof(TrHyp), hipMemcpyDeviceToHost, H->stream));
    CHK(hipStreamSynchronize(H->stream));
    for (int i = 0; i < nhyp; i++) if (hy[i].ok == -2) {
        ldso_set_error("ldso_tr_track: the cooperating workgroups of a hypothesis did not become co-resident (device shared with another process or CU-masked?); set LDSO_TR_NO_COOP=1");
        return LDSO_E_HIP;
    }
    for (int i = 0; i < nhyp; i++) {
        memcpy(T_inout + i * 12, hy[i].T, 96);
        aff_inout[2 * i] = hy[i].a; aff_inout[2 * i + 1] = hy[i].b;
        if (lastResiduals) memcpy(lastResiduals + i * 5, hy[i].lastResiduals, 40);
        if (flow) memcpy(flow + i * 3, hy[i].flow, 24);
        if (ok) ok[i] = hy[i].ok;
        if (iterations) iterations[i] = hy[i].iterations;
        if (i == 0) { memcpy(H->lastEvals, hy[i].evals, sizeof(H->lastEvals)); H->lastPivotedSolves = 0; }
        H->lastPivotedSolves += hy[i].pivotedSolves;
#if LD_STAMP_ON_TR
        if (i == 0) { long long ph[5][8]; tr_fetch_phase_stamps(ph);
            for (int l = 0; l < 5; l++) if (ph[l][7]) fprintf(stderr, "[tr phases] lvl %d: setup %.2f pass %.2f dpp %.2f barrier %.2f sum %.2f us per eval (%d evals)\n", l, ph[l][0] / 100.0 / ph[l][7], ph[l][1] / 100.0 / ph[l][7], ph[l][2] / 100.0 / ph[l][7], ph[l][3] / 100.0 / ph[l][7], ph[l][4] / 100.0 / ph[l][7], (int) ph[l][7]); }
#endif
        if (LD_STAMP_ON_TR && i == 0) fprintf(stderr, "[tr stamps] evals %d: %.1f us in tr_eval of %.1f us kernel; per-eval us by level 0..4: %.1f %.1f %.1f %.1f %.1f; solve %.1f step %.1f post %.1f us\n", (int) hy[i].dbg[2], hy[i].dbg[0] / 100.0, hy[i].dbg[1] / 100.0, hy[i].dbg[3] / 100, hy[i].dbg[4] / 100, hy[i].dbg[5] / 100, hy[i].dbg[6] / 100, hy[i].dbg[7] / 100, hy[i].dbg[8] / 100, hy[i].dbg[9] / 100, hy[i].dbg[10] / 100);
    }
    return LDSO_OK;
}

// Vec4 FullSystem::trackNewCoarse (FullSystem.cc:179-386) on a tracker whose reference and new frame are set.  The reference runs its tries
// one after the other and stops at the first one that is good enough (:355) - almost always the first.  Here: try 0 alone (cooperative
// single-hypothesis launch); only if the loop would go on, ALL remaining tries in one batched launch, and ldso_tr_select_hypothesis replays
// the sequential accept / abort / early-exit decisions on the residuals (a try the sequential loop would have aborted on a coarse level
// counts as aborted).  lastCoarseRMSE: in / out (FullSystem::lastCoarseRMSE); result4 = (achievedRes[0], flow[0..2]); new_w2c = the pose
// handed to the new frame (:376-377), aff_out its aff_g2l; good = 0 is the reference's "tracking failed entirely" branch (:359-365).
int ldso_tr_track_new_coarse(ldso_tracker_t *H, const double sprelast[12], const double slast[12], const double lastF[12], int poses_valid, const float aff_last[2],
                             double lastCoarseRMSE[5], double reTrackThreshold, double result4[4], double new_w2c[12], float aff_out[2], int *tries_consumed, int *good) {
    REQ(H && aff_last && lastCoarseRMSE && result4 && new_w2c && aff_out, "ldso_tr_track_new_coarse: null argument");
    TrNewCoarse S;
    RUN(tr_new_coarse_before(S, H->levels, sprelast, slast, lastF, poses_valid, aff_last));
    RUN(ldso_tr_track_batch(H, 1, S.T.data(), S.aff.data(), S.coarsest, nullptr, S.lr.data(), S.flow.data(), S.ok.data(), nullptr));
    RUN(tr_new_coarse_between(S, lastCoarseRMSE, reTrackThreshold));
    const bool rest = !S.done && S.n > 1;
    if (rest) RUN(ldso_tr_track_batch(H, S.n - 1, S.T.data() + 12, S.aff.data() + 2, S.coarsest, nullptr, S.lr.data() + 5, S.flow.data() + 3, S.ok.data() + 1, nullptr));
    return tr_new_coarse_after(S, rest, lastF, aff_last, lastCoarseRMSE, reTrackThreshold, result4, new_w2c, aff_out, tries_consumed, good);
}

// calcRes evaluations per level of the last ldso_tr_track / hypothesis 0 of the last batch, and the reference point counts pc_n:
// the algorithmic bytes of that track are sum_l evals[l] * pc_n[l] * 64 (16 B point + 48 B taps per evaluation)
int ldso_tr_last_track_evals(ldso_tracker_t *H, int evals[5], int pc_n[5]) {
    REQ(H && evals && pc_n, "null argument");
    for (int l = 0; l < 5; l++) { evals[l] = H->lastEvals[l]; pc_n[l] = (l < H->levels) ? H->P.lv[l].n : 0; }
    return LDSO_OK;
}

// LM solves of the last ldso_tr_track / ldso_tr_track_batch call whose 8 x 8 system was rank-deficient to float precision (a pivot below 1e-6 of the diagonal entry it started from) and went
// through the reference's pivoted LDL^T instead of the unpivoted register version (0 on any normal track)
int ldso_tr_last_track_pivoted_solves(ldso_tracker_t *H, int *n) {
    REQ(H && n, "null argument");
    *n = H->lastPivotedSolves;
    return LDSO_OK;
}

int ldso_tr_debug_solve8(const double H[64], const double b[8], double diag_scale, double x[8], int *pivoted) {
    REQ(H && b && x && pivoted, "ldso_tr_debug_solve8: null argument");
    double *d = nullptr;
    CHK(hipMalloc((void **) &d, (64 + 8 + 8 + 1) * sizeof(double)));
    CHK(hipMemcpy(d, H, 64 * sizeof(double), hipMemcpyHostToDevice));
    CHK(hipMemcpy(d + 64, b, 8 * sizeof(double), hipMemcpyHostToDevice));
    CHK(tr_launch_solve8(d, d + 64, diag_scale, d + 72, (int *) (d + 80)));
    CHK(hipMemcpy(x, d + 72, 8 * sizeof(double), hipMemcpyDeviceToHost));
    CHK(hipMemcpy(pivoted, d + 80, sizeof(int), hipMemcpyDeviceToHost));
    CHK(hipFree(d));
    return LDSO_OK;
}

int ldso_tr_track(ldso_tracker_t *H, double T[12], float aff[2], int coarsestLvl, const double minRes[5], double lastResiduals[5], double flow[3], int *ok, int *iterations) {
    return ldso_tr_track_batch(H, 1, T, aff, coarsestLvl, minRes, lastResiduals, flow, ok, iterations);
}

// the launch-shape rule of a track by itself (tracker.h: tr_coop_width): pure host function
int ldso_tr_coop_width(int count, int num_cu, int *G) {
    REQ(G && count >= 1 && num_cu >= 1, "ldso_tr_coop_width: bad arguments");
    *G = tr_coop_width(count, num_cu);
    return LDSO_OK;
}

int ldso_tr_get_pc(ldso_tracker_t *H, int lvl, float *u, float *v, float *idepth, float *color, int *n) {
    REQ(H && lvl >= 0 && lvl < H->levels, "ldso_tr_get_pc: bad arguments");
    CHK(hipSetDevice(H->device));
    const TrLevel &L = H->P.lv[lvl];
    if (n) *n = L.n;
    size_t bytes = (size_t) L.n * 4;
    if (u) CHK(hipMemcpyAsync(u, L.pc_u, bytes, hipMemcpyDeviceToHost, H->stream));
    if (v) CHK(hipMemcpyAsync(v, L.pc_v, bytes, hipMemcpyDeviceToHost, H->stream));
    if (idepth) CHK(hipMemcpyAsync(idepth, L.pc_idepth, bytes, hipMemcpyDeviceToHost, H->stream));
    if (color) CHK(hipMemcpyAsync(color, L.pc_color, bytes, hipMemcpyDeviceToHost, H->stream));
    CHK(hipStreamSynchronize(H->stream));
    return LDSO_OK;
}

}  // extern "C"
