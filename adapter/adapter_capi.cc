// adapter_capi.cc — C entry points for tests/test_adapter_gpu.py: run the compiled drop-in adapter (ldso_gpu_adapter.cc) on reference object
// graphs that oracle/ref_driver.cc builds (libldso_ref.so: the reference's own translation units).  Test plumbing, not part of the adapter.
#include <cstdio>
#include <exception>
#include <memory>
#include <vector>
#include <cmath>
// test plumbing reaches into FullSystem's private members exactly as the adapter's units do: through the same private header (see ldso_gpu_adapter.h)
#include "adapter_internal.h"

using namespace ldso;
using namespace ldso::internal;

static thread_local char g_err[512];
#define GUARD(...) try { __VA_ARGS__; return 0; } catch (const std::exception &e) { std::snprintf(g_err, sizeof(g_err), "%s", e.what()); return -1; }

extern "C" {

const char *adp_last_error() { return g_err; }
void *adp_create(int device, int maxFrames, int maxPoints) {
    try { return new GpuBackend(device, maxFrames, maxPoints); } catch (const std::exception &e) { std::snprintf(g_err, sizeof(g_err), "%s", e.what()); return nullptr; }
}
void adp_destroy(void *b) { delete (GpuBackend *) b; }
// fs = ref_fs_handle(window) of libldso_ref.so
int adp_optimize(void *b, void *fs, int iterations, float *rmse, int *executed, int *lost) {
    GUARD(*rmse = ((GpuBackend *) b)->optimize(*(FullSystem *) fs, iterations); *executed = ((GpuBackend *) b)->lastIterations; *lost = ((FullSystem *) fs)->isLost ? 1 : 0)
}
// fs = ref_tr_prepare(tracker ...), tracker = ref_tr_coarse_tracker, fhs = ref_tr_frame_hessians, newfh = ref_tr_new_frame_hessian, calib = ref_tr_calib_hessian
int adp_track_new_coarse(void *b, void *fs_, void *tracker, void *fhs, void *newfh, void *calib, double *result4) {
    GUARD(
        GpuBackend &B = *(GpuBackend *) b; FullSystem &fs = *(FullSystem *) fs_; CoarseTracker &tr = *(CoarseTracker *) tracker;
        B.makeK(tr, *(std::shared_ptr<CalibHessian> *) calib);
        B.setCoarseTrackingRef(tr, *(std::vector<std::shared_ptr<FrameHessian>> *) fhs);
        Vec4 r = B.trackNewCoarse(fs, *(std::shared_ptr<FrameHessian> *) newfh);
        for (int i = 0; i < 4; i++) result4[i] = r[i])
}
// one CoarseTracker::trackNewestCoarse through the adapter (T row-major [R|t] in / out)
int adp_track_newest_coarse(void *b, void *tracker, void *fhs, void *newfh, void *calib, double *T, float *ab, int coarsestLvl, const double *minRes, double *lastResiduals, int *ok) {
    GUARD(
        GpuBackend &B = *(GpuBackend *) b; CoarseTracker &tr = *(CoarseTracker *) tracker;
        B.makeK(tr, *(std::shared_ptr<CalibHessian> *) calib);
        B.setCoarseTrackingRef(tr, *(std::vector<std::shared_ptr<FrameHessian>> *) fhs);
        Mat33 R; Vec3 t;
        for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) R(i, j) = T[i * 4 + j]; t[i] = T[i * 4 + 3]; }
        SE3 pose(R, t); AffLight aff(ab[0], ab[1]); Vec5 mr;
        for (int i = 0; i < 5; i++) mr[i] = minRes[i];
        *ok = B.trackNewestCoarse(tr, *(std::shared_ptr<FrameHessian> *) newfh, pose, aff, coarsestLvl, mr) ? 1 : 0;
        Eigen::Matrix<double, 3, 4> M = pose.matrix3x4();
        for (int i = 0; i < 3; i++) for (int j = 0; j < 4; j++) T[i * 4 + j] = M(i, j);
        ab[0] = aff.a; ab[1] = aff.b;
        for (int i = 0; i < 5; i++) lastResiduals[i] = tr.lastResiduals[i])
}

// toOptimize = ref_fs_build_immature(window, ...) of libldso_ref.so.  out: per candidate the verdict, the new point's inverse depth, and per
// window frame 0 where the new point got a PointFrameResidual (state IN) / -1 elsewhere; last[k][0..1] = state of lastResiduals[0..1] (-1: no residual)
int adp_activate_points(void *b, void *fs_, void *toOptimize, int n, int F, int *ok, float *idepth, int *res_target /*n*F*/, int *last /*n*2*/) {
    GUARD(
        auto &cand = *(std::vector<std::shared_ptr<ImmaturePoint>> *) toOptimize;
        std::vector<std::shared_ptr<PointHessian>> made;
        ((GpuBackend *) b)->activatePoints(*(FullSystem *) fs_, cand, made);
        for (int i = 0; i < n; i++) {
            ok[i] = made[i] ? 1 : 0; idepth[i] = made[i] ? made[i]->idepth : NAN;
            for (int t = 0; t < F; t++) res_target[i * F + t] = -1;
            last[2 * i] = last[2 * i + 1] = -1;
            if (!made[i]) continue;
            for (auto &r : made[i]->residuals) res_target[i * F + r->target.lock()->idx] = (int) r->state_state;
            for (int j = 0; j < 2; j++) last[2 * i + j] = made[i]->lastResiduals[j].first ? (int) made[i]->lastResiduals[j].second : -1;
        })
}

// fh = ref_fs_new_frame(window, ...): GpuBackend::traceNewCoarse in place of FullSystem::traceNewCoarse; counts = its six trace_* counters
int adp_trace_new_coarse(void *b, void *fs, void *fh, int *counts) {
    GUARD(((GpuBackend *) b)->traceNewCoarse(*(FullSystem *) fs, *(std::shared_ptr<FrameHessian> *) fh); for (int i = 0; i < 6; i++) counts[i] = ((GpuBackend *) b)->lastTraceCounts[i])
}

// fh = ref_fs_new_frame(window, ...): GpuBackend::makeNewTraces in place of FullSystem::makeNewTraces with setting_pointSelection = 1 and
// setting_desiredImmatureDensity = n_desired; response = CalibHessian::B to use (256 floats) or null (the window's own, identity by default).
// Returns what the frame's features hold afterwards, at most cap of them: feat [cap][5] = u, v, score, isCorner, angle; desc [cap][32]; imm [cap] = the
// ImmaturePoint of each (host = index of its frame in the window, -1 when it is not a window frame); counts[4] = features detected, corners, dropped, frame->features.size()
int adp_make_new_traces(void *b, void *fs_, void *fh_, const int *orb_pattern, int n_desired, const float *response, int cap, float *feat, unsigned char *desc, ldso_immature_t *imm, int *counts) {
    GUARD(
        GpuBackend &B = *(GpuBackend *) b; FullSystem &fs = *(FullSystem *) fs_; std::shared_ptr<FrameHessian> fh = *(std::shared_ptr<FrameHessian> *) fh_;
        setting_pointSelection = 1; setting_desiredImmatureDensity = n_desired; setting_gammaWeightsPixelSelect = 1;
        if (response) for (int i = 0; i < 256; i++) fs.Hcalib->mpCH->B[i] = response[i];
        B.orbPattern = orb_pattern;
        fh->frame->features.clear();
        B.makeNewTraces(fs, fh);
        for (int i = 0; i < 3; i++) counts[i] = B.lastNewTraces[i];
        counts[3] = (int) fh->frame->features.size();
        int hostIdx = -1;
        for (size_t f = 0; f < fs.frames.size(); f++) if (fs.frames[f] == fh->frame) hostIdx = (int) f;
        int k = 0;
        for (auto &f : fh->frame->features) {
            if (k >= cap) break;
            float *o = feat + 5 * k;
            o[0] = f->uv[0]; o[1] = f->uv[1]; o[2] = f->score; o[3] = f->isCorner ? 1 : 0; o[4] = f->angle;
            memcpy(desc + 32 * k, f->descriptor, 32);
            ldso_immature_t &q = imm[k];
            memset(&q, 0, sizeof(q));
            ImmaturePoint &ip = *f->ip;
            q.u = f->uv[0]; q.v = f->uv[1];
            memcpy(q.color, ip.color, sizeof(q.color)); memcpy(q.weights, ip.weights, sizeof(q.weights));
            q.gradH[0] = ip.gradH(0, 0); q.gradH[1] = ip.gradH(0, 1); q.gradH[2] = ip.gradH(1, 0); q.gradH[3] = ip.gradH(1, 1);
            q.energyTH = ip.energyTH; q.idepth_min = ip.idepth_min; q.idepth_max = ip.idepth_max; q.quality = ip.quality;
            q.lastTraceStatus = (int32_t) ip.lastTraceStatus; q.lastTraceUV[0] = ip.lastTraceUV[0]; q.lastTraceUV[1] = ip.lastTraceUV[1];
            q.lastTracePixelInterval = ip.lastTracePixelInterval; q.host = hostIdx;
            k++;
        })
}

// fh = ref_fs_new_frame(window, ...): makeNewTraces with setting_pointSelection = 0 and setting_desiredImmatureDensity = density on one frame - b == nullptr:
// the reference's own FullSystem::makeNewTraces (FullSystem.cc:1284-1304), else GpuBackend::makeNewTraces.  The reference's member reads absSquaredGrad and
// levels 1-2, which ref_fs_new_frame does not build: for that leg the frame's images are made here by FrameHessian::makeImages from the irradiance of its level 0
// (the rows of absSquaredGrad[1] / [2] that makeImages never writes zeroed, as ldso_hip.h defines them) and taken away again before the entry returns.
// potential_inout = pixelSelector->currentPotential before / after.  Out as adp_make_new_traces: uv [cap][2], imm [cap] (host = the frame's window index or -1),
// type [cap] = my_type; counts[4] = points made, 0, dropped, frame->features.size().  The three process-wide settings are restored before the entry returns.
int adp_make_new_traces_pixsel(void *b, void *fs_, void *fh_, float density, const float *response, int *potential_inout, int cap, float *uv, ldso_immature_t *imm, float *type, int *counts) {
    if (!fs_ || !fh_ || !potential_inout || !counts) return LDSO_E_INVALID;
    const int savedSelection = setting_pointSelection; const float savedDensity = setting_desiredImmatureDensity; const int savedGamma = setting_gammaWeightsPixelSelect;
    struct Restore { int s; float d; int g; ~Restore() { setting_pointSelection = s; setting_desiredImmatureDensity = d; setting_gammaWeightsPixelSelect = g; } } restore{savedSelection, savedDensity, savedGamma};
    GUARD(
        FullSystem &fs = *(FullSystem *) fs_; std::shared_ptr<FrameHessian> fh = *(std::shared_ptr<FrameHessian> *) fh_;
        setting_pointSelection = 0; setting_desiredImmatureDensity = density; setting_gammaWeightsPixelSelect = 1;
        if (response) for (int i = 0; i < 256; i++) fs.Hcalib->mpCH->B[i] = response[i];
        fs.pixelSelector->currentPotential = *potential_inout;
        fh->frame->features.clear();
        for (int i = 0; i < 4; i++) counts[i] = 0;
        if (b) {
            GpuBackend &B = *(GpuBackend *) b;
            B.makeNewTraces(fs, fh);
            for (int i = 0; i < 3; i++) counts[i] = B.lastNewTraces[i];
        } else {
            Vec3f *level0 = fh->dIp[0];
            std::vector<float> color((size_t) wG[0] * hG[0]);
            for (size_t i = 0; i < color.size(); i++) color[i] = level0[i][0];
            fh->makeImages(color.data(), fs.Hcalib->mpCH);
            for (int l = 1; l < 3 && l < pyrLevelsUsed; l++) for (int x = 0; x < wG[l]; x++) fh->absSquaredGrad[l][x + (hG[l] - 1) * wG[l]] = 0;
            fs.makeNewTraces(fh, nullptr);
            for (int l = 0; l < pyrLevelsUsed; l++) { delete[] fh->dIp[l]; delete[] fh->absSquaredGrad[l]; fh->dIp[l] = nullptr; fh->absSquaredGrad[l] = nullptr; }
            fh->dIp[0] = level0; fh->dI = level0;
            fs.pixelSelector->gradHistFrame = nullptr;          // its histogram belongs to images that are gone
            counts[0] = (int) fh->frame->features.size();
        }
        *potential_inout = fs.pixelSelector->currentPotential;
        counts[3] = (int) fh->frame->features.size();
        int hostIdx = -1;
        for (size_t f = 0; f < fs.frames.size(); f++) if (fs.frames[f] == fh->frame) hostIdx = (int) f;
        int k = 0;
        for (auto &f : fh->frame->features) {
            if (k >= cap) break;
            uv[2 * k] = f->uv[0]; uv[2 * k + 1] = f->uv[1];
            ldso_immature_t &q = imm[k];
            memset(&q, 0, sizeof(q));
            ImmaturePoint &ip = *f->ip;
            q.u = f->uv[0]; q.v = f->uv[1];
            memcpy(q.color, ip.color, sizeof(q.color)); memcpy(q.weights, ip.weights, sizeof(q.weights));
            q.gradH[0] = ip.gradH(0, 0); q.gradH[1] = ip.gradH(0, 1); q.gradH[2] = ip.gradH(1, 0); q.gradH[3] = ip.gradH(1, 1);
            q.energyTH = ip.energyTH; q.idepth_min = ip.idepth_min; q.idepth_max = ip.idepth_max; q.quality = ip.quality;
            q.lastTraceStatus = (int32_t) ip.lastTraceStatus; q.lastTraceUV[0] = ip.lastTraceUV[0]; q.lastTraceUV[1] = ip.lastTraceUV[1];
            q.lastTracePixelInterval = ip.lastTracePixelInterval; q.host = hostIdx;
            type[k] = ip.my_type;
            k++;
        })
}

// the three process-wide settings the makeNewTraces entries write
int adp_point_selection_settings(int *pointSelection, float *desiredImmatureDensity, int *gammaWeightsPixelSelect) {
    if (!pointSelection || !desiredImmatureDensity || !gammaWeightsPixelSelect) return LDSO_E_INVALID;
    *pointSelection = setting_pointSelection; *desiredImmatureDensity = setting_desiredImmatureDensity; *gammaWeightsPixelSelect = setting_gammaWeightsPixelSelect;
    return 0;
}

// ---- raw camera frames (tests/test_undistort_adapter_gpu.py) ---------------------------------------------------------------------------------
// GpuBackend::setUndistortion under the two settings it reads; the output size is the window's (wG[0] x hG[0])
int adp_set_undistortion(void *b, int wOrg, int hOrg, const float *remapX, const float *remapY, const float *G, int GDepth, const float *vignetteMapInv, int photometricCalibration, int useExposure) {
    GUARD(setting_photometricCalibration = photometricCalibration; setting_useExposure = useExposure != 0;
          ((GpuBackend *) b)->setUndistortion(wOrg, hOrg, remapX, remapY, G, GDepth, vignetteMapInv))
}
// fh = ref_fs_new_frame(window, ...): its Frame::id, the key undistortFrame registers the pyramid under
long adp_frame_id(void *fh) { return (long) (*(std::shared_ptr<FrameHessian> *) fh)->frame->id; }
int adp_undistort_frame(void *b, long frameId, const void *raw, int bytesPerPixel, float exposure, float factor, float *hostIrradiance, float *exposureOut) {
    GUARD(*exposureOut = ((GpuBackend *) b)->undistortFrame((unsigned long) frameId, raw, bytesPerPixel, exposure, factor, hostIrradiance))
}
int adp_pyr_levels_used() { return pyrLevelsUsed; }
// level lvl of the device pyramid the backend holds for fh (built from fh->dIp[0] if there is none yet): wG[lvl] * hG[lvl] * 3 floats
int adp_get_pyramid_level(void *b, void *fh, int lvl, float *out) { GUARD(((GpuBackend *) b)->getPyramidLevel(*(std::shared_ptr<FrameHessian> *) fh, lvl, out)) }

int adp_set_device_pyramids(void *b, int on) { ((GpuBackend *) b)->useDevicePyramids = on != 0; return 0; }
int adp_pyramids_built(void *b) { return ((GpuBackend *) b)->pyramidsBuilt; }
int adp_set_write_back_jacobians(void *b, int on) { ((GpuBackend *) b)->writeBackJacobians = on != 0; return 0; }
// the window resident across optimize() calls (ldso_ba_update_window) or flattened and uploaded every time; how many uploads of each kind so far
int adp_set_resident_window(void *b, int on) { ((GpuBackend *) b)->residentWindow = on != 0; return 0; }
int adp_upload_counts(void *b, int *delta, int *fresh) { *delta = ((GpuBackend *) b)->uploadsDelta; *fresh = ((GpuBackend *) b)->uploadsFresh; return 0; }
// GpuBackend::marginalizeFrame: how often the Schur complement ran on the device (ldso_ba_marginalize_frame) and how often the call fell back to the reference's host member
int adp_marg_frame_counts(void *b, int *device, int *hostFallback) { *device = ((GpuBackend *) b)->margFrameDevice; *hostFallback = ((GpuBackend *) b)->margFrameHostFallback; return 0; }
// wall-clock split of the last GpuBackend::optimize (seconds): flatten + upload, device (ldso_ba_optimize incl. its read-back of the energies), fetch, write-back into the objects
int adp_last_optimize_times(void *b, double *out4) { for (int i = 0; i < 4; i++) out4[i] = ((GpuBackend *) b)->lastOptimizeSeconds[i]; return 0; }
int adp_last_upload_times(void *b, double *out6) { for (int i = 0; i < 6; i++) out6[i] = ((GpuBackend *) b)->lastUploadSeconds[i]; return 0; }

// ---- the immature set resident on the device (GpuBackend::residentImmature; tests/test_immature_resident_*.py) -----------------------------------------------
// the three entries refuse a missing backend / graph / output with LDSO_E_INVALID and touch nothing
int adp_set_resident_immature(void *b, int on) { if (!b) return LDSO_E_INVALID; ((GpuBackend *) b)->residentImmature = on != 0; return 0; }
// GpuBackend::syncImmaturePoints: the device's trace state into the ImmaturePoint objects
int adp_sync_immature(void *b, void *fs) { if (!b || !fs) return LDSO_E_INVALID; GUARD(((GpuBackend *) b)->syncImmaturePoints(*(FullSystem *) fs)) }
// how the reconcile steps of this backend went: [rows unchanged, one compaction, full upload]
int adp_immature_reconcile_counts(void *b, int *out3) { if (!b || !out3) return LDSO_E_INVALID; for (int i = 0; i < 3; i++) out3[i] = ((GpuBackend *) b)->immatureReconcile[i]; return 0; }
// the decision of GpuBackend::reconcileImmature (adp::planReconcile) on plain data, no backend and no device: integer ids stand for the ImmaturePoints.  Rows
// (id, host index the device record carries) against the graph's current list (id, host index now).  Returns 0 same / 1 compact / 2 re-upload, or
// LDSO_E_INVALID; keep[nRows] and hostMap[LDSO_MAX_FRAMES] (-1: unset) are written for outcome 1 only.
int adp_reconcile_plan(int nRows, const int *rowId, const int *rowHost, int nCur, const int *curId, const int *curHost, int haveTracer, unsigned char *keep, int *hostMap) {
    if (nRows < 0 || nCur < 0 || (nRows && (!rowId || !rowHost)) || (nCur && (!curId || !curHost)) || !keep || !hostMap) return LDSO_E_INVALID;
    const std::vector<int> rows(rowId, rowId + nRows), rHost(rowHost, rowHost + nRows), cur(curId, curId + nCur), cHost(curHost, curHost + nCur);
    const adp::ReconcilePlan plan = adp::planReconcile(cur, cHost, rows, rHost, haveTracer != 0);
    if (plan.outcome == adp::ReconcilePlan::Compact) {
        for (int i = 0; i < nRows; i++) keep[i] = plan.keep[i];
        for (int f = 0; f < LDSO_MAX_FRAMES; f++) hostMap[f] = plan.hostMap[f];
    }
    return (int) plan.outcome;
}

// a new tracer of this backend holds at least n records (GpuBackend::tracerMinCapacity): a small value lets a test reach the path on which the tracer has to grow
int adp_set_tracer_min_capacity(void *b, int n) { if (!b || n < 1) return LDSO_E_INVALID; ((GpuBackend *) b)->tracerMinCapacity = n; return 0; }
// GpuBackend::makeNewTraces on key frame frameIdx of the window, behind the features it already has (adp_make_new_traces clears them and takes a frame from
// ref_fs_new_frame): the new immature points are hosted by a frame of the window, so the traces and activations that follow see them.  counts[4] as there.
int adp_make_new_traces_window(void *b, void *fs_, int frameIdx, const int *orb_pattern, int n_desired, int *counts) {
    if (!b || !fs_ || !counts) return LDSO_E_INVALID;
    GUARD(
        GpuBackend &B = *(GpuBackend *) b; FullSystem &fs = *(FullSystem *) fs_;
        if (frameIdx < 0 || frameIdx >= (int) fs.frames.size()) throw std::runtime_error("adp_make_new_traces_window: no such key frame");
        setting_pointSelection = 1; setting_desiredImmatureDensity = n_desired; setting_gammaWeightsPixelSelect = 1;
        B.orbPattern = orb_pattern;
        shared_ptr<FrameHessian> fh = fs.frames[frameIdx]->frameHessian;
        B.makeNewTraces(fs, fh);
        for (int i = 0; i < 3; i++) counts[i] = B.lastNewTraces[i];
        counts[3] = (int) fh->frame->features.size())
}

// ---- one key frame in the order of FullSystem::makeKeyFrame (FullSystem.cc:410-640) on a reference object graph -----------------------------
// b == nullptr: the reference's own members everywhere.  b != nullptr: GpuBackend::traceNewCoarse / activatePoints / optimize in place of
// FullSystem::traceNewCoarse (:429), the optimizeImmaturePoint loop of activatePointsMT (:1157-1166) and FullSystem::optimize (:478); everything
// else - ef->insertFrame, the new residuals of old points, removeOutliers, flagPointsForRemoval, dropPointsF, marginalizePointsF,
// marginalizeFrame - is the reference's host code on both graphs, as in a first integration of the drop-in.
// What is POLICY upstream of the hot path is decided by the caller, identically for both graphs: which frame is flagged for marginalisation
// (flagFramesForMarginalization -> margIdx, -1: none), the key-frame number (globalMap->NumFrames() -> kfId), and the candidate selection of
// activatePointsMT, which is restated below WITHOUT the distance map (every immature point that passes the canActivate rule and projects into
// the newest frame is a candidate).  The coarse-tracker swap (:515-522) and makeNewTraces (:539: pixel selection) are the caller's business.
// newfh = shared_ptr<FrameHessian>* of ref_fs_new_frame.  stats: [candidates, activated, residuals added for old points, points after, lost]
static bool deviceMarginalisation = false;
int adp_set_device_marginalisation(int on) { deviceMarginalisation = on != 0; return 0; }
// FullSystem::activatePointsMT WITH the distance map and the density controller: GpuBackend::activatePointsMT with a backend, the reference's own member without
// one, in place of the restated candidate rule below.  Then stats[0] = immature points that left that state (selected or deleted), stats[1] = new active points.
static bool distanceMap = false;
static std::vector<float> minActDistTrace;          // fs.currentMinActDist after every activatePointsMT of adp_make_keyframe since the switch was last set
int adp_set_distance_map(int on) { distanceMap = on != 0; minActDistTrace.clear(); return 0; }
int adp_min_act_dist_trace(int cap, float *out) { for (int i = 0; i < cap && i < (int) minActDistTrace.size(); i++) out[i] = minActDistTrace[i]; return (int) minActDistTrace.size(); }
static void count_points(FullSystem &fs, int &active, int &immature) {
    active = immature = 0;
    for (auto &fr : fs.frames) for (auto &feat : fr->features) {
        if (feat->status == Feature::FeatureStatus::VALID && feat->point && feat->point->status == Point::PointStatus::ACTIVE) active++;
        else if (feat->status == Feature::FeatureStatus::IMMATURE && feat->ip) immature++;
    }
}
int adp_make_keyframe(void *b, void *fs_, void *newfh, int margIdx, int kfId, int iterations, float *rmse, int *stats) {
    GUARD(
        GpuBackend *B = (GpuBackend *) b; FullSystem &fs = *(FullSystem *) fs_;
        shared_ptr<FrameHessian> fh = *(shared_ptr<FrameHessian> *) newfh;
        for (int i = 0; i < 5; i++) stats[i] = 0;
        // :429 trace new keyframe
        if (B) B->traceNewCoarse(fs, fh); else fs.traceNewCoarse(fh);
        // :434 flag frames to be marginalised (policy: the caller's choice)
        if (margIdx >= 0) fs.frames[margIdx]->frameHessian->flaggedForMarginalization = true;
        // :437-442 add the new frame
        fh->idx = fs.frames.size();
        fs.frames.push_back(fh->frame);
        fh->frame->kfId = fh->frameID = kfId;
        fs.ef->insertFrame(fh, fs.Hcalib->mpCH);
        fs.setPrecalcValues();
        // :447-470 new residuals for old points
        for (auto fht : fs.frames) {
            shared_ptr<FrameHessian> &fh1 = fht->frameHessian;
            if (fh1 == fh) continue;
            for (auto feat : fht->features) {
                if (feat->status == Feature::FeatureStatus::VALID && feat->point->status == Point::PointStatus::ACTIVE) {
                    shared_ptr<PointHessian> ph = feat->point->mpPH;
                    shared_ptr<PointFrameResidual> r(new PointFrameResidual(ph, fh1, fh));
                    r->setState(ResState::IN);
                    ph->residuals.push_back(r);
                    fs.ef->insertResidual(r);
                    ph->lastResiduals[1] = ph->lastResiduals[0];
                    ph->lastResiduals[0] = std::pair<shared_ptr<PointFrameResidual>, ResState>(r, ResState::IN);
                    stats[2]++;
                }
            }
        }
        // :473 activatePointsMT: candidate rule of :1090-1150 (no distance map), the optimizeImmaturePoint loop, the object hand-over of :1168-1190
        if (distanceMap) {
            int a0, i0, a1, i1;
            count_points(fs, a0, i0);
            if (B) B->activatePointsMT(fs); else fs.activatePointsMT();
            count_points(fs, a1, i1);
            stats[0] = i0 - i1; stats[1] = a1 - a0;
            minActDistTrace.push_back(fs.currentMinActDist);
        } else {
            auto newestFr = fs.frames.back();
            fs.coarseDistanceMap->makeK(fs.Hcalib->mpCH);
            std::vector<shared_ptr<ImmaturePoint>> toOptimize;
            for (auto fr : fs.frames) {
                shared_ptr<FrameHessian> host = fr->frameHessian;
                if (host == newestFr->frameHessian) continue;
                SE3 fhToNew = newestFr->frameHessian->PRE_worldToCam * host->PRE_camToWorld;
                Mat33f KRKi = (fs.coarseDistanceMap->K[1] * fhToNew.rotationMatrix().cast<float>() * fs.coarseDistanceMap->Ki[0]);
                Vec3f Kt = (fs.coarseDistanceMap->K[1] * fhToNew.translation().cast<float>());
                for (size_t i = 0; i < host->frame->features.size(); i++) {
                    shared_ptr<Feature> &feat = host->frame->features[i];
                    if (!(feat->status == Feature::FeatureStatus::IMMATURE && feat->ip)) continue;
                    shared_ptr<ImmaturePoint> &ph = feat->ip;
                    ph->idxInImmaturePoints = i;
                    if (!std::isfinite(ph->idepth_max) || ph->lastTraceStatus == IPS_OUTLIER) { feat->status = Feature::FeatureStatus::OUTLIER; feat->ReleaseImmature(); continue; }
                    bool canActivate = (ph->lastTraceStatus == IPS_GOOD || ph->lastTraceStatus == IPS_SKIPPED || ph->lastTraceStatus == IPS_BADCONDITION || ph->lastTraceStatus == IPS_OOB)
                                       && ph->lastTracePixelInterval < 8 && ph->quality > setting_minTraceQuality && (ph->idepth_max + ph->idepth_min) > 0;
                    if (!canActivate) {
                        if (ph->feature->host.lock()->frameHessian->flaggedForMarginalization || ph->lastTraceStatus == IPS_OOB) { feat->status = Feature::FeatureStatus::OUTLIER; feat->ReleaseImmature(); }
                        continue;
                    }
                    Vec3f ptp = KRKi * Vec3f(feat->uv[0], feat->uv[1], 1) + Kt * (0.5f * (ph->idepth_max + ph->idepth_min));
                    int u = ptp[0] / ptp[2] + 0.5f;
                    int v = ptp[1] / ptp[2] + 0.5f;
                    if ((u > 0 && v > 0 && u < wG[1] && v < hG[1])) toOptimize.push_back(ph);
                    else { feat->status = Feature::FeatureStatus::OUTLIER; feat->ReleaseImmature(); }
                }
            }
            stats[0] = (int) toOptimize.size();
            std::vector<shared_ptr<PointHessian>> optimized(toOptimize.size());
            if (B) { if (!toOptimize.empty()) B->activatePoints(fs, toOptimize, optimized); }
            else fs.activatePointsMT_Reductor(&optimized, &toOptimize, 0, (int) toOptimize.size(), 0, 0);
            for (size_t k = 0; k < toOptimize.size(); k++) {
                shared_ptr<PointHessian> newpoint = optimized[k];
                shared_ptr<ImmaturePoint> ph = toOptimize[k];
                if (newpoint != nullptr) {
                    ph->feature->status = Feature::FeatureStatus::VALID;
                    ph->feature->point->mpPH = newpoint;
                    ph->feature->ReleaseImmature();
                    newpoint->takeData();
                    for (auto r : newpoint->residuals) fs.ef->insertResidual(r);
                    stats[1]++;
                } else if (newpoint == nullptr || ph->lastTraceStatus == IPS_OOB) {
                    ph->feature->status = Feature::FeatureStatus::OUTLIER;
                    ph->feature->ReleaseImmature();
                }
            }
        }
        fs.ef->makeIDX();
        // :477-478 optimize
        fh->frameEnergyTH = fs.frames.back()->frameHessian->frameEnergyTH;
        *rmse = B ? B->optimize(fs, iterations) : fs.optimize(iterations);
        if (fs.isLost) { stats[4] = 1; return 0; }
        // :511 remove outliers; :526-536 flag / drop / marginalise points
        fs.removeOutliers();
        if (B && deviceMarginalisation) {
            // the device keeps the window of optimize(): the policy on the host, the re-linearise / fix / accumulate of the marginalised points on the device
            B->flagPointsForRemoval(fs);
            fs.ef->dropPointsF();
            fs.getNullspaces(fs.ef->lastNullspaces_pose, fs.ef->lastNullspaces_scale, fs.ef->lastNullspaces_affA, fs.ef->lastNullspaces_affB);
            B->marginalizePoints(fs);
        } else {
            fs.flagPointsForRemoval();
            fs.ef->dropPointsF();
            fs.getNullspaces(fs.ef->lastNullspaces_pose, fs.ef->lastNullspaces_scale, fs.ef->lastNullspaces_affA, fs.ef->lastNullspaces_affB);
            fs.ef->marginalizePointsF();
        }
        // :594-603 marginalise the flagged frames (their pyramids live in the driver's image store: ~FrameHessian must not delete[] them)
        for (unsigned int i = 0; i < fs.frames.size(); i++)
            if (fs.frames[i]->frameHessian->flaggedForMarginalization) {
                shared_ptr<Frame> fr = fs.frames[i];
                for (int l = 0; l < PYR_LEVELS; l++) { fr->frameHessian->dIp[l] = nullptr; fr->frameHessian->absSquaredGrad[l] = nullptr; }
                if (B && deviceMarginalisation) B->marginalizeFrame(fs, fr); else fs.marginalizeFrame(fr);
                i = 0;
            }
        for (auto &fr : fs.frames) for (auto &feat : fr->features) if (feat->status == Feature::FeatureStatus::VALID && feat->point && feat->point->status == Point::PointStatus::ACTIVE) stats[3]++;
    )
}

// What a trajectory / map comparison needs of the graph after a key frame: per frame [Frame::id, camToWorld 3x4 row-major (PRE_camToWorld), a, b, active points
// hosted, residuals hosted, immature points hosted, frameEnergyTH] (18 doubles), then HM (n x n) and bM (n) with n = 8 F + 4; returns F
int adp_graph_summary(void *fs_, int capFrames, double *frames18, double *HM, double *bM, double *calib4) {
    FullSystem &fs = *(FullSystem *) fs_;
    const int F = (int) fs.frames.size();
    for (int f = 0; f < F && f < capFrames; f++) {
        FrameHessian &fh = *fs.frames[f]->frameHessian;
        double *o = frames18 + 18 * f;
        o[0] = (double) fs.frames[f]->id;
        Eigen::Matrix<double, 3, 4> M = fh.PRE_camToWorld.matrix3x4();
        for (int i = 0; i < 3; i++) for (int j = 0; j < 4; j++) o[1 + i * 4 + j] = M(i, j);
        o[13] = fh.aff_g2l().a; o[14] = fh.aff_g2l().b;
        int np = 0, nr = 0, ni = 0;
        for (auto &feat : fs.frames[f]->features) {
            if (feat->status == Feature::FeatureStatus::VALID && feat->point && feat->point->status == Point::PointStatus::ACTIVE) { np++; nr += (int) feat->point->mpPH->residuals.size(); }
            else if (feat->status == Feature::FeatureStatus::IMMATURE && feat->ip) ni++;
        }
        o[15] = np; o[16] = nr; o[17] = ni;
    }
    const int n = (int) fs.ef->HM.rows();
    if (HM) for (int i = 0; i < n; i++) { for (int j = 0; j < n; j++) HM[(size_t) i * n + j] = fs.ef->HM(i, j); bM[i] = fs.ef->bM[i]; }
    if (calib4) for (int i = 0; i < 4; i++) calib4[i] = fs.Hcalib->mpCH->value[i];
    return F;
}
// inverse depths of the active points in traversal order (frames, then their features) - up to cap; returns the count.  host = Frame::id of the host
// key frame, uv = the point's pixel: (host, u, v) identifies a point across two object graphs whose point sets differ by a few threshold cases
int adp_graph_idepths(void *fs_, int cap, float *idepth, int *host, float *uv) {
    FullSystem &fs = *(FullSystem *) fs_;
    int n = 0;
    for (size_t f = 0; f < fs.frames.size(); f++)
        for (auto &feat : fs.frames[f]->features)
            if (feat->status == Feature::FeatureStatus::VALID && feat->point && feat->point->status == Point::PointStatus::ACTIVE) {
                if (n < cap) { idepth[n] = feat->point->mpPH->idepth; host[n] = (int) fs.frames[f]->id; uv[2 * n] = feat->uv[0]; uv[2 * n + 1] = feat->uv[1]; }
                n++;
            }
    return n;
}

// ---- candidate selection (FullSystem::activatePointsMT, FullSystem.cc:1052-1189) ------------------------------------------------------------
// setting_desiredPointDensity (Settings.h:69); returns the value it replaces
float adp_set_desired_point_density(float v) { const float old = setting_desiredPointDensity; setting_desiredPointDensity = v; return old; }
float adp_get_min_act_dist(void *fs) { return ((FullSystem *) fs)->currentMinActDist; }
void adp_set_min_act_dist(void *fs, float v) { ((FullSystem *) fs)->currentMinActDist = v; }
int adp_ef_npoints(void *fs) { return ((FullSystem *) fs)->ef->nPoints; }
void adp_set_ef_npoints(void *fs, int n) { ((FullSystem *) fs)->ef->nPoints = n; }
// coarseDistanceMap->fwdWarpedIDDistFinal, wG[1] * hG[1] floats; returns that count
int adp_get_ref_distance_map(void *fs_, float *out) {
    FullSystem &fs = *(FullSystem *) fs_;
    const int n = wG[1] * hG[1];
    if (out) memcpy(out, fs.coarseDistanceMap->fwdWarpedIDDistFinal, (size_t) n * sizeof(float));
    return n;
}
// the reference's own member
int adp_ref_activate_points_mt(void *fs) { GUARD(((FullSystem *) fs)->activatePointsMT()) }
int adp_activate_points_mt(void *b, void *fs, int *counts3) { GUARD(((GpuBackend *) b)->activatePointsMT(*(FullSystem *) fs); for (int i = 0; i < 3; i++) counts3[i] = ((GpuBackend *) b)->lastSelection[i]) }
// ImmaturePoint::my_type of the immature points of the graph in traversal order (all frames, then their features: the order of ref_fs_get_immature)
int adp_set_immature_types(void *fs_, int n, const float *types) {
    FullSystem &fs = *(FullSystem *) fs_;
    int k = 0;
    for (auto &fr : fs.frames) for (auto &feat : fr->features) if (feat->status == Feature::FeatureStatus::IMMATURE && feat->ip) { if (k < n) feat->ip->my_type = types[k]; k++; }
    return k;
}
// Point::status of every point of the graph (a graph without ACTIVE points has no seeds for the distance map); returns how many were set
int adp_set_all_point_status(void *fs_, int status) {
    FullSystem &fs = *(FullSystem *) fs_;
    int k = 0;
    for (auto &fr : fs.frames) for (auto &feat : fr->features) if (feat->point) { feat->point->status = (Point::PointStatus) status; k++; }
    return k;
}
// Feature::status of every feature of the graph in traversal order (up to cap); returns the count
int adp_feature_statuses(void *fs_, int cap, int *status) {
    FullSystem &fs = *(FullSystem *) fs_;
    int k = 0;
    for (auto &fr : fs.frames) for (auto &feat : fr->features) { if (k < cap) status[k] = (int) feat->status; k++; }
    return k;
}
// What the selection reads from the graph (GpuBackend::gatherSelection), as flat arrays: the common state handed to the device leg of a comparison.
// counts: [seeds, candidates, hosts]; any output may be NULL (first call: sizes only)
int adp_gather_selection(void *fs_, int *counts, ldso_act_seed_t *seeds, ldso_immature_t *cand, float *myType, float *KRKi, float *Kt, int *flagged) {
    GUARD(
        GpuBackend::SelectionInputs in;
        GpuBackend::gatherSelection(*(FullSystem *) fs_, in);
        counts[0] = (int) in.seeds.size(); counts[1] = (int) in.cand.size(); counts[2] = (int) in.flagged.size();
        if (seeds && !in.seeds.empty()) memcpy(seeds, in.seeds.data(), in.seeds.size() * sizeof(ldso_act_seed_t));
        if (cand && !in.cand.empty()) memcpy(cand, in.cand.data(), in.cand.size() * sizeof(ldso_immature_t));
        if (myType && !in.myType.empty()) memcpy(myType, in.myType.data(), in.myType.size() * sizeof(float));
        if (KRKi) memcpy(KRKi, in.KRKi.data(), in.KRKi.size() * sizeof(float));
        if (Kt) memcpy(Kt, in.Kt.data(), in.Kt.size() * sizeof(float));
        if (flagged) memcpy(flagged, in.flagged.data(), in.flagged.size() * sizeof(int)))
}
// the immature points the selection loop visits, in its order (:1088-1098)
static std::vector<shared_ptr<ImmaturePoint>> selection_candidates(FullSystem &fs) {
    std::vector<shared_ptr<ImmaturePoint>> v;
    shared_ptr<FrameHessian> newest = fs.frames.back()->frameHessian;
    for (auto fr : fs.frames) {
        if (fr->frameHessian == newest) continue;
        for (size_t i = 0; i < fr->features.size(); i++) {
            shared_ptr<Feature> &feat = fr->features[i];
            if (feat->status == Feature::FeatureStatus::IMMATURE && feat->ip) { feat->ip->idxInImmaturePoints = i; v.push_back(feat->ip); }
        }
    }
    return v;
}
// The selection of FullSystem::activatePointsMT (:1075-1152) at `currentMinActDist`, driven through the reference's COMPILED CoarseDistanceMap members (makeK,
// makeDistanceMap, addIntoDistFinal) on fs.coarseDistanceMap.  Nothing of the graph changes (no status is written, nothing is activated): decision [n] =
// 0 keep / 1 drop / 2 selected per candidate in the loop's order, selected [n] = the selected indices in toOptimize's order, mapBefore / mapAfter [wG[1] * hG[1]].
// Returns the number of candidates (call with NULL outputs for the size), -1 on error.
int adp_ref_select_candidates(void *fs_, float currentMinActDist, int cap, int *decision, int *selected, int *nSelected, float *mapBefore, float *mapAfter) {
    try {
        FullSystem &fs = *(FullSystem *) fs_;
        std::vector<shared_ptr<ImmaturePoint>> cand = selection_candidates(fs);
        if (!decision) return (int) cand.size();
        if ((int) cand.size() > cap) throw std::runtime_error("adp_ref_select_candidates: output too small");
        auto newestFr = fs.frames.back();
        vector<shared_ptr<FrameHessian>> frameHessians;
        for (auto fr : fs.frames) frameHessians.push_back(fr->frameHessian);
        fs.coarseDistanceMap->makeK(fs.Hcalib->mpCH);
        fs.coarseDistanceMap->makeDistanceMap(frameHessians, newestFr->frameHessian);
        const size_t cells = (size_t) wG[1] * hG[1];
        if (mapBefore) memcpy(mapBefore, fs.coarseDistanceMap->fwdWarpedIDDistFinal, cells * sizeof(float));
        int k = 0, ns = 0;
        for (auto host : frameHessians) {
            if (host == newestFr->frameHessian) continue;
            SE3 fhToNew = newestFr->frameHessian->PRE_worldToCam * host->PRE_camToWorld;
            Mat33f KRKi = (fs.coarseDistanceMap->K[1] * fhToNew.rotationMatrix().cast<float>() * fs.coarseDistanceMap->Ki[0]);
            Vec3f Kt = (fs.coarseDistanceMap->K[1] * fhToNew.translation().cast<float>());
            for (size_t i = 0; i < host->frame->features.size(); i++) {
                shared_ptr<Feature> &feat = host->frame->features[i];
                if (!(feat->status == Feature::FeatureStatus::IMMATURE && feat->ip)) continue;
                shared_ptr<ImmaturePoint> &ph = feat->ip;
                int &dec = decision[k++];
                dec = 0;
                if (!std::isfinite(ph->idepth_max) || ph->lastTraceStatus == IPS_OUTLIER) { dec = 1; continue; }
                bool canActivate = (ph->lastTraceStatus == IPS_GOOD || ph->lastTraceStatus == IPS_SKIPPED || ph->lastTraceStatus == IPS_BADCONDITION || ph->lastTraceStatus == IPS_OOB)
                                   && ph->lastTracePixelInterval < 8 && ph->quality > setting_minTraceQuality && (ph->idepth_max + ph->idepth_min) > 0;
                if (!canActivate) {
                    if (ph->feature->host.lock()->frameHessian->flaggedForMarginalization || ph->lastTraceStatus == IPS_OOB) dec = 1;
                    continue;
                }
                Vec3f ptp = KRKi * Vec3f(feat->uv[0], feat->uv[1], 1) + Kt * (0.5f * (ph->idepth_max + ph->idepth_min));
                int u = ptp[0] / ptp[2] + 0.5f;
                int v = ptp[1] / ptp[2] + 0.5f;
                if ((u > 0 && v > 0 && u < wG[1] && v < hG[1])) {
                    float dist = fs.coarseDistanceMap->fwdWarpedIDDistFinal[u + wG[1] * v] + (ptp[0] - floorf((float) (ptp[0])));
                    if (dist >= currentMinActDist * ph->my_type) {
                        fs.coarseDistanceMap->addIntoDistFinal(u, v);
                        dec = 2; selected[ns++] = k - 1;
                    }
                } else dec = 1;
            }
        }
        *nSelected = ns;
        if (mapAfter) memcpy(mapAfter, fs.coarseDistanceMap->fwdWarpedIDDistFinal, cells * sizeof(float));
        return k;
    } catch (const std::exception &e) { std::snprintf(g_err, sizeof(g_err), "%s", e.what()); return -1; }
}
// what follows the selection in the member, on the host, for a selection made by adp_ref_select_candidates on this graph: the statuses of the deleted candidates
// (:1105-1108, :1121-1125, :1145-1148), the reference's activatePointsMT_Reductor on the selected ones (:1154-1164) and the hand-over of :1166-1188
int adp_ref_apply_selection(void *fs_, int n, const int *decision, int nSelected, const int *selected) {
    GUARD(
        FullSystem &fs = *(FullSystem *) fs_;
        std::vector<shared_ptr<ImmaturePoint>> cand = selection_candidates(fs);
        if ((int) cand.size() != n) throw std::runtime_error("adp_ref_apply_selection: the graph changed since the selection");
        std::vector<shared_ptr<ImmaturePoint>> toOptimize;
        for (int k = 0; k < nSelected; k++) toOptimize.push_back(cand[selected[k]]);
        for (int i = 0; i < n; i++) if (decision[i] == 1) { shared_ptr<Feature> feat = cand[i]->feature; feat->status = Feature::FeatureStatus::OUTLIER; feat->ReleaseImmature(); }
        std::vector<shared_ptr<PointHessian>> optimized(toOptimize.size());
        fs.activatePointsMT_Reductor(&optimized, &toOptimize, 0, (int) toOptimize.size(), 0, 0);
        for (size_t k = 0; k < toOptimize.size(); k++) {
            shared_ptr<PointHessian> newpoint = optimized[k];
            shared_ptr<ImmaturePoint> ph = toOptimize[k];
            shared_ptr<Feature> feat = ph->feature;
            if (newpoint != nullptr) {
                feat->status = Feature::FeatureStatus::VALID;
                feat->point->mpPH = newpoint;
                feat->ReleaseImmature();
                newpoint->takeData();
                for (auto r : newpoint->residuals) fs.ef->insertResidual(r);
            } else { feat->status = Feature::FeatureStatus::OUTLIER; feat->ReleaseImmature(); }
        })
}
// wall time of `reps` adp_ref_select_candidates-style selections (seconds each into out[reps]): scripts/time_activate_select.py's reference leg
int adp_time_ref_select_candidates(void *fs_, float currentMinActDist, int reps, double *out) {
    FullSystem &fs = *(FullSystem *) fs_;
    const int n = adp_ref_select_candidates(fs_, currentMinActDist, 0, nullptr, nullptr, nullptr, nullptr, nullptr);
    std::vector<int> dec(n + 1), sel(n + 1); int ns = 0;
    for (int r = 0; r < reps; r++) {
        auto t0 = std::chrono::steady_clock::now();
        if (adp_ref_select_candidates(fs_, currentMinActDist, n + 1, dec.data(), sel.data(), &ns, nullptr, nullptr) < 0) return -1;
        out[r] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
    (void) fs;
    return ns;
}

}  // extern "C"
