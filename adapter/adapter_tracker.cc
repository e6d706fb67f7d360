// adapter_tracker.cc — the coarse tracker: the tracker handles (GpuBackend::TrackerHandles) and the replacement bodies of CoarseTracker::makeK /
// setCoarseTrackingRef / trackNewestCoarse and FullSystem::trackNewCoarse.
#include "adapter_internal.h"

using namespace ldso::internal;
using namespace ldso::adp;

namespace ldso {

// ---- GpuBackend::TrackerHandles: the only code that takes its mutex --------------------------------------------------------------------------------------
ldso_tracker_t *GpuBackend::TrackerHandles::of(CoarseTracker &tr, int device) {
    std::lock_guard<std::mutex> lk(mutex_);
    auto it = trackers_.find(&tr);
    if (it != trackers_.end()) return it->second;
    ldso_tracker_t *t = nullptr;
    throwOn(ldso_tr_create(device, wG[0], hG[0], pyrLevelsUsed, &t), "ldso_tr_create");
    trackers_[&tr] = t;
    return t;
}

bool GpuBackend::TrackerHandles::newFrameResident(ldso_tracker_t *t, const shared_ptr<FrameHessian> &fh) {
    const unsigned long id = fh->frame ? fh->frame->id : ~0ul;
    std::lock_guard<std::mutex> lk(mutex_);
    auto it = newFrameId_.find(t);
    if (it != newFrameId_.end() && it->second == id && id != ~0ul) return true;
    newFrameId_[t] = id;
    return false;
}

void GpuBackend::TrackerHandles::holdRef(ldso_tracker_t *t, const PyrRef &pr) { std::lock_guard<std::mutex> lk(mutex_); pyr_[t].ref = pr; }
void GpuBackend::TrackerHandles::holdNewFrame(ldso_tracker_t *t, const PyrRef &pr) { std::lock_guard<std::mutex> lk(mutex_); pyr_[t].newFrame = pr; }
void GpuBackend::TrackerHandles::destroyAll() {          // ~GpuBackend: no other thread is left
    for (auto &kv : trackers_) ldso_tr_destroy(kv.second);
    trackers_.clear();
}

// a tracker gets its new frame: the pyramid (or the host arrays) goes over once per frame, not once per hypothesis
void GpuBackend::handNewFrame(ldso_tracker_t *t, const shared_ptr<FrameHessian> &fh) {
    if (trackers_.newFrameResident(t, fh)) return;
    if (useDevicePyramids && fh->frame) {
        PyrRef pr = pyramidOf(fh);
        trackers_.holdNewFrame(t, pr);
        throwOn(ldso_tr_set_new_frame_pyramid(t, pr->p, fh->ab_exposure), "ldso_tr_set_new_frame_pyramid");
    } else {
        const float *pyr[PYR_LEVELS];
        for (int l = 0; l < pyrLevelsUsed; l++) pyr[l] = (const float *) fh->dIp[l];
        throwOn(ldso_tr_set_new_frame(t, pyr, fh->ab_exposure), "ldso_tr_set_new_frame");
    }
}

// void CoarseTracker::makeK(shared_ptr<CalibHessian>)                                                            CoarseTracker.cc:219-246
void GpuBackend::makeK(CoarseTracker &tr, shared_ptr<CalibHessian> HCalib) {
    tr.makeK(HCalib);                                  // the host copies (w[], h[], K[] ...) other LDSO code reads; 20 scalar operations
    ldso_tracker_t *t = trackerOf(tr);
    const ldso_settings_t st = flatSettings();
    throwOn(ldso_tr_set_settings(t, &st), "ldso_tr_set_settings");
    const ldso_calib_t c = flatCalib(*HCalib);
    throwOn(ldso_tr_make_k(t, &c), "ldso_tr_make_k");
}

// void CoarseTracker::setCoarseTrackingRef(std::vector<shared_ptr<FrameHessian>> &)                               CoarseTracker.cc:248-256
void GpuBackend::setCoarseTrackingRef(CoarseTracker &tr, std::vector<shared_ptr<FrameHessian>> &frameHessians) {
    tr.lastRef = frameHessians.back();
    // makeCoarseDepthL0's inputs (:264-283): every active point whose newest residual is IN, as (Ku, Kv, new_idepth, HdiF); the scatter, the
    // pyramid of the depth map, the dilation and the point-cloud build (:285-438) run on the device
    std::vector<float> pts;
    for (shared_ptr<FrameHessian> &fh : frameHessians)
        for (shared_ptr<Feature> &feat : fh->frame->features) {
            if (!(feat->status == Feature::FeatureStatus::VALID && feat->point->status == Point::PointStatus::ACTIVE)) continue;
            shared_ptr<PointHessian> ph = feat->point->mpPH;
            if (ph->lastResiduals[0].first != 0 && ph->lastResiduals[0].second == ResState::IN) {
                shared_ptr<PointFrameResidual> r = ph->lastResiduals[0].first;
                pts.push_back(r->centerProjectedTo[0]); pts.push_back(r->centerProjectedTo[1]); pts.push_back(r->centerProjectedTo[2]); pts.push_back(ph->HdiF);
            }
        }
    tr.refFrameID = tr.lastRef->frame->id;
    tr.lastRef_aff_g2l = tr.lastRef->aff_g2l();
    tr.firstCoarseRMSE = -1;
    if (useDevicePyramids && tr.lastRef->frame) {
        ldso_tracker_t *t = trackerOf(tr);
        PyrRef pr = pyramidOf(tr.lastRef);
        trackers_.holdRef(t, pr);
        throwOn(ldso_tr_set_ref_pyramid(t, pr->p, tr.lastRef_aff_g2l.a, tr.lastRef_aff_g2l.b, tr.lastRef->ab_exposure, pts.data(), (int) (pts.size() / 4)),
                "ldso_tr_set_ref_pyramid");
        return;
    }
    const float *pyr[PYR_LEVELS];
    for (int l = 0; l < pyrLevelsUsed; l++) pyr[l] = (const float *) tr.lastRef->dIp[l];
    throwOn(ldso_tr_set_ref(trackerOf(tr), pyr, tr.lastRef_aff_g2l.a, tr.lastRef_aff_g2l.b, tr.lastRef->ab_exposure, pts.data(), (int) (pts.size() / 4)), "ldso_tr_set_ref");
}

// bool CoarseTracker::trackNewestCoarse(newFrameHessian, lastToNew_out, aff_g2l_out, coarsestLvl, minResForAbort)  CoarseTracker.cc:61-217
bool GpuBackend::trackNewestCoarse(CoarseTracker &tr, shared_ptr<FrameHessian> newFrameHessian, SE3 &lastToNew_out, AffLight &aff_g2l_out, int coarsestLvl,
                                   Vec5 minResForAbort) {
    ldso_tracker_t *t = trackerOf(tr);
    tr.newFrame = newFrameHessian;
    handNewFrame(t, newFrameHessian);
    double T[12], mr[5], lr[5], fl[3];
    float ab[2] = {(float) aff_g2l_out.a, (float) aff_g2l_out.b};
    toRowMajor34(lastToNew_out, T);
    for (int i = 0; i < 5; i++) mr[i] = minResForAbort[i];
    int ok = 0, its = 0;
    throwOn(ldso_tr_track(t, T, ab, coarsestLvl, mr, lr, fl, &ok, &its), "ldso_tr_track");
    for (int i = 0; i < 5; i++) tr.lastResiduals[i] = lr[i];
    for (int i = 0; i < 3; i++) tr.lastFlowIndicators[i] = fl[i];
    // `return false` from the level loop (:188-189, residual above 1.5 x minResForAbort) leaves the outputs untouched; the affine sanity
    // checks (:202-211) fail AFTER "set!" (:198-199)
    bool aborted = false;
    for (int l = coarsestLvl; l >= 0 && !aborted; l--) aborted = lr[l] > 1.5 * mr[l];
    if (!aborted) { lastToNew_out = fromRowMajor34(T); aff_g2l_out = AffLight(ab[0], ab[1]); }
    return ok != 0;
}

// Vec4 FullSystem::trackNewCoarse(shared_ptr<FrameHessian> fh)                                                   FullSystem.cc:179-386
Vec4 GpuBackend::trackNewCoarse(FullSystem &fs, shared_ptr<FrameHessian> fh) {
    CoarseTracker &tr = *fs.coarseTracker;
    ldso_tracker_t *t = trackerOf(tr);
    shared_ptr<FrameHessian> lastF = tr.lastRef;
    tr.newFrame = fh;
    handNewFrame(t, fh);
    double sprelast[12], slast[12], lastFw2c[12];
    float aff_last[2] = {0, 0};
    int posesValid = 0;
    if (fs.allFrameHistory.size() != 2) {                    // :192-195: with two frames in the history the reference ends up with an empty try list (its TODO)
        shared_ptr<Frame> s1 = fs.allFrameHistory[fs.allFrameHistory.size() - 2], s2 = fs.allFrameHistory[fs.allFrameHistory.size() - 3];
        unique_lock<mutex> crlock(fs.shellPoseMutex);
        toRowMajor34(s2->getPose(), sprelast); toRowMajor34(s1->getPose(), slast); toRowMajor34(lastF->frame->getPose(), lastFw2c);
        aff_last[0] = (float) s1->aff_g2l.a; aff_last[1] = (float) s1->aff_g2l.b;
        posesValid = (s1->poseValid && s2->poseValid && lastF->frame->poseValid) ? 1 : 0;
    } else {
        const double I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
        memcpy(sprelast, I, sizeof(I)); memcpy(slast, I, sizeof(I)); toRowMajor34(lastF->frame->getPose(), lastFw2c);
    }
    double rmse[5], res4[4], w2c[12];
    float aff_out[2];
    int tries = 0, good = 0;
    for (int i = 0; i < 5; i++) rmse[i] = fs.lastCoarseRMSE[i];
    throwOn(ldso_tr_track_new_coarse(t, sprelast, slast, lastFw2c, posesValid, aff_last, rmse, setting_reTrackThreshold, res4, w2c, aff_out, &tries, &good), "ldso_tr_track_new_coarse");
    if (!good) LOG(WARNING) << "BIG ERROR! tracking failed entirely. Take predicted pose and hope we may somehow recover." << endl;
    for (int i = 0; i < 5; i++) fs.lastCoarseRMSE[i] = rmse[i];
    fh->frame->setPose(fromRowMajor34(w2c));                                                     // :376-377
    fh->frame->aff_g2l = AffLight(aff_out[0], aff_out[1]);
    if (tr.firstCoarseRMSE < 0) tr.firstCoarseRMSE = rmse[0];
    return Vec4(res4[0], res4[1], res4[2], res4[3]);
}

}  // namespace ldso
