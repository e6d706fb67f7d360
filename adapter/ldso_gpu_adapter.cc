// ldso_gpu_adapter.cc — see ldso_gpu_adapter.h.  Compiles against the reference's headers (LDSO include/ + its Eigen / Sophus) and links
// libldso_hip.so; every function is the replacement body of the reference member function it cites.  This unit: the backend's lifetime and optimize() with its
// write-back.  The other jobs: adapter_pyramids.cc (device pyramids, undistortion, BA image slots), adapter_window.cc (the window's upload and its resident
// host view), adapter_marginalize.cc, adapter_activate.cc, adapter_immature.cc (tracing, the resident immature set, makeNewTraces), adapter_tracker.cc.
#include "adapter_internal.h"

using namespace ldso::internal;
using namespace ldso::adp;

namespace ldso {

GpuBackend::GpuBackend(int device, int maxFrames, int maxPoints) : device_(device), maxFrames_(maxFrames), maxPoints_(maxPoints) {
    throwOn(ldso_ba_create(device, wG[0], hG[0], maxFrames, maxPoints, &ba_), "ldso_ba_create");
    slotOwner_.assign(maxFrames, -1);
}

GpuBackend::~GpuBackend() {
    trackers_.destroyAll();
    if (features_) ldso_feat_destroy(features_);
    if (pixsel_) ldso_pixsel_destroy(pixsel_);
    if (undist_) ldso_undist_destroy(undist_);
    if (ba_) ldso_ba_destroy(ba_);
    // the pyramids go with the members, after the handles above that name them on the device
}

const char *GpuBackend::lastError() const { return ldso_last_error(); }

// ------------------------------------------------------------------------------------------------------------------------------------
// float FullSystem::optimize(int mnumOptIts)                                                                       FullSystem.cc:725-864
// ------------------------------------------------------------------------------------------------------------------------------------
float GpuBackend::optimize(FullSystem &fs, int mnumOptIts) {
    if (fs.frames.size() < 2) return 0;
    if (fs.frames.size() < 3) mnumOptIts = 20;
    if (fs.frames.size() < 4) mnumOptIts = 15;

    std::vector<shared_ptr<PointHessian>> allPoints;
    if (useDevicePyramids) releasePyramids(fs);
    const auto tWall0 = std::chrono::steady_clock::now();
    auto lap = [&](int i, std::chrono::steady_clock::time_point &t) { const auto n_ = std::chrono::steady_clock::now(); lastOptimizeSeconds[i] = std::chrono::duration<double>(n_ - t).count(); t = n_; };
    auto tLap = tWall0;
    if (uploadWindow(fs, allPoints, /*trustIndices*/ true) == 0) return 0;
    lap(0, tLap);
    const int F = (int) fs.frames.size(), P = (int) allPoints.size(), R = (int) window_.flat.size();
    const std::vector<PointFrameResidual *> &flat = window_.flat;
    const std::vector<int32_t> &resBegin = window_.resBegin;

    // activeResiduals (:735-755): only FullSystem::optimize itself reads the list (see fillActiveResiduals in the header)
    fs.activeResiduals.clear();
    if (fillActiveResiduals)
        for (int k = 0; k < P; k++) for (shared_ptr<PointFrameResidual> &r : allPoints[k]->residuals) if (!r->isLinearized) fs.activeResiduals.push_back(r);

    // the whole loop of :757-843 and the tail :845-851 (re-anchor the newest frame, adjoints, precalc, linearizeAll(true)) on the device
    float rmse = 0;
    const int rc = ldso_ba_optimize(ba_, mnumOptIts, /*force_all_iterations*/ 0, &rmse, &lastIterations);
    throwOn(rc, "ldso_ba_optimize");
    if (rc == LDSO_E_NONFINITE) { LOG(WARNING) << "KF Tracking failed: LOST!"; fs.isLost = true; }         // :853-857
    lap(1, tLap);

    // ---- write back ----------------------------------------------------------------------------------------------------------------
    // the landing buffers are members: 1 MB of fresh vectors per call is 1 MB of page faults and zero fill per call; everything in them is overwritten by the fetch
    if (wbRes_.size() < (size_t) R) { wbRes_.resize((size_t) R); wbState_.resize((size_t) R); wbActive_.resize((size_t) R); wbRemove_.resize((size_t) R); }
    if (wbPoints_.size() < (size_t) P) wbPoints_.resize((size_t) P);
    if (wbFrames_.size() < (size_t) F) { wbFrames_.resize((size_t) F); wbStep_.resize((size_t) F * 10); }
    std::vector<ldso_res_out_t> &ro = wbRes_; std::vector<int32_t> &st = wbState_, &act = wbActive_, &rem = wbRemove_;
    std::vector<ldso_point_out_t> &po = wbPoints_; std::vector<ldso_frame_t> &fo = wbFrames_; std::vector<double> &fstep = wbStep_;
    double cv[4], cs[4];
    throwOn(ldso_ba_get_results(ba_, ro.data(), st.data(), act.data(), rem.data(), po.data(), fo.data(), fstep.data(), cv, cs), "ldso_ba_get_results");      // one synchronisation
    std::vector<ldso_rawjac_t> Jv;
    if (writeBackJacobians) {
        std::vector<int32_t> ids((size_t) R);
        for (int i = 0; i < R; i++) ids[i] = i;
        Jv.resize((size_t) R);
        throwOn(ldso_ba_get_jacobians(ba_, ids.data(), R, Jv.data()), "ldso_ba_get_jacobians");
    }

    lap(2, tLap);
    // calibration and frames: the states through the reference's own setters (they rebuild state_scaled, PRE_worldToCam / PRE_camToWorld);
    // the newest frame was re-anchored (:845-848: setEvalPT(PRE_worldToCam, [0..0, a, b, 0, 0]))
    VecC v, vs;
    for (int i = 0; i < 4; i++) { v[i] = cv[i]; vs[i] = cs[i]; }
    fs.Hcalib->mpCH->setValue(v); fs.Hcalib->mpCH->step = vs;
    for (int f = 0; f < F; f++) {
        FrameHessian &fh = *fs.frames[f]->frameHessian;
        Vec10 s;
        for (int i = 0; i < 10; i++) { s[i] = fo[f].state[i]; fh.step[i] = fstep[(size_t) f * 10 + i]; }
        if (f == F - 1) fh.setEvalPT(fromRowMajor34(fo[f].worldToCam_evalPT), s); else fh.setState(s);
        fh.frameEnergyTH = fo[f].frameEnergyTH;                                                  // setNewFrameEnergyTH (:1762-1793)
    }
    // points (doStepFromBackup :1595-1606, AccumulatedSCHessian.cc:9-51, the fixing pass :1521-1536)
    for (int k = 0; k < P; k++) {
        if (k + 8 < P) { const char *nx = (const char *) allPoints[k + 8].get(); __builtin_prefetch(nx, 1); __builtin_prefetch(nx + 64, 1); __builtin_prefetch(nx + 192, 1); __builtin_prefetch(nx + 256, 1); }      // 304-byte objects
        PointHessian &ph = *allPoints[k];
        ph.setIdepth(po[k].idepth); ph.setIdepthZero(po[k].idepth);
        ph.step = po[k].step; ph.HdiF = po[k].HdiF; ph.bdSumF = po[k].bdSumF; ph.idepth_hessian = po[k].idepth_hessian;
        ph.Hdd_accAF = po[k].Hdd_accAF; ph.bd_accAF = po[k].bd_accAF; ph.Hdd_accLF = po[k].Hdd_accLF; ph.bd_accLF = po[k].bd_accLF;
        for (int i = 0; i < 4; i++) { ph.Hcd_accAF[i] = po[k].Hcd_accAF[i]; ph.Hcd_accLF[i] = po[k].Hcd_accLF[i]; }
        ph.maxRelBaseline = po[k].maxRelBaseline; ph.numGoodResiduals = po[k].numGoodResiduals;
    }
    // residuals: applyRes(true) of the fixing pass (Residuals.h:70-87), lastResiduals bookkeeping and removal (:1472-1489)
    for (int i = 0; i < R; i++) {
        // 12 000 separately allocated objects: the walk is a chain of cache misses unless the next ones are already on their way
        if (i + 12 < R) { const char *nx = (const char *) flat[i + 12]; __builtin_prefetch(nx, 1); __builtin_prefetch(nx + 176, 1); __builtin_prefetch(nx + 240, 1); __builtin_prefetch(nx + 287, 1); }      // state | centre | JpJdF (288-byte objects)
        PointFrameResidual &r = *flat[i];
        if (r.isLinearized) continue;                                                            // not in activeResiduals: untouched by optimize()
        r.state_NewEnergy = ro[i].state_NewEnergy; r.state_NewEnergyWithOutlier = ro[i].state_NewEnergyWithOutlier; r.state_NewState = (ResState) ro[i].state_NewState;
        r.state_state = (ResState) st[i]; r.state_energy = ro[i].state_NewEnergy; r.isActiveAndIsGoodNEW = act[i] != 0;
        for (int k = 0; k < 3; k++) r.centerProjectedTo[k] = ro[i].centerProjectedTo[k];
        for (int k = 0; k < 8; k++) r.JpJdF[k] = ro[i].JpJdF[k];
        if (writeBackJacobians && r.state_NewState != ResState::OOB) fromRaw(Jv[i], *r.J);
    }
    // (the residuals of point k are flat[resBegin[k] .. resBegin[k + 1]): no weak_ptr::lock() per residual to find the point)
    for (int k = 0; k < P; k++) {
        PointHessian &ph = *allPoints[k];
        for (int i = resBegin[k]; i < resBegin[k + 1]; i++) {
            PointFrameResidual *r = flat[i];
            if (r->isLinearized) continue;
            if (ph.lastResiduals[0].first.get() == r) ph.lastResiduals[0].second = r->state_state;
            else if (ph.lastResiduals[1].first.get() == r) ph.lastResiduals[1].second = r->state_state;
        }
    }
    for (int k = 0; k < P; k++)
        for (int i = resBegin[k]; i < resBegin[k + 1]; i++)
            if (rem[i]) ResidentWindow::dropResidual(window_.rows[k], flat[i], *fs.ef);           // :1472-1489, EnergyFunctional.cc:44-56
    int resInA = 0, resInL = 0;
    throwOn(ldso_ba_get_counts(ba_, &resInA, &resInL), "ldso_ba_get_counts");
    fs.ef->resInA = resInA; fs.ef->resInL = resInL;

    // host mirrors of what the device computed on its side (:849-851): adjoints, pair precalc, deltas - the reference's own functions
    EFDeltaValid = false; EFAdjointsValid = false;
    fs.ef->setAdjointsF(fs.Hcalib->mpCH);
    fs.setPrecalcValues();

    // :859-869 unchanged: hand the estimated poses to the frames
    {
        unique_lock<mutex> crlock(fs.shellPoseMutex);
        for (auto fr : fs.frames) {
            fr->setPose(fr->frameHessian->PRE_camToWorld.inverse());
            if (fr->kfId >= fs.globalMap->getLatestOptimizedKfId()) fr->setPoseOpti(Sim3(fr->getPose().matrix()));
            fr->aff_g2l = fr->frameHessian->aff_g2l();
        }
    }
    lap(3, tLap);
    return rmse;
}

}  // namespace ldso
