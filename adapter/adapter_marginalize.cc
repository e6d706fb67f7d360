// adapter_marginalize.cc — what follows optimize() in makeKeyFrame: the removal policy, point marginalisation and frame marginalisation on the resident window.
#include "adapter_internal.h"

using namespace ldso::internal;
using namespace ldso::adp;

namespace ldso {

// ------------------------------------------------------------------------------------------------------------------------------------
// void FullSystem::flagPointsForRemoval()                                                                       FullSystem.cc:1208-1270
// The policy, line for line; the inner loop of :1241-1250 (re-linearise and fix the residuals of a point that is marginalised) is what
// ldso_ba_marginalize_points runs on the device for the points flagged here.
// ------------------------------------------------------------------------------------------------------------------------------------
void GpuBackend::flagPointsForRemoval(FullSystem &fs) {
    std::vector<shared_ptr<FrameHessian>> fhsToMargPoints;
    for (int i = 0; i < (int) fs.frames.size(); i++)
        if (fs.frames[i]->frameHessian->flaggedForMarginalization) fhsToMargPoints.push_back(fs.frames[i]->frameHessian);
    for (auto &fr : fs.frames) {
        shared_ptr<FrameHessian> host = fr->frameHessian;
        for (auto &feat : fr->features) {
            if (!(feat->status == Feature::FeatureStatus::VALID && feat->point->status == Point::PointStatus::ACTIVE)) continue;
            shared_ptr<PointHessian> ph = feat->point->mpPH;
            if (ph->idepth_scaled < 0 || ph->residuals.size() == 0) {
                ph->point->status = Point::PointStatus::OUTLIER;
                feat->status = Feature::FeatureStatus::OUTLIER;
            } else if (ph->isOOB(fhsToMargPoints) || host->flaggedForMarginalization) {
                if (ph->isInlierNew()) {
                    // (:1241-1250 happens on the device, see marginalizePoints)
                    if (ph->idepth_hessian > setting_minIdepthH_marg) ph->point->status = Point::PointStatus::MARGINALIZED;
                    else ph->point->status = Point::PointStatus::OUT;
                } else ph->point->status = Point::PointStatus::OUT;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------------------
// void EnergyFunctional::marginalizePointsF()                                                          EnergyFunctional.cc:165-222
// ------------------------------------------------------------------------------------------------------------------------------------
void GpuBackend::marginalizePoints(FullSystem &fs) {
    EnergyFunctional &ef = *fs.ef;
    const int P = (int) window_.points.size();
    if (P == 0) throw std::runtime_error("GpuBackend::marginalizePoints: no window resident (call optimize first)");
    std::vector<int32_t> flags((size_t) P, 0);
    int nMarg = 0;
    for (int k = 0; k < P; k++)
        if (window_.points[k]->point && window_.points[k]->point->status == Point::PointStatus::MARGINALIZED) { flags[k] = 1; nMarg++; }
    const int n = CPARS + 8 * (int) fs.frames.size();
    if ((int) ef.HM.rows() != n) throw std::runtime_error("GpuBackend::marginalizePoints: the prior does not have the window's dimension");
    if (nMarg > 0) {
        // (the settings the device pass reads - margWeightFac, idepthFixPriorMargFac - went up with optimize(); so did ef.HM / ef.bM)
        std::vector<double> HM((size_t) n * n), bM((size_t) n);
        throwOn(ldso_ba_marginalize_points(ba_, flags.data(), HM.data(), bM.data()), "ldso_ba_marginalize_points");
        priorFromRowMajor(ef, n, HM, bM);
    }
    // the reference's bookkeeping around the accumulation (:169-184, :193, :199, :219-220)
    ef.allPointsToMarg.clear();
    for (int k = 0; k < P; k++) {
        if (!flags[k]) continue;
        shared_ptr<PointHessian> p = window_.points[k];
        p->priorF *= setting_idepthFixPriorMargFac;
        for (auto r : p->residuals)
            if (r->isActive()) { ef.connectivityMap[(((uint64_t) r->host.lock()->frameID) << 32) + ((uint64_t) r->target.lock()->frameID)][1]++; ef.resInM++; }
        ef.allPointsToMarg.push_back(p);
    }
    for (auto p : ef.allPointsToMarg) ef.removePoint(p);
    EFIndicesValid = false;
    ef.makeIDX();
}

// ------------------------------------------------------------------------------------------------------------------------------------
// void FullSystem::marginalizeFrame(shared_ptr<Frame> &frame)                                                      FullSystem.cc:602-645
// ------------------------------------------------------------------------------------------------------------------------------------
void GpuBackend::marginalizeFrame(FullSystem &fs, shared_ptr<Frame> &frame) {
    EnergyFunctional &ef = *fs.ef;
    shared_ptr<FrameHessian> fh = frame->frameHessian;
    const int F = (int) fs.frames.size(), n = CPARS + 8 * F, nd = n - 8;
    int col = -1;
    for (int f = 0; f < F; f++) if (fs.frames[f].get() == frame.get()) col = f;
    const bool resident = window_.valid && (int) window_.frames.size() == F && col >= 0 && window_.frames[col].get() == frame.get();
    if (!resident || (int) ef.HM.rows() != n) { margFrameHostFallback++; fs.marginalizeFrame(frame); return; }          // no window of these frames on the device: the reference's member (counted)
    margFrameDevice++;
    // ---- EnergyFunctional::marginalizeFrame: the arithmetic (:80-136) on the device, on ef's own prior ----
    {
        std::vector<double> HM, bM, oH((size_t) nd * nd), ob((size_t) nd);
        priorToRowMajor(ef, n, HM, bM);
        throwOn(ldso_ba_set_prior(ba_, HM.data(), bM.data()), "ldso_ba_set_prior");
        throwOn(ldso_ba_marginalize_frame(ba_, col, oH.data(), ob.data()), "ldso_ba_marginalize_frame");
        ef.HM.resize(nd, nd); ef.bM.resize(nd);
        priorFromRowMajor(ef, nd, oH, ob);
    }
    // ... its bookkeeping (:138-150)
    for (unsigned int i = fh->idx; i + 1 < ef.frames.size(); i++) { ef.frames[i] = ef.frames[i + 1]; ef.frames[i]->idx = i; }
    ef.frames.pop_back();
    ef.nFrames--;
    EFIndicesValid = false; EFAdjointsValid = false; EFDeltaValid = false;
    ef.makeIDX();
    // ---- drop all observations of existing points in that frame (:607-632): column `col` of the resident rows ----
    for (ResidentWindow::Row &row : window_.rows) {
        if (!row.res[col] || row.host == col) continue;
        if (!(row.feat->status == Feature::FeatureStatus::VALID && row.feat->point && row.feat->point->status == Point::PointStatus::ACTIVE)) continue;
        ResidentWindow::dropResidual(row, row.res[col], ef);
    }
    // ---- :634-644 ----
    frame->ReleaseAll();
    ldso::internal::deleteOutOrder<shared_ptr<Frame>>(fs.frames, frame);
    for (unsigned int i = 0; i < fs.frames.size(); i++) fs.frames[i]->frameHessian->idx = i;
    fs.setPrecalcValues();
    ef.setAdjointsF(fs.Hcalib->mpCH);
}

}  // namespace ldso
