// adapter_activate.cc — point activation: the optimizeImmaturePoint calls alone (activatePoints) and the whole of FullSystem::activatePointsMT.
#include "adapter_internal.h"

using namespace ldso::internal;
using namespace ldso::adp;

namespace ldso {

// ------------------------------------------------------------------------------------------------------------------------------------
// Point activation: the optimizeImmaturePoint calls of FullSystem::activatePointsMT_Reductor (:1196-1206) as one device call, then the
// object construction of optimizeImmaturePoint's tail (:977-1008) on the host.
// ------------------------------------------------------------------------------------------------------------------------------------
void GpuBackend::activatePoints(FullSystem &fs, std::vector<shared_ptr<ImmaturePoint>> &toOptimize, std::vector<shared_ptr<PointHessian>> &optimized) {
    optimized.assign(toOptimize.size(), nullptr);
    if (toOptimize.empty()) return;
    std::vector<shared_ptr<PointHessian>> allPoints;
    if (uploadWindow(fs, allPoints) == 0) throw std::runtime_error("GpuBackend::activatePoints: the window holds no active point yet (activate on the host)");
    std::vector<ldso_immature_t> in(toOptimize.size());
    for (size_t k = 0; k < toOptimize.size(); k++) {
        const ImmaturePoint &ip = *toOptimize[k];
        fillRecord(in[k], *ip.feature, ip, ip.feature->host.lock()->frameHessian->idx);
    }
    std::vector<ldso_activation_t> out(toOptimize.size());
    throwOn(ldso_ba_activate_points(ba_, (int) in.size(), in.data(), /*minObs*/ 1, setting_minIdepthH_act, setting_GNItsOnPointActivation, out.data()), "ldso_ba_activate_points");
    for (size_t k = 0; k < toOptimize.size(); k++) optimized[k] = makePoint(fs, toOptimize[k], out[k]);
}

// the tail of FullSystem::optimizeImmaturePoint (:977-1008) from the device's record: the new PointHessian with its residuals, or nullptr
shared_ptr<PointHessian> GpuBackend::makePoint(FullSystem &fs, const shared_ptr<ImmaturePoint> &point, const ldso_activation_t &out) {
    if (!out.ok) return nullptr;                                                                 // return 0 / nullptr (:924-926, :945-947, :968-975)
    const int F = (int) fs.frames.size();
    point->feature->CreateFromImmature();                                                        // :977
    shared_ptr<PointHessian> p = point->feature->point->mpPH;
    p->lastResiduals[0].first = nullptr; p->lastResiduals[0].second = ResState::OOB;
    p->lastResiduals[1].first = nullptr; p->lastResiduals[1].second = ResState::OOB;
    p->setIdepthZero(out.idepth); p->setIdepth(out.idepth);
    shared_ptr<FrameHessian> host = point->feature->host.lock()->frameHessian;
    for (int t = 0; t < F; t++) {
        if (out.res_state[t] != 0) continue;                                                     // ResState::IN only (:989)
        shared_ptr<FrameHessian> target = fs.frames[t]->frameHessian;
        shared_ptr<PointFrameResidual> r(new PointFrameResidual(p, host, target));
        r->state_NewEnergy = r->state_energy = 0; r->state_NewState = ResState::OUTLIER; r->setState(ResState::IN);
        p->residuals.push_back(r);
        if (target == fs.frames.back()->frameHessian) { p->lastResiduals[0].first = r; p->lastResiduals[0].second = ResState::IN; }
        else if (target == (fs.frames.size() < 2 ? nullptr : fs.frames[fs.frames.size() - 2]->frameHessian)) { p->lastResiduals[1].first = r; p->lastResiduals[1].second = ResState::IN; }
    }
    return p;
}

// ------------------------------------------------------------------------------------------------------------------------------------
// void FullSystem::activatePointsMT()                                                                            FullSystem.cc:1052-1189
// gatherSelection: what the member reads from the object graph, flattened in its own iteration order - the seeds of makeDistanceMap (CoarseTracker.cc:699-717),
// the immature points of :1088-1102 (idxInImmaturePoints set as there), the per-host K[1] R Ki[0] / K[1] t of :1092-1094 by the reference's own expressions
// (after coarseDistanceMap->makeK, :1081) and the hosts' flaggedForMarginalization.
// ------------------------------------------------------------------------------------------------------------------------------------
void GpuBackend::selectionPoses(FullSystem &fs, SelectionInputs &in) {
    const int F = (int) fs.frames.size();
    in.KRKi.assign((size_t) F * 9, 0.0f); in.Kt.assign((size_t) F * 3, 0.0f); in.flagged.assign(F, 0);
    fs.coarseDistanceMap->makeK(fs.Hcalib->mpCH);
    shared_ptr<FrameHessian> newest = fs.frames.back()->frameHessian;
    for (int f = 0; f < F; f++) {
        shared_ptr<FrameHessian> host = fs.frames[f]->frameHessian;
        in.flagged[f] = host->flaggedForMarginalization ? 1 : 0;
        if (host == newest) continue;
        SE3 fhToNew = newest->PRE_worldToCam * host->PRE_camToWorld;
        Mat33f KRKi = (fs.coarseDistanceMap->K[1] * fhToNew.rotationMatrix().cast<float>() * fs.coarseDistanceMap->Ki[0]);
        Vec3f Kt = (fs.coarseDistanceMap->K[1] * fhToNew.translation().cast<float>());
        flatPose(KRKi, Kt, f, in.KRKi, in.Kt);
    }
}

void GpuBackend::gatherSelection(FullSystem &fs, SelectionInputs &in) {
    in.seeds.clear(); in.cand.clear(); in.myType.clear(); in.who.clear();
    const int F = (int) fs.frames.size();
    selectionPoses(fs, in);
    shared_ptr<FrameHessian> newest = fs.frames.back()->frameHessian;
    for (int f = 0; f < F; f++) {
        shared_ptr<FrameHessian> host = fs.frames[f]->frameHessian;
        if (host == newest) continue;
        for (auto &feat : host->frame->features)
            if (feat->point && feat->point->status == Point::PointStatus::ACTIVE) {
                auto ph = feat->point->mpPH;
                ldso_act_seed_t s; s.u = ph->u; s.v = ph->v; s.idepth_scaled = ph->idepth_scaled; s.host = f;
                in.seeds.push_back(s);
            }
    }
    for (int f = 0; f < F; f++) {
        shared_ptr<FrameHessian> host = fs.frames[f]->frameHessian;
        if (host == newest) continue;
        for (size_t i = 0; i < host->frame->features.size(); i++) {
            shared_ptr<Feature> &feat = host->frame->features[i];
            if (!(feat->status == Feature::FeatureStatus::IMMATURE && feat->ip)) continue;
            feat->ip->idxInImmaturePoints = i;                                                   // :1102
            ldso_immature_t q;
            fillRecord(q, *feat, *feat->ip, f);
            in.cand.push_back(q); in.myType.push_back(feat->ip->my_type); in.who.push_back(feat->ip);
        }
    }
}

// the host side of activatePointsMT's decisions: status hand-over of the deleted candidates, object hand-over of the new points (lastSelection[2] counts them)
void GpuBackend::handOverSelection(FullSystem &fs, const std::vector<shared_ptr<ImmaturePoint>> &who, const std::vector<int32_t> &decision, const std::vector<int32_t> &selected, int nSel,
                                   const std::vector<ldso_activation_t> &out) {
    const int n = (int) decision.size();
    // :1105-1108, :1121-1125, :1145-1148 the candidates the loop deletes
    for (int i = 0; i < n; i++)
        if (decision[i] == LDSO_ACT_DROP) {
            shared_ptr<Feature> feat = who[i]->feature;
            feat->status = Feature::FeatureStatus::OUTLIER;
            feat->ReleaseImmature();
        }
    // :1166-1188 the selected ones
    for (int k = 0; k < nSel; k++) {
        shared_ptr<ImmaturePoint> ph = who[selected[k]];
        shared_ptr<PointHessian> newpoint = makePoint(fs, ph, out[k]);
        shared_ptr<Feature> feat = ph->feature;
        if (newpoint != nullptr) {
            feat->status = Feature::FeatureStatus::VALID;
            feat->point->mpPH = newpoint;
            feat->ReleaseImmature();
            newpoint->takeData();
            for (auto r : newpoint->residuals) fs.ef->insertResidual(r);
            lastSelection[2]++;
        } else {
            feat->status = Feature::FeatureStatus::OUTLIER;
            feat->ReleaseImmature();
        }
    }
}

void GpuBackend::activatePointsMT(FullSystem &fs) {
    // :1054-1073 the density controller
    throwOn(ldso_act_update_min_dist(fs.currentMinActDist, fs.ef->nPoints, setting_desiredPointDensity, &fs.currentMinActDist), "ldso_act_update_min_dist");
    // :1075-1102 what the selection reads
    SelectionInputs in;
    std::vector<int32_t> decision, selected;
    std::vector<ldso_activation_t> out;
    int n = 0, nSel = 0;
    lastSelection[0] = lastSelection[1] = lastSelection[2] = 0;
    if (residentImmature) {
        // the candidates are the tracer's rows, the seeds the resident window's points: only the poses and flags are gathered, nothing of the set goes up
        reconcileImmature(fs, true);
        const int F = (int) fs.frames.size();
        n = (int) imm_.size();
        for (int i = 0; i < n; i++) if (imm_.host()[i] != F - 1) lastSelection[0]++;
        if (lastSelection[0] == 0) return;
        selectionPoses(fs, in);
        std::vector<shared_ptr<PointHessian>> allPoints;
        if (uploadWindow(fs, allPoints) == 0) throw std::runtime_error("GpuBackend::activatePointsMT: the window holds no active point yet (activate on the host)");
        decision.resize(n); selected.resize(n); out.resize(n);
        int nLeft = 0;
        imm_.guarded([&] {          // the tracer may or may not have compacted when the call fails
            throwOn(ldso_ba_select_activate_tracer(ba_, imm_.tracer, F, in.KRKi.data(), in.Kt.data(), in.flagged.data(), fs.currentMinActDist, setting_minTraceQuality, /*minObs*/ 1,
                                                   setting_minIdepthH_act, setting_GNItsOnPointActivation, /*compact*/ 1, decision.data(), selected.data(), &nSel, out.data(), &nLeft),
                    "ldso_ba_select_activate_tracer");
        });
        in.who = imm_.who();
        // the rows the device kept: the same decisions compact the host's view of them
        std::vector<uint8_t> keep((size_t) n);
        for (int i = 0; i < n; i++) keep[i] = decision[i] == LDSO_ACT_KEEP;
        imm_.compact(keep);
        if ((int) imm_.size() != nLeft) { imm_.forget(); throw std::runtime_error("GpuBackend::activatePointsMT: the tracer's count after the compaction differs from the decisions'"); }
    } else {
        gatherSelection(fs, in);
        lastSelection[0] = (int) in.cand.size();
        if (in.cand.empty()) return;
        std::vector<shared_ptr<PointHessian>> allPoints;
        if (uploadWindow(fs, allPoints) == 0) throw std::runtime_error("GpuBackend::activatePointsMT: the window holds no active point yet (activate on the host)");
        // :1080-1164 distance map, selection and optimizeImmaturePoint of the selected points: one enqueue, one wait
        n = (int) in.cand.size();
        decision.resize(n); selected.resize(n); out.resize(n);
        throwOn(ldso_ba_select_activate_points(ba_, (int) in.seeds.size(), in.seeds.data(), n, in.cand.data(), in.myType.data(), (int) fs.frames.size(), in.KRKi.data(), in.Kt.data(),
                                               in.flagged.data(), fs.currentMinActDist, setting_minTraceQuality, /*minObs*/ 1, setting_minIdepthH_act, setting_GNItsOnPointActivation,
                                               decision.data(), selected.data(), &nSel, out.data()), "ldso_ba_select_activate_points");
    }
    lastSelection[1] = nSel;
    handOverSelection(fs, in.who, decision, selected, nSel, out);
}

}  // namespace ldso
