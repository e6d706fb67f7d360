// adapter_immature.cc — the immature points: the tracer's row set (GpuBackend::ImmatureRows), its reconcile with the graph, traceNewCoarse, and makeNewTraces
// in both selection modes.
#include "adapter_internal.h"

using namespace ldso::internal;
using namespace ldso::adp;

namespace ldso {

// ---- GpuBackend::ImmatureRows: the only code that changes the row list ----------------------------------------------------------------------------------
GpuBackend::ImmatureRows::~ImmatureRows() { if (tracer) ldso_trace_destroy(tracer); }

void GpuBackend::ImmatureRows::forget() { who_.clear(); host_.clear(); }

void GpuBackend::ImmatureRows::ensure(int device, int need, int minCapacity) {
    if (tracer && need <= cap_) return;
    if (tracer) ldso_trace_destroy(tracer);
    tracer = nullptr;
    forget();                                            // a new tracer starts empty: the rows go with the old one
    cap_ = std::max(need * 2, minCapacity);
    throwOn(ldso_trace_create(device, wG[0], hG[0], cap_, &tracer), "ldso_trace_create");
}

void GpuBackend::ImmatureRows::adopt(std::vector<shared_ptr<ImmaturePoint>> &cur, std::vector<int> &curHost) { who_.swap(cur); host_.swap(curHost); }

void GpuBackend::ImmatureRows::append(const std::vector<shared_ptr<ImmaturePoint>> &fresh, int hostIdx) {
    for (auto &ip : fresh) { who_.push_back(ip); host_.push_back(hostIdx); }
}

void GpuBackend::ImmatureRows::compact(const std::vector<uint8_t> &keep) {
    size_t k = 0;
    for (size_t i = 0; i < who_.size(); i++) if (keep[i]) { who_[k] = who_[i]; host_[k] = host_[i]; k++; }
    who_.resize(k); host_.resize(k);
}

// the device's records into the objects of the rows (alive: only rows i with (*alive)[i] != 0)
void GpuBackend::downloadImmature(const std::vector<char> *alive) {
    if (!imm_.tracer || imm_.size() == 0) return;
    std::vector<ldso_immature_t> rec(imm_.size());
    throwOn(ldso_trace_get_points(imm_.tracer, rec.data()), "ldso_trace_get_points");
    for (size_t i = 0; i < imm_.size(); i++) if (!alive || (*alive)[i]) writeTraceState(*imm_.who()[i], rec[i]);
}

void GpuBackend::syncImmaturePoints(FullSystem &fs) {
    unique_lock<mutex> lock(fs.mapMutex);
    downloadImmature(nullptr);
}

// resident mode: bring the tracer's rows in line with the immature points of the graph (ldso_gpu_adapter.h: the three outcomes; adp::planReconcile decides)
void GpuBackend::reconcileImmature(FullSystem &fs, bool setIdxInImmaturePoints) {
    const int F = (int) fs.frames.size();
    std::vector<shared_ptr<ImmaturePoint>> cur;
    std::vector<int> curHost;
    for (int f = 0; f < F; f++) {
        auto &features = fs.frames[f]->features;
        for (size_t i = 0; i < features.size(); i++) {
            shared_ptr<Feature> &feat = features[i];
            if (!(feat->status == Feature::FeatureStatus::IMMATURE && feat->ip)) continue;
            if (setIdxInImmaturePoints && f != F - 1) feat->ip->idxInImmaturePoints = i;           // :1102
            cur.push_back(feat->ip); curHost.push_back(f);
        }
    }
    ReconcilePlan plan = planReconcile(cur, curHost, imm_.who(), imm_.host(), imm_.tracer != nullptr);
    if (plan.outcome == ReconcilePlan::Same) { immatureReconcile[0]++; return; }
    if (plan.outcome == ReconcilePlan::Compact) {
        imm_.guarded([&] {
            int nLeft = 0;
            throwOn(ldso_trace_compact(imm_.tracer, plan.keep.data(), LDSO_MAX_FRAMES, plan.hostMap, &nLeft), "ldso_trace_compact");
            if (nLeft != (int) cur.size()) throw std::runtime_error("GpuBackend: the tracer's count after the compaction differs from the graph's");
        });
        imm_.adopt(cur, curHost);
        immatureReconcile[1]++;
        return;
    }
    // the host holds points the device has not seen: what the device knows goes into the objects that are still there, then everything goes up
    if (imm_.tracer && imm_.size() > 0) {
        std::vector<ImmaturePoint *> sorted;
        for (auto &p : cur) sorted.push_back(p.get());
        std::sort(sorted.begin(), sorted.end());
        std::vector<char> alive(imm_.size());
        for (size_t i = 0; i < imm_.size(); i++) alive[i] = std::binary_search(sorted.begin(), sorted.end(), imm_.who()[i].get()) ? 1 : 0;
        downloadImmature(&alive);
    }
    imm_.forget();
    immatureReconcile[2]++;
    if (cur.empty()) { if (imm_.tracer) throwOn(ldso_trace_set_points(imm_.tracer, 0, nullptr), "ldso_trace_set_points"); return; }
    imm_.ensure(device_, (int) cur.size(), tracerMinCapacity);
    std::vector<ldso_immature_t> rec(cur.size());
    std::vector<float> types(cur.size());
    for (size_t k = 0; k < cur.size(); k++) { fillRecord(rec[k], *cur[k]->feature, *cur[k], curHost[k]); types[k] = cur[k]->my_type; }
    throwOn(ldso_trace_set_points(imm_.tracer, (int) rec.size(), rec.data()), "ldso_trace_set_points");
    throwOn(ldso_trace_set_point_types(imm_.tracer, types.data()), "ldso_trace_set_point_types");
    imm_.adopt(cur, curHost);
}

// ------------------------------------------------------------------------------------------------------------------------------------
// void FullSystem::traceNewCoarse(shared_ptr<FrameHessian> fh)                                                   FullSystem.cc:1012-1050
// Every immature point of the window's key frames is traced into the new frame by one ldso_trace_on call (one wavefront per point);
// the per-host KRKi / Kt / affine transfer are formed here exactly as the reference forms them (its own Eigen / Sophus expressions).
// ------------------------------------------------------------------------------------------------------------------------------------
void GpuBackend::traceNewCoarse(FullSystem &fs, shared_ptr<FrameHessian> fh) {
    unique_lock<mutex> lock(fs.mapMutex);
    for (int i = 0; i < 6; i++) lastTraceCounts[i] = 0;
    const int F = (int) fs.frames.size();
    std::vector<ldso_immature_t> rec;
    std::vector<ImmaturePoint *> who;
    if (residentImmature) {
        reconcileImmature(fs, false);
        if (imm_.size() == 0) return;
    } else {
        for (int f = 0; f < F; f++)
            for (auto &feat : fs.frames[f]->features) {
                if (!(feat->status == Feature::FeatureStatus::IMMATURE && feat->ip)) continue;
                ldso_immature_t q;
                fillRecord(q, *feat, *feat->ip, f);
                rec.push_back(q); who.push_back(feat->ip.get());
            }
        if (rec.empty()) return;
        imm_.ensure(device_, (int) rec.size(), tracerMinCapacity);
        imm_.forget();                                   // ldso_trace_set_points below replaces whatever rows a resident phase left
    }
    ldso_tracer_t *tracer = imm_.tracer;
    ldso_trace_settings_t ts;
    ldso_trace_settings_default(&ts);
    ts.maxPixSearch = setting_maxPixSearch; ts.trace_stepsize = setting_trace_stepsize; ts.trace_GNThreshold = setting_trace_GNThreshold;
    ts.trace_extraSlackOnTH = setting_trace_extraSlackOnTH; ts.trace_slackInterval = setting_trace_slackInterval;
    ts.trace_minImprovementFactor = setting_trace_minImprovementFactor; ts.huberTH = setting_huberTH;
    ts.trace_GNIterations = setting_trace_GNIterations; ts.minTraceTestRadius = setting_minTraceTestRadius;
    throwOn(ldso_trace_set_settings(tracer, &ts), "ldso_trace_set_settings");
    // :1018-1032, per host frame
    Mat33f K = Mat33f::Identity();
    K(0, 0) = fs.Hcalib->mpCH->fxl(); K(1, 1) = fs.Hcalib->mpCH->fyl(); K(0, 2) = fs.Hcalib->mpCH->cxl(); K(1, 2) = fs.Hcalib->mpCH->cyl();
    std::vector<float> KRKi((size_t) F * 9), Kt((size_t) F * 3), aff((size_t) F * 2);
    for (int f = 0; f < F; f++) {
        shared_ptr<FrameHessian> host = fs.frames[f]->frameHessian;
        SE3 hostToNew = fh->PRE_worldToCam * host->PRE_camToWorld;
        Mat33f M = K * hostToNew.rotationMatrix().cast<float>() * K.inverse();
        Vec3f t = K * hostToNew.translation().cast<float>();
        Vec2f a = AffLight::fromToVecExposure(host->ab_exposure, fh->ab_exposure, host->aff_g2l(), fh->aff_g2l()).cast<float>();
        flatPose(M, t, f, KRKi, Kt);
        aff[(size_t) f * 2] = a[0]; aff[(size_t) f * 2 + 1] = a[1];
    }
    if (!residentImmature) throwOn(ldso_trace_set_points(tracer, (int) rec.size(), rec.data()), "ldso_trace_set_points");
    if (useDevicePyramids && fh->frame) { tracerPyr_ = pyramidOf(fh); throwOn(ldso_trace_set_frame_pyramid(tracer, tracerPyr_->p), "ldso_trace_set_frame_pyramid"); }
    else throwOn(ldso_trace_set_frame(tracer, (const float *) fh->dIp[0]), "ldso_trace_set_frame");
    throwOn(ldso_trace_on(tracer, F, KRKi.data(), Kt.data(), aff.data(), lastTraceCounts), "ldso_trace_on");
    if (residentImmature) return;                      // the records stay where they are: syncImmaturePoints brings them over on demand
    throwOn(ldso_trace_get_points(tracer, rec.data()), "ldso_trace_get_points");
    for (size_t i = 0; i < rec.size(); i++) writeTraceState(*who[i], rec[i]);
}

// ------------------------------------------------------------------------------------------------------------------------------------
// void FullSystem::makeNewTraces(shared_ptr<FrameHessian> newFrame, float *gtDepth), setting_pointSelection == 1 (FullSystem.cc:1272-1283) and 0 (:1284-1304)
// ------------------------------------------------------------------------------------------------------------------------------------
// what either selection mode reports for a frame: one record per point; its my_type (empty: 1 for all); its feature (corner mode only)
struct GpuBackend::NewTraces {
    std::vector<ldso_immature_t> rec;
    std::vector<float> types;
    std::vector<ldso_feature_t> feats;
};

// Resident mode, both selection modes: the records of a key frame go behind the tracer's rows as they lie in device memory (typeDev: their my_type, or null = 1),
// the ones dropped for a non-finite energyTH are compacted away, and the ImmaturePoints kept (`fresh`) join the row list.
void GpuBackend::appendFreshRecords(const NewTraces &nt, const void *immDev, const void *typeDev, int nDev, const std::vector<shared_ptr<ImmaturePoint>> &fresh, int hostIdx) {
    const int n = (int) nt.rec.size(), nRows = (int) imm_.size(), need = nRows + n;
    if (nDev != n) throw std::runtime_error("GpuBackend::makeNewTraces: the device buffer does not hold the records that were reported");
    if (imm_.tracer && need > imm_.capacity() && nRows > 0) {
        // the tracer has to grow: its state goes into the objects, and the next reconcile uploads the whole set (the new objects hold their records already)
        downloadImmature(nullptr);
        imm_.ensure(device_, need, tracerMinCapacity);
        return;
    }
    imm_.ensure(device_, need, tracerMinCapacity);
    imm_.guarded([&] {
        throwOn(ldso_trace_append_points_device(imm_.tracer, n, immDev), "ldso_trace_append_points_device");
        if (typeDev) throwOn(ldso_trace_set_tail_types_device(imm_.tracer, n, typeDev), "ldso_trace_set_tail_types_device");
        if (fresh.size() != nt.rec.size()) {
            std::vector<uint8_t> keep((size_t) need, 1);
            for (int i = 0; i < n; i++) if (!std::isfinite(nt.rec[i].energyTH)) keep[nRows + i] = 0;
            int nLeft = 0;
            throwOn(ldso_trace_compact(imm_.tracer, keep.data(), LDSO_MAX_FRAMES, nullptr, &nLeft), "ldso_trace_compact");
            if (nLeft != nRows + (int) fresh.size()) throw std::runtime_error("GpuBackend::makeNewTraces: the tracer's count after the compaction differs from the points kept");
        }
    });
    imm_.append(fresh, hostIdx);
}

// setting_pointSelection == 1: FeatureDetector::DetectCorners and the ImmaturePoint constructors as one device call.  false: the detector's grid is empty
bool GpuBackend::detectCorners(FullSystem &fs, const shared_ptr<FrameHessian> &newFrame, int hostIdx, NewTraces &out) {
    const int w = wG[0], h = hG[0], want = (int) setting_desiredImmatureDensity;
    int capacity = 0;
    throwOn(ldso_feat_grid(w, h, want, nullptr, nullptr, nullptr, nullptr, nullptr, &capacity), "ldso_feat_grid");
    newFrame->frame->features.reserve(want);                                                         // :1276
    if (capacity == 0) return false;
    if (!features_ || capacity > featuresCap_ || featuresPattern_ != orbPattern) {
        if (features_) ldso_feat_destroy(features_);
        features_ = nullptr;
        featuresCap_ = std::max(capacity, 4096);
        throwOn(ldso_feat_create(device_, w, h, featuresCap_, orbPattern, &features_), "ldso_feat_create");
        featuresPattern_ = orbPattern;
    }
    shared_ptr<CalibHessian> calib = fs.Hcalib ? fs.Hcalib->mpCH : nullptr;
    throwOn(ldso_feat_set_response(features_, setting_gammaWeightsPixelSelect == 1 && calib ? calib->B : nullptr), "ldso_feat_set_response");
    PyrRef pyr = pyramidOf(newFrame);
    int n = 0, nCorners = 0;
    throwOn(ldso_feat_detect(features_, pyr->p, want, hostIdx, &n, &nCorners), "ldso_feat_detect");
    out.feats.resize((size_t) n); out.rec.resize((size_t) n);
    throwOn(ldso_feat_get(features_, out.feats.data(), out.rec.data()), "ldso_feat_get");
    lastNewTraces[1] = nCorners;
    return true;
}

// setting_pointSelection == 0 (FullSystem.cc:1284-1304): PixelSelector::makeMaps, the raster scan of the map and the ImmaturePoint constructors on the device.
// fs.pixelSelector stays the owner of currentPotential: read before the call and written back after it, so host and device calls can alternate.  Nothing of
// the frame is read on the host but the positions and records that come back.
void GpuBackend::selectPixels(FullSystem &fs, const shared_ptr<FrameHessian> &newFrame, int hostIdx, NewTraces &out) {
    const int w = wG[0], h = hG[0];
    if (pixsel_ && (pixselPattern_ != fs.pixelSelector->randomPattern || pixselW_ != w || pixselH_ != h)) { ldso_pixsel_destroy(pixsel_); pixsel_ = nullptr; }
    if (!pixsel_) {                                                                                  // the pattern goes up once per PixelSelector and image size
        throwOn(ldso_pixsel_create(device_, w, h, fs.pixelSelector->randomPattern, &pixsel_), "ldso_pixsel_create");
        pixselPattern_ = fs.pixelSelector->randomPattern; pixselW_ = w; pixselH_ = h;
    }
    shared_ptr<CalibHessian> calib = fs.Hcalib ? fs.Hcalib->mpCH : nullptr;
    throwOn(ldso_pixsel_set_response(pixsel_, setting_gammaWeightsPixelSelect == 1 && calib ? calib->B : nullptr), "ldso_pixsel_set_response");
    throwOn(ldso_pixsel_set_settings(pixsel_, setting_minGradHistCut, setting_minGradHistAdd, setting_gradDownweightPerLevel, setting_selectDirectionDistribution ? 1 : 0), "ldso_pixsel_set_settings");
    throwOn(ldso_pixsel_set_potential(pixsel_, fs.pixelSelector->currentPotential), "ldso_pixsel_set_potential");
    PyrRef pyr = pyramidOf(newFrame);
    fs.pixelSelector->allowFast = true;                                                              // :1286
    int numPointsTotal = 0, n = 0;
    throwOn(ldso_pixsel_make_maps(pixsel_, pyr->p, setting_desiredImmatureDensity, 1, 1.0f, &numPointsTotal, nullptr, nullptr), "ldso_pixsel_make_maps");          // :1287
    throwOn(ldso_pixsel_get_potential(pixsel_, &fs.pixelSelector->currentPotential), "ldso_pixsel_get_potential");
    newFrame->frame->features.reserve(numPointsTotal);                                               // :1288
    const int rc = ldso_pixsel_make_points(pixsel_, pyr->p, hostIdx, &n);
    if (rc != LDSO_E_NONFINITE) throwOn(rc, "ldso_pixsel_make_points");                              // a non-finite colour: those records are dropped by the caller (:1298)
    out.rec.resize((size_t) n); out.types.resize((size_t) n);
    throwOn(ldso_pixsel_get_points(pixsel_, out.rec.data(), out.types.data()), "ldso_pixsel_get_points");
}

// Both modes: reconcile, detect or select on the frame's device pyramid, one Feature + ImmaturePoint per record with a finite energyTH (the reference's
// constructor, then its fields overwritten from the record), and in resident mode the records appended behind the tracer's rows device to device.
void GpuBackend::makeNewTraces(FullSystem &fs, shared_ptr<FrameHessian> newFrame) {
    const bool corners = setting_pointSelection == 1;
    if (!corners && setting_pointSelection != 0) throw std::runtime_error("GpuBackend::makeNewTraces: only setting_pointSelection == 0 (PixelSelector::makeMaps) and 1 (FeatureDetector::DetectCorners) run on the device");
    for (int i = 0; i < 3; i++) lastNewTraces[i] = 0;
    if (!corners && pyrLevelsUsed < 3) throw std::runtime_error("GpuBackend::makeNewTraces: PixelSelector::select reads three pyramid levels");
    const int w = wG[0], h = hG[0];
    shared_ptr<Frame> frame = newFrame->frame;
    if (residentImmature) reconcileImmature(fs, false);                                              // the rows in line with the graph before the new ones follow them
    int hostIdx = (int) fs.frames.size();                                                            // the frame's index in the window (the new key frame is its last)
    for (size_t f = 0; f < fs.frames.size(); f++) if (fs.frames[f] == frame) hostIdx = (int) f;
    NewTraces nt;
    if (corners) { if (!detectCorners(fs, newFrame, hostIdx, nt)) return; } else selectPixels(fs, newFrame, hostIdx, nt);
    const int n = (int) nt.rec.size();
    lastNewTraces[0] = n;
    shared_ptr<CalibHessian> calib = fs.Hcalib ? fs.Hcalib->mpCH : nullptr;
    std::vector<shared_ptr<ImmaturePoint>> fresh;
    for (int i = 0; i < n; i++) {
        const ldso_immature_t &q = nt.rec[i];
        if (!std::isfinite(q.energyTH)) { lastNewTraces[2]++; continue; }                            // as :1298 does
        // the ImmaturePoint constructor samples the host image itself; its sampling stays inside the image (pixel selector: 3 <= x < w - 4 anyway; a corner's
        // position is clamped for the call) and its results are replaced by the device record's
        shared_ptr<Feature> feat;
        shared_ptr<ImmaturePoint> ip;
        if (corners) {                                                                               // uv, score, isCorner, angle, descriptor (:1280-1281)
            const ldso_feature_t &g = nt.feats[i];
            feat.reset(new Feature(g.u, g.v, frame));
            feat->score = g.score; feat->isCorner = g.is_corner != 0; feat->angle = g.angle;
            memcpy(feat->descriptor, g.descriptor, 32);
            feat->uv = Vec2f(std::min(std::max(g.u, 8.0f), (float) w - 9), std::min(std::max(g.v, 8.0f), (float) h - 9));
            ip.reset(new ImmaturePoint(frame, feat, 1, calib));
            feat->uv = Vec2f(g.u, g.v);
        } else {                                                                                     // :1295-1297
            feat.reset(new Feature(q.u, q.v, frame));
            ip.reset(new ImmaturePoint(frame, feat, nt.types[i], calib));
        }
        overwriteFromRecord(*ip, q);
        feat->ip = ip;
        frame->features.push_back(feat);
        fresh.push_back(ip);
    }
    if (!residentImmature || n == 0) return;
    // the records never leave the device: appended behind the tracer's rows as they lie in the detector's / selector's buffer, the dropped ones compacted away
    const void *featDev = nullptr, *immDev = nullptr, *typeDev = nullptr;
    int nDev = 0;
    if (corners) throwOn(ldso_feat_device(features_, &featDev, &immDev, &nDev), "ldso_feat_device");
    else throwOn(ldso_pixsel_device(pixsel_, &immDev, &typeDev, &nDev), "ldso_pixsel_device");
    appendFreshRecords(nt, immDev, typeDev, nDev, fresh, hostIdx);
}

}  // namespace ldso
