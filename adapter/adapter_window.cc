// adapter_window.cc — the window's way to the device, and the resident window's host view (GpuBackend::ResidentWindow).
#include "adapter_internal.h"

using namespace ldso::internal;
using namespace ldso::adp;

namespace ldso {

// ---- GpuBackend::ResidentWindow ------------------------------------------------------------------------------------------------------------------------
bool GpuBackend::ResidentWindow::buildRow(Row &row, PointHessian &ph, Feature *feat, int host, int F, Columns how) {
    row = Row::empty(&ph, feat, host);
    for (shared_ptr<PointFrameResidual> &r : ph.residuals) {
        int t;
        if (how == Columns::FromTargetNotLinearized) {
            const shared_ptr<FrameHessian> target = r->target.lock();          // FrameHessian::idx = window position (uploadWindow sets it)
            t = (r->isLinearized || !target) ? -1 : target->idx;
        } else {
            // makeIDX (EnergyFunctional.cc:380-401): LDSO's own flow reaches optimize() with valid indices (two weak_ptr::lock() per residual are two
            // atomic read-modify-write pairs, 24 000 of them a quarter of the flatten at C3)
            r->hostIDX = host;
            if (how == Columns::FromTarget) r->targetIDX = r->target.lock()->idx;
            t = r->targetIDX;
        }
        if (t < 0 || t >= F || t == host || ((row.mask >> t) & 1u)) return false;
        row.mask |= 1u << t; row.res[t] = r.get();
    }
    return true;
}

void GpuBackend::ResidentWindow::rebuildFlat(int F) {
    flat.clear(); resBegin.assign(1, 0);
    for (const Row &r : rows) {
        for (int t = 0; t < F; t++) if ((r.mask >> t) & 1u) flat.push_back(r.res[t]);
        resBegin.push_back((int32_t) flat.size());
    }
}

void GpuBackend::ResidentWindow::dropResidual(Row &row, const PointFrameResidual *res, EnergyFunctional &ef) {
    PointHessian &ph = *row.ph;
    shared_ptr<PointFrameResidual> r;
    for (shared_ptr<PointFrameResidual> &q : ph.residuals) if (q.get() == res) { r = q; break; }
    if (!r) return;
    if (ph.lastResiduals[0].first == r) ph.lastResiduals[0].first = nullptr;
    else if (ph.lastResiduals[1].first == r) ph.lastResiduals[1].first = nullptr;
    ef.dropResidual(r);                                                                           // EnergyFunctional.cc:44-56
    for (int t = 0; t < kMaxCols; t++) if (row.res[t] == res) { row.res[t] = nullptr; row.mask &= ~(1u << t); }
}

// ------------------------------------------------------------------------------------------------------------------------------------
// Flatten the window in the reference's own orders: frames = FullSystem::frames (= EnergyFunctional::frames, idx = position), points in
// the order of EnergyFunctional::makeIDX (EnergyFunctional.cc:380-401: frames, then the host frame's features), residuals in
// PointHessian::residuals order; a residual's slot is (hostIDX, targetIDX).  allPoints / flat give the write-back its objects.
// ------------------------------------------------------------------------------------------------------------------------------------
// The whole window from the objects (the first optimize() of a handle, windows with linearised residuals, after invalidateWindow(), or when the delta path below
// gave up).  Residuals of a point go over target-ascending: the flat order ldso_ba_update_window keeps, so that both paths describe the same window.
void GpuBackend::uploadFresh(FullSystem &fs, const std::vector<int32_t> &slots, std::vector<shared_ptr<PointHessian>> &allPoints, bool trustIndices) {
    const int F = (int) fs.frames.size();
    allPoints.clear(); window_.flat.clear(); window_.rows.clear();
    window_.resBegin.assign(1, 0);
    std::vector<ldso_point_t> P; std::vector<ldso_residual_t> R; std::vector<ldso_rawjac_t> LJ; std::vector<float> RTZ, mrb; std::vector<int32_t> ngr;
    P.reserve(4096); R.reserve(32768); window_.flat.reserve(32768); window_.rows.reserve(4096);
    // linearised residuals (none in LDSO's own flow: flagPointsForRemoval clears isLinearized, FullSystem.cc:1243) carry their Jacobian and
    // res_toZeroF across; the 296-byte records are only built from the first one on (the residuals in front of it get empty ones then)
    bool anyLin = false;
    for (int f = 0; f < F; f++)
        for (shared_ptr<Feature> &feat : fs.frames[f]->features) {
            if (!(feat->status == Feature::FeatureStatus::VALID && feat->point && feat->point->status == Point::PointStatus::ACTIVE)) continue;
            shared_ptr<PointHessian> ph = feat->point->mpPH;
            ldso_point_t p;
            flatPoint(*ph, f, p);
            p.res_begin = (int32_t) R.size(); p.res_count = (int32_t) ph->residuals.size();
            // PRECONDITION of trustIndices: ef->makeIDX() ran after the last insertResidual (makeKeyFrame does, FullSystem.cc:474) - insertResidual does not
            // clear EFIndicesValid, so a caller that adds residuals and skips makeIDX would hand over stale / zero target indices.  Fresh residuals are appended:
            // the NEWEST residual of the point is checked against the frame it names (one weak_ptr::lock per point, not per residual); a mismatch derives the
            // indices of this point the slow way
            bool trust = trustIndices && EFIndicesValid;
            if (trust && !ph->residuals.empty()) {
                const PointFrameResidual &rl = *ph->residuals.back();
                trust = rl.targetIDX >= 0 && rl.targetIDX < F && fs.frames[rl.targetIDX]->frameHessian.get() == rl.target.lock().get();
            }
            ResidentWindow::Row row;
            if (!ResidentWindow::buildRow(row, *ph, feat.get(), f, F, trust ? ResidentWindow::Columns::Stored : ResidentWindow::Columns::FromTarget))
                throw std::runtime_error("GpuBackend: a residual names a frame outside the window, its host, or a target twice");
            for (int t = 0; t < F; t++) {
                if (!((row.mask >> t) & 1u)) continue;
                PointFrameResidual &r = *row.res[t];
                ldso_residual_t q;
                flatResidual(r, (int32_t) P.size(), f, t, q);
                if (r.isLinearized && !anyLin) { anyLin = true; LJ.resize(R.size()); RTZ.resize(R.size() * 8, 0.0f); for (auto &j : LJ) memset(&j, 0, sizeof(j)); }
                R.push_back(q); window_.flat.push_back(&r);
                if (anyLin) {
                    ldso_rawjac_t j;
                    memset(&j, 0, sizeof(j));
                    if (r.isLinearized) toRaw(*r.J, j);
                    LJ.push_back(j);
                    for (int k = 0; k < 8; k++) RTZ.push_back(r.isLinearized ? r.res_toZeroF[k] : 0.0f);
                }
            }
            P.push_back(p); allPoints.push_back(ph); window_.rows.push_back(row);
            mrb.push_back(ph->maxRelBaseline); ngr.push_back(ph->numGoodResiduals);
            window_.resBegin.push_back((int32_t) R.size());
        }
    if (P.empty()) return;
    lastUploadSeconds[1] += lapSince();
    throwOn(ldso_ba_set_window(ba_, F, slots.data(), (int) P.size(), P.data(), (int) R.size(), R.data(), anyLin ? LJ.data() : nullptr, anyLin ? RTZ.data() : nullptr), "ldso_ba_set_window");
    lastUploadSeconds[2] += lapSince();
    throwOn(ldso_ba_set_point_stats(ba_, mrb.data(), ngr.data()), "ldso_ba_set_point_stats");
    lastUploadSeconds[3] += lapSince();
    window_.valid = !anyLin;                                        // ldso_ba_update_window does not carry linearised residuals: the next call uploads in full again
    if (anyLin) uploadsFreshBecauseLinearized++;                     // (counted: in LDSO's own flow isLinearized is never set - FullSystem.cc:1241-1250 fixes and marginalises in one go)
}

// The window as a delta against the one the last optimize() left on the device (ldso_ba_update_window).  Surviving points are recognised by walking the new
// window (frames, then the host frame's features: makeIDX order) against the rows of the resident one - both in the same stable order, so one pass with two
// cursors; a row is skipped when its point is gone (host frame left, point no longer ACTIVE).  Returns false when the resident window cannot express the new
// one (linearised residuals, an inconsistency): the caller uploads everything.
bool GpuBackend::uploadDelta(FullSystem &fs, const std::vector<int32_t> &slots, std::vector<shared_ptr<PointHessian>> &allPoints) {
    const int F = (int) fs.frames.size(), oF = (int) window_.frames.size();
    if (F > ResidentWindow::kMaxCols || oF > ResidentWindow::kMaxCols || window_.rows.empty()) return false;
    int32_t frameFrom[ResidentWindow::kMaxCols], oldToNew[ResidentWindow::kMaxCols];
    for (int c = 0; c < ResidentWindow::kMaxCols; c++) { frameFrom[c] = -1; oldToNew[c] = -1; }
    int lastOld = -1, nInserted = 0;
    for (int f = 0; f < F; f++) {
        for (int o = 0; o < oF; o++) if (window_.frames[o].get() == fs.frames[f].get()) frameFrom[f] = o;          // identity, not Frame::id: another object graph may reuse the ids
        if (frameFrom[f] >= 0) { if (frameFrom[f] <= lastOld) return false; lastOld = frameFrom[f]; oldToNew[frameFrom[f]] = f; } else nInserted++;
    }
    if (nInserted == F) return false;          // nothing of the resident window is left
    const size_t oP = window_.rows.size();
    auto alive = [&](const ResidentWindow::Row &r) {          // the frame first: features of a frame that left the window may be gone with it
        return oldToNew[r.host] >= 0 && r.feat->status == Feature::FeatureStatus::VALID && r.feat->point && r.feat->point->status == Point::PointStatus::ACTIVE
               && r.feat->point->mpPH.get() == r.ph;
    };
    std::vector<ResidentWindow::Row> rows; rows.reserve(oP + 512);
    std::vector<int32_t> pointFrom; pointFrom.reserve(oP + 512);
    std::vector<uint32_t> mask; mask.reserve(oP + 512);
    std::vector<shared_ptr<PointHessian>> pts; pts.reserve(oP + 512);
    std::vector<ldso_point_t> fresh; std::vector<ldso_residual_t> freshRes; std::vector<float> fmrb; std::vector<int32_t> fngr;
    size_t j = 0;
    auto columnOf = [&](const PointFrameResidual &r) { const shared_ptr<FrameHessian> t = r.target.lock(); return t ? t->idx : -1; };      // FrameHessian::idx = window position (set above)
    for (int f = 0; f < F; f++)
        for (shared_ptr<Feature> &feat : fs.frames[f]->features) {
            if (!(feat->status == Feature::FeatureStatus::VALID && feat->point && feat->point->status == Point::PointStatus::ACTIVE)) continue;
            PointHessian *ph = feat->point->mpPH.get();
            while (j < oP && window_.rows[j].ph != ph && !alive(window_.rows[j])) j++;
            ResidentWindow::Row n = ResidentWindow::Row::empty(ph, feat.get(), f);
            const int have = (int) ph->residuals.size();
            auto reread = [&]() { return ResidentWindow::buildRow(n, *ph, feat.get(), f, F, ResidentWindow::Columns::FromTargetNotLinearized); };          // the point's residual list from the objects
            if (j < oP && window_.rows[j].ph == ph) {
                // ---- a point of the resident window: its residuals by column, minus the frames that left, plus what was appended since ----
                const ResidentWindow::Row &o = window_.rows[j];
                if (oldToNew[o.host] != f) return false;
                for (int c = 0; c < oF; c++)
                    if (((o.mask >> c) & 1u) && oldToNew[c] >= 0) { n.mask |= 1u << oldToNew[c]; n.res[oldToNew[c]] = o.res[c]; }
                int cnt = __builtin_popcount(n.mask);
                // (a point that got NO residual for a frame inserted since - LDSO gives every active point one, FullSystem.cc:447-470 - may as well have lost one
                // and gained one: equal counts prove nothing then, its list is re-read)
                bool ok = have >= cnt && have - cnt <= nInserted && !(nInserted > 0 && have == cnt);
                for (int k = cnt; ok && k < have; k++) {          // insertResidual appends (FullSystem.cc:447-470): the new ones are the last
                    PointFrameResidual &r = *ph->residuals[k];
                    const int t = columnOf(r);
                    ok = !r.isLinearized && t >= 0 && t < F && t != f && frameFrom[t] < 0 && !((n.mask >> t) & 1u);
                    if (ok) { n.mask |= 1u << t; n.res[t] = &r; }
                }
                // every residual of the point's CURRENT list must be one of the pointers cached above, and every cached pointer must still be in the list: a host
                // that dropped a residual and created another one for the same target between two optimize() calls (equal counts, nothing inserted) would
                // otherwise leave a dangling PointFrameResidual* in the flat list (round-5 advisor).  targetIDX is the hint (makeIDX keeps it current in LDSO's own
                // flow: one compare per residual), the scan over the row is the fallback.
                if (ok) {
                    uint32_t seen = 0;
                    for (int k = 0; ok && k < have; k++) {
                        const PointFrameResidual *r = ph->residuals[k].get();
                        int c = r->targetIDX;
                        if (!(c >= 0 && c < F && n.res[c] == r)) { c = -1; for (int t = 0; t < F; t++) if (n.res[t] == r) { c = t; break; } }
                        if (c < 0 || ((seen >> c) & 1u)) ok = false; else seen |= 1u << c;
                    }
                    ok = ok && seen == n.mask;
                    if (!ok) residentPointerMismatches++;
                }
                if (!ok && !reread()) return false;
                pointFrom.push_back((int32_t) j);
                pts.push_back(window_.points[j]);
                j++;
            } else {
                // ---- a fresh point (activated since the last optimize()): its records cross PCIe ----
                if (!reread()) return false;
                const int k = (int) fresh.size();
                ldso_point_t p;
                flatPoint(*ph, f, p);
                p.res_begin = (int32_t) freshRes.size(); p.res_count = have;
                fresh.push_back(p); fmrb.push_back(ph->maxRelBaseline); fngr.push_back(ph->numGoodResiduals);
                for (int t = 0; t < F; t++) if ((n.mask >> t) & 1u) { ldso_residual_t q; flatResidual(*n.res[t], k, f, t, q); freshRes.push_back(q); }
                pointFrom.push_back(-1 - k);
                pts.push_back(feat->point->mpPH);
            }
            rows.push_back(n); mask.push_back(n.mask);
        }
    for (; j < oP; j++) if (alive(window_.rows[j])) return false;          // a point of the resident window that the walk did not meet
    if (rows.empty()) return false;
    lastUploadSeconds[1] += lapSince();
    const int rc = ldso_ba_update_window(ba_, F, slots.data(), frameFrom, (int) rows.size(), pointFrom.data(), mask.data(), (int) fresh.size(), fresh.data(), (int) freshRes.size(),
                                         freshRes.data(), fmrb.data(), fngr.data());
    lastUploadSeconds[2] += lapSince();
    if (rc != LDSO_OK) { LOG(WARNING) << "GpuBackend: ldso_ba_update_window refused the delta (" << ldso_last_error() << "), uploading the whole window"; return false; }
    window_.rows.swap(rows); allPoints.swap(pts);
    window_.rebuildFlat(F);
    return true;
}

int GpuBackend::uploadWindow(FullSystem &fs, std::vector<shared_ptr<PointHessian>> &allPoints, bool trustIndices) {
    lapSince();
    for (double &t : lastUploadSeconds) t = 0;
    const ldso_settings_t st = flatSettings();
    throwOn(ldso_ba_set_settings(ba_, &st), "ldso_ba_set_settings");
    std::vector<int32_t> slots;
    syncImageSlots(fs, slots);
    lastUploadSeconds[0] += lapSince();
    const int F = (int) fs.frames.size();
    std::vector<ldso_frame_t> Fv((size_t) F);
    for (int f = 0; f < F; f++) {
        FrameHessian &fh = *fs.frames[f]->frameHessian;
        fh.idx = f;
        ldso_frame_t &o = Fv[f];
        memset(&o, 0, sizeof(o));
        toRowMajor34(fh.get_worldToCam_evalPT(), o.worldToCam_evalPT);
        for (int i = 0; i < 10; i++) { o.state[i] = fh.get_state()[i]; o.state_zero[i] = fh.get_state_zero()[i]; }
        for (int i = 0; i < 8; i++) o.prior[i] = fh.prior[i];                                      // FrameHessian::takeData (FrameHessian.cc:115)
        for (int r = 0; r < 6; r++) for (int c = 0; c < 6; c++) o.nullspaces_pose[r * 6 + c] = fh.nullspaces_pose(r, c);
        for (int r = 0; r < 6; r++) o.nullspaces_scale[r] = fh.nullspaces_scale[r];
        for (int r = 0; r < 4; r++) for (int c = 0; c < 2; c++) o.nullspaces_affine[r * 2 + c] = fh.nullspaces_affine(r, c);
        o.ab_exposure = fh.ab_exposure; o.frameEnergyTH = fh.frameEnergyTH; o.frameID = (int32_t) fh.frame->id;   // getPrior keys on frame->id == 0
    }
    lastUploadWasDelta = residentWindow && window_.valid && uploadDelta(fs, slots, allPoints);
    if (!lastUploadWasDelta) { window_.valid = false; uploadFresh(fs, slots, allPoints, trustIndices); }
    (lastUploadWasDelta ? uploadsDelta : uploadsFresh)++;
    if (allPoints.empty()) { window_.valid = false; return 0; }
    window_.frames.assign(fs.frames.begin(), fs.frames.end());
    window_.points = allPoints;                                         // keeps the rows' PointHessian objects alive while the window is resident
    lapSince();
    const ldso_calib_t c = flatCalib(*fs.Hcalib->mpCH);
    throwOn(ldso_ba_set_frames(ba_, Fv.data(), &c), "ldso_ba_set_frames");                      // setAdjointsF + setPrecalcValues on the device
    lastUploadSeconds[4] += lapSince();
    const int n = CPARS + 8 * F;
    if ((int) fs.ef->HM.rows() == n) {
        std::vector<double> HM, bM;
        priorToRowMajor(*fs.ef, n, HM, bM);
        throwOn(ldso_ba_set_prior(ba_, HM.data(), bM.data()), "ldso_ba_set_prior");
    }
    lastUploadSeconds[5] += lapSince();
    return (int) allPoints.size();
}

}  // namespace ldso
