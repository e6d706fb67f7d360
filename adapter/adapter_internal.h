// adapter_internal.h — the private header of the drop-in adapter: every unit of libldso_gpu_adapter.so, and the test harness adapter_capi.cc, includes it FIRST.
// It holds the one inclusion of the reference's FullSystem.h / CoarseTracker.h with the access specifiers open (ldso_gpu_adapter.h says why), so every unit of
// a program sees the same class definitions, and the small conversions between LDSO's objects and the records of include/ldso_hip.h that more than one unit
// uses.  The ones that sit in the flatten and the write-back loops (flatPoint, flatResidual, toRaw, fromRaw) are inline HERE so that they stay inlined there.
#pragma once
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <deque>
#include <iostream>
#include <list>
#include <map>
#include <memory>
#include <mutex>
#include <queue>
#include <set>
#include <sstream>
#include <string>
#include <thread>
#include <vector>
#include <unistd.h>

#ifndef LDSO_ADAPTER_OPEN_PRIVATE
#define LDSO_ADAPTER_OPEN_PRIVATE 1      // see ldso_gpu_adapter.h: stands in for `friend class ldso::GpuBackend;` in FullSystem.h / CoarseTracker.h
#endif
#if LDSO_ADAPTER_OPEN_PRIVATE
#include <Eigen/Core>
#include <glog/logging.h>
#define private public
#define protected public
#include "frontend/CoarseTracker.h"
#include "frontend/FullSystem.h"
#undef private
#undef protected
#endif
#include "ldso_gpu_adapter.h"

#include "internal/CalibHessian.h"
#include "internal/FrameHessian.h"
#include "internal/GlobalCalib.h"
#include "internal/GlobalFuncs.h"
#include "internal/ImmaturePoint.h"
#include "internal/OptimizationBackend/EnergyFunctional.h"
#include "internal/PointHessian.h"
#include "internal/Residuals.h"

namespace ldso {
namespace adp {

using namespace ldso::internal;

inline void throwOn(int rc, const char *what) {
    if (rc != LDSO_OK && rc != LDSO_E_NONFINITE) throw std::runtime_error(std::string(what) + ": " + ldso_last_error());
}
inline void toRowMajor34(const SE3 &T, double *m) {
    Eigen::Matrix<double, 3, 4> M = T.matrix3x4();
    for (int i = 0; i < 3; i++) for (int j = 0; j < 4; j++) m[i * 4 + j] = M(i, j);
}
inline SE3 fromRowMajor34(const double *m) {
    Mat33 R; Vec3 t;
    for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) R(i, j) = m[i * 4 + j]; t[i] = m[i * 4 + 3]; }
    return SE3(R, t);
}
inline ldso_calib_t flatCalib(const CalibHessian &c) {
    ldso_calib_t o;
    for (int i = 0; i < 4; i++) { o.value[i] = c.value[i]; o.value_zero[i] = c.value_zero[i]; }
    return o;
}
inline ldso_settings_t flatSettings() {      // the setting_* globals the hot path reads (Settings.h), as the library's ldso_settings_t
    ldso_settings_t s;
    ldso_settings_default(&s);
    s.huberTH = setting_huberTH; s.outlierTHSumComponent = setting_outlierTHSumComponent;
    s.affineOptModeA = setting_affineOptModeA; s.affineOptModeB = setting_affineOptModeB;
    s.frameEnergyTHN = setting_frameEnergyTHN; s.frameEnergyTHFacMedian = setting_frameEnergyTHFacMedian;
    s.frameEnergyTHConstWeight = setting_frameEnergyTHConstWeight; s.overallEnergyTHWeight = setting_overallEnergyTHWeight;
    s.initialCalibHessian = setting_initialCalibHessian; s.margWeightFac = setting_margWeightFac;
    s.idepthFixPriorMargFac = setting_idepthFixPriorMargFac; s.thOptIterations = setting_thOptIterations;
    s.coarseCutoffTH = setting_coarseCutoffTH; s.minOptIterations = setting_minOptIterations;
    s.solverMode = setting_solverMode; s.forceAcceptStep = setting_forceAceptStep ? 1 : 0; s.solverModeDelta = setting_solverModeDelta;
    return s;
}
inline void toRaw(const RawResidualJacobian &J, ldso_rawjac_t &j) {
    for (int i = 0; i < 8; i++) { j.resF[i] = J.resF[i]; j.JIdx[0][i] = J.JIdx[0][i]; j.JIdx[1][i] = J.JIdx[1][i]; j.JabF[0][i] = J.JabF[0][i]; j.JabF[1][i] = J.JabF[1][i]; }
    for (int i = 0; i < 6; i++) { j.Jpdxi[0][i] = J.Jpdxi[0][i]; j.Jpdxi[1][i] = J.Jpdxi[1][i]; }
    for (int i = 0; i < 4; i++) { j.Jpdc[0][i] = J.Jpdc[0][i]; j.Jpdc[1][i] = J.Jpdc[1][i]; }
    j.Jpdd[0] = J.Jpdd[0]; j.Jpdd[1] = J.Jpdd[1];
    for (int a = 0; a < 2; a++) for (int b = 0; b < 2; b++) { j.JIdx2[a * 2 + b] = J.JIdx2(a, b); j.JabJIdx[a * 2 + b] = J.JabJIdx(a, b); j.Jab2[a * 2 + b] = J.Jab2(a, b); }
}
inline void fromRaw(const ldso_rawjac_t &j, RawResidualJacobian &J) {
    for (int i = 0; i < 8; i++) { J.resF[i] = j.resF[i]; J.JIdx[0][i] = j.JIdx[0][i]; J.JIdx[1][i] = j.JIdx[1][i]; J.JabF[0][i] = j.JabF[0][i]; J.JabF[1][i] = j.JabF[1][i]; }
    for (int i = 0; i < 6; i++) { J.Jpdxi[0][i] = j.Jpdxi[0][i]; J.Jpdxi[1][i] = j.Jpdxi[1][i]; }
    for (int i = 0; i < 4; i++) { J.Jpdc[0][i] = j.Jpdc[0][i]; J.Jpdc[1][i] = j.Jpdc[1][i]; }
    J.Jpdd[0] = j.Jpdd[0]; J.Jpdd[1] = j.Jpdd[1];
    for (int a = 0; a < 2; a++) for (int b = 0; b < 2; b++) { J.JIdx2(a, b) = j.JIdx2[a * 2 + b]; J.JabJIdx(a, b) = j.JabJIdx[a * 2 + b]; J.Jab2(a, b) = j.Jab2[a * 2 + b]; }
}

// one point / one residual of the window as ldso_ba_set_window / ldso_ba_update_window take them
inline void flatPoint(const PointHessian &ph, int host, ldso_point_t &p) {
    memset(&p, 0, sizeof(p));
    p.u = ph.u; p.v = ph.v; p.idepth = ph.idepth; p.idepth_zero = ph.idepth_zero; p.priorF = ph.priorF;
    memcpy(p.color, ph.color, sizeof(p.color)); memcpy(p.weights, ph.weights, sizeof(p.weights));
    p.host = host;
}
inline void flatResidual(const PointFrameResidual &r, int point, int host, int target, ldso_residual_t &q) {
    q.point = point; q.host = host; q.target = target; q.state_state = (int32_t) r.state_state;
    q.is_linearized = r.isLinearized ? 1 : 0; q.is_active = r.isActive() ? 1 : 0; q.is_new = r.isNew ? 1 : 0; q.state_energy = (float) r.state_energy;
}

// ---- an ImmaturePoint and its device record ---------------------------------------------------------------------------------------------------------------
inline void fillRecord(ldso_immature_t &q, const Feature &feat, const ImmaturePoint &ip, int host) {
    memset(&q, 0, sizeof(q));
    q.u = feat.uv[0]; q.v = feat.uv[1];
    memcpy(q.color, ip.color, sizeof(q.color)); memcpy(q.weights, ip.weights, sizeof(q.weights));
    q.gradH[0] = ip.gradH(0, 0); q.gradH[1] = ip.gradH(0, 1); q.gradH[2] = ip.gradH(1, 0); q.gradH[3] = ip.gradH(1, 1);
    q.energyTH = ip.energyTH; q.idepth_min = ip.idepth_min; q.idepth_max = ip.idepth_max; q.quality = ip.quality;
    q.lastTraceStatus = (int32_t) ip.lastTraceStatus; q.lastTraceUV[0] = ip.lastTraceUV[0]; q.lastTraceUV[1] = ip.lastTraceUV[1];
    q.lastTracePixelInterval = ip.lastTracePixelInterval; q.host = host;
}
inline void writeTraceState(ImmaturePoint &ip, const ldso_immature_t &q) {          // what ImmaturePoint::traceOn leaves in the object (ImmaturePoint.cc:47-310)
    ip.idepth_min = q.idepth_min; ip.idepth_max = q.idepth_max; ip.quality = q.quality;
    ip.lastTraceStatus = (ImmaturePointStatus) q.lastTraceStatus;
    ip.lastTraceUV = Vec2f(q.lastTraceUV[0], q.lastTraceUV[1]); ip.lastTracePixelInterval = q.lastTracePixelInterval;
}
// what both selection modes of makeNewTraces do with a fresh device record: the fields the reference's constructor computed are replaced by the record's
inline void overwriteFromRecord(ImmaturePoint &ip, const ldso_immature_t &q) {
    memcpy(ip.color, q.color, sizeof(q.color)); memcpy(ip.weights, q.weights, sizeof(q.weights));
    ip.gradH(0, 0) = q.gradH[0]; ip.gradH(0, 1) = q.gradH[1]; ip.gradH(1, 0) = q.gradH[2]; ip.gradH(1, 1) = q.gradH[3];
    ip.energyTH = q.energyTH;
    writeTraceState(ip, q);
}

// ---- EnergyFunctional::HM / bM (Eigen) and the row-major arrays ldso_ba_set_prior / ldso_ba_marginalize_* speak -------------------------------------------
inline void priorToRowMajor(const EnergyFunctional &ef, int n, std::vector<double> &HM, std::vector<double> &bM) {
    HM.resize((size_t) n * n); bM.resize((size_t) n);
    for (int i = 0; i < n; i++) { for (int j = 0; j < n; j++) HM[(size_t) i * n + j] = ef.HM(i, j); bM[i] = ef.bM[i]; }
}
inline void priorFromRowMajor(EnergyFunctional &ef, int n, const std::vector<double> &HM, const std::vector<double> &bM) {          // ef.HM / ef.bM have dimension n
    for (int i = 0; i < n; i++) { for (int j = 0; j < n; j++) ef.HM(i, j) = HM[(size_t) i * n + j]; ef.bM[i] = bM[i]; }
}

// row f of a per-host pose table (F * 9 / F * 3 floats): K R Ki and K t of host f -> the frame the caller projects into, K as the caller's reference code has it
inline void flatPose(const Mat33f &KRKi, const Vec3f &Kt, int f, std::vector<float> &tableKRKi, std::vector<float> &tableKt) {
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) tableKRKi[(size_t) f * 9 + r * 3 + c] = KRKi(r, c); tableKt[(size_t) f * 3 + r] = Kt[r]; }
}

// ---- GpuBackend::reconcileImmature's decision, as a function of plain data (tests/test_immature_reconcile_cpu.py through adp_reconcile_plan) ----------------
// The graph's current list (identity and host index of every immature point, in the graph's order) against the tracer's rows (identity and the host index the
// device record carries):
//   Same      the list equals the rows, host indices included
//   Compact   the list is an ordered subsequence of the rows under ONE map of the host indices: keep[row] = 1 for the rows that stay, hostMap[old] = new
//             host index (-1: no row that stays has that host)
//   Reupload  anything else - no tracer, a point the rows do not hold, another order, one old host under two new ones, an old host index outside the map
// keep and hostMap mean something for Compact only.
struct ReconcilePlan {
    enum Outcome { Same = 0, Compact = 1, Reupload = 2 } outcome = Reupload;
    std::vector<uint8_t> keep;
    int32_t hostMap[LDSO_MAX_FRAMES];
};
template <class Id>
inline ReconcilePlan planReconcile(const std::vector<Id> &cur, const std::vector<int> &curHost, const std::vector<Id> &rows, const std::vector<int> &rowHost, bool haveTracer) {
    ReconcilePlan plan;
    if (!haveTracer) return plan;
    if (cur == rows && curHost == rowHost) { plan.outcome = ReconcilePlan::Same; return plan; }
    const size_t nRows = rows.size();
    if (cur.size() > nRows) return plan;
    plan.keep.assign(nRows, 0);
    for (int f = 0; f < LDSO_MAX_FRAMES; f++) plan.hostMap[f] = -1;
    size_t row = 0;
    for (size_t k = 0; k < cur.size(); k++) {
        while (row < nRows && !(rows[row] == cur[k])) row++;
        if (row == nRows) return plan;
        const int oldHost = rowHost[row];
        if (oldHost < 0 || oldHost >= LDSO_MAX_FRAMES || (plan.hostMap[oldHost] >= 0 && plan.hostMap[oldHost] != curHost[k])) return plan;
        plan.hostMap[oldHost] = curHost[k];
        plan.keep[row++] = 1;
    }
    plan.outcome = ReconcilePlan::Compact;
    return plan;
}

}  // namespace adp
}  // namespace ldso
