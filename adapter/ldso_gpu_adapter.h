// ldso_gpu_adapter.h — the host-side drop-in: LDSO's own types in, libldso_hip.so (include/ldso_hip.h, C-ABI) underneath.
//
// This is the code INTEGRATION.md describes, as a real translation unit against the reference's headers
// (include/frontend/FullSystem.h, include/frontend/CoarseTracker.h, include/internal/*.h): every function below is the new BODY of the
// reference member function it names.  Nothing of LDSO's object graph changes: Frame / Feature / Point / FrameHessian / PointHessian /
// PointFrameResidual / CalibHessian / EnergyFunctional stay the owners of all state; the library owns device memory only.
//
//   GpuBackend::optimize(fs, n)                     float FullSystem::optimize(int mnumOptIts)                      FullSystem.cc:725-864
//   GpuBackend::makeK / setCoarseTrackingRef        CoarseTracker::makeK / setCoarseTrackingRef                     CoarseTracker.cc:219-256
//   GpuBackend::trackNewestCoarse                   bool CoarseTracker::trackNewestCoarse(...)                      CoarseTracker.cc:61-217
//   GpuBackend::trackNewCoarse(fs, fh)              Vec4 FullSystem::trackNewCoarse(shared_ptr<FrameHessian>)       FullSystem.cc:179-386
//   GpuBackend::activatePoints(fs, ...)             the optimizeImmaturePoint loop of activatePointsMT              FullSystem.cc:892-1010,1196-1206
//   GpuBackend::activatePointsMT(fs)                void FullSystem::activatePointsMT() with CoarseDistanceMap      FullSystem.cc:1052-1189, CoarseTracker.cc:686-818
//   GpuBackend::traceNewCoarse(fs, fh)              void FullSystem::traceNewCoarse(shared_ptr<FrameHessian>)       FullSystem.cc:1012-1050
//   GpuBackend::makeNewTraces(fs, fh)               void FullSystem::makeNewTraces(fh, gtDepth), pointSelection 0 / 1 FullSystem.cc:1272-1304
//   GpuBackend::residentImmature / syncImmaturePoints   the three members above with the immature set resident on the device (no reference counterpart)
//   GpuBackend::flagPointsForRemoval(fs)            the policy of void FullSystem::flagPointsForRemoval()           FullSystem.cc:1208-1270
//   GpuBackend::marginalizePoints(fs)               void EnergyFunctional::marginalizePointsF() + FullSystem.cc:1241-1250   EnergyFunctional.cc:165-222
//   GpuBackend::undistortFrame(id, raw, ...)        ImageAndExposure *Undistort::undistort<T>(...) + makeImages     Undistort.cc:357-457
//
// The functions reach into private members of FullSystem / CoarseTracker (frames, ef, activeResiduals, allFrameHistory, lastCoarseRMSE,
// shellPoseMutex ...): a maintainer makes them member functions or adds `friend class ldso::GpuBackend;` to the two classes.  The reference tree
// is read-only in this repository, so adapter_internal.h opens the access specifiers for the adapter's own inclusion of the two headers instead
// (LDSO_ADAPTER_OPEN_PRIVATE) - the class layout is unchanged, the object files link against the reference's own.
#pragma once
#include <map>
#include <memory>
#include <chrono>
#include <deque>
#include <mutex>
#include <set>
#include <vector>

#include "frontend/CoarseTracker.h"
#include "frontend/FullSystem.h"
#include "internal/ImmaturePoint.h"
#include "ldso_hip.h"

namespace ldso {

class GpuBackend {
public:
    // One backend per FullSystem (the BA handle belongs to the mapping thread, the tracker handles to whoever holds the respective
    // CoarseTracker - the reference's mutex discipline, FullSystem.h:272-306).  Image size / pyramid depth come from the globals of
    // internal/GlobalCalib.h (wG[0], hG[0], pyrLevelsUsed), like the reference's own constructors.
    GpuBackend(int device, int maxFrames, int maxPoints);
    ~GpuBackend();
    GpuBackend(const GpuBackend &) = delete;
    GpuBackend &operator=(const GpuBackend &) = delete;

    // ---- windowed bundle adjustment -------------------------------------------------------------------------------------------------
    float optimize(FullSystem &fs, int mnumOptIts);
    // also store RawResidualJacobian (296 B per residual: 3.5 MB at C3) back into r->J.  Off by default: nothing of makeKeyFrame reads the J that
    // optimize() leaves behind - flagPointsForRemoval re-linearises the residuals it marginalises (FullSystem.cc:1241-1250: r->linearize writes
    // r->J itself) and the next optimize() re-linearises everything.  On for host code that still accumulates from r->J.
    bool writeBackJacobians = false;
    // The window stays RESIDENT on the device between two optimize() calls: the second call uploads a delta (ldso_ba_update_window) - which frames and points
    // stayed, one bit per residual, the records of the freshly activated points - instead of flattening and uploading 2000 points and 12 000 residuals again.
    // What the delta path relies on is what LDSO does: between two optimize() calls the host does not change a SURVIVING point's u / v / colours / inverse depth
    // or the state of its residuals (it only removes points and residuals, adds one residual per point for the new key frame, and activates new points;
    // FullSystem::makeKeyFrame :429-640).  Residual counts are checked per point and a point whose residual list changed in another way is re-read in full;
    // invalidateWindow() (or residentWindow = false) forces the next optimize() to upload everything.
    bool residentWindow = true;
    void invalidateWindow() { window_.valid = false; }
    bool lastUploadWasDelta = false;
    int uploadsDelta = 0, uploadsFresh = 0;          // how the windows of this backend's lifetime went over
    int uploadsFreshBecauseLinearized = 0;           // ... of the full uploads: windows that held linearised residuals (ldso_ba_update_window does not carry them)
    int residentPointerMismatches = 0;               // resident points whose cached residual pointers no longer matched PointHessian::residuals (their list was re-read)
    // marginalizeFrame(): how often the device path ran, and how often the call fell back to the reference's HOST member (FullSystem::marginalizeFrame ->
    // EnergyFunctional.cc:72-151) because no window of these frames was resident - a maintainer sees here when the drop-in did not take the device path
    int margFrameDevice = 0, margFrameHostFallback = 0;
    // FullSystem::activeResiduals is only read inside FullSystem::optimize itself (FullSystem.cc:735-1770: linearizeAll / applyRes / setNewFrameEnergyTH - all of
    // which run on the device here); filling it costs 12 000 shared_ptr copies per call.  On for host code that wants the list anyway.
    bool fillActiveResiduals = false;
    int lastIterations = 0;              // GN iterations the device executed in the last optimize()
    double lastUploadSeconds[6] = {0, 0, 0, 0, 0, 0};  // of that: settings + image slots | flatten (host walk) | ldso_ba_set_window | set_point_stats | set_frames | set_prior
    double lastOptimizeSeconds[4] = {0, 0, 0, 0};      // wall clock of the last optimize(): flatten + upload | device | fetch | write-back into the objects

    // void FullSystem::marginalizeFrame(shared_ptr<Frame> &frame) (FullSystem.cc:602-645): the Schur complement of EnergyFunctional::marginalizeFrame
    // (EnergyFunctional.cc:72-151) through ldso_ba_marginalize_frame on the window optimize() left resident (ef's H_M / b_M go up first: 29 KB), the reference's
    // bookkeeping on the host - with the residuals that target the frame found through the resident window's host view (one pointer per point) instead of a
    // weak_ptr::lock() per residual of the window.
    void marginalizeFrame(FullSystem &fs, shared_ptr<Frame> &frame);
    // ---- point marginalisation on the device (what follows optimize() in makeKeyFrame, FullSystem.cc:526-536) ----------------------------
    // flagPointsForRemoval: the POLICY of FullSystem::flagPointsForRemoval (FullSystem.cc:1208-1270: which points go OUT / OUTLIER / MARGINALIZED) without its inner
    // loop (:1241-1250: resetOOB + linearize + applyRes + fixLinearizationF of every residual of a point that gets marginalised) - the device pass of
    // marginalizePoints does exactly that to exactly those points.  marginalizePoints: EnergyFunctional::marginalizePointsF (EnergyFunctional.cc:165-222) through
    // ldso_ba_marginalize_points on the window GpuBackend::optimize left resident (same frames, same point order), H_M / b_M written back into ef, the
    // reference's bookkeeping (priorF, connectivity counts, removePoint, makeIDX) on the host.  Call order as the reference: flagPointsForRemoval,
    // ef->dropPointsF(), marginalizePoints.
    void flagPointsForRemoval(FullSystem &fs);
    void marginalizePoints(FullSystem &fs);

    // ---- coarse tracker -------------------------------------------------------------------------------------------------------------
    void makeK(CoarseTracker &tr, shared_ptr<CalibHessian> HCalib);
    void setCoarseTrackingRef(CoarseTracker &tr, std::vector<shared_ptr<FrameHessian>> &frameHessians);
    bool trackNewestCoarse(CoarseTracker &tr, shared_ptr<FrameHessian> newFrameHessian, SE3 &lastToNew_out, AffLight &aff_g2l_out, int coarsestLvl,
                           Vec5 minResForAbort);
    Vec4 trackNewCoarse(FullSystem &fs, shared_ptr<FrameHessian> fh);

    // ---- point activation (the optimizeImmaturePoint calls of activatePointsMT_Reductor) ---------------------------------------------
    // optimized[k] = the new PointHessian of toOptimize[k] or nullptr, exactly what FullSystem::optimizeImmaturePoint returns
    void activatePoints(FullSystem &fs, std::vector<shared_ptr<internal::ImmaturePoint>> &toOptimize, std::vector<shared_ptr<PointHessian>> &optimized);

    // ---- void FullSystem::activatePointsMT()                                                                    FullSystem.cc:1052-1189
    // The whole member: the density controller on fs.currentMinActDist (:1054-1073), then distance map, candidate selection and optimizeImmaturePoint of the
    // selected points as ONE device call (ldso_ba_select_activate_points: makeDistanceMap / the loop of :1088-1152 / addIntoDistFinal / :1154-1164), the
    // status hand-over of the deleted candidates (:1105-1149) and the object hand-over of the new points (:1166-1188) on the host.
    void activatePointsMT(FullSystem &fs);
    int lastSelection[3] = {0, 0, 0};                   // of the last activatePointsMT: candidates, selected, activated
    // what the selection reads from the object graph, in the member's own iteration order (also the test harness's way to hand one state to both sides)
    struct SelectionInputs {
        std::vector<ldso_act_seed_t> seeds;
        std::vector<ldso_immature_t> cand;
        std::vector<float> myType, KRKi, Kt;
        std::vector<int32_t> flagged;
        std::vector<shared_ptr<internal::ImmaturePoint>> who;
    };
    static void gatherSelection(FullSystem &fs, SelectionInputs &in);
    // of that, the per-host part alone: KRKi / Kt of host -> newest frame (:1092-1094) and the hosts' flaggedForMarginalization
    static void selectionPoses(FullSystem &fs, SelectionInputs &in);

    // ---- immature-point tracing: void FullSystem::traceNewCoarse(shared_ptr<FrameHessian> fh)                   FullSystem.cc:1012-1050
    void traceNewCoarse(FullSystem &fs, shared_ptr<FrameHessian> fh);
    int lastTraceCounts[6] = {0, 0, 0, 0, 0, 0};        // good, oob, outlier, skipped, bad condition, uninitialised (the function's trace_* counters)

    // ---- the immature set RESIDENT on the device from detection through activation ------------------------------------------------------------------------
    // Off (default): every member above and below does what it always did - traceNewCoarse and activatePointsMT flatten every ImmaturePoint of the window,
    // upload the records, and traceNewCoarse downloads them again and writes six fields back into every object.
    // On: the tracer owns the set.  The backend remembers which ImmaturePoint every tracer row belongs to; a RECONCILE step at the head of traceNewCoarse,
    // activatePointsMT and makeNewTraces walks the graph (pointers only) and compares:
    //   - the graph's list equals the rows, host indices unchanged                      nothing is uploaded                          immatureReconcile[0]
    //   - it is an ordered subsequence of the rows (points released by host code, a frame marginalised, host indices shifted)
    //                                                                                   one ldso_trace_compact (mask + host map)     immatureReconcile[1]
    //   - anything else (the host created points the device has not seen, the tracer was re-created, the mode was just switched on)
    //                                  the device records are written into the surviving objects, then everything goes up anew        immatureReconcile[2]
    // traceNewCoarse then only sends the poses and traces (no record crosses PCIe, no object is written: lastTraceCounts as before); activatePointsMT runs
    // ldso_ba_select_activate_tracer with the compaction by its decisions and does the host hand-over.  makePoint uses the constructor's fields of an
    // ImmaturePoint; CreateFromImmature's PointHessian constructor also reads the STALE idepth_min / idepth_max (PointHessian.cc:14), which is harmless only
    // because makePoint overwrites the inverse depth with setIdepthZero / setIdepth right after - a makePoint that starts to use trace state needs a sync first; makeNewTraces appends the new records device to device.  Between two syncImmaturePoints calls the six fields traceOn writes (idepth_min,
    // idepth_max, quality, lastTraceStatus, lastTraceUV, lastTracePixelInterval) are current on the DEVICE only: host code that reads them (a viewer, a switch
    // back to the host path with the flag off) calls syncImmaturePoints first.
    bool residentImmature = false;
    int tracerMinCapacity = 16384;                   // records a new tracer holds at least (it is created with twice what is needed, or this)
    int immatureReconcile[3] = {0, 0, 0};
    void syncImmaturePoints(FullSystem &fs);

    // ---- new features of a key frame: void FullSystem::makeNewTraces(shared_ptr<FrameHessian> newFrame, float *gtDepth)   FullSystem.cc:1272-1283
    // for setting_pointSelection == 0: PixelSelector::makeMaps(newFrame, selectionMap, setting_desiredImmatureDensity) (:1287), the raster scan of :1290-1303 and
    // the ImmaturePoint constructors on the device (ldso_pixsel_make_maps / _make_points on the frame's device pyramid; image sizes that are multiples of 32).
    // fs.pixelSelector keeps currentPotential: read before and written after every call, so the reference's member and this one can alternate; its
    // randomPattern goes up once.  frame->features gets one Feature(x, y) per point, in raster order, my_type = the map value; lastNewTraces[1] stays 0.
    // for setting_pointSelection == 1 (2 throws): FeatureDetector::DetectCorners(setting_desiredImmatureDensity, frame) and the ImmaturePoint
    // constructors as ONE device call (ldso_feat_detect on the frame's device pyramid), then frame->features filled in the reference's order - uv, score,
    // isCorner, angle, descriptor - each with its ImmaturePoint (constructed, then its fields overwritten from the device record).  A feature whose record
    // has a non-finite energyTH is dropped, as :1298 does for the other selection modes.  The gamma weight of absSquaredGrad follows
    // setting_gammaWeightsPixelSelect and Hcalib->mpCH->B (FrameHessian.cc:93-97).
    // orbPattern: the 1024 ints of ldso::bit_pattern_31_ (src/frontend/FeatureDetector.cc), set by the caller before the first call; null: descriptors stay zero.
    const int *orbPattern = nullptr;
    void makeNewTraces(FullSystem &fs, shared_ptr<FrameHessian> newFrame);
    int lastNewTraces[3] = {0, 0, 0};                   // of the last makeNewTraces: features detected, corners among them, features dropped

    // ---- FrameHessian::dIp on the device: one ldso_pyramid_t per frame (FrameHessian.cc:44-113 on the device from the frame's irradiance, 4 bytes per pixel
    // over PCIe once per frame), shared zero-copy by the BA image slot, the tracer and both roles of the coarse trackers - as the reference shares fh->dIp by
    // pointer.  Off: every consumer uploads the host arrays it needs (12 bytes per pixel and consumer).  Pyramids of frames that left the window and are neither
    // a tracker's reference nor among the most recent frames are released at the next optimize().
    bool useDevicePyramids = true;
    int pyramidsBuilt = 0;               // statistics: pyramids built so far (one per frame seen)

    // ---- raw camera frames: ImageAndExposure *Undistort::undistort<T>(image_raw, exposure, timestamp, factor)       Undistort.cc:357-457
    // setUndistortion: the calibration as the plain arrays the reference's constructors leave (they are protected / private members, Undistort.h:55-61, :97-106:
    // INTEGRATION.md names the two accessors a maintainer adds).  remapX / remapY: wG[0] * hG[0] floats each, both null for a passthrough undistorter;
    // G: GDepth entries or null (no valid photometric calibration); vignetteMapInv: wOrg * hOrg floats (needed for setting_photometricCalibration == 2).
    // setting_photometricCalibration and setting_useExposure are read here, once.
    void setUndistortion(int wOrg, int hOrg, const float *remapX, const float *remapY, const float *G, int GDepth, const float *vignetteMapInv);
    // undistortFrame: the raw frame (wOrg * hOrg pixels of 1 or 2 bytes) goes up, the irradiance is written into a new device pyramid and the pyramid is
    // built behind it on the same stream, registered under frameId = Frame::id: the tracker, the tracer and the BA slot of that frame find it (pyramidOf)
    // instead of building one from fh->dIp[0]; until the first of them has, releasePyramids() leaves it alone (for the kMaxPending most recent such
    // frames), whichever thread runs it.  No host synchronisation unless hostIrradiance (wG[0] * hG[0] floats, optional) asks for the image.
    // Returns ImageAndExposure::exposure_time.  One deliberate difference from the reference: a remap entry whose four taps are not all inside the raw
    // frame gives 0, where the reference reads one row past the frame for the entry xxi == 0 && yyi == hOrg - 1 (include/ldso_hip.h).
    float undistortFrame(unsigned long frameId, const void *raw, int bytesPerPixel, float exposure, float factor, float *hostIrradiance = nullptr);
    // test fetch: level lvl of the frame's device pyramid ((wG[lvl] * hG[lvl] * 3 floats), built from fh->dIp[0] if the frame has none yet
    void getPyramidLevel(const shared_ptr<FrameHessian> &fh, int lvl, float *out);

    const char *lastError() const;

private:
    // The private state, grouped by the invariant that spans it; every group is a small nested type that owns what its invariant needs and offers the
    // operations that keep it.  WHICH THREAD TOUCHES WHAT: only the pyramid registry and the tracker handles are shared between the tracking thread
    // (undistortFrame, trackNewCoarse, trackNewestCoarse on coarseTracker) and the mapping thread (everything else; coarseTracker_forNewKF under
    // coarseTrackerSwapMutex) - each has its mutex, taken by its own operations and by no other code.  Everything else belongs to the mapping thread, but for
    // undist_, which setUndistortion sets before the first frame.  DESTRUCTION ORDER: the pyramids go after every handle that names one on the device (BA image
    // slots, tracer, trackers): ~GpuBackend destroys the BA, tracker and selector handles in its body, the tracer goes with its row set, and the registry is declared before every
    // consumer's reference (tracerPyr_ before the row set).
    int device_, maxFrames_, maxPoints_;

    // ---- the pyramid registry (adapter_pyramids.cc): one device pyramid per frame (Frame::id), REFERENCE-COUNTED.  The registry holds one reference, every
    // consumer that names the pyramid on the device holds another (the BA image slot, the tracer, a tracker's reference frame / new frame).  release() only drops
    // the REGISTRY's reference of frames that left the window and that nobody else holds; the device memory goes when the last holder lets go - no guessing which
    // tracker may still read it, no reading of another thread's state.
    struct PyrHolder {
        ldso_pyramid_t *p = nullptr;
        std::vector<float> irradiance;                               // the host copy of channel 0 the build read from
        ~PyrHolder();
    };
    typedef std::shared_ptr<PyrHolder> PyrRef;
    class PyramidRegistry {
    public:
        // the frame's pyramid, built from fh->dIp[0] if the frame has none yet (`built` counts the builds); the caller holds it from here on
        PyrRef getOrBuild(const shared_ptr<FrameHessian> &fh, int device, int &built);
        // a pyramid undistortFrame filled, under its Frame::id: pending until the first consumer asks for it
        void registerUndistorted(unsigned long frameId, const PyrRef &e, int &built);
        // drops the registry's reference of every frame that is not in `keep`, not pending, and held by nobody else
        void release(const std::set<unsigned long> &keep);
    private:
        std::map<unsigned long, PyrRef> pyr_;                        // Frame::id -> pyramid
        std::mutex mutex_;                                           // tracking thread (new frame / reference) and mapping thread (window, tracer) share the map
        // Frames registerUndistorted took that no consumer has asked for yet: such a frame is in no window and no consumer holds its pyramid, so release() -
        // the mapping thread may run it between the tracking thread's undistortFrame(id) and its trackNewCoarse(fh) - would take the registry's reference
        // for the last one.  It spares these ids; getOrBuild() takes an id off the list when it hands the pyramid out.  At most kMaxPending ids: a frame that
        // never reaches a consumer loses the protection when kMaxPending newer frames have been registered, and is released then.
        static constexpr size_t kMaxPending = 8;
        std::deque<unsigned long> pending_;
    };
    PyramidRegistry pyramids_;                                       // declared before every consumer's PyrRef below: destroyed after them
    PyrRef pyramidOf(const shared_ptr<FrameHessian> &fh) { return pyramids_.getOrBuild(fh, device_, pyramidsBuilt); }
    void releasePyramids(FullSystem &fs);
    ldso_undistorter_t *undist_ = nullptr;

    // ---- the BA handle and its image slots (mapping thread) ----
    ldso_ba_t *ba_ = nullptr;
    std::map<unsigned long, int> slotOf_;                            // key frame (Frame::id: addresses get reused) -> image slot of the BA handle
    std::vector<long> slotOwner_;                                    // slot -> Frame::id, -1 = free
    std::vector<PyrRef> slotPyr_;                                    // slot -> the pyramid it aliases
    void syncImageSlots(FullSystem &fs, std::vector<int32_t> &slots);

    // ---- the resident window as the host sees it (adapter_window.cc): one row per point in device order, its residual objects by window column (= target
    // frame index).  rows, flat and resBegin describe the same residuals: flat / resBegin are rebuilt from the rows, a residual leaves through dropResidual.
    struct ResidentWindow {
        static constexpr int kMaxCols = 16;
        static_assert(kMaxCols >= LDSO_MAX_FRAMES, "a row of the resident window holds one residual pointer per window column");
        struct Row {
            PointHessian *ph; Feature *feat; uint32_t mask; int host; PointFrameResidual *res[kMaxCols];
            static Row empty(PointHessian *ph, Feature *feat, int host) { Row r; r.ph = ph; r.feat = feat; r.mask = 0; r.host = host; for (int c = 0; c < kMaxCols; c++) r.res[c] = nullptr; return r; }
        };
        std::vector<Row> rows;
        std::vector<PointFrameResidual *> flat;                      // the residual objects in the device's flat order (point-major, target-ascending)
        std::vector<int32_t> resBegin;                               // the residuals of point k are flat[resBegin[k] .. resBegin[k + 1])
        std::vector<shared_ptr<Frame>> frames;                       // the frame of every column (held: the rows point into their features)
        std::vector<shared_ptr<PointHessian>> points;                // the points of the window optimize() left on the device, in its order (held for the rows)
        bool valid = false;
        // The row of one point from its residual list: mask and one pointer per column.  Where a residual's column comes from: Stored = its targetIDX as
        // makeIDX left it, FromTarget = its target frame's idx (one weak_ptr::lock); both write hostIDX / targetIDX into the residual, as a full upload
        // does.  FromTargetNotLinearized = the target frame's idx, nothing written, a linearised residual refused (the delta path).  false: a residual names
        // a frame outside the window, the host, or a target twice, or is refused (the row is not to be used then)
        enum class Columns { Stored, FromTarget, FromTargetNotLinearized };
        static bool buildRow(Row &row, PointHessian &ph, Feature *feat, int host, int F, Columns how);
        void rebuildFlat(int F);
        // one residual of a row leaves the graph (lastResiduals, EnergyFunctional::dropResidual) and the row (pointer and mask bit: the next delta says so
        // through the cleared bit); nothing happens when the point's list does not hold it
        static void dropResidual(Row &row, const PointFrameResidual *res, internal::EnergyFunctional &ef);
    };
    ResidentWindow window_;
    bool uploadDelta(FullSystem &fs, const std::vector<int32_t> &slots, std::vector<shared_ptr<PointHessian>> &allPoints);
    void uploadFresh(FullSystem &fs, const std::vector<int32_t> &slots, std::vector<shared_ptr<PointHessian>> &allPoints, bool trustIndices);
    int uploadWindow(FullSystem &fs, std::vector<shared_ptr<PointHessian>> &allPoints, bool trustIndices = false);
    // optimize()'s write-back: where ldso_ba_get_results lands (kept across calls)
    std::vector<ldso_res_out_t> wbRes_; std::vector<int32_t> wbState_, wbActive_, wbRemove_;
    std::vector<ldso_point_out_t> wbPoints_; std::vector<ldso_frame_t> wbFrames_; std::vector<double> wbStep_;
    std::chrono::steady_clock::time_point lapT_;
    double lapSince() { const auto n = std::chrono::steady_clock::now(); const double d = std::chrono::duration<double>(n - lapT_).count(); lapT_ = n; return d; }
    // the host hand-over of activatePointsMT (:1105-1149, :1166-1188): the deleted candidates, then the selected ones
    void handOverSelection(FullSystem &fs, const std::vector<shared_ptr<internal::ImmaturePoint>> &who, const std::vector<int32_t> &decision, const std::vector<int32_t> &selected, int nSel,
                           const std::vector<ldso_activation_t> &out);
    static shared_ptr<PointHessian> makePoint(FullSystem &fs, const shared_ptr<internal::ImmaturePoint> &point, const ldso_activation_t &out);

    // ---- the immature row set (adapter_immature.cc): the tracer and, in resident mode, the ImmaturePoint of every tracer row in order (held: a released
    // point's address must not come back as a new one's) with the host index the device record carries.  THE RULE: the row list and the tracer's count move
    // together; whatever fails in between forgets the rows, and the next reconcile uploads the set anew.  The list changes through the operations below only.
    class ImmatureRows {
    public:
        ~ImmatureRows();                                 // the tracer goes with its rows
        ldso_tracer_t *tracer = nullptr;
        const std::vector<shared_ptr<internal::ImmaturePoint>> &who() const { return who_; }
        const std::vector<int> &host() const { return host_; }
        size_t size() const { return who_.size(); }
        int capacity() const { return cap_; }
        // a tracer that holds `need` records (created with twice that, or minCapacity); a new one starts with no rows
        void ensure(int device, int need, int minCapacity);
        void forget();
        void adopt(std::vector<shared_ptr<internal::ImmaturePoint>> &cur, std::vector<int> &curHost);          // the rows are now these (taken by swap)
        void append(const std::vector<shared_ptr<internal::ImmaturePoint>> &fresh, int hostIdx);
        void compact(const std::vector<uint8_t> &keep);                                                         // the rows with keep[row] != 0 stay, in order
        // a device call that changes the tracer's count: the rows are forgotten when it throws
        template <class Call> void guarded(Call &&call) { try { call(); } catch (...) { forget(); throw; } }
    private:
        int cap_ = 0;
        std::vector<shared_ptr<internal::ImmaturePoint>> who_;
        std::vector<int> host_;
    };
    PyrRef tracerPyr_;                                               // the frame the tracer currently reads (declared before the tracer: released after it)
    ImmatureRows imm_;
    void reconcileImmature(FullSystem &fs, bool setIdxInImmaturePoints);
    void downloadImmature(const std::vector<char> *alive);
    // makeNewTraces: the detector (setting_pointSelection == 1) and the pixel selector (== 0) with what each is recreated for
    ldso_features_t *features_ = nullptr;
    int featuresCap_ = 0;
    const int *featuresPattern_ = nullptr;
    ldso_pixsel_t *pixsel_ = nullptr;                    // created at the first call with fs.pixelSelector's randomPattern
    const unsigned char *pixselPattern_ = nullptr;      // ... which it is recreated for when another PixelSelector or image size comes along
    int pixselW_ = 0, pixselH_ = 0;
    struct NewTraces;                                    // what either mode reports: records, types, features
    bool detectCorners(FullSystem &fs, const shared_ptr<FrameHessian> &newFrame, int hostIdx, NewTraces &out);
    void selectPixels(FullSystem &fs, const shared_ptr<FrameHessian> &newFrame, int hostIdx, NewTraces &out);
    void appendFreshRecords(const NewTraces &nt, const void *immDev, const void *typeDev, int nDev, const std::vector<shared_ptr<ImmaturePoint>> &fresh, int hostIdx);

    // ---- the tracker handles (adapter_tracker.cc): the reference double-buffers two CoarseTrackers (FullSystem.h:296-297); of() / newFrameResident() / hold*()
    // run on the tracking thread (coarseTracker) AND on the mapping thread (coarseTracker_forNewKF, FullSystem.cc makeKeyFrame)
    class TrackerHandles {
    public:
        ldso_tracker_t *of(CoarseTracker &tr, int device);
        // true when handle t already holds this frame's pyramid as its new frame; otherwise records that it is about to
        bool newFrameResident(ldso_tracker_t *t, const shared_ptr<FrameHessian> &fh);
        void holdRef(ldso_tracker_t *t, const PyrRef &pr);
        void holdNewFrame(ldso_tracker_t *t, const PyrRef &pr);
        void destroyAll();
    private:
        struct Held { PyrRef ref, newFrame; };
        std::map<CoarseTracker *, ldso_tracker_t *> trackers_;
        std::map<ldso_tracker_t *, Held> pyr_;
        // whose pyramid a handle currently holds as "new frame": keyed by Frame::id, not by address (LDSO releases the FrameHessian of a non-key frame
        // after tracking, the allocator may hand the same address to the next frame)
        std::map<ldso_tracker_t *, unsigned long> newFrameId_;
        std::mutex mutex_;
    };
    TrackerHandles trackers_;
    ldso_tracker_t *trackerOf(CoarseTracker &tr) { return trackers_.of(tr, device_); }
    void handNewFrame(ldso_tracker_t *t, const shared_ptr<FrameHessian> &fh);
};

}  // namespace ldso
