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
// is read-only in this repository, so ldso_gpu_adapter.cc opens the access specifiers for its own inclusion of the two headers instead
// (LDSO_ADAPTER_OPEN_PRIVATE) - the class layout is unchanged, the object files link against the reference's own.
#pragma once
#include <map>
#include <memory>
#include <chrono>
#include <deque>
#include <mutex>
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
    void invalidateWindow() { residentValid_ = false; }
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
    ldso_undistorter_t *undist_ = nullptr;
    ldso_ba_t *ba_ = nullptr;
    static shared_ptr<PointHessian> makePoint(FullSystem &fs, const shared_ptr<internal::ImmaturePoint> &point, const ldso_activation_t &out);
    ldso_tracer_t *tracer_ = nullptr;
    int tracerCap_ = 0;
    // resident mode: the ImmaturePoint of every tracer row in order (held: a released point's address must not come back as a new one's), and the host index
    // the device record carries
    std::vector<shared_ptr<internal::ImmaturePoint>> who_;
    std::vector<int> whoHost_;
    void reconcileImmature(FullSystem &fs, bool setIdxInImmaturePoints);
    void ensureTracer(int capacity);
    void downloadImmature(const std::vector<char> *alive);
    ldso_features_t *features_ = nullptr;
    int featuresCap_ = 0;
    const int *featuresPattern_ = nullptr;
    ldso_pixsel_t *pixsel_ = nullptr;                    // setting_pointSelection == 0: created at the first call with fs.pixelSelector's randomPattern
    const unsigned char *pixselPattern_ = nullptr;      // ... which it is recreated for when another PixelSelector or image size comes along
    int pixselW_ = 0, pixselH_ = 0;
    void makeNewTracesPixelSelector(FullSystem &fs, shared_ptr<FrameHessian> newFrame);
    void appendFreshRecords(const std::vector<ldso_immature_t> &rec, const void *immDev, const void *typeDev, const std::vector<shared_ptr<ImmaturePoint>> &fresh, int hostIdx);
    std::map<CoarseTracker *, ldso_tracker_t *> trackers_;          // the reference double-buffers two CoarseTrackers (FullSystem.h:296-297)
    std::map<unsigned long, int> slotOf_;                            // key frame (Frame::id: addresses get reused) -> image slot of the BA handle
    std::vector<long> slotOwner_;                                    // slot -> Frame::id, -1 = free
    std::vector<shared_ptr<PointHessian>> lastPoints_;               // the points of the window optimize() left on the device, in its order
    // One device pyramid per frame (Frame::id), REFERENCE-COUNTED: the map below holds one reference, every consumer that names the pyramid on the device
    // holds another (the BA image slot, the tracer, a tracker's reference frame / new frame).  releasePyramids() only drops the MAP's reference of frames that
    // left the window and that nobody else holds; the device memory goes when the last holder lets go - no guessing which tracker may still read it, no
    // reading of another thread's state (the keep-set was built from an unsynchronised read of the trackers' maps and of lastRef).
    struct PyrHolder {
        ldso_pyramid_t *p = nullptr;
        std::vector<float> irradiance;                               // the host copy of channel 0 the build read from
        ~PyrHolder();
    };
    typedef std::shared_ptr<PyrHolder> PyrRef;
    std::map<unsigned long, PyrRef> pyr_;                            // Frame::id -> pyramid
    std::mutex pyrMutex_;                                            // tracking thread (new frame / reference) and mapping thread (window, tracer) share the map
    // Frames undistortFrame registered that no consumer has asked for yet (guarded by pyrMutex_): such a frame is in no window and no consumer holds its
    // pyramid, so releasePyramids() - the mapping thread may run it between the tracking thread's undistortFrame(id) and its trackNewCoarse(fh) - would
    // take the map's reference for the last one.  It spares these ids; pyramidOf() takes an id off the list when it hands the pyramid out.  At most
    // kMaxPending ids: a frame that never reaches a consumer loses the protection when kMaxPending newer frames have been registered, and is released then.
    static constexpr size_t kMaxPending = 8;
    std::deque<unsigned long> pendingPyr_;
    std::vector<PyrRef> slotPyr_;                                    // BA image slot -> the pyramid it aliases (mapping thread only)
    PyrRef tracerPyr_;                                               // the frame the tracer currently reads (mapping thread only)
    struct TrackerPyr { PyrRef ref, newFrame; };
    std::map<ldso_tracker_t *, TrackerPyr> trackerPyr_;              // guarded by handlesMutex_
    PyrRef pyramidOf(const shared_ptr<FrameHessian> &fh);
    void releasePyramids(FullSystem &fs);
    std::vector<int32_t> resBegin_;                                  // last upload: the residuals of point k are flat_[resBegin_[k] .. resBegin_[k + 1])
    // the resident window as the host sees it: one row per point in device order, its residual objects by window column (= target frame index)
    static constexpr int kMaxCols = 16;
    static_assert(kMaxCols >= LDSO_MAX_FRAMES, "a row of the resident window holds one residual pointer per window column");
    struct Row { PointHessian *ph; Feature *feat; uint32_t mask; int host; PointFrameResidual *res[kMaxCols]; };
    std::vector<Row> rows_;
    // optimize()'s write-back: where ldso_ba_get_results lands (kept across calls)
    std::vector<ldso_res_out_t> wbRes_; std::vector<int32_t> wbState_, wbActive_, wbRemove_;
    std::vector<ldso_point_out_t> wbPoints_; std::vector<ldso_frame_t> wbFrames_; std::vector<double> wbStep_;
    std::vector<shared_ptr<Frame>> rowFrames_;                       // the frame of every column of the resident window (held: the rows point into their features)
    std::vector<PointFrameResidual *> flat_;                         // the residual objects in the device's flat order (point-major, target-ascending)
    bool residentValid_ = false;
    std::chrono::steady_clock::time_point lapT_;
    double lapSince() { const auto n = std::chrono::steady_clock::now(); const double d = std::chrono::duration<double>(n - lapT_).count(); lapT_ = n; return d; }
    bool uploadDelta(FullSystem &fs, const std::vector<int32_t> &slots, std::vector<shared_ptr<PointHessian>> &allPoints);
    void uploadFresh(FullSystem &fs, const std::vector<int32_t> &slots, std::vector<shared_ptr<PointHessian>> &allPoints, bool trustIndices);
    int device_, maxFrames_, maxPoints_;
    // whose pyramid a tracker handle currently holds as "new frame": keyed by Frame::id, not by address (LDSO releases the FrameHessian of a
    // non-key frame after tracking, the allocator may hand the same address to the next frame)
    std::map<ldso_tracker_t *, unsigned long> trackerNewFrameId_;
    // trackerOf / newFrameResident run on the tracking thread (coarseTracker) AND on the mapping thread (coarseTracker_forNewKF under
    // coarseTrackerSwapMutex, FullSystem.cc makeKeyFrame): the two maps above are shared between them
    std::mutex handlesMutex_;
    bool newFrameResident(ldso_tracker_t *t, const shared_ptr<FrameHessian> &fh);
    ldso_tracker_t *trackerOf(CoarseTracker &tr);
    int uploadWindow(FullSystem &fs, std::vector<shared_ptr<PointHessian>> &allPoints, bool trustIndices = false);
    void syncImageSlots(FullSystem &fs, std::vector<int32_t> &slots);
};

}  // namespace ldso
