// adapter_pyramids.cc — FrameHessian::dIp on the device (FrameHessian.cc:44-113): the pyramid registry, raw-frame undistortion into a pyramid, and the image
// slots of the BA handle.  A pyramid is built once per frame from channel 0 of dIp[0] (= the irradiance makeImages started from; the device build is
// bit-identical to the host arrays, tests/test_pyramid_gpu.py) or by undistortFrame, keyed by Frame::id.
#include "adapter_internal.h"

using namespace ldso::internal;
using namespace ldso::adp;

namespace ldso {

GpuBackend::PyrHolder::~PyrHolder() { if (p) ldso_pyr_destroy(p); }

// ---- the registry: the only code that takes its mutex ----------------------------------------------------------------------------------------------------
GpuBackend::PyrRef GpuBackend::PyramidRegistry::getOrBuild(const shared_ptr<FrameHessian> &fh, int device, int &built) {
    const unsigned long id = fh->frame->id;
    std::lock_guard<std::mutex> lk(mutex_);
    auto it = pyr_.find(id);
    if (it != pyr_.end()) {
        pending_.erase(std::remove(pending_.begin(), pending_.end(), id), pending_.end());          // the caller holds it from here on
        return it->second;
    }
    PyrRef e = std::make_shared<PyrHolder>();
    const size_t n = (size_t) wG[0] * hG[0];
    e->irradiance.resize(n);
    const Vec3f *src = fh->dIp[0];
    for (size_t i = 0; i < n; i++) e->irradiance[i] = src[i][0];
    int rc = ldso_pyr_create(device, wG[0], hG[0], pyrLevelsUsed, &e->p);
    if (rc == LDSO_OK) rc = ldso_pyr_make_images(e->p, e->irradiance.data(), nullptr);
    throwOn(rc, "ldso_pyr_create / ldso_pyr_make_images");          // e (and its half-built pyramid) goes with the exception
    pyr_[id] = e;
    built++;
    return e;
}

void GpuBackend::PyramidRegistry::registerUndistorted(unsigned long frameId, const PyrRef &e, int &built) {
    std::lock_guard<std::mutex> lk(mutex_);
    pyr_[frameId] = e;
    pending_.erase(std::remove(pending_.begin(), pending_.end(), frameId), pending_.end());
    pending_.push_back(frameId);
    if (pending_.size() > kMaxPending) pending_.pop_front();
    built++;
}

// Frames outside `keep` AND that no consumer holds any more (use_count 1 = the registry alone) AND that are not waiting for their first consumer (pending_).
// A consumer can only gain a reference through getOrBuild, i.e. under the mutex: a count of 1 seen here cannot grow behind our back; a consumer letting go
// concurrently only delays the release by one call.
void GpuBackend::PyramidRegistry::release(const std::set<unsigned long> &keep) {
    std::vector<PyrRef> dying;                                       // destroyed outside the lock
    {
        std::lock_guard<std::mutex> lk(mutex_);
        for (auto it = pyr_.begin(); it != pyr_.end();) {
            const bool pending = std::find(pending_.begin(), pending_.end(), it->first) != pending_.end();          // undistorted, not yet asked for
            if (!keep.count(it->first) && !pending && it->second.use_count() == 1) { dying.push_back(std::move(it->second)); it = pyr_.erase(it); } else ++it;
        }
    }
}

// the pyramids of frames that left the window
void GpuBackend::releasePyramids(FullSystem &fs) {
    std::set<unsigned long> keep;
    for (auto &fr : fs.frames) keep.insert(fr->id);
    pyramids_.release(keep);
}

// Undistort::undistort<T> (Undistort.cc:357-457) on the device, straight into the frame's pyramid
void GpuBackend::setUndistortion(int wOrg, int hOrg, const float *remapX, const float *remapY, const float *G, int GDepth, const float *vignetteMapInv) {
    if (undist_) { ldso_undist_destroy(undist_); undist_ = nullptr; }
    throwOn(ldso_undist_create(device_, wOrg, hOrg, wG[0], hG[0], &undist_), "ldso_undist_create");
    throwOn(ldso_undist_set_remap(undist_, remapX, remapY), "ldso_undist_set_remap");
    throwOn(ldso_undist_set_photometric(undist_, G, GDepth, vignetteMapInv, setting_photometricCalibration, setting_useExposure ? 1 : 0), "ldso_undist_set_photometric");
}

float GpuBackend::undistortFrame(unsigned long frameId, const void *raw, int bytesPerPixel, float exposure, float factor, float *hostIrradiance) {
    if (!undist_) throw std::runtime_error("GpuBackend::undistortFrame: setUndistortion has not been called");
    PyrRef e = std::make_shared<PyrHolder>();
    float exposureOut = exposure;
    int rc = ldso_pyr_create(device_, wG[0], hG[0], pyrLevelsUsed, &e->p);
    if (rc == LDSO_OK) rc = ldso_undist_frame(undist_, raw, bytesPerPixel, exposure, factor, e->p, &exposureOut);
    throwOn(rc, "ldso_pyr_create / ldso_undist_frame");
    if (hostIrradiance) {          // the holder's host copy only when somebody wants the image on the host
        e->irradiance.resize((size_t) wG[0] * hG[0]);
        throwOn(ldso_undist_get(undist_, e->irradiance.data()), "ldso_undist_get");
        memcpy(hostIrradiance, e->irradiance.data(), e->irradiance.size() * sizeof(float));
    }
    pyramids_.registerUndistorted(frameId, e, pyramidsBuilt);
    return exposureOut;
}

void GpuBackend::getPyramidLevel(const shared_ptr<FrameHessian> &fh, int lvl, float *out) {
    PyrRef pr = pyramidOf(fh);
    throwOn(ldso_pyr_get_level(pr->p, lvl, out), "ldso_pyr_get_level");
}

// ------------------------------------------------------------------------------------------------------------------------------------
// Images: FrameHessian::dIp[0] of a key frame goes to the device once, when the frame first appears in the window; its slot is
// recycled when the frame has left (FullSystem::marginalizeFrame).
// ------------------------------------------------------------------------------------------------------------------------------------
void GpuBackend::syncImageSlots(FullSystem &fs, std::vector<int32_t> &slots) {
    std::set<unsigned long> live;
    for (auto &fr : fs.frames) live.insert(fr->id);
    for (size_t s = 0; s < slotOwner_.size(); s++)
        if (slotOwner_[s] >= 0 && !live.count((unsigned long) slotOwner_[s])) { slotOf_.erase((unsigned long) slotOwner_[s]); slotOwner_[s] = -1; if (s < slotPyr_.size()) slotPyr_[s].reset(); }
    slots.clear();
    for (auto &fr : fs.frames) {
        FrameHessian *fh = fr->frameHessian.get();
        auto it = slotOf_.find(fr->id);
        if (it == slotOf_.end()) {
            size_t s = 0;
            while (s < slotOwner_.size() && slotOwner_[s] >= 0) s++;
            if (s == slotOwner_.size()) throw std::runtime_error("GpuBackend: more key frames than maxFrames");
            if (useDevicePyramids && fr->frameHessian->frame) {      // zero-copy: level 0 of the frame's pyramid, held for as long as the slot names it
                PyrRef pr = pyramidOf(fr->frameHessian);
                throwOn(ldso_ba_set_image_pyramid(ba_, (int) s, pr->p), "ldso_ba_set_image_pyramid");
                if (slotPyr_.size() < slotOwner_.size()) slotPyr_.resize(slotOwner_.size());
                slotPyr_[s] = pr;
            } else throwOn(ldso_ba_set_image(ba_, (int) s, (const float *) fh->dIp[0]), "ldso_ba_set_image");      // Vec3f AoS (I, dx, dy): a straight copy
            slotOwner_[s] = (long) fr->id; it = slotOf_.emplace(fr->id, (int) s).first;
        }
        slots.push_back(it->second);
    }
}

}  // namespace ldso
