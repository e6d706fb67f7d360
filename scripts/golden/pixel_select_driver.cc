// Driver around the LDSO sources' own FrameHessian::makeImages, PixelSelector and ImmaturePoint constructor, for recording
// tests/golden/ref_pixel_select.npz (scripts/golden/make_ref_pixel_select.py has the build line).  Our own code: it only calls the library.
// PixelSelector keeps randomPattern, ths, thsSmoothed and select() private; its header (alone: what it includes is read before) is read with `private`
// opened so that they can be recorded.
#include "NumTypes.h"
#include "Settings.h"
#include "Frame.h"
#include "Feature.h"
#include "Camera.h"
#define private public
#include "frontend/PixelSelector2.h"
#undef private
#include "internal/GlobalCalib.h"
#include "internal/FrameHessian.h"
#include "internal/CalibHessian.h"
#include "internal/ImmaturePoint.h"
#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>

using namespace ldso;
using namespace ldso::internal;

struct PsFrame { shared_ptr<Camera> cam; shared_ptr<Frame> fr; shared_ptr<CalibHessian> calib; };

extern "C" {

// the global calibration for w x h; select reads three levels whatever setGlobalCalib's size rule says for a small test image
void ps_init(int w, int h) {
    Eigen::Matrix3f K = Eigen::Matrix3f::Identity(); K(0, 2) = w / 2.0f; K(1, 2) = h / 2.0f;
    setGlobalCalib(w, h, K);
    if (pyrLevelsUsed < 3) { pyrLevelsUsed = 3; for (int l = 1; l < 3; l++) { wG[l] = w >> l; hG[l] = h >> l; } }
    setting_enableLoopClosing = false;
    setting_gammaWeightsPixelSelect = 1;
}

// settings[4] = setting_minGradHistCut, setting_minGradHistAdd, setting_gradDownweightPerLevel, setting_selectDirectionDistribution
void ps_settings(const float *s) { setting_minGradHistCut = s[0]; setting_minGradHistAdd = s[1]; setting_gradDownweightPerLevel = s[2]; setting_selectDirectionDistribution = s[3] != 0; }

// makeImages of `color` (B: 256-entry response table or NULL); then the rows of absSquaredGrad[1] and [2] that makeImages never writes are zeroed
void *ps_frame(const float *color, const float *B) {
    const int w = wG[0], h = hG[0];
    PsFrame *F = new PsFrame();
    F->cam.reset(new Camera(1, 1, w / 2.0, h / 2.0));
    F->cam->CreateCH(F->cam);
    if (B) { for (int i = 0; i < 256; i++) F->cam->mpCH->B[i] = B[i]; F->calib = F->cam->mpCH; }
    F->fr.reset(new Frame());
    F->fr->CreateFH(F->fr);
    std::vector<float> c(color, color + (size_t) w * h);
    F->fr->frameHessian->makeImages(c.data(), F->calib);
    for (int l = 1; l < 3; l++) for (int x = 0; x < wG[l]; x++) F->fr->frameHessian->absSquaredGrad[l][x + (hG[l] - 1) * wG[l]] = 0;
    return F;
}
void ps_frame_free(void *f) { delete (PsFrame *) f; }

void *ps_selector() { return new PixelSelector(wG[0], hG[0]); }
void ps_selector_free(void *s) { delete (PixelSelector *) s; }
void ps_pattern(void *s, unsigned char *out) { memcpy(out, ((PixelSelector *) s)->randomPattern, (size_t) wG[0] * hG[0]); }
void ps_set_potential(void *s, int p) { ((PixelSelector *) s)->currentPotential = p; }
int ps_get_potential(void *s) { return ((PixelSelector *) s)->currentPotential; }

// makeMaps; map: w * h floats; returns its return value
int ps_make_maps(void *s, void *f, float *map, float density, int recursionsLeft, float thFactor) {
    return ((PixelSelector *) s)->makeMaps(((PsFrame *) f)->fr->frameHessian, map, density, recursionsLeft, false, thFactor);
}
// one select pass at `pot` (after makeHists of this frame): counts[3] = (n2, n3, n4)
void ps_select(void *s, void *f, float *map, int pot, float thFactor, int *counts) {
    PixelSelector *S = (PixelSelector *) s;
    shared_ptr<FrameHessian> fh = ((PsFrame *) f)->fr->frameHessian;
    if (fh != S->gradHistFrame) S->makeHists(fh);
    Eigen::Vector3i n = S->select(fh, map, pot, thFactor);
    for (int i = 0; i < 3; i++) counts[i] = n[i];
}
void ps_thresholds(void *s, float *ths, float *thsSmoothed) {
    const int n = (wG[0] / 32) * (hG[0] / 32);
    memcpy(ths, ((PixelSelector *) s)->ths, n * sizeof(float)); memcpy(thsSmoothed, ((PixelSelector *) s)->thsSmoothed, n * sizeof(float));
}

// the raster scan of FullSystem::makeNewTraces for setting_pointSelection == 0 over `map`: imm [cap][23] = u, v, color[8], weights[8], gradH[4], energyTH;
// type [cap] = my_type.  Every constructed point is recorded, those with a non-finite energyTH too.  Returns their number.
int ps_points(void *f, const float *map, int cap, float *imm, float *type) {
    PsFrame *F = (PsFrame *) f;
    int k = 0;
    for (int y = patternPadding + 1; y < hG[0] - patternPadding - 2; y++)
        for (int x = patternPadding + 1; x < wG[0] - patternPadding - 2; x++) {
            const int i = x + y * wG[0];
            if (map[i] == 0) continue;
            if (k >= cap) return -1;
            shared_ptr<Feature> feat(new Feature(x, y, F->fr));
            shared_ptr<ImmaturePoint> ip(new ImmaturePoint(F->fr, feat, map[i], F->cam->mpCH));
            float *q = imm + 23 * k;
            q[0] = feat->uv[0]; q[1] = feat->uv[1];
            memcpy(q + 2, ip->color, 32); memcpy(q + 10, ip->weights, 32);
            q[18] = ip->gradH(0, 0); q[19] = ip->gradH(0, 1); q[20] = ip->gradH(1, 0); q[21] = ip->gradH(1, 1); q[22] = ip->energyTH;
            type[k] = ip->my_type;
            k++;
        }
    return k;
}

// median milliseconds of `reps` makeMaps calls, each on a fresh histogram and from potential `pot`
double ps_time(void *s, void *f, float *map, float density, int pot, int reps) {
    PixelSelector *S = (PixelSelector *) s;
    std::vector<double> t;
    for (int r = 0; r < reps; r++) {
        S->gradHistFrame = nullptr; S->currentPotential = pot;
        auto t0 = std::chrono::steady_clock::now();
        S->makeMaps(((PsFrame *) f)->fr->frameHessian, map, density);
        t.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    std::sort(t.begin(), t.end());
    return t[t.size() / 2];
}

}
