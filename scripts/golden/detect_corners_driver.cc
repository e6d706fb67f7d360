// Driver around the LDSO sources' own FeatureDetector::DetectCorners and ImmaturePoint constructor, for recording
// tests/golden/ref_detect_corners.npz (scripts/golden/make_ref_detect_corners.py has the build line).  Our own code: it only calls the library.
#include "Frame.h"
#include "Feature.h"
#include "Camera.h"
#include "Settings.h"
#include "frontend/FeatureDetector.h"
#include "internal/GlobalCalib.h"
#include "internal/FrameHessian.h"
#include "internal/CalibHessian.h"
#include "internal/ImmaturePoint.h"
#include <chrono>
#include <cstring>
#include <vector>

using namespace ldso;
using namespace ldso::internal;

namespace ldso { extern int bit_pattern_31_[256 * 4]; }

extern "C" {

void gd_pattern(int *out) { memcpy(out, ldso::bit_pattern_31_, sizeof(int) * 1024); }

// color: w*h irradiance values; B: 256-entry response table or NULL (identity, no gamma weighting); feat [cap][6] = u, v, score, isCorner, angle, dropped;
// desc [cap][32]; imm [cap][21] = color[8], weights[8], gradH[4], energyTH.  Returns the number of features; *n_corners = DetectCorners' return value;
// *ms = milliseconds per DetectCorners call (median of `reps`, 0 when reps == 0).
int gd_detect(int w, int h, const float *color, const float *B, int n, int cap, float *feat, unsigned char *desc, float *imm, int *n_corners, int reps, double *ms) {
    Eigen::Matrix3f K = Eigen::Matrix3f::Identity(); K(0, 2) = w / 2.0f; K(1, 2) = h / 2.0f;
    setGlobalCalib(w, h, K);
    pyrLevelsUsed = 1;
    setting_enableLoopClosing = false;
    setting_gammaWeightsPixelSelect = 1;
    shared_ptr<Camera> cam(new Camera(1, 1, w / 2.0, h / 2.0));
    cam->CreateCH(cam);
    if (B) for (int i = 0; i < 256; i++) cam->mpCH->B[i] = B[i];
    shared_ptr<CalibHessian> noCalib;
    shared_ptr<Frame> fr(new Frame());
    fr->CreateFH(fr);
    std::vector<float> c(color, color + (size_t) w * h);
    fr->frameHessian->makeImages(c.data(), B ? cam->mpCH : noCalib);
    FeatureDetector det;
    if (ms) *ms = 0;
    if (reps > 0) {
        std::vector<double> t;
        for (int r = 0; r < reps; r++) {
            fr->features.clear();
            auto t0 = std::chrono::steady_clock::now();
            det.DetectCorners(n, fr);
            t.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        }
        std::sort(t.begin(), t.end());
        *ms = t[t.size() / 2];
        fr->features.clear();
    }
    *n_corners = det.DetectCorners(n, fr);
    int k = 0;
    for (auto &f : fr->features) {
        if (k >= cap) break;
        float *o = feat + 6 * k;
        o[0] = f->uv[0]; o[1] = f->uv[1]; o[2] = f->score; o[3] = f->isCorner ? 1 : 0; o[4] = f->angle; o[5] = 0;
        memcpy(desc + 32 * k, f->descriptor, 32);
        shared_ptr<ImmaturePoint> ip(new ImmaturePoint(fr, f, 1, cam->mpCH));
        float *q = imm + 21 * k;
        memcpy(q, ip->color, 32); memcpy(q + 8, ip->weights, 32);
        q[16] = ip->gradH(0, 0); q[17] = ip->gradH(0, 1); q[18] = ip->gradH(1, 0); q[19] = ip->gradH(1, 1); q[20] = ip->energyTH;
        k++;
    }
    return k;
}

}
