// Driver around the LDSO sources' own CoarseInitializer::setFirst, makePixelStatus and CoarseInitializer::makeNN, for recording
// tests/golden/ref_init_first.npz (scripts/golden/make_ref_init_first.py has the build line).  Our own code: it only calls the library.
// makeNN is a private member of CoarseInitializer; its header (alone: what it includes is read before) is read with `private` opened.
#include "NumTypes.h"
#include "Settings.h"
#include "Frame.h"
#include "Feature.h"
#include "Camera.h"
#include "frontend/PixelSelector2.h"
#include "frontend/nanoflann.h"
#define private public
#include "frontend/CoarseInitializer.h"
#undef private
#include "internal/GlobalCalib.h"
#include "internal/FrameHessian.h"
#include "internal/CalibHessian.h"
#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>

using namespace ldso;
using namespace ldso::internal;

struct IfFrame { shared_ptr<Camera> cam; shared_ptr<Frame> fr; };

extern "C" {

void if_init(int w, int h, int levels) {
    Eigen::Matrix3f K = Eigen::Matrix3f::Identity(); K(0, 2) = w / 2.0f; K(1, 2) = h / 2.0f;
    setGlobalCalib(w, h, K);
    pyrLevelsUsed = levels;
    for (int l = 0; l < levels; l++) { wG[l] = w >> l; hG[l] = h >> l; }
    setting_enableLoopClosing = false;
}

// makeImages of `color` without a response table; the rows of absSquaredGrad[1], [2] that makeImages never writes are zeroed (read by makeMaps)
void *if_frame(const float *color, const float *calib4) {
    const int w = wG[0], h = hG[0];
    IfFrame *F = new IfFrame();
    F->cam.reset(new Camera(calib4[0], calib4[1], calib4[2], calib4[3]));
    F->cam->CreateCH(F->cam);
    F->fr.reset(new Frame());
    F->fr->CreateFH(F->fr);
    std::vector<float> c(color, color + (size_t) w * h);
    F->fr->frameHessian->makeImages(c.data(), nullptr);
    for (int l = 1; l < std::min(3, pyrLevelsUsed); l++) for (int x = 0; x < wG[l]; x++) F->fr->frameHessian->absSquaredGrad[l][x + (hG[l] - 1) * wG[l]] = 0;
    return F;
}
void if_frame_free(void *f) { delete (IfFrame *) f; }

int if_get_sparsity() { return sparsityFactor; }
void if_set_sparsity(int s) { sparsityFactor = s; }

// makePixelStatus on level lvl from the current sparsityFactor; map: wG[lvl] * hG[lvl] bytes
int if_pixel_status(void *f, int lvl, float desired, int recsLeft, float THFac, unsigned char *map) {
    IfFrame *F = (IfFrame *) f;
    const int n = wG[lvl] * hG[lvl];
    bool *m = new bool[n];
    const int r = makePixelStatus(F->fr->frameHessian->dIp[lvl], m, wG[lvl], hG[lvl], desired, recsLeft, THFac);
    for (int i = 0; i < n; i++) map[i] = m[i] ? 1 : 0;
    delete[] m;
    return r;
}

void *if_initializer() { return new CoarseInitializer(wG[0], hG[0]); }
void if_initializer_free(void *c) { delete (CoarseInitializer *) c; }
void if_set_first(void *c, void *f, int *numPoints) {
    IfFrame *F = (IfFrame *) f;
    CoarseInitializer *ci = (CoarseInitializer *) c;
    ci->setFirst(F->cam->mpCH, F->fr->frameHessian);
    for (int l = 0; l < pyrLevelsUsed; l++) numPoints[l] = ci->numPoints[l];
}
// the members setFirst and makeNN define: fields [n][8] = u, v, idepth, iR, energy[2] ... see the script; nb [n][10], nbd [n][10], par [n], pard [n]
void if_points(void *c, int lvl, float *fields, int *good, int *nb, float *nbd, int *par, float *pard) {
    CoarseInitializer *ci = (CoarseInitializer *) c;
    for (int i = 0; i < ci->numPoints[lvl]; i++) {
        const Pnt &p = ci->points[lvl][i];
        float *q = fields + 10 * i;
        q[0] = p.u; q[1] = p.v; q[2] = p.idepth; q[3] = p.iR; q[4] = p.energy[0]; q[5] = p.energy[1]; q[6] = p.lastHessian; q[7] = p.lastHessian_new;
        q[8] = p.my_type; q[9] = p.outlierTH;
        good[i] = p.isGood ? 1 : 0;
        for (int k = 0; k < 10; k++) { nb[10 * i + k] = p.neighbours[k]; nbd[10 * i + k] = p.neighboursDist[k]; }
        par[i] = p.parent; pard[i] = p.parentDist;
    }
}

// makeNN on positions handed in: uv[l] = n[l] pairs.  Out per level: neighbours, neighboursDist, parent, parentDist as makeNN leaves them.
void if_make_nn(int levels, const float *const *uv, const int *n, int *const *nb, float *const *nbd, int *const *par, float *const *pard) {
    const int keep = pyrLevelsUsed;
    pyrLevelsUsed = levels;
    {
    CoarseInitializer ci(wG[0], hG[0]);          // constructor and destructor walk pyrLevelsUsed levels
    for (int l = 0; l < levels; l++) {
        ci.points[l] = new Pnt[n[l]];
        ci.numPoints[l] = n[l];
        for (int i = 0; i < n[l]; i++) { ci.points[l][i].u = uv[l][2 * i]; ci.points[l][i].v = uv[l][2 * i + 1]; }
    }
    ci.makeNN();
    for (int l = 0; l < levels; l++)
        for (int i = 0; i < n[l]; i++) {
            const Pnt &p = ci.points[l][i];
            for (int k = 0; k < 10; k++) { nb[l][10 * i + k] = p.neighbours[k]; nbd[l][10 * i + k] = p.neighboursDist[k]; }
            par[l][i] = p.parent; pard[l][i] = p.parentDist;
        }
    }
    pyrLevelsUsed = keep;
}

// the squared distances findNeighbors returns, which makeNN turns into weights and drops: the same tree type, built the same way, asked the same questions
void if_nn_distances(int n, const float *uv, int nq, const float *q, int k, int *idx, float *dist) {
    typedef nanoflann::KDTreeSingleIndexAdaptor<nanoflann::L2_Simple_Adaptor<float, FLANNPointcloud>, FLANNPointcloud, 2> KDTree;
    std::vector<Pnt> pts(n);
    for (int i = 0; i < n; i++) { pts[i].u = uv[2 * i]; pts[i].v = uv[2 * i + 1]; }
    FLANNPointcloud pc(n, pts.data());
    KDTree tree(2, pc, nanoflann::KDTreeSingleIndexAdaptorParams(5));
    tree.buildIndex();
    nanoflann::KNNResultSet<float, int, int> rs(k);
    for (int i = 0; i < nq; i++) {
        rs.init(idx + (size_t) i * k, dist + (size_t) i * k);
        Vec2f pt(q[2 * i], q[2 * i + 1]);
        tree.findNeighbors(rs, (float *) &pt, nanoflann::SearchParams());
    }
}

// median milliseconds of `reps` setFirst calls on one initialiser, sparsityFactor reset to `sparsity` before each
double if_time_set_first(void *c, void *f, int sparsity, int reps) {
    IfFrame *F = (IfFrame *) f;
    CoarseInitializer *ci = (CoarseInitializer *) c;
    std::vector<double> t;
    for (int r = 0; r < reps; r++) {
        sparsityFactor = sparsity;
        auto t0 = std::chrono::steady_clock::now();
        ci->setFirst(F->cam->mpCH, F->fr->frameHessian);
        t.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    std::sort(t.begin(), t.end());
    return t[t.size() / 2];
}

}
