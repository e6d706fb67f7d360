// Driver around the LDSO sources' own Undistort / PhotometricUndistorter, for recording tests/golden/ref_undistort.npz
// (scripts/golden/make_ref_undistort.py has the build line).  Our own code: it only calls the library, hands it an in-memory vignette image
// in place of the two IOWrap readers, and reads the tables its constructors leave.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <fstream>
#include <iostream>
#include <iterator>
#include <map>
#include <memory>
#include <sstream>
#include <string>
#include <vector>
#include <Eigen/Core>
#include "NumTypes.h"
#include "Settings.h"
#include "frontend/ImageAndExposure.h"
#include "frontend/MinimalImage.h"
#include "frontend/ImageRW.h"
// the tables are private / protected members (Undistort.h:55-61, :97-106)
#define private public
#define protected public
#include "frontend/Undistort.h"
#undef private
#undef protected

using namespace ldso;

static std::vector<unsigned short> g_vignette;
static int g_vw = 0, g_vh = 0;

namespace ldso {
namespace IOWrap {
MinimalImage<unsigned short> *readImageBW_16U(std::string) {
    if (g_vignette.empty()) return 0;
    MinimalImage<unsigned short> *m = new MinimalImage<unsigned short>(g_vw, g_vh);
    memcpy(m->data, g_vignette.data(), g_vignette.size() * sizeof(unsigned short));
    return m;
}
MinimalImageB *readImageBW_8U(std::string) { return 0; }
}
}

extern "C" {

void ud_set_vignette(int w, int h, const unsigned short *v) { g_vw = w; g_vh = h; g_vignette.assign(v, v + (size_t) w * h); }

// Undistort::getUndistorterForFile with setting_photometricCalibration = 2 while the tables are built
void *ud_create(const char *calib, const char *gamma, const char *vignette) {
    setting_photometricCalibration = 2;
    return Undistort::getUndistorterForFile(calib, gamma, vignette);
}
void ud_destroy(void *u) { delete (Undistort *) u; }

// info[7] = w, h, wOrg, hOrg, passthrough, GDepth, photometric calibration valid
void ud_info(void *u_, int *info) {
    Undistort *u = (Undistort *) u_;
    info[0] = u->w; info[1] = u->h; info[2] = u->wOrg; info[3] = u->hOrg; info[4] = u->passthrough ? 1 : 0;
    info[5] = u->photometricUndist->GDepth; info[6] = u->photometricUndist->valid ? 1 : 0;
}
// remapX / remapY [w * h], G [GDepth], vignetteMapInv [wOrg * hOrg]; any may be NULL
void ud_tables(void *u_, float *remapX, float *remapY, float *G, float *vignetteMapInv) {
    Undistort *u = (Undistort *) u_;
    const size_t n = (size_t) u->w * u->h, nOrg = (size_t) u->wOrg * u->hOrg;
    if (remapX) memcpy(remapX, u->remapX, n * sizeof(float));
    if (remapY) memcpy(remapY, u->remapY, n * sizeof(float));
    if (G) memcpy(G, u->photometricUndist->G, (size_t) u->photometricUndist->GDepth * sizeof(float));
    if (vignetteMapInv) memcpy(vignetteMapInv, u->photometricUndist->vignetteMapInv, nOrg * sizeof(float));
}
// undistort<unsigned char | unsigned short>(raw, exposure, 0, factor) under the two settings; out [w * h]; returns the result's exposure_time
float ud_run(void *u_, const void *raw, int bytes_per_pixel, float exposure, float factor, int photometricCalibration, int useExposure, float *out) {
    Undistort *u = (Undistort *) u_;
    setting_photometricCalibration = photometricCalibration;
    setting_useExposure = useExposure != 0;
    ImageAndExposure *r;
    if (bytes_per_pixel == 1) { MinimalImage<unsigned char> img(u->wOrg, u->hOrg, (unsigned char *) raw); r = u->undistort<unsigned char>(&img, exposure, 0, factor); }
    else { MinimalImage<unsigned short> img(u->wOrg, u->hOrg, (unsigned short *) raw); r = u->undistort<unsigned short>(&img, exposure, 0, factor); }
    memcpy(out, r->image, (size_t) u->w * u->h * sizeof(float));
    const float e = r->exposure_time;
    delete r;
    return e;
}
// median milliseconds of `reps` undistort<unsigned char> calls (photometricCalibration 2, exposure 1)
double ud_time(void *u_, const unsigned char *raw, int reps) {
    Undistort *u = (Undistort *) u_;
    setting_photometricCalibration = 2;
    setting_useExposure = true;
    MinimalImage<unsigned char> img(u->wOrg, u->hOrg, (unsigned char *) raw);
    std::vector<double> t;
    for (int r = 0; r < reps; r++) {
        auto t0 = std::chrono::steady_clock::now();
        ImageAndExposure *res = u->undistort<unsigned char>(&img, 1.0f, 0, 1.0f);
        t.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        delete res;
    }
    std::sort(t.begin(), t.end());
    return t[t.size() / 2];
}

}
