// undistort_px.h — one output pixel of Undistort::undistort<T> (reference src/frontend/Undistort.cc:357-457): the photometric part
// (PhotometricUndistorter::processFrame, :189-227) applied to each of the four source taps, then the bilinear remap (:390-443) in the
// reference's operand order.  Plain C++ without the HIP headers (tests/test_undistort_cpu.py compiles it with g++); the kernel of
// undistort.hip and the CPU tests share this one definition.  All arithmetic is float and nothing may be contracted (-ffp-contract=off).
//
// THE ONE DELIBERATE DIFFERENCE FROM THE REFERENCE: the validity rule of the remap tables (:853-864) reads `iy < wOrg - 1` (not hOrg), so
// for wOrg > hOrg a table can hold rows at or beyond hOrg - 1.  The reference's range check (:428) zeroes nearly all of them; the entry
// xxi == 0 && yyi == hOrg - 1 passes it and reads src[wOrg], src[1 + wOrg] one row past the end of the source image.  Here a pixel is 0
// unless all four taps (xxi, yyi) .. (xxi + 1, yyi + 1) lie inside the wOrg x hOrg image, whatever the tables hold (NaN, huge and negative
// entries included): nothing outside the buffer is ever read.  For every entry the reference computes without over-reading, the bits are the same.
// benchmark_varNoise / benchmark_varBlurNoise (:376-413, :468-555; both 0 in Setting.cc) are out of scope.
#pragma once

#if defined(__HIPCC__)
#define UNDIST_HD __host__ __device__ __forceinline__
#else
#define UNDIST_HD inline
#endif

// which path of processFrame a frame takes
#define UNDIST_PLAIN 0          // calibration invalid, exposure <= 0 or setting_photometricCalibration == 0: factor * raw (:200-202)
#define UNDIST_RESPONSE 1       // G[raw] (:206-208)
#define UNDIST_VIGNETTE 2       // G[raw] * vignetteMapInv (:210-218; an infinite entry is multiplied in as well)

// processFrame for source pixel i; raw: wOrg * hOrg pixels of bpp = 1 or 2 bytes; G needs 256 (bpp 1) or 65536 (bpp 2) entries
static UNDIST_HD float undist_photo(const void *raw, int bpp, int i, const float *G, const float *vignetteMapInv, int mode, float factor) {
    const int v = bpp == 1 ? (int) ((const unsigned char *) raw)[i] : (int) ((const unsigned short *) raw)[i];
    if (mode == UNDIST_PLAIN) return factor * v;
    float d = G[v];
    if (mode == UNDIST_VIGNETTE) d *= vignetteMapInv[i];
    return d;
}

// output pixel for the remap entry (xx, yy) = (remapX[idx], remapY[idx])
static UNDIST_HD float undist_px(const void *raw, int bpp, const float *G, const float *vignetteMapInv, int mode, float factor, float xx, float yy, int wOrg, int hOrg) {
    if (!(xx >= 0)) return 0;                                                        // :416 (a NaN goes here too)
    if (!(xx < (float) wOrg) || !(yy > -1.0f) || !(yy < (float) hOrg)) return 0;      // so that the conversions below are defined
    const int xxi = (int) xx, yyi = (int) yy;
    if (xxi + 1 > wOrg - 1 || yyi < 0 || yyi + 1 > hOrg - 1) return 0;               // all four taps inside the image (covers the range check :428)
    xx -= xxi;
    yy -= yyi;
    const float xxyy = xx * yy;
    const int o = xxi + yyi * wOrg;
    return xxyy * undist_photo(raw, bpp, o + 1 + wOrg, G, vignetteMapInv, mode, factor)
           + (yy - xxyy) * undist_photo(raw, bpp, o + wOrg, G, vignetteMapInv, mode, factor)
           + (xx - xxyy) * undist_photo(raw, bpp, o + 1, G, vignetteMapInv, mode, factor)
           + (1 - xx - yy + xxyy) * undist_photo(raw, bpp, o, G, vignetteMapInv, mode, factor);
}
