// immature_record.h — the ImmaturePoint constructor (reference src/internal/ImmaturePoint.cc:14-38) as one device function: what features.hip and
// pixel_select.hip write for every new point of a key frame.  Every float expression keeps the reference's operand order (-ffp-contract=off).
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/ldso_window.h"

// getInterpolatedElement33BiLin (GlobalFuncs.h:186-207); a tap outside the image gives NaN
static __device__ __forceinline__ void feat_interp33(const float *img, float x, float y, int w, int h, float &c, float &gx, float &gy) {
    const int ix = (int) x, iy = (int) y;
    if (ix < 0 || iy < 0 || ix + 1 >= w || iy + 1 >= h) { c = gx = gy = __int_as_float(0x7fc00000); return; }
    const float *bp = img + 3 * ((size_t) iy * w + ix);
    const float tl = bp[0], tr = bp[3], bl = bp[3 * w], br = bp[3 * w + 3];
    const float dx = x - ix, dy = y - iy;
    const float topInt = dx * tr + (1 - dx) * tl, botInt = dx * br + (1 - dx) * bl;
    const float leftInt = dy * bl + (1 - dy) * tl, rightInt = dy * br + (1 - dy) * tr;
    c = dx * rightInt + (1 - dx) * leftInt; gx = rightInt - leftInt; gy = botInt - topInt;
}

// the record of a point at (u, v) of level 0 `img` (12-byte pixels); bad = true when a colour is not finite (energyTH = NaN, :28-31)
static __device__ __forceinline__ ldso_immature_t imm_record(const float *img, float u, float v, int w, int h, int hostIndex, bool &bad) {
    ldso_immature_t q;
    memset(&q, 0, sizeof(q));
    q.u = u; q.v = v;
    const int ox[8] = {0, -1, 1, -2, 0, 2, -1, 0}, oy[8] = {-2, -1, -1, 0, 0, 0, 1, 2};               // staticPattern[8], Setting.cc:221
    float g00 = 0, g01 = 0, g10 = 0, g11 = 0;
    q.energyTH = 8 * 12.0f * 12.0f;                                // patternNum * setting_outlierTH
    q.energyTH *= 1.0f * 1.0f;                                     // setting_overallEnergyTHWeight^2
    for (int k = 0; k < 8; k++) {
        float c, gx, gy;
        feat_interp33(img, u + ox[k], v + oy[k], w, h, c, gx, gy);
        q.color[k] = c;
        if (!isfinite(c)) { q.energyTH = __int_as_float(0x7fc00000); bad = true; break; }             // :28-31
        g00 += gx * gx; g01 += gx * gy; g10 += gy * gx; g11 += gy * gy;
        q.weights[k] = sqrtf(2500.0f / (2500.0f + (gx * gx + gy * gy)));                              // setting_outlierTHSumComponent = 50 * 50
    }
    q.gradH[0] = g00; q.gradH[1] = g01; q.gradH[2] = g10; q.gradH[3] = g11;
    q.idepth_min = 0; q.idepth_max = __int_as_float(0x7fc00000); q.quality = 10000;
    q.lastTraceStatus = LDSO_IPS_UNINITIALIZED; q.lastTraceUV[0] = -1; q.lastTraceUV[1] = -1;
    q.host = hostIndex;
    return q;
}
