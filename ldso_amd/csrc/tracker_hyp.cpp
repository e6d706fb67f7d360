// tracker_hyp.cpp — the motion hypotheses of FullSystem::trackNewCoarse and the choice among their results: host arithmetic only, no device work
// (the batched launch in between is ldso_tr_track_batch, tracker_api.hip).
#include "host_only.h"
#include "lie_dev.h"

// The hypothesis loop of FullSystem::trackNewCoarse (FullSystem.cc:319-356) replayed on the results of ONE
// ldso_tr_track_batch call that ran every try to the end (minRes = NaN): try i is accepted / aborted exactly as the
// sequential loop would have done with the `achievedRes` of the tries before it - a try whose residual on some level exceeds
// 1.5 x achievedRes there counts as aborted at that level (finer levels NaN, trackingIsGood = false), `achievedRes` is taken
// over "always" once one try was good, and the loop stops at the first try with achievedRes[0] < lastCoarseRMSE0 *
// reTrackThreshold.  Pure host function (no device work).  best = -1: tracking failed entirely.
extern "C" int ldso_tr_select_hypothesis(int nhyp, int coarsestLvl, const double *lastResiduals /*nhyp*5*/, const int *ok /*nhyp*/, double lastCoarseRMSE0,
                              double reTrackThreshold, int *best, int *tries_consumed, double achievedRes_out[5]) {
    if (nhyp < 0 || coarsestLvl < 0 || coarsestLvl > 4 || (nhyp > 0 && (!lastResiduals || !ok)) || !best) { ldso_set_error("ldso_tr_select_hypothesis: bad arguments"); return LDSO_E_INVALID; }
    double achieved[5] = {NAN, NAN, NAN, NAN, NAN};
    bool haveOneGood = false;
    int tries = 0, win = -1;
    for (int i = 0; i < nhyp; i++) {
        double lr[5] = {NAN, NAN, NAN, NAN, NAN};
        bool good = ok[i] != 0;
        for (int lvl = coarsestLvl; lvl >= 0; lvl--) {
            lr[lvl] = lastResiduals[i * 5 + lvl];
            if (lr[lvl] > 1.5 * achieved[lvl]) { good = false; break; }          // CoarseTracker.cc:193-200 (false with a NaN threshold)
        }
        tries++;
        if (good && std::isfinite((float) lr[0]) && !(lr[0] >= achieved[0])) { win = i; haveOneGood = true; }
        if (haveOneGood)
            for (int l = 0; l < 5; l++) if (!std::isfinite((float) achieved[l]) || achieved[l] > lr[l]) achieved[l] = lr[l];
        if (haveOneGood && achieved[0] < lastCoarseRMSE0 * reTrackThreshold) break;
    }
    *best = win;
    if (tries_consumed) *tries_consumed = tries;
    if (achievedRes_out) for (int l = 0; l < 5; l++) achievedRes_out[l] = achieved[l];
    return LDSO_OK;
}

// The motion-hypothesis list of FullSystem::trackNewCoarse (FullSystem.cc:189-309) from the worldToCam poses (Frame::getPose()) of the two
// frames before the new one in allFrameHistory (sprelast, slast) and of the tracker's reference key frame (lastF): constant / double / half /
// zero motion, identity, and 3 x 26 small rotations about the constant-motion guess (rotDelta = 0.02, 0.03, 0.04 as the reference's float
// counter produces them; Sophus' SO3 constructor normalises the quaternion (1, +-d, +-d, +-d)).  Pure host function.
static void tr_quat_to_pose(double w, double x, double y, double z, double *T) {
    const double n = sqrt(w * w + x * x + y * y + z * z);
    w /= n; x /= n; y /= n; z /= n;
    const double tx = 2 * x, ty = 2 * y, tz = 2 * z, twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
    T[0] = 1 - (tyy + tzz); T[1] = txy - twz; T[2] = txz + twy; T[3] = 0;
    T[4] = txy + twz; T[5] = 1 - (txx + tzz); T[6] = tyz - twx; T[7] = 0;
    T[8] = txz - twy; T[9] = tyz + twx; T[10] = 1 - (txx + tyy); T[11] = 0;
}
extern "C" int ldso_tr_motion_hypotheses(const double sprelast[12], const double slast[12], const double lastF[12], int poses_valid, double *out, int *n_out) {
    REQ(sprelast && slast && lastF && out && n_out, "ldso_tr_motion_hypotheses: null argument");
    const double I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    if (!poses_valid) { memcpy(out, I, sizeof(I)); *n_out = 1; return LDSO_OK; }       // FullSystem.cc:306-309
    double inv[12], fh_2_slast[12], lastF_2_slast[12], fi[12], cm[12], tmp[12], xi[6], h[12];
    ld::se3_inv(slast, inv); ld::se3_mul(sprelast, inv, fh_2_slast);                    // slast_2_sprelast, "assumed to be the same as fh_2_slast"
    ld::se3_inv(lastF, inv); ld::se3_mul(slast, inv, lastF_2_slast);
    ld::se3_inv(fh_2_slast, fi);
    int n = 0;
    ld::se3_mul(fi, lastF_2_slast, cm); memcpy(out + 12 * n++, cm, 96);                 // constant motion
    ld::se3_mul(fi, cm, tmp); memcpy(out + 12 * n++, tmp, 96);                          // double motion (a frame was skipped)
    ld::se3_log(fh_2_slast, xi); for (int i = 0; i < 6; i++) xi[i] *= 0.5;
    ld::se3_exp(xi, h); ld::se3_inv(h, tmp); ld::se3_mul(tmp, lastF_2_slast, h); memcpy(out + 12 * n++, h, 96);      // half motion
    memcpy(out + 12 * n++, lastF_2_slast, 96);                                          // zero motion
    memcpy(out + 12 * n++, I, 96);                                                      // zero motion from the key frame
    static const int sgn[26][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {-1, 0, 0}, {0, -1, 0}, {0, 0, -1}, {1, 1, 0}, {0, 1, 1}, {1, 0, 1}, {-1, 1, 0}, {0, -1, 1}, {-1, 0, 1},
                                      {1, -1, 0}, {0, 1, -1}, {1, 0, -1}, {-1, -1, 0}, {0, -1, -1}, {-1, 0, -1}, {-1, -1, -1}, {-1, -1, 1}, {-1, 1, -1}, {-1, 1, 1},
                                      {1, -1, -1}, {1, -1, 1}, {1, 1, -1}, {1, 1, 1}};
    for (float rotDelta = 0.02; rotDelta < 0.05; rotDelta += 0.01)
        for (int k = 0; k < 26; k++) {
            double q[12];
            tr_quat_to_pose(1, sgn[k][0] * rotDelta, sgn[k][1] * rotDelta, sgn[k][2] * rotDelta, q);
            ld::se3_mul(cm, q, out + 12 * n++);
        }
    *n_out = n;
    return LDSO_OK;
}
