/*
 * ldso_hip.h — C-ABI of libldso_hip.so: the MI355X (gfx950) implementation of LDSO's windowed
 * photometric bundle-adjustment hot path and CoarseTracker image alignment.
 *
 * The reference has no FFI layer; its boundary is two C++ member functions:
 *     float FullSystem::optimize(int mnumOptIts)                       src/frontend/FullSystem.cc:725
 *     bool  CoarseTracker::trackNewestCoarse(fh, SE3&, AffLight&, int, Vec5)   src/frontend/CoarseTracker.cc:61
 * Each entry point below names the reference function it replaces.  All functions are extern "C",
 * take plain pointers and sizes (layouts: ldso_window.h), return 0 on success or a negative
 * ldso_status code, never throw, and never free caller memory.  Handles are not thread-safe; distinct
 * handles are independent (one BA handle on the mapping thread, tracker handles on the tracking
 * thread, as FullSystem uses them).  Non-finite results are reported as LDSO_E_NONFINITE, the
 * analogue of the reference's isLost path (FullSystem.cc:845-849).
 */
#ifndef LDSO_HIP_H_
#define LDSO_HIP_H_

#include "ldso_window.h"
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

enum ldso_status {
    LDSO_OK = 0,
    LDSO_E_INVALID = -1,      /* bad argument / window exceeds the handle's capacity            */
    LDSO_E_HIP = -2,          /* a HIP runtime call failed (see ldso_last_error)                */
    LDSO_E_NONFINITE = -3,    /* NaN/Inf in energies or the solve (reference: isLost = true)    */
    LDSO_E_UNSUPPORTED = -4,  /* a setting_* mode this implementation does not provide          */
    LDSO_E_NODEVICE = -5      /* no HIP device visible                                          */
};

int ldso_version(void);
const char *ldso_last_error(void);
int ldso_device_count(void);

/* ------------------------------------------------------------------------------------------------
 * Host-side helpers mirroring small reference functions that stay on the CPU.
 * ---------------------------------------------------------------------------------------------- */
/* FrameHessian::setEvalPT (FrameHessian.h:104-109) + setStateZero (FrameHessian.cc:12-42): fills
 * worldToCam_evalPT, state, state_zero and the numeric nullspaces of *f. */
int ldso_frame_set_evalPT(ldso_frame_t *f, const double worldToCam[12], const double state[10]);
/* FrameHessian::getPrior (FrameHessian.h:129-154): writes f->prior from f->frameID and the settings. */
int ldso_frame_set_prior(ldso_frame_t *f, const ldso_settings_t *s);
/* Defaults of src/Setting.cc for every field of ldso_settings_t. */
int ldso_settings_default(ldso_settings_t *s);
/* setGlobalCalib's pyramid rule (GlobalCalib.cc:20-29). */
int ldso_pyr_levels_used(int w, int h);

/* ------------------------------------------------------------------------------------------------
 * FrameHessian::dIp resident in HBM: one image pyramid per frame, built on the device from the raw irradiance
 * (FrameHessian::makeImages, FrameHessian.cc:44-113: level l >= 1 is the 2x2 mean of level l-1, pixels are (I, dx, dy) with
 * central-difference gradients) and shared BY POINTER between the coarse tracker (CoarseTracker.cc:248-256, :636-642: fh->dIp[lvl]),
 * the immature-point tracer (ImmaturePoint.cc:89: frame->dI) and the bundle adjustment (Residuals.cc:84: target->dI) - the
 * reference shares the same host arrays the same way.  4 bytes per pixel cross PCIe once per frame; every consumer below is
 * zero-copy and stream-ordered after the build (hipStreamWaitEvent on the pyramid's event, no host synchronisation).  The caller keeps
 * a pyramid alive while a consumer refers to it (until the consumer's next set_* call for that role / slot).
 * ---------------------------------------------------------------------------------------------- */
typedef struct ldso_pyramid ldso_pyramid_t;
int ldso_pyr_create(int device, int w, int h, int levels, ldso_pyramid_t **out);
int ldso_pyr_destroy(ldso_pyramid_t *p);
/* irradiance: w*h floats on the host / on the device; enqueued on hip_stream (NULL: the default stream) */
int ldso_pyr_make_images(ldso_pyramid_t *p, const float *irradiance, void *hip_stream);
int ldso_pyr_make_images_device(ldso_pyramid_t *p, const void *irradiance_dev, void *hip_stream);
/* device pointer and size of a level ((w>>lvl)*(h>>lvl)*3 floats); ldso_pyr_get_level: test fetch to the host */
int ldso_pyr_level(ldso_pyramid_t *p, int lvl, const void **dev_ptr, int *wl, int *hl);
int ldso_pyr_get_level(ldso_pyramid_t *p, int lvl, float *out);
/* A group of pyramids: FrameHessian::makeImages (FrameHessian.cc:44-113) of the new frames of many sequences on one card.  ldso_pyr_make_images is
 * 2 x levels small launches per pyramid; a group call builds every active member in at most 2 x Lmax launches whatever n (Lmax = the largest level count
 * among them), with the job tables of all levels in one upload.  Every level of every member holds the bytes ldso_pyr_make_images gives it.
 * 1 <= n <= 128 pyramids of one device; sizes and level counts are free.  A pyramid belongs to at most one group and stays usable on its own between
 * group calls; ldso_pyr_destroy of a member is refused while the group lives. */
typedef struct ldso_pyr_group ldso_pyr_group_t;
int ldso_pyr_group_create(ldso_pyramid_t *const *pyramids, int n, ldso_pyr_group_t **out);
int ldso_pyr_group_destroy(ldso_pyr_group_t *g);
/* irradiance: n host pointers (member i: w_i * h_i floats; entries of inactive members are not read), copied straight into the members' own staging
 * images on hip_stream; active: n bytes or NULL = all.  Like the solo entries the call does not wait: every active member's event is recorded behind the
 * last launch, and every consumer (ldso_tr_set_new_frame_pyramid, ldso_trace_set_frame_pyramid, ...) orders itself behind it.  The host images must stay
 * valid until the stream has passed the copies.  LDSO_E_INVALID (a NULL image of an active member, no active member) before anything is enqueued. */
int ldso_pyr_group_make_images(ldso_pyr_group_t *g, const uint8_t *active /* n or NULL */, const float *const *irradiance /* n host pointers */, void *hip_stream);
/* the same from n device pointers */
int ldso_pyr_group_make_images_device(ldso_pyr_group_t *g, const uint8_t *active /* n or NULL */, const void *const *irradiance_dev /* n device pointers */, void *hip_stream);

/* ------------------------------------------------------------------------------------------------
 * Windowed bundle adjustment (EnergyFunctional + the optimisation slice of FullSystem).
 * ---------------------------------------------------------------------------------------------- */
typedef struct ldso_ba ldso_ba_t;

/* Allocate device state for windows up to max_frames x max_points on HIP device `device`. */
int ldso_ba_create(int device, int w, int h, int max_frames, int max_points, ldso_ba_t **out);
int ldso_ba_destroy(ldso_ba_t *h);
/* Run all launches on the caller's hipStream_t (e.g. torch's current stream); NULL = internal stream. */
int ldso_ba_set_stream(ldso_ba_t *h, void *hip_stream);
int ldso_ba_set_settings(ldso_ba_t *h, const ldso_settings_t *s);

/* Upload FrameHessian::dIp[0] (w*h Vec3f AoS: I,dx,dy; FrameHessian.h:169-175) into image slot
 * `slot` (0..max_frames-1).  Done once per new keyframe; slots are recycled on marginalisation. */
int ldso_ba_set_image(ldso_ba_t *h, int slot, const float *dI_level0_host);
/* Same, the pyramid level already being device-resident (zero-copy hand-over, not retained after the
 * next ldso_ba_set_image* on that slot).  A resident window that uses the slot follows the new buffer. */
int ldso_ba_set_image_device(ldso_ba_t *h, int slot, const void *dI_level0_dev);
/* The same slot from the RAW level-0 irradiance (w*h floats): FrameHessian::makeImages level 0 (FrameHessian.cc:44-113: copy +
 * central-difference gradients) runs on the device, 4 instead of 12 bytes per pixel cross PCIe.  ldso_ba_get_image: test fetch. */
int ldso_ba_set_image_raw(ldso_ba_t *h, int slot, const float *irradiance);
/* The slot from level 0 of a resident ldso_pyramid_t (zero-copy, as ldso_ba_set_image_device, ordered after the pyramid's build). */
int ldso_ba_set_image_pyramid(ldso_ba_t *h, int slot, ldso_pyramid_t *pyr);
int ldso_ba_get_image(ldso_ba_t *h, int slot, float *out_w_h_3);

/* K-splits (workgroups) per 16 x 16 tile of the Schur complement in the GN fast path (the device counterpart of AccumulatedSCHessianSSE's per-thread accumulators,
 * AccumulatedSCHessian.cc:53-119: each split owns a range of points and adds its fp32 partial tile into the fp64 system).  8 for a lone window (latency), 4 for the
 * windows of a batch of four or more (throughput).  Two runs agree bit for bit only under the same number. */
int ldso_ba_set_reduce_splits(ldso_ba_t *h, int splits);
/* Describe the window: EnergyFunctional::frames / allPoints / p->residuals after makeIDX
 * (EnergyFunctional.cc:380-401).  image_slot[f] = slot holding frame f's image.  linJ / lin_res_toZeroF
 * (R entries, may be NULL) are read where residuals[i].is_linearized != 0. */
int ldso_ba_set_window(ldso_ba_t *h, int F, const int32_t *image_slot, int P, const ldso_point_t *points,
                       int R, const ldso_residual_t *residuals, const ldso_rawjac_t *linJ, const float *lin_res_toZeroF);
/* The window of the next optimize() as a DELTA against the resident one: what the reference's own maintenance calls do to the window between two key
 * frames, in one call on the order EnergyFunctional::makeIDX produces (EnergyFunctional.cc: insertFrame :32, insertResidual :26, dropResidual :63,
 * removePoint :153, dropPointsF :224, marginalizeFrame :72, makeIDX :380).  Nothing of the surviving points crosses PCIe: their geometry, colours, inverse
 * depths, maxRelBaseline / numGoodResiduals and per-residual state / energy / activity are taken from the resident window on the device.
 *   frame_from[f]  old index of new frame f (old frames that appear nowhere were marginalised; survivors keep their order), -1 = insertFrame (last)
 *   point_from[i]  old row of new point i (old rows that appear nowhere were removed / dropped / marginalised; survivors keep their order),
 *                  -1 - k = the k-th fresh point (insertPoint), numbered in window order
 *   res_mask[i]    bit t: point i has a residual with target frame t (new numbering).  Set where the resident slot is empty = insertResidual (IN, energy 0,
 *                  isNew); clear where it is occupied = dropResidual
 *   fresh[n_fresh], fresh_res[n_fresh_res], fresh_mrb, fresh_ngr   the new points as in ldso_ba_set_window (host = new frame index), their residuals
 *                  point-major and target-ascending with .point = index into fresh, PointHessian::maxRelBaseline / numGoodResiduals
 * Flat residual order of the new window: point-major, target-ascending.  The result equals a fresh ldso_ba_set_window + ldso_ba_set_point_stats of the same
 * objects byte for byte (tests/test_resident_gpu.py); ldso_ba_set_frames / ldso_ba_set_prior follow as after ldso_ba_set_window.  Windows with linearised
 * residuals, shards and the first window of a handle go through ldso_ba_set_window. */
int ldso_ba_update_window(ldso_ba_t *h, int F, const int32_t *image_slot, const int32_t *frame_from, int P, const int32_t *point_from, const uint32_t *res_mask,
                          int n_fresh, const ldso_point_t *fresh, int n_fresh_res, const ldso_residual_t *fresh_res, const float *fresh_mrb,
                          const int32_t *fresh_ngr);
/* The same delta recorded call by call, as the reference edits its window (EnergyFunctional.cc; host-side bookkeeping until the commit, which applies the
 * edit as ONE ldso_ba_update_window and rejects an invalid one without touching the resident window).  Frames and residual targets are named by their index
 * in the RESIDENT window (frames inserted during the edit: the id ldso_ba_insert_frame returns), points by their resident row:
 *   ldso_ba_remove_frame    EnergyFunctional::marginalizeFrame :72 / FullSystem::marginalizeFrame FullSystem.cc:602-645 - the frame leaves, with the residuals
 *                           that target it and the points it hosts (the prior's Schur complement is ldso_ba_marginalize_frame)
 *   ldso_ba_insert_frame    insertFrame :32
 *   ldso_ba_remove_points   removePoint :153, dropPointsF :224, the points marginalizePointsF :165 absorbed
 *   ldso_ba_drop_residuals  dropResidual :63          ldso_ba_add_residuals   insertResidual :26 (IN, energy 0, isNew)
 *   ldso_ba_add_points      insertPoint + its residuals: n points in the layout of ldso_ba_set_window (host / target = frame ids of this edit, residuals[].point =
 *                           index into the call's points), each placed in front of resident row before_row[i] (number of rows = at the end): makeIDX :380 order
 *   ldso_ba_window_commit   surviving frames keep their order, inserted frames follow */
int ldso_ba_window_begin(ldso_ba_t *h);
int ldso_ba_remove_frame(ldso_ba_t *h, int frame_idx);
int ldso_ba_insert_frame(ldso_ba_t *h, int image_slot, int *frame_id_out);
int ldso_ba_remove_points(ldso_ba_t *h, int n, const int32_t *rows);
int ldso_ba_drop_residuals(ldso_ba_t *h, int n, const int32_t *rows, const int32_t *targets);
int ldso_ba_add_residuals(ldso_ba_t *h, int n, const int32_t *rows, const int32_t *targets);
int ldso_ba_add_points(ldso_ba_t *h, int n, const ldso_point_t *points, const int32_t *before_row, int n_res, const ldso_residual_t *residuals,
                       const float *max_rel_baseline, const int32_t *num_good_residuals);
int ldso_ba_window_commit(ldso_ba_t *h);
/* the dimensions of the window the handle holds (what the getters below write: R residual records, P point records, F frames); any pointer may be NULL */
int ldso_ba_get_dims(ldso_ba_t *h, int *F, int *P, int *R);
/* Frame / calibration state (FrameHessian::setState..., CalibHessian::setValue) and the
 * marginalisation prior HM,bM ((8F+4)^2 row-major, (8F+4); NULL = zero).  ldso_ba_set_frames also performs
 * EnergyFunctional::setAdjointsF (EnergyFunctional.cc:431-489) and FullSystem::setPrecalcValues
 * (FullSystem.cc:1423-1431) on the device.  Lifetime of the prior: ldso_ba_set_window resets it to zero (the
 * dimension 8F+4 changes with the window); ldso_ba_set_frames leaves it alone, so the two calls below may
 * come in either order after ldso_ba_set_window. */
int ldso_ba_set_frames(ldso_ba_t *h, const ldso_frame_t *frames, const ldso_calib_t *calib);
int ldso_ba_set_prior(ldso_ba_t *h, const double *HM, const double *bM);
/* Optional, after ldso_ba_set_window: PointHessian::maxRelBaseline / numGoodResiduals of the P points as the reference's objects hold them
 * (they persist across optimize() calls: FullSystem.cc:1521-1536, AccumulatedSCHessian.cc:14-21).  Without the call both start at zero. */
int ldso_ba_set_point_stats(ldso_ba_t *h, const float *maxRelBaseline, const int32_t *numGoodResiduals);

/* Multi-GPU: this rank owns points [begin,end) of the window (whole points only).
 * reduce_buf_dev is a caller-allocated device buffer of ldso_ba_reduce_doubles() doubles that the
 * caller all-reduces (sum) between ldso_ba_reduce_local() and ldso_ba_solve_reduced(). */
int ldso_ba_set_shard(ldso_ba_t *h, int point_begin, int point_end);
/* Points per workgroup of the fused linearisation kernel: 0 (default) = as few as keep one window's grid within one workgroup per CU (the
 * latency of a single window); n > 0 (multiple of 4) = fixed chunks of n points (ldso_ba_batch_create applies its own to the windows of a
 * batch: many windows fill the launch, a workgroup then takes several points per wavefront).  The fp32 partial sums of the top Hessian
 * are formed per chunk: two handles agree bit for bit only under the same chunking. */
int ldso_ba_set_chunk_points(ldso_ba_t *h, int points_per_workgroup);
int ldso_ba_get_chunk_points(ldso_ba_t *h, int *points_per_workgroup, int *workgroups);
/* The chunks themselves: ends[i] = one past the last point of chunk i (ascending, the last one = number of points; chunks never straddle a host frame -
 * a cut is added at every host boundary).  ldso_ba_batch_create cuts the windows of a batch UNEVENLY (every workgroup of the batched launch gets the same
 * amount of work, round 6); ldso_ba_get_chunk_cuts returns the cuts in force (n_out = their number; ends may be NULL to ask for the count),
 * ldso_ba_set_chunk_cuts applies them to another handle holding a window of the same shape (n = 0: back to ldso_ba_set_chunk_points' policy). */
int ldso_ba_get_chunk_cuts(ldso_ba_t *h, int32_t *ends, int cap, int *n_out);
int ldso_ba_set_chunk_cuts(ldso_ba_t *h, const int32_t *ends, int n);
size_t ldso_ba_reduce_doubles(ldso_ba_t *h);

/* --- the optimisation slice, one entry per reference function ------------------------------------ */
/* FullSystem::optimize preamble (FullSystem.cc:735-755): activeResiduals = !isLinearized, resetOOB. */
int ldso_ba_collect_active(ldso_ba_t *h);
/* FullSystem::linearizeAll(fix) (FullSystem.cc:1442-1492) = PointFrameResidual::linearize on every
 * active residual (Residuals.cc:13-214) + setNewFrameEnergyTH (:1762-1793); with fix != 0 also
 * applyRes, maxRelBaseline/numGoodResiduals and removal flags.  energy_out = Vec3[0]. */
int ldso_ba_linearize_all(ldso_ba_t *h, int fixLinearization, double *energy_out);
/* FullSystem::applyRes_Reductor(true) (FullSystem.cc:1706-1709) -> PointFrameResidual::applyRes. */
int ldso_ba_apply_res(ldso_ba_t *h);
/* FullSystem::backupState (FullSystem.cc:1625-1673, non-momentum branch). */
int ldso_ba_backup_state(ldso_ba_t *h);
/* FullSystem::solveSystem (FullSystem.cc:1433-1440) -> EnergyFunctional::solveSystemF
 * (EnergyFunctional.cc:240-351): accumulate A/L/SC, stitch, solve, orthogonalise, resubstitute. */
int ldso_ba_solve_system(ldso_ba_t *h, int iteration, double lambda);
/* FullSystem::doStepFromBackup(1,1,1,1,1) (FullSystem.cc:1546-1623) incl. setPrecalcValues. */
int ldso_ba_do_step(ldso_ba_t *h, int *canbreak_out);
/* FullSystem::loadSateBackup (FullSystem.cc:1675-1692). */
int ldso_ba_load_state_backup(ldso_ba_t *h);
/* EnergyFunctional::calcMEnergyF and calcLEnergyF_MT (EnergyFunctional.cc:353-378, 627-682) at the current state: the prior /
 * linearised-residual energies of the LM accept test (FullSystem.cc:805-826).  ldso_ba_optimize uses them when
 * settings.forceAcceptStep == 0 (accept / loadSateBackup + lambda *= 100, one host round trip per stage). */
int ldso_ba_calc_lm_energies(ldso_ba_t *h, double *energy_M, double *energy_L);
/* FullSystem::optimize(mnumOptIts) (FullSystem.cc:725-864) with everything on the device and no host
 * synchronisation inside the loop.  force_all_iterations != 0 ignores `canbreak` (BASELINE config C3).
 * rmse_out = the function's return value; iterations_out = GN iterations executed. */
int ldso_ba_optimize(ldso_ba_t *h, int mnumOptIts, int force_all_iterations, float *rmse_out, int *iterations_out);
/* EnergyFunctional::marginalizePointsF (EnergyFunctional.cc:165-222) for the points with flags[p] != 0 (the caller's
 * PS_MARGINALIZED decision, FullSystem.cc:1208-1270), fused with the reset + re-linearise + fixLinearizationF pass that
 * FullSystem::flagPointsForRemoval runs on exactly these points (FullSystem.cc:1241-1250, Residuals.cc:216-242):
 * HM += margWeightFac (M - Msc), bM += margWeightFac (Mb - Mbsc) on the device (and copied to HM_out / bM_out when
 * non-NULL, (8F+4)^2 row-major and 8F+4 doubles).  The window's applied state is unchanged; the caller removes the
 * points (next ldso_ba_set_window) and calls EnergyFunctional::marginalizeFrame on the returned prior as before. */
int ldso_ba_marginalize_points(ldso_ba_t *h, const int32_t *flags, double *HM_out, double *bM_out);
/* EnergyFunctional::marginalizeFrame (EnergyFunctional.cc:72-151) on the device prior H_M / b_M (as set by
 * ldso_ba_set_prior or left by ldso_ba_marginalize_points) with the frame's prior / delta_prior: out = prior of the window
 * without frame `frame_idx`, (8(F-1)+4)^2 row-major and 8(F-1)+4 doubles. */
int ldso_ba_marginalize_frame(ldso_ba_t *h, int frame_idx, double *HM_out, double *bM_out);
/* Point activation: FullSystem::optimizeImmaturePoint (FullSystem.cc:892-1010; ImmaturePoint::linearizeResidual,
 * ImmaturePoint.cc:312-381) for n immature points against the key frames of the resident window (its images, calibration and
 * CURRENT poses, i.e. after ldso_ba_set_frames): up to gn_iterations LM steps on the inverse depth from the middle of
 * [idepth_min, idepth_max]; min_obs = 1, min_idepth_hessian = setting_minIdepthH_act (100), gn_iterations =
 * setting_GNItsOnPointActivation (3) in the reference (FullSystem.cc:1204).  out[i].ok says whether the point is created;
 * out[i].res_state[t] == 0 lists the target frames that get a PointFrameResidual. */
int ldso_ba_activate_points(ldso_ba_t *h, int n, const ldso_immature_t *points, int min_obs, float min_idepth_hessian, int gn_iterations,
                            ldso_activation_t *out);
/* The density controller at the head of FullSystem::activatePointsMT (FullSystem.cc:1054-1073): currentMinActDist moved by how far ef->nPoints is from
 * setting_desiredPointDensity - the reference's mixed if / else-if ladder as written - and clamped to [0, 4].  Host only. */
int ldso_act_update_min_dist(float current, int nPoints, float desiredDensity, float *out);
/* Which immature points get activated: CoarseDistanceMap::makeDistanceMap (CoarseTracker.cc:686-721, growDistBFS :723-811) from the seeds, then the greedy,
 * order-dependent loop of FullSystem::activatePointsMT (FullSystem.cc:1088-1152) with addIntoDistFinal (CoarseTracker.cc:813-818) for every accepted candidate.
 * The map is level 1 of the handle's image size.  points / my_type (ImmaturePoint::my_type, ImmaturePoint.h:114): the candidates in the reference's iteration
 * order (host frames in window order, features in vector order); points[i].host and seeds[i].host index KRKi [n_hosts][9] / Kt [n_hosts][3] - K[1] * R * Ki[0]
 * and K[1] * t of host -> newest frame (FullSystem.cc:1093-1094, the convention of ldso_trace_on at pyramid level 1) - and host_flagged [n_hosts]
 * (FrameHessian::flaggedForMarginalization).  decision_out [n]: LDSO_ACT_*; selected_out [n]: the first *n_selected_out entries are the indices of the
 * SELECTED candidates in the order the reference pushes them into toOptimize. */
int ldso_ba_select_candidates(ldso_ba_t *h, int n_seeds, const ldso_act_seed_t *seeds, int n, const ldso_immature_t *points, const float *my_type, int n_hosts,
                              const float *KRKi, const float *Kt, const int32_t *host_flagged, float currentMinActDist, float minTraceQuality,
                              int32_t *decision_out, int32_t *selected_out, int *n_selected_out);
/* The same selection followed by ldso_ba_activate_points on the selected list (FullSystem.cc:1080-1164) in one enqueue: the list stays on the device, the host
 * waits once.  Preconditions of ldso_ba_activate_points (resident window, its images and current poses; n_hosts = its frame count).  out [n]: out[k] is the
 * record of candidate selected_out[k] for k < *n_selected_out, identical to what ldso_ba_activate_points returns for that list. */
int ldso_ba_select_activate_points(ldso_ba_t *h, int n_seeds, const ldso_act_seed_t *seeds, int n, const ldso_immature_t *points, const float *my_type, int n_hosts,
                                   const float *KRKi, const float *Kt, const int32_t *host_flagged, float currentMinActDist, float minTraceQuality, int min_obs,
                                   float min_idepth_hessian, int gn_iterations, int32_t *decision_out, int32_t *selected_out, int *n_selected_out,
                                   ldso_activation_t *out);
/* Debug: CoarseDistanceMap::fwdWarpedIDDistFinal as the last selection on this handle left it, (w >> 1) * (h >> 1) floats: 0..39 and 1000. */
int ldso_ba_get_distance_map(ldso_ba_t *h, float *out_w1_h1);
/* Asynchronous variant used by bench.py: enqueue `iters` Gauss-Newton iterations (solveSystem +
 * doStepFromBackup + linearizeAll + applyRes) on the handle's stream and return immediately.  The launch sequence of a call is captured into a HIP graph the
 * first time and replayed when the same call comes again (same window, settings, stream, first iteration and count: the key is a hash of every launch
 * argument); LDSO_GN_GRAPHS=0 in the environment at handle creation: launch by launch.  Same kernels, same arguments, same order either way. */
int ldso_ba_enqueue_gn(ldso_ba_t *h, int first_iteration, int iters);
int ldso_ba_sync(ldso_ba_t *h);

/* multi-GPU split of solveSystemF: local accumulate+stitch into the reduce buffer, then (after the
 * caller's all-reduce) the replicated solve + step + precalc. */
/* Multi-GPU fast path (what bench.py --gpus N runs): the all-reduce buffer IS the HFinal / bFinal accumulator of the
 * 3-launch iteration.  Layout, ldso_ba_gn_reduce_doubles() doubles: [HFinal lower triangle (8F+4)^2 | bFinal 8F+4 |
 * 8 scalar sums | P newest-frame energy candidates (value+1)].  Per iteration: ldso_ba_gn_reduce_local (rank-local
 * accumulate; the H_M / prior / lambda terms are added by the rank that owns point 0) -> all-reduce(sum) by the caller
 * -> ldso_ba_gn_solve_reduced (replicated solve + step + linearizeAll of the shard + applyRes).  lambda as solveSystemF. */
size_t ldso_ba_gn_reduce_doubles(ldso_ba_t *h);
int ldso_ba_gn_reduce_local(ldso_ba_t *h, void *reduce_buf_dev, double lambda);
int ldso_ba_gn_solve_reduced(ldso_ba_t *h, const void *reduce_buf_dev, int iteration, double lambda);
/* Batched windows (one 7-keyframe window is tiny for an MI355X): the forced Gauss-Newton iteration of n
 * INDEPENDENT windows (several agents, sequences or hypotheses) with three launches per iteration for the whole batch
 * (k_reduce_batch -> k_gn_solve_batch -> k_linearize_batch).  Per-window arithmetic is that of ldso_ba_enqueue_gn.  The handles
 * share one device and one stream, hold windows of the same slot-table width (all F <= 8 or all F in 9..16) without linearised
 * residuals, and have been brought to the same stage (window set, ldso_ba_linearize_all + ldso_ba_apply_res).  Results are
 * fetched per handle as usual. */
typedef struct ldso_ba_batch ldso_ba_batch_t;
int ldso_ba_batch_create(ldso_ba_t *const *handles, int n, ldso_ba_batch_t **out);
int ldso_ba_batch_reduce_splits(ldso_ba_batch_t *b, int *splits);          /* K-splits per Schur tile the batch reduces its windows with (ldso_ba_set_reduce_splits) */
/* The chunking ldso_ba_batch_create applies, as host logic without a device (tests/test_batch_balance_cpu.py): n_seg runs of points that may share a chunk (one window's
 * points of one host frame each, in launch order), n_wg workgroups, a chunk costing chunk_cost points on top of its own -> chunk_end[] (cumulative point counts, ascending,
 * a chunk never spans two segments) and wg_first_chunk[n_wg + 1] (workgroup w works through the chunks [wg_first_chunk[w], wg_first_chunk[w + 1])), chosen so that the
 * largest workgroup load (points + chunk_cost per chunk) is minimal for this greedy cut (bisection on the budget, *budget_out).  Returns the number of chunks. */
int ldso_ba_balance_chunks(int n_seg, const int32_t *seg_points, int n_wg, int chunk_cost, int32_t *chunk_end, int cap, int32_t *wg_first_chunk, int64_t *budget_out);
/* ldso_ba_batch_enqueue_gn needs every window at the same ping-pong parity ("the same stage") and refuses otherwise - also after a ldso_ba_batch_optimize
 * whose windows stopped at iterations of different parity. */
int ldso_ba_batch_enqueue_gn(ldso_ba_batch_t *b, int first_iteration, int iters);
/* FullSystem::optimize(mnumOptIts) for every window of the batch: per window exactly what ldso_ba_optimize(handle, mnumOptIts, force_all_iterations, ...) gives on
 * that handle alone (resetOOB preamble, lambda = 1e-1 * 0.25^it, the window's own iteration cap - 15 below four key frames unless forced - and device-side
 * canbreak exit, the tail with linearizeAll(true), energy log, rmse), with a number of launches that does not depend on n and one host synchronisation at the end.
 * The windows need not be at the same parity, and stop at iterations of their own.  rmse_out / iterations_out / status_out: n entries each, any of them may
 * be NULL; status_out[i] is LDSO_OK or LDSO_E_NONFINITE by the test of ldso_ba_optimize.  Returns LDSO_OK when every window is, LDSO_E_NONFINITE when at least
 * one is not (the others' results are unaffected), other codes as usual.  Afterwards every handle is where ldso_ba_optimize would have left it: the per-handle
 * getters, ldso_ba_get_energy_log, ldso_ba_marginalize_points / _frame and a second ldso_ba_batch_optimize work on it.
 * Beyond ldso_ba_batch_create's conditions: every window has at least 2 key frames and at most 8 (the 8-slot table). */
int ldso_ba_batch_optimize(ldso_ba_batch_t *b, int mnumOptIts, int force_all_iterations, float *rmse_out /*n*/, int *iterations_out /*n*/, int *status_out /*n*/);
/* The two steps FullSystem::makeKeyFrame runs right behind optimize(), for every window of the batch, with a number of launches and host <-> device copies that
 * does not depend on n (three launches for the points, one for the frames; one upload, one download and one host synchronisation each).
 * ldso_ba_batch_marginalize_points: EnergyFunctional::marginalizePointsF (EnergyFunctional.cc:165-222; FullSystem.cc:527) with the re-linearise + fixLinearizationF
 * pass of FullSystem::flagPointsForRemoval (FullSystem.cc:1241-1250) - per window exactly what ldso_ba_marginalize_points(handle_i, flags[i], ...) gives: flags[i] holds
 * P_i entries; the applied state is unchanged, the handle's prior becomes H_M += margWeightFac (M - Msc), b_M += margWeightFac (Mb - Mbsc) (from zero where it had
 * none) and counts as present from then on, also for the next ldso_ba_batch_optimize / _enqueue_gn.  flags[i] == NULL: window i takes no part - its prior and its
 * output slots stay untouched.  HM_out / bM_out ((8 F_i + 4)^2 row-major, 8 F_i + 4 doubles): NULL as arrays or per entry where the result is not wanted.
 * ldso_ba_batch_marginalize_frame: EnergyFunctional::marginalizeFrame (EnergyFunctional.cc:72-151; FullSystem.cc:574-583) - per window exactly what
 * ldso_ba_marginalize_frame(handle_i, frame_idx[i], HM_out[i], bM_out[i]) gives ((8 (F_i - 1) + 4)^2 row-major, 8 (F_i - 1) + 4 doubles); the handles keep their priors
 * and windows.  frame_idx[i] < 0: window i takes no part.
 * Both refuse (LDSO_E_INVALID) a NULL batch, NULL flags / frame_idx, a frame index >= F_i, a window with a pending ldso_ba_linearize_all result, a sharded handle
 * and windows of more than 8 key frames (the 8-slot table, as ldso_ba_batch_optimize). */
int ldso_ba_batch_marginalize_points(ldso_ba_batch_t *b, const int32_t *const *flags /*n*/, double *const *HM_out /*n or NULL*/, double *const *bM_out /*n or NULL*/);
int ldso_ba_batch_marginalize_frame(ldso_ba_batch_t *b, const int32_t *frame_idx /*n*/, double *const *HM_out /*n*/, double *const *bM_out /*n*/);
/* The next step of FullSystem::makeKeyFrame, activatePointsMT (FullSystem.cc:1052-1189; CoarseTracker.cc:686-818 the distance map), for every window of the batch, with
 * a number of launches that does not depend on n (one per kernel) and one upload, one download and one host synchronisation per call.  Per window each entry gives
 * exactly - byte for byte - what its single-window counterpart gives on that handle alone: the same device functions run on the same bytes.
 * ldso_ba_batch_activate_points = ldso_ba_activate_points(handle_i, n[i], points[i], ..., out[i]); n[i] == 0 or points[i] == NULL: window i takes no part.
 * ldso_ba_batch_select_candidates = ldso_ba_select_candidates(handle_i, <jobs[i]>, minTraceQuality, ...), ldso_ba_batch_select_activate_points =
 * ldso_ba_select_activate_points(handle_i, <jobs[i]>, ...): the arguments and outputs of the single-window entries, per window in a ldso_act_job_t (selected_out
 * may be NULL in the first, as there).  jobs[i].n_hosts == 0: window i takes no part.  A window may bring no candidates (n == 0: it builds its map only) or no seeds.
 * The windows may differ in image size; a distance map that does not fit into a workgroup's LDS is kept in global memory, window by window, in the same launch.
 * Afterwards ldso_ba_get_distance_map(handle_i) returns the map the call left for window i.  A window that takes no part keeps its outputs, its handle and its map.
 * All three refuse (LDSO_E_INVALID, nothing enqueued, no output written): a NULL batch or array, a participating window without its arrays, a candidate or seed whose
 * host is outside [0, n_hosts), a sharded handle, windows of more than 8 key frames (the 8-slot table, as ldso_ba_batch_optimize); the two that activate also
 * n_hosts != F_i and a missing key-frame image, as their single-window counterparts. */
typedef struct {            /* one window's share of a batched selection */
    int n_seeds; const ldso_act_seed_t *seeds;
    int n; const ldso_immature_t *points; const float *my_type;
    int n_hosts; const float *KRKi, *Kt; const int32_t *host_flagged;
    float currentMinActDist;
    int32_t *decision_out /*n*/, *selected_out /*n*/; int n_selected;          /* out */
    ldso_activation_t *out;                                                    /* out [n]: ldso_ba_batch_select_activate_points only */
} ldso_act_job_t;
int ldso_ba_batch_activate_points(ldso_ba_batch_t *b, const int *n /*n_win*/, const ldso_immature_t *const *points /*n_win*/, int min_obs, float min_idepth_hessian,
                                  int gn_iterations, ldso_activation_t *const *out /*n_win*/);
int ldso_ba_batch_select_candidates(ldso_ba_batch_t *b, ldso_act_job_t *jobs /*n_win*/, float minTraceQuality);
int ldso_ba_batch_select_activate_points(ldso_ba_batch_t *b, ldso_act_job_t *jobs /*n_win*/, float minTraceQuality, int min_obs, float min_idepth_hessian,
                                         int gn_iterations);
/* ldso_ba_batch_select_activate_tracers: activatePointsMT (FullSystem.cc:1052-1189) with every window's immature set where it lives - per window exactly what
 * ldso_ba_select_activate_tracer(handle_i, jobs[i].tracer, ...) gives on that handle alone: the candidates are the tracer's records and types, in their order, the
 * seeds every point of the resident window i whose host is not the newest frame, at its current inverse depth; decisions, selected list, activation records and the
 * distance map (ldso_ba_get_distance_map(handle_i)) byte for byte, and with compact != 0 the tracer's records, types and count afterwards (everything the loop did
 * not KEEP leaves its set, :1105-1188; the same stable compaction as ldso_trace_compact, :602-645).  Only KRKi / Kt / host_flagged go up.  Whatever n_win: one upload
 * (the tables of the kernels and the pose arrays), four launches (k_act_select_batch, k_activate_batch, k_compact_count_group, k_compact_move_group over the windows
 * that compact), one download (decisions, lists, records and the compactions' counts) and one wait on the batch's stream.  tracer == NULL: window i takes no part and
 * keeps its outputs, its handle and its map.  A tracer without records builds its window's map only.  decision_out / selected_out / out: n = the tracer's count before
 * the call; n_selected and n_left (the tracer's count afterwards) are written by the call.  A tracer may be a member of a ldso_trace_group_t; it must be idle, as for
 * ldso_ba_select_activate_tracer.  Refused (LDSO_E_INVALID, nothing enqueued, no output or tracer touched): everything ldso_ba_batch_select_activate_points refuses,
 * a tracer on another device than the batch, the same tracer in two jobs, a sharded handle, n_hosts != F_i, missing outputs where the tracer holds records. */
typedef struct {                      /* one window's share; tracer == NULL: the window takes no part */
    struct ldso_tracer *tracer;       /* a ldso_tracer_t (the immature-point tracer, below) */
    int n_hosts; const float *KRKi, *Kt; const int32_t *host_flagged;
    float currentMinActDist; int compact;
    int32_t *decision_out /*n*/, *selected_out /*n*/; int n_selected /*out*/;
    ldso_activation_t *out /*n*/; int n_left /*out*/;        /* n = the tracer's count before the call */
} ldso_act_tracer_job_t;
int ldso_ba_batch_select_activate_tracers(ldso_ba_batch_t *b, ldso_act_tracer_job_t *jobs /*n_win*/, float minTraceQuality, int min_obs, float min_idepth_hessian,
                                          int gn_iterations);
/* The step that closes the key-frame loop: every window of the batch becomes the next one, with a number of launches, copies and host synchronisations that does not
 * depend on n, and the batch stays usable (it re-cuts itself).
 * ldso_ba_batch_update_windows = ldso_ba_update_window(handle_i, <jobs[i]>) for every window with jobs[i].frame_from != NULL: the arguments of the single-window entry in a
 * ldso_win_job_t; per window the result is byte for byte what that entry leaves on the handle alone (window image, zero fills, prior reset, no applied linearisation).  One
 * upload through the batch's arena (every window's delta, chunk tables and one transfer table), three launches (k_win_rebuild_batch -> k_win_scatter_batch ->
 * k_point_stats_batch), one wait.  Validation comes first and is all-or-nothing: the checks of ldso_ba_update_window run for every participating window before anything is
 * written; LDSO_E_INVALID leaves every handle and the batch as they were.  Also refused: a NULL batch or job array, a handle with a pending linearisation or linearised
 * residuals, a sharded handle, a new F whose slot-table width differs from the batch's (in practice F > 8), a call in which no window takes part.
 * The batch then re-runs the chunk policy of ldso_ba_batch_create on the new point counts (it may change between balanced and regular chunks) and re-cuts every window.
 * The cost of sitting out: a window with jobs[i].frame_from == NULL keeps its window bytes and its applied state, but is re-cut like the others - one re-linearisation
 * launch, its own small chunk-table copies and wait, and its ping-pong parity flips, as in ldso_ba_batch_create.
 * A failure behind the validation (allocation, launch) leaves the participating handles without a window and the batch refusing every call but ldso_ba_batch_destroy.
 * ldso_ba_update_window on a member outside this call is still refused by the next batched call of a balanced batch.
 * ldso_ba_batch_set_frames = ldso_ba_set_frames(handle_i, frames, calib) followed by ldso_ba_set_prior(handle_i, HM, bM) for every window with jobs[i].frames != NULL
 * (HM / bM NULL = zero; the prior counts as present when either is given, as ldso_ba_set_prior has it): one upload, one distributing launch, one launch for the adjoints
 * and the precalc values of all windows, one wait; per window the device state is byte for byte that of the two single-window calls. */
typedef struct {            /* one window's share of ldso_ba_batch_update_windows: the arguments of ldso_ba_update_window */
    int F; const int32_t *image_slot, *frame_from;                             /* frame_from == NULL: the window takes no part */
    int P; const int32_t *point_from; const uint32_t *res_mask;
    int n_fresh; const ldso_point_t *fresh;
    int n_fresh_res; const ldso_residual_t *fresh_res; const float *fresh_mrb; const int32_t *fresh_ngr;
} ldso_win_job_t;
typedef struct {            /* one window's share of ldso_ba_batch_set_frames */
    const ldso_frame_t *frames; const ldso_calib_t *calib;                     /* frames == NULL: the window takes no part */
    const double *HM, *bM;                                                     /* (8F+4)^2 row-major, 8F+4; NULL = zero */
} ldso_frames_job_t;
int ldso_ba_batch_update_windows(ldso_ba_batch_t *b, const ldso_win_job_t *jobs /*n_win*/);
int ldso_ba_batch_set_frames(ldso_ba_batch_t *b, const ldso_frames_job_t *jobs /*n_win*/);
/* 1: the batch runs balanced cuts (one workgroup per CU and launch works through a run of chunks cut to measure), 0: regular chunks (ldso_ba_batch_chunk_points) */
int ldso_ba_batch_balanced(ldso_ba_batch_t *b, int *balanced);
/* the marginalisation prior as the handle holds it on the device ((8F+4)^2 row-major, 8F+4; either may be NULL), and whether it counts as present */
int ldso_ba_get_prior(ldso_ba_t *h, double *HM, double *bM, int *has_prior);
int ldso_ba_batch_destroy(ldso_ba_batch_t *b);
/* points per workgroup ldso_ba_batch_create gave the windows of the batch - since round 6 the AVERAGE, rounded: the cuts are uneven, ldso_ba_get_chunk_cuts has
 * them - (0: their single-window chunking was kept; ldso_ba_batch_destroy restores it) */
int ldso_ba_batch_chunk_points(ldso_ba_batch_t *b, int *points_per_workgroup);
/* bench / profiling: average duration [us] of the batched k_linearize over `reps` back-to-back launches (HIP events on the batch's stream) */
int ldso_ba_batch_time_linearize(ldso_ba_batch_t *b, int reps, double *avg_us);
/* The same sharded iteration with the collective inside, for a C / C++ host (north_star: host code stays C++): `iters` forced
 * Gauss-Newton iterations of this rank's shard - k_reduce into the handle's all-reduce buffer, ncclAllReduce (RCCL, fp64 sum, in
 * place, ~29 KB + 8 P bytes at F = 7) on the handle's stream, replicated solve, linearize of the shard - enqueued without a host
 * synchronisation.  `nccl_comm` is an ncclComm_t created by the caller (one rank per GPU, ncclCommInitRank); ncclAllReduce is
 * resolved at run time from the RCCL already in the process, else from librccl.so.  Every rank calls it with the same arguments. */
int ldso_ba_enqueue_gn_rccl(ldso_ba_t *h, void *nccl_comm, int first_iteration, int iters);
/* The same sharded iteration with a ONE-SHOT PEER-WRITE all-reduce instead of RCCL's ring (the message is 29 KB + 8 P bytes,
 * latency-bound): every rank owns a receive window (2 parities x n_ranks slots) that its peers address over xGMI; a rank writes its partial
 * into its slot of EVERY window as self-validating 64-bit words (payload | exchange number: no fence across the fabric) and sums the slots
 * of its own window in rank order (deterministic).  ldso_ba_p2p_window_alloc: this rank's window (uncached device memory) and, optionally,
 * its hipIpcMemHandle_t (64 bytes) for a peer PROCESS, which maps it with ldso_ba_p2p_window_open; ranks inside one process (or with peer
 * access enabled) pass the pointers themselves.  windows[q] = rank q's window as this process addresses it, windows[rank] = the own one.
 * Every rank calls ldso_ba_enqueue_gn_p2p with the same (first_iteration, iters).  ldso_ba_p2p_check (after ldso_ba_sync): LDSO_E_HIP when
 * a peer's words did not arrive within the kernel's 2 s poll limit.
 * The slots of a window are laid out by the CAPACITY of the handle (ldso_ba_create's max_frames / max_points), not by the current window: all ranks
 * create their handles with the same capacities, and a window change (ldso_ba_set_window) between two exchanges moves nothing.  Where uncached
 * device memory cannot be had ldso_ba_p2p_window_alloc fails with LDSO_E_UNSUPPORTED (cached memory would never show a polling kernel its peers' stores).
 * The exchange number lives in the HANDLE (1, 2, 3 ... over all ldso_ba_enqueue_gn_p2p calls of its lifetime) and must advance in lock-step
 * on all ranks: the handles and windows of the n_ranks ranks form ONE generation.  When any rank re-creates its handle, every rank re-creates
 * its handle and re-allocates its window (alloc zeroes it) - words of an older generation carrying the same number would otherwise be taken
 * for the new partial, numbers that never meet end in the 2 s timeout. */
size_t ldso_ba_p2p_window_bytes(ldso_ba_t *h, int n_ranks);
int ldso_ba_p2p_window_alloc(ldso_ba_t *h, int n_ranks, void **window_out, void *ipc_handle_out_64_bytes);
int ldso_ba_p2p_window_open(ldso_ba_t *h, const void *ipc_handle_64_bytes, void **window_out);
int ldso_ba_p2p_window_close(ldso_ba_t *h, void *window, int opened_from_handle);
int ldso_ba_enqueue_gn_p2p(ldso_ba_t *h, int rank, int n_ranks, void *const *windows, int first_iteration, int iters);
int ldso_ba_p2p_check(ldso_ba_t *h);
int ldso_ba_reduce_local(ldso_ba_t *h, void *reduce_buf_dev);
int ldso_ba_solve_reduced(ldso_ba_t *h, const void *reduce_buf_dev, int iteration, double lambda, int do_step);

/* --- results --------------------------------------------------------------------------------------- */
/* Per-residual outputs in the caller's flat residual order (any pointer may be NULL). */
int ldso_ba_get_residuals(ldso_ba_t *h, ldso_res_out_t *out, int32_t *state_state, int32_t *is_active, int32_t *to_remove);
int ldso_ba_get_points(ldso_ba_t *h, ldso_point_out_t *out);
int ldso_ba_get_frames(ldso_ba_t *h, ldso_frame_t *frames, double *step /*F*10*/, double *calib_value, double *calib_step,
                       double *pre_worldToCam /*F*12*/);
/* ldso_ba_get_residuals + ldso_ba_get_points + ldso_ba_get_frames behind ONE stream synchronisation (what FullSystem::optimize's tail reads back in one go:
 * FullSystem.cc:815-864).  res / state_state / is_active / to_remove / frames / step / calib_* may be NULL, points must not; the outputs equal the three getters'. */
int ldso_ba_get_results(ldso_ba_t *h, ldso_res_out_t *res, int32_t *state_state, int32_t *is_active, int32_t *to_remove, ldso_point_out_t *points,
                        ldso_frame_t *frames, double *step /*F*10*/, double *calib_value, double *calib_step);
/* Stitched systems of the last solve, (8F+4)^2 / (8F+4) doubles, reference ordering [calib | frames]. */
int ldso_ba_get_system(ldso_ba_t *h, double *HA, double *bA, double *HL, double *bL, double *Hsc, double *bsc,
                       double *HFinal, double *bFinal, double *x);
/* RawResidualJacobian of selected residuals (for fixLinearizationF callers): recomputed on demand at the
 * current state, or - with ldso_ba_set_debug_dump(h,1) - the copy written by the last linearize pass. */
int ldso_ba_set_debug_dump(ldso_ba_t *h, int enable);
/* Debug / test: run the reduce and the control step of a fast-path iteration as two launches (k_reduce, k_gn_solve) even where
 * the fused k_reduce_solve launch applies - the two schedules must agree (tests/test_ba_gpu.py::test_fused_launch_stress). */
int ldso_ba_set_debug_split_launch(ldso_ba_t *h, int enable);
int ldso_ba_get_jacobians(ldso_ba_t *h, const int32_t *res_ids, int n, ldso_rawjac_t *out);
/* Pair precalc [h*F+t][27] as FrameFramePrecalc: KRKi 9, Kt 3, R0 9, t0 3, aff 2, b0 1. */
int ldso_ba_get_precalc(ldso_ba_t *h, float *out);
/* Pair transforms of the CURRENT state [h*F+t][14]: PRE_RTll 9, PRE_tTll 3, PRE_aff_mode 2 (what point activation reads). */
int ldso_ba_get_pair_rt(ldso_ba_t *h, float *out);
int ldso_ba_get_counts(ldso_ba_t *h, int *resInA, int *resInL);
/* energies of the linearizeAll calls inside the last ldso_ba_optimize (<= cap values), returns count */
int ldso_ba_get_energy_log(ldso_ba_t *h, double *out, int cap);
/* The hand-over inside the fused reduce + control-step launch of a forced iteration (k_reduce_solve): its reduce workgroups arrive on a fixed number of words,
 * workgroup q (dispatch index behind the control workgroups) on word ldso_ba_arrival_shard(q), and the control workgroup waits on every word for its share of
 * the launch's `total` arrivers.  Host logic without a device, by the functions the kernel compiles (tests/test_reduce_arrival_cpu.py):
 * ldso_ba_arrival_targets fills that share for every word and returns the number of words (at most 64). */
int ldso_ba_arrival_targets(int total, int *targets);
int ldso_ba_arrival_shard(int q);
/* Debug / test: the arrival words of the handle behind a stream synchronisation - all zero between launches (the control workgroup re-arms them).  Returns the
 * number of words, or LDSO_E_NONFINITE (words filled all the same) when the iteration's non-finite status is set, which is also where a wait of the control
 * workgroup that ran out of polls ends; ldso_ba_enqueue_gn has no status of its own. */
int ldso_ba_get_arrival_words(ldso_ba_t *h, int *words);
/* -DLDSO_STAMPS builds of k_reduce_solve (scripts/reduce_chain_stamps.py): the records of the last fused launch, three wall-clock values per reduce workgroup in
 * dispatch order - started | data atomics acknowledged | arrival atomic returned.  Copies the first `cap` doubles of the buffer that holds them (the pair
 * contributions of the step-wise path, which a product build leaves there), returns how many. */
int ldso_ba_get_reduce_stamps(ldso_ba_t *h, double *out, int cap);
/* bench.py roofline: average duration (us) of `reps` back-to-back launches of the dominant kernel (k_linearize, applied state
 * -> scratch set, nothing applied) between one pair of HIP events on the handle's stream. */
int ldso_ba_time_linearize(ldso_ba_t *h, int reps, double *avg_us);
/* average device time (ms) per launch of kernel `which` since the last reset (HIP events on the
 * handle's stream); which: 0 = linearize, 1 = reduce+gather, 2 = solve, 3 = point step, 4 = an empty event pair
 * recorded right after every linearize launch (the event overhead to subtract). */
int ldso_ba_kernel_time_ms(ldso_ba_t *h, int which, double *avg_ms, int *launches);
int ldso_ba_profile(ldso_ba_t *h, int enable);

/* ------------------------------------------------------------------------------------------------
 * CoarseTracker (src/frontend/CoarseTracker.cc).
 * ---------------------------------------------------------------------------------------------- */
typedef struct ldso_tracker ldso_tracker_t;

int ldso_tr_create(int device, int w, int h, int levels, ldso_tracker_t **out);
int ldso_tr_destroy(ldso_tracker_t *t);
int ldso_tr_set_stream(ldso_tracker_t *t, void *hip_stream);
int ldso_tr_set_settings(ldso_tracker_t *t, const ldso_settings_t *s);
/* CoarseTracker::makeK (CoarseTracker.cc:219-246). */
int ldso_tr_make_k(ldso_tracker_t *t, const ldso_calib_t *calib);
/* CoarseTracker::setCoarseTrackingRef (CoarseTracker.cc:248-256) + makeCoarseDepthL0 (:258-438).
 * ref_dIp: `levels` host pointers to the reference keyframe pyramid; pts = n x (Ku,Kv,new_idepth,HdiF)
 * of the active points whose lastResiduals[0] is IN, in the reference's iteration order. */
int ldso_tr_set_ref(ldso_tracker_t *t, const float *const *ref_dIp, float ref_aff_a, float ref_aff_b, float ref_exposure,
                    const float *pts, int n);
/* the frame to be tracked (FrameHessian::dIp[0..levels-1]) */
int ldso_tr_set_new_frame(ldso_tracker_t *t, const float *const *new_dIp, float exposure);
/* The new frame from its RAW level-0 irradiance (w*h floats): the whole FrameHessian::makeImages pyramid (2x2 mean pooling +
 * gradients per level, FrameHessian.cc:44-113) is built on the device.  ldso_tr_get_new_frame_level: test fetch of one level. */
int ldso_tr_set_new_frame_image(ldso_tracker_t *t, const float *irradiance, float exposure);
int ldso_tr_get_new_frame_level(ldso_tracker_t *t, int lvl, float *out);
/* Both frames as resident ldso_pyramid_t (zero-copy): the frame that was tracked becomes the next reference without any copy. */
int ldso_tr_set_new_frame_pyramid(ldso_tracker_t *t, ldso_pyramid_t *pyr, float exposure);
int ldso_tr_set_ref_pyramid(ldso_tracker_t *t, ldso_pyramid_t *pyr, float ref_aff_a, float ref_aff_b, float ref_exposure,
                            const float *pts, int n);
/* CoarseTracker::calcRes (CoarseTracker.cc:440-572). rs_out = Vec6; returns buf_warped_n via n_warped. */
int ldso_tr_calc_res(ldso_tracker_t *t, int lvl, const double T_ref2new[12], float aff_a, float aff_b, float cutoffTH,
                     double rs_out[6], int *n_warped);
/* CoarseTracker::calcGSSSE (CoarseTracker.cc:574-632) for the buffers of the last calcRes. */
int ldso_tr_calc_gs(ldso_tracker_t *t, int lvl, const double T_ref2new[12], float aff_a, float aff_b, double H_out[64], double b_out[8]);
/* CoarseTracker::trackNewestCoarse (CoarseTracker.cc:61-217): whole LM pyramid loop on the device. */
int ldso_tr_track(ldso_tracker_t *t, double T_ref2new_inout[12], float aff_inout[2], int coarsestLvl, const double minResForAbort[5],
                  double lastResiduals_out[5], double lastFlowIndicators_out[3], int *ok_out, int *iterations_out);
/* evaluate nhyp motion hypotheses of FullSystem::trackNewCoarse (FullSystem.cc:213-357)
 * concurrently, one workgroup each (nhyp <= 128).  Arrays are nhyp-major. */
int ldso_tr_track_batch(ldso_tracker_t *t, int nhyp, double *T_ref2new_inout, float *aff_inout, int coarsestLvl, const double minResForAbort[5],
                        double *lastResiduals_out, double *lastFlowIndicators_out, int *ok_out, int *iterations_out);
/* The hypothesis loop of FullSystem::trackNewCoarse (FullSystem.cc:319-356) replayed on the results of one
 * ldso_tr_track_batch call that ran every try with minRes = NaN: reproduces the sequential accept / abort / early-exit decisions
 * (a try counts as aborted at the level where its residual exceeds 1.5 x the `achievedRes` of the tries before it).  Host only.
 * best_out = index of the winning try or -1; tries_consumed_out = how many tries the sequential loop would have run. */
/* calcRes evaluations per pyramid level of the last track (hypothesis 0 of a batch) and the reference point counts pc_n[lvl] */
int ldso_tr_last_track_evals(ldso_tracker_t *t, int evals[5], int pc_n[5]);
/* LM solves of the last track call (all hypotheses) whose 8 x 8 system was rank-deficient to float precision (a pivot below 1e-6 of the diagonal entry it started from: fewer than
 * eight reference points on a level) and were solved by the reference's diagonally pivoted LDL^T (Eigen's `Hl.ldlt().solve(-b)`, CoarseTracker.cc:120-128) instead of the unpivoted register
 * factorisation; 0 on any normal track. */
int ldso_tr_last_track_pivoted_solves(ldso_tracker_t *t, int *n);
/* Debug / test entry: the 8 x 8 LM solve of the tracking kernel on its own - H with diag_scale (= 1 + lambda) on the diagonal, x = -b (`Hl.ldlt().solve(-b)`,
 * CoarseTracker.cc:120-128); *pivoted = 1 when the system went through the pivoted factorisation.  Runs on the current device, synchronous. */
int ldso_tr_debug_solve8(const double H[64], const double b[8], double diag_scale, double x[8], int *pivoted);
int ldso_tr_select_hypothesis(int nhyp, int coarsestLvl, const double *lastResiduals /*nhyp*5*/, const int *ok /*nhyp*/, double lastCoarseRMSE0,
                              double reTrackThreshold, int *best_out, int *tries_consumed_out, double achievedRes_out[5]);
/* The motion-hypothesis list of FullSystem::trackNewCoarse (FullSystem.cc:189-309): worldToCam poses [R|t] (Frame::getPose()) of
 * allFrameHistory[size-3] (sprelast), allFrameHistory[size-2] (slast) and coarseTracker->lastRef (lastF) -> up to 83 lastF_2_fh tries
 * (out: 83 x 12 doubles).  poses_valid = 0 (one of the three poses invalid, :306-309): the identity alone.  Pure host function. */
int ldso_tr_motion_hypotheses(const double sprelast_w2c[12], const double slast_w2c[12], const double lastF_w2c[12], int poses_valid,
                              double *lastF_2_fh_tries_out, int *n_out);
/* Vec4 FullSystem::trackNewCoarse(fh) (FullSystem.cc:179-386) on a tracker whose reference and new frame are set: hypothesis list, the try
 * loop with its achievedRes abort thresholds and reTrackThreshold early exit (try 0 alone; the remaining tries, if the loop goes on, as one
 * batched launch + ldso_tr_select_hypothesis), the pose / affine hand-over.  lastCoarseRMSE: FullSystem::lastCoarseRMSE in / out;
 * result4 = (achievedRes[0], flowVecs); new_frame_w2c / aff_out = what :376-378 write into fh->frame; *good = 0: "tracking failed entirely". */
int ldso_tr_track_new_coarse(ldso_tracker_t *t, const double sprelast_w2c[12], const double slast_w2c[12], const double lastF_w2c[12], int poses_valid,
                             const float aff_last[2], double lastCoarseRMSE_inout[5], double reTrackThreshold, double result4[4],
                             double new_frame_w2c[12], float aff_out[2], int *tries_consumed, int *good);
int ldso_tr_get_pc(ldso_tracker_t *t, int lvl, float *u, float *v, float *idepth, float *color, int *n);

/* ------------------------------------------------------------------------------------------------
 * A group of trackers: the per-frame leg of many sequences on one card.  CoarseTracker::trackNewestCoarse (CoarseTracker.cc:61-217) runs on
 * every frame of every sequence; one track alone is latency bound and occupies 16 of the CUs, so the tracks of a group share launches.
 * All arrays are member-major (member i of ldso_tr_group_create at row i).
 * ---------------------------------------------------------------------------------------------- */
/* The launch shape of a track: *G = how many workgroups share each of `count` concurrent tracks on a device with num_cu CUs
 * (16 / 12 / 8 / 4 while count * G <= num_cu: all workgroups of a cooperative launch must be resident; else 1).  Pure host function. */
int ldso_tr_coop_width(int count, int num_cu, int *G);
typedef struct ldso_tr_group ldso_tr_group_t;
/* 1 <= n <= 128 trackers on one device and one stream (ldso_tr_set_stream); image size, level count, settings and point counts may differ.  A tracker
 * belongs to at most one group and stays usable on its own between group calls (ldso_tr_set_ref*, ldso_tr_set_new_frame*, ldso_tr_track): the group
 * reads every member's current frames and settings at each call.  ldso_tr_destroy of a member is refused while the group lives. */
int ldso_tr_group_create(ldso_tracker_t *const *trackers, int n, ldso_tr_group_t **out);
int ldso_tr_group_destroy(ldso_tr_group_t *g);
/* what a launch of n_jobs tracks uses on the group's device (ldso_tr_coop_width with its CU count) */
int ldso_tr_group_coop_width(ldso_tr_group_t *g, int n_jobs, int *G);
/* CoarseTracker::trackNewestCoarse (CoarseTracker.cc:61-217) = ldso_tr_track for every member with active[i] != 0 (active == NULL: all), in ONE launch with
 * one upload, one download and one wait.  Rows of inactive members are left untouched.  minResForAbort: n x 5 or NULL (never abort). */
int ldso_tr_group_track(ldso_tr_group_t *g, const uint8_t *active /* n or NULL = all */, double *T_ref2new_inout /* n*12 */, float *aff_inout /* n*2 */,
                        const int *coarsestLvl /* n */, const double *minResForAbort /* n*5 or NULL */, double *lastResiduals_out /* n*5 */,
                        double *lastFlowIndicators_out /* n*3 */, int *ok_out /* n */, int *iterations_out /* n */);
/* Vec4 FullSystem::trackNewCoarse(fh) (FullSystem.cc:179-386) = ldso_tr_track_new_coarse for every active member, in two launches for the whole group:
 * try 0 of every member, then the remaining tries of all members whose loop goes on (:355 not met) in one. */
int ldso_tr_group_track_new_coarse(ldso_tr_group_t *g, const uint8_t *active, const double *sprelast_w2c /* n*12 */, const double *slast_w2c, const double *lastF_w2c,
                                   const int *poses_valid /* n */, const float *aff_last /* n*2 */, double *lastCoarseRMSE_inout /* n*5 */, const double *reTrackThreshold /* n */,
                                   double *result4 /* n*4 */, double *new_frame_w2c /* n*12 */, float *aff_out /* n*2 */, int *tries_consumed /* n */, int *good /* n */);

/* ------------------------------------------------------------------------------------------------------------
 * Immature-point tracing: FullSystem::traceNewCoarse (FullSystem.cc:1012-1050) = ImmaturePoint::traceOn
 * (src/internal/ImmaturePoint.cc:47-310) for every immature point of the window against a new frame, one launch.
 * The points stay resident on the device between frames (set once per key frame, traced on every frame).
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct ldso_tracer ldso_tracer_t;
int ldso_trace_settings_default(ldso_trace_settings_t *s);
int ldso_trace_create(int device, int w, int h, int max_points, ldso_tracer_t **out);
int ldso_trace_destroy(ldso_tracer_t *t);
int ldso_trace_set_settings(ldso_tracer_t *t, const ldso_trace_settings_t *s);
int ldso_trace_set_points(ldso_tracer_t *t, int n, const ldso_immature_t *points);
int ldso_trace_get_points(ldso_tracer_t *t, ldso_immature_t *points_out);
/* n records that already lie in device memory (ldso_feat_device) are copied device-to-device behind the tracer's current points: the fresh points of
 * FullSystem::makeNewTraces (FullSystem.cc:1272-1325) never cross to the host and back.  LDSO_E_INVALID when they would exceed max_points. */
int ldso_trace_append_points_device(ldso_tracer_t *t, int n, const void *immature_dev);
/* ImmaturePoint::my_type (ImmaturePoint.h:114; the factor on currentMinActDist, FullSystem.cc:1141) travels with the record, in an array of the tracer's own beside
 * the records: ldso_trace_set_points resets it to 1 for its n records, ldso_trace_append_points_device sets 1 for the appended ones (FullSystem.cc:1281 constructs
 * the points of setting_pointSelection == 1 with my_type = 1).  my_type / out: one float per current record. */
int ldso_trace_set_point_types(ldso_tracer_t *t, const float *my_type);
/* my_type of the LAST n records from n floats in device memory (ldso_pixsel_device): behind ldso_trace_append_points_device for the points of
 * setting_pointSelection == 0, whose my_type is their map value (FullSystem.cc:1297).  LDSO_E_INVALID when n exceeds the tracer's count. */
int ldso_trace_set_tail_types_device(ldso_tracer_t *t, int n, const void *type_dev);
int ldso_trace_get_point_types(ldso_tracer_t *t, float *out);
/* What leaves the immature set leaves it on the device: a STABLE compaction of the records and their types.  Record i stays iff keep[i] != 0 (keep: n bytes of
 * host memory, NULL: all kept) and host_map[record.host] >= 0 (host_map: n_hosts entries, NULL: the identity); a record whose host is outside [0, n_hosts) is
 * dropped, not dereferenced.  A surviving record gets host = host_map[host]: one call covers points released by host code (FullSystem.cc:1105-1188), the points
 * of a marginalised frame (FullSystem.cc:602-645) and the shift of the host indices behind it.  The survivors keep their relative order - the reference's
 * iteration order (FullSystem.cc:1088-1098), on which the greedy selection depends.  The records move out of place into a second buffer of the tracer's and
 * the two swap.  One synchronisation, behind which *n_out (optional) = the new count. */
int ldso_trace_compact(ldso_tracer_t *t, const uint8_t *keep_or_null, int n_hosts, const int32_t *host_map_or_null, int *n_out);
/* ldso_ba_select_activate_points (FullSystem.cc:1080-1164) with the immature set where it lives: the candidates are the tracer's records and types, in their
 * order, the seeds every point of the handle's resident window whose host is not the newest frame, at its CURRENT inverse depth (PointHessian::idepth_scaled,
 * CoarseTracker.cc:706-709).  Only KRKi / Kt / host_flagged go up.  A record hosted by frame n_hosts - 1 is no candidate (the loop skips the newest frame,
 * :1089): its decision is LDSO_ACT_KEEP and it is not touched.  A candidate or window point whose host is no frame of the window is dropped / skipped by the
 * kernel.  compact != 0: every record whose decision is not LDSO_ACT_KEEP leaves the tracer's set in the same enqueue - the deleted candidates and every
 * SELECTED one, whether optimizeImmaturePoint accepts it or not (:1170-1187).  decision_out / selected_out / out: n = the tracer's count before the call, as
 * ldso_ba_select_activate_points; *n_left_out (optional) = its count afterwards.  ldso_ba_get_distance_map works as after the explicit call.
 * Preconditions beyond ldso_ba_select_activate_points': an unsharded window, n_hosts = its frame count, tracer and handle on one device, the tracer idle (all of
 * its entry points synchronise before they return).  A violation gives LDSO_E_INVALID before anything is launched.  Runs on the handle's stream, one wait. */
int ldso_ba_select_activate_tracer(ldso_ba_t *h, ldso_tracer_t *t, int n_hosts, const float *KRKi, const float *Kt, const int32_t *host_flagged,
                                   float currentMinActDist, float minTraceQuality, int min_obs, float min_idepth_hessian, int gn_iterations, int compact,
                                   int32_t *decision_out /*n*/, int32_t *selected_out /*n*/, int *n_selected_out, ldso_activation_t *out /*n*/, int *n_left_out);
/* the new frame: level-0 image as FrameHessian::dIp[0] (w*h*3 floats), or the raw irradiance (makeImages on the device) */
int ldso_trace_set_frame(ldso_tracer_t *t, const float *dI_level0);
int ldso_trace_set_frame_raw(ldso_tracer_t *t, const float *irradiance);
int ldso_trace_set_frame_pyramid(ldso_tracer_t *t, ldso_pyramid_t *pyr);
/* per host key frame h < n_hosts (FullSystem.cc:1025-1032): KRKi[h] = K R K^-1 (row-major 3x3), Kt[h] = K t,
 * aff[h] = AffLight::fromToVecExposure(host, new).  counts_out[6] (optional): points per resulting LDSO_IPS_* status. */
int ldso_trace_on(ldso_tracer_t *t, int n_hosts, const float *KRKi, const float *Kt, const float *aff, int *counts_out);
/* The caller's stream instead of the tracer's own (NULL: an own one again).  The tracer holds no frame afterwards (the wait ldso_trace_set_frame_pyramid
 * queued for the frame's build stands on the old stream): set the frame again before the next trace. */
int ldso_trace_set_stream(ldso_tracer_t *t, void *hip_stream);

/* ------------------------------------------------------------------------------------------------------------
 * A group of tracers: FullSystem::traceNewCoarse (FullSystem.cc:1012-1050) = ImmaturePoint::traceOn (src/internal/ImmaturePoint.cc:47-310) of the
 * new frames of many sequences on one card.  One ldso_trace_on is a pose upload, a memset, a launch, a download and a wait; a group call traces the points of
 * all active members in ONE launch (one wavefront per point, the members' points packed wavefront by wavefront) with one upload, one download and one wait.
 * A member's records and counts are those of its own ldso_trace_on from the same input, byte for byte.  All arrays are member-major.
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct ldso_trace_group ldso_trace_group_t;
/* The member-lookup rule of a grouped launch: first[j] = the wavefronts in front of job j (first[0] = 0, non-decreasing), first[n_jobs] = all of them;
 * *job_out = the job j with first[j] <= wave < first[j + 1] - jobs without wavefronts are skipped.  LDSO_E_INVALID for a wave outside
 * [0, first[n_jobs]).  Pure host function; the kernel runs the same search. */
int ldso_trace_group_member_of(const int *first, int n_jobs, int wave, int *job_out);
/* 1 <= n <= 128 tracers on one device and one stream (ldso_trace_set_stream); image size, max_points, settings and point counts may differ.  A tracer belongs to
 * at most one group and stays usable on its own between group calls (ldso_trace_set_points, ldso_trace_set_frame*, ldso_trace_on, ldso_trace_compact, ...): the
 * group reads every member's current records, frame and settings at each call, and every call checks that the members still share their stream.
 * ldso_trace_destroy of a member is refused while the group lives. */
int ldso_trace_group_create(ldso_tracer_t *const *tracers, int n, ldso_trace_group_t **out);
int ldso_trace_group_destroy(ldso_trace_group_t *g);
/* ldso_trace_on for every member with active[i] != 0 (NULL: all).  Member i brings n_hosts[i] hosts: KRKi[i], Kt[i], aff[i] point to n_hosts[i] x 9, 3 and 2
 * floats (entries of inactive members are not read).  counts_out: n x 6 or NULL; rows of inactive members are left untouched.  Everything is checked before
 * anything is enqueued: a member without a frame or an n_hosts outside 1..LDSO_MAX_FRAMES gives LDSO_E_INVALID with the member's index in the message, and no
 * record of any member changes. */
int ldso_trace_group_on(ldso_trace_group_t *g, const uint8_t *active /* n or NULL = all */, const int *n_hosts /* n */, const float *const *KRKi /* n pointers */,
                        const float *const *Kt /* n pointers */, const float *const *aff /* n pointers */, int *counts_out /* n*6 or NULL */);
/* ldso_trace_group_compact = ldso_trace_compact(member_i, keep[i], n_hosts[i], host_map[i], &n_out[i]) for every member with active[i] != 0 (NULL: all): what leaves the immature sets of many
 * sequences when each marginalises a frame (FullSystem.cc:602-645: its records go, the host indices behind it shift) or host code released points
 * (FullSystem.cc:1052-1189).  keep: n pointers to the members' keep bytes (an entry or the array NULL: all kept); host_map: n pointers to n_hosts[i] entries (an entry
 * or the array NULL: the identity).  A member's records, types and count afterwards are those of its own ldso_trace_compact, byte for byte.  One upload (job table,
 * prefix table, host maps, keep bytes), two launches, one download of the counts and one wait on the group's stream, whatever n.  n_out: n or NULL; rows of inactive
 * members are left alone, an active member without records reports 0.  Everything is checked before anything is enqueued: an n_hosts outside 1..LDSO_MAX_FRAMES or
 * a map entry >= LDSO_MAX_FRAMES (the member's index in the message), or members that no longer share the stream, give LDSO_E_INVALID and no member's records,
 * types or count change. */
int ldso_trace_group_compact(ldso_trace_group_t *g, const uint8_t *active /* n or NULL = all */, const uint8_t *const *keep /* n pointers or NULL */,
                             const int *n_hosts /* n */, const int32_t *const *host_map /* n pointers or NULL */, int *n_out /* n or NULL */);

/* ------------------------------------------------------------------------------------------------------------
 * New features of a key frame: FullSystem::makeNewTraces (FullSystem.cc:1272-1325) for setting_pointSelection == 1 (the default, Setting.cc:125) =
 * FeatureDetector::DetectCorners (src/frontend/FeatureDetector.cc:34-130; ShiTomasiScore and IC_Angle: include/frontend/FeatureDetector.h:49-114;
 * ComputeDescriptor: FeatureDetector.cc:132-189) and one ImmaturePoint constructor per feature (src/internal/ImmaturePoint.cc:14-38), on level 0 of a
 * resident pyramid.  Features come in the reference's order (cells gx-major, gy inner, by rank inside a cell); where the reference leaves the order of
 * equal scores to std::sort, the lower idx = y * gridsize + x comes first.  Two calls on the same input give byte-identical buffers.
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct ldso_features ldso_features_t;
/* Host only, no device: the grid of FeatureDetector.cc:37-42 for n wanted features (0 < n <= w * h).  per_cell = picks per cell (:88-91),
 * capacity = cells visited (:44-45) * per_cell = the most features a call can return.  Every output pointer is optional. */
int ldso_feat_grid(int w, int h, int n, int *gridsize, int *gridX, int *gridY, int *skip, int *per_cell, int *capacity);
/* orb_pattern: the 1024 ints of ldso::bit_pattern_31_ (FeatureDetector.cc:213-471), copied; NULL: descriptors stay zero, angles are still computed */
int ldso_feat_create(int device, int w, int h, int max_features, const int32_t *orb_pattern_1024_or_null, ldso_features_t **out);
int ldso_feat_destroy(ldso_features_t *f);
int ldso_feat_set_stream(ldso_features_t *f, void *hip_stream);
/* CalibHessian::B (CalibHessian.h:138) for the gamma weight of absSquaredGrad (FrameHessian.cc:93-97, getBGradOnly: CalibHessian.h:102-111);
 * NULL: no weighting (HCalib == 0 there), which equals the identity table */
int ldso_feat_set_response(ldso_features_t *f, const float *B_256_or_null);
/* DetectCorners(n_features, frame) + the ImmaturePoint constructors with host = host_index: one call, one synchronisation at its end.
 * *n_corners_out = DetectCorners' return value.  LDSO_E_INVALID when the grid's capacity exceeds max_features, LDSO_E_UNSUPPORTED for a gridsize above 64,
 * LDSO_E_NONFINITE when a pixel read by the selection, a score, an angle or a record's colour is not finite (the results are still there to be fetched; a
 * NaN score never wins a comparison, a record with a non-finite colour has energyTH = NaN as ImmaturePoint.cc:28-31 leaves it: FullSystem.cc:1298 drops it). */
int ldso_feat_detect(ldso_features_t *f, ldso_pyramid_t *pyr, int n_features, int host_index, int *n_features_out, int *n_corners_out);
/* the results of the last ldso_feat_detect on the host (immature_out optional) / as device pointers (valid until the next detect or destroy) */
int ldso_feat_get(ldso_features_t *f, ldso_feature_t *out, ldso_immature_t *immature_out_or_null);
int ldso_feat_device(ldso_features_t *f, const void **features_dev, const void **immature_dev, int *n);
/* enable != 0: ldso_feat_detect brackets its kernels with HIP events; us_out[4] (optional) = microseconds of the last profiled call:
 * cells + compaction (FeatureDetector.cc:44-95), corners (:98-118), angle + descriptor (:120-128), records (ImmaturePoint.cc:14-38) */
int ldso_feat_profile(ldso_features_t *f, int enable, float us_out[4]);

/* ------------------------------------------------------------------------------------------------------------
 * A group of detectors: FullSystem::makeNewTraces (FullSystem.cc:1272-1325) for setting_pointSelection == 1 = FeatureDetector::DetectCorners
 * (src/frontend/FeatureDetector.cc:34-130) and the ImmaturePoint constructors (src/internal/ImmaturePoint.cc:14-38) of the key frames that many sequences on one
 * card make in the same step.  One ldso_feat_detect is a memset, five launches (most of its time on a handful of workgroups), a download and a wait, and
 * ldso_trace_append_points_device waits once more; a group call runs the same kernel bodies for all active members in five launches, six with the append, with one
 * upload, one download and one wait, whatever n.  A member's features, records, counts and appended records are those of its own solo calls from the same input,
 * byte for byte.  All arrays are member-major.
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct ldso_feat_group ldso_feat_group_t;
/* 1 <= n <= 128 detectors on one device and one stream (ldso_feat_set_stream); image size, max_features, response table and pattern may differ.  A detector
 * belongs to at most one group and stays usable on its own between group calls (ldso_feat_set_response, ldso_feat_detect, ldso_feat_get, ldso_feat_device, ...): the
 * group reads every member's current state at each call and writes every result but the control words into the member's own buffers, and every call checks that
 * the members still share their stream.  ldso_feat_destroy of a member is refused while the group lives. */
int ldso_feat_group_create(ldso_features_t *const *members, int n, ldso_feat_group_t **out);
int ldso_feat_group_destroy(ldso_feat_group_t *g);
/* ldso_feat_detect(member_i, pyr[i], n_features[i], host_index[i], ...) for every member with active[i] != 0 (NULL: all; entries of inactive members are not
 * read).  tracers: NULL, or n pointers of which an entry may be NULL; member i's fresh records are appended to tracers[i] with my_type = 1 in the same enqueue, as
 * ldso_trace_append_points_device(tracers[i], n_i, member i's records) would, and the tracer's count grows behind the call's wait.  Everything is checked before
 * anything is enqueued, every refusal names the member's index, and nothing of any member or tracer changes: LDSO_E_INVALID for an n_features out of range, a
 * grid's capacity above max_features, a pyramid that does not fit the member or holds no image, a tracer that is not on the group's device and stream, the same
 * tracer for two members, or a tracer with max_points - n below the GRID'S CAPACITY (ldso_feat_grid) - the count is not known before the wait, so this is stricter
 * than the solo append, which needs room for the features found only; LDSO_E_UNSUPPORTED for a gridsize above 64.
 * n_features_out, n_corners_out, status_out: n each or NULL; rows of inactive members are left untouched.  A non-finite pixel, score, angle or colour in member i
 * sets status_out[i] = LDSO_E_NONFINITE (LDSO_OK otherwise); the call then returns LDSO_E_NONFINITE and the message names the first such member.  As in the solo
 * call every member's results are there to be fetched, and the appends have happened: such records carry energyTH = NaN, and FullSystem.cc:1298 drops them. */
int ldso_feat_group_detect(ldso_feat_group_t *g, const uint8_t *active /* n or NULL = all */, ldso_pyramid_t *const *pyr /* n */, const int *n_features /* n */,
                           const int *host_index /* n */, ldso_tracer_t *const *tracers /* n pointers or NULL */, int *n_features_out, int *n_corners_out,
                           int *status_out /* each n or NULL */);
/* ldso_feat_get of every active member: features_out[i] / immature_out[i] take the member's last count of records (an entry or an array NULL: not fetched);
 * exactly-sized copies, one wait.  A member's own ldso_feat_get and ldso_feat_device give the same after a group call. */
int ldso_feat_group_get(ldso_feat_group_t *g, const uint8_t *active /* n or NULL = all */, ldso_feature_t *const *features_out /* n pointers or NULL */,
                        ldso_immature_t *const *immature_out /* n pointers or NULL */);
/* enable != 0: ldso_feat_group_detect brackets its launches with HIP events; us_out[5] (optional) = microseconds of the last profiled call:
 * cells + compaction, corners, angle + descriptor, records, append */
int ldso_feat_group_profile(ldso_feat_group_t *g, int enable, float us_out[5]);

/* ------------------------------------------------------------------------------------------------------------
 * DSO's gradient pixels of a key frame: FullSystem::makeNewTraces for setting_pointSelection == 0 (FullSystem.cc:1284-1304) = PixelSelector::makeMaps
 * (src/frontend/PixelSelector2.cc:111-168; makeHists :36-109, computeHistQuantil :27-34, select :170-315), the raster scan of the map and one ImmaturePoint
 * constructor per hit (src/internal/ImmaturePoint.cc:14-38), on levels 0-2 of a resident pyramid.  Maps, counts, potentials and thresholds are exactly the
 * reference's; two calls on the same input give byte-identical buffers.  Three reads the reference leaves undefined are defined here:
 *   - the last row of absSquaredGrad[2] (never written: FrameHessian.cc:81 stops a row early, :49 clears bytes; read for y = h - 4) is 0;
 *   - thsSmoothed[(x >> 5) + (y >> 5) * (w / 32)] runs past the table when w or h is no multiple of 32: such sizes give LDSO_E_UNSUPPORTED;
 *   - a non-finite pixel (int(sqrtf(.)) is undefined there) gives LDSO_E_NONFINITE; a NaN never wins a comparison, as in ldso_feat_detect.
 * Bins 50..90 of the gradient histogram, which computeHistQuantil can reach only for a cut near 1, are empty.
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct ldso_pixsel ldso_pixsel_t;
/* Host only, no device: LDSO_OK when the selector takes a w x h image (both multiples of 32), else LDSO_E_UNSUPPORTED */
int ldso_pixsel_supported(int w, int h);
/* Host only, no device: the scalar arithmetic of makeMaps :125-153 behind one select pass with counts (n2, n3, n4) at `potential`.  *action = 1: select
 * again at *new_potential (:133-147); 0: done, *new_potential = the idealPotential :165 stores, *char_th = charTH of :153 or -1 when nothing is thinned. */
int ldso_pixsel_plan(const int counts[3], float density, int potential, int recursions_left, int *action, int *new_potential, int *char_th);
/* random_pattern: the w * h bytes of PixelSelector::randomPattern (:10-13: rand() & 0xFF after srand(3141592)), copied; currentPotential starts at 3 (:14) */
int ldso_pixsel_create(int device, int w, int h, const unsigned char *random_pattern, ldso_pixsel_t **out);
int ldso_pixsel_destroy(ldso_pixsel_t *p);
int ldso_pixsel_set_stream(ldso_pixsel_t *p, void *hip_stream);
/* CalibHessian::B for the gamma weight of absSquaredGrad, as ldso_feat_set_response */
int ldso_pixsel_set_response(ldso_pixsel_t *p, const float *B_256_or_null);
/* setting_minGradHistCut, setting_minGradHistAdd, setting_gradDownweightPerLevel, setting_selectDirectionDistribution (Setting.cc:83-87: 0.5, 7, 0.75, true) */
int ldso_pixsel_set_settings(ldso_pixsel_t *p, float minGradHistCut, float minGradHistAdd, float gradDownweightPerLevel, int selectDirectionDistribution);
/* PixelSelector::currentPotential, which one makeMaps leaves for the next (:165) */
int ldso_pixsel_set_potential(ldso_pixsel_t *p, int potential);
int ldso_pixsel_get_potential(ldso_pixsel_t *p, int *potential);
/* makeMaps(fh, map, density, recursions_left, plot, th_factor) (:111-168): one histogram pass, one select pass per recursion (one wait each for the counts),
 * the thinning.  *n_out = its return value, counts_out = (n2, n3, n4) of the last select pass, *potential_used = that pass's potential; outputs optional. */
int ldso_pixsel_make_maps(ldso_pixsel_t *p, ldso_pyramid_t *pyr, float density, int recursions_left, float th_factor, int *n_out, int counts_out[3], int *potential_used);
/* the map of the last ldso_pixsel_make_maps: w * h floats 0 / 1 / 2 / 4;  ths / thsSmoothed (:64, :107): (w / 32) * (h / 32) floats each, either optional */
int ldso_pixsel_get_map(ldso_pixsel_t *p, float *map_out);
int ldso_pixsel_get_thresholds(ldso_pixsel_t *p, float *ths_out, float *ths_smoothed_out);
/* FullSystem.cc:1290-1303 on that map: one record per selected pixel with patternPadding + 1 <= x < w - patternPadding - 2 (likewise y), in raster order,
 * host = host_index, my_type = the map value.  A record with a non-finite colour is kept, has energyTH = NaN and makes the call return LDSO_E_NONFINITE
 * (:1298 drops it). */
int ldso_pixsel_make_points(ldso_pixsel_t *p, ldso_pyramid_t *pyr, int host_index, int *n_out);
/* the records of the last ldso_pixsel_make_points and their my_type on the host (type_out optional) / as device pointers (valid until the next make_points
 * or destroy; immature_dev is what ldso_trace_append_points_device takes) */
int ldso_pixsel_get_points(ldso_pixsel_t *p, ldso_immature_t *out, float *type_out_or_null);
int ldso_pixsel_device(ldso_pixsel_t *p, const void **immature_dev, const void **type_dev, int *n);
/* enable != 0: the calls bracket their kernels with HIP events; us_out[5] (optional) = microseconds of the last profiled make_maps + make_points:
 * histogram (:36-109), masks + scan, select (both summed over the recursion's passes), thinning (:150-163), records */
int ldso_pixsel_profile(ldso_pixsel_t *p, int enable, float us_out[5]);

/* ------------------------------------------------------------------------------------------------------------
 * Raw camera frames: Undistort::undistort<T> (src/frontend/Undistort.cc:357-457) = PhotometricUndistorter::processFrame (:189-227) and the bilinear remap
 * (:390-443) as one kernel.  The raw 8- or 16-bit frame goes up (1 or 2 bytes per pixel), the irradiance is written into a frame's pyramid and
 * FrameHessian::makeImages follows on the same stream: the frame never exists on the host as floats.  The calibration arrives as the plain arrays the
 * reference's constructors leave (Undistort::remapX / remapY, Undistort.h:105-106; PhotometricUndistorter::G, GDepth, vignetteMapInv, Undistort.h:56-59).
 * The result is bit for bit what the reference returns, with ONE deliberate difference: the validity rule of the tables (:853-864) compares the row with
 * wOrg - 1 (not hOrg - 1), so a table can hold rows at or beyond hOrg - 1; the reference's range check (:428) zeroes them except for xxi == 0 && yyi == hOrg - 1,
 * which reads one row past the end of the source image.  Here a pixel whose four taps are not all inside the wOrg x hOrg image is 0 and nothing outside
 * the raw buffer is read, whatever the tables hold.  benchmark_varNoise / benchmark_varBlurNoise (:376-413, :468-555; both 0 in Setting.cc) are out of scope.
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct ldso_undistorter ldso_undistorter_t;
/* wOrg x hOrg: the raw frame (Undistort::getOriginalSize), w x h: the output (getSize).  Tables are set by the two calls below before the first frame. */
int ldso_undist_create(int device, int wOrg, int hOrg, int w, int h, ldso_undistorter_t **out);
int ldso_undist_destroy(ldso_undistorter_t *u);
int ldso_undist_set_stream(ldso_undistorter_t *u, void *hip_stream);
/* Undistort::remapX / remapY (w*h floats each, copied).  Both NULL: passthrough (rectification "none", :450-452; needs w == wOrg && h == hOrg).
 * LDSO_E_INVALID for a non-finite entry. */
int ldso_undist_set_remap(ldso_undistorter_t *u, const float *remapX, const float *remapY);
/* PhotometricUndistorter::G (GDepth entries, 256..65536, as the constructor :43-158 leaves them) and vignetteMapInv (wOrg*hOrg, required for mode 2), copied;
 * G == NULL: no valid calibration (:197 `!valid`), every frame takes factor * raw.  photometricCalibration = setting_photometricCalibration (0, 1, 2),
 * useExposure = setting_useExposure. */
int ldso_undist_set_photometric(ldso_undistorter_t *u, const float *G, int GDepth, const float *vignetteMapInv, int photometricCalibration, int useExposure);
/* undistort<unsigned char / unsigned short>(image_raw, exposure, timestamp, factor): raw = wOrg*hOrg pixels of bytes_per_pixel (1 | 2) bytes, copied to a pinned
 * staging buffer before the call returns.  Copy, kernel, and - with a pyramid (w x h, same device) - its build and its `ready` event are enqueued on the
 * undistorter's stream; no host synchronisation.  Without a pyramid the irradiance stays in the undistorter's own buffer.  *exposure_out (optional) =
 * ImageAndExposure::exposure_time (:203, :220, :224-225).  The writes into the pyramid are ordered on the undistorter's stream only, as those of
 * ldso_pyr_make_images are on its stream: handing in a pyramid that a consumer on another stream may still be reading is the caller's to avoid.  LDSO_E_INVALID for a 16-bit frame on a calibrated path with fewer than 65536 entries of G
 * (the reference indexes G unchecked). */
int ldso_undist_frame(ldso_undistorter_t *u, const void *raw, int bytes_per_pixel, float exposure, float factor, ldso_pyramid_t *pyr_or_null, float *exposure_out);
/* the last frame's irradiance (w*h floats) on the host (synchronises) / as a device pointer: the pyramid's staging when the frame went into one (valid
 * while that pyramid lives and holds this frame), else the undistorter's buffer (valid until the next frame) */
int ldso_undist_get(ldso_undistorter_t *u, float *irradiance_out);
int ldso_undist_device(ldso_undistorter_t *u, const void **dev_ptr);
/* enable != 0: ldso_undist_frame brackets its stages with HIP events; us_out[3] (optional) = microseconds of the last profiled frame: copy of the raw
 * frame, undistortion kernel, pyramid build (this call waits for that frame) */
int ldso_undist_profile(ldso_undistorter_t *u, int enable, float us_out[3]);
/* A group of undistorters: Undistort::undistort<T> (Undistort.cc:357-457) of the raw frames of many sequences on one card.  n ldso_undist_frame calls are n
 * copies, n launches and n x 2 x levels pyramid launches; a group call stages the raw frames of all active members and its job table into one pinned arena,
 * moves them in ONE copy (1 or 2 bytes per pixel), undistorts them in ONE launch and - into a pyramid group - builds the pyramids in at most 2 x Lmax more.
 * Every member's irradiance and every pyramid level hold the bytes ldso_undist_frame gives them.  1 <= n <= 128 undistorters on one device and one stream
 * (ldso_undist_set_stream; checked at create and at every call); sizes, tables, calibration and settings are free per member.  An undistorter belongs to at
 * most one group and stays usable on its own between group calls; ldso_undist_destroy of a member is refused while the group lives. */
typedef struct ldso_undist_group ldso_undist_group_t;
int ldso_undist_group_create(ldso_undistorter_t *const *u, int n, ldso_undist_group_t **out);
int ldso_undist_group_destroy(ldso_undist_group_t *g);
/* ldso_undist_frame of every active member (active: n bytes or NULL = all; entries of inactive members are read in none of the arrays): raw[i] = wOrg_i * hOrg_i
 * pixels of bytes_per_pixel[i] (1 | 2) bytes, copied to the group's pinned arena before the call returns (the caller may reuse them at once).  Copy, kernel and
 * the pyramid builds are enqueued on the members' stream; no host synchronisation.  pyr_group_or_null == NULL: every member's irradiance stays in its own
 * buffer.  Otherwise a pyramid group of exactly n members on the same device: pyramid i takes the frame of undistorter i (w x h of every active pair must
 * match), and exactly the active members' pyramids are built and get their `ready` events, as by ldso_pyr_group_make_images_device.  exposure_out (n floats or
 * NULL): ImageAndExposure::exposure_time per active member; entries of inactive members are not written.  Afterwards ldso_undist_get / ldso_undist_device
 * answer per member.  LDSO_E_INVALID before anything is staged or enqueued, every member's last output untouched, the message naming the member at fault:
 * a NULL array, no active member, a NULL raw frame, a bytes_per_pixel other than 1 or 2, a member without ldso_undist_set_remap, a 16-bit frame on a
 * calibrated path with fewer than 65536 entries of G, members no longer on one stream, a pyramid group of another length, size or device. */
int ldso_undist_group_frames(ldso_undist_group_t *g, const uint8_t *active /* n or NULL */, const void *const *raw /* n */, const int *bytes_per_pixel /* n */,
                             const float *exposure /* n */, const float *factor /* n */, ldso_pyr_group_t *pyr_group_or_null, float *exposure_out /* n or NULL */);
/* as ldso_undist_profile, of the last profiled group call: the one copy, the undistortion kernel, the grouped pyramid build */
int ldso_undist_group_profile(ldso_undist_group_t *g, int enable, float us_out[3]);

/* ------------------------------------------------------------------------------------------------------------
 * Monocular initialiser: CoarseInitializer (src/frontend/CoarseInitializer.cc, include/frontend/CoarseInitializer.h).
 * Replaces setFirst (:547-619) twice over: ldso_init_set_first takes finished point records (selection and neighbours are the caller's), ldso_init_set_first_frame
 * further down takes a resident pyramid and does the pixel selection of every level, the records and the k-d tree searches of makeNN itself;
 * trackFrame (:40-178) and what it calls: calcResAndGS (:181-405), calcEC (:412-428), optReg (:430-459), propagateUp/Down
 * (:462-522), resetPoints (:621-643), doStep (:645-671), applyStep (:673-687), makeK (:689-715).
 * The whole Levenberg-Marquardt loop of one trackFrame runs on the device without a host round trip.
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct ldso_initializer ldso_initializer_t;
int ldso_init_create(int device, int w, int h, int pyr_levels, ldso_initializer_t **out);
int ldso_init_destroy(ldso_initializer_t *t);
int ldso_init_set_stream(ldso_initializer_t *t, void *hip_stream);
/* makeK + setFirst: calib = CalibHessian fxl,fyl,cxl,cyl of level 0; the first frame as raw irradiance (w*h floats, makeImages on
 * the device) with its exposure; points[lvl] / n_points[lvl]: the selected pixels of every level with neighbours and parents. */
int ldso_init_set_first(ldso_initializer_t *t, const float calib[4], const float *irradiance, float ab_exposure,
                        const ldso_init_point_t *const *points, const int *n_points, float huberTH, int fixAffine);
/* trackFrame(newFrame): returns the state after the call in state_out (optional) */
int ldso_init_track_frame(ldso_initializer_t *t, const float *irradiance, float ab_exposure, ldso_init_state_t *state_out);
int ldso_init_get_state(ldso_initializer_t *t, ldso_init_state_t *state_out);
int ldso_init_set_state(ldso_initializer_t *t, const ldso_init_state_t *state);
int ldso_init_get_points(ldso_initializer_t *t, int lvl, ldso_init_point_t *points_out);
int ldso_init_set_points(ldso_initializer_t *t, int lvl, const ldso_init_point_t *points);
/* stage entry for parity tests: one calcResAndGS(lvl, refToNew, aff) on the current new frame; idepth_new of the points is used
 * as it stands.  H,Hsc 8x8 row-major, b,bsc 8, res = (E.A, alphaEnergy, E.num), ec = calcEC(lvl). */
int ldso_init_calc_res_and_gs(ldso_initializer_t *t, int lvl, const double refToNew[12], double aff_a, double aff_b,
                              float *H, float *b, float *Hsc, float *bsc, float *res, float *ec);
/* debug entries for the tests of the evaluation kernel (tests/test_init_stage_gpu.py); neither is part of trackFrame.
 * get_jb: JbBuffer_new [n][10] of level lvl as the last evaluation wrote it (rows of points that are not good after it are not written).
 * eval_step: one evaluation as trackFrame runs it, outside of it: the lazily applied applyStep of an accepted step (apply_pending), then resetPoints'
 *   per-point part (mode 0) or doStep with inc[8] and lambda on the JbBuffer the previous evaluation wrote (mode 1), then calcResAndGS and calcEC at the
 *   resulting idepth_new.  Outputs as ldso_init_calc_res_and_gs.  No step is pending afterwards; the next ldso_init_track_frame starts as after any other call. */
int ldso_init_debug_get_jb(ldso_initializer_t *t, int lvl, float *jb_out);
int ldso_init_debug_eval_step(ldso_initializer_t *t, int lvl, int mode, int apply_pending, const float inc[8], float lambda, const double refToNew[12],
                              double aff_a, double aff_b, float *H, float *b, float *Hsc, float *bsc, float *res, float *ec);
int ldso_init_set_new_frame(ldso_initializer_t *t, const float *irradiance, float ab_exposure);
/* Launch schedule of ldso_init_track_frame (tuning / debugging; the results do not depend on it, bit for bit: tests/test_init_gpu.py).
 * first_steps: control steps (evaluation + control launch) enqueued before the state is read back for the first time; the rest of the
 *   frame's maximum is enqueued only if the frame has not finished by then.  0 (default) = what the previous frame took + 25 % + 4 (first frame: half of the maximum).
 * prepare_on_grid: 1 (default) = the inputs of the optReg sweeps are prepared by a grid kernel between evaluation and control step
 *   once the initialiser has snapped; 0 = by the control block itself (one compute unit), as in the frame that snaps. */
int ldso_init_set_schedule(ldso_initializer_t *t, int first_steps, int prepare_on_grid);
/* Host logic, no device: the schedule of the in-place optReg sweep (CoarseInitializer.cc:430-459: points are updated in index order, reading neighbours that
 * may already have been updated) as ldso_init_set_first builds it for one level.  neighbours [n][10] (-1 = none), width = points per pass (32 on the device).
 * pass_out[i] = pass of point i: every neighbour j < i in an earlier pass, every neighbour j > i in the same or a later one, <= width points per pass.
 * Returns the number of passes, or a negative LDSO_E_* code. */
int ldso_init_sweep_schedule(int n, const int *neighbours, int width, int *pass_out);
/* debug builds (LDSO_STAMPS=1): accumulated device-side counters, zeros otherwise */
int ldso_init_debug_counters(ldso_initializer_t *t, long long out[8]);

/* ------------------------------------------------------------------------------------------------------------
 * setFirst from a resident pyramid (CoarseInitializer.cc:547-619): the pixel selection of every level (level 0: PixelSelector::makeMaps with thFactor 2
 * on the caller's selector; levels >= 1: makePixelStatus, include/frontend/PixelSelector2.h:63-277), the Pnt records (:567-603) and makeNN (:717-783) with the
 * k-d tree built and searched as nanoflann does it (include/frontend/nanoflann.h): on pixel grids most rows have equally distant candidates for their last
 * places, and which of them a row keeps is decided by the tree's leaf order and traversal, not by any tie rule.  Selection, records and searches run on the
 * device; the tree is built on the host (sequential in the reference as well: planeSplit permutes one array in place), as are the sweep schedules of
 * ldso_init_set_first, which this entry reuses.
 * ------------------------------------------------------------------------------------------------------------ */
/* The members of Pnt that setFirst and makeNN leave uninitialised (the reference allocates with new Pnt[npts]) are DEFINED here, once, as the existing
 * records of ldso_init_set_first's callers have them: idepth_new = 1, everything else 0. */
#define LDSO_INIT_POINT_FILL_UNSET(p) do { (p).idepth_new = 1.0f; (p).maxstep = 0.0f; (p).iRSumNum = 0.0f; (p).isGood_new = 0; \
                                           (p).energy_new[0] = 0.0f; (p).energy_new[1] = 0.0f; (p).pad_ = 0.0f; } while (0)
/* One node of the tree, in nanoflann's allocation order (a node, then child1's subtree, then child2's; node 0 is the root).
 * Leaf: child1 = child2 = -1, the points are vind[left_or_feat .. right).  Inner node: left_or_feat = divfeat (0: u, 1: v), divlow / divhigh as :1036-1037. */
typedef struct ldso_nn_node {
    int32_t child1, child2;
    int32_t left_or_feat, right;
    float divlow, divhigh;
} ldso_nn_node_t;                     /* 24 bytes */
typedef struct ldso_nn_tree ldso_nn_tree_t;
/* Host only, no device.  buildIndex (:827-834) with leaf size 5 over n > 0 points (uv: n pairs u, v; copied).  LDSO_E_INVALID for a non-finite position. */
int ldso_init_nn_build(int n, const float *uv, ldso_nn_tree_t **out);
int ldso_init_nn_free(ldso_nn_tree_t *tree);
/* every output optional.  depth = inner nodes above the deepest leaf (what a search's stack must hold); root_box = low u, high u, low v, high v */
int ldso_init_nn_info(const ldso_nn_tree_t *tree, int *n, int *n_nodes, int *depth, float root_box[4]);
/* the node array (n_nodes entries) and nanoflann's permuted index array vind (n entries), either optional */
int ldso_init_nn_get(const ldso_nn_tree_t *tree, ldso_nn_node_t *nodes_out, int32_t *vind_out);
/* findNeighbors (:869-881) with a KNNResultSet of k entries for n_query positions: idx_out / dist_out [n_query][k], the squared distances ascending, places
 * the tree could not fill hold -1 / FLT_MAX.  k is 1 or 10, the two sizes makeNN uses (LDSO_E_UNSUPPORTED otherwise). */
int ldso_init_nn_search_host(const ldso_nn_tree_t *tree, int n_query, const float *query_uv, int k, int32_t *idx_out, float *dist_out);
/* Host only, no device: the scalar arithmetic of makePixelStatus :253-276 behind one gridMaxSelection pass that set n_good pixels with block size `sparsity`
 * (>= 1) and th_fac.  *action = 1: select again with *new_sparsity and *new_th_fac, recs_left - 1; 0: done.  *new_sparsity is what sparsityFactor becomes
 * either way. */
int ldso_init_pixel_status_plan(int n_good, float desired, int sparsity, int recs_left, float th_fac, int *action, int *new_sparsity, float *new_th_fac);
/* sparsityFactor (a process-wide global in the reference, 5 in Setting.cc:126) is state of the handle: it starts at 5 and is carried from level to level and
 * from one first frame to the next, as the global is. */
int ldso_init_set_sparsity(ldso_initializer_t *t, int sparsity);
int ldso_init_get_sparsity(ldso_initializer_t *t, int *sparsity);
/* Stage entry: makePixelStatus(dIp[lvl], map, w >> lvl, h >> lvl, desired_density, recs_left, th_fac) on level lvl >= 1 of the pyramid (same device and size
 * as the handle), from the handle's sparsity, which it updates.  One wait per pass.  *n_out = its return value (pixels set anywhere on the level, not the record
 * count), *passes_out = gridMaxSelection passes run.  A non-finite gradient gives LDSO_E_NONFINITE (the map is still there; a NaN never wins a comparison); a pyramid
 * built by this library holds none above level 0's intensity, makeImages zeroes a non-finite dx / dy (FrameHessian.cc:86-87). */
int ldso_init_pixel_status(ldso_initializer_t *t, ldso_pyramid_t *pyr, int lvl, float desired_density, int recs_left, float th_fac, int *n_out, int *passes_out);
/* the byte map (0 / 1) of the last pixel-status pass, (w >> lvl) * (h >> lvl) bytes of the level it ran on; *lvl_out optional */
int ldso_init_get_status_map(ldso_initializer_t *t, unsigned char *map_out, int *lvl_out);
/* Stage entry: the searches of makeNN on the device for arbitrary positions.  uv[l] = n[l] pairs (copied), n[l] >= 10.  The trees are built on the host, one
 * lane searches for one point.  Per level, each optional: nb_idx / nb_dist [n][10] = the 10 nearest of the same level and their squared distances in result
 * order; parent_idx / parent_dist [n] = the nearest point of level l + 1 to (u, v) * 0.5 - (0.25, 0.25) (level n_levels - 1: -1 / -1).
 * LDSO_E_UNSUPPORTED, before anything is launched, for a level with fewer than 10 points or a tree deeper than 64. */
int ldso_init_make_nn(ldso_initializer_t *t, int n_levels, const float *const *uv, const int *n, int32_t *const *nb_idx_out, float *const *nb_dist_out,
                      int32_t *const *parent_idx_out, float *const *parent_dist_out);
/* makeK + setFirst on the frame the pyramid holds (built by ldso_pyr_make_images or ldso_undist_frame; at least the handle's levels and three, same device and
 * size): level 0 through ldso_pixsel_set_potential(3) and ldso_pixsel_make_maps(0.03 * w * h, 1, th_factor 2) on `pixsel`, levels >= 1 through makePixelStatus
 * with densities {0.03, 0.05, 0.15, 0.5, 1}[lvl] * w * h, the records in raster order over patternPadding + 1 <= x < wl - patternPadding - 2 (likewise y),
 * the searches; then everything ldso_init_set_first does with finished records.  The handle's first-frame images are device copies of the pyramid's levels.
 * n_points_out[lvl] (optional) = numPoints[lvl].  ldso_init_get_points afterwards returns all fields of the records, neighboursDist, parentDist and my_type
 * included.  Two calls on the same input leave byte-identical records and maps.  Defined where the reference is not:
 *   - more than 5 levels (densities[5] is read past the array): LDSO_E_UNSUPPORTED.  ldso_init_create already refuses such a handle;
 *   - a level with fewer than 10 records (makeNN copies stale ret_index entries into the neighbour list): LDSO_E_UNSUPPORTED, before any search is launched;
 *   - a width or height that is no multiple of 32: the code of ldso_pixsel_make_maps, passed on;
 *   - more than 36000 records on a level: LDSO_E_INVALID, as ldso_init_set_first;
 *   - a non-finite gradient: LDSO_E_NONFINITE, by the rule of ldso_pixsel_make_maps (a NaN never wins a comparison).
 * After any of these the handle holds no first frame and takes the next one as a fresh handle would; the sparsity keeps what the passes that ran left. */
int ldso_init_set_first_frame(ldso_initializer_t *t, const float calib[4], ldso_pyramid_t *pyr, float ab_exposure, ldso_pixsel_t *pixsel, float huberTH,
                              int fixAffine, int n_points_out[]);
/* enable != 0: ldso_init_set_first_frame times its stages (each ends in a wait; host clock between the waits); us_out[6] (optional) = microseconds of the last
 * profiled call: level-0 maps, coarser-level maps, records, tree build on the host, searches, schedule build with its uploads and the image copies */
int ldso_init_first_profile(ldso_initializer_t *t, int enable, float us_out[6]);

#ifdef __cplusplus
}
#endif
#endif /* LDSO_HIP_H_ */
