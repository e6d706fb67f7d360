// initializer_api.hip — the handle of the monocular initialiser and the ldso_init_* functions (include/ldso_hip.h): the first frame with its points and sweep
// schedules, the frames to track, state and point fetches (SoA on the device <-> ldso_init_point_t records).  The kernels are initializer.hip, the optReg
// schedule initializer_sched.cpp, what the files share is initializer.h.
#include "initializer.h"

template <class T> static int ini_upload(ldso_initializer *H, T **dst, const std::vector<T> &src) {
    DALLOC(H->levelAllocs, *dst, src.size());
    if (!src.empty()) CHK(hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    return LDSO_OK;
}

// SoA <-> record conversion: the float arrays of a level with the record members they hold
#define INI_FIELDS(X) X(u, u) X(v, v) X(idepth, idepth) X(idepth_new, idepth_new) X(iR, iR) X(iRSumNum, iRSumNum) X(lastHessian, lastHessian) X(lastHessian_new, lastHessian_new) \
                      X(maxstep, maxstep) X(outlierTH, outlierTH) X(energy0, energy[0]) X(energy1, energy[1]) X(energy_new0, energy_new[0]) X(energy_new1, energy_new[1])

static int ini_put_points(ldso_initializer *H, int l, const ldso_init_point_t *pts) {
    IniLevel &L = H->P.L[l];
    const int n = H->n[l];
    std::vector<float> f(n);
    std::vector<int> g(n);
#define X(dst, expr) for (int i = 0; i < n; i++) f[i] = pts[i].expr; if (n) CHK(hipMemcpy(L.dst, f.data(), (size_t) n * 4, hipMemcpyHostToDevice));
    INI_FIELDS(X)
#undef X
#define XI(dst, expr) for (int i = 0; i < n; i++) g[i] = pts[i].expr; if (n) CHK(hipMemcpy(L.dst, g.data(), (size_t) n * 4, hipMemcpyHostToDevice));
    XI(isGood, isGood) XI(isGood_new, isGood_new)
#undef XI
    return LDSO_OK;
}

extern "C" {

static int ini_create_body(ldso_initializer *H, int device, int w, int h, int levels) {
    H->device = device; H->w = w; H->h = h; H->levels = levels;
    CHK(hipStreamCreateWithFlags(&H->stream, hipStreamNonBlocking));
    H->ownStream = true;
    memset(&H->P, 0, sizeof(H->P));
    H->P.levels = levels; H->P.fixAffine = 1; H->P.huberTH = 9.0f; H->P.firstExposure = 1; H->P.newExposure = 1;
    for (int l = 0; l < levels; l++) {
        const size_t npx = (size_t) (w >> l) * (h >> l);
        DALLOC(H->allocs, H->d_first[l], npx * 3); DALLOC(H->allocs, H->d_new[l], npx * 3);
        H->P.L[l].first = H->d_first[l]; H->P.L[l].cur = H->d_new[l];
        H->P.L[l].w = w >> l; H->P.L[l].h = h >> l;
    }
    DALLOC(H->allocs, H->d_color, (size_t) w * h);
    DALLOC(H->allocs, H->P.ctl, 1);
    DALLOC(H->allocs, H->P.part, (size_t) INI_MAXBLK * INI_NPART);
    IniCtl c; memset(&c, 0, sizeof(c));
    c.Tcur[0] = c.Tcur[5] = c.Tcur[10] = 1.0; c.Tnew[0] = c.Tnew[5] = c.Tnew[10] = 1.0; c.frameID = -1; c.done = 1;
    CHK(hipMemcpy(H->P.ctl, &c, sizeof(c), hipMemcpyHostToDevice));
    return LDSO_OK;
}

int ldso_init_create(int device, int w, int h, int levels, ldso_initializer_t **out) {
    REQ(out && w > 16 && h > 16 && levels >= 1 && levels <= INI_MAXL && (w >> (levels - 1)) >= 8, "ldso_init_create: bad arguments (at most 5 pyramid levels)");
    RUN(open_device(device, "ldso_init_create"));
    ldso_initializer *H = new ldso_initializer();
    return finish_create(ini_create_body(H, device, w, h, levels), H, out, ldso_init_destroy);      // nothing of a half-built handle leaks
}

int ldso_init_destroy(ldso_initializer_t *H) {
    if (!H) return LDSO_OK;
    hipSetDevice(H->device);
    hipDeviceSynchronize();
    for (void *p : H->allocs) hipFree(p);
    for (void *p : H->levelAllocs) hipFree(p);
    for (void *p : H->firstAllocs) hipFree(p);
    if (H->ownStream && H->stream) hipStreamDestroy(H->stream);
    delete H;
    return LDSO_OK;
}

int ldso_init_set_stream(ldso_initializer_t *H, void *s) {
    REQ(H, "null handle");
    return swap_stream(H->stream, H->ownStream, s);
}

static int ini_images(ldso_initializer *H, const float *irr, float *const *levels) {
    CHK(hipSetDevice(H->device));
    RUN(raw_to_images(H->d_color, irr, H->w, H->h, H->levels, levels, H->stream));
    CHK(hipStreamSynchronize(H->stream));      // the host buffer may be reused by the caller
    return LDSO_OK;
}

int ldso_init_set_first(ldso_initializer_t *H, const float calib[4], const float *irradiance, float ab_exposure,
                        const ldso_init_point_t *const *points, const int *n_points, float huberTH, int fixAffine) {
    REQ(H && calib && irradiance && points && n_points, "ldso_init_set_first: null argument");
    RUN(ini_set_first_records(H, calib, ab_exposure, points, n_points, huberTH, fixAffine));
    RUN(ini_images(H, irradiance, H->d_first));
    H->haveFirst = true; H->haveNew = false;
    return LDSO_OK;
}

}  // extern "C"

int ini_set_first_records(ldso_initializer *H, const float calib[4], float ab_exposure, const ldso_init_point_t *const *points, const int *n_points, float huberTH, int fixAffine) {
    CHK(hipSetDevice(H->device));
    CHK(hipStreamSynchronize(H->stream));
    for (void *p : H->levelAllocs) hipFree(p);
    H->levelAllocs.clear();
    H->P.huberTH = huberTH; H->P.fixAffine = fixAffine ? 1 : 0; H->P.firstExposure = ab_exposure;
    // makeK (:689-715): doubles from the float level-0 intrinsics
    double fx[INI_MAXL], fy[INI_MAXL], cx[INI_MAXL], cy[INI_MAXL];
    fx[0] = calib[0]; fy[0] = calib[1]; cx[0] = calib[2]; cy[0] = calib[3];
    for (int l = 1; l < H->levels; l++) {
        fx[l] = fx[l - 1] * 0.5; fy[l] = fy[l - 1] * 0.5;
        cx[l] = (cx[0] + 0.5) / ((int) 1 << l) - 0.5; cy[l] = (cy[0] + 0.5) / ((int) 1 << l) - 0.5;
    }
    size_t maxN = 64;
    for (int l = 0; l < H->levels; l++) {
        IniLevel &L = H->P.L[l];
        const int n = n_points[l];
        REQ(n >= 0 && n <= 36000, "ldso_init_set_first: more than 36000 points on one level (LDS working set of the sweeps)");
        REQ(n == 0 || points[l], "ldso_init_set_first: null point array");
        H->n[l] = n; L.n = n;
        maxN = std::max<size_t>(maxN, n);
        L.fx = (float) fx[l]; L.fy = (float) fy[l]; L.cx = (float) cx[l]; L.cy = (float) cy[l];
        // K^-1 of the upper-triangular K in double (Eigen's cofactor inverse gives the same entries up to 1 ulp of double)
        for (int q = 0; q < 9; q++) L.Ki[q] = 0;
        L.Ki[0] = 1.0 / fx[l]; L.Ki[2] = -cx[l] / fx[l]; L.Ki[4] = 1.0 / fy[l]; L.Ki[5] = -cy[l] / fy[l]; L.Ki[8] = 1.0;
#define X(name, member) DALLOC(H->levelAllocs, L.name, n);
        INI_FIELDS(X)
        X(isGood,) X(isGood_new,)
#undef X
        DALLOC(H->levelAllocs, L.jb[0], (size_t) n * 10); DALLOC(H->levelAllocs, L.jb[1], (size_t) n * 10);
        const ldso_init_point_t *pts = points[l];
        const int nUp = (l + 1 < H->levels) ? n_points[l + 1] : 0, nDown = (l > 0) ? n_points[l - 1] : 0;
        std::vector<int> parent(n), nb((size_t) n * INI_NB, -1);
        for (int i = 0; i < n; i++) {
            parent[i] = pts[i].parent;
            REQ(l + 1 >= H->levels || (parent[i] >= 0 && parent[i] < nUp), "ldso_init_set_first: parent index out of range");
            for (int q = 0; q < 10; q++) {
                const int j = pts[i].neighbours[q];
                REQ(j >= -1 && j < n, "ldso_init_set_first: neighbour index out of range");
                nb[(size_t) i * INI_NB + q] = j;
            }
        }
        RUN(ini_upload(H, &L.parent, parent));
        RUN(ini_upload(H, &L.nb, nb));
        // optReg sweep schedule (all levels; two lanes per point: passes of <= 32 points): ini_sweep_schedule
        {
            std::vector<int> pass(n, 0), nb10((size_t) n * 10);
            for (int i = 0; i < n; i++) for (int q = 0; q < 10; q++) nb10[(size_t) i * 10 + q] = nb[(size_t) i * INI_NB + q];
            L.nPass2 = ini_sweep_schedule(n, nb10.data(), 32, pass.data());
            std::vector<int> slotOf(n), at(L.nPass2, 0), idleSlot;
            for (int i = 0; i < n; i++) slotOf[i] = pass[i] * 32 + at[pass[i]]++;
            for (int p = 0; p < L.nPass2 + INI_SWPAD; p++) for (int q = (p < L.nPass2 ? at[p] : 0); q < 32; q++) idleSlot.push_back(p * 32 + q);
            L.nIdle = (int) idleSlot.size();
            { int *p = nullptr; RUN(ini_upload(H, &p, slotOf)); L.slotOf = p; }
            { int *p = nullptr; RUN(ini_upload(H, &p, idleSlot)); L.idleSlot = p; }
            DALLOC(H->levelAllocs, L.swRec, (size_t) (L.nPass2 + INI_SWPAD) * 64 * 2);      // per-lane inputs: ini_prep writes them before every sweep (the places without a point: once)
        }
        if (l + 1 < H->levels) { L.nPass = 0; L.sched = nullptr; L.schedOff = nullptr; L.schedNb = nullptr; }
        else {
        // resetPoints sweep schedule (top level): dep(i) = max(dep(j) + 1 over neighbours j < i, dep(k) over readers k < i of i)
        std::vector<int> dep(n, 0);
        {
            std::vector<int> rd(n, 0);      // max dep of the lower-indexed readers seen so far
            for (int i = 0; i < n; i++) {
                int d = rd[i];
                for (int q = 0; q < 10; q++) { const int j = nb[(size_t) i * INI_NB + q]; if (j >= 0 && j < i) d = std::max(d, dep[j] + 1); }
                dep[i] = d;
                for (int q = 0; q < 10; q++) { const int j = nb[(size_t) i * INI_NB + q]; if (j > i) rd[j] = std::max(rd[j], d); }
            }
        }
        int nDep = 0;
        for (int i = 0; i < n; i++) nDep = std::max(nDep, dep[i] + 1);
        std::vector<std::vector<int>> byDep(nDep);
        for (int i = 0; i < n; i++) byDep[dep[i]].push_back(i);
        std::vector<int> sched;
        for (int d = 0; d < nDep; d++)
            for (size_t o = 0; o < byDep[d].size(); o += 64) {
                for (size_t q = 0; q < 64; q++) sched.push_back(o + q < byDep[d].size() ? byDep[d][o + q] : -1);
            }
        L.nPass = (int) (sched.size() / 64);
        sched.resize(sched.size() + (size_t) INI_SWPAD * 64, -1);
        { int *p = nullptr; RUN(ini_upload(H, &p, sched)); L.sched = p; }
        {
            const int dummy = n * 4;
            std::vector<int> snb(sched.size() * INI_NB, dummy), soff(sched.size(), dummy);
            for (size_t q = 0; q < sched.size(); q++)
                if (sched[q] >= 0) {
                    soff[q] = sched[q] * 4;
                    for (int e = 0; e < 10; e++) { const int j = nb[(size_t) sched[q] * INI_NB + e]; snb[q * INI_NB + e] = (j >= 0) ? j * 4 : dummy; }
                }
            int *p = nullptr; int r_ = ini_upload(H, &p, snb); if (r_ != LDSO_OK) return r_; L.schedNb = p;
            p = nullptr; r_ = ini_upload(H, &p, soff); if (r_ != LDSO_OK) return r_; L.schedOff = p;
        }
        }
        // children lists (points of level l-1 whose parent is p), ascending child index
        std::vector<int> off(n + 1, 0), idx(nDown);
        if (l > 0) {
            const ldso_init_point_t *ch = points[l - 1];
            for (int c = 0; c < nDown; c++) { REQ(ch[c].parent >= 0 && ch[c].parent < n, "ldso_init_set_first: parent index out of range"); off[ch[c].parent + 1]++; }
            for (int p = 0; p < n; p++) off[p + 1] += off[p];
            std::vector<int> cur(off.begin(), off.end() - 1);
            for (int c = 0; c < nDown; c++) idx[cur[ch[c].parent]++] = c;
        }
        { int *p = nullptr; RUN(ini_upload(H, &p, off)); L.childOff = p; }
        { int *p = nullptr; RUN(ini_upload(H, &p, idx)); L.childIdx = p; }
        RUN(ini_put_points(H, l, pts));
    }
    H->ldsBytes = (maxN + INI_LDS_EXTRA) * sizeof(float);
    H->prepBlocks = (int) std::max<size_t>(1, (maxN + INI_PT - 1) / INI_PT);
    CHK(ini_ctl_reserve_lds(H->ldsBytes));
    H->snappedAtFrameStart = false;
    // state of setFirst (:612-614)
    IniCtl c; memset(&c, 0, sizeof(c));
    c.Tcur[0] = c.Tcur[5] = c.Tcur[10] = 1.0; c.Tnew[0] = c.Tnew[5] = c.Tnew[10] = 1.0; c.done = 1;
    CHK(hipMemcpy(H->P.ctl, &c, sizeof(c), hipMemcpyHostToDevice));
    for (int l = 0; l < INI_MAXL; l++) H->firstRec[l].clear();
    return LDSO_OK;
}

extern "C" {

int ldso_init_set_new_frame(ldso_initializer_t *H, const float *irradiance, float ab_exposure) {
    REQ(H && irradiance, "ldso_init_set_new_frame: null argument");
    REQ(H->haveFirst, "ldso_init_set_new_frame: no first frame");
    H->P.newExposure = ab_exposure;
    int r_ = ini_images(H, irradiance, H->d_new);
    if (r_ != LDSO_OK) return r_;
    H->haveNew = true;
    return LDSO_OK;
}

int ldso_init_get_state(ldso_initializer_t *H, ldso_init_state_t *s) {
    REQ(H && s, "null argument");
    CHK(hipSetDevice(H->device));
    IniCtl c;
    CHK(hipMemcpyAsync(&c, H->P.ctl, sizeof(c), hipMemcpyDeviceToHost, H->stream));
    CHK(hipStreamSynchronize(H->stream));
    memcpy(s->thisToNext, c.Tcur, sizeof(c.Tcur));
    H->snappedAtFrameStart = c.snapped != 0; H->frameDone = c.done != 0; H->stepsTaken = c.steps;
    s->aff_a = c.aCur; s->aff_b = c.bCur; s->snapped = c.snapped; s->snappedAt = c.snappedAt; s->frameID = c.frameID;
    s->ready = c.snapped && c.frameID > c.snappedAt + 5; s->evals = c.evals; s->pad_ = 0;
    return LDSO_OK;
}

int ldso_init_set_state(ldso_initializer_t *H, const ldso_init_state_t *s) {
    REQ(H && s, "null argument");
    CHK(hipSetDevice(H->device));
    IniCtl c;
    CHK(hipMemcpyAsync(&c, H->P.ctl, sizeof(c), hipMemcpyDeviceToHost, H->stream));
    CHK(hipStreamSynchronize(H->stream));
    memcpy(c.Tcur, s->thisToNext, sizeof(c.Tcur)); memcpy(c.Tnew, s->thisToNext, sizeof(c.Tnew));
    c.aCur = (float) s->aff_a; c.bCur = (float) s->aff_b; c.aNew = c.aCur; c.bNew = c.bCur;
    c.snapped = s->snapped; c.snappedAt = s->snappedAt; c.frameID = s->frameID;
    H->snappedAtFrameStart = c.snapped != 0;
    CHK(hipMemcpyAsync(H->P.ctl, &c, sizeof(c), hipMemcpyHostToDevice, H->stream));
    CHK(hipStreamSynchronize(H->stream));
    return LDSO_OK;
}

int ldso_init_track_frame(ldso_initializer_t *H, const float *irradiance, float ab_exposure, ldso_init_state_t *state_out) {
    REQ(H, "null handle");
    REQ(H->haveFirst, "ldso_init_track_frame: no first frame");
    CHK(hipSetDevice(H->device));
    if (irradiance) RUN(ldso_init_set_new_frame(H, irradiance, ab_exposure));
    REQ(H->haveNew, "ldso_init_track_frame: no new frame");
    const int maxIterations[5] = {5, 5, 10, 30, 50};
    int steps = 0;                                                          // the most control steps a frame can take
    for (int l = 0; l < H->levels; l++) steps += maxIterations[l] + 2;
    steps += 2 * (H->levels - 1);                                           // the transition steps of a snapped frame (down and up)
    // Control steps behind the one that finishes the frame return at once, but each still costs a dispatch (2-3 us, three kernels per step): a frame takes 19-40 of
    // the 58 possible steps at four levels.  So: enqueue what the previous frame took plus a margin, read the state back (the call does that anyway), and enqueue
    // the rest only if the frame is not finished - one more round trip in the rare case, 10-30 empty steps fewer in the usual one.  (First frame: half of the maximum.)
    int first = std::min(steps, H->firstSteps > 0 ? H->firstSteps : H->lastSteps > 0 ? H->lastSteps + H->lastSteps / 4 + 4 : (steps + 1) / 2);
    const bool prep = H->snappedAtFrameStart && H->prepareOnGrid;
    ini_launch_ctl(H->P, INI_BEGIN, H->ldsBytes, H->stream);
    ldso_init_state_t st;
    for (int from = 0; from < steps;) {
        for (int p = from; p < first; p++) {
            ini_launch_eval(H->P, 0, H->stream);
            if (prep) ini_launch_prep(H->P, H->prepBlocks, H->stream);
            ini_launch_ctl(H->P, INI_STEP, H->ldsBytes, H->stream);
        }
        CHK(hipGetLastError());
        int r_ = ldso_init_get_state(H, &st);
        if (r_ != LDSO_OK) return r_;
        if (H->frameDone) break;
        from = first; first = steps;
    }
    REQ(H->frameDone, "ldso_init_track_frame: the frame did not finish within the maximal number of control steps (internal)");
    H->lastSteps = H->stepsTaken;
    bool fin = true;
    for (int q = 0; q < 12; q++) fin = fin && std::isfinite(st.thisToNext[q]);
    if (state_out) *state_out = st;
    if (!fin) { ldso_set_error("ldso_init_track_frame: non-finite pose"); return LDSO_E_NONFINITE; }
    return LDSO_OK;
}

int ldso_init_set_schedule(ldso_initializer_t *H, int first_steps, int prepare_on_grid) {
    REQ(H && first_steps >= 0, "ldso_init_set_schedule: bad argument");
    H->firstSteps = first_steps; H->prepareOnGrid = prepare_on_grid != 0;
    return LDSO_OK;
}

// debug (LDSO_STAMPS builds): accumulated device-side ticks (100 MHz): sweep ticks, sweep passes, control-kernel ticks, sweeps, fill + prepare ticks,
// ticks up to the accept decision, ticks of the next increment (solve, exp), -
int ldso_init_debug_counters(ldso_initializer_t *H, long long out[8]) {
    REQ(H && out, "null argument");
    CHK(hipSetDevice(H->device));
    CHK(hipStreamSynchronize(H->stream));
    IniCtl c;
    CHK(hipMemcpy(&c, H->P.ctl, sizeof(c), hipMemcpyDeviceToHost));
    out[0] = c.dbgSweepTicks; out[1] = c.dbgSweepPasses; out[2] = c.dbgCtlTicks; out[3] = c.dbgSweeps; out[4] = c.dbgPrepTicks; out[5] = c.dbgFrontTicks; out[6] = c.dbgTailTicks; out[7] = c.dbgSpare;
    return LDSO_OK;
}

int ldso_init_get_points(ldso_initializer_t *H, int l, ldso_init_point_t *out) {
    REQ(H && out && l >= 0 && l < H->levels, "ldso_init_get_points: bad argument");
    CHK(hipSetDevice(H->device));
    CHK(hipStreamSynchronize(H->stream));
    IniCtl c;
    CHK(hipMemcpy(&c, H->P.ctl, sizeof(c), hipMemcpyDeviceToHost));
    REQ(!c.applyPending, "ldso_init_get_points: a step is pending (internal)");
    const IniLevel &L = H->P.L[l];
    const int n = H->n[l];
    std::vector<float> f(n);
    std::vector<int> g(n), nb((size_t) n * INI_NB);
#define X(src, expr) if (n) CHK(hipMemcpy(f.data(), L.src, n * 4, hipMemcpyDeviceToHost)); for (int i = 0; i < n; i++) out[i].expr = f[i];
    INI_FIELDS(X)
#undef X
#define XI(src, expr) if (n) CHK(hipMemcpy(g.data(), L.src, n * 4, hipMemcpyDeviceToHost)); for (int i = 0; i < n; i++) out[i].expr = g[i];
    XI(isGood, isGood) XI(isGood_new, isGood_new) XI(parent, parent)
#undef XI
    if (n) CHK(hipMemcpy(nb.data(), L.nb, (size_t) n * INI_NB * 4, hipMemcpyDeviceToHost));
    for (int i = 0; i < n; i++) for (int q = 0; q < 10; q++) out[i].neighbours[q] = nb[(size_t) i * INI_NB + q];
    // what the device arrays do not carry comes from the records ldso_init_set_first_frame built, where it built them
    if ((int) H->firstRec[l].size() == n)
        for (int i = 0; i < n; i++) {
            const ldso_init_point_t &r = H->firstRec[l][i];
            out[i].parentDist = r.parentDist; out[i].my_type = r.my_type; out[i].pad_ = r.pad_;
            for (int q = 0; q < 10; q++) out[i].neighboursDist[q] = r.neighboursDist[q];
        }
    return LDSO_OK;
}

int ldso_init_set_points(ldso_initializer_t *H, int l, const ldso_init_point_t *pts) {
    REQ(H && pts && l >= 0 && l < H->levels, "ldso_init_set_points: bad argument");
    CHK(hipSetDevice(H->device));
    CHK(hipStreamSynchronize(H->stream));
    return ini_put_points(H, l, pts);
}

// One evaluation outside trackFrame: the control record c goes up, k_ini_eval (stage: calcResAndGS alone; otherwise as a step of trackFrame) and the
// summing part of the control step run, and what they leave in the record is handed out.
static int ini_stage_eval(ldso_initializer *H, IniCtl &c, int stage, float *Hm, float *b, float *Hsc, float *bsc, float *res, float *ec) {
    CHK(hipMemcpy(H->P.ctl, &c, sizeof(c), hipMemcpyHostToDevice));
    ini_launch_eval(H->P, stage, H->stream);
    ini_launch_ctl(H->P, INI_STAGE, H->ldsBytes, H->stream);
    CHK(hipGetLastError());
    CHK(hipStreamSynchronize(H->stream));
    CHK(hipMemcpy(&c, H->P.ctl, sizeof(c), hipMemcpyDeviceToHost));
    if (Hm) memcpy(Hm, c.Hn, sizeof(c.Hn));
    if (b) memcpy(b, c.bn, sizeof(c.bn));
    if (Hsc) memcpy(Hsc, c.Hscn, sizeof(c.Hscn));
    if (bsc) memcpy(bsc, c.bscn, sizeof(c.bscn));
    if (res) memcpy(res, c.resNew, sizeof(c.resNew));
    if (ec) memcpy(ec, c.ec, sizeof(c.ec));
    return LDSO_OK;
}

int ldso_init_calc_res_and_gs(ldso_initializer_t *H, int lvl, const double refToNew[12], double aff_a, double aff_b,
                              float *Hm, float *b, float *Hsc, float *bsc, float *res, float *ec) {
    REQ(H && refToNew && lvl >= 0 && lvl < H->levels, "ldso_init_calc_res_and_gs: bad argument");
    REQ(H->haveFirst && H->haveNew, "ldso_init_calc_res_and_gs: frames missing");
    CHK(hipSetDevice(H->device));
    CHK(hipStreamSynchronize(H->stream));
    IniCtl c;
    CHK(hipMemcpy(&c, H->P.ctl, sizeof(c), hipMemcpyDeviceToHost));
    memcpy(c.Tnew, refToNew, sizeof(c.Tnew));
    c.aNew = (float) aff_a; c.bNew = (float) aff_b; c.lvl = lvl;
    return ini_stage_eval(H, c, 1, Hm, b, Hsc, bsc, res, ec);
}

int ldso_init_debug_eval_step(ldso_initializer_t *H, int lvl, int mode, int apply_pending, const float inc[8], float lambda, const double refToNew[12],
                              double aff_a, double aff_b, float *Hm, float *b, float *Hsc, float *bsc, float *res, float *ec) {
    REQ(H && inc && refToNew && lvl >= 0 && lvl < H->levels && (mode == 0 || mode == 1), "ldso_init_debug_eval_step: bad argument");
    REQ(H->haveFirst && H->haveNew, "ldso_init_debug_eval_step: frames missing");
    CHK(hipSetDevice(H->device));
    CHK(hipStreamSynchronize(H->stream));
    IniCtl c;
    CHK(hipMemcpy(&c, H->P.ctl, sizeof(c), hipMemcpyDeviceToHost));
    memcpy(c.Tnew, refToNew, sizeof(c.Tnew));
    c.aNew = (float) aff_a; c.bNew = (float) aff_b; c.lvl = lvl;
    c.mode = mode; c.applyPending = apply_pending ? 1 : 0; c.lambda = lambda; c.done = 0; c.sweepDue = 0;
    memcpy(c.inc, inc, sizeof(c.inc));
    c.jbSel ^= 1;                                                           // as an accepted step does: what the previous evaluation wrote is JbBuffer now
    RUN(ini_stage_eval(H, c, 0, Hm, b, Hsc, bsc, res, ec));
    c.applyPending = 0;                                                     // the step is applied; ldso_init_get_points takes the handle again
    CHK(hipMemcpy(H->P.ctl, &c, sizeof(c), hipMemcpyHostToDevice));
    return LDSO_OK;
}

int ldso_init_debug_get_jb(ldso_initializer_t *H, int lvl, float *out) {
    REQ(H && out && lvl >= 0 && lvl < H->levels, "ldso_init_debug_get_jb: bad argument");
    REQ(H->haveFirst, "ldso_init_debug_get_jb: no first frame");
    CHK(hipSetDevice(H->device));
    CHK(hipStreamSynchronize(H->stream));
    IniCtl c;
    CHK(hipMemcpy(&c, H->P.ctl, sizeof(c), hipMemcpyDeviceToHost));
    if (H->n[lvl]) CHK(hipMemcpy(out, H->P.L[lvl].jb[c.jbSel ^ 1], (size_t) H->n[lvl] * 10 * sizeof(float), hipMemcpyDeviceToHost));
    return LDSO_OK;
}

}  // extern "C"
