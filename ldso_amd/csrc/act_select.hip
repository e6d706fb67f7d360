// act_select.hip — which immature points get activated, on the device (gfx950): the first half of FullSystem::activatePointsMT (reference
// src/frontend/FullSystem.cc:1052-1152) with CoarseDistanceMap::makeDistanceMap / growDistBFS / addIntoDistFinal (src/frontend/CoarseTracker.cc:686-818).
//
// One persistent workgroup.  The level-1 distance map is one byte per cell (0..39, 255 = the reference's 1000) in LDS where it fits (320 x 240 = 76 800 B of the
// CU's 160 KiB) and in global memory otherwise - the same code either way.
//   phase A (all waves)  fill, project the seeds, grow 39 rounds in parallel (a round writes k into every far cell next to a cell of value k - 1 that is not on
//                        the border: exactly the reference's frontier, whose order within a round does not matter), then every candidate's canActivate / delete
//                        rules, projection and bounds test, and the distance test against the INITIAL map: map values only ever decrease, so a candidate that
//                        fails it here fails it at its turn too - only the others stay pending.
//   phase B (wave 0)     the pending candidates in order; an accepted one is inserted as addIntoDistFinal does: cell = 0, then the pruned BFS from that single
//                        seed over a frontier list (a cell joins the next frontier only when the round lowered it), until the frontier is empty.
// Float projections in the reference's operation order, no contraction, IEEE division, int conversion by truncation after + 0.5f (as trace.hip, ba_activate.hip).
// For a batch of windows (ldso_ba_batch_select_candidates / _select_activate_points / _select_activate_tracers / _activate_points, at the end of the file) the same body
// runs as one workgroup per window in one launch, k_act_select_batch, each window with its own sizes and map placement.
//
// The host side, behind the kernels: all eight entries of point activation (ldso_ba_activate_points, the three single-window selections, the four batched calls).  What
// can be said of a selection without a device - the job, its checks, the layout of its arenas, packing and unpacking - is act_stage.h, once for both paths; this file
// adds the device: sel_args (regions -> pointers), sel_arena (growth of ldso_ba::d_sel), sel_lds_rule (the map in LDS or not), act_preconditions, then sel_run for one window
// and batch_select_run for a batch, each: check every job, lay out, stage, fill SelArgs, launch, download, unpack.
#include <hip/hip_runtime.h>
#include "ba_host.h"
#include "act_stage.h"

namespace {

constexpr int SEL_THREADS = 1024;
constexpr int SEL_FRONTIER = 512;                 // a round's frontier lies on the octagon of radius k <= 39 around the seed: at most 8 k = 312 cells
constexpr int SEL_LIST_BYTES = 2 * SEL_FRONTIER * 4;
constexpr int SEL_LDS_MAX = 160 * 1024;
constexpr int SEL_PENDING = 3;                    // internal: passed every rule and the test against the initial map
constexpr unsigned char SEL_FAR = 255;

struct SelArgs {
    const ldso_act_seed_t *seeds;
    const ldso_immature_t *pts;
    const float *myType, *KRKi, *Kt;
    const int32_t *flagged;
    int nSeeds, n, nHosts, w1, h1;
    float minDist, minQuality;
    // the seeds straight from a resident window instead of `seeds` (pgeo != null): every point whose host is not `newestHost`, at its CURRENT inverse depth
    // (PointHessian::idepth_scaled, CoarseTracker.cc:706-709)
    const PtGeo *pgeo;
    const int32_t *phost;
    int nWin;
    int newestHost;                               // candidates hosted by this frame are no candidates (FullSystem.cc:1089): KEEP, never touched; < 0: none
    unsigned char *gmap;                          // [w1 * h1] the map in global memory: the working copy of the large path, the final map of both
    int ldsMap;                                   // k_act_select_batch: this window's working map lies in LDS (k_act_select has the choice as its template argument)
    int32_t *decision, *selected, *nSelected, *cell;
    float *frac, *thr;
};

static __device__ __forceinline__ float map_value(unsigned char m) { return m == SEL_FAR ? 1000.0f : (float) m; }

// Vec3f ptp = KRKi * Vec3f(u, v, 1) + Kt * idepth; int u = ptp[0] / ptp[2] + 0.5f (CoarseTracker.cc:709-712, FullSystem.cc:1130-1135)
static __device__ __forceinline__ bool project(const float *KRKi, const float *Kt, float pu, float pv, float idepth, int w1, int h1, int &u, int &v, float &p0) {
    p0 = ((KRKi[0] * pu + KRKi[1] * pv) + KRKi[2] * 1.0f) + Kt[0] * idepth;
    const float p1 = ((KRKi[3] * pu + KRKi[4] * pv) + KRKi[5] * 1.0f) + Kt[1] * idepth;
    const float p2 = ((KRKi[6] * pu + KRKi[7] * pv) + KRKi[8] * 1.0f) + Kt[2] * idepth;
    u = (int) (p0 / p2 + 0.5f);
    v = (int) (p1 / p2 + 0.5f);
    return u > 0 && v > 0 && u < w1 && v < h1;
}

// addIntoDistFinal(u, v) by one wavefront: growDistBFS(1) from the single seed.  Lanes take the frontier's cells 64 at a time and step through the neighbour
// directions together: within one direction two different cells never share a neighbour, so a cell is lowered (and listed) once per round.
static __device__ void insert_seed(unsigned char *map, uint32_t *listA, uint32_t *listB, int cellIdx, int w1, int h1, int lane) {
    uint32_t *cur = listA, *nxt = listB;
    if (lane == 0) { map[cellIdx] = 0; cur[0] = (uint32_t) (cellIdx % w1) | ((uint32_t) (cellIdx / w1) << 16); }
    __threadfence_block();
    int cnt = 1;
    for (int k = 1; k < 40 && cnt > 0; k++) {
        const int ndir = (k & 1) ? 8 : 4;
        int ncnt = 0;
        for (int p = 0; p < cnt; p += 64) {
            const int e = p + lane;
            int x = 0, y = 0;
            bool act = e < cnt;
            if (act) {
                const uint32_t c = cur[e];
                x = (int) (c & 0xffffu); y = (int) (c >> 16);
                act = !(x == 0 || y == 0 || x == w1 - 1 || y == h1 - 1);          // a border cell holds a value but never spreads (CoarseTracker.cc:736, :764)
            }
            for (int d = 0; d < ndir; d++) {
                // the reference's order: +x, -x, +y, -y, then (+,+), (-,+), (-,-), (+,-)
                const int dx = (d == 0 || d == 4 || d == 7) ? 1 : (d == 1 || d == 5 || d == 6) ? -1 : 0;
                const int dy = (d == 2 || d == 4 || d == 5) ? 1 : (d == 3 || d == 6 || d == 7) ? -1 : 0;
                const int nx = x + dx, ny = y + dy;
                bool set = false;
                if (act) {
                    const int j = nx + ny * w1;
                    if (map[j] > k) { map[j] = (unsigned char) k; set = true; }
                }
                const unsigned long long bm = __ballot(set);
                if (set) {
                    const int pos = ncnt + __popcll(bm & ((1ull << lane) - 1ull));
                    if (pos < SEL_FRONTIER) nxt[pos] = (uint32_t) nx | ((uint32_t) ny << 16);
                }
                ncnt += __popcll(bm);
                __threadfence_block();
            }
        }
        uint32_t *t = cur; cur = nxt; nxt = t;
        cnt = ncnt < SEL_FRONTIER ? ncnt : SEL_FRONTIER;
    }
}

// One window's selection by one workgroup: the body of k_act_select and k_act_select_batch.  sel_lds: the workgroup's dynamic LDS, [frontier lists | the map if LDS].
template <bool LDS>
static __device__ __forceinline__ void act_select_body(const SelArgs &A, unsigned char *sel_lds) {
    uint32_t *listA = (uint32_t *) sel_lds, *listB = listA + SEL_FRONTIER;
    unsigned char *map = LDS ? sel_lds + SEL_LIST_BYTES : A.gmap;
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63;
    const int w1 = A.w1, h1 = A.h1, wh = w1 * h1;

    // ---- makeDistanceMap (CoarseTracker.cc:686-721) ----
    for (int i = tid; i < wh; i += nt) map[i] = SEL_FAR;
    __syncthreads();
    for (int i = tid; i < A.nSeeds; i += nt) {
        const ldso_act_seed_t s = A.seeds[i];
        if (s.host < 0 || s.host >= A.nHosts) continue;
        int u, v; float p0;
        if (project(A.KRKi + 9 * s.host, A.Kt + 3 * s.host, s.u, s.v, s.idepth_scaled, w1, h1, u, v, p0)) map[u + w1 * v] = 0;
    }
    if (A.pgeo) for (int i = tid; i < A.nWin; i += nt) {
        const int host = A.phost[i];
        if (host < 0 || host >= A.nHosts || host == A.newestHost) continue;
        const PtGeo &g = A.pgeo[i];
        int u, v; float p0;
        if (project(A.KRKi + 9 * host, A.Kt + 3 * host, g.u, g.v, g.idepth, w1, h1, u, v, p0)) map[u + w1 * v] = 0;
    }
    __syncthreads();
    // ---- growDistBFS (CoarseTracker.cc:723-811): every cell is far or final here, so the frontier of round k is the set of cells holding k - 1 ----
    for (int k = 1; k < 40; k++) {
        int spread = 0;
        for (int i = tid; i < wh; i += nt) {
            if (map[i] != k - 1) continue;
            const int x = i % w1, y = i / w1;
            if (x == 0 || y == 0 || x == w1 - 1 || y == h1 - 1) continue;
            spread = 1;
            if (map[i + 1] > k) map[i + 1] = (unsigned char) k;
            if (map[i - 1] > k) map[i - 1] = (unsigned char) k;
            if (map[i + w1] > k) map[i + w1] = (unsigned char) k;
            if (map[i - w1] > k) map[i - w1] = (unsigned char) k;
            if (k & 1) {
                if (map[i + 1 + w1] > k) map[i + 1 + w1] = (unsigned char) k;
                if (map[i - 1 + w1] > k) map[i - 1 + w1] = (unsigned char) k;
                if (map[i - 1 - w1] > k) map[i - 1 - w1] = (unsigned char) k;
                if (map[i + 1 - w1] > k) map[i + 1 - w1] = (unsigned char) k;
            }
        }
        if (!__syncthreads_or(spread)) break;
    }

    // ---- the candidate rules of FullSystem.cc:1096-1149, in parallel; the distance test against the initial map ----
    for (int i = tid; i < A.n; i += nt) {
        const ldso_immature_t &P = A.pts[i];
        const int host = P.host, st = P.lastTraceStatus;
        const float idmin = P.idepth_min, idmax = P.idepth_max;
        int dec = LDSO_ACT_KEEP;
        if (A.newestHost >= 0 && host == A.newestHost) { A.decision[i] = dec; continue; }                                                  // :1089
        if (host < 0 || host >= A.nHosts || !isfinite(idmax) || st == LDSO_IPS_OUTLIER) dec = LDSO_ACT_DROP;                               // :1105
        else {
            const bool canActivate = (st == LDSO_IPS_GOOD || st == LDSO_IPS_SKIPPED || st == LDSO_IPS_BADCONDITION || st == LDSO_IPS_OOB)
                                     && P.lastTracePixelInterval < 8 && P.quality > A.minQuality && (idmax + idmin) > 0;                   // :1111-1117
            if (!canActivate) { if (A.flagged[host] != 0 || st == LDSO_IPS_OOB) dec = LDSO_ACT_DROP; }                                     // :1121-1124
            else {
                int u, v; float p0;
                if (!project(A.KRKi + 9 * host, A.Kt + 3 * host, P.u, P.v, 0.5f * (idmax + idmin), w1, h1, u, v, p0)) dec = LDSO_ACT_DROP; // :1145-1148
                else {
                    const int c = u + w1 * v;
                    const float fr = p0 - floorf(p0), th = A.minDist * A.myType[i];                                                        // :1137-1141
                    if (map_value(map[c]) + fr >= th) { dec = SEL_PENDING; A.cell[i] = c; A.frac[i] = fr; A.thr[i] = th; }
                }
            }
        }
        A.decision[i] = dec;
    }
    __syncthreads();

    // ---- the greedy pass of FullSystem.cc:1137-1144 over the pending candidates, in order ----
    if (tid < 64) {
        int nsel = 0;
        for (int base = 0; base < A.n; base += 64) {
            const int i = base + lane;
            int dec = i < A.n ? A.decision[i] : LDSO_ACT_KEEP;
            int c = 0; float fr = 0, th = 0;
            if (dec == SEL_PENDING) { c = A.cell[i]; fr = A.frac[i]; th = A.thr[i]; }
            unsigned long long m = __ballot(dec == SEL_PENDING);
            while (m) {
                const int b = __ffsll((long long) m) - 1;
                m &= m - 1;
                const int cc = __shfl(c, b, 64);
                const float f = __shfl(fr, b, 64), t = __shfl(th, b, 64);
                const bool accept = map_value(map[cc]) + f >= t;
                if (lane == b) dec = accept ? LDSO_ACT_SELECTED : LDSO_ACT_KEEP;
                if (accept) {
                    if (lane == 0) A.selected[nsel] = base + b;
                    nsel++;
                    insert_seed(map, listA, listB, cc, w1, h1, lane);
                }
            }
            if (i < A.n) A.decision[i] = dec;
        }
        if (lane == 0) *A.nSelected = nsel;
    }
    __syncthreads();
    if (LDS) for (int i = tid; i < wh; i += nt) A.gmap[i] = map[i];
}

template <bool LDS>
__global__ __launch_bounds__(SEL_THREADS) void k_act_select(SelArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sel_lds[];
    act_select_body<LDS>(A, sel_lds);
}

// The windows of a batch in one launch (ldso_ba_batch_select_candidates / _select_activate_points): workgroup b runs the selection tab[b] describes, sizes and map
// placement its own.  The launch's dynamic LDS is that of the largest map that lies in LDS.
__global__ __launch_bounds__(SEL_THREADS) void k_act_select_batch(const SelArgs *tab) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sel_lds[];
    SelArgs A = tab[blockIdx.x];
    // pointers that come out of a table are generic to the compiler; all of these lie in global memory, and saying so keeps the body on global_load / global_store
#define SEL_GLOBAL(p) p = (decltype(p)) (__attribute__((address_space(1))) void *) (uintptr_t) (p)
    SEL_GLOBAL(A.seeds); SEL_GLOBAL(A.pts); SEL_GLOBAL(A.myType); SEL_GLOBAL(A.KRKi); SEL_GLOBAL(A.Kt); SEL_GLOBAL(A.flagged); SEL_GLOBAL(A.gmap); SEL_GLOBAL(A.decision);
    SEL_GLOBAL(A.selected); SEL_GLOBAL(A.nSelected); SEL_GLOBAL(A.cell); SEL_GLOBAL(A.frac); SEL_GLOBAL(A.thr); SEL_GLOBAL(A.pgeo); SEL_GLOBAL(A.phost);
#undef SEL_GLOBAL
    if (A.ldsMap) act_select_body<true>(A, sel_lds);
    else act_select_body<false>(A, sel_lds);
}

// ---- the host side.  What a job is, its checks, where its bytes lie and the two host copies: act_stage.h, for the single-window entries and the batch alike; here: what
// needs the device ----

// the kernel's view of job J: its regions on the device addresses of the three arenas, its map at gmap
SelArgs sel_args(const ActJob &J, const ActRegions &R, char *dUp, char *dDown, char *dScr, unsigned char *gmap, float minQuality) {
    SelArgs A;
    memset(&A, 0, sizeof(A));
    A.seeds = (const ldso_act_seed_t *) (dUp + R.seeds); A.pts = (const ldso_immature_t *) (dUp + R.pts); A.myType = (const float *) (dUp + R.type);
    A.KRKi = (const float *) (dUp + R.KRKi); A.Kt = (const float *) (dUp + R.Kt); A.flagged = (const int32_t *) (dUp + R.flag);
    A.nSeeds = J.nSeeds; A.n = J.n; A.nHosts = J.nHosts; A.w1 = J.w1; A.h1 = J.h1; A.minDist = J.minDist; A.minQuality = minQuality; A.newestHost = -1; A.gmap = gmap;
    A.nSelected = (int32_t *) (dDown + R.nSel); A.decision = (int32_t *) (dDown + R.dec); A.selected = (int32_t *) (dDown + R.sel);
    A.cell = (int32_t *) (dScr + R.cell); A.frac = (float *) (dScr + R.frac); A.thr = (float *) (dScr + R.thr);
    return A;
}

// H's device arena with at least `need` bytes; one that is too small is replaced by one of `room`, and the map the last selection left in it is gone with it
int sel_arena(ldso_ba *H, size_t need, size_t room) {
    if (need <= H->selCap) return LDSO_OK;
    if (H->d_sel) hipFree(H->d_sel);
    H->d_sel = nullptr; H->selCap = 0; H->selW1 = 0; H->selH1 = 0;
    CHK(hipMalloc(&H->d_sel, room));
    H->selCap = room;
    return LDSO_OK;
}

// A map of mapBytes lies in LDS (ldsMap) where a workgroup of `kernel` can have that much beside the frontier lists and the kernel's own static bytes, in global memory
// otherwise.  ldsBytes: the launch's dynamic LDS, raised to hold the map; limit / set: what the owner of the kernel's attribute remembers (-1: not asked yet; raised to).
int sel_lds_rule(const void *kernel, int device, int &limit, int &set, size_t mapBytes, size_t &ldsBytes, int &ldsMap) {
    if (limit < 0) {
        hipFuncAttributes fa; int perBlock = 0;
        CHK(hipFuncGetAttributes(&fa, kernel));
        CHK(hipDeviceGetAttribute(&perBlock, hipDeviceAttributeMaxSharedMemoryPerBlock, device));
        limit = std::max(0, std::min(perBlock, SEL_LDS_MAX) - (int) fa.sharedSizeBytes);
    }
    ldsMap = SEL_LIST_BYTES + mapBytes <= (size_t) limit ? 1 : 0;
    if (ldsMap) ldsBytes = std::max(ldsBytes, SEL_LIST_BYTES + mapBytes);
    if (ldsMap && (int) ldsBytes > set) { CHK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) ldsBytes)); set = (int) ldsBytes; }
    return LDSO_OK;
}

// what point activation needs of the resident window; n_hosts: the frames the caller brought poses for
int act_preconditions(const ldso_ba *H, const std::string &who, int n_hosts, bool images = true) {
    REQ(H->D.F >= 2, who + ": set the window and the frames first");
    REQ(n_hosts == H->D.F, who + ": one KRKi / Kt / flag per frame of the resident window");
    for (int f = 0; images && f < H->D.F; f++) REQ(H->B.img[f] != nullptr, who + ": a key-frame image is missing");
    return LDSO_OK;
}

struct SelCall { ActRegions R; ActBases total; SelArgs A; char *dDown = nullptr; };          // an enqueued single-window selection: its regions, arena sizes and device view

// One window alone: the arena is H->d_sel, [upload | download | scratch | map], staged through H->selHost.  Selection, k_activate on the selected list where the selection
// kernel left it if the job wants records, and the download, all enqueued; the caller waits and unpacks.  T: the tracer of a resident job.
int sel_run(ldso_ba *H, const char *who, const ActJob &J, const ldso_tracer *T, float minQuality, int min_obs, float min_idepth_hessian, int gn_iterations, SelCall &C) {
    RUN(act_job_check(J, who, ACT_MISSING_SOLO));
    CHK(hipSetDevice(H->device));
    C.R = act_layout(J, C.total);
    const ActBases &t = C.total;
    const size_t oMap = t.up + t.down + t.scratch, total = oMap + C.R.mapBytes;
    RUN(sel_arena(H, total, total + total / 2));
    char *d = (char *) H->d_sel, *hs;
    C.dDown = d + t.up;
    H->selHost.resize(std::max(t.up, t.down));
    hs = H->selHost.data();
    memset(hs, 0, t.up);
    act_pack(J, C.R, hs);
    CHK(hipMemcpyAsync(d, hs, t.up, hipMemcpyHostToDevice, H->stream));
    SelArgs &A = C.A;
    A = sel_args(J, C.R, d, C.dDown, C.dDown + t.down, (unsigned char *) d + oMap, minQuality);
    // the seeds straight from the resident window: every point whose host is not the newest frame
    if (J.resident) { A.pts = T->d_pts; A.myType = T->d_type; A.pgeo = H->B.pgeo; A.phost = H->B.phost; A.nWin = H->D.P; A.newestHost = J.nHosts - 1; }
    size_t ldsBytes = SEL_LIST_BYTES;
    RUN(sel_lds_rule((const void *) k_act_select<true>, H->device, H->selLdsLimit, H->selLdsSet, C.R.mapBytes, ldsBytes, A.ldsMap));
    if (A.ldsMap) hipLaunchKernelGGL(k_act_select<true>, dim3(1), dim3(SEL_THREADS), ldsBytes, H->stream, A);
    else hipLaunchKernelGGL(k_act_select<false>, dim3(1), dim3(SEL_THREADS), ldsBytes, H->stream, A);
    CHK(hipGetLastError());
    H->selW1 = J.w1; H->selH1 = J.h1; H->selMapOffset = oMap;
    if (J.records) CHK(ba_launch_activate(H->B, H->D, H->settings, act_win(A.pts, (ldso_activation_t *) (C.dDown + C.R.act), J.n, min_obs, min_idepth_hessian, gn_iterations, A.selected, A.nSelected, 0).A, H->stream));
    CHK(hipMemcpyAsync(hs, C.dDown, t.down, hipMemcpyDeviceToHost, H->stream));
    return LDSO_OK;
}

}  // namespace

extern "C" {

// The density controller of FullSystem::activatePointsMT (FullSystem.cc:1054-1073), its mixed if / else-if ladder as written: currentMinActDist is a float,
// the constants are doubles, ef->nPoints an int against float * double.
int ldso_act_update_min_dist(float current, int nPoints, float desiredDensity, float *out) {
    REQ(out, "ldso_act_update_min_dist: null argument");
    float currentMinActDist = current;
    if (nPoints < desiredDensity * 0.66)
        currentMinActDist -= 0.8;
    if (nPoints < desiredDensity * 0.8)
        currentMinActDist -= 0.5;
    else if (nPoints < desiredDensity * 0.9)
        currentMinActDist -= 0.2;
    else if (nPoints < desiredDensity)
        currentMinActDist -= 0.1;

    if (nPoints > desiredDensity * 1.5)
        currentMinActDist += 0.8;
    if (nPoints > desiredDensity * 1.3)
        currentMinActDist += 0.5;
    if (nPoints > desiredDensity * 1.15)
        currentMinActDist += 0.2;
    if (nPoints > desiredDensity)
        currentMinActDist += 0.1;

    if (currentMinActDist < 0) currentMinActDist = 0;
    if (currentMinActDist > 4) currentMinActDist = 4;
    *out = currentMinActDist;
    return LDSO_OK;
}

// FullSystem::optimizeImmaturePoint (FullSystem.cc:892-1010) for n immature points against the key frames of the window that is resident in the handle
// (ldso_ba_set_image*, ldso_ba_set_window, ldso_ba_set_frames: images, calibration, current poses).  Its arena, d_act [n records | n results], stays its own: in d_sel
// the call would overwrite, or with a larger n take away, the distance map ldso_ba_get_distance_map still reads.
int ldso_ba_activate_points(ldso_ba_t *H, int n, const ldso_immature_t *pts, int min_obs, float min_idepth_hessian, int gn_iterations, ldso_activation_t *out) {
    REQ(H && n >= 0 && (n == 0 || (pts && out)) && gn_iterations >= 0, "ldso_ba_activate_points: bad arguments");
    RUN(act_preconditions(H, "ldso_ba_activate_points", H->D.F, n > 0));
    if (n == 0) return LDSO_OK;
    CHK(hipSetDevice(H->device));
    if (n > H->actCap) {
        if (H->d_act) hipFree(H->d_act);
        H->d_act = nullptr; H->actCap = 0;
        CHK(hipMalloc(&H->d_act, (size_t) n * (sizeof(ldso_immature_t) + sizeof(ldso_activation_t))));
        H->actCap = n;
    }
    ldso_immature_t *dp = (ldso_immature_t *) H->d_act;
    ldso_activation_t *dout = (ldso_activation_t *) ((char *) H->d_act + (size_t) H->actCap * sizeof(ldso_immature_t));
    CHK(hipMemcpyAsync(dp, pts, (size_t) n * sizeof(ldso_immature_t), hipMemcpyHostToDevice, H->stream));
    CHK(ba_launch_activate(H->B, H->D, H->settings, act_win(dp, dout, n, min_obs, min_idepth_hessian, gn_iterations, nullptr, nullptr, 0).A, H->stream));
    CHK(hipMemcpyAsync(out, dout, (size_t) n * sizeof(ldso_activation_t), hipMemcpyDeviceToHost, H->stream));
    CHK(hipStreamSynchronize(H->stream));
    return LDSO_OK;
}

// makeDistanceMap + the selection loop of FullSystem::activatePointsMT (FullSystem.cc:1080-1152, CoarseTracker.cc:686-818)
int ldso_ba_select_candidates(ldso_ba_t *H, int n_seeds, const ldso_act_seed_t *seeds, int n, const ldso_immature_t *points, const float *my_type, int n_hosts, const float *KRKi,
                              const float *Kt, const int32_t *host_flagged, float currentMinActDist, float minTraceQuality, int32_t *decision_out, int32_t *selected_out,
                              int *n_selected_out) {
    REQ(H && (n <= 0 || decision_out), "ldso_ba_select_candidates: bad arguments");
    const ActJob J = act_job(n_seeds, seeds, n, points, my_type, n_hosts, KRKi, Kt, host_flagged, currentMinActDist, H->w, H->h, false, decision_out, selected_out, nullptr);
    SelCall C;
    RUN(sel_run(H, "ldso_ba_select_candidates", J, nullptr, minTraceQuality, 0, 0.0f, 0, C));
    CHK(hipStreamSynchronize(H->stream));
    const int ns = act_unpack(J, C.R, H->selHost.data());
    if (n_selected_out) *n_selected_out = ns;
    return LDSO_OK;
}

// ... followed by the optimizeImmaturePoint loop (FullSystem.cc:1154-1164, 892-1010) on the selected list, which never leaves the device: k_activate reads the
// list and its length where the selection kernel left them.  One synchronisation.  out[k] belongs to candidate selected_out[k], k < *n_selected_out.
int ldso_ba_select_activate_points(ldso_ba_t *H, int n_seeds, const ldso_act_seed_t *seeds, int n, const ldso_immature_t *points, const float *my_type, int n_hosts,
                                   const float *KRKi, const float *Kt, const int32_t *host_flagged, float currentMinActDist, float minTraceQuality, int min_obs,
                                   float min_idepth_hessian, int gn_iterations, int32_t *decision_out, int32_t *selected_out, int *n_selected_out, ldso_activation_t *out) {
    REQ(H && gn_iterations >= 0 && n_selected_out && (n <= 0 || (decision_out && selected_out && out)), "ldso_ba_select_activate_points: bad arguments");
    RUN(act_preconditions(H, "ldso_ba_select_activate_points", n_hosts));
    const ActJob J = act_job(n_seeds, seeds, n, points, my_type, n_hosts, KRKi, Kt, host_flagged, currentMinActDist, H->w, H->h, true, decision_out, selected_out, out);
    SelCall C;
    RUN(sel_run(H, "ldso_ba_select_activate_points", J, nullptr, minTraceQuality, min_obs, min_idepth_hessian, gn_iterations, C));
    CHK(hipStreamSynchronize(H->stream));
    *n_selected_out = act_unpack(J, C.R, H->selHost.data());
    return LDSO_OK;
}

// The same with nothing of the immature set crossing PCIe: the candidates are the tracer's resident records and types where they lie, the seeds the points of
// the resident window at their current inverse depth, and with compact != 0 everything the loop did not KEEP leaves the tracer's set behind the activation
// (FullSystem.cc:1105-1108, :1121-1125, :1145-1148 the deleted candidates; :1166-1188 the selected ones, accepted or not).  All on the handle's stream, one wait.
int ldso_ba_select_activate_tracer(ldso_ba_t *H, ldso_tracer_t *T, int n_hosts, const float *KRKi, const float *Kt, const int32_t *host_flagged, float currentMinActDist,
                                   float minTraceQuality, int min_obs, float min_idepth_hessian, int gn_iterations, int compact, int32_t *decision_out, int32_t *selected_out,
                                   int *n_selected_out, ldso_activation_t *out, int *n_left_out) {
    REQ(H && T && gn_iterations >= 0 && n_selected_out, "ldso_ba_select_activate_tracer: bad arguments");
    const int n = T->n;
    REQ(n <= 0 || (decision_out && selected_out && out), "ldso_ba_select_activate_tracer: bad arguments");
    REQ(T->device == H->device, "ldso_ba_select_activate_tracer: the tracer and the window live on different devices");
    REQ_UNSHARDED("ldso_ba_select_activate_tracer");
    RUN(act_preconditions(H, "ldso_ba_select_activate_tracer", n_hosts));
    ActJob J = act_job(0, nullptr, n, nullptr, nullptr, n_hosts, KRKi, Kt, host_flagged, currentMinActDist, H->w, H->h, true, decision_out, selected_out, out);
    J.resident = true;
    SelCall C;
    RUN(sel_run(H, "ldso_ba_select_activate_tracer", J, T, minTraceQuality, min_obs, min_idepth_hessian, gn_iterations, C));
    const int rcCompact = compact ? trace_compact_enqueue(T, nullptr, C.A.decision, LDSO_ACT_KEEP, n_hosts, false, H->stream) : LDSO_OK;
    CHK(hipStreamSynchronize(H->stream));          // also where the compaction could not be enqueued: the copy into selHost is in flight
    if (rcCompact != LDSO_OK) return rcCompact;
    if (compact) trace_compact_finish(T);
    *n_selected_out = act_unpack(J, C.R, H->selHost.data());
    if (n_left_out) *n_left_out = T->n;
    return LDSO_OK;
}

}  // extern "C"

// ---- the batch: activatePointsMT (FullSystem.cc:1052-1189) for every window of a ldso_ba_batch, one launch per kernel whatever the number of windows ----------------
namespace {

// what every batched activation entry refuses: for the batch as a whole (`solo`: the single-window entry the message points to), and for a window that takes part
// (`window`: the entry reads the resident window, for n_hosts frames)
int batch_act_checks(const ldso_ba_batch *Bt, const std::string &w, const char *solo) {
    REQ(Bt->FS == 8, w + ": windows of more than 8 key frames are not supported in a batched activation (every window needs F <= 8): run them with " + solo);
    return LDSO_OK;
}
int batch_act_window_checks(const ldso_ba *H, const std::string &w, bool window, int n_hosts) {
    REQ(H->D.pBegin == 0 && H->D.pEnd == H->D.P, w + ": not available on a sharded handle (ldso_ba_set_shard)");
    return window ? act_preconditions(H, w, n_hosts) : LDSO_OK;
}

// a participating window, its job and its share of the call's arenas; T: the tracer of a resident job, `compact`: its set is compacted by the decisions
struct SelPart { int win; ActJob J; ActRegions R; ldso_tracer *T = nullptr; bool compact = false; };

// The arenas of a batched call lie in the batch's staging pair (batch_stage): [the tables of act_batch_tables | every window's upload] go up, [every window's download |
// the counts of the compactions] come down, the scratch lies behind them on the device; a window's map lies in its own d_sel at offset 0, where ldso_ba_get_distance_map
// reads it.  jobOf(i, H, p, takes): window i's job into p (J, and T / compact of a resident one) with the entry's own refusals, takes = false: it sits out;
// done(p, nSelected): the window's results are unpacked, behind the wait (a compacted tracer has its new count).
template <class JobOf, class Done>
int batch_select_run(ldso_ba_batch *Bt, const char *who, const char *solo, bool haveJobs, const char *missing, float minTraceQuality, bool activate, int min_obs,
                     float min_idepth_hessian, int gn_iterations, JobOf jobOf, Done done) {
    const std::string w(who);
    REQ(Bt, w + ": null batch");
    REQ(haveJobs && gn_iterations >= 0, w + ": bad arguments (null jobs)");
    RUN(batch_act_checks(Bt, w, solo));
    ldso_ba *H0 = Bt->h[0];
    // ---- every refusal, before anything is enqueued or written; the regions of the arenas on the way ----
    std::vector<SelPart> part;
    ActBases at;
    size_t cands = 0;
    int nAct = 0, nCmp = 0;
    for (int i = 0; i < (int) Bt->h.size(); i++) {
        const ldso_ba *H = Bt->h[(size_t) i];
        SelPart p;
        bool takes = false;
        p.win = i;
        RUN(jobOf(i, H, p, takes));
        if (!takes) continue;
        RUN(act_job_check(p.J, w, missing));
        RUN(batch_act_window_checks(H, w, activate, p.J.nHosts));
        p.R = act_layout(p.J, at);
        p.compact = p.compact && p.J.n > 0;
        if (activate && p.J.n > 0) nAct++;
        if (p.compact) nCmp++;
        cands += (size_t) p.J.n;
        part.push_back(p);
    }
    REQ(cands < (size_t) 1 << 30, w + ": too many candidates");
    const int nPart = (int) part.size();
    if (nPart == 0) return LDSO_OK;
    CHK(hipSetDevice(H0->device));
    if (activate) RUN(batch_refresh(Bt));
    const ActBatchTables O = act_batch_tables((size_t) nPart, (size_t) nAct, (size_t) nCmp, sizeof(SelArgs), sizeof(ActWin), sizeof(CompactArgs));
    const size_t up = O.in + at.up, oCnt = at.down, down = oCnt + act_batch_counts((size_t) nCmp);
    RUN(batch_stage(Bt, up, down + at.scratch));
    char *hs = Bt->h_stage, *d = Bt->d_stage, *dOut = d + up;
    SelArgs *tab = (SelArgs *) (hs + O.sel);
    ActWin *act = (ActWin *) (hs + O.act);
    int32_t *wave = (int32_t *) (hs + O.wave);
    CompactArgs *cmp = (CompactArgs *) (hs + O.cmp);
    size_t ldsBytes = SEL_LIST_BYTES;
    int waves = 0, ia = 0, ic = 0;
    for (int k = 0; k < nPart; k++) {
        const SelPart &p = part[(size_t) k];
        ldso_ba *H = Bt->h[(size_t) p.win];
        act_pack(p.J, p.R, hs + O.in);
        RUN(sel_arena(H, p.R.mapBytes, p.R.mapBytes));
        SelArgs &A = tab[k];
        A = sel_args(p.J, p.R, d + O.in, dOut, dOut + down, (unsigned char *) H->d_sel, minTraceQuality);
        // the candidates where the tracer holds them, the seeds straight from the resident window: every point whose host is not the newest frame (as sel_run)
        if (p.J.resident) { A.pts = p.T->d_pts; A.myType = p.T->d_type; A.pgeo = H->B.pgeo; A.phost = H->B.phost; A.nWin = H->D.P; A.newestHost = p.J.nHosts - 1; }
        RUN(sel_lds_rule((const void *) k_act_select_batch, H0->device, Bt->selLdsLimit, Bt->selLdsSet, p.R.mapBytes, ldsBytes, A.ldsMap));
        if (activate && p.J.n > 0) {
            act[ia] = act_win(A.pts, (ldso_activation_t *) (dOut + p.R.act), p.J.n, min_obs, min_idepth_hessian, gn_iterations, A.selected, A.nSelected, p.win);
            wave[ia++] = waves; waves += p.J.n;
        }
        if (p.compact) { cmp[ic] = trace_compact_job(p.T, nullptr, A.decision, LDSO_ACT_KEEP, p.J.nHosts, nullptr, (int32_t *) (dOut + oCnt) + ic); ic++; }
    }
    wave[ia] = waves;
    const int cmpBlocks = nCmp ? group_prefix(nCmp, (int *) (hs + O.first), [&](int c) { return compact_blocks(cmp[c].n); }) : 0;
    CHK(hipMemcpyAsync(d, hs, up, hipMemcpyHostToDevice, H0->stream));
    hipLaunchKernelGGL(k_act_select_batch, dim3(nPart), dim3(SEL_THREADS), ldsBytes, H0->stream, (const SelArgs *) (d + O.sel));
    CHK(hipGetLastError());
    for (const SelPart &p : part) { ldso_ba *H = Bt->h[(size_t) p.win]; H->selW1 = p.J.w1; H->selH1 = p.J.h1; H->selMapOffset = 0; }
    if (activate) CHK(ba_launch_activate_batch(Bt->d_items, (const ActWin *) (d + O.act), (const int32_t *) (d + O.wave), nAct, waves, Bt->Dmax.nsg, H0->settings, H0->stream));
    if (cmpBlocks > 0) CHK(trace_launch_compact_group((const CompactArgs *) (d + O.cmp), (const int *) (d + O.first), nCmp, cmpBlocks, H0->stream));
    CHK(hipMemcpyAsync(hs + up, dOut, down, hipMemcpyDeviceToHost, H0->stream));
    CHK(hipStreamSynchronize(H0->stream));
    const int32_t *cnt = (const int32_t *) (hs + up + oCnt);
    ic = 0;
    for (const SelPart &p : part) {
        if (p.compact) trace_compact_finish_group(p.T, cnt[ic++]);
        done(p, act_unpack(p.J, p.R, hs + up));
    }
    return LDSO_OK;
}

// the explicit-array entries: jobs[i].n_hosts == 0: window i takes no part
int batch_select_arrays(ldso_ba_batch *Bt, const char *who, const char *solo, ldso_act_job_t *jobs, float minTraceQuality, bool activate, int min_obs, float min_idepth_hessian,
                        int gn_iterations) {
    return batch_select_run(Bt, who, solo, jobs != nullptr, ACT_MISSING_BATCH, minTraceQuality, activate, min_obs, min_idepth_hessian, gn_iterations,
        [&](int i, const ldso_ba *H, SelPart &p, bool &takes) -> int { takes = jobs[i].n_hosts != 0; if (takes) p.J = act_job(jobs[i], H->w, H->h, activate); return LDSO_OK; },
        [&](const SelPart &p, int ns) { jobs[p.win].n_selected = ns; });
}

}  // namespace

extern "C" {

// FullSystem::optimizeImmaturePoint (FullSystem.cc:892-1010) for the candidates of every window i of the batch with n[i] > 0 and points[i] != NULL: per window what
// ldso_ba_activate_points gives on its handle alone.  One upload (the window table, the wavefront offsets, all records), one launch (k_activate_batch), one
// download, one wait.
int ldso_ba_batch_activate_points(ldso_ba_batch_t *Bt, const int *n_pts, const ldso_immature_t *const *points, int min_obs, float min_idepth_hessian, int gn_iterations,
                                  ldso_activation_t *const *out) {
    const std::string w("ldso_ba_batch_activate_points");
    REQ(Bt, w + ": null batch");
    REQ(n_pts && points && out && gn_iterations >= 0, w + ": bad arguments (null array)");
    RUN(batch_act_checks(Bt, w, "ldso_ba_activate_points"));
    const int n = (int) Bt->h.size();
    ldso_ba *H0 = Bt->h[0];
    std::vector<int> part;
    size_t total = 0;
    for (int i = 0; i < n; i++) {
        if (n_pts[i] == 0 || points[i] == nullptr) continue;
        REQ(n_pts[i] > 0 && out[i], w + ": a window that takes part needs n[i] > 0 and its out[i]");
        RUN(batch_act_window_checks(Bt->h[(size_t) i], w, true, Bt->h[(size_t) i]->D.F));
        part.push_back(i);
        total += (size_t) n_pts[i];
    }
    const int nTab = (int) part.size();
    if (nTab == 0) return LDSO_OK;
    REQ(total < (size_t) 1 << 30, w + ": too many candidates");
    CHK(hipSetDevice(H0->device));
    RUN(batch_refresh(Bt));
    const size_t oWave = up16((size_t) nTab * sizeof(ActWin)), oPts = oWave + up16(((size_t) nTab + 1) * 4), up = oPts + total * sizeof(ldso_immature_t), down = total * sizeof(ldso_activation_t);
    RUN(batch_stage(Bt, up, down));
    char *hs = Bt->h_stage, *d = Bt->d_stage;
    ActWin *tab = (ActWin *) hs;
    int32_t *wave = (int32_t *) (hs + oWave);
    size_t at = 0;
    for (int k = 0; k < nTab; k++) {
        const int i = part[(size_t) k];
        memcpy(hs + oPts + at * sizeof(ldso_immature_t), points[i], (size_t) n_pts[i] * sizeof(ldso_immature_t));
        tab[k] = act_win((const ldso_immature_t *) (d + oPts) + at, (ldso_activation_t *) (d + up) + at, n_pts[i], min_obs, min_idepth_hessian, gn_iterations, nullptr, nullptr, i);
        wave[k] = (int32_t) at;
        at += (size_t) n_pts[i];
    }
    wave[nTab] = (int32_t) at;
    CHK(hipMemcpyAsync(d, hs, up, hipMemcpyHostToDevice, H0->stream));
    CHK(ba_launch_activate_batch(Bt->d_items, (const ActWin *) d, (const int32_t *) (d + oWave), nTab, (int) at, Bt->Dmax.nsg, H0->settings, H0->stream));
    CHK(hipMemcpyAsync(hs + up, d + up, down, hipMemcpyDeviceToHost, H0->stream));
    CHK(hipStreamSynchronize(H0->stream));
    at = 0;
    for (int k = 0; k < nTab; k++) {
        const int i = part[(size_t) k];
        memcpy(out[i], hs + up + at * sizeof(ldso_activation_t), (size_t) n_pts[i] * sizeof(ldso_activation_t));
        at += (size_t) n_pts[i];
    }
    return LDSO_OK;
}

// makeDistanceMap + the selection loop of FullSystem::activatePointsMT (FullSystem.cc:1080-1152, CoarseTracker.cc:686-818) for every window i of the batch with
// jobs[i].n_hosts != 0: per window what ldso_ba_select_candidates gives on its handle alone, its final map where ldso_ba_get_distance_map(handle_i) reads it.  One
// upload (the argument table and all inputs), one launch (k_act_select_batch: a workgroup per window), one download, one wait.
int ldso_ba_batch_select_candidates(ldso_ba_batch_t *Bt, ldso_act_job_t *jobs, float minTraceQuality) {
    return batch_select_arrays(Bt, "ldso_ba_batch_select_candidates", "ldso_ba_select_candidates", jobs, minTraceQuality, false, 0, 0.0f, 0);
}

// ... followed by the optimizeImmaturePoint loop (FullSystem.cc:1154-1164, 892-1010) on every window's selected list where the selection left it (k_activate_batch:
// the wavefronts beyond a window's count leave at once): per window what ldso_ba_select_activate_points gives.  Two launches, one wait.
int ldso_ba_batch_select_activate_points(ldso_ba_batch_t *Bt, ldso_act_job_t *jobs, float minTraceQuality, int min_obs, float min_idepth_hessian, int gn_iterations) {
    return batch_select_arrays(Bt, "ldso_ba_batch_select_activate_points", "ldso_ba_select_activate_points", jobs, minTraceQuality, true, min_obs, min_idepth_hessian, gn_iterations);
}

// The same with every window's immature set where it lives (ldso_ba_select_activate_tracer, per window): the candidates are the records and types of jobs[i].tracer,
// the seeds the points of the resident window i, and with jobs[i].compact != 0 whatever the loop did not KEEP leaves that tracer's set in the same enqueue
// (FullSystem.cc:1105-1188).  One upload (the tables of the three kernels and KRKi / Kt / flags), four launches (k_act_select_batch, k_activate_batch,
// k_compact_count_group, k_compact_move_group over the windows that compact: keep32 = the window's decisions), one download (decisions, lists, records and the
// compactions' counts), one wait, whatever the number of windows.  jobs[i].tracer == NULL: window i takes no part.
int ldso_ba_batch_select_activate_tracers(ldso_ba_batch_t *Bt, ldso_act_tracer_job_t *jobs, float minTraceQuality, int min_obs, float min_idepth_hessian, int gn_iterations) {
    const std::string w("ldso_ba_batch_select_activate_tracers");
    return batch_select_run(Bt, w.c_str(), "ldso_ba_select_activate_tracer", jobs != nullptr, ACT_MISSING_TRACERS, minTraceQuality, true, min_obs, min_idepth_hessian, gn_iterations,
        [&](int i, const ldso_ba *H, SelPart &p, bool &takes) -> int {
            const ldso_act_tracer_job_t &j = jobs[i];
            takes = j.tracer != nullptr;
            if (!takes) return LDSO_OK;
            REQ(j.tracer->device == H->device, w + ": window " + std::to_string(i) + ": the tracer and the batch live on different devices");
            for (int k = 0; k < i; k++) REQ(jobs[k].tracer != j.tracer, w + ": window " + std::to_string(i) + ": the same tracer in two jobs");
            p.J = act_job(0, nullptr, j.tracer->n, nullptr, nullptr, j.n_hosts, j.KRKi, j.Kt, j.host_flagged, j.currentMinActDist, H->w, H->h, true, j.decision_out, j.selected_out, j.out);
            p.J.resident = true; p.T = j.tracer; p.compact = j.compact != 0;
            return LDSO_OK;
        },
        [&](const SelPart &p, int ns) { jobs[p.win].n_selected = ns; jobs[p.win].n_left = p.T->n; });
}

// debug: CoarseDistanceMap::fwdWarpedIDDistFinal as the last selection left it, (w >> 1) * (h >> 1) floats, 0..39 and 1000
int ldso_ba_get_distance_map(ldso_ba_t *H, float *out) {
    REQ(H && out, "ldso_ba_get_distance_map: null argument");
    REQ(H->d_sel && H->selW1 > 0, "ldso_ba_get_distance_map: no selection has run on this handle");
    CHK(hipSetDevice(H->device));
    const size_t wh = (size_t) H->selW1 * H->selH1;
    std::vector<unsigned char> m(wh);
    CHK(hipMemcpyAsync(m.data(), (const char *) H->d_sel + H->selMapOffset, wh, hipMemcpyDeviceToHost, H->stream));
    CHK(hipStreamSynchronize(H->stream));
    for (size_t i = 0; i < wh; i++) out[i] = m[i] == SEL_FAR ? 1000.0f : (float) m[i];
    return LDSO_OK;
}

}  // extern "C"

