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
// For a batch of windows (ldso_ba_batch_select_candidates / _select_activate_points / _activate_points, at the end of the file) the same body runs as one workgroup per
// window in one launch, k_act_select_batch, each window with its own sizes and map placement.
#include <hip/hip_runtime.h>
#include "ba_host.h"

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
    SEL_GLOBAL(A.selected); SEL_GLOBAL(A.nSelected); SEL_GLOBAL(A.cell); SEL_GLOBAL(A.frac); SEL_GLOBAL(A.thr);
#undef SEL_GLOBAL
    if (A.ldsMap) act_select_body<true>(A, sel_lds);
    else act_select_body<false>(A, sel_lds);
}

struct SelBuffers {                // the carve-up of ldso_ba::d_sel for one call
    char *in = nullptr; size_t inBytes = 0;                       // [points | seeds | my_type | KRKi | Kt | flagged]: one upload
    char *out = nullptr; size_t outBytes = 0;                     // [n_selected (16 B) | decision | selected | activation records]: one download
    ldso_immature_t *pts = nullptr; ldso_act_seed_t *seeds = nullptr; float *myType = nullptr, *KRKi = nullptr, *Kt = nullptr; int32_t *flagged = nullptr;
    int32_t *nSelected = nullptr, *decision = nullptr, *selected = nullptr; ldso_activation_t *act = nullptr;
    int32_t *cell = nullptr; float *frac = nullptr, *thr = nullptr; unsigned char *gmap = nullptr;
};

static size_t up16(size_t x) { return (x + 15) / 16 * 16; }

}  // namespace

// Where a selection takes its candidates and seeds from: flat host arrays (uploaded with the poses), or device memory - the records and types of a tracer's
// resident set and the points of the handle's resident window - of which nothing is uploaded.
struct SelSource {
    int nSeeds = 0; const ldso_act_seed_t *seeds = nullptr;                          // host
    int n = 0; const ldso_immature_t *points = nullptr; const float *myType = nullptr;      // host
    const ldso_immature_t *d_points = nullptr; const float *d_myType = nullptr;      // device (then points / myType / seeds are null)
    bool windowSeeds = false;
    int newestHost = -1;
};

static int sel_enqueue(ldso_ba *H, const char *who, const SelSource &I, int n_hosts, const float *KRKi, const float *Kt, const int32_t *host_flagged, float currentMinActDist,
                       float minTraceQuality, SelBuffers &S) {
    const int n = I.n, n_seeds = I.nSeeds;
    const bool onDevice = I.d_points != nullptr || I.windowSeeds;
    REQ(H && n_seeds >= 0 && n >= 0 && n_hosts >= 1 && n_hosts <= LDSO_MAX_FRAMES && KRKi && Kt && host_flagged && (n_seeds == 0 || I.seeds)
        && (n == 0 || (I.points && I.myType) || (I.d_points && I.d_myType)), std::string(who) + ": bad arguments");
    const int w1 = H->w >> 1, h1 = H->h >> 1;
    REQ(w1 >= 3 && h1 >= 3 && w1 < 65536 && h1 < 65536, std::string(who) + ": image size out of range");
    // device data cannot be range-checked here: the kernel drops a candidate and skips a seed whose host is not a frame of the window
    for (int i = 0; !onDevice && i < n; i++) REQ(I.points[i].host >= 0 && I.points[i].host < n_hosts, std::string(who) + ": a candidate's host is not a frame of the window");
    for (int i = 0; i < n_seeds; i++) REQ(I.seeds[i].host >= 0 && I.seeds[i].host < n_hosts, std::string(who) + ": a seed's host is not a frame of the window");
    CHK(hipSetDevice(H->device));
    const size_t wh = (size_t) w1 * h1, nn = (size_t) n, nUp = I.points ? nn : 0;
    const size_t oPts = 0, oSeeds = oPts + nUp * sizeof(ldso_immature_t), oType = oSeeds + up16((size_t) n_seeds * sizeof(ldso_act_seed_t)), oKRKi = oType + up16(nUp * 4),
                 oKt = oKRKi + up16((size_t) n_hosts * 36), oFlag = oKt + up16((size_t) n_hosts * 12), inBytes = oFlag + up16((size_t) n_hosts * 4);
    const size_t oDec = 16, oSel = oDec + up16(nn * 4), oAct = oSel + up16(nn * 4), outBytes = oAct + nn * sizeof(ldso_activation_t);
    const size_t oCell = inBytes + outBytes, oFrac = oCell + up16(nn * 4), oThr = oFrac + up16(nn * 4), oMap = oThr + up16(nn * 4), total = oMap + up16(wh);
    if (total > H->selCap) {
        if (H->d_sel) hipFree(H->d_sel);
        H->d_sel = nullptr; H->selCap = 0;
        CHK(hipMalloc(&H->d_sel, total + total / 2));
        H->selCap = total + total / 2;
    }
    char *d = (char *) H->d_sel;
    S.in = d; S.inBytes = inBytes; S.out = d + inBytes; S.outBytes = outBytes;
    S.pts = (ldso_immature_t *) (d + oPts); S.seeds = (ldso_act_seed_t *) (d + oSeeds); S.myType = (float *) (d + oType); S.KRKi = (float *) (d + oKRKi); S.Kt = (float *) (d + oKt);
    S.flagged = (int32_t *) (d + oFlag);
    S.nSelected = (int32_t *) S.out; S.decision = (int32_t *) (S.out + oDec); S.selected = (int32_t *) (S.out + oSel); S.act = (ldso_activation_t *) (S.out + oAct);
    S.cell = (int32_t *) (d + oCell); S.frac = (float *) (d + oFrac); S.thr = (float *) (d + oThr); S.gmap = (unsigned char *) (d + oMap);
    H->selHost.resize(std::max(inBytes, outBytes));
    char *hs = H->selHost.data();
    memset(hs, 0, inBytes);
    if (nUp) { memcpy(hs + oPts, I.points, nn * sizeof(ldso_immature_t)); memcpy(hs + oType, I.myType, nn * 4); }
    if (n_seeds) memcpy(hs + oSeeds, I.seeds, (size_t) n_seeds * sizeof(ldso_act_seed_t));
    memcpy(hs + oKRKi, KRKi, (size_t) n_hosts * 36); memcpy(hs + oKt, Kt, (size_t) n_hosts * 12); memcpy(hs + oFlag, host_flagged, (size_t) n_hosts * 4);
    CHK(hipMemcpyAsync(S.in, hs, inBytes, hipMemcpyHostToDevice, H->stream));
    SelArgs A;
    A.seeds = S.seeds; A.pts = I.d_points ? I.d_points : S.pts; A.myType = I.d_points ? I.d_myType : S.myType; A.KRKi = S.KRKi; A.Kt = S.Kt; A.flagged = S.flagged;
    A.nSeeds = n_seeds; A.n = n; A.nHosts = n_hosts; A.w1 = w1; A.h1 = h1; A.minDist = currentMinActDist; A.minQuality = minTraceQuality;
    A.pgeo = I.windowSeeds ? H->B.pgeo : nullptr; A.phost = I.windowSeeds ? H->B.phost : nullptr; A.nWin = I.windowSeeds ? H->D.P : 0; A.newestHost = I.newestHost;
    A.gmap = S.gmap; A.ldsMap = 0; A.decision = S.decision; A.selected = S.selected; A.nSelected = S.nSelected; A.cell = S.cell; A.frac = S.frac; A.thr = S.thr;
    // the map in LDS where the workgroup can have that much (beside the kernel's own static bytes), in global memory otherwise
    const size_t ldsBytes = SEL_LIST_BYTES + up16(wh);
    if (H->selLdsLimit < 0) {
        hipFuncAttributes fa; int perBlock = 0;
        CHK(hipFuncGetAttributes(&fa, (const void *) k_act_select<true>));
        CHK(hipDeviceGetAttribute(&perBlock, hipDeviceAttributeMaxSharedMemoryPerBlock, H->device));
        H->selLdsLimit = std::max(0, std::min(perBlock, SEL_LDS_MAX) - (int) fa.sharedSizeBytes);
    }
    if (ldsBytes <= (size_t) H->selLdsLimit) {
        if ((int) ldsBytes > H->selLdsSet) { CHK(hipFuncSetAttribute((const void *) k_act_select<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) ldsBytes)); H->selLdsSet = (int) ldsBytes; }
        hipLaunchKernelGGL(k_act_select<true>, dim3(1), dim3(SEL_THREADS), ldsBytes, H->stream, A);
    } else hipLaunchKernelGGL(k_act_select<false>, dim3(1), dim3(SEL_THREADS), SEL_LIST_BYTES, H->stream, A);
    CHK(hipGetLastError());
    H->selW1 = w1; H->selH1 = h1; H->selMapOffset = oMap;
    return LDSO_OK;
}

static SelSource host_source(int n_seeds, const ldso_act_seed_t *seeds, int n, const ldso_immature_t *points, const float *my_type) {
    SelSource I;
    I.nSeeds = n_seeds; I.seeds = seeds; I.n = n; I.points = points; I.myType = my_type;
    return I;
}

// the preconditions of point activation on the resident window (ldso_ba_activate_points)
static int act_preconditions(const ldso_ba *H, const char *who, int n_hosts) {
    REQ(H->D.F >= 2, std::string(who) + ": set the window and the frames first");
    REQ(n_hosts == H->D.F, std::string(who) + ": one KRKi / Kt / flag per frame of the resident window");
    for (int f = 0; f < H->D.F; f++) REQ(H->B.img[f] != nullptr, std::string(who) + ": a key-frame image is missing");
    return LDSO_OK;
}

// selection, then k_activate on the selected list where the selection kernel left it; the results come down with the caller's one synchronisation
static int sel_activate_enqueue(ldso_ba *H, const char *who, const SelSource &I, int n_hosts, const float *KRKi, const float *Kt, const int32_t *host_flagged, float currentMinActDist,
                                float minTraceQuality, int min_obs, float min_idepth_hessian, int gn_iterations, SelBuffers &S) {
    RUN(sel_enqueue(H, who, I, n_hosts, KRKi, Kt, host_flagged, currentMinActDist, minTraceQuality, S));
    CHK(ba_launch_activate_selected(H->B, H->D, H->settings, I.d_points ? I.d_points : S.pts, S.selected, S.nSelected, S.act, I.n, min_obs, min_idepth_hessian, gn_iterations, H->stream));
    CHK(hipMemcpyAsync(H->selHost.data(), S.out, S.outBytes, hipMemcpyDeviceToHost, H->stream));
    return LDSO_OK;
}

static void sel_unpack_activations(const ldso_ba *H, int n, int n_selected, ldso_activation_t *out) {
    const size_t oAct = 16 + 2 * up16((size_t) n * 4);
    if (n_selected > 0) memcpy(out, H->selHost.data() + oAct, (size_t) n_selected * sizeof(ldso_activation_t));
}

static void sel_unpack(const ldso_ba *H, int n, int32_t *decision_out, int32_t *selected_out, int *n_selected_out) {
    const char *hs = H->selHost.data();
    const int ns = *(const int32_t *) hs;
    const size_t oDec = 16, oSel = oDec + up16((size_t) n * 4);
    if (n) memcpy(decision_out, hs + oDec, (size_t) n * 4);
    if (selected_out && ns > 0) memcpy(selected_out, hs + oSel, (size_t) ns * 4);
    if (n_selected_out) *n_selected_out = ns;
}

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

// makeDistanceMap + the selection loop of FullSystem::activatePointsMT (FullSystem.cc:1080-1152, CoarseTracker.cc:686-818)
int ldso_ba_select_candidates(ldso_ba_t *H, int n_seeds, const ldso_act_seed_t *seeds, int n, const ldso_immature_t *points, const float *my_type, int n_hosts, const float *KRKi,
                              const float *Kt, const int32_t *host_flagged, float currentMinActDist, float minTraceQuality, int32_t *decision_out, int32_t *selected_out,
                              int *n_selected_out) {
    REQ(H && (n <= 0 || decision_out), "ldso_ba_select_candidates: bad arguments");
    SelBuffers S;
    RUN(sel_enqueue(H, "ldso_ba_select_candidates", host_source(n_seeds, seeds, n, points, my_type), n_hosts, KRKi, Kt, host_flagged, currentMinActDist, minTraceQuality, S));
    const size_t bytes = 16 + 2 * up16((size_t) n * 4);
    CHK(hipMemcpyAsync(H->selHost.data(), S.out, bytes, hipMemcpyDeviceToHost, H->stream));
    CHK(hipStreamSynchronize(H->stream));
    sel_unpack(H, n, decision_out, selected_out, n_selected_out);
    return LDSO_OK;
}

// ... followed by the optimizeImmaturePoint loop (FullSystem.cc:1154-1164, 892-1010) on the selected list, which never leaves the device: k_activate reads the
// list and its length where the selection kernel left them.  One synchronisation.  out[k] belongs to candidate selected_out[k], k < *n_selected_out.
int ldso_ba_select_activate_points(ldso_ba_t *H, int n_seeds, const ldso_act_seed_t *seeds, int n, const ldso_immature_t *points, const float *my_type, int n_hosts,
                                   const float *KRKi, const float *Kt, const int32_t *host_flagged, float currentMinActDist, float minTraceQuality, int min_obs,
                                   float min_idepth_hessian, int gn_iterations, int32_t *decision_out, int32_t *selected_out, int *n_selected_out, ldso_activation_t *out) {
    REQ(H && gn_iterations >= 0 && n_selected_out && (n <= 0 || (decision_out && selected_out && out)), "ldso_ba_select_activate_points: bad arguments");
    RUN(act_preconditions(H, "ldso_ba_select_activate_points", n_hosts));
    SelBuffers S;
    RUN(sel_activate_enqueue(H, "ldso_ba_select_activate_points", host_source(n_seeds, seeds, n, points, my_type), n_hosts, KRKi, Kt, host_flagged, currentMinActDist, minTraceQuality,
                             min_obs, min_idepth_hessian, gn_iterations, S));
    CHK(hipStreamSynchronize(H->stream));
    sel_unpack(H, n, decision_out, selected_out, n_selected_out);
    sel_unpack_activations(H, n, *n_selected_out, out);
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
    SelSource I;
    I.n = n; I.d_points = T->d_pts; I.d_myType = T->d_type; I.windowSeeds = true; I.newestHost = n_hosts - 1;
    SelBuffers S;
    RUN(sel_activate_enqueue(H, "ldso_ba_select_activate_tracer", I, n_hosts, KRKi, Kt, host_flagged, currentMinActDist, minTraceQuality, min_obs, min_idepth_hessian,
                             gn_iterations, S));
    const int rcCompact = compact ? trace_compact_enqueue(T, nullptr, S.decision, LDSO_ACT_KEEP, n_hosts, false, H->stream) : LDSO_OK;
    CHK(hipStreamSynchronize(H->stream));          // also where the compaction could not be enqueued: the copy into selHost is in flight
    if (rcCompact != LDSO_OK) return rcCompact;
    if (compact) trace_compact_finish(T);
    sel_unpack(H, n, decision_out, selected_out, n_selected_out);
    sel_unpack_activations(H, n, *n_selected_out, out);
    if (n_left_out) *n_left_out = T->n;
    return LDSO_OK;
}

}  // extern "C"

// ---- the batch: activatePointsMT (FullSystem.cc:1052-1189) for every window of a ldso_ba_batch, one launch per kernel whatever the number of windows ----------------
namespace {

struct SelPlan {                   // a participating window's share of the call's arena; offsets in bytes into the upload, the download and the scratch region
    int win = 0, w1 = 0, h1 = 0;
    size_t oPts = 0, oSeeds = 0, oType = 0, oKRKi = 0, oKt = 0, oFlag = 0, oOut = 0, oDec = 0, oSel = 0, oAct = 0, oCell = 0, oFrac = 0, oThr = 0, mapBytes = 0;
};

// what every batched activation entry refuses: for the batch as a whole, and for a window that takes part (`images`: the entry reads the resident window); `solo`: the
// single-window entry the message points to
int batch_act_checks(const ldso_ba_batch *Bt, const std::string &w, const char *solo) {
    REQ(Bt->FS == 8, w + ": windows of more than 8 key frames are not supported in a batched activation (every window needs F <= 8): run them with " + solo);
    return LDSO_OK;
}
int batch_act_window_checks(const ldso_ba *H, const std::string &w, bool images) {
    REQ(H->D.pBegin == 0 && H->D.pEnd == H->D.P, w + ": not available on a sharded handle (ldso_ba_set_shard)");
    if (images) {
        REQ(H->D.F >= 2, w + ": set the window and the frames first");
        for (int f = 0; f < H->D.F; f++) REQ(H->B.img[f] != nullptr, w + ": a key-frame image is missing");
    }
    return LDSO_OK;
}

// the map of window H for a batched selection: in the handle's own arena, where ldso_ba_get_distance_map looks for it
int batch_sel_map(ldso_ba *H, size_t mapBytes, unsigned char **gmap) {
    if (mapBytes > H->selCap) {
        if (H->d_sel) hipFree(H->d_sel);
        H->d_sel = nullptr; H->selCap = 0; H->selW1 = 0; H->selH1 = 0;
        CHK(hipMalloc(&H->d_sel, mapBytes));
        H->selCap = mapBytes;
    }
    *gmap = (unsigned char *) H->d_sel;
    return LDSO_OK;
}

int batch_select_run(ldso_ba_batch *Bt, const char *who, const char *solo, ldso_act_job_t *jobs, float minTraceQuality, bool activate, int min_obs, float min_idepth_hessian,
                     int gn_iterations) {
    const std::string w(who);
    REQ(Bt, w + ": null batch");
    REQ(jobs && gn_iterations >= 0, w + ": bad arguments (null jobs)");
    RUN(batch_act_checks(Bt, w, solo));
    const int n = (int) Bt->h.size();
    ldso_ba *H0 = Bt->h[0];
    // ---- every refusal, before anything is enqueued or written; the regions of the arena on the way ----
    std::vector<SelPlan> plan;
    size_t in = 0, down = 0, scratch = 0, cands = 0;
    int nAct = 0;
    for (int i = 0; i < n; i++) {
        const ldso_act_job_t &J = jobs[i];
        if (J.n_hosts == 0) continue;
        const ldso_ba *H = Bt->h[i];
        REQ(J.n_seeds >= 0 && J.n >= 0 && J.n_hosts >= 1 && J.n_hosts <= LDSO_MAX_FRAMES && J.KRKi && J.Kt && J.host_flagged && (J.n_seeds == 0 || J.seeds)
            && (J.n == 0 || (J.points && J.my_type && J.decision_out)) && (!activate || J.n == 0 || (J.selected_out && J.out)),
            w + ": a window that takes part needs its arrays (seeds, points, my_type, KRKi, Kt, host_flagged and the outputs)");
        RUN(batch_act_window_checks(H, w, false));
        if (activate) RUN(act_preconditions(H, who, J.n_hosts));
        SelPlan p;
        p.win = i; p.w1 = H->w >> 1; p.h1 = H->h >> 1;
        REQ(p.w1 >= 3 && p.h1 >= 3 && p.w1 < 65536 && p.h1 < 65536, w + ": image size out of range");
        for (int k = 0; k < J.n; k++) REQ(J.points[k].host >= 0 && J.points[k].host < J.n_hosts, w + ": a candidate's host is not a frame of the window");
        for (int k = 0; k < J.n_seeds; k++) REQ(J.seeds[k].host >= 0 && J.seeds[k].host < J.n_hosts, w + ": a seed's host is not a frame of the window");
        const size_t nn = (size_t) J.n;
        p.oPts = in; p.oSeeds = p.oPts + nn * sizeof(ldso_immature_t); p.oType = p.oSeeds + up16((size_t) J.n_seeds * sizeof(ldso_act_seed_t)); p.oKRKi = p.oType + up16(nn * 4);
        p.oKt = p.oKRKi + up16((size_t) J.n_hosts * 36); p.oFlag = p.oKt + up16((size_t) J.n_hosts * 12); in = p.oFlag + up16((size_t) J.n_hosts * 4);
        p.oOut = down; p.oDec = p.oOut + 16; p.oSel = p.oDec + up16(nn * 4); p.oAct = p.oSel + up16(nn * 4); down = p.oAct + (activate ? nn * sizeof(ldso_activation_t) : 0);
        p.oCell = scratch; p.oFrac = p.oCell + up16(nn * 4); p.oThr = p.oFrac + up16(nn * 4); scratch = p.oThr + up16(nn * 4);
        p.mapBytes = up16((size_t) p.w1 * p.h1);
        if (activate && J.n > 0) nAct++;
        cands += nn;
        plan.push_back(p);
    }
    REQ(cands < (size_t) 1 << 30, w + ": too many candidates");
    const int nPart = (int) plan.size();
    if (nPart == 0) return LDSO_OK;
    CHK(hipSetDevice(H0->device));
    if (activate) RUN(batch_refresh(Bt));
    // the upload: [nPart SelArgs | nAct ActWin | nAct + 1 wavefront offsets | every window's inputs]
    const size_t oTab = 0, oAct = oTab + up16((size_t) nPart * sizeof(SelArgs)), oWave = oAct + up16((size_t) nAct * sizeof(ActWin)), oIn = oWave + up16(((size_t) nAct + 1) * 4), up = oIn + in;
    RUN(batch_stage(Bt, up, down + scratch));
    if (Bt->selLdsLimit < 0) {
        hipFuncAttributes fa; int perBlock = 0;
        CHK(hipFuncGetAttributes(&fa, (const void *) k_act_select_batch));
        CHK(hipDeviceGetAttribute(&perBlock, hipDeviceAttributeMaxSharedMemoryPerBlock, H0->device));
        Bt->selLdsLimit = std::max(0, std::min(perBlock, SEL_LDS_MAX) - (int) fa.sharedSizeBytes);
    }
    char *hs = Bt->h_stage, *d = Bt->d_stage, *dIn = d + oIn, *dOut = d + up, *dScr = d + up + down;
    SelArgs *tab = (SelArgs *) (hs + oTab);
    ActWin *act = (ActWin *) (hs + oAct);
    int32_t *wave = (int32_t *) (hs + oWave);
    size_t ldsBytes = SEL_LIST_BYTES;
    int waves = 0, ia = 0;
    for (int k = 0; k < nPart; k++) {
        const SelPlan &p = plan[(size_t) k];
        const ldso_act_job_t &J = jobs[p.win];
        ldso_ba *H = Bt->h[(size_t) p.win];
        const size_t nn = (size_t) J.n;
        char *hi = hs + oIn;
        if (J.n) { memcpy(hi + p.oPts, J.points, nn * sizeof(ldso_immature_t)); memcpy(hi + p.oType, J.my_type, nn * 4); }
        if (J.n_seeds) memcpy(hi + p.oSeeds, J.seeds, (size_t) J.n_seeds * sizeof(ldso_act_seed_t));
        memcpy(hi + p.oKRKi, J.KRKi, (size_t) J.n_hosts * 36); memcpy(hi + p.oKt, J.Kt, (size_t) J.n_hosts * 12); memcpy(hi + p.oFlag, J.host_flagged, (size_t) J.n_hosts * 4);
        SelArgs &A = tab[k];
        memset(&A, 0, sizeof(A));
        A.seeds = (const ldso_act_seed_t *) (dIn + p.oSeeds); A.pts = (const ldso_immature_t *) (dIn + p.oPts); A.myType = (const float *) (dIn + p.oType);
        A.KRKi = (const float *) (dIn + p.oKRKi); A.Kt = (const float *) (dIn + p.oKt); A.flagged = (const int32_t *) (dIn + p.oFlag);
        A.nSeeds = J.n_seeds; A.n = J.n; A.nHosts = J.n_hosts; A.w1 = p.w1; A.h1 = p.h1; A.minDist = J.currentMinActDist; A.minQuality = minTraceQuality;
        A.pgeo = nullptr; A.phost = nullptr; A.nWin = 0; A.newestHost = -1;
        RUN(batch_sel_map(H, p.mapBytes, &A.gmap));
        // the map in LDS where the workgroup can have that much, in global memory otherwise: the rule of the single-window entry, window by window
        A.ldsMap = SEL_LIST_BYTES + p.mapBytes <= (size_t) Bt->selLdsLimit ? 1 : 0;
        if (A.ldsMap) ldsBytes = std::max(ldsBytes, SEL_LIST_BYTES + p.mapBytes);
        A.nSelected = (int32_t *) (dOut + p.oOut); A.decision = (int32_t *) (dOut + p.oDec); A.selected = (int32_t *) (dOut + p.oSel);
        A.cell = (int32_t *) (dScr + p.oCell); A.frac = (float *) (dScr + p.oFrac); A.thr = (float *) (dScr + p.oThr);
        if (activate && J.n > 0) {
            ActWin &T = act[ia];
            memset(&T, 0, sizeof(T));
            T.A.pts = A.pts; T.A.out = (ldso_activation_t *) (dOut + p.oAct); T.A.n = J.n; T.A.minObs = min_obs; T.A.GNIts = gn_iterations; T.A.minIdepthH_act = min_idepth_hessian;
            T.A.sel = A.selected; T.A.nSel = A.nSelected; T.item = p.win;
            wave[ia++] = waves; waves += J.n;
        }
    }
    wave[ia] = waves;
    CHK(hipMemcpyAsync(d, hs, up, hipMemcpyHostToDevice, H0->stream));
    if ((int) ldsBytes > Bt->selLdsSet) { CHK(hipFuncSetAttribute((const void *) k_act_select_batch, hipFuncAttributeMaxDynamicSharedMemorySize, (int) ldsBytes)); Bt->selLdsSet = (int) ldsBytes; }
    hipLaunchKernelGGL(k_act_select_batch, dim3(nPart), dim3(SEL_THREADS), ldsBytes, H0->stream, (const SelArgs *) (d + oTab));
    CHK(hipGetLastError());
    for (const SelPlan &p : plan) { ldso_ba *H = Bt->h[(size_t) p.win]; H->selW1 = p.w1; H->selH1 = p.h1; H->selMapOffset = 0; }
    if (activate) CHK(ba_launch_activate_batch(Bt->d_items, (const ActWin *) (d + oAct), (const int32_t *) (d + oWave), nAct, waves, Bt->Dmax.nsg, H0->settings, H0->stream));
    CHK(hipMemcpyAsync(hs + up, dOut, down, hipMemcpyDeviceToHost, H0->stream));
    CHK(hipStreamSynchronize(H0->stream));
    for (const SelPlan &p : plan) {
        ldso_act_job_t &J = jobs[p.win];
        const char *ho = hs + up;
        const int ns = std::min(std::max(*(const int32_t *) (ho + p.oOut), 0), J.n);
        if (J.n) memcpy(J.decision_out, ho + p.oDec, (size_t) J.n * 4);
        if (J.selected_out && ns > 0) memcpy(J.selected_out, ho + p.oSel, (size_t) ns * 4);
        if (activate && ns > 0) memcpy(J.out, ho + p.oAct, (size_t) ns * sizeof(ldso_activation_t));
        J.n_selected = ns;
    }
    return LDSO_OK;
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
        RUN(batch_act_window_checks(Bt->h[(size_t) i], w, true));
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
        ActWin &T = tab[k];
        memset(&T, 0, sizeof(T));
        memcpy(hs + oPts + at * sizeof(ldso_immature_t), points[i], (size_t) n_pts[i] * sizeof(ldso_immature_t));
        T.A.pts = (const ldso_immature_t *) (d + oPts) + at; T.A.out = (ldso_activation_t *) (d + up) + at; T.A.n = n_pts[i]; T.A.minObs = min_obs; T.A.GNIts = gn_iterations;
        T.A.minIdepthH_act = min_idepth_hessian; T.A.sel = nullptr; T.A.nSel = nullptr; T.item = i;
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
    return batch_select_run(Bt, "ldso_ba_batch_select_candidates", "ldso_ba_select_candidates", jobs, minTraceQuality, false, 0, 0.0f, 0);
}

// ... followed by the optimizeImmaturePoint loop (FullSystem.cc:1154-1164, 892-1010) on every window's selected list where the selection left it (k_activate_batch:
// the wavefronts beyond a window's count leave at once): per window what ldso_ba_select_activate_points gives.  Two launches, one wait.
int ldso_ba_batch_select_activate_points(ldso_ba_batch_t *Bt, ldso_act_job_t *jobs, float minTraceQuality, int min_obs, float min_idepth_hessian, int gn_iterations) {
    return batch_select_run(Bt, "ldso_ba_batch_select_activate_points", "ldso_ba_select_activate_points", jobs, minTraceQuality, true, min_obs, min_idepth_hessian, gn_iterations);
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
