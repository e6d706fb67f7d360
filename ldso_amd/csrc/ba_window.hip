// ba_window.hip — the window of a handle: upload through the staging arena (ldso_ba_set_window), the delta against the resident window
// (ldso_ba_update_window and the edit API that records one), the flattening into chunks; the same delta, and the frames / prior behind it, for every window of a batch
// (ldso_ba_batch_update_windows, ldso_ba_batch_set_frames).
#include "ba_host.h"

// One entry of the upload table at the head of the staging arena: copy `words` 32-bit words from arena offset `src` (bytes) to `dst`,
// or fill `dst` with zeros (src == LD_XFER_ZERO).
struct WinXfer { void *dst; unsigned long long src; unsigned long long words; };
#define LD_XFER_ZERO 0xFFFFFFFFFFFFFFFFull
#define LD_XFER_MAX 96
__global__ __launch_bounds__(256) void k_win_scatter(const char *__restrict__ arena, int nEntries) {
    const WinXfer *tab = reinterpret_cast<const WinXfer *>(arena);
    for (int e = 0; e < nEntries; e++) {
        const WinXfer x = tab[e];
        unsigned *dst = static_cast<unsigned *>(x.dst);
        const size_t n = (size_t) x.words, stride = (size_t) gridDim.x * blockDim.x;
        if (x.src == LD_XFER_ZERO) { for (size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) dst[i] = 0u; }
        else {
            const unsigned *src = reinterpret_cast<const unsigned *>(arena + x.src);
            for (size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) dst[i] = src[i];
        }
    }
}
// The scatter of a whole batch of windows (ldso_ba_batch_update_windows / _set_frames): ONE table over all windows.  With 32 x ~25 entries a workgroup that walked every
// entry (k_win_scatter) would spend its life in the loop head, so the WORDS are dealt out instead: a work unit is LD_XFER_UNIT consecutive words of one entry, unit0[e]
// the first unit of entry e (unit0[nEntries] = the grid), and a workgroup finds its entry by bisection (uniform: scalar loads).  16-byte accesses where both sides allow.
#define LD_XFER_UNIT 4096
__global__ __launch_bounds__(256) void k_win_scatter_batch(const char *__restrict__ arena, const WinXfer *__restrict__ tab, const int32_t *__restrict__ unit0, int nEntries) {
    const int u = blockIdx.x;
    int lo = 0, hi = nEntries - 1;          // the last entry whose first unit is <= u
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (unit0[mid] <= u) lo = mid; else hi = mid - 1; }
    const WinXfer x = tab[lo];
    const size_t w0 = (size_t) (u - unit0[lo]) * LD_XFER_UNIT;
    if (w0 >= (size_t) x.words) return;
    const size_t left = (size_t) x.words - w0, n = left < (size_t) LD_XFER_UNIT ? left : (size_t) LD_XFER_UNIT;
    unsigned *dst = static_cast<unsigned *>(x.dst) + w0;
    const bool zero = x.src == LD_XFER_ZERO;
    const unsigned *src = zero ? nullptr : reinterpret_cast<const unsigned *>(arena + x.src) + w0;
    const bool wide = ((reinterpret_cast<size_t>(dst) | (zero ? (size_t) 0 : reinterpret_cast<size_t>(src))) & 15) == 0;
    const size_t n4 = wide ? n / 4 : 0;
    for (size_t i = threadIdx.x; i < n4; i += blockDim.x) reinterpret_cast<uint4 *>(dst)[i] = zero ? make_uint4(0u, 0u, 0u, 0u) : reinterpret_cast<const uint4 *>(src)[i];
    for (size_t i = n4 * 4 + threadIdx.x; i < n; i += blockDim.x) dst[i] = zero ? 0u : src[i];
}
static __device__ __forceinline__ void point_stats_one(PtRec *__restrict__ a, PtRec *__restrict__ b, const float *__restrict__ mrb, const int32_t *__restrict__ ngr, const int i) {
    const float m = mrb[i]; const int32_t g = ngr[i];
    a[i].maxRelBS = m; a[i].numGood = g; b[i].maxRelBS = m; b[i].numGood = g;
}
__global__ __launch_bounds__(256) void k_point_stats(PtRec *__restrict__ a, PtRec *__restrict__ b, const float *__restrict__ mrb, const int32_t *__restrict__ ngr, int P) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    point_stats_one(a, b, mrb, ngr, i);
}
// ---------------------------------------------------------------------------------------------------------------------------------------------------
// ldso_ba_update_window: the staging image a full ldso_ba_set_window of the SAME window would have uploaded, built ON THE DEVICE from the resident window
// (the applied set) and a small delta - which frames stay (EnergyFunctional::marginalizeFrame / insertFrame), which points stay and in which order (removePoint,
// dropPointsF, makeIDX), which residuals a point has (insertResidual / dropResidual as one bit per target frame) and the records of the fresh points.  One thread
// per (point, slot).  What is carried over is exactly what the host objects carry between two optimize() calls: u, v, priorF, colour / weights, the inverse depth,
// maxRelBaseline / numGoodResiduals, and per residual state_state, state_energy, isActive, isNew - everything else starts as ldso_ba_set_window starts it, so
// that the resident window and a fresh upload of the same objects are the same bytes (tests/test_resident_gpu.py).
// ---------------------------------------------------------------------------------------------------------------------------------------------------
struct WinDelta {
    // the resident window (read)
    const PtGeo *oGeo; const PtCw *oPcw; const int32_t *oHost; const SlotTab *oTab; const SlotRec *oSlot; const PtRec *oPt;
    int oF, oFS, oP;
    // the delta (device copies inside the staging arena)
    const int32_t *frameFrom;      // [F]  old index of new frame f, -1 = inserted
    const int32_t *pointFrom;      // [P]  old row of new point i, -1 - k = the k-th fresh point
    const uint32_t *resMask;       // [P]  bit t: the point has a residual whose target is frame t
    const int32_t *resBegin;       // [P + 1] flat index of the point's first residual (flat order: point-major, target-ascending)
    const ldso_point_t *fresh; const ldso_residual_t *freshRes; const int32_t *freshResBegin;      // the fresh points, their residuals (target-ascending), first residual of fresh point k
    const float *freshMrb; const int32_t *freshNgr;
    int F, FS, P;
    // the image (written)
    PtGeo *geo; PtCw *pcw; int32_t *phost; SlotTab *tab; SlotRec *sr; float *mrb; int32_t *ngr;
    // the PtRecs of both sets that take mrb / ngr once the scatter has zeroed them (k_point_stats_batch)
    PtRec *pt0, *pt1;
};
static __device__ __forceinline__ void win_rebuild_pair(const WinDelta &W, const int q) {          // one (point, slot) pair of the image: the body of both kernels below
    const int row = q / W.FS, col = q - row * W.FS;
    const int from = W.pointFrom[row];
    const uint32_t mask = W.resMask[row];
    SlotTab t{-1, 0, 0, -1};
    SlotRec r;
#pragma unroll
    for (int k = 0; k < 8; k++) { r.e[k].jp = 0.0f; r.e[k].m.i = 0; }
    r.e[LD_SM_STATE].m.i = LDSO_RES_OOB;
    if (col < W.F && ((mask >> col) & 1u)) {
        const int below = __popc(mask & ((1u << col) - 1u));
        t.rflat = W.resBegin[row] + below;
        const int oc = (from >= 0) ? W.frameFrom[col] : -1;
        if (from >= 0) {
            const size_t os = (size_t) from * W.oFS + (oc >= 0 ? oc : 0);
            if (oc >= 0 && W.oTab[os].rflat >= 0) {          // the residual was there: its state lives on
                const SlotRec o = W.oSlot[os];
                t.rnew = W.oTab[os].rnew;
                r.e[LD_SM_STATE].m.i = o.e[LD_SM_STATE].m.i; r.e[LD_SM_ACTIVE].m.i = o.e[LD_SM_ACTIVE].m.i; r.e[LD_SM_ENERGY].m.f = o.e[LD_SM_ENERGY].m.f;
            } else {                                          // insertResidual for a point of the window (FullSystem.cc:447-470: state IN, energy 0, not active yet)
                t.rnew = 1;
                r.e[LD_SM_STATE].m.i = LDSO_RES_IN; r.e[LD_SM_ACTIVE].m.i = 0; r.e[LD_SM_ENERGY].m.f = 0.0f;
            }
        } else {
            const ldso_residual_t fr = W.freshRes[W.freshResBegin[-1 - from] + below];
            t.rnew = fr.is_new ? 1 : 0;
            r.e[LD_SM_STATE].m.i = fr.state_state; r.e[LD_SM_ACTIVE].m.i = fr.is_active ? 1 : 0; r.e[LD_SM_ENERGY].m.f = fr.state_energy;
        }
    }
    W.tab[q] = t; W.sr[q] = r;
    if (col < 8) W.pcw[(size_t) row * 8 + col] = (from >= 0) ? W.oPcw[(size_t) from * 8 + col] : PtCw{W.fresh[-1 - from].color[col], W.fresh[-1 - from].weights[col]};
    if (col == 0) {
        PtGeo g;
        memset(&g, 0, sizeof(g));
        int host;
        if (from >= 0) {
            const PtGeo o = W.oGeo[from];
            g.u = o.u; g.v = o.v; g.priorF = o.priorF; g.idepth = o.idepth; g.idepth_zero = o.idepth; g.idepth_backup = o.idepth;          // setIdepthZero(idepth) after every optimize()
            const int oh = W.oHost[from];
            host = -1;
            for (int f = 0; f < W.F; f++) host = (W.frameFrom[f] == oh) ? f : host;
            W.mrb[row] = W.oPt[from].maxRelBS; W.ngr[row] = W.oPt[from].numGood;
        } else {
            const ldso_point_t &p = W.fresh[-1 - from];
            g.u = p.u; g.v = p.v; g.priorF = p.priorF; g.idepth = p.idepth; g.idepth_zero = p.idepth_zero; g.idepth_backup = p.idepth;
            host = p.host;
            W.mrb[row] = W.freshMrb[-1 - from]; W.ngr[row] = W.freshNgr[-1 - from];
        }
        W.geo[row] = g; W.phost[row] = host;
    }
}
__global__ __launch_bounds__(256) void k_win_rebuild(WinDelta W) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= W.P * W.FS) return;
    win_rebuild_pair(W, q);
}
// every window of a batched update in one grid: blockIdx.y = the window's entry in the staged WinDelta table, blockIdx.x covers the largest window's pairs
__global__ __launch_bounds__(256) void k_win_rebuild_batch(const WinDelta *__restrict__ tab) {
    const WinDelta &W = tab[blockIdx.y];
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= W.P * W.FS) return;
    win_rebuild_pair(W, q);
}
__global__ __launch_bounds__(256) void k_point_stats_batch(const WinDelta *__restrict__ tab) {
    const WinDelta &W = tab[blockIdx.y];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= W.P) return;
    point_stats_one(W.pt0, W.pt1, W.mrb, W.ngr, i);
}

// host side of the arena: reserve (16-byte aligned) room, remember where it goes
struct WinStage {
    char *base, *devBase; size_t cap, used; WinXfer *tab; int n, maxN;
    // over a pinned arena and its device twin, with the transfer table (room for maxN entries; a batch brings a size of its own) at its head
    WinStage(char *h, char *d, size_t cap_, int maxN_ = LD_XFER_MAX) : base(h), devBase(d), cap(cap_), used(align_up((size_t) maxN_ * sizeof(WinXfer), 16)), tab(reinterpret_cast<WinXfer *>(h)), n(0), maxN(maxN_) {}
    template <class T> T *dev(T *hp) const { return reinterpret_cast<T *>(devBase + (reinterpret_cast<const char *>(hp) - base)); }          // where staged data lies on the device
    template <class T> T *put(T *dst, size_t count) {          // room for `count` elements that will land at dst; returns where to write them
        const size_t bytes = align_up(count * sizeof(T), 16);
        if (n >= maxN || used + bytes > cap) return nullptr;
        T *p = reinterpret_cast<T *>(base + used);
        if (count) { tab[n].dst = dst; tab[n].src = used; tab[n].words = count * sizeof(T) / 4; n++; }
        used += bytes;
        return p;
    }
    template <class T> T *raw(size_t count) {          // room without a destination (operands of k_win_rebuild)
        const size_t bytes = align_up(count * sizeof(T), 16);
        if (used + bytes > cap) return nullptr;
        T *p = reinterpret_cast<T *>(base + used);
        used += bytes;
        return p;
    }
    template <class T> bool again(T *dst, const T *staged, size_t count) {      // the same staged data to a second destination
        if (n >= maxN) return false;
        if (count) { tab[n].dst = dst; tab[n].src = (size_t) (reinterpret_cast<const char *>(staged) - base); tab[n].words = count * sizeof(T) / 4; n++; }
        return true;
    }
    template <class T> bool zero(T *dst, size_t count) {
        if (n >= maxN) return false;
        if (count) { tab[n].dst = dst; tab[n].src = LD_XFER_ZERO; tab[n].words = count * sizeof(T) / 4; n++; }
        return true;
    }
};

template <class T> static int h2d(ldso_ba *H, T *dst, const std::vector<T> &src) {
    if (src.empty()) return LDSO_OK;
    CHK(hipMemcpyAsync(dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice, H->stream));
    return LDSO_OK;
}
#define H2D(dst, vec) do { int r_ = h2d(H, (dst), (vec)); if (r_ != LDSO_OK) return r_; } while (0)

// The chunks of a window in two parts.  plan_chunks: host logic - the tables (first point, size and host of every chunk, first chunk of every host) from the
// window's host runs and the handle's chunk policy; adopt_chunks: the handle's own copies of them (block records, chunk starts, the closed form k_linearize_one
// reads).  How the tables reach the device is the caller's: build_chunks copies them on the handle's stream and waits, ldso_ba_batch_update_windows stages them
// with every other window's into the batch's one upload.
struct ChunkPlan { std::vector<int32_t> p0, cn, ch, cs; int CH; };
static int plan_chunks(ldso_ba *H, ChunkPlan &C) {
    // host-major chunks over the local shard [pBegin,pEnd)
    const BaDims &D = H->D;
    // smallest multiple of 4 points per chunk that keeps the grid within one wave of workgroups (one per CU)
    int CH = 4;
    if (!H->chunkCuts.empty() && H->chunkCuts.back() != D.pEnd) H->chunkCuts.clear();          // cuts made for another window: back to the regular policy
    const std::vector<int32_t> &cuts = H->chunkCuts;          // explicit ends (ascending): a chunk also ends at every host boundary
    if (!cuts.empty()) CH = 1 << 30;
    else if (H->chunkPoints > 0) CH = H->chunkPoints;      // ldso_ba_set_chunk_points / ldso_ba_batch_create: many windows share a launch, fewer and fatter workgroups
    else for (;; CH += 4) {
        int cnt = 0, run = 0, prev = -1;
        for (int q = D.pBegin; q < D.pEnd; q++) { int hq = H->h_phost[q]; if (hq != prev) { cnt += (run + CH - 1) / CH; run = 0; prev = hq; } run++; }
        cnt += (run + CH - 1) / CH;
        if (cnt <= H->numCU || CH >= 1024) break;
    }
    std::vector<int32_t> &p0 = C.p0, &cn = C.cn, &ch = C.ch, &cs = C.cs;
    p0.clear(); cn.clear(); ch.clear(); cs.assign(D.F + 1, 0);
    C.CH = CH;
    int p = D.pBegin;
    size_t ci = 0;
    for (int hst = 0; hst < D.F; hst++) {
        cs[hst] = (int) p0.size();
        while (p < D.pEnd && H->h_phost[p] == hst) {
            int e = p;
            while (ci < cuts.size() && cuts[ci] <= p) ci++;
            const int stop = ci < cuts.size() ? cuts[ci] : D.pEnd;
            while (e < D.pEnd && H->h_phost[e] == hst && e - p < CH && e < stop) e++;
            p0.push_back(p); cn.push_back(e - p); ch.push_back(hst);
            p = e;
        }
    }
    cs[D.F] = (int) p0.size();
    REQ(p == D.pEnd, "ldso_ba_set_window: points must be ordered by host frame (EnergyFunctional::allPoints order)");
    REQ((int) p0.size() <= H->maxChunks, "too many chunks");
    return LDSO_OK;
}
static void adopt_chunks(ldso_ba *H, const ChunkPlan &C) {
    BaDims &D = H->D;
    const std::vector<int32_t> &p0 = C.p0, &cn = C.cn, &ch = C.ch, &cs = C.cs;
    const int CH = C.CH;
    D.nChunks = (int) p0.size();
    H->h_blocks.resize(p0.size());
    for (size_t i = 0; i < p0.size(); i++) H->h_blocks[i] = BatchBlock{0, p0[i], cn[i], ch[i] | ((int32_t) i << 8)};
    for (int i = 0; i <= LD_MAXF; i++) H->chunkStarts.v[i] = (i <= D.F) ? cs[i] : cs[D.F];
    {
        LinHead &L = H->linHead;
        memset(&L, 0, sizeof(L));
        L.CH = CH; L.F = D.F;
        int q = D.pBegin;
        for (int hst = 0; hst <= LD_MAXF; hst++) {
            L.cs[hst] = (hst <= D.F) ? cs[hst] : cs[D.F];
            L.hostP0[hst] = q;
            while (hst < D.F && q < D.pEnd && H->h_phost[q] == hst) q++;
        }
        // the closed form must reproduce the table (it does for every chunking build_chunks makes; checked, not assumed)
        bool ok = true;
        for (size_t i = 0; i < p0.size() && ok; i++) {
            const int hst = ch[i];
            ok = p0[i] == L.hostP0[hst] + ((int) i - L.cs[hst]) * CH && cn[i] == std::min(CH, L.hostP0[hst + 1] - p0[i]);
        }
        H->linHeadOk = ok;
    }
}
int build_chunks(ldso_ba *H) {
    ChunkPlan C;
    RUN(plan_chunks(H, C));
    adopt_chunks(H, C);
    H2D(H->B.chunk_p0, C.p0); H2D(H->B.chunk_n, C.cn); H2D(H->B.chunk_host, C.ch); H2D(H->d_chunkStart, C.cs);
    CHK(hipMemcpyAsync(H->d_blocks, H->h_blocks.data(), H->h_blocks.size() * sizeof(BatchBlock), hipMemcpyHostToDevice, H->stream));
    CHK(hipStreamSynchronize(H->stream));
    return LDSO_OK;
}

// New chunks for the resident window.  The applied residual set carries per-chunk partial sums (top Hessian, energies) that the next
// reduce reads: under a new chunking they are re-formed by linearising the applied state once more with the decisions of the original pass
// kept (stepMode bit 2: same residual states, energies and activity - the Jacobians are a function of the state - only the partials are cut
// differently).
int rechunk(ldso_ba *H) {
    H->itemValid = false;
    RUN(build_chunks(H));
    if (H->appliedValid && !H->pendingApply) { RUN(launch_linearize(H, false, 4, -1)); H->cur ^= 1; }
    return LDSO_OK;
}

// ---- the pieces of a window upload, shared by ldso_ba_set_window, ldso_ba_update_window and ldso_ba_batch_update_windows (one window's delta is a ldso_win_job_t in the last two) ----
// The handle's arena with room for `need` bytes, free for the caller to fill: a copy out of it that may still be in flight (stageBusy) has landed.  The arena only
// ever holds staging data: growing it loses nothing of the resident window
static int handle_stage(ldso_ba *H, size_t need) {
    RUN(grow_arena(H->h_stage, H->d_stage, H->stageCap, need, 4, H->stream));
    if (H->stageBusy) { CHK(hipStreamSynchronize(H->stream)); H->stageBusy = false; }          // (after a growth the stream has drained already: the wait returns at once)
    return LDSO_OK;
}
// what the validation derives on the way: the flat residual index of every point's first residual, of every fresh point's first record, the new host of every point
struct WinPlan { std::vector<int32_t> resBegin, freshResBegin, newHost; int R = 0; };
// The checks of a delta against the resident window of H (indices only; nothing of the resident data is read back, nothing is written).  `who` names the entry.
static int check_window_delta(const ldso_ba *H, const char *who_, const ldso_win_job_t &J, WinPlan &Pl) {
    const std::string who(who_);
    const int F = J.F, P = J.P, n_fresh = J.n_fresh, n_fresh_res = J.n_fresh_res;
    const int32_t *image_slot = J.image_slot, *frame_from = J.frame_from, *point_from = J.point_from;
    const uint32_t *res_mask = J.res_mask;
    const ldso_point_t *fresh = J.fresh;
    const ldso_residual_t *fresh_res = J.fresh_res;
    REQ(H && image_slot && frame_from && point_from && res_mask, who + ": null argument");
    REQ(H->D.P > 0 && !H->pendingApply, who + ": no resident window, or a linearisation is pending (ldso_ba_apply_res first)");
    REQ(!H->hasL, who + ": the resident window holds linearised residuals (use ldso_ba_set_window)");
    REQ(H->D.pBegin == 0 && H->D.pEnd == H->D.P, who + ": sharded window");
    REQ(F >= 2 && F <= H->maxF && P >= 1 && P <= H->maxP && n_fresh >= 0 && n_fresh_res >= 0, who + ": window exceeds the handle's capacity");
    REQ(n_fresh == 0 || (fresh && J.fresh_mrb && J.fresh_ngr), who + ": fresh points without records");
    REQ(n_fresh_res == 0 || fresh_res, who + ": fresh residuals without records");
    const BaDims &oD = H->D;
    {
        std::vector<char> seen(oD.F, 0);
        for (int f = 0; f < F; f++) {
            REQ(frame_from[f] >= -1 && frame_from[f] < oD.F, who + ": frame_from out of range");
            if (frame_from[f] >= 0) { REQ(!seen[frame_from[f]], who + ": an old frame appears twice"); seen[frame_from[f]] = 1; }
            REQ(f == 0 || frame_from[f] < 0 || frame_from[f - 1] < frame_from[f], who + ": surviving frames must keep their order, inserted frames come last");
            REQ(image_slot[f] >= 0 && image_slot[f] < H->maxF && H->imgSlots[image_slot[f]] != nullptr, who + ": image slot not set");
        }
    }
    std::vector<int32_t> &resBegin = Pl.resBegin, &freshResBegin = Pl.freshResBegin, &newHost = Pl.newHost;
    resBegin.assign((size_t) P + 1, 0); freshResBegin.assign((size_t) n_fresh + 1, 0); newHost.assign((size_t) P, 0);
    {
        std::vector<int32_t> oldToNew(oD.F, -1);
        for (int f = 0; f < F; f++) if (frame_from[f] >= 0) oldToNew[frame_from[f]] = f;
        int lastOld = -1, nextFresh = 0, acc = 0;
        const uint32_t fmask = (F >= 32) ? 0xFFFFFFFFu : ((1u << F) - 1u);
        int fr = 0;
        for (int i = 0; i < P; i++) {
            const int from = point_from[i];
            int host;
            if (from >= 0) {
                REQ(from < oD.P && from > lastOld, who + ": surviving points must keep their order");
                lastOld = from;
                host = oldToNew[H->h_phost[from]];
                REQ(host >= 0, who + ": a surviving point is hosted by a frame that left the window");
            } else {
                REQ(-1 - from == nextFresh && nextFresh < n_fresh, who + ": fresh points must be numbered in window order");
                host = fresh[nextFresh].host;
                REQ(host >= 0 && host < F, who + ": fresh point host out of range");
                const int cnt = __builtin_popcount(res_mask[i]);
                freshResBegin[nextFresh] = fr;
                for (int c = 0; c < cnt; c++) {
                    REQ(fr < n_fresh_res && fresh_res[fr].target >= 0 && fresh_res[fr].target < F && fresh_res[fr].host == host,
                        who + ": fresh residual names a target outside the window or another host than its point's");
                    REQ(fresh_res[fr].point == nextFresh && !fresh_res[fr].is_linearized && ((res_mask[i] >> fresh_res[fr].target) & 1u)
                        && (c == 0 || fresh_res[fr - 1].target < fresh_res[fr].target), who + ": fresh residuals must be point-major, target-ascending and match res_mask");
                    fr++;
                }
                nextFresh++;
            }
            REQ((res_mask[i] & ~fmask) == 0 && !((res_mask[i] >> host) & 1u), who + ": res_mask names a frame outside the window or the host itself");
            REQ(i == 0 || newHost[i - 1] <= host, who + ": points must be ordered by host frame (EnergyFunctional::allPoints order)");
            newHost[i] = host;
            resBegin[i] = acc; acc += __builtin_popcount(res_mask[i]);
        }
        resBegin[P] = acc;
        freshResBegin[n_fresh] = fr;
        REQ(nextFresh == n_fresh && fr == n_fresh_res, who + ": unused fresh points / residuals");
    }
    Pl.R = resBegin[P];
    return LDSO_OK;
}
// arena bytes of one window: the delta (crosses PCIe) and the image (written on the device)
static size_t delta_bytes(const ldso_win_job_t &J) {
    const size_t F = (size_t) J.F, P = (size_t) J.P, nf = (size_t) J.n_fresh, nr = (size_t) J.n_fresh_res;
    return align_up(F * 4, 16) + 2 * align_up(P * 4, 16) + align_up((P + 1) * 4, 16) + align_up(nf * sizeof(ldso_point_t), 16) + align_up(nr * sizeof(ldso_residual_t), 16) + align_up((nf + 1) * 4, 16) + 2 * align_up(nf * 4, 16);
}
static size_t image_bytes(int F, int P_) {
    const size_t P = (size_t) P_, PS = P * (size_t) ((F + 7) / 8 * 8);
    return align_up(P * sizeof(PtGeo), 16) + align_up(P * 8 * sizeof(PtCw), 16) + align_up(P * 4, 16) + align_up(PS * sizeof(SlotTab), 16) + align_up(PS * sizeof(SlotRec), 16) + 2 * align_up(P * 4, 16);
}
// what k_win_rebuild reads of the resident window: taken BEFORE the handle adopts the new one
static void delta_resident(const ldso_ba *H, WinDelta &Wd) {
    const BaPtrs &B = H->B;
    const ResSet &So = H->sets[H->cur];
    Wd.oGeo = B.pgeo; Wd.oPcw = B.pcw; Wd.oHost = B.phost; Wd.oTab = B.rtab; Wd.oSlot = So.slot; Wd.oPt = So.pt; Wd.oF = H->D.F; Wd.oFS = H->D.FS; Wd.oP = H->D.P;
}
// room for the delta behind what the arena holds, filled; Wd receives its device addresses.  false: arena too small
static bool stage_delta(WinStage &W, const ldso_win_job_t &J, const WinPlan &Pl, WinDelta &Wd) {
    const int F = J.F, P = J.P, n_fresh = J.n_fresh, n_fresh_res = J.n_fresh_res;
    int32_t *hFrameFrom = W.raw<int32_t>(F), *hPointFrom = W.raw<int32_t>(P);
    uint32_t *hMask = W.raw<uint32_t>(P);
    int32_t *hResBegin = W.raw<int32_t>((size_t) P + 1);
    ldso_point_t *hFresh = W.raw<ldso_point_t>(n_fresh);
    ldso_residual_t *hFreshRes = W.raw<ldso_residual_t>(n_fresh_res);
    int32_t *hFreshResBegin = W.raw<int32_t>((size_t) n_fresh + 1);
    float *hMrb = W.raw<float>(n_fresh); int32_t *hNgr = W.raw<int32_t>(n_fresh);
    if (!(hFrameFrom && hPointFrom && hMask && hResBegin && hFresh && hFreshRes && hFreshResBegin && hMrb && hNgr)) return false;
    memcpy(hFrameFrom, J.frame_from, (size_t) F * 4); memcpy(hPointFrom, J.point_from, (size_t) P * 4); memcpy(hMask, J.res_mask, (size_t) P * 4);
    memcpy(hResBegin, Pl.resBegin.data(), ((size_t) P + 1) * 4); memcpy(hFreshResBegin, Pl.freshResBegin.data(), ((size_t) n_fresh + 1) * 4);
    if (n_fresh) { memcpy(hFresh, J.fresh, (size_t) n_fresh * sizeof(ldso_point_t)); memcpy(hMrb, J.fresh_mrb, (size_t) n_fresh * 4); memcpy(hNgr, J.fresh_ngr, (size_t) n_fresh * 4); }
    if (n_fresh_res) memcpy(hFreshRes, J.fresh_res, (size_t) n_fresh_res * sizeof(ldso_residual_t));
    Wd.frameFrom = W.dev(hFrameFrom); Wd.pointFrom = W.dev(hPointFrom); Wd.resMask = W.dev(hMask); Wd.resBegin = W.dev(hResBegin);
    Wd.fresh = W.dev(hFresh); Wd.freshRes = W.dev(hFreshRes); Wd.freshResBegin = W.dev(hFreshResBegin);
    Wd.freshMrb = W.dev(hMrb); Wd.freshNgr = W.dev(hNgr);
    Wd.F = F; Wd.FS = (F + 7) / 8 * 8; Wd.P = P;
    return true;
}
// The handle's dimensions for a window of F frames on the image slots `image_slot`, P points, R residuals (the caller holds a WinGuard: a slot without an image leaves the
// handle without a window).  What the callers set differently stays theirs: D.nL / hasL, cur, pendingApply, appliedValid, hasPrior, itemValid, h_phost, flat2slot
static int adopt_dims(ldso_ba *H, const std::string &who, int F, const int32_t *image_slot, int P, int R) {
    BaDims &D = H->D;
    D.F = F; D.FS = (F + 7) / 8 * 8; D.P = P; D.R = R; D.n = 8 * F + 4; D.GS = 8 * D.FS + LD_GEXTRA; D.w = H->w; D.h = H->h; D.nsg = D.FS / 8; D.ks = H->reduceSplits;
    D.pBegin = 0; D.pEnd = P; D.wM3G = (float) (H->w - 3); D.hM3G = (float) (H->h - 3);
    H->GSP = (D.GS + 15) / 16 * 16;
    H->R = R;
    H->imageSlot.assign(image_slot, image_slot + F);
    for (int f = 0; f < F; f++) {
        REQ(image_slot[f] >= 0 && image_slot[f] < H->maxF && H->imgSlots[image_slot[f]] != nullptr, who + ": image slot not set");
        H->B.img[f] = H->imgSlots[image_slot[f]];
    }
    return LDSO_OK;
}
// the handle describes the new window of a checked delta: dimensions, image slots, host-side tables; no applied linearisation, no prior (the caller holds a WinGuard)
static int adopt_window(ldso_ba *H, const char *who, const ldso_win_job_t &J, const WinPlan &Pl) {
    const int F = J.F, P = J.P, R = Pl.R;
    RUN(adopt_dims(H, who, F, J.image_slot, P, R));
    const int FS = H->D.FS;
    H->D.nL = 0;
    H->h_phost.assign(Pl.newHost.begin(), Pl.newHost.end());
    H->flat2slot.assign(R, -1);
    for (int i = 0; i < P; i++) { int k = Pl.resBegin[i]; for (int t = 0; t < F; t++) if ((J.res_mask[i] >> t) & 1u) H->flat2slot[k++] = (int32_t) ((size_t) i * FS + t); }
    H->hasL = false; H->cur = 0; H->pendingApply = false; H->appliedValid = false; H->itemValid = false;
    H->hasPrior = false;
    return LDSO_OK;
}
// The image of the window H has adopted, the ONE list of its destinations and zero fills: room in the arena for the five parts that are copied to the window's buffers
// (both residual sets take the same slot records), zero for everything else a new window starts from - the point records and accumulators of both sets, the
// marginalisation prior (a new window has a new dimension 8F+4; ldso_ba_set_prior follows when there is one), the scalars, the Schur partials.  16 table entries.
// `stats`: room for maxRelBaseline / numGoodResiduals behind the parts (no destination: k_point_stats reads them where they lie).  false: arena or table too small
struct WinImage { PtGeo *geo; PtCw *pcw; int32_t *phost; SlotTab *tab; SlotRec *sr; float *mrb; int32_t *ngr; };          // host pointers into the arena
static bool stage_image(ldso_ba *H, WinStage &W, bool stats, WinImage &I) {
    BaPtrs &B = H->B;
    const BaDims &D = H->D;
    const size_t P = (size_t) D.P, PS = P * (size_t) D.FS;
    I.geo = W.put(B.pgeo, P);
    I.pcw = W.put(B.pcw, P * 8);
    I.phost = W.put(B.phost, P);
    I.tab = W.put(B.rtab, PS);
    I.sr = W.put(H->sets[0].slot, PS);
    if (!(I.geo && I.pcw && I.phost && I.tab && I.sr)) return false;
    I.mrb = stats ? W.raw<float>(P) : nullptr; I.ngr = stats ? W.raw<int32_t>(P) : nullptr;
    if (stats && !(I.mrb && I.ngr)) return false;
    bool okT = W.again(H->sets[1].slot, I.sr, PS);
    for (int s_ = 0; s_ < 2; s_++) {
        ResSet &S = H->sets[s_];
        okT = okT && W.zero(S.pt, P) && W.zero(S.acc, P) && W.zero(S.G, P * D.GS);
    }
    okT = okT && W.zero(B.HM, (size_t) D.n * D.n) && W.zero(B.bM, (size_t) D.n) && W.zero(B.scalars, (size_t) 16) && W.zero(B.scPart, (size_t) LD_SC_SPLITS * H->GSP * H->GSP);
    return okT;
}
// the image as k_win_rebuild writes it and k_point_stats reads it: the device addresses of its parts
static bool stage_delta_image(ldso_ba *H, WinStage &W, WinDelta &Wd) {
    WinImage I;
    if (!stage_image(H, W, true, I)) return false;
    Wd.geo = W.dev(I.geo); Wd.pcw = W.dev(I.pcw); Wd.phost = W.dev(I.phost); Wd.tab = W.dev(I.tab); Wd.sr = W.dev(I.sr); Wd.mrb = W.dev(I.mrb); Wd.ngr = W.dev(I.ngr);
    Wd.pt0 = H->sets[0].pt; Wd.pt1 = H->sets[1].pt;
    return true;
}

extern "C" {

int ldso_ba_set_window(ldso_ba_t *H, int F, const int32_t *image_slot, int P, const ldso_point_t *pts, int R, const ldso_residual_t *res,
                       const ldso_rawjac_t *linJ, const float *lin_rtz) {
    REQ(H && image_slot && pts && res, "ldso_ba_set_window: null argument");
    REQ(F >= 2 && F <= H->maxF && P >= 1 && P <= H->maxP && R >= 0, "ldso_ba_set_window: window exceeds the handle's capacity");
    CHK(hipSetDevice(H->device));
    BaDims &D = H->D;
    BaPtrs &B = H->B;
    WinGuard guard{H, false};          // a failure from here on leaves the handle without a window (ba_host.h)
    RUN(adopt_dims(H, "ldso_ba_set_window", F, image_slot, P, R));
    const int FS = D.FS;
    const size_t PS = (size_t) P * FS;
    // ---- staging arena: everything the window needs goes over PCIe in ONE copy and is distributed (or zero-filled) by ONE kernel ----
    size_t nLin = 0;
    for (int i = 0; i < R; i++) nLin += res[i].is_linearized ? 1 : 0;
    REQ(nLin == 0 || (linJ && lin_rtz), "ldso_ba_set_window: linearised residual without linJ / lin_res_toZeroF");
    RUN(handle_stage(H, align_up(LD_XFER_MAX * sizeof(WinXfer), 16) + image_bytes(F, P) + align_up(nLin * sizeof(ldso_rawjac_t), 16) + align_up(nLin * 32, 16) + 64));
    WinStage W(H->h_stage, H->d_stage, H->stageCap);
    WinImage I;
    REQ(stage_image(H, W, false, I), "ldso_ba_set_window: staging arena too small or upload table overflow (internal)");
    // the image's parts are filled from the caller's records; behind them what only this entry brings: the linearised residuals' Jacobians and res_toZeroF
    PtGeo *geo = I.geo; PtCw *pcw = I.pcw; int32_t *phost = I.phost; SlotTab *tab = I.tab; SlotRec *sr = I.sr;
    ldso_rawjac_t *Jl = W.put(B.Jlin, nLin);
    float *rtz = W.put(B.rtz, nLin * 8);
    REQ(Jl && rtz, "ldso_ba_set_window: staging arena too small (internal)");
    H->h_phost.resize(P);
    for (int i = 0; i < P; i++) {
        PtGeo g_;
        memset(&g_, 0, sizeof(g_));           // step, the scalars of the last solve: zero
        g_.u = pts[i].u; g_.v = pts[i].v; g_.priorF = pts[i].priorF; g_.idepth = pts[i].idepth; g_.idepth_zero = pts[i].idepth_zero; g_.idepth_backup = pts[i].idepth;
        geo[i] = g_;
        REQ(pts[i].host >= 0 && pts[i].host < F, "ldso_ba_set_window: point host out of range");
        H->h_phost[i] = pts[i].host; phost[i] = pts[i].host;
        for (int k = 0; k < 8; k++) pcw[(size_t) i * 8 + k] = PtCw{pts[i].color[k], pts[i].weights[k]};
    }
    memset(sr, 0, PS * sizeof(SlotRec));          // JpJdF, centre, energies, activity, removal flag: zero
    for (size_t q = 0; q < PS; q++) { tab[q] = SlotTab{-1, 0, 0, -1}; sr[q].e[LD_SM_STATE].m.i = LDSO_RES_OOB; }
    H->flat2slot.assign(R, -1);
    size_t nl = 0;
    for (int i = 0; i < R; i++) {
        const ldso_residual_t &r = res[i];
        REQ(r.point >= 0 && r.point < P && r.target >= 0 && r.target < F && r.host == pts[r.point].host && r.target != r.host, "ldso_ba_set_window: bad residual indices");
        size_t slot = (size_t) r.point * FS + r.target;
        REQ(tab[slot].rflat < 0, "ldso_ba_set_window: two residuals of one point target the same frame");
        tab[slot].rflat = i; tab[slot].rlin = r.is_linearized ? 1 : 0; tab[slot].rnew = r.is_new ? 1 : 0;
        sr[slot].e[LD_SM_STATE].m.i = r.state_state; sr[slot].e[LD_SM_ACTIVE].m.i = r.is_active ? 1 : 0; sr[slot].e[LD_SM_ENERGY].m.f = r.state_energy;
        H->flat2slot[i] = (int32_t) slot;
        if (r.is_linearized) {
            tab[slot].rlidx = (int32_t) nl;
            Jl[nl] = linJ[i];
            for (int k = 0; k < 8; k++) rtz[nl * 8 + k] = lin_rtz[(size_t) i * 8 + k];
            nl++;
            // takeData (Residuals.h:123-128)
            const ldso_rawjac_t &J = linJ[i];
            float v0 = J.JIdx2[0] * J.Jpdd[0] + J.JIdx2[1] * J.Jpdd[1], v1 = J.JIdx2[2] * J.Jpdd[0] + J.JIdx2[3] * J.Jpdd[1];
            for (int k = 0; k < 6; k++) sr[slot].e[k].jp = J.Jpdxi[0][k] * v0 + J.Jpdxi[1][k] * v1;
            sr[slot].e[6].jp = J.JabJIdx[0] * J.Jpdd[0] + J.JabJIdx[1] * J.Jpdd[1];
            sr[slot].e[7].jp = J.JabJIdx[2] * J.Jpdd[0] + J.JabJIdx[3] * J.Jpdd[1];
        }
    }
    D.nL = (int) nLin;
    H->hasL = D.nL > 0;
    H->cur = 0; H->pendingApply = false; H->appliedValid = false;
    H->hasPrior = false;
    CHK(hipMemcpyAsync(H->d_stage, H->h_stage, W.used, hipMemcpyHostToDevice, H->stream));
    hipLaunchKernelGGL(k_win_scatter, dim3(256), dim3(256), 0, H->stream, (const char *) H->d_stage, W.n);
    CHK(hipGetLastError());
    CHK(hipStreamSynchronize(H->stream));
    const int rc_ = build_chunks(H);
    guard.ok = (rc_ == LDSO_OK);
    return rc_;
}

// PointHessian::maxRelBaseline / numGoodResiduals live across optimize() calls in the reference (FullSystem.cc:1521-1536 updates them in the
// fixing pass, AccumulatedSCHessian.cc:14-21 zeroes maxRelBaseline of points without an active residual).  ldso_ba_set_window starts both at
// zero; a caller that keeps the reference's objects seeds them here so that ldso_ba_get_points returns the values to store back.
int ldso_ba_set_point_stats(ldso_ba_t *H, const float *maxRelBaseline, const int32_t *numGoodResiduals) {
    REQ(H && H->D.P > 0 && maxRelBaseline && numGoodResiduals, "ldso_ba_set_point_stats: bad arguments / no window");
    CHK(hipSetDevice(H->device));
    // one 4-byte field of every 64-byte PtRec of both sets: through the pinned staging arena of ldso_ba_set_window (free again: that call ends
    // synchronised) and one scatter kernel - four strided 2-D copies took 0.25 ms for 2000 points
    const size_t P = (size_t) H->D.P;
    REQ(H->h_stage && H->stageCap >= 8 * P, "ldso_ba_set_point_stats: staging arena missing (internal)");
    if (H->stageBusy) { CHK(hipStreamSynchronize(H->stream)); H->stageBusy = false; }
    memcpy(H->h_stage, maxRelBaseline, 4 * P); memcpy(H->h_stage + 4 * P, numGoodResiduals, 4 * P);
    CHK(hipMemcpyAsync(H->d_stage, H->h_stage, 8 * P, hipMemcpyHostToDevice, H->stream));
    hipLaunchKernelGGL(k_point_stats, dim3((unsigned) ((P + 255) / 256)), dim3(256), 0, H->stream, H->sets[0].pt, H->sets[1].pt, (const float *) H->d_stage, (const int32_t *) (H->d_stage + 4 * P), (int) P);
    CHK(hipGetLastError());
    CHK(hipStreamSynchronize(H->stream));          // the arena is handed back to the next ldso_ba_set_window
    return LDSO_OK;
}

// The window of the next optimize() as a DELTA against the resident one - what the reference's own maintenance calls do to the window between two key frames
// (EnergyFunctional.cc: insertFrame :32, insertResidual :26, dropResidual :63, removePoint :153, dropPointsF :224, marginalizeFrame :72, makeIDX :380), expressed
// in one call on the order makeIDX produces:
//   frame_from[f]   the old index of new frame f (frames that appear nowhere were marginalised), -1 = insertFrame
//   point_from[i]   the old row of new point i (rows that appear nowhere were removed / dropped / marginalised), -1 - k = the k-th fresh point (insertPoint);
//                   surviving points keep their relative order (makeIDX walks frames, then the host frame's features: both orders are stable)
//   res_mask[i]     bit t set: point i has a residual with target frame t (NEW numbering).  Against the resident slots this says insertResidual (bit set, slot
//                   empty: the residual starts IN, energy 0, isNew) and dropResidual (slot occupied, bit clear)
//   fresh / fresh_res / fresh_mrb / fresh_ngr   the new points in the layout of ldso_ba_set_window (host = new frame index), their residuals point-major and
//                   target-ascending with .point = index into `fresh`, PointHessian::maxRelBaseline / numGoodResiduals
// The flat residual order of the new window (ldso_ba_get_residuals ...) is point-major, target-ascending.  The result is the window a fresh ldso_ba_set_window +
// ldso_ba_set_point_stats of the same objects produces, byte for byte; ldso_ba_set_frames / ldso_ba_set_prior follow as they do there.
int ldso_ba_update_window(ldso_ba_t *H, int F, const int32_t *image_slot, const int32_t *frame_from, int P, const int32_t *point_from, const uint32_t *res_mask,
                          int n_fresh, const ldso_point_t *fresh, int n_fresh_res, const ldso_residual_t *fresh_res, const float *fresh_mrb, const int32_t *fresh_ngr) {
    const ldso_win_job_t J{F, image_slot, frame_from, P, point_from, res_mask, n_fresh, fresh, n_fresh_res, fresh_res, fresh_mrb, fresh_ngr};
    WinPlan Pl;
    RUN(check_window_delta(H, "ldso_ba_update_window", J, Pl));
    CHK(hipSetDevice(H->device));
    // ---- arena: [table | delta | image]; only table + delta cross PCIe ----
    RUN(handle_stage(H, align_up(LD_XFER_MAX * sizeof(WinXfer), 16) + delta_bytes(J) + image_bytes(F, P) + 64));
    WinStage W(H->h_stage, H->d_stage, H->stageCap);
    WinDelta Wd;
    delta_resident(H, Wd);
    REQ(stage_delta(W, J, Pl, Wd), "ldso_ba_update_window: staging arena too small (internal)");
    const size_t upBytes = W.used;
    // from here on the handle describes the new window (a failure leaves it without one, as in ldso_ba_set_window)
    WinGuard guard{H, false};
    RUN(adopt_window(H, "ldso_ba_update_window", J, Pl));
    REQ(stage_delta_image(H, W, Wd), "ldso_ba_update_window: staging arena too small or upload table overflow (internal)");
    CHK(hipMemcpyAsync(H->d_stage, H->h_stage, upBytes, hipMemcpyHostToDevice, H->stream));
    hipLaunchKernelGGL(k_win_rebuild, dim3((unsigned) (((size_t) Wd.P * Wd.FS + 255) / 256)), dim3(256), 0, H->stream, Wd);
    CHK(hipGetLastError());
    hipLaunchKernelGGL(k_win_scatter, dim3(256), dim3(256), 0, H->stream, (const char *) H->d_stage, W.n);
    CHK(hipGetLastError());
    hipLaunchKernelGGL(k_point_stats, dim3((unsigned) ((P + 255) / 256)), dim3(256), 0, H->stream, H->sets[0].pt, H->sets[1].pt, (const float *) Wd.mrb, (const int32_t *) Wd.ngr, P);
    CHK(hipGetLastError());
    CHK(hipStreamSynchronize(H->stream));
    const int rc_ = build_chunks(H);
    guard.ok = (rc_ == LDSO_OK);
    return rc_;
}

// ---------------------------------------------------------------------------------------------------------------------------------------------------
// The same step for every window of a batch (include/ldso_hip.h: ldso_ba_batch_update_windows): the pieces above per window - check_window_delta for ALL windows
// first, then stage_delta / adopt_window / stage_delta_image into ONE arena (the batch's, batch_stage) laid out [transfer table | work units | n WinDelta | every
// window's delta | every window's chunk tables || every window's image]: what stands in front of || goes up in one copy, the images are written by
// k_win_rebuild_batch and distributed, with the chunk tables and the zero fills, by k_win_scatter_batch.  In between the batch re-runs its chunk policy on the new
// point counts (batch_chunk_policy, as ldso_ba_batch_create): the participating windows hold no applied linearisation, so cutting them is host work (plan_chunks)
// whose tables ride in the same upload; a window that sits out is re-cut by rechunk.
// ---------------------------------------------------------------------------------------------------------------------------------------------------
#define LD_BATCH_XFER_PER_WIN 24          // transfer-table entries of one window: 5 image parts, 1 copy for the second set, 10 zero fills, 5 chunk tables (+ slack)
static_assert(sizeof(ldso_win_job_t) == 96 && sizeof(ldso_frames_job_t) == 32, "the job records of the batched entries as the Python binding declares them");
// the work units of a finished transfer table (k_win_scatter_batch) -> unit0[0 .. n]; returns the grid
static int xfer_units(const WinStage &W, int32_t *unit0) {
    int u = 0;
    for (int e = 0; e < W.n; e++) { unit0[e] = u; u += (int) ((W.tab[e].words + LD_XFER_UNIT - 1) / LD_XFER_UNIT); }
    unit0[W.n] = u;
    return u;
}
struct BatchWinGuard {
    ldso_ba_batch *Bt; std::vector<ldso_ba *> taking; bool ok;
    ~BatchWinGuard() { if (!ok) { for (ldso_ba *H : taking) { WinGuard g{H, false}; } Bt->lost = true; } }
};
int ldso_ba_batch_update_windows(ldso_ba_batch_t *Bt, const ldso_win_job_t *jobs) {
    REQ(Bt, "ldso_ba_batch_update_windows: null batch");
    REQ(jobs, "ldso_ba_batch_update_windows: null job array");
    REQ(!Bt->lost, "ldso_ba_batch_update_windows: an earlier call left windows of the batch unset: destroy and re-create the batch");
    ldso_ba *H0 = Bt->h[0];
    const int n = (int) Bt->h.size();
    // ---- validation of every participating window before anything is written ----
    std::vector<WinPlan> plans((size_t) n);
    std::vector<int> part;
    for (int i = 0; i < n; i++) {
        if (jobs[i].frame_from == nullptr) continue;
        RUN(check_window_delta(Bt->h[(size_t) i], "ldso_ba_batch_update_windows", jobs[i], plans[(size_t) i]));
        REQ((jobs[i].F + 7) / 8 * 8 == Bt->FS, "ldso_ba_batch_update_windows: the new window's slot-table width differs from the batch's (all F <= 8 or all 9 <= F <= 16)");
        part.push_back(i);
    }
    REQ(!part.empty(), "ldso_ba_batch_update_windows: no window takes part (every frame_from is NULL)");
    const int nPart = (int) part.size();
    CHK(hipSetDevice(H0->device));
    // ---- the arena ----
    const int maxEntries = nPart * LD_BATCH_XFER_PER_WIN;
    const size_t headBytes = align_up((size_t) maxEntries * sizeof(WinXfer), 16) + align_up(((size_t) maxEntries + 1) * 4, 16) + align_up((size_t) nPart * sizeof(WinDelta), 16);
    size_t up = headBytes, img = 64;
    for (int i : part) {
        const ldso_ba *H = Bt->h[(size_t) i];
        up += delta_bytes(jobs[i]) + 3 * align_up((size_t) H->maxChunks * 4, 16) + align_up(((size_t) jobs[i].F + 1) * 4, 16) + align_up((size_t) H->maxChunks * sizeof(BatchBlock), 16);
        img += image_bytes(jobs[i].F, jobs[i].P);
    }
    RUN(batch_stage(Bt, up, img));          // (may wait for the stream and replace the arena: nothing of the windows lives there)
    WinStage W(Bt->h_stage, Bt->d_stage, Bt->stageCap, maxEntries);
    int32_t *unit0 = W.raw<int32_t>((size_t) maxEntries + 1);
    WinDelta *hWd = W.raw<WinDelta>((size_t) nPart);
    REQ(unit0 && hWd, "ldso_ba_batch_update_windows: staging arena too small (internal)");
    std::vector<WinDelta> Wd((size_t) nPart);
    for (int k = 0; k < nPart; k++) {
        delta_resident(Bt->h[(size_t) part[(size_t) k]], Wd[(size_t) k]);
        REQ(stage_delta(W, jobs[part[(size_t) k]], plans[(size_t) part[(size_t) k]], Wd[(size_t) k]), "ldso_ba_batch_update_windows: staging arena too small (internal)");
    }
    // ---- from here on the participating handles describe their new windows: a failure leaves them without one and the batch fit for ldso_ba_batch_destroy only ----
    BatchWinGuard guard{Bt, {}, false};
    for (int i : part) guard.taking.push_back(Bt->h[(size_t) i]);
    for (int i : part) RUN(adopt_window(Bt->h[(size_t) i], "ldso_ba_batch_update_windows", jobs[i], plans[(size_t) i]));
    // the batch re-cuts itself: the policy of ldso_ba_batch_create on the new point counts (the cuts the batch gave its windows are its own to replace)
    if (Bt->balanced) for (ldso_ba *H : Bt->h) H->chunkCuts.clear();
    BatchCuts C;
    batch_chunk_policy(Bt->h.data(), n, C);
    for (int i : part) {
        ldso_ba *H = Bt->h[(size_t) i];
        ChunkPlan Cp;
        RUN(batch_cut_window(H, i, C, true, [&](ldso_ba *Hc) { return plan_chunks(Hc, Cp); }));
        adopt_chunks(H, Cp);
        int32_t *p0 = W.put(H->B.chunk_p0, Cp.p0.size()), *cn = W.put(H->B.chunk_n, Cp.cn.size()), *ch = W.put(H->B.chunk_host, Cp.ch.size()), *cs = W.put(H->d_chunkStart, Cp.cs.size());
        BatchBlock *bl = W.put(H->d_blocks, H->h_blocks.size());
        REQ(p0 && cn && ch && cs && bl, "ldso_ba_batch_update_windows: staging arena too small or upload table overflow (internal)");
        memcpy(p0, Cp.p0.data(), Cp.p0.size() * 4); memcpy(cn, Cp.cn.data(), Cp.cn.size() * 4); memcpy(ch, Cp.ch.data(), Cp.ch.size() * 4); memcpy(cs, Cp.cs.data(), Cp.cs.size() * 4);
        memcpy(bl, H->h_blocks.data(), H->h_blocks.size() * sizeof(BatchBlock));
    }
    size_t upBytes = W.used;
    size_t maxPS = 0, maxP = 0;
    for (int k = 0; k < nPart; k++) {
        REQ(stage_delta_image(Bt->h[(size_t) part[(size_t) k]], W, Wd[(size_t) k]), "ldso_ba_batch_update_windows: staging arena too small or upload table overflow (internal)");
        maxPS = std::max(maxPS, (size_t) Wd[(size_t) k].P * Wd[(size_t) k].FS); maxP = std::max(maxP, (size_t) Wd[(size_t) k].P);
    }
    REQ(upBytes <= up && W.used <= Bt->stageCap, "ldso_ba_batch_update_windows: staging arena too small (internal)");
    memcpy(hWd, Wd.data(), (size_t) nPart * sizeof(WinDelta));
    const int units = xfer_units(W, unit0);
    hipStream_t st = H0->stream;
    CHK(hipMemcpyAsync(Bt->d_stage, Bt->h_stage, upBytes, hipMemcpyHostToDevice, st));
    // the order of the single-window path: the rebuild reads the resident windows that the scatter overwrites
    hipLaunchKernelGGL(k_win_rebuild_batch, dim3((unsigned) ((maxPS + 255) / 256), (unsigned) nPart), dim3(256), 0, st, (const WinDelta *) W.dev(hWd));
    CHK(hipGetLastError());
    hipLaunchKernelGGL(k_win_scatter_batch, dim3((unsigned) units), dim3(256), 0, st, (const char *) Bt->d_stage, (const WinXfer *) Bt->d_stage, (const int32_t *) W.dev(unit0), W.n);
    CHK(hipGetLastError());
    hipLaunchKernelGGL(k_point_stats_batch, dim3((unsigned) ((maxP + 255) / 256), (unsigned) nPart), dim3(256), 0, st, (const WinDelta *) W.dev(hWd));
    CHK(hipGetLastError());
    // the cost of sitting out: the window keeps its bytes and its applied state, re-formed under the batch's new chunks (one linearisation launch, the parity flips)
    for (int i = 0; i < n; i++) if (jobs[i].frame_from == nullptr) RUN(batch_cut_window(Bt->h[(size_t) i], i, C, true, rechunk));
    Bt->balanced = C.balanced;
    for (int u = 0; u < 3; u++) Bt->wg[u] = C.wg[u];
    Bt->chunkPoints = batch_chunk_points(Bt->h.data(), n, C);
    Bt->Dmax = H0->D;
    for (ldso_ba *H : Bt->h) if (H->D.F > Bt->Dmax.F) Bt->Dmax = H->D;
    RUN(batch_refresh(Bt));
    CHK(hipStreamSynchronize(st));          // the arena is handed back to the next batched call
    guard.ok = true;
    return LDSO_OK;
}

// ldso_ba_set_frames + ldso_ba_set_prior for every window of the batch that brings frames: the records of all of them in one upload, distributed (and the absent
// priors zero-filled) by k_win_scatter_batch, then the adjoints and the precalc values of all windows in one k_solve_batch over a table of the participating
// windows' descriptors that rides in the same upload (SK_ADJ | SK_PRECALC read neither the residual sets nor the scalars the kernel picks its set by).
int ldso_ba_batch_set_frames(ldso_ba_batch_t *Bt, const ldso_frames_job_t *jobs) {
    REQ(Bt, "ldso_ba_batch_set_frames: null batch");
    REQ(jobs, "ldso_ba_batch_set_frames: null job array");
    REQ(!Bt->lost, "ldso_ba_batch_set_frames: an earlier ldso_ba_batch_update_windows left windows of the batch unset: destroy and re-create the batch");
    ldso_ba *H0 = Bt->h[0];
    const int n = (int) Bt->h.size();
    std::vector<int> part;
    size_t up = 0;
    for (int i = 0; i < n; i++) {
        if (jobs[i].frames == nullptr) continue;
        const ldso_ba *H = Bt->h[(size_t) i];
        REQ(jobs[i].calib && H->D.P > 0 && H->D.F > 0, "ldso_ba_batch_set_frames: a window that takes part needs its calibration and a resident window");
        part.push_back(i);
        up += align_up((size_t) H->D.F * sizeof(DevFrame), 16) + align_up(sizeof(DevCalib), 16) + align_up((size_t) H->D.n * H->D.n * 8, 16) + align_up((size_t) H->D.n * 8, 16);
    }
    if (part.empty()) return LDSO_OK;
    const int nPart = (int) part.size(), maxEntries = 4 * nPart;
    up += align_up((size_t) maxEntries * sizeof(WinXfer), 16) + align_up(((size_t) maxEntries + 1) * 4, 16) + align_up((size_t) nPart * sizeof(BatchItem), 16) + 64;
    CHK(hipSetDevice(H0->device));
    RUN(batch_stage(Bt, up, 0));
    WinStage W(Bt->h_stage, Bt->d_stage, Bt->stageCap, maxEntries);
    int32_t *unit0 = W.raw<int32_t>((size_t) maxEntries + 1);
    BatchItem *hItems = W.raw<BatchItem>((size_t) nPart);
    REQ(unit0 && hItems, "ldso_ba_batch_set_frames: staging arena too small (internal)");
    for (int k = 0; k < nPart; k++) {
        ldso_ba *H = Bt->h[(size_t) part[(size_t) k]];
        const ldso_frames_job_t &J = jobs[part[(size_t) k]];
        const size_t nn = (size_t) H->D.n;
        DevFrame *df = W.put(H->B.frames, (size_t) H->D.F);
        DevCalib *dc = W.put(H->B.calib, 1);
        REQ(df && dc, "ldso_ba_batch_set_frames: staging arena too small (internal)");
        fill_dev_frames(H, J.frames, J.calib, df, dc);
        bool ok = true;
        if (J.HM) { double *q = W.put(H->B.HM, nn * nn); ok = ok && q; if (q) memcpy(q, J.HM, nn * nn * 8); } else ok = ok && W.zero(H->B.HM, nn * nn);
        if (J.bM) { double *q = W.put(H->B.bM, nn); ok = ok && q; if (q) memcpy(q, J.bM, nn * 8); } else ok = ok && W.zero(H->B.bM, nn);
        REQ(ok, "ldso_ba_batch_set_frames: staging arena too small (internal)");
        H->hasPrior = (J.HM != nullptr) || (J.bM != nullptr);
        fill_item(hItems[k], H, Bt->ks, true, part[(size_t) k]);          // the window's descriptors as batch_refresh writes them
    }
    const int units = xfer_units(W, unit0);
    hipStream_t st = H0->stream;
    CHK(hipMemcpyAsync(Bt->d_stage, Bt->h_stage, W.used, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_win_scatter_batch, dim3((unsigned) units), dim3(256), 0, st, (const char *) Bt->d_stage, (const WinXfer *) Bt->d_stage, (const int32_t *) W.dev(unit0), W.n);
    CHK(hipGetLastError());
    CHK(ba_launch_solve_batch((const BatchItem *) W.dev(hItems), nPart, Bt->Dmax, H0->settings, SK_ADJ | SK_PRECALC, 0, nullptr, st));
    CHK(hipStreamSynchronize(st));
    return LDSO_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------------------------
// The same delta, recorded call by call as the reference edits its window (EnergyFunctional.cc): ldso_ba_window_begin, then any sequence of
//   ldso_ba_remove_frame    marginalizeFrame :72 (:138-150: the frame leaves; FullSystem::marginalizeFrame :607-632: so do the residuals that target it and the points it hosts)
//   ldso_ba_insert_frame    insertFrame :32 (the new frame's id for the calls below is returned: oF, oF + 1, ...)
//   ldso_ba_remove_points   removePoint :153 / dropPointsF :224 / the points marginalizePointsF :165 has absorbed
//   ldso_ba_drop_residuals  dropResidual :63
//   ldso_ba_add_residuals   insertResidual :26 for points of the window
//   ldso_ba_add_points      insertPoint + insertResidual for freshly activated points, each placed in front of a resident row (makeIDX :380 order)
// and ldso_ba_window_commit, which numbers the surviving frames (in order) and the inserted ones behind them and applies everything as ONE
// ldso_ba_update_window.  Host-side bookkeeping only until the commit; an invalid edit is rejected there and leaves the resident window as it was.
// ---------------------------------------------------------------------------------------------------------------------------------------------------
int ldso_ba_window_begin(ldso_ba_t *H) {
    REQ(H && H->D.P > 0 && !H->hasL && !H->pendingApply, "ldso_ba_window_begin: no resident window to edit (or linearised residuals / a pending linearisation)");
    ldso_ba::WindowEdit &E = H->edit;
    E = ldso_ba::WindowEdit();
    E.active = true; E.oF = H->D.F; E.oP = H->D.P;
    E.frameGone.assign(E.oF, 0); E.rowGone.assign(E.oP, 0); E.mask.assign(E.oP, 0u);
    for (int i = 0; i < H->R; i++) { const int sl = H->flat2slot[i]; E.mask[sl / H->D.FS] |= 1u << (sl % H->D.FS); }
    return LDSO_OK;
}
#define REQ_EDIT(name) REQ(H && H->edit.active, name ": no edit in progress (ldso_ba_window_begin first)")
int ldso_ba_remove_frame(ldso_ba_t *H, int frame_idx) {
    REQ_EDIT("ldso_ba_remove_frame");
    REQ(frame_idx >= 0 && frame_idx < H->edit.oF && !H->edit.frameGone[frame_idx], "ldso_ba_remove_frame: not a frame of the resident window");
    H->edit.frameGone[frame_idx] = 1;
    for (int r = 0; r < H->edit.oP; r++) { if (H->h_phost[r] == frame_idx) H->edit.rowGone[r] = 1; H->edit.mask[r] &= ~(1u << frame_idx); }
    return LDSO_OK;
}
int ldso_ba_insert_frame(ldso_ba_t *H, int image_slot, int *frame_id_out) {
    REQ_EDIT("ldso_ba_insert_frame");
    REQ(image_slot >= 0 && image_slot < H->maxF && H->imgSlots[image_slot] != nullptr, "ldso_ba_insert_frame: image slot not set");
    REQ(H->edit.oF + (int) H->edit.insertedSlots.size() < 32, "ldso_ba_insert_frame: too many frames in one edit");
    if (frame_id_out) *frame_id_out = H->edit.oF + (int) H->edit.insertedSlots.size();
    H->edit.insertedSlots.push_back(image_slot);
    return LDSO_OK;
}
int ldso_ba_remove_points(ldso_ba_t *H, int n, const int32_t *rows) {
    REQ_EDIT("ldso_ba_remove_points");
    REQ(n >= 0 && (n == 0 || rows), "ldso_ba_remove_points: bad arguments");
    for (int i = 0; i < n; i++) REQ(rows[i] >= 0 && rows[i] < H->edit.oP, "ldso_ba_remove_points: row out of range");
    for (int i = 0; i < n; i++) H->edit.rowGone[rows[i]] = 1;
    return LDSO_OK;
}
static int edit_residuals(ldso_ba *H, int n, const int32_t *rows, const int32_t *targets, bool add, const char *) {
    const int nF = H->edit.oF + (int) H->edit.insertedSlots.size();
    for (int i = 0; i < n; i++) {
        REQ(rows[i] >= 0 && rows[i] < H->edit.oP && targets[i] >= 0 && targets[i] < nF, "residual edit: row / target out of range");
        const bool has = (H->edit.mask[rows[i]] >> targets[i]) & 1u;
        REQ(add ? (!has && targets[i] != H->h_phost[rows[i]] && (targets[i] >= H->edit.oF || !H->edit.frameGone[targets[i]])) : has,
            add ? "ldso_ba_add_residuals: the point already has that residual, or the target is its host / a removed frame" : "ldso_ba_drop_residuals: the point has no such residual");
    }
    for (int i = 0; i < n; i++) { if (add) H->edit.mask[rows[i]] |= 1u << targets[i]; else H->edit.mask[rows[i]] &= ~(1u << targets[i]); }
    return LDSO_OK;
}
int ldso_ba_drop_residuals(ldso_ba_t *H, int n, const int32_t *rows, const int32_t *targets) {
    REQ_EDIT("ldso_ba_drop_residuals");
    REQ(n >= 0 && (n == 0 || (rows && targets)), "ldso_ba_drop_residuals: bad arguments");
    return edit_residuals(H, n, rows, targets, false, "");
}
int ldso_ba_add_residuals(ldso_ba_t *H, int n, const int32_t *rows, const int32_t *targets) {
    REQ_EDIT("ldso_ba_add_residuals");
    REQ(n >= 0 && (n == 0 || (rows && targets)), "ldso_ba_add_residuals: bad arguments");
    return edit_residuals(H, n, rows, targets, true, "");
}
int ldso_ba_add_points(ldso_ba_t *H, int n, const ldso_point_t *pts, const int32_t *before_row, int n_res, const ldso_residual_t *res, const float *mrb, const int32_t *ngr) {
    REQ_EDIT("ldso_ba_add_points");
    REQ(n >= 0 && n_res >= 0 && (n == 0 || (pts && before_row)) && (n_res == 0 || res), "ldso_ba_add_points: bad arguments");
    const int nF = H->edit.oF + (int) H->edit.insertedSlots.size();
    const size_t first = H->edit.fresh.size();
    for (int i = 0; i < n; i++) {
        REQ(before_row[i] >= 0 && before_row[i] <= H->edit.oP && pts[i].host >= 0 && pts[i].host < nF, "ldso_ba_add_points: before_row / host out of range");
        ldso_ba::NewPoint q; q.p = pts[i]; q.before = before_row[i]; q.mrb = mrb ? mrb[i] : 0.0f; q.ngr = ngr ? ngr[i] : 0;
        H->edit.fresh.push_back(q);
    }
    for (int i = 0; i < n_res; i++) {
        if (!(res[i].point >= 0 && res[i].point < n && res[i].target >= 0 && res[i].target < nF && !res[i].is_linearized)) {
            H->edit.fresh.resize(first); ldso_set_error("ldso_ba_add_points: residual names a point / frame outside the call, or is linearised"); return LDSO_E_INVALID;
        }
        H->edit.fresh[first + res[i].point].res.push_back(res[i]);
    }
    return LDSO_OK;
}
int ldso_ba_window_commit(ldso_ba_t *H) {
    REQ_EDIT("ldso_ba_window_commit");
    ldso_ba::WindowEdit &E = H->edit;
    const int nIns = (int) E.insertedSlots.size();
    std::vector<int32_t> idToNew(E.oF + nIns, -1), frameFrom, slots;
    for (int f = 0; f < E.oF; f++) if (!E.frameGone[f]) { idToNew[f] = (int) frameFrom.size(); frameFrom.push_back(f); slots.push_back(H->imageSlot[f]); }
    for (int k = 0; k < nIns; k++) { idToNew[E.oF + k] = (int) frameFrom.size(); frameFrom.push_back(-1); slots.push_back(E.insertedSlots[k]); }
    const int F = (int) frameFrom.size();
    auto translate = [&](uint32_t m) { uint32_t o = 0; for (int f = 0; f < E.oF + nIns; f++) if (((m >> f) & 1u) && idToNew[f] >= 0) o |= 1u << idToNew[f]; return o; };
    // fresh points in front of their rows, in call order (stable)
    std::vector<int> order(E.fresh.size());
    for (size_t i = 0; i < order.size(); i++) order[i] = (int) i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return E.fresh[a].before < E.fresh[b].before; });
    std::vector<int32_t> pointFrom; std::vector<uint32_t> mask; std::vector<ldso_point_t> fp; std::vector<ldso_residual_t> fr; std::vector<float> fm; std::vector<int32_t> fg;
    size_t nx = 0;
    int rc = LDSO_OK;
    auto emitFresh = [&](int idx) {
        ldso_ba::NewPoint q = E.fresh[idx];
        const int k = (int) fp.size();
        if (idToNew[q.p.host] < 0) { rc = LDSO_E_INVALID; return; }
        q.p.host = idToNew[q.p.host];
        uint32_t m = 0;
        for (ldso_residual_t &r : q.res) { if (idToNew[r.target] < 0) { rc = LDSO_E_INVALID; return; } r.target = idToNew[r.target]; r.host = q.p.host; r.point = k; m |= 1u << r.target; }
        std::sort(q.res.begin(), q.res.end(), [](const ldso_residual_t &a, const ldso_residual_t &b) { return a.target < b.target; });
        fp.push_back(q.p); fm.push_back(q.mrb); fg.push_back(q.ngr);
        for (const ldso_residual_t &r : q.res) fr.push_back(r);
        pointFrom.push_back(-1 - k); mask.push_back(m);
    };
    for (int r = 0; r <= E.oP; r++) {
        while (nx < order.size() && E.fresh[order[nx]].before == r) emitFresh(order[nx++]);
        if (r < E.oP && !E.rowGone[r]) { pointFrom.push_back(r); mask.push_back(translate(E.mask[r])); }
    }
    E.active = false;
    if (rc != LDSO_OK) { ldso_set_error("ldso_ba_window_commit: a fresh point or residual names a removed frame"); return rc; }
    REQ(!pointFrom.empty() && F >= 2, "ldso_ba_window_commit: the edit leaves no window");
    return ldso_ba_update_window(H, F, slots.data(), frameFrom.data(), (int) pointFrom.size(), pointFrom.data(), mask.data(), (int) fp.size(), fp.data(), (int) fr.size(), fr.data(), fm.data(), fg.data());
}

// Points per workgroup of the fused linearisation.  0 (default): the smallest chunk that keeps ONE window's grid within one workgroup per CU
// (latency of a single window).  n > 0 (multiple of 4): fixed chunks of n points - what ldso_ba_batch_create applies to its windows, where
// the launch is filled by many windows and a workgroup's fixed costs (operand staging, block reduction) should be spread over more points.
// The fp32 partial sums of the top Hessian are formed per chunk: two handles agree bit for bit only under the same chunking.
int ldso_ba_set_chunk_points(ldso_ba_t *H, int points_per_workgroup) {
    REQ(H && points_per_workgroup >= 0 && points_per_workgroup % 4 == 0 && points_per_workgroup <= 1024, "ldso_ba_set_chunk_points: 0 or a multiple of 4 up to 1024");
    REQ(!H->pendingApply, "ldso_ba_set_chunk_points: a linearisation is pending (ldso_ba_apply_res first)");
    H->chunkPoints = points_per_workgroup;
    if (H->D.P > 0) { CHK(hipSetDevice(H->device)); return rechunk(H); }
    return LDSO_OK;
}
// K-splits (workgroups) per 16 x 16 tile of the Schur complement in the GN fast path of THIS handle: the fp32 partial sums of a tile are formed per split, so two runs
// agree bit for bit only under the same number (a batch uses ldso_ba_batch_reduce_splits; default LD_SCT_KS = 8).  Takes effect with the next reduction.
int ldso_ba_set_reduce_splits(ldso_ba_t *H, int splits) {
    REQ(H && splits >= 1 && splits <= 16, "ldso_ba_set_reduce_splits: bad arguments");
    REQ(!H->inBatch, "ldso_ba_set_reduce_splits: the handle is part of a batch");
    H->reduceSplits = splits; H->D.ks = splits;
    return LDSO_OK;
}

int ldso_ba_get_chunk_cuts(ldso_ba_t *H, int32_t *ends, int cap, int *n_out) {
    REQ(H && n_out && H->D.P > 0, "ldso_ba_get_chunk_cuts: bad arguments / no window");
    const int n = (int) H->h_blocks.size();
    *n_out = n;
    if (ends) { REQ(cap >= n, "ldso_ba_get_chunk_cuts: buffer too small"); for (int i = 0; i < n; i++) ends[i] = H->h_blocks[i].p0 + H->h_blocks[i].np; }
    return LDSO_OK;
}
int ldso_ba_set_chunk_cuts(ldso_ba_t *H, const int32_t *ends, int n) {
    REQ(H && n >= 0 && (n == 0 || ends), "ldso_ba_set_chunk_cuts: bad arguments");
    REQ(!H->pendingApply, "ldso_ba_set_chunk_cuts: a linearisation is pending (ldso_ba_apply_res first)");
    REQ(H->inBatch == nullptr, "ldso_ba_set_chunk_cuts: the handle belongs to a batch (its chunks are the batch's)");
    for (int i = 0; i < n; i++) REQ(ends[i] > (i ? ends[i - 1] : 0) && ends[i] <= (H->D.P > 0 ? H->D.P : H->maxP), "ldso_ba_set_chunk_cuts: ends must ascend and stay inside the window");
    H->chunkCuts.assign(ends, ends + n);
    if (H->D.P > 0) { CHK(hipSetDevice(H->device)); return rechunk(H); }
    return LDSO_OK;
}
int ldso_ba_get_chunk_points(ldso_ba_t *H, int *points_per_workgroup, int *workgroups) {
    REQ(H && points_per_workgroup, "ldso_ba_get_chunk_points: null argument");
    *points_per_workgroup = H->chunkPoints;
    if (workgroups) *workgroups = H->D.nChunks;
    return LDSO_OK;
}

int ldso_ba_set_shard(ldso_ba_t *H, int pb, int pe) {
    REQ(H && pb >= 0 && pe >= pb && pe <= H->D.P, "ldso_ba_set_shard: bad range");
    H->D.pBegin = pb; H->D.pEnd = pe;
    return build_chunks(H);
}

}  // extern "C"
