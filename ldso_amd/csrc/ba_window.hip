// ba_window.hip — the window of a handle: upload through the staging arena (ldso_ba_set_window), the delta against the resident window
// (ldso_ba_update_window and the edit API that records one), the flattening into chunks.
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
__global__ __launch_bounds__(256) void k_point_stats(PtRec *__restrict__ a, PtRec *__restrict__ b, const float *__restrict__ mrb, const int32_t *__restrict__ ngr, int P) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    const float m = mrb[i]; const int32_t g = ngr[i];
    a[i].maxRelBS = m; a[i].numGood = g; b[i].maxRelBS = m; b[i].numGood = g;
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
};
__global__ __launch_bounds__(256) void k_win_rebuild(WinDelta W) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= W.P * W.FS) return;
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

// host side of the arena: reserve (16-byte aligned) room, remember where it goes
struct WinStage {
    char *base; size_t cap, used; WinXfer *tab; int n;
    template <class T> T *put(T *dst, size_t count) {          // room for `count` elements that will land at dst; returns where to write them
        const size_t bytes = (count * sizeof(T) + 15) & ~(size_t) 15;
        if (n >= LD_XFER_MAX || used + bytes > cap) return nullptr;
        T *p = reinterpret_cast<T *>(base + used);
        if (count) { tab[n].dst = dst; tab[n].src = used; tab[n].words = count * sizeof(T) / 4; n++; }
        used += bytes;
        return p;
    }
    template <class T> T *raw(size_t count) {          // room without a destination (operands of k_win_rebuild)
        const size_t bytes = (count * sizeof(T) + 15) & ~(size_t) 15;
        if (used + bytes > cap) return nullptr;
        T *p = reinterpret_cast<T *>(base + used);
        used += bytes;
        return p;
    }
    template <class T> bool again(T *dst, const T *staged, size_t count) {      // the same staged data to a second destination
        if (n >= LD_XFER_MAX) return false;
        if (count) { tab[n].dst = dst; tab[n].src = (size_t) (reinterpret_cast<const char *>(staged) - base); tab[n].words = count * sizeof(T) / 4; n++; }
        return true;
    }
    template <class T> bool zero(T *dst, size_t count) {
        if (n >= LD_XFER_MAX) return false;
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

int build_chunks(ldso_ba *H) {
    // host-major chunks over the local shard [pBegin,pEnd)
    BaDims &D = H->D;
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
    std::vector<int32_t> p0, cn, ch, cs(D.F + 1, 0);
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
    D.nChunks = (int) p0.size();
    H2D(H->B.chunk_p0, p0); H2D(H->B.chunk_n, cn); H2D(H->B.chunk_host, ch); H2D(H->d_chunkStart, cs);
    H->h_blocks.resize(p0.size());
    for (size_t i = 0; i < p0.size(); i++) H->h_blocks[i] = BatchBlock{0, p0[i], cn[i], ch[i] | ((int32_t) i << 8)};
    CHK(hipMemcpyAsync(H->d_blocks, H->h_blocks.data(), p0.size() * sizeof(BatchBlock), hipMemcpyHostToDevice, H->stream));
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

extern "C" {

int ldso_ba_set_window(ldso_ba_t *H, int F, const int32_t *image_slot, int P, const ldso_point_t *pts, int R, const ldso_residual_t *res,
                       const ldso_rawjac_t *linJ, const float *lin_rtz) {
    REQ(H && image_slot && pts && res, "ldso_ba_set_window: null argument");
    REQ(F >= 2 && F <= H->maxF && P >= 1 && P <= H->maxP && R >= 0, "ldso_ba_set_window: window exceeds the handle's capacity");
    CHK(hipSetDevice(H->device));
    BaDims &D = H->D;
    BaPtrs &B = H->B;
    // a call that fails half way (bad indices, allocation) must not leave the dimensions of the NEW window over the data of the old one:
    // the handle then holds no window (every entry point that needs one says so)
    struct WinGuard { ldso_ba *H; bool ok; ~WinGuard() { if (!ok) { H->D.P = 0; H->D.R = 0; H->R = 0; H->appliedValid = false; H->itemValid = false; } } } guard{H, false};
    D.F = F; D.FS = (F + 7) / 8 * 8; D.P = P; D.R = R; D.n = 8 * F + 4; D.GS = 8 * D.FS + LD_GEXTRA; D.w = H->w; D.h = H->h; D.nsg = D.FS / 8; D.ks = H->reduceSplits;
    D.pBegin = 0; D.pEnd = P; D.wM3G = (float) (H->w - 3); D.hM3G = (float) (H->h - 3);
    H->GSP = (D.GS + 15) / 16 * 16;
    H->R = R;
    H->imageSlot.assign(image_slot, image_slot + F);
    for (int f = 0; f < F; f++) {
        REQ(image_slot[f] >= 0 && image_slot[f] < H->maxF && H->imgSlots[image_slot[f]] != nullptr, "ldso_ba_set_window: image slot not set");
        B.img[f] = H->imgSlots[image_slot[f]];
    }
    const int FS = D.FS;
    const size_t PS = (size_t) P * FS;
    // ---- staging arena: everything the window needs goes over PCIe in ONE copy and is distributed (or zero-filled) by ONE kernel ----
    size_t nLin = 0;
    for (int i = 0; i < R; i++) nLin += res[i].is_linearized ? 1 : 0;
    REQ(nLin == 0 || (linJ && lin_rtz), "ldso_ba_set_window: linearised residual without linJ / lin_res_toZeroF");
    auto A16 = [](size_t b) { return (b + 15) & ~(size_t) 15; };
    const size_t tabBytes = A16(LD_XFER_MAX * sizeof(WinXfer));
    const size_t need = tabBytes + A16((size_t) P * sizeof(PtGeo)) + A16((size_t) P * 8 * sizeof(PtCw)) + A16((size_t) P * 4) + A16(PS * sizeof(SlotTab)) + A16(nLin * sizeof(ldso_rawjac_t)) + A16(nLin * 32)
                      + A16(PS * sizeof(SlotRec)) + 64;
    if (need > H->stageCap) {
        CHK(hipStreamSynchronize(H->stream));
        if (H->h_stage) hipHostFree(H->h_stage);
        if (H->d_stage) hipFree(H->d_stage);
        H->h_stage = nullptr; H->d_stage = nullptr; H->stageCap = 0;
        const size_t cap = need + need / 4;
        CHK(hipHostMalloc((void **) &H->h_stage, cap));
        CHK(hipMalloc((void **) &H->d_stage, cap));
        H->stageCap = cap;
    }
    if (H->stageBusy) { CHK(hipStreamSynchronize(H->stream)); H->stageBusy = false; }
    WinStage W{H->h_stage, H->stageCap, tabBytes, reinterpret_cast<WinXfer *>(H->h_stage), 0};
    PtGeo *geo = W.put(B.pgeo, P);
    PtCw *pcw = W.put(B.pcw, (size_t) P * 8);
    int32_t *phost = W.put(B.phost, P);
    SlotTab *tab = W.put(B.rtab, PS);
    ldso_rawjac_t *Jl = W.put(B.Jlin, nLin);
    float *rtz = W.put(B.rtz, nLin * 8);
    SlotRec *sr = W.put(H->sets[0].slot, PS);
    REQ(geo && pcw && phost && tab && Jl && rtz && sr, "ldso_ba_set_window: staging arena too small (internal)");
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
    bool okT = W.again(H->sets[1].slot, sr, PS);
    for (int s_ = 0; s_ < 2; s_++) {
        ResSet &S = H->sets[s_];
        okT = okT && W.zero(S.pt, (size_t) P) && W.zero(S.acc, (size_t) P) && W.zero(S.G, (size_t) P * D.GS);
    }
    // a new window has a new dimension 8F+4: the marginalisation prior starts at zero (ldso_ba_set_prior follows when there is one)
    okT = okT && W.zero(B.HM, (size_t) D.n * D.n) && W.zero(B.bM, (size_t) D.n) && W.zero(B.scalars, (size_t) 16)
              && W.zero(B.scPart, (size_t) LD_SC_SPLITS * H->GSP * H->GSP);
    REQ(okT, "ldso_ba_set_window: upload table overflow (internal)");
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
    REQ(H && image_slot && frame_from && point_from && res_mask, "ldso_ba_update_window: null argument");
    REQ(H->D.P > 0 && !H->pendingApply, "ldso_ba_update_window: no resident window, or a linearisation is pending (ldso_ba_apply_res first)");
    REQ(!H->hasL, "ldso_ba_update_window: the resident window holds linearised residuals (use ldso_ba_set_window)");
    REQ(H->D.pBegin == 0 && H->D.pEnd == H->D.P, "ldso_ba_update_window: sharded window");
    REQ(F >= 2 && F <= H->maxF && P >= 1 && P <= H->maxP && n_fresh >= 0 && n_fresh_res >= 0, "ldso_ba_update_window: window exceeds the handle's capacity");
    REQ(n_fresh == 0 || (fresh && fresh_mrb && fresh_ngr), "ldso_ba_update_window: fresh points without records");
    REQ(n_fresh_res == 0 || fresh_res, "ldso_ba_update_window: fresh residuals without records");
    CHK(hipSetDevice(H->device));
    const BaDims oD = H->D;
    const int FS = (F + 7) / 8 * 8;
    const size_t PS = (size_t) P * FS;
    // ---- validate the delta on the host (indices only; nothing of the resident data is read back) ----
    {
        std::vector<char> seen(oD.F, 0);
        for (int f = 0; f < F; f++) {
            REQ(frame_from[f] >= -1 && frame_from[f] < oD.F, "ldso_ba_update_window: frame_from out of range");
            if (frame_from[f] >= 0) { REQ(!seen[frame_from[f]], "ldso_ba_update_window: an old frame appears twice"); seen[frame_from[f]] = 1; }
            REQ(f == 0 || frame_from[f] < 0 || frame_from[f - 1] < frame_from[f], "ldso_ba_update_window: surviving frames must keep their order, inserted frames come last");
            REQ(image_slot[f] >= 0 && image_slot[f] < H->maxF && H->imgSlots[image_slot[f]] != nullptr, "ldso_ba_update_window: image slot not set");
        }
    }
    std::vector<int32_t> resBegin((size_t) P + 1), freshResBegin((size_t) n_fresh + 1, 0), newHost((size_t) P);
    {
        std::vector<int32_t> oldToNew(oD.F, -1);
        for (int f = 0; f < F; f++) if (frame_from[f] >= 0) oldToNew[frame_from[f]] = f;
        int lastOld = -1, nextFresh = 0, acc = 0;
        const uint32_t fmask = (F >= 32) ? 0xFFFFFFFFu : ((1u << F) - 1u);
        for (int k = 0; k < n_fresh; k++) freshResBegin[k + 1] = 0;
        int fr = 0;
        for (int i = 0; i < P; i++) {
            const int from = point_from[i];
            int host;
            if (from >= 0) {
                REQ(from < oD.P && from > lastOld, "ldso_ba_update_window: surviving points must keep their order");
                lastOld = from;
                host = oldToNew[H->h_phost[from]];
                REQ(host >= 0, "ldso_ba_update_window: a surviving point is hosted by a frame that left the window");
            } else {
                REQ(-1 - from == nextFresh && nextFresh < n_fresh, "ldso_ba_update_window: fresh points must be numbered in window order");
                host = fresh[nextFresh].host;
                REQ(host >= 0 && host < F, "ldso_ba_update_window: fresh point host out of range");
                const int cnt = __builtin_popcount(res_mask[i]);
                freshResBegin[nextFresh] = fr;
                for (int c = 0; c < cnt; c++) {
                    REQ(fr < n_fresh_res && fresh_res[fr].target >= 0 && fresh_res[fr].target < F && fresh_res[fr].host == host,
                        "ldso_ba_update_window: fresh residual names a target outside the window or another host than its point's");
                    REQ(fresh_res[fr].point == nextFresh && !fresh_res[fr].is_linearized && ((res_mask[i] >> fresh_res[fr].target) & 1u)
                        && (c == 0 || fresh_res[fr - 1].target < fresh_res[fr].target), "ldso_ba_update_window: fresh residuals must be point-major, target-ascending and match res_mask");
                    fr++;
                }
                nextFresh++;
            }
            REQ((res_mask[i] & ~fmask) == 0 && !((res_mask[i] >> host) & 1u), "ldso_ba_update_window: res_mask names a frame outside the window or the host itself");
            REQ(i == 0 || newHost[i - 1] <= host, "ldso_ba_update_window: points must be ordered by host frame (EnergyFunctional::allPoints order)");
            newHost[i] = host;
            resBegin[i] = acc; acc += __builtin_popcount(res_mask[i]);
        }
        resBegin[P] = acc;
        freshResBegin[n_fresh] = fr;
        REQ(nextFresh == n_fresh && fr == n_fresh_res, "ldso_ba_update_window: unused fresh points / residuals");
    }
    const int R = resBegin[P];
    // ---- arena: [table | delta | image]; only table + delta cross PCIe ----
    auto A16 = [](size_t b) { return (b + 15) & ~(size_t) 15; };
    const size_t tabBytes = A16(LD_XFER_MAX * sizeof(WinXfer));
    const size_t deltaBytes = A16((size_t) F * 4) + 2 * A16((size_t) P * 4) + A16(((size_t) P + 1) * 4) + A16((size_t) n_fresh * sizeof(ldso_point_t)) + A16((size_t) n_fresh_res * sizeof(ldso_residual_t))
                              + A16(((size_t) n_fresh + 1) * 4) + 2 * A16((size_t) n_fresh * 4);
    const size_t need = tabBytes + deltaBytes + A16((size_t) P * sizeof(PtGeo)) + A16((size_t) P * 8 * sizeof(PtCw)) + A16((size_t) P * 4) + A16(PS * sizeof(SlotTab)) + A16(PS * sizeof(SlotRec))
                        + 2 * A16((size_t) P * 4) + 64;
    if (need > H->stageCap) {          // the arena only ever holds staging data: growing it loses nothing of the resident window
        CHK(hipStreamSynchronize(H->stream));
        if (H->h_stage) hipHostFree(H->h_stage);
        if (H->d_stage) hipFree(H->d_stage);
        H->h_stage = nullptr; H->d_stage = nullptr; H->stageCap = 0; H->stageBusy = false;
        const size_t cap = need + need / 4;
        CHK(hipHostMalloc((void **) &H->h_stage, cap));
        CHK(hipMalloc((void **) &H->d_stage, cap));
        H->stageCap = cap;
    }
    if (H->stageBusy) { CHK(hipStreamSynchronize(H->stream)); H->stageBusy = false; }
    WinStage W{H->h_stage, H->stageCap, tabBytes, reinterpret_cast<WinXfer *>(H->h_stage), 0};
    int32_t *hFrameFrom = W.raw<int32_t>(F), *hPointFrom = W.raw<int32_t>(P);
    uint32_t *hMask = W.raw<uint32_t>(P);
    int32_t *hResBegin = W.raw<int32_t>((size_t) P + 1);
    ldso_point_t *hFresh = W.raw<ldso_point_t>(n_fresh);
    ldso_residual_t *hFreshRes = W.raw<ldso_residual_t>(n_fresh_res);
    int32_t *hFreshResBegin = W.raw<int32_t>((size_t) n_fresh + 1);
    float *hMrb = W.raw<float>(n_fresh); int32_t *hNgr = W.raw<int32_t>(n_fresh);
    REQ(hFrameFrom && hPointFrom && hMask && hResBegin && hFresh && hFreshRes && hFreshResBegin && hMrb && hNgr, "ldso_ba_update_window: staging arena too small (internal)");
    const size_t upBytes = W.used;
    memcpy(hFrameFrom, frame_from, (size_t) F * 4); memcpy(hPointFrom, point_from, (size_t) P * 4); memcpy(hMask, res_mask, (size_t) P * 4);
    memcpy(hResBegin, resBegin.data(), ((size_t) P + 1) * 4); memcpy(hFreshResBegin, freshResBegin.data(), ((size_t) n_fresh + 1) * 4);
    if (n_fresh) { memcpy(hFresh, fresh, (size_t) n_fresh * sizeof(ldso_point_t)); memcpy(hMrb, fresh_mrb, (size_t) n_fresh * 4); memcpy(hNgr, fresh_ngr, (size_t) n_fresh * 4); }
    if (n_fresh_res) memcpy(hFreshRes, fresh_res, (size_t) n_fresh_res * sizeof(ldso_residual_t));
    BaPtrs &B = H->B;
    // the image region: same destinations, same order, same zero fills as ldso_ba_set_window
    PtGeo *geo = W.put(B.pgeo, P);
    PtCw *pcw = W.put(B.pcw, (size_t) P * 8);
    int32_t *phost = W.put(B.phost, P);
    SlotTab *tab = W.put(B.rtab, PS);
    SlotRec *sr = W.put(H->sets[0].slot, PS);
    REQ(geo && pcw && phost && tab && sr, "ldso_ba_update_window: staging arena too small (internal)");
    float *mrb = W.raw<float>(P); int32_t *ngr = W.raw<int32_t>(P);
    REQ(mrb && ngr, "ldso_ba_update_window: staging arena too small (internal)");
    auto dev = [&](const void *hp) { return H->d_stage + (reinterpret_cast<const char *>(hp) - H->h_stage); };
    WinDelta Wd;
    const ResSet &So = H->sets[H->cur];
    Wd.oGeo = B.pgeo; Wd.oPcw = B.pcw; Wd.oHost = B.phost; Wd.oTab = B.rtab; Wd.oSlot = So.slot; Wd.oPt = So.pt; Wd.oF = oD.F; Wd.oFS = oD.FS; Wd.oP = oD.P;
    Wd.frameFrom = (const int32_t *) dev(hFrameFrom); Wd.pointFrom = (const int32_t *) dev(hPointFrom); Wd.resMask = (const uint32_t *) dev(hMask); Wd.resBegin = (const int32_t *) dev(hResBegin);
    Wd.fresh = (const ldso_point_t *) dev(hFresh); Wd.freshRes = (const ldso_residual_t *) dev(hFreshRes); Wd.freshResBegin = (const int32_t *) dev(hFreshResBegin);
    Wd.freshMrb = (const float *) dev(hMrb); Wd.freshNgr = (const int32_t *) dev(hNgr);
    Wd.F = F; Wd.FS = FS; Wd.P = P;
    Wd.geo = (PtGeo *) dev(geo); Wd.pcw = (PtCw *) dev(pcw); Wd.phost = (int32_t *) dev(phost); Wd.tab = (SlotTab *) dev(tab); Wd.sr = (SlotRec *) dev(sr); Wd.mrb = (float *) dev(mrb); Wd.ngr = (int32_t *) dev(ngr);
    // from here on the handle describes the new window (a failure leaves it without one, as in ldso_ba_set_window)
    struct WinGuard { ldso_ba *H; bool ok; ~WinGuard() { if (!ok) { H->D.P = 0; H->D.R = 0; H->R = 0; H->appliedValid = false; H->itemValid = false; } } } guard{H, false};
    BaDims &D = H->D;
    D.F = F; D.FS = FS; D.P = P; D.R = R; D.n = 8 * F + 4; D.GS = 8 * D.FS + LD_GEXTRA; D.w = H->w; D.h = H->h; D.nsg = D.FS / 8; D.ks = H->reduceSplits;
    D.pBegin = 0; D.pEnd = P; D.wM3G = (float) (H->w - 3); D.hM3G = (float) (H->h - 3); D.nL = 0;
    H->GSP = (D.GS + 15) / 16 * 16;
    H->R = R;
    H->imageSlot.assign(image_slot, image_slot + F);
    for (int f = 0; f < F; f++) B.img[f] = H->imgSlots[image_slot[f]];
    H->h_phost.assign(newHost.begin(), newHost.end());
    H->flat2slot.assign(R, -1);
    for (int i = 0; i < P; i++) { int k = resBegin[i]; for (int t = 0; t < F; t++) if ((res_mask[i] >> t) & 1u) H->flat2slot[k++] = (int32_t) ((size_t) i * FS + t); }
    H->hasL = false; H->cur = 0; H->pendingApply = false; H->appliedValid = false; H->itemValid = false;
    bool okT = W.again(H->sets[1].slot, sr, PS);
    for (int s_ = 0; s_ < 2; s_++) {
        ResSet &S = H->sets[s_];
        okT = okT && W.zero(S.pt, (size_t) P) && W.zero(S.acc, (size_t) P) && W.zero(S.G, (size_t) P * D.GS);
    }
    okT = okT && W.zero(B.HM, (size_t) D.n * D.n) && W.zero(B.bM, (size_t) D.n) && W.zero(B.scalars, (size_t) 16) && W.zero(B.scPart, (size_t) LD_SC_SPLITS * H->GSP * H->GSP);
    REQ(okT, "ldso_ba_update_window: upload table overflow (internal)");
    H->hasPrior = false;
    CHK(hipMemcpyAsync(H->d_stage, H->h_stage, upBytes, hipMemcpyHostToDevice, H->stream));
    hipLaunchKernelGGL(k_win_rebuild, dim3((unsigned) ((PS + 255) / 256)), dim3(256), 0, H->stream, Wd);
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
