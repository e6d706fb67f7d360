// ---- batched windows: B independent windows per launch ---------------------------------------------------------------------------
// One 7-keyframe window is tiny for an MI355X (SURVEY 7 hard part 1, 8e): a batch runs the Gauss-Newton iteration of several
// independent windows (several agents / sequences / hypotheses) with three launches per iteration for ALL of them: k_reduce_batch
// (every window's reduce workgroups) -> k_gn_solve_batch (two control workgroups per window) -> k_linearize_batch (every window's
// chunks).  Per-window arithmetic is exactly that of ldso_ba_enqueue_gn's split schedule; the windows only share the launches.
// Behind optimize(), the key frame's two marginalisations for the whole batch: k_linearize_batch_marg -> k_reduce_batch_marg -> k_marg_gather_update_batch
// (ldso_ba_batch_marginalize_points) and k_marg_frame_batch (ldso_ba_batch_marginalize_frame), per window the arithmetic of the single-window entries.  The step behind
// them, activatePointsMT for the batch (ldso_ba_batch_activate_points / _select_candidates / _select_activate_points), lives in act_select.hip beside the selection's buffers, and
// the step that closes the loop - every window becomes its next one (ldso_ba_batch_update_windows / _set_frames) - in ba_window.hip beside the single-window update it shares its
// pieces with; the chunk policy it re-runs is batch_chunk_policy here.
#include "ba_host.h"

// a device table of the batch (d_blocks, d_wg) with room for `n` elements: one that is too small is replaced once both streams, whose launches read it, have drained
template <class T> static int grow_table(ldso_ba_batch *Bt, T *&d, size_t &cap, size_t n) {
    if (n <= cap) return LDSO_OK;
    CHK(hipStreamSynchronize(Bt->h[0]->stream));
    if (Bt->aux) CHK(hipStreamSynchronize(Bt->aux));
    if (d) (void) hipFree(d);
    d = nullptr; cap = 0;
    CHK(hipMalloc((void **) &d, n * sizeof(T)));
    cap = n;
    return LDSO_OK;
}
int batch_refresh(ldso_ba_batch *Bt) {
    REQ(!Bt->lost, "ldso_ba_batch: a ldso_ba_batch_update_windows that failed behind its validation left windows of the batch unset: destroy and re-create the batch");
    ldso_ba *H0 = Bt->h[0];
    const size_t n = Bt->h.size();
    for (int pass = 0; pass < 2; pass++) {          // pass 0: blocks numbered over the whole batch; pass 1: per half
        int lin = 0, red = 0;
        for (size_t i = 0; i < n; i++) {
            ldso_ba *H = Bt->h[i];
            BatchItem &it = Bt->items[pass * n + i];
            if (pass == 1 && (int) i == Bt->n0) { Bt->halfChunks[0] = lin; Bt->halfReduce[0] = red; lin = 0; red = 0; }
            if (H->B.acc != H->ownAcc) H->B.acc = H->ownAcc;
            // the per-window parity: set[0] = the window's applied set, so the launches name the sets relative to it and windows at different parities share them
            fill_item(it, H, Bt->ks, true, (int) i);
            it.linBlock0 = lin; it.redBlock0 = red;
            lin += H->D.nChunks;
            red += reduce_grid(H->D.F, 0, Bt->ks, H->GSP).total;
        }
        if (pass == 0) { Bt->totalChunks = lin; Bt->totalReduce = red; }
        else if (Bt->n0 == (int) n) { Bt->halfChunks[0] = lin; Bt->halfReduce[0] = red; Bt->halfChunks[1] = 0; Bt->halfReduce[1] = 0; }
        else { Bt->halfChunks[1] = lin; Bt->halfReduce[1] = red; }
    }
    CHK(hipMemcpyAsync(Bt->d_items, Bt->items.data(), Bt->items.size() * sizeof(BatchItem), hipMemcpyHostToDevice, H0->stream));
    // the workgroup table: whole batch (window index into items[0..n)), then half A (index into items[n..n+n0)) and half B (items[n+n0..))
    Bt->blocks.clear();
    for (size_t i = 0; i < n; i++) for (const BatchBlock &b : Bt->h[i]->h_blocks) Bt->blocks.push_back(BatchBlock{(int32_t) i, b.p0, b.np, b.host_chunk});
    for (size_t i = 0; i < n; i++) { const int32_t w = (int) i < Bt->n0 ? (int32_t) i : (int32_t) i - Bt->n0; for (const BatchBlock &b : Bt->h[i]->h_blocks) Bt->blocks.push_back(BatchBlock{w, b.p0, b.np, b.host_chunk}); }
    RUN(grow_table(Bt, Bt->d_blocks, Bt->blocksCap, Bt->blocks.size()));
    CHK(hipMemcpyAsync(Bt->d_blocks, Bt->blocks.data(), Bt->blocks.size() * sizeof(BatchBlock), hipMemcpyHostToDevice, H0->stream));
    if (Bt->balanced) {
        // the per-workgroup block ranges of the three launches (whole batch | half A | half B), valid while the windows keep the chunks ldso_ba_batch_create cut
        bool ok = (int) Bt->wg[0].size() >= 2 && Bt->wg[0].back() == Bt->totalChunks && Bt->wg[1].back() == Bt->halfChunks[0] && (Bt->halfChunks[1] == 0 || Bt->wg[2].back() == Bt->halfChunks[1]);
        REQ(ok, "ldso_ba_batch: the windows of the batch were re-chunked behind its back (ldso_ba_set_window / ldso_ba_set_chunk_points on a member): destroy and re-create the batch");
        std::vector<int32_t> all;
        for (int u = 0; u < 3; u++) { Bt->wgOff[u] = all.size(); Bt->nWG[u] = Bt->wg[u].empty() ? 0 : (int) Bt->wg[u].size() - 1; all.insert(all.end(), Bt->wg[u].begin(), Bt->wg[u].end()); }
        RUN(grow_table(Bt, Bt->d_wg, Bt->wgCap, all.size()));
        Bt->wgHost.swap(all);
        CHK(hipMemcpyAsync(Bt->d_wg, Bt->wgHost.data(), Bt->wgHost.size() * sizeof(int32_t), hipMemcpyHostToDevice, H0->stream));
    }
    return LDSO_OK;
}

// Cut the windows [i0, i1) of a batch into chunks so that `nWG` workgroups, each working through a run of consecutive chunks, carry the same load.  A chunk
// (= one pass of linearize_body: operand staging, software-pipeline fill, block reduction) costs `c0` point-equivalents on top of its points, and never
// straddles a host frame.  The smallest per-workgroup budget that fits all points into nWG workgroups is found by bisection; cuts[i] receives the chunk ends
// of window i, wg the first chunk of every workgroup (nWG + 1 entries, counted over the windows [i0, i1) in order).
// The balancer proper, host logic without a device (C-ABI: ldso_ba_balance_chunks, tests/test_batch_balance_cpu.py): segments (runs of points that may share a chunk: one
// window's points of one host frame) in launch order -> chunk ends per segment (relative to the segment) and the first chunk of every workgroup.
struct BalSeg { int owner, p0, n; };
static long balance_segments(const std::vector<BalSeg> &segs, int nWG, int c0, std::vector<std::vector<int32_t>> *cutsByOwner, std::vector<int32_t> *wg, std::vector<int32_t> *flatEnds) {
    long total = 0;
    for (const BalSeg &sg : segs) total += sg.n;
    auto run = [&](long budget, bool emit) -> bool {
        size_t si = 0; int used = 0;          // points of segs[si] already handed out
        int blocks = 0;
        if (emit) { if (wg) wg->assign(1, 0); if (flatEnds) flatEnds->clear(); }
        for (int w = 0; w < nWG && si < segs.size(); w++) {
            long left = budget;
            while (si < segs.size()) {
                const int rem = segs[si].n - used;
                long can = left - c0;
                if (can < LD_WAVES && left != budget) break;          // not worth a chunk of its own here: the next workgroup takes it
                if (can < 1) can = 1;
                int take = (int) std::min<long>(rem, can);
                if (take < rem) { take = std::max(take / LD_WAVES * LD_WAVES, 1); if (rem - take < LD_WAVES) take = rem; }          // whole rounds of the workgroup's wavefronts, no crumbs left behind
                if (emit) {
                    if (cutsByOwner) (*cutsByOwner)[(size_t) segs[si].owner].push_back(segs[si].p0 + used + take);
                    if (flatEnds) flatEnds->push_back(segs[si].p0 + used + take);
                }
                blocks++; left -= c0 + take; used += take;
                if (used == segs[si].n) { si++; used = 0; }
                if (left <= 0) break;
            }
            if (emit && wg) wg->push_back(blocks);
        }
        if (emit && wg) while ((int) wg->size() < nWG + 1) wg->push_back(blocks);
        return si == segs.size();
    };
    long lo = std::max<long>(1, total / std::max(nWG, 1)), hi = total + (long) c0 * (long) segs.size() + 1;
    while (lo < hi) { const long mid = (lo + hi) / 2; if (run(mid, false)) hi = mid; else lo = mid + 1; }
    run(lo, true);
    return lo;
}
static void balance_batch(ldso_ba *const *handles, int i0, int i1, int nWG, int c0, std::vector<std::vector<int32_t>> &cuts, std::vector<int32_t> &wg) {
    std::vector<BalSeg> segs;
    for (int i = i0; i < i1; i++) {
        const ldso_ba *H = handles[i];
        cuts[i].clear();
        int p = 0;
        while (p < H->D.P) { int e = p; while (e < H->D.P && H->h_phost[e] == H->h_phost[p]) e++; segs.push_back(BalSeg{i, p, e - p}); p = e; }
    }
    balance_segments(segs, nWG, c0, &cuts, &wg, nullptr);
}
// Chunking of a batch: the launch is filled by all windows together, so a workgroup takes several points per wavefront (its fixed
// costs - operand staging, block reduction, ~4.5 us - are then a fraction of its life) while the grid still holds a few workgroups
// per CU for balance.  Handles with an explicit ldso_ba_set_chunk_points keep theirs.  Host logic on the windows' point counts and host
// runs (D.P, h_phost); ldso_ba_batch_create applies it with rechunk, ldso_ba_batch_update_windows re-runs it on the new windows.
void batch_chunk_policy(ldso_ba *const *handles, int n, BatchCuts &C) {
    ldso_ba *H0 = handles[0];
    C.balanced = false; C.CH = 0;
    C.cuts.assign((size_t) n, std::vector<int32_t>());
    for (int u = 0; u < 3; u++) C.wg[u].clear();
    long total = 0;
    for (int i = 0; i < n; i++) total += handles[i]->D.P;
    int ppw = (int) (total / ((long) H0->numCU * LD_WAVES));               // points per wavefront slot of the chip
    bool every = true;
    for (int i = 0; i < n; i++) every = every && handles[i]->chunkPoints == 0 && handles[i]->chunkCuts.empty();
    if (ppw > 1 && every) {
        // Round 6: every workgroup of a launch gets the SAME load.  With regular chunks the batched launch ran as ceil(chunks / CUs) rounds of equal
        // workgroups - 1344 on 256 CUs: the last round a quarter full - and every chunk paid its fixed costs (staging, pipeline fill, block reduction:
        // about two points per wavefront) for six points per wavefront.  Now one workgroup per CU and launch works through a run of chunks cut to measure.
        const int c0 = 2 * LD_WAVES;          // fixed cost of a chunk in points (two rounds of the workgroup's wavefronts)
        const int n0 = (n >= 4) ? n / 2 : n;
        // A half-batch launch does not take every CU: the other half's k_reduce_batch_dense / k_gn_solve_batch run beside it (two streams), and a workgroup that
        // owns its CU for the whole launch leaves them nothing to start on.  Measured (32 windows, MI355X): 128 / 192 / 208 / 224 / 240 / 256 workgroups per half
        // -> 141.6 / 159.2 / 162.2 / 168.3 / 167.7 / 149.5 k window-iterations/s (profiles/r06_batch_sweeps.log).
        const int nWG = (n >= 4) ? std::max(1, H0->numCU * 7 / 8) : H0->numCU;
        balance_batch(handles, 0, n0, nWG, c0, C.cuts, C.wg[1]);
        if (n0 < n) balance_batch(handles, n0, n, nWG, c0, C.cuts, C.wg[2]);
        // the whole-batch launch (ldso_ba_batch_time_linearize) runs the two halves' workgroups one after the other
        C.wg[0] = C.wg[1];
        if (n0 < n) for (size_t u = 1; u < C.wg[2].size(); u++) C.wg[0].push_back(C.wg[1].back() + C.wg[2][u]);
        C.balanced = true;
    } else {
        // regular chunks of up to 6 points per wavefront (round 4, B = 32: 122.0 / 139.3 / 128.6 k window-iterations/s at 4 / 6 / 8)
        ppw = ppw < 1 ? 1 : ppw > 6 ? 6 : ppw;
        C.CH = ppw > 1 ? ppw * LD_WAVES : 0;          // ppw == 1: the single-window chunking already is the right one
    }
}
// what ldso_ba_batch_chunk_points reports for windows cut by the policy: the regular chunk, or the rounded average of the balanced cuts
int batch_chunk_points(ldso_ba *const *handles, int n, const BatchCuts &C) {
    if (!C.balanced) return C.CH;
    long total = 0, chunks = 0;
    for (int i = 0; i < n; i++) { total += handles[i]->D.P; chunks += handles[i]->D.nChunks; }
    return (int) std::max<long>(1, (total + chunks / 2) / std::max<long>(chunks, 1));
}
extern "C" {

// host logic, no device: `n_seg` segments of seg_points[i] points each (in launch order; a chunk never spans two segments), `n_wg` workgroups, `chunk_cost` points of fixed
// cost per chunk -> chunk_end[] (cumulative over ALL points, ascending, the last one = the total), wg_first_chunk[n_wg + 1]; returns the number of chunks (< 0: error / cap too small)
int ldso_ba_balance_chunks(int n_seg, const int32_t *seg_points, int n_wg, int chunk_cost, int32_t *chunk_end, int cap, int32_t *wg_first_chunk, int64_t *budget_out) {
    REQ(n_seg >= 1 && seg_points && n_wg >= 1 && chunk_cost >= 0 && chunk_end && wg_first_chunk, "ldso_ba_balance_chunks: bad arguments");
    std::vector<BalSeg> segs;
    int p = 0;
    for (int i = 0; i < n_seg; i++) { REQ(seg_points[i] >= 1, "ldso_ba_balance_chunks: empty segment"); segs.push_back(BalSeg{0, p, seg_points[i]}); p += seg_points[i]; }
    std::vector<int32_t> wg, ends;
    const long budget = balance_segments(segs, n_wg, chunk_cost, nullptr, &wg, &ends);
    if ((int) ends.size() > cap) { ldso_set_error("ldso_ba_balance_chunks: chunk_end[] too small"); return LDSO_E_INVALID; }
    for (size_t i = 0; i < ends.size(); i++) chunk_end[i] = ends[i];
    for (int w = 0; w <= n_wg; w++) wg_first_chunk[w] = wg[(size_t) w];
    if (budget_out) *budget_out = budget;
    return (int) ends.size();
}

int ldso_ba_batch_create(ldso_ba_t *const *handles, int n, ldso_ba_batch_t **out) {
    REQ(handles && n >= 1 && out, "ldso_ba_batch_create: bad arguments");
    ldso_ba *H0 = handles[0];
    REQ(H0 && H0->D.P > 0, "ldso_ba_batch_create: window 0 is not set");
    for (int i = 0; i < n; i++) {
        ldso_ba *H = handles[i];
        REQ(H && H->D.P > 0, "ldso_ba_batch_create: every handle needs a resident window");
        REQ(H->device == H0->device && H->stream == H0->stream, "ldso_ba_batch_create: the handles of a batch share one device and one stream (ldso_ba_set_stream)");
        REQ(H->D.FS == H0->D.FS, "ldso_ba_batch_create: the windows of a batch use the same slot-table width (all F <= 8 or all 9 <= F <= 16)");
        REQ(H->inBatch == nullptr, "ldso_ba_batch_create: a handle belongs to at most one batch at a time");
        for (int k = 0; k < i; k++) REQ(handles[k] != H, "ldso_ba_batch_create: the same handle twice");
        REQ(!H->hasL, "ldso_ba_batch_create: windows with linearised residuals run on their own handle");
        REQ(H->D.pBegin == 0 && H->D.pEnd == H->D.P, "ldso_ba_batch_create: sharded handles cannot be batched");
        REQ(H->settings.forceAcceptStep && !H->pendingApply, "ldso_ba_batch_create: forced-accept schedule, no pending linearisation");
        REQ(memcmp(&H->settings, &H0->settings, sizeof(H0->settings)) == 0, "ldso_ba_batch_create: the batched kernels run with ONE ldso_settings_t: every handle of a batch must have been created with identical settings");
        // re-chunking re-forms a window's partial sums into its OTHER ping-pong set: the windows stay at one parity only if all of them are re-cut or none
        REQ(H->chunkPoints == H0->chunkPoints, "ldso_ba_batch_create: the handles of a batch share one chunking policy (ldso_ba_set_chunk_points: all automatic or all the same value)");
    }
    CHK(hipSetDevice(H0->device));
    // the chunk policy (batch_chunk_policy), applied: a window's applied state is re-formed under its new chunks (rechunk)
    BatchCuts cutsOf;
    batch_chunk_policy(handles, n, cutsOf);
    for (int i = 0; i < n; i++) {
        const int r_ = batch_cut_window(handles[i], i, cutsOf, false, rechunk);
        if (r_ != LDSO_OK) { for (int k = 0; k <= i; k++) { if (cutsOf.balanced) handles[k]->chunkCuts.clear(); rechunk(handles[k]); } return r_; }      // leave nobody with the batch's chunks
    }
    const int Bt_chunk = batch_chunk_points(handles, n, cutsOf);
    const bool balanced = cutsOf.balanced;
    const std::vector<int32_t> *wgTab = cutsOf.wg;
    ldso_ba_batch *Bt = new ldso_ba_batch();
    Bt->chunkPoints = Bt_chunk;
    Bt->balanced = balanced;
    for (int u = 0; u < 3; u++) Bt->wg[u] = wgTab[u];
    Bt->h.assign(handles, handles + n);
    Bt->items.resize(2 * (size_t) n);
    Bt->n0 = (n >= 4) ? n / 2 : n;
    // K-splits per Schur tile of the batched reduction: a lone window spreads every 16 x 16 tile of its Schur complement over LD_SCT_KS = 8 workgroups (latency); the
    // windows of a batch fill the chip anyway and halve the workgroups and the fp64 atomics (round 6, A/B on one box: 4 -> +3.3 % window-iterations/s at B = 32, 2 -> -11 %)
    Bt->ks = (n >= 4) ? 4 : LD_SCT_KS;
    Bt->FS = H0->D.FS;
    Bt->Dmax = H0->D;
    for (int i = 0; i < n; i++) if (handles[i]->D.F > Bt->Dmax.F) Bt->Dmax = handles[i]->D;
    void *q = nullptr;
    for (int i = 0; i < n; i++) handles[i]->inBatch = Bt;
    // every failure from here on goes through ldso_ba_batch_destroy: it restores the single-window chunking and releases the handles
    if (hipMalloc(&q, 2 * (size_t) n * sizeof(BatchItem)) != hipSuccess) { (void) hipGetLastError(); ldso_ba_batch_destroy(Bt); ldso_set_error("ldso_ba_batch_create: hipMalloc failed"); return LDSO_E_HIP; }
    Bt->d_items = (BatchItem *) q;
    const size_t scBytes = (size_t) n * 16 * sizeof(double);          // ldso_ba_batch_optimize reads every window's scalars back in one copy
    if (hipMalloc(&q, scBytes) != hipSuccess) { (void) hipGetLastError(); ldso_ba_batch_destroy(Bt); ldso_set_error("ldso_ba_batch_create: hipMalloc failed"); return LDSO_E_HIP; }
    Bt->d_scalars = (double *) q;
    if (hipHostMalloc(&q, scBytes, hipHostMallocDefault) != hipSuccess) { (void) hipGetLastError(); ldso_ba_batch_destroy(Bt); ldso_set_error("ldso_ba_batch_create: hipHostMalloc failed"); return LDSO_E_HIP; }
    Bt->h_scalars = (double *) q;
    if (Bt->n0 < n) {
        if (hipStreamCreateWithFlags(&Bt->aux, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&Bt->ev0, hipEventDisableTiming) != hipSuccess
            || hipEventCreateWithFlags(&Bt->ev1, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&Bt->evEnd, hipEventDisableTiming) != hipSuccess) {
            ldso_ba_batch_destroy(Bt); ldso_set_error("ldso_ba_batch_create: stream / event creation failed"); return LDSO_E_HIP;
        }
    }
    *out = Bt;
    return LDSO_OK;
}

// points per workgroup ldso_ba_batch_create chose for the windows of this batch (0: it left their single-window chunking alone)
// K-splits per Schur tile the batch reduces its windows with (see ldso_ba_set_reduce_splits)
int ldso_ba_batch_reduce_splits(ldso_ba_batch_t *Bt, int *splits) {
    REQ(Bt && splits, "ldso_ba_batch_reduce_splits: bad arguments");
    *splits = Bt->ks;
    return LDSO_OK;
}

int ldso_ba_batch_chunk_points(ldso_ba_batch_t *Bt, int *points_per_workgroup) {
    REQ(Bt && points_per_workgroup, "ldso_ba_batch_chunk_points: null argument");
    *points_per_workgroup = Bt->chunkPoints;
    return LDSO_OK;
}
// which of the policy's two modes the batch is in: 1 = balanced cuts (one workgroup per CU works through a run of chunks), 0 = regular chunks
int ldso_ba_batch_balanced(ldso_ba_batch_t *Bt, int *balanced) {
    REQ(Bt && balanced, "ldso_ba_batch_balanced: null argument");
    *balanced = Bt->balanced ? 1 : 0;
    return LDSO_OK;
}

int ldso_ba_batch_destroy(ldso_ba_batch_t *Bt) {
    if (!Bt) return LDSO_OK;
    hipSetDevice(Bt->h[0]->device);
    hipStreamSynchronize(Bt->h[0]->stream);
    if (Bt->aux) { hipStreamSynchronize(Bt->aux); hipStreamDestroy(Bt->aux); }
    if (Bt->ev0) hipEventDestroy(Bt->ev0);
    if (Bt->ev1) hipEventDestroy(Bt->ev1);
    if (Bt->evEnd) hipEventDestroy(Bt->evEnd);
    if (Bt->d_items) hipFree(Bt->d_items);
    if (Bt->d_scalars) hipFree(Bt->d_scalars);
    if (Bt->h_scalars) hipHostFree(Bt->h_scalars);
    if (Bt->d_blocks) hipFree(Bt->d_blocks);
    if (Bt->d_wg) hipFree(Bt->d_wg);
    if (Bt->d_stage) hipFree(Bt->d_stage);
    if (Bt->h_stage) hipHostFree(Bt->h_stage);
    // back to the single-window chunking (handles that were re-chunked by ldso_ba_batch_create)
    if (Bt->balanced) { for (ldso_ba *H : Bt->h) { H->chunkCuts.clear(); if (H->D.P > 0) rechunk(H); } }
    else if (Bt->chunkPoints > 0) for (ldso_ba *H : Bt->h) if (H->chunkPoints == 0 && H->D.P > 0) rechunk(H);
    for (ldso_ba *H : Bt->h) if (H->inBatch == Bt) H->inBatch = nullptr;
    delete Bt;
    return LDSO_OK;
}

// `iters` forced Gauss-Newton iterations of every window of the batch: 3 launches per iteration for the whole batch, no host
// synchronisation.  Every window must hold an applied linearisation (ldso_ba_linearize_all + ldso_ba_apply_res, or a previous
// optimize / enqueue) and all of them must be at the same ping-pong parity (true after identical call sequences; not, in general, after
// ldso_ba_batch_optimize, whose windows stop at iterations of their own).
int ldso_ba_batch_enqueue_gn(ldso_ba_batch_t *Bt, int first_iteration, int iters) {
    REQ(Bt && iters >= 0, "ldso_ba_batch_enqueue_gn: bad arguments");
    ldso_ba *H0 = Bt->h[0];
    CHK(hipSetDevice(H0->device));
    for (ldso_ba *H : Bt->h) REQ(H->cur == H0->cur && !H->pendingApply, "ldso_ba_batch_enqueue_gn: the windows of a batch must be at the same stage");
    RUN(batch_refresh(Bt));
    const Damping d = damping(H0->settings, 1e-1);
    int cur = 0;          // relative to every window's applied set (BatchItem::set[0], batch_refresh)
    // The control step of a batch occupies two workgroups per window for ~30 us: the batch runs as two halves on two streams, the second
    // half an iteration behind the first, so that one half's reduce + control step overlap the other half's (chip-filling) linearisation.
    const int n = (int) Bt->h.size(), n0 = Bt->n0, n1 = n - n0;
    const BatchItem *itA = Bt->d_items + n, *itB = Bt->d_items + n + n0;
    if (n1 > 0 && iters > 0) { CHK(hipEventRecord(Bt->ev0, H0->stream)); CHK(hipStreamWaitEvent(Bt->aux, Bt->ev0, 0)); }
    for (int i = 0; i < iters; i++) {
        CHK(ba_launch_reduce_batch(itA, n0, Bt->halfReduce[0], cur, H0->settings.initialCalibHessian, d.l1, d.il, H0->stream));
        CHK(ba_launch_gn_solve_batch(itA, n0, Bt->Dmax, cur, H0->settings, first_iteration + i, 1e-1, H0->stream));
        if (n1 > 0 && i == 0) { CHK(hipEventRecord(Bt->ev1, H0->stream)); CHK(hipStreamWaitEvent(Bt->aux, Bt->ev1, 0)); }
        CHK(ba_launch_linearize_batch(itA, Bt->d_blocks + Bt->totalChunks, Bt->halfChunks[0], Bt->balanced ? Bt->d_wg + Bt->wgOff[1] : nullptr, Bt->nWG[1], Bt->FS, cur, H0->settings, 1, H0->settings.initialCalibHessian, H0->stream));
        if (n1 > 0) {
            CHK(ba_launch_reduce_batch(itB, n1, Bt->halfReduce[1], cur, H0->settings.initialCalibHessian, d.l1, d.il, Bt->aux));
            CHK(ba_launch_gn_solve_batch(itB, n1, Bt->Dmax, cur, H0->settings, first_iteration + i, 1e-1, Bt->aux));
            CHK(ba_launch_linearize_batch(itB, Bt->d_blocks + Bt->totalChunks + Bt->halfChunks[0], Bt->halfChunks[1], Bt->balanced ? Bt->d_wg + Bt->wgOff[2] : nullptr, Bt->nWG[2], Bt->FS, cur, H0->settings, 1, H0->settings.initialCalibHessian, Bt->aux));
        }
        cur ^= 1;
    }
    if (n1 > 0 && iters > 0) { CHK(hipEventRecord(Bt->evEnd, Bt->aux)); CHK(hipStreamWaitEvent(H0->stream, Bt->evEnd, 0)); }      // ldso_ba_sync(handle) covers both halves
    for (ldso_ba *H : Bt->h) H->cur ^= cur;
    return LDSO_OK;
}

// FullSystem::optimize(mnumOptIts) (FullSystem.cc:725-884, forced-accept schedule) of every window of the batch: per window what ldso_ba_optimize gives on its
// handle alone - resetOOB preamble, lambda = 1e-1 * 0.25^it, its own iteration cap and device-side canbreak exit, the tail (statistics, setNewFrameEnergyTH,
// re-anchoring, adjoints, precalc, linearizeAll(true)), energy log, rmse, non-finite verdict.  Launches per call: one k_batch_begin, then 4 + 3 cap per half (preamble, 3 per iteration, 3 of the tail; cap = the largest iteration cap
// of the batch), whatever the number of windows; no host synchronisation before the one that reads the n scalar blocks.  The schedule of the iterations is that of ldso_ba_batch_enqueue_gn (two
// halves on two streams from four windows on); a window that has stopped costs its workgroups one test of its own scalars[LD_SC_STOP] per launch.
int ldso_ba_batch_optimize(ldso_ba_batch_t *Bt, int mnumOptIts, int force_all_iterations, float *rmse_out, int *iterations_out, int *status_out) {
    REQ(Bt && mnumOptIts >= 0, "ldso_ba_batch_optimize: bad arguments");
    ldso_ba *H0 = Bt->h[0];
    const int n = (int) Bt->h.size(), n0 = Bt->n0, n1 = n - n0;
    REQ(Bt->FS == 8, "ldso_ba_batch_optimize: windows of more than 8 key frames are not supported in a batched optimize (every window needs F <= 8): run them with ldso_ba_optimize");
    int caps = 0;
    for (ldso_ba *H : Bt->h) {
        REQ(H->D.F >= 2, "ldso_ba_batch_optimize: every window of the batch needs at least 2 key frames (F >= 2)");
        REQ(!H->pendingApply, "ldso_ba_batch_optimize: a window has a pending linearisation (ldso_ba_apply_res first)");
        caps = std::max(caps, optimize_iteration_cap(H->D.F, mnumOptIts, force_all_iterations));          // k_batch_begin gives every window its own
    }
    REQ(caps + 2 < 64, "ldso_ba_batch_optimize: too many iterations");
    CHK(hipSetDevice(H0->device));
    RUN(batch_refresh(Bt));
    const ldso_settings_t &St = H0->settings;
    const BatchItem *itH[2] = {Bt->d_items + n, Bt->d_items + n + n0};
    const BatchBlock *blH[2] = {Bt->d_blocks + Bt->totalChunks, Bt->d_blocks + Bt->totalChunks + Bt->halfChunks[0]};
    const int nH[2] = {n0, n1};
    hipStream_t stH[2] = {H0->stream, Bt->aux};
    const int halves = n1 > 0 ? 2 : 1;
    auto linearize = [&](int u, int cur, int stepMode, int itCheck) -> hipError_t {
        return ba_launch_linearize_batch(itH[u], blH[u], Bt->halfChunks[u], Bt->balanced ? Bt->d_wg + Bt->wgOff[1 + u] : nullptr, Bt->nWG[1 + u], Bt->FS, cur, St, stepMode, St.initialCalibHessian, stH[u], itCheck);
    };
    // energy logs cleared, every window's LD_SC_STOP = its cap - 1 (both halves: one launch in front of the fork)
    CHK(ba_launch_batch_begin(Bt->d_items, n, mnumOptIts, force_all_iterations ? 1 : 0, H0->stream));
    if (halves == 2) { CHK(hipEventRecord(Bt->ev0, H0->stream)); CHK(hipStreamWaitEvent(Bt->aux, Bt->ev0, 0)); }
    // linearizeAll(false) with the resetOOB of the preamble fused in (stepMode bit 1) + applyRes: set[0] -> set[1]
    for (int u = 0; u < halves; u++) CHK(linearize(u, 0, 2, -1));
    double lambda = 1e-1;
    for (int i = 0; i < caps; i++) {
        const int cur = 1 ^ (i & 1), itCheck = force_all_iterations ? -1 : i;
        const Damping d = damping(St, lambda);
        for (int u = 0; u < halves; u++) {
            CHK(ba_launch_reduce_batch(itH[u], nH[u], Bt->halfReduce[u], cur, St.initialCalibHessian, d.l1, d.il, stH[u], itCheck));
            CHK(ba_launch_gn_solve_batch(itH[u], nH[u], Bt->Dmax, cur, St, i, lambda, stH[u], i, itCheck));          // POST / THRESH / LOG of the previous linearisation ride along
            if (halves == 2 && u == 0 && i == 0) { CHK(hipEventRecord(Bt->ev1, H0->stream)); CHK(hipStreamWaitEvent(Bt->aux, Bt->ev1, 0)); }      // the second half runs half an iteration behind
            CHK(linearize(u, cur, 1, itCheck));
        }
        lambda *= 0.25;
    }
    // tail: statistics of the last linearisation, re-anchor the newest frame, adjoints, precalc; linearizeAll(true); its statistics
    for (int u = 0; u < halves; u++) {
        CHK(ba_launch_solve_batch(itH[u], nH[u], Bt->Dmax, St, SK_POST | SK_THRESH | SK_LOG | SK_REANCHOR | SK_ADJ | SK_NONULLSPACE | SK_PRECALC, 0, nullptr, stH[u]));
        CHK(ba_launch_linearize_batch_fix(itH[u], blH[u], Bt->halfChunks[u], Bt->balanced ? Bt->d_wg + Bt->wgOff[1 + u] : nullptr, Bt->nWG[1 + u], St, St.initialCalibHessian, stH[u]));
        CHK(ba_launch_solve_batch(itH[u], nH[u], Bt->Dmax, St, SK_POST | SK_THRESH | SK_LOG, 1, Bt->d_scalars, stH[u]));
    }
    if (halves == 2) { CHK(hipEventRecord(Bt->evEnd, Bt->aux)); CHK(hipStreamWaitEvent(H0->stream, Bt->evEnd, 0)); }
    CHK(hipMemcpyAsync(Bt->h_scalars, Bt->d_scalars, (size_t) n * 16 * sizeof(double), hipMemcpyDeviceToHost, H0->stream));
    CHK(hipStreamSynchronize(H0->stream));
    int rc = LDSO_OK;
    for (int i = 0; i < n; i++) {
        ldso_ba *H = Bt->h[i];
        const double *sc = Bt->h_scalars + (size_t) i * 16;
        const int done = (int) sc[LD_SC_STOP] + 1;          // the scalar names the last iteration the window executed
        H->cur ^= done & 1;                                 // preamble + done iterations + the fixing pass swapped the sets done + 2 times
        H->pendingApply = false; H->appliedValid = true; H->lastIterations = done;
        const bool bad = !std::isfinite(sc[0]) || sc[4] != 0.0;
        if (bad) rc = LDSO_E_NONFINITE;
        if (iterations_out) iterations_out[i] = done;
        if (rmse_out) rmse_out[i] = sqrtf((float) (sc[0] / (8 * sc[9])));
        if (status_out) status_out[i] = bad ? LDSO_E_NONFINITE : LDSO_OK;
    }
    return rc;
}

}  // extern "C"

// The staging arena of the batched key-frame steps (marginalisations, activations, window update, frames): `up` bytes go up (the marginalisations:
// [n MargWin | flags]), `down` bytes come down, or are written on the device, behind them.  Grown on demand with half as much again; both streams are idle when it
// is replaced (every user of the arena ends with a wait on the batch's stream).
int batch_stage(ldso_ba_batch *Bt, size_t up, size_t down) {
    return grow_arena(Bt->h_stage, Bt->d_stage, Bt->stageCap, up + down, 2, Bt->h[0]->stream);
}
// what both entries refuse, worded like ldso_ba_batch_optimize; `solo`: the single-window entry the message points to, `part(i)`: does window i take part
template <class Part> static int marg_checks(ldso_ba_batch *Bt, const char *who, const char *solo, Part part) {
    const std::string w(who);
    REQ(Bt->FS == 8, w + ": windows of more than 8 key frames are not supported in a batched marginalisation (every window needs F <= 8): run them with " + solo);
    for (size_t i = 0; i < Bt->h.size(); i++) {
        const ldso_ba *H = Bt->h[i];
        if (!part((int) i)) continue;
        REQ(H->D.P > 0 && H->D.F >= 2, w + ": a window of the batch is not set");
        REQ(!H->pendingApply, w + ": a window has a pending linearizeAll result (ldso_ba_apply_res first)");
        REQ(H->D.pBegin == 0 && H->D.pEnd == H->D.P, w + ": not available on a sharded handle");
    }
    return LDSO_OK;
}

extern "C" {

// EnergyFunctional::marginalizePointsF (EnergyFunctional.cc:165-222) with the re-linearise + fixLinearizationF pass of FullSystem::flagPointsForRemoval
// (FullSystem.cc:1241-1250) for every window i of the batch with flags[i] != NULL: per window what ldso_ba_marginalize_points gives on its handle alone.  One
// upload (the window table and all flags), three launches (k_linearize_batch_marg -> k_reduce_batch_marg -> k_marg_gather_update_batch), one download, one wait,
// whatever the number of windows.
int ldso_ba_batch_marginalize_points(ldso_ba_batch_t *Bt, const int32_t *const *flags, double *const *HM_out, double *const *bM_out) {
    REQ(Bt, "ldso_ba_batch_marginalize_points: null batch");
    REQ(flags, "ldso_ba_batch_marginalize_points: null flags");
    RUN(marg_checks(Bt, "ldso_ba_batch_marginalize_points", "ldso_ba_marginalize_points", [&](int i) { return flags[i] != nullptr; }));
    ldso_ba *H0 = Bt->h[0];
    const int n = (int) Bt->h.size();
    CHK(hipSetDevice(H0->device));
    RUN(batch_refresh(Bt));
    size_t nFlags = 0, nOut = 0;
    int red = 0, maxGSP = 0, maxN = 0, taking = 0;
    std::vector<MargWin> tab((size_t) n);
    for (int i = 0; i < n; i++) {
        const ldso_ba *H = Bt->h[i];
        MargWin &m = tab[(size_t) i];
        memset(&m, 0, sizeof(m));
        m.active = flags[i] != nullptr ? 1 : 0; m.flagOff = (int32_t) nFlags; m.frameIdx = -1; m.redBlock0 = red; m.outOff = (int32_t) nOut;
        if (!m.active) continue;
        taking++;
        nFlags += (size_t) H->D.P; nOut += (size_t) H->D.n * H->D.n + H->D.n;
        red += reduce_pairs(H->D.F, false) + LD_SC_SPLITS;
        maxGSP = std::max(maxGSP, H->GSP); maxN = std::max(maxN, (int) H->D.n);
    }
    if (taking == 0) return LDSO_OK;
    const size_t up = (n * sizeof(MargWin) + nFlags * sizeof(int32_t) + 7) & ~(size_t) 7, down = nOut * sizeof(double);
    RUN(batch_stage(Bt, up, down));
    memcpy(Bt->h_stage, tab.data(), n * sizeof(MargWin));
    int32_t *h_flags = (int32_t *) (Bt->h_stage + n * sizeof(MargWin));
    for (int i = 0; i < n; i++) if (tab[(size_t) i].active) memcpy(h_flags + tab[(size_t) i].flagOff, flags[i], (size_t) Bt->h[i]->D.P * sizeof(int32_t));
    CHK(hipMemcpyAsync(Bt->d_stage, Bt->h_stage, up, hipMemcpyHostToDevice, H0->stream));
    const MargWin *d_mw = (const MargWin *) Bt->d_stage;
    const int32_t *d_flags = (const int32_t *) (Bt->d_stage + n * sizeof(MargWin));
    double *d_out = (double *) (Bt->d_stage + up);
    CHK(ba_launch_linearize_batch_marg(Bt->d_items, Bt->d_blocks, Bt->totalChunks, Bt->balanced ? Bt->d_wg + Bt->wgOff[0] : nullptr, Bt->nWG[0], d_mw, d_flags, H0->settings, H0->stream));
    CHK(ba_launch_reduce_batch_marg(Bt->d_items, d_mw, n, red, maxGSP, H0->stream));
    CHK(ba_launch_marg_gather_update_batch(Bt->d_items, d_mw, n, maxN, (double) H0->settings.margWeightFac, d_out, H0->stream));
    for (int i = 0; i < n; i++) if (tab[(size_t) i].active) Bt->h[i]->hasPrior = true;          // the next batch_refresh / refresh_item hands it to the iteration kernels
    CHK(hipMemcpyAsync(Bt->h_stage + up, d_out, down, hipMemcpyDeviceToHost, H0->stream));
    CHK(hipStreamSynchronize(H0->stream));
    const double *h_out = (const double *) (Bt->h_stage + up);
    for (int i = 0; i < n; i++) {
        const MargWin &m = tab[(size_t) i];
        if (!m.active) continue;
        const size_t nn = (size_t) Bt->h[i]->D.n;
        if (HM_out && HM_out[i]) memcpy(HM_out[i], h_out + m.outOff, nn * nn * sizeof(double));
        if (bM_out && bM_out[i]) memcpy(bM_out[i], h_out + m.outOff + nn * nn, nn * sizeof(double));
    }
    return LDSO_OK;
}

// EnergyFunctional::marginalizeFrame (EnergyFunctional.cc:72-151) on the device prior of every window i of the batch with frame_idx[i] >= 0: per window what
// ldso_ba_marginalize_frame(handle_i, frame_idx[i], ...) gives ((8(F-1)+4)^2 row-major, 8(F-1)+4); the handles keep their priors and windows.  One upload, one
// launch (k_marg_frame_batch, a workgroup per window), one download, one wait.
int ldso_ba_batch_marginalize_frame(ldso_ba_batch_t *Bt, const int32_t *frame_idx, double *const *HM_out, double *const *bM_out) {
    REQ(Bt, "ldso_ba_batch_marginalize_frame: null batch");
    REQ(frame_idx, "ldso_ba_batch_marginalize_frame: null frame_idx");
    RUN(marg_checks(Bt, "ldso_ba_batch_marginalize_frame", "ldso_ba_marginalize_frame", [&](int i) { return frame_idx[i] >= 0; }));
    ldso_ba *H0 = Bt->h[0];
    const int n = (int) Bt->h.size();
    size_t nOut = 0;
    int taking = 0;
    std::vector<MargWin> tab((size_t) n);
    for (int i = 0; i < n; i++) {
        const ldso_ba *H = Bt->h[i];
        MargWin &m = tab[(size_t) i];
        memset(&m, 0, sizeof(m));
        m.active = frame_idx[i] >= 0 ? 1 : 0; m.frameIdx = frame_idx[i]; m.outOff = (int32_t) nOut;
        if (!m.active) continue;
        REQ(frame_idx[i] < H->D.F, "ldso_ba_batch_marginalize_frame: a frame index is not a key frame of its window (frame_idx[i] < F_i)");
        REQ(HM_out && bM_out && HM_out[i] && bM_out[i], "ldso_ba_batch_marginalize_frame: a window that takes part needs its HM_out[i] and bM_out[i]");
        taking++;
        const size_t nd = (size_t) H->D.n - 8;
        nOut += nd * nd + nd;
    }
    if (taking == 0) return LDSO_OK;
    CHK(hipSetDevice(H0->device));
    RUN(batch_refresh(Bt));
    const size_t up = (n * sizeof(MargWin) + 7) & ~(size_t) 7, down = nOut * sizeof(double);
    RUN(batch_stage(Bt, up, down));
    memcpy(Bt->h_stage, tab.data(), n * sizeof(MargWin));
    CHK(hipMemcpyAsync(Bt->d_stage, Bt->h_stage, up, hipMemcpyHostToDevice, H0->stream));
    double *d_out = (double *) (Bt->d_stage + up);
    CHK(ba_launch_marg_frame_batch(Bt->d_items, n, (const MargWin *) Bt->d_stage, d_out, H0->stream));
    CHK(hipMemcpyAsync(Bt->h_stage + up, d_out, down, hipMemcpyDeviceToHost, H0->stream));
    CHK(hipStreamSynchronize(H0->stream));
    const double *h_out = (const double *) (Bt->h_stage + up);
    for (int i = 0; i < n; i++) {
        const MargWin &m = tab[(size_t) i];
        if (!m.active) continue;
        const size_t nd = (size_t) Bt->h[i]->D.n - 8;
        memcpy(HM_out[i], h_out + m.outOff, nd * nd * sizeof(double));
        memcpy(bM_out[i], h_out + m.outOff + nd * nd, nd * sizeof(double));
    }
    return LDSO_OK;
}

// average duration of the batched k_linearize for bench.py's roofline: `reps` back-to-back launches on the applied state (read set ->
// scratch set, no point step: idempotent) between one pair of HIP events on the batch's stream
int ldso_ba_batch_time_linearize(ldso_ba_batch_t *Bt, int reps, double *avg_us) {
    REQ(Bt && reps > 0 && avg_us, "ldso_ba_batch_time_linearize: bad arguments");
    ldso_ba *H0 = Bt->h[0];
    CHK(hipSetDevice(H0->device));
    RUN(batch_refresh(Bt));
    return time_launches(H0->stream, reps, avg_us, [Bt, H0]() -> int {
        CHK(ba_launch_linearize_batch(Bt->d_items, Bt->d_blocks, Bt->totalChunks, Bt->balanced ? Bt->d_wg + Bt->wgOff[0] : nullptr, Bt->nWG[0], Bt->FS, 0, H0->settings, 0, H0->settings.initialCalibHessian, H0->stream));
        return LDSO_OK;
    });
}
}  // extern "C"
