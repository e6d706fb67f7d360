// tracker_ref.hip — the reference key frame's point cloud of the coarse tracker: CoarseTracker::makeCoarseDepthL0 (reference src/frontend/CoarseTracker.cc:258-438)
// as k_tr_scatter / k_tr_pool / k_tr_dilate / k_tr_count + scan + write, and tr_set_ref_common as their launcher.
#include "tracker.h"

// The reference adds the points to the level-0 maps one after the other (CoarseTracker.cc:268-283): float sums in point order.
// Deterministic and in that order here, without float atomics: a first kernel threads the points of every pixel into a list
// (integer atomics: the list order is arbitrary, its content is not), the second lets the lowest-indexed point of a pixel add all of
// the pixel's points in ascending index order (lists are short: a selection walk).  Points that round to a pixel outside the image
// (the reference would write out of bounds) are ignored.
__device__ __forceinline__ int tr_pt_pixel(const float *pts, int i, int w, int h) {
    const int u = (int) (pts[4 * i + 0] + 0.5f), v = (int) (pts[4 * i + 1] + 0.5f);
    return (u >= 0 && u < w && v >= 0 && v < h) ? u + w * v : -1;
}
__global__ void k_tr_scatter_link(const float *pts, int n, int *head /*w*h, -1*/, int *next /*n*/, int w, int h) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int px = tr_pt_pixel(pts, i, w, h);
    if (px >= 0) next[i] = atomicExch(&head[px], i);
}
__global__ void k_tr_scatter(const float *pts, int n, float *idepth, float *wsum, const int *head, const int *next, int w, int h) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int px = tr_pt_pixel(pts, i, w, h);
    if (px < 0) return;
    for (int j = head[px]; j >= 0; j = next[j]) if (j < i) return;       // an earlier point owns this pixel
    float sid = 0.f, sw = 0.f;
    int cur = i;
    while (cur >= 0) {
        const float new_idepth = pts[4 * cur + 2];
        const float weight = sqrtf((float) (1e-3 / ((double) pts[4 * cur + 3] + 1e-12)));
        sid += new_idepth * weight;
        sw += weight;
        int nxt = -1;                                                     // the smallest index above cur
        for (int j = head[px]; j >= 0; j = next[j]) if (j > cur && (nxt < 0 || j < nxt)) nxt = j;
        cur = nxt;
    }
    idepth[px] = sid; wsum[px] = sw;
}

__global__ void k_tr_pool(const float *id_lm, const float *ws_lm, float *id_l, float *ws_l, int wl, int hl, int wlm1) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= wl * hl) return;
    int x = i % wl, y = i / wl;
    int bidx = 2 * x + 2 * y * wlm1;
    id_l[i] = id_lm[bidx] + id_lm[bidx + 1] + id_lm[bidx + wlm1] + id_lm[bidx + wlm1 + 1];
    ws_l[i] = ws_lm[bidx] + ws_lm[bidx + 1] + ws_lm[bidx + wlm1] + ws_lm[bidx + wlm1 + 1];
}

// in-place dilation exactly as the reference: reads the weight backup and idepth of pixels with weight > 0,
// writes only pixels with weight <= 0, so a parallel sweep equals the sequential one.
__global__ void k_tr_dilate(float *idepth, float *wsum, const float *bak, int wl, int hl, int diagonal) {
    int i = blockIdx.x * blockDim.x + threadIdx.x + wl;
    int wh = wl * hl - wl;
    if (i >= wh) return;
    if (bak[i] <= 0) {
        float sum = 0, num = 0, numn = 0;
        int o0 = diagonal ? 1 + wl : 1, o1 = diagonal ? -1 - wl : -1, o2 = diagonal ? wl - 1 : wl, o3 = diagonal ? -wl + 1 : -wl;
        if (bak[i + o0] > 0) { sum += idepth[i + o0]; num += bak[i + o0]; numn++; }
        if (bak[i + o1] > 0) { sum += idepth[i + o1]; num += bak[i + o1]; numn++; }
        if (bak[i + o2] > 0) { sum += idepth[i + o2]; num += bak[i + o2]; numn++; }
        if (bak[i + o3] > 0) { sum += idepth[i + o3]; num += bak[i + o3]; numn++; }
        if (numn > 0) { idepth[i] = sum / numn; wsum[i] = num / numn; }
    }
}

// order-preserving compaction over the interior (2 <= x < w-2, 2 <= y < h-2), row-major like the reference
__device__ __forceinline__ bool tr_keep(const float *idepth, const float *wsum, const float *ref, int i, float &id, float &col) {
    float ws = wsum[i];
    if (!(ws > 0)) return false;
    id = idepth[i] / ws;
    col = ref[3 * i];
    return isfinite(col) && (id > 0);
}

__global__ void k_tr_count(TrLevel L) {
    __shared__ int sc[256 / 64];
    int wi = L.w - 4, hi = L.h - 4;
    int e = blockIdx.x * blockDim.x + threadIdx.x;
    bool keep = false;
    if (e < wi * hi) { int x = 2 + e % wi, y = 2 + e / wi; float id, col; keep = tr_keep(L.idepth, L.wsum, L.refImg, x + y * L.w, id, col); }
    int c = __popcll(__ballot(keep));
    if ((threadIdx.x & 63) == 0) sc[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) L.blockCnt[blockIdx.x] = sc[0] + sc[1] + sc[2] + sc[3];
}

__global__ void k_tr_scan(int *cnt, int nb, int *total) {     // single block exclusive scan
    __shared__ int carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < nb; base += blockDim.x) {
        int i = base + threadIdx.x;
        int v = (i < nb) ? cnt[i] : 0;
        int inc = v;
        for (int o = 1; o < 64; o <<= 1) { int t = __shfl_up(inc, o, 64); if ((threadIdx.x & 63) >= o) inc += t; }
        __shared__ int ws[16];
        if ((threadIdx.x & 63) == 63) ws[threadIdx.x >> 6] = inc;
        __syncthreads();
        int off = carry;
        for (int wv = 0; wv < (int) (threadIdx.x >> 6); wv++) off += ws[wv];
        if (i < nb) cnt[i] = off + inc - v;
        __syncthreads();
        if (threadIdx.x == blockDim.x - 1) carry = off + inc;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}

__global__ void k_tr_write(TrLevel L) {
    __shared__ int sc[256 / 64];
    int wi = L.w - 4, hi = L.h - 4;
    int e = blockIdx.x * blockDim.x + threadIdx.x;
    bool keep = false;
    float id = 0, col = 0;
    int x = 0, y = 0;
    if (e < wi * hi) { x = 2 + e % wi; y = 2 + e / wi; keep = tr_keep(L.idepth, L.wsum, L.refImg, x + y * L.w, id, col); }
    unsigned long long m = __ballot(keep);
    int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) sc[wv] = __popcll(m);
    __syncthreads();
    int off = L.blockCnt[blockIdx.x];
    for (int q = 0; q < wv; q++) off += sc[q];
    off += __popcll(m & ((1ull << lane) - 1ull));
    if (keep) { L.pc_u[off] = (float) x; L.pc_v[off] = (float) y; L.pc_idepth[off] = id; L.pc_color[off] = col; }
}

int tr_set_ref_common(ldso_tracker *H, float ref_a, float ref_b, float ref_exposure, const float *pts, int n) {
    H->P.ref_a = ref_a; H->P.ref_b = ref_b; H->P.ref_exposure = ref_exposure;
    if (n > H->ptsCap) {
        if (H->d_pts) hipFree(H->d_pts);
        if (H->d_next) hipFree(H->d_next);
        H->d_pts = nullptr; H->d_next = nullptr; H->ptsCap = 0;
        void *q; CHK(hipMalloc(&q, (size_t) n * 16)); H->d_pts = (float *) q;
        CHK(hipMalloc(&q, (size_t) n * 4)); H->d_next = (int *) q;
        H->ptsCap = n;
    }
    if (n) CHK(hipMemcpyAsync(H->d_pts, pts, (size_t) n * 16, hipMemcpyHostToDevice, H->stream));
    // makeCoarseDepthL0
    TrLevel *lv = H->P.lv;
    CHK(hipMemsetAsync(lv[0].idepth, 0, (size_t) lv[0].w * lv[0].h * 4, H->stream));
    CHK(hipMemsetAsync(lv[0].wsum, 0, (size_t) lv[0].w * lv[0].h * 4, H->stream));
    if (n) {
        int *head = reinterpret_cast<int *>(lv[0].wsum_bak);        // free until the dilation below
        CHK(hipMemsetAsync(head, 0xFF, (size_t) lv[0].w * lv[0].h * 4, H->stream));
        hipLaunchKernelGGL(k_tr_scatter_link, dim3((n + 255) / 256), dim3(256), 0, H->stream, H->d_pts, n, head, H->d_next, lv[0].w, lv[0].h);
        hipLaunchKernelGGL(k_tr_scatter, dim3((n + 255) / 256), dim3(256), 0, H->stream, H->d_pts, n, lv[0].idepth, lv[0].wsum, head, H->d_next, lv[0].w, lv[0].h);
    }
    for (int l = 1; l < H->levels; l++) {
        int npx = lv[l].w * lv[l].h;
        hipLaunchKernelGGL(k_tr_pool, dim3((npx + 255) / 256), dim3(256), 0, H->stream, lv[l - 1].idepth, lv[l - 1].wsum, lv[l].idepth, lv[l].wsum, lv[l].w, lv[l].h, lv[l - 1].w);
    }
    for (int l = 0; l < H->levels; l++) {
        int npx = lv[l].w * lv[l].h;
        CHK(hipMemcpyAsync(lv[l].wsum_bak, lv[l].wsum, (size_t) npx * 4, hipMemcpyDeviceToDevice, H->stream));
        hipLaunchKernelGGL(k_tr_dilate, dim3((npx + 255) / 256), dim3(256), 0, H->stream, lv[l].idepth, lv[l].wsum, lv[l].wsum_bak, lv[l].w, lv[l].h, l < 2 ? 1 : 0);
    }
    for (int l = 0; l < H->levels; l++) {
        int ni = (lv[l].w - 4) * (lv[l].h - 4);
        int nb = (ni + 255) / 256;
        hipLaunchKernelGGL(k_tr_count, dim3(nb), dim3(256), 0, H->stream, lv[l]);
        hipLaunchKernelGGL(k_tr_scan, dim3(1), dim3(1024), 0, H->stream, lv[l].blockCnt, nb, H->d_total + l);
        hipLaunchKernelGGL(k_tr_write, dim3(nb), dim3(256), 0, H->stream, lv[l]);
    }
    int tot[TR_MAXL] = {0};
    CHK(hipMemcpyAsync(tot, H->d_total, (size_t) H->levels * 4, hipMemcpyDeviceToHost, H->stream));      // one read-back for all levels
    CHK(hipStreamSynchronize(H->stream));
    for (int l = 0; l < H->levels; l++) lv[l].n = tot[l];
    CHK(hipGetLastError());
    return LDSO_OK;
}
