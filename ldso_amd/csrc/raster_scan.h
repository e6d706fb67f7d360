// raster_scan.h — the raster rank of the set pixels of a byte map, for the thinning and the records of pixel_select.hip and the records of init_first.hip: one
// wavefront per row counts (k_raster_rows), one workgroup turns the counts into row starts (k_raster_rowscan), and raster_walk hands every set pixel of a row to the
// caller's statement with its rank = row start + set pixels before it in the row.  The library is built without relocatable device code, so the two kernels are
// static (each including file gets its own copy) and the walk is instantiated beside its statement.
#pragma once
#include "hip_host.h"
#include "lane.h"
#include "select_dev.h"

struct ScanRect { int x0, x1, y0, y1; };          // [x0, x1) x [y0, y1)

// the pixels makeNewTraces and setFirst scan: patternPadding + 1 <= x < w - patternPadding - 2 (patternPadding = 2, Settings.h:164)
static inline ScanRect scan_rect(int w, int h) { return {3, w - 4, 3, h - 4}; }
static inline dim3 raster_grid(int h) { return dim3((h + 3) / 4); }          // one wavefront per row, four rows per workgroup of 256
static __device__ __forceinline__ int raster_row() { return blockIdx.x * 4 + (threadIdx.x >> 6); }

// set pixels per row inside r (0 for the rows outside)
static __global__ __launch_bounds__(256) void k_raster_rows(const unsigned char *__restrict__ map, int w, int h, ScanRect r, int32_t *__restrict__ rowCount) {
    const int lane = threadIdx.x & 63, y = raster_row();
    if (y >= h) return;
    int c = 0;
    if (y >= r.y0 && y < r.y1) for (int x = r.x0 + lane; x < r.x1; x += 64) c += map[(size_t) y * w + x] != 0;
    c = wave_sum(c);
    if (lane == 0) rowCount[y] = c;
}

// one workgroup of 256: exclusive prefix sum of the rows' counts
static __global__ __launch_bounds__(256) void k_raster_rowscan(const int32_t *__restrict__ rowCount, int32_t *__restrict__ rowStart, int h, int32_t *__restrict__ total) {
    __shared__ int part[256];
    const Segment s = segment_scan256(rowCount, h, part, total);
    int off = s.off;
    for (int y = s.b; y < s.e; y++) { rowStart[y] = off; off += rowCount[y]; }
}

// emit(x, value, rank) for every set pixel of columns [x0, x1) of row y, called by the whole wavefront; emit may clear the pixel it is given
template <class Emit>
static __device__ __forceinline__ void raster_walk(const unsigned char *map, int w, int x0, int x1, int y, const int32_t *rowStart, Emit emit) {
    const int lane = threadIdx.x & 63;
    int base = rowStart[y];
    for (int xb = x0; xb < x1; xb += 64) {
        const int x = xb + lane;
        const int v = x < x1 ? map[(size_t) y * w + x] : 0;
        const unsigned long long bal = __ballot(v != 0);
        if (v != 0) emit(x, v, base + __popcll(bal & ((1ull << lane) - 1)));
        base += __popcll(bal);
    }
}

// The counting half of a scan on `st`: rows and row starts of `map` (w x h) inside r, the number of set pixels to *total (device) and, where the caller has to size
// record buffers before it emits, to *n on the host (one download, one wait; n = nullptr: neither)
static inline int raster_count(const unsigned char *map, int w, int h, ScanRect r, int32_t *rowCount, int32_t *rowStart, int32_t *total, hipStream_t st, int *n) {
    hipLaunchKernelGGL(k_raster_rows, raster_grid(h), dim3(256), 0, st, map, w, h, r, rowCount);
    hipLaunchKernelGGL(k_raster_rowscan, dim3(1), dim3(256), 0, st, rowCount, rowStart, h, total);
    CHK(hipGetLastError());
    if (n) { CHK(hipMemcpyAsync(n, total, sizeof(int), hipMemcpyDeviceToHost, st)); CHK(hipStreamSynchronize(st)); }
    return LDSO_OK;
}
