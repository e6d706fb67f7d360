// select_dev.h — the device functions that more than one selector uses (features.hip, pixel_select.hip, init_first.hip): absSquaredGrad with the response
// table, the argmax key, the lanes a pot x pot block gets, the non-finite report and the 256-thread prefix sum.  Every float expression keeps the reference's
// operand order (-ffp-contract=off).  The raster scan built on the prefix sum is raster_scan.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define SEL_FLAG_NONFINITE 1            // bit 0 of a selector's flag word: a non-finite value was read

// absSquaredGrad (FrameHessian.cc:91-96) of a pixel whose gradient the caller holds
static __device__ __forceinline__ float abs_sq_grad(float I, float dx, float dy, const float *B, bool &bad) {
    if (!isfinite(I) || !isfinite(dx) || !isfinite(dy)) bad = true;
    float d = dx * dx + dy * dy;
    if (B) {
        int c = isfinite(I) ? (int) (I + 0.5f) : 5;                // CalibHessian::getBGradOnly (CalibHessian.h:102-111)
        if (c < 5) c = 5;
        if (c > 250) c = 250;
        const float gw = B[c + 1] - B[c];
        d *= gw * gw;
    }
    return d;
}
// ... of the 12-byte pixel px = (I, dx, dy), whose gradient it hands back
static __device__ __forceinline__ float abs_sq_grad(const float *px, const float *B, bool &bad, float &dx, float &dy) {
    const float I = px[0]; dx = px[1]; dy = px[2];
    return abs_sq_grad(I, dx, dy, B, bad);
}

// argmax over (value, index) as one 64-bit integer maximum: the larger value and, among equals, the SMALLEST index; `bits` (of a float >= 0, say) order as unsigned, 0 = none
static __device__ __forceinline__ unsigned long long argmax_key(unsigned bits, int index) { return ((unsigned long long) bits << 32) | (unsigned) (0x7fffffff - index); }
static __device__ __forceinline__ unsigned long long argmax_key(float v, int index) { return argmax_key((unsigned) __float_as_int(v), index); }
static __device__ __forceinline__ int argmax_index(unsigned long long key) { return 0x7fffffff - (int) (unsigned) key; }

// lanes that share a pot x pot block: 1, 4, 16 or 64, so a block never straddles a wavefront
static __host__ __device__ inline int lanes_per_block(int pot) { return pot <= 1 ? 1 : pot == 2 ? 4 : pot <= 4 ? 16 : 64; }

// one atomic per wavefront that read something non-finite (every lane of the wavefront calls it).  `bad` by reference: by value the compiler normalises the
// bool first and k_pix_select comes out three vector registers larger
static __device__ __forceinline__ void report_nonfinite(const bool &bad, int32_t *flagWord) {
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flagWord, SEL_FLAG_NONFINITE);
}

// Exclusive prefix sum of counts[0 .. n) by one workgroup of 256 (part: 256 ints of LDS): thread t owns the segment [b, e) - empty behind the end - and gets
// the sum of everything before it in `off`; thread 0 writes the sum of all to *total.
struct Segment { int b, e, off; };
static __device__ __forceinline__ Segment segment_scan256(const int32_t *counts, int n, int *part, int32_t *total) {
    const int tid = threadIdx.x, per = (n + 255) / 256, b = min(tid * per, n), e = min(b + per, n);
    int s = 0;
    for (int i = b; i < e; i++) s += counts[i];
    part[tid] = s;
    __syncthreads();
    if (tid == 0) { int a = 0; for (int i = 0; i < 256; i++) { const int t = part[i]; part[i] = a; a += t; } *total = a; }
    __syncthreads();
    return {b, e, part[tid]};
}
