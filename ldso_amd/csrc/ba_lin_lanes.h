// ba_lin_lanes.h — the lane exchanges of the linearisation kernels alone (wave64, lane = slot * 8 + pattern pixel): broadcasts and choices inside the 8 lanes of a
// slot, the reference-order sum over them, the sums over the slots of a wavefront.  Built on lane.h, which keeps the names that more than one kernel file uses.
#pragma once
#include <hip/hip_runtime.h>
#include "lane.h"

__device__ __forceinline__ float dpp_quad_xor3(float x) { return dpp_mov<0x1B>(x); }   // quad_perm [3,2,1,0]
// lane j (0..3) of each quad broadcast to its quad
template <int J> __device__ __forceinline__ float dpp_quad_bcast(float x) { return dpp_mov<J * 0x55>(x); }
// element J and element 4 + J of every 8-lane group, in all 8 lanes of the group (two DPP moves and two selects instead of two ds_bpermute)
template <int J> __device__ __forceinline__ void group_bcast_pair(float x, int k, float &lo, float &hi) {
    const float a = dpp_quad_bcast<J>(x);           // lanes 0-3: x[J], lanes 4-7: x[4 + J]
    const float b = dpp_half_mirror(a);             // lanes 0-3: x[4 + J], lanes 4-7: x[J]
    lo = (k < 4) ? a : b; hi = (k < 4) ? b : a;
}

// lane-indexed choice among wave-uniform-per-slot values (k = pattern lane 0..7) as a binary tree over the bits of k: 7 (6: 5, 4: 3) v_cndmask with THREE lane masks.
// Written with array elements in a chain of ternaries the choice became control flow (clang evaluates an array element of a conditional operator under a
// branch; the chain of k == c branches is folded into a switch and lowered, for a divergent k, as a tree of exec-mask branches: ~14 vector + ~25 scalar
// instructions per choice, round 6 ISA count) - scalar arguments of a function are selected.
static __device__ __forceinline__ float sel2(const bool c, const float a, const float b) { return c ? a : b; }
static __device__ __forceinline__ float selk8(const int k, const float a0, const float a1, const float a2, const float a3, const float a4, const float a5, const float a6, const float a7) {
    const bool b0 = (k & 1) != 0, b1 = (k & 2) != 0, b2 = (k & 4) != 0;
    const float l0 = sel2(b0, a1, a0), l1 = sel2(b0, a3, a2), l2 = sel2(b0, a5, a4), l3 = sel2(b0, a7, a6);
    const float m0 = sel2(b1, l1, l0), m1 = sel2(b1, l3, l2);
    return sel2(b2, m1, m0);
}
static __device__ __forceinline__ float selk4(const int k, const float a0, const float a1, const float a2, const float a3) {
    const bool b0 = (k & 1) != 0, b1 = (k & 2) != 0;
    return sel2(b1, sel2(b0, a3, a2), sel2(b0, a1, a0));
}
// k in 0..5 (lanes 6, 7 receive a4 / a5: their callers overwrite the result)
static __device__ __forceinline__ float selk6(const int k, const float a0, const float a1, const float a2, const float a3, const float a4, const float a5) {
    const bool b0 = (k & 1) != 0, b1 = (k & 2) != 0, b2 = (k & 4) != 0;
    const float l0 = sel2(b0, a1, a0), l1 = sel2(b0, a3, a2), l2 = sel2(b0, a5, a4);
    const float m0 = sel2(b1, l1, l0);
    return sel2(b2, l2, m0);
}

// sum over the 8 lanes in the reference's sequential order ((((x0+x1)+x2)+...)+x7), result in all 8 lanes.
// The running sum lives in lane 7 of each group (lanes 7 and 15 of a row): step j adds x_j fetched with row_shr:(7-j) - one
// v_add_f32_dpp per step whose DPP operand (x) is old, so no hazard padding; other lanes compute values nobody reads.
__device__ __forceinline__ float seq8(float x, int k, int lane) {
    float t = dpp_row_shr<7>(x);
    t = t + dpp_row_shr<6>(x);
    t = t + dpp_row_shr<5>(x);
    t = t + dpp_row_shr<4>(x);
    t = t + dpp_row_shr<3>(x);
    t = t + dpp_row_shr<2>(x);
    t = t + dpp_row_shr<1>(x);
    t = t + x;
    (void) lane;
    float lo, hi;
    group_bcast_pair<3>(t, k, lo, hi);          // hi = element 7 of the group
    return hi;
}

// sum over the 8 slots of a wave (lanes with equal k), result in every lane: slot pairs by row_ror:8, then the four rows by two ds_bpermute
// butterflies (tree order; the sequential-order sums that decide residual states use seq8).  gfx950's v_permlane16_swap / v_permlane32_swap
// butterflies were measured against this in rounds 3 and 4: bit-identical, 2 % slower in every configuration - removed.
__device__ __forceinline__ float sum_slots(float x, int a16, int a32) {
    x += dpp_row_ror8(x);
    x += lane_perm(x, a16);
    x += lane_perm(x, a32);
    return x;
}
// sum over the 4 slots of a half-wave (lanes with equal k inside lanes 0..31 / 32..63), result in every lane of the half: the first two steps of sum_slots
__device__ __forceinline__ float sum_half(float x, int a16) {
    x += dpp_row_ror8(x);
    x += lane_perm(x, a16);
    return x;
}
