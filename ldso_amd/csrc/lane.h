// lane.h — the lane-exchange wrappers of the kernels (wave64): one name for each builtin and for each DPP control word that more than one kernel file uses.
// A wrapper is the builtin with the float <-> int bit casts around it and nothing else.  A floating-point sum across lanes adds in an order of its own and stays
// with its kernel; integer sums and maxima do not depend on the order, so their butterflies over the wavefront are here (wave_sum, wave_max).
#pragma once
#include <hip/hip_runtime.h>

// v_mov_b32 with a DPP control (all rows and banks, lanes without a source keep 0)
template <int CTRL> __device__ __forceinline__ int dpp_mov(int x) { return __builtin_amdgcn_update_dpp(0, x, CTRL, 0xF, 0xF, true); }
template <int CTRL> __device__ __forceinline__ float dpp_mov(float x) { return __builtin_bit_cast(float, dpp_mov<CTRL>(__builtin_bit_cast(int, x))); }
__device__ __forceinline__ float dpp_quad_xor1(float x) { return dpp_mov<0xB1>(x); }          // quad_perm [1,0,3,2]
__device__ __forceinline__ float dpp_quad_xor2(float x) { return dpp_mov<0x4E>(x); }          // quad_perm [2,3,0,1]
__device__ __forceinline__ float dpp_half_mirror(float x) { return dpp_mov<0x141>(x); }       // lane i <-> 7-i within each 8-lane half row
__device__ __forceinline__ float dpp_row_ror8(float x) { return dpp_mov<0x128>(x); }          // lane i <-> i ^ 8 within each 16-lane row
// lane i receives lane i-J of its 16-lane row (0 when that leaves the row)
template <int J> __device__ __forceinline__ float dpp_row_shr(float x) { return dpp_mov<0x110 + J>(x); }
// sum over the 8 lanes of a group, result in all 8 lanes (tree order)
__device__ __forceinline__ float sum8(float x) { x += dpp_quad_xor1(x); x += dpp_quad_xor2(x); x += dpp_half_mirror(x); return x; }
// v_readlane_b32: lane l (wave-uniform) of x in every lane
__device__ __forceinline__ int lane_read_i(int x, int l) { return __builtin_amdgcn_readlane(x, l); }
__device__ __forceinline__ int lane_read_i(float x, int l) { return lane_read_i(__builtin_bit_cast(int, x), l); }
__device__ __forceinline__ float lane_read(float x, int l) { return __builtin_bit_cast(float, lane_read_i(x, l)); }
// ds_bpermute_b32: every lane reads x of the lane its byte address (lane << 2) names
__device__ __forceinline__ float lane_perm(float x, int byteAddr) { return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(byteAddr, __builtin_bit_cast(int, x))); }
__device__ __forceinline__ float lane_shfl(float x, int lane) { return lane_perm(x, lane << 2); }
// xor butterflies over the 64 lanes, result in every lane
__device__ __forceinline__ int wave_sum(int x) { for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64); return x; }
__device__ __forceinline__ unsigned long long wave_max(unsigned long long m) { for (int o = 32; o > 0; o >>= 1) { const unsigned long long x = __shfl_xor(m, o, 64); if (x > m) m = x; } return m; }
__device__ __forceinline__ float wave_max(float m) { for (int o = 32; o > 0; o >>= 1) { const float x = __shfl_xor(m, o, 64); if (x > m) m = x; } return m; }          // a NaN never wins
