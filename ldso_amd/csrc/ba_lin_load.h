// ba_lin_load.h — how the linearisation kernels reach a window's tables and what a wavefront loads for one point (gfx950): the just-in-time pointer groups
// (ldg16 / ldg4 / GP and the indices inside a group), the one-dword-per-lane records (PtIn, RLF / RLI, the GEO_* / REC_* dwords), 32-bit-offset global
// access (AT), and the record loads of a point (load_point) and of a pair of points (load_pair).
// The macros of this header (GP, OFF_B0, OFF_S0, RLF, RLI, GEO_*, REC_*, AT) are seen outside it, on purpose: linearize_body uses them, and ba_linearize_body.h,
// the one file that includes this header, undefines them where it ends.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include "ba_dev.h"

// ---- just-in-time pointer groups ------------------------------------------------------------------------------------------------
// The kernel touches ~55 device arrays per point.  Held in scalar registers for the whole kernel (what the compiler does with a
// descriptor it may load once) they do not fit the 102 SGPRs of a wave: 105 of them were spilled into VGPR lanes, and every use paid
// two v_readlane plus a 64-bit VGPR address (v_lshl_add_u64, flat_load / flat_store) - 260 of the 1234 vector instructions of the point
// loop.  Where the descriptor lives in device memory (k_linearize_batch; DESC = true) a group of eight pointers (64 consecutive bytes of
// BaPtrs / ResSet, see ba_dev.h) is fetched with ONE s_load_dwordx16 right where it is used (scalar cache hit, no vector instruction)
// and is dead a few instructions later; `asm volatile` keeps the compiler from hoisting the load back to the top of the kernel.
typedef int v16i_t __attribute__((ext_vector_type(16)));
template <bool DESC, int OFF> static __device__ __forceinline__ v16i_t ldg16(const void *base) {
    v16i_t t;
    if (DESC) asm volatile("s_load_dwordx16 %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) : "s"(base), "n"(OFF) : "memory");
    else __builtin_memcpy(&t, (const char *) base + OFF, 64);          // kernel arguments: the compiler's own scalar loads
    return t;
}
typedef int v4i_t __attribute__((ext_vector_type(4)));
template <bool DESC, int OFF> static __device__ __forceinline__ v4i_t ldg4(const void *base) {          // two pointers
    v4i_t t;
    if (DESC) asm volatile("s_load_dwordx4 %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) : "s"(base), "n"(OFF) : "memory");
    else __builtin_memcpy(&t, (const char *) base + OFF, 16);
    return t;
}
// two groups with one wait
template <bool DESC, int OFFA, int OFFB> static __device__ __forceinline__ void ldg16x2(v16i_t &a, const void *baseA, v16i_t &b, const void *baseB) {
    if (DESC) asm volatile("s_load_dwordx16 %0, %2, %4\n\ts_load_dwordx16 %1, %3, %5\n\ts_waitcnt lgkmcnt(0)" : "=&s"(a), "=&s"(b) : "s"(baseA), "s"(baseB), "n"(OFFA), "n"(OFFB) : "memory");
    else { __builtin_memcpy(&a, (const char *) baseA + OFFA, 64); __builtin_memcpy(&b, (const char *) baseB + OFFB, 64); }
}
#define GP(T, t16, i) ((T *) ((((unsigned long long) (unsigned) (t16)[2 * (i) + 1]) << 32) | (unsigned long long) (unsigned) (t16)[2 * (i)]))
#define OFF_B0 ((int) offsetof(BaPtrs, pgeo))
enum { BP_GEO = 0, BP_CW = 1, BP_RTAB = 2, BP_PHOST = 3, BP_JLIN = 4, BP_RTZ = 5 };      // indices of the BaPtrs pointers inside their group
#define OFF_S0 ((int) offsetof(ResSet, slot))
static_assert(offsetof(BaPtrs, chunk_n) == offsetof(BaPtrs, pgeo) + 56, "BaPtrs pointer group (ba_dev.h)");
static_assert(offsetof(ResSet, slot) == 0 && offsetof(ResSet, chunkEnergy) == 56 && offsetof(ResSet, chunkCnt) == 64, "ResSet pointer group (ba_dev.h)");
// indices of the ResSet pointers inside their group
enum { RS_SLOT = 0, RS_PT = 1, RS_ACC = 2, RS_CAND = 3, RS_G = 4, RS_TOPA = 5, RS_TOPL = 6, RS_CHUNKE = 7 };

// flat index of entry (r,c), r<=c, in the packed upper triangle of a 13x13 matrix
__host__ __device__ constexpr int tri13(int r, int c) { return r * 13 - (r * (r - 1)) / 2 + (c - r); }

// Everything a wave reads from HBM for one point besides the image taps.  Round 6: the records of a point are loaded TWO points ahead of the
// arithmetic that consumes them and its image taps ONE point ahead (software pipeline of linearize_body), so nothing of a point may sit in scalar
// registers while it waits (an outstanding s_load makes every LDS wait of the point in front of it a full lgkmcnt(0)): the 64-byte PtGeo and PtRec
// of the point arrive as ONE VGPR each (lane L holds dword L & 15 - the 16 lanes of a row read one 64-byte line, the four rows the same line) and
// are read out with v_readlane where they are used.
template <int NSG>
struct PtIn {
    float rgeo, rrec;             // dword (lane & 15) of the point's PtGeo / of its PtRec in the applied set
    float color, wgt;
    int rflat[NSG], rlin[NSG], rnew[NSG], rlidx[NSG];     // SlotTab of this lane's slot(s)
    float jp[NSG], m[NSG];        // this lane's pair of the slot record: JpJdF[k] and scalar k (LD_SM_*; integers as raw bits)
    const float *ls;              // where the point's records are parked in the wavefront's LDS (STASH, linearize_body): [64 lanes][rgeo, rrec, colour, weight] | [64 lanes][rflat, rlin, jp, m]
};
// dword i of a record held one-dword-per-lane (wave-uniform result: a scalar register).  Macros on purpose: through lane.h's lane_read (the same builtin as a
// function) the compiler schedules and allocates these kernels differently
#define RLF(v, i) __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, (v)), (i)))
#define RLI(v, i) __builtin_amdgcn_readlane(__builtin_bit_cast(int, (v)), (i))
// PtGeo dwords (ba_dev.h)
#define GEO_U 0
#define GEO_V 1
#define GEO_PRIOR 2
#define GEO_IDP 4
#define GEO_IDZ 5
#define GEO_STEP 6
// PtRec dwords (ba_dev.h)
#define REC_HDI 0
#define REC_BDSUM 1
#define REC_IDH 2
#define REC_NACT 3
#define REC_HCDA 4
#define REC_HCDL 8
#define REC_MAXRELBS 12
#define REC_NUMGOOD 13

// element i of a device array with the BYTE offset computed in 32 bits: base pointer (SGPR pair) + zero-extended
// lane offset is the addressing mode the hardware has (saddr + voffset); a 64-bit per-lane address costs two registers and a
// 64-bit shift-add per access.  Every table of a window is far below 4 GB.
// The pointers of a window are generic (flat) pointers to the compiler: accessed as such they become flat_load / flat_store, which have no
// scalar-base addressing mode (two v_mov + v_lshl_add_u64 per access to build a 64-bit VGPR address) and count against lgkmcnt as well as
// vmcnt (every s_waitcnt lgkmcnt(0) of a scalar load then waits for all vector memory traffic in flight).  Every table of a window is
// hipMalloc'ed device memory: the access is made through an address_space(1) (global) pointer -> global_load/store v, v_off, s[base].
template <class T> using gptr_t = __attribute__((address_space(1))) T *;
template <class T> static __device__ __forceinline__ __attribute__((address_space(1))) T &at_g(T *p, unsigned i) { return *(gptr_t<T>) ((gptr_t<char>) p + (size_t) (i * (unsigned) sizeof(T))); }
#define AT(ptr, i) (at_g((ptr), (unsigned) (i)))

typedef int v4i32_t __attribute__((ext_vector_type(4)));
typedef float v8f_t __attribute__((ext_vector_type(8)));
typedef int v2i32_t __attribute__((ext_vector_type(2)));
typedef float v2f_t __attribute__((ext_vector_type(2)));
typedef float v4f_t __attribute__((ext_vector_type(4)));

// The record of one point as a wavefront needs it: one dword of its PtGeo and of its PtRec per lane, this lane's (colour, weight) pair (one
// dwordx2), and per slot group one dwordx2 / dwordx4 (SlotTab, the same 16 bytes for the 8 lanes of a slot) and one dwordx2 (this lane's pair of
// the 64-byte SlotRec): 3 + 2 NSG vector loads, no scalar load.
template <int NSG, bool HAS_L, bool FIX, bool DESC>
static __device__ __forceinline__ void load_point(PtIn<NSG> &q, const BaPtrs &B, const ResSet &cur, unsigned FS, unsigned p, unsigned s, unsigned k, unsigned lane) {
    const unsigned pU = (unsigned) __builtin_amdgcn_readfirstlane((int) p);
    {
        const v16i_t b0 = ldg16<DESC, OFF_B0>(&B);
        const float *geo = GP(const float, b0, BP_GEO);
        const v2f_t *pcw = GP(const v2f_t, b0, BP_CW);
        const v4i32_t *rtab = GP(const v4i32_t, b0, BP_RTAB);
        // addresses = (uniform base advanced to the point, on the scalar side) + (a lane offset that never changes)
        q.rgeo = AT(geo + (size_t) pU * (sizeof(PtGeo) / 4), lane & 15u);
        const v2f_t cw = AT(pcw + (size_t) pU * 8, k);
        q.color = cw.x; q.wgt = cw.y;
#pragma unroll
        for (int g = 0; g < NSG; g++) {
            // slot tables are dense [P][FS]: every index is readable.  Only the half of the entry this variant uses is loaded
            if constexpr (FIX || HAS_L) {
                const v4i32_t t4 = AT(rtab + (size_t) pU * FS, g * 8 + s);
                q.rflat[g] = t4.x; q.rlin[g] = t4.y; q.rnew[g] = FIX ? t4.z : 0; q.rlidx[g] = HAS_L ? t4.w : 0;
            } else {
                const v2i32_t t2 = AT((const v2i32_t *) (rtab + (size_t) pU * FS), (g * 8 + s) * 2);
                q.rflat[g] = t2.x; q.rlin[g] = t2.y; q.rnew[g] = 0; q.rlidx[g] = 0;
            }
        }
    }
    {
        const v16i_t s0 = ldg16<DESC, OFF_S0>(&cur);
        const v2f_t *slots = GP(const v2f_t, s0, RS_SLOT);
        const float *pts = GP(const float, s0, RS_PT);
        q.rrec = AT(pts + (size_t) pU * (sizeof(PtRec) / 4), lane & 15u);
#pragma unroll
        for (int g = 0; g < NSG; g++) {
            const v2f_t e = AT(slots + (size_t) pU * FS * 8, (g * 8 + s) * 8 + k);
            q.jp[g] = e.x; q.m[g] = e.y;
        }
    }
}

// Pair mode (round 6, windows of 9..12 key frames): the second slot group of such a window uses 4 of its 8 slots, so TWO points share its pass - lanes 0..31 work on the
// targets 8..11 of point A, lanes 32..63 on the targets 8..11 of point B (3 passes per 2 points instead of 4).  The records of a pair: PtGeo / PtRec with A in lanes
// 0..31 and B in lanes 32..63 (dword lane & 15), both points' colours / weights, the first group's slot records of A and of B, the shared second group's.
struct PairIn {
    float rgeo, rrec, colA, wgtA, colB, wgtB;
    int rfA0, rfB0, rf1;
    float jpA0, mA0, jpB0, mB0, jp1, m1;
};
template <bool DESC>
static __device__ __forceinline__ void load_pair(PairIn &q, const BaPtrs &B, const ResSet &cur, unsigned FS, unsigned pA, unsigned dAB, unsigned s, unsigned k, unsigned lane) {
    const unsigned pU = (unsigned) __builtin_amdgcn_readfirstlane((int) pA), dU = (unsigned) __builtin_amdgcn_readfirstlane((int) dAB);
    const unsigned hoff = (lane & 32u) ? dU : 0u;          // this lane's point, relative to A
    const unsigned s1 = 8u + (s & 3u);                     // this lane's slot of the shared second group
    {
        const v16i_t b0 = ldg16<DESC, OFF_B0>(&B);
        const float *geo = GP(const float, b0, BP_GEO);
        const v2f_t *pcw = GP(const v2f_t, b0, BP_CW);
        const v2i32_t *rtab = (const v2i32_t *) GP(const v4i32_t, b0, BP_RTAB);          // two dwordx2 per 16-byte entry: {rflat, rlin} first
        q.rgeo = AT(geo + (size_t) pU * (sizeof(PtGeo) / 4), hoff * (unsigned) (sizeof(PtGeo) / 4) + (lane & 15u));
        const v2f_t ca = AT(pcw + (size_t) pU * 8, k), cb = AT(pcw + (size_t) pU * 8, dU * 8u + k);
        q.colA = ca.x; q.wgtA = ca.y; q.colB = cb.x; q.wgtB = cb.y;
        q.rfA0 = AT(rtab + (size_t) pU * FS * 2, s * 2u).x;
        q.rfB0 = AT(rtab + (size_t) pU * FS * 2, (dU * FS + s) * 2u).x;
        q.rf1 = AT(rtab + (size_t) pU * FS * 2, (hoff * FS + s1) * 2u).x;
    }
    {
        const v16i_t s0 = ldg16<DESC, OFF_S0>(&cur);
        const v2f_t *slots = GP(const v2f_t, s0, RS_SLOT);
        const float *pts = GP(const float, s0, RS_PT);
        q.rrec = AT(pts + (size_t) pU * (sizeof(PtRec) / 4), hoff * (unsigned) (sizeof(PtRec) / 4) + (lane & 15u));
        const v2f_t a0 = AT(slots + (size_t) pU * FS * 8, s * 8u + k), b0_ = AT(slots + (size_t) pU * FS * 8, (dU * FS + s) * 8u + k);
        const v2f_t p1 = AT(slots + (size_t) pU * FS * 8, (hoff * FS + s1) * 8u + k);
        q.jpA0 = a0.x; q.mA0 = a0.y; q.jpB0 = b0_.x; q.mB0 = b0_.y; q.jp1 = p1.x; q.m1 = p1.y;
    }
}

