// ba_linearize.hip — the linearisation kernels of ONE window and their launchers (gfx950): k_linearize (the descriptor in the kernel arguments, every variant of
// linearizeAll and the marginalisation accumulate) and k_linearize_one (the Gauss-Newton iteration).  The arithmetic is linearize_body (ba_linearize_body.h); the
// kernels of a batch of windows are in ba_linearize_batch.hip.
#include <hip/hip_runtime.h>
#include "ba_host.h"
#include "ba_linearize_body.h"

template <int NSG, bool HAS_L, bool FIX, bool MARG>
__global__ __launch_bounds__(64 * LD_WAVES) void k_linearize(BaPtrs B, BaDims D, ResSet cur, ResSet nxt, ldso_settings_t S, int stepMode, GnInit gi,
                                                             const int32_t *__restrict__ margFlags) {
    static_assert(sizeof(BaPtrs) + sizeof(BaDims) + 2 * sizeof(ResSet) + sizeof(ldso_settings_t) + sizeof(GnInit) + 256 >= 14 * 64 - 60, "k_linearize: ld_touch_kernarg<14> must stay inside the explicit arguments + the 256 bytes of hidden arguments behind them (the kernel uses dynamic LDS: the whole hidden block is part of its kernarg segment)");
    ld_touch_kernarg<14>();          // 952 bytes of arguments into the scalar cache with one wait (ba_dev.h)
    const int chunk = (int) blockIdx.x;
    linearize_body<NSG, HAS_L, FIX, MARG, false>(B, D, cur, nxt, S, stepMode, gi, margFlags, chunk, (int) gridDim.x, B.chunk_p0[chunk], B.chunk_n[chunk], B.chunk_host[chunk]);
}

// The GN-iteration linearisation of ONE window with everything a workgroup needs before its first operand load in the KERNEL ARGUMENTS: the whole
// descriptor (BaPtrs / BaDims / the two residual sets) by value - it stays in the kernarg segment, the body fetches its pointer groups from there just
// in time exactly as from a BatchItem in device memory (DESC = true: `&B` is an address in the constant kernarg segment) - and the chunk of the
// workgroup computed from the by-value host tables of LinHead instead of a table entry in memory.  The prologue of this kernel is a chain of dependent
// memory levels and nothing else (window of 5 MB on a chip that moves that in 0.7 us): kernel arguments -> workgroup table entry -> descriptor ->
// operands -> LDS was four levels (k_linearize_batch<NSG, false>), this is two.
struct OneArgs { BaPtrs B; BaDims D; ResSet cur, nxt; ldso_settings_t S; int stepMode; GnInit gi; LinHead hd; };
template <int NSG, bool PAIR = false>
__global__ __launch_bounds__(64 * LD_WAVES) void k_linearize_one(OneArgs a) {
    // The descriptor is addressed IN the kernarg segment (the only parameter starts at its offset 0): taking the address of the by-value parameter
    // itself would make the compiler copy it to scratch memory (536 bytes per lane, and a scalar load from a private address is meaningless).
    const OneArgs &A = *(const OneArgs *) __builtin_amdgcn_kernarg_segment_ptr();
    static_assert(sizeof(OneArgs) >= 12 * 64 && sizeof(OneArgs) <= 16 * 64, "k_linearize_one: 16 lines = the explicit arguments (>= 768 bytes) + the 256 bytes of hidden arguments behind them");
    ld_touch_kernarg<16>();          // the whole argument block into the scalar cache with one wait (ba_dev.h): 10.6 -> 9.9 us at C3, 43.0 -> 42.3 us at C5
    const LinHead &hd = a.hd;
    const int chunk = (int) blockIdx.x;
    int h = 0;
#pragma unroll
    for (int i = 1; i < LD_MAXF; i++) h += (i < hd.F && chunk >= hd.cs[i]) ? 1 : 0;          // hosts without points have cs[i] == cs[i + 1]: they are skipped
    int c0 = 0, q0 = 0, q1 = 0;
#pragma unroll
    for (int i = 0; i < LD_MAXF; i++) { const bool m = (i == h); c0 = m ? hd.cs[i] : c0; q0 = m ? hd.hostP0[i] : q0; q1 = m ? hd.hostP0[i + 1] : q1; }
    const int p0 = q0 + (chunk - c0) * hd.CH, np = min(hd.CH, q1 - p0);
    linearize_body<NSG, false, false, false, true, true, PAIR>(A.B, A.D, A.cur, A.nxt, a.S, a.stepMode, a.gi, nullptr, chunk, (int) gridDim.x, p0, np, h);
}

// ---------------------------------------------------------------------------------------------------------
// launcher
// ---------------------------------------------------------------------------------------------------------
template <int NSG, bool HAS_L, bool FIX, bool MARG = false>
static hipError_t launch_one(const BaPtrs &B, const BaDims &D, const ResSet &cur, const ResSet &nxt, const ldso_settings_t &S, int stepMode, const GnInit &gi, hipStream_t st,
                            const int32_t *margFlags = nullptr) {
    return launch_lds(k_linearize<NSG, HAS_L, FIX, MARG>, dim3(D.nChunks), dim3(64 * LD_WAVES), ba_linearize_lds_bytes(D.FS, HAS_L), st, B, D, cur, nxt, S, stepMode, gi, margFlags);
}

// (nsg, hasL, fix) -> the instantiation of k_linearize, one run-time choice per level
template <int NSG, bool HAS_L>
static hipError_t launch_fix(bool fix, const BaPtrs &B, const BaDims &D, const ResSet &cur, const ResSet &nxt, const ldso_settings_t &S, int stepMode, const GnInit &gi, hipStream_t st) {
    return fix ? launch_one<NSG, HAS_L, true>(B, D, cur, nxt, S, stepMode, gi, st) : launch_one<NSG, HAS_L, false>(B, D, cur, nxt, S, stepMode, gi, st);
}
template <int NSG>
static hipError_t launch_hasl(bool hasL, bool fix, const BaPtrs &B, const BaDims &D, const ResSet &cur, const ResSet &nxt, const ldso_settings_t &S, int stepMode, const GnInit &gi, hipStream_t st) {
    return hasL ? launch_fix<NSG, true>(fix, B, D, cur, nxt, S, stepMode, gi, st) : launch_fix<NSG, false>(fix, B, D, cur, nxt, S, stepMode, gi, st);
}

hipError_t ba_launch_linearize(const BaPtrs &B, const BaDims &D, const ResSet &cur, const ResSet &nxt, const ldso_settings_t &S,
                               bool hasL, bool fix, int stepMode, const GnInit &gi, hipStream_t st) {
    if (D.nChunks == 0) return hipSuccess;
    return (D.nsg == 1) ? launch_hasl<1>(hasL, fix, B, D, cur, nxt, S, stepMode, gi, st) : launch_hasl<2>(hasL, fix, B, D, cur, nxt, S, stepMode, gi, st);
}

hipError_t ba_launch_linearize_one(const BaPtrs &B, const BaDims &D, const ResSet &cur, const ResSet &nxt, const ldso_settings_t &S, int stepMode, const GnInit &gi, const LinHead &hd,
                                   hipStream_t st) {
    if (D.nChunks == 0) return hipSuccess;
    const size_t lds = ba_linearize_lds_bytes(D.FS, false);
    OneArgs a;
    a.B = B; a.D = D; a.cur = cur; a.nxt = nxt; a.S = S; a.stepMode = stepMode; a.gi = gi; a.hd = hd;
    const dim3 grid(D.nChunks), block(64 * LD_WAVES);
    if (D.nsg == 1) return launch_lds(k_linearize_one<1>, grid, block, lds, st, a);
    // 9..12 key frames: the second slot group uses 4 of its 8 slots - two points share its pass (pair mode, round 6)
    if (D.F <= 12) return launch_lds(k_linearize_one<2, true>, grid, block, lds, st, a);
    return launch_lds(k_linearize_one<2>, grid, block, lds, st, a);
}

// marginalizePointsF accumulate for the flagged points (see the MARG note at linearize_body); `nxt` is scratch
hipError_t ba_launch_linearize_marg(const BaPtrs &B, const BaDims &D, const ResSet &cur, const ResSet &nxt, const ldso_settings_t &S, const int32_t *margFlags,
                                    hipStream_t st) {
    if (D.nChunks == 0) return hipSuccess;
    const GnInit gi{0, 0, 0.0f};
    if (D.nsg == 1) return launch_one<1, false, false, true>(B, D, cur, nxt, S, 0, gi, st, margFlags);
    return launch_one<2, false, false, true>(B, D, cur, nxt, S, 0, gi, st, margFlags);
}

