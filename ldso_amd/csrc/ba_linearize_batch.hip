// ba_linearize_batch.hip — the linearisation kernels of a batch of windows and their launchers (gfx950): k_linearize_batch (the Gauss-Newton iteration),
// k_linearize_batch_fix (linearizeAll(true)) and k_linearize_batch_marg (the marginalisation accumulate).  The arithmetic is linearize_body (ba_linearize_body.h),
// fed from descriptors in device memory; the kernels of one window are in ba_linearize.hip.
#include <hip/hip_runtime.h>
#include "ba_host.h"
#include "ba_linearize_body.h"

// Batched windows (one 7-keyframe window is tiny for the chip): the chunks of nWin independent windows in one
// launch.  Workgroup -> window by the block table (BatchBlock::win); `cur` = which residual set is read, RELATIVE to every window's own applied set
// (BatchItem::set[0], see batch_refresh: the windows of a batch need not be at the same ping-pong parity, and with itCheck >= 0 each stops on its own).
template <int NSG>
__global__ __launch_bounds__(64 * LD_WAVES) void k_linearize_batch(const BatchItem *__restrict__ items, const BatchBlock *__restrict__ blocks, const int32_t *__restrict__ wgStart, int cur,
                                                                   ldso_settings_t S, int stepMode, float calibPrior, int itCheck) {
    // wgStart != nullptr (round 6): this workgroup works through the blocks [wgStart[w], wgStart[w + 1]) - ldso_ba_batch_create cut the windows so that every
    // workgroup of the launch (one per CU) carries the same load; nullptr: one block per workgroup
    int b0 = (int) blockIdx.x, b1 = b0 + 1;
    if (wgStart != nullptr) { b0 = wgStart[blockIdx.x]; b1 = wgStart[blockIdx.x + 1]; }
#pragma clang loop unroll(disable)
    for (int b = b0; b < b1; b++) {
        const BatchBlock bb = blocks[b];                            // one scalar 16-byte load: window, first point, point count, host | chunk
        const BatchItem &it = items[bb.win];
        GnInit gi; gi.enable = 1; gi.hasPrior = it.hasPrior; gi.calibPrior = calibPrior; gi.itCheck = itCheck;
        linearize_body<NSG, false, false, false, true>(it.B, it.D, it.set[cur], it.set[cur ^ 1], S, stepMode, gi, nullptr, bb.host_chunk >> 8, it.D.nChunks, bb.p0, bb.np, bb.host_chunk & 0xFF);
        __syncthreads();                                            // the next block re-uses the operand / reduction LDS
    }
}

// linearizeAll(true) at the end of a batched optimize() (ldso_ba_batch_optimize), one slot group per point: every window reads ITS applied set, which the parity
// of its own last executed iteration names (scalars[LD_SC_STOP], see k_solve_batch in ba_solve_batch.hip), and writes the other one.
__global__ __launch_bounds__(64 * LD_WAVES) void k_linearize_batch_fix(const BatchItem *__restrict__ items, const BatchBlock *__restrict__ blocks, const int32_t *__restrict__ wgStart,
                                                                       ldso_settings_t S, float calibPrior) {
    int b0 = (int) blockIdx.x, b1 = b0 + 1;
    if (wgStart != nullptr) { b0 = wgStart[blockIdx.x]; b1 = wgStart[blockIdx.x + 1]; }
#pragma clang loop unroll(disable)
    for (int b = b0; b < b1; b++) {
        const BatchBlock bb = blocks[b];
        const BatchItem &it = items[bb.win];
        const int applied = __builtin_amdgcn_readfirstlane((int) it.B.scalars[LD_SC_STOP]) & 1;          // wave-uniform: the body fetches the sets' pointer groups with scalar loads
        GnInit gi; gi.enable = 1; gi.hasPrior = it.hasPrior; gi.calibPrior = calibPrior; gi.itCheck = -1;
        linearize_body<1, false, true, false, true>(it.B, it.D, it.set[applied], it.set[applied ^ 1], S, 0, gi, nullptr, bb.host_chunk >> 8, it.D.nChunks, bb.p0, bb.np, bb.host_chunk & 0xFF);
        __syncthreads();
    }
}

// The marginalizePointsF accumulate (MARG, see linearize_body) of every window of a batch that takes part in ldso_ba_batch_marginalize_points: each window reads its
// applied set (BatchItem::set[0]) and writes its scratch set, one slot group per point; its flags start at flagsAll + mw[window].flagOff.  The blocks of a window
// that takes no part are passed over.  Per point and per chunk the arithmetic of k_linearize<1, false, false, true>.
__global__ __launch_bounds__(64 * LD_WAVES) void k_linearize_batch_marg(const BatchItem *__restrict__ items, const BatchBlock *__restrict__ blocks, const int32_t *__restrict__ wgStart,
                                                                        const MargWin *__restrict__ mw, const int32_t *__restrict__ flagsAll, ldso_settings_t S) {
    int b0 = (int) blockIdx.x, b1 = b0 + 1;
    if (wgStart != nullptr) { b0 = wgStart[blockIdx.x]; b1 = wgStart[blockIdx.x + 1]; }
#pragma clang loop unroll(disable)
    for (int b = b0; b < b1; b++) {
        const BatchBlock bb = blocks[b];
        const MargWin m = mw[bb.win];
        if (!m.active) continue;                                    // (workgroup-uniform: nobody of this workgroup is inside the body, no barrier is skipped by a part of it)
        const BatchItem &it = items[bb.win];
        GnInit gi; gi.enable = 0; gi.hasPrior = 0; gi.calibPrior = 0.0f; gi.itCheck = -1;
        linearize_body<1, false, false, true, true>(it.B, it.D, it.set[0], it.set[1], S, 0, gi, flagsAll + m.flagOff, bb.host_chunk >> 8, it.D.nChunks, bb.p0, bb.np, bb.host_chunk & 0xFF);
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------------------
// One workgroup per entry of the balanced table (d_wgStart: nWG workgroups) or, without it, per chunk; nothing to do is no launch.  Every batched kernel begins with
// (items, blocks, wgStart) and uses the record stash.
template <class Kernel, class... Args>
static hipError_t launch_batch(Kernel kernel, int FS, const BatchItem *d_items, const BatchBlock *d_blocks, int totalChunks, const int32_t *d_wgStart, int nWG, hipStream_t st, const Args &... args) {
    if (totalChunks == 0) return hipSuccess;
    const int grid = d_wgStart != nullptr ? nWG : totalChunks;
    if (grid <= 0) return hipSuccess;
    return launch_lds(kernel, dim3(grid), dim3(64 * LD_WAVES), ba_linearize_lds_bytes(FS, false, true), st, d_items, d_blocks, d_wgStart, args...);
}

hipError_t ba_launch_linearize_batch(const BatchItem *d_items, const BatchBlock *d_blocks, int totalChunks, const int32_t *d_wgStart, int nWG, int FS, int cur, const ldso_settings_t &S, int stepMode,
                                     float calibPrior, hipStream_t st, int itCheck) {
    if (FS == 8) return launch_batch(k_linearize_batch<1>, FS, d_items, d_blocks, totalChunks, d_wgStart, nWG, st, cur, S, stepMode, calibPrior, itCheck);
    return launch_batch(k_linearize_batch<2>, FS, d_items, d_blocks, totalChunks, d_wgStart, nWG, st, cur, S, stepMode, calibPrior, itCheck);
}

// ldso_ba_batch_marginalize_points: windows of at most 8 key frames (the caller has checked)
hipError_t ba_launch_linearize_batch_marg(const BatchItem *d_items, const BatchBlock *d_blocks, int totalChunks, const int32_t *d_wgStart, int nWG, const MargWin *d_mw, const int32_t *d_flags,
                                          const ldso_settings_t &S, hipStream_t st) {
    return launch_batch(k_linearize_batch_marg, 8, d_items, d_blocks, totalChunks, d_wgStart, nWG, st, d_mw, d_flags, S);
}

hipError_t ba_launch_linearize_batch_fix(const BatchItem *d_items, const BatchBlock *d_blocks, int totalChunks, const int32_t *d_wgStart, int nWG, const ldso_settings_t &S, float calibPrior, hipStream_t st) {
    return launch_batch(k_linearize_batch_fix, 8, d_items, d_blocks, totalChunks, d_wgStart, nWG, st, S, calibPrior);
}
