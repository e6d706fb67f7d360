// ba_solve_batch.hip — the reduce and control kernels of a batch of windows (gfx950, ldso_ba_batch_optimize): the bodies of ba_reduce_body.h and
// ba_solve_body.h, one launch for all windows, the descriptors (BatchItem) in device memory.  The single-window kernels are ba_solve.hip.
#include <hip/hip_runtime.h>
#include "ba_host.h"

#include "ba_reduce_body.h"          // before ba_solve_body.h: it names a template parameter NT
#include "ba_solve_body.h"

// ---------------------------------------------------------------------------------------------------------
// Batched windows: k_reduce and the control step of nWin independent windows, one launch each (the fused k_reduce_solve needs
// every workgroup of a window resident at once - with many windows per launch a kernel boundary orders the two instead).
// ---------------------------------------------------------------------------------------------------------
// Two register allocations of the same kernel.  Its workgroups are latency-bound (each lives ~10 us whatever the load), so for a launch
// that queues many of them per CU residency is throughput, while a launch that fits the chip in one go only sees the spill code.  Measured,
// B = 32 (2080 workgroups per half-batch launch, 8 per CU): 3 per CU (132 VGPRs, the unconstrained allocation) and 4 (126) 101.4 k
// window-iterations/s, 5 (96 VGPRs, 30 spilled; also fits beside the two resident k_linearize_batch wavefronts of a SIMD, 2 x 205 + 96 <= 512, so
// the reduce of one half-batch overlaps the linearisation of the other) 104.8 k, 6 (80 VGPRs, 48 spilled) 83.0 k; B = 8 (520 workgroups per
// launch, 2 per CU): 82 k unconstrained, 75.7 k with the 96-register allocation (different boxes, same day).
#define LD_REDB_BLOCKS 4             // the dense variant: workgroups per CU its register allocation leaves room for (round 4, against the record-layout
                                     // k_linearize_batch of 187 VGPRs, B = 32 different windows: 3 -> 122.4 k, 4 -> 122.4 k, 5 -> 96.8 k, 6 -> 87.5 k window-iterations/s,
                                     // unconstrained 107.8 k; with round 3's 205-VGPR kernel 5 had been the best: 104.8 k)
#define LD_REDB_DENSE_PER_CU 6       // launches with at least this many workgroups per CU take the dense variant
static __device__ __forceinline__ void reduce_batch_body(const BatchItem *__restrict__ items, int nWin, int cur, float calibPrior, double l1, double il, int itCheck) {
    int w = 0;
    for (int i = 1; i < nWin; i++) if ((int) blockIdx.x >= items[i].redBlock0) w = i;
    const BatchItem &it = items[w];
    reduce_body<RT_STAGED>(it.B, it.D, it.set[cur], it.cs, 0, it.GSP, 1, it.hasPrior, calibPrior, l1, il, itCheck, (int) blockIdx.x - it.redBlock0);
}
__global__ __launch_bounds__(NT) void k_reduce_batch(const BatchItem *__restrict__ items, int nWin, int cur, float calibPrior, double l1, double il, int itCheck) {
    reduce_batch_body(items, nWin, cur, calibPrior, l1, il, itCheck);
}
__global__ __launch_bounds__(NT, LD_REDB_BLOCKS) void k_reduce_batch_dense(const BatchItem *__restrict__ items, int nWin, int cur, float calibPrior, double l1, double il, int itCheck) {
    reduce_batch_body(items, nWin, cur, calibPrior, l1, il, itCheck);
}

// logIdx / itCheck >= 0: an iteration of ldso_ba_batch_optimize (energy log entry of the previous linearisation; un-forced: the window's own LD_SC_STOP decides
// whether its two workgroups still have work)
__global__ __launch_bounds__(NT) void k_gn_solve_batch(const BatchItem *__restrict__ items, int cur, ldso_settings_t St, int iteration, double lambda, int logIdx, int itCheck) {
    const BatchItem &it = items[blockIdx.x >> 1];
    SolveArgs A;
    A.iteration = iteration; A.lambda = lambda; A.hasPrior = it.hasPrior; A.GSP = it.GSP; A.logIdx = logIdx; A.itCheck = itCheck;
    gn_solve_body<false>(it.B, it.D, it.set[cur], St, A, (int) (blockIdx.x & 1));
}

// ---- ldso_ba_batch_optimize: what surrounds the iterations --------------------------------------------------------------------------------------------
// A window of a batched optimize() stops on its own: scalars[LD_SC_STOP] starts at (its iteration cap - 1) and canbreak only lowers it (gn_tail), so it always
// names the LAST iteration the window executes - the per-window cap and the early exit are the same test (LD_ITER_SKIPPED), and the tail derives from it,
// on the device, how many iterations ran and which of the window's two residual sets is the applied one.  set[0] of a BatchItem is the set that was applied
// when the call began (batch_refresh): the preamble linearises set[0] -> set[1], iteration i reads set[1 ^ (i & 1)].
__global__ __launch_bounds__(64) void k_batch_begin(const BatchItem *__restrict__ items, int mnumOptIts, int forceAll) {
    const BatchItem &it = items[blockIdx.x];
    it.B.energyLog[threadIdx.x] = 0.0;
    if (threadIdx.x == 0) it.B.scalars[LD_SC_STOP] = (double) (optimize_iteration_cap(it.D.F, mnumOptIts, forceAll) - 1);
}
// The tail of optimize() for every window of a (half-)batch.  phase 0 (two workgroups per window): flags on the applied set, log entry `done`; phase 1 (one
// workgroup per window): flags on the set the fixing linearisation wrote, log entry `done + 1`, then the window's 16 scalars into the batch's read-back block.
__global__ __launch_bounds__(NT) void k_solve_batch(const BatchItem *__restrict__ items, ldso_settings_t St, unsigned flags, int phase, int nRoles, double *__restrict__ scalarsOut) {
    const int w = (int) blockIdx.x / nRoles, role = (int) blockIdx.x % nRoles;
    const BatchItem &it = items[w];
    const int stop = (int) it.B.scalars[LD_SC_STOP], applied = stop & 1;          // = 1 ^ (done & 1), done = stop + 1
    SolveArgs A;
    A.flags = flags; A.hasPrior = it.hasPrior; A.GSP = it.GSP; A.logIdx = stop + 1 + phase;
    solve_body(it.B, it.D, it.set[applied ^ phase], St, A, nRoles, role);
    if (scalarsOut != nullptr) {
        __syncthreads();
        if (threadIdx.x < 16) scalarsOut[(size_t) it.outSlot * 16 + threadIdx.x] = it.B.scalars[threadIdx.x];
    }
}

hipError_t ba_launch_reduce_batch(const BatchItem *d_items, int nWin, int totalBlocks, int cur, float calibPrior, double l1, double il, hipStream_t st, int itCheck) {
    static int numCU[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    if (numCU[dev] == 0) { int cu = 0; if (hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cu <= 0) cu = 256; numCU[dev] = cu; }
    return launch_lds(totalBlocks >= LD_REDB_DENSE_PER_CU * numCU[dev] ? k_reduce_batch_dense : k_reduce_batch, dim3(totalBlocks), dim3(NT), reduce_atomic_lds_bytes(RT_STAGED), st,
                      d_items, nWin, cur, calibPrior, l1, il, itCheck);
}

// Dmax: the window of the batch with the most frames.  It sizes the LDS of the launch; every window lays itself out by its own F (lds_layouts_ok: none needs more)
hipError_t ba_launch_gn_solve_batch(const BatchItem *d_items, int nWin, const BaDims &Dmax, int cur, const ldso_settings_t &St, int iteration, double lambda, hipStream_t st, int logIdx, int itCheck) {
    return launch_lds(k_gn_solve_batch, dim3(2 * nWin), dim3(NT), gn_lds_bytes(Dmax.F, Dmax.n), st, d_items, cur, St, iteration, lambda, logIdx, itCheck);
}

hipError_t ba_launch_batch_begin(const BatchItem *d_items, int nWin, int mnumOptIts, int forceAll, hipStream_t st) {
    hipLaunchKernelGGL(k_batch_begin, dim3(nWin), dim3(64), 0, st, d_items, mnumOptIts, forceAll);
    return hipGetLastError();
}

hipError_t ba_launch_solve_batch(const BatchItem *d_items, int nWin, const BaDims &Dmax, const ldso_settings_t &St, unsigned flags, int phase, double *d_scalarsOut, hipStream_t st) {
    const int nRoles = solve_roles(flags);
    return launch_lds(k_solve_batch, dim3(nRoles * nWin), dim3(NT), solve_lds_bytes(Dmax.n), st, d_items, St, flags, phase, nRoles, d_scalarsOut);
}
