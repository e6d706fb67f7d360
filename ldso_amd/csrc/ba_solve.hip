// ba_solve.hip — the "control" side of a Gauss-Newton iteration (gfx950): everything the reference does sequentially on
// the host between two residual passes, so that an iteration needs no host synchronisation.
//
// The single-window control kernels; they share the bodies of ba_solve_body.h with the batched ones (ba_solve_batch.hip):
//   k_gn_solve      the forced-accept fast path (ldso_ba_optimize / ldso_ba_enqueue_gn / ldso_ba_gn_solve_reduced): two concurrent
//                   workgroups - block 0: solve_core (+ backupState, doStepFromBackup, canbreak, setPrecalcValues) on an LDS mirror of
//                   the frames; block 1: statistics of the previous linearizeAll (energy sums, setNewFrameEnergyTH, energy log).
//   k_reduce_solve  k_reduce and k_gn_solve of one iteration in one launch (the single-GPU fast path)
//   k_solve         one workgroup, flag-selected pieces for the step-wise C entry points (LM rejection, debugging, old multi-GPU path):
//                   the SK_ flags, see solve_body
// The kernels that never touch the solver (point step, LM energies, multi-GPU export) are ba_step.hip.
#include <hip/hip_runtime.h>
#include "ba_host.h"

#include "ba_reduce_body.h"          // before ba_solve_body.h: it names a template parameter NT
#include "ba_solve_body.h"

__global__ __launch_bounds__(NT) void k_solve(BaPtrs B, BaDims D, ResSet S, ldso_settings_t St, SolveArgs A) {
    solve_body(B, D, S, St, A, (int) gridDim.x, (int) blockIdx.x);
}

// ---------------------------------------------------------------------------------------------------------
// k_gn_solve — the control step of ONE forced-accept Gauss-Newton iteration, two concurrent workgroups:
//   block 0 (critical path): solve_core + backupState + doStepFromBackup + setPrecalcValues, working on an LDS
//            mirror of the frames / calibration that is written back once at the end;
//   block 1 (statistics of the previous linearizeAll): energy sums, setNewFrameEnergyTH, energy log.
// The two blocks touch disjoint data: block 0 never reads frameEnergyTH (the linearize kernel takes the pair
// maximum itself) and skips that word in its write-back; canbreak's sumNID is recomputed from the chunk sums.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void k_gn_solve(BaPtrs B, BaDims D, ResSet S, ldso_settings_t St, SolveArgs A) {
    // the 672 bytes of arguments into the scalar cache with one wait (ba_dev.h) - for the systems up to 64 x 64 only: measured (round 4, A/B on one box)
    // 27.2 -> 26.5 us at C3 (n = 60), but 62.1 -> 63.6 us at C5 (n = 100, the generic factorisation)
    static_assert(sizeof(BaPtrs) + sizeof(BaDims) + sizeof(ResSet) + sizeof(ldso_settings_t) + sizeof(SolveArgs) >= 10 * 64 - 60, "k_gn_solve: ld_touch_kernarg<10> must stay inside the arguments");
    if (LD_SOLVE_NB(D.n) == 4) ld_touch_kernarg<10>();
    gn_solve_body<false>(B, D, S, St, A, (int) blockIdx.x);
}

// ---------------------------------------------------------------------------------------------------------
// k_reduce_solve — k_reduce and k_gn_solve of one GN iteration in ONE launch (single-GPU fast path): workgroup 0 is the control
// step, workgroup 1 the statistics, workgroups 2.. the reduce workgroups.  The control workgroup stages everything that does not
// depend on the system (frames, calibration, adjoints, nullspace projector, LDS set-up) while the reduce workgroups run, waits
// until all of them have arrived and only then loads HFinal / bFinal.  An arrival is one atomic increment once the workgroup's data atomics are acknowledged, on
// one of LD_ARRIVE_SHARDS words chosen by dispatch index (ba_dev.h: arrive_shard - the tile workgroups of a 7-frame launch arrive faster than a single word takes
// atomics); lane s of the control workgroup's first wavefront polls word s for its share of the arrivers (arrive_target), re-arms it, and an acquire fence
// follows the workgroup barrier.  This removes one kernel boundary and hides the launch-to-first-data latency of the control
// step (about 5 us of a 50 us iteration).  All workgroups of the launch are resident at once (F*F + 4*tiles + 3 <= 256 CUs), and the
// waiting workgroup has the lowest index, so it never keeps a producer from being scheduled.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void k_reduce_solve(BaPtrs B, BaDims D, ResSet S, ldso_settings_t St, SolveArgs A, ChunkStarts chunkStart, int atomicMode,
                                                     float calibPrior, double l1, double il) {
    static_assert(sizeof(BaPtrs) + sizeof(BaDims) + sizeof(ResSet) + sizeof(ldso_settings_t) + sizeof(SolveArgs) + sizeof(ChunkStarts) + 24 >= 12 * 64 - 60, "k_reduce_solve: ld_touch_kernarg<12> must stay inside the arguments");
    ld_touch_kernarg<12>();          // 768 bytes of arguments into the scalar cache with one wait (ba_dev.h): 31.8 -> 31.25 us at C3
    if (blockIdx.x >= LD_FUSED_CTL) {
        const long long tStart_ = LD_STAMP_ON ? wall_clock64() : 0;
        if (LD_ITER_SKIPPED(B, A.itCheck)) return;
        // dispatch order = index order: the Schur tile workgroups (the longest) get the lowest indices, then the pair workgroups,
        // the extras workgroup last; reduce_body numbers them pairs | tiles | extras
        const ReduceGrid rg = reduce_grid(D.F, A.hasL, D.ks, A.GSP);
        const int q = (int) blockIdx.x - LD_FUSED_CTL;
        const int bid = (q < rg.nTile) ? rg.nPair + q : (q < rg.nTile + rg.nPair) ? q - rg.nTile : q;
        reduce_body<RT_DIRECT>(B, D, S, chunkStart, A.hasL, A.GSP, atomicMode, A.hasPrior, calibPrior, l1, il, -1, bid);
        // Everything a reduce workgroup hands to the control workgroup went through device-scope atomics (performed at the memory
        // side): waiting for their acknowledgement is enough - a release FENCE would also write the whole L2 back (the outputs of
        // the previous k_linearize are still dirty there), which costs more than the kernel boundary this fusion removes.
        __builtin_amdgcn_s_waitcnt(0);
        __syncthreads();
        if (threadIdx.x == 0) {
            // stamps builds: one record per reduce workgroup in B.pairC (idle in atomic mode) - started | data atomics acknowledged (every wave's wait, behind the
            // barrier) | arrival atomic returned; the comparison makes the last stamp wait for the returned value (scripts/reduce_chain_stamps.py)
            double *rec = B.pairC + 3 * q;
            const bool recOk = LD_STAMP_ON && 3 * q + 2 < 2 * D.F * D.F * LD_PAIRC;
            if (recOk) { rec[0] = (double) tStart_; rec[1] = (double) wall_clock64(); }
            // the arrival: one of LD_ARRIVE_SHARDS words by dispatch index, so that workgroups that finish together do not queue on one word (ba_dev.h);
            // nobody reads the returned value outside stamps builds
            const int prev = __hip_atomic_fetch_add(A.waitCtr + arrive_shard(q) * LD_ARRIVE_STRIDE, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (recOk && prev >= 0) rec[2] = (double) wall_clock64();
        }
        return;
    }
    gn_solve_body<true>(B, D, S, St, A, (int) blockIdx.x);
}

hipError_t ba_launch_solve(const BaPtrs &B, const BaDims &D, const ResSet &S, const ldso_settings_t &St, const SolveArgs &A, hipStream_t st) {
    return launch_lds(k_solve, dim3(solve_roles(A.flags)), dim3(NT), solve_lds_bytes(D.n), st, B, D, S, St, A);
}

hipError_t ba_launch_gn_solve(const BaPtrs &B, const BaDims &D, const ResSet &S, const ldso_settings_t &St, const SolveArgs &A, hipStream_t st) {
    return launch_lds(k_gn_solve, dim3(2), dim3(NT), gn_lds_bytes(D.F, D.n), st, B, D, S, St, A);          // control step | statistics
}

// the control workgroup waits until every reduce workgroup of the launch has signalled: the grid and the wait target come from the same reduce_grid
hipError_t ba_launch_reduce_solve(const BaPtrs &B, const BaDims &D, const ResSet &S, const ldso_settings_t &St, const SolveArgs &A, const ChunkStarts &chunkStart,
                                  int atomicMode, float calibPrior, double l1, double il, hipStream_t st) {
    const ReduceGrid rg = reduce_grid(D.F, A.hasL, D.ks, A.GSP);
    SolveArgs A2 = A;
    A2.waitTarget = rg.total;
    return launch_lds(k_reduce_solve, dim3(rg.total + LD_FUSED_CTL), dim3(NT), std::max(gn_lds_bytes(D.F, D.n), reduce_atomic_lds_bytes(RT_DIRECT)), st,
                      B, D, S, St, A2, chunkStart, atomicMode, calibPrior, l1, il);
}
