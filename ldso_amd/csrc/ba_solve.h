// ba_solve.h — launch arguments of the control kernels (see ba_solve.hip, ba_solve_body.h)
#pragma once
#include <stdint.h>

enum {
    SK_POST = 1u << 0, SK_ADJ = 1u << 1, SK_GATHER = 1u << 2, SK_SOLVE = 1u << 3, SK_BACKUP = 1u << 4, SK_STEP = 1u << 5,
    SK_LOADBK = 1u << 6, SK_PRECALC = 1u << 7, SK_REANCHOR = 1u << 8, SK_COLLECT = 1u << 9, SK_LOG = 1u << 10,
    SK_FROMREDUCED = 1u << 11, SK_THRESH = 1u << 12, SK_EXPORT = 1u << 13,
    SK_NONULLSPACE = 1u << 14      // with SK_ADJ: adjoints only, keep the gauge nullspace basis (no solve follows)
};
enum { PS_RESUB = 1, PS_BACKUP = 2, PS_STEP = 4, PS_LOAD = 8 };

// the tail of optimize(): flags of both groups and of nothing else = two workgroups (roles), the statistics (role 1) next to the independent control part (role 0)
enum { SK_STATS = SK_POST | SK_THRESH | SK_LOG, SK_CTL = SK_REANCHOR | SK_ADJ | SK_NONULLSPACE | SK_PRECALC };
static inline int solve_roles(unsigned flags) { return ((flags & SK_STATS) && (flags & SK_CTL) && !(flags & ~(unsigned) (SK_STATS | SK_CTL))) ? 2 : 1; }
struct SolveArgs {          // every field starts neutral: the callers set what differs
    unsigned flags = 0;
    int iteration = 0;
    double lambda = 0;
    int hasL = 0;
    int hasPrior = 0;           // HM/bM non-zero
    int GSP = 0;
    int logIdx = -1;
    double *reduceOut = nullptr;          // multi-GPU: rank-local sums are exported here (SK_GATHER)
    const double *reduceIn = nullptr;     // multi-GPU: all-reduced sums are read from here (SK_FROMREDUCED)
    int itCheck = -1;           // k_gn_solve: >= 0 = un-forced optimize(): iteration index for the device-side `canbreak` early exit
    int *waitCtr = nullptr;     // k_reduce_solve: the arrival words (ba_dev.h: arrive_shard) the reduce workgroups of the same launch add to when their sums are in B.acc
    int waitTarget = 0;         //                 ... and how many of them arrive in all; the kernel derives every word's share (arrive_target)
    int *hostStop = nullptr;    // un-forced optimize(): host-mapped word that receives the index of the iteration that ended the loop (canbreak, or the
    int lastIt = -1;            //                       last enqueued iteration lastIt) as soon as the device knows it - no stream synchronisation
};
