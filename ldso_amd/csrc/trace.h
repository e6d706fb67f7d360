// trace.h — what the units that work on a tracer's immature points share (trace.hip, trace_group.hip; features.hip appends to tracers, act_select.hip compacts
// them): the job rows the kernels of trace.hip read, the tracer and its group, and the launchers and compaction steps that cross files.
#pragma once
#include "hip_host.h"

// One trace as the kernels of trace.hip read it: the by-value argument of k_trace_on, one row of the job table of k_trace_group (device memory there, every pointer
// a device pointer; the rows of a launch share nothing)
struct TraceJob {
    ldso_immature_t *pts;
    int n;
    const float *img;       // level-0 image of the new frame, 12-byte AoS (I, dx, dy)
    int w, h;
    const float *KRKi, *Kt, *aff;      // per host: 9, 3, 2 floats
    int nHosts;
    ldso_trace_settings_t s;
    int *counts;            // [6] per resulting status (a row of 8 ints)
};
hipError_t trace_launch_group(const TraceJob *d_jobs, const int *d_first, int nJobs, int totalWaves, hipStream_t st);      // trace.hip: totalWaves = first[nJobs] > 0

// One stable compaction of a tracer's records as the kernels of trace.hip read it: the by-value argument of k_compact_count / k_compact_move, one row of the job table of
// k_compact_count_group / k_compact_move_group (device memory there, every pointer a device pointer or null).  A workgroup serves CMP_THREADS records.
constexpr int CMP_THREADS = 256;
struct CompactArgs {
    const ldso_immature_t *src; ldso_immature_t *dst;
    const float *srcType; float *dstType;
    int n, nHosts;
    const unsigned char *keep8;      // keep flags as bytes, or
    const int32_t *keep32;           // ... record i is kept where keep32[i] == keepValue, or (both null) every record
    int keepValue;
    const int32_t *hostMap;          // [nHosts] new host index, < 0: the frame left; null: identity
    unsigned char *flag;             // [n]
    int32_t *blockCount;             // [ceil(n / 256)]
    int32_t *nOut;
};
inline int compact_blocks(int n) { return n > 0 ? (n + CMP_THREADS - 1) / CMP_THREADS : 0; }
// trace.hip: the two launches over a job table; first[j] = the workgroups in front of job j (compact_blocks of its records), totalBlocks = first[nJobs] > 0
hipError_t trace_launch_compact_group(const CompactArgs *d_jobs, const int *d_first, int nJobs, int totalBlocks, hipStream_t st);

// the immature-point tracer (trace.hip)
struct ldso_tracer {
    int device = 0, w = 0, h = 0, maxPoints = 0, n = 0;
    hipStream_t stream = nullptr;
    bool ownStream = false;
    const void *inGroup = nullptr;    // the ldso_trace_group this tracer belongs to (at most one; ldso_trace_destroy refuses while set: the group dereferences its members)
    ldso_trace_settings_t settings;
    ldso_immature_t *d_pts = nullptr, *d_alt = nullptr;     // the resident records; the buffer the next compaction writes (the two swap)
    float *d_type = nullptr, *d_typeAlt = nullptr;          // ImmaturePoint::my_type of every record (ImmaturePoint.h:114), beside d_pts / d_alt
    unsigned char *d_keep = nullptr, *d_flag = nullptr;     // [maxPoints] compaction: the caller's keep flags, the flags of the count pass
    int32_t *d_cmp = nullptr;                               // [LDSO_MAX_FRAMES host map | 4: the new count | maxPoints / 256 workgroup counts]
    int nAfterCompact = 0;                                  // where an enqueued compaction's count lands (trace_compact_finish)
    float *d_img = nullptr, *d_color = nullptr, *d_pose = nullptr;      // pose: [LDSO_MAX_FRAMES][14]
    const float *img = nullptr;       // the frame traced on: d_img, or level 0 of a shared ldso_pyramid_t
    int *d_counts = nullptr;
    bool haveFrame = false;
};

// a group of tracers whose traces share one launch (trace_group.hip)
struct ldso_trace_group {
    std::vector<ldso_tracer *> m;
    int device = 0;
    GroupArena arena;
};

#pragma GCC visibility push(hidden)
// trace.hip: the compaction of the tracer's resident immature set with keep flags that lie in device memory (ldso_ba_select_activate_tracer, act_select.hip):
// record i stays where d_keep8[i] != 0 / d_keep32[i] == keepValue (both null: everywhere) and its host is a frame of the window.  Enqueued on `st`;
// trace_compact_finish swaps the buffers and takes the new count once the caller has synchronised `st`.
int trace_compact_enqueue(ldso_tracer *T, const unsigned char *d_keep8, const int32_t *d_keep32, int keepValue, int n_hosts, bool haveMap, hipStream_t st);
void trace_compact_finish(ldso_tracer *T);
// The same compaction as a row of a grouped launch (T->n > 0): the map and the count lie where the caller says (its arena), the flags and workgroup counts are the
// tracer's own.  Behind the caller's wait: trace_compact_finish_group with the count that came down.
CompactArgs trace_compact_job(const ldso_tracer *T, const unsigned char *d_keep8, const int32_t *d_keep32, int keepValue, int n_hosts, const int32_t *d_hostMap, int32_t *d_nOut);
void trace_compact_finish_group(ldso_tracer *T, int nOut);
#pragma GCC visibility pop
