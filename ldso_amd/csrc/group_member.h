// group_member.h — the member-lookup rule of the grouped launches (k_trace_group: wavefronts, the grouped image kernels: workgroups), defined once for host and device.
// `first` has nJobs + 1 entries: first[j] = the units (wavefronts / workgroups) in front of job j, first[nJobs] = all of them.  Unit u belongs to the job j with
// first[j] <= u < first[j + 1]: an upper-bound search for the smallest j whose END lies beyond u.  A job without units has first[j] == first[j + 1]; its end is
// never the first one beyond u (the job in front of it ends at the same place), so empty jobs are skipped wherever they stand.  The caller guarantees
// 0 <= u < first[nJobs]; ldso_trace_group_member_of (trace_group.hip) is the checked host form.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LD_HOST_DEVICE __host__ __device__
#else
#define LD_HOST_DEVICE
#endif

#if defined(__HIPCC__)
// A pointer that a kernel reads out of its job table is a generic one to the compiler (flat instructions, both memory counters).  The tables hold device memory
// only; a kernel says so by reading its rows through a twin of the row type whose pointers carry this address space, and gets global instructions, as for a
// pointer that arrives as a kernel argument.  (A cast at the point of use does not: generic -> global -> generic folds away.)
#define LD_GLOBAL __attribute__((address_space(1)))
#endif

LD_HOST_DEVICE inline int group_member_of(const int *first, int nJobs, int u) {
    int lo = 0, hi = nJobs - 1;          // the answer lies in [lo, hi]: first[hi + 1] = first[nJobs] > u
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (first[mid + 1] > u) hi = mid; else lo = mid + 1;
    }
    return lo;
}
