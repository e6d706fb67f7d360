// group_stage.h — what the grouped calls (ldso_tr_group_*, ldso_trace_group_*, ldso_pyr_group_*, ldso_undist_group_*, ldso_feat_group_*) share as far as it can be said without a
// device: who may be a member, which members take part in a call, the prefix table that group_member_of searches, and where the regions of each group's staging
// arena lie.  The device side of an arena (GroupArena, AsyncArena) is in hip_host.h.  No HIP header: it compiles with a plain C++ compiler
// (tests/test_group_stage_cpu.py, tests/test_compact_group_stage_cpu.py and tests/test_feat_group_abi_cpu.py run it under the sanitizers).  A further group starts here: a rule, a layout, and its entries on top of both.
#pragma once
#include <string>
#include <vector>
#include "host_only.h"
#include "group_member.h"

// x rounded up to a multiple of a (a > 0): the one rounding helper of the library
inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// ---------------------------------------------------------------------------------------------------------
// Membership.  A member type has `device`, `inGroup` (const void *: the live group it belongs to, or null; its own destroy refuses while set, since the group
// dereferences its members) and, unless its group takes the stream per call, `stream`, compared as an opaque pointer.
// ---------------------------------------------------------------------------------------------------------
constexpr int GROUP_MAX_MEMBERS = 128;

struct GroupRule {
    const char *noun;            // the member with its article: "a tracker", "an undistorter"
    const char *setStream;       // the members share one stream, and this entry moves a member to another; null: they share the device only
    int maxN;
};

template <class M> auto group_stream_of(const M *m, int) -> decltype((const void *) m->stream) { return (const void *) m->stream; }
template <class M> const void *group_stream_of(const M *, long) { return nullptr; }          // a member type without a stream

// what create and every call check of a group before anything is enqueued: the members (still) share the device and the stream the group was made on
template <class M> int group_check(M *const *m, size_t n, const char *who, const GroupRule &R) {
    for (size_t i = 0; i < n; i++)
        REQ(m[i]->device == m[0]->device && (!R.setStream || group_stream_of(m[i], 0) == group_stream_of(m[0], 0)),
            std::string(who) + ": the members of a group share one device" + (R.setStream ? std::string(" and one stream (") + R.setStream + ")" : std::string()));
    return LDSO_OK;
}

// every check of a create entry `who`; nothing is written: group_join follows once the group exists
template <class M> int group_admit(M *const *m, int n, const void *out, const char *who, const GroupRule &R) {
    const std::string w = std::string(who) + ": ", bare = strchr(R.noun, ' ') + 1;
    REQ(m && out && n >= 1 && n <= R.maxN, w + "bad arguments (1 <= n <= " + std::to_string(R.maxN) + " " + bare + "s)");
    for (int i = 0; i < n; i++) {
        REQ(m[i], w + "null " + bare);
        REQ(m[i]->inGroup == nullptr, w + R.noun + " belongs to at most one group at a time");
        for (int k = 0; k < i; k++) REQ(m[k] != m[i], w + "the same " + bare + " twice");
    }
    return group_check(m, (size_t) n, who, R);
}

template <class G> void group_join(G *g) { for (auto *M : g->m) M->inGroup = g; }
template <class G> void group_leave(G *g) { for (auto *M : g->m) if (M->inGroup == g) M->inGroup = nullptr; }          // not a member that has joined another group since

// ---------------------------------------------------------------------------------------------------------
// The active list of a call: the indices i < n with active == null or active[i] != 0, each passed by check(i) -> null, or what the call refuses of member i.
// ---------------------------------------------------------------------------------------------------------
template <class Check> int group_active(int n, const uint8_t *active, const char *who, std::vector<int> &members, Check check) {
    members.clear();
    for (int i = 0; i < n; i++) {
        if (active && !active[i]) continue;
        const char *refusal = check(i);
        REQ(!refusal, std::string(who) + ": member " + std::to_string(i) + ": " + refusal);
        members.push_back(i);
    }
    REQ(!members.empty(), std::string(who) + ": no active member");
    return LDSO_OK;
}

// first[0 .. nJobs] as group_member_of reads it, from units(j) = the wavefronts / workgroups of job j (0: the job is skipped) -> all of them = first[nJobs]
template <class Units> int group_prefix(int nJobs, int *first, Units units) {
    int sum = 0;
    for (int j = 0; j < nJobs; j++) { first[j] = sum; sum += units(j); }
    first[nJobs] = sum;
    return sum;
}

// ---------------------------------------------------------------------------------------------------------
// The arenas: byte offsets from counts and row sizes alone.  Every arena goes up in one copy of `total` bytes; `down`/`downBytes` is what comes back.
// ---------------------------------------------------------------------------------------------------------

// tracker group: [TrParams of the np members that take part | TrJob x nj | TrHyp x nj], each region 16-byte aligned; the records come down
struct TrGroupLayout { size_t params, jobs, down, downBytes, total; };
inline TrGroupLayout tr_group_layout(size_t np, size_t nj, size_t paramBytes, size_t jobBytes, size_t hypBytes) {
    TrGroupLayout L;
    L.params = 0; L.jobs = align_up(np * paramBytes, 16); L.down = align_up(L.jobs + nj * jobBytes, 16); L.downBytes = nj * hypBytes; L.total = L.down + L.downBytes;
    return L;
}

// tracer group: [pose blocks, 14 floats per host | TraceJob x nj | first, nj + 1 | count rows, nj x 8 ints], 16-byte aligned; the count rows come down
struct TraceGroupLayout { size_t poses, jobs, first, down, downBytes, total; };
inline TraceGroupLayout trace_group_layout(size_t poseFloats, size_t nj, size_t jobBytes) {
    TraceGroupLayout L;
    L.poses = 0; L.jobs = align_up(poseFloats * 4, 16); L.first = align_up(L.jobs + nj * jobBytes, 16); L.down = align_up(L.first + (nj + 1) * 4, 16);
    L.downBytes = nj * 8 * 4; L.total = L.down + L.downBytes;
    return L;
}

// tracer group, compaction: [CompactArgs x nj | first, nj + 1 | host maps, mapInts per job | the keep bytes of every job | counts, nj ints], every region and every
// job's keep bytes 16-byte aligned; the counts come down.  keepBytes(j) = the keep flags job j uploads (0: it keeps every record, or has none)
struct CompactGroupLayout { size_t jobs, first, maps; std::vector<size_t> keep; size_t down, downBytes, total; };
template <class KeepBytes> CompactGroupLayout compact_group_layout(size_t nj, size_t jobBytes, size_t mapInts, KeepBytes keepBytes) {
    CompactGroupLayout L;
    L.jobs = 0; L.first = align_up(nj * jobBytes, 16); L.maps = align_up(L.first + (nj + 1) * 4, 16);
    size_t at = align_up(L.maps + nj * mapInts * 4, 16);
    L.keep.resize(nj);
    for (size_t j = 0; j < nj; j++) { L.keep[j] = at; at = align_up(at + keepBytes(j), 16); }
    L.down = at; L.downBytes = nj * 4; L.total = L.down + L.downBytes;
    return L;
}

// features group: [FeatArgs x nj | four prefix tables of nj + 1: cells, compaction, corners and records (they share one), angle + descriptor | ctl rows, nj x 8 ints],
// each region 16-byte aligned; the ctl rows go up zeroed and come down
struct FeatGroupLayout { size_t jobs, firstCells, firstCompact, firstCorners, firstDescribe, down, downBytes, total; };
inline FeatGroupLayout feat_group_layout(size_t nj, size_t jobBytes) {
    FeatGroupLayout L;
    const size_t table = align_up((nj + 1) * 4, 16);
    L.jobs = 0; L.firstCells = align_up(nj * jobBytes, 16); L.firstCompact = L.firstCells + table; L.firstCorners = L.firstCompact + table; L.firstDescribe = L.firstCorners + table;
    L.down = L.firstDescribe + table; L.downBytes = nj * 8 * 4; L.total = L.down + L.downBytes;
    return L;
}

// pyramid group: per level [ImgJob of the nl members that have it | nl + 1 workgroup prefixes of the intensity launch | nl + 1 of the gradient launch], every
// level 16-byte aligned.  membersAt(l) = nl
struct PyrLevelLayout { size_t jobs, firstI, firstG; int nl; };
struct PyrGroupLayout { std::vector<PyrLevelLayout> level; size_t total; };
template <class MembersAt> PyrGroupLayout pyr_group_layout(int levels, size_t jobBytes, MembersAt membersAt) {
    PyrGroupLayout P;
    P.level.resize((size_t) levels);
    P.total = 0;
    for (int l = 0; l < levels; l++) {
        PyrLevelLayout &L = P.level[(size_t) l];
        L.nl = membersAt(l);
        L.jobs = P.total; L.firstI = L.jobs + (size_t) L.nl * jobBytes; L.firstG = L.firstI + (size_t) (L.nl + 1) * 4;
        P.total = align_up(L.firstG + (size_t) (L.nl + 1) * 4, 16);
    }
    return P;
}

// undistorter group: [UndistJob x nj | wgFirst, nj + 1], then the raw frame of every job, each 64-byte aligned.  frameBytes(j) = the bytes of job j's frame
struct UndistGroupLayout { size_t jobs, first; std::vector<size_t> frame; size_t total; };
template <class FrameBytes> UndistGroupLayout undist_group_layout(size_t nj, size_t jobBytes, FrameBytes frameBytes) {
    UndistGroupLayout L;
    L.jobs = 0; L.first = nj * jobBytes; L.total = align_up(L.first + (nj + 1) * 4, 64);
    L.frame.resize(nj);
    for (size_t j = 0; j < nj; j++) { L.frame[j] = L.total; L.total = align_up(L.total + frameBytes(j), 64); }
    return L;
}
