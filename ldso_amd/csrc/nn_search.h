// nn_search.h — the k-nearest-neighbour search of CoarseInitializer::makeNN (CoarseInitializer.cc:717-783) over the k-d tree init_nn_tree.cpp builds, as
// nanoflann searches it (include/frontend/nanoflann.h: findNeighbors :869-881, computeInitialDistances :1139-1155, searchLevel :1162-1207, KNNResultSet::addPoint
// :50-69, the distance of FLANNPointcloud, CoarseInitializer.h:171-175).  One text for host and device: the search kernel of init_first.hip and
// ldso_init_nn_search_host run every line below.  No HIP header here: init_nn_tree.cpp compiles as plain C++.
//
// Which of several equally distant points a row keeps is decided by the order of arrival, i.e. by the traversal; so the traversal is the reference's, step by step:
//   - the near child is child1 iff (val - divlow) + (val - divhigh) < 0; cut_dist is the squared distance to the OTHER side's bound;
//   - the far child is visited iff mindistsq + cut_dist - dists[feat] (evaluated left to right), times 1.0f, is <= worstDist at that moment;
//   - a leaf reads worstDist once on entry and admits dist < that value, in the leaf's index order;
//   - the result set shifts entries that are strictly greater: equal distances stay in arrival order.  worstDist is FLT_MAX until the set is full.
// The recursion becomes an explicit stack with one entry per inner node on the current path.  An entry is written when the search descends into the near child
// and holds what searchLevel still has to do after that call returns: the far child, the mindistsq to enter it with, cut_dist (the value dists[feat] takes while
// the far child is searched) and the dists[feat] to restore afterwards.  dists[feat] is the same on return from the near child as on entry to it - every level
// restores what it changed - so "mindistsq + cut_dist - dst" is formed when the entry is pushed, from the same three values in the same order.
#pragma once
#include "../../include/ldso_hip.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NN_HD __host__ __device__ __forceinline__
#else
#define NN_HD inline
#endif

#define NN_FLT_MAX 3.402823466e+38f
#define NN_K 10                // neighbours per point (CoarseInitializer.cc:733)
#define NN_LEAF 5              // KDTreeSingleIndexAdaptorParams(5), :729

// one stack entry, 16 bytes.  tag = far child * 4 + feat * 2 + phase; phase 0: the far child is still to be decided on, 1: it is being searched, restore on return
struct NnEntry { int tag; float mind, cut, dst; };

// KNNResultSet<float, int, int>(K) with its arrays in registers: K sorted distances, FLT_MAX in the places not yet filled.  That is addPoint :50-69 for every
// distance it is handed here - only dist < worstDist <= FLT_MAX is admitted, so a place that is "not counted yet" and a place that holds FLT_MAX shift alike.
template <int K> struct NnSet {
    float d[K];
    int i[K];
    NN_HD void init() {
#pragma unroll
        for (int k = 0; k < K; k++) { d[k] = NN_FLT_MAX; i[k] = -1; }
    }
    NN_HD float worst() const { return d[K - 1]; }
    // the new entry goes behind every entry that is <= dist (strict > shifts, :56); fully unrolled, no runtime index
    NN_HD void add(float dist, int index) {
#pragma unroll
        for (int k = K - 1; k >= 0; k--) {
            const bool stay = d[k] <= dist;                               // sorted: true on a prefix
            const bool fromBelow = k > 0 && d[k > 0 ? k - 1 : 0] > dist;
            const float pd = d[k > 0 ? k - 1 : 0];
            const int pi = i[k > 0 ? k - 1 : 0];
            d[k] = stay ? d[k] : fromBelow ? pd : dist;
            i[k] = stay ? i[k] : fromBelow ? pi : index;
        }
    }
};

// FLANNPointcloud::kdtree_distance: two differences, two products, one sum, in float, uncontracted (the library is built with -ffp-contract=off)
NN_HD float nn_dist(float qx, float qy, float px, float py) {
    const float d0 = qx - px, d1 = qy - py;
    return d0 * d0 + d1 * d1;
}

// findNeighbors for the query (qx, qy).  nodes / vind / uv: the tree (ldso_nn_node_t, the permuted index array, the points as u, v pairs); root: the root
// box (low u, high u, low v, high v).  stack[e * stride]: entry e of this query's stack; the caller has made sure the tree's depth fits.
template <int K, class Stack>
NN_HD void nn_search(const ldso_nn_node_t *nodes, const int *vind, const float *uv, const float *root, float qx, float qy, Stack stack, NnSet<K> &R) {
    R.init();
    // computeInitialDistances: a query outside the root box starts with its squared distance to the box, per axis
    float ds0 = 0.0f, ds1 = 0.0f, mind = 0.0f;
    if (qx < root[0]) { ds0 = (qx - root[0]) * (qx - root[0]); mind += ds0; }
    if (qx > root[1]) { ds0 = (qx - root[1]) * (qx - root[1]); mind += ds0; }
    if (qy < root[2]) { ds1 = (qy - root[2]) * (qy - root[2]); mind += ds1; }
    if (qy > root[3]) { ds1 = (qy - root[3]) * (qy - root[3]); mind += ds1; }
    int sp = 0, node = 0;
    for (;;) {
        // descend to a leaf, near child first
        for (;;) {
            const ldso_nn_node_t N = nodes[node];
            if (N.child1 < 0) {
                const float worst = R.worst();                            // read once per leaf (:1167)
                for (int q = N.left_or_feat; q < N.right; q++) {
                    const int index = vind[q];
                    const float dist = nn_dist(qx, qy, uv[2 * index], uv[2 * index + 1]);
                    if (dist < worst) R.add(dist, index);
                }
                break;
            }
            const int feat = N.left_or_feat;
            const float val = feat ? qy : qx;
            const float diff1 = val - N.divlow, diff2 = val - N.divhigh;
            const bool low = (diff1 + diff2) < 0;
            const float bound = low ? N.divhigh : N.divlow;
            const float cut = (val - bound) * (val - bound);
            const float dst = feat ? ds1 : ds0;
            NnEntry e;
            e.tag = (low ? N.child2 : N.child1) * 4 + feat * 2;
            e.mind = mind + cut - dst;
            e.cut = cut; e.dst = dst;
            stack.put(sp++, e);
            node = low ? N.child1 : N.child2;
        }
        // back up: restore behind far children that are done, enter the next far child that is still in reach
        bool found = false;
        while (sp > 0) {
            NnEntry e = stack.get(sp - 1);
            const int feat = (e.tag >> 1) & 1;
            if (e.tag & 1) { if (feat) ds1 = e.dst; else ds0 = e.dst; sp--; continue; }
            if (e.mind * 1.0f <= R.worst()) {
                if (feat) ds1 = e.cut; else ds0 = e.cut;
                e.tag |= 1;
                stack.put(sp - 1, e);
                mind = e.mind; node = e.tag >> 2;
                found = true;
                break;
            }
            sp--;                                                         // dists[feat] = cut_dist; dists[feat] = dst: nothing read it in between
        }
        if (!found) return;
    }
}

// the stack of one query in an array of its own (host) / interleaved with the other lanes' stacks (LDS: entry e of lane t at e * stride + t)
struct NnStack {
    NnEntry *p; int stride;
    NN_HD void put(int e, const NnEntry &v) const { p[(long) e * stride] = v; }
    NN_HD NnEntry get(int e) const { return p[(long) e * stride]; }
};
