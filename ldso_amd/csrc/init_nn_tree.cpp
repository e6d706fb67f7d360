// init_nn_tree.cpp — host only: the k-d tree of CoarseInitializer::makeNN (CoarseInitializer.cc:717-731) built as nanoflann builds it
// (include/frontend/nanoflann.h: buildIndex :827-834, computeBoundingBox :972-990, divideTree :1000-1046, computeMinMax :1049-1057, middleSplit_ :1059-1098,
// planeSplit :1110-1137; leaf size 5), the host search over it (nn_search.h) and the scalar recursion of makePixelStatus (PixelSelector2.h:253-276).
// The build is sequential on purpose: planeSplit permutes ONE index array in place, the order it leaves inside a leaf is the order in which a search meets
// equally distant points, and that order decides which of them a neighbour list keeps.  The device searches this tree; it does not build one.
#include "host_only.h"
#include "nn_search.h"

struct ldso_nn_tree {
    int n = 0, depth = 0;                   // depth: inner nodes above the deepest leaf = stack entries a search can need
    std::vector<float> uv;                  // the points, u v pairs (copied)
    std::vector<int> vind;                  // nanoflann's vind after the build
    std::vector<ldso_nn_node_t> nodes;      // in allocation order: a node before its subtrees, child1's subtree before child2's; node 0 is the root
    float root[4] = {0, 0, 0, 0};           // root_bbox: low u, high u, low v, high v
};

namespace {

struct Box { float low[2], high[2]; };

struct Builder {
    ldso_nn_tree &T;
    std::vector<size_t> ind;                // IndexType is size_t in the reference's tree: the `right &&` / `!right` tests of planeSplit are written for it
    explicit Builder(ldso_nn_tree &t) : T(t), ind(t.n) { for (size_t i = 0; i < ind.size(); i++) ind[i] = i; }
    float get(size_t idx, int dim) const { return T.uv[2 * idx + dim]; }

    void min_max(const size_t *p, size_t count, int element, float &mn, float &mx) const {
        mn = get(p[0], element); mx = get(p[0], element);
        for (size_t i = 1; i < count; i++) {
            const float val = get(p[i], element);
            if (val < mn) mn = val;
            if (val > mx) mx = val;
        }
    }

    // two passes: < cutval to the front, then <= cutval; lim1 / lim2 = where each pass stopped
    void plane_split(size_t *p, const size_t count, int cutfeat, float cutval, size_t &lim1, size_t &lim2) const {
        size_t left = 0, right = count - 1;
        for (;;) {
            while (left <= right && get(p[left], cutfeat) < cutval) ++left;
            while (right && left <= right && get(p[right], cutfeat) >= cutval) --right;
            if (left > right || !right) break;
            std::swap(p[left], p[right]);
            ++left; --right;
        }
        lim1 = left;
        right = count - 1;
        for (;;) {
            while (left <= right && get(p[left], cutfeat) <= cutval) ++left;
            while (right && left <= right && get(p[right], cutfeat) > cutval) --right;
            if (left > right || !right) break;
            std::swap(p[left], p[right]);
            ++left; --right;
        }
        lim2 = left;
    }

    void middle_split(size_t *p, size_t count, size_t &index, int &cutfeat, float &cutval, const Box &b) const {
        const float EPS = 0.00001f;
        float max_span = b.high[0] - b.low[0];
        { const float span = b.high[1] - b.low[1]; if (span > max_span) max_span = span; }
        float max_spread = -1;
        cutfeat = 0;
        for (int i = 0; i < 2; i++) {
            const float span = b.high[i] - b.low[i];
            if (span > (1 - EPS) * max_span) {
                float mn, mx;
                min_max(p, count, cutfeat, mn, mx);          // sic: the spread of `cutfeat`, not of `i` (nanoflann.h:1075).  With two axes: axis 1 is cut
                const float spread = mx - mn;                // iff the box's span on axis 0 fails the test above, whatever the points' spread on axis 1
                if (spread > max_spread) { cutfeat = i; max_spread = spread; }
            }
        }
        const float split_val = (b.low[cutfeat] + b.high[cutfeat]) / 2;
        float mn, mx;
        min_max(p, count, cutfeat, mn, mx);
        if (split_val < mn) cutval = mn;
        else if (split_val > mx) cutval = mx;
        else cutval = split_val;
        size_t lim1, lim2;
        plane_split(p, count, cutfeat, cutval, lim1, lim2);
        if (lim1 > count / 2) index = lim1;
        else if (lim2 < count / 2) index = lim2;
        else index = count / 2;
    }

    int divide(size_t left, size_t right, Box &b, int level) {
        const int me = (int) T.nodes.size();
        T.nodes.push_back(ldso_nn_node_t());
        if (right - left <= NN_LEAF) {
            ldso_nn_node_t N;
            N.child1 = N.child2 = -1; N.left_or_feat = (int) left; N.right = (int) right; N.divlow = N.divhigh = 0;
            T.nodes[me] = N;
            for (int i = 0; i < 2; i++) b.low[i] = b.high[i] = get(ind[left], i);
            for (size_t k = left + 1; k < right; k++)
                for (int i = 0; i < 2; i++) {
                    if (b.low[i] > get(ind[k], i)) b.low[i] = get(ind[k], i);
                    if (b.high[i] < get(ind[k], i)) b.high[i] = get(ind[k], i);
                }
            T.depth = std::max(T.depth, level);
            return me;
        }
        size_t idx; int cutfeat; float cutval;
        middle_split(ind.data() + left, right - left, idx, cutfeat, cutval, b);
        Box lb = b; lb.high[cutfeat] = cutval;
        const int c1 = divide(left, left + idx, lb, level + 1);
        Box rb = b; rb.low[cutfeat] = cutval;
        const int c2 = divide(left + idx, right, rb, level + 1);
        ldso_nn_node_t N;
        N.child1 = c1; N.child2 = c2; N.left_or_feat = cutfeat; N.right = 0;
        N.divlow = lb.high[cutfeat]; N.divhigh = rb.low[cutfeat];
        T.nodes[me] = N;
        for (int i = 0; i < 2; i++) { b.low[i] = std::min(lb.low[i], rb.low[i]); b.high[i] = std::max(lb.high[i], rb.high[i]); }
        return me;
    }
};

template <int K> void search_rows(const ldso_nn_tree *T, int nq, const float *q, int32_t *idx, float *dist) {
    std::vector<NnEntry> st(std::max(1, T->depth));
    for (int r = 0; r < nq; r++) {
        NnSet<K> R;
        nn_search<K>(T->nodes.data(), T->vind.data(), T->uv.data(), T->root, q[2 * r], q[2 * r + 1], NnStack{st.data(), 1}, R);
        for (int k = 0; k < K; k++) { idx[(size_t) r * K + k] = R.i[k]; dist[(size_t) r * K + k] = R.d[k]; }
    }
}

}  // namespace

extern "C" {

int ldso_init_nn_build(int n, const float *uv, ldso_nn_tree_t **out) {
    REQ(out && uv && n > 0 && n < (1 << 28), "ldso_init_nn_build: bad arguments (n > 0)");
    for (size_t i = 0; i < (size_t) n * 2; i++) REQ(std::isfinite(uv[i]), "ldso_init_nn_build: non-finite position");
    ldso_nn_tree *T = new ldso_nn_tree();
    T->n = n; T->uv.assign(uv, uv + (size_t) n * 2);
    Builder B(*T);
    Box b;
    for (int i = 0; i < 2; i++) b.low[i] = b.high[i] = B.get(0, i);
    for (size_t k = 1; k < (size_t) n; k++)
        for (int i = 0; i < 2; i++) {
            if (B.get(k, i) < b.low[i]) b.low[i] = B.get(k, i);
            if (B.get(k, i) > b.high[i]) b.high[i] = B.get(k, i);
        }
    T->nodes.reserve((size_t) n);
    B.divide(0, (size_t) n, b, 0);           // the box comes back merged from the leaves: that is root_bbox (:832-833 hand in the same object)
    T->root[0] = b.low[0]; T->root[1] = b.high[0]; T->root[2] = b.low[1]; T->root[3] = b.high[1];
    T->vind.resize(n);
    for (int i = 0; i < n; i++) T->vind[i] = (int) B.ind[i];
    *out = T;
    return LDSO_OK;
}

int ldso_init_nn_free(ldso_nn_tree_t *T) { delete T; return LDSO_OK; }

int ldso_init_nn_info(const ldso_nn_tree_t *T, int *n, int *n_nodes, int *depth, float root_box[4]) {
    REQ(T, "ldso_init_nn_info: null tree");
    if (n) *n = T->n;
    if (n_nodes) *n_nodes = (int) T->nodes.size();
    if (depth) *depth = T->depth;
    if (root_box) memcpy(root_box, T->root, sizeof(T->root));
    return LDSO_OK;
}

int ldso_init_nn_get(const ldso_nn_tree_t *T, ldso_nn_node_t *nodes_out, int32_t *vind_out) {
    REQ(T, "ldso_init_nn_get: null tree");
    if (nodes_out) memcpy(nodes_out, T->nodes.data(), T->nodes.size() * sizeof(ldso_nn_node_t));
    if (vind_out) memcpy(vind_out, T->vind.data(), T->vind.size() * sizeof(int32_t));
    return LDSO_OK;
}

int ldso_init_nn_search_host(const ldso_nn_tree_t *T, int n_query, const float *query_uv, int k, int32_t *idx_out, float *dist_out) {
    REQ(T && n_query >= 0 && (n_query == 0 || (query_uv && idx_out && dist_out)), "ldso_init_nn_search_host: bad arguments");
    if (k != 1 && k != NN_K) { ldso_set_error("ldso_init_nn_search_host: k is 1 (the parent) or 10 (the neighbours)"); return LDSO_E_UNSUPPORTED; }
    if (k == 1) search_rows<1>(T, n_query, query_uv, idx_out, dist_out);
    else search_rows<NN_K>(T, n_query, query_uv, idx_out, dist_out);
    return LDSO_OK;
}

// makePixelStatus :253-276 behind one gridMaxSelection pass that set n_good pixels at `sparsity` (>= 1, :230 has clamped it) with th_fac
int ldso_init_pixel_status_plan(int n_good, float desired, int sparsity, int recs_left, float th_fac, int *action, int *new_sparsity, float *new_th_fac) {
    REQ(action && new_sparsity && new_th_fac && n_good >= 0 && sparsity >= 1 && recs_left >= 0, "ldso_init_pixel_status_plan: bad arguments");
    const float quotia = n_good / (float) desired;
    int newSparsity = (sparsity * sqrtf(quotia)) + 0.7f;
    if (newSparsity < 1) newSparsity = 1;
    const float oldTHFac = th_fac;
    if (newSparsity == 1 && sparsity == 1) th_fac = 0.5;
    const bool done = (std::abs(newSparsity - sparsity) < 1 && th_fac == oldTHFac) || (quotia > 0.8 && 1.0f / quotia > 0.8) || recs_left == 0;
    *action = done ? 0 : 1; *new_sparsity = newSparsity; *new_th_fac = th_fac;
    return LDSO_OK;
}

}  // extern "C"
