// initializer_sched.cpp — the schedule of the initialiser's optReg sweep: host arithmetic only, no device work.
#include "host_only.h"

// The schedule of the optReg sweep: pass[i] for every point such that (a) every neighbour j < i of i sits in an EARLIER pass (i reads j's new value), (b) every
// neighbour j > i of i sits in the SAME or a later pass (i reads j's old value; reads come before writes within a pass) and (c) no pass holds more than `width`
// points.  The reference's in-place loop over i (CoarseInitializer.cc:430-459) is pass 0, 1, 2, ... of this schedule executed in order.
// Two constructions, the shorter one wins: first fit in index order (both conditions only look at lower indices), and list scheduling by the length of the
// chain that still hangs on a point (the dependency depth is a diagonal front through the raster; where it is wider than a pass, the points with the longest
// tails go first).  640 x 480 (8.4k / 18.4k / 17.2k / 3.8k points, depth 341 / 586 / 412 / 196): first fit 341 / 719 / 654 / 196 passes, list 341 / 642 / 606 / 196.
static bool ini_schedule_valid(int n, const int *nb, int width, const std::vector<int> &pass, int nPass) {
    std::vector<int> cnt(std::max(nPass, 1), 0);
    for (int i = 0; i < n; i++) {
        if (pass[i] < 0 || pass[i] >= nPass || ++cnt[pass[i]] > width) return false;
        for (int q = 0; q < 10; q++) {
            const int j = nb[(size_t) i * 10 + q];
            if (j < 0 || j == i) continue;
            if (j < i ? !(pass[j] < pass[i]) : !(pass[j] >= pass[i])) return false;
        }
    }
    return true;
}
int ini_sweep_schedule(int n, const int *nb, int width, int *passOut) {
    if (n <= 0) return 0;
    // first fit
    std::vector<int> ff(n, 0), rd(n, 0), fillOf;
    for (int i = 0; i < n; i++) {
        int e = rd[i];
        for (int q = 0; q < 10; q++) { const int j = nb[(size_t) i * 10 + q]; if (j >= 0 && j < i) e = std::max(e, ff[j] + 1); }
        while (e < (int) fillOf.size() && fillOf[e] >= width) e++;
        if (e >= (int) fillOf.size()) fillOf.resize(e + 1, 0);
        ff[i] = e;
        for (int q = 0; q < 10; q++) { const int j = nb[(size_t) i * 10 + q]; if (j > i && j < n) rd[j] = std::max(rd[j], e); }
        fillOf[e]++;
    }
    const int nFF = (int) fillOf.size();
    // list scheduling.  after[j]: the points i > j that have j as a neighbour (i waits for j's pass to be over); before[j]: the readers i < j of j (j must not
    // come before them); tail[i]: passes that must still follow the pass of i
    std::vector<int> offA(n + 1, 0), offB(n + 1, 0), waits(n, 0);
    for (int i = 0; i < n; i++) for (int q = 0; q < 10; q++) { const int j = nb[(size_t) i * 10 + q]; if (j < 0 || j >= n || j == i) continue; if (j < i) { offA[j + 1]++; waits[i]++; } else offB[j + 1]++; }
    for (int i = 0; i < n; i++) { offA[i + 1] += offA[i]; offB[i + 1] += offB[i]; }
    std::vector<int> after(offA[n]), before(offB[n]), curA(offA.begin(), offA.end() - 1), curB(offB.begin(), offB.end() - 1);
    for (int i = 0; i < n; i++) for (int q = 0; q < 10; q++) { const int j = nb[(size_t) i * 10 + q]; if (j < 0 || j >= n || j == i) continue; if (j < i) after[curA[j]++] = i; else before[curB[j]++] = i; }
    std::vector<int> tail(n, 0);
    for (int i = n - 1; i >= 0; i--) {
        int t = 0;
        for (int a = offA[i]; a < offA[i + 1]; a++) t = std::max(t, tail[after[a]] + 1);
        for (int q = 0; q < 10; q++) { const int j = nb[(size_t) i * 10 + q]; if (j > i && j < n) t = std::max(t, tail[j]); }
        tail[i] = t;
    }
    std::vector<int> ls(n, -1), ready, chosen, deferred;
    std::vector<char> inPass(n, 0);
    for (int i = 0; i < n; i++) if (waits[i] == 0) ready.push_back(i);
    int left = n, t = 0;
    bool stuck = false;
    while (left > 0 && !stuck) {
        std::sort(ready.begin(), ready.end(), [&](int a, int b) { return tail[a] != tail[b] ? tail[a] > tail[b] : a < b; });
        chosen.clear(); deferred.clear();
        auto free_ = [&](int i) { for (int a = offB[i]; a < offB[i + 1]; a++) { const int k = before[a]; if (ls[k] < 0 && !inPass[k]) return false; } return true; };
        for (int i : ready) { if ((int) chosen.size() < width && free_(i)) { chosen.push_back(i); inPass[i] = 1; } else deferred.push_back(i); }
        for (bool again = true; again && (int) chosen.size() < width;) {          // readers chosen later in the priority order free the points they held back
            again = false;
            for (size_t d = 0; d < deferred.size(); d++) {
                const int i = deferred[d];
                if (i >= 0 && (int) chosen.size() < width && free_(i)) { chosen.push_back(i); inPass[i] = 1; deferred[d] = -1; again = true; }
            }
        }
        if (chosen.empty()) { stuck = true; break; }
        ready.clear();
        for (int i : deferred) if (i >= 0) ready.push_back(i);
        for (int i : chosen) { ls[i] = t; inPass[i] = 0; left--; }
        for (int i : chosen) for (int a = offA[i]; a < offA[i + 1]; a++) if (--waits[after[a]] == 0) ready.push_back(after[a]);
        t++;
    }
    const bool useList = !stuck && t < nFF && ini_schedule_valid(n, nb, width, ls, t);
    for (int i = 0; i < n; i++) passOut[i] = useList ? ls[i] : ff[i];
    return useList ? t : nFF;
}

// the optReg sweep schedule ldso_init_set_first builds for a level, checked
extern "C" int ldso_init_sweep_schedule(int n, const int *neighbours, int width, int *pass_out) {
    REQ(n >= 0 && (n == 0 || (neighbours && pass_out)) && width >= 1, "ldso_init_sweep_schedule: bad argument");
    for (size_t q = 0; q < (size_t) n * 10; q++) REQ(neighbours[q] >= -1 && neighbours[q] < n, "ldso_init_sweep_schedule: neighbour index out of range");
    std::vector<int> pass(n);
    const int np = ini_sweep_schedule(n, neighbours, width, pass.data());
    REQ(ini_schedule_valid(n, neighbours, width, pass, np), "ldso_init_sweep_schedule: internal error (schedule violates the update order)");
    for (int i = 0; i < n; i++) pass_out[i] = pass[i];
    return np;
}
