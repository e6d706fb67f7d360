// host_only.h — what the translation units without device work (tracker_hyp.cpp, initializer_sched.cpp) share with the rest of the library: the error
// channel and the prototypes that cross into them.  No HIP header: these files compile with a plain C++ compiler.
#pragma once
#include <string>
#include <vector>
#include <cstring>
#include <cmath>
#include <algorithm>
#include "../../include/ldso_hip.h"

void ldso_set_error(const std::string &s);          // ba_api.hip (thread-local, read by ldso_last_error)
#define REQ(cond, msg) do { if (!(cond)) { ldso_set_error(msg); return LDSO_E_INVALID; } } while (0)
#define RUN(x) do { int r_ = (x); if (r_ != LDSO_OK) return r_; } while (0)

// initializer_sched.cpp: the pass of every point in the optReg sweep (passes of at most `width` points); returns the number of passes
__attribute__((visibility("hidden"))) int ini_sweep_schedule(int n, const int *nb, int width, int *passOut);
