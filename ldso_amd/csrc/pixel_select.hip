// pixel_select.hip — DSO's gradient pixels of a new key frame on the device (gfx950): PixelSelector::makeMaps (reference src/frontend/PixelSelector2.cc:111-168
// with makeHists :36-109, computeHistQuantil :27-34 and select :170-315) and the raster scan + ImmaturePoint constructors of FullSystem::makeNewTraces for
// setting_pointSelection == 0 (FullSystem.cc:1284-1304).  Input: levels 0-2 of a resident ldso_pyramid_t, 12-byte pixels (I, dx, dy); absSquaredGrad is
// computed on the fly (FrameHessian.cc:91-96).
//
//   k_pix_hist     one workgroup per 32 x 32 cell: 50-bin integer histogram of int(sqrtf(absSquaredGrad[0])) in LDS (integer atomics), quantile -> ths
//   k_pix_smooth   one lane per cell: thsSmoothed = square of the 3 x 3 mean, summed in the reference's order (:67-108)
//   k_pix_masks    per pot block a 16-bit mask: under which of the 16 directions does the block select at level 1 (a pixel passes the threshold AND its score
//                  |g . dir| is > 0)?  L = lanes_per_block(pot) lanes share a block, an OR across them; masks are stored in the reference's NESTED order
//   k_pix_scan     one wavefront: n2 (level-1 selections so far, :215/:224/:233) at every pot block, 64 blocks per step.  A step whose masks are all 0 or
//                  0xffff is a ballot; otherwise the 64 blocks are resolved one after another on scalar registers, the next 64 pattern bytes held in a vector
//                  register.  Output: the direction index randomPattern[n2] & 15 of every pot block
//   k_pix_select   one wavefront per 4 pot block: the three rules of select with the directions known; a pot / 2 pot / 4 pot block of any size is walked
//                  by the 64 lanes (nothing is staged in LDS), the winner is a 64-bit integer maximum of (score bits, first in the reference's order)
//   k_pix_thin / k_pix_points   the thinning of :150-163 and the records of FullSystem.cc:1290-1303, each one statement per selected pixel in raster rank
//                  order: the rank (per-row counts, one prefix sum, ballots inside a row) is the raster scan of raster_scan.h
//
// select decomposes because bestVal2 is reset per pot block, a 2 pot block reaches its level-2 result only if none of its pot blocks selected, and a 4 pot
// block its level-3 result only if nothing inside selected; the one sequential quantity is n2.  Every float expression keeps the reference's operand order
// and width (-ffp-contract=off); no floating-point sum crosses lanes.  Three reads the reference leaves undefined are defined (ldso_hip.h): the last row of
// absSquaredGrad[2] is 0, sizes that are no multiples of 32 are refused, a non-finite pixel gives LDSO_E_NONFINITE (and never wins a comparison).
#include "hip_host.h"
#include "immature_record.h"
#include "raster_scan.h"

#define PIX_RP_LDS 65536                // bytes of the random pattern k_pix_scan stages in LDS
enum { PIX_FLAGS = 0, PIX_N2 = 1, PIX_N3 = 2, PIX_N4 = 3, PIX_REMOVED = 4, PIX_TOTAL = 5, PIX_SCAN_N2 = 6 };

struct PixArgs {
    const float *lv[3]; int w, h, w1, w2;
    const float *B;                     // 256-entry response table or null
    const unsigned char *rp;            // randomPattern, w * h bytes
    float *ths, *thsSmoothed; int w32, h32;
    float cut, add, dw1, thFactor; int sdd;
    int pot, nbx, nby;
    unsigned short *mask; unsigned char *dir, *map;
    int32_t *rowStart, *ctl;
};

// select's 16 directions (:185-201), converted from the same double literals
__device__ const float PIX_DX[16] = {(float) 0, (float) 0.3827, (float) 0.1951, (float) 0.9239, (float) 0.7071, (float) 0.3827, (float) 0.8315, (float) 0.8315,
                                     (float) 0.5556, (float) 0.9808, (float) 0.9239, (float) 0.7071, (float) 0.5556, (float) 0.9808, (float) 1.0000, (float) 0.1951};
__device__ const float PIX_DY[16] = {(float) 1.0000, (float) 0.9239, (float) 0.9808, (float) 0.3827, (float) 0.7071, (float) -0.9239, (float) 0.5556, (float) -0.5556,
                                     (float) -0.8315, (float) 0.1951, (float) -0.3827, (float) -0.7071, (float) 0.8315, (float) -0.1951, (float) 0.0000, (float) -0.9808};

// Place of pot block (bx, by) in the traversal of :209-226: 4 pot blocks in raster order, the 2 pot blocks inside each in raster order, the pot blocks inside
// those in raster order; edge blocks are clipped, so a 4 pot block holds cx x cy pot blocks (1..4 each way).
static __host__ __device__ inline int pix_order(int bx, int by, int nbx, int nby) {
    const int X4 = bx >> 2, Y4 = by >> 2, cx = min(4, nbx - 4 * X4), cy = min(4, nby - 4 * Y4);
    const int lx = bx & 3, ly = by & 3, x2 = lx >> 1, y2 = ly >> 1, c2x = min(2, cx - 2 * x2), c2y = min(2, cy - 2 * y2);
    return Y4 * 4 * nbx + X4 * 4 * cy + y2 * 2 * cx + x2 * 2 * c2y + (ly & 1) * c2x + (lx & 1);
}

// makeHists :47-65
__global__ __launch_bounds__(256) void k_pix_hist(PixArgs A) {
    __shared__ int hist[64];
    const int tid = threadIdx.x, cx = blockIdx.x % A.w32, cy = blockIdx.x / A.w32, w = A.w, h = A.h;
    if (tid < 64) hist[tid] = 0;
    __syncthreads();
    bool bad = false;
    for (int p = tid; p < 1024; p += 256) {
        const int it = (p & 31) + 32 * cx, jt = (p >> 5) + 32 * cy;
        float dx, dy;
        const float ag = abs_sq_grad(A.lv[0] + 3 * ((size_t) jt * w + it), A.B, bad, dx, dy);
        if (it > w - 2 || jt > h - 2 || it < 1 || jt < 1) continue;
        const float s = __fsqrt_rn(ag);
        const int g = s < 48.0f ? (int) s : 48;                    // `if (g > 48) g = 48`; a NaN lands here too
        atomicAdd(&hist[g + 1], 1);
    }
    __syncthreads();
    report_nonfinite(bad, &A.ctl[PIX_FLAGS]);
    if (tid == 0) {
        int total = 0;
        for (int i = 1; i < 50; i++) total += hist[i];
        int th = total * A.cut + 0.5f;                             // computeHistQuantil :28; the bins from 50 on are empty
        int q = 90;
        for (int i = 0; i < 90; i++) {
            th -= i + 1 < 50 ? hist[i + 1] : 0;
            if (th < 0) { q = i; break; }
        }
        A.ths[blockIdx.x] = q + A.add;
    }
}

// makeHists :67-108
__global__ __launch_bounds__(256) void k_pix_smooth(PixArgs A) {
    const int c = blockIdx.x * 256 + threadIdx.x, w32 = A.w32, h32 = A.h32;
    if (c >= w32 * h32) return;
    const int x = c % w32, y = c / w32;
    const float *ths = A.ths;
    float sum = 0, num = 0;
    if (x > 0) {
        if (y > 0) { num++; sum += ths[x - 1 + (y - 1) * w32]; }
        if (y < h32 - 1) { num++; sum += ths[x - 1 + (y + 1) * w32]; }
        num++; sum += ths[x - 1 + y * w32];
    }
    if (x < w32 - 1) {
        if (y > 0) { num++; sum += ths[x + 1 + (y - 1) * w32]; }
        if (y < h32 - 1) { num++; sum += ths[x + 1 + (y + 1) * w32]; }
        num++; sum += ths[x + 1 + y * w32];
    }
    if (y > 0) { num++; sum += ths[x + (y - 1) * w32]; }
    if (y < h32 - 1) { num++; sum += ths[x + (y + 1) * w32]; }
    num++; sum += ths[x + y * w32];
    A.thsSmoothed[c] = (sum / num) * (sum / num);
}

// the pixels select never looks at (:242)
static __device__ __forceinline__ bool pix_outside(int xf, int yf, int w, int h) { return xf < 4 || xf >= w - 5 || yf < 4 || yf > h - 4; }

// L = lanes_per_block(pot) lanes per pot block (256 / L blocks per workgroup)
__global__ __launch_bounds__(256) void k_pix_masks(PixArgs A, int L) {
    const long long gid = (long long) blockIdx.x * 256 + threadIdx.x;
    const int b = (int) (gid / L), sub = (int) (gid % L), w = A.w, h = A.h, pot = A.pot;
    const bool valid = b < A.nbx * A.nby;
    const int bx = b % A.nbx, by = b / A.nbx, x0 = bx * pot, y0 = by * pot;
    unsigned m = 0;
    bool bad = false;
    if (valid) {
        const int mx = min(pot, w - x0), my = min(pot, h - y0);
        for (int p = sub; p < mx * my; p += L) {
            const int xf = x0 + p % mx, yf = y0 + p / mx;
            if (pix_outside(xf, yf, w, h)) continue;
            const float th0 = A.thsSmoothed[(xf >> 5) + (yf >> 5) * A.w32];
            float dx, dy;
            const float ag0 = abs_sq_grad(A.lv[0] + 3 * ((size_t) yf * w + xf), A.B, bad, dx, dy);
            if (ag0 > th0 * A.thFactor) {
                if (!A.sdd) { if (ag0 > 0) m = 0xffffu; }
                else for (int d = 0; d < 16; d++) if (fabsf(dx * PIX_DX[d] + dy * PIX_DY[d]) > 0) m |= 1u << d;
            }
        }
    }
    for (int o = L >> 1; o > 0; o >>= 1) m |= (unsigned) __shfl_xor((int) m, o, 64);
    if (valid && sub == 0) A.mask[pix_order(bx, by, A.nbx, A.nby)] = (unsigned short) m;
    report_nonfinite(bad, &A.ctl[PIX_FLAGS]);
}

// One workgroup; all of it stages the head of the random pattern in LDS, then wavefront 0 walks the pot blocks in the reference's order, 64 per step.
__global__ __launch_bounds__(1024) void k_pix_scan(PixArgs A, int NB, int rpn) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rpl[];
    const int tid = threadIdx.x, wh = A.w * A.h;
    for (int i = tid * 4; i < rpn; i += 4096) *(unsigned *) (rpl + i) = *(const unsigned *) (A.rp + i);
    __syncthreads();
    if (tid >= 64) return;
    const int lane = tid;
    int n2 = 0;
    int mnext = lane < NB ? A.mask[lane] : 0;
    for (int t0 = 0; t0 < NB; t0 += 64) {
        const int m = mnext;
        mnext = t0 + 64 + lane < NB ? A.mask[t0 + 64 + lane] : 0;
        // randomPattern[n2 .. n2 + 63]: a step adds at most 64 to n2, and block i of the step has seen at most i selections before it
        const int wi = n2 + lane;
        const int rw = wi < rpn ? rpl[wi] : (wi < wh ? A.rp[wi] : 0);
        unsigned long long sel;
        if (__ballot(m != 0 && m != 0xffff) == 0) sel = __ballot(m == 0xffff);
        else {
            sel = 0;
            int k = 0, cur = __builtin_amdgcn_readlane(rw, 0);
#pragma unroll
            for (int i = 0; i < 64; i++) {
                const int mi = __builtin_amdgcn_readlane(m, i);
                const int s = (mi >> (cur & 15)) & 1;
                sel |= (unsigned long long) s << i;
                k += s;
                cur = __builtin_amdgcn_readlane(rw, k & 63);       // k <= i + 1: 64 only behind the last block, where cur is not read again
            }
        }
        const int before = __popcll(sel & ((1ull << lane) - 1));
        const int d = __shfl(rw, before, 64) & 15;
        if (t0 + lane < NB) A.dir[t0 + lane] = (unsigned char) d;
        n2 += __popcll(sel);
    }
    if (lane == 0) A.ctl[PIX_SCAN_N2] = n2;
}

// candidate key: larger score first, then the earlier place in the reference's order; 0 = none (scores are > 0, so their bits order as integers)
// (not select_dev.h's argmax_key: `order` is an unsigned place running across the pot blocks of a 4 pot block, biased by 0xffffffff)
static __device__ __forceinline__ unsigned long long pix_key(float s, unsigned order) { return ((unsigned long long) (unsigned) __float_as_int(s) << 32) | (0xffffffffu - order); }

// one wavefront per 4 pot block (:209-311)
__global__ __launch_bounds__(256) void k_pix_select(PixArgs A) {
    const int lane = threadIdx.x & 63, nbx = A.nbx, nby = A.nby, nb4x = (nbx + 3) >> 2, nb4y = (nby + 3) >> 2;
    const int b4 = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b4 >= nb4x * nb4y) return;
    const int X4 = b4 % nb4x, Y4 = b4 / nb4x, cx = min(4, nbx - 4 * X4), cy = min(4, nby - 4 * Y4), w = A.w, h = A.h, pot = A.pot;
    const float thF = A.thFactor, dw1 = A.dw1, dw2 = dw1 * dw1;
    // lane l < 16: mask and direction of pot block (l & 3, l >> 2) of this 4 pot block
    int myDir = 0; bool mySel = false;
    if (lane < 16 && (lane & 3) < cx && (lane >> 2) < cy) {
        const int t = pix_order(4 * X4 + (lane & 3), 4 * Y4 + (lane >> 2), nbx, nby);
        myDir = A.dir[t];
        mySel = (A.mask[t] >> myDir) & 1;
    }
    const unsigned selBits = (unsigned) __ballot(mySel);
    const int d4 = __shfl(myDir, 0, 64);
    const float d4x = PIX_DX[d4], d4y = PIX_DY[d4];
    const bool need3 = selBits == 0;
    unsigned long long best4 = 0; int idx4 = 0;
    unsigned ord = 0;
    bool any2 = false, bad = false;
    for (int b2 = 0; b2 < 4; b2++) {
        const int x2 = b2 & 1, y2 = b2 >> 1;
        if (2 * x2 >= cx || 2 * y2 >= cy) continue;
        const bool need2 = (selBits & (0x33u << (2 * x2 + 8 * y2))) == 0;
        const int d3 = __shfl(myDir, 8 * y2 + 2 * x2, 64);
        const float d3x = PIX_DX[d3], d3y = PIX_DY[d3];
        unsigned long long best3 = 0; int idx3 = 0;
        for (int b1 = 0; b1 < 4; b1++) {
            const int lx = 2 * x2 + (b1 & 1), ly = 2 * y2 + (b1 >> 1);
            if (lx >= cx || ly >= cy) continue;
            const bool sel1 = (selBits >> (4 * ly + lx)) & 1;
            const int d2 = __shfl(myDir, 4 * ly + lx, 64);
            const float d2x = PIX_DX[d2], d2y = PIX_DY[d2];
            const int x0 = (4 * X4 + lx) * pot, y0 = (4 * Y4 + ly) * pot, mx = min(pot, w - x0), my = min(pot, h - y0), np = mx * my;
            if (sel1 || need2 || need3) {
                unsigned long long best2 = 0; int idx2 = 0;
                for (int p = lane; p < np; p += 64) {
                    const int xf = x0 + p % mx, yf = y0 + p / mx;
                    if (pix_outside(xf, yf, w, h)) continue;
                    const int idx = xf + w * yf;
                    const float pixelTH0 = A.thsSmoothed[(xf >> 5) + (yf >> 5) * A.w32];
                    const float pixelTH1 = pixelTH0 * dw1;
                    const float pixelTH2 = pixelTH1 * dw2;
                    float dx, dy, ex, ey;
                    const float ag0 = abs_sq_grad(A.lv[0] + 3 * (size_t) idx, A.B, bad, dx, dy);
                    if (sel1 && ag0 > pixelTH0 * thF) {
                        const float s = A.sdd ? fabsf(dx * d2x + dy * d2y) : ag0;
                        if (s > 0) { const unsigned long long k = pix_key(s, (unsigned) p); if (k > best2) { best2 = k; idx2 = idx; } }
                    }
                    if (need2) {
                        const float ag1 = abs_sq_grad(A.lv[1] + 3 * (size_t) ((int) (xf * 0.5f + 0.25f) + (int) (yf * 0.5f + 0.25f) * A.w1), A.B, bad, ex, ey);
                        if (ag1 > pixelTH1 * thF) {
                            const float s = A.sdd ? fabsf(dx * d3x + dy * d3y) : ag1;
                            if (s > 0) { const unsigned long long k = pix_key(s, ord + (unsigned) p); if (k > best3) { best3 = k; idx3 = idx; } }
                        }
                    }
                    if (need3) {
                        const float ag2 = abs_sq_grad(A.lv[2] + 3 * (size_t) ((int) (xf * 0.25f + 0.125) + (int) (yf * 0.25f + 0.125) * A.w2), A.B, bad, ex, ey);
                        if (ag2 > pixelTH2 * thF) {
                            const float s = A.sdd ? fabsf(dx * d4x + dy * d4y) : ag2;
                            if (s > 0) { const unsigned long long k = pix_key(s, ord + (unsigned) p); if (k > best4) { best4 = k; idx4 = idx; } }
                        }
                    }
                }
                if (sel1) {
                    const unsigned long long top = wave_max(best2);
                    if (top != 0 && top == best2) { A.map[idx2] = 1; atomicAdd(&A.ctl[PIX_N2], 1); }
                }
            }
            ord += (unsigned) np;
        }
        if (need2) {
            const unsigned long long top = wave_max(best3);
            if (top != 0) any2 = true;
            if (top != 0 && top == best3) { A.map[idx3] = 2; atomicAdd(&A.ctl[PIX_N3], 1); }
        }
    }
    if (need3 && !any2) {
        const unsigned long long top = wave_max(best4);
        if (top != 0 && top == best4) { A.map[idx4] = 4; atomicAdd(&A.ctl[PIX_N4], 1); }
    }
    report_nonfinite(bad, &A.ctl[PIX_FLAGS]);
}

// makeMaps :150-163: the selected pixel of raster rank rn goes when randomPattern[rn] > charTH
__global__ __launch_bounds__(256) void k_pix_thin(PixArgs A, int charTH) {
    const int y = raster_row();
    if (y >= A.h) return;
    int gone = 0;
    raster_walk(A.map, A.w, 0, A.w, y, A.rowStart, [&](int x, int, int rank) { if ((int) A.rp[rank] > charTH) { A.map[(size_t) y * A.w + x] = 0; gone++; } });
    gone = wave_sum(gone);
    if ((threadIdx.x & 63) == 0 && gone) atomicAdd(&A.ctl[PIX_REMOVED], gone);
}

// FullSystem.cc:1290-1303: one record per selected pixel of the scanned rectangle, in raster order; my_type = the map value
__global__ __launch_bounds__(256) void k_pix_points(PixArgs A, ScanRect r, int hostIndex, ldso_immature_t *imm, float *type, int cap) {
    const int y = raster_row();
    if (y < r.y0 || y >= r.y1) return;
    bool bad = false;
    raster_walk(A.map, A.w, r.x0, r.x1, y, A.rowStart, [&](int x, int v, int rank) {
        if (rank < cap) { imm[rank] = imm_record(A.lv[0], (float) x, (float) y, A.w, A.h, hostIndex, bad); type[rank] = (float) v; }
    });
    report_nonfinite(bad, &A.ctl[PIX_FLAGS]);
}

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
struct ldso_pixsel {
    int device = 0, w = 0, h = 0, potential = 3, n = 0, cap = 0;
    hipStream_t stream = nullptr;
    bool ownStream = false, hasB = false;
    float cut = 0.5f, add = 7.0f, dw1 = 0.75f; int sdd = 1;          // Setting.cc:83-87
    unsigned char *d_rp = nullptr, *d_dir = nullptr, *d_map = nullptr;
    unsigned short *d_mask = nullptr;
    float *d_B = nullptr, *d_ths = nullptr, *d_thsSmoothed = nullptr, *d_type = nullptr;
    int32_t *d_rowCount = nullptr, *d_rowStart = nullptr, *d_ctl = nullptr;
    ldso_immature_t *d_imm = nullptr;
    StageClock<5> clock;                // make_maps: histogram, masks + scan, select, thinning (1 and 2 summed over the recursion rounds); make_points: the records
};

static int pix_size_ok(int w, int h) { return w % 32 == 0 && h % 32 == 0; }

static PixArgs pix_args(const ldso_pixsel *P, const ldso_pyramid *pyr, int pot, float thFactor) {
    PixArgs A;
    memset(&A, 0, sizeof(A));
    if (pyr) for (int l = 0; l < 3; l++) A.lv[l] = pyr->lv[l];
    A.w = P->w; A.h = P->h; A.w1 = P->w >> 1; A.w2 = P->w >> 2;
    A.B = P->hasB ? P->d_B : nullptr; A.rp = P->d_rp;
    A.ths = P->d_ths; A.thsSmoothed = P->d_thsSmoothed; A.w32 = P->w / 32; A.h32 = P->h / 32;
    A.cut = P->cut; A.add = P->add; A.dw1 = P->dw1; A.thFactor = thFactor; A.sdd = P->sdd;
    A.pot = pot; A.nbx = (P->w + pot - 1) / pot; A.nby = (P->h + pot - 1) / pot;
    A.mask = P->d_mask; A.dir = P->d_dir; A.map = P->d_map;
    A.rowStart = P->d_rowStart; A.ctl = P->d_ctl;
    return A;
}

extern "C" {

int ldso_pixsel_supported(int w, int h) {
    if (w <= 0 || h <= 0 || (long long) w * h >= (1ll << 30)) { ldso_set_error("ldso_pixsel_supported: bad size"); return LDSO_E_INVALID; }
    if (!pix_size_ok(w, h)) { ldso_set_error("ldso_pixsel: width and height must be multiples of 32 (thsSmoothed is undefined elsewhere)"); return LDSO_E_UNSUPPORTED; }
    return LDSO_OK;
}

int ldso_pixsel_plan(const int counts[3], float density, int potential, int recursions_left, int *action, int *new_potential, int *char_th) {
    REQ(counts && potential >= 1 && density > 0 && counts[0] >= 0 && counts[1] >= 0 && counts[2] >= 0, "ldso_pixsel_plan: bad arguments (potential >= 1, density > 0)");
    float numHave = counts[0] + counts[1] + counts[2];             // :125
    const float numWant = density;
    const float quotia = numWant / numHave;
    const float K = numHave * (potential + 1) * (potential + 1);  // :129
    int idealPotential = sqrtf(K / numWant) - 1;                   // :130
    if (idealPotential < 1) idealPotential = 1;
    int act = 0, cth = -1;
    if (recursions_left > 0 && quotia > 1.25 && potential > 1) {   // :133-140
        if (idealPotential >= potential) idealPotential = potential - 1;
        act = 1;
    } else if (recursions_left > 0 && quotia < 0.25) {             // :141-147
        if (idealPotential <= potential) idealPotential = potential + 1;
        act = 1;
    } else if (quotia < 0.95) cth = (unsigned char) (255 * quotia); // :150-153
    if (action) *action = act;
    if (new_potential) *new_potential = idealPotential;
    if (char_th) *char_th = cth;
    return LDSO_OK;
}

int ldso_pixsel_destroy(ldso_pixsel_t *P) {
    if (!P) return LDSO_OK;
    (void) hipSetDevice(P->device);
    (void) hipDeviceSynchronize();
    for (void *d : {(void *) P->d_rp, (void *) P->d_dir, (void *) P->d_map, (void *) P->d_mask, (void *) P->d_B, (void *) P->d_ths, (void *) P->d_thsSmoothed, (void *) P->d_type,
                    (void *) P->d_rowCount, (void *) P->d_rowStart, (void *) P->d_ctl, (void *) P->d_imm}) if (d) (void) hipFree(d);
    P->clock.destroy();
    if (P->ownStream && P->stream) (void) hipStreamDestroy(P->stream);
    delete P;
    return LDSO_OK;
}

// the allocations and uploads of ldso_pixsel_create: the first failure is reported as what it is
static int pix_create_body(ldso_pixsel *P, const unsigned char *random_pattern) {
    const size_t wh = (size_t) P->w * P->h, cells = (size_t) (P->w / 32) * (P->h / 32);
    CHK(hipStreamCreateWithFlags(&P->stream, hipStreamNonBlocking));
    P->ownStream = true;
    CHK(hipMalloc(&P->d_rp, wh)); CHK(hipMalloc(&P->d_dir, wh)); CHK(hipMalloc(&P->d_map, wh)); CHK(hipMalloc(&P->d_mask, wh * 2));
    CHK(hipMalloc(&P->d_B, 256 * 4)); CHK(hipMalloc(&P->d_ths, cells * 4)); CHK(hipMalloc(&P->d_thsSmoothed, cells * 4));
    CHK(hipMalloc(&P->d_rowCount, (size_t) P->h * 4)); CHK(hipMalloc(&P->d_rowStart, (size_t) P->h * 4)); CHK(hipMalloc(&P->d_ctl, 8 * 4));
    RUN(P->clock.create());
    CHK(hipMemcpy(P->d_rp, random_pattern, wh, hipMemcpyHostToDevice));
    return zero_fill(P->d_map, wh);
}

int ldso_pixsel_create(int device, int w, int h, const unsigned char *random_pattern, ldso_pixsel_t **out) {
    REQ(out && random_pattern, "ldso_pixsel_create: null argument");
    RUN(ldso_pixsel_supported(w, h));
    RUN(open_device(device, "ldso_pixsel_create"));
    ldso_pixsel *P = new ldso_pixsel();
    P->device = device; P->w = w; P->h = h;
    return finish_create(pix_create_body(P, random_pattern), P, out, ldso_pixsel_destroy);
}

int ldso_pixsel_set_stream(ldso_pixsel_t *P, void *s) {
    REQ(P, "ldso_pixsel_set_stream: null handle");
    return swap_stream(P->stream, P->ownStream, s);
}

int ldso_pixsel_set_response(ldso_pixsel_t *P, const float *B) {
    REQ(P, "ldso_pixsel_set_response: null handle");
    CHK(hipSetDevice(P->device));
    if (B) { CHK(hipMemcpyAsync(P->d_B, B, 256 * 4, hipMemcpyHostToDevice, P->stream)); CHK(hipStreamSynchronize(P->stream)); }
    P->hasB = B != nullptr;
    return LDSO_OK;
}

int ldso_pixsel_set_settings(ldso_pixsel_t *P, float minGradHistCut, float minGradHistAdd, float gradDownweightPerLevel, int selectDirectionDistribution) {
    REQ(P && std::isfinite(minGradHistCut) && std::isfinite(minGradHistAdd) && std::isfinite(gradDownweightPerLevel), "ldso_pixsel_set_settings: bad arguments");
    P->cut = minGradHistCut; P->add = minGradHistAdd; P->dw1 = gradDownweightPerLevel; P->sdd = selectDirectionDistribution != 0;
    return LDSO_OK;
}

int ldso_pixsel_set_potential(ldso_pixsel_t *P, int potential) {
    REQ(P && potential >= 1, "ldso_pixsel_set_potential: bad arguments (potential >= 1)");
    P->potential = potential;
    return LDSO_OK;
}

int ldso_pixsel_get_potential(ldso_pixsel_t *P, int *potential) {
    REQ(P && potential, "ldso_pixsel_get_potential: null argument");
    *potential = P->potential;
    return LDSO_OK;
}

int ldso_pixsel_profile(ldso_pixsel_t *P, int enable, float us_out[5]) {
    REQ(P, "ldso_pixsel_profile: null handle");
    return P->clock.report(P->device, enable, us_out);
}

int ldso_pixsel_make_maps(ldso_pixsel_t *P, ldso_pyramid_t *pyr, float density, int recursions_left, float th_factor, int *n_out, int counts_out[3], int *potential_used) {
    REQ(P && pyr, "ldso_pixsel_make_maps: null argument");
    REQ(density > 0 && std::isfinite(density) && std::isfinite(th_factor) && recursions_left >= 0, "ldso_pixsel_make_maps: bad arguments (density > 0, recursions_left >= 0)");
    hipStream_t st = P->stream;
    RUN(pyramid_wait(pyr, P->device, P->w, P->h, 3, st, "ldso_pixsel_make_maps", "the selector (device, size, three levels)"));
    const size_t wh = (size_t) P->w * P->h;
    StageClock<5> &clk = P->clock.begin();
    float usAcc[5] = {0, 0, 0, 0, 0};
    int pot = P->potential, ctl[8] = {0}, flags = 0;
    PixArgs A = pix_args(P, pyr, pot, th_factor);
    CHK(hipMemsetAsync(P->d_ctl, 0, 8 * 4, st));
    // one histogram pass per call: the recursion reuses it (gradHistFrame, :119)
    RUN(clk.mark(0, st));
    hipLaunchKernelGGL(k_pix_hist, dim3(A.w32 * A.h32), dim3(256), 0, st, A);
    CHK(hipGetLastError());
    hipLaunchKernelGGL(k_pix_smooth, dim3((A.w32 * A.h32 + 255) / 256), dim3(256), 0, st, A);
    CHK(hipGetLastError());
    RUN(clk.mark(1, st));
    const int rpn = (int) std::min<size_t>(wh, PIX_RP_LDS);
    int act = 0, ideal = pot, charTH = -1, counts[3] = {0, 0, 0};
    for (bool first = true;; first = false) {
        A = pix_args(P, pyr, pot, th_factor);
        const int NB = A.nbx * A.nby, L = lanes_per_block(pot);
        if (!first) { CHK(hipMemsetAsync(P->d_ctl + PIX_N2, 0, 3 * 4, st)); RUN(clk.mark(1, st)); }
        CHK(hipMemsetAsync(P->d_map, 0, wh, st));
        hipLaunchKernelGGL(k_pix_masks, dim3((unsigned) (((long long) NB * L + 255) / 256)), dim3(256), 0, st, A, L);
        CHK(hipGetLastError());
        CHK(launch_lds(k_pix_scan, dim3(1), dim3(1024), (size_t) rpn, st, A, NB, rpn));
        RUN(clk.mark(2, st));
        hipLaunchKernelGGL(k_pix_select, dim3((((A.nbx + 3) / 4) * ((A.nby + 3) / 4) + 3) / 4), dim3(256), 0, st, A);
        CHK(hipGetLastError());
        RUN(clk.mark(3, st));
        // the recursion decision needs the three counts: one wait per select pass
        CHK(hipMemcpyAsync(ctl, P->d_ctl, 8 * 4, hipMemcpyDeviceToHost, st));
        CHK(hipStreamSynchronize(st));
        for (int i = first ? 0 : 1; i < 3; i++) { float us = 0; RUN(clk.lap(i, us)); usAcc[i] += us; }
        flags |= ctl[PIX_FLAGS];
        counts[0] = ctl[PIX_N2]; counts[1] = ctl[PIX_N3]; counts[2] = ctl[PIX_N4];
        // two kernels count the level-1 selections: the scan from the masks, the select pass from the pixels it marked
        if (ctl[PIX_SCAN_N2] != ctl[PIX_N2]) { ldso_set_error("ldso_pixsel_make_maps: the scan and the select pass disagree on n2"); return LDSO_E_HIP; }
        RUN(ldso_pixsel_plan(counts, density, pot, recursions_left, &act, &ideal, &charTH));
        if (!act) break;
        pot = ideal; recursions_left--;                           // :139-140 / :145-146
    }
    int n = counts[0] + counts[1] + counts[2];
    if (charTH >= 0 && n > 0) {
        RUN(clk.mark(3, st));
        RUN(raster_count(P->d_map, P->w, P->h, ScanRect{0, P->w, 0, P->h}, P->d_rowCount, P->d_rowStart, P->d_ctl + PIX_TOTAL, st, nullptr));          // the whole image; no total on the host
        hipLaunchKernelGGL(k_pix_thin, raster_grid(P->h), dim3(256), 0, st, A, charTH);
        CHK(hipGetLastError());
        RUN(clk.mark(4, st));
        CHK(hipMemcpyAsync(ctl, P->d_ctl, 8 * 4, hipMemcpyDeviceToHost, st));
        CHK(hipStreamSynchronize(st));
        RUN(clk.lap(3, usAcc[3]));
        n -= ctl[PIX_REMOVED];
    }
    for (int i = 0; i < 4; i++) clk.set(i, usAcc[i]);
    P->potential = ideal;                                          // :165
    if (n_out) *n_out = n;
    if (counts_out) for (int i = 0; i < 3; i++) counts_out[i] = counts[i];
    if (potential_used) *potential_used = pot;
    if (flags & SEL_FLAG_NONFINITE) { ldso_set_error("ldso_pixsel_make_maps: non-finite pixel"); return LDSO_E_NONFINITE; }
    return LDSO_OK;
}

int ldso_pixsel_get_map(ldso_pixsel_t *P, float *map_out) {
    REQ(P && map_out, "ldso_pixsel_get_map: null argument");
    CHK(hipSetDevice(P->device));
    const size_t wh = (size_t) P->w * P->h;
    std::vector<unsigned char> m(wh);
    CHK(hipMemcpyAsync(m.data(), P->d_map, wh, hipMemcpyDeviceToHost, P->stream));
    CHK(hipStreamSynchronize(P->stream));
    for (size_t i = 0; i < wh; i++) map_out[i] = (float) m[i];
    return LDSO_OK;
}

int ldso_pixsel_get_thresholds(ldso_pixsel_t *P, float *ths_out, float *ths_smoothed_out) {
    REQ(P, "ldso_pixsel_get_thresholds: null handle");
    CHK(hipSetDevice(P->device));
    const size_t bytes = (size_t) (P->w / 32) * (P->h / 32) * 4;
    if (ths_out) CHK(hipMemcpyAsync(ths_out, P->d_ths, bytes, hipMemcpyDeviceToHost, P->stream));
    if (ths_smoothed_out) CHK(hipMemcpyAsync(ths_smoothed_out, P->d_thsSmoothed, bytes, hipMemcpyDeviceToHost, P->stream));
    CHK(hipStreamSynchronize(P->stream));
    return LDSO_OK;
}

int ldso_pixsel_make_points(ldso_pixsel_t *P, ldso_pyramid_t *pyr, int host_index, int *n_out) {
    REQ(P && pyr, "ldso_pixsel_make_points: null argument");
    hipStream_t st = P->stream;
    RUN(pyramid_wait(pyr, P->device, P->w, P->h, 1, st, "ldso_pixsel_make_points", "the selector (device, size)"));
    PixArgs A = pix_args(P, pyr, 1, 1.0f);
    const ScanRect r = scan_rect(P->w, P->h);
    StageClock<5> &clk = P->clock.begin();
    CHK(hipMemsetAsync(P->d_ctl, 0, 8 * 4, st));
    RUN(clk.mark(4, st));
    int n = 0, ctl[8] = {0};
    RUN(raster_count(P->d_map, P->w, P->h, r, P->d_rowCount, P->d_rowStart, P->d_ctl + PIX_TOTAL, st, &n));
    if (n > P->cap) {                                              // the record buffers grow to what a call needs
        (void) hipFree(P->d_imm); (void) hipFree(P->d_type);
        P->d_imm = nullptr; P->d_type = nullptr; P->cap = 0;
        const int cap = std::max(n, 4096);
        CHK(hipMalloc(&P->d_imm, (size_t) cap * sizeof(ldso_immature_t)));
        CHK(hipMalloc(&P->d_type, (size_t) cap * 4));
        P->cap = cap;
    }
    P->n = 0;
    if (n > 0) {
        hipLaunchKernelGGL(k_pix_points, raster_grid(P->h), dim3(256), 0, st, A, r, host_index, P->d_imm, P->d_type, P->cap);
        CHK(hipGetLastError());
    }
    RUN(clk.mark(5, st));
    CHK(hipMemcpyAsync(ctl, P->d_ctl, 8 * 4, hipMemcpyDeviceToHost, st));
    CHK(hipStreamSynchronize(st));
    RUN(clk.read(4));
    P->n = n;
    if (n_out) *n_out = n;
    if (ctl[PIX_FLAGS] & SEL_FLAG_NONFINITE) { ldso_set_error("ldso_pixsel_make_points: non-finite colour"); return LDSO_E_NONFINITE; }
    return LDSO_OK;
}

int ldso_pixsel_get_points(ldso_pixsel_t *P, ldso_immature_t *out, float *type_out) {
    REQ(P && (P->n == 0 || out), "ldso_pixsel_get_points: bad arguments");
    CHK(hipSetDevice(P->device));
    if (P->n) {
        CHK(hipMemcpyAsync(out, P->d_imm, (size_t) P->n * sizeof(ldso_immature_t), hipMemcpyDeviceToHost, P->stream));
        if (type_out) CHK(hipMemcpyAsync(type_out, P->d_type, (size_t) P->n * 4, hipMemcpyDeviceToHost, P->stream));
    }
    CHK(hipStreamSynchronize(P->stream));
    return LDSO_OK;
}

int ldso_pixsel_device(ldso_pixsel_t *P, const void **immature_dev, const void **type_dev, int *n) {
    REQ(P, "ldso_pixsel_device: null handle");
    if (immature_dev) *immature_dev = P->d_imm;
    if (type_dev) *type_dev = P->d_type;
    if (n) *n = P->n;
    return LDSO_OK;
}

}  // extern "C"

// for ldso_init_set_first_frame (init_first.hip), which scans the level-0 map where it lies
__attribute__((visibility("hidden"))) const unsigned char *pix_map_device(const ldso_pixsel *P, int *w, int *h, int *device) {
    *w = P->w; *h = P->h; *device = P->device;
    return P->d_map;
}
