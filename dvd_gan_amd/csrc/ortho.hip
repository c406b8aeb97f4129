// Orthogonal regularization of fp32 master weights (Brock et al. 2019, eq. 3): for every matrix W [h][w] of a table,
//   M = (W W^T) with a zero diagonal,   g += 2 beta * M W,   penalty = sum 1/2 ||M||_F^2.
// Two launches serve the whole table, both on v_mfma_f32_32x32x2_f32 (the operands are fp32 masters: exact products):
//
//   Gram   one workgroup per 64 x 64 tile (I, J >= I) of the upper triangle of M; four waves, one 32 x 32 MFMA tile each.  Both
//          operands are row blocks of the same W and rows are K-contiguous: [64 rows][32 k] slabs go through LDS with coalesced
//          row loads (row pitch 33 floats: the fragment reads of 32 rows at one k hit 32 banks), the next slab's loads are in
//          flight while the current one is multiplied, a diagonal tile stages one slab.  The tile is stored with exact zeros on
//          the diagonal and mirrored into (J, I); its sum of squares (fp64) goes into the slot of this block.
//   apply  one workgroup per 64 x 128 tile of M W; K = h; four waves, 32 x 64 each.  M is symmetric bit for bit (the products of
//          (i, j) and (j, i) are the same numbers added in the same order), so its operand is read along rows like W's:
//          both slabs are [16 k][columns] with coalesced loads and conflict-free fragment reads.  Epilogue: g = fl(g + fl(s acc)).
//
// Blocks are laid out item by item in the planner's order (deepest K first: the nine 512 x 19200 gates have 19200-deep chains
// on a few dozen tiles each and must not start last).  Every output element is written by exactly one thread, every sum has a
// fixed order: no atomics, an item's result does not depend on what else the table holds.  All loads are scalar dwords with
// bounds checks: offsets in the flat parameter buffer and row pitches are only 4-byte aligned.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>
#include "common.h"

namespace {

constexpr int OR_THREADS = 256;
constexpr int OG_TILE = 64, OG_KC = 32, OG_LD = OG_KC + 1;           // Gram: tile side, k per slab, LDS row pitch
constexpr int OA_TI = 64, OA_TJ = 128, OA_KC = 16;                   // apply: tile rows x columns, k per slab
constexpr int C_ = DVD_ORTHO_COLS;

// rank search: the last rank whose item starts at or before block `bid` (items without blocks sit at the end with first = total)
__device__ __forceinline__ int ortho_find(const long long* tab, int n, int order_col, int first_col, long long bid) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tab[tab[mid * C_ + order_col] * C_ + first_col] <= bid) lo = mid; else hi = mid;
    }
    return (int)tab[lo * C_ + order_col];
}

__global__ __launch_bounds__(OR_THREADS) void ortho_gram_kernel(const float* __restrict__ p, const long long* __restrict__ tab, int n,
                                                                float* __restrict__ ws, double* __restrict__ part) {
    __shared__ float sA[OG_TILE * OG_LD], sB[OG_TILE * OG_LD];
    __shared__ double red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const long long bid = blockIdx.x;
    const int it = ortho_find(tab, n, DVD_ORTHO_GORDER, DVD_ORTHO_GRAM0, bid);
    const long long* row = tab + (long long)it * C_;
    const int h = (int)row[DVD_ORTHO_H];
    const long long w = row[DVD_ORTHO_W];
    const float* W = p + row[DVD_ORTHO_OFF];
    float* M = ws + row[DVD_ORTHO_WS];
    // tile (I, J >= I) number t of the upper triangle, row by row
    int t = (int)(bid - row[DVD_ORTHO_GRAM0]), I = 0;
    for (int len = (h + OG_TILE - 1) / OG_TILE; t >= len; --len) { t -= len; ++I; }
    const int J = I + t;
    const bool diag = I == J;

    const int kk = tid & 31, r0 = tid >> 5;                          // staging: 8 rows x 32 k per pass, 8 passes
    float ra[8], rb[8];
    auto gload = [&](long long k0) {
        const long long k = k0 + kk;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int ri = I * OG_TILE + r0 + 8 * j, rj = J * OG_TILE + r0 + 8 * j;
            ra[j] = (ri < h && k < w) ? W[(long long)ri * w + k] : 0.f;
            rb[j] = (!diag && rj < h && k < w) ? W[(long long)rj * w + k] : 0.f;
        }
    };
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    // a wave whose 32 rows or 32 columns lie past h has nothing to compute (it still stages and keeps the barriers)
    const bool active = I * OG_TILE + wm * 32 < h && J * OG_TILE + wn * 32 < h;
    const float* As = sA + (wm * 32 + (lane & 31)) * OG_LD + (lane >> 5);
    const float* Bs = (diag ? sA : sB) + (wn * 32 + (lane & 31)) * OG_LD + (lane >> 5);

    gload(0);
    for (long long k0 = 0; k0 < w; k0 += OG_KC) {
        __syncthreads();                                             // the previous slab has been read
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            sA[(r0 + 8 * j) * OG_LD + kk] = ra[j];
            if (!diag) sB[(r0 + 8 * j) * OG_LD + kk] = rb[j];
        }
        __syncthreads();
        if (k0 + OG_KC < w) gload(k0 + OG_KC);                       // (the ragged last slab is zero-filled past w)
        if (active) {
#pragma unroll
            for (int k = 0; k < OG_KC; k += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[k], Bs[k], acc, 0, 0, 0);
        }
    }

    double sq = 0.0;
    if (active) {
        const int gj = J * OG_TILE + wn * 32 + (lane & 31);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int gi = I * OG_TILE + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            if (gi < h && gj < h) {
                const float v = gi == gj ? 0.f : acc[r];
                M[(long long)gi * h + gj] = v;
                if (!diag) M[(long long)gj * h + gi] = v;
                sq += (double)v * (double)v;
            }
        }
        if (!diag) sq *= 2.0;                                        // the mirrored tile holds the same values
    }
    sq = wave_sum_d(sq);
    if (lane == 0) red[wave] = sq;
    __syncthreads();
    if (tid == 0) part[bid] = ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(OR_THREADS) void ortho_apply_kernel(const float* __restrict__ p, float* __restrict__ g,
                                                                 const long long* __restrict__ tab, int n,
                                                                 const float* __restrict__ ws, float s) {
    __shared__ float sM[OA_KC * OA_TI], sW[OA_KC * OA_TJ];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const long long bid = blockIdx.x;
    const int it = ortho_find(tab, n, DVD_ORTHO_AORDER, DVD_ORTHO_APPLY0, bid);
    const long long* row = tab + (long long)it * C_;
    const int h = (int)row[DVD_ORTHO_H];
    const long long w = row[DVD_ORTHO_W];
    const float* W = p + row[DVD_ORTHO_OFF];
    float* G = g + row[DVD_ORTHO_OFF];
    const float* M = ws + row[DVD_ORTHO_WS];
    const long long t = bid - row[DVD_ORTHO_APPLY0];
    const int nbi = (h + OA_TI - 1) / OA_TI;
    const int bi = (int)(t % nbi);                                   // row tiles fastest: neighbours share the slab of W
    const long long bj = t / nbi;

    const int mc = tid & 63, mr = tid >> 6, wc = tid & 127, wr = tid >> 7;
    const int gmi = bi * OA_TI + mc;
    const long long gwj = bj * OA_TJ + wc;
    float rm[4], rw[8];
    auto gload = [&](int k0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = k0 + mr + 4 * j;
            rm[j] = (k < h && gmi < h) ? M[(long long)k * h + gmi] : 0.f;       // M[k][i] == M[i][k]
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = k0 + wr + 2 * j;
            rw[j] = (k < h && gwj < w) ? W[(long long)k * w + gwj] : 0.f;
        }
    };
    f32x16 acc[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc[0][r] = 0.f; acc[1][r] = 0.f; }
    const bool active = bi * OA_TI + wm * 32 < h && bj * OA_TJ + wn * 64 < w;
    const float* As = sM + (lane >> 5) * OA_TI + wm * 32 + (lane & 31);
    const float* Bs = sW + (lane >> 5) * OA_TJ + wn * 64 + (lane & 31);

    gload(0);
    for (int k0 = 0; k0 < h; k0 += OA_KC) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) sM[(mr + 4 * j) * OA_TI + mc] = rm[j];
#pragma unroll
        for (int j = 0; j < 8; ++j) sW[(wr + 2 * j) * OA_TJ + wc] = rw[j];
        __syncthreads();
        if (k0 + OA_KC < h) gload(k0 + OA_KC);
        if (active) {
#pragma unroll
            for (int k = 0; k < OA_KC; k += 2) {
                const float a = As[k * OA_TI], b0 = Bs[k * OA_TJ], b1 = Bs[k * OA_TJ + 32];
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, acc[1], 0, 0, 0);
            }
        }
    }
    if (!active) return;
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) {
        const long long gj = bj * OA_TJ + wn * 64 + tn * 32 + (lane & 31);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int gi = bi * OA_TI + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            if (gi < h && gj < w) {
#pragma clang fp contract(off)
                const long long idx = (long long)gi * w + gj;
                const float term = s * acc[tn][r];                   // two roundings, never an fma: tests replay them bit for bit
                G[idx] = G[idx] + term;
            }
        }
    }
}

// *penalty = 1/2 * (the tile slots added in a fixed order: a strided sum per thread, lanes by xor shuffles, the four waves in order)
__global__ __launch_bounds__(OR_THREADS) void ortho_penalty_kernel(const double* __restrict__ part, long long nslots,
                                                                   double* __restrict__ penalty) {
    __shared__ double red[4];
    double s = 0.0;
    for (long long i = threadIdx.x; i < nslots; i += OR_THREADS) s += part[i];
    s = wave_sum_d(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) *penalty = 0.5 * (((red[0] + red[1]) + red[2]) + red[3]);
}

struct OrthoPlan { long long ws_floats, part_off, gram_blocks, apply_blocks; };

// Fills the planner's columns of items[n][DVD_ORTHO_COLS] (host memory).  Workspace: M_0 | M_1 | ... | (even offset) one double per Gram block.
int ortho_plan(long long* items, int n, OrthoPlan* plan) {
    if (!items || n < 1) return DVD_E_ARG;
    long long ws = 0;
    for (int i = 0; i < n; ++i) {
        long long* r = items + (long long)i * C_;
        if (r[DVD_ORTHO_OFF] < 0 || r[DVD_ORTHO_H] < 1 || r[DVD_ORTHO_W] < 1) return DVD_E_ARG;
        if (r[DVD_ORTHO_H] > DVD_ORTHO_MAX_H || r[DVD_ORTHO_W] > (1ll << 40) / r[DVD_ORTHO_H] || r[DVD_ORTHO_OFF] > (1ll << 40))
            return DVD_E_SHAPE;
        r[DVD_ORTHO_WS] = ws;
        if (r[DVD_ORTHO_H] > 1) ws += r[DVD_ORTHO_H] * r[DVD_ORTHO_H];
    }
    // launch order: deepest product first (Gram: K = w, apply: K = h), ties in table order; items without blocks (h = 1) last
    std::vector<int> order(n);
    for (int pass = 0; pass < 2; ++pass) {
        const int key = pass ? DVD_ORTHO_H : DVD_ORTHO_W, ocol = pass ? DVD_ORTHO_AORDER : DVD_ORTHO_GORDER;
        const int fcol = pass ? DVD_ORTHO_APPLY0 : DVD_ORTHO_GRAM0;
        for (int i = 0; i < n; ++i) order[i] = i;
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
            const long long* ra = items + (long long)a * C_, * rb = items + (long long)b * C_;
            const bool ea = ra[DVD_ORTHO_H] == 1, eb = rb[DVD_ORTHO_H] == 1;
            if (ea != eb) return eb;
            return ra[key] > rb[key];
        });
        long long blocks = 0;
        for (int r = 0; r < n; ++r) {
            long long* it = items + (long long)order[r] * C_;
            items[(long long)r * C_ + ocol] = order[r];
            it[fcol] = blocks;
            const long long h = it[DVD_ORTHO_H], w = it[DVD_ORTHO_W];
            if (h == 1) continue;
            if (pass) {
                blocks += ((h + OA_TI - 1) / OA_TI) * ((w + OA_TJ - 1) / OA_TJ);
            } else {
                const long long nb = (h + OG_TILE - 1) / OG_TILE;
                blocks += nb * (nb + 1) / 2;
            }
            if (blocks > 0x7fffffffll) return DVD_E_SHAPE;
        }
        (pass ? plan->apply_blocks : plan->gram_blocks) = blocks;
    }
    plan->part_off = (ws + 1) & ~1ll;
    plan->ws_floats = plan->part_off + 2 * plan->gram_blocks;
    return DVD_OK;
}

}  // namespace

extern "C" long long dvd_ortho_prepare(long long* items, int n, long long* ws_floats) {
    if (!ws_floats) return DVD_E_ARG;
    OrthoPlan plan;
    const int rc = ortho_plan(items, n, &plan);
    if (rc != DVD_OK) return rc;
    *ws_floats = plan.ws_floats;
    return plan.gram_blocks;
}

extern "C" int dvd_ortho_grad(const float* p, float* g, const long long* items_host, const long long* items_dev, int n,
                              float strength, float* ws, double* penalty, void* stream) {
    if (!p || !g || !items_host || !items_dev || n < 1) return DVD_E_ARG;
    if (!std::isfinite(strength) || strength < 0.f) return DVD_E_ARG;
    std::vector<long long> tab(items_host, items_host + (size_t)n * C_);
    OrthoPlan plan;
    const int rc = ortho_plan(tab.data(), n, &plan);
    if (rc != DVD_OK) return rc;
    if (std::memcmp(tab.data(), items_host, sizeof(long long) * (size_t)n * C_) != 0) return DVD_E_ARG;    // not a prepared table
    if (plan.gram_blocks == 0) {                                     // nothing but h = 1 items
        if (penalty && hipMemsetAsync(penalty, 0, sizeof(double), (hipStream_t)stream) != hipSuccess) return DVD_E_LAUNCH;
        return DVD_OK;
    }
    if (!ws || ((uintptr_t)ws & 7) || ((uintptr_t)p & 3) || ((uintptr_t)g & 3)) return DVD_E_ARG;
    double* part = reinterpret_cast<double*>(ws + plan.part_off);
    const float s = 2.f * strength;                                  // exact doubling
    hipStream_t st = (hipStream_t)stream;
    ortho_gram_kernel<<<(unsigned)plan.gram_blocks, OR_THREADS, 0, st>>>(p, items_dev, n, ws, part);
    ortho_apply_kernel<<<(unsigned)plan.apply_blocks, OR_THREADS, 0, st>>>(p, g, items_dev, n, ws, s);
    if (penalty) ortho_penalty_kernel<<<1, OR_THREADS, 0, st>>>(part, plan.gram_blocks, penalty);
    return launch_status();
}
