// libdvdgan_hip_eval.so (include/dvdgan_hip_eval.h): the statistics behind FID / FVD / KID on sample features.
//
//   pool     [R][P][C] activation -> [R / g][C] = mean over g rows of sum_p relu(x).  One thread owns 8 (bf16) / 4 (fp32) channels of
//            one output row and walks its g * P input rows in order: 16-byte loads, fp32 sums, a single pass.
//   moments  S2 += (X - c)^T (X - c), S1 += sum (X - c).  One workgroup per 64 x 64 tile (I, J >= I) of the upper triangle; four
//            waves, one 32 x 32 tile of v_mfma_f32_32x32x2_f32 each, K = the n rows of the call.  X is [n][d] with d contiguous, so
//            both operands are [32 k][64 columns] slabs with coalesced row loads (256 B per wave and row) and conflict-free
//            fragment reads (lanes 0..31 read one k row, lanes 32..63 the next).  The pivot is subtracted while staging, the next
//            slab's loads are in flight while the current one is multiplied, a diagonal tile stages one slab and also owns the
//            S1 entries of its 64 columns (fp64 sums of the values it stages, per thread in row order, four row groups added in
//            order).  The fp32 tile is added once into its fp64 state tile.
//   kid      per subset the tiles (I, J >= I) of k(x, x) and k(y, y) and every tile of k(x, y); the gathered rows are K-contiguous
//            like ortho.hip's Gram operands: [64 rows][32 k] slabs, row pitch 33.  Epilogue in fp64: t = acc / d + 1, t^3, the
//            diagonal left out by position, off-diagonal tiles of the symmetric terms counted twice; the tile sum goes into the
//            slot of this block.  A second launch adds the slots of a subset in a fixed order and writes the result.
//
// Budgets (hipcc -O3, gfx950; the .res file beside the object must show no scratch for any kernel):
//   eval_moments_kernel   LDS 16 KB + 2 KB (two slabs, the S1 combine); 16 accumulator + 16 staging registers, 88 VGPRs as built
//   eval_kid_kernel       LDS 16.5 KB (two slabs of 64 x 33 floats); 16 accumulator + 16 staging + 32 row-offset registers, 80 VGPRs
//   both stay under 128 VGPRs (four workgroups per CU fit by registers and by LDS)
// Every output element has one owner and every sum a fixed order: no atomics.  All loads of X / Y are scalar dwords with bounds
// checks (row strides are only 4-byte aligned).
#include <algorithm>
#include "../common.h"
#include "../../../include/dvdgan_hip_eval.h"

namespace {

constexpr int EV_THREADS = 256;
constexpr int EV_T = DVD_EVAL_TILE;                 // tile side: four waves, 32 x 32 each
#ifndef DVD_EVAL_MOMENTS_KC                         // (a multiple of 4; the results do not depend on it.  64 was measured and buys
#define DVD_EVAL_MOMENTS_KC 32                      //  nothing: profiles/distmetrics_numbers.md)
#endif
constexpr int EM_KC = DVD_EVAL_MOMENTS_KC, EM_PASS = EM_KC / 4;   // moments: rows per slab, staging passes of 4 rows
constexpr int EK_KC = 32, EK_LD = EK_KC + 1;        // kid: k per slab, LDS row pitch
constexpr long long EV_MAX_ELEMS = 1ll << 40;
static_assert(EV_T == 64, "the kernels below are written for 64 x 64 tiles");

// tile number t of the upper triangle (row by row) of nb x nb tiles -> (I, J >= I)
__device__ __forceinline__ void tri_decode(int t, int nb, int& I, int& J) {
    I = 0;
    for (int len = nb; t >= len; --len) { t -= len; ++I; }
    J = I + t;
}

// ----------------------------------------------------------------------------- pool
template <typename T, int V> __device__ __forceinline__ void pool_load(const T* p, float (&v)[V]);
template <> __device__ __forceinline__ void pool_load<bf16_t, 8>(const bf16_t* p, float (&v)[8]) { load8<bf16_t>(p, v); }
template <> __device__ __forceinline__ void pool_load<float, 4>(const float* p, float (&v)[4]) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p);
    v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3];
}
template <> __device__ __forceinline__ void pool_load<bf16_t, 1>(const bf16_t* p, float (&v)[1]) { v[0] = bf16_to_f32(*p); }
template <> __device__ __forceinline__ void pool_load<float, 1>(const float* p, float (&v)[1]) { v[0] = *p; }

template <typename T, int V>
__global__ __launch_bounds__(EV_THREADS) void eval_pool_kernel(const T* __restrict__ x, long long Q, int P, int C, int g,
                                                               float* __restrict__ out) {
    const int cv_n = C / V;
    const long long total = Q * cv_n, rows = (long long)g * P;
    const float div = (float)g;
    for (long long i = (long long)blockIdx.x * EV_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * EV_THREADS) {
        const long long q = i / cv_n;
        const int c0 = (int)(i - q * cv_n) * V;
        const T* p = x + q * rows * C + c0;
        float acc[V];
#pragma unroll
        for (int e = 0; e < V; ++e) acc[e] = 0.f;
        for (long long r = 0; r < rows; ++r, p += C) {
            float v[V];
            pool_load<T, V>(p, v);
#pragma unroll
            for (int e = 0; e < V; ++e) acc[e] += fmaxf(v[e], 0.f);
        }
#pragma unroll
        for (int e = 0; e < V; ++e) out[q * C + c0 + e] = acc[e] / div;
    }
}

// ----------------------------------------------------------------------------- moments
// pivot[j] = fl(mean_k X[k][j]): per thread an fp64 sum over the rows k = kr, kr + 4, ...; the four row groups added in order
__global__ __launch_bounds__(EV_THREADS) void eval_pivot_kernel(const float* __restrict__ X, long long n, int d, long long ldx,
                                                                float* __restrict__ pivot) {
    __shared__ double red[4 * EV_T];
    const int col = threadIdx.x & 63, kr = threadIdx.x >> 6;
    const int gj = blockIdx.x * EV_T + col;
    double s = 0.0;
    if (gj < d)
        for (long long k = kr; k < n; k += 4) s += (double)X[k * ldx + gj];
    red[kr * EV_T + col] = s;
    __syncthreads();
    if (kr == 0 && gj < d)
        pivot[gj] = (float)((((red[col] + red[EV_T + col]) + red[2 * EV_T + col]) + red[3 * EV_T + col]) / (double)n);
}

__global__ __launch_bounds__(EV_THREADS) void eval_moments_kernel(const float* __restrict__ X, long long n, int d, long long ldx,
                                                                  const float* __restrict__ pivot, double* __restrict__ state,
                                                                  int first) {
    __shared__ float sA[EM_KC * EV_T], sB[EM_KC * EV_T];
    __shared__ double red[4 * EV_T];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int nb = (d + EV_T - 1) / EV_T;
    int I, J;
    tri_decode((int)blockIdx.x, nb, I, J);
    const bool diag = I == J;

    const int col = tid & 63, kr = tid >> 6;                         // staging: 4 rows x 64 columns per pass
    const int gi = I * EV_T + col, gj = J * EV_T + col;
    const bool ia = gi < d, ib = !diag && gj < d;
    const float ca = ia ? pivot[gi] : 0.f, cb = ib ? pivot[gj] : 0.f;
    float ra[EM_PASS], rb[EM_PASS];
    auto gload = [&](long long k0) {
#pragma unroll
        for (int j = 0; j < EM_PASS; ++j) {
            const long long k = k0 + kr + 4 * j;
            ra[j] = (ia && k < n) ? X[k * ldx + gi] : ca;            // rows past n and columns past d: the pivot itself, staged
            rb[j] = (ib && k < n) ? X[k * ldx + gj] : cb;            // as an exact zero
        }
    };
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    // a wave whose 32 rows or 32 columns lie past d has nothing to compute (it still stages and keeps the barriers)
    const bool active = I * EV_T + wm * 32 < d && J * EV_T + wn * 32 < d;
    const float* As = sA + (lane >> 5) * EV_T + wm * 32 + (lane & 31);
    const float* Bs = (diag ? sA : sB) + (lane >> 5) * EV_T + wn * 32 + (lane & 31);
    double s1 = 0.0;

    gload(0);
    for (long long k0 = 0; k0 < n; k0 += EM_KC) {
        __syncthreads();                                             // the previous slab has been read
#pragma unroll
        for (int j = 0; j < EM_PASS; ++j) {
            // the pivot is subtracted here, not at the load: nothing waits for the loads before the slab in LDS is multiplied
            const float ya = ra[j] - ca;
            sA[(kr + 4 * j) * EV_T + col] = ya;
            if (!diag) sB[(kr + 4 * j) * EV_T + col] = rb[j] - cb;
            if (diag) s1 += (double)ya;
        }
        __syncthreads();
        if (k0 + EM_KC < n) gload(k0 + EM_KC);
        if (active) {
#pragma unroll
            for (int k = 0; k < EM_KC; k += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[k * EV_T], Bs[k * EV_T], acc, 0, 0, 0);
        }
    }

    // the tile's own state: every entry has one owner (entries past d hold the zeros that were staged)
    if (active || first) {
        double* st = state + d + (long long)blockIdx.x * (EV_T * EV_T);
        const int lj = wn * 32 + (lane & 31);
        // all sixteen old values are requested before the first one is used (one round trip to memory, not sixteen)
        double old[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) old[r] = 0.0;
        if (!first) {
#pragma unroll
            for (int r = 0; r < 16; ++r) old[r] = st[(wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)) * EV_T + lj];
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) st[(wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)) * EV_T + lj] = old[r] + (double)acc[r];
    }
    if (diag) {
        red[kr * EV_T + col] = s1;
        __syncthreads();
        if (kr == 0 && ia) {
            const double s = ((red[col] + red[EV_T + col]) + red[2 * EV_T + col]) + red[3 * EV_T + col];
            state[gi] = first ? s : state[gi] + s;
        }
    }
}

// ----------------------------------------------------------------------------- kid
__global__ __launch_bounds__(EV_THREADS) void eval_kid_kernel(const float* __restrict__ X, long long ldx, const float* __restrict__ Y,
                                                              long long ldy, int d, const int* __restrict__ ix,
                                                              const int* __restrict__ iy, int s, int nb, double* __restrict__ slots) {
    __shared__ float sA[EV_T * EK_LD], sB[EV_T * EK_LD];
    __shared__ double red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int sub = blockIdx.y, t = blockIdx.x, tri = nb * (nb + 1) / 2;
    const int term = t < tri ? 0 : t < 2 * tri ? 1 : 2;              // k(x, x) | k(y, y) | k(x, y)
    int I, J;
    if (term < 2) {
        tri_decode(t - term * tri, nb, I, J);
    } else {
        I = (t - 2 * tri) / nb;
        J = (t - 2 * tri) % nb;
    }
    const bool sym = term < 2, diag = sym && I == J;
    const float* A = term == 1 ? Y : X;
    const float* B = term == 0 ? X : Y;
    const long long lda = term == 1 ? ldy : ldx, ldb = term == 0 ? ldx : ldy;
    const int* ta = (term == 1 ? iy : ix) + (long long)sub * s;
    const int* tb = (term == 0 ? ix : iy) + (long long)sub * s;

    const int kk = tid & 31, r0 = tid >> 5;                          // staging: 8 rows x 32 k per pass, 8 passes
    long long oa[8], ob[8];                                          // element offsets of this thread's gathered rows, -1 = past s
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int li = I * EV_T + r0 + 8 * j, lj = J * EV_T + r0 + 8 * j;
        oa[j] = li < s ? (long long)ta[li] * lda : -1;
        ob[j] = (!diag && lj < s) ? (long long)tb[lj] * ldb : -1;
    }
    float ra[8], rb[8];
    auto gload = [&](int k0) {
        const int k = k0 + kk;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            ra[j] = (oa[j] >= 0 && k < d) ? A[oa[j] + k] : 0.f;
            rb[j] = (ob[j] >= 0 && k < d) ? B[ob[j] + k] : 0.f;
        }
    };
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const bool active = I * EV_T + wm * 32 < s && J * EV_T + wn * 32 < s;
    const float* As = sA + (wm * 32 + (lane & 31)) * EK_LD + (lane >> 5);
    const float* Bs = (diag ? sA : sB) + (wn * 32 + (lane & 31)) * EK_LD + (lane >> 5);

    gload(0);
    for (int k0 = 0; k0 < d; k0 += EK_KC) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            sA[(r0 + 8 * j) * EK_LD + kk] = ra[j];
            if (!diag) sB[(r0 + 8 * j) * EK_LD + kk] = rb[j];
        }
        __syncthreads();
        if (k0 + EK_KC < d) gload(k0 + EK_KC);
        if (active) {
#pragma unroll
            for (int k = 0; k < EK_KC; k += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[k], Bs[k], acc, 0, 0, 0);
        }
    }

    double sum = 0.0;
    if (active) {
        const int gj = J * EV_T + wn * 32 + (lane & 31);
        const double dd = (double)d;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int gi = I * EV_T + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            if (gi < s && gj < s && !(sym && gi == gj)) {
                const double tt = (double)acc[r] / dd + 1.0;
                sum += tt * tt * tt;
            }
        }
        if (sym && !diag) sum *= 2.0;                                // the mirrored tile holds the same values
    }
    sum = wave_sum_d(sum);
    if (lane == 0) red[wave] = sum;
    __syncthreads();
    if (tid == 0) slots[(long long)sub * gridDim.x + t] = ((red[0] + red[1]) + red[2]) + red[3];
}

// one workgroup per subset: the slots of each term in a fixed order (a strided sum per thread, lanes by xor shuffles, the four
// waves in order), then the weights
__global__ __launch_bounds__(EV_THREADS) void eval_kid_reduce_kernel(const double* __restrict__ slots, int nb, int s,
                                                                     double* __restrict__ out, double* __restrict__ terms) {
    __shared__ double red[3][4];
    const int tri = nb * (nb + 1) / 2, per = 2 * tri + nb * nb;
    const double* p = slots + (long long)blockIdx.x * per;
    const int lo[4] = {0, tri, 2 * tri, per};
#pragma unroll
    for (int term = 0; term < 3; ++term) {
        double v = 0.0;
        for (int i = lo[term] + (int)threadIdx.x; i < lo[term + 1]; i += EV_THREADS) v += p[i];
        v = wave_sum_d(v);
        if ((threadIdx.x & 63) == 0) red[term][threadIdx.x >> 6] = v;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double sums[3];
#pragma unroll
    for (int term = 0; term < 3; ++term) sums[term] = ((red[term][0] + red[term][1]) + red[term][2]) + red[term][3];
    const double pairs = (double)s * (double)(s - 1), all = (double)s * (double)s;
    out[blockIdx.x] = sums[0] / pairs + sums[1] / pairs - 2.0 * sums[2] / all;
    if (terms)
        for (int term = 0; term < 3; ++term) terms[3ll * blockIdx.x + term] = sums[term];
}

inline bool strided_ok(long long rows, long long ld) { return ld <= EV_MAX_ELEMS / rows; }
inline int kid_nb(int s) { return (s + EV_T - 1) / EV_T; }

}  // namespace

#define S_ ((hipStream_t)stream)

extern "C" const char* dvd_eval_strerror(int code) {
    switch (code) {
        case DVD_OK: return "ok";
        case DVD_E_ARG: return "bad argument (null pointer / non-positive size / stride below the row length / group not dividing the rows / "
                               "subset size below 2 / index out of range / misaligned state)";
        case DVD_E_SHAPE: return "unsupported shape (feature width outside [1, 4096], too many subsets, too many elements)";
        case DVD_E_LAUNCH: return "kernel launch failed";
        default: return "unknown error";
    }
}

extern "C" int dvd_eval_pool_features(int dtype, const void* x, long long R, int P, int C, int g, float* out, void* stream) {
    if (!x || !out || (dtype != DVD_F32 && dtype != DVD_BF16) || R < 1 || P < 1 || C < 1 || g < 1 || R % g != 0) return DVD_E_ARG;
    if ((long long)P * C > EV_MAX_ELEMS / R) return DVD_E_SHAPE;
    const long long Q = R / g;
    const int V = dtype == DVD_BF16 ? 8 : 4;
    const bool vec = C % V == 0 && ((uintptr_t)x & 15) == 0;
    const long long threads = Q * (vec ? C / V : C);
    const unsigned grid = (unsigned)std::min<long long>((threads + EV_THREADS - 1) / EV_THREADS, 1 << 20);
    if (dtype == DVD_BF16) {
        if (vec) eval_pool_kernel<bf16_t, 8><<<grid, EV_THREADS, 0, S_>>>((const bf16_t*)x, Q, P, C, g, out);
        else eval_pool_kernel<bf16_t, 1><<<grid, EV_THREADS, 0, S_>>>((const bf16_t*)x, Q, P, C, g, out);
    } else {
        if (vec) eval_pool_kernel<float, 4><<<grid, EV_THREADS, 0, S_>>>((const float*)x, Q, P, C, g, out);
        else eval_pool_kernel<float, 1><<<grid, EV_THREADS, 0, S_>>>((const float*)x, Q, P, C, g, out);
    }
    return launch_status();
}

extern "C" long long dvd_eval_moments_state_doubles(int d) {
    if (d < 1 || d > DVD_EVAL_MAX_D) return -1;
    const long long nb = (d + EV_T - 1) / EV_T;
    return d + nb * (nb + 1) / 2 * (EV_T * EV_T);
}

extern "C" int dvd_eval_moments_update(const float* X, long long n, int d, long long ldx, float* pivot, double* state, int first,
                                       void* stream) {
    if (!X || !pivot || !state || n < 1) return DVD_E_ARG;
    if (d < 1 || d > DVD_EVAL_MAX_D) return DVD_E_SHAPE;
    if (ldx < d || ((uintptr_t)state & 7) || ((uintptr_t)X & 3) || ((uintptr_t)pivot & 3)) return DVD_E_ARG;
    if (!strided_ok(n, ldx)) return DVD_E_SHAPE;
    const int nb = (d + EV_T - 1) / EV_T;
    if (first) eval_pivot_kernel<<<nb, EV_THREADS, 0, S_>>>(X, n, d, ldx, pivot);
    eval_moments_kernel<<<nb * (nb + 1) / 2, EV_THREADS, 0, S_>>>(X, n, d, ldx, pivot, state, first ? 1 : 0);
    return launch_status();
}

extern "C" long long dvd_eval_kid_ws_doubles(int n_sub, int s) {
    if (n_sub < 1 || s < 2) return DVD_E_ARG;
    if (n_sub > DVD_EVAL_MAX_SUBSETS || s > 65536) return DVD_E_SHAPE;
    const long long nb = kid_nb(s);
    return (long long)n_sub * (nb * (nb + 1) + nb * nb);
}

extern "C" int dvd_eval_kid(const float* X, long long n, long long ldx, const float* Y, long long m, long long ldy, int d,
                            const int* ix_host, const int* iy_host, const int* ix_dev, const int* iy_dev, int n_sub, int s,
                            double* ws, double* out, double* terms, void* stream) {
    if (!X || !Y || !ix_host || !iy_host || !ix_dev || !iy_dev || !ws || !out) return DVD_E_ARG;
    if (n < 1 || m < 1 || n_sub < 1 || s < 2) return DVD_E_ARG;
    if (d < 1 || d > DVD_EVAL_MAX_D || n_sub > DVD_EVAL_MAX_SUBSETS || s > 65536) return DVD_E_SHAPE;
    if (ldx < d || ldy < d || ((uintptr_t)ws & 7) || ((uintptr_t)out & 7) || ((uintptr_t)terms & 7)) return DVD_E_ARG;
    if (((uintptr_t)X & 3) || ((uintptr_t)Y & 3)) return DVD_E_ARG;
    if (!strided_ok(n, ldx) || !strided_ok(m, ldy)) return DVD_E_SHAPE;
    const long long entries = (long long)n_sub * s;
    for (long long i = 0; i < entries; ++i)
        if (ix_host[i] < 0 || ix_host[i] >= n || iy_host[i] < 0 || iy_host[i] >= m) return DVD_E_ARG;
    const int nb = kid_nb(s);
    const unsigned per = (unsigned)(nb * (nb + 1) + nb * nb);
    eval_kid_kernel<<<dim3(per, (unsigned)n_sub), EV_THREADS, 0, S_>>>(X, ldx, Y, ldy, d, ix_dev, iy_dev, s, nb, ws);
    eval_kid_reduce_kernel<<<(unsigned)n_sub, EV_THREADS, 0, S_>>>(ws, nb, s, out, terms);
    return launch_status();
}
