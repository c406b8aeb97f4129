// dvdx_zcr_dist / dvdx_zcr_dist_grad (include/dvdx_zcr.h), built into libdvdx_zcr.so: the clip distance of latent consistency
// regularization -- term = -weight * mean((a - b)^2) over the generator's clips of the base and of the perturbed latents -- and its
// gradient.  Two streams over fp32 [pairs, n], tens of millions of floats at the benchmark shape: a capped grid of 256-thread
// workgroups (8 per compute unit), each thread with four 16-byte loads in flight (128 KiB per compute unit), 64-bit indices, a
// 4-byte path where a pointer is not 16-byte aligned.  Every partial sum has one owner and every sum one order: no atomics, two
// launches give the same bits.
#include "../../csrc/common.h"
#include "../../../include/dvdx_zcr.h"

// the header states every expression rounding by rounding
#pragma clang fp contract(off)

namespace {

constexpr int kThreads = DVDX_ZCR_THREADS;
constexpr int kWaves = kThreads / 64;

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}

__device__ __forceinline__ void add_gap(float x, float y, double& sum, float& big) {
    const float gap = x - y;
    sum += (double)gap * (double)gap;
    big = fmaxf(big, fabsf(gap));
}

__device__ __forceinline__ void add_gap4(const f32x4& x, const f32x4& y, double& sum, float& big) {
    add_gap(x[0], y[0], sum, big);
    add_gap(x[1], y[1], sum, big);
    add_gap(x[2], y[2], sum, big);
    add_gap(x[3], y[3], sum, big);
}

// work unit u = row u / chunks, chunk u % chunks: the sum of squared gaps of the chunk -> ws[2u], its largest |gap| -> ws[2u + 1]
__global__ __launch_bounds__(kThreads) void zcr_dist_kernel(const float* __restrict__ a, const float* __restrict__ b, long long n,
                                                           long long chunks, long long chunk_len, long long units,
                                                           double* __restrict__ ws) {
    __shared__ double sh_sum[kWaves];
    __shared__ float sh_max[kWaves];
    const int t = threadIdx.x;
    for (long long u = blockIdx.x; u < units; u += gridDim.x) {
        const long long p = u / chunks, start = (u - p * chunks) * chunk_len;
        long long len = n - start;
        len = len < 0 ? 0 : (len < chunk_len ? len : chunk_len);
        const float* ra = a + (p * n + start);
        const float* rb = b + (p * n + start);
        double sum = 0.0;
        float big = 0.f;
        if ((((uintptr_t)ra | (uintptr_t)rb) & 15) == 0) {
            const long long full = len >> 2;
            const f32x4* va = reinterpret_cast<const f32x4*>(ra);
            const f32x4* vb = reinterpret_cast<const f32x4*>(rb);
            long long g = t;
            for (; g + kThreads < full; g += 2 * kThreads) {
                const f32x4 x0 = va[g], y0 = vb[g], x1 = va[g + kThreads], y1 = vb[g + kThreads];
                add_gap4(x0, y0, sum, big);
                add_gap4(x1, y1, sum, big);
            }
            if (g < full) {
                const f32x4 x0 = va[g], y0 = vb[g];
                add_gap4(x0, y0, sum, big);
                g += kThreads;
            }
            if (g == full)                                  // the owner of the last, shorter group
                for (long long i = full << 2; i < len; ++i) add_gap(ra[i], rb[i], sum, big);
        } else {
            long long i = t;
            for (; i + 3 * kThreads < len; i += 4 * kThreads) {
                const float x0 = ra[i], y0 = rb[i], x1 = ra[i + kThreads], y1 = rb[i + kThreads];
                const float x2 = ra[i + 2 * kThreads], y2 = rb[i + 2 * kThreads], x3 = ra[i + 3 * kThreads], y3 = rb[i + 3 * kThreads];
                add_gap(x0, y0, sum, big);
                add_gap(x1, y1, sum, big);
                add_gap(x2, y2, sum, big);
                add_gap(x3, y3, sum, big);
            }
            for (; i < len; i += kThreads) add_gap(ra[i], rb[i], sum, big);
        }
        sum = wave_sum_d(sum);
        big = wave_max(big);
        if ((t & 63) == 0) {
            sh_sum[t >> 6] = sum;
            sh_max[t >> 6] = big;
        }
        __syncthreads();
        if (t == 0) {
            sum = sh_sum[0];
            big = sh_max[0];
#pragma unroll
            for (int k = 1; k < kWaves; ++k) {
                sum += sh_sum[k];
                big = fmaxf(big, sh_max[k]);
            }
            ws[2 * u] = sum;
            ws[2 * u + 1] = (double)big;
        }
        __syncthreads();                                    // the LDS words are the next unit's
    }
}

// one workgroup: the rows' sums in chunk order, the total in row order per thread, lanes and waves as in the header
__global__ __launch_bounds__(kThreads) void zcr_finish_kernel(const double* __restrict__ ws, long long pairs, long long n,
                                                             long long chunks, float weight, float* __restrict__ term,
                                                             float* __restrict__ stats) {
    __shared__ double sh_sum[kWaves];
    __shared__ float sh_max[kWaves], sh_lo[kWaves], sh_hi[kWaves];
    const int t = threadIdx.x;
    double total = 0.0;
    float big = 0.f, lo = __builtin_inff(), hi = 0.f;
    for (long long p = t; p < pairs; p += kThreads) {
        const double* row = ws + 2 * p * chunks;
        double s = 0.0;
        for (long long c = 0; c < chunks; ++c) {
            s += row[2 * c];
            big = fmaxf(big, (float)row[2 * c + 1]);
        }
        const float mean = (float)(s / (double)n);
        lo = fminf(lo, mean);
        hi = fmaxf(hi, mean);
        total += s;
    }
    total = wave_sum_d(total);
    big = wave_max(big);
    lo = wave_min(lo);
    hi = wave_max(hi);
    if ((t & 63) == 0) {
        sh_sum[t >> 6] = total;
        sh_max[t >> 6] = big;
        sh_lo[t >> 6] = lo;
        sh_hi[t >> 6] = hi;
    }
    __syncthreads();
    if (t != 0) return;
    total = sh_sum[0];
    big = sh_max[0];
    lo = sh_lo[0];
    hi = sh_hi[0];
#pragma unroll
    for (int k = 1; k < kWaves; ++k) {
        total += sh_sum[k];
        big = fmaxf(big, sh_max[k]);
        lo = fminf(lo, sh_lo[k]);
        hi = fmaxf(hi, sh_hi[k]);
    }
    const double count = (double)pairs * (double)n;
    const float value = (float)(-(((double)weight * total) / count));
    *term = value;
    if (stats) {
        stats[DVDX_ZCR_STAT_TERM] = value;
        stats[DVDX_ZCR_STAT_MSQ] = (float)(total / count);
        stats[DVDX_ZCR_STAT_MIN_PAIR] = lo;
        stats[DVDX_ZCR_STAT_MAX_PAIR] = hi;
        stats[DVDX_ZCR_STAT_MAXABS] = big;
        stats[DVDX_ZCR_STAT_PAIRS] = (float)pairs;
    }
}

__device__ __forceinline__ float flip(float v) { return __uint_as_float(__float_as_uint(v) ^ 0x80000000u); }

__device__ __forceinline__ void grad4(const f32x4& x, const f32x4& y, float g, f32x4& dx, f32x4& dy) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float gap = x[k] - y[k];
        dy[k] = g * gap;
        dx[k] = flip(dy[k]);
    }
}

// total elements of either half, n4 of them as whole 16-byte vectors (0: a pointer is only 4-byte aligned, all of it element by
// element)
__global__ __launch_bounds__(kThreads) void zcr_grad_kernel(const float* __restrict__ a, const float* __restrict__ b, long long total,
                                                           long long n4, float scale, const float* __restrict__ upstream,
                                                           float* __restrict__ da, float* __restrict__ db) {
    const float g = upstream[0] * scale;
    const long long stride = (long long)gridDim.x * kThreads;
    long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (n4) {
        const f32x4* va = reinterpret_cast<const f32x4*>(a);
        const f32x4* vb = reinterpret_cast<const f32x4*>(b);
        f32x4* vda = reinterpret_cast<f32x4*>(da);
        f32x4* vdb = reinterpret_cast<f32x4*>(db);
        long long v = i;
        for (; v + stride < n4; v += 2 * stride) {
            const f32x4 x0 = va[v], y0 = vb[v], x1 = va[v + stride], y1 = vb[v + stride];
            f32x4 dx, dy;
            grad4(x0, y0, g, dx, dy);
            vda[v] = dx;
            vdb[v] = dy;
            grad4(x1, y1, g, dx, dy);
            vda[v + stride] = dx;
            vdb[v + stride] = dy;
        }
        if (v < n4) {
            f32x4 dx, dy;
            grad4(va[v], vb[v], g, dx, dy);
            vda[v] = dx;
            vdb[v] = dy;
        }
    }
    for (long long e = 4 * n4 + i; e < total; e += stride) {
        const float gap = a[e] - b[e];
        const float d = g * gap;
        db[e] = d;
        da[e] = flip(d);
    }
}

bool weight_ok(float w) { return w >= 0.f && w <= 3.402823466e+38f; }      // false for NaN as well

long long chunks_of(long long pairs, long long n) {
    const long long by_len = (n + DVDX_ZCR_MIN_CHUNK - 1) / DVDX_ZCR_MIN_CHUNK;
    long long by_grid = DVDX_ZCR_MAX_BLOCKS / pairs;
    if (by_grid < 1) by_grid = 1;
    return by_len < by_grid ? by_len : by_grid;
}

}  // namespace

#define S_ ((hipStream_t)stream)

extern "C" int dvdx_zcr_abi_version(void) { return DVDX_ZCR_ABI_VERSION; }

extern "C" const char* dvdx_zcr_strerror(int code) {
    switch (code) {
    case DVD_OK: return "ok";
    case DVD_E_ARG:
        return "null clip, workspace, term, upstream or gradient pointer, fewer than one pair or element, a workspace smaller than "
               "dvdx_zcr_ws_doubles, or a weight that is negative or not finite";
    case DVD_E_SHAPE: return "unsupported shape: more than 65536 pairs or more than 2^40 elements a row";
    case DVD_E_LAUNCH: return "kernel launch failed";
    default: return "unknown error";
    }
}

extern "C" long long dvdx_zcr_chunks(long long pairs, long long n) {
    if (pairs < 1 || n < 1 || pairs > DVDX_ZCR_MAX_PAIRS || n > DVDX_ZCR_MAX_N) return 0;
    return chunks_of(pairs, n);
}

extern "C" long long dvdx_zcr_ws_doubles(long long pairs, long long n) { return 2 * pairs * dvdx_zcr_chunks(pairs, n); }

extern "C" int dvdx_zcr_dist(const float* a, const float* b, long long pairs, long long n, float weight, double* ws,
                             long long ws_doubles, float* term, float* stats, void* stream) {
    if (!a || !b || !ws || !term || pairs < 1 || n < 1 || !weight_ok(weight)) return DVD_E_ARG;
    if (pairs > DVDX_ZCR_MAX_PAIRS || n > DVDX_ZCR_MAX_N) return DVD_E_SHAPE;
    const long long chunks = chunks_of(pairs, n), units = pairs * chunks;
    if (ws_doubles < 2 * units) return DVD_E_ARG;
    const long long chunk_len = 4 * (((n + chunks - 1) / chunks + 3) / 4);
    const unsigned grid = units < DVDX_ZCR_MAX_BLOCKS ? (unsigned)units : DVDX_ZCR_MAX_BLOCKS;
    zcr_dist_kernel<<<grid, kThreads, 0, S_>>>(a, b, n, chunks, chunk_len, units, ws);
    zcr_finish_kernel<<<1, kThreads, 0, S_>>>(ws, pairs, n, chunks, weight, term, stats);
    return launch_status();
}

extern "C" int dvdx_zcr_dist_grad(const float* a, const float* b, long long pairs, long long n, float weight, const float* upstream,
                                  float* da, float* db, void* stream) {
    if (!a || !b || !upstream || !da || !db || pairs < 1 || n < 1 || !weight_ok(weight)) return DVD_E_ARG;
    if (pairs > DVDX_ZCR_MAX_PAIRS || n > DVDX_ZCR_MAX_N) return DVD_E_SHAPE;
    const long long total = pairs * n;
    const float scale = (float)((2.0 * (double)weight) / ((double)pairs * (double)n));
    const long long n4 = flat_n4(total, (uintptr_t)a | (uintptr_t)b | (uintptr_t)da | (uintptr_t)db);
    zcr_grad_kernel<<<flat_grid(total, n4), kThreads, 0, S_>>>(a, b, total, n4, scale, upstream, da, db);
    return launch_status();
}
