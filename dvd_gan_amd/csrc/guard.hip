// Gradient-norm clipping and non-finite step skipping (optim.FlatAdam(clip_norm, skip_nonfinite, norm_log)): one memory-bound
// read of the flat fp32 gradient that leaves its norm, the clipping coefficient and the skip decision in device memory, and an
// Adam launch that obeys them.  Nothing comes back to the host; include/dvdgan_hip.h states the contract.
#include "common.h"

namespace {

constexpr int CH = DVD_GUARD_CH;                 // elements of one workgroup of grad_sumsq_kernel
constexpr int SUMSQ_THREADS = 256;
constexpr int SUMSQ_ITERS = CH / (SUMSQ_THREADS * 4);
constexpr int FIN_THREADS = 1024;
static_assert(CH % (SUMSQ_THREADS * 4) == 0, "a chunk is whole rounds of one 16-byte vector per thread");

// inf / NaN by the exponent field; such an element is counted and enters the sum as an exact zero
__device__ __forceinline__ void sumsq_take(float x, double& acc, unsigned& bad) {
    const bool nf = (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u;
    const double d = (double)(nf ? 0.f : x);
    acc += d * d;                                // the product is exact in fp64: one rounding, fused or not
    bad += nf ? 1u : 0u;
}

__device__ __forceinline__ unsigned wave_sum_u(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ unsigned long long wave_sum_ull(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Element i of chunk w = i / CH, j = i % CH: thread (j / 4) % 256, round (j / 4) / 256, accumulator j % 4.  `vec` (g 16-byte
// aligned) only chooses the load instruction.  A thread adds its rounds in order into four accumulators, (a0 + a1) + (a2 + a3),
// xor shuffles within the wave, the four waves in order.
__global__ __launch_bounds__(SUMSQ_THREADS) void grad_sumsq_kernel(const float* g, long long n, int vec, double* partial,
                                                                  unsigned* bad) {
    __shared__ double sh_s[SUMSQ_THREADS / 64];
    __shared__ unsigned sh_b[SUMSQ_THREADS / 64];
    const long long base = (long long)blockIdx.x * CH;
    const float* gc = g + base;
    const long long left = n - base;             // > 0: the grid is ceil(n / CH)
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    unsigned nb = 0;
    if (vec && left >= CH) {
#pragma unroll 8
        for (int k = 0; k < SUMSQ_ITERS; ++k) {
            const f32x4 x = reinterpret_cast<const f32x4*>(gc)[k * SUMSQ_THREADS + threadIdx.x];
            sumsq_take(x[0], a0, nb);
            sumsq_take(x[1], a1, nb);
            sumsq_take(x[2], a2, nb);
            sumsq_take(x[3], a3, nb);
        }
    } else {
        for (int k = 0; k < SUMSQ_ITERS; ++k) {
            const long long j = (long long)(k * SUMSQ_THREADS + threadIdx.x) * 4;
            if (j >= left) break;
            if (vec && j + 4 <= left) {
                const f32x4 x = *reinterpret_cast<const f32x4*>(gc + j);
                sumsq_take(x[0], a0, nb);
                sumsq_take(x[1], a1, nb);
                sumsq_take(x[2], a2, nb);
                sumsq_take(x[3], a3, nb);
            } else {
                sumsq_take(gc[j], a0, nb);
                if (j + 1 < left) sumsq_take(gc[j + 1], a1, nb);
                if (j + 2 < left) sumsq_take(gc[j + 2], a2, nb);
                if (j + 3 < left) sumsq_take(gc[j + 3], a3, nb);
            }
        }
    }
    const double s = wave_sum_d((a0 + a1) + (a2 + a3));
    nb = wave_sum_u(nb);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sh_s[w] = s; sh_b[w] = nb; }
    __syncthreads();
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = ((sh_s[0] + sh_s[1]) + sh_s[2]) + sh_s[3];
        bad[blockIdx.x] = ((sh_b[0] + sh_b[1]) + sh_b[2]) + sh_b[3];
    }
}

// One workgroup: thread t adds partials t, t + 1024, ... in order, xor shuffles, the sixteen waves in order; thread 0 decides.
__global__ __launch_bounds__(FIN_THREADS) void grad_guard_finalize_kernel(const double* partial, const unsigned* bad,
                                                                          long long nwg, float max_norm, int skip_nonfinite,
                                                                          long long step, double* total, double* state,
                                                                          double* ring, int ring_rows) {
    __shared__ double sh_s[FIN_THREADS / 64];
    __shared__ unsigned long long sh_b[FIN_THREADS / 64];
    double s = 0.0;
    unsigned long long b = 0;
    for (long long i = threadIdx.x; i < nwg; i += FIN_THREADS) {
        s += partial[i];
        b += bad[i];
    }
    s = wave_sum_d(s);
    b = wave_sum_ull(b);
    if ((threadIdx.x & 63) == 0) { sh_s[threadIdx.x >> 6] = s; sh_b[threadIdx.x >> 6] = b; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double S = sh_s[0];
    unsigned long long B = sh_b[0];
    for (int w = 1; w < FIN_THREADS / 64; ++w) { S += sh_s[w]; B += sh_b[w]; }
    *total = S;
    const double norm = sqrt(S);
    const double coef = fmin(1.0, (double)max_norm / (norm + 1e-6));
    const bool skip = skip_nonfinite && B > 0;
    const float coef32 = skip ? 0.f : (float)coef;
    state[0] = norm;
    state[1] = (double)coef32;
    state[2] = (double)B;
    state[3] = skip ? 1.0 : 0.0;
    state[4] += 1.0;
    if (skip) state[5] += 1.0;
    if (!skip && coef32 < 1.f) state[6] += 1.0;
    state[7] = 0.0;
    if (ring) {
        double* row = ring + ((step - 1) % ring_rows) * 4;
        row[0] = (double)step;
        row[1] = norm;
        row[2] = (double)coef32;
        row[3] = (double)B;
    }
}

// the clipped gradient element: a product of its own, whatever it is inlined into (adam_elem's first use of it is a subtraction)
__device__ __forceinline__ float guard_scale(float g, float c) {
#pragma clang fp contract(off)
    return g * c;
}

// adam_ema_kernel's stream (misc.hip) on g * coef32, the average optional, nothing at all on a skipped step
template <bool EMA>
__global__ __launch_bounds__(256) void adam_guard_kernel(float* p, const float* g, float* m, float* v, float* ema, long long n,
                                                         long long n4, float lr_over_bc1, float b1, float b2, float eps,
                                                         float bc2_sqrt, float d, float omd, const double* state) {
    if (state[3] != 0.0) return;
    const float c = (float)state[1];             // stored from a float: exact
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    for (long long i = t; i < n4; i += stride) {
        f32x4 pv = reinterpret_cast<const f32x4*>(p)[i];
        const f32x4 gv = reinterpret_cast<const f32x4*>(g)[i];
        f32x4 mv = reinterpret_cast<const f32x4*>(m)[i], vv = reinterpret_cast<const f32x4*>(v)[i];
        f32x4 ev;
        if constexpr (EMA) ev = reinterpret_cast<const f32x4*>(ema)[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float mk = mv[k], vk = vv[k];
            const float pk = adam_elem(pv[k], guard_scale(gv[k], c), mk, vk, lr_over_bc1, b1, b2, eps, bc2_sqrt);
            mv[k] = mk;
            vv[k] = vk;
            pv[k] = pk;
            if constexpr (EMA) ev[k] = ema_elem(ev[k], pk, d, omd);
        }
        reinterpret_cast<f32x4*>(m)[i] = mv;
        reinterpret_cast<f32x4*>(v)[i] = vv;
        reinterpret_cast<f32x4*>(p)[i] = pv;
        if constexpr (EMA) reinterpret_cast<f32x4*>(ema)[i] = ev;
    }
    for (long long i = n4 * 4 + t; i < n; i += stride) {
        float mi = m[i], vi = v[i];
        const float pi = adam_elem(p[i], guard_scale(g[i], c), mi, vi, lr_over_bc1, b1, b2, eps, bc2_sqrt);
        m[i] = mi;
        v[i] = vi;
        p[i] = pi;
        if constexpr (EMA) ema[i] = ema_elem(ema[i], pi, d, omd);
    }
}

inline long long guard_nwg(long long n) { return (n + CH - 1) / CH; }

}  // namespace

#define S_ ((hipStream_t)stream)

extern "C" long long dvd_grad_guard_ws_bytes(long long n) {
    if (n <= 0) return 0;
    const long long nwg = guard_nwg(n);
    return (nwg + 1) * 8 + (nwg * 4 + 7) / 8 * 8;       // double partial[nwg] | double S | unsigned bad[nwg]
}

extern "C" int dvd_grad_guard(const float* g, long long n, float max_norm, int skip_nonfinite, long long step, void* ws,
                              double* state, double* ring, int ring_rows, void* stream) {
    if (!g || !ws || !state || n <= 0 || step <= 0 || !(max_norm > 0.f) || ring_rows < 0 || (!ring && ring_rows > 0))
        return DVD_E_ARG;
    if (((uintptr_t)ws | (uintptr_t)state | (uintptr_t)ring) & 7) return DVD_E_ARG;
    const long long nwg = guard_nwg(n);
    if (nwg > 0x7fffffffLL) return DVD_E_SHAPE;
    double* partial = (double*)ws;
    double* total = partial + nwg;
    unsigned* bad = (unsigned*)(total + 1);
    grad_sumsq_kernel<<<(unsigned)nwg, SUMSQ_THREADS, 0, S_>>>(g, n, ((uintptr_t)g & 15) == 0, partial, bad);
    grad_guard_finalize_kernel<<<1, FIN_THREADS, 0, S_>>>(partial, bad, nwg, max_norm, skip_nonfinite, step, total, state,
                                                          ring_rows > 0 ? ring : nullptr, ring_rows);
    return launch_status();
}

extern "C" int dvd_adam_guard_step(float* p, const float* g, float* m, float* v, float* ema, long long n, float lr,
                                   float beta1, float beta2, float eps, int step, float decay, const double* state,
                                   void* stream) {
    if (!p || !g || !m || !v || !state || n <= 0 || step <= 0 || (ema && !decay_ok(decay))) return DVD_E_ARG;
    const double bc1 = 1.0 - pow((double)beta1, (double)step);
    const double bc2 = 1.0 - pow((double)beta2, (double)step);
    const long long n4 = flat_n4(n, (uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema);
    const float lr_over_bc1 = (float)((double)lr / bc1), bc2_sqrt = (float)sqrt(bc2);
    if (ema)
        adam_guard_kernel<true><<<flat_grid(n, n4), 256, 0, S_>>>(p, g, m, v, ema, n, n4, lr_over_bc1, beta1, beta2, eps, bc2_sqrt,
                                                                  decay, (float)(1.0 - (double)decay), state);
    else
        adam_guard_kernel<false><<<flat_grid(n, n4), 256, 0, S_>>>(p, g, m, v, nullptr, n, n4, lr_over_bc1, beta1, beta2, eps,
                                                                   bc2_sqrt, 0.f, 1.f, state);
    return launch_status();
}
