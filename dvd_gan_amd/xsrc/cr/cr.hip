// dvdx_cr_pair (include/dvdx_cr.h), built into libdvdx_cr.so: the pair loss of balanced consistency regularization on a
// discriminator's logits -- weight * mean((aug - clean)^2), both gradients and a row of statistics.  A few thousand floats at the
// most: one workgroup, latency-sized like the adversarial-loss launch beside it in the step.  Every pair has one owner and the sum
// has one order (thread stride, xor butterfly, waves in order through LDS): no atomics, two launches give the same bits.
#include "../../csrc/common.h"
#include "../../../include/dvdx_cr.h"

// the header states every expression rounding by rounding
#pragma clang fp contract(off)

namespace {

constexpr int kThreads = DVDX_CR_THREADS;
constexpr int kWaves = kThreads / 64;

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(kThreads) void cr_pair_kernel(const float* aug, const float* clean, int n, float weight, float scale,
                                                          float* loss, float* d_aug, float* d_clean, float* stats) {
    __shared__ double sh_sum[kWaves];
    __shared__ float sh_max[kWaves];
    __shared__ int sh_cnt[kWaves];
    double sum = 0.0;
    float big = 0.f;
    int cnt = 0;
    for (int i = threadIdx.x; i < n; i += kThreads) {
        const float gap = aug[i] - clean[i];
        const float g = scale * gap;
        d_aug[i] = g;
        d_clean[i] = __uint_as_float(__float_as_uint(g) ^ 0x80000000u);
        sum += (double)gap * (double)gap;
        big = fmaxf(big, fabsf(gap));
        cnt += gap != 0.f ? 1 : 0;
    }
    sum = wave_sum_d(sum);
    big = wave_max(big);
    cnt = wave_sum_i(cnt);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        sh_sum[w] = sum;
        sh_max[w] = big;
        sh_cnt[w] = cnt;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    sum = sh_sum[0];
    big = sh_max[0];
    cnt = sh_cnt[0];
#pragma unroll
    for (int k = 1; k < kWaves; ++k) {
        sum += sh_sum[k];
        big = fmaxf(big, sh_max[k]);
        cnt += sh_cnt[k];
    }
    const float penalty = (float)(((double)weight * sum) / (double)n);
    *loss = penalty;
    if (stats) {
        stats[DVDX_CR_STAT_PENALTY] = penalty;
        stats[DVDX_CR_STAT_MSQ] = (float)(sum / (double)n);
        stats[DVDX_CR_STAT_MAXABS] = big;
        stats[DVDX_CR_STAT_NONZERO] = (float)cnt;
        stats[DVDX_CR_STAT_N] = (float)n;
    }
}

}  // namespace

#define S_ ((hipStream_t)stream)

extern "C" int dvdx_cr_abi_version(void) { return DVDX_CR_ABI_VERSION; }

extern "C" const char* dvdx_cr_strerror(int code) {
    switch (code) {
    case DVD_OK: return "ok";
    case DVD_E_ARG: return "null logits, loss or gradient pointer, fewer than one pair, or a weight that is negative or not finite";
    case DVD_E_SHAPE: return "unsupported shape: more than 2^20 pairs";
    case DVD_E_LAUNCH: return "kernel launch failed";
    default: return "unknown error";
    }
}

extern "C" int dvdx_cr_pair(const float* aug, const float* clean, long long n, float weight, float* loss, float* d_aug,
                            float* d_clean, float* stats, void* stream) {
    if (!aug || !clean || !loss || !d_aug || !d_clean || n < 1) return DVD_E_ARG;
    if (!(weight >= 0.f && weight <= 3.402823466e+38f)) return DVD_E_ARG;
    if (n > DVDX_CR_MAX_N) return DVD_E_SHAPE;
    const float scale = (2.f * weight) / (float)n;
    cr_pair_kernel<<<1, kThreads, 0, S_>>>(aug, clean, (int)n, weight, scale, loss, d_aug, d_clean, stats);
    return launch_status();
}
