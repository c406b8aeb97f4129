// Weight images of the convolution kernels: the forward / backward-data operand packs of an fp32 master weight
// (dvd_pack_conv_weight) and the fragment-major image of a bf16 pack (dvd_conv_fragment_major; layout: conv_gb.hip).  Each has a
// batched form -- n items in one launch, whole blocks per item -- that runs the same __device__ item function.
#include "conv_common.h"
#include <vector>

namespace {

struct PackK {
    const float* w; const float* sigma; char* wf; char* wd;
    int Cout, Cin, ntaps, Cip, co_off, co_tot_f, co_tot_d, kt, kh, kw, ci_off, ci_tot;
};
// element i = (co, ci_pad, tap) of the forward pack; writes both packs
template <typename T>
__device__ __forceinline__ void pack_weight_item(const PackK& p, long long i) {
    if (i >= (long long)p.Cout * p.Cip * p.ntaps) return;
    const int tap = (int)(i % p.ntaps);
    const long long r = i / p.ntaps;
    const int ci = (int)(r % p.Cip), co = (int)(r / p.Cip);
    float v = 0.f;
    if (ci < p.Cin) {
        v = p.w[((size_t)co * p.ci_tot + p.ci_off + ci) * p.ntaps + tap];
        if (p.sigma) v = v / *p.sigma;
    }
    if (p.wf) stf(reinterpret_cast<T*>(p.wf) + ((size_t)tap * p.co_tot_f + p.co_off + co) * p.Cip + ci, v);
    if (p.wd) {
        const int ftap = p.ntaps - 1 - tap;     // flipping every axis == reversing the flat tap index
        stf(reinterpret_cast<T*>(p.wd) + ((size_t)ftap * p.Cip + ci) * p.co_tot_d + p.co_off + co, v);
    }
}

// standard forward pack [tap][Cout][C] (bf16) -> fragment-major [tap][chunk][nb32][kk][lane][8] (zeros in every padded position)
struct FragK { const bf16_t* w; bf16_t* wq; int ntaps, Cout, C, kchunks, nb32; };
__device__ __forceinline__ void fragment_major_item(const FragK& p, long long i) {      // i: 16-byte unit of the image
    if (i >= (long long)p.ntaps * p.kchunks * p.nb32 * 2 * 64) return;
    const int l = (int)(i & 63);
    long long r = i >> 6;
    const int kk = (int)(r & 1); r >>= 1;
    const int nb = (int)(r % p.nb32); r /= p.nb32;
    const int cc = (int)(r % p.kchunks);
    const int tap = (int)(r / p.kchunks);
    const int co = nb * 32 + (l & 31), ci = cc * 32 + (kk * 2 + (l >> 5)) * 8;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (co < p.Cout && ci < p.C) v = *reinterpret_cast<const u32x4*>(p.w + ((size_t)tap * p.Cout + co) * p.C + ci);   // C % 8 == 0
    *reinterpret_cast<u32x4*>(p.wq + i * 8) = v;
}

// n items in one launch: block b serves item j with first[j] <= b < first[j + 1] (whole blocks per item)
template <class Item, int N> struct BatchK { Item it[N]; int first[N + 1]; int n; };
template <class Item, int N>
__device__ __forceinline__ long long batch_item(const BatchK<Item, N>& b, int& j) {     // -> index inside item j
    j = 0;
    while (j + 1 < b.n && (int)blockIdx.x >= b.first[j + 1]) ++j;
    return (long long)((int)blockIdx.x - b.first[j]) * blockDim.x + threadIdx.x;
}
using PackBatchK = BatchK<PackK, 24>;
using FragBatchK = BatchK<FragK, 32>;
template <typename T> __global__ void pack_weight_kernel(PackK p) { pack_weight_item<T>(p, (long long)blockIdx.x * blockDim.x + threadIdx.x); }
template <typename T> __global__ void pack_weight_batched_kernel(PackBatchK b) { int j; const long long i = batch_item(b, j); pack_weight_item<T>(b.it[j], i); }
__global__ void fragment_major_kernel(FragK p) { fragment_major_item(p, (long long)blockIdx.x * blockDim.x + threadIdx.x); }
__global__ void fragment_major_batched_kernel(FragBatchK b) { int j; const long long i = batch_item(b, j); fragment_major_item(b.it[j], i); }

// validation + kernel arguments of one item, shared by the single and the batched entry point
int pack_item(const dvd_pack_item& t, PackK& p) {
    if (!t.w || (!t.wf && !t.wd) || t.Cout <= 0 || t.Cin <= 0 || t.ntaps != t.kt * t.kh * t.kw) return DVD_E_ARG;
    const int ci_off = t.ci_tot <= 0 ? 0 : t.ci_off, ci_tot = t.ci_tot <= 0 ? t.Cin : t.ci_tot;
    if (ci_off < 0 || ci_off + t.Cin > ci_tot) return DVD_E_ARG;
    if ((t.Cip & 7) || t.Cip < t.Cin || (t.wd && (t.co_tot_d & 7))) return DVD_E_SHAPE;
    p = PackK{t.w, t.sigma, (char*)t.wf, (char*)t.wd, t.Cout, t.Cin, t.ntaps, t.Cip, t.co_off, t.co_tot_f, t.co_tot_d, t.kt, t.kh, t.kw, ci_off, ci_tot};
    return DVD_OK;
}
int frag_item(const dvd_frag_item& t, FragK& p) {
    if (!t.w || !t.wq || t.ntaps <= 0 || t.Cout <= 0 || t.C <= 0) return DVD_E_ARG;
    if (t.C & 7) return DVD_E_SHAPE;
    p = FragK{(const bf16_t*)t.w, (bf16_t*)t.wq, t.ntaps, t.Cout, t.C, (t.C + 31) / 32, (t.Cout + 127) / 128 * 4};
    return DVD_OK;
}
long long pack_blocks(const PackK& p) { return cdiv((long long)p.Cout * p.Cip * p.ntaps, 256); }
long long frag_blocks(const FragK& p) { return cdiv((long long)p.ntaps * p.kchunks * p.nb32 * 128, 256); }

// The next batch of the validated items its[0 .. n): fills b, returns its blocks.
template <class Item, int N>
long long fill_batch(BatchK<Item, N>& b, const Item* its, int n, long long (*blocks_of)(const Item&)) {
    long long blocks = 0;
    b.n = n < N ? n : N;
    for (int j = 0; j < b.n; ++j) { b.it[j] = its[j]; b.first[j] = (int)blocks; blocks += blocks_of(its[j]); }
    b.first[b.n] = (int)blocks;
    return blocks;
}

}  // namespace

extern "C" int dvd_pack_conv_weight(int dtype, const float* w, const float* sigma, int Cout, int Cin, int ntaps,
                                    int Cip, int co_off, int co_tot_f, int co_tot_d, void* wf, void* wd,
                                    int kt, int kh, int kw, int ci_off, int ci_tot, void* stream) {
    PackK p;
    if (const int rc = pack_item(dvd_pack_item{w, sigma, wf, wd, Cout, Cin, ntaps, Cip, co_off, co_tot_f, co_tot_d, kt, kh, kw, ci_off, ci_tot}, p))
        return rc;
    if (dtype == DVD_BF16) pack_weight_kernel<bf16_t><<<(unsigned)pack_blocks(p), 256, 0, (hipStream_t)stream>>>(p);
    else if (dtype == DVD_F32) pack_weight_kernel<float><<<(unsigned)pack_blocks(p), 256, 0, (hipStream_t)stream>>>(p);
    else return DVD_E_ARG;
    return launch_status();
}

extern "C" int dvd_pack_conv_weight_batched(int dtype, const dvd_pack_item* items, int n, void* stream) {
    if (!items || n <= 0) return DVD_E_ARG;
    if (dtype != DVD_BF16 && dtype != DVD_F32) return DVD_E_ARG;
    std::vector<PackK> its(n);
    for (int i = 0; i < n; ++i)             // validate everything before the first launch
        if (const int rc = pack_item(items[i], its[i])) return rc;
    for (int i0 = 0; i0 < n; i0 += 24) {
        PackBatchK b;
        const long long blocks = fill_batch(b, &its[i0], n - i0, pack_blocks);
        if (blocks >= (1ll << 31)) return DVD_E_SHAPE;
        if (dtype == DVD_BF16) pack_weight_batched_kernel<bf16_t><<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(b);
        else pack_weight_batched_kernel<float><<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(b);
    }
    return launch_status();
}

// Fragment-major image of a forward (or backward-data) pack for conv_halo_gb_kernel; see the comment at the top of conv_gb.hip.
extern "C" long long dvd_conv_fragment_major_bytes(int ntaps, int Cout, int C) {
    if (ntaps <= 0 || Cout <= 0 || C <= 0) return 0;
    return (long long)ntaps * ((C + 31) / 32) * ((Cout + 127) / 128 * 4) * 2048;       // kchunks x nb32 records of 2 KiB per tap
}
extern "C" int dvd_conv_fragment_major(int dtype, const void* w, void* wq, int ntaps, int Cout, int C, void* stream) {
    FragK p;
    const int rc = frag_item(dvd_frag_item{w, wq, ntaps, Cout, C}, p);
    if (rc == DVD_E_ARG) return rc;
    if (dtype != DVD_BF16 || rc) return DVD_E_SHAPE;
    fragment_major_kernel<<<(unsigned)frag_blocks(p), 256, 0, (hipStream_t)stream>>>(p);
    return launch_status();
}
extern "C" int dvd_conv_fragment_major_batched(int dtype, const dvd_frag_item* items, int n, void* stream) {
    if (!items || n <= 0) return DVD_E_ARG;
    if (dtype != DVD_BF16) return DVD_E_SHAPE;
    std::vector<FragK> its(n);
    for (int i = 0; i < n; ++i)
        if (const int rc = frag_item(items[i], its[i])) return rc;
    for (int i0 = 0; i0 < n; i0 += 32) {
        FragBatchK b;
        const long long blocks = fill_batch(b, &its[i0], n - i0, frag_blocks);
        if (blocks >= (1ll << 31)) return DVD_E_SHAPE;
        fragment_major_batched_kernel<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(b);
    }
    return launch_status();
}
