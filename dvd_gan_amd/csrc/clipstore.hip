// Device-resident clip store (data.ClipStore.gather): crop + Pillow's 8-bit bilinear resize + flip + normalise + layout, one launch
// per batch, from a uint8 blob of decoded frames [frame][h][w][3] to the fp32 [B][3][T][S][S] batch the trainer takes.
//
// The resize is Pillow's ImagingResample for 8-bit images (Resample.c: ImagingResampleHorizontal_8bpc, then ..Vertical_8bpc):
// integer arithmetic on 22-bit coefficients, the horizontal result ROUNDED TO uint8 before the vertical pass.  The coefficient
// tables come from the host (data.resize_coeffs, fp64 like precompute_coeffs / normalize_coeffs_8bpc), so the kernel only adds
// and shifts and its bytes equal `img.crop(box).resize((S, S), Image.BILINEAR)`.
//
// One workgroup serves a band of R output rows of one frame: pass 1 leaves the horizontally resized source rows the band needs as
// uint8 [row][c][x] in LDS, pass 2 walks them vertically and stores fp32 with x fastest (coalesced, also when mirrored).  In pass 1
// neighbouring lanes read source bytes 3 * scale apart (the same 64-byte lines; the L1 serves the overlap of neighbouring taps).
// A frame's result depends on that frame and its tables alone: no atomics, nothing shared between workgroups.
#include "common.h"

namespace {

constexpr int kLdsBytes = 64 * 1024;

// Pillow's ksize for in -> out samples (bilinear: filter support 1): 2 * ceil(max(in / out, 1)) + 1.  fp64 on both sides of the
// launch (IEEE division and ceil: the same value as the Python that laid the table out).
__host__ __device__ inline int resize_ksize(int in, int out) {
    const double scale = (double)in / (double)out;
    return 2 * (int)ceil(scale < 1.0 ? 1.0 : scale) + 1;
}

// Source rows a band of R output rows can need: its first and last centres are (R - 1) * scale apart, either end adds the filter
// support and one row of truncation: (R - 1) * scale + 2 * support + 1 <= floor((R - 1) * scale) + ksize + 1; one more for safety.
inline long long band_src_rows(int in, int out, int R) {
    return (long long)floor((double)(R - 1) * ((double)in / (double)out)) + resize_ksize(in, out) + 2;
}
inline int lds_rows(int S) { return kLdsBytes / (3 * S); }
// Largest R <= S whose source rows fit the LDS; 0 = not even one output row does.
inline int band_rows(int in, int S) {
    const long long cap = lds_rows(S);
    for (int R = S; R >= 1; --R)
        if (band_src_rows(in, S, R) <= cap) return R;
    return 0;
}

struct ClipK {
    const unsigned char* blob; const long long* clips; const int* tab; float* dst; const float* ms;
    long long B; int T, S, R, cap; float norm;
};

__device__ __forceinline__ int clip8(int acc) {
    const int v = acc >> 22;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

__global__ void __launch_bounds__(256) clip_gather_kernel(ClipK p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char hres[];      // [rows][3][S]
    const long long f = blockIdx.x, b = f / p.T;
    const int t = (int)(f - b * p.T), S = p.S, S3 = 3 * S;
    const long long* d = p.clips + b * DVD_CLIP_COLS;
    const int w = (int)d[DVD_CLIP_W];
    const int x0 = (int)d[DVD_CLIP_X0], y0 = (int)d[DVD_CLIP_Y0], cw = (int)d[DVD_CLIP_CW], ch = (int)d[DVD_CLIP_CH];
    const long long frame = p.clips[p.B * DVD_CLIP_COLS + f];
    const unsigned char* src = p.blob + d[DVD_CLIP_OFF] + frame * ((long long)d[DVD_CLIP_H] * w * 3) + ((long long)y0 * w + x0) * 3;
    const int kx = resize_ksize(cw, S), ky = resize_ksize(ch, S);
    const int* xb = p.tab + d[DVD_CLIP_XTAB];       // [S][2] first sample, count; then [S][kx] coefficients
    const int* xk = xb + 2 * S;
    const int* yb = p.tab + d[DVD_CLIP_YTAB];
    const int* yk = yb + 2 * S;
    const int y_lo = blockIdx.y * p.R;
    if (y_lo >= S) return;                          // (workgroup-uniform)
    const int nby = min(p.R, S - y_lo);
    // source rows of the band: the tables' first samples never decrease with the output index
    const int r0 = min(max(yb[2 * y_lo], 0), ch - 1);
    const int r1 = yb[2 * (y_lo + nby - 1)] + yb[2 * (y_lo + nby - 1) + 1];
    const int nrows = max(0, min(min(r1, ch) - r0, p.cap));

    // pass 1: horizontal, source rows r0 .. r0 + nrows - 1 of the crop -> uint8 in LDS.  (The clamps are no-ops on tables made by
    // data.resize_coeffs; they keep every read inside the crop whatever the table holds.)
    for (int i = threadIdx.x; i < nrows * S3; i += 256) {
        const int row = i / S3, rem = i - row * S3, c = rem / S, x = rem - c * S;
        const int xmin = min(max(xb[2 * x], 0), cw - 1);
        const int n = min(min(xb[2 * x + 1], kx), cw - xmin);
        const unsigned char* s = src + ((long long)(r0 + row) * w + xmin) * 3 + c;
        const int* k = xk + (long long)x * kx;
        int acc = 1 << 21;
        for (int j = 0; j < n; ++j) acc += (int)s[3 * j] * k[j];
        hres[i] = (unsigned char)clip8(acc);
    }
    __syncthreads();
    // pass 2: vertical from LDS, flip, normalise, store [b][c][t][y][x]
    const int flip = d[DVD_CLIP_FLIP] != 0;
    for (int i = threadIdx.x; i < 3 * nby * S; i += 256) {
        const int x = i % S, q = i / S, yy = q % nby, c = q / nby, y = y_lo + yy;
        const int ymin = min(max(yb[2 * y] - r0, 0), max(nrows - 1, 0));
        const int n = min(min(yb[2 * y + 1], ky), nrows - ymin);
        const unsigned char* s = hres + (ymin * 3 + c) * S + x;
        const int* k = yk + (long long)y * ky;
        int acc = 1 << 21;
        for (int j = 0; j < n; ++j) acc += (int)s[j * S3] * k[j];
        const float v = (float)clip8(acc);
        const int xo = flip ? S - 1 - x : x;
        p.dst[(((b * 3 + c) * p.T + t) * S + y) * (long long)S + xo] = (v / p.norm - p.ms[c]) / p.ms[3 + c];
    }
}

}  // namespace

extern "C" int dvd_clip_gather_band_rows(int crop_h, int S) {
    if (crop_h <= 0 || crop_h > DVD_CLIP_MAX_SIDE || S <= 0 || S > DVD_CLIP_MAX_OUT) return 0;
    return band_rows(crop_h, S);
}

extern "C" int dvd_clip_gather(const unsigned char* blob, long long blob_bytes, const long long* clips_host,
                               const long long* clips_dev, const int* tables, long long table_ints, float* dst, long long B, int T,
                               int S, float norm_value, const float* mean_std, void* stream) {
    if (!blob || !clips_host || !clips_dev || !tables || !dst || !mean_std || blob_bytes <= 0 || table_ints <= 0 || B <= 0 ||
        T <= 0 || S <= 0 || !(norm_value != 0.f))
        return DVD_E_ARG;
    if (S > DVD_CLIP_MAX_OUT || B > (long long)0x7fffffff / T) return DVD_E_SHAPE;
    int R = S;
    long long rows = 1;
    for (long long b = 0; b < B; ++b) {
        const long long* d = clips_host + b * DVD_CLIP_COLS;
        const long long off = d[DVD_CLIP_OFF], h = d[DVD_CLIP_H], w = d[DVD_CLIP_W], nf = d[DVD_CLIP_FRAMES];
        const long long x0 = d[DVD_CLIP_X0], y0 = d[DVD_CLIP_Y0], cw = d[DVD_CLIP_CW], ch = d[DVD_CLIP_CH];
        if (h <= 0 || w <= 0 || nf <= 0 || off < 0 || cw <= 0 || ch <= 0 || x0 < 0 || y0 < 0) return DVD_E_ARG;
        if (h > DVD_CLIP_MAX_SIDE || w > DVD_CLIP_MAX_SIDE) return DVD_E_SHAPE;
        if (x0 > w - cw || y0 > h - ch) return DVD_E_ARG;                           // the box leaves the frame
        if (nf > (blob_bytes - off) / (h * w * 3)) return DVD_E_ARG;                  // the video leaves the blob
        const int kx = resize_ksize((int)cw, S), ky = resize_ksize((int)ch, S);
        const long long xt = d[DVD_CLIP_XTAB], yt = d[DVD_CLIP_YTAB];
        if (xt < 0 || yt < 0 || xt > table_ints - (long long)S * (2 + kx) || yt > table_ints - (long long)S * (2 + ky)) return DVD_E_ARG;
        for (int t = 0; t < T; ++t) {
            const long long fr = clips_host[B * DVD_CLIP_COLS + b * T + t];
            if (fr < 0 || fr >= nf) return DVD_E_ARG;
        }
        const int r = band_rows((int)ch, S);
        if (r == 0) return DVD_E_SHAPE;
        if (r < R) R = r;
    }
    for (long long b = 0; b < B; ++b) {             // LDS rows of the launch: the largest need of any clip at the common R
        const long long need = band_src_rows((int)clips_host[b * DVD_CLIP_COLS + DVD_CLIP_CH], S, R);
        if (need > rows) rows = need;
    }
    ClipK p{blob, clips_dev, tables, dst, mean_std, B, T, S, R, (int)rows, norm_value};
    const size_t lds = ((size_t)rows * 3 * S + 15) & ~(size_t)15;
    const dim3 grid((unsigned)(B * T), cdiv(S, R));
    clip_gather_kernel<<<grid, 256, lds, (hipStream_t)stream>>>(p);
    return launch_status();
}
