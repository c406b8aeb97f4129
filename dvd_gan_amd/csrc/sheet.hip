// Sample sheets (sheets.make_sheets, Trainer.save_samples): fp32 frames -> 8-bit RGB sheets in PNG scanline form, one launch.  The
// write-side mirror of clipstore.hip: denormalise, quantise, tile with borders and go from planar to interleaved in one read of the
// floats and one write of the bytes.
//
// Geometry = torchvision's make_grid(nrow, padding, pad_value) (utils.py), except that a single tile keeps its border:
//   xmaps = min(nrow, total_slots), ymaps = ceil(total_slots / xmaps), Hs = ymaps (H + padding) + padding, Ws likewise with xmaps,
//   slot k at ((k / xmaps) (H + padding) + padding, (k % xmaps) (W + padding) + padding).
// Value = helpers.denorm then torchvision's save_image, every operation rounded on its own in fp32 (contraction is off for this
// file): x = clamp((v + 1) / 2, 0, 1), q = clamp(x * 255 + 0.5, 0, 255), byte = q truncated.  fmaxf / fminf drop a NaN operand, so
// NaN -> 0, -inf -> 0, +inf -> 255.
//
// One workgroup serves kChunk bytes of one destination row, counted from the 4-byte boundary at or below the row's first byte
// (rows are tight: 3 Ws or 1 + 3 Ws bytes, so rows and sheets start at any address).  Pass 1 walks the chunk's pixels plane by plane,
// x fastest (coalesced reads), and leaves every byte with a "write me" flag in LDS; pass 2 stores one dword per thread where all
// four flags are set and single bytes elsewhere (row ends, and the edges of this launch's tiles when it does not fill).  Every
// destination byte has one owner: no atomics, nothing shared between workgroups.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kChunk = 1024;                    // bytes of a row per workgroup: one dword per thread
constexpr int kPix = kChunk / 3 + 2;            // pixels that can touch a chunk: 343 (3 * 343 = 1029 >= 1024 + 2 at either phase)

__host__ __device__ inline unsigned quant8(float x) {        // x taken as a [0, 1] value
    x = fminf(fmaxf(x, 0.f), 1.f);
    float q = x * 255.f;
    q = q + 0.5f;
    q = fminf(fmaxf(q, 0.f), 255.f);
    return (unsigned)(int)q;
}

struct Geom {
    int xmaps, ymaps, Hs, Ws;
    long long row_bytes;
};

// DVD_OK and the geometry, or the refusal
inline int sheet_geom(int total_slots, int H, int W, int nrow, int padding, int row_prefix, Geom* g) {
    if (total_slots < 1 || nrow < 1 || padding < 0 || padding > DVD_SHEET_MAX_PADDING || (row_prefix != 0 && row_prefix != 1))
        return DVD_E_ARG;
    if (H < 1 || W < 1 || H > DVD_SHEET_MAX_TILE || W > DVD_SHEET_MAX_TILE) return DVD_E_SHAPE;
    const long long xmaps = nrow < total_slots ? nrow : total_slots;
    const long long ymaps = ((long long)total_slots + xmaps - 1) / xmaps;
    const long long Hs = ymaps * (H + padding) + padding, Ws = xmaps * (W + padding) + padding;
    if (Hs > DVD_SHEET_MAX_SIDE || Ws > DVD_SHEET_MAX_SIDE) return DVD_E_SHAPE;
    g->xmaps = (int)xmaps; g->ymaps = (int)ymaps; g->Hs = (int)Hs; g->Ws = (int)Ws;
    g->row_bytes = row_prefix + 3 * Ws;
    return DVD_OK;
}

struct SheetK {
    const float* src; unsigned char* dst;
    long long ss, st, sc;
    int n_tiles, H, W, first_slot, xmaps, Hs, Ws, padding, prefix, row_bytes, fill, is_signed;
    unsigned pad_byte;
};

__global__ void __launch_bounds__(256) sample_sheet_kernel(SheetK p) {
    __shared__ uint32_t val[kChunk / 4], flag[kChunk / 4];
    unsigned char* val8 = reinterpret_cast<unsigned char*>(val);
    unsigned char* flag8 = reinterpret_cast<unsigned char*>(flag);
    const long long r = blockIdx.x;                          // row of the destination, over all sheets
    const long long s = r / p.Hs;
    const int y = (int)(r - s * p.Hs);
    unsigned char* row = p.dst + r * p.row_bytes;
    const int mis = (int)(reinterpret_cast<uintptr_t>(row) & 3);
    const int i0 = (int)blockIdx.y * kChunk - mis;           // first byte of the chunk, counted from the row's first byte
    if (i0 >= p.row_bytes) return;                           // (workgroup-uniform)

    // the row of tiles this destination row cuts through, if any
    const int chh = p.H + p.padding, cww = p.W + p.padding;
    const int ty = y - p.padding;
    const int gy = ty >= 0 ? ty / chh : -1, yy = ty >= 0 ? ty - gy * chh : 0;
    const bool in_tiles = ty >= 0 && yy < p.H;
    const float* srow = p.src + s * p.ss + (long long)yy * p.W;

    // pass 1: byte i = prefix + 3 * px + c, every i of the chunk exactly once (px = -1, c = 2 is the prefix byte)
    const int d = i0 - p.prefix;
    const int p_lo = d >= 0 ? d / 3 : -((2 - d) / 3);        // floor(d / 3)
    for (int idx = threadIdx.x; idx < 3 * kPix; idx += 256) {
        const int c = idx / kPix, px = p_lo + (idx - c * kPix);
        const int i = p.prefix + 3 * px + c, j = i - i0;
        if (j < 0 || j >= kChunk) continue;
        unsigned v = 0, f = 0;
        if (px >= 0 && px < p.Ws) {
            v = p.pad_byte; f = p.fill;
            const int tx = px - p.padding;
            if (in_tiles && tx >= 0) {
                const int gx = tx / cww, xx = tx - gx * cww;
                const int k = gy * p.xmaps + gx - p.first_slot;
                if (xx < p.W && k >= 0 && k < p.n_tiles) {
                    const float x = srow[k * p.st + c * p.sc + xx];
                    v = quant8(p.is_signed ? (x + 1.f) * 0.5f : x);
                    f = 1;
                }
            }
        } else if (i == 0 && p.prefix) {
            f = p.fill;                                      // PNG filter type 0
        }
        val8[j] = (unsigned char)v;
        flag8[j] = (unsigned char)f;
    }
    __syncthreads();
    // pass 2: thread t owns the aligned dword t of the chunk
    const int j = threadIdx.x * 4;
    const uint32_t f = flag[threadIdx.x], v = val[threadIdx.x];
    unsigned char* out = row + i0 + j;
    if (f == 0x01010101u) {
        *reinterpret_cast<uint32_t*>(out) = v;
    } else if (f) {
#pragma unroll
        for (int b = 0; b < 4; ++b)
            if ((f >> (8 * b)) & 1) out[b] = (unsigned char)(v >> (8 * b));
    }
}

inline bool mul_add_ok(long long n, long long stride, long long* acc) {     // *acc += n * stride without leaving 63 bits
    long long t;
    return !__builtin_mul_overflow(n, stride, &t) && !__builtin_add_overflow(*acc, t, acc);
}

}  // namespace

extern "C" int dvd_sample_sheet_shape(int total_slots, int H, int W, int nrow, int padding, int row_prefix, int* Hs, int* Ws,
                                      long long* sheet_bytes) {
    if (!Hs || !Ws || !sheet_bytes) return DVD_E_ARG;
    Geom g;
    const int rc = sheet_geom(total_slots, H, W, nrow, padding, row_prefix, &g);
    if (rc != DVD_OK) return rc;
    *Hs = g.Hs; *Ws = g.Ws; *sheet_bytes = g.Hs * g.row_bytes;
    return DVD_OK;
}

extern "C" int dvd_sample_sheet(const float* src, long long s_sheet, long long s_tile, long long s_chan, long long n_sheets,
                                int n_tiles, int H, int W, int first_slot, int total_slots, int nrow, int padding, float pad_value,
                                int row_prefix, int flags, unsigned char* dst, void* stream) {
    if (!src || !dst || n_sheets < 1 || n_tiles < 1 || first_slot < 0 || (flags & ~(DVD_SHEET_FILL | DVD_SHEET_SIGNED)))
        return DVD_E_ARG;
    Geom g;
    const int rc = sheet_geom(total_slots, H, W, nrow, padding, row_prefix, &g);
    if (rc != DVD_OK) return rc;
    if ((long long)first_slot + n_tiles > total_slots) return DVD_E_ARG;
    if (s_sheet < 0 || s_tile < 0 || s_chan < (long long)H * W) return DVD_E_ARG;       // channel planes would overlap
    // the last float read and the last byte written, in 63 bits (the float's BYTE offset too)
    long long last = (long long)H * W - 1;
    if (!mul_add_ok(n_sheets - 1, s_sheet, &last) || !mul_add_ok(n_tiles - 1, s_tile, &last) || !mul_add_ok(2, s_chan, &last) ||
        last > 0x7fffffffffffffffLL / 4)
        return DVD_E_SHAPE;
    long long bytes = 0;
    if (!mul_add_ok(n_sheets, g.Hs * g.row_bytes, &bytes) || n_sheets > 0x7fffffffLL / g.Hs) return DVD_E_SHAPE;
    SheetK p{src, dst, s_sheet, s_tile, s_chan, n_tiles, H, W, first_slot, g.xmaps, g.Hs, g.Ws, padding, row_prefix,
             (int)g.row_bytes, (flags & DVD_SHEET_FILL) ? 1 : 0, (flags & DVD_SHEET_SIGNED) ? 1 : 0, quant8(pad_value)};
    // chunks per row: the row's bytes plus up to 3 in front of them (rows start at any address)
    const dim3 grid((unsigned)(n_sheets * g.Hs), cdiv(g.row_bytes + 3, kChunk));
    sample_sheet_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(p);
    return launch_status();
}
