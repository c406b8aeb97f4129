// Halo-staged forward / backward-data convolutions whose weight operand is read straight from L2 in fragment-major order
// (bf16): conv_halo_gb_kernel (frames >= 16 pixels wide), conv_halo_gbs_kernel (whole 4 x 4 / 8 x 8 frames per tile), and the
// GROUPED launches of both (several independent convolutions in one grid: the layer wavefront of the ConvGRU stacks, gru.hip).
//
// Same GEMM as conv_halo_kernel (conv_igemm.hip): the input footprint of an output patch sits in LDS for all taps of a 32-channel
// chunk (LDS-DMA, zero fill by out-of-range offsets, double-buffered over chunks).  The weights exist a second time in
// fragment-major order (dvd_conv_fragment_major): record (tap, chunk, 32-column block nb, k-half pair kk) is 1 KiB whose 16 bytes
// l = (kh2 = l >> 5, col = l & 31) are the 8 channels chunk*32 + (2 kk + kh2)*8 .. +7 of output column nb*32 + col.  The tiles
// multiply on v_mfma_f32_16x16x32_bf16 (the chip holds a higher clock on it than on 32x32x16: profiles/mfma16_numbers.md): one
// instruction takes a whole 32-channel chunk of 16 pixels x 16 columns; lane l holds k group kg = l >> 4 (channels 8 kg .. 8 kg + 7)
// of pixel row / column l & 15, so a B fragment is four 256-byte runs of two records -- one buffer_load_dwordx4 per lane, four per
// wave and K step, prefetched one K step ahead -- and an A fragment one ds_read_b128 of 16 footprint rows (FragRows, conv_common.h).
// Nothing is handed between waves inside a chunk: no per-tap LDS-DMA, wait or barrier; the waves of a workgroup meet once per chunk
// (footprint hand-over).
//
// Round 5: the filter size KS (3 or 5) is a template parameter.  The tap loop of a chunk is `for (row) { unrolled KS taps }`:
// the LDS offset of tap ix is an immediate, the weight record advances by a running scalar add (records are [tap][chunk], so the
// taps of a chunk are a constant stride apart), the footprint of the next chunk goes out in the first step of row 0 only, and the
// per-step tap counters / record multiplications / branchy iterator of the runtime-tap form (about 40 scalar instructions and
// three branches per 16 MFMAs) are gone.  Lane-validity of the footprint rows is folded into the offsets (an invalid row carries
// an offset beyond the descriptor's range) instead of living in lane-mask register pairs across the loop.
#include "conv_common.h"

namespace {

#ifndef DVD_GB_EPI_DEEP
#define DVD_GB_EPI_DEEP 0
#endif

// Footprint offsets: the descriptor of a tile's input starts at the first frame it can touch and is clamped to 1 GiB, a footprint row
// outside the frame (or past the group count) carries kRowOOB, a time step outside the clip adds kStepOOB: every combination lands
// at or beyond 1 GiB (no wrap-around below it), where the hardware returns zeros.  Valid offsets stay below 3 frames (< 1 GiB).
constexpr unsigned kRowOOB = 0x80000000u, kStepOOB = 0x40000000u, kRangeCap = 0x3fffffffu;

template <int TM, int WN, int WMV, bool UP2> struct HaloGbCfg {
    using Rows = std::conditional_t<UP2, RowsUp2, RowsHalo>;      // fragment h = 1: 4 footprint rows to the right of fragment 0
    static_assert(Rows::pix(1, 0) == (UP2 ? 8 : 4), "fragment 1 = fragment 0 moved 4 footprint columns");
    static constexpr int PITCH = HaloGeo<UP2>::PITCH;
    static constexpr int NWAVE = WMV * WN;
    static constexpr int PH = WMV * TM * 2;                             // patch: PH lines x 16 columns
    static constexpr int HG = UP2 ? ((PH / 2 + 3) * PITCH + 15) / 16 : ((PH + 4) * PITCH + 15) / 16;
    static constexpr int HBYTES = HG * 1024;
    static constexpr int EPI = NWAVE * 32 * 64 * 4;
    static constexpr int LDSB = 2 * HBYTES + 1024 > EPI ? 2 * HBYTES + 1024 : EPI;
};

// One K step = one tap of one 32-channel chunk on v_mfma_f32_16x16x32_bf16: 2 * TM units (sub-tile tm = u >> 1, fragment h = u & 1)
// of four MFMAs, one per 16-column block of the wave's 64 columns; the A fragment of unit u + 2 is requested before the MFMAs of
// unit u, the B fragments of the NEXT step (record nrec) right behind the first MFMA group -- behind the point where the compiler
// waits for this step's own fragments -- and, when `foot` is given, the next chunk's footprint DMAs with them.  (The request is
// unconditional: behind a branch hipcc assumes the smaller outstanding count and drains the prefetch in the middle of a step.)
template <int TM, bool RELU, class Rows, class LdA, class Next>
__device__ __forceinline__ void gb_step(Acc16<Rows> (&acc)[TM], const bf16x8 (&b)[4], LdA ldA, Next next) {
    constexpr int NU = 2 * TM;
#ifndef DVD_GB_ADEPTH
#define DVD_GB_ADEPTH 2
#endif
    constexpr int AD = (RELU && TM == 4) ? 1 : DVD_GB_ADEPTH;     // A fragments requested this many units ahead (ReLU on 256 rows: no registers for two)
    bf16x8 a[NU];
#pragma unroll
    for (int u = 0; u < AD && u < NU; ++u) a[u] = ldA(u);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        if (u + AD < NU) a[u + AD] = ldA(u + AD);
        const int tm = u >> 1, h = u & 1;
        if constexpr (RELU) a[u] = __builtin_bit_cast(bf16x8, relu16_bf16(__builtin_bit_cast(u32x4, a[u])));
#pragma unroll
        for (int j = 0; j < 4; ++j)
            acc[tm].q[h][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[u], b[j], acc[tm].q[h][j], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        if (u == 0) {
#ifndef DVD_EXP_NODMA
            next();
#endif
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

// waves: WMV (M) x WN (N), wave tile (TM*32 pixels) x 64 columns: 4 x 2 x 2 = the 256 x 128 tile, 2 x 2 x 2 = 128 x 128 (launches with
// few rows), 2 x 1 x 4 = 256 x 64 (thin outputs).  `ltile`: index of the output tile among the convolution's tiles (tickets / slabs
// of the in-launch split-K combine).
template <int TM, int WN, int WMV, bool RELU, bool UP2, int KS>
__device__ __forceinline__ void conv_halo_gb_tile(const ConvK& p, char* const smem, const int mt, const int nt, const int z, const int ltile) {
    using T = bf16_t;
    using G = HaloGeo<UP2>;
    using Cfg = HaloGbCfg<TM, WN, WMV, UP2>;
    using Rows = typename Cfg::Rows;
    constexpr int NWAVE = Cfg::NWAVE;
    constexpr int PITCH = G::PITCH;
    constexpr int BNt = WN * 64;
    constexpr int PH = Cfg::PH, HG = Cfg::HG, HBYTES = Cfg::HBYTES;
    constexpr int NH = (HG + NWAVE - 1) / NWAVE;
    constexpr int ntap2 = KS * KS;
    constexpr int pad = KS >> 1, cpad = (pad + 1) >> 1;
    constexpr int HWa = UP2 ? ((15 + pad) >> 1) + cpad + 1 : 16 + 2 * pad;
    constexpr int HHa = UP2 ? ((PH - 1 + pad) >> 1) + cpad + 1 : PH + 2 * pad;
    char* const hbuf0 = &smem[0];
    char* const dump = &smem[2 * HBYTES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN, kg = lane >> 4;
    const int n0 = nt * BNt;
    const int pw = p.W >> 4, ppf = pw * (p.H / PH);
    // (uniform, but the divisions run on the vector unit: back into scalar registers, or they occupy vector registers to the epilogue)
    const int ft = __builtin_amdgcn_readfirstlane(mt / ppf), pidx = mt - ft * ppf;
    const int y0 = __builtin_amdgcn_readfirstlane((pidx / pw) * PH), x0 = __builtin_amdgcn_readfirstlane((pidx % pw) * 16);
    const int nouter = p.kchunks * p.kt;
    const int per = (nouter + p.nsplit - 1) / p.nsplit;
    const int oc_begin = z * per, oc_end = min(nouter, oc_begin + per);
    constexpr unsigned esz = 2;
    const int iy_lo = UP2 ? (y0 >> 1) - cpad : y0 - pad, ix_lo = UP2 ? (x0 >> 1) - cpad : x0 - pad;

    const int wu = __builtin_amdgcn_readfirstlane(wave);
    const int lrow = lane >> 2;
    const unsigned ldb = (unsigned)p.ldi * esz;
    const int tt = p.kt > 1 ? ft % p.T : 0;
    const int base_frame = max(0, ft - (p.kt >> 1));
    const size_t fbytes = (size_t)p.Hin * p.Win * ldb;
    const size_t base_b = (size_t)base_frame * fbytes;
    const size_t left_b = p.in_bytes - base_b;
    const __amdgpu_buffer_rsrc_t rin = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(p.in + base_b), 0, left_b > kRangeCap ? kRangeCap : (unsigned)left_b, 0x00020000);
    // fragment-major weights: [tap][chunk][nb32][kk][lane][16 B]; nb32 = 32-column blocks, padded to whole 128-column tiles
    const int nb32 = p.nb32;
    const __amdgpu_buffer_rsrc_t rwq = __builtin_amdgcn_make_buffer_rsrc(
        (void*)p.wq, 0, (unsigned)((size_t)p.kt * ntap2 * p.kchunks * nb32 * 2048), 0x00020000);
    // footprint row of DMA group i for this lane: its logical 16-byte slot is XOR-swizzled into the offset (see HaloGeo)
    auto hrow = [&](int i, int lrow, int& hy, int& hx) __attribute__((always_inline)) {
        const int h = (i * NWAVE + wu) * 16 + lrow;
        hy = h / PITCH; hx = h - hy * PITCH;
    };
    auto hoff_of = [&](int i, int ln) __attribute__((always_inline)) -> unsigned {
        const int g = i * NWAVE + wu;
        int hy, hx;
        hrow(i, ln >> 2, hy, hx);
        const int yin = iy_lo + hy, xin = ix_lo + hx;
        const int hq = (ln & 3) ^ G::sw(hy, hx);
        const bool ok = g < HG && hy < HHa && hx < HWa && (unsigned)yin < (unsigned)p.Hin && (unsigned)xin < (unsigned)p.Win;
        return ok ? (unsigned)(yin * p.Win + xin) * ldb + hq * 16 : kRowOOB;
    };
    // The 256-row tile with ReLU on its fragments has no registers left for the NH offsets across the K loop (they went to scratch):
    // it forms them again for every footprint, once per chunk, from an opaque copy of the lane index.
    constexpr bool REOFF = RELU && TM == 4;
    unsigned hoff[NH];
#pragma unroll
    for (int i = 0; i < NH; ++i) hoff[i] = REOFF ? 0u : hoff_of(i, lane);
    const bool ragged = (p.C & 31) != 0;                                 // last chunk holds fewer than 32 channels (uniform)
    auto dmaH = [&](int hb, int cc_, int it_) __attribute__((always_inline)) {
        const int dt_ = it_ - (p.kt >> 1);
        const bool ok_ = (unsigned)(tt + dt_) < (unsigned)p.T || p.kt == 1;
        const unsigned ud_ = ok_ ? (unsigned)(ft + dt_ - base_frame) * (unsigned)fbytes + cc_ * 64 : kStepOOB;
        const bool part_ = ragged && cc_ == p.kchunks - 1;
        int ln_ = lane;
        if (part_ || REOFF) asm volatile("" : "+v"(ln_));                // (opaque: hoisted out of the K loop the slots below cost NH registers)
#pragma unroll
        for (int i = 0; i < NH; ++i) {
            const int g = i * NWAVE + wu;
            char* dst_ = g < HG ? hbuf0 + hb * HBYTES + g * 1024 : dump;
            unsigned off_ = (REOFF ? hoff_of(i, ln_) : hoff[i]) + ud_;
            if (part_) {                                                 // channels past C: zeros (rare: thin / odd-width inputs)
                int hy, hx;
                hrow(i, ln_ >> 2, hy, hx);
                const int hq = (ln_ & 3) ^ G::sw(hy, hx);
                off_ = cc_ * 32 + hq * 8 < p.C ? off_ : kRowOOB;
            }
            dma16(rin, dst_, off_);
        }
    };
    // B fragments: the 16 columns x 32 channels of column block j (0 .. 3) of this wave's 64 columns sit in the record's block
    // nb = j >> 1, k-half pair kg >> 1, at its lanes (kg & 1) * 32 + (j & 1) * 16 + column.  voffset = this wave's column half + that
    // slot without j (per lane), soffset = record of (tap, chunk, N tile) (uniform) + j's part
    const unsigned bvoff = (unsigned)(wn * 2 * 2048 + (kg >> 1) * 1024 + ((kg & 1) * 32 + (lane & 15)) * 16);
    const unsigned bnt = (unsigned)(nt * (BNt / 32)) * 2048u;
    const unsigned brec = (unsigned)nb32 * 2048u;                       // bytes per (tap, chunk)
    const unsigned tapstep = (unsigned)p.kchunks * brec;                // record stride between two taps of one chunk
    auto ldBq = [&](bf16x8 (&b)[4], unsigned rec) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            b[j] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rwq, bvoff, rec + (unsigned)((j >> 1) * 2048 + (j & 1) * 256), 0));
    };
    // record of tap 0 of outer index (chunk cc, time tap it)
    auto rec0 = [&](int cc_, int it_) __attribute__((always_inline)) -> unsigned {
        return ((unsigned)(it_ * ntap2) * p.kchunks + cc_) * brec + bnt;
    };

    Acc16<Rows> acc[TM];
#pragma unroll
    for (int a = 0; a < TM; ++a) acc_zero(acc[a]);
    // this lane's A row: pixel Rows::pix(h, lane & 15) of each sub-tile (two lines x 16 px) and its channels 8 kg .. 8 kg + 7
    const int pix0 = Rows::pix(0, lane & 15);
    const int px = pix0 & 15, py0 = wm * (TM * 2) + (pix0 >> 4);
    constexpr int TMSTRIDE = (UP2 ? 1 : 2) * PITCH * 64;
#ifdef DVD_EXP_NOMAIN
    const int nouter_z = 0;
#else
    const int nouter_z = oc_end - oc_begin;
#endif
    if (nouter_z > 0) {
        int m_cc = oc_begin / p.kt, m_it = oc_begin - m_cc * p.kt;      // (chunk, dt) being multiplied
        int h_cc = m_cc, h_it = m_it;                                   // ... of the next footprint to fetch
        bf16x8 bq0[4], bq1[4];
        unsigned rec = rec0(m_cc, m_it);
        dmaH(0, h_cc, h_it);
        if (++h_it == p.kt) { h_it = 0; ++h_cc; }
        ldBq(bq0, rec);
        __builtin_amdgcn_s_waitcnt(0x0070 | (0xf << 8));                // vmcnt(0): footprint 0 (this wave's part) landed
        __builtin_amdgcn_s_barrier();
        // The K loop runs over filter ROWS (KS unrolled taps each), two rows per iteration: KS is odd, so a row ends on the other
        // B register set than it started on -- alternating the sets by a branch per row instead makes hipcc keep a second copy of
        // the accumulators at the join (408 spilled registers in the 256 x 128 tile).  Chunk boundaries (footprint hand-over, next
        // chunk's record) are uniform side blocks of the row that ends / starts a chunk.
        int hb = 0, iy = 0, left = nouter_z;                            // footprint buffer, filter row, chunks left incl. the current
        auto row = [&](bf16x8 (&b0)[4], bf16x8 (&b1)[4]) __attribute__((always_inline)) {
            const bool first = iy == 0, last = iy == KS - 1, more = left > 1;
            const int hy = UP2 ? ((py0 + iy - pad) >> 1) + cpad : py0 + iy;
            const char* const Arow = hbuf0 + hb * HBYTES + hy * (PITCH * 64);
#pragma unroll
            for (int ix = 0; ix < KS; ++ix) {
                const int hx = UP2 ? ((px + ix - pad) >> 1) + cpad : px + ix;
                const int swz[2] = {G::sw(hy, hx), G::sw(hy, hx + 4)};
                const char* const Ah = Arow + hx * 64;
                auto ldA = [&](int u) __attribute__((always_inline)) -> bf16x8 {
                    const int tm = u >> 1, h = u & 1;
                    const int sl = (UP2 && (tm & 1)) ? (kg ^ 2) : kg;        // one footprint line down: sw + 2
                    return *reinterpret_cast<const bf16x8*>(Ah + tm * TMSTRIDE + h * 256 + ((sl ^ swz[h]) << 4));
                };
                unsigned nrec = rec + tapstep;
                if (ix == KS - 1 && last) {                             // next chunk's first record; none left: re-read this one
                    int n_cc = m_cc, n_it = m_it + 1;
                    if (n_it == p.kt) { n_it = 0; ++n_cc; }
                    nrec = more ? rec0(n_cc, n_it) : rec;
                    m_cc = n_cc; m_it = n_it;
                }
                auto next = [&]() __attribute__((always_inline)) {
                    ldBq((ix & 1) ? b0 : b1, nrec);
                    if (ix == 0 && first && more) { dmaH(hb ^ 1, h_cc, h_it); if (++h_it == p.kt) { h_it = 0; ++h_cc; } }
                };
                gb_step<TM, RELU>(acc, (ix & 1) ? b1 : b0, ldA, next);
                rec = nrec;
            }
            ++iy;
            if (last) {
                // chunk boundary: every wave has finished reading footprint hb (it is overwritten one chunk from now) and has seen
                // its own part of footprint hb ^ 1 land (the in-order drain in front of the steps since): one barrier per chunk
                iy = 0; hb ^= 1; --left;
                if (more) {
#ifndef DVD_EXP_NOWAIT
                    __builtin_amdgcn_s_waitcnt(0xc07f);                 // lgkmcnt(0): this wave's fragment reads are done
#endif
#ifndef DVD_EXP_NOBAR
                    __builtin_amdgcn_s_barrier();
#endif
                }
            }
        };
        const int nrows = nouter_z * KS;
        int r = 0;
#pragma unroll 1
        for (; r + 1 < nrows; r += 2) { row(bq0, bq1); row(bq1, bq0); }
        if (r < nrows) row(bq0, bq1);
    }
    __syncthreads();

    // (the epilogue's lane values come from an opaque copy of the thread index: carried across the K loop they cost it registers)
    int te = tid;
    asm volatile("" : "+v"(te));
    const int elane = te & 63, ewave = te >> 6, ewm = ewave / WN, ewn = ewave % WN;
    float* ep = reinterpret_cast<float*>(&smem[0]) + ewave * (32 * 64);
    const int ecol = (elane & 7) * 8, erow = elane >> 3;
    const long long frame_row0 = (long long)ft * (p.H * p.W);
    conv_epilogue<T, TM, DVD_GB_EPI_DEEP>(p, acc, ep, elane, n0 + ewn * 64 + ecol, z, ltile, frame_row0, [&](int tm, int j) __attribute__((always_inline)) {
        const int pi = ewm * (TM * 32) + tm * 32 + j * 8 + erow;
        return (y0 + (pi >> 4)) * p.W + x0 + (pi & 15);
    });
}

// XCD-aware order: workgroup b runs on XCD b % 8 (observed dispatch order, used for speed only); each XCD gets a contiguous run
__device__ __forceinline__ int xcd_order(int bid, int nwg) {
    const int xcd = bid & 7, qd = nwg >> 3, rr = nwg & 7;
    return (xcd < rr ? xcd * (qd + 1) : rr * (qd + 1) + (xcd - rr) * qd) + (bid >> 3);
}
// tile index -> (M tile, N tile): M-major, or N-major (a run of workgroups shares the weight tile) for weight-heavy launches
struct TileMN { int mt, nt; };
__device__ __forceinline__ TileMN tile_of(int nmajor, int tilesN, int t, int ntiles) {
    const int d = nmajor ? ntiles / tilesN : tilesN;        // divisor: tiles per N tile / per M tile
    const int q = t / d, r = t - q * d;
    TileMN o;
    o.mt = nmajor ? r : q; o.nt = nmajor ? q : r;
    return o;
}

// (waves per SIMD the register allocation must leave room for: three of the 128-row tiles, two of the 256-row tiles)
template <int TM, int WN, int WMV, bool RELU, bool UP2, int KS>
__global__ __launch_bounds__(256, TM == 2 ? 3 : 2) void conv_halo_gb_kernel(ConvK p) {
    __shared__ __attribute__((aligned(16))) char smem[HaloGbCfg<TM, WN, WMV, UP2>::LDSB];
    const int bid = xcd_order(blockIdx.x, gridDim.x);
    const TileMN t = tile_of(p.nmajor, p.tilesN, bid, gridDim.x);
    conv_halo_gb_tile<TM, WN, WMV, RELU, UP2, KS>(p, smem, t.mt, t.nt, blockIdx.z, (int)blockIdx.x);
}

// ---------------------------------------------------------------------------- the same for frames of 8 x 8 and 4 x 4 pixels
// The recurrent convolutions of the first two generator stages (Generator.py:39,43: ConvGRUs on 4 x 4 / 8 x 8 latents): the M tile is
// G WHOLE frames (TM*64 / S^2 of them), whose zero-padded footprints ((S+4) x (S+4) rows of 64 bytes per frame, PITCH = S + 4
// whatever the filter size) sit in LDS for all 9 / 25 taps of a channel chunk; weights from L2 in fragment-major order as above.
// 16-byte slot swizzle: (line of the footprint) & 3 -- brute-forced conflict-free for both ds_read_b128 lane groups, every tap,
// S = 8 (a 32-row sub-tile = 4 lines of one frame) and S = 4 (= 2 frames).
template <int TM, int S> struct HaloGbsCfg {
    using Rows = std::conditional_t<S == 8, RowsF8, RowsHalo>;           // fragment h = 1: one footprint line below fragment 0
    static_assert(Rows::pix(1, 0) == S, "fragment 1 = fragment 0 moved one line down");
    static constexpr int PITCH = S + 4, FR = PITCH * PITCH;             // rows per frame footprint
    static constexpr int G = TM * 64 / (S * S);                         // frames per tile
    static constexpr int HG = (G * FR + 15) / 16;
    static constexpr int HBYTES = HG * 1024;
    static constexpr int EPI = 4 * 32 * 64 * 4;
    static constexpr int LDSB = 2 * HBYTES + 1024 > EPI ? 2 * HBYTES + 1024 : EPI;
};

template <int TM, int S, bool RELU, int KS>
__device__ __forceinline__ void conv_halo_gbs_tile(const ConvK& p, char* const smem, const int mt, const int nt, const int z, const int ltile) {
    using T = bf16_t;
    using Cfg = HaloGbsCfg<TM, S>;
    using Rows = typename Cfg::Rows;
    constexpr int WN = 2, NWAVE = 4, BNt = 128;
    constexpr int PITCH = Cfg::PITCH, FR = Cfg::FR, G = Cfg::G, HG = Cfg::HG, HBYTES = Cfg::HBYTES;
    constexpr int NH = (HG + NWAVE - 1) / NWAVE;
    constexpr int SS = S * S;
    constexpr int ntap2 = KS * KS, pad = KS >> 1, ext = S + 2 * pad;   // footprint extent actually used by this filter
    char* const hbuf0 = &smem[0];
    char* const dump = &smem[2 * HBYTES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN, kg = lane >> 4;
    const int n0 = nt * BNt;
    const int ft0 = mt * G, nframes = p.M / SS;
    const int per = (p.kchunks + p.nsplit - 1) / p.nsplit;
    const int cc_begin = z * per, cc_end = min(p.kchunks, cc_begin + per);
    constexpr unsigned esz = 2;

    const int wu = __builtin_amdgcn_readfirstlane(wave);
    const int lrow = lane >> 2;
    const unsigned ldb = (unsigned)p.ldi * esz;
    const size_t base_b = (size_t)ft0 * SS * ldb;
    const size_t left_b = p.in_bytes - base_b;
    const __amdgpu_buffer_rsrc_t rin = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(p.in + base_b), 0, left_b > kRangeCap ? kRangeCap : (unsigned)left_b, 0x00020000);
    const int nb32 = p.nb32;
    const __amdgpu_buffer_rsrc_t rwq = __builtin_amdgcn_make_buffer_rsrc(
        (void*)p.wq, 0, (unsigned)((size_t)ntap2 * p.kchunks * nb32 * 2048), 0x00020000);
    auto hrow = [&](int i, int lrow, int& fl, int& hy, int& hx) __attribute__((always_inline)) {
        const int h = (i * NWAVE + wu) * 16 + lrow;
        fl = h / FR;
        const int r = h - fl * FR;
        hy = r / PITCH; hx = r - hy * PITCH;
    };
    unsigned hoff[NH];
#pragma unroll
    for (int i = 0; i < NH; ++i) {
        const int g = i * NWAVE + wu;
        int fl, hy, hx;
        hrow(i, lrow, fl, hy, hx);
        const int yin = hy - pad, xin = hx - pad;
        const int hq = (lane & 3) ^ (hy & 3);
        const bool ok = g < HG && fl < G && ft0 + fl < nframes && hy < ext && hx < ext && (unsigned)yin < (unsigned)S && (unsigned)xin < (unsigned)S;
        hoff[i] = ok ? (unsigned)((fl * S + yin) * S + xin) * ldb + hq * 16 : kRowOOB;
    }
    const bool ragged = (p.C & 31) != 0;
    auto dmaH = [&](int hb, int cc_) __attribute__((always_inline)) {
        const bool part_ = ragged && cc_ == p.kchunks - 1;
        int ln_ = lane;
        if (part_) asm volatile("" : "+v"(ln_));                         // (opaque: see conv_halo_gb_tile)
#pragma unroll
        for (int i = 0; i < NH; ++i) {
            const int g = i * NWAVE + wu;
            char* dst_ = g < HG ? hbuf0 + hb * HBYTES + g * 1024 : dump;
            unsigned off_ = hoff[i] + cc_ * 64;
            if (part_) {
                int fl, hy, hx;
                hrow(i, ln_ >> 2, fl, hy, hx);
                const int hq = (ln_ & 3) ^ (hy & 3);
                off_ = cc_ * 32 + hq * 8 < p.C ? off_ : kRowOOB;
            }
            dma16(rin, dst_, off_);
        }
    };
    const unsigned bvoff = (unsigned)(wn * 2 * 2048 + (kg >> 1) * 1024 + ((kg & 1) * 32 + (lane & 15)) * 16);
    const unsigned bnt = (unsigned)(nt * (BNt / 32)) * 2048u;
    const unsigned brec = (unsigned)nb32 * 2048u;
    const unsigned tapstep = (unsigned)p.kchunks * brec;
    auto ldBq = [&](bf16x8 (&b)[4], unsigned rec) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            b[j] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rwq, bvoff, rec + (unsigned)((j >> 1) * 2048 + (j & 1) * 256), 0));
    };

    Acc16<Rows> acc[TM];
#pragma unroll
    for (int a = 0; a < TM; ++a) acc_zero(acc[a]);
    // this lane's A rows: pixel pi = (wm*TM + tm)*32 + Rows::pix(h, lane & 15) of the tile -> (frame, y, x); sub-tile tm sits a
    // compile-time number of footprint rows further (S = 8: 4 lines or a whole frame, S = 4: two frames; y & 3 is the same for
    // every tm), fragment 1 one line below fragment 0
    const int pi0 = wm * (TM * 32) + Rows::pix(0, lane & 15);
    const int f0 = pi0 / SS, y0 = (pi0 % SS) / S, x0 = pi0 % S;
    const int arow0 = f0 * FR + y0 * PITCH + x0;
    auto tmoff = [](int tm) constexpr -> int { return S == 8 ? ((tm >> 1) * FR + (tm & 1) * 4 * PITCH) * 64 : tm * 2 * FR * 64; };
#ifdef DVD_EXP_NOMAIN
    const int nch = 0;
#else
    const int nch = cc_end - cc_begin;
#endif
    if (nch > 0) {
        unsigned rec = (unsigned)cc_begin * brec + bnt;                 // tap 0 of the first chunk; records are [tap][chunk]
        bf16x8 bq0[4], bq1[4];
        dmaH(0, cc_begin);
        ldBq(bq0, rec);
        __builtin_amdgcn_s_waitcnt(0x0070 | (0xf << 8));                // vmcnt(0)
        __builtin_amdgcn_s_barrier();
        int hb = 0, iy = 0, cc = cc_begin;                              // (row loop: see conv_halo_gb_tile)
        auto row = [&](bf16x8 (&b0)[4], bf16x8 (&b1)[4]) __attribute__((always_inline)) {
            const bool first = iy == 0, last = iy == KS - 1, more = cc + 1 < cc_end;
            const int swz[2] = {(y0 + iy) & 3, (y0 + iy + 1) & 3};
            const char* const Arow = hbuf0 + hb * HBYTES + (arow0 + iy * PITCH) * 64;
#pragma unroll
            for (int ix = 0; ix < KS; ++ix) {
                const char* const Ah = Arow + ix * 64;
                auto ldA = [&](int u) __attribute__((always_inline)) -> bf16x8 {
                    const int tm = u >> 1, h = u & 1;
                    return *reinterpret_cast<const bf16x8*>(Ah + tmoff(tm) + h * (PITCH * 64) + ((kg ^ swz[h]) << 4));
                };
                unsigned nrec = rec + tapstep;
                if (ix == KS - 1 && last) nrec = more ? (unsigned)(cc + 1) * brec + bnt : rec;
                auto next = [&]() __attribute__((always_inline)) {
                    ldBq((ix & 1) ? b0 : b1, nrec);
                    if (ix == 0 && first && more) dmaH(hb ^ 1, cc + 1);
                };
                gb_step<TM, RELU>(acc, (ix & 1) ? b1 : b0, ldA, next);
                rec = nrec;
            }
            ++iy;
            if (last) {
                iy = 0; hb ^= 1; ++cc;
                if (more) {
                    __builtin_amdgcn_s_waitcnt(0xc07f);
                    __builtin_amdgcn_s_barrier();
                }
            }
        };
        const int nrows = nch * KS;
        int r = 0;
#pragma unroll 1
        for (; r + 1 < nrows; r += 2) { row(bq0, bq1); row(bq1, bq0); }
        if (r < nrows) row(bq0, bq1);
    }
    __syncthreads();

    int te = tid;                                                        // (opaque: see conv_halo_gb_tile)
    asm volatile("" : "+v"(te));
    const int elane = te & 63, ewave = te >> 6, ewm = ewave / WN, ewn = ewave % WN;
    float* ep = reinterpret_cast<float*>(&smem[0]) + ewave * (32 * 64);
    const int ecol = (elane & 7) * 8, erow = elane >> 3;
    const long long row0 = (long long)ft0 * SS;
    conv_epilogue<T, TM, DVD_GB_EPI_DEEP>(p, acc, ep, elane, n0 + ewn * 64 + ecol, z, ltile, row0, [&](int tm, int j) __attribute__((always_inline)) {
        const int pi = ewm * (TM * 32) + tm * 32 + j * 8 + erow;          // the tile's rows are G consecutive whole frames
        return row0 + pi < p.M ? pi : -1;
    });
}

template <int TM, int S, bool RELU, int KS>
__global__ __launch_bounds__(256, TM == 2 && S == 8 ? 3 : 2) void conv_halo_gbs_kernel(ConvK p) {
    __shared__ __attribute__((aligned(16))) char smem[HaloGbsCfg<TM, S>::LDSB];
    const int bid = xcd_order(blockIdx.x, gridDim.x);
    const TileMN t = tile_of(p.nmajor, p.tilesN, bid, gridDim.x);
    conv_halo_gbs_tile<TM, S, RELU, KS>(p, smem, t.mt, t.nt, blockIdx.z, (int)blockIdx.x);
}

// ---------------------------------------------------------------------------- grouped launches
// Several INDEPENDENT convolutions in one grid (gru.hip: the recurrent / x-part convolutions of the layers of a ConvGRU stack that
// a layer wavefront makes independent).  A one-round launch runs its workgroups in lock step: prologue, main loop and the HBM-bound
// gate epilogue of all of them coincide and overlap with nothing.  In a grouped launch the workgroup slots of a CU hold tiles of
// different convolutions with different K lengths and epilogues, so one tile's epilogue runs under another's main loop, and the
// launch has several rounds.  Slot order: see ConvGroup (conv_common.h).
template <class TileFn>
__device__ __forceinline__ void group_dispatch(const ConvGroup& grp, TileFn fn) {
    const int x = blockIdx.x & 7;
    int rem = blockIdx.x >> 3;                                           // this XCD's rem-th workgroup
    auto share = [&](int m) __attribute__((always_inline)) -> int { const int w = grp.wgs[m]; return (w >> 3) + (x < (w & 7) ? 1 : 0); };
    const int m0 = grp.order[0], m1 = grp.n > 1 ? grp.order[1] : m0;
    const int s0 = share(m0), s1 = grp.n > 1 ? share(m1) : 0;
    const int h0 = min(grp.head, s0), h1 = min(grp.head, s1);
    int g = -1, off = 0;
    if (rem < h0) { g = m0; off = rem; }
    else if ((rem -= h0) < h1) { g = m1; off = rem; }
    else if ((rem -= h1) < s0 - h0) { g = m0; off = h0 + rem; }
    else if ((rem -= s0 - h0) < s1 - h1) { g = m1; off = h1 + rem; }
    else {
        rem -= s1 - h1;
        for (int k = 2; k < grp.n; ++k) {
            const int m = grp.order[k], s = share(m);
            if (rem < s) { g = m; off = rem; break; }
            rem -= s;
        }
    }
    if (g < 0) return;
    const int w = grp.wgs[g];
    const int local = x * (w >> 3) + min(x, w & 7) + off;               // index among member g's workgroups (tiles x slices)
    const ConvK& p = grp.c[g];
    const int t = local / p.nsplit, z = local - t * p.nsplit;
    const TileMN mn = tile_of(p.nmajor, p.tilesN, t, w / p.nsplit);
    fn(p, mn.mt, mn.nt, z, t);
}

template <int TM, int WN, int WMV>
__global__ __launch_bounds__(256, TM == 2 ? 3 : 2) void conv_group_gb_kernel(ConvGroup grp) {
    __shared__ __attribute__((aligned(16))) char smem[HaloGbCfg<TM, WN, WMV, false>::LDSB];
    group_dispatch(grp, [&](const ConvK& p, int mt, int nt, int z, int t) __attribute__((always_inline)) {
        if (p.kh == 5) conv_halo_gb_tile<TM, WN, WMV, false, false, 5>(p, smem, mt, nt, z, t);
        else conv_halo_gb_tile<TM, WN, WMV, false, false, 3>(p, smem, mt, nt, z, t);
    });
}

template <int TM, int S>
__global__ __launch_bounds__(256, TM == 2 && S == 8 ? 3 : 2) void conv_group_gbs_kernel(ConvGroup grp) {
    __shared__ __attribute__((aligned(16))) char smem[HaloGbsCfg<TM, S>::LDSB];
    group_dispatch(grp, [&](const ConvK& p, int mt, int nt, int z, int t) __attribute__((always_inline)) {
        if (p.kh == 5) conv_halo_gbs_tile<TM, S, false, 5>(p, smem, mt, nt, z, t);
        else conv_halo_gbs_tile<TM, S, false, 3>(p, smem, mt, nt, z, t);
    });
}

}  // namespace

// ---------------------------------------------------------------------------- launch tables (conv_igemm.hip: cv_launch; gru.hip)
namespace dvdk {
#define GB(R, C, KS, RL, UP) cv_key(CV_HALO_L2, 0, R, C, KS, RL, UP)
#define GBS(F, R, KS, RL) cv_key(F, 0, R, 128, KS, RL, 0)
static const ConvRow kGbRows[] = {
#ifdef DVD_GB_PROBE      // ISA inspection build (tools/isa_probe.sh): one instantiation of each kernel family
    {GB(256, 128, 5, 0, 0), conv_halo_gb_kernel<4, 2, 2, false, false, 5>}, {GBS(CV_FRAME8, 128, 3, 0), conv_halo_gbs_kernel<2, 8, false, 3>},
#else
    // weights from L2, frames >= 16 pixels: 256 x 128, 128 x 128 (launches with few rows), 256 x 64 (thin outputs); relu_in 0 | 1
    {GB(256, 128, 3, 0, 0), conv_halo_gb_kernel<4, 2, 2, false, false, 3>}, {GB(256, 128, 3, 1, 0), conv_halo_gb_kernel<4, 2, 2, true, false, 3>},
    {GB(256, 128, 3, 0, 1), conv_halo_gb_kernel<4, 2, 2, false, true, 3>},  {GB(256, 128, 3, 1, 1), conv_halo_gb_kernel<4, 2, 2, true, true, 3>},
    {GB(256, 128, 5, 0, 0), conv_halo_gb_kernel<4, 2, 2, false, false, 5>}, {GB(256, 128, 5, 1, 0), conv_halo_gb_kernel<4, 2, 2, true, false, 5>},
    {GB(256, 128, 5, 0, 1), conv_halo_gb_kernel<4, 2, 2, false, true, 5>},  {GB(256, 128, 5, 1, 1), conv_halo_gb_kernel<4, 2, 2, true, true, 5>},
    {GB(128, 128, 3, 0, 0), conv_halo_gb_kernel<2, 2, 2, false, false, 3>}, {GB(128, 128, 3, 1, 0), conv_halo_gb_kernel<2, 2, 2, true, false, 3>},
    {GB(128, 128, 3, 0, 1), conv_halo_gb_kernel<2, 2, 2, false, true, 3>},  {GB(128, 128, 3, 1, 1), conv_halo_gb_kernel<2, 2, 2, true, true, 3>},
    {GB(128, 128, 5, 0, 0), conv_halo_gb_kernel<2, 2, 2, false, false, 5>}, {GB(128, 128, 5, 1, 0), conv_halo_gb_kernel<2, 2, 2, true, false, 5>},
    {GB(128, 128, 5, 0, 1), conv_halo_gb_kernel<2, 2, 2, false, true, 5>},  {GB(128, 128, 5, 1, 1), conv_halo_gb_kernel<2, 2, 2, true, true, 5>},
    {GB(256, 64, 3, 0, 0), conv_halo_gb_kernel<2, 1, 4, false, false, 3>},  {GB(256, 64, 3, 1, 0), conv_halo_gb_kernel<2, 1, 4, true, false, 3>},
    {GB(256, 64, 3, 0, 1), conv_halo_gb_kernel<2, 1, 4, false, true, 3>},   {GB(256, 64, 3, 1, 1), conv_halo_gb_kernel<2, 1, 4, true, true, 3>},
    {GB(256, 64, 5, 0, 0), conv_halo_gb_kernel<2, 1, 4, false, false, 5>},  {GB(256, 64, 5, 1, 0), conv_halo_gb_kernel<2, 1, 4, true, false, 5>},
    {GB(256, 64, 5, 0, 1), conv_halo_gb_kernel<2, 1, 4, false, true, 5>},   {GB(256, 64, 5, 1, 1), conv_halo_gb_kernel<2, 1, 4, true, true, 5>},
    // whole-frame footprints: 8 x 8 frames on 256- or 128-row tiles, 4 x 4 frames on 128-row tiles
    {GBS(CV_FRAME8, 256, 3, 0), conv_halo_gbs_kernel<4, 8, false, 3>},      {GBS(CV_FRAME8, 256, 3, 1), conv_halo_gbs_kernel<4, 8, true, 3>},
    {GBS(CV_FRAME8, 256, 5, 0), conv_halo_gbs_kernel<4, 8, false, 5>},      {GBS(CV_FRAME8, 256, 5, 1), conv_halo_gbs_kernel<4, 8, true, 5>},
    {GBS(CV_FRAME8, 128, 3, 0), conv_halo_gbs_kernel<2, 8, false, 3>},      {GBS(CV_FRAME8, 128, 3, 1), conv_halo_gbs_kernel<2, 8, true, 3>},
    {GBS(CV_FRAME8, 128, 5, 0), conv_halo_gbs_kernel<2, 8, false, 5>},      {GBS(CV_FRAME8, 128, 5, 1), conv_halo_gbs_kernel<2, 8, true, 5>},
    {GBS(CV_FRAME4, 128, 3, 0), conv_halo_gbs_kernel<2, 4, false, 3>},      {GBS(CV_FRAME4, 128, 3, 1), conv_halo_gbs_kernel<2, 4, true, 3>},
    {GBS(CV_FRAME4, 128, 5, 0), conv_halo_gbs_kernel<2, 4, false, 5>},      {GBS(CV_FRAME4, 128, 5, 1), conv_halo_gbs_kernel<2, 4, true, 5>},
#endif
};
#undef GB
#undef GBS
bool launch_gb(unsigned key, const ConvK& p, dim3 grid, hipStream_t st) { return cv_launch_row(kGbRows, (int)(sizeof kGbRows / sizeof kGbRows[0]), key, p, grid, 256, st); }
// the kernel of kGroupKind[kind] (<rows / 64, 2, 2> | <rows / 64, side>); every member: bf16, fragment-major weights, no input ReLU, no upsample
static void (*const kGroupKernel[])(ConvGroup) = {
#ifdef DVD_GB_PROBE
    conv_group_gb_kernel<4, 2, 2>, conv_group_gb_kernel<4, 2, 2>, conv_group_gb_kernel<4, 2, 2>, conv_group_gb_kernel<4, 2, 2>, conv_group_gb_kernel<4, 2, 2>,
#else
    conv_group_gb_kernel<4, 2, 2>, conv_group_gb_kernel<2, 2, 2>, conv_group_gbs_kernel<4, 8>, conv_group_gbs_kernel<2, 8>, conv_group_gbs_kernel<2, 4>,
#endif
};
static_assert(sizeof kGroupKernel / sizeof kGroupKernel[0] == kGroupKinds, "one kernel per row of kGroupKind");
void launch_group(const ConvGroup& grp, int kind, hipStream_t st) { kGroupKernel[kind]<<<dim3(grp.nslots), 256, 0, st>>>(grp); }
}  // namespace dvdk
