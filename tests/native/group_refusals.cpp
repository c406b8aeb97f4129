// Host program of tests/test_abi_cpu.py::test_group_refusals_are_pinned.  dvd_conv_forward_group is internal (hidden from the shared
// library's exports), so the test links this file against the library's object files and reads "label return-code" lines.  Every call
// below is refused by the entry point's host-side checks: the placeholder pointers are never dereferenced and nothing is launched.
#include "common.h"
#include <cstdio>

static void* const kPtr = (void*)64;

static dvd_conv_desc member(int side, int relu_in = 0, int up2 = 0, bool ws = false) {
    dvd_conv_desc d = {};
    d.dtype = DVD_BF16; d.frames = 4; d.T = 1; d.H = d.W = side; d.C = d.ldi = 64; d.Cout = d.ldo = 64;
    d.kt = 1; d.kh = d.kw = 3; d.nsplit = 1; d.relu_in = relu_in; d.up2 = up2;
    d.in = d.w = d.wq = kPtr; d.out = kPtr; d.wq_kind = 1;
    if (ws) d.ws = (float*)kPtr;
    return d;
}

int main() {
    const GruEpi g[8] = {};                              // mode 0: direct epilogue
    dvd_conv_desc d[8];
    for (auto& m : d) m = member(16);
    std::printf("n=0 %d\n", dvd_conv_forward_group(d, g, 0, 0, 0, nullptr));
    std::printf("n=7 %d\n", dvd_conv_forward_group(d, g, 7, 0, 0, nullptr));
    std::printf("kind=-1 %d\n", dvd_conv_forward_group(d, g, 1, -1, 0, nullptr));
    std::printf("kind=5 %d\n", dvd_conv_forward_group(d, g, 1, 5, 0, nullptr));
    // a member whose geometry does not fit `kind`: 16 x 16 frames fit kinds 0 / 1, 8 x 8 frames kinds 2 / 3, 4 x 4 frames kind 4
    const int sides[3] = {16, 8, 4};
    for (int side : sides)
        for (int kind = 0; kind < 5; ++kind) {
            if (side == 16 ? kind <= 1 : side == 8 ? (kind == 2 || kind == 3) : kind == 4) continue;      // (fits: would launch)
            d[0] = member(side);
            std::printf("side=%d,kind=%d %d\n", side, kind, dvd_conv_forward_group(d, g, 1, kind, 0, nullptr));
        }
    // a fitting first member, then one with relu_in / up2 / ws
    for (int side : sides) {
        const int kind = side == 16 ? 0 : side == 8 ? 3 : 4;
        d[0] = member(side);
        d[1] = member(side, 1);
        std::printf("side=%d,relu_in %d\n", side, dvd_conv_forward_group(d, g, 2, kind, 0, nullptr));
        d[1] = member(side, 0, 1);
        std::printf("side=%d,up2 %d\n", side, dvd_conv_forward_group(d, g, 2, kind, 0, nullptr));
        d[1] = member(side, 0, 0, true);
        std::printf("side=%d,ws %d\n", side, dvd_conv_forward_group(d, g, 2, kind, 0, nullptr));
    }
    return 0;
}
