// Host program of tests/test_abi_cpu.py::test_stack_schedule_is_pinned.  dvd_convgru_stack_dump is internal (hidden from the shared
// library's exports), so the test links this file against the library's object files and compares what it prints with
// tests/native/stack_schedule.txt.  Recording a schedule is host arithmetic on the descriptor: the placeholder pointers are never
// dereferenced and nothing is launched.
#include "common.h"
#include <cstdio>
#include <initializer_list>

static char* const kPtr = (char*)64;

struct Spec {
    const char* name;
    int S, B, T, n;
    int hid[4], k[4];
    int h0;                    // bit l: layer l has a supplied initial state (and wants its gradient)
    int outer;                 // 1: every layer below the top one gets a gradient from outside the stack as well
    int layer_policy, ns_cap;
};

static dvd_gru_stack_desc stack(const Spec& c) {
    dvd_gru_stack_desc s = {};
    s.n_layers = c.n; s.layer_policy = c.layer_policy; s.ws = (float*)kPtr;
    for (int l = 0; l < c.n; ++l) {
        dvd_gru_desc& d = s.layer[l];
        d.dtype = DVD_BF16; d.T = c.T; d.B = c.B; d.H = d.W = c.S; d.hidden = c.hid[l]; d.k = c.k[l]; d.ns_cap = c.ns_cap;
        d.gx_stride = (long long)c.B * c.S * c.S * 3 * c.hid[l];
        d.gx = d.w_ur = d.w_o = d.wd_ur = d.wd_o = d.w_ur_q = d.w_o_q = d.wd_ur_q = d.wd_o_q = kPtr;
        d.h_all = d.u_all = d.r_all = d.o_all = d.hr_all = d.dg = kPtr;
        d.h32 = d.carry = (float*)kPtr; d.tickets = (unsigned*)kPtr;
        if ((c.h0 >> l) & 1) { d.h0 = kPtr; d.dh0 = (float*)kPtr; }
        if (l == c.n - 1 || c.outer) d.dh_out = kPtr;
        if (l) {
            s.cin[l] = c.hid[l - 1];
            s.wx[l] = s.wx_q[l] = s.wdx[l] = s.wdx_q[l] = kPtr; s.bx[l] = (const float*)kPtr; s.dh_mid[l] = kPtr;
        }
    }
    return s;
}

int main() {
    const Spec specs[] = {
        // the four ConvGRUs of the generator at ch = 32, B = 64
        {"gru0 S=4", 4, 64, 6, 3, {256, 512, 256}, {3, 5, 3}, 0, 0, 0, 0},
        {"gru1 S=8", 8, 64, 6, 3, {256, 512, 256}, {3, 5, 3}, 0, 0, 0, 0},
        {"gru2 S=16", 16, 64, 6, 3, {256, 512, 256}, {3, 5, 3}, 0, 0, 0, 0},
        {"gru3 S=32", 32, 64, 6, 3, {128, 256, 128}, {3, 5, 5}, 0, 0, 0, 0},
        {"S=8 h0 on every layer, outer gradients", 8, 64, 6, 3, {256, 512, 256}, {3, 5, 3}, 7, 1, 0, 0},
        {"S=4 h0 on layers 0 and 2", 4, 64, 6, 3, {256, 512, 256}, {3, 5, 3}, 5, 0, 0, 0},
        {"S=4 B=16", 4, 16, 6, 3, {256, 512, 256}, {3, 5, 3}, 0, 0, 0, 0},
        {"S=32 B=16", 32, 16, 6, 3, {128, 256, 128}, {3, 5, 5}, 0, 0, 0, 0},
        {"S=8 layer_policy=1 ns_cap=2", 8, 64, 6, 3, {256, 512, 256}, {3, 5, 3}, 0, 0, 1, 2},
        {"S=16 T=1", 16, 64, 1, 3, {256, 512, 256}, {3, 5, 3}, 0, 0, 0, 0},
        {"S=16 T=2", 16, 64, 2, 3, {256, 512, 256}, {3, 5, 3}, 0, 0, 0, 0},
        {"one layer S=4 h=512 k=5", 4, 64, 6, 1, {512}, {5}, 0, 0, 0, 0},
        // four layers on 8 x 8 frames: groups of five and six members (the coordinate-descent split-K search)
        {"four layers S=8 T=8", 8, 64, 8, 4, {256, 512, 256, 256}, {3, 5, 3, 3}, 0, 0, 0, 0},
    };
    for (const Spec& c : specs)
        for (int backward : {0, 1}) {
            const dvd_gru_stack_desc s = stack(c);
            std::printf("== %s, %s\n", c.name, backward ? "backward" : "forward");
            const int rc = dvd_convgru_stack_dump(&s, backward, stdout);
            if (rc) std::printf("rc=%d\n", rc);
        }
    return 0;
}
