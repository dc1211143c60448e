// conv_tile_table.cpp -- the route conv_route gives each row of tests/conv_tile_cases.py.
//
// tests/test_conv_tile_cases_cpu.py builds this for the host only, links it against libdlpm_amd.so and feeds it one line per row on
// standard input (conv_tile_cases.descriptor_line):
//   name B C0 C1 Hin Win Hout Wout Cout ups coef+silu R0 rescat bias in_nchw out_nchw force_direct scratch_floats
// For each it attaches the weight layouts as dlpm_conv2d_f32 (csrc/unet.hip: conv2d_entry) would for the row's force bits and scratch
// size and prints
//   name family route-name frag_weight_floats(Cout, Cin)
// conv_route is a pure host function: no GPU is touched, the weight pointers are dummies that nobody follows.
#include <cstdint>
#include <cstdio>

#include "../dlpm_amd/csrc/conv.h"

using namespace dlpm;

static const float DUMMY[4] = {0.f, 0.f, 0.f, 0.f};
static const char *const FAMILY[] = {"HEAD_FUSED", "HEAD_GEMM", "HEAD", "SPLIT", "WINO4SP", "WINO4", "WINO", "IGEMM", "STEM", "DIRECT"};

// conv2d_entry's placement, for the bits the table uses (1, 2, 32, 64, 128): which layouts fit the scratch buffer front to back
static void attach(ConvLaunch &L, int fd, int64_t cap) {
    const int Cin = L.C0 + L.C1;
    const bool ig = !(fd & 1) && igemm_supported(L);
    L.gemm = DLPM_GEMM_F32;
    L.w = DUMMY;
    int64_t used = (int64_t)L.Cout * Cin * L.ks * L.ks;       // the plain copy, whatever the size says
    const bool wino_shape = L.ks == 3 && !(fd & 2) && L.stride == 1 && !L.in_nchw && !L.out_nchw;
    if (ig && L.ks == 3 && Cin % 32 == 0) {
        const int64_t frag = frag_weight_floats(L.Cout, Cin);
        if (used + frag <= cap) {
            L.w_frag = DUMMY;
            used += frag;
        }
        if (wino_shape && L.Cout % 64 == 0 && used + wino_weight_floats(L.Cout, Cin) <= cap) L.w_wino = DUMMY;
    }
    const bool head_shape = L.ks == 3 && L.C0 % 32 == 0 && L.C1 == 0;
    const int ask_head = !head_shape || L.Cout > 3 ? 0 : (fd & 64) ? 64 : (fd & 32);
    if (ask_head == 64) {
        L.gemm = (fd & 128) ? DLPM_GEMM_F32 : DLPM_GEMM_AUTO;
        if (head_fused_weight_floats(Cin) <= cap) L.w_hfused = DUMMY;
    } else if (ask_head == 32) {
        if ((int64_t)head_taps_rows(L.Cout) * Cin <= cap - head_gemm_scratch_floats(L)) L.w_taps = DUMMY;
    } else if (!(fd & 7) && head_shape && L.Cout <= 4) {
        const int64_t front = cap - (int64_t)9 * Cin * 4;
        if (front >= (int64_t)L.Cout * Cin * 9 + frag_weight_floats(L.Cout, Cin)) L.w_small = DUMMY;
    }
}

int main() {
    char name[128];
    int B, C0, C1, Hin, Win, Hout, Wout, Cout, ups, act, R0, rescat, bias, in_nchw, out_nchw, fd;
    long long cap;
    while (scanf("%127s %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %lld", name, &B, &C0, &C1, &Hin, &Win, &Hout, &Wout, &Cout, &ups, &act, &R0,
                 &rescat, &bias, &in_nchw, &out_nchw, &fd, &cap) == 18) {
        ConvLaunch L;
        L.ks = 3; L.stride = 1; L.ups = ups;
        L.B = B; L.C0 = C0; L.C1 = C1; L.Hin = Hin; L.Win = Win; L.Hout = Hout; L.Wout = Wout; L.Cout = Cout;
        L.src0 = DUMMY; L.src1 = C1 ? DUMMY : nullptr;
        if (bias) L.bias = DUMMY;
        if (act) L.coefA = L.coefB = DUMMY;
        L.act_silu = act;
        if (R0) { L.res0 = DUMMY; L.R0 = R0; }
        if (rescat) L.res1 = DUMMY;
        L.in_nchw = in_nchw; L.out_nchw = out_nchw;
        attach(L, fd, cap);
        const ConvRoute r = conv_route(L);
        printf("%s %s %s %lld\n", name, FAMILY[r.family], r.name[0] ? r.name : "-", (long long)frag_weight_floats(Cout, C0 + C1));
    }
    return 0;
}
