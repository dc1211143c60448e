// conv_route_table.cpp -- one row per convolution descriptor of a fixed grid: the route conv_route gives it.
//
// tests/test_conv_route_cpu.py builds this for the host only, links it against libdlpm_amd.so and compares its output row by row with
// tests/golden/conv_routes.txt, which the selector cascade wrote before conv_route replaced it (same grid, the first-true selector in
// the launch order, conv_stats_pixels behind the gate the callers put in front of it, conv_ksplit_for, the grid formulas at
// dispatch_B).  conv_route is a pure host function: no GPU is touched, the weight pointers are dummies that nobody follows.
//
// The grid: the cross product of the axes below, pruned of combinations no caller can build, and subsampled by a hash of the
// combination's index (a function of the grid alone, never of a route).  (24, 0) input channels stand beside the layer widths of the
// nets: the F(4x4) kernel takes channels in multiples of 8, the implicit GEMM in multiples of 32.
#include <cstdint>
#include <cstdio>

#include "../dlpm_amd/csrc/conv.h"

using namespace dlpm;

static const float DUMMY[4] = {0.f, 0.f, 0.f, 0.f};
static const char *const FAMILY[] = {"HEAD_FUSED", "HEAD_GEMM", "HEAD", "SPLIT", "WINO4SP", "WINO4", "WINO", "IGEMM", "STEM", "DIRECT"};

// family bh bw nimg nq stats_px ksplit grid
static void route_columns(const ConvLaunch &L) {
    const ConvRoute r = conv_route(L);
    printf("%s %d %d %d %d %d %d %lld", FAMILY[r.family], r.bh, r.bw, r.nimg, r.nq, r.stats_px, r.ksplit, (long long)r.grid);
}

// The weight layouts a launch carries.  'p': what the UNet's prep_conv builds for the layer (and, under a small declared batch, the
// narrow F(4x4) copies); 'w': the plain weights only; the others: what dlpm_conv2d_f32 attaches -- 'd' with no force bit, '2' without
// the Winograd copies, '8' F(4x4), 's' (bit 16) bf16x3 split, 't' (bit 32) head taps, 'h' (bit 64) fused head, 'u' (bit 256) sub-pixel.
static void attach(ConvLaunch &L, char set) {
    const int Cin = L.C0 + L.C1;
    const bool ig = igemm_supported(L);
    const bool head_shape = L.ks == 3 && L.C0 % 32 == 0 && L.C1 == 0;
    L.w = DUMMY;
    if (set == 'w') return;
    if (set == 'p') {
        const bool plain = !L.in_nchw && !L.out_nchw && L.stride == 1;     // prep_conv's boundary 0
        if (ig && L.ks == 1) {
            if (L.Cout % 128 == 0 && Cin % 32 == 0 && plain) L.w_split = DUMMY;
            return;
        }
        if (L.ks == 3 && L.Cout <= 4 && Cin % 32 == 0) {
            L.w_small = DUMMY;
            if (L.Cout <= 3) L.w_taps = DUMMY;
            if (L.Cout <= 3 && Cin <= 128) L.w_hfused = DUMMY;
        }
        if (ig && L.ks == 3 && L.stride == 2 && L.Cout % 128 == 0 && Cin % 32 == 0) L.w_split = DUMMY;
        if (ig && L.ks == 3 && Cin % 32 == 0) {
            L.w_frag = DUMMY;
            if (L.Cout % 64 == 0 && plain) L.w_wino = DUMMY;
            if (wino4_enabled() && L.Cout % 32 == 0 && plain) {
                L.w_wino4 = DUMMY;
                if (L.ups && wino4sp_layer_ok(L.Cout, Cin, L.Hin, L.Win)) L.w_wino4sp = DUMMY;
                if (L.Cout % 128 == 0 && L.dispatch_B > 0 && L.dispatch_B <= 512) L.w_wino4_n64 = L.w_wino4_n32 = DUMMY;
            }
        }
        return;
    }
    if (ig && set == 's' && L.Cout % 128 == 0 && Cin % 32 == 0) L.w_split = DUMMY;
    const bool wino_shape = L.ks == 3 && !L.w_split && set != '2' && L.stride == 1 && !L.in_nchw && !L.out_nchw;
    if (ig && L.ks == 3 && !L.w_split && Cin % 32 == 0) {
        L.w_frag = DUMMY;
        if (wino_shape && L.Cout % 64 == 0) L.w_wino = DUMMY;
    }
    if (wino_shape && (set == '8' || set == 'u') && L.Cout % 32 == 0 && Cin % 8 == 0) {
        L.w_wino4 = DUMMY;
        L.w_wino = nullptr;
        if (set == 'u' && L.Cout % 128 == 0) L.w_wino4sp = DUMMY;
    }
    if (set == 'h' && head_shape && L.Cout <= 3) L.w_hfused = DUMMY;
    else if (set == 't' && head_shape && L.Cout <= 3) L.w_taps = DUMMY;
    else if (set == 'd' && head_shape && L.Cout <= 4) L.w_small = DUMMY;
}

int main() {
    static const int GEOM[][3] = {{1, 1, 0}, {3, 1, 0}, {3, 2, 0}, {3, 1, 1}};                        // ks, stride, ups
    static const int SIZE[][2] = {{4, 4}, {8, 8}, {14, 14}, {16, 16}, {28, 28}, {32, 32}, {64, 64}, {8, 16}};   // Hout, Wout
    static const int CIN[][2] = {{1, 0}, {3, 0}, {16, 16}, {24, 0}, {32, 0}, {32, 32}, {64, 64}, {128, 0}, {128, 128}, {256, 128}};
    static const int COUT[] = {1, 3, 32, 64, 96, 128, 256};
    static const int64_t DISPATCH[] = {0, 2, 64, 256, 4096};
    static const int BATCH[] = {2, 5, 64};
    static const char SETS[] = "pwd28sthu";
    uint64_t index = 0;
    for (const auto &g : GEOM) for (const auto &sz : SIZE) for (const auto &ci : CIN) for (int Cout : COUT)
    for (int res = 0; res < 3; res++) for (int coef = 0; coef < 2; coef++) for (int gen = 0; gen < 4; gen++) for (int64_t dB : DISPATCH)
    for (int gemm = 0; gemm < 3; gemm++) for (int B : BATCH) for (const char *set = SETS; *set; set++) {
        const bool in_nchw = ci[0] < 16, out_nchw = Cout < 32;
        // pruned: a boundary layout on a 1x1 / resampling / concat / residual launch, both boundaries at once; the head without its GroupNorm
        if ((in_nchw || out_nchw) && (g[0] != 3 || g[1] != 1 || g[2] || res)) continue;
        if ((in_nchw && out_nchw) || (out_nchw && !coef)) continue;
        // 1 in `keep` of the surviving combinations is kept, by a hash of their running index.  The rate follows the DESCRIPTOR so that the rare
        // kernels get their rows: the head shapes with a head layout, the upsampling launches with sub-pixel weights, the stem shapes
        const bool head_set = *set == 'd' || *set == 'p' || *set == 'h' || *set == 't';
        const uint64_t keep = out_nchw ? (*set == 'd' ? 60 : head_set ? 120 : 1500) : in_nchw ? 1200 : (g[2] && (*set == 'p' || *set == 'u')) ? 1200 : 5200;
        uint64_t h = ++index * 0x9E3779B97F4A7C15ull;
        h ^= h >> 29;
        if (h % keep != 0) continue;
        ConvLaunch L;
        L.ks = g[0]; L.stride = g[1]; L.ups = g[2];
        L.Hout = sz[0]; L.Wout = sz[1];
        L.Hin = L.stride == 2 ? 2 * L.Hout : L.ups ? L.Hout / 2 : L.Hout;
        L.Win = L.stride == 2 ? 2 * L.Wout : L.ups ? L.Wout / 2 : L.Wout;
        L.C0 = ci[0]; L.C1 = ci[1]; L.Cout = Cout; L.B = B;
        L.src0 = DUMMY; L.src1 = L.C1 ? DUMMY : nullptr; L.bias = DUMMY;
        L.in_nchw = in_nchw; L.out_nchw = out_nchw;
        if (coef) L.coefA = L.coefB = DUMMY;
        L.act_silu = out_nchw;
        if (res) { L.res0 = DUMMY; L.R0 = res == 1 ? Cout : Cout / 2; }
        if (res == 2) L.res1 = DUMMY;
        L.gen = gen; L.dispatch_B = dB; L.gemm = gemm;
        attach(L, *set);
        printf("k%ds%du%d %dx%d c%d+%d o%d r%d a%d g%d d%lld m%d b%d %c | ", L.ks, L.stride, L.ups, L.Hout, L.Wout, L.C0, L.C1, Cout, res, coef, gen,
               (long long)dB, gemm, B, *set);
        route_columns(L);
        printf("\n");
    }
    return 0;
}
