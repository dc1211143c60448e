// conv_layout_table.cpp -- one row per layer of a fixed grid: the weight layouts conv_layouts (conv.h) grants it, each with its float count.
//
// tests/test_conv_layouts_cpu.py builds this for the host only, links it against libdlpm_amd.so and compares its output row by row with
// tests/golden/conv_layouts.txt, which was written before the table existed: by conv3_layouts, the *_weight_floats functions and the
// conditions prep_conv spelled out inline (same grid).  conv_layouts is a pure host function: no GPU is touched.
//
// The grid: layer kind x kernel size x image size x input channels x output channels x declared batch, pruned of the combinations no net
// builds (the time MLP is 1x1 on one pixel; the stem, the head, the stride-2 and the Upsample convolutions are 3x3; the stem has at most 3
// input channels, the head at most 3 output channels, and only they), and subsampled by a hash of the combination's index (a function of
// the grid alone).  The size is the one the layer's input has: a stride-2 layer halves it, an Upsample layer doubles it.
#include <cstdint>
#include <cstdio>

#include "../dlpm_amd/csrc/conv.h"

using namespace dlpm;

enum Kind { ORDINARY, STEM, HEAD, TIME_MLP, STRIDE2, UPSAMPLE, KINDS };
static const char *const KIND[KINDS] = {"ordinary", "stem", "head", "time_mlp", "stride2", "upsample"};

int main() {
    static const int KS[] = {1, 3};
    static const int SIZE[] = {4, 8, 16, 32};
    static const int CIN[][2] = {{1, 0}, {3, 0}, {16, 16}, {24, 0}, {32, 0}, {32, 32}, {64, 64}, {128, 0}, {128, 128}, {256, 128}};   // conv_route_table.cpp's
    static const int COUT[] = {1, 3, 32, 64, 96, 128, 256};
    static const int64_t DISPATCH[] = {0, 2, 64, 512, 513, 4096};
    static const uint64_t KEEP[KINDS] = {2, 1, 1, 1, 2, 2};      // 1 in KEEP[kind] of the surviving combinations is kept
    uint64_t index = 0;
    for (int kind = 0; kind < KINDS; kind++) for (int ks : KS) for (int H : SIZE) for (const auto &ci : CIN) for (int Cout : COUT)
    for (int64_t dB : DISPATCH) {
        if (kind == TIME_MLP ? (ks != 1 || H != SIZE[0]) : kind != ORDINARY && ks != 3) continue;
        if ((kind == STEM) != (ci[0] < 16) || (kind == HEAD) != (Cout < 32)) continue;
        if (kind != ORDINARY && ci[1] != 0) continue;        // only a ResBlock's convolutions read a concat
        uint64_t h = ++index * 0x9E3779B97F4A7C15ull;
        h ^= h >> 29;
        if (h % KEEP[kind] != 0) continue;
        ConvLaunch L;       // the layer as the UNet describes it to conv_layouts
        L.C0 = ci[0]; L.C1 = ci[1]; L.Cout = Cout; L.ks = ks; L.dispatch_B = dB;
        L.Hin = L.Win = L.Hout = L.Wout = kind == TIME_MLP ? 1 : H;
        if (kind == STEM) L.in_nchw = 1;
        if (kind == HEAD) L.out_nchw = 1;
        if (kind == TIME_MLP) L.gemm = DLPM_GEMM_F32;
        if (kind == STRIDE2) { L.stride = 2; L.Hout = L.Wout = (H - 1) / 2 + 1; }
        if (kind == UPSAMPLE) { L.ups = 1; L.Hout = L.Wout = 2 * H; }
        printf("%s k%d %dx%d c%d+%d o%d d%lld |", KIND[kind], ks, L.Hin, L.Win, L.C0, L.C1, Cout, (long long)dB);
        const unsigned m = conv_layouts(L);
        for (int l = 0; l < CONV_LAYOUT_COUNT; l++)
            if (m >> l & 1) printf(" %s:%lld", conv_layout(l).name, (long long)conv_layout(l).floats(L));
        printf("\n");
    }
    return 0;
}
