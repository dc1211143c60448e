// conv_layouts.hip -- the weight layouts of a convolution layer (conv.h: ConvLayout): which a layer gets, how large each is, which call
// builds it and which ConvLaunch field receives it.  Host code only; the sizes and relayout kernels themselves live with the kernels
// that read the layout.
#include "conv.h"

namespace dlpm {

// One LAYOUT per row: the size in floats and the relayout call, as expressions over the layer c (Cin: its input channels), the OIHW
// weights w, the destination d and the stream st; the ConvLaunch field that receives the layout.  (Plain functions and a function-local
// table: a lambda or a namespace-scope constant in a HIP source is compiled for the device as well.)
#define LAYOUT(id, FLOATS, BUILD, FIELD)                                                            \
    static int64_t id##_floats(const ConvLaunch &c) {                                               \
        const int Cin = c.C0 + c.C1;                                                                \
        return FLOATS;                                                                              \
    }                                                                                               \
    static int id##_build(const ConvLaunch &c, const float *w, float *d, hipStream_t st) {          \
        const int Cin = c.C0 + c.C1;                                                                \
        return BUILD;                                                                               \
    }                                                                                               \
    static void id##_attach(ConvLaunch &c, const float *p) { c.FIELD = p; }
LAYOUT(plain, (int64_t)c.Cout * Cin * c.ks * c.ks, relayout_weight(w, d, c.Cout, Cin, c.ks, true, st), w)
LAYOUT(plain_direct, (int64_t)c.Cout * Cin * c.ks * c.ks, relayout_weight(w, d, c.Cout, Cin, c.ks, false, st), w)
LAYOUT(frag, frag_weight_floats(c.Cout, Cin), relayout_weight_frag(w, d, c.Cout, Cin, st), w_frag)
LAYOUT(wino, wino_weight_floats(c.Cout, Cin), relayout_weight_wino(w, d, c.Cout, Cin, st), w_wino)
LAYOUT(wino4, wino4_weight_floats(c.Cout, Cin), relayout_weight_wino4(w, d, c.Cout, Cin, st), w_wino4)
LAYOUT(wino4sp, wino4sp_weight_floats(c.Cout, Cin), relayout_weight_wino4sp(w, d, c.Cout, Cin, st), w_wino4sp)
LAYOUT(wino4_one, wino4_weight_floats(c.Cout, Cin), relayout_weight_wino4(w, d, c.Cout, Cin, st, 64), w_wino4_one)
LAYOUT(wino4_n64, wino4_weight_floats(c.Cout, Cin), relayout_weight_wino4(w, d, c.Cout, Cin, st, 64), w_wino4_n64)
LAYOUT(wino4_n32, wino4_weight_floats(c.Cout, Cin), relayout_weight_wino4(w, d, c.Cout, Cin, st, 32), w_wino4_n32)
LAYOUT(split, split_weight_floats(c.Cout, Cin, c.ks * c.ks), relayout_weight_split(w, d, c.Cout, Cin, c.ks * c.ks, st), w_split)
LAYOUT(head, (int64_t)9 * Cin * 4, relayout_weight_head(w, d, c.Cout, Cin, st), w_small)
LAYOUT(head_taps, (int64_t)head_taps_rows(c.Cout) * Cin, relayout_weight_head_taps(w, d, c.Cout, Cin, st), w_taps)
LAYOUT(head_fused, head_fused_weight_floats(Cin), relayout_weight_head_fused(w, d, c.Cout, Cin, st), w_hfused)
LAYOUT(small, small_weight_floats(c.Cout, Cin, c.ks), relayout_weight_small(w, d, c.Cout, Cin, c.ks, st), w)   // (small_attach: unused)
#undef LAYOUT

const ConvLayoutRow &conv_layout(int l) {
#define ROW(id) {#id, id##_floats, id##_build, id##_attach}
    static const ConvLayoutRow rows[CONV_LAYOUT_COUNT] = {      // in the order of the enum
        ROW(plain), ROW(plain_direct), ROW(frag), ROW(wino), ROW(wino4), ROW(wino4sp), ROW(wino4_one), ROW(wino4_n64), ROW(wino4_n32),
        ROW(split), ROW(head), ROW(head_taps), ROW(head_fused), {"small", small_floats, small_build, nullptr},
    };
#undef ROW
    return rows[l];
}

unsigned conv_layouts(const ConvLaunch &c) {
    const int Cin = c.C0 + c.C1;
    const bool ig = igemm_supported(c);
    const bool plain = !c.in_nchw && !c.out_nchw && c.stride == 1;     // neither a boundary layer nor a downsampling convolution ...
    const bool mixed = plain && c.gemm != DLPM_GEMM_F32;               // ... nor one that stays on the fp32 pipe: an ordinary layer of the plan
    unsigned m = 0;
    if (!(ig && c.ks == 1)) m |= lay_bit(ig ? LAY_PLAIN : LAY_PLAIN_DIRECT);   // ([O][I] row-major is already the 1x1 implicit GEMM's layout)
    if (mixed && small_weight_ok(c.Cout, Cin, c.ks)) m |= lay_bit(LAY_SMALL);
    // bf16x3 planes: the ordinary 1x1 convolutions and the stride-2 downsampling ones
    if (ig && c.Cout % 128 == 0 && Cin % 32 == 0 && (c.ks == 1 ? mixed : c.stride == 2)) m |= lay_bit(LAY_SPLIT);
    if (c.ks != 3) return m;
    if (c.Cout <= 4 && Cin % 32 == 0) {
        m |= lay_bit(LAY_HEAD);
        if (c.Cout <= 3) m |= lay_bit(LAY_HEAD_TAPS);
        if (c.Cout <= 3 && Cin <= 128) m |= lay_bit(LAY_HEAD_FUSED);
    }
    if (!ig || Cin % 32 != 0) return m;
    m |= lay_bit(LAY_FRAG);
    if (plain && c.Cout % 64 == 0 && Cin % 16 == 0) m |= lay_bit(LAY_WINO);      // Winograd-domain copy (stride-1 launches pick it up)
    if (!(plain && wino4_enabled() && c.Cout % 32 == 0 && Cin % 8 == 0)) return m;
    m |= lay_bit(LAY_WINO4);                                                       // F(4x4,3x3) copy (128-, 64- or 32-channel n-tiles)
    if (c.ups && wino4sp_layer_ok(c.Cout, Cin, c.Hin, c.Win)) m |= lay_bit(LAY_WINO4SP);                    // sub-pixel copy of an Upsample convolution
    if (!c.ups && wino4_one_layer_ok(c.Cout, c.C0, c.C1, c.Hout, c.Wout)) m |= lay_bit(LAY_WINO4_ONE);      // one-tile copy of a layer on 4x4-pixel tensors
    // 64- / 32-channel n-tile copies: under a small declared batch the narrow shapes give 2-4x as many workgroups (3x the F(4x4) weight bytes)
    if (c.Cout % 128 == 0 && c.dispatch_B > 0 && c.dispatch_B <= NARROW_COPIES_MAX_BATCH) m |= lay_bit(LAY_WINO4_N64) | lay_bit(LAY_WINO4_N32);
    return m;
}

unsigned place_conv_layouts(const ConvLaunch &layer, unsigned mask, float *base, int64_t align, int64_t cap, float *at[CONV_LAYOUT_COUNT],
                            int64_t *used) {
    unsigned placed = 0;
    for (int l = 0; l < CONV_LAYOUT_COUNT; l++) {
        if (!(mask >> l & 1)) continue;
        const int64_t lo = (*used + align - 1) / align * align, n = conv_layout(l).floats(layer);
        if (lo + n > cap) continue;
        at[l] = base + lo;
        *used = (lo + n + align - 1) / align * align;
        placed |= 1u << l;
    }
    return placed;
}

int build_conv_layouts(const ConvLaunch &layer, unsigned mask, const float *oihw_dev, float *const at[CONV_LAYOUT_COUNT], hipStream_t st) {
    for (int l = 0; l < CONV_LAYOUT_COUNT; l++)
        if (mask >> l & 1) {
            const int r = conv_layout(l).build(layer, oihw_dev, at[l], st);
            if (r != DLPM_OK) return r;
        }
    return DLPM_OK;
}

void attach_conv_layouts(ConvLaunch &c, float *const at[CONV_LAYOUT_COUNT]) {
    for (int l = 0; l < CONV_LAYOUT_COUNT; l++)
        if (at[l] && conv_layout(l).attach) conv_layout(l).attach(c, at[l]);
}

}  // namespace dlpm
