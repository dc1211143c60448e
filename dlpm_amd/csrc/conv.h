// conv.h -- launch descriptors shared by the convolution kernels and the UNet plan.
#pragma once
#include "common.h"

namespace dlpm {

// One conv2d / conv1d(k=1) / Linear launch over NHWC fp32 activations.
struct ConvLaunch {
    const float *src0 = nullptr, *src1 = nullptr;  // virtual channel concat [src0 | src1]
    int C0 = 0, C1 = 0;
    int B = 0, Hin = 0, Win = 0, Hout = 0, Wout = 0;
    int ks = 1, stride = 1, ups = 0;
    const float *w = nullptr;      // igemm: [ks*ks][Cout][Cin]   direct: [ks*ks][Cin][Cout]
    const float *w_frag = nullptr; // optional, 3x3 only: MFMA B-fragment order [n-blocks of 32][Cin/32][9][4][64 lanes][4], padded with zero
                                   // n-blocks to whole BN tiles (see k_conv3x3_halo_ws, frag_weight_floats): each wave streams it straight into registers
    const float *w_wino = nullptr; // optional, 3x3 s1 only: Winograd-domain weights U = G g G^T in fragment order
                                   // (see conv_wino.hip); when the shape qualifies the F(2x2,3x3) kernel runs
    const float *w_wino4 = nullptr;// optional, 3x3 s1 only: F(4x4,3x3) Winograd-domain weights (conv_wino4.hip); preferred over w_wino
    const float *w_wino4_n64 = nullptr, *w_wino4_n32 = nullptr;   // optional, Cout % 128 == 0 only: the same weights in the fragment order of 64- / 32-channel
                                   // n-tiles (round 6: at a small DECLARED batch the narrow shapes give 2-4x as many workgroups; same bits)
    const float *w_wino4sp = nullptr; // optional, ups launches with Cout % 128 == 0 only: the four parity classes' F(4x4,2x2) weights
                                   // (conv_wino4.hip: k_conv3x3_wino4sp); taken where wino4_route says so
    const float *w_wino4_one = nullptr; // optional, 4x4-pixel tensors with Cout % 64 == 0, Cin % 16 == 0 only: the F(4x4,3x3) weights in the fragment
                                   // order of 64-channel n-tiles (conv_wino4.hip: k_conv3x3_wino4_one); taken where wino4_route says so
    const void *w_split = nullptr; // optional: the weights as three bf16 planes in stage-tile order (conv_split.hip); a 3x3 launch
                                   // that carries it is a stride-2 downsampling convolution, or a test forcing the path
    const float *w_small = nullptr;// optional, 3x3 with Cout <= 4 (the head): [tap][Cin][4] for k_conv3x3_head
    const float *w_taps = nullptr; // optional, 3x3 with Cout <= 3 (the head): [9 Cout -> 32][Cin], the head as a 1x1 GEMM + gather (launch_conv_head_gemm)
    const float *w_hfused = nullptr; // optional, the head: W' in MFMA fragment order for the one-pass head + update kernel (head_fused.hip)
    const float *bias = nullptr;   // [Cout] or null
    const float *coefA = nullptr, *coefB = nullptr;  // [B, Cin] fused GroupNorm affine, or null
    int act_silu = 0;
    const float *res0 = nullptr, *res1 = nullptr;    // residual (virtual concat), NHWC at output size
    int R0 = 0;
    float *out = nullptr;
    int Cout = 0;
    int in_nchw = 0, out_nchw = 0;  // boundary layouts
    // Which kernel generation a 3x3 stride-1 launch takes is a function of the LAYER (geometry + this policy), never of the
    // batch the launch happens to carry: the generations round differently, and a sample must not depend on how its batch
    // was sharded or chunked.  gen = DLPM_CONV_AUTO / _F4 / _F2 / _IGEMM (include/dlpm_amd.h); dispatch_B > 0 lets AUTO
    // weigh grid occupancy for a caller-declared batch (a property of the configuration, the same on every rank / chunk).
    int gen = 0;
    int64_t dispatch_B = 0;
    int gemm = 0;                   // DLPM_GEMM_AUTO / _F32 / _BF16X3: which matrix pipe the 1x1 and downsampling convolutions take (conv_split.hip)
    // Round 6, split-K (ConvRoute::ksplit): > 1 = the launch runs `ksplit` copies of its grid, copy s walking the input channels
    // [s Cin / ksplit, (s + 1) Cin / ksplit) and writing its partial outputs to out + s B Hout Wout Cout (bias / residual / statistics
    // are null in such a launch: launch_splitk_reduce adds them).  Taken by the narrow F(4x4) shapes and the F(2x2) kernel only.
    int ksplit = 0;
    // Optional fused GroupNorm statistics of the OUTPUT: per (image, pixel tile, channel) the
    // pair (mean, centred sum of squares) over the tile's pixels, written by the MFMA kernels'
    // epilogue when the tile lies inside one image.  [B][HW/tile][Cout] float2 with tile =
    // conv_route(launch).stats_px: 128 for the implicit-GEMM kernels, 256 for the Winograd kernel
    // (the sub-pixel kernel: one partial per block AND parity class, [B][HW/256][Cout] in (block, class) order, or [B][4 classes][Cout]).
    float2 *stats_out = nullptr;
#ifdef DLPM_PHASE_TIMING
    unsigned long long *phase = nullptr;
#endif
};

// true when the MFMA implicit-GEMM kernel covers this shape (conv_layouts chooses the plain weight layout by it)
bool igemm_supported(const ConvLaunch &c);

// The ONE routing decision of a convolution launch: which kernel family runs it, on what block geometry, and what follows from
// that for the plan (statistics tile, split-K factor, head scratch).  conv_route computes it, launch_conv launches it, the UNet plan
// and dlpm_conv2d_f32 read it -- nobody re-derives a part of it.  Two invariants:
//  * the route is a function of the LAYER and the declared policy (gen, dispatch_B, gemm), never of the batch the launch happens to carry:
//    the generations round differently, and a sample must not depend on how its batch was sharded or chunked;
//  * the single exception is the F(2x2) small-launch shape (conv_wino.hip: wino_small_launch), bit-identical either way.
// Order of the cascade: the head kernels; bf16x3 split; sub-pixel F(4x4); F(4x4) (both also where igemm_supported is false: their input
// channels come in multiples of 8); then, where igemm_supported: F(2x2), the implicit-GEMM kernels; otherwise the stem or the direct kernel.
enum ConvFamily { CONV_HEAD_FUSED, CONV_HEAD_GEMM, CONV_HEAD, CONV_SPLIT, CONV_WINO4SP, CONV_WINO4, CONV_WINO, CONV_IGEMM, CONV_STEM, CONV_DIRECT };
struct ConvRoute {
    ConvFamily family = CONV_DIRECT;
    int bh = 0, bw = 0, nimg = 0;   // Winograd families: tiles per block (rows, columns), images per block
    int nq = 0;                     // Winograd families: n-tile width in channels
    int one = 0;                    // CONV_WINO4 only: 1 = the one-tile shape (16 whole 4x4 images x 64 channels, K split in-block: k_conv3x3_wino4_one)
    int64_t grid = 0;               // Winograd families under a declared batch: workgroups at dispatch_B (what AUTO and split-K weigh)
    int stats_px = 0;               // pixels behind one stats_out partial (0: the kernel that will run cannot emit statistics)
    int ksplit = 1;                 // split-K factor (1: none), see ConvLaunch::ksplit
    int64_t scratch_floats = 0;     // CONV_HEAD_GEMM: the tap-channel tensor launch_conv wants as head_scratch
    char name[96] = "";             // profiler class of the MFMA families (the VALU launchers -- heads, stem, direct -- name their own scope)
    bool head() const { return family <= CONV_HEAD; }
};
ConvRoute conv_route(const ConvLaunch &c);
struct HeadUpdate;
// computes the route and launches it; hu: the sampler's update in the head's epilogue (head families only); head_scratch: see scratch_floats
int launch_conv(const ConvLaunch &c, const HeadUpdate *hu, float *head_scratch, hipStream_t st);
int launch_conv_direct(const ConvLaunch &c, hipStream_t st);
int launch_conv_stem(const ConvLaunch &c, hipStream_t st);
// head convolution (Cout <= 4) as a VALU kernel (conv_direct.hip), optionally with the sampler's reverse update fused into
// its epilogue: x <- (x - c_eps[t,b] eps) / g[t] + c_noise[t,b] z on the NCHW state the eps would have been subtracted from
struct HeadUpdate {
    float *x = nullptr;                 // [B, Cout*H*W] state, updated in place (null: plain convolution, eps -> ConvLaunch::out)
    const float *z = nullptr;           // injected normals, or null = in-kernel Philox (update_step.h)
    const int32_t *t = nullptr;         // device step counter
    const float *g = nullptr, *c_eps = nullptr, *c_noise = nullptr;   // [T], [T,B], [T,B]
    const uint64_t *key = nullptr;      // optional device {seed, sample_offset}
    uint64_t seed = 0;
    int64_t sample_offset = 0;
    float *const *hist_pp = nullptr;    // optional history cell (dlpm_update_args::hist_pp)
    float *eps_out = nullptr;           // optional: also keep eps
    int32_t T = 0;
    int64_t B = 0;
};
bool head_conv_ok(const ConvLaunch &c);
int launch_conv_head(const ConvLaunch &c, const HeadUpdate *hu, hipStream_t st);
int relayout_weight_head(const float *oihw_dev, float *dst_dev, int Cout, int Cin, hipStream_t st);
// the head as a 1x1 GEMM onto 9 Cout (padded to 32) tap channels + a 9-point gather that also carries the update (conv_direct.hip);
// P = scratch of head_gemm_scratch_floats(c) floats
bool head_gemm_ok(const ConvLaunch &c);
int head_taps_rows(int Cout);
int64_t head_gemm_scratch_floats(const ConvLaunch &c);
int launch_conv_head_gemm(const ConvLaunch &c, const HeadUpdate *hu, float *P, hipStream_t st);
int relayout_weight_head_taps(const float *oihw_dev, float *dst_dev, int Cout, int Cin, hipStream_t st);
// the head and the reverse update in ONE pass over HBM (head_fused.hip): the tap-channel tensor stays in LDS
bool head_fused_ok(const ConvLaunch &c);
int64_t head_fused_weight_floats(int Cin);
int relayout_weight_head_fused(const float *oihw_dev, float *dst_dev, int Cout, int Cin, hipStream_t st);
int launch_conv_head_fused(const ConvLaunch &c, const HeadUpdate *hu, hipStream_t st);
// Winograd F(2x2,3x3) path (conv_wino.hip); wino_route: geometry -> r (family CONV_WINO), false where the kernel does not take the launch
bool wino_route(const ConvLaunch &c, ConvRoute *r);
int launch_conv_wino(const ConvLaunch &c, const ConvRoute &r, hipStream_t st);
int64_t wino_weight_floats(int Cout, int Cin);
int relayout_weight_wino(const float *oihw_dev, float *dst_dev, int Cout, int Cin, hipStream_t st);
// Winograd F(4x4,3x3) path (conv_wino4.hip): 16 tiles of 4x4 outputs x 128 channels per workgroup
bool wino4_enabled();                  // DLPM_WINO_F4
bool wino4_route(const ConvLaunch &c, ConvRoute *r);   // geometry + dispatch policy -> r (family CONV_WINO4 or CONV_WINO4SP), false where neither takes the launch
int launch_conv_wino4(const ConvLaunch &c, const ConvRoute &r, hipStream_t st);
int64_t wino4_weight_floats(int Cout, int Cin);
int relayout_weight_wino4(const float *oihw_dev, float *dst_dev, int Cout, int Cin, hipStream_t st, int nq = 0);   // nq: n-tile width (0: the layer's own)
// the nearest-x2 Upsample convolutions as four parity-class F(4x4,2x2) convolutions on the low-res image (conv_wino4.hip: k_conv3x3_wino4sp)
bool wino4sp_enabled();                // DLPM_WINO4_SUBPIX
bool wino4sp_layer_ok(int Cout, int Cin, int Hlo, int Wlo);               // worth building the weights for
int launch_conv_wino4sp(const ConvLaunch &c, const ConvRoute &r, hipStream_t st);
int64_t wino4sp_weight_floats(int Cout, int Cin);
int relayout_weight_wino4sp(const float *oihw_dev, float *dst_dev, int Cout, int Cin, hipStream_t st);
// 4x4-pixel tensors (one F(4x4) tile per image) on 16-image x 64-channel blocks with the K loop split over two groups of four waves
// (conv_wino4.hip: k_conv3x3_wino4_one); weights: relayout_weight_wino4(.., nq = 64), wino4_weight_floats
bool wino4_one_enabled();              // DLPM_WINO4_ONE
bool wino4_one_layer_ok(int Cout, int C0, int C1, int H, int W);           // worth building the weights for
// A WHOLE ResBlock with 32 output channels on 32x32 images in one launch (round 6, conv_wino4.hip: k_resblock_wino4_img): GroupNorm-1
// coefficients from the producers' statistics (or given), conv1 as F(4x4,3x3), GroupNorm-2 with scale-shift inside the workgroup (an image
// is one workgroup), conv2 over the activated intermediate (which makes one trip through L2, never a second launch), skip, output
// statistics.  The 1x1 skip convolution of the concat blocks stays a launch of its own (its result arrives as `res`).
struct ResImgLaunch {
    const float *x0 = nullptr, *x1 = nullptr;        // NHWC input, virtual concat [x0 | x1]
    int C0 = 0, C1 = 0, B = 0;
    int H = 32;                                      // 32: 32 output channels on 32x32 images (k_resblock_wino4_img); 16: 64 output channels on 16x16
                                                     // images (k_resblock_wino4_img16: the intermediate stays in LDS, hbuf unused, stats_out = [B][64])
    const float2 *st0 = nullptr, *st1 = nullptr;     // producers' statistics ([B][nt][C] float2) -> GroupNorm-1 inside the kernel, or
    int nt0 = 1, nt1 = 1;
    const float *coefA1 = nullptr, *coefB1 = nullptr;   // ... its coefficients [B][Cin] computed by a launch in front (sources without statistics)
    const float *gn1_w = nullptr, *gn1_b = nullptr, *gn2_w = nullptr, *gn2_b = nullptr;
    const float *w1 = nullptr, *b1 = nullptr;        // in_layers.2 (3x3, Cin -> 32): F(4x4) fragment stream (relayout_weight_wino4)
    const float *w2 = nullptr, *b2 = nullptr;        // out_layers.3 (3x3, 32 -> 32)
    const float *emb = nullptr;                      // emb_layers output rows: scale at [emb_off + c], shift at [emb_off + 32 + c]
    int64_t emb_stride = 0;
    int emb_off = 0;
    const float *res = nullptr;                      // [B][1024][32]: x itself (identity skip) or the 1x1 skip convolution's output
    float *hbuf = nullptr;                           // [B][1024][32] scratch: silu(GN2(conv1(..)) (1 + scale) + shift)
    float *out = nullptr;                            // [B][1024][32]
    float2 *stats_out = nullptr;                     // optional [B][4][32]: (mean, M2) per 256-pixel quadrant, as the convolution kernels emit
#ifdef DLPM_PHASE_TIMING
    unsigned long long *phase = nullptr;
#endif
};
bool res_img_ok(const ResImgLaunch &r);
int launch_resblock_img(const ResImgLaunch &r, hipStream_t st);

// 1x1 convolutions, and 3x3 ones as an implicit GEMM, on the bf16 matrix pipe with fp32 operands split exactly into three
// bf16 planes (conv_split.hip); taps = 1 or 9
bool conv_split_ok(const ConvLaunch &c);
int launch_conv_split(const ConvLaunch &c, hipStream_t st);
int64_t split_weight_floats(int Cout, int Cin, int taps);
int relayout_weight_split(const float *oihw_dev, void *dst_dev, int Cout, int Cin, int taps, hipStream_t st);
// The weight layouts of a convolution layer: ONE table (conv_layouts.hip) with a row per layout -- its name, its size in floats for a
// layer, the call that builds it from the OIHW parameter, the ConvLaunch field that receives it -- and ONE rule, conv_layouts, for which
// layouts a layer gets.  The UNet's finalize / set_conv_policy, dlpm_conv_policy_f32 and dlpm_conv2d_f32 all place, build and attach
// through it; the *_weight_floats and relayout_weight_* functions of the kernel files are what the rows call.  The order of the enum is
// the order in which layouts are placed in a scratch buffer.
enum ConvLayout {
    LAY_PLAIN,          // [tap][Cout][Cin], the implicit GEMM's order (ConvLaunch::w)
    LAY_PLAIN_DIRECT,   // [tap][Cin][Cout], the direct and stem kernels' order (ConvLaunch::w as well: a layer has one of the two, or, as a
                        // 1x1 implicit GEMM, neither -- its [O][I] parameter is that layout already)
    LAY_FRAG, LAY_WINO, LAY_WINO4, LAY_WINO4SP, LAY_WINO4_ONE, LAY_WINO4_N64, LAY_WINO4_N32, LAY_SPLIT, LAY_HEAD, LAY_HEAD_TAPS, LAY_HEAD_FUSED,
    LAY_SMALL,          // fragment order of the fused small-image blocks: no ConvLaunch field, it feeds ResSmallLaunch / AttnSmallLaunch
    CONV_LAYOUT_COUNT
};
constexpr unsigned lay_bit(ConvLayout l) { return 1u << l; }
struct ConvLayoutRow {
    const char *name;
    int64_t (*floats)(const ConvLaunch &layer);
    int (*build)(const ConvLaunch &layer, const float *oihw_dev, float *dst_dev, hipStream_t st);
    void (*attach)(ConvLaunch &c, const float *p);      // null: see LAY_SMALL
};
const ConvLayoutRow &conv_layout(int l);              // the table, by ConvLayout
// The layouts a layer gets, as a mask of lay_bit.  Reads of `layer`: C0, C1, Cout, ks, stride, in_nchw / out_nchw (a boundary or stride-2
// layer gets the fragment copy only), ups with Hin x Win (the low-res size of an Upsample convolution), Hout x Wout (the one-tile copy of
// a layer on 4x4-pixel tensors; 0 x 0: unknown, none), dispatch_B (the narrow F(4x4) copies exist for Cout % 128 == 0 under a declared
// batch of at most NARROW_COPIES_MAX_BATCH), gemm (DLPM_GEMM_F32: the layer stays on the fp32 pipe -- the time MLP and the emb linears --
// and gets neither the bf16x3 planes nor the fused blocks' order).
constexpr int64_t NARROW_COPIES_MAX_BATCH = 512;
unsigned conv_layouts(const ConvLaunch &layer);
// Places the layouts of `mask` one behind the other from base + *used, in the order of the enum, each at a multiple of `align` floats
// from base: at[l] = where layout l goes, *used = the floats from base to the end of the last one (a multiple of `align`).  A layout
// that would end past `cap` floats is left out (at[l] stays as it was).  Returns the mask of the layouts placed.  Nothing is read
// through a pointer.
unsigned place_conv_layouts(const ConvLaunch &layer, unsigned mask, float *base, int64_t align, int64_t cap, float *at[CONV_LAYOUT_COUNT],
                            int64_t *used);
// Builds the layouts of `mask` from the OIHW weights into at[l], in the order of the enum, on `st`
int build_conv_layouts(const ConvLaunch &layer, unsigned mask, const float *oihw_dev, float *const at[CONV_LAYOUT_COUNT], hipStream_t st);
// Points the launch at every layout of at[] that is not null and has a ConvLaunch field
void attach_conv_layouts(ConvLaunch &c, float *const at[CONV_LAYOUT_COUNT]);
// A convolution launch as its route asks for it (conv_splitk.hip): launch_conv where r.ksplit <= 1; otherwise the split-K form -- the launch
// stripped of bias / residual / statistics runs r.ksplit grid copies into part (splitk_partial_floats(c, r) floats, left holding the
// partial outputs), then launch_splitk_reduce forms c.out.  r = conv_route(c).
int64_t splitk_partial_floats(const ConvLaunch &c, const ConvRoute &r);
int launch_conv_splitk(const ConvLaunch &c, const ConvRoute &r, float *part, hipStream_t st);
// out = bias + sum_s part[s] (+ residual [res0 | res1]) over n = B Hout Wout pixels x Cout channels, partials summed in ascending s
int launch_splitk_reduce(const float *part, int S, int64_t npix, int Cout, const float *bias, const float *res0, const float *res1, int R0,
                         float *out, hipStream_t st);
// weight re-layout kernels: OIHW -> [tap][Cout][Cin] (igemm) or [tap][Cin][Cout] (direct)
int relayout_weight(const float *oihw_dev, float *dst_dev, int Cout, int Cin, int ks, bool for_igemm, hipStream_t st);
// OIHW 3x3 -> fragment order for k_conv3x3_halo_ws; dst holds frag_weight_floats(Cout, Cin) floats
int64_t frag_weight_floats(int Cout, int Cin);
int relayout_weight_frag(const float *oihw_dev, float *dst_dev, int Cout, int Cin, hipStream_t st);

int launch_gn_coeffs(const float *src0, const float *src1, int C0, int C1, int B, int HW, int groups,
                     const float *gamma, const float *beta, const float *ss, int64_t ss_stride, int64_t ss_offset,
                     float *coefA, float *coefB, hipStream_t st);
// GroupNorm coefficients from per-tile channel statistics (see ConvLaunch::stats_out) instead of the
// activations: st0/st1 = statistics of the two concat sources, nt0/nt1 = their tiles per image.
int launch_gn_coeffs_from_stats(const float2 *st0, const float2 *st1, int C0, int C1, int B, int nt0, int nt1, int HW, int groups,
                                const float *gamma, const float *beta, const float *ss, int64_t ss_stride,
                                int64_t ss_offset, float *coefA, float *coefB, hipStream_t st);
int launch_attention(const float *qkv, float *out, int B, int T, int C, int heads, hipStream_t st);
int launch_attention_general(const float *qkv, float *out, int B, int T, int C, int heads, hipStream_t st);   // always k_attention_any

// Whole blocks of small images in one launch, activations resident in LDS (block_small.hip): 64-output-channel ResBlocks on
// 8x8 / 4x4 images, one workgroup per image.
struct ResSmallLaunch {
    const float *x0 = nullptr, *x1 = nullptr;   // NHWC input, virtual concat [x0 | x1]
    int C0 = 0, C1 = 0, B = 0, H = 0, W = 0;
    const float *gn1_w = nullptr, *gn1_b = nullptr, *gn2_w = nullptr, *gn2_b = nullptr;
    const float *w1f = nullptr, *b1 = nullptr;   // in_layers.2 (3x3, Cin -> 64), fragment order (relayout_weight_small)
    const float *w2f = nullptr, *b2 = nullptr;   // out_layers.3 (3x3, 64 -> 64)
    const float *wsf = nullptr, *bs = nullptr;   // skip_connection (1x1, Cin -> 64) or null = identity
    const float *emb = nullptr;                  // emb_layers output rows: scale at [emb_off + c], shift at [emb_off + 64 + c]
    int64_t emb_stride = 0;
    int emb_off = 0;
    float *out = nullptr;                        // [B][H W][64]
    float2 *stats_out = nullptr;                 // optional [B][64] (mean, M2) of the output per image and channel
};
struct AttnSmallLaunch {                         // AttentionBlock, 64 channels, 4 heads, 8x8 / 4x4 images
    const float *x = nullptr;                    // [B][H W][64]
    int C = 0, heads = 0, B = 0, H = 0, W = 0;
    const float *gn_w = nullptr, *gn_b = nullptr;
    const float *wqkv = nullptr, *bqkv = nullptr;    // qkv (1x1, 64 -> 192), fragment order
    const float *wproj = nullptr, *bproj = nullptr;  // proj_out (1x1, 64 -> 64), fragment order
    float *out = nullptr;
    float2 *stats_out = nullptr;
#ifdef DLPM_PHASE_TIMING
    unsigned long long *phase = nullptr;
#endif
};
bool attn_small_ok(const AttnSmallLaunch &a);
int launch_attnblock_small(const AttnSmallLaunch &a, hipStream_t st);
bool attn16_ok(const AttnSmallLaunch &a);        // 16x16 images (round 6): the whole block, one head at a time
int launch_attnblock16(const AttnSmallLaunch &a, hipStream_t st);
bool gnqkv_small_ok(const AttnSmallLaunch &a);   // 16x16 images: GroupNorm + qkv only, out = qkv [B][256][192]
int launch_gnqkv_small(const AttnSmallLaunch &a, hipStream_t st);
bool small_blocks_enabled();                     // DLPM_NO_FUSED_BLOCKS
bool small_weight_ok(int Cout, int Cin, int ks);
int64_t small_weight_floats(int Cout, int Cin, int ks);
int relayout_weight_small(const float *oihw_dev, float *dst_dev, int Cout, int Cin, int ks, hipStream_t st);
bool res_small_ok(const ResSmallLaunch &r);
int launch_resblock_small(const ResSmallLaunch &r, hipStream_t st);
int launch_timestep_embedding(const float *t, float *emb, int64_t B, int dim, hipStream_t st);
// out[b] = src[row(b)] + w[y[b]] over `dim` columns (embed.hip): row(b) = (row_dev ? *row_dev : 0) + b * src_row_stride; a label
// outside [0, K) gives a NaN row and no read of w
int launch_label_embedding_add(const float *src, const int32_t *row_dev, int src_row_stride, const float *w, const int64_t *y, int64_t K,
                               int64_t B, int dim, float *out, hipStream_t st);

__device__ __forceinline__ float silu_f(float v) {
    // x * sigmoid(x), sigmoid = 1/(1+exp(-x))  (nn.py:12-14).  v_exp_f32 + v_rcp_f32 (1 ulp each): the IEEE
    // division sequence costs ~10 instructions per element and this runs once per staged activation.
    return v * __builtin_amdgcn_rcpf(1.0f + __expf(-v));
}

}  // namespace dlpm
