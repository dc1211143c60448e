// unet.hip -- the improved-DDPM UNet score network as a launch plan over the HIP kernels.
//
// Replaces UNetModel.forward and its blocks (dlpm/models/unet.py:33-250,276-492) for the
// constructor arguments of _unet_model (dlpm/dlpm_experiment.py:38-56: use_scale_shift_norm=True,
// dims=2, no class conditioning, conv_resample=True).  Weights arrive under the reference's
// state_dict keys, so reference checkpoints load unchanged.
//
// Data layout in HBM: activations NHWC fp32 in a caller-provided workspace, handed out by an arena
// that recycles every buffer after its last consumer has been enqueued (skip-connection tensors live
// until their output block); the (B,C,H,W) boundary tensors are read/written in place by the
// stem/head kernels.  Fusions:
//   GroupNorm(+scale-shift)+SiLU  -> coefficient kernel + the consumer conv's tile staging
//   cat([h, skip])                -> two-pointer reads in the conv / GroupNorm kernels
//   nearest upsample              -> index arithmetic in the conv
//   bias, residual add            -> conv epilogue
//   22 per-ResBlock Linear(4mc -> 2C) -> one GEMM against the row-concatenated weights
#include <cmath>
#include <cstdlib>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "conv.h"
#include "../../include/dlpm_amd_chains.h"
#include "../../include/dlpm_amd_conv.h"

using namespace dlpm;

namespace {

struct Param {
    std::string key;
    int64_t numel = 0;
    float *dev = nullptr;   // reference layout
    bool set = false;
};

enum LayerKind { L_STEM, L_RES, L_ATTN, L_DOWN, L_UP };

struct ConvW {            // one convolution's weights
    int p_w = -1, p_b = -1;  // param indices (p_w < 0: the stacked emb linears, dlpm_unet::embcat_w)
    int cout = 0, cin = 0, ks = 1;
    ConvLaunch layer;        // the layer as conv_layouts (conv.h) is asked about it: what dlpm_unet_finalize describes, under the declared batch
    float *lay[CONV_LAYOUT_COUNT] = {};   // the device copies of the weights this convolution owns, by ConvLayout (sync_layouts)
};

struct Layer {
    LayerKind kind;
    std::string pre;
    int cin = 0, cout = 0;       // RES: cin = total input channels
    int emb_off = 0;             // RES: column offset into the fused emb GEMM output
    ConvW c1, c2, skip;          // RES: in conv, out conv, 1x1 skip | ATTN: c1 = qkv, c2 = proj | STEM/DOWN/UP: c1
    bool has_skip = false;
    int p_gn1_w = -1, p_gn1_b = -1, p_gn2_w = -1, p_gn2_b = -1;
    int p_emb_w = -1, p_emb_b = -1;
};

struct Tensor4 {
    float *p = nullptr;
    int C = 0, H = 0, W = 0;
    float2 *stats = nullptr;  // per (image, pixel tile, channel) (mean, M2) emitted by the producing conv, or null
    int stats_px = 0;         // pixels per tile of `stats` (128: implicit-GEMM kernels, 256: Winograd kernel)
};

// Activation arena: a first-fit free list over the caller's workspace.  Launches are stream-ordered, so a buffer can be
// handed out again as soon as every launch that touches it has been ENQUEUED; the plan releases each tensor right after
// its last consumer (skip-connection tensors when their output block pops them).  A dry run (no base pointer: offsets
// from a fake base, never dereferenced) runs the same walk with every launch suppressed to size the workspace = the peak.  A real
// walk that outgrows the caller's workspace sets `overflow`, and from then on nothing is enqueued (Ctx: PLAN_ENQUEUES).
struct Bump {
    char *base = nullptr;
    int64_t cap = 0, off = 0, peak = 0, nalloc = 0;
    bool dry = false, overflow = false, reuse = true;
    std::vector<std::pair<int64_t, int64_t>> holes;     // (offset, bytes), sorted by offset, coalesced
    std::map<int64_t, int64_t> live;                    // offset -> bytes
    char *origin() const { return dry ? reinterpret_cast<char *>(uintptr_t(1) << 20) : base; }
    float *alloc(int64_t nfloats) {
        const int64_t bytes = (nfloats * 4 + 255) / 256 * 256;
        int64_t at = -1;
        nalloc++;
        if (reuse) {
            size_t best = holes.size();                  // best fit: the smallest hole that holds the request
            for (size_t i = 0; i < holes.size(); i++)
                if (holes[i].second >= bytes && (best == holes.size() || holes[i].second < holes[best].second)) best = i;
            if (best != holes.size()) {
                at = holes[best].first;
                if (holes[best].second == bytes) holes.erase(holes.begin() + best);
                else { holes[best].first += bytes; holes[best].second -= bytes; }
            }
        }
        if (at < 0) {
            at = off;
            off += bytes;
            if (off > peak) peak = off;
            if (!dry && off > cap) overflow = true;
        }
        live[at] = bytes;
        return reinterpret_cast<float *>(origin() + at);
    }
    void release(const void *p) {
        if (!p || !reuse) return;
        const int64_t at = reinterpret_cast<const char *>(p) - origin();
        auto it = live.find(at);
        if (it == live.end()) return;
        int64_t lo = at, n = it->second;
        live.erase(it);
        size_t i = 0;
        while (i < holes.size() && holes[i].first < lo) i++;
        if (i > 0 && holes[i - 1].first + holes[i - 1].second == lo) { lo = holes[i - 1].first; n += holes[i - 1].second; holes.erase(holes.begin() + --i); }
        if (i < holes.size() && lo + n == holes[i].first) { n += holes[i].second; holes.erase(holes.begin() + i); }
        if (lo + n == off) { off = lo; return; }         // the top of the arena shrinks back
        holes.insert(holes.begin() + i, std::make_pair(lo, n));
    }
};

void drop(Bump &ws, Tensor4 &t) {   // release a tensor and the statistics that ride with it
    ws.release(t.p);
    ws.release(t.stats);
    t.p = nullptr;
    t.stats = nullptr;
}

}  // namespace

struct dlpm_unet {
    dlpm_unet_config cfg;
    std::vector<Param> params;
    std::map<std::string, int> index;
    std::vector<std::vector<Layer>> in_blocks, out_blocks;
    std::vector<Layer> mid;
    std::vector<int> skip_ch;        // channels pushed by each input block
    ConvW te0, te2, embcat, head;
    int p_head_gn_w = -1, p_head_gn_b = -1;
    float *embcat_w = nullptr, *embcat_b = nullptr;
    int emb_total = 0, ted = 0, final_ch = 0;
    int num_classes = 0;             // dlpm_unet_create_conditional: K > 0 adds label_emb.weight [K][ted]
    int p_label = -1;
    bool finalized = false;
    std::vector<Tensor4> feats;      // block outputs of the last forward
    int64_t flops = 0;
    bool keep_feats = false;         // dlpm_unet_keep_features: block outputs stay valid after the forward (no arena reuse)
    int gen = DLPM_CONV_AUTO;        // dlpm_unet_set_conv_policy
    int64_t dispatch_B = 0;
    int gemm = DLPM_GEMM_AUTO;       // dlpm_unet_set_gemm_policy
    int64_t plan_version = 0;

    int add(const std::string &key, int64_t numel) {
        Param p;
        p.key = key;
        p.numel = numel;
        params.push_back(p);
        index[key] = (int)params.size() - 1;
        return (int)params.size() - 1;
    }
    ConvW conv(const std::string &pre, int cout, int cin, int ks) {
        ConvW c;
        c.cout = cout; c.cin = cin; c.ks = ks;
        c.p_w = add(pre + "weight", (int64_t)cout * cin * ks * ks);
        c.p_b = add(pre + "bias", cout);
        return c;
    }
    Layer res(const std::string &pre, int cin, int cout) {
        Layer L;
        L.kind = L_RES; L.pre = pre; L.cin = cin; L.cout = cout;
        L.p_gn1_w = add(pre + "in_layers.0.weight", cin);
        L.p_gn1_b = add(pre + "in_layers.0.bias", cin);
        L.c1 = conv(pre + "in_layers.2.", cout, cin, 3);
        L.p_emb_w = add(pre + "emb_layers.1.weight", (int64_t)2 * cout * ted);
        L.p_emb_b = add(pre + "emb_layers.1.bias", 2 * cout);
        L.p_gn2_w = add(pre + "out_layers.0.weight", cout);
        L.p_gn2_b = add(pre + "out_layers.0.bias", cout);
        L.c2 = conv(pre + "out_layers.3.", cout, cout, 3);
        L.has_skip = cin != cout;
        if (L.has_skip) L.skip = conv(pre + "skip_connection.", cout, cin, 1);
        L.emb_off = emb_total;
        emb_total += 2 * cout;
        return L;
    }
    Layer attn(const std::string &pre, int ch) {
        Layer L;
        L.kind = L_ATTN; L.pre = pre; L.cin = L.cout = ch;
        L.p_gn1_w = add(pre + "norm.weight", ch);
        L.p_gn1_b = add(pre + "norm.bias", ch);
        L.c1 = conv(pre + "qkv.", 3 * ch, ch, 1);
        L.c2 = conv(pre + "proj_out.", ch, ch, 1);
        return L;
    }
    bool has_attn(int ds) const {
        for (int i = 0; i < cfg.n_attn; i++)
            if (cfg.attention_resolutions[i] == ds) return true;
        return false;
    }
};

namespace {

void policy_of(const dlpm_unet *u, ConvLaunch &L) {
    L.gen = u->gen;
    L.dispatch_B = u->dispatch_B;
    L.gemm = u->gemm;
}

// The block structure the reference constructor produces (unet.py:334-436).
void build_arch(dlpm_unet *u) {
    const dlpm_unet_config &c = u->cfg;
    const int mc = c.model_channels;
    u->ted = 4 * mc;
    u->te0 = u->conv("time_embed.0.", u->ted, mc, 1);
    u->te2 = u->conv("time_embed.2.", u->ted, u->ted, 1);
    if (u->num_classes > 0) u->p_label = u->add("label_emb.weight", (int64_t)u->num_classes * u->ted);   // unet.py:341-342
    {
        Layer L;
        L.kind = L_STEM; L.pre = "input_blocks.0.0."; L.cin = c.in_channels; L.cout = mc;
        L.c1 = u->conv(L.pre, mc, c.in_channels, 3);
        u->in_blocks.push_back({L});
        u->skip_ch.push_back(mc);
    }
    int ch = mc, ds = 1;
    for (int level = 0; level < c.n_mult; level++) {
        const int mult = c.channel_mult[level];
        for (int r = 0; r < c.num_res_blocks; r++) {
            const std::string pre = "input_blocks." + std::to_string(u->in_blocks.size()) + ".";
            std::vector<Layer> seq;
            seq.push_back(u->res(pre + "0.", ch, mult * mc));
            ch = mult * mc;
            if (u->has_attn(ds)) seq.push_back(u->attn(pre + "1.", ch));
            u->in_blocks.push_back(seq);
            u->skip_ch.push_back(ch);
        }
        if (level != c.n_mult - 1) {
            Layer L;
            L.kind = L_DOWN; L.pre = "input_blocks." + std::to_string(u->in_blocks.size()) + ".0.op.";
            L.cin = L.cout = ch;
            L.c1 = u->conv(L.pre, ch, ch, 3);
            u->in_blocks.push_back({L});
            u->skip_ch.push_back(ch);
            ds *= 2;
        }
    }
    u->mid.push_back(u->res("middle_block.0.", ch, ch));
    u->mid.push_back(u->attn("middle_block.1.", ch));
    u->mid.push_back(u->res("middle_block.2.", ch, ch));
    std::vector<int> stack = u->skip_ch;
    for (int level = c.n_mult - 1; level >= 0; level--) {
        const int mult = c.channel_mult[level];
        for (int i = 0; i <= c.num_res_blocks; i++) {
            const std::string pre = "output_blocks." + std::to_string(u->out_blocks.size()) + ".";
            const int ich = stack.back();
            stack.pop_back();
            std::vector<Layer> seq;
            seq.push_back(u->res(pre + "0.", ch + ich, mc * mult));
            ch = mc * mult;
            int k = 1;
            if (u->has_attn(ds)) seq.push_back(u->attn(pre + std::to_string(k++) + ".", ch));
            if (level && i == c.num_res_blocks) {
                Layer L;
                L.kind = L_UP; L.pre = pre + std::to_string(k++) + ".conv.";
                L.cin = L.cout = ch;
                L.c1 = u->conv(L.pre, ch, ch, 3);
                seq.push_back(L);
                ds /= 2;
            }
            u->out_blocks.push_back(seq);
        }
    }
    u->final_ch = ch;
    u->p_head_gn_w = u->add("out.0.weight", ch);
    u->p_head_gn_b = u->add("out.0.bias", ch);
    u->head = u->conv("out.2.", c.out_channels, mc, 3);
}

const float *oihw_of(const dlpm_unet *u, const ConvW &c) { return c.p_w >= 0 ? u->params[c.p_w].dev : u->embcat_w; }

// the launch descriptor with the net's policy and this convolution's weight layouts attached: the ONE place a ConvW is copied into a launch
void attach_conv(const dlpm_unet *u, const ConvW &c, ConvLaunch &L) {
    policy_of(u, L);
    L.w = oihw_of(u, c);       // (a 1x1 implicit GEMM owns no plain copy: its [O][I] parameter is that layout)
    attach_conv_layouts(L, c.lay);
    L.ks = c.ks;
    L.Cout = c.cout;
}

int run_conv(const dlpm_unet *u, const ConvW &c, ConvLaunch L, hipStream_t st, const HeadUpdate *hu = nullptr, float *head_scratch = nullptr) {
    attach_conv(u, c, L);      // (the time path describes its launches by hand; a descriptor from conv_io carries the same values already)
    return launch_conv(L, hu, head_scratch, st);
}

#define TRY(expr)                  \
    do {                           \
        int _r = (expr);           \
        if (_r != DLPM_OK) return _r; \
    } while (0)

struct Ctx {
    dlpm_unet *u;
    int B;
    Bump ws;
    hipStream_t st;
    float *embout = nullptr;
    bool uniform_t = false;      // every sample has the same timestep: the time MLP and the emb linears run on ONE row
    const int64_t *y = nullptr;  // class labels [B] (int64) of a conditional net: B emb rows whatever uniform_t says
    // row pitch of the per-ResBlock scale/shift rows: 0 when all samples read the one row of a uniform-t unconditional forward
    int64_t emb_pitch() const { return (uniform_t && !y) ? 0 : u->emb_total; }
    const HeadUpdate *hu = nullptr;   // the sampler's reverse update, fused into the head convolution (dlpm_unet_forward_update)
    bool dry() const { return ws.dry; }
};

// ONE walk sizes the workspace and launches the plan: the code below allocates, releases and describes its launches the same way in both
// modes, and everything it enqueues goes through a helper that opens with PLAN_ENQUEUES.  A dry run enqueues nothing.  A real walk
// whose arena has outgrown the caller's workspace -- it asked for more than the dry run did -- refuses instead of writing past the end.
int arena_overflow(const Ctx &cx) {
    set_error("unet plan: the walk at batch %d asked the arena for %lld bytes, past the workspace of %lld bytes that dlpm_unet_workspace_bytes sized",
              cx.B, (long long)cx.ws.peak, (long long)cx.ws.cap);
    return DLPM_ERR_NOMEM;
}
#define PLAN_ENQUEUES(cx)                                   \
    do {                                                    \
        if ((cx).dry()) return DLPM_OK;                     \
        if ((cx).ws.overflow) return arena_overflow(cx);    \
    } while (0)

// any launch_* function of conv.h that takes its stream last
template <class Fn, class... A>
int enqueue(Ctx &cx, Fn launch, const A &...a) {
    PLAN_ENQUEUES(cx);
    return launch(a..., cx.st);
}

int run_conv(Ctx &cx, const ConvW &c, const ConvLaunch &L, const HeadUpdate *hu = nullptr, float *head_scratch = nullptr) {
    PLAN_ENQUEUES(cx);
    return run_conv(cx.u, c, L, cx.st, hu, head_scratch);
}

Tensor4 new_tensor(Ctx &cx, int C, int H, int W) {
    Tensor4 t;
    t.C = C; t.H = H; t.W = W;
    t.p = cx.ws.alloc((int64_t)cx.B * H * W * C);
    return t;
}

// The launch of convolution `c` of the plan on [x0 | x1] -> o, the descriptor the plan asks the selectors about AND runs: layouts, policy,
// sources, batch, bias, output, and the geometry the two sizes give (same size; a smaller output is the stride-2 downsampling convolution, a
// larger one the nearest x2 upsample).  The call site adds what the layer fuses: GroupNorm coefficients, SiLU, residual, a boundary layout.
ConvLaunch conv_io(const Ctx &cx, const ConvW &c, const Tensor4 &x0, const Tensor4 &x1, const Tensor4 &o) {
    ConvLaunch L;
    attach_conv(cx.u, c, L);
    L.src0 = x0.p; L.src1 = x1.p; L.C0 = x0.C; L.C1 = x1.C; L.B = cx.B;
    L.Hin = x0.H; L.Win = x0.W; L.Hout = o.H; L.Wout = o.W;
    L.stride = o.H < x0.H ? 2 : 1; L.ups = o.H > x0.H ? 1 : 0;
    L.bias = cx.u->params[c.p_b].dev; L.out = o.p;
    return L;
}

// GroupNorm statistics can ride on the producing conv's epilogue when its pixel tiles stay inside one image and the conv runs on the
// MFMA kernels with the row epilogue (or the stem kernels).  Decides whether `t`, the output of launch `L`, carries statistics,
// allocates them (tile size per the route of the launch itself) and points the launch at them.
void plan_stats(Ctx &cx, Tensor4 &t, ConvLaunch &L) {
    static const int off = env_switch("DLPM_NO_GN_FUSION", 0, true);
    t.stats = nullptr;
    t.stats_px = 0;
    const int px = off ? 0 : conv_route(L).stats_px;
    if (px <= 0) return;
    t.stats_px = px;
    t.stats = L.stats_out = reinterpret_cast<float2 *>(cx.ws.alloc((int64_t)2 * cx.B * (t.H * t.W / px) * t.C));
}

// GroupNorm(+scale/shift from the emb rows at column ss_offset) coefficients of the virtual concat [x0 | x1], from the producers' statistics where both carry them
int gn_any(Ctx &cx, Tensor4 x0, Tensor4 x1, int p_gamma, int p_beta, const float *ss, int64_t ss_offset, float *cA, float *cB) {
    PLAN_ENQUEUES(cx);
    const int HW = x0.H * x0.W, C = x0.C + x1.C, groups = C < 32 ? C : 32;
    const float *gamma = cx.u->params[p_gamma].dev, *beta = cx.u->params[p_beta].dev;
    const int64_t ss_stride = ss ? cx.emb_pitch() : 0;   // row pitch 0: all samples read the one emb row
    if (x0.stats && (x1.C == 0 || x1.stats))
        return launch_gn_coeffs_from_stats(x0.stats, x1.stats, x0.C, x1.C, cx.B, HW / x0.stats_px, x1.C ? HW / x1.stats_px : 1, HW,
                                           groups, gamma, beta, ss, ss_stride, ss_offset, cA, cB, cx.st);
    return launch_gn_coeffs(x0.p, x1.p, x0.C, x1.C, cx.B, HW, groups, gamma, beta, ss, ss_stride, ss_offset, cA, cB, cx.st);
}

// A 3x3 stride-1 convolution of the plan, cut over S = ConvRoute::ksplit grid copies where the layer and the declared batch ask for it
// (conv_splitk.hip: launch_conv_splitk, the one definition of that launch): the copies write their partial outputs into an arena buffer,
// launch_splitk_reduce adds bias / residual.  L comes from conv_io, layouts and policy attached.
int run_conv3(Ctx &cx, const ConvW &c, const ConvLaunch &L) {
    const ConvRoute r = conv_route(L);
    if (r.ksplit <= 1) return run_conv(cx, c, L);
    float *part = cx.ws.alloc(splitk_partial_floats(L, r));
    const int rc = enqueue(cx, launch_conv_splitk, L, r, part);
    cx.ws.release(part);
    return rc;
}

// The whole-image ResBlock kernel reads its residual as ONE tensor of Cout channels per pixel: the skip convolution's output, or an input
// that is not a concat (an identity residual over [x0 | x1] would be read from x0 with the wrong pitch).  run_res and dlpm_resblock_img_f32 ask.
bool res_img_residual_ok(bool has_skip, int C1) { return has_skip || C1 == 0; }

int run_res(Ctx &cx, const Layer &L, Tensor4 x0, Tensor4 x1, Tensor4 *out) {
    dlpm_unet *u = cx.u;
    const int B = cx.B, H = x0.H, W = x0.W, HW = H * W;
    const int C0 = x0.C, C1 = x1.C, Cin = C0 + C1, Co = L.cout;
    {
        // small images, 64 channels: the whole block in one launch (block_small.hip).  A function of the layer and of the net's
        // policy only -- never of the batch -- like every other kernel choice (the fused block rounds differently).
        ResSmallLaunch r;
        r.x0 = x0.p; r.x1 = x1.p; r.C0 = C0; r.C1 = C1; r.B = B; r.H = H; r.W = W;
        r.w1f = L.c1.lay[LAY_SMALL]; r.w2f = L.c2.lay[LAY_SMALL]; r.wsf = L.has_skip ? L.skip.lay[LAY_SMALL] : nullptr;
        if (u->gen == DLPM_CONV_AUTO && Co == 64 && (!L.has_skip || r.wsf) && res_small_ok(r)) {
            *out = new_tensor(cx, Co, H, W);
            out->stats = reinterpret_cast<float2 *>(cx.ws.alloc((int64_t)2 * B * Co));
            out->stats_px = HW;
            r.gn1_w = u->params[L.p_gn1_w].dev; r.gn1_b = u->params[L.p_gn1_b].dev;
            r.gn2_w = u->params[L.p_gn2_w].dev; r.gn2_b = u->params[L.p_gn2_b].dev;
            r.b1 = u->params[L.c1.p_b].dev; r.b2 = u->params[L.c2.p_b].dev;
            r.bs = L.has_skip ? u->params[L.skip.p_b].dev : nullptr;
            r.emb = cx.embout; r.emb_stride = cx.emb_pitch(); r.emb_off = L.emb_off;
            r.out = out->p; r.stats_out = out->stats;
            return enqueue(cx, launch_resblock_small, r);
        }
    }
    if (u->gen == DLPM_CONV_AUTO && ((Co == 32 && H == 32 && W == 32) || (Co == 64 && H == 16 && W == 16)) && L.c1.lay[LAY_WINO4] && L.c2.lay[LAY_WINO4]) {
        // 32 channels on 32x32 images: the whole block in ONE launch, one workgroup per image (conv_wino4.hip: k_resblock_wino4_img) -- the
        // bits of the separate launches below (a function of the layer and the policy only).  GroupNorm-1 runs inside the kernel when both
        // sources carry statistics; the 1x1 skip convolution of the concat blocks stays a launch of its own.
        // 64 channels on 16x16 images likewise (k_resblock_wino4_img16: the intermediate stays in LDS; it rounds differently from the launches below).
        ResImgLaunch r;
        r.x0 = x0.p; r.x1 = x1.p; r.C0 = C0; r.C1 = C1; r.B = B; r.H = H;
        const bool from_stats = x0.stats && (C1 == 0 || x1.stats);
        r.w1 = L.c1.lay[LAY_WINO4]; r.w2 = L.c2.lay[LAY_WINO4];
        float *cA1 = from_stats ? nullptr : cx.ws.alloc((int64_t)B * Cin), *cB1 = from_stats ? nullptr : cx.ws.alloc((int64_t)B * Cin);
        Tensor4 sk = L.has_skip ? new_tensor(cx, Co, H, W) : Tensor4();
        Tensor4 hb = H == 32 ? new_tensor(cx, Co, H, W) : Tensor4();     // the activated intermediate (it stays in LDS at 16x16)
        Tensor4 o = new_tensor(cx, Co, H, W);
        r.hbuf = hb.p; r.res = L.has_skip ? sk.p : x0.p;
        if (from_stats) {
            r.st0 = x0.stats; r.nt0 = HW / x0.stats_px;
            if (C1) { r.st1 = x1.stats; r.nt1 = HW / x1.stats_px; }
        } else {
            r.coefA1 = cA1; r.coefB1 = cB1;
        }
        const bool take = res_img_residual_ok(L.has_skip, C1) && res_img_ok(r);
        if (take) {
            *out = o;
            hb.C = Co; hb.H = H; hb.W = W;
            ConvLaunch b = conv_io(cx, L.c2, hb, Tensor4(), o);     // the kernel emits the output statistics that conv2's own launch would
            plan_stats(cx, *out, b);
            if (!from_stats) TRY(gn_any(cx, x0, x1, L.p_gn1_w, L.p_gn1_b, nullptr, 0, cA1, cB1));
            if (L.has_skip) TRY(run_conv(cx, L.skip, conv_io(cx, L.skip, x0, x1, sk)));
            r.gn1_w = u->params[L.p_gn1_w].dev; r.gn1_b = u->params[L.p_gn1_b].dev;
            r.gn2_w = u->params[L.p_gn2_w].dev; r.gn2_b = u->params[L.p_gn2_b].dev;
            r.b1 = u->params[L.c1.p_b].dev; r.b2 = u->params[L.c2.p_b].dev;
            r.emb = cx.embout; r.emb_stride = cx.emb_pitch(); r.emb_off = L.emb_off;
            r.out = o.p; r.stats_out = out->stats;
            TRY(enqueue(cx, launch_resblock_img, r));
        }
        cx.ws.release(cA1); cx.ws.release(cB1); cx.ws.release(sk.p); cx.ws.release(hb.p);
        if (take) return DLPM_OK;
        cx.ws.release(o.p);
    }
    float *cA1 = cx.ws.alloc((int64_t)B * Cin), *cB1 = cx.ws.alloc((int64_t)B * Cin);
    Tensor4 h1 = new_tensor(cx, Co, H, W);
    ConvLaunch a = conv_io(cx, L.c1, x0, x1, h1);
    a.coefA = cA1; a.coefB = cB1; a.act_silu = 1;
    plan_stats(cx, h1, a);
    float *cA2 = cx.ws.alloc((int64_t)B * Co), *cB2 = cx.ws.alloc((int64_t)B * Co);
    Tensor4 sk = L.has_skip ? new_tensor(cx, Co, H, W) : Tensor4();
    *out = new_tensor(cx, Co, H, W);
    ConvLaunch b = conv_io(cx, L.c2, h1, Tensor4(), *out);
    b.coefA = cA2; b.coefB = cB2; b.act_silu = 1;
    if (L.has_skip) { b.res0 = sk.p; b.R0 = Co; }
    else { b.res0 = x0.p; b.res1 = x1.p; b.R0 = C0; }
    plan_stats(cx, *out, b);
    TRY(gn_any(cx, x0, x1, L.p_gn1_w, L.p_gn1_b, nullptr, 0, cA1, cB1));
    TRY(run_conv3(cx, L.c1, a));
    TRY(gn_any(cx, h1, Tensor4(), L.p_gn2_w, L.p_gn2_b, cx.embout, L.emb_off, cA2, cB2));
    if (L.has_skip) TRY(run_conv(cx, L.skip, conv_io(cx, L.skip, x0, x1, sk)));
    TRY(run_conv3(cx, L.c2, b));
    cx.ws.release(cA1);
    cx.ws.release(cB1);
    drop(cx.ws, h1);
    cx.ws.release(cA2);
    cx.ws.release(cB2);
    cx.ws.release(sk.p);
    return DLPM_OK;
}

int run_attn(Ctx &cx, const Layer &L, Tensor4 x, Tensor4 *out) {
    dlpm_unet *u = cx.u;
    const int B = cx.B, C = x.C, T = x.H * x.W;
    // small images: GroupNorm -> qkv -> attention -> proj -> + x in one launch, one workgroup per image (block_small.hip); 16x16 images
    // that do not take it: GroupNorm + qkv of one image in one launch
    AttnSmallLaunch a;
    a.x = x.p; a.C = C; a.heads = u->cfg.num_heads; a.B = B; a.H = x.H; a.W = x.W;
    a.wqkv = L.c1.lay[LAY_SMALL]; a.wproj = L.c2.lay[LAY_SMALL];
    a.gn_w = u->params[L.p_gn1_w].dev; a.gn_b = u->params[L.p_gn1_b].dev;
    a.bqkv = u->params[L.c1.p_b].dev; a.bproj = u->params[L.c2.p_b].dev;
    const bool whole16 = attn16_ok(a);
    if (u->gen == DLPM_CONV_AUTO && (attn_small_ok(a) || whole16)) {
        *out = new_tensor(cx, C, x.H, x.W);
        out->stats = reinterpret_cast<float2 *>(cx.ws.alloc((int64_t)2 * B * C));
        out->stats_px = T;
        a.out = out->p; a.stats_out = out->stats;
        return enqueue(cx, whole16 ? launch_attnblock16 : launch_attnblock_small, a);
    }
    float *cA = cx.ws.alloc((int64_t)B * C), *cB = cx.ws.alloc((int64_t)B * C);
    Tensor4 qkv = new_tensor(cx, 3 * C, x.H, x.W), av = new_tensor(cx, C, x.H, x.W);
    *out = new_tensor(cx, C, x.H, x.W);
    ConvLaunch p = conv_io(cx, L.c2, av, Tensor4(), *out);
    p.res0 = x.p; p.R0 = C;
    plan_stats(cx, *out, p);
    a.wproj = nullptr; a.bproj = nullptr; a.out = qkv.p;
    if (u->gen == DLPM_CONV_AUTO && gnqkv_small_ok(a)) {
        TRY(enqueue(cx, launch_gnqkv_small, a));
    } else {
        TRY(gn_any(cx, x, Tensor4(), L.p_gn1_w, L.p_gn1_b, nullptr, 0, cA, cB));
        ConvLaunch q = conv_io(cx, L.c1, x, Tensor4(), qkv);
        q.coefA = cA; q.coefB = cB;
        TRY(run_conv(cx, L.c1, q));
    }
    TRY(enqueue(cx, launch_attention, qkv.p, av.p, B, T, C, u->cfg.num_heads));
    TRY(run_conv(cx, L.c2, p));
    cx.ws.release(cA);
    cx.ws.release(cB);
    cx.ws.release(qkv.p);
    cx.ws.release(av.p);
    return DLPM_OK;
}

// free0 / free1: the sequence is the last consumer of x0 / x1 (released once its first layer has been enqueued)
int run_seq(Ctx &cx, const std::vector<Layer> &seq, Tensor4 x0, Tensor4 x1, Tensor4 *out, bool free0 = false, bool free1 = false) {
    Tensor4 h = x0;
    for (size_t i = 0; i < seq.size(); i++) {
        const Layer &L = seq[i];
        Tensor4 o;
        switch (L.kind) {
            case L_STEM: {     // h is the (B,C,H,W) input image
                o = new_tensor(cx, L.cout, h.H, h.W);
                ConvLaunch a = conv_io(cx, L.c1, h, Tensor4(), o);
                a.in_nchw = 1;
                plan_stats(cx, o, a);
                TRY(run_conv(cx, L.c1, a));
                break;
            }
            case L_RES:
                TRY(run_res(cx, L, h, (i == 0) ? x1 : Tensor4(), &o));
                break;
            case L_ATTN:
                TRY(run_attn(cx, L, h, &o));
                break;
            case L_DOWN:
            case L_UP: {
                const bool up = L.kind == L_UP;
                o = new_tensor(cx, h.C, up ? h.H * 2 : (h.H - 1) / 2 + 1, up ? h.W * 2 : (h.W - 1) / 2 + 1);
                ConvLaunch a = conv_io(cx, L.c1, h, Tensor4(), o);
                plan_stats(cx, o, a);
                TRY(up ? run_conv3(cx, L.c1, a) : run_conv(cx, L.c1, a));
                break;
            }
        }
        if (i == 0) {
            if (free0) drop(cx.ws, x0);
            if (free1) drop(cx.ws, x1);
        } else {
            drop(cx.ws, h);      // an intermediate of this sequence: the layer just enqueued was its only reader
        }
        h = o;
    }
    *out = h;
    return DLPM_OK;
}

__global__ void k_table_row(const float *__restrict__ table, const int32_t *__restrict__ row, int n, float *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = table[(int64_t)(*row) * n + i];
}

// time embedding -> time MLP, for M rows of t: e2[M][ted] = time_embed(timestep_embedding(t)) (unet.py:336-338, 470)
int time_mlp(dlpm_unet *u, const float *t, int M, float *e0, float *e1, float *e2, hipStream_t st) {
    const int mc = u->cfg.model_channels, ted = u->ted;
    TRY(launch_timestep_embedding(t, e0, M, mc, st));
    ConvLaunch g;
    g.B = M; g.Hin = g.Win = g.Hout = g.Wout = 1;
    g.src0 = e0; g.C0 = mc; g.bias = u->params[u->te0.p_b].dev; g.out = e1;
    TRY(run_conv(u, u->te0, g, st));
    g.src0 = e1; g.C0 = ted; g.bias = u->params[u->te2.p_b].dev; g.out = e2; g.act_silu = 1;
    return run_conv(u, u->te2, g, st);
}

// the row-concatenated per-ResBlock emb linears (SiLU on the input) of M rows emb[M][ted] (unet.py:147-150)
int emb_linears(dlpm_unet *u, const float *emb, int M, float *out, hipStream_t st) {
    ConvLaunch g;
    g.B = M; g.Hin = g.Win = g.Hout = g.Wout = 1;
    g.src0 = emb; g.C0 = u->ted; g.bias = u->embcat_b; g.out = out; g.act_silu = 1;
    return run_conv(u, u->embcat, g, st);
}

// time embedding -> time MLP -> the row-concatenated per-ResBlock emb linears, for M rows of t (unet.py:147-150, 336-338, 470)
int time_path(dlpm_unet *u, const float *t, int M, float *e0, float *e1, float *e2, float *out, hipStream_t st) {
    TRY(time_mlp(u, t, M, e0, e1, e2, st));
    return emb_linears(u, e2, M, out, st);
}

// optional [T][emb_total] table of the time path's output (time embedding -> time MLP -> the per-ResBlock emb linears) and the device
// step counter that picks its row: bound by the sampler around its forward calls (dlpm_unet_bind_time_table), per host thread
thread_local const dlpm_unet *tl_time_net = nullptr;
thread_local const float *tl_time_table = nullptr;
thread_local const int32_t *tl_time_index = nullptr;

// The plan's scale/shift rows cx.embout: time embedding -> time MLP -> the per-ResBlock emb linears (unet.py:147-150, 336-338, 470).  In
// the sampling loop t is the same for the whole batch (GenerativeLevyProcess.py:319), so these run for one row instead of B identical
// ones (a row's dot products do not depend on how many rows the GEMM has: bit-identical to the batched form)
int emb_rows(Ctx &cx, const float *t, float *e0, float *e1, float *e2) {
    PLAN_ENQUEUES(cx);
    dlpm_unet *u = cx.u;
    const int B = cx.B, Bt = cx.uniform_t ? 1 : B;
    const bool table = cx.uniform_t && tl_time_net == u && tl_time_table;
    if (u->num_classes > 0) {
        // class-conditional: emb = time_embed(t) + label_emb(y) per sample (unet.py:470-473), then the emb linears over B rows.  The
        // time-MLP row comes from the bound [T][ted] table (the sampler's), from one row (uniform t) or from B rows; the rows a GEMM
        // produces do not depend on how many it has, so a sample's emb row has the same bits on all three paths
        if (!table) TRY(time_mlp(u, t, Bt, e0, e1, e2, cx.st));
        TRY(launch_label_embedding_add(table ? tl_time_table : e2, table ? tl_time_index : nullptr, cx.uniform_t ? 0 : 1,
                                       u->params[u->p_label].dev, cx.y, u->num_classes, B, u->ted, e1, cx.st));
        return emb_linears(u, e1, B, cx.embout, cx.st);
    }
    if (!table) return time_path(u, t, Bt, e0, e1, e2, cx.embout, cx.st);
    // the whole time path is a function of the step index alone: its output for every step was computed once
    // (dlpm_unet_time_embeddings, same kernels, one row per step -- same bits) and the step reads its row
    k_table_row<<<(unsigned)ceil_div(u->emb_total, 256), 256, 0, cx.st>>>(tl_time_table, tl_time_index, u->emb_total, cx.embout);
    DLPM_LAUNCH_CHECK();
    return DLPM_OK;
}

int walk(dlpm_unet *u, Ctx &cx, const float *x, const float *t, float *eps) {
    const int B = cx.B, mc = u->cfg.model_channels, ted = u->ted;
    float *e0 = cx.ws.alloc((int64_t)B * mc), *e1 = cx.ws.alloc((int64_t)B * ted), *e2 = cx.ws.alloc((int64_t)B * ted);
    cx.embout = cx.ws.alloc((int64_t)B * u->emb_total);
    TRY(emb_rows(cx, t, e0, e1, e2));
    cx.ws.release(e0);
    cx.ws.release(e1);
    cx.ws.release(e2);
    u->feats.clear();
    std::vector<Tensor4> hs;
    Tensor4 h;     // the (B,C,H,W) input image first: the stem only reads it, and it is not the arena's to release
    h.p = const_cast<float *>(x); h.C = u->cfg.in_channels; h.H = h.W = u->cfg.image_size;
    // every input-block output waits on the skip stack for its output block; the middle block's input is the last of them
    for (auto &seq : u->in_blocks) {
        TRY(run_seq(cx, seq, h, Tensor4(), &h));
        hs.push_back(h);
        u->feats.push_back(h);
    }
    TRY(run_seq(cx, u->mid, h, Tensor4(), &h));
    u->feats.push_back(h);
    for (auto &seq : u->out_blocks) {
        Tensor4 skip = hs.back();
        hs.pop_back();
        if (skip.H != h.H || skip.W != h.W) {
            set_error("unet: skip connection %dx%d does not match %dx%d (image_size must be divisible by 2^(levels-1))",
                      skip.H, skip.W, h.H, h.W);
            return DLPM_ERR_ARG;
        }
        TRY(run_seq(cx, seq, h, skip, &h, true, true));   // last readers of the previous output and of the skip tensor
        u->feats.push_back(h);
    }
    float *cA = cx.ws.alloc((int64_t)B * h.C), *cB = cx.ws.alloc((int64_t)B * h.C);
    Tensor4 e;     // eps, (B,C,H,W) in the caller's buffer
    e.p = eps; e.C = u->head.cout; e.H = h.H; e.W = h.W;
    ConvLaunch a = conv_io(cx, u->head, h, Tensor4(), e);
    a.coefA = cA; a.coefB = cB; a.act_silu = 1; a.out_nchw = 1;
    // the head as a GEMM onto its 9 Cout tap channels + gather: the tap-channel tensor P lives in the arena
    const int64_t nP = conv_route(a).scratch_floats;
    float *P = nP ? cx.ws.alloc(nP) : nullptr;
    TRY(gn_any(cx, h, Tensor4(), u->p_head_gn_w, u->p_head_gn_b, nullptr, 0, cA, cB));
    TRY(run_conv(cx, u->head, a, cx.hu, P));
    if (!cx.ws.reuse) return DLPM_OK;
    for (auto &f : u->feats) f.p = nullptr;     // the arena has recycled them: dlpm_unet_get_feature needs dlpm_unet_keep_features
    return DLPM_OK;
}

// every layer in the order the plan runs them; fn(layer, cat): cat marks the first layer of an output block, whose input is [h | skip]
template <class F>
void for_each_layer(dlpm_unet *u, F fn) {
    for (auto &s : u->in_blocks)
        for (auto &L : s) fn(L, false);
    for (auto &L : u->mid) fn(L, false);
    for (auto &s : u->out_blocks)
        for (size_t i = 0; i < s.size(); i++) fn(s[i], i == 0);
}

// ... and every convolution, the time MLP's, the stacked emb linears and the head included
template <class F>
void for_each_conv(dlpm_unet *u, F fn) {
    for_each_layer(u, [&](Layer &L, bool) {
        fn(L.c1);
        if (L.kind == L_RES || L.kind == L_ATTN) fn(L.c2);
        if (L.kind == L_RES && L.has_skip) fn(L.skip);
    });
    fn(u->te0);
    fn(u->te2);
    fn(u->embcat);
    fn(u->head);
}

int64_t count_flops(dlpm_unet *u) {
    // 2*MAC per sample: conv / linear / attention matmuls
    int64_t f = 0;
    auto convf = [&](const ConvW &c, int H, int W) { f += 2LL * c.cout * c.cin * c.ks * c.ks * H * W; };
    convf(u->te0, 1, 1);
    convf(u->te2, 1, 1);
    f += 2LL * u->emb_total * u->ted;
    int H = u->cfg.image_size;
    for_each_layer(u, [&](const Layer &L, bool) {
        switch (L.kind) {
            case L_STEM: convf(L.c1, H, H); break;
            case L_RES:
                convf(L.c1, H, H); convf(L.c2, H, H);
                if (L.has_skip) convf(L.skip, H, H);
                break;
            case L_ATTN:
                convf(L.c1, H, H); convf(L.c2, H, H);
                f += 4LL * (H * H) * (H * H) * L.cin;
                break;
            case L_DOWN: H = (H - 1) / 2 + 1; convf(L.c1, H, H); break;
            case L_UP: H *= 2; convf(L.c1, H, H); break;
        }
    });
    convf(u->head, H, H);
    return f;
}

}  // namespace

static int create_net(const dlpm_unet_config *cfg, int32_t num_classes, dlpm_unet **out) {
    DLPM_CHECK_ARG(cfg && out, "dlpm_unet_create: null argument");
    DLPM_CHECK_ARG(cfg->in_channels > 0 && cfg->model_channels > 0 && cfg->out_channels > 0 && cfg->num_res_blocks > 0,
                   "dlpm_unet_create: channels / res blocks must be positive");
    DLPM_CHECK_ARG(cfg->n_mult > 0 && cfg->n_mult <= 8 && cfg->n_attn >= 0 && cfg->n_attn <= 8,
                   "dlpm_unet_create: bad channel_mult / attention_resolutions length");
    DLPM_CHECK_ARG(cfg->num_heads > 0 && cfg->image_size > 0, "dlpm_unet_create: bad num_heads / image_size");
    DLPM_CHECK_ARG(cfg->image_size % (1 << (cfg->n_mult - 1)) == 0,
                   "dlpm_unet_create: image_size %d not divisible by 2^%d (the reference UNet fails on such sizes too)",
                   cfg->image_size, cfg->n_mult - 1);
    dlpm_unet *u = new dlpm_unet();
    u->cfg = *cfg;
    u->num_classes = num_classes;
    build_arch(u);
    *out = u;
    return DLPM_OK;
}

extern "C" int dlpm_unet_create(const dlpm_unet_config *cfg, dlpm_unet **out) { return create_net(cfg, 0, out); }

extern "C" int dlpm_unet_create_conditional(const dlpm_unet_config *cfg, int32_t num_classes, dlpm_unet **out) {
    DLPM_CHECK_ARG(num_classes > 0, "dlpm_unet_create_conditional: num_classes must be positive, got %d", num_classes);
    return create_net(cfg, num_classes, out);
}

extern "C" int32_t dlpm_unet_num_classes(const dlpm_unet *net) { return net ? net->num_classes : 0; }

extern "C" int dlpm_unet_num_params(const dlpm_unet *net) { return net ? (int)net->params.size() : 0; }

extern "C" const char *dlpm_unet_param_key(const dlpm_unet *net, int i, int64_t *numel_out) {
    if (!net || i < 0 || i >= (int)net->params.size()) return nullptr;
    if (numel_out) *numel_out = net->params[i].numel;
    return net->params[i].key.c_str();
}

extern "C" int dlpm_unet_set_param(dlpm_unet *net, const char *key, const float *host, int64_t numel) {
    DLPM_CHECK_ARG(net && key && host, "dlpm_unet_set_param: null argument");
    auto it = net->index.find(key);
    DLPM_CHECK_ARG(it != net->index.end(), "dlpm_unet_set_param: unexpected key '%s' for this architecture", key);
    Param &p = net->params[it->second];
    DLPM_CHECK_ARG(p.numel == numel, "dlpm_unet_set_param: '%s' has %lld elements, expected %lld", key, (long long)numel,
                   (long long)p.numel);
    if (!p.dev) DLPM_HIP(hipMalloc(&p.dev, (size_t)numel * sizeof(float)));
    DLPM_HIP(hipMemcpy(p.dev, host, (size_t)numel * sizeof(float), hipMemcpyHostToDevice));
    p.set = true;
    net->finalized = false;
    return DLPM_OK;
}

static void free_dev(float *&p) {
    if (p) (void)hipFree(p);
    p = nullptr;
}

static void free_conv(ConvW &c) {
    for (float *&p : c.lay) free_dev(p);
}

// Brings every convolution's device copies in line with conv_layouts (conv.h) of its layer under the declared batch: frees what is present
// and not wanted, allocates and builds what is wanted and absent (after free_conv: everything).  So the 64- / 32-channel n-tile copies of
// the F(4x4) weights come and go with dlpm_unet_set_conv_policy's dispatch_batch.  Built from the parameters, on the null stream.
static int sync_layouts(dlpm_unet *u) {
    int rc = DLPM_OK;
    for_each_conv(u, [&](ConvW &c) {
        c.layer.dispatch_B = u->dispatch_B;
        const unsigned want = conv_layouts(c.layer);
        unsigned absent = 0;
        for (int l = 0; l < CONV_LAYOUT_COUNT && rc == DLPM_OK; l++) {
            if (!(want >> l & 1)) free_dev(c.lay[l]);
            if (!(want >> l & 1) || c.lay[l]) continue;
            if (hipMalloc(&c.lay[l], (size_t)conv_layout(l).floats(c.layer) * sizeof(float)) != hipSuccess) { c.lay[l] = nullptr; rc = DLPM_ERR_HIP; set_error("sync_layouts: hipMalloc failed"); continue; }
            absent |= 1u << l;
        }
        if (rc == DLPM_OK) rc = build_conv_layouts(c.layer, absent, oihw_of(u, c), c.lay, nullptr);
    });
    if (rc == DLPM_OK && hipDeviceSynchronize() != hipSuccess) { set_error("sync_layouts: synchronize failed"); rc = DLPM_ERR_HIP; }
    return rc;
}

// the layer of convolution `c` as conv_layouts is asked about it: C0 channels from the first concat source, images of `in` -> `out` pixels a side
static ConvLaunch layer_of(const ConvW &c, int C0, int in, int out) {
    ConvLaunch d;
    d.C0 = C0; d.C1 = c.cin - C0; d.Cout = c.cout; d.ks = c.ks;
    d.Hin = d.Win = in; d.Hout = d.Wout = out;
    return d;
}

// ... of the convolutions of one layer of the plan; C0: channels of the first concat source (an output block's first layer), res: the
// image size at the layer (as run_seq walks it)
static void describe_layer(Layer &L, int C0, int &res) {
    const int in = res;
    if (L.kind == L_DOWN) res = (res - 1) / 2 + 1;
    if (L.kind == L_UP) res *= 2;
    L.c1.layer = layer_of(L.c1, C0, in, res);
    L.c1.layer.in_nchw = L.kind == L_STEM; L.c1.layer.stride = L.kind == L_DOWN ? 2 : 1; L.c1.layer.ups = L.kind == L_UP;
    if (L.kind == L_RES || L.kind == L_ATTN) L.c2.layer = layer_of(L.c2, L.c2.cin, res, res);
    if (L.kind == L_RES && L.has_skip) L.skip.layer = layer_of(L.skip, C0, res, res);
}

// fused emb GEMM: this ResBlock's emb_layers.1 rows into the stacked weights
static int stack_emb(dlpm_unet *u, const Layer &L) {
    DLPM_HIP(hipMemcpy(u->embcat_w + (size_t)L.emb_off * u->ted, u->params[L.p_emb_w].dev, (size_t)2 * L.cout * u->ted * sizeof(float),
                       hipMemcpyDeviceToDevice));
    DLPM_HIP(hipMemcpy(u->embcat_b + L.emb_off, u->params[L.p_emb_b].dev, (size_t)2 * L.cout * sizeof(float), hipMemcpyDeviceToDevice));
    return DLPM_OK;
}

extern "C" int dlpm_unet_finalize(dlpm_unet *u) {
    DLPM_CHECK_ARG(u, "dlpm_unet_finalize: null handle");
    for (auto &p : u->params)
        if (!p.set) {
            set_error("dlpm_unet_finalize: parameter '%s' was never set", p.key.c_str());
            return DLPM_ERR_STATE;
        }
    for_each_conv(u, free_conv);
    if (u->embcat_w) (void)hipFree(u->embcat_w);
    if (u->embcat_b) (void)hipFree(u->embcat_b);
    DLPM_HIP(hipMalloc(&u->embcat_w, (size_t)u->emb_total * u->ted * sizeof(float)));
    DLPM_HIP(hipMalloc(&u->embcat_b, (size_t)u->emb_total * sizeof(float)));
    int rc = DLPM_OK, res = u->cfg.image_size, ch = 0;      // ch: channels of h entering the layer = the previous layer's cout
    for_each_layer(u, [&](Layer &L, bool cat) {
        describe_layer(L, cat ? ch : L.c1.cin, res);
        if (rc == DLPM_OK && L.kind == L_RES) rc = stack_emb(u, L);
        ch = L.cout;
    });
    TRY(rc);
    u->embcat.cout = u->emb_total; u->embcat.cin = u->ted; u->embcat.ks = 1;
    for (ConvW *c : {&u->te0, &u->te2, &u->embcat}) {
        c->layer = layer_of(*c, c->cin, 1, 1);
        c->layer.gemm = DLPM_GEMM_F32;     // the time path stays on the fp32 pipe whatever its row count
    }
    u->head.layer = layer_of(u->head, u->head.cin, res, res);
    u->head.layer.out_nchw = 1;
    TRY(sync_layouts(u));     // (under the dispatch batch declared before finalize, if any)
    u->flops = count_flops(u);
    u->finalized = true;
    u->plan_version++;
    return DLPM_OK;
}

extern "C" int dlpm_unet_set_conv_policy(dlpm_unet *u, int32_t generation, int64_t dispatch_batch) {
    DLPM_CHECK_ARG(u, "dlpm_unet_set_conv_policy: null handle");
    DLPM_CHECK_ARG(generation >= DLPM_CONV_AUTO && generation <= DLPM_CONV_IGEMM, "dlpm_unet_set_conv_policy: unknown generation %d",
                   generation);
    DLPM_CHECK_ARG(dispatch_batch >= 0, "dlpm_unet_set_conv_policy: negative dispatch batch");
    if (u->gen == generation && u->dispatch_B == dispatch_batch) return DLPM_OK;
    u->gen = generation;
    u->dispatch_B = dispatch_batch;
    u->plan_version++;
    if (u->finalized) TRY(sync_layouts(u));
    return DLPM_OK;
}

extern "C" int dlpm_unet_set_gemm_policy(dlpm_unet *u, int32_t mode) {
    DLPM_CHECK_ARG(u, "dlpm_unet_set_gemm_policy: null handle");
    DLPM_CHECK_ARG(mode >= DLPM_GEMM_AUTO && mode <= DLPM_GEMM_BF16X3, "dlpm_unet_set_gemm_policy: unknown mode %d", mode);
    if (u->gemm == mode) return DLPM_OK;
    u->gemm = mode;
    u->plan_version++;
    return DLPM_OK;
}

extern "C" int64_t dlpm_unet_time_embedding_width(const dlpm_unet *u) { return u ? u->emb_total : -1; }
extern "C" int64_t dlpm_unet_time_embeddings_scratch_bytes(const dlpm_unet *u, int64_t M) {
    return (u && M > 0) ? M * (u->cfg.model_channels + 2 * (int64_t)u->ted) * (int64_t)sizeof(float) : -1;
}

extern "C" int dlpm_unet_time_embeddings(dlpm_unet *net, const float *t_dev, int64_t M, float *out_dev, void *scratch_dev, int64_t scratch_bytes,
                                         dlpm_stream_t stream) {
    DLPM_CHECK_ARG(net && t_dev && out_dev && scratch_dev && M > 0 && M < (1 << 24), "dlpm_unet_time_embeddings: bad argument");
    if (net->num_classes > 0) {
        set_error("dlpm_unet_time_embeddings: the emb rows of a class-conditional net depend on the label, not on t alone");
        return DLPM_ERR_UNSUPPORTED;
    }
    if (!net->finalized) {
        set_error("dlpm_unet_time_embeddings: call dlpm_unet_finalize first");
        return DLPM_ERR_STATE;
    }
    const int64_t need = dlpm_unet_time_embeddings_scratch_bytes(net, M);
    if (scratch_bytes < need) {
        set_error("dlpm_unet_time_embeddings: scratch of %lld bytes, need %lld", (long long)scratch_bytes, (long long)need);
        return DLPM_ERR_NOMEM;
    }
    float *e0 = static_cast<float *>(scratch_dev), *e1 = e0 + M * net->cfg.model_channels, *e2 = e1 + M * net->ted;
    return time_path(net, t_dev, (int)M, e0, e1, e2, out_dev, as_stream(stream));
}

int64_t dlpm::unet_time_mlp_width(const dlpm_unet *net) { return net ? net->ted : -1; }

// the time-MLP rows of a conditional net (before the label term): out_dev[M][4 * model_channels], same scratch as above
int dlpm::unet_time_mlp_rows(dlpm_unet *net, const float *t_dev, int64_t M, float *out_dev, void *scratch_dev, int64_t scratch_bytes,
                             hipStream_t st) {
    DLPM_CHECK_ARG(net && t_dev && out_dev && scratch_dev && M > 0 && M < (1 << 24), "unet_time_mlp_rows: bad argument");
    if (!net->finalized) {
        set_error("unet_time_mlp_rows: call dlpm_unet_finalize first");
        return DLPM_ERR_STATE;
    }
    if (scratch_bytes < dlpm_unet_time_embeddings_scratch_bytes(net, M)) {
        set_error("unet_time_mlp_rows: scratch too small");
        return DLPM_ERR_NOMEM;
    }
    float *e0 = static_cast<float *>(scratch_dev), *e1 = e0 + M * net->cfg.model_channels;
    return time_mlp(net, t_dev, (int)M, e0, e1, out_dev, st);
}

extern "C" int dlpm_unet_bind_time_table(dlpm_unet *net, const float *table_dev, const int32_t *row_index_dev) {
    DLPM_CHECK_ARG(net && ((table_dev == nullptr) == (row_index_dev == nullptr)), "dlpm_unet_bind_time_table: give both pointers or neither");
    // per HOST THREAD, not per net: two samplers that share one net from different threads each see their own binding while
    // they enqueue (round 3 kept it in the net, where one thread's table could be baked into the other's captured graph)
    // ONE binding per host thread: binding a second net replaces the first; un-binding (null pointers) clears the slot only if
    // `net` is the net it holds -- un-binding net A must not drop net B's table
    if (!table_dev && tl_time_net != net) return DLPM_OK;
    tl_time_net = table_dev ? net : nullptr;
    tl_time_table = table_dev;
    tl_time_index = row_index_dev;
    return DLPM_OK;
}

extern "C" int64_t dlpm_unet_plan_version(const dlpm_unet *u) { return u ? u->plan_version : -1; }

// the dry run of the plan at batch B: the arena's peak, and how many blocks the plan asks the arena for
static int64_t dry_walk(const dlpm_unet *net, int64_t B, int64_t *nalloc) {
    if (!net || B <= 0) return -1;
    Ctx cx;
    cx.u = const_cast<dlpm_unet *>(net);
    cx.B = (int)B;
    cx.ws.dry = true;
    cx.ws.reuse = !net->keep_feats;
    cx.st = nullptr;
    std::vector<Tensor4> keep = net->feats;
    int r = walk(cx.u, cx, nullptr, nullptr, nullptr);
    cx.u->feats = keep;
    if (nalloc) *nalloc = cx.ws.nalloc;
    return r == DLPM_OK ? cx.ws.peak : -1;
}

extern "C" int64_t dlpm_unet_workspace_bytes(const dlpm_unet *net, int64_t B) { return dry_walk(net, B, nullptr); }

// The workspace of a batch walked as `chains` independent row ranges (dlpm_sampler's two-chain step): chain c covers rows
// [rows_off[c], rows_off[c] + rows[c]) -- B / chains each, the remainder going to the last chains, so B = 5 is 2 + 3 -- and owns the
// arena [arena_off[c], arena_off[c] + arena_bytes[c]) of the one allocation, sized by dlpm_unet_workspace_bytes(net, rows[c]).  Every
// block of the plan is proportional to the batch and rounded up to the arena's 256-byte granule, so the arenas together may exceed
// the single arena of B only by that rounding: *slack_bytes = 256 bytes per block the plan asks for, per chain.  Returns the bytes the
// arenas need together (compare with *single_bytes + *slack_bytes), -1 on error.
extern "C" int64_t dlpm_unet_chain_workspace(const dlpm_unet *net, int64_t B, int32_t chains, int64_t *rows_off, int64_t *rows,
                                             int64_t *arena_off, int64_t *arena_bytes, int64_t *single_bytes, int64_t *slack_bytes) {
    if (!net || chains < 1 || chains > DLPM_MAX_CHAINS || B < chains || !rows_off || !rows || !arena_off || !arena_bytes) {
        set_error("dlpm_unet_chain_workspace: bad argument");
        return -1;
    }
    const int64_t single = dry_walk(net, B, nullptr);
    if (single < 0) return -1;
    int64_t at = 0, b0 = 0, slack = 0;
    for (int c = 0; c < chains; c++) {
        const int64_t n = B / chains + (c >= chains - B % chains ? 1 : 0);
        int64_t blocks = 0;
        const int64_t need = dry_walk(net, n, &blocks);
        if (need < 0) return -1;
        rows_off[c] = b0; rows[c] = n;
        arena_off[c] = at; arena_bytes[c] = need;      // (a peak is a sum of 256-byte blocks: every arena starts on a granule)
        b0 += n; at += need; slack += 256 * blocks;
    }
    if (single_bytes) *single_bytes = single;
    if (slack_bytes) *slack_bytes = slack;
    return at;
}

static int unet_forward(dlpm_unet *net, const float *x_dev, const float *t_dev, float *eps_dev, int64_t B, void *workspace_dev,
                        int64_t workspace_bytes, dlpm_stream_t stream, bool uniform_t, const int64_t *y_dev,
                        const HeadUpdate *hu = nullptr);

extern "C" int dlpm_unet_forward(dlpm_unet *net, const float *x_dev, const float *t_dev, float *eps_dev, int64_t B,
                                 void *workspace_dev, int64_t workspace_bytes, dlpm_stream_t stream) {
    return unet_forward(net, x_dev, t_dev, eps_dev, B, workspace_dev, workspace_bytes, stream, false, nullptr);
}

extern "C" int dlpm_unet_forward_uniform_t(dlpm_unet *net, const float *x_dev, const float *t_dev, float *eps_dev, int64_t B,
                                           void *workspace_dev, int64_t workspace_bytes, dlpm_stream_t stream) {
    return unet_forward(net, x_dev, t_dev, eps_dev, B, workspace_dev, workspace_bytes, stream, true, nullptr);
}

extern "C" int dlpm_unet_forward_labels(dlpm_unet *net, const float *x_dev, const float *t_dev, const int64_t *y_dev, float *eps_dev,
                                        int64_t B, void *workspace_dev, int64_t workspace_bytes, dlpm_stream_t stream) {
    DLPM_CHECK_ARG(y_dev, "dlpm_unet_forward_labels: null labels");
    return unet_forward(net, x_dev, t_dev, eps_dev, B, workspace_dev, workspace_bytes, stream, false, y_dev);
}

extern "C" int dlpm_unet_forward_uniform_t_labels(dlpm_unet *net, const float *x_dev, const float *t_dev, const int64_t *y_dev,
                                                  float *eps_dev, int64_t B, void *workspace_dev, int64_t workspace_bytes,
                                                  dlpm_stream_t stream) {
    DLPM_CHECK_ARG(y_dev, "dlpm_unet_forward_uniform_t_labels: null labels");
    return unet_forward(net, x_dev, t_dev, eps_dev, B, workspace_dev, workspace_bytes, stream, true, y_dev);
}

// the reverse update as the head convolution's epilogue carries it
static HeadUpdate head_update_of(const dlpm_update_args *upd) {
    HeadUpdate hu;
    hu.x = upd->x_dev; hu.z = upd->z_dev; hu.t = upd->t_dev; hu.g = upd->g_dev; hu.c_eps = upd->c_eps_dev; hu.c_noise = upd->c_noise_dev;
    hu.key = upd->key_dev; hu.seed = upd->seed; hu.sample_offset = upd->sample_offset; hu.hist_pp = upd->hist_pp;
    hu.T = upd->T; hu.B = upd->B;
    return hu;
}

// Whether this net's head convolution runs on the kernel that can carry the update (a property of the architecture).
static bool head_fusable(const dlpm_unet *u) {
    ConvLaunch L;
    const int H = u->cfg.image_size;
    attach_conv(u, u->head, L);
    L.C0 = u->head.cin; L.Hin = L.Hout = H; L.Win = L.Wout = H; L.out_nchw = 1;
    L.coefA = L.coefB = reinterpret_cast<const float *>(u);   // (the head always carries its GroupNorm: only non-null matters here)
    L.act_silu = 1;
    return conv_route(L).head();
}

extern "C" int dlpm_unet_forward_update(dlpm_unet *net, const float *x_in_dev, const float *t_dev, const dlpm_update_args *upd,
                                        float *eps_scratch_dev, int64_t B, void *workspace_dev, int64_t workspace_bytes,
                                        dlpm_stream_t stream) {
    return dlpm::unet_forward_update_labels(net, x_in_dev, t_dev, nullptr, upd, eps_scratch_dev, B, workspace_dev, workspace_bytes,
                                            as_stream(stream));
}

// dlpm_unet_forward_update with the class labels of a conditional net (dlpm_sampler's step; y_dev null for an unconditional net)
int dlpm::unet_forward_update_labels(dlpm_unet *net, const float *x_in_dev, const float *t_dev, const int64_t *y_dev,
                                     const dlpm_update_args *upd, float *eps_scratch_dev, int64_t B, void *workspace_dev,
                                     int64_t workspace_bytes, hipStream_t stream) {
    DLPM_CHECK_ARG(net && x_in_dev && t_dev && upd && upd->x_dev && upd->t_dev && upd->g_dev && upd->c_eps_dev && upd->c_noise_dev,
                   "dlpm_unet_forward_update: null argument");
    DLPM_CHECK_ARG(upd->B == B, "dlpm_unet_forward_update: update batch %lld != %lld", (long long)upd->B, (long long)B);
    const int64_t D = (int64_t)net->cfg.out_channels * net->cfg.image_size * net->cfg.image_size;
    DLPM_CHECK_ARG(upd->D == D, "dlpm_unet_forward_update: state of %lld elements per sample, the net emits %lld", (long long)upd->D,
                   (long long)D);
    const bool aligned = ((reinterpret_cast<uintptr_t>(upd->x_dev) | reinterpret_cast<uintptr_t>(upd->z_dev)) % 16) == 0;
    const bool fuse = net->finalized && head_fusable(net) && aligned &&
                      !(upd->flags & (DLPM_UPD_DLIM | DLPM_UPD_CLIP | DLPM_UPD_ELEMENTWISE));
    if (!fuse) {   // the variants the head's epilogue does not carry: eps through HBM, then the update kernels
        DLPM_CHECK_ARG(eps_scratch_dev, "dlpm_unet_forward_update: this update variant needs the eps scratch buffer");
        int r = unet_forward(net, x_in_dev, t_dev, eps_scratch_dev, B, workspace_dev, workspace_bytes, stream, true, y_dev);
        if (r != DLPM_OK) return r;
        dlpm_update_args a = *upd;
        a.eps_dev = eps_scratch_dev;
        return dlpm_update_f32(&a, stream);
    }
    const HeadUpdate hu = head_update_of(upd);     // (upd->B == B, checked above)
    float dummy;   // walk() wants a non-null eps pointer; the fused head never writes it
    int r = unet_forward(net, x_in_dev, t_dev, eps_scratch_dev ? eps_scratch_dev : &dummy, B, workspace_dev, workspace_bytes, stream, true,
                         y_dev, &hu);
    if (r != DLPM_OK) return r;
    if (upd->flags & DLPM_UPD_ADVANCE) return launch_step_advance(const_cast<int32_t *>(upd->t_dev), stream);
    return DLPM_OK;
}

// Whether the plain reverse update of this net rides in its head convolution (what unet_forward_update_labels decides per call)
bool dlpm::unet_head_carries_update(const dlpm_unet *net) { return net && net->finalized && head_fusable(net); }

// The forward + fused update of Bc rows of a larger batch (dlpm_sampler's chains): `upd` describes the rows -- x_dev, c_eps_dev and
// c_noise_dev point at the first of them, upd->B stays the row pitch of the [T,B] tables, the key holds the global index of the first
// row -- and the net walks Bc samples in a workspace of its own.  The plain stochastic update only, never advances the step counter
// (the caller does, once all chains have read it), no history row.  Kernel choice follows the declared dispatch batch as in every
// other forward, so the rows get the bits the whole batch would give them.
int dlpm::unet_forward_update_rows(dlpm_unet *net, const float *x_in_dev, const float *t_dev, const dlpm_update_args *upd, int64_t Bc,
                                   void *workspace_dev, int64_t workspace_bytes, hipStream_t stream) {
    DLPM_CHECK_ARG(net && x_in_dev && t_dev && upd && upd->x_dev && upd->t_dev && upd->g_dev && upd->c_eps_dev && upd->c_noise_dev,
                   "unet_forward_update_rows: null argument");
    DLPM_CHECK_ARG(Bc > 0 && Bc <= upd->B, "unet_forward_update_rows: %lld rows of a batch of %lld", (long long)Bc, (long long)upd->B);
    const int64_t D = (int64_t)net->cfg.out_channels * net->cfg.image_size * net->cfg.image_size;
    DLPM_CHECK_ARG(upd->D == D, "unet_forward_update_rows: state of %lld elements per sample, the net emits %lld", (long long)upd->D,
                   (long long)D);
    const bool aligned = ((reinterpret_cast<uintptr_t>(upd->x_dev) | reinterpret_cast<uintptr_t>(upd->z_dev)) % 16) == 0;
    if (!dlpm::unet_head_carries_update(net) || !aligned || net->num_classes > 0 || upd->hist_pp ||
        (upd->flags & (DLPM_UPD_DLIM | DLPM_UPD_CLIP | DLPM_UPD_ELEMENTWISE | DLPM_UPD_ADVANCE))) {
        set_error("unet_forward_update_rows: only the plain update fused into the head convolution runs on a row range");
        return DLPM_ERR_UNSUPPORTED;
    }
    const HeadUpdate hu = head_update_of(upd);     // (no history row: refused above)
    float dummy;   // walk() wants a non-null eps pointer; the fused head never writes it
    return unet_forward(net, x_in_dev, t_dev, &dummy, Bc, workspace_dev, workspace_bytes, stream, true, nullptr, &hu);
}

static int unet_forward(dlpm_unet *net, const float *x_dev, const float *t_dev, float *eps_dev, int64_t B, void *workspace_dev,
                        int64_t workspace_bytes, dlpm_stream_t stream, bool uniform_t, const int64_t *y_dev, const HeadUpdate *hu) {
    DLPM_CHECK_ARG(net && x_dev && t_dev && eps_dev && workspace_dev, "dlpm_unet_forward: null argument");
    // the reference asserts that labels are given iff the net is class-conditional (unet.py:463-466)
    DLPM_CHECK_ARG(net->num_classes == 0 || y_dev, "dlpm_unet_forward: must specify y if and only if the model is class-conditional "
                   "(this net has %d classes: call the *_labels forward)", net->num_classes);
    DLPM_CHECK_ARG(net->num_classes > 0 || !y_dev, "dlpm_unet_forward: must specify y if and only if the model is class-conditional "
                   "(labels given to an unconditional net)");
    DLPM_CHECK_ARG(B > 0 && B < (1 << 24), "dlpm_unet_forward: bad batch %lld", (long long)B);
    if (!net->finalized) {
        set_error("dlpm_unet_forward: call dlpm_unet_finalize first");
        return DLPM_ERR_STATE;
    }
    const int64_t need = dlpm_unet_workspace_bytes(net, B);
    if (need < 0) return DLPM_ERR_ARG;
    if (workspace_bytes < need) {
        set_error("dlpm_unet_forward: workspace of %lld bytes, need %lld", (long long)workspace_bytes, (long long)need);
        return DLPM_ERR_NOMEM;
    }
    Ctx cx;
    cx.u = net;
    cx.B = (int)B;
    cx.ws.base = static_cast<char *>(workspace_dev);
    cx.ws.cap = workspace_bytes;
    cx.ws.reuse = !net->keep_feats;
    cx.st = as_stream(stream);
    cx.uniform_t = uniform_t;
    cx.y = y_dev;
    cx.hu = hu;
    return walk(net, cx, x_dev, t_dev, eps_dev);
}

extern "C" int dlpm_unet_keep_features(dlpm_unet *net, int on) {
    DLPM_CHECK_ARG(net, "dlpm_unet_keep_features: null handle");
    net->keep_feats = on != 0;
    net->plan_version++;       // the workspace size changes with it
    return DLPM_OK;
}

extern "C" int dlpm_unet_num_features(const dlpm_unet *net) {
    return net ? (int)(net->in_blocks.size() + 1 + net->out_blocks.size()) : 0;
}

extern "C" int dlpm_unet_feature_shape(const dlpm_unet *net, int i, int32_t *C, int32_t *H, int32_t *W) {
    DLPM_CHECK_ARG(net && i >= 0 && i < (int)net->feats.size(), "dlpm_unet_feature_shape: no such feature (run a forward first)");
    if (C) *C = net->feats[i].C;
    if (H) *H = net->feats[i].H;
    if (W) *W = net->feats[i].W;
    return DLPM_OK;
}

extern "C" int dlpm_unet_get_feature(dlpm_unet *net, int i, float *out_nchw_dev, int64_t B, dlpm_stream_t stream) {
    DLPM_CHECK_ARG(net && out_nchw_dev && i >= 0 && i < (int)net->feats.size() && net->feats[i].p,
                   "dlpm_unet_get_feature: no such feature (call dlpm_unet_keep_features(net, 1), then run a forward)");
    const Tensor4 &f = net->feats[i];
    return dlpm_nhwc_to_nchw_f32(f.p, out_nchw_dev, (int32_t)B, f.C, f.H, f.W, stream);
}

extern "C" int64_t dlpm_unet_flops_per_sample(const dlpm_unet *net) { return net ? net->flops : 0; }

extern "C" void dlpm_unet_destroy(dlpm_unet *u) {
    if (!u) return;
    for_each_conv(u, free_conv);
    if (u->embcat_w) (void)hipFree(u->embcat_w);
    if (u->embcat_b) (void)hipFree(u->embcat_b);
    for (auto &p : u->params)
        if (p.dev) (void)hipFree(p.dev);
    delete u;
}

// ---------------------------------------------------------------------------------------------
// building-block entry points (parity tests call each kernel through the C ABI)
// ---------------------------------------------------------------------------------------------
// the launch a dlpm_conv_args describes, no weights or policy attached yet
static ConvLaunch launch_of_args(const dlpm_conv_args *a) {
    ConvLaunch L;
    L.src0 = a->src0; L.src1 = a->src1; L.C0 = a->C0; L.C1 = a->C1; L.B = a->B;
    L.Hin = a->Hin; L.Win = a->Win; L.Hout = a->Hout; L.Wout = a->Wout;
    L.ks = a->ksize; L.stride = a->stride; L.ups = a->upsample;
    L.bias = a->bias; L.coefA = a->coefA; L.coefB = a->coefB; L.act_silu = a->act_silu;
    L.res0 = a->res0; L.res1 = a->res1; L.R0 = a->R0; L.out = a->out; L.Cout = a->Cout;
    L.in_nchw = a->in_nchw; L.out_nchw = a->out_nchw;
    return L;
}
static int conv2d_entry(const dlpm_conv_args *a, float *scratch_dev, float *stats_out, int32_t *stats_px, dlpm_stream_t stream);
extern "C" int dlpm_conv2d_f32(const dlpm_conv_args *a, float *scratch_dev, dlpm_stream_t stream) {
    return conv2d_entry(a, scratch_dev, nullptr, nullptr, stream);
}
extern "C" int dlpm_conv2d_stats_f32(const dlpm_conv_args *a, float *scratch_dev, float *stats_out, int32_t *stats_px, dlpm_stream_t stream) {
    DLPM_CHECK_ARG(stats_out && stats_px, "dlpm_conv2d_stats_f32: null argument");
    return conv2d_entry(a, scratch_dev, stats_out, stats_px, stream);
}
// stats_out: the launch also emits the GroupNorm statistics partials of its output, wherever its route can (ConvRoute::stats_px > 0)
static int conv2d_entry(const dlpm_conv_args *a, float *scratch_dev, float *stats_out, int32_t *stats_px, dlpm_stream_t stream) {
    DLPM_CHECK_ARG(a && a->src0 && a->weight && a->out && scratch_dev, "dlpm_conv2d_f32: null argument");
    DLPM_CHECK_ARG(a->ksize == 1 || a->ksize == 3, "dlpm_conv2d_f32: ksize must be 1 or 3");
    DLPM_CHECK_ARG(a->stride == 1 || a->stride == 2, "dlpm_conv2d_f32: stride must be 1 or 2");
    DLPM_CHECK_ARG((a->C1 == 0) == (a->src1 == nullptr), "dlpm_conv2d_f32: src1/C1 mismatch");
    ConvLaunch L = launch_of_args(a);
    const int fd = a->force_direct, Cin_ = a->C0 + a->C1;
    const bool ig = !(fd & 1) && igemm_supported(L);
    if ((a->in_nchw || a->out_nchw) && a->C1 != 0) {
        set_error("dlpm_conv2d_f32: NCHW boundary layouts do not combine with a concat input");
        return DLPM_ERR_UNSUPPORTED;
    }
    if (fd & 4) {
        set_error("dlpm_conv2d_f32: force_direct bit 2 (value 4) asked for 1x1 convolutions on the weight-streaming kernel, which was removed");
        return DLPM_ERR_UNSUPPORTED;
    }
    L.gemm = DLPM_GEMM_F32;
    // The force_direct bits as masks of layouts asked for (sizes, relayout calls and ConvLaunch fields: the table of conv.h), placed in the
    // scratch buffer front to back.  A layout that does not fit is left out, and the launch takes what its route makes of the rest.
    const int64_t cap = a->scratch_floats;
    float *at[CONV_LAYOUT_COUNT] = {};
    int64_t used = 0;      // floats of the front of the scratch taken so far
    auto place = [&](unsigned mask, int64_t &from, int64_t room) { return place_conv_layouts(L, mask, scratch_dev, 1, room, at, &from); };
    auto floats = [&](ConvLayout l) { return conv_layout(l).floats(L); };
    unsigned have = place(lay_bit(ig ? LAY_PLAIN : LAY_PLAIN_DIRECT), used, INT64_MAX);       // the plain copy: whatever the size says
    // bit 16: the bf16x3 planes, behind the plain copy
    if (ig && (fd & 16) && a->Cout % 128 == 0 && Cin_ % 32 == 0 && place(lay_bit(LAY_SPLIT), used, cap)) {
        have |= lay_bit(LAY_SPLIT);
        L.gemm = DLPM_GEMM_BF16X3;
    }
    const bool split = (have & lay_bit(LAY_SPLIT)) != 0;
    // no split copy (it sits where these would go): the fragment copy, the F(2x2) copy unless bit 2 says no, and under bit 8 (or 256 / 512, which
    // need it) the F(4x4,3x3) copy behind them (128-, 64- or 32-channel n-tiles).  That kernel takes input channels in multiples of 8, also where
    // the implicit GEMM (multiples of 32) does not
    const bool wino_shape = a->ksize == 3 && !split && !(fd & 2) && a->stride == 1 && !a->in_nchw && !a->out_nchw;
    unsigned ask = 0;
    if (ig && a->ksize == 3 && !split && Cin_ % 32 == 0) ask |= lay_bit(LAY_FRAG) | (wino_shape && a->Cout % 64 == 0 ? lay_bit(LAY_WINO) : 0);
    if (wino_shape && (fd & (8 | 256 | 512)) && a->Cout % 32 == 0 && Cin_ % 8 == 0) ask |= lay_bit(LAY_WINO4);
    have |= place(ask, used, cap);
    const bool ask_f4 = (have & lay_bit(LAY_WINO4)) != 0;
    if (ask_f4) {          // no F(2x2) alternative: the launch takes the F(4x4) kernel (whose copy stays behind the F(2x2) copy's place)
        have &= ~lay_bit(LAY_WINO);
        at[LAY_WINO] = nullptr;
    }
    // bit 256: an upsampling convolution through the sub-pixel kernel (four parity-class F(4x4,2x2) convolutions on the low-res image); bit 512: a
    // layer on 4x4-pixel tensors through the one-tile kernel (k_conv3x3_wino4_one).  Either copy goes behind the F(4x4,3x3) copy
    if ((fd & 256) && ask_f4 && a->Cout % 128 == 0) have |= place(lay_bit(LAY_WINO4SP), used, cap);
    const bool ask_one = (fd & 512) != 0;
    if (ask_one && ask_f4 && !at[LAY_WINO4SP] && !a->upsample && wino4_one_layer_ok(a->Cout, a->C0, a->C1, a->Hout, a->Wout) &&
        place(lay_bit(LAY_WINO4_ONE), used, cap)) {
        have |= lay_bit(LAY_WINO4_ONE);
        L.gen = DLPM_CONV_F4;     // (this entry declares no batch: the generation under which the shape is taken without one)
    }
    // the head kernels (Cout <= 4): bit 64 the one-pass kernel (head_fused.hip; in the UNet it also carries the sampler's update), W' fragments
    // at the front of the scratch buffer; bit 32 the head as a 1x1 GEMM onto 9 Cout tap channels + gather, W' at the front, P behind it;
    // no bit: k_conv3x3_head where it takes the shape, its [tap][cin][4] copy at the END of the scratch buffer (the front holds the layouts above)
    const bool head_shape = a->ksize == 3 && a->C0 % 32 == 0 && a->C1 == 0;
    const int ask_head = !head_shape || a->Cout > 3 ? 0 : (fd & 64) ? 64 : (fd & 32);
    int64_t front = 0;
    if (ask_head == 64) {
        L.gemm = (fd & 128) ? DLPM_GEMM_F32 : DLPM_GEMM_AUTO;   // bit 128: its fp32-MFMA form instead of the bf16 x 3 one
        have |= place(lay_bit(LAY_HEAD_FUSED), front, cap);
    } else if (ask_head == 32) {
        have |= place(lay_bit(LAY_HEAD_TAPS), front, cap - head_gemm_scratch_floats(L));
    } else if (!(fd & 7) && head_shape && a->Cout <= 4) {
        front = cap - floats(LAY_HEAD);
        if (front >= floats(LAY_PLAIN) + floats(LAY_FRAG)) have |= place(lay_bit(LAY_HEAD), front, cap);
    }
    attach_conv_layouts(L, at);
    // A bit ASKS for its kernel: a route that is not the family asked for (a geometry or scratch size the kernel cannot take, e.g. 16 one-tile
    // 4x4 images on a 64- / 32-channel F(4x4) n-tile) is an error, not a silent drop to another kernel -- tests that compare "the F(4x4)
    // kernel" with the default path must not pass for the wrong reason
    const ConvRoute R = conv_route(L);
    const bool f4 = R.family == CONV_WINO4 || R.family == CONV_WINO4SP;
    const bool direct = (fd & 1) && !R.head() && !f4;    // bit 0: the direct kernel, whatever the route (it has no statistics epilogue)
    const int px = direct ? 0 : R.stats_px;
    const struct { bool asked, got; const char *msg; } asks[] = {
        {ask_f4, f4, "dlpm_conv2d_f32: force_direct bit 8 asks for the F(4x4,3x3) kernel, which does not take this geometry"},
        {(fd & 256) != 0, R.family == CONV_WINO4SP,
         "dlpm_conv2d_f32: force_direct bit 256 asks for the sub-pixel upsampling kernel, which does not take this geometry / scratch size"},
        {ask_one, R.family == CONV_WINO4 && R.one,
         "dlpm_conv2d_f32: force_direct bit 512 asks for the one-tile F(4x4) kernel, which does not take this geometry / scratch size"},
        {stats_out != nullptr, px > 0,
         "dlpm_conv2d_stats_f32: this launch emits no statistics (its kernel has no statistics epilogue, or its partials would not lie inside one image)"},
        {ask_head == 64, R.family == CONV_HEAD_FUSED, "dlpm_conv2d_f32: the one-pass head kernel does not take this shape / scratch size"},
        {ask_head == 32, R.family == CONV_HEAD_GEMM, "dlpm_conv2d_f32: the GEMM + gather head does not take this shape / scratch size"},
    };
    for (const auto &q : asks)
        if (q.asked && !q.got) {
            set_error("%s", q.msg);
            return DLPM_ERR_UNSUPPORTED;
        }
    if (stats_out) {
        L.stats_out = reinterpret_cast<float2 *>(stats_out);
        *stats_px = px;
    }
    hipStream_t st = as_stream(stream);
    if (R.family != CONV_HEAD) have &= ~lay_bit(LAY_HEAD);      // (k_conv3x3_head's copy is offered unasked: built where the route takes it)
    TRY(build_conv_layouts(L, have, a->weight, at, st));         // in the order of the enum: a head copy at the front overwrites the plain one
    if (direct) return launch_conv_direct(L, st);
    return launch_conv(L, nullptr, scratch_dev + floats(LAY_HEAD_TAPS), st);
}

// ---- a 3x3 stride-1 launch under a declared policy (include/dlpm_amd_conv.h)
// The launch of `a` under (generation, dispatch_batch) with the layouts conv_layouts gives the layer (*mask), laid out one behind the other
// from `base` in the order of the enum (each at a multiple of 64 floats: at[]); *used = their floats together.  Nothing is read through a pointer.
static int policy_launch(const dlpm_conv_args *a, int32_t generation, int64_t dispatch_batch, float *base, ConvLaunch *out,
                         float *at[CONV_LAYOUT_COUNT], unsigned *mask, int64_t *used) {
    DLPM_CHECK_ARG(a, "dlpm_conv_policy: null argument");
    DLPM_CHECK_ARG(generation >= DLPM_CONV_AUTO && generation <= DLPM_CONV_IGEMM, "dlpm_conv_policy: unknown generation %d", generation);
    DLPM_CHECK_ARG(dispatch_batch >= 0, "dlpm_conv_policy: negative dispatch batch");
    if (a->ksize != 3 || a->stride != 1 || a->in_nchw || a->out_nchw || a->Cout <= 4 || a->force_direct != 0) {
        set_error("dlpm_conv_policy: takes 3x3 stride-1 NHWC launches with Cout > 4 and force_direct = 0");
        return DLPM_ERR_UNSUPPORTED;
    }
    const int up = a->upsample ? 2 : 1;
    DLPM_CHECK_ARG(a->B > 0 && a->C0 > 0 && a->C1 >= 0 && a->Hin > 0 && a->Win > 0 && a->Hout == up * a->Hin && a->Wout == up * a->Win &&
                   a->R0 >= 0 && a->R0 <= a->Cout,
                   "dlpm_conv_policy: B %d, C0 %d, C1 %d, %dx%d -> %dx%d, R0 %d", a->B, a->C0, a->C1, a->Hin, a->Win, a->Hout, a->Wout, a->R0);
    ConvLaunch L = launch_of_args(a);
    L.ups = a->upsample ? 1 : 0;
    L.gen = generation;
    L.dispatch_B = dispatch_batch;
    *mask = conv_layouts(L) & ~lay_bit(LAY_SMALL);     // (the fused blocks' order belongs to no launch)
    *used = 0;
    place_conv_layouts(L, *mask, base, 64, INT64_MAX, at, used);
    attach_conv_layouts(L, at);
    *out = L;
    return DLPM_OK;
}

static void policy_route_out(const ConvLaunch &L, const ConvRoute &R, int64_t used, dlpm_conv_route *r) {
    r->family = (int32_t)R.family;
    r->bh = R.bh; r->bw = R.bw; r->nimg = R.nimg; r->nq = R.nq; r->stats_px = R.stats_px; r->ksplit = R.ksplit;
    r->reserved = 0;
    r->grid = R.grid;
    r->scratch_floats = used;
    r->partial_floats = splitk_partial_floats(L, R);
}

extern "C" int dlpm_conv_policy_route(const dlpm_conv_args *a, int32_t generation, int64_t dispatch_batch, dlpm_conv_route *route) {
    DLPM_CHECK_ARG(route, "dlpm_conv_policy_route: null argument");
    ConvLaunch L;
    float *at[CONV_LAYOUT_COUNT] = {};
    unsigned mask = 0;
    int64_t used = 0;
    // (a base that is never dereferenced, as the plan's dry run: conv_route asks only which layouts a launch carries)
    TRY(policy_launch(a, generation, dispatch_batch, reinterpret_cast<float *>(uintptr_t(1) << 20), &L, at, &mask, &used));
    policy_route_out(L, conv_route(L), used, route);
    return DLPM_OK;
}

extern "C" int dlpm_conv_policy_f32(const dlpm_conv_args *a, int32_t generation, int64_t dispatch_batch, float *scratch_dev,
                                    float *partial_dev, int64_t partial_floats, float *stats_out, int32_t *stats_px, dlpm_conv_route *route,
                                    dlpm_stream_t stream) {
    DLPM_CHECK_ARG(a && a->src0 && a->weight && a->out && scratch_dev, "dlpm_conv_policy_f32: null argument");
    DLPM_CHECK_ARG((a->C1 == 0) == (a->src1 == nullptr), "dlpm_conv_policy_f32: src1/C1 mismatch");
    DLPM_CHECK_ARG((stats_out == nullptr) == (stats_px == nullptr), "dlpm_conv_policy_f32: stats_out and stats_px go together");
    ConvLaunch L;
    float *at[CONV_LAYOUT_COUNT] = {};
    unsigned mask = 0;
    int64_t used = 0;
    TRY(policy_launch(a, generation, dispatch_batch, scratch_dev, &L, at, &mask, &used));
    const ConvRoute R = conv_route(L);
    const int64_t need = splitk_partial_floats(L, R);
    if (a->scratch_floats < used) {
        set_error("dlpm_conv_policy_f32: the weight layouts of this layer take %lld floats of scratch, %lld given", (long long)used,
                  (long long)a->scratch_floats);
        return DLPM_ERR_NOMEM;
    }
    if (need > 0 && (!partial_dev || partial_floats < need)) {
        set_error("dlpm_conv_policy_f32: split-K over %d copies writes %lld floats of partial outputs, %lld given", R.ksplit, (long long)need,
                  (long long)(partial_dev ? partial_floats : 0));
        return DLPM_ERR_NOMEM;
    }
    if (stats_out && R.stats_px <= 0) {
        set_error("dlpm_conv_policy_f32: this launch emits no statistics (a split-K launch, or a kernel whose partials would not lie inside one image)");
        return DLPM_ERR_UNSUPPORTED;
    }
    hipStream_t st = as_stream(stream);
    TRY(build_conv_layouts(L, mask, a->weight, at, st));
    if (stats_out) {
        L.stats_out = reinterpret_cast<float2 *>(stats_out);
        *stats_px = R.stats_px;
    }
    if (route) policy_route_out(L, R, used, route);
    return launch_conv_splitk(L, R, partial_dev, st);
}

extern "C" int dlpm_groupnorm_coeffs_f32(const float *src0, const float *src1, int32_t C0, int32_t C1, int32_t B, int32_t HW,
                                         int32_t groups, const float *gamma, const float *beta, const float *ss,
                                         int64_t ss_stride, int64_t ss_offset, float *coefA, float *coefB,
                                         dlpm_stream_t stream) {
    DLPM_CHECK_ARG(src0 && gamma && beta && coefA && coefB, "dlpm_groupnorm_coeffs_f32: null argument");
    DLPM_CHECK_ARG(groups > 0 && (C0 + C1) % groups == 0, "dlpm_groupnorm_coeffs_f32: %d channels not divisible by %d groups",
                   C0 + C1, groups);
    return launch_gn_coeffs(src0, src1, C0, C1, B, HW, groups, gamma, beta, ss, ss_stride, ss_offset, coefA, coefB,
                            as_stream(stream));
}

extern "C" int dlpm_groupnorm_coeffs_from_stats_f32(const float *st0, const float *st1, int32_t C0, int32_t C1, int32_t B, int32_t nt0,
                                                    int32_t nt1, int32_t HW, int32_t groups, const float *gamma, const float *beta,
                                                    const float *ss, int64_t ss_stride, int64_t ss_offset, float *coefA, float *coefB,
                                                    dlpm_stream_t stream) {
    DLPM_CHECK_ARG(st0 && gamma && beta && coefA && coefB, "dlpm_groupnorm_coeffs_from_stats_f32: null argument");
    DLPM_CHECK_ARG((C1 == 0) == (st1 == nullptr), "dlpm_groupnorm_coeffs_from_stats_f32: st1/C1 mismatch");
    DLPM_CHECK_ARG(groups > 0 && (C0 + C1) % groups == 0, "dlpm_groupnorm_coeffs_from_stats_f32: %d channels not divisible by %d groups",
                   C0 + C1, groups);
    DLPM_CHECK_ARG(C0 > 0 && C1 >= 0 && B > 0 && HW > 0, "dlpm_groupnorm_coeffs_from_stats_f32: C0 %d, C1 %d, B %d, HW %d", C0, C1, B, HW);
    DLPM_CHECK_ARG(nt0 > 0 && HW % nt0 == 0 && (C1 == 0 || (nt1 > 0 && HW % nt1 == 0)),
                   "dlpm_groupnorm_coeffs_from_stats_f32: %d / %d partials do not divide %d pixels", nt0, nt1, HW);
    return launch_gn_coeffs_from_stats(reinterpret_cast<const float2 *>(st0), reinterpret_cast<const float2 *>(st1), C0, C1, B, nt0,
                                       C1 ? nt1 : 1, HW, groups, gamma, beta, ss, ss_stride, ss_offset, coefA, coefB, as_stream(stream));
}

extern "C" int dlpm_attention_f32(const float *qkv, float *out, int32_t B, int32_t T, int32_t C, int32_t heads,
                                  dlpm_stream_t stream) {
    DLPM_CHECK_ARG(qkv && out && B > 0, "dlpm_attention_f32: null argument");
    return launch_attention(qkv, out, B, T, C, heads, as_stream(stream));
}

extern "C" int dlpm_attention_general_f32(const float *qkv, float *out, int32_t B, int32_t T, int32_t C, int32_t heads,
                                          dlpm_stream_t stream) {
    DLPM_CHECK_ARG(qkv && out && B > 0, "dlpm_attention_general_f32: null argument");
    return launch_attention_general(qkv, out, B, T, C, heads, as_stream(stream));
}

extern "C" int dlpm_resblock_small_f32(const dlpm_resblock_args *a, float *scratch_dev, int64_t scratch_floats, dlpm_stream_t stream) {
    DLPM_CHECK_ARG(a && a->x0 && a->conv1_w && a->conv2_w && a->ss && a->out && scratch_dev, "dlpm_resblock_small_f32: null argument");
    // every parameter the kernel reads at entry (it has no optional ones but the skip convolution and the statistics)
    DLPM_CHECK_ARG(a->gn1_w && a->gn1_b && a->gn2_w && a->gn2_b && a->conv1_b && a->conv2_b, "dlpm_resblock_small_f32: null GroupNorm / bias parameter");
    DLPM_CHECK_ARG(!a->skip_w || a->skip_b, "dlpm_resblock_small_f32: skip_w without skip_b");
    DLPM_CHECK_ARG(a->B > 0 && a->H == a->W && (a->H == 8 || a->H == 4), "dlpm_resblock_small_f32: B %d, %d x %d images (8x8 or 4x4)", a->B, a->H, a->W);
    DLPM_CHECK_ARG((a->C1 == 0) == (a->x1 == nullptr), "dlpm_resblock_small_f32: x1/C1 mismatch");
    const int Cin = a->C0 + a->C1;
    const int64_t n1 = (int64_t)64 * Cin * 9, n2 = (int64_t)64 * 64 * 9, ns = a->skip_w ? (int64_t)64 * Cin : 0;
    DLPM_CHECK_ARG(scratch_floats >= n1 + n2 + ns, "dlpm_resblock_small_f32: scratch of %lld floats, need %lld", (long long)scratch_floats,
                   (long long)(n1 + n2 + ns));
    DLPM_CHECK_ARG(small_weight_ok(64, Cin, 3), "dlpm_resblock_small_f32: %d input channels (64 or 128)", Cin);
    hipStream_t st = as_stream(stream);
    ResSmallLaunch r;
    r.x0 = a->x0; r.x1 = a->x1; r.C0 = a->C0; r.C1 = a->C1; r.B = a->B; r.H = a->H; r.W = a->W;
    r.gn1_w = a->gn1_w; r.gn1_b = a->gn1_b; r.gn2_w = a->gn2_w; r.gn2_b = a->gn2_b;
    r.w1f = scratch_dev; r.b1 = a->conv1_b; r.w2f = scratch_dev + n1; r.b2 = a->conv2_b;
    r.wsf = a->skip_w ? scratch_dev + n1 + n2 : nullptr; r.bs = a->skip_b;
    r.emb = a->ss; r.emb_stride = a->ss_stride; r.emb_off = 0;
    r.out = a->out; r.stats_out = reinterpret_cast<float2 *>(a->stats_out);
    // (asked before the first launch: a refused block leaves the scratch untouched)
    if (!res_small_ok(r)) {
        if (!small_blocks_enabled())
            set_error("dlpm_resblock_small_f32: the fused blocks are switched off (DLPM_NO_FUSED_BLOCKS=1)");
        else
            set_error("dlpm_resblock_small_f32: %d + %d input channels %s skip_w (each source a multiple of 4; skip_w exactly when C0 + C1 = 128)",
                      a->C0, a->C1, a->skip_w ? "with" : "without");
        return DLPM_ERR_UNSUPPORTED;
    }
    TRY(relayout_weight_small(a->conv1_w, scratch_dev, 64, Cin, 3, st));
    TRY(relayout_weight_small(a->conv2_w, scratch_dev + n1, 64, 64, 3, st));
    if (a->skip_w) TRY(relayout_weight_small(a->skip_w, scratch_dev + n1 + n2, 64, Cin, 1, st));
    return launch_resblock_small(r, st);
}

extern "C" int64_t dlpm_resblock_img_scratch_floats(int64_t B, int32_t Cin) {
    if (B <= 0 || Cin <= 0) return -1;
    // (sized for either shape: 32 channels on 32x32 images, 64 channels on 16x16 ones)
    return wino4_weight_floats(64, Cin) + wino4_weight_floats(64, 64) + 2 * B * Cin + 2 * B * 1024 * 32 + 64;
}

extern "C" int dlpm_resblock_img_f32(const dlpm_resblock_args *a, float *scratch_dev, int64_t scratch_floats, dlpm_stream_t stream) {
    DLPM_CHECK_ARG(a && a->x0 && a->conv1_w && a->conv2_w && a->ss && a->out && scratch_dev, "dlpm_resblock_img_f32: null argument");
    DLPM_CHECK_ARG(a->gn1_w && a->gn1_b && a->gn2_w && a->gn2_b && a->conv1_b && a->conv2_b, "dlpm_resblock_img_f32: null GroupNorm / bias parameter");
    DLPM_CHECK_ARG(a->B > 0 && a->H == a->W && (a->H == 32 || a->H == 16), "dlpm_resblock_img_f32: B %d, %d x %d images (32x32 or 16x16)", a->B, a->H, a->W);
    const int CO = a->H == 32 ? 32 : 64, HW = a->H * a->W;
    DLPM_CHECK_ARG((a->C1 == 0) == (a->x1 == nullptr), "dlpm_resblock_img_f32: x1/C1 mismatch");
    const int Cin = a->C0 + a->C1;
    DLPM_CHECK_ARG(Cin >= 32 && Cin <= 128 && Cin % 8 == 0 && a->C0 % 8 == 0, "dlpm_resblock_img_f32: %d + %d input channels", a->C0, a->C1);
    DLPM_CHECK_ARG((Cin == CO) == (a->skip_w == nullptr) && (!a->skip_w || a->skip_b), "dlpm_resblock_img_f32: skip_w / skip_b (required unless C0 + C1 = the output channels)");
    DLPM_CHECK_ARG(res_img_residual_ok(a->skip_w != nullptr, a->C1),
                   "dlpm_resblock_img_f32: a concat input (C1 = %d) needs the skip weights skip_w / skip_b: without them the residual is x0 alone, %d of the %d channels per pixel",
                   a->C1, a->C0, CO);
    DLPM_CHECK_ARG(scratch_floats >= dlpm_resblock_img_scratch_floats(a->B, Cin), "dlpm_resblock_img_f32: scratch of %lld floats, need %lld",
                   (long long)scratch_floats, (long long)dlpm_resblock_img_scratch_floats(a->B, Cin));
    hipStream_t st = as_stream(stream);
    float *w1 = scratch_dev, *w2 = w1 + wino4_weight_floats(CO, Cin), *cA = w2 + wino4_weight_floats(CO, CO), *cB = cA + (int64_t)a->B * Cin;
    float *hb = cB + (int64_t)a->B * Cin, *sk = hb + (int64_t)a->B * HW * CO;
    hb += (64 - ((hb - scratch_dev) & 63)) & 63;          // (16-byte rows: float4 staging loads)
    sk = hb + (int64_t)a->B * HW * CO;
    ResImgLaunch r;
    r.x0 = a->x0; r.x1 = a->x1; r.C0 = a->C0; r.C1 = a->C1; r.B = a->B; r.H = a->H;
    r.coefA1 = cA; r.coefB1 = cB;
    r.gn1_w = a->gn1_w; r.gn1_b = a->gn1_b; r.gn2_w = a->gn2_w; r.gn2_b = a->gn2_b;
    r.w1 = w1; r.b1 = a->conv1_b; r.w2 = w2; r.b2 = a->conv2_b;
    r.emb = a->ss; r.emb_stride = a->ss_stride; r.emb_off = 0;
    r.hbuf = hb; r.out = a->out; r.stats_out = reinterpret_cast<float2 *>(a->stats_out);
    r.res = a->skip_w ? sk : a->x0;
    ConvLaunch s;
    if (a->skip_w) {
        s.src0 = a->x0; s.src1 = a->x1; s.C0 = a->C0; s.C1 = a->C1; s.B = a->B; s.Hin = s.Hout = a->H; s.Win = s.Wout = a->W;
        s.ks = 1; s.Cout = CO; s.w = a->skip_w; s.bias = a->skip_b; s.out = sk; s.gemm = DLPM_GEMM_F32;
        // (skip_w is in the reference's [O][I] layout, which is the implicit GEMM's: the direct kernel would misread it)
        DLPM_CHECK_ARG(igemm_supported(s), "dlpm_resblock_img_f32: the skip convolution takes %d + %d input channels only in multiples of 32 per source", a->C0, a->C1);
    }
    // (every refusal before the first launch: a refused block leaves the scratch untouched)
    if (!res_img_ok(r)) {
        ResImgLaunch plain = r;      // 64 input channels from one source: refused only when the kernel is switched off
        plain.C0 = 64; plain.C1 = 0;
        if (!res_img_ok(plain))
            set_error("dlpm_resblock_img_f32: the whole-image ResBlock kernel is switched off (DLPM_RES_IMG=0 / DLPM_RES_IMG16=0 / DLPM_WINO_F4=0)");
        else
            set_error("dlpm_resblock_img_f32: the whole-image ResBlock kernel does not take %d + %d input channels on %d x %d images", a->C0, a->C1, a->H, a->W);
        return DLPM_ERR_UNSUPPORTED;
    }
    TRY(relayout_weight_wino4(a->conv1_w, w1, CO, Cin, st));
    TRY(relayout_weight_wino4(a->conv2_w, w2, CO, CO, st));
    TRY(launch_gn_coeffs(a->x0, a->x1, a->C0, a->C1, a->B, HW, 32, a->gn1_w, a->gn1_b, nullptr, 0, 0, cA, cB, st));
    if (a->skip_w) TRY(launch_conv(s, nullptr, nullptr, st));
    return launch_resblock_img(r, st);
}

extern "C" int dlpm_attnblock_small_f32(const dlpm_attnblock_args *a, float *scratch_dev, int64_t scratch_floats, dlpm_stream_t stream) {
    DLPM_CHECK_ARG(a && a->x && a->qkv_w && a->proj_w && a->out && scratch_dev, "dlpm_attnblock_small_f32: null argument");
    DLPM_CHECK_ARG(a->gn_w && a->gn_b && a->qkv_b && a->proj_b, "dlpm_attnblock_small_f32: null GroupNorm / bias parameter");
    DLPM_CHECK_ARG(a->B > 0 && a->H == a->W && (a->H == 16 || a->H == 8 || a->H == 4), "dlpm_attnblock_small_f32: B %d, %d x %d images (16x16, 8x8 or 4x4)", a->B, a->H, a->W);
    DLPM_CHECK_ARG(a->C == 64 && a->heads == 4, "dlpm_attnblock_small_f32: 64 channels, 4 heads (got %d, %d)", a->C, a->heads);
    const int64_t nq = (int64_t)192 * 64, np = (int64_t)64 * 64;
    DLPM_CHECK_ARG(scratch_floats >= nq + np, "dlpm_attnblock_small_f32: scratch of %lld floats, need %lld", (long long)scratch_floats,
                   (long long)(nq + np));
    hipStream_t st = as_stream(stream);
    TRY(relayout_weight_small(a->qkv_w, scratch_dev, 192, 64, 1, st));
    TRY(relayout_weight_small(a->proj_w, scratch_dev + nq, 64, 64, 1, st));
    AttnSmallLaunch l;
    l.x = a->x; l.C = a->C; l.heads = a->heads; l.B = a->B; l.H = a->H; l.W = a->W;
    l.gn_w = a->gn_w; l.gn_b = a->gn_b; l.wqkv = scratch_dev; l.bqkv = a->qkv_b; l.wproj = scratch_dev + nq; l.bproj = a->proj_b;
    l.out = a->out; l.stats_out = reinterpret_cast<float2 *>(a->stats_out);
    return a->H == 16 ? launch_attnblock16(l, st) : launch_attnblock_small(l, st);
}

extern "C" int dlpm_timestep_embedding_f32(const float *t, float *emb, int64_t B, int32_t dim, dlpm_stream_t stream) {
    DLPM_CHECK_ARG(t && emb && B > 0 && dim > 0, "dlpm_timestep_embedding_f32: bad argument");
    return launch_timestep_embedding(t, emb, B, dim, as_stream(stream));
}
