// sampler.hip -- the reverse-time loop x_T -> x_0 as a replayed hipGraph.
//
// Replaces p_sample_loop_progressive / ddim_sample_loop_progressive
// (dlpm/methods/GenerativeLevyProcess.py:291-330, 418-452).  One reverse step is
//     tvec <- t/T ; eps <- model(x, tvec) ; x <- update(x, eps, tables[t]) ; t <- t - 1
// Every per-step scalar is read from device tables indexed by a device-resident step counter, so
// the captured graph of ONE step is replayed T-1 times with no host patching in between.
#include <vector>

#include "common.h"
#include "../../include/dlpm_amd_chains.h"

using namespace dlpm;

extern "C" int dlpm_mlp_forward(dlpm_mlp *, const float *, const float *, float *, int64_t, dlpm_stream_t);
extern "C" int32_t dlpm_mlp_tile_rows(const dlpm_mlp *);   // > 0: the net takes the general forward (include/dlpm_amd_mlp.h)

struct dlpm_sampler {
    dlpm_sampler_config cfg;
    int64_t D = 0;
    float *g = nullptr, *bg = nullptr, *s = nullptr, *bs = nullptr;  // device schedule [T]
    float bs_last = 0.f;
    float *A = nullptr, *c_eps = nullptr, *c_noise = nullptr;         // [T,B]; [T,B,D] when non-isotropic
    bool elem = false;             // DLPM_UPD_ELEMENTWISE: per-element tables
    int64_t cols = 0;              // table columns: B, or B*D when non-isotropic
    bool lim = false;              // DLPM_SMP_LIM: continuous-time LIM updates (T = steps + 1)
    float *lim_ts = nullptr, *lim_tmp = nullptr, *lim_cx = nullptr, *lim_cs = nullptr, *lim_cn = nullptr;
    float *in_scale = nullptr, *xin = nullptr;   // input_scaling table [T] and the scaled copy the net reads
    float **hist_cell = nullptr;   // device cell with the history base (see dlpm_update_args::hist_pp)
    float *hist = nullptr;         // its current value (caller-owned [T,B,D] buffer or null)
    float *x = nullptr, *eps = nullptr, *tvec = nullptr;
    float *emb_tab = nullptr;      // UNet, DLPM loop: the time path's output for every step, [T][emb width] (dlpm_unet_time_embeddings);
                                   // class-conditional net: the time MLP's output for every step, [T][4 * model_channels]
    bool cond = false;             // the UNet is class-conditional: every forward reads `labels`
    int64_t *labels = nullptr;     // [B] class labels (dlpm_sampler_set_labels), read by the captured graph
    bool labels_set = false;
    int32_t *t_dev = nullptr;
    uint64_t *key_dev = nullptr;   // {seed, sample_offset}: read by the update kernel, so reseeding keeps the graph; one pair per
                                   // chain ({seed, sample_offset + first row of the chain}), the whole batch's = chain 0's first
    int graph_steps = 0;           // steps inside the captured graph
    void *ws = nullptr;
    int64_t ws_bytes = 0;
    int32_t t_host = 0;
    int64_t plan_version = 0;      // dlpm_unet_plan_version at capture / workspace sizing time
    bool key_dirty = false;        // dlpm_sampler_reseed happened: key_dev is rewritten by the next begin*()
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    // Graph capture is illegal on the legacy default stream (which is what torch hands out by
    // default), so graph work runs on a private non-blocking stream fenced to the caller's stream
    // with events at both ends of every dlpm_sampler_steps call.
    hipStream_t own = nullptr;
    hipEvent_t ev_in = nullptr, ev_out = nullptr;
    // The two-chain step (one_step): rows [0, B/2) on the stream of the step, rows [B/2, B) on `side`, forked and joined with
    // events -- under capture two parallel branches of the one graph.  `chains` is what the net, the variant and the workspace
    // admit (chain_layout: 1 or 2); rows and arenas per chain below.
    int chains = 1;
    int64_t row0[DLPM_MAX_CHAINS] = {0, 0}, nrows[DLPM_MAX_CHAINS] = {0, 0};
    int64_t ws_off[DLPM_MAX_CHAINS] = {0, 0}, ws_len[DLPM_MAX_CHAINS] = {0, 0};
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    int graph_chains = 0;          // chains of the step the live graph was captured with
    int64_t captures = 0;          // graphs captured so far (dlpm_sampler_graph_captures)
};

namespace {

__global__ void k_set_t(int32_t *t, int32_t v) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *t = v;
}
__global__ void k_set_key(uint64_t *key, uint64_t seed, uint64_t offset, uint64_t row1) {
    if (threadIdx.x == 0 && blockIdx.x == 0) { key[0] = seed; key[1] = offset; key[2] = seed; key[3] = offset + row1; }
}
__global__ void k_set_ptr(float **cell, float *v) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *cell = v;
}

#define TRY(expr)                     \
    do {                              \
        int _r = (expr);              \
        if (_r != DLPM_OK) return _r; \
    } while (0)

// The time path (time embedding -> MLP -> per-ResBlock emb linears) is a function of the step index alone: one row per step,
// computed with the kernels the forward would run (t = float(i) * (1 / T), k_fill_t's arithmetic), replaces four launches of
// every step.  DLPM loop only (the LIM loop feeds its own time grid).  DLPM_NO_TIME_TABLE=1: off.  The rows depend on the net's
// WEIGHTS and on its GEMM policy, so sync_plan() rebuilds them whenever the net's plan version moved under a live sampler
// (dlpm_unet_set_param + dlpm_unet_finalize, dlpm_unet_set_gemm_policy): round 3 built them once at create, and a sampler that
// outlived a weight upload or a pipe switch kept conditioning on the old rows.
int build_time_table(dlpm_sampler *s) {
    if (!s->cfg.unet || s->lim) return DLPM_OK;
    const char *nt = getenv("DLPM_NO_TIME_TABLE");
    // a conditional net's emb rows depend on the label: the table holds the time MLP's rows, the label term and the emb linears
    // run in every step (per sample, as in every other forward of such a net)
    const int64_t ew = s->cond ? unet_time_mlp_width(s->cfg.unet) : dlpm_unet_time_embedding_width(s->cfg.unet);
    if ((nt && nt[0] == '1') || ew <= 0) return DLPM_OK;
    const int T = s->cfg.T;
    std::vector<float> tv(T);
    for (int i = 0; i < T; i++) tv[i] = (float)i * (1.0f / (float)T);
    float *tv_dev = nullptr;
    void *scr = nullptr;
    const int64_t scr_bytes = dlpm_unet_time_embeddings_scratch_bytes(s->cfg.unet, T);
    int r = DLPM_OK;
    hipError_t e = hipMalloc(&tv_dev, T * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(tv_dev, tv.data(), T * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc(&scr, (size_t)scr_bytes);
    if (e == hipSuccess && !s->emb_tab) e = hipMalloc(&s->emb_tab, (size_t)T * ew * sizeof(float));
    if (e == hipSuccess) {
        r = s->cond ? unet_time_mlp_rows(s->cfg.unet, tv_dev, T, s->emb_tab, scr, scr_bytes, nullptr)
                    : dlpm_unet_time_embeddings(s->cfg.unet, tv_dev, T, s->emb_tab, scr, scr_bytes, nullptr);
        e = hipDeviceSynchronize();
    }
    if (tv_dev) (void)hipFree(tv_dev);
    if (scr) (void)hipFree(scr);
    if (e != hipSuccess) {
        set_error("dlpm_sampler: time table: %s", hipGetErrorString(e));
        return DLPM_ERR_HIP;
    }
    return r;
}

// DLPM_SAMPLER_CHAINS (read once): 1 = every step is one chain of kernels on one stream, 2 (default) = two half-batch chains where
// the step admits them
int chains_wanted() {
    static int v = -1;
    if (v < 0) { const char *e = getenv("DLPM_SAMPLER_CHAINS"); v = (e && e[0] == '1' && !e[1]) ? 1 : 2; }
    return v;
}

void drop_graph(dlpm_sampler *s) {
    if (s->exec) (void)hipGraphExecDestroy(s->exec);
    if (s->graph) (void)hipGraphDestroy(s->graph);
    s->exec = nullptr;
    s->graph = nullptr;
    s->graph_chains = 0;
}

// Rows and arenas of the chains, and the workspace the sampler needs: *need = the single arena of B, or the two arenas together
// where they exceed it by the rounding of the arena's blocks (they are both walks of the same plan, every block of which is
// proportional to the batch: dlpm_unet_chain_workspace).  What of the step can be decided once per sampler and plan is decided here;
// history, injected z and the profiling pass are looked at per step (chains_now).
// The chained form needs B >= 2: kernel choice reads the DECLARED dispatch batch and the layer alone (conv_route: conv_wino4.hip
// wino4_nq_for, the split-K factor; the block_small selectors), never the batch of a launch, so the declared
// policy keeps its kernels down to a chain of ONE sample and the threshold is 2 x 1.  An odd B splits as B/2 and B - B/2 rows.
// One chain stays: the MLP sampler; LIM, DLIM, clip and non-isotropic tables; mean types other than eps (predict + update run as
// kernels of their own); label-conditional nets; input scaling (its scaled copy is one buffer); a net whose head cannot carry the
// update; a half-batch whose first row is not 16-byte aligned in the state (the fused head stores float4).
int chain_layout(dlpm_sampler *s, int64_t *need) {
    const dlpm_sampler_config &c = s->cfg;
    s->chains = 1;
    s->row0[0] = 0; s->nrows[0] = c.B; s->ws_off[0] = 0;
    const int64_t single = dlpm_unet_workspace_bytes(c.unet, c.B);
    if (single < 0) return DLPM_ERR_STATE;
    s->ws_len[0] = single;
    *need = single;
    const bool plain = !s->lim && !s->elem && !s->cond && !s->in_scale && c.mean_type == DLPM_MEAN_EPSILON &&
                       !(c.flags & (DLPM_UPD_DLIM | DLPM_UPD_CLIP | DLPM_UPD_ELEMENTWISE));
    if (chains_wanted() < 2 || !plain || c.B < 2 || !unet_head_carries_update(c.unet) || ((c.B / 2) * s->D) % 4 != 0) return DLPM_OK;
    int64_t r0[DLPM_MAX_CHAINS], n[DLPM_MAX_CHAINS], off[DLPM_MAX_CHAINS], len[DLPM_MAX_CHAINS], one = 0, slack = 0;
    const int64_t both = dlpm_unet_chain_workspace(c.unet, c.B, 2, r0, n, off, len, &one, &slack);
    if (both < 0) return DLPM_ERR_STATE;
    // The halves must not cost memory the whole does not.  Both are walks of one plan whose blocks are proportional to the batch,
    // so the two peaks exceed the one by the rounding of the blocks at most -- unless a best-fit choice of the arena falls the
    // other way at the smaller size, which no configuration here does; such a batch stays on one chain.
    if (both > one + slack) return DLPM_OK;
    s->chains = 2;
    for (int i = 0; i < 2; i++) { s->row0[i] = r0[i]; s->nrows[i] = n[i]; s->ws_off[i] = off[i]; s->ws_len[i] = len[i]; }
    if (both > *need) *need = both;
    return DLPM_OK;
}

// The net's launch plan may change under a live sampler (dlpm_unet_set_conv_policy / set_gemm_policy, re-uploaded weights):
// drop the captured graph, re-size the activation workspace and rebuild the time table before the next step.
int sync_plan(dlpm_sampler *s) {
    if (!s->cfg.unet) return DLPM_OK;
    const int64_t v = dlpm_unet_plan_version(s->cfg.unet);
    if (v == s->plan_version) return DLPM_OK;
    DLPM_HIP(hipDeviceSynchronize());
    drop_graph(s);
    int64_t need = 0;
    TRY(chain_layout(s, &need));
    s->key_dirty = true;           // (the second chain's first row may have moved with the layout)
    if (need > s->ws_bytes) {
        if (s->ws) DLPM_HIP(hipFree(s->ws));
        s->ws = nullptr;
        DLPM_HIP(hipMalloc(&s->ws, (size_t)need));
        s->ws_bytes = need;
    }
    if (s->emb_tab) TRY(build_time_table(s));
    s->plan_version = v;
    return DLPM_OK;
}

// RAII: the net reads its time path from the sampler's table while one of the sampler's forward calls is being enqueued
struct TimeTableBinding {
    dlpm_unet *u = nullptr;
    explicit TimeTableBinding(const dlpm_sampler *s) {
        if (s->cfg.unet && s->emb_tab) {
            u = s->cfg.unet;
            (void)dlpm_unet_bind_time_table(u, s->emb_tab, s->t_dev);
        }
    }
    ~TimeTableBinding() {
        if (u) (void)dlpm_unet_bind_time_table(u, nullptr, nullptr);
    }
};

int model_forward(dlpm_sampler *s, hipStream_t st) {
    TimeTableBinding bound(s);
    const float *xin = s->x;
    if (s->in_scale) {
        TRY(dlpm_scale_by_table_f32(s->x, s->xin, s->cfg.B * s->D, s->t_dev, s->in_scale, st));
        xin = s->xin;
    }
    if (s->cond)
        return dlpm_unet_forward_uniform_t_labels(s->cfg.unet, xin, s->tvec, s->labels, s->eps, s->cfg.B, s->ws, s->ws_bytes, st);
    if (s->cfg.unet)
        return dlpm_unet_forward_uniform_t(s->cfg.unet, xin, s->tvec, s->eps, s->cfg.B, s->ws, s->ws_bytes, st);   // t = [i] * B
    return dlpm_mlp_forward(s->cfg.mlp, xin, s->tvec, s->eps, s->cfg.B, st);
}

// chains of the next plain step: what chain_layout admitted, unless this step records history (the history row is addressed through
// a device cell, whole batch only), takes injected z, or runs under the per-launch profiler (one stream, one launch at a time)
int chains_now(const dlpm_sampler *s, const float *z) { return (s->chains == 2 && !s->hist && !z && !prof_enabled()) ? 2 : 1; }

int one_step(dlpm_sampler *s, const float *z, bool advance, hipStream_t st) {
    if (s->lim) {
        TRY(dlpm_fill_table_t_f32(s->tvec, s->t_dev, s->lim_ts, s->cfg.T, s->cfg.B, st));
        TRY(model_forward(s, st));
        dlpm_lim_update_args a{};
        a.x_dev = s->x; a.eps_dev = s->eps; a.z_dev = z; a.t_dev = s->t_dev;
        a.tmp_dev = s->lim_tmp; a.cx_dev = s->lim_cx; a.cs_dev = s->lim_cs; a.cn_dev = s->lim_cn;
        a.A_dev = s->cfg.alpha == 2.0 ? nullptr : s->A;      // alpha = 2: e_B = randn_like(x) (sampler.py:135)
        a.B = s->cfg.B; a.D = s->D; a.T = s->cfg.T;
        a.flags = (s->cfg.flags & DLPM_UPD_DLIM) | (advance ? DLPM_UPD_ADVANCE : 0) | (s->hist ? DLPM_UPD_HIST_ON : 0);
        a.clamp_eps = (float)s->cfg.clamp_eps;
        a.seed = s->cfg.seed; a.sample_offset = s->cfg.sample_offset; a.key_dev = s->key_dev;
        a.hist_pp = s->hist_cell;
        return dlpm_lim_update_f32(&a, st);
    }
    // (with the time table bound the UNet reads its row by the step counter and never looks at tvec: one launch less per step)
    if (!(s->cfg.unet && s->emb_tab)) TRY(dlpm_fill_scaled_t_f32(s->tvec, s->t_dev, s->cfg.T, s->cfg.B, st));
    dlpm_update_args a{};
    a.x_dev = s->x; a.eps_dev = s->eps; a.z_dev = z; a.t_dev = s->t_dev;
    a.g_dev = s->g; a.bg_dev = s->bg; a.bs_dev = s->bs;
    a.c_eps_dev = s->c_eps; a.c_noise_dev = s->c_noise; a.A_dev = s->A;
    a.B = s->cfg.B; a.D = s->D; a.T = s->cfg.T;
    a.flags = (s->cfg.flags & (DLPM_UPD_DLIM | DLPM_UPD_CLIP | DLPM_UPD_ELEMENTWISE)) | (advance ? DLPM_UPD_ADVANCE : 0) |
              (s->hist ? DLPM_UPD_HIST_ON : 0);
    a.hist_pp = s->hist_cell;
    a.dlim_eta = s->cfg.dlim_eta; a.alpha = (float)s->cfg.alpha;
    a.seed = s->cfg.seed; a.sample_offset = s->cfg.sample_offset; a.key_dev = s->key_dev;
    if (s->cfg.mean_type != DLPM_MEAN_EPSILON) {
        // the net predicts x_0 / z_t / the anterior mean: model output -> x_0 -> (clamp) -> eps in one pass over the eps buffer
        // (p_mean_variance's else-branch, GenerativeLevyProcess.py:185-207), then the plain step
        TRY(model_forward(s, st));
        dlpm_predict_args q{};
        q.x_dev = s->x; q.in_dev = s->eps; q.out_dev = s->eps; q.t_dev = s->t_dev;
        q.g_dev = s->g; q.bg_dev = s->bg; q.bs_dev = s->bs; q.c_eps_dev = s->c_eps; q.A_dev = s->A;
        q.B = s->cfg.B; q.D = s->D; q.T = s->cfg.T; q.mean_type = s->cfg.mean_type;
        q.flags = DLPM_PRED_TO_XSTART | DLPM_PRED_TO_EPS | ((s->cfg.flags & DLPM_UPD_CLIP) ? DLPM_PRED_CLIP : 0) |
                  (s->elem ? DLPM_PRED_ELEMENTWISE : 0);
        TRY(dlpm_predict_f32(&q, st));
        a.flags &= ~DLPM_UPD_CLIP;
        return dlpm_update_f32(&a, st);
    }
    if (s->cfg.unet && chains_now(s, z) == 2) {
        // Two independent chains of kernels, one per half of the batch: nothing of a step crosses samples before the state is
        // read back (GroupNorm statistics are per image, the noise is keyed by global sample index, the step counter is only
        // read), so while one chain sits in a launch gap, a one-workgroup coefficient kernel or an epilogue burst the other's
        // convolution has the CUs.  Each chain launches the kernels the whole batch would (the policy reads the declared batch).
        if (!s->side) {
            DLPM_HIP(hipStreamCreateWithFlags(&s->side, hipStreamNonBlocking));
            DLPM_HIP(hipEventCreateWithFlags(&s->ev_fork, hipEventDisableTiming));
            DLPM_HIP(hipEventCreateWithFlags(&s->ev_join, hipEventDisableTiming));
        }
        DLPM_HIP(hipEventRecord(s->ev_fork, st));
        DLPM_HIP(hipStreamWaitEvent(s->side, s->ev_fork, 0));
        TimeTableBinding bound(s);
        a.flags &= ~(DLPM_UPD_ADVANCE | DLPM_UPD_HIST_ON);
        a.hist_pp = nullptr;
        int r = DLPM_OK;
        for (int c = 0; c < 2 && r == DLPM_OK; c++) {
            dlpm_update_args h = a;             // h.B stays the row pitch of the [T,B] tables
            h.x_dev = s->x + s->row0[c] * s->D;
            h.c_eps_dev = s->c_eps + s->row0[c];
            h.c_noise_dev = s->c_noise + s->row0[c];
            h.sample_offset = s->cfg.sample_offset + s->row0[c];
            h.key_dev = s->key_dev + 2 * c;
            r = unet_forward_update_rows(s->cfg.unet, h.x_dev, s->tvec, &h, s->nrows[c], static_cast<char *>(s->ws) + s->ws_off[c],
                                         s->ws_len[c], c == 0 ? st : s->side);
        }
        // join even after a failed enqueue: a capture in progress must not be left with an unjoined branch
        DLPM_HIP(hipEventRecord(s->ev_join, s->side));
        DLPM_HIP(hipStreamWaitEvent(st, s->ev_join, 0));
        TRY(r);
        return advance ? launch_step_advance(s->t_dev, st) : DLPM_OK;   // both chains have read t
    }
    if (s->cfg.unet) {   // the UNet's head convolution applies the update itself where the variant allows (eps stays on chip)
        const float *xin = s->x;
        if (s->in_scale) {
            TRY(dlpm_scale_by_table_f32(s->x, s->xin, s->cfg.B * s->D, s->t_dev, s->in_scale, st));
            xin = s->xin;
        }
        TimeTableBinding bound(s);
        return unet_forward_update_labels(s->cfg.unet, xin, s->tvec, s->cond ? s->labels : nullptr, &a, s->eps, s->cfg.B, s->ws,
                                          s->ws_bytes, st);
    }
    TRY(model_forward(s, st));
    return dlpm_update_f32(&a, st);
}

int flush_key(dlpm_sampler *s, hipStream_t st) {
    if (!s->key_dirty) return DLPM_OK;
    k_set_key<<<1, 64, 0, st>>>(s->key_dev, s->cfg.seed, (uint64_t)s->cfg.sample_offset, (uint64_t)s->row0[1]);
    DLPM_LAUNCH_CHECK();
    s->key_dirty = false;
    return DLPM_OK;
}

// a conditional net samples nothing before dlpm_sampler_set_labels
int need_labels(const dlpm_sampler *s) {
    if (!s->cond || s->labels_set) return DLPM_OK;
    set_error("dlpm_sampler: the net is class-conditional: call dlpm_sampler_set_labels first");
    return DLPM_ERR_STATE;
}

int build_tables(dlpm_sampler *s, hipStream_t st) {
    TRY(flush_key(s, st));
    if (!s->lim)
        TRY(dlpm_coeff_tables_f32(s->A, s->g, s->s, s->bs, s->cfg.T, s->cols, s->c_eps, s->c_noise, nullptr, st));
    if (s->hist)   // row 0 of the history is x_T (GenerativeLevyProcess.py:314)
        DLPM_HIP(hipMemcpyAsync(s->hist, s->x, (size_t)s->cfg.B * s->D * sizeof(float), hipMemcpyDeviceToDevice, st));
    k_set_t<<<1, 64, 0, st>>>(s->t_dev, s->cfg.T - 1);
    DLPM_LAUNCH_CHECK();
    s->t_host = s->cfg.T - 1;
    return DLPM_OK;
}

}  // namespace

extern "C" int dlpm_sampler_create(const dlpm_sampler_config *cfg, dlpm_sampler **out) {
    DLPM_CHECK_ARG(cfg && out, "dlpm_sampler_create: null argument");
    DLPM_CHECK_ARG((cfg->unet != nullptr) != (cfg->mlp != nullptr), "dlpm_sampler_create: exactly one of unet / mlp");
    DLPM_CHECK_ARG(cfg->B > 0 && cfg->C > 0 && cfg->H > 0 && cfg->W > 0, "dlpm_sampler_create: bad shape");
    DLPM_CHECK_ARG(cfg->T >= 2, "dlpm_sampler_create: reverse_steps must be >= 2, got %d", cfg->T);
    DLPM_CHECK_ARG(cfg->alpha > 0.0 && cfg->alpha <= 2.0, "Wrong value of alpha (%g) for skewed levy r.v generation", cfg->alpha);
    const bool have = cfg->g && cfg->bg && cfg->s && cfg->bs;
    DLPM_CHECK_ARG(have || (!cfg->g && !cfg->bg && !cfg->s && !cfg->bs), "dlpm_sampler_create: give all four schedule arrays or none");
    DLPM_CHECK_ARG(!(cfg->in_scale && (cfg->flags & DLPM_SMP_LIM)), "dlpm_sampler_create: input scaling belongs to the DLPM loop");
    const bool is_lim = (cfg->flags & DLPM_SMP_LIM) != 0;
    const bool have_lim = cfg->lim_ts && cfg->lim_tmp && cfg->lim_cx && cfg->lim_cs && cfg->lim_cn;
    DLPM_CHECK_ARG(!is_lim || have_lim || (!cfg->lim_ts && !cfg->lim_tmp && !cfg->lim_cx && !cfg->lim_cs && !cfg->lim_cn),
                   "dlpm_sampler_create: give all five LIM tables or none");
    DLPM_CHECK_ARG(cfg->mean_type >= DLPM_MEAN_EPSILON && cfg->mean_type <= DLPM_MEAN_PREVIOUS_X, "dlpm_sampler_create: unknown mean type %d", cfg->mean_type);
    DLPM_CHECK_ARG(!is_lim || cfg->mean_type == DLPM_MEAN_EPSILON, "LIM only supports epsilon prediction, fixed variance and rescaled timesteps");
    DLPM_CHECK_ARG(!is_lim || !(cfg->flags & (DLPM_UPD_CLIP | DLPM_UPD_ELEMENTWISE)),
                   "dlpm_sampler_create: the LIM sampler has no clip_denoised / non-isotropic variant (the reference's are commented out)");
    const bool cond = cfg->unet && dlpm_unet_num_classes(cfg->unet) > 0;
    if (cond && is_lim) {
        set_error("dlpm_sampler_create: the LIM sampler does not take class labels (class-conditional nets sample with the DLPM loop)");
        return DLPM_ERR_UNSUPPORTED;
    }
    dlpm_sampler *s = new dlpm_sampler();
    s->cfg = *cfg;
    s->cond = cond;
    s->D = (int64_t)cfg->C * cfg->H * cfg->W;
    s->lim = is_lim;
    s->elem = (cfg->flags & DLPM_UPD_ELEMENTWISE) != 0;
    s->cols = s->elem ? cfg->B * s->D : cfg->B;
    if (s->elem && cfg->mlp) {
        set_error("dlpm_sampler_create: the toy MLP takes isotropic noise only (the reference asserts the same, Model.py:44)");
        delete s;
        return DLPM_ERR_UNSUPPORTED;
    }
    const int T = cfg->T;
    const int64_t B = cfg->B;
    std::vector<float> hg(T), hbg(T), hs(T), hbs(T);
    std::vector<float> lts(T), ltmp(T), lcx(T), lcs(T), lcn(T);
    if (is_lim) {
        if (have_lim) {
            for (int i = 0; i < T; i++) lts[i] = cfg->lim_ts[i];
            for (int i = 0; i < T - 1; i++) { ltmp[i] = cfg->lim_tmp[i]; lcx[i] = cfg->lim_cx[i]; lcs[i] = cfg->lim_cs[i]; lcn[i] = cfg->lim_cn[i]; }
        } else {
            int r = dlpm_lim_tables_f32(cfg->alpha, T - 1, (cfg->flags & DLPM_UPD_DLIM) != 0, lts.data(), ltmp.data(), lcx.data(),
                                        lcs.data(), lcn.data());
            if (r != DLPM_OK) { delete s; return r; }
        }
        hbs[T - 1] = 1.0f;   // x_0 = gen_eps.generate(shape), unscaled (GenerativeLevyProcess.py:464)
    } else if (have) {
        for (int i = 0; i < T; i++) { hg[i] = cfg->g[i]; hbg[i] = cfg->bg[i]; hs[i] = cfg->s[i]; hbs[i] = cfg->bs[i]; }
    } else {
        int r = dlpm_schedule_f32(T, cfg->alpha, hg.data(), hbg.data(), hs.data(), hbs.data());
        if (r != DLPM_OK) { delete s; return r; }
    }
    s->cfg.g = s->cfg.bg = s->cfg.s = s->cfg.bs = nullptr;  // host pointers are not retained
    s->cfg.lim_ts = s->cfg.lim_tmp = s->cfg.lim_cx = s->cfg.lim_cs = s->cfg.lim_cn = nullptr;
    const float *h_in_scale = cfg->in_scale;
    s->cfg.in_scale = nullptr;
    s->bs_last = hbs[T - 1];
    auto fail = [&](hipError_t e) {
        set_error("dlpm_sampler_create: %s", hipGetErrorString(e));
        dlpm_sampler_destroy(s);
        return DLPM_ERR_HIP;
    };
    hipError_t e;
    float **sched[4] = {&s->g, &s->bg, &s->s, &s->bs};
    std::vector<float> *hsrc[4] = {&hg, &hbg, &hs, &hbs};
    for (int i = 0; i < 4; i++) {
        if ((e = hipMalloc(sched[i], T * sizeof(float))) != hipSuccess) return fail(e);
        if ((e = hipMemcpy(*sched[i], hsrc[i]->data(), T * sizeof(float), hipMemcpyHostToDevice)) != hipSuccess) return fail(e);
    }
    if (is_lim) {
        float **ld[5] = {&s->lim_ts, &s->lim_tmp, &s->lim_cx, &s->lim_cs, &s->lim_cn};
        std::vector<float> *lsrc[5] = {&lts, &ltmp, &lcx, &lcs, &lcn};
        for (int i = 0; i < 5; i++) {
            if ((e = hipMalloc(ld[i], T * sizeof(float))) != hipSuccess) return fail(e);
            if ((e = hipMemcpy(*ld[i], lsrc[i]->data(), T * sizeof(float), hipMemcpyHostToDevice)) != hipSuccess) return fail(e);
        }
    }
    if (h_in_scale) {
        if ((e = hipMalloc(&s->in_scale, T * sizeof(float))) != hipSuccess) return fail(e);
        if ((e = hipMemcpy(s->in_scale, h_in_scale, T * sizeof(float), hipMemcpyHostToDevice)) != hipSuccess) return fail(e);
        if ((e = hipMalloc(&s->xin, (size_t)B * s->D * sizeof(float))) != hipSuccess) return fail(e);
    }
    const size_t tb = (size_t)T * s->cols * sizeof(float);
    if ((e = hipMalloc(&s->A, tb)) != hipSuccess) return fail(e);
    // Non-isotropic tables are T*B*D floats each (12.6 GB for [1024,3,32,32], T = 1000): A is only read again by
    // DLIM with eta > 0, otherwise c_eps is computed in place over it.
    const bool keepA = !s->elem || ((cfg->flags & DLPM_UPD_DLIM) && cfg->dlim_eta != 0.0f) || cfg->mean_type == DLPM_MEAN_Z;
    if (is_lim) {
        s->c_eps = s->A;     // LIM has no coefficient tables: A[i,b] is read directly by the update
        s->c_noise = nullptr;
    } else if (keepA) {
        if ((e = hipMalloc(&s->c_eps, tb)) != hipSuccess) return fail(e);
    } else {
        s->c_eps = s->A;
    }
    if (!is_lim && (e = hipMalloc(&s->c_noise, tb)) != hipSuccess) return fail(e);
    if ((e = hipMalloc(&s->hist_cell, sizeof(float *))) != hipSuccess) return fail(e);
    if ((e = hipMemset(s->hist_cell, 0, sizeof(float *))) != hipSuccess) return fail(e);
    if ((e = hipMalloc(&s->x, (size_t)B * s->D * sizeof(float))) != hipSuccess) return fail(e);
    if ((e = hipMalloc(&s->eps, (size_t)B * s->D * sizeof(float))) != hipSuccess) return fail(e);
    if ((e = hipMalloc(&s->tvec, (size_t)B * sizeof(float))) != hipSuccess) return fail(e);
    if ((e = hipMalloc(&s->t_dev, sizeof(int32_t))) != hipSuccess) return fail(e);
    if (cond && (e = hipMalloc(&s->labels, (size_t)B * sizeof(int64_t))) != hipSuccess) return fail(e);
    if ((e = hipMalloc(&s->key_dev, 2 * DLPM_MAX_CHAINS * sizeof(uint64_t))) != hipSuccess) return fail(e);
    s->nrows[0] = B;
    if (cfg->unet) {
        int r = chain_layout(s, &s->ws_bytes);
        if (r != DLPM_OK) {
            dlpm_sampler_destroy(s);
            return r;
        }
    }
    {
        uint64_t key[4] = {cfg->seed, (uint64_t)cfg->sample_offset, cfg->seed, (uint64_t)(cfg->sample_offset + s->row0[1])};
        if ((e = hipMemcpy(s->key_dev, key, sizeof(key), hipMemcpyHostToDevice)) != hipSuccess) return fail(e);
    }
    if (cfg->unet) {
        if ((e = hipMalloc(&s->ws, (size_t)s->ws_bytes)) != hipSuccess) return fail(e);
        s->plan_version = dlpm_unet_plan_version(cfg->unet);
        int r = build_time_table(s);
        if (r != DLPM_OK) {
            dlpm_sampler_destroy(s);
            return r;
        }
    }
    *out = s;
    return DLPM_OK;
}

extern "C" int dlpm_sampler_reseed(dlpm_sampler *s, uint64_t seed, int64_t sample_offset) {
    DLPM_CHECK_ARG(s, "dlpm_sampler_reseed: null handle");
    if (seed == s->cfg.seed && sample_offset == s->cfg.sample_offset) return DLPM_OK;
    s->cfg.seed = seed;
    s->cfg.sample_offset = sample_offset;
    // The key is read from device memory by the captured update node: no recapture needed.  It is written by a
    // one-thread kernel on the stream of the next begin*() / set_state / steps / step_injected, whichever comes first --
    // stream order puts it behind every replay of the previous trajectory (dlpm_sampler_steps fences its private stream
    // back into the caller's), so nothing synchronises here.
    s->key_dirty = true;
    return DLPM_OK;
}

extern "C" int dlpm_sampler_begin(dlpm_sampler *s, dlpm_stream_t stream) {
    DLPM_CHECK_ARG(s, "dlpm_sampler_begin: null handle");
    TRY(need_labels(s));
    hipStream_t st = as_stream(stream);
    const dlpm_sampler_config &c = s->cfg;
    if (s->lim) {
        // per-step a (unclamped: gen_sas draws its own, Distributions.py:63-64) for steps i = 0..T-2, then x_0
        if (c.alpha != 2.0 && !(c.flags & DLPM_UPD_DLIM))
            TRY(dlpm_skewed_levy_philox_f32(s->A, c.T - 1, c.B, c.alpha, -1.0, c.seed, c.sample_offset, st));
        TRY(dlpm_init_state_philox_f32(s->x, c.B, s->D, c.alpha, c.clamp_eps, 1.0f, c.seed, c.sample_offset, st));
    } else if (s->elem) {
        TRY(dlpm_skewed_levy_elem_philox_f32(s->A, c.T, c.B, s->D, c.alpha, c.clamp_a, c.seed, c.sample_offset, st));
        TRY(dlpm_init_state_elem_philox_f32(s->x, c.B, s->D, c.alpha, c.clamp_eps, s->bs_last, c.seed, c.sample_offset, st));
    } else {
        TRY(dlpm_skewed_levy_philox_f32(s->A, c.T, c.B, c.alpha, c.clamp_a, c.seed, c.sample_offset, st));
        TRY(dlpm_init_state_philox_f32(s->x, c.B, s->D, c.alpha, c.clamp_eps, s->bs_last, c.seed, c.sample_offset, st));
    }
    return build_tables(s, st);
}

extern "C" int dlpm_sampler_begin_injected(dlpm_sampler *s, const float *A_dev, const float *xT_dev, dlpm_stream_t stream) {
    DLPM_CHECK_ARG(s && A_dev && xT_dev, "dlpm_sampler_begin_injected: null argument");
    TRY(need_labels(s));
    hipStream_t st = as_stream(stream);
    DLPM_HIP(hipMemcpyAsync(s->A, A_dev, (size_t)(s->lim ? s->cfg.T - 1 : s->cfg.T) * s->cols * sizeof(float),
                            hipMemcpyDeviceToDevice, st));
    DLPM_HIP(hipMemcpyAsync(s->x, xT_dev, (size_t)s->cfg.B * s->D * sizeof(float), hipMemcpyDeviceToDevice, st));
    return build_tables(s, st);
}

extern "C" int dlpm_sampler_set_state(dlpm_sampler *s, const float *x_dev, int32_t t, dlpm_stream_t stream) {
    DLPM_CHECK_ARG(s, "dlpm_sampler_set_state: null handle");
    DLPM_CHECK_ARG(t >= 1 && t <= s->cfg.T - 1, "dlpm_sampler_set_state: t = %d outside 1..%d", t, s->cfg.T - 1);
    hipStream_t st = as_stream(stream);
    TRY(flush_key(s, st));   // reseed -> set_state -> steps (resuming a trajectory under a new key) must not draw with the old one
    if (x_dev)
        DLPM_HIP(hipMemcpyAsync(s->x, x_dev, (size_t)s->cfg.B * s->D * sizeof(float), hipMemcpyDeviceToDevice, st));
    k_set_t<<<1, 64, 0, st>>>(s->t_dev, t);
    DLPM_LAUNCH_CHECK();
    s->t_host = t;
    return DLPM_OK;
}

extern "C" int dlpm_sampler_step_injected(dlpm_sampler *s, const float *z_dev, dlpm_stream_t stream) {
    DLPM_CHECK_ARG(s, "dlpm_sampler_step_injected: null handle");
    if (s->t_host < 1) return DLPM_OK;
    TRY(need_labels(s));
    TRY(sync_plan(s));
    TRY(flush_key(s, as_stream(stream)));
    TRY(one_step(s, z_dev, true, as_stream(stream)));
    s->t_host -= 1;
    return DLPM_OK;
}

static int steps_on(dlpm_sampler *s, int32_t nsteps, hipStream_t st, bool graph) {
    if (graph && !s->exec) {
        // the first step runs eagerly (sets function attributes, pages code in), then `use_graph`
        // consecutive steps are captured into one graph
        TRY(one_step(s, nullptr, true, st));
        s->t_host -= 1;
        nsteps -= 1;
        const int gs = s->cfg.use_graph;
        if (nsteps >= gs) {
            DLPM_HIP(hipStreamSynchronize(st));
            DLPM_HIP(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
            int r = DLPM_OK;
            for (int i = 0; i < gs && r == DLPM_OK; i++) r = one_step(s, nullptr, true, st);
            hipError_t e = hipStreamEndCapture(st, &s->graph);
            if (r != DLPM_OK) {
                if (s->graph) (void)hipGraphDestroy(s->graph);
                s->graph = nullptr;
                return r;
            }
            DLPM_HIP(e);
            DLPM_HIP(hipGraphInstantiate(&s->exec, s->graph, nullptr, nullptr, 0));
            s->graph_steps = gs;
            s->graph_chains = chains_now(s, nullptr);
            s->captures++;
            // capture only records: nothing ran, so t is unchanged and the replays below do the work
        }
    }
    while (nsteps > 0) {
        if (graph && s->exec && nsteps >= s->graph_steps) {
            DLPM_HIP(hipGraphLaunch(s->exec, st));
            nsteps -= s->graph_steps;
            s->t_host -= s->graph_steps;
        } else {
            TRY(one_step(s, nullptr, true, st));
            nsteps -= 1;
            s->t_host -= 1;
        }
    }
    return DLPM_OK;
}

extern "C" int dlpm_sampler_steps(dlpm_sampler *s, int32_t nsteps, dlpm_stream_t stream) {
    DLPM_CHECK_ARG(s && nsteps >= 0, "dlpm_sampler_steps: bad argument");
    hipStream_t st = as_stream(stream);
    if (nsteps > s->t_host) nsteps = s->t_host;
    if (nsteps == 0) return DLPM_OK;
    TRY(need_labels(s));
    TRY(sync_plan(s));
    TRY(flush_key(s, st));   // one thread, stream-ordered before the (replayed) steps; free when the key is clean
    // toy net, plain stochastic DLPM steps: the whole run of steps is one launch (state in registers)
    // (one wave per sample: best while the batch is latency-bound; beyond ~16k samples the 4-samples-per-wave
    //  forward kernel + update kernel reuse the weights better)
    // (a net on the general forward has no such loop: it takes the per-step path below)
    if (s->cfg.mlp && dlpm_mlp_tile_rows(s->cfg.mlp) == 0 && !(s->cfg.flags & (DLPM_UPD_DLIM | DLPM_UPD_CLIP | DLPM_SMP_NO_FUSED_MLP | DLPM_SMP_LIM)) && s->D <= 4 && s->cfg.mean_type == DLPM_MEAN_EPSILON &&
        s->cfg.B <= 16384 && !s->hist && !s->in_scale && !prof_enabled()) {
        TRY(dlpm_mlp_sample_steps_f32(s->cfg.mlp, s->x, s->c_eps, s->c_noise, s->g, s->cfg.T, s->cfg.B, s->t_host, nsteps,
                                      s->cfg.seed, s->cfg.sample_offset, s->key_dev, st));
        s->t_host -= nsteps;
        k_set_t<<<1, 64, 0, st>>>(s->t_dev, s->t_host);
        DLPM_LAUNCH_CHECK();
        return DLPM_OK;
    }
    const bool graph = s->cfg.use_graph && !prof_enabled();
    if (!graph) return steps_on(s, nsteps, st, false);
    if (s->exec && s->graph_chains != chains_now(s, nullptr)) {   // a history buffer came or went since the capture
        DLPM_HIP(hipDeviceSynchronize());
        drop_graph(s);
    }
    if (!s->own) {
        DLPM_HIP(hipStreamCreateWithFlags(&s->own, hipStreamNonBlocking));
        DLPM_HIP(hipEventCreateWithFlags(&s->ev_in, hipEventDisableTiming));
        DLPM_HIP(hipEventCreateWithFlags(&s->ev_out, hipEventDisableTiming));
    }
    DLPM_HIP(hipEventRecord(s->ev_in, st));            // everything the caller queued so far ...
    DLPM_HIP(hipStreamWaitEvent(s->own, s->ev_in, 0)); // ... precedes the replayed steps
    int r = steps_on(s, nsteps, s->own, true);
    DLPM_HIP(hipEventRecord(s->ev_out, s->own));
    DLPM_HIP(hipStreamWaitEvent(st, s->ev_out, 0));    // and the caller's later work follows them
    return r;
}

extern "C" int dlpm_sampler_set_labels(dlpm_sampler *s, const int64_t *y_dev, dlpm_stream_t stream) {
    DLPM_CHECK_ARG(s && y_dev, "dlpm_sampler_set_labels: null argument");
    DLPM_CHECK_ARG(s->cond, "dlpm_sampler_set_labels: the sampler's net is not class-conditional");
    // into the buffer the captured graph reads: new labels never force a recapture.  Stream-ordered behind every earlier replay
    // (dlpm_sampler_steps fences its private stream back into the caller's) and ahead of the next one
    DLPM_HIP(hipMemcpyAsync(s->labels, y_dev, (size_t)s->cfg.B * sizeof(int64_t), hipMemcpyDeviceToDevice, as_stream(stream)));
    s->labels_set = true;
    return DLPM_OK;
}

extern "C" int dlpm_sampler_set_history(dlpm_sampler *s, float *hist_dev, dlpm_stream_t stream) {
    DLPM_CHECK_ARG(s, "dlpm_sampler_set_history: null handle");
    if (hist_dev == s->hist) return DLPM_OK;
    // the captured update node reads the base from a device cell, so the graph follows the new buffer; the cell is
    // written in stream order (earlier replays were fenced back into the caller's stream), no host synchronisation
    k_set_ptr<<<1, 64, 0, as_stream(stream)>>>(s->hist_cell, hist_dev);
    DLPM_LAUNCH_CHECK();
    s->hist = hist_dev;
    return DLPM_OK;
}

extern "C" int dlpm_sampler_copy_state(dlpm_sampler *s, float *out_dev, dlpm_stream_t stream) {
    DLPM_CHECK_ARG(s && out_dev, "dlpm_sampler_copy_state: null argument");
    DLPM_HIP(hipMemcpyAsync(out_dev, s->x, (size_t)s->cfg.B * s->D * sizeof(float), hipMemcpyDeviceToDevice, as_stream(stream)));
    return DLPM_OK;
}

extern "C" float *dlpm_sampler_state(dlpm_sampler *s) { return s ? s->x : nullptr; }
extern "C" int32_t dlpm_sampler_t(const dlpm_sampler *s) { return s ? s->t_host : -1; }
extern "C" int32_t dlpm_sampler_chains(const dlpm_sampler *s) { return s ? chains_now(s, nullptr) : -1; }
extern "C" int64_t dlpm_sampler_graph_captures(const dlpm_sampler *s) { return s ? s->captures : -1; }
extern "C" float *dlpm_sampler_table(dlpm_sampler *s, int which) {
    if (!s) return nullptr;
    switch (which) {
        case 0: return s->A;
        case 1: return s->c_eps;
        case 2: return s->c_noise;
        case 3: return s->eps;
        default: return nullptr;
    }
}

extern "C" void dlpm_sampler_destroy(dlpm_sampler *s) {
    if (!s) return;
    if (s->exec) (void)hipGraphExecDestroy(s->exec);
    if (s->graph) (void)hipGraphDestroy(s->graph);
    if (s->ev_in) (void)hipEventDestroy(s->ev_in);
    if (s->ev_out) (void)hipEventDestroy(s->ev_out);
    if (s->ev_fork) (void)hipEventDestroy(s->ev_fork);
    if (s->ev_join) (void)hipEventDestroy(s->ev_join);
    if (s->own) (void)hipStreamDestroy(s->own);
    if (s->side) (void)hipStreamDestroy(s->side);
    void *bufs[] = {s->g, s->bg, s->s, s->bs, s->A, s->c_eps == s->A ? nullptr : s->c_eps, s->c_noise, s->x, s->eps, s->tvec, s->emb_tab,
                    s->t_dev, s->key_dev, s->ws, s->hist_cell, s->lim_ts, s->lim_tmp, s->lim_cx, s->lim_cs, s->lim_cn,
                    s->in_scale, s->xin, s->labels};
    for (void *p : bufs)
        if (p) (void)hipFree(p);
    delete s;
}
