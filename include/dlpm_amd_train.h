/* dlpm_amd_train.h -- training of the 2-D toy net (MLPModel) in libdlpm_amd: same library, same ABI version as dlpm_amd.h, which
 * this header includes; the functions live here so that the table of dlpm_amd.h stays as it is.
 *
 * One optimisation step of dlpm/bem/TrainingManager.py (_train_epochs) for the toy net is, after the forward half the library
 * already has (dlpm_loss_elements_f32 / dlpm_lim_loss_elements_f32, dlpm_mlp_forward, dlpm_loss_terms_f32, dlpm_loss_reduce_f32):
 *   dlpm_loss_grad_f32         d loss / d model_eps
 *   dlpm_mlp_backward_f32      d loss / d (every parameter), optionally d loss / d x
 *   dlpm_grad_clip_coef_f32    clip_grad_norm_ as a device scalar
 *   dlpm_adamw_step_f32        torch.optim.AdamW and up to 8 EMA shadows in one pass
 *   dlpm_mlp_import_params_f32 the new parameters into the net's packed blob
 * No entry point synchronises, reads a device value on the host or uses a floating-point atomic: every sum is taken in a fixed
 * order, so the same inputs give the same bits whatever the grid.  UNet training is out of scope. */
#ifndef DLPM_AMD_TRAIN_H
#define DLPM_AMD_TRAIN_H
#include "dlpm_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The flat parameter vector is torch.nn.utils.parameters_to_vector(model.parameters()) of MLPModel: named_parameters() order
 * (group_norm_in, time_emb, time_mlp.2, linear_in, then per block group_norm1, group_norm2, mlp_1.1, t_proj.1, mlp_2.1 for
 * midblocks.0 .. and outblocks_mean.0, then outblocks_mean.1), weight before bias, every tensor in torch's layout ([out][in]),
 * every alias of the state_dict once.  The map between it and the packed, transposed blob the kernels read is the library's.
 * dlpm_mlp_param_floats: its length P (55 010 for the shipped net); < 0 for a null handle. */
int64_t dlpm_mlp_param_floats(const dlpm_mlp *m);

/* flat_dev[P] <- the net's parameters.  DLPM_ERR_ARG for a null pointer or n != P, DLPM_ERR_STATE before dlpm_mlp_finalize. */
int dlpm_mlp_export_params_f32(dlpm_mlp *m, float *flat_dev, int64_t n, dlpm_stream_t stream);

/* The net's parameters <- flat_dev[P], on the stream: the blob, the float4 copies the fused sampling loop reads, and the copy
 * the backward reads; the per-timestep table of dlpm_mlp_sample_steps_f32 is invalidated (rebuilt by its next call).  The
 * host copy that dlpm_mlp_set_param fills is not updated: a later dlpm_mlp_finalize uploads what set_param was given.
 * A sampler created on this handle that has captured a graph must be dropped by the caller.  Refusals as for export. */
int dlpm_mlp_import_params_f32(dlpm_mlp *m, const float *flat_dev, int64_t n, dlpm_stream_t stream);

/* Bytes of workspace dlpm_mlp_backward_f32 needs for `rows` rows; < 0 for a null handle or rows <= 0. */
int64_t dlpm_mlp_backward_workspace_bytes(const dlpm_mlp *m, int64_t rows);

/* Given dout = dL/d(output) [rows,F] at the inputs x [rows,F], t [rows]: grad_flat[P] = dL/d(parameter) in the flat order above
 * and, when dx_dev is given, dx [rows,F] = dL/dx.  The whole architecture of dlpm_mlp_forward: the time embedding
 * Linear(1,TE) -> SiLU -> Linear(TE,TE) -> SiLU, Linear(F,64) -> LayerNorm -> SiLU, nblocks + 1 conditioned blocks (t_proj, two
 * LayerNorms, the skip), Linear(64,F); any F >= 1, 1 <= TE <= 64, nblocks >= 0, rows >= 1.
 * Two kernels and a sum.  The first recomputes the forward with the very operations of dlpm_mlp_forward (one wavefront per 4
 * rows; rows past the end carry dout = 0 and write nothing) and walks it back, leaving per row every layer's input and
 * dL/d(pre-activation) in the workspace.  The second forms every dW = dY^T A, bias and LayerNorm gradient over chunks of 64
 * rows, rows in order within a chunk (the matrices in fp32, the single columns -- biases, LayerNorm weights -- in fp64); the
 * third adds the chunk partials in chunk order in fp64 and rounds once.
 * DLPM_ERR_ARG for a null pointer or rows <= 0, DLPM_ERR_NOMEM for a short workspace, DLPM_ERR_STATE before
 * dlpm_mlp_finalize -- all before any launch. */
int dlpm_mlp_backward_f32(dlpm_mlp *m, const float *x_dev, const float *t_dev, const float *dout_dev, int64_t rows,
                          float *grad_flat_dev, float *dx_dev, void *workspace_dev, int64_t workspace_bytes, dlpm_stream_t stream);

/* The derivative of dlpm_loss_terms_f32 followed by dlpm_loss_reduce_f32 with respect to model_eps [outer*inner*B, D].
 * With d = model_eps - target and term = terms_dev[row] (what dlpm_loss_terms_f32 wrote, out_stride = B, out_offset = 0):
 *   lploss  2: d / (D term), and 0 where term == 0 (torch's autograd gives NaN there)
 *   lploss  1: clamp(d, -1, 1) / D
 *   lploss -1: 2 d / D
 * times the weight of the row (o, i, b) = (o*inner + i)*B + b: 1 / (outer inner B) under the mean estimator
 * (median_index_dev == NULL); under the median of means 1 / (inner B) where o == median_index_dev[b] -- the index
 * dlpm_loss_reduce_f32 returns -- and 0 elsewhere.  Evaluated in fp64 and rounded once.  The LIM objective is lploss = 1
 * against `score`, outer = inner = 1.
 * DLPM_ERR_ARG before any launch for a null pointer, B, outer, inner or D <= 0, lploss not in {2, 1, -1}, outer > 64 with a
 * median index. */
int dlpm_loss_grad_f32(const float *model_eps_dev, const float *target_dev, const float *terms_dev, const int32_t *median_index_dev,
                       float *dmodel_dev, int64_t B, int32_t outer, int32_t inner, int64_t D, int32_t lploss, dlpm_stream_t stream);

/* torch.nn.utils.clip_grad_norm_ without the host: norm_out_dev[0] = sqrt(sum g^2), the sum in fp64 in a fixed order (one
 * workgroup), coef_out_dev[0] = min(1, max_norm / (norm + 1e-6)); both fp32, both left on the device.  The gradient is not
 * scaled here: dlpm_adamw_step_f32 takes the coefficient.  DLPM_ERR_ARG for a null pointer, n <= 0 or max_norm not > 0. */
int dlpm_grad_clip_coef_f32(const float *grad_dev, int64_t n, double max_norm, float *norm_out_dev, float *coef_out_dev,
                            dlpm_stream_t stream);

#define DLPM_ADAMW_MAX_EMA 8

typedef struct dlpm_adamw_args {
    float *theta_dev;            /* [n] parameters, updated in place                                                     */
    const float *grad_dev;       /* [n]                                                                                  */
    float *exp_avg_dev;          /* [n] first moment, updated in place                                                   */
    float *exp_avg_sq_dev;       /* [n] second moment, updated in place                                                  */
    int64_t n;
    double lr;                   /* per call: a schedule is host arithmetic                                              */
    double beta1, beta2;         /* each in [0, 1)                                                                       */
    double eps, weight_decay;
    int64_t step;                /* 1-based: the step this call takes                                                    */
    const float *coef_dev;       /* nullable device scalar: g <- g * coef_dev[0] first (dlpm_grad_clip_coef_f32)         */
    int32_t n_ema;               /* 0 .. DLPM_ADAMW_MAX_EMA                                                              */
    int32_t reserved;            /* 0                                                                                    */
    float *ema_dev[DLPM_ADAMW_MAX_EMA];    /* [n] each: shadow <- (1 - mu) theta_new + mu shadow (bem/utils_ema.py:22-28) */
    double ema_mu[DLPM_ADAMW_MAX_EMA];
} dlpm_adamw_args;

/* torch.optim.AdamW (decoupled decay first), one elementwise pass:
 *   theta <- theta (1 - lr wd);  m <- b1 m + (1 - b1) g;  v <- b2 v + (1 - b2) g^2;
 *   theta <- theta - (lr / (1 - b1^step)) m / (sqrt(v) / sqrt(1 - b2^step) + eps)
 * and the EMA shadows from the new theta.  Each element is evaluated in fp64 from the fp32 state and every stored value is
 * rounded once, so the stored moments are within half an ulp of the exact update of the stored state.
 * DLPM_ERR_ARG before any launch for a null pointer (a shadow included), n <= 0, n_ema outside [0, 8], a beta outside [0, 1),
 * step < 1, lr, eps or weight_decay negative or not finite. */
int dlpm_adamw_step_f32(const dlpm_adamw_args *args, dlpm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DLPM_AMD_TRAIN_H */
