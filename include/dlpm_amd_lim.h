/* dlpm_amd_lim.h -- the LIM held-out loss entry points of libdlpm_amd (same library, same ABI version as dlpm_amd.h, which this
 * header includes; the two functions live here so that the table of dlpm_amd.h stays as it is).
 *
 * The forward half of LIM's objective as an evaluation metric (no backward pass).  Reference:
 * GenerativeLevyProcess.training_losses_lim (dlpm/methods/GenerativeLevyProcess.py:680-709) and loss_fn
 * (dlpm/methods/LIM/functions/loss.py:12-41) on VPSDE(alpha, 'cosine') (LIM/functions/sde.py):
 *   e   symmetric alpha-stable, sqrt(a) z with ONE unclamped a per sample (gen_sas), or z itself at alpha = 2 (randn_like)
 *   t   uniform on [1e-5, T), continuous
 *   x_t = x0 diffusion_coeff(t) + e marginal_std(t),   score = -e / alpha  (-e at alpha = 2)
 * followed by one forward of the score net on (x_t, t) and the mean smooth-L1 of its output against `score`.  That last step is
 * dlpm_loss_terms_f32(output, score, lploss = 1, replicas = 1) and dlpm_loss_reduce_f32(outer = inner = 1, mean) of dlpm_amd.h.
 *
 * The two coefficients are differences of nearly equal numbers: with lm(t) = log cos((t + s)/(1 + s) pi/2) - log cos(s/(1 + s) pi/2),
 * s = 0.008, diffusion_coeff = exp(lm) and marginal_std = (1 - exp(alpha lm))^(1/alpha), and near t = 1e-5 the two logarithms are
 * values 6e-8 apart from 0 -- the reference's fp32 evaluation is off by up to 12 % there and depends on the libm behind it.  So the
 * coefficients are either INPUTS (what the caller's own evaluation gave) or evaluated here in fp64 and rounded once. */
#ifndef DLPM_AMD_LIM_H
#define DLPM_AMD_LIM_H
#include "dlpm_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dlpm_lim_loss_args {
    const float *x0_dev;       /* [B,D] x_start                                                                              */
    const float *t_dev;        /* [B] injected times, or NULL = Philox: U 24-bit in [0,1), t = U (float)(t_max - 1e-5) + 1e-5f  */
    const float *e_dev;        /* [B,D] injected noise (used as given: no clamp), or NULL = Philox                           */
    const float *x_coeff_dev;  /* [B] injected diffusion_coeff(t), or NULL = fp64 in the kernel from the fp32 t              */
    const float *sigma_dev;    /* [B] injected marginal_std(t); given if and only if x_coeff_dev is                          */
    float *x_t_dev;            /* [B,D] out: what the net reads                                                              */
    float *score_dev;          /* [B,D] out: the regression target                                                           */
    float *tvec_out_dev;       /* [B] out: the times the net is fed                                                          */
    float *a_out_dev;          /* [B] out, nullable: the a drawn (1 where none is: alpha = 2 or injected e)                  */
    float *e_out_dev;          /* [B,D] out, nullable: the noise used                                                        */
    float *x_coeff_out_dev;    /* [B] out, nullable: the coefficients used                                                   */
    float *sigma_out_dev;      /* [B] out, nullable                                                                          */
    int64_t B, D;
    double alpha;
    double clamp_eps;          /* < 0: none; applied to Philox draws as gen_sas does                                         */
    double t_max;              /* VPSDE.T (0.9946), in (1e-5, 1)                                                             */
    uint64_t seed;             /* Philox key                                                                                 */
    int64_t sample_offset;     /* global index of sample 0 of this call                                                      */
} dlpm_lim_loss_args;

/* One workgroup per sample; x_t = x0 cx + e sigma as two fp32 products and one fp32 sum in that order (no contraction), score =
 * -(e / (float)alpha).  Philox draws are keyed by (seed, global sample index, element) only: a sample's loss does not depend on
 * how a dataset is cut into calls.  No atomic, no host read; capturable in a hipGraph.  HBM-bound: 12 B/element with Philox draws.
 * DLPM_ERR_ARG before any launch for a null x0 / x_t / score / tvec_out, B or D <= 0, alpha outside (0, 2], t_max outside
 * (1e-5, 1), or one of x_coeff_dev / sigma_dev without the other. */
int dlpm_lim_loss_elements_f32(const dlpm_lim_loss_args *args, dlpm_stream_t stream);

/* x_coeff_dev[b] = exp(lm(t_b)), sigma_dev[b] = (-expm1(alpha lm(t_b)))^(1/alpha) in fp64 from the fp32 t_dev[B], rounded once:
 * the evaluation the elements kernel runs when no coefficients are injected, on its own. */
int dlpm_lim_coeffs_f32(const float *t_dev, int64_t B, double alpha, float *x_coeff_dev, float *sigma_dev, dlpm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DLPM_AMD_LIM_H */
