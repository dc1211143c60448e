/* dlpm_amd_step.h -- the step-level entry points of libdlpm_amd (same library, same ABI version as dlpm_amd.h, which this header
 * includes; the two functions live here so that the table of dlpm_amd.h stays as it is).
 *
 * What the reference exposes BETWEEN its whole-trajectory entry points (dlpm/methods/dlpm.py:250-370):
 *   dlpm_anterior_f32          the moments of one reverse step as outputs (anterior_mean_variance_dlpm / _dlim, :272-297) -- the
 *                              same formulas dlpm_update_f32 applies in place, returned instead of applied
 *   dlpm_two_rv_elements_f32   the Proposition-8 loss elements at a per-sample timestep (get_two_rv_loss_elements, :308-370)
 * Both are elementwise and HBM-bound: one workgroup per sample, 16-byte accesses when D % 4 == 0 and every pointer is 16-byte
 * aligned, a scalar path otherwise; the per-sample scalars are formed once per row; no atomic, no host read, capturable in a
 * hipGraph.  Every product and sum the reference rounds separately is rounded separately here (no contraction). */
#ifndef DLPM_AMD_STEP_H
#define DLPM_AMD_STEP_H
#include "dlpm_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum dlpm_anterior_mode { DLPM_ANT_DLPM = 0, DLPM_ANT_DLIM = 1 } dlpm_anterior_mode;

typedef struct dlpm_anterior_args {
    const float *x_dev;        /* [B,D] x_t                                                                                  */
    const float *eps_dev;      /* [B,D] the eps the step formulas take                                                       */
    const int32_t *t_dev;      /* device scalar: the timestep, clamped into [1, T-1] by the kernel                           */
    const float *g_dev;        /* [T] gammas                                                                                 */
    const float *bs_dev;       /* [T] barsigmas                                                                              */
    const float *Sigmas_dev;   /* [T,n] (DLPM mode): the process's own table or any the caller holds                         */
    const float *A_dev;        /* [T,n] (DLIM mode with eta != 0)                                                            */
    float *mean_dev;           /* [B,D] out                                                                                  */
    float *var_dev;            /* [n] out, nullable                                                                          */
    int64_t B, D;              /* n = B, or B * D with DLPM_UPD_ELEMENTWISE                                                  */
    int32_t T;
    int32_t mode;              /* dlpm_anterior_mode                                                                         */
    int32_t flags;             /* 0 or DLPM_UPD_ELEMENTWISE (non-isotropic noise: one table entry per element)               */
    float alpha, eta;
} dlpm_anterior_args;

/* DLPM:         Gamma = 1 - (g_t^2 Sigma_{t-1}) / Sigma_t;  mean = (x - (bs_t Gamma) eps) / g_t;  var = Gamma Sigma_{t-1}
 * DLIM eta = 0: mean = (x - bs_t eps) / g_t + bs_{t-1} eps;  var = 0
 * DLIM eta > 0: s' = eta bs_{t-1};  mean = (x - bs_t eps) / g_t + (bs_{t-1}^alpha - s'^alpha)^(1/alpha) eps;  var = 1[t != 1] s'^2 A_t
 * DLPM_ERR_ARG before any launch for a null pointer the mode reads, B or D <= 0, B >= 2^31, T < 2, an unknown mode or flag. */
int dlpm_anterior_f32(const dlpm_anterior_args *args, dlpm_stream_t stream);

typedef struct dlpm_two_rv_args {
    const float *x0_dev;       /* [B,D]                                                                                      */
    const int32_t *t_dev;      /* [B] per-sample timesteps, clamped into [1, T-1] by the kernel                              */
    const float *g_dev, *bg_dev, *s_dev, *bs_dev;   /* [T] the schedule                                                      */
    const float *a0_dev;       /* [n] injected a_{t,0} (zeroed where t == 1 by the kernel), or NULL = Philox                 */
    const float *a1_dev;       /* [n] injected a_{t,1}; given if and only if a0_dev is                                       */
    const float *z_dev;        /* [B,D] injected normals, or NULL = Philox                                                   */
    float *x_t_dev, *eps_t_dev, *m_tilde_dev;                                       /* [B,D] out, each nullable              */
    float *Sigma_tilde_dev, *lambda_dev, *Sigma_prime_t_1_dev, *Sigma_prime_t_dev, *Gamma_prime_dev;   /* [n] out, nullable  */
    float *a0_out_dev, *a1_out_dev;                                                 /* [n] out, nullable: the a used         */
    int64_t B, D;              /* n = B, or B * D with DLPM_LOSS_ELEMENTWISE                                                 */
    int32_t T;
    int32_t flags;             /* 0 or DLPM_LOSS_ELEMENTWISE                                                                 */
    double alpha;
    double clamp_a;            /* < 0: none; applied to Philox draws as gen_a does                                           */
    uint64_t seed;             /* Philox key                                                                                 */
    int64_t sample_offset;     /* global index of sample 0 of this call                                                      */
} dlpm_two_rv_args;

/* a0 <- 0 where t == 1;  S'_{t-1} = bs_{t-1}^2 a0;  S'_t = s_t^2 a1 + g_t^2 S'_{t-1};  G' = 1 - (g_t^2 S'_{t-1}) / S'_t;
 * x_t = bg_t x0 + sqrt(S'_t) z;  eps_t = (x_t - x0 bg_t) / bs_t;  m~ = (x_t - (bs_t G') eps_t) / g_t;  S~ = G' S'_{t-1};
 * lambda = bs_t / ((2 g_t) S'_{t-1})  (+inf at t == 1, as in the reference).
 * Philox draws are keyed as dlpm_loss_elements_f32 keys its own -- counter (global sample, element, purpose | which << 8) -- so a
 * sample's elements do not depend on how a batch is cut into calls.  DLPM_ERR_ARG before any launch for a null x0 / t / schedule
 * pointer, B or D <= 0, B >= 2^31, D >= 2^32, T < 2, alpha outside (0, 2], or one of a0_dev / a1_dev without the other. */
int dlpm_two_rv_elements_f32(const dlpm_two_rv_args *args, dlpm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DLPM_AMD_STEP_H */
