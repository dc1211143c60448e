/* dlpm_amd_toy.h -- the 2-D toy data distributions of libdlpm_amd (same library, same ABI version as dlpm_amd.h, which this header
 * includes; the three functions live here so that the table of dlpm_amd.h stays as it is).
 *
 * The real samples of a 2-D config, drawn on the device.  Reference: bem/datasets/Distributions.py (sample_2_gmm, sample_grid_gmm,
 * gen_swiss_roll, sample_grid_sas), which draws them on the host with sklearn, scipy and the numpy / torch generators.  Two stages:
 *
 *   A  the raw draw, one thread per row.  Row i of a call is global sample first_index + i; every random number is a function of
 *      (seed, stream, global index, element, purpose) through Philox4x32-10: 53-bit uniforms, normals by Box-Muller in fp64.
 *        gmm_2       component k of 2 at (+theta, 0), (-theta, 0);  x = mean_k + std z
 *        gmm_grid    component k = i n + j of n x n at (i, j), NOT centred;  x = mean_k + std z
 *        swiss_roll  t = 1.5 pi (1 + 2 u);  x = (t cos t + std z0, t sin t + std z1)     (t, cos, sin in fp64)
 *        sas_grid    x = std sqrt(a) z + (i, j) - (n / 2, n / 2), a the totally skewed data_alpha / 2 stable draw (one per row when
 *                    isotropic, one per element otherwise; a = 2 at data_alpha = 2)
 *      The gmm kinds take the first k with u < cum[k] (the last k when there is none): an iid categorical choice, so their rows and
 *      swiss_roll's do not depend on N.  sas_grid assigns components in EXACT proportions as the reference does: position p of the
 *      output holds source row pi(p), pi a keyed bijection of [0, N) (4-round balanced Feistel network on the smallest even bit
 *      width covering N, Philox as round function, cycle-walked into range), and source row r belongs to component k when
 *      bounds[k] <= r < bounds[k + 1]; a row at or past bounds[count] gets no grid offset.  Its rows depend on N: it is drawn whole.
 *   B  the finish, in place on a raw [N, 2] array (drawn or the caller's own):
 *        normalize   (x - m) / s with SCALAR m, s over all 2 N values, fp64 sums in a fixed order, divisor 2 N (numpy std) or
 *                    2 N - 1 (torch std)
 *        between     per column the order statistics of rank round_half_even(q (N - 1)) and round_half_even((1 - q) (N - 1)) by
 *                    an exact radix select (torch.quantile, interpolation='nearest'), c = max(|hi|, |lo|), clamp to +-c, divide by c
 *      The reference's asserts hi >= 0 and lo <= 0 become bits of a status word. */
#ifndef DLPM_AMD_TOY_H
#define DLPM_AMD_TOY_H
#include "dlpm_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum dlpm_toy_kind { DLPM_TOY_GMM_2 = 0, DLPM_TOY_GMM_GRID = 1, DLPM_TOY_SWISS_ROLL = 2, DLPM_TOY_SAS_GRID = 3 } dlpm_toy_kind;

/* bits of the status word dlpm_toy_finish_f32 writes */
#define DLPM_TOY_STATUS_HIGH_NEGATIVE 1 /* a column's high quantile is < 0 (Distributions.py:97) */
#define DLPM_TOY_STATUS_LOW_POSITIVE 2  /* a column's low quantile is > 0 (:98)                  */

typedef struct dlpm_toy_draw_args {
    float *out_dev;               /* [N,2] out                                                                                 */
    int64_t *perm_out_dev;        /* [N] out, nullable: pi(p) of sas_grid (debug)                                              */
    const double *weights_host;   /* [count] HOST: the mixture weights, read by the checks only (gmm kinds, sas_grid)          */
    const double *cum_dev;        /* [count] np.cumsum(weights) in fp64 (gmm kinds)                                            */
    const int64_t *bounds_dev;    /* [count + 1] int(np.cumsum([0, weights]) N) (sas_grid)                                     */
    int64_t N;                    /* rows of this call                                                                         */
    int64_t first_index;          /* global index of row 0; must be 0 for sas_grid                                             */
    int32_t kind;                 /* dlpm_toy_kind                                                                             */
    int32_t n_mixture;            /* components of a grid kind: a perfect square, at most 4096                                 */
    int32_t count;                /* number of weights: 2 (gmm_2) or n_mixture (grid kinds)                                    */
    int32_t isotropic;            /* sas_grid: one a per row (1) or per element (0)                                            */
    double std, theta, data_alpha;
    uint64_t seed;                /* Philox key                                                                                */
    uint32_t stream;              /* independent streams of one seed (train / test), below 2^24                                */
    uint32_t reserved;
} dlpm_toy_draw_args;

/* Stage A.  DLPM_ERR_ARG before any launch for: N <= 0, an unknown kind, n_mixture that is no perfect square or above 4096 (grid
 * kinds), count != components, a negative or non-finite weight, weights summing above 1 + 1e-12, data_alpha outside (0, 2]
 * (sas_grid), std < 0 or not finite, first_index < 0, first_index != 0 for sas_grid, stream >= 2^24, a null pointer that the kind
 * reads.  weights_host is read by these checks, on the host, before the launch; the kernel reads device memory only, uses no atomic
 * and runs on the caller's stream. */
int dlpm_toy_draw_f32(const dlpm_toy_draw_args *args, dlpm_stream_t stream);

/* bytes of workspace dlpm_toy_finish_f32 needs for N rows (DLPM_ERR_ARG, negative, for N <= 0) */
int64_t dlpm_toy_workspace_bytes(int64_t N);

/* Stage B in place on x_dev[N,2].  std_divisor: 0 = 2 N (numpy std), 1 = 2 N - 1 (torch std); read when normalize != 0.  between != 0
 * applies the quantile clamp with quantile_cutoff = q in (0.5, 1].  out_dev[8] (fp64): m, s, then per column hi, lo, c (2 .. 7);
 * status_dev[1] (int32): 0 or DLPM_TOY_STATUS_* bits -- the data is then left normalised but not clamped.  One workgroup per
 * column for the select, one for the moments; sums and selects do not depend on the launch.  DLPM_ERR_ARG before any launch for
 * N <= 0, q outside (0.5, 1] when between, a null or misaligned pointer; DLPM_ERR_NOMEM for a short workspace. */
int dlpm_toy_finish_f32(float *x_dev, int64_t N, int32_t normalize, int32_t std_divisor, int32_t between, double quantile_cutoff,
                        void *workspace_dev, int64_t workspace_bytes, double *out_dev, int32_t *status_dev, dlpm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DLPM_AMD_TOY_H */
