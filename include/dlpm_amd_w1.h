/* dlpm_amd_w1.h -- the exact Wasserstein-1 entry points of libdlpm_amd (same library, same ABI version as dlpm_amd.h, which this
 * header includes; the two functions live here so that the table of dlpm_amd.h stays as it is).
 *
 * W1 between two sets of n points x [n, D] and y [n, D], fp32 on the device, every point of mass 1 / n:
 *   W = (1 / n) min over permutations s of sum_i c(i, s(i)),
 *   c = mean_d |x_d - y_d|  (DLPM_W1_L1_MEAN: the cost of the manual_compute branch of bem/evaluate/wasserstein.py:23-46)  or
 *   c = |x - y|_2           (DLPM_W1_EUCLIDEAN).
 * The costs are computed in fp64, scaled by 2^e so that the largest lies in [2^23, 2^24], rounded to integers q, and the assignment
 * problem on q is solved EXACTLY by a forward auction with eps-scaling in integer arithmetic (integer atomics only): the same inputs
 * give the same permutation, prices, round and phase counts, bit for bit.  W is the fp64 cost of that permutation, so
 * 0 <= W - W_opt <= 2^-e.  The host enqueues batches of rounds and reads a small header once per batch: dlpm_w1_f32 WAITS ON THE
 * STREAM and cannot be captured in a hipGraph. */
#ifndef DLPM_AMD_W1_H
#define DLPM_AMD_W1_H
#include "dlpm_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DLPM_W1_L1_MEAN 0
#define DLPM_W1_EUCLIDEAN 1

/* Bytes of workspace for dlpm_w1_f32(n, D): the n x n int32 cost matrix plus O(n).  DLPM_ERR_ARG (-1) for n outside 1..32768 or D
 * outside 1..4096. */
int64_t dlpm_w1_workspace_bytes(int64_t n, int64_t D);

/* out_dev: double [8] = W, the integer optimum sum_i q(i, perm[i]), the scale exponent e, rounds, phases, cmax (the largest cost),
 * status, rounds run by the one-workgroup kernel.  status 1 = a non-finite input value, status 2 = max_rounds reached before the end;
 * W is NaN under both.  perm_out_dev: int32 [n] or null, perm[i] = the row of y matched with row i of x; prices_out_dev: int64 [n] or
 * null, the final prices.  A round with at most tail_threshold bidders runs in the one-workgroup kernel (0 = never, >= n = always);
 * the choice changes no bit of the results.  DLPM_ERR_ARG for a null or misaligned pointer (x, y, out; perm and prices when given), n
 * outside 1..32768, D outside 1..4096, an unknown ground, max_rounds < 1 or tail_threshold < 0; DLPM_ERR_NOMEM for a short workspace
 * (which must be 16-byte aligned) -- before any launch. */
int dlpm_w1_f32(const float *x_dev, const float *y_dev, int64_t n, int64_t D, int32_t ground, int64_t max_rounds, int64_t tail_threshold,
                void *workspace_dev, int64_t workspace_bytes, int32_t *perm_out_dev, int64_t *prices_out_dev, double *out_dev,
                dlpm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DLPM_AMD_W1_H */
