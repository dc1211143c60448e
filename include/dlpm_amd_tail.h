/* dlpm_amd_tail.h -- the tail figures of libdlpm_amd (same library, same ABI version as dlpm_amd.h, which this header includes; the
 * two functions live here so that the table of dlpm_amd.h stays as it is).
 *
 * Two fp32 sets x [n1, D] and y [n2, D] on the device.  Each becomes a vector v of N non-negative fp32 values (the marginal):
 *   DLPM_TAIL_NORM: N = n,     v_i = (float)sqrt(sum_d (double)x_id^2), d ascending, every product and every sum rounded on its own;
 *   DLPM_TAIL_ABS:  N = n * D, v = |x| of every scalar.
 * With s the sorted values, the levels u_j = xi + ((1 - xi) * j) / levels (j = 0 .. levels - 1, fp64) and numpy's 'linear' quantile
 *   q(u) = s[lo] + (h - lo) (s[min(lo + 1, N - 1)] - s[lo]),  h = u (N - 1),  lo = floor(h)                      (fp64),
 * the figures are
 *   msle  = (1 / levels) sum_j (log q_x(u_j) - log q_y(u_j))^2, the terms added one after the other, j ascending;
 *   Hill  = k / sum_{i > r0} (log s[i] - log s[r0]),  r0 = min(floor(xi (N - 1)), N - 2),  k = N - 1 - r0, per set: the k terms are cut
 *           into 1024 runs of ceil(k / 1024) consecutive ranks, each run added in rank order from 0, the runs then added in order.
 * An all-tie tail gives Hill = +inf.  The order statistics come from an exact radix select and an exact sort of the keys above
 * s[r0]: they are the sorted array's own values, bit for bit.  DESIGN 3.23. */
#ifndef DLPM_AMD_TAIL_H
#define DLPM_AMD_TAIL_H
#include "dlpm_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DLPM_TAIL_NORM 0
#define DLPM_TAIL_ABS 1
#define DLPM_TAIL_MAX_LEVELS 65536

/* Bytes of workspace for dlpm_tail_f32 with the same arguments: the keys of both marginals, twice the at most (1 - xi) N + 1 keys
 * above each threshold, the counters of their sort (2 KB per 2048 keys of the longer tail) and O(levels).  DLPM_ERR_ARG (-1) for n1 < 2, n2 < 2, D < 1, more than 2^31 - 1 values in a set, an unknown
 * marginal, xi outside [0.5, 1) or levels outside [1, 65536]. */
int64_t dlpm_tail_workspace_bytes(int64_t n1, int64_t n2, int64_t D, int32_t marginal, double xi, int32_t levels);

/* out_dev: double [8] = msle, Hill index of x, Hill index of y, k of x, s[r0] of x, k of y, s[r0] of y, status.
 * status 1 = a non-finite value in a marginal (a NaN or an infinity in the data, or a norm beyond fp32): the three figures and the
 * thresholds are NaN.  status 2 = a quantile or a threshold <= 0, where a logarithm is undefined: msle is NaN if any of the
 * 2 x levels quantiles is <= 0, a set's Hill index is NaN if its s[r0] <= 0, the other figures are given.
 * quantiles_out_dev: null, or double [2][levels], the quantiles q_x(u_j) then q_y(u_j) (NaN under status 1).
 * One enqueue sequence on `stream` with no host synchronisation and no device value read on the host: the call can be captured in a
 * graph.  Integer atomics only, every fp64 sum in the fixed order above: the same inputs give the same bits.
 * DLPM_ERR_ARG for what dlpm_tail_workspace_bytes refuses and for a null or misaligned pointer (x, y: 4 bytes; out, quantiles: 8
 * bytes); a workspace that is not 16-byte aligned is DLPM_ERR_ARG, a short one DLPM_ERR_NOMEM -- all before any launch. */
int dlpm_tail_f32(const float *x_dev, int64_t n1, const float *y_dev, int64_t n2, int64_t D, int32_t marginal, double xi, int32_t levels,
                  void *workspace_dev, int64_t workspace_bytes, double *quantiles_out_dev, double *out_dev, dlpm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DLPM_AMD_TAIL_H */
