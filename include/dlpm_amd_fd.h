/* dlpm_amd_fd.h -- the Frechet distance entry points of libdlpm_amd (same library, same ABI version as dlpm_amd.h, which this
 * header includes; the four functions live here so that the table of dlpm_amd.h stays as it is).
 *
 * Frechet distance between the Gaussians fitted to two feature sets x [n1, F] and y [n2, F], fp32 on the device:
 *   fd = |mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr (S1 S2)^1/2,   mu = column means, S = (X - mu)^T (X - mu) / (n - 1)  (np.mean, np.cov)
 * i.e. calculate_frechet_distance(mu1, sigma1, mu2, sigma2) of bem/evaluate/fid_score.py:118-171 on the statistics of
 * calculate_activation_statistics.  Geometry on two arrays: no network, no weights; "FID" is this figure on Inception pool3 features.
 * All arithmetic is fp64 with summation orders fixed by the shape: the same inputs give the same bits.  The covariance is a rank-n
 * update on the fp64 MFMA; tr (S1 S2)^1/2 = sum sqrt(eig K), K = H S2 H with H = S1^1/2, real and symmetric (no imaginary parts to
 * strip), from two cyclic one-sided Jacobi eigen-solves in round-robin order and two F x F x F products on the fp64 MFMA.  The host
 * reads a rotation counter once per sweep: the calls that solve (from_stats, fd_f32) WAIT ON THE STREAM and cannot be captured in a
 * hipGraph.  dlpm_fd_stats_f32 is one enqueue sequence without a synchronisation. */
#ifndef DLPM_AMD_FD_H
#define DLPM_AMD_FD_H
#include "dlpm_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace for dlpm_fd_f32(n1, n2, F); dlpm_fd_stats_f32 of n rows needs the answer for (n, n, F), dlpm_fd_from_stats_f64
 * the answer for (2, 2, F).  O(F^2) plus the covariance partial tiles.  DLPM_ERR_ARG (-1) for n1 < 2, n2 < 2, F < 1 or F > 4096. */
int64_t dlpm_fd_workspace_bytes(int64_t n1, int64_t n2, int64_t F);

/* mu_out_dev: double [F] column means; sigma_out_dev: double [F, F] covariance, symmetric bit for bit; status_out_dev: int32 [1],
 * 1 = a non-finite input value (the statistics then hold non-finite values), else 0.  DLPM_ERR_ARG for n < 2, F outside 1..4096 or a
 * null / misaligned pointer; DLPM_ERR_NOMEM for a short workspace (which must be 16-byte aligned) -- before any launch. */
int dlpm_fd_stats_f32(const float *x_dev, int64_t n, int64_t F, void *workspace_dev, int64_t workspace_bytes, double *mu_out_dev,
                      double *sigma_out_dev, int32_t *status_out_dev, dlpm_stream_t stream);

/* out_dev: double [8] = fd, |mu1 - mu2|^2, tr S1, tr S2, tr (S1 S2)^1/2, status, sweeps of the solve of S1, sweeps of the solve of K.
 * status 1 = a non-finite value in the statistics (the five figures are NaN); status 2 = a solve still rotated in its 60th sweep (the
 * figures are those of the unfinished solve).  sigma1 / sigma2: double [F, F], symmetric.  Refusals as above. */
int dlpm_fd_from_stats_f64(const double *mu1_dev, const double *sigma1_dev, const double *mu2_dev, const double *sigma2_dev, int64_t F,
                           void *workspace_dev, int64_t workspace_bytes, double *out_dev, dlpm_stream_t stream);

/* dlpm_fd_stats_f32 of x and of y (into the workspace) and dlpm_fd_from_stats_f64 in one call; status 1 also for a non-finite value
 * in x or y. */
int dlpm_fd_f32(const float *x_dev, int64_t n1, const float *y_dev, int64_t n2, int64_t F, void *workspace_dev, int64_t workspace_bytes,
                double *out_dev, dlpm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DLPM_AMD_FD_H */
