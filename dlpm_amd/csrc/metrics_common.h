// metrics_common.h -- what the device metrics (mmd.hip, prd.hip, wass.hip) and toy.hip share: the point set behind two pointers, the carving of a
// workspace into 256-byte aligned regions and its check, and the chunked fp64 column statistics.  Everything here has internal
// linkage; what a region holds stays in each file's own Layout.
#pragma once
#include "common.h"

namespace dlpm {
namespace {

// the concatenation [x; y] of two fp32 row sets (n = n1 + n2 rows of D values) without a copy
struct Pts {
    const float *x, *y;
    int64_t n1, n, D;
};

__device__ inline const float *row_ptr(const Pts &p, int64_t i) { return i < p.n1 ? p.x + i * p.D : p.y + (i - p.n1) * p.D; }

// byte offsets of a workspace's regions, each a multiple of 256: take() returns where the region starts; `total` is the size so far
struct Carve {
    int64_t total = 0;
    int64_t take(int64_t bytes) {
        const int64_t at = total;
        total += (bytes + 255) / 256 * 256;
        return at;
    }
};

int check_workspace(const char *who, const void *ws, int64_t have, int64_t need) {
    DLPM_CHECK_ARG(reinterpret_cast<uintptr_t>(ws) % 16 == 0, "%s: misaligned workspace", who);
    if (have < need) {
        set_error("%s: workspace of %lld bytes, %lld needed", who, (long long)have, (long long)need);
        return DLPM_ERR_NOMEM;
    }
    return DLPM_OK;
}

constexpr int kColChunks = 32;      // row chunks of the column statistics

// sum x (SQ: and sum x^2) per column and row chunk, one thread per column and chunk, rows in index order:
// colpart[chunk][d] (SQ: colpart[chunk][d][2]).  Grid (ceil(D / 256), kColChunks).
template <bool SQ>
__global__ void __launch_bounds__(256) k_colstats(Pts p, double *colpart) {
    const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (d >= p.D) return;
    const int64_t per = (p.n + kColChunks - 1) / kColChunks;
    const int64_t r0 = (int64_t)blockIdx.y * per, r1 = r0 + per < p.n ? r0 + per : p.n;
    double acc = 0.0, q = 0.0;
    for (int64_t i = r0; i < r1; i++) {
        const double v = (double)row_ptr(p, i)[d];
        acc += v;
        if (SQ) q += v * v;
    }
    double *o = colpart + ((int64_t)blockIdx.y * p.D + d) * (SQ ? 2 : 1);
    o[0] = acc;
    if (SQ) o[1] = q;
}

// order-preserving 32-bit key of an fp32 (-0.0 sorts just below +0.0) and its inverse: what the exact selects of wass.hip and
// toy.hip sort by
__device__ inline unsigned int key_of(float v) {
    const unsigned int u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ inline float value_of(unsigned int k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

}  // namespace
}  // namespace dlpm
