// metrics_common.h -- what the device metrics (mmd.hip, prd.hip, wass.hip, prdc.hip, fd.hip) and toy.hip share: the point set behind
// two pointers and its non-finite scan, the carving of a workspace into 256-byte aligned regions and its check, the alignment
// predicate, the chunked fp64 column statistics and their mean, the upper-triangle tile decode and the choice of a direct-form
// instantiation by D.  Everything here has internal linkage; what a region holds stays in each file's own Layout.  The fp64 MFMA tile
// loop of prdc.hip and fd.hip is in mfma64_tile.h.
#pragma once
#include <algorithm>
#include <type_traits>

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

bool aligned(const void *p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

int check_workspace(const char *who, const void *ws, int64_t have, int64_t need) {
    DLPM_CHECK_ARG(aligned(ws, 16), "%s: misaligned workspace", who);
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

// mean[d] = (T)(sum of the kColChunks partials of k_colstats<false>, in chunk order, / n).  Grid ceil(D / 256).
template <typename T>
__global__ void __launch_bounds__(256) k_colmean(const double *colpart, int64_t n, int64_t D, T *mean) {
    const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (d >= D) return;
    double acc = 0.0;
    for (int c = 0; c < kColChunks; c++) acc += colpart[(int64_t)c * D + d];
    mean[d] = (T)(acc / (double)n);
}

// *flag |= 1 where a value of p is not finite; scan_grid(p.n * p.D) workgroups.  A template, so that only the files that launch it
// carry it.
template <int THREADS>
__global__ void __launch_bounds__(THREADS) k_nonfinite(Pts p, int *flag) {
    const int64_t total = p.n * p.D, first = p.n1 * p.D;
    bool bad = false;
    for (int64_t e = (int64_t)blockIdx.x * THREADS + threadIdx.x; e < total; e += (int64_t)gridDim.x * THREADS) {
        const float v = e < first ? p.x[e] : p.y[e - first];
        bad |= !isfinite(v);
    }
    if (bad) atomicOr(flag, 1);
}

unsigned scan_grid(int64_t total) { return (unsigned)std::min<int64_t>(ceil_div(total, 256), 2048); }

// The upper triangle of a T x T tiling, row by row: row t holds the tiles (t, t) .. (t, T - 1) and starts at tile_row_start(t, T);
// tile b -> (ti, tj), ti <= tj.
__device__ inline int64_t tile_row_start(int64_t t, int64_t T) { return t * T - t * (t - 1) / 2; }

__device__ inline void tile_of(int64_t b, int64_t T, int64_t &ti, int64_t &tj) {
    const double s = 2.0 * (double)T + 1.0;
    int64_t t = (int64_t)((s - sqrt(fmax(s * s - 8.0 * (double)b, 0.0))) * 0.5);
    t = t < 0 ? 0 : (t > T - 1 ? T - 1 : t);
    while (t > 0 && tile_row_start(t, T) > b) t--;
    while (t + 1 < T && tile_row_start(t + 1, T) <= b) t++;
    ti = t;
    tj = t + (b - tile_row_start(t, T));
}

// The direct forms pad a row with zeros to DT = 2, 4, 8 or 16 values: f(std::integral_constant<int, DT>{}) for the smallest DT >= D,
// D <= 16.
template <typename F>
auto with_dt(int64_t D, F f) {
    if (D <= 2) return f(std::integral_constant<int, 2>{});
    if (D <= 4) return f(std::integral_constant<int, 4>{});
    if (D <= 8) return f(std::integral_constant<int, 8>{});
    return f(std::integral_constant<int, 16>{});
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
