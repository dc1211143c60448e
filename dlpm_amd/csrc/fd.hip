// fd.hip -- Frechet distance between the Gaussians fitted to two feature sets X [n1, F] and Y [n2, F] (calculate_frechet_distance,
// bem/evaluate/fid_score.py:118-171, fed by calculate_activation_statistics = np.mean + np.cov):
//   fd = |mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr (S1 S2)^1/2
// in its real symmetric form.  With S1 = V L V^T the matrix K = H S2 H, H = V L^1/2 V^T, has the eigenvalues of S1 S2 and is
// symmetric positive semi-definite; it is formed in the eigenbasis of S1, K' = V^T K V = L^1/2 (V^T S2 V) L^1/2 (an orthogonal
// similarity: the same eigenvalues, and H itself is never multiplied out), and tr (S1 S2)^1/2 = sum sqrt(eig K').  No imaginary parts.
// All arithmetic is fp64, every summation order is fixed by the shape alone (the same bits on every call), no float atomics.
//   * statistics: column means from k_colstats<false>, added in chunk order; S = (X - mu)^T (X - mu) / (n - 1) as a rank-n update on
//     v_mfma_f64_16x16x4_f64 in 128 x 128 tiles, centred in fp64 while staged; upper-triangle tiles only; the rows are cut into a
//     number of chunks that depends on (n, F) only, every (chunk, tile) writes its own partial tile, k_fd_cov_reduce adds them in chunk
//     order, divides and mirrors (S is symmetric bit for bit).
//   * eigenproblem: cyclic one-sided (Hestenes) Jacobi on the ROWS of W (W = S at the start, S symmetric) with the rotations gathered
//     in Vt (= I at the start): at the end the rows of W = V^T S are orthogonal, |row i| = eigenvalue i >= 0, the rows of Vt are the
//     eigenvectors.  Order: round-robin tournament, m = F (+ 1 if odd: the bye) players, m - 1 rounds of m / 2 disjoint pairs, one
//     launch per round and one workgroup per pair; pair k of round r is (m - 1, r) for k = 0, else ((r + k) mod (m - 1),
//     (r - k) mod (m - 1)).  Rows p, q with a = |w_p|^2, b = |w_q|^2, g = w_p . w_q are rotated unless
//         |g| <= tol max(sqrt(a b), tol |S|_F^2),   tol = F 2^-53:
//     the first term is the usual relative test, the second the absolute floor that lets rows of norm ~ tol |S|_F (null directions:
//     constant or duplicated features, n < F) settle -- their mutual angles are rounding noise and the relative test alone never ends.
//     What the floor leaves undone moves an eigenvalue by at most ~F^1/2 tol |S|_F.  Convergence is an integer rotation counter that the
//     host reads once per sweep (so the call cannot be captured in a graph); no grid-wide barrier, no persistent kernel.  60 sweeps at
//     the most (status 2).
//   * the two F x F x F products T = Vt S2 and K' = T Vt^T are one NT kernel (C = A B^T, S2 symmetric) on the same MFMA tile loop.
#include <algorithm>
#include <cmath>

#include "metrics_common.h"
#include "mfma64_tile.h"
#include "../../include/dlpm_amd_fd.h"

using namespace dlpm;

namespace {

constexpr int64_t kMaxF = 4096;
constexpr int64_t kMaxRows = 1ll << 31;
constexpr int kMaxSweeps = 60;
constexpr int64_t kTargetBlocks = 512;      // workgroups the covariance pass aims at (two per CU)
constexpr int64_t kMaxChunks = 64;
constexpr int64_t kMinChunkRows = 256;

struct Header {
    int nonfinite, rotations;
    double norm2;                            // |W|_F^2 at the start of a Jacobi run
};

// The chunk rule, a function of (n, F) alone: `count` row chunks of `per` rows (a multiple of 16; the last may be shorter),
// about kTargetBlocks / tiles of them, none shorter than 256 rows, 64 at the most.
struct Chunks {
    int64_t per, count;
};

inline int64_t tiles_of(int64_t F) {
    const int64_t T = ceil_div(F, kTile);
    return T * (T + 1) / 2;
}

Chunks chunks_of(int64_t n, int64_t F) {
    int64_t want = std::min<int64_t>(kMaxChunks, std::max<int64_t>(1, kTargetBlocks / tiles_of(F)));
    want = std::max<int64_t>(1, std::min<int64_t>(want, n / kMinChunkRows));
    const int64_t per = ceil_div(ceil_div(n, want), 16) * 16;
    return Chunks{per, ceil_div(n, per)};
}

struct TileJob {
    // covariance partials: rows [chunk * per, ...) of x, centred on mean; part[(chunk * ntiles + tile)][128][128]
    const float *x;
    const double *mean;
    int64_t n, per;
    double *part;
    // NT product C = A B^T of F x F matrices, scaled by scale[i] scale[j] where scale is given
    const double *A, *B, *scale;
    double *C;
    int64_t F;
    int T;
};

// 128 x 128 tile on the tile loop of mfma64_tile.h.
// COV: K runs over the samples of a chunk; a step is 16 samples x 128 features of the two feature blocks, thread = (sample, 8
// features 16 apart), centred in fp64 as it is staged.  NT: K runs along the rows of A and B, thread = (row, 8-value half of the step).
template <bool COV>
__global__ void __launch_bounds__(kThreads) k_fd_tile(TileJob w) {
    __shared__ double smem[kImage];
    const int tid = threadIdx.x;
    const Lanes l = lanes_of(tid);
    int64_t ti, tj;
    if (COV) tile_of(blockIdx.x, w.T, ti, tj);
    else {
        ti = blockIdx.x / w.T;
        tj = blockIdx.x - ti * w.T;
    }
    const int64_t i0 = ti * kTile, j0 = tj * kTile, F = w.F;
    const int64_t r0 = COV ? (int64_t)blockIdx.y * w.per : 0;
    const int64_t r1 = COV ? (r0 + w.per < w.n ? r0 + w.per : w.n) : F;
    double va[8], vb[8];
    // COV: sample ck of the step, features cf + 16 e.  NT: row sr, values sk .. sk + 7 of the step.
    const int ck = tid >> 4, cf = tid & 15, sr = tid >> 1, sk = (tid & 1) * 8;
    double ma[8], mb[8];
    if (COV) {
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const int64_t fa = i0 + cf + 16 * e, fb = j0 + cf + 16 * e;
            ma[e] = fa < F ? w.mean[fa] : 0.0;
            mb[e] = fb < F ? w.mean[fb] : 0.0;
        }
    }
    auto load = [&](int64_t s) {
        if (COV) {
            const int64_t r = r0 + s * kKC + ck;
            const bool rok = r < r1;
            const float *row = w.x + (rok ? r : 0) * F;
#pragma unroll
            for (int e = 0; e < 8; e++) {
                const int64_t fa = i0 + cf + 16 * e, fb = j0 + cf + 16 * e;
                va[e] = (rok && fa < F) ? (double)row[fa] - ma[e] : 0.0;
                vb[e] = (rok && fb < F) ? (double)row[fb] - mb[e] : 0.0;
            }
        } else {
            const bool a_ok = i0 + sr < F, b_ok = j0 + sr < F;
            const double *pa = w.A + (a_ok ? i0 + sr : 0) * F, *pb = w.B + (b_ok ? j0 + sr : 0) * F;
#pragma unroll
            for (int e = 0; e < 8; e++) {
                const int64_t k = s * kKC + sk + e;
                va[e] = (a_ok && k < F) ? pa[k] : 0.0;
                vb[e] = (b_ok && k < F) ? pb[k] : 0.0;
            }
        }
    };

    auto store = [&]() {
        if (COV) {
#pragma unroll
            for (int e = 0; e < 8; e++) {
                smem[(cf + 16 * e) * kLD + ck] = va[e];
                smem[kTile * kLD + (cf + 16 * e) * kLD + ck] = vb[e];
            }
        } else {
            store_rows(smem, sr, sk, va, vb);
        }
    };

    Acc acc;
    acc_zero(acc);
    tile_loop(smem, r1 - r0, l, acc, load, store);

    const int64_t ntiles = (int64_t)w.T * (w.T + 1) / 2;
    double *pt = COV ? w.part + ((int64_t)blockIdx.y * ntiles + blockIdx.x) * (kTile * kTile) : nullptr;
#pragma unroll
    for (int bi = 0; bi < 4; bi++)
#pragma unroll
        for (int bj = 0; bj < 4; bj++)
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const int rl = tile_row(l, bi, reg), cl = tile_col(l, bj);
                const double v = acc[bi][bj][reg];
                if (COV) {
                    pt[rl * kTile + cl] = v;                   // the whole tile, its zero padding included: always inside `part`
                } else {
                    const int64_t gi = i0 + rl, gj = j0 + cl;
                    if (gi < F && gj < F) w.C[gi * F + gj] = w.scale ? (w.scale[gi] * v) * w.scale[gj] : v;
                }
            }
}

// S[i][j] = S[j][i] = (sum over the chunks, in chunk order) / (n - 1) for i <= j.  Grid (ntiles, 64), thread = one tile element.
__global__ void __launch_bounds__(256) k_fd_cov_reduce(const double *part, int64_t chunks, int T, int64_t F, int64_t n, double *sigma) {
    int64_t ti, tj;
    tile_of(blockIdx.x, T, ti, tj);
    const int e = (int)blockIdx.y * 256 + threadIdx.x, rl = e >> 7, cl = e & (kTile - 1);
    const int64_t gi = ti * kTile + rl, gj = tj * kTile + cl;
    if (gi > gj || gj >= F) return;
    const int64_t ntiles = (int64_t)T * (T + 1) / 2;
    double acc = 0.0;
    for (int64_t c = 0; c < chunks; c++) acc += part[(c * ntiles + blockIdx.x) * (kTile * kTile) + e];
    acc /= (double)(n - 1);
    sigma[gi * F + gj] = acc;
    sigma[gj * F + gi] = acc;
}

__global__ void k_fd_init(Header *h) {
    h->nonfinite = 0;
    h->rotations = 0;
    h->norm2 = 0.0;
}

// the statistics handed to dlpm_fd_from_stats_f64; the fp32 rows go through k_nonfinite
__global__ void __launch_bounds__(256) k_fd_finite(const double *p, int64_t total, Header *h) {
    bool bad = false;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) bad |= !isfinite(p[e]);
    if (bad) atomicOr(&h->nonfinite, 1);
}

__global__ void k_fd_status(const Header *h, int32_t *status) { *status = h->nonfinite ? 1 : 0; }

__global__ void __launch_bounds__(256) k_fd_identity(double *V, int64_t F) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < F * F) V[e] = (e / F == e % F) ? 1.0 : 0.0;
}

// sq[i] = |row i of W|^2, one workgroup per row
__global__ void __launch_bounds__(256) k_fd_rowsq(const double *W, int64_t F, double *sq) {
    __shared__ double sh[256];
    const double *row = W + (int64_t)blockIdx.x * F;
    double acc = 0.0;
    for (int64_t d = threadIdx.x; d < F; d += 256) acc += row[d] * row[d];
    const double t = block_sum<256>(acc, sh);
    if (threadIdx.x == 0) sq[blockIdx.x] = t;
}

// the start of a Jacobi run: |W|_F^2 from the row sums, the rotation counter to 0
__global__ void __launch_bounds__(256) k_fd_norm2(const double *sq, int64_t F, Header *h) {
    __shared__ double sh[256];
    double acc = 0.0;
    for (int64_t d = threadIdx.x; d < F; d += 256) acc += sq[d];
    const double t = block_sum<256>(acc, sh);
    if (threadIdx.x == 0) {
        h->norm2 = t;
        h->rotations = 0;
    }
}

__global__ void k_fd_zero_rotations(Header *h) { h->rotations = 0; }

// One round of the tournament, workgroup = pair.  Rows p and q of W (and of Vt where given) belong to this workgroup alone in this round.
template <int THREADS>
__global__ void __launch_bounds__(THREADS) k_fd_jacobi_round(double *W, double *Vt, int64_t F, int m, int r, double tol, Header *h) {
    __shared__ double sh[THREADS];
    const int k = blockIdx.x;
    const int p = k == 0 ? m - 1 : (r + k) % (m - 1), q = (r - k + (m - 1)) % (m - 1);
    if (p >= F || q >= F) return;                              // the bye of an odd F
    double *wp = W + (int64_t)p * F, *wq = W + (int64_t)q * F;
    double a = 0.0, b = 0.0, g = 0.0;
    for (int64_t d = threadIdx.x; d < F; d += THREADS) {
        const double x = wp[d], y = wq[d];
        a += x * x;
        b += y * y;
        g += x * y;
    }
    a = block_sum<THREADS>(a, sh);
    b = block_sum<THREADS>(b, sh);
    g = block_sum<THREADS>(g, sh);
    const double lim = tol * fmax(sqrt(a * b), tol * h->norm2);
    if (!(fabs(g) > lim)) return;                              // also where anything is NaN: a run on non-finite input ends at once
    if (threadIdx.x == 0) atomicAdd(&h->rotations, 1);
    const double zeta = (b - a) / (g + g);
    const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
    for (int64_t d = threadIdx.x; d < F; d += THREADS) {
        const double x = wp[d], y = wq[d];
        wp[d] = c * x - s * y;
        wq[d] = s * x + c * y;
    }
    if (Vt) {
        double *vp = Vt + (int64_t)p * F, *vq = Vt + (int64_t)q * F;
        for (int64_t d = threadIdx.x; d < F; d += THREADS) {
            const double x = vp[d], y = vq[d];
            vp[d] = c * x - s * y;
            vq[d] = s * x + c * y;
        }
    }
}

// sq[i] = |row i|^2 = eigenvalue^2  ->  eigenvalue^1/2
__global__ void __launch_bounds__(256) k_fd_root_scale(double *sq, int64_t F) {
    const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (d < F) sq[d] = sqrt(sqrt(sq[d]));
}

// K <- (K + K^T) / 2, thread = one pair i < j
__global__ void __launch_bounds__(256) k_fd_symmetrise(double *K, int64_t F) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= F * F) return;
    const int64_t i = e / F, j = e - i * F;
    if (i >= j) return;
    const double v = 0.5 * (K[i * F + j] + K[j * F + i]);
    K[i * F + j] = v;
    K[j * F + i] = v;
}

// out[8] = fd, |mu1 - mu2|^2, tr S1, tr S2, tr (S1 S2)^1/2, status, sweeps of run 1, sweeps of run 2; musq[i] = (eigenvalue i of K')^2
__global__ void __launch_bounds__(256) k_fd_final(const Header *h, const double *mu1, const double *s1, const double *mu2, const double *s2,
                                                 const double *musq, int64_t F, int capped, int sweeps1, int sweeps2, double *out) {
    __shared__ double sh[256];
    double dm = 0.0, t1 = 0.0, t2 = 0.0, tr = 0.0;
    for (int64_t d = threadIdx.x; d < F; d += 256) {
        const double df = mu1[d] - mu2[d];
        dm += df * df;
        t1 += s1[d * F + d];
        t2 += s2[d * F + d];
        tr += sqrt(sqrt(musq[d]));
    }
    dm = block_sum<256>(dm, sh);
    t1 = block_sum<256>(t1, sh);
    t2 = block_sum<256>(t2, sh);
    tr = block_sum<256>(tr, sh);
    if (threadIdx.x == 0) {
        const bool bad = h->nonfinite != 0;
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        out[0] = bad ? nan : ((dm + t1) + t2) - (tr + tr);
        out[1] = bad ? nan : dm;
        out[2] = bad ? nan : t1;
        out[3] = bad ? nan : t2;
        out[4] = bad ? nan : tr;
        out[5] = bad ? 1.0 : (capped ? 2.0 : 0.0);
        out[6] = (double)sweeps1;
        out[7] = (double)sweeps2;
    }
}

struct Layout {
    Chunks c1, c2;
    int64_t header, colpart, rowsq, mu1, mu2, sigma1, sigma2, W, Vt, T, part, total;   // byte offsets; what depends on n comes last
};

Layout layout_of(int64_t n1, int64_t n2, int64_t F) {
    Layout L{};
    L.c1 = chunks_of(n1, F);
    L.c2 = chunks_of(n2, F);
    const int64_t dbl = (int64_t)sizeof(double), mat = F * F * dbl;
    Carve c;
    L.header = c.take((int64_t)sizeof(Header));
    L.colpart = c.take(F * kColChunks * dbl);
    L.rowsq = c.take(F * dbl);
    L.mu1 = c.take(F * dbl);
    L.mu2 = c.take(F * dbl);
    L.sigma1 = c.take(mat);
    L.sigma2 = c.take(mat);
    L.W = c.take(mat);
    L.Vt = c.take(mat);
    L.T = c.take(mat);
    L.part = c.take(std::max(L.c1.count, L.c2.count) * tiles_of(F) * kTile * kTile * dbl);   // the two sets take turns
    L.total = c.total;
    return L;
}

int check_shape(const char *who, int64_t n1, int64_t n2, int64_t F) {
    DLPM_CHECK_ARG(n1 >= 2 && n2 >= 2, "%s: a covariance needs at least 2 rows, got n1=%lld n2=%lld", who, (long long)n1, (long long)n2);
    DLPM_CHECK_ARG(n1 < kMaxRows && n2 < kMaxRows, "%s: row count out of range", who);
    DLPM_CHECK_ARG(F >= 1 && F <= kMaxF, "%s: F must be in [1, %lld], got %lld", who, (long long)kMaxF, (long long)F);
    return DLPM_OK;
}

struct Ws {
    Header *hdr;
    double *colpart, *rowsq, *mu1, *mu2, *sigma1, *sigma2, *W, *Vt, *T, *part;
};

Ws carve(void *workspace, const Layout &L) {
    char *ws = static_cast<char *>(workspace);
    auto d = [&](int64_t off) { return reinterpret_cast<double *>(ws + off); };
    return Ws{reinterpret_cast<Header *>(ws + L.header), d(L.colpart), d(L.rowsq), d(L.mu1), d(L.mu2), d(L.sigma1), d(L.sigma2), d(L.W),
              d(L.Vt), d(L.T), d(L.part)};
}

// mean and covariance of one set; the header has been initialised
int stats_run(const float *x, int64_t n, int64_t F, const Chunks &ch, const Ws &w, double *mu, double *sigma, hipStream_t st) {
    ProfScope ps("fd_stats", 2.0 * (double)n * F * F, 4.0 * (double)n * F, st);
    const int T = (int)ceil_div(F, kTile);
    const int64_t ntiles = tiles_of(F);
    const Pts p{x, x, n, n, F};
    k_nonfinite<256><<<scan_grid(n * F), 256, 0, st>>>(p, &w.hdr->nonfinite);
    DLPM_LAUNCH_CHECK();
    k_colstats<false><<<dim3((unsigned)ceil_div(F, 256), kColChunks), 256, 0, st>>>(p, w.colpart);
    DLPM_LAUNCH_CHECK();
    k_colmean<double><<<(unsigned)ceil_div(F, 256), 256, 0, st>>>(w.colpart, n, F, mu);
    DLPM_LAUNCH_CHECK();
    TileJob j{};
    j.x = x;
    j.mean = mu;
    j.n = n;
    j.per = ch.per;
    j.part = w.part;
    j.F = F;
    j.T = T;
    k_fd_tile<true><<<dim3((unsigned)ntiles, (unsigned)ch.count), kThreads, 0, st>>>(j);
    DLPM_LAUNCH_CHECK();
    k_fd_cov_reduce<<<dim3((unsigned)ntiles, kTile * kTile / 256), 256, 0, st>>>(w.part, ch.count, T, F, n, sigma);
    DLPM_LAUNCH_CHECK();
    return DLPM_OK;
}

int product_nt(const double *A, const double *B, const double *scale, double *C, int64_t F, hipStream_t st) {
    TileJob j{};
    j.A = A;
    j.B = B;
    j.scale = scale;
    j.C = C;
    j.F = F;
    j.T = (int)ceil_div(F, kTile);
    k_fd_tile<false><<<(unsigned)(j.T * j.T), kThreads, 0, st>>>(j);
    DLPM_LAUNCH_CHECK();
    return DLPM_OK;
}

// cyclic Jacobi on the rows of W until a sweep rotates nothing; the number of sweeps made, 0 < *sweeps <= 60, *capped if the last one
// still rotated.  The host waits for the stream once per sweep.
int jacobi_run(const char *name, double *W, double *Vt, int64_t F, const Ws &w, int *sweeps, int *capped, hipStream_t st) {
    ProfScope ps(name, 0.0, 0.0, st);
    k_fd_rowsq<<<(unsigned)F, 256, 0, st>>>(W, F, w.rowsq);
    DLPM_LAUNCH_CHECK();
    k_fd_norm2<<<1, 256, 0, st>>>(w.rowsq, F, w.hdr);
    DLPM_LAUNCH_CHECK();
    const int m = (int)(F + (F & 1));
    const double tol = (double)F * 0x1p-53;
    *capped = 0;
    for (int s = 1;; s++) {
        for (int r = 0; r < m - 1; r++) {
            if (F <= 512) k_fd_jacobi_round<64><<<(unsigned)(m / 2), 64, 0, st>>>(W, Vt, F, m, r, tol, w.hdr);
            else k_fd_jacobi_round<256><<<(unsigned)(m / 2), 256, 0, st>>>(W, Vt, F, m, r, tol, w.hdr);
            DLPM_LAUNCH_CHECK();
        }
        int rotations = 0;
        DLPM_HIP(hipMemcpyAsync(&rotations, &w.hdr->rotations, sizeof(int), hipMemcpyDeviceToHost, st));
        DLPM_HIP(hipStreamSynchronize(st));
        *sweeps = s;
        if (rotations == 0) break;
        if (s == kMaxSweeps) {
            *capped = 1;
            break;
        }
        k_fd_zero_rotations<<<1, 1, 0, st>>>(w.hdr);
        DLPM_LAUNCH_CHECK();
    }
    return DLPM_OK;
}

// the figure from two pairs of statistics; the header has been initialised
int figure_run(const double *mu1, const double *s1, const double *mu2, const double *s2, int64_t F, const Ws &w, double *out, hipStream_t st) {
    const int64_t mat = F * F;
    k_fd_finite<<<scan_grid(F), 256, 0, st>>>(mu1, F, w.hdr);
    k_fd_finite<<<scan_grid(F), 256, 0, st>>>(mu2, F, w.hdr);
    k_fd_finite<<<scan_grid(mat), 256, 0, st>>>(s1, mat, w.hdr);
    k_fd_finite<<<scan_grid(mat), 256, 0, st>>>(s2, mat, w.hdr);
    DLPM_LAUNCH_CHECK();
    DLPM_HIP(hipMemcpyAsync(w.W, s1, (size_t)mat * sizeof(double), hipMemcpyDeviceToDevice, st));
    k_fd_identity<<<(unsigned)ceil_div(mat, 256), 256, 0, st>>>(w.Vt, F);
    DLPM_LAUNCH_CHECK();
    int sweeps1 = 0, sweeps2 = 0, cap1 = 0, cap2 = 0;
    int rc = jacobi_run("fd_jacobi_1", w.W, w.Vt, F, w, &sweeps1, &cap1, st);
    if (rc != DLPM_OK) return rc;
    {
        ProfScope ps("fd_gemm", 4.0 * (double)F * F * F, 40.0 * (double)mat, st);
        k_fd_rowsq<<<(unsigned)F, 256, 0, st>>>(w.W, F, w.rowsq);             // eigenvalue^2 of S1 ...
        DLPM_LAUNCH_CHECK();
        k_fd_root_scale<<<(unsigned)ceil_div(F, 256), 256, 0, st>>>(w.rowsq, F);   // ... -> eigenvalue^1/2
        DLPM_LAUNCH_CHECK();
        rc = product_nt(w.Vt, s2, nullptr, w.T, F, st);                       // T = V^T S2
        if (rc != DLPM_OK) return rc;
        rc = product_nt(w.T, w.Vt, w.rowsq, w.W, F, st);                      // K' = L^1/2 (T V) L^1/2
        if (rc != DLPM_OK) return rc;
        k_fd_symmetrise<<<(unsigned)ceil_div(mat, 256), 256, 0, st>>>(w.W, F);
        DLPM_LAUNCH_CHECK();
    }
    rc = jacobi_run("fd_jacobi_2", w.W, nullptr, F, w, &sweeps2, &cap2, st);
    if (rc != DLPM_OK) return rc;
    k_fd_rowsq<<<(unsigned)F, 256, 0, st>>>(w.W, F, w.rowsq);
    DLPM_LAUNCH_CHECK();
    k_fd_final<<<1, 256, 0, st>>>(w.hdr, mu1, s1, mu2, s2, w.rowsq, F, cap1 | cap2, sweeps1, sweeps2, out);
    DLPM_LAUNCH_CHECK();
    return DLPM_OK;
}

}  // namespace

extern "C" int64_t dlpm_fd_workspace_bytes(int64_t n1, int64_t n2, int64_t F) {
    const int rc = check_shape("dlpm_fd_workspace_bytes", n1, n2, F);
    if (rc != DLPM_OK) return rc;
    return layout_of(n1, n2, F).total;
}

extern "C" int dlpm_fd_stats_f32(const float *x_dev, int64_t n, int64_t F, void *workspace_dev, int64_t workspace_bytes, double *mu_out_dev,
                                 double *sigma_out_dev, int32_t *status_out_dev, dlpm_stream_t stream) {
    const int rc = check_shape("dlpm_fd_stats_f32", n, n, F);
    if (rc != DLPM_OK) return rc;
    DLPM_CHECK_ARG(x_dev && workspace_dev && mu_out_dev && sigma_out_dev && status_out_dev, "dlpm_fd_stats_f32: null pointer");
    DLPM_CHECK_ARG(aligned(x_dev, 4) && aligned(mu_out_dev, 8) && aligned(sigma_out_dev, 8) && aligned(status_out_dev, 4),
                   "dlpm_fd_stats_f32: misaligned input or output");
    const Layout L = layout_of(n, n, F);
    const int ws_rc = check_workspace("dlpm_fd_stats_f32", workspace_dev, workspace_bytes, L.total);
    if (ws_rc != DLPM_OK) return ws_rc;
    hipStream_t st = as_stream(stream);
    const Ws w = carve(workspace_dev, L);
    k_fd_init<<<1, 1, 0, st>>>(w.hdr);
    DLPM_LAUNCH_CHECK();
    const int r = stats_run(x_dev, n, F, L.c1, w, mu_out_dev, sigma_out_dev, st);
    if (r != DLPM_OK) return r;
    k_fd_status<<<1, 1, 0, st>>>(w.hdr, status_out_dev);
    DLPM_LAUNCH_CHECK();
    return DLPM_OK;
}

extern "C" int dlpm_fd_from_stats_f64(const double *mu1_dev, const double *sigma1_dev, const double *mu2_dev, const double *sigma2_dev,
                                      int64_t F, void *workspace_dev, int64_t workspace_bytes, double *out_dev, dlpm_stream_t stream) {
    const int rc = check_shape("dlpm_fd_from_stats_f64", 2, 2, F);
    if (rc != DLPM_OK) return rc;
    DLPM_CHECK_ARG(mu1_dev && sigma1_dev && mu2_dev && sigma2_dev && workspace_dev && out_dev, "dlpm_fd_from_stats_f64: null pointer");
    DLPM_CHECK_ARG(aligned(mu1_dev, 8) && aligned(sigma1_dev, 8) && aligned(mu2_dev, 8) && aligned(sigma2_dev, 8) && aligned(out_dev, 8),
                   "dlpm_fd_from_stats_f64: misaligned input or output");
    const Layout L = layout_of(2, 2, F);
    const int ws_rc = check_workspace("dlpm_fd_from_stats_f64", workspace_dev, workspace_bytes, L.total);
    if (ws_rc != DLPM_OK) return ws_rc;
    hipStream_t st = as_stream(stream);
    const Ws w = carve(workspace_dev, L);
    k_fd_init<<<1, 1, 0, st>>>(w.hdr);
    DLPM_LAUNCH_CHECK();
    return figure_run(mu1_dev, sigma1_dev, mu2_dev, sigma2_dev, F, w, out_dev, st);
}

extern "C" int dlpm_fd_f32(const float *x_dev, int64_t n1, const float *y_dev, int64_t n2, int64_t F, void *workspace_dev,
                           int64_t workspace_bytes, double *out_dev, dlpm_stream_t stream) {
    const int rc = check_shape("dlpm_fd_f32", n1, n2, F);
    if (rc != DLPM_OK) return rc;
    DLPM_CHECK_ARG(x_dev && y_dev && workspace_dev && out_dev, "dlpm_fd_f32: null pointer");
    DLPM_CHECK_ARG(aligned(x_dev, 4) && aligned(y_dev, 4) && aligned(out_dev, 8), "dlpm_fd_f32: misaligned input or output");
    const Layout L = layout_of(n1, n2, F);
    const int ws_rc = check_workspace("dlpm_fd_f32", workspace_dev, workspace_bytes, L.total);
    if (ws_rc != DLPM_OK) return ws_rc;
    hipStream_t st = as_stream(stream);
    const Ws w = carve(workspace_dev, L);
    k_fd_init<<<1, 1, 0, st>>>(w.hdr);
    DLPM_LAUNCH_CHECK();
    int r = stats_run(x_dev, n1, F, L.c1, w, w.mu1, w.sigma1, st);
    if (r != DLPM_OK) return r;
    r = stats_run(y_dev, n2, F, L.c2, w, w.mu2, w.sigma2, st);
    if (r != DLPM_OK) return r;
    return figure_run(w.mu1, w.sigma1, w.mu2, w.sigma2, F, w, out_dev, st);
}
