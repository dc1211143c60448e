// prd.hip -- the PRD precision / recall of bem/evaluate/prd_score.py:48-191 (called through prd_legacy.py:6-16 at
// EvaluationManager.py:157-168): num_runs k-means clusterings of the union of two point sets, the two cluster histograms of each, the
// precision-recall curve of the histograms averaged over the runs, and the maxima of F_beta and F_1/beta over the curve.
// The reference fits sklearn's MiniBatchKMeans(n_init=10) num_runs times, one after the other; here ALL run x init instances advance in
// lockstep in one grid (blockIdx.y = instance), as full-batch Lloyd iterations from a k-means++ seeding:
//   * points: the concatenation [eval; ref] (two pointers: Pts of metrics_common.h), fp32 rows; centres, sums, inertias, the curve: fp64.
//   * assign + accumulate, D <= 16: a workgroup stages its instance's K centres in LDS, a thread holds its point in registers (rows
//     zero-padded to DT), finds the nearest centre by sum (x - c)^2 in fp64 (lowest index on ties), writes the label; then thread (k, d)
//     scans the chunk's labels in index order and sums its members' coordinates, thread k counts them by set.
//   * assign + accumulate, D > 16: the same structure with the centres walked through LDS in tiles of 8 centres x 32 columns; the
//     sums go column by column (thread = column, points in index order).  Not tuned.
//   * update: one workgroup per instance merges the chunk partials in chunk order, divides (an empty cluster keeps its centre), sums the
//     shift, sets done[instance] at shift <= tol * mean per-feature variance (sklearn's rule) and `fixed` at shift == 0 (the labels
//     reproduce the centres).  Every kernel returns at entry for a done instance; the host enqueues max_iter rounds and reads nothing.
//   * k-means++: K steps of (distance to the newest centre, block sums) + (one workgroup per instance draws by inverse CDF over the
//     block sums, then inside the block); the draw is Philox keyed by (seed, run, init, step).
// No floating-point atomics anywhere, every reduction in a fixed order: the same inputs give the same bits.
#include <algorithm>

#include "metrics_common.h"
#include "philox.h"

using namespace dlpm;

namespace {

constexpr int kMaxK = 256;          // labels are bytes
constexpr int kDirectMaxD = 16;     // D <= this: point in registers
constexpr int64_t kMaxD = 4096;
constexpr int kMaxChunks = 512;     // point chunks per instance (a chunk is 256 * S points)
constexpr int kTileK = 8, kTileD = 32;   // centre tile of the general form
constexpr int64_t kMaxAngles = 1000000;
constexpr uint32_t kPurposeSeed = 0x50524431u;   // Philox purpose of the k-means++ draws

// instance = run * n_init + init; chunk c of an instance covers the points [c * 256 * S, (c + 1) * 256 * S)
struct Geo {
    int64_t n, D;
    int K, S, C, I, n_init, run0;
};

struct Work {
    double *centres;      // [I][K][D]
    double *psum;         // [I][C][K][D]
    int32_t *pcnt;        // [I][C][2][K]
    double *pinert;       // [I][C]
    double *mind2;        // [I][n]
    double *bsum;         // [I][C]
    uint8_t *labels;      // [I][n]
    int32_t *done, *iters, *fixed;   // [I]
    double *colpart;      // [kColChunks][D][2]
    double *tolvar;       // [1]
    double *cmax;         // [3 * curve blocks]
};

__device__ inline double uniform53(uint64_t seed, uint32_t run, uint32_t init, uint32_t step) {
    const uint4 r = philox4x32_10(make_uint4(run, init, step, kPurposeSeed), seed);
    const uint64_t bits = ((uint64_t)r.x << 21) | (uint64_t)(r.y >> 11);
    return (double)bits * (1.0 / 9007199254740992.0);      // [0, 1)
}

__global__ void __launch_bounds__(256) k_prd_init(int I, int32_t *done, int32_t *iters, int32_t *fixed) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < I) done[i] = iters[i] = fixed[i] = 0;
}

// tolvar = tol * mean over the columns of the (biased) variance: sklearn's _tolerance, from the chunk sums of k_colstats<true>
__global__ void __launch_bounds__(256) k_prd_tolvar(const double *colpart, int64_t n, int64_t D, double tol, double *tolvar) {
    __shared__ double sh[256];
    double acc = 0.0;
    for (int64_t d = threadIdx.x; d < D; d += 256) {
        double s = 0.0, q = 0.0;
        for (int c = 0; c < kColChunks; c++) {
            s += colpart[((int64_t)c * D + d) * 2];
            q += colpart[((int64_t)c * D + d) * 2 + 1];
        }
        const double m = s / (double)n;
        acc += fmax(q / (double)n - m * m, 0.0);
    }
    const double t = block_sum<256>(acc, sh);
    if (threadIdx.x == 0) tolvar[0] = tol * t / (double)D;
}

// k-means++ step `step` >= 1, first half: distance of every point to centre step - 1, running minimum, block sums
__global__ void __launch_bounds__(256) k_prd_seed_dist(Pts p, Geo g, Work w, int step) {
    __shared__ double sh[256];
    const int inst = blockIdx.y;
    const double *c = w.centres + ((int64_t)inst * g.K + (step - 1)) * g.D;
    double *md = w.mind2 + (int64_t)inst * g.n;
    double acc = 0.0;
    for (int s = 0; s < g.S; s++) {
        const int64_t i = ((int64_t)blockIdx.x * g.S + s) * 256 + threadIdx.x;
        if (i < g.n) {
            const float *row = row_ptr(p, i);
            double dist = 0.0;
            for (int64_t d = 0; d < g.D; d++) {
                const double df = (double)row[d] - c[d];
                dist += df * df;
            }
            if (step > 1) dist = fmin(dist, md[i]);
            md[i] = dist;
            acc += dist;
        }
    }
    const double t = block_sum<256>(acc, sh);
    if (threadIdx.x == 0) w.bsum[(int64_t)inst * g.C + blockIdx.x] = t;
}

// second half: centre `step` of every instance.  step 0: a uniform point; later: point i with probability mind2[i] / sum, by inverse
// CDF over the block sums (chunk order) and then over the chunk's points (index order); all distances 0: a uniform point.
__global__ void __launch_bounds__(256) k_prd_seed_draw(Pts p, Geo g, Work w, uint64_t seed, int step) {
    __shared__ double sb[kMaxChunks];
    __shared__ double sm[256];
    __shared__ long long chosen;
    __shared__ int chunk;
    __shared__ double rest;
    const int inst = blockIdx.x, tid = threadIdx.x;
    const double u = uniform53(seed, (uint32_t)(g.run0 + inst / g.n_init), (uint32_t)(inst % g.n_init), (uint32_t)step);
    int64_t uni = (int64_t)(u * (double)g.n);
    uni = uni > g.n - 1 ? g.n - 1 : uni;
    if (step == 0) {
        if (tid == 0) chosen = uni;
    } else {
        for (int c = tid; c < g.C; c += 256) sb[c] = w.bsum[(int64_t)inst * g.C + c];
        __syncthreads();
        if (tid == 0) {
            double total = 0.0;
            for (int c = 0; c < g.C; c++) total += sb[c];
            chosen = -1;
            chunk = -1;
            if (!(total > 0.0)) {
                chosen = uni;
            } else {
                double r = u * total;
                int last = 0;
                for (int c = 0; c < g.C; c++) {
                    if (sb[c] > 0.0) {
                        last = c;
                        if (r < sb[c]) {
                            chunk = c;
                            break;
                        }
                        r -= sb[c];
                    }
                }
                if (chunk < 0) {          // rounding walked past the end: the last chunk that holds weight, at its end
                    chunk = last;
                    r = sb[last];
                }
                rest = r;
            }
        }
        __syncthreads();
        if (chunk >= 0) {
            const double *md = w.mind2 + (int64_t)inst * g.n;
            for (int s = 0; s < g.S; s++) {
                const int64_t base = ((int64_t)chunk * g.S + s) * 256;
                sm[tid] = base + tid < g.n ? md[base + tid] : 0.0;
                __syncthreads();
                if (tid == 0 && chosen < 0) {
                    double r = rest;
                    for (int j = 0; j < 256; j++) {
                        if (sm[j] > 0.0) {
                            if (r < sm[j]) {
                                chosen = base + j;
                                break;
                            }
                            r -= sm[j];
                        }
                    }
                    rest = r;
                }
                __syncthreads();
            }
            if (tid == 0 && chosen < 0) {     // the same rounding inside the chunk: its last point that holds weight
                const int64_t b0 = (int64_t)chunk * g.S * 256, b1 = b0 + (int64_t)g.S * 256 < g.n ? b0 + (int64_t)g.S * 256 : g.n;
                int64_t pick = b0;
                for (int64_t i = b0; i < b1; i++)
                    if (md[i] > 0.0) pick = i;
                chosen = pick;
            }
        }
    }
    __syncthreads();
    const float *row = row_ptr(p, (int64_t)chosen);
    double *c = w.centres + ((int64_t)inst * g.K + step) * g.D;
    for (int64_t d = tid; d < g.D; d += 256) c[d] = (double)row[d];
}

// counts of the chunk's labels by set and the inertia partial: the tail both assign kernels share
__device__ inline void count_members(const int *sl, int64_t base, int64_t n1, int K, int &ce, int &cr) {
    const int k = threadIdx.x;
    if (k < K) {
        for (int j = 0; j < 256; j++)
            if (sl[j] == k) {
                if (base + j < n1) ce++;
                else cr++;
            }
    }
}

// Direct form, rows padded with zeros to DT >= D ((0 - 0)^2 adds an exact 0).  force: the pass after the last round, which runs for
// done instances too (labels, counts and inertia of the final centres).
template <int DT>
__global__ void __launch_bounds__(256) k_prd_assign(Pts p, Geo g, Work w, int force) {
    __shared__ double sc[kMaxK * DT];
    __shared__ float sp[256 * DT];
    __shared__ int sl[256];
    __shared__ double sh[256];
    const int inst = blockIdx.y, tid = threadIdx.x, K = g.K;
    if (!force && w.done[inst]) return;
    const double *cen = w.centres + (int64_t)inst * K * g.D;
    for (int e = tid; e < K * DT; e += 256) {
        const int k = e / DT, d = e - k * DT;
        sc[e] = d < g.D ? cen[(int64_t)k * g.D + d] : 0.0;
    }
    double acc[DT];
#pragma unroll
    for (int q = 0; q < DT; q++) acc[q] = 0.0;
    int ce = 0, cr = 0;
    double inert = 0.0;
    uint8_t *lab = w.labels + (int64_t)inst * g.n;
    for (int s = 0; s < g.S; s++) {
        const int64_t base = ((int64_t)blockIdx.x * g.S + s) * 256, i = base + tid;
        const bool ok = i < g.n;
        float a[DT];
        const float *row = row_ptr(p, ok ? i : 0);
#pragma unroll
        for (int d = 0; d < DT; d++) {
            a[d] = (ok && d < g.D) ? row[d] : 0.f;
            sp[tid * DT + d] = a[d];
        }
        __syncthreads();                       // the centres (first pass) and last pass's readers of sp / sl
        double best = 0.0;
        int bk = 0;
        for (int k = 0; k < K; k++) {
            double dist = 0.0;
#pragma unroll
            for (int d = 0; d < DT; d++) {
                const double df = (double)a[d] - sc[k * DT + d];
                dist += df * df;
            }
            if (k == 0 || dist < best) {
                best = dist;
                bk = k;
            }
        }
        sl[tid] = ok ? bk : -1;
        if (ok) {
            lab[i] = (uint8_t)bk;
            inert += best;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < DT; q++) {
            const int e = tid + 256 * q;
            if (e < K * DT) {
                const int k = e / DT, d = e - k * DT;
                double t = acc[q];
                for (int j = 0; j < 256; j++)
                    if (sl[j] == k) t += (double)sp[j * DT + d];
                acc[q] = t;
            }
        }
        count_members(sl, base, p.n1, K, ce, cr);
        __syncthreads();
    }
    const int64_t slot = (int64_t)inst * g.C + blockIdx.x;
    double *ps = w.psum + slot * K * g.D;
#pragma unroll
    for (int q = 0; q < DT; q++) {
        const int e = tid + 256 * q;
        if (e < K * DT) {
            const int k = e / DT, d = e - k * DT;
            if (d < g.D) ps[(int64_t)k * g.D + d] = acc[q];
        }
    }
    if (tid < K) {
        w.pcnt[slot * 2 * K + tid] = ce;
        w.pcnt[slot * 2 * K + K + tid] = cr;
    }
    const double t = block_sum<256>(inert, sh);
    if (tid == 0) w.pinert[slot] = t;
}

// General form (D > 16): centres through LDS in tiles of kTileK x kTileD, the point read from memory; the partial sums are built in
// place in the workspace, thread = column, points in index order.
__global__ void __launch_bounds__(256) k_prd_assign_general(Pts p, Geo g, Work w, int force) {
    __shared__ double sc[kTileK * kTileD];
    __shared__ int sl[256];
    __shared__ double sh[256];
    const int inst = blockIdx.y, tid = threadIdx.x, K = g.K;
    if (!force && w.done[inst]) return;
    const int64_t D = g.D;
    const double *cen = w.centres + (int64_t)inst * K * D;
    const int64_t slot = (int64_t)inst * g.C + blockIdx.x;
    double *ps = w.psum + slot * K * D;
    for (int64_t e = tid; e < (int64_t)K * D; e += 256) ps[e] = 0.0;
    int ce = 0, cr = 0;
    double inert = 0.0;
    uint8_t *lab = w.labels + (int64_t)inst * g.n;
    const int kk_s = tid / kTileD, dd_s = tid - kk_s * kTileD;
    for (int s = 0; s < g.S; s++) {
        const int64_t base = ((int64_t)blockIdx.x * g.S + s) * 256, i = base + tid;
        const bool ok = i < g.n;
        const float *row = row_ptr(p, ok ? i : 0);
        double best = 0.0;
        int bk = 0;
        for (int k0 = 0; k0 < K; k0 += kTileK) {
            double acc[kTileK];
#pragma unroll
            for (int kk = 0; kk < kTileK; kk++) acc[kk] = 0.0;
            for (int64_t d0 = 0; d0 < D; d0 += kTileD) {
                __syncthreads();
                sc[tid] = (k0 + kk_s < K && d0 + dd_s < D) ? cen[(int64_t)(k0 + kk_s) * D + d0 + dd_s] : 0.0;
                __syncthreads();
                const int dn = D - d0 < kTileD ? (int)(D - d0) : kTileD;
                for (int dd = 0; dd < dn; dd++) {
                    const double x = (double)row[d0 + dd];
#pragma unroll
                    for (int kk = 0; kk < kTileK; kk++) {
                        const double df = x - sc[kk * kTileD + dd];
                        acc[kk] += df * df;
                    }
                }
            }
#pragma unroll
            for (int kk = 0; kk < kTileK; kk++)
                if (k0 + kk < K && ((k0 == 0 && kk == 0) || acc[kk] < best)) {
                    best = acc[kk];
                    bk = k0 + kk;
                }
        }
        __syncthreads();                       // last pass's readers of sl
        sl[tid] = ok ? bk : -1;
        if (ok) {
            lab[i] = (uint8_t)bk;
            inert += best;
        }
        __syncthreads();
        for (int64_t d = tid; d < D; d += 256)
            for (int j = 0; j < 256; j++) {
                const int l = sl[j];
                if (l >= 0) ps[(int64_t)l * D + d] += (double)row_ptr(p, base + j)[d];
            }
        count_members(sl, base, p.n1, K, ce, cr);
    }
    if (tid < K) {
        w.pcnt[slot * 2 * K + tid] = ce;
        w.pcnt[slot * 2 * K + K + tid] = cr;
    }
    const double t = block_sum<256>(inert, sh);
    if (tid == 0) w.pinert[slot] = t;
}

__global__ void __launch_bounds__(256) k_prd_update(Geo g, Work w) {
    __shared__ double sh[256];
    const int inst = blockIdx.x, K = g.K;
    if (w.done[inst]) return;
    const int64_t D = g.D, KD = (int64_t)K * D;
    double *cen = w.centres + (int64_t)inst * KD;
    const double *ps = w.psum + (int64_t)inst * g.C * KD;
    const int32_t *pc = w.pcnt + (int64_t)inst * g.C * 2 * K;
    double shift = 0.0;
    for (int64_t e = threadIdx.x; e < KD; e += 256) {
        const int k = (int)(e / D);
        double sum = 0.0;
        int64_t cnt = 0;
        for (int c = 0; c < g.C; c++) {
            sum += ps[(int64_t)c * KD + e];
            cnt += pc[(int64_t)c * 2 * K + k] + pc[(int64_t)c * 2 * K + K + k];
        }
        if (cnt > 0) {
            const double nc = sum / (double)cnt, df = nc - cen[e];
            cen[e] = nc;
            shift += df * df;
        }
    }
    const double t = block_sum<256>(shift, sh);
    if (threadIdx.x == 0) {
        w.iters[inst] += 1;
        if (t <= w.tolvar[0]) w.done[inst] = 1;
        if (t == 0.0) w.fixed[inst] = 1;
    }
}

// per run: the init of lowest inertia (lowest index on ties); its centres, labels, merged counts, inertia, rounds, fixed-point flag
__global__ void __launch_bounds__(256) k_prd_select(Geo g, Work w, double *centres_out, uint8_t *labels_out, int32_t *counts_out,
                                                    double *inertia_out, int32_t *iters_out, int32_t *fixed_out) {
    __shared__ double sh[256];
    const int run = blockIdx.x, tid = threadIdx.x, K = g.K;
    int best = 0;
    double bi = 0.0;
    for (int j = 0; j < g.n_init; j++) {
        const double *pi = w.pinert + ((int64_t)run * g.n_init + j) * g.C;
        double acc = 0.0;
        for (int c = tid; c < g.C; c += 256) acc += pi[c];
        const double t = block_sum<256>(acc, sh);
        if (j == 0 || t < bi) {
            bi = t;
            best = j;
        }
    }
    const int64_t inst = (int64_t)run * g.n_init + best, KD = (int64_t)K * g.D;
    if (centres_out)
        for (int64_t e = tid; e < KD; e += 256) centres_out[(int64_t)run * KD + e] = w.centres[inst * KD + e];
    if (labels_out)
        for (int64_t i = tid; i < g.n; i += 256) labels_out[(int64_t)run * g.n + i] = w.labels[inst * g.n + i];
    for (int e = tid; e < 2 * K; e += 256) {
        int32_t cnt = 0;
        for (int c = 0; c < g.C; c++) cnt += w.pcnt[(inst * g.C + c) * 2 * K + e];
        counts_out[(int64_t)run * 2 * K + e] = cnt;
    }
    if (tid == 0) {
        if (inertia_out) inertia_out[run] = bi;
        if (iters_out) iters_out[run] = w.iters[inst];
        if (fixed_out) fixed_out[run] = w.fixed[inst];
    }
}

// prd_score.py:84-103 per run, :189-190 over the runs, :226-227 for both betas.  angles as numpy's linspace: i * step + start, the
// last one the stop value itself.  out: precision[A], recall[A]; cmax[block] = (max F_beta, max F_1/beta, max before clipping).
__global__ void __launch_bounds__(256) k_prd_curve(const int32_t *counts, int64_t n1, int64_t n2, int K, int R, int A, double eps,
                                                   double beta, double *out, double *cmax) {
    __shared__ double sh[256];
    const int a = blockIdx.x * 256 + threadIdx.x;
    double fb = 0.0, fi = 0.0, raw = 0.0;
    if (a < A) {
        const double start = eps, stop = 1.5707963267948966 - eps, step = (stop - start) / (double)(A - 1);
        const double angle = a == A - 1 ? stop : (double)a * step + start;
        const double slope = tan(angle);
        double ps = 0.0, rs = 0.0;
        for (int r = 0; r < R; r++) {
            const int32_t *ce = counts + (int64_t)r * 2 * K, *cr = ce + K;
            double pr = 0.0;
            for (int k = 0; k < K; k++) pr += fmin((double)cr[k] / (double)n2 * slope, (double)ce[k] / (double)n1);
            const double rc = pr / slope;
            raw = fmax(raw, fmax(pr, rc));
            ps += fmin(fmax(pr, 0.0), 1.0);
            rs += fmin(fmax(rc, 0.0), 1.0);
        }
        const double pm = ps / (double)R, rm = rs / (double)R;
        out[a] = pm;
        out[A + a] = rm;
        const double b2 = beta * beta, ib = 1.0 / beta, i2 = ib * ib;
        fb = (1.0 + b2) * (pm * rm) / ((b2 * pm) + rm + 1e-10);
        fi = (1.0 + i2) * (pm * rm) / ((i2 * pm) + rm + 1e-10);
    }
    const double v[3] = {fb, fi, raw};
    for (int q = 0; q < 3; q++) {
        const double m = block_max<256>(v[q], sh);
        if (threadIdx.x == 0) cmax[(int64_t)blockIdx.x * 3 + q] = m;
    }
}

__global__ void __launch_bounds__(256) k_prd_curve_final(const double *cmax, int blocks, double *out3) {
    __shared__ double sh[256];
    for (int q = 0; q < 3; q++) {
        double m = 0.0;
        for (int b = threadIdx.x; b < blocks; b += 256) m = fmax(m, cmax[(int64_t)b * 3 + q]);
        m = block_max<256>(m, sh);
        if (threadIdx.x == 0) out3[q] = m;
    }
}

__global__ void __launch_bounds__(256) k_prd_copy_f64(const double *src, double *dst, int64_t count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < count) dst[i] = src[i];
}

struct Layout {
    Geo g;
    int64_t centres, psum, pcnt, pinert, mind2, bsum, labels, flags, colpart, tolvar, cmax;    // Work, byte offsets
    int64_t o_centres, o_labels, o_counts, o_inertia, o_iters, o_fixed;                          // outputs the caller did not ask for
    int64_t total;
};

Layout layout_of(int64_t n, int64_t D, int K, int R, int n_init) {
    Layout L{};
    Geo &g = L.g;
    g.n = n;
    g.D = D;
    g.K = K;
    g.S = (int)std::max<int64_t>(1, ceil_div(n, 256 * (int64_t)kMaxChunks));
    g.C = (int)ceil_div(n, 256 * (int64_t)g.S);
    g.I = R * n_init;
    g.n_init = n_init;
    g.run0 = 0;
    const int64_t I = g.I, KD = (int64_t)K * D;
    Carve c;
    L.centres = c.take(I * KD * 8);
    L.psum = c.take(I * g.C * KD * 8);
    L.pcnt = c.take(I * g.C * 2 * K * 4);
    L.pinert = c.take(I * g.C * 8);
    L.mind2 = c.take(I * n * 8);
    L.bsum = c.take(I * g.C * 8);
    L.labels = c.take(I * n);
    L.flags = c.take(3 * I * 4);
    L.colpart = c.take((int64_t)kColChunks * D * 2 * 8);
    L.tolvar = c.take(8);
    L.cmax = c.take(ceil_div(kMaxAngles, 256) * 3 * 8);
    L.o_centres = c.take((int64_t)R * KD * 8);
    L.o_labels = c.take((int64_t)R * n);
    L.o_counts = c.take((int64_t)R * 2 * K * 4);
    L.o_inertia = c.take((int64_t)R * 8);
    L.o_iters = c.take((int64_t)R * 4);
    L.o_fixed = c.take((int64_t)R * 4);
    L.total = c.total;
    return L;
}

Work work_of(const Layout &L, void *workspace) {
    char *ws = static_cast<char *>(workspace);
    Work w{};
    w.centres = reinterpret_cast<double *>(ws + L.centres);
    w.psum = reinterpret_cast<double *>(ws + L.psum);
    w.pcnt = reinterpret_cast<int32_t *>(ws + L.pcnt);
    w.pinert = reinterpret_cast<double *>(ws + L.pinert);
    w.mind2 = reinterpret_cast<double *>(ws + L.mind2);
    w.bsum = reinterpret_cast<double *>(ws + L.bsum);
    w.labels = reinterpret_cast<uint8_t *>(ws + L.labels);
    w.done = reinterpret_cast<int32_t *>(ws + L.flags);
    w.iters = w.done + L.g.I;
    w.fixed = w.iters + L.g.I;
    w.colpart = reinterpret_cast<double *>(ws + L.colpart);
    w.tolvar = reinterpret_cast<double *>(ws + L.tolvar);
    w.cmax = reinterpret_cast<double *>(ws + L.cmax);
    return w;
}

int check_shape(const char *who, int64_t n1, int64_t n2, int64_t D, int64_t K, int64_t R, int64_t n_init) {
    DLPM_CHECK_ARG(n1 >= 1 && n2 >= 1 && D >= 1, "%s: bad shape n1=%lld n2=%lld D=%lld", who, (long long)n1, (long long)n2, (long long)D);
    DLPM_CHECK_ARG(D <= kMaxD, "%s: D must be at most %lld, got %lld", who, (long long)kMaxD, (long long)D);
    DLPM_CHECK_ARG(n1 + n2 < (1ll << 31), "%s: more than 2^31 - 1 points in all", who);   // the counts are 32-bit
    DLPM_CHECK_ARG(K >= 1 && K <= kMaxK, "%s: num_clusters must be in [1, %d], got %lld", who, kMaxK, (long long)K);
    DLPM_CHECK_ARG(K <= n1 + n2, "%s: num_clusters %lld exceeds the %lld points", who, (long long)K, (long long)(n1 + n2));
    DLPM_CHECK_ARG(R >= 1, "%s: num_runs must be at least 1, got %lld", who, (long long)R);
    DLPM_CHECK_ARG(n_init >= 1, "%s: n_init must be at least 1, got %lld", who, (long long)n_init);
    DLPM_CHECK_ARG(R * n_init <= 65535 && R <= 65535 && n_init <= 65535, "%s: num_runs * n_init must be at most 65535", who);
    return DLPM_OK;
}

int check_curve(const char *who, int64_t A, double eps, double beta) {
    DLPM_CHECK_ARG(A >= 3 && A <= kMaxAngles, "%s: num_angles must be in [3, 1e6], got %lld", who, (long long)A);
    DLPM_CHECK_ARG(eps > 0.0 && eps < 0.1, "%s: epsilon must be in (0, 0.1), got %g", who, eps);
    DLPM_CHECK_ARG(beta > 0.0, "%s: beta must be positive, got %g", who, beta);
    return DLPM_OK;
}

int launch_assign(const Pts &p, const Geo &g, const Work &w, int force, hipStream_t st) {
    const dim3 grid((unsigned)g.C, (unsigned)g.I);
    if (g.D <= kDirectMaxD) with_dt(g.D, [&](auto dt) { k_prd_assign<decltype(dt)::value><<<grid, 256, 0, st>>>(p, g, w, force); });
    else k_prd_assign_general<<<grid, 256, 0, st>>>(p, g, w, force);
    DLPM_LAUNCH_CHECK();
    return DLPM_OK;
}

struct Outs {
    double *centres;
    uint8_t *labels;
    int32_t *counts;
    double *inertia;
    int32_t *iters, *fixed;
};

// null outputs land in the workspace
Outs outs_of(const Layout &L, void *workspace, Outs o) {
    char *ws = static_cast<char *>(workspace);
    if (!o.centres) o.centres = reinterpret_cast<double *>(ws + L.o_centres);
    if (!o.labels) o.labels = reinterpret_cast<uint8_t *>(ws + L.o_labels);
    if (!o.counts) o.counts = reinterpret_cast<int32_t *>(ws + L.o_counts);
    if (!o.inertia) o.inertia = reinterpret_cast<double *>(ws + L.o_inertia);
    if (!o.iters) o.iters = reinterpret_cast<int32_t *>(ws + L.o_iters);
    if (!o.fixed) o.fixed = reinterpret_cast<int32_t *>(ws + L.o_fixed);
    return o;
}

int finish(const Pts &p, const Geo &g, const Work &w, const Outs &o, hipStream_t st) {
    ProfScope ps("prd_finish", 3.0 * (double)g.I * g.n * g.K * g.D, 4.0 * (double)g.I * g.n * g.D, st);
    const int rc = launch_assign(p, g, w, 1, st);
    if (rc != DLPM_OK) return rc;
    k_prd_select<<<(unsigned)(g.I / g.n_init), 256, 0, st>>>(g, w, o.centres, o.labels, o.counts, o.inertia, o.iters, o.fixed);
    DLPM_LAUNCH_CHECK();
    return DLPM_OK;
}

int run_kmeans(const Pts &p, const Geo &g, const Work &w, const Outs &o, int max_iter, double tol, uint64_t seed, hipStream_t st) {
    k_prd_init<<<(unsigned)ceil_div(g.I, 256), 256, 0, st>>>(g.I, w.done, w.iters, w.fixed);
    DLPM_LAUNCH_CHECK();
    k_colstats<true><<<dim3((unsigned)ceil_div(g.D, 256), kColChunks), 256, 0, st>>>(p, w.colpart);
    DLPM_LAUNCH_CHECK();
    k_prd_tolvar<<<1, 256, 0, st>>>(w.colpart, g.n, g.D, tol, w.tolvar);
    DLPM_LAUNCH_CHECK();
    const dim3 grid((unsigned)g.C, (unsigned)g.I);
    {
        ProfScope ps("prd_seed", 3.0 * (double)g.I * g.n * g.K * g.D, 4.0 * (double)g.I * g.n * g.D * g.K, st);
        for (int step = 0; step < g.K; step++) {
            if (step > 0) {
                k_prd_seed_dist<<<grid, 256, 0, st>>>(p, g, w, step);
                DLPM_LAUNCH_CHECK();
            }
            k_prd_seed_draw<<<(unsigned)g.I, 256, 0, st>>>(p, g, w, seed, step);
            DLPM_LAUNCH_CHECK();
        }
    }
    {
        ProfScope ps("prd_lloyd", 3.0 * (double)g.I * g.n * g.K * g.D * max_iter, 4.0 * (double)g.I * g.n * g.D * max_iter, st);
        for (int it = 0; it < max_iter; it++) {
            const int rc = launch_assign(p, g, w, 0, st);
            if (rc != DLPM_OK) return rc;
            k_prd_update<<<(unsigned)g.I, 256, 0, st>>>(g, w);
            DLPM_LAUNCH_CHECK();
        }
    }
    return finish(p, g, w, o, st);
}

int run_curve(const int32_t *counts, int64_t n1, int64_t n2, int K, int R, int A, double eps, double beta, double *cmax, double *out,
              hipStream_t st) {
    ProfScope ps("prd_curve", 4.0 * (double)A * R * K, 8.0 * (double)A * 2, st);
    const int blocks = (int)ceil_div(A, 256);
    k_prd_curve<<<blocks, 256, 0, st>>>(counts, n1, n2, K, R, A, eps, beta, out, cmax);
    DLPM_LAUNCH_CHECK();
    k_prd_curve_final<<<1, 256, 0, st>>>(cmax, blocks, out + 2 * (int64_t)A);
    DLPM_LAUNCH_CHECK();
    return DLPM_OK;
}

}  // namespace

extern "C" int64_t dlpm_prd_workspace_bytes(int64_t n1, int64_t n2, int64_t D, int32_t num_clusters, int32_t num_runs, int32_t n_init) {
    const int rc = check_shape("dlpm_prd_workspace_bytes", n1, n2, D, num_clusters, num_runs, n_init);
    if (rc != DLPM_OK) return rc;
    return layout_of(n1 + n2, D, num_clusters, num_runs, n_init).total;
}

extern "C" int dlpm_kmeans_f32(const float *x_dev, int64_t n1, const float *y_dev, int64_t n2, int64_t D, int32_t num_clusters,
                               int32_t num_runs, int32_t n_init, int32_t max_iter, double tol, uint64_t seed, int32_t first_run,
                               void *workspace_dev, int64_t workspace_bytes, double *centres_out_dev, uint8_t *labels_out_dev,
                               int32_t *counts_out_dev, double *inertia_out_dev, int32_t *iters_out_dev, int32_t *converged_out_dev,
                               dlpm_stream_t stream) {
    const char *who = "dlpm_kmeans_f32";
    int rc = check_shape(who, n1, n2, D, num_clusters, num_runs, n_init);
    if (rc != DLPM_OK) return rc;
    DLPM_CHECK_ARG(max_iter >= 1, "%s: max_iter must be at least 1, got %d", who, max_iter);
    DLPM_CHECK_ARG(tol >= 0.0, "%s: tol must not be negative, got %g", who, tol);
    DLPM_CHECK_ARG(first_run >= 0, "%s: first_run must not be negative, got %d", who, first_run);
    DLPM_CHECK_ARG(x_dev && y_dev && workspace_dev && centres_out_dev && labels_out_dev && counts_out_dev && inertia_out_dev &&
                       iters_out_dev && converged_out_dev, "%s: null pointer", who);
    Layout L = layout_of(n1 + n2, D, num_clusters, num_runs, n_init);
    rc = check_workspace(who, workspace_dev, workspace_bytes, L.total);
    if (rc != DLPM_OK) return rc;
    L.g.run0 = first_run;
    const Pts p{x_dev, y_dev, n1, n1 + n2, D};
    const Outs o{centres_out_dev, labels_out_dev, counts_out_dev, inertia_out_dev, iters_out_dev, converged_out_dev};
    return run_kmeans(p, L.g, work_of(L, workspace_dev), o, max_iter, tol, seed, as_stream(stream));
}

extern "C" int dlpm_prd_histograms_f32(const float *x_dev, int64_t n1, const float *y_dev, int64_t n2, int64_t D, int32_t num_clusters,
                                       int32_t num_runs, const double *centres_dev, void *workspace_dev, int64_t workspace_bytes,
                                       uint8_t *labels_out_dev, int32_t *counts_out_dev, double *inertia_out_dev, dlpm_stream_t stream) {
    const char *who = "dlpm_prd_histograms_f32";
    int rc = check_shape(who, n1, n2, D, num_clusters, num_runs, 1);
    if (rc != DLPM_OK) return rc;
    DLPM_CHECK_ARG(x_dev && y_dev && centres_dev && workspace_dev && labels_out_dev && counts_out_dev && inertia_out_dev,
                   "%s: null pointer", who);
    const Layout L = layout_of(n1 + n2, D, num_clusters, num_runs, 1);
    rc = check_workspace(who, workspace_dev, workspace_bytes, L.total);
    if (rc != DLPM_OK) return rc;
    hipStream_t st = as_stream(stream);
    const Pts p{x_dev, y_dev, n1, n1 + n2, D};
    const Work w = work_of(L, workspace_dev);
    const int64_t count = (int64_t)num_runs * num_clusters * D;
    k_prd_init<<<(unsigned)ceil_div(L.g.I, 256), 256, 0, st>>>(L.g.I, w.done, w.iters, w.fixed);
    DLPM_LAUNCH_CHECK();
    k_prd_copy_f64<<<(unsigned)ceil_div(count, 256), 256, 0, st>>>(centres_dev, w.centres, count);
    DLPM_LAUNCH_CHECK();
    Outs o = outs_of(L, workspace_dev, Outs{nullptr, labels_out_dev, counts_out_dev, inertia_out_dev, nullptr, nullptr});
    o.centres = nullptr;     // the caller holds them
    return finish(p, L.g, w, o, st);
}

extern "C" int dlpm_prd_curve_f64(const int32_t *counts_dev, int64_t n1, int64_t n2, int32_t num_clusters, int32_t num_runs,
                                  int32_t num_angles, double epsilon, double beta, void *workspace_dev, int64_t workspace_bytes,
                                  double *out_dev, dlpm_stream_t stream) {
    const char *who = "dlpm_prd_curve_f64";
    int rc = check_shape(who, n1, n2, 1, num_clusters, num_runs, 1);
    if (rc != DLPM_OK) return rc;
    rc = check_curve(who, num_angles, epsilon, beta);
    if (rc != DLPM_OK) return rc;
    DLPM_CHECK_ARG(counts_dev && workspace_dev && out_dev, "%s: null pointer", who);
    const int64_t need = ceil_div(num_angles, 256) * 3 * 8;
    rc = check_workspace(who, workspace_dev, workspace_bytes, need);
    if (rc != DLPM_OK) return rc;
    return run_curve(counts_dev, n1, n2, num_clusters, num_runs, num_angles, epsilon, beta, static_cast<double *>(workspace_dev), out_dev,
                     as_stream(stream));
}

extern "C" int dlpm_prd_f32(const float *x_dev, int64_t n1, const float *y_dev, int64_t n2, int64_t D, int32_t num_clusters,
                            int32_t num_runs, int32_t n_init, int32_t max_iter, double tol, uint64_t seed, int32_t num_angles,
                            double epsilon, double beta, void *workspace_dev, int64_t workspace_bytes, double *centres_out_dev,
                            uint8_t *labels_out_dev, int32_t *counts_out_dev, double *out_dev, dlpm_stream_t stream) {
    const char *who = "dlpm_prd_f32";
    int rc = check_shape(who, n1, n2, D, num_clusters, num_runs, n_init);
    if (rc != DLPM_OK) return rc;
    rc = check_curve(who, num_angles, epsilon, beta);
    if (rc != DLPM_OK) return rc;
    DLPM_CHECK_ARG(max_iter >= 1, "%s: max_iter must be at least 1, got %d", who, max_iter);
    DLPM_CHECK_ARG(tol >= 0.0, "%s: tol must not be negative, got %g", who, tol);
    DLPM_CHECK_ARG(x_dev && y_dev && workspace_dev && out_dev, "%s: null pointer", who);
    const Layout L = layout_of(n1 + n2, D, num_clusters, num_runs, n_init);
    rc = check_workspace(who, workspace_dev, workspace_bytes, L.total);
    if (rc != DLPM_OK) return rc;
    hipStream_t st = as_stream(stream);
    const Pts p{x_dev, y_dev, n1, n1 + n2, D};
    const Work w = work_of(L, workspace_dev);
    const Outs o = outs_of(L, workspace_dev, Outs{centres_out_dev, labels_out_dev, counts_out_dev, nullptr, nullptr, nullptr});
    rc = run_kmeans(p, L.g, w, o, max_iter, tol, seed, st);
    if (rc != DLPM_OK) return rc;
    return run_curve(o.counts, n1, n2, num_clusters, num_runs, num_angles, epsilon, beta, w.cmax, out_dev, st);
}
