// prdc.hip -- precision / recall / density / coverage of the `prdc` package (compute_prdc, called at bem/evaluate/fid_score.py:303-336)
// between real rows R [n1, D] and fake rows G [n2, D] by k-nearest-neighbour geometry, without any n x n array:
//   r_i = the (k+1)-th smallest of {d(R_i, R_l) : all l} (l = i included, with multiplicity), g_j the same within G,
//   precision = #{j : some i has d(R_i, G_j) < r_i} / n2      recall   = #{i : some j has d(R_i, G_j) < g_j} / n1
//   density   = #{(i, j) : d(R_i, G_j) < r_i} / (k n2)        coverage = #{i : min_j d(R_i, G_j) < r_i} / n1      (all strict)
// Every comparison is made on SQUARED distances in fp64.  Two forms, chosen by D alone as in mmd.hip:
//   * direct form (D <= 16): sum (a - b)^2 in d order on the VALU in fp64 -- exact on integer-valued inputs, so duplicates and ties
//     follow the definition exactly;
//   * Gram form (D > 16): rows centred on the pooled mean of both sets (fp64 subtraction from the fp32 inputs), 128 x 128 tiles of
//     C C^T on v_mfma_f64_16x16x4_f64 with one K order per pair, d^2 = |c_i|^2 + |c_j|^2 - 2 c_i.c_j clamped at 0, the diagonal of
//     the two within-set passes an exact 0.  Ties here are those of fp64 rounding, not of exact arithmetic.
// Radii passes (R x R, G x G): a workgroup owns 128 rows and walks one SEGMENT of the column tiles; each of its 256 threads (a row and
// one half of every tile's columns) keeps the k+1 smallest squared distances it has met in LDS -- a candidate enters only when it is
// below the list's largest -- and writes them to the workspace; k_prdc_select takes the (k+1)-th smallest of a row's
// segments x 2 x (k+1) survivors.  An order statistic of a multiset does not depend on the arrival order: the same bits on every call.
// Cross pass (R x G): one walk, one tile per workgroup; per fake column the inside count, per real row "inside some fake ball" and the
// minimum squared distance, reduced in the tile and combined across tiles with integer atomics only (atomicAdd / atomicOr on int,
// atomicMin on the bit pattern of the non-negative double).  k_prdc_final turns them into the four counts and the six figures.
// All row and tile indices are 64-bit; rows past n and columns past D are staged as zeros and masked out of every selection and count.
#include <algorithm>
#include <cmath>

#include "metrics_common.h"
#include "mfma64_tile.h"

using namespace dlpm;

namespace {

constexpr int kDirectMaxD = 16;         // D <= this: direct form
constexpr int kMaxK = 32;               // nearest_k
constexpr int64_t kMaxRows = 1ll << 22; // per set: T1 * T2 cross tiles fit a 1-D grid
constexpr int64_t kTargetBlocks = 512;  // workgroups of a radii pass the segment rule aims at (two per CU)

typedef unsigned long long u64;

struct Set {
    const float *p;
    int64_t n;
};

// The segment rule, a function of n alone: T = ceil(n / 128) column tiles are cut into `count` segments of `per` tiles (the last one
// may be shorter), count = ceil(T / per) with per = ceil(T / min(T, ceil(512 / T))): T x count workgroups, about 512 from n = 2900 to
// n = 65536 (T = 79, n = 10^4: 7 segments of 12 tiles, 553 workgroups), one segment per row block beyond.
struct Segments {
    int64_t per, count;
};

__host__ __device__ inline Segments segments_of(int64_t n) {
    const int64_t T = (n + kTile - 1) / kTile;
    const int64_t cap = (kTargetBlocks + T - 1) / T;
    const int64_t want = T < cap ? T : cap;
    const int64_t per = (T + want - 1) / want;
    return Segments{per, (T + per - 1) / per};
}

// what a tile kernel walks: rows of a against rows of b
struct Walk {
    Set a, b;
    int64_t D;
    int within;                          // a and b are the same set: the diagonal is an exact 0 (Gram form)
    const double *mean, *rna, *rnb;      // Gram form: the pooled mean [D], |c|^2 of the rows of a and of b
    // radii pass
    int64_t per, nseg;
    int K1;                              // k + 1
    double *surv;                        // [nseg * 2 * K1][a.n]
    // cross pass
    int64_t tcols;                       // column tiles
    const double *r2a, *r2b;             // squared radii of the rows of a (real) and of b (fake)
    int *colcnt, *rowflag;
    u64 *rowmin;
};

// The K1 smallest values met so far, unordered, element q at lst[q * stride]; mx = the largest of them at slot mp.  It starts as K1
// times +inf, so there is no warm-up case; an equal value does not enter (the order statistic is the same either way).
struct Top {
    double mx;
    int mp;
};

__device__ inline void top_init(double *lst, int K1, int stride, Top &t) {
    for (int q = 0; q < K1; q++) lst[q * stride] = INFINITY;
    t.mx = INFINITY;
    t.mp = 0;
}

__device__ inline void top_offer(double *lst, int K1, int stride, Top &t, double v) {
    if (!(v < t.mx)) return;
    lst[t.mp * stride] = v;
    double mx = lst[0];
    int mp = 0;
    for (int q = 1; q < K1; q++) {
        const double w = lst[q * stride];
        if (w > mx) {
            mx = w;
            mp = q;
        }
    }
    t.mx = mx;
    t.mp = mp;
}

__device__ inline void write_survivors(const Walk &w, const double *lst, int64_t seg, int half, int64_t i) {
    if (i >= w.a.n) return;
    const int64_t slot0 = (seg * 2 + half) * w.K1;
    for (int q = 0; q < w.K1; q++) w.surv[(slot0 + q) * w.a.n + i] = lst[q * kThreads];
}

// which tile(s) a workgroup walks: the cross pass one (ti, tj) per workgroup, a radii pass row block ti and the tiles of segment seg
__device__ inline void tiles_of(const Walk &w, bool cross, int64_t &ti, int64_t &seg, int64_t &t0, int64_t &t1) {
    const int64_t b = blockIdx.x;
    if (cross) {
        ti = b / w.tcols;
        seg = 0;
        t0 = b - ti * w.tcols;
        t1 = t0 + 1;
    } else {
        const int64_t T = (w.b.n + kTile - 1) / kTile;
        ti = b / w.nseg;
        seg = b - ti * w.nseg;
        t0 = seg * w.per;
        t1 = t0 + w.per < T ? t0 + w.per : T;
    }
}

// the cross pass's tile results in LDS: per column the inside count, per row the recall flag and the minimum (as bits)
struct CrossLds {
    double r2[kTile], g2[kTile];
    int cnt[kTile], flag[kTile];
    u64 mn[kTile];
};

__device__ inline void cross_begin(const Walk &w, CrossLds &s, int64_t i0, int64_t j0) {
    const int t = threadIdx.x;
    if (t < kTile) {
        s.r2[t] = i0 + t < w.a.n ? w.r2a[i0 + t] : 0.0;
        s.g2[t] = j0 + t < w.b.n ? w.r2b[j0 + t] : 0.0;
        s.cnt[t] = 0;
        s.flag[t] = 0;
        s.mn[t] = (u64)__double_as_longlong(INFINITY);
    }
}

// after a barrier: one integer atomic per column / row that has something to say
__device__ inline void cross_publish(const Walk &w, const CrossLds &s, int64_t i0, int64_t j0) {
    const int t = threadIdx.x;
    if (t >= kTile) return;
    const int64_t i = i0 + t, j = j0 + t;
    if (j < w.b.n && s.cnt[t] > 0) atomicAdd(w.colcnt + j, s.cnt[t]);
    if (i < w.a.n) {
        if (s.flag[t]) atomicOr(w.rowflag + i, 1);
        if (s.mn[t] < w.rowmin[i]) atomicMin(w.rowmin + i, s.mn[t]);      // the stored minimum only ever falls: a stale read only costs an atomic
    }
}

// Direct form, rows padded with zeros to DT >= D.  Thread = one row of the block (its point in fp64 registers) x one half of a tile's
// columns; a wave reads the same column point from LDS (broadcast).
template <int DT, bool CROSS>
__global__ void __launch_bounds__(kThreads) k_prdc_direct(Walk w) {
    __shared__ float sb[kTile * DT];
    __shared__ CrossLds cs;
    extern __shared__ double lists[];
    int64_t ti, seg, t0, t1;
    tiles_of(w, CROSS, ti, seg, t0, t1);
    const int tid = threadIdx.x, r = tid & (kTile - 1), half = tid >> 7;
    const int64_t i0 = ti * kTile, i = i0 + r;
    double a[DT];
#pragma unroll
    for (int d = 0; d < DT; d++) a[d] = (i < w.a.n && d < w.D) ? (double)w.a.p[i * w.D + d] : 0.0;
    Top top;
    double *lst = lists + tid;
    if (!CROSS) top_init(lst, w.K1, kThreads, top);
    for (int64_t tj = t0; tj < t1; tj++) {
        const int64_t j0 = tj * kTile;
        __syncthreads();
        for (int e = tid; e < kTile * DT; e += kThreads) {
            const int rr = e / DT, d = e - rr * DT;
            const int64_t j = j0 + rr;
            sb[e] = (j < w.b.n && d < w.D) ? w.b.p[j * w.D + d] : 0.f;
        }
        if (CROSS) cross_begin(w, cs, i0, j0);
        __syncthreads();
        const int cols = w.b.n - j0 < kTile ? (int)(w.b.n - j0) : kTile;
        const int c1 = min(half * 64 + 64, cols);
        if (i < w.a.n) {
            const double r2i = CROSS ? cs.r2[r] : 0.0;
            double mn = INFINITY;
            int flag = 0;
            for (int c = half * 64; c < c1; c++) {
                double d2 = 0.0;
#pragma unroll
                for (int d = 0; d < DT; d++) {
                    const double df = a[d] - (double)sb[c * DT + d];
                    d2 += df * df;
                }
                if (CROSS) {
                    if (d2 < r2i) atomicAdd(&cs.cnt[c], 1);
                    if (d2 < cs.g2[c]) flag = 1;
                    mn = fmin(mn, d2);
                } else {
                    top_offer(lst, w.K1, kThreads, top, d2);
                }
            }
            if (CROSS) {
                if (flag) cs.flag[r] = 1;
                if (mn < INFINITY) atomicMin(&cs.mn[r], (u64)__double_as_longlong(mn));
            }
        }
        if (CROSS) {
            __syncthreads();
            cross_publish(w, cs, i0, j0);
        }
    }
    if (!CROSS) write_survivors(w, lst, seg, half, i);
}

// |p_i - m|^2 of the fp64 centred row (the very values the Gram tiles multiply), one workgroup per row of the concatenation
__global__ void __launch_bounds__(256) k_prdc_rownorm(Pts p, const double *mean, double *rn) {
    __shared__ double sh[256];
    const int64_t i = blockIdx.x;
    const float *row = row_ptr(p, i);
    double acc = 0.0;
    for (int64_t d = threadIdx.x; d < p.D; d += 256) {
        const double c = (double)row[d] - mean[d];
        acc += c * c;
    }
    const double t = block_sum<256>(acc, sh);
    if (threadIdx.x == 0) rn[i] = t;
}

// Gram form: 128 x 128 tiles of C C^T on the tile loop of mfma64_tile.h; thread = (row, 8-value half of the step), centred in fp64
// while staged.
template <bool CROSS>
__global__ void __launch_bounds__(kThreads) k_prdc_gram(Walk w) {
    constexpr int SLAB = 32, SLD = SLAB + 1;
    static_assert(kTile * SLD <= kImage, "the distance slab lives in the staging image");
    __shared__ double smem[kImage];
    __shared__ double s_rna[kTile], s_rnb[kTile];
    __shared__ CrossLds cs;
    extern __shared__ double lists[];
    int64_t ti, seg, t0, t1;
    tiles_of(w, CROSS, ti, seg, t0, t1);
    const int tid = threadIdx.x, sr = tid >> 1, sk = (tid & 1) * 8;
    const Lanes l = lanes_of(tid);
    const int64_t i0 = ti * kTile;
    const bool a_ok = i0 + sr < w.a.n;
    const float *pa = w.a.p + (a_ok ? i0 + sr : 0) * w.D;
    Top top;
    double *lst = lists + tid;
    if (!CROSS) top_init(lst, w.K1, kThreads, top);

    for (int64_t tj = t0; tj < t1; tj++) {
        const int64_t j0 = tj * kTile;
        const bool b_ok = j0 + sr < w.b.n;
        const float *pb = w.b.p + (b_ok ? j0 + sr : 0) * w.D;
        double va[8], vb[8];
        auto load = [&](int64_t s) {
#pragma unroll
            for (int e = 0; e < 8; e++) {
                const int64_t k = s * kKC + sk + e;
                const bool ok = k < w.D;
                const double m = ok ? w.mean[k] : 0.0;
                va[e] = (ok && a_ok) ? (double)pa[k] - m : 0.0;
                vb[e] = (ok && b_ok) ? (double)pb[k] - m : 0.0;
            }
        };
        __syncthreads();                                   // the previous tile's epilogue has read the slab and the norms
        if (tid < kTile) s_rna[tid] = i0 + tid < w.a.n ? w.rna[i0 + tid] : 0.0;
        else s_rnb[tid - kTile] = j0 + tid - kTile < w.b.n ? w.rnb[j0 + tid - kTile] : 0.0;
        if (CROSS) cross_begin(w, cs, i0, j0);

        Acc acc;
        acc_zero(acc);
        tile_loop(smem, w.D, l, acc, load, [&]() { store_rows(smem, sr, sk, va, vb); });

        // ---- epilogue
        if (CROSS) {
            double rmin[4][4];
#pragma unroll
            for (int bi = 0; bi < 4; bi++)
#pragma unroll
                for (int reg = 0; reg < 4; reg++) rmin[bi][reg] = INFINITY;
#pragma unroll
            for (int bj = 0; bj < 4; bj++) {
                const int cl = tile_col(l, bj);
                if (j0 + cl >= w.b.n) continue;
                const double rj = s_rnb[cl], g2c = cs.g2[cl];
                int cnt = 0;
#pragma unroll
                for (int bi = 0; bi < 4; bi++)
#pragma unroll
                    for (int reg = 0; reg < 4; reg++) {
                        const int rl = tile_row(l, bi, reg);
                        if (i0 + rl >= w.a.n) continue;
                        const double g = acc[bi][bj][reg];
                        const double d2 = fmax((s_rna[rl] + rj) - (g + g), 0.0);
                        if (d2 < cs.r2[rl]) cnt++;
                        if (d2 < g2c) cs.flag[rl] = 1;
                        rmin[bi][reg] = fmin(rmin[bi][reg], d2);
                    }
                if (cnt) atomicAdd(&cs.cnt[cl], cnt);
            }
#pragma unroll
            for (int bi = 0; bi < 4; bi++)
#pragma unroll
                for (int reg = 0; reg < 4; reg++)
                    if (rmin[bi][reg] < INFINITY)
                        atomicMin(&cs.mn[tile_row(l, bi, reg)], (u64)__double_as_longlong(rmin[bi][reg]));
            __syncthreads();
            cross_publish(w, cs, i0, j0);
        } else {
            // the tile's squared distances go through LDS in four slabs of 32 columns (a column past n as +inf), where the thread that
            // owns (row, half) offers its 16 of them to its list
            double *slab = smem;
            const int r = tid & (kTile - 1), half = tid >> 7;
#pragma unroll
            for (int sbi = 0; sbi < 4; sbi++) {
                if (l.wn == (sbi >> 1)) {
#pragma unroll
                    for (int jj = 0; jj < 2; jj++) {
                        const int bj = 2 * (sbi & 1) + jj;
                        const int cl = tile_col(l, bj);
                        const int64_t j = j0 + cl;
                        const double rj = s_rnb[cl];
#pragma unroll
                        for (int bi = 0; bi < 4; bi++)
#pragma unroll
                            for (int reg = 0; reg < 4; reg++) {
                                const int rl = tile_row(l, bi, reg);
                                const double g = acc[bi][bj][reg];
                                double d2 = fmax((s_rna[rl] + rj) - (g + g), 0.0);
                                if (w.within && i0 + rl == j) d2 = 0.0;
                                if (j >= w.b.n) d2 = INFINITY;
                                slab[rl * SLD + jj * 16 + l.l15] = d2;
                            }
                    }
                }
                __syncthreads();
                if (i0 + r < w.a.n) {
#pragma unroll 4
                    for (int c = 0; c < 16; c++) top_offer(lst, w.K1, kThreads, top, slab[r * SLD + half * 16 + c]);
                }
                __syncthreads();
            }
        }
    }
    if (!CROSS) write_survivors(w, lst, seg, tid >> 7, i0 + (tid & (kTile - 1)));
}

// the (k+1)-th smallest of a row's `slots` survivors: r2[i], and its square root to radii_out (nullable).  Thread = row.
__global__ void __launch_bounds__(128) k_prdc_select(const double *surv, int64_t n, int64_t slots, int K1, double *r2, double *radii_out) {
    __shared__ double lists[(kMaxK + 1) * 128];
    const int64_t i = (int64_t)blockIdx.x * 128 + threadIdx.x;
    if (i >= n) return;
    double *lst = lists + threadIdx.x;
    Top top;
    top_init(lst, K1, 128, top);
    for (int64_t s = 0; s < slots; s++) top_offer(lst, K1, 128, top, surv[s * n + i]);
    r2[i] = top.mx;
    if (radii_out) radii_out[i] = sqrt(top.mx);
}

// header of the workspace
struct Header {
    int nonfinite;
};

__global__ void __launch_bounds__(256) k_prdc_init(Header *h, int *colcnt, int64_t n2, int *rowflag, u64 *rowmin, int64_t n1) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t == 0) h->nonfinite = 0;
    if (t < n2) colcnt[t] = 0;
    if (t < n1) {
        rowflag[t] = 0;
        rowmin[t] = (u64)__double_as_longlong(INFINITY);
    }
}

template <int THREADS>
__device__ inline long long block_sum_i64(long long v, long long *sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int s = THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    const long long out = sh[0];
    __syncthreads();
    return out;
}

__device__ inline double f_1(double a, double b) { return a + b > 0.0 ? 2.0 * a * b / (a + b) : 0.0; }

__global__ void __launch_bounds__(1024) k_prdc_final(const Header *h, const int *colcnt, const int *rowflag, const u64 *rowmin,
                                                     const double *r2a, int64_t n1, int64_t n2, int k, int64_t *counts, double *out) {
    __shared__ long long sh[1024];
    long long ph = 0, rh = 0, dp = 0, ch = 0;
    for (int64_t j = threadIdx.x; j < n2; j += 1024) {
        const int c = colcnt[j];
        ph += c > 0;
        dp += c;
    }
    for (int64_t i = threadIdx.x; i < n1; i += 1024) {
        rh += rowflag[i] != 0;
        ch += __longlong_as_double((long long)rowmin[i]) < r2a[i];
    }
    ph = block_sum_i64<1024>(ph, sh);
    rh = block_sum_i64<1024>(rh, sh);
    dp = block_sum_i64<1024>(dp, sh);
    ch = block_sum_i64<1024>(ch, sh);
    if (threadIdx.x == 0) {
        const bool bad = h->nonfinite != 0;
        counts[0] = bad ? 0 : ph;
        counts[1] = bad ? 0 : rh;
        counts[2] = bad ? 0 : dp;
        counts[3] = bad ? 0 : ch;
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        const double P = (double)ph / (double)n2, R = (double)rh / (double)n1;
        const double Dn = (double)dp / ((double)k * (double)n2), C = (double)ch / (double)n1;
        out[0] = bad ? nan : P;
        out[1] = bad ? nan : R;
        out[2] = bad ? nan : Dn;
        out[3] = bad ? nan : C;
        out[4] = bad ? nan : f_1(P, R);
        out[5] = bad ? nan : f_1(Dn, C);
        out[6] = bad ? 1.0 : 0.0;
        out[7] = 0.0;
    }
}

struct Layout {
    Segments s1, s2;
    bool gram;
    int64_t header, mean, colpart, rn, r2a, r2b, surv, colcnt, rowflag, rowmin, total;   // byte offsets
};

Layout layout_of(int64_t n1, int64_t n2, int64_t D, int k) {
    Layout L{};
    L.s1 = segments_of(n1);
    L.s2 = segments_of(n2);
    L.gram = D > kDirectMaxD;
    const int64_t dbl = (int64_t)sizeof(double);
    Carve c;
    L.header = c.take((int64_t)sizeof(Header));
    if (L.gram) {
        L.mean = c.take(D * dbl);
        L.colpart = c.take(D * kColChunks * dbl);
        L.rn = c.take((n1 + n2) * dbl);
    }
    L.r2a = c.take(n1 * dbl);
    L.r2b = c.take(n2 * dbl);
    L.surv = c.take(std::max(n1 * L.s1.count, n2 * L.s2.count) * 2 * (k + 1) * dbl);     // the two radii passes take turns
    L.colcnt = c.take(n2 * (int64_t)sizeof(int));
    L.rowflag = c.take(n1 * (int64_t)sizeof(int));
    L.rowmin = c.take(n1 * (int64_t)sizeof(u64));
    L.total = c.total;
    return L;
}

int check_shape(const char *who, int64_t n1, int64_t n2, int64_t D, int32_t k) {
    DLPM_CHECK_ARG(n1 >= 1 && n2 >= 1 && D >= 1, "%s: bad shape n1=%lld n2=%lld D=%lld", who, (long long)n1, (long long)n2, (long long)D);
    DLPM_CHECK_ARG(n1 <= kMaxRows && n2 <= kMaxRows && D < (1ll << 31), "%s: shape out of range", who);
    DLPM_CHECK_ARG(k >= 1 && k <= kMaxK, "%s: nearest_k must be in [1, %d], got %d", who, kMaxK, k);
    DLPM_CHECK_ARG(k < std::min(n1, n2), "%s: nearest_k = %d needs more than %d points in both sets, got %lld and %lld", who, k, k,
                   (long long)n1, (long long)n2);
    return DLPM_OK;
}

template <bool CROSS>
int launch_walk(const Walk &w, bool gram, unsigned grid, hipStream_t st) {
    const size_t shmem = CROSS ? 0 : (size_t)kThreads * w.K1 * sizeof(double);
    using Kernel = void (*)(Walk);
    const Kernel fn = gram ? &k_prdc_gram<CROSS> : with_dt(w.D, [](auto dt) -> Kernel { return &k_prdc_direct<decltype(dt)::value, CROSS>; });
    if (!CROSS) {                                          // the lists of k = 32 (66 KB) beside the tile image pass 64 KB of LDS; the limit counts against 160 KB minus the static 36 KB
        const int r = ensure_dynamic_lds(reinterpret_cast<const void *>(fn), 96 * 1024);
        if (r != DLPM_OK) return r;
    }
    fn<<<grid, kThreads, shmem, st>>>(w);
    DLPM_LAUNCH_CHECK();
    return DLPM_OK;
}

}  // namespace

extern "C" int64_t dlpm_prdc_workspace_bytes(int64_t n1, int64_t n2, int64_t D, int32_t nearest_k) {
    const int rc = check_shape("dlpm_prdc_workspace_bytes", n1, n2, D, nearest_k);
    if (rc != DLPM_OK) return rc;
    return layout_of(n1, n2, D, nearest_k).total;
}

extern "C" int dlpm_prdc_f32(const float *x_dev, int64_t n1, const float *y_dev, int64_t n2, int64_t D, int32_t nearest_k,
                             void *workspace_dev, int64_t workspace_bytes, double *radii_real_out_dev, double *radii_fake_out_dev,
                             int64_t *counts_out_dev, double *out_dev, dlpm_stream_t stream) {
    const int rc = check_shape("dlpm_prdc_f32", n1, n2, D, nearest_k);
    if (rc != DLPM_OK) return rc;
    DLPM_CHECK_ARG(x_dev && y_dev && workspace_dev && counts_out_dev && out_dev, "dlpm_prdc_f32: null pointer");
    DLPM_CHECK_ARG(aligned(x_dev, 4) && aligned(y_dev, 4) && aligned(radii_real_out_dev, 8) && aligned(radii_fake_out_dev, 8) &&
                       aligned(counts_out_dev, 8) && aligned(out_dev, 8),
                   "dlpm_prdc_f32: misaligned input or output");
    const Layout L = layout_of(n1, n2, D, nearest_k);
    const int ws_rc = check_workspace("dlpm_prdc_f32", workspace_dev, workspace_bytes, L.total);
    if (ws_rc != DLPM_OK) return ws_rc;
    hipStream_t st = as_stream(stream);
    char *ws = static_cast<char *>(workspace_dev);
    Header *hdr = reinterpret_cast<Header *>(ws + L.header);
    double *mean = reinterpret_cast<double *>(ws + L.mean), *colpart = reinterpret_cast<double *>(ws + L.colpart);
    double *rn = reinterpret_cast<double *>(ws + L.rn), *r2a = reinterpret_cast<double *>(ws + L.r2a);
    double *r2b = reinterpret_cast<double *>(ws + L.r2b), *surv = reinterpret_cast<double *>(ws + L.surv);
    int *colcnt = reinterpret_cast<int *>(ws + L.colcnt), *rowflag = reinterpret_cast<int *>(ws + L.rowflag);
    u64 *rowmin = reinterpret_cast<u64 *>(ws + L.rowmin);
    const int64_t n = n1 + n2, T1 = ceil_div(n1, kTile), T2 = ceil_div(n2, kTile);
    const Pts p{x_dev, y_dev, n1, n, D};
    const int K1 = nearest_k + 1;

    k_prdc_init<<<(unsigned)ceil_div(std::max(n1, n2), 256), 256, 0, st>>>(hdr, colcnt, n2, rowflag, rowmin, n1);
    DLPM_LAUNCH_CHECK();
    k_nonfinite<256><<<scan_grid(n * D), 256, 0, st>>>(p, &hdr->nonfinite);
    DLPM_LAUNCH_CHECK();
    if (L.gram) {
        ProfScope ps("prdc_centre", 3.0 * (double)n * D, 8.0 * (double)n * D, st);
        k_colstats<false><<<dim3((unsigned)ceil_div(D, 256), kColChunks), 256, 0, st>>>(p, colpart);
        DLPM_LAUNCH_CHECK();
        k_colmean<double><<<(unsigned)ceil_div(D, 256), 256, 0, st>>>(colpart, n, D, mean);
        DLPM_LAUNCH_CHECK();
        k_prdc_rownorm<<<(unsigned)n, 256, 0, st>>>(p, mean, rn);
        DLPM_LAUNCH_CHECK();
    }
    Walk w{};
    w.D = D;
    w.mean = mean;
    w.K1 = K1;
    w.surv = surv;
    for (int pass = 0; pass < 2; pass++) {                 // the radii of R, then of G
        const Set s = pass == 0 ? Set{x_dev, n1} : Set{y_dev, n2};
        const Segments sg = pass == 0 ? L.s1 : L.s2;
        const int64_t T = pass == 0 ? T1 : T2;
        w.a = w.b = s;
        w.within = 1;
        w.rna = w.rnb = pass == 0 ? rn : rn + n1;
        w.per = sg.per;
        w.nseg = sg.count;
        {
            ProfScope ps(pass == 0 ? "prdc_radii_real" : "prdc_radii_fake", 2.0 * (double)s.n * s.n * D, 8.0 * (double)T * sg.count * kTile * D, st);
            const int r = launch_walk<false>(w, L.gram, (unsigned)(T * sg.count), st);
            if (r != DLPM_OK) return r;
        }
        k_prdc_select<<<(unsigned)ceil_div(s.n, 128), 128, 0, st>>>(surv, s.n, sg.count * 2 * K1, K1, pass == 0 ? r2a : r2b,
                                                                   pass == 0 ? radii_real_out_dev : radii_fake_out_dev);
        DLPM_LAUNCH_CHECK();
    }
    w.a = Set{x_dev, n1};
    w.b = Set{y_dev, n2};
    w.within = 0;
    w.rna = rn;
    w.rnb = rn + n1;
    w.tcols = T2;
    w.r2a = r2a;
    w.r2b = r2b;
    w.colcnt = colcnt;
    w.rowflag = rowflag;
    w.rowmin = rowmin;
    {
        ProfScope ps("prdc_cross", 2.0 * (double)n1 * n2 * D, 8.0 * (double)T1 * T2 * kTile * D, st);
        const int r = launch_walk<true>(w, L.gram, (unsigned)(T1 * T2), st);
        if (r != DLPM_OK) return r;
    }
    k_prdc_final<<<1, 1024, 0, st>>>(hdr, colcnt, rowflag, rowmin, r2a, n1, n2, nearest_k, counts_out_dev, out_dev);
    DLPM_LAUNCH_CHECK();
    return DLPM_OK;
}
