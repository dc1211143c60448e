// mmd.hip -- the multi-bandwidth Gaussian MMD of bem/evaluate/mmd_loss.py:5-37 between two point sets, without any n x n array:
//   L2[i,j] = |p_i - p_j|^2 over the concatenation p = [x; y] (n = n1 + n2 rows), bandwidth = sum L2 / (n^2 - n),
//   K[i,j] = sum_k exp(-L2 / (bandwidth / mul^(num/2) * mul^k)),  mmd = sum XX / n1^2 + sum YY / n2^2 - 2 sum XY / (n1 n2).
// The pairs are walked in 128 x 128 tiles of the UPPER triangle (K is symmetric): a tile off the diagonal counts twice in XX and YY,
// and its x-row / y-column elements are exactly the XY quadrant; a diagonal tile takes every element once and leaves YX out.
//   * direct form (D <= 16): (a - b)^2 summed in d order on the VALU, points staged through LDS -- the reference's own formula.
//     Pass 1 sums L2 (bandwidth), pass 2 the kernels.
//   * Gram form (D > 16): the points are centred on their mean (L2 is translation invariant; |c|^2 is 4x smaller than |p|^2 on [0,1]
//     pixels), tiles of C C^T go through v_mfma_f32_32x32x2_f32 (exact fp32), L2 = |c_i|^2 + |c_j|^2 - 2 c_i.c_j clamped at 0 with
//     an exact 0 on the diagonal, the exponentials run in the tile epilogue.  The bandwidth needs no pair pass here:
//     sum_ij |p_i - p_j|^2 = 2n sum_i |p_i - m|^2 - 2 |sum_i (p_i - m)|^2, and the last term vanishes at the mean (the fp32 rounding of
//     m leaves n^2 D ulp(m)^2 / 4 of it, 1e-14 of the sum), so the row norms the Gram form needs anyway give it in O(n D).
// The form is a function of D alone.  Reductions: every workgroup adds in fp64 and writes its partial sums to the workspace, one
// workgroup adds them in a fixed order -- no atomics, the same bits on every call.  All row, pair and tile indices are 64-bit.
#include <algorithm>

#include "metrics_common.h"

using namespace dlpm;

namespace {

constexpr int kTile = 128;          // rows and columns of a pair tile
constexpr int kMaxKernels = 16;     // kernel_num
constexpr int kDirectMaxD = 16;     // D <= this: direct form
constexpr int64_t kMaxTilesSide = 65535;   // T (T + 1) / 2 tiles fit a 1-D grid

typedef float floatx16 __attribute__((ext_vector_type(16)));

struct Sums {
    double xx, yy, xy;
};

__device__ inline float kernel_sum(float l2, const float (&cf)[kMaxKernels], int num) {
    float k = 0.f;
#pragma unroll
    for (int q = 0; q < kMaxKernels; q++)
        if (q < num) k += expf(l2 * cf[q]);      // cf[q] = -1 / bandwidth_q
    return k;
}

__device__ inline void add_pair(Sums &s, int64_t i, int64_t j, int64_t n1, float k, bool offdiag) {
    const bool ix = i < n1, jx = j < n1;
    const double kd = (double)k;
    if (ix == jx) {
        const double w = offdiag ? kd + kd : kd;
        if (ix) s.xx += w;
        else s.yy += w;
    } else if (ix) {
        s.xy += kd;                              // (y row, x column) is the YX copy: left out
    }
}

__device__ inline void load_coef(const float *coef, int num, float (&cf)[kMaxKernels]) {
#pragma unroll
    for (int q = 0; q < kMaxKernels; q++) cf[q] = q < num ? coef[q] : 0.f;
}

__device__ inline void write_sums(Sums s, double *sh, double *partials) {
    const double xx = block_sum<256>(s.xx, sh), yy = block_sum<256>(s.yy, sh), xy = block_sum<256>(s.xy, sh);
    if (threadIdx.x == 0) {
        double *o = partials + (int64_t)blockIdx.x * 3;
        o[0] = xx;
        o[1] = yy;
        o[2] = xy;
    }
}

// Direct form, rows padded with zeros to DT >= D ((0 - 0)^2 adds an exact 0).  Thread = one row of the tile (its point in registers) x
// one half of the columns; a wave reads the same column point from LDS (broadcast).  KERN = false: pass 1, partials[b] = sum L2.
template <int DT, bool KERN>
__global__ void __launch_bounds__(256) k_mmd_direct(Pts p, int64_t T, const float *coef, int num, double *partials) {
    __shared__ float sa[kTile * DT], sb[kTile * DT];
    __shared__ double sh[256];
    int64_t ti, tj;
    tile_of(blockIdx.x, T, ti, tj);
    const int64_t i0 = ti * kTile, j0 = tj * kTile;
    for (int e = threadIdx.x; e < kTile * DT; e += 256) {
        const int r = e / DT, d = e - r * DT;
        const int64_t i = i0 + r, j = j0 + r;
        sa[e] = (i < p.n && d < p.D) ? row_ptr(p, i)[d] : 0.f;
        sb[e] = (j < p.n && d < p.D) ? row_ptr(p, j)[d] : 0.f;
    }
    __syncthreads();
    const int r = threadIdx.x & (kTile - 1), half = threadIdx.x >> 7;
    const int64_t i = i0 + r;
    const bool offdiag = ti != tj;
    float a[DT];
#pragma unroll
    for (int d = 0; d < DT; d++) a[d] = sa[r * DT + d];
    float cf[kMaxKernels];
    if (KERN) load_coef(coef, num, cf);
    Sums s{0.0, 0.0, 0.0};
    double l2sum = 0.0;
    if (i < p.n) {
        const int cols = p.n - j0 < kTile ? (int)(p.n - j0) : kTile;
        const int c1 = min(half * 64 + 64, cols);
        for (int c = half * 64; c < c1; c++) {
            float l2 = 0.f;
#pragma unroll
            for (int d = 0; d < DT; d++) {
                const float df = a[d] - sb[c * DT + d];
                l2 += df * df;
            }
            if (KERN) add_pair(s, i, j0 + c, p.n1, kernel_sum(l2, cf, num), offdiag);
            else l2sum += offdiag ? (double)l2 + (double)l2 : (double)l2;
        }
    }
    if (KERN) {
        write_sums(s, sh, partials);
    } else {
        const double t = block_sum<256>(l2sum, sh);
        if (threadIdx.x == 0) partials[blockIdx.x] = t;
    }
}

// |p_i - m|^2 of the fp32 centred row (the very values the Gram tiles multiply), one workgroup per row
__global__ void __launch_bounds__(256) k_mmd_rownorm(Pts p, const float *mean, float *rn, double *rsum) {
    __shared__ double sh[256];
    const int64_t i = blockIdx.x;
    const float *row = row_ptr(p, i);
    double acc = 0.0;
    for (int64_t d = threadIdx.x; d < p.D; d += 256) {
        const float c = __fsub_rn(row[d], mean[d]);
        acc += (double)c * (double)c;
    }
    const double t = block_sum<256>(acc, sh);
    if (threadIdx.x == 0) {
        rn[i] = (float)t;
        rsum[i] = t;
    }
}

// bandwidth = fix_sigma, or scale * sum(vals) (fixed order); the ladder as coef[q] = -1 / (bandwidth / mul^(num/2) * mul^q)
__global__ void __launch_bounds__(1024) k_mmd_bandwidth(const double *vals, int64_t count, double scale, double fix_sigma, double mul,
                                                        int num, float *coef, double *out) {
    __shared__ double sh[1024];
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < count; i += 1024) acc += vals[i];
    const double sum = block_sum<1024>(acc, sh);
    if (threadIdx.x == 0) {
        const double bw = fix_sigma > 0.0 ? fix_sigma : sum * scale;
        out[1] = bw;
        double div = 1.0;
        for (int q = 0; q < num / 2; q++) div *= mul;
        const double b0 = bw / div;
        double m = 1.0;
        for (int q = 0; q < num; q++) {
            coef[q] = (float)(-1.0 / (b0 * m));      // bandwidth 0 (all points equal): -inf, and 0 * -inf = NaN as the reference's 0 / 0
            m *= mul;
        }
    }
}

__global__ void __launch_bounds__(1024) k_mmd_final(const double *partials, int64_t blocks, int64_t n1, int64_t n2, double *out) {
    __shared__ double sh[1024];
    double xx = 0.0, yy = 0.0, xy = 0.0;
    for (int64_t b = threadIdx.x; b < blocks; b += 1024) {
        xx += partials[b * 3];
        yy += partials[b * 3 + 1];
        xy += partials[b * 3 + 2];
    }
    xx = block_sum<1024>(xx, sh);
    yy = block_sum<1024>(yy, sh);
    xy = block_sum<1024>(xy, sh);
    if (threadIdx.x == 0) {
        const double a = (double)n1, b = (double)n2;
        out[2] = xx;
        out[3] = yy;
        out[4] = xy;
        out[0] = xx / (a * a) + yy / (b * b) - 2.0 * xy / (a * b);
    }
}

// Gram form: one 128 x 128 tile of C C^T per workgroup, 4 waves as 2 x 2, each 64 x 64 = 2 x 2 MFMA 32x32 accumulators; K in steps
// of 16 through a double-buffered LDS image (rows padded to 20 floats), staged as in conv_igemm.hip: thread = (row, 8-float half of
// the step), centred while staged; rows past n and columns past D are staged as zeros.  VEC: D % 4 == 0 and 16-byte aligned rows.
template <bool VEC>
__global__ void __launch_bounds__(256) k_mmd_gram(Pts p, int64_t T, const float *mean, const float *rn, const float *coef, int num,
                                                  double *partials) {
    constexpr int KC = 16, LD = KC + 4, BUF = 2 * kTile * LD;
    __shared__ __attribute__((aligned(16))) float smem[2 * BUF];
    __shared__ double sh[256];
    int64_t ti, tj;
    tile_of(blockIdx.x, T, ti, tj);
    const int64_t i0 = ti * kTile, j0 = tj * kTile;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1, l31 = lane & 31, kh = lane >> 5;
    const int sr = tid >> 1, sk = (tid & 1) * 8;
    const bool a_ok = i0 + sr < p.n, b_ok = j0 + sr < p.n;
    const float *pa = row_ptr(p, a_ok ? i0 + sr : 0), *pb = row_ptr(p, b_ok ? j0 + sr : 0);
    float va[8], vb[8];

    auto load_step = [&](int64_t s) {
        const int64_t k = s * KC + sk;
        if (VEC) {
#pragma unroll
            for (int v = 0; v < 2; v++) {
                const int64_t kk = k + 4 * v;
                float4 m = make_float4(0.f, 0.f, 0.f, 0.f), xa = m, xb = m;
                if (kk < p.D) {
                    m = *reinterpret_cast<const float4 *>(mean + kk);
                    xa = a_ok ? *reinterpret_cast<const float4 *>(pa + kk) : m;
                    xb = b_ok ? *reinterpret_cast<const float4 *>(pb + kk) : m;
                }
                va[4 * v] = __fsub_rn(xa.x, m.x);
                va[4 * v + 1] = __fsub_rn(xa.y, m.y);
                va[4 * v + 2] = __fsub_rn(xa.z, m.z);
                va[4 * v + 3] = __fsub_rn(xa.w, m.w);
                vb[4 * v] = __fsub_rn(xb.x, m.x);
                vb[4 * v + 1] = __fsub_rn(xb.y, m.y);
                vb[4 * v + 2] = __fsub_rn(xb.z, m.z);
                vb[4 * v + 3] = __fsub_rn(xb.w, m.w);
            }
        } else {
#pragma unroll
            for (int e = 0; e < 8; e++) {
                const int64_t kk = k + e;
                const bool ok = kk < p.D;
                const float m = ok ? mean[kk] : 0.f;
                va[e] = (ok && a_ok) ? __fsub_rn(pa[kk], m) : 0.f;
                vb[e] = (ok && b_ok) ? __fsub_rn(pb[kk], m) : 0.f;
            }
        }
    };
    auto store_step = [&](int buf) {
        float *As = smem + buf * BUF, *Bs = As + kTile * LD;
        float4 *da = reinterpret_cast<float4 *>(As + sr * LD + sk), *db = reinterpret_cast<float4 *>(Bs + sr * LD + sk);
        da[0] = make_float4(va[0], va[1], va[2], va[3]);
        da[1] = make_float4(va[4], va[5], va[6], va[7]);
        db[0] = make_float4(vb[0], vb[1], vb[2], vb[3]);
        db[1] = make_float4(vb[4], vb[5], vb[6], vb[7]);
    };

    floatx16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[i][j][r] = 0.f;

    const int64_t nsteps = (p.D + KC - 1) / KC;
    load_step(0);
    store_step(0);
    __syncthreads();
    for (int64_t s = 0; s < nsteps; s++) {
        const int buf = (int)(s & 1);
        if (s + 1 < nsteps) load_step(s + 1);            // global loads in flight under the MFMAs
        const float *As = smem + buf * BUF, *Bs = As + kTile * LD;
        const float *ap = As + (wm * 64 + l31) * LD + kh * 4, *bp = Bs + (wn * 64 + l31) * LD + kh * 4;
#pragma unroll
        for (int kk = 0; kk < KC / 8; kk++) {
            float4 af[2], bf[2];
#pragma unroll
            for (int i = 0; i < 2; i++) af[i] = *reinterpret_cast<const float4 *>(ap + i * 32 * LD + kk * 8);
#pragma unroll
            for (int j = 0; j < 2; j++) bf[j] = *reinterpret_cast<const float4 *>(bp + j * 32 * LD + kk * 8);
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int j = 0; j < 2; j++) {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].x, bf[j].x, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].y, bf[j].y, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].z, bf[j].z, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].w, bf[j].w, acc[i][j], 0, 0, 0);
                }
        }
        if (s + 1 < nsteps) store_step(buf ^ 1);         // buf ^ 1 was last read in step s - 1 (barrier since)
        __syncthreads();
    }

    // ---- epilogue: the row norms of both tile sides through LDS, then L2 -> kernels -> quadrant sums.
    //      C/D layout of the 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    float *srn = smem;
    {
        const int64_t g = (tid < kTile ? i0 : j0 - kTile) + tid;
        srn[tid] = g < p.n ? rn[g] : 0.f;
    }
    __syncthreads();
    float cf[kMaxKernels];
    load_coef(coef, num, cf);
    const bool offdiag = ti != tj;
    Sums sums{0.0, 0.0, 0.0};
#pragma unroll
    for (int jj = 0; jj < 2; jj++) {
        const int cj = (wn * 2 + jj) * 32 + l31;
        const int64_t j = j0 + cj;
        if (j >= p.n) continue;
        const float rj = srn[kTile + cj];
#pragma unroll
        for (int ii = 0; ii < 2; ii++) {
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int ci = (wm * 2 + ii) * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
                const int64_t i = i0 + ci;
                if (i >= p.n) continue;
                const float g = acc[ii][jj][r];
                float l2 = fmaxf((srn[ci] + rj) - (g + g), 0.f);
                if (i == j) l2 = 0.f;
                add_pair(sums, i, j, p.n1, kernel_sum(l2, cf, num), offdiag);
            }
        }
    }
    write_sums(sums, sh, partials);
}

struct Layout {
    int64_t T, tiles;
    int64_t coef, partials, mean, colpart, rn, rsum, total;   // byte offsets
    bool gram;
};

Layout layout_of(int64_t n, int64_t D) {
    Layout L{};
    L.T = ceil_div(n, kTile);
    L.tiles = L.T * (L.T + 1) / 2;
    L.gram = D > kDirectMaxD;
    Carve c;
    L.coef = c.take(kMaxKernels * (int64_t)sizeof(float));
    L.partials = c.take(L.tiles * 3 * (int64_t)sizeof(double));
    if (L.gram) {
        L.mean = c.take(D * (int64_t)sizeof(float));
        L.colpart = c.take(D * kColChunks * (int64_t)sizeof(double));
        L.rn = c.take(n * (int64_t)sizeof(float));
        L.rsum = c.take(n * (int64_t)sizeof(double));
    }
    L.total = c.total;
    return L;
}

int check_shape(const char *who, int64_t n1, int64_t n2, int64_t D) {
    DLPM_CHECK_ARG(n1 >= 1 && n2 >= 1 && D >= 1, "%s: bad shape n1=%lld n2=%lld D=%lld", who, (long long)n1, (long long)n2, (long long)D);
    DLPM_CHECK_ARG(n1 <= kMaxTilesSide * kTile && n2 <= kMaxTilesSide * kTile && D < (1ll << 31), "%s: shape out of range", who);
    if (ceil_div(n1 + n2, kTile) > kMaxTilesSide) {
        set_error("%s: more than %lld points in all", who, (long long)(kMaxTilesSide * kTile));
        return DLPM_ERR_UNSUPPORTED;
    }
    return DLPM_OK;
}

void launch_direct(bool kern, const Pts &p, const Layout &L, const float *coef, int num, double *partials, hipStream_t st) {
    with_dt(p.D, [&](auto dt) {
        constexpr int DT = decltype(dt)::value;
        if (kern) k_mmd_direct<DT, true><<<(unsigned)L.tiles, 256, 0, st>>>(p, L.T, coef, num, partials);
        else k_mmd_direct<DT, false><<<(unsigned)L.tiles, 256, 0, st>>>(p, L.T, coef, num, partials);
    });
}

}  // namespace

extern "C" int64_t dlpm_mmd_workspace_bytes(int64_t n1, int64_t n2, int64_t D) {
    const int rc = check_shape("dlpm_mmd_workspace_bytes", n1, n2, D);
    if (rc != DLPM_OK) return rc;
    return layout_of(n1 + n2, D).total;
}

extern "C" int dlpm_mmd_f32(const float *x_dev, int64_t n1, const float *y_dev, int64_t n2, int64_t D, double kernel_mul,
                            int32_t kernel_num, double fix_sigma, void *workspace_dev, int64_t workspace_bytes, double *out_dev,
                            dlpm_stream_t stream) {
    const int rc = check_shape("dlpm_mmd_f32", n1, n2, D);
    if (rc != DLPM_OK) return rc;
    DLPM_CHECK_ARG(kernel_num >= 1 && kernel_num <= kMaxKernels, "dlpm_mmd_f32: kernel_num must be in [1, %d], got %d", kMaxKernels,
                   kernel_num);
    DLPM_CHECK_ARG(kernel_mul > 0.0, "dlpm_mmd_f32: kernel_mul must be positive, got %g", kernel_mul);
    DLPM_CHECK_ARG(x_dev && y_dev && workspace_dev && out_dev, "dlpm_mmd_f32: null pointer");
    DLPM_CHECK_ARG(aligned(workspace_dev, 16) && aligned(out_dev, 8), "dlpm_mmd_f32: misaligned workspace or output");
    const int64_t n = n1 + n2;
    const Layout L = layout_of(n, D);
    const int ws_rc = check_workspace("dlpm_mmd_f32", workspace_dev, workspace_bytes, L.total);
    if (ws_rc != DLPM_OK) return ws_rc;
    hipStream_t st = as_stream(stream);
    char *ws = static_cast<char *>(workspace_dev);
    float *coef = reinterpret_cast<float *>(ws + L.coef);
    double *partials = reinterpret_cast<double *>(ws + L.partials);
    const Pts p{x_dev, y_dev, n1, n, D};
    const double pairs = (double)n * (double)n - (double)n;
    const bool from_data = !(fix_sigma > 0.0);
    if (!L.gram) {
        if (from_data) {
            ProfScope ps("mmd_direct_l2", 1.5 * (double)n * n * D, 4.0 * (double)n * D, st);
            launch_direct(false, p, L, coef, kernel_num, partials, st);
            DLPM_LAUNCH_CHECK();
        }
        k_mmd_bandwidth<<<1, 1024, 0, st>>>(partials, from_data ? L.tiles : 0, 1.0 / pairs, fix_sigma, kernel_mul, kernel_num, coef, out_dev);
        DLPM_LAUNCH_CHECK();
        {
            ProfScope ps("mmd_direct_kernels", 1.5 * (double)n * n * D, 4.0 * (double)n * D, st);
            launch_direct(true, p, L, coef, kernel_num, partials, st);
            DLPM_LAUNCH_CHECK();
        }
    } else {
        float *mean = reinterpret_cast<float *>(ws + L.mean), *rn = reinterpret_cast<float *>(ws + L.rn);
        double *colpart = reinterpret_cast<double *>(ws + L.colpart), *rsum = reinterpret_cast<double *>(ws + L.rsum);
        {
            ProfScope ps("mmd_centre", 3.0 * (double)n * D, 8.0 * (double)n * D, st);
            k_colstats<false><<<dim3((unsigned)ceil_div(D, 256), kColChunks), 256, 0, st>>>(p, colpart);
            DLPM_LAUNCH_CHECK();
            k_colmean<float><<<(unsigned)ceil_div(D, 256), 256, 0, st>>>(colpart, n, D, mean);
            DLPM_LAUNCH_CHECK();
            k_mmd_rownorm<<<(unsigned)n, 256, 0, st>>>(p, mean, rn, rsum);
            DLPM_LAUNCH_CHECK();
        }
        k_mmd_bandwidth<<<1, 1024, 0, st>>>(rsum, from_data ? n : 0, 2.0 * (double)n / pairs, fix_sigma, kernel_mul, kernel_num, coef, out_dev);
        DLPM_LAUNCH_CHECK();
        {
            // the upper triangle with its diagonal tiles: T (T + 1) / 2 tiles of 128 x 128 x D multiply-adds
            ProfScope ps("mmd_gram", 2.0 * (double)L.tiles * kTile * kTile * D, 8.0 * (double)L.tiles * kTile * D, st);
            if (D % 4 == 0 && aligned(x_dev, 16) && aligned(y_dev, 16))
                k_mmd_gram<true><<<(unsigned)L.tiles, 256, 0, st>>>(p, L.T, mean, rn, coef, kernel_num, partials);
            else
                k_mmd_gram<false><<<(unsigned)L.tiles, 256, 0, st>>>(p, L.T, mean, rn, coef, kernel_num, partials);
            DLPM_LAUNCH_CHECK();
        }
    }
    k_mmd_final<<<1, 1024, 0, st>>>(partials, L.tiles, n1, n2, out_dev);
    DLPM_LAUNCH_CHECK();
    return DLPM_OK;
}
