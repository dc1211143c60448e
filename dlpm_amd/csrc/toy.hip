// toy.hip -- the 2-D toy data distributions of bem/datasets/Distributions.py on the device (include/dlpm_amd_toy.h):
//   * k_toy_draw      stage A: one thread per row, every random number a function of (seed, stream, global row, element, purpose)
//   * k_toy_moments   stage B: scalar mean and standard deviation of all 2 N values, two passes, fp64, one workgroup, fixed order
//   * k_toy_normalize (x - m) / s in fp64, rounded once
//   * k_toy_select    the two order statistics of a column by an exact binary radix select on the ordered keys, one workgroup each
//   * k_toy_clamp     clamp to +-c and divide by c, as _between_minus_1_1_with_quantile
// Drawn once per evaluation: latency bound, nothing here is tuned beyond coalesced 8-byte accesses.  No atomics; vector stores only.
#include <algorithm>
#include <cmath>

#include "../../include/dlpm_amd_toy.h"
#include "cms.h"
#include "metrics_common.h"
#include "philox.h"

using namespace dlpm;

namespace {

// Philox purposes of the toy draws (1-6: the sampler, 7-10: the DLPM loss, 11-13: the LIM loss).  Counter = (global row lo, hi,
// element, purpose | stream << 8); the permutation's counter is (half, round, width, purpose | stream << 8).
constexpr uint32_t kPurposeToyU = 14;    // the component choice of a gmm row / swiss_roll's t
constexpr uint32_t kPurposeToyZ = 15;    // the two normals of a row
constexpr uint32_t kPurposeToyA = 16;    // sas_grid's heavy-tailed a (element 0: the row's, or one per element)
constexpr uint32_t kPurposeToyPi = 17;   // the round function of sas_grid's permutation

constexpr int kThreads = 1024;
constexpr int kMaxComponents = 4096;
constexpr double kPi = 3.141592653589793;

struct State {
    double m, s;
    float os[2][2];     // [column][0: high, 1: low] order statistics
    int flag[2][2];     // the reference's two asserts, per column
};

// two 53-bit uniforms in (0, 1), as cms_draw builds its own
__device__ inline void uniform53x2(uint64_t seed, uint64_t gidx, uint32_t elem, uint32_t word, double &U, double &V) {
    const uint4 r = philox4x32_10(make_uint4((uint32_t)gidx, (uint32_t)(gidx >> 32), elem, word), seed);
    U = ((double)(((uint64_t)r.x << 21) ^ (r.y >> 11)) + 0.5) * (1.0 / 9007199254740992.0);
    V = ((double)(((uint64_t)r.z << 21) ^ (r.w >> 11)) + 0.5) * (1.0 / 9007199254740992.0);
}

// two N(0, 1) by Box-Muller in fp64: the tails reach sqrt(2 * 54 ln 2) = 8.6 sigma
__device__ inline void normal2(uint64_t seed, uint64_t gidx, uint32_t word, double &z0, double &z1) {
    double U, V;
    uniform53x2(seed, gidx, 0u, word, U, V);
    const double r = sqrt(-2.0 * log(U));
    z0 = r * cos(2.0 * kPi * V);
    z1 = r * sin(2.0 * kPi * V);
}

// pi(p): 4-round balanced Feistel network on `width` bits (even, 2^width >= N), cycle-walked into [0, N).  A Feistel network is a
// bijection of [0, 2^width) whatever its round function; following the cycle of p until it re-enters [0, N) keeps it one of [0, N),
// and the walk ends because p itself lies on that cycle.  Expected length below 4 (2^width < 4 N).
__device__ inline uint64_t toy_permute(uint64_t p, uint64_t N, int width, uint64_t seed, uint32_t word) {
    const int half = width / 2;
    const uint32_t mask = (uint32_t)((1ull << half) - 1ull);
    uint64_t v = p;
    do {
        uint32_t L = (uint32_t)(v >> half) & mask, R = (uint32_t)v & mask;
        for (uint32_t round = 0; round < 4; round++) {
            const uint32_t f = philox4x32_10(make_uint4(R, round, (uint32_t)width, word), seed).x & mask;
            const uint32_t nl = R;
            R = L ^ f;
            L = nl;
        }
        v = ((uint64_t)L << half) | R;
    } while (v >= N);
    return v;
}

__global__ void __launch_bounds__(256) k_toy_draw(dlpm_toy_draw_args p, int n, int width) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.N) return;
    const uint64_t gidx = (uint64_t)(p.first_index + i);
    const uint32_t hi = p.stream << 8;
    double z0, z1;
    normal2(p.seed, gidx, kPurposeToyZ | hi, z0, z1);
    float x0, x1;
    if (p.kind == DLPM_TOY_GMM_2 || p.kind == DLPM_TOY_GMM_GRID) {
        double U, V;
        uniform53x2(p.seed, gidx, 0u, kPurposeToyU | hi, U, V);
        // the first k with U < cum[k]; cum is non-decreasing, so a bisection finds it.  None: the last component.
        int lo = 0, up = p.count - 1;
        while (lo < up) {
            const int mid = (lo + up) >> 1;
            if (U < p.cum_dev[mid]) up = mid;
            else lo = mid + 1;
        }
        const int k = lo;
        double m0, m1;
        if (p.kind == DLPM_TOY_GMM_2) {
            m0 = k == 0 ? p.theta : -p.theta;
            m1 = 0.0;
        } else {
            m0 = (double)(k / n);
            m1 = (double)(k % n);
        }
        x0 = (float)(m0 + p.std * z0);          // fp64 points, rounded once (torch.tensor(x, dtype=float32))
        x1 = (float)(m1 + p.std * z1);
    } else if (p.kind == DLPM_TOY_SWISS_ROLL) {
        double U, V;
        uniform53x2(p.seed, gidx, 0u, kPurposeToyU | hi, U, V);
        const double t = 1.5 * kPi * (1.0 + 2.0 * U);
        x0 = (float)(t * cos(t) + p.std * z0);
        x1 = (float)(t * sin(t) + p.std * z1);
    } else {
        // sample_grid_sas, operation by operation in fp32: std * (sqrt(a) * z) + (i, j) - (n / 2, n / 2)
        float a0 = 2.0f, a1 = 2.0f;
        if (p.data_alpha != 2.0) {
            const Cms c = cms_setup(p.data_alpha);
            a0 = cms_draw(c, p.seed, gidx, 0u, kPurposeToyA, p.stream);
            a1 = p.isotropic ? a0 : cms_draw(c, p.seed, gidx, 1u, kPurposeToyA, p.stream);
        }
        const float sd = (float)p.std;
        x0 = __fmul_rn(sd, __fmul_rn((float)sqrt((double)a0), (float)z0));
        x1 = __fmul_rn(sd, __fmul_rn((float)sqrt((double)a1), (float)z1));
        const uint64_t r = toy_permute((uint64_t)i, (uint64_t)p.N, width, p.seed, kPurposeToyPi | hi);
        if (p.perm_out_dev) p.perm_out_dev[i] = (int64_t)r;
        // the component whose [bounds[k], bounds[k + 1]) holds source row r (bounds is non-decreasing); none: no offset
        int k = -1;
        if ((int64_t)r < p.bounds_dev[p.count]) {
            int lo = 0, up = p.count - 1;
            while (lo < up) {
                const int mid = (lo + up) >> 1;
                if ((int64_t)r < p.bounds_dev[mid + 1]) up = mid;
                else lo = mid + 1;
            }
            k = lo;
        }
        if (k >= 0) {
            x0 = __fadd_rn(x0, (float)(k / n));
            x1 = __fadd_rn(x1, (float)(k % n));
        }
        const float centre = (float)((double)n / 2.0);
        x0 = __fsub_rn(x0, centre);
        x1 = __fsub_rn(x1, centre);
    }
    reinterpret_cast<float2 *>(p.out_dev)[i] = make_float2(x0, x1);
}

// m = sum / M and s = sqrt(sum (x - m)^2 / (M - ddof)) over the M = 2 N values: thread t owns the values t, t + 1024, ..., the
// partial sums meet in block_sum's fixed tree.  Two passes: the squares are centred, no cancellation.
__global__ void __launch_bounds__(kThreads) k_toy_moments(const float *x, int64_t M, int ddof, State *st, double *out) {
    __shared__ double sh[kThreads];
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < M; i += kThreads) acc += (double)x[i];
    const double m = block_sum<kThreads>(acc, sh) / (double)M;
    double q = 0.0;
    for (int64_t i = threadIdx.x; i < M; i += kThreads) {
        const double d = (double)x[i] - m;
        q += d * d;
    }
    const double s = sqrt(block_sum<kThreads>(q, sh) / (double)(M - ddof));
    if (threadIdx.x == 0) {
        st->m = m;
        st->s = s;
        if (out) {
            out[0] = m;
            out[1] = s;
        }
    }
}

__global__ void __launch_bounds__(256) k_toy_normalize(float *x, int64_t N, const State *st) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const double m = st->m, s = st->s;
    float2 v = reinterpret_cast<float2 *>(x)[i];
    v.x = (float)(((double)v.x - m) / s);
    v.y = (float)(((double)v.y - m) / s);
    reinterpret_cast<float2 *>(x)[i] = v;
}

// blockIdx.x = 2 * column + which (0: the high rank, 1: the low rank).  The key of the order statistic bit by bit from the top:
// among the keys that carry the prefix found so far, those with a 0 at this bit sort first; the rank says which side it is on.
// Counts are integers carried in fp64 (exact below 2^53) through block_sum.
__global__ void __launch_bounds__(kThreads) k_toy_select(const float *x, int64_t N, int64_t rank_hi, int64_t rank_lo, State *st,
                                                         double *out) {
    __shared__ double sh[kThreads];
    const int col = blockIdx.x >> 1, which = blockIdx.x & 1;
    long long rank = which == 0 ? rank_hi : rank_lo;
    unsigned int prefix = 0u;
    for (int bit = 31; bit >= 0; bit--) {
        const unsigned int keep = bit == 31 ? 0u : ~0u << (bit + 1);
        long long zeros = 0;
        for (int64_t i = threadIdx.x; i < N; i += kThreads) {
            const unsigned int k = key_of(x[2 * i + col]);
            zeros += ((k & keep) == prefix) && !((k >> bit) & 1u);
        }
        const long long total = (long long)block_sum<kThreads>((double)zeros, sh);
        if (rank >= total) {
            rank -= total;
            prefix |= 1u << bit;
        }
    }
    if (threadIdx.x == 0) {
        const float v = value_of(prefix);
        st->os[col][which] = v;
        st->flag[col][which] = which == 0 ? (v < 0.0f) : (v > 0.0f);
        if (out) out[2 + 3 * col + which] = (double)v;
    }
}

__device__ inline int toy_status(const State *st) {
    return ((st->flag[0][0] | st->flag[1][0]) ? DLPM_TOY_STATUS_HIGH_NEGATIVE : 0) |
           ((st->flag[0][1] | st->flag[1][1]) ? DLPM_TOY_STATUS_LOW_POSITIVE : 0);
}

__global__ void __launch_bounds__(256) k_toy_clamp(float *x, int64_t N, const State *st, double *out, int32_t *status) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int bad = toy_status(st);
    const float c0 = fmaxf(fabsf(st->os[0][0]), fabsf(st->os[0][1])), c1 = fmaxf(fabsf(st->os[1][0]), fabsf(st->os[1][1]));
    if (i == 0) {
        *status = bad;
        if (out) {
            out[4] = (double)c0;
            out[7] = (double)c1;
        }
    }
    if (i >= N || bad) return;
    float2 v = reinterpret_cast<float2 *>(x)[i];
    v.x = __fdiv_rn(fminf(fmaxf(v.x, -c0), c0), c0);       // torch.clamp, then tmp /= clamp_value
    v.y = __fdiv_rn(fminf(fmaxf(v.y, -c1), c1), c1);
    reinterpret_cast<float2 *>(x)[i] = v;
}

__global__ void k_toy_status_ok(int32_t *status) { *status = 0; }

// torch.quantile's rank on an fp32 tensor: q becomes an fp32 scalar, q * (N - 1) is an fp32 product, round() is half-even
int64_t nearest_rank(double q, int64_t N) { return std::min<int64_t>((int64_t)nearbyintf((float)q * (float)(N - 1)), N - 1); }

int int_sqrt(int v) {
    int n = (int)std::lround(std::sqrt((double)v));
    return n * n == v ? n : -1;
}

}  // namespace

extern "C" int dlpm_toy_draw_f32(const dlpm_toy_draw_args *a, dlpm_stream_t stream) {
    DLPM_CHECK_ARG(a, "dlpm_toy_draw_f32: null pointer");
    DLPM_CHECK_ARG(a->N > 0 && a->N < (1ll << 31), "dlpm_toy_draw_f32: N must lie in [1, 2^31), got %lld", (long long)a->N);
    DLPM_CHECK_ARG(a->kind >= DLPM_TOY_GMM_2 && a->kind <= DLPM_TOY_SAS_GRID, "dlpm_toy_draw_f32: unknown kind %d", a->kind);
    DLPM_CHECK_ARG(a->first_index >= 0, "dlpm_toy_draw_f32: first_index must not be negative, got %lld", (long long)a->first_index);
    DLPM_CHECK_ARG(a->stream < (1u << 24), "dlpm_toy_draw_f32: stream must lie below 2^24, got %u", a->stream);
    DLPM_CHECK_ARG(std::isfinite(a->std) && a->std >= 0.0, "dlpm_toy_draw_f32: std must be finite and not negative, got %g", a->std);
    DLPM_CHECK_ARG(a->out_dev, "dlpm_toy_draw_f32: null pointer");
    DLPM_CHECK_ARG(reinterpret_cast<uintptr_t>(a->out_dev) % 8 == 0 && reinterpret_cast<uintptr_t>(a->perm_out_dev) % 8 == 0 &&
                       reinterpret_cast<uintptr_t>(a->cum_dev) % 8 == 0 && reinterpret_cast<uintptr_t>(a->bounds_dev) % 8 == 0,
                   "dlpm_toy_draw_f32: misaligned pointer");
    const bool grid = a->kind == DLPM_TOY_GMM_GRID || a->kind == DLPM_TOY_SAS_GRID;
    int n = 0;
    if (grid) {
        DLPM_CHECK_ARG(a->n_mixture >= 1 && a->n_mixture <= kMaxComponents, "dlpm_toy_draw_f32: n_mixture must lie in [1, %d], got %d",
                       kMaxComponents, a->n_mixture);
        n = int_sqrt(a->n_mixture);
        DLPM_CHECK_ARG(n > 0, "dlpm_toy_draw_f32: n_mixture = %d is not a perfect square", a->n_mixture);
    }
    if (a->kind != DLPM_TOY_SWISS_ROLL) {
        const int components = grid ? n * n : 2;
        DLPM_CHECK_ARG(a->count == components, "dlpm_toy_draw_f32: %d weights for %d components", a->count, components);
        DLPM_CHECK_ARG(a->weights_host, "dlpm_toy_draw_f32: null weights");
        double sum = 0.0;
        for (int k = 0; k < a->count; k++) {
            const double w = a->weights_host[k];
            DLPM_CHECK_ARG(std::isfinite(w) && w >= 0.0, "dlpm_toy_draw_f32: weight %d is %g; weights are finite and not negative", k, w);
            sum += w;
        }
        DLPM_CHECK_ARG(sum <= 1.0 + 1e-12, "dlpm_toy_draw_f32: the weights sum to %.17g, above 1", sum);
    }
    int width = 2;
    if (a->kind == DLPM_TOY_SAS_GRID) {
        DLPM_CHECK_ARG(a->data_alpha > 0.0 && a->data_alpha <= 2.0, "Wrong value of alpha (%g) for skewed levy r.v generation", a->data_alpha);
        DLPM_CHECK_ARG(a->first_index == 0, "dlpm_toy_draw_f32: sas_grid assigns its components in exact proportions of N and is drawn "
                                            "whole: first_index must be 0, got %lld", (long long)a->first_index);
        DLPM_CHECK_ARG(a->bounds_dev, "dlpm_toy_draw_f32: null bounds");
        while ((1ll << width) < a->N) width += 2;
    } else if (a->kind != DLPM_TOY_SWISS_ROLL) {
        DLPM_CHECK_ARG(a->cum_dev, "dlpm_toy_draw_f32: null cumulative weights");
    }
    ProfScope ps("toy_draw", 0.0, 8.0 * (double)a->N, as_stream(stream));
    k_toy_draw<<<(unsigned)ceil_div(a->N, 256), 256, 0, as_stream(stream)>>>(*a, n, width);
    DLPM_LAUNCH_CHECK();
    return DLPM_OK;
}

extern "C" int64_t dlpm_toy_workspace_bytes(int64_t N) {
    DLPM_CHECK_ARG(N > 0 && N < (1ll << 31), "dlpm_toy_workspace_bytes: N must lie in [1, 2^31), got %lld", (long long)N);
    Carve c;
    c.take((int64_t)sizeof(State));
    return c.total;
}

extern "C" int dlpm_toy_finish_f32(float *x_dev, int64_t N, int32_t normalize, int32_t std_divisor, int32_t between, double q,
                                   void *workspace_dev, int64_t workspace_bytes, double *out_dev, int32_t *status_dev,
                                   dlpm_stream_t stream) {
    DLPM_CHECK_ARG(N > 0 && N < (1ll << 31), "dlpm_toy_finish_f32: N must lie in [1, 2^31), got %lld", (long long)N);
    DLPM_CHECK_ARG(x_dev && workspace_dev && status_dev, "dlpm_toy_finish_f32: null pointer");
    DLPM_CHECK_ARG(std_divisor == 0 || std_divisor == 1, "dlpm_toy_finish_f32: std_divisor is 0 (2 N) or 1 (2 N - 1), got %d", std_divisor);
    DLPM_CHECK_ARG(!between || (q > 0.5 && q <= 1.0), "dlpm_toy_finish_f32: quantile_cutoff must lie in (0.5, 1], got %g", q);
    DLPM_CHECK_ARG(reinterpret_cast<uintptr_t>(x_dev) % 8 == 0 && reinterpret_cast<uintptr_t>(out_dev) % 8 == 0 &&
                       reinterpret_cast<uintptr_t>(status_dev) % 4 == 0,
                   "dlpm_toy_finish_f32: misaligned pointer");
    const int rc = check_workspace("dlpm_toy_finish_f32", workspace_dev, workspace_bytes, dlpm_toy_workspace_bytes(N));
    if (rc != DLPM_OK) return rc;
    hipStream_t st = as_stream(stream);
    State *s = static_cast<State *>(workspace_dev);
    const unsigned blocks = (unsigned)ceil_div(N, 256);
    if (normalize) {
        ProfScope ps("toy_normalize", 0.0, 32.0 * (double)N, st);
        k_toy_moments<<<1, kThreads, 0, st>>>(x_dev, 2 * N, std_divisor, s, out_dev);
        DLPM_LAUNCH_CHECK();
        k_toy_normalize<<<blocks, 256, 0, st>>>(x_dev, N, s);
        DLPM_LAUNCH_CHECK();
    }
    if (between) {
        ProfScope ps("toy_between", 0.0, (32.0 * 8.0 + 16.0) * (double)N, st);
        k_toy_select<<<4, kThreads, 0, st>>>(x_dev, N, nearest_rank(q, N), nearest_rank(1.0 - q, N), s, out_dev);
        DLPM_LAUNCH_CHECK();
        k_toy_clamp<<<blocks, 256, 0, st>>>(x_dev, N, s, out_dev, status_dev);
        DLPM_LAUNCH_CHECK();
    } else {
        k_toy_status_ok<<<1, 1, 0, st>>>(status_dev);
        DLPM_LAUNCH_CHECK();
    }
    return DLPM_OK;
}
