// tail.hip -- the tail figures of two sample sets (include/dlpm_amd_tail.h): the mean squared logarithmic error between
// their upper quantiles (MSLE above a level xi, Allouche et al. 2022) and the Hill estimate of each set's tail index.  Both are
// functions of the order statistics s[r0 .. N - 1] of a non-negative marginal, r0 = min(floor(xi (N - 1)), N - 2), and those are
// found exactly:
//   k_tail_init -> k_tail_values -> 4 x (k_tail_digits -> k_tail_pick) -> k_tail_compact ->
//   4 x (k_tail_radix_count -> k_tail_radix_scan -> k_tail_radix_scatter) -> k_tail_quantiles -> k_tail_hill -> k_tail_finish
//   * values: the marginal of every sample as the order-preserving key of an fp32 (key_of), with the non-finite flag;
//   * select: the key of rank r0 by a 4 x 8-bit radix select, both sets in one grid (blockIdx.y); it also gives the number m of keys
//     strictly above it.  This file's own select: the kernels of wass.hip and toy.hip stay as they are;
//   * compact: the m keys above the threshold into a buffer of k = N - 1 - r0 slots (m <= k), a slot per key from one integer atomic
//     per wavefront; slot order is arbitrary, the sort follows.  Ranks r0 .. N - 1 - m hold the threshold itself and need no storage;
//   * sort: an LSD radix sort of the compacted keys, 4 x 8 bits, stable by construction (no atomics on global memory).  Rank by
//     counting was built first and took more than select and compaction together from 50 000 keys on (profiles/tail/README.md);
//   * quantiles, Hill, finish: numpy's 'linear' rule, ocml's fp64 log, every sum in the order the header states.
// One enqueue sequence, no host synchronisation, integer atomics only: graph-capturable, and the same inputs give the same bits.
#include <cmath>
#include <limits>

#include "metrics_common.h"
#include "../../include/dlpm_amd_tail.h"

using namespace dlpm;

namespace {

constexpr int kThreads = 256;
constexpr int kStreamBlocks = 1024;       // most workgroups per set of a streaming pass (grid-stride beyond)
constexpr int kRunKeys = 2048;            // slots per run of the radix sort where k allows, and
constexpr int kMaxRuns = 1024;            // the most runs (longer runs beyond)
constexpr int kHillRuns = 1024;           // runs of consecutive ranks of the Hill sum
constexpr int kTermTile = 4096;           // MSLE terms per LDS tile of the final sequential sum

enum Status { kOk = 0, kNonFinite = 1, kNoLogarithm = 2 };

struct SetState {
    unsigned int prefix, threshold, above, slots;     // select prefix; key of s[r0]; keys strictly above it; compaction counter
    long long rank;                                   // ranks still to skip below the current prefix
    double hill;
    int bad, pad;                                     // threshold <= 0
};

struct State {
    SetState set[2];
    int nonfinite, bad_q;
};

// what every kernel knows from the host: per set the source, the N marginal values' keys, the k slots of the compacted and the
// sorted tail, r0, and D
struct Sets {
    const float *src[2];
    unsigned int *keys[2], *raw[2], *sorted[2];
    int64_t N[2], r0[2], cap[2];
    int64_t D;
    int marginal;
};

__global__ void __launch_bounds__(512) k_tail_init(State *st, unsigned int *digits, Sets S) {
    digits[threadIdx.x] = 0u;
    if (threadIdx.x == 0) {
        *st = State{};
        st->set[0].rank = S.r0[0];
        st->set[1].rank = S.r0[1];
    }
}

// the marginal value of sample i as a key; norm: one thread per row, d ascending, every operation rounded on its own
__global__ void __launch_bounds__(kThreads) k_tail_values(Sets S, State *st) {
    const int set = blockIdx.y;
    const float *x = S.src[set];
    unsigned int *keys = S.keys[set];
    const int64_t N = S.N[set], D = S.D;
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < N; i += (int64_t)gridDim.x * kThreads) {
        float v;
        if (S.marginal == DLPM_TAIL_ABS) {
            v = fabsf(x[i]);
        } else {
            const float *row = x + i * D;
            double acc = 0.0;
            for (int64_t d = 0; d < D; d++) {
                const double t = (double)row[d];
                acc = __dadd_rn(acc, __dmul_rn(t, t));
            }
            v = (float)__dsqrt_rn(acc);
        }
        bad |= !isfinite(v);
        keys[i] = key_of(v);
    }
    if (bad) atomicOr(&st->nonfinite, 1);
}

// One 8-bit pass of the radix select: the digit histogram of the keys that carry the set's prefix
__global__ void __launch_bounds__(kThreads) k_tail_digits(Sets S, const State *st, unsigned int *digits, int pass) {
    __shared__ unsigned int h[256];
    if (st->nonfinite) return;
    const int set = blockIdx.y;
    h[threadIdx.x] = 0u;
    __syncthreads();
    const unsigned int *keys = S.keys[set];
    const int64_t N = S.N[set];
    const unsigned int prefix = st->set[set].prefix;
    const int shift = 24 - 8 * pass;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < N; i += (int64_t)gridDim.x * kThreads) {
        const unsigned int k = keys[i];
        if (pass == 0 || (k >> (shift + 8)) == prefix) atomicAdd(&h[(k >> shift) & 255u], 1u);
    }
    __syncthreads();
    const unsigned int v = h[threadIdx.x];
    if (v) atomicAdd(&digits[set * 256 + threadIdx.x], v);
}

// The digit of rank r0 and the new prefix; after the last pass the threshold key and the number of keys strictly above it
__global__ void __launch_bounds__(512) k_tail_pick(Sets S, State *st, unsigned int *digits, int pass) {
    __shared__ unsigned int h[512];
    h[threadIdx.x] = digits[threadIdx.x];
    digits[threadIdx.x] = 0u;
    __syncthreads();
    if (threadIdx.x >= 2 || st->nonfinite) return;
    const int set = threadIdx.x;
    SetState &q = st->set[set];
    const unsigned int *c = h + set * 256;
    long long r = q.rank;
    int d = 0;
    while (d < 255 && r >= (long long)c[d]) r -= (long long)c[d++];
    q.rank = r;
    q.prefix = (q.prefix << 8) | (unsigned int)d;
    if (pass == 3) {
        q.threshold = q.prefix;
        const long long below = S.r0[set] - r, equal = (long long)c[d];
        long long m = S.N[set] - below - equal;                           // ranks r0 + 1 .. N - 1 that are not ties of s[r0]
        m = m < 0 ? 0 : (m > S.cap[set] ? S.cap[set] : m);
        q.above = (unsigned int)m;
    }
}

// the keys strictly above the threshold into raw[0 .. m): one atomic per wavefront reserves its slots
__global__ void __launch_bounds__(kThreads) k_tail_compact(Sets S, State *st) {
    if (st->nonfinite) return;
    const int set = blockIdx.y;
    const unsigned int *keys = S.keys[set];
    unsigned int *raw = S.raw[set];
    const int64_t N = S.N[set], cap = S.cap[set];
    const unsigned int T = st->set[set].threshold;
    const int lane = threadIdx.x & 63;
    for (int64_t base = (int64_t)blockIdx.x * kThreads; base < N; base += (int64_t)gridDim.x * kThreads) {
        const int64_t i = base + threadIdx.x;
        const unsigned int k = i < N ? keys[i] : 0u;
        const bool mine = i < N && k > T;
        const unsigned long long mask = __ballot(mine);
        if (mask == 0ull) continue;
        const int leader = __ffsll((long long)mask) - 1;
        unsigned int first = 0u;
        if (lane == leader) first = atomicAdd(&st->set[set].slots, (unsigned int)__popcll(mask));
        first = __shfl(first, leader);
        if (mine) {
            const int64_t slot = (int64_t)first + __popcll(mask & ((1ull << lane) - 1ull));
            if (slot < cap) raw[slot] = k;
        }
    }
}

// The exact sort of the m compacted keys: an LSD radix sort, 4 passes of 8 bits, each pass count -> scan -> scatter.  The keys are cut
// into G runs of ceil(m / G) consecutive slots, one wavefront (a 64-thread workgroup) per run; G comes from the host (from k), m from
// the device.  A pass is stable: a run keeps its order (tiles of 64 in order, lanes in order inside a tile), runs go in order.
struct Run {
    unsigned int first, last;
};

__device__ inline Run run_of(unsigned int m, unsigned int G, unsigned int g) {
    const unsigned int per = (m + G - 1u) / G;
    const unsigned long long a = (unsigned long long)g * per, b = a + per;
    return Run{(unsigned int)(a < m ? a : m), (unsigned int)(b < m ? b : m)};
}

// hist[set][digit][run]: how many keys of the run carry the digit.  Every entry is written.  Grid (G, 2), 64 threads.
__global__ void __launch_bounds__(64) k_tail_radix_count(Sets S, const State *st, unsigned int *hist, int pass) {
    __shared__ unsigned int h[256];
    if (st->nonfinite) return;
    const int set = blockIdx.y, lane = threadIdx.x, shift = 8 * pass;
    const unsigned int *src = (pass & 1) ? S.sorted[set] : S.raw[set];
    const Run r = run_of(st->set[set].above, gridDim.x, blockIdx.x);
    for (int d = lane; d < 256; d += 64) h[d] = 0u;
    __syncthreads();
    for (unsigned int i = r.first + lane; i < r.last; i += 64) atomicAdd(&h[(src[i] >> shift) & 255u], 1u);
    __syncthreads();
    for (int d = lane; d < 256; d += 64) hist[((size_t)set * 256 + d) * gridDim.x + blockIdx.x] = h[d];
}

// the exclusive prefix of hist[set] in (digit, run) order, in place: where every (digit, run) group starts.  Grid 2, 1024 threads.
__global__ void __launch_bounds__(1024) k_tail_radix_scan(const State *st, unsigned int *hist, unsigned int G) {
    __shared__ unsigned int part[1024];
    if (st->nonfinite) return;
    unsigned int *h = hist + (size_t)blockIdx.x * 256 * G;
    const unsigned int total = 256u * G, per = (total + 1023u) / 1024u;
    const unsigned int a = min(threadIdx.x * per, total), b = min(a + per, total);
    unsigned int sum = 0u;
    for (unsigned int i = a; i < b; i++) sum += h[i];
    part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned int acc = 0u;
        for (int t = 0; t < 1024; t++) {
            const unsigned int v = part[t];
            part[t] = acc;
            acc += v;
        }
    }
    __syncthreads();
    unsigned int acc = part[threadIdx.x];
    for (unsigned int i = a; i < b; i++) {
        const unsigned int v = h[i];
        h[i] = acc;
        acc += v;
    }
}

// every key to the start of its (digit, run) group plus the number of keys of that digit before it in the run.  Grid (G, 2), 64 threads.
__global__ void __launch_bounds__(64) k_tail_radix_scatter(Sets S, const State *st, const unsigned int *hist, int pass) {
    __shared__ unsigned int off[256];
    if (st->nonfinite) return;
    const int set = blockIdx.y, lane = threadIdx.x, shift = 8 * pass;
    const unsigned int *src = (pass & 1) ? S.sorted[set] : S.raw[set];
    unsigned int *dst = (pass & 1) ? S.raw[set] : S.sorted[set];
    const unsigned int m = st->set[set].above;
    const Run r = run_of(m, gridDim.x, blockIdx.x);
    for (int d = lane; d < 256; d += 64) off[d] = hist[((size_t)set * 256 + d) * gridDim.x + blockIdx.x];
    __syncthreads();
    for (unsigned int base = r.first; base < r.last; base += 64) {
        const unsigned int i = base + lane;
        const bool mine = i < r.last;
        const unsigned int key = mine ? src[i] : 0u, d = (key >> shift) & 255u;
        unsigned long long same = __ballot(mine);                         // the lanes of this tile that carry my digit
        for (int bit = 0; bit < 8; bit++) {
            const bool one = (d >> bit) & 1u;
            const unsigned long long with = __ballot(one);
            same &= one ? with : ~with;
        }
        const unsigned int before = (unsigned int)__popcll(same & ((1ull << lane) - 1ull));
        const unsigned int start = off[d];
        __syncthreads();
        if (mine) {
            const unsigned int to = start + before;
            if (to < m) dst[to] = key;
            if (before == 0u) off[d] = start + (unsigned int)__popcll(same);
        }
        __syncthreads();
    }
}

// s[r] for r0 <= r <= N - 1: the threshold up to rank N - 1 - m, the sorted tail above
__device__ inline float at_rank(const Sets &S, const State *st, int set, int64_t r) {
    const int64_t first = S.N[set] - (int64_t)st->set[set].above;
    return value_of(r < first ? st->set[set].threshold : S.sorted[set][r - first]);
}

__device__ inline double quantile(const Sets &S, const State *st, int set, double u) {
    const int64_t N = S.N[set];
    const double h = __dmul_rn(u, (double)(N - 1));
    int64_t lo = (int64_t)floor(h);
    lo = lo < S.r0[set] ? S.r0[set] : (lo > N - 1 ? N - 1 : lo);          // both hold already: u >= xi, and u <= 1
    const int64_t hi = lo + 1 < N - 1 ? lo + 1 : N - 1;
    const double a = (double)at_rank(S, st, set, lo), b = (double)at_rank(S, st, set, hi);
    return __dadd_rn(a, __dmul_rn(__dsub_rn(h, (double)lo), __dsub_rn(b, a)));
}

// level j: both quantiles, the flag for one <= 0, and the term (log q_x - log q_y)^2
__global__ void __launch_bounds__(kThreads) k_tail_quantiles(Sets S, State *st, double xi, int levels, double *q, double *terms) {
    const int j = blockIdx.x * kThreads + threadIdx.x;
    if (j >= levels) return;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    if (st->nonfinite) {
        q[j] = q[levels + j] = terms[j] = nan;
        return;
    }
    const double u = __dadd_rn(xi, __ddiv_rn(__dmul_rn(__dsub_rn(1.0, xi), (double)j), (double)levels));
    const double qx = quantile(S, st, 0, u), qy = quantile(S, st, 1, u);
    q[j] = qx;
    q[levels + j] = qy;
    if (!(qx > 0.0) || !(qy > 0.0)) {
        atomicOr(&st->bad_q, 1);
        terms[j] = nan;
        return;
    }
    const double d = __dsub_rn(log(qx), log(qy));
    terms[j] = __dmul_rn(d, d);
}

// Hill index of set blockIdx.x: thread c adds run c of the k log ratios in rank order, thread 0 the 1024 runs in order
__global__ void __launch_bounds__(kHillRuns) k_tail_hill(Sets S, State *st) {
    __shared__ double part[kHillRuns];
    if (st->nonfinite) return;
    const int set = blockIdx.x;
    const float T = value_of(st->set[set].threshold);
    if (!(T > 0.0f)) {
        if (threadIdx.x == 0) {
            st->set[set].hill = std::numeric_limits<double>::quiet_NaN();
            st->set[set].bad = 1;
        }
        return;
    }
    const int64_t r0 = S.r0[set], k = S.N[set] - 1 - r0, per = (k + kHillRuns - 1) / kHillRuns;
    const double logT = log((double)T);
    const int64_t lo = (int64_t)threadIdx.x * per, t0 = lo < k ? lo : k, t1 = t0 + per < k ? t0 + per : k;
    double acc = 0.0;
    for (int64_t t = t0; t < t1; t++) acc = __dadd_rn(acc, __dsub_rn(log((double)at_rank(S, st, set, r0 + 1 + t)), logT));
    part[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double sum = 0.0;
        for (int c = 0; c < kHillRuns; c++) sum = __dadd_rn(sum, part[c]);
        st->set[set].hill = __ddiv_rn((double)k, sum);                    // all ties: k / +0 = +inf
    }
}

// msle = (sum of the terms, one after the other) / levels, and the output vector
__global__ void __launch_bounds__(kThreads) k_tail_finish(Sets S, const State *st, int levels, const double *terms, double *out) {
    __shared__ double tile[kTermTile];
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const bool sum_it = !st->nonfinite && !st->bad_q;
    double sum = 0.0;
    if (sum_it) {
        for (int base = 0; base < levels; base += kTermTile) {
            const int count = min(kTermTile, levels - base);
            __syncthreads();
            for (int q = threadIdx.x; q < count; q += kThreads) tile[q] = terms[base + q];
            __syncthreads();
            if (threadIdx.x == 0)
                for (int q = 0; q < count; q++) sum = __dadd_rn(sum, tile[q]);
        }
    }
    if (threadIdx.x != 0) return;
    const bool bad = st->nonfinite != 0;
    out[0] = sum_it ? __ddiv_rn(sum, (double)levels) : nan;
    for (int set = 0; set < 2; set++) {
        out[1 + set] = bad ? nan : st->set[set].hill;
        out[3 + 2 * set] = (double)(S.N[set] - 1 - S.r0[set]);
        out[4 + 2 * set] = bad ? nan : (double)value_of(st->set[set].threshold);
    }
    out[7] = (double)(bad ? kNonFinite : ((st->bad_q || st->set[0].bad || st->set[1].bad) ? kNoLogarithm : kOk));
}

struct Layout {
    int64_t state, digits, keys[2], raw[2], sorted[2], hist, q, terms, total;
    int64_t runs;
    int64_t N[2], r0[2], cap[2];
};

Layout layout_of(int64_t n1, int64_t n2, int64_t D, int marginal, double xi, int64_t levels) {
    Layout L{};
    Carve c;
    const int64_t n[2] = {n1, n2};
    for (int s = 0; s < 2; s++) {
        L.N[s] = marginal == DLPM_TAIL_ABS ? n[s] * D : n[s];
        L.r0[s] = std::min<int64_t>((int64_t)std::floor(xi * (double)(L.N[s] - 1)), L.N[s] - 2);
        L.cap[s] = L.N[s] - 1 - L.r0[s];
    }
    L.state = c.take((int64_t)sizeof(State));
    L.digits = c.take(2 * 256 * (int64_t)sizeof(unsigned int));
    for (int s = 0; s < 2; s++) L.keys[s] = c.take(L.N[s] * (int64_t)sizeof(unsigned int));
    for (int s = 0; s < 2; s++) L.raw[s] = c.take(L.cap[s] * (int64_t)sizeof(unsigned int));
    for (int s = 0; s < 2; s++) L.sorted[s] = c.take(L.cap[s] * (int64_t)sizeof(unsigned int));
    L.runs = std::min<int64_t>(kMaxRuns, ceil_div(std::max(L.cap[0], L.cap[1]), kRunKeys));
    L.hist = c.take(2 * 256 * L.runs * (int64_t)sizeof(unsigned int));
    L.q = c.take(2 * levels * (int64_t)sizeof(double));
    L.terms = c.take(levels * (int64_t)sizeof(double));
    L.total = c.total;
    return L;
}

int check_shape(const char *who, int64_t n1, int64_t n2, int64_t D, int marginal, double xi, int64_t levels) {
    DLPM_CHECK_ARG(n1 >= 2 && n2 >= 2 && D >= 1, "%s: bad shape n1=%lld n2=%lld D=%lld (at least 2 samples a set)", who, (long long)n1,
                   (long long)n2, (long long)D);
    DLPM_CHECK_ARG(n1 <= INT32_MAX / D && n2 <= INT32_MAX / D, "%s: shape out of range (more than 2^31 - 1 values in a set)", who);
    DLPM_CHECK_ARG(marginal == DLPM_TAIL_NORM || marginal == DLPM_TAIL_ABS, "%s: unknown marginal %d", who, marginal);
    DLPM_CHECK_ARG(xi >= 0.5 && xi < 1.0, "%s: xi must be in [0.5, 1), got %g", who, xi);
    DLPM_CHECK_ARG(levels >= 1 && levels <= DLPM_TAIL_MAX_LEVELS, "%s: levels must be in [1, %d], got %lld", who, DLPM_TAIL_MAX_LEVELS,
                   (long long)levels);
    return DLPM_OK;
}

}  // namespace

extern "C" int64_t dlpm_tail_workspace_bytes(int64_t n1, int64_t n2, int64_t D, int32_t marginal, double xi, int32_t levels) {
    const int rc = check_shape("dlpm_tail_workspace_bytes", n1, n2, D, marginal, xi, levels);
    if (rc != DLPM_OK) return rc;
    return layout_of(n1, n2, D, marginal, xi, levels).total;
}

extern "C" int dlpm_tail_f32(const float *x_dev, int64_t n1, const float *y_dev, int64_t n2, int64_t D, int32_t marginal, double xi,
                             int32_t levels, void *workspace_dev, int64_t workspace_bytes, double *quantiles_out_dev, double *out_dev,
                             dlpm_stream_t stream) {
    const int rc = check_shape("dlpm_tail_f32", n1, n2, D, marginal, xi, levels);
    if (rc != DLPM_OK) return rc;
    DLPM_CHECK_ARG(x_dev && y_dev && workspace_dev && out_dev, "dlpm_tail_f32: null pointer");
    DLPM_CHECK_ARG(aligned(x_dev, 4) && aligned(y_dev, 4) && aligned(out_dev, 8) && aligned(quantiles_out_dev, 8),
                   "dlpm_tail_f32: misaligned pointer");
    const Layout L = layout_of(n1, n2, D, marginal, xi, levels);
    const int ws_rc = check_workspace("dlpm_tail_f32", workspace_dev, workspace_bytes, L.total);
    if (ws_rc != DLPM_OK) return ws_rc;

    hipStream_t st = as_stream(stream);
    char *ws = static_cast<char *>(workspace_dev);
    State *state = reinterpret_cast<State *>(ws + L.state);
    unsigned int *digits = reinterpret_cast<unsigned int *>(ws + L.digits);
    double *q = quantiles_out_dev ? quantiles_out_dev : reinterpret_cast<double *>(ws + L.q);
    double *terms = reinterpret_cast<double *>(ws + L.terms);
    Sets S{};
    S.src[0] = x_dev;
    S.src[1] = y_dev;
    S.D = D;
    S.marginal = marginal;
    for (int s = 0; s < 2; s++) {
        S.keys[s] = reinterpret_cast<unsigned int *>(ws + L.keys[s]);
        S.raw[s] = reinterpret_cast<unsigned int *>(ws + L.raw[s]);
        S.sorted[s] = reinterpret_cast<unsigned int *>(ws + L.sorted[s]);
        S.N[s] = L.N[s];
        S.r0[s] = L.r0[s];
        S.cap[s] = L.cap[s];
    }
    const int64_t Nmax = std::max(L.N[0], L.N[1]);
    const dim3 values_grid((unsigned)std::min<int64_t>(kStreamBlocks, ceil_div(Nmax, kThreads)), 2);
    const dim3 stream_grid((unsigned)std::min<int64_t>(kStreamBlocks, ceil_div(Nmax, (int64_t)kThreads * 8)), 2);
    const double key_bytes = 4.0 * (double)(L.N[0] + L.N[1]);

    k_tail_init<<<1, 512, 0, st>>>(state, digits, S);
    DLPM_LAUNCH_CHECK();
    {
        ProfScope ps("tail_values", 0.0, 4.0 * (double)((n1 + n2) * D) + key_bytes, st);
        k_tail_values<<<values_grid, kThreads, 0, st>>>(S, state);
        DLPM_LAUNCH_CHECK();
    }
    {
        ProfScope ps("tail_select", 0.0, 4.0 * key_bytes, st);
        for (int pass = 0; pass < 4; pass++) {
            k_tail_digits<<<stream_grid, kThreads, 0, st>>>(S, state, digits, pass);
            DLPM_LAUNCH_CHECK();
            k_tail_pick<<<1, 512, 0, st>>>(S, state, digits, pass);
            DLPM_LAUNCH_CHECK();
        }
    }
    {
        ProfScope ps("tail_compact", 0.0, key_bytes, st);
        k_tail_compact<<<stream_grid, kThreads, 0, st>>>(S, state);
        DLPM_LAUNCH_CHECK();
    }
    {
        ProfScope ps("tail_sort", 0.0, 0.0, st);
        unsigned int *hist = reinterpret_cast<unsigned int *>(ws + L.hist);
        const dim3 runs((unsigned)L.runs, 2);
        for (int pass = 0; pass < 4; pass++) {
            k_tail_radix_count<<<runs, 64, 0, st>>>(S, state, hist, pass);
            DLPM_LAUNCH_CHECK();
            k_tail_radix_scan<<<2, 1024, 0, st>>>(state, hist, (unsigned)L.runs);
            DLPM_LAUNCH_CHECK();
            k_tail_radix_scatter<<<runs, 64, 0, st>>>(S, state, hist, pass);
            DLPM_LAUNCH_CHECK();
        }
    }
    for (int s = 0; s < 2; s++) S.sorted[s] = S.raw[s];                  // four passes: the sorted keys are back in the first buffer
    {
        ProfScope ps("tail_figures", 0.0, 0.0, st);
        k_tail_quantiles<<<(unsigned)ceil_div(levels, kThreads), kThreads, 0, st>>>(S, state, xi, levels, q, terms);
        DLPM_LAUNCH_CHECK();
        k_tail_hill<<<2, kHillRuns, 0, st>>>(S, state);
        DLPM_LAUNCH_CHECK();
        k_tail_finish<<<1, kThreads, 0, st>>>(S, state, levels, terms, out_dev);
        DLPM_LAUNCH_CHECK();
    }
    return DLPM_OK;
}
