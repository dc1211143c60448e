// wass.hip -- the `wass` figure of bem/evaluate/EvaluationManager.py:146-151: compute_wasserstein_distance (bem/evaluate/wasserstein.py:47-52)
// = pyemd.emd_samples: both arrays FLATTENED, one shared histogram range, two normalised histograms, and the transport optimum with
// the distance between bin centres as ground metric.  That is a 1-D earth mover's distance, whose optimum is the closed form
//   wass = sum_i |F_i - G_i| (c_{i+1} - c_i),   F, G the cumulative histograms, c the bin centres        
// so no solver is needed: a pooled min / max, numpy's 'auto' bin rule (exact quartiles of the pooled values), two histograms with
// numpy's exact bin assignment, and a scan.  One enqueue sequence on the caller's stream, no host synchronisation:
//   k_wass_init -> k_wass_range -> k_wass_setup -> ['auto': 4 x (k_wass_digits -> k_wass_pick)] -> k_wass_zero -> k_wass_hist -> k_wass_emd
// Integer atomics only (min / max of ordered keys, counts); cumulative counts are int64; the fp64 terms are added in a fixed order:
// the same inputs give the same bits.  All element indices are 64-bit.
#include <cmath>
#include <limits>

#include "metrics_common.h"

using namespace dlpm;

namespace {

constexpr int kLdsBins = 16384;           // both int32 histograms in LDS up to this many bins (2 x 64 KB of the 160 KB)
constexpr int kMaxBinsLimit = 1 << 20;
constexpr int kStreamBlocks = 1024;       // most workgroups of a streaming pass (grid-stride beyond)
constexpr int kThreads = 1024;

enum Status { kOk = 0, kNonFiniteData = 1, kNonFiniteRange = 2, kInvertedRange = 3, kTooManyBins = 4 };

struct State {
    unsigned int minkey, maxkey, nonfinite;      // ordered keys of the smallest / largest value inside the range
    int status, nb, nslots;
    unsigned long long m;                        // values inside the range, both arrays
    double lo, hi, width, q25, q75, gamma[2];
    long long rank[4];                           // radix select: ranks still to skip below the current prefix (75 %: 0, 1; 25 %: 2, 3)
    unsigned int prefix[4], slot_prefix[4];
    int slot_of[4];                              // ranks with the same prefix share one digit histogram
    float os[4];
};

// every value of p[0 .. count) once across the grid: 16-byte loads from the first aligned element, scalar head and tail
template <class F>
__device__ inline void for_values(const float *p, int64_t count, F f) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, S = (int64_t)gridDim.x * blockDim.x;
    int64_t head = (int64_t)((4 - ((reinterpret_cast<uintptr_t>(p) >> 2) & 3)) & 3);
    head = head < count ? head : count;
    const int64_t nvec = (count - head) / 4, tail = count - head - 4 * nvec;
    const float4 *v = reinterpret_cast<const float4 *>(p + head);
    for (int64_t i = g; i < nvec; i += S) {
        const float4 q = v[i];
        f(q.x);
        f(q.y);
        f(q.z);
        f(q.w);
    }
    if (g < head) f(p[g]);
    if (g < tail) f(p[head + 4 * nvec + g]);
}

__global__ void __launch_bounds__(kThreads) k_wass_init(State *s, unsigned long long *digits) {
    if (threadIdx.x == 0) {
        *s = State{};
        s->minkey = 0xffffffffu;
    }
    digits[threadIdx.x] = 0ull;
}

// min / max / count of the values inside [lo, hi] (has_range) or of all values, with a flag for a non-finite one
__global__ void __launch_bounds__(kThreads) k_wass_range(const float *x, int64_t c1, const float *y, int64_t c2, int has_range, double lo,
                                                         double hi, State *s) {
    __shared__ unsigned int smin, smax, sbad;
    __shared__ unsigned long long scount;
    if (threadIdx.x == 0) {
        smin = 0xffffffffu;
        smax = 0u;
        sbad = 0u;
        scount = 0ull;
    }
    __syncthreads();
    unsigned int kmin = 0xffffffffu, kmax = 0u, bad = 0u;
    unsigned long long count = 0ull;
    auto f = [&](float v) {
        if (has_range) {
            const double d = (double)v;
            if (!(d >= lo && d <= hi)) return;
        } else if (!isfinite(v)) {
            bad = 1u;
            return;
        }
        const unsigned int k = key_of(v);
        kmin = k < kmin ? k : kmin;
        kmax = k > kmax ? k : kmax;
        count++;
    };
    for_values(x, c1, f);
    for_values(y, c2, f);
    if (count) {
        atomicMin(&smin, kmin);
        atomicMax(&smax, kmax);
        atomicAdd(&scount, count);
    }
    if (bad) atomicOr(&sbad, 1u);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (scount) {
            atomicMin(&s->minkey, smin);
            atomicMax(&s->maxkey, smax);
            atomicAdd(&s->m, scount);
        }
        if (sbad) atomicOr(&s->nonfinite, 1u);
    }
}

__device__ inline void write_head(const State *s, double *out) {
    out[1] = (double)s->nb;
    out[2] = s->lo;
    out[3] = s->hi;
    out[4] = s->width;
    out[5] = s->q25;
    out[6] = s->q75;
    for (int j = 0; j < 4; j++) out[7 + j] = (double)s->os[j];
    out[11] = (double)s->status;
}

// The outer edges as np.histogram's _get_outer_edges (an explicit range arrives already checked and widened: range_status), the bin
// count when the caller gives it, and for 'auto' the four ranks np.percentile(pooled, [75, 25]) interpolates between.
__global__ void k_wass_setup(State *s, int bins, int has_range, double lo, double hi, int range_status, int max_bins, double *out) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    s->q25 = s->q75 = s->width = nan;
    for (int j = 0; j < 4; j++) s->os[j] = std::numeric_limits<float>::quiet_NaN();
    if (has_range) {
        s->status = range_status;
        s->lo = lo;
        s->hi = hi;
    } else if (s->nonfinite) {
        s->status = kNonFiniteData;
        s->lo = s->hi = nan;
    } else {
        float a = value_of(s->minkey), b = value_of(s->maxkey);          // np.float32 scalars: the widening runs in fp32
        if (a == b) {
            a = __fsub_rn(a, 0.5f);
            b = __fadd_rn(b, 0.5f);
        }
        s->lo = (double)a;
        s->hi = (double)b;
    }
    if (s->status == kOk && bins > 0) {
        if (bins > max_bins) s->status = kTooManyBins;
        else {
            s->nb = bins;
            s->width = __ddiv_rn(__dsub_rn(s->hi, s->lo), (double)bins);
        }
    }
    if (s->status == kOk && bins == 0) {
        const long long m = (long long)s->m;
        if (m == 0) {
            s->nb = 1;                                                   // numpy: no selector on an empty array
        } else {
            const double q[2] = {0.75, 0.25};
            for (int j = 0; j < 2; j++) {
                // method='linear': virtual index (n - 1) * q, then _get_indexes / _get_gamma (q = 0.75 or 0.25 in fp64)
                const double vi = __dmul_rn((double)(m - 1), q[j]);
                long long prev = (long long)floor(vi), next = prev + 1;
                double g = __dsub_rn(vi, (double)prev);
                if (vi >= (double)(m - 1)) {
                    prev = next = m - 1;
                    g = __dsub_rn(vi, -1.0);
                }
                s->rank[2 * j] = prev;
                s->rank[2 * j + 1] = next;
                s->gamma[j] = g;
            }
            s->nslots = 1;
        }
    }
    write_head(s, out);
    out[0] = nan;
}

// One 8-bit pass of the radix select: digit histograms of the keys that carry a rank's prefix, one histogram per distinct prefix
__global__ void __launch_bounds__(kThreads) k_wass_digits(const float *x, int64_t c1, const float *y, int64_t c2, const State *s,
                                                          unsigned long long *digits, int pass) {
    __shared__ unsigned int h[4 * 256];
    if (s->status != kOk || s->nslots == 0) return;
    h[threadIdx.x] = 0u;
    __syncthreads();
    const int nslots = s->nslots, shift = 24 - 8 * pass;
    const double lo = s->lo, hi = s->hi;
    unsigned int pre[4];
    for (int j = 0; j < 4; j++) pre[j] = s->slot_prefix[j];
    auto f = [&](float v) {
        const double d = (double)v;
        if (!(d >= lo && d <= hi)) return;
        const unsigned int k = key_of(v), top = pass == 0 ? 0u : k >> (shift + 8), digit = (k >> shift) & 255u;
        for (int j = 0; j < nslots; j++)
            if (top == pre[j]) atomicAdd(&h[j * 256 + digit], 1u);
    };
    for_values(x, c1, f);
    for_values(y, c2, f);
    __syncthreads();
    const unsigned int v = h[threadIdx.x];
    if (v && (int)(threadIdx.x >> 8) < nslots) atomicAdd(&digits[threadIdx.x], (unsigned long long)v);
}

// numpy's _hist_bin_auto on fp32 data, operation by operation and dtype by dtype (numpy 2.x, NEP 50): np.percentile's q is fp64
// ([75, 25] / np.float32(100) is an int64 array over an fp32 SCALAR), _lerp's b - a is fp32 and its products fp64, _ptp is fp32 and
// divided by an fp64, last_edge - first_edge is fp32 for autodetected edges (fp64 for a range of Python floats), the quotient fp64.
__device__ void auto_bins(State *s, int has_range, int max_bins) {
    const double m = (double)s->m;
    double qv[2];
    for (int j = 0; j < 2; j++) {
        const float a = s->os[2 * j], b = s->os[2 * j + 1];
        const double diff = (double)__fsub_rn(b, a), t = s->gamma[j];
        double r = __dadd_rn((double)a, __dmul_rn(diff, t));
        if (t >= 0.5) r = __dsub_rn((double)b, __dmul_rn(diff, __dsub_rn(1.0, t)));
        qv[j] = r;
    }
    s->q75 = qv[0];
    s->q25 = qv[1];
    const double iqr = __dsub_rn(qv[0], qv[1]);
    const double fd = __dmul_rn(__dmul_rn(2.0, iqr), pow(m, -1.0 / 3.0));
    const double ptp = (double)__fsub_rn(value_of(s->maxkey), value_of(s->minkey));
    const double sturges = __ddiv_rn(ptp, __dadd_rn(log2(m), 1.0));
    const double width = fd != 0.0 ? (sturges < fd ? sturges : fd) : sturges;       // Python's min(fd, sturges)
    s->width = width;
    const double span = has_range ? __dsub_rn(s->hi, s->lo) : (double)__fsub_rn((float)s->hi, (float)s->lo);
    double count = 1.0;
    if (width != 0.0) count = ceil(__ddiv_rn(span, width));
    if (!(count <= (double)max_bins)) {
        s->status = kTooManyBins;
        return;
    }
    s->nb = count < 1.0 ? 1 : (int)count;
}

// The digit of every rank, the new prefixes and their sharing; after the last pass the order statistics and the bin count
__global__ void __launch_bounds__(kThreads) k_wass_pick(State *s, unsigned long long *digits, int pass, int has_range, int max_bins,
                                                        double *out) {
    __shared__ unsigned long long h[4 * 256];
    h[threadIdx.x] = digits[threadIdx.x];
    digits[threadIdx.x] = 0ull;
    __syncthreads();
    if (threadIdx.x != 0 || s->status != kOk || s->nslots == 0) return;
    for (int j = 0; j < 4; j++) {
        const unsigned long long *c = h + s->slot_of[j] * 256;
        long long r = s->rank[j];
        int d = 0;
        while (d < 255 && r >= (long long)c[d]) r -= (long long)c[d++];
        s->rank[j] = r;
        s->prefix[j] = (s->prefix[j] << 8) | (unsigned int)d;
    }
    int n = 0;
    for (int j = 0; j < 4; j++) {
        int at = -1;
        for (int q = 0; q < n; q++)
            if (s->slot_prefix[q] == s->prefix[j]) at = q;
        if (at < 0) {
            at = n++;
            s->slot_prefix[at] = s->prefix[j];
        }
        s->slot_of[j] = at;
    }
    s->nslots = n;
    if (pass == 3) {
        for (int j = 0; j < 4; j++) s->os[j] = value_of(s->prefix[j]);
        auto_bins(s, has_range, max_bins);
        write_head(s, out);
    }
}

__global__ void __launch_bounds__(kThreads) k_wass_zero(const State *s, int32_t *hist, int64_t stride) {
    const int nb = s->status == kOk ? s->nb : 0;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < nb; i += (int64_t)gridDim.x * kThreads) {
        hist[i] = 0;
        hist[stride + i] = 0;
    }
}

// np.linspace(lo, hi, nb + 1) in fp64: arange * step + start, each edge a separately rounded multiply then add; the last is hi itself
struct Edges {
    double lo, hi, delta, step;
    int nb;
    __device__ Edges(const State *s) : lo(s->lo), hi(s->hi), nb(s->nb) {
        delta = __dsub_rn(hi, lo);
        step = __ddiv_rn(delta, (double)nb);
    }
    __device__ double at(int i) const {
        if (i >= nb) return hi;
        if (step == 0.0) return __dadd_rn(__dmul_rn(__ddiv_rn((double)i, (double)nb), delta), lo);
        return __dadd_rn(__dmul_rn((double)i, step), lo);
    }
    // np.histogram's uniform-bin assignment: the estimate from the quotient, then its correction against the actual edges;
    // -1 for a value outside [lo, hi] (NaN included)
    __device__ int bin(float v) const {
        const double d = (double)v;
        if (!(d >= lo && d <= hi)) return -1;
        int i = (int)__dmul_rn(__ddiv_rn(__dsub_rn(d, lo), delta), (double)nb);
        if (i >= nb) i = nb - 1;
        if (d < at(i)) i--;
        if (i != nb - 1 && d >= at(i + 1)) i++;
        return i < 0 ? 0 : (i > nb - 1 ? nb - 1 : i);
    }
};

// One pass over each array.  Counts are privatised per workgroup in LDS when both histograms fit `lds_bins`, then flushed with global
// integer atomics; above that every value is one global atomic.
__global__ void __launch_bounds__(kThreads) k_wass_hist(const float *x, int64_t c1, const float *y, int64_t c2, const State *s,
                                                        int32_t *hist, int64_t stride, int lds_bins) {
    extern __shared__ __attribute__((aligned(16))) int32_t lh[];
    if (s->status != kOk || s->nb < 1) return;
    const Edges e(s);
    const int nb = e.nb;
    if (nb <= lds_bins) {
        for (int i = threadIdx.x; i < 2 * nb; i += kThreads) lh[i] = 0;
        __syncthreads();
        for_values(x, c1, [&](float v) {
            const int b = e.bin(v);
            if (b >= 0) atomicAdd(&lh[b], 1);
        });
        for_values(y, c2, [&](float v) {
            const int b = e.bin(v);
            if (b >= 0) atomicAdd(&lh[nb + b], 1);
        });
        __syncthreads();
        for (int i = threadIdx.x; i < 2 * nb; i += kThreads) {
            const int32_t v = lh[i];
            if (v) atomicAdd(i < nb ? &hist[i] : &hist[stride + (i - nb)], v);
        }
    } else {
        for_values(x, c1, [&](float v) {
            const int b = e.bin(v);
            if (b >= 0) atomicAdd(&hist[b], 1);
        });
        for_values(y, c2, [&](float v) {
            const int b = e.bin(v);
            if (b >= 0) atomicAdd(&hist[stride + b], 1);
        });
    }
}

// One workgroup: exact int64 cumulative counts, F_i - G_i = C1_i / n1' - C2_i / n2' in fp64, times the centre spacing
// c_{i+1} - c_i = (edge[i+2] - edge[i]) / 2 (one rounded subtraction of the edges: its error is relative to the spacing, not to |lo|),
// thread t owning the bins [t * chunk, (t + 1) * chunk) and the partial sums added by the fixed tree of block_sum.
__global__ void __launch_bounds__(kThreads) k_wass_emd(const State *s, const int32_t *hist, int64_t stride, double *out) {
    __shared__ long long p1[kThreads], p2[kThreads];
    __shared__ double sh[kThreads];
    __shared__ long long tot[2];
    const int t = threadIdx.x;
    if (s->status != kOk || s->nb < 1) {
        if (t == 0) {
            write_head(s, out);
            out[0] = std::numeric_limits<double>::quiet_NaN();
        }
        return;
    }
    const Edges e(s);
    const int nb = e.nb, chunk = (nb + kThreads - 1) / kThreads;
    const int b0 = min(t * chunk, nb), b1 = min(b0 + chunk, nb);
    long long s1 = 0, s2 = 0;
    for (int i = b0; i < b1; i++) {
        s1 += hist[i];
        s2 += hist[stride + i];
    }
    p1[t] = s1;
    p2[t] = s2;
    __syncthreads();
    if (t == 0) {
        long long a = 0, b = 0;
        for (int i = 0; i < kThreads; i++) {
            const long long va = p1[i], vb = p2[i];
            p1[i] = a;
            p2[i] = b;
            a += va;
            b += vb;
        }
        tot[0] = a;
        tot[1] = b;
    }
    __syncthreads();
    const double n1 = (double)tot[0], n2 = (double)tot[1];           // counts inside the range; 0 gives 0 / 0 = NaN as pyemd
    long long C1 = p1[t], C2 = p2[t];
    double acc = 0.0;
    for (int i = b0; i < b1; i++) {
        C1 += hist[i];
        C2 += hist[stride + i];
        if (i < nb - 1) {
            const double diff = fabs(__dsub_rn(__ddiv_rn((double)C1, n1), __ddiv_rn((double)C2, n2)));
            const double spacing = __dmul_rn(0.5, __dsub_rn(e.at(i + 2), e.at(i)));
            acc = __dadd_rn(acc, __dmul_rn(diff, spacing));
        }
    }
    if (nb == 1 && t == 0) acc = __dmul_rn(0.0, __dadd_rn(__ddiv_rn(0.0, n1), __ddiv_rn(0.0, n2)));     // NaN for an empty set
    const double total = block_sum<kThreads>(acc, sh);
    if (t == 0) {
        write_head(s, out);
        out[0] = total;
    }
}

struct Layout {
    int64_t state, digits, hist, total;
};

Layout layout_of(int64_t max_bins) {
    Layout L{};
    Carve c;
    L.state = c.take((int64_t)sizeof(State));
    L.digits = c.take(4 * 256 * (int64_t)sizeof(unsigned long long));
    L.hist = c.take(2 * max_bins * (int64_t)sizeof(int32_t));
    L.total = c.total;
    return L;
}

int check_shape(const char *who, int64_t n1, int64_t n2, int64_t D, int64_t max_bins) {
    DLPM_CHECK_ARG(n1 >= 1 && n2 >= 1 && D >= 1, "%s: bad shape n1=%lld n2=%lld D=%lld", who, (long long)n1, (long long)n2, (long long)D);
    DLPM_CHECK_ARG(max_bins >= 1 && max_bins <= kMaxBinsLimit, "%s: max_bins must be in [1, %d], got %lld", who, kMaxBinsLimit,
                   (long long)max_bins);
    // int32 bin counts: no array may hold more than 2^31 - 1 values
    DLPM_CHECK_ARG(n1 <= INT32_MAX / D && n2 <= INT32_MAX / D, "%s: shape out of range (more than 2^31 - 1 values in an array)", who);
    return DLPM_OK;
}

}  // namespace

extern "C" int64_t dlpm_wass_workspace_bytes(int64_t n1, int64_t n2, int64_t D, int64_t max_bins) {
    const int rc = check_shape("dlpm_wass_workspace_bytes", n1, n2, D, max_bins);
    if (rc != DLPM_OK) return rc;
    return layout_of(max_bins).total;
}

extern "C" int dlpm_wass_f32(const float *x_dev, int64_t n1, const float *y_dev, int64_t n2, int64_t D, int32_t bins, int32_t has_range,
                             double lo, double hi, int64_t max_bins, void *workspace_dev, int64_t workspace_bytes, int32_t *hist_out_dev,
                             double *out_dev, dlpm_stream_t stream) {
    const int rc = check_shape("dlpm_wass_f32", n1, n2, D, max_bins);
    if (rc != DLPM_OK) return rc;
    DLPM_CHECK_ARG(bins >= 0, "dlpm_wass_f32: bins must be positive, or 0 for numpy's 'auto' rule, got %d", bins);
    DLPM_CHECK_ARG(x_dev && y_dev && workspace_dev && out_dev, "dlpm_wass_f32: null pointer");
    DLPM_CHECK_ARG(reinterpret_cast<uintptr_t>(workspace_dev) % 16 == 0 && reinterpret_cast<uintptr_t>(out_dev) % 8 == 0 &&
                       reinterpret_cast<uintptr_t>(x_dev) % 4 == 0 && reinterpret_cast<uintptr_t>(y_dev) % 4 == 0 &&
                       reinterpret_cast<uintptr_t>(hist_out_dev) % 4 == 0,
                   "dlpm_wass_f32: misaligned pointer");
    const Layout L = layout_of(max_bins);
    const int ws_rc = check_workspace("dlpm_wass_f32", workspace_dev, workspace_bytes, L.total);
    if (ws_rc != DLPM_OK) return ws_rc;
    int range_status = kOk;
    if (has_range) {                                   // _get_outer_edges on Python floats: checks, then the widening, in fp64
        if (lo > hi) range_status = kInvertedRange;
        else if (!(std::isfinite(lo) && std::isfinite(hi))) range_status = kNonFiniteRange;
        else if (lo == hi) {
            lo -= 0.5;
            hi += 0.5;
        }
    }
    hipStream_t st = as_stream(stream);
    char *ws = static_cast<char *>(workspace_dev);
    State *s = reinterpret_cast<State *>(ws + L.state);
    unsigned long long *digits = reinterpret_cast<unsigned long long *>(ws + L.digits);
    int32_t *hist = hist_out_dev ? hist_out_dev : reinterpret_cast<int32_t *>(ws + L.hist);
    const int64_t c1 = n1 * D, c2 = n2 * D;
    const unsigned blocks = (unsigned)std::min<int64_t>(kStreamBlocks, ceil_div(c1 + c2, (int64_t)kThreads * 16));
    const bool automatic = bins == 0;
    const double bytes = 4.0 * (double)(c1 + c2);
    const int lds_bins = automatic ? (int)std::min<int64_t>(max_bins, kLdsBins) : (bins <= kLdsBins ? bins : 0);
    const size_t shmem = std::max<size_t>(16, 2 * (size_t)lds_bins * sizeof(int32_t));
    if (shmem > 48 * 1024) {                                             // before the first launch: a refusal enqueues nothing
        const int r = ensure_dynamic_lds(reinterpret_cast<const void *>(&k_wass_hist), 2 * kLdsBins * (int)sizeof(int32_t));
        if (r != DLPM_OK) return r;
    }

    k_wass_init<<<1, kThreads, 0, st>>>(s, digits);
    DLPM_LAUNCH_CHECK();
    if (automatic || !has_range) {
        ProfScope ps("wass_range", 0.0, bytes, st);
        k_wass_range<<<blocks, kThreads, 0, st>>>(x_dev, c1, y_dev, c2, has_range, lo, hi, s);
        DLPM_LAUNCH_CHECK();
    }
    k_wass_setup<<<1, 1, 0, st>>>(s, bins, has_range, lo, hi, range_status, (int)max_bins, out_dev);
    DLPM_LAUNCH_CHECK();
    if (automatic) {
        ProfScope ps("wass_select", 0.0, 4.0 * bytes, st);
        for (int pass = 0; pass < 4; pass++) {
            k_wass_digits<<<blocks, kThreads, 0, st>>>(x_dev, c1, y_dev, c2, s, digits, pass);
            DLPM_LAUNCH_CHECK();
            k_wass_pick<<<1, kThreads, 0, st>>>(s, digits, pass, has_range, (int)max_bins, out_dev);
            DLPM_LAUNCH_CHECK();
        }
    }
    const int64_t known = automatic ? max_bins : bins;                   // most bins this call can end up with
    k_wass_zero<<<(unsigned)std::min<int64_t>(256, ceil_div(known, kThreads)), kThreads, 0, st>>>(s, hist, max_bins);
    DLPM_LAUNCH_CHECK();
    {
        ProfScope ps("wass_hist", 0.0, bytes, st);
        k_wass_hist<<<blocks, kThreads, shmem, st>>>(x_dev, c1, y_dev, c2, s, hist, max_bins, lds_bins);
        DLPM_LAUNCH_CHECK();
    }
    k_wass_emd<<<1, kThreads, 0, st>>>(s, hist, max_bins, out_dev);
    DLPM_LAUNCH_CHECK();
    return DLPM_OK;
}
