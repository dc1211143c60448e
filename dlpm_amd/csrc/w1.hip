// w1.hip -- the exact Wasserstein-1 distance between two sets of n points, X [n, D] and Y [n, D] in fp32, each point of mass 1 / n:
//   W = (1 / n) min over permutations s of sum_i c(i, s(i)),
//   c = mean_d |x_d - y_d| (ground 0, 'l1_mean': compute_mean_lploss with lploss = 1, the cost of the manual_compute branch of
//   bem/evaluate/wasserstein.py:23-46) or c = |x - y|_2 (ground 1, 'euclidean').  DESIGN 3.22.
//   * cost pass: c in fp64 from the fp32 inputs, one accumulator per pair, d ascending, every operation rounded on its own; the
//     largest cost by an integer atomicMax on its bit pattern; e = 23 - floor(log2 cmax); q = llrint(c 2^e) as int32 [n][ld], written
//     once.  Rows of D <= 16 values come from registers (with_dt), wider ones from LDS panels of 32 values of both sets.
//   * solver: forward auction with eps-scaling in integers, synchronous (Jacobi) rounds.  Benefits a_ij = -q_ij (n + 1), prices int64
//     from 0, eps_0 = max(1, C / 2), eps_{k+1} = max(1, eps_k / 4), C = qmax (n + 1); a phase starts with everybody unassigned and
//     keeps the prices.  In a round every unassigned person i finds j1 = arg max_j (a_ij - p_j) (lowest j on ties), w2 = the best
//     value over j != j1 (= w1 when n = 1) and bids p_j1 + (w1 - w2) + eps; an object goes to its highest bid (lowest person on ties),
//     its previous owner becomes unassigned, its price the winning bid.  (bid, person) is one 64-bit key under atomicMax
//     (w1_layout.h); integer atomics only.  A bid depends on the prices alone, so prices, rounds, phases and the assignment are a
//     function of the inputs.  Since the benefits are multiples of n + 1 and the last eps is 1, the assignment is optimal for q.
//   * two round kernels with ONE rule (bid_row, finish_round): k_w1_bid (a workgroup per unassigned person) + k_w1_resolve for rounds
//     with many bidders, and k_w1_tail, one workgroup that runs up to kTailRounds rounds of at most tail_threshold bidders per launch.
//     Which of them ran a round changes no bit.  The phase switch and the done flag live in the header on the device; every kernel
//     launched after the end is a no-op; the host enqueues kBatch steps and reads the header once per batch, so the call WAITS ON THE
//     STREAM and cannot be captured in a graph.  The loop is bounded by max_rounds (status 2, W NaN).
//   * value: (1 / n) sum_i c(i, perm[i]) with c recomputed in fp64 by the cost pass's own function, partials in index order, one
//     fixed tree (block_sum).
#include <algorithm>
#include <cmath>

#include "metrics_common.h"
#include "w1_layout.h"
#include "../../include/dlpm_amd_w1.h"

using namespace dlpm;

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 64;                  // the cost kernels write 64 x 64 tiles of q
constexpr int kPanel = 32;                 // values of a row per LDS panel (D > 16)
constexpr int kTailRounds = 512;           // rounds one launch of k_w1_tail runs at the most
constexpr int kBatch = 32;                 // steps the host enqueues between two reads of the header
constexpr unsigned kBidGrid = 1024;        // workgroups of k_w1_bid at the most

struct Header {
    int nonfinite, done, status, phases;
    long long rounds, tail_rounds, max_rounds, eps, qmax;
    unsigned long long cmax_bits;
    int e, count, cur, tail_threshold;      // count persons in list[cur] are unassigned
};
static_assert(sizeof(Header) <= kW1HeaderBytes, "header region");

struct Ws {
    Header *hdr;
    int32_t *q;
    long long *prices;
    unsigned long long *keys;
    int32_t *owner, *assigned, *bidobj, *list[2];
    int64_t n, ld;
};

Ws carve(void *ws, const W1Layout &L, int64_t n) {
    char *b = static_cast<char *>(ws);
    Ws w{};
    w.hdr = reinterpret_cast<Header *>(b + L.hdr);
    w.q = reinterpret_cast<int32_t *>(b + L.q);
    w.prices = reinterpret_cast<long long *>(b + L.prices);
    w.keys = reinterpret_cast<unsigned long long *>(b + L.keys);
    w.owner = reinterpret_cast<int32_t *>(b + L.owner);
    w.assigned = reinterpret_cast<int32_t *>(b + L.assigned);
    w.bidobj = reinterpret_cast<int32_t *>(b + L.bidobj);
    w.list[0] = reinterpret_cast<int32_t *>(b + L.list0);
    w.list[1] = reinterpret_cast<int32_t *>(b + L.list1);
    w.n = n;
    w.ld = L.ld;
    return w;
}

// ---------------------------------------------------------------------------------------------- the cost, one definition
// G = 0: l1_mean, G = 1: euclidean.  acc starts at 0; a pair of zeros (padding) adds exactly 0.
template <int G>
__device__ inline double cost_term(double acc, double xv, double yv) {
    const double d = xv - yv;
    return G == 0 ? acc + fabs(d) : acc + d * d;
}
template <int G>
__device__ inline double cost_finish(double acc, int64_t D) { return G == 0 ? acc / (double)D : sqrt(acc); }

template <int G>
__device__ inline double pair_cost(const float *xr, const float *yr, int64_t D) {
    double acc = 0.0;
    for (int64_t d = 0; d < D; d++) acc = cost_term<G>(acc, (double)xr[d], (double)yr[d]);
    return cost_finish<G>(acc, D);
}

__device__ inline int32_t quantise(double c, int e) { return (int32_t)llrint(ldexp(c, e)); }

// A 64 x 64 tile of costs: thread = (column tid & 63, rows 16 (tid >> 6) ..+15).  WRITE: q = quantise(c); else the tile's largest
// cost joins hdr->cmax_bits (non-negative doubles order as their bit patterns).  Grid (ceil(n / 64), ceil(n / 64)).
template <int G, bool WRITE>
__device__ inline void cost_store(const double (&acc)[16], int64_t D, int64_t n, int64_t ld, int64_t i0, int64_t j, Header *hdr, int32_t *q,
                                  double *sh) {
    const int e = hdr->e;
    double cm = 0.0;
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int64_t i = i0 + r;
        if (i < n && j < n) {
            const double c = cost_finish<G>(acc[r], D);
            if (WRITE) q[i * ld + j] = quantise(c, e);
            else cm = fmax(cm, c);
        }
    }
    if (!WRITE) {
        cm = block_max<kThreads>(cm, sh);
        if (threadIdx.x == 0) atomicMax(&hdr->cmax_bits, (unsigned long long)__double_as_longlong(cm));
    }
}

template <int DT, int G, bool WRITE>
__global__ void __launch_bounds__(kThreads) k_w1_cost_reg(Pts p, Header *hdr, int32_t *q, int64_t ld) {
    __shared__ double sh[kThreads];
    if (hdr->nonfinite) return;
    const int64_t n = p.n1, D = p.D;
    const int64_t j = (int64_t)blockIdx.x * kTile + (threadIdx.x & 63), i0 = (int64_t)blockIdx.y * kTile + (threadIdx.x >> 6) * 16;
    double yv[DT];
#pragma unroll
    for (int d = 0; d < DT; d++) yv[d] = (j < n && d < D) ? (double)p.y[j * D + d] : 0.0;
    double acc[16];
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int64_t i = i0 + r;
        double a = 0.0;
#pragma unroll
        for (int d = 0; d < DT; d++) {
            const double xv = (i < n && j < n && d < D) ? (double)p.x[i * D + d] : 0.0;
            a = cost_term<G>(a, xv, yv[d]);
        }
        acc[r] = a;
    }
    cost_store<G, WRITE>(acc, D, n, ld, i0, j, hdr, q, sh);
}

template <int G, bool WRITE>
__global__ void __launch_bounds__(kThreads) k_w1_cost_lds(Pts p, Header *hdr, int32_t *q, int64_t ld) {
    __shared__ double sh[kThreads];
    __shared__ float xs[kTile][kPanel + 1], ys[kTile][kPanel + 1];
    if (hdr->nonfinite) return;
    const int64_t n = p.n1, D = p.D;
    const int col = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int64_t J0 = (int64_t)blockIdx.x * kTile, I0 = (int64_t)blockIdx.y * kTile;
    double acc[16];
#pragma unroll
    for (int r = 0; r < 16; r++) acc[r] = 0.0;
    for (int64_t d0 = 0; d0 < D; d0 += kPanel) {
#pragma unroll
        for (int k = 0; k < kTile * kPanel / kThreads; k++) {
            const int idx = threadIdx.x + k * kThreads, r = idx >> 5, dd = idx & 31;
            const bool dok = d0 + dd < D;
            xs[r][dd] = (dok && I0 + r < n) ? p.x[(I0 + r) * D + d0 + dd] : 0.0f;
            ys[r][dd] = (dok && J0 + r < n) ? p.y[(J0 + r) * D + d0 + dd] : 0.0f;
        }
        __syncthreads();
        for (int dd = 0; dd < kPanel; dd++) {
            const double yv = (double)ys[col][dd];
#pragma unroll
            for (int r = 0; r < 16; r++) acc[r] = cost_term<G>(acc[r], (double)xs[rg * 16 + r][dd], yv);
        }
        __syncthreads();
    }
    cost_store<G, WRITE>(acc, D, n, ld, I0 + rg * 16, J0 + col, hdr, q, sh);
}

// ---------------------------------------------------------------------------------------------- header
__global__ void k_w1_init(Header *hdr, long long max_rounds, int tail_threshold) {
    Header h{};
    h.max_rounds = max_rounds;
    h.tail_threshold = tail_threshold;
    *hdr = h;
}

// after the cmax pass: the scale exponent, qmax and the first eps; a non-finite input ends the call here (status 1)
__global__ void k_w1_scale(Header *hdr, int64_t n) {
    if (hdr->nonfinite) {
        hdr->status = 1;
        hdr->done = 1;
        return;
    }
    const double cmax = __longlong_as_double((long long)hdr->cmax_bits);
    int e = 0;
    long long qmax = 0;
    if (cmax > 0.0) {
        e = 23 - ilogb(cmax);
        qmax = llrint(ldexp(cmax, e));
    }
    const long long C = qmax * (long long)(n + 1);
    hdr->e = e;
    hdr->qmax = qmax;
    hdr->eps = C / 2 > 1 ? C / 2 : 1;
}

// everybody unassigned, every price 0, phase 1.  Grid ceil(n / 256).
__global__ void __launch_bounds__(kThreads) k_w1_start(Ws w) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < w.n) {
        w.prices[i] = 0;
        w.keys[i] = 0;
        w.owner[i] = -1;
        w.assigned[i] = -1;
        w.bidobj[i] = -1;
        w.list[0][i] = (int32_t)i;
    }
    if (i == 0 && !w.hdr->done) {
        w.hdr->count = (int)w.n;
        w.hdr->cur = 0;
        w.hdr->phases = 1;
    }
}

// ---------------------------------------------------------------------------------------------- one round, one rule
struct Best {
    long long w1, w2;      // the best value and the best value over j != j1
    int j1;
};
constexpr long long kLowest = (long long)0x8000000000000000ull;

__device__ inline void merge(Best &a, long long bw1, int bj1, long long bw2) {
    if (bw1 > a.w1 || (bw1 == a.w1 && bj1 < a.j1)) {
        a.w2 = a.w1 > bw2 ? a.w1 : bw2;
        a.w1 = bw1;
        a.j1 = bj1;
    } else {
        a.w2 = a.w2 > bw1 ? a.w2 : bw1;
    }
}

// The bid of person i, by the whole workgroup: scan row i of q 16 bytes at a time against the prices, reduce (w1, j1, w2) over the
// wave and the four waves, and let thread 0 place the bid.  Ends with a barrier.
__device__ inline void bid_row(const Ws &w, int i, long long eps, Best *sh) {
    const int64_t n = w.n;
    const long long scale = (long long)(n + 1);
    const int4 *row = reinterpret_cast<const int4 *>(w.q + (int64_t)i * w.ld);
    Best b{kLowest, kLowest, 0x7fffffff};
    for (int64_t g = threadIdx.x; g * 4 < n; g += kThreads) {
        const int4 v = row[g];
        const int qs[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int64_t j = g * 4 + k;
            if (j < n) merge(b, -(long long)qs[k] * scale - w.prices[j], (int)j, kLowest);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const long long ow1 = __shfl_down(b.w1, off), ow2 = __shfl_down(b.w2, off);
        const int oj1 = __shfl_down(b.j1, off);
        merge(b, ow1, oj1, ow2);
    }
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = b;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 1; k < kThreads / 64; k++) merge(b, sh[k].w1, sh[k].j1, sh[k].w2);
        const long long w2 = n == 1 ? b.w1 : b.w2;
        const long long bid = w.prices[b.j1] + (b.w1 - w2) + eps;
        atomicMax(&w.keys[b.j1], (unsigned long long)w1_key(bid, i));
        w.bidobj[i] = b.j1;
    }
    __syncthreads();
}

// After every bid of the round has been placed: hand the objects over, build the next list of unassigned persons, count the round,
// and at an empty list end the phase (or the solve).  One workgroup; ends with a barrier.
__device__ inline void finish_round(const Ws &w, bool tail, int *s_next) {
    Header *hdr = w.hdr;
    const int count = hdr->count, cur = hdr->cur;
    const int32_t *list = w.list[cur];
    int32_t *next = w.list[cur ^ 1];
    if (threadIdx.x == 0) *s_next = 0;
    __syncthreads();
    for (int t = threadIdx.x; t < count; t += kThreads) {
        const int i = list[t], j = w.bidobj[i];
        // the keys are written by atomics (at the L2): read them there too, not from a line this CU loaded a round ago
        const unsigned long long key = __hip_atomic_load(&w.keys[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((int)(kW1PersonMask - (long long)(key & (unsigned long long)kW1PersonMask)) == i) {
            const int prev = w.owner[j];
            w.owner[j] = i;
            w.assigned[i] = j;
            w.prices[j] = (long long)(key >> kW1PersonBits);
            if (prev >= 0) {
                w.assigned[prev] = -1;
                next[atomicAdd(s_next, 1)] = prev;
            }
        } else {
            next[atomicAdd(s_next, 1)] = i;
        }
    }
    __syncthreads();
    const int left = *s_next;
    const long long eps = hdr->eps;
    __syncthreads();
    if (left == 0 && eps > 1) {                // the next phase: everybody unassigned again, the prices stay
        for (int64_t i = threadIdx.x; i < w.n; i += kThreads) {
            w.keys[i] = 0;
            w.owner[i] = -1;
            w.assigned[i] = -1;
            next[i] = (int32_t)i;
        }
    }
    if (threadIdx.x == 0) {
        hdr->rounds += 1;
        if (tail) hdr->tail_rounds += 1;
        hdr->cur = cur ^ 1;
        if (left > 0) hdr->count = left;
        else if (eps > 1) {
            hdr->count = (int)w.n;
            hdr->eps = eps / 4 > 1 ? eps / 4 : 1;
            hdr->phases += 1;
        } else {
            hdr->count = 0;
            hdr->done = 1;
        }
    }
    __syncthreads();
}

// whether a round may run: not after the end, and not beyond the cap (which ends the solve with status 2)
__device__ inline bool round_allowed(Header *hdr, bool mark) {
    if (hdr->done) return false;
    if (hdr->rounds >= hdr->max_rounds) {
        if (mark && threadIdx.x == 0) {
            hdr->status = 2;
            hdr->done = 1;
        }
        return false;
    }
    return true;
}

// rounds with more than tail_threshold bidders: a workgroup per bidder, then one workgroup hands over
__global__ void __launch_bounds__(kThreads) k_w1_bid(Ws w) {
    __shared__ Best sh[kThreads / 64];
    Header *hdr = w.hdr;
    const int count = hdr->count;
    if (!round_allowed(hdr, false) || count <= hdr->tail_threshold) return;
    const int32_t *list = w.list[hdr->cur];
    const long long eps = hdr->eps;
    for (int b = blockIdx.x; b < count; b += gridDim.x) bid_row(w, list[b], eps, sh);
}

__global__ void __launch_bounds__(kThreads) k_w1_resolve(Ws w) {
    __shared__ int s_next;
    Header *hdr = w.hdr;
    const bool small = hdr->count <= hdr->tail_threshold;
    if (hdr->done || small) return;
    if (!round_allowed(hdr, true)) return;
    finish_round(w, false, &s_next);
}

// rounds with at most tail_threshold bidders: one workgroup, up to kTailRounds rounds per launch, one row at a time
__global__ void __launch_bounds__(kThreads) k_w1_tail(Ws w) {
    __shared__ Best sh[kThreads / 64];
    __shared__ int s_next;
    Header *hdr = w.hdr;
    for (int it = 0; it < kTailRounds; it++) {
        const int count = hdr->count;
        const bool small = count <= hdr->tail_threshold;
        if (hdr->done || !small) break;
        const bool go = round_allowed(hdr, true);
        if (!go) break;
        const int32_t *list = w.list[hdr->cur];
        const long long eps = hdr->eps;
        for (int b = 0; b < count; b++) bid_row(w, list[b], eps, sh);
        finish_round(w, true, &s_next);
    }
}

// ---------------------------------------------------------------------------------------------- the value
template <int G>
__global__ void __launch_bounds__(kThreads) k_w1_value(Pts p, Ws w, int32_t *perm_out, long long *prices_out, double *out) {
    __shared__ double sh[kThreads];
    __shared__ unsigned long long s_q;
    Header *hdr = w.hdr;
    const int64_t n = w.n;
    const int status = hdr->done ? hdr->status : 2;
    if (threadIdx.x == 0) s_q = 0;
    __syncthreads();
    double acc = 0.0;
    unsigned long long qs = 0;
    for (int64_t i = threadIdx.x; i < n; i += kThreads) {
        const int j = w.assigned[i];
        if (perm_out) perm_out[i] = j;
        if (prices_out) prices_out[i] = w.prices[i];
        if (status == 0) {
            acc += pair_cost<G>(p.x + i * p.D, p.y + (int64_t)j * p.D, p.D);
            qs += (unsigned long long)w.q[i * w.ld + j];
        }
    }
    atomicAdd(&s_q, qs);
    const double total = block_sum<kThreads>(acc, sh);
    if (threadIdx.x == 0) {
        const bool ok = status == 0;
        out[0] = ok ? total / (double)n : __longlong_as_double(0x7ff8000000000000ll);
        out[1] = ok ? (double)s_q : 0.0;
        out[2] = (double)hdr->e;
        out[3] = (double)hdr->rounds;
        out[4] = (double)hdr->phases;
        out[5] = status == 1 ? __longlong_as_double(0x7ff8000000000000ll) : __longlong_as_double((long long)hdr->cmax_bits);
        out[6] = (double)status;
        out[7] = (double)hdr->tail_rounds;
    }
}

// ---------------------------------------------------------------------------------------------- host
int check_shape(const char *who, int64_t n, int64_t D) {
    DLPM_CHECK_ARG(n >= 1 && n <= kW1MaxN, "%s: n must be in [1, %lld], got %lld", who, (long long)kW1MaxN, (long long)n);
    DLPM_CHECK_ARG(D >= 1 && D <= kW1MaxD, "%s: D must be in [1, %lld], got %lld", who, (long long)kW1MaxD, (long long)D);
    return DLPM_OK;
}

template <int G, bool WRITE>
void launch_cost(const Pts &p, const Ws &w, hipStream_t st) {
    const unsigned T = (unsigned)ceil_div(p.n1, kTile);
    const dim3 grid(T, T);
    if (p.D <= 16) {
        with_dt(p.D, [&](auto dt) {
            constexpr int DT = decltype(dt)::value;
            k_w1_cost_reg<DT, G, WRITE><<<grid, kThreads, 0, st>>>(p, w.hdr, w.q, w.ld);
        });
    } else {
        k_w1_cost_lds<G, WRITE><<<grid, kThreads, 0, st>>>(p, w.hdr, w.q, w.ld);
    }
}

template <int G>
int run(const Pts &p, const Ws &w, int64_t max_rounds, int64_t tail_threshold, int32_t *perm_out, long long *prices_out, double *out,
        hipStream_t st) {
    const int64_t n = p.n1;
    const int thr = (int)std::min<int64_t>(tail_threshold, n);
    k_w1_init<<<1, 1, 0, st>>>(w.hdr, (long long)max_rounds, thr);
    DLPM_LAUNCH_CHECK();
    k_nonfinite<256><<<scan_grid(p.n * p.D), 256, 0, st>>>(p, &w.hdr->nonfinite);
    DLPM_LAUNCH_CHECK();
    {
        ProfScope ps("w1_cost", 6.0 * (double)n * n * p.D, 4.0 * (double)n * n, st);
        launch_cost<G, false>(p, w, st);
        DLPM_LAUNCH_CHECK();
        k_w1_scale<<<1, 1, 0, st>>>(w.hdr, n);
        DLPM_LAUNCH_CHECK();
        launch_cost<G, true>(p, w, st);
        DLPM_LAUNCH_CHECK();
    }
    k_w1_start<<<(unsigned)ceil_div(n, kThreads), kThreads, 0, st>>>(w);
    DLPM_LAUNCH_CHECK();
    {
        ProfScope ps("w1_auction", 0.0, 0.0, st);
        const unsigned bid_grid = (unsigned)std::min<int64_t>(n, kBidGrid);
        // every step runs at least one round unless the solve has ended, so max_rounds / kBatch + 1 batches reach the cap at the latest
        const int64_t batches = max_rounds / kBatch + 2;
        for (int64_t b = 0; b < batches; b++) {
            for (int s = 0; s < kBatch; s++) {
                if (thr > 0) k_w1_tail<<<1, kThreads, 0, st>>>(w);
                if (thr < n) {
                    k_w1_bid<<<bid_grid, kThreads, 0, st>>>(w);
                    k_w1_resolve<<<1, kThreads, 0, st>>>(w);
                }
            }
            DLPM_LAUNCH_CHECK();
            Header h{};
            DLPM_HIP(hipMemcpyAsync(&h, w.hdr, sizeof(Header), hipMemcpyDeviceToHost, st));
            DLPM_HIP(hipStreamSynchronize(st));
            if (h.done) break;
        }
    }
    k_w1_value<G><<<1, kThreads, 0, st>>>(p, w, perm_out, prices_out, out);
    DLPM_LAUNCH_CHECK();
    return DLPM_OK;
}

}  // namespace

extern "C" int64_t dlpm_w1_workspace_bytes(int64_t n, int64_t D) {
    const int rc = check_shape("dlpm_w1_workspace_bytes", n, D);
    if (rc != DLPM_OK) return rc;
    return w1_layout_of<Carve>(n).total;
}

extern "C" int dlpm_w1_f32(const float *x_dev, const float *y_dev, int64_t n, int64_t D, int32_t ground, int64_t max_rounds,
                           int64_t tail_threshold, void *workspace_dev, int64_t workspace_bytes, int32_t *perm_out_dev,
                           int64_t *prices_out_dev, double *out_dev, dlpm_stream_t stream) {
    const int rc = check_shape("dlpm_w1_f32", n, D);
    if (rc != DLPM_OK) return rc;
    DLPM_CHECK_ARG(ground == DLPM_W1_L1_MEAN || ground == DLPM_W1_EUCLIDEAN, "dlpm_w1_f32: unknown ground %d", (int)ground);
    DLPM_CHECK_ARG(max_rounds >= 1, "dlpm_w1_f32: max_rounds must be at least 1, got %lld", (long long)max_rounds);
    DLPM_CHECK_ARG(tail_threshold >= 0, "dlpm_w1_f32: tail_threshold must not be negative, got %lld", (long long)tail_threshold);
    DLPM_CHECK_ARG(x_dev && y_dev && workspace_dev && out_dev, "dlpm_w1_f32: null pointer");
    DLPM_CHECK_ARG(aligned(x_dev, 4) && aligned(y_dev, 4) && aligned(out_dev, 8) && aligned(perm_out_dev, 4) && aligned(prices_out_dev, 8),
                   "dlpm_w1_f32: misaligned input or output");
    const W1Layout L = w1_layout_of<Carve>(n);
    const int ws_rc = check_workspace("dlpm_w1_f32", workspace_dev, workspace_bytes, L.total);
    if (ws_rc != DLPM_OK) return ws_rc;
    const Ws w = carve(workspace_dev, L, n);
    const Pts p{x_dev, y_dev, n, 2 * n, D};
    long long *prices_out = reinterpret_cast<long long *>(prices_out_dev);
    hipStream_t st = as_stream(stream);
    return ground == DLPM_W1_L1_MEAN ? run<0>(p, w, max_rounds, tail_threshold, perm_out_dev, prices_out, out_dev, st)
                                     : run<1>(p, w, max_rounds, tail_threshold, perm_out_dev, prices_out, out_dev, st);
}
