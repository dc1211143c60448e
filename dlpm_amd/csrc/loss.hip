// loss.hip -- the forward half of the Proposition-9 objective as an evaluation metric (no backward pass):
//   * k_loss_elements  q(x_t | x_0, a) at a per-sample timestep, eps_t and the net input   (dlpm.py:384-401,242-248,198-202,
//                                                                                           GenerativeLevyProcess.py:645-661)
//   * k_loss_terms     one loss term per extended sample                                    (GenerativeLevyProcess.py:19-31)
//   * k_loss_reduce    mean / median-of-means estimator and the non-finite flag             (GenerativeLevyProcess.py:667-677)
// All three are HBM/latency bound.  One workgroup owns one extended sample j = r * B + b, so the timestep, the schedule
// entries and (isotropic noise) the heavy-tailed a are wave-uniform: thread 0 draws them once, the row is then streamed
// with 16-byte accesses.  x_0 is read by index b for every replica r; nothing is repeated in memory.
#include <algorithm>

#include "cms.h"
#include "common.h"
#include "philox.h"

using namespace dlpm;

namespace {

// Philox purposes of the loss draws (1-6 belong to the sampler: noise.hip, philox.h).  Counter = (global sample,
// element quad / element, purpose | replica << 8): a sample's loss is a function of (seed, global index, replica) only.
constexpr int kPurposeLossT = 7;      // the timestep of a sample (shared by its replicas)
constexpr int kPurposeLossA = 8;      // isotropic a, replica r mod outer
constexpr int kPurposeLossAElem = 9;  // non-isotropic a per element, replica r mod outer
constexpr int kPurposeLossZ = 10;     // the Gaussian z, replica r

// (11-13 belong to the LIM loss: lim_loss.hip)

__device__ inline float draw_a(const dlpm_loss_args &p, const Cms &c, uint64_t gidx, uint32_t row, uint32_t purpose, uint32_t rep) {
    if (p.alpha == 2.0) return 2.0f;
    float v = cms_draw(c, p.seed, gidx, row, purpose, rep);
    if (p.clamp_a >= 0.0) v = fminf(fmaxf(v, 0.0f), (float)p.clamp_a);
    return v;
}

// the reference's fp32 operation order, one correctly rounded operation each (no contraction)
__device__ inline void loss_element(float x0, float z, float a, float bg, float bs, float bs2, float isc, bool scaled,
                                    float &x_t, float &eps, float &x_in) {
    const float sig = __fmul_rn(a, bs2);                                        // Sigma' = a_t * bs[t]**2       dlpm.py:392
    // the correctly rounded fp32 square root: the fp64 one rounded once (53 >= 2 * 24 + 2 bits, so the double rounding is
    // innocuous); __fsqrt_rn is the hardware approximation here, 1 ulp off for some inputs
    const float sq = (float)sqrt((double)sig);
    x_t = __fadd_rn(__fmul_rn(bg, x0), __fmul_rn(sq, z));                       // bg[t] x0 + Sigma'**(1/2) z    dlpm.py:247
    eps = __fdiv_rn(__fsub_rn(x_t, __fmul_rn(x0, bg)), bs);                     // predict_eps                   dlpm.py:201
    x_in = scaled ? __fmul_rn(x_t, isc) : x_t;                                  // GenerativeLevyProcess.py:658-661
}

template <bool VEC>
__global__ void __launch_bounds__(256) k_loss_elements(dlpm_loss_args p) {
    __shared__ int s_t;
    __shared__ float s_a;
    const int64_t j = blockIdx.x;            // extended sample
    const int64_t r = j / p.B, b = j - r * p.B;
    const uint32_t ra = (uint32_t)(r % p.outer);          // A is drawn for outer * B samples and repeated `inner` times (:650-651)
    const bool elem = p.flags & DLPM_LOSS_ELEMENTWISE;
    const uint64_t gidx = (uint64_t)(p.sample_offset + b);
    Cms c{};
    if (!p.a_dev && p.alpha != 2.0 && (elem || threadIdx.x == 0)) c = cms_setup(p.alpha);
    if (threadIdx.x == 0) {
        int t;
        if (p.t_dev) {
            t = p.t_dev[b];
        } else {
            // uniform on [1, T-1] (torch.randint(1, T)): the high word of u32 * (T - 1)
            uint4 u = philox4x32_10(make_uint4((uint32_t)gidx, (uint32_t)(gidx >> 32), 0u, kPurposeLossT), p.seed);
            t = 1 + (int)(((uint64_t)u.x * (uint64_t)(p.T - 1)) >> 32);
        }
        t = min(max(t, 0), p.T - 1);         // an injected t outside the table never becomes a read outside it
        s_t = t;
        float a = 0.f;
        if (!elem) {
            a = p.a_dev ? p.a_dev[(int64_t)ra * p.B + b] : draw_a(p, c, gidx, 0u, kPurposeLossA, ra);
            if (p.a_out_dev && r < p.outer) p.a_out_dev[(int64_t)ra * p.B + b] = a;
        }
        s_a = a;
        if (p.t_out_dev && r == 0) p.t_out_dev[b] = t;
        if (p.tvec_out_dev)
            p.tvec_out_dev[j] = (p.flags & DLPM_LOSS_RESCALE_T) ? __fmul_rn((float)t, 1.0f / (float)p.T) : (float)t;
    }
    __syncthreads();
    const int t = s_t;
    const float a_s = s_a;
    const float bg = p.bg_dev[t], bs = p.bs_dev[t], bs2 = __fmul_rn(bs, bs);
    const bool scaled = p.in_scale_dev != nullptr;
    const float isc = scaled ? p.in_scale_dev[t] : 1.0f;
    const int64_t D = p.D;
    const float *x0 = p.x0_dev + b * D;
    const float *zr = p.z_dev ? p.z_dev + j * D : nullptr;
    const float *ar = (elem && p.a_dev) ? p.a_dev + ((int64_t)ra * p.B + b) * D : nullptr;
    float *aor = (elem && p.a_out_dev && r < p.outer) ? p.a_out_dev + ((int64_t)ra * p.B + b) * D : nullptr;
    float *o_in = p.x_in_dev + j * D, *o_eps = p.eps_dev + j * D, *o_xt = p.x_t_dev ? p.x_t_dev + j * D : nullptr;
    constexpr int W = VEC ? 4 : 1;
    const int64_t n = D / W;
    for (int64_t q = threadIdx.x; q < n; q += blockDim.x) {
        float xv[W], zv[W], av[W], xt[W], ev[W], xi[W];
        if (VEC) {
            *reinterpret_cast<float4 *>(xv) = reinterpret_cast<const float4 *>(x0)[q];
            if (zr) *reinterpret_cast<float4 *>(zv) = reinterpret_cast<const float4 *>(zr)[q];
            if (ar) *reinterpret_cast<float4 *>(av) = reinterpret_cast<const float4 *>(ar)[q];
        } else {
            xv[0] = x0[q];
            if (zr) zv[0] = zr[q];
            if (ar) av[0] = ar[q];
        }
        if (!zr) {
            float4 z = philox_normal4(p.seed, gidx, (uint32_t)(VEC ? q : q >> 2), kPurposeLossZ, (uint32_t)r);
            float zz[4] = {z.x, z.y, z.z, z.w};
#pragma unroll
            for (int k = 0; k < W; k++) zv[k] = zz[VEC ? k : (int)(q & 3)];
        }
#pragma unroll
        for (int k = 0; k < W; k++) {
            if (!elem) av[k] = a_s;
            else if (!ar) av[k] = draw_a(p, c, gidx, (uint32_t)(q * W + k), kPurposeLossAElem, ra);
            loss_element(xv[k], zv[k], av[k], bg, bs, bs2, isc, scaled, xt[k], ev[k], xi[k]);
        }
        if (VEC) {
            reinterpret_cast<float4 *>(o_in)[q] = *reinterpret_cast<float4 *>(xi);
            reinterpret_cast<float4 *>(o_eps)[q] = *reinterpret_cast<float4 *>(ev);
            if (o_xt) reinterpret_cast<float4 *>(o_xt)[q] = *reinterpret_cast<float4 *>(xt);
            if (aor) reinterpret_cast<float4 *>(aor)[q] = *reinterpret_cast<float4 *>(av);
        } else {
            o_in[q] = xi[0];
            o_eps[q] = ev[0];
            if (o_xt) o_xt[q] = xt[0];
            if (aor) aor[q] = av[0];
        }
    }
}

__device__ inline float loss_value(float m, float e, int lploss) {
    const float d = __fsub_rn(m, e);
    if (lploss == 1) {                       // smooth-L1, beta = 1
        const float ad = fabsf(d);
        return ad < 1.0f ? __fmul_rn(__fmul_rn(0.5f, d), d) : __fsub_rn(ad, 0.5f);
    }
    return __fmul_rn(d, d);                  // lploss 2 and -1: the squared error
}

// one workgroup per extended sample; each thread adds its strided elements in fp64 in index order, then the tree
template <bool VEC>
__global__ void __launch_bounds__(256) k_loss_terms(const float *model_eps, const float *eps_t, float *out, int64_t B, int64_t D,
                                                    int lploss, int64_t out_stride, int64_t out_offset) {
    __shared__ double sh[256];
    const int64_t j = blockIdx.x;
    const float *m = model_eps + j * D, *e = eps_t + j * D;
    double acc = 0.0;
    if (VEC) {
        const int64_t n = D / 4;
        for (int64_t q = threadIdx.x; q < n; q += 256) {
            const float4 mv = reinterpret_cast<const float4 *>(m)[q], ev = reinterpret_cast<const float4 *>(e)[q];
            acc += (double)loss_value(mv.x, ev.x, lploss);
            acc += (double)loss_value(mv.y, ev.y, lploss);
            acc += (double)loss_value(mv.z, ev.z, lploss);
            acc += (double)loss_value(mv.w, ev.w, lploss);
        }
    } else {
        for (int64_t q = threadIdx.x; q < D; q += 256) acc += (double)loss_value(m[q], e[q], lploss);
    }
    const double sum = block_sum<256>(acc, sh);
    if (threadIdx.x == 0) {
        const double mean = sum / (double)D;
        const int64_t r = j / B, b = j - r * B;
        out[r * out_stride + out_offset + b] = lploss == 2 ? (float)sqrt(mean) : (float)mean;
    }
}

constexpr int kMaxOuter = 64;

// One workgroup, one launch.  mean: all R * N terms.  median: terms viewed as [outer, inner, N] -> fp32 mean over inner ->
// LOWER median over outer (torch.median) -> mean over N.
__global__ void __launch_bounds__(1024) k_loss_reduce(const float *terms, int64_t N, int outer, int inner, int median,
                                                      float *loss_out, int32_t *flag_out, int32_t *med_idx_out) {
    __shared__ double sh[1024];
    __shared__ int s_bad;
    if (threadIdx.x == 0) s_bad = 0;
    __syncthreads();
    const int64_t total = (int64_t)outer * inner * N;
    double acc = 0.0;
    bool bad = false;
    int64_t count;
    if (!median) {
        for (int64_t i = threadIdx.x; i < total; i += 1024) {
            const float v = terms[i];
            bad |= !isfinite(v);
            acc += (double)v;
        }
        count = total;
    } else {
        const int k = (outer - 1) / 2;
        for (int64_t b = threadIdx.x; b < N; b += 1024) {
            float v[kMaxOuter];
            for (int o = 0; o < outer; o++) {
                float s = 0.f;
                for (int i = 0; i < inner; i++) {
                    const float x = terms[((int64_t)o * inner + i) * N + b];
                    bad |= !isfinite(x);
                    s = __fadd_rn(s, x);
                }
                v[o] = __fdiv_rn(s, (float)inner);
            }
            float med = __builtin_nanf("");
            int at = -1;
            for (int o = 0; o < outer; o++) {
                int rank = 0;
                for (int o2 = 0; o2 < outer; o2++) rank += (v[o2] < v[o]) || (v[o2] == v[o] && o2 < o);
                if (rank == k) { med = v[o]; at = o; }
            }
            if (med_idx_out) med_idx_out[b] = at;
            acc += (double)med;
        }
        count = N;
    }
    if (bad) s_bad = 1;          // every writer stores the same value
    const double sum = block_sum<1024>(acc, sh);
    if (threadIdx.x == 0) {
        const float loss = (float)(sum / (double)count);
        *loss_out = loss;
        *flag_out = (s_bad || !isfinite(loss)) ? 1 : 0;
    }
}

// the per-sample-t forms of sample_x_t_from_xstart / predict_eps / predict_xstart (dlpm.py:191-217), reference rounding order
__global__ void __launch_bounds__(256) k_at_t(int mode, const float *u, const float *v, const int32_t *t, const float *bg,
                                              const float *bs, float *out, int64_t B, int64_t D, int T) {
    const int64_t n = B * D;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int tt = min(max(t[i / D], 0), T - 1);
        const float g = bg[tt], s = bs[tt];
        float o;
        if (mode == DLPM_AT_T_Q_SAMPLE) o = __fadd_rn(__fmul_rn(g, u[i]), __fmul_rn(s, v[i]));
        else if (mode == DLPM_AT_T_PREDICT_EPS) o = __fdiv_rn(__fsub_rn(u[i], __fmul_rn(v[i], g)), s);
        else o = __fdiv_rn(__fsub_rn(u[i], __fmul_rn(v[i], s)), g);
        out[i] = o;
    }
}

bool aligned16(const void *p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

}  // namespace

extern "C" int dlpm_loss_elements_f32(const dlpm_loss_args *a, dlpm_stream_t stream) {
    DLPM_CHECK_ARG(a && a->x0_dev && a->bg_dev && a->bs_dev && a->x_in_dev && a->eps_dev, "dlpm_loss_elements_f32: null pointer");
    DLPM_CHECK_ARG(a->B > 0 && a->D > 0 && a->D < (1ll << 32) && a->T >= 2, "dlpm_loss_elements_f32: bad shape B=%lld D=%lld T=%d",
                   (long long)a->B, (long long)a->D, a->T);
    DLPM_CHECK_ARG(a->outer >= 1 && a->inner >= 1 && (int64_t)a->outer * a->inner < (1 << 24),
                   "dlpm_loss_elements_f32: monte_carlo_outer * monte_carlo_inner must be in [1, 2^24)");
    DLPM_CHECK_ARG(a->B * a->outer * a->inner < (1ll << 31), "dlpm_loss_elements_f32: more than 2^31 extended samples");
    DLPM_CHECK_ARG(a->alpha > 0.0 && a->alpha <= 2.0, "Wrong value of alpha (%g) for skewed levy r.v generation", a->alpha);
    const int64_t rows = a->B * a->outer * a->inner;
    const bool vec = (a->D % 4 == 0) && aligned16(a->x0_dev) && aligned16(a->z_dev) && aligned16(a->x_in_dev) &&
                     aligned16(a->eps_dev) && aligned16(a->x_t_dev) &&
                     (!(a->flags & DLPM_LOSS_ELEMENTWISE) || (aligned16(a->a_dev) && aligned16(a->a_out_dev)));
    const int64_t items = vec ? a->D / 4 : a->D;
    const unsigned threads = items >= 256 ? 256 : 64;
    // algorithmic bytes: read x0, write x_in and eps_t (+ x_t, + injected z, + elementwise a)
    const double per = 3 + (a->x_t_dev ? 1 : 0) + (a->z_dev ? 1 : 0) + (((a->flags & DLPM_LOSS_ELEMENTWISE) && a->a_dev) ? 1 : 0);
    ProfScope ps("loss_elements", 0.0, 4.0 * per * (double)rows * a->D, as_stream(stream));
    if (vec) k_loss_elements<true><<<(unsigned)rows, threads, 0, as_stream(stream)>>>(*a);
    else k_loss_elements<false><<<(unsigned)rows, threads, 0, as_stream(stream)>>>(*a);
    DLPM_LAUNCH_CHECK();
    return DLPM_OK;
}

extern "C" int dlpm_loss_terms_f32(const float *model_eps_dev, const float *eps_t_dev, float *terms_dev, int64_t B, int32_t replicas,
                                   int64_t D, int32_t lploss, int64_t out_stride, int64_t out_offset, dlpm_stream_t stream) {
    DLPM_CHECK_ARG(model_eps_dev && eps_t_dev && terms_dev, "dlpm_loss_terms_f32: null pointer");
    DLPM_CHECK_ARG(B > 0 && replicas >= 1 && D > 0 && B * replicas < (1ll << 31), "dlpm_loss_terms_f32: bad shape");
    DLPM_CHECK_ARG(lploss == 2 || lploss == 1 || lploss == -1, "lploss must be 2, 1 or -1, got %d", lploss);
    DLPM_CHECK_ARG(out_offset >= 0 && out_stride >= out_offset + B, "dlpm_loss_terms_f32: [offset, offset + B) outside the row stride");
    const int64_t rows = B * replicas;
    const bool vec = (D % 4 == 0) && aligned16(model_eps_dev) && aligned16(eps_t_dev);
    ProfScope ps("loss_terms", 0.0, 8.0 * (double)rows * D, as_stream(stream));
    if (vec) k_loss_terms<true><<<(unsigned)rows, 256, 0, as_stream(stream)>>>(model_eps_dev, eps_t_dev, terms_dev, B, D, lploss,
                                                                               out_stride, out_offset);
    else k_loss_terms<false><<<(unsigned)rows, 256, 0, as_stream(stream)>>>(model_eps_dev, eps_t_dev, terms_dev, B, D, lploss,
                                                                             out_stride, out_offset);
    DLPM_LAUNCH_CHECK();
    return DLPM_OK;
}

extern "C" int dlpm_loss_reduce_f32(const float *terms_dev, int64_t N, int32_t outer, int32_t inner, int32_t median,
                                    float *loss_dev, int32_t *flag_dev, int32_t *median_index_dev, dlpm_stream_t stream) {
    DLPM_CHECK_ARG(terms_dev && loss_dev && flag_dev, "dlpm_loss_reduce_f32: null pointer");
    DLPM_CHECK_ARG(N > 0 && outer >= 1 && inner >= 1, "dlpm_loss_reduce_f32: bad shape");
    DLPM_CHECK_ARG(!median || outer <= kMaxOuter, "dlpm_loss_reduce_f32: median of means takes monte_carlo_outer <= %d, got %d",
                   kMaxOuter, outer);
    ProfScope ps("loss_reduce", 0.0, 4.0 * (double)N * outer * inner, as_stream(stream));
    k_loss_reduce<<<1, 1024, 0, as_stream(stream)>>>(terms_dev, N, outer, inner, median, loss_dev, flag_dev, median_index_dev);
    DLPM_LAUNCH_CHECK();
    return DLPM_OK;
}

extern "C" int dlpm_at_t_f32(int32_t mode, const float *u_dev, const float *v_dev, const int32_t *t_dev, const float *bg_dev,
                             const float *bs_dev, float *out_dev, int64_t B, int64_t D, int32_t T, dlpm_stream_t stream) {
    DLPM_CHECK_ARG(u_dev && v_dev && t_dev && bg_dev && bs_dev && out_dev, "dlpm_at_t_f32: null pointer");
    DLPM_CHECK_ARG(mode >= DLPM_AT_T_Q_SAMPLE && mode <= DLPM_AT_T_PREDICT_XSTART, "dlpm_at_t_f32: unknown mode %d", mode);
    DLPM_CHECK_ARG(B > 0 && D > 0 && T >= 1, "dlpm_at_t_f32: bad shape");
    const int64_t n = B * D;
    ProfScope ps("at_t", 0.0, 12.0 * (double)n, as_stream(stream));
    k_at_t<<<(unsigned)std::min<int64_t>(ceil_div(n, 256), 256 * 16), 256, 0, as_stream(stream)>>>(mode, u_dev, v_dev, t_dev, bg_dev,
                                                                                               bs_dev, out_dev, B, D, T);
    DLPM_LAUNCH_CHECK();
    return DLPM_OK;
}
