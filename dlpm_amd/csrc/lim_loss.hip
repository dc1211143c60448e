// lim_loss.hip -- the forward half of LIM's objective as an evaluation metric (no backward pass):
//   * k_lim_loss_elements  e, t, x_t = x0 diffusion_coeff(t) + e marginal_std(t) and the target -e / alpha
//                          (GenerativeLevyProcess.py:680-709, LIM/functions/loss.py:12-41, LIM/functions/sde.py)
//   * k_lim_coeffs         the two VPSDE coefficients of a time in fp64, on their own
// The per-sample terms and the estimator are loss.hip's k_loss_terms (smooth-L1) and k_loss_reduce (mean), unchanged.
// HBM/latency bound.  One workgroup owns one sample, so the time, the two coefficients and the heavy-tailed a are wave-uniform:
// thread 0 produces them once, the row is then streamed with 16-byte accesses.
#include "../../include/dlpm_amd_lim.h"
#include "cms.h"
#include "common.h"
#include "philox.h"

using namespace dlpm;

namespace {

// Philox purposes of the LIM loss draws (1-6: the sampler, 7-10: the DLPM loss).  Counter = (global sample, element quad, purpose):
// a sample's draws are a function of (seed, global index) only.
constexpr int kPurposeLimT = 11;   // the time of a sample
constexpr int kPurposeLimA = 12;   // its heavy-tailed a
constexpr int kPurposeLimZ = 13;   // the Gaussian z

// VPSDE(alpha, 'cosine').diffusion_coeff / marginal_std in fp64 from the fp32 time, rounded once.  In fp32 the two logarithms
// below are 6e-8 apart from 0 near t = 1e-5 and their difference is noise (up to 12 % in sigma); fp64 leaves ~1e-9 relative.
__device__ inline void lim_coeffs(float t, double alpha, float &cx, float &sigma) {
    const double pi = 3.141592653589793, s = 0.008;
    const double lm = log(cos(((double)t + s) / (1.0 + s) * pi / 2.0)) - log(cos(s / (1.0 + s) * pi / 2.0));
    cx = (float)exp(lm);
    sigma = (float)pow(-expm1(alpha * lm), 1.0 / alpha);
}

template <bool VEC>
__global__ void __launch_bounds__(256) k_lim_loss_elements(dlpm_lim_loss_args p) {
    __shared__ float s_cx, s_sigma, s_sqrt_a;
    const int64_t b = blockIdx.x;
    const uint64_t gidx = (uint64_t)(p.sample_offset + b);
    const bool gauss = p.alpha == 2.0;
    if (threadIdx.x == 0) {
        float t;
        if (p.t_dev) {
            t = p.t_dev[b];
        } else {
            // torch.rand(n) * (T - 1e-5) + 1e-5: a 24-bit uniform in [0, 1), one fp32 product, one fp32 sum
            const uint4 u = philox4x32_10(make_uint4((uint32_t)gidx, (uint32_t)(gidx >> 32), 0u, kPurposeLimT), p.seed);
            const float U = (float)(u.x >> 8) * (1.0f / 16777216.0f);
            t = __fadd_rn(__fmul_rn(U, (float)(p.t_max - 1e-5)), (float)1e-5);
        }
        float cx, sigma;
        if (p.x_coeff_dev) {
            cx = p.x_coeff_dev[b];
            sigma = p.sigma_dev[b];
        } else {
            lim_coeffs(t, p.alpha, cx, sigma);
        }
        float a = 1.0f;
        if (!p.e_dev && !gauss) a = cms_draw(cms_setup(p.alpha), p.seed, gidx, 0u, kPurposeLimA, 0u);   // gen_sas: no clamp_a
        s_cx = cx;
        s_sigma = sigma;
        s_sqrt_a = (float)sqrt((double)a);      // torch.sqrt: correctly rounded (the fp64 root rounded once)
        p.tvec_out_dev[b] = t;
        if (p.a_out_dev) p.a_out_dev[b] = a;
        if (p.x_coeff_out_dev) p.x_coeff_out_dev[b] = cx;
        if (p.sigma_out_dev) p.sigma_out_dev[b] = sigma;
    }
    __syncthreads();
    const float cx = s_cx, sigma = s_sigma, sqrt_a = s_sqrt_a;
    const float alpha_f = (float)p.alpha, clamp = (float)p.clamp_eps;
    const bool clamped = p.clamp_eps >= 0.0;
    const int64_t D = p.D;
    const float *x0 = p.x0_dev + b * D;
    const float *er = p.e_dev ? p.e_dev + b * D : nullptr;
    float *o_xt = p.x_t_dev + b * D, *o_sc = p.score_dev + b * D, *o_e = p.e_out_dev ? p.e_out_dev + b * D : nullptr;
    constexpr int W = VEC ? 4 : 1;
    const int64_t n = D / W;
    for (int64_t q = threadIdx.x; q < n; q += blockDim.x) {
        float xv[W], ev[W], xt[W], sc[W];
        if (VEC) {
            *reinterpret_cast<float4 *>(xv) = reinterpret_cast<const float4 *>(x0)[q];
            if (er) *reinterpret_cast<float4 *>(ev) = reinterpret_cast<const float4 *>(er)[q];
        } else {
            xv[0] = x0[q];
            if (er) ev[0] = er[q];
        }
        if (!er) {
            const float4 z = philox_normal4(p.seed, gidx, (uint32_t)(VEC ? q : q >> 2), kPurposeLimZ, 0u);
            const float zz[4] = {z.x, z.y, z.z, z.w};
#pragma unroll
            for (int k = 0; k < W; k++) {
                const float zk = zz[VEC ? k : (int)(q & 3)];
                float e = gauss ? zk : __fmul_rn(sqrt_a, zk);                          // Distributions.py:70
                if (clamped) e = e < -clamp ? -clamp : (e > clamp ? clamp : e);        // :72 (a NaN stays a NaN, as torch.clamp)
                ev[k] = e;
            }
        }
#pragma unroll
        for (int k = 0; k < W; k++) {
            xt[k] = __fadd_rn(__fmul_rn(xv[k], cx), __fmul_rn(ev[k], sigma));          // loss.py:24
            sc[k] = gauss ? -ev[k] : -__fdiv_rn(ev[k], alpha_f);                       // loss.py:26-29
        }
        if (VEC) {
            reinterpret_cast<float4 *>(o_xt)[q] = *reinterpret_cast<float4 *>(xt);
            reinterpret_cast<float4 *>(o_sc)[q] = *reinterpret_cast<float4 *>(sc);
            if (o_e) reinterpret_cast<float4 *>(o_e)[q] = *reinterpret_cast<float4 *>(ev);
        } else {
            o_xt[q] = xt[0];
            o_sc[q] = sc[0];
            if (o_e) o_e[q] = ev[0];
        }
    }
}

__global__ void __launch_bounds__(256) k_lim_coeffs(const float *t, int64_t B, double alpha, float *cx, float *sigma) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    float c, s;
    lim_coeffs(t[i], alpha, c, s);
    cx[i] = c;
    sigma[i] = s;
}

bool aligned16(const void *p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

}  // namespace

extern "C" int dlpm_lim_loss_elements_f32(const dlpm_lim_loss_args *a, dlpm_stream_t stream) {
    DLPM_CHECK_ARG(a && a->x0_dev && a->x_t_dev && a->score_dev && a->tvec_out_dev, "dlpm_lim_loss_elements_f32: null pointer");
    DLPM_CHECK_ARG(a->B > 0 && a->B < (1ll << 31) && a->D > 0 && a->D < (1ll << 32), "dlpm_lim_loss_elements_f32: bad shape B=%lld D=%lld",
                   (long long)a->B, (long long)a->D);
    DLPM_CHECK_ARG(a->alpha > 0.0 && a->alpha <= 2.0, "Wrong value of alpha (%g) for skewed levy r.v generation", a->alpha);
    DLPM_CHECK_ARG(a->t_max > 1e-5 && a->t_max < 1.0, "dlpm_lim_loss_elements_f32: t_max must lie in (1e-5, 1), got %g", a->t_max);
    DLPM_CHECK_ARG((a->x_coeff_dev != nullptr) == (a->sigma_dev != nullptr),
                   "dlpm_lim_loss_elements_f32: x_coeff_dev and sigma_dev are given together or not at all");
    const bool vec = (a->D % 4 == 0) && aligned16(a->x0_dev) && aligned16(a->e_dev) && aligned16(a->x_t_dev) && aligned16(a->score_dev) &&
                     aligned16(a->e_out_dev);
    const int64_t items = vec ? a->D / 4 : a->D;
    const unsigned threads = items >= 256 ? 256 : 64;
    // algorithmic bytes: read x0, write x_t and score (+ injected e, + e_out)
    const double per = 3 + (a->e_dev ? 1 : 0) + (a->e_out_dev ? 1 : 0);
    ProfScope ps("lim_loss_elements", 0.0, 4.0 * per * (double)a->B * a->D, as_stream(stream));
    if (vec) k_lim_loss_elements<true><<<(unsigned)a->B, threads, 0, as_stream(stream)>>>(*a);
    else k_lim_loss_elements<false><<<(unsigned)a->B, threads, 0, as_stream(stream)>>>(*a);
    DLPM_LAUNCH_CHECK();
    return DLPM_OK;
}

extern "C" int dlpm_lim_coeffs_f32(const float *t_dev, int64_t B, double alpha, float *x_coeff_dev, float *sigma_dev,
                                   dlpm_stream_t stream) {
    DLPM_CHECK_ARG(t_dev && x_coeff_dev && sigma_dev, "dlpm_lim_coeffs_f32: null pointer");
    DLPM_CHECK_ARG(B > 0 && B < (1ll << 31), "dlpm_lim_coeffs_f32: bad shape B=%lld", (long long)B);
    DLPM_CHECK_ARG(alpha > 0.0 && alpha <= 2.0, "Wrong value of alpha (%g) for skewed levy r.v generation", alpha);
    ProfScope ps("lim_coeffs", 0.0, 12.0 * (double)B, as_stream(stream));
    k_lim_coeffs<<<(unsigned)ceil_div(B, 256), 256, 0, as_stream(stream)>>>(t_dev, B, alpha, x_coeff_dev, sigma_dev);
    DLPM_LAUNCH_CHECK();
    return DLPM_OK;
}
