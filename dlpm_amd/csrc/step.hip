// step.hip -- the step-level kernels (include/dlpm_amd_step.h):
//   * k_anterior   the moments of one reverse step as outputs          (dlpm.py:250-297)
//   * k_two_rv     the Proposition-8 loss elements at a per-sample t   (dlpm.py:308-370)
// Both are HBM bound.  One workgroup owns one sample, so the timestep, the schedule entries and (isotropic noise) the table
// entries are wave-uniform: they are formed once per row, then the row is streamed with 16-byte accesses (VEC: D % 4 == 0 and
// aligned pointers) or element by element.  No atomics; every output element has one writer.
#include "../../include/dlpm_amd_step.h"
#include "cms.h"
#include "common.h"
#include "philox.h"

using namespace dlpm;

namespace {

// Philox purposes of the two-rv draws (1-6: the sampler, 7-10: the DLPM loss, 11-13: the LIM loss, 14-17: the toy data).
// Counter = (global sample, element quad / element, purpose | which << 8) with which = 0 for a_{t,0} and 1 for a_{t,1}.
constexpr int kPurposeTwoRvA = 18;      // isotropic a
constexpr int kPurposeTwoRvAElem = 19;  // non-isotropic a per element
constexpr int kPurposeTwoRvZ = 20;      // the Gaussian z

bool aligned16(const void *p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

// Gamma = 1 - (g^2 Sigma_{t-1}) / Sigma_t and var = Gamma Sigma_{t-1}, the reference's rounding order (dlpm.py:253,257)
__device__ inline void gamma_var(float g2, float sig_prev, float sig, float &gam, float &var) {
    gam = __fsub_rn(1.0f, __fdiv_rn(__fmul_rn(g2, sig_prev), sig));
    var = __fmul_rn(gam, sig_prev);
}

template <bool VEC>
__global__ void __launch_bounds__(256) k_anterior(dlpm_anterior_args p) {
    constexpr int W = VEC ? 4 : 1;
    const int64_t b = blockIdx.x, D = p.D;
    const int t = min(max(*p.t_dev, 1), p.T - 1);            // a t outside the tables never becomes a read outside them
    const float g = p.g_dev[t], bs = p.bs_dev[t], bs_prev = p.bs_dev[t - 1];
    const float g2 = __fmul_rn(g, g);
    const bool elem = p.flags & DLPM_UPD_ELEMENTWISE, dlim = p.mode == DLPM_ANT_DLIM;
    const int64_t n = elem ? p.B * D : p.B;
    // the row's scalars: ce multiplies eps inside the quotient, add multiplies eps after it (DLIM), var_s is the variance
    float ce = bs, add = bs_prev, var_s = 0.0f, sig2 = 0.0f;
    if (dlim && p.eta != 0.0f) {
        const float sp = __fmul_rn(p.eta, bs_prev);                                                 // sigma_t = eta bs[t-1]   :289
        add = powf(__fsub_rn(powf(bs_prev, p.alpha), powf(sp, p.alpha)), 1.0f / p.alpha);          // :292
        sig2 = t != 1 ? __fmul_rn(sp, sp) : 0.0f;                                                   // mask sigma_t^2          :295
        if (!elem) var_s = __fmul_rn(sig2, p.A_dev[(int64_t)t * n + b]);
    } else if (!dlim && !elem) {
        float gam;
        gamma_var(g2, p.Sigmas_dev[(int64_t)(t - 1) * n + b], p.Sigmas_dev[(int64_t)t * n + b], gam, var_s);
        ce = __fmul_rn(bs, gam);                                                                    // bs[t] Gamma_t           :276
    }
    if (!elem && p.var_dev && threadIdx.x == 0) p.var_dev[b] = var_s;
    const float *xr = p.x_dev + b * D, *er = p.eps_dev + b * D;
    float *mr = p.mean_dev + b * D;
    float *vr = (elem && p.var_dev) ? p.var_dev + b * D : nullptr;
    const float *sp_r = (elem && !dlim) ? p.Sigmas_dev + (int64_t)(t - 1) * n + b * D : nullptr;
    const float *sc_r = (elem && !dlim) ? p.Sigmas_dev + (int64_t)t * n + b * D : nullptr;
    const float *a_r = (elem && dlim && p.eta != 0.0f) ? p.A_dev + (int64_t)t * n + b * D : nullptr;
    const int64_t items = D / W;
    for (int64_t q = threadIdx.x; q < items; q += blockDim.x) {
        float xv[W], ev[W], s0[W], s1[W], av[W], m[W], v[W];
        if (VEC) {
            *reinterpret_cast<float4 *>(xv) = reinterpret_cast<const float4 *>(xr)[q];
            *reinterpret_cast<float4 *>(ev) = reinterpret_cast<const float4 *>(er)[q];
            if (sp_r) {
                *reinterpret_cast<float4 *>(s0) = reinterpret_cast<const float4 *>(sp_r)[q];
                *reinterpret_cast<float4 *>(s1) = reinterpret_cast<const float4 *>(sc_r)[q];
            }
            if (a_r) *reinterpret_cast<float4 *>(av) = reinterpret_cast<const float4 *>(a_r)[q];
        } else {
            xv[0] = xr[q];
            ev[0] = er[q];
            if (sp_r) { s0[0] = sp_r[q]; s1[0] = sc_r[q]; }
            if (a_r) av[0] = a_r[q];
        }
#pragma unroll
        for (int k = 0; k < W; k++) {
            float c = ce;
            v[k] = var_s;
            if (sp_r) {
                float gam;
                gamma_var(g2, s0[k], s1[k], gam, v[k]);
                c = __fmul_rn(bs, gam);
            } else if (a_r) {
                v[k] = __fmul_rn(sig2, av[k]);
            }
            m[k] = __fdiv_rn(__fsub_rn(xv[k], __fmul_rn(c, ev[k])), g);
            if (dlim) m[k] = __fadd_rn(m[k], __fmul_rn(add, ev[k]));
        }
        if (VEC) {
            reinterpret_cast<float4 *>(mr)[q] = *reinterpret_cast<float4 *>(m);
            if (vr) reinterpret_cast<float4 *>(vr)[q] = *reinterpret_cast<float4 *>(v);
        } else {
            mr[q] = m[0];
            if (vr) vr[q] = v[0];
        }
    }
}

struct TwoRv {
    float sp1, sp, gam, sig_tilde, lam;
};

// the [n] constants of Proposition 8 from one (a0, a1) pair, the reference's rounding order (dlpm.py:327-331,253,257,352)
__device__ inline TwoRv two_rv_consts(float a0, float a1, float g, float s, float bs, float bs_prev) {
    TwoRv r;
    const float g2 = __fmul_rn(g, g);
    r.sp1 = __fmul_rn(__fmul_rn(bs_prev, bs_prev), a0);                              // bs[t-1]**2 * a_t_0
    r.sp = __fadd_rn(__fmul_rn(__fmul_rn(s, s), a1), __fmul_rn(g2, r.sp1));          // s[t]**2 * a_t_1 + g[t]**2 * Sigma'_{t-1}
    gamma_var(g2, r.sp1, r.sp, r.gam, r.sig_tilde);
    r.lam = __fdiv_rn(bs, __fmul_rn(__fmul_rn(2.0f, g), r.sp1));                     // bs[t] / (2 * g[t] * Sigma'_{t-1})
    return r;
}

__device__ inline float two_rv_draw(const dlpm_two_rv_args &p, const Cms &c, uint64_t gidx, uint32_t row, uint32_t purpose,
                                    uint32_t which) {
    if (p.alpha == 2.0) return 2.0f;
    float v = cms_draw(c, p.seed, gidx, row, purpose, which);
    if (p.clamp_a >= 0.0) v = fminf(fmaxf(v, 0.0f), (float)p.clamp_a);
    return v;
}

template <bool VEC>
__global__ void __launch_bounds__(256) k_two_rv(dlpm_two_rv_args p) {
    constexpr int W = VEC ? 4 : 1;
    __shared__ float s_a[2];
    const int64_t b = blockIdx.x, D = p.D;
    const bool elem = p.flags & DLPM_LOSS_ELEMENTWISE;
    const uint64_t gidx = (uint64_t)(p.sample_offset + b);
    const int t = min(max(p.t_dev[b], 1), p.T - 1);          // a t outside the tables never becomes a read outside them
    const float g = p.g_dev[t], bg = p.bg_dev[t], s = p.s_dev[t], bs = p.bs_dev[t], bs_prev = p.bs_dev[t - 1];
    Cms c{};
    if (!p.a0_dev && p.alpha != 2.0 && (elem || threadIdx.x == 0)) c = cms_setup(p.alpha);
    TwoRv r{};
    float sq = 0.0f, ce = 0.0f;
    if (!elem) {
        if (threadIdx.x == 0) {              // one draw per row, shared through LDS: a CMS draw costs two fp64 pow
            float a0 = p.a0_dev ? p.a0_dev[b] : two_rv_draw(p, c, gidx, 0u, kPurposeTwoRvA, 0u);
            const float a1 = p.a1_dev ? p.a1_dev[b] : two_rv_draw(p, c, gidx, 0u, kPurposeTwoRvA, 1u);
            if (t == 1) a0 = 0.0f;           // zero variance when t == 1 (:310-316)
            s_a[0] = a0;
            s_a[1] = a1;
        }
        __syncthreads();
        r = two_rv_consts(s_a[0], s_a[1], g, s, bs, bs_prev);
        // Sigma'**(1/2) as the correctly rounded fp32 root (the fp64 one rounded once), as k_loss_elements takes it
        sq = (float)sqrt((double)r.sp);
        ce = __fmul_rn(bs, r.gam);
        if (threadIdx.x == 0) {
            if (p.Sigma_tilde_dev) p.Sigma_tilde_dev[b] = r.sig_tilde;
            if (p.lambda_dev) p.lambda_dev[b] = r.lam;
            if (p.Sigma_prime_t_1_dev) p.Sigma_prime_t_1_dev[b] = r.sp1;
            if (p.Sigma_prime_t_dev) p.Sigma_prime_t_dev[b] = r.sp;
            if (p.Gamma_prime_dev) p.Gamma_prime_dev[b] = r.gam;
            if (p.a0_out_dev) p.a0_out_dev[b] = s_a[0];
            if (p.a1_out_dev) p.a1_out_dev[b] = s_a[1];
        }
    }
    const int64_t row = b * D;
    const float *x0 = p.x0_dev + row;
    const float *zr = p.z_dev ? p.z_dev + row : nullptr;
    const float *a0r = (elem && p.a0_dev) ? p.a0_dev + row : nullptr;
    const float *a1r = (elem && p.a1_dev) ? p.a1_dev + row : nullptr;
    float *outs[3] = {p.x_t_dev, p.eps_t_dev, p.m_tilde_dev};
    float *nouts[7] = {p.Sigma_tilde_dev, p.lambda_dev, p.Sigma_prime_t_1_dev, p.Sigma_prime_t_dev, p.Gamma_prime_dev,
                       p.a0_out_dev, p.a1_out_dev};
    const int64_t items = D / W;
    for (int64_t q = threadIdx.x; q < items; q += blockDim.x) {
        float xv[W], zv[W], a0v[W], a1v[W], o[3][W], no[7][W];
        if (VEC) {
            *reinterpret_cast<float4 *>(xv) = reinterpret_cast<const float4 *>(x0)[q];
            if (zr) *reinterpret_cast<float4 *>(zv) = reinterpret_cast<const float4 *>(zr)[q];
            if (a0r) {
                *reinterpret_cast<float4 *>(a0v) = reinterpret_cast<const float4 *>(a0r)[q];
                *reinterpret_cast<float4 *>(a1v) = reinterpret_cast<const float4 *>(a1r)[q];
            }
        } else {
            xv[0] = x0[q];
            if (zr) zv[0] = zr[q];
            if (a0r) { a0v[0] = a0r[q]; a1v[0] = a1r[q]; }
        }
        if (!zr) {
            const float4 z = philox_normal4(p.seed, gidx, (uint32_t)(VEC ? q : q >> 2), kPurposeTwoRvZ, 0u);
            const float zz[4] = {z.x, z.y, z.z, z.w};
#pragma unroll
            for (int k = 0; k < W; k++) zv[k] = zz[VEC ? k : (int)(q & 3)];
        }
#pragma unroll
        for (int k = 0; k < W; k++) {
            float sqk = sq, cek = ce;
            if (elem) {
                const uint32_t e = (uint32_t)(q * W + k);
                float a0 = a0r ? a0v[k] : two_rv_draw(p, c, gidx, e, kPurposeTwoRvAElem, 0u);
                const float a1 = a0r ? a1v[k] : two_rv_draw(p, c, gidx, e, kPurposeTwoRvAElem, 1u);
                if (t == 1) a0 = 0.0f;
                const TwoRv re = two_rv_consts(a0, a1, g, s, bs, bs_prev);
                sqk = (float)sqrt((double)re.sp);
                cek = __fmul_rn(bs, re.gam);
                no[0][k] = re.sig_tilde; no[1][k] = re.lam; no[2][k] = re.sp1; no[3][k] = re.sp; no[4][k] = re.gam;
                no[5][k] = a0; no[6][k] = a1;
            }
            const float xt = __fadd_rn(__fmul_rn(bg, xv[k]), __fmul_rn(sqk, zv[k]));           // bg[t] x0 + Sigma'**(1/2) z    :247
            const float ep = __fdiv_rn(__fsub_rn(xt, __fmul_rn(xv[k], bg)), bs);               // predict_eps                   :201
            o[0][k] = xt;
            o[1][k] = ep;
            o[2][k] = __fdiv_rn(__fsub_rn(xt, __fmul_rn(cek, ep)), g);                         // compute_m_tilde_t_1           :262
        }
#pragma unroll
        for (int j = 0; j < 3; j++) {
            if (!outs[j]) continue;
            if (VEC) reinterpret_cast<float4 *>(outs[j] + row)[q] = *reinterpret_cast<float4 *>(o[j]);
            else outs[j][row + q] = o[j][0];
        }
        if (elem) {
#pragma unroll
            for (int j = 0; j < 7; j++) {
                if (!nouts[j]) continue;
                if (VEC) reinterpret_cast<float4 *>(nouts[j] + row)[q] = *reinterpret_cast<float4 *>(no[j]);
                else nouts[j][row + q] = no[j][0];
            }
        }
    }
}

}  // namespace

extern "C" int dlpm_anterior_f32(const dlpm_anterior_args *a, dlpm_stream_t stream) {
    DLPM_CHECK_ARG(a && a->x_dev && a->eps_dev && a->t_dev && a->g_dev && a->bs_dev && a->mean_dev, "dlpm_anterior_f32: null pointer");
    DLPM_CHECK_ARG(a->B > 0 && a->B < (1ll << 31) && a->D > 0 && a->T >= 2, "dlpm_anterior_f32: bad shape B=%lld D=%lld T=%d",
                   (long long)a->B, (long long)a->D, a->T);
    DLPM_CHECK_ARG(a->mode == DLPM_ANT_DLPM || a->mode == DLPM_ANT_DLIM, "dlpm_anterior_f32: unknown mode %d", a->mode);
    DLPM_CHECK_ARG((a->flags & ~DLPM_UPD_ELEMENTWISE) == 0, "dlpm_anterior_f32: unknown flag in %d", a->flags);
    if (a->mode == DLPM_ANT_DLPM) DLPM_CHECK_ARG(a->Sigmas_dev, "dlpm_anterior_f32: the DLPM moments need Sigmas");
    else if (a->eta != 0.0f) DLPM_CHECK_ARG(a->A_dev, "dlpm_anterior_f32: DLIM with eta > 0 needs A");
    const bool elem = a->flags & DLPM_UPD_ELEMENTWISE;
    const bool vec = (a->D % 4 == 0) && aligned16(a->x_dev) && aligned16(a->eps_dev) && aligned16(a->mean_dev) &&
                     (!elem || (aligned16(a->Sigmas_dev) && aligned16(a->A_dev) && aligned16(a->var_dev)));
    const int64_t items = vec ? a->D / 4 : a->D;
    const unsigned threads = items >= 256 ? 256 : 64;
    // algorithmic bytes: read x and eps, write mean (+ elementwise: two table rows or one, and var)
    const double per = 3 + (elem ? (a->mode == DLPM_ANT_DLPM ? 2 : (a->eta != 0.0f ? 1 : 0)) + (a->var_dev ? 1 : 0) : 0);
    ProfScope ps("anterior", 0.0, 4.0 * per * (double)a->B * a->D, as_stream(stream));
    if (vec) k_anterior<true><<<(unsigned)a->B, threads, 0, as_stream(stream)>>>(*a);
    else k_anterior<false><<<(unsigned)a->B, threads, 0, as_stream(stream)>>>(*a);
    DLPM_LAUNCH_CHECK();
    return DLPM_OK;
}

extern "C" int dlpm_two_rv_elements_f32(const dlpm_two_rv_args *a, dlpm_stream_t stream) {
    DLPM_CHECK_ARG(a && a->x0_dev && a->t_dev && a->g_dev && a->bg_dev && a->s_dev && a->bs_dev, "dlpm_two_rv_elements_f32: null pointer");
    DLPM_CHECK_ARG(a->B > 0 && a->B < (1ll << 31) && a->D > 0 && a->D < (1ll << 32) && a->T >= 2,
                   "dlpm_two_rv_elements_f32: bad shape B=%lld D=%lld T=%d", (long long)a->B, (long long)a->D, a->T);
    DLPM_CHECK_ARG(a->alpha > 0.0 && a->alpha <= 2.0, "Wrong value of alpha (%g) for skewed levy r.v generation", a->alpha);
    DLPM_CHECK_ARG((a->a0_dev == nullptr) == (a->a1_dev == nullptr), "dlpm_two_rv_elements_f32: a0 and a1 are given together or not at all");
    DLPM_CHECK_ARG((a->flags & ~DLPM_LOSS_ELEMENTWISE) == 0, "dlpm_two_rv_elements_f32: unknown flag in %d", a->flags);
    const bool elem = a->flags & DLPM_LOSS_ELEMENTWISE;
    const void *rows[] = {a->x0_dev, a->z_dev, a->x_t_dev, a->eps_t_dev, a->m_tilde_dev};
    const void *cols[] = {a->a0_dev, a->a1_dev, a->Sigma_tilde_dev, a->lambda_dev, a->Sigma_prime_t_1_dev, a->Sigma_prime_t_dev,
                          a->Gamma_prime_dev, a->a0_out_dev, a->a1_out_dev};
    bool vec = a->D % 4 == 0;
    for (const void *q : rows) vec = vec && aligned16(q);
    if (elem) for (const void *q : cols) vec = vec && aligned16(q);
    const int64_t items = vec ? a->D / 4 : a->D;
    const unsigned threads = items >= 256 ? 256 : 64;
    double per = 1 + (a->z_dev ? 1 : 0) + (a->x_t_dev ? 1 : 0) + (a->eps_t_dev ? 1 : 0) + (a->m_tilde_dev ? 1 : 0);
    if (elem) for (const void *q : cols) per += q ? 1 : 0;
    ProfScope ps("two_rv_elements", 0.0, 4.0 * per * (double)a->B * a->D, as_stream(stream));
    if (vec) k_two_rv<true><<<(unsigned)a->B, threads, 0, as_stream(stream)>>>(*a);
    else k_two_rv<false><<<(unsigned)a->B, threads, 0, as_stream(stream)>>>(*a);
    DLPM_LAUNCH_CHECK();
    return DLPM_OK;
}
