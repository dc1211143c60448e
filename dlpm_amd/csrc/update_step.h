// update_step.h -- the one definition of the sampler's reverse step
//     x <- (x - c_eps eps) / gamma_t + c_noise z        (dlpm.py:272-297, GenerativeLevyProcess.py:225-239)
// for every kernel that carries it: the update kernels (noise.hip), the epilogues of the head convolutions (conv_direct.hip,
// head_fused.hip) and the toy net's one-launch loop (mlp.hip).  Two arithmetic forms:
//   * rows form (row_update4): one quad of one sample, wave-uniform coefficients, the division as a reciprocal multiply plus one
//     Newton step -- the plain stochastic step of the fast kernels;
//   * reference-rounded form (step_exact): the reference's operation order with every product rounded, optional clipping and the
//     DLIM term -- every other variant.
// and what both share: the Philox key / counter rule of the step normals and the history row.
#pragma once
#include "philox.h"

namespace dlpm {

// Philox 'purpose' of the per-step normals of the reverse update (the other purposes live in noise.hip)
constexpr int kPurposeStepZ = 4;

// ---- key and counter rule: the seed, and the GLOBAL index of sample b (a device pair {seed, sample_offset} overrides the launch's)
struct StepKey {
    uint64_t seed, gidx;
};
__device__ __forceinline__ StepKey step_key(const uint64_t *key_dev, uint64_t seed, int64_t sample_offset, int64_t b) {
    return {key_dev ? key_dev[0] : seed, (uint64_t)((key_dev ? (int64_t)key_dev[1] : sample_offset) + b)};
}
// the step normals of element quad `quad` of the key's sample at step t
__device__ __forceinline__ float4 step_philox4(const StepKey &k, uint32_t quad, int t) {
    return philox_normal4(k.seed, k.gidx, quad, kPurposeStepZ, (uint32_t)t);
}
// ... drawn only where the step adds noise
__device__ __forceinline__ float4 step_draw4(const StepKey &k, uint32_t quad, int t, float cn) {
    return (cn != 0.0f) ? step_philox4(k, quad, t) : make_float4(0.f, 0.f, 0.f, 0.f);
}
// ... or the injected normals z[off .. off + 3], where a pointer is given
__device__ __forceinline__ float4 step_normals(const float *z, int64_t off, const StepKey &k, uint32_t quad, int t, float cn) {
    if (z) return *reinterpret_cast<const float4 *>(z + off);
    return step_draw4(k, quad, t, cn);
}

// ---- history row: row T - t of the [T,B,D] buffer whose base sits in a device cell (null cell or null base: no history)
__device__ __forceinline__ float *history_base(float *const *hist_pp) { return hist_pp ? *hist_pp : nullptr; }
__device__ __forceinline__ float *history_row_of(float *base, int T, int t, int64_t B, int64_t b, int64_t D) {
    return base ? base + ((int64_t)(T - t) * B + b) * D : nullptr;
}
__device__ __forceinline__ float *history_row(float *const *hist_pp, int T, int t, int64_t B, int64_t b, int64_t D) {
    return history_row_of(history_base(hist_pp), T, t, B, b, D);
}

// ---- rows form
// a / g as the correctly rounded quotient refined from the reciprocal (one Newton step on the residual; exact except for ties,
// where the reference divides)
__device__ __forceinline__ float div_by(float a, float g, float rg) {
    const float q = a * rg;
    return fmaf(fmaf(-q, g, a), rg, q);
}
struct RowCoeffs {
    float g, rg, ce, cn;   // gamma_t, 1 / gamma_t, c_eps[t,b], c_noise[t,b]
};
__device__ __forceinline__ RowCoeffs row_coeffs(const float *g, const float *c_eps, const float *c_noise, int t, int64_t B, int64_t b) {
    const float gt = g[t];
    return {gt, 1.0f / gt, c_eps[(int64_t)t * B + b], c_noise[(int64_t)t * B + b]};
}
__device__ __forceinline__ float4 row_update4(const float4 &x, const float4 &e, const float4 &z, const RowCoeffs &c) {
    float4 o;
    o.x = fmaf(c.cn, z.x, div_by(x.x - c.ce * e.x, c.g, c.rg));
    o.y = fmaf(c.cn, z.y, div_by(x.y - c.ce * e.y, c.g, c.rg));
    o.z = fmaf(c.cn, z.z, div_by(x.z - c.ce * e.z, c.g, c.rg));
    o.w = fmaf(c.cn, z.w, div_by(x.w - c.ce * e.w, c.g, c.rg));
    return o;
}

// ---- reference-rounded form
struct StepScalars {
    float g, bg, bs, bs_prev;
};
__device__ __forceinline__ StepScalars step_scalars(const float *g, const float *bg, const float *bs, int t) {
    return {g[t], bg[t], bs[t], bs[t > 0 ? t - 1 : 0]};
}
__device__ inline float clip_eps(float x, float e, const StepScalars &c) {
    // predict_xstart -> clamp -> predict_eps (dlpm.py:191-202)
    float xs = __fdiv_rn(x - __fmul_rn(e, c.bs), c.bg);
    xs = fminf(fmaxf(xs, -1.0f), 1.0f);
    return __fdiv_rn(x - __fmul_rn(xs, c.bg), c.bs);
}
// DLIM (dlpm.py:281-297): the mean gains `mean` eps; eta > 0: s' = eta bs_{t-1} scales the noise and
// mean = (bs_{t-1}^alpha - s'^alpha)^(1/alpha) in place of bs_{t-1}
struct DlimCoeffs {
    float mean, sig;
};
__device__ __forceinline__ DlimCoeffs dlim_coeffs(bool dlim, float eta, float alpha, float bs_prev) {
    DlimCoeffs d{bs_prev, 0.f};
    if (dlim && eta != 0.0f) {
        d.sig = eta * bs_prev;
        d.mean = powf(powf(bs_prev, alpha) - powf(d.sig, alpha), 1.0f / alpha);
    }
    return d;
}
// one element; ce / cn: the step's coefficients (c_eps, c_noise; under DLIM bs_t and s' sqrt(A_t))
__device__ __forceinline__ float step_exact(float x, float e, float z, float ce, float cn, const StepScalars &c, bool clip, bool dlim,
                                            float dl_mean) {
    const float ee = clip ? clip_eps(x, e, c) : e;
    float m = __fdiv_rn(x - __fmul_rn(ce, ee), c.g);
    if (dlim) m = __fadd_rn(m, __fmul_rn(dl_mean, ee));
    return __fadd_rn(m, __fmul_rn(cn, z));
}

}  // namespace dlpm
