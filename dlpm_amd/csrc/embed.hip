// embed.hip -- sinusoidal timestep embedding, [cos | sin] halves (dlpm/models/nn.py:103-121).
// t arrives already divided by T (GenerativeLevyProcess._scale_timesteps, :92-96).
// Also the label term of a class-conditional net: emb = time_embed(t) + label_emb(y) (unet.py:470-473).
#include "conv.h"

namespace dlpm {
namespace {

__global__ void k_timestep_embedding(const float *__restrict__ t, float *__restrict__ emb, int64_t B, int dim) {
    const int half = dim / 2;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * dim) return;
    const int64_t b = i / dim;
    const int j = (int)(i - b * dim);
    float v = 0.f;  // odd dim: trailing zero column
    if (j < 2 * half) {
        const int k = (j < half) ? j : j - half;
        // freqs = exp(-ln(10000) * arange(half) / half), every op rounded to fp32 as torch does
        const float f = expf(__fdiv_rn(__fmul_rn(-9.210340371976184f, (float)k), (float)half));
        const float ang = __fmul_rn(t[b], f);
        v = (j < half) ? cosf(ang) : sinf(ang);
    }
    emb[i] = v;
}

// out[b][j] = src[row(b)][j] + w[y[b]][j], row(b) = (row_dev ? *row_dev : 0) + b * src_row_stride: per-sample rows (stride 1),
// one shared row (stride 0), or the row of a [T][dim] table picked by the device step counter (row_dev, stride 0).
// A label outside [0, K) never indexes w: its sample's row is NaN.
__global__ void k_label_embedding_add(const float *__restrict__ src, const int32_t *__restrict__ row_dev, int src_row_stride,
                                      const float *__restrict__ w, const int64_t *__restrict__ y, int64_t K, int64_t B, int dim,
                                      float *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * dim) return;
    const int64_t b = i / dim;
    const int j = (int)(i - b * dim);
    const int64_t row = (row_dev ? (int64_t)*row_dev : 0) + b * src_row_stride;
    const int64_t c = y[b];
    out[i] = (c >= 0 && c < K) ? __fadd_rn(src[row * dim + j], w[c * dim + j]) : __builtin_nanf("");
}

}  // namespace

int launch_label_embedding_add(const float *src, const int32_t *row_dev, int src_row_stride, const float *w, const int64_t *y, int64_t K,
                               int64_t B, int dim, float *out, hipStream_t st) {
    k_label_embedding_add<<<(unsigned)ceil_div(B * dim, 256), 256, 0, st>>>(src, row_dev, src_row_stride, w, y, K, B, dim, out);
    DLPM_LAUNCH_CHECK();
    return DLPM_OK;
}

int launch_timestep_embedding(const float *t, float *emb, int64_t B, int dim, hipStream_t st) {
    k_timestep_embedding<<<(unsigned)ceil_div(B * dim, 256), 256, 0, st>>>(t, emb, B, dim);
    DLPM_LAUNCH_CHECK();
    return DLPM_OK;
}

}  // namespace dlpm
