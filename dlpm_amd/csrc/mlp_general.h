// mlp_general.h -- what the general toy-net forward (mlp_general.hip) and its backward (mlp_general_grad.hip) share: the kernel
// arguments, the MFMA tile loop, the row sums and the LayerNorm over a row tile.  These building blocks have one definition; the
// SEQUENCE of the forward is written out in both kernels (k_mlp_general and the first half of k_mlp_general_backward) and has to
// be kept the same by hand, operation for operation: the build does not contract, so the source order is the rounding order.
// (Running one shared body in both kernels gives the same bits, but hipcc allocates the backward's registers differently from
// the same IR and its smallest row passes measured 0.7 % slower: profiles/mlp_forward_body/README.md.)
#pragma once
#include "mlp.h"

namespace dlpm {

typedef float floatx4 __attribute__((ext_vector_type(4)));

struct GenArgs {
    const float *P;
    MlpGenLayout L;
    const float *x, *t;
    float *out;
    int64_t B;
    int ln, skip;
};

// acc[m][n] += A[16 m .. 16 m + 15][0 .. 16 KG) * (column tile n of the packed operand Wp); Wp points at this wave's first tile
template <int MT, int NT>
__device__ __forceinline__ void gemm_tiles(const float4 *__restrict__ Wp, int KG, const float *A, int ld, int lane,
                                           floatx4 (&acc)[MT][NT]) {
    const float *arow = A + (lane & 15) * ld + 4 * (lane >> 4);
    const float4 *wl = Wp + lane;
    for (int g = 0; g < KG; g++) {
        float4 b[NT], a[MT];
#pragma unroll
        for (int n = 0; n < NT; n++) b[n] = wl[((int64_t)n * KG + g) * 64];
#pragma unroll
        for (int m = 0; m < MT; m++) a[m] = *reinterpret_cast<const float4 *>(arow + m * 16 * ld + 16 * g);
#pragma unroll
        for (int m = 0; m < MT; m++)
#pragma unroll
            for (int n = 0; n < NT; n++) acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m].x, b[n].x, acc[m][n], 0, 0, 0);
#pragma unroll
        for (int m = 0; m < MT; m++)
#pragma unroll
            for (int n = 0; n < NT; n++) acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m].y, b[n].y, acc[m][n], 0, 0, 0);
#pragma unroll
        for (int m = 0; m < MT; m++)
#pragma unroll
            for (int n = 0; n < NT; n++) acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m].z, b[n].z, acc[m][n], 0, 0, 0);
#pragma unroll
        for (int m = 0; m < MT; m++)
#pragma unroll
            for (int n = 0; n < NT; n++) acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m].w, b[n].w, acc[m][n], 0, 0, 0);
    }
}

// the sum over the 16 lanes that hold one row of a column tile; every one of them gets the same bits
__device__ __forceinline__ float row16_sum(float v) {
#pragma unroll
    for (int m = 1; m <= 8; m <<= 1) v += __shfl_xor(v, m);
    return v;
}

// torch's LayerNorm over the NU real columns of every row (mlp.h::layer_norm: mean, centred variance, eps 1e-5), the row sums
// taken over this thread's tiles, its 16 lanes and then the waves in order through part[2][W][M].  With KEEP the backward's copy of
// the normalised value xh and of 1 / sigma rs come out too; v gets the same bits either way.
template <int MT, int NT, bool KEEP = false>
__device__ __forceinline__ void layer_norm_rows(floatx4 (&v)[MT][NT], const float *__restrict__ gam, const float *__restrict__ bet,
                                                const int (&col)[NT], int NU, float *part, int W, int w, int lane,
                                                floatx4 (*xh)[NT] = nullptr, float (*rs)[4] = nullptr) {
    constexpr int M = 16 * MT;
    const float inv = 1.0f / (float)NU;
    const int q4 = 4 * (lane >> 4);
    float mean[MT][4];
#pragma unroll
    for (int m = 0; m < MT; m++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            float s = 0.f;
#pragma unroll
            for (int n = 0; n < NT; n++) s += v[m][n][r];       // padded columns hold exactly 0
            s = row16_sum(s);
            if ((lane & 15) == 0) part[w * M + 16 * m + q4 + r] = s;
        }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < MT; m++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            float s = 0.f;
            for (int ww = 0; ww < W; ww++) s += part[ww * M + 16 * m + q4 + r];
            mean[m][r] = s * inv;
        }
    float *part2 = part + W * M;
#pragma unroll
    for (int m = 0; m < MT; m++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            float s = 0.f;
#pragma unroll
            for (int n = 0; n < NT; n++) {
                const float d = col[n] < NU ? v[m][n][r] - mean[m][r] : 0.f;   // a padded column is no part of the variance
                v[m][n][r] = d;
                s += d * d;
            }
            s = row16_sum(s);
            if ((lane & 15) == 0) part2[w * M + 16 * m + q4 + r] = s;
        }
    __syncthreads();
    float g[NT], be[NT];
#pragma unroll
    for (int n = 0; n < NT; n++) { g[n] = gam[col[n]]; be[n] = bet[col[n]]; }
#pragma unroll
    for (int m = 0; m < MT; m++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            float s = 0.f;
            for (int ww = 0; ww < W; ww++) s += part2[ww * M + 16 * m + q4 + r];
            const float rstd = 1.0f / sqrtf(s * inv + 1e-5f);
            if constexpr (KEEP) rs[m][r] = rstd;
#pragma unroll
            for (int n = 0; n < NT; n++) {
                const float t = v[m][n][r] * rstd;
                if constexpr (KEEP) xh[m][n][r] = t;
                v[m][n][r] = t * g[n] + be[n];
            }
        }
}

// this thread's elements into the activation image: rows 16 m + 4 (lane >> 4) + r, columns col[n]
template <int MT, int NT>
__device__ __forceinline__ void store_tiles(float *A, int ld, const floatx4 (&v)[MT][NT], const int (&col)[NT], int lane) {
#pragma unroll
    for (int m = 0; m < MT; m++)
#pragma unroll
        for (int n = 0; n < NT; n++)
#pragma unroll
            for (int r = 0; r < 4; r++) A[(16 * m + 4 * (lane >> 4) + r) * ld + col[n]] = v[m][n][r];
}

}  // namespace dlpm
