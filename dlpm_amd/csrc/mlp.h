// mlp.h -- what mlp.hip (forward, fused sampling loop) and mlp_train.hip (backward, parameter layout) share: the handle, the
// offsets of the packed parameter blob and the per-wave building blocks of the forward.  One definition, so the backward's
// recomputed forward rounds exactly as k_mlp_forward does.
#pragma once
#include <map>
#include <string>
#include <vector>

#include "common.h"
#include "mlp_pack.h"

namespace dlpm {

constexpr int NU = 64;   // hidden units == wavefront width
constexpr int SPW = 4;   // samples per wave

struct MlpOffsets {      // offsets (floats) into the packed parameter blob
    int te_w, te_b, tm_w, tm_b, in_w, in_b, in_g, in_be, blk0, blk_stride, out_w, out_b;
    // per block: w1T[64*64] b1 g1 be1 twT[TE*64] tb w2T[64*64] b2 g2 be2
    int b_w1, b_b1, b_g1, b_be1, b_tw, b_tb, b_w2, b_b2, b_g2, b_be2;
};

#ifdef __HIPCC__
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

__device__ __forceinline__ float silu(float v) { return v / (1.0f + __expf(-v)); }

// acc[s] += sum_k WT[k][lane] * act[k][s]
__device__ __forceinline__ void matvec(const float *__restrict__ WT, int K, const float *actT, int lane, float acc[SPW]) {
#pragma unroll 8
    for (int k = 0; k < K; k++) {
        const float w = WT[k * NU + lane];
        const float4 h = *reinterpret_cast<const float4 *>(actT + k * SPW);
        acc[0] = fmaf(w, h.x, acc[0]);
        acc[1] = fmaf(w, h.y, acc[1]);
        acc[2] = fmaf(w, h.z, acc[2]);
        acc[3] = fmaf(w, h.w, acc[3]);
    }
}

__device__ __forceinline__ void layer_norm(float v[SPW], float gam, float bet) {
#pragma unroll
    for (int s = 0; s < SPW; s++) {
        const float mean = wave_sum(v[s]) * (1.0f / NU);
        const float d = v[s] - mean;
        const float var = wave_sum(d * d) * (1.0f / NU);
        v[s] = d * (1.0f / sqrtf(var + 1e-5f)) * gam + bet;
    }
}
#endif

}  // namespace dlpm

struct dlpm_mlp {
    int F, nunits, nblocks, TE;
    std::vector<float> host;       // packed blob, filled by set_param
    std::map<std::string, bool> seen;
    dlpm::MlpOffsets off;
    float *dev = nullptr;
    float4 *q4 = nullptr;      // float4-interleaved copies of the 64x64 matrices (k_mlp_sample)
    float *tp = nullptr;       // [T][nblocks+1][64] step-only terms
    int tp_T = 0;
    bool finalized = false;
    // training (mlp_train.hip): the parameters once more as torch lays them out, parameters_to_vector(model.parameters()), and
    // the index of every element of that vector in the blob.  `flat` is what the backward multiplies by (W[n][k] is the
    // transpose of the blob's WT[k][n]); finalize() marks it stale, the next training call regathers it.
    float *flat = nullptr;
    int32_t *flat_map = nullptr;
    bool flat_valid = false;
    // the general forward (mlp_general.hip): every net the lane kernels do not take.  Such a handle uses none of the fields above
    // but `finalized`: set_param keeps the tensors as given, finalize packs them into the MFMA blob.
    int flags = 0;                 // DLPM_MLP_* of dlpm_mlp_create_ex
    bool ln = true, skip = true;   // LayerNorm / skip connection
    bool general = false;
    dlpm::MlpGenLayout gen{};
    int gen_M = 0;                 // rows of the tallest tile a workgroup may own: 32 where the LDS holds them, else 16
    std::map<std::string, std::vector<float>> raw;
    float *gen_dev = nullptr;      // the forward's blob, then the transposed operands of the backward (MlpGenGradLayout)
    int64_t *gen_map = nullptr;    // [2][P]: the flat vector's map into both regions (mlp_general_grad.hip), built on first use
};

namespace dlpm {
// mlp_general.hip
int mlp_general_init(dlpm_mlp *m);
int mlp_general_set_param(dlpm_mlp *m, const char *key, const float *w, int64_t numel);
int mlp_general_finalize(dlpm_mlp *m);
int mlp_general_forward(dlpm_mlp *m, const float *x_dev, const float *t_dev, float *eps_dev, int64_t B, hipStream_t st);
}  // namespace dlpm

// the fused trainer's entry points and the one-launch sampling loop run the lane kernels' net only (any net's gradients:
// mlp_general_grad.hip)
#define DLPM_MLP_REFUSE_GENERAL(m, name, what)                                                                                  \
    do {                                                                                                                        \
        if ((m)->general) {                                                                                                     \
            ::dlpm::set_error(name ": " what " runs at the shipped 64-unit architecture (nunits 64, time_emb_size <= 64, "       \
                              "LayerNorm, skip connections); this net (nunits %d, time_emb_size %d) takes the general forward, " \
                              "whose gradients come through dlpm_amd_mlp_grad.h (MLPModel(differentiable=True))",               \
                              (m)->nunits, (m)->TE);                                                                            \
            return DLPM_ERR_UNSUPPORTED;                                                                                        \
        }                                                                                                                       \
    } while (0)
