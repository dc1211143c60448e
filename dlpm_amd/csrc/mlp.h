// mlp.h -- what mlp.hip (forward, fused sampling loop) and mlp_train.hip (backward, the flat parameter vector) share: the handle and
// the lane kernels' forward.  lane_forward is the ONE definition of the net up to the last block's output: k_mlp_forward runs it
// with a tap that keeps nothing, k_mlp_backward_rows with a tap that writes the per-row records of its walk back, so the backward's
// recomputed forward is the forward, bit for bit, by construction.
// k_mlp_sample and k_mlp_tp_table (mlp.hip) are no instances of it: they read the float4-interleaved q4 copies of the weights, give
// one sample to a wave, and take every term that depends on the step alone from a table.
#pragma once
#include <map>
#include <string>
#include <vector>

#include "common.h"
#include "mlp_pack.h"

namespace dlpm {

constexpr int NU = LANE_NU;   // hidden units == wavefront width
constexpr int SPW = 4;        // samples per wave

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

// d silu(v) / dv with the forward's own sigmoid
__device__ __forceinline__ float dsilu(float v) {
    const float sg = 1.0f / (1.0f + __expf(-v));
    return sg * (1.0f + v * (1.0f - sg));
}

// with KEEP the backward's copy of the normalised value xh and of 1 / sigma rs come out too; v gets the same bits either way
template <bool KEEP = false>
__device__ __forceinline__ void layer_norm(float v[SPW], float gam, float bet, float *xh = nullptr, float *rs = nullptr) {
#pragma unroll
    for (int s = 0; s < SPW; s++) {
        const float mean = wave_sum(v[s]) * (1.0f / NU);
        const float d = v[s] - mean;
        const float var = wave_sum(d * d) * (1.0f / NU);
        const float r = 1.0f / sqrtf(var + 1e-5f);
        const float n = d * r;
        if constexpr (KEEP) { rs[s] = r; xh[s] = n; }
        v[s] = n * gam + bet;
    }
}

// a tap that keeps nothing: the plain forward
struct LaneNoTap {
    static constexpr bool KEEP = false;
    __device__ __forceinline__ void time_emb0(const float *, const float *) {}
    __device__ __forceinline__ void time_emb1(const float *, const float *) {}
    __device__ __forceinline__ void norm_in(const float *, const float *) {}
    __device__ __forceinline__ void block_in(int, const float *) {}
    __device__ __forceinline__ void norm1(int, const float *, const float *) {}
    __device__ __forceinline__ void t_proj(int, const float *) {}
    __device__ __forceinline__ void block_mid(int, const float *) {}
    __device__ __forceinline__ void norm2(int, const float *, const float *) {}
};

// The forward of the wave's SPW rows s0 .. s0 + 3 (rows from B on are zeros) up to and including the last block: h is the input
// of the output layer.  lane = hidden unit; actT and tembT are [NU][SPW] floats of LDS.  The tap sees, where they arise: the two
// time-embedding layers' pre-activations and activations (zeros in the lanes from TE on), every LayerNorm's normalised value and
// 1 / sigma (only a tap with KEEP), and per block its input h, its t_proj output and the input y of its second Linear.
template <class Tap>
__device__ __forceinline__ void lane_forward(const float *P, const MlpOffsets &o, const float *x, const float *t, int64_t B, int F,
                                             int TE, int nblk, int lane, int64_t s0, float *actT, float *tembT, float (&h)[SPW],
                                             Tap &tap) {
    // ---- time embedding (Model.py:64,68-72,191): Linear(1,TE) -> SiLU -> Linear(TE,TE) -> SiLU
    float tv[SPW], pre[SPW], act[SPW];
#pragma unroll
    for (int s = 0; s < SPW; s++) { tv[s] = (s0 + s < B) ? t[s0 + s] : 0.f; pre[s] = 0.f; act[s] = 0.f; }
    if (lane < TE) {
        const float w = P[o.te_w + lane], b = P[o.te_b + lane];
#pragma unroll
        for (int s = 0; s < SPW; s++) { pre[s] = fmaf(w, tv[s], b); act[s] = silu(pre[s]); actT[lane * SPW + s] = act[s]; }
    }
    tap.time_emb0(pre, act);
    __syncthreads();
#pragma unroll
    for (int s = 0; s < SPW; s++) { pre[s] = 0.f; act[s] = 0.f; }
    if (lane < TE) {
        float acc[SPW];
        const float b = P[o.tm_b + lane];
#pragma unroll
        for (int s = 0; s < SPW; s++) acc[s] = b;
        for (int k = 0; k < TE; k++) {
            const float w = P[o.tm_w + k * TE + lane];
#pragma unroll
            for (int s = 0; s < SPW; s++) acc[s] = fmaf(w, actT[k * SPW + s], acc[s]);
        }
#pragma unroll
        for (int s = 0; s < SPW; s++) { pre[s] = acc[s]; act[s] = silu(acc[s]); tembT[lane * SPW + s] = act[s]; }
    }
    tap.time_emb1(pre, act);
    __syncthreads();

    // ---- input layer (Model.py:93-97): Linear(F,64) -> LayerNorm -> SiLU
    float xh[SPW], rs[SPW];   // written by a LayerNorm with KEEP only
    {
        const float b = P[o.in_b + lane];
#pragma unroll
        for (int s = 0; s < SPW; s++) h[s] = b;
        for (int f = 0; f < F; f++) {
            const float w = P[o.in_w + f * NU + lane];
#pragma unroll
            for (int s = 0; s < SPW; s++) h[s] = fmaf(w, (s0 + s < B) ? x[(s0 + s) * F + f] : 0.f, h[s]);
        }
        layer_norm<Tap::KEEP>(h, P[o.in_g + lane], P[o.in_be + lane], xh, rs);
        tap.norm_in(xh, rs);
#pragma unroll
        for (int s = 0; s < SPW; s++) h[s] = silu(h[s]);
    }

    // ---- conditioned residual blocks (DiffusionBlocks.py:125-136)
    for (int bi = 0; bi < nblk; bi++) {
        const float *Q = P + o.blk0 + (int64_t)bi * o.blk_stride;
        tap.block_in(bi, h);
#pragma unroll
        for (int s = 0; s < SPW; s++) actT[lane * SPW + s] = h[s];
        __syncthreads();
        float y[SPW], tp[SPW];
        const float b1 = Q[o.b_b1 + lane], tb = Q[o.b_tb + lane];
#pragma unroll
        for (int s = 0; s < SPW; s++) { y[s] = b1; tp[s] = tb; }
        matvec(Q + o.b_w1, NU, actT, lane, y);
        layer_norm<Tap::KEEP>(y, Q[o.b_g1 + lane], Q[o.b_be1 + lane], xh, rs);
        tap.norm1(bi, xh, rs);
        matvec(Q + o.b_tw, TE, tembT, lane, tp);
        tap.t_proj(bi, tp);
#pragma unroll
        for (int s = 0; s < SPW; s++) y[s] = silu(y[s]) + silu(tp[s]);
        tap.block_mid(bi, y);
        __syncthreads();  // everyone is done reading actT
#pragma unroll
        for (int s = 0; s < SPW; s++) actT[lane * SPW + s] = y[s];
        __syncthreads();
        float z[SPW];
        const float b2 = Q[o.b_b2 + lane];
#pragma unroll
        for (int s = 0; s < SPW; s++) z[s] = b2;
        matvec(Q + o.b_w2, NU, actT, lane, z);
        layer_norm<Tap::KEEP>(z, Q[o.b_g2 + lane], Q[o.b_be2 + lane], xh, rs);
        tap.norm2(bi, xh, rs);
#pragma unroll
        for (int s = 0; s < SPW; s++) h[s] = silu(z[s] + h[s]);
        __syncthreads();
    }
}
#endif

}  // namespace dlpm

struct dlpm_mlp {
    int F, nunits, nblocks, TE;
    std::vector<float> host;       // packed blob, filled by set_param
    int blob_floats = 0;           // its size (mlp_lane_offsets)
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
    int64_t *flat_map = nullptr;
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
    int64_t *gen_map = nullptr;    // [2][P]: the flat vector's map into both regions (mlp_train.hip), built on first use
};

namespace dlpm {
// the flat parameter vector of the handle's net, parameters_to_vector(model.parameters()) (mlp_pack.h)
inline MlpFlat mlp_flat_of(const dlpm_mlp *m) { return mlp_flat(m->F, m->nunits, m->TE, m->nblocks, m->ln); }
// mlp_general.hip
int mlp_general_init(dlpm_mlp *m);
int mlp_general_set_param(dlpm_mlp *m, const char *key, const float *w, int64_t numel);
int mlp_general_finalize(dlpm_mlp *m);
int mlp_general_forward(dlpm_mlp *m, const float *x_dev, const float *t_dev, float *eps_dev, int64_t B, hipStream_t st);
// mlp_general_grad.hip: the general handle's half of the workspace size and of the backward (mlp_train.hip: mlp_backward), from the
// first check that depends on the kind of handle on; `name` is the entry point the messages name
int64_t mlp_general_workspace_bytes(const dlpm_mlp *m, const char *name, int64_t rows);
int mlp_general_backward(dlpm_mlp *m, const char *name, const float *x_dev, const float *t_dev, const float *dout_dev, int64_t rows,
                         float *grad_flat_dev, float *dx_dev, void *workspace_dev, int64_t workspace_bytes, hipStream_t st);
}  // namespace dlpm

// the fused trainer's entry points and the one-launch sampling loop run the lane kernels' net only (any net's gradients:
// dlpm_amd_mlp_grad.h); `name` is a string, literal or not
#define DLPM_MLP_REFUSE_GENERAL(m, name, what)                                                                                  \
    do {                                                                                                                        \
        if ((m)->general) {                                                                                                     \
            ::dlpm::set_error("%s: " what " runs at the shipped 64-unit architecture (nunits 64, time_emb_size <= 64, "          \
                              "LayerNorm, skip connections); this net (nunits %d, time_emb_size %d) takes the general forward, " \
                              "whose gradients come through dlpm_amd_mlp_grad.h (MLPModel(differentiable=True))",               \
                              name, (m)->nunits, (m)->TE);                                                                      \
            return DLPM_ERR_UNSUPPORTED;                                                                                        \
        }                                                                                                                       \
    } while (0)

// every entry point that needs the device blob
#define DLPM_MLP_NEED_FINALIZED(m, name)                                   \
    do {                                                                   \
        if (!(m)->finalized) {                                             \
            ::dlpm::set_error("%s: call dlpm_mlp_finalize first", name);   \
            return DLPM_ERR_STATE;                                         \
        }                                                                  \
    } while (0)
