// mlp_train.hip -- training of the toy net (include/dlpm_amd_train.h): the backward of k_mlp_forward, the loss gradient, the
// gradient-norm clip, AdamW with EMA shadows, and torch's flat parameter vector for either kind of handle: the entry points of
// dlpm_amd_train.h and of dlpm_amd_mlp_grad.h (the general handle's backward itself: mlp_general_grad.hip).
//
// Backward.  The net is 55 k parameters; per row the backward is ~210 kFLOP of matrix-vector work plus, per 64x64 matrix, one
// rank-1 update of its gradient.  The matrix-vector half keeps the forward's mapping (one wavefront owns 4 rows, lanes = hidden
// units, a Linear is a k-loop of coalesced weight loads against a 16-byte LDS broadcast): dL/d(input) = W^T dY needs W[n][k] with
// the lane on k, which is torch's own layout, so the handle keeps the flat vector next to the transposed blob.  The rank-1
// updates are a reduction over rows and must not depend on the grid: k_mlp_backward_rows leaves every layer's input A and
// dL/d(pre-activation) dY per row in the workspace, k_mlp_wgrad forms dY^T A over chunks of 64 rows (rows in order; plain FMAs:
// 113 MFLOP per step of 1024 rows leave the matrix pipe nothing to win), and
// k_mlp_wgrad_sum adds the chunk partials in chunk order in fp64.  No atomics anywhere.
#include <algorithm>
#include <cmath>

#include "mlp.h"
#include "../../include/dlpm_amd_mlp_grad.h"
#include "../../include/dlpm_amd_train.h"

using namespace dlpm;

namespace {

constexpr int RC = 64;   // rows per chunk of the weight-gradient reduction

// 64-wide per-row records in the workspace: [record][row][64]
enum { R_E0 = 0, R_TEMB, R_DA0, R_DA1, R_XHIN, R_DLNIN, R_DZIN, R_HFIN, R_GLOBAL };
enum { B_H = 0, B_XH1, B_TP, B_Y, B_XH2, B_DLN1, B_DLN2, B_DZ1, B_DZ2, B_DTP, R_PER_BLOCK };
// per-row scalars (the LayerNorms' 1/sigma): [scalar][row]; 0 = input layer, 1 + 2 bi, 2 + 2 bi = block bi

struct BwdArgs {
    const float *P;      // packed blob ([k][unit])
    const float *W;      // flat vector (torch layout)
    MlpOffsets o;        // offsets into P
    MlpFlat fo;          // offsets into W
    const float *x, *t, *dout;
    float *dx;
    float *rec, *sc, *part;
    int64_t rows;
    int F, TE, nblk;
    int64_t nparam;
};

__device__ __forceinline__ float *rec_at(const BwdArgs &a, int q, int64_t row) { return a.rec + ((int64_t)q * a.rows + row) * NU; }

#define FOR_S for (int s = 0; s < SPW; s++)

// dL/d(LayerNorm input) from dL/d(LayerNorm output) g
__device__ __forceinline__ void layer_norm_back(const float g[SPW], const float xh[SPW], const float rs[SPW], float gam, float dz[SPW]) {
#pragma unroll
    for (int s = 0; s < SPW; s++) {
        const float dxh = g[s] * gam;
        const float m1 = wave_sum(dxh) * (1.0f / NU);
        const float m2 = wave_sum(dxh * xh[s]) * (1.0f / NU);
        dz[s] = rs[s] * (dxh - m1 - xh[s] * m2);
    }
}

// The per-row records of the wave's 4 rows in the workspace: lane_forward's tap writes what the recomputed forward leaves there,
// the walk back reads it and adds its own
struct RowRecords {
    static constexpr bool KEEP = true;
    const BwdArgs &a;
    const int lane;
    const int64_t s0;
    bool live[SPW];
    float a0[SPW], a1[SPW];   // the time embedding's pre-activations
    __device__ __forceinline__ RowRecords(const BwdArgs &a_, int lane_, int64_t s0_) : a(a_), lane(lane_), s0(s0_) {
#pragma unroll
        FOR_S live[s] = s0 + s < a.rows;
    }
    __device__ __forceinline__ void put(int q, const float *v) const {
#pragma unroll
        FOR_S if (live[s]) rec_at(a, q, s0 + s)[lane] = v[s];
    }
    __device__ __forceinline__ void get(int q, float *v) const {
#pragma unroll
        FOR_S v[s] = live[s] ? rec_at(a, q, s0 + s)[lane] : 0.f;
    }
    // every lane stores and later reads back the same word: each reads its own store
    __device__ __forceinline__ void put_sc(int q, const float *v) const {
#pragma unroll
        FOR_S if (live[s]) a.sc[(int64_t)q * a.rows + s0 + s] = v[s];
    }
    __device__ __forceinline__ void get_sc(int q, float *v) const {
#pragma unroll
        FOR_S v[s] = live[s] ? a.sc[(int64_t)q * a.rows + s0 + s] : 0.f;
    }
    // lane_forward's hooks
    __device__ __forceinline__ void time_emb0(const float *pre, const float *act) {
#pragma unroll
        FOR_S a0[s] = pre[s];
        put(R_E0, act);
    }
    __device__ __forceinline__ void time_emb1(const float *pre, const float *act) {
#pragma unroll
        FOR_S a1[s] = pre[s];
        put(R_TEMB, act);
    }
    __device__ __forceinline__ void norm_in(const float *xh, const float *rs) { put(R_XHIN, xh); put_sc(0, rs); }
    __device__ __forceinline__ void block_in(int bi, const float *h) { put(R_GLOBAL + bi * R_PER_BLOCK + B_H, h); }
    __device__ __forceinline__ void norm1(int bi, const float *xh, const float *rs) { put(R_GLOBAL + bi * R_PER_BLOCK + B_XH1, xh); put_sc(1 + 2 * bi, rs); }
    __device__ __forceinline__ void t_proj(int bi, const float *tp) { put(R_GLOBAL + bi * R_PER_BLOCK + B_TP, tp); }
    __device__ __forceinline__ void block_mid(int bi, const float *y) { put(R_GLOBAL + bi * R_PER_BLOCK + B_Y, y); }
    __device__ __forceinline__ void norm2(int bi, const float *xh, const float *rs) { put(R_GLOBAL + bi * R_PER_BLOCK + B_XH2, xh); put_sc(2 + 2 * bi, rs); }
};

__global__ void __launch_bounds__(64) k_mlp_backward_rows(BwdArgs a) {
    __shared__ __attribute__((aligned(16))) float actT[NU * SPW];
    __shared__ __attribute__((aligned(16))) float tembT[NU * SPW];
    __shared__ __attribute__((aligned(16))) float gT[NU * SPW];
    const int lane = threadIdx.x;
    const int64_t s0 = (int64_t)blockIdx.x * SPW;
    const float *P = a.P;
    const MlpOffsets &o = a.o;
    const MlpFlat &fo = a.fo;
    const int TE = a.TE, F = a.F;
    RowRecords recs(a, lane, s0);

    // ================================================================ forward: lane_forward, as k_mlp_forward runs it
    float h[SPW], xh[SPW], rs[SPW];
    lane_forward(P, o, a.x, a.t, a.rows, F, TE, a.nblk, lane, s0, actT, tembT, h, recs);
    recs.put(R_HFIN, h);

    // ================================================================ backward
    float dh[SPW], dtemb[SPW];
#pragma unroll
    FOR_S { dh[s] = 0.f; dtemb[s] = 0.f; }
    for (int f = 0; f < F; f++) {      // out[f] = sum_n out_w[f][n] h[n] + b[f]
        const float w = P[o.out_w + f * NU + lane];
#pragma unroll
        FOR_S dh[s] = fmaf(w, recs.live[s] ? a.dout[(s0 + s) * F + f] : 0.f, dh[s]);
    }
    for (int bi = a.nblk - 1; bi >= 0; bi--) {
        const float *Q = P + o.blk0 + (int64_t)bi * o.blk_stride;
        const float *WQ = a.W + fo.blk0 + (int64_t)bi * fo.blk_stride;
        const int rb = R_GLOBAL + bi * R_PER_BLOCK;
        float hin[SPW], ds[SPW], dz[SPW];
        // h_out = silu(LN2(W2 y + b2) + h_in)
        recs.get(rb + B_H, hin);
        recs.get(rb + B_XH2, xh);
        recs.get_sc(2 + 2 * bi, rs);
        const float g2 = Q[o.b_g2 + lane], be2 = Q[o.b_be2 + lane];
#pragma unroll
        FOR_S ds[s] = dh[s] * dsilu(xh[s] * g2 + be2 + hin[s]);
        recs.put(rb + B_DLN2, ds);
        layer_norm_back(ds, xh, rs, g2, dz);
        recs.put(rb + B_DZ2, dz);
#pragma unroll
        FOR_S gT[lane * SPW + s] = dz[s];
        __syncthreads();
        float dy[SPW];
#pragma unroll
        FOR_S dy[s] = 0.f;
        matvec(WQ + fo.b_w2, NU, gT, lane, dy);       // dy[k] = sum_n W2[n][k] dz[n]
        // y = silu(LN1(W1 h_in + b1)) + silu(Wt temb + tb)
        float tp[SPW], du[SPW], dtp[SPW];
        recs.get(rb + B_XH1, xh);
        recs.get_sc(1 + 2 * bi, rs);
        recs.get(rb + B_TP, tp);
        const float g1 = Q[o.b_g1 + lane], be1 = Q[o.b_be1 + lane];
#pragma unroll
        FOR_S { du[s] = dy[s] * dsilu(xh[s] * g1 + be1); dtp[s] = dy[s] * dsilu(tp[s]); }
        recs.put(rb + B_DLN1, du);
        recs.put(rb + B_DTP, dtp);
        __syncthreads();
#pragma unroll
        FOR_S gT[lane * SPW + s] = dtp[s];
        __syncthreads();
        if (lane < TE) {                              // dtemb[k] += sum_n Wt[n][k] dtp[n]
            const float *Wt = WQ + fo.b_tw;
            for (int n = 0; n < NU; n++) {
                const float w = Wt[n * TE + lane];
                const float4 g = *reinterpret_cast<const float4 *>(gT + n * SPW);
                dtemb[0] = fmaf(w, g.x, dtemb[0]);
                dtemb[1] = fmaf(w, g.y, dtemb[1]);
                dtemb[2] = fmaf(w, g.z, dtemb[2]);
                dtemb[3] = fmaf(w, g.w, dtemb[3]);
            }
        }
        layer_norm_back(du, xh, rs, g1, dz);
        recs.put(rb + B_DZ1, dz);
        __syncthreads();
#pragma unroll
        FOR_S gT[lane * SPW + s] = dz[s];
        __syncthreads();
#pragma unroll
        FOR_S dh[s] = ds[s];                          // the skip
        matvec(WQ + fo.b_w1, NU, gT, lane, dh);       // + sum_n W1[n][k] dz[n]
        __syncthreads();
    }
    {   // h_0 = silu(LN(W_in x + b))
        float du[SPW], dz[SPW];
        recs.get(R_XHIN, xh);
        recs.get_sc(0, rs);
        const float g = P[o.in_g + lane], be = P[o.in_be + lane];
#pragma unroll
        FOR_S du[s] = dh[s] * dsilu(xh[s] * g + be);
        recs.put(R_DLNIN, du);
        layer_norm_back(du, xh, rs, g, dz);
        recs.put(R_DZIN, dz);
        if (a.dx)
            for (int f = 0; f < F; f++) {
                const float w = P[o.in_w + f * NU + lane];
#pragma unroll
                FOR_S {
                    const float r = wave_sum(w * dz[s]);
                    if (lane == 0 && recs.live[s]) a.dx[(s0 + s) * F + f] = r;
                }
            }
    }
    {   // temb = silu(a1), a1 = Wtm e0 + b, e0 = silu(a0), a0 = w t + b
        float da1[SPW], da0[SPW];
#pragma unroll
        FOR_S { da1[s] = lane < TE ? dtemb[s] * dsilu(recs.a1[s]) : 0.f; da0[s] = 0.f; }
        recs.put(R_DA1, da1);
#pragma unroll
        FOR_S gT[lane * SPW + s] = da1[s];
        __syncthreads();
        if (lane < TE) {
            const float *Wtm = a.W + fo.tm_w;
            float de[SPW] = {0.f, 0.f, 0.f, 0.f};
            for (int n = 0; n < TE; n++) {
                const float w = Wtm[n * TE + lane];
#pragma unroll
                FOR_S de[s] = fmaf(w, gT[n * SPW + s], de[s]);
            }
#pragma unroll
            FOR_S da0[s] = de[s] * dsilu(recs.a0[s]);
        }
        recs.put(R_DA0, da0);
    }
}

// One reduction over rows: M[n][k] = sum_r Y[r][n] A[r][k] (Y a 64-wide record; without Y the column sums of A), optionally the column sums of Y and
// sum_r Y[r][n] Ad[r][n] (the LayerNorm weight).  Results go to flat offsets.
struct Job {
    const float *Y;       // [rows][64], or null: out[k] = sum_r A[r][k]
    const float *A;       // [rows][ldA]
    const float *Ad;      // [rows][64] or null
    int ldA, K, nmax, outW, sN, sK, outC, outD;
};

__device__ Job job_of(const BwdArgs &a, int j) {
    Job b;
    const MlpFlat &fo = a.fo;
    b.Y = nullptr; b.A = nullptr; b.Ad = nullptr;
    b.ldA = NU; b.K = 0; b.nmax = NU; b.outW = 0; b.sN = 0; b.sK = 0; b.outC = -1; b.outD = -1;
    const int F = a.F, TE = a.TE;
    if (j == 0) {            // time_emb: Linear(1, TE)
        b.Y = rec_at(a, R_DA0, 0); b.A = a.t; b.ldA = 1; b.K = 1; b.nmax = TE; b.outW = fo.te_w; b.sN = 1; b.sK = 1; b.outC = fo.te_b;
    } else if (j == 1) {     // time_mlp.2: Linear(TE, TE)
        b.Y = rec_at(a, R_DA1, 0); b.A = rec_at(a, R_E0, 0); b.K = TE; b.nmax = TE; b.outW = fo.tm_w; b.sN = TE; b.sK = 1; b.outC = fo.tm_b;
    } else if (j == 2) {     // linear_in: Linear(F, 64)
        b.Y = rec_at(a, R_DZIN, 0); b.A = a.x; b.ldA = F; b.K = F; b.outW = fo.in_w; b.sN = F; b.sK = 1; b.outC = fo.in_b;
    } else if (j == 3) {     // group_norm_in
        b.Y = rec_at(a, R_DLNIN, 0); b.Ad = rec_at(a, R_XHIN, 0); b.outD = fo.in_g; b.outC = fo.in_be;
    } else if (j == 4) {     // outblocks_mean.1.weight [F][64] = sum_r dout[r][f] h[r][n]
        b.Y = rec_at(a, R_HFIN, 0); b.A = a.dout; b.ldA = F; b.K = F; b.outW = fo.out_w; b.sN = 1; b.sK = NU;
    } else if (j == 5) {     // outblocks_mean.1.bias [F] = sum_r dout[r][f]
        b.A = a.dout; b.ldA = F; b.K = F; b.nmax = 1; b.outW = fo.out_b; b.sN = 0; b.sK = 1;
    } else {
        const int bi = (j - 6) / 5, w = (j - 6) % 5;
        const int rb = R_GLOBAL + bi * R_PER_BLOCK, base = fo.blk0 + bi * fo.blk_stride;
        if (w == 0) {        // mlp_1.1
            b.Y = rec_at(a, rb + B_DZ1, 0); b.A = rec_at(a, rb + B_H, 0); b.K = NU; b.outW = base + fo.b_w1; b.sN = NU; b.sK = 1; b.outC = base + fo.b_b1;
        } else if (w == 1) { // mlp_2.1
            b.Y = rec_at(a, rb + B_DZ2, 0); b.A = rec_at(a, rb + B_Y, 0); b.K = NU; b.outW = base + fo.b_w2; b.sN = NU; b.sK = 1; b.outC = base + fo.b_b2;
        } else if (w == 2) { // t_proj.1
            b.Y = rec_at(a, rb + B_DTP, 0); b.A = rec_at(a, R_TEMB, 0); b.K = TE; b.outW = base + fo.b_tw; b.sN = TE; b.sK = 1; b.outC = base + fo.b_tb;
        } else if (w == 3) { // group_norm1
            b.Y = rec_at(a, rb + B_DLN1, 0); b.Ad = rec_at(a, rb + B_XH1, 0); b.outD = base + fo.b_g1; b.outC = base + fo.b_be1;
        } else {             // group_norm2
            b.Y = rec_at(a, rb + B_DLN2, 0); b.Ad = rec_at(a, rb + B_XH2, 0); b.outD = base + fo.b_g2; b.outC = base + fo.b_be2;
        }
    }
    return b;
}

// grid (jobs, chunks), 256 threads: thread (n = tid & 63, kg = tid >> 6) holds M[n][k0 + 16 kg .. + 15] of one 64-wide k tile
__global__ void __launch_bounds__(256) k_mlp_wgrad(BwdArgs a) {
    const Job b = job_of(a, blockIdx.x);
    const int n = threadIdx.x & 63, kg = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t r0 = (int64_t)blockIdx.y * RC, r1 = min(a.rows, r0 + RC);
    float *part = a.part + (int64_t)blockIdx.y * a.nparam;
    if (!b.Y) {          // the column sums of A alone (the output bias): one column per thread, fp64
        for (int k = threadIdx.x; k < b.K; k += 256) {
            double c = 0.0;
            for (int64_t r = r0; r < r1; r++) c += (double)b.A[r * b.ldA + k];
            part[b.outW + k * b.sK] = (float)c;
        }
        return;
    }
    for (int kt = 0; kt < b.K; kt += NU) {
        const int k0 = kt + kg * 16;
        float acc[16];
#pragma unroll
        for (int j = 0; j < 16; j++) acc[j] = 0.f;
        for (int64_t r = r0; r < r1; r++) {
            const float y = b.Y[r * NU + n];
            const float *Ar = b.A + r * b.ldA;
#pragma unroll
            for (int j = 0; j < 16; j++)
                if (k0 + j < b.K) acc[j] = fmaf(y, Ar[k0 + j], acc[j]);
        }
        if (n < b.nmax)
#pragma unroll
            for (int j = 0; j < 16; j++)
                if (k0 + j < b.K) part[b.outW + n * b.sN + (k0 + j) * b.sK] = acc[j];
    }
    // bias and LayerNorm gradients are single columns: 64 additions each, taken in fp64 and rounded once
    if (kg == 0 && n < b.nmax && (b.outC >= 0 || b.outD >= 0)) {
        double c = 0.0, d = 0.0;
        for (int64_t r = r0; r < r1; r++) {
            const double y = (double)b.Y[r * NU + n];
            c += y;
            if (b.Ad) d += y * (double)b.Ad[r * NU + n];
        }
        if (b.outC >= 0) part[b.outC + n] = (float)c;
        if (b.outD >= 0) part[b.outD + n] = (float)d;
    }
}

__global__ void __launch_bounds__(256) k_mlp_wgrad_sum(const float *__restrict__ part, float *__restrict__ grad, int64_t P, int chunks) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    double s = 0.0;
    for (int c = 0; c < chunks; c++) s += (double)part[(int64_t)c * P + i];
    grad[i] = (float)s;
}

// ------------------------------------------------------------------------------------------------ the flat parameter vector
// torch's parameters_to_vector(model.parameters()) of either kind of handle (mlp_pack.h: MlpFlat and the two maps into the blobs)
__global__ void __launch_bounds__(256) k_flat_gather(const float *__restrict__ blob, const int64_t *__restrict__ map,
                                                     float *__restrict__ flat, int64_t P) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < P) flat[i] = blob[map[i]];
}

// blob <- flat, through map and, where there is one, the second map (a general handle's transposed operands; -1: no second place),
// then the handle's own flat copy <- flat where it keeps one.  Padded elements are never written, so they stay 0.
__global__ void __launch_bounds__(256) k_flat_scatter(const float *__restrict__ flat, const int64_t *__restrict__ map,
                                                      const int64_t *__restrict__ map2, float *__restrict__ blob,
                                                      float *__restrict__ keep, int64_t P) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < P) {
        const float v = flat[i];
        blob[map[i]] = v;
        if (map2) {
            const int64_t t = map2[i];
            if (t >= 0) blob[t] = v;
        }
        if (keep) keep[i] = v;
    }
}

// the float4 copies of the 64x64 matrices as dlpm_mlp_finalize lays them out: [blk][2][k/4][unit] = W[unit][4kq .. 4kq+3]
__global__ void __launch_bounds__(256) k_q4_refresh(const float *__restrict__ blob, MlpOffsets o, float4 *__restrict__ q4, int nb) {
    const int i = blockIdx.x * 256 + threadIdx.x;      // (bi, which, kq, u)
    if (i >= nb * 2 * (NU / 4) * NU) return;
    const int u = i % NU, kq = (i / NU) % (NU / 4), which = (i / (NU * NU / 4)) % 2, bi = i / (NU * NU / 2);
    const float *src = blob + o.blk0 + (int64_t)bi * o.blk_stride + (which ? o.b_w2 : o.b_w1);
    q4[i] = make_float4(src[(4 * kq + 0) * NU + u], src[(4 * kq + 1) * NU + u], src[(4 * kq + 2) * NU + u], src[(4 * kq + 3) * NU + u]);
}

// a lane handle's flat copy and map, allocated on the first training call; the copy regathered when finalize() made it stale
int ensure_flat(dlpm_mlp *m, hipStream_t st) {
    const MlpFlat f = mlp_flat_of(m);
    if (!m->flat_map) {
        std::vector<int64_t> map((size_t)f.P);
        mlp_lane_flat_map(m->off, f, m->F, m->TE, m->nblocks, map.data());
        for (int64_t v : map)
            if (v < 0 || v >= m->blob_floats) {
                set_error("dlpm_mlp: internal error: the flat parameter map has a hole");
                return DLPM_ERR_STATE;
            }
        DLPM_HIP(hipMalloc(&m->flat_map, f.P * sizeof(int64_t)));
        DLPM_HIP(hipMemcpy(m->flat_map, map.data(), f.P * sizeof(int64_t), hipMemcpyHostToDevice));
    }
    if (!m->flat) {
        DLPM_HIP(hipMalloc(&m->flat, f.P * sizeof(float)));
        m->flat_valid = false;
    }
    if (!m->flat_valid) {
        k_flat_gather<<<(unsigned)ceil_div(f.P, 256), 256, 0, st>>>(m->dev, m->flat_map, m->flat, f.P);
        DLPM_LAUNCH_CHECK();
        m->flat_valid = true;
    }
    return DLPM_OK;
}

// a general handle's map into both regions of its blob, built and uploaded on the first call that needs it; it keeps no flat copy
int ensure_map(dlpm_mlp *m) {
    if (m->gen_map) return DLPM_OK;
    const MlpFlat f = mlp_flat_of(m);
    const MlpGenGradLayout G = mlp_gen_grad_layout(m->gen);
    std::vector<int64_t> map((size_t)(2 * f.P));
    mlp_general_flat_map(m->gen, G, f, map.data(), map.data() + f.P);
    for (int64_t i = 0; i < f.P; i++)
        if (map[i] < 0 || map[i] >= m->gen.total || map[f.P + i] >= m->gen.total + G.total) {
            set_error("dlpm_mlp_grad: internal error: the flat parameter map has a hole");
            return DLPM_ERR_STATE;
        }
    DLPM_HIP(hipMalloc(&m->gen_map, map.size() * sizeof(int64_t)));
    DLPM_HIP(hipMemcpy(m->gen_map, map.data(), map.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    return DLPM_OK;
}

int64_t backward_floats(const dlpm_mlp *m, int64_t rows, int64_t *rec_floats, int64_t *sc_floats) {
    const int nb = m->nblocks + 1;
    const int64_t rec = (int64_t)(R_GLOBAL + nb * R_PER_BLOCK) * rows * NU;
    const int64_t sc = ((int64_t)(1 + 2 * nb) * rows + 3) / 4 * 4;
    if (rec_floats) *rec_floats = rec;
    if (sc_floats) *sc_floats = sc;
    return rec + sc + ceil_div(rows, RC) * mlp_flat_of(m).P;
}

// ------------------------------------------------------------------------------------------------ the five operations
// Each serves its entry point of dlpm_amd_train.h (lane_only: the fused trainer's, which refuses a general handle) and of
// dlpm_amd_mlp_grad.h (either kind of handle); `name` is the entry point, for the messages.
int64_t param_floats(const dlpm_mlp *m, const char *name, bool lane_only) {
    if (!m) return -1;
    if (lane_only) DLPM_MLP_REFUSE_GENERAL(m, name, "training");
    return mlp_flat_of(m).P;
}

int export_params(dlpm_mlp *m, const char *name, bool lane_only, float *flat_dev, int64_t n, dlpm_stream_t stream) {
    DLPM_CHECK_ARG(m && flat_dev, "%s: null argument", name);
    if (lane_only) DLPM_MLP_REFUSE_GENERAL(m, name, "training");
    const int64_t P = mlp_flat_of(m).P;
    DLPM_CHECK_ARG(n == P, "%s: n = %lld, the net has %lld parameters", name, (long long)n, (long long)P);
    DLPM_MLP_NEED_FINALIZED(m, name);
    hipStream_t st = as_stream(stream);
    if (m->general) {
        if (int rc = ensure_map(m)) return rc;
        k_flat_gather<<<(unsigned)ceil_div(P, 256), 256, 0, st>>>(m->gen_dev, m->gen_map, flat_dev, P);
        DLPM_LAUNCH_CHECK();
    } else {
        if (int rc = ensure_flat(m, st)) return rc;
        DLPM_HIP(hipMemcpyAsync(flat_dev, m->flat, n * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    return DLPM_OK;
}

int import_params(dlpm_mlp *m, const char *name, bool lane_only, const float *flat_dev, int64_t n, dlpm_stream_t stream) {
    DLPM_CHECK_ARG(m && flat_dev, "%s: null argument", name);
    if (lane_only) DLPM_MLP_REFUSE_GENERAL(m, name, "training");
    const int64_t P = mlp_flat_of(m).P;
    DLPM_CHECK_ARG(n == P, "%s: n = %lld, the net has %lld parameters", name, (long long)n, (long long)P);
    DLPM_MLP_NEED_FINALIZED(m, name);
    hipStream_t st = as_stream(stream);
    if (m->general) {
        if (int rc = ensure_map(m)) return rc;
        k_flat_scatter<<<(unsigned)ceil_div(P, 256), 256, 0, st>>>(flat_dev, m->gen_map, m->gen_map + P, m->gen_dev, nullptr, P);
        DLPM_LAUNCH_CHECK();
    } else {
        if (int rc = ensure_flat(m, st)) return rc;
        k_flat_scatter<<<(unsigned)ceil_div(P, 256), 256, 0, st>>>(flat_dev, m->flat_map, nullptr, m->dev, m->flat, P);
        DLPM_LAUNCH_CHECK();
        const int nb = m->nblocks + 1;
        k_q4_refresh<<<(unsigned)ceil_div((int64_t)nb * 2 * (NU / 4) * NU, 256), 256, 0, st>>>(m->dev, m->off, m->q4, nb);
        DLPM_LAUNCH_CHECK();
        m->tp_T = 0;
    }
    return DLPM_OK;
}

int64_t workspace_bytes(const dlpm_mlp *m, const char *name, bool lane_only, int64_t rows) {
    if (!m || rows <= 0) return -1;
    if (lane_only) DLPM_MLP_REFUSE_GENERAL(m, name, "training");
    if (m->general) return mlp_general_workspace_bytes(m, name, rows);
    return backward_floats(m, rows, nullptr, nullptr) * (int64_t)sizeof(float);
}

int backward(dlpm_mlp *m, const char *name, bool lane_only, const float *x_dev, const float *t_dev, const float *dout_dev, int64_t rows,
             float *grad_flat_dev, float *dx_dev, void *workspace_dev, int64_t workspace_bytes, dlpm_stream_t stream) {
    DLPM_CHECK_ARG(m && x_dev && t_dev && dout_dev && grad_flat_dev && workspace_dev, "%s: null argument", name);
    DLPM_CHECK_ARG(rows > 0, "%s: rows must be positive (got %lld)", name, (long long)rows);
    if (lane_only) DLPM_MLP_REFUSE_GENERAL(m, name, "training");
    hipStream_t st = as_stream(stream);
    if (m->general)
        return mlp_general_backward(m, name, x_dev, t_dev, dout_dev, rows, grad_flat_dev, dx_dev, workspace_dev, workspace_bytes, st);
    DLPM_CHECK_ARG(ceil_div(rows, SPW) < (1ll << 31) && ceil_div(rows, RC) <= 65535, "%s: rows = %lld is beyond the grid of one call "
                   "(at most %d)", name, (long long)rows, 65535 * RC);
    int64_t rec_floats, sc_floats;
    const int64_t need = backward_floats(m, rows, &rec_floats, &sc_floats) * (int64_t)sizeof(float);
    if (workspace_bytes < need) {
        set_error("%s: the workspace has %lld bytes, %lld are needed", name, (long long)workspace_bytes, (long long)need);
        return DLPM_ERR_NOMEM;
    }
    DLPM_MLP_NEED_FINALIZED(m, name);
    if (int rc = ensure_flat(m, st)) return rc;
    BwdArgs a;
    a.P = m->dev; a.W = m->flat; a.o = m->off; a.fo = mlp_flat_of(m);
    a.nparam = a.fo.P;
    a.x = x_dev; a.t = t_dev; a.dout = dout_dev; a.dx = dx_dev;
    a.rec = static_cast<float *>(workspace_dev); a.sc = a.rec + rec_floats; a.part = a.sc + sc_floats;
    a.rows = rows; a.F = m->F; a.TE = m->TE; a.nblk = m->nblocks + 1;
    const int chunks = (int)ceil_div(rows, RC);
    k_mlp_backward_rows<<<(unsigned)ceil_div(rows, SPW), 64, 0, st>>>(a);
    DLPM_LAUNCH_CHECK();
    k_mlp_wgrad<<<dim3(6 + 5 * a.nblk, chunks), 256, 0, st>>>(a);
    DLPM_LAUNCH_CHECK();
    k_mlp_wgrad_sum<<<(unsigned)ceil_div(a.nparam, 256), 256, 0, st>>>(a.part, grad_flat_dev, a.nparam, chunks);
    DLPM_LAUNCH_CHECK();
    return DLPM_OK;
}

}  // namespace

extern "C" int64_t dlpm_mlp_param_floats(const dlpm_mlp *m) { return param_floats(m, "dlpm_mlp_param_floats", true); }
extern "C" int64_t dlpm_mlp_grad_param_floats(const dlpm_mlp *m) { return param_floats(m, "dlpm_mlp_grad_param_floats", false); }

extern "C" int dlpm_mlp_export_params_f32(dlpm_mlp *m, float *flat_dev, int64_t n, dlpm_stream_t stream) {
    return export_params(m, "dlpm_mlp_export_params_f32", true, flat_dev, n, stream);
}
extern "C" int dlpm_mlp_grad_export_params_f32(dlpm_mlp *m, float *flat_dev, int64_t n, dlpm_stream_t stream) {
    return export_params(m, "dlpm_mlp_grad_export_params_f32", false, flat_dev, n, stream);
}

extern "C" int dlpm_mlp_import_params_f32(dlpm_mlp *m, const float *flat_dev, int64_t n, dlpm_stream_t stream) {
    return import_params(m, "dlpm_mlp_import_params_f32", true, flat_dev, n, stream);
}
extern "C" int dlpm_mlp_grad_import_params_f32(dlpm_mlp *m, const float *flat_dev, int64_t n, dlpm_stream_t stream) {
    return import_params(m, "dlpm_mlp_grad_import_params_f32", false, flat_dev, n, stream);
}

extern "C" int64_t dlpm_mlp_backward_workspace_bytes(const dlpm_mlp *m, int64_t rows) {
    return workspace_bytes(m, "dlpm_mlp_backward_workspace_bytes", true, rows);
}
extern "C" int64_t dlpm_mlp_grad_workspace_bytes(const dlpm_mlp *m, int64_t rows) {
    return workspace_bytes(m, "dlpm_mlp_grad_workspace_bytes", false, rows);
}

extern "C" int dlpm_mlp_backward_f32(dlpm_mlp *m, const float *x_dev, const float *t_dev, const float *dout_dev, int64_t rows,
                                     float *grad_flat_dev, float *dx_dev, void *workspace_dev, int64_t workspace_bytes,
                                     dlpm_stream_t stream) {
    return backward(m, "dlpm_mlp_backward_f32", true, x_dev, t_dev, dout_dev, rows, grad_flat_dev, dx_dev, workspace_dev, workspace_bytes,
                    stream);
}
extern "C" int dlpm_mlp_grad_backward_f32(dlpm_mlp *m, const float *x_dev, const float *t_dev, const float *dout_dev, int64_t rows,
                                          float *grad_flat_dev, float *dx_dev, void *workspace_dev, int64_t workspace_bytes,
                                          dlpm_stream_t stream) {
    return backward(m, "dlpm_mlp_grad_backward_f32", false, x_dev, t_dev, dout_dev, rows, grad_flat_dev, dx_dev, workspace_dev,
                    workspace_bytes, stream);
}

// ------------------------------------------------------------------------------------------------ loss gradient
namespace {

__global__ void __launch_bounds__(256) k_loss_grad(const float *__restrict__ me, const float *__restrict__ tg, const float *__restrict__ terms,
                                                   const int32_t *__restrict__ med, float *__restrict__ out, int64_t B, int outer,
                                                   int inner, int64_t D, int lploss) {
    const int64_t total = (int64_t)outer * inner * B * D;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / D, b = row % B, o = row / ((int64_t)inner * B);
        double w;
        if (med) w = (o == med[b]) ? 1.0 / ((double)inner * (double)B) : 0.0;
        else w = 1.0 / ((double)outer * (double)inner * (double)B);
        const double d = (double)me[i] - (double)tg[i];
        double g;
        if (lploss == 2) {
            const double term = (double)terms[row];
            g = term == 0.0 ? 0.0 : d / ((double)D * term);
        } else if (lploss == 1) {
            g = fmin(fmax(d, -1.0), 1.0) / (double)D;
        } else {
            g = 2.0 * d / (double)D;
        }
        out[i] = w == 0.0 ? 0.f : (float)(g * w);
    }
}

__global__ void __launch_bounds__(1024) k_grad_clip_coef(const float *__restrict__ g, int64_t n, double max_norm, float *__restrict__ norm_out,
                                                         float *__restrict__ coef_out) {
    __shared__ double sh[1024];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 1024) s += (double)g[i] * (double)g[i];
    s = block_sum<1024>(s, sh);
    if (threadIdx.x == 0) {
        const double norm = sqrt(s);
        norm_out[0] = (float)norm;
        coef_out[0] = (float)fmin(1.0, max_norm / (norm + 1e-6));
    }
}

struct AdamwDev {
    float *theta, *m, *v;
    const float *g, *coef;
    int64_t n;
    double decay, b1, b2, step_size, inv_bc2_sqrt, eps;
    int n_ema;
    float *ema[DLPM_ADAMW_MAX_EMA];
    double mu[DLPM_ADAMW_MAX_EMA];
};

__global__ void __launch_bounds__(256) k_adamw(AdamwDev a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    double g = (double)a.g[i];
    if (a.coef) g *= (double)a.coef[0];
    const double th = (double)a.theta[i] * a.decay;
    const double m = a.b1 * (double)a.m[i] + (1.0 - a.b1) * g;
    const double v = a.b2 * (double)a.v[i] + (1.0 - a.b2) * g * g;
    const double tn = th - a.step_size * m / (sqrt(v) * a.inv_bc2_sqrt + a.eps);
    a.theta[i] = (float)tn;
    a.m[i] = (float)m;
    a.v[i] = (float)v;
    for (int e = 0; e < a.n_ema; e++) a.ema[e][i] = (float)((1.0 - a.mu[e]) * tn + a.mu[e] * (double)a.ema[e][i]);
}

}  // namespace

extern "C" int dlpm_loss_grad_f32(const float *model_eps_dev, const float *target_dev, const float *terms_dev,
                                  const int32_t *median_index_dev, float *dmodel_dev, int64_t B, int32_t outer, int32_t inner, int64_t D,
                                  int32_t lploss, dlpm_stream_t stream) {
    DLPM_CHECK_ARG(model_eps_dev && target_dev && terms_dev && dmodel_dev, "dlpm_loss_grad_f32: null argument");
    DLPM_CHECK_ARG(B > 0 && outer > 0 && inner > 0 && D > 0, "dlpm_loss_grad_f32: B, outer, inner and D must be positive");
    DLPM_CHECK_ARG(lploss == 2 || lploss == 1 || lploss == -1, "dlpm_loss_grad_f32: lploss must be 2, 1 or -1 (got %d)", lploss);
    DLPM_CHECK_ARG(!median_index_dev || outer <= 64, "dlpm_loss_grad_f32: median of means takes outer <= 64 (got %d)", outer);
    const int64_t total = (int64_t)outer * inner * B * D;
    const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(total, 256), 65536);
    k_loss_grad<<<grid, 256, 0, as_stream(stream)>>>(model_eps_dev, target_dev, terms_dev, median_index_dev, dmodel_dev, B, outer, inner,
                                                     D, lploss);
    DLPM_LAUNCH_CHECK();
    return DLPM_OK;
}

extern "C" int dlpm_grad_clip_coef_f32(const float *grad_dev, int64_t n, double max_norm, float *norm_out_dev, float *coef_out_dev,
                                       dlpm_stream_t stream) {
    DLPM_CHECK_ARG(grad_dev && norm_out_dev && coef_out_dev, "dlpm_grad_clip_coef_f32: null argument");
    DLPM_CHECK_ARG(n > 0, "dlpm_grad_clip_coef_f32: n must be positive");
    DLPM_CHECK_ARG(max_norm > 0.0, "dlpm_grad_clip_coef_f32: max_norm must be positive");
    k_grad_clip_coef<<<1, 1024, 0, as_stream(stream)>>>(grad_dev, n, max_norm, norm_out_dev, coef_out_dev);
    DLPM_LAUNCH_CHECK();
    return DLPM_OK;
}

extern "C" int dlpm_adamw_step_f32(const dlpm_adamw_args *p, dlpm_stream_t stream) {
    DLPM_CHECK_ARG(p, "dlpm_adamw_step_f32: null args");
    DLPM_CHECK_ARG(p->theta_dev && p->grad_dev && p->exp_avg_dev && p->exp_avg_sq_dev, "dlpm_adamw_step_f32: null vector");
    DLPM_CHECK_ARG(p->n > 0, "dlpm_adamw_step_f32: n must be positive");
    DLPM_CHECK_ARG(p->n_ema >= 0 && p->n_ema <= DLPM_ADAMW_MAX_EMA, "dlpm_adamw_step_f32: n_ema must be in [0, %d] (got %d)",
                   DLPM_ADAMW_MAX_EMA, p->n_ema);
    DLPM_CHECK_ARG(p->beta1 >= 0.0 && p->beta1 < 1.0 && p->beta2 >= 0.0 && p->beta2 < 1.0, "dlpm_adamw_step_f32: betas must be in [0, 1)");
    DLPM_CHECK_ARG(p->step >= 1, "dlpm_adamw_step_f32: step is 1-based (got %lld)", (long long)p->step);
    DLPM_CHECK_ARG(std::isfinite(p->lr) && p->lr >= 0.0 && std::isfinite(p->eps) && p->eps >= 0.0 && std::isfinite(p->weight_decay) &&
                   p->weight_decay >= 0.0, "dlpm_adamw_step_f32: lr, eps and weight_decay must be finite and >= 0");
    AdamwDev a;
    for (int e = 0; e < DLPM_ADAMW_MAX_EMA; e++) { a.ema[e] = nullptr; a.mu[e] = 0.0; }
    for (int e = 0; e < p->n_ema; e++) {
        DLPM_CHECK_ARG(p->ema_dev[e], "dlpm_adamw_step_f32: null EMA shadow %d", e);
        DLPM_CHECK_ARG(p->ema_mu[e] >= 0.0 && p->ema_mu[e] <= 1.0, "dlpm_adamw_step_f32: EMA rate %d outside [0, 1]", e);
        a.ema[e] = p->ema_dev[e];
        a.mu[e] = p->ema_mu[e];
    }
    a.theta = p->theta_dev; a.m = p->exp_avg_dev; a.v = p->exp_avg_sq_dev; a.g = p->grad_dev; a.coef = p->coef_dev;
    a.n = p->n; a.n_ema = p->n_ema;
    a.decay = 1.0 - p->lr * p->weight_decay;
    a.b1 = p->beta1; a.b2 = p->beta2; a.eps = p->eps;
    a.step_size = p->lr / (1.0 - std::pow(p->beta1, (double)p->step));
    a.inv_bc2_sqrt = 1.0 / std::sqrt(1.0 - std::pow(p->beta2, (double)p->step));
    k_adamw<<<(unsigned)ceil_div(p->n, 256), 256, 0, as_stream(stream)>>>(a);
    DLPM_LAUNCH_CHECK();
    return DLPM_OK;
}
