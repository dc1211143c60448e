// mlp_general_grad.hip -- the backward of the general toy-net forward (mlp_general.hip) on the fp32 MFMA (include/dlpm_amd_mlp_grad.h,
// DESIGN 3.21; the entry points and the flat parameter vector: mlp_train.hip).
//
// Row pass (k_mlp_general_backward).  The forward's tile ownership: one workgroup owns 16 MT rows for the whole net, wave w the
// same NT column tiles of every layer.  It recomputes the forward with the building blocks of mlp_general.h -- the very operations
// of k_mlp_general -- leaving per row in the workspace what the weight gradients need (every Linear's input, every LayerNorm's
// normalised value and 1 / sigma), then walks back.  Every hidden dX = dY W is gemm_tiles over the dY tile in the activation
// image against the transposed operand of the blob's second region (mlp_pack.h: MlpGenGradLayout); the dtemb sum over the blocks
// is kept in the time-embedding image.  Linear(1,TE), Linear(F,nunits) and Linear(nunits,F) stay on the VALU as in the forward.
// A row's dx depends on that row alone, for the reasons the forward's output does.  Rows past the end of a ragged tile are zeros
// with dout = 0 and write nothing.
//
// Weight pass.  k_gen_wgrad: every dW = dY^T A as 16x16x4 fp32 MFMAs whose reduction runs over the rows -- both operands are read
// straight from the row records, 16 consecutive columns of 4 consecutive rows per load.  Chunks of GEN_GRAD_RC rows accumulate in
// fp32, the chunk partials of a slot are added in chunk order in fp64 (mlp_pack.h: the slots).  k_gen_wgrad_cols: biases and
// LayerNorm weights and biases, single columns, in fp64 throughout.  k_gen_wgrad_sum: the slots in order in fp64, rounded once.
// No atomics anywhere.
#include <vector>

#include "mlp_general.h"
#include "../../include/dlpm_amd_mlp.h"
#include "../../include/dlpm_amd_mlp_grad.h"
#include "../../include/dlpm_amd_train.h"

using namespace dlpm;

namespace {

struct GradArgs {
    const float *P;          // the blob: the forward's region, then the transposed operands
    MlpGenLayout L;
    MlpGenGradLayout G;
    MlpGenRecords R;
    MlpFlat f;
    const float *x, *t, *dout;
    float *dx;               // nullable
    float *ws;               // the records
    double *part;            // [slots][P]
    int64_t B, rows_per_slot;
    int ln, skip, slots;
};

template <int MT, int NT>
__global__ void __launch_bounds__(64 * GEN_MAX_WAVES) k_mlp_general_backward(GradArgs a) {
    extern __shared__ __attribute__((aligned(16))) float gen_lds[];
    constexpr int M = 16 * MT;
    const MlpGenLayout &L = a.L;
    const MlpGenRecords &R = a.R;
    const int F = L.F, NP = L.NP, TEP = L.TEP, LD = L.LD, LDT = L.LDT, W = L.W, NU = L.NU;
    float *A = gen_lds;                 // [M][LD] activations; in the walk back the dY tile
    float *temb = A + M * LD;           // [M][LDT] time embedding; in the walk back dL/d(temb)
    float *xs = temb + M * LDT;         // [M][F] x; in the walk back dout
    float *ts = xs + M * F;             // [M]
    float *part = ts + M;               // [2][W][M] row partial sums
    const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, w = tid >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * M, B = a.B;
    const float *__restrict__ P = a.P;
    const float *__restrict__ PT = a.P + a.G.base;
    const int KG = NP / 16, KGT = TEP / 16;
    const int q4 = 4 * (lane >> 4);
    float *ws = a.ws;

    int col[NT];
#pragma unroll
    for (int n = 0; n < NT; n++) col[n] = 16 * (w * NT + n) + (lane & 15);
    // record `off` (width NP), this thread's elements; dead rows write nothing and read zeros
    auto put = [&](int64_t off, const floatx4 (&v)[MT][NT]) {
#pragma unroll
        for (int m = 0; m < MT; m++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int64_t row = r0 + 16 * m + q4 + r;
                if (row < B)
#pragma unroll
                    for (int n = 0; n < NT; n++) ws[off * B + row * NP + col[n]] = v[m][n][r];
            }
    };
    auto get = [&](int64_t off, floatx4 (&v)[MT][NT]) {
#pragma unroll
        for (int m = 0; m < MT; m++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int64_t row = r0 + 16 * m + q4 + r;
#pragma unroll
                for (int n = 0; n < NT; n++) v[m][n][r] = row < B ? ws[off * B + row * NP + col[n]] : 0.f;
            }
    };
    // 1 / sigma of this thread's rows: element e of the 4-wide scalar record `off`; every thread of a row holds the same value and
    // one of them writes it
    auto put_rs = [&](int64_t off, int e, const float (&rs)[MT][4]) {
        if (w == 0 && (lane & 15) == 0)
#pragma unroll
            for (int m = 0; m < MT; m++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int64_t row = r0 + 16 * m + q4 + r;
                    if (row < B) ws[off * B + row * 4 + e] = rs[m][r];
                }
    };
    auto get_rs = [&](int64_t off, int e, float (&rs)[MT][4]) {
#pragma unroll
        for (int m = 0; m < MT; m++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int64_t row = r0 + 16 * m + q4 + r;
                rs[m][r] = row < B ? ws[off * B + row * 4 + e] : 0.f;
            }
    };
    // LayerNorm (or none) with what the backward keeps: record `noff` <- the normalised value (without LayerNorm the value itself)
    auto norm_keep = [&](floatx4 (&v)[MT][NT], const float *gam, const float *bet, int64_t noff, int64_t rsoff, int e) {
        if (a.ln) {
            floatx4 xh[MT][NT];
            float rs[MT][4];
            layer_norm_rows<MT, NT, true>(v, gam, bet, col, NU, part, W, w, lane, xh, rs);
            put(noff, xh);
            put_rs(rsoff, e, rs);
        } else {
            put(noff, v);
            __syncthreads();                          // A is read out, as in the forward
        }
    };
    // dL/d(LayerNorm input) from g = dL/d(LayerNorm output): the row sums in layer_norm_rows' order; padded columns are 0
    auto norm_back = [&](floatx4 (&g)[MT][NT], const floatx4 (&xh)[MT][NT], const float (&rs)[MT][4], const float *gam) {
        const float inv = 1.0f / (float)NU;
        float gm[NT];
#pragma unroll
        for (int n = 0; n < NT; n++) gm[n] = gam[col[n]];
#pragma unroll
        for (int m = 0; m < MT; m++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                float s1 = 0.f, s2 = 0.f;
#pragma unroll
                for (int n = 0; n < NT; n++) {
                    const float d = g[m][n][r] * gm[n];
                    g[m][n][r] = d;
                    s1 += d;
                    s2 += d * xh[m][n][r];
                }
                s1 = row16_sum(s1);
                s2 = row16_sum(s2);
                if ((lane & 15) == 0) {
                    part[w * M + 16 * m + q4 + r] = s1;
                    part[(W + w) * M + 16 * m + q4 + r] = s2;
                }
            }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < MT; m++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                float s1 = 0.f, s2 = 0.f;
                for (int ww = 0; ww < W; ww++) {
                    s1 += part[ww * M + 16 * m + q4 + r];
                    s2 += part[(W + ww) * M + 16 * m + q4 + r];
                }
                const float m1 = s1 * inv, m2 = s2 * inv;
#pragma unroll
                for (int n = 0; n < NT; n++)
                    g[m][n][r] = col[n] < NU ? rs[m][r] * (g[m][n][r] - m1 - xh[m][n][r] * m2) : 0.f;
            }
        __syncthreads();                              // part may be written again
    };

    // ================================================================ forward, operation for operation as k_mlp_general
    for (int i = tid; i < M * F; i += nthr) xs[i] = (r0 * F + i < B * F) ? a.x[r0 * F + i] : 0.f;
    for (int i = tid; i < M; i += nthr) ts[i] = (r0 + i < B) ? a.t[r0 + i] : 0.f;
    __syncthreads();
    for (int i = tid; i < M * TEP; i += nthr) {
        const int row = i / TEP, k = i - row * TEP;
        const float e = silu(fmaf(P[L.te_w + k], ts[row], P[L.te_b + k]));
        A[row * LD + k] = e;
        if (r0 + row < B) ws[R.e0 * B + (r0 + row) * TEP + k] = e;
    }
    __syncthreads();
    for (int j = w; j < KGT; j += W) {
        floatx4 acc[MT][1];
        const float b = P[L.tm_b + 16 * j + (lane & 15)];
#pragma unroll
        for (int m = 0; m < MT; m++) acc[m][0] = floatx4{b, b, b, b};
        gemm_tiles<MT, 1>(reinterpret_cast<const float4 *>(P + L.tm_w) + (int64_t)j * KGT * 64, KGT, A, LD, lane, acc);
#pragma unroll
        for (int m = 0; m < MT; m++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int row = 16 * m + q4 + r, k = 16 * j + (lane & 15);
                const float te = silu(acc[m][0][r]);
                temb[row * LDT + k] = te;
                if (r0 + row < B) {
                    ws[R.a1 * B + (r0 + row) * TEP + k] = acc[m][0][r];
                    ws[R.temb * B + (r0 + row) * TEP + k] = te;
                }
            }
    }
    __syncthreads();

    floatx4 h[MT][NT];
    {
#pragma unroll
        for (int n = 0; n < NT; n++) {
            const float b = P[L.in_b + col[n]];
#pragma unroll
            for (int m = 0; m < MT; m++) h[m][n] = floatx4{b, b, b, b};
        }
        for (int f = 0; f < F; f++) {
#pragma unroll
            for (int n = 0; n < NT; n++) {
                const float wv = P[L.in_w + (int64_t)f * NP + col[n]];
#pragma unroll
                for (int m = 0; m < MT; m++)
#pragma unroll
                    for (int r = 0; r < 4; r++) h[m][n][r] = fmaf(wv, xs[(16 * m + q4 + r) * F + f], h[m][n][r]);
            }
        }
        if (a.ln) {
            floatx4 xh[MT][NT];
            float rs[MT][4];
            layer_norm_rows<MT, NT, true>(h, P + L.in_g, P + L.in_be, col, NU, part, W, w, lane, xh, rs);
            put(R.nin, xh);
            put_rs(R.rsin, 0, rs);
        } else {
            put(R.nin, h);
        }
#pragma unroll
        for (int m = 0; m < MT; m++)
#pragma unroll
            for (int n = 0; n < NT; n++)
#pragma unroll
                for (int r = 0; r < 4; r++) h[m][n][r] = silu(h[m][n][r]);
    }
    for (int bi = 0; bi < L.nblk; bi++) {
        const float *__restrict__ Q = P + L.blk0 + (int64_t)bi * L.blk_stride;
        const int64_t rb = R.blk0 + (int64_t)bi * R.blk_stride;
        put(rb + R.b_h, h);
        store_tiles<MT, NT>(A, LD, h, col, lane);
        __syncthreads();
        floatx4 y[MT][NT];
#pragma unroll
        for (int n = 0; n < NT; n++) {
            const float b = Q[L.b_b1 + col[n]];
#pragma unroll
            for (int m = 0; m < MT; m++) y[m][n] = floatx4{b, b, b, b};
        }
        gemm_tiles<MT, NT>(reinterpret_cast<const float4 *>(Q + L.b_w1) + (int64_t)w * NT * KG * 64, KG, A, LD, lane, y);
        norm_keep(y, Q + L.b_g1, Q + L.b_be1, rb + R.b_n1, rb + R.b_rs, 0);
        {
            floatx4 tpv[MT][NT];
#pragma unroll
            for (int n = 0; n < NT; n++) {
                floatx4 tp[MT][1];
                const float b = Q[L.b_tb + col[n]];
#pragma unroll
                for (int m = 0; m < MT; m++) tp[m][0] = floatx4{b, b, b, b};
                gemm_tiles<MT, 1>(reinterpret_cast<const float4 *>(Q + L.b_tw) + (int64_t)(w * NT + n) * KGT * 64, KGT, temb, LDT, lane, tp);
#pragma unroll
                for (int m = 0; m < MT; m++) {
                    tpv[m][n] = tp[m][0];
#pragma unroll
                    for (int r = 0; r < 4; r++) y[m][n][r] = silu(y[m][n][r]) + silu(tp[m][0][r]);
                }
            }
            put(rb + R.b_tp, tpv);
        }
        put(rb + R.b_y, y);
        store_tiles<MT, NT>(A, LD, y, col, lane);
        __syncthreads();
#pragma unroll
        for (int n = 0; n < NT; n++) {
            const float b = Q[L.b_b2 + col[n]];
#pragma unroll
            for (int m = 0; m < MT; m++) y[m][n] = floatx4{b, b, b, b};
        }
        gemm_tiles<MT, NT>(reinterpret_cast<const float4 *>(Q + L.b_w2) + (int64_t)w * NT * KG * 64, KG, A, LD, lane, y);
        norm_keep(y, Q + L.b_g2, Q + L.b_be2, rb + R.b_n2, rb + R.b_rs, 1);
#pragma unroll
        for (int m = 0; m < MT; m++)
#pragma unroll
            for (int n = 0; n < NT; n++)
#pragma unroll
                for (int r = 0; r < 4; r++) h[m][n][r] = silu(a.skip ? y[m][n][r] + h[m][n][r] : y[m][n][r]);
    }
    put(R.hfin, h);

    // ================================================================ backward
    // every wave is past its reads of A, temb and xs: a barrier closed the last layer
    for (int i = tid; i < M * F; i += nthr) xs[i] = (r0 * F + i < B * F) ? a.dout[r0 * F + i] : 0.f;
    for (int i = tid; i < M * TEP; i += nthr) {
        const int row = i / TEP, k = i - row * TEP;
        temb[row * LDT + k] = 0.f;
    }
    __syncthreads();
    floatx4 dh[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; m++)
#pragma unroll
        for (int n = 0; n < NT; n++) dh[m][n] = floatx4{0.f, 0.f, 0.f, 0.f};
    for (int f = 0; f < F; f++) {       // out[f] = sum_n out_w[f][n] h[n] + b[f]
#pragma unroll
        for (int n = 0; n < NT; n++) {
            const float wv = P[L.out_w + (int64_t)f * NP + col[n]];
#pragma unroll
            for (int m = 0; m < MT; m++)
#pragma unroll
                for (int r = 0; r < 4; r++) dh[m][n][r] = fmaf(wv, xs[(16 * m + q4 + r) * F + f], dh[m][n][r]);
        }
    }
    for (int bi = L.nblk - 1; bi >= 0; bi--) {
        const float *__restrict__ Q = P + L.blk0 + (int64_t)bi * L.blk_stride;
        const float *__restrict__ QT = PT + a.G.blk0 + (int64_t)bi * a.G.blk_stride;
        const int64_t rb = R.blk0 + (int64_t)bi * R.blk_stride;
        floatx4 nv[MT][NT], ds[MT][NT];
        float rs[MT][4];
        // h_out = silu(LN2(W2 y + b2) [+ h_in])
        get(rb + R.b_n2, nv);
        {
            floatx4 hin[MT][NT];
            if (a.skip) get(rb + R.b_h, hin);
#pragma unroll
            for (int n = 0; n < NT; n++) {
                const float g2 = a.ln ? Q[L.b_g2 + col[n]] : 1.f, be2 = a.ln ? Q[L.b_be2 + col[n]] : 0.f;
#pragma unroll
                for (int m = 0; m < MT; m++)
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        float pre = a.ln ? nv[m][n][r] * g2 + be2 : nv[m][n][r];
                        if (a.skip) pre = pre + hin[m][n][r];
                        ds[m][n][r] = dh[m][n][r] * dsilu(pre);
                    }
            }
        }
#pragma unroll
        for (int m = 0; m < MT; m++)
#pragma unroll
            for (int n = 0; n < NT; n++) dh[m][n] = ds[m][n];                // dh: now dL/d(LN2 output), soon dL/d(W2 y + b2)
        if (a.ln) {
            put(rb + R.b_dln2, dh);
            get_rs(rb + R.b_rs, 1, rs);
            norm_back(dh, nv, rs, Q + L.b_g2);
        }
        put(rb + R.b_dz2, dh);
        store_tiles<MT, NT>(A, LD, dh, col, lane);
        __syncthreads();
#pragma unroll
        for (int m = 0; m < MT; m++)
#pragma unroll
            for (int n = 0; n < NT; n++) dh[m][n] = floatx4{0.f, 0.f, 0.f, 0.f};
        // dy[k] = sum_n dz[n] W2[n][k]
        gemm_tiles<MT, NT>(reinterpret_cast<const float4 *>(QT + a.G.b_w2T) + (int64_t)w * NT * KG * 64, KG, A, LD, lane, dh);
        __syncthreads();
        // y = silu(LN1(W1 h_in + b1)) + silu(Wt temb + tb)
        {
            floatx4 dtp[MT][NT];
            get(rb + R.b_tp, dtp);
#pragma unroll
            for (int m = 0; m < MT; m++)
#pragma unroll
                for (int n = 0; n < NT; n++)
#pragma unroll
                    for (int r = 0; r < 4; r++) dtp[m][n][r] = dh[m][n][r] * dsilu(dtp[m][n][r]);
            put(rb + R.b_dtp, dtp);
            store_tiles<MT, NT>(A, LD, dtp, col, lane);
        }
        __syncthreads();
        for (int j = w; j < KGT; j += W) {      // dtemb[k] += sum_n dtp[n] Wt[n][k], tile j of the time embedding's columns
            floatx4 acc[MT][1];
#pragma unroll
            for (int m = 0; m < MT; m++)
#pragma unroll
                for (int r = 0; r < 4; r++) acc[m][0][r] = temb[(16 * m + q4 + r) * LDT + 16 * j + (lane & 15)];
            gemm_tiles<MT, 1>(reinterpret_cast<const float4 *>(QT + a.G.b_twT) + (int64_t)j * KG * 64, KG, A, LD, lane, acc);
#pragma unroll
            for (int m = 0; m < MT; m++)
#pragma unroll
                for (int r = 0; r < 4; r++) temb[(16 * m + q4 + r) * LDT + 16 * j + (lane & 15)] = acc[m][0][r];
        }
        get(rb + R.b_n1, nv);
#pragma unroll
        for (int n = 0; n < NT; n++) {
            const float g1 = a.ln ? Q[L.b_g1 + col[n]] : 1.f, be1 = a.ln ? Q[L.b_be1 + col[n]] : 0.f;
#pragma unroll
            for (int m = 0; m < MT; m++)
#pragma unroll
                for (int r = 0; r < 4; r++) dh[m][n][r] = dh[m][n][r] * dsilu(a.ln ? nv[m][n][r] * g1 + be1 : nv[m][n][r]);
        }
        __syncthreads();                        // A (the dtp tile) is read out
        if (a.ln) {
            put(rb + R.b_dln1, dh);
            get_rs(rb + R.b_rs, 0, rs);
            norm_back(dh, nv, rs, Q + L.b_g1);
        }
        put(rb + R.b_dz1, dh);
        store_tiles<MT, NT>(A, LD, dh, col, lane);
        __syncthreads();
#pragma unroll
        for (int m = 0; m < MT; m++)
#pragma unroll
            for (int n = 0; n < NT; n++)
#pragma unroll
                for (int r = 0; r < 4; r++) dh[m][n][r] = a.skip ? ds[m][n][r] : 0.f;      // the skip
        gemm_tiles<MT, NT>(reinterpret_cast<const float4 *>(QT + a.G.b_w1T) + (int64_t)w * NT * KG * 64, KG, A, LD, lane, dh);
        __syncthreads();
    }
    {   // h_0 = silu(LN(W_in x + b))
        floatx4 nv[MT][NT];
        float rs[MT][4];
        get(R.nin, nv);
#pragma unroll
        for (int n = 0; n < NT; n++) {
            const float g = a.ln ? P[L.in_g + col[n]] : 1.f, be = a.ln ? P[L.in_be + col[n]] : 0.f;
#pragma unroll
            for (int m = 0; m < MT; m++)
#pragma unroll
                for (int r = 0; r < 4; r++) dh[m][n][r] = dh[m][n][r] * dsilu(a.ln ? nv[m][n][r] * g + be : nv[m][n][r]);
        }
        if (a.ln) {
            put(R.dlnin, dh);
            get_rs(R.rsin, 0, rs);
            norm_back(dh, nv, rs, P + L.in_g);
        }
        put(R.dzin, dh);
        if (a.dx) {     // dx[f] = sum_n dz[n] in_w[f][n]: per wave a partial over its columns, then the waves in order (through A)
            for (int f = 0; f < F; f++) {
                float wv[NT];
#pragma unroll
                for (int n = 0; n < NT; n++) wv[n] = P[L.in_w + (int64_t)f * NP + col[n]];
#pragma unroll
                for (int m = 0; m < MT; m++)
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        float s = 0.f;
#pragma unroll
                        for (int n = 0; n < NT; n++) s = fmaf(dh[m][n][r], wv[n], s);
                        s = row16_sum(s);
                        if ((lane & 15) == 0) A[(w * M + 16 * m + q4 + r) * F + f] = s;
                    }
            }
            __syncthreads();
            for (int i = tid; i < M * F; i += nthr) {
                const int row = i / F, f = i - row * F;
                float s = 0.f;
                for (int ww = 0; ww < W; ww++) s += A[(ww * M + row) * F + f];
                if (r0 + row < B) a.dx[(r0 + row) * F + f] = s;
            }
        }
    }
    __syncthreads();
    // temb = silu(a1), a1 = Wtm e0 + b, e0 = silu(a0), a0 = w t + b
    for (int i = tid; i < M * TEP; i += nthr) {
        const int row = i / TEP, k = i - row * TEP;
        float d = 0.f;
        if (r0 + row < B) {
            d = temb[row * LDT + k] * dsilu(ws[R.a1 * B + (r0 + row) * TEP + k]);
            ws[R.da1 * B + (r0 + row) * TEP + k] = d;
        }
        temb[row * LDT + k] = d;
    }
    __syncthreads();
    for (int j = w; j < KGT; j += W) {
        floatx4 acc[MT][1];
#pragma unroll
        for (int m = 0; m < MT; m++) acc[m][0] = floatx4{0.f, 0.f, 0.f, 0.f};
        gemm_tiles<MT, 1>(reinterpret_cast<const float4 *>(PT + a.G.tm_wT) + (int64_t)j * KGT * 64, KGT, temb, LDT, lane, acc);
#pragma unroll
        for (int m = 0; m < MT; m++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int row = 16 * m + q4 + r, k = 16 * j + (lane & 15);
                if (r0 + row < B)
                    ws[R.da0 * B + (r0 + row) * TEP + k] = acc[m][0][r] * dsilu(fmaf(P[L.te_w + k], ts[row], P[L.te_b + k]));
            }
    }
}

// ------------------------------------------------------------------------------------------------ weight pass
// dW[n][k] = sum_r Y[r][n] A[r][k] into flat[out + n K + k]
struct MatJob {
    const float *Y, *A;
    int64_t ldY, ldA, out;
    int N, K;
};
// c[n] = sum_r Y[r][n] -> flat[outC + n]; d[n] = sum_r Y[r][n] Yd[r][n] -> flat[outD + n]
struct ColJob {
    const float *Y, *Yd;
    int64_t ldY, outC, outD;
    int N;
};

__device__ MatJob mat_job(const GradArgs &a, int j) {
    const MlpGenLayout &L = a.L;
    const MlpGenRecords &R = a.R;
    const MlpFlat &f = a.f;
    const int64_t B = a.B;
    auto rec = [&](int64_t off) { return a.ws + off * B; };
    MatJob b;
    if (j == 0) {            // time_emb: Linear(1, TE)
        b.Y = rec(R.da0); b.ldY = L.TEP; b.N = L.TE; b.A = a.t; b.ldA = 1; b.K = 1; b.out = f.te_w;
    } else if (j == 1) {     // time_mlp.2
        b.Y = rec(R.da1); b.ldY = L.TEP; b.N = L.TE; b.A = rec(R.e0); b.ldA = L.TEP; b.K = L.TE; b.out = f.tm_w;
    } else if (j == 2) {     // linear_in
        b.Y = rec(R.dzin); b.ldY = L.NP; b.N = L.NU; b.A = a.x; b.ldA = L.F; b.K = L.F; b.out = f.in_w;
    } else if (j == 3) {     // outblocks_mean.1.weight [F][NU] = sum_r dout[r][f] h[r][n]
        b.Y = a.dout; b.ldY = L.F; b.N = L.F; b.A = rec(R.hfin); b.ldA = L.NP; b.K = L.NU; b.out = f.out_w;
    } else {
        const int bi = (j - 4) / 3, which = (j - 4) % 3;
        const int64_t rb = R.blk0 + (int64_t)bi * R.blk_stride, fb = f.blk0 + (int64_t)bi * f.blk_stride;
        // selects, not a third level of branches: hipcc (ROCm 7.2) lowers the nested if-chain with the last branch reading the
        // middle one's K (seen in the ISA and on the device: mlp_2's gradient came out with time_emb_size columns)
        const bool w1 = which == 0, tw = which == 1;
        b.ldY = L.NP; b.N = L.NU;
        b.Y = rec(rb + (w1 ? R.b_dz1 : tw ? R.b_dtp : R.b_dz2));
        b.A = tw ? rec(R.temb) : rec(rb + (w1 ? R.b_h : R.b_y));
        b.ldA = tw ? L.TEP : L.NP;
        b.K = tw ? L.TE : L.NU;
        b.out = fb + (w1 ? f.b_w1 : tw ? f.b_tw : f.b_w2);
    }
    return b;
}

__device__ ColJob col_job(const GradArgs &a, int j) {
    const MlpGenLayout &L = a.L;
    const MlpGenRecords &R = a.R;
    const MlpFlat &f = a.f;
    const int64_t B = a.B;
    auto rec = [&](int64_t off) { return a.ws + off * B; };
    ColJob c;
    c.Yd = nullptr; c.outD = -1; c.ldY = L.NP; c.N = L.NU;
    const int nb = L.nblk;
    if (j == 0) {
        c.Y = rec(R.da0); c.ldY = L.TEP; c.N = L.TE; c.outC = f.te_b;
    } else if (j == 1) {
        c.Y = rec(R.da1); c.ldY = L.TEP; c.N = L.TE; c.outC = f.tm_b;
    } else if (j == 2) {
        c.Y = rec(R.dzin); c.outC = f.in_b;
    } else if (j == 3) {
        c.Y = a.dout; c.ldY = L.F; c.N = L.F; c.outC = f.out_b;
    } else if (j < 4 + 3 * nb) {
        const int bi = (j - 4) / 3, which = (j - 4) % 3;
        const int64_t rb = R.blk0 + (int64_t)bi * R.blk_stride, fb = f.blk0 + (int64_t)bi * f.blk_stride;
        c.Y = rec(rb + (which == 0 ? R.b_dz1 : which == 1 ? R.b_dtp : R.b_dz2));
        c.outC = fb + (which == 0 ? f.b_b1 : which == 1 ? f.b_tb : f.b_b2);
    } else if (j == 4 + 3 * nb) {        // the LayerNorms (only launched with LayerNorm on)
        c.Y = rec(R.dlnin); c.Yd = rec(R.nin); c.outC = f.in_be; c.outD = f.in_g;
    } else {
        const int q = j - (5 + 3 * nb), bi = q / 2, which = q % 2;
        const int64_t rb = R.blk0 + (int64_t)bi * R.blk_stride, fb = f.blk0 + (int64_t)bi * f.blk_stride;
        c.Y = rec(rb + (which ? R.b_dln2 : R.b_dln1)); c.Yd = rec(rb + (which ? R.b_n2 : R.b_n1));
        c.outC = fb + (which ? f.b_be2 : f.b_be1); c.outD = fb + (which ? f.b_g2 : f.b_g1);
    }
    return c;
}

constexpr int WG_ZSPLIT = 16;   // workgroups that share the tiles of one matrix and slot
constexpr int WG_KT = 4;        // a wave's tile: 16 n x 64 k

// grid (matrix jobs, slots, WG_ZSPLIT), 4 waves: wave tiles are dealt round-robin over z and the waves
__global__ void __launch_bounds__(256) k_gen_wgrad(GradArgs a) {
    const MatJob b = mat_job(a, blockIdx.x);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int slot = blockIdx.y;
    const int64_t rbeg = (int64_t)slot * a.rows_per_slot, rend = min(a.B, rbeg + a.rows_per_slot);
    double *part = a.part + (int64_t)slot * a.f.P;
    const int ntk = (b.K + 16 * WG_KT - 1) / (16 * WG_KT), ntn = (b.N + 15) / 16;
    const int lr = lane >> 4, lc = lane & 15;
    for (int tile = blockIdx.z * 4 + wave; tile < ntn * ntk; tile += 4 * WG_ZSPLIT) {
        const int n0 = (tile / ntk) * 16, k0 = (tile % ntk) * 16 * WG_KT;
        double acc64[WG_KT][4];
#pragma unroll
        for (int q = 0; q < WG_KT; q++)
#pragma unroll
            for (int r = 0; r < 4; r++) acc64[q][r] = 0.0;
        const bool nok = n0 + lc < b.N;
        for (int64_t c0 = rbeg; c0 < rend; c0 += GEN_GRAD_RC) {
            const int64_t c1 = min(rend, c0 + GEN_GRAD_RC);
            floatx4 acc[WG_KT];
#pragma unroll
            for (int q = 0; q < WG_KT; q++) acc[q] = floatx4{0.f, 0.f, 0.f, 0.f};
            for (int64_t r = c0; r < c1; r += 4) {
                const int64_t rr = r + lr;
                const bool ok = rr < c1;
                const float y = (ok && nok) ? b.Y[rr * b.ldY + n0 + lc] : 0.f;
#pragma unroll
                for (int q = 0; q < WG_KT; q++) {
                    const int k = k0 + 16 * q + lc;
                    const float v = (ok && k < b.K) ? b.A[rr * b.ldA + k] : 0.f;
                    acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(y, v, acc[q], 0, 0, 0);
                }
            }
#pragma unroll
            for (int q = 0; q < WG_KT; q++)
#pragma unroll
                for (int r = 0; r < 4; r++) acc64[q][r] += (double)acc[q][r];
        }
#pragma unroll
        for (int q = 0; q < WG_KT; q++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int n = n0 + 4 * lr + r, k = k0 + 16 * q + lc;
                if (n < b.N && k < b.K) part[b.out + (int64_t)n * b.K + k] = acc64[q][r];
            }
    }
}

// grid (column jobs, slots)
__global__ void __launch_bounds__(256) k_gen_wgrad_cols(GradArgs a) {
    const ColJob c = col_job(a, blockIdx.x);
    const int slot = blockIdx.y;
    const int64_t rbeg = (int64_t)slot * a.rows_per_slot, rend = min(a.B, rbeg + a.rows_per_slot);
    double *part = a.part + (int64_t)slot * a.f.P;
    for (int n = threadIdx.x; n < c.N; n += 256) {
        double s = 0.0, d = 0.0;
        for (int64_t r = rbeg; r < rend; r++) {
            const double y = (double)c.Y[r * c.ldY + n];
            s += y;
            if (c.Yd) d += y * (double)c.Yd[r * c.ldY + n];
        }
        part[c.outC + n] = s;
        if (c.outD >= 0) part[c.outD + n] = d;
    }
}

__global__ void __launch_bounds__(256) k_gen_wgrad_sum(const double *__restrict__ part, float *__restrict__ grad, int64_t P, int slots) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    double s = 0.0;
    for (int c = 0; c < slots; c++) s += part[(int64_t)c * P + i];
    grad[i] = (float)s;
}

// the tile height of the backward: the forward's choice, but 16 rows where a wave owns 8 column tiles (registers)
int grad_tile_rows(const dlpm_mlp *m, int64_t rows) {
    if (m->gen.NT == 8 && !(m->flags & DLPM_MLP_TILE_32)) return 16;
    return (m->gen_M == 32 && !(m->flags & DLPM_MLP_TILE_32) && ceil_div(rows, 32) < GEN_FILL_TILES) ? 16 : m->gen_M;
}

template <int MT>
int launch_backward(const dlpm_mlp *m, const char *name, const GradArgs &a, unsigned grid, size_t lds, hipStream_t st) {
    void (*fn)(GradArgs) = nullptr;
    switch (m->gen.NT) {
        case 1: fn = k_mlp_general_backward<MT, 1>; break;
        case 2: fn = k_mlp_general_backward<MT, 2>; break;
        case 4: fn = k_mlp_general_backward<MT, 4>; break;
        case 8: fn = k_mlp_general_backward<MT, 8>; break;
    }
    if (!fn) {
        set_error("%s: no general kernel for %d column tiles per wave", name, m->gen.NT);
        return DLPM_ERR_UNSUPPORTED;
    }
    const int r = ensure_dynamic_lds(reinterpret_cast<const void *>(fn), GEN_LDS_LIMIT);
    if (r != DLPM_OK) return r;
    fn<<<grid, 64 * m->gen.W, lds, st>>>(a);
    DLPM_LAUNCH_CHECK();
    return DLPM_OK;
}

}  // namespace

namespace dlpm {

int64_t mlp_general_workspace_bytes(const dlpm_mlp *m, const char *name, int64_t rows) {
    const int M = grad_tile_rows(m, rows);
    const int64_t lds = mlp_gen_grad_lds_bytes(m->gen, M);
    if ((M != 16 && M != 32) || lds > GEN_LDS_LIMIT) {
        set_error("%s: a %d-row tile of this net's backward takes %lld bytes of LDS, a workgroup has %d", name, M, (long long)lds,
                  GEN_LDS_LIMIT);
        return DLPM_ERR_UNSUPPORTED;
    }
    return mlp_gen_grad_workspace_bytes(m->gen, mlp_flat_of(m), rows);
}

int mlp_general_backward(dlpm_mlp *m, const char *name, const float *x_dev, const float *t_dev, const float *dout_dev, int64_t rows,
                         float *grad_flat_dev, float *dx_dev, void *workspace_dev, int64_t workspace_bytes, hipStream_t st) {
    const int M = grad_tile_rows(m, rows);
    const int64_t lds = mlp_gen_grad_lds_bytes(m->gen, M);
    if ((M != 16 && M != 32) || lds > GEN_LDS_LIMIT) {
        set_error("%s: a %d-row tile of this net's backward takes %lld bytes of LDS, a workgroup has %d", name, M, (long long)lds,
                  GEN_LDS_LIMIT);
        return DLPM_ERR_UNSUPPORTED;
    }
    const int64_t grid = ceil_div(rows, M);
    DLPM_CHECK_ARG(grid < (1ll << 31), "%s: rows = %lld is beyond the grid of one call", name, (long long)rows);
    GradArgs a;
    a.f = mlp_flat_of(m);
    const int64_t need = mlp_gen_grad_workspace_bytes(m->gen, a.f, rows);
    if (workspace_bytes < need) {
        set_error("%s: the workspace has %lld bytes, %lld are needed", name, (long long)workspace_bytes, (long long)need);
        return DLPM_ERR_NOMEM;
    }
    DLPM_CHECK_ARG(reinterpret_cast<uintptr_t>(workspace_dev) % 8 == 0, "%s: the workspace must be 8-byte aligned", name);
    DLPM_MLP_NEED_FINALIZED(m, name);
    a.P = m->gen_dev; a.L = m->gen; a.G = mlp_gen_grad_layout(m->gen); a.R = mlp_gen_records(m->gen);
    a.x = x_dev; a.t = t_dev; a.dout = dout_dev; a.dx = dx_dev;
    a.ws = static_cast<float *>(workspace_dev);
    a.part = reinterpret_cast<double *>(a.ws + (a.R.per_row * rows + 1) / 2 * 2);
    a.B = rows; a.ln = m->ln; a.skip = m->skip;
    mlp_gen_grad_slots(rows, &a.slots, &a.rows_per_slot);
    if (int rc = M == 32 ? launch_backward<2>(m, name, a, (unsigned)grid, (size_t)lds, st) : launch_backward<1>(m, name, a, (unsigned)grid, (size_t)lds, st))
        return rc;
    const int nb = m->gen.nblk;
    k_gen_wgrad<<<dim3(4 + 3 * nb, a.slots, WG_ZSPLIT), 256, 0, st>>>(a);
    DLPM_LAUNCH_CHECK();
    k_gen_wgrad_cols<<<dim3(4 + 3 * nb + (m->ln ? 1 + 2 * nb : 0), a.slots), 256, 0, st>>>(a);
    DLPM_LAUNCH_CHECK();
    k_gen_wgrad_sum<<<(unsigned)ceil_div(a.f.P, 256), 256, 0, st>>>(a.part, grad_flat_dev, a.f.P, a.slots);
    DLPM_LAUNCH_CHECK();
    return DLPM_OK;
}

}  // namespace dlpm
