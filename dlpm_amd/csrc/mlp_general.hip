// mlp_general.hip -- MLPModel.forward (dlpm/models/Model.py:148-211, DiffusionBlocks.py:125-136) at any width, on the fp32 MFMA
// (include/dlpm_amd_mlp.h).  The lane kernels of mlp.hip keep the shipped 64-unit net; this file takes every other
// architecture: nunits and time_emb_size 1 .. 1024, nfeatures 1 .. 64, nblocks >= 0, LayerNorm and skip on or off.
//
// Mapping.  One workgroup owns M = 16 MT rows (MT = 1 or 2) for the whole net.  Its W <= 8 waves split the NP = 16 W NT padded
// output columns: wave w owns the NT column tiles w NT .. w NT + NT - 1 of EVERY layer, so the element (row, column) of every
// activation -- the skip value among them -- belongs to one thread throughout and the skip stays in registers.  A Linear is, per
// group of 16 k: MT 16-byte LDS reads (A fragments), NT 16-byte weight loads from the packed blob (B fragments, shared by all
// workgroups, L2-resident) and 4 MT NT v_mfma_f32_16x16x4_f32.  The activations pass from layer to layer through ONE LDS image
// [M][LD]; the barriers of the LayerNorm reductions are also the ones that order its reads and writes.
// K and N are zero-padded in the blob (mlp_pack.h), never in the loops: a padded column has zero weights, bias, gamma and beta,
// so it is exactly 0 after every layer and feeds zeros to the next.
//
// A row's bits depend on that row alone: an MFMA output row is a k-ordered fma chain over its own A row, the LayerNorm sums of a
// row go over the thread's tiles, a 16-lane butterfly and the waves in order, and neither M nor the row's place in the tile enters.
#include <cstring>

#include "mlp_general.h"
#include "../../include/dlpm_amd_mlp.h"

using namespace dlpm;

namespace {

template <int MT, int NT>
__global__ void __launch_bounds__(64 * GEN_MAX_WAVES) k_mlp_general(GenArgs a) {
    extern __shared__ __attribute__((aligned(16))) float gen_lds[];
    constexpr int M = 16 * MT;
    const MlpGenLayout &L = a.L;
    const int F = L.F, NP = L.NP, TEP = L.TEP, LD = L.LD, LDT = L.LDT, W = L.W;
    float *A = gen_lds;                 // [M][LD] activations (first the time embedding's first layer, last the output partials)
    float *temb = A + M * LD;           // [M][LDT] time embedding
    float *xs = temb + M * LDT;         // [M][F]
    float *ts = xs + M * F;             // [M]
    float *part = ts + M;               // [2][W][M] LayerNorm partial sums
    const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, w = tid >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * M;
    const float *__restrict__ P = a.P;
    const int KG = NP / 16, KGT = TEP / 16;

    // ---- the tile's inputs; the dead rows of a ragged last tile are zeros
    for (int i = tid; i < M * F; i += nthr) xs[i] = (r0 * F + i < a.B * F) ? a.x[r0 * F + i] : 0.f;
    for (int i = tid; i < M; i += nthr) ts[i] = (r0 + i < a.B) ? a.t[r0 + i] : 0.f;
    __syncthreads();

    // ---- time embedding (Model.py:62,68-72,192): Linear(1,TE) -> SiLU on the VALU, Linear(TE,TE) -> SiLU on the MFMA
    for (int i = tid; i < M * TEP; i += nthr) {
        const int row = i / TEP, k = i - row * TEP;
        A[row * LD + k] = silu(fmaf(P[L.te_w + k], ts[row], P[L.te_b + k]));
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
            for (int r = 0; r < 4; r++) temb[(16 * m + 4 * (lane >> 4) + r) * LDT + 16 * j + (lane & 15)] = silu(acc[m][0][r]);
    }
    __syncthreads();

    // ---- input layer (Model.py:92-96): Linear(F,nunits) on the VALU, in the MFMA's C layout -> LayerNorm -> SiLU
    int col[NT];
#pragma unroll
    for (int n = 0; n < NT; n++) col[n] = 16 * (w * NT + n) + (lane & 15);
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
                    for (int r = 0; r < 4; r++) h[m][n][r] = fmaf(wv, xs[(16 * m + 4 * (lane >> 4) + r) * F + f], h[m][n][r]);
            }
        }
        if (a.ln) layer_norm_rows<MT, NT>(h, P + L.in_g, P + L.in_be, col, L.NU, part, W, w, lane);
#pragma unroll
        for (int m = 0; m < MT; m++)
#pragma unroll
            for (int n = 0; n < NT; n++)
#pragma unroll
                for (int r = 0; r < 4; r++) h[m][n][r] = silu(h[m][n][r]);
    }

    // ---- conditioned blocks (DiffusionBlocks.py:125-136)
    for (int bi = 0; bi < L.nblk; bi++) {
        const float *__restrict__ Q = P + L.blk0 + (int64_t)bi * L.blk_stride;
        store_tiles<MT, NT>(A, LD, h, col, lane);     // every wave is past its reads of A: a barrier closed the last layer
        __syncthreads();
        floatx4 y[MT][NT];
#pragma unroll
        for (int n = 0; n < NT; n++) {
            const float b = Q[L.b_b1 + col[n]];
#pragma unroll
            for (int m = 0; m < MT; m++) y[m][n] = floatx4{b, b, b, b};
        }
        gemm_tiles<MT, NT>(reinterpret_cast<const float4 *>(Q + L.b_w1) + (int64_t)w * NT * KG * 64, KG, A, LD, lane, y);
        if (a.ln) layer_norm_rows<MT, NT>(y, Q + L.b_g1, Q + L.b_be1, col, L.NU, part, W, w, lane);
        else __syncthreads();                         // A is read out: y may go there
        // y = SiLU(y) + SiLU(t_proj(temb)), one column tile of t_proj at a time
#pragma unroll
        for (int n = 0; n < NT; n++) {
            floatx4 tp[MT][1];
            const float b = Q[L.b_tb + col[n]];
#pragma unroll
            for (int m = 0; m < MT; m++) tp[m][0] = floatx4{b, b, b, b};
            gemm_tiles<MT, 1>(reinterpret_cast<const float4 *>(Q + L.b_tw) + (int64_t)(w * NT + n) * KGT * 64, KGT, temb, LDT, lane, tp);
#pragma unroll
            for (int m = 0; m < MT; m++)
#pragma unroll
                for (int r = 0; r < 4; r++) y[m][n][r] = silu(y[m][n][r]) + silu(tp[m][0][r]);
        }
        store_tiles<MT, NT>(A, LD, y, col, lane);
        __syncthreads();
#pragma unroll
        for (int n = 0; n < NT; n++) {
            const float b = Q[L.b_b2 + col[n]];
#pragma unroll
            for (int m = 0; m < MT; m++) y[m][n] = floatx4{b, b, b, b};
        }
        gemm_tiles<MT, NT>(reinterpret_cast<const float4 *>(Q + L.b_w2) + (int64_t)w * NT * KG * 64, KG, A, LD, lane, y);
        if (a.ln) layer_norm_rows<MT, NT>(y, Q + L.b_g2, Q + L.b_be2, col, L.NU, part, W, w, lane);
        else __syncthreads();
#pragma unroll
        for (int m = 0; m < MT; m++)
#pragma unroll
            for (int n = 0; n < NT; n++)
#pragma unroll
                for (int r = 0; r < 4; r++) h[m][n][r] = silu(a.skip ? y[m][n][r] + h[m][n][r] : y[m][n][r]);
    }

    // ---- output layer Linear(nunits,F) (Model.py:126) on the VALU: per wave a partial over its columns, then the waves in order
    // (the partials go to A: the barrier after the last block's second Linear closed its reads)
    for (int f = 0; f < F; f++) {
        float wv[NT];
#pragma unroll
        for (int n = 0; n < NT; n++) wv[n] = P[L.out_w + (int64_t)f * NP + col[n]];
#pragma unroll
        for (int m = 0; m < MT; m++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                float s = 0.f;
#pragma unroll
                for (int n = 0; n < NT; n++) s = fmaf(h[m][n][r], wv[n], s);
                s = row16_sum(s);
                if ((lane & 15) == 0) A[(w * M + 16 * m + 4 * (lane >> 4) + r) * F + f] = s;
            }
    }
    __syncthreads();
    for (int i = tid; i < M * F; i += nthr) {
        const int row = i / F, f = i - row * F;
        float s = 0.f;
        for (int ww = 0; ww < W; ww++) s += A[(ww * M + row) * F + f];
        if (r0 + row < a.B) a.out[(r0 + row) * F + f] = s + P[L.out_b + f];
    }
}

bool ends_with(const std::string &s, const char *suffix) {
    const size_t n = strlen(suffix);
    return s.size() >= n && s.compare(s.size() - n, n, suffix) == 0;
}

// the element count of the tensor a key names; 0 for an alias the reference's state_dict repeats (accepted, ignored); -1 for a
// key this architecture does not have
int64_t expected_numel(const dlpm_mlp *m, const std::string &key) {
    const int64_t F = m->F, NU = m->nunits, TE = m->TE;
    if (ends_with(key, "time_mlp.0.weight") || ends_with(key, "time_mlp.0.bias") || ends_with(key, "inblock.0.weight") ||
        ends_with(key, "inblock.0.bias"))
        return 0;
    if (m->ln && (ends_with(key, "inblock.1.weight") || ends_with(key, "inblock.1.bias") || ends_with(key, "mlp_1.2.weight") ||
                  ends_with(key, "mlp_1.2.bias") || ends_with(key, "mlp_2.2.weight") || ends_with(key, "mlp_2.2.bias")))
        return 0;
    if (key == "time_emb.weight" || key == "time_emb.bias" || key == "time_mlp.2.bias") return TE;
    if (key == "time_mlp.2.weight") return TE * TE;
    if (key == "linear_in.weight") return NU * F;
    if (key == "linear_in.bias") return NU;
    if (m->ln && (key == "group_norm_in.weight" || key == "group_norm_in.bias")) return NU;
    if (key == "outblocks_mean.1.weight") return F * NU;
    if (key == "outblocks_mean.1.bias") return F;
    std::string rest;
    if (key.rfind("midblocks.", 0) == 0) {
        const size_t dot = key.find('.', 10);
        if (dot == std::string::npos || dot == 10) return -1;
        for (size_t i = 10; i < dot; i++)
            if (key[i] < '0' || key[i] > '9') return -1;
        if (dot - 10 > 9 || std::stoll(key.substr(10, dot - 10)) >= m->nblocks) return -1;
        rest = key.substr(dot + 1);
    } else if (key.rfind("outblocks_mean.0.", 0) == 0) {
        rest = key.substr(17);
    } else {
        return -1;
    }
    if (rest == "mlp_1.1.weight" || rest == "mlp_2.1.weight") return NU * NU;
    if (rest == "t_proj.1.weight") return NU * TE;
    if (rest == "mlp_1.1.bias" || rest == "mlp_2.1.bias" || rest == "t_proj.1.bias") return NU;
    if (m->ln && (rest == "group_norm1.weight" || rest == "group_norm1.bias" || rest == "group_norm2.weight" || rest == "group_norm2.bias"))
        return NU;
    return -1;
}

template <int MT>
int launch_general(const dlpm_mlp *m, const GenArgs &a, unsigned grid, size_t lds, hipStream_t st) {
    void (*fn)(GenArgs) = nullptr;
    switch (m->gen.NT) {
        case 1: fn = k_mlp_general<MT, 1>; break;
        case 2: fn = k_mlp_general<MT, 2>; break;
        case 4: fn = k_mlp_general<MT, 4>; break;
        case 8: fn = k_mlp_general<MT, 8>; break;
    }
    if (!fn) {
        set_error("dlpm_mlp_forward: no general kernel for %d column tiles per wave", m->gen.NT);
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

int mlp_general_init(dlpm_mlp *m) {
    m->general = true;
    m->gen = mlp_gen_layout(m->F, m->nunits, m->TE, m->nblocks);
    m->gen_M = 0;
    for (int M : {32, 16}) {
        if (M == 32 && (m->flags & DLPM_MLP_TILE_16)) continue;
        if (mlp_gen_lds_bytes(m->gen, M) <= GEN_LDS_LIMIT) { m->gen_M = M; break; }
    }
    if ((m->flags & DLPM_MLP_TILE_32) && m->gen_M != 32) {
        set_error("dlpm_mlp_create: DLPM_MLP_TILE_32: a 32-row tile of this net (nfeatures %d, nunits %d, time_emb_size %d) takes %lld "
                  "bytes of LDS, a workgroup has %d", m->F, m->nunits, m->TE, (long long)mlp_gen_lds_bytes(m->gen, 32), GEN_LDS_LIMIT);
        return DLPM_ERR_UNSUPPORTED;
    }
    if (!m->gen_M) {
        set_error("dlpm_mlp_create: a 16-row tile of this net (nfeatures %d, nunits %d, time_emb_size %d) takes %lld bytes of LDS, "
                  "a workgroup has %d", m->F, m->nunits, m->TE, (long long)mlp_gen_lds_bytes(m->gen, 16), GEN_LDS_LIMIT);
        return DLPM_ERR_UNSUPPORTED;
    }
    return DLPM_OK;
}

int mlp_general_set_param(dlpm_mlp *m, const char *key_c, const float *w, int64_t numel) {
    const std::string key = key_c;
    const int64_t n = expected_numel(m, key);
    if (n < 0) {
        set_error("dlpm_mlp_set_param: unexpected key '%s' for this architecture (LayerNorm %s, %d blocks)", key_c, m->ln ? "on" : "off",
                  m->nblocks);
        return DLPM_ERR_ARG;
    }
    if (n == 0) return DLPM_OK;
    if (n != numel) {
        set_error("dlpm_mlp_set_param: '%s' has %lld elements, expected %lld", key_c, (long long)numel, (long long)n);
        return DLPM_ERR_ARG;
    }
    m->finalized = false;
    m->raw[key].assign(w, w + numel);
    return DLPM_OK;
}

int mlp_general_finalize(dlpm_mlp *m) {
    const MlpGenLayout &L = m->gen;
    const int F = m->F, NU = m->nunits, TE = m->TE;
    const MlpGenGradLayout G = mlp_gen_grad_layout(L);
    std::vector<float> blob((size_t)(L.total + G.total), 0.f);
    const std::string *missing = nullptr;
    std::string name;
    auto get = [&](const std::string &key) -> const float * {
        auto it = m->raw.find(key);
        if (it == m->raw.end()) {
            if (!missing) { name = key; missing = &name; }
            return nullptr;
        }
        return it->second.data();
    };
    auto vec = [&](int64_t off, const std::string &key, int n, int npad) { if (const float *v = get(key)) mlp_pack_vector(&blob[off], v, n, npad); };
    // a hidden Linear: the forward's operand and, in the second region, its transpose for the backward's dX = dY W
    auto op = [&](int64_t off, int64_t offT, const std::string &key, int N, int K, int NPad, int KPad) {
        if (const float *v = get(key)) {
            mlp_pack_operand(&blob[off], v, N, K, NPad, KPad);
            mlp_pack_operand_t(&blob[G.base + offT], v, N, K, NPad, KPad);
        }
    };
    vec(L.te_w, "time_emb.weight", TE, L.TEP); vec(L.te_b, "time_emb.bias", TE, L.TEP);
    op(L.tm_w, G.tm_wT, "time_mlp.2.weight", TE, TE, L.TEP, L.TEP); vec(L.tm_b, "time_mlp.2.bias", TE, L.TEP);
    if (const float *v = get("linear_in.weight")) mlp_pack_transposed(&blob[L.in_w], v, NU, F, L.NP);
    vec(L.in_b, "linear_in.bias", NU, L.NP);
    if (m->ln) { vec(L.in_g, "group_norm_in.weight", NU, L.NP); vec(L.in_be, "group_norm_in.bias", NU, L.NP); }
    for (int bi = 0; bi <= m->nblocks; bi++) {
        const std::string pre = bi < m->nblocks ? "midblocks." + std::to_string(bi) + "." : std::string("outblocks_mean.0.");
        const int64_t b = L.blk0 + (int64_t)bi * L.blk_stride, bT = G.blk0 + (int64_t)bi * G.blk_stride;
        op(b + L.b_w1, bT + G.b_w1T, pre + "mlp_1.1.weight", NU, NU, L.NP, L.NP); vec(b + L.b_b1, pre + "mlp_1.1.bias", NU, L.NP);
        op(b + L.b_tw, bT + G.b_twT, pre + "t_proj.1.weight", NU, TE, L.NP, L.TEP); vec(b + L.b_tb, pre + "t_proj.1.bias", NU, L.NP);
        op(b + L.b_w2, bT + G.b_w2T, pre + "mlp_2.1.weight", NU, NU, L.NP, L.NP); vec(b + L.b_b2, pre + "mlp_2.1.bias", NU, L.NP);
        if (m->ln) {
            vec(b + L.b_g1, pre + "group_norm1.weight", NU, L.NP); vec(b + L.b_be1, pre + "group_norm1.bias", NU, L.NP);
            vec(b + L.b_g2, pre + "group_norm2.weight", NU, L.NP); vec(b + L.b_be2, pre + "group_norm2.bias", NU, L.NP);
        }
    }
    if (const float *v = get("outblocks_mean.1.weight")) mlp_pack_rows(&blob[L.out_w], v, F, NU, L.NP);
    vec(L.out_b, "outblocks_mean.1.bias", F, F);
    if (missing) {
        set_error("dlpm_mlp_finalize: parameter tensor '%s' was not set (%zu tensors were)", missing->c_str(), m->raw.size());
        return DLPM_ERR_STATE;
    }
    if (!m->gen_dev) DLPM_HIP(hipMalloc(&m->gen_dev, blob.size() * sizeof(float)));
    DLPM_HIP(hipMemcpy(m->gen_dev, blob.data(), blob.size() * sizeof(float), hipMemcpyHostToDevice));
    m->finalized = true;
    return DLPM_OK;
}

int mlp_general_forward(dlpm_mlp *m, const float *x_dev, const float *t_dev, float *eps_dev, int64_t B, hipStream_t st) {
    // 32-row tiles read every weight once per 32 rows, but a grid of them that leaves compute units idle is slower than twice as
    // many 16-row tiles; the choice changes no bit of any row
    const int M = (m->gen_M == 32 && !(m->flags & DLPM_MLP_TILE_32) && ceil_div(B, 32) < GEN_FILL_TILES) ? 16 : m->gen_M;
    const int64_t lds = mlp_gen_lds_bytes(m->gen, M);
    if ((M != 16 && M != 32) || lds > GEN_LDS_LIMIT) {
        set_error("dlpm_mlp_forward: a %d-row tile of this net takes %lld bytes of LDS, a workgroup has %d", M, (long long)lds, GEN_LDS_LIMIT);
        return DLPM_ERR_UNSUPPORTED;
    }
    const int64_t grid = ceil_div(B, M);
    DLPM_CHECK_ARG(grid < (1ll << 31), "dlpm_mlp_forward: B = %lld is beyond the grid of one call", (long long)B);
    GenArgs a;
    a.P = m->gen_dev; a.L = m->gen; a.x = x_dev; a.t = t_dev; a.out = eps_dev; a.B = B; a.ln = m->ln; a.skip = m->skip;
    return M == 32 ? launch_general<2>(m, a, (unsigned)grid, (size_t)lds, st) : launch_general<1>(m, a, (unsigned)grid, (size_t)lds, st);
}

}  // namespace dlpm

extern "C" int32_t dlpm_mlp_tile_rows(const dlpm_mlp *m) {
    if (!m) return -1;
    return m->general ? m->gen_M : 0;
}

extern "C" int64_t dlpm_mlp_lds_bytes(const dlpm_mlp *m) {
    if (!m) return -1;
    return m->general ? mlp_gen_lds_bytes(m->gen, m->gen_M) : 0;
}
