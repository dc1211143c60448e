// mlp_pack.h -- the host side of the general toy-net forward (mlp_general.hip) and of its backward (mlp_general_grad.hip): how a net
// of any width is cut into MFMA tiles, where every tensor lies in the packed blob, the routine that lays a Linear weight out as the
// B operand of v_mfma_f32_16x16x4_f32, and for the backward the transposed operands, the per-row records and the slots of the weight
// pass.  Also the ONE definition of torch's flat parameter vector (MlpFlat) with its map into the general blob and into the lane
// kernels' blob (MlpOffsets, mlp.hip).
// Plain C++ with no HIP in it, so that the packing can be compiled into a stand-alone program and run under a host sanitizer.
#pragma once
#include <cstdint>

namespace dlpm {

constexpr int GEN_TILE = 16;              // the MFMA tile: every N and K of the blob is zero-padded to a multiple of it
constexpr int GEN_MAX_WAVES = 8;          // waves of a workgroup; they split the output columns
constexpr int GEN_LDS_LIMIT = 160 * 1024; // bytes of LDS a workgroup may take on gfx950
constexpr int GEN_FILL_TILES = 256;       // 32-row tiles are taken from this many on (one per compute unit), 16-row tiles below
constexpr int GEN_MAX_UNITS = 1024, GEN_MAX_TE = 1024, GEN_MAX_FEATURES = 64;

struct MlpGenLayout {
    int F, NU, TE, nblk;      // the net; nblk = nblocks + 1 conditioned blocks
    int NP, TEP;              // nunits and time_emb_size padded: NP = 16 W NT, TEP = 16 ceil(TE / 16)
    int W, NT;                // waves per workgroup and 16-column tiles per wave
    int LD, LDT;              // row strides (floats) of the activation and the time-embedding image in LDS
    // offsets (floats) into the blob.  Vectors are zero-padded to NP (TEP for the time path); in_w and out_w are [F][NP];
    // tm_w, b_w1, b_tw, b_w2 are MFMA operands (mlp_pack_operand)
    int64_t te_w, te_b, tm_w, tm_b, in_w, in_b, in_g, in_be, blk0, blk_stride, out_w, out_b, total;
    int64_t b_w1, b_b1, b_g1, b_be1, b_tw, b_tb, b_w2, b_b2, b_g2, b_be2;
};

inline int gen_pad(int n) { return (n + GEN_TILE - 1) / GEN_TILE * GEN_TILE; }

inline MlpGenLayout mlp_gen_layout(int F, int NU, int TE, int nblocks) {
    MlpGenLayout L{};
    L.F = F; L.NU = NU; L.TE = TE; L.nblk = nblocks + 1;
    const int tiles = gen_pad(NU) / GEN_TILE;
    L.NT = 1;
    while ((tiles + L.NT - 1) / L.NT > GEN_MAX_WAVES) L.NT *= 2;
    L.W = (tiles + L.NT - 1) / L.NT;
    L.NP = GEN_TILE * L.W * L.NT;
    L.TEP = gen_pad(TE);
    // + 4: a row stride of an odd number of 16-byte units, so the 16 rows of an A fragment start in 16 different bank quads.
    // The activation image also holds the first time-embedding layer and, at the end, the waves' partial outputs [W][M][F].
    int widest = L.NP > L.TEP ? L.NP : L.TEP;
    if (L.W * F > widest) widest = gen_pad(L.W * F);
    L.LD = widest + 4;
    L.LDT = L.TEP + 4;
    int64_t p = 0;
    auto take = [&](int64_t n) { int64_t r = p; p += (n + 3) / 4 * 4; return r; };
    L.te_w = take(L.TEP); L.te_b = take(L.TEP); L.tm_w = take((int64_t)L.TEP * L.TEP); L.tm_b = take(L.TEP);
    L.in_w = take((int64_t)F * L.NP); L.in_b = take(L.NP); L.in_g = take(L.NP); L.in_be = take(L.NP);
    int64_t q = 0;
    auto takeb = [&](int64_t n) { int64_t r = q; q += (n + 3) / 4 * 4; return r; };
    L.b_w1 = takeb((int64_t)L.NP * L.NP); L.b_b1 = takeb(L.NP); L.b_g1 = takeb(L.NP); L.b_be1 = takeb(L.NP);
    L.b_tw = takeb((int64_t)L.NP * L.TEP); L.b_tb = takeb(L.NP);
    L.b_w2 = takeb((int64_t)L.NP * L.NP); L.b_b2 = takeb(L.NP); L.b_g2 = takeb(L.NP); L.b_be2 = takeb(L.NP);
    L.blk_stride = q;
    L.blk0 = take(q * L.nblk);
    L.out_w = take((int64_t)F * L.NP); L.out_b = take(F);
    L.total = p;
    return L;
}

// bytes of LDS of a workgroup that owns M rows: activations [M][LD], time embedding [M][LDT], x [M][F], t [M] and the LayerNorm
// partial sums [2][W][M]
inline int64_t mlp_gen_lds_bytes(const MlpGenLayout &L, int M) {
    return 4 * ((int64_t)M * L.LD + (int64_t)M * L.LDT + (int64_t)M * L.F + M + 2 * (int64_t)L.W * M);
}

// A Linear weight w[N][K] (row-major, as the state_dict has it) as the B operand of the 16x16x4 fp32 MFMA, zero-padded to
// [NPad][KPad]: dst[column tile j][k group g][lane l][s] = w[16 j + (l & 15)][16 g + 4 (l >> 4) + s].  One 16-byte load per lane
// then feeds four MFMAs: step s of group g multiplies k = 16 g + 4 (l >> 4) + s, the k the A fragment's float4 holds in element s.
inline void mlp_pack_operand(float *dst, const float *w, int N, int K, int NPad, int KPad) {
    const int KG = KPad / GEN_TILE;
    for (int j = 0; j < NPad / GEN_TILE; j++)
        for (int g = 0; g < KG; g++)
            for (int l = 0; l < 64; l++)
                for (int s = 0; s < 4; s++) {
                    const int n = GEN_TILE * j + (l & 15), k = GEN_TILE * g + 4 * (l >> 4) + s;
                    dst[(((int64_t)j * KG + g) * 64 + l) * 4 + s] = (n < N && k < K) ? w[(int64_t)n * K + k] : 0.0f;
                }
}

// a vector of n values zero-padded to npad
inline void mlp_pack_vector(float *dst, const float *v, int n, int npad) {
    for (int i = 0; i < npad; i++) dst[i] = i < n ? v[i] : 0.0f;
}

// a Linear weight w[N][K] transposed to [K][NPad] (the input layer's), zero-padded
inline void mlp_pack_transposed(float *dst, const float *w, int N, int K, int NPad) {
    for (int k = 0; k < K; k++)
        for (int n = 0; n < NPad; n++) dst[(int64_t)k * NPad + n] = n < N ? w[(int64_t)n * K + k] : 0.0f;
}

// rows w[R][K] each zero-padded to KPad (the output layer's [F][NP])
inline void mlp_pack_rows(float *dst, const float *w, int R, int K, int KPad) {
    for (int r = 0; r < R; r++) mlp_pack_vector(dst + (int64_t)r * KPad, w + (int64_t)r * K, K, KPad);
}

// ------------------------------------------------------------------------------------------------ the backward (mlp_general_grad.hip)
// Weight pass: the rows are cut into chunks of GEN_GRAD_RC; a chunk's dW = dY^T A is one fp32 MFMA accumulation, rows in order.
// The chunks are dealt to at most GEN_GRAD_SLOTS slots, each a contiguous run of chunks whose partials are added in chunk order in
// fp64; the slots' fp64 sums are then added in slot order and rounded once.  So the workspace holds at most GEN_GRAD_SLOTS copies
// of the gradient (fp64) whatever the row count, and the result does not depend on the grid.
constexpr int GEN_GRAD_RC = 64;
constexpr int GEN_GRAD_SLOTS = 16;

// where mlp_pack_operand puts w[n][k] of an operand padded to KPad columns
inline int64_t mlp_operand_index(int n, int k, int KPad) {
    const int KG = KPad / GEN_TILE, j = n / GEN_TILE, g = k / GEN_TILE, l = (n & 15) + 16 * ((k & 15) >> 2), s = k & 3;
    return (((int64_t)j * KG + g) * 64 + l) * 4 + s;
}

// the transpose of w[N][K] as an operand: mlp_pack_operand with N and K exchanged, the B operand of dX = dY W (its output columns
// run over k, its reduction over n); dst holds [KPad / 16 column tiles][NPad / 16 groups][64][4]
inline void mlp_pack_operand_t(float *dst, const float *w, int N, int K, int NPad, int KPad) {
    for (int64_t i = 0; i < (int64_t)NPad * KPad; i++) dst[i] = 0.0f;
    for (int n = 0; n < N; n++)
        for (int k = 0; k < K; k++) dst[mlp_operand_index(k, n, NPad)] = w[(int64_t)n * K + k];
}

// the second blob region, behind the forward's MlpGenLayout::total floats: the transposed operands of the four hidden Linears
struct MlpGenGradLayout {
    int64_t base;                        // = MlpGenLayout::total
    int64_t tm_wT, blk0, blk_stride;     // relative to base
    int64_t b_w1T, b_twT, b_w2T;         // relative to a block
    int64_t total;                       // floats of this region
};

inline MlpGenGradLayout mlp_gen_grad_layout(const MlpGenLayout &L) {
    MlpGenGradLayout G{};
    G.base = L.total;
    G.tm_wT = 0;
    G.b_w1T = 0;
    G.b_twT = (int64_t)L.NP * L.NP;
    G.b_w2T = G.b_twT + (int64_t)L.NP * L.TEP;
    G.blk_stride = G.b_w2T + (int64_t)L.NP * L.NP;
    G.blk0 = (int64_t)L.TEP * L.TEP;
    G.total = G.blk0 + G.blk_stride * L.nblk;
    return G;
}

// LDS of a workgroup of the backward that owns M rows.  The backward's dY image is the forward's activation image and its dtemb
// accumulator the time-embedding image: everything the walk back needs of the forward lies per row in the workspace, so once the
// recomputed forward is through both images are free, and the budget is the forward's.
inline int64_t mlp_gen_grad_lds_bytes(const MlpGenLayout &L, int M) { return mlp_gen_lds_bytes(L, M); }

// the flat parameter vector, parameters_to_vector(model.parameters()): named_parameters() order, torch's [out][in] layout, every
// alias once; a net without LayerNorm has no group_norm tensors (their offsets are -1)
struct MlpFlat {
    int64_t in_g, in_be, te_w, te_b, tm_w, tm_b, in_w, in_b, blk0, blk_stride, out_w, out_b, P;
    int64_t b_g1, b_be1, b_g2, b_be2, b_w1, b_b1, b_tw, b_tb, b_w2, b_b2;
};

inline MlpFlat mlp_flat(int F, int NU, int TE, int nblocks, bool ln) {
    MlpFlat f{};
    int64_t p = 0;
    auto take = [&](int64_t n) { int64_t r = p; p += n; return r; };
    f.in_g = ln ? take(NU) : -1; f.in_be = ln ? take(NU) : -1;
    f.te_w = take(TE); f.te_b = take(TE);
    f.tm_w = take((int64_t)TE * TE); f.tm_b = take(TE);
    f.in_w = take((int64_t)NU * F); f.in_b = take(NU);
    int64_t q = 0;
    auto takeb = [&](int64_t n) { int64_t r = q; q += n; return r; };
    f.b_g1 = ln ? takeb(NU) : -1; f.b_be1 = ln ? takeb(NU) : -1; f.b_g2 = ln ? takeb(NU) : -1; f.b_be2 = ln ? takeb(NU) : -1;
    f.b_w1 = takeb((int64_t)NU * NU); f.b_b1 = takeb(NU);
    f.b_tw = takeb((int64_t)NU * TE); f.b_tb = takeb(NU);
    f.b_w2 = takeb((int64_t)NU * NU); f.b_b2 = takeb(NU);
    f.blk_stride = q;
    f.blk0 = take(q * (nblocks + 1));
    f.out_w = take((int64_t)F * NU); f.out_b = take(F);
    f.P = p;
    return f;
}

// fwd[i] = index in the blob of element i of the flat vector; tr[i] = index of its copy in the transposed region (from the start
// of the blob), -1 for a tensor that has none.  Both arrays hold MlpFlat::P entries.
inline void mlp_general_flat_map(const MlpGenLayout &L, const MlpGenGradLayout &G, const MlpFlat &f, int64_t *fwd, int64_t *tr) {
    const int F = L.F, NU = L.NU, TE = L.TE;
    for (int64_t i = 0; i < f.P; i++) { fwd[i] = -1; tr[i] = -1; }
    auto vec = [&](int64_t fo, int64_t bo, int n) { if (fo >= 0) for (int i = 0; i < n; i++) fwd[fo + i] = bo + i; };
    auto op = [&](int64_t fo, int64_t bo, int64_t to, int N, int K, int NPad, int KPad) {
        for (int n = 0; n < N; n++)
            for (int k = 0; k < K; k++) {
                fwd[fo + (int64_t)n * K + k] = bo + mlp_operand_index(n, k, KPad);
                tr[fo + (int64_t)n * K + k] = G.base + to + mlp_operand_index(k, n, NPad);
            }
    };
    vec(f.in_g, L.in_g, NU); vec(f.in_be, L.in_be, NU);
    vec(f.te_w, L.te_w, TE); vec(f.te_b, L.te_b, TE);
    op(f.tm_w, L.tm_w, G.tm_wT, TE, TE, L.TEP, L.TEP); vec(f.tm_b, L.tm_b, TE);
    for (int n = 0; n < NU; n++)
        for (int k = 0; k < F; k++) fwd[f.in_w + (int64_t)n * F + k] = L.in_w + (int64_t)k * L.NP + n;
    vec(f.in_b, L.in_b, NU);
    for (int bi = 0; bi < L.nblk; bi++) {
        const int64_t fb = f.blk0 + bi * f.blk_stride, b = L.blk0 + bi * L.blk_stride, t = G.blk0 + bi * G.blk_stride;
        if (f.b_g1 >= 0) {
            vec(fb + f.b_g1, b + L.b_g1, NU); vec(fb + f.b_be1, b + L.b_be1, NU);
            vec(fb + f.b_g2, b + L.b_g2, NU); vec(fb + f.b_be2, b + L.b_be2, NU);
        }
        op(fb + f.b_w1, b + L.b_w1, t + G.b_w1T, NU, NU, L.NP, L.NP); vec(fb + f.b_b1, b + L.b_b1, NU);
        op(fb + f.b_tw, b + L.b_tw, t + G.b_twT, NU, TE, L.NP, L.TEP); vec(fb + f.b_tb, b + L.b_tb, NU);
        op(fb + f.b_w2, b + L.b_w2, t + G.b_w2T, NU, NU, L.NP, L.NP); vec(fb + f.b_b2, b + L.b_b2, NU);
    }
    for (int k = 0; k < F; k++)
        for (int n = 0; n < NU; n++) fwd[f.out_w + (int64_t)k * NU + n] = L.out_w + (int64_t)k * L.NP + n;
    vec(f.out_b, L.out_b, F);
}

// ------------------------------------------------------------------------------------------------ the lane kernels' blob (mlp.hip)
constexpr int LANE_NU = 64;   // hidden units of the lane kernels' net == wavefront width (mlp.h: NU)

struct MlpOffsets {      // offsets (floats) into the lane kernels' packed parameter blob; every tensor starts on a 16-byte boundary
    int te_w, te_b, tm_w, tm_b, in_w, in_b, in_g, in_be, blk0, blk_stride, out_w, out_b;
    // per block: w1T[64*64] b1 g1 be1 twT[TE*64] tb w2T[64*64] b2 g2 be2; a Linear weight [N][K] lies transposed, [K][64]
    int b_w1, b_b1, b_g1, b_be1, b_tw, b_tb, b_w2, b_b2, b_g2, b_be2;
};

// the layout of a net's blob and, through `total`, its size in floats
inline MlpOffsets mlp_lane_offsets(int F, int TE, int nblocks, int *total) {
    MlpOffsets o{};
    int p = 0;
    auto take = [&](int n) { int r = p; p += (n + 3) / 4 * 4; return r; };
    o.te_w = take(TE); o.te_b = take(TE); o.tm_w = take(TE * TE); o.tm_b = take(TE);
    o.in_w = take(F * LANE_NU); o.in_b = take(LANE_NU); o.in_g = take(LANE_NU); o.in_be = take(LANE_NU);
    int q = 0;
    auto takeb = [&](int n) { int r = q; q += (n + 3) / 4 * 4; return r; };
    o.b_w1 = takeb(LANE_NU * LANE_NU); o.b_b1 = takeb(LANE_NU); o.b_g1 = takeb(LANE_NU); o.b_be1 = takeb(LANE_NU);
    o.b_tw = takeb(TE * LANE_NU); o.b_tb = takeb(LANE_NU);
    o.b_w2 = takeb(LANE_NU * LANE_NU); o.b_b2 = takeb(LANE_NU); o.b_g2 = takeb(LANE_NU); o.b_be2 = takeb(LANE_NU);
    o.blk_stride = q;
    o.blk0 = take(q * (nblocks + 1));
    o.out_w = take(F * LANE_NU); o.out_b = take(F);
    *total = p;
    return o;
}

// map[i] = index in the lane blob of element i of the flat vector f = mlp_flat(F, 64, TE, nblocks, true); MlpFlat::P entries
inline void mlp_lane_flat_map(const MlpOffsets &o, const MlpFlat &f, int F, int TE, int nblocks, int64_t *map) {
    for (int64_t i = 0; i < f.P; i++) map[i] = -1;
    auto vec = [&](int64_t fo, int bo, int n) { for (int i = 0; i < n; i++) map[fo + i] = bo + i; };
    // a Linear weight [N][K] in the flat vector, transposed to [K][ld] in the blob
    auto mat = [&](int64_t fo, int bo, int N, int K, int ld) {
        for (int n = 0; n < N; n++)
            for (int k = 0; k < K; k++) map[fo + n * K + k] = bo + k * ld + n;
    };
    vec(f.in_g, o.in_g, LANE_NU); vec(f.in_be, o.in_be, LANE_NU);
    vec(f.te_w, o.te_w, TE); vec(f.te_b, o.te_b, TE);
    mat(f.tm_w, o.tm_w, TE, TE, TE); vec(f.tm_b, o.tm_b, TE);
    mat(f.in_w, o.in_w, LANE_NU, F, LANE_NU); vec(f.in_b, o.in_b, LANE_NU);
    for (int bi = 0; bi <= nblocks; bi++) {
        const int64_t fb = f.blk0 + bi * f.blk_stride;
        const int ob = o.blk0 + bi * o.blk_stride;
        vec(fb + f.b_g1, ob + o.b_g1, LANE_NU); vec(fb + f.b_be1, ob + o.b_be1, LANE_NU);
        vec(fb + f.b_g2, ob + o.b_g2, LANE_NU); vec(fb + f.b_be2, ob + o.b_be2, LANE_NU);
        mat(fb + f.b_w1, ob + o.b_w1, LANE_NU, LANE_NU, LANE_NU); vec(fb + f.b_b1, ob + o.b_b1, LANE_NU);
        mat(fb + f.b_tw, ob + o.b_tw, LANE_NU, TE, LANE_NU); vec(fb + f.b_tb, ob + o.b_tb, LANE_NU);
        mat(fb + f.b_w2, ob + o.b_w2, LANE_NU, LANE_NU, LANE_NU); vec(fb + f.b_b2, ob + o.b_b2, LANE_NU);
    }
    vec(f.out_w, o.out_w, F * LANE_NU); vec(f.out_b, o.out_b, F);      // the blob keeps outblocks_mean.1.weight as [F][64]
}

// the backward's per-row records in the workspace, in floats per row: record q of width wq lies at ws[off_q rows + row wq + column]
struct MlpGenRecords {
    int64_t e0, a1, temb, da1, da0;                           // width TEP
    int64_t nin, dlnin, dzin, hfin;                           // width NP
    int64_t rsin;                                             // width 4 (element 0)
    int64_t blk0, blk_stride;                                 // per block, width NP:
    int64_t b_h, b_n1, b_tp, b_y, b_n2, b_dln1, b_dln2, b_dz1, b_dz2, b_dtp;
    int64_t b_rs;                                             // width 4: 1 / sigma of LayerNorm 1 and 2
    int64_t per_row;
};

inline MlpGenRecords mlp_gen_records(const MlpGenLayout &L) {
    MlpGenRecords r{};
    int64_t p = 0;
    auto take = [&](int64_t n) { int64_t v = p; p += n; return v; };
    r.e0 = take(L.TEP); r.a1 = take(L.TEP); r.temb = take(L.TEP); r.da1 = take(L.TEP); r.da0 = take(L.TEP);
    r.nin = take(L.NP); r.dlnin = take(L.NP); r.dzin = take(L.NP); r.hfin = take(L.NP); r.rsin = take(4);
    int64_t q = 0;
    auto takeb = [&](int64_t n) { int64_t v = q; q += n; return v; };
    r.b_h = takeb(L.NP); r.b_n1 = takeb(L.NP); r.b_tp = takeb(L.NP); r.b_y = takeb(L.NP); r.b_n2 = takeb(L.NP);
    r.b_dln1 = takeb(L.NP); r.b_dln2 = takeb(L.NP); r.b_dz1 = takeb(L.NP); r.b_dz2 = takeb(L.NP); r.b_dtp = takeb(L.NP);
    r.b_rs = takeb(4);
    r.blk_stride = q;
    r.blk0 = take(q * L.nblk);
    r.per_row = p;
    return r;
}

// the slots of the weight pass for `rows` rows: how many, and the rows of each (a multiple of GEN_GRAD_RC)
inline void mlp_gen_grad_slots(int64_t rows, int *slots, int64_t *rows_per_slot) {
    const int64_t chunks = (rows + GEN_GRAD_RC - 1) / GEN_GRAD_RC;
    const int64_t per = (chunks + GEN_GRAD_SLOTS - 1) / GEN_GRAD_SLOTS;
    *rows_per_slot = per * GEN_GRAD_RC;
    *slots = (int)((chunks + per - 1) / per);
}

// bytes of workspace of the backward: the records, then slots x P fp64 partial sums
inline int64_t mlp_gen_grad_workspace_bytes(const MlpGenLayout &L, const MlpFlat &f, int64_t rows) {
    int slots;
    int64_t rps;
    mlp_gen_grad_slots(rows, &slots, &rps);
    const int64_t rec = (mlp_gen_records(L).per_row * rows + 1) / 2 * 2;
    return rec * 4 + (int64_t)slots * f.P * 8;
}

}  // namespace dlpm
