// mlp_pack.h -- the host side of the general toy-net forward (mlp_general.hip): how a net of any width is cut into MFMA tiles, where
// every tensor lies in the packed blob, and the routine that lays a Linear weight out as the B operand of v_mfma_f32_16x16x4_f32.
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

}  // namespace dlpm
