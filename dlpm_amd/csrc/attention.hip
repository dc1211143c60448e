// attention.hip -- QKVAttention on the fp32 MFMA (v_mfma_f32_16x16x4_f32), softmax in fp32.
//
// Replaces QKVAttention.forward (dlpm/models/unet.py:236-250):
//   w = softmax((q * s)(k * s)^T), s = ch^(-1/4);  out = w v
// on qkv laid out NHWC [B, T, 3C] whose channel axis is head-major [head][q | k | v][ch] -- the
// layout the reference's reshape(b*heads, 3*ch, T) + split produces (unet.py:224,243-244).
//
// One workgroup per (sample, head): K (pre-scaled) and V of the head are staged ONCE in LDS and up to 8 waves walk the
// query tiles (16 queries each).  A wave computes S^T = K Q^T tile by tile, which leaves the query on the lane and the
// keys in registers: the row softmax is an in-register reduction plus two cross-lane steps, and -- because the MFMA's k
// index may be permuted freely as long as A and B agree -- the normalised probabilities are ALREADY in the A-operand
// layout of the P V product.  No score matrix is ever written to LDS or HBM.
// The same freedom picks the operand layouts for wide LDS reads: in Q K^T the contraction slot lk of MFMA kk is channel
// lk CH/4 + kk, so a lane reads CH/4 CONTIGUOUS floats of its K row (ds_read_b128s instead of one ds_read_b32 per MFMA);
// in P V output column li of tile ct is channel li CH/16 + ct, so one read of CH/16 contiguous floats of a V row feeds
// the CH/16 independent accumulators (which also removes the 40-cycle dependent-accumulator stall of a single chain),
// and the result leaves as whole float4s.
#include "conv.h"

namespace dlpm {
namespace {

typedef float floatx4 __attribute__((ext_vector_type(4)));

template <int CH, int NT>
__global__ void __launch_bounds__(512) k_attention(const float *__restrict__ qkv, float *__restrict__ out, int T, int C,
                                                   int heads, float scale) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int LD = CH + 4;
    constexpr int KQ = CH / 4;      // channels per contraction slot in Q K^T
    constexpr int NCT = CH / 16;    // output-channel tiles in P V
    float *Ks = lds, *Vs = lds + (size_t)T * LD;
    const int tid = threadIdx.x, nthreads = blockDim.x;
    const int b = blockIdx.x / heads, h = blockIdx.x % heads;
    const int64_t rs = 3 * (int64_t)C;  // row stride of qkv
    const float *base = qkv + (int64_t)b * T * rs + (int64_t)h * 3 * CH;

    for (int idx = tid; idx < T * (CH / 4); idx += nthreads) {
        const int s = idx / (CH / 4), c4 = (idx % (CH / 4)) * 4;
        float4 k = *reinterpret_cast<const float4 *>(base + s * rs + CH + c4);
        float4 v = *reinterpret_cast<const float4 *>(base + s * rs + 2 * CH + c4);
        k.x *= scale; k.y *= scale; k.z *= scale; k.w *= scale;
        *reinterpret_cast<float4 *>(Ks + s * LD + c4) = k;
        *reinterpret_cast<float4 *>(Vs + s * LD + c4) = v;
    }
    __syncthreads();

    const int wave = tid >> 6, nw = nthreads >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
    for (int t0 = wave * 16; t0 < T; t0 += nw * 16) {
        float qf[KQ];
        {
            const float *qrow = base + (int64_t)(t0 + li) * rs + lk * KQ;
#pragma unroll
            for (int q = 0; q < KQ / 4; q++) {
                const float4 v = *reinterpret_cast<const float4 *>(qrow + 4 * q);
                qf[4 * q] = v.x * scale; qf[4 * q + 1] = v.y * scale; qf[4 * q + 2] = v.z * scale; qf[4 * q + 3] = v.w * scale;
            }
        }
        // S^T tiles: acc[j][r] = S[t0 + li][16 j + 4 lk + r]
        floatx4 acc[NT];
        // (two key tiles at a time: their accumulator chains interleave, so no MFMA waits on the 40-cycle latency of its predecessor)
#pragma unroll
        for (int j = 0; j < NT; j += 2) {
            constexpr int J2 = NT > 1 ? 2 : 1;
            float kf[J2][KQ];
#pragma unroll
            for (int u = 0; u < J2; u++) {
                acc[j + u] = floatx4{0.f, 0.f, 0.f, 0.f};
                const float *krow = Ks + (16 * (j + u) + li) * LD + lk * KQ;
#pragma unroll
                for (int q = 0; q < KQ / 4; q++) *reinterpret_cast<float4 *>(kf[u] + 4 * q) = *reinterpret_cast<const float4 *>(krow + 4 * q);
            }
#pragma unroll
            for (int kk = 0; kk < KQ; kk++)
#pragma unroll
                for (int u = 0; u < J2; u++) acc[j + u] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[u][kk], qf[kk], acc[j + u], 0, 0, 0);
        }

        // softmax over the key axis (registers j, r and the 4 lane groups lk)
        float mx = -INFINITY;
#pragma unroll
        for (int j = 0; j < NT; j++)
#pragma unroll
            for (int r = 0; r < 4; r++) mx = fmaxf(mx, acc[j][r]);
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < NT; j++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                acc[j][r] = __expf(acc[j][r] - mx);      // v_exp_f32 on (x - max) log2 e: <= 0, relative error ~1e-7 (|x - max| < 90)
                sum += acc[j][r];
            }
        sum += __shfl_xor(sum, 16);
        sum += __shfl_xor(sum, 32);
        const float rsum = 1.0f / sum;                   // one IEEE division per row, 4 NT multiplies (<= 1 ulp from dividing each)
#pragma unroll
        for (int j = 0; j < NT; j++)
#pragma unroll
            for (int r = 0; r < 4; r++) acc[j][r] = acc[j][r] * rsum;

        // O = P V: MFMA step (j, r) contracts the keys s = 16 j + 4 lk + r over the 4 lane groups; tile ct, column li = channel li NCT + ct
        floatx4 o[NCT];
#pragma unroll
        for (int ct = 0; ct < NCT; ct++) o[ct] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < NT; j++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const float *vrow = Vs + (16 * j + 4 * lk + r) * LD + li * NCT;
                float vf[NCT];
                if (NCT == 1) vf[0] = vrow[0];
                else if (NCT == 2) *reinterpret_cast<float2 *>(vf) = *reinterpret_cast<const float2 *>(vrow);
                else {
#pragma unroll
                    for (int q = 0; q < NCT / 4; q++) *reinterpret_cast<float4 *>(vf + 4 * q) = *reinterpret_cast<const float4 *>(vrow + 4 * q);
                }
#pragma unroll
                for (int ct = 0; ct < NCT; ct++) o[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(acc[j][r], vf[ct], o[ct], 0, 0, 0);
            }
        // D layout: row = 4 lk + r (query), col = li -> channels li NCT .. li NCT + NCT - 1: contiguous per lane
        float *orow = out + ((int64_t)b * T + t0) * C + (int64_t)h * CH + li * NCT;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            float *dst = orow + (int64_t)(4 * lk + r) * C;
            if (NCT == 1) dst[0] = o[0][r];
            else if (NCT == 2) *reinterpret_cast<float2 *>(dst) = make_float2(o[0][r], o[1][r]);
            else {
#pragma unroll
                for (int q = 0; q < NCT / 4; q++)
                    *reinterpret_cast<float4 *>(dst + 4 * q) = make_float4(o[4 * q][r], o[4 * q + 1][r], o[4 * q + 2][r], o[4 * q + 3][r]);
            }
        }
    }
}

int launch_any(const float *qkv, float *out, int B, int T, int C, int heads, hipStream_t st);

template <int CH, int NT>
int launch_t(const float *qkv, float *out, int B, int T, int C, int heads, hipStream_t st) {
    const int nw = (T / 16) < 8 ? (T / 16) : 8;
    const size_t shmem = (size_t)2 * T * (CH + 4) * sizeof(float);
    if (shmem > 160 * 1024) return launch_any(qkv, out, B, T, C, heads, st);   // K / V of the head do not fit the LDS (T 256, ch 128)
    if (shmem > 64 * 1024) {
        int r = ensure_dynamic_lds(reinterpret_cast<const void *>(&k_attention<CH, NT>), (int)shmem);
        if (r != DLPM_OK) return r;
    }
    const float scale = (float)(1.0 / std::sqrt(std::sqrt((double)CH)));
    k_attention<CH, NT><<<(unsigned)(B * heads), 64 * nw, shmem, st>>>(qkv, out, T, C, heads, scale);
    DLPM_LAUNCH_CHECK();
    return DLPM_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// k_attention_any: the same arithmetic for ANY sequence length (1..4096) and head dim (1..256), flash-style.
//
// One workgroup per (sample, head; query block of up to 8 x 16 queries); its waves own one 16-query tile each.  K (pre-scaled)
// and V stream through LDS in blocks of KB keys, double-buffered (one barrier per block: block kb + 1 is written to the other
// buffer while block kb is read).  Per key block a wave computes S^T = K Q^T as above (query on the lane, P left in the A-operand
// layout of P V) and keeps the online-softmax state of its 16 rows: running max m and lane-partial sum l.  When a block raises
// the max, O (whose query index is 4 lk + r, not the lane) is rescaled by exp(m_old - m_new), fetched from the row's lane.
// Tails: keys >= T score -inf before the max (every block holds >= 1 real key, so m stays finite and exp(-inf - m) = 0), queries
// >= T read the clamped row T - 1 and are never stored.  The head dim is padded to CHP with zeros in LDS and registers; the
// scale is the real ch^(-1/4).  VEC (ch % 4 == 0, so every row offset is a multiple of 4 floats) picks float4 global accesses.
template <int CHP, int KB>
__global__ void __launch_bounds__(512) k_attention_any(const float *__restrict__ qkv, float *__restrict__ out, int T, int C,
                                                       int heads, int ch, float scale, int vec) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int LD = CHP + 4;
    constexpr int KQ = CHP / 4;
    constexpr int NCT = CHP / 16;
    constexpr int NT = KB / 16;
    constexpr int BUF = 2 * KB * LD;      // one buffer: K block then V block
    const int tid = threadIdx.x, nthreads = blockDim.x;
    const int nw = nthreads >> 6;
    const int bh = blockIdx.x, b = bh / heads, h = bh % heads;
    const int64_t rs = 3 * (int64_t)C;
    const float *base = qkv + (int64_t)b * T * rs + (int64_t)h * 3 * ch;
    const int nkb = (T + KB - 1) / KB;

    auto stage = [&](int kb, float *dst) {
        float *Ks = dst, *Vs = dst + KB * LD;
        const int k0 = kb * KB;
        if (vec) {
            for (int idx = tid; idx < KB * (CHP / 4); idx += nthreads) {
                const int s = idx / (CHP / 4), c4 = (idx % (CHP / 4)) * 4;
                float4 k = make_float4(0.f, 0.f, 0.f, 0.f), v = k;
                if (k0 + s < T && c4 < ch) {
                    const float *row = base + (int64_t)(k0 + s) * rs;
                    k = *reinterpret_cast<const float4 *>(row + ch + c4);
                    v = *reinterpret_cast<const float4 *>(row + 2 * ch + c4);
                    k.x *= scale; k.y *= scale; k.z *= scale; k.w *= scale;
                }
                *reinterpret_cast<float4 *>(Ks + s * LD + c4) = k;
                *reinterpret_cast<float4 *>(Vs + s * LD + c4) = v;
            }
        } else {
            for (int idx = tid; idx < KB * CHP; idx += nthreads) {
                const int s = idx / CHP, c = idx % CHP;
                float k = 0.f, v = 0.f;
                if (k0 + s < T && c < ch) {
                    const float *row = base + (int64_t)(k0 + s) * rs;
                    k = row[ch + c] * scale;
                    v = row[2 * ch + c];
                }
                Ks[s * LD + c] = k;
                Vs[s * LD + c] = v;
            }
        }
    };

    const int wave = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
    const int t0 = (blockIdx.y * nw + wave) * 16;
    float qf[KQ];
    {
        const int tq = min(t0 + li, T - 1);
        const float *qrow = base + (int64_t)tq * rs + lk * KQ;
#pragma unroll
        for (int q = 0; q < KQ / 4; q++) {
            const int c = lk * KQ + 4 * q;
            if (vec) {
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (c < ch) v = *reinterpret_cast<const float4 *>(qrow + 4 * q);
                qf[4 * q] = v.x * scale; qf[4 * q + 1] = v.y * scale; qf[4 * q + 2] = v.z * scale; qf[4 * q + 3] = v.w * scale;
            } else {
#pragma unroll
                for (int e = 0; e < 4; e++) qf[4 * q + e] = c + e < ch ? qrow[4 * q + e] * scale : 0.f;
            }
        }
    }
    floatx4 o[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ct++) o[ct] = floatx4{0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, l = 0.f;     // running max of row li (uniform over lk), lane-partial running sum

    stage(0, lds);
    __syncthreads();
    for (int kb = 0; kb < nkb; kb++) {
        if (kb + 1 < nkb) stage(kb + 1, lds + ((kb + 1) & 1) * BUF);
        const float *Ks = lds + (kb & 1) * BUF, *Vs = Ks + KB * LD;
        const int kvalid = T - kb * KB;    // keys of this block that exist (>= 1)
        floatx4 acc[NT];
        // acc[j][r] = S[t0 + li][kb KB + 16 j + 4 lk + r]
#pragma unroll
        for (int j = 0; j < NT; j += 2) {
            constexpr int J2 = (NT > 1 && CHP <= 128) ? 2 : 1;
#pragma unroll
            for (int jj = 0; jj < 2; jj += J2) {
                if (j + jj >= NT) break;
                float kf[J2][KQ];
#pragma unroll
                for (int u = 0; u < J2; u++) {
                    acc[j + jj + u] = floatx4{0.f, 0.f, 0.f, 0.f};
                    const float *krow = Ks + (16 * (j + jj + u) + li) * LD + lk * KQ;
#pragma unroll
                    for (int q = 0; q < KQ / 4; q++) *reinterpret_cast<float4 *>(kf[u] + 4 * q) = *reinterpret_cast<const float4 *>(krow + 4 * q);
                }
#pragma unroll
                for (int kk = 0; kk < KQ; kk++)
#pragma unroll
                    for (int u = 0; u < J2; u++) acc[j + jj + u] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[u][kk], qf[kk], acc[j + jj + u], 0, 0, 0);
            }
        }
        if (kvalid < KB) {
#pragma unroll
            for (int j = 0; j < NT; j++)
#pragma unroll
                for (int r = 0; r < 4; r++)
                    if (16 * j + 4 * lk + r >= kvalid) acc[j][r] = -INFINITY;
        }
        float mb = -INFINITY;
#pragma unroll
        for (int j = 0; j < NT; j++)
#pragma unroll
            for (int r = 0; r < 4; r++) mb = fmaxf(mb, acc[j][r]);
        mb = fmaxf(mb, __shfl_xor(mb, 16));
        mb = fmaxf(mb, __shfl_xor(mb, 32));
        const float mn = fmaxf(m, mb);           // finite: the block holds a real key
        if (__any(mn > m)) {
            // rescale row li by exp(m - mn) (0 on the first block); O's row 4 lk + r lives on lane 4 lk + r
            const float alpha = __expf(m - mn);
            l *= alpha;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const float ar = __shfl(alpha, 4 * lk + r);
#pragma unroll
                for (int ct = 0; ct < NCT; ct++) o[ct][r] *= ar;
            }
            m = mn;
        }
#pragma unroll
        for (int j = 0; j < NT; j++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                acc[j][r] = __expf(acc[j][r] - m);
                l += acc[j][r];
            }
#pragma unroll
        for (int j = 0; j < NT; j++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const float *vrow = Vs + (16 * j + 4 * lk + r) * LD + li * NCT;
                float vf[NCT];
                if (NCT == 1) vf[0] = vrow[0];
                else if (NCT == 2) *reinterpret_cast<float2 *>(vf) = *reinterpret_cast<const float2 *>(vrow);
                else {
#pragma unroll
                    for (int q = 0; q < NCT / 4; q++) *reinterpret_cast<float4 *>(vf + 4 * q) = *reinterpret_cast<const float4 *>(vrow + 4 * q);
                }
#pragma unroll
                for (int ct = 0; ct < NCT; ct++) o[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(acc[j][r], vf[ct], o[ct], 0, 0, 0);
            }
        __syncthreads();
    }

    l += __shfl_xor(l, 16);
    l += __shfl_xor(l, 32);
    const float rl = 1.0f / l;
    if (t0 >= T) return;
    const int c0 = li * NCT;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const float rr = __shfl(rl, 4 * lk + r);
        const int tq = t0 + 4 * lk + r;
        if (tq >= T) continue;
        float *dst = out + ((int64_t)b * T + tq) * C + (int64_t)h * ch + c0;
        if (NCT >= 4 && vec) {
#pragma unroll
            for (int q = 0; q < NCT / 4; q++)
                if (c0 + 4 * q < ch)
                    *reinterpret_cast<float4 *>(dst + 4 * q) = make_float4(o[4 * q][r] * rr, o[4 * q + 1][r] * rr, o[4 * q + 2][r] * rr, o[4 * q + 3][r] * rr);
        } else {
#pragma unroll
            for (int ct = 0; ct < NCT; ct++)
                if (c0 + ct < ch) dst[ct] = o[ct][r] * rr;
        }
    }
}

template <int CHP>
int launch_any_t(const float *qkv, float *out, int B, int T, int C, int heads, hipStream_t st) {
    constexpr int KB = CHP <= 128 ? 64 : 32;
    const int ch = C / heads;
    const int tiles = (T + 15) / 16;
    const int nw = tiles < 8 ? tiles : 8;
    const int nqb = (tiles + nw - 1) / nw;
    const size_t shmem = (size_t)2 * 2 * KB * (CHP + 4) * sizeof(float);
    if (shmem > 64 * 1024) {
        int r = ensure_dynamic_lds(reinterpret_cast<const void *>(&k_attention_any<CHP, KB>), (int)shmem);
        if (r != DLPM_OK) return r;
    }
    const float scale = (float)(1.0 / std::sqrt(std::sqrt((double)ch)));
    const int vec = (ch % 4 == 0 && (reinterpret_cast<uintptr_t>(qkv) & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0) ? 1 : 0;
    k_attention_any<CHP, KB><<<dim3((unsigned)(B * heads), (unsigned)nqb), 64 * nw, shmem, st>>>(qkv, out, T, C, heads, ch, scale, vec);
    DLPM_LAUNCH_CHECK();
    return DLPM_OK;
}

int launch_any(const float *qkv, float *out, int B, int T, int C, int heads, hipStream_t st) {
    const int ch = C / heads;
    if (T < 1 || T > 4096) {
        set_error("attention: unsupported sequence length T=%d (supported: 1 .. 4096)", T);
        return DLPM_ERR_UNSUPPORTED;
    }
    if (ch <= 16) return launch_any_t<16>(qkv, out, B, T, C, heads, st);
    if (ch <= 32) return launch_any_t<32>(qkv, out, B, T, C, heads, st);
    if (ch <= 64) return launch_any_t<64>(qkv, out, B, T, C, heads, st);
    if (ch <= 128) return launch_any_t<128>(qkv, out, B, T, C, heads, st);
    if (ch <= 256) return launch_any_t<256>(qkv, out, B, T, C, heads, st);
    set_error("attention: unsupported head dim %d (supported: 1 .. 256)", ch);
    return DLPM_ERR_UNSUPPORTED;
}

template <int CH>
int launch_ch(const float *qkv, float *out, int B, int T, int C, int heads, hipStream_t st) {
    switch (T) {
        case 16: return launch_t<CH, 1>(qkv, out, B, T, C, heads, st);
        case 64: return launch_t<CH, 4>(qkv, out, B, T, C, heads, st);
        case 256: return launch_t<CH, 16>(qkv, out, B, T, C, heads, st);
        default: return launch_any(qkv, out, B, T, C, heads, st);
    }
}

}  // namespace

int launch_attention(const float *qkv, float *out, int B, int T, int C, int heads, hipStream_t st) {
    if (heads <= 0 || C % heads != 0) {
        set_error("attention: channels %d not divisible by heads %d", C, heads);
        return DLPM_ERR_ARG;
    }
    const int ch = C / heads;
    ProfScope ps("attention", 4.0 * B * (double)T * T * C, 4.0 * 4.0 * B * (double)T * C, st);
    switch (ch) {
        case 16: return launch_ch<16>(qkv, out, B, T, C, heads, st);
        case 32: return launch_ch<32>(qkv, out, B, T, C, heads, st);
        case 64: return launch_ch<64>(qkv, out, B, T, C, heads, st);
        case 128: return launch_ch<128>(qkv, out, B, T, C, heads, st);
        default: return launch_any(qkv, out, B, T, C, heads, st);
    }
}

int launch_attention_general(const float *qkv, float *out, int B, int T, int C, int heads, hipStream_t st) {
    if (heads <= 0 || C % heads != 0) {
        set_error("attention: channels %d not divisible by heads %d", C, heads);
        return DLPM_ERR_ARG;
    }
    ProfScope ps("attention_any", 4.0 * B * (double)T * T * C, 4.0 * 4.0 * B * (double)T * C, st);
    return launch_any(qkv, out, B, T, C, heads, st);
}

}  // namespace dlpm
