// mfma64_tile.h -- the 128 x 128 tile loop on v_mfma_f64_16x16x4_f64 that k_prdc_gram (prdc.hip) and k_fd_tile (fd.hip) share: its
// geometry, the lane decomposition with the operand and C/D maps, the 4 x 4 accumulator block of a wave, the pipelined K loop and the
// row-major staging store.  What is loaded, and every epilogue, stays with the kernels.  Everything here has internal linkage; the LDS
// image belongs to the caller, which passes a pointer to it.
#pragma once
#include "common.h"

namespace dlpm {
namespace {

constexpr int kTile = 128;                  // rows and columns of a tile
constexpr int kThreads = 256;               // 4 waves as 2 x 2, each 64 x 64 = 4 x 4 accumulators
constexpr int kKC = 16, kLD = kKC + 1;      // K step of the tile loop, LDS row pitch in doubles
constexpr int kImage = 2 * kTile * kLD;     // doubles of the LDS image: the A rows [128][17], then the B rows

typedef double doublex4 __attribute__((ext_vector_type(4)));
typedef doublex4 Acc[4][4];

// A/B operand of the fp64 MFMA: lane l holds [row l & 15][k = l >> 4]; C/D: col = lane & 15, row = (lane >> 4) + 4 reg -- NOT the map
// of the other MFMAs.  Element (bi, bj, reg) of a lane is tile row wm 64 + bi 16 + lk + 4 reg, tile column wn 64 + bj 16 + l15.
struct Lanes {
    int wm, wn, l15, lk;
};

__device__ inline Lanes lanes_of(int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    return Lanes{wave >> 1, wave & 1, lane & 15, lane >> 4};
}

__device__ inline int tile_row(const Lanes &l, int bi, int reg) { return l.wm * 64 + bi * 16 + l.lk + 4 * reg; }
__device__ inline int tile_col(const Lanes &l, int bj) { return l.wn * 64 + bj * 16 + l.l15; }

__device__ __forceinline__ void acc_zero(Acc &acc) {
#pragma unroll
    for (int bi = 0; bi < 4; bi++)
#pragma unroll
        for (int bj = 0; bj < 4; bj++) acc[bi][bj] = doublex4{0.0, 0.0, 0.0, 0.0};
}

// one K step of the image: 4 x (4 operand reads per side, 16 MFMAs)
__device__ __forceinline__ void acc_step(const double *img, const Lanes &l, Acc &acc) {
    const double *ap = img + (l.wm * 64 + l.l15) * kLD + l.lk, *bp = img + kTile * kLD + (l.wn * 64 + l.l15) * kLD + l.lk;
#pragma unroll
    for (int kk = 0; kk < kKC / 4; kk++) {
        double af[4], bf[4];
#pragma unroll
        for (int b = 0; b < 4; b++) {
            af[b] = ap[b * 16 * kLD + kk * 4];
            bf[b] = bp[b * 16 * kLD + kk * 4];
        }
#pragma unroll
        for (int bi = 0; bi < 4; bi++)
#pragma unroll
            for (int bj = 0; bj < 4; bj++) acc[bi][bj] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[bi], bf[bj], acc[bi][bj], 0, 0, 0);
    }
}

// acc += A B^T over K values in ceil(K / 16) steps: load(s) fills the caller's registers with step s, store() writes them to the image;
// the next step's global loads are in flight under the MFMAs.  (The step count is formed here: handed in ready-made it costs
// k_prdc_gram<false> two more AGPRs.)
template <typename Load, typename Store>
__device__ __forceinline__ void tile_loop(const double *img, int64_t K, const Lanes &l, Acc &acc, const Load &load, const Store &store) {
    const int64_t nsteps = (K + kKC - 1) / kKC;
    load(0);
    for (int64_t s = 0; s < nsteps; s++) {
        store();
        __syncthreads();
        if (s + 1 < nsteps) load(s + 1);
        acc_step(img, l, acc);
        __syncthreads();
    }
}

// the row-major staging: thread = (row sr = tid >> 1, 8-value half sk = (tid & 1) * 8 of the step)
__device__ __forceinline__ void store_rows(double *img, int sr, int sk, const double (&va)[8], const double (&vb)[8]) {
#pragma unroll
    for (int e = 0; e < 8; e++) {
        img[sr * kLD + sk + e] = va[e];
        img[kTile * kLD + sr * kLD + sk + e] = vb[e];
    }
}

}  // namespace
}  // namespace dlpm
