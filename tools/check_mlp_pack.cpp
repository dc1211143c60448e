// check_mlp_pack.cpp -- the host-side packing of the general toy-net forward (dlpm_amd/csrc/mlp_pack.h) as a stand-alone program,
// meant for a host sanitizer:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I dlpm_amd/csrc tools/check_mlp_pack.cpp -o check_mlp_pack
//     ./check_mlp_pack
// It lays out the 72- and the 264-unit nets of tests/mlp_general_refs.py, packs every kind of tensor into a blob of exactly the
// layout's size and checks that every real element lands where a naive index says, that every padded element is 0, that the
// regions of the blob do not overlap and that the LDS budget holds.  Exit status 0 and "ok" when all of it holds.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mlp_pack.h"

using namespace dlpm;

static int failures = 0;
#define CHECK(cond, ...)                  \
    do {                                  \
        if (!(cond)) {                    \
            if (failures++ < 20) {        \
                std::printf(__VA_ARGS__); \
                std::printf("\n");        \
            }                             \
        }                                 \
    } while (0)

// a value that names its tensor and its element, never 0
static float tag(int tensor, int n, int k) { return (float)(1 + tensor) * 1000.0f + (float)n + (float)k / 2048.0f + 0.25f; }

static void check_operand(const std::vector<float> &blob, int64_t off, int tensor, int N, int K, int NPad, int KPad) {
    const int KG = KPad / 16;
    int64_t real = 0;
    for (int j = 0; j < NPad / 16; j++)
        for (int g = 0; g < KG; g++)
            for (int l = 0; l < 64; l++)
                for (int s = 0; s < 4; s++) {
                    // the lane l of the MFMA holds column l & 15 and, in step s of group g, k = 16 g + 4 (l >> 4) + s
                    const int n = 16 * j + l % 16, k = 16 * g + 4 * (l / 16) + s;
                    const float got = blob[off + (((int64_t)j * KG + g) * 64 + l) * 4 + s];
                    if (n < N && k < K) {
                        CHECK(got == tag(tensor, n, k), "operand %d: element (%d, %d) is %g", tensor, n, k, got);
                        real++;
                    } else {
                        CHECK(got == 0.0f, "operand %d: padded element (%d, %d) is %g", tensor, n, k, got);
                    }
                }
    CHECK(real == (int64_t)N * K, "operand %d: %lld real elements, expected %lld", tensor, (long long)real, (long long)N * K);
}

static void check_net(int F, int NU, int TE, int nblocks) {
    const MlpGenLayout L = mlp_gen_layout(F, NU, TE, nblocks);
    CHECK(L.NP >= NU && L.NP % 16 == 0 && L.NP == 16 * L.W * L.NT && L.W >= 1 && L.W <= GEN_MAX_WAVES, "bad column split for %d units", NU);
    CHECK(L.TEP >= TE && L.TEP % 16 == 0 && L.TEP - TE < 16, "bad TE padding");
    CHECK((L.LD / 4) % 2 == 1 && (L.LDT / 4) % 2 == 1 && L.LD >= L.NP + 4 && L.LD >= L.TEP + 4 && L.LD >= L.W * F, "bad LDS strides");
    CHECK(mlp_gen_lds_bytes(L, 16) <= GEN_LDS_LIMIT, "a 16-row tile takes %lld bytes", (long long)mlp_gen_lds_bytes(L, 16));
    std::vector<float> blob((size_t)L.total, -7.0f);   // exactly the layout's size: a write past the end is the sanitizer's
    std::vector<char> owner((size_t)L.total, 0);
    auto claim = [&](int64_t off, int64_t n) {
        for (int64_t i = 0; i < n; i++) {
            CHECK(off + i < L.total && !owner[off + i], "blob float %lld is claimed twice or lies past the end", (long long)(off + i));
            if (off + i < L.total) owner[off + i] = 1;
        }
    };
    int tensor = 0;
    auto weight = [&](int N, int K) {
        std::vector<float> w((size_t)N * K);      // exactly N x K: a read past the end is the sanitizer's
        for (int n = 0; n < N; n++)
            for (int k = 0; k < K; k++) w[(size_t)n * K + k] = tag(tensor, n, k);
        return w;
    };
    auto operand = [&](int64_t off, int N, int K, int NPad, int KPad) {
        const std::vector<float> w = weight(N, K);
        mlp_pack_operand(&blob[off], w.data(), N, K, NPad, KPad);
        claim(off, (int64_t)NPad * KPad);
        check_operand(blob, off, tensor, N, K, NPad, KPad);
        tensor++;
    };
    auto vector = [&](int64_t off, int n, int npad) {
        const std::vector<float> v = weight(1, n);
        mlp_pack_vector(&blob[off], v.data(), n, npad);
        claim(off, npad);
        for (int i = 0; i < npad; i++)
            CHECK(blob[off + i] == (i < n ? tag(tensor, 0, i) : 0.0f), "vector %d: element %d is %g", tensor, i, blob[off + i]);
        tensor++;
    };
    vector(L.te_w, TE, L.TEP); vector(L.te_b, TE, L.TEP);
    operand(L.tm_w, TE, TE, L.TEP, L.TEP); vector(L.tm_b, TE, L.TEP);
    {
        const std::vector<float> w = weight(NU, F);
        mlp_pack_transposed(&blob[L.in_w], w.data(), NU, F, L.NP);
        claim(L.in_w, (int64_t)F * L.NP);
        for (int f = 0; f < F; f++)
            for (int n = 0; n < L.NP; n++)
                CHECK(blob[L.in_w + (int64_t)f * L.NP + n] == (n < NU ? tag(tensor, n, f) : 0.0f), "linear_in (%d, %d)", n, f);
        tensor++;
    }
    vector(L.in_b, NU, L.NP); vector(L.in_g, NU, L.NP); vector(L.in_be, NU, L.NP);
    for (int bi = 0; bi <= nblocks; bi++) {
        const int64_t b = L.blk0 + (int64_t)bi * L.blk_stride;
        operand(b + L.b_w1, NU, NU, L.NP, L.NP); vector(b + L.b_b1, NU, L.NP); vector(b + L.b_g1, NU, L.NP); vector(b + L.b_be1, NU, L.NP);
        operand(b + L.b_tw, NU, TE, L.NP, L.TEP); vector(b + L.b_tb, NU, L.NP);
        operand(b + L.b_w2, NU, NU, L.NP, L.NP); vector(b + L.b_b2, NU, L.NP); vector(b + L.b_g2, NU, L.NP); vector(b + L.b_be2, NU, L.NP);
    }
    {
        const std::vector<float> w = weight(F, NU);
        mlp_pack_rows(&blob[L.out_w], w.data(), F, NU, L.NP);
        claim(L.out_w, (int64_t)F * L.NP);
        for (int f = 0; f < F; f++)
            for (int n = 0; n < L.NP; n++)
                CHECK(blob[L.out_w + (int64_t)f * L.NP + n] == (n < NU ? tag(tensor, f, n) : 0.0f), "out (%d, %d)", f, n);
        tensor++;
    }
    vector(L.out_b, F, F);
    int64_t unclaimed = 0;
    for (int64_t i = 0; i < L.total; i++) unclaimed += !owner[i];
    CHECK(unclaimed < 4 * 64, "%lld floats of the blob belong to no tensor (only the round-up to 4 may)", (long long)unclaimed);
    std::printf("nunits %4d  TE %4d  F %d  blocks %d+1: NP %d TEP %d, %d waves x %d tiles, blob %lld floats, LDS %lld / %lld bytes at 16 / 32 rows\n",
                NU, TE, F, nblocks, L.NP, L.TEP, L.W, L.NT, (long long)L.total, (long long)mlp_gen_lds_bytes(L, 16),
                (long long)mlp_gen_lds_bytes(L, 32));
}

int main() {
    check_net(2, 72, 32, 1);      // not a multiple of 16
    check_net(2, 264, 130, 1);    // ragged TE and width across several K steps
    check_net(64, 1024, 1024, 0); // every cap at once
    check_net(1, 1, 1, 0);
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
