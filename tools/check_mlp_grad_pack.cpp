// check_mlp_grad_pack.cpp -- the host-side layout of the toy net's flat parameter vector and backward (dlpm_amd/csrc/mlp_pack.h)
// as a stand-alone program, meant for a host sanitizer:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I dlpm_amd/csrc tools/check_mlp_grad_pack.cpp -o check_mlp_grad_pack
//     ./check_mlp_grad_pack
// For the 72- and the 264-unit nets of tests/mlp_general_refs.py, with and without LayerNorm, and at the caps it fills a flat
// parameter vector with values that name their tensor and element, scatters it through the flat map into a zeroed blob of exactly
// both regions' size (what dlpm_mlp_grad_import_params_f32 does on the device) and checks that
//   - every real element of the forward's and of the transposed operands sits where a naive index says, every padded one is 0;
//   - the packing routines dlpm_mlp_finalize uses (mlp_pack_operand, mlp_pack_operand_t) give the same floats as the scatter;
//   - no two regions of the second blob region overlap and they fill it;
//   - the flat map is a bijection onto the real elements of the forward region, and onto those of the transposed region for the
//     four hidden Linears;
//   - the per-row records do not overlap, the slots cover every row once, and the LDS budget holds.
// For the lane kernels' 64-unit net (nfeatures 1, 2, 4 x time_emb_size 8, 32, 64 x nblocks 0, 1, 4) it checks the flat map into the
// lane blob the same way: every flat element has exactly one blob element, inside the blob, and a scatter through the map puts every
// tensor where the kernels read it (a Linear weight transposed, [k][unit]).
// Exit status 0 and "ok" when all of it holds.
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

// a value that names its flat index, never 0 and exact in fp32 up to 2^24 parameters
static float tag(int64_t i) { return (float)(i + 1); }

// the operand at blob[off] against a naive index: lane l of the MFMA holds column 16 j + (l & 15) and, in step s of group g,
// k = 16 g + 4 (l >> 4) + s; `at(n, k)` is the flat index of element (n, k) of the operand's matrix [N][K]
template <class At>
static void check_operand(const std::vector<float> &blob, int64_t off, const char *name, int N, int K, int NPad, int KPad, At at) {
    const int KG = KPad / 16;
    int64_t real = 0;
    for (int j = 0; j < NPad / 16; j++)
        for (int g = 0; g < KG; g++)
            for (int l = 0; l < 64; l++)
                for (int s = 0; s < 4; s++) {
                    const int n = 16 * j + l % 16, k = 16 * g + 4 * (l / 16) + s;
                    const float got = blob[off + (((int64_t)j * KG + g) * 64 + l) * 4 + s];
                    if (n < N && k < K) {
                        CHECK(got == tag(at(n, k)), "%s: element (%d, %d) is %g", name, n, k, got);
                        real++;
                    } else {
                        CHECK(got == 0.0f, "%s: padded element (%d, %d) is %g", name, n, k, got);
                    }
                }
    CHECK(real == (int64_t)N * K, "%s: %lld real elements, expected %lld", name, (long long)real, (long long)N * K);
}

static void check_net(int F, int NU, int TE, int nblocks, bool ln) {
    const MlpGenLayout L = mlp_gen_layout(F, NU, TE, nblocks);
    const MlpGenGradLayout G = mlp_gen_grad_layout(L);
    const MlpFlat f = mlp_flat(F, NU, TE, nblocks, ln);
    const int64_t total = L.total + G.total;
    CHECK(G.base == L.total && G.base % 4 == 0, "the second region does not start behind the first on a 16-byte boundary");

    // ---- the parameter count, by the module's own arithmetic
    const int64_t norm = ln ? 2 * NU : 0;
    const int64_t per_block = 2 * norm + 2 * ((int64_t)NU * NU + NU) + (int64_t)NU * TE + NU;
    const int64_t P = norm + 2 * TE + (int64_t)TE * TE + TE + (int64_t)NU * F + NU + per_block * (nblocks + 1) + (int64_t)F * NU + F;
    CHECK(f.P == P, "the flat vector has %lld floats, the modules %lld", (long long)f.P, (long long)P);
    CHECK(f.P < (1 << 24), "tags are exact up to 2^24 parameters");

    // ---- the map: in range, injective into each region
    std::vector<int64_t> fwd((size_t)f.P), tr((size_t)f.P);      // exactly P each: a write past the end is the sanitizer's
    mlp_general_flat_map(L, G, f, fwd.data(), tr.data());
    std::vector<char> owner((size_t)total, 0);
    int64_t with_t = 0;
    for (int64_t i = 0; i < f.P; i++) {
        CHECK(fwd[i] >= 0 && fwd[i] < L.total, "flat %lld maps to %lld, outside the forward region", (long long)i, (long long)fwd[i]);
        if (fwd[i] >= 0 && fwd[i] < L.total) {
            CHECK(!owner[fwd[i]], "two parameters map to blob float %lld", (long long)fwd[i]);
            owner[fwd[i]] = 1;
        }
        if (tr[i] >= 0) {
            with_t++;
            CHECK(tr[i] >= L.total && tr[i] < total, "flat %lld: transposed copy at %lld, outside the second region", (long long)i, (long long)tr[i]);
            if (tr[i] >= L.total && tr[i] < total) {
                CHECK(!owner[tr[i]], "two parameters map to blob float %lld", (long long)tr[i]);
                owner[tr[i]] = 1;
            }
        }
    }
    CHECK(with_t == (int64_t)TE * TE + (nblocks + 1) * (2 * (int64_t)NU * NU + (int64_t)NU * TE),
          "%lld parameters have a transposed copy", (long long)with_t);

    // ---- the import: scatter into a zeroed blob of exactly both regions' size
    std::vector<float> blob((size_t)total, 0.0f);
    for (int64_t i = 0; i < f.P; i++) {
        blob[fwd[i]] = tag(i);
        if (tr[i] >= 0) blob[tr[i]] = tag(i);
    }
    int64_t nonzero = 0;
    for (int64_t i = 0; i < total; i++) nonzero += blob[i] != 0.0f;
    CHECK(nonzero == f.P + with_t, "%lld floats of the blob are set, %lld expected", (long long)nonzero, (long long)(f.P + with_t));

    // ---- every region against a naive index; the second region's parts claimed once each
    std::vector<char> claimed((size_t)G.total, 0);
    auto claim = [&](int64_t off, int64_t n) {
        for (int64_t i = 0; i < n; i++) {
            CHECK(off + i < G.total && !claimed[off + i], "float %lld of the second region is claimed twice or lies past its end", (long long)(off + i));
            if (off + i < G.total) claimed[off + i] = 1;
        }
    };
    // a hidden Linear [N][K] at flat offset fo: its operand at bo, its transposed operand at to (within the second region)
    auto linear = [&](const char *name, int64_t fo, int64_t bo, int64_t to, int N, int K, int NPad, int KPad) {
        check_operand(blob, bo, name, N, K, NPad, KPad, [&](int n, int k) { return fo + (int64_t)n * K + k; });
        // transposed: the operand of the matrix [K][N], output columns over k, reduction over n
        check_operand(blob, G.base + to, name, K, N, KPad, NPad, [&](int k, int n) { return fo + (int64_t)n * K + k; });
        claim(to, (int64_t)NPad * KPad);
        // what finalize packs from the tensor itself
        std::vector<float> w((size_t)N * K), a((size_t)NPad * KPad, -7.0f), b((size_t)NPad * KPad, -7.0f);
        for (int64_t i = 0; i < (int64_t)N * K; i++) w[i] = tag(fo + i);
        mlp_pack_operand(a.data(), w.data(), N, K, NPad, KPad);
        mlp_pack_operand_t(b.data(), w.data(), N, K, NPad, KPad);
        for (int64_t i = 0; i < (int64_t)NPad * KPad; i++) {
            CHECK(a[i] == blob[bo + i], "%s: mlp_pack_operand and the scatter differ at %lld", name, (long long)i);
            CHECK(b[i] == blob[G.base + to + i], "%s: mlp_pack_operand_t and the scatter differ at %lld", name, (long long)i);
        }
    };
    auto vector = [&](const char *name, int64_t fo, int64_t bo, int n, int npad) {
        for (int i = 0; i < npad; i++)
            CHECK(blob[bo + i] == (i < n ? tag(fo + i) : 0.0f), "%s: element %d is %g", name, i, blob[bo + i]);
    };
    if (ln) { vector("group_norm_in.weight", f.in_g, L.in_g, NU, L.NP); vector("group_norm_in.bias", f.in_be, L.in_be, NU, L.NP); }
    vector("time_emb.weight", f.te_w, L.te_w, TE, L.TEP); vector("time_emb.bias", f.te_b, L.te_b, TE, L.TEP);
    linear("time_mlp.2.weight", f.tm_w, L.tm_w, G.tm_wT, TE, TE, L.TEP, L.TEP); vector("time_mlp.2.bias", f.tm_b, L.tm_b, TE, L.TEP);
    for (int k = 0; k < F; k++)
        for (int n = 0; n < L.NP; n++)
            CHECK(blob[L.in_w + (int64_t)k * L.NP + n] == (n < NU ? tag(f.in_w + (int64_t)n * F + k) : 0.0f), "linear_in (%d, %d)", n, k);
    vector("linear_in.bias", f.in_b, L.in_b, NU, L.NP);
    for (int bi = 0; bi <= nblocks; bi++) {
        const int64_t fb = f.blk0 + bi * f.blk_stride, b = L.blk0 + bi * L.blk_stride, t = G.blk0 + bi * G.blk_stride;
        if (ln) {
            vector("group_norm1.weight", fb + f.b_g1, b + L.b_g1, NU, L.NP); vector("group_norm1.bias", fb + f.b_be1, b + L.b_be1, NU, L.NP);
            vector("group_norm2.weight", fb + f.b_g2, b + L.b_g2, NU, L.NP); vector("group_norm2.bias", fb + f.b_be2, b + L.b_be2, NU, L.NP);
        }
        linear("mlp_1.1.weight", fb + f.b_w1, b + L.b_w1, t + G.b_w1T, NU, NU, L.NP, L.NP); vector("mlp_1.1.bias", fb + f.b_b1, b + L.b_b1, NU, L.NP);
        linear("t_proj.1.weight", fb + f.b_tw, b + L.b_tw, t + G.b_twT, NU, TE, L.NP, L.TEP); vector("t_proj.1.bias", fb + f.b_tb, b + L.b_tb, NU, L.NP);
        linear("mlp_2.1.weight", fb + f.b_w2, b + L.b_w2, t + G.b_w2T, NU, NU, L.NP, L.NP); vector("mlp_2.1.bias", fb + f.b_b2, b + L.b_b2, NU, L.NP);
    }
    for (int k = 0; k < F; k++)
        for (int n = 0; n < L.NP; n++)
            CHECK(blob[L.out_w + (int64_t)k * L.NP + n] == (n < NU ? tag(f.out_w + (int64_t)k * NU + n) : 0.0f), "out (%d, %d)", k, n);
    vector("outblocks_mean.1.bias", f.out_b, L.out_b, F, F);
    int64_t unclaimed = 0;
    for (int64_t i = 0; i < G.total; i++) unclaimed += !claimed[i];
    CHECK(unclaimed == 0, "%lld floats of the second region belong to no operand", (long long)unclaimed);

    // ---- the per-row records: disjoint, inside per_row
    const MlpGenRecords R = mlp_gen_records(L);
    std::vector<char> rec((size_t)R.per_row, 0);
    auto record = [&](int64_t off, int64_t width) {
        for (int64_t i = 0; i < width; i++) {
            CHECK(off + i < R.per_row && !rec[off + i], "record float %lld is claimed twice or lies past the end", (long long)(off + i));
            if (off + i < R.per_row) rec[off + i] = 1;
        }
    };
    for (int64_t o : {R.e0, R.a1, R.temb, R.da1, R.da0}) record(o, L.TEP);
    for (int64_t o : {R.nin, R.dlnin, R.dzin, R.hfin}) record(o, L.NP);
    record(R.rsin, 4);
    for (int bi = 0; bi <= nblocks; bi++) {
        const int64_t rb = R.blk0 + bi * R.blk_stride;
        for (int64_t o : {R.b_h, R.b_n1, R.b_tp, R.b_y, R.b_n2, R.b_dln1, R.b_dln2, R.b_dz1, R.b_dz2, R.b_dtp}) record(rb + o, L.NP);
        record(rb + R.b_rs, 4);
    }
    int64_t free_floats = 0;
    for (int64_t i = 0; i < R.per_row; i++) free_floats += !rec[i];
    CHECK(free_floats == 0, "%lld floats of a row's records belong to no record", (long long)free_floats);

    // ---- the slots: at most GEN_GRAD_SLOTS, whole chunks, every row once
    for (int64_t rows : {(int64_t)1, (int64_t)GEN_GRAD_RC, (int64_t)GEN_GRAD_RC + 1, (int64_t)GEN_GRAD_RC * GEN_GRAD_SLOTS + 1, (int64_t)32000}) {
        int slots;
        int64_t rps;
        mlp_gen_grad_slots(rows, &slots, &rps);
        CHECK(slots >= 1 && slots <= GEN_GRAD_SLOTS && rps % GEN_GRAD_RC == 0, "rows %lld: %d slots of %lld rows", (long long)rows, slots, (long long)rps);
        CHECK((int64_t)(slots - 1) * rps < rows && (int64_t)slots * rps >= rows, "rows %lld: the slots do not cover the rows once", (long long)rows);
        CHECK(mlp_gen_grad_workspace_bytes(L, f, rows) >= R.per_row * rows * 4 + (int64_t)slots * f.P * 8, "rows %lld: short workspace", (long long)rows);
    }
    CHECK(mlp_gen_grad_lds_bytes(L, 16) <= GEN_LDS_LIMIT, "a 16-row tile of the backward takes %lld bytes", (long long)mlp_gen_grad_lds_bytes(L, 16));
    std::printf("nunits %4d  TE %4d  F %2d  blocks %d+1  LayerNorm %d: P %lld, second region %lld floats, %lld floats per row, LDS %lld / %lld bytes at 16 / 32 rows\n",
                NU, TE, F, nblocks, (int)ln, (long long)f.P, (long long)G.total, (long long)R.per_row, (long long)mlp_gen_grad_lds_bytes(L, 16),
                (long long)mlp_gen_grad_lds_bytes(L, 32));
}

// the lane kernels' blob (mlp_lane_offsets) and the flat vector's map into it (mlp_lane_flat_map)
static void check_lane_net(int F, int TE, int nblocks) {
    int total = 0;
    const MlpOffsets o = mlp_lane_offsets(F, TE, nblocks, &total);
    const MlpFlat f = mlp_flat(F, LANE_NU, TE, nblocks, true);
    constexpr int NU = LANE_NU;
    const int64_t per_block = 4 * NU + 2 * ((int64_t)NU * NU + NU) + (int64_t)NU * TE + NU;
    const int64_t P = 2 * NU + 2 * TE + (int64_t)TE * TE + TE + (int64_t)NU * F + NU + per_block * (nblocks + 1) + (int64_t)F * NU + F;
    CHECK(f.P == P, "lane net: the flat vector has %lld floats, the modules %lld", (long long)f.P, (long long)P);
    std::vector<int64_t> map((size_t)f.P);                       // exactly P: a write past the end is the sanitizer's
    mlp_lane_flat_map(o, f, F, TE, nblocks, map.data());
    std::vector<float> blob((size_t)total, 0.0f);
    int64_t holes = 0;
    for (int64_t i = 0; i < f.P; i++) {
        if (map[i] < 0) { holes++; continue; }
        CHECK(map[i] < total, "lane net: flat %lld maps to %lld, outside the blob of %d floats", (long long)i, (long long)map[i], total);
        if (map[i] >= total) continue;
        CHECK(blob[map[i]] == 0.0f, "lane net: two parameters map to blob float %lld", (long long)map[i]);
        blob[map[i]] = tag(i);
    }
    CHECK(holes == 0, "lane net: the flat map has %lld holes", (long long)holes);
    int64_t nonzero = 0;
    for (int i = 0; i < total; i++) nonzero += blob[i] != 0.0f;
    CHECK(nonzero == f.P, "lane net: %lld floats of the blob are set, %lld expected", (long long)nonzero, (long long)f.P);
    // every tensor where the kernels read it
    auto vector = [&](const char *name, int64_t fo, int bo, int n) {
        for (int i = 0; i < n; i++) CHECK(blob[bo + i] == tag(fo + i), "lane net %s: element %d is %g", name, i, blob[bo + i]);
    };
    auto linear = [&](const char *name, int64_t fo, int bo, int N, int K, int ld) {      // W[n][k] at blob[k * ld + n]
        for (int n = 0; n < N; n++)
            for (int k = 0; k < K; k++)
                CHECK(blob[bo + k * ld + n] == tag(fo + (int64_t)n * K + k), "lane net %s: element (%d, %d) is %g", name, n, k, blob[bo + k * ld + n]);
    };
    vector("group_norm_in.weight", f.in_g, o.in_g, NU); vector("group_norm_in.bias", f.in_be, o.in_be, NU);
    vector("time_emb.weight", f.te_w, o.te_w, TE); vector("time_emb.bias", f.te_b, o.te_b, TE);
    linear("time_mlp.2.weight", f.tm_w, o.tm_w, TE, TE, TE); vector("time_mlp.2.bias", f.tm_b, o.tm_b, TE);
    linear("linear_in.weight", f.in_w, o.in_w, NU, F, NU); vector("linear_in.bias", f.in_b, o.in_b, NU);
    for (int bi = 0; bi <= nblocks; bi++) {
        const int64_t fb = f.blk0 + bi * f.blk_stride;
        const int b = o.blk0 + bi * o.blk_stride;
        vector("group_norm1.weight", fb + f.b_g1, b + o.b_g1, NU); vector("group_norm1.bias", fb + f.b_be1, b + o.b_be1, NU);
        vector("group_norm2.weight", fb + f.b_g2, b + o.b_g2, NU); vector("group_norm2.bias", fb + f.b_be2, b + o.b_be2, NU);
        linear("mlp_1.1.weight", fb + f.b_w1, b + o.b_w1, NU, NU, NU); vector("mlp_1.1.bias", fb + f.b_b1, b + o.b_b1, NU);
        linear("t_proj.1.weight", fb + f.b_tw, b + o.b_tw, NU, TE, NU); vector("t_proj.1.bias", fb + f.b_tb, b + o.b_tb, NU);
        linear("mlp_2.1.weight", fb + f.b_w2, b + o.b_w2, NU, NU, NU); vector("mlp_2.1.bias", fb + f.b_b2, b + o.b_b2, NU);
    }
    vector("outblocks_mean.1.weight", f.out_w, o.out_w, F * NU); vector("outblocks_mean.1.bias", f.out_b, o.out_b, F);
    std::printf("lane net  TE %2d  F %d  blocks %d+1: P %lld, blob %d floats\n", TE, F, nblocks, (long long)f.P, total);
}

int main() {
    check_net(2, 72, 32, 1, true);       // not a multiple of 16
    check_net(2, 72, 32, 1, false);
    check_net(2, 264, 130, 1, false);    // ragged TE and width across several K steps
    check_net(2, 264, 130, 1, true);
    check_net(64, 1024, 1024, 0, true);  // every cap at once
    check_net(1, 1, 1, 0, true);
    for (int F : {1, 2, 4})
        for (int TE : {8, 32, 64})
            for (int nblocks : {0, 1, 4}) check_lane_net(F, TE, nblocks);
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
