// check_w1_layout.cpp -- the host-side arithmetic of the exact W1 (dlpm_amd/csrc/w1_layout.h) as a stand-alone program, meant for a
// host sanitizer:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I dlpm_amd/csrc tools/check_w1_layout.cpp -o check_w1_layout
//     ./check_w1_layout
// It checks, for n in {1, 2, 63, 4096, 32768},
//   - the workspace carve: every region starts on a multiple of 256 bytes, holds what w1.hip puts there, no two regions overlap, they
//     come in ascending order and the last one ends within `total` (printed, so that a test can compare it with
//     dlpm_w1_workspace_bytes); a byte map of the small layouts is painted region by region (the sanitizer watches the painting);
//   - the row pitch of q: a multiple of 4 values, at least n;
// and at n = 32768 with qmax = 2^24 - 1 and 2^24 (the largest integer cost the quantisation can give)
//   - the price bound of DESIGN 3.22 lies below 2^48, the width of the bid field;
//   - the key of (bound, person) fits 63 bits, orders by bid first and by the LOWER person among equal bids, and unpacks to what went in;
//   - a benefit minus a price, -C - bound, is far inside int64.
// The carve below is a copy of metrics_common.h's Carve (which sits behind the HIP headers): 256-byte granules.
// Exit status 0 and "ok" when all of it holds.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "w1_layout.h"

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

struct Carve {
    int64_t total = 0;
    int64_t take(int64_t bytes) {
        const int64_t at = total;
        total += (bytes + 255) / 256 * 256;
        return at;
    }
};

struct Region {
    const char *name;
    int64_t at, bytes;
};

static void check_layout(int64_t n) {
    const W1Layout L = w1_layout_of<Carve>(n);
    CHECK(L.ld >= n && L.ld % 4 == 0 && L.ld < n + 4, "n %lld: row pitch %lld", (long long)n, (long long)L.ld);
    const Region regions[] = {{"hdr", L.hdr, kW1HeaderBytes}, {"q", L.q, n * L.ld * 4},  {"prices", L.prices, n * 8},
                              {"keys", L.keys, n * 8},        {"owner", L.owner, n * 4}, {"assigned", L.assigned, n * 4},
                              {"bidobj", L.bidobj, n * 4},    {"list0", L.list0, n * 4}, {"list1", L.list1, n * 4}};
    int64_t end = 0;
    for (const Region &r : regions) {
        CHECK(r.at % 256 == 0, "n %lld: region %s starts at %lld", (long long)n, r.name, (long long)r.at);
        CHECK(r.at >= end, "n %lld: region %s at %lld overlaps its predecessor, which ends at %lld", (long long)n, r.name, (long long)r.at,
              (long long)end);
        CHECK(r.bytes > 0, "n %lld: region %s is empty", (long long)n, r.name);
        end = r.at + r.bytes;
    }
    CHECK(end <= L.total && L.total - end < 256 && L.total % 256 == 0, "n %lld: regions end at %lld, total %lld", (long long)n,
          (long long)end, (long long)L.total);
    if (L.total <= (1 << 26)) {              // paint every byte of every region once
        std::vector<unsigned char> map((size_t)L.total, 0);
        for (const Region &r : regions)
            for (int64_t b = 0; b < r.bytes; b++) {
                CHECK(map[(size_t)(r.at + b)] == 0, "n %lld: byte %lld of %s is taken", (long long)n, (long long)b, r.name);
                map[(size_t)(r.at + b)] = 1;
            }
    }
    std::printf("n %lld: total %lld\n", (long long)n, (long long)L.total);
}

static void check_keys(int64_t n, int64_t qmax) {
    const int64_t C = qmax * (n + 1), bound = w1_price_bound(n, qmax);
    CHECK(bound > C && bound < (1ll << kW1BidBits), "qmax %lld: price bound %lld outside (C, 2^%d)", (long long)qmax, (long long)bound,
          kW1BidBits);
    CHECK(n - 1 <= kW1PersonMask, "person field");
    CHECK(kW1BidBits + kW1PersonBits <= 63, "key wider than 63 bits");
    const uint64_t top = w1_key(bound, 0);
    CHECK(top < (1ull << 63), "qmax %lld: key %llu does not fit 63 bits", (long long)qmax, (unsigned long long)top);
    CHECK((int64_t)(top >> kW1PersonBits) == bound && kW1PersonMask - (int64_t)(top & (uint64_t)kW1PersonMask) == 0, "unpack of the top key");
    const int64_t bids[] = {1, 2, C, bound - 1, bound}, persons[] = {0, 1, n / 2, n - 2, n - 1};
    for (int64_t b1 : bids)
        for (int64_t p1 : persons) {
            const uint64_t k1 = w1_key(b1, p1);
            CHECK(k1 > 0, "a key of a bid is never the empty key");
            CHECK((int64_t)(k1 >> kW1PersonBits) == b1 && kW1PersonMask - (int64_t)(k1 & (uint64_t)kW1PersonMask) == p1, "unpack (%lld, %lld)",
                  (long long)b1, (long long)p1);
            for (int64_t b2 : bids)
                for (int64_t p2 : persons) {
                    const bool wins = b1 > b2 || (b1 == b2 && p1 < p2);
                    CHECK((k1 > w1_key(b2, p2)) == wins, "order of (%lld, %lld) against (%lld, %lld)", (long long)b1, (long long)p1,
                          (long long)b2, (long long)p2);
                }
        }
    // v = a - p >= -C - bound, and the sentinel of "no value" is INT64_MIN
    CHECK(-C - bound > INT64_MIN / 2, "values");
    std::printf("n %lld qmax %lld: C %lld, price bound %lld = 2^%.2f\n", (long long)n, (long long)qmax, (long long)C, (long long)bound,
                __builtin_log2((double)bound));
}

int main() {
    for (int64_t n : {1ll, 2ll, 63ll, 4096ll, 32768ll}) check_layout(n);
    check_keys(kW1MaxN, (1ll << kW1QBits) - 1);
    check_keys(kW1MaxN, 1ll << kW1QBits);
    if (failures) {
        std::printf("%d failure(s)\n", failures);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
