// w1_layout.h -- the host-side arithmetic of w1.hip in plain C++ (no HIP header), so that tools/check_w1_layout.cpp can run it under a
// host sanitizer: the limits, the packing of a bid and its bidder into one 64-bit key, the bound on every price the auction can
// reach, and the carving of the workspace.  `CarveT` is metrics_common.h's Carve in the library.
#pragma once
#include <cstdint>

namespace dlpm {

constexpr int64_t kW1MaxN = 32768, kW1MaxD = 4096;
constexpr int kW1QBits = 24;                    // every integer cost lies in [0, 2^24]
constexpr int kW1PersonBits = 15;               // a person index < 2^15 = kW1MaxN
constexpr int kW1BidBits = 48;                  // every bid < 2^48: key = bid << 15 | (32767 - person) < 2^63
constexpr int64_t kW1PersonMask = (1ll << kW1PersonBits) - 1;

// key of (bid, person): larger for a higher bid, and among equal bids for the LOWER person; 0 = "no bid yet" (a bid is >= 1)
constexpr uint64_t w1_key(int64_t bid, int64_t person) { return ((uint64_t)bid << kW1PersonBits) | (uint64_t)(kW1PersonMask - person); }

// An upper bound on every price (hence on every bid) of the whole solve, DESIGN 3.22: with C = qmax (n + 1) a phase of step eps
// raises the largest price by at most 2 (C + eps), and the phases are eps_0 = max(1, C / 2), eps_{k+1} = max(1, eps_k / 4) down to 1.
inline int64_t w1_price_bound(int64_t n, int64_t qmax) {
    const int64_t C = qmax * (n + 1);
    int64_t eps = C / 2 > 1 ? C / 2 : 1, bound = 0;
    for (;;) {
        bound += 2 * (C + eps);
        if (eps == 1) break;
        eps = eps / 4 > 1 ? eps / 4 : 1;
    }
    return bound;
}

// byte offsets of the regions of the workspace; ld = the row pitch of q in int32 (n rounded up to 4: rows are read 16 bytes at a time)
struct W1Layout {
    int64_t ld, hdr, q, prices, keys, owner, assigned, bidobj, list0, list1, total;
};

constexpr int64_t kW1HeaderBytes = 256;

template <typename CarveT>
inline W1Layout w1_layout_of(int64_t n) {
    W1Layout L{};
    CarveT c;
    L.ld = (n + 3) / 4 * 4;
    L.hdr = c.take(kW1HeaderBytes);
    L.q = c.take(n * L.ld * 4);          // int32 [n][ld]
    L.prices = c.take(n * 8);            // int64 [n]: price of object j
    L.keys = c.take(n * 8);              // uint64 [n]: best (bid, person) key of object j in this phase
    L.owner = c.take(n * 4);             // int32 [n]: person holding object j, -1 = nobody
    L.assigned = c.take(n * 4);          // int32 [n]: object of person i, -1 = unassigned
    L.bidobj = c.take(n * 4);            // int32 [n]: the object person i bid on in this round
    L.list0 = c.take(n * 4);             // int32 [n] x 2: the unassigned persons of this round and of the next
    L.list1 = c.take(n * 4);
    L.total = c.total;
    return L;
}

}  // namespace dlpm
