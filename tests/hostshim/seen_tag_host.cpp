// Host build of katome_amd/csrc/seen_tag.h (the delta tag of a first-seen build's tagged records) with its own main: every check
// aborts with a message on failure, "ok <checks>" otherwise (tests/test_seen_tag_host.py runs it plain and under ASan + UBSan).
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <map>
#include <random>
#include <vector>

#include "../../katome_amd/csrc/seen_tag.h"

using namespace katome;

static unsigned long long checks = 0;
#define CHECK(c) do { ++checks; if (!(c)) { fprintf(stderr, "seen_tag_host: line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

static void round_trip(u64 P, u64 Q) {
    CHECK(delta_packs(P, Q));
    const u64 t = delta_pack(P, Q);
    CHECK(delta_p(t) == P && delta_q(t) == Q);
    if (Q >= DELTA_P_LIMIT) return;                     // (only the first number has a limit of its own: no other orientation to pack)
    const u64 s = delta_swap(t);                        // the other orientation: the two numbers change places
    CHECK(delta_packs(Q, P) && delta_p(s) == Q && delta_q(s) == P && delta_swap(s) == t);
}

// the numbers of a read of W windows whose range starts at `base` (pt_graph.rs:282-308): window i goes in at base + i, its reverse
// complement at base + 2W - 1 - i
static u64 fwd_no(u64 base, u32 i) { return base + i; }
static u64 rev_no(u64 base, u32 W, u32 i) { return base + 2ull * W - 1 - i; }

int main() {
    // ---- limits -------------------------------------------------------------------------------------------------------
    const u64 top = DELTA_P_LIMIT - 1;                  // 2^47 - 1
    round_trip(0, 0); round_trip(0, 65535); round_trip(65535, 0); round_trip(top, top);
    round_trip(top, top - 65535); round_trip(top - 65535, top); round_trip(top, top + 65535);
    CHECK(!delta_packs(0, 65536) && !delta_packs(65536, 0) && !delta_packs(top, top - 65536) && !delta_packs(top, top + 65536));
    CHECK(!delta_packs(DELTA_P_LIMIT, DELTA_P_LIMIT) && !delta_packs(~0ull, ~0ull));
    CHECK(2ull * DELTA_MAX_WINDOWS < DELTA_BIAS);       // |Q - P| < 2 W: a read of DELTA_MAX_WINDOWS windows packs wherever a record lies in it

    // ---- the sub-window rule against a literal loop over a read's windows ---------------------------------------------------
    // a tile of n_sub sub-tiles of `stride` windows each, first window i0: P and Q are the numbers of its first window as cut and of
    // the first window of its reverse complement; sub-tile o must get the numbers of ITS first window on either strand
    std::mt19937_64 rng(12345);
    for (int trial = 0; trial < 2000; ++trial) {
        const u32 stride = 1 + rng() % 9, n_sub = 1 + rng() % 33, span = stride * n_sub;
        const u32 W = span + rng() % 300, i0 = rng() % (W - span + 1);
        const u64 base = rng() % (1ull << 40);
        // first window of a stretch of s windows starting at i: forward base + i; its reverse complement starts with rc(window i + s - 1)
        const u64 P = fwd_no(base, i0), Q = rev_no(base, W, i0 + span - 1);
        CHECK(Q == base + 2ull * W - i0 - span);        // (seq_pair.h, var_seq_pair's Q)
        round_trip(P, Q);
        for (u32 o = 0; o < n_sub; ++o) {
            u64 Ps, Qs;
            delta_sub(P, Q, o, n_sub, stride, Ps, Qs);
            const u32 i = i0 + o * stride;
            CHECK(Ps == fwd_no(base, i) && Qs == rev_no(base, W, i + stride - 1));
            CHECK(delta_packs(Ps, Qs));
        }
    }

    // ---- the ordering claim: minima taken record by record, through the tags, are the minima of the true numbers and pack again ------
    for (int set = 0; set < 10000; ++set) {
        const u32 n_reads = 1 + rng() % 12, n_keys = 1 + rng() % 20;
        u64 base = rng() % (1ull << 44);
        struct Min { u64 p = ~0ull, q = ~0ull, tp = ~0ull, tq = ~0ull; };
        std::map<u32, Min> by_key;
        for (u32 r = 0; r < n_reads; ++r) {
            const u32 W = set % 50 == 0 ? DELTA_MAX_WINDOWS - rng() % 3 : 1 + rng() % 200;
            const u32 step = W > 1000 ? 997 : 1;        // (a long read: a sample of its windows, the last one included)
            for (u32 i = 0; i < W; i += (i + step < W || i == W - 1) ? step : W - 1 - i) {
                const u32 key = rng() % n_keys;
                const bool flipped = (rng() & 1) != 0;  // the stored orientation is the reverse complement of what the read holds
                const u64 a = fwd_no(base, i), b = rev_no(base, W, i);
                const u64 P = flipped ? b : a, Q = flipped ? a : b;
                CHECK(delta_packs(P, Q));
                const u64 t = delta_pack(P, Q);
                Min& m = by_key[key];
                m.p = std::min(m.p, P); m.q = std::min(m.q, Q);                              // the true numbers
                m.tp = std::min(m.tp, delta_p(t)); m.tq = std::min(m.tq, delta_q(t));      // what the counting kernel lowers
            }
            base += 2ull * W;                           // the next read's range: disjoint, ascending
        }
        for (const auto& kv : by_key) {
            const Min& m = kv.second;
            CHECK(m.tp == m.p && m.tq == m.q);
            CHECK(delta_packs(m.tp, m.tq));             // both from the first read that holds the key: the list entry packs
            const u64 t = delta_pack(m.tp, m.tq);
            CHECK(delta_p(t) == m.p && delta_q(t) == m.q);
        }
    }
    printf("ok %llu\n", checks);
    return 0;
}
