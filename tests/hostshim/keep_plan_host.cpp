// Host build of katome_amd/csrc/keep_plan.h (grow, keep or refuse for the records kept aside between batches).  As a shared library
// it is what tests/test_keep_plan_host.py asks through ctypes; as a program its main runs the pinned cases: every check aborts with a
// message on failure, "ok <checks>" otherwise (the test runs it plain and under ASan + UBSan).
#include <stdio.h>
#include <stdlib.h>

#include "../../katome_amd/csrc/keep_plan.h"

using namespace katome;

static const KeepPolicy& policy_of(int set) { return set == 0 ? KEEP_TILES : KEEP_REST; }

extern "C" {

// set: 0 the tile records, 1 the left-over windows; returns the action (0 keep as is, 1 grow to *want, 2 refuse)
int hs_keep_plan(int set, uint64_t n, uint64_t cap, uint64_t n_new, uint32_t words, uint64_t free_driver, uint64_t free_pool, uint64_t total,
                 uint64_t limit, uint64_t* want) {
    const KeepPlan p = keep_plan(policy_of(set), n, cap, n_new, words, free_driver, free_pool, total, limit);
    *want = p.want;
    return (int)p.action;
}
// what KeptRecords does with the policy beyond the plan: bit 0 a failed allocation refuses, bit 1 an empty set starts out exact
int hs_keep_policy_bits(int set) { return (policy_of(set).alloc_fail_refuses ? 1 : 0) | (policy_of(set).exact_while_empty ? 2 : 0); }

}

static unsigned long long checks = 0;
#define CHECK(c) do { ++checks; if (!(c)) { fprintf(stderr, "keep_plan_host: line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

static const uint64_t GiB = 1ull << 30, NONE = ~0ull;
static bool grows(int set, uint64_t n, uint64_t cap, uint64_t n_new, uint32_t w, uint64_t free_b, uint64_t pool, uint64_t total, uint64_t limit, uint64_t to) {
    uint64_t want = 0;
    return hs_keep_plan(set, n, cap, n_new, w, free_b, pool, total, limit, &want) == KEEP_GROW && want == to;
}
static bool refuses(int set, uint64_t n, uint64_t cap, uint64_t n_new, uint32_t w, uint64_t free_b, uint64_t pool, uint64_t total, uint64_t limit) {
    uint64_t want = 0;
    return hs_keep_plan(set, n, cap, n_new, w, free_b, pool, total, limit, &want) == KEEP_REFUSE;
}

int main() {
    // ---- the tile records: sixteen batches to begin with, doubled after that ---------------------------------------------------
    CHECK(grows(0, 0, 0, 100, 2, 200 * GiB, 0, 288 * GiB, NONE, 1600));
    CHECK(grows(0, 1600, 1600, 100, 2, 200 * GiB, 0, 288 * GiB, NONE, 3200));
    CHECK(grows(0, 1600, 1600, 5000, 2, 200 * GiB, 0, 288 * GiB, NONE, 6600));          // (a batch larger than the doubling)
    uint64_t want = 7;
    CHECK(hs_keep_plan(0, 1500, 1600, 100, 2, 0, 0, 0, 0, &want) == KEEP_AS_IS);          // (room: nothing is asked, not even the limit)
    // the limit counts records handed over
    CHECK(grows(0, 8000, 8000, 1000, 2, 200 * GiB, 0, 288 * GiB, 9000, 16000));
    CHECK(refuses(0, 8000, 8000, 1001, 2, 200 * GiB, 0, 288 * GiB, 9000));
    // three times the new array against the free memory, the pool's idle bytes and the old array: 3 * 1600 * 16 = 76800
    CHECK(grows(0, 0, 0, 100, 2, 76800, 0, 288 * GiB, NONE, 1600) && refuses(0, 0, 0, 100, 2, 76799, 0, 288 * GiB, NONE));
    CHECK(grows(0, 0, 0, 100, 2, 70000, 6800, 288 * GiB, NONE, 1600) && refuses(0, 0, 0, 100, 2, 70000, 6799, 288 * GiB, NONE));
    CHECK(grows(0, 800, 800, 100, 2, 76800 - 800 * 16, 0, 288 * GiB, NONE, 1600) && refuses(0, 800, 800, 100, 2, 76800 - 800 * 16 - 1, 0, 288 * GiB, NONE));
    // a sixth of the card: 1600 * 16 = 25600 bytes of 153600
    CHECK(grows(0, 0, 0, 100, 2, 200 * GiB, 0, 153600, NONE, 1600) && refuses(0, 0, 0, 100, 2, 200 * GiB, 0, 153599, NONE));
    // ---- the left-over windows: what is needed, at least doubled ---------------------------------------------------------------
    CHECK(grows(1, 0, 0, 100, 1, 200 * GiB, 0, 288 * GiB, NONE, 100));
    CHECK(grows(1, 100, 100, 100, 1, 200 * GiB, 0, 288 * GiB, NONE, 200));
    CHECK(grows(1, 200, 200, 100, 1, 200 * GiB, 0, 288 * GiB, NONE, 400));
    CHECK(grows(1, 200, 200, 100, 1, 200 * GiB, 0, 288 * GiB, 0, 400));                 // (no limit on this set)
    // the new array and the records kept against half of the driver's free memory, whatever the pool holds: (400 + 200) * 8 = 4800
    CHECK(grows(1, 200, 200, 100, 1, 9600, 0, 288 * GiB, NONE, 400) && refuses(1, 200, 200, 100, 1, 9599, 0, 288 * GiB, NONE));
    CHECK(grows(1, 200, 200, 100, 1, 9601, 0, 288 * GiB, NONE, 400));                   // (half of an odd number rounds down)
    CHECK(refuses(1, 200, 200, 100, 1, 9599, 200 * GiB, 288 * GiB, NONE) && grows(1, 200, 200, 100, 1, 9600, 200 * GiB, 288 * GiB, NONE, 400));
    // an eighth of the card: 400 * 8 = 3200 bytes of 25600
    CHECK(grows(1, 200, 200, 100, 1, 200 * GiB, 0, 25600, NONE, 400) && refuses(1, 200, 200, 100, 1, 200 * GiB, 0, 25599, NONE));
    // ---- what a failed allocation and an empty set mean ------------------------------------------------------------------------
    CHECK(hs_keep_policy_bits(0) == 3 && hs_keep_policy_bits(1) == 0);
    printf("ok %llu\n", checks);
    return 0;
}
