// keep_plan.h -- records kept aside between batches (builder.h, KeptRecords): does the array take n_new more as it is, does it
// grow, or is keeping given up?  Nothing of HIP in here: KeptRecords::reserve (kept_records.hip) asks, and tests/hostshim compiles
// it for the host (tests/test_keep_plan_host.py holds the same rules written out in Python).
#pragma once
#include <stdint.h>

namespace katome {

// The two record sets differ in their rule, not in their code.  A record is `w` words of 8 bytes; `want` is the capacity asked for.
struct KeepPolicy {
    uint32_t first_batches;     // the first array holds this many batches like the one that asks for it; later ones double
    uint32_t copies;            // the memory test charges `want` records this many times over ...
    bool charge_kept;           // ... and the n records kept so far once more (they stay until the grown array has them)
    bool idle_counts;           // what the library's pool holds idle, and the array that is given up, count as free
    uint32_t free_div;          // ... all of it against this fraction of the free memory
    uint32_t total_div;         // the array itself may take no more than this fraction of the card
    bool limited;               // `limit` (records) applies
    bool alloc_fail_refuses;    // the allocation fails after all: give up keeping (true) or report the error (false)
    bool exact_while_empty;     // a set with nothing kept yet starts out `exact`: the host knows the count until a batch with holes comes
};
// the big-tile records: room for sixteen batches to begin with (a build is a dozen batches); the counting needs the records twice
// more -- the passes' scratch and the next level --, and no more than a sixth of the card
constexpr KeepPolicy KEEP_TILES = {16, 3, false, true, 1, 6, true, true, true};
// the left-over windows: they are sorted with the tiles' k-mers later -- past an eighth of the card they stop being a side matter.
// (That a failed allocation is an error here and a refusal above looks like an accident of two functions written apart, and so does
// asking the driver alone: the rules came through as they were, on purpose)
constexpr KeepPolicy KEEP_REST = {1, 1, true, false, 2, 8, false, false, false};

enum KeepAction { KEEP_AS_IS = 0, KEEP_GROW = 1, KEEP_REFUSE = 2 };
struct KeepPlan { KeepAction action; uint64_t want; };      // want: the new capacity in records (KEEP_GROW)

// n records kept in an array of cap, n_new to come, `words` words each; free_driver / total: what the driver reports, free_pool:
// what the library's pool holds idle (bytes); limit: no more than this many records are kept (sets with `limited`)
static inline KeepPlan keep_plan(const KeepPolicy& p, uint64_t n, uint64_t cap, uint64_t n_new, uint32_t words, uint64_t free_driver,
                                 uint64_t free_pool, uint64_t total, uint64_t limit) {
    if (n + n_new <= cap) return {KEEP_AS_IS, cap};
    const uint64_t rec = 8ull * words, first = cap ? cap * 2 : n_new * p.first_batches;
    const uint64_t want = first > n + n_new ? first : n + n_new;
    const uint64_t need = (want * p.copies + (p.charge_kept ? n : 0)) * rec;
    const uint64_t have = (free_driver + (p.idle_counts ? free_pool + cap * rec : 0)) / p.free_div;
    if ((p.limited && n + n_new > limit) || need > have || want * rec > total / p.total_div) return {KEEP_REFUSE, 0};
    return {KEEP_GROW, want};
}

}  // namespace katome
