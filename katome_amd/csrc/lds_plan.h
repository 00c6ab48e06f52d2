// lds_plan.h -- the sizes of the LDS counting tables (lds_count.hip) and the arithmetic that plans a level with them: how many
// sub-rounds, which table.  Nothing of HIP in here: the kernels take their constants from it, the host code its decisions, and
// tests/hostshim compiles it for the host (tests/test_lds_plan_host.py holds the same rules written out in Python).
#pragma once
#include <math.h>
#include <stdint.h>

namespace katome {

constexpr uint32_t LC_THREADS = 1024;          // one workgroup per CU; every thread reads PER slots of its table out
constexpr uint32_t LC_MAX_ROUNDS = 32;
#ifndef KATOME_LC_LU
#define KATOME_LC_LU 4          // records in flight per thread in the counting loops
#endif
template <int PER> struct LcTable {             // 8 B key + 4 B count (lds_count_kernel, lds_count_wide_kernel), PER = 8 or 13
    static constexpr uint32_t SLOTS = LC_THREADS * PER;
    static constexpr uint32_t FILL = (uint32_t)(SLOTS / 4096.0 * 2900);   // records a sub-round may hold at most on average (all new: load 0.71)
};
constexpr int LCS_PER = 5;                      // first-seen builds (lds_count_seen_kernel): 5120 slots of 28 bytes = 140 KiB
typedef LcTable<LCS_PER> LcsTable;
template <int LF_PER> struct LfTable {          // whole two-word keys (lds_count_full_kernel): 16 B key + 4 B count, LF_PER = 4 or 7
    static constexpr uint32_t SLOTS = LC_THREADS * LF_PER;
    static constexpr uint32_t FILL = SLOTS / 20 * 11;                  // distinct keys a group may hold (load 0.55)
};
template <int PER> struct Lf3Table {            // whole three-word keys (lds_count_full3_kernel)
    static constexpr uint32_t SLOTS = LC_THREADS * PER;                // PER = 5: 5120 x 28 B = 140 KiB; 3: 3072 x 28 B = 84 KiB
    static constexpr uint32_t FILL = SLOTS / 20 * 11;
};
constexpr uint32_t LP_PER = 19;
constexpr uint32_t LP_SLOTS = LC_THREADS * LP_PER;                    // 8-byte slots (lds_count_packed_kernel, _ordered): 19456 x 8 B = 152 KiB

static inline uint32_t at_least_one(uint64_t r) { return (uint32_t)(r ? r : 1); }
// R: the sub-rounds in which a group of `avg` records fits a table even if every record is a new key
static inline uint32_t lc_rounds(uint64_t avg, uint32_t fill) { return at_least_one((avg + fill - 1) / fill); }
// R_try: the sub-rounds of the first attempt, which takes `optimism` of a group's records for distinct
static inline uint32_t lc_rounds_try(uint64_t avg, double optimism, uint32_t fill) { return at_least_one((uint64_t)ceil((double)avg * optimism / fill)); }
// the 8-byte-slot table is planned on the guess that 56 % of a group's records are distinct (C3: 0.56), at load 0.66: R_p, its visits
// per record, and whether a group goes through in one
constexpr double LP_DISTINCT = 0.56, LP_LOAD = 0.66;
static inline uint32_t lp_rounds(uint64_t avg) { return at_least_one((uint64_t)ceil((double)avg * LP_DISTINCT / (LP_SLOTS * LP_LOAD))); }
static inline bool lp_group_fits(uint64_t avg) { return !((double)avg * LP_DISTINCT > LP_SLOTS * LP_LOAD); }
// whole keys: the small table only where it stays a third full (per_group: a group's distinct keys)
static inline bool lf_small_table(uint64_t per_group, uint32_t small_slots) { return per_group <= small_slots / 20 * 7; }
// the records of a level are within what LC_MAX_ROUNDS sub-rounds of 2^16 groups hold; a first-seen level's positions are 32-bit as well
static inline bool lc_level_fits(uint64_t n, uint32_t fill) { return (n >> 16) <= (uint64_t)LC_MAX_ROUNDS * fill; }
static inline bool lcs_level_fits(uint64_t n) { return n < (1ull << 32) && lc_level_fits(n, LcsTable::FILL); }

}  // namespace katome
