// Host build of katome_amd/csrc/lds_plan.h for the CPU tests (tests/test_lds_plan_host.py).
#include "../../katome_amd/csrc/lds_plan.h"

using namespace katome;

extern "C" {

// {slots, fill} of a table shape: 0 LcTable<8>, 1 LcTable<13>, 2 the first-seen table, 3 / 4 LfTable<4> / <7>, 5 / 6 Lf3Table<3> / <5>,
// 7 the 8-byte slots (no fill: planned by lp_rounds); then {LC_THREADS, LC_MAX_ROUNDS}
void hs_lds_table(int shape, uint32_t out[2]) {
    switch (shape) {
        case 0: out[0] = LcTable<8>::SLOTS; out[1] = LcTable<8>::FILL; break;
        case 1: out[0] = LcTable<13>::SLOTS; out[1] = LcTable<13>::FILL; break;
        case 2: out[0] = LcsTable::SLOTS; out[1] = LcsTable::FILL; break;
        case 3: out[0] = LfTable<4>::SLOTS; out[1] = LfTable<4>::FILL; break;
        case 4: out[0] = LfTable<7>::SLOTS; out[1] = LfTable<7>::FILL; break;
        case 5: out[0] = Lf3Table<3>::SLOTS; out[1] = Lf3Table<3>::FILL; break;
        case 6: out[0] = Lf3Table<5>::SLOTS; out[1] = Lf3Table<5>::FILL; break;
        case 7: out[0] = LP_SLOTS; out[1] = 0; break;
        default: out[0] = LC_THREADS; out[1] = LC_MAX_ROUNDS;
    }
}
uint32_t hs_lc_rounds(uint64_t avg, uint32_t fill) { return lc_rounds(avg, fill); }
uint32_t hs_lc_rounds_try(uint64_t avg, double optimism, uint32_t fill) { return lc_rounds_try(avg, optimism, fill); }
uint32_t hs_lp_rounds(uint64_t avg) { return lp_rounds(avg); }
int hs_lp_group_fits(uint64_t avg) { return lp_group_fits(avg); }
int hs_lf_small_table(uint64_t per_group, uint32_t small_slots) { return lf_small_table(per_group, small_slots); }
int hs_lc_level_fits(uint64_t n, uint32_t fill) { return lc_level_fits(n, fill); }
int hs_lcs_level_fits(uint64_t n) { return lcs_level_fits(n); }

}
