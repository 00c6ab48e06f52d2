// Host build of katome_amd/csrc/s2_regions.h (the 256 regions S2 of the ordered k-mer count is written into: their sizes from a
// sample, their starts, and the list of logical tiles the remaining partition pass walks).  As a shared library it is what
// tests/test_s2_regions_host.py asks through ctypes; as a program its main runs pinned cases: every check aborts with a message on
// failure, "ok <checks>" otherwise (the test runs it plain and under ASan + UBSan).
#include <stdio.h>
#include <stdlib.h>

#include "../../katome_amd/csrc/s2_regions.h"

using namespace katome;

extern "C" {

void hs_s2_sample(uint64_t n, uint64_t* rows, uint64_t* stride, uint64_t* records) {
    const S2Sample s = s2_sample_plan(n);
    *rows = s.rows; *stride = s.stride; *records = s2_sample_records(n, s);
}
void hs_s2_caps(const uint32_t* counts, uint64_t sampled, uint64_t n, uint64_t* cap) { s2_region_caps(counts, sampled, n, cap); }
void hs_s2_starts(const uint64_t* cap, uint64_t* start) { s2_region_starts(cap, start); }
void hs_s2_tiles(const uint64_t* used, uint32_t* tile_first) { s2_region_tiles(used, tile_first); }
void hs_s2_tile(uint32_t t, const uint32_t* tile_first, const uint64_t* start, const uint64_t* used, uint32_t* region, uint64_t* first, uint32_t* keys) {
    const S2Tile x = s2_region_tile(t, tile_first, start, used);
    *region = x.region; *first = x.first; *keys = x.keys;
}

}

static unsigned long long checks = 0;
#define CHECK(c) do { ++checks; if (!(c)) { fprintf(stderr, "s2_regions_host: line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

int main() {
    // ---- the sample: every row of a small level, every 32nd of a large one --------------------------------------------------------
    uint64_t rows, stride, rec;
    hs_s2_sample(0, &rows, &stride, &rec);
    CHECK(rows == 0 && rec == 0);
    hs_s2_sample(1000, &rows, &stride, &rec);
    CHECK(rows == 4 && stride == 1 && rec == 1000);
    hs_s2_sample((1ull << 22) - 1, &rows, &stride, &rec);
    CHECK(stride == 1 && rec == (1ull << 22) - 1);
    hs_s2_sample(1ull << 22, &rows, &stride, &rec);
    CHECK(stride == 32 && rows == 512 && rec == 512 * 256);
    hs_s2_sample((1ull << 22) + 1, &rows, &stride, &rec);          // (row 16384 holds one record; it is the 513th sampled row)
    CHECK(rows == 513 && rec == 512 * 256 + 1);
    hs_s2_sample(1450000000ull, &rows, &stride, &rec);
    CHECK(rec >= 1450000000ull / 32 && rec * 64 >= 1450000000ull);
    // ---- sizes: the estimate, a sixteenth, 4096 keys, whole tiles, never more than the level ------------------------------------------
    uint32_t counts[S2_REGIONS] = {0};
    uint64_t cap[S2_REGIONS], start[S2_REGIONS + 1];
    counts[0] = 1000; counts[7] = 100000; counts[255] = 1;
    hs_s2_caps(counts, 101001, 101001, cap);          // (the whole level sampled)
    CHECK(cap[0] == 2 * 4096 && cap[1] == 4096 && cap[255] == 2 * 4096);
    CHECK(cap[7] == 101001 / 4096 * 4096 + 4096);          // (100000 + 6250 + 4096 is more than the level: its 101001 keys in whole tiles)
    hs_s2_caps(counts, 101001, 101001ull * 64, cap);       // (one record in 64 sampled)
    CHECK(cap[0] == (64000 + 4000 + 4096 + 4095) / 4096 * 4096 && cap[255] == (64 + 4 + 4096 + 4095) / 4096 * 4096);
    hs_s2_starts(cap, start);
    CHECK(start[0] == 0 && start[1] == cap[0] && start[256] - start[255] == cap[255]);
    // ---- the logical tiles ----------------------------------------------------------------------------------------------------------
    uint64_t used[S2_REGIONS] = {0};
    uint32_t first[S2_REGIONS + 1];
    hs_s2_tiles(used, first);
    CHECK(first[256] == 0);
    used[3] = 1; used[4] = 4095; used[5] = 4096; used[6] = 4097; used[200] = 8192;
    for (uint32_t d = 0; d < S2_REGIONS; ++d) cap[d] = 3 * 4096;
    hs_s2_starts(cap, start);
    hs_s2_tiles(used, first);
    CHECK(first[3] == 0 && first[4] == 1 && first[5] == 2 && first[6] == 3 && first[7] == 5 && first[200] == 5 && first[201] == 7 && first[256] == 7);
    uint32_t region, keys; uint64_t at;
    hs_s2_tile(0, first, start, used, &region, &at, &keys);
    CHECK(region == 3 && at == start[3] && keys == 1);
    hs_s2_tile(3, first, start, used, &region, &at, &keys);
    CHECK(region == 6 && at == start[6] && keys == 4096);
    hs_s2_tile(4, first, start, used, &region, &at, &keys);
    CHECK(region == 6 && at == start[6] + 4096 && keys == 1);
    hs_s2_tile(6, first, start, used, &region, &at, &keys);
    CHECK(region == 200 && at == start[200] + 4096 && keys == 4096);
    printf("ok %llu\n", checks);
    return 0;
}
