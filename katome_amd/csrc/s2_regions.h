// s2_regions.h -- S2 of the ordered k-mer count written by its first partition digit (lds_count.hip, lds_count_ordered_kernel with
// REGIONS): 256 regions, one per value of bits 2k - 16 .. 2k - 9 of a reverse complement, each a whole number of sort tiles with an
// append cursor of its own.  Here the arithmetic: which records are sampled for the regions' sizes, the sizes and starts from the
// sample's digit counts, and the table that lets the remaining partition pass walk the regions' used parts as one list of tiles.
// Nothing of HIP in here: ordered_count and dev_s2_region_pass ask, and tests/hostshim compiles it for the host
// (tests/test_s2_regions_host.py).
#pragma once
#include <stdint.h>

namespace katome {

constexpr uint32_t S2_REGIONS = 256;
constexpr uint64_t S2_REGION_TILE = 4096;            // keys of a sort tile of one-word records (radix.hip asserts it is SortTile<1>::KEYS)
constexpr uint64_t S2_SAMPLE_ROW = 256;              // the sample is whole rows of this many records ...
constexpr uint64_t S2_SAMPLE_ALL = 1ull << 22;       // ... every row of a level below this many records ...
constexpr uint64_t S2_SAMPLE_STRIDE = 32;            // ... else every 32nd: n / 32 records or more, never fewer than n / 64
constexpr uint64_t S2_REGION_SLACK = 4096;           // keys a region takes beyond its estimate and a sixteenth of it
// The level's records from which the regions pay (KATOME_S2_REGIONS=1).  A group costs the count kernel about 10 000 shader clocks
// more whatever it holds (five barriers, the bins' scan, the cursors' round trip, which a small group's reorder does not cover) and
// 1.6 more per kept key; the pass it saves is worth 4.7 per key.  So a group pays from about 3 100 kept keys.  The kept keys are
// not known before the count, the records are: 1.45e9 records of 1.8 to a key gain 3 ms (12 300 kept keys to a group), 5.5e8 of 4.2
// to a key lose 0.4 to 0.6 ms (2 000 to a group) -- profiles/r22_s2_regions.md.  From 2^30 records on a group has 16 384 of them.
constexpr uint64_t S2_REGIONS_MIN_RECORDS = 1ull << 30;

static inline uint64_t s2_tiles(uint64_t keys) { return (keys + S2_REGION_TILE - 1) / S2_REGION_TILE; }

// The sample of n records: rows r * stride, r = 0 .. rows - 1, of S2_SAMPLE_ROW records each (the level's last row may be short)
struct S2Sample { uint64_t rows, stride; };
static inline S2Sample s2_sample_plan(uint64_t n) {
    const uint64_t all = (n + S2_SAMPLE_ROW - 1) / S2_SAMPLE_ROW;
    if (n < S2_SAMPLE_ALL) return {all, 1};
    return {(all + S2_SAMPLE_STRIDE - 1) / S2_SAMPLE_STRIDE, S2_SAMPLE_STRIDE};
}
static inline uint64_t s2_sample_records(uint64_t n, const S2Sample& s) {
    if (!s.rows) return 0;
    const uint64_t last = (s.rows - 1) * s.stride * S2_SAMPLE_ROW;          // first record of the last sampled row
    return (s.rows - 1) * S2_SAMPLE_ROW + (n - last < S2_SAMPLE_ROW ? n - last : S2_SAMPLE_ROW);
}

// cap[d]: the keys region d takes, a whole number of tiles.  counts[d]: the sampled records whose reverse complement has first digit
// d, `sampled` of them in all, of a level of n records.  A region's kept distinct keys never outnumber the level's records with its
// digit, so with the whole level sampled the estimate is a bound; with a sample it is scaled, and a sixteenth and S2_REGION_SLACK on
// top take the sample's error (a region that fills all the same is the way back's business, not an error).  The estimates are
// rounded down: they add up to n at most, the regions to n + n / 16 + 512 tiles at most.
static inline void s2_region_caps(const uint32_t counts[S2_REGIONS], uint64_t sampled, uint64_t n, uint64_t cap[S2_REGIONS]) {
    for (uint32_t d = 0; d < S2_REGIONS; ++d) {
        const uint64_t est = sampled ? (uint64_t)(((unsigned __int128)counts[d] * n) / sampled) : 0;
        uint64_t c = est + est / 16 + S2_REGION_SLACK;
        if (c > n) c = n;
        cap[d] = s2_tiles(c) * S2_REGION_TILE;
    }
}
// start[d]: region d's first key; start[S2_REGIONS]: the keys of all regions
static inline void s2_region_starts(const uint64_t cap[S2_REGIONS], uint64_t start[S2_REGIONS + 1]) {
    start[0] = 0;
    for (uint32_t d = 0; d < S2_REGIONS; ++d) start[d + 1] = start[d] + cap[d];
}
// The regions' used parts as one list of tiles in digit order: region d holds the logical tiles tile_first[d] .. tile_first[d + 1],
// ceil(used[d] / 4096) of them -- the last one partial, none for an empty region; tile_first[S2_REGIONS] is their number.
static inline void s2_region_tiles(const uint64_t used[S2_REGIONS], uint32_t tile_first[S2_REGIONS + 1]) {
    tile_first[0] = 0;
    for (uint32_t d = 0; d < S2_REGIONS; ++d) tile_first[d + 1] = tile_first[d] + (uint32_t)s2_tiles(used[d]);
}
// logical tile t (< tile_first[S2_REGIONS]): its region, its first key's index in the region arrays and its keys
struct S2Tile { uint32_t region; uint64_t first; uint32_t keys; };
static inline S2Tile s2_region_tile(uint32_t t, const uint32_t tile_first[S2_REGIONS + 1], const uint64_t start[S2_REGIONS],
                                    const uint64_t used[S2_REGIONS]) {
    uint32_t lo = 0, hi = S2_REGIONS;          // the last region whose first tile is not beyond t: never an empty one
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) / 2; if (tile_first[mid] <= t) lo = mid; else hi = mid; }
    const uint64_t at = (uint64_t)(t - tile_first[lo]) * S2_REGION_TILE, left = used[lo] - at;
    return {lo, start[lo] + at, (uint32_t)(left < S2_REGION_TILE ? left : S2_REGION_TILE)};
}

}  // namespace katome
