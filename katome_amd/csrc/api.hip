// api.hip -- the device half of the C ABI of include/katome_gpu.h (katome_dev_*, the counting levels, finalize): the
// build driver behind `Build::create` (reference src/katome/algorithms/builder.rs:42-54) and the PtGraph::create
// post-pass (collections/graphs/pt_graph.rs:333-345), composed from the kernels in extract.hip, table.hip, radix.hip,
// node_ids.hip and first_seen.hip.  The entries that take and return host memory are in host_build.cpp.  No CPU
// fallback: every entry that needs the device fails with KATOME_E_DEVICE when there is none.
#include <stdlib.h>

#include <algorithm>
#include <chrono>
#include <memory>
#include <new>
#include <vector>

#include "builder.h"
#include "seen_tag.h"

extern "C" {

uint32_t katome_abi_version(void) { return KATOME_ABI_VERSION; }
const char* katome_last_error(void) { return get_error(); }
uint32_t katome_record_words(uint32_t k) { return (uint32_t)key_words_for_k(k); }

int katome_builder_create(const katome_settings* s, katome_builder** out) {
    if (!s || !out) { set_error("null argument"); return KATOME_E_ARG; }
    *out = nullptr;
    KCHECK(check_k(s->k));
    KCHECK(use_device(s->device));
    katome_builder* b = new (std::nothrow) katome_builder();
    if (!b) { set_error("out of host memory"); return KATOME_E_OOM; }
    b->s = *s;
    b->nw = (uint32_t)key_words_for_k(s->k);
    b->rc = s->reverse_complement != 0;
    b->first_seen = (s->flags & KATOME_FLAG_FIRST_SEEN_ORDER) != 0;
    if ((s->flags & KATOME_FLAG_REMOVE_DEAD_PATHS) && !b->first_seen) {
        delete b;
        set_error("KATOME_FLAG_REMOVE_DEAD_PATHS needs KATOME_FLAG_FIRST_SEEN_ORDER: the reference's pruning depends on petgraph's numbering");
        return KATOME_E_ARG;
    }
    b->table.track_seen = b->tiles.track_seen = b->tiles2.track_seen = b->first_seen;
    *out = b;
    return KATOME_OK;
}

void katome_builder_destroy(katome_builder* b) {
    if (!b) return;
    (void)hipSetDevice(b->s.device);
    delete b;
}

// first-seen order numbers window i of read r as r * 2W + i: every fixed-length batch of a build must have the same length
// (reads of several lengths go through katome_dev_extract_var*, which numbers by window prefix sums)
static int check_seen_len(katome_builder* b, uint32_t read_len) {
    if (b->first_seen && b->reads_inserted && b->seen_read_len && b->seen_read_len != read_len) {
        set_error("first-seen order: fixed-length batches of %u and %u bases in one build (use the variable-length entry points)", b->seen_read_len, read_len);
        return KATOME_E_ARG;
    }
    return KATOME_OK;
}

int katome_dev_extract_fixed(katome_builder* b, const uint8_t* d_packed, uint64_t n_reads, uint32_t read_len,
                             const uint8_t* d_skip, uint64_t* d_records, void* stream) {
    KCHECK_HIP(hipSetDevice(b->s.device));
    KCHECK(check_seen_len(b, read_len));
    PhaseScope ps(b->prof, PH_EXTRACT, (hipStream_t)stream);
    b->seen_read_len = read_len;
    return launch_extract_fixed(b->s.k, b->rc, d_packed, n_reads, read_len, d_skip, d_records, (hipStream_t)stream, 1,
                                b->first_seen && b->rc);
}

// Tiled counting (table.hip): largest span in 2..32 that divides the windows per read and keeps the tile in 128 bits
uint32_t katome_tile_span(uint32_t k, uint32_t read_len) {
    if (getenv("KATOME_NO_TILES") || read_len < k) return 1;
    const uint32_t W = read_len - k + 1;
    if (const char* e = getenv("KATOME_TILE_SPAN")) {        // experiments: any span that divides W and fits 128 bits
        const uint32_t s = (uint32_t)atoi(e);
        if (s >= 1 && W % s == 0 && k + s - 1 <= 63) return s;
    }
    for (uint32_t s = 32; s >= 2; --s) if (W % s == 0 && k + s - 1 <= 63) return s;
    return 1;
}
// how a read of `read_len` bases is best counted: `tiles` tiles of `span` windows from the front, then `remainder`
// single windows.  Fewest table insertions per read; spans above 16 without a divisor to break them into mid tiles
// (two-level expansion) are charged for it.  Tiles may take up to `max_tile_words` u64 words (3: 95 bases, which is what
// lets k = 63 be tiled at all).  Returns 0 (span 1) when tiling does not pay or is switched off.
uint32_t katome_tile_plan_limited(uint32_t k, uint32_t read_len, uint32_t max_tile_words, uint32_t* span, uint32_t* tiles,
                                  uint32_t* remainder) {
    uint32_t best_s = 1, best_cost = 0xFFFFFFFFu;
    const uint32_t W = read_len >= k ? read_len - k + 1 : 0;
    const uint32_t max_bases = max_tile_words >= 3 ? 95u : max_tile_words == 2 ? 63u : 31u;
    if (W >= 2 && !getenv("KATOME_NO_TILES")) {
        if (const char* e = getenv("KATOME_TILE_SPAN")) {
            const uint32_t s = (uint32_t)atoi(e);
            if (s >= 2 && s <= W && k + s - 1 <= max_bases) { best_s = s; best_cost = 0; }
        }
        for (uint32_t s = 2; best_cost != 0 && s <= TILE_SPAN_MAX && s <= W && k + s - 1 <= max_bases; ++s) {
            const uint32_t cost = tile_cost(W, s);
            if (cost < best_cost || (cost == best_cost && s > best_s)) { best_cost = cost; best_s = s; }
        }
        if (best_cost != 0 && best_cost >= W) best_s = 1;
    }
    if (span) *span = best_s;
    if (tiles) *tiles = best_s > 1 ? W / best_s : 0;
    if (remainder) *remainder = best_s > 1 ? W % best_s : W;
    return best_s > 1;
}
uint32_t katome_tile_plan(uint32_t k, uint32_t read_len, uint32_t* span, uint32_t* tiles, uint32_t* remainder) {
    return katome_tile_plan_limited(k, read_len, 3, span, tiles, remainder);
}
uint32_t katome_tile_words(uint32_t k, uint32_t span) { return (uint32_t)key_words_for_k(k + span - 1); }

}  // extern "C"

// The same plan for reads of several lengths (`len`, none shorter than k): one span for the whole input, the one with the fewest
// table insertions over all reads -- tiles from the front of every read + the windows left over.  1: tiling does not pay.
uint32_t tile_span_for_lengths(uint32_t k, const uint32_t* len, uint64_t n_reads, uint64_t total_windows) {
    if (getenv("KATOME_NO_TILES")) return 1;
    std::vector<uint64_t> hist;                             // hist[W]: reads of W windows
    uint64_t best = total_windows;                          // every window on its own: one insertion each
    for (uint64_t r = 0; r < n_reads; ++r) {
        const uint32_t W = len[r] - k + 1;
        if (W >= hist.size()) hist.resize(W + 1, 0);
        hist[W] += 1;
    }
    uint32_t span = 1;
    for (uint32_t sp = 2; sp <= TILE_SPAN_MAX && k + sp - 1 <= 95; ++sp) {
        uint64_t cost = 0;
        for (size_t W = 1; W < hist.size(); ++W) cost += hist[W] * tile_cost((uint32_t)W, sp);
        if (cost < best || (cost == best && span > 1)) { best = cost; span = sp; }
    }
    if (const char* e = getenv("KATOME_TILE_SPAN")) { const uint32_t sp = (uint32_t)atoi(e); if (sp >= 1 && k + sp - 1 <= 95) span = sp; }
    return span;
}

extern "C" {

uint32_t katome_tile_span_for_lengths(uint32_t k, const uint32_t* len, uint64_t n_reads) {
    uint64_t total = 0;
    for (uint64_t r = 0; r < n_reads; ++r) {
        if (len[r] < k) return 1;                         // (a read with no window: the builds refuse it; no plan)
        total += len[r] - k + 1;
    }
    return tile_span_for_lengths(k, len, n_reads, total);
}

int katome_dev_extract_tiles(katome_builder* b, const uint8_t* d_packed, uint64_t n_reads, uint32_t read_len, uint32_t span,
                             const uint8_t* d_skip, uint64_t* d_records, void* stream) {
    KCHECK_HIP(hipSetDevice(b->s.device));
    if (span < 1 || b->s.k + span - 1 > 95) { set_error("bad tile span %u", span); return KATOME_E_ARG; }
    KCHECK(check_seen_len(b, read_len));
    PhaseScope ps(b->prof, PH_EXTRACT, (hipStream_t)stream);
    b->seen_read_len = read_len;
    return launch_extract_fixed(b->s.k, b->rc, d_packed, n_reads, read_len, d_skip, d_records, (hipStream_t)stream, span,
                                b->first_seen && b->rc);
}

int katome_dev_extract_remainder(katome_builder* b, const uint8_t* d_packed, uint64_t n_reads, uint32_t read_len, uint32_t span,
                                 const uint8_t* d_skip, uint64_t* d_records, void* stream) {
    KCHECK_HIP(hipSetDevice(b->s.device));
    if (span < 1 || read_len < b->s.k) { set_error("bad tile span %u", span); return KATOME_E_ARG; }
    const uint32_t W = read_len - b->s.k + 1, first = (W / span) * span, rest = W - first;
    if (rest == 0) return KATOME_OK;
    KCHECK(check_seen_len(b, read_len));
    PhaseScope ps(b->prof, PH_EXTRACT, (hipStream_t)stream);
    b->seen_read_len = read_len;
    b->rem_pending = true; b->rem_win0 = first; b->rem_per_read = rest;
    return launch_extract_fixed(b->s.k, b->rc, d_packed, n_reads, read_len, d_skip, d_records, (hipStream_t)stream, 1,
                                b->first_seen && b->rc, first, rest);
}

static int extract_var_common(katome_builder* b, const uint8_t* d_packed, uint64_t packed_bytes, const uint64_t* d_byte_off,
                              const uint32_t* d_len, const uint64_t* d_rec_prefix, const uint64_t* d_win_prefix, uint64_t n_reads,
                              uint64_t n_records, uint64_t total_windows, uint32_t span, uint32_t mode, uint64_t* d_records, void* stream) {
    KCHECK_HIP(hipSetDevice(b->s.device));
    if (mode == 1 && (span < 2 || b->s.k + span - 1 > 95)) { set_error("bad tile span %u", span); return KATOME_E_ARG; }
    if (b->first_seen) {
        if (b->reads_inserted) { set_error("first-seen order: fixed- and variable-length batches cannot be mixed in one build"); return KATOME_E_UNSUPPORTED; }
        // the insert that follows reads these
        b->var_prefix = d_win_prefix; b->var_reads = n_reads; b->var_windows = total_windows;
        b->var_rec_prefix = d_rec_prefix; b->var_records = n_records; b->var_mode = mode; b->var_span = span;
    }
    PhaseScope ps(b->prof, PH_EXTRACT, (hipStream_t)stream);
    return launch_extract_var(b->s.k, b->rc, d_packed, packed_bytes, d_byte_off, d_len, d_rec_prefix, n_reads, n_records,
                              d_records, (hipStream_t)stream, b->first_seen && b->rc, span, mode);
}

int katome_dev_extract_var(katome_builder* b, const uint8_t* d_packed, uint64_t packed_bytes, const uint64_t* d_byte_off,
                           const uint32_t* d_len, const uint64_t* d_win_prefix, uint64_t n_reads, uint64_t total_windows,
                           uint64_t* d_records, void* stream) {
    return extract_var_common(b, d_packed, packed_bytes, d_byte_off, d_len, d_win_prefix, d_win_prefix, n_reads, total_windows,
                              total_windows, 1, 0, d_records, stream);
}
int katome_dev_extract_var_tiles(katome_builder* b, const uint8_t* d_packed, uint64_t packed_bytes, const uint64_t* d_byte_off,
                                 const uint32_t* d_len, const uint64_t* d_tile_prefix, const uint64_t* d_win_prefix, uint64_t n_reads,
                                 uint64_t total_tiles, uint64_t total_windows, uint32_t span, uint64_t* d_records, void* stream) {
    return extract_var_common(b, d_packed, packed_bytes, d_byte_off, d_len, d_tile_prefix, d_win_prefix, n_reads, total_tiles,
                              total_windows, span, 1, d_records, stream);
}
int katome_dev_extract_var_remainder(katome_builder* b, const uint8_t* d_packed, uint64_t packed_bytes, const uint64_t* d_byte_off,
                                     const uint32_t* d_len, const uint64_t* d_rest_prefix, const uint64_t* d_win_prefix, uint64_t n_reads,
                                     uint64_t total_rest, uint64_t total_windows, uint32_t span, uint64_t* d_records, void* stream) {
    if (span < 1) { set_error("bad tile span %u", span); return KATOME_E_ARG; }
    return extract_var_common(b, d_packed, packed_bytes, d_byte_off, d_len, d_rest_prefix, d_win_prefix, n_reads, total_rest,
                              total_windows, span, 2, d_records, stream);
}

int katome_dev_partition(int device, const uint64_t* d_records, const uint32_t* d_values, uint64_t n_records, uint32_t key_words,
                         uint32_t n_parts, uint64_t* d_out, uint32_t* d_values_out, uint64_t* h_counts, void* stream) {
    KCHECK(use_device(device));
    return dev_partition(d_records, d_values, n_records, key_words, n_parts, d_out, d_values_out, h_counts, (hipStream_t)stream);
}
int katome_dev_partition_core(int device, const uint64_t* d_records, const uint32_t* d_values, uint64_t n_records, uint32_t key_words,
                              uint32_t core_shift, uint32_t core_bases, uint32_t n_parts, uint64_t* d_out, uint32_t* d_values_out,
                              uint64_t* h_counts, void* stream) {
    KCHECK(use_device(device));
    if (core_bases == 0) { set_error("partition_core: core_bases must be > 0"); return KATOME_E_ARG; }
    return dev_partition(d_records, d_values, n_records, key_words, n_parts, d_out, d_values_out, h_counts, (hipStream_t)stream,
                         core_shift, core_bases);
}
uint32_t katome_key_owner(const uint64_t* key, uint32_t key_words, uint32_t core_shift, uint32_t core_bases, uint32_t n_parts) {
    if (key_words == 1) {
        Key<1> a; a.w[0] = key[0];
        return (uint32_t)(core_bases ? core_owner(a, core_shift, core_bases, n_parts) : whole_key_owner(a, n_parts));
    }
    if (key_words == 3) {
        Key<3> a; a.w[0] = key[0]; a.w[1] = key[1]; a.w[2] = key[2];
        return (uint32_t)(core_bases ? core_owner(a, core_shift, core_bases, n_parts) : whole_key_owner(a, n_parts));
    }
    Key<2> a; a.w[0] = key[0]; a.w[1] = key[1];
    return (uint32_t)(core_bases ? core_owner(a, core_shift, core_bases, n_parts) : whole_key_owner(a, n_parts));
}

}  // extern "C"

// Table capacity policy.  A chunk of records may only be handed to the insert kernel when even in the
// worst case (every record a new key) the table stays below MAX_LOAD, which bounds every probe sequence;
// the table is doubled when its real occupancy passes GROW_LOAD.  `room` returns how many records may go in now.
static constexpr double MAX_LOAD = 0.9, GROW_LOAD = 0.6;

static int table_budget(katome_builder* b, double frac, uint64_t* slots) {
    size_t free_b = 0, total_b = 0;
    KCHECK_HIP(hipMemGetInfo(&free_b, &total_b));
    free_b += dev_cached_bytes();           // cached blocks are handed back when an allocation needs them
    *slots = (uint64_t)(free_b * frac) / (b->nw == 1 ? 16 : 32);
    return KATOME_OK;
}

static int ensure_table(katome_builder* b, Table& table, bool& ready, uint32_t nw, uint64_t hint, uint64_t incoming,
                        uint64_t* room, hipStream_t stream) {
    if (!ready) {
        uint64_t want = hint ? hint : std::min<uint64_t>(incoming, 1ull << 28) * 2;
        want = std::max<uint64_t>(want, 1u << 16);
        uint64_t budget = 0;
        KCHECK(table_budget(b, 0.5, &budget));
        budget = budget * 16 / (nw == 1 ? 16 : 32) * (b->nw == 1 ? 1 : 2);     // table_budget counts b->nw-sized slots
        if (want > budget) want = budget;
        KCHECK(table_alloc(table, nw, want, stream));
        ready = true;
    }
    for (;;) {
        uint64_t occ = 0;
        KCHECK(table_occupied(table, &occ, stream));
        const uint64_t limit = (uint64_t)(MAX_LOAD * (double)table.cap);
        const uint64_t r = limit > occ ? limit - occ : 0;
        const bool crowded = (double)occ > GROW_LOAD * (double)table.cap;
        if (!crowded && r >= std::min<uint64_t>(incoming, 1u << 20)) { *room = r; return KATOME_OK; }
        uint64_t want = table.cap * 2, budget = 0;
        KCHECK(table_budget(b, 0.9, &budget));
        budget = budget * 16 / (nw == 1 ? 16 : 32) * (b->nw == 1 ? 1 : 2);
        if (want > budget) want = budget;
        if (want <= table.cap + table.cap / 8) {
            if (r > 0) { *room = r; return KATOME_OK; }      // cannot grow: run on, up to the hard limit
            set_error("k-mer table is full (%llu keys in %llu slots) and cannot grow in device memory",
                      (unsigned long long)occ, (unsigned long long)table.cap);
            return KATOME_E_OOM;
        }
        KCHECK(table_grow(table, want, stream));
    }
}
static int ensure_table(katome_builder* b, uint64_t incoming, uint64_t* room, hipStream_t stream) {
    return ensure_table(b, b->table, b->table_ready, b->nw, b->s.table_slots_hint, incoming, room, stream);
}

int builder_insert(katome_builder* b, Table& table, bool& ready, uint32_t nw, uint64_t hint, const uint64_t* d_records,
                   const uint32_t* d_weights, uint64_t n, SeenOrigin* origin, int phase, hipStream_t stream) {
    for (uint64_t done = 0; done < n;) {
        uint64_t room = 0;
        KCHECK(ensure_table(b, table, ready, nw, hint, n - done, &room, stream));
        const uint64_t m = std::min(n - done, room);
        PhaseScope ps(b->prof, phase, stream);
        if (origin) origin->rec0 = done;               // (idx / pairs of an explicit origin are indexed from the batch's start)
        KCHECK(table_insert(table, d_records + done * nw, d_weights ? d_weights + done : nullptr, m, stream, table.track_seen ? origin : nullptr));
        done += m;
    }
    return KATOME_OK;
}

// span of the mid tiles a big tile is broken into: the divisor of `span` in 2..8 closest to 6; 0 = expand directly
uint32_t mid_span(uint32_t span) {
    if (span <= 16 || getenv("KATOME_ONE_LEVEL_TILES")) return 0;
    if (const char* e = getenv("KATOME_MID_SPAN")) {         // experiments: any divisor of the span
        const uint32_t s = (uint32_t)atoi(e);
        if (s >= 2 && s < span && span % s == 0) return s;
    }
    static const uint32_t pref[] = {6, 5, 7, 4, 8, 9, 3, 2};       // (9 before 3: k = 40 at 150 bp, span 27 -- 103.5 against 106.3 ms per 50 M reads)
    for (uint32_t s : pref) if (span % s == 0) return s;
    return 0;
}

// walk `from` in slot ranges small enough that even if every sub-window of the range were a new key, `to` stays
// under its load limit (so it keeps the size its hint gave it); every tile adds its count to its n_sub sub-windows
static int expand_level(katome_builder* b, Table& from, Table& to, bool& to_ready, uint32_t to_nw, uint64_t to_hint,
                        uint32_t sub_len, uint32_t n_sub, uint32_t stride, int phase, hipStream_t stream) {
    for (uint64_t s0 = 0; s0 < from.cap;) {
        uint64_t room = 0;
        KCHECK(ensure_table(b, to, to_ready, to_nw, to_hint, (uint64_t)n_sub << 20, &room, stream));
        const uint64_t slots = std::max<uint64_t>(std::min<uint64_t>(from.cap - s0, room / n_sub), 1);
        PhaseScope ps(b->prof, phase, stream);
        KCHECK(table_expand_tiles(from, s0, s0 + slots, to, sub_len, n_sub, stride, b->rc, stream));
        s0 += slots;
    }
    return KATOME_OK;
}

// big tiles -> mid tiles (when the span is large); leaves the tiles that hold k-mers directly in `*last`
int expand_to_last_level(katome_builder* b, Table** last, uint32_t* last_span, hipStream_t stream) {
    if (b->tiles2_ready && b->tiles.cap == 0) { *last = &b->tiles2; *last_span = b->span2; return KATOME_OK; }      // (done before)
    uint64_t n_tiles = 0;
    KCHECK(table_occupied(b->tiles, &n_tiles, stream));
    b->stat_tiles = n_tiles; b->stat_tile_slots = b->tiles.cap;
    b->span2 = mid_span(b->span);
    *last = &b->tiles; *last_span = b->span;
    if (b->span2 && n_tiles) {
        const uint32_t kk2 = b->s.k + b->span2 - 1, n_sub = b->span / b->span2;
        // the mid-tile table is sized from what is known by now: n_tiles distinct tiles make at most n_tiles * n_sub mid
        // tiles (C3: 1.6 per tile); five slots per tile keep its load near 1/3 (78 -> 68 ms for this level at C3)
        const uint64_t mid_hint = std::max<uint64_t>(b->s.table_slots_hint / 4, std::min<uint64_t>(n_tiles * 5, n_tiles * n_sub * 2));
        KCHECK(expand_level(b, b->tiles, b->tiles2, b->tiles2_ready, (uint32_t)key_words_for_k(kk2), mid_hint,
                            kk2, n_sub, b->span2, PH_EXPAND_MID, stream));
        b->tiles.release();
        KCHECK(table_occupied(b->tiles2, &b->stat_tiles2, stream));
        b->stat_tile2_slots = b->tiles2.cap;
        *last = &b->tiles2; *last_span = b->span2;
    }
    return KATOME_OK;
}

void release_tile_tables(katome_builder* b) { b->tiles.release(); b->tiles2.release(); b->tiles_ready = false; b->tiles2_ready = false; }

// every distinct tile adds its count to its k-mers; afterwards the tile tables are released
int expand_tiles(katome_builder* b, hipStream_t stream) {
    if (b->tile_recs_n) KCHECK(flush_tile_recs(b, stream));
    if (b->rest_n) KCHECK(flush_rest(b, stream));
    if (!b->tiles_ready) return KATOME_OK;
    Table* last = nullptr; uint32_t last_span = 1;
    KCHECK(expand_to_last_level(b, &last, &last_span, stream));
    if (b->stat_tiles) {
        // Without a hint from the caller the k-mer table is sized from what is known by now: the distinct tiles of the last
        // level hold at most (their number x span) distinct k-mers (C3: 36 % of that).  Starting small and doubling eight
        // times re-inserted every k-mer once more on the way (C3: +40 ms).
        uint64_t hint = b->s.table_slots_hint;
        if (!hint) {
            const uint64_t last_tiles = b->span2 ? b->stat_tiles2 : b->stat_tiles;
            hint = std::max<uint64_t>(last_tiles * last_span, 1u << 16);
            if (b->table_ready && b->table.cap < hint) {          // (left-over windows went in first: one growth step instead of many)
                uint64_t budget = 0;
                KCHECK(table_budget(b, 0.9, &budget));
                const uint64_t want = std::min(hint, budget);
                if (want > b->table.cap + b->table.cap / 8) KCHECK(table_grow(b->table, want, stream));
            }
        }
        KCHECK(expand_level(b, *last, b->table, b->table_ready, b->nw, hint, b->s.k, last_span, 1, PH_EXPAND_TILES, stream));
    }
    release_tile_tables(b);
    return KATOME_OK;
}

// how many 8-bit region passes to run in front of an insert, from the table size (KATOME_REGION_PASSES overrides)
static int region_passes(uint64_t table_bytes) {
    (void)table_bytes;
    if (const char* e = getenv("KATOME_REGION_PASSES")) return std::max(0, std::min(2, atoi(e)));
    return 0;
}

// BFCounter input: one edge per kept line and strand, never merged (add_single_edge_bfc, pt_graph.rs:201-213, calls
// add_edge unconditionally).  d_fwd: the lines' k-mers as packed keys in line order, d_w their weights.  Leaves the
// builder with its sorted edge list, as katome_dev_edges would.
int bfc_set_edges(katome_builder* b, const uint64_t* d_fwd, const uint32_t* d_w, uint64_t n_lines, hipStream_t stream) {
    const uint64_t E = n_lines * (b->rc ? 2 : 1);
    const uint32_t nw = b->nw;
    if (b->edges_ready || b->table_ready || b->tiles_ready) { set_error("BFCounter input cannot be mixed with counted reads"); return KATOME_E_ARG; }
    b->drop_edge_heads();
    b->n_edges = E; b->direct_edges = E;
    KCHECK(b->edge_key.alloc((E + 1) * 8 * nw, stream));
    KCHECK(b->edge_weight.alloc((E + 1) * 4, stream));
    PhaseScope ps(b->prof, PH_SORT_EDGES, stream);
    if (b->first_seen) {
        if (E >= (1ull << 32)) { set_error("first-seen order: more than 2^32 edges on one GPU"); return KATOME_E_UNSUPPORTED; }
        DevBuf raw_w(stream), raw_seq(stream), idx(stream);
        KCHECK(raw_w.alloc((E + 1) * 4)); KCHECK(raw_seq.alloc((E + 1) * 8)); KCHECK(idx.alloc((E + 1) * 4));
        KCHECK(dev_bfc_edges(d_fwd, d_w, n_lines, b->s.k, b->rc, b->edge_key.as<u64>(), raw_w.as<u32>(), raw_seq.as<u64>(), stream));
        KCHECK(dev_iota(idx.as<u32>(), E, stream));
        KCHECK(dev_sort_bufs(b->edge_key, &idx, E, nw, 2 * b->s.k, stream));
        KCHECK(b->edge_seq.alloc((E + 1) * 8, stream));
        KCHECK(dev_gather_u64(raw_seq.as<u64>(), idx.as<u32>(), E, b->edge_seq.as<u64>(), stream));
        KCHECK(dev_gather_u32(raw_w.as<u32>(), idx.as<u32>(), E, b->edge_weight.as<u32>(), stream));
    } else {
        KCHECK(dev_bfc_edges(d_fwd, d_w, n_lines, b->s.k, b->rc, b->edge_key.as<u64>(), b->edge_weight.as<u32>(), nullptr, stream));
        KCHECK(dev_sort_bufs(b->edge_key, &b->edge_weight, E, nw, 2 * b->s.k, stream));   // stable: a k-mer's lines stay in file order
    }
    b->edges_ready = true;
    return KATOME_OK;
}

int sorted_count_mode() {
    static const int mode = env_int("KATOME_SORTED_COUNT", 1);
    return mode;
}
// is counting n records by sorting worth its extra launches?  (KATOME_SORTED_COUNT=2: however few -- tests)
bool sorting_pays(uint64_t n) { return n && (n >= (1ull << 22) || sorted_count_mode() == 2); }
// the most records a caller hands to the LDS counting route (2^16 hash groups of 32 sub-rounds of 2900 records)
bool lds_route_takes(uint64_t n) { return (n >> 21) <= 2900; }

// plain (weight-1 or weighted) records into the k-mer table, by packed key (no origin)
static int insert_plain(katome_builder* b, const uint64_t* d_records, const uint32_t* d_weights, uint64_t n_records, hipStream_t stream) {
    for (uint64_t done = 0; done < n_records;) {
        uint64_t room = 0;
        KCHECK(ensure_table(b, n_records - done, &room, stream));
        const uint64_t n = std::min(n_records - done, room);
        PhaseScope ps(b->prof, PH_INSERT, stream);
        KCHECK(table_insert(b->table, d_records + done * b->nw, d_weights ? d_weights + done : nullptr, n, stream, nullptr));
        done += n;
    }
    return KATOME_OK;
}

// First-seen order, reads of varying length: the levels counted by sorting, the batches' records kept aside with delta tags
// (seen_tag.h).  KATOME_SEEN_VAR_SORTED=1 switches it on; off, such a build counts every level in the tables
static bool seen_var_sorted() { static const bool on = env_flag("KATOME_SEEN_VAR_SORTED", false); return on; }
// how the builder's tagged records spell their two numbers
static SeenTag builder_tag(const katome_builder* b) {
    return b->seen_delta ? SeenTag::by_delta() : SeenTag::fixed(2ull * (b->seen_read_len - b->s.k + 1));
}

// how many valid records wait in b->rest_k (the device cursor; b->rest_n counts what was handed over, skipped reads included)
static int rest_valid(katome_builder* b, uint64_t* n, hipStream_t stream) {
    *n = 0;
    if (!b->rest_n || !b->rest_count.p) return KATOME_OK;
    KCHECK_HIP(hipMemcpyAsync(n, b->rest_count.p, 8, hipMemcpyDeviceToHost, stream));
    KCHECK_HIP(hipStreamSynchronize(stream));
    return KATOME_OK;
}
static void rest_reset(katome_builder* b) { b->rest_k.release(); b->rest_count.release(); b->rest_n = b->rest_cap = 0; }

int flush_rest(katome_builder* b, hipStream_t stream) {
    uint64_t n_valid = 0;
    KCHECK(rest_valid(b, &n_valid, stream));
    if (n_valid && b->first_seen) {            // tagged records: back into keys + their two sequence numbers for the table
        DevBuf keys(stream), pairs(stream);
        KCHECK(keys.alloc(n_valid * 8 * b->nw + 16)); KCHECK(pairs.alloc(n_valid * 16 + 16));
        KCHECK(table_tagged_to_pairs(b->rest_k.as<u64>(), n_valid, b->nw, builder_tag(b), keys.as<u64>(), pairs.as<u64>(), stream));
        SeenOrigin origin;
        origin.pairs = pairs.as<u64>(); origin.rc = b->rc;
        KCHECK(builder_insert(b, b->table, b->table_ready, b->nw, b->s.table_slots_hint, keys.as<u64>(), nullptr, n_valid, &origin, PH_INSERT, stream));
    } else if (n_valid) {
        KCHECK(insert_plain(b, b->rest_k.as<u64>(), nullptr, n_valid, stream));
    }
    rest_reset(b);
    b->rest_closed = true;
    return KATOME_OK;
}

// KATOME_SORTED_FAIL=mid|last: that level's counting by sorting reports a group too large -- tests of the way back into the tables
bool sorted_fail(const char* level) {
    static const char* at = getenv("KATOME_SORTED_FAIL");
    return at && !strcmp(at, level);
}
// KATOME_SORTED_TILES: 2 (default) both tile levels are counted by sorting -- the big tiles' records are kept aside batch by batch
// (two-word tiles of one-word k-mers, either numbering; anything else takes the table) --, 1 the big tiles in their table and only
// the mid tiles by sorting, out of that table; 0 both tile levels in tables.  C3 by packed key: 200 / 210 / 239 ms per build.
int sorted_tiles_mode() {
    static const int mode = env_int("KATOME_SORTED_TILES", 2);
    return mode;
}

// Tile / k-mer shapes whose levels are all counted by sorting: tiles of two or three words (32..95 bases) over k-mers of one or two
// (round 4: three-word tiles -- every k from 32 to 63 at 150 bp, the reference's example k = 40 and BASELINE's k = 63 -- and two-word
// tiles of two-word k-mers); in the reference's numbering two-word tiles of one-word k-mers (the tagged kernels' shapes).
// KATOME_SORTED_WIDE=0: the round-3 rule (A/B against the tables).
bool tile_recs_shape(uint32_t nwt, uint32_t nw, bool first_seen) {
    static const bool wide = env_flag("KATOME_SORTED_WIDE", true);
    if (first_seen || !wide) return nwt == 2 && nw == 1;
    return (nwt == 2 || nwt == 3) && nw <= 2 && nw <= nwt;
}

// the tile records kept aside (builder.h) go into the tile table after all: another consumer wants the table, or the sorted
// counting of the tiles gave up
int tile_recs_valid(katome_builder* b, uint64_t* n, hipStream_t stream) {
    *n = 0;
    if (b->tile_recs_exact) { *n = b->tile_recs_n; return KATOME_OK; }       // (every record kept so far was valid: nothing to ask the device)
    if (!b->tile_recs_n || !b->tile_recs_count.p) return KATOME_OK;
    KCHECK_HIP(hipMemcpyAsync(n, b->tile_recs_count.p, 8, hipMemcpyDeviceToHost, stream));
    KCHECK_HIP(hipStreamSynchronize(stream));
    return KATOME_OK;
}
// no tile records are kept from here on (they were counted, or went into the tile table)
static void close_tile_recs(katome_builder* b) {
    b->tile_recs.release(); b->tile_recs_count.release(); b->tile_recs_n = b->tile_recs_cap = 0;
    b->tile_recs_hist.release(); b->tile_recs_hist_ok = false;
    b->tile_recs_exact = false; b->tile_recs_closed = true;
}
int flush_tile_recs(katome_builder* b, hipStream_t stream) {
    if (b->tile_recs_n) {
        const uint32_t nwt = (uint32_t)key_words_for_k(b->s.k + b->span - 1);
        uint64_t n = 0;
        KCHECK(tile_recs_valid(b, &n, stream));
        b->tile_recs_n = 0;
        if (b->first_seen && n) {            // tagged records: back into keys + their two sequence numbers for the table
            DevBuf keys(stream), pairs(stream);
            KCHECK(keys.alloc(n * 8 * nwt + 16)); KCHECK(pairs.alloc(n * 16 + 16));
            KCHECK(table_tagged_to_pairs(b->tile_recs.as<u64>(), n, nwt, builder_tag(b), keys.as<u64>(), pairs.as<u64>(), stream));
            b->tile_recs.release();
            SeenOrigin origin;
            origin.pairs = pairs.as<u64>(); origin.rc = b->rc;
            KCHECK(builder_insert(b, b->tiles, b->tiles_ready, nwt, b->s.table_slots_hint / 4, keys.as<u64>(), nullptr, n, &origin, PH_INSERT_TILES, stream));
        } else
        for (uint64_t done = 0; done < n;) {
            uint64_t room = 0;
            KCHECK(ensure_table(b, b->tiles, b->tiles_ready, nwt, b->s.table_slots_hint / 4, n - done, &room, stream));
            const uint64_t m = std::min(n - done, room);
            PhaseScope ps(b->prof, PH_INSERT_TILES, stream);
            KCHECK(table_insert(b->tiles, b->tile_recs.as<u64>() + done * nwt, nullptr, m, stream, nullptr));
            done += m;
        }
    }
    close_tile_recs(b);
    return KATOME_OK;
}

// room for n more tile records behind those kept aside; *ok = false: no room (or over the limit) -- what was kept has gone into the
// tile table and later batches follow it there
static int reserve_tile_recs(katome_builder* b, uint64_t n, uint32_t nwt, bool* ok, hipStream_t stream) {
    *ok = false;
    if (b->tile_recs_n + n > b->tile_recs_cap) {
        size_t free_b = 0, total_b = 0;
        KCHECK_HIP(hipMemGetInfo(&free_b, &total_b));
        uint64_t pool[3] = {0, 0, 0};
        dev_cache_stats(b->s.device, pool);
        free_b += pool[1];                         // (what the caching allocator holds idle is as good as free)
        // room for sixteen batches like this one to begin with (a build is a dozen batches), doubled when that was too little
        const uint64_t want = std::max<uint64_t>(b->tile_recs_cap ? b->tile_recs_cap * 2 : n * 16, b->tile_recs_n + n);
        // (the counting needs the records twice more -- the passes' scratch and the next level)
        // (KATOME_TILE_RECS_LIMIT: no more records than this are kept aside -- tests; by default a sixth of the card's memory)
        static const uint64_t limit = getenv("KATOME_TILE_RECS_LIMIT") ? strtoull(getenv("KATOME_TILE_RECS_LIMIT"), nullptr, 10) : ~0ull;
        if (b->tile_recs_n + n > limit || want * 8 * nwt * 3 > free_b + b->tile_recs_cap * 8 * nwt || want * 8 * nwt > total_b / 6) {
            KCHECK(flush_tile_recs(b, stream));
            return KATOME_OK;
        }
        DevBuf grown(stream);
        if (grown.alloc(want * 8 * nwt + 16) != KATOME_OK) {          // (no room after all: the table takes over)
            KCHECK(flush_tile_recs(b, stream));
            return KATOME_OK;
        }
        if (b->tile_recs_n) KCHECK_HIP(hipMemcpyAsync(grown.p, b->tile_recs.p, b->tile_recs_n * 8 * nwt, hipMemcpyDeviceToDevice, stream));
        const size_t grown_bytes = grown.bytes;
        b->tile_recs.adopt(grown.take(), grown_bytes);
        b->tile_recs.stream = stream;
        b->tile_recs_cap = want;
    }
    if (b->tile_recs_n == 0) b->tile_recs_exact = true;          // (nothing kept yet: the host knows the count until a batch with holes comes)
    *ok = true;
    return KATOME_OK;
}

// the device cursor of the tile records, ready for a kernel that appends behind it
static int tile_recs_cursor(katome_builder* b, hipStream_t stream) {
    if (!b->tile_recs_count.p) KCHECK(b->tile_recs_count.alloc(8, stream));
    if (b->tile_recs_exact) {
        // from here on only the device knows how many of the records handed over were valid: its cursor starts at what the host knew
        const uint64_t start = b->tile_recs_n;
        KCHECK_HIP(hipMemcpyAsync(b->tile_recs_count.p, &start, 8, hipMemcpyHostToDevice, stream));
        KCHECK_HIP(hipStreamSynchronize(stream));
        b->tile_recs_exact = false;
    }
    return KATOME_OK;
}

// a batch's tiles kept aside as records; *kept = false: they go into the tile table
int keep_tile_recs(katome_builder* b, const uint64_t* d_records, uint64_t n, uint32_t nwt, bool* kept, hipStream_t stream) {
    *kept = false;
    b->tile_recs_hist_ok = false;          // (records that nobody counted as they were written)
    bool ok = false;
    // (first-seen order: a record is kept with its tag -- read << 32 | number of its first window << 16 | of its reverse complement's)
    const uint32_t words = nwt + (b->first_seen ? 1 : 0);
    KCHECK(reserve_tile_recs(b, n, words, &ok, stream));
    if (!ok) return KATOME_OK;
    KCHECK(tile_recs_cursor(b, stream));
    if (b->first_seen) {
        const uint32_t W = b->seen_read_len - b->s.k + 1;
        KCHECK(table_keep_rest(d_records, n, nwt, true, b->reads_inserted, W / b->span, 0, 2 * W, b->tile_recs.as<u64>(), b->tile_recs_count.as<u64>(), stream,
                               b->span, b->span));
    } else
    KCHECK(table_keep_rest(d_records, n, nwt, false, 0, 1, 0, 0, b->tile_recs.as<u64>(), b->tile_recs_count.as<u64>(), stream));      // (the valid ones, behind the cursor)
    b->tile_recs_n += n;
    *kept = true;
    return KATOME_OK;
}

// Device memory a counting level may plan with: what the driver has free plus what the library's cache holds idle
// (KATOME_LEVEL_BUDGET: no more than this many bytes -- tests of the ways back into the tables at sizes the oracle can check)
static uint64_t level_budget() {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); return ~0ull; }
    const uint64_t avail = (uint64_t)free_b + dev_cached_bytes();
    const char* e = getenv("KATOME_LEVEL_BUDGET");
    return e ? std::min<uint64_t>(avail, strtoull(e, nullptr, 10)) : avail;
}
// a level counted by sorting holds its records, the partition passes' scratch of the same size and an output list sized for the case
// that no record repeats: three times the records (oriented edges: the output twice over)
static bool level_fits(uint64_t n_records, uint32_t key_words, bool oriented, const char* what) {
    const char* sl = getenv("KATOME_LEVEL_SLACK");           // (room left for everything else: group index, cursors, the allocator's rounding)
    const uint64_t slack = sl ? strtoull(sl, nullptr, 10) : (256ull << 20);
    // (+ a byte per record where the partition passes keep a digit stream -- records of two or three words -- and a byte per oriented
    // edge for S2's first digits)
    const uint64_t digits = (dev_digit_stream_pays(key_words) ? 1 : 0) + (oriented ? 1 : 0);
    const uint64_t pair = 8ull * key_words + 4, need = n_records * (pair * (oriented ? 4 : 3) + digits) + slack, have = level_budget();
    if (need <= have) return true;
    if (getenv("KATOME_LEVEL_TRACE"))
        fprintf(stderr, "[katome levels] %s: %llu records need %.1f GiB by sorting, %.1f GiB available -- this level and those below are counted in tables\n",
                what, (unsigned long long)n_records, need / 1073741824.0, have / 1073741824.0);
    return false;
}
// a list that was sized for its records and holds far fewer keys gives the room behind them back (thin coverage: the room is needed).
// The list already sits at the front of its block, so the block is trimmed where it lies (DevBuf::trim); KATOME_TRIM_IN_PLACE=0: the
// list moves into a buffer of its own size instead, as it did before the allocator could trim
static int shrink_to_fit(DevBuf& buf, size_t used, hipStream_t stream) {
    if (!buf.p || buf.bytes < (1ull << 30) || used * 2 > buf.bytes) return KATOME_OK;
    static const bool in_place = env_flag("KATOME_TRIM_IN_PLACE", true);
    if (in_place) {
        const size_t before = buf.bytes;
        if (buf.trim(used + 64) && getenv("KATOME_LC_TRACE"))
            fprintf(stderr, "[levels] list trimmed in place: %zu -> %zu bytes\n", before, buf.bytes);
        return KATOME_OK;
    }
    DevBuf small(stream);
    if (small.alloc(used + 64) != KATOME_OK) return KATOME_OK;          // (no room for the copy: the list stays where it is)
    if (used) KCHECK_HIP(hipMemcpyAsync(small.p, buf.p, used, hipMemcpyDeviceToDevice, stream));
    const size_t n = small.bytes;
    buf.adopt(small.take(), n);
    buf.stream = stream;
    return KATOME_OK;
}

// The k-mer level of an input whose tiles hardly repeat, when its records do not fit the card at once (thin coverage at hundreds of
// millions of reads): the last tile level's list is taken in P parts -- a part's tiles -> their k-mer records -> counted by sorting,
// strands not yet told apart, into a list of (canonical k-mer, count) --, and the parts' lists, put behind one another, ARE weighted
// k-mer records again: the caller counts them once more, as it would have counted the level's records, and has its edges.  A k-mer
// that several parts hold is counted 1 + 1/P times over instead of once; the alternative is the k-mer table at a third of the speed
// (profiles/r04_coverage_sweep.jsonl).  KATOME_E_UNSUPPORTED: not this way either (the caller goes on in tables; the list is untouched).
// KATOME_LEVEL_PARTS=0: never
static int kmer_records_in_parts(katome_builder* b, const uint64_t* lk, const uint32_t* lw, uint64_t n_last, uint32_t last_bases, uint32_t last_span,
                                 DevBuf& keys, DevBuf& weights, uint64_t* n_records, uint64_t extra_room, hipStream_t stream) {
    static const bool on = env_flag("KATOME_LEVEL_PARTS", true);
    if (!on) return KATOME_E_UNSUPPORTED;
    const uint32_t nw = b->nw, k = b->s.k, nwl = (uint32_t)key_words_for_k(last_bases);
    const uint64_t pair = 8ull * nw + 4, total = n_last * last_span, have = level_budget();
    const char* sl = getenv("KATOME_LEVEL_SLACK");
    const uint64_t slack = sl ? strtoull(sl, nullptr, 10) : (256ull << 20);
    // a part's records, the passes' scratch and its list (three times the records) in half of what is there; the other half holds the lists
    uint32_t P = 2;
    const uint64_t digits = dev_digit_stream_pays(nw) ? 1 : 0;          // (the passes' digit stream, where records of this width keep one)
    while (P <= 64 && (total / P + last_span) * (pair * 3 + digits) + slack > have / 2) P *= 2;
    if (P > 64 || n_last < P) return KATOME_E_UNSUPPORTED;
    if (getenv("KATOME_LEVEL_TRACE")) fprintf(stderr, "[katome levels] k-mers: counted in %u parts of %llu records\n", P, (unsigned long long)(total / P));
    PhaseScope ps(b->prof, PH_EXPAND_TILES, stream);
    std::unique_ptr<DevBuf[]> pk(new DevBuf[P]), pw(new DevBuf[P]);
    for (uint32_t p = 0; p < P; ++p) { pk[p].stream = stream; pw[p].stream = stream; }
    std::vector<uint64_t> pn(P, 0);
    uint64_t n_p = 0;
    for (uint32_t p = 0; p < P; ++p) {
        const uint64_t lo = n_last * p / P, hi = n_last * (p + 1) / P;
        if (hi == lo) continue;
        DevBuf rk(stream), rw(stream);
        uint64_t n_rec = 0, ne = 0, nd = 0;
        int rc = table_list_to_records(lk + lo * nwl, lw + lo, hi - lo, last_bases, k, last_span, 1, b->rc, rk, rw, &n_rec, stream, 0, nullptr);
        if (rc == KATOME_OK) rc = records_to_edges_sorted(rk, rw, n_rec, k, false, 0, pk[p], pw[p], &ne, &nd, stream);
        if (rc == KATOME_E_OOM || rc == KATOME_E_UNSUPPORTED) return KATOME_E_UNSUPPORTED;          // (less room than was planned with: the tables)
        if (rc != KATOME_OK) return rc;
        rk.release(); rw.release();
        KCHECK(shrink_to_fit(pk[p], ne * 8 * nw, stream)); KCHECK(shrink_to_fit(pw[p], ne * 4, stream));
        pn[p] = ne; n_p += ne;
    }
    if (!level_fits(n_p + extra_room, nw, b->rc, "k-mers (the parts' lists)")) return KATOME_E_UNSUPPORTED;
    if (keys.alloc((n_p + extra_room + 1) * 8 * nw, stream) != KATOME_OK || weights.alloc((n_p + extra_room + 1) * 4, stream) != KATOME_OK) {
        keys.release(); weights.release();
        return KATOME_E_UNSUPPORTED;
    }
    uint64_t at = 0;
    for (uint32_t p = 0; p < P; ++p) {
        if (!pn[p]) continue;
        KCHECK_HIP(hipMemcpyAsync(keys.as<u64>() + at * nw, pk[p].p, pn[p] * 8 * nw, hipMemcpyDeviceToDevice, stream));
        KCHECK_HIP(hipMemcpyAsync(weights.as<u32>() + at, pw[p].p, pn[p] * 4, hipMemcpyDeviceToDevice, stream));
        at += pn[p];
        pk[p].release(); pw[p].release();
    }
    *n_records = n_p;
    return KATOME_OK;
}

// The tile records kept aside -> the (k-mer, count) records of the last tile level, every level counted by sorting (DESIGN.md
// section 4): records -> two hash passes -> counted in LDS -> a compact list of distinct tiles with their counts; the next level's
// records are cut out of that list.  KATOME_OK: keys / weights hold *n_records records (room for extra_room more behind them) and
// the tile records are gone.  KATOME_E_UNSUPPORTED: a level could not be counted this way (or there is nothing to count) -- the
// tile records, or the distinct big tiles with their counts, are in the tile table instead and the caller goes on in tables.
int tile_recs_to_kmer_records(katome_builder* b, DevBuf& keys, DevBuf& weights, uint64_t* n_records, uint64_t extra_room, hipStream_t stream,
                              DevBuf* first_counts, bool rep, RecordSource* src) {
    *n_records = 0;
    const uint32_t k = b->s.k, span = b->span, tile_bases = k + span - 1, nwt = (uint32_t)key_words_for_k(tile_bases);
    b->span2 = mid_span(span);
    DevBuf t1k(stream), t1w(stream);
    uint64_t n1 = 0, d1 = 0;
    int rc;
    {
        PhaseScope ps(b->prof, PH_INSERT_TILES, stream);
        TileLevelScope tl;
        DevBuf ones(stream);          // (stays empty: records without weights count once each, and the passes move 16 bytes a record, not 20)
        uint64_t n = 0;
        KCHECK(tile_recs_valid(b, &n, stream));
        // (the whole array is ordered in this one call: the counts the extraction left, where they cover it, are its first pass's)
        u32* const first = b->tile_recs_hist_ok && n == b->tile_recs_n && nwt == 2 ? b->tile_recs_hist.as<u32>() : nullptr;
        rc = n ? records_to_edges_sorted(b->tile_recs, ones, n, tile_bases, false, 0, t1k, t1w, &n1, &d1, stream, nullptr, first)
               : KATOME_E_UNSUPPORTED;                          // (every read was skipped: nothing to count)
        b->tile_recs_hist_ok = false;                           // (the pass worked in them: prefixes now)
        if (rc != KATOME_OK && rc != KATOME_E_UNSUPPORTED) return rc;
    }
    if (rc == KATOME_E_UNSUPPORTED) {
        KCHECK(flush_tile_recs(b, stream));          // (the records are all still there, in another order: into the table with them)
        return KATOME_E_UNSUPPORTED;
    }
    close_tile_recs(b);
    b->stat_tiles = n1; b->stat_tile_slots = 0; b->stat_tiles2 = 0; b->stat_tile2_slots = 0;
    KCHECK(shrink_to_fit(t1k, n1 * 8 * nwt, stream)); KCHECK(shrink_to_fit(t1w, n1 * 4, stream));
    const uint64_t* lk = t1k.as<u64>(); const uint32_t* lw = t1w.as<u32>();
    uint64_t n_last = n1; uint32_t last_bases = tile_bases, last_span = span;
    DevBuf t2k(stream), t2w(stream);
    if (b->span2 && n1) {
        const uint32_t kk2 = k + b->span2 - 1, n_sub = span / b->span2;
        PhaseScope ps(b->prof, PH_EXPAND_MID, stream);
        TileLevelScope tl;
        DevBuf mk(stream), mw(stream);
        uint64_t n_mid = 0, n2 = 0, d2 = 0;
        DevBuf mid_counts(stream);        // (the first partition pass's digit counts per tile, made while the records are written)
        RecordSource mid_src;             // (... or instead of them: that pass then cuts the records out of the list, which stays until the level is counted)
        // (input whose tiles hardly repeat -- thin coverage -- multiplies records level by level: a level that would not fit the card
        // by sorting is counted in a table, which takes its upserts in slot ranges of any size)
        if (sorted_fail("mid") || !level_fits(n1 * n_sub, (uint32_t)key_words_for_k(kk2), false, "mid tiles")) rc = KATOME_E_UNSUPPORTED;
        else {
            KCHECK(table_list_to_records(lk, lw, n1, tile_bases, kk2, n_sub, b->span2, b->rc, mk, mw, &n_mid, stream, 0, &mid_counts, false, &mid_src));
            rc = records_to_edges_sorted(mk, mw, n_mid, kk2, false, 0, t2k, t2w, &n2, &d2, stream, nullptr, mid_counts.as<u32>(), nullptr, &mid_src);
        }
        if (rc != KATOME_OK && rc != KATOME_E_UNSUPPORTED) return rc;
        if (rc == KATOME_E_UNSUPPORTED) {
            // the mid tiles cannot be counted this way: the distinct big tiles go into the tile table with their counts, and the build
            // goes on from there as if they had been counted in it
            mk.release(); mw.release(); t2k.release(); t2w.release();
            KCHECK(builder_insert(b, b->tiles, b->tiles_ready, nwt, b->s.table_slots_hint / 4, t1k.as<u64>(), t1w.as<u32>(), n1, nullptr, PH_INSERT_TILES, stream));
            return KATOME_E_UNSUPPORTED;
        }
        b->stat_tiles2 = n2;
        t1k.release(); t1w.release();
        mk.release(); mw.release();
        KCHECK(shrink_to_fit(t2k, n2 * 8 * key_words_for_k(kk2), stream)); KCHECK(shrink_to_fit(t2w, n2 * 4, stream));
        lk = t2k.as<u64>(); lw = t2w.as<u32>(); n_last = n2; last_bases = kk2; last_span = b->span2;
    }
    if (n_last && !level_fits(n_last * last_span + extra_room, b->nw, b->rc, "k-mers")) {
        // in parts first (kmer_records_in_parts): their lists stand in for the level's records
        if (first_counts) first_counts->release();
        const int prc = kmer_records_in_parts(b, lk, lw, n_last, last_bases, last_span, keys, weights, n_records, extra_room, stream);
        if (prc == KATOME_OK && rep && b->rc) return table_orient_records(keys.as<u64>(), *n_records, k, true, stream);
        if (prc != KATOME_E_UNSUPPORTED) return prc;
        keys.release(); weights.release(); *n_records = 0;
        // the k-mer level would not fit by sorting: the distinct tiles of the last level go into their table with their counts (the mid
        // tiles into `tiles2`, with nothing in `tiles`: expand_to_last_level's "done before" state) and the k-mers are counted in theirs
        const uint32_t nwl = (uint32_t)key_words_for_k(last_bases);
        if (b->span2) {
            KCHECK(builder_insert(b, b->tiles2, b->tiles2_ready, nwl, std::max<uint64_t>(b->s.table_slots_hint / 4, n_last * 2), lk, lw, n_last, nullptr, PH_EXPAND_MID, stream));
            b->tiles_ready = true;                   // (with b->tiles empty)
            b->stat_tile2_slots = b->tiles2.cap;
        } else {
            KCHECK(builder_insert(b, b->tiles, b->tiles_ready, nwl, b->s.table_slots_hint / 4, lk, lw, n_last, nullptr, PH_INSERT_TILES, stream));
        }
        return KATOME_E_UNSUPPORTED;
    }
    PhaseScope ps(b->prof, PH_EXPAND_TILES, stream);
    // (first_counts: for a caller that orders exactly these records by the whole k-mer's hash next -- table_list_to_records)
    KCHECK(table_list_to_records(lk, lw, n_last, last_bases, k, last_span, 1, b->rc, keys, weights, n_records, stream, extra_room, first_counts, rep, src));
    if (src && src->pending) {
        // the list has to outlive the first pass, which these locals do not: the source takes it and gives it up right after that pass
        DevBuf& ok = b->span2 && t2k.p ? t2k : t1k; DevBuf& ow = b->span2 && t2w.p ? t2w : t1w;
        src->own_tiles.stream = src->own_counts.stream = stream;
        const size_t kbytes = ok.bytes, wbytes = ow.bytes;
        src->own_tiles.adopt(ok.take(), kbytes); src->own_counts.adopt(ow.take(), wbytes);
    }
    return KATOME_OK;
}

// The k-mer level counted in order (lds_count.hip, lds_count_ordered_kernel): half of the edges leave the count sorted, the edge sort takes
// only the reverse complements and one merge (half_sort_finish).  Where lds_count_packed_kernel would run: one-word k-mers of odd k
// (k >= 9: 16 key bits name the group) or one strand, default numbering, no owner split.  KATOME_EDGE_HALF_SORT=0: the full edge sort
static bool half_sort_route(const katome_builder* b) {
    static const bool on = env_flag("KATOME_EDGE_HALF_SORT", true);
    const uint32_t k = b->s.k;
    return on && b->nw == 1 && !b->first_seen && k >= 9 && ((k & 1) || !b->rc);
}

// room for n more left-over windows behind those kept aside, and their cursor; *ok = false: too many -- what was kept has gone into
// the table and these follow it there
static int reserve_rest(katome_builder* b, uint64_t n, bool* ok, hipStream_t stream) {
    *ok = false;
    const uint32_t words = b->nw + (b->first_seen ? 1 : 0);          // (first-seen order: tagged records)
    if (b->rest_n + n > b->rest_cap) {
        size_t free_b = 0, total_b = 0;
        KCHECK_HIP(hipMemGetInfo(&free_b, &total_b));
        const uint64_t want = std::max<uint64_t>(b->rest_n + n, b->rest_cap * 2);
        // (they are sorted with the tiles' k-mers later: past an eighth of the card they stop being a side matter)
        if ((want + b->rest_n) * 8 * words > free_b / 2 || want * 8 * words > total_b / 8) { KCHECK(flush_rest(b, stream)); return KATOME_OK; }
        DevBuf grown(stream);
        KCHECK(grown.alloc(want * 8 * words + 16));
        if (b->rest_n) KCHECK_HIP(hipMemcpyAsync(grown.p, b->rest_k.p, b->rest_n * 8 * words, hipMemcpyDeviceToDevice, stream));
        const size_t grown_bytes = grown.bytes;
        b->rest_k.adopt(grown.take(), grown_bytes);
        b->rest_k.stream = stream;
        b->rest_cap = want;
    }
    if (!b->rest_count.p) { KCHECK(b->rest_count.alloc(8, stream)); KCHECK_HIP(hipMemsetAsync(b->rest_count.p, 0, 8, stream)); }
    *ok = true;
    return KATOME_OK;
}

// keeps a batch's left-over windows aside (see builder.h); *kept = false: they have to go into the table
static int keep_rest(katome_builder* b, const uint64_t* d_records, uint64_t n, bool* kept, hipStream_t stream) {
    *kept = false;
    bool ok = false;
    KCHECK(reserve_rest(b, n, &ok, stream));
    if (!ok) return KATOME_OK;
    KCHECK(table_keep_rest(d_records, n, b->nw, b->first_seen, b->last_batch_read0, b->rem_per_read, b->rem_win0,
                           b->first_seen ? 2u * (b->seen_read_len - b->s.k + 1) : 0u, b->rest_k.as<u64>(), b->rest_count.as<u64>(), stream));
    b->rest_n += n;
    *kept = true;
    return KATOME_OK;
}

// ---- first-seen order, reads of varying length: a batch's records kept aside with delta tags (KATOME_SEEN_VAR_SORTED) ----------
// Does every read of the batch just extracted pack (seen_tag.h)?  No read of more than DELTA_MAX_WINDOWS windows -- |Q - P| < 2 W for
// every record cut from a read of W windows, and for the minima of a key --, and numbers below DELTA_P_LIMIT.
// Asked once per batch, not per insert (a batch's tiles and its left-over windows share one prefix): the answer is kept under the
// prefix's address AND the batch's sequence base.  The address alone would not do -- a caller may hand the next batch's prefix in at
// the same address --, the base tells batches apart because every batch holds a read, a read a window, and the base moves on by twice
// the batch's windows when the batch is closed.
static int var_batch_packs(katome_builder* b, bool* ok, hipStream_t stream) {
    if (b->var_checked != b->var_prefix || b->var_checked_base != b->var_seq_base) {
        uint64_t max_w = 0;
        KCHECK(table_max_windows(b->var_prefix, b->var_reads, &max_w, stream));
        b->var_checked = b->var_prefix; b->var_checked_base = b->var_seq_base;
        b->var_checked_ok = max_w <= DELTA_MAX_WINDOWS && b->var_seq_base + 2 * b->var_windows < DELTA_P_LIMIT;
    }
    *ok = b->var_checked_ok;
    return KATOME_OK;
}
// a batch that does not pack closes the route: what was kept goes into the tables with its pairs, and the build goes on there
static int close_seen_var(katome_builder* b, hipStream_t stream) {
    if (!b->tile_recs_closed) KCHECK(flush_tile_recs(b, stream));
    if (!b->rest_closed) KCHECK(flush_rest(b, stream));
    return KATOME_OK;
}
// the tiles of the last katome_dev_extract_var_tiles call behind the tile records kept so far; *kept = false: into the tile table
static int keep_var_tiles(katome_builder* b, const uint64_t* d_records, uint64_t n, uint32_t nwt, bool* kept, hipStream_t stream) {
    *kept = false;
    bool ok = false;
    KCHECK(var_batch_packs(b, &ok, stream));
    if (!ok) return close_seen_var(b, stream);
    b->tile_recs_hist_ok = false;
    KCHECK(reserve_tile_recs(b, n, nwt + 1, &ok, stream));
    if (!ok) return KATOME_OK;
    KCHECK(tile_recs_cursor(b, stream));
    KCHECK(table_keep_var_tagged(d_records, n, nwt, b->rc, b->var_prefix, b->var_rec_prefix, b->var_reads, 1, b->var_span, b->var_seq_base,
                                 b->tile_recs.as<u64>(), b->tile_recs_count.as<u64>(), stream));
    b->tile_recs_n += n;
    b->seen_delta = true;
    *kept = true;
    return KATOME_OK;
}
// ... and its windows (all of them, or those after the last whole tile) behind the left-over windows; *kept = false: into the k-mer table
static int keep_var_rest(katome_builder* b, const uint64_t* d_records, uint64_t n, bool* kept, hipStream_t stream) {
    *kept = false;
    bool ok = false;
    KCHECK(var_batch_packs(b, &ok, stream));
    if (!ok) return close_seen_var(b, stream);
    KCHECK(reserve_rest(b, n, &ok, stream));
    if (!ok) return KATOME_OK;
    KCHECK(table_keep_var_tagged(d_records, n, b->nw, b->rc, b->var_prefix, b->var_rec_prefix, b->var_reads, b->var_mode, b->var_span, b->var_seq_base,
                                 b->rest_k.as<u64>(), b->rest_count.as<u64>(), stream));
    b->rest_n += n;
    b->seen_delta = true;
    *kept = true;
    return KATOME_OK;
}

extern "C" {

int katome_dev_insert_weighted(katome_builder* b, const uint64_t* d_records, const uint32_t* d_weights, uint64_t n_records,
                               void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    KCHECK_HIP(hipSetDevice(b->s.device));
    if (b->edges_ready) { set_error("builder already finalized"); return KATOME_E_ARG; }
    if (n_records == 0) {
        if (b->first_seen && b->var_prefix && b->var_mode != 1 && b->var_records == 0) {   // a batch whose reads are all whole tiles
            b->var_seq_base += 2 * b->var_windows;
            b->var_prefix = b->var_rec_prefix = nullptr; b->var_reads = b->var_windows = 0;
        }
        return KATOME_OK;
    }
    if (!b->first_seen && !d_weights && (b->tiles_ready || b->tile_recs_n) && !b->table_ready && !b->rest_closed && b->nw <= 2 && sorted_count_mode()) {
        bool kept = false;
        KCHECK(keep_rest(b, d_records, n_records, &kept, stream));
        if (kept) return KATOME_OK;
    }
    // first-seen order, reads of one length: the windows after the batch's tiles wait as tagged records (slot_bits.h, seen_pack)
    if (b->first_seen && b->rem_pending && !d_weights && !b->var_prefix && !b->var_seq_base && (b->tiles_ready || b->tile_recs_n) && !b->table_ready && !b->rest_closed &&
        b->nw <= 2 && sorted_count_mode() && b->seen_read_len >= b->s.k && 2ull * (b->seen_read_len - b->s.k + 1) <= 0xFFFFu &&
        b->last_batch_read0 + b->last_batch_reads < (1ull << 32) && n_records == b->last_batch_reads * b->rem_per_read) {
        bool kept = false;
        KCHECK(keep_rest(b, d_records, n_records, &kept, stream));
        if (kept) { b->rem_pending = false; return KATOME_OK; }
    }
    // ... reads of varying length: the batch's windows -- all of them, or those after its tiles -- wait as delta-tagged records (seen_tag.h)
    if (b->first_seen && b->var_prefix && seen_var_sorted() && !d_weights && b->var_mode != 1 && n_records == b->var_records && !b->table_ready &&
        !b->rest_closed && !b->direct_edges && b->nw <= 2 && sorted_count_mode()) {
        bool kept = false;
        KCHECK(keep_var_rest(b, d_records, n_records, &kept, stream));
        if (kept) {
            b->var_seq_base += 2 * b->var_windows;          // the batch is complete, as below
            b->var_prefix = b->var_rec_prefix = nullptr; b->var_reads = b->var_windows = 0;
            b->rem_pending = false;
            return KATOME_OK;
        }
    }
    uint64_t room = 0;
    KCHECK(ensure_table(b, n_records, &room, stream));
    // Optional: order the batch by table region first (streaming radix passes over the hash prefix), so
    // that the insert kernel's working set stays cache-sized.  Off unless KATOME_REGION_PASSES says so:
    // measured on MI355X the insert kernel is bound by atomic throughput, not by where the slots live.
    const uint64_t* k_in = d_records; const uint32_t* w_in = d_weights;
    SeenOrigin origin;
    if (b->first_seen && b->var_prefix) {
        if (b->var_mode == 1 || n_records != b->var_records) { set_error("first-seen order: insert exactly the records the last katome_dev_extract_var* call produced"); return KATOME_E_ARG; }
        origin.win_prefix = b->var_prefix; origin.n_reads = b->var_reads; origin.seq_base = b->var_seq_base; origin.rc = b->rc;
        origin.rec_prefix = b->var_rec_prefix; origin.mode = b->var_mode; origin.span = b->var_span;
    } else if (b->first_seen) {
        if (b->var_seq_base) { set_error("first-seen order: fixed- and variable-length batches cannot be mixed in one build"); return KATOME_E_UNSUPPORTED; }
        if (b->seen_read_len < b->s.k) { set_error("first-seen order: extract the records with this builder first"); return KATOME_E_ARG; }
        origin.windows = b->seen_read_len - b->s.k + 1; origin.span = 1; origin.rc = b->rc;
        if (b->rem_pending) {           // the windows after the tiles of the batch that was just inserted
            origin.per_read = b->rem_per_read; origin.win0 = b->rem_win0; origin.read0 = b->last_batch_read0;
            if (n_records != b->last_batch_reads * origin.per_read) { set_error("first-seen order: insert the remainder of the batch whose tiles were inserted last"); return KATOME_E_ARG; }
        } else {
            origin.per_read = origin.windows; origin.read0 = b->reads_inserted;
            if (n_records % origin.per_read) { set_error("first-seen order: a batch must hold whole reads"); return KATOME_E_ARG; }
        }
    }
    const int passes = b->first_seen ? 0 : region_passes(b->table.cap * b->table.slot_bytes());
    if (passes > 0 && n_records >= (1u << 16)) {
        for (int i = 0; i < 2; ++i) {
            if ((i == 0 || passes > 1) && b->scratch_k[i].bytes < n_records * 8 * b->nw) KCHECK(b->scratch_k[i].alloc(n_records * 8 * b->nw, stream));
            if (d_weights && (i == 0 || passes > 1) && b->scratch_w[i].bytes < n_records * 4) KCHECK(b->scratch_w[i].alloc(n_records * 4, stream));
        }
        PhaseScope ps(b->prof, PH_REGION_ORDER, stream);
        KCHECK(dev_region_order(d_records, d_weights, n_records, b->nw, passes, b->scratch_k[0].as<u64>(), b->scratch_k[1].as<u64>(),
                                b->scratch_w[0].as<u32>(), b->scratch_w[1].as<u32>(), &k_in, &w_in, stream));
    }
    for (uint64_t done = 0; done < n_records;) {
        if (done) KCHECK(ensure_table(b, n_records - done, &room, stream));
        const uint64_t n = std::min(n_records - done, room);
        PhaseScope ps(b->prof, PH_INSERT, stream);
        origin.rec0 = done;
        KCHECK(table_insert(b->table, k_in + done * b->nw, w_in ? w_in + done : nullptr, n, stream, b->first_seen ? &origin : nullptr));
        done += n;
    }
    if (b->first_seen && origin.win_prefix) {
        b->var_seq_base += 2 * b->var_windows;          // the batch is complete: its reads' windows, both strands
        b->var_prefix = b->var_rec_prefix = nullptr; b->var_reads = b->var_windows = 0;
    } else if (b->first_seen && !b->rem_pending) {
        b->reads_inserted += n_records / origin.per_read;
    }
    b->rem_pending = false;
    return KATOME_OK;
}
int katome_dev_insert(katome_builder* b, const uint64_t* d_records, uint64_t n_records, void* stream) {
    return katome_dev_insert_weighted(b, d_records, nullptr, n_records, stream);
}

// may this builder keep a batch's tile records aside and count them by sorting at the end?
static bool keeps_tile_recs(const katome_builder* b, uint32_t nwt) {
    // (the reference's numbering, reads of varying length: the tiles of the last katome_dev_extract_var_tiles call, tagged with their
    // numbers themselves -- keep_var_tiles, which asks whether they pack.  One-word tiles too: short reads make short tiles)
    if (b->first_seen && (b->var_prefix || b->var_seq_base))
        return b->var_prefix && b->var_mode == 1 && seen_var_sorted() && !b->direct_edges && nwt <= 2 && b->nw == 1 && !b->tiles_ready && !b->table_ready &&
               !b->tile_recs_closed && sorted_count_mode() && sorted_tiles_mode() == 2;
    // (the reference's numbering: reads of one length whose numbers pack into a record word -- lds_count_seen_kernel's rule)
    const bool seen_ok = !b->first_seen || (!b->direct_edges && b->seen_read_len >= b->s.k &&
                                            2ull * (b->seen_read_len - b->s.k + 1) <= 0xFFFFull && (b->reads_inserted >> 31) == 0);
    return seen_ok && tile_recs_shape(nwt, b->nw, b->first_seen) && !b->tiles_ready && !b->table_ready && !b->tile_recs_closed && sorted_count_mode() &&
           sorted_tiles_mode() == 2;
}

// room in b->tile_recs_hist for the counts of n_total kept records (the record array's capacity; what is there is kept);
// false: no room -- the first pass counts for itself
static bool reserve_tile_hist(katome_builder* b, uint64_t n_total, uint32_t sort_tile, bool keep, hipStream_t stream) {
    const uint64_t need = ((n_total + sort_tile - 1) / sort_tile) * 256 * 4 + 16;
    if (need <= b->tile_recs_hist.bytes) return true;
    DevBuf grown(stream);
    if (grown.alloc(need) != KATOME_OK) return false;
    if (keep && b->tile_recs_hist.p &&
        hipMemcpyAsync(grown.p, b->tile_recs_hist.p, ((b->tile_recs_n + sort_tile - 1) / sort_tile) * 256 * 4, hipMemcpyDeviceToDevice, stream) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    const size_t grown_bytes = grown.bytes;
    b->tile_recs_hist.adopt(grown.take(), grown_bytes);
    b->tile_recs_hist.stream = stream;
    return true;
}

int katome_dev_count_tiles(katome_builder* b, const uint8_t* d_packed, uint64_t n_reads, uint32_t read_len, uint32_t span,
                           const uint8_t* d_skip, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!b || (!d_packed && n_reads)) { set_error("null argument"); return KATOME_E_ARG; }
    KCHECK_HIP(hipSetDevice(b->s.device));
    if (b->edges_ready) { set_error("builder already finalized"); return KATOME_E_ARG; }
    if (read_len < b->s.k || span < 2 || b->s.k + span - 1 > 95) { set_error("bad tile span %u", span); return KATOME_E_ARG; }
    const uint32_t per_read = (read_len - b->s.k + 1) / span, nwt = (uint32_t)key_words_for_k(b->s.k + span - 1);
    const uint64_t n = n_reads * per_read;
    if (n == 0) return KATOME_OK;
    // No read skipped and every record kept so far valid: the records are made where they are kept -- no buffer in between, no copy
    // (C3: 12.8 GB not read and not written again per build).  Otherwise: into a scratch of the builder's, then as
    // katome_dev_insert_tiles does.
    if (!d_skip && !b->first_seen && keeps_tile_recs(b, nwt) && (b->tile_recs_n == 0 || (b->tile_recs_exact && span == b->span))) {
        bool ok = false;
        {
            PhaseScope ps(b->prof, PH_INSERT_TILES, stream);
            KCHECK(reserve_tile_recs(b, n, nwt, &ok, stream));
        }
        if (ok && b->tile_recs_exact) {
            // The extraction knows the index of every record it writes, so where this batch starts on a sort-tile boundary of the kept
            // array -- and every batch before it did -- it also leaves the first partition pass's digit counts of the sort tiles it
            // fills (KATOME_FUSED_HIST=0: never; the pass counts for itself, as it does in every other case)
            const uint32_t sort_tile = dev_sort_tile_keys(nwt);
            u64* const dst = b->tile_recs.as<u64>() + b->tile_recs_n * nwt;
            const bool counted = fused_hist_on() && (b->tile_recs_n == 0 || b->tile_recs_hist_ok) && b->tile_recs_n % sort_tile == 0 &&
                                 extract_tile_counts_ok(b->s.k, read_len, span, sort_tile, d_packed, dst) &&
                                 reserve_tile_hist(b, std::max<uint64_t>(b->tile_recs_n + n, b->tile_recs_cap), sort_tile, b->tile_recs_n != 0, stream);
            if (getenv("KATOME_LC_TRACE"))
                fprintf(stderr, "[tiles] batch of %llu records at %llu: %s\n", (unsigned long long)n, (unsigned long long)b->tile_recs_n,
                        counted ? "first-pass counts from the extraction" : "no counts");
            if (counted) {
                KCHECK(check_seen_len(b, read_len));
                PhaseScope ps(b->prof, PH_EXTRACT, stream);
                b->seen_read_len = read_len;
                KCHECK(launch_extract_tiles_counted(b->s.k, b->rc, d_packed, n_reads, read_len, span, dst, b->tile_recs_hist.as<u32>() + (b->tile_recs_n / sort_tile) * 256,
                                                    sort_tile, stream));
            } else {
                KCHECK(katome_dev_extract_tiles(b, d_packed, n_reads, read_len, span, nullptr, dst, stream));
            }
            b->tile_recs_hist_ok = counted;
            b->span = span;
            b->tile_recs_n += n;
            return KATOME_OK;
        }
    }
    KCHECK(b->tile_scratch.alloc(n * 8 * nwt + 64, stream));
    KCHECK(katome_dev_extract_tiles(b, d_packed, n_reads, read_len, span, d_skip, b->tile_scratch.as<u64>(), stream));
    return katome_dev_insert_tiles(b, b->tile_scratch.as<u64>(), n, span, stream);
}

int katome_dev_insert_tiles(katome_builder* b, const uint64_t* d_records, uint64_t n_records, uint32_t span, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    KCHECK_HIP(hipSetDevice(b->s.device));
    if (b->edges_ready) { set_error("builder already finalized"); return KATOME_E_ARG; }
    if (span < 2 || b->s.k + span - 1 > 95 || ((b->tiles_ready || b->tile_recs_n) && span != b->span)) { set_error("bad tile span %u", span); return KATOME_E_ARG; }
    if (b->first_seen && b->var_prefix && b->s.k + span - 1 > 95) { set_error("variable-length reads: tiles of at most 95 bases"); return KATOME_E_ARG; }
    if (n_records == 0) return KATOME_OK;
    b->span = span;
    const uint32_t nwt = (uint32_t)key_words_for_k(b->s.k + span - 1);
    const bool var_tiles = b->first_seen && b->var_prefix != nullptr;
    if (var_tiles && b->var_span == span && n_records == b->var_records && keeps_tile_recs(b, nwt)) {
        bool kept = false;
        PhaseScope ps(b->prof, PH_INSERT_TILES, stream);
        KCHECK(keep_var_tiles(b, d_records, n_records, nwt, &kept, stream));
        if (kept) return KATOME_OK;          // (the insert of the batch's left-over windows closes it, as on the table route)
    } else if (!var_tiles && keeps_tile_recs(b, nwt)) {
        const uint32_t per_read = b->first_seen ? (b->seen_read_len - b->s.k + 1) / span : 1;
        if (b->first_seen && (per_read == 0 || n_records % per_read)) { set_error("first-seen order: a batch must hold whole reads"); return KATOME_E_ARG; }
        bool kept = false;
        PhaseScope ps(b->prof, PH_INSERT_TILES, stream);
        KCHECK(keep_tile_recs(b, d_records, n_records, nwt, &kept, stream));
        if (kept) {
            if (b->first_seen) {
                b->last_batch_read0 = b->reads_inserted; b->last_batch_reads = n_records / per_read;
                b->reads_inserted += n_records / per_read;
            }
            return KATOME_OK;
        }
    }
    SeenOrigin origin;
    if (var_tiles) {
        if (b->var_mode != 1 || b->var_span != span || n_records != b->var_records) { set_error("first-seen order: insert exactly the tiles katome_dev_extract_var_tiles produced"); return KATOME_E_ARG; }
        origin.win_prefix = b->var_prefix; origin.n_reads = b->var_reads; origin.seq_base = b->var_seq_base; origin.rc = b->rc;
        origin.rec_prefix = b->var_rec_prefix; origin.mode = 1; origin.span = span;
    } else if (b->first_seen) {
        if (b->var_seq_base) { set_error("first-seen order: fixed- and variable-length batches cannot be mixed in one build"); return KATOME_E_UNSUPPORTED; }
        if (b->seen_read_len < b->s.k) { set_error("first-seen order: extract the records with this builder first"); return KATOME_E_ARG; }
        origin.windows = b->seen_read_len - b->s.k + 1; origin.per_read = origin.windows / span; origin.span = span; origin.rc = b->rc;
        origin.read0 = b->reads_inserted;
        if (origin.per_read == 0 || n_records % origin.per_read) { set_error("first-seen order: a batch must hold whole reads"); return KATOME_E_ARG; }
    }
    for (uint64_t done = 0; done < n_records;) {
        uint64_t room = 0;
        KCHECK(ensure_table(b, b->tiles, b->tiles_ready, nwt, b->s.table_slots_hint / 4, n_records - done, &room, stream));
        const uint64_t n = std::min(n_records - done, room);
        PhaseScope ps(b->prof, PH_INSERT_TILES, stream);
        origin.rec0 = done;
        KCHECK(table_insert(b->tiles, d_records + done * nwt, nullptr, n, stream, b->first_seen ? &origin : nullptr));
        done += n;
    }
    if (b->first_seen && !var_tiles) {
        b->last_batch_read0 = b->reads_inserted; b->last_batch_reads = n_records / origin.per_read;
        b->reads_inserted += n_records / origin.per_read;
    }
    return KATOME_OK;
}

/* multi-GPU: the (k-mer, weight) records of this rank's tiles, to be routed to the k-mers' owners */
int katome_dev_expand_tiles(katome_builder* b, uint64_t** d_keys, uint32_t** d_weights, uint64_t* n_records, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    KCHECK_HIP(hipSetDevice(b->s.device));
    *n_records = 0; *d_keys = nullptr; *d_weights = nullptr;
    if (b->first_seen) { set_error("first-seen order is not available on the multi-GPU route"); return KATOME_E_UNSUPPORTED; }
    if (b->tile_recs_n) KCHECK(flush_tile_recs(b, stream));
    if (b->rest_n) KCHECK(flush_rest(b, stream));
    if (!b->tiles_ready) return KATOME_OK;
    Table* last = nullptr; uint32_t last_span = 1;
    KCHECK(expand_to_last_level(b, &last, &last_span, stream));
    {
        PhaseScope ps(b->prof, PH_EXPAND_TILES, stream);
        KCHECK(table_expand_tiles_to_records(*last, b->s.k, last_span, b->rc, b->scratch_k[0], b->scratch_w[0], n_records, stream));
    }
    release_tile_tables(b);
    *d_keys = b->scratch_k[0].as<u64>(); *d_weights = b->scratch_w[0].as<u32>();
    return KATOME_OK;
}

static int weak_edges_ordered(katome_builder* b, uint32_t threshold, hipStream_t stream) {
    PruneGraph g{&b->edge_src, &b->edge_dst, &b->edge_weight, &b->edge_key, &b->node_key, &b->edge_age, b->n_edges, b->n_nodes, b->nw};
    KCHECK(dev_remove_weak_edges_ordered(g, threshold, stream));
    b->n_edges = g.n_edges; b->n_nodes = g.n_nodes;
    return KATOME_OK;
}

int katome_dev_remove_weak_edges(katome_builder* b, uint32_t threshold, void* stream_) {
    if (!b) { set_error("null argument"); return KATOME_E_ARG; }
    hipStream_t stream = (hipStream_t)stream_;
    if (b->finalized && b->first_seen) {
        // on the finished graph, with petgraph's numbering (retain_edges / retain_nodes: descending swap_removes)
        KCHECK_HIP(hipSetDevice(b->s.device));
        KCHECK(weak_edges_ordered(b, threshold, stream));
        KCHECK(dev_labels(b->edge_key.as<u64>(), b->n_edges, b->s.k, b->edge_label.as<uint8_t>(), stream));
        KCHECK_HIP(hipStreamSynchronize(stream));
        return KATOME_OK;
    }
    if (b->edges_ready) { set_error("builder already finalized"); return KATOME_E_ARG; }
    b->prune_weight = threshold;
    return KATOME_OK;
}

int katome_dev_table_count(katome_builder* b, uint64_t* out, void* stream) {
    KCHECK_HIP(hipSetDevice(b->s.device));
    *out = 0;
    if (b->rest_n) KCHECK(flush_rest(b, (hipStream_t)stream));
    if (!b->table_ready) return KATOME_OK;
    return table_occupied(b->table, out, (hipStream_t)stream);
}

// The left-over windows kept aside (b->rest_k, `words` words each: nw, or nw + 1 for tagged records) behind the n_rec records in
// keys / weights, weight 1 each.  orient: the records are in their representative orientation (the half sort's k-mer records)
static int append_rest(katome_builder* b, DevBuf& keys, DevBuf& weights, uint64_t* n_rec, uint64_t n_rest, uint32_t words, bool orient, hipStream_t stream) {
    if (!n_rest) return KATOME_OK;
    KCHECK_HIP(hipMemcpyAsync(keys.as<u64>() + *n_rec * words, b->rest_k.p, n_rest * 8 * words, hipMemcpyDeviceToDevice, stream));
    KCHECK(dev_fill_u32(weights.as<u32>() + *n_rec, n_rest, 1u, stream));
    if (orient) KCHECK(table_orient_records(keys.as<u64>() + *n_rec * words, n_rest, b->s.k, true, stream));
    *n_rec += n_rest;
    return KATOME_OK;
}

// The last level counted by sorting instead of in a table (lds_count.hip, lds_count_kernel / lds_count_wide_kernel): k <= 63, by packed
// key, nothing in the k-mer table yet (left-over windows were kept aside).  With the tiles kept as records (katome_dev_insert_tiles)
// the tile levels above it are counted the same way: every level is "records -> two hash passes -> counted in LDS -> a compact list
// of distinct keys with their counts", the next level's records are cut out of that list (table.hip, list_to_records_kernel).
// on fallback: the tiles are in their table, or the k-mer records with their counts in b->table; n_edges == 0
static int edges_from_tile_recs(katome_builder* b, bool* counted, hipStream_t stream) {
    const uint32_t k = b->s.k;
    DevBuf rk(stream), rw(stream);
    uint64_t n_rec = 0, n_rest = 0, distinct = 0;
    KCHECK(rest_valid(b, &n_rest, stream));
    DevBuf first_counts(stream);
    const bool half = half_sort_route(b);
    HalfSort hs;
    RecordSource src;          // (the k-mer records may be left to their first partition pass: see RecordSource)
    int rc = tile_recs_to_kmer_records(b, rk, rw, &n_rec, n_rest, stream, &first_counts, half, &src);
    if (rc == KATOME_E_UNSUPPORTED) return KATOME_OK;          // (the tiles are in their table now, the table routes take it from there)
    if (rc != KATOME_OK) return rc;
    {
        PhaseScope ps(b->prof, PH_EXPAND_TILES, stream);
        KCHECK(append_rest(b, rk, rw, &n_rec, n_rest, b->nw, half && b->rc, stream));
        rest_reset(b);
        const bool fail = sorted_fail("last");
        if (fail) KCHECK(table_materialise_records(src));          // (the table wants the records)
        if (fail && half && b->rc) KCHECK(table_orient_records(rk.as<u64>(), n_rec, k, false, stream));     // (the table takes canonical k-mers)
        rc = fail ? KATOME_E_UNSUPPORTED
            : records_to_edges_sorted(rk, rw, n_rec, k, b->rc, b->prune_weight, b->edge_key, b->edge_weight, &b->n_edges, &distinct, stream, nullptr,
                                      n_rest ? nullptr : first_counts.as<u32>(), half ? &hs : nullptr, &src);
        if (rc != KATOME_OK && rc != KATOME_E_UNSUPPORTED) return rc;
    }
    if (rc != KATOME_OK) {
        // the k-mers cannot be counted this way (a hash group beyond the LDS route): their records, counts and all, go into the k-mer
        // table and the edges are read out of it
        b->n_edges = 0;
        return builder_insert(b, b->table, b->table_ready, b->nw, b->s.table_slots_hint, rk.as<u64>(), rw.as<u32>(), n_rec, nullptr, PH_INSERT, stream);
    }
    b->stat_kmers = distinct; b->stat_kmer_slots = 0;
    rk.release(); rw.release();
    first_counts.release();                  // (the order call worked in them: prefixes now, of no use to anyone)
    PhaseScope ps(b->prof, PH_SORT_EDGES, stream);
    if (hs.taken) {
        KCHECK(half_sort_finish(hs, b->edge_key, b->edge_weight, stream, &b->edge_heads));
        if (b->edge_heads.p) { b->edge_heads_key = b->edge_key.p; b->edge_heads_n = b->n_edges; }
    } else KCHECK(dev_sort_bufs(b->edge_key, &b->edge_weight, b->n_edges, b->nw, 2 * k, stream, true));
    *counted = true;
    return KATOME_OK;
}

// The k-mers counted by sorting when the big tiles are in their table (KATOME_SORTED_TILES=1, a build that could not keep them aside
// as records, or one that had to give them up half-way), the mid tiles too where they can be.
// on fallback: the tiles are in their table (the big ones still there if the mid tiles were counted by sorting), b->table is empty; n_edges == 0
static int edges_from_tile_table(katome_builder* b, bool* counted, hipStream_t stream) {
    if (!sorted_count_mode() || !b->tiles_ready || !b->tiles.cap || b->table_ready || b->nw > 2) return KATOME_OK;
    uint64_t n_tiles = 0;
    KCHECK(table_occupied(b->tiles, &n_tiles, stream));
    const uint64_t bound = n_tiles * b->span + b->rest_n;        // the k-mer records can be no more than this
    const uint32_t nwt = b->tiles.nw;
    const bool shapes = (b->nw == 1 && nwt <= 2) || (b->nw == 2 && (nwt == 2 || nwt == 3));      // (what tiles_to_records streams)
    if (!shapes || !sorting_pays(bound) || !lds_route_takes(bound)) return KATOME_OK;
    Table* last = nullptr; uint32_t last_span = 1;
    // The mid tiles are counted by sorting all the same: the big tiles' sub-tiles leave the tile table as records, two hash passes,
    // counted in LDS into a compact list of (mid tile, count), and the k-mer records are cut out of that list -- no mid-tile table,
    // no 7e8 128-bit upserts (C3: 45 -> 32 ms for the level).
    DevBuf t2k(stream), t2w(stream);
    uint64_t n_mid_list = 0;
    bool mid_sorted = false;
    const uint32_t sp2 = mid_span(b->span);
    if (sorted_tiles_mode() && nwt == 2 && b->nw == 1 && sp2 && !b->tiles2_ready && b->tiles.cap && n_tiles &&
        level_fits(n_tiles * (b->span / sp2), (uint32_t)key_words_for_k(b->s.k + sp2 - 1), false, "mid tiles (big tiles in their table)")) {
        const uint32_t kk2 = b->s.k + sp2 - 1, n_sub = b->span / sp2;
        PhaseScope ps(b->prof, PH_EXPAND_MID, stream);
        TileLevelScope tl;
        DevBuf mk(stream), mw(stream);
        uint64_t n_mid = 0, d2 = 0;
        KCHECK(table_expand_tiles_to_subtiles(b->tiles, kk2, n_sub, sp2, b->rc, mk, mw, &n_mid, stream, nullptr));
        int rc2 = (n_mid && !sorted_fail("mid")) ? records_to_edges_sorted(mk, mw, n_mid, kk2, false, 0, t2k, t2w, &n_mid_list, &d2, stream) : KATOME_E_UNSUPPORTED;
        if (rc2 != KATOME_OK && rc2 != KATOME_E_UNSUPPORTED) return rc2;
        if (rc2 == KATOME_OK) {
            mid_sorted = true;           // (the big-tile table stays until the k-mers are counted: the table route's way back)
            b->stat_tiles = n_tiles; b->stat_tile_slots = b->tiles.cap;
            b->span2 = sp2; b->stat_tiles2 = n_mid_list; b->stat_tile2_slots = 0;
            last_span = sp2;
        } else { t2k.release(); t2w.release(); }
    }
    if (!mid_sorted) KCHECK(expand_to_last_level(b, &last, &last_span, stream));
    if (!mid_sorted && !((b->nw == 1 && last->nw <= 2) || (b->nw == 2 && (last->nw == 2 || last->nw == 3)))) return KATOME_OK;
    uint64_t last_tiles = n_mid_list;          // (... and the records of the level fit the card with their scratch and their output)
    if (!mid_sorted) KCHECK(table_occupied(*last, &last_tiles, stream));
    if (!level_fits(last_tiles * last_span + b->rest_n, b->nw, b->rc, "k-mers (tiles in their table)")) return KATOME_OK;
    DevBuf rk(stream), rw(stream);
    uint64_t n_rec = 0, distinct = 0;
    int rc = KATOME_OK;
    {
        PhaseScope ps(b->prof, PH_EXPAND_TILES, stream);
        uint64_t n_rest = 0;
        KCHECK(rest_valid(b, &n_rest, stream));
        if (mid_sorted) {
            KCHECK(table_list_to_records(t2k.as<u64>(), t2w.as<u32>(), n_mid_list, b->s.k + sp2 - 1, b->s.k, sp2, 1, b->rc, rk, rw, &n_rec, stream, n_rest));
            t2k.release(); t2w.release();
        } else
        KCHECK(table_tiles_to_records_fast(*last, b->s.k, last_span, b->rc, rk, rw, &n_rec, stream, n_rest));
        KCHECK(append_rest(b, rk, rw, &n_rec, n_rest, b->nw, false, stream));
        rc = sorted_fail("last") ? KATOME_E_UNSUPPORTED
            : records_to_edges_sorted(rk, rw, n_rec, b->s.k, b->rc, b->prune_weight, b->edge_key, b->edge_weight, &b->n_edges, &distinct, stream);
        if (rc != KATOME_OK && rc != KATOME_E_UNSUPPORTED) return rc;
    }
    // (a group too large for the LDS route: the table counts, from the tiles that are still there)
    if (rc != KATOME_OK) { b->n_edges = 0; return KATOME_OK; }
    release_tile_tables(b);
    rest_reset(b);
    b->stat_kmers = distinct; b->stat_kmer_slots = 0;
    for (int i = 0; i < 2; ++i) { b->scratch_k[i].release(); b->scratch_w[i].release(); }
    rk.release(); rw.release();
    PhaseScope ps(b->prof, PH_SORT_EDGES, stream);
    KCHECK(dev_sort_bufs(b->edge_key, &b->edge_weight, b->n_edges, b->nw, 2 * b->s.k, stream, true));
    *counted = true;
    return KATOME_OK;
}

// edges_from_tile_recs for a first-seen-order build, with the tiles kept as TAGGED records (keep_tile_recs in such a build): every level's
// distinct keys leave with their counts and their two lowered numbers packed into a tag again (lds_count_seen_kernel, LIST), the
// next level's tagged records are cut out of that list (list_to_tagged_records_kernel: a sub-window's numbers are its tile's plus its
// place in it).
// on fallback: the tile records, or the distinct big tiles with their counts and numbers, are in the tile table; n_edges == 0
static int seen_edges_from_tile_recs(katome_builder* b, DevBuf& raw_seq, bool* counted, hipStream_t stream) {
    const uint32_t k = b->s.k, span = b->span, tile_bases = k + span - 1;
    const SeenTag tag = builder_tag(b);          // (reads of varying length: the delta tag)
    b->span2 = mid_span(span);
    uint64_t n = 0, n1 = 0, d1 = 0, distinct = 0;
    KCHECK(tile_recs_valid(b, &n, stream));
    DevBuf l1(stream), c1(stream);
    int rc = KATOME_E_UNSUPPORTED;
    if (n) {
        PhaseScope ps(b->prof, PH_INSERT_TILES, stream);
        TileLevelScope tl;
        DevBuf ones(stream);               // (stays empty: the records count once each)
        rc = tagged_records_sorted(b->tile_recs, ones, n, tile_bases, b->rc, tag, true, l1, c1, &n1, &d1, stream);
        if (rc != KATOME_OK && rc != KATOME_E_UNSUPPORTED) return rc;
    }
    if (rc == KATOME_E_UNSUPPORTED) return flush_tile_recs(b, stream);      // (the records are all still there, in another order: into the table with them)
    close_tile_recs(b);
    b->stat_tiles = n1; b->stat_tile_slots = 0; b->stat_tiles2 = 0; b->stat_tile2_slots = 0;
    const uint64_t* lk = l1.as<u64>(); const uint32_t* lw = c1.as<u32>();
    uint64_t n_last = n1; uint32_t last_bases = tile_bases, last_span = span;
    DevBuf l2(stream), c2(stream);
    if (b->span2 && n1) {
        const uint32_t kk2 = k + b->span2 - 1, n_sub = span / b->span2;
        PhaseScope ps(b->prof, PH_EXPAND_MID, stream);
        TileLevelScope tl;
        DevBuf mk(stream), mw(stream);
        uint64_t n_mid = 0, n2 = 0, d2 = 0;
        DevBuf mid_counts(stream);         // (the first partition pass's digit counts per tile, made while the records are written)
        KCHECK(table_list_to_tagged_records(lk, lw, n1, tile_bases, kk2, n_sub, b->span2, b->rc, mk, mw, &n_mid, stream, 0, &mid_counts, tag.delta));
        rc = sorted_fail("mid") ? KATOME_E_UNSUPPORTED
            : tagged_records_sorted(mk, mw, n_mid, kk2, b->rc, tag, true, l2, c2, &n2, &d2, stream, mid_counts.as<u32>());
        if (rc != KATOME_OK && rc != KATOME_E_UNSUPPORTED) return rc;
        if (rc == KATOME_OK) { b->stat_tiles2 = n2; lk = l2.as<u64>(); lw = c2.as<u32>(); n_last = n2; last_bases = kk2; last_span = b->span2; }
    }
    if (rc == KATOME_OK) {
        PhaseScope ps(b->prof, PH_EXPAND_TILES, stream);
        DevBuf kr(stream), kw(stream);
        uint64_t n_rec = 0, n_rest = 0;
        KCHECK(rest_valid(b, &n_rest, stream));
        DevBuf last_counts(stream);
        KCHECK(table_list_to_tagged_records(lk, lw, n_last, last_bases, k, last_span, 1, b->rc, kr, kw, &n_rec, stream, n_rest, &last_counts, tag.delta));
        l2.release(); c2.release();
        KCHECK(append_rest(b, kr, kw, &n_rec, n_rest, b->nw + 1, false, stream));
        rc = sorted_fail("last") ? KATOME_E_UNSUPPORTED
            : tagged_records_sorted(kr, kw, n_rec, k, b->rc, tag, false, b->edge_key, raw_seq, &b->n_edges, &distinct, stream, last_counts.as<u32>());
        if (rc != KATOME_OK && rc != KATOME_E_UNSUPPORTED) return rc;
    }
    if (rc == KATOME_OK) {
        l1.release(); c1.release();
        rest_reset(b);
        b->stat_kmers = distinct; b->stat_kmer_slots = 0;
        *counted = true;
        return KATOME_OK;
    }
    // a level below gave up: the distinct big tiles go into the tile table with their counts and their numbers, and the build goes on
    // from there as if they had been counted in it
    b->n_edges = 0;
    l2.release(); c2.release();
    const uint32_t nwt = (uint32_t)key_words_for_k(tile_bases);
    DevBuf keys(stream), pairs(stream);
    KCHECK(keys.alloc(n1 * 8 * nwt + 16)); KCHECK(pairs.alloc(n1 * 16 + 16));
    KCHECK(table_tagged_to_pairs(l1.as<u64>(), n1, nwt, tag, keys.as<u64>(), pairs.as<u64>(), stream));
    l1.release();
    SeenOrigin origin;
    origin.pairs = pairs.as<u64>(); origin.rc = b->rc;
    return builder_insert(b, b->tiles, b->tiles_ready, nwt, b->s.table_slots_hint / 4, keys.as<u64>(), c1.as<u32>(), n1, &origin, PH_INSERT_TILES, stream);
}

// The k-mers of a first-seen-order build counted by sorting out of the tile table (lds_count.hip, lds_count_seen_kernel): reads of one
// length whose windows are whole tiles, so that a record's two sequence numbers pack into one word -- or, KATOME_SEEN_VAR_SORTED, reads
// of varying length, whose tiles' pairs pack as they are (the delta tag); the left-over windows join as tagged records.
// on fallback: the tiles are in their table (mid tiles in b->tiles2 if it made them); n_edges == 0
static int seen_edges_from_tile_table(katome_builder* b, DevBuf& raw_seq, bool* counted, hipStream_t stream) {
    const bool var = b->var_seq_base || b->var_prefix;
    if (!sorted_count_mode() || !b->tiles_ready || b->table_ready || b->nw > 2 || b->direct_edges || (var ? !seen_var_sorted() : b->seen_read_len < b->s.k))
        return KATOME_OK;
    const SeenTag tag = var ? SeenTag::by_delta() : builder_tag(b);
    uint64_t n_tiles = 0;
    KCHECK(table_occupied(b->tiles, &n_tiles, stream));
    if (!sorting_pays(n_tiles * b->span)) return KATOME_OK;     // (the last level's own size is checked where its records are made)
    Table* last = nullptr; uint32_t last_span = 1;
    KCHECK(expand_to_last_level(b, &last, &last_span, stream));
    uint64_t distinct = 0;
    int rc = KATOME_OK;
    {
        PhaseScope ps(b->prof, PH_EXPAND_TILES, stream);
        uint64_t n_rest = 0;
        KCHECK(rest_valid(b, &n_rest, stream));
        rc = sorted_fail("last") && var ? KATOME_E_UNSUPPORTED
            : tiles_to_edges_sorted_seen(*last, b->s.k, last_span, b->rc, tag, b->edge_key, raw_seq, &b->n_edges,
                                         &distinct, stream, n_rest ? b->rest_k.as<u64>() : nullptr, n_rest);
        if (rc != KATOME_OK && rc != KATOME_E_UNSUPPORTED) return rc;
    }
    // (numbers that do not pack, or a group too large: the table counts, from the tiles that are still there)
    if (rc != KATOME_OK) { b->n_edges = 0; return KATOME_OK; }
    release_tile_tables(b);
    rest_reset(b);
    b->stat_kmers = distinct; b->stat_kmer_slots = 0;
    *counted = true;
    return KATOME_OK;
}

// ... and of one that kept windows only (KATOME_SEEN_VAR_SORTED: reads of varying length cut window by window, or none of them as long
// as a tile): the tagged records kept aside are the level's records.
// on fallback: they are still kept aside, in another order (the table route flushes them); n_edges == 0
static int seen_edges_from_rest(katome_builder* b, DevBuf& raw_seq, bool* counted, hipStream_t stream) {
    if (!b->seen_delta || !sorted_count_mode() || b->tiles_ready || b->table_ready || b->tile_recs_n || !b->rest_n || b->nw > 2) return KATOME_OK;
    uint64_t n_rest = 0, distinct = 0;
    KCHECK(rest_valid(b, &n_rest, stream));
    if (!sorting_pays(n_rest)) return KATOME_OK;
    PhaseScope ps(b->prof, PH_EXPAND_TILES, stream);
    DevBuf ones(stream);               // (stays empty: the records count once each)
    const int rc = sorted_fail("last") ? KATOME_E_UNSUPPORTED
        : tagged_records_sorted(b->rest_k, ones, n_rest, b->s.k, b->rc, SeenTag::by_delta(), false, b->edge_key, raw_seq, &b->n_edges, &distinct, stream);
    if (rc != KATOME_OK && rc != KATOME_E_UNSUPPORTED) return rc;
    if (rc != KATOME_OK) { b->n_edges = 0; return KATOME_OK; }
    rest_reset(b);
    b->stat_kmers = distinct; b->stat_kmer_slots = 0;
    *counted = true;
    return KATOME_OK;
}

// The table route: what is left in the tile tables adds its counts to the k-mer table, whose edges are emitted and sorted.  It is
// also the first-seen routes' sort tail: seen_counted -- their edges are in edge_key / raw_seq already, only the sort is left.
static int edges_from_table(katome_builder* b, bool seen_counted, DevBuf& raw_seq, hipStream_t stream) {
    DevBuf raw_w(stream);
    if (!seen_counted) {
        KCHECK(expand_tiles(b, stream));
        if (!b->table_ready) {                    // (nothing was counted: an empty edge list)
            KCHECK(b->edge_key.alloc(16, stream)); KCHECK(b->edge_weight.alloc(16, stream));
            return KATOME_OK;
        }
        KCHECK(table_occupied(b->table, &b->stat_kmers, stream));
        b->stat_kmer_slots = b->table.cap;
        PhaseScope ps(b->prof, PH_EMIT_EDGES, stream);
        // (first-seen order: the threshold is applied after the numbering, as the reference's retain passes do)
        if (b->first_seen) KCHECK(table_emit_edges(b->table, b->s.k, b->rc, 0, b->edge_key, raw_w, &b->n_edges, stream, &raw_seq));
        else KCHECK(table_emit_edges(b->table, b->s.k, b->rc, b->prune_weight, b->edge_key, b->edge_weight, &b->n_edges, stream));
    }
    for (int i = 0; i < 2; ++i) { b->scratch_k[i].release(); b->scratch_w[i].release(); }
    b->table.release();                       // the table is spent; its memory serves the sort
    b->table_ready = false;
    PhaseScope ps(b->prof, PH_SORT_EDGES, stream);
    if (!b->first_seen) return dev_sort_bufs(b->edge_key, &b->edge_weight, b->n_edges, b->nw, 2 * b->s.k, stream, true);
    // sort (key, position) and bring weight and sequence number along through the positions
    if (b->n_edges >= (1ull << 32)) { set_error("first-seen order: more than 2^32 edges on one GPU"); return KATOME_E_UNSUPPORTED; }
    DevBuf idx(stream);
    KCHECK(idx.alloc((b->n_edges + 1) * 4));
    KCHECK(dev_iota(idx.as<u32>(), b->n_edges, stream));
    KCHECK(dev_sort_bufs(b->edge_key, &idx, b->n_edges, b->nw, 2 * b->s.k, stream));
    KCHECK(b->edge_weight.alloc((b->n_edges + 1) * 4, stream));
    KCHECK(b->edge_seq.alloc((b->n_edges + 1) * 8, stream));
    return dev_gather_seq_weight(raw_seq.as<u64>(), idx.as<u32>(), b->n_edges, b->edge_seq.as<u64>(), b->edge_weight.as<u32>(), stream);
}

// The builder's sorted distinct edges: the counting routes are tried in turn, each leaving to the next what it could not count
int katome_dev_edges(katome_builder* b, uint64_t** d_edge_key, uint32_t** d_edge_weight, uint64_t* n_edges, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    KCHECK_HIP(hipSetDevice(b->s.device));
    if (!b->edges_ready) {
        b->n_edges = 0;
        b->drop_edge_heads();
        b->tile_scratch.release();
        // (tile records with k-mers in the table already, or too few of them to be worth sorting: into the tile table)
        if (b->tile_recs_n && (b->table_ready || !sorting_pays(b->tile_recs_n * b->span))) KCHECK(flush_tile_recs(b, stream));
        bool counted = false;
        DevBuf raw_seq(stream);                  // (first-seen order: the edges' sequence numbers and weights until the sort tail)
        if (!b->first_seen) {
            if (b->tile_recs_n) KCHECK(edges_from_tile_recs(b, &counted, stream));
            if (!counted) KCHECK(edges_from_tile_table(b, &counted, stream));
            if (!counted) KCHECK(edges_from_table(b, false, raw_seq, stream));
        } else {
            const char* route = "tile records";
            if (b->tile_recs_n) KCHECK(seen_edges_from_tile_recs(b, raw_seq, &counted, stream));
            if (!counted) { route = "tile table, k-mers by sorting"; KCHECK(seen_edges_from_tile_table(b, raw_seq, &counted, stream)); }
            if (!counted) { route = "windows kept aside"; KCHECK(seen_edges_from_rest(b, raw_seq, &counted, stream)); }
            if (b->var_seq_base && getenv("KATOME_LC_TRACE"))
                fprintf(stderr, "[first-seen order, reads of varying length] levels counted %s%s (KATOME_SEEN_VAR_SORTED=%d)\n", counted ? "by sorting: " : "in the tables",
                        counted ? route : "", (int)seen_var_sorted());
            KCHECK(edges_from_table(b, counted, raw_seq, stream));
        }
        b->edges_ready = true;
    }
    if (d_edge_key) *d_edge_key = b->edge_key.as<u64>();
    if (d_edge_weight) *d_edge_weight = b->edge_weight.as<u32>();
    if (n_edges) *n_edges = b->n_edges;
    return KATOME_OK;
}

// the finalized graph as the caller sees it: pointers into the builder's arrays as they stand
static void graph_view(const katome_builder* b, katome_dev_graph* out) {
    out->n_nodes = b->n_nodes; out->n_edges = b->n_edges;
    out->key_words = b->nw; out->label_stride = label_stride_for_k(b->s.k);
    out->d_edge_key = b->edge_key.as<u64>(); out->d_edge_weight = b->edge_weight.as<u32>();
    out->d_edge_src = b->edge_src.as<u64>(); out->d_edge_dst = b->edge_dst.as<u64>();
    out->d_edge_label = b->edge_label.as<uint8_t>(); out->d_node_key = b->node_key.as<u64>();
    out->d_edge_age = b->edge_age.p ? b->edge_age.as<u32>() : nullptr;
}

int katome_dev_finalize(katome_builder* b, katome_dev_graph* out, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (b && b->finalized) return out ? katome_dev_current_graph(b, out) : KATOME_OK;      // (also: a graph installed by katome_dist_gather)
    KCHECK(katome_dev_edges(b, nullptr, nullptr, nullptr, stream_));
    const uint64_t E = b->n_edges;
    const uint32_t k = b->s.k;
    // node set = every source and target (k-1)-mer (add_fasta_node, pt_graph.rs:142-154): read off the
    // sorted edge list (node_ids.hip, dev_node_ids)
    KCHECK(b->edge_src.alloc((E + 1) * 8, stream));
    KCHECK(b->edge_dst.alloc((E + 1) * 8, stream));
    DevBuf node_first(stream);                 // first-seen order: the nodes' first touches come out of the same merge
    uint64_t n_marked = 0;                     // ... and, for targets below this index, "this edge touches it first" as a mark in edge_dst
    const size_t label_bytes = (E + 1) * (size_t)label_stride_for_k(k) + 16;
    // default numbering: the edges stay where they are, so the pass that writes their source ids writes their labels too (node_ids.hip
    // src_write_kernel) and no kernel reads the keys again for them.  KATOME_LABELS_IN_IDS=0: dev_labels afterwards, as in first-seen
    // order, whose edges are renumbered first
    static const bool labels_in_ids = env_flag("KATOME_LABELS_IN_IDS", true);
    const bool labels_early = labels_in_ids && !b->first_seen && E;
    if (labels_early) KCHECK(b->edge_label.alloc(label_bytes, stream));
    {
        PhaseScope ps(b->prof, PH_NODE_SET, stream);
        const bool fs = b->first_seen && E && b->edge_seq.p;
        // (the merge's head counts, if they were made for exactly this edge list)
        const bool heads = b->edge_heads.p && b->edge_heads_key == b->edge_key.p && b->edge_heads_n == E;
        const int rc = dev_node_ids(b->edge_key.as<u64>(), E, k, b->node_key, b->edge_src.as<u64>(), b->edge_dst.as<u64>(), &b->n_nodes, stream,
                                    fs ? b->edge_seq.as<u64>() : nullptr, fs ? &node_first : nullptr, &n_marked, heads ? b->edge_heads.as<u32>() : nullptr,
                                    labels_early ? b->edge_label.as<uint8_t>() : nullptr);
        b->drop_edge_heads();
        if (rc != KATOME_OK) { b->edge_label.release(); return rc; }      // (a builder that is not finalized holds no labels)
    }
    if (b->first_seen && E) {
        // Re-number everything the way the reference's loop would have: edges by the sequence number of their first
        // insertion, nodes by the first insertion that touches them (source of a strand's first window: 2*seq;
        // target: 2*seq + 1).  petgraph hands out indices in exactly that order (pt_graph.rs:149,194).
        PhaseScope ps(b->prof, PH_FIRST_SEEN, stream);
        const uint64_t max_seq = b->direct_edges ? 2 * b->direct_edges + 2
                                 : b->var_seq_base ? 2 * b->var_seq_base + 2
                                                   : 2 * (b->reads_inserted + 1) * 2 * (uint64_t)(b->seen_read_len - k + 1) + 2;
        uint32_t bits = 1;
        while (bits < 64 && (max_seq >> bits)) ++bits;
        FirstSeenGraph g{&b->edge_key, &b->edge_weight, &b->edge_src, &b->edge_dst, &b->edge_seq, &b->node_key, E, b->n_nodes, b->nw, k};
        KCHECK(dev_first_seen_order(g, node_first, n_marked, bits, stream));
        if (b->prune_weight) KCHECK(weak_edges_ordered(b, b->prune_weight, stream));
    }
    if (!labels_early) {
        KCHECK(b->edge_label.alloc(label_bytes, stream));
        PhaseScope ps(b->prof, PH_LABELS, stream);
        KCHECK(dev_labels(b->edge_key.as<u64>(), b->n_edges, k, b->edge_label.as<uint8_t>(), stream));
    }
    KCHECK_HIP(hipStreamSynchronize(stream));
    b->finalized = true;
    if (out) graph_view(b, out);
    return KATOME_OK;
}

int katome_dev_remove_dead_paths(katome_builder* b, katome_dev_graph* out, katome_prune_stats* stats, void* stream_) {
    if (!b) { set_error("null argument"); return KATOME_E_ARG; }
    hipStream_t stream = (hipStream_t)stream_;
    KCHECK_HIP(hipSetDevice(b->s.device));
    if (!b->first_seen) { set_error("remove_dead_paths needs a KATOME_FLAG_FIRST_SEEN_ORDER builder"); return KATOME_E_ARG; }
    if (!b->finalized) { set_error("remove_dead_paths: call katome_dev_finalize first"); return KATOME_E_ARG; }
    const auto t0 = std::chrono::steady_clock::now();
    PruneGraph g{&b->edge_src, &b->edge_dst, &b->edge_weight, &b->edge_key, &b->node_key, &b->edge_age, b->n_edges, b->n_nodes, b->nw};
    g.parallel_edges = b->direct_edges != 0;
    katome_prune_stats st;
    {
        PhaseScope ps(b->prof, PH_DEAD_PATHS, stream);
        KCHECK(dev_remove_dead_paths(g, b->s.k, &st, stream));
        b->n_edges = g.n_edges; b->n_nodes = g.n_nodes;
        // the labels follow their edges: rewrite them from the keys (kmer_to_edge, compress.rs:231-233)
        KCHECK(dev_labels(b->edge_key.as<u64>(), b->n_edges, b->s.k, b->edge_label.as<uint8_t>(), stream));
    }
    KCHECK_HIP(hipStreamSynchronize(stream));
    st.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (stats) *stats = st;
    if (out) graph_view(b, out);
    return KATOME_OK;
}

int katome_dev_standardize_contigs(katome_builder* b, void* stream_) {
    if (!b) { set_error("null argument"); return KATOME_E_ARG; }
    hipStream_t stream = (hipStream_t)stream_;
    KCHECK_HIP(hipSetDevice(b->s.device));
    if (!b->finalized) { set_error("standardize_contigs: call katome_dev_finalize first"); return KATOME_E_ARG; }
    KCHECK(dev_standardize_contigs(b->edge_src.as<u64>(), b->edge_dst.as<u64>(), b->edge_weight.as<u32>(), b->n_edges, b->n_nodes, stream));
    KCHECK_HIP(hipStreamSynchronize(stream));
    return KATOME_OK;
}

int katome_dev_standardize_edges(katome_builder* b, uint64_t original_genome_length, uint32_t threshold, void* stream_) {
    if (!b) { set_error("null argument"); return KATOME_E_ARG; }
    hipStream_t stream = (hipStream_t)stream_;
    KCHECK_HIP(hipSetDevice(b->s.device));
    if (!b->finalized) { set_error("standardize_edges: call katome_dev_finalize first"); return KATOME_E_ARG; }
    KCHECK(dev_standardize_scale(b->edge_weight.as<u32>(), b->n_edges, original_genome_length, b->s.k, threshold, stream));
    KCHECK(weak_edges_ordered(b, 1, stream));          // "remove edges with weight 0" (standardizer.rs:68-69)
    KCHECK(dev_labels(b->edge_key.as<u64>(), b->n_edges, b->s.k, b->edge_label.as<uint8_t>(), stream));
    KCHECK_HIP(hipStreamSynchronize(stream));
    return KATOME_OK;
}

int katome_dev_shrink(katome_builder* b, katome_dev_contigs* out, void* stream_) {
    return katome_dev_shrink_mode(b, KATOME_SHRINK_AUTO, out, nullptr, stream_);
}
int katome_dev_shrink_mode(katome_builder* b, uint32_t mode, katome_dev_contigs* out, double* host_ms, void* stream_) {
    if (!b || !out) { set_error("null argument"); return KATOME_E_ARG; }
    hipStream_t stream = (hipStream_t)stream_;
    KCHECK_HIP(hipSetDevice(b->s.device));
    if (host_ms) *host_ms = 0;
    if (!b->finalized) { set_error("shrink: call katome_dev_finalize first"); return KATOME_E_ARG; }
    if (mode > KATOME_SHRINK_EXACT) { set_error("shrink: unknown mode %u", mode); return KATOME_E_ARG; }
    // (auto: a graph in the reference's numbering gets the reference's own result -- its numbering is what the stage after it reads)
    const bool exact = mode == KATOME_SHRINK_EXACT || (mode == KATOME_SHRINK_AUTO && b->first_seen);
    ShrinkInput in{b->edge_src.as<u64>(), b->edge_dst.as<u64>(), b->edge_weight.as<u32>(), b->edge_key.as<u64>(), b->node_key.as<u64>(),
                   b->n_edges, b->n_nodes, b->nw, b->s.k};
    {
        PhaseScope ps(b->prof, PH_SHRINK, stream);
        if (exact) KCHECK(dev_shrink_exact(in, b->edge_age.p ? b->edge_age.as<u32>() : nullptr, b->shrunk, host_ms, stream));
        else KCHECK(dev_shrink(in, b->shrunk, stream));
    }
    memset(out, 0, sizeof *out);
    out->n_nodes = b->shrunk.n_nodes; out->n_edges = b->shrunk.n_edges; out->label_bytes = b->shrunk.label_bytes;
    out->key_words = b->nw;
    out->d_edge_src = b->shrunk.edge_src.as<u64>(); out->d_edge_dst = b->shrunk.edge_dst.as<u64>();
    out->d_edge_weight = b->shrunk.edge_weight.as<u32>(); out->d_edge_kmers = b->shrunk.edge_kmers.as<u32>();
    out->d_edge_label_off = b->shrunk.edge_label_off.as<u64>(); out->d_edge_label = b->shrunk.edge_label.as<uint8_t>();
    out->d_node_key = b->shrunk.node_key.as<u64>();
    return KATOME_OK;
}

}  // extern "C"

static void assembly_view(const TextOutput& t, katome_dev_assembly* out) {
    memset(out, 0, sizeof *out);
    out->n_contigs = t.n_contigs; out->text_bytes = t.text_bytes; out->layout = t.layout;
    out->d_contig_off = t.contig_off.as<u64>(); out->d_contig_len = t.contig_len.as<u32>(); out->d_text = t.text.as<uint8_t>();
}
// (lengths: the contigs' bases as the walk knows them -- host_build.cpp's stats need no copy from the device)
int builder_collapse(katome_builder* b, uint32_t layout, katome_dev_assembly* out, katome_collapse_stats* stats, std::vector<uint64_t>* lengths,
                     hipStream_t stream) {
    KCHECK_HIP(hipSetDevice(b->s.device));
    if (!b->finalized) { set_error("collapse: call katome_dev_finalize first"); return KATOME_E_ARG; }
    ShrinkInput in{b->edge_src.as<u64>(), b->edge_dst.as<u64>(), b->edge_weight.as<u32>(), b->edge_key.as<u64>(), b->node_key.as<u64>(),
                   b->n_edges, b->n_nodes, b->nw, b->s.k};
    {
        PhaseScope ps(b->prof, PH_COLLAPSE, stream);
        KCHECK(dev_collapse(in, b->edge_age.p ? b->edge_age.as<u32>() : nullptr, b->collapse_shrunk, layout, b->assembly, stats, lengths, stream));
    }
    if (out) assembly_view(b->assembly, out);
    return KATOME_OK;
}

extern "C" {

int katome_dev_collapse(katome_builder* b, uint32_t layout, katome_dev_assembly* out, katome_collapse_stats* stats, void* stream_) {
    if (!b || !out) { set_error("null argument"); return KATOME_E_ARG; }
    return builder_collapse(b, layout, out, stats, nullptr, (hipStream_t)stream_);
}
int katome_dev_contigs_text(katome_builder* b, const katome_dev_contigs* c, uint32_t layout, katome_dev_assembly* out, void* stream_) {
    if (!b || !c || !out) { set_error("null argument"); return KATOME_E_ARG; }
    hipStream_t stream = (hipStream_t)stream_;
    KCHECK_HIP(hipSetDevice(b->s.device));
    if (c->n_edges != b->shrunk.n_edges || c->d_edge_label != b->shrunk.edge_label.as<uint8_t>() || c->d_edge_label_off != b->shrunk.edge_label_off.as<u64>()) {
        set_error("contigs_text: not the result of this builder's last katome_dev_shrink");
        return KATOME_E_ARG;
    }
    {
        PhaseScope ps(b->prof, PH_COLLAPSE, stream);
        KCHECK(dev_pieces_text(b->s.k, c->d_edge_label, c->d_edge_label_off, c->n_edges, nullptr, c->n_edges, layout, 0, b->unitig_text, stream));
    }
    assembly_view(b->unitig_text, out);
    return KATOME_OK;
}
int katome_dev_pieces_text(int device, uint32_t k, const uint8_t* d_label, const uint64_t* d_label_off, uint64_t n_labels, const uint32_t* d_pieces,
                           uint64_t n_pieces, uint32_t layout, uint64_t* d_contig_off, uint32_t* d_contig_len, uint64_t contig_cap, uint8_t* d_text,
                           uint64_t text_cap, uint64_t* n_contigs, uint64_t* text_bytes, void* stream_) {
    return katome_dev_pieces_text_numbered(device, k, d_label, d_label_off, n_labels, d_pieces, n_pieces, layout, 0, d_contig_off, d_contig_len, contig_cap,
                                           d_text, text_cap, n_contigs, text_bytes, stream_);
}
int katome_dev_pieces_text_numbered(int device, uint32_t k, const uint8_t* d_label, const uint64_t* d_label_off, uint64_t n_labels,
                                    const uint32_t* d_pieces, uint64_t n_pieces, uint32_t layout, uint64_t first_contig, uint64_t* d_contig_off,
                                    uint32_t* d_contig_len, uint64_t contig_cap, uint8_t* d_text, uint64_t text_cap, uint64_t* n_contigs,
                                    uint64_t* text_bytes, void* stream_) {
    KCHECK(use_device(device));
    KCHECK(check_k(k));
    if (!n_contigs || !text_bytes) { set_error("null argument"); return KATOME_E_ARG; }
    *n_contigs = *text_bytes = 0;
    hipStream_t stream = (hipStream_t)stream_;
    if ((uintptr_t)d_label & 3) { set_error("text: d_label must be 4-byte aligned (the kernel reads the aligned words around the bytes it needs)"); return KATOME_E_ARG; }
    if (!d_pieces && n_pieces && n_pieces != n_labels) { set_error("text: without pieces there is one per label"); return KATOME_E_ARG; }
    TextPlan plan;
    KCHECK(dev_text_plan(k, d_label, d_label_off, n_labels, d_pieces, n_pieces, layout, first_contig, plan, stream));
    *n_contigs = plan.n_contigs; *text_bytes = plan.text_bytes;
    if (!d_text || plan.text_bytes == 0) return KATOME_OK;
    if (!d_contig_off || !d_contig_len || contig_cap < plan.n_contigs || text_cap < (plan.text_bytes + 15) / 16 * 16 || ((uintptr_t)d_text & 15)) {
        set_error("text: %llu contigs and %llu bytes (rounded up to 16, 16-byte aligned) do not fit the caller's arrays", (unsigned long long)plan.n_contigs,
                  (unsigned long long)plan.text_bytes);
        return KATOME_E_ARG;
    }
    KCHECK(dev_text_write(k, d_label, d_label_off, d_pieces, n_pieces, layout, first_contig, plan, d_contig_off, d_contig_len, d_text, stream));
    KCHECK_HIP(hipStreamSynchronize(stream));
    return KATOME_OK;
}

int katome_dev_current_graph(katome_builder* b, katome_dev_graph* out) {
    if (!b || !out) { set_error("null argument"); return KATOME_E_ARG; }
    if (!b->finalized) { set_error("katome_dev_current_graph: call katome_dev_finalize first"); return KATOME_E_ARG; }
    graph_view(b, out);
    return KATOME_OK;
}

// Stats<CollectionStats>::stats (stats/collections.rs:137-168) and the weight spectrum of the finalized graph as it stands;
// nothing in the builder changes
int katome_dev_graph_stats(katome_builder* b, katome_stats* out, void* stream_) {
    if (!b || !out) { set_error("null argument"); return KATOME_E_ARG; }
    if (!b->finalized) { set_error("graph_stats: call katome_dev_finalize first"); return KATOME_E_ARG; }
    hipStream_t stream = (hipStream_t)stream_;
    KCHECK_HIP(hipSetDevice(b->s.device));
    PhaseScope ps(b->prof, PH_GRAPH_STATS, stream);
    return dev_graph_stats(b->edge_src.as<u64>(), b->edge_dst.as<u64>(), b->edge_weight.as<u32>(), b->n_edges, b->n_nodes, out, stream);
}
int katome_dev_weight_spectrum(katome_builder* b, uint64_t* bins, uint32_t n_bins, void* stream_) {
    if (!b) { set_error("null argument"); return KATOME_E_ARG; }
    KCHECK(check_spectrum_bins(bins, n_bins));
    if (!b->finalized) { set_error("weight_spectrum: call katome_dev_finalize first"); return KATOME_E_ARG; }
    hipStream_t stream = (hipStream_t)stream_;
    KCHECK_HIP(hipSetDevice(b->s.device));
    PhaseScope ps(b->prof, PH_WEIGHT_SPECTRUM, stream);
    return dev_weight_spectrum(b->edge_weight.as<u32>(), b->n_edges, bins, n_bins, stream);
}

int katome_builder_counts(katome_builder* b, uint64_t* out8) {
    if (!b || !out8) { set_error("null argument"); return KATOME_E_ARG; }
    out8[0] = b->stat_tiles; out8[1] = b->stat_tile_slots; out8[2] = b->stat_kmers; out8[3] = b->stat_kmer_slots;
    out8[4] = b->stat_tiles2; out8[5] = b->stat_tile2_slots; out8[6] = b->span; out8[7] = b->span2;
    return KATOME_OK;
}

int katome_builder_profile(katome_builder* b, int enable) {
    if (!b) { set_error("null argument"); return KATOME_E_ARG; }
    b->prof.on = enable != 0;
    b->prof.clear();
    return KATOME_OK;
}
uint32_t katome_phase_count(void) { return PH_COUNT; }
const char* katome_phase_name(uint32_t phase) { return phase < PH_COUNT ? PHASE_NAMES[phase] : ""; }
int katome_builder_profile_read_work(katome_builder* b, double* total_ms, uint64_t* launches, uint64_t* work) {
    if (!b || !total_ms || !launches) { set_error("null argument"); return KATOME_E_ARG; }
    KCHECK_HIP(hipSetDevice(b->s.device));
    KCHECK_HIP(hipDeviceSynchronize());
    for (int i = 0; i < PH_COUNT; ++i) { total_ms[i] = 0; launches[i] = 0; if (work) work[i] = 0; }
    for (auto& e : b->prof.evs) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, e.a, e.b) == hipSuccess) { total_ms[e.phase] += ms; launches[e.phase] += 1; if (work) work[e.phase] += e.work; }
    }
    b->prof.clear();
    return KATOME_OK;
}
int katome_builder_profile_read(katome_builder* b, double* total_ms, uint64_t* launches) {
    return katome_builder_profile_read_work(b, total_ms, launches, nullptr);
}

int katome_dev_release_cache(int device) {
    KCHECK(use_device(device));
    dev_release_cache(device);
    return KATOME_OK;
}

int katome_dev_cache_stats(int device, uint64_t out[3]) {
    if (!out) { set_error("null argument"); return KATOME_E_ARG; }
    dev_cache_stats(device, out);
    return KATOME_OK;
}

int katome_dev_sort(int device, uint64_t* d_keys, uint32_t* d_vals, uint64_t n, uint32_t key_words, uint32_t key_bits, void* stream) {
    KCHECK(use_device(device));
    return dev_sort(d_keys, d_vals, n, key_words, key_bits, (hipStream_t)stream);
}
int katome_dev_replay_edge_removals(int device, const uint32_t* d_pos, const uint32_t* d_mult, uint64_t u, uint64_t n_edges,
                                    uint32_t* d_victims, uint32_t* d_move_to, uint32_t* d_move_from, uint64_t* counts, void* stream_) {
    KCHECK(use_device(device));
    if (!counts || (u && (!d_pos || !d_mult || !d_victims || !d_move_to || !d_move_from))) { set_error("null argument"); return KATOME_E_ARG; }
    if (n_edges >= 0xFFFFFFFFull) { set_error("more than 2^32 edges"); return KATOME_E_UNSUPPORTED; }
    hipStream_t stream = (hipStream_t)stream_;
    ReplayScratch sc(stream);
    DevBuf victims(stream), to(stream), from(stream);
    uint64_t m = 0, left = n_edges, moves = 0, dups = 0;
    KCHECK(dev_replay_edges(d_pos, d_mult, u, n_edges, sc, victims, to, from, &m, &left, &moves, &dups, stream));
    if (m) KCHECK_HIP(hipMemcpyAsync(d_victims, victims.p, m * 4, hipMemcpyDeviceToDevice, stream));
    if (moves) {
        KCHECK_HIP(hipMemcpyAsync(d_move_to, to.p, moves * 4, hipMemcpyDeviceToDevice, stream));
        KCHECK_HIP(hipMemcpyAsync(d_move_from, from.p, moves * 4, hipMemcpyDeviceToDevice, stream));
    }
    KCHECK_HIP(hipStreamSynchronize(stream));
    counts[0] = m; counts[1] = moves; counts[2] = left; counts[3] = dups;
    return KATOME_OK;
}
int katome_dev_replay_node_removals(int device, const uint32_t* d_die, uint64_t m, uint64_t n_nodes, uint32_t* d_move_to, uint32_t* d_move_from,
                                    uint64_t* counts, void* stream_) {
    KCHECK(use_device(device));
    if (!counts || (m && (!d_die || !d_move_to || !d_move_from))) { set_error("null argument"); return KATOME_E_ARG; }
    if (n_nodes >= 0xFFFFFFFFull || m >= 0x7FFFFFFFull) { set_error("more than 2^32 nodes"); return KATOME_E_UNSUPPORTED; }
    hipStream_t stream = (hipStream_t)stream_;
    NodeReplayScratch sc(stream);
    DevBuf to(stream), from(stream);
    uint64_t moves = 0, left = n_nodes;
    int fell_back = 0;
    KCHECK(dev_replay_nodes(d_die, m, n_nodes, sc, to, from, &moves, &left, &fell_back, stream));
    if (moves) {
        KCHECK_HIP(hipMemcpyAsync(d_move_to, to.p, moves * 4, hipMemcpyDeviceToDevice, stream));
        KCHECK_HIP(hipMemcpyAsync(d_move_from, from.p, moves * 4, hipMemcpyDeviceToDevice, stream));
    }
    KCHECK_HIP(hipStreamSynchronize(stream));
    counts[0] = moves; counts[1] = left; counts[2] = (uint64_t)fell_back;
    return KATOME_OK;
}
// the same two replays on 64-bit positions (dist_prune.hip: a graph sharded over several GPUs may hold more than 2^32 edges);
// only the marked entries and the tail that disappears are touched, so n_edges / n_nodes may be far beyond any buffer here
int katome_dev_replay_edge_removals64(int device, const uint64_t* d_pos, const uint32_t* d_mult, uint64_t u, uint64_t n_edges,
                                      uint64_t* d_victims, uint64_t* d_move_to, uint64_t* d_move_from, uint64_t* counts, void* stream_) {
    KCHECK(use_device(device));
    if (!counts || (u && (!d_pos || !d_mult || !d_victims || !d_move_to || !d_move_from))) { set_error("null argument"); return KATOME_E_ARG; }
    hipStream_t stream = (hipStream_t)stream_;
    ReplayScratch sc(stream);
    DevBuf victims(stream), to(stream), from(stream);
    uint64_t m = 0, left = n_edges, moves = 0, dups = 0;
    KCHECK(dev_replay_edges64(d_pos, d_mult, u, n_edges, sc, victims, to, from, &m, &left, &moves, &dups, stream));
    if (m) KCHECK_HIP(hipMemcpyAsync(d_victims, victims.p, m * 8, hipMemcpyDeviceToDevice, stream));
    if (moves) {
        KCHECK_HIP(hipMemcpyAsync(d_move_to, to.p, moves * 8, hipMemcpyDeviceToDevice, stream));
        KCHECK_HIP(hipMemcpyAsync(d_move_from, from.p, moves * 8, hipMemcpyDeviceToDevice, stream));
    }
    KCHECK_HIP(hipStreamSynchronize(stream));
    counts[0] = m; counts[1] = moves; counts[2] = left; counts[3] = dups;
    return KATOME_OK;
}
int katome_dev_replay_node_removals64(int device, const uint64_t* d_die, uint64_t m, uint64_t n_nodes, uint64_t* d_move_to, uint64_t* d_move_from,
                                      uint64_t* counts, void* stream_) {
    KCHECK(use_device(device));
    if (!counts || (m && (!d_die || !d_move_to || !d_move_from))) { set_error("null argument"); return KATOME_E_ARG; }
    hipStream_t stream = (hipStream_t)stream_;
    NodeReplayScratch sc(stream);
    DevBuf to(stream), from(stream);
    uint64_t moves = 0, left = n_nodes;
    int fell_back = 0;
    KCHECK(dev_replay_nodes64(d_die, m, n_nodes, sc, to, from, &moves, &left, &fell_back, stream));
    if (moves) {
        KCHECK_HIP(hipMemcpyAsync(d_move_to, to.p, moves * 8, hipMemcpyDeviceToDevice, stream));
        KCHECK_HIP(hipMemcpyAsync(d_move_from, from.p, moves * 8, hipMemcpyDeviceToDevice, stream));
    }
    KCHECK_HIP(hipStreamSynchronize(stream));
    counts[0] = moves; counts[1] = left; counts[2] = (uint64_t)fell_back;
    return KATOME_OK;
}
int katome_dev_scan_counts(int device, const uint32_t* d_counts, uint64_t m, uint64_t* d_offs, void* stream) {
    KCHECK(use_device(device));
    if (!d_offs || (m && !d_counts)) { set_error("null argument"); return KATOME_E_ARG; }
    return dev_scan_counts(d_counts, m, d_offs, (hipStream_t)stream);
}
int katome_dev_list_first_pass(int device, const uint64_t* d_tiles, const uint32_t* d_counts, uint64_t n_tiles, uint32_t tile_bases, uint32_t k, uint32_t span,
                               uint32_t stride, int rc, int rep, int fused, uint64_t* d_keys, uint32_t* d_weights, uint32_t* d_digit_counts, void* stream) {
    KCHECK(use_device(device));
    if (n_tiles && (!d_tiles || !d_counts || !d_keys || !d_weights || !d_digit_counts)) { set_error("null argument"); return KATOME_E_ARG; }
    if (!span || tile_bases < k || (uint64_t)stride * (span - 1) + k > tile_bases || k < 9 || tile_bases > 64) { set_error("first pass off a list: the sub-windows do not lie in the tile"); return KATOME_E_ARG; }
    return dev_list_first_pass(d_tiles, d_counts, n_tiles, tile_bases, k, span, stride, rc != 0, rep != 0, fused != 0, d_keys, d_weights, d_digit_counts, (hipStream_t)stream);
}
int katome_dev_unique(int device, uint64_t* d_keys, uint64_t n, uint32_t key_words, uint64_t* n_out, void* stream) {
    KCHECK(use_device(device));
    if (key_words != 1 && key_words != 2) { set_error("key_words must be 1 or 2"); return KATOME_E_ARG; }
    return dev_unique(d_keys, n, key_words, n_out, (hipStream_t)stream);
}
int katome_dev_rank(int device, const uint64_t* d_sorted, uint64_t n_sorted, uint32_t key_words, uint32_t key_bits,
                    const uint64_t* d_queries, uint64_t n_queries, uint64_t* d_rank_out, void* stream) {
    KCHECK(use_device(device));
    if (key_words != 1 && key_words != 2) { set_error("key_words must be 1 or 2"); return KATOME_E_ARG; }
    return dev_rank(d_sorted, n_sorted, key_words, key_bits, d_queries, n_queries, d_rank_out, (hipStream_t)stream);
}
int katome_dev_node_ids(int device, const uint64_t* d_edge_key, uint64_t n_edges, uint32_t k, uint64_t* d_node_key,
                        uint64_t* d_edge_src, uint64_t* d_edge_dst, uint64_t* n_nodes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    KCHECK(use_device(device));
    KCHECK(check_k(k));
    DevBuf nodes(stream);
    KCHECK(dev_node_ids(d_edge_key, n_edges, k, nodes, d_edge_src, d_edge_dst, n_nodes, stream));
    if (*n_nodes) KCHECK_HIP(hipMemcpyAsync(d_node_key, nodes.p, *n_nodes * 8 * key_words_for_k(k), hipMemcpyDeviceToDevice, stream));
    return KATOME_OK;
}

int katome_dev_source_ids(int device, const uint64_t* d_edge_key, uint64_t n_edges, uint32_t k, uint64_t* d_node_key,
                          uint64_t* d_edge_src, uint64_t* n_sources, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    KCHECK(use_device(device));
    KCHECK(check_k(k));
    DevBuf nodes(stream);
    KCHECK(dev_source_ids(d_edge_key, n_edges, k, nodes, d_edge_src, n_sources, stream));
    if (*n_sources) KCHECK_HIP(hipMemcpyAsync(d_node_key, nodes.p, *n_sources * 8 * key_words_for_k(k), hipMemcpyDeviceToDevice, stream));
    return KATOME_OK;
}
int katome_dev_endpoints(int device, const uint64_t* d_edge_key, uint64_t n, uint32_t k, uint64_t* d_src_key, uint64_t* d_dst_key, void* stream) {
    KCHECK(use_device(device));
    KCHECK(check_k(k));
    return dev_endpoints(d_edge_key, n, k, d_src_key, d_dst_key, (hipStream_t)stream);
}
int katome_dev_labels(int device, const uint64_t* d_edge_key, uint64_t n, uint32_t k, uint8_t* d_label, void* stream) {
    KCHECK(use_device(device));
    KCHECK(check_k(k));
    return dev_labels(d_edge_key, n, k, d_label, (hipStream_t)stream);
}
int katome_dev_synth_reads(int device, uint64_t first_read, uint64_t n_reads, uint32_t read_len, uint64_t genome_len,
                           double err_rate, uint32_t n_inject_percent, uint8_t* d_packed, uint8_t* d_skip, void* stream) {
    KCHECK(use_device(device));
    return launch_synth(first_read, n_reads, read_len, genome_len, err_rate, n_inject_percent, d_packed, d_skip, (hipStream_t)stream);
}

}  // extern "C"
