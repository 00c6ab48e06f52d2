// api.hip -- the device half of the C ABI of include/katome_gpu.h (katome_dev_*: extraction, the table side, the insert entries,
// finalize and the stages after it): the build driver behind `Build::create` (reference src/katome/algorithms/builder.rs:42-54) and
// the PtGraph::create post-pass (collections/graphs/pt_graph.rs:333-345), composed from the kernels in extract.hip, table.hip,
// radix.hip, node_ids.hip and first_seen.hip.  The records kept aside between batches are kept_records.hip's, katome_dev_edges and its
// counting routes count_routes.hip's; the entries that take and return host memory are in host_build.cpp.  No CPU fallback: every
// entry that needs the device fails with KATOME_E_DEVICE when there is none.
#include <stdlib.h>

#include <algorithm>
#include <chrono>
#include <new>
#include <vector>

#include "builder.h"
#include "s2_regions.h"

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
    if (b->tile_recs.n) KCHECK(flush_tile_recs(b, stream));
    if (b->rest.n) KCHECK(flush_rest(b, stream));
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

// ---- first-seen order: where a batch's records sit in the read-ordered stream ---------------------------------------------------
// the batch of variable-length reads last extracted is complete: its reads' windows, both strands, have their numbers
static void close_var_batch(katome_builder* b) {
    b->var_seq_base += 2 * b->var_windows;
    b->var_prefix = b->var_rec_prefix = nullptr; b->var_reads = b->var_windows = 0;
}
// n_records records of the last katome_dev_extract_var* call; mode 1: they are inserted as its tiles of `span` windows, else as windows
static int var_origin(const katome_builder* b, uint64_t n_records, uint32_t mode, uint32_t span, SeenOrigin* origin) {
    if (mode == 1) {
        if (b->var_mode != 1 || b->var_span != span || n_records != b->var_records) { set_error("first-seen order: insert exactly the tiles katome_dev_extract_var_tiles produced"); return KATOME_E_ARG; }
    } else if (b->var_mode == 1 || n_records != b->var_records) { set_error("first-seen order: insert exactly the records the last katome_dev_extract_var* call produced"); return KATOME_E_ARG; }
    origin->win_prefix = b->var_prefix; origin->n_reads = b->var_reads; origin->seq_base = b->var_seq_base; origin->rc = b->rc;
    origin->rec_prefix = b->var_rec_prefix; origin->mode = b->var_mode; origin->span = b->var_span;
    return KATOME_OK;
}
// n_records records of reads of one length, cut in steps of `span` windows; remainder: they are the windows after the tiles of the
// batch that was just inserted
static int fixed_origin(const katome_builder* b, uint64_t n_records, uint32_t span, bool remainder, SeenOrigin* origin) {
    if (b->var_seq_base) { set_error("first-seen order: fixed- and variable-length batches cannot be mixed in one build"); return KATOME_E_UNSUPPORTED; }
    if (b->seen_read_len < b->s.k) { set_error("first-seen order: extract the records with this builder first"); return KATOME_E_ARG; }
    origin->windows = b->seen_read_len - b->s.k + 1; origin->span = span; origin->rc = b->rc;
    if (remainder) {
        origin->per_read = b->rem_per_read; origin->win0 = b->rem_win0; origin->read0 = b->last_batch_read0;
        if (n_records != b->last_batch_reads * origin->per_read) { set_error("first-seen order: insert the remainder of the batch whose tiles were inserted last"); return KATOME_E_ARG; }
    } else {
        origin->per_read = origin->windows / span; origin->read0 = b->reads_inserted;
        if (origin->per_read == 0 || n_records % origin->per_read) { set_error("first-seen order: a batch must hold whole reads"); return KATOME_E_ARG; }
    }
    return KATOME_OK;
}

// ---- may a batch's windows wait aside (katome_builder::rest) instead of going into the k-mer table? -----------------------------
// default numbering: the windows left over after a batch's tiles
static bool keeps_rest_plain(const katome_builder* b, const uint32_t* d_weights) {
    return !b->first_seen && !d_weights && (b->tiles_ready || b->tile_recs.n) && !b->table_ready && !b->rest.closed && b->nw <= 2 && sorted_count_mode();
}
// first-seen order, reads of one length: the windows after the batch's tiles wait as tagged records (slot_bits.h, seen_pack)
static bool keeps_rest_seen_fixed(const katome_builder* b, const uint32_t* d_weights, uint64_t n_records) {
    return b->first_seen && b->rem_pending && !d_weights && !b->var_prefix && !b->var_seq_base && (b->tiles_ready || b->tile_recs.n) && !b->table_ready && !b->rest.closed &&
           b->nw <= 2 && sorted_count_mode() && b->seen_read_len >= b->s.k && 2ull * (b->seen_read_len - b->s.k + 1) <= 0xFFFFu &&
           b->last_batch_read0 + b->last_batch_reads < (1ull << 32) && n_records == b->last_batch_reads * b->rem_per_read;
}
// ... reads of varying length: the batch's windows -- all of them, or those after its tiles -- wait as delta-tagged records (seen_tag.h)
static bool keeps_rest_seen_var(const katome_builder* b, const uint32_t* d_weights, uint64_t n_records) {
    return b->first_seen && b->var_prefix && seen_var_sorted() && !d_weights && b->var_mode != 1 && n_records == b->var_records && !b->table_ready &&
           !b->rest.closed && !b->direct_edges && b->nw <= 2 && sorted_count_mode();
}

extern "C" {

int katome_dev_insert_weighted(katome_builder* b, const uint64_t* d_records, const uint32_t* d_weights, uint64_t n_records,
                               void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    KCHECK_HIP(hipSetDevice(b->s.device));
    if (b->edges_ready) { set_error("builder already finalized"); return KATOME_E_ARG; }
    if (n_records == 0) {
        if (b->first_seen && b->var_prefix && b->var_mode != 1 && b->var_records == 0) close_var_batch(b);   // a batch whose reads are all whole tiles
        return KATOME_OK;
    }
    if (keeps_rest_plain(b, d_weights)) {
        bool kept = false;
        KCHECK(keep_rest(b, d_records, n_records, &kept, stream));
        if (kept) return KATOME_OK;
    }
    if (keeps_rest_seen_fixed(b, d_weights, n_records)) {
        bool kept = false;
        KCHECK(keep_rest(b, d_records, n_records, &kept, stream));
        if (kept) { b->rem_pending = false; return KATOME_OK; }
    }
    if (keeps_rest_seen_var(b, d_weights, n_records)) {
        bool kept = false;
        KCHECK(keep_var_rest(b, d_records, n_records, &kept, stream));
        if (kept) {
            close_var_batch(b);
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
    if (b->first_seen && b->var_prefix) KCHECK(var_origin(b, n_records, 0, 1, &origin));
    else if (b->first_seen) KCHECK(fixed_origin(b, n_records, 1, b->rem_pending, &origin));
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
        close_var_batch(b);
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
               !b->tile_recs.closed && sorted_count_mode() && sorted_tiles_mode() == 2;
    // (the reference's numbering: reads of one length whose numbers pack into a record word -- lds_count_seen_kernel's rule)
    const bool seen_ok = !b->first_seen || (!b->direct_edges && b->seen_read_len >= b->s.k &&
                                            2ull * (b->seen_read_len - b->s.k + 1) <= 0xFFFFull && (b->reads_inserted >> 31) == 0);
    return seen_ok && tile_recs_shape(nwt, b->nw, b->first_seen) && !b->tiles_ready && !b->table_ready && !b->tile_recs.closed && sorted_count_mode() &&
           sorted_tiles_mode() == 2;
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
    if (!d_skip && !b->first_seen && keeps_tile_recs(b, nwt) && (b->tile_recs.n == 0 || (b->tile_recs.exact && span == b->span))) {
        bool ok = false;
        {
            PhaseScope ps(b->prof, PH_INSERT_TILES, stream);
            KCHECK(b->tile_recs.reserve(b, n, nwt, &ok, stream));
        }
        if (ok && b->tile_recs.exact) {
            // The extraction knows the index of every record it writes, so where this batch starts on a sort-tile boundary of the kept
            // array -- and every batch before it did -- it also leaves the first partition pass's digit counts of the sort tiles it
            // fills (KATOME_FUSED_HIST=0: never; the pass counts for itself, as it does in every other case)
            const uint32_t sort_tile = dev_sort_tile_keys(nwt);
            u64* const dst = b->tile_recs.recs.as<u64>() + b->tile_recs.n * nwt;
            const bool counted = fused_hist_on() && (b->tile_recs.n == 0 || b->tile_recs_hist_ok) && b->tile_recs.n % sort_tile == 0 &&
                                 extract_tile_counts_ok(b->s.k, read_len, span, sort_tile, d_packed, dst) &&
                                 reserve_tile_hist(b, std::max<uint64_t>(b->tile_recs.n + n, b->tile_recs.cap), sort_tile, b->tile_recs.n != 0, stream);
            if (getenv("KATOME_LC_TRACE"))
                fprintf(stderr, "[tiles] batch of %llu records at %llu: %s\n", (unsigned long long)n, (unsigned long long)b->tile_recs.n,
                        counted ? "first-pass counts from the extraction" : "no counts");
            if (counted) {
                KCHECK(check_seen_len(b, read_len));
                PhaseScope ps(b->prof, PH_EXTRACT, stream);
                b->seen_read_len = read_len;
                KCHECK(launch_extract_tiles_counted(b->s.k, b->rc, d_packed, n_reads, read_len, span, dst, b->tile_recs_hist.as<u32>() + (b->tile_recs.n / sort_tile) * 256,
                                                    sort_tile, stream));
            } else {
                KCHECK(katome_dev_extract_tiles(b, d_packed, n_reads, read_len, span, nullptr, dst, stream));
            }
            b->tile_recs_hist_ok = counted;
            b->span = span;
            b->tile_recs.n += n;
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
    if (span < 2 || b->s.k + span - 1 > 95 || ((b->tiles_ready || b->tile_recs.n) && span != b->span)) { set_error("bad tile span %u", span); return KATOME_E_ARG; }
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
    if (var_tiles) KCHECK(var_origin(b, n_records, 1, span, &origin));
    else if (b->first_seen) KCHECK(fixed_origin(b, n_records, span, false, &origin));
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
    if (b->tile_recs.n) KCHECK(flush_tile_recs(b, stream));
    if (b->rest.n) KCHECK(flush_rest(b, stream));
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
        b->depth_index.drop();
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
    if (b->rest.n) KCHECK(flush_rest(b, (hipStream_t)stream));
    if (!b->table_ready) return KATOME_OK;
    return table_occupied(b->table, out, (hipStream_t)stream);
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
    b->depth_index.drop();
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
    b->depth_index.drop();
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
    b->depth_index.drop();
    KCHECK(dev_standardize_scale(b->edge_weight.as<u32>(), b->n_edges, original_genome_length, b->s.k, threshold, stream));
    KCHECK(weak_edges_ordered(b, 1, stream));          // "remove edges with weight 0" (standardizer.rs:68-69)
    KCHECK(dev_labels(b->edge_key.as<u64>(), b->n_edges, b->s.k, b->edge_label.as<uint8_t>(), stream));
    KCHECK_HIP(hipStreamSynchronize(stream));
    return KATOME_OK;
}

int katome_dev_shrink(katome_builder* b, katome_dev_contigs* out, void* stream_) {
    return katome_dev_shrink_mode(b, KATOME_SHRINK_AUTO, out, nullptr, stream_);
}
// every shrink entry: `cov` null drops the builder's coverage (none can outlive the result it belongs to), non-null fills it
static int builder_shrink(katome_builder* b, uint32_t mode, katome_dev_contigs* out, katome_dev_coverage* cov, bool want_cov, double* host_ms,
                          hipStream_t stream) {
    if (!b || !out || (want_cov && !cov)) { set_error("null argument"); return KATOME_E_ARG; }
    KCHECK_HIP(hipSetDevice(b->s.device));
    if (host_ms) *host_ms = 0;
    if (!b->finalized) { set_error("shrink: call katome_dev_finalize first"); return KATOME_E_ARG; }
    if (mode > KATOME_SHRINK_EXACT) { set_error("shrink: unknown mode %u", mode); return KATOME_E_ARG; }
    // (auto: a graph in the reference's numbering gets the reference's own result -- its numbering is what the stage after it reads)
    const bool exact = mode == KATOME_SHRINK_EXACT || (mode == KATOME_SHRINK_AUTO && b->first_seen);
    ShrinkInput in{b->edge_src.as<u64>(), b->edge_dst.as<u64>(), b->edge_weight.as<u32>(), b->edge_key.as<u64>(), b->node_key.as<u64>(),
                   b->n_edges, b->n_nodes, b->nw, b->s.k};
    b->shrunk_cov.drop();
    ShrinkCoverage* sc = want_cov ? &b->shrunk_cov : nullptr;
    {
        PhaseScope ps(b->prof, PH_SHRINK, stream);
        if (exact) KCHECK(dev_shrink_exact(in, b->edge_age.p ? b->edge_age.as<u32>() : nullptr, b->shrunk, host_ms, stream, nullptr, nullptr, sc));
        else KCHECK(dev_shrink(in, b->shrunk, stream, sc));
    }
    memset(out, 0, sizeof *out);
    out->n_nodes = b->shrunk.n_nodes; out->n_edges = b->shrunk.n_edges; out->label_bytes = b->shrunk.label_bytes;
    out->key_words = b->nw;
    out->d_edge_src = b->shrunk.edge_src.as<u64>(); out->d_edge_dst = b->shrunk.edge_dst.as<u64>();
    out->d_edge_weight = b->shrunk.edge_weight.as<u32>(); out->d_edge_kmers = b->shrunk.edge_kmers.as<u32>();
    out->d_edge_label_off = b->shrunk.edge_label_off.as<u64>(); out->d_edge_label = b->shrunk.edge_label.as<uint8_t>();
    out->d_node_key = b->shrunk.node_key.as<u64>();
    if (want_cov) {
        memset(cov, 0, sizeof *cov);
        cov->n_edges = b->shrunk_cov.n_edges;
        cov->d_kmer_sum = b->shrunk_cov.kmer_sum.as<u64>(); cov->d_kmer_min = b->shrunk_cov.kmer_min.as<u32>(); cov->d_kmer_max = b->shrunk_cov.kmer_max.as<u32>();
    }
    return KATOME_OK;
}
int katome_dev_shrink_mode(katome_builder* b, uint32_t mode, katome_dev_contigs* out, double* host_ms, void* stream_) {
    return builder_shrink(b, mode, out, nullptr, false, host_ms, (hipStream_t)stream_);
}
int katome_dev_shrink_coverage(katome_builder* b, uint32_t mode, katome_dev_contigs* out, katome_dev_coverage* cov, double* host_ms, void* stream_) {
    return builder_shrink(b, mode, out, cov, true, host_ms, (hipStream_t)stream_);
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
    b->collapse_valid = false; b->collapse_pieces.release(); b->collapse_n_pieces = 0;
    {
        PhaseScope ps(b->prof, PH_COLLAPSE, stream);
        KCHECK(dev_collapse(in, b->edge_age.p ? b->edge_age.as<u32>() : nullptr, b->collapse_shrunk, layout, b->assembly, stats, lengths, stream,
                            &b->collapse_pieces, &b->collapse_n_pieces));
    }
    b->collapse_valid = true;          // (no edges: no pieces, and a text of the header line alone)
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
    // KATOME_TEXT_TRACE=1: the writing kernel's time on stderr (there is no builder whose profile could hold it; tools/bench_unique.py)
    ArraysTrace trace("KATOME_TEXT_TRACE", "katome_dev_pieces_text");
    TextPlan plan;
    {
        PhaseScope ps(trace.prof, PH_COLLAPSE, stream);
        KCHECK(dev_text_plan(k, d_label, d_label_off, n_labels, d_pieces, n_pieces, layout, first_contig, plan, stream));
        *n_contigs = plan.n_contigs; *text_bytes = plan.text_bytes;
        if (!d_text || plan.text_bytes == 0) return KATOME_OK;
        if (!d_contig_off || !d_contig_len || contig_cap < plan.n_contigs || text_cap < (plan.text_bytes + 15) / 16 * 16 || ((uintptr_t)d_text & 15)) {
            set_error("text: %llu contigs and %llu bytes (rounded up to 16, 16-byte aligned) do not fit the caller's arrays", (unsigned long long)plan.n_contigs,
                      (unsigned long long)plan.text_bytes);
            return KATOME_E_ARG;
        }
        KCHECK(dev_text_write(k, d_label, d_label_off, d_pieces, n_pieces, layout, first_contig, plan, d_contig_off, d_contig_len, d_text, stream));
    }
    KCHECK_HIP(hipStreamSynchronize(stream));
    trace.print(K_TEXT_WRITE, K_TEXT_WRITE, plan.text_bytes, n_pieces, "pieces", plan.n_contigs, "contigs");
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
int katome_dev_count_in_key(int device, const uint64_t* d_tiles, const uint32_t* d_counts, uint64_t n_tiles, uint32_t tile_bases, uint32_t k, uint32_t span,
                            uint32_t stride, int rc, int packed, uint64_t* d_pass1_keys, uint32_t* d_pass1_weights, uint64_t* d_pass2_keys,
                            uint32_t* d_pass2_weights, uint64_t* d_out_keys, uint32_t* d_out_weights, uint64_t* n_out, int* took_packed, void* stream) {
    KCHECK(use_device(device));
    if (!n_out || !took_packed || (n_tiles && (!d_tiles || !d_counts || !d_out_keys || !d_out_weights))) { set_error("null argument"); return KATOME_E_ARG; }
    if (!d_pass1_keys != !d_pass1_weights || !d_pass2_keys != !d_pass2_weights) { set_error("count in key: a pass's keys and weights go together"); return KATOME_E_ARG; }
    if (!span || tile_bases < k || (uint64_t)stride * (span - 1) + k > tile_bases || k < 9 || tile_bases > 64) { set_error("count in key: the sub-windows do not lie in the tile"); return KATOME_E_ARG; }
    uint64_t* const pk[2] = {d_pass1_keys, d_pass2_keys}; uint32_t* const pw[2] = {d_pass1_weights, d_pass2_weights};
    return dev_count_in_key_level(d_tiles, d_counts, n_tiles, tile_bases, k, span, stride, rc != 0, packed != 0, pk, pw, d_out_keys, d_out_weights, n_out, took_packed,
                                  (hipStream_t)stream);
}
int katome_dev_count_records(int device, const uint64_t* d_keys, const uint32_t* d_weights, uint64_t n, uint32_t k, int rc, uint32_t min_weight, uint32_t n_parts,
                             uint64_t* d_out_keys, uint32_t* d_out_weights, uint64_t out_capacity, uint64_t* n_out, uint64_t* n_distinct, uint64_t* owner_base,
                             uint64_t* owner_count, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    KCHECK(use_device(device));
    if (!n_out || !n_distinct || (n_parts && (!owner_base || !owner_count)) || (n && (!d_keys || !d_out_keys || !d_out_weights))) { set_error("null argument"); return KATOME_E_ARG; }
    *n_out = 0; *n_distinct = 0;
    if (k < 2 || k > 95) { set_error("count records: k = 2 .. 95"); return KATOME_E_ARG; }
    if (n_parts > (uint32_t)KATOME_MAX_RANKS) { set_error("count records: at most %d owners", KATOME_MAX_RANKS); return KATOME_E_ARG; }
    if (n >= (1ull << 40) || out_capacity < (rc ? 2 : 1) * n + 1) { set_error("count records: room for (rc ? 2 : 1) * n + 1 entries"); return KATOME_E_ARG; }
    for (uint32_t p = 0; p < n_parts; ++p) owner_base[p] = owner_count[p] = 0;
    if (!n) return KATOME_OK;
    const size_t nw = (size_t)key_words_for_k(k);
    DevBuf keys(stream), weights(stream), ok(stream), ow(stream);          // (copies: the count consumes and permutes its records)
    KCHECK(keys.alloc((n + 1) * 8 * nw));
    KCHECK_HIP(hipMemcpyAsync(keys.p, d_keys, n * 8 * nw, hipMemcpyDeviceToDevice, stream));
    if (d_weights) {
        KCHECK(weights.alloc((n + 1) * 4));
        KCHECK_HIP(hipMemcpyAsync(weights.p, d_weights, n * 4, hipMemcpyDeviceToDevice, stream));
    }
    OwnerSplit split;
    split.n_parts = n_parts; split.core_shift = 2; split.core_bases = k - 2;          // (as dist.hip sets them)
    uint64_t n_list = 0, distinct = 0;
    const int st = records_to_edges_sorted(keys, weights, n, k, rc != 0, min_weight, ok, ow, &n_list, &distinct, stream, n_parts ? &split : nullptr, nullptr, nullptr, nullptr);
    if (st != KATOME_OK) { hipStreamSynchronize(stream); return st; }
    // (with owners the stretches lie where the owners' first records lay: anywhere among the first n entries)
    const uint64_t n_copy = n_parts ? n : n_list;
    if (n_copy > out_capacity || n_list > out_capacity) { set_error("count records: %llu entries of %llu records", (unsigned long long)n_list, (unsigned long long)n); return KATOME_E_DEVICE; }
    KCHECK_HIP(hipMemcpyAsync(d_out_keys, ok.p, n_copy * 8 * nw, hipMemcpyDeviceToDevice, stream));
    KCHECK_HIP(hipMemcpyAsync(d_out_weights, ow.p, n_copy * 4, hipMemcpyDeviceToDevice, stream));
    KCHECK_HIP(hipStreamSynchronize(stream));
    for (uint32_t p = 0; p < n_parts; ++p) { owner_base[p] = split.base[p]; owner_count[p] = split.count[p]; }
    *n_out = n_list; *n_distinct = distinct;
    return KATOME_OK;
}
void katome_s2_region_starts(const uint64_t* used, uint64_t* start) {
    uint64_t cap[S2_REGIONS];
    for (uint32_t d = 0; d < S2_REGIONS; ++d) cap[d] = s2_tiles(used[d]) * S2_REGION_TILE;
    s2_region_starts(cap, start);
}
int katome_dev_s2_region_pass(int device, uint32_t k, const uint64_t* used, const uint64_t* d_keys, const uint32_t* d_weights, const uint8_t* d_digits,
                              uint64_t* d_keys_out, uint32_t* d_weights_out, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    KCHECK(use_device(device));
    if (!used || !d_keys || !d_weights || !d_digits || !d_keys_out || !d_weights_out) { set_error("null argument"); return KATOME_E_ARG; }
    uint64_t start[S2_REGIONS + 1];
    katome_s2_region_starts(used, start);
    KCHECK(dev_s2_region_pass(d_keys, d_weights, d_digits, k, start, used, d_keys_out, d_weights_out, nullptr, stream));
    KCHECK_HIP(hipStreamSynchronize(stream));
    return KATOME_OK;
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
