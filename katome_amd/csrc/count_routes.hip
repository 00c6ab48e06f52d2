// count_routes.hip -- katome_dev_edges: the builder's sorted distinct edges.  The counting routes are tried in turn, each leaving to
// the next what it could not count: the levels counted by sorting (lds_count.hip) out of the records kept aside (kept_records.hip)
// or out of the tile table, and the table route (api.hip's expand_tiles).  With them what they plan with -- the knobs, the memory a
// level may take -- and tile_recs_to_kmer_records, which the one-exchange sharded route (dist.hip) shares.  Host control flow only.
#include <stdlib.h>

#include <algorithm>
#include <memory>
#include <vector>

#include "builder.h"
#include "seen_tag.h"

int sorted_count_mode() {
    static const int mode = env_int("KATOME_SORTED_COUNT", 1);
    return mode;
}
// is counting n records by sorting worth its extra launches?  (KATOME_SORTED_COUNT=2: however few -- tests)
bool sorting_pays(uint64_t n) { return n && (n >= (1ull << 22) || sorted_count_mode() == 2); }
// the most records a caller hands to the LDS counting route (2^16 hash groups of 32 sub-rounds of 2900 records)
bool lds_route_takes(uint64_t n) { return (n >> 21) <= 2900; }

// First-seen order, reads of varying length: the levels counted by sorting, the batches' records kept aside with delta tags
// (seen_tag.h).  KATOME_SEEN_VAR_SORTED=1 switches it on; off, such a build counts every level in the tables
bool seen_var_sorted() { static const bool on = env_flag("KATOME_SEEN_VAR_SORTED", false); return on; }

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
        KCHECK(b->tile_recs.valid(&n, stream));
        // (the whole array is ordered in this one call: the counts the extraction left, where they cover it, are its first pass's)
        u32* const first = b->tile_recs_hist_ok && n == b->tile_recs.n && nwt == 2 ? b->tile_recs_hist.as<u32>() : nullptr;
        rc = n ? records_to_edges_sorted(b->tile_recs.recs, ones, n, tile_bases, false, 0, t1k, t1w, &n1, &d1, stream, nullptr, first)
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

// The left-over windows kept aside (b->rest, of the width they were kept with: nw words, or nw + 1 for tagged records) behind the
// n_rec records in keys / weights, weight 1 each.  orient: the records are in their representative orientation (the half sort's k-mer records)
static int append_rest(katome_builder* b, DevBuf& keys, DevBuf& weights, uint64_t* n_rec, uint64_t n_rest, bool orient, hipStream_t stream) {
    if (!n_rest) return KATOME_OK;
    const uint32_t words = b->rest.words;
    KCHECK_HIP(hipMemcpyAsync(keys.as<u64>() + *n_rec * words, b->rest.recs.p, n_rest * 8 * words, hipMemcpyDeviceToDevice, stream));
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
    KCHECK(b->rest.valid(&n_rest, stream));
    DevBuf first_counts(stream);
    const bool half = half_sort_route(b);
    HalfSort hs;
    RecordSource src;          // (the k-mer records may be left to their first partition pass: see RecordSource)
    int rc = tile_recs_to_kmer_records(b, rk, rw, &n_rec, n_rest, stream, &first_counts, half, &src);
    if (rc == KATOME_E_UNSUPPORTED) return KATOME_OK;          // (the tiles are in their table now, the table routes take it from there)
    if (rc != KATOME_OK) return rc;
    {
        PhaseScope ps(b->prof, PH_EXPAND_TILES, stream);
        KCHECK(append_rest(b, rk, rw, &n_rec, n_rest, half && b->rc, stream));
        b->rest.reset();
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
    const uint64_t bound = n_tiles * b->span + b->rest.n;        // the k-mer records can be no more than this
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
    if (!level_fits(last_tiles * last_span + b->rest.n, b->nw, b->rc, "k-mers (tiles in their table)")) return KATOME_OK;
    DevBuf rk(stream), rw(stream);
    uint64_t n_rec = 0, distinct = 0;
    int rc = KATOME_OK;
    {
        PhaseScope ps(b->prof, PH_EXPAND_TILES, stream);
        uint64_t n_rest = 0;
        KCHECK(b->rest.valid(&n_rest, stream));
        if (mid_sorted) {
            KCHECK(table_list_to_records(t2k.as<u64>(), t2w.as<u32>(), n_mid_list, b->s.k + sp2 - 1, b->s.k, sp2, 1, b->rc, rk, rw, &n_rec, stream, n_rest));
            t2k.release(); t2w.release();
        } else
        KCHECK(table_tiles_to_records_fast(*last, b->s.k, last_span, b->rc, rk, rw, &n_rec, stream, n_rest));
        KCHECK(append_rest(b, rk, rw, &n_rec, n_rest, false, stream));
        rc = sorted_fail("last") ? KATOME_E_UNSUPPORTED
            : records_to_edges_sorted(rk, rw, n_rec, b->s.k, b->rc, b->prune_weight, b->edge_key, b->edge_weight, &b->n_edges, &distinct, stream);
        if (rc != KATOME_OK && rc != KATOME_E_UNSUPPORTED) return rc;
    }
    // (a group too large for the LDS route: the table counts, from the tiles that are still there)
    if (rc != KATOME_OK) { b->n_edges = 0; return KATOME_OK; }
    release_tile_tables(b);
    b->rest.reset();
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
    KCHECK(b->tile_recs.valid(&n, stream));
    DevBuf l1(stream), c1(stream);
    int rc = KATOME_E_UNSUPPORTED;
    if (n) {
        PhaseScope ps(b->prof, PH_INSERT_TILES, stream);
        TileLevelScope tl;
        DevBuf ones(stream);               // (stays empty: the records count once each)
        rc = tagged_records_sorted(b->tile_recs.recs, ones, n, tile_bases, b->rc, tag, true, l1, c1, &n1, &d1, stream);
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
        KCHECK(b->rest.valid(&n_rest, stream));
        DevBuf last_counts(stream);
        KCHECK(table_list_to_tagged_records(lk, lw, n_last, last_bases, k, last_span, 1, b->rc, kr, kw, &n_rec, stream, n_rest, &last_counts, tag.delta));
        l2.release(); c2.release();
        KCHECK(append_rest(b, kr, kw, &n_rec, n_rest, false, stream));
        rc = sorted_fail("last") ? KATOME_E_UNSUPPORTED
            : tagged_records_sorted(kr, kw, n_rec, k, b->rc, tag, false, b->edge_key, raw_seq, &b->n_edges, &distinct, stream, last_counts.as<u32>());
        if (rc != KATOME_OK && rc != KATOME_E_UNSUPPORTED) return rc;
    }
    if (rc == KATOME_OK) {
        l1.release(); c1.release();
        b->rest.reset();
        b->stat_kmers = distinct; b->stat_kmer_slots = 0;
        *counted = true;
        return KATOME_OK;
    }
    // a level below gave up: the distinct big tiles go into the tile table with their counts and their numbers, and the build goes on
    // from there as if they had been counted in it
    b->n_edges = 0;
    l2.release(); c2.release();
    return insert_tagged(b, b->tiles, b->tiles_ready, (uint32_t)key_words_for_k(tile_bases), b->s.table_slots_hint / 4, l1.as<u64>(), c1.as<u32>(), n1,
                         PH_INSERT_TILES, stream, &l1);
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
        KCHECK(b->rest.valid(&n_rest, stream));
        rc = sorted_fail("last") && var ? KATOME_E_UNSUPPORTED
            : tiles_to_edges_sorted_seen(*last, b->s.k, last_span, b->rc, tag, b->edge_key, raw_seq, &b->n_edges,
                                         &distinct, stream, n_rest ? b->rest.recs.as<u64>() : nullptr, n_rest);
        if (rc != KATOME_OK && rc != KATOME_E_UNSUPPORTED) return rc;
    }
    // (numbers that do not pack, or a group too large: the table counts, from the tiles that are still there)
    if (rc != KATOME_OK) { b->n_edges = 0; return KATOME_OK; }
    release_tile_tables(b);
    b->rest.reset();
    b->stat_kmers = distinct; b->stat_kmer_slots = 0;
    *counted = true;
    return KATOME_OK;
}

// ... and of one that kept windows only (KATOME_SEEN_VAR_SORTED: reads of varying length cut window by window, or none of them as long
// as a tile): the tagged records kept aside are the level's records.
// on fallback: they are still kept aside, in another order (the table route flushes them); n_edges == 0
static int seen_edges_from_rest(katome_builder* b, DevBuf& raw_seq, bool* counted, hipStream_t stream) {
    if (!b->seen_delta || !sorted_count_mode() || b->tiles_ready || b->table_ready || b->tile_recs.n || !b->rest.n || b->nw > 2) return KATOME_OK;
    uint64_t n_rest = 0, distinct = 0;
    KCHECK(b->rest.valid(&n_rest, stream));
    if (!sorting_pays(n_rest)) return KATOME_OK;
    PhaseScope ps(b->prof, PH_EXPAND_TILES, stream);
    DevBuf ones(stream);               // (stays empty: the records count once each)
    const int rc = sorted_fail("last") ? KATOME_E_UNSUPPORTED
        : tagged_records_sorted(b->rest.recs, ones, n_rest, b->s.k, b->rc, SeenTag::by_delta(), false, b->edge_key, raw_seq, &b->n_edges, &distinct, stream);
    if (rc != KATOME_OK && rc != KATOME_E_UNSUPPORTED) return rc;
    if (rc != KATOME_OK) { b->n_edges = 0; return KATOME_OK; }
    b->rest.reset();
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

extern "C" {

// The builder's sorted distinct edges: the counting routes are tried in turn, each leaving to the next what it could not count
int katome_dev_edges(katome_builder* b, uint64_t** d_edge_key, uint32_t** d_edge_weight, uint64_t* n_edges, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    KCHECK_HIP(hipSetDevice(b->s.device));
    if (!b->edges_ready) {
        b->n_edges = 0;
        b->drop_edge_heads();
        b->tile_scratch.release();
        // (tile records with k-mers in the table already, or too few of them to be worth sorting: into the tile table)
        if (b->tile_recs.n && (b->table_ready || !sorting_pays(b->tile_recs.n * b->span))) KCHECK(flush_tile_recs(b, stream));
        bool counted = false;
        DevBuf raw_seq(stream);                  // (first-seen order: the edges' sequence numbers and weights until the sort tail)
        if (!b->first_seen) {
            if (b->tile_recs.n) KCHECK(edges_from_tile_recs(b, &counted, stream));
            if (!counted) KCHECK(edges_from_tile_table(b, &counted, stream));
            if (!counted) KCHECK(edges_from_table(b, false, raw_seq, stream));
        } else {
            const char* route = "tile records";
            if (b->tile_recs.n) KCHECK(seen_edges_from_tile_recs(b, raw_seq, &counted, stream));
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

}  // extern "C"
