// kept_records.hip -- the records a build keeps aside between batches (builder.h, KeptRecords: the big-tile records and the left-over
// windows), so that their levels can be counted by sorting when the edges are asked for (count_routes.hip): what keeps a batch, and
// the ways back into the tables when keeping is given up.  Host control flow only; the kernels are table.hip's.
#include <stdlib.h>

#include "builder.h"
#include "seen_tag.h"

// how the builder's tagged records spell their two numbers
SeenTag builder_tag(const katome_builder* b) {
    return b->seen_delta ? SeenTag::by_delta() : SeenTag::fixed(2ull * (b->seen_read_len - b->s.k + 1));
}

// ---- KeptRecords -------------------------------------------------------------------------------------------------------------------
// (n counts what was handed over, skipped reads included: only the device cursor knows how many of them were valid, unless `exact`)
int KeptRecords::valid(uint64_t* n_valid, hipStream_t stream) {
    *n_valid = 0;
    if (exact) { *n_valid = n; return KATOME_OK; }       // (every record kept so far was valid: nothing to ask the device)
    if (!n || !count.p) return KATOME_OK;
    KCHECK_HIP(hipMemcpyAsync(n_valid, count.p, 8, hipMemcpyDeviceToHost, stream));
    KCHECK_HIP(hipStreamSynchronize(stream));
    return KATOME_OK;
}

int KeptRecords::reserve(katome_builder* b, uint64_t n_new, uint32_t w, bool* ok, hipStream_t stream) {
    *ok = false;
    if (n + n_new > cap) {
        size_t free_b = 0, total_b = 0;
        KCHECK_HIP(hipMemGetInfo(&free_b, &total_b));
        uint64_t pool[3] = {0, 0, 0};
        if (policy.idle_counts) dev_cache_stats(b->s.device, pool);          // (what the caching allocator holds idle is as good as free)
        // (KATOME_TILE_RECS_LIMIT: no more tile records than this are kept aside -- tests)
        static const uint64_t limit = getenv("KATOME_TILE_RECS_LIMIT") ? strtoull(getenv("KATOME_TILE_RECS_LIMIT"), nullptr, 10) : ~0ull;
        const KeepPlan plan = keep_plan(policy, n, cap, n_new, w, free_b, pool[1], total_b, limit);
        if (plan.action == KEEP_REFUSE) return flush(b, stream);
        DevBuf grown(stream);
        if (const int rc = grown.alloc(plan.want * 8 * w + 16)) {
            if (!policy.alloc_fail_refuses) return rc;
            return flush(b, stream);                       // (no room after all: the table takes over)
        }
        if (n) KCHECK_HIP(hipMemcpyAsync(grown.p, recs.p, n * 8 * w, hipMemcpyDeviceToDevice, stream));
        recs.adopt(grown);
        recs.stream = stream;
        cap = plan.want;
        words = w;
    }
    if (n == 0 && policy.exact_while_empty) exact = true;
    *ok = true;
    return KATOME_OK;
}

int KeptRecords::cursor(hipStream_t stream) {
    const bool fresh = !count.p;
    if (fresh) KCHECK(count.alloc(8, stream));
    if (exact) {
        // from here on only the device knows how many of the records handed over were valid: its cursor starts at what the host knew
        const uint64_t start = n;
        KCHECK_HIP(hipMemcpyAsync(count.p, &start, 8, hipMemcpyHostToDevice, stream));
        KCHECK_HIP(hipStreamSynchronize(stream));
        exact = false;
    } else if (fresh) {
        KCHECK_HIP(hipMemsetAsync(count.p, 0, 8, stream));
    }
    return KATOME_OK;
}

// ---- the ways back into the tables -----------------------------------------------------------------------------------------------
int insert_tagged(katome_builder* b, Table& table, bool& ready, uint32_t nw, uint64_t hint, const uint64_t* d_tagged, const uint32_t* d_counts,
                  uint64_t n, int phase, hipStream_t stream, DevBuf* spent) {
    DevBuf keys(stream), pairs(stream);
    KCHECK(keys.alloc(n * 8 * nw + 16)); KCHECK(pairs.alloc(n * 16 + 16));
    KCHECK(table_tagged_to_pairs(d_tagged, n, nw, builder_tag(b), keys.as<u64>(), pairs.as<u64>(), stream));
    if (spent) spent->release();
    SeenOrigin origin;
    origin.pairs = pairs.as<u64>(); origin.rc = b->rc;
    return builder_insert(b, table, ready, nw, hint, keys.as<u64>(), d_counts, n, &origin, phase, stream);
}

// the left-over windows kept aside go into the k-mer table after all: another consumer wants the table, or there are too many of them
int flush_rest(katome_builder* b, hipStream_t stream) {
    uint64_t n = 0;
    KCHECK(b->rest.valid(&n, stream));
    // (first-seen order: tagged records -- back into keys + their two sequence numbers for the table)
    if (n && b->first_seen) KCHECK(insert_tagged(b, b->table, b->table_ready, b->nw, b->s.table_slots_hint, b->rest.recs.as<u64>(), nullptr, n, PH_INSERT, stream));
    else if (n) KCHECK(builder_insert(b, b->table, b->table_ready, b->nw, b->s.table_slots_hint, b->rest.recs.as<u64>(), nullptr, n, nullptr, PH_INSERT, stream));
    b->rest.close();
    return KATOME_OK;
}

// no tile records are kept from here on (they were counted, or went into the tile table)
void close_tile_recs(katome_builder* b) {
    b->tile_recs.close();
    b->tile_recs_hist.release(); b->tile_recs_hist_ok = false;
}
// the tile records kept aside go into the tile table after all: another consumer wants the table, or the sorted counting of the tiles
// gave up
int flush_tile_recs(katome_builder* b, hipStream_t stream) {
    if (b->tile_recs.n) {
        const uint32_t nwt = (uint32_t)key_words_for_k(b->s.k + b->span - 1);
        const uint64_t hint = b->s.table_slots_hint / 4;
        uint64_t n = 0;
        KCHECK(b->tile_recs.valid(&n, stream));
        b->tile_recs.n = 0;
        // (first-seen order: tagged records, whose array goes as soon as they are keys and pairs)
        if (n && b->first_seen) KCHECK(insert_tagged(b, b->tiles, b->tiles_ready, nwt, hint, b->tile_recs.recs.as<u64>(), nullptr, n, PH_INSERT_TILES, stream, &b->tile_recs.recs));
        else if (n) KCHECK(builder_insert(b, b->tiles, b->tiles_ready, nwt, hint, b->tile_recs.recs.as<u64>(), nullptr, n, nullptr, PH_INSERT_TILES, stream));
    }
    close_tile_recs(b);
    return KATOME_OK;
}

// ---- keeping a batch ---------------------------------------------------------------------------------------------------------------
// a batch's tiles kept aside as records; *kept = false: they go into the tile table
int keep_tile_recs(katome_builder* b, const uint64_t* d_records, uint64_t n, uint32_t nwt, bool* kept, hipStream_t stream) {
    *kept = false;
    b->tile_recs_hist_ok = false;          // (records that nobody counted as they were written)
    bool ok = false;
    KeptRecords& t = b->tile_recs;
    // (first-seen order: a record is kept with its tag -- read << 32 | number of its first window << 16 | of its reverse complement's)
    const uint32_t words = nwt + (b->first_seen ? 1 : 0);
    KCHECK(t.reserve(b, n, words, &ok, stream));
    if (!ok) return KATOME_OK;
    KCHECK(t.cursor(stream));
    if (b->first_seen) {
        const uint32_t W = b->seen_read_len - b->s.k + 1;
        KCHECK(table_keep_rest(d_records, n, nwt, true, b->reads_inserted, W / b->span, 0, 2 * W, t.recs.as<u64>(), t.count.as<u64>(), stream,
                               b->span, b->span));
    } else
    KCHECK(table_keep_rest(d_records, n, nwt, false, 0, 1, 0, 0, t.recs.as<u64>(), t.count.as<u64>(), stream));      // (the valid ones, behind the cursor)
    t.n += n;
    *kept = true;
    return KATOME_OK;
}

// keeps a batch's left-over windows aside (see builder.h); *kept = false: they have to go into the table
int keep_rest(katome_builder* b, const uint64_t* d_records, uint64_t n, bool* kept, hipStream_t stream) {
    *kept = false;
    bool ok = false;
    KeptRecords& r = b->rest;
    KCHECK(r.reserve(b, n, b->nw + (b->first_seen ? 1 : 0), &ok, stream));          // (first-seen order: tagged records)
    if (!ok) return KATOME_OK;
    KCHECK(r.cursor(stream));
    KCHECK(table_keep_rest(d_records, n, b->nw, b->first_seen, b->last_batch_read0, b->rem_per_read, b->rem_win0,
                           b->first_seen ? 2u * (b->seen_read_len - b->s.k + 1) : 0u, r.recs.as<u64>(), r.count.as<u64>(), stream));
    r.n += n;
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
    if (!b->tile_recs.closed) KCHECK(flush_tile_recs(b, stream));
    if (!b->rest.closed) KCHECK(flush_rest(b, stream));
    return KATOME_OK;
}
// the tiles of the last katome_dev_extract_var_tiles call behind the tile records kept so far; *kept = false: into the tile table
int keep_var_tiles(katome_builder* b, const uint64_t* d_records, uint64_t n, uint32_t nwt, bool* kept, hipStream_t stream) {
    *kept = false;
    bool ok = false;
    KeptRecords& t = b->tile_recs;
    KCHECK(var_batch_packs(b, &ok, stream));
    if (!ok) return close_seen_var(b, stream);
    b->tile_recs_hist_ok = false;
    KCHECK(t.reserve(b, n, nwt + 1, &ok, stream));
    if (!ok) return KATOME_OK;
    KCHECK(t.cursor(stream));
    KCHECK(table_keep_var_tagged(d_records, n, nwt, b->rc, b->var_prefix, b->var_rec_prefix, b->var_reads, 1, b->var_span, b->var_seq_base,
                                 t.recs.as<u64>(), t.count.as<u64>(), stream));
    t.n += n;
    b->seen_delta = true;
    *kept = true;
    return KATOME_OK;
}
// ... and its windows (all of them, or those after the last whole tile) behind the left-over windows; *kept = false: into the k-mer table
int keep_var_rest(katome_builder* b, const uint64_t* d_records, uint64_t n, bool* kept, hipStream_t stream) {
    *kept = false;
    bool ok = false;
    KeptRecords& r = b->rest;
    KCHECK(var_batch_packs(b, &ok, stream));
    if (!ok) return close_seen_var(b, stream);
    KCHECK(r.reserve(b, n, b->nw + 1, &ok, stream));
    if (!ok) return KATOME_OK;
    KCHECK(r.cursor(stream));
    KCHECK(table_keep_var_tagged(d_records, n, b->nw, b->rc, b->var_prefix, b->var_rec_prefix, b->var_reads, b->var_mode, b->var_span, b->var_seq_base,
                                 r.recs.as<u64>(), r.count.as<u64>(), stream));
    r.n += n;
    b->seen_delta = true;
    *kept = true;
    return KATOME_OK;
}

// room in b->tile_recs_hist for the counts of n_total kept records (the record array's capacity; what is there is kept);
// false: no room -- the first pass counts for itself
bool reserve_tile_hist(katome_builder* b, uint64_t n_total, uint32_t sort_tile, bool keep, hipStream_t stream) {
    const uint64_t need = ((n_total + sort_tile - 1) / sort_tile) * 256 * 4 + 16;
    if (need <= b->tile_recs_hist.bytes) return true;
    DevBuf grown(stream);
    if (grown.alloc(need) != KATOME_OK) return false;
    if (keep && b->tile_recs_hist.p &&
        hipMemcpyAsync(grown.p, b->tile_recs_hist.p, ((b->tile_recs.n + sort_tile - 1) / sort_tile) * 256 * 4, hipMemcpyDeviceToDevice, stream) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    b->tile_recs_hist.adopt(grown);
    b->tile_recs_hist.stream = stream;
    return true;
}
