// builder.h -- one GPU's share of a build: the state behind `katome_builder` and the internal steps that the C ABI
// (api.hip, kept_records.hip, count_routes.hip, gfa.hip, host_build.cpp) and the sharded driver (dist.hip) compose.  Reference path: Build::create (builder.rs:42-54) ->
// add_read_fastaq (pt_graph.rs:277-315) -> add_single_edge_fastaq (172-198) -> post-pass (333-345).
#pragma once
#include <vector>

#include "common.h"
#include "keep_plan.h"

using namespace katome;

// what crosses a file boundary inside the library, but not the library's: not among its dynamic symbols
#define KATOME_INTERNAL __attribute__((visibility("hidden")))

struct katome_builder;
KATOME_INTERNAL int flush_tile_recs(katome_builder* b, hipStream_t stream);    // the tile records kept aside -> b->tiles
KATOME_INTERNAL int flush_rest(katome_builder* b, hipStream_t stream);         // the left-over windows kept aside -> b->table

// Records kept aside between batches, to be counted by sorting when the edges are asked for: a device array that kernels append to
// behind a device cursor.  The builder has two, the big-tile records and the left-over windows; they differ in their KeepPolicy
// (keep_plan.h) and in where `flush` puts them when keeping is given up.  Defined in kept_records.hip
struct KATOME_INTERNAL KeptRecords {
    const KeepPolicy policy;
    int (*const flush)(katome_builder*, hipStream_t);      // what was kept goes into its table, and the set is closed
    DevBuf recs, count;                 // count: the 8-byte device cursor -- how many of the records handed over were valid
    uint64_t n = 0, cap = 0;            // n: records handed over so far (an upper bound of the cursor)
    uint32_t words = 0;                 // u64 words per record the array was last grown for (first-seen order: key + tag)
    bool closed = false;                // nothing is kept from here on (they were counted, or went into their table)
    bool exact = false;                 // every record handed over so far was valid: n IS the count (katome_dev_count_tiles writes in place)
    KeptRecords(const KeepPolicy& p, int (*f)(katome_builder*, hipStream_t)) : policy(p), flush(f) {}
    // how many valid records wait
    int valid(uint64_t* n_valid, hipStream_t stream);
    // room for n_new more behind those kept; *ok = false: no room (or over the limit) -- what was kept has been flushed into its table
    // and later batches follow it there
    int reserve(katome_builder* b, uint64_t n_new, uint32_t words, bool* ok, hipStream_t stream);
    // the device cursor, ready for a kernel that appends behind it
    int cursor(hipStream_t stream);
    void reset() { recs.release(); count.release(); n = cap = 0; exact = false; }
    void close() { reset(); closed = true; }
};

// depth.hip: what katome_dev_depth searches -- the graph's edge keys in ascending order with a bucket directory over their top bits.
// keys / perm are empty where the graph's own d_edge_key ascends strictly (a by-key build): it is then searched as it lies; otherwise
// keys is a sorted copy and perm[i] the edge index of keys[i].  of_keys / n: the edge list the index was built for
struct KATOME_INTERNAL DepthIndex {
    DevBuf keys, perm, dir;
    uint32_t B = 0;
    bool valid = false;
    const void* of_keys = nullptr;
    uint64_t n = 0;
    void drop() { keys.release(); perm.release(); dir.release(); B = 0; valid = false; of_keys = nullptr; n = 0; }
    uint64_t bytes() const { return (keys.p ? keys.bytes : 0) + (perm.p ? perm.bytes : 0) + (dir.p ? dir.bytes : 0); }
};
// result of katome_dev_depth (its own buffers)
struct KATOME_INTERNAL DepthOutput {
    DevBuf present, invalid, sum, mn, mx, window_off, window_edge, edge_hits;
};

struct katome_builder {
    katome_settings s;
    Profiler prof;
    uint32_t nw = 1;
    bool rc = false;
    Table table;
    bool table_ready = false;
    // tiled counting: (k+span-1)-mers counted first, expanded into `table` before the edges are read out
    Table tiles;
    bool tiles_ready = false;
    uint32_t span = 1;
    // big tiles (span > 16) are first broken into mid tiles of span2 windows (a second tile table), those into k-mers
    Table tiles2;
    bool tiles2_ready = false;
    uint32_t span2 = 0;
    uint64_t stat_tiles2 = 0, stat_tile2_slots = 0;
    // bookkeeping for katome_builder_counts: distinct tiles, tile-table slots, distinct stored k-mers, k-mer-table slots
    // first-seen-order mode (KATOME_FLAG_FIRST_SEEN_ORDER)
    bool first_seen = false;
    uint64_t reads_inserted = 0;       // reads whose records have been handed to an insert so far
    uint32_t seen_read_len = 0;        // read length of the last extraction (records per read follow from it)
    // reads whose windows are not a whole number of tiles: the trailing windows come as plain k-mer records right after
    // the batch's tiles (katome_dev_extract_remainder); first-seen order needs to know where they sit in their reads
    bool rem_pending = false;
    uint32_t rem_win0 = 0, rem_per_read = 0;
    uint64_t last_batch_read0 = 0, last_batch_reads = 0;
    const uint64_t* var_prefix = nullptr;   // variable-length reads: window prefix of the last extraction (device), its reads
    uint64_t var_reads = 0, var_windows = 0;   // and windows; var_seq_base: sequence numbers handed out by earlier batches
    uint64_t var_seq_base = 0;
    const uint64_t* var_rec_prefix = nullptr;  // records before each read for the records just extracted (tiles / left-over windows)
    uint64_t var_records = 0;                  // how many of them: the insert that follows must take exactly these
    uint32_t var_mode = 0, var_span = 1;       // 0 every window, 1 whole tiles, 2 the windows after the last whole tile
    // first-seen order, reads of varying length, levels counted by sorting (KATOME_SEEN_VAR_SORTED): the tagged records kept aside
    // (tile_recs, rest) carry the delta tag of seen_tag.h, not seen_pack's; set with the first batch kept so
    bool seen_delta = false;
    // ... which is kept only if every read of it packs: the last batch asked about (its prefix and sequence base) and the answer
    const uint64_t* var_checked = nullptr; uint64_t var_checked_base = ~0ull; bool var_checked_ok = false;
    DevBuf edge_seq;                   // sequence number of each edge's first insertion, aligned with edge_key
    // by-packed-key builds: the windows left over after a batch's tiles wait here (records of weight 1), so that the last level can
    // be counted by sorting (lds_count.hip, records_to_edges_sorted) together with the tiles' k-mers; any other consumer of the k-mer
    // table flushes them into it first (flush_rest)
    // by-packed-key builds with two-word tiles and one-word k-mers: the tiles themselves are kept as records too and counted by
    // sorting when the edges are asked for (count_routes.hip, edges_from_tile_recs) -- no tile table, no device-scope atomics at any level
    KeptRecords tile_recs{KEEP_TILES, flush_tile_recs};      // (a skipped read's tiles are all-ones: not valid, not kept)
    // tile_recs_hist: counts[sort tile][256] of the first partition pass's digit over tile_recs, left by the extraction that wrote the
    // records (katome_dev_count_tiles); tile_recs_hist_ok: they cover all of tile_recs -- every batch so far started on a sort-tile
    // boundary and was written in place.  They grow and go with the records (close_tile_recs).
    DevBuf tile_recs_hist;
    bool tile_recs_hist_ok = false;
    DevBuf tile_scratch;                // katome_dev_count_tiles: a batch's records when they cannot be made where they are kept
    // (reads with N leave invalid left-over windows; rest.closed: too many to keep aside -- from now on they go into the table directly)
    KeptRecords rest{KEEP_REST, flush_rest};
    uint64_t direct_edges = 0;         // BFCounter input: the edges were listed one per line and strand (no table); their count
    uint32_t prune_weight = 0;      // Clean::remove_weak_edges threshold applied when the edges are read out
    uint64_t stat_tiles = 0, stat_tile_slots = 0, stat_kmers = 0, stat_kmer_slots = 0;
    // sorted distinct oriented edges
    bool edges_ready = false;
    DevBuf edge_key, edge_weight;
    uint64_t n_edges = 0;
    // the source run heads per block of edges, where the edges' merge counted them (half_sort_finish), and the edge list they were
    // counted for: katome_dev_finalize hands them to dev_node_ids only if edge_key and n_edges are still those.  Whoever installs
    // other edges drops them
    DevBuf edge_heads;
    const void* edge_heads_key = nullptr;
    uint64_t edge_heads_n = 0;
    void drop_edge_heads() { edge_heads.release(); edge_heads_key = nullptr; edge_heads_n = 0; }
    // scratch for ordering a batch by table region before it is inserted
    DevBuf scratch_k[2], scratch_w[2];
    // finalized graph
    DevBuf edge_src, edge_dst, edge_label, node_key;
    ShrinkOutput shrunk;               // result of katome_dev_shrink
    ShrinkCoverage shrunk_cov;         // ... and, after katome_dev_shrink_coverage only, its k-mer count sum / min / max (any other shrink drops them)
    ShrinkOutput collapse_shrunk;      // katome_dev_collapse: the shrunk graph its pieces name ...
    TextOutput assembly;               // ... and its result
    DevBuf collapse_pieces;            // ... and its piece list (4 bytes a piece), kept for katome_dev_collapse_gfa until the next collapse
    uint64_t collapse_n_pieces = 0;
    bool collapse_valid = false;       // the three above belong to one successful katome_dev_collapse
    GfaPathsOutput gfa_paths;          // result of katome_dev_collapse_gfa (its own buffers)
    GfaStrandPathsOutput gfa_strand_paths;      // result of katome_dev_collapse_gfa_strands (its own buffers)
    UniqueOutput unique;               // result of katome_dev_collapse_unique (its own buffers)
    TextOutput unitig_text;            // result of katome_dev_contigs_text
    GfaOutput gfa;                     // result of katome_dev_contigs_gfa
    GfaStrandsOutput gfa_strands;      // result of katome_dev_contigs_gfa_strands (its own buffers: neither call touches the other's result)
    DevBuf edge_age;                   // first-seen-order graphs once remove_* has moved edges (PruneGraph::edge_age)
    DepthIndex depth_index;            // katome_dev_depth's index over edge_key, kept between calls; whoever changes the set or the order
                                       // of the edges drops it (weights are read from edge_weight as it stands: they may change freely)
    DepthOutput depth;                 // result of katome_dev_depth
    uint64_t n_nodes = 0;
    bool finalized = false;
};


// ---- internal steps, by the file that defines them; dist.hip and host_build.cpp compose them too ------------------------------

// ---- api.hip: the table side ---------------------------------------------------------------------------------------------------
// find-or-insert `n` records (weights: nullptr = 1 each) into `table`, growing it under the load policy; `origin` places
// the records in the read-ordered stream when the builder tracks first-seen order (its rec0 is set per launch)
KATOME_INTERNAL int builder_insert(katome_builder* b, Table& table, bool& ready, uint32_t nw, uint64_t hint, const uint64_t* d_records,
                                   const uint32_t* d_weights, uint64_t n, SeenOrigin* origin, int phase, hipStream_t stream);
// big tiles -> mid tiles (when the span is large); leaves the tiles that hold k-mers directly in `*last`
KATOME_INTERNAL int expand_to_last_level(katome_builder* b, Table** last, uint32_t* last_span, hipStream_t stream);
KATOME_INTERNAL void release_tile_tables(katome_builder* b);     // b->tiles and b->tiles2 are spent
KATOME_INTERNAL int expand_tiles(katome_builder* b, hipStream_t stream);       // every distinct tile adds its count to its k-mers (b->table); the tile tables go
KATOME_INTERNAL uint32_t mid_span(uint32_t span);      // span of the mid tiles a big tile is broken into (0: expanded directly)

// ---- kept_records.hip: KeptRecords, what keeps a batch aside and the ways back into the tables (flush_* are declared above) ----
KATOME_INTERNAL SeenTag builder_tag(const katome_builder* b);      // how the builder's tagged records spell their two numbers
KATOME_INTERNAL void close_tile_recs(katome_builder* b);           // no tile records are kept from here on; their digit counts go with them
// a batch's valid tile records behind those kept so far; *kept = false: they go into the tile table
KATOME_INTERNAL int keep_tile_recs(katome_builder* b, const uint64_t* d_records, uint64_t n, uint32_t nwt, bool* kept, hipStream_t stream);
// ... its left-over windows (see katome_builder::rest); *kept = false: they have to go into the table
KATOME_INTERNAL int keep_rest(katome_builder* b, const uint64_t* d_records, uint64_t n, bool* kept, hipStream_t stream);
// first-seen order, reads of varying length: the records of the last katome_dev_extract_var* call with their delta tags
KATOME_INTERNAL int keep_var_tiles(katome_builder* b, const uint64_t* d_records, uint64_t n, uint32_t nwt, bool* kept, hipStream_t stream);
KATOME_INTERNAL int keep_var_rest(katome_builder* b, const uint64_t* d_records, uint64_t n, bool* kept, hipStream_t stream);
// room in b->tile_recs_hist for the counts of n_total kept records; false: no room -- the first pass counts for itself
KATOME_INTERNAL bool reserve_tile_hist(katome_builder* b, uint64_t n_total, uint32_t sort_tile, bool keep, hipStream_t stream);
// n tagged records (key + tag; d_counts: their weights, nullptr = 1 each) back into keys and pairs of numbers, and into `table`.
// spent: the buffer that holds d_tagged, given up between the two steps
KATOME_INTERNAL int insert_tagged(katome_builder* b, Table& table, bool& ready, uint32_t nw, uint64_t hint, const uint64_t* d_tagged,
                                  const uint32_t* d_counts, uint64_t n, int phase, hipStream_t stream, DevBuf* spent = nullptr);

// ---- count_routes.hip: katome_dev_edges, its routes and their knobs --------------------------------------------------------------
// the tile records kept aside counted level by level by sorting, down to the (k-mer, count) records of the last tile level
KATOME_INTERNAL int tile_recs_to_kmer_records(katome_builder* b, DevBuf& keys, DevBuf& weights, uint64_t* n_records, uint64_t extra_room,
                                              hipStream_t stream, DevBuf* first_counts = nullptr, bool rep = false,
                                              RecordSource* src = nullptr);      // (rep: the k-mer records in their representative orientation)
KATOME_INTERNAL int sorted_count_mode();            // KATOME_SORTED_COUNT
KATOME_INTERNAL bool sorting_pays(uint64_t n);       // n records are worth counting by sorting
KATOME_INTERNAL bool lds_route_takes(uint64_t n);    // ... and not too many for the LDS counting route
KATOME_INTERNAL int sorted_tiles_mode();            // KATOME_SORTED_TILES
KATOME_INTERNAL bool tile_recs_shape(uint32_t nwt, uint32_t nw, bool first_seen);   // tile / k-mer word counts whose levels are all counted by sorting
KATOME_INTERNAL bool sorted_fail(const char* level);     // KATOME_SORTED_FAIL (tests)
KATOME_INTERNAL bool seen_var_sorted();              // KATOME_SEEN_VAR_SORTED

// ---- what the GFA entry points (gfa.hip, gfa_strands.hip, gfa_paths.hip, gfa_strand_paths.hip, unique_contigs.hip) share -----------------------------
inline GfaGraph gfa_graph_of(uint32_t k, const ShrinkOutput& sh) {
    return GfaGraph{k, sh.n_nodes, sh.n_edges, sh.edge_src.as<u64>(), sh.edge_dst.as<u64>(), sh.edge_weight.as<u32>(), sh.edge_kmers.as<u32>(),
                    sh.edge_label_off.as<u64>(), sh.edge_label.as<uint8_t>(), sh.label_bytes};
}
// c is the result of b's last katome_dev_shrink
inline bool is_last_shrink(const katome_builder* b, const katome_dev_contigs* c) {
    const ShrinkOutput& sh = b->shrunk;
    return c->n_edges == sh.n_edges && c->n_nodes == sh.n_nodes && c->d_edge_src == sh.edge_src.as<u64>() && c->d_edge_label == sh.edge_label.as<uint8_t>() &&
           c->d_edge_label_off == sh.edge_label_off.as<u64>();
}
inline int check_label_alignment(const void* d_edge_label) {
    if ((uintptr_t)d_edge_label & 3) { set_error("gfa: d_edge_label must be 4-byte aligned (the kernel reads the aligned words around the bytes it needs)"); return KATOME_E_ARG; }
    return KATOME_OK;
}
// `bytes` of text, rounded up to 16, fit the caller's `cap` bytes at a 16-byte aligned d_text
inline bool text_fits(uint64_t bytes, uint64_t cap, const void* d_text) { return cap >= (bytes + 15) / 16 * 16 && !((uintptr_t)d_text & 15); }
// KATOME_*_TRACE of an *_arrays entry (there is no builder whose profile could hold its kernels' times): a profiler that is on where
// `env` is set, to open a PhaseScope on round the launches, and the events of the phases first .. last on stderr afterwards, one line
// each, in the form the tools/bench_gfa*.py parse
struct ArraysTrace {
    Profiler prof;
    const char* entry;
    ArraysTrace(const char* env, const char* entry_) : entry(entry_) { prof.on = getenv(env) != nullptr; }
    void print(int first_phase, int last_phase, uint64_t bytes, uint64_t n1, const char* what1, uint64_t n2, const char* what2) const {
        for (const Profiler::Ev& e : prof.evs) {
            float ms = 0;
            if (e.phase >= first_phase && e.phase <= last_phase && hipEventElapsedTime(&ms, e.a, e.b) == hipSuccess)
                fprintf(stderr, "[%s] %s %.4f ms, %llu bytes, %llu %s, %llu %s\n", entry, PHASE_NAMES[e.phase], ms, (unsigned long long)bytes, (unsigned long long)n1,
                        what1, (unsigned long long)n2, what2);
        }
    }
};

// ---- dist_gfa.hip: the k-mers on ALL ranks' merged edges of the last katome_dist_shrink (collective; katome_unitigs_gfa_*'s total_bases)
struct katome_dist_builder;
KATOME_INTERNAL int dist_gfa_total_kmers(katome_dist_builder* d, uint64_t* total, hipStream_t stream);

// ---- api.hip: what the host entry points (host_build.cpp) take from it ------------------------------------------------------------
// BFCounter input: one edge per kept line and strand; leaves the builder with its sorted edge list
KATOME_INTERNAL int bfc_set_edges(katome_builder* b, const uint64_t* d_fwd, const uint32_t* d_w, uint64_t n_lines, hipStream_t stream);
// katome_dev_collapse, also handing back every contig's length in bases (host: the walk knows them)
KATOME_INTERNAL int builder_collapse(katome_builder* b, uint32_t layout, katome_dev_assembly* out, katome_collapse_stats* stats,
                                     std::vector<uint64_t>* lengths, hipStream_t stream);
// one tile span for reads of several lengths (none shorter than k), by katome_tile_plan's charges; 1: no tiles
KATOME_INTERNAL uint32_t tile_span_for_lengths(uint32_t k, const uint32_t* len, uint64_t n_reads, uint64_t total_windows);
