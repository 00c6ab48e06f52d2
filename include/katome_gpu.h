/*
 * katome_gpu.h -- C ABI of the MI355X-native replacement for katome's `build` stage.
 *
 * Drop-in boundary: `Build::create(input_files, ft, reverse_complement, minimal_weight_threshold)
 * -> (Self, usize)` (reference src/katome/algorithms/builder.rs:42-54), called by
 * `BasicAsm::assemble` / `assemble_with_gir` (asm/basic_assembler.rs:22-26, 37-40) after
 * `set_global_k_sizes(config.k_mer_size)` (basic_assembler.rs:19-21, prelude.rs:34-43).
 * A Rust `GpuGIR` type binds these symbols with `extern "C"` and implements
 * `Convert<GpuGIR> for PtGraph` (collections/girs/mod.rs:16-29) from the arrays of `katome_graph`.
 *
 * Plain pointers and sizes only; nothing unwinds across the boundary (the reference panics:
 * builder.rs:62,67,71,124,148,153, pt_graph.rs:278 -- here every entry returns a status code and
 * `katome_last_error()` holds the message the reference would have panicked with).
 *
 * Threading: synchronous, one build at a time per process (the reference keeps k in `static mut`
 * globals, prelude.rs:21-25); the library uses HIP streams internally.
 */
#ifndef KATOME_GPU_H
#define KATOME_GPU_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KATOME_ABI_VERSION 2

/* settings.flags.  FIRST_SEEN_ORDER: number edges and nodes exactly as the reference's sequential loop does --
 * petgraph edge indices in the order `add_edge` is first called for them, node indices in the order `add_node`
 * is (pt_graph.rs:149,194) -- instead of by packed key.  Downstream stages that walk petgraph's adjacency
 * (pruner.rs:241, collapser.rs:120) then see the same graph, index for index.  Costs two extra atomics per
 * counted record and two more sorts at the end; one GPU (reads of unequal length go through the general
 * one-record-per-window route).                                                                     */
#define KATOME_FLAG_FIRST_SEEN_ORDER 1u
/* REMOVE_DEAD_PATHS (host entries katome_build_*): run Prunable::remove_dead_paths (pruner.rs:36-82) on the built
 * graph before it is handed back, as assemble() does right after the build (asm/basic_assembler.rs:58-62).  The reference's
 * walks and swap-removes depend on petgraph's numbering, so this needs FIRST_SEEN_ORDER as well (KATOME_E_ARG
 * otherwise); the result then equals the reference's pruned PtGraph index for index.                      */
#define KATOME_FLAG_REMOVE_DEAD_PATHS 2u
/* n_devices > 1 only: all ranks of the sharded build run on settings.device (peer copies instead of RCCL, which refuses two
 * ranks on one GPU).  Exercises the whole multi-GPU route -- sharding, routing, exchanges, global numbering -- on a
 * one-GPU box; no performance meaning.                                                                       */
#define KATOME_FLAG_RANKS_SHARE_DEVICE 4u
/* katome_unitigs_gfa_files / katome_unitigs_gfa_packed only (every other entry ignores it, as unknown flag bits are ignored): the
 * shrink is katome_dev_shrink_coverage(FAST) and the text katome_dev_contigs_gfa_coverage's -- KC is the SUM of the unitig's
 * k-mer counts and every S line ends in mn / mx.  With settings.n_devices > 1: katome_dist_shrink_coverage and
 * katome_dist_contigs_gfa_coverage.                                                                              */
#define KATOME_FLAG_PATH_COVERAGE 8u

/* status codes: the reference's panics, one code each */
enum {
    KATOME_OK = 0,
    KATOME_E_PATH = -1,        /* builder.rs:62  "Coulndt resolve path: ..."            */
    KATOME_E_IS_DIR = -2,      /* builder.rs:67  "... is a directory"                   */
    KATOME_E_NOT_EXIST = -3,   /* builder.rs:71  "... does not exist"                   */
    KATOME_E_OPEN = -4,        /* builder.rs:124,148 "Couldn't open all files: ..."     */
    KATOME_E_PARSE = -5,       /* builder.rs:128,153 record `.unwrap()` on a bad record */
    KATOME_E_SHORT_READ = -6,  /* pt_graph.rs:278 / hm_gir.rs:40 "Read is too short!"   */
    KATOME_E_ARG = -7,         /* prelude.rs:35 `assert!(k_size > 1)`, bad settings     */
    KATOME_E_DEVICE = -8,      /* no usable MI355X / HIP error: there is NO CPU fallback */
    KATOME_E_OOM = -9,
    KATOME_E_UNSUPPORTED = -10
};

/* Config<P> (config.rs:18-37) + prelude globals, as a plain struct */
typedef struct {
    uint32_t k;                  /* k_mer_size; supported 3..63 (k<=31: 64-bit keys, else 128-bit) */
    uint8_t  file_type;          /* InputFileType (config.rs:5-14): 0 Fasta, 1 Fastq, 2 BFCounter   */
    uint8_t  reverse_complement; /* Config::reverse_complement                                     */
    uint16_t flags;              /* KATOME_FLAG_*                                                   */
    uint32_t min_weight;         /* minimal_weight_threshold (BFCounter ingest only, builder.rs:106)*/
    int32_t  device;             /* HIP device ordinal of the (first) MI355X to build on             */
    uint64_t table_slots_hint;   /* 0 = size the (k-1)-mer/edge table automatically (whole build)   */
    /* GPUs of this node to build on: 0 or 1 = settings.device alone; n > 1 = devices device .. device+n-1,
     * one host thread and one rank per GPU INSIDE this call, reads sharded by index, records routed to their owners over
     * RCCL (katome_build_files / katome_build_packed; fixed-length reads -- other inputs are built on `device` alone).
     * The result does not depend on n in FIRST_SEEN_ORDER (the reference's numbering); by packed key, edges and nodes
     * come rank by rank (every rank's in ascending order).                                                   */
    int32_t  n_devices;
    uint32_t _reserved;
} katome_settings;

/* Result of a build, host memory, owned by the library until katome_graph_free().
 * What `Convert<GpuGIR> for PtGraph` needs (pt_graph.rs:33): node count, and per edge
 * (source, target, weight, label) with the label in compress_edge format (compress.rs:250-271),
 * i.e. what SEQUENCES[EdgeSlice.idx()] holds after PtGraph::create (pt_graph.rs:339-343).
 * Edge order = ascending packed k-mer.  Node ids (deterministic): the nodes that have out-edges in
 * ascending packed-(k-1)-mer order, then the nodes without out-edges in ascending order.
 * With KATOME_FLAG_FIRST_SEEN_ORDER: edges and nodes in the reference's own (first-seen) order.    */
typedef struct {
    uint64_t n_nodes, n_edges;
    uint64_t read_bytes;          /* sum of accepted read lengths (builder.rs:158)              */
    uint32_t k;
    uint32_t key_words;           /* u64 words per key: 1 (k<=31) or 2                          */
    uint32_t label_stride;        /* 1 + ceil(k/4)                                              */
    uint32_t _pad;
    const uint64_t *edge_src;     /* [n_edges] dense node id of the source (k-1)-mer            */
    const uint64_t *edge_dst;     /* [n_edges] dense node id of the target (k-1)-mer            */
    const uint32_t *edge_weight;  /* [n_edges] EdgeWeight = u32 (prelude.rs:9), wrapping        */
    const uint8_t  *edge_label;   /* [n_edges][label_stride] compress_edge format               */
    const uint64_t *edge_key;     /* [n_edges][key_words] packed k-mer, right-aligned, w[0] = high word */
    const uint64_t *node_key;     /* [n_nodes][key_words] packed (k-1)-mer, right-aligned       */
    /* FIRST_SEEN_ORDER graphs after remove_dead_paths / remove_weak_edges (NULL otherwise: age == index): the
     * first-seen index every edge had BEFORE the removals re-numbered it.  petgraph's swap_remove re-labels edges but
     * keeps every adjacency list in insertion order, so the reference's graph at this point is "these indices, lists
     * ordered by age" (first_edge = the live edge with the largest age); see INTEGRATION.md                    */
    const uint32_t *edge_age;
} katome_graph;

/* CollectionStats (stats/collections.rs:38-57) as computed for PtGraph (137-168) */
typedef struct {
    uint64_t node_count, edge_count;
    uint32_t max_edge_weight;
    uint32_t _pad;
    double   avg_edge_weight;
    uint64_t max_in_degree, max_out_degree;
    double   avg_out_degree;
    uint64_t incoming_vert_count, outgoing_vert_count;
} katome_stats;

/* ---- the drop-in entry points --------------------------------------------------------- */

/* Build::create over files (builder.rs:42-54 -> check_files 57-77 -> create_fastq 142-165 /
 * create_fasta 118-140): parse, skip reads with a non-ACGT byte, pack 2 bits/base, build on
 * the GPU, copy the graph back. */
int katome_build_files(const katome_settings *s, const char *const *paths, size_t n_paths,
                       katome_graph **out);
/* the build followed by stages of assemble_with_graph (asm/basic_assembler.rs:58-72), on the device, in the order
 * `stages` names them: 'd' Prunable::remove_dead_paths, 'c' Standardizable::standardize_contigs, 'w'
 * Clean::remove_weak_edges(settings.min_weight), 'e' standardize_edges(original_genome_length, k, settings.min_weight).
 * "dcwced" is everything the reference does before collapse().  Needs KATOME_FLAG_FIRST_SEEN_ORDER; the result carries
 * edge_age (see katome_graph).                                                                              */
int katome_build_files_staged(const katome_settings *s, const char *const *paths, size_t n_paths, const char *stages,
                              uint64_t original_genome_length, katome_graph **out);

/* Same build from reads that are already 2-bit packed (A0 C1 G2 T3, 4 bases per byte, first
 * base in the two most significant bits: the bit order of compress_node, compress.rs:55-73).
 * Read r occupies bytes [r*ceil(read_len/4), +ceil(read_len/4)).  `skip` (nullable) has one
 * byte per read; non-zero = the read held a non-ACGT byte and is not added (builder.rs:155-157).
 * read_len < k is KATOME_E_SHORT_READ (pt_graph.rs:278). */
int katome_build_packed(const katome_settings *s, const uint8_t *packed, uint64_t n_reads,
                        uint32_t read_len, const uint8_t *skip, katome_graph **out);
/* katome_build_packed followed by the stages of katome_build_files_staged.  With settings.n_devices > 1 they run on the
 * sharded graph when KATOME_DIST_STAGES=sharded is set or when the graph cannot be gathered (2^32 edges or nodes and more),
 * else on the graph gathered to the first GPU (KATOME_DIST_STAGES=gather forces that); the same holds for
 * katome_build_files_staged.  On the sharded route the KATOME_FLAG_REMOVE_DEAD_PATHS pruning runs sharded as well, whatever
 * KATOME_DIST_PRUNE says (a gathered graph cannot go back to the shares).  katome_graph.edge_age is 32 bits wide: after a
 * stage that may remove edges, a surviving edge aged 2^32 or more makes the copy-out fail with KATOME_E_UNSUPPORTED; such a
 * graph is read through katome_dist_* (katome_dist_graph.d_edge_age is 64-bit). */
int katome_build_packed_staged(const katome_settings *s, const uint8_t *packed, uint64_t n_reads, uint32_t read_len,
                               const uint8_t *skip, const char *stages, uint64_t original_genome_length, katome_graph **out);
/* The two staged entries that also describe the graph where assemble_with_graph logs it (graph.log_stats(),
 * asm/basic_assembler.rs:58-75 -> stats/collections.rs:137-168), computed on the device before anything is copied out:
 * stage_stats is the caller's array of strlen(stages) + 1 entries (NULL: KATOME_E_ARG); entry 0 is the graph as built, after
 * the pruning KATOME_FLAG_REMOVE_DEAD_PATHS asks for, entry i the graph after the i-th letter of `stages`.  With "dcwced" and
 * no flag, entries 0, 1, 3, 5 and 6 are the reference's five lines.  `stages` NULL or empty: entry 0 alone, and a packed-key
 * build is taken as well (stats need no numbering).  With settings.n_devices > 1 the numbers come from whichever route the
 * build takes: katome_dist_graph_stats on the shares (rank 0 writes the array) or katome_dev_graph_stats on the gathered
 * graph.  Everything else as for the staged entries above. */
int katome_build_files_staged_stats(const katome_settings *s, const char *const *paths, size_t n_paths, const char *stages,
                                    uint64_t original_genome_length, katome_stats *stage_stats, katome_graph **out);
int katome_build_packed_staged_stats(const katome_settings *s, const uint8_t *packed, uint64_t n_reads, uint32_t read_len,
                                     const uint8_t *skip, const char *stages, uint64_t original_genome_length,
                                     katome_stats *stage_stats, katome_graph **out);

void katome_graph_free(katome_graph *g);

/* Stats<CollectionStats>::stats for the built graph (stats/collections.rs:137-168); host side */
int katome_graph_stats(const katome_graph *g, katome_stats *out);

/* message of the last failing call on this thread's process (what the reference panics with) */
const char *katome_last_error(void);

uint32_t katome_abi_version(void);

/* ---- host ingest alone (the step in front of the path; builder.rs:57-77,118-165) -------- */
typedef struct {
    uint64_t n_records;       /* records seen                                              */
    uint64_t n_reads;         /* accepted (all-ACGT) reads                                 */
    uint64_t read_bytes;      /* sum of accepted read lengths                              */
    uint64_t packed_bytes;
    uint64_t total_windows;   /* sum over reads of (len - k + 1)                           */
    uint32_t fixed_len;       /* != 0 iff every accepted read has this length              */
    uint32_t _pad;
    const uint8_t  *packed;   /* reads packed back to back, each starting on a byte        */
    const uint64_t *byte_off; /* [n_reads+1] start byte of each read in `packed`           */
    const uint32_t *len;      /* [n_reads] bases                                           */
} katome_reads;

int  katome_ingest_files(const katome_settings *s, const char *const *paths, size_t n_paths,
                         katome_reads **out);
void katome_reads_free(katome_reads *r);

/* ---- device-resident API -----------------------------------------------------------------
 * Used by bench.py (inputs already in HBM when the timed region starts) and by the multi-GPU
 * driver (one process per GPU; the k-mer exchange between extraction and insertion is an RCCL
 * all-to-all done by the caller).  All `d_` pointers are device pointers on settings.device;
 * `stream` is a hipStream_t (NULL = the default stream).  Calls are asynchronous on `stream`
 * unless they return a count.                                                              */
typedef struct katome_builder katome_builder;

int  katome_builder_create(const katome_settings *s, katome_builder **out);
void katome_builder_destroy(katome_builder *b);

/* optional per-phase timing with HIP events recorded on the caller's stream (bench.py's roofline
 * figures).  total_ms / launches have katome_phase_count() entries, named by katome_phase_name():
 * extract, region_order, insert, emit_edges, sort_edges, node_set, rank, labels, insert_tiles,
 * expand_tiles, expand_mid_tiles, first_seen_order ... (new names are appended: an index keeps its name).  Reading
 * synchronises the device and clears the record.                                            */
int  katome_builder_profile(katome_builder *b, int enable);
int  katome_builder_profile_read(katome_builder *b, double *total_ms, uint64_t *launches);
/* same, plus work[i] = elements processed by the launches of entry i (the per-kernel entries "k:...": keys of a sort pass,
 * slots of a table scan ...), so that launches of different sizes add up to one rate                              */
int  katome_builder_profile_read_work(katome_builder *b, double *total_ms, uint64_t *launches, uint64_t *work);
uint32_t katome_phase_count(void);
const char *katome_phase_name(uint32_t phase);

/* sizes seen by the last katome_dev_edges/finalize: out8 = {distinct tiles, tile-table slots, distinct stored
 * k-mers (one per strand pair when reverse_complement), k-mer-table slots, distinct mid tiles, mid-tile-table
 * slots, tile span, mid-tile span (0 = tiles expand straight into k-mers)}                          */
int  katome_builder_counts(katome_builder *b, uint64_t *out8);

/* u64 words per k-mer record for this k (1 or 2) */
uint32_t katome_record_words(uint32_t k);

/* k-mer extraction (compress_kmer / compress_kmer_with_rev_compl, compress.rs:18-48, over
 * read.windows(K), pt_graph.rs:294,310): one record per forward window, record =
 * packed k-mer (reverse_complement=0) or min(k-mer, reverse complement) (=1);
 * windows of skipped reads hold the invalid marker (all ones).
 * d_records: [n_reads*(read_len-k+1)][record_words] u64.                                   */
int katome_dev_extract_fixed(katome_builder *b, const uint8_t *d_packed, uint64_t n_reads,
                             uint32_t read_len, const uint8_t *d_skip, uint64_t *d_records,
                             void *stream);
/* variable-length reads: d_byte_off[n_reads+1], d_len[n_reads], d_win_prefix[n_reads+1]
 * (exclusive prefix sum of len-k+1); d_records: [total_windows][record_words]              */
int katome_dev_extract_var(katome_builder *b, const uint8_t *d_packed, uint64_t packed_bytes,
                           const uint64_t *d_byte_off, const uint32_t *d_len,
                           const uint64_t *d_win_prefix, uint64_t n_reads, uint64_t total_windows,
                           uint64_t *d_records, void *stream);

/* variable-length reads counted as tiles: with one span for the whole batch, read r yields (len_r-k+1)/span whole tiles
 * from its front (extract_var_tiles: d_tile_prefix[n_reads+1] = tiles before each read; records of
 * katome_tile_words(k, span) words, to katome_dev_insert_tiles) and its (len_r-k+1) mod span trailing windows as plain
 * k-mer records (extract_var_remainder: d_rest_prefix likewise; to katome_dev_insert, which also closes the batch --
 * call it even when total_rest is 0 on a FIRST_SEEN_ORDER builder).  d_win_prefix / total_windows as above.          */
int katome_dev_extract_var_tiles(katome_builder *b, const uint8_t *d_packed, uint64_t packed_bytes,
                                 const uint64_t *d_byte_off, const uint32_t *d_len, const uint64_t *d_tile_prefix,
                                 const uint64_t *d_win_prefix, uint64_t n_reads, uint64_t total_tiles,
                                 uint64_t total_windows, uint32_t span, uint64_t *d_records, void *stream);
int katome_dev_extract_var_remainder(katome_builder *b, const uint8_t *d_packed, uint64_t packed_bytes,
                                     const uint64_t *d_byte_off, const uint32_t *d_len, const uint64_t *d_rest_prefix,
                                     const uint64_t *d_win_prefix, uint64_t n_reads, uint64_t total_rest,
                                     uint64_t total_windows, uint32_t span, uint64_t *d_records, void *stream);

/* group records of `key_words` (1..3) u64 words by owner rank = mulhi(mix(key), n_parts) (stable; invalid records are
 * dropped); optional u32 values travel with their records (both d_values and d_values_out, or neither).
 * d_out: same size as d_records; h_counts[n_parts] receives the records per part (synchronises)       */
int katome_dev_partition(int device, const uint64_t *d_records, const uint32_t *d_values, uint64_t n_records,
                         uint32_t key_words, uint32_t n_parts, uint64_t *d_out, uint32_t *d_values_out,
                         uint64_t *h_counts, void *stream);
/* same, with the owner taken from the key's CORE instead of the whole key: the `core_bases` bases that end
 * `core_shift` bits above the key's low end, canonically (smaller of the core and its reverse complement):
 * owner = mulhi(mix(canonical core), n_parts).  The multi-GPU build routes k-mers with (core_shift 2, core k-2) --
 * the middle (k-2)-mer, which a k-mer shares with its reverse complement and with its source node's tail -- and
 * (k-1)-mer nodes with (0, k-2), so that every out-edge of a node, in either orientation's bookkeeping, lives on
 * the rank that owns the node (the HmGIR shape, hm_gir.rs:91-153: a node and its <= 4 out-edges in one place). */
int katome_dev_partition_core(int device, const uint64_t *d_records, const uint32_t *d_values, uint64_t n_records,
                              uint32_t key_words, uint32_t core_shift, uint32_t core_bases, uint32_t n_parts,
                              uint64_t *d_out, uint32_t *d_values_out, uint64_t *h_counts, void *stream);
/* host helper: the owner the two calls above compute for one key (core_bases 0 = whole key) */
uint32_t katome_key_owner(const uint64_t *key, uint32_t key_words, uint32_t core_shift, uint32_t core_bases,
                          uint32_t n_parts);

/* add_single_edge_fastaq (pt_graph.rs:172-198) for a batch: find-or-insert each record's
 * k-mer in the open-address table and add 1 to its weight (u32, wrapping).  Grows the table
 * when needed (synchronises).                                                              */
int katome_dev_insert(katome_builder *b, const uint64_t *d_records, uint64_t n_records, void *stream);
/* same with an explicit weight per record (BFCounter input, pt_graph.rs:201-213; and merging
 * pre-aggregated partial tables)                                                           */
int katome_dev_insert_weighted(katome_builder *b, const uint64_t *d_records, const uint32_t *d_weights,
                               uint64_t n_records, void *stream);

/* Tiled counting.  The insert kernel is bound by the rate of device-scope atomics, one per window.  For
 * fixed-length reads the windows can instead be counted in TILES -- the (k+span-1)-mers that cover `span`
 * consecutive windows, (read_len-k+1)/span per read -- and every distinct tile then adds its count to its
 * span k-mers at once (same sums as `weight += 1` per window, pt_graph.rs:186-191; ~span x fewer atomics).
 * katome_tile_span: the span the library would use for these reads (1 = plain counting); spans above 16 are
 * broken into mid tiles first (two levels of the same expansion).
 * Records of katome_dev_extract_tiles: [n_reads*((read_len-k+1)/span)][katome_tile_words(k, span)] u64 (whole tiles only).
 * Tiles are expanded into the k-mer table by katome_dev_edges / katome_dev_finalize; the multi-GPU
 * driver takes them out with katome_dev_expand_tiles as (k-mer, weight) records (library-owned, valid until
 * the next insert) and routes those to the k-mers' owners (katome_dev_insert_weighted).            */
uint32_t katome_tile_span(uint32_t k, uint32_t read_len);
uint32_t katome_tile_words(uint32_t k, uint32_t span);
/* Reads whose window count is not a multiple of a useful span (101 bp at k = 31: 71 windows) are counted as
 * *tiles from the front plus the windows that are left over*: katome_tile_plan picks the span with the fewest table
 * insertions per read (71 windows: 5 tiles of 14 + 1 single window = 6 instead of 71) and returns 1 if tiling
 * pays; katome_dev_extract_tiles then yields `tiles` records per read and katome_dev_extract_remainder the
 * `remainder` trailing windows of every read as plain k-mer records ([n_reads*remainder][katome_record_words(k)]),
 * to be passed to katome_dev_insert right after the tiles of the same batch.                          */
uint32_t katome_tile_plan(uint32_t k, uint32_t read_len, uint32_t *span, uint32_t *tiles, uint32_t *remainder);
/* same with tiles of at most max_tile_words u64 words (1: 31 bases, 2: 63, 3: 95 -- three-word tiles are what lets
 * k = 63 be tiled at all; katome_tile_plan = limit 3; the multi-GPU route, whose partition passes take one- and
 * two-word records, asks for 2)                                                                          */
uint32_t katome_tile_plan_limited(uint32_t k, uint32_t read_len, uint32_t max_tile_words, uint32_t *span,
                                  uint32_t *tiles, uint32_t *remainder);
/* the same plan for reads of several lengths (host array `len`, none shorter than k): the one span katome_build_files uses
 * for the whole input -- tiles from the front of every read + the windows left over; 1: tiling does not pay             */
uint32_t katome_tile_span_for_lengths(uint32_t k, const uint32_t *len, uint64_t n_reads);
int katome_dev_extract_remainder(katome_builder *b, const uint8_t *d_packed, uint64_t n_reads, uint32_t read_len,
                                 uint32_t span, const uint8_t *d_skip, uint64_t *d_records, void *stream);
int katome_dev_extract_tiles(katome_builder *b, const uint8_t *d_packed, uint64_t n_reads, uint32_t read_len,
                             uint32_t span, const uint8_t *d_skip, uint64_t *d_records, void *stream);
int katome_dev_insert_tiles(katome_builder *b, const uint64_t *d_records, uint64_t n_records, uint32_t span,
                            void *stream);
/* katome_dev_extract_tiles + katome_dev_insert_tiles in one call, without a record buffer of the caller's: one batch of reads
 * of one length counted as tiles (add_read_fastaq's windows, pt_graph.rs:277-315, `span` at a time).  When the builder keeps tile
 * records aside to count them by sorting (by packed key, tiles of two words) and no read is skipped (d_skip == NULL), the records
 * are written where they are kept.  The windows behind a read's last whole tile still go through
 * katome_dev_extract_remainder + katome_dev_insert.                                                        */
int katome_dev_count_tiles(katome_builder *b, const uint8_t *d_packed, uint64_t n_reads, uint32_t read_len,
                           uint32_t span, const uint8_t *d_skip, void *stream);
int katome_dev_expand_tiles(katome_builder *b, uint64_t **d_keys, uint32_t **d_weights, uint64_t *n_records,
                            void *stream);

/* Clean::remove_weak_edges(threshold) for PtGraph (pruner.rs:84-93): keep the edges with weight >= threshold,
 * then drop the vertices left without neighbours.  Call before katome_dev_edges / katome_dev_finalize: the
 * filter is applied when the edges are read out of the table, so the sort and the node numbering only see
 * the surviving edges (and the nodes are exactly their endpoints).
 * FIRST_SEEN_ORDER builders instead number the whole graph first and then remove as petgraph's retain_edges /
 * retain_nodes do (indices visited in descending order, rejected ones swap_removed), so the result keeps the
 * reference's numbering; on such a builder the call is also accepted AFTER katome_dev_finalize (e.g. after
 * katome_dev_remove_dead_paths, the order of asm/basic_assembler.rs:58-66) and then acts at once.       */
int katome_dev_remove_weak_edges(katome_builder *b, uint32_t threshold, void *stream);

/* number of distinct keys in the table so far (synchronises) */
int katome_dev_table_count(katome_builder *b, uint64_t *out, void *stream);

/* device-resident graph; arrays owned by the builder until destroy / next finalize */
typedef struct {
    uint64_t n_nodes, n_edges;
    uint32_t key_words, label_stride;
    uint64_t *d_edge_key;     /* [n_edges][key_words], ascending */
    uint32_t *d_edge_weight;
    uint64_t *d_edge_src, *d_edge_dst;
    uint8_t  *d_edge_label;
    uint64_t *d_node_key;     /* [n_nodes][key_words]: sources ascending, then out-edge-less nodes ascending */
    uint32_t *d_edge_age;     /* see katome_graph.edge_age; NULL while age == index */
} katome_dev_graph;

/* Table -> distinct oriented edges, sorted by packed k-mer (both strands when
 * reverse_complement, pt_graph.rs:282-308); then node numbering, endpoints and labels
 * (the PtGraph::create post-pass, pt_graph.rs:339-343 -> kmer_to_edge compress.rs:231-233). */
int katome_dev_finalize(katome_builder *b, katome_dev_graph *out, void *stream);

/* Prunable::remove_dead_paths for PtGraph (pruner.rs:36-82; Externals 165-195, remove_paths 199-217,
 * check_dead_path 229-257), in place on the finalized graph of a FIRST_SEEN_ORDER builder: call after
 * katome_dev_finalize; `graph` is updated (counts shrink, labels are rewritten).  Everything runs on the device:
 * the walks, the degree bookkeeping, the two swap_remove replays that fix petgraph's re-numbering (edges: a scan
 * + pointer jumping; nodes: the vacated tail positions settled in rounds) and the array moves.  Only a pass whose
 * node moves chain further than the device form follows is replayed sequentially on the host (see prune.hip).  */
typedef struct {
    uint64_t passes;                 /* iterations of the reference's outer loop, the last (empty) one included */
    uint64_t walks, dead_walks;      /* walks started from vertices without incoming edges / walks found dead   */
    uint64_t marked;                 /* edge indices collected, duplicates counted                              */
    uint64_t removed_edges, removed_by_duplicates, removed_nodes;
    double   host_ms;                /* time in sequential host replays (0 unless a pass fell back to them)     */
    double   total_ms;
} katome_prune_stats;
int katome_dev_remove_dead_paths(katome_builder *b, katome_dev_graph *graph, katome_prune_stats *stats, void *stream);

/* the finalized graph as it stands now (after katome_dev_remove_dead_paths / katome_dev_remove_weak_edges) */
int katome_dev_current_graph(katome_builder *b, katome_dev_graph *out);
/* Stats<CollectionStats>::stats for PtGraph (stats/collections.rs:137-168) and the weight spectrum (see
 * katome_dev_weight_spectrum_arrays) of the finalized graph as it stands, in either numbering, after any of
 * katome_dev_remove_dead_paths, katome_dev_remove_weak_edges and katome_dev_standardize_*: what graph.log_stats() prints
 * at that point (asm/basic_assembler.rs:58-75), without copying the graph out.  Nothing in the builder changes.  Before
 * katome_dev_finalize: KATOME_E_ARG.  Both synchronise.  Profile phases "graph_stats" and "weight_spectrum". */
int katome_dev_graph_stats(katome_builder *b, katome_stats *out, void *stream);
int katome_dev_weight_spectrum(katome_builder *b, uint64_t *bins /* host, [n_bins] */, uint32_t n_bins, void *stream);

/* Standardizable for PtGraph (standardizer.rs:41-128), the two weight passes assemble_with_graph runs between its
 * prunings (asm/basic_assembler.rs:63-70), in place on the finalized graph as it stands:
 *  - standardize_contigs (72-122): every contig -- an out-edge of an ambiguous vertex (pt_graph.rs:54-62) followed while
 *    the vertex reached has one out-edge and is not ambiguous -- gets the rounded mean of its weights; no re-numbering;
 *  - standardize_edges (42-70): weights scaled by (original_genome_length - k) / (sum of weights - sum of the weights
 *    under `threshold`), rounded, then remove_weak_edges(1) (same numbering rules as katome_dev_remove_weak_edges).
 * With katome_dev_remove_dead_paths / katome_dev_remove_weak_edges this covers every stage of the reference up to
 * `collapse`, index for index on a FIRST_SEEN_ORDER builder (fetch the arrays with katome_dev_current_graph).      */
int katome_dev_standardize_contigs(katome_builder *b, void *stream);
int katome_dev_standardize_edges(katome_builder *b, uint64_t original_genome_length, uint32_t threshold, void *stream);

/* host result of katome_shrink_files / katome_shrink_packed: the build (with the pruning the flags ask for) followed by
 * Shrinkable::shrink, see katome_dev_shrink below for what the arrays mean.  Owned by the library until katome_contigs_free.
 * With settings.n_devices > 1 a FIRST_SEEN_ORDER build is gathered to one GPU and shrunk there (KATOME_SHRINK_AUTO); with
 * KATOME_DIST_SHRINK=sharded a build in either numbering is shrunk on the sharded graph (katome_dist_shrink, the fast form;
 * edges in the order of their head edges, nodes by new id), KATOME_DIST_SHRINK=gather gathers and runs the fast form. */
typedef struct {
    uint64_t n_nodes, n_edges, label_bytes, read_bytes;
    uint32_t k, key_words;
    const uint64_t *edge_src, *edge_dst;       /* [n_edges] ids into node_key                                  */
    const uint32_t *edge_weight, *edge_kmers;  /* weight of the path's first k-mer; k-mers merged into the edge  */
    const uint64_t *edge_label_off;            /* [n_edges + 1] byte offsets into edge_label                    */
    const uint8_t  *edge_label;                /* compress_edge format, edge i = bytes [off[i], off[i+1])        */
    const uint64_t *node_key;                  /* [n_nodes][key_words] packed (k-1)-mers                         */
} katome_contigs;
int  katome_shrink_files(const katome_settings *s, const char *const *paths, size_t n_paths, katome_contigs **out);
int  katome_shrink_packed(const katome_settings *s, const uint8_t *packed, uint64_t n_reads, uint32_t read_len,
                          const uint8_t *skip, katome_contigs **out);
void katome_contigs_free(katome_contigs *c);

/* Shrinkable::shrink for PtGraph (shrinker.rs:165-209; labels merged as EdgeSlice::merge does, slices.rs:23-34) on
 * the finalized graph as it stands: every maximal straight path (inner vertices with exactly one edge in and one out)
 * becomes ONE edge spelling the whole path, with the weight of the path's first edge (shrinker.rs:181,200); the inner
 * vertices disappear (remove_single_vertices, shrinker.rs:172).  The graph of the builder is left untouched; the
 * result is a separate set of device arrays owned by the builder (valid until the next call or destroy):
 *   d_edge_label: the paths in compress_edge format (compress.rs:250-271: [pad][packed bases, left-aligned]), edge i
 *   at bytes [d_edge_label_off[i], d_edge_label_off[i+1]); d_edge_kmers[i] = k-mers merged into edge i.
 * Two forms (katome_dev_shrink_mode):
 *  - KATOME_SHRINK_EXACT: the reference's own result -- where ShrinkTraverse (shrinker.rs:62-135) cuts paths on tangled graphs
 *    and cycles, and the edge / node indices petgraph's swap_removes and add_edges leave (shrink_single_path 178-209,
 *    remove_single_vertices) -- index for index.  That order is a sequential depth-first traversal interleaved with the
 *    mutation, so it is computed on one host core over petgraph's own layout (csrc/shrink_exact.h; *host_ms reports it);
 *    adjacency order (edge ages) before and weights, k-mer counts and labels after are the device's.
 *  - KATOME_SHRINK_FAST: everything on the device, traversal-free: the same SET of merged edges wherever the reference's
 *    traversal starts from a vertex without incoming edges, cycles of inner vertices cut at their smallest vertex; numbering
 *    = edges in the order of their first k-mer in the input graph, vertices in their input order.
 *  - KATOME_SHRINK_AUTO (katome_dev_shrink): exact on a FIRST_SEEN_ORDER builder, fast otherwise. */
#define KATOME_SHRINK_AUTO  0u
#define KATOME_SHRINK_FAST  1u
#define KATOME_SHRINK_EXACT 2u
typedef struct {
    uint64_t  n_nodes, n_edges, label_bytes;
    uint32_t  key_words, _pad;
    uint64_t *d_edge_src, *d_edge_dst;
    uint32_t *d_edge_weight, *d_edge_kmers;
    uint64_t *d_edge_label_off;
    uint8_t  *d_edge_label;
    uint64_t *d_node_key;
} katome_dev_contigs;
int katome_dev_shrink(katome_builder *b, katome_dev_contigs *out, void *stream);
int katome_dev_shrink_mode(katome_builder *b, uint32_t mode, katome_dev_contigs *out, double *host_ms, void *stream);
/* Unitig coverage.  The shrunk edge carries the weight of its path's FIRST k-mer only; katome_dev_shrink_coverage is
 * katome_dev_shrink_mode(b, mode, out, host_ms, stream), array for array and in every mode, and ALSO leaves, per merged edge, what
 * the k-mer counts (edge_weight) of the input edges on its path come to: their sum in 64 bits (the graph's u32 weights may have
 * wrapped; the sum of what the graph holds does not), the smallest and the largest.  They are accumulated by the walk that
 * writes the result anyway (fast form: the label writer; exact form: the chain measure), nothing is walked twice.  A cycle of
 * inner vertices counts each of its edges once; the exact form counts the chain behind each slot, whatever the traversal's
 * cuts made of it.  No edges: zero-length arrays, KATOME_OK.  Null out or cov: KATOME_E_ARG; before katome_dev_finalize: the
 * refusal of katome_dev_shrink_mode.
 * The arrays are owned by the builder until its next shrink OF ANY KIND or destroy: a later katome_dev_shrink or
 * katome_dev_shrink_mode drops them, so a coverage can never outlive the shrink result it belongs to.  (A stage that changes
 * the graph after a shrink leaves both the result and its coverage describing the graph as it was.)                          */
typedef struct {
    uint64_t  n_edges;                 /* = the shrink result's n_edges                                        */
    uint64_t *d_kmer_sum;              /* [n_edges] sum of the input edges' weights on the path                */
    uint32_t *d_kmer_min, *d_kmer_max; /* [n_edges] their smallest / largest                                   */
} katome_dev_coverage;
int katome_dev_shrink_coverage(katome_builder *b, uint32_t mode, katome_dev_contigs *out, katome_dev_coverage *cov,
                               double *host_ms, void *stream);

/* ---- depth of any sequence against the graph (csrc/depth.hip) ---------------------------------------------------------------------
 * Every window of every query sequence is looked up among the edges of the finalized graph AS IT STANDS NOW -- after whichever
 * stages have run, in either numbering -- and reduced per sequence; no record array is made in between.
 * Query: n_seqs sequences in d_seq (seq_bytes bytes); sequence s starts at byte d_byte_off[s] ([n_seqs]) and has d_len[s] bases.
 *   KATOME_DEPTH_PACKED: 2-bit packed, 4 bases per byte, every sequence starting on a byte (katome_dev_extract_var's input);
 *   KATOME_DEPTH_ASCII:  one byte per base; upper-case A, C, G, T are bases, EVERY other byte (N, lower case, a newline) is not.
 * Windows: sequence s has max(0, len_s - k + 1) of them; one shorter than k has none and is not an error.  d_seq_window_off is the
 *   exclusive prefix of those counts ([n_seqs + 1]); window w of the call belongs to the sequence whose range holds w.
 * A window's k-mer is looked up as spelled.  (A reverse-complement build holds both strands as edges: the forward lookup is complete.)
 *   present: the k-mer is edge e.  Value e -- the index in katome_dev_current_graph's arrays --, weight edge_weight[e] as it is now;
 *            an edge of weight 0 is still present.
 *   KATOME_DEPTH_EITHER_STRAND: a window whose k-mer is no edge but whose reverse complement is edge e is present too, with value
 *            e | KATOME_DEPTH_REVERSE and weight edge_weight[e].  A palindrome is found forward.
 *   invalid: under ASCII, a window that covers a byte other than A, C, G, T.  Counted in n_invalid / d_seq_invalid, not present,
 *            value KATOME_DEPTH_INVALID.  PACKED has none.
 *   absent:  every other window, value KATOME_DEPTH_ABSENT.
 * Per sequence: d_seq_present / d_seq_invalid count its present / invalid windows, d_seq_sum is the 64-bit sum of the present
 *   windows' weights, d_seq_min / d_seq_max the smallest / largest of them (nothing present: min = all ones, max = 0).
 * Totals: n_present, n_invalid, weight_sum are the arrays' sums; n_edges is the graph's edge count.
 * KATOME_DEPTH_WINDOWS: d_window_edge[w] is window w's value.  KATOME_DEPTH_EDGE_HITS: d_edge_hits[e] is the number of present
 *   windows OF THIS CALL whose value names e on either strand (nothing accumulates across calls), n_edges_hit the edges with a
 *   count above 0.  Without the flag the pointer is NULL (n_edges_hit 0) and the array is neither allocated nor written.
 * A graph that holds one k-mer on several edges (BFCounter input lists it so) answers with one of them.
 * Status: no sequences or no edges: well-formed zero results, KATOME_OK.  Before katome_dev_finalize, NULL out, an unknown encoding
 *   or flag bit: KATOME_E_ARG.  Offsets that do not ascend, or a sequence that runs past seq_bytes (PACKED: d_byte_off[s] +
 *   ceil(len / 4); ASCII: + len): KATOME_E_ARG naming the sequence, found on the device BEFORE anything is read through them.
 *   2^32 windows or more in one call: KATOME_E_UNSUPPORTED with the number; the caller batches.
 * Memory: the lookup keeps an index in the builder between calls -- a directory of at most n_edges / 8 eight-byte entries over the
 *   top bits of the keys and, where d_edge_key does not ascend strictly (first-seen order, or after removals), a sorted copy of the
 *   keys with the permutation back: 8 * key_words + 4 bytes per edge (katome_dev_depth_index_bytes: what it holds now).  Every call
 *   that changes the set or the order of the edges drops it (finalize, remove_dead_paths, remove_weak_edges, standardize_edges);
 *   weights are read from d_edge_weight, so standardize_contigs needs no rebuild.  A call takes 28 bytes per sequence and, when
 *   asked, 8 per window and 4 per edge.
 * The result has its own buffers, owned by the builder until its next katome_dev_depth or destroy; no other result and nothing in
 * the graph is touched.  The call synchronises.  Profile phase "depth", kernels "k:depth_kernel" and "k:depth_index".
 * Not offered: a sharded query without a gather (katome_depth_paths gathers), k outside 3..63, lower-case bases as bases.                         */
#define KATOME_DEPTH_PACKED        0u
#define KATOME_DEPTH_ASCII         1u
#define KATOME_DEPTH_EITHER_STRAND 1u   /* flags */
#define KATOME_DEPTH_WINDOWS       2u
#define KATOME_DEPTH_EDGE_HITS     4u
#define KATOME_DEPTH_ABSENT   0xFFFFFFFFFFFFFFFFull
#define KATOME_DEPTH_INVALID  0xFFFFFFFFFFFFFFFEull
#define KATOME_DEPTH_REVERSE  0x8000000000000000ull
typedef struct {
    uint64_t  n_seqs, n_windows, n_present, n_invalid, n_edges, n_edges_hit;
    uint64_t  weight_sum;
    uint64_t *d_seq_present, *d_seq_invalid, *d_seq_sum;   /* [n_seqs] */
    uint32_t *d_seq_min, *d_seq_max;                       /* [n_seqs] */
    uint64_t *d_seq_window_off;                            /* [n_seqs + 1] */
    uint64_t *d_window_edge;                               /* [n_windows] or NULL */
    uint32_t *d_edge_hits;                                 /* [n_edges]  or NULL */
} katome_dev_depth_result;             /* (C has one name space for types and functions: the struct cannot share the entry's name) */
int katome_dev_depth(katome_builder *b, uint32_t encoding, uint32_t flags, const uint8_t *d_seq, uint64_t seq_bytes,
                     const uint64_t *d_byte_off, const uint32_t *d_len, uint64_t n_seqs, katome_dev_depth_result *out, void *stream);
uint64_t katome_dev_depth_index_bytes(katome_builder *b);      /* device bytes the kept index holds now (0: none is kept) */
/* The same kernels on the caller's arrays, like the other *_arrays entries: n_edges keys (katome_record_words(k) words each) in ANY
 * order but distinct -- two equal keys are KATOME_E_ARG naming one such pair --, their weights, the query as above; the caller's
 * per-sequence arrays ([n_seqs], d_seq_window_off [n_seqs + 1]), d_window_edge (room for window_cap values; needed with
 * KATOME_DEPTH_WINDOWS, KATOME_E_ARG if the windows do not fit) and d_edge_hits ([n_edges]; needed with KATOME_DEPTH_EDGE_HITS).
 * totals: {n_windows, n_present, n_invalid, weight_sum, n_edges_hit}.  The index is built and dropped inside the call.      */
/* The same from files, with host arrays (csrc/host_build.cpp): the graph is built from the read files exactly as
 * katome_build_files_staged builds it (an empty `stages` is allowed in either numbering; stage letters need
 * KATOME_FLAG_FIRST_SEEN_ORDER), then EVERY record of the query files is queried, in file order, in ASCII, in batches under the
 * window limit.  query_file_type: 0 FASTA (a record's lines are joined) or 1 FASTQ; BFCounter (2) is KATOME_E_ARG.  The query
 * scanner drops nothing: a record with an N keeps its valid windows, one shorter than k (or empty) is a record without windows and
 * no short-read error.  A query path that is missing, a directory or unreadable gives the ingest's own status (KATOME_E_PATH ...),
 * a malformed record KATOME_E_PARSE.  flags: KATOME_DEPTH_EITHER_STRAND, KATOME_DEPTH_EDGE_HITS (edge_hits is NULL without it); the
 * result has no per-window array, so KATOME_DEPTH_WINDOWS, like an unknown bit, is KATOME_E_ARG.  Names of query records are not kept.
 * settings.n_devices > 1: the query runs on the graph gathered to the first GPU, which takes a first-seen build (the gather's own
 * rule; a packed-key build on several GPUs is KATOME_E_ARG) and one that can be gathered (else the gather's KATOME_E_UNSUPPORTED).
 * A sharded query without a gather is not offered.  Free with katome_depth_free.
 * (The entry is katome_depth_PATHS: the *_files names are the halves of the files / packed pairs, every one of which has a twin that
 * takes packed reads; a query has two sets of paths and no such twin.)                                                       */
typedef struct {
    uint64_t  read_bytes;                                  /* of the reads the graph was built from                */
    uint64_t  n_records, n_windows, n_present, n_invalid, n_edges, n_edges_hit, weight_sum;
    const uint64_t *seq_present, *seq_invalid, *seq_sum;   /* [n_records], in file order                            */
    const uint32_t *seq_min, *seq_max;                     /* [n_records]                                           */
    const uint32_t *edge_hits;                             /* [n_edges] or NULL                                     */
} katome_depth;
int  katome_depth_paths(const katome_settings *s, const char *const *read_paths, size_t n_read_paths, const char *stages,
                        uint64_t original_genome_length, const char *const *query_paths, size_t n_query_paths,
                        uint32_t query_file_type, uint32_t flags, katome_depth **out);
void katome_depth_free(katome_depth *d);
int katome_dev_depth_arrays(int device, uint32_t k, const uint64_t *d_edge_key, const uint32_t *d_edge_weight, uint64_t n_edges,
                            uint32_t encoding, uint32_t flags, const uint8_t *d_seq, uint64_t seq_bytes, const uint64_t *d_byte_off,
                            const uint32_t *d_len, uint64_t n_seqs, uint64_t *d_seq_present, uint64_t *d_seq_invalid,
                            uint64_t *d_seq_sum, uint32_t *d_seq_min, uint32_t *d_seq_max, uint64_t *d_seq_window_off,
                            uint64_t *d_window_edge, uint64_t window_cap, uint32_t *d_edge_hits, uint64_t totals[5], void *stream);

/* ---- collapse: the contigs, their text, FASTA and stats (collapser.rs:25-273, asm/mod.rs:57-72, stats/contigs.rs:31-89) --------
 * Collapsable::collapse is `self.shrink()` followed by a walk that consumes edge weights one at a time and swap-removes edges
 * and nodes as it goes: which contigs come out, and in which order, depends on petgraph's indices at every step.  As with the
 * exact shrink that order is computed on one host core over petgraph's own layout (csrc/collapse_exact.h, after
 * csrc/shrink_exact.h), which emits PIECES: piece p names the shrunk edge appended at step p (its index in the shrunk graph),
 * with KATOME_PIECE_WHOLE set on a piece that begins a contig (EdgeSlice::name(), the whole label; every other piece is
 * remainder(), the label from base k-1 on).  The number of pieces is the sum of the shrunk edges' weights.  The text is
 * written on the device (csrc/collapse.hip), partitioned by output bytes, in one of two layouts:
 *   KATOME_TEXT_PLAIN: the contigs back to back, ASCII ACGT;
 *   KATOME_TEXT_FASTA: byte for byte what Contigs::save_to_file writes: record i = ">katome_<i>\n<contig>\n".
 * d_contig_off[i] = offset of contig i's first base in d_text, d_contig_len[i] = its bases; d_text holds text_bytes bytes
 * (the buffer is a multiple of 16 bytes; what lies past text_bytes is unspecified).                                    */
#define KATOME_TEXT_PLAIN 0u
#define KATOME_TEXT_FASTA 1u
#define KATOME_PIECE_WHOLE 0x80000000u
typedef struct {
    uint64_t  n_contigs, text_bytes;
    uint32_t  layout, _pad;
    uint64_t *d_contig_off;
    uint32_t *d_contig_len;
    uint8_t  *d_text;
} katome_dev_assembly;
typedef struct {
    uint64_t n_pieces, n_contigs;
    uint64_t nodes_left, edges_left;     /* what the walk left of the graph: (0, 0)                                    */
    uint64_t steps;                      /* iterations of contigs_from_vertex's loop that appended an edge              */
    uint64_t ambiguity_cuts;             /* contigs ended at an ambiguous vertex                                        */
    uint64_t self_loops, simple_loops;   /* taken                                                                       */
    uint64_t scc_restarts;               /* starts from tarjan_scc(..).last()[0] (no vertex without incoming edges left) */
    uint64_t nodes_removed;
    uint64_t ambiguity_moves;            /* removals that copied a set ambiguity bit of the last node onto a lower index */
    uint64_t shrunk_nodes, shrunk_edges; /* the graph after the shrink collapse starts with                             */
    double   shrink_host_ms;             /* one host core: ShrinkExact                                                  */
    double   host_ms;                    /* one host core: the walk                                                     */
    double   text_ms;                    /* wall time of measuring, scanning and writing the text on the device         */
} katome_collapse_stats;
/* collapse() of the finalized graph as it stands (after finalize or any of the pruning / standardize stages), in either
 * numbering: on a by-key builder it is the reference's collapse of THAT graph (no edge ages: index order).  The exact shrink
 * inside is katome_dev_shrink_mode(KATOME_SHRINK_EXACT)'s.  The builder's graph is left untouched; the result arrays are owned
 * by the builder until its next katome_dev_collapse or destroy.  An edge of weight 0 (the reference's decrement would wrap):
 * KATOME_E_ARG.  2^31 pieces or more, or a contig of 2^32 bases or more: KATOME_E_UNSUPPORTED, with the number; pieces that do
 * not fit host memory: KATOME_E_OOM.  No edges: zero contigs, KATOME_OK.  `stats` may be NULL.  Profile phase "collapse",
 * kernel "k:text_write_kernel".  Synchronises.  The device piece list (4 bytes per piece) and the shrunk graph it names stay
 * in the builder until the next katome_dev_collapse or destroy: katome_dev_collapse_gfa below writes the contigs' paths from them. */
int katome_dev_collapse(katome_builder *b, uint32_t layout, katome_dev_assembly *out, katome_collapse_stats *stats, void *stream);
/* the text of a shrink result (fast or exact), one contig per merged edge, each its whole label: no piece list.  `contigs` is
 * what katome_dev_shrink / katome_dev_shrink_mode of this builder returned last.  Result owned by the builder until its next
 * katome_dev_contigs_text or destroy.                                                                                  */
int katome_dev_contigs_text(katome_builder *b, const katome_dev_contigs *contigs, uint32_t layout, katome_dev_assembly *out,
                            void *stream);
/* ---- the unitig graph as GFA 1 (csrc/gfa.hip): segments, links and k-mer counts ------------------------------------------
 * The text of a shrink result (n_edges merged edges over n_nodes vertices), byte for byte:
 *   H\tVN:Z:1.0\n
 *   S\t<i>\t<bases of edge i>\tLN:i:<bases>\tKC:i:<weight_i * kmers_i>\tew:i:<weight_i>\n    i = 0 .. n_edges - 1, in index order
 *   L\t<a>\t+\t<b>\t+\t<k-1>M\n                                                              every (a, b) with edge_dst[a] == edge_src[b]
 * Segment i is merged edge i, named by its decimal index: the record >katome_<i> of katome_dev_contigs_text on the same result;
 * <bases> = edge_kmers[i] + k - 1.  KC is the 64-bit product (up to 20 digits) of what the shrunk edge carries: shrink keeps only
 * the weight of a path's FIRST k-mer (shrinker.rs:181,200), so KC is that weight times the k-mers merged into the edge, not the
 * sum of the path's k-mer counts (katome_dev_contigs_gfa_coverage below writes that sum); ew is that weight itself.  Links are ordered by a, then b; a self-loop links to itself, parallel
 * merged edges are distinct segments, every orientation is + (the two strands of a reverse_complement build are separate edges
 * and therefore separate segments; katome_dev_contigs_gfa_strands below merges strand twins).  No edges: the header line alone.
 * d_text holds text_bytes bytes in a buffer that is a multiple of 16 bytes (zeros behind the text up to the next multiple);
 * d_segment_off[i] = offset of segment i's first base; the links of segment a are lines d_link_first[a] .. d_link_first[a + 1]
 * of the L region (d_link_first[n_segments] = n_links).
 * Everything the writer reads through is validated on the device first -- edge_src / edge_dst >= n_nodes, label offsets outside
 * the labels, a pad byte > 3, a label shorter than k bases or whose bases are not edge_kmers + k - 1: KATOME_E_ARG, with a
 * message.  2^32 segments or links or more (or 2^32 - 1 lines in all): KATOME_E_UNSUPPORTED, with the number.  Scratch and
 * result beyond the text are a few words per segment, per vertex and per link (DESIGN.md section 11b has the bytes), never a
 * second copy of the text.  Profile phase "gfa", kernel "k:gfa_write_kernel".  Synchronises.                              */
typedef struct {
    uint64_t  n_segments, n_links, text_bytes;
    uint8_t  *d_text;
    uint64_t *d_segment_off;             /* [n_segments]                                                               */
    uint64_t *d_link_first;              /* [n_segments + 1]                                                           */
} katome_dev_gfa;
/* `contigs` is what katome_dev_shrink / katome_dev_shrink_mode of this builder returned last, in either numbering and either
 * form.  The builder's graph and the shrink result are left untouched; the result is owned by the builder until its next
 * katome_dev_contigs_gfa or destroy.                                                                                      */
int katome_dev_contigs_gfa(katome_builder *b, const katome_dev_contigs *contigs, katome_dev_gfa *out, void *stream);
/* The same text with the unitig's coverage: only the S lines differ,
 *   S\t<i>\t<bases>\tLN:i:<bases>\tKC:i:<kmer_sum_i>\tew:i:<weight_i>\tmn:i:<kmer_min_i>\tmx:i:<kmer_max_i>\n
 * KC is the sum of the path's k-mer counts, so KC / kmers is the unitig's mean k-mer depth; ew stays the shrunk edge's weight
 * (what collapse would consume); mn / mx are the smallest and largest count on the path (lower-case: user-space tags).  Header,
 * names, L lines, ordering, d_segment_off, d_link_first, zero fill and limits are katome_dev_contigs_gfa's.
 * `contigs` must be the builder's last shrink result AND that shrink a katome_dev_shrink_coverage: KATOME_E_ARG otherwise, the
 * message says which.  The result shares katome_dev_contigs_gfa's buffers: each call invalidates the other's result
 * (katome_dev_contigs_gfa_strands keeps its own).  The bidirected writer has no coverage form: a merged segment would need a
 * rule for combining its two strands' counts, which is left open; katome_gfa_* and katome_gfa_strands_* (the gather routes)
 * are unchanged too.  The sharded form is katome_dist_contigs_gfa_coverage.                                                */
int katome_dev_contigs_gfa_coverage(katome_builder *b, const katome_dev_contigs *contigs, katome_dev_gfa *out, void *stream);

/* ---- the unitig graph as BIDIRECTED GFA 1 (csrc/gfa_strands.hip): strand twins merged into one segment, +/- links ----------
 * The same shrink result with a merged edge and its reverse complement written as ONE double-stranded segment, as GFA readers
 * model it.  twin(i) = the j whose bases are the reverse complement of edge i's, or none: j is found through its first k-mer
 * (revcomp of i's last k-mer; a k-mer lies on one merged edge, so a first k-mer names its segment) and counts only if the WHOLE
 * text agrees, base for base (after remove_dead_paths a strand's middle can differ).  twin(i) == i: a self-twin.
 * rep(i) = min(i, twin(i)), or i without a twin; o(i) = '-' where twin(i) < i, '+' otherwise (unpaired segments and self-twins too).
 * The text, byte for byte:
 *   H\tVN:Z:1.0\n
 *   S\t<r>\t<bases of edge r>\tLN:i:<bases>\tKC:i:<w_r * kmers_r>\tew:i:<w_r>[\trc:i:<j>\trw:i:<w_j>]\n   one per representative r, ascending
 *   L\t<x>\t<ox>\t<y>\t<oy>\t<k-1>M\n
 * The bracketed tags are there exactly when r has a twin j (a self-twin: j = r).  The name stays the merged edge's own index, so
 * S <r> is still the record >katome_<r> of the unitig FASTA and rc:i: names the record that was folded in; rw is the twin's weight
 * (shrink keeps the weight of a path's FIRST k-mer, which for the twin is r's last: the two generally differ).
 * Links: every (a, b) with edge_dst[a] == edge_src[b] spells (rep a, o a, rep b, o b); its conjugate spelling is
 * (rep b, flip o b, rep a, flip o a), where flip exchanges + and - but leaves a self-twin at +.  The smaller of the two under the
 * order (x, ox, y, oy) with + < - is kept, duplicates are dropped, and the lines ascend in that order: a link and its mirror are
 * one line, a hairpin (x + x -) is written once, a link whose mirror is missing is still written.  No edges: the header alone.
 * d_text as for katome_dev_gfa; d_segment_name[s] = the s-th S line's name r; d_segment_off[s] = offset of its first base; the
 * links whose x is that segment are lines d_link_first[s] .. d_link_first[s + 1] of the L region; d_edge_twin[i] = twin(i), all
 * ones for none.  n_unpaired: merged edges without a twin; n_self_twins: those that are their own.
 * Validation and limits as for katome_dev_gfa; two segments with the same first k-mer (not a shrink result): KATOME_E_ARG, with a
 * message that names one such pair.  Scratch: a few words per segment, per vertex and per link, never a
 * second copy of the text or the labels.  Profile phase "gfa_strands".  Synchronises.  The merged form of the sharded shrink
 * without a gather (katome_dist_contigs_gfa) is not offered.                                                                */
typedef struct {
    uint64_t  n_segments, n_links, text_bytes, n_unpaired, n_self_twins;
    uint8_t  *d_text;
    uint64_t *d_segment_name;            /* [n_segments]                                                               */
    uint64_t *d_segment_off;             /* [n_segments]                                                               */
    uint64_t *d_link_first;              /* [n_segments + 1]                                                           */
    uint64_t *d_edge_twin;               /* [contigs->n_edges]                                                         */
} katome_dev_gfa_strands;
/* ownership as for katome_dev_contigs_gfa; the result has its own buffers: a later katome_dev_contigs_gfa leaves it valid, and
 * this call leaves that one's.                                                                                            */
int katome_dev_contigs_gfa_strands(katome_builder *b, const katome_dev_contigs *contigs, katome_dev_gfa_strands *out, void *stream);

/* ---- the GFA of the ASSEMBLY (csrc/gfa_paths.hip): collapse's contigs as P lines over the segments of its shrunk graph --------
 * katome_dev_collapse's piece p names the shrunk edge appended at step p, and segment <i> of the GFA of that shrunk graph is that
 * edge: a contig is a path over segments.  The text is, byte for byte, what katome_dev_contigs_gfa writes for the collapse's
 * shrunk graph (H, the S lines in index order, the L lines), followed by the path region:
 *   P\tkatome_<c>\t<s0>+,<s1>+,...,<sn>+\t*\n            run 0 of contig c
 *   P\tkatome_<c>.<r>\t<s..>+,...\t*\n                    run r = 1, 2, ... of contig c
 * <c> is the contig's number (katome_<c> is its FASTA header), <s> a piece's shrunk edge index in decimal; every orientation is +
 * (the collapse runs on the two-strand graph) and the overlap column is * (the L lines carry <k-1>M).  Contigs in order, the runs
 * of a contig in order.  A contig is not always one path: when contigs_from_vertex takes a simple loop (collapser.rs:181-193) it
 * appends the entering edge b->c, the return edge c->b and continues from c, so the next piece does not start where the last one
 * ended and the two have no L line.  Piece p therefore starts a run iff it has KATOME_PIECE_WHOLE or
 * edge_dst[id(p - 1)] != edge_src[id(p)] (a jump), and n_paths = n_contigs + n_jumps.  Inside a P line every consecutive pair is
 * an L line.  Concatenated in order (the first run's first piece whole, every other piece of every run from base k-1 on), the runs
 * of contig c spell the text katome_dev_collapse writes for contig c.  No pieces: an empty region.
 * On the device the path region starts at d_path_text = d_text + text_bytes rounded up to 16, with zeros behind each part up to
 * its multiple of 16 (the two-part convention of katome_dist_gfa); in host memory and in the file the two parts are contiguous.
 * d_path_line_off[j] = offset of path j's line in the path region ([n_paths] = path_bytes), d_path_contig[j] = its contig,
 * d_path_first_piece[j] = its first piece ([n_paths] = n_pieces).
 * Validated on the device before anything is read through the values, each KATOME_E_ARG with a message: a piece id >= n_edges, a
 * first piece without KATOME_PIECE_WHOLE, n_pieces >= 2^31.  Scratch: at most 28 bytes per piece while the sizes are made, 16 of
 * them while the text is written, 24 bytes per path and 8 per contig.  Profile phase "gfa_paths", kernel
 * "k:gfa_paths_write_kernel".  Synchronises.
 * Out of scope: the coverage form of the S lines and anything on the sharded graph -- collapse needs the gathered graph.  The
 * bidirected form with paths is katome_dev_collapse_gfa_strands below.                                                     */
typedef struct {
    uint64_t  n_segments, n_links, text_bytes;
    uint8_t  *d_text;
    uint64_t *d_segment_off;             /* [n_segments]                                                               */
    uint64_t *d_link_first;              /* [n_segments + 1]                                                           */
    uint64_t  n_paths, n_jumps, path_bytes;
    uint8_t  *d_path_text;               /* d_text + text_bytes rounded up to 16                                       */
    uint64_t *d_path_line_off;           /* [n_paths + 1]                                                              */
    uint64_t *d_path_contig;             /* [n_paths]                                                                  */
    uint64_t *d_path_first_piece;        /* [n_paths + 1]                                                              */
} katome_dev_gfa_paths;
/* the whole text for the builder's LAST katome_dev_collapse (either layout), which keeps its device piece list in the builder
 * until the next collapse or destroy for this call: 4 bytes per piece.  No collapse result (none yet, or the last one failed):
 * KATOME_E_ARG, "collapse_gfa: no collapse result".  The result has its own buffers, owned by the builder until its next
 * katome_dev_collapse_gfa or destroy: the results of katome_dev_contigs_gfa, katome_dev_contigs_gfa_strands and
 * katome_dev_collapse stay valid, and the builder's graph is untouched.                                                   */
int katome_dev_collapse_gfa(katome_builder *b, katome_dev_gfa_paths *out, void *stream);

/* ---- the BIDIRECTED GFA of the assembly (csrc/gfa_strand_paths.hip): the contigs as P lines over MERGED segments, and mirrors ----
 * katome_dev_collapse_gfa writes its paths over the two-strand graph, so a reverse_complement assembly reaches a viewer as two
 * disconnected mirror images.  Here the text is, byte for byte, what katome_dev_contigs_gfa_strands writes for the collapse's shrunk
 * graph (H, one S line per representative, the canonical L lines), followed at text_bytes rounded up to 16 by the path region:
 *   P\tkatome_<c>\t<r0><o0>,<r1><o1>,...,<rn><on>\t*\n   run 0 of contig c
 *   P\tkatome_<c>.<r>\t...\t*\n                           run r = 1, 2, ... of contig c
 * For a piece with shrunk edge i, <r> = rep(i) and <o> = o(i) exactly as katome_dev_contigs_gfa_strands defines them: rep =
 * min(i, twin i), or i without a twin; '-' only where twin(i) < i; a self-twin and an unpaired edge are '+'.
 * Runs: names, contig order and the run rule are katome_dev_collapse_gfa's, evaluated on the TWO-STRAND arrays (a piece starts a
 * run iff it has KATOME_PIECE_WHOLE or edge_dst[id(p - 1)] != edge_src[id(p)]).  Merging cannot heal a seam: the conjugate of a
 * pair (x, y) is (twin y, twin x), and that pair is adjacent only if x and y were.  So n_paths, n_jumps, d_path_contig and
 * d_path_first_piece EQUAL katome_dev_collapse_gfa's for the same collapse; only the bytes and d_path_line_off differ.
 * Inside a P line every consecutive pair (x ox),(y oy) is an L line of the merged text, either as written or in its conjugate
 * spelling (y, flip oy, x, flip ox), where flip leaves a self-twin at +.
 * Mirrors.  Collapse walks both strands, so most contigs come twice.  For path j with piece ids a_0 .. a_{n-1}, mirror(j) = the
 * smallest q with n_q == n and id_q[t] == twin(a_{n-1-t}) for every t; an edge without a twin matches nothing; no such q: all ones.
 * mirror(j) == j is a self-mirror (the path [a, twin a]).  d_path_mirror[j] = mirror(j); n_mirrored = the paths that have one,
 * n_self_mirror = those that are their own.  The text does not change with it (optional fields on P lines are not something every
 * reader accepts): the array lets a caller keep one path per molecule, those with no mirror or mirror(j) >= j.
 * Validated on the device before anything is read through a value, each KATOME_E_ARG with a message: katome_dev_collapse_gfa's
 * piece checks, and on the arrays entry, where the caller supplies the twin map, a twin entry that is neither all ones nor below
 * n_edges and twin(twin(i)) != i.  Scratch beyond katome_dev_contigs_gfa_strands' and katome_dev_collapse_gfa's: 4 bytes per piece
 * (the oriented names) and about 50 bytes per path while the mirrors are found.  Profile phase
 * "gfa_strand_paths", kernel "k:gfa_strand_paths_write_kernel".  Synchronises.
 * Out of scope: the coverage form of merged S lines, folding mirror paths out of the text (katome_dev_collapse_unique below
 * selects one strand per molecule by CONTIG, and its kept names select their P lines), and anything on the sharded graph.   */
typedef struct {
    uint64_t  n_segments, n_links, text_bytes, n_unpaired, n_self_twins;
    uint8_t  *d_text;
    uint64_t *d_segment_name;            /* [n_segments]                                                               */
    uint64_t *d_segment_off;             /* [n_segments]                                                               */
    uint64_t *d_link_first;              /* [n_segments + 1]                                                           */
    uint64_t *d_edge_twin;               /* [n_edges]                                                                  */
    uint64_t  n_paths, n_jumps, path_bytes;
    uint8_t  *d_path_text;               /* d_text + text_bytes rounded up to 16                                       */
    uint64_t *d_path_line_off;           /* [n_paths + 1]                                                              */
    uint64_t *d_path_contig;             /* [n_paths]                                                                  */
    uint64_t *d_path_first_piece;        /* [n_paths + 1]                                                              */
    uint64_t  n_mirrored, n_self_mirror;
    uint64_t *d_path_mirror;             /* [n_paths], all ones: none                                                  */
    uint64_t  n_edges;                   /* merged edges of the collapse's shrunk graph (both strands)                 */
} katome_dev_gfa_strand_paths;
/* the whole text for the builder's LAST katome_dev_collapse, as katome_dev_collapse_gfa.  No collapse result: KATOME_E_ARG,
 * "collapse_gfa_strands: no collapse result".  The result has its own buffers, owned by the builder until its next
 * katome_dev_collapse_gfa_strands or destroy: the results of katome_dev_collapse, katome_dev_collapse_gfa, katome_dev_contigs_gfa
 * and katome_dev_contigs_gfa_strands stay valid, and the builder's graph is untouched.                                      */
int katome_dev_collapse_gfa_strands(katome_builder *b, katome_dev_gfa_strand_paths *out, void *stream);

/* ---- the STRAND-UNIQUE assembly (csrc/unique_contigs.hip): one FASTA record per molecule, on the device ----------------------------
 * A reverse_complement build keeps a k-mer and its reverse complement as two edges and collapse walks both strands, so the FASTA of
 * katome_dev_collapse holds nearly every molecule twice, once per strand.  For the builder's last katome_dev_collapse this gives
 * every contig's mirror, the kept set -- one strand per molecule, with all copies of that strand -- and the text of the kept contigs.
 *   Contig.  Contig c is the pieces from the c-th piece that has KATOME_PIECE_WHOLE up to the next such piece.  Its ids are
 *     a_0 .. a_{n-1}, each piece & ~KATOME_PIECE_WHOLE.  Runs and jumps (katome_dev_collapse_gfa) play no part: a contig with a seam
 *     is still one sequence of ids.
 *   Mirror.  mirror(c) is the smallest q with n_q == n and id_q[t] == twin(a_{n-1-t}) for every t.  twin is
 *     katome_dev_contigs_gfa_strands', verified base for base.  A contig that has an edge without a twin has no mirror (all ones).
 *     mirror(c) == c is a self-mirror.
 *   First copy.  first(c) = mirror(mirror(c)) where a mirror exists.  Because twin is an involution, this is the smallest contig
 *     with c's own piece sequence.  It costs two gathers and no second search.
 *   Kept.  Contig c is kept iff mirror(c) is none or mirror(mirror(c)) <= mirror(c).  Of a molecule's two strands, the one whose
 *     first copy comes first in the FASTA is kept, with all its copies.  Every copy of the other strand is dropped.  Contigs without
 *     a mirror and self-mirrors are all kept.  n_kept >= 1 whenever there is a contig.
 *   Text.  The kept contigs follow in ascending c.  KATOME_TEXT_PLAIN: their bases back to back.  KATOME_TEXT_FASTA:
 *     ">katome_<c>\n<bases>\n" with the ORIGINAL number c.  The result is byte for byte the concatenation of the kept records of
 *     katome_dev_collapse's FASTA.  Numbers have gaps.  A record is then the P lines katome_<c>, katome_<c>.1 ... of the assembly's
 *     GFA files, and the same record in the full FASTA.
 *   Sequence agreement.  Where c and mirror(c) are both single-run contigs, their texts are reverse complements of each other.
 *     Lengths agree for every mirrored pair.  At a seam the texts need not agree, so the definition goes by pieces and not by bases.
 * (The per-PATH rule of katome_dev_collapse_gfa_strands' d_path_mirror, mirror(j) >= j, keeps an irregular subset of a strand's
 * copies; this is the rule that keeps them all.)
 * d_contig_mirror[c] = mirror(c); n_mirrored = the contigs that have one, n_self_mirror = those that are their own.  d_kept_name
 * ascends; d_kept_off[i] / d_kept_len[i] = the first base in d_text and the bases of kept contig i.  d_text holds text_bytes bytes;
 * the buffer is a multiple of 16 bytes, with zeros behind the text up to it.
 * Scratch: 20 bytes per piece for the plan of the checks, 12 per piece and 12 per contig for the selection,
 * about 50 bytes per contig while the mirrors are found, then 4 + 16 bytes per kept piece for the compacted list and its text plan.
 * Profile phase "unique_contigs", kernels "k:text_write_named_kernel" and "k:unique_contigs selection"; the mirror search reports
 * to katome_dev_collapse_gfa_strands' "k:mirror_*" entries.
 * Out of scope: a GFA with the dropped contigs' P lines folded out (the kept names already select them), coverage on merged S lines,
 * anything on the sharded graph, and deduplicating by base sequence, such as contained or overlapping contigs.               */
typedef struct {
    uint64_t  n_contigs, n_mirrored, n_self_mirror;
    uint64_t *d_contig_mirror;           /* [n_contigs], all ones: none                                                */
    uint64_t  n_kept, text_bytes;
    uint32_t  layout, _pad;
    uint64_t *d_kept_name;               /* [n_kept], ascending: the contigs' numbers in katome_dev_collapse's result  */
    uint64_t *d_kept_off;                /* [n_kept]                                                                   */
    uint32_t *d_kept_len;                /* [n_kept]                                                                   */
    uint8_t  *d_text;
} katome_dev_unique_assembly;
/* for the builder's LAST katome_dev_collapse, whatever layout that collapse used.  No collapse result: KATOME_E_ARG,
 * "collapse_unique: no collapse result".  No contigs: all zero, KATOME_OK.  The twins are computed here (candidates, pairing,
 * base-for-base verification, after the segments' validation), without katome_dev_contigs_gfa_strands' link join, link sort or
 * line sizes.  The result has its own buffers, owned by the builder until its next katome_dev_collapse_unique or destroy: the
 * results of katome_dev_collapse, katome_dev_collapse_gfa, katome_dev_collapse_gfa_strands, katome_dev_contigs_gfa and
 * katome_dev_contigs_gfa_strands stay valid, and the builder's graph is untouched.  Synchronises.                           */
int katome_dev_collapse_unique(katome_builder *b, uint32_t layout, katome_dev_unique_assembly *out, void *stream);

/* Contigs::stats (stats/contigs.rs:31-89) from the contigs' lengths: host, pure.  No contigs: all zeros.  A tipping point of 0
 * with contigs present (sum / 2, (0.1 * sum) truncated, original_genome_length / 2), where the reference panics on
 * `.last().unwrap()`: KATOME_E_ARG, with a message that names which one.                                               */
typedef struct { uint64_t n50, l50, n90, ng50; } katome_contig_stats;
int katome_contig_stats_of(const uint64_t *lengths, uint64_t n, uint64_t original_genome_length, katome_contig_stats *out);

/* BasicAsm::assemble (asm/basic_assembler.rs:58-80) in host memory: the build, the stages "dcwced" with settings.min_weight and
 * original_genome_length, collapse, Contigs::stats and -- with out_path -- Contigs::save_to_file.  Needs
 * KATOME_FLAG_FIRST_SEEN_ORDER, like the staged entries.  The text is in KATOME_TEXT_FASTA layout: text[0, text_bytes) is the
 * file, contig i its bytes [contig_off[i], contig_off[i] + contig_len[i]).  Owned by the library until katome_assembly_free.
 * Errors, one status per panic site: the build's and the stages' as for katome_build_*_staged; a tipping point of 0 in the
 * stats (see katome_contig_stats_of): KATOME_E_ARG; a path that cannot be created: KATOME_E_OPEN, "couldn't create <path>:
 * <why>" (asm/mod.rs:62) -- the assembly is then still handed back when `out` is given.  With settings.n_devices > 1 the graph
 * is built sharded, gathered to the first GPU in the reference's numbering, and the stages and collapse run there; a graph that
 * cannot be gathered (2^32 edges or nodes) gives KATOME_E_UNSUPPORTED with a message that says so (collapse on the sharded
 * graph is out of scope).                                                                                               */
typedef struct {
    uint64_t n_contigs, text_bytes, read_bytes;
    uint32_t k, layout;
    const uint64_t *contig_off;
    const uint32_t *contig_len;
    const uint8_t  *text;
    katome_contig_stats   stats;
    katome_collapse_stats collapse;
} katome_assembly;
int  katome_assemble_files(const katome_settings *s, const char *const *paths, size_t n_paths, uint64_t original_genome_length,
                           const char *out_path /* nullable */, katome_assembly **out);
int  katome_assemble_packed(const katome_settings *s, const uint8_t *packed, uint64_t n_reads, uint32_t read_len,
                            const uint8_t *skip, uint64_t original_genome_length, const char *out_path /* nullable */,
                            katome_assembly **out);
/* Contigs::save_to_file (asm/mod.rs:57-72): KATOME_E_OPEN when the path cannot be created */
int  katome_assembly_save(const katome_assembly *a, const char *path);
void katome_assembly_free(katome_assembly *a);

/* katome_assemble_* followed by katome_dev_collapse_unique(KATOME_TEXT_FASTA), which has the definitions: one build, the stages, one
 * collapse, then the strand-unique form of its contigs in host memory.  text[0, text_bytes) is the file of the kept records, kept
 * contig i (numbered kept_name[i] in the full FASTA) its bytes [kept_off[i], kept_off[i] + kept_len[i]); stats:
 * katome_contig_stats_of over the kept lengths (a tipping point of 0: KATOME_E_ARG, as in katome_assemble_*).  fasta_path (all
 * contigs) and unique_path (the kept ones) are written when given; asm_out and unique_out are filled when given; all four NULL:
 * KATOME_E_ARG.  Statuses are katome_assemble_gfa_*'s: KATOME_FLAG_FIRST_SEEN_ORDER is needed; a file that cannot be created gives
 * KATOME_E_OPEN, "couldn't create <path>: <why>", with both results still handed back -- the FASTA path is tried first, the first
 * failure is the one reported, and the other file is still written; settings.n_devices > 1 is built sharded and gathered to the first
 * GPU.  Owned by the library until katome_unique_assembly_free.                                                              */
typedef struct {
    uint64_t n_contigs, n_kept, text_bytes, read_bytes;
    uint32_t k, _pad;
    uint64_t n_mirrored, n_self_mirror;
    const uint64_t *contig_mirror;       /* [n_contigs], all ones: none                                                */
    const uint64_t *kept_name;           /* [n_kept], ascending                                                        */
    const uint64_t *kept_off;            /* [n_kept]                                                                   */
    const uint32_t *kept_len;            /* [n_kept]                                                                   */
    const uint8_t  *text;
    katome_contig_stats stats;
} katome_unique_assembly;
int  katome_assemble_unique_files(const katome_settings *s, const char *const *paths, size_t n_paths, uint64_t original_genome_length,
                                  const char *fasta_path /* nullable */, const char *unique_path /* nullable */,
                                  katome_assembly **asm_out /* nullable */, katome_unique_assembly **unique_out /* nullable */);
int  katome_assemble_unique_packed(const katome_settings *s, const uint8_t *packed, uint64_t n_reads, uint32_t read_len,
                                   const uint8_t *skip, uint64_t original_genome_length, const char *fasta_path /* nullable */,
                                   const char *unique_path /* nullable */, katome_assembly **asm_out /* nullable */,
                                   katome_unique_assembly **unique_out /* nullable */);
int  katome_unique_assembly_save(const katome_unique_assembly *u, const char *path);
void katome_unique_assembly_free(katome_unique_assembly *u);

/* The unitig graph of a read set as GFA 1 in host memory: the build, the stage letters as the staged entries take them (d, c, w,
 * e; they need KATOME_FLAG_FIRST_SEEN_ORDER, an empty string works on a by-key build), katome_dev_shrink (AUTO) and
 * katome_dev_contigs_gfa; text[0, text_bytes) is the file, written when out_path is given.  segment_off / link_first as in
 * katome_dev_gfa.  Owned by the library until katome_gfa_free.  A path that cannot be created: KATOME_E_OPEN, "couldn't create
 * <path>: <why>" -- the result is then still handed back when `out` is given (katome_assemble_*'s rule).  With
 * settings.n_devices > 1 the graph is built sharded and gathered to the first GPU, as for katome_assemble_* (needs
 * KATOME_FLAG_FIRST_SEEN_ORDER; the GFA of the sharded shrink without a gather is katome_dist_contigs_gfa / katome_unitigs_gfa_*). */
typedef struct {
    uint64_t n_segments, n_links, text_bytes, read_bytes;
    uint32_t k, _pad;
    const uint8_t  *text;
    const uint64_t *segment_off;         /* [n_segments]                                                               */
    const uint64_t *link_first;          /* [n_segments + 1]                                                           */
} katome_gfa;
int  katome_gfa_files(const katome_settings *s, const char *const *paths, size_t n_paths, const char *stages,
                      uint64_t original_genome_length, const char *out_path /* nullable */, katome_gfa **out);
int  katome_gfa_packed(const katome_settings *s, const uint8_t *packed, uint64_t n_reads, uint32_t read_len, const uint8_t *skip,
                       const char *stages, uint64_t original_genome_length, const char *out_path /* nullable */, katome_gfa **out);
int  katome_gfa_save(const katome_gfa *g, const char *path);
void katome_gfa_free(katome_gfa *g);
/* the same with strand twins merged (katome_dev_contigs_gfa_strands has the format): stage letters, shrink (AUTO), out_path, the
 * result handed back on KATOME_E_OPEN and n_devices > 1 (built sharded, gathered to the first GPU) exactly as katome_gfa_*.  The
 * merged GFA of the sharded shrink WITHOUT a gather is not offered: katome_unitigs_gfa_* writes the two-strand form only.     */
typedef struct {
    uint64_t n_segments, n_links, text_bytes, read_bytes;
    uint32_t k, _pad;
    const uint8_t  *text;
    const uint64_t *segment_off;         /* [n_segments]                                                               */
    const uint64_t *link_first;          /* [n_segments + 1]                                                           */
    uint64_t n_edges, n_unpaired, n_self_twins;
    const uint64_t *segment_name;        /* [n_segments]                                                               */
    const uint64_t *edge_twin;           /* [n_edges], all ones: none                                                  */
} katome_gfa_strands;
int  katome_gfa_strands_files(const katome_settings *s, const char *const *paths, size_t n_paths, const char *stages,
                              uint64_t original_genome_length, const char *out_path /* nullable */, katome_gfa_strands **out);
int  katome_gfa_strands_packed(const katome_settings *s, const uint8_t *packed, uint64_t n_reads, uint32_t read_len, const uint8_t *skip,
                               const char *stages, uint64_t original_genome_length, const char *out_path /* nullable */,
                               katome_gfa_strands **out);
int  katome_gfa_strands_save(const katome_gfa_strands *g, const char *path);
void katome_gfa_strands_free(katome_gfa_strands *g);

/* katome_assemble_* followed by katome_dev_collapse_gfa: the assembly (FASTA) and the GFA of its shrunk graph with the contigs as
 * P lines, from one build.  text[0, text_bytes) holds the H, S and L lines and text[text_bytes, text_bytes + path_bytes) the P
 * lines, contiguous: text_bytes + path_bytes bytes are the file.  segment_off / link_first as in katome_dev_gfa; path_line_off
 * (relative to the path region), path_contig and path_first_piece as in katome_dev_gfa_paths.  Owned by the library until
 * katome_gfa_paths_free.  fasta_path, gfa_path, asm_out and gfa_out are each nullable (all four NULL: KATOME_E_ARG).
 * Preconditions and statuses are katome_assemble_*'s: KATOME_FLAG_FIRST_SEEN_ORDER is required; a path that cannot be created
 * gives KATOME_E_OPEN, "couldn't create <path>: <why>", with both results still handed back (the FASTA path is tried first; the
 * first failure is the one reported, the other file is still written); with settings.n_devices > 1 the graph is built sharded
 * and gathered to the first GPU.                                                                                          */
typedef struct {
    uint64_t n_segments, n_links, text_bytes, read_bytes;
    uint32_t k, _pad;
    const uint8_t  *text;                /* text_bytes + path_bytes                                                    */
    const uint64_t *segment_off;         /* [n_segments]                                                               */
    const uint64_t *link_first;          /* [n_segments + 1]                                                           */
    uint64_t n_paths, n_jumps, path_bytes;
    const uint64_t *path_line_off;       /* [n_paths + 1]                                                              */
    const uint64_t *path_contig;         /* [n_paths]                                                                  */
    const uint64_t *path_first_piece;    /* [n_paths + 1]                                                              */
} katome_gfa_paths;
int  katome_assemble_gfa_files(const katome_settings *s, const char *const *paths, size_t n_paths, uint64_t original_genome_length,
                               const char *fasta_path /* nullable */, const char *gfa_path /* nullable */,
                               katome_assembly **asm_out /* nullable */, katome_gfa_paths **gfa_out /* nullable */);
int  katome_assemble_gfa_packed(const katome_settings *s, const uint8_t *packed, uint64_t n_reads, uint32_t read_len,
                                const uint8_t *skip, uint64_t original_genome_length, const char *fasta_path /* nullable */,
                                const char *gfa_path /* nullable */, katome_assembly **asm_out /* nullable */,
                                katome_gfa_paths **gfa_out /* nullable */);
int  katome_gfa_paths_save(const katome_gfa_paths *g, const char *path);
void katome_gfa_paths_free(katome_gfa_paths *g);
/* the same with strand twins merged: katome_assemble_* followed by katome_dev_collapse_gfa_strands (which has the format).  The
 * fields of katome_gfa_strands, then those of katome_gfa_paths, then the mirrors; text[0, text_bytes) holds the H, S and L lines
 * and text[text_bytes, text_bytes + path_bytes) the P lines.  Arguments, nullable files and results, KATOME_E_OPEN with the results
 * still handed back and n_devices > 1 (built sharded, gathered to the first GPU) exactly as katome_assemble_gfa_*.  Owned by the
 * library until katome_gfa_strand_paths_free.                                                                               */
typedef struct {
    uint64_t n_segments, n_links, text_bytes, read_bytes;
    uint32_t k, _pad;
    const uint8_t  *text;                /* text_bytes + path_bytes                                                    */
    const uint64_t *segment_off;         /* [n_segments]                                                               */
    const uint64_t *link_first;          /* [n_segments + 1]                                                           */
    uint64_t n_edges, n_unpaired, n_self_twins;
    const uint64_t *segment_name;        /* [n_segments]                                                               */
    const uint64_t *edge_twin;           /* [n_edges], all ones: none                                                  */
    uint64_t n_paths, n_jumps, path_bytes;
    const uint64_t *path_line_off;       /* [n_paths + 1]                                                              */
    const uint64_t *path_contig;         /* [n_paths]                                                                  */
    const uint64_t *path_first_piece;    /* [n_paths + 1]                                                              */
    uint64_t n_mirrored, n_self_mirror;
    const uint64_t *path_mirror;         /* [n_paths], all ones: none                                                  */
} katome_gfa_strand_paths;
int  katome_assemble_gfa_strands_files(const katome_settings *s, const char *const *paths, size_t n_paths, uint64_t original_genome_length,
                                       const char *fasta_path /* nullable */, const char *gfa_path /* nullable */,
                                       katome_assembly **asm_out /* nullable */, katome_gfa_strand_paths **gfa_out /* nullable */);
int  katome_assemble_gfa_strands_packed(const katome_settings *s, const uint8_t *packed, uint64_t n_reads, uint32_t read_len,
                                        const uint8_t *skip, uint64_t original_genome_length, const char *fasta_path /* nullable */,
                                        const char *gfa_path /* nullable */, katome_assembly **asm_out /* nullable */,
                                        katome_gfa_strand_paths **gfa_out /* nullable */);
int  katome_gfa_strand_paths_save(const katome_gfa_strand_paths *g, const char *path);
void katome_gfa_strand_paths_free(katome_gfa_strand_paths *g);

/* first half of finalize only: sorted distinct edges (key, weight); used by the multi-GPU
 * driver, which resolves node ids across ranks itself                                      */
int katome_dev_edges(katome_builder *b, uint64_t **d_edge_key, uint32_t **d_edge_weight,
                     uint64_t *n_edges, void *stream);

/* The library keeps freed device blocks for reuse (hipMalloc/hipFree of multi-GiB buffers are slow);
 * this hands them back to the driver.                                                         */
int katome_dev_release_cache(int device);
/* out[0] = bytes the library holds from the driver on `device` (all segments), out[1] = how many of them are free
 * (cached), out[2] = blocks handed out and not yet returned.  After katome_dev_release_cache() out[0] is what live
 * builders / results still pin -- 0 when everything was closed.                                                   */
int katome_dev_cache_stats(int device, uint64_t out[3]);

/* ---- multi-GPU: the sharded build, one rank per GPU -------------------------------------------------------
 * The reference is one sequential loop (builder.rs:152-160); what shards is the read set.  Reads are split contiguously by
 * index over the ranks; every rank extracts its own records and routes each to its owner rank; owners count; the graph
 * is numbered across ranks.  Inside katome_build_* (settings.n_devices) the ranks are host threads of the calling process;
 * a job that runs one PROCESS per GPU (bench.py under a launcher) creates a communicator per process and drives
 * katome_dist_* itself.                                                                                       */
typedef struct katome_comm katome_comm;
#define KATOME_COMM_ID_BYTES 128
/* rank 0 makes the id (ncclGetUniqueId), every rank gets it out of band and joins (ncclCommInitRank) */
int katome_comm_unique_id(uint8_t *id /* [KATOME_COMM_ID_BYTES] */);
int katome_comm_create_rccl(const uint8_t *id, int rank, int world, int device, katome_comm **out);
/* the caller moves the bytes (tests: torch.distributed/gloo): element counts and offsets per peer, host or device
 * buffers (on_device); op: 0 sum, 1 max, 2 min.  Non-zero return = failure.                                 */
typedef struct {
    void *user;
    int (*alltoallv)(void *user, const void *send, const uint64_t *send_off, const uint64_t *send_cnt, void *recv,
                     const uint64_t *recv_off, const uint64_t *recv_cnt, uint64_t elem_bytes, int on_device);
    int (*allreduce_u64)(void *user, uint64_t *vals, uint64_t n, int op);
} katome_comm_callbacks;
int katome_comm_create_callbacks(const katome_comm_callbacks *cb, int rank, int world, int device, katome_comm **out);
void katome_comm_destroy(katome_comm *c);
int katome_comm_rank(const katome_comm *c);
int katome_comm_world(const katome_comm *c);
const char *katome_comm_kind(const katome_comm *c);               /* "rccl", "local", "callbacks" */
/* a single message above this many bytes travels in rounds (default 1 GiB) */
int katome_comm_set_max_message_bytes(katome_comm *c, uint64_t bytes);
int katome_comm_allreduce_u64(katome_comm *c, uint64_t *vals, uint64_t n, int op);
/* variable all-to-all: `send` holds send_cnt[p] elements for each peer p, in peer order; recv_cnt[p] is filled in and
 * `recv` (room for recv_capacity elements) receives them grouped by source.  Collective.                   */
int katome_comm_exchange(katome_comm *c, const void *send, const uint64_t *send_cnt, void *recv, uint64_t recv_capacity,
                         uint64_t *recv_cnt, uint64_t elem_bytes, int on_device, void *stream);

typedef struct katome_dist_builder katome_dist_builder;
/* one rank's share of the graph, device arrays owned by the builder */
typedef struct {
    uint64_t n_edges, n_nodes;            /* on this rank: its edges are the out-edges of the nodes it owns ...      */
    uint64_t total_edges, total_nodes;    /* ... of the whole graph                                                  */
    uint64_t node_base;                   /* by packed key: global id of this rank's node i = node_base + i           */
    uint32_t key_words, label_stride;
    uint64_t *d_edge_key;                 /* [n_edges][key_words] ascending                                          */
    uint32_t *d_edge_weight;
    uint64_t *d_edge_src, *d_edge_dst;    /* GLOBAL node ids                                                         */
    uint8_t  *d_edge_label;
    uint64_t *d_node_key;                 /* [n_nodes][key_words]                                                    */
    uint64_t *d_edge_id, *d_node_id;      /* FIRST_SEEN_ORDER: the reference's (petgraph) index of every edge / node of
                                             this rank; NULL by packed key                                           */
    uint64_t *d_edge_age;                 /* after katome_dist_remove_dead_paths or a stage that may remove edges
                                             (katome_dist_prune_weak_edges, _standardize_edges): the index each edge had when it was built
                                             (= its place in petgraph's adjacency lists, see katome_graph.edge_age); else NULL */
} katome_dist_graph;
/* settings as for katome_builder_create (settings.device = this rank's GPU; table_slots_hint for the WHOLE build);
 * the communicator stays the caller's.  Every call below is collective: all ranks make it, in the same order.        */
int  katome_dist_create(const katome_settings *s, katome_comm *comm, katome_dist_builder **out);
void katome_dist_destroy(katome_dist_builder *d);
/* this rank's reads, device pointers: reads [first_read, first_read + n_reads) of the whole input in input order (the
 * reference's numbering needs the global index), fixed length, in batches of batch_reads (0 = default).  May be called
 * again with the reads that follow.                                                                           */
int  katome_dist_add_reads(katome_dist_builder *d, const uint8_t *d_packed, uint64_t first_read, uint64_t n_reads,
                           uint32_t read_len, const uint8_t *d_skip, uint64_t batch_reads, void *stream);
/* this rank's reads of VARYING length, device pointers in katome_dev_extract_var's layout: read r is len[r] bases at byte
 * byte_off[r] of d_packed (2 bits per base, packed_bytes in all).  first_window: the global window index of this rank's
 * first read -- the sum of len - k + 1 over every read before it in input order (the reference's numbering needs it, as the
 * fixed-length entry needs first_read); it is the same on every call of a rank: a later call continues with the reads that
 * follow, after the windows of this rank's earlier calls.  Batches of about batch_windows windows (0 = default).
 * Collective, every call (a rank without reads calls with n_reads = 0): the first call agrees one tile span from all ranks'
 * reads; a read shorter than k gives KATOME_E_SHORT_READ, and any failure the same error, on every rank.  In first-seen
 * order a build takes either this entry or katome_dist_add_reads (KATOME_E_UNSUPPORTED for the mix); by packed key both,
 * except after a batch of one length that planned the supermer route (KATOME_E_UNSUPPORTED).  Routes "local" and "tiles";
 * with KATOME_DIST_ROUTE=supermers these reads plan the tiles route, which later batches of one length then take.
 * batch_windows is capped at 2^31 (a batch's records are indexed by 32 bits).                                        */
int  katome_dist_add_reads_var(katome_dist_builder *d, const uint8_t *d_packed, uint64_t packed_bytes, const uint64_t *d_byte_off,
                               const uint32_t *d_len, uint64_t n_reads, uint64_t first_window, uint64_t batch_windows, void *stream);
/* Clean::remove_weak_edges(threshold) when the edges are read out (by packed key only; see katome_dev_remove_weak_edges) */
int  katome_dist_remove_weak_edges(katome_dist_builder *d, uint32_t threshold);
int  katome_dist_finalize(katome_dist_builder *d, katome_dist_graph *out, void *stream);
/* FIRST_SEEN_ORDER: bring the whole graph to rank `root` in the reference's index order and hand it to a single-GPU
 * builder there (*root_builder; NULL on the other ranks; owned by `d`), on which katome_dev_remove_dead_paths,
 * katome_dev_remove_weak_edges, katome_dev_standardize_*, katome_dev_shrink and katome_dev_current_graph work as after
 * katome_dev_finalize.  The pruning of BASELINE config 5 runs this way: its walks and swap-removes depend on the global
 * numbering; the whole graph has to fit the root's HBM (< 2^32 edges).                           */
int  katome_dist_gather(katome_dist_builder *d, int root, katome_builder **root_builder, void *stream);
/* Prunable::remove_dead_paths (pruner.rs:36-82) on the SHARDED graph of a finalized FIRST_SEEN_ORDER build, no gather: walkers
 * hop from owner to owner along first out-edges (one all-to-all per step, < 2k steps), marked (position, count) pairs go to
 * rank 0, which replays petgraph's swap_removes on 64-bit positions and answers where every candidate edge / node ends up
 * (katome_amd/csrc/dist_prune.hip).  The graph may hold more than 2^32 edges (a rank's share may not).  Afterwards `out`
 * describes this rank's share of the pruned graph: d_edge_id / d_node_id are the indices the reference's PtGraph would hold,
 * d_edge_age the edges' ages.  Collective.                                                                              */
int  katome_dist_remove_dead_paths(katome_dist_builder *d, katome_dist_graph *out, katome_prune_stats *stats, void *stream);
/* The stages of assemble_with_graph after the first pruning (asm/basic_assembler.rs:63-72) on the SHARDED graph of a
 * finalized FIRST_SEEN_ORDER build whose shares were not gathered, no gather (katome_amd/csrc/dist_stages.hip); each may
 * run straight after katome_dist_finalize or after katome_dist_remove_dead_paths, in any order, any number of times.  A
 * packed-key or gathered builder gets KATOME_E_ARG.  Afterwards `out` describes this rank's share as after
 * katome_dist_remove_dead_paths: d_edge_id / d_node_id hold petgraph's indices, d_edge_age the ages (which move with their
 * edges) once a stage that may remove edges has run; edges stay on the rank that owns their source.  Collective.
 * KATOME_DIST_STAGES_FAIL=edges|nodes (tests): rank 0's index replay of that kind fails, and every rank returns the error.
 *   standardize_contigs (standardizer.rs:72-122): every contig gets the rounded mean of its weights, bit for bit as on one
 *     GPU, by one of two routes with the same result.  "table": every rank holds a table of 12 bytes per node of the WHOLE
 *     graph while it runs.  "ranked" (katome_amd/csrc/dist_contigs.hip): the contigs are ranked by pointer jumping with
 *     sums, memory per rank O(share), the exchange rounds grow with log2 of the longest contig.  Without
 *     KATOME_DIST_CONTIGS the table is taken when every rank has room for it and the ranked route otherwise (BASELINE
 *     config 5 in full: DESIGN.md section 6); KATOME_DIST_CONTIGS=table gives KATOME_E_OOM on every rank when a rank has
 *     no room, KATOME_DIST_CONTIGS=ranked takes the ranked route, any other value and ranks that disagree give
 *     KATOME_E_ARG on every rank.  A contig of 2^32 edges or more: KATOME_E_UNSUPPORTED (ranked).
 *     KATOME_DIST_CONTIGS_CHUNK=<n> (default 2^24): the most questions a rank sends in one exchange of the ranked route.
 *     Tests: KATOME_DIST_CONTIGS_TABLE_LIMIT=<bytes> stands in for a rank's free memory; KATOME_DIST_CONTIGS_FAIL=<rank>:
 *     that rank fails after the first ranking round and every rank returns KATOME_E_UNSUPPORTED naming it.
 *     KATOME_DIST_CONTIGS_TRACE (set to anything): every rank prints one line per call on stderr, the stage's wall time,
 *     its route and what katome_dist_standardize_stats_read would give.  All of these are read on every call.
 * A rank's share stays below 2^32 edges and 2^32 nodes (KATOME_E_UNSUPPORTED on every rank otherwise), and one retain may
 * remove fewer than 2^32 edges / nodes.
 *   prune_weak_edges: Clean::remove_weak_edges(threshold) (pruner.rs:84-93), at once: retain_edges, then retain_nodes,
 *     petgraph's swap_remove numbering on 64-bit positions.  (katome_dist_remove_weak_edges is another thing: by packed
 *     key, the threshold applied when the edges are read out.)
 *   standardize_edges (standardizer.rs:42-70): the weight sums of all ranks, the scaling of the one-GPU form, then
 *     prune_weak_edges(1); original_genome_length < k: KATOME_E_ARG on every rank.
 * After a stage that removed edges or nodes, katome_dist_remove_dead_paths runs for real again.                        */
int  katome_dist_standardize_contigs(katome_dist_builder *d, katome_dist_graph *out, void *stream);
int  katome_dist_prune_weak_edges(katome_dist_builder *d, uint32_t threshold, katome_dist_graph *out, void *stream);
int  katome_dist_standardize_edges(katome_dist_builder *d, uint64_t original_genome_length, uint32_t threshold,
                                   katome_dist_graph *out, void *stream);
/* what the last katome_dist_standardize_contigs that finished on this builder did (the host entries reach the stage
 * through the same function); KATOME_E_ARG before any such call                                                     */
typedef struct {
    uint32_t route;          /* 0 table, 1 ranked: what the last katome_dist_standardize_contigs of this builder took */
    uint32_t rank_rounds;    /* ranked: pointer-jumping rounds                                  */
    uint64_t exchanges;      /* ranked: question/answer exchanges over all rounds (chunks)      */
    uint64_t contigs;        /* ranked: contigs of the whole graph                              */
    uint64_t longest_contig; /* ranked: edges of the longest one                                */
    uint64_t cycle_edges;    /* ranked: edges of the whole graph left on cycles, untouched      */
    uint64_t bytes_sent;     /* bytes this rank sent during the call, either route              */
} katome_dist_standardize_stats;
int  katome_dist_standardize_stats_read(katome_dist_builder *d, katome_dist_standardize_stats *out);
/* this rank's merged edges after katome_dist_shrink, device arrays owned by the builder (valid until its next
 * katome_dist_shrink or destroy).  Node ids are the NEW ones: a surviving vertex's id is the number of surviving vertices
 * with a smaller global id, so they run over [0, total_nodes).                                                      */
typedef struct {
    uint64_t n_edges, n_nodes;            /* on this rank: the merged edges whose head edge it holds, the surviving nodes it owns */
    uint64_t total_edges, total_nodes;    /* ... of the whole shrunk graph                                          */
    uint64_t label_bytes;
    uint32_t key_words, _pad;
    uint64_t *d_edge_src, *d_edge_dst;    /* new global node ids                                                     */
    uint32_t *d_edge_weight;              /* the head edge's weight                                                  */
    uint32_t *d_edge_kmers;               /* k-mers on the path                                                      */
    uint64_t *d_edge_label_off;           /* [n_edges + 1]: edge i's compress_edge label at d_edge_label[off[i], off[i+1]) */
    uint8_t  *d_edge_label;
    uint64_t *d_edge_head_id;             /* the head edge's global index in the input graph: its petgraph index in
                                             FIRST_SEEN_ORDER, by packed key the rank's edge base + its local index  */
    uint64_t *d_node_id;                  /* [n_nodes] new id of every surviving node of this rank ...               */
    uint64_t *d_node_key;                 /* ... and its (k-1)-mer, [n_nodes][key_words]                            */
} katome_dist_contigs;
typedef struct {
    uint32_t rank_rounds;                 /* exchange rounds of the list ranking (grows with log2 of the longest path) */
    uint32_t cycle_rounds;                /* rounds of the second ranking over the cycles of inner vertices (0: none)  */
    uint64_t cycles;                      /* cycles of inner vertices in the whole graph                               */
    uint64_t longest_path;                /* k-mers on the longest merged edge                                         */
    uint64_t bytes_sent;                  /* bytes this rank sent to its peers during the call                         */
} katome_dist_shrink_stats;
/* Shrinkable::shrink in the traversal-free form of katome_dev_shrink_mode(KATOME_SHRINK_FAST) on the SHARDED graph, no
 * gather (katome_amd/csrc/dist_shrink.hip): a finalized build in either numbering, straight after katome_dist_finalize or
 * after katome_dist_remove_dead_paths and the katome_dist_standardize_* / katome_dist_prune_weak_edges stages, in any order.
 * Every maximal straight path becomes one edge on the rank that holds its head edge (the edge whose source is not inner),
 * spelling the whole path, with the head's weight; a cycle of inner vertices becomes a self-loop at its smallest global
 * node id.  The paths are ranked by pointer jumping: the exchange rounds grow with log2 of the longest path.  The rank's
 * graph is left as it is, so the other stages still run afterwards.  Ordered by d_edge_head_id (edges) and by new id
 * (nodes), FIRST_SEEN_ORDER shares give array for array what katome_dev_shrink_mode(FAST) gives on one GPU.  A builder
 * that was not finalized or whose shares were gathered gets KATOME_E_ARG; a share of 2^32 edges or nodes or more, node
 * ids of 2^40 or more and a path of 2^32 k-mers or more give KATOME_E_UNSUPPORTED, on every rank.  Memory per rank is
 * O(share).  KATOME_DIST_SHRINK_FAIL=<rank> (tests): that rank fails after the first ranking round, and every rank returns
 * the error.  `out` and `stats` may be NULL.  Collective.                                                              */
int  katome_dist_shrink(katome_dist_builder *d, katome_dist_contigs *out, katome_dist_shrink_stats *stats, void *stream);
/* katome_dist_shrink plus this rank's coverage (katome_dev_coverage, as katome_dev_shrink_coverage leaves it): entry j belongs to
 * this rank's merged edge j, like every array of katome_dist_contigs; matched by d_edge_head_id the ranks' values are the one-GPU
 * FAST coverage of the same graph.  Every non-head edge sends its weight to the rank of its head next to its base (one more
 * exchange over the same routing, counted in stats->bytes_sent); there the weights are staged where the bases are (4 bytes per
 * non-head edge, transient) and reduced per merged edge together with the head's own weight.  Collective, with the
 * preconditions, limits and KATOME_DIST_SHRINK_FAIL behaviour of katome_dist_shrink; cov NULL: KATOME_E_ARG.  A failing call
 * leaves no coverage behind, and a later katome_dist_shrink drops it.                                                     */
int  katome_dist_shrink_coverage(katome_dist_builder *d, katome_dist_contigs *out, katome_dev_coverage *cov,
                                 katome_dist_shrink_stats *stats, void *stream);
/* ---- the end of the sharded pipeline, no gather (katome_amd/csrc/dist_text.hip): text, Contigs::stats and the FASTA file of the
 * merged edges (unitigs) of the builder's last katome_dist_shrink.  All three are collective; a builder without such a result, or
 * whose shares were gathered, gets KATOME_E_ARG on every rank.  A failure of a rank's own allocations, launches or checks comes
 * back on every rank with a message that names the rank (csrc/dist_agree.h).  Memory per rank is O(share).
 *
 * katome_dist_contigs_text: the text of this rank's merged edges, each its whole label, in KATOME_TEXT_PLAIN or KATOME_TEXT_FASTA
 * layout (see katome_dev_collapse).  The order is RANK-MAJOR: contig first_contig + j is this rank's merged edge j, entry j
 * of every array of katome_dist_contigs (by packed key that is d_edge_head_id order, and one rank's text is the one-GPU text byte
 * for byte; in FIRST_SEEN_ORDER it is the order of the rank's own edges), and the ranks' texts one after the other, in rank
 * order, are one valid text -- in FASTA layout a file with the headers >katome_0 ... >katome_<total_contigs - 1> in sequence.
 * Sorting the records into the global head-id order of the one-GPU result would move the whole text between ranks and is
 * deliberately not done: a reader that wants that order sorts by d_edge_head_id.  2^31 merged edges
 * on a rank or a contig of 2^32 bases: KATOME_E_UNSUPPORTED.  KATOME_DIST_TEXT_FAIL=<rank> (tests): that rank fails after the
 * sizes are known, and every rank returns KATOME_E_UNSUPPORTED naming it.  The arrays are owned by the builder until its next
 * katome_dist_contigs_text or destroy; a katome_dist_shrink in between makes the result stale for katome_dist_contigs_save. */
typedef struct {
    uint64_t n_contigs, first_contig, total_contigs;    /* this rank's merged edges; contigs on lower ranks; all ranks */
    uint64_t text_bytes, text_base, total_text_bytes;   /* this rank's bytes; bytes of lower ranks; the whole text     */
    uint32_t layout, _pad;
    uint64_t *d_contig_off;                             /* offsets relative to this rank's d_text                      */
    uint32_t *d_contig_len;
    uint8_t  *d_text;
} katome_dist_assembly;
int  katome_dist_contigs_text(katome_dist_builder *d, uint32_t layout, katome_dist_assembly *out, void *stream);
/* Contigs::stats (see katome_contig_stats_of) of ALL ranks' contigs, the same on every rank and equal, field for field and status
 * for status, to katome_contig_stats_of over the ranks' lengths put together -- without any rank holding another rank's lengths:
 * the reference's scans are four radix selections over the k-mer counts (csrc/contig_select.h), four passes over the rank's
 * d_edge_kmers with one allreduce of 2048 words each.  A contig's length is its k-mer count + k - 1.  The first form works on the
 * caller's device array (n may be 0), the second on the builder's last katome_dist_shrink. */
int  katome_dist_contig_stats_arrays(katome_comm *c, int device, const uint32_t *d_edge_kmers, uint64_t n, uint32_t k,
                                     uint64_t original_genome_length, katome_contig_stats *out, void *stream);
int  katome_dist_contig_stats(katome_dist_builder *d, uint64_t original_genome_length, katome_contig_stats *out, void *stream);
/* the file of `a` (what this builder's last katome_dist_contigs_text returned), written by all ranks: rank 0 creates `path` and
 * sets its length to total_text_bytes -- failure: KATOME_E_OPEN, "couldn't create <path>: <why>" (asm/mod.rs:62), on every rank --,
 * then every rank copies its text down in chunks of KATOME_DIST_TEXT_CHUNK bytes (default 64 MiB: host memory is O(chunk)) and
 * writes them at text_base.  Write errors are agreed at the end; when the call fails after the file was created, rank 0 removes
 * it.  For ranks that are threads of one process, and for process ranks that see one filesystem. */
int  katome_dist_contigs_save(katome_dist_builder *d, const katome_dist_assembly *a, const char *path);
/* katome_unitigs_*, the host entry that ends in that file: the build, the flag's remove_dead_paths, the stage letters of `stages` (see
 * katome_build_*_staged; NULL or "": none), the traversal-free shrink (KATOME_SHRINK_FAST), Contigs::stats of its merged edges
 * and -- with out_path -- their FASTA file.  The result is a plain struct; the text goes to the file only.  With
 * settings.n_devices > 1 everything runs on the ranks' shares, never a gather, whatever the environment says (so a graph of
 * 2^32 edges and more gets its unitigs): katome_dist_remove_dead_paths, the katome_dist_* stages, katome_dist_shrink,
 * katome_dist_contigs_text, katome_dist_contig_stats and katome_dist_contigs_save; the file's records are then in rank-major
 * order.  On one GPU: katome_dev_shrink_mode(FAST), katome_dev_contigs_text, katome_contig_stats_of.  Stage letters or
 * KATOME_FLAG_REMOVE_DEAD_PATHS without KATOME_FLAG_FIRST_SEEN_ORDER: KATOME_E_ARG; a packed-key build without them is fine.  A
 * tipping point of 0 in the stats: KATOME_E_ARG, with `out` filled and the file written all the same; a path that cannot be
 * created: KATOME_E_OPEN, "couldn't create <path>: <why>". */
typedef struct {
    uint64_t n_contigs, text_bytes, total_bases, longest, read_bytes;   /* text_bytes: of the FASTA text, written or not */
    uint32_t k, n_devices;
    katome_contig_stats stats;
    katome_dist_shrink_stats shrink;       /* zeros on one GPU */
} katome_unitigs;
int  katome_unitigs_files(const katome_settings *s, const char *const *paths, size_t n_paths, const char *stages,
                          uint64_t original_genome_length, const char *out_path /* nullable */, katome_unitigs *out);
int  katome_unitigs_packed(const katome_settings *s, const uint8_t *packed, uint64_t n_reads, uint32_t read_len,
                           const uint8_t *skip, const char *stages, uint64_t original_genome_length,
                           const char *out_path /* nullable */, katome_unitigs *out);
/* ---- the unitig graph of the sharded shrink as GFA 1, no gather (katome_amd/csrc/dist_gfa.hip) ---------------------------------
 * Segments are numbered RANK-MAJOR, exactly like the records of katome_dist_contigs_text: segment first_segment + j is this
 * rank's merged edge j (entry j of every array of katome_dist_contigs), first_segment the merged edges of the ranks before it, so
 * segment <i> and the record >katome_<i> of the sharded FASTA of the same shrink result are the same unitig.  The whole text is
 *   H\tVN:Z:1.0\n
 *   the S lines of rank 0, of rank 1, ...       (each as for katome_dev_gfa, its name the global number)
 *   the L lines of rank 0, of rank 1, ...       (a rank writes the links whose a is one of its segments, by a, then b)
 * with links (a, b) where edge_dst[a] == edge_src[b] over the NEW global node ids, a and b global segment numbers, every
 * orientation +, the overlap <k-1>M, KC and ew as for katome_dev_gfa: byte for byte what katome_dev_gfa_arrays gives for the
 * ranks' arrays put together in rank order (on one rank: the one-GPU text of the same arrays).  Every rank therefore owns two byte
 * ranges of the file: its S part at s_base (on rank 0 the header line comes first, s_base = 0) and its L part at l_base.  On the
 * device they are one buffer: the S part at d_text, the L part at d_link_text = d_text + s_bytes rounded up to 16, zeros behind
 * each up to its multiple of 16.  Segment names, link ends, offsets and totals are 64-bit (the whole graph may hold 2^32 segments
 * and more); one rank's part has fewer than 2^32 - 2 lines, or every rank gets KATOME_E_UNSUPPORTED naming the rank and the number.
 * The links cross ranks: every merged edge registers its number with the owner of its source vertex (vertex v lives on rank
 * v / ceil(total_nodes / world)), every merged edge asks the owner of its target and gets the at most four out-segments back in
 * ascending order, in chunks of KATOME_DIST_GFA_CHUNK records per rank and exchange (default 2^24).  A vertex with a fifth
 * out-segment is a broken invariant: KATOME_E_DEVICE on every rank.  Memory per rank is O(share), never a second copy of the text
 * (DESIGN.md section 11c has the bytes).  Preconditions as for katome_dist_contigs_text: no shrink result, or gathered shares:
 * KATOME_E_ARG on every rank; the result is stale for katome_dist_gfa_save after the next katome_dist_shrink.  No edges anywhere:
 * the header line alone, on rank 0.  KATOME_DIST_GFA_FAIL=<rank> (tests): that rank fails after the sizes are known, and every
 * rank returns KATOME_E_UNSUPPORTED naming it.  KATOME_DIST_GFA_TRACE=1: every rank's wall time per call on stderr.  Profile
 * phase "gfa"; the exchanges are accounted with the other sharded stages'.  Arrays owned by the builder until its next
 * katome_dist_contigs_gfa or destroy.  Collective. */
typedef struct {
    uint64_t n_segments, first_segment, total_segments;
    uint64_t n_links, total_links;
    uint64_t s_bytes, s_base, l_bytes, l_base, total_text_bytes;   /* this rank's two parts and where they start in the whole text */
    uint8_t  *d_text, *d_link_text;                               /* S part (rank 0: the header first); L part                     */
    uint64_t *d_segment_off;                                       /* [n_segments], relative to d_text                              */
    uint64_t *d_link_first;                                        /* [n_segments + 1]                                              */
    uint64_t *d_link_b;                                            /* [n_links] global number of every link's second segment        */
} katome_dist_gfa;
int  katome_dist_contigs_gfa(katome_dist_builder *d, katome_dist_gfa *out, void *stream);
/* katome_dist_contigs_gfa with the S lines of katome_dev_contigs_gfa_coverage (KC the sum, mn / mx behind ew).  The builder's last
 * shrink must have been a katome_dist_shrink_coverage: KATOME_E_ARG otherwise, on every rank.  It shares katome_dist_contigs_gfa's
 * buffers and staleness rule; katome_dist_gfa_save writes its result unchanged.  Collective. */
int  katome_dist_contigs_gfa_coverage(katome_dist_builder *d, katome_dist_gfa *out, void *stream);
/* the file of `g` (what this builder's last katome_dist_contigs_gfa returned), written by all ranks as katome_dist_contigs_save
 * writes the FASTA file: rank 0 creates `path` at total_text_bytes -- failure: KATOME_E_OPEN, "couldn't create <path>: <why>", on
 * every rank --, every rank writes its two parts at s_base and l_base in chunks of KATOME_DIST_TEXT_CHUNK bytes, write errors are
 * agreed at the end and no partial file is left behind. */
int  katome_dist_gfa_save(katome_dist_builder *d, const katome_dist_gfa *g, const char *path);
/* katome_unitigs_gfa_*: katome_unitigs_* with the graph as its ending -- the same pipeline and the same refusals (stage letters or
 * KATOME_FLAG_REMOVE_DEAD_PATHS without KATOME_FLAG_FIRST_SEEN_ORDER: KATOME_E_ARG; a packed-key build without them is fine; the
 * create error as there).  With settings.n_devices > 1 everything runs on the shares and ends in katome_dist_contigs_gfa and
 * katome_dist_gfa_save; on one GPU it is katome_dev_shrink_mode(FAST) and katome_dev_contigs_gfa, and the file is that entry's
 * text.  The result is a plain struct; the text goes to the file only.  With KATOME_FLAG_PATH_COVERAGE in settings.flags the
 * shrink is the _coverage one and the text the coverage form's (KC the sum, mn / mx), on one GPU and on the shares alike. */
typedef struct {
    uint64_t n_segments, n_links, text_bytes, total_bases, longest, read_bytes;
    uint32_t k, n_devices;
    katome_dist_shrink_stats shrink;     /* zeros on one GPU */
} katome_unitigs_gfa;
int  katome_unitigs_gfa_files (const katome_settings *s, const char *const *paths, size_t n_paths, const char *stages,
                               uint64_t original_genome_length, const char *out_path /* nullable */, katome_unitigs_gfa *out);
int  katome_unitigs_gfa_packed(const katome_settings *s, const uint8_t *packed, uint64_t n_reads, uint32_t read_len,
                               const uint8_t *skip, const char *stages, uint64_t original_genome_length,
                               const char *out_path /* nullable */, katome_unitigs_gfa *out);
/* this rank's share of the graph as it stands (after katome_dist_finalize / katome_dist_remove_dead_paths / the stages) */
int  katome_dist_current_graph(katome_dist_builder *d, katome_dist_graph *out);
/* katome_dev_graph_stats / katome_dev_weight_spectrum for the SHARDED graph, no gather (katome_amd/csrc/dist_stats.hip): the
 * numbers of the WHOLE graph, the same on every rank, for a finalized build in either numbering, straight after
 * katome_dist_finalize, after katome_dist_remove_dead_paths and after the katome_dist_standardize_* /
 * katome_dist_prune_weak_edges stages.  Out-degrees and weights are local; for the in-degrees every edge sends its target's
 * address to the target's owner, at most KATOME_DIST_STATS_CHUNK (default 2^24) records per rank and exchange; two allreduces
 * (sums, maxima) combine the ranks.  All counts are u64: the graph may hold more than 2^32 edges, a rank's share may not
 * (KATOME_E_UNSUPPORTED on every rank).  Memory per rank is O(share).  Not finalized, or gathered: KATOME_E_ARG.  A failure
 * of a rank's own allocations, launches or checks comes back on every rank, with a message that names the rank (what the
 * exchange layer allocates inside one exchange is not agreed, as in the other sharded stages); KATOME_DIST_STATS_FAIL=<rank>
 * (tests): that rank fails after the first exchange.  The bytes sent are accounted to the "prune" exchange phase.  Where a stage has dropped
 * the links of a FIRST_SEEN_ORDER build, katome_dist_graph_stats rebuilds them (as katome_dist_shrink and
 * katome_dist_remove_dead_paths do), which re-orders the rank's node arrays: fetch them again with katome_dist_current_graph.
 * Collective. */
int  katome_dist_graph_stats(katome_dist_builder *d, katome_stats *out, void *stream);
int  katome_dist_weight_spectrum(katome_dist_builder *d, uint64_t *bins /* host, [n_bins] */, uint32_t n_bins, void *stream);
/* the rank's single-GPU builder underneath (per-phase kernel timing: katome_builder_profile*) */
katome_builder *katome_dist_inner(katome_dist_builder *d);
/* which records travel in this build: "local" (every rank counts its own reads, distinct k-mers routed: up to two ranks), "tiles"
 * (tiles, mid tiles and k-mer records routed level by level: three ranks and more), "supermers" (one exchange of 16-byte supermer
 * records before any counting: KATOME_DIST_ROUTE=supermers, by packed key, k <= 31); KATOME_DIST_ROUTE overrides the choice */
const char *katome_dist_route(const katome_dist_builder *d);
/* exchange accounting since the last read: katome_dist_exchange_count() phases named by katome_dist_exchange_name(),
 * out[4*i..] = {calls, bytes that left this rank, largest single (rank -> peer) message, microseconds inside the exchange} */
uint32_t katome_dist_exchange_count(void);
const char *katome_dist_exchange_name(uint32_t phase);
int  katome_dist_exchange_read(katome_dist_builder *d, uint64_t *out);
/* contiguous shard of `total_reads` for `rank` (starts are multiples of 64 reads: 16-byte aligned packed rows) */
void katome_shard_range(uint64_t total_reads, uint32_t world, uint32_t rank, uint64_t *first, uint64_t *count);

/* ---- device primitives the finalize is built from (exported for the multi-GPU driver and
 * for unit tests; each is a hand-written HIP kernel set) -------------------------------- */
/* LSD radix sort of n keys of `key_words` u64 words on bits [0, key_bits); optional u32
 * values.  d_keys/d_vals are sorted in place (a temporary of equal size is allocated).     */
int katome_dev_sort(int device, uint64_t *d_keys, uint32_t *d_vals, uint64_t n, uint32_t key_words,
                    uint32_t key_bits, void *stream);
/* remove_paths' edge removals (pruner.rs:199-217: the collected indices sorted descending, Graph::remove_edge =
 * swap_remove, an index listed twice removes what was moved in) as katome_dev_remove_dead_paths runs them: d_pos[u]
 * ascending marked positions, d_mult[u] how often each is listed, of n_edges edges.  -> d_victims (identity of every
 * removed edge, in removal order; room for sum(d_mult)), the moves d_move_to[i] <- d_move_from[i] that fill the marked
 * positions below the new count (room for u), counts = {removed, moves, edges left, removals owed to repeats}      */
int katome_dev_replay_edge_removals(int device, const uint32_t *d_pos, const uint32_t *d_mult, uint64_t u, uint64_t n_edges,
                                    uint32_t *d_victims, uint32_t *d_move_to, uint32_t *d_move_from, uint64_t *counts,
                                    void *stream);
/* remove_single_node after every removed edge (pruner.rs:206-225; Graph::remove_node = swap_remove): d_die[2t],
 * d_die[2t+1] = the source / target that edge removal t leaves without edges (0xFFFFFFFF: stays); when both go, the
 * one at the larger current index goes first.  -> the moves d_move_to[i] <- d_move_from[i] of the nodes that end up
 * re-numbered (room for as many as die), counts = {moves, nodes left, 1 if the device form gave up (chains of moves
 * longer than it follows: katome_dev_remove_dead_paths then runs the sequential replay on the host; nothing is written)} */
int katome_dev_replay_node_removals(int device, const uint32_t *d_die, uint64_t m, uint64_t n_nodes, uint32_t *d_move_to,
                                    uint32_t *d_move_from, uint64_t *counts, void *stream);
/* the same two replays on 64-bit positions (0xFFFFFFFFFFFFFFFF: stays): what katome_dist_remove_dead_paths runs on rank 0 for
 * a graph sharded over several GPUs, which may hold more than 2^32 edges (BASELINE config 5: 1.1e10).  Only the marked
 * entries and the tail positions that disappear are touched, so n_edges / n_nodes are not bounded by any buffer.         */
int katome_dev_replay_edge_removals64(int device, const uint64_t *d_pos, const uint32_t *d_mult, uint64_t u, uint64_t n_edges,
                                      uint64_t *d_victims, uint64_t *d_move_to, uint64_t *d_move_from, uint64_t *counts,
                                      void *stream);
int katome_dev_replay_node_removals64(int device, const uint64_t *d_die, uint64_t m, uint64_t n_nodes, uint64_t *d_move_to,
                                      uint64_t *d_move_from, uint64_t *counts, void *stream);
/* exclusive prefix sums of m u32 counts as u64: d_offs[i] = counts[0] + .. + counts[i-1], d_offs[m] = the total   */
int katome_dev_scan_counts(int device, const uint32_t *d_counts, uint64_t m, uint64_t *d_offs, void *stream);
/* test entry: the (sub-window, count) records of a list of n_tiles tiles of tile_bases bases -- record p is sub-window p % span (k
 * bases, starts `stride` apart) of tile p / span, canonical (rc) or in the representative orientation (rep) -- after their first
 * partition pass, in d_keys / d_weights, and that pass's digit counts per sort tile in d_digit_counts ([tiles][256]).  fused: the pass
 * cuts its records out of the list; otherwise they are written first and the pass reads them (synchronises)                         */
int katome_dev_list_first_pass(int device, const uint64_t *d_tiles, const uint32_t *d_counts, uint64_t n_tiles, uint32_t tile_bases,
                               uint32_t k, uint32_t span, uint32_t stride, int rc, int rep, int fused, uint64_t *d_keys,
                               uint32_t *d_weights, uint32_t *d_digit_counts, void *stream);
/* test entry: a list-fed level of two-word records on its own, from the list to the list of its distinct (key, count) -- the records
 * of katome_dev_list_first_pass (rep = 0) through both partition passes and the count in LDS.  packed: 1 -- where the sub-windows have
 * 33 .. 39 bases the records carry their count in the free bits of their first word and there is no
 * weights array (csrc/counted_key.h); 0 -- plain keys and weights.  *took_packed says which it was.  d_pass1_* / d_pass2_* (null: not
 * wanted): the n_tiles * span records after the first and the second pass as plain keys ([n][2]) and weights.  d_out_keys /
 * d_out_weights: room for n_tiles * span entries; *n_out of them are written, in no particular order (synchronises)                     */
int katome_dev_count_in_key(int device, const uint64_t *d_tiles, const uint32_t *d_counts, uint64_t n_tiles, uint32_t tile_bases, uint32_t k,
                            uint32_t span, uint32_t stride, int rc, int packed, uint64_t *d_pass1_keys, uint32_t *d_pass1_weights,
                            uint64_t *d_pass2_keys, uint32_t *d_pass2_weights, uint64_t *d_out_keys, uint32_t *d_out_weights,
                            uint64_t *n_out, int *took_packed, void *stream);
/* test entry: the count of a level by sorting on records of the caller's own -- n (key, count) records in any order, d_keys [n][nw]
 * with nw the words of a key of k bases (k = 2 .. 95: one, two or three words), d_weights [n] or NULL (two and three words only:
 * every record counts once) -- to the distinct keys with their counts summed in u32 (sums wrap).  rc: every key leaves with its
 * reverse complement, both with the sum; a key that is its own reverse complement once with twice the sum; the records must hold
 * one orientation of a k-mer only.  min_weight: an edge stays when its final weight is at least that.  Three words: rc = 0 and
 * min_weight = 0 only.  n_parts > 0 (one word, rc = 0, min_weight = 0, at most 16): the keys leave grouped by the owner of their
 * core, the middle k - 2 bases (katome_key_owner with core_shift 2, core_bases k - 2): owner p's in [owner_base[p], owner_base[p] +
 * owner_count[p]) of the output; n_parts = 0: one stretch, owner_base / owner_count may be NULL.  The input is copied (the count
 * permutes its records).  d_out_keys [out_capacity][nw] / d_out_weights [out_capacity], out_capacity >= (rc ? 2 : 1) * n + 1;
 * *n_out entries in no particular order, *n_distinct distinct keys met.  The status is the count's own: KATOME_E_UNSUPPORTED where a
 * build would count the level in the hash table instead (synchronises)                                                        */
int katome_dev_count_records(int device, const uint64_t *d_keys, const uint32_t *d_weights, uint64_t n, uint32_t k, int rc,
                             uint32_t min_weight, uint32_t n_parts, uint64_t *d_out_keys, uint32_t *d_out_weights,
                             uint64_t out_capacity, uint64_t *n_out, uint64_t *n_distinct, uint64_t *owner_base,
                             uint64_t *owner_count, void *stream);
/* test entry: the one partition pass that S2 of the ordered k-mer count takes when its writer placed it by its first digit.
 * used[256] (host): the keys of every region; region d lies from start[d] on in d_keys / d_weights / d_digits, start[] (257 of them,
 * the last one the arrays' length) being what katome_s2_region_starts gives for `used` -- every region a whole number of 4096-key
 * tiles.  d_digits: bits 2k - 8 .. 2k - 1 of every key, one byte each at the key's index.  d_keys_out / d_weights_out: the sum of
 * used[] records, the regions read in digit order and partitioned by those bits, stable (synchronises)                              */
void katome_s2_region_starts(const uint64_t *used, uint64_t *start);
int katome_dev_s2_region_pass(int device, uint32_t k, const uint64_t *used, const uint64_t *d_keys, const uint32_t *d_weights,
                              const uint8_t *d_digits, uint64_t *d_keys_out, uint32_t *d_weights_out, void *stream);
/* in-place unique of sorted keys; returns the new count (synchronises)                     */
int katome_dev_unique(int device, uint64_t *d_keys, uint64_t n, uint32_t key_words, uint64_t *n_out,
                      void *stream);
/* rank of each query key in a sorted unique key array (every query must be present; absent
 * keys yield UINT64_MAX)                                                                   */
int katome_dev_rank(int device, const uint64_t *d_sorted, uint64_t n_sorted, uint32_t key_words,
                    uint32_t key_bits, const uint64_t *d_queries, uint64_t n_queries,
                    uint64_t *d_rank_out, void *stream);
/* node numbering of a sorted distinct edge list (what katome_dev_finalize does): d_node_key receives the
 * node keys (capacity [2*n_edges][key_words]: the sources in ascending order, then the out-edge-less
 * targets in ascending order), d_edge_src/d_edge_dst [n_edges] the positions of each edge's endpoints in
 * it; *n_nodes the node count (synchronises)                                                    */
int katome_dev_node_ids(int device, const uint64_t *d_edge_key, uint64_t n_edges, uint32_t k, uint64_t *d_node_key,
                        uint64_t *d_edge_src, uint64_t *d_edge_dst, uint64_t *n_nodes, void *stream);
/* derive (k-1)-mer endpoint keys of each edge: d_src/d_dst [n][key_words]                  */
/* first half of katome_dev_node_ids: the distinct source (k-1)-mers of sorted edges, ascending (d_node_key:
 * room for n_edges keys), and each edge's position among them                                          */
int katome_dev_source_ids(int device, const uint64_t *d_edge_key, uint64_t n_edges, uint32_t k,
                          uint64_t *d_node_key, uint64_t *d_edge_src, uint64_t *n_sources, void *stream);
/* source / target (k-1)-mer of every edge (either output may be NULL) */
int katome_dev_endpoints(int device, const uint64_t *d_edge_key, uint64_t n, uint32_t k,
                         uint64_t *d_src_key, uint64_t *d_dst_key, void *stream);
/* compress_edge-format labels (compress.rs:250-271) of packed k-mers                       */
int katome_dev_labels(int device, const uint64_t *d_edge_key, uint64_t n, uint32_t k,
                      uint8_t *d_label, void *stream);
/* the text kernel on the caller's arrays: n_labels labels in compress_edge format (compress.rs:250-271), label i at bytes
 * [d_label_off[i], d_label_off[i + 1]) of d_label, and n_pieces pieces (see katome_dev_collapse; d_pieces NULL: piece p = label p,
 * whole).  *n_contigs and *text_bytes are always set.  d_text NULL: nothing else is written (a size query).  Otherwise
 * d_contig_off / d_contig_len need room for contig_cap >= *n_contigs entries and d_text, 16-byte aligned, for text_cap >=
 * *text_bytes rounded up to 16 (KATOME_E_ARG when they are too small).  d_label must be 4-byte aligned and lie in an allocation
 * whose size is a multiple of 4 (KATOME_E_ARG for a misaligned pointer): the kernel reads the aligned 32-bit words that hold the
 * bytes it needs, so up to 3 bytes on either side of a label inside those words are read and ignored.  A piece that names no label, a label shorter than k bases
 * or malformed offsets: KATOME_E_ARG, before anything is read through them.  n_pieces >= 2^31 or a contig of 2^32 bases or more:
 * KATOME_E_UNSUPPORTED.  KATOME_TEXT_TRACE=1 in the environment: the writing kernel's time on stderr.  Synchronises. */
int katome_dev_pieces_text(int device, uint32_t k, const uint8_t *d_label, const uint64_t *d_label_off, uint64_t n_labels,
                           const uint32_t *d_pieces, uint64_t n_pieces, uint32_t layout, uint64_t *d_contig_off,
                           uint32_t *d_contig_len, uint64_t contig_cap, uint8_t *d_text, uint64_t text_cap, uint64_t *n_contigs,
                           uint64_t *text_bytes, void *stream);
/* the same with a starting number: contig c's FASTA header reads ">katome_<first_contig + c>", up to 20 digits (a part of a text
 * whose other parts are written elsewhere: katome_dist_contigs_text).  katome_dev_pieces_text is this with first_contig = 0.
 * first_contig + *n_contigs past 2^64: KATOME_E_UNSUPPORTED. */
int katome_dev_pieces_text_numbered(int device, uint32_t k, const uint8_t *d_label, const uint64_t *d_label_off, uint64_t n_labels,
                                    const uint32_t *d_pieces, uint64_t n_pieces, uint32_t layout, uint64_t first_contig,
                                    uint64_t *d_contig_off, uint32_t *d_contig_len, uint64_t contig_cap, uint8_t *d_text,
                                    uint64_t text_cap, uint64_t *n_contigs, uint64_t *text_bytes, void *stream);
/* katome_dev_contigs_gfa on the caller's arrays (the layout of katome_dev_contigs; label_bytes: the size of d_edge_label, which
 * every label offset is checked against).  *n_links and *text_bytes are always set.  d_text NULL: nothing else is written (a
 * size query).  Otherwise d_segment_off needs room for n_edges entries, d_link_first for n_edges + 1, and d_text, 16-byte
 * aligned, for text_cap >= *text_bytes rounded up to 16 (KATOME_E_ARG when it is too small).  d_edge_label as for
 * katome_dev_pieces_text: 4-byte aligned, in an allocation whose size is a multiple of 4.  KATOME_GFA_TRACE=1 in the environment:
 * the writing kernel's time on stderr (there is no builder whose profile could hold it).  Synchronises. */
int katome_dev_gfa_arrays(int device, uint32_t k, uint64_t n_nodes, uint64_t n_edges, const uint64_t *d_edge_src,
                          const uint64_t *d_edge_dst, const uint32_t *d_edge_weight, const uint32_t *d_edge_kmers,
                          const uint64_t *d_edge_label_off, const uint8_t *d_edge_label, uint64_t label_bytes,
                          uint64_t *d_segment_off, uint64_t *d_link_first, uint8_t *d_text, uint64_t text_cap,
                          uint64_t *n_links, uint64_t *text_bytes, void *stream);
/* katome_dev_contigs_gfa_coverage on the caller's arrays: katome_dev_gfa_arrays with the three coverage arrays (n_edges entries
 * each) behind d_edge_kmers; the size query works the same.  On top of katome_dev_gfa_arrays' validation, per segment and on
 * the device: min <= weight <= max and min * kmers <= sum <= max * kmers (64-bit) -- a violation: KATOME_E_ARG, "gfa: a segment's
 * coverage does not fit its weight and k-mer count", and no line size is computed from the bad values.  A null coverage array
 * with n_edges > 0: KATOME_E_ARG. */
int katome_dev_gfa_coverage_arrays(int device, uint32_t k, uint64_t n_nodes, uint64_t n_edges, const uint64_t *d_edge_src,
                                   const uint64_t *d_edge_dst, const uint32_t *d_edge_weight, const uint32_t *d_edge_kmers,
                                   const uint64_t *d_kmer_sum, const uint32_t *d_kmer_min, const uint32_t *d_kmer_max,
                                   const uint64_t *d_edge_label_off, const uint8_t *d_edge_label, uint64_t label_bytes,
                                   uint64_t *d_segment_off, uint64_t *d_link_first, uint8_t *d_text, uint64_t text_cap,
                                   uint64_t *n_links, uint64_t *text_bytes, void *stream);
/* katome_dev_contigs_gfa_strands on the caller's arrays, in the form of katome_dev_gfa_arrays.  counts[5] = {n_segments, n_links,
 * text_bytes, n_unpaired, n_self_twins} are always set.  d_text NULL: nothing else is written (a size query).  Otherwise
 * d_segment_name and d_segment_off need room for n_segments entries, d_link_first for n_segments + 1, d_edge_twin for n_edges
 * (n_segments <= n_edges), and d_text, 16-byte aligned, for text_cap >= text_bytes rounded up to 16.  Synchronises. */
int katome_dev_gfa_strands_arrays(int device, uint32_t k, uint64_t n_nodes, uint64_t n_edges, const uint64_t *d_edge_src,
                                  const uint64_t *d_edge_dst, const uint32_t *d_edge_weight, const uint32_t *d_edge_kmers,
                                  const uint64_t *d_edge_label_off, const uint8_t *d_edge_label, uint64_t label_bytes,
                                  uint64_t *d_segment_name, uint64_t *d_segment_off, uint64_t *d_link_first, uint64_t *d_edge_twin,
                                  uint8_t *d_text, uint64_t text_cap, uint64_t *counts, void *stream);
/* the path region of katome_dev_collapse_gfa alone, on the caller's arrays: n_pieces pieces (see katome_dev_collapse) over a graph
 * of n_edges edges, of which only d_edge_src and d_edge_dst are read.  counts[3] = {n_paths, n_jumps, text_bytes} are always set
 * (zeros on an error).  d_text NULL: nothing else is written (a size query).  Otherwise d_path_line_off and d_path_first_piece
 * need room for path_cap + 1 entries, d_path_contig for path_cap, with path_cap >= n_paths, and d_text, 16-byte aligned, for
 * text_cap >= text_bytes rounded up to 16 (zeros behind the text up to that multiple): KATOME_E_ARG when either is too small.
 * Validation as for katome_dev_collapse_gfa.  KATOME_GFA_PATHS_TRACE=1 in the environment: the writing kernel's time on stderr.
 * Synchronises. */
int katome_dev_gfa_paths_arrays(int device, uint64_t n_edges, const uint64_t *d_edge_src, const uint64_t *d_edge_dst,
                                const uint32_t *d_pieces, uint64_t n_pieces, uint64_t *d_path_line_off /* [n_paths + 1] */,
                                uint64_t *d_path_contig /* [n_paths] */, uint64_t *d_path_first_piece /* [n_paths + 1] */,
                                uint64_t path_cap, uint8_t *d_text, uint64_t text_cap, uint64_t *counts /* [3] */, void *stream);
/* the path region of katome_dev_collapse_gfa_strands and d_path_mirror alone, on the caller's arrays: katome_dev_gfa_paths_arrays
 * with the twin map d_edge_twin (n_edges entries as katome_dev_gfa_strands.d_edge_twin gives them: all ones for none) behind
 * d_edge_dst and d_path_mirror (path_cap entries) behind d_path_first_piece.  counts[5] = {n_paths, n_jumps, text_bytes,
 * n_mirrored, n_self_mirror} are always set (zeros on an error); d_text NULL: a size query.  The twin map is validated on the
 * device first: an entry that is neither all ones nor below n_edges, or twin(twin(i)) != i: KATOME_E_ARG, each with its message;
 * then the pieces as for katome_dev_gfa_paths_arrays.  2^32 - 1 edges or more: KATOME_E_UNSUPPORTED.
 * KATOME_GFA_STRAND_PATHS_TRACE=1 in the environment: the times of the writer and of the mirror search's parts on stderr.
 * Synchronises. */
int katome_dev_gfa_strand_paths_arrays(int device, uint64_t n_edges, const uint64_t *d_edge_src, const uint64_t *d_edge_dst,
                                       const uint64_t *d_edge_twin, const uint32_t *d_pieces, uint64_t n_pieces,
                                       uint64_t *d_path_line_off /* [n_paths + 1] */, uint64_t *d_path_contig /* [n_paths] */,
                                       uint64_t *d_path_first_piece /* [n_paths + 1] */, uint64_t *d_path_mirror /* [n_paths] */,
                                       uint64_t path_cap, uint8_t *d_text, uint64_t text_cap, uint64_t *counts /* [5] */, void *stream);
/* katome_dev_collapse_unique on the caller's arrays: the labels and offsets of katome_dev_pieces_text (d_label aligned as there), a
 * twin map of n_labels entries as katome_dev_gfa_strand_paths_arrays takes it (all ones: none) and checked by the same rules, the
 * pieces (not NULL when n_pieces > 0) and the layout.  counts[5] = {n_contigs, n_kept, text_bytes, n_mirrored, n_self_mirror} are
 * always set (zeros on an error); d_text NULL: nothing else is written (a size query).  Otherwise d_contig_mirror needs room for
 * contig_cap >= n_contigs entries, d_kept_name / d_kept_off / d_kept_len for kept_cap >= n_kept, and d_text, 16-byte aligned, for
 * text_cap >= text_bytes rounded up to 16 (zeros behind the text up to that multiple): KATOME_E_ARG when one is too small.
 * Validated on the device before anything is read through a value, each KATOME_E_ARG with its message: the twin map (an entry that
 * is neither all ones nor below n_labels, twin(twin(i)) != i), then the pieces and labels as for katome_dev_pieces_text.  2^31
 * pieces or more, or 2^32 - 1 labels or more: KATOME_E_UNSUPPORTED.  KATOME_UNIQUE_TRACE=1 in the environment: the times of the
 * named writer, the selection and the mirror search's parts on stderr.  Synchronises. */
int katome_dev_unique_contigs_arrays(int device, uint32_t k, const uint8_t *d_label, const uint64_t *d_label_off, uint64_t n_labels,
                                     const uint64_t *d_edge_twin, const uint32_t *d_pieces, uint64_t n_pieces, uint32_t layout,
                                     uint64_t *d_contig_mirror /* [n_contigs] */, uint64_t contig_cap,
                                     uint64_t *d_kept_name /* [n_kept] */, uint64_t *d_kept_off /* [n_kept] */,
                                     uint32_t *d_kept_len /* [n_kept] */, uint64_t kept_cap, uint8_t *d_text, uint64_t text_cap,
                                     uint64_t *counts /* [5] */, void *stream);
/* the GFA writer on a numbered PART of a text whose other parts are written elsewhere (katome_dist_contigs_gfa): segment i is named
 * first_segment + i (up to 20 digits), its links are d_link_b[d_link_first[i] .. d_link_first[i + 1]) -- global numbers, n_links =
 * d_link_first[n_edges] --, the header line is written or not.  d_text holds the S part (the header first) at 0 and the L part
 * at *l_offset = *s_bytes rounded up to 16, zeros behind each part up to its multiple of 16; it must be 16-byte aligned with
 * text_cap >= *l_offset + *l_bytes rounded up to 16.  The three sizes are always set; d_text NULL: a size query.  Labels are
 * validated on the device first and d_edge_label is aligned as for katome_dev_gfa_arrays; malformed labels or a d_link_first that
 * does not ascend from 0: KATOME_E_ARG.  first_segment + n_edges past 2^64, or 2^32 - 2 lines or more: KATOME_E_UNSUPPORTED.
 * With first_segment = 0, with_header = 1 and the links of katome_dev_gfa_arrays, the S part followed by the L part is that
 * entry's text byte for byte.  Synchronises. */
int katome_dev_gfa_part_arrays(int device, uint32_t k, uint64_t n_edges, const uint32_t *d_edge_weight, const uint32_t *d_edge_kmers,
                               const uint64_t *d_edge_label_off, const uint8_t *d_edge_label, uint64_t label_bytes,
                               uint64_t first_segment, int with_header,
                               const uint64_t *d_link_first /* [n_edges + 1] */, const uint64_t *d_link_b /* [n_links] global numbers */,
                               uint64_t *d_segment_off, uint8_t *d_text, uint64_t text_cap,
                               uint64_t *s_bytes, uint64_t *l_offset, uint64_t *l_bytes, void *stream);
/* Stats<CollectionStats>::stats for PtGraph (stats/collections.rs:137-168) from device arrays, filled exactly as
 * katome_graph_stats fills it from host arrays: u64 sums, the two averages one f64 division each on the host (no edges:
 * avg_edge_weight is NaN, no nodes: avg_out_degree is NaN, as the reference's 0.0 / 0.0); externals(Incoming) and
 * externals(Outgoing) (pt_graph.rs:64-77) both count isolated nodes; a self-loop counts once in and once out.  n_edges >=
 * 2^32: KATOME_E_UNSUPPORTED.  Every id must be below n_nodes: the caller's contract, NOT checked.  Scratch: 8 bytes per
 * node from the library's allocator (KATOME_E_OOM when there is no room).  Synchronises. */
int katome_dev_stats_arrays(int device, const uint64_t *d_edge_src, const uint64_t *d_edge_dst,
                            const uint32_t *d_edge_weight, uint64_t n_edges, uint64_t n_nodes,
                            katome_stats *out, void *stream);
/* the weight spectrum (the k-mer abundance histogram minimal_weight_threshold and standardize_edges' threshold,
 * standardizer.rs:42-70, are chosen from): bins[w] = records of weight w for w < n_bins - 1, bins[n_bins - 1] = records of
 * weight >= n_bins - 1; the bins add up to n.  2 <= n_bins <= 16384, anything else is KATOME_E_ARG before the device is
 * touched.  Synchronises. */
int katome_dev_weight_spectrum_arrays(int device, const uint32_t *d_weight, uint64_t n,
                                      uint64_t *bins /* host, [n_bins] */, uint32_t n_bins, void *stream);

/* ---- synthetic workload generator (bench/tests; DESIGN.md "Synthetic workload") ---------- */
int katome_dev_synth_reads(int device, uint64_t first_read, uint64_t n_reads, uint32_t read_len,
                           uint64_t genome_len, double err_rate, uint32_t n_inject_percent,
                           uint8_t *d_packed, uint8_t *d_skip, void *stream);

#ifdef __cplusplus
}
#endif
#endif
