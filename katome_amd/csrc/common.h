// common.h -- shared host-side plumbing of libkatome_gpu (error state, HIP checks, device buffers)
#pragma once
#include <hip/hip_runtime.h>
#include <errno.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <chrono>
#include <type_traits>
#include <vector>

#include "../../include/katome_gpu.h"
#include "env.h"
#include "kmer_bits.h"

namespace katome {

// ---- error state (katome_last_error) -------------------------------------------------------
void set_error(const char* fmt, ...);
const char* get_error();

#define KCHECK_HIP(expr)                                                                         \
    do {                                                                                         \
        hipError_t _e = (expr);                                                                  \
        if (_e != hipSuccess) {                                                                  \
            katome::set_error("HIP error %d (%s) at %s:%d: %s", (int)_e, hipGetErrorString(_e),  \
                              __FILE__, __LINE__, #expr);                                        \
            return _e == hipErrorOutOfMemory ? KATOME_E_OOM : KATOME_E_DEVICE;                   \
        }                                                                                        \
    } while (0)

#define KCHECK(expr)                  \
    do {                              \
        int _rc = (expr);             \
        if (_rc != KATOME_OK) return _rc; \
    } while (0)

// caching allocator (mem.cpp): blocks are reused across phases and across builds
int dev_malloc(void** out, size_t bytes, hipStream_t stream);
void dev_free(void* p, hipStream_t stream);
// a live block keeps its first `keep` bytes and gives its tail back to the cache without a copy (mem_pool.h trim); returns the
// block's size afterwards (unchanged where the tail would be too small to keep), 0 for a pointer the cache does not know
size_t dev_trim(void* p, size_t keep);
size_t dev_cached_bytes();
// call before hipStreamDestroy: cached blocks remember the stream they were last used on
void dev_retire_stream(hipStream_t stream);
void dev_release_cache(int device);
void dev_cache_stats(int device, uint64_t out[3]);   // {bytes held from the driver, of them free, live blocks} on `device`

// gfx950 erratum (profiles/r03_shift64_erratum.md, tools/probe_shift64_top_vgpr.hip): v_lshlrev_b64 / v_lshrrev_b64 / v_ashrrev_i64
// with the shift AMOUNT in the last VGPR of the wave's allocation sometimes shift by v0 instead (LLVM's Shift64HighRegBug, worked
// around by the compiler for gfx90a only).  The build checks every kernel's ISA for that shape (tools/scan_shift64_top_vgpr.py, run
// by the Makefile); a kernel it flags -- the amount in v<N>, N = 8n+7 -- puts KATOME_SHIFT64_GUARD(N+1) at its top: naming the next
// register makes the allocation a granule larger, so that the register after the amount exists.
#define KATOME_SHIFT64_GUARD(next_vgpr) asm volatile("" ::: "v" #next_vgpr)

// device buffer with RAII; `stream` is the stream the buffer's users are ordered on
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    hipStream_t stream = nullptr;
    DevBuf() {}
    explicit DevBuf(hipStream_t s) : stream(s) {}
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    int alloc(size_t n) {
        release();
        if (n == 0) n = 16;
        int rc = dev_malloc(&p, n, stream);
        if (rc != KATOME_OK) { p = nullptr; return rc; }
        bytes = n;
        return KATOME_OK;
    }
    int alloc(size_t n, hipStream_t s) { stream = s; return alloc(n); }
    void release() {
        if (p) dev_free(p, stream);
        p = nullptr; bytes = 0;
    }
    // keeps the first `keep` bytes where they are; true: the rest went back to the cache (`bytes` is what the block still holds)
    bool trim(size_t keep) {
        if (!p || keep >= bytes) return false;
        const size_t left = dev_trim(p, keep);
        if (!left || left >= bytes) return false;
        bytes = left;
        return true;
    }
    void* take() { void* q = p; p = nullptr; bytes = 0; return q; }
    void adopt(void* q, size_t n) { release(); p = q; bytes = n; }
    void adopt(DevBuf& from) { const size_t n = from.bytes; adopt(from.take(), n); }      // (neither stream changes)
    template <class T> T* as() const { return (T*)p; }
};

// Optional HIP-event timing on the stream the kernels are launched on (bench.py's roofline figures).  PHASES bracket a step of
// the build (several launches); the K_* entries bracket ONE kernel launch each, so that a kernel's own average duration can be
// priced against its algorithmic bytes -- the free-standing primitives (radix.hip, node_ids.hip, table.hip) find the builder's profiler
// through a thread-local pointer that the enclosing PhaseScope sets.
enum Phase { PH_EXTRACT, PH_REGION_ORDER, PH_INSERT, PH_EMIT_EDGES, PH_SORT_EDGES, PH_NODE_SET, PH_RANK, PH_LABELS,
             PH_INSERT_TILES, PH_EXPAND_TILES, PH_EXPAND_MID, PH_FIRST_SEEN, PH_DEAD_PATHS, PH_SHRINK,
             K_SORT_SCATTER, K_SORT_HIST, K_RUN_SORT, K_HASH_SCATTER, K_HASH_HIST, K_OWNER_SCATTER, K_OWNER_HIST, K_PASS_OFFSETS,
             K_RECORDS, K_GROUP_INDEX, K_LDS_COUNT, K_SRC_IDS, K_DST_MERGE, K_EXPAND, K_SORT_SCATTER_KEYS, K_RUN_SORT_KEYS,
             K_TILE_HASH_SCATTER, K_TILE_HASH_HIST, K_TILE_RECORDS, K_TILE_GROUP_INDEX, K_TILE_LDS_COUNT, K_HALF_MERGE, K_GROUP_MERGE,
             // (appended: the indices above are what callers of katome_phase_name have seen so far)
             PH_GRAPH_STATS, PH_WEIGHT_SPECTRUM, K_STATS_DEGREES, K_STATS_WEIGHTS, K_STATS_NODES, K_SPECTRUM,
             PH_COLLAPSE, K_TEXT_WRITE,
             PH_GFA, K_GFA_SORT, K_GFA_SIZES, K_GFA_WRITE,
             PH_GFA_STRANDS, K_GFAS_KEYS, K_GFAS_SEARCH, K_GFAS_VERIFY, K_GFAS_LINKS, K_GFAS_SIZES, K_GFAS_WRITE,
             PH_GFA_PATHS, K_GFA_PATHS_WRITE,
             PH_GFA_STRAND_PATHS, K_GFASP_WRITE, K_GFASP_SIGS, K_GFASP_SORT, K_GFASP_SEARCH, K_GFASP_VERIFY,
             PH_UNIQUE_CONTIGS, K_TEXT_WRITE_NAMED, K_UNIQUE_SELECT,
             PH_DEPTH, K_DEPTH_KERNEL, K_DEPTH_INDEX,
             PH_COUNT };
static const char* const PHASE_NAMES[PH_COUNT] = {
    "extract", "region_order", "insert", "emit_edges", "sort_edges", "node_set", "rank", "labels", "insert_tiles", "expand_tiles",
    "expand_mid_tiles", "first_seen_order", "remove_dead_paths", "shrink",
    "k:radix_scatter_kernel<RadixDigit>", "k:radix_hist_kernel<RadixDigit>", "k:run_sort", "k:radix_scatter_kernel<HashDigit>",
    "k:radix_hist_kernel<HashDigit>", "k:radix_scatter_kernel<OwnerDigit>", "k:radix_hist_kernel<OwnerDigit>", "k:radix_chunk+offsets",
    "k:tiles_to_records_kernel", "k:hash_group_index_kernel", "k:lds_count_kernel", "k:src_count+src_write", "k:dst_merge_kernel",
    "k:expand_tiles_kernel",
    // (the keys-only instantiations -- the small sort of the nodes without out-edges -- are kernels of their own in a trace)
    "k:radix_scatter_kernel<RadixDigit> (keys only)", "k:run_sort (keys only)",
    // (the same kernels counting a TILE level by sorting -- other record sizes, so timed apart: TileLevelScope)
    "k:radix_scatter_kernel<HashDigit> (tile records)", "k:radix_hist_kernel<HashDigit> (tile records)", "k:tiles_to_records_kernel (tile records)",
    "k:hash_group_index_kernel (tile records)", "k:lds_count_kernel (tile records)", "k:half_merge_kernel",
    "k:group_merge_kernel",
    "graph_stats", "weight_spectrum", "k:stats_degree_kernel", "k:stats_weight_kernel", "k:stats_node_kernel", "k:spectrum_kernel",
    "collapse", "k:text_write_kernel",
    "gfa", "k:gfa link sort", "k:gfa sizes", "k:gfa_write_kernel",
    "gfa_strands", "k:gfa_strands keys+sort", "k:strand_search_kernel", "k:strand_verify_kernel", "k:gfa_strands links", "k:gfa_strands sizes", "k:gfa_strands_write_kernel",
    "gfa_paths", "k:gfa_paths_write_kernel",
    "gfa_strand_paths", "k:gfa_strand_paths_write_kernel", "k:mirror_sig_kernel", "k:mirror signature sort", "k:mirror_search_kernel", "k:mirror_verify_kernel",
    "unique_contigs", "k:text_write_named_kernel", "k:unique_contigs selection",
    "depth", "k:depth_kernel", "k:depth_index"};
struct Profiler {
    bool on = false;
    struct Ev { int phase; hipEvent_t a, b; uint64_t work; };      // work: elements the launch processed (K_* entries)
    std::vector<Ev> evs;
    ~Profiler() { clear(); }
    void clear() { for (auto& e : evs) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); } evs.clear(); }
};
inline Profiler*& current_profiler() { static thread_local Profiler* p = nullptr; return p; }
struct PhaseScope {
    Profiler* p; hipStream_t s; hipEvent_t a = nullptr, b = nullptr; int phase; Profiler* outer;
    PhaseScope(Profiler& prof, int ph, hipStream_t st) : p(prof.on ? &prof : nullptr), s(st), phase(ph), outer(current_profiler()) {
        if (p && hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess) (void)hipEventRecord(a, s); else p = nullptr;
        if (p) current_profiler() = p;
    }
    ~PhaseScope() { if (p) { (void)hipEventRecord(b, s); p->evs.push_back({phase, a, b, 0}); current_profiler() = outer; } }
};
// while one of these is alive on the thread, the record/count kernels report to the K_TILE_* timers: a tile level counted by
// sorting runs the last level's kernels on records of another size, and a timer prices ONE record size
inline bool& counting_tile_level() { static thread_local bool on = false; return on; }
struct TileLevelScope {
    bool outer;
    TileLevelScope() : outer(counting_tile_level()) { counting_tile_level() = true; }
    ~TileLevelScope() { counting_tile_level() = outer; }
};
inline int tile_level_timer(int ph) {
    if (!counting_tile_level()) return ph;
    switch (ph) {
        case K_HASH_SCATTER: return K_TILE_HASH_SCATTER;
        case K_HASH_HIST:    return K_TILE_HASH_HIST;
        case K_RECORDS:      return K_TILE_RECORDS;
        case K_GROUP_INDEX:  return K_TILE_GROUP_INDEX;
        case K_LDS_COUNT:    return K_TILE_LDS_COUNT;
        default:             return ph;
    }
}
// one kernel launch (or a couple of tiny ones) inside a phase; a no-op unless a profiling PhaseScope is open on this thread
struct KernelScope {
    Profiler* p; hipStream_t s; hipEvent_t a = nullptr, b = nullptr; int phase; uint64_t work;
    KernelScope(int ph, hipStream_t st, uint64_t elements = 0) : p(current_profiler()), s(st), phase(tile_level_timer(ph)), work(elements) {
        if (p && hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess) (void)hipEventRecord(a, s); else p = nullptr;
    }
    ~KernelScope() { if (p) { (void)hipEventRecord(b, s); p->evs.push_back({phase, a, b, work}); } }
};

inline int use_device(int device) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        set_error("no HIP device available (%s): this library has no CPU fallback",
                  e == hipSuccess ? "device count 0" : hipGetErrorString(e));
        (void)hipGetLastError();
        return KATOME_E_DEVICE;
    }
    if (device < 0 || device >= n) { set_error("device ordinal %d out of range (0..%d)", device, n - 1); return KATOME_E_DEVICE; }
    KCHECK_HIP(hipSetDevice(device));
    return KATOME_OK;
}

inline int check_k(uint32_t k) {
    if (k <= 1) { set_error("assertion failed: k_size > 1"); return KATOME_E_ARG; }   // prelude.rs:35
    if (k < 3 || k > 63) { set_error("k = %u unsupported (3..63)", k); return KATOME_E_UNSUPPORTED; }   // valid for the reference, not here
    return KATOME_OK;
}

constexpr int BLOCK = 256;
#ifdef __HIPCC__
__device__ __forceinline__ u32 wave_sum(u32 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}
#endif
inline unsigned grid_for(uint64_t work_items, unsigned per_block, unsigned cap = 256u * 16u) {
    uint64_t g = (work_items + per_block - 1) / per_block;
    if (g < 1) g = 1;
    return (unsigned)(g > cap ? cap : g);
}
// a grid-stride kernel over n items: workgroups of BLOCK, at most 32 per compute unit
#define KLAUNCH(kernel, n, stream, ...) hipLaunchKernelGGL(kernel, dim3(grid_for((n), BLOCK, 256u * 32u)), dim3(BLOCK), 0, stream, __VA_ARGS__)
// wall clock, for the stage traces and the host_ms / total_ms of the stats
inline double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// a run-time flag as a template argument: f gets it as a std::integral_constant (kernel<decltype(flag)::value>) and returns a status
template <bool B> using BoolC = std::integral_constant<bool, B>;
template <int I> using IntC = std::integral_constant<int, I>;
template <class F> int with_bool(bool b, F f) { return b ? f(BoolC<true>{}) : f(BoolC<false>{}); }

// ---- launchers implemented in the .hip files (all asynchronous on `stream`) -----------------
int launch_extract_fixed(uint32_t k, bool rc, const uint8_t* d_packed, uint64_t n_reads, uint32_t read_len,
                         const uint8_t* d_skip, uint64_t* d_records, hipStream_t stream, uint32_t span = 1, bool mark = false,
                         uint32_t first_window = 0, uint32_t records_per_read = 0);
// (the tiles of a batch of clean reads written where they are kept, with the first partition pass's digit counts per sort tile: extract.hip)
bool extract_tile_counts_ok(uint32_t k, uint32_t read_len, uint32_t span, uint32_t sort_tile, const uint8_t* d_packed, const uint64_t* d_records);
int launch_extract_tiles_counted(uint32_t k, bool rc, const uint8_t* d_packed, uint64_t n_reads, uint32_t read_len, uint32_t span,
                                 uint64_t* d_records, uint32_t* d_counts, uint32_t sort_tile, hipStream_t stream);
int launch_extract_var(uint32_t k, bool rc, const uint8_t* d_packed, uint64_t packed_bytes, const uint64_t* d_byte_off,
                       const uint32_t* d_len, const uint64_t* d_win_prefix, uint64_t n_reads, uint64_t total_windows,
                       uint64_t* d_records, hipStream_t stream, bool mark = false, uint32_t span = 1, uint32_t mode = 0);

// radix.hip
int dev_sort(uint64_t* d_keys, uint32_t* d_vals, uint64_t n, uint32_t nw, uint32_t key_bits, hipStream_t stream);
struct DevBuf;
// (distinct_keys: no two keys are equal -- the first pass then need not be stable: radix.hip)
int dev_sort_bufs(DevBuf& keys, DevBuf* vals, uint64_t n, uint32_t nw, uint32_t key_bits, hipStream_t stream, bool distinct_keys = false);
int dev_partition(const uint64_t* d_in, const uint32_t* v_in, uint64_t n, uint32_t nw, uint32_t n_parts, uint64_t* d_out,
                  uint32_t* v_out, uint64_t* h_counts, hipStream_t stream, uint32_t core_shift = 0, uint32_t core_bases = 0, uint32_t minimizer = 0);
// supermer.hip: the sharded build's exchange unit
constexpr uint32_t SUPERMER_M = 11;        // bases of the minimizer that names a k-mer's owner on the supermer route
uint32_t supermer_slots(uint32_t k, uint32_t read_len, uint32_t m);
bool supermer_route_takes(uint32_t k, uint32_t read_len, uint32_t m);
int dev_supermers_extract(const uint8_t* d_packed, uint64_t n_reads, uint32_t read_len, const uint8_t* d_skip, uint32_t k, uint32_t m, bool rc,
                          uint32_t n_owners, uint32_t slots, uint64_t* d_out, uint64_t* d_spill, uint64_t spill_cap, uint64_t* d_spill_cursor,
                          hipStream_t stream);
int dev_supermers_expand(const uint64_t* d_list, const uint32_t* d_counts, uint64_t n, uint32_t k, bool rc, DevBuf& keys, DevBuf& weights,
                         uint64_t* n_records, hipStream_t stream);
int dev_partition_supermers(const uint64_t* d_in, uint64_t n, uint32_t n_parts, uint64_t* d_out, uint64_t* h_counts, hipStream_t stream);
int dev_partition_range(const uint64_t* d_vals, const uint32_t* idx_in, uint64_t n, const uint64_t* d_bounds, uint32_t n_parts,
                        uint64_t* d_out, uint32_t* idx_out, uint64_t* h_counts, hipStream_t stream);
int dev_hash_order_core(const uint64_t* d_in, const uint32_t* w_in, uint64_t n, uint32_t core_shift, uint32_t core_bases, uint64_t* ka, uint64_t* kb,
                        uint32_t* wa, uint32_t* wb, const uint64_t** k_out, const uint32_t** w_out, uint32_t* group_bits, hipStream_t stream);
// KATOME_FUSED_RECORDS=0: a list-fed level's records are written out before their first partition pass, as they were before that pass
// could cut them out of the list itself
inline bool fused_records_on() { static const bool on = env_flag("KATOME_FUSED_RECORDS", true); return on; }
// KATOME_ENTRY_CUT=0: the kernels that make such records off the list (radix.hip ListSource, table.hip list_digit_counts_kernel) cut
// them once per record, as they did before entry_cut.h, instead of once per list entry
inline bool entry_cut_on() { static const bool on = env_flag("KATOME_ENTRY_CUT", true); return on; }
// A level's records that are not written yet (table_list_to_records with a RecordSource): record p is sub-window p % span of list
// entry p / span, in its level's orientation, with that entry's count.  While `pending`, *keys / *weights are not allocated; the first
// partition pass (dev_key_order, dev_hash_order) makes its tiles from the list, gives the list up where the source owns it
// (own_tiles / own_counts: a list that would otherwise be gone by then) and only then allocates *keys / *weights, the second pass's
// destination -- after the two passes the records lie ordered there exactly as if they had been written first.  Whoever wants the
// records BEFORE the first pass calls table_materialise_records, which writes them (list_to_records_kernel) and ends `pending`.
struct RecordSource {
    const uint64_t* tiles = nullptr; const uint32_t* counts = nullptr;
    uint64_t n_tiles = 0;
    uint32_t tile_bases = 0, k = 0, span = 0, stride = 0;
    bool rc = false, rep = false, pending = false;
    DevBuf* keys = nullptr; DevBuf* weights = nullptr;      // where the records go, and how large those buffers are to be
    size_t key_bytes = 0, weight_bytes = 0;
    hipStream_t stream = nullptr;
    DevBuf own_tiles, own_counts;
    // (test entry katome_dev_count_in_key: where dev_hash_order leaves copies of the records after its first and its second pass, as
    // plain keys and weights whichever form they travel in)
    uint64_t* tap_keys[2] = {nullptr, nullptr}; uint32_t* tap_weights[2] = {nullptr, nullptr};
    uint64_t n_records() const { return n_tiles * span; }
    // the first pass is launched: the list is not needed again, the records' buffers are
    int first_pass_done() {
        pending = false; tiles = nullptr; counts = nullptr;
        own_tiles.release(); own_counts.release();
        if (int rc = keys->alloc(key_bytes, stream)) return rc;
        return weight_bytes ? weights->alloc(weight_bytes, stream) : (int)KATOME_OK;      // (0: the counts ride in the keys, counted_key.h)
    }
};
// which lists the first pass can take its records from: two-word tiles into two-word sub-tiles ordered by hash, and one- or two-word
// tiles into one-word k-mers in their representative orientation ordered by key (the two list-fed levels of a build with k <= 31)
bool fused_records_takes(uint32_t nwt, uint32_t nwk, bool rep, uint32_t span);
int table_materialise_records(RecordSource& src);
// (first_counts of the three order calls below: the first pass's digit counts per tile, made by whoever wrote the records.  The pass
// works IN that buffer and leaves prefixes there: its contents are gone after the call, and no caller reads them again)
int dev_hash_order_tagged(const uint64_t* d_in, const uint32_t* w_in, uint64_t n, uint32_t nwk, uint64_t* ka, uint64_t* kb, uint32_t* wa, uint32_t* wb,
                          const uint64_t** k_out, const uint32_t** w_out, uint32_t* group_bits, hipStream_t stream, uint32_t* first_counts = nullptr);
int dev_region_order(const uint64_t* d_in, const uint32_t* w_in, uint64_t n, uint32_t nw, int passes, uint64_t* ka, uint64_t* kb,
                     uint32_t* wa, uint32_t* wb, const uint64_t** k_out, const uint32_t** w_out, hipStream_t stream);
int dev_hash_order(const uint64_t* d_in, const uint32_t* w_in, uint64_t n, uint32_t nw, uint64_t* ka, uint64_t* kb, uint32_t* wa, uint32_t* wb,
                   const uint64_t** k_out, const uint32_t** w_out, uint32_t* group_bits, hipStream_t stream, uint32_t* first_counts = nullptr,
                   RecordSource* src = nullptr);
// (true: dev_hash_order makes the records of src with their count in the key word, counted_key.h -- *w_out comes back
// null, no weights buffer is touched, and what *k_out points at is unpacked with dev_counted_unpack or counted as it is)
bool dev_hash_order_counts_in_key(const RecordSource* src, uint32_t nw, const uint32_t* first_counts);
void dev_count_in_key_force(int v);          // (test entry: 0 / 1 -- the route whatever KATOME_COUNT_IN_KEY says; -1 -- the switch again)
// test entry (katome_dev_count_in_key): a list-fed two-word level from the list to the list of distinct (key, count), as
// tile_recs_to_kmer_records runs its mid level.  packed: 1 the counted-key route where the level fits, 0 plain keys and weights.
// d_pass_keys / d_pass_weights (two each, null: not wanted): the records after the first and the second partition pass, unpacked.
// d_out_keys / d_out_weights: room for n_tiles * span entries; *n_out distinct keys.  *took_packed: which form the records took.
int dev_count_in_key_level(const uint64_t* d_tiles, const uint32_t* d_counts, uint64_t n_tiles, uint32_t tile_bases, uint32_t k, uint32_t span, uint32_t stride,
                           bool rc, bool packed, uint64_t* const d_pass_keys[2], uint32_t* const d_pass_weights[2], uint64_t* d_out_keys,
                           uint32_t* d_out_weights, uint64_t* n_out, int* took_packed, hipStream_t stream);
int dev_counted_unpack(const uint64_t* d_in, uint64_t n, uint64_t* d_keys, uint32_t* d_weights, hipStream_t stream);
// (src, here and in dev_key_order: records still to be made -- d_in / w_in and the second destination kb / wb are then taken from the
// source once its first pass is launched, and first_counts are the counts table_list_to_records made for it)
uint32_t dev_sort_tile_keys(uint32_t nw);
// KATOME_FUSED_HIST=0: whoever writes a level's records does not count the first pass's digits per tile; the pass counts them itself
inline bool fused_hist_on() { static const bool on = env_flag("KATOME_FUSED_HIST", true); return on; }
// one-word records by their leading 16 key bits (k = 8..32): two stable passes; the result where *k_out / *w_out point (kb / wb)
// (first_digits: the first pass's digit of every record -- bits 2k - 16 .. 2k - 9 of its key --, one byte each at the record's index in
// a buffer of dev_digit_stream_bytes(n, 1) bytes, left by whoever wrote the records; the pass then counts from them, not the keys)
int dev_key_order(const uint64_t* d_in, const uint32_t* w_in, uint64_t n, uint32_t k, uint64_t* ka, uint64_t* kb, uint32_t* wa, uint32_t* wb,
                  const uint64_t** k_out, const uint32_t** w_out, hipStream_t stream, uint32_t* first_counts = nullptr,
                  const uint8_t* first_digits = nullptr, RecordSource* src = nullptr);
// test entry (katome_dev_list_first_pass): the records of a list after their first partition pass, in d_keys / d_weights, and that
// pass's digit counts per tile in d_counts -- fused: the count-only kernel and the pass that makes its tiles from the list; otherwise
// list_to_records_hist_kernel and the pass over the written records
int dev_list_first_pass(const uint64_t* d_tiles, const uint32_t* d_counts, uint64_t n_tiles, uint32_t tile_bases, uint32_t k, uint32_t span, uint32_t stride,
                        bool rc, bool rep, bool fused, uint64_t* d_keys, uint32_t* d_weights, uint32_t* d_digit_counts, hipStream_t stream);
// One-word (key, count) records lying in the 256 regions of s2_regions.h -- region d from start[d] on, used[d] of them, all of first
// digit d; digits: bits 2k - 8 .. 2k - 1 of every key, one byte each at the key's index -- partitioned by those bits into k_out /
// w_out, dense and stable: the regions in digit order, so that the 16-bit groups come out contiguous.  Counts its tiles from the
// bytes.  *n_tiles: the tiles the pass walked.  (katome_dev_s2_region_pass is its test entry)
int dev_s2_region_pass(const uint64_t* d_keys, const uint32_t* d_w, const uint8_t* d_digits, uint32_t k, const uint64_t* start, const uint64_t* used,
                       uint64_t* k_out, uint32_t* w_out, uint64_t* n_tiles, hipStream_t stream);
size_t dev_digit_stream_bytes(uint64_t n, uint32_t nw);
bool dev_digit_stream_pays(uint32_t nw);        // do records of nw words get a digit stream between their two partition passes?
// index[g] (65537 of them) = first of n ascending one-word keys whose bits [shift, shift + 16) are >= g
int dev_key_group_index(const uint64_t* d_keys, uint64_t n, uint32_t shift, uint64_t* d_index, hipStream_t stream);
// merges, per 16-bit key prefix g, a_count[g] ascending keys at a_key + a_first[g] with the sorted b_key[b_first[g] .. b_first[g + 1])
// into out + a_off[g] + b_first[g] (a_off: exclusive sums of a_count)
int dev_half_merge(const uint64_t* a_key, const uint32_t* a_w, const uint64_t* a_first, const uint32_t* a_count, const uint64_t* a_off,
                   const uint64_t* b_key, const uint32_t* b_w, const uint64_t* b_first, uint64_t* out_key, uint32_t* out_w, uint64_t n_out,
                   hipStream_t stream);
// the same without a sort of B: b_key / b_w only partitioned by the 16-bit prefix (dev_key_order), at most dev_group_merge_cap() keys
// to a prefix (dev_key_group_max), weights below 2^16; B's groups are put in key order in LDS (radix.hip group_merge_kernel)
// (head_counts, dev_source_head_blocks(n_out) of them: also counts the source run heads of every block of output edges, which
// dev_node_ids, node_ids.hip, then need not count again)
uint32_t dev_group_merge_cap();
uint64_t dev_source_head_blocks(uint64_t n_edges);
int dev_group_merge(const uint64_t* a_key, const uint32_t* a_w, const uint64_t* a_first, const uint32_t* a_count, const uint64_t* a_off,
                    const uint64_t* b_key, const uint32_t* b_w, const uint64_t* b_first, uint32_t k, uint64_t* out_key, uint32_t* out_w,
                    uint64_t n_out, hipStream_t stream, uint32_t* head_counts = nullptr);
// *d_out = the largest index[g + 1] - index[g], g < 65536 (the largest group of a dev_key_group_index)
int dev_key_group_max(const uint64_t* d_index, uint64_t* d_out, hipStream_t stream);
int dev_unique(uint64_t* d_keys, uint64_t n, uint32_t nw, uint64_t* n_out, hipStream_t stream);
int dev_rank(const uint64_t* d_sorted, uint64_t n_sorted, uint32_t nw, uint32_t key_bits, const uint64_t* d_q, uint64_t nq,
             uint64_t* d_out, hipStream_t stream);
// dev_rank's index over the top B of key_bits bits of n ascending keys: d_index[b] ((1 << B) + 1 of them) = first key whose top bits are >= b
int dev_bucket_index(const uint64_t* d_sorted, uint64_t n, uint32_t nw, uint32_t key_bits, uint32_t B, uint64_t* d_index, hipStream_t stream);
int dev_iota(uint32_t* d, uint64_t n, hipStream_t stream);
int dev_fill_u32(uint32_t* d, uint64_t n, uint32_t v, hipStream_t stream);
int dev_gather_seq_weight(const uint64_t* pairs, const uint32_t* idx, uint64_t n, uint64_t* seq, uint32_t* weight, hipStream_t stream);
int dev_gather_u32(const uint32_t* src, const uint32_t* idx, uint64_t n, uint32_t* dst, hipStream_t stream);
int dev_gather_u64(const uint64_t* src, const uint32_t* idx, uint64_t n, uint64_t* dst, hipStream_t stream);
int dev_gather_keys(const uint64_t* src, const uint32_t* idx, uint64_t n, uint32_t nw, uint64_t* dst, hipStream_t stream);
// exclusive scan of m u32 counts into u64 offsets (offs[m] = total), one workgroup
int dev_scan_counts(const uint32_t* d_counts, uint64_t m, uint64_t* d_offs, hipStream_t stream);

// node_ids.hip: the graph read off the sorted edge list
int dev_source_ids(const uint64_t* d_edge_key, uint64_t n_edges, uint32_t k, DevBuf& node_key, uint64_t* d_edge_src, uint64_t* n_src,
                   hipStream_t stream);
// d_seq + node_first (first-seen order): also the nodes' first touches, filled on the way; node_first comes back EMPTY when that was
// not done (dev_first_seen_order then fills it)
// head_counts: dev_group_merge's, made for exactly these edges (the heads are then not counted again); d_label: the edges' labels
// (dev_labels' bytes) are written in the same pass as the source ids
int dev_node_ids(const uint64_t* d_edge_key, uint64_t n_edges, uint32_t k, DevBuf& node_key, uint64_t* d_edge_src,
                 uint64_t* d_edge_dst, uint64_t* n_nodes, hipStream_t stream, const uint64_t* d_seq = nullptr, DevBuf* node_first = nullptr,
                 uint64_t* n_marked = nullptr, const uint32_t* head_counts = nullptr, uint8_t* d_label = nullptr);
int dev_endpoints(const uint64_t* d_edge_key, uint64_t n, uint32_t k, uint64_t* d_src, uint64_t* d_dst, hipStream_t stream);
int dev_labels(const uint64_t* d_edge_key, uint64_t n, uint32_t k, uint8_t* d_label, hipStream_t stream);
// BFCounter lines -> one edge per line (and per strand), unmerged (pt_graph.rs:201-213); seq (nullable) = petgraph index
int dev_bfc_edges(const uint64_t* d_fwd, const uint32_t* d_w, uint64_t n, uint32_t k, bool rc, uint64_t* d_edge_key,
                  uint32_t* d_edge_weight, uint64_t* d_edge_seq, hipStream_t stream);

// first_seen.hip: first-seen order (pt_graph.rs:149,194) -- edges to the order of their first insertion (edge_seq, below 2^seq_bits,
// comes back ascending), nodes to the order of their first touch; counts stay, buffers are replaced.  node_first, n_marked: what
// dev_node_ids left (node_first is given back on the way)
struct FirstSeenGraph { DevBuf *edge_key, *edge_weight, *edge_src, *edge_dst, *edge_seq, *node_key; uint64_t n_edges, n_nodes; uint32_t nw, k; };
int dev_first_seen_order(FirstSeenGraph& g, DevBuf& node_first, uint64_t n_marked, uint32_t seq_bits, hipStream_t stream);

// prune.hip: Prunable::remove_dead_paths on a first-seen-ordered graph, in place (counts shrink, buffers stay)
struct PruneGraph {
    DevBuf *edge_src, *edge_dst, *edge_weight, *edge_key, *node_key;
    DevBuf *edge_age;      // u32 per edge: its first-seen index = its place in petgraph's adjacency lists (swap_remove re-labels
                           // edges but never reorders the lists); empty = the edges still sit at their first-seen positions
    uint64_t n_edges, n_nodes;
    uint32_t nw;
    bool parallel_edges = false;   // BFCounter graphs may hold the same k-mer on several edges: no per-base adjacency slots then
};
// scratch of dev_replay_edges, kept across the passes of remove_dead_paths
struct ReplayScratch {
    DevBuf agg, carry, size_before, jump, totals;
    explicit ReplayScratch(hipStream_t stream) : agg(stream), carry(stream), size_before(stream), jump(stream), totals(stream) {}
};
int dev_replay_edges(const uint32_t* d_pos, const uint32_t* d_mult, uint64_t u, uint64_t n_edges, ReplayScratch& scratch, DevBuf& victims,
                     DevBuf& move_to, DevBuf& move_from, uint64_t* n_removed, uint64_t* n_left, uint64_t* n_moves, uint64_t* n_dups,
                     hipStream_t stream);
int dev_replay_edges64(const uint64_t* d_pos, const uint32_t* d_mult, uint64_t u, uint64_t n_edges, ReplayScratch& scratch, DevBuf& victims,
                       DevBuf& move_to, DevBuf& move_from, uint64_t* n_removed, uint64_t* n_left, uint64_t* n_moves, uint64_t* n_dups,
                       hipStream_t stream);
struct NodeReplayScratch {
    DevBuf counts, offs, first, hole, dead, flags;
    explicit NodeReplayScratch(hipStream_t stream) : counts(stream), offs(stream), first(stream), hole(stream), dead(stream), flags(stream) {}
};
int dev_replay_nodes(const uint32_t* d_die, uint64_t m, uint64_t n_nodes, NodeReplayScratch& scratch, DevBuf& move_to, DevBuf& move_from,
                     uint64_t* n_moves, uint64_t* n_left, int* fell_back, hipStream_t stream);
int dev_replay_nodes64(const uint64_t* d_die, uint64_t m, uint64_t n_nodes, NodeReplayScratch& scratch, DevBuf& move_to, DevBuf& move_from,
                       uint64_t* n_moves, uint64_t* n_left, int* fell_back, hipStream_t stream);
int dev_remove_dead_paths(PruneGraph& g, uint32_t k, katome_prune_stats* st, hipStream_t stream);
// Clean::remove_weak_edges with petgraph's retain_edges / retain_nodes numbering, same graph, in place
int dev_remove_weak_edges_ordered(PruneGraph& g, uint32_t threshold, hipStream_t stream);

// standardize.hip: Standardizable (standardizer.rs:41-128)
int dev_standardize_contigs(const uint64_t* src, const uint64_t* dst, uint32_t* weight, uint64_t E, uint64_t N, hipStream_t stream);
int dev_standardize_scale(uint32_t* weight, uint64_t E, uint64_t original_genome_length, uint32_t k, uint32_t threshold, hipStream_t stream);
// its parts, for the sharded form (dist_stages.hip), which sums over all ranks in between
int dev_weight_sums(const uint32_t* weight, uint64_t E, uint32_t threshold, uint64_t sums[2], hipStream_t stream);
double standardization_ratio(uint64_t original_genome_length, uint32_t k, const uint64_t sums[2]);
int dev_scale_weights(uint32_t* weight, uint64_t E, double p, uint32_t threshold, hipStream_t stream);

// stats.hip: Stats<CollectionStats> for PtGraph (stats/collections.rs:137-168) and the weight spectrum
int dev_graph_stats(const uint64_t* src, const uint64_t* dst, const uint32_t* weight, uint64_t E, uint64_t N, katome_stats* out, hipStream_t stream);
int check_spectrum_bins(const uint64_t* bins, uint32_t n_bins);       // 2 <= n_bins <= 16384 and somewhere to put them, else KATOME_E_ARG
int dev_weight_spectrum(const uint32_t* weight, uint64_t n, uint64_t* bins, uint32_t n_bins, hipStream_t stream);      // (bins: host)
// their parts, for the sharded form (dist_stats.hip), which reduces over all ranks in between.  d_res: STATS_WORDS u64 on the
// device, zeroed by the caller: {weight sum, max weight, max in-degree, max out-degree, nodes without in-edges, nodes without
// out-edges, out-degree sum}; d_deg: one word per node, in-degree in the low half, out-degree in the high half
constexpr int STATS_WORDS = 8;
int dev_weight_max_sum(const uint32_t* weight, uint64_t n, uint64_t* d_res, hipStream_t stream);
int dev_degree_reduce(const uint64_t* d_deg, uint64_t N, uint64_t* d_res, hipStream_t stream);
void fill_stats(uint64_t n_nodes, uint64_t n_edges, const uint64_t res[STATS_WORDS], katome_stats* out);

// shrink.hip: Shrinkable::shrink (shrinker.rs:165-209) on a finalized graph; the result lives in its own buffers
struct ShrinkInput {
    const uint64_t *edge_src, *edge_dst; const uint32_t* edge_weight; const uint64_t *edge_key, *node_key;
    uint64_t n_edges, n_nodes; uint32_t nw, k;
};
struct ShrinkOutput {
    DevBuf edge_src, edge_dst, edge_weight, edge_kmers, edge_label_off, edge_label, node_key;
    uint64_t n_edges = 0, n_nodes = 0, label_bytes = 0;
};
// what a shrink with coverage leaves beside its result: per merged edge the sum (64 bits: the graph's u32 weights add up without
// wrapping), the smallest and the largest of the weights of the input edges on its path.  valid: they belong to the last shrink
struct ShrinkCoverage {
    DevBuf kmer_sum, kmer_min, kmer_max;
    uint64_t n_edges = 0;
    bool valid = false;
    void drop() { kmer_sum.release(); kmer_min.release(); kmer_max.release(); n_edges = 0; valid = false; }
};
int dev_shrink(const ShrinkInput& g, ShrinkOutput& out, hipStream_t stream, ShrinkCoverage* cov = nullptr);
// the reference's own result: its cuts and petgraph's numbering (shrink_exact.h on the host for the order, the device for the bytes)
// (keep / kept: the caller's ShrinkExact is used and left as run() leaves it, with the nodes it kept -- where collapse starts)
struct ShrinkExact;
int dev_shrink_exact(const ShrinkInput& g, const uint32_t* edge_age, ShrinkOutput& out, double* host_ms, hipStream_t stream,
                     ShrinkExact* keep = nullptr, std::vector<uint32_t>* kept = nullptr, ShrinkCoverage* cov = nullptr);

// collapse.hip: Collapsable::collapse (collapser.rs:25-273): the walk on the host (collapse_exact.h), the text on the device
struct TextOutput {
    DevBuf contig_off, contig_len, text;
    uint64_t n_contigs = 0, text_bytes = 0;
    uint32_t layout = 0;
};
// (first_contig: contig c's FASTA header reads ">katome_<first_contig + c>"; first_contig + the contigs past 2^64: KATOME_E_UNSUPPORTED)
// sizes of the text of `n_pieces` pieces over `n_labels` labels (validated on the device first): every piece's contig (contig_idx) and output offset (piece_off), both scanned, one entry more than pieces
struct TextPlan {
    DevBuf contig_idx, piece_off;
    uint64_t n_contigs = 0, text_bytes = 0;
};
// (names, optional, device, one per contig: contig c's header reads ">katome_<names[c]>" instead -- first_contig is then not looked at;
// the same list goes to both calls)
int dev_text_plan(uint32_t k, const uint8_t* label, const uint64_t* label_off, uint64_t n_labels, const uint32_t* pieces, uint64_t n_pieces,
                  uint32_t layout, uint64_t first_contig, TextPlan& plan, hipStream_t stream, const uint64_t* names = nullptr);
int dev_text_write(uint32_t k, const uint8_t* label, const uint64_t* label_off, const uint32_t* pieces, uint64_t n_pieces, uint32_t layout,
                   uint64_t first_contig, const TextPlan& plan, uint64_t* contig_off, uint32_t* contig_len, uint8_t* text, hipStream_t stream,
                   const uint64_t* names = nullptr);
int dev_pieces_text(uint32_t k, const uint8_t* label, const uint64_t* label_off, uint64_t n_labels, const uint32_t* pieces, uint64_t n_pieces,
                    uint32_t layout, uint64_t first_contig, TextOutput& out, hipStream_t stream);
// (keep_pieces, optional: the device piece list, n_pieces u32, is handed over instead of freed -- katome_dev_collapse_gfa reads it)
int dev_collapse(const ShrinkInput& g, const uint32_t* edge_age, ShrinkOutput& shrunk, uint32_t layout, TextOutput& out,
                 katome_collapse_stats* stats, std::vector<uint64_t>* lengths, hipStream_t stream, DevBuf* keep_pieces = nullptr,
                 uint64_t* n_pieces = nullptr);

// gfa.hip: a shrink result as GFA 1 (include/katome_gpu.h has the format): the join of every edge into a vertex with every edge out
// of it, the records' sizes and the text, partitioned by output bytes
// (optional: per segment the sum, smallest and largest of its path's k-mer counts -- all three or none; with them KC is the sum and
// every S line ends in mn / mx)
struct GfaCoverage {
    const uint64_t* kmer_sum = nullptr; const uint32_t *kmer_min = nullptr, *kmer_max = nullptr;
    bool any() const { return kmer_sum || kmer_min || kmer_max; }
    bool all() const { return kmer_sum && kmer_min && kmer_max; }
};
struct GfaGraph {
    uint32_t k; uint64_t n_nodes, n_edges;
    const uint64_t *edge_src, *edge_dst; const uint32_t *edge_weight, *edge_kmers;
    const uint64_t* label_off; const uint8_t* label; uint64_t label_bytes;
    GfaCoverage cov = {};
};
// what dev_gfa_plan leaves for the writer: every line's offset (line 0 the header, 1 + i segment i, 1 + n_edges + l link l; one entry
// more than lines), every segment's first base, every segment's first link (n_edges + 1), every link's two segments
struct GfaPlan {
    DevBuf line_off, segment_off, link_first, link_ab;
    uint64_t n_links = 0, text_bytes = 0;
};
struct GfaOutput {
    DevBuf text, segment_off, link_first;
    uint64_t n_segments = 0, n_links = 0, text_bytes = 0;
};
int dev_gfa_plan(const GfaGraph& g, GfaPlan& plan, hipStream_t stream);                         // validates, joins, measures; synchronises
int dev_gfa_validate(const GfaGraph& g, hipStream_t stream);                                    // dev_gfa_plan's checks alone; synchronises
int dev_gfa_write(const GfaGraph& g, const GfaPlan& plan, uint8_t* text, hipStream_t stream);  // text: plan.text_bytes rounded up to 16
int dev_gfa(const GfaGraph& g, GfaOutput& out, hipStream_t stream);
// a numbered part of a GFA text whose other parts are written elsewhere (dist_gfa.hip): segment i is named first_segment + i, the
// links of segment a are link_b[link_first[a] .. link_first[a + 1]) (global numbers); the header line is there or not.  The part's
// text is one buffer: the S part (with the header) at 0, the L part at l_offset(), the next multiple of 16, zeros behind each
struct GfaPart {
    uint32_t k; uint64_t n_edges;
    const uint32_t *edge_weight, *edge_kmers; const uint64_t* label_off; const uint8_t* label; uint64_t label_bytes;
    uint64_t first_segment; bool with_header;
    const uint64_t *link_first, *link_b;
    GfaCoverage cov = {};
};
struct GfaPartPlan {
    DevBuf s_line_off, l_line_off, segment_off, link_a;      // line offsets of the two parts (one entry more than lines); every link's local a
    uint64_t n_links = 0, s_bytes = 0, l_bytes = 0;
    uint64_t l_offset() const { return (s_bytes + 15) / 16 * 16; }
    uint64_t buffer_bytes() const { return l_offset() + (l_bytes + 15) / 16 * 16; }
};
int dev_gfa_part_plan(const GfaPart& g, GfaPartPlan& plan, hipStream_t stream);                        // validates, measures; synchronises
int dev_gfa_part_write(const GfaPart& g, const GfaPartPlan& plan, uint8_t* text, hipStream_t stream);  // text: plan.buffer_bytes()
// gfa_strands.hip: the same graph with strand twins folded into one segment and +/- links (include/katome_gpu.h has the format).
// The plan: every line's offset (line 0 the header, 1 + s representative name[s], 1 + n_segments + l link l), every representative's
// first base and first link, every edge's twin (all-ones: none) and the distinct links as keys of key_words words:
// (2 * x + (ox == '-')) above (2 * y + (oy == '-')), field_bits each in one word, a word each in two
struct GfaStrandsPlan {
    DevBuf line_off, segment_off, link_first, name, twin, link_keys;
    uint32_t key_words = 1, field_bits = 2;
    uint64_t n_segments = 0, n_links = 0, text_bytes = 0, n_unpaired = 0, n_self_twins = 0;
};
struct GfaStrandsOutput {
    DevBuf text, segment_name, segment_off, link_first, edge_twin;
    uint64_t n_segments = 0, n_links = 0, text_bytes = 0, n_unpaired = 0, n_self_twins = 0;
};
int dev_gfa_strands_plan(const GfaGraph& g, GfaStrandsPlan& plan, hipStream_t stream);      // validates (dev_gfa_plan), pairs, verifies, measures; synchronises
// the twins alone (what dev_gfa_strands_plan begins with): candidates by first k-mer, the pairs that name each other, verified base for
// base.  twin: allocated here, n_edges u32, NO_TWIN = none.  validate: the segments are checked first (dev_gfa_validate) -- a caller that
// has run dev_gfa_plan on g passes false.  No link is joined or sorted, no line is measured.  The verifying kernel is left running on `stream`
int dev_strand_twins(const GfaGraph& g, DevBuf& twin, bool validate, hipStream_t stream);
// text: plan.text_bytes rounded up to 16; segment_name: n_segments entries; edge_twin: n_edges entries
int dev_gfa_strands_write(const GfaGraph& g, const GfaStrandsPlan& plan, uint8_t* text, uint64_t* segment_name, uint64_t* edge_twin, hipStream_t stream);
int dev_gfa_strands(const GfaGraph& g, GfaStrandsOutput& out, hipStream_t stream);
// gfa_paths.hip: collapse's contigs as P lines over the segments of the shrunk graph's GFA (include/katome_gpu.h has the format): one
// line per run of properly linked pieces.  The plan: every piece's path (path_idx, the exclusive scan of the run flags: a piece
// starts a run where path_idx[p + 1] != path_idx[p]) and byte offset (piece_off), one entry more than pieces each; every contig's
// first path; and what the caller gets: every path's line offset and first piece (one entry more than paths) and its contig
struct GfaPathsPlan {
    DevBuf path_idx, piece_off, contig_first_path, path_line_off, path_contig, path_first_piece;
    uint64_t n_paths = 0, n_contigs = 0, text_bytes = 0;
};
// the whole text: H, S and L lines at 0 (text_bytes), the P lines at text_bytes rounded up to 16 (path_bytes), zeros behind each part
struct GfaPathsOutput {
    DevBuf text, segment_off, link_first, path_line_off, path_contig, path_first_piece;
    uint64_t n_segments = 0, n_links = 0, text_bytes = 0, n_paths = 0, n_jumps = 0, path_bytes = 0;
};
// validates (an id below n_edges, a first piece that begins a contig, fewer than 2^31 pieces: KATOME_E_ARG), flags, scans; synchronises
int dev_gfa_paths_plan(uint64_t n_edges, const uint64_t* edge_src, const uint64_t* edge_dst, const uint32_t* pieces, uint64_t n_pieces, GfaPathsPlan& plan,
                       hipStream_t stream);
// its two halves, for a writer with sizes of its own (gfa_strand_paths.hip): the checks and the run structure (everything of the plan
// but piece_off, path_line_off and text_bytes; *size: room for a u32 per piece), then those three from every piece's bytes
int dev_gfa_paths_runs(uint64_t n_edges, const uint64_t* edge_src, const uint64_t* edge_dst, const uint32_t* pieces, uint64_t n_pieces, GfaPathsPlan& plan,
                       DevBuf& size, hipStream_t stream);
int dev_gfa_paths_offsets(uint64_t n_pieces, const uint32_t* size, GfaPathsPlan& plan, hipStream_t stream);
int dev_gfa_paths_write(const uint32_t* pieces, uint64_t n_pieces, const GfaPathsPlan& plan, uint8_t* text, hipStream_t stream);   // text: plan.text_bytes rounded up to 16
// gfa_strand_paths.hip: the same paths over the MERGED segments of gfa_strands.hip (piece i reads <rep i><o i>), and every path's mirror:
// the smallest path that spells the same double-stranded molecule from its other end (all-ones: none).  twin: n_edges u32, NO_TWIN = none
struct GfaStrandPathsPlan {
    GfaPathsPlan runs;                 // 11e's run structure with THIS text's piece_off / path_line_off / text_bytes
    DevBuf oname;                      // every piece's oriented name: rep << 1 | (o == '-')
    DevBuf mirror;                     // [n_paths] u64
    uint64_t n_mirrored = 0, n_self_mirror = 0;
};
struct GfaStrandPathsOutput {
    DevBuf text, segment_name, segment_off, link_first, edge_twin, path_line_off, path_contig, path_first_piece, path_mirror;
    uint64_t n_segments = 0, n_links = 0, text_bytes = 0, n_unpaired = 0, n_self_twins = 0, n_paths = 0, n_jumps = 0, path_bytes = 0, n_mirrored = 0,
             n_self_mirror = 0;
};
// validates the pieces (dev_gfa_paths_runs), names, measures, finds the mirrors; synchronises.  twin is trusted: an involution below n_edges
int dev_gfa_strand_paths_plan(uint64_t n_edges, const uint64_t* edge_src, const uint64_t* edge_dst, const uint32_t* twin, const uint32_t* pieces,
                              uint64_t n_pieces, GfaStrandPathsPlan& plan, hipStream_t stream);
int dev_gfa_strand_paths_write(uint64_t n_pieces, const GfaStrandPathsPlan& plan, uint8_t* text, hipStream_t stream);   // text: runs.text_bytes rounded up to 16
// the mirror search itself, over any grouping of consecutive pieces (the paths above; collapse's contigs in unique_contigs.hip): group_idx
// is the EXCLUSIVE scan of the flags that begin a group (n_pieces + 1 entries), group_first every group's first piece (n_groups + 1).
// mirror: allocated here, [n_groups] u64, all ones: none.  twin is trusted, every piece's id is below its length.  Synchronises
int dev_find_mirrors(const uint32_t* pieces, uint64_t n_pieces, const uint32_t* twin, const uint64_t* group_idx, const uint64_t* group_first, uint64_t n_groups,
                     DevBuf& mirror, uint64_t* n_mirrored, uint64_t* n_self_mirror, hipStream_t stream);
// a caller's 64-bit twin map (all ones: none) checked on the device -- an entry is all ones or below n_edges, and names its edge back:
// KATOME_E_ARG, the message begun with `who` -- and narrowed into twin (n_edges u32, NO_TWIN: none).  Synchronises
int dev_strand_twin_check(const char* who, uint64_t n_edges, const uint64_t* twin64, uint32_t* twin, hipStream_t stream);

// unique_contigs.hip: one strand per molecule (include/katome_gpu.h has the definitions).  Everything the result holds, in its own buffers
struct UniqueOutput {
    DevBuf contig_mirror, kept_name, kept_off, kept_len, text;
    uint64_t n_contigs = 0, n_mirrored = 0, n_self_mirror = 0, n_kept = 0, text_bytes = 0;
    uint32_t layout = 0;
};
// what the selection leaves for the writer: the mirrors, the kept contigs' names and their pieces, compacted, with the text's plan
struct UniquePlan {
    DevBuf mirror, name, pieces;
    TextPlan text;
    uint64_t n_contigs = 0, n_mirrored = 0, n_self_mirror = 0, n_kept = 0, n_kept_pieces = 0;
};
// validates the pieces (dev_text_plan), finds the contigs' mirrors, selects, compacts, measures; synchronises.  twin: n_labels u32, trusted
int dev_unique_plan(uint32_t k, const uint8_t* label, const uint64_t* label_off, uint64_t n_labels, const uint32_t* twin, const uint32_t* pieces,
                    uint64_t n_pieces, uint32_t layout, UniquePlan& plan, hipStream_t stream);
// kept_off / kept_len: n_kept entries; text: plan.text.text_bytes rounded up to 16
int dev_unique_write(uint32_t k, const uint8_t* label, const uint64_t* label_off, uint32_t layout, const UniquePlan& plan, uint64_t* kept_off, uint32_t* kept_len,
                     uint8_t* text, hipStream_t stream);

// Contigs::stats' panic sites as a status (contig_stats.h's 1, 2, 3: which tipping point is 0), one message wherever the stats are made
inline int contig_stats_status(int which) {
    if (which <= 0) return KATOME_OK;
    static const char* const names[] = {"", "n50 (sum of the lengths / 2)", "n90 (0.1 * sum of the lengths, truncated)", "ng50 (original_genome_length / 2)"};
    set_error("called `Option::unwrap()` on a `None` value: the tipping point of %s is 0", names[which < 4 ? which : 0]);       // stats/contigs.rs:86-88
    return KATOME_E_ARG;
}
// io::Error::description() of the kinds File::create meets (asm/mod.rs:62, "couldn't create <path>: <why>"), as an index that can travel
static const char* const CREATE_ERROR_KINDS[5] = {"", "entity not found", "permission denied", "entity already exists", "other os error"};
inline uint32_t create_error_kind(int e) { return e == ENOENT ? 1 : (e == EACCES || e == EPERM) ? 2 : e == EEXIST ? 3 : 4; }

constexpr int KATOME_MAX_RANKS = 16;      // ranks of a sharded build (an MI355X node has 8 GPUs)

// table.hip (the table in HBM) and lds_count.hip (a level counted by sorting)
struct Table {
    DevBuf slots;          // NW=1: {u64 key|OCC, u32 count, u32 pad}; NW=2: {u64 hi|flags, u64 lo, u32 count, u32 pad[3]}
    DevBuf counter;        // u64 occupied
    DevBuf seen;           // first-seen-order mode: [cap][2] u64 earliest sequence base per strand (table.hip)
    bool track_seen = false;
    uint64_t cap = 0;
    uint32_t nw = 1;
    size_t slot_bytes() const { return nw == 1 ? 16 : 32; }
    void release() { slots.release(); counter.release(); seen.release(); cap = 0; }      // (cap == 0: "no table" -- expand_to_last_level's test)
};
// where a batch of records sits in the read-ordered stream (first-seen-order mode)
struct SeenOrigin {
    uint64_t read0 = 0, rec0 = 0; uint32_t per_read = 1, span = 1, windows = 1; bool rc = false;
    uint32_t win0 = 0;                 // first window the batch's records cover in every read (the windows after the tiles)
    // variable-length reads: record g of the batch is window g - win_prefix[r] of the read r with win_prefix[r] <= g;
    // seq_base = sequence numbers used by the batches before this one
    const uint64_t* win_prefix = nullptr; uint64_t n_reads = 0, seq_base = 0;
    // ... whose records may be whole tiles (mode 1) or the windows after them (mode 2): rec_prefix = records before each read
    const uint64_t* rec_prefix = nullptr; uint32_t mode = 0;
    // sharded build: the records arrive grouped by the rank that extracted them (n_seg segments, segment p = records
    // [seg_off[p], seg_off[p+1]) of the batch, cut from reads seg_read0[p]...), each with its index in THAT rank's batch ...
    const uint32_t* idx = nullptr; uint32_t n_seg = 0;
    uint64_t seg_off[KATOME_MAX_RANKS + 1] = {0}, seg_read0[KATOME_MAX_RANKS] = {0};
    // ... or with both sequence numbers spelled out ([n][2]: stored orientation, its reverse complement): k-mer records made
    // out of another rank's tiles
    const uint64_t* pairs = nullptr;
};
// How a first-seen build's tagged records spell their two sequence numbers: reads of one length as read << 32 | offset << 16 | offset
// (slot_bits.h, seen_pack; seq_per_read = 2 x windows turns the offsets back into numbers), reads of varying length as the numbers
// themselves (seen_tag.h, the delta tag; seq_per_read means nothing)
struct SeenTag {
    bool delta = false; uint64_t seq_per_read = 0;
    static SeenTag fixed(uint64_t seq_per_read) { SeenTag t; t.seq_per_read = seq_per_read; return t; }
    static SeenTag by_delta() { SeenTag t; t.delta = true; return t; }
    bool packs() const { return delta || (seq_per_read != 0 && seq_per_read <= 0xFFFFu); }
};
int table_alloc(Table& t, uint32_t nw, uint64_t cap, hipStream_t stream);
int table_insert(Table& t, const uint64_t* d_records, const uint32_t* d_weights, uint64_t n, hipStream_t stream,
                 const SeenOrigin* origin = nullptr);
int table_occupied(Table& t, uint64_t* out, hipStream_t stream);
int table_grow(Table& t, uint64_t new_cap, hipStream_t stream);
// tiled counting: every tile (key of k+span-1 bases, weight n) adds n to each of its `span` k-mers
int table_expand_tiles(Table& tiles, uint64_t slot0, uint64_t slot1, Table& kmers, uint32_t k, uint32_t span, uint32_t stride,
                       bool rc, hipStream_t stream);
// same, but the (k-mer, weight) records are written out instead (multi-GPU: they travel to their owners)
// (seen: when the tile table tracks first-seen order, the records' two sequence numbers, [n][2])
int table_expand_tiles_to_records(Table& tiles, uint32_t k, uint32_t span, bool rc, DevBuf& keys, DevBuf& weights,
                                  uint64_t* n_records, hipStream_t stream, DevBuf* seen = nullptr);
int table_list_to_records(const uint64_t* d_tiles, const uint32_t* d_counts, uint64_t n_tiles, uint32_t tile_bases, uint32_t k, uint32_t span, uint32_t stride, bool rc,
                          DevBuf& keys, DevBuf& weights, uint64_t* n_records, hipStream_t stream, uint64_t extra_room = 0, DevBuf* first_counts = nullptr,
                          bool rep = false, RecordSource* src = nullptr);
// (src, with first_counts: where the first pass can make the records itself -- fused_records_takes, nothing to append -- no record is
// written: first_counts are counted from the list alone, *src describes the records and keys / weights stay unallocated, see RecordSource)
// (rep: the k-mers in their representative orientation -- kmer_bits.h rep_orientation -- for the ordered count, records_to_edges_sorted
// with a HalfSort; first_counts are then that count's first key digit)
// in place: n one-word k-mer records into their representative orientation (rep) or back into the canonical one
int table_orient_records(uint64_t* d_keys, uint64_t n, uint32_t k, bool rep, hipStream_t stream);
// (first_counts: filled with the digit counts per tile of the first partition pass over these records -- dev_hash_order's first_counts --
// when the kernel can make them as it writes; released otherwise)
// (extra_room: records the caller will append behind them -- the windows left over after the tiles)
int table_tiles_to_records_fast(Table& tiles, uint32_t k, uint32_t span, bool rc, DevBuf& keys, DevBuf& weights, uint64_t* n_records, hipStream_t stream,
                                uint64_t extra_room = 0);
// first-seen builds, last level counted by sorting: the tiles' k-mers as (k-mer, packed sequence numbers) records, counted and
// numbered in LDS; edge_key (unsorted) and seq_weight ([n][2]: {sequence number, weight}) come out as table_emit_edges leaves them.
// tag: how the records spell their two numbers; E_UNSUPPORTED when the packing does not fit (the caller counts in the table)
// (d_extra / n_extra: tagged records to count with them -- the windows left over after the tiles, table_rest_to_tagged)
int tiles_to_edges_sorted_seen(Table& tiles, uint32_t k, uint32_t span, bool rc, SeenTag tag, DevBuf& edge_key, DevBuf& seq_weight,
                               uint64_t* n_edges, uint64_t* n_distinct, hipStream_t stream, const uint64_t* d_extra = nullptr, uint64_t n_extra = 0);
// appends the valid records of d_rec behind *d_cursor in d_out (tagged: as records of nw + 1 words, see seen_pack in slot_bits.h)
int table_keep_rest(const uint64_t* d_rec, uint64_t n, uint32_t nw, bool tagged, uint64_t read0, uint32_t per_read, uint32_t win0, uint32_t seq_per_read,
                    uint64_t* d_out, uint64_t* d_cursor, hipStream_t stream, uint32_t win_stride = 1, uint32_t span = 1);
int tagged_records_sorted(DevBuf& recs, DevBuf& wts, uint64_t n, uint32_t k, bool rc, SeenTag tag, bool list, DevBuf& out_keys,
                          DevBuf& out_second, uint64_t* n_out, uint64_t* n_distinct, hipStream_t stream, uint32_t* first_counts = nullptr);
int table_list_to_tagged_records(const uint64_t* d_list, const uint32_t* d_counts, uint64_t n_tiles, uint32_t tile_bases, uint32_t sub_len, uint32_t n_sub,
                                 uint32_t stride, bool rc, DevBuf& recs, DevBuf& weights, uint64_t* n_records, hipStream_t stream, uint64_t extra_room = 0,
                                 DevBuf* first_counts = nullptr, bool delta = false);
int table_tagged_to_pairs(const uint64_t* d_tagged, uint64_t n, uint32_t nw, SeenTag tag, uint64_t* d_keys, uint64_t* d_pairs, hipStream_t stream);
// The records of a batch of variable-length reads (mode / span / prefixes: seq_pair.h, var_seq_pair) as delta-tagged records of nw + 1
// words: the valid ones are appended behind *d_cursor in d_out.  The caller has checked that every read of the batch packs
// (table_max_windows: no read of more than DELTA_MAX_WINDOWS windows, numbers below DELTA_P_LIMIT)
int table_keep_var_tagged(const uint64_t* d_rec, uint64_t n, uint32_t nw, bool rc, const uint64_t* d_win_prefix, const uint64_t* d_rec_prefix, uint64_t n_reads,
                          uint32_t mode, uint32_t span, uint64_t seq_base, uint64_t* d_out, uint64_t* d_cursor, hipStream_t stream);
int table_max_windows(const uint64_t* d_win_prefix, uint64_t n_reads, uint64_t* max_windows, hipStream_t stream);      // the longest read's windows (synchronises)
// A rank's own distinct k-mers on their way to their owners (sharded build): with an OwnerSplit the records are grouped by the hash
// of their CORE instead of the whole k-mer's, and every group's keys are written into its owner's stretch of the output -- base[p],
// count[p] on return --, so that no partition pass is needed before the exchange.  One-word k-mers, one record per k-mer (rc = false).
struct OwnerSplit {
    uint32_t n_parts = 0, core_shift = 0, core_bases = 0;
    uint64_t base[KATOME_MAX_RANKS] = {0}, count[KATOME_MAX_RANKS] = {0};
};
// The k-mer level's ordered count (lds_count_ordered_kernel): S1, the representatives in key order with holes (s1_key / s1_w at
// group_first[g], group_count[g] of them), and S2, their reverse complements in no order (n_s2).  half_sort_finish orders S2 (per
// 16-bit group inside the merge, or by a full sort) and merges the two into the sorted edge list -- the arrays a sort of all edges
// gives -- and releases them.
struct HalfSort {
    DevBuf s1_key, s1_w, group_first, group_count, s2_key, s2_w;
    DevBuf s2_digit;           // (beside s2_key: the first partition digit of every S2 key, one byte each -- dev_key_order's first_digits)
    uint64_t n_s1 = 0, n_s2 = 0;
    uint32_t k = 0;
    bool taken = false;
    // regions (s2_regions.h): S2 lies in 256 regions by its first partition digit -- region d from region_start[d] on, region_used[d]
    // keys --, and s2_digit holds the SECOND digit of every key; half_sort_finish makes it dense with that one pass (dev_s2_region_pass)
    bool regions = false;
    uint64_t region_start[257] = {0}, region_used[256] = {0};
    void release() {
        s1_key.release(); s1_w.release(); group_first.release(); group_count.release(); s2_key.release(); s2_w.release(); s2_digit.release();
        n_s1 = n_s2 = 0; taken = false; regions = false;
    }
};
// (head_counts: filled with the merge's source run heads per block of edges -- dev_group_merge -- where the merge makes them, else released)
int half_sort_finish(HalfSort& hs, DevBuf& edge_key, DevBuf& edge_weight, hipStream_t stream, DevBuf* head_counts = nullptr);
// (half: the records are in their representative orientation -- table_list_to_records with rep -- and the level is counted in order
// into *half when it can be (half->taken); otherwise they are turned back and counted the usual way, with unsorted edges out)
// (first_counts, here and in tagged_records_sorted: handed to the order call, which overwrites them -- see dev_hash_order)
int records_to_edges_sorted(DevBuf& keys, DevBuf& weights, uint64_t n, uint32_t k, bool rc, uint32_t min_weight, DevBuf& edge_key,
                            DevBuf& edge_weight, uint64_t* n_edges, uint64_t* n_distinct, hipStream_t stream, OwnerSplit* split = nullptr,
                            uint32_t* first_counts = nullptr, HalfSort* half = nullptr, RecordSource* src = nullptr);
// (src: keys / weights may be records still to be made.  KATOME_E_UNSUPPORTED leaves them written all the same: before the passes
// they are materialised, after the passes they lie ordered in keys / weights)
// (test entry katome_dev_count_records, api.hip: this function on copies of the caller's records, without first_counts, half or src,
// its status handed on as it is -- what tests/test_gpu_count_records.py compares with a dictionary, strategy by strategy)
int table_to_records(Table& t, DevBuf& keys, DevBuf& weights, uint64_t* n_records, hipStream_t stream, DevBuf* seen_pairs = nullptr);
int table_expand_tiles_to_subtiles(Table& tiles, uint32_t k, uint32_t span, uint32_t stride, bool rc, DevBuf& keys, DevBuf& weights,
                                   uint64_t* n_records, hipStream_t stream, DevBuf* seen = nullptr);
// distinct oriented edges (unsorted): allocates d_keys/d_weights
int table_emit_edges(Table& t, uint32_t k, bool rc, uint32_t min_weight, DevBuf& keys, DevBuf& weights, uint64_t* n_edges,
                     hipStream_t stream, DevBuf* seqs = nullptr);

// synth.hip
int launch_synth(uint64_t first_read, uint64_t n_reads, uint32_t read_len, uint64_t genome_len, double err_rate,
                 uint32_t n_inject_percent, uint8_t* d_packed, uint8_t* d_skip, hipStream_t stream);

// ingest.cpp (host only)
struct HostReads {
    uint64_t n_records = 0, n_reads = 0, read_bytes = 0, total_windows = 0;
    uint32_t fixed_len = 0;
    bool all_fixed = true;
    uint8_t* packed = nullptr; uint64_t packed_bytes = 0, packed_cap = 0;
    uint64_t* byte_off = nullptr; uint32_t* len = nullptr; uint64_t cap_reads = 0;
    uint32_t* weight = nullptr;          // BFCounter input only: one weight per k-mer line (builder.rs:96-105)
    ~HostReads();
};
int ingest_files(const katome_settings* s, const char* const* paths, size_t n_paths, HostReads& out);
// the records of query files (katome_depth_paths) as they are spelled: EVERY record is kept -- one with an N, one shorter than k, an
// empty one --, its bases as ASCII bytes back to back in `text`, record i at off[i], len[i] bytes
struct HostQuery {
    std::vector<uint8_t> text;
    std::vector<uint64_t> off;
    std::vector<uint32_t> len;
};
// file_type: 0 FASTA (a record's lines are joined), 1 FASTQ; anything else is KATOME_E_ARG
int scan_query(uint32_t file_type, const uint8_t* p, size_t n, HostQuery& q);
int ingest_query_files(uint32_t file_type, const char* const* paths, size_t n_paths, HostQuery& out);

}  // namespace katome
