// dist_builder.h -- state of one rank of the sharded build (dist.hip; the distributed pruning in dist_prune.hip works on it)
#pragma once
#include <algorithm>
#include <vector>

#include "builder.h"
#include "comm.h"

enum XPhase { X_RECORDS, X_KMERS, X_TARGETS, X_IDS, X_RANK_NODES, X_RANK_EDGES, X_GATHER, X_MID_TILES, X_PRUNE, X_COUNT };
extern const char* const XPHASE_NAMES[X_COUNT];

struct katome_dist_builder {
    katome_settings s;
    katome_comm* comm = nullptr;
    katome_builder* b = nullptr;             // this rank's single-GPU builder (tables, sorted edges)
    uint32_t nw = 1;
    bool rc = false, first_seen = false;
    // the plan, the same on every rank (a function of k and the read length)
    bool planned = false;
    uint32_t read_len = 0, W = 0, span = 1, tiles_per_read = 0, rest = 0, nwt = 1;
    uint64_t reads_end = 0;                  // one past the last read this rank has added (first-seen: bounds the sequence numbers)
    // reads of varying length (katome_dist_add_reads_var): the span was agreed from all ranks' reads at the first call; this
    // rank's reads start at global window var_first_window, its calls so far added var_windows windows (first-seen: the
    // sequence numbers of its next read start at 2 * (var_first_window + var_windows))
    bool var = false, fixed_added = false;
    uint64_t var_first_window = 0, var_windows = 0, var_calls = 0;
    bool finalized = false;
    // Which records travel.  Few ranks share few links: every rank counts its own reads down to k-mers and
    // sends each DISTINCT k-mer once ("local first": one exchange, 12 B per k-mer and rank).  Many ranks: tiles, mid tiles and
    // k-mer records are routed to owners level by level (no level is counted twice, at the price of three exchanges).
    bool local_first = false;
    // Round 4 (KATOME_DIST_ROUTE=supermers; by packed key, k <= 31, reads of one length): ONE exchange before anything is counted --
    // a read travels as its supermers (supermer.hip: runs of windows with one minimizer, a 16-byte record each, owner = a hash of the
    // minimizer), every rank then counts what it received as one GPU counts its own reads.  `owner_m` > 0: a k-mer's / node's owner
    // is named by the minimizer of that many bases of its core (the finalize's target look-ups use the same function).
    bool want_supermers = false, supermers = false;
    uint32_t owner_m = 0, sm_slots = 0;
    DevBuf sm_recs;                          // [sm_n][2]: per add_reads call the reads' slots, then that call's spill region
    uint64_t sm_n = 0, sm_cap = 0;
    hipStream_t xstream = nullptr;           // the exchanges of route_weighted run here, beside the insertions on the build's stream
    // this rank's share of the numbered graph
    DevBuf edge_src, edge_dst, edge_label, node_key, edge_gid, node_gid;
    uint64_t n_edges = 0, n_nodes = 0, total_edges = 0, total_nodes = 0, node_base = 0;
    katome::ExchangeStats xstats[X_COUNT];
    // kept for the stages that run on the sharded graph (dist_prune.hip; first-seen order only): every edge's source as the
    // LOCAL index of the node (all out-edges of a node live on the node's owner) and its target as (owner rank, local index there);
    // released by whatever removes edges or nodes, rebuilt by dist_rebuild_links
    DevBuf edge_lsrc, edge_drank, edge_dlocal;
    DevBuf edge_age;                         // after katome_dist_remove_dead_paths or a stage that may remove edges (dist_stages.hip):
                                             // the first-seen index each surviving edge had (u64)
    uint64_t n_src = 0;                      // this rank's nodes [0, n_src) have out-edges (ascending by key), the rest do not
    bool dead_paths_removed = false;         // katome_dist_remove_dead_paths has run to its fixpoint and no edge or node went since
    bool gathered = false;                   // katome_dist_gather has consumed the ranks' shares
    // the last katome_dist_shrink's merged edges on this rank (dist_shrink.hip), kept until the next call or destroy
    DevBuf sh_src, sh_dst, sh_weight, sh_kmers, sh_label_off, sh_label, sh_head, sh_node_id, sh_node_key;
    uint64_t sh_edges = 0, sh_nodes = 0, sh_total_edges = 0, sh_total_nodes = 0, sh_label_bytes = 0;
    bool sh_valid = false;                   // a katome_dist_shrink has finished and none has started since
    uint64_t sh_serial = 0;                  // katome_dist_shrink calls so far
    katome::ShrinkCoverage sh_cov;           // katome_dist_shrink_coverage: the k-mer count sum / min / max of this rank's merged edges;
                                             // dropped by the next shrink of either kind
    // the text of that result on this rank (dist_text.hip, katome_dist_contigs_text), kept until the next call or destroy
    katome::TextOutput sh_text;
    uint64_t sh_text_serial = 0, sh_text_first = 0, sh_text_base = 0, sh_text_total = 0, sh_text_contigs = 0;
    bool sh_text_valid = false;
    // the GFA text of that result on this rank (dist_gfa.hip, katome_dist_contigs_gfa): one buffer, the S part at 0 and the L part at
    // the next multiple of 16; kept until the next call or destroy
    DevBuf sh_gfa_text, sh_gfa_segment_off, sh_gfa_link_first, sh_gfa_link_b;
    katome_dist_gfa sh_gfa = {};             // what the call handed out (katome_dist_gfa_save checks against it)
    uint64_t sh_gfa_serial = 0;
    bool sh_gfa_valid = false;
    // what the last katome_dist_standardize_contigs that finished on this builder did (katome_dist_standardize_stats_read)
    katome_dist_standardize_stats contigs_stats = {};
    bool contigs_stats_valid = false;

    int world() const { return comm->world(); }
    int rank() const { return comm->rank(); }
    // all-to-all of records grouped by destination, accounted to `phase`
    // (RCCL only enqueues: with the builder's profile switched on the exchange is timed with HIP events on its stream)
    struct XEvent { int phase; hipEvent_t a, b; };
    std::vector<XEvent> xevents;
    int xchg(int phase, const void* send, const uint64_t* send_cnt, void* recv, const uint64_t* recv_cnt, size_t elem_bytes, hipStream_t stream,
             bool one_round = false, uint64_t known_max = katome_comm::MAX_UNKNOWN, const uint64_t* send_off = nullptr) {
        const katome::ExchangeStats before = comm->stats;
        hipEvent_t ea = nullptr, eb = nullptr;
        bool timed = b->prof.on && hipEventCreate(&ea) == hipSuccess;
        if (timed && hipEventCreate(&eb) != hipSuccess) { (void)hipEventDestroy(ea); ea = nullptr; timed = false; }
        // (the sharded pruning makes dozens of exchanges per pass: finished pairs are folded into the phase's time instead of piling up)
        if (timed && xevents.size() >= 256) fold_xevents();
        if (timed) (void)hipEventRecord(ea, stream);
        const int rc = comm->exchange(send, send_cnt, recv, recv_cnt, elem_bytes, 1, stream, one_round, known_max, send_off);
        if (timed) { (void)hipEventRecord(eb, stream); xevents.push_back({phase, ea, eb}); }
        if (rc != KATOME_OK) return rc;
        katome::ExchangeStats& x = xstats[phase];
        x.calls += comm->stats.calls - before.calls; x.bytes_out += comm->stats.bytes_out - before.bytes_out;
        x.bytes_in += comm->stats.bytes_in - before.bytes_in;
        if (!timed) x.ms += comm->stats.ms - before.ms;
        for (int p = 0; p < world(); ++p) if (p != rank()) x.max_pair_bytes = std::max<uint64_t>(x.max_pair_bytes, send_cnt[p] * elem_bytes);
        return KATOME_OK;
    }
    // the pairs whose second event has completed: their time goes to their phase, the events are destroyed
    void fold_xevents() {
        size_t kept = 0;
        for (auto& e : xevents) {
            float ms = 0;
            if (hipEventQuery(e.b) == hipSuccess) {
                if (hipEventElapsedTime(&ms, e.a, e.b) == hipSuccess) xstats[e.phase].ms += ms;
                (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b);
            } else xevents[kept++] = e;
        }
        xevents.resize(kept);
    }
    ~katome_dist_builder() {
        for (auto& e : xevents) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
        if (xstream) { (void)hipSetDevice(s.device); dev_retire_stream(xstream); (void)hipStreamDestroy(xstream); }
    }
};

// dist_stages.hip: edge_lsrc / edge_drank / edge_dlocal / n_src of the share as it stands (collective)
int dist_rebuild_links(katome_dist_builder* d, hipStream_t stream);
// dist_contigs.hip: standardize_contigs by list ranking, memory O(share) (collective; the caller has checked the builder and the sizes)
int dist_contigs_ranked(katome_dist_builder* d, hipStream_t stream, katome_dist_standardize_stats* st);
