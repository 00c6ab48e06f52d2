// dist_stats.hip -- Stats<CollectionStats> (reference src/katome/stats/collections.rs:137-168) and the weight spectrum of the
// SHARDED graph, no gather: what graph.log_stats() prints at the five points of assemble_with_graph (asm/basic_assembler.rs:
// 58-75), for a graph that may hold more than 2^32 edges (a rank's share may not).
//
// A rank's edges are the out-edges of the nodes it owns, so out-degrees, the weight sum and the largest weight are local
// (stats.hip's passes over the share).  For the in-degrees every edge sends its target's address -- (owner rank << 56) |
// local index there, the addressing of dist_links.h -- to the owner through the Router, in chunks of at most 2^24 records
// per rank and exchange (KATOME_DIST_STATS_CHUNK=<n>: tests); the owner adds 1 to the low half of the node's degree word, and
// the counts add up over the chunks.  Memory per rank: 8 B per node and 12 B per edge, plus the chunk in flight; nothing
// is replicated.  Two allreduces put the whole graph's numbers on every rank: sums (edges, nodes, weight sum, out-degree sum,
// the two externals() counts; every spectrum bin) and maxima (weight, in-degree, out-degree).
//
// No rank leaves the others waiting: what a rank did on its own since the last collective (allocations, launches, the
// checks of what it received) is a status that all ranks exchange before the next one, and every rank returns the first
// failing rank's status with a message that names it.  What the Router allocates inside send() before it exchanges counts
// is not covered, as in the other sharded stages.  KATOME_DIST_STATS_FAIL=<rank> (tests): that rank fails after the first
// exchange.
#include <string>

#include "dist_agree.h"
#include "dist_links.h"

namespace {

constexpr uint64_t DEFAULT_STATS_CHUNK = 1ull << 24;

__global__ __launch_bounds__(BLOCK) void st_out_deg_kernel(const u32* __restrict__ lsrc, u64 E, u64 N, u64* __restrict__ deg, unsigned long long* __restrict__ bad) {
    WLOOP(e, E) if (e < E) {
        if (lsrc[e] < N) atomicAdd((unsigned long long*)&deg[lsrc[e]], 1ull << 32);
        else atomicAdd(bad, 1ull);
    }
}
__global__ __launch_bounds__(BLOCK) void st_in_deg_kernel(const u64* __restrict__ A, u64 n, u64 N, u64* __restrict__ deg, unsigned long long* __restrict__ bad) {
    WLOOP(i, n) if (i < n) {
        if (local_of(A[i]) < N) atomicAdd((unsigned long long*)&deg[local_of(A[i])], 1ull);
        else atomicAdd(bad, 1ull);
    }
}

int check_stats_builder(katome_dist_builder* d, const char* name) {
    if (!d) { set_error("null argument"); return KATOME_E_ARG; }
    if (!d->finalized) { set_error("%s: call katome_dist_finalize first", name); return KATOME_E_ARG; }
    if (d->gathered) { set_error("%s: the ranks' shares were gathered (katome_dist_gather); ask the gathered graph's builder on its root", name); return KATOME_E_ARG; }
    return KATOME_OK;
}
int check_share(katome_dist_builder* d, const char* name) {
    if (d->n_edges >= 0xFFFFFFFFull || d->n_nodes >= 0xFFFFFFFFull) { set_error("%s: 2^32 edges or nodes or more on one rank", name); return KATOME_E_UNSUPPORTED; }
    return KATOME_OK;
}

int dist_graph_stats(katome_dist_builder* d, katome_stats* out, hipStream_t stream) {
    const char* name = "katome_dist_graph_stats";
    Collective C(d->comm, name);
    const uint64_t E = d->n_edges, N = d->n_nodes, me = (uint64_t)C.rank;
    const int world = C.world;
    const long long fail_at = getenv("KATOME_DIST_STATS_FAIL") ? atoll(getenv("KATOME_DIST_STATS_FAIL")) : -1;
    uint64_t chunk = DEFAULT_STATS_CHUNK;
    if (const char* e = getenv("KATOME_DIST_STATS_CHUNK")) chunk = std::max<long long>(1, atoll(e));
    KCHECK(d->comm->allreduce(&chunk, 1, OP_MIN));          // (process ranks may see different environments: the smallest holds)
    uint64_t n_chunks = (E + chunk - 1) / chunk;
    KCHECK(C.agree(check_share(d, name), &n_chunks));
    if (d->first_seen) {   // a stage of dist_stages.hip dropped the links: rebuild them, a collective, so all ranks agree first (dist_prune.hip)
        uint64_t stale = (!d->edge_lsrc.p || !d->edge_drank.p || !d->edge_dlocal.p) ? 1 : 0;
        KCHECK(d->comm->allreduce(&stale, 1, OP_MAX));
        if (stale) KCHECK(dist_rebuild_links(d, stream));
    }
    std::vector<uint64_t> n_of(world, 0), bases(world + 1, 0);
    KCHECK(d->comm->allgather(N, n_of.data()));
    for (int p = 0; p < world; ++p) bases[p + 1] = bases[p] + n_of[p];
    // ---- this rank alone: targets, out-degrees, weights -------------------------------------------------------------------
    Router router(d, stream);
    DevBuf dbases(stream), lsrc(stream), tgt(stream), deg(stream), res(stream);
    unsigned long long* bad = nullptr;
    auto local = [&]() -> int {
        KCHECK(dbases.alloc((world + 1) * 8)); KCHECK(lsrc.alloc((E + 1) * 4)); KCHECK(tgt.alloc((E + 1) * 8)); KCHECK(deg.alloc((N + 1) * 8));
        KCHECK(res.alloc((STATS_WORDS + 1) * 8));
        bad = res.as<unsigned long long>() + STATS_WORDS;
        KCHECK_HIP(hipMemcpyAsync(dbases.p, bases.data(), (world + 1) * 8, hipMemcpyHostToDevice, stream));
        KCHECK_HIP(hipMemsetAsync(deg.p, 0, (N + 1) * 8, stream));
        KCHECK_HIP(hipMemsetAsync(res.p, 0, (STATS_WORDS + 1) * 8, stream));
        if (E) {
            KLAUNCH(target_kernel, E, stream, d->edge_src.as<u64>(), d->edge_dst.as<u64>(), E, d->first_seen ? d->edge_lsrc.as<u64>() : nullptr,
                    d->edge_drank.as<u64>(), d->edge_dlocal.as<u64>(), dbases.as<u64>(), (u32)world, d->node_base, lsrc.as<u32>(), tgt.as<u64>());
            KLAUNCH(st_out_deg_kernel, E, stream, lsrc.as<u32>(), E, N, deg.as<u64>(), bad);
            KCHECK_HIP(hipGetLastError());
        }
        KCHECK(dev_weight_max_sum(d->b->edge_weight.as<u32>(), E, res.as<u64>(), stream));
        KCHECK(router.init());                               // (synchronises: bases may go out of use)
        return KATOME_OK;
    };
    KCHECK(C.agree(local()));
    lsrc.release();
    // ---- in-degrees: every edge's target address to the target's owner, chunk by chunk ------------------------------------
    bool knob = fail_at == (long long)me;
    auto struck = [&]() -> int {
        if (!knob) return KATOME_OK;
        knob = false;
        set_error("KATOME_DIST_STATS_FAIL=%lld", fail_at);
        return KATOME_E_UNSUPPORTED;
    };
    for (uint64_t c = 0; c < n_chunks; ++c) {
        const uint64_t at = std::min(E, c * chunk), cnt = std::min(E - at, chunk);
        Routed r(stream);
        KCHECK(router.send(tgt.as<u64>() + at, nullptr, cnt, r));
        auto add = [&]() -> int {
            if (r.n) KLAUNCH(st_in_deg_kernel, r.n, stream, r.a.as<u64>(), r.n, N, deg.as<u64>(), bad);
            KCHECK_HIP(hipGetLastError());
            KCHECK_HIP(hipStreamSynchronize(stream));        // (r's buffers go with the chunk)
            return struck();
        };
        KCHECK(C.agree(add()));
    }
    tgt.release();
    // ---- the rank's numbers, then the whole graph's -----------------------------------------------------------------------
    uint64_t h[STATS_WORDS + 1] = {0};
    auto reduce = [&]() -> int {
        KCHECK(struck());                                    // (no exchange was needed: the knob strikes here)
        KCHECK(dev_degree_reduce(deg.as<u64>(), N, res.as<u64>(), stream));
        KCHECK_HIP(hipMemcpyAsync(h, res.p, sizeof h, hipMemcpyDeviceToHost, stream));
        KCHECK_HIP(hipStreamSynchronize(stream));
        if (h[STATS_WORDS]) { set_error("%llu edges name a node their owner does not hold", (unsigned long long)h[STATS_WORDS]); return KATOME_E_DEVICE; }
        return KATOME_OK;
    };
    KCHECK(C.agree(reduce()));
    uint64_t sums[6] = {E, N, h[0], h[6], h[4], h[5]}, maxima[3] = {h[1], h[2], h[3]};
    KCHECK(d->comm->allreduce(sums, 6, OP_SUM));
    KCHECK(d->comm->allreduce(maxima, 3, OP_MAX));
    const uint64_t whole[STATS_WORDS] = {sums[2], maxima[0], maxima[1], maxima[2], sums[4], sums[5], sums[3], 0};
    fill_stats(sums[1], sums[0], whole, out);
    return KATOME_OK;
}

int dist_weight_spectrum(katome_dist_builder* d, uint64_t* bins, uint32_t n_bins, hipStream_t stream) {
    const char* name = "katome_dist_weight_spectrum";
    Collective C(d->comm, name);
    auto local = [&]() -> int {
        KCHECK(check_share(d, name));
        return dev_weight_spectrum(d->b->edge_weight.as<u32>(), d->n_edges, bins, n_bins, stream);
    };
    KCHECK(C.agree(local()));
    return d->comm->allreduce(bins, n_bins, OP_SUM);
}

}  // namespace

extern "C" {

int katome_dist_graph_stats(katome_dist_builder* d, katome_stats* out, void* stream_) {
    KCHECK(check_stats_builder(d, "katome_dist_graph_stats"));
    if (!out) { set_error("null argument"); return KATOME_E_ARG; }
    hipStream_t stream = (hipStream_t)stream_;
    KCHECK_HIP(hipSetDevice(d->s.device));
    d->comm->use_stream(stream);
    PhaseScope ps(d->b->prof, PH_GRAPH_STATS, stream);
    return dist_graph_stats(d, out, stream);
}

int katome_dist_weight_spectrum(katome_dist_builder* d, uint64_t* bins, uint32_t n_bins, void* stream_) {
    KCHECK(check_spectrum_bins(bins, n_bins));
    KCHECK(check_stats_builder(d, "katome_dist_weight_spectrum"));
    hipStream_t stream = (hipStream_t)stream_;
    KCHECK_HIP(hipSetDevice(d->s.device));
    d->comm->use_stream(stream);
    PhaseScope ps(d->b->prof, PH_WEIGHT_SPECTRUM, stream);
    return dist_weight_spectrum(d, bins, n_bins, stream);
}

}  // extern "C"
