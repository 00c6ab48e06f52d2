// dist_links.h -- degrees and links of the SHARDED graph, the first step of everything that follows its straight paths
// (dist_shrink.hip: the merged edges; dist_contigs.hip: the contigs of standardize_contigs).  Every edge sends (its target's
// address, its own address) to the owner of its target (first-seen order: edge_drank / edge_dlocal, rebuilt by
// dist_rebuild_links when a stage dropped them; by packed key: the allgathered node_base ranges).  The owner counts
// in-degrees, keeps the address (rank << 56 | local index) of the edge that comes in and answers whether the target is INNER:
// in-degree = out-degree = 1 and its two edges are not one self-loop.  Every edge then finds its predecessor -- the in-edge of
// its source, if the source is inner -- in its own rank's tables.  Internal to the file that includes it.
#pragma once
#include "dist_route.h"

namespace {

__device__ __forceinline__ u32 local_of(u64 a) { return (u32)a; }

// every edge: its source's local index and its target's address (first-seen: the links; by packed key: the node_base ranges)
__global__ __launch_bounds__(BLOCK) void target_kernel(const u64* __restrict__ src, const u64* __restrict__ dst, u64 E, const u64* __restrict__ lsrc_fs,
                                                       const u64* __restrict__ drank, const u64* __restrict__ dlocal, const u64* __restrict__ bases,
                                                       u32 world, u64 my_base, u32* __restrict__ lsrc, u64* __restrict__ tgt) {
    WLOOP(e, E) if (e < E) {
        if (lsrc_fs) { lsrc[e] = (u32)lsrc_fs[e]; tgt[e] = (drank[e] << 56) | dlocal[e]; continue; }
        lsrc[e] = (u32)(src[e] - my_base);
        const u64 v = dst[e];
        u32 p = 0;
        while (p + 1 < world && bases[p + 1] <= v) ++p;
        tgt[e] = ((u64)p << 56) | (v - bases[p]);
    }
}
__global__ __launch_bounds__(BLOCK) void own_addr_kernel(u64 E, u64 me, u64* __restrict__ out) { WLOOP(e, E) if (e < E) out[e] = (me << 56) | e; }
__global__ __launch_bounds__(BLOCK) void out_deg_kernel(const u32* __restrict__ lsrc, u64 E, u32* __restrict__ outdeg, u32* __restrict__ out_edge) {
    WLOOP(e, E) if (e < E) { atomicAdd(&outdeg[lsrc[e]], 1u); out_edge[lsrc[e]] = (u32)e; }
}
__global__ __launch_bounds__(BLOCK) void in_rec_kernel(const u64* __restrict__ A, const u64* __restrict__ B, u64 n, u64 N, u32* __restrict__ indeg, u64* __restrict__ in_edge) {
    WLOOP(i, n) if (i < n && local_of(A[i]) < N) { atomicAdd(&indeg[local_of(A[i])], 1u); in_edge[local_of(A[i])] = B[i]; }
}
__global__ __launch_bounds__(BLOCK) void inner_kernel(u64 N, const u32* __restrict__ indeg, const u32* __restrict__ outdeg, const u64* __restrict__ in_edge,
                                                      const u32* __restrict__ out_edge, u64 me, unsigned char* __restrict__ inner) {
    WLOOP(j, N) if (j < N) inner[j] = indeg[j] == 1 && outdeg[j] == 1 && in_edge[j] != ((me << 56) | out_edge[j]);
}
__global__ __launch_bounds__(BLOCK) void answer_u8_kernel(const u64* __restrict__ A, u64 n, u64 N, const unsigned char* __restrict__ v, u64* __restrict__ out) {
    WLOOP(i, n) if (i < n) out[i] = local_of(A[i]) < N ? v[local_of(A[i])] : 0;
}

// what the step leaves: per edge the local index of its source (u32) and whether its target is inner (u64, 0 / 1); per node
// whether it is inner (u8) and the address of the edge that comes in (u64; meaningful where the in-degree is 1)
struct Links {
    DevBuf lsrc, dst_inner, inner, in_edge;
    uint64_t edge_base = 0;                  // the edges of the ranks before this one
    explicit Links(hipStream_t s) : lsrc(s), dst_inner(s), inner(s), in_edge(s) {}
    void release() { lsrc.release(); dst_inner.release(); inner.release(); in_edge.release(); }
};

// collective; 21 B per node and 28 B per edge while it runs, 9 B per node and 12 B per edge stay in `out`.  chunk = 0: every
// edge's record in ONE exchange and the answer on its way back (the Router holds 64 B per record meanwhile); chunk > 0: at
// most that many records per rank and exchange
int dist_links(katome_dist_builder* d, Router& router, hipStream_t stream, Links& out, uint64_t chunk = 0) {
    const uint64_t E = d->n_edges, N = d->n_nodes, me = (uint64_t)d->rank();
    const int world = d->world();
    if (d->first_seen && !d->edge_lsrc.p) KCHECK(dist_rebuild_links(d, stream));
    std::vector<uint64_t> n_of(world, 0), bases(world + 1, 0), e_of(world, 0);
    KCHECK(d->comm->allgather(N, n_of.data()));
    KCHECK(d->comm->allgather(E, e_of.data()));
    out.edge_base = 0;
    for (int p = 0; p < world; ++p) { bases[p + 1] = bases[p] + n_of[p]; if (p < (int)me) out.edge_base += e_of[p]; }
    DevBuf dbases(stream), tgt(stream), mine(stream);
    KCHECK(dbases.alloc((world + 1) * 8)); KCHECK(out.lsrc.alloc((E + 1) * 4)); KCHECK(tgt.alloc((E + 1) * 8)); KCHECK(mine.alloc((E + 1) * 8));
    KCHECK_HIP(hipMemcpyAsync(dbases.p, bases.data(), (world + 1) * 8, hipMemcpyHostToDevice, stream));
    if (E) {
        KLAUNCH(target_kernel, E, stream, d->edge_src.as<u64>(), d->edge_dst.as<u64>(), E, d->first_seen ? d->edge_lsrc.as<u64>() : nullptr,
                d->edge_drank.as<u64>(), d->edge_dlocal.as<u64>(), dbases.as<u64>(), (u32)world, d->node_base, out.lsrc.as<u32>(), tgt.as<u64>());
        KLAUNCH(own_addr_kernel, E, stream, E, me, mine.as<u64>());
    }
    KCHECK_HIP(hipGetLastError());
    DevBuf indeg(stream), outdeg(stream), out_edge(stream);
    KCHECK(indeg.alloc((N + 1) * 4)); KCHECK(outdeg.alloc((N + 1) * 4)); KCHECK(out.in_edge.alloc((N + 1) * 8)); KCHECK(out_edge.alloc((N + 1) * 4));
    KCHECK(out.inner.alloc(N + 16)); KCHECK(out.dst_inner.alloc((E + 1) * 8));
    KCHECK_HIP(hipMemsetAsync(indeg.p, 0, (N + 1) * 4, stream)); KCHECK_HIP(hipMemsetAsync(outdeg.p, 0, (N + 1) * 4, stream));
    if (E) KLAUNCH(out_deg_kernel, E, stream, out.lsrc.as<u32>(), E, outdeg.as<u32>(), out_edge.as<u32>());
    if (!chunk) {
        Routed r(stream);
        KCHECK(router.send(tgt.as<u64>(), mine.as<u64>(), E, r));
        if (r.n) KLAUNCH(in_rec_kernel, r.n, stream, r.a.as<u64>(), r.b.as<u64>(), r.n, N, indeg.as<u32>(), out.in_edge.as<u64>());
        if (N) KLAUNCH(inner_kernel, N, stream, N, indeg.as<u32>(), outdeg.as<u32>(), out.in_edge.as<u64>(), out_edge.as<u32>(), me, out.inner.as<unsigned char>());
        KCHECK_HIP(hipGetLastError());
        DevBuf a(stream);
        KCHECK(a.alloc((r.n + 1) * 8));
        if (r.n) KLAUNCH(answer_u8_kernel, r.n, stream, r.a.as<u64>(), r.n, N, out.inner.as<unsigned char>(), a.as<u64>());
        KCHECK_HIP(hipGetLastError());
        KCHECK(router.reply(r, a.as<u64>(), out.dst_inner.as<u64>()));
        return KATOME_OK;
    }
    // in chunks: the records first (the counts add up over the chunks), then, once the owners know which nodes are inner,
    // the targets once more as questions -- 8 bytes more per edge on the wire for 64 B less per edge in the Router's buffers
    uint64_t n_chunks = (E + chunk - 1) / chunk;
    KCHECK(d->comm->allreduce(&n_chunks, 1, OP_MAX));
    for (uint64_t c = 0; c < n_chunks; ++c) {
        const uint64_t at = std::min(E, c * chunk), cnt = std::min(E - at, chunk);
        Routed r(stream);
        KCHECK(router.send(tgt.as<u64>() + at, mine.as<u64>() + at, cnt, r));
        if (r.n) KLAUNCH(in_rec_kernel, r.n, stream, r.a.as<u64>(), r.b.as<u64>(), r.n, N, indeg.as<u32>(), out.in_edge.as<u64>());
        KCHECK_HIP(hipGetLastError());
    }
    mine.release();
    if (N) KLAUNCH(inner_kernel, N, stream, N, indeg.as<u32>(), outdeg.as<u32>(), out.in_edge.as<u64>(), out_edge.as<u32>(), me, out.inner.as<unsigned char>());
    KCHECK_HIP(hipGetLastError());
    DevBuf a(stream);
    for (uint64_t c = 0; c < n_chunks; ++c) {
        const uint64_t at = std::min(E, c * chunk), cnt = std::min(E - at, chunk);
        Routed r(stream);
        KCHECK(router.send(tgt.as<u64>() + at, nullptr, cnt, r));
        KCHECK(a.alloc((r.n + 1) * 8));
        if (r.n) KLAUNCH(answer_u8_kernel, r.n, stream, r.a.as<u64>(), r.n, N, out.inner.as<unsigned char>(), a.as<u64>());
        KCHECK_HIP(hipGetLastError());
        KCHECK(router.reply(r, a.as<u64>(), out.dst_inner.as<u64>() + at));
    }
    return KATOME_OK;
}

}  // namespace
