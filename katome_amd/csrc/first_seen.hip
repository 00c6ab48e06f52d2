// first_seen.hip -- first-seen order (gfx950): the finalized graph's edges brought into the order of their first insertion and its
// nodes into the order of their first touch, which is the order in which the reference's loop hands out petgraph indices
// (collections/graphs/pt_graph.rs:149,194).  dev_first_seen_order at the end of the file is the algorithm; the kernels come first.
#include <chrono>

#include "common.h"
#include "edge_keys.h"

namespace katome {

// dst[i] = map[src[idx[i]]]
__global__ __launch_bounds__(BLOCK) void gather_mapped_kernel(const u64* __restrict__ src, const u32* __restrict__ idx, const u64* __restrict__ map,
                                                               u64 n, u64* __restrict__ dst) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK) dst[i] = map[src[idx[i]]];
}
// inverse of a permutation: inv[perm[i]] = i
__global__ __launch_bounds__(BLOCK) void invert_kernel(const u32* __restrict__ perm, u64 n, u64* __restrict__ inv) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK) inv[perm[i]] = i;
}
// a node is created by the first edge insertion that touches it: as the source of the first window of a strand
// (2*seq) or as a target (2*seq + 1) -- add_single_edge_fastaq, pt_graph.rs:180-185
// Source role: the edges are in key order, so a node's out-edges are one run of equal src (and src ascending): the run's head
// takes the minimum over its run and stores it plainly -- one writer per node, no atomic.  Target role: atomicMin, afterwards.
__global__ __launch_bounds__(BLOCK) void node_first_src_kernel(const u64* __restrict__ src, const u64* __restrict__ seq, u64 n, u64* __restrict__ node_first) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK) {
        const u64 s = src[i];
        if (i > 0 && src[i - 1] == s) continue;
        u64 m = seq[i];
        for (u64 j = i + 1; j < n && src[j] == s; ++j) m = seq[j] < m ? seq[j] : m;      // (<= 4 out-edges per node; BFCounter lists may repeat)
        node_first[s] = 2 * m;
    }
}
__global__ __launch_bounds__(BLOCK) void node_first_dst_kernel(const u64* __restrict__ dst, const u64* __restrict__ seq, u64 n, u64* node_first) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK)
        atomicMin((unsigned long long*)&node_first[dst[i]], (unsigned long long)(2 * seq[i] + 1));
}
// first-seen order: the edges leave key order for sequence order.  Four separate gathers cost six random reads per edge
// (two of them through the node map); packing each edge into one 32-byte record first (its end points already mapped,
// the source map read nearly in order because sources ascend with the keys) leaves two.
struct PackedEdge { u64 k0, k1; u32 src, dst, weight, pad; };
static_assert(sizeof(PackedEdge) == 32, "packed edge layout");
template <int NW>
__global__ __launch_bounds__(BLOCK) void pack_edges_kernel(const u64* __restrict__ key, const u32* __restrict__ weight, const u64* __restrict__ src,
                                                            const u64* __restrict__ dst, const u64* __restrict__ new_id, u64 n,
                                                            PackedEdge* __restrict__ out) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK) {
        PackedEdge e;
        e.k0 = key[i * NW]; e.k1 = NW == 2 ? key[i * NW + 1] : 0;
        e.src = (u32)new_id[src[i]]; e.dst = (u32)new_id[dst[i]]; e.weight = weight[i]; e.pad = 0;
        out[i] = e;
    }
}
template <int NW>
__global__ __launch_bounds__(BLOCK) void unpack_edges_kernel(const PackedEdge* __restrict__ in, const u32* __restrict__ idx, u64 n,
                                                              u64* __restrict__ key, u32* __restrict__ weight, u64* __restrict__ src,
                                                              u64* __restrict__ dst) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK) {
        const PackedEdge e = in[idx[i]];
        key[i * NW] = e.k0;
        if (NW == 2) key[i * NW + 1] = e.k1;
        weight[i] = e.weight; src[i] = e.src; dst[i] = e.dst;
    }
}
// in place: edge arrays permuted by idx (new position i <- old position idx[i]) with end points mapped through new_id;
// `scratch` needs n * 32 bytes
static int permute_edges(uint64_t* key, uint32_t* weight, uint64_t* src, uint64_t* dst, const uint64_t* new_id, const uint32_t* idx,
                         uint64_t n, uint32_t nw, void* scratch, hipStream_t stream) {
    if (n == 0) return KATOME_OK;
    PackedEdge* aos = (PackedEdge*)scratch;
    const dim3 grid(grid_for(n, BLOCK, 256u * 32u)), blk(BLOCK);
    if (nw == 1) {
        hipLaunchKernelGGL(pack_edges_kernel<1>, grid, blk, 0, stream, key, weight, src, dst, new_id, n, aos);
        hipLaunchKernelGGL(unpack_edges_kernel<1>, grid, blk, 0, stream, aos, idx, n, key, weight, src, dst);
    } else {
        hipLaunchKernelGGL(pack_edges_kernel<2>, grid, blk, 0, stream, key, weight, src, dst, new_id, n, aos);
        hipLaunchKernelGGL(unpack_edges_kernel<2>, grid, blk, 0, stream, aos, idx, n, key, weight, src, dst);
    }
    KCHECK_HIP(hipGetLastError());
    return KATOME_OK;
}

// ---- first-seen order without sorting the nodes -------------------------------------------------------------------------
// A node's index is the rank of its first touch (2 * seq as the source of an edge's first insertion, 2 * seq + 1 as its
// target), and every touch belongs to exactly one edge: once the edges are in sequence order, the node indices are a running
// count of "this edge introduces its source / its target" -- a scan over the edges instead of a sort of the nodes.
// pack: the 32-byte record of permute_edges with the OLD end points and, in `pad`, bit 0 = introduces its source,
// bit 1 = introduces its target (node_first: the nodes' first touches)
template <int NW>
__global__ __launch_bounds__(BLOCK) void pack_edges_intro_kernel(const u64* __restrict__ key, const u32* __restrict__ weight, const u64* __restrict__ src,
                                                                  const u64* __restrict__ dst, const u64* __restrict__ seq,
                                                                  const u64* __restrict__ node_first, u64 n, u64 n_marked, PackedEdge* __restrict__ out) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK) {
        PackedEdge e;
        e.k0 = key[i * NW]; e.k1 = NW == 2 ? key[i * NW + 1] : 0;
        const u64 s = src[i], dm = dst[i], d = dm & ~DST_MARKS, q = seq[i];
        e.src = (u32)s; e.dst = (u32)d; e.weight = weight[i];
        const bool out1 = (i == 0 || src[i - 1] != s) && (i + 1 >= n || src[i + 1] != s);     // the source has this out-edge only
        // (targets below n_marked carry the answer as a mark from the merge; the others -- nodes without out-edges, or no merge --
        // are looked up: node_first[s] is read in order, node_first[d] is not)
        const bool fd = d < n_marked ? (dm & DST_FD) != 0 : node_first[d] == 2 * q + 1;
        e.pad = (node_first[s] == 2 * q ? 1u : 0u) | (fd ? 2u : 0u) | ((dm & DST_IN1) ? 4u : 0u) | (out1 ? 8u : 0u);
        out[i] = e;
    }
}
// unpack in sequence order (new position i <- old position idx[i]); the flags ride in bit 32 of the (old) end points;
// cnt[i] = nodes the edge introduces
template <int NW>
__global__ __launch_bounds__(BLOCK) void unpack_edges_intro_kernel(const PackedEdge* __restrict__ in, const u32* __restrict__ idx, u64 n,
                                                                    u64* __restrict__ key, u32* __restrict__ weight, u64* __restrict__ src,
                                                                    u64* __restrict__ dst, u32* __restrict__ cnt) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK) {
        const PackedEdge e = in[idx[i]];
        key[i * NW] = e.k0;
        if (NW == 2) key[i * NW + 1] = e.k1;
        weight[i] = e.weight;
        src[i] = (u64)e.src | ((u64)(e.pad & 1u) << 32) | ((u64)((e.pad >> 3) & 1u) << 33);
        dst[i] = (u64)e.dst | ((u64)((e.pad >> 1) & 1u) << 32) | ((u64)((e.pad >> 2) & 1u) << 33);
        cnt[i] = (e.pad & 1u) + ((e.pad >> 1) & 1u);
    }
}
// offs = exclusive scan of cnt: the edge's nodes get indices offs[i] (source, if introduced) and the next one (target).
// The indices reach the OTHER edges of a node through new_id[old index] -- a scattered write and a scattered read per node,
// the two most expensive steps of the renumbering.  Most nodes never need either: in sequence order an edge is usually
// followed by the next window of the same read, so a node is introduced as the target of edge i and used as the source of
// edge i + 1 (remap_ends_kernel reads it off its neighbour); when it has no other in- or out-edge (bits 33: marks from the
// merge and from the runs of sources) nobody else will ask for it and the write is left out as well.
template <int NW>
__global__ __launch_bounds__(BLOCK) void assign_nodes_kernel(const u64* __restrict__ key, const u64* __restrict__ src, const u64* __restrict__ dst,
                                                              const u64* __restrict__ offs, u64 n, u32 k, u64* __restrict__ new_id,
                                                              u64* __restrict__ node_key) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK) {
        const u64 s = src[i], d = dst[i];
        const u32 fs = (u32)(s >> 32) & 1u, fd = (u32)(d >> 32) & 1u;
        if (!(fs | fd)) continue;
        const Key<NW> e = load_key<NW>(key, i);
        const u64 base = offs[i];
        if (fs) { new_id[(u32)s] = base; store_key<NW>(node_key, base, source_node(e)); }
        if (fd) {
            store_key<NW>(node_key, base + fs, target_node(e, k));
            bool alone = false;                         // one in-edge (this one), one out-edge, and that one comes next
            if (((d >> 33) & 1u) && i + 1 < n) { const u64 s1 = src[i + 1]; alone = ((s1 >> 33) & 1u) && (u32)s1 == (u32)d; }
            if (!alone) new_id[(u32)d] = base + fs;
        }
    }
}
__global__ __launch_bounds__(BLOCK) void remap_ends_kernel(const u64* __restrict__ src, const u64* __restrict__ dst, const u64* __restrict__ offs,
                                                            const u64* __restrict__ new_id, u64 n, u64* __restrict__ osrc, u64* __restrict__ odst) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK) {
        const u64 s = src[i], d = dst[i];
        const u32 fs = (u32)(s >> 32) & 1u, fd = (u32)(d >> 32) & 1u;
        const u64 base = (fs | fd) ? offs[i] : 0;
        u64 so;
        if (fs) so = base;
        else {
            const u64 dp = i ? dst[i - 1] : 0;
            if (i && ((dp >> 32) & 1u) && (u32)dp == (u32)s) so = offs[i - 1] + ((src[i - 1] >> 32) & 1u);      // introduced by the edge before
            else so = new_id[(u32)s];
        }
        osrc[i] = so;
        odst[i] = fd ? base + fs : new_id[(u32)d];
    }
}
__global__ __launch_bounds__(BLOCK) void clear_marks_kernel(u64* __restrict__ v, u64 n) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK) v[i] &= ~DST_MARKS;
}
static int pack_edges_intro(const uint64_t* key, const uint32_t* weight, const uint64_t* src, const uint64_t* dst, const uint64_t* seq,
                            const uint64_t* node_first, uint64_t n, uint32_t nw, void* aos, hipStream_t stream, uint64_t n_marked) {
    if (n == 0) return KATOME_OK;
    const dim3 grid(grid_for(n, BLOCK, 256u * 32u)), blk(BLOCK);
    if (nw == 1) hipLaunchKernelGGL(pack_edges_intro_kernel<1>, grid, blk, 0, stream, key, weight, src, dst, seq, node_first, n, n_marked, (PackedEdge*)aos);
    else         hipLaunchKernelGGL(pack_edges_intro_kernel<2>, grid, blk, 0, stream, key, weight, src, dst, seq, node_first, n, n_marked, (PackedEdge*)aos);
    KCHECK_HIP(hipGetLastError());
    return KATOME_OK;
}
static int unpack_edges_intro(const void* aos, const uint32_t* idx, uint64_t n, uint32_t nw, uint64_t* key, uint32_t* weight, uint64_t* src,
                              uint64_t* dst, uint32_t* cnt, hipStream_t stream) {
    if (n == 0) return KATOME_OK;
    const dim3 grid(grid_for(n, BLOCK, 256u * 32u)), blk(BLOCK);
    if (nw == 1) hipLaunchKernelGGL(unpack_edges_intro_kernel<1>, grid, blk, 0, stream, (const PackedEdge*)aos, idx, n, key, weight, src, dst, cnt);
    else         hipLaunchKernelGGL(unpack_edges_intro_kernel<2>, grid, blk, 0, stream, (const PackedEdge*)aos, idx, n, key, weight, src, dst, cnt);
    KCHECK_HIP(hipGetLastError());
    return KATOME_OK;
}
static int assign_nodes(const uint64_t* key, const uint64_t* src, const uint64_t* dst, const uint64_t* offs, uint64_t n, uint32_t nw, uint32_t k,
                        uint64_t* new_id, uint64_t* node_key, uint64_t* out_src, uint64_t* out_dst, hipStream_t stream) {
    if (n == 0) return KATOME_OK;
    const dim3 grid(grid_for(n, BLOCK, 256u * 32u)), blk(BLOCK);
    if (nw == 1) hipLaunchKernelGGL(assign_nodes_kernel<1>, grid, blk, 0, stream, key, src, dst, offs, n, k, new_id, node_key);
    else         hipLaunchKernelGGL(assign_nodes_kernel<2>, grid, blk, 0, stream, key, src, dst, offs, n, k, new_id, node_key);
    hipLaunchKernelGGL(remap_ends_kernel, grid, blk, 0, stream, src, dst, offs, new_id, n, out_src, out_dst);
    KCHECK_HIP(hipGetLastError());
    return KATOME_OK;
}

// ---- the algorithm ---------------------------------------------------------------------------------------------------------------
// KATOME_TRACE_FINALIZE: the time since the lap before, stream drained, on stderr
struct Laps {
    hipStream_t stream;
    const bool trace = getenv("KATOME_TRACE_FINALIZE") != nullptr;
    std::chrono::steady_clock::time_point t_last = std::chrono::steady_clock::now();
    void operator()(const char* what) {
        if (!trace) return;
        (void)hipStreamSynchronize(stream);
        const auto t = std::chrono::steady_clock::now();
        fprintf(stderr, "[finalize] %-22s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(t - t_last).count());
        t_last = t;
    }
};

// No sort of the nodes: every node is introduced by exactly one edge (the one whose first insertion is the node's first touch), so
// with the edges in sequence order the node indices are a running count.  aos: E * 32 + 64 bytes, eperm: E + 1 u32; both are
// given back on the way, as is node_first
static int order_by_introducing_edge(FirstSeenGraph& g, DevBuf& node_first, uint64_t n_marked, uint32_t seq_bits, DevBuf& eperm, DevBuf& aos,
                                     Laps& lap, hipStream_t stream) {
    const u64 E = g.n_edges, N = g.n_nodes;
    const u32 nw = g.nw;
    DevBuf new_id(stream);
    KCHECK(pack_edges_intro(g.edge_key->as<u64>(), g.edge_weight->as<u32>(), g.edge_src->as<u64>(), g.edge_dst->as<u64>(), g.edge_seq->as<u64>(),
                            node_first.as<u64>(), E, nw, aos.p, stream, n_marked));
    node_first.release();
    lap("pack + who introduces");
    KCHECK(dev_iota(eperm.as<u32>(), E, stream));
    KCHECK(dev_sort_bufs(*g.edge_seq, &eperm, E, 1, seq_bits, stream));       // eperm[new] = old; edge_seq now ascending
    lap("sort edges by seq");
    DevBuf cnt(stream), offs(stream), onode(stream);
    KCHECK(cnt.alloc((E + 1) * 4));
    KCHECK(unpack_edges_intro(aos.p, eperm.as<u32>(), E, nw, g.edge_key->as<u64>(), g.edge_weight->as<u32>(), g.edge_src->as<u64>(), g.edge_dst->as<u64>(),
                              cnt.as<u32>(), stream));
    aos.release(); eperm.release();
    lap("edges to seq order");
    KCHECK(offs.alloc((E + 2) * 8));
    KCHECK(dev_scan_counts(cnt.as<u32>(), E, offs.as<u64>(), stream));
    uint64_t introduced = 0;
    KCHECK_HIP(hipMemcpyAsync(&introduced, offs.as<u64>() + E, 8, hipMemcpyDeviceToHost, stream));
    KCHECK_HIP(hipStreamSynchronize(stream));
    lap("scan");
    if (introduced != N) { set_error("first-seen order: %llu nodes introduced, %llu nodes known", (unsigned long long)introduced, (unsigned long long)N); return KATOME_E_DEVICE; }
    cnt.release();
    DevBuf osrc(stream), odst(stream);
    KCHECK(new_id.alloc((N + 1) * 8));
    KCHECK(onode.alloc((N + 1) * 8 * nw));
    KCHECK(osrc.alloc((E + 1) * 8));
    KCHECK(odst.alloc((E + 1) * 8));
    KCHECK(assign_nodes(g.edge_key->as<u64>(), g.edge_src->as<u64>(), g.edge_dst->as<u64>(), offs.as<u64>(), E, nw, g.k, new_id.as<u64>(), onode.as<u64>(),
                        osrc.as<u64>(), odst.as<u64>(), stream));
    g.node_key->adopt(onode);
    g.edge_src->adopt(osrc);
    g.edge_dst->adopt(odst);
    lap("node indices + end points");
    return KATOME_OK;
}

// the edges to the order eperm (new position i <- old position eperm[i]), their end points through new_id, one array at a time:
// six random reads per edge, for when permute_edges' scratch is not to be had
static int permute_edges_by_gathers(FirstSeenGraph& g, const DevBuf& new_id, const DevBuf& eperm, hipStream_t stream) {
    const u64 E = g.n_edges;
    {
        DevBuf o(stream);
        KCHECK(o.alloc((E + 1) * 8 * g.nw));
        KCHECK(dev_gather_keys(g.edge_key->as<u64>(), eperm.as<u32>(), E, g.nw, o.as<u64>(), stream));
        g.edge_key->adopt(o);
    }
    {
        DevBuf o(stream);
        KCHECK(o.alloc((E + 1) * 4));
        KCHECK(dev_gather_u32(g.edge_weight->as<u32>(), eperm.as<u32>(), E, o.as<u32>(), stream));
        g.edge_weight->adopt(o);
    }
    for (DevBuf* ends : {g.edge_src, g.edge_dst}) {
        DevBuf o(stream);
        KCHECK(o.alloc((E + 1) * 8));
        hipLaunchKernelGGL(gather_mapped_kernel, dim3(grid_for(E, BLOCK, 256u * 32u)), dim3(BLOCK), 0, stream, ends->as<u64>(), eperm.as<u32>(), new_id.as<u64>(), E,
                           o.as<u64>());
        KCHECK_HIP(hipGetLastError());
        ends->adopt(o);
    }
    return KATOME_OK;
}

// KATOME_SORT_NODES, or no room for the route above: the nodes are sorted by their first touch, the edges by their sequence number
static int order_by_sorting_nodes(FirstSeenGraph& g, DevBuf& node_first, uint32_t seq_bits, DevBuf& eperm, Laps& lap, hipStream_t stream) {
    const u64 E = g.n_edges, N = g.n_nodes;
    const u32 nw = g.nw;
    DevBuf new_id(stream);
    // (the merge's marks: only the other route reads them)
    hipLaunchKernelGGL(clear_marks_kernel, dim3(grid_for(E, BLOCK, 256u * 32u)), dim3(BLOCK), 0, stream, g.edge_dst->as<u64>(), E);
    KCHECK_HIP(hipGetLastError());
    KCHECK(new_id.alloc((N + 1) * 8));
    {
        DevBuf nperm(stream), onode(stream);
        KCHECK(nperm.alloc((N + 1) * 4));
        KCHECK(dev_iota(nperm.as<u32>(), N, stream));
        KCHECK(dev_sort_bufs(node_first, &nperm, N, 1, seq_bits, stream));        // nperm[new] = old
        lap("sort nodes");
        node_first.release();
        hipLaunchKernelGGL(invert_kernel, dim3(grid_for(N, BLOCK, 256u * 32u)), dim3(BLOCK), 0, stream, nperm.as<u32>(), N, new_id.as<u64>());   // new_id[old] = new
        KCHECK_HIP(hipGetLastError());
        KCHECK(onode.alloc((N + 1) * 8 * nw));
        KCHECK(dev_gather_keys(g.node_key->as<u64>(), nperm.as<u32>(), N, nw, onode.as<u64>(), stream));
        g.node_key->adopt(onode);
        lap("invert + node keys");
    }
    KCHECK(dev_iota(eperm.as<u32>(), E, stream));
    KCHECK(dev_sort_bufs(*g.edge_seq, &eperm, E, 1, seq_bits, stream));           // eperm[new] = old; edge_seq now ascending
    lap("sort edges by seq");
    // one 32-byte record per edge, read once at random (permute_edges); if that much scratch is not to be had, the four separate gathers
    DevBuf aos2(stream);
    if (aos2.alloc(E * 32 + 64) != KATOME_OK) return permute_edges_by_gathers(g, new_id, eperm, stream);
    return permute_edges(g.edge_key->as<u64>(), g.edge_weight->as<u32>(), g.edge_src->as<u64>(), g.edge_dst->as<u64>(), new_id.as<u64>(), eperm.as<u32>(), E, nw,
                         aos2.p, stream);
}

int dev_first_seen_order(FirstSeenGraph& g, DevBuf& node_first, uint64_t n_marked, uint32_t seq_bits, hipStream_t stream) {
    const u64 E = g.n_edges, N = g.n_nodes;
    if (E == 0) return KATOME_OK;
    if (N >= (1ull << 32)) { set_error("first-seen order: more than 2^32 nodes on one GPU"); return KATOME_E_UNSUPPORTED; }
    Laps lap{stream};
    // (buffers are taken and given back one at a time: at C3 every one of them is 6-13 GB)
    DevBuf eperm(stream), aos(stream);
    if (!node_first.p) {
        // a node is created by the first edge insertion that touches it (the edges are in key order: src ascending in runs)
        KCHECK(node_first.alloc((N + 1) * 8));
        KCHECK_HIP(hipMemsetAsync(node_first.p, 0xFF, N * 8, stream));
        const dim3 grid(grid_for(E, BLOCK, 256u * 32u)), blk(BLOCK);
        hipLaunchKernelGGL(node_first_src_kernel, grid, blk, 0, stream, g.edge_src->as<u64>(), g.edge_seq->as<u64>(), E, node_first.as<u64>());
        hipLaunchKernelGGL(node_first_dst_kernel, grid, blk, 0, stream, g.edge_dst->as<u64>(), g.edge_seq->as<u64>(), E, node_first.as<u64>());
        KCHECK_HIP(hipGetLastError());
    }
    lap("node_first");
    KCHECK(eperm.alloc((E + 1) * 4));
    if (!getenv("KATOME_SORT_NODES") && aos.alloc(E * 32 + 64) == KATOME_OK) {
        KCHECK(order_by_introducing_edge(g, node_first, n_marked, seq_bits, eperm, aos, lap, stream));
    } else {
        aos.release();
        KCHECK(order_by_sorting_nodes(g, node_first, seq_bits, eperm, lap, stream));
    }
    lap("edges to seq order");
    return KATOME_OK;
}

}  // namespace katome
