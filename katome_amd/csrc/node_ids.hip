// node_ids.hip -- the graph's nodes read off the sorted edge list (gfx950): PtGraph node numbering (reference
// collections/graphs/pt_graph.rs:142-154), every edge's source and target id, the endpoints of each edge (compress_kmer halves,
// compress.rs:23-26) and the compress_edge labels (compress.rs:250-271; post-pass pt_graph.rs:339-343).  The sort, unique and scan it
// calls are radix.hip's.  All streaming, HBM-bound passes; no MFMA (integer keys).
#include <algorithm>

#include "common.h"
#include "edge_keys.h"

namespace katome {

// ---- node numbering straight from the sorted edge list --------------------------------------------
// Edges are sorted by packed k-mer, so their source (k-1)-mers (key >> 2) are sorted too: the nodes
// that have out-edges are the run heads of that sequence -- no sort needed.  Targets are looked up in
// that list; the few that are absent (nodes without out-edges: read ends nothing continues) are
// collected, sorted and appended.  Node ids: sources in ascending key order, then the out-edge-less
// nodes in ascending key order (add_fasta_node, pt_graph.rs:142-154, numbers in first-seen order; no
// order is pinned by the reference -- DESIGN.md section 1).
template <int NW>
__global__ __launch_bounds__(BLOCK) void src_count_kernel(const u64* __restrict__ keys, u64 n, u32* __restrict__ block_counts) {
    __shared__ u32 wsum[BLOCK / 64];
    const u64 base = (u64)blockIdx.x * UNIQ_TILE + threadIdx.x;          // rows of BLOCK consecutive edges: coalesced loads
    u32 mine = 0;
#pragma unroll
    for (int j = 0; j < UNIQ_ITEMS; ++j) if (base + (u64)j * BLOCK < n && is_src_head<NW>(keys, base + (u64)j * BLOCK)) ++mine;
    u32 total;
    (void)block_excl_scan(mine, wsum, total);
    if (threadIdx.x == 0) block_counts[blockIdx.x] = total;
}
// writes the distinct sources (= node keys) and every edge's source id.  Rows of BLOCK consecutive edges are
// taken one after the other (coalesced loads and stores); a ballot scan per row keeps the running head count.
// LABELS: the edges' labels too (labels_kernel's bytes exactly: [pad][ceil(k/4) bytes] per edge), from the keys the kernel holds
// anyway -- built in LDS, UNIQ_TILE * stride bytes, and written out as whole dwords, so that no second pass reads the keys
template <int NW, bool LABELS = false>
__global__ __launch_bounds__(BLOCK) void src_write_kernel(const u64* __restrict__ keys, u64 n, const u64* __restrict__ block_offs,
                                                           u64* __restrict__ nodes, u64* __restrict__ edge_src, u64* __restrict__ seg_edge, u32 seg_nodes,
                                                           u32 k, uint8_t* __restrict__ labels) {
    __shared__ u32 wtot[UNIQ_ITEMS][BLOCK / 64];
    extern __shared__ u32 src_lbuf[];                      // LABELS: [UNIQ_TILE * stride / 4]
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64 base = (u64)blockIdx.x * UNIQ_TILE;
    bool head[UNIQ_ITEMS]; u32 before[UNIQ_ITEMS];
    Key<NW> key[UNIQ_ITEMS], prev[UNIQ_ITEMS];             // the block's keys, which stay in registers, and the keys of the edges before them
    const u32 stride = LABELS ? label_stride_for_k(k) : 0u, pad = LABELS ? label_pad_for_k(k) : 0u;
    // A whole block (every block but the list's last) loads its keys and their predecessors without a test, so that all of them go
    // out together: behind `e < n && ...` in the loop below hipcc 7.2 waited for every row's predecessor before it loaded the next
    // (9.8 -> 8.5 ms at C3, profiles/load_chains.md).  Edge 0 has no predecessor and reads itself: it is a head whatever it reads.
    if (base + UNIQ_TILE <= n) {
#pragma unroll
        for (int j = 0; j < UNIQ_ITEMS; ++j) {
            const u64 e = base + (u64)j * BLOCK + threadIdx.x;
            key[j] = load_key<NW>(keys, e); prev[j] = load_key<NW>(keys, e ? e - 1 : 0);
        }
    } else {
#pragma unroll
        for (int j = 0; j < UNIQ_ITEMS; ++j) {
            const u64 e = base + (u64)j * BLOCK + threadIdx.x;
            if (e < n) { key[j] = load_key<NW>(keys, e); prev[j] = load_key<NW>(keys, e ? e - 1 : 0); }
        }
    }
#pragma unroll
    for (int j = 0; j < UNIQ_ITEMS; ++j) {
        const u64 e = base + (u64)j * BLOCK + threadIdx.x;
        head[j] = e < n && (e == 0 || !key_eq(key_shr(key[j], 2), key_shr(prev[j], 2)));          // (is_src_head)
        const u64 m = __ballot(head[j]);
        before[j] = __popcll(m & (lane ? (~0ull >> (64 - lane)) : 0ull));
        if (lane == 0) wtot[j][wave] = __popcll(m);
        if constexpr (LABELS) {
            if (e < n) {
                uint8_t* p = reinterpret_cast<uint8_t*>(src_lbuf) + (j * BLOCK + threadIdx.x) * stride;
                p[0] = (uint8_t)pad;
                for (u32 i = 0; i + 1 < stride; ++i) p[1 + i] = label_byte(key[j], k, i);
            }
        }
    }
    __syncthreads();
    if constexpr (LABELS) {
        // UNIQ_TILE * stride is a multiple of 4, so a block's labels start on a dword; the array's last bytes leave one by one
        const u32 cnt = (u32)((n - base) < (u64)UNIQ_TILE ? (n - base) : (u64)UNIQ_TILE), nbytes = cnt * stride;
        const u64 byte0 = base * stride;
        u32* o32 = reinterpret_cast<u32*>(labels + byte0);
        for (u32 i = threadIdx.x; i < nbytes / 4; i += BLOCK) o32[i] = src_lbuf[i];
        for (u32 i = (nbytes / 4) * 4 + threadIdx.x; i < nbytes; i += BLOCK) labels[byte0 + i] = reinterpret_cast<uint8_t*>(src_lbuf)[i];
    }
    u64 carry = block_offs[blockIdx.x];
#pragma unroll
    for (int j = 0; j < UNIQ_ITEMS; ++j) {
        u32 woff = 0, total = 0;
#pragma unroll
        for (int w = 0; w < BLOCK / 64; ++w) { if (w < (int)wave) woff += wtot[j][w]; total += wtot[j][w]; }
        const u64 e = base + (u64)j * BLOCK + threadIdx.x;
        if (e < n) {
            const u64 pos = carry + woff + before[j];           // heads strictly before this edge
            if (head[j]) {
                store_key<NW>(nodes, pos, key_shr(key[j], 2));
                if (seg_edge && pos % seg_nodes == 0) seg_edge[pos / seg_nodes] = e;      // first out-edge of every seg_nodes-th source
            }
            edge_src[e] = head[j] ? pos : pos - 1;
        }
        carry += total;
    }
}
// edge_dst[e] = position of the edge's target in `nodes`, or ~0 when it is not a source of any edge
template <int NW>
__global__ __launch_bounds__(BLOCK) void dst_rank_kernel(const u64* __restrict__ nodes, u64 n_nodes, u32 key_bits, u32 B,
                                                          const u64* __restrict__ index, const u64* __restrict__ keys, u64 n,
                                                          u32 k, u64* __restrict__ edge_dst, u64* __restrict__ n_missing) {
    u32 miss = 0;
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK) {
        Key<NW> key = target_node(load_key<NW>(keys, i), k);
        u32 b = top_bits(key, key_bits, B);
        u64 lo = index[b], hi = index[b + 1];
        while (lo < hi) {
            u64 mid = (lo + hi) >> 1;
            if (key_lt(load_key<NW>(nodes, mid), key)) lo = mid + 1; else hi = mid;
        }
        const bool found = lo < n_nodes && key_eq(load_key<NW>(nodes, lo), key);
        edge_dst[i] = found ? lo : ~0ull;
        miss += !found;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) miss += __shfl_down(miss, o, 64);
    if ((threadIdx.x & 63) == 0 && miss) atomicAdd((unsigned long long*)n_missing, (unsigned long long)miss);
}
// gather the targets that were not found (unordered; they are sorted afterwards).  One cursor atomic per
// workgroup tile: the misses are sparse, and one atomic per wave on a single address serialises.
template <int NW>
__global__ __launch_bounds__(BLOCK) void missing_gather_kernel(const u64* __restrict__ keys, u64 n, u32 k, const u64* __restrict__ edge_dst,
                                                                u64* __restrict__ out, u64* __restrict__ out_edge, u64* cursor) {
    __shared__ u32 wsum[BLOCK / 64];
    __shared__ u64 block_base;
    const u64 tile = (u64)BLOCK * UNIQ_ITEMS;
    for (u64 t0 = (u64)blockIdx.x * tile; t0 < n; t0 += (u64)gridDim.x * tile) {
        bool miss[UNIQ_ITEMS]; u32 mine = 0;
#pragma unroll
        for (int j = 0; j < UNIQ_ITEMS; ++j) {
            const u64 i = t0 + (u64)j * BLOCK + threadIdx.x;
            miss[j] = i < n && edge_dst[i] == ~0ull;
            mine += miss[j];
        }
        u32 total;
        const u32 excl = block_excl_scan(mine, wsum, total);
        if (threadIdx.x == 0 && total) block_base = atomicAdd((unsigned long long*)cursor, (unsigned long long)total);
        __syncthreads();
        if (total) {
            u64 pos = block_base + excl;
#pragma unroll
            for (int j = 0; j < UNIQ_ITEMS; ++j)
                if (miss[j]) {
                    const u64 e = t0 + (u64)j * BLOCK + threadIdx.x;
                    store_key<NW>(out, pos, target_node(load_key<NW>(keys, e), k));
                    out_edge[pos] = e;
                    ++pos;
                }
        }
        __syncthreads();
    }
}
// second lookup, only for the edges whose target was not a source: id = n_sources + rank among the extra nodes
template <int NW>
__global__ __launch_bounds__(BLOCK) void missing_rank_kernel(const u64* __restrict__ miss_key, const u64* __restrict__ miss_edge, u64 n_miss,
                                                              const u64* __restrict__ extra, u64 n_extra, u64 n_sources,
                                                              u64* __restrict__ edge_dst) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n_miss; i += (u64)gridDim.x * BLOCK) {
        Key<NW> key = load_key<NW>(miss_key, i);
        u64 lo = 0, hi = n_extra;
        while (lo < hi) {
            u64 mid = (lo + hi) >> 1;
            if (key_lt(load_key<NW>(extra, mid), key)) lo = mid + 1; else hi = mid;
        }
        edge_dst[miss_edge[i]] = n_sources + lo;
    }
}

// ---- targets looked up by merging ----------------------------------------------------------------------------------
// Sorted by packed k-mer, the edges fall into four quarters by their first base, and inside a quarter the TARGETS (the low
// 2(k-1) bits) ascend too.  The sources (ascending) are cut into segments of DST_SEG nodes; a workgroup stages its segment
// in LDS and walks, quarter by quarter, the one contiguous stretch of edges whose targets lie in the segment's key range:
// sources and edges are each read once, coalesced, and a target costs a binary search in LDS -- instead of a bucket look-up
// and a binary search in HBM per edge (dst_rank_kernel) and a second pass that collects the targets not found
// (missing_gather_kernel): those are staged in LDS and leave with one cursor atomic per MISS_CAP of them.
#ifndef KATOME_DST_SEG
#define KATOME_DST_SEG 2048
#endif
constexpr u32 DST_SEG = KATOME_DST_SEG;
// edges per thread and trip (loads and searches in flight): 2 for one-word k-mers, 4 for two-word ones -- measured both ways at C3
// (11.4 ms with 2, 15.4 with 4) and at k = 40 / 50 M reads (12.0 with 2, 9.2 with 4); -DKATOME_DST_ROWS=n sets both
template <int NW> struct DstRows {
#ifdef KATOME_DST_ROWS
    static constexpr u32 value = KATOME_DST_ROWS;
#else
    static constexpr u32 value = NW == 1 ? 2 : 4;
#endif
};
template <int NW> struct MissCap { static constexpr u32 value = (DstRows<NW>::value > 2 ? 2048 : 1024) / NW; };
static_assert(MissCap<1>::value >= DstRows<1>::value * BLOCK && MissCap<2>::value >= DstRows<2>::value * BLOCK, "a whole trip of misses fits the staging buffer");

template <int NW> __device__ __forceinline__ Key<NW> with_quarter(Key<NW> node, u32 q, u32 node_bits) {
    if (NW == 1) node.w[0] |= (u64)q << node_bits;
    else if (node_bits >= 64) node.w[0] |= (u64)q << (node_bits - 64);
    else { node.w[NW - 1] |= (u64)q << node_bits; node.w[0] |= (u64)q >> (64 - node_bits); }      // (k = 32: node_bits = 62)
    return node;
}
template <int NW> __device__ __forceinline__ u64 lower_bound_keys(const u64* __restrict__ keys, u64 n, const Key<NW>& x) {
    u64 lo = 0, hi = n;
    while (lo < hi) {
        const u64 mid = (lo + hi) >> 1;
        if (key_lt(load_key<NW>(keys, mid), x)) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// seg[q][s] = first edge of quarter q whose target is not below the first source of segment s (s = 0: the quarter's start;
// s = n_seg: its end)
template <int NW>
__global__ __launch_bounds__(BLOCK) void dst_seg_kernel(const u64* __restrict__ nodes, const u64* __restrict__ keys, u64 n, u32 node_bits,
                                                         u64 n_seg, u64* __restrict__ seg) {
    const u64 total = 4 * (n_seg + 1);
    for (u64 t = (u64)blockIdx.x * BLOCK + threadIdx.x; t < total; t += (u64)gridDim.x * BLOCK) {
        const u32 q = (u32)(t / (n_seg + 1));
        const u64 s = t % (n_seg + 1);
        Key<NW> v;
#pragma unroll
        for (int j = 0; j < NW; ++j) v.w[j] = 0;
        u64 pos;
        if (s == n_seg) pos = q == 3 ? n : lower_bound_keys<NW>(keys, n, with_quarter(v, q + 1, node_bits));
        else {
            if (s) v = load_key<NW>(nodes, s * DST_SEG);
            pos = lower_bound_keys<NW>(keys, n, with_quarter(v, q, node_bits));
        }
        seg[t] = pos;
    }
}
// edge_dst[e] = position of the edge's target among the sources, or ~0; the targets not found go to miss_key / miss_edge
// (unordered, as many as fit miss_cap) and are counted in *cursor
// FIRST (first-seen order): seq[e] = sequence number of the edge's first insertion; node_first[v] (holding the source-role
// minimum, 2*seq, or all-ones) is lowered to the first touch as a target, 2*seq + 1, with atomics in LDS only
template <int NW, bool FIRST>
__global__ __launch_bounds__(BLOCK) void dst_merge_kernel(const u64* __restrict__ nodes, u64 n_src, const u64* __restrict__ keys, u32 k,
                                                           u64 n_seg, const u64* __restrict__ seg, u64* __restrict__ edge_dst,
                                                           u64* __restrict__ miss_key, u64* __restrict__ miss_edge, u64 miss_cap, u64* cursor,
                                                           const u64* __restrict__ seq, u64* __restrict__ node_first,
                                                           const u64* __restrict__ edge_src, const u64* __restrict__ seg_edge, u64 n_edges) {
    constexpr u32 MISS_CAP = MissCap<NW>::value, DST_ROWS = DstRows<NW>::value;
    extern __shared__ u64 lmem[];
    u64* ls = lmem;                                     // [DST_SEG * NW] the segment's sources
    u64* lmk = ls + DST_SEG * NW;                       // [MISS_CAP * NW] + [MISS_CAP]: targets not found, and their edges
    u64* lme = lmk + MISS_CAP * NW;
    u64* lfirst = lme + MISS_CAP;                       // FIRST: [DST_SEG] first touch as a target
    u32* lonce = reinterpret_cast<u32*>(lfirst + DST_SEG);   // FIRST: two bitmaps [DST_SEG / 32]: has an in-edge, has several
    u32* lmore = lonce + DST_SEG / 32;
    __shared__ u32 lmiss;
    __shared__ u64 lbase;
    const u32 tid = threadIdx.x;
    auto flush = [&]() {                                // (called by every thread, between barriers)
        const u32 m = lmiss;
        if (tid == 0 && m) lbase = atomicAdd((unsigned long long*)cursor, (unsigned long long)m);
        __syncthreads();
        if (m) {
            const u64 base = lbase;
            for (u32 j = tid; j < m; j += BLOCK)
                if (base + j < miss_cap) {
                    Key<NW> x;
#pragma unroll
                    for (int w = 0; w < NW; ++w) x.w[w] = lmk[j * NW + w];
                    store_key<NW>(miss_key, base + j, x);
                    miss_edge[base + j] = lme[j];
                }
        }
        __syncthreads();
        if (tid == 0) lmiss = 0;
        __syncthreads();
    };
    for (u64 sg = blockIdx.x; sg < n_seg; sg += gridDim.x) {
        const u64 a = sg * DST_SEG;
        const u32 cnt = (u32)((n_src - a) < (u64)DST_SEG ? (n_src - a) : (u64)DST_SEG);
        // the four stretches (one per quarter) are walked as one list of `total` edges, so that a trip is full whatever the
        // quarters' sizes, and the loads of the next trip are issued before this one's searches (a segment was a chain of
        // ~9 memory round trips: two per quarter, the second nearly empty)
        const u64 lo0 = seg[sg], lo1 = seg[(n_seg + 1) + sg], lo2 = seg[2 * (n_seg + 1) + sg], lo3 = seg[3 * (n_seg + 1) + sg];
        const u64 c1 = seg[sg + 1] - lo0, c2 = c1 + (seg[(n_seg + 1) + sg + 1] - lo1), c3 = c2 + (seg[2 * (n_seg + 1) + sg + 1] - lo2);
        const u64 total = c3 + (seg[3 * (n_seg + 1) + sg + 1] - lo3);
        auto edge_of = [&](u64 v) -> u64 { return v < c1 ? lo0 + v : v < c2 ? lo1 + (v - c1) : v < c3 ? lo2 + (v - c2) : lo3 + (v - c3); };
        Key<NW> e[DST_ROWS], en[DST_ROWS]; u64 sq[DST_ROWS], sqn[DST_ROWS], ei[DST_ROWS], ein[DST_ROWS];
        auto fetch = [&](u64 c, Key<NW>* ek, u64* es, u64* ex) {
#pragma unroll
            for (u32 r = 0; r < DST_ROWS; ++r) {
                const u64 v = c + (u64)r * BLOCK + tid;
#pragma unroll
                for (int w = 0; w < NW; ++w) ek[r].w[w] = 0;
                es[r] = 0; ex[r] = ~0ull;
                if (v < total) { const u64 i = edge_of(v); ex[r] = i; ek[r] = load_key<NW>(keys, i); if (FIRST) es[r] = seq[i]; }
            }
        };
        fetch(0, e, sq, ei);                            // (in flight together with the segment's sources below)
        Key<NW> stage[DST_SEG / BLOCK];
#pragma unroll
        for (u32 r = 0; r < DST_SEG / BLOCK; ++r) { const u32 j = r * BLOCK + tid; if (j < cnt) stage[r] = load_key<NW>(nodes, a + j); }
#pragma unroll
        for (u32 r = 0; r < DST_SEG / BLOCK; ++r) {
            const u32 j = r * BLOCK + tid;
            if (j < cnt) {
#pragma unroll
                for (int w = 0; w < NW; ++w) ls[j * NW + w] = stage[r].w[w];
                if (FIRST) lfirst[j] = ~0ull;
            }
        }
        if (FIRST && tid < 2 * (DST_SEG / 32)) lonce[tid] = 0;          // (lmore follows lonce)
        if (tid == 0) lmiss = 0;
        __syncthreads();
        if (FIRST) {    // source role: the segment's out-edges are one stretch of the edge list; first touch 2 * seq (pt_graph.rs:180-185)
            const u64 e0 = seg_edge[sg], e1 = sg + 1 < n_seg ? seg_edge[sg + 1] : n_edges;
            for (u64 e = e0 + tid; e < e1; e += BLOCK)
                atomicMin((unsigned long long*)&lfirst[(u32)(edge_src[e] - a)], (unsigned long long)(2 * seq[e]));
        }
        for (u64 c = 0; c < total; c += (u64)DST_ROWS * BLOCK) {
            fetch(c + (u64)DST_ROWS * BLOCK, en, sqn, ein);
            // the searches of a thread's edges advance in lockstep, a fixed number of halving steps each (branch-free lower
            // bound): DST_ROWS independent LDS reads are in flight per step
            Key<NW> d[DST_ROWS]; u32 l[DST_ROWS];
#pragma unroll
            for (u32 r = 0; r < DST_ROWS; ++r) { d[r] = target_node(e[r], k); l[r] = 0; }
#pragma unroll
            for (u32 step = DST_SEG; step >= 1; step >>= 1) {
#pragma unroll
                for (u32 r = 0; r < DST_ROWS; ++r) {
                    const u32 idx = l[r] + step;
                    const bool in = idx <= cnt;
                    Key<NW> x;
#pragma unroll
                    for (int w = 0; w < NW; ++w) x.w[w] = ls[(in ? idx - 1 : 0) * NW + w];
                    if (in && key_lt(x, d[r])) l[r] = idx;
                }
            }
#pragma unroll
            for (u32 r = 0; r < DST_ROWS; ++r) {
                const u64 i = ei[r];
                if (i == ~0ull) continue;
                bool found = false;
                if (l[r] < cnt) {
                    Key<NW> x;
#pragma unroll
                    for (int w = 0; w < NW; ++w) x.w[w] = ls[l[r] * NW + w];
                    found = key_eq(x, d[r]);
                }
                if (found) {
                    edge_dst[i] = a + l[r];
                    if (FIRST) {
                        atomicMin((unsigned long long*)&lfirst[l[r]], (unsigned long long)(2 * sq[r] + 1));
                        const u32 bit = 1u << (l[r] & 31);
                        if (atomicOr(&lonce[l[r] >> 5], bit) & bit) atomicOr(&lmore[l[r] >> 5], bit);
                    }
                } else {
                    edge_dst[i] = ~0ull;
                    const u32 p = atomicAdd(&lmiss, 1u);
#pragma unroll
                    for (int w = 0; w < NW; ++w) lmk[p * NW + w] = d[r].w[w];
                    lme[p] = i;
                }
            }
            // room for another trip's misses?  Every wave must decide the same, so the count is read between two barriers: a
            // wave that ran ahead into the next trip could otherwise add to it before a slower one had looked (with the loads
            // prefetched that did happen: waves parted ways at flush()'s barriers and the grid never finished)
            __syncthreads();
            const u32 staged = lmiss;
            __syncthreads();
            if (staged + DST_ROWS * BLOCK > MISS_CAP) flush();
#pragma unroll
            for (u32 r = 0; r < DST_ROWS; ++r) { e[r] = en[r]; sq[r] = sqn[r]; ei[r] = ein[r]; }
        }
        flush();
        if (FIRST) {                                    // (flush ends with a barrier: the segment's minima are complete)
            for (u32 j = tid; j < cnt; j += BLOCK) node_first[a + j] = lfirst[j];      // the node's first touch, either role
            // (no barrier needed before the sweep below reads lfirst: flush ended with one, and nobody has written since)
            // second sweep: the edge that is the first to touch its target is marked (DST_FD: what the renumbering asks of every
            // edge, here without a look-up), and so is an edge whose target has no other in-edge (DST_IN1) -- with the matching
            // mark on the source side (one out-edge) the renumbering can tell the nodes nobody will ever look up (assign_nodes_kernel, first_seen.hip)
            for (u64 v = tid; v < total; v += BLOCK) {              // (the thread that wrote edge_dst[i])
                const u64 i = edge_of(v);
                const u64 d = edge_dst[i];
                if (d == ~0ull) continue;
                const u32 l = (u32)(d - a), bit = 1u << (l & 31);
                u64 marks = (lmore[l >> 5] & bit) ? 0 : DST_IN1;
                if (lfirst[l] == 2 * seq[i] + 1) marks |= DST_FD;
                if (marks) edge_dst[i] = d | marks;
            }
            __syncthreads();
        }
    }
}
// the targets that are no source (their ids were written by missing_rank_kernel): first touch of these nodes
__global__ __launch_bounds__(BLOCK) void missing_first_kernel(const u64* __restrict__ miss_edge, u64 n_miss, const u64* __restrict__ edge_dst,
                                                               const u64* __restrict__ seq, u64* node_first) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n_miss; i += (u64)gridDim.x * BLOCK) {
        const u64 e = miss_edge[i];
        atomicMin((unsigned long long*)&node_first[edge_dst[e]], (unsigned long long)(2 * seq[e] + 1));
    }
}

// the distinct source (k-1)-mers of sorted edges (the run heads of key >> 2), ascending, and every edge's position among them
// (`slack`: room kept behind them in node_key, in nodes, for the caller to append to)
// (head_counts: the run heads of every block of UNIQ_TILE edges, counted already by whoever wrote the edges -- group_merge_kernel --
// so that src_count_kernel need not read them; labels: the edges' labels (dev_labels' bytes) are written on the way, k their k)
template <int NW>
static int source_ids_t(const u64* d_edge_key, u64 E, DevBuf& node_key, u64* edge_src, u64* n_src_out, hipStream_t stream, bool with_slack = false,
                        DevBuf* seg_edge = nullptr, const u32* head_counts = nullptr, u32 k = 0, uint8_t* labels = nullptr) {
    *n_src_out = 0;
    if (E == 0) { KCHECK(node_key.alloc(16, stream)); return KATOME_OK; }
    const u64 nblocks = (E + UNIQ_TILE - 1) / UNIQ_TILE;
    if (nblocks > 0x7fffffffull) { set_error("node numbering: too many edges"); return KATOME_E_ARG; }
    if (labels && (uintptr_t)labels % 4) { set_error("label buffer must be 4-byte aligned"); return KATOME_E_ARG; }
    DevBuf counts(stream), offs(stream);
    if (!head_counts) KCHECK(counts.alloc(nblocks * 4));
    KCHECK(offs.alloc((nblocks + 1) * 8));
    {
        KernelScope ks(K_SRC_IDS, stream, E);
        if (!head_counts) hipLaunchKernelGGL(src_count_kernel<NW>, dim3((unsigned)nblocks), dim3(BLOCK), 0, stream, d_edge_key, E, counts.as<u32>());
        else if (getenv("KATOME_LC_TRACE")) fprintf(stderr, "[node ids] heads from the merge\n");
        KCHECK(dev_scan_counts(head_counts ? head_counts : counts.as<u32>(), nblocks, offs.as<u64>(), stream));      // (C3: 8e5 counts -- one workgroup walking them alone took 1.2 ms)
    }
    u64 n_src = 0;
    KCHECK_HIP(hipMemcpyAsync(&n_src, offs.as<u64>() + nblocks, 8, hipMemcpyDeviceToHost, stream));
    KCHECK_HIP(hipStreamSynchronize(stream));
    // (with_slack: the caller appends the nodes without out-edges -- usually a few percent -- instead of copying the lot)
    KCHECK(node_key.alloc((n_src + (with_slack ? n_src / 8 + (1u << 16) : 0) + 1) * 8 * NW, stream));
    if (seg_edge) KCHECK(seg_edge->alloc(((n_src + DST_SEG - 1) / DST_SEG + 1) * 8));        // first out-edge of every DST_SEG-th source
    {
        KernelScope ks(K_SRC_IDS, stream, E);
        if (labels) {
            if (getenv("KATOME_LC_TRACE")) fprintf(stderr, "[node ids] labels written with the source ids\n");
            const size_t lds = (size_t)UNIQ_TILE * label_stride_for_k(k);          // (18 KiB at k = 31, 34 KiB at k = 63)
            hipLaunchKernelGGL((src_write_kernel<NW, true>), dim3((unsigned)nblocks), dim3(BLOCK), lds, stream, d_edge_key, E, offs.as<u64>(), node_key.as<u64>(),
                               edge_src, seg_edge ? seg_edge->as<u64>() : nullptr, DST_SEG, k, labels);
        } else {
            hipLaunchKernelGGL((src_write_kernel<NW, false>), dim3((unsigned)nblocks), dim3(BLOCK), 0, stream, d_edge_key, E, offs.as<u64>(), node_key.as<u64>(), edge_src,
                               seg_edge ? seg_edge->as<u64>() : nullptr, DST_SEG, 0u, (uint8_t*)nullptr);
        }
    }
    KCHECK_HIP(hipGetLastError());
    *n_src_out = n_src;
    return KATOME_OK;
}
int dev_source_ids(const uint64_t* d_edge_key, uint64_t n_edges, uint32_t k, DevBuf& node_key, uint64_t* d_edge_src, uint64_t* n_src,
                   hipStream_t stream) {
    if (key_words_for_k(k) == 1) return source_ids_t<1>(d_edge_key, n_edges, node_key, d_edge_src, n_src, stream);
    return source_ids_t<2>(d_edge_key, n_edges, node_key, d_edge_src, n_src, stream);
}


// seq + node_first (first-seen order, both or neither): node_first[v] = the first touch of node v, 2*seq as a source, 2*seq + 1
// as a target; left empty when the merging look-up is switched off (dev_first_seen_order then fills it)
template <int NW>
static int node_ids_t(const u64* d_edge_key, u64 E, u32 k, DevBuf& node_key, u64* edge_src, u64* edge_dst, u64* n_nodes,
                      hipStream_t stream, const u64* seq = nullptr, DevBuf* node_first = nullptr, u64* n_marked = nullptr,
                      const u32* head_counts = nullptr, uint8_t* labels = nullptr) {
    *n_nodes = 0;
    if (n_marked) *n_marked = 0;
    if (node_first) node_first->release();
    if (E == 0) { KCHECK(node_key.alloc(16, stream)); return KATOME_OK; }
    const u32 node_bits = 2 * (k - 1);
    DevBuf aux(stream);
    KCHECK(aux.alloc(16));
    KCHECK_HIP(hipMemsetAsync(aux.p, 0, 16, stream));
    u64 n_src = 0;
    static const bool old_lookup = getenv("KATOME_DST_RANK") != nullptr;
    const bool first = seq && node_first && !old_lookup;
    DevBuf seg_edge(stream);
    KCHECK((source_ids_t<NW>(d_edge_key, E, node_key, edge_src, &n_src, stream, true, first ? &seg_edge : nullptr, head_counts, k, labels)));
    u64* nodes = node_key.as<u64>();
    // targets -> positions among the sources
    if (first && n_marked) *n_marked = n_src;            // (edge_dst carries the merge's marks for the targets that are sources)
    DevBuf miss_key(stream), miss_edge(stream);
    u64 miss_cap = 0, n_missing = 0;
    if (!old_lookup) {
        // merged against the sources segment by segment; the targets that are no source are set aside on the way
        const u64 n_seg = (n_src + DST_SEG - 1) / DST_SEG;
        DevBuf seg(stream);
        KCHECK(seg.alloc(4 * (n_seg + 1) * 8));
        miss_cap = E / 8 + (1u << 16);
        if (miss_key.alloc(miss_cap * 8 * NW + 16) != KATOME_OK || miss_edge.alloc(miss_cap * 8 + 16) != KATOME_OK) {
            miss_key.release(); miss_edge.release();
            miss_cap = 1u << 16;
            KCHECK(miss_key.alloc(miss_cap * 8 * NW + 16));
            KCHECK(miss_edge.alloc(miss_cap * 8 + 16));
        }
        hipLaunchKernelGGL(dst_seg_kernel<NW>, dim3(grid_for(4 * (n_seg + 1), BLOCK)), dim3(BLOCK), 0, stream, nodes, d_edge_key, E, node_bits, n_seg, seg.as<u64>());
        const size_t lds = (size_t)(DST_SEG * NW + MissCap<NW>::value * (NW + 1) + (first ? DST_SEG : 0)) * 8 + (first ? 2 * (DST_SEG / 32) * 4 : 0);
        const dim3 grid((unsigned)std::min<u64>(n_seg, 256u * 32u));
        KernelScope ks(K_DST_MERGE, stream, E);
        if (first) {
            // (room for the nodes without out-edges, like node_key's)
            // (the merge writes the first touch of every source; the room behind them, for the nodes without out-edges, starts at all-ones)
            KCHECK(node_first->alloc(node_key.bytes / NW));
            KCHECK_HIP(hipMemsetAsync(node_first->as<u64>() + n_src, 0xFF, node_first->bytes - n_src * 8, stream));
            hipLaunchKernelGGL((dst_merge_kernel<NW, true>), grid, dim3(BLOCK), lds, stream, nodes, n_src, d_edge_key, k, n_seg, seg.as<u64>(), edge_dst,
                               miss_key.as<u64>(), miss_edge.as<u64>(), miss_cap, aux.as<u64>(), seq, node_first->as<u64>(), edge_src, seg_edge.as<u64>(), E);
        } else {
            hipLaunchKernelGGL((dst_merge_kernel<NW, false>), grid, dim3(BLOCK), lds, stream, nodes, n_src, d_edge_key, k, n_seg, seg.as<u64>(), edge_dst,
                               miss_key.as<u64>(), miss_edge.as<u64>(), miss_cap, aux.as<u64>(), nullptr, nullptr, nullptr, nullptr, E);
        }
        KCHECK_HIP(hipGetLastError());
    } else {
        u32 B = 1;
        while ((2ull << B) <= n_src / 8 && B < 27) ++B;
        if (B > node_bits) B = node_bits;
        DevBuf index(stream);
        KCHECK(index.alloc(((1ull << B) + 2) * 8));
        KCHECK(dev_bucket_index(nodes, n_src, NW, node_bits, B, index.as<u64>(), stream));
        hipLaunchKernelGGL(dst_rank_kernel<NW>, dim3(grid_for(E, BLOCK, 256u * 32u)), dim3(BLOCK), 0, stream, nodes, n_src, node_bits, B,
                           index.as<u64>(), d_edge_key, E, k, edge_dst, aux.as<u64>());
        KCHECK_HIP(hipGetLastError());
    }
    KCHECK_HIP(hipMemcpyAsync(&n_missing, aux.p, 8, hipMemcpyDeviceToHost, stream));
    KCHECK_HIP(hipStreamSynchronize(stream));
    u64 n_extra = 0;
    if (n_missing) {
        DevBuf extra(stream);
        KCHECK(extra.alloc(n_missing * 8 * NW + 16));
        if (n_missing > miss_cap) {
            // (the old look-up, or more targets without out-edges than were given room: a second pass over edge_dst collects
            // them.  Setting them aside inside dst_rank_kernel was tried: 62 % of its waves hold one, and that many atomics
            // on one cursor cost more than this pass)
            miss_key.release(); miss_edge.release();
            KCHECK(miss_key.alloc(n_missing * 8 * NW + 16));
            KCHECK(miss_edge.alloc(n_missing * 8 + 16));
            hipLaunchKernelGGL(missing_gather_kernel<NW>, dim3(grid_for(E, BLOCK * UNIQ_ITEMS, 256u * 16u)), dim3(BLOCK), 0, stream, d_edge_key, E, k,
                               edge_dst, miss_key.as<u64>(), miss_edge.as<u64>(), aux.as<u64>() + 1);
            KCHECK_HIP(hipGetLastError());
        }
        KCHECK_HIP(hipMemcpyAsync(extra.p, miss_key.p, n_missing * 8 * NW, hipMemcpyDeviceToDevice, stream));
        KCHECK(dev_sort(extra.as<u64>(), nullptr, n_missing, NW, node_bits, stream));
        n_extra = n_missing;
        KCHECK(dev_unique(extra.as<u64>(), n_missing, NW, &n_extra, stream));
        hipLaunchKernelGGL(missing_rank_kernel<NW>, dim3(grid_for(n_missing, BLOCK)), dim3(BLOCK), 0, stream, miss_key.as<u64>(),
                           miss_edge.as<u64>(), n_missing, extra.as<u64>(), n_extra, n_src, edge_dst);
        KCHECK_HIP(hipGetLastError());
        if (first) {
            if ((n_src + n_extra + 1) * 8 > node_first->bytes) {
                DevBuf all(stream);
                KCHECK(all.alloc((n_src + n_extra + 1) * 8));
                KCHECK_HIP(hipMemcpyAsync(all.p, node_first->p, n_src * 8, hipMemcpyDeviceToDevice, stream));
                KCHECK_HIP(hipMemsetAsync(all.as<u64>() + n_src, 0xFF, (n_extra + 1) * 8, stream));
                const size_t bytes = all.bytes;
                node_first->adopt(all.take(), bytes);
            }
            hipLaunchKernelGGL(missing_first_kernel, dim3(grid_for(n_missing, BLOCK)), dim3(BLOCK), 0, stream, miss_edge.as<u64>(), n_missing, edge_dst, seq,
                               node_first->as<u64>());
            KCHECK_HIP(hipGetLastError());
        }
        // node_key = sources ++ extra
        if ((n_src + n_extra + 1) * 8 * NW <= node_key.bytes) {
            KCHECK_HIP(hipMemcpyAsync(nodes + n_src * NW, extra.p, n_extra * 8 * NW, hipMemcpyDeviceToDevice, stream));
        } else {
            DevBuf all(stream);
            KCHECK(all.alloc((n_src + n_extra + 1) * 8 * NW));
            KCHECK_HIP(hipMemcpyAsync(all.p, nodes, n_src * 8 * NW, hipMemcpyDeviceToDevice, stream));
            KCHECK_HIP(hipMemcpyAsync(all.as<u64>() + n_src * NW, extra.p, n_extra * 8 * NW, hipMemcpyDeviceToDevice, stream));
            const size_t bytes = all.bytes;
            node_key.adopt(all.take(), bytes);
        }
    }
    *n_nodes = n_src + n_extra;
    return KATOME_OK;
}

int dev_node_ids(const uint64_t* d_edge_key, uint64_t n_edges, uint32_t k, DevBuf& node_key, uint64_t* d_edge_src,
                 uint64_t* d_edge_dst, uint64_t* n_nodes, hipStream_t stream, const uint64_t* d_seq, DevBuf* node_first, uint64_t* n_marked,
                 const uint32_t* head_counts, uint8_t* d_label) {
    if (key_words_for_k(k) == 1) return node_ids_t<1>(d_edge_key, n_edges, k, node_key, d_edge_src, d_edge_dst, n_nodes, stream, d_seq, node_first, n_marked,
                                                      head_counts, d_label);
    return node_ids_t<2>(d_edge_key, n_edges, k, node_key, d_edge_src, d_edge_dst, n_nodes, stream, d_seq, node_first, n_marked, head_counts, d_label);
}

// ---- edge -> endpoints, labels ----------------------------------------------------------------
template <int NW>
__global__ __launch_bounds__(BLOCK) void endpoints_kernel(const u64* __restrict__ ek, u64 n, u32 k, u64* __restrict__ src, u64* __restrict__ dst) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK) {
        Key<NW> key = load_key<NW>(ek, i);
        if (src) store_key<NW>(src, i, source_node(key));
        if (dst) store_key<NW>(dst, i, target_node(key, k));
    }
}
int dev_endpoints(const uint64_t* d_edge_key, uint64_t n, uint32_t k, uint64_t* d_src, uint64_t* d_dst, hipStream_t stream) {
    if (n == 0) return KATOME_OK;
    dim3 grid(grid_for(n, BLOCK)), block(BLOCK);
    if (key_words_for_k(k) == 1) hipLaunchKernelGGL(endpoints_kernel<1>, grid, block, 0, stream, d_edge_key, n, k, d_src, d_dst);
    else                         hipLaunchKernelGGL(endpoints_kernel<2>, grid, block, 0, stream, d_edge_key, n, k, d_src, d_dst);
    KCHECK_HIP(hipGetLastError());
    return KATOME_OK;
}

// BFCounter input (create_bfc builder.rs:79-115 -> add_read_bfc pt_graph.rs:317-330 -> add_single_edge_bfc 201-213): every
// kept line is ONE edge -- and with reverse_complement a second one for its reverse complement, right after it -- added
// with `add_edge` unconditionally: a k-mer listed twice, or a k-mer that is its own reverse complement, stays as parallel
// edges.  So there is no table here: line i becomes edge i (2i and 2i+1 with both strands), whose sequence number is its
// petgraph index.
template <int NW>
__global__ __launch_bounds__(BLOCK) void bfc_edges_kernel(const u64* __restrict__ fwd, const u32* __restrict__ w, u64 n, u32 k, bool rc,
                                                           u64* __restrict__ ek, u32* __restrict__ ew, u64* __restrict__ seq) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK) {
        Key<NW> key = load_key<NW>(fwd, i);
        const u32 wi = w[i];
        if (rc) {
            store_key<NW>(ek, 2 * i, key); store_key<NW>(ek, 2 * i + 1, revcomp(key, k));
            ew[2 * i] = wi; ew[2 * i + 1] = wi;
            if (seq) { seq[2 * i] = 2 * i; seq[2 * i + 1] = 2 * i + 1; }
        } else {
            store_key<NW>(ek, i, key);
            ew[i] = wi;
            if (seq) seq[i] = i;
        }
    }
}
int dev_bfc_edges(const uint64_t* d_fwd, const uint32_t* d_w, uint64_t n, uint32_t k, bool rc, uint64_t* d_edge_key,
                  uint32_t* d_edge_weight, uint64_t* d_edge_seq, hipStream_t stream) {
    if (n == 0) return KATOME_OK;
    dim3 grid(grid_for(n, BLOCK)), block(BLOCK);
    if (key_words_for_k(k) == 1) hipLaunchKernelGGL(bfc_edges_kernel<1>, grid, block, 0, stream, d_fwd, d_w, n, k, rc, d_edge_key, d_edge_weight, d_edge_seq);
    else                         hipLaunchKernelGGL(bfc_edges_kernel<2>, grid, block, 0, stream, d_fwd, d_w, n, k, rc, d_edge_key, d_edge_weight, d_edge_seq);
    KCHECK_HIP(hipGetLastError());
    return KATOME_OK;
}

// compress_edge format: [pad][ceil(k/4) bytes].  A workgroup builds the labels of LABEL_ITEMS * 256 edges in LDS and streams
// them out as whole dwords (the byte stride is odd for most k); four keys per thread are loaded before the first is used (with
// 256 edges per trip a workgroup moved 4 KB and a CU had too few bytes in flight: 8.1 ms for C3's 27.6 GB).
constexpr u32 LABEL_ITEMS = 4;
template <int NW>
__global__ __launch_bounds__(BLOCK) void labels_kernel(const u64* __restrict__ ek, u64 n, u32 k, uint8_t* __restrict__ out) {
    extern __shared__ u32 lbuf[];
    uint8_t* lb = reinterpret_cast<uint8_t*>(lbuf);
    const u32 stride = label_stride_for_k(k), nb = stride - 1, pad = label_pad_for_k(k);
    constexpr u32 TILE = BLOCK * LABEL_ITEMS;
    const u64 ntiles = (n + TILE - 1) / TILE;
    for (u64 t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const u64 e0 = t * TILE;
        const u32 cnt = (u32)((n - e0) < (u64)TILE ? (n - e0) : (u64)TILE);
        Key<NW> key[LABEL_ITEMS];
#pragma unroll
        for (u32 r = 0; r < LABEL_ITEMS; ++r) { const u32 j = r * BLOCK + threadIdx.x; if (j < cnt) key[r] = load_key<NW>(ek, e0 + j); }
#pragma unroll
        for (u32 r = 0; r < LABEL_ITEMS; ++r) {
            const u32 j = r * BLOCK + threadIdx.x;
            if (j < cnt) {
                uint8_t* p = lb + j * stride;
                p[0] = (uint8_t)pad;
                for (u32 i = 0; i < nb; ++i) p[1 + i] = label_byte(key[r], k, i);
            }
        }
        __syncthreads();
        const u64 byte0 = e0 * stride;                 // TILE*stride is a multiple of 4 -> dword aligned
        const u32 nbytes = cnt * stride;
        u32* o32 = reinterpret_cast<u32*>(out + byte0);
        for (u32 i = threadIdx.x; i < nbytes / 4; i += BLOCK) o32[i] = lbuf[i];
        for (u32 i = (nbytes / 4) * 4 + threadIdx.x; i < nbytes; i += BLOCK) out[byte0 + i] = lb[i];
        __syncthreads();
    }
}
int dev_labels(const uint64_t* d_edge_key, uint64_t n, uint32_t k, uint8_t* d_label, hipStream_t stream) {
    if (n == 0) return KATOME_OK;
    const size_t lds = (size_t)BLOCK * LABEL_ITEMS * label_stride_for_k(k) + 16;
    dim3 grid(grid_for(n, BLOCK * LABEL_ITEMS, 256u * 16u)), block(BLOCK);
    if ((uintptr_t)d_label % 4) { set_error("label buffer must be 4-byte aligned"); return KATOME_E_ARG; }
    if (key_words_for_k(k) == 1) hipLaunchKernelGGL(labels_kernel<1>, grid, block, lds, stream, d_edge_key, n, k, d_label);
    else                         hipLaunchKernelGGL(labels_kernel<2>, grid, block, lds, stream, d_edge_key, n, k, d_label);
    KCHECK_HIP(hipGetLastError());
    return KATOME_OK;
}

}  // namespace katome
