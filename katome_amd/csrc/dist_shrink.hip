// dist_shrink.hip -- the traversal-free Shrinkable::shrink (shrink.hip's fast form) on the SHARDED graph,
// no gather, in either numbering:
//   * a vertex is INNER when in-degree = out-degree = 1 and its edges are not one self-loop; an edge whose source is not inner
//     is a HEAD and starts one merged edge; a cycle of inner vertices becomes a self-loop at its smallest global node id.
//   * degrees and links (dist_links.h, shared with dist_contigs.hip): every edge sends one record to the owner of its target
//     (first-seen order: edge_drank / edge_dlocal; by packed key: the allgathered node_base ranges).  The owner counts
//     in-degrees, remembers the address (rank << 56 | local index) of the edge that comes in and answers whether the target is
//     inner.  Every edge then knows its PREDECESSOR -- the in-edge of its source, if the source is inner -- from its own
//     rank's tables.
//   * list ranking by pointer jumping (Wyllie): one state pair per edge, A = RESOLVED | head address or the address of the
//     edge 2^round steps back, B = offset from the head or the smallest source id over the jumped span.  A round is one
//     question (the pointer) and two answers (that edge's A and B) through the Router; every unresolved edge's span is 2^round
//     edges, so it is implicit.  The rounds stop when everything is resolved, or when a round resolved nothing (what is left
//     lies on cycles of inner vertices) and 2^round covers every unresolved edge (each then knows its cycle's smallest vertex).
//     The edge leaving that vertex becomes the cycle's head and a second, shorter ranking gives the cycle edges their offsets.
//   * merged edges live on the rank of their head: the last edge of each path sends its end node there, every other edge
//     (offset, last base of its key); the bases land at fixed places of a one-byte-per-base staging array (offsets are dense
//     per path: no sort, no atomics) that a pack kernel turns into compress_edge labels.
//   * coverage (katome_dist_shrink_coverage only): every non-head edge also sends (head, offset << 32 | its weight) over the same
//     routing; the weights land where the bases do, in a 4-byte staging array, and one wave per merged edge reduces them with the
//     head's own weight to their sum, smallest and largest.  No atomics here either.
//   * node numbering: a surviving vertex's new id is the number of surviving vertices with a smaller global id, counted per
//     directory range (id / ceil(TN / world)), one question and answer per endpoint of a merged edge and per node of the share.
// Memory per rank is O(share) (plus the staging of the paths whose heads it holds).  A rank's share stays below 2^32 edges
// and nodes, node ids below 2^40, a path below 2^32 k-mers; every failure is agreed by an allreduce.
#include <cstdio>
#include <cstdlib>

#include "dist_links.h"

namespace {

constexpr u64 RESOLVED = 1ull << 55;                  // state word A: the head's address follows (bits 56.. rank, 0..31 index)
constexpr u64 ADDR = (0xFFull << 56) | 0xFFFFFFFFull;
constexpr u64 ID_LIMIT = 1ull << 40;

// the ranking's start: heads are resolved at offset 0, every other edge points at its predecessor (span 1, its source id)
__global__ __launch_bounds__(BLOCK) void init_kernel(u64 E, const u32* __restrict__ lsrc, const u64* __restrict__ src, const unsigned char* __restrict__ inner,
                                                     const u64* __restrict__ in_edge, const u64* __restrict__ dst_inner, u64 me, u64* __restrict__ pred,
                                                     u64* __restrict__ st_a, u64* __restrict__ st_b, unsigned char* __restrict__ last) {
    WLOOP(e, E) if (e < E) {
        const u32 l = lsrc[e];
        if (inner[l]) { pred[e] = in_edge[l]; st_a[e] = in_edge[l]; st_b[e] = src[e]; }
        else { pred[e] = NONE64; st_a[e] = RESOLVED | (me << 56) | e; st_b[e] = 0; }
        last[e] = dst_inner[e] == 0;
    }
}
// the unresolved edges: their pointer (the question) and themselves
__global__ __launch_bounds__(BLOCK) void active_kernel(const u64* __restrict__ st_a, u64 E, u64* __restrict__ q, u32* __restrict__ who, unsigned long long* cursor) {
    TLOOP(t0, E) {
        u32 mine = 0, have = 0;
#pragma unroll
        for (int k = 0; k < CA_ITEMS; ++k) {
            const u64 e = t0 + (u64)k * BLOCK + threadIdx.x;
            if (e < E && !(st_a[e] & RESOLVED)) { have |= 1u << k; ++mine; }
        }
        u64 at = block_append(mine, cursor);
#pragma unroll
        for (int k = 0; k < CA_ITEMS; ++k) if (have & (1u << k)) { const u64 e = t0 + (u64)k * BLOCK + threadIdx.x; q[at] = st_a[e] & ADDR; who[at] = (u32)e; ++at; }
    }
}
// the asked edge's state as it stood at the start of the round (the answers are the second buffer)
__global__ __launch_bounds__(BLOCK) void answer_state_kernel(const u64* __restrict__ A, u64 n, u64 E, const u64* __restrict__ st_a, const u64* __restrict__ st_b,
                                                             u64* __restrict__ ans_a, u64* __restrict__ ans_b) {
    WLOOP(i, n) if (i < n) {
        const u32 l = local_of(A[i]);
        ans_a[i] = l < E ? st_a[l] : A[i];          // (a pointer at no edge stays where it is: the rounds run out and report it)
        ans_b[i] = l < E ? st_b[l] : NONE64;
    }
}
// span = 2^round: resolved through the pointer at offset span + its offset, or the pointer doubles and the minimum follows
__global__ __launch_bounds__(BLOCK) void apply_kernel(const u32* __restrict__ who, u64 n, const u64* __restrict__ ans_a, const u64* __restrict__ ans_b, u64 span,
                                                      u64* __restrict__ st_a, u64* __restrict__ st_b) {
    WLOOP(i, n) if (i < n) {
        const u32 e = who[i];
        const u64 a = ans_a[i], b = ans_b[i];
        st_a[e] = a;
        st_b[e] = (a & RESOLVED) ? span + b : (b < st_b[e] ? b : st_b[e]);
    }
}
// what the first ranking left lies on cycles of inner vertices, each edge with its cycle's smallest vertex: the edge leaving
// it becomes the head, the edge entering it the last edge, the others point at their predecessors again
__global__ __launch_bounds__(BLOCK) void cycle_kernel(u64 E, const u64* __restrict__ src, const u64* __restrict__ dst, const u64* __restrict__ pred, u64 me,
                                                      u64* __restrict__ st_a, u64* __restrict__ st_b, unsigned char* __restrict__ last, unsigned long long* n_heads) {
    WLOOP(e, E) if (e < E && !(st_a[e] & RESOLVED)) {
        const u64 mn = st_b[e];
        if (dst[e] == mn) last[e] = 1;
        if (src[e] == mn) { st_a[e] = RESOLVED | (me << 56) | e; st_b[e] = 0; atomicAdd(n_heads, 1ull); }
        else { st_a[e] = pred[e]; st_b[e] = 0; }
    }
}
__global__ __launch_bounds__(BLOCK) void max_kernel(const u64* __restrict__ v, u64 n, unsigned long long* out) {
    u64 m = 0;
    WLOOP(i, n) if (i < n && v[i] > m) m = v[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const u64 t = __shfl_xor(m, o, 64); if (t > m) m = t; }
    if ((threadIdx.x & 63) == 0 && m) atomicMax(out, (unsigned long long)m);
}
__global__ __launch_bounds__(BLOCK) void is_head_kernel(const u64* __restrict__ st_a, u64 E, u64 me, unsigned char* __restrict__ head) {
    WLOOP(e, E) if (e < E) head[e] = st_a[e] == (RESOLVED | (me << 56) | e);
}
__global__ __launch_bounds__(BLOCK) void slot_kernel(const u32* __restrict__ heads, u64 H, u32* __restrict__ slot, u32* __restrict__ m) {
    WLOOP(i, H) if (i < H) { slot[heads[i]] = (u32)i; m[i] = 1; }
}
// last edges -> (head, end node); every other non-head edge -> (head, offset << 2 | the last base of its key)
// COV (katome_dist_shrink_coverage): and, for the same head address, (offset << 32 | the edge's weight) -- offsets stay below 2^32
template <int NW, bool COV>
__global__ __launch_bounds__(BLOCK) void path_rec_kernel(const u64* __restrict__ st_a, const u64* __restrict__ st_b, const u64* __restrict__ dst,
                                                         const u64* __restrict__ key, const unsigned char* __restrict__ last, u64 E, u64 me,
                                                         u64* __restrict__ endA, u64* __restrict__ endB, u64* __restrict__ baseA, u64* __restrict__ baseB,
                                                         unsigned long long* cursors, const u32* __restrict__ weight, u64* __restrict__ baseW) {
    WLOOP(e, E) {
        const bool ok = e < E;
        const u64 a = ok ? st_a[e] : 0;
        const bool head = ok && a == (RESOLVED | (me << 56) | e);
        const bool is_last = ok && last[e], is_base = ok && !head;
        const u64 at_end = wave_append(is_last, cursors), at_base = wave_append(is_base, cursors + 1);
        if (is_last) { endA[at_end] = a & ADDR; endB[at_end] = dst[e]; }
        if (is_base) {
            baseA[at_base] = a & ADDR; baseB[at_base] = (st_b[e] << 2) | (key[e * NW + NW - 1] & 3);
            if constexpr (COV) baseW[at_base] = (st_b[e] << 32) | weight[e];
        }
    }
}
// (records name head edges of this rank: slot < H; the checks only keep a broken invariant from writing out of bounds)
__global__ __launch_bounds__(BLOCK) void end_place_kernel(const u64* __restrict__ A, const u64* __restrict__ B, u64 n, const u32* __restrict__ slot, u64 E,
                                                          u64 H, u64* __restrict__ end_node, unsigned long long* n_bad) {
    WLOOP(i, n) if (i < n) {
        const u32 l = local_of(A[i]), s = l < E ? slot[l] : NONE32;
        if (s < H) end_node[s] = B[i]; else atomicAdd(n_bad, 1ull);
    }
}
__global__ __launch_bounds__(BLOCK) void base_len_kernel(const u64* __restrict__ A, const u64* __restrict__ B, u64 n, const u32* __restrict__ slot, u64 E, u64 H,
                                                         u32* __restrict__ m, unsigned long long* n_bad) {
    WLOOP(i, n) if (i < n) {
        const u32 l = local_of(A[i]), s = l < E ? slot[l] : NONE32;
        if (s < H && (B[i] >> 2) >= 1 && (B[i] >> 2) < 0xFFFFFFFFull) atomicMax(&m[s], (u32)(B[i] >> 2) + 1u); else atomicAdd(n_bad, 1ull);
    }
}
__global__ __launch_bounds__(BLOCK) void measure_kernel(const u32* __restrict__ m, u64 H, u32 k, u32* __restrict__ label_bytes, u32* __restrict__ staged) {
    WLOOP(i, H) if (i < H) { label_bytes[i] = 1 + (k + m[i] - 1 + 3) / 4; staged[i] = m[i] - 1; }
}
__global__ __launch_bounds__(BLOCK) void base_place_kernel(const u64* __restrict__ A, const u64* __restrict__ B, u64 n, const u32* __restrict__ slot, u64 E,
                                                           u64 H, const u32* __restrict__ m, const u64* __restrict__ stage_off, unsigned char* __restrict__ stage) {
    WLOOP(i, n) if (i < n) {
        const u32 l = local_of(A[i]), s = l < E ? slot[l] : NONE32;
        const u64 off = B[i] >> 2;
        if (s < H && off >= 1 && off < m[s]) stage[stage_off[s] + off - 1] = (unsigned char)(B[i] & 3);
    }
}
// coverage: every non-head edge's weight at the place its base has in the byte staging -- stage_off[s] + offset - 1, dense and
// collision-free per path -- of a 4-byte staging array
__global__ __launch_bounds__(BLOCK) void weight_place_kernel(const u64* __restrict__ A, const u64* __restrict__ W, u64 n, const u32* __restrict__ slot, u64 E,
                                                             u64 H, const u32* __restrict__ m, const u64* __restrict__ stage_off, u32* __restrict__ wstage) {
    WLOOP(i, n) if (i < n) {
        const u32 l = local_of(A[i]), s = l < E ? slot[l] : NONE32;
        const u64 off = W[i] >> 32;
        if (s < H && off >= 1 && off < m[s]) wstage[stage_off[s] + off - 1] = (u32)W[i];
    }
}
// one wave per merged edge (as pack_kernel): the head's own weight and the staged ones, reduced to their sum, smallest and largest
__global__ __launch_bounds__(BLOCK) void weight_reduce_kernel(const u32* __restrict__ heads, u64 H, const u32* __restrict__ weight, const u32* __restrict__ m,
                                                              const u64* __restrict__ stage_off, const u32* __restrict__ wstage, u64* __restrict__ o_sum,
                                                              u32* __restrict__ o_min, u32* __restrict__ o_max) {
    const u32 lane = threadIdx.x & 63;
    for (u64 i = ((u64)blockIdx.x * BLOCK + threadIdx.x) >> 6; i < H; i += ((u64)gridDim.x * BLOCK) >> 6) {
        const u32 hw = weight[heads[i]], staged = m[i] - 1;
        const u32* st = wstage + stage_off[i];
        u64 sum = lane == 0 ? hw : 0;
        u32 mn = hw, mx = hw;
        for (u32 j = lane; j < staged; j += 64) { const u32 w = st[j]; sum += w; mn = min(mn, w); mx = max(mx, w); }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            sum += __shfl_xor(sum, o, 64);
            mn = min(mn, (u32)__shfl_xor(mn, o, 64)); mx = max(mx, (u32)__shfl_xor(mx, o, 64));
        }
        if (lane == 0) { o_sum[i] = sum; o_min[i] = mn; o_max[i] = mx; }
    }
}
// one wave per merged edge: compress_edge's padding byte, then 4 bases a byte (the head's k, then the staged ones), left-aligned
template <int NW>
__global__ __launch_bounds__(BLOCK) void pack_kernel(const u32* __restrict__ heads, u64 H, const u64* __restrict__ key, const u32* __restrict__ m,
                                                     const u64* __restrict__ label_off, const u64* __restrict__ stage_off,
                                                     const unsigned char* __restrict__ stage, u32 k, unsigned char* __restrict__ label) {
    const u32 lane = threadIdx.x & 63;
    for (u64 i = ((u64)blockIdx.x * BLOCK + threadIdx.x) >> 6; i < H; i += ((u64)gridDim.x * BLOCK) >> 6) {
        const u32 len = k + m[i] - 1, nbytes = (len + 3) / 4;
        unsigned char* out = label + label_off[i];
        const unsigned char* st = stage + stage_off[i];
        Key<NW> hk;
#pragma unroll
        for (int q = 0; q < NW; ++q) hk.w[q] = key[(u64)heads[i] * NW + q];
        if (lane == 0) out[0] = (unsigned char)((4 - len % 4) % 4);
        for (u32 j = lane; j < nbytes; j += 64) {
            u32 byte = 0;
#pragma unroll
            for (u32 q = 0; q < 4; ++q) {
                const u32 p = 4 * j + q;
                const u32 b = p >= len ? 0u : p < k ? key_digit(hk, 2 * (k - 1 - p), 2) : (u32)st[p - k];
                byte = (byte << 2) | b;
            }
            out[1 + j] = (unsigned char)byte;
        }
    }
}
// the directory rank of a node id: (id / per_rank) << 56 | id
__global__ __launch_bounds__(BLOCK) void head_ends_kernel(const u32* __restrict__ heads, u64 H, const u64* __restrict__ src, const u64* __restrict__ end_node,
                                                          u64 per_rank, u64* __restrict__ qs, u64* __restrict__ qd) {
    WLOOP(i, H) if (i < H) {
        const u64 s = src[heads[i]], t = end_node[i];
        qs[i] = ((s / per_rank) << 56) | s; qd[i] = ((t / per_rank) << 56) | t;
    }
}
__global__ __launch_bounds__(BLOCK) void node_q_kernel(const u64* __restrict__ gid, u64 N, u64 node_base, u64 per_rank, u64* __restrict__ q) {
    WLOOP(j, N) if (j < N) { const u64 g = gid ? gid[j] : node_base + j; q[j] = ((g / per_rank) << 56) | g; }
}
__global__ __launch_bounds__(BLOCK) void touch_kernel(const u64* __restrict__ A, u64 n, u64 base, u64 range, u32* __restrict__ touched) {
    WLOOP(i, n) if (i < n) { const u64 l = (A[i] & LOW56) - base; if (l < range) touched[l] = 1u; }
}
// new id = surviving ids below this range (every rank's counts) + those below the id within it; NONE64 for a vertex that goes
__global__ __launch_bounds__(BLOCK) void new_id_kernel(const u64* __restrict__ A, u64 n, u64 base, const u32* __restrict__ touched, const u64* __restrict__ offs,
                                                       u64 range, u64 below, u64* __restrict__ out) {
    WLOOP(i, n) if (i < n) { const u64 l = (A[i] & LOW56) - base; out[i] = l < range && touched[l] ? below + offs[l] : NONE64; }
}
__global__ __launch_bounds__(BLOCK) void kept_kernel(const u64* __restrict__ nid, u64 N, unsigned char* __restrict__ keep) {
    WLOOP(j, N) if (j < N) keep[j] = nid[j] != NONE64;
}
__global__ __launch_bounds__(BLOCK) void head_out_kernel(const u32* __restrict__ heads, u64 H, const u32* __restrict__ weight, const u64* __restrict__ gid,
                                                         u64 edge_base, u32* __restrict__ o_weight, u64* __restrict__ o_head) {
    WLOOP(i, H) if (i < H) { const u32 h = heads[i]; o_weight[i] = weight[h]; o_head[i] = gid ? gid[h] : edge_base + h; }
}

// KATOME_DIST_SHRINK_FAIL=<rank> (tests): that rank reports a failure after the first ranking round
int fail_rank() {
    const char* at = getenv("KATOME_DIST_SHRINK_FAIL");
    return at && *at ? atoi(at) : -1;
}

struct Shrink {
    katome_dist_builder* d; hipStream_t stream; int rank, world; uint64_t E, N;
    Router router; DevBuf cursors;
    Shrink(katome_dist_builder* d_, hipStream_t s) : d(d_), stream(s), rank(d_->rank()), world(d_->world()), E(d_->n_edges), N(d_->n_nodes),
        router(d_, s), cursors(s) {}
    unsigned long long* cur() { return cursors.as<unsigned long long>(); }
    int reset() { KCHECK_HIP(hipMemsetAsync(cursors.p, 0, 64, stream)); return KATOME_OK; }
    int read(uint64_t* h, int n) {
        KCHECK_HIP(hipMemcpyAsync(h, cursors.p, 8 * n, hipMemcpyDeviceToHost, stream));
        KCHECK_HIP(hipStreamSynchronize(stream));
        return KATOME_OK;
    }
    // the set bytes' indices, ascending
    int keep_list(const unsigned char* flag, uint64_t n, DevBuf& keep, uint64_t* n_keep) {
        KCHECK(keep.alloc((n + 1) * 4));
        KCHECK(reset());
        if (n) KLAUNCH_T(alive_list_kernel, n, stream, flag, n, keep.as<u32>(), cur());
        KCHECK_HIP(hipGetLastError());
        KCHECK(read(n_keep, 1));
        if (*n_keep > 1) {                                   // (workgroups append in no particular order)
            DevBuf k64(stream);
            KCHECK(k64.alloc((*n_keep + 1) * 8));
            KLAUNCH(widen_kernel, *n_keep, stream, keep.as<u32>(), *n_keep, k64.as<u64>());
            KCHECK(dev_sort(k64.as<u64>(), nullptr, *n_keep, 1, 32, stream));
            KLAUNCH(narrow_kernel, *n_keep, stream, k64.as<u64>(), *n_keep, keep.as<u32>());
            KCHECK_HIP(hipGetLastError());
        }
        return KATOME_OK;
    }
    // Wyllie's rounds until everything is resolved or only cycles of inner vertices are left (see the top of the file);
    // `knob`: the first ranking, where KATOME_DIST_SHRINK_FAIL may strike after round 1.  *left: unresolved edges of all ranks
    int rank_lists(u64* st_a, u64* st_b, bool knob, uint32_t* rounds, uint64_t* left) {
        const int fail_at = knob ? fail_rank() : -1;
        DevBuf q(stream), who(stream), ans_a(stream), ans_b(stream), got_a(stream), got_b(stream);
        KCHECK(q.alloc((E + 1) * 8)); KCHECK(who.alloc((E + 1) * 4)); KCHECK(got_a.alloc((E + 1) * 8)); KCHECK(got_b.alloc((E + 1) * 8));
        uint64_t prev = ~0ull, U = 0;
        uint32_t t = 0;
        for (;; ++t) {
            KCHECK(reset());
            if (E) KLAUNCH_T(active_kernel, E, stream, st_a, E, q.as<u64>(), who.as<u32>(), cur());
            KCHECK_HIP(hipGetLastError());
            uint64_t n_act = 0;
            KCHECK(read(&n_act, 1));
            const bool check_knob = fail_at >= 0 && t == 1;
            uint64_t agg[2] = {n_act, check_knob && fail_at == rank ? 1ull + (uint64_t)rank : 0};
            KCHECK(d->comm->allreduce(agg, 2, OP_SUM));
            if (agg[1]) {
                const int who_failed = (int)agg[1] - 1;
                if (who_failed == rank) set_error("katome_dist_shrink: KATOME_DIST_SHRINK_FAIL=%d: rank %d fails after ranking round 1", fail_at, rank);
                else set_error("katome_dist_shrink: rank %d failed after ranking round 1", who_failed);
                return KATOME_E_UNSUPPORTED;
            }
            U = agg[0];
            const bool stop = U == 0 || (t >= 1 && U == prev && (t >= 63 || (1ull << t) >= U));
            // (the knob strikes after round 1 even when the ranking needs fewer rounds)
            if (stop && !(fail_at >= 0 && t < 1)) break;
            if (t >= 64) { set_error("katome_dist_shrink: the ranking did not converge"); return KATOME_E_DEVICE; }
            prev = U;
            Routed asked(stream);
            KCHECK(router.send(q.as<u64>(), nullptr, n_act, asked));
            KCHECK(ans_a.alloc((asked.n + 1) * 8)); KCHECK(ans_b.alloc((asked.n + 1) * 8));
            if (asked.n) KLAUNCH(answer_state_kernel, asked.n, stream, asked.a.as<u64>(), asked.n, E, st_a, st_b, ans_a.as<u64>(), ans_b.as<u64>());
            KCHECK_HIP(hipGetLastError());
            KCHECK(router.reply(asked, ans_a.as<u64>(), got_a.as<u64>()));
            KCHECK(router.reply(asked, ans_b.as<u64>(), got_b.as<u64>()));
            if (n_act) KLAUNCH(apply_kernel, n_act, stream, who.as<u32>(), n_act, got_a.as<u64>(), got_b.as<u64>(), t >= 63 ? (1ull << 63) : (1ull << t),
                               st_a, st_b);
            KCHECK_HIP(hipGetLastError());
        }
        *rounds = t; *left = U;
        return KATOME_OK;
    }
};

int check_shrink_builder(katome_dist_builder* d) {
    if (!d) { set_error("null argument"); return KATOME_E_ARG; }
    if (!d->finalized) { set_error("katome_dist_shrink: call katome_dist_finalize first"); return KATOME_E_ARG; }
    if (d->gathered) { set_error("katome_dist_shrink: the ranks' shares were gathered (katome_dist_gather); shrink the gathered graph on its root"); return KATOME_E_ARG; }
    return KATOME_OK;
}

// (want_cov: every rank's merged edges also get the sum, smallest and largest weight along their paths: d->sh_cov)
int dist_shrink(katome_dist_builder* d, katome_dist_shrink_stats* stats, hipStream_t stream, bool want_cov) {
    Shrink S(d, stream);
    KCHECK(S.cursors.alloc(64)); KCHECK(S.router.init());
    katome_builder* b = d->b;
    const uint64_t E = S.E, N = S.N, me = (uint64_t)S.rank;
    const int world = S.world;
    const uint32_t k = d->s.k, nw = d->nw;
    const uint64_t bytes0 = d->comm->stats.bytes_out;
    {
        uint64_t bad = (E >= 0xFFFFFFFFull || N >= 0xFFFFFFFFull || d->total_nodes >= ID_LIMIT) ? 1 : 0;
        KCHECK(d->comm->allreduce(&bad, 1, OP_MAX));
        if (bad) { set_error("katome_dist_shrink: more than 2^32 edges or nodes on one rank, or more than 2^40 nodes"); return KATOME_E_UNSUPPORTED; }
    }
    // ---- degrees and links (dist_links.h) --------------------------------------------------------------------------------
    Links links(stream);
    KCHECK(dist_links(d, S.router, stream, links));
    const uint64_t edge_base = links.edge_base;
    const u64* src = d->edge_src.as<u64>(); const u64* dst = d->edge_dst.as<u64>();
    DevBuf pred(stream), st_a(stream), st_b(stream), last(stream);
    KCHECK(pred.alloc((E + 1) * 8)); KCHECK(st_a.alloc((E + 1) * 8)); KCHECK(st_b.alloc((E + 1) * 8)); KCHECK(last.alloc(E + 16));
    if (E) KLAUNCH(init_kernel, E, stream, E, links.lsrc.as<u32>(), src, links.inner.as<unsigned char>(), links.in_edge.as<u64>(), links.dst_inner.as<u64>(), me,
                   pred.as<u64>(), st_a.as<u64>(), st_b.as<u64>(), last.as<unsigned char>());
    KCHECK_HIP(hipGetLastError());
    links.release();
    // ---- list ranking; then the cycles of inner vertices ------------------------------------------------------------------
    uint32_t rounds = 0, cycle_rounds = 0;
    uint64_t left = 0, n_cycles = 0;
    KCHECK(S.rank_lists(st_a.as<u64>(), st_b.as<u64>(), true, &rounds, &left));
    if (left) {
        KCHECK(S.reset());
        if (E) KLAUNCH(cycle_kernel, E, stream, E, src, dst, pred.as<u64>(), me, st_a.as<u64>(), st_b.as<u64>(), last.as<unsigned char>(), S.cur());
        KCHECK_HIP(hipGetLastError());
        KCHECK(S.read(&n_cycles, 1));
        KCHECK(d->comm->allreduce(&n_cycles, 1, OP_SUM));
        uint64_t left2 = 0;
        KCHECK(S.rank_lists(st_a.as<u64>(), st_b.as<u64>(), false, &cycle_rounds, &left2));
        if (left2 || n_cycles == 0) { set_error("katome_dist_shrink: %llu edges on no path and no cycle", (unsigned long long)(left2 ? left2 : left)); return KATOME_E_DEVICE; }
    }
    pred.release();
    uint64_t longest = 0;
    KCHECK(S.reset());
    if (E) KLAUNCH(max_kernel, E, stream, st_b.as<u64>(), E, S.cur());
    KCHECK_HIP(hipGetLastError());
    KCHECK(S.read(&longest, 1));
    KCHECK(d->comm->allreduce(&longest, 1, OP_MAX));
    if (longest + 1 >= 0xFFFFFFFFull) { set_error("katome_dist_shrink: a path of 2^32 k-mers or more (edge_kmers is 32 bits)"); return KATOME_E_UNSUPPORTED; }
    longest += d->total_edges ? 1 : 0;
    // ---- merged edges on the ranks of their heads ------------------------------------------------------------------------
    DevBuf is_head(stream), heads(stream), slot(stream), m(stream);
    uint64_t H = 0;
    KCHECK(is_head.alloc(E + 16));
    if (E) KLAUNCH(is_head_kernel, E, stream, st_a.as<u64>(), E, me, is_head.as<unsigned char>());
    KCHECK_HIP(hipGetLastError());
    KCHECK(S.keep_list(is_head.as<unsigned char>(), E, heads, &H));
    is_head.release();
    KCHECK(slot.alloc((E + 1) * 4)); KCHECK(m.alloc((H + 1) * 4));
    KCHECK_HIP(hipMemsetAsync(slot.p, 0xFF, (E + 1) * 4, stream));
    if (H) KLAUNCH(slot_kernel, H, stream, heads.as<u32>(), H, slot.as<u32>(), m.as<u32>());
    DevBuf endA(stream), endB(stream), baseA(stream), baseB(stream), baseW(stream), end_node(stream);
    KCHECK(endA.alloc((E + 1) * 8)); KCHECK(endB.alloc((E + 1) * 8)); KCHECK(baseA.alloc((E + 1) * 8)); KCHECK(baseB.alloc((E + 1) * 8));
    if (want_cov) KCHECK(baseW.alloc((E + 1) * 8));
    KCHECK(end_node.alloc((H + 1) * 8));
    KCHECK(S.reset());
    if (E) {
        auto rec_kernel = nw == 1 ? (want_cov ? path_rec_kernel<1, true> : path_rec_kernel<1, false>) : (want_cov ? path_rec_kernel<2, true> : path_rec_kernel<2, false>);
        KLAUNCH(rec_kernel, E, stream, st_a.as<u64>(), st_b.as<u64>(), dst, b->edge_key.as<u64>(), last.as<unsigned char>(), E, me, endA.as<u64>(), endB.as<u64>(),
                baseA.as<u64>(), baseB.as<u64>(), S.cur(), b->edge_weight.as<u32>(), baseW.as<u64>());
    }
    KCHECK_HIP(hipGetLastError());
    uint64_t nrec[2] = {0, 0};
    KCHECK(S.read(nrec, 2));
    st_a.release(); st_b.release(); last.release();
    DevBuf label_off(stream), stage_off(stream), label(stream);
    uint64_t label_bytes = 0;
    {
        Routed ends(stream), bases_r(stream), weights_r(stream);
        KCHECK(S.router.send(endA.as<u64>(), endB.as<u64>(), nrec[0], ends));
        endA.release(); endB.release();
        KCHECK(S.router.send(baseA.as<u64>(), baseB.as<u64>(), nrec[1], bases_r));
        if (want_cov) KCHECK(S.router.send(baseA.as<u64>(), baseW.as<u64>(), nrec[1], weights_r));       // (the same routing: the same A array)
        baseA.release(); baseB.release(); baseW.release();
        KCHECK(S.reset());
        if (ends.n) KLAUNCH(end_place_kernel, ends.n, stream, ends.a.as<u64>(), ends.b.as<u64>(), ends.n, slot.as<u32>(), E, H, end_node.as<u64>(), S.cur() + 7);
        if (bases_r.n) KLAUNCH(base_len_kernel, bases_r.n, stream, bases_r.a.as<u64>(), bases_r.b.as<u64>(), bases_r.n, slot.as<u32>(), E, H, m.as<u32>(), S.cur() + 7);
        KCHECK_HIP(hipGetLastError());
        uint64_t h8[8] = {0};
        KCHECK(S.read(h8, 8));
        uint64_t bad = (ends.n != H || h8[7]) ? 1 : 0;
        KCHECK(d->comm->allreduce(&bad, 1, OP_MAX));
        if (bad) { set_error("katome_dist_shrink: a merged edge has no last edge, or two, or a record names no head"); return KATOME_E_DEVICE; }
        // the labels' sizes, one scan each for the label bytes and the staged bases
        DevBuf lb(stream), staged(stream), stage(stream);
        KCHECK(lb.alloc((H + 1) * 4)); KCHECK(staged.alloc((H + 1) * 4)); KCHECK(label_off.alloc((H + 2) * 8)); KCHECK(stage_off.alloc((H + 2) * 8));
        uint64_t n_staged = 0;
        if (H) {
            KLAUNCH(measure_kernel, H, stream, m.as<u32>(), H, k, lb.as<u32>(), staged.as<u32>());
            KCHECK_HIP(hipGetLastError());
            KCHECK(dev_scan_counts(lb.as<u32>(), H, label_off.as<u64>(), stream));
            KCHECK(dev_scan_counts(staged.as<u32>(), H, stage_off.as<u64>(), stream));
            KCHECK_HIP(hipMemcpyAsync(&label_bytes, label_off.as<u64>() + H, 8, hipMemcpyDeviceToHost, stream));
            KCHECK_HIP(hipMemcpyAsync(&n_staged, stage_off.as<u64>() + H, 8, hipMemcpyDeviceToHost, stream));
            KCHECK_HIP(hipStreamSynchronize(stream));
        } else {
            KCHECK_HIP(hipMemsetAsync(label_off.p, 0, 8, stream));
        }
        bad = (n_staged != bases_r.n || (want_cov && weights_r.n != bases_r.n)) ? 1 : 0;       // (the weights' places are the bases': one check for both)
        KCHECK(d->comm->allreduce(&bad, 1, OP_MAX));
        if (bad) { set_error("katome_dist_shrink: the offsets of a path are not dense"); return KATOME_E_DEVICE; }
        KCHECK(stage.alloc(n_staged + 16)); KCHECK(label.alloc(label_bytes + 16));
        if (bases_r.n) KLAUNCH(base_place_kernel, bases_r.n, stream, bases_r.a.as<u64>(), bases_r.b.as<u64>(), bases_r.n, slot.as<u32>(), E, H, m.as<u32>(),
                               stage_off.as<u64>(), stage.as<unsigned char>());
        const dim3 pg(grid_for(H * 64, BLOCK, 256u * 32u));
        if (H && nw == 1) hipLaunchKernelGGL(pack_kernel<1>, pg, dim3(BLOCK), 0, stream, heads.as<u32>(), H, b->edge_key.as<u64>(), m.as<u32>(), label_off.as<u64>(),
                                             stage_off.as<u64>(), stage.as<unsigned char>(), k, label.as<unsigned char>());
        if (H && nw == 2) hipLaunchKernelGGL(pack_kernel<2>, pg, dim3(BLOCK), 0, stream, heads.as<u32>(), H, b->edge_key.as<u64>(), m.as<u32>(), label_off.as<u64>(),
                                             stage_off.as<u64>(), stage.as<unsigned char>(), k, label.as<unsigned char>());
        KCHECK_HIP(hipGetLastError());
        DevBuf wstage(stream);                             // coverage: 4 bytes per non-head edge whose head this rank holds, transient
        if (want_cov) {
            KCHECK(wstage.alloc((n_staged + 4) * 4));
            KCHECK(d->sh_cov.kmer_sum.alloc((H + 1) * 8, stream)); KCHECK(d->sh_cov.kmer_min.alloc((H + 1) * 4, stream)); KCHECK(d->sh_cov.kmer_max.alloc((H + 1) * 4, stream));
            if (weights_r.n) KLAUNCH(weight_place_kernel, weights_r.n, stream, weights_r.a.as<u64>(), weights_r.b.as<u64>(), weights_r.n, slot.as<u32>(), E, H, m.as<u32>(),
                                     stage_off.as<u64>(), wstage.as<u32>());
            if (H) hipLaunchKernelGGL(weight_reduce_kernel, pg, dim3(BLOCK), 0, stream, heads.as<u32>(), H, b->edge_weight.as<u32>(), m.as<u32>(), stage_off.as<u64>(),
                                      wstage.as<u32>(), d->sh_cov.kmer_sum.as<u64>(), d->sh_cov.kmer_min.as<u32>(), d->sh_cov.kmer_max.as<u32>());
            KCHECK_HIP(hipGetLastError());
        }
        KCHECK_HIP(hipStreamSynchronize(stream));
    }
    slot.release(); stage_off.release();
    // ---- node numbering through the directory ranges ---------------------------------------------------------------------
    const uint64_t TN = d->total_nodes, per_rank = std::max<uint64_t>(1, (TN + world - 1) / world);
    const uint64_t dbase = std::min<uint64_t>(TN, me * per_rank), range = std::min<uint64_t>(TN, dbase + per_rank) - dbase;
    DevBuf qs(stream), qd(stream), touched(stream), offs(stream), o_src(stream), o_dst(stream), nid(stream);
    KCHECK(qs.alloc((H + 1) * 8)); KCHECK(qd.alloc((H + 1) * 8)); KCHECK(touched.alloc((range + 1) * 4)); KCHECK(offs.alloc((range + 2) * 8));
    KCHECK(o_src.alloc((H + 1) * 8, stream)); KCHECK(o_dst.alloc((H + 1) * 8, stream)); KCHECK(nid.alloc((N + 1) * 8));
    KCHECK_HIP(hipMemsetAsync(touched.p, 0, (range + 1) * 4, stream));
    if (H) KLAUNCH(head_ends_kernel, H, stream, heads.as<u32>(), H, src, end_node.as<u64>(), per_rank, qs.as<u64>(), qd.as<u64>());
    KCHECK_HIP(hipGetLastError());
    end_node.release();
    uint64_t n_new = 0, below = 0, TN_new = 0;
    {
        Routed rs(stream), rd(stream), rn(stream);
        KCHECK(S.router.send(qs.as<u64>(), nullptr, H, rs));
        KCHECK(S.router.send(qd.as<u64>(), nullptr, H, rd));
        if (rs.n) KLAUNCH(touch_kernel, rs.n, stream, rs.a.as<u64>(), rs.n, dbase, range, touched.as<u32>());
        if (rd.n) KLAUNCH(touch_kernel, rd.n, stream, rd.a.as<u64>(), rd.n, dbase, range, touched.as<u32>());
        KCHECK_HIP(hipGetLastError());
        if (range) {
            KCHECK(dev_scan_counts(touched.as<u32>(), range, offs.as<u64>(), stream));
            KCHECK_HIP(hipMemcpyAsync(&n_new, offs.as<u64>() + range, 8, hipMemcpyDeviceToHost, stream));
            KCHECK_HIP(hipStreamSynchronize(stream));
        }
        std::vector<uint64_t> cnt(world, 0);
        KCHECK(d->comm->allgather(n_new, cnt.data()));
        for (int p = 0; p < world; ++p) { if (p < S.rank) below += cnt[p]; TN_new += cnt[p]; }
        DevBuf a(stream);
        for (Routed* r : {&rs, &rd}) {
            KCHECK(a.alloc((r->n + 1) * 8));
            if (r->n) KLAUNCH(new_id_kernel, r->n, stream, r->a.as<u64>(), r->n, dbase, touched.as<u32>(), offs.as<u64>(), range, below, a.as<u64>());
            KCHECK_HIP(hipGetLastError());
            KCHECK(S.router.reply(*r, a.as<u64>(), r == &rs ? o_src.as<u64>() : o_dst.as<u64>()));
        }
        // every node of the share asks whether it stays, and its new id
        DevBuf nq(stream);
        KCHECK(nq.alloc((N + 1) * 8));
        if (N) KLAUNCH(node_q_kernel, N, stream, d->first_seen ? d->node_gid.as<u64>() : nullptr, N, d->node_base, per_rank, nq.as<u64>());
        KCHECK_HIP(hipGetLastError());
        KCHECK(S.router.send(nq.as<u64>(), nullptr, N, rn));
        KCHECK(a.alloc((rn.n + 1) * 8));
        if (rn.n) KLAUNCH(new_id_kernel, rn.n, stream, rn.a.as<u64>(), rn.n, dbase, touched.as<u32>(), offs.as<u64>(), range, below, a.as<u64>());
        KCHECK_HIP(hipGetLastError());
        KCHECK(S.router.reply(rn, a.as<u64>(), nid.as<u64>()));
    }
    qs.release(); qd.release(); touched.release(); offs.release();
    DevBuf keep(stream), kept(stream), o_nid(stream), o_nkey(stream), o_weight(stream), o_head(stream);
    uint64_t NK = 0;
    KCHECK(keep.alloc(N + 16));
    if (N) KLAUNCH(kept_kernel, N, stream, nid.as<u64>(), N, keep.as<unsigned char>());
    KCHECK_HIP(hipGetLastError());
    KCHECK(S.keep_list(keep.as<unsigned char>(), N, kept, &NK));
    KCHECK(o_nid.alloc((NK + 1) * 8, stream)); KCHECK(o_nkey.alloc((NK + 1) * 8 * nw, stream));
    if (NK) {
        KLAUNCH(gather_by_kernel<u64>, NK, stream, nid.as<u64>(), kept.as<u32>(), NK, o_nid.as<u64>());
        if (nw == 1) KLAUNCH(gather_keys_by_kernel<1>, NK, stream, d->node_key.as<u64>(), kept.as<u32>(), NK, o_nkey.as<u64>());
        else         KLAUNCH(gather_keys_by_kernel<2>, NK, stream, d->node_key.as<u64>(), kept.as<u32>(), NK, o_nkey.as<u64>());
    }
    KCHECK(o_weight.alloc((H + 1) * 4, stream)); KCHECK(o_head.alloc((H + 1) * 8, stream));
    if (H) KLAUNCH(head_out_kernel, H, stream, heads.as<u32>(), H, b->edge_weight.as<u32>(), d->first_seen ? d->edge_gid.as<u64>() : nullptr, edge_base,
                   o_weight.as<u32>(), o_head.as<u64>());
    KCHECK_HIP(hipGetLastError());
    KCHECK_HIP(hipStreamSynchronize(stream));
    uint64_t TE_new = H;
    KCHECK(d->comm->allreduce(&TE_new, 1, OP_SUM));
    // the result stays in the builder until the next call or destroy
    auto install = [&](DevBuf& to, DevBuf& from) { const size_t bytes = from.bytes; to.stream = stream; to.adopt(from.take(), bytes); };
    install(d->sh_src, o_src); install(d->sh_dst, o_dst); install(d->sh_weight, o_weight); install(d->sh_kmers, m);
    install(d->sh_label_off, label_off); install(d->sh_label, label); install(d->sh_head, o_head); install(d->sh_node_id, o_nid);
    install(d->sh_node_key, o_nkey);
    d->sh_edges = H; d->sh_nodes = NK; d->sh_total_edges = TE_new; d->sh_total_nodes = TN_new; d->sh_label_bytes = label_bytes;
    if (want_cov) { d->sh_cov.n_edges = H; d->sh_cov.valid = true; }
    if (stats) {
        stats->rank_rounds = rounds; stats->cycle_rounds = cycle_rounds; stats->cycles = n_cycles;
        stats->longest_path = longest; stats->bytes_sent = d->comm->stats.bytes_out - bytes0;
    }
    return KATOME_OK;
}

}  // namespace

extern "C" {

// katome_dist_shrink and katome_dist_shrink_coverage: the coverage of an earlier call never survives a later one of either kind
static int dist_shrink_entry(katome_dist_builder* d, katome_dist_contigs* out, katome_dev_coverage* cov, bool want_cov, katome_dist_shrink_stats* stats, void* stream_) {
    if (out) memset(out, 0, sizeof *out);
    if (cov) memset(cov, 0, sizeof *cov);
    if (stats) memset(stats, 0, sizeof *stats);
    KCHECK(check_shrink_builder(d));
    if (want_cov && !cov) { set_error("null argument"); return KATOME_E_ARG; }
    hipStream_t stream = (hipStream_t)stream_;
    KCHECK_HIP(hipSetDevice(d->s.device));
    d->comm->use_stream(stream);
    static const bool trace = getenv("KATOME_DIST_SHRINK_TRACE") != nullptr;
    katome_dist_shrink_stats st;
    const double t0 = now_ms();
    d->sh_valid = false; ++d->sh_serial;      // (what katome_dist_contigs_text made of the last result is no longer this builder's text)
    d->sh_cov.drop();
    const int rc = dist_shrink(d, &st, stream, want_cov);
    if (rc != KATOME_OK) { d->sh_cov.drop(); return rc; }
    d->sh_valid = true;
    if (trace)
        fprintf(stderr, "[katome_dist_shrink] rank %d/%d: %.2f ms, ranking rounds %u, cycle rounds %u, longest path %llu, sent %llu bytes\n", d->rank(),
                d->world(), now_ms() - t0, st.rank_rounds, st.cycle_rounds, (unsigned long long)st.longest_path, (unsigned long long)st.bytes_sent);
    if (stats) *stats = st;
    if (out) {
        out->n_edges = d->sh_edges; out->n_nodes = d->sh_nodes; out->total_edges = d->sh_total_edges; out->total_nodes = d->sh_total_nodes;
        out->label_bytes = d->sh_label_bytes; out->key_words = d->nw;
        out->d_edge_src = d->sh_src.as<uint64_t>(); out->d_edge_dst = d->sh_dst.as<uint64_t>();
        out->d_edge_weight = d->sh_weight.as<uint32_t>(); out->d_edge_kmers = d->sh_kmers.as<uint32_t>();
        out->d_edge_label_off = d->sh_label_off.as<uint64_t>(); out->d_edge_label = d->sh_label.as<uint8_t>();
        out->d_edge_head_id = d->sh_head.as<uint64_t>(); out->d_node_id = d->sh_node_id.as<uint64_t>(); out->d_node_key = d->sh_node_key.as<uint64_t>();
    }
    if (want_cov) {
        cov->n_edges = d->sh_cov.n_edges;
        cov->d_kmer_sum = d->sh_cov.kmer_sum.as<uint64_t>(); cov->d_kmer_min = d->sh_cov.kmer_min.as<uint32_t>(); cov->d_kmer_max = d->sh_cov.kmer_max.as<uint32_t>();
    }
    return KATOME_OK;
}

int katome_dist_shrink(katome_dist_builder* d, katome_dist_contigs* out, katome_dist_shrink_stats* stats, void* stream_) {
    return dist_shrink_entry(d, out, nullptr, false, stats, stream_);
}
int katome_dist_shrink_coverage(katome_dist_builder* d, katome_dist_contigs* out, katome_dev_coverage* cov, katome_dist_shrink_stats* stats, void* stream_) {
    return dist_shrink_entry(d, out, cov, true, stats, stream_);
}

}  // extern "C"
