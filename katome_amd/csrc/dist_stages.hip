// dist_stages.hip -- the stages of assemble_with_graph between the two prunings (asm/basic_assembler.rs:63-72) on the
// SHARDED graph of a first-seen-ordered build, in the reference's numbering and without a gather:
//   * standardize_contigs (standardizer.rs:72-122), the TABLE route (the other one, list ranking in O(share) memory, is
//     dist_contigs.hip; contigs_route below chooses: KATOME_DIST_CONTIGS, or whether the table fits): a REPLICATED table,
//     one 8-byte word and one 4-byte weight per node of the whole graph (ambiguous / end / pass-through with (owner rank,
//     target) of its single out-edge), is composed on the directory rank of each node id (in-degrees and out-records
//     arrive there in one exchange each) and all-gathered.  Every rank then walks the contigs that start at its own
//     ambiguous nodes with the one-GPU loop, writes the first edge's mean itself and sends (node id, mean) to the owner
//     of every other edge of the contig: one exchange.
//   * prune_weak_edges (Clean::remove_weak_edges, pruner.rs:84-93): retain_edges and then retain_nodes, both "visit the
//     indices in descending order, swap_remove the rejected ones".  The rejected positions go to rank 0, which replays
//     the swap_removes on 64-bit positions (prune.hip's scan + pointer jumping, dev_replay_edges64, every position listed
//     once); only the edges / nodes in the vacated tail ask where they move.  A node is rejected when no surviving edge
//     touches it, which its directory rank knows.
//   * standardize_edges (standardizer.rs:42-70): the two weight sums are allreduced as u64, every rank scales its own
//     weights with the same p, then prune_weak_edges(1).
// Nothing narrower than 64 bits carries an index on the wire or in a replay; a rank's own share stays below 2^32 edges.
// Node ids are below 2^40 (the table words carry them in 40 bits).  DESIGN.md section 6 has the bytes per stage.
#include <math.h>
#include <stdio.h>

#include "dist_route.h"

namespace {

constexpr u64 ID_MASK = (1ull << 40) - 1;
constexpr u64 T_AMBIGUOUS = ~0ull, T_END = ~0ull - 1;     // table words; any other: (owner rank << 40) | target of the single out-edge
constexpr u64 OUT_MORE = 1ull << 44, OUT_HAS = 1ull << 45;

// to the directory rank of a node id: (id / per_rank) << 56 | id
__global__ __launch_bounds__(BLOCK) void dir_addr_kernel(const u64* __restrict__ ids, u64 n, u64 per_rank, u64* __restrict__ out) {
    WLOOP(i, n) if (i < n) out[i] = ((ids[i] / per_rank) << 56) | ids[i];
}
__global__ __launch_bounds__(BLOCK) void dir_count_kernel(const u64* __restrict__ msg, u64 n, u64 base, u32* cnt) {
    WLOOP(i, n) if (i < n) atomicAdd(&cnt[(msg[i] & LOW56) - base], 1u);
}
__global__ __launch_bounds__(BLOCK) void dir_touch_kernel(const u64* __restrict__ msg, u64 n, u64 base, unsigned char* __restrict__ touched) {
    WLOOP(i, n) if (i < n) touched[(msg[i] & LOW56) - base] = 1;
}
__global__ __launch_bounds__(BLOCK) void dir_answer_u8_kernel(const u64* __restrict__ msg, u64 n, u64 base, const unsigned char* __restrict__ v, u64* __restrict__ out) {
    WLOOP(i, n) if (i < n) out[i] = v[(msg[i] & LOW56) - base];
}
__global__ __launch_bounds__(BLOCK) void dir_answer_u64_kernel(const u64* __restrict__ msg, u64 n, u64 base, const u64* __restrict__ v, u64* __restrict__ out) {
    WLOOP(i, n) if (i < n) out[i] = v[(msg[i] & LOW56) - base];
}
__global__ __launch_bounds__(BLOCK) void dir_fill_kernel(const u64* __restrict__ A, const u64* __restrict__ B, u64 n, u64 base, u64* __restrict__ dir) {
    WLOOP(i, n) if (i < n) dir[(A[i] & LOW56) - base] = B[i];
}

// ---- standardize_contigs ---------------------------------------------------------------------------------------------
// one record per node with out-edges (a run of this rank's edges, which are grouped by source), to the node's directory rank:
// A = dir << 56 | (weight & 0xFFFF) << 40 | source id, B = (weight >> 16) << 48 | more than one << 44 | owner << 40 | target
__global__ __launch_bounds__(BLOCK) void out_rec_kernel(const u64* __restrict__ src, const u64* __restrict__ dst, const u32* __restrict__ w, u64 E,
                                                        u64 per_rank, u64 my_rank, u64* __restrict__ A, u64* __restrict__ B, unsigned long long* cursor) {
    WLOOP(e, E) {
        const bool head = e < E && (e == 0 || src[e - 1] != src[e]);
        const u64 at = wave_append(head, cursor);
        if (head) {
            const bool single = e + 1 == E || src[e + 1] != src[e];
            const u64 s = src[e], wt = single ? w[e] : 0u;
            A[at] = ((s / per_rank) << 56) | ((wt & 0xFFFFull) << 40) | s;
            B[at] = ((wt >> 16) << 48) | (single ? 0ull : OUT_MORE) | (my_rank << 40) | dst[e];
        }
    }
}
__global__ __launch_bounds__(BLOCK) void out_place_kernel(const u64* __restrict__ A, const u64* __restrict__ B, u64 n, u64 base, u64* __restrict__ word,
                                                          u32* __restrict__ wt) {
    WLOOP(i, n) if (i < n) {
        const u64 a = A[i], b = B[i], at = (a & ID_MASK) - base;
        word[at] = OUT_HAS | (b & (OUT_MORE | ID_MASK | (0xFull << 40)));
        wt[at] = (u32)(((a >> 40) & 0xFFFFull) | ((b >> 48) << 16));
    }
}
// pt_graph.rs:54-62: ambiguous = in > 1 || out > 1 || (in == 0 && out >= 1); a contig runs through in == out == 1
__global__ __launch_bounds__(BLOCK) void compose_kernel(u64 n, const u32* __restrict__ indeg, u64* __restrict__ word) {
    WLOOP(i, n) if (i < n) {
        const u64 o = word[i];
        const u32 in = indeg[i], out = !(o & OUT_HAS) ? 0u : (o & OUT_MORE) ? 2u : 1u;
        word[i] = (in > 1 || out > 1 || (in == 0 && out >= 1)) ? T_AMBIGUOUS : out == 1 ? (o & (ID_MASK | (0xFull << 40))) : T_END;
    }
}
// the contigs that start at this rank's ambiguous nodes: mean (the one-GPU contig_mean_kernel's u64 sum, f64 division and
// round()), the first edge's weight set here, the number of edges that belong to other nodes' owners
__global__ __launch_bounds__(BLOCK) void contig_walk_kernel(const u64* __restrict__ src, const u64* __restrict__ dst, u64 E, const u64* __restrict__ W,
                                                            const u32* __restrict__ WT, u64 TN, u32* __restrict__ weight, u32* __restrict__ len,
                                                            u32* __restrict__ mean_of, unsigned long long* n_bad) {
    WLOOP(e, E) if (e < E) {
        len[e] = 0;
        if (W[src[e]] != T_AMBIGUOUS) continue;
        u64 v = dst[e], w = W[v], sum = weight[e], L = 1;
        while (w < T_END && L <= TN) { sum += WT[v]; ++L; v = w & ID_MASK; w = W[v]; }
        if (L > TN || L - 1 > 0xFFFFFFFFull) { atomicAdd(n_bad, 1ull); continue; }        // (cannot happen: a contig enters no cycle)
        const u32 mean = (u32)round((double)sum / (double)L);
        weight[e] = mean;
        len[e] = (u32)(L - 1); mean_of[e] = mean;
    }
}
__global__ __launch_bounds__(BLOCK) void contig_emit_kernel(const u64* __restrict__ dst, u64 E, const u64* __restrict__ W, const u32* __restrict__ len,
                                                            const u32* __restrict__ mean_of, const u64* __restrict__ offs, u64* __restrict__ A, u64* __restrict__ B) {
    WLOOP(e, E) if (e < E && len[e]) {
        u64 v = dst[e], at = offs[e];
        for (u32 s = 0; s < len[e]; ++s) {
            const u64 w = W[v];
            A[at + s] = (((w >> 40) & 0xFull) << 56) | v;
            B[at + s] = mean_of[e];
            v = w & ID_MASK;
        }
    }
}
// this rank's edges whose source has no other out-edge: (source id, edge), looked up when the means come back
__global__ __launch_bounds__(BLOCK) void single_list_kernel(const u64* __restrict__ src, u64 E, u64* __restrict__ key, u32* __restrict__ idx, unsigned long long* cursor) {
    WLOOP(e, E) {
        const bool one = e < E && (e == 0 || src[e - 1] != src[e]) && (e + 1 == E || src[e + 1] != src[e]);
        const u64 at = wave_append(one, cursor);
        if (one) { key[at] = src[e]; idx[at] = (u32)e; }
    }
}
__global__ __launch_bounds__(BLOCK) void strip_kernel(const u64* __restrict__ in, u64 n, u64* __restrict__ out) { WLOOP(i, n) if (i < n) out[i] = in[i] & LOW56; }
__global__ __launch_bounds__(BLOCK) void mean_apply_kernel(const u64* __restrict__ found, const u64* __restrict__ mean, u64 n, const u32* __restrict__ idx,
                                                           u32* __restrict__ weight, unsigned long long* n_bad) {
    WLOOP(i, n) if (i < n) {
        if (found[i] == NONE64) { atomicAdd(n_bad, 1ull); continue; }
        weight[idx[found[i]]] = (u32)mean[i];
    }
}

// ---- retain_edges / retain_nodes ---------------------------------------------------------------------------------------
// rejected edges: alive[e] = 0 and their positions for rank 0
__global__ __launch_bounds__(BLOCK) void weak_kernel(const u32* __restrict__ weight, const u64* __restrict__ gid, u64 E, u32 threshold,
                                                     unsigned char* __restrict__ alive, u64* __restrict__ pos, unsigned long long* cursor) {
    TLOOP(t0, E) {
        u32 mine = 0, have = 0;
#pragma unroll
        for (int k = 0; k < CA_ITEMS; ++k) {
            const u64 e = t0 + (u64)k * BLOCK + threadIdx.x;
            if (e < E) { const bool weak = weight[e] < threshold; alive[e] = !weak; if (weak) { have |= 1u << k; ++mine; } }
        }
        u64 at = block_append(mine, cursor);
#pragma unroll
        for (int k = 0; k < CA_ITEMS; ++k) if (have & (1u << k)) pos[at++] = gid[t0 + (u64)k * BLOCK + threadIdx.x];
    }
}
__global__ __launch_bounds__(BLOCK) void ones_kernel(u32* __restrict__ out, u64 n) { WLOOP(i, n) if (i < n) out[i] = 1u; }
// the survivors at positions >= n_new (the tail that disappears): they ask where they move
__global__ __launch_bounds__(BLOCK) void tail_kernel(const u64* __restrict__ ids, const unsigned char* __restrict__ alive, u64 n, u64 n_new,
                                                     u64* __restrict__ q, u32* __restrict__ who, unsigned long long* cursor) {
    TLOOP(t0, n) {
        u32 mine = 0, have = 0;
#pragma unroll
        for (int k = 0; k < CA_ITEMS; ++k) {
            const u64 i = t0 + (u64)k * BLOCK + threadIdx.x;
            if (i < n && (!alive || alive[i]) && ids[i] >= n_new) { have |= 1u << k; ++mine; }
        }
        u64 at = block_append(mine, cursor);
#pragma unroll
        for (int k = 0; k < CA_ITEMS; ++k) if (have & (1u << k)) { const u64 i = t0 + (u64)k * BLOCK + threadIdx.x; q[at] = ids[i]; who[at] = (u32)i; ++at; }
    }
}
// rank 0: where the survivor that sat at the asked position moves (found: its place among the sorted "from" positions)
__global__ __launch_bounds__(BLOCK) void moved_to_kernel(const u64* __restrict__ found, u64 n, const u32* __restrict__ idx, const u64* __restrict__ to, u64* __restrict__ out) {
    WLOOP(i, n) if (i < n) out[i] = found[i] == NONE64 ? NONE64 : to[idx[found[i]]];
}
__global__ __launch_bounds__(BLOCK) void move_apply_kernel(const u32* __restrict__ who, const u64* __restrict__ ans, u64 n, u64* __restrict__ ids, unsigned long long* n_bad) {
    WLOOP(i, n) if (i < n) {
        if (ans[i] == NONE64) { atomicAdd(n_bad, 1ull); continue; }
        ids[who[i]] = ans[i];
    }
}
// rejected nodes (no surviving edge touches them): alive[j] = 0 and their positions for rank 0
__global__ __launch_bounds__(BLOCK) void lone_kernel(const u64* __restrict__ touched, const u64* __restrict__ gid, u64 N, unsigned char* __restrict__ alive,
                                                     u64* __restrict__ pos, unsigned long long* cursor) {
    TLOOP(t0, N) {
        u32 mine = 0, have = 0;
#pragma unroll
        for (int k = 0; k < CA_ITEMS; ++k) {
            const u64 j = t0 + (u64)k * BLOCK + threadIdx.x;
            if (j < N) { const bool lone = touched[j] == 0; alive[j] = !lone; if (lone) { have |= 1u << k; ++mine; } }
        }
        u64 at = block_append(mine, cursor);
#pragma unroll
        for (int k = 0; k < CA_ITEMS; ++k) if (have & (1u << k)) pos[at++] = gid[t0 + (u64)k * BLOCK + threadIdx.x];
    }
}

// ---- links for remove_dead_paths --------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void head_kernel(const u64* __restrict__ src, u64 E, u32* __restrict__ head) {
    WLOOP(e, E) if (e < E) head[e] = (e == 0 || src[e - 1] != src[e]) ? 1u : 0u;
}
__global__ __launch_bounds__(BLOCK) void run_of_kernel(const u64* __restrict__ src, const u32* __restrict__ head, const u64* __restrict__ offs, u64 E,
                                                       u64* __restrict__ lsrc, u64* __restrict__ run_id) {
    WLOOP(e, E) if (e < E) {
        lsrc[e] = offs[e] + head[e] - 1;
        if (head[e]) run_id[offs[e]] = src[e];
    }
}
__global__ __launch_bounds__(BLOCK) void src_node_kernel(const u64* __restrict__ found, u64 n, const u32* __restrict__ idx, u32* __restrict__ perm,
                                                         unsigned char* __restrict__ other, unsigned long long* n_bad) {
    WLOOP(r, n) if (r < n) {
        if (found[r] == NONE64) { atomicAdd(n_bad, 1ull); perm[r] = 0; continue; }
        const u32 j = idx[found[r]];
        perm[r] = j; other[j] = 0;
    }
}
__global__ __launch_bounds__(BLOCK) void dir_rec_kernel(const u64* __restrict__ gid, u64 N, u64 per_rank, u64 my_rank, u64* __restrict__ A, u64* __restrict__ B) {
    WLOOP(j, N) if (j < N) { A[j] = ((gid[j] / per_rank) << 56) | gid[j]; B[j] = (my_rank << 56) | j; }
}
__global__ __launch_bounds__(BLOCK) void split_dir_kernel(const u64* __restrict__ in, u64 n, u64 world, u64* __restrict__ drank, u64* __restrict__ dlocal,
                                                          unsigned long long* n_bad) {
    WLOOP(i, n) if (i < n) {
        const u64 v = in[i];
        if (v == NONE64 || (v >> 56) >= world) { atomicAdd(n_bad, 1ull); drank[i] = 0; dlocal[i] = 0; continue; }    // (no node registered that id)
        drank[i] = v >> 56; dlocal[i] = v & LOW56;
    }
}

// KATOME_DIST_STAGES_FAIL=edges|nodes: rank 0's replay of that kind reports a failure (tests of "every rank leaves with the
// same error, nobody is left waiting in a collective")
bool stage_fail_at(const char* what) {
    const char* at = getenv("KATOME_DIST_STAGES_FAIL");
    return at && !strcmp(at, what);
}

// what one stage needs on every call
struct Stage {
    katome_dist_builder* d; hipStream_t stream; int rank, world; uint64_t E, N, TE, TN, per_rank, base, range; uint32_t pos_bits;
    Router router; DevBuf cursors;
    Stage(katome_dist_builder* d_, hipStream_t s) : d(d_), stream(s), rank(d_->rank()), world(d_->world()), E(d_->n_edges), N(d_->n_nodes),
        TE(d_->total_edges), TN(d_->total_nodes), router(d_, s), cursors(s) {
        per_rank = std::max<uint64_t>(1, (TN + world - 1) / world);
        base = std::min<uint64_t>(TN, (uint64_t)rank * per_rank);
        range = std::min<uint64_t>(TN, base + per_rank) - base;
        pos_bits = 1;
        while (pos_bits < 64 && ((std::max(TE, TN) + 1) >> pos_bits)) ++pos_bits;
    }
    unsigned long long* cur() { return cursors.as<unsigned long long>(); }
    int init() { KCHECK(cursors.alloc(64)); return router.init(); }
    int reset() { KCHECK_HIP(hipMemsetAsync(cursors.p, 0, 64, stream)); return KATOME_OK; }
    int read(uint64_t* h, int n) {
        KCHECK_HIP(hipMemcpyAsync(h, cursors.p, 8 * n, hipMemcpyDeviceToHost, stream));
        KCHECK_HIP(hipStreamSynchronize(stream));
        return KATOME_OK;
    }
    // indices of the set bytes, ascending
    int keep_list(const unsigned char* alive, uint64_t n, DevBuf& keep, uint64_t* n_keep) {
        KCHECK(keep.alloc((n + 1) * 4));
        KCHECK(reset());
        if (n) KLAUNCH_T(alive_list_kernel, n, stream, alive, n, keep.as<u32>(), cur());
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
    // a device counter that must have stayed 0: a broken invariant is an error on every rank
    int agree_clean(const char* what) {
        uint64_t h[8] = {0};
        KCHECK(read(h, 8));
        uint64_t bad = h[7];
        KCHECK(d->comm->allreduce(&bad, 1, OP_MAX));
        if (bad) { set_error("sharded stages: %s (%llu inconsistent records)", what, (unsigned long long)bad); return KATOME_E_DEVICE; }
        return KATOME_OK;
    }
};

int check_builder(katome_dist_builder* d, const char* name) {
    if (!d) { set_error("null argument"); return KATOME_E_ARG; }
    if (!d->finalized || !d->first_seen) { set_error("%s: a finalized FIRST_SEEN_ORDER build only (petgraph's numbering decides what the stage does)", name); return KATOME_E_ARG; }
    if (d->gathered) { set_error("%s: the ranks' shares were gathered (katome_dist_gather); run the stage on the gathered graph's root", name); return KATOME_E_ARG; }
    return KATOME_OK;
}
// every rank's share below 2^32 edges and nodes, the node ids below 2^40 (agreed: nobody leaves alone)
int check_sizes(katome_dist_builder* d) {
    uint64_t bad = (d->n_edges >= 0xFFFFFFFFull || d->n_nodes >= 0xFFFFFFFFull || d->total_nodes > ID_MASK) ? 1 : 0;
    KCHECK(d->comm->allreduce(&bad, 1, OP_MAX));
    if (bad) { set_error("sharded stages: more than 2^32 edges or nodes on one rank, or more than 2^40 nodes"); return KATOME_E_UNSUPPORTED; }
    return KATOME_OK;
}

// positions of this rank's items that the replay may move: `ids` updated in place, `alive` which of them survive (null: all);
// fewer than 2^32 items per list, so that an item's place in its list and a Router send of the list fit 32 bits
struct IdList { u64* ids; const unsigned char* alive; uint64_t n; };

// rank 0 replays "swap_remove every listed position, descending" over n positions (its `pos` hold the listed positions of
// every rank); every rank learns the new count and moves the survivors of its lists that sat in the vacated tail
int retain_replay(Stage& S, const u64* pos, uint64_t u_local, uint64_t n, const IdList* lists, int n_lists, const char* kind,
                  uint64_t* n_new_out) {
    hipStream_t stream = S.stream;
    uint64_t u_total = u_local;
    KCHECK(S.d->comm->allreduce(&u_total, 1, OP_SUM));
    *n_new_out = n - u_total;
    if (u_total == 0) return KATOME_OK;
    Routed at_root(stream);
    KCHECK(S.router.send(pos, nullptr, u_local, at_root));           // (positions < 2^56: top byte 0, everything goes to rank 0)
    DevBuf to(stream), from(stream), from_sorted(stream), from_idx(stream);
    uint64_t removed = 0, n_new = n, n_moves = 0;
    auto root_replay = [&]() -> int {
        const uint64_t u = at_root.n;
        if (u >= 0xFFFFFFFFull) { set_error("sharded stages: 2^32 %s or more removed in one retain", kind); return KATOME_E_UNSUPPORTED; }
        DevBuf mult(stream), victims(stream);
        ReplayScratch sc(stream);
        KCHECK(mult.alloc((u + 1) * 4));
        KLAUNCH(ones_kernel, u, stream, mult.as<u32>(), u);
        KCHECK(dev_sort(at_root.a.as<u64>(), nullptr, u, 1, S.pos_bits, stream));
        uint64_t dups = 0;
        KCHECK(dev_replay_edges64(at_root.a.as<u64>(), mult.as<u32>(), u, n, sc, victims, to, from, &removed, &n_new, &n_moves, &dups, stream));
        if (removed != u) { set_error("sharded stages: the %s replay removed %llu of %llu listed positions", kind, (unsigned long long)removed, (unsigned long long)u); return KATOME_E_DEVICE; }
        KCHECK(from_sorted.alloc((n_moves + 1) * 8)); KCHECK(from_idx.alloc((n_moves + 1) * 4));
        if (n_moves) {
            KCHECK_HIP(hipMemcpyAsync(from_sorted.p, from.p, n_moves * 8, hipMemcpyDeviceToDevice, stream));
            KLAUNCH(iota32_kernel, n_moves, stream, from_idx.as<u32>(), n_moves);
            KCHECK(dev_sort(from_sorted.as<u64>(), from_idx.as<u32>(), n_moves, 1, S.pos_bits, stream));
        }
        KCHECK_HIP(hipGetLastError());
        return KATOME_OK;
    };
    int root_rc = S.rank == 0 ? root_replay() : KATOME_OK;
    if (S.rank == 0 && root_rc == KATOME_OK && stage_fail_at(kind)) { set_error("sharded stages: KATOME_DIST_STAGES_FAIL=%s", kind); root_rc = KATOME_E_UNSUPPORTED; }
    // (what failed on rank 0 alone travels with the count every rank agrees on, and every rank returns it)
    uint64_t agreed[2] = {S.rank == 0 && root_rc == KATOME_OK ? n_new : 0, (uint64_t)(-root_rc)};
    KCHECK(S.d->comm->allreduce(agreed, 2, OP_MAX));
    if (agreed[1]) {
        if (S.rank != 0) set_error("sharded stages: rank 0 failed in the replay of the removed %s (status %d)", kind, -(int)agreed[1]);
        return -(int)agreed[1];
    }
    n_new = agreed[0];
    if (n_new != n - u_total) { set_error("sharded stages: the %s replay disagrees with the count of listed positions", kind); return KATOME_E_DEVICE; }
    // the survivors in the tail [n_new, n) ask rank 0 where they go, list by list (the same lists on every rank)
    for (int l = 0; l < n_lists; ++l) {
        const IdList& L = lists[l];
        DevBuf q(stream), who(stream), ans(stream);
        KCHECK(q.alloc((L.n + 1) * 8)); KCHECK(who.alloc((L.n + 1) * 4));
        KCHECK(S.reset());
        if (L.n) KLAUNCH_T(tail_kernel, L.n, stream, L.ids, L.alive, L.n, n_new, q.as<u64>(), who.as<u32>(), S.cur());
        KCHECK_HIP(hipGetLastError());
        uint64_t h[1] = {0};
        KCHECK(S.read(h, 1));
        const uint64_t n_q = h[0];
        KCHECK(ans.alloc((n_q + 1) * 8));
        Routed asked(stream);
        KCHECK(S.router.send(q.as<u64>(), nullptr, n_q, asked));
        DevBuf found(stream), a(stream);
        KCHECK(found.alloc((asked.n + 1) * 8)); KCHECK(a.alloc((asked.n + 1) * 8));
        if (asked.n) {                                                  // (rank 0 only)
            if (n_moves) KCHECK(dev_rank(from_sorted.as<u64>(), n_moves, 1, S.pos_bits, asked.a.as<u64>(), asked.n, found.as<u64>(), stream));
            else KCHECK_HIP(hipMemsetAsync(found.p, 0xFF, asked.n * 8, stream));
            KLAUNCH(moved_to_kernel, asked.n, stream, found.as<u64>(), asked.n, from_idx.as<u32>(), to.as<u64>(), a.as<u64>());
            KCHECK_HIP(hipGetLastError());
        }
        KCHECK(S.router.reply(asked, a.as<u64>(), ans.as<u64>()));
        KCHECK(S.reset());
        if (n_q) KLAUNCH(move_apply_kernel, n_q, stream, who.as<u32>(), ans.as<u64>(), n_q, L.ids, S.cur() + 7);
        KCHECK_HIP(hipGetLastError());
        KCHECK(S.agree_clean("a survivor in the vacated tail has no place"));
    }
    return KATOME_OK;
}

template <class T>
int compact(DevBuf& buf, const DevBuf& keep, uint64_t n, hipStream_t stream) {
    DevBuf out(stream);
    KCHECK(out.alloc((n + 1) * sizeof(T)));
    if (n) KLAUNCH(gather_by_kernel<T>, n, stream, buf.as<T>(), keep.as<u32>(), n, out.as<T>());
    KCHECK_HIP(hipGetLastError());
    const size_t bytes = out.bytes;
    buf.stream = stream; buf.adopt(out.take(), bytes);
    return KATOME_OK;
}
int compact_keys(DevBuf& buf, const DevBuf& keep, uint64_t n, uint32_t nw, hipStream_t stream) {
    DevBuf out(stream);
    KCHECK(out.alloc((n + 1) * 8 * nw));
    if (n && nw == 1) KLAUNCH(gather_keys_by_kernel<1>, n, stream, buf.as<u64>(), keep.as<u32>(), n, out.as<u64>());
    if (n && nw == 2) KLAUNCH(gather_keys_by_kernel<2>, n, stream, buf.as<u64>(), keep.as<u32>(), n, out.as<u64>());
    KCHECK_HIP(hipGetLastError());
    const size_t bytes = out.bytes;
    buf.stream = stream; buf.adopt(out.take(), bytes);
    return KATOME_OK;
}

// Clean::remove_weak_edges (pruner.rs:84-93): retain_edges(weight >= threshold), then retain_nodes(has a neighbour)
int prune_weak(katome_dist_builder* d, uint32_t threshold, hipStream_t stream) {
    Stage S(d, stream);
    KCHECK(S.init());
    katome_builder* b = d->b;
    if (S.TE == 0) return KATOME_OK;                         // (as the one-GPU form: an empty graph is left as it is)
    uint64_t E = S.E, N = S.N;
    if (!d->edge_age.p) {                                    // the ages move with their edges: remove_dead_paths may follow
        KCHECK(d->edge_age.alloc((E + 1) * 8, stream));
        if (E) KCHECK_HIP(hipMemcpyAsync(d->edge_age.p, d->edge_gid.p, E * 8, hipMemcpyDeviceToDevice, stream));
    }
    // ---- retain_edges ----------------------------------------------------------------------------------------------------
    DevBuf alive(stream), pos(stream);
    KCHECK(alive.alloc(E + 16)); KCHECK(pos.alloc((E + 1) * 8));
    KCHECK(S.reset());
    if (E) KLAUNCH_T(weak_kernel, E, stream, b->edge_weight.as<u32>(), d->edge_gid.as<u64>(), E, threshold, alive.as<unsigned char>(), pos.as<u64>(), S.cur());
    KCHECK_HIP(hipGetLastError());
    uint64_t h[1] = {0};
    KCHECK(S.read(h, 1));
    uint64_t TE_new = S.TE;
    {
        const IdList edges[1] = {{d->edge_gid.as<u64>(), alive.as<unsigned char>(), E}};
        KCHECK(retain_replay(S, pos.as<u64>(), h[0], S.TE, edges, 1, "edges", &TE_new));
    }
    pos.release();
    const bool edges_went = TE_new != S.TE;
    if (edges_went) {
        DevBuf keep(stream);
        uint64_t E2 = 0;
        KCHECK(S.keep_list(alive.as<unsigned char>(), E, keep, &E2));
        KCHECK(compact_keys(b->edge_key, keep, E2, d->nw, stream));
        KCHECK(compact<u32>(b->edge_weight, keep, E2, stream));
        KCHECK(compact<u64>(d->edge_src, keep, E2, stream)); KCHECK(compact<u64>(d->edge_dst, keep, E2, stream));
        KCHECK(compact<u64>(d->edge_gid, keep, E2, stream)); KCHECK(compact<u64>(d->edge_age, keep, E2, stream));
        E = E2;
    }
    alive.release();
    // ---- retain_nodes: a node no surviving edge touches goes (its directory rank knows) -----------------------------------
    DevBuf touched(stream), msg(stream);
    KCHECK(touched.alloc(S.range + 16));
    KCHECK_HIP(hipMemsetAsync(touched.p, 0, S.range + 16, stream));
    KCHECK(msg.alloc((E + 1) * 8));
    for (const DevBuf* end : {&d->edge_src, &d->edge_dst}) {          // (one send per end: a send stays below 2^32 records)
        if (E) KLAUNCH(dir_addr_kernel, E, stream, end->as<u64>(), E, S.per_rank, msg.as<u64>());
        KCHECK_HIP(hipGetLastError());
        Routed r(stream);
        KCHECK(S.router.send(msg.as<u64>(), nullptr, E, r));
        if (r.n) KLAUNCH(dir_touch_kernel, r.n, stream, r.a.as<u64>(), r.n, S.base, touched.as<unsigned char>());
        KCHECK_HIP(hipGetLastError());
    }
    DevBuf ntouch(stream);
    KCHECK(ntouch.alloc((N + 1) * 8));
    {
        KCHECK(msg.alloc((N + 1) * 8));
        if (N) KLAUNCH(dir_addr_kernel, N, stream, d->node_gid.as<u64>(), N, S.per_rank, msg.as<u64>());
        KCHECK_HIP(hipGetLastError());
        Routed asked(stream);
        KCHECK(S.router.send(msg.as<u64>(), nullptr, N, asked));
        DevBuf a(stream);
        KCHECK(a.alloc((asked.n + 1) * 8));
        if (asked.n) KLAUNCH(dir_answer_u8_kernel, asked.n, stream, asked.a.as<u64>(), asked.n, S.base, touched.as<unsigned char>(), a.as<u64>());
        KCHECK_HIP(hipGetLastError());
        KCHECK(S.router.reply(asked, a.as<u64>(), ntouch.as<u64>()));
    }
    touched.release(); msg.release();
    DevBuf nalive(stream), npos(stream);
    KCHECK(nalive.alloc(N + 16)); KCHECK(npos.alloc((N + 1) * 8));
    KCHECK(S.reset());
    if (N) KLAUNCH_T(lone_kernel, N, stream, ntouch.as<u64>(), d->node_gid.as<u64>(), N, nalive.as<unsigned char>(), npos.as<u64>(), S.cur());
    KCHECK_HIP(hipGetLastError());
    KCHECK(S.read(h, 1));
    ntouch.release();
    // the ids that may move, in place: this rank's surviving nodes and both endpoints of its edges (a dead node has no edge)
    uint64_t TN_new = S.TN;
    {
        const IdList ends[3] = {{d->node_gid.as<u64>(), nalive.as<unsigned char>(), N}, {d->edge_src.as<u64>(), nullptr, E},
                                {d->edge_dst.as<u64>(), nullptr, E}};
        KCHECK(retain_replay(S, npos.as<u64>(), h[0], S.TN, ends, 3, "nodes", &TN_new));
    }
    npos.release();
    const bool nodes_went = TN_new != S.TN;
    if (nodes_went) {
        DevBuf keep(stream);
        uint64_t N2 = 0;
        KCHECK(S.keep_list(nalive.as<unsigned char>(), N, keep, &N2));
        KCHECK(compact_keys(d->node_key, keep, N2, d->nw, stream));
        KCHECK(compact<u64>(d->node_gid, keep, N2, stream));
        N = N2;
    }
    if (edges_went) {
        const uint32_t lstride = label_stride_for_k(d->s.k);
        KCHECK(d->edge_label.alloc((E + 1) * (size_t)lstride + 16, stream));
        KCHECK(dev_labels(b->edge_key.as<u64>(), E, d->s.k, d->edge_label.as<uint8_t>(), stream));
    }
    KCHECK_HIP(hipStreamSynchronize(stream));
    if (edges_went || nodes_went) {
        // local node indices and target links of the old share are stale: katome_dist_remove_dead_paths rebuilds them, and
        // runs for real (something has changed since its last fixpoint)
        b->edge_seq.release();
        d->edge_lsrc.release(); d->edge_drank.release(); d->edge_dlocal.release();
        d->n_src = 0;
        d->dead_paths_removed = false;
    }
    b->n_edges = E;
    d->n_edges = E; d->n_nodes = N; d->total_edges = TE_new; d->total_nodes = TN_new;
    return KATOME_OK;
}

}  // namespace

// remove_dead_paths after a stage that removed edges or nodes: every edge's source as the local index of its node (the nodes
// with out-edges first, in the order of their edges' runs) and its target as (owner rank, local index there), through the
// directory sharded by node id
int dist_rebuild_links(katome_dist_builder* d, hipStream_t stream) {
    Stage S(d, stream);
    KCHECK(S.init());
    const uint64_t E = S.E, N = S.N;
    DevBuf head(stream), offs(stream), lsrc(stream), run_id(stream);
    KCHECK(head.alloc((E + 1) * 4)); KCHECK(offs.alloc((E + 2) * 8)); KCHECK(lsrc.alloc((E + 1) * 8)); KCHECK(run_id.alloc((E + 1) * 8));
    uint64_t n_src = 0;
    if (E) {
        KLAUNCH(head_kernel, E, stream, d->edge_src.as<u64>(), E, head.as<u32>());
        KCHECK(dev_scan_counts(head.as<u32>(), E, offs.as<u64>(), stream));
        KLAUNCH(run_of_kernel, E, stream, d->edge_src.as<u64>(), head.as<u32>(), offs.as<u64>(), E, lsrc.as<u64>(), run_id.as<u64>());
        KCHECK_HIP(hipGetLastError());
        KCHECK_HIP(hipMemcpyAsync(&n_src, offs.as<u64>() + E, 8, hipMemcpyDeviceToHost, stream));
        KCHECK_HIP(hipStreamSynchronize(stream));
    }
    head.release(); offs.release();
    // the local node of every run: its id among this rank's sorted node ids
    DevBuf sorted(stream), sidx(stream), found(stream), perm(stream), other(stream);
    KCHECK(sorted.alloc((N + 1) * 8)); KCHECK(sidx.alloc((N + 1) * 4)); KCHECK(found.alloc((n_src + 1) * 8));
    KCHECK(perm.alloc((N + 1) * 4)); KCHECK(other.alloc(N + 16));
    KCHECK(S.reset());
    if (N) {
        KCHECK_HIP(hipMemcpyAsync(sorted.p, d->node_gid.p, N * 8, hipMemcpyDeviceToDevice, stream));
        KLAUNCH(iota32_kernel, N, stream, sidx.as<u32>(), N);
        KCHECK(dev_sort(sorted.as<u64>(), sidx.as<u32>(), N, 1, S.pos_bits, stream));
        KCHECK_HIP(hipMemsetAsync(other.p, 1, N, stream));
    }
    if (n_src) {
        KCHECK(dev_rank(sorted.as<u64>(), N, 1, S.pos_bits, run_id.as<u64>(), n_src, found.as<u64>(), stream));
        KLAUNCH(src_node_kernel, n_src, stream, found.as<u64>(), n_src, sidx.as<u32>(), perm.as<u32>(), other.as<unsigned char>(), S.cur() + 7);
    }
    KCHECK_HIP(hipGetLastError());
    KCHECK(S.agree_clean("an edge's source is not a node of its rank"));
    sorted.release(); sidx.release(); found.release(); run_id.release();
    {   // the nodes without out-edges follow, in their order
        DevBuf rest(stream);
        uint64_t n_rest = 0;
        KCHECK(S.keep_list(other.as<unsigned char>(), N, rest, &n_rest));
        uint64_t bad = n_src + n_rest != N ? 1 : 0;                   // (agreed: the directory exchange below is collective)
        KCHECK(d->comm->allreduce(&bad, 1, OP_MAX));
        if (bad) { set_error("sharded stages: a node is the source of two runs"); return KATOME_E_DEVICE; }
        if (n_rest) KCHECK_HIP(hipMemcpyAsync(perm.as<u32>() + n_src, rest.p, n_rest * 4, hipMemcpyDeviceToDevice, stream));
        KCHECK(compact_keys(d->node_key, perm, N, d->nw, stream));
        KCHECK(compact<u64>(d->node_gid, perm, N, stream));
    }
    // the directory: node id -> (owner rank << 56) | local index
    DevBuf dir(stream), da(stream), db(stream);
    KCHECK(dir.alloc((S.range + 1) * 8)); KCHECK(da.alloc((N + 1) * 8)); KCHECK(db.alloc((N + 1) * 8));
    KCHECK_HIP(hipMemsetAsync(dir.p, 0xFF, (S.range + 1) * 8, stream));
    if (N) KLAUNCH(dir_rec_kernel, N, stream, d->node_gid.as<u64>(), N, S.per_rank, (u64)S.rank, da.as<u64>(), db.as<u64>());
    KCHECK_HIP(hipGetLastError());
    {
        Routed r(stream);
        KCHECK(S.router.send(da.as<u64>(), db.as<u64>(), N, r));
        if (r.n) KLAUNCH(dir_fill_kernel, r.n, stream, r.a.as<u64>(), r.b.as<u64>(), r.n, S.base, dir.as<u64>());
        KCHECK_HIP(hipGetLastError());
    }
    da.release(); db.release();
    DevBuf q(stream), where(stream), drank(stream), dlocal(stream);
    KCHECK(q.alloc((E + 1) * 8)); KCHECK(where.alloc((E + 1) * 8)); KCHECK(drank.alloc((E + 1) * 8)); KCHECK(dlocal.alloc((E + 1) * 8));
    if (E) KLAUNCH(dir_addr_kernel, E, stream, d->edge_dst.as<u64>(), E, S.per_rank, q.as<u64>());
    KCHECK_HIP(hipGetLastError());
    {
        Routed asked(stream);
        KCHECK(S.router.send(q.as<u64>(), nullptr, E, asked));
        DevBuf a(stream);
        KCHECK(a.alloc((asked.n + 1) * 8));
        if (asked.n) KLAUNCH(dir_answer_u64_kernel, asked.n, stream, asked.a.as<u64>(), asked.n, S.base, dir.as<u64>(), a.as<u64>());
        KCHECK_HIP(hipGetLastError());
        KCHECK(S.router.reply(asked, a.as<u64>(), where.as<u64>()));
    }
    KCHECK(S.reset());
    if (E) KLAUNCH(split_dir_kernel, E, stream, where.as<u64>(), E, (u64)S.world, drank.as<u64>(), dlocal.as<u64>(), S.cur() + 7);
    KCHECK_HIP(hipGetLastError());
    KCHECK(S.agree_clean("an edge's target is a node no rank holds"));
    auto install = [&](DevBuf& to, DevBuf& from) { const size_t bytes = from.bytes; to.stream = stream; to.adopt(from.take(), bytes); };
    install(d->edge_lsrc, lsrc); install(d->edge_drank, drank); install(d->edge_dlocal, dlocal);
    d->n_src = n_src;
    return KATOME_OK;
}

namespace {

// KATOME_DIST_CONTIGS=table|ranked names the route of katome_dist_standardize_contigs; unset: the table when it fits every
// rank, the ranked route (dist_contigs.hip) otherwise.  One allreduce: the ranks' environments and whether the table fits;
// ranks that disagree, or a value that names no route, are KATOME_E_ARG on every rank.
// KATOME_DIST_CONTIGS_TABLE_LIMIT=<bytes> (tests) stands in for the free memory.
enum ContigsRoute { CONTIGS_TABLE = 0, CONTIGS_RANKED = 1 };
int contigs_route(katome_dist_builder* d, const Stage& S, uint32_t* route) {
    const char* e = getenv("KATOME_DIST_CONTIGS");
    const int said = !e || !*e ? 0 : !strcmp(e, "table") ? 1 : !strcmp(e, "ranked") ? 2 : 3;
    // the replicated table: 12 bytes per node of the whole graph on every rank
    size_t free_b = 0, total_b = 0;
    KCHECK_HIP(hipMemGetInfo(&free_b, &total_b));
    free_b += dev_cached_bytes();
    const char* lim = getenv("KATOME_DIST_CONTIGS_TABLE_LIMIT");
    if (lim && *lim) free_b = (size_t)strtoull(lim, nullptr, 10);
    const uint64_t need = (S.TN + 1) * 12 + S.range * 28 + (S.E + 1) * 40 + (1ull << 30);
    uint64_t v[5] = {said == 0, said == 1, said == 2, said == 3, need < free_b ? 0ull : 1ull};      // [4]: no room on some rank
    KCHECK(d->comm->allreduce(v, 5, OP_MAX));
    if (v[3]) { set_error("katome_dist_standardize_contigs: KATOME_DIST_CONTIGS must be table or ranked%s%s", said == 3 ? ", not " : " on every rank", said == 3 ? e : ""); return KATOME_E_ARG; }
    if (v[0] + v[1] + v[2] != 1) { set_error("katome_dist_standardize_contigs: the ranks disagree on KATOME_DIST_CONTIGS"); return KATOME_E_ARG; }
    if (v[1] && v[4]) { set_error("katome_dist_standardize_contigs: the replicated node table (%llu nodes, 12 B each) does not fit a rank's free HBM", (unsigned long long)S.TN); return KATOME_E_OOM; }
    *route = v[2] || (v[0] && v[4]) ? CONTIGS_RANKED : CONTIGS_TABLE;
    return KATOME_OK;
}
int contigs_table(katome_dist_builder* d, Stage& S, hipStream_t stream);

}  // namespace

extern "C" {

int katome_dist_standardize_contigs(katome_dist_builder* d, katome_dist_graph* out, void* stream_) {
    KCHECK(check_builder(d, "katome_dist_standardize_contigs"));
    hipStream_t stream = (hipStream_t)stream_;
    KCHECK_HIP(hipSetDevice(d->s.device));
    d->comm->use_stream(stream);
    KCHECK(check_sizes(d));
    Stage S(d, stream);
    KCHECK(S.init());
    const bool trace = getenv("KATOME_DIST_CONTIGS_TRACE") != nullptr;       // (asked for on every call, as the stage's other switches)
    katome_dist_standardize_stats st = {};
    const uint64_t bytes0 = d->comm->stats.bytes_out;
    const double t0 = now_ms();
    KCHECK(contigs_route(d, S, &st.route));
    if (st.route == CONTIGS_RANKED) KCHECK(dist_contigs_ranked(d, stream, &st));
    else KCHECK(contigs_table(d, S, stream));
    st.bytes_sent = d->comm->stats.bytes_out - bytes0;
    d->contigs_stats = st; d->contigs_stats_valid = true;
    if (trace)
        fprintf(stderr, "[katome_dist_standardize_contigs] rank %d/%d: %.2f ms, route %s, ranking rounds %u, exchanges %llu, contigs %llu, longest %llu, "
                "cycle edges %llu, sent %llu bytes\n", d->rank(), d->world(), now_ms() - t0, st.route == CONTIGS_RANKED ? "ranked" : "table", st.rank_rounds,
                (unsigned long long)st.exchanges, (unsigned long long)st.contigs, (unsigned long long)st.longest_contig, (unsigned long long)st.cycle_edges,
                (unsigned long long)st.bytes_sent);
    return katome_dist_current_graph(d, out);
}

}  // extern "C"

namespace {

// the table route
int contigs_table(katome_dist_builder* d, Stage& S, hipStream_t stream) {
    katome_builder* b = d->b;
    const uint64_t E = S.E, TN = S.TN;
    const u64* src = d->edge_src.as<u64>(); const u64* dst = d->edge_dst.as<u64>();
    // ---- in-degrees on the directory rank of each node id ---------------------------------------------------------------
    DevBuf indeg(stream), word(stream), wt(stream);
    KCHECK(indeg.alloc((S.range + 1) * 4)); KCHECK(word.alloc((S.range + 1) * 8)); KCHECK(wt.alloc((S.range + 1) * 4));
    KCHECK_HIP(hipMemsetAsync(indeg.p, 0, (S.range + 1) * 4, stream));
    KCHECK_HIP(hipMemsetAsync(word.p, 0, (S.range + 1) * 8, stream));
    KCHECK_HIP(hipMemsetAsync(wt.p, 0, (S.range + 1) * 4, stream));
    {
        DevBuf msg(stream);
        KCHECK(msg.alloc((E + 1) * 8));
        if (E) KLAUNCH(dir_addr_kernel, E, stream, dst, E, S.per_rank, msg.as<u64>());
        KCHECK_HIP(hipGetLastError());
        Routed r(stream);
        KCHECK(S.router.send(msg.as<u64>(), nullptr, E, r));
        if (r.n) KLAUNCH(dir_count_kernel, r.n, stream, r.a.as<u64>(), r.n, S.base, indeg.as<u32>());
        KCHECK_HIP(hipGetLastError());
    }
    // ---- out-degree class, single out-edge and its weight: one record per node with out-edges -----------------------------
    {
        DevBuf A(stream), B(stream);
        KCHECK(A.alloc((E + 1) * 8)); KCHECK(B.alloc((E + 1) * 8));
        KCHECK(S.reset());
        if (E) KLAUNCH(out_rec_kernel, E, stream, src, dst, b->edge_weight.as<u32>(), E, S.per_rank, (u64)S.rank, A.as<u64>(), B.as<u64>(), S.cur());
        KCHECK_HIP(hipGetLastError());
        uint64_t h[1] = {0};
        KCHECK(S.read(h, 1));
        Routed r(stream);
        KCHECK(S.router.send(A.as<u64>(), B.as<u64>(), h[0], r));
        if (r.n) KLAUNCH(out_place_kernel, r.n, stream, r.a.as<u64>(), r.b.as<u64>(), r.n, S.base, word.as<u64>(), wt.as<u32>());
        if (S.range) KLAUNCH(compose_kernel, S.range, stream, S.range, indeg.as<u32>(), word.as<u64>());
        KCHECK_HIP(hipGetLastError());
    }
    indeg.release();
    // ---- every rank's ranges -> the whole table on every rank ---------------------------------------------------------------
    DevBuf W(stream), WT(stream);
    uint64_t got_w = 0, got_t = 0;
    KCHECK(S.router.allgather(word.p, S.range, 8, W, &got_w));
    KCHECK(S.router.allgather(wt.p, S.range, 4, WT, &got_t));
    word.release(); wt.release();
    if (got_w != TN || got_t != TN) { set_error("katome_dist_standardize_contigs: the table has %llu of %llu nodes", (unsigned long long)got_w, (unsigned long long)TN); return KATOME_E_DEVICE; }
    // ---- the walks from this rank's ambiguous nodes; the means of the other edges go to their owners ----------------------
    DevBuf len(stream), mean_of(stream), offs(stream);
    KCHECK(len.alloc((E + 1) * 4)); KCHECK(mean_of.alloc((E + 1) * 4)); KCHECK(offs.alloc((E + 2) * 8));
    KCHECK(S.reset());
    if (E) KLAUNCH(contig_walk_kernel, E, stream, src, dst, E, W.as<u64>(), WT.as<u32>(), TN, b->edge_weight.as<u32>(), len.as<u32>(), mean_of.as<u32>(), S.cur() + 7);
    KCHECK_HIP(hipGetLastError());
    KCHECK(S.agree_clean("a contig walk did not end"));
    uint64_t n_rec = 0;
    if (E) {
        KCHECK(dev_scan_counts(len.as<u32>(), E, offs.as<u64>(), stream));
        KCHECK_HIP(hipMemcpyAsync(&n_rec, offs.as<u64>() + E, 8, hipMemcpyDeviceToHost, stream));
        KCHECK_HIP(hipStreamSynchronize(stream));
    }
    DevBuf A(stream), B(stream);
    KCHECK(A.alloc((n_rec + 1) * 8)); KCHECK(B.alloc((n_rec + 1) * 8));
    if (n_rec) KLAUNCH(contig_emit_kernel, E, stream, dst, E, W.as<u64>(), len.as<u32>(), mean_of.as<u32>(), offs.as<u64>(), A.as<u64>(), B.as<u64>());
    KCHECK_HIP(hipGetLastError());
    len.release(); mean_of.release(); offs.release();
    W.release(); WT.release();
    // the owner writes each mean on the single out-edge of the node it names: its edges whose source has no other out-edge,
    // sorted by source id
    DevBuf skey(stream), sidx(stream);
    KCHECK(skey.alloc((E + 1) * 8)); KCHECK(sidx.alloc((E + 1) * 4));
    KCHECK(S.reset());
    if (E) KLAUNCH(single_list_kernel, E, stream, src, E, skey.as<u64>(), sidx.as<u32>(), S.cur());
    KCHECK_HIP(hipGetLastError());
    uint64_t h[1] = {0};
    KCHECK(S.read(h, 1));
    const uint64_t n_single = h[0];
    if (n_single) KCHECK(dev_sort(skey.as<u64>(), sidx.as<u32>(), n_single, 1, S.pos_bits, stream));
    // (the contigs one rank walks may hold more edges than its share: the records travel in rounds below 2^32 each, as many
    // rounds on every rank)
    const uint64_t round_max = 1ull << 31;
    uint64_t rounds = (n_rec + round_max - 1) / round_max;
    KCHECK(d->comm->allreduce(&rounds, 1, OP_MAX));
    KCHECK(S.reset());
    for (uint64_t t = 0; t < rounds; ++t) {
        const uint64_t at = std::min(n_rec, t * round_max), cnt = std::min(n_rec - at, round_max);
        Routed r(stream);
        KCHECK(S.router.send(A.as<u64>() + at, B.as<u64>() + at, cnt, r));
        if (r.n) {
            DevBuf q(stream), found(stream);
            KCHECK(q.alloc((r.n + 1) * 8)); KCHECK(found.alloc((r.n + 1) * 8));
            KLAUNCH(strip_kernel, r.n, stream, r.a.as<u64>(), r.n, q.as<u64>());
            if (n_single) KCHECK(dev_rank(skey.as<u64>(), n_single, 1, S.pos_bits, q.as<u64>(), r.n, found.as<u64>(), stream));
            else KCHECK_HIP(hipMemsetAsync(found.p, 0xFF, r.n * 8, stream));
            KLAUNCH(mean_apply_kernel, r.n, stream, found.as<u64>(), r.b.as<u64>(), r.n, sidx.as<u32>(), b->edge_weight.as<u32>(), S.cur() + 7);
            KCHECK_HIP(hipGetLastError());
        }
    }
    A.release(); B.release();
    KCHECK(S.agree_clean("a contig's mean names a node that is not a single-out-edge node of its owner"));
    return KATOME_OK;
}

}  // namespace

extern "C" {

int katome_dist_prune_weak_edges(katome_dist_builder* d, uint32_t threshold, katome_dist_graph* out, void* stream_) {
    KCHECK(check_builder(d, "katome_dist_prune_weak_edges"));
    hipStream_t stream = (hipStream_t)stream_;
    KCHECK_HIP(hipSetDevice(d->s.device));
    d->comm->use_stream(stream);
    KCHECK(check_sizes(d));
    KCHECK(prune_weak(d, threshold, stream));
    return katome_dist_current_graph(d, out);
}

int katome_dist_standardize_edges(katome_dist_builder* d, uint64_t original_genome_length, uint32_t threshold, katome_dist_graph* out, void* stream_) {
    KCHECK(check_builder(d, "katome_dist_standardize_edges"));
    hipStream_t stream = (hipStream_t)stream_;
    KCHECK_HIP(hipSetDevice(d->s.device));
    d->comm->use_stream(stream);
    KCHECK(check_sizes(d));
    const uint32_t k = d->s.k;
    {
        uint64_t bad = original_genome_length < k ? 1 : 0;
        KCHECK(d->comm->allreduce(&bad, 1, OP_MAX));
        if (bad) { set_error("standardize_edges: original_genome_length < k"); return KATOME_E_ARG; }
    }
    // standardize.hip's sums and scaling; the sums of all ranks in between, so every rank computes the same p bit for bit
    const uint64_t E = d->n_edges;
    u32* weight = d->b->edge_weight.as<u32>();
    uint64_t h[2] = {0, 0};
    KCHECK(dev_weight_sums(weight, E, threshold, h, stream));
    KCHECK(d->comm->allreduce(h, 2, OP_SUM));
    if (d->total_edges)                                     // (the one-GPU form leaves an empty graph as it is)
        KCHECK(dev_scale_weights(weight, E, standardization_ratio(original_genome_length, k, h), threshold, stream));
    KCHECK(prune_weak(d, 1, stream));                       // "remove edges with weight 0" (standardizer.rs:68-69)
    return katome_dist_current_graph(d, out);
}

}  // extern "C"
