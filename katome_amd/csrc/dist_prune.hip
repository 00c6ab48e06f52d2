// dist_prune.hip -- Prunable::remove_dead_paths (pruner.rs:36-82) on the SHARDED graph, in the reference's numbering.
//
// After katome_dist_finalize (first-seen order) every rank holds the out-edges of the nodes it owns, each edge with its global
// petgraph index, its source as a LOCAL node and its target as (owner rank, local node there).  What the reference does per
// pass (check_dead_path 229-257 from every vertex without incoming edges, then remove_paths 199-217: swap_remove by
// descending index, remove_single_node after every edge) is cut along what depends on what:
//   * the WALKS follow first_edge(Outgoing) -- the live out-edge added last = largest first-seen index, which never changes
//     (swap_remove re-labels edges, petgraph's lists keep their order) -- for fewer than 2k steps.  A node's out-edges, its
//     degrees and its first out-edge are local to its owner; what a walk reads of a node -- its successor, whether it has an
//     out-edge, whether three or more edges come in -- is one word, and ONE WORD PER NODE OF THE WHOLE GRAPH fits every rank's
//     288 GB (C5 in full: 88 GB): the table is replicated, the words a pass changes are all-gathered, and the walks are the
//     one-GPU loop over a table.  Dead walks are walked a second time; every vertex they pass is a mark that goes to the
//     vertex's owner through a directory sharded by node id.  (Without room for the table: 16-byte walkers that hop from
//     owner to owner, one all-to-all per step, <= 2k - 1 steps.)
//   * the two INDEX REPLAYS (which edge / node sits where after every swap_remove) only involve the marked indices and the
//     tail positions that disappear -- O(what the pass removes), not O(graph).  They run on rank 0 with 64-bit positions
//     (prune.hip's scan + pointer jumping, templated on the index width): the ranks send their marked (position, count)
//     pairs, ask for the fate of their candidate edges (marked, or sitting in the vacated tail) and nodes, and apply the
//     answers -- an edge dies with its removal number or moves to a new position; nothing else of the graph moves.
//   * degrees are kept current incrementally (an out-edge's source is local, its target gets a message), "the removal that
//     touched a vertex last speaks for it" decides which removal takes an endpoint with it (prune.hip, death_emit_kernel).
// No gather: the graph stays sharded, and no index is narrower than 64 bits on the wire or in the replays, so a graph of
// more than 2^32 edges (BASELINE config 5 in full: 1.1e10) is in range; a rank's own share stays below 2^32 edges.
//
// The driver follows the kernels.  DistPrune holds one call's state (the persistent buffers, the Router, the running totals, the
// stats, the trace), Pass what one pass allocates and more than one step needs.  katome_dist_remove_dead_paths: setup,
// choose_walk_route [, setup_table], then per pass
//     walks                    first out-edges; share_changed_words + walks_on_table, or walks_by_hopping
//     collect_marks            allreduce: marks of all ranks (none: done); the marks -> rank 0
//     agree_on_edge_replay     rank 0: root_edge_replay; allreduce: removed edges, duplicates, rank 0's status
//     ask_edge_fates           candidates -> rank 0, two replies
//     apply_edge_fates
//     send_losses_and_dies     losses -> targets' owners; barrier allreduce; dies -> rank 0
//     agree_on_node_replay     rank 0: root_node_replay; allreduce: removed nodes, rank 0's status
//     ask_node_moves           candidates -> rank 0, one reply
// and install_result (one question to the targets' owners) and the sum of the stats (allreduce).  Every rank passes through
// exactly these collectives in this order.  Agreed between the ranks are the checks at the entry and a failure of rank 0's two
// replays; any other failure of one rank alone (an allocation, say) still leaves the others waiting: ADVICE.md.
#include <chrono>
#include <cstring>

#include "dist_route.h"

namespace {

// ---- set-up -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void run_start_kernel(const u64* __restrict__ lsrc, u64 E, u64 n_src, u64* __restrict__ start) {
    WLOOP(e, E + 1) {
        if (e < E) { if (e == 0 || lsrc[e - 1] != lsrc[e]) start[lsrc[e]] = e; }
        else if (e == E) start[n_src] = E;
    }
}
__global__ __launch_bounds__(BLOCK) void node_init_kernel(u64 N, u64 n_src, const u64* __restrict__ start, u32* __restrict__ outdeg, u32* __restrict__ indeg,
                                                          u32* __restrict__ last_touch, unsigned char* __restrict__ alive) {
    WLOOP(j, N) if (j < N) { outdeg[j] = j < n_src ? (u32)(start[j + 1] - start[j]) : 0u; indeg[j] = 0; last_touch[j] = 0; alive[j] = 1; }
}
// message to a target's owner: (owner rank << 56) | local index there
__global__ __launch_bounds__(BLOCK) void target_msg_kernel(const u64* __restrict__ drank, const u64* __restrict__ dlocal, u64 E, u64* __restrict__ out) {
    WLOOP(e, E) if (e < E) out[e] = (drank[e] << 56) | dlocal[e];
}
__global__ __launch_bounds__(BLOCK) void indeg_add_kernel(const u64* __restrict__ msg, u64 n, u32* indeg) {
    WLOOP(i, n) if (i < n) atomicAdd(&indeg[(u32)(msg[i] & LOW56)], 1u);
}
// first_edge(Outgoing) of every node with out-edges: the live edge of its run with the largest first-seen index
__global__ __launch_bounds__(BLOCK) void first_out_kernel(u64 n_src, const u64* __restrict__ start, const u64* __restrict__ age,
                                                          const unsigned char* __restrict__ alive_e, u32* __restrict__ first_out) {
    WLOOP(j, n_src) if (j < n_src) {
        u64 best = 0; u32 at = NONE32;
        for (u64 e = start[j]; e < start[j + 1]; ++e)
            if (alive_e[e] && (at == NONE32 || age[e] > best)) { best = age[e]; at = (u32)e; }
        first_out[j] = at;
    }
}

// ---- walks ------------------------------------------------------------------------------------------------------------
// walker: A = (rank of the node it stands on << 56) | (that node's local index << 8) | edges collected so far,
//         B = (start rank << 32) | start node's local index
__global__ __launch_bounds__(BLOCK) void input_kernel(u64 N, u64 my_rank, const u32* __restrict__ indeg, const u32* __restrict__ outdeg,
                                                      const unsigned char* __restrict__ alive, u64* __restrict__ A, u64* __restrict__ B,
                                                      unsigned long long* cursor) {
    WLOOP(j, N) {
        const bool is_in = j < N && alive[j] && indeg[j] == 0 && outdeg[j] > 0;      // Externals: Input (pruner.rs:181-183)
        const u64 at = wave_append(is_in, cursor);
        if (is_in) { A[at] = (my_rank << 56) | (j << 8); B[at] = (my_rank << 32) | j; }
    }
}
// one step of check_dead_path for every walker standing on one of this rank's nodes.  -> the walkers that go on (to the
// owner of the next node) and the verdicts of the walks that end dead: D = (start rank << 56) | (start local << 8) | edges
__global__ __launch_bounds__(BLOCK) void walk_step_kernel(const u64* __restrict__ A, const u64* __restrict__ B, u64 n, u32 arrived, u32 two_k,
                                                          const u32* __restrict__ indeg, const u32* __restrict__ outdeg, const u32* __restrict__ first_out,
                                                          const u64* __restrict__ drank, const u64* __restrict__ dlocal,
                                                          u64* __restrict__ oA, u64* __restrict__ oB, unsigned long long* n_out,
                                                          u64* __restrict__ dead, unsigned long long* n_dead) {
    WLOOP(i, n) {
        bool go = false, die = false;
        u64 a = 0, b = 0, steps = 0, nextA = 0;
        if (i < n) {
            a = A[i]; b = B[i];
            const u32 v = (u32)((a & LOW56) >> 8);
            steps = a & 0xFF;
            if (arrived && indeg[v] >= 3) die = true;                       // neighbors_directed(.., Incoming).nth(2) (pruner.rs:253)
            else if (steps + 1 >= two_k) { /* cnt >= 2K: not a dead path (pruner.rs:235-239) */ }
            else if (outdeg[v] == 0) die = true;                            // no first_edge: the path ends here (248-251)
            else {
                const u32 e = first_out[v];
                go = true;
                nextA = (drank[e] << 56) | (dlocal[e] << 8) | (steps + 1);
            }
        }
        const u64 at = wave_append(go, n_out);
        if (go) { oA[at] = nextA; oB[at] = b; }
        const u64 dt = wave_append(die, n_dead);
        if (die) dead[dt] = ((b >> 32) << 56) | ((b & 0xFFFFFFFFull) << 8) | steps;
    }
}
// the second walk of a dead path: its edges are collected (a count per edge: two walks may share a trunk), `left` more to go
__global__ __launch_bounds__(BLOCK) void mark_step_kernel(const u64* __restrict__ M, u64 n, const u32* __restrict__ first_out,
                                                          const u64* __restrict__ drank, const u64* __restrict__ dlocal, u32* mult,
                                                          u64* __restrict__ oM, unsigned long long* n_out) {
    WLOOP(i, n) {
        bool go = false; u64 next = 0;
        if (i < n) {
            const u64 m = M[i], left = m & 0xFF;
            if (left) {
                const u32 v = (u32)((m & LOW56) >> 8), e = first_out[v];
                atomicAdd(&mult[e], 1u);
                if (left > 1) { go = true; next = (drank[e] << 56) | (dlocal[e] << 8) | (left - 1); }
            }
        }
        const u64 at = wave_append(go, n_out);
        if (go) oM[at] = next;
    }
}

// ---- walks on a REPLICATED successor table ------------------------------------------------------------------------------
// 288 GB of HBM per MI355X: one 8-byte word per node of the WHOLE graph -- successor along the first out-edge, "has an
// out-edge", in-degree saturated at 3, alive -- fits every rank (C3/C4: 12.6 GB; C5 in full: 88 GB), indexed by the node's
// first-seen id, which never changes.  With it a walk is local (the one-GPU kernel's loop over a table), and a pass needs a
// handful of collectives instead of two per walk step: the words that changed are all-gathered (O(what the pass removed)),
// the marks of the dead walks travel to their edges' owners through a directory sharded by node id.
constexpr u64 RW_SUCC = (1ull << 40) - 1, RW_HAS_OUT = 1ull << 40, RW_ALIVE = 1ull << 43;
constexpr u32 RW_INDEG_SHIFT = 41;
__global__ __launch_bounds__(BLOCK) void own_words_kernel(u64 N, u64 n_src, const u32* __restrict__ first_out, const u64* __restrict__ edst,
                                                          const u32* __restrict__ indeg, const unsigned char* __restrict__ alive, u64* __restrict__ out) {
    WLOOP(j, N) if (j < N) {
        u64 w = 0;
        if (alive[j]) {
            const u32 fo = j < n_src ? first_out[j] : NONE32;
            const u32 in = indeg[j] < 3u ? indeg[j] : 3u;
            w = RW_ALIVE | ((u64)in << RW_INDEG_SHIFT) | (fo != NONE32 ? (RW_HAS_OUT | (edst[fo] & RW_SUCC)) : RW_SUCC);
        }
        out[j] = w;
    }
}
// the words that differ from what the other ranks hold: {node id, word}
__global__ __launch_bounds__(BLOCK) void delta_kernel(u64 N, const u64* __restrict__ now, u64* __restrict__ held, const u64* __restrict__ gid,
                                                      u64* __restrict__ out, unsigned long long* cursor) {
    TLOOP(t0, N) {
        u64 w[CA_ITEMS]; u32 mine = 0, have = 0;
#pragma unroll
        for (int k = 0; k < CA_ITEMS; ++k) {
            const u64 j = t0 + (u64)k * BLOCK + threadIdx.x;
            if (j < N) { w[k] = now[j]; if (w[k] != held[j]) { have |= 1u << k; ++mine; } }
        }
        u64 at = block_append(mine, cursor);
#pragma unroll
        for (int k = 0; k < CA_ITEMS; ++k) if (have & (1u << k)) {
            const u64 j = t0 + (u64)k * BLOCK + threadIdx.x;
            out[2 * at] = gid[j]; out[2 * at + 1] = w[k]; held[j] = w[k]; ++at;
        }
    }
}
__global__ __launch_bounds__(BLOCK) void apply_words_kernel(const u64* __restrict__ list, u64 n, u64* __restrict__ table) {
    WLOOP(i, n) if (i < n) table[list[2 * i]] = list[2 * i + 1];
}
__global__ __launch_bounds__(BLOCK) void input_list_kernel(u64 N, const u32* __restrict__ indeg, const u32* __restrict__ outdeg,
                                                           const unsigned char* __restrict__ alive, u32* __restrict__ out, unsigned long long* cursor) {
    TLOOP(t0, N) {
        u32 mine = 0, have = 0;
#pragma unroll
        for (int k = 0; k < CA_ITEMS; ++k) {
            const u64 j = t0 + (u64)k * BLOCK + threadIdx.x;
            if (j < N && alive[j] && indeg[j] == 0 && outdeg[j] > 0) { have |= 1u << k; ++mine; }      // Externals: Input (pruner.rs:181-183)
        }
        u64 at = block_append(mine, cursor);
#pragma unroll
        for (int k = 0; k < CA_ITEMS; ++k) if (have & (1u << k)) out[at++] = (u32)(t0 + (u64)k * BLOCK + threadIdx.x);
    }
}
// check_dead_path (pruner.rs:229-257) from every listed vertex, on the replicated table: len[i] = edges of the dead path, 0 = not dead
__global__ __launch_bounds__(BLOCK) void walk_table_kernel(const u32* __restrict__ list, u64 n, const u64* __restrict__ gid, const u64* __restrict__ W,
                                                           u32 two_k, u32* __restrict__ len, unsigned long long* n_dead) {
    u32 dead = 0;
    WLOOP(i, n) if (i < n) {
        u64 cur = gid[list[i]];
        u32 steps = 0, L = 0;
        for (;;) {
            const u64 w = W[cur];
            if (steps && ((w >> RW_INDEG_SHIFT) & 3u) >= 3u) { L = steps; break; }     // nth(2) of the incoming neighbours (253-255)
            if (steps + 1 >= two_k) break;                                              // cnt >= 2K: kept (235-239)
            if (!(w & RW_HAS_OUT)) { L = steps; break; }                                // no first_edge (248-251)
            cur = w & RW_SUCC;
            ++steps;
        }
        len[i] = L;
        dead += L != 0;
    }
    if (dead) atomicAdd(n_dead, (unsigned long long)dead);
}
// the vertices a dead walk passes (their first out-edges are its edges), each addressed to the directory rank of its id
__global__ __launch_bounds__(BLOCK) void walk_marks_kernel(const u32* __restrict__ list, u64 n, const u64* __restrict__ gid, const u64* __restrict__ W,
                                                           const u32* __restrict__ len, const u64* __restrict__ offs, u64 per_rank, u64* __restrict__ out) {
    WLOOP(i, n) if (i < n) {
        const u32 L = len[i];
        u64 cur = gid[list[i]], at = offs[i];
        for (u32 s = 0; s < L; ++s) {
            out[at + s] = ((cur / per_rank) << 56) | cur;
            cur = W[cur] & RW_SUCC;
        }
    }
}
// directory: node id -> (owner rank << 56) | local index there
__global__ __launch_bounds__(BLOCK) void dir_msg_kernel(u64 N, u64 my_rank, const u64* __restrict__ gid, u64 per_rank, u64* __restrict__ A, u64* __restrict__ B) {
    WLOOP(j, N) if (j < N) { A[j] = ((gid[j] / per_rank) << 56) | gid[j]; B[j] = (my_rank << 56) | j; }
}
__global__ __launch_bounds__(BLOCK) void dir_fill_kernel(const u64* __restrict__ A, const u64* __restrict__ B, u64 n, u64 base, u64* __restrict__ dir) {
    WLOOP(i, n) if (i < n) dir[(A[i] & LOW56) - base] = B[i];
}
__global__ __launch_bounds__(BLOCK) void dir_forward_kernel(const u64* __restrict__ marks, u64 n, u64 base, const u64* __restrict__ dir, u64* __restrict__ out) {
    WLOOP(i, n) if (i < n) out[i] = dir[(marks[i] & LOW56) - base];
}
__global__ __launch_bounds__(BLOCK) void mark_nodes_kernel(const u64* __restrict__ msg, u64 n, const u32* __restrict__ first_out, u32* mult) {
    WLOOP(i, n) if (i < n) atomicAdd(&mult[first_out[(u32)(msg[i] & LOW56)]], 1u);
}

// ---- marks, candidates, answers -----------------------------------------------------------------------------------------
// (everything that goes to rank 0 carries rank 0 in the top byte: positions stay below 2^56)
__global__ __launch_bounds__(BLOCK) void marks_kernel(const u32* __restrict__ mult, const u64* __restrict__ pos, u64 E, u64* __restrict__ out_pos,
                                                      u64* __restrict__ out_mult, unsigned long long* cursor, unsigned long long* total) {
    u64 sum = 0;
    TLOOP(t0, E) {
        u32 m[CA_ITEMS], mine = 0;
#pragma unroll
        for (int k = 0; k < CA_ITEMS; ++k) {
            const u64 e = t0 + (u64)k * BLOCK + threadIdx.x;
            m[k] = e < E ? mult[e] : 0u;
            mine += m[k] != 0;
        }
        u64 at = block_append(mine, cursor);
#pragma unroll
        for (int k = 0; k < CA_ITEMS; ++k) if (m[k]) {
            const u64 e = t0 + (u64)k * BLOCK + threadIdx.x;
            out_pos[at] = pos[e]; out_mult[at] = m[k]; sum += m[k]; ++at;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_down(sum, o, 64);
    if ((threadIdx.x & 63) == 0 && sum) atomicAdd(total, (unsigned long long)sum);
}
// edges whose fate the replay decides: the marked ones and those in the tail [E_new, E) that disappears
__global__ __launch_bounds__(BLOCK) void edge_cand_kernel(const u32* __restrict__ mult, const u64* __restrict__ pos, const unsigned char* __restrict__ alive,
                                                          u64 E, u64 E_new, u64* __restrict__ q, u32* __restrict__ who, unsigned long long* cursor) {
    TLOOP(t0, E) {
        u64 p[CA_ITEMS]; u32 mine = 0, have = 0;
#pragma unroll
        for (int k = 0; k < CA_ITEMS; ++k) {
            const u64 e = t0 + (u64)k * BLOCK + threadIdx.x;
            if (e < E && alive[e]) { p[k] = pos[e]; if (mult[e] != 0 || p[k] >= E_new) { have |= 1u << k; ++mine; } }
        }
        u64 at = block_append(mine, cursor);
#pragma unroll
        for (int k = 0; k < CA_ITEMS; ++k) if (have & (1u << k)) { q[at] = p[k]; who[at] = (u32)(t0 + (u64)k * BLOCK + threadIdx.x); ++at; }
    }
}
__global__ __launch_bounds__(BLOCK) void node_cand_kernel(const u64* __restrict__ npos, const unsigned char* __restrict__ alive, u64 N, u64 N_new,
                                                          u64* __restrict__ q, u32* __restrict__ who, unsigned long long* cursor) {
    TLOOP(t0, N) {
        u64 p[CA_ITEMS]; u32 mine = 0, have = 0;
#pragma unroll
        for (int k = 0; k < CA_ITEMS; ++k) {
            const u64 j = t0 + (u64)k * BLOCK + threadIdx.x;
            if (j < N && alive[j]) { p[k] = npos[j]; if (p[k] >= N_new) { have |= 1u << k; ++mine; } }
        }
        u64 at = block_append(mine, cursor);
#pragma unroll
        for (int k = 0; k < CA_ITEMS; ++k) if (have & (1u << k)) { q[at] = p[k]; who[at] = (u32)(t0 + (u64)k * BLOCK + threadIdx.x); ++at; }
    }
}
// rank 0: answer[i] = table value at the query's place in the sorted key list, NONE64 if the query is not a key
__global__ __launch_bounds__(BLOCK) void answer_u32_kernel(const u64* __restrict__ found, u64 n, const u32* __restrict__ val, u64* __restrict__ out) {
    WLOOP(i, n) if (i < n) out[i] = found[i] == NONE64 ? NONE64 : (u64)val[found[i]];
}
__global__ __launch_bounds__(BLOCK) void answer_to_kernel(const u64* __restrict__ found, u64 n, const u32* __restrict__ idx, const u64* __restrict__ to, u64* __restrict__ out) {
    WLOOP(i, n) if (i < n) out[i] = found[i] == NONE64 ? NONE64 : to[idx[found[i]]];
}
// apply the edge answers: removal number (the edge dies: its source's degree and last touch here, a message to its target's
// owner) or new position
__global__ __launch_bounds__(BLOCK) void edge_apply_kernel(const u32* __restrict__ who, const u64* __restrict__ ord, const u64* __restrict__ newpos, u64 n,
                                                           u64 my_rank, u64* pos, unsigned char* alive_e, const u64* __restrict__ lsrc,
                                                           const u64* __restrict__ drank, const u64* __restrict__ dlocal, u32* outdeg, u32* last_touch,
                                                           u32* __restrict__ dead_e, u32* __restrict__ dead_t, u64* __restrict__ msgA, u64* __restrict__ msgB,
                                                           unsigned long long* n_dead) {
    WLOOP(i, n) {
        bool dies = false; u32 e = 0; u64 t = 0;
        if (i < n) {
            e = who[i];
            if (ord[i] != NONE64) { dies = true; t = ord[i]; }
            else if (newpos[i] != NONE64) pos[e] = newpos[i];
        }
        const u64 at = wave_append(dies, n_dead);
        if (dies) {
            alive_e[e] = 0;
            const u32 a = (u32)lsrc[e];
            atomicSub(&outdeg[a], 1u);
            atomicMax(&last_touch[a], (u32)t + 1u);
            const bool self = drank[e] == my_rank && dlocal[e] == (u64)a;     // (the target role never speaks for a self-loop, prune.hip)
            dead_e[at] = e; dead_t[at] = (u32)t;
            msgA[at] = (drank[e] << 56) | dlocal[e];
            msgB[at] = (t + 1) | (self ? (1ull << 32) : 0ull);
        }
    }
}
__global__ __launch_bounds__(BLOCK) void target_loss_kernel(const u64* __restrict__ msgA, const u64* __restrict__ msgB, u64 n, u32* indeg, u32* last_touch) {
    WLOOP(i, n) if (i < n) {
        const u32 b = (u32)(msgA[i] & LOW56);
        atomicSub(&indeg[b], 1u);
        atomicMax(&last_touch[b], (u32)(msgB[i] & 0xFFFFFFFFull));
    }
}
// which endpoints a removal takes with it: the removal that touched a node last speaks for it (source role here ...
__global__ __launch_bounds__(BLOCK) void die_src_kernel(const u32* __restrict__ dead_e, const u32* __restrict__ dead_t, u64 n, const u64* __restrict__ lsrc,
                                                        const u32* __restrict__ indeg, const u32* __restrict__ outdeg, const u32* __restrict__ last_touch,
                                                        const u64* __restrict__ npos, unsigned char* alive_n, u64* __restrict__ X, u64* __restrict__ Y,
                                                        unsigned long long* cursor) {
    WLOOP(i, n) {
        bool d = false; u32 a = 0; u64 t = 0;
        if (i < n) {
            a = (u32)lsrc[dead_e[i]]; t = dead_t[i];
            d = last_touch[a] == (u32)t + 1u && indeg[a] == 0 && outdeg[a] == 0;
        }
        const u64 at = wave_append(d, cursor);
        if (d) { X[at] = 2 * t; Y[at] = npos[a]; alive_n[a] = 0; }
    }
}
// ... target role at the target's owner)
__global__ __launch_bounds__(BLOCK) void die_dst_kernel(const u64* __restrict__ msgA, const u64* __restrict__ msgB, u64 n, const u32* __restrict__ indeg,
                                                        const u32* __restrict__ outdeg, const u32* __restrict__ last_touch, const u64* __restrict__ npos,
                                                        unsigned char* alive_n, u64* __restrict__ X, u64* __restrict__ Y, unsigned long long* cursor) {
    WLOOP(i, n) {
        bool d = false; u32 b = 0; u64 t1 = 0;
        if (i < n) {
            b = (u32)(msgA[i] & LOW56); t1 = msgB[i] & 0xFFFFFFFFull;
            d = !(msgB[i] >> 32) && last_touch[b] == (u32)t1 && indeg[b] == 0 && outdeg[b] == 0;
        }
        const u64 at = wave_append(d, cursor);
        if (d) { X[at] = 2 * (t1 - 1) + 1; Y[at] = npos[b]; alive_n[b] = 0; }
    }
}
// the last-touch marks are per pass: cleared where this pass set them, once every removal has spoken
__global__ __launch_bounds__(BLOCK) void untouch_src_kernel(const u32* __restrict__ dead_e, u64 n, const u64* __restrict__ lsrc, u32* last_touch) {
    WLOOP(i, n) if (i < n) last_touch[(u32)lsrc[dead_e[i]]] = 0;
}
__global__ __launch_bounds__(BLOCK) void untouch_dst_kernel(const u64* __restrict__ msgA, u64 n, u32* last_touch) {
    WLOOP(i, n) if (i < n) last_touch[(u32)(msgA[i] & LOW56)] = 0;
}
__global__ __launch_bounds__(BLOCK) void fill64_kernel(u64* __restrict__ p, u64 n, u64 v) { WLOOP(i, n) if (i < n) p[i] = v; }
__global__ __launch_bounds__(BLOCK) void scatter64_kernel(const u64* __restrict__ at, const u64* __restrict__ val, u64 n, u64* __restrict__ out) {
    WLOOP(i, n) if (i < n) out[at[i]] = val[i];
}
__global__ __launch_bounds__(BLOCK) void node_apply_kernel(const u32* __restrict__ who, const u64* __restrict__ newpos, u64 n, u64* npos) {
    WLOOP(i, n) if (i < n && newpos[i] != NONE64) npos[who[i]] = newpos[i];
}
__global__ __launch_bounds__(BLOCK) void clear_marks_kernel(const u32* __restrict__ who, u64 n, u32* mult) { WLOOP(i, n) if (i < n) mult[who[i]] = 0; }

__global__ __launch_bounds__(BLOCK) void npos_of_kernel(const u64* __restrict__ msg, u64 n, const u64* __restrict__ npos, u64* __restrict__ out) {
    WLOOP(i, n) if (i < n) out[i] = npos[(u32)(msg[i] & LOW56)];
}
__global__ __launch_bounds__(BLOCK) void gather_src_kernel(const u32* __restrict__ keep, u64 n, const u64* __restrict__ lsrc, const u64* __restrict__ npos, u64* __restrict__ out) {
    WLOOP(i, n) if (i < n) out[i] = npos[(u32)lsrc[keep[i]]];
}



// KATOME_DIST_PRUNE_FAIL=edges|nodes: rank 0's replay of that kind reports a failure in the first pass -- tests of "every rank
// leaves with the same error, nobody is left waiting in a collective"
static bool fail_at(const char* what) {
    const char* at = getenv("KATOME_DIST_PRUNE_FAIL");
    return at && !strcmp(at, what);
}
// what rank 0 could not do, as every rank's return value (rank 0 keeps its own message)
static int root_failed(int rank, int neg_status, const char* what) {
    if (rank != 0) set_error("distributed pruning: rank 0 failed in %s (status %d)", what, -neg_status);
    return -neg_status;
}

// ---- the driver: one call's state, a pass as named steps ----------------------------------------------------------------
// sections of the KATOME_DIST_PRUNE_TRACE line, in the order a pass goes through them
enum Section {
    S_BETWEEN,                                                                  // from one pass's last step to the next one's first (not printed)
    S_FIRST_OUT,
    S_WORDS_DELTA, S_ALLGATHER_APPLY, S_INPUT_LIST, S_WALK, S_SCAN_MARKS,       // the table route's walks
    S_WALKS_MARKS,                // hopping: the walks and their marks, all of them; on the table: the marks routed to their edges' owners
    S_MARKS_KERNEL, S_MARKS_SEND, S_SORT_REPLAY, S_EDGE_REPLAY,
    S_EDGE_QUESTIONS, S_APPLY_LOSSES, S_DIES_NODE_REPLAY, S_NODE_QUESTIONS,
    S_COUNT
};

// What a pass allocates and more than one step needs.  All of it goes at the end of the pass and nothing of it sooner, except
// rank 0's seven edge tables: released as soon as the edge questions are answered.
struct Pass {
    Routed marks;                                                // at rank 0: every rank's marked (position, count) pairs
    DevBuf victims, to_e, from_e, vict_sorted, vict_ord, from_sorted, from_idx;      // rank 0: the edge replay, as sorted tables to look up
    ReplayScratch sc;
    uint64_t m_removed = 0, E_new = 0, n_moves = 0, dups = 0;
    DevBuf q, who, ans_ord, ans_pos;                             // this rank's candidate edges: position, local index, the two answers
    uint64_t n_q = 0;
    DevBuf dead_e, dead_t, msgA, msgB;                           // its edges that die, their removal numbers, the messages to their targets' owners
    uint64_t n_dead = 0;
    Routed losses;                                               // ... as they arrive here
    DevBuf X, Y;
    Routed dies;                                                 // at rank 0: (2 * removal + role, node position) of every endpoint that goes
    DevBuf to_n, from_n, nfrom_sorted, nfrom_idx;                // rank 0: the node replay
    uint64_t n_nmoves = 0, N_new = 0;
    explicit Pass(hipStream_t s)
        : marks(s), victims(s), to_e(s), from_e(s), vict_sorted(s), vict_ord(s), from_sorted(s), from_idx(s), sc(s), q(s), who(s), ans_ord(s), ans_pos(s),
          dead_e(s), dead_t(s), msgA(s), msgB(s), losses(s), X(s), Y(s), dies(s), to_n(s), from_n(s), nfrom_sorted(s), nfrom_idx(s) {}
};

struct DistPrune {
    katome_dist_builder* const d; katome_builder* const b; const hipStream_t stream;
    Router router;
    const int rank, world;
    const uint32_t nw, k, two_k;
    const uint64_t E, N, n_src;                       // this rank's share; its nodes [0, n_src) have out-edges
    const u64 *lsrc, *drank, *dlocal;                 // every edge's source as a local node, its target as (owner rank, local node there)
    const u64* edst;                                  // ... and as a first-seen node id (the call installs new arrays at the end)
    const uint64_t TN0, per_rank;                     // the directory and the marks are sharded by first-seen node id, per_rank ids each
    uint32_t pos_bits = 1;                            // positions (of edges and of nodes alike) fit this many bits: what rank 0's sorts and look-ups work on
    bool use_table = true;
    // ages: the first-seen index an edge was given never changes; `pos` / `npos` is where an edge / a node sits now
    DevBuf age, pos, alive_e, mult, start, npos, indeg, outdeg, first_out, last_touch, alive_n, cursors;
    DevBuf w_table, w_now, w_held, ngid0, dir;        // the table route: every rank's copy, this rank's words now / as the others hold them, ids, directory
    uint64_t TE, TN;                                  // edges and nodes of the whole graph, as the passes shrink it
    katome_prune_stats st;
    const bool trace;
    double t_sec[S_COUNT] = {0}, t_mark = 0;

    DistPrune(katome_dist_builder* d_, hipStream_t s, bool trace_)
        : d(d_), b(d_->b), stream(s), router(d_, s), rank(d_->rank()), world(d_->world()), nw(d_->nw), k(d_->s.k), two_k(2 * d_->s.k), E(d_->n_edges),
          N(d_->n_nodes), n_src(d_->n_src), lsrc(d_->edge_lsrc.as<u64>()), drank(d_->edge_drank.as<u64>()), dlocal(d_->edge_dlocal.as<u64>()),
          edst(d_->edge_dst.as<u64>()), TN0(d_->total_nodes), per_rank(std::max<uint64_t>(1, (TN0 + world - 1) / world)), age(s), pos(s), alive_e(s),
          mult(s), start(s), npos(s), indeg(s), outdeg(s), first_out(s), last_touch(s), alive_n(s), cursors(s), w_table(s), w_now(s), w_held(s), ngid0(s),
          dir(s), TE(d_->total_edges), TN(d_->total_nodes), trace(trace_) {
        memset(&st, 0, sizeof st);
        while (pos_bits < 64 && ((std::max(d->total_edges, d->total_nodes) + 1) >> pos_bits)) ++pos_bits;
    }
    // (synchronizes, so only under the trace)
    void lap(Section s) { if (trace) { (void)hipStreamSynchronize(stream); const double t = now_ms(); t_sec[s] += t - t_mark; t_mark = t; } }

    // ---- the three patterns --------------------------------------------------------------------------------------------
    // a launch that appends through cursors: they are reset, `launch` gets them, and the one or two counts it declares are read back
    template <class F> int counted(F launch, uint64_t* c0, uint64_t* c1 = nullptr) {
        KCHECK_HIP(hipMemsetAsync(cursors.p, 0, 64, stream));
        launch(cursors.as<unsigned long long>());
        KCHECK_HIP(hipGetLastError());
        uint64_t h[2] = {0, 0};
        KCHECK_HIP(hipMemcpyAsync(h, cursors.p, c1 ? 16 : 8, hipMemcpyDeviceToHost, stream));
        KCHECK_HIP(hipStreamSynchronize(stream));
        *c0 = h[0];
        if (c1) *c1 = h[1];
        return KATOME_OK;
    }
    // a column of n positions in ascending order, with where each stood: sorted[i] = col[idx[i]]
    int sorted_with_index(const DevBuf& col, uint64_t n, DevBuf& sorted, DevBuf& idx) {
        KCHECK(sorted.alloc((n + 1) * 8)); KCHECK(idx.alloc((n + 1) * 4));
        if (n) {
            KCHECK_HIP(hipMemcpyAsync(sorted.p, col.p, n * 8, hipMemcpyDeviceToDevice, stream));
            KLAUNCH(iota32_kernel, n, stream, idx.as<u32>(), n);
            KCHECK(dev_sort(sorted.as<u64>(), idx.as<u32>(), n, 1, pos_bits, stream));
        }
        return KATOME_OK;
    }
    // found[i] = where the i-th question stands in sorted[n], NONE64 if it is not there
    int rank_or_none(const DevBuf& sorted, uint64_t n, const Routed& asked, DevBuf& found) {
        if (n) KCHECK(dev_rank(sorted.as<u64>(), n, 1, pos_bits, asked.a.as<u64>(), asked.n, found.as<u64>(), stream));
        else KCHECK_HIP(hipMemsetAsync(found.p, 0xFF, asked.n * 8, stream));
        return KATOME_OK;
    }
    // ... and for a table of moves: out[i] = where what sits at the asked position goes, NONE64 if it stays
    int answer_moves(const DevBuf& from_sorted, const DevBuf& from_idx, const DevBuf& to, uint64_t n, const Routed& asked, DevBuf& found, DevBuf& out) {
        KCHECK(rank_or_none(from_sorted, n, asked, found));
        KLAUNCH(answer_to_kernel, asked.n, stream, found.as<u64>(), asked.n, from_idx.as<u32>(), to.as<u64>(), out.as<u64>());
        return KATOME_OK;
    }

    // ---- once per call ---------------------------------------------------------------------------------------------------
    // allocations, ages and positions, run starts, degrees (in-degrees: one message per edge to its target's owner; kept current afterwards)
    int setup() {
        KCHECK(router.init());
        KCHECK(age.alloc((E + 1) * 8)); KCHECK(pos.alloc((E + 1) * 8)); KCHECK(alive_e.alloc(E + 16)); KCHECK(mult.alloc((E + 1) * 4));
        KCHECK(start.alloc((n_src + 2) * 8));
        KCHECK(npos.alloc((N + 1) * 8)); KCHECK(indeg.alloc((N + 1) * 4)); KCHECK(outdeg.alloc((N + 1) * 4)); KCHECK(first_out.alloc((n_src + 1) * 4));
        KCHECK(last_touch.alloc((N + 1) * 4)); KCHECK(alive_n.alloc(N + 16)); KCHECK(cursors.alloc(64));
        if (E) {
            // (after a stage that removed edges the ages are kept in edge_age: a position is no age any more)
            KCHECK_HIP(hipMemcpyAsync(age.p, d->edge_age.p ? d->edge_age.p : d->edge_gid.p, E * 8, hipMemcpyDeviceToDevice, stream));
            KCHECK_HIP(hipMemcpyAsync(pos.p, d->edge_gid.p, E * 8, hipMemcpyDeviceToDevice, stream));
            KCHECK_HIP(hipMemsetAsync(alive_e.p, 1, E, stream));
            KCHECK_HIP(hipMemsetAsync(mult.p, 0, E * 4, stream));
        }
        KLAUNCH(run_start_kernel, E + 1, stream, lsrc, E, n_src, start.as<u64>());
        if (N) {
            KCHECK_HIP(hipMemcpyAsync(npos.p, d->node_gid.p, N * 8, hipMemcpyDeviceToDevice, stream));
            KLAUNCH(node_init_kernel, N, stream, N, n_src, start.as<u64>(), outdeg.as<u32>(), indeg.as<u32>(), last_touch.as<u32>(), alive_n.as<unsigned char>());
        }
        KCHECK_HIP(hipGetLastError());
        DevBuf msg(stream);
        KCHECK(msg.alloc((E + 1) * 8));
        if (E) KLAUNCH(target_msg_kernel, E, stream, drank, dlocal, E, msg.as<u64>());
        Routed r(stream);
        KCHECK(router.send(msg.as<u64>(), nullptr, E, r));
        if (r.n) KLAUNCH(indeg_add_kernel, r.n, stream, r.a.as<u64>(), r.n, indeg.as<u32>());
        KCHECK_HIP(hipGetLastError());
        return KATOME_OK;
    }
    // The walks: on a replicated successor table when every rank has room for one word per node of the whole graph (the
    // default), else walkers that hop from owner to owner (KATOME_DIST_PRUNE_WALKS=table|hop overrides; all ranks agree)
    int choose_walk_route() {
        size_t free_b = 0, total_b = 0;
        KCHECK_HIP(hipMemGetInfo(&free_b, &total_b));
        free_b += dev_cached_bytes();
        uint64_t ok = (TN0 + 1) * 8 + (N + 1) * 24 + per_rank * 8 + (4ull << 30) < free_b ? 1 : 0;
        if (const char* e = getenv("KATOME_DIST_PRUNE_WALKS")) ok = strcmp(e, "hop") == 0 ? 0 : strcmp(e, "table") == 0 ? 1 : ok;
        KCHECK(d->comm->allreduce(&ok, 1, OP_MIN));
        use_table = ok != 0;
        return KATOME_OK;
    }
    // the table route's words (all 0: no live node's word is, so the first pass sends them all) and its directory, sharded by node
    // id: where each node lives
    int setup_table() {
        KCHECK(w_table.alloc((TN0 + 1) * 8)); KCHECK(w_now.alloc((N + 1) * 8)); KCHECK(w_held.alloc((N + 1) * 8)); KCHECK(ngid0.alloc((N + 1) * 8));
        KCHECK(dir.alloc((per_rank + 1) * 8));
        KCHECK_HIP(hipMemsetAsync(w_table.p, 0, (TN0 + 1) * 8, stream));
        KCHECK_HIP(hipMemsetAsync(w_held.p, 0, (N + 1) * 8, stream));
        if (N) KCHECK_HIP(hipMemcpyAsync(ngid0.p, d->node_gid.p, N * 8, hipMemcpyDeviceToDevice, stream));
        DevBuf da(stream), db(stream);
        KCHECK(da.alloc((N + 1) * 8)); KCHECK(db.alloc((N + 1) * 8));
        if (N) KLAUNCH(dir_msg_kernel, N, stream, N, (u64)rank, ngid0.as<u64>(), per_rank, da.as<u64>(), db.as<u64>());
        Routed r(stream);
        KCHECK(router.send(da.as<u64>(), db.as<u64>(), N, r));
        if (r.n) KLAUNCH(dir_fill_kernel, r.n, stream, r.a.as<u64>(), r.b.as<u64>(), r.n, (u64)rank * per_rank, dir.as<u64>());
        KCHECK_HIP(hipGetLastError());
        KCHECK_HIP(hipStreamSynchronize(stream));
        return KATOME_OK;
    }

    // ---- the walks of a pass: every dead walk's edges counted in mult ------------------------------------------------------
    int walks() {
        lap(S_BETWEEN);
        if (n_src) KLAUNCH(first_out_kernel, n_src, stream, n_src, start.as<u64>(), age.as<u64>(), alive_e.as<unsigned char>(), first_out.as<u32>());
        lap(S_FIRST_OUT);
        if (use_table) {
            KCHECK(share_changed_words());
            KCHECK(walks_on_table());
        } else {
            KCHECK(walks_by_hopping());
        }
        lap(S_WALKS_MARKS);
        return KATOME_OK;
    }
    // the words of this rank's nodes that changed -> every rank's copy of the table
    int share_changed_words() {
        if (N) KLAUNCH(own_words_kernel, N, stream, N, n_src, first_out.as<u32>(), edst, indeg.as<u32>(), alive_n.as<unsigned char>(), w_now.as<u64>());
        DevBuf delta(stream), all_delta(stream);
        KCHECK(delta.alloc((N + 1) * 16));
        uint64_t n_mine = 0, n_delta = 0;
        KCHECK(counted([&](auto* c) { if (N) KLAUNCH_T(delta_kernel, N, stream, N, w_now.as<u64>(), w_held.as<u64>(), ngid0.as<u64>(), delta.as<u64>(), c); }, &n_mine));
        lap(S_WORDS_DELTA);
        KCHECK(router.allgather(delta.p, n_mine, 16, all_delta, &n_delta));
        if (n_delta) KLAUNCH(apply_words_kernel, n_delta, stream, all_delta.as<u64>(), n_delta, w_table.as<u64>());
        delta.release(); all_delta.release();
        lap(S_ALLGATHER_APPLY);
        return KATOME_OK;
    }
    // walks from every vertex without incoming edges, local; the vertices the dead ones pass -> the directory rank of each -> its
    // owner, where its first out-edge is counted
    int walks_on_table() {
        DevBuf inputs(stream), len(stream), offs(stream), marks(stream);
        KCHECK(inputs.alloc((N + 1) * 4));
        uint64_t n_in = 0, n_dead_walks = 0, n_marks = 0;
        KCHECK(counted([&](auto* c) { if (N) KLAUNCH_T(input_list_kernel, N, stream, N, indeg.as<u32>(), outdeg.as<u32>(), alive_n.as<unsigned char>(), inputs.as<u32>(), c); }, &n_in));
        st.walks += n_in;
        lap(S_INPUT_LIST);
        KCHECK(len.alloc((n_in + 1) * 4)); KCHECK(offs.alloc((n_in + 2) * 8));
        KCHECK(counted([&](auto* c) { if (n_in) KLAUNCH(walk_table_kernel, n_in, stream, inputs.as<u32>(), n_in, ngid0.as<u64>(), w_table.as<u64>(), two_k, len.as<u32>(), c); }, &n_dead_walks));
        st.dead_walks += n_dead_walks;
        lap(S_WALK);
        if (n_in) {
            KCHECK(dev_scan_counts(len.as<u32>(), n_in, offs.as<u64>(), stream));
            KCHECK_HIP(hipMemcpyAsync(&n_marks, offs.as<u64>() + n_in, 8, hipMemcpyDeviceToHost, stream));
            KCHECK_HIP(hipStreamSynchronize(stream));
        }
        KCHECK(marks.alloc((n_marks + 1) * 8));
        if (n_marks) KLAUNCH(walk_marks_kernel, n_in, stream, inputs.as<u32>(), n_in, ngid0.as<u64>(), w_table.as<u64>(), len.as<u32>(), offs.as<u64>(), per_rank, marks.as<u64>());
        KCHECK_HIP(hipGetLastError());
        lap(S_SCAN_MARKS);
        Routed at_dir(stream), at_owner(stream);
        KCHECK(router.send(marks.as<u64>(), nullptr, n_marks, at_dir));
        DevBuf fwd(stream);
        KCHECK(fwd.alloc((at_dir.n + 1) * 8));
        if (at_dir.n) KLAUNCH(dir_forward_kernel, at_dir.n, stream, at_dir.a.as<u64>(), at_dir.n, (u64)rank * per_rank, dir.as<u64>(), fwd.as<u64>());
        KCHECK_HIP(hipGetLastError());
        KCHECK(router.send(fwd.as<u64>(), nullptr, at_dir.n, at_owner));
        if (at_owner.n) KLAUNCH(mark_nodes_kernel, at_owner.n, stream, at_owner.a.as<u64>(), at_owner.n, first_out.as<u32>(), mult.as<u32>());
        KCHECK_HIP(hipGetLastError());
        return KATOME_OK;
    }
    // without room for the table: walkers hop from owner to owner, then the dead walks again from their start vertices to collect
    // their edges.  One exchange per step; its count matrix tells every rank whether any walker moved anywhere (no agreement round
    // of its own), so all ranks leave a loop after the same step
    int walks_by_hopping() {
        DevBuf A(stream), B(stream), deadv(stream);
        uint64_t n_deadv = 0;
        Routed arrivals(stream);
        KCHECK(hop_walks(A, B, arrivals, deadv, &n_deadv));
        st.dead_walks += n_deadv;
        return hop_marks(deadv, n_deadv);
    }
    int hop_walks(DevBuf& A, DevBuf& B, Routed& arrivals, DevBuf& deadv, uint64_t* n_deadv_out) {
        KCHECK(A.alloc((N + 1) * 8)); KCHECK(B.alloc((N + 1) * 8));
        uint64_t n_walk = 0, n_deadv = 0, deadv_cap = 0;
        KCHECK(counted([&](auto* c) { if (N) KLAUNCH(input_kernel, N, stream, N, (u64)rank, indeg.as<u32>(), outdeg.as<u32>(), alive_n.as<unsigned char>(), A.as<u64>(), B.as<u64>(), c); }, &n_walk));
        st.walks += n_walk;
        const u64 *wA = A.as<u64>(), *wB = B.as<u64>();
        for (uint32_t step = 0;; ++step) {
            if (step > two_k) { set_error("distributed pruning: a walk did not end within 2k steps"); return KATOME_E_DEVICE; }
            DevBuf oA(stream), oB(stream);
            KCHECK(oA.alloc((n_walk + 1) * 8)); KCHECK(oB.alloc((n_walk + 1) * 8));
            if (n_deadv + n_walk > deadv_cap) {                              // the verdicts collected on this rank so far + this step's
                DevBuf bigger(stream);
                deadv_cap = (n_deadv + n_walk) * 2 + 1024;
                KCHECK(bigger.alloc(deadv_cap * 8));
                if (n_deadv) KCHECK_HIP(hipMemcpyAsync(bigger.p, deadv.p, n_deadv * 8, hipMemcpyDeviceToDevice, stream));
                const size_t bytes = bigger.bytes;
                deadv.adopt(bigger.take(), bytes);
            }
            uint64_t n_go = 0, n_die = 0;
            if (n_walk) KCHECK(counted([&](auto* c) {
                KLAUNCH(walk_step_kernel, n_walk, stream, wA, wB, n_walk, step ? 1u : 0u, two_k, indeg.as<u32>(), outdeg.as<u32>(), first_out.as<u32>(),
                        drank, dlocal, oA.as<u64>(), oB.as<u64>(), c, deadv.as<u64>() + n_deadv, c + 1);
            }, &n_go, &n_die));
            n_deadv += n_die;
            KCHECK(router.send(oA.as<u64>(), oB.as<u64>(), n_go, arrivals));
            wA = arrivals.a.as<u64>(); wB = arrivals.b.as<u64>(); n_walk = arrivals.n;
            if (arrivals.moved == 0) break;
        }
        *n_deadv_out = n_deadv;
        return KATOME_OK;
    }
    int hop_marks(const DevBuf& deadv, uint64_t n_deadv) {
        Routed m(stream);
        KCHECK(router.send(deadv.as<u64>(), nullptr, n_deadv, m));
        const u64* wM = m.a.as<u64>();
        uint64_t n_m = m.n;
        Routed arrived(stream);
        for (uint32_t step = 0;; ++step) {
            if (step > two_k) { set_error("distributed pruning: a marking walk did not end within 2k steps"); return KATOME_E_DEVICE; }
            DevBuf oM(stream);
            KCHECK(oM.alloc((n_m + 1) * 8));
            uint64_t n_go = 0;
            if (n_m) KCHECK(counted([&](auto* c) {       // (synchronises: the list just walked may be given up below)
                KLAUNCH(mark_step_kernel, n_m, stream, wM, n_m, first_out.as<u32>(), drank, dlocal, mult.as<u32>(), oM.as<u64>(), c);
            }, &n_go));
            KCHECK(router.send(oM.as<u64>(), nullptr, n_go, arrived));
            wM = arrived.a.as<u64>(); n_m = arrived.n;
            if (arrived.moved == 0) break;
        }
        return KATOME_OK;
    }

    // ---- the edges of a pass ------------------------------------------------------------------------------------------------
    // this rank's marked (position, count) pairs; all ranks agree on how many there are in all.  None: "if to_remove.is_empty() ...
    // Graph is pruned" (pruner.rs:69-72), the caller leaves.  Else they go to rank 0 (top byte 0)
    int collect_marks(Pass& p, uint64_t* u_local, uint64_t* u_total) {
        DevBuf mp(stream), mm(stream);
        KCHECK(mp.alloc((E + 1) * 8)); KCHECK(mm.alloc((E + 1) * 8));
        uint64_t n_marked = 0;
        KCHECK(counted([&](auto* c) { if (E) KLAUNCH_T(marks_kernel, E, stream, mult.as<u32>(), pos.as<u64>(), E, mp.as<u64>(), mm.as<u64>(), c, c + 1); }, u_local, &n_marked));
        st.marked += n_marked;
        *u_total = *u_local;
        KCHECK(d->comm->allreduce(u_total, 1, OP_SUM));
        if (*u_total == 0) return KATOME_OK;
        lap(S_MARKS_KERNEL);
        KCHECK(router.send(mp.as<u64>(), mm.as<u64>(), *u_local, p.marks));
        lap(S_MARKS_SEND);
        mp.release(); mm.release();
        return KATOME_OK;
    }
    // rank 0 replays remove_paths' swap_removes: the victims by position with their removal numbers, the moves by where they come from
    int root_edge_replay(Pass& p) {
        const uint64_t u = p.marks.n;
        DevBuf m32(stream);
        KCHECK(m32.alloc((u + 1) * 4));
        KLAUNCH(narrow_kernel, u, stream, p.marks.b.as<u64>(), u, m32.as<u32>());
        KCHECK(dev_sort(p.marks.a.as<u64>(), m32.as<u32>(), u, 1, pos_bits, stream));
        KCHECK(dev_replay_edges64(p.marks.a.as<u64>(), m32.as<u32>(), u, TE, p.sc, p.victims, p.to_e, p.from_e, &p.m_removed, &p.E_new, &p.n_moves, &p.dups, stream));
        lap(S_SORT_REPLAY);
        if (p.m_removed >= 0xFFFFFFFFull) { set_error("more than 2^32 edges removed in one pass"); return KATOME_E_UNSUPPORTED; }
        KCHECK(sorted_with_index(p.victims, p.m_removed, p.vict_sorted, p.vict_ord));
        KCHECK(sorted_with_index(p.from_e, p.n_moves, p.from_sorted, p.from_idx));
        KCHECK_HIP(hipGetLastError());
        return KATOME_OK;
    }
    // What fails on rank 0 alone must not leave the others waiting in the next collective: its status travels with the counts every
    // rank agrees on, and all of them return it
    int agree_on_edge_replay(Pass& p) {
        p.E_new = TE;
        int root_rc = rank == 0 ? root_edge_replay(p) : KATOME_OK;
        if (rank == 0 && root_rc == KATOME_OK && fail_at("edges")) { set_error("distributed pruning: KATOME_DIST_PRUNE_FAIL=edges"); root_rc = KATOME_E_UNSUPPORTED; }
        lap(S_EDGE_REPLAY);
        uint64_t agreed[3] = {rank == 0 && root_rc == KATOME_OK ? TE - p.E_new : 0, rank == 0 ? p.dups : 0, (uint64_t)(-root_rc)};
        KCHECK(d->comm->allreduce(agreed, 3, OP_MAX));
        if (agreed[2]) return root_failed(rank, (int)agreed[2], "the replay of the removed edges");
        p.m_removed = agreed[0]; p.E_new = TE - p.m_removed;
        st.removed_edges += p.m_removed; st.removed_by_duplicates += agreed[1];
        return KATOME_OK;
    }
    // every rank asks for the fate of its candidate edges: its removal number if it dies, its new position if it moves
    int ask_edge_fates(Pass& p) {
        KCHECK(p.q.alloc((E + 1) * 8)); KCHECK(p.who.alloc((E + 1) * 4));
        KCHECK(counted([&](auto* c) {
            if (E) KLAUNCH_T(edge_cand_kernel, E, stream, mult.as<u32>(), pos.as<u64>(), alive_e.as<unsigned char>(), E, p.E_new, p.q.as<u64>(), p.who.as<u32>(), c);
        }, &p.n_q));
        KCHECK(p.ans_ord.alloc((p.n_q + 1) * 8)); KCHECK(p.ans_pos.alloc((p.n_q + 1) * 8));
        {
            Routed asked(stream);
            KCHECK(router.send(p.q.as<u64>(), nullptr, p.n_q, asked));
            DevBuf found(stream), a1(stream), a2(stream);
            KCHECK(found.alloc((asked.n + 1) * 8)); KCHECK(a1.alloc((asked.n + 1) * 8)); KCHECK(a2.alloc((asked.n + 1) * 8));
            if (asked.n) {                                                   // (rank 0 only)
                KCHECK(rank_or_none(p.vict_sorted, p.m_removed, asked, found));
                KLAUNCH(answer_u32_kernel, asked.n, stream, found.as<u64>(), asked.n, p.vict_ord.as<u32>(), a1.as<u64>());
                KCHECK(answer_moves(p.from_sorted, p.from_idx, p.to_e, p.n_moves, asked, found, a2));
                KCHECK_HIP(hipGetLastError());
            }
            KCHECK(router.reply(asked, a1.as<u64>(), p.ans_ord.as<u64>()));
            KCHECK(router.reply(asked, a2.as<u64>(), p.ans_pos.as<u64>()));
        }
        p.victims.release(); p.to_e.release(); p.from_e.release(); p.vict_sorted.release(); p.vict_ord.release(); p.from_sorted.release(); p.from_idx.release();
        lap(S_EDGE_QUESTIONS);
        return KATOME_OK;
    }
    // apply the answers: dead edges, their sources' degrees here, the messages for their targets' owners
    int apply_edge_fates(Pass& p) {
        const uint64_t n_q = p.n_q;
        KCHECK(p.dead_e.alloc((n_q + 1) * 4)); KCHECK(p.dead_t.alloc((n_q + 1) * 4)); KCHECK(p.msgA.alloc((n_q + 1) * 8)); KCHECK(p.msgB.alloc((n_q + 1) * 8));
        return counted([&](auto* c) {
            if (!n_q) return;
            KLAUNCH(edge_apply_kernel, n_q, stream, p.who.as<u32>(), p.ans_ord.as<u64>(), p.ans_pos.as<u64>(), n_q, (u64)rank, pos.as<u64>(), alive_e.as<unsigned char>(),
                    lsrc, drank, dlocal, outdeg.as<u32>(), last_touch.as<u32>(), p.dead_e.as<u32>(), p.dead_t.as<u32>(), p.msgA.as<u64>(), p.msgB.as<u64>(), c);
            KLAUNCH(clear_marks_kernel, n_q, stream, p.who.as<u32>(), n_q, mult.as<u32>());
        }, &p.n_dead);
    }

    // ---- the nodes of a pass ------------------------------------------------------------------------------------------------
    // the targets' owners learn of their losses; once every rank has applied every loss (the barrier), each removal's endpoints
    // that go with it -> rank 0
    int send_losses_and_dies(Pass& p) {
        const uint64_t n_dead = p.n_dead;
        Routed& losses = p.losses;
        KCHECK(router.send(p.msgA.as<u64>(), p.msgB.as<u64>(), n_dead, losses));
        if (losses.n) KLAUNCH(target_loss_kernel, losses.n, stream, losses.a.as<u64>(), losses.b.as<u64>(), losses.n, indeg.as<u32>(), last_touch.as<u32>());
        KCHECK_HIP(hipGetLastError());
        KCHECK_HIP(hipStreamSynchronize(stream));
        { uint64_t bar = 0; KCHECK(d->comm->allreduce(&bar, 1, OP_MAX)); }   // every rank has applied every loss before anyone decides who dies
        lap(S_APPLY_LOSSES);
        KCHECK(p.X.alloc((n_dead + losses.n + 1) * 8)); KCHECK(p.Y.alloc((n_dead + losses.n + 1) * 8));
        uint64_t n_dies = 0;
        KCHECK(counted([&](auto* c) {
            if (n_dead) KLAUNCH(die_src_kernel, n_dead, stream, p.dead_e.as<u32>(), p.dead_t.as<u32>(), n_dead, lsrc, indeg.as<u32>(), outdeg.as<u32>(), last_touch.as<u32>(),
                                npos.as<u64>(), alive_n.as<unsigned char>(), p.X.as<u64>(), p.Y.as<u64>(), c);
            if (losses.n) KLAUNCH(die_dst_kernel, losses.n, stream, losses.a.as<u64>(), losses.b.as<u64>(), losses.n, indeg.as<u32>(), outdeg.as<u32>(), last_touch.as<u32>(),
                                  npos.as<u64>(), alive_n.as<unsigned char>(), p.X.as<u64>(), p.Y.as<u64>(), c);
            if (n_dead) KLAUNCH(untouch_src_kernel, n_dead, stream, p.dead_e.as<u32>(), n_dead, lsrc, last_touch.as<u32>());
            if (losses.n) KLAUNCH(untouch_dst_kernel, losses.n, stream, losses.a.as<u64>(), losses.n, last_touch.as<u32>());
        }, &n_dies));
        return router.send(p.X.as<u64>(), p.Y.as<u64>(), n_dies, p.dies);
    }
    // rank 0 replays remove_single_node: the moves of the tail nodes that stay, by where they come from
    int root_node_replay(Pass& p) {
        const uint64_t m = p.m_removed;
        DevBuf die(stream);
        NodeReplayScratch nsc(stream);
        KCHECK(die.alloc((2 * m + 2) * 8));
        KLAUNCH(fill64_kernel, 2 * m, stream, die.as<u64>(), 2 * m, NONE64);
        if (p.dies.n) KLAUNCH(scatter64_kernel, p.dies.n, stream, p.dies.a.as<u64>(), p.dies.b.as<u64>(), p.dies.n, die.as<u64>());
        KCHECK_HIP(hipGetLastError());
        int fell_back = 0;      // (1: the pass's node moves chained further than the device form follows and were replayed on the host)
        const double t_replay = now_ms();
        KCHECK(dev_replay_nodes64(die.as<u64>(), m, TN, nsc, p.to_n, p.from_n, &p.n_nmoves, &p.N_new, &fell_back, stream));
        if (fell_back) st.host_ms += now_ms() - t_replay;
        KCHECK(sorted_with_index(p.from_n, p.n_nmoves, p.nfrom_sorted, p.nfrom_idx));
        KCHECK_HIP(hipGetLastError());
        return KATOME_OK;
    }
    // (rank 0's status travels as in agree_on_edge_replay)
    int agree_on_node_replay(Pass& p) {
        p.N_new = TN;
        int root_rc = rank == 0 ? root_node_replay(p) : KATOME_OK;
        if (rank == 0 && root_rc == KATOME_OK && fail_at("nodes")) { set_error("distributed pruning: KATOME_DIST_PRUNE_FAIL=nodes"); root_rc = KATOME_E_UNSUPPORTED; }
        lap(S_DIES_NODE_REPLAY);
        uint64_t removed_nodes[2] = {rank == 0 && root_rc == KATOME_OK ? TN - p.N_new : 0, (uint64_t)(-root_rc)};
        KCHECK(d->comm->allreduce(removed_nodes, 2, OP_MAX));
        if (removed_nodes[1]) return root_failed(rank, (int)removed_nodes[1], "the replay of the removed nodes");
        p.N_new = TN - removed_nodes[0];
        st.removed_nodes += removed_nodes[0];
        return KATOME_OK;
    }
    // the nodes in the vacated tail that stay ask where they go
    int ask_node_moves(Pass& p) {
        DevBuf nq(stream), nwho(stream), nans(stream);
        KCHECK(nq.alloc((N + 1) * 8)); KCHECK(nwho.alloc((N + 1) * 4));
        uint64_t n_nq = 0;
        KCHECK(counted([&](auto* c) { if (N) KLAUNCH_T(node_cand_kernel, N, stream, npos.as<u64>(), alive_n.as<unsigned char>(), N, p.N_new, nq.as<u64>(), nwho.as<u32>(), c); }, &n_nq));
        KCHECK(nans.alloc((n_nq + 1) * 8));
        Routed asked(stream);
        KCHECK(router.send(nq.as<u64>(), nullptr, n_nq, asked));
        DevBuf found(stream), a2(stream);
        KCHECK(found.alloc((asked.n + 1) * 8)); KCHECK(a2.alloc((asked.n + 1) * 8));
        if (asked.n) {
            KCHECK(answer_moves(p.nfrom_sorted, p.nfrom_idx, p.to_n, p.n_nmoves, asked, found, a2));
            KCHECK_HIP(hipGetLastError());
        }
        KCHECK(router.reply(asked, a2.as<u64>(), nans.as<u64>()));
        if (n_nq) KLAUNCH(node_apply_kernel, n_nq, stream, nwho.as<u32>(), nans.as<u64>(), n_nq, npos.as<u64>());
        KCHECK_HIP(hipGetLastError());
        return KATOME_OK;
    }
    void end_pass(const Pass& p) { TE = p.E_new; TN = p.N_new; lap(S_NODE_QUESTIONS); }

    void print_trace() const {
        if (!trace) return;
        fprintf(stderr, "[dist prune] rank %d router: %llu sends, %llu replies; host ms: partition %.1f, count rounds %.1f, exchanges %.1f\n", rank,
                (unsigned long long)router.n_send, (unsigned long long)router.n_reply, router.t_part, router.t_counts, router.t_xchg);
        // (S_WALKS_MARKS stands twice: as the walks' total where they hop, as the last part of the walks on the table)
        fprintf(stderr, "[dist prune] rank %d: %llu passes; ms: walks+marks %.1f, marks->root+edge replay %.1f, edge questions %.1f, apply+losses %.1f, "
                        "dies+node replay %.1f, node questions %.1f; of the second: marks kernel %.1f, send %.1f, sort+replay %.1f; walks: first_out %.1f, words+delta %.1f, allgather+apply %.1f, "
                        "input list %.1f, walk %.1f, scan+marks %.1f, marks routed %.1f\n", rank, (unsigned long long)st.passes, t_sec[S_WALKS_MARKS], t_sec[S_EDGE_REPLAY],
                t_sec[S_EDGE_QUESTIONS], t_sec[S_APPLY_LOSSES], t_sec[S_DIES_NODE_REPLAY], t_sec[S_NODE_QUESTIONS], t_sec[S_MARKS_KERNEL], t_sec[S_MARKS_SEND],
                t_sec[S_SORT_REPLAY], t_sec[S_FIRST_OUT], t_sec[S_WORDS_DELTA], t_sec[S_ALLGATHER_APPLY], t_sec[S_INPUT_LIST], t_sec[S_WALK], t_sec[S_SCAN_MARKS],
                t_sec[S_WALKS_MARKS]);
    }

    // ---- the pruned graph, still sharded: survivors compacted, positions as indices, ages kept -------------------------------
    // (block_append hands out places in no particular order: back into local order, which is key order)
    int in_local_order(DevBuf& keep, uint64_t n, DevBuf& k64) {
        if (n < 2) return KATOME_OK;
        KLAUNCH(widen_kernel, n, stream, keep.as<u32>(), n, k64.as<u64>());
        KCHECK(dev_sort(k64.as<u64>(), nullptr, n, 1, 32, stream));
        KLAUNCH(narrow_kernel, n, stream, k64.as<u64>(), n, keep.as<u32>());
        KCHECK_HIP(hipGetLastError());
        return KATOME_OK;
    }
    // the targets' indices, asked of their owners (all edges; the dead ones are dropped)
    int target_positions(const DevBuf& keep_e, uint64_t E2, DevBuf& e_dst) {
        DevBuf msg(stream), dst_all(stream), ans(stream);
        KCHECK(msg.alloc((E + 1) * 8)); KCHECK(dst_all.alloc((E + 1) * 8));
        if (E) KLAUNCH(target_msg_kernel, E, stream, drank, dlocal, E, msg.as<u64>());
        Routed asked(stream);
        KCHECK(router.send(msg.as<u64>(), nullptr, E, asked));
        KCHECK(ans.alloc((asked.n + 1) * 8));
        if (asked.n) KLAUNCH(npos_of_kernel, asked.n, stream, asked.a.as<u64>(), asked.n, npos.as<u64>(), ans.as<u64>());
        KCHECK_HIP(hipGetLastError());
        KCHECK(router.reply(asked, ans.as<u64>(), dst_all.as<u64>()));
        if (E2) KLAUNCH(gather_by_kernel<u64>, E2, stream, dst_all.as<u64>(), keep_e.as<u32>(), E2, e_dst.as<u64>());
        return KATOME_OK;
    }
    int install_result() {
        DevBuf keep_e(stream), keep_n(stream);
        KCHECK(keep_e.alloc((E + 1) * 4)); KCHECK(keep_n.alloc((N + 1) * 4));
        uint64_t E2 = 0, N2 = 0;
        KCHECK(counted([&](auto* c) {
            if (E) KLAUNCH_T(alive_list_kernel, E, stream, alive_e.as<unsigned char>(), E, keep_e.as<u32>(), c);
            if (N) KLAUNCH_T(alive_list_kernel, N, stream, alive_n.as<unsigned char>(), N, keep_n.as<u32>(), c + 1);
        }, &E2, &N2));
        {
            DevBuf k64(stream);
            KCHECK(k64.alloc((std::max(E2, N2) + 1) * 8));
            KCHECK(in_local_order(keep_e, E2, k64)); KCHECK(in_local_order(keep_n, N2, k64));
        }
        DevBuf n_key(stream), n_gid(stream), e_key(stream), e_w(stream), e_gid(stream), e_age(stream), e_src(stream), e_dst(stream);
        KCHECK(n_key.alloc((N2 + 1) * 8 * nw)); KCHECK(n_gid.alloc((N2 + 1) * 8));
        KCHECK(e_key.alloc((E2 + 1) * 8 * nw)); KCHECK(e_w.alloc((E2 + 1) * 4)); KCHECK(e_gid.alloc((E2 + 1) * 8)); KCHECK(e_age.alloc((E2 + 1) * 8));
        KCHECK(e_src.alloc((E2 + 1) * 8)); KCHECK(e_dst.alloc((E2 + 1) * 8));
        KCHECK(target_positions(keep_e, E2, e_dst));
        if (E2) {
            KLAUNCH(gather_src_kernel, E2, stream, keep_e.as<u32>(), E2, lsrc, npos.as<u64>(), e_src.as<u64>());
            KLAUNCH(gather_by_kernel<u64>, E2, stream, pos.as<u64>(), keep_e.as<u32>(), E2, e_gid.as<u64>());
            KLAUNCH(gather_by_kernel<u64>, E2, stream, age.as<u64>(), keep_e.as<u32>(), E2, e_age.as<u64>());
            KLAUNCH(gather_by_kernel<u32>, E2, stream, b->edge_weight.as<u32>(), keep_e.as<u32>(), E2, e_w.as<u32>());
            if (nw == 1) KLAUNCH(gather_keys_by_kernel<1>, E2, stream, b->edge_key.as<u64>(), keep_e.as<u32>(), E2, e_key.as<u64>());
            else         KLAUNCH(gather_keys_by_kernel<2>, E2, stream, b->edge_key.as<u64>(), keep_e.as<u32>(), E2, e_key.as<u64>());
        }
        if (N2) {
            KLAUNCH(gather_by_kernel<u64>, N2, stream, npos.as<u64>(), keep_n.as<u32>(), N2, n_gid.as<u64>());
            if (nw == 1) KLAUNCH(gather_keys_by_kernel<1>, N2, stream, d->node_key.as<u64>(), keep_n.as<u32>(), N2, n_key.as<u64>());
            else         KLAUNCH(gather_keys_by_kernel<2>, N2, stream, d->node_key.as<u64>(), keep_n.as<u32>(), N2, n_key.as<u64>());
        }
        KCHECK_HIP(hipGetLastError());
        KCHECK_HIP(hipStreamSynchronize(stream));
        auto install = [&](DevBuf& dst, DevBuf& src) { const size_t bytes = src.bytes; dst.stream = stream; dst.adopt(src.take(), bytes); };
        install(b->edge_key, e_key); install(b->edge_weight, e_w); install(d->edge_src, e_src); install(d->edge_dst, e_dst);
        install(d->edge_gid, e_gid); install(d->edge_age, e_age); install(d->node_key, n_key); install(d->node_gid, n_gid);
        b->edge_seq.release();
        d->edge_lsrc.release(); d->edge_drank.release(); d->edge_dlocal.release();      // (local indices of the unpruned share: stale now)
        KCHECK(d->edge_label.alloc((E2 + 1) * (size_t)label_stride_for_k(k) + 16, stream));
        KCHECK(dev_labels(b->edge_key.as<u64>(), E2, k, d->edge_label.as<uint8_t>(), stream));
        KCHECK_HIP(hipStreamSynchronize(stream));
        b->n_edges = E2;
        d->n_edges = E2; d->n_nodes = N2; d->total_edges = TE; d->total_nodes = TN; d->n_src = 0;
        d->dead_paths_removed = true;
        return KATOME_OK;
    }
};

}  // namespace

// The passes (the file's header has why they are cut this way).  Every rank goes through the same collectives in the same order:
// a step that only rank 0 can fail in hands its status to all of them in the agreement that follows it.
extern "C" int katome_dist_remove_dead_paths(katome_dist_builder* d, katome_dist_graph* out, katome_prune_stats* st_out, void* stream_) {
    if (!d) { set_error("null argument"); return KATOME_E_ARG; }
    if (!d->finalized || !d->first_seen) { set_error("katome_dist_remove_dead_paths: a finalized FIRST_SEEN_ORDER build only (petgraph's numbering decides what a repeated index removes)"); return KATOME_E_ARG; }
    if (d->gathered) { set_error("katome_dist_remove_dead_paths: the ranks' shares were gathered (katome_dist_gather); prune the gathered graph on its root"); return KATOME_E_ARG; }
    if (d->dead_paths_removed) {
        // Called again (the reference's pipeline does: asm/basic_assembler.rs:59,73): the first call ran to the fixpoint and nothing has
        // removed an edge or a node of the sharded graph since (a stage of dist_stages.hip that does clears the flag), so the
        // reference's loop would make one pass, find no dead path and leave (pruner.rs:69-72).  Every rank takes this branch: no
        // collective is needed.
        if (st_out) { memset(st_out, 0, sizeof *st_out); st_out->passes = 1; }
        return katome_dist_current_graph(d, out);
    }
    hipStream_t stream = (hipStream_t)stream_;
    KCHECK_HIP(hipSetDevice(d->s.device));
    d->comm->use_stream(stream);
    const double t_begin = now_ms();
    if (2 * d->s.k > 255) { set_error("k too large for the walker's step counter"); return KATOME_E_UNSUPPORTED; }       // (the same on every rank)
    {   // a rank whose share cannot be pruned says so to all of them: nobody may leave alone before a collective the others wait in
        uint64_t bad = (d->n_edges >= 0xFFFFFFFFull || d->n_nodes >= 0xFFFFFFFFull) ? 1 : 0;
        KCHECK(d->comm->allreduce(&bad, 1, OP_MAX));
        if (bad) { set_error("more than 2^32 edges or nodes on one rank"); return KATOME_E_UNSUPPORTED; }
    }
    {   // a stage of dist_stages.hip removed edges or nodes since the links were made: rebuild them (all ranks agree first)
        uint64_t stale = (!d->edge_lsrc.p || !d->edge_drank.p || !d->edge_dlocal.p) ? 1 : 0;
        KCHECK(d->comm->allreduce(&stale, 1, OP_MAX));
        if (stale) KCHECK(dist_rebuild_links(d, stream));
    }
    static const bool trace = getenv("KATOME_DIST_PRUNE_TRACE") != nullptr;
    DistPrune S(d, stream, trace);                    // (after the rebuild: the links and n_src are current)
    KCHECK(S.setup());
    KCHECK(S.choose_walk_route());
    if (S.use_table) KCHECK(S.setup_table());
    S.t_mark = now_ms();
    for (;;) {
        ++S.st.passes;
        Pass p(stream);
        uint64_t u_local = 0, u_total = 0;
        KCHECK(S.walks());                            // first out-edges; the walks, on the table or hopping; the dead walks' edges marked
        KCHECK(S.collect_marks(p, &u_local, &u_total));       // the marked (position, count) pairs, to rank 0 ...
        if (u_total == 0) break;                              // ... unless no rank has any: the graph is pruned
        KCHECK(S.agree_on_edge_replay(p));            // rank 0 replays the edge removals; all ranks agree on their number
        KCHECK(S.ask_edge_fates(p));                  // every rank's candidate edges: which die, which move where
        KCHECK(S.apply_edge_fates(p));
        KCHECK(S.send_losses_and_dies(p));            // losses to the targets' owners, the barrier, the endpoints that go to rank 0
        KCHECK(S.agree_on_node_replay(p));            // rank 0 replays the node removals; all ranks agree on their number
        KCHECK(S.ask_node_moves(p));                  // the tail nodes that stay: where they go
        S.end_pass(p);
    }
    S.print_trace();
    KCHECK(S.install_result());
    katome_prune_stats& st = S.st;
    {   // the walks and marks of all ranks
        uint64_t sums[3] = {st.walks, st.dead_walks, st.marked};
        KCHECK(d->comm->allreduce(sums, 3, OP_SUM));
        st.walks = sums[0]; st.dead_walks = sums[1]; st.marked = sums[2];
    }
    st.total_ms = now_ms() - t_begin;
    if (st_out) *st_out = st;
    return katome_dist_current_graph(d, out);
}

