// collapse_exact.h -- Collapsable::collapse for PtGraph exactly as the reference computes it (src/katome/algorithms/collapser.rs:25-273),
// after its first line: `self.shrink()` is ShrinkExact::run, and this file starts from the state that leaves in host memory.  What
// follows there is a walk that consumes edge weights one at a time and swap-removes edges and nodes as it goes -- which contigs come
// out, and in which order, is a function of petgraph 0.4.13's indices and adjacency order at every step, so it is restated
// sequentially over the same layout (ShrinkExact's arrays and its remove_edge).  The walk does not build strings: it emits PIECES --
// piece p names the shrunk edge appended at step p by its identity (its index in the shrunk graph before the walk), with one flag
// bit on a piece that begins a contig (EdgeSlice::name(), the whole label; every other piece is remainder(), the label from base
// k-1 on).  The text is the device's (collapse.hip).
// Host-only, no HIP: included by collapse.hip and by tests/hostshim (checked there against the oracle on hand-made graphs).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "shrink_exact.h"

namespace katome {

struct CollapseExact {
    static constexpr uint32_t END = ShrinkExact::END;
    static constexpr uint32_t WHOLE = 0x80000000u;         // flag bit of a piece that begins a contig; identities stay below it
    ShrinkExact& g;                                        // petgraph's layout; edge_slot[e] holds the IDENTITY of edge e from prepare() on
    std::vector<uint32_t> slot_of;                         // identity -> the slot (original edge) ShrinkExact gave the shrunk edge
    std::vector<uint32_t> weight;                          // identity -> what is left of its EdgeWeight
    std::vector<uint8_t> ambiguous;                        // FixedBitSet::with_capacity(node_count) (collapser.rs:33): never shrinks
    std::vector<uint32_t> single;                          // single_vertices
    // every node without incoming edges is in `cand` (with stale and repeated entries): the externals of a round are its entries that
    // still are such nodes, ascending -- the same nodes in the same order as a scan of all nodes gives (literal_externals: that scan)
    std::vector<uint32_t> cand, externals;
    bool literal_externals = false;
    // tarjan_scc
    std::vector<uint32_t> scc_index, scc_low, scc_stack;
    std::vector<uint8_t> scc_on_stack;
    struct Frame { uint32_t v, e; };
    std::vector<Frame> scc_calls;
    // ---- output ----
    uint32_t* pieces = nullptr;
    uint64_t n_pieces = 0, cap_pieces = 0, n_contigs = 0;
    bool overflow = false;
    // ---- statistics ----
    uint64_t steps = 0, ambiguity_cuts = 0, self_loops = 0, simple_loops = 0, scc_restarts = 0, nodes_removed = 0;
    uint64_t ambiguity_moves = 0;                          // removals that copied a SET bit of the last node onto a lower index

    explicit CollapseExact(ShrinkExact& graph) : g(graph) {}

    // the number of pieces the walk will emit: every decrement emits one and the loop ends on an empty graph
    static uint64_t piece_count(const uint32_t* shrunk_weight, uint32_t n_edges) {
        uint64_t s = 0;
        for (uint32_t e = 0; e < n_edges; ++e) s += shrunk_weight[e];
        return s;
    }

    // remove_single_vertices (shrinker.rs:172) applied to the node arrays: ShrinkExact::run re-numbered edge_node only.  kept[i] = the
    // old index of node i (retain_nodes: indices descending, swap_remove)
    void compact_nodes(const std::vector<uint32_t>& kept) {
        for (int d = 0; d < 2; ++d) {
            std::vector<uint32_t> next(kept.size());
            for (size_t i = 0; i < kept.size(); ++i) next[i] = g.node_next[d][kept[i]];
            g.node_next[d].swap(next);
        }
        g.n_nodes = (uint32_t)kept.size();
    }
    // shrunk_weight[e] = weight of edge e of the shrunk graph; `out` has room for piece_count() pieces
    void prepare(const std::vector<uint32_t>& kept, const uint32_t* shrunk_weight, uint32_t* out, uint64_t cap) {
        compact_nodes(kept);
        slot_of.assign(g.edge_slot.begin(), g.edge_slot.begin() + g.n_edges);
        weight.assign(shrunk_weight, shrunk_weight + g.n_edges);
        for (uint32_t e = 0; e < g.n_edges; ++e) g.edge_slot[e] = e;
        ambiguous.assign(g.n_nodes, 0);
        single.clear(); cand.clear();
        for (uint32_t n = 0; n < g.n_nodes; ++n) if (g.node_next[1][n] == END) cand.push_back(n);
        pieces = out; cap_pieces = cap; n_pieces = n_contigs = 0; overflow = false;
    }

    uint32_t degree(uint32_t n, int d) const {
        uint32_t c = 0;
        for (uint32_t e = g.node_next[d][n]; e != END; e = g.edge_next[d][e]) ++c;
        return c;
    }
    void remove_edge(uint32_t e) {
        const uint32_t target = g.edge_node[1][e];
        g.remove_edge(e);
        if (g.node_next[1][target] == END) cand.push_back(target);
    }
    // Graph::remove_node: every edge of both lists first, then swap_remove and re-point the moved node's edges
    void remove_node(uint32_t a) {
        if (a >= g.n_nodes) return;
        for (int d = 0; d < 2; ++d) while (g.node_next[d][a] != END) remove_edge(g.node_next[d][a]);
        const uint32_t last = --g.n_nodes;
        ++nodes_removed;
        if (a == last) return;
        for (int d = 0; d < 2; ++d) {
            g.node_next[d][a] = g.node_next[d][last];
            for (uint32_t e = g.node_next[d][a]; e != END; e = g.edge_next[d][e]) g.edge_node[d][e] = a;
        }
        if (g.node_next[1][a] == END) cand.push_back(a);
    }
    // remove_single_with_ambiguity (collapser.rs:84-96)
    void remove_single_with_ambiguity() {
        std::sort(single.begin(), single.end(), [](uint32_t a, uint32_t b) { return a > b; });
        uint32_t last_node = g.n_nodes;
        for (const uint32_t node : single) {
            last_node -= 1;
            const uint8_t bit = last_node < ambiguous.size() ? ambiguous[last_node] : 0;      // copy_bit(last_node, node)
            if (bit && node < last_node) ++ambiguity_moves;
            ambiguous[node] = bit;
            remove_node(node);
        }
        single.clear();
    }

    // self_loop (collapser.rs:215-225)
    uint32_t self_loop(uint32_t node) const {
        if (degree(node, 1) > 2) return END;
        for (uint32_t e = g.node_next[0][node]; e != END; e = g.edge_next[0][e]) if (g.edge_node[1][e] == g.edge_node[0][e]) return e;
        return END;
    }
    // simple_loop (collapser.rs:235-259)
    uint32_t simple_loop(uint32_t edge) const {
        const uint32_t source = g.edge_node[0][edge], target = g.edge_node[1][edge];
        const uint32_t in_source = degree(source, 1);
        if (in_source == 0 || in_source > 2) return END;
        if (degree(target, 1) != 1 || degree(target, 0) != 2) return END;
        for (uint32_t e = g.node_next[0][target]; e != END; e = g.edge_next[0][e])
            if (g.edge_node[1][e] == source && weight[g.edge_slot[e]] < weight[g.edge_slot[edge]]) return e;
        return END;
    }
    // decrease_weight (collapser.rs:262-273)
    void decrease_weight(uint32_t edge) {
        uint32_t& w = weight[g.edge_slot[edge]];
        w -= 1;
        if (w > 0) return;
        remove_edge(edge);
    }
    void emit(uint32_t edge, bool whole) {
        if (n_pieces >= cap_pieces) { overflow = true; ++n_pieces; return; }
        pieces[n_pieces++] = g.edge_slot[edge] | (whole ? WHOLE : 0u);
        n_contigs += whole;
    }

    // contigs_from_vertex (collapser.rs:99-205); `open` = !contig.is_empty(): a contig that is pushed ends where the next whole piece begins
    void contigs_from_vertex(uint32_t v) {
        bool open = false;
        uint32_t current_vertex = v;
        uint32_t num_in = degree(current_vertex, 1), num_out = degree(current_vertex, 0);
        for (;;) {
            uint32_t simple_loop_ = END;
            if (num_out == 0) {
                if (num_in == 0) single.push_back(current_vertex);
                return;
            }
            uint32_t current_edge_index = g.node_next[0][current_vertex];      // first_edge(current_vertex, Outgoing)
            bool cut = false;
            if (ambiguous[current_vertex]) {
                cut = true;
            } else if (num_in == 2 && num_out == 1) {
                if (self_loop(current_vertex) == END) {
                    simple_loop_ = simple_loop(current_edge_index);
                    if (simple_loop_ == END) { ambiguous[current_vertex] = 1; cut = true; }
                }
            } else if ((num_in == 1 || num_in == 2) && num_out == 2) {
                const uint32_t e = self_loop(current_vertex);
                if (e != END) { current_edge_index = e; ++self_loops; }
                else { ambiguous[current_vertex] = 1; cut = true; }
            } else if ((num_in == 0 || num_in == 1) && num_out == 1) {
            } else {
                ambiguous[current_vertex] = 1; cut = true;
            }
            if (cut && open) { open = false; ++ambiguity_cuts; }
            emit(current_edge_index, !open);
            open = true;
            ++steps;
            const uint32_t target = g.edge_node[1][current_edge_index];
            num_in = degree(target, 1);
            if (simple_loop_ != END) {
                emit(simple_loop_, false);
                ++simple_loops;
                if (current_edge_index < simple_loop_) { decrease_weight(simple_loop_); decrease_weight(current_edge_index); }   // the higher index first
                else { decrease_weight(current_edge_index); decrease_weight(simple_loop_); }
            } else {
                decrease_weight(current_edge_index);
            }
            num_out = degree(target, 0);
            if (g.isolated(current_vertex)) single.push_back(current_vertex);
            current_vertex = target;
        }
    }

    // tarjan_scc(&graph).iter().last()[0] (collapser.rs:63; petgraph 0.4.13 algo::tarjan_scc): nodes are visited in index order,
    // neighbours in outgoing-list order (newest edge first), an SCC is emitted when its root finishes, its nodes in pop order.  The
    // reference recurses; this keeps its frames (node, next edge to look at) on a vector, so a long cycle costs memory, not stack.
    uint32_t last_scc_first_node() {
        const uint32_t N = g.n_nodes;
        scc_index.assign(N, END); scc_low.resize(N); scc_on_stack.assign(N, 0);
        scc_stack.clear(); scc_calls.clear();
        uint32_t counter = 0, result = END;
        for (uint32_t root = 0; root < N; ++root) {
            if (scc_index[root] != END) continue;
            scc_index[root] = scc_low[root] = counter++; scc_stack.push_back(root); scc_on_stack[root] = 1;
            scc_calls.push_back({root, g.node_next[0][root]});
            while (!scc_calls.empty()) {
                const uint32_t v = scc_calls.back().v, e = scc_calls.back().e;
                if (e != END) {
                    scc_calls.back().e = g.edge_next[0][e];
                    const uint32_t w = g.edge_node[1][e];
                    if (scc_index[w] == END) {
                        scc_index[w] = scc_low[w] = counter++; scc_stack.push_back(w); scc_on_stack[w] = 1;
                        scc_calls.push_back({w, g.node_next[0][w]});
                    } else if (scc_on_stack[w]) {
                        scc_low[v] = std::min(scc_low[v], scc_index[w]);
                    }
                    continue;
                }
                scc_calls.pop_back();
                if (scc_low[v] == scc_index[v]) {
                    result = scc_stack.back();                     // the SCC's first node in pop order
                    for (;;) { const uint32_t w = scc_stack.back(); scc_stack.pop_back(); scc_on_stack[w] = 0; if (w == v) break; }
                }
                if (!scc_calls.empty()) { const uint32_t p = scc_calls.back().v; scc_low[p] = std::min(scc_low[p], scc_low[v]); }
            }
        }
        return result;
    }

    void collect_externals() {
        externals.clear();
        if (literal_externals) {
            for (uint32_t n = 0; n < g.n_nodes; ++n) if (g.node_next[1][n] == END) externals.push_back(n);
            return;
        }
        std::sort(cand.begin(), cand.end());
        cand.erase(std::unique(cand.begin(), cand.end()), cand.end());
        for (const uint32_t n : cand) if (n < g.n_nodes && g.node_next[1][n] == END) externals.push_back(n);
        cand = externals;                                          // (those that survive the round are externals of the next one)
    }

    // Collapsable::collapse (collapser.rs:36-74).  false: the walk stopped without emptying the graph (a round that neither emitted
    // a piece nor removed a node: cannot happen on a graph whose weights are all positive) or ran out of room for its pieces
    bool run() {
        for (;;) {
            for (;;) {
                collect_externals();
                if (externals.empty()) break;
                for (size_t i = 0; i < externals.size(); ++i) contigs_from_vertex(externals[i]);
                remove_single_with_ambiguity();
            }
            if (g.n_nodes == 0) break;
            const uint64_t before = n_pieces + nodes_removed;
            const uint32_t node_in_cycle = last_scc_first_node();
            ++scc_restarts;
            contigs_from_vertex(node_in_cycle);
            remove_single_with_ambiguity();
            if (n_pieces + nodes_removed == before) return false;
        }
        return !overflow;
    }
};

}  // namespace katome
