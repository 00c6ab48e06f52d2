// C entry to katome_amd/csrc/collapse_exact.h and contig_stats.h for tests/test_collapse_exact_host.py and
// tests/test_contig_stats_host.py (no GPU)
#include <string.h>

#include "../../katome_amd/csrc/collapse_exact.h"
#include "../../katome_amd/csrc/contig_stats.h"
#include "../../katome_amd/csrc/multi_route.h"

// (n_nodes, edges in add order, weights) -> ShrinkExact, then the walk.  out_slot[i] = the original edge whose slot shrunk edge i
// (identity i) holds, chain_next the chains behind the slots; pieces has room for cap_pieces entries.
// counts = {shrunk edges, shrunk nodes, pieces, contigs, nodes left, edges left, steps, ambiguity cuts, self loops, simple loops,
//           SCC restarts, nodes removed, ambiguity moves, sum of the shrunk weights}
extern "C" int hs_collapse_exact(const uint32_t* src, const uint32_t* dst, const uint32_t* by_age, const uint32_t* weight, uint32_t E, uint32_t N,
                                 int literal_externals, uint32_t* pieces, uint64_t cap_pieces, uint32_t* out_slot, uint32_t* chain_next,
                                 uint64_t* counts) {
    katome::ShrinkExact s;
    s.init(src, dst, by_age, E, N);
    std::vector<uint32_t> kept;
    s.run(kept);
    const uint32_t H = s.n_edges;
    std::vector<uint32_t> w(H);
    for (uint32_t e = 0; e < H; ++e) { out_slot[e] = s.edge_slot[e]; w[e] = weight[s.edge_slot[e]]; }
    if (E) memcpy(chain_next, s.chain_next.data(), (size_t)E * 4);
    const uint64_t want = katome::CollapseExact::piece_count(w.data(), H);
    katome::CollapseExact c(s);
    c.literal_externals = literal_externals != 0;
    c.prepare(kept, w.data(), pieces, cap_pieces);
    const bool ok = c.run();
    counts[0] = H; counts[1] = kept.size(); counts[2] = c.n_pieces; counts[3] = c.n_contigs; counts[4] = s.n_nodes; counts[5] = s.n_edges;
    counts[6] = c.steps; counts[7] = c.ambiguity_cuts; counts[8] = c.self_loops; counts[9] = c.simple_loops; counts[10] = c.scc_restarts;
    counts[11] = c.nodes_removed; counts[12] = c.ambiguity_moves; counts[13] = want;
    return ok ? 0 : 1;
}

extern "C" int hs_contig_stats(const uint64_t* lengths, uint64_t n, uint64_t original_genome_length, uint64_t* out4) {
    katome::ContigStats st;
    const int rc = katome::contig_stats(lengths, n, original_genome_length, &st);
    out4[0] = st.n50; out4[1] = st.l50; out4[2] = st.n90; out4[3] = st.ng50;
    return rc;
}

// the route of katome_assemble_* over several GPUs (multi_route.h, plan_multi_route with `assembling`), as the bits of
// tests/hostshim/multi_route_host.cpp: 1 sharded shrink, 2 fast shrink after the gather, 4 KATOME_E_ARG, 8 direct, 16 gathers,
// 32 remove_dead_paths on the sharded graph, 64 the stage letters on the sharded graph, 128 local transport
extern "C" uint32_t hs_assemble_route(uint32_t flags, uint64_t total_edges, uint64_t total_nodes) {
    const katome::MultiRoute p = katome::plan_multi_route(flags, false, "dcwced", true);
    return (p.sharded_shrink ? 1u : 0) | (p.gather_fast ? 2u : 0) | (p.bad_arg ? 4u : 0) | (p.direct ? 8u : 0) |
           (p.gathers(total_edges, total_nodes) ? 16u : 0) | (p.sharded_dead_paths() ? 32u : 0) | (p.sharded_stage_letters() ? 64u : 0) |
           (p.local_comm ? 128u : 0);
}
