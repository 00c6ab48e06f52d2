// Host build of katome_amd/csrc/multi_route.h for tests/test_unitigs_route_host.py: the route of katome_unitigs_* (plan_multi_route
// with `unitigs`) beside the route of the same request without it.
#include "../../katome_amd/csrc/multi_route.h"

using namespace katome;

extern "C" {

// the bits of tests/hostshim/multi_route_host.cpp -- 1 sharded shrink, 2 fast shrink after the gather, 4 KATOME_E_ARG, 8 direct,
// 16 gathers(total_edges, total_nodes), 32 remove_dead_paths on the sharded graph, 64 the stage letters on the sharded graph,
// 128 local transport -- and 256: the unitigs route
uint32_t hs_unitigs_route(uint32_t flags, int want_contigs, const char* stages, int unitigs, uint64_t total_edges, uint64_t total_nodes) {
    const MultiRoute p = plan_multi_route(flags, want_contigs != 0, stages, false, unitigs != 0);
    return (p.sharded_shrink ? 1u : 0) | (p.gather_fast ? 2u : 0) | (p.bad_arg ? 4u : 0) | (p.direct ? 8u : 0) |
           (p.gathers(total_edges, total_nodes) ? 16u : 0) | (p.sharded_dead_paths() ? 32u : 0) | (p.sharded_stage_letters() ? 64u : 0) |
           (p.local_comm ? 128u : 0) | (p.unitigs ? 256u : 0);
}

}
