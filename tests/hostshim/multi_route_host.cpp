// Host build of katome_amd/csrc/multi_route.h for the CPU tests (tests/test_multi_route_host.py).
#include "../../katome_amd/csrc/multi_route.h"

using namespace katome;

extern "C" {

// the plan for these flags and this request under the environment of the moment, as bits:
// 1 sharded shrink, 2 fast shrink after the gather, 4 KATOME_E_ARG, 8 direct, 16 gathers(total_edges, total_nodes),
// 32 remove_dead_paths on the sharded graph, 64 the stage letters on the sharded graph, 128 local transport
uint32_t hs_multi_route(uint32_t flags, int want_contigs, const char* stages, uint64_t total_edges, uint64_t total_nodes) {
    const MultiRoute p = plan_multi_route(flags, want_contigs != 0, stages);
    return (p.sharded_shrink ? 1u : 0) | (p.gather_fast ? 2u : 0) | (p.bad_arg ? 4u : 0) | (p.direct ? 8u : 0) |
           (p.gathers(total_edges, total_nodes) ? 16u : 0) | (p.sharded_dead_paths() ? 32u : 0) | (p.sharded_stage_letters() ? 64u : 0) |
           (p.local_comm ? 128u : 0);
}

}
