// dist_gfa_dir.h -- the directory by new node id that dist_gfa.hip joins links through: vertex v of [0, total) lives on rank
// v / ceil(total / world), the scheme dist_shrink.hip numbers the surviving nodes by.  Plain C++, no HIP: tests/hostshim checks it.
#pragma once
#include <stdint.h>

namespace katome {

struct GfaDirectory {
    uint64_t total, per;      // vertices of the whole shrunk graph; vertices per rank (at least 1: total may be 0)
    uint32_t world;
    GfaDirectory(uint64_t total_nodes, uint32_t world_) : total(total_nodes), per((total_nodes + world_ - 1) / world_), world(world_) { if (per == 0) per = 1; }
    uint64_t owner(uint64_t v) const { return v / per; }                                              // (< world for v < total)
    uint64_t base(uint32_t rank) const { const uint64_t b = (uint64_t)rank * per; return b < total ? b : total; }
    uint64_t range(uint32_t rank) const { const uint64_t b = base(rank), e = b + per < total ? b + per : total; return e - b; }   // may be 0
    uint64_t address(uint64_t v) const { return (owner(v) << 56) | v; }                               // what the Router routes by (ids < 2^56)
};

}  // namespace katome
