// Host build of katome_amd/csrc/dist_gfa_dir.h for the CPU tests (tests/test_dist_gfa_host.py).
#include "../../katome_amd/csrc/dist_gfa_dir.h"

using namespace katome;

extern "C" {

uint64_t hs_gfa_dir_per(uint64_t total, uint32_t world) { return GfaDirectory(total, world).per; }
uint64_t hs_gfa_dir_base(uint64_t total, uint32_t world, uint32_t rank) { return GfaDirectory(total, world).base(rank); }
uint64_t hs_gfa_dir_range(uint64_t total, uint32_t world, uint32_t rank) { return GfaDirectory(total, world).range(rank); }
uint64_t hs_gfa_dir_owner(uint64_t total, uint32_t world, uint64_t v) { return GfaDirectory(total, world).owner(v); }
uint64_t hs_gfa_dir_address(uint64_t total, uint32_t world, uint64_t v) { return GfaDirectory(total, world).address(v); }

}
