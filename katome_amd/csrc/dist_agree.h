// dist_agree.h -- how the ranks of a collective call keep in step about failures (dist_stats.hip, dist_text.hip): what a rank did
// on its own since the last collective -- allocations, launches, checks -- is a status that all ranks exchange before the next one,
// so that no rank is left waiting inside a collective for one that has already given up.
#pragma once
#include <algorithm>
#include <string>
#include <vector>

#include "comm.h"

namespace katome {

struct Collective {
    katome_comm* comm; const char* name; int rank, world;
    std::vector<uint64_t> all;
    Collective(katome_comm* c, const char* name_) : comm(c), name(name_), rank(c->rank()), world(c->world()), all(c->world(), 0) {}
    // every rank's status since the last collective (0 or a KATOME_E_* code of its own, its message set) and a number below
    // 2^48 of which all ranks get the largest.  One allgather; a failure anywhere comes back on every rank, naming the rank
    int agree(int mine, uint64_t* largest = nullptr) {
        const std::string why = mine ? get_error() : "";
        const uint64_t word = ((uint64_t)(mine ? -mine : 0) << 48) | (largest ? *largest & ((1ull << 48) - 1) : 0);
        KCHECK(comm->allgather(word, all.data()));
        uint64_t mx = 0;
        for (int p = 0; p < world; ++p) {
            const int status = -(int)(all[p] >> 48);
            if (status) {
                if (p == rank) set_error("%s: rank %d of %d failed: %s", name, p, world, why.c_str());
                else set_error("%s: rank %d of %d failed (status %d)", name, p, world, status);
                return status;
            }
            mx = std::max<uint64_t>(mx, all[p] & ((1ull << 48) - 1));
        }
        if (largest) *largest = mx;
        return KATOME_OK;
    }
};

}  // namespace katome
