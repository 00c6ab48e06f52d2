// multi_route.h -- which way a host build over several GPUs goes (host_build.cpp, build_multi): decided once, from the
// settings' flags, what the caller asked for and the environment, before any communicator or rank thread exists.  Nothing of
// HIP in here: tests/hostshim compiles it for the host (tests/test_multi_route_host.py walks every combination).
//
// What the code below does not say by itself.  The gathered route collects the graph on the first GPU and finishes it there
// with the one-GPU code; the direct route leaves it sharded, and every rank copies its share into the host arrays.  The two
// forms of shrink number their results differently (gathered, AUTO: the exact form in first-seen order; KATOME_DIST_SHRINK=
// sharded: the traversal-free form of dist_shrink.hip, in either numbering), so nothing switches from one to the other without
// being asked; KATOME_DIST_SHRINK=gather is the gather followed by the fast form, for comparisons with the sharded one.  The
// stages after the build leave the gathered route only when asked (KATOME_DIST_STAGES=sharded) or when they must: a graph of
// 2^32 edges or nodes and more cannot be gathered.  KATOME_DIST_PRUNE=gather sends a build that would go direct through the
// gather as well.
#pragma once
#include <stdint.h>

#include "../../include/katome_gpu.h"
#include "env.h"

namespace katome {

struct MultiRoute {
    bool first_seen = false, remove_dead_paths = false;      // settings.flags
    bool contigs = false, stages = false;                    // the caller wants the shrunk graph / named stages to run first
    bool sharded_shrink = false;    // shrink on the sharded graph, its parts put together on the host
    bool gather_fast = false;       // shrink after the gather in its fast form
    bool bad_arg = false;           // KATOME_E_ARG: this call needs KATOME_FLAG_FIRST_SEEN_ORDER
    bool direct = false;            // first-seen order and no gather, whatever the graph's size
    bool stages_sharded = false, stages_gathered = false;    // KATOME_DIST_STAGES = sharded / gather
    bool local_comm = false;        // the ranks exchange through host rendezvous and device copies, not RCCL
    bool unitigs = false;           // katome_unitigs_*: everything on the shares, through the sharded shrink to its text; never a gather

    // after finalize, every rank with the same totals: gather the graph to the first GPU and finish it there?
    bool gathers(uint64_t total_edges, uint64_t total_nodes) const {
        if (unitigs || !first_seen || direct) return false;
        if (contigs || !stages) return true;
        const bool too_big = total_edges >= 0xFFFFFFFFull || total_nodes >= 0xFFFFFFFFull;
        return !(stages_sharded || (too_big && !stages_gathered));
    }
    // on the sharded graph, in this order: remove_dead_paths; then the sharded shrink and nothing further; else the stage
    // letters; then the copy-out
    bool sharded_dead_paths() const { return first_seen && remove_dead_paths; }
    bool sharded_stage_letters() const { return first_seen && stages && !sharded_shrink; }
};

// assembling (katome_assemble_*): the stages "dcwced" and collapse run on the graph gathered to the first GPU, whatever the
// environment says about shrink and the stages -- the exact shrink and the walk behind it are one GPU's
// unitigs (katome_unitigs_*): remove_dead_paths, the stage letters, the traversal-free shrink, its text and its stats all run on the
// shares, whatever the environment says; the sharded stages need the links of a first-seen build, a packed-key build without
// stages does not
static inline MultiRoute plan_multi_route(uint32_t flags, bool want_contigs, const char* stages, bool assembling = false, bool unitigs = false) {
    MultiRoute p;
    if (unitigs) {
        p.unitigs = true;
        p.first_seen = (flags & KATOME_FLAG_FIRST_SEEN_ORDER) != 0;
        p.remove_dead_paths = (flags & KATOME_FLAG_REMOVE_DEAD_PATHS) != 0;
        p.stages = stages && *stages;
        p.bad_arg = !p.first_seen && (p.stages || p.remove_dead_paths);
        p.local_comm = (flags & KATOME_FLAG_RANKS_SHARE_DEVICE) != 0 || env_is("KATOME_COMM", "local");
        return p;
    }
    if (assembling) {
        p.first_seen = (flags & KATOME_FLAG_FIRST_SEEN_ORDER) != 0;
        p.remove_dead_paths = (flags & KATOME_FLAG_REMOVE_DEAD_PATHS) != 0;
        p.contigs = true;                    // (as for a shrink: gathers() whatever the graph's size, and the gather refuses what does not fit)
        p.bad_arg = !p.first_seen;      // (no stage letters on the shares: "dcwced" runs after the gather)
        p.local_comm = (flags & KATOME_FLAG_RANKS_SHARE_DEVICE) != 0 || env_is("KATOME_COMM", "local");
        return p;
    }
    p.first_seen = (flags & KATOME_FLAG_FIRST_SEEN_ORDER) != 0;
    p.remove_dead_paths = (flags & KATOME_FLAG_REMOVE_DEAD_PATHS) != 0;
    p.contigs = want_contigs;
    p.stages = stages && *stages;
    p.sharded_shrink = want_contigs && env_is("KATOME_DIST_SHRINK", "sharded");
    p.gather_fast = want_contigs && env_is("KATOME_DIST_SHRINK", "gather");
    p.bad_arg = !p.first_seen && ((want_contigs && !p.sharded_shrink) || p.stages || p.remove_dead_paths);
    p.direct = p.first_seen && (!want_contigs || p.sharded_shrink) && !p.stages && !env_is("KATOME_DIST_PRUNE", "gather");
    p.stages_sharded = env_is("KATOME_DIST_STAGES", "sharded");
    p.stages_gathered = env_is("KATOME_DIST_STAGES", "gather");
    p.local_comm = (flags & KATOME_FLAG_RANKS_SHARE_DEVICE) != 0 || env_is("KATOME_COMM", "local");
    return p;
}

}  // namespace katome
