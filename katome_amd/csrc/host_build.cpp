// host_build.cpp -- the host-memory half of the C ABI of include/katome_gpu.h: katome_build_packed*, katome_build_files*,
// katome_shrink_*, katome_gfa_*, the host result arrays and the driver of a build over several GPUs.  No kernel is defined or launched here:
// everything on the device goes through the device ABI (api.hip) and the sharded builder (dist*.hip).
#include <stdlib.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <initializer_list>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include <sys/mman.h>

#include <errno.h>

#include "builder.h"
#include "comm.h"
#include "contig_stats.h"
#include "multi_route.h"

extern "C" {

struct GraphOwner {            // katome_graph followed by what it owns
    katome_graph g;
    std::vector<void*> mem;
};

void katome_graph_free(katome_graph* g) {
    if (!g) return;
    GraphOwner* o = reinterpret_cast<GraphOwner*>(g);
    for (void* p : o->mem) free(p);
    delete o;
}

struct ContigsOwner {          // katome_contigs followed by what it owns
    katome_contigs c;
    std::vector<void*> mem;
};
void katome_contigs_free(katome_contigs* c) {
    if (!c) return;
    ContigsOwner* o = reinterpret_cast<ContigsOwner*>(c);
    for (void* p : o->mem) free(p);
    delete o;
}

struct AssemblyOwner {         // katome_assembly followed by what it owns
    katome_assembly a;
    std::vector<void*> mem;
};
void katome_assembly_free(katome_assembly* a) {
    if (!a) return;
    AssemblyOwner* o = reinterpret_cast<AssemblyOwner*>(a);
    for (void* p : o->mem) free(p);
    delete o;
}

struct GfaOwner {              // katome_gfa followed by what it owns
    katome_gfa g;
    std::vector<void*> mem;
};
void katome_gfa_free(katome_gfa* g) {
    if (!g) return;
    GfaOwner* o = reinterpret_cast<GfaOwner*>(g);
    for (void* p : o->mem) free(p);
    delete o;
}

struct GfaStrandsOwner {       // katome_gfa_strands followed by what it owns
    katome_gfa_strands g;
    std::vector<void*> mem;
};
void katome_gfa_strands_free(katome_gfa_strands* g) {
    if (!g) return;
    GfaStrandsOwner* o = reinterpret_cast<GfaStrandsOwner*>(g);
    for (void* p : o->mem) free(p);
    delete o;
}

struct GfaPathsOwner {         // katome_gfa_paths followed by what it owns
    katome_gfa_paths g;
    std::vector<void*> mem;
};
void katome_gfa_paths_free(katome_gfa_paths* g) {
    if (!g) return;
    GfaPathsOwner* o = reinterpret_cast<GfaPathsOwner*>(g);
    for (void* p : o->mem) free(p);
    delete o;
}

struct GfaStrandPathsOwner {   // katome_gfa_strand_paths followed by what it owns
    katome_gfa_strand_paths g;
    std::vector<void*> mem;
};
void katome_gfa_strand_paths_free(katome_gfa_strand_paths* g) {
    if (!g) return;
    GfaStrandPathsOwner* o = reinterpret_cast<GfaStrandPathsOwner*>(g);
    for (void* p : o->mem) free(p);
    delete o;
}

struct UniqueAssemblyOwner {   // katome_unique_assembly followed by what it owns
    katome_unique_assembly u;
    std::vector<void*> mem;
};
void katome_unique_assembly_free(katome_unique_assembly* u) {
    if (!u) return;
    UniqueAssemblyOwner* o = reinterpret_cast<UniqueAssemblyOwner*>(u);
    for (void* p : o->mem) free(p);
    delete o;
}

}  // extern "C"

// KATOME_TRACE_BUILD=1: wall time of the host entries' stages on stderr
static void build_lap(const char* what, bool reset = false) {
    static const bool on = getenv("KATOME_TRACE_BUILD") != nullptr;
    static std::chrono::steady_clock::time_point last;
    if (!on) return;
    const auto now = std::chrono::steady_clock::now();
    if (!reset) fprintf(stderr, "[build] %-28s %9.2f ms\n", what, std::chrono::duration<double, std::milli>(now - last).count());
    last = now;
}

// Host memory for a result array.  A device -> host copy into pages the process has never touched runs at the rate one
// thread takes page faults (~9 GB/s measured on the MI355X box; into touched pages, pinned or not, the same copy runs at
// ~55 GB/s), so large arrays are taken 2 MiB-aligned, offered to the kernel as huge pages and first touched by several
// threads at once.  Released with free().
static void* host_result_reserve(size_t bytes) {          // (pages not touched yet)
    const size_t big = (size_t)64 << 20, huge = (size_t)2 << 20;
    if (bytes < big) return malloc(std::max<size_t>(bytes, 1));
    void* p = nullptr;
    if (posix_memalign(&p, huge, (bytes + huge - 1) / huge * huge) != 0) return nullptr;
    (void)madvise(p, bytes, MADV_HUGEPAGE);
    return p;
}
static void host_result_touch(void* p, size_t bytes) {
    if (bytes < ((size_t)64 << 20)) return;
    unsigned T = std::thread::hardware_concurrency();
    T = std::max(1u, std::min(T ? T : 4u, 16u));
    const size_t pages = (bytes + 4095) / 4096, per = (pages + T - 1) / T;
    std::vector<std::thread> th;
    for (unsigned t = 0; t < T; ++t)
        th.emplace_back([=]() {
            volatile char* c = static_cast<volatile char*>(p);
            for (size_t pg = t * per; pg < std::min(pages, (t + 1) * per); ++pg) c[pg * 4096] = 0;
        });
    for (auto& x : th) x.join();
}
static void* host_result_alloc(size_t bytes) {
    void* p = host_result_reserve(bytes);
    if (p) host_result_touch(p, bytes);
    return p;
}

// room for a result array of `bytes` bytes, recorded in the owner that will free it (nullptr and *oom set: out of host memory)
template <class Owner> static void* take(Owner* o, size_t bytes, bool* oom, bool touch = true) {
    void* p = touch ? host_result_alloc(bytes) : host_result_reserve(bytes);
    if (p) o->mem.push_back(p); else *oom = true;
    return p;
}

// Several result arrays: while array i comes over PCIe, the pages of array i + 1 are being touched (a third of the time of
// a 7 GB graph was the touching, done array by array in front of each copy).
struct HostCopy { void* h; size_t bytes; const void* src; };      // (h: reserved, its pages not touched yet)
static int d2h_all(const std::vector<HostCopy>& jobs) {
    std::mutex m; std::condition_variable cv; size_t touched = 0;
    std::thread toucher([&]() {
        for (auto& j : jobs) {
            host_result_touch(j.h, j.bytes);
            { std::lock_guard<std::mutex> lk(m); ++touched; }
            cv.notify_all();
        }
    });
    int rc = KATOME_OK;
    for (size_t i = 0; i < jobs.size(); ++i) {
        { std::unique_lock<std::mutex> lk(m); cv.wait(lk, [&]() { return touched > i; }); }
        if (rc == KATOME_OK && jobs[i].bytes && hipMemcpy(jobs[i].h, jobs[i].src, jobs[i].bytes, hipMemcpyDeviceToHost) != hipSuccess) {
            set_error("device -> host copy failed: %s", hipGetErrorString(hipGetLastError()));
            rc = KATOME_E_DEVICE;
        }
    }
    toucher.join();
    return rc;
}

template <class T, class Owner> static int d2h(Owner* o, const T** dst, const void* d_src, size_t count) {
    bool oom = false;
    T* h = (T*)take(o, std::max<size_t>(count, 1) * sizeof(T), &oom);
    if (oom) { set_error("out of host memory"); return KATOME_E_OOM; }
    if (count) KCHECK_HIP(hipMemcpy(h, d_src, count * sizeof(T), hipMemcpyDeviceToHost));
    *dst = h;
    return KATOME_OK;
}

// these device -> host copies queued on `stream`, then the stream synchronised; the first failure is the one reported
struct StreamCopy { void* h; const void* src; size_t bytes; };
static int copy_down(std::initializer_list<StreamCopy> jobs, hipStream_t stream) {
    hipError_t e = hipSuccess;
    for (const StreamCopy& j : jobs)
        if (j.bytes && e == hipSuccess) e = hipMemcpyAsync(j.h, j.src, j.bytes, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) { set_error("D2H copy failed: %s", hipGetErrorString(e)); return KATOME_E_DEVICE; }
    return KATOME_OK;
}

// A katome_graph of the given totals: its header filled in and its arrays reserved, their pages not touched yet.  `arrays`
// lists them in the order edge_src, edge_dst, edge_weight, edge_label, edge_key, node_key and, with `ages`, edge_age.
static int new_host_graph(uint64_t n_nodes, uint64_t n_edges, uint32_t k, uint32_t key_words, uint32_t label_stride, bool ages,
                          uint64_t read_bytes, GraphOwner** out, std::vector<HostCopy>& arrays) {
    GraphOwner* o = new (std::nothrow) GraphOwner();
    if (!o) { set_error("out of host memory"); return KATOME_E_OOM; }
    memset(&o->g, 0, sizeof o->g);
    katome_graph* g = &o->g;
    g->n_nodes = n_nodes; g->n_edges = n_edges; g->read_bytes = read_bytes;
    g->k = k; g->key_words = key_words; g->label_stride = label_stride;
    bool oom = false;
    auto room = [&](size_t bytes) { arrays.push_back({take(o, bytes, &oom, false), bytes, nullptr}); return arrays.back().h; };
    g->edge_src = (uint64_t*)room(n_edges * 8); g->edge_dst = (uint64_t*)room(n_edges * 8);
    g->edge_weight = (uint32_t*)room(n_edges * 4); g->edge_label = (uint8_t*)room(n_edges * (size_t)label_stride);
    g->edge_key = (uint64_t*)room(n_edges * 8 * (size_t)key_words); g->node_key = (uint64_t*)room(n_nodes * 8 * (size_t)key_words);
    if (ages) g->edge_age = (uint32_t*)room(n_edges * 4);
    if (oom) { katome_graph_free(g); set_error("out of host memory"); return KATOME_E_OOM; }
    *out = o;
    return KATOME_OK;
}

// The stages of assemble_with_graph (asm/basic_assembler.rs:58-72) a host entry may ask for after the build, in the order
// given: d = remove_dead_paths, c = standardize_contigs, w = remove_weak_edges(min_weight), e = standardize_edges(
// original_genome_length, k, min_weight).  `ops` runs them: on one GPU's builder, or on this rank's share of a sharded graph.
struct BuilderStages {
    katome_builder* b; uint64_t genome_len;
    int dead_paths() const { return katome_dev_remove_dead_paths(b, nullptr, nullptr, nullptr); }
    int contigs() const { return katome_dev_standardize_contigs(b, nullptr); }
    int weak_edges() const { return katome_dev_remove_weak_edges(b, b->s.min_weight, nullptr); }
    int edges() const { return katome_dev_standardize_edges(b, genome_len, b->s.min_weight, nullptr); }
};
struct ShardedStages {
    katome_dist_builder* d; katome_dist_graph* g; uint32_t min_weight; uint64_t genome_len; hipStream_t stream;
    int dead_paths() const { return katome_dist_remove_dead_paths(d, g, nullptr, stream); }
    int contigs() const { return katome_dist_standardize_contigs(d, g, stream); }
    int weak_edges() const { return katome_dist_prune_weak_edges(d, min_weight, g, stream); }
    int edges() const { return katome_dist_standardize_edges(d, genome_len, min_weight, g, stream); }
};
// `at_stage` (optional) is called with 0 before the first stage and with i after the i-th: where assemble_with_graph logs the
// graph (graph.log_stats(), asm/basic_assembler.rs:58-75)
struct NoStageHook { int operator()(size_t) const { return KATOME_OK; } };
template <class Ops, class Hook = NoStageHook> static int run_stages(const char* stages, const Ops& ops, const Hook& at_stage = Hook()) {
    KCHECK(at_stage(0));
    size_t done = 0;
    for (const char* st = stages ? stages : ""; *st; ++st) {
        switch (*st) {
            case 'd': KCHECK(ops.dead_paths()); break;
            case 'c': KCHECK(ops.contigs()); break;
            case 'w': KCHECK(ops.weak_edges()); break;
            case 'e': KCHECK(ops.edges()); break;
            default: set_error("unknown stage '%c' (d, c, w, e)", *st); return KATOME_E_ARG;      // (on the sharded graph: the same on every rank)
        }
        KCHECK(at_stage(++done));
    }
    return KATOME_OK;
}

// (stage_stats: the caller's strlen(stages) + 1 entries, filled on the device as the stages go by)
static int graph_to_host(katome_builder* b, uint64_t read_bytes, katome_graph** out, const char* stages = nullptr, uint64_t genome_len = 0,
                         katome_stats* stage_stats = nullptr) {
    katome_dev_graph dg;
    if (stages && *stages && !b->first_seen) { set_error("stages after the build need KATOME_FLAG_FIRST_SEEN_ORDER"); return KATOME_E_ARG; }
    build_lap("counting (H2D, kernels)");
    KCHECK(katome_dev_finalize(b, &dg, nullptr));
    build_lap("finalize");
    if (b->s.flags & KATOME_FLAG_REMOVE_DEAD_PATHS) KCHECK(katome_dev_remove_dead_paths(b, &dg, nullptr, nullptr));
    KCHECK(run_stages(stages, BuilderStages{b, genome_len},
                      [&](size_t i) { return stage_stats ? katome_dev_graph_stats(b, &stage_stats[i], nullptr) : KATOME_OK; }));
    KCHECK(katome_dev_current_graph(b, &dg));
    build_lap("stages after the build");
    GraphOwner* o = nullptr;
    std::vector<HostCopy> jobs;
    KCHECK(new_host_graph(dg.n_nodes, dg.n_edges, b->s.k, dg.key_words, dg.label_stride, dg.d_edge_age != nullptr, read_bytes, &o, jobs));
    const void* from[] = {dg.d_edge_src, dg.d_edge_dst, dg.d_edge_weight, dg.d_edge_label, dg.d_edge_key, dg.d_node_key, dg.d_edge_age};
    for (size_t i = 0; i < jobs.size(); ++i) jobs[i].src = from[i];
    const int rc = d2h_all(jobs);
    if (rc) { katome_graph_free(&o->g); return rc; }
    build_lap("graph to host arrays");
    *out = &o->g;
    return KATOME_OK;
}

// finalize (+ the pruning the flags ask for) + shrink, copied to host arrays
static int contigs_to_host(katome_builder* b, uint64_t read_bytes, katome_contigs** out, uint32_t shrink_mode = KATOME_SHRINK_AUTO) {
    katome_dev_graph dg;
    KCHECK(katome_dev_finalize(b, &dg, nullptr));
    if (b->s.flags & KATOME_FLAG_REMOVE_DEAD_PATHS) KCHECK(katome_dev_remove_dead_paths(b, &dg, nullptr, nullptr));
    katome_dev_contigs dc;
    KCHECK(katome_dev_shrink_mode(b, shrink_mode, &dc, nullptr, nullptr));
    ContigsOwner* o = new (std::nothrow) ContigsOwner();
    if (!o) { set_error("out of host memory"); return KATOME_E_OOM; }
    memset(&o->c, 0, sizeof o->c);
    katome_contigs* c = &o->c;
    c->n_nodes = dc.n_nodes; c->n_edges = dc.n_edges; c->label_bytes = dc.label_bytes; c->read_bytes = read_bytes;
    c->k = b->s.k; c->key_words = dc.key_words;
    int rc = KATOME_OK;
    if ((rc = d2h(o, &c->edge_src, dc.d_edge_src, dc.n_edges)) || (rc = d2h(o, &c->edge_dst, dc.d_edge_dst, dc.n_edges)) ||
        (rc = d2h(o, &c->edge_weight, dc.d_edge_weight, dc.n_edges)) || (rc = d2h(o, &c->edge_kmers, dc.d_edge_kmers, dc.n_edges)) ||
        (rc = d2h(o, &c->edge_label_off, dc.d_edge_label_off, dc.n_edges ? dc.n_edges + 1 : 0)) ||
        (rc = d2h(o, &c->edge_label, dc.d_edge_label, dc.label_bytes)) ||
        (rc = d2h(o, &c->node_key, dc.d_node_key, dc.n_nodes * dc.key_words))) {
        katome_contigs_free(c);
        return rc;
    }
    if (dc.n_edges == 0) const_cast<uint64_t*>(c->edge_label_off)[0] = 0;       // (d2h hands out room for one entry even when asked for none)
    *out = c;
    return KATOME_OK;
}

extern "C" int katome_contig_stats_of(const uint64_t* lengths, uint64_t n, uint64_t original_genome_length, katome_contig_stats* out) {
    if (!out || (n && !lengths)) { set_error("null argument"); return KATOME_E_ARG; }
    ContigStats st;
    const int which = contig_stats(lengths, n, original_genome_length, &st);
    out->n50 = st.n50; out->l50 = st.l50; out->n90 = st.n90; out->ng50 = st.ng50;
    return contig_stats_status(which);
}

// Contigs::save_to_file (asm/mod.rs:57-72): the text in FASTA layout is the file
extern "C" int katome_assembly_save(const katome_assembly* a, const char* path) {
    if (!a || !path) { set_error("null argument"); return KATOME_E_ARG; }
    if (a->layout != KATOME_TEXT_FASTA) { set_error("assembly_save: the text is not in FASTA layout"); return KATOME_E_ARG; }
    FILE* f = fopen(path, "wb");
    if (!f) {
        set_error("couldn't create %s: %s", path, CREATE_ERROR_KINDS[create_error_kind(errno)]);      // asm/mod.rs:62
        return KATOME_E_OPEN;
    }
    const size_t n = a->text_bytes ? fwrite(a->text, 1, a->text_bytes, f) : 0;
    if (fclose(f) != 0 || n != a->text_bytes) { set_error("couldn't write %s", path); return KATOME_E_OPEN; }
    return KATOME_OK;
}

static int save_gfa_text(const uint8_t* text, uint64_t text_bytes, const char* path);
extern "C" int katome_gfa_paths_save(const katome_gfa_paths* g, const char* path) {
    if (!g || !path) { set_error("null argument"); return KATOME_E_ARG; }
    return save_gfa_text(g->text, g->text_bytes + g->path_bytes, path);      // (the two parts are contiguous on the host)
}
// katome_dev_collapse_gfa of the builder's last collapse in host arrays: the two parts of the text back to back
static int gfa_paths_to_host(katome_builder* b, uint64_t read_bytes, katome_gfa_paths** out) {
    katome_dev_gfa_paths d;
    KCHECK(katome_dev_collapse_gfa(b, &d, nullptr));
    GfaPathsOwner* o = new (std::nothrow) GfaPathsOwner();
    if (!o) { set_error("out of host memory"); return KATOME_E_OOM; }
    memset(&o->g, 0, sizeof o->g);
    katome_gfa_paths* g = &o->g;
    g->n_segments = d.n_segments; g->n_links = d.n_links; g->text_bytes = d.text_bytes; g->read_bytes = read_bytes; g->k = b->s.k;
    g->n_paths = d.n_paths; g->n_jumps = d.n_jumps; g->path_bytes = d.path_bytes;
    bool oom = false;
    uint8_t* text = (uint8_t*)take(o, std::max<uint64_t>(d.text_bytes + d.path_bytes, 1), &oom);
    int rc = KATOME_OK;
    if (oom) { set_error("out of host memory"); rc = KATOME_E_OOM; }
    if (!rc && d.text_bytes && hipMemcpy(text, d.d_text, d.text_bytes, hipMemcpyDeviceToHost) != hipSuccess) rc = KATOME_E_DEVICE;
    if (!rc && d.path_bytes && hipMemcpy(text + d.text_bytes, d.d_path_text, d.path_bytes, hipMemcpyDeviceToHost) != hipSuccess) rc = KATOME_E_DEVICE;
    if (rc == KATOME_E_DEVICE) set_error("device -> host copy failed: %s", hipGetErrorString(hipGetLastError()));
    g->text = text;
    if (!rc) rc = d2h(o, &g->segment_off, d.d_segment_off, d.n_segments);
    if (!rc) rc = d2h(o, &g->link_first, d.d_link_first, d.n_segments + 1);
    if (!rc) rc = d2h(o, &g->path_line_off, d.d_path_line_off, d.n_paths + 1);
    if (!rc) rc = d2h(o, &g->path_contig, d.d_path_contig, d.n_paths);
    if (!rc) rc = d2h(o, &g->path_first_piece, d.d_path_first_piece, d.n_paths + 1);
    if (rc) { katome_gfa_paths_free(g); return rc; }
    *out = g;
    return KATOME_OK;
}

extern "C" int katome_gfa_strand_paths_save(const katome_gfa_strand_paths* g, const char* path) {
    if (!g || !path) { set_error("null argument"); return KATOME_E_ARG; }
    return save_gfa_text(g->text, g->text_bytes + g->path_bytes, path);      // (the two parts are contiguous on the host)
}
// katome_dev_collapse_gfa_strands of the builder's last collapse in host arrays: the two parts of the text back to back
static int gfa_strand_paths_to_host(katome_builder* b, uint64_t read_bytes, katome_gfa_strand_paths** out) {
    katome_dev_gfa_strand_paths d;
    KCHECK(katome_dev_collapse_gfa_strands(b, &d, nullptr));
    GfaStrandPathsOwner* o = new (std::nothrow) GfaStrandPathsOwner();
    if (!o) { set_error("out of host memory"); return KATOME_E_OOM; }
    memset(&o->g, 0, sizeof o->g);
    katome_gfa_strand_paths* g = &o->g;
    g->n_segments = d.n_segments; g->n_links = d.n_links; g->text_bytes = d.text_bytes; g->read_bytes = read_bytes; g->k = b->s.k;
    g->n_edges = d.n_edges; g->n_unpaired = d.n_unpaired; g->n_self_twins = d.n_self_twins;
    g->n_paths = d.n_paths; g->n_jumps = d.n_jumps; g->path_bytes = d.path_bytes; g->n_mirrored = d.n_mirrored; g->n_self_mirror = d.n_self_mirror;
    bool oom = false;
    uint8_t* text = (uint8_t*)take(o, std::max<uint64_t>(d.text_bytes + d.path_bytes, 1), &oom);
    int rc = KATOME_OK;
    if (oom) { set_error("out of host memory"); rc = KATOME_E_OOM; }
    if (!rc && d.text_bytes && hipMemcpy(text, d.d_text, d.text_bytes, hipMemcpyDeviceToHost) != hipSuccess) rc = KATOME_E_DEVICE;
    if (!rc && d.path_bytes && hipMemcpy(text + d.text_bytes, d.d_path_text, d.path_bytes, hipMemcpyDeviceToHost) != hipSuccess) rc = KATOME_E_DEVICE;
    if (rc == KATOME_E_DEVICE) set_error("device -> host copy failed: %s", hipGetErrorString(hipGetLastError()));
    g->text = text;
    if (!rc) rc = d2h(o, &g->segment_off, d.d_segment_off, d.n_segments);
    if (!rc) rc = d2h(o, &g->link_first, d.d_link_first, d.n_segments + 1);
    if (!rc) rc = d2h(o, &g->segment_name, d.d_segment_name, d.n_segments);
    if (!rc) rc = d2h(o, &g->edge_twin, d.d_edge_twin, d.n_edges);
    if (!rc) rc = d2h(o, &g->path_line_off, d.d_path_line_off, d.n_paths + 1);
    if (!rc) rc = d2h(o, &g->path_contig, d.d_path_contig, d.n_paths);
    if (!rc) rc = d2h(o, &g->path_first_piece, d.d_path_first_piece, d.n_paths + 1);
    if (!rc) rc = d2h(o, &g->path_mirror, d.d_path_mirror, d.n_paths);
    if (rc) { katome_gfa_strand_paths_free(g); return rc; }
    *out = g;
    return KATOME_OK;
}

extern "C" int katome_unique_assembly_save(const katome_unique_assembly* u, const char* path) {
    if (!u || !path) { set_error("null argument"); return KATOME_E_ARG; }
    return save_gfa_text(u->text, u->text_bytes, path);      // (File::create's statuses and message, as for every text here)
}
// katome_dev_collapse_unique(FASTA) of the builder's last collapse in host arrays; lengths: every contig's bases, as the walk knows them
static int unique_to_host(katome_builder* b, uint64_t read_bytes, const std::vector<uint64_t>& lengths, uint64_t genome_len, katome_unique_assembly** out) {
    katome_dev_unique_assembly d;
    KCHECK(katome_dev_collapse_unique(b, KATOME_TEXT_FASTA, &d, nullptr));
    UniqueAssemblyOwner* o = new (std::nothrow) UniqueAssemblyOwner();
    if (!o) { set_error("out of host memory"); return KATOME_E_OOM; }
    memset(&o->u, 0, sizeof o->u);
    katome_unique_assembly* u = &o->u;
    u->n_contigs = d.n_contigs; u->n_kept = d.n_kept; u->text_bytes = d.text_bytes; u->read_bytes = read_bytes; u->k = b->s.k;
    u->n_mirrored = d.n_mirrored; u->n_self_mirror = d.n_self_mirror;
    int rc = d2h(o, &u->contig_mirror, d.d_contig_mirror, d.n_contigs);
    if (!rc) rc = d2h(o, &u->kept_name, d.d_kept_name, d.n_kept);
    if (!rc) rc = d2h(o, &u->kept_off, d.d_kept_off, d.n_kept);
    if (!rc) rc = d2h(o, &u->kept_len, d.d_kept_len, d.n_kept);
    if (!rc) rc = d2h(o, &u->text, d.d_text, d.text_bytes);
    if (!rc) {
        std::vector<uint64_t> kept;
        try { kept.reserve(d.n_kept); }
        catch (const std::bad_alloc&) { set_error("out of host memory"); rc = KATOME_E_OOM; }
        for (uint64_t i = 0; i < d.n_kept && !rc; ++i) {
            const uint64_t c = u->kept_name[i];
            if (c >= lengths.size() || lengths[c] != u->kept_len[i]) { set_error("collapse_unique: kept contig %llu does not have the walk's length", (unsigned long long)c); rc = KATOME_E_DEVICE; }
            else kept.push_back(lengths[c]);
        }
        if (!rc) rc = katome_contig_stats_of(kept.data(), kept.size(), genome_len, &u->stats);
    }
    if (rc) { katome_unique_assembly_free(u); return rc; }
    *out = u;
    return KATOME_OK;
}

// the stages "dcwced" (asm/basic_assembler.rs:58-75), collapse, Contigs::stats and, with a path, save_to_file: host arrays
// (with_gfa: katome_assemble_gfa_* -- the GFA of the collapse's shrunk graph with the contigs as P lines too; merge_strands:
// katome_assemble_gfa_strands_* -- that GFA with strand twins merged, handed back through strands_out)
struct AssembleWant {
    katome_assembly** out; const char* path; bool with_gfa = false; katome_gfa_paths** gfa_out = nullptr; const char* gfa_path = nullptr;
    bool merge_strands = false; katome_gfa_strand_paths** strands_out = nullptr;
    // (unique: katome_assemble_unique_* -- the strand-unique form of the contigs beside the assembly, no GFA)
    bool unique = false; katome_unique_assembly** unique_out = nullptr; const char* unique_path = nullptr;
};
static int assembly_to_host(katome_builder* b, uint64_t read_bytes, const AssembleWant& want, uint64_t genome_len) {
    katome_dev_graph dg;
    if (!b->first_seen) { set_error("assemble needs KATOME_FLAG_FIRST_SEEN_ORDER"); return KATOME_E_ARG; }
    KCHECK(katome_dev_finalize(b, &dg, nullptr));
    if (b->s.flags & KATOME_FLAG_REMOVE_DEAD_PATHS) KCHECK(katome_dev_remove_dead_paths(b, &dg, nullptr, nullptr));
    KCHECK(run_stages("dcwced", BuilderStages{b, genome_len}));
    build_lap("build and stages");
    AssemblyOwner* o = new (std::nothrow) AssemblyOwner();
    if (!o) { set_error("out of host memory"); return KATOME_E_OOM; }
    memset(&o->a, 0, sizeof o->a);
    katome_assembly* a = &o->a;
    katome_dev_assembly da;
    memset(&da, 0, sizeof da);
    std::vector<uint64_t> lengths;
    int rc = builder_collapse(b, KATOME_TEXT_FASTA, &da, &a->collapse, &lengths, nullptr);
    build_lap("collapse");
    a->n_contigs = da.n_contigs; a->text_bytes = da.text_bytes; a->read_bytes = read_bytes; a->k = b->s.k; a->layout = KATOME_TEXT_FASTA;
    if (!rc) rc = d2h(o, &a->contig_off, da.d_contig_off, da.n_contigs);
    if (!rc) rc = d2h(o, &a->contig_len, da.d_contig_len, da.n_contigs);
    if (!rc) rc = d2h(o, &a->text, da.d_text, da.text_bytes);
    if (!rc) rc = katome_contig_stats_of(lengths.data(), lengths.size(), genome_len, &a->stats);      // contigs.log_stats()
    if (rc) { katome_assembly_free(a); return rc; }
    if (want.unique) {
        katome_unique_assembly* u = nullptr;
        rc = unique_to_host(b, read_bytes, lengths, genome_len, &u);
        build_lap("collapse_unique");
        if (rc) { katome_assembly_free(a); return rc; }
        if (want.out) *want.out = a;
        if (want.unique_out) *want.unique_out = u;
        rc = want.path ? katome_assembly_save(a, want.path) : KATOME_OK;      // (both files are tried; the first failure is the one reported)
        const std::string first_err = rc ? get_error() : "";
        const int rc_unique = want.unique_path ? katome_unique_assembly_save(u, want.unique_path) : KATOME_OK;
        if (rc) set_error("%s", first_err.c_str()); else rc = rc_unique;
        if (!want.out) katome_assembly_free(a);
        if (!want.unique_out) katome_unique_assembly_free(u);
        return rc;
    }
    if (want.with_gfa) {
        katome_gfa_paths* g = nullptr;
        katome_gfa_strand_paths* gs = nullptr;
        rc = want.merge_strands ? gfa_strand_paths_to_host(b, read_bytes, &gs) : gfa_paths_to_host(b, read_bytes, &g);
        build_lap(want.merge_strands ? "collapse_gfa_strands" : "collapse_gfa");
        if (rc) { katome_assembly_free(a); return rc; }
        if (want.out) *want.out = a;
        if (want.gfa_out) *want.gfa_out = g;
        if (want.strands_out) *want.strands_out = gs;
        rc = want.path ? katome_assembly_save(a, want.path) : KATOME_OK;      // (both files are tried; the first failure is the one reported)
        const std::string first_err = rc ? get_error() : "";
        const int rc_gfa = !want.gfa_path ? KATOME_OK : gs ? katome_gfa_strand_paths_save(gs, want.gfa_path) : katome_gfa_paths_save(g, want.gfa_path);
        if (rc) set_error("%s", first_err.c_str()); else rc = rc_gfa;
        if (!want.out) katome_assembly_free(a);
        if (!want.gfa_out) katome_gfa_paths_free(g);
        if (!want.strands_out) katome_gfa_strand_paths_free(gs);
        return rc;
    }
    if (want.out) *want.out = a;
    rc = want.path ? katome_assembly_save(a, want.path) : KATOME_OK;
    if (!want.out) katome_assembly_free(a);
    return rc;
}

// katome_unitigs_* on one GPU: the flag's remove_dead_paths, the stage letters, the traversal-free shrink, its text in FASTA layout,
// Contigs::stats of the merged edges and, with a path, the file -- copied down a chunk at a time, the text is never whole on the host
// (katome_unitigs_gfa_*: the same pipeline with the graph as its ending -- `gfa` set, `out` not)
struct UnitigsWant { katome_unitigs* out; const char* path; katome_unitigs_gfa* gfa = nullptr; };
static int save_device_bytes(const uint8_t* d_text, uint64_t text_bytes, const char* path) {
    FILE* f = fopen(path, "wb");
    if (!f) { set_error("couldn't create %s: %s", path, CREATE_ERROR_KINDS[create_error_kind(errno)]); return KATOME_E_OPEN; }      // asm/mod.rs:62
    const size_t chunk = std::min<uint64_t>(std::max<uint64_t>(text_bytes, 1), (uint64_t)64 << 20);
    std::vector<uint8_t> buf;
    int rc = KATOME_OK;
    try { buf.resize(chunk); }
    catch (const std::bad_alloc&) { set_error("out of host memory"); rc = KATOME_E_OOM; }
    for (uint64_t at = 0; at < text_bytes && !rc; at += chunk) {
        const size_t n = std::min<uint64_t>(chunk, text_bytes - at);
        if (hipMemcpy(buf.data(), d_text + at, n, hipMemcpyDeviceToHost) != hipSuccess) { set_error("device -> host copy failed: %s", hipGetErrorString(hipGetLastError())); rc = KATOME_E_DEVICE; }
        else if (fwrite(buf.data(), 1, n, f) != n) { set_error("couldn't write %s", path); rc = KATOME_E_OPEN; }
    }
    if (fclose(f) != 0 && !rc) { set_error("couldn't write %s", path); rc = KATOME_E_OPEN; }
    if (rc) (void)remove(path);
    return rc;
}
static int save_device_text(const katome_dev_assembly& da, const char* path) { return save_device_bytes(da.d_text, da.text_bytes, path); }
static int unitigs_to_host(katome_builder* b, uint64_t read_bytes, const UnitigsWant& want, const char* stages, uint64_t genome_len) {
    katome_dev_graph dg;
    KCHECK(katome_dev_finalize(b, &dg, nullptr));
    if (b->s.flags & KATOME_FLAG_REMOVE_DEAD_PATHS) KCHECK(katome_dev_remove_dead_paths(b, &dg, nullptr, nullptr));
    KCHECK(run_stages(stages, BuilderStages{b, genome_len}));
    katome_dev_contigs dc;
    const bool coverage = want.gfa && (b->s.flags & KATOME_FLAG_PATH_COVERAGE);      // (the graph's ending only: every other entry ignores the flag)
    katome_dev_coverage cov;
    if (coverage) KCHECK(katome_dev_shrink_coverage(b, KATOME_SHRINK_FAST, &dc, &cov, nullptr, nullptr));
    else KCHECK(katome_dev_shrink_mode(b, KATOME_SHRINK_FAST, &dc, nullptr, nullptr));
    if (want.gfa) {                                                  // the graph: katome_dev_contigs_gfa's text is the file
        katome_dev_gfa dgfa;
        if (coverage) KCHECK(katome_dev_contigs_gfa_coverage(b, &dc, &dgfa, nullptr));
        else KCHECK(katome_dev_contigs_gfa(b, &dc, &dgfa, nullptr));
        katome_unitigs_gfa* u = want.gfa;
        u->n_segments = dgfa.n_segments; u->n_links = dgfa.n_links; u->text_bytes = dgfa.text_bytes; u->read_bytes = read_bytes; u->k = b->s.k; u->n_devices = 1;
        std::vector<uint32_t> kmers;
        try { kmers.resize(dc.n_edges); }
        catch (const std::bad_alloc&) { set_error("out of host memory"); return KATOME_E_OOM; }
        if (dc.n_edges) KCHECK_HIP(hipMemcpy(kmers.data(), dc.d_edge_kmers, dc.n_edges * 4, hipMemcpyDeviceToHost));
        for (uint64_t i = 0; i < dc.n_edges; ++i) {
            const uint64_t len = (uint64_t)kmers[i] + b->s.k - 1;
            u->total_bases += len; u->longest = std::max(u->longest, len);
        }
        return want.path ? save_device_bytes(dgfa.d_text, dgfa.text_bytes, want.path) : KATOME_OK;
    }
    katome_dev_assembly da;
    KCHECK(katome_dev_contigs_text(b, &dc, KATOME_TEXT_FASTA, &da, nullptr));
    katome_unitigs* u = want.out;
    u->n_contigs = da.n_contigs; u->text_bytes = da.text_bytes; u->read_bytes = read_bytes; u->k = b->s.k; u->n_devices = 1;
    std::vector<uint32_t> kmers;
    std::vector<uint64_t> lengths;
    try { kmers.resize(dc.n_edges); lengths.resize(dc.n_edges); }
    catch (const std::bad_alloc&) { set_error("out of host memory"); return KATOME_E_OOM; }
    if (dc.n_edges) KCHECK_HIP(hipMemcpy(kmers.data(), dc.d_edge_kmers, dc.n_edges * 4, hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < dc.n_edges; ++i) {
        lengths[i] = (uint64_t)kmers[i] + b->s.k - 1;
        u->total_bases += lengths[i]; u->longest = std::max(u->longest, lengths[i]);
    }
    const int stats_rc = katome_contig_stats_of(lengths.data(), lengths.size(), genome_len, &u->stats);      // (a tipping point of 0: the file is written all the same)
    const std::string stats_err = stats_rc ? get_error() : "";
    if (want.path) KCHECK(save_device_text(da, want.path));
    if (stats_rc) set_error("%s", stats_err.c_str());
    return stats_rc;
}

// the GFA's text is the file
static int save_gfa_text(const uint8_t* text, uint64_t text_bytes, const char* path) {
    FILE* f = fopen(path, "wb");
    if (!f) {
        set_error("couldn't create %s: %s", path, CREATE_ERROR_KINDS[create_error_kind(errno)]);      // (katome_assembly_save's message)
        return KATOME_E_OPEN;
    }
    const size_t n = text_bytes ? fwrite(text, 1, text_bytes, f) : 0;
    if (fclose(f) != 0 || n != text_bytes) { set_error("couldn't write %s", path); return KATOME_E_OPEN; }
    return KATOME_OK;
}
extern "C" int katome_gfa_save(const katome_gfa* g, const char* path) {
    if (!g || !path) { set_error("null argument"); return KATOME_E_ARG; }
    return save_gfa_text(g->text, g->text_bytes, path);
}
extern "C" int katome_gfa_strands_save(const katome_gfa_strands* g, const char* path) {
    if (!g || !path) { set_error("null argument"); return KATOME_E_ARG; }
    return save_gfa_text(g->text, g->text_bytes, path);
}

// katome_gfa_*: the flag's remove_dead_paths, the stage letters, shrink (AUTO: exact on a first-seen build, fast otherwise), the GFA of
// the result copied to host arrays and, with a path, the file
// (strands: the merged form, katome_gfa_strands_* -- the same pipeline up to the shrink)
struct GfaWant { katome_gfa** out; const char* path; katome_gfa_strands** strands = nullptr; bool merge = false; };
static int gfa_strands_to_host(katome_builder* b, const katome_dev_contigs& dc, uint64_t read_bytes, const GfaWant& want) {
    katome_dev_gfa_strands d;
    KCHECK(katome_dev_contigs_gfa_strands(b, &dc, &d, nullptr));
    GfaStrandsOwner* o = new (std::nothrow) GfaStrandsOwner();
    if (!o) { set_error("out of host memory"); return KATOME_E_OOM; }
    memset(&o->g, 0, sizeof o->g);
    katome_gfa_strands* g = &o->g;
    g->n_segments = d.n_segments; g->n_links = d.n_links; g->text_bytes = d.text_bytes; g->read_bytes = read_bytes; g->k = b->s.k;
    g->n_edges = dc.n_edges; g->n_unpaired = d.n_unpaired; g->n_self_twins = d.n_self_twins;
    int rc = d2h(o, &g->text, d.d_text, d.text_bytes);
    if (!rc) rc = d2h(o, &g->segment_off, d.d_segment_off, d.n_segments);
    if (!rc) rc = d2h(o, &g->link_first, d.d_link_first, d.n_segments + 1);
    if (!rc) rc = d2h(o, &g->segment_name, d.d_segment_name, d.n_segments);
    if (!rc) rc = d2h(o, &g->edge_twin, d.d_edge_twin, dc.n_edges);
    if (rc) { katome_gfa_strands_free(g); return rc; }
    if (want.strands) *want.strands = g;
    rc = want.path ? katome_gfa_strands_save(g, want.path) : KATOME_OK;
    if (!want.strands) katome_gfa_strands_free(g);
    return rc;
}
static int gfa_to_host(katome_builder* b, uint64_t read_bytes, const GfaWant& want, const char* stages, uint64_t genome_len) {
    katome_dev_graph dg;
    if (stages && *stages && !b->first_seen) { set_error("stages after the build need KATOME_FLAG_FIRST_SEEN_ORDER"); return KATOME_E_ARG; }
    KCHECK(katome_dev_finalize(b, &dg, nullptr));
    if (b->s.flags & KATOME_FLAG_REMOVE_DEAD_PATHS) KCHECK(katome_dev_remove_dead_paths(b, &dg, nullptr, nullptr));
    KCHECK(run_stages(stages, BuilderStages{b, genome_len}));
    katome_dev_contigs dc;
    KCHECK(katome_dev_shrink(b, &dc, nullptr));
    if (want.merge) return gfa_strands_to_host(b, dc, read_bytes, want);
    katome_dev_gfa dgfa;
    KCHECK(katome_dev_contigs_gfa(b, &dc, &dgfa, nullptr));
    GfaOwner* o = new (std::nothrow) GfaOwner();
    if (!o) { set_error("out of host memory"); return KATOME_E_OOM; }
    memset(&o->g, 0, sizeof o->g);
    katome_gfa* g = &o->g;
    g->n_segments = dgfa.n_segments; g->n_links = dgfa.n_links; g->text_bytes = dgfa.text_bytes; g->read_bytes = read_bytes; g->k = b->s.k;
    int rc = d2h(o, &g->text, dgfa.d_text, dgfa.text_bytes);
    if (!rc) rc = d2h(o, &g->segment_off, dgfa.d_segment_off, dgfa.n_segments);
    if (!rc) rc = d2h(o, &g->link_first, dgfa.d_link_first, dgfa.n_segments + 1);
    if (rc) { katome_gfa_free(g); return rc; }
    if (want.out) *want.out = g;
    rc = want.path ? katome_gfa_save(g, want.path) : KATOME_OK;
    if (!want.out) katome_gfa_free(g);
    return rc;
}

// what a host entry hands back: the graph, the graph after shrink, the assembly, the unitigs' numbers (and their file), or the GFA
struct Finish {
    katome_graph** graph; katome_contigs** contigs;
    AssembleWant assemble{nullptr, nullptr}; bool assembling = false;
    UnitigsWant unitigs{nullptr, nullptr}; bool want_unitigs = false;
    GfaWant gfa{nullptr, nullptr}; bool want_gfa = false;
    const char* stages = nullptr; uint64_t genome_len = 0;
    uint32_t shrink_mode = KATOME_SHRINK_AUTO;
    katome_stats* stage_stats = nullptr;      // katome_build_*_staged_stats: the graph described before the first stage and after each
    int operator()(katome_builder* b, uint64_t read_bytes) const {
        if (assembling) return assembly_to_host(b, read_bytes, assemble, genome_len);
        if (want_unitigs) return unitigs_to_host(b, read_bytes, unitigs, stages, genome_len);
        if (want_gfa) return gfa_to_host(b, read_bytes, gfa, stages, genome_len);
        return contigs ? contigs_to_host(b, read_bytes, contigs, shrink_mode) : graph_to_host(b, read_bytes, graph, stages, genome_len, stage_stats);
    }
};

// records per extraction batch: bounded by a slice of free device memory
static uint64_t batch_records(uint32_t nw) {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return 1ull << 24;
    free_b += dev_cached_bytes();
    uint64_t r = (uint64_t)(free_b / 8) / (8ull * nw);
    return std::min<uint64_t>(std::max<uint64_t>(r, 1ull << 20), 1ull << 30);
}

struct RankShrunk {                                              // one rank's part of a result of katome_dist_shrink, on the host
    std::vector<uint64_t> src, dst, off, head, nid, nkey;
    std::vector<uint32_t> weight, kmers;
    std::vector<uint8_t> label;
    uint64_t total_edges = 0, total_nodes = 0;
    uint32_t key_words = 1;
};
static int shrunk_to_host(katome_dist_builder* d, RankShrunk& P, hipStream_t stream) {
    katome_dist_contigs c;
    KCHECK(katome_dist_shrink(d, &c, nullptr, stream));
    const uint64_t H = c.n_edges, NK = c.n_nodes, nw = c.key_words;
    try {
        P.src.resize(H); P.dst.resize(H); P.off.resize(H + 1); P.head.resize(H); P.nid.resize(NK); P.nkey.resize(NK * nw);
        P.weight.resize(H); P.kmers.resize(H); P.label.resize(c.label_bytes);
    } catch (const std::bad_alloc&) { set_error("out of host memory"); return KATOME_E_OOM; }
    KCHECK(copy_down({{P.src.data(), c.d_edge_src, H * 8}, {P.dst.data(), c.d_edge_dst, H * 8}, {P.off.data(), c.d_edge_label_off, (H + 1) * 8},
                      {P.head.data(), c.d_edge_head_id, H * 8}, {P.nid.data(), c.d_node_id, NK * 8}, {P.nkey.data(), c.d_node_key, NK * 8 * nw},
                      {P.weight.data(), c.d_edge_weight, H * 4}, {P.kmers.data(), c.d_edge_kmers, H * 4}, {P.label.data(), c.d_edge_label, c.label_bytes}},
                     stream));
    P.total_edges = c.total_edges; P.total_nodes = c.total_nodes; P.key_words = c.key_words;
    return KATOME_OK;
}
// the ranks' parts as one katome_contigs: edges in the order of their head edges' global indices, nodes at their new ids
static int assemble_shrunk(std::vector<RankShrunk>& parts, uint32_t k, uint64_t read_bytes, katome_contigs** out) {
    const uint32_t nw = parts.empty() ? 1 : parts[0].key_words;
    const uint64_t TE = parts.empty() ? 0 : parts[0].total_edges, TN = parts.empty() ? 0 : parts[0].total_nodes;
    std::vector<std::pair<uint64_t, std::pair<uint32_t, uint32_t>>> order;          // (head id, (rank, index there))
    uint64_t lb = 0;
    try {
        order.reserve(TE);
        for (size_t r = 0; r < parts.size(); ++r)
            for (uint64_t i = 0; i < parts[r].head.size(); ++i) order.push_back({parts[r].head[i], {(uint32_t)r, (uint32_t)i}});
    } catch (const std::bad_alloc&) { set_error("out of host memory"); return KATOME_E_OOM; }
    std::sort(order.begin(), order.end());
    for (auto& p : parts) lb += p.label.size();
    ContigsOwner* o = new (std::nothrow) ContigsOwner();
    if (!o) { set_error("out of host memory"); return KATOME_E_OOM; }
    memset(&o->c, 0, sizeof o->c);
    katome_contigs* c = &o->c;
    bool oom = false;
    uint64_t* src = (uint64_t*)take(o, TE * 8, &oom); uint64_t* dst = (uint64_t*)take(o, TE * 8, &oom); uint32_t* w = (uint32_t*)take(o, TE * 4, &oom);
    uint32_t* km = (uint32_t*)take(o, TE * 4, &oom); uint64_t* off = (uint64_t*)take(o, (TE + 1) * 8, &oom); uint8_t* lab = (uint8_t*)take(o, lb, &oom);
    uint64_t* nkey = (uint64_t*)take(o, TN * 8 * nw, &oom); uint8_t* seen = (uint8_t*)take(o, TN, &oom);
    if (oom) { katome_contigs_free(c); set_error("out of host memory"); return KATOME_E_OOM; }
    bool bad = order.size() != TE;
    uint64_t at = 0;
    off[0] = 0;
    for (uint64_t i = 0; i < order.size() && !bad; ++i) {
        const RankShrunk& P = parts[order[i].second.first];
        const uint32_t j = order[i].second.second;
        const uint64_t n = P.off[j + 1] - P.off[j];
        src[i] = P.src[j]; dst[i] = P.dst[j]; w[i] = P.weight[j]; km[i] = P.kmers[j];
        if (at + n > lb || src[i] >= TN || dst[i] >= TN) { bad = true; break; }
        memcpy(lab + at, P.label.data() + P.off[j], n);
        at += n; off[i + 1] = at;
    }
    memset(seen, 0, TN);
    uint64_t placed = 0;
    for (auto& P : parts)
        for (uint64_t j = 0; j < P.nid.size() && !bad; ++j) {
            const uint64_t id = P.nid[j];
            if (id >= TN || seen[id]) { bad = true; break; }
            seen[id] = 1; ++placed;
            for (uint32_t q = 0; q < nw; ++q) nkey[id * nw + q] = P.nkey[j * nw + q];
        }
    if (bad || placed != TN) { katome_contigs_free(c); set_error("sharded shrink: the ranks' merged edges or nodes do not fit together"); return KATOME_E_DEVICE; }
    c->n_nodes = TN; c->n_edges = TE; c->label_bytes = lb; c->read_bytes = read_bytes; c->k = k; c->key_words = nw;
    c->edge_src = src; c->edge_dst = dst; c->edge_weight = w; c->edge_kmers = km; c->edge_label_off = off; c->edge_label = lab; c->node_key = nkey;
    *out = c;
    return KATOME_OK;
}

// ---- settings.n_devices > 1: the sharded build (dist.hip) with the ranks as host threads of this call, one per GPU -----------
// Reads are split contiguously by index; every rank copies its own share to its GPU (`add_reads(rank, world, builder, stream)`:
// fixed- or variable-length reads).  Which way the build goes from there: multi_route.h.
namespace {
struct MultiBuild {                      // what the rank threads of one call share
    const katome_settings* s; const Finish& finish; const MultiRoute& route; uint64_t read_bytes;
    std::shared_ptr<LocalGroup> sync;    // host rendezvous of the rank threads, whatever moves the data
    std::vector<int> rc; std::vector<std::string> err;
    std::vector<uint64_t> n_edges;       // by packed key: the ranks' edge counts (the host arrays are their shares one after the other)
    GraphOwner* owner = nullptr; int alloc_rc = KATOME_OK;      // the host graph every rank copies its share into (rank 0 makes it)
    std::vector<RankShrunk> shrunk;
};
}  // namespace

// A rank whose step failed must not leave the others waiting inside the next collective: everybody meets here first, and a
// failed rank has poisoned the meeting.
static int meet(MultiBuild& mb) {
    if (mb.sync->barrier()) return KATOME_OK;
    set_error("%s", RANK_GAVE_UP);
    return KATOME_E_DEVICE;
}

// the graph gathered to rank 0, which finishes it as a one-GPU build would (the stages and the shrink the caller asked for run there)
static int gathered_finish(MultiBuild& mb, int r, katome_dist_builder* d, hipStream_t stream) {
    katome_builder* root = nullptr;
    const auto t_gather = std::chrono::steady_clock::now();
    KCHECK(katome_dist_gather(d, 0, &root, stream));
    if (r != 0) return KATOME_OK;
    root->s.flags = mb.s->flags; root->s.min_weight = mb.s->min_weight;
    Finish f = mb.finish;
    if (mb.route.gather_fast) f.shrink_mode = KATOME_SHRINK_FAST;
    const int rc = f(root, mb.read_bytes);
    if (mb.route.gather_fast && getenv("KATOME_DIST_SHRINK_TRACE"))
        fprintf(stderr, "[katome_dist_shrink] gather + fast form on rank 0: %.2f ms (result in host arrays)\n",
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_gather).count());
    return rc;
}

// rank 0, between the two meetings: the host graph of the whole result (mb.owner; nullptr and mb.alloc_rc: no memory for it)
static void alloc_shared_graph(MultiBuild& mb, const katome_dist_graph& g) {
    std::vector<HostCopy> arrays;
    mb.alloc_rc = new_host_graph(g.total_nodes, g.total_edges, mb.s->k, g.key_words, g.label_stride, g.d_edge_age != nullptr, mb.read_bytes,
                                 &mb.owner, arrays);
    if (mb.alloc_rc == KATOME_OK) for (const HostCopy& a : arrays) host_result_touch(a.h, a.bytes);
}

// by packed key the host arrays are the ranks' shares one after the other: rank r's edges start where those of the ranks
// before it end, its nodes at node_base
static int copy_out_by_key(MultiBuild& mb, int r, const katome_dist_graph& g, hipStream_t stream) {
    const katome_graph* hg = &mb.owner->g;
    uint64_t e0 = 0;
    for (int p = 0; p < r; ++p) e0 += mb.n_edges[p];
    const uint64_t E = g.n_edges, N = g.n_nodes;
    const uint32_t nwk = g.key_words, ls = g.label_stride;
    return copy_down({{const_cast<uint64_t*>(hg->edge_src) + e0, g.d_edge_src, E * 8}, {const_cast<uint64_t*>(hg->edge_dst) + e0, g.d_edge_dst, E * 8},
                      {const_cast<uint32_t*>(hg->edge_weight) + e0, g.d_edge_weight, E * 4},
                      {const_cast<uint8_t*>(hg->edge_label) + e0 * ls, g.d_edge_label, E * (size_t)ls},
                      {const_cast<uint64_t*>(hg->edge_key) + e0 * nwk, g.d_edge_key, E * 8 * nwk},
                      {const_cast<uint64_t*>(hg->node_key) + g.node_base * nwk, g.d_node_key, N * 8 * nwk}},
                     stream);
}

// in the reference's numbering every edge and node goes to its petgraph index: the rank's share comes over in its own order
// and is placed on the host
static int copy_out_by_index(MultiBuild& mb, const katome_dist_graph& g, hipStream_t stream) {
    const katome_graph* hg = &mb.owner->g;
    const bool pruned = g.d_edge_age != nullptr;      // (the ages come along once a stage that may remove edges has run)
    const uint64_t E = g.n_edges, N = g.n_nodes;
    const uint32_t nwk = g.key_words, ls = g.label_stride;
    std::vector<uint64_t> id(E), src(E), dst(E), key(E * nwk), nid(N), nkey(N * nwk), age(pruned ? E : 0);
    std::vector<uint32_t> w(E);
    std::vector<uint8_t> lab(E * (size_t)ls);
    KCHECK(copy_down({{id.data(), g.d_edge_id, E * 8}, {src.data(), g.d_edge_src, E * 8}, {dst.data(), g.d_edge_dst, E * 8},
                      {w.data(), g.d_edge_weight, E * 4}, {lab.data(), g.d_edge_label, E * (size_t)ls}, {key.data(), g.d_edge_key, E * 8 * nwk},
                      {nid.data(), g.d_node_id, N * 8}, {nkey.data(), g.d_node_key, N * 8 * nwk}, {age.data(), g.d_edge_age, age.size() * 8}},
                     stream));
    uint64_t* h_src = const_cast<uint64_t*>(hg->edge_src); uint64_t* h_dst = const_cast<uint64_t*>(hg->edge_dst);
    uint32_t* h_w = const_cast<uint32_t*>(hg->edge_weight); uint8_t* h_lab = const_cast<uint8_t*>(hg->edge_label);
    uint64_t* h_key = const_cast<uint64_t*>(hg->edge_key); uint64_t* h_nkey = const_cast<uint64_t*>(hg->node_key);
    uint32_t* h_age = const_cast<uint32_t*>(hg->edge_age);
    bool bad = false;
    for (uint64_t i = 0; i < E; ++i) {
        const uint64_t at = id[i];
        if (at >= hg->n_edges) { bad = true; break; }
        h_src[at] = src[i]; h_dst[at] = dst[i]; h_w[at] = w[i];
        memcpy(h_lab + at * ls, lab.data() + i * (size_t)ls, ls);
        for (uint32_t q = 0; q < nwk; ++q) h_key[at * nwk + q] = key[i * nwk + q];
        if (pruned) { if (age[i] > 0xFFFFFFFFull) bad = true; h_age[at] = (uint32_t)age[i]; }
    }
    for (uint64_t j = 0; j < N && !bad; ++j) {
        const uint64_t at = nid[j];
        if (at >= hg->n_nodes) { bad = true; break; }
        for (uint32_t q = 0; q < nwk; ++q) h_nkey[at * nwk + q] = nkey[j * nwk + q];
    }
    if (bad) { set_error("sharded build: an index does not fit the host result (katome_graph.edge_age is 32 bits wide)"); return KATOME_E_UNSUPPORTED; }
    return KATOME_OK;
}

// FASTA headers ">katome_<i>\n" of contigs 0 .. n - 1 take this many bytes (9 + the digits of i)
static uint64_t fasta_header_bytes(uint64_t n) {
    uint64_t bytes = 0, lo = 0, digits = 1;
    for (uint64_t hi = 10; lo < n; lo = hi, hi = hi > ~0ull / 10 ? ~0ull : hi * 10, ++digits) bytes += (std::min(hi, n) - lo) * (9 + digits);
    return bytes;
}

// katome_unitigs_* on the shares, after the stages: the sharded shrink, its text, the stats of all ranks' contigs and the file, every
// call collective; rank 0 fills the caller's struct.  Every rank takes the same way through it: the statuses are agreed inside the calls
static int sharded_unitigs(MultiBuild& mb, int r, int n, katome_dist_builder* d, hipStream_t stream) {
    const UnitigsWant& want = mb.finish.unitigs;
    katome_dist_shrink_stats ss;
    const bool coverage = want.gfa && (mb.s->flags & KATOME_FLAG_PATH_COVERAGE);      // (the same settings on every rank)
    katome_dev_coverage cov;
    if (coverage) KCHECK(katome_dist_shrink_coverage(d, nullptr, &cov, &ss, stream));
    else KCHECK(katome_dist_shrink(d, nullptr, &ss, stream));
    if (want.gfa) {                                                  // the graph: the join across ranks, the numbered text, the file
        katome_dist_gfa g;
        if (coverage) KCHECK(katome_dist_contigs_gfa_coverage(d, &g, stream));
        else KCHECK(katome_dist_contigs_gfa(d, &g, stream));
        uint64_t bases[1] = {0};                                     // (the k-mers on all ranks' merged edges: their bases are k - 1 more each)
        KCHECK(dist_gfa_total_kmers(d, bases, stream));
        if (r == 0) {
            katome_unitigs_gfa* u = want.gfa;
            u->n_segments = g.total_segments; u->n_links = g.total_links; u->text_bytes = g.total_text_bytes; u->read_bytes = mb.read_bytes;
            u->k = mb.s->k; u->n_devices = (uint32_t)n;
            u->total_bases = bases[0] + g.total_segments * (uint64_t)(mb.s->k - 1);
            u->longest = g.total_segments ? ss.longest_path + mb.s->k - 1 : 0;
            u->shrink = ss;
        }
        return want.path ? katome_dist_gfa_save(d, &g, want.path) : KATOME_OK;
    }
    katome_dist_assembly a;
    KCHECK(katome_dist_contigs_text(d, KATOME_TEXT_FASTA, &a, stream));
    katome_contig_stats cs;
    const int stats_rc = katome_dist_contig_stats(d, mb.finish.genome_len, &cs, stream);
    if (stats_rc && stats_rc != KATOME_E_ARG) return stats_rc;       // (KATOME_E_ARG: a tipping point of 0 -- the file is written all the same)
    const std::string stats_err = stats_rc ? get_error() : "";
    if (r == 0) {
        katome_unitigs* u = want.out;
        u->n_contigs = a.total_contigs; u->text_bytes = a.total_text_bytes; u->read_bytes = mb.read_bytes; u->k = mb.s->k; u->n_devices = (uint32_t)n;
        // (the FASTA text is the headers, the bases and one newline per contig)
        u->total_bases = a.total_text_bytes - a.total_contigs - fasta_header_bytes(a.total_contigs);
        u->longest = a.total_contigs ? ss.longest_path + mb.s->k - 1 : 0;
        u->stats = cs; u->shrink = ss;
    }
    if (want.path) KCHECK(katome_dist_contigs_save(d, &a, want.path));
    if (stats_rc) set_error("%s", stats_err.c_str());
    return stats_rc;
}

// one rank from its reads to its share of the result; the two meetings and the order of everything between them are what keeps
// a failing rank from leaving the others waiting
template <class AddReads>
static int rank_build(MultiBuild& mb, int r, int n, katome_dist_builder* d, const AddReads& add_reads, hipStream_t stream) {
    const MultiRoute& route = mb.route;
    KCHECK(add_reads(r, n, d, stream));
    KCHECK(meet(mb));
    katome_dist_graph g;
    KCHECK(katome_dist_finalize(d, &g, stream));
    // (every rank sees the same totals and the same plan: they all take the same route)
    if (route.gathers(g.total_edges, g.total_nodes)) return gathered_finish(mb, r, d, stream);
    if (route.sharded_dead_paths()) KCHECK(katome_dist_remove_dead_paths(d, &g, nullptr, stream));
    if (route.sharded_shrink) return shrunk_to_host(d, mb.shrunk[r], stream);
    if (route.unitigs) {
        if (route.sharded_stage_letters()) KCHECK(run_stages(mb.finish.stages, ShardedStages{d, &g, mb.s->min_weight, mb.finish.genome_len, stream}));
        return sharded_unitigs(mb, r, n, d, stream);
    }
    // (the whole graph's stats are the same on every rank: rank 0 writes the caller's array)
    auto describe = [&](size_t i) -> int {
        if (!mb.finish.stage_stats) return KATOME_OK;
        katome_stats st;
        KCHECK(katome_dist_graph_stats(d, &st, stream));
        if (r == 0) mb.finish.stage_stats[i] = st;
        return katome_dist_current_graph(d, &g);      // (the call may have rebuilt the links, which re-orders the rank's node arrays)
    };
    if (route.sharded_stage_letters()) KCHECK(run_stages(mb.finish.stages, ShardedStages{d, &g, mb.s->min_weight, mb.finish.genome_len, stream}, describe));
    else KCHECK(describe(0));
    mb.n_edges[r] = g.n_edges;
    KCHECK(meet(mb));
    if (r == 0) alloc_shared_graph(mb, g);
    KCHECK(meet(mb));
    if (!mb.owner) return mb.alloc_rc ? mb.alloc_rc : KATOME_E_OOM;
    return route.first_seen ? copy_out_by_index(mb, g, stream) : copy_out_by_key(mb, r, g, stream);
}

template <class AddReads>
static int rank_thread(MultiBuild& mb, int r, int n, int device, katome_comm* comm, const AddReads& add_reads) {
    KCHECK(use_device(device));
    hipStream_t stream = nullptr;
    KCHECK_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    katome_settings mine = *mb.s;
    mine.device = device;
    katome_dist_builder* d = nullptr;
    int rc = katome_dist_create(&mine, comm, &d);
    if (!rc) rc = rank_build(mb, r, n, d, add_reads, stream);
    if (d) katome_dist_destroy(d);
    dev_retire_stream(stream);
    (void)hipStreamDestroy(stream);
    return rc;
}

template <class AddReads>
static int build_multi(const katome_settings* s, const Finish& finish, uint64_t read_bytes, const AddReads& add_reads) {
    const int n = s->n_devices;
    const bool share = (s->flags & KATOME_FLAG_RANKS_SHARE_DEVICE) != 0;
    // (a GFA takes the assembly's route: gathered to the first GPU, where the stages, the shrink and the text run -- links cross ranks)
    const MultiRoute route = plan_multi_route(s->flags, finish.contigs != nullptr, finish.stages, finish.assembling || finish.want_gfa, finish.want_unitigs);
    if (n > KATOME_MAX_RANKS) { set_error("n_devices = %d: at most %d", n, KATOME_MAX_RANKS); return KATOME_E_UNSUPPORTED; }
    KCHECK(use_device(s->device));
    int n_visible = 0;
    KCHECK_HIP(hipGetDeviceCount(&n_visible));
    if (!share && s->device + n > n_visible) { set_error("n_devices = %d from device %d, but %d GPU(s) are visible", n, s->device, n_visible); return KATOME_E_DEVICE; }
    if (route.bad_arg && route.unitigs) {
        set_error("unitigs: stage letters and KATOME_FLAG_REMOVE_DEAD_PATHS need KATOME_FLAG_FIRST_SEEN_ORDER");
        return KATOME_E_ARG;
    }
    if (route.bad_arg) {
        set_error("n_devices > 1: shrink and the stages after the build need KATOME_FLAG_FIRST_SEEN_ORDER (they run on the graph gathered in the reference's numbering; KATOME_DIST_SHRINK=sharded shrinks a packed-key build)");
        return KATOME_E_ARG;
    }
    std::vector<int> devices(n);
    for (int r = 0; r < n; ++r) devices[r] = share ? s->device : s->device + r;
    std::vector<katome_comm*> comms(n, nullptr);
    MultiBuild mb{s, finish, route, read_bytes, std::make_shared<LocalGroup>(n)};
    std::shared_ptr<LocalGroup> group;                           // (the local transport's own rendezvous, poisoned with mb.sync)
    if (route.local_comm) {
        group = std::make_shared<LocalGroup>(n);
        for (int r = 0; r < n; ++r) KCHECK(make_local_comm(group, r, devices[r], &comms[r]));
    } else {
        KCHECK(make_rccl_comms_all(devices.data(), n, comms.data()));
    }
    mb.rc.assign(n, KATOME_OK); mb.err.resize(n); mb.n_edges.assign(n, 0);
    if (route.sharded_shrink) mb.shrunk.resize(n);
    std::vector<std::thread> threads;
    for (int r = 0; r < n; ++r)
        threads.emplace_back([&, r]() {
            mb.rc[r] = rank_thread(mb, r, n, devices[r], comms[r], add_reads);
            if (mb.rc[r]) { mb.err[r] = get_error(); mb.sync->poison(); if (group) group->poison(); }     // (ranks waiting at a host rendezvous give up)
        });
    for (auto& t : threads) t.join();
    for (int r = 0; r < n; ++r) katome_comm_destroy(comms[r]);
    // the first rank that failed by itself is the one reported, before any that gave up because of it
    int rc = KATOME_OK;
    for (const bool gave_up : {false, true})
        for (int r = 0; r < n && !rc; ++r)
            if (mb.rc[r] && (gave_up || mb.err[r] != RANK_GAVE_UP)) { rc = mb.rc[r]; set_error("rank %d of %d: %s", r, n, mb.err[r].c_str()); }
    if (rc == KATOME_OK && route.sharded_shrink) rc = assemble_shrunk(mb.shrunk, s->k, read_bytes, finish.contigs);
    if (mb.owner) {                                              // (the ranks' shares were copied out: no gathered route ran)
        if (rc == KATOME_OK && finish.graph) *finish.graph = &mb.owner->g;
        else katome_graph_free(&mb.owner->g);
    }
    return rc;
}

static int build_packed_multi(const katome_settings* s, const uint8_t* packed, uint64_t n_reads, uint32_t read_len,
                              const uint8_t* skip, const Finish& finish, uint64_t read_bytes) {
    const uint32_t stride = (read_len + 3) / 4;
    return build_multi(s, finish, read_bytes, [&](int r, int n, katome_dist_builder* d, hipStream_t stream) -> int {
        uint64_t first = 0, cnt = 0;
        katome_shard_range(n_reads, (uint32_t)n, (uint32_t)r, &first, &cnt);
        DevBuf d_packed(stream), d_skip(stream);
        KCHECK(d_packed.alloc(cnt * stride + 32));
        if (cnt && hipMemcpyAsync(d_packed.p, packed + first * stride, cnt * stride, hipMemcpyHostToDevice, stream) != hipSuccess) { set_error("H2D copy failed"); return KATOME_E_DEVICE; }
        if (skip) {
            KCHECK(d_skip.alloc(cnt + 16));
            if (cnt && hipMemcpyAsync(d_skip.p, skip + first, cnt, hipMemcpyHostToDevice, stream) != hipSuccess) { set_error("H2D copy failed"); return KATOME_E_DEVICE; }
        }
        return katome_dist_add_reads(d, d_packed.as<uint8_t>(), first, cnt, read_len, skip ? d_skip.as<uint8_t>() : nullptr, 0, stream);
    });
}

// Reads of varying length on the sharded route: split contiguously by index, every rank copies its slice (its bytes, its byte
// offsets rebased to the slice, its lengths) and starts at the global window of its first read.  Every rank takes part in the
// collective katome_dist_add_reads_var, a rank without reads too.
static int build_var_multi(const katome_settings* s, const HostReads& hr, const Finish& finish) {
    const int n = s->n_devices;
    std::vector<uint64_t> first_window(std::max(n, 1) + 1, 0);
    for (int r = 0; r < n; ++r) {                        // (each rank's window offset: the windows of the ranks before it)
        uint64_t first = 0, cnt = 0, w = 0;
        katome_shard_range(hr.n_reads, (uint32_t)n, (uint32_t)r, &first, &cnt);
        for (uint64_t i = first; i < first + cnt; ++i) w += hr.len[i] >= s->k ? hr.len[i] - s->k + 1 : 0;
        first_window[r + 1] = first_window[r] + w;
    }
    // (KATOME_DIST_VAR_BATCH_WINDOWS: tests -- many small batches)
    const uint64_t batch = getenv("KATOME_DIST_VAR_BATCH_WINDOWS") ? strtoull(getenv("KATOME_DIST_VAR_BATCH_WINDOWS"), nullptr, 10) : 0;
    return build_multi(s, finish, hr.read_bytes, [&](int r, int n, katome_dist_builder* d, hipStream_t stream) -> int {
        uint64_t first = 0, cnt = 0;
        katome_shard_range(hr.n_reads, (uint32_t)n, (uint32_t)r, &first, &cnt);
        const uint64_t b0 = hr.byte_off[first], bytes = hr.byte_off[first + cnt] - b0;
        std::vector<uint64_t> off(cnt + 1, 0);
        for (uint64_t i = 0; i < cnt; ++i) off[i] = hr.byte_off[first + i] - b0;
        off[cnt] = bytes;
        DevBuf d_packed(stream), d_off(stream), d_len(stream);
        KCHECK(d_packed.alloc(bytes + 32)); KCHECK(d_off.alloc((cnt + 1) * 8)); KCHECK(d_len.alloc(cnt * 4 + 16));
        if (cnt && (hipMemcpyAsync(d_packed.p, hr.packed + b0, bytes, hipMemcpyHostToDevice, stream) != hipSuccess ||
                    hipMemcpyAsync(d_off.p, off.data(), (cnt + 1) * 8, hipMemcpyHostToDevice, stream) != hipSuccess ||
                    hipMemcpyAsync(d_len.p, hr.len + first, cnt * 4, hipMemcpyHostToDevice, stream) != hipSuccess)) { set_error("H2D copy failed"); return KATOME_E_DEVICE; }
        // (the copies come from pageable host memory the call owns until it returns; the reads are taken before that)
        return katome_dist_add_reads_var(d, d_packed.as<uint8_t>(), bytes, d_off.as<u64>(), d_len.as<u32>(), cnt, first_window[r], batch, stream);
    });
}

static int build_packed_impl(const katome_settings* s, const uint8_t* packed, uint64_t n_reads, uint32_t read_len,
                             const uint8_t* skip, const Finish& finish, const uint64_t* read_bytes_override = nullptr) {
    if (!s || (!packed && n_reads)) { set_error("null argument"); return KATOME_E_ARG; }
    KCHECK(check_k(s->k));
    // (KATOME_FORCE_SHARDED=1: one GPU through the sharded route as well -- a world of one rank with the transport a larger
    // world would use; testing)
    if ((s->n_devices > 1 || (s->n_devices == 1 && getenv("KATOME_FORCE_SHARDED"))) && n_reads && read_len >= s->k) {
        uint64_t read_bytes = 0;
        if (read_bytes_override) read_bytes = *read_bytes_override;
        else for (uint64_t r = 0; r < n_reads; ++r) if (!skip || !skip[r]) read_bytes += read_len;
        return build_packed_multi(s, packed, n_reads, read_len, skip, finish, read_bytes);
    }
    if (n_reads && read_len < s->k) {
        // only an ACCEPTED read can be too short (builder.rs:155-158 filters first)
        bool any = !skip;
        for (uint64_t r = 0; skip && r < n_reads && !any; ++r) any = skip[r] == 0;
        if (any) { set_error("Read is too short!"); return KATOME_E_SHORT_READ; }
        n_reads = 0;
    }
    katome_builder* b = nullptr;
    KCHECK(katome_builder_create(s, &b));
    build_lap("", true);
    int rc = KATOME_OK;
    do {
        const uint32_t stride = (read_len + 3) / 4, W = read_len >= s->k ? read_len - s->k + 1 : 0;
        uint64_t read_bytes = 0;
        for (uint64_t r = 0; r < n_reads; ++r) if (!skip || !skip[r]) read_bytes += read_len;
        DevBuf d_packed, d_skip, d_rec;
        if ((rc = d_packed.alloc(n_reads * stride + 32))) break;
        if (n_reads && hipMemcpy(d_packed.p, packed, n_reads * stride, hipMemcpyHostToDevice) != hipSuccess) { set_error("H2D copy failed"); rc = KATOME_E_DEVICE; break; }
        if (skip) {
            if ((rc = d_skip.alloc(n_reads + 16))) break;
            if (n_reads && hipMemcpy(d_skip.p, skip, n_reads, hipMemcpyHostToDevice) != hipSuccess) { set_error("H2D copy failed"); rc = KATOME_E_DEVICE; break; }
        }
        if (n_reads && W) {
            uint64_t reads_per_batch = std::max<uint64_t>(batch_records(b->nw) / W, 64);
            reads_per_batch = (reads_per_batch / 64) * 64;       // keeps batch starts 16-byte aligned
            if ((rc = d_rec.alloc(std::min(reads_per_batch, n_reads) * W * 8 * b->nw + 16))) break;
            uint32_t span = 1, tiles = 0, rest = 0;
            katome_tile_plan(s->k, read_len, &span, &tiles, &rest);
            for (uint64_t r0 = 0; r0 < n_reads && !rc; r0 += reads_per_batch) {
                const uint64_t nr = std::min(reads_per_batch, n_reads - r0);
                if (span > 1) {       // tiled counting: W/span tile records per read, then the windows that are left over
                    rc = katome_dev_count_tiles(b, d_packed.as<uint8_t>() + r0 * stride, nr, read_len, span,
                                                skip ? d_skip.as<uint8_t>() + r0 : nullptr, nullptr);
                    if (!rc && rest) {
                        rc = katome_dev_extract_remainder(b, d_packed.as<uint8_t>() + r0 * stride, nr, read_len, span,
                                                          skip ? d_skip.as<uint8_t>() + r0 : nullptr, d_rec.as<u64>(), nullptr);
                        if (!rc) rc = katome_dev_insert(b, d_rec.as<u64>(), nr * rest, nullptr);
                    }
                } else {
                    rc = katome_dev_extract_fixed(b, d_packed.as<uint8_t>() + r0 * stride, nr, read_len,
                                                  skip ? d_skip.as<uint8_t>() + r0 : nullptr, d_rec.as<u64>(), nullptr);
                    if (!rc) rc = katome_dev_insert(b, d_rec.as<u64>(), nr * W, nullptr);
                }
            }
            if (rc) break;
        }
        d_rec.release(); d_packed.release(); d_skip.release();
        rc = finish(b, read_bytes_override ? *read_bytes_override : read_bytes);
    } while (0);
    katome_builder_destroy(b);
    return rc;
}

extern "C" {

int katome_build_packed(const katome_settings* s, const uint8_t* packed, uint64_t n_reads, uint32_t read_len,
                        const uint8_t* skip, katome_graph** out) {
    if (!out) { set_error("null argument"); return KATOME_E_ARG; }
    *out = nullptr;
    return build_packed_impl(s, packed, n_reads, read_len, skip, Finish{out, nullptr});
}
int katome_build_packed_staged(const katome_settings* s, const uint8_t* packed, uint64_t n_reads, uint32_t read_len,
                               const uint8_t* skip, const char* stages, uint64_t original_genome_length, katome_graph** out) {
    if (!out) { set_error("null argument"); return KATOME_E_ARG; }
    *out = nullptr;
    Finish f{out, nullptr};
    f.stages = stages; f.genome_len = original_genome_length;
    return build_packed_impl(s, packed, n_reads, read_len, skip, f);
}
int katome_build_packed_staged_stats(const katome_settings* s, const uint8_t* packed, uint64_t n_reads, uint32_t read_len, const uint8_t* skip,
                                     const char* stages, uint64_t original_genome_length, katome_stats* stage_stats, katome_graph** out) {
    if (!out || !stage_stats) { set_error("null argument"); return KATOME_E_ARG; }
    *out = nullptr;
    Finish f{out, nullptr};
    f.stages = stages; f.genome_len = original_genome_length; f.stage_stats = stage_stats;
    return build_packed_impl(s, packed, n_reads, read_len, skip, f);
}
int katome_assemble_packed(const katome_settings* s, const uint8_t* packed, uint64_t n_reads, uint32_t read_len, const uint8_t* skip,
                           uint64_t original_genome_length, const char* out_path, katome_assembly** out) {
    if (!out && !out_path) { set_error("null argument"); return KATOME_E_ARG; }
    if (out) *out = nullptr;
    Finish f{nullptr, nullptr};
    f.assemble = AssembleWant{out, out_path}; f.assembling = true; f.genome_len = original_genome_length;
    return build_packed_impl(s, packed, n_reads, read_len, skip, f);
}
// katome_assemble_gfa_*: the assembly and the GFA of its shrunk graph with the contigs as P lines (the same check on both routes)
static int assemble_gfa_finish(uint64_t genome_len, const char* fasta_path, const char* gfa_path, katome_assembly** asm_out, katome_gfa_paths** gfa_out, Finish& f) {
    if (asm_out) *asm_out = nullptr;
    if (gfa_out) *gfa_out = nullptr;
    if (!fasta_path && !gfa_path && !asm_out && !gfa_out) { set_error("null argument"); return KATOME_E_ARG; }
    f.assemble = AssembleWant{asm_out, fasta_path, true, gfa_out, gfa_path}; f.assembling = true; f.genome_len = genome_len;
    return KATOME_OK;
}
int katome_assemble_gfa_packed(const katome_settings* s, const uint8_t* packed, uint64_t n_reads, uint32_t read_len, const uint8_t* skip,
                               uint64_t original_genome_length, const char* fasta_path, const char* gfa_path, katome_assembly** asm_out,
                               katome_gfa_paths** gfa_out) {
    Finish f{nullptr, nullptr};
    KCHECK(assemble_gfa_finish(original_genome_length, fasta_path, gfa_path, asm_out, gfa_out, f));
    return build_packed_impl(s, packed, n_reads, read_len, skip, f);
}
// katome_assemble_gfa_strands_*: the same with strand twins merged
static int assemble_gfa_strands_finish(uint64_t genome_len, const char* fasta_path, const char* gfa_path, katome_assembly** asm_out,
                                       katome_gfa_strand_paths** gfa_out, Finish& f) {
    if (asm_out) *asm_out = nullptr;
    if (gfa_out) *gfa_out = nullptr;
    if (!fasta_path && !gfa_path && !asm_out && !gfa_out) { set_error("null argument"); return KATOME_E_ARG; }
    f.assemble = AssembleWant{asm_out, fasta_path, true, nullptr, gfa_path, true, gfa_out}; f.assembling = true; f.genome_len = genome_len;
    return KATOME_OK;
}
int katome_assemble_gfa_strands_packed(const katome_settings* s, const uint8_t* packed, uint64_t n_reads, uint32_t read_len, const uint8_t* skip,
                                       uint64_t original_genome_length, const char* fasta_path, const char* gfa_path, katome_assembly** asm_out,
                                       katome_gfa_strand_paths** gfa_out) {
    Finish f{nullptr, nullptr};
    KCHECK(assemble_gfa_strands_finish(original_genome_length, fasta_path, gfa_path, asm_out, gfa_out, f));
    return build_packed_impl(s, packed, n_reads, read_len, skip, f);
}
// katome_assemble_unique_*: the assembly and the strand-unique form of its contigs
static int assemble_unique_finish(uint64_t genome_len, const char* fasta_path, const char* unique_path, katome_assembly** asm_out,
                                  katome_unique_assembly** unique_out, Finish& f) {
    if (asm_out) *asm_out = nullptr;
    if (unique_out) *unique_out = nullptr;
    if (!fasta_path && !unique_path && !asm_out && !unique_out) { set_error("null argument"); return KATOME_E_ARG; }
    f.assemble = AssembleWant{asm_out, fasta_path};
    f.assemble.unique = true; f.assemble.unique_out = unique_out; f.assemble.unique_path = unique_path;
    f.assembling = true; f.genome_len = genome_len;
    return KATOME_OK;
}
int katome_assemble_unique_packed(const katome_settings* s, const uint8_t* packed, uint64_t n_reads, uint32_t read_len, const uint8_t* skip,
                                  uint64_t original_genome_length, const char* fasta_path, const char* unique_path, katome_assembly** asm_out,
                                  katome_unique_assembly** unique_out) {
    Finish f{nullptr, nullptr};
    KCHECK(assemble_unique_finish(original_genome_length, fasta_path, unique_path, asm_out, unique_out, f));
    return build_packed_impl(s, packed, n_reads, read_len, skip, f);
}
// (the same check on every route: the stages work on the links of a first-seen build)
static int unitigs_refusal(const katome_settings* s, const char* stages) {
    if (s && !(s->flags & KATOME_FLAG_FIRST_SEEN_ORDER) && ((stages && *stages) || (s->flags & KATOME_FLAG_REMOVE_DEAD_PATHS))) {
        set_error("unitigs: stage letters and KATOME_FLAG_REMOVE_DEAD_PATHS need KATOME_FLAG_FIRST_SEEN_ORDER");
        return KATOME_E_ARG;
    }
    return KATOME_OK;
}
static int unitigs_finish(const katome_settings* s, const char* stages, uint64_t genome_len, const char* out_path, katome_unitigs* out, Finish& f) {
    if (!out) { set_error("null argument"); return KATOME_E_ARG; }
    memset(out, 0, sizeof *out);
    KCHECK(unitigs_refusal(s, stages));
    f.unitigs = UnitigsWant{out, out_path}; f.want_unitigs = true; f.stages = stages; f.genome_len = genome_len;
    return KATOME_OK;
}
int katome_unitigs_packed(const katome_settings* s, const uint8_t* packed, uint64_t n_reads, uint32_t read_len, const uint8_t* skip,
                          const char* stages, uint64_t original_genome_length, const char* out_path, katome_unitigs* out) {
    Finish f{nullptr, nullptr};
    KCHECK(unitigs_finish(s, stages, original_genome_length, out_path, out, f));
    return build_packed_impl(s, packed, n_reads, read_len, skip, f);
}
// katome_unitigs_gfa_*: the unitigs route with the graph as its ending
static int unitigs_gfa_finish(const katome_settings* s, const char* stages, uint64_t genome_len, const char* out_path, katome_unitigs_gfa* out, Finish& f) {
    if (!out) { set_error("null argument"); return KATOME_E_ARG; }
    memset(out, 0, sizeof *out);
    KCHECK(unitigs_refusal(s, stages));
    f.unitigs = UnitigsWant{nullptr, out_path, out}; f.want_unitigs = true; f.stages = stages; f.genome_len = genome_len;
    return KATOME_OK;
}
int katome_unitigs_gfa_packed(const katome_settings* s, const uint8_t* packed, uint64_t n_reads, uint32_t read_len, const uint8_t* skip,
                              const char* stages, uint64_t original_genome_length, const char* out_path, katome_unitigs_gfa* out) {
    Finish f{nullptr, nullptr};
    KCHECK(unitigs_gfa_finish(s, stages, original_genome_length, out_path, out, f));
    return build_packed_impl(s, packed, n_reads, read_len, skip, f);
}
// (the same check on every route, before any GPU work)
static int gfa_finish(const katome_settings* s, const char* stages, uint64_t genome_len, const char* out_path, katome_gfa** out, Finish& f) {
    if (!out && !out_path) { set_error("null argument"); return KATOME_E_ARG; }
    if (out) *out = nullptr;
    if (s && !(s->flags & KATOME_FLAG_FIRST_SEEN_ORDER) && stages && *stages) {
        set_error("stages after the build need KATOME_FLAG_FIRST_SEEN_ORDER");
        return KATOME_E_ARG;
    }
    f.gfa = GfaWant{out, out_path}; f.want_gfa = true; f.stages = stages; f.genome_len = genome_len;
    return KATOME_OK;
}
static int gfa_strands_finish(const katome_settings* s, const char* stages, uint64_t genome_len, const char* out_path, katome_gfa_strands** out, Finish& f) {
    if (!out && !out_path) { set_error("null argument"); return KATOME_E_ARG; }
    if (out) *out = nullptr;
    katome_gfa* none = nullptr;
    KCHECK(gfa_finish(s, stages, genome_len, out_path, &none, f));      // (the same refusals, the same route)
    f.gfa = GfaWant{nullptr, out_path, out, true};
    return KATOME_OK;
}
int katome_gfa_strands_packed(const katome_settings* s, const uint8_t* packed, uint64_t n_reads, uint32_t read_len, const uint8_t* skip, const char* stages,
                              uint64_t original_genome_length, const char* out_path, katome_gfa_strands** out) {
    Finish f{nullptr, nullptr};
    KCHECK(gfa_strands_finish(s, stages, original_genome_length, out_path, out, f));
    return build_packed_impl(s, packed, n_reads, read_len, skip, f);
}
int katome_gfa_packed(const katome_settings* s, const uint8_t* packed, uint64_t n_reads, uint32_t read_len, const uint8_t* skip, const char* stages,
                      uint64_t original_genome_length, const char* out_path, katome_gfa** out) {
    Finish f{nullptr, nullptr};
    KCHECK(gfa_finish(s, stages, original_genome_length, out_path, out, f));
    return build_packed_impl(s, packed, n_reads, read_len, skip, f);
}
int katome_shrink_packed(const katome_settings* s, const uint8_t* packed, uint64_t n_reads, uint32_t read_len,
                         const uint8_t* skip, katome_contigs** out) {
    if (!out) { set_error("null argument"); return KATOME_E_ARG; }
    *out = nullptr;
    return build_packed_impl(s, packed, n_reads, read_len, skip, Finish{nullptr, out});
}

int katome_ingest_files(const katome_settings* s, const char* const* paths, size_t n_paths, katome_reads** out) {
    if (!s || !out || (!paths && n_paths)) { set_error("null argument"); return KATOME_E_ARG; }
    *out = nullptr;
    HostReads* hr = new (std::nothrow) HostReads();
    if (!hr) { set_error("out of host memory"); return KATOME_E_OOM; }
    int rc = ingest_files(s, paths, n_paths, *hr);
    if (rc) { delete hr; return rc; }
    struct Owner { katome_reads r; HostReads* hr; };
    Owner* o = new (std::nothrow) Owner();
    if (!o) { delete hr; set_error("out of host memory"); return KATOME_E_OOM; }
    o->hr = hr;
    o->r.n_records = hr->n_records; o->r.n_reads = hr->n_reads; o->r.read_bytes = hr->read_bytes;
    o->r.packed_bytes = hr->packed_bytes; o->r.total_windows = hr->total_windows; o->r.fixed_len = hr->fixed_len; o->r._pad = 0;
    o->r.packed = hr->packed; o->r.byte_off = hr->byte_off; o->r.len = hr->len;
    *out = &o->r;
    return KATOME_OK;
}
void katome_reads_free(katome_reads* r) {
    if (!r) return;
    struct Owner { katome_reads r; HostReads* hr; };
    Owner* o = reinterpret_cast<Owner*>(r);
    delete o->hr;
    delete o;
}

}  // extern "C"

// BFCounter (create_bfc, builder.rs:79-115; add_read_bfc, pt_graph.rs:317-330): every kept line is a k-mer with a weight -> one
// edge per line and strand, exactly as add_single_edge_bfc (pt_graph.rs:201-213) adds them: lines naming the same k-mer, and a
// k-mer that is its own reverse complement, stay parallel edges.
static int build_bfc(const katome_settings* s, const HostReads& hr, const Finish& finish) {
    katome_builder* b = nullptr;
    KCHECK(katome_builder_create(s, &b));
    int rc = KATOME_OK;
    do {
        if (hr.n_reads) {
            DevBuf d_packed, d_w, d_rec;
            if ((rc = d_packed.alloc(hr.packed_bytes + 32)) || (rc = d_w.alloc(hr.n_reads * 4)) || (rc = d_rec.alloc(hr.n_reads * 8 * b->nw + 16))) break;
            if (hipMemcpy(d_packed.p, hr.packed, hr.packed_bytes, hipMemcpyHostToDevice) != hipSuccess ||
                hipMemcpy(d_w.p, hr.weight, hr.n_reads * 4, hipMemcpyHostToDevice) != hipSuccess) { set_error("H2D copy failed"); rc = KATOME_E_DEVICE; break; }
            // the lines' k-mers as they are written (no canonical form: both strands become edges of their own)
            if ((rc = launch_extract_fixed(s->k, false, d_packed.as<uint8_t>(), hr.n_reads, s->k, nullptr, d_rec.as<u64>(), nullptr))) break;
            if ((rc = bfc_set_edges(b, d_rec.as<u64>(), d_w.as<u32>(), hr.n_reads, nullptr))) break;
            if (hipStreamSynchronize(nullptr) != hipSuccess) { set_error("device failure during build"); rc = KATOME_E_DEVICE; break; }
        }
        rc = finish(b, hr.read_bytes);
    } while (0);
    katome_builder_destroy(b);
    return rc;
}

static int build_files_impl(const katome_settings* s, const char* const* paths, size_t n_paths, const Finish& finish) {
    if (!s || (!paths && n_paths)) { set_error("null argument"); return KATOME_E_ARG; }
    HostReads hr;
    build_lap("", true);
    KCHECK(ingest_files(s, paths, n_paths, hr));           // path / parse / short-read errors surface before any GPU work
    build_lap("ingest (host)");
    if (s->file_type == 2) return build_bfc(s, hr, finish);
    if (hr.fixed_len) return build_packed_impl(s, hr.packed, hr.n_reads, hr.fixed_len, nullptr, finish, &hr.read_bytes);
    // reads of unequal length over several GPUs (or, KATOME_FORCE_SHARDED=1, one GPU as a world of one rank): the sharded route
    if (hr.n_reads && (s->n_devices > 1 || (s->n_devices == 1 && getenv("KATOME_FORCE_SHARDED")))) {
        KCHECK(check_k(s->k));
        return build_var_multi(s, hr, finish);
    }
    katome_builder* b = nullptr;
    KCHECK(katome_builder_create(s, &b));
    int rc = KATOME_OK;
    do {
        if (hr.n_reads == 0) { rc = finish(b, hr.read_bytes); break; }
        DevBuf d_packed, d_off, d_len, d_pref, d_rec;
        if ((rc = d_packed.alloc(hr.packed_bytes + 32)) || (rc = d_off.alloc((hr.n_reads + 1) * 8)) || (rc = d_len.alloc(hr.n_reads * 4))) break;
        if (hipMemcpy(d_packed.p, hr.packed, hr.packed_bytes, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(d_off.p, hr.byte_off, (hr.n_reads + 1) * 8, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(d_len.p, hr.len, hr.n_reads * 4, hipMemcpyHostToDevice) != hipSuccess) { set_error("H2D copy failed"); rc = KATOME_E_DEVICE; break; }
        uint64_t cap = batch_records(b->nw);
        if (const char* e = getenv("KATOME_VAR_BATCH_RECORDS")) cap = std::max<uint64_t>(1, strtoull(e, nullptr, 10));   // tests: many small batches
        // one span for the whole input (tiles from the front of every read + the windows left over, as for fixed-length reads)
        const uint32_t span = tile_span_for_lengths(s->k, hr.len, hr.n_reads, hr.total_windows);
        DevBuf d_tpref, d_rpref;
        std::vector<uint64_t> pref, tpref, rpref;
        for (uint64_t r0 = 0; r0 < hr.n_reads && !rc;) {
            pref.assign(1, 0); tpref.assign(1, 0); rpref.assign(1, 0);
            uint64_t r1 = r0;
            while (r1 < hr.n_reads && (r1 == r0 || pref.back() + (hr.len[r1] - s->k + 1) <= cap)) {
                const uint64_t W = hr.len[r1] - s->k + 1;
                pref.push_back(pref.back() + W);
                tpref.push_back(tpref.back() + W / span);
                rpref.push_back(rpref.back() + W % span);
                ++r1;
            }
            const uint64_t windows = pref.back(), tiles = tpref.back(), rest = rpref.back(), nr = r1 - r0;
            if ((rc = d_pref.alloc(pref.size() * 8)) || (rc = d_rec.alloc(windows * 8 * b->nw + 16))) break;
            if (hipMemcpy(d_pref.p, pref.data(), pref.size() * 8, hipMemcpyHostToDevice) != hipSuccess) { set_error("H2D copy failed"); rc = KATOME_E_DEVICE; break; }
            if (span > 1) {
                if ((rc = d_tpref.alloc(tpref.size() * 8)) || (rc = d_rpref.alloc(rpref.size() * 8))) break;
                if (hipMemcpy(d_tpref.p, tpref.data(), tpref.size() * 8, hipMemcpyHostToDevice) != hipSuccess ||
                    hipMemcpy(d_rpref.p, rpref.data(), rpref.size() * 8, hipMemcpyHostToDevice) != hipSuccess) { set_error("H2D copy failed"); rc = KATOME_E_DEVICE; break; }
                if (tiles) {
                    rc = katome_dev_extract_var_tiles(b, d_packed.as<uint8_t>(), hr.packed_bytes, d_off.as<u64>() + r0, d_len.as<u32>() + r0,
                                                      d_tpref.as<u64>(), d_pref.as<u64>(), nr, tiles, windows, span, d_rec.as<u64>(), nullptr);
                    if (!rc) rc = katome_dev_insert_tiles(b, d_rec.as<u64>(), tiles, span, nullptr);
                }
                if (!rc) rc = katome_dev_extract_var_remainder(b, d_packed.as<uint8_t>(), hr.packed_bytes, d_off.as<u64>() + r0, d_len.as<u32>() + r0,
                                                               d_rpref.as<u64>(), d_pref.as<u64>(), nr, rest, windows, span, d_rec.as<u64>(), nullptr);
                if (!rc) rc = katome_dev_insert(b, d_rec.as<u64>(), rest, nullptr);       // (also closes the batch when nothing is left over)
            } else {
                rc = katome_dev_extract_var(b, d_packed.as<uint8_t>(), hr.packed_bytes, d_off.as<u64>() + r0, d_len.as<u32>() + r0,
                                            d_pref.as<u64>(), nr, windows, d_rec.as<u64>(), nullptr);
                if (!rc) rc = katome_dev_insert(b, d_rec.as<u64>(), windows, nullptr);
            }
            if (!rc && hipStreamSynchronize(nullptr) != hipSuccess) { set_error("device failure during build"); rc = KATOME_E_DEVICE; }
            r0 = r1;
        }
        if (rc) break;
        d_rec.release(); d_packed.release(); d_off.release(); d_len.release(); d_pref.release();
        rc = finish(b, hr.read_bytes);
    } while (0);
    katome_builder_destroy(b);
    return rc;
}

extern "C" {

int katome_build_files(const katome_settings* s, const char* const* paths, size_t n_paths, katome_graph** out) {
    if (!out) { set_error("null argument"); return KATOME_E_ARG; }
    *out = nullptr;
    return build_files_impl(s, paths, n_paths, Finish{out, nullptr});
}
int katome_build_files_staged(const katome_settings* s, const char* const* paths, size_t n_paths, const char* stages,
                              uint64_t original_genome_length, katome_graph** out) {
    if (!out) { set_error("null argument"); return KATOME_E_ARG; }
    *out = nullptr;
    Finish f{out, nullptr};
    f.stages = stages; f.genome_len = original_genome_length;
    return build_files_impl(s, paths, n_paths, f);
}
int katome_build_files_staged_stats(const katome_settings* s, const char* const* paths, size_t n_paths, const char* stages,
                                    uint64_t original_genome_length, katome_stats* stage_stats, katome_graph** out) {
    if (!out || !stage_stats) { set_error("null argument"); return KATOME_E_ARG; }
    *out = nullptr;
    Finish f{out, nullptr};
    f.stages = stages; f.genome_len = original_genome_length; f.stage_stats = stage_stats;
    return build_files_impl(s, paths, n_paths, f);
}
int katome_assemble_files(const katome_settings* s, const char* const* paths, size_t n_paths, uint64_t original_genome_length, const char* out_path,
                          katome_assembly** out) {
    if (!out && !out_path) { set_error("null argument"); return KATOME_E_ARG; }
    if (out) *out = nullptr;
    Finish f{nullptr, nullptr};
    f.assemble = AssembleWant{out, out_path}; f.assembling = true; f.genome_len = original_genome_length;
    return build_files_impl(s, paths, n_paths, f);
}
int katome_assemble_gfa_files(const katome_settings* s, const char* const* paths, size_t n_paths, uint64_t original_genome_length, const char* fasta_path,
                              const char* gfa_path, katome_assembly** asm_out, katome_gfa_paths** gfa_out) {
    Finish f{nullptr, nullptr};
    KCHECK(assemble_gfa_finish(original_genome_length, fasta_path, gfa_path, asm_out, gfa_out, f));
    return build_files_impl(s, paths, n_paths, f);
}
int katome_assemble_gfa_strands_files(const katome_settings* s, const char* const* paths, size_t n_paths, uint64_t original_genome_length,
                                      const char* fasta_path, const char* gfa_path, katome_assembly** asm_out, katome_gfa_strand_paths** gfa_out) {
    Finish f{nullptr, nullptr};
    KCHECK(assemble_gfa_strands_finish(original_genome_length, fasta_path, gfa_path, asm_out, gfa_out, f));
    return build_files_impl(s, paths, n_paths, f);
}
int katome_assemble_unique_files(const katome_settings* s, const char* const* paths, size_t n_paths, uint64_t original_genome_length,
                                 const char* fasta_path, const char* unique_path, katome_assembly** asm_out, katome_unique_assembly** unique_out) {
    Finish f{nullptr, nullptr};
    KCHECK(assemble_unique_finish(original_genome_length, fasta_path, unique_path, asm_out, unique_out, f));
    return build_files_impl(s, paths, n_paths, f);
}
int katome_unitigs_files(const katome_settings* s, const char* const* paths, size_t n_paths, const char* stages, uint64_t original_genome_length,
                         const char* out_path, katome_unitigs* out) {
    Finish f{nullptr, nullptr};
    KCHECK(unitigs_finish(s, stages, original_genome_length, out_path, out, f));
    return build_files_impl(s, paths, n_paths, f);
}
int katome_unitigs_gfa_files(const katome_settings* s, const char* const* paths, size_t n_paths, const char* stages, uint64_t original_genome_length,
                             const char* out_path, katome_unitigs_gfa* out) {
    Finish f{nullptr, nullptr};
    KCHECK(unitigs_gfa_finish(s, stages, original_genome_length, out_path, out, f));
    return build_files_impl(s, paths, n_paths, f);
}
int katome_gfa_strands_files(const katome_settings* s, const char* const* paths, size_t n_paths, const char* stages, uint64_t original_genome_length,
                             const char* out_path, katome_gfa_strands** out) {
    Finish f{nullptr, nullptr};
    KCHECK(gfa_strands_finish(s, stages, original_genome_length, out_path, out, f));
    return build_files_impl(s, paths, n_paths, f);
}
int katome_gfa_files(const katome_settings* s, const char* const* paths, size_t n_paths, const char* stages, uint64_t original_genome_length,
                     const char* out_path, katome_gfa** out) {
    Finish f{nullptr, nullptr};
    KCHECK(gfa_finish(s, stages, original_genome_length, out_path, out, f));
    return build_files_impl(s, paths, n_paths, f);
}
int katome_shrink_files(const katome_settings* s, const char* const* paths, size_t n_paths, katome_contigs** out) {
    if (!out) { set_error("null argument"); return KATOME_E_ARG; }
    *out = nullptr;
    return build_files_impl(s, paths, n_paths, Finish{nullptr, out});
}

// Stats<CollectionStats> for PtGraph (stats/collections.rs:137-168), from the host arrays
int katome_graph_stats(const katome_graph* g, katome_stats* st) {
    if (!g || !st) { set_error("null argument"); return KATOME_E_ARG; }
    memset(st, 0, sizeof *st);
    st->node_count = g->n_nodes; st->edge_count = g->n_edges;
    std::vector<uint32_t> outd(g->n_nodes, 0), ind(g->n_nodes, 0);
    uint64_t sum_w = 0;
    for (uint64_t e = 0; e < g->n_edges; ++e) {
        st->max_edge_weight = std::max(st->max_edge_weight, g->edge_weight[e]);
        sum_w += g->edge_weight[e];
        ++outd[g->edge_src[e]]; ++ind[g->edge_dst[e]];
    }
    st->avg_edge_weight = (double)sum_w / (double)g->n_edges;
    uint64_t sum_out = 0;
    for (uint64_t n = 0; n < g->n_nodes; ++n) {
        st->max_out_degree = std::max<uint64_t>(st->max_out_degree, outd[n]);
        st->max_in_degree = std::max<uint64_t>(st->max_in_degree, ind[n]);
        sum_out += outd[n];
        if (ind[n] == 0) ++st->incoming_vert_count;      // externals(Incoming)
        if (outd[n] == 0) ++st->outgoing_vert_count;     // externals(Outgoing)
    }
    st->avg_out_degree = (double)sum_out / (double)g->n_nodes;
    return KATOME_OK;
}

}  // extern "C"
