// host_build.cpp -- the host-memory half of the C ABI of include/katome_gpu.h: katome_build_packed*, katome_build_files*,
// katome_shrink_*, katome_assemble_*, katome_unitigs_*, katome_gfa_*, the host results and the driver of a build over several GPUs.
// No kernel is defined or launched here: everything on the device goes through the device ABI (api.hip) and the sharded builder
// (dist*.hip).  In the order of the file: the host results (one owner type, one copier), the endings (what a build hands back:
// `Finish`), the build over several GPUs, the two read sources (packed reads, files) and the entries, each ending written once.
#include <stddef.h>
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
#include <type_traits>
#include <vector>

#include <sys/mman.h>

#include <errno.h>

#include "builder.h"
#include "comm.h"
#include "contig_stats.h"
#include "multi_route.h"

// ---- host results ------------------------------------------------------------------------------------------------------------
// A result as the caller sees it, followed by what it owns: the arrays its pointers name, each released with free().  The
// public struct comes first, so that the pointer the caller holds is also the pointer to the whole.
template <class T> struct Owned { T v; std::vector<void*> mem; };
template <class T> static Owned<T>* owner_of(T* v) {
    static_assert(std::is_standard_layout<Owned<T>>::value && offsetof(Owned<T>, v) == 0, "a result's public struct is the first thing in its owner");
    return reinterpret_cast<Owned<T>*>(v);
}
template <class T> static void free_result(T* v) {
    if (!v) return;
    Owned<T>* o = owner_of(v);
    for (void* p : o->mem) free(p);
    delete o;
}
// a result under construction: freed with everything it has taken so far unless it is release()d to the caller
template <class T> struct ResultFree { void operator()(T* v) const { free_result(v); } };
template <class T> using Result = std::unique_ptr<T, ResultFree<T>>;
// a zeroed T that owns nothing yet (nullptr and the error set: out of host memory)
template <class T> static Result<T> make_result() {
    Owned<T>* o = new (std::nothrow) Owned<T>();
    if (!o) { set_error("out of host memory"); return nullptr; }
    memset(&o->v, 0, sizeof o->v);
    return Result<T>(&o->v);
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

// room for an array of `bytes` bytes of the result `v`, recorded in its owner, which will free it (nullptr and *oom set: out of
// host memory)
template <class T> static void* take(T* v, size_t bytes, bool* oom, bool touch = true) {
    void* p = touch ? host_result_alloc(bytes) : host_result_reserve(bytes);
    if (p) owner_of(v)->mem.push_back(p); else *oom = true;
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

// `count` elements from the device into an array of the result `v`; a count of 0 still gets room for one element
template <class E, class T> static int d2h(T* v, const E** dst, const void* d_src, size_t count) {
    bool oom = false;
    E* h = (E*)take(v, std::max<size_t>(count, 1) * sizeof(E), &oom);
    if (oom) { set_error("out of host memory"); return KATOME_E_OOM; }
    if (count) KCHECK_HIP(hipMemcpy(h, d_src, count * sizeof(E), hipMemcpyDeviceToHost));
    *dst = h;
    return KATOME_OK;
}

// The arrays of one result, copied down one after the other: the first failure is kept in `rc` and everything after it skipped.
template <class T> struct Copier {
    T* v; int rc = KATOME_OK;
    template <class E> void operator()(const E** dst, const void* d_src, size_t count) { if (!rc) rc = d2h(v, dst, d_src, count); }
    // two texts back to back in one array, `first` then `second` (a GFA's lines and its P lines: together they are the file)
    void back_to_back(const uint8_t** dst, const void* d_first, uint64_t first, const void* d_second, uint64_t second) {
        if (rc) return;
        bool oom = false;
        uint8_t* text = (uint8_t*)take(v, std::max<uint64_t>(first + second, 1), &oom);
        if (oom) { set_error("out of host memory"); rc = KATOME_E_OOM; return; }
        if ((first && hipMemcpy(text, d_first, first, hipMemcpyDeviceToHost) != hipSuccess) ||
            (second && hipMemcpy(text + first, d_second, second, hipMemcpyDeviceToHost) != hipSuccess)) {
            set_error("device -> host copy failed: %s", hipGetErrorString(hipGetLastError()));
            rc = KATOME_E_DEVICE;
        }
        *dst = text;
    }
};

extern "C" {      // (every katome_*_free of the header is the one free_result)
void katome_graph_free(katome_graph* g) { free_result(g); }
void katome_contigs_free(katome_contigs* c) { free_result(c); }
void katome_assembly_free(katome_assembly* a) { free_result(a); }
void katome_unique_assembly_free(katome_unique_assembly* u) { free_result(u); }
void katome_gfa_free(katome_gfa* g) { free_result(g); }
void katome_gfa_strands_free(katome_gfa_strands* g) { free_result(g); }
void katome_gfa_paths_free(katome_gfa_paths* g) { free_result(g); }
void katome_gfa_strand_paths_free(katome_gfa_strand_paths* g) { free_result(g); }
void katome_depth_free(katome_depth* d) { free_result(d); }
}  // extern "C"

#ifndef KATOME_HOST_RESULTS_ONLY      // (tests/hostshim/host_results_selftest.cpp builds the part above for the host alone)

// One result of a build and its file: the result is handed out before the file is tried, so that a path that cannot be created
// leaves the caller with the result all the same; a caller who did not ask for the result does not get one to free.
template <class T> static int hand_out(Result<T> r, T** out, const char* path, int (*save)(const T*, const char*)) {
    if (out) *out = r.get();
    const int rc = path ? save(r.get(), path) : KATOME_OK;
    if (out) (void)r.release();
    return rc;
}
// Two results of one build and their two files, the assembly's FASTA first: both results are handed out before any file is
// tried, both files are tried, and the first failure is the one reported.
template <class T> static int hand_out_both(Result<katome_assembly> a, katome_assembly** a_out, const char* a_path, Result<T> r, T** out,
                                            const char* path, int (*save)(const T*, const char*)) {
    if (a_out) *a_out = a.get();
    if (out) *out = r.get();
    int rc = a_path ? katome_assembly_save(a.get(), a_path) : KATOME_OK;
    const std::string first_err = rc ? get_error() : "";
    const int rc_second = path ? save(r.get(), path) : KATOME_OK;
    if (rc) set_error("%s", first_err.c_str()); else rc = rc_second;
    if (a_out) (void)a.release();
    if (out) (void)r.release();
    return rc;
}

// these host bytes as a file, with File::create's statuses and message (asm/mod.rs:62); what a failed write leaves stays
static int save_host_text(const uint8_t* text, uint64_t bytes, const char* path) {
    FILE* f = fopen(path, "wb");
    if (!f) {
        set_error("couldn't create %s: %s", path, CREATE_ERROR_KINDS[create_error_kind(errno)]);
        return KATOME_E_OPEN;
    }
    const size_t n = bytes ? fwrite(text, 1, bytes, f) : 0;
    if (fclose(f) != 0 || n != bytes) { set_error("couldn't write %s", path); return KATOME_E_OPEN; }
    return KATOME_OK;
}
// katome_*_save: the result's text is the file (the two parts of a GFA with paths are contiguous on the host)
template <class T> static uint64_t file_bytes(const T& v) { return v.text_bytes; }
static uint64_t file_bytes(const katome_gfa_paths& g) { return g.text_bytes + g.path_bytes; }
static uint64_t file_bytes(const katome_gfa_strand_paths& g) { return g.text_bytes + g.path_bytes; }
template <class T> static int save_result(const T* v, const char* path) {
    if (!v || !path) { set_error("null argument"); return KATOME_E_ARG; }
    return save_host_text(v->text, file_bytes(*v), path);
}
extern "C" {
// Contigs::save_to_file (asm/mod.rs:57-72): the text in FASTA layout is the file
int katome_assembly_save(const katome_assembly* a, const char* path) {
    if (a && path && a->layout != KATOME_TEXT_FASTA) { set_error("assembly_save: the text is not in FASTA layout"); return KATOME_E_ARG; }
    return save_result(a, path);
}
int katome_unique_assembly_save(const katome_unique_assembly* u, const char* path) { return save_result(u, path); }
int katome_gfa_save(const katome_gfa* g, const char* path) { return save_result(g, path); }
int katome_gfa_strands_save(const katome_gfa_strands* g, const char* path) { return save_result(g, path); }
int katome_gfa_paths_save(const katome_gfa_paths* g, const char* path) { return save_result(g, path); }
int katome_gfa_strand_paths_save(const katome_gfa_strand_paths* g, const char* path) { return save_result(g, path); }

int katome_contig_stats_of(const uint64_t* lengths, uint64_t n, uint64_t original_genome_length, katome_contig_stats* out) {
    if (!out || (n && !lengths)) { set_error("null argument"); return KATOME_E_ARG; }
    ContigStats st;
    const int which = contig_stats(lengths, n, original_genome_length, &st);
    out->n50 = st.n50; out->l50 = st.l50; out->n90 = st.n90; out->ng50 = st.ng50;
    return contig_stats_status(which);
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
                          uint64_t read_bytes, Result<katome_graph>& out, std::vector<HostCopy>& arrays) {
    Result<katome_graph> g = make_result<katome_graph>();
    if (!g) return KATOME_E_OOM;
    g->n_nodes = n_nodes; g->n_edges = n_edges; g->read_bytes = read_bytes;
    g->k = k; g->key_words = key_words; g->label_stride = label_stride;
    bool oom = false;
    auto room = [&](size_t bytes) { arrays.push_back({take(g.get(), bytes, &oom, false), bytes, nullptr}); return arrays.back().h; };
    g->edge_src = (uint64_t*)room(n_edges * 8); g->edge_dst = (uint64_t*)room(n_edges * 8);
    g->edge_weight = (uint32_t*)room(n_edges * 4); g->edge_label = (uint8_t*)room(n_edges * (size_t)label_stride);
    g->edge_key = (uint64_t*)room(n_edges * 8 * (size_t)key_words); g->node_key = (uint64_t*)room(n_nodes * 8 * (size_t)key_words);
    if (ages) g->edge_age = (uint32_t*)room(n_edges * 4);
    if (oom) { set_error("out of host memory"); return KATOME_E_OOM; }
    out = std::move(g);
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

// ---- the endings on one GPU ----------------------------------------------------------------------------------------------------
// What every ending starts with: finalize, the pruning the flag asks for, the stage letters
template <class Hook = NoStageHook> static int prepare(katome_builder* b, const char* stages, uint64_t genome_len, const Hook& at_stage = Hook()) {
    katome_dev_graph dg;
    build_lap("counting (H2D, kernels)");
    KCHECK(katome_dev_finalize(b, &dg, nullptr));
    build_lap("finalize");
    if (b->s.flags & KATOME_FLAG_REMOVE_DEAD_PATHS) KCHECK(katome_dev_remove_dead_paths(b, &dg, nullptr, nullptr));
    KCHECK(run_stages(stages, BuilderStages{b, genome_len}, at_stage));
    build_lap("stages after the build");
    return KATOME_OK;
}
// (the stages work on the links of a first-seen build)
static int stages_need_order(bool first_seen, const char* stages) {
    if (first_seen || !stages || !*stages) return KATOME_OK;
    set_error("stages after the build need KATOME_FLAG_FIRST_SEEN_ORDER");
    return KATOME_E_ARG;
}

// (stage_stats: the caller's strlen(stages) + 1 entries, filled on the device as the stages go by)
static int graph_to_host(katome_builder* b, uint64_t read_bytes, katome_graph** out, const char* stages, uint64_t genome_len, katome_stats* stage_stats) {
    KCHECK(stages_need_order(b->first_seen, stages));
    KCHECK(prepare(b, stages, genome_len, [&](size_t i) { return stage_stats ? katome_dev_graph_stats(b, &stage_stats[i], nullptr) : KATOME_OK; }));
    katome_dev_graph dg;
    KCHECK(katome_dev_current_graph(b, &dg));
    Result<katome_graph> g;
    std::vector<HostCopy> jobs;
    KCHECK(new_host_graph(dg.n_nodes, dg.n_edges, b->s.k, dg.key_words, dg.label_stride, dg.d_edge_age != nullptr, read_bytes, g, jobs));
    const void* from[] = {dg.d_edge_src, dg.d_edge_dst, dg.d_edge_weight, dg.d_edge_label, dg.d_edge_key, dg.d_node_key, dg.d_edge_age};
    for (size_t i = 0; i < jobs.size(); ++i) jobs[i].src = from[i];
    KCHECK(d2h_all(jobs));
    build_lap("graph to host arrays");
    *out = g.release();
    return KATOME_OK;
}

// finalize (+ the pruning the flags ask for) + shrink, copied to host arrays
static int contigs_to_host(katome_builder* b, uint64_t read_bytes, katome_contigs** out, uint32_t shrink_mode) {
    KCHECK(prepare(b, nullptr, 0));
    katome_dev_contigs dc;
    KCHECK(katome_dev_shrink_mode(b, shrink_mode, &dc, nullptr, nullptr));
    Result<katome_contigs> c = make_result<katome_contigs>();
    if (!c) return KATOME_E_OOM;
    c->n_nodes = dc.n_nodes; c->n_edges = dc.n_edges; c->label_bytes = dc.label_bytes; c->read_bytes = read_bytes;
    c->k = b->s.k; c->key_words = dc.key_words;
    Copier<katome_contigs> down{c.get()};
    down(&c->edge_src, dc.d_edge_src, dc.n_edges);
    down(&c->edge_dst, dc.d_edge_dst, dc.n_edges);
    down(&c->edge_weight, dc.d_edge_weight, dc.n_edges);
    down(&c->edge_kmers, dc.d_edge_kmers, dc.n_edges);
    down(&c->edge_label_off, dc.d_edge_label_off, dc.n_edges ? dc.n_edges + 1 : 0);
    down(&c->edge_label, dc.d_edge_label, dc.label_bytes);
    down(&c->node_key, dc.d_node_key, dc.n_nodes * dc.key_words);
    KCHECK(down.rc);
    if (dc.n_edges == 0) const_cast<uint64_t*>(c->edge_label_off)[0] = 0;       // (d2h hands out room for one entry even when asked for none)
    *out = c.release();
    return KATOME_OK;
}

// The GFA family.  A host struct katome_gfa* and the device struct katome_dev_gfa* it is copied from name their fields alike, and
// the four forms are made of three blocks: the segments (all four), the merged strands, the paths.
template <class H, class D> static void segments_block(Copier<H>& down, const D& d, uint32_t k, uint64_t read_bytes) {
    H* g = down.v;
    g->n_segments = d.n_segments; g->n_links = d.n_links; g->text_bytes = d.text_bytes; g->read_bytes = read_bytes; g->k = k;
    down(&g->segment_off, d.d_segment_off, d.n_segments);
    down(&g->link_first, d.d_link_first, d.n_segments + 1);
}
// (n_edges: the merged edges the twins were sought among)
template <class H, class D> static void strands_block(Copier<H>& down, const D& d, uint64_t n_edges) {
    H* g = down.v;
    g->n_edges = n_edges; g->n_unpaired = d.n_unpaired; g->n_self_twins = d.n_self_twins;
    down(&g->segment_name, d.d_segment_name, d.n_segments);
    down(&g->edge_twin, d.d_edge_twin, n_edges);
}
// (the text: the H, S and L lines and, straight after them, the P lines)
template <class H, class D> static void paths_block(Copier<H>& down, const D& d) {
    H* g = down.v;
    g->n_paths = d.n_paths; g->n_jumps = d.n_jumps; g->path_bytes = d.path_bytes;
    down.back_to_back(&g->text, d.d_text, d.text_bytes, d.d_path_text, d.path_bytes);
    down(&g->path_line_off, d.d_path_line_off, d.n_paths + 1);
    down(&g->path_contig, d.d_path_contig, d.n_paths);
    down(&g->path_first_piece, d.d_path_first_piece, d.n_paths + 1);
}

// katome_dev_contigs_gfa of a shrunk graph in host arrays
static int gfa_to_host(katome_builder* b, const katome_dev_contigs& dc, uint64_t read_bytes, Result<katome_gfa>& out) {
    katome_dev_gfa d;
    KCHECK(katome_dev_contigs_gfa(b, &dc, &d, nullptr));
    if (!(out = make_result<katome_gfa>())) return KATOME_E_OOM;
    Copier<katome_gfa> down{out.get()};
    down(&out->text, d.d_text, d.text_bytes);
    segments_block(down, d, b->s.k, read_bytes);
    return down.rc;
}
// katome_dev_contigs_gfa_strands of a shrunk graph in host arrays
static int gfa_strands_to_host(katome_builder* b, const katome_dev_contigs& dc, uint64_t read_bytes, Result<katome_gfa_strands>& out) {
    katome_dev_gfa_strands d;
    KCHECK(katome_dev_contigs_gfa_strands(b, &dc, &d, nullptr));
    if (!(out = make_result<katome_gfa_strands>())) return KATOME_E_OOM;
    Copier<katome_gfa_strands> down{out.get()};
    down(&out->text, d.d_text, d.text_bytes);
    segments_block(down, d, b->s.k, read_bytes);
    strands_block(down, d, dc.n_edges);
    return down.rc;
}
// katome_dev_collapse_gfa of the builder's last collapse in host arrays
static int gfa_paths_to_host(katome_builder* b, uint64_t read_bytes, Result<katome_gfa_paths>& out) {
    katome_dev_gfa_paths d;
    KCHECK(katome_dev_collapse_gfa(b, &d, nullptr));
    if (!(out = make_result<katome_gfa_paths>())) return KATOME_E_OOM;
    Copier<katome_gfa_paths> down{out.get()};
    paths_block(down, d);
    segments_block(down, d, b->s.k, read_bytes);
    return down.rc;
}
// katome_dev_collapse_gfa_strands of the builder's last collapse in host arrays
static int gfa_strand_paths_to_host(katome_builder* b, uint64_t read_bytes, Result<katome_gfa_strand_paths>& out) {
    katome_dev_gfa_strand_paths d;
    KCHECK(katome_dev_collapse_gfa_strands(b, &d, nullptr));
    if (!(out = make_result<katome_gfa_strand_paths>())) return KATOME_E_OOM;
    Copier<katome_gfa_strand_paths> down{out.get()};
    paths_block(down, d);
    segments_block(down, d, b->s.k, read_bytes);
    strands_block(down, d, d.n_edges);
    out->n_mirrored = d.n_mirrored; out->n_self_mirror = d.n_self_mirror;
    down(&out->path_mirror, d.d_path_mirror, d.n_paths);
    return down.rc;
}

// katome_dev_collapse_unique(FASTA) of the builder's last collapse in host arrays; lengths: every contig's bases, as the walk knows them
static int unique_to_host(katome_builder* b, uint64_t read_bytes, const std::vector<uint64_t>& lengths, uint64_t genome_len,
                          Result<katome_unique_assembly>& out) {
    katome_dev_unique_assembly d;
    KCHECK(katome_dev_collapse_unique(b, KATOME_TEXT_FASTA, &d, nullptr));
    if (!(out = make_result<katome_unique_assembly>())) return KATOME_E_OOM;
    katome_unique_assembly* u = out.get();
    u->n_contigs = d.n_contigs; u->n_kept = d.n_kept; u->text_bytes = d.text_bytes; u->read_bytes = read_bytes; u->k = b->s.k;
    u->n_mirrored = d.n_mirrored; u->n_self_mirror = d.n_self_mirror;
    Copier<katome_unique_assembly> down{u};
    down(&u->contig_mirror, d.d_contig_mirror, d.n_contigs);
    down(&u->kept_name, d.d_kept_name, d.n_kept);
    down(&u->kept_off, d.d_kept_off, d.n_kept);
    down(&u->kept_len, d.d_kept_len, d.n_kept);
    down(&u->text, d.d_text, d.text_bytes);
    KCHECK(down.rc);
    std::vector<uint64_t> kept;
    try { kept.reserve(d.n_kept); }
    catch (const std::bad_alloc&) { set_error("out of host memory"); return KATOME_E_OOM; }
    for (uint64_t i = 0; i < d.n_kept; ++i) {
        const uint64_t c = u->kept_name[i];
        if (c >= lengths.size() || lengths[c] != u->kept_len[i]) {
            set_error("collapse_unique: kept contig %llu does not have the walk's length", (unsigned long long)c);
            return KATOME_E_DEVICE;
        }
        kept.push_back(lengths[c]);
    }
    return katome_contig_stats_of(kept.data(), kept.size(), genome_len, &u->stats);
}

// the stages "dcwced" (asm/basic_assembler.rs:58-75), collapse, Contigs::stats and, with a path, save_to_file: host arrays.
// `with`: what else the same collapse hands back, with a file of its own (`with_path`) -- katome_assemble_gfa_*: the GFA of the
// collapse's shrunk graph with the contigs as P lines; katome_assemble_gfa_strands_*: that GFA with strand twins merged;
// katome_assemble_unique_*: the strand-unique form of the contigs
struct AssembleWant {
    katome_assembly** out; const char* path;
    enum With { Alone, GfaPaths, GfaStrandPaths, Unique } with = Alone;
    const char* with_path = nullptr;
    katome_gfa_paths** gfa_out = nullptr; katome_gfa_strand_paths** strands_out = nullptr; katome_unique_assembly** unique_out = nullptr;
};
static int assembly_to_host(katome_builder* b, uint64_t read_bytes, const AssembleWant& want, uint64_t genome_len) {
    if (!b->first_seen) { set_error("assemble needs KATOME_FLAG_FIRST_SEEN_ORDER"); return KATOME_E_ARG; }
    KCHECK(prepare(b, "dcwced", genome_len));
    Result<katome_assembly> a = make_result<katome_assembly>();
    if (!a) return KATOME_E_OOM;
    katome_dev_assembly da;
    memset(&da, 0, sizeof da);
    std::vector<uint64_t> lengths;
    const int collapse_rc = builder_collapse(b, KATOME_TEXT_FASTA, &da, &a->collapse, &lengths, nullptr);
    build_lap("collapse");
    KCHECK(collapse_rc);
    a->n_contigs = da.n_contigs; a->text_bytes = da.text_bytes; a->read_bytes = read_bytes; a->k = b->s.k; a->layout = KATOME_TEXT_FASTA;
    Copier<katome_assembly> down{a.get()};
    down(&a->contig_off, da.d_contig_off, da.n_contigs);
    down(&a->contig_len, da.d_contig_len, da.n_contigs);
    down(&a->text, da.d_text, da.text_bytes);
    KCHECK(down.rc);
    KCHECK(katome_contig_stats_of(lengths.data(), lengths.size(), genome_len, &a->stats));      // contigs.log_stats()
    switch (want.with) {
        case AssembleWant::GfaPaths: {
            Result<katome_gfa_paths> g;
            const int rc = gfa_paths_to_host(b, read_bytes, g);
            build_lap("collapse_gfa");
            KCHECK(rc);
            return hand_out_both(std::move(a), want.out, want.path, std::move(g), want.gfa_out, want.with_path, katome_gfa_paths_save);
        }
        case AssembleWant::GfaStrandPaths: {
            Result<katome_gfa_strand_paths> g;
            const int rc = gfa_strand_paths_to_host(b, read_bytes, g);
            build_lap("collapse_gfa_strands");
            KCHECK(rc);
            return hand_out_both(std::move(a), want.out, want.path, std::move(g), want.strands_out, want.with_path, katome_gfa_strand_paths_save);
        }
        case AssembleWant::Unique: {
            Result<katome_unique_assembly> u;
            const int rc = unique_to_host(b, read_bytes, lengths, genome_len, u);
            build_lap("collapse_unique");
            KCHECK(rc);
            return hand_out_both(std::move(a), want.out, want.path, std::move(u), want.unique_out, want.with_path, katome_unique_assembly_save);
        }
        case AssembleWant::Alone: break;
    }
    return hand_out(std::move(a), want.out, want.path, katome_assembly_save);
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
// every merged edge's bases (its k-mers and k - 1 more): their total, the longest and, where asked for, each of them
static int unitig_bases(const katome_builder* b, const katome_dev_contigs& dc, uint64_t* total, uint64_t* longest, std::vector<uint64_t>* lengths) {
    std::vector<uint32_t> kmers;
    try { kmers.resize(dc.n_edges); if (lengths) lengths->resize(dc.n_edges); }
    catch (const std::bad_alloc&) { set_error("out of host memory"); return KATOME_E_OOM; }
    if (dc.n_edges) KCHECK_HIP(hipMemcpy(kmers.data(), dc.d_edge_kmers, dc.n_edges * 4, hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < dc.n_edges; ++i) {
        const uint64_t len = (uint64_t)kmers[i] + b->s.k - 1;
        if (lengths) (*lengths)[i] = len;
        *total += len; *longest = std::max(*longest, len);
    }
    return KATOME_OK;
}
static int unitigs_to_host(katome_builder* b, uint64_t read_bytes, const UnitigsWant& want, const char* stages, uint64_t genome_len) {
    KCHECK(prepare(b, stages, genome_len));
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
        KCHECK(unitig_bases(b, dc, &u->total_bases, &u->longest, nullptr));
        return want.path ? save_device_bytes(dgfa.d_text, dgfa.text_bytes, want.path) : KATOME_OK;
    }
    katome_dev_assembly da;
    KCHECK(katome_dev_contigs_text(b, &dc, KATOME_TEXT_FASTA, &da, nullptr));
    katome_unitigs* u = want.out;
    u->n_contigs = da.n_contigs; u->text_bytes = da.text_bytes; u->read_bytes = read_bytes; u->k = b->s.k; u->n_devices = 1;
    std::vector<uint64_t> lengths;
    KCHECK(unitig_bases(b, dc, &u->total_bases, &u->longest, &lengths));
    const int stats_rc = katome_contig_stats_of(lengths.data(), lengths.size(), genome_len, &u->stats);      // (a tipping point of 0: the file is written all the same)
    const std::string stats_err = stats_rc ? get_error() : "";
    if (want.path) KCHECK(save_device_bytes(da.d_text, da.text_bytes, want.path));
    if (stats_rc) set_error("%s", stats_err.c_str());
    return stats_rc;
}

// katome_gfa_*: the flag's remove_dead_paths, the stage letters, shrink (AUTO: exact on a first-seen build, fast otherwise), the GFA of
// the result copied to host arrays and, with a path, the file
// (merge: the merged form, katome_gfa_strands_*, handed back through `strands` -- the same pipeline up to the shrink)
struct GfaWant { katome_gfa** out; const char* path; katome_gfa_strands** strands = nullptr; bool merge = false; };
static int gfa_ending(katome_builder* b, uint64_t read_bytes, const GfaWant& want, const char* stages, uint64_t genome_len) {
    KCHECK(stages_need_order(b->first_seen, stages));
    KCHECK(prepare(b, stages, genome_len));
    katome_dev_contigs dc;
    KCHECK(katome_dev_shrink(b, &dc, nullptr));
    if (want.merge) {
        Result<katome_gfa_strands> g;
        KCHECK(gfa_strands_to_host(b, dc, read_bytes, g));
        return hand_out(std::move(g), want.strands, want.path, katome_gfa_strands_save);
    }
    Result<katome_gfa> g;
    KCHECK(gfa_to_host(b, dc, read_bytes, g));
    return hand_out(std::move(g), want.out, want.path, katome_gfa_save);
}

// katome_depth_paths: the flag's remove_dead_paths, the stage letters, then every record of the query files, in file order and in ASCII,
// through katome_dev_depth in batches under its window limit (KATOME_DEPTH_BATCH_WINDOWS: a smaller one, for tests); the per-record
// arrays land in the result batch by batch, the hits of the batches are added up on the host
struct DepthWant { katome_depth** out; const char* const* paths; size_t n_paths; uint32_t file_type, flags; };
static uint64_t depth_batch_windows() {
    if (const char* e = getenv("KATOME_DEPTH_BATCH_WINDOWS")) { const long long v = atoll(e); if (v > 0) return std::min<uint64_t>((uint64_t)v, 0xFFFFFFFFull); }
    return 1ull << 31;
}
static int depth_ending(katome_builder* b, uint64_t read_bytes, const DepthWant& want, const char* stages, uint64_t genome_len) {
    KCHECK(stages_need_order(b->first_seen, stages));
    HostQuery q;
    KCHECK(ingest_query_files(want.file_type, want.paths, want.n_paths, q));
    KCHECK(prepare(b, stages, genome_len));
    const uint32_t k = b->s.k;
    const uint64_t n = q.len.size(), E = b->n_edges;
    Result<katome_depth> r = make_result<katome_depth>();
    if (!r) return KATOME_E_OOM;
    bool oom = false;
    uint64_t* present = (uint64_t*)take(r.get(), std::max<uint64_t>(n, 1) * 8, &oom);
    uint64_t* invalid = (uint64_t*)take(r.get(), std::max<uint64_t>(n, 1) * 8, &oom);
    uint64_t* sum = (uint64_t*)take(r.get(), std::max<uint64_t>(n, 1) * 8, &oom);
    uint32_t* mn = (uint32_t*)take(r.get(), std::max<uint64_t>(n, 1) * 4, &oom);
    uint32_t* mx = (uint32_t*)take(r.get(), std::max<uint64_t>(n, 1) * 4, &oom);
    const bool want_hits = (want.flags & KATOME_DEPTH_EDGE_HITS) != 0;
    uint32_t* hits = want_hits ? (uint32_t*)take(r.get(), std::max<uint64_t>(E, 1) * 4, &oom) : nullptr;
    if (oom) { set_error("out of host memory"); return KATOME_E_OOM; }
    if (hits) memset(hits, 0, std::max<uint64_t>(E, 1) * 4);
    r->read_bytes = read_bytes; r->n_records = n; r->n_edges = E;
    r->seq_present = present; r->seq_invalid = invalid; r->seq_sum = sum; r->seq_min = mn; r->seq_max = mx; r->edge_hits = hits;
    std::vector<uint64_t> off;
    std::vector<uint32_t> batch_hits;
    DevBuf d_text, d_off, d_len;
    const uint64_t limit = depth_batch_windows();
    for (uint64_t r0 = 0; r0 < n;) {
        uint64_t r1 = r0, w = 0;
        while (r1 < n) {      // (one record has fewer than 2^32 windows: a batch always takes one at least)
            const uint64_t wn = q.len[r1] >= k ? (uint64_t)q.len[r1] - k + 1 : 0;
            if (r1 > r0 && w + wn >= limit) break;
            w += wn; ++r1;
        }
        const uint64_t m = r1 - r0, t0 = q.off[r0], t1 = r1 < n ? q.off[r1] : q.text.size();
        off.resize(m);
        for (uint64_t i = 0; i < m; ++i) off[i] = q.off[r0 + i] - t0;
        KCHECK(d_text.alloc(t1 - t0)); KCHECK(d_off.alloc(m * 8)); KCHECK(d_len.alloc(m * 4));
        if (t1 > t0) KCHECK_HIP(hipMemcpy(d_text.p, q.text.data() + t0, t1 - t0, hipMemcpyHostToDevice));
        KCHECK_HIP(hipMemcpy(d_off.p, off.data(), m * 8, hipMemcpyHostToDevice));
        KCHECK_HIP(hipMemcpy(d_len.p, q.len.data() + r0, m * 4, hipMemcpyHostToDevice));
        katome_dev_depth_result d;
        KCHECK(katome_dev_depth(b, KATOME_DEPTH_ASCII, want.flags, d_text.as<uint8_t>(), t1 - t0, d_off.as<uint64_t>(), d_len.as<uint32_t>(), m, &d, nullptr));
        KCHECK_HIP(hipMemcpy(present + r0, d.d_seq_present, m * 8, hipMemcpyDeviceToHost));
        KCHECK_HIP(hipMemcpy(invalid + r0, d.d_seq_invalid, m * 8, hipMemcpyDeviceToHost));
        KCHECK_HIP(hipMemcpy(sum + r0, d.d_seq_sum, m * 8, hipMemcpyDeviceToHost));
        KCHECK_HIP(hipMemcpy(mn + r0, d.d_seq_min, m * 4, hipMemcpyDeviceToHost));
        KCHECK_HIP(hipMemcpy(mx + r0, d.d_seq_max, m * 4, hipMemcpyDeviceToHost));
        r->n_windows += d.n_windows; r->n_present += d.n_present; r->n_invalid += d.n_invalid; r->weight_sum += d.weight_sum;
        if (hits && E) {
            batch_hits.resize(E);
            KCHECK_HIP(hipMemcpy(batch_hits.data(), d.d_edge_hits, E * 4, hipMemcpyDeviceToHost));
            for (uint64_t e = 0; e < E; ++e) hits[e] += batch_hits[e];
        }
        r0 = r1;
    }
    if (hits) for (uint64_t e = 0; e < E; ++e) r->n_edges_hit += hits[e] != 0;
    build_lap("depth of the query files");
    *want.out = r.release();
    return KATOME_OK;
}

// What a host entry hands back: the graph, the graph after shrink, the assembly, the unitigs' numbers (and their file), or the
// GFA -- and what that ending needs.  The ending runs on the builder of a one-GPU build or of a graph gathered to one GPU.
enum class Ending { Graph, Contigs, Assembly, Unitigs, Gfa, Depth };
struct Finish {
    Ending ending;
    const char* stages = nullptr; uint64_t genome_len = 0;      // (Contigs takes no stages; Assembly runs its own)
    katome_graph** graph = nullptr;                               // Graph
    katome_stats* stage_stats = nullptr;                          // katome_build_*_staged_stats: the graph described before the first stage and after each
    katome_contigs** contigs = nullptr;                           // Contigs
    uint32_t shrink_mode = KATOME_SHRINK_AUTO;
    AssembleWant assemble{nullptr, nullptr};                      // Assembly
    UnitigsWant unitigs{nullptr, nullptr};                        // Unitigs
    GfaWant gfa{nullptr, nullptr};                                // Gfa
    DepthWant depth{nullptr, nullptr, 0, 0, 0};                   // Depth
    int operator()(katome_builder* b, uint64_t read_bytes) const {
        switch (ending) {
            case Ending::Graph: return graph_to_host(b, read_bytes, graph, stages, genome_len, stage_stats);
            case Ending::Contigs: return contigs_to_host(b, read_bytes, contigs, shrink_mode);
            case Ending::Assembly: return assembly_to_host(b, read_bytes, assemble, genome_len);
            case Ending::Unitigs: return unitigs_to_host(b, read_bytes, unitigs, stages, genome_len);
            case Ending::Gfa: return gfa_ending(b, read_bytes, gfa, stages, genome_len);
            case Ending::Depth: return depth_ending(b, read_bytes, depth, stages, genome_len);
        }
        set_error("unknown ending");
        return KATOME_E_ARG;
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
    Result<katome_contigs> owned = make_result<katome_contigs>();
    if (!owned) return KATOME_E_OOM;
    katome_contigs* c = owned.get();
    bool oom = false;
    uint64_t* src = (uint64_t*)take(c, TE * 8, &oom); uint64_t* dst = (uint64_t*)take(c, TE * 8, &oom); uint32_t* w = (uint32_t*)take(c, TE * 4, &oom);
    uint32_t* km = (uint32_t*)take(c, TE * 4, &oom); uint64_t* off = (uint64_t*)take(c, (TE + 1) * 8, &oom); uint8_t* lab = (uint8_t*)take(c, lb, &oom);
    uint64_t* nkey = (uint64_t*)take(c, TN * 8 * nw, &oom); uint8_t* seen = (uint8_t*)take(c, TN, &oom);
    if (oom) { set_error("out of host memory"); return KATOME_E_OOM; }
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
    if (bad || placed != TN) { set_error("sharded shrink: the ranks' merged edges or nodes do not fit together"); return KATOME_E_DEVICE; }
    c->n_nodes = TN; c->n_edges = TE; c->label_bytes = lb; c->read_bytes = read_bytes; c->k = k; c->key_words = nw;
    c->edge_src = src; c->edge_dst = dst; c->edge_weight = w; c->edge_kmers = km; c->edge_label_off = off; c->edge_label = lab; c->node_key = nkey;
    *out = owned.release();
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
    Result<katome_graph> graph; int alloc_rc = KATOME_OK;       // the host graph every rank copies its share into (rank 0 makes it)
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

// rank 0, between the two meetings: the host graph of the whole result (mb.graph; nullptr and mb.alloc_rc: no memory for it)
static void alloc_shared_graph(MultiBuild& mb, const katome_dist_graph& g) {
    std::vector<HostCopy> arrays;
    mb.alloc_rc = new_host_graph(g.total_nodes, g.total_edges, mb.s->k, g.key_words, g.label_stride, g.d_edge_age != nullptr, mb.read_bytes,
                                 mb.graph, arrays);
    if (mb.alloc_rc == KATOME_OK) for (const HostCopy& a : arrays) host_result_touch(a.h, a.bytes);
}

// by packed key the host arrays are the ranks' shares one after the other: rank r's edges start where those of the ranks
// before it end, its nodes at node_base
static int copy_out_by_key(MultiBuild& mb, int r, const katome_dist_graph& g, hipStream_t stream) {
    const katome_graph* hg = mb.graph.get();
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
    const katome_graph* hg = mb.graph.get();
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
    if (!mb.graph) return mb.alloc_rc ? mb.alloc_rc : KATOME_E_OOM;
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
    // (a GFA takes the assembly's route: gathered to the first GPU, where the stages, the shrink and the text run -- links cross ranks;
    // so does a depth query: the lookup needs all the edges in one index)
    const MultiRoute route = plan_multi_route(s->flags, finish.ending == Ending::Contigs, finish.stages,
                                               finish.ending == Ending::Assembly || finish.ending == Ending::Gfa || finish.ending == Ending::Depth,
                                               finish.ending == Ending::Unitigs);
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
    // (mb.graph: the ranks' shares were copied out, no gathered route ran; a failed build frees it)
    if (mb.graph && rc == KATOME_OK && finish.graph) *finish.graph = mb.graph.release();
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

// ---- the entries ---------------------------------------------------------------------------------------------------------------
// Where the reads come from: 2-bit packed reads of one length in the caller's memory, or files.  Each builds with any ending.
struct PackedReads {
    const uint8_t* packed; uint64_t n_reads; uint32_t read_len; const uint8_t* skip;
    int build(const katome_settings* s, const Finish& finish) const { return build_packed_impl(s, packed, n_reads, read_len, skip, finish); }
};
struct FileReads {
    const char* const* paths; size_t n_paths;
    int build(const katome_settings* s, const Finish& finish) const { return build_files_impl(s, paths, n_paths, finish); }
};

// Every ending's entry, once for both sources.  The order decides which error a caller sees: the caller's output pointers, then
// the outputs cleared, then the ending's own refusals -- before any GPU work, the same on every route -- and only then the
// source's checks (settings, reads or paths, k), the ingest and the device.
static int null_argument() { set_error("null argument"); return KATOME_E_ARG; }

// katome_build_*, katome_build_*_staged, katome_build_*_staged_stats (with_stats: the caller must bring stage_stats)
template <class Reads> static int graph_entry(const Reads& reads, const katome_settings* s, const char* stages, uint64_t genome_len, bool with_stats,
                                              katome_stats* stage_stats, katome_graph** out) {
    if (!out || (with_stats && !stage_stats)) return null_argument();
    *out = nullptr;
    Finish f{Ending::Graph};
    f.graph = out; f.stages = stages; f.genome_len = genome_len; f.stage_stats = stage_stats;
    return reads.build(s, f);
}
// katome_shrink_*
template <class Reads> static int contigs_entry(const Reads& reads, const katome_settings* s, katome_contigs** out) {
    if (!out) return null_argument();
    *out = nullptr;
    Finish f{Ending::Contigs};
    f.contigs = out;
    return reads.build(s, f);
}
// katome_assemble_*, katome_assemble_gfa_*, katome_assemble_gfa_strands_*, katome_assemble_unique_*: a result or a file must be asked for
template <class Reads> static int assemble_entry(const Reads& reads, const katome_settings* s, uint64_t genome_len, const AssembleWant& want) {
    if (!want.out && !want.path && !want.with_path && !want.gfa_out && !want.strands_out && !want.unique_out) return null_argument();
    if (want.out) *want.out = nullptr;
    if (want.gfa_out) *want.gfa_out = nullptr;
    if (want.strands_out) *want.strands_out = nullptr;
    if (want.unique_out) *want.unique_out = nullptr;
    Finish f{Ending::Assembly};
    f.assemble = want; f.genome_len = genome_len;
    return reads.build(s, f);
}
// katome_unitigs_* (out) and katome_unitigs_gfa_* (gfa): the caller's plain struct
template <class Reads> static int unitigs_entry(const Reads& reads, const katome_settings* s, const char* stages, uint64_t genome_len, const char* out_path,
                                                katome_unitigs* out, katome_unitigs_gfa* gfa) {
    if (!out && !gfa) return null_argument();
    if (out) memset(out, 0, sizeof *out);
    if (gfa) memset(gfa, 0, sizeof *gfa);
    // (the stages work on the links of a first-seen build, on every route)
    if (s && !(s->flags & KATOME_FLAG_FIRST_SEEN_ORDER) && ((stages && *stages) || (s->flags & KATOME_FLAG_REMOVE_DEAD_PATHS))) {
        set_error("unitigs: stage letters and KATOME_FLAG_REMOVE_DEAD_PATHS need KATOME_FLAG_FIRST_SEEN_ORDER");
        return KATOME_E_ARG;
    }
    Finish f{Ending::Unitigs};
    f.unitigs = UnitigsWant{out, out_path, gfa}; f.stages = stages; f.genome_len = genome_len;
    return reads.build(s, f);
}
// katome_gfa_* (out) and katome_gfa_strands_* (strands): the result or the file must be asked for
template <class Reads> static int gfa_entry(const Reads& reads, const katome_settings* s, const char* stages, uint64_t genome_len, const char* out_path,
                                            katome_gfa** out, katome_gfa_strands** strands, bool merge) {
    if (!out && !strands && !out_path) return null_argument();
    if (out) *out = nullptr;
    if (strands) *strands = nullptr;
    if (s) KCHECK(stages_need_order((s->flags & KATOME_FLAG_FIRST_SEEN_ORDER) != 0, stages));
    Finish f{Ending::Gfa};
    f.gfa = GfaWant{out, out_path, strands, merge}; f.stages = stages; f.genome_len = genome_len;
    return reads.build(s, f);
}

// katome_depth_paths
template <class Reads> static int depth_entry(const Reads& reads, const katome_settings* s, const char* stages, uint64_t genome_len, const DepthWant& want) {
    if (!want.out) return null_argument();
    *want.out = nullptr;
    if (want.file_type > 1) { set_error("depth: query files are FASTA (0) or FASTQ (1), not file type %u", want.file_type); return KATOME_E_ARG; }
    if (want.flags & ~(uint32_t)(KATOME_DEPTH_EITHER_STRAND | KATOME_DEPTH_EDGE_HITS)) {
        set_error("depth: flag bits 0x%x (the host result takes KATOME_DEPTH_EITHER_STRAND and KATOME_DEPTH_EDGE_HITS; it has no per-window array)", want.flags);
        return KATOME_E_ARG;
    }
    if (want.n_paths && !want.paths) return null_argument();
    if (s) KCHECK(stages_need_order((s->flags & KATOME_FLAG_FIRST_SEEN_ORDER) != 0, stages));
    Finish f{Ending::Depth};
    f.depth = want; f.stages = stages; f.genome_len = genome_len;
    return reads.build(s, f);
}

extern "C" {

int katome_depth_paths(const katome_settings* s, const char* const* read_paths, size_t n_read_paths, const char* stages, uint64_t original_genome_length,
                       const char* const* query_paths, size_t n_query_paths, uint32_t query_file_type, uint32_t flags, katome_depth** out) {
    return depth_entry(FileReads{read_paths, n_read_paths}, s, stages, original_genome_length, DepthWant{out, query_paths, n_query_paths, query_file_type, flags});
}

int katome_build_packed(const katome_settings* s, const uint8_t* packed, uint64_t n_reads, uint32_t read_len, const uint8_t* skip, katome_graph** out) {
    return graph_entry(PackedReads{packed, n_reads, read_len, skip}, s, nullptr, 0, false, nullptr, out);
}
int katome_build_files(const katome_settings* s, const char* const* paths, size_t n_paths, katome_graph** out) {
    return graph_entry(FileReads{paths, n_paths}, s, nullptr, 0, false, nullptr, out);
}
int katome_build_packed_staged(const katome_settings* s, const uint8_t* packed, uint64_t n_reads, uint32_t read_len, const uint8_t* skip,
                               const char* stages, uint64_t original_genome_length, katome_graph** out) {
    return graph_entry(PackedReads{packed, n_reads, read_len, skip}, s, stages, original_genome_length, false, nullptr, out);
}
int katome_build_files_staged(const katome_settings* s, const char* const* paths, size_t n_paths, const char* stages,
                              uint64_t original_genome_length, katome_graph** out) {
    return graph_entry(FileReads{paths, n_paths}, s, stages, original_genome_length, false, nullptr, out);
}
int katome_build_packed_staged_stats(const katome_settings* s, const uint8_t* packed, uint64_t n_reads, uint32_t read_len, const uint8_t* skip,
                                     const char* stages, uint64_t original_genome_length, katome_stats* stage_stats, katome_graph** out) {
    return graph_entry(PackedReads{packed, n_reads, read_len, skip}, s, stages, original_genome_length, true, stage_stats, out);
}
int katome_build_files_staged_stats(const katome_settings* s, const char* const* paths, size_t n_paths, const char* stages,
                                    uint64_t original_genome_length, katome_stats* stage_stats, katome_graph** out) {
    return graph_entry(FileReads{paths, n_paths}, s, stages, original_genome_length, true, stage_stats, out);
}

int katome_shrink_packed(const katome_settings* s, const uint8_t* packed, uint64_t n_reads, uint32_t read_len, const uint8_t* skip, katome_contigs** out) {
    return contigs_entry(PackedReads{packed, n_reads, read_len, skip}, s, out);
}
int katome_shrink_files(const katome_settings* s, const char* const* paths, size_t n_paths, katome_contigs** out) {
    return contigs_entry(FileReads{paths, n_paths}, s, out);
}

int katome_assemble_packed(const katome_settings* s, const uint8_t* packed, uint64_t n_reads, uint32_t read_len, const uint8_t* skip,
                           uint64_t original_genome_length, const char* out_path, katome_assembly** out) {
    return assemble_entry(PackedReads{packed, n_reads, read_len, skip}, s, original_genome_length, AssembleWant{out, out_path});
}
int katome_assemble_files(const katome_settings* s, const char* const* paths, size_t n_paths, uint64_t original_genome_length, const char* out_path,
                          katome_assembly** out) {
    return assemble_entry(FileReads{paths, n_paths}, s, original_genome_length, AssembleWant{out, out_path});
}
int katome_assemble_gfa_packed(const katome_settings* s, const uint8_t* packed, uint64_t n_reads, uint32_t read_len, const uint8_t* skip,
                               uint64_t original_genome_length, const char* fasta_path, const char* gfa_path, katome_assembly** asm_out,
                               katome_gfa_paths** gfa_out) {
    return assemble_entry(PackedReads{packed, n_reads, read_len, skip}, s, original_genome_length,
                          AssembleWant{asm_out, fasta_path, AssembleWant::GfaPaths, gfa_path, gfa_out});
}
int katome_assemble_gfa_files(const katome_settings* s, const char* const* paths, size_t n_paths, uint64_t original_genome_length, const char* fasta_path,
                              const char* gfa_path, katome_assembly** asm_out, katome_gfa_paths** gfa_out) {
    return assemble_entry(FileReads{paths, n_paths}, s, original_genome_length, AssembleWant{asm_out, fasta_path, AssembleWant::GfaPaths, gfa_path, gfa_out});
}
int katome_assemble_gfa_strands_packed(const katome_settings* s, const uint8_t* packed, uint64_t n_reads, uint32_t read_len, const uint8_t* skip,
                                       uint64_t original_genome_length, const char* fasta_path, const char* gfa_path, katome_assembly** asm_out,
                                       katome_gfa_strand_paths** gfa_out) {
    return assemble_entry(PackedReads{packed, n_reads, read_len, skip}, s, original_genome_length,
                          AssembleWant{asm_out, fasta_path, AssembleWant::GfaStrandPaths, gfa_path, nullptr, gfa_out});
}
int katome_assemble_gfa_strands_files(const katome_settings* s, const char* const* paths, size_t n_paths, uint64_t original_genome_length,
                                      const char* fasta_path, const char* gfa_path, katome_assembly** asm_out, katome_gfa_strand_paths** gfa_out) {
    return assemble_entry(FileReads{paths, n_paths}, s, original_genome_length,
                          AssembleWant{asm_out, fasta_path, AssembleWant::GfaStrandPaths, gfa_path, nullptr, gfa_out});
}
int katome_assemble_unique_packed(const katome_settings* s, const uint8_t* packed, uint64_t n_reads, uint32_t read_len, const uint8_t* skip,
                                  uint64_t original_genome_length, const char* fasta_path, const char* unique_path, katome_assembly** asm_out,
                                  katome_unique_assembly** unique_out) {
    return assemble_entry(PackedReads{packed, n_reads, read_len, skip}, s, original_genome_length,
                          AssembleWant{asm_out, fasta_path, AssembleWant::Unique, unique_path, nullptr, nullptr, unique_out});
}
int katome_assemble_unique_files(const katome_settings* s, const char* const* paths, size_t n_paths, uint64_t original_genome_length,
                                 const char* fasta_path, const char* unique_path, katome_assembly** asm_out, katome_unique_assembly** unique_out) {
    return assemble_entry(FileReads{paths, n_paths}, s, original_genome_length,
                          AssembleWant{asm_out, fasta_path, AssembleWant::Unique, unique_path, nullptr, nullptr, unique_out});
}

int katome_unitigs_packed(const katome_settings* s, const uint8_t* packed, uint64_t n_reads, uint32_t read_len, const uint8_t* skip,
                          const char* stages, uint64_t original_genome_length, const char* out_path, katome_unitigs* out) {
    return unitigs_entry(PackedReads{packed, n_reads, read_len, skip}, s, stages, original_genome_length, out_path, out, nullptr);
}
int katome_unitigs_files(const katome_settings* s, const char* const* paths, size_t n_paths, const char* stages, uint64_t original_genome_length,
                         const char* out_path, katome_unitigs* out) {
    return unitigs_entry(FileReads{paths, n_paths}, s, stages, original_genome_length, out_path, out, nullptr);
}
int katome_unitigs_gfa_packed(const katome_settings* s, const uint8_t* packed, uint64_t n_reads, uint32_t read_len, const uint8_t* skip,
                              const char* stages, uint64_t original_genome_length, const char* out_path, katome_unitigs_gfa* out) {
    return unitigs_entry(PackedReads{packed, n_reads, read_len, skip}, s, stages, original_genome_length, out_path, nullptr, out);
}
int katome_unitigs_gfa_files(const katome_settings* s, const char* const* paths, size_t n_paths, const char* stages, uint64_t original_genome_length,
                             const char* out_path, katome_unitigs_gfa* out) {
    return unitigs_entry(FileReads{paths, n_paths}, s, stages, original_genome_length, out_path, nullptr, out);
}

int katome_gfa_packed(const katome_settings* s, const uint8_t* packed, uint64_t n_reads, uint32_t read_len, const uint8_t* skip, const char* stages,
                      uint64_t original_genome_length, const char* out_path, katome_gfa** out) {
    return gfa_entry(PackedReads{packed, n_reads, read_len, skip}, s, stages, original_genome_length, out_path, out, nullptr, false);
}
int katome_gfa_files(const katome_settings* s, const char* const* paths, size_t n_paths, const char* stages, uint64_t original_genome_length,
                     const char* out_path, katome_gfa** out) {
    return gfa_entry(FileReads{paths, n_paths}, s, stages, original_genome_length, out_path, out, nullptr, false);
}
int katome_gfa_strands_packed(const katome_settings* s, const uint8_t* packed, uint64_t n_reads, uint32_t read_len, const uint8_t* skip, const char* stages,
                              uint64_t original_genome_length, const char* out_path, katome_gfa_strands** out) {
    return gfa_entry(PackedReads{packed, n_reads, read_len, skip}, s, stages, original_genome_length, out_path, nullptr, out, true);
}
int katome_gfa_strands_files(const katome_settings* s, const char* const* paths, size_t n_paths, const char* stages, uint64_t original_genome_length,
                             const char* out_path, katome_gfa_strands** out) {
    return gfa_entry(FileReads{paths, n_paths}, s, stages, original_genome_length, out_path, nullptr, out, true);
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

#endif  // KATOME_HOST_RESULTS_ONLY
