// dist_gfa.hip -- the unitig graph of the sharded shrink as GFA 1, no gather: the join of links across ranks, the numbered text of
// this rank's two parts (gfa.hip's kernel in its numbered form) and the file written by all ranks (dist_save.h).  The format, the
// rank-major numbering and the layout of the whole text are fixed in include/katome_gpu.h (katome_dist_gfa).
//
// The join works on the shrink result the builder holds: sh_src / sh_dst are NEW global node ids over [0, sh_total_nodes), and
// vertex v lives in the directory of rank v / ceil(total_nodes / world) (dist_gfa_dir.h, dist_shrink.hip's scheme).
//   1. Every merged edge b registers (address of src[b], its global number first + b) with that directory, through the Router.
//      The directory keeps a count and four slots per vertex of its range: a vertex of a shrunk de Bruijn graph has at most four
//      out-segments (each starts with a distinct out-edge; a cycle's head is an inner vertex).  A fifth registration, or an address
//      outside the range, is a broken invariant: KATOME_E_DEVICE on every rank.  Each vertex's slots are then sorted in registers.
//   2. Every merged edge a asks the directory of dst[a] and gets FOUR words back in one reply (Router::reply with a width): the
//      out-segments in ascending order, NONE64 behind the last.  The one-word form (first number, count) would need all
//      out-segments of a vertex on one rank at adjacent numbers.  That holds by packed key, where a node's out-edges are adjacent
//      on its owner and every head survives in order, but NOT in first-seen order, where a rank's edges are in the order they were
//      first seen and the out-edges of one vertex lie anywhere in it.  The four-word answer is right in both numberings and needs no
//      condition to be verified; it costs 32 B instead of 8 B per question on the way back.
//   3. The answers' counts are scanned into link_first, the numbers compacted into link_b; the four-word answers go.
// Questions and registrations travel in chunks of KATOME_DIST_GFA_CHUNK records per rank and exchange (default 2^24; the chunk
// count is agreed, so the Router's buffers stay bounded).  Memory per rank: directory 4 + 32 B per vertex of its range; 32 B per
// segment while the answers wait, then 8 B per segment (link_first) + 8 B per link (link_b) + 4 B per link (its local a); the
// writer's line offsets (8 B per line) and the text itself, once.  Never another rank's text.
//
// Between collectives every rank's own status is agreed (dist_agree.h), as in dist_text.hip.  KATOME_DIST_GFA_FAIL=<rank> (tests):
// that rank fails after the sizes are known.  KATOME_DIST_GFA_TRACE=1: every rank's wall time per call on stderr, with the join's
// time and the bytes it sent (tools/bench_dist_gfa.py).
#include "dist_agree.h"
#include "dist_gfa_dir.h"
#include "dist_route.h"
#include "dist_save.h"

namespace {

constexpr uint64_t DEFAULT_GFA_CHUNK = 1ull << 24;
constexpr u32 MAX_OUT = 4;

// KATOME_DIST_GFA_TRACE: "[<call>] rank r/n: <ms> ms, <bytes> bytes" when the call returns; katome_dist_contigs_gfa adds the join's
// wall time and the bytes it sent, and the writer kernels' own time (HIP events around the two launches) over this rank's bytes
struct GfaTrace {
    const char* name; katome_comm* comm; const uint64_t* bytes; double join_ms = -1; uint64_t join_bytes = 0; float write_ms = 0; uint64_t write_bytes = 0;
    double t0 = now_ms();
    static bool on() { static const bool v = getenv("KATOME_DIST_GFA_TRACE") != nullptr; return v; }
    ~GfaTrace() {
        if (!on()) return;
        if (join_ms < 0) fprintf(stderr, "[%s] rank %d/%d: %.3f ms, %llu bytes\n", name, comm->rank(), comm->world(), now_ms() - t0, (unsigned long long)(bytes ? *bytes : 0));
        else fprintf(stderr, "[%s] rank %d/%d: %.3f ms, %llu bytes, join %.3f ms, %llu bytes sent, write %.4f ms, %llu bytes\n", name, comm->rank(), comm->world(),
                     now_ms() - t0, (unsigned long long)(bytes ? *bytes : 0), join_ms, (unsigned long long)join_bytes, write_ms, (unsigned long long)write_bytes);
    }
};

// a chunk of this rank's merged edges [at, at + n): the directory address of one end [and the segment's global number]
__global__ __launch_bounds__(BLOCK) void dg_address_kernel(const u64* __restrict__ node, u64 at, u64 n, u64 per, u64 first, u64* __restrict__ A, u64* __restrict__ B) {
    WLOOP(i, n) if (i < n) {
        const u64 v = node[at + i];
        A[i] = ((v / per) << 56) | v;
        if (B) B[i] = first + at + i;
    }
}
// the directory takes a registration: bad[0] counts addresses outside its range, bad[1] fifth out-segments
__global__ __launch_bounds__(BLOCK) void dg_register_kernel(const u64* __restrict__ A, const u64* __restrict__ B, u64 n, u64 dbase, u64 range, u32* __restrict__ cnt,
                                                            u64* __restrict__ slots, unsigned long long* __restrict__ bad) {
    WLOOP(i, n) if (i < n) {
        const u64 v = A[i] & LOW56;
        if (v < dbase || v - dbase >= range) { atomicAdd(&bad[0], 1ull); continue; }
        const u32 s = atomicAdd(&cnt[v - dbase], 1u);
        if (s < MAX_OUT) slots[(v - dbase) * MAX_OUT + s] = B[i];
        else atomicAdd(&bad[1], 1ull);
    }
}
// a vertex's out-segments in ascending order, NONE64 behind them (the slots were filled with NONE64 before)
__global__ __launch_bounds__(BLOCK) void dg_sort_kernel(u64* __restrict__ slots, u64 range) {
    WLOOP(j, range) if (j < range) {
        u64 a = slots[j * 4], b = slots[j * 4 + 1], c = slots[j * 4 + 2], e = slots[j * 4 + 3], t;
#define DG_CSWAP(x, y) if (x > y) { t = x; x = y; y = t; }
        DG_CSWAP(a, b) DG_CSWAP(c, e) DG_CSWAP(a, c) DG_CSWAP(b, e) DG_CSWAP(b, c)
#undef DG_CSWAP
        slots[j * 4] = a; slots[j * 4 + 1] = b; slots[j * 4 + 2] = c; slots[j * 4 + 3] = e;
    }
}
// ... and answers a question with the vertex's four words
__global__ __launch_bounds__(BLOCK) void dg_answer_kernel(const u64* __restrict__ A, u64 n, u64 dbase, u64 range, const u64* __restrict__ slots, u64* __restrict__ ans,
                                                          unsigned long long* __restrict__ bad) {
    WLOOP(i, n) if (i < n) {
        const u64 v = A[i] & LOW56;
        const bool ok = v >= dbase && v - dbase < range;
        if (!ok) atomicAdd(&bad[0], 1ull);
#pragma unroll
        for (u32 q = 0; q < MAX_OUT; ++q) ans[i * MAX_OUT + q] = ok ? slots[(v - dbase) * MAX_OUT + q] : NONE64;
    }
}
__global__ __launch_bounds__(BLOCK) void dg_count_kernel(const u64* __restrict__ ans, u64 H, u32* __restrict__ count) {
    WLOOP(a, H) if (a < H) {
        u32 c = 0;
#pragma unroll
        for (u32 q = 0; q < MAX_OUT; ++q) c += ans[a * MAX_OUT + q] != NONE64;
        count[a] = c;
    }
}
__global__ __launch_bounds__(BLOCK) void dg_links_kernel(const u64* __restrict__ ans, const u64* __restrict__ link_first, u64 H, u64* __restrict__ link_b) {
    WLOOP(a, H) if (a < H) {
        u64 at = link_first[a];
#pragma unroll
        for (u32 q = 0; q < MAX_OUT; ++q) { const u64 b = ans[a * MAX_OUT + q]; if (b != NONE64) link_b[at++] = b; }
    }
}

int check_gfa_builder(katome_dist_builder* d, const char* name) {
    if (!d) { set_error("null argument"); return KATOME_E_ARG; }
    if (d->gathered) { set_error("%s: the ranks' shares were gathered (katome_dist_gather)", name); return KATOME_E_ARG; }
    if (!d->sh_valid) { set_error("%s: call katome_dist_shrink first (the builder holds no result of it)", name); return KATOME_E_ARG; }
    return KATOME_OK;
}

// link_first / link_b of this rank's merged edges, through the directory; *L = this rank's links
int dist_gfa_join(katome_dist_builder* d, Collective& C, uint64_t first, DevBuf& link_first, DevBuf& link_b, uint64_t* L, hipStream_t stream) {
    const char* name = C.name;
    const uint64_t H = d->sh_edges;
    const GfaDirectory dir(d->sh_total_nodes, (uint32_t)C.world);
    const uint64_t dbase = dir.base((uint32_t)C.rank), range = dir.range((uint32_t)C.rank);
    uint64_t chunk = DEFAULT_GFA_CHUNK;
    if (const char* e = getenv("KATOME_DIST_GFA_CHUNK")) chunk = std::max<long long>(1, atoll(e));
    KCHECK(d->comm->allreduce(&chunk, 1, OP_MIN));          // (process ranks may see different environments: the smallest holds)
    uint64_t n_chunks = (H + chunk - 1) / chunk;
    auto sizes = [&]() -> int {
        if (H >= 0xFFFFFFFEull) { set_error("%s: %llu segments on one rank, fewer than 2^32 - 2 lines", name, (unsigned long long)H); return KATOME_E_UNSUPPORTED; }
        return KATOME_OK;
    };
    KCHECK(C.agree(sizes(), &n_chunks));
    Router router(d, stream);
    DevBuf cnt(stream), slots(stream), A(stream), B(stream), bad(stream), ans(stream), count(stream);
    const uint64_t room = std::min(H, chunk) + 1;
    const u64 *src = d->sh_src.as<u64>(), *dst = d->sh_dst.as<u64>();
    auto local = [&]() -> int {
        KCHECK(cnt.alloc((range + 1) * 4)); KCHECK(slots.alloc((range + 1) * 8 * MAX_OUT)); KCHECK(A.alloc(room * 8)); KCHECK(B.alloc(room * 8)); KCHECK(bad.alloc(16));
        KCHECK_HIP(hipMemsetAsync(cnt.p, 0, (range + 1) * 4, stream));
        KCHECK_HIP(hipMemsetAsync(slots.p, 0xFF, (range + 1) * 8 * MAX_OUT, stream));
        KCHECK_HIP(hipMemsetAsync(bad.p, 0, 16, stream));
        return router.init();
    };
    KCHECK(C.agree(local()));
    // ---- 1. registrations -------------------------------------------------------------------------------------------------------
    for (uint64_t c = 0; c < n_chunks; ++c) {
        const uint64_t at = std::min(H, c * chunk), n = std::min(H - at, chunk);
        if (n) KLAUNCH(dg_address_kernel, n, stream, src, at, n, dir.per, first, A.as<u64>(), B.as<u64>());
        Routed r(stream);
        KCHECK(router.send(A.as<u64>(), B.as<u64>(), n, r));
        auto take = [&]() -> int {
            if (r.n) KLAUNCH(dg_register_kernel, r.n, stream, r.a.as<u64>(), r.b.as<u64>(), r.n, dbase, range, cnt.as<u32>(), slots.as<u64>(), bad.as<unsigned long long>());
            KCHECK_HIP(hipGetLastError());
            KCHECK_HIP(hipStreamSynchronize(stream));        // (r's buffers go with the chunk)
            return KATOME_OK;
        };
        KCHECK(C.agree(take()));
    }
    uint64_t h_bad[2] = {0, 0};
    auto sorted = [&]() -> int {
        if (range) KLAUNCH(dg_sort_kernel, range, stream, slots.as<u64>(), range);
        KCHECK_HIP(hipGetLastError());
        KCHECK_HIP(hipMemcpyAsync(h_bad, bad.p, 16, hipMemcpyDeviceToHost, stream));
        KCHECK_HIP(hipStreamSynchronize(stream));
        if (h_bad[0]) { set_error("%llu merged edges start at a vertex outside their directory's range", (unsigned long long)h_bad[0]); return KATOME_E_DEVICE; }
        if (h_bad[1]) { set_error("%llu out-segments beyond the fourth at a vertex", (unsigned long long)h_bad[1]); return KATOME_E_DEVICE; }
        cnt.release(); B.release();
        return ans.alloc((H + 1) * 8 * MAX_OUT);
    };
    KCHECK(C.agree(sorted()));
    // ---- 2. questions and their four-word answers -------------------------------------------------------------------------------
    for (uint64_t c = 0; c < n_chunks; ++c) {
        const uint64_t at = std::min(H, c * chunk), n = std::min(H - at, chunk);
        if (n) KLAUNCH(dg_address_kernel, n, stream, dst, at, n, dir.per, first, A.as<u64>(), (u64*)nullptr);
        Routed r(stream);
        KCHECK(router.send(A.as<u64>(), nullptr, n, r));
        DevBuf reply(stream);
        auto answer = [&]() -> int {
            KCHECK(reply.alloc((r.n + 1) * 8 * MAX_OUT));
            if (r.n) KLAUNCH(dg_answer_kernel, r.n, stream, r.a.as<u64>(), r.n, dbase, range, slots.as<u64>(), reply.as<u64>(), bad.as<unsigned long long>());
            KCHECK_HIP(hipGetLastError());
            return KATOME_OK;
        };
        KCHECK(C.agree(answer()));
        KCHECK(router.reply(r, reply.as<u64>(), ans.as<u64>() + at * MAX_OUT, MAX_OUT));
    }
    // ---- 3. link_first and link_b -----------------------------------------------------------------------------------------------
    auto compact = [&]() -> int {
        slots.release(); A.release();
        KCHECK_HIP(hipMemcpyAsync(h_bad, bad.p, 16, hipMemcpyDeviceToHost, stream));
        KCHECK(count.alloc((H + 1) * 4)); KCHECK(link_first.alloc((H + 1) * 8));
        if (H) {
            KLAUNCH(dg_count_kernel, H, stream, ans.as<u64>(), H, count.as<u32>());
            KCHECK_HIP(hipGetLastError());
            KCHECK(dev_scan_counts(count.as<u32>(), H, link_first.as<u64>(), stream));
        } else KCHECK_HIP(hipMemsetAsync(link_first.p, 0, 8, stream));
        KCHECK_HIP(hipMemcpyAsync(L, link_first.as<u64>() + H, 8, hipMemcpyDeviceToHost, stream));
        KCHECK_HIP(hipStreamSynchronize(stream));
        if (h_bad[0]) { set_error("%llu merged edges end at a vertex outside their directory's range", (unsigned long long)h_bad[0]); return KATOME_E_DEVICE; }
        KCHECK(link_b.alloc((*L + 1) * 8));
        if (H) KLAUNCH(dg_links_kernel, H, stream, ans.as<u64>(), link_first.as<u64>(), H, link_b.as<u64>());
        KCHECK_HIP(hipGetLastError());
        KCHECK_HIP(hipStreamSynchronize(stream));
        return KATOME_OK;
    };
    return C.agree(compact());
}

// (coverage: the S lines of katome_dev_contigs_gfa_coverage, from d->sh_cov)
int dist_contigs_gfa(katome_dist_builder* d, const char* name, bool coverage, GfaTrace& trace, hipStream_t stream) {
    Collective C(d->comm, name);
    const int world = C.world, me = C.rank;
    const uint64_t H = d->sh_edges;
    const long long fail_at = getenv("KATOME_DIST_GFA_FAIL") ? atoll(getenv("KATOME_DIST_GFA_FAIL")) : -1;
    std::vector<uint64_t> per(world, 0);
    KCHECK(d->comm->allgather(H, per.data()));               // (the sizes depend on where this rank's numbers start)
    uint64_t first = 0, total = 0;
    for (int p = 0; p < world; ++p) { if (p < me) first += per[p]; total += per[p]; }
    uint64_t L = 0;
    const double t_join = now_ms();
    const uint64_t sent_before = d->xstats[X_PRUNE].bytes_out;
    KCHECK(dist_gfa_join(d, C, first, d->sh_gfa_link_first, d->sh_gfa_link_b, &L, stream));
    trace.join_ms = now_ms() - t_join; trace.join_bytes = d->xstats[X_PRUNE].bytes_out - sent_before;
    GfaPart part{d->s.k, H, d->sh_weight.as<u32>(), d->sh_kmers.as<u32>(), d->sh_label_off.as<u64>(), d->sh_label.as<uint8_t>(), d->sh_label_bytes,
                 first, me == 0, d->sh_gfa_link_first.as<u64>(), d->sh_gfa_link_b.as<u64>()};
    if (coverage) part.cov = GfaCoverage{d->sh_cov.kmer_sum.as<u64>(), d->sh_cov.kmer_min.as<u32>(), d->sh_cov.kmer_max.as<u32>()};
    GfaPartPlan plan;
    auto measure = [&]() -> int {
        KCHECK(dev_gfa_part_plan(part, plan, stream));
        if (fail_at == (long long)me) { set_error("KATOME_DIST_GFA_FAIL=%lld", fail_at); return KATOME_E_UNSUPPORTED; }
        return KATOME_OK;
    };
    KCHECK(C.agree(measure()));
    uint64_t s_base = 0, s_total = 0, l_before = 0, l_total = 0, links_total = 0;
    KCHECK(d->comm->allgather(plan.s_bytes, per.data()));
    for (int p = 0; p < world; ++p) { if (p < me) s_base += per[p]; s_total += per[p]; }
    KCHECK(d->comm->allgather(plan.l_bytes, per.data()));
    for (int p = 0; p < world; ++p) { if (p < me) l_before += per[p]; l_total += per[p]; }
    KCHECK(d->comm->allgather(L, per.data()));
    for (int p = 0; p < world; ++p) links_total += per[p];
    auto write = [&]() -> int {
        KCHECK(d->sh_gfa_text.alloc(plan.buffer_bytes() + 16));
        hipEvent_t ea = nullptr, eb = nullptr;
        const bool timed = GfaTrace::on() && hipEventCreate(&ea) == hipSuccess && hipEventCreate(&eb) == hipSuccess;
        if (timed) (void)hipEventRecord(ea, stream);
        const int rc = dev_gfa_part_write(part, plan, d->sh_gfa_text.as<uint8_t>(), stream);
        if (timed) (void)hipEventRecord(eb, stream);
        d->sh_gfa_segment_off.adopt(plan.segment_off);
        const hipError_t synced = hipStreamSynchronize(stream);
        if (timed && !rc && synced == hipSuccess && hipEventElapsedTime(&trace.write_ms, ea, eb) == hipSuccess) trace.write_bytes = plan.s_bytes + plan.l_bytes;
        if (ea) (void)hipEventDestroy(ea);
        if (eb) (void)hipEventDestroy(eb);
        KCHECK(rc);
        KCHECK_HIP(synced);
        return KATOME_OK;
    };
    KCHECK(C.agree(write()));
    katome_dist_gfa& g = d->sh_gfa;
    g.n_segments = H; g.first_segment = first; g.total_segments = total;
    g.n_links = L; g.total_links = links_total;
    g.s_bytes = plan.s_bytes; g.s_base = s_base; g.l_bytes = plan.l_bytes; g.l_base = s_total + l_before; g.total_text_bytes = s_total + l_total;
    g.d_text = d->sh_gfa_text.as<uint8_t>(); g.d_link_text = g.d_text + plan.l_offset();
    g.d_segment_off = d->sh_gfa_segment_off.as<u64>(); g.d_link_first = d->sh_gfa_link_first.as<u64>(); g.d_link_b = d->sh_gfa_link_b.as<u64>();
    d->sh_gfa_serial = d->sh_serial; d->sh_gfa_valid = true;
    return KATOME_OK;
}

}  // namespace

int dist_gfa_total_kmers(katome_dist_builder* d, uint64_t* total, hipStream_t stream) {
    KCHECK(check_gfa_builder(d, "katome_unitigs_gfa"));
    Collective C(d->comm, "katome_unitigs_gfa");
    std::vector<uint32_t> kmers;
    auto local = [&]() -> int {
        try { kmers.resize(d->sh_edges); }
        catch (const std::bad_alloc&) { set_error("out of host memory"); return KATOME_E_OOM; }
        if (d->sh_edges) KCHECK_HIP(hipMemcpyAsync(kmers.data(), d->sh_kmers.p, d->sh_edges * 4, hipMemcpyDeviceToHost, stream));
        KCHECK_HIP(hipStreamSynchronize(stream));
        return KATOME_OK;
    };
    KCHECK(C.agree(local()));
    *total = 0;
    for (uint32_t m : kmers) *total += m;
    return d->comm->allreduce(total, 1, OP_SUM);
}

extern "C" {

static int dist_contigs_gfa_entry(katome_dist_builder* d, const char* name, bool coverage, katome_dist_gfa* out, void* stream_) {
    if (out) memset(out, 0, sizeof *out);
    KCHECK(check_gfa_builder(d, name));
    if (!out) { set_error("null argument"); return KATOME_E_ARG; }
    if (coverage && (!d->sh_cov.valid || d->sh_cov.n_edges != d->sh_edges)) {       // (every rank's last shrink was the same call: the same answer everywhere)
        set_error("%s: this builder's last shrink was not a katome_dist_shrink_coverage", name);
        return KATOME_E_ARG;
    }
    hipStream_t stream = (hipStream_t)stream_;
    KCHECK_HIP(hipSetDevice(d->s.device));
    d->comm->use_stream(stream);
    d->sh_gfa_valid = false;
    d->sh_gfa_text.stream = d->sh_gfa_segment_off.stream = d->sh_gfa_link_first.stream = d->sh_gfa_link_b.stream = stream;
    GfaTrace trace{name, d->comm, &d->sh_gfa.total_text_bytes};
    {
        PhaseScope ps(d->b->prof, PH_GFA, stream);
        KCHECK(dist_contigs_gfa(d, name, coverage, trace, stream));
    }
    *out = d->sh_gfa;
    return KATOME_OK;
}
int katome_dist_contigs_gfa(katome_dist_builder* d, katome_dist_gfa* out, void* stream_) {
    return dist_contigs_gfa_entry(d, "katome_dist_contigs_gfa", false, out, stream_);
}
int katome_dist_contigs_gfa_coverage(katome_dist_builder* d, katome_dist_gfa* out, void* stream_) {
    return dist_contigs_gfa_entry(d, "katome_dist_contigs_gfa_coverage", true, out, stream_);
}

int katome_dist_gfa_save(katome_dist_builder* d, const katome_dist_gfa* g, const char* path) {
    const char* name = "katome_dist_gfa_save";
    KCHECK(check_gfa_builder(d, name));
    if (!g || !path) { set_error("null argument"); return KATOME_E_ARG; }
    if (!d->sh_gfa_valid || d->sh_gfa_serial != d->sh_serial || memcmp(g, &d->sh_gfa, sizeof *g) != 0) {
        set_error("%s: not the result of this builder's last katome_dist_contigs_gfa (or the builder was shrunk again since)", name);
        return KATOME_E_ARG;
    }
    KCHECK_HIP(hipSetDevice(d->s.device));
    hipStream_t stream = d->sh_gfa_text.stream;              // (the stream the text was written on)
    d->comm->use_stream(stream);
    const uint64_t my_bytes = g->s_bytes + g->l_bytes;
    GfaTrace trace{name, d->comm, &my_bytes};
    const FilePart parts[2] = {{g->d_text, g->s_bytes, g->s_base}, {g->d_link_text, g->l_bytes, g->l_base}};
    return save_parts(d->comm, name, path, g->total_text_bytes, parts, 2, stream);
}

}  // extern "C"
