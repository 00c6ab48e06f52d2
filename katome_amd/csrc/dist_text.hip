// dist_text.hip -- what comes out at the end of the sharded pipeline, no gather: the text of the sharded shrink's merged edges
// (unitigs), Contigs::stats of all ranks' contigs (reference src/katome/stats/contigs.rs:31-89) and the FASTA file
// (Contigs::save_to_file, asm/mod.rs:57-72), written by every rank at its own offset (dist_save.h).  Memory per rank is O(share) -- the text of
// its own merged edges -- plus one chunk of host memory while the file is written.
//
// The order is RANK-MAJOR: contig first_contig + j is this rank's merged edge j -- entry j of every array of katome_dist_contigs,
// which by packed key is d_edge_head_id order and in first-seen order the order of the rank's own edges --, first_contig the merged
// edges of the ranks before it, so the ranks' texts one after the other are one valid text with headers >katome_0 ...
// >katome_<total - 1>.  Sorting the records into the global head-id order of the one-GPU result would move the whole text between
// ranks; that is deliberately left out (a reader that wants that order sorts by d_edge_head_id).
//
// The text is collapse.hip's kernel on the rank's labels with a starting number (dev_text_plan / dev_text_write, no piece list).
// The stats never see another rank's lengths: contig_select.h restates the reference's scans as four radix selections over the
// k-mer counts, 32 bits in four 8-bit passes; per pass contig_select_kernel reads the rank's counts once and adds (count, sum) of
// the contigs under each selection's prefix into 256 LDS bins (u64, 16 KiB in all), one allreduce of 4 * 256 * 2 words follows
// and the host picks the digits.  Nearly every unitig is short, so in the first passes a whole wave falls into one bin: a wave
// whose digits agree adds its sum once instead of serialising 64 atomics on one address.
//
// Between collectives every rank's own status is agreed (dist_agree.h): allocations, launches, plan errors -- 2^31 edges on a
// rank, a contig of 2^32 bases -- and write errors come back on every rank with a message that names the rank.
// KATOME_DIST_TEXT_FAIL=<rank> (tests): that rank fails after the plan.  KATOME_DIST_TEXT_CHUNK=<bytes>: the host buffer of the
// file writer (default 64 MiB).  KATOME_DIST_TEXT_TRACE=1: every rank's wall time per call on stderr (tools/bench_dist_text.py).
#include <chrono>

#include "contig_select.h"
#include "dist_agree.h"
#include "dist_builder.h"
#include "dist_save.h"

namespace {

struct Trace {                         // KATOME_DIST_TEXT_TRACE: "[<call>] rank r/n: <ms> ms, <bytes> bytes" when the call returns
    const char* name; katome_comm* comm; const uint64_t* bytes;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    ~Trace() {
        static const bool on = getenv("KATOME_DIST_TEXT_TRACE") != nullptr;
        if (on) fprintf(stderr, "[%s] rank %d/%d: %.3f ms, %llu bytes\n", name, comm->rank(), comm->world(),
                        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(), (unsigned long long)(bytes ? *bytes : 0));
    }
};

struct SelectPrefixes { u32 p[SELECTS]; };

// one pass of the selections over this rank's contigs: bins[s][digit] += {1, m} for every m whose bits above the digit equal
// pre.p[s] (first pass: every m, and selection 0 stands for all four)
__global__ __launch_bounds__(BLOCK) void contig_select_kernel(const u32* __restrict__ kmers, u64 n, u32 shift, u32 first, SelectPrefixes pre,
                                                              unsigned long long* __restrict__ bins) {
    __shared__ unsigned long long s_bins[SELECT_WORDS];
    for (u32 i = threadIdx.x; i < (u32)SELECT_WORDS; i += BLOCK) s_bins[i] = 0;
    __syncthreads();
    const u32 lane = threadIdx.x & 63;
    const int n_sel = first ? 1 : SELECTS;
    for (u64 base = (u64)blockIdx.x * BLOCK; base < n; base += (u64)gridDim.x * BLOCK) {      // (whole waves stay in the loop: they vote)
        const u64 i = base + threadIdx.x;
        const bool valid = i < n;
        const u32 m = valid ? kmers[i] : 0;
        const u32 digit = (m >> shift) & 255u;
        const u32 high = first ? 0 : m >> (shift + 8);
        for (int s = 0; s < n_sel; ++s) {
            const bool in = valid && (first || high == pre.p[s]);
            const u32 key = in ? digit : 256u;
            const u32 lead = __builtin_amdgcn_readfirstlane(key);
            if (__all(key == lead)) {                        // one bin for the whole wave (or nothing to add)
                if (lead != 256u) {
                    const u64 sum = (u64)wave_sum(m & 0xFFFFu) + ((u64)wave_sum(m >> 16) << 16);
                    if (lane == 0) {
                        atomicAdd(&s_bins[((u32)s * SELECT_BINS + lead) * 2], 64ull);
                        atomicAdd(&s_bins[((u32)s * SELECT_BINS + lead) * 2 + 1], (unsigned long long)sum);
                    }
                }
            } else if (in) {
                atomicAdd(&s_bins[((u32)s * SELECT_BINS + digit) * 2], 1ull);
                atomicAdd(&s_bins[((u32)s * SELECT_BINS + digit) * 2 + 1], (unsigned long long)m);
            }
        }
    }
    __syncthreads();
    for (u32 i = threadIdx.x; i < (u32)(n_sel * SELECT_BINS * 2); i += BLOCK)
        if (s_bins[i]) atomicAdd(&bins[i], s_bins[i]);
}

int contig_stats_shards(katome_comm* comm, const u32* d_kmers, u64 n, u32 k, u64 genome_len, katome_contig_stats* out, hipStream_t stream) {
    const char* name = "katome_dist_contig_stats";
    Collective C(comm, name);
    ContigSelect sel(k, genome_len);
    DevBuf bins(stream);
    std::vector<uint64_t> h(SELECT_WORDS, 0);
    bool more = true;
    for (int pass = 0; pass < SELECT_PASSES && more; ++pass) {
        auto local = [&]() -> int {
            if (pass == 0) {
                if (n && !d_kmers) { set_error("null argument"); return KATOME_E_ARG; }
                KCHECK(bins.alloc(SELECT_WORDS * 8));
            }
            KCHECK_HIP(hipMemsetAsync(bins.p, 0, SELECT_WORDS * 8, stream));
            if (n) {
                SelectPrefixes pre;
                for (int s = 0; s < SELECTS; ++s) pre.p[s] = sel.prefix[s];
                hipLaunchKernelGGL(contig_select_kernel, dim3(grid_for(n, BLOCK * 8, 256u * 8u)), dim3(BLOCK), 0, stream, d_kmers, n,
                                   ContigSelect::shift_of(pass), pass == 0 ? 1u : 0u, pre, bins.as<unsigned long long>());
                KCHECK_HIP(hipGetLastError());
            }
            KCHECK_HIP(hipMemcpyAsync(h.data(), bins.p, SELECT_WORDS * 8, hipMemcpyDeviceToHost, stream));
            KCHECK_HIP(hipStreamSynchronize(stream));
            if (pass == 0) for (int s = 1; s < SELECTS; ++s) std::copy(h.begin(), h.begin() + SELECT_BINS * 2, h.begin() + (size_t)s * SELECT_BINS * 2);
            return KATOME_OK;
        };
        KCHECK(C.agree(local()));
        KCHECK(comm->allreduce(h.data(), SELECT_WORDS, OP_SUM));
        more = sel.step(h.data());
    }
    ContigStats st;
    const int which = sel.result(&st);
    out->n50 = st.n50; out->l50 = st.l50; out->n90 = st.n90; out->ng50 = st.ng50;
    if (which < 0) { set_error("%s: the ranks' bins do not add up to one list of contigs", name); return KATOME_E_DEVICE; }
    return contig_stats_status(which);
}

int check_text_builder(katome_dist_builder* d, const char* name) {
    if (!d) { set_error("null argument"); return KATOME_E_ARG; }
    if (d->gathered) { set_error("%s: the ranks' shares were gathered (katome_dist_gather)", name); return KATOME_E_ARG; }
    if (!d->sh_valid) { set_error("%s: call katome_dist_shrink first (the builder holds no result of it)", name); return KATOME_E_ARG; }
    return KATOME_OK;
}

int dist_contigs_text(katome_dist_builder* d, uint32_t layout, hipStream_t stream) {
    const char* name = "katome_dist_contigs_text";
    Collective C(d->comm, name);
    const int world = C.world, me = C.rank;
    const uint64_t H = d->sh_edges;
    const long long fail_at = getenv("KATOME_DIST_TEXT_FAIL") ? atoll(getenv("KATOME_DIST_TEXT_FAIL")) : -1;
    std::vector<uint64_t> per(world, 0);
    KCHECK(d->comm->allgather(H, per.data()));               // (the FASTA sizes depend on where this rank's numbers start)
    uint64_t first = 0, total = 0;
    for (int p = 0; p < world; ++p) { if (p < me) first += per[p]; total += per[p]; }
    TextPlan plan;
    TextOutput& out = d->sh_text;
    const uint8_t* label = d->sh_label.as<uint8_t>();
    const uint64_t* label_off = d->sh_label_off.as<uint64_t>();
    auto measure = [&]() -> int {
        KCHECK(dev_text_plan(d->s.k, label, label_off, H, nullptr, H, layout, first, plan, stream));
        if (fail_at == (long long)me) { set_error("KATOME_DIST_TEXT_FAIL=%lld", fail_at); return KATOME_E_UNSUPPORTED; }
        return KATOME_OK;
    };
    KCHECK(C.agree(measure()));
    KCHECK(d->comm->allgather(plan.text_bytes, per.data()));
    uint64_t base = 0, total_bytes = 0;
    for (int p = 0; p < world; ++p) { if (p < me) base += per[p]; total_bytes += per[p]; }
    auto write = [&]() -> int {
        KCHECK(out.contig_off.alloc((plan.n_contigs + 1) * 8, stream)); KCHECK(out.contig_len.alloc((plan.n_contigs + 1) * 4, stream));
        KCHECK(out.text.alloc((plan.text_bytes + 15) / 16 * 16 + 16, stream));
        KCHECK(dev_text_write(d->s.k, label, label_off, nullptr, H, layout, first, plan, out.contig_off.as<uint64_t>(), out.contig_len.as<uint32_t>(),
                              out.text.as<uint8_t>(), stream));
        KCHECK_HIP(hipStreamSynchronize(stream));
        return KATOME_OK;
    };
    KCHECK(C.agree(write()));
    out.n_contigs = plan.n_contigs; out.text_bytes = plan.text_bytes; out.layout = layout;
    d->sh_text_first = first; d->sh_text_contigs = total; d->sh_text_base = base; d->sh_text_total = total_bytes;
    d->sh_text_serial = d->sh_serial; d->sh_text_valid = true;
    return KATOME_OK;
}

// the FASTA file: this rank's text is one part of it (dist_save.h)
int dist_contigs_save(katome_dist_builder* d, const char* path, hipStream_t stream) {
    const FilePart part{d->sh_text.text.as<uint8_t>(), d->sh_text.text_bytes, d->sh_text_base};
    return save_parts(d->comm, "katome_dist_contigs_save", path, d->sh_text_total, &part, 1, stream);
}

}  // namespace

extern "C" {

int katome_dist_contigs_text(katome_dist_builder* d, uint32_t layout, katome_dist_assembly* out, void* stream_) {
    const char* name = "katome_dist_contigs_text";
    if (out) memset(out, 0, sizeof *out);
    KCHECK(check_text_builder(d, name));
    if (!out) { set_error("null argument"); return KATOME_E_ARG; }
    if (layout > KATOME_TEXT_FASTA) { set_error("%s: unknown layout %u", name, layout); return KATOME_E_ARG; }
    hipStream_t stream = (hipStream_t)stream_;
    KCHECK_HIP(hipSetDevice(d->s.device));
    d->comm->use_stream(stream);
    d->sh_text_valid = false;
    Trace trace{name, d->comm, &d->sh_text.text_bytes};
    {
        PhaseScope ps(d->b->prof, PH_COLLAPSE, stream);
        KCHECK(dist_contigs_text(d, layout, stream));
    }
    const TextOutput& t = d->sh_text;
    out->n_contigs = t.n_contigs; out->first_contig = d->sh_text_first; out->total_contigs = d->sh_text_contigs;
    out->text_bytes = t.text_bytes; out->text_base = d->sh_text_base; out->total_text_bytes = d->sh_text_total;
    out->layout = layout;
    out->d_contig_off = t.contig_off.as<uint64_t>(); out->d_contig_len = t.contig_len.as<uint32_t>(); out->d_text = t.text.as<uint8_t>();
    return KATOME_OK;
}

int katome_dist_contig_stats_arrays(katome_comm* c, int device, const uint32_t* d_edge_kmers, uint64_t n, uint32_t k, uint64_t original_genome_length,
                                    katome_contig_stats* out, void* stream_) {
    if (!c || !out) { set_error("null argument"); return KATOME_E_ARG; }
    memset(out, 0, sizeof *out);
    KCHECK(use_device(device));
    KCHECK(check_k(k));
    hipStream_t stream = (hipStream_t)stream_;
    c->use_stream(stream);
    const uint64_t bytes = n * 4 * SELECT_PASSES;
    Trace trace{"katome_dist_contig_stats", c, &bytes};
    return contig_stats_shards(c, d_edge_kmers, n, k, original_genome_length, out, stream);
}

int katome_dist_contig_stats(katome_dist_builder* d, uint64_t original_genome_length, katome_contig_stats* out, void* stream_) {
    if (out) memset(out, 0, sizeof *out);
    KCHECK(check_text_builder(d, "katome_dist_contig_stats"));
    if (!out) { set_error("null argument"); return KATOME_E_ARG; }
    hipStream_t stream = (hipStream_t)stream_;
    KCHECK_HIP(hipSetDevice(d->s.device));
    d->comm->use_stream(stream);
    const uint64_t bytes = d->sh_edges * 4 * SELECT_PASSES;
    Trace trace{"katome_dist_contig_stats", d->comm, &bytes};
    return contig_stats_shards(d->comm, d->sh_kmers.as<uint32_t>(), d->sh_edges, d->s.k, original_genome_length, out, stream);
}

int katome_dist_contigs_save(katome_dist_builder* d, const katome_dist_assembly* a, const char* path) {
    const char* name = "katome_dist_contigs_save";
    KCHECK(check_text_builder(d, name));
    if (!a || !path) { set_error("null argument"); return KATOME_E_ARG; }
    if (!d->sh_text_valid || d->sh_text_serial != d->sh_serial || a->d_text != d->sh_text.text.as<uint8_t>() || a->text_bytes != d->sh_text.text_bytes ||
        a->text_base != d->sh_text_base || a->total_text_bytes != d->sh_text_total) {
        set_error("%s: not the result of this builder's last katome_dist_contigs_text (or the builder was shrunk again since)", name);
        return KATOME_E_ARG;
    }
    KCHECK_HIP(hipSetDevice(d->s.device));
    hipStream_t stream = d->sh_text.text.stream;             // (the stream the text was written on)
    d->comm->use_stream(stream);
    Trace trace{name, d->comm, &d->sh_text.text_bytes};
    return dist_contigs_save(d, path, stream);
}

}  // extern "C"
