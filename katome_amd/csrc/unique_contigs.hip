// unique_contigs.hip -- the strand-unique assembly: one FASTA record per molecule (include/katome_gpu.h has the definitions, word for
// word).  A reverse_complement build keeps a k-mer and its reverse complement as two edges and collapse walks both
// strands, so nearly every molecule comes twice.  For the pieces of one collapse this file gives every contig's mirror BY PIECE
// SEQUENCE, the kept set -- of a molecule's two strands the one whose first copy comes first, with all its copies -- and the text of
// the kept contigs under their ORIGINAL numbers.
//   Contigs.  dev_text_plan validates the pieces and scans the WHOLE flags: piece p lies in contig contig_idx[p + 1] - 1.
//   contig_first_kernel gives every contig its first piece.
//   Mirrors.  dev_find_mirrors (gfa_strand_paths.hip) with that scan and those first pieces: the signature, sort, search, verify and
//   settle steps of the path mirrors, on contigs.  Runs and jumps play no part.
//   Selection.  keep_flag_kernel: contig c is kept iff mirror(c) is none or mirror(mirror(c)) <= mirror(c) -- two gathers, no second
//   search, because twin is an involution and mirror(mirror(c)) is therefore the first contig with c's own pieces.  A scan gives every
//   kept contig its ordinal; piece_keep_kernel flags the pieces of kept contigs, a scan gives them their new places, and
//   compact_kernel scatters them into a new piece list (4 bytes per kept piece) and writes name[ordinal] = c.  A dropped contig vanishes
//   from the list: the text writer relies on every piece being at least a byte.
//   Text.  collapse.hip's writer over the compacted list with the names as its number source (text_write_named_kernel): by output
//   bytes, 8192-byte tiles, 128-bit stores.
// Everything is partitioned by pieces or by output bytes, never by contig: one contig can be 10^6 pieces and the next 10^6 one piece each.
#include "builder.h"
#include "strand_bits.h"

namespace katome {
namespace {

// contig c's first piece (first[n_contigs] = P)
__global__ __launch_bounds__(BLOCK) void contig_first_kernel(const u32* __restrict__ pieces, u64 P, const u64* __restrict__ contig_idx, u64 n_contigs,
                                                             u64* __restrict__ first) {
    if (blockIdx.x == 0 && threadIdx.x == 0) first[n_contigs] = P;
    for (u64 p = (u64)blockIdx.x * BLOCK + threadIdx.x; p < P; p += (u64)gridDim.x * BLOCK)
        if (pieces[p] >> 31) first[contig_idx[p]] = p;
}
// kept iff there is no mirror, or the contig's first copy does not come behind its mirror's
__global__ __launch_bounds__(BLOCK) void keep_flag_kernel(u64 n, const u64* __restrict__ mirror, u32* __restrict__ keep) {
    for (u64 c = (u64)blockIdx.x * BLOCK + threadIdx.x; c < n; c += (u64)gridDim.x * BLOCK) {
        const u64 m = mirror[c];
        keep[c] = m == ~0ull || mirror[m] <= m ? 1u : 0u;
    }
}
__global__ __launch_bounds__(BLOCK) void piece_keep_kernel(u64 P, const u64* __restrict__ contig_idx, const u32* __restrict__ keep, u32* __restrict__ piece_keep) {
    for (u64 p = (u64)blockIdx.x * BLOCK + threadIdx.x; p < P; p += (u64)gridDim.x * BLOCK) piece_keep[p] = keep[contig_idx[p + 1] - 1];
}
// the pieces of kept contigs at their new places (piece_at: the exclusive scan of piece_keep), and every kept contig's name at its
// ordinal (kept_at: the exclusive scan of keep)
__global__ __launch_bounds__(BLOCK) void compact_kernel(const u32* __restrict__ pieces, u64 P, const u64* __restrict__ contig_idx, const u64* __restrict__ kept_at,
                                                        const u64* __restrict__ piece_at, u32* __restrict__ out, u64* __restrict__ name) {
    for (u64 p = (u64)blockIdx.x * BLOCK + threadIdx.x; p < P; p += (u64)gridDim.x * BLOCK) {
        const u64 at = piece_at[p];
        if (piece_at[p + 1] == at) continue;
        const u32 w = pieces[p];
        out[at] = w;
        if (w >> 31) { const u64 c = contig_idx[p]; name[kept_at[c]] = c; }
    }
}

}  // namespace

int dev_unique_plan(uint32_t k, const uint8_t* label, const uint64_t* label_off, uint64_t n_labels, const uint32_t* twin, const uint32_t* pieces,
                    uint64_t n_pieces, uint32_t layout, UniquePlan& plan, hipStream_t stream) {
    plan.n_contigs = plan.n_mirrored = plan.n_self_mirror = plan.n_kept = plan.n_kept_pieces = 0;
    plan.text.n_contigs = plan.text.text_bytes = 0;
    if (layout > KATOME_TEXT_FASTA) { set_error("text: unknown layout %u", layout); return KATOME_E_ARG; }
    const u64 P = n_pieces;
    if (P && (!pieces || !twin)) { set_error("null argument"); return KATOME_E_ARG; }
    plan.mirror.stream = plan.name.stream = plan.pieces.stream = stream;
    TextPlan full;                                       // the checks of every piece and label, and the scan of the WHOLE flags
    KCHECK(dev_text_plan(k, label, label_off, n_labels, pieces, P, KATOME_TEXT_PLAIN, 0, full, stream));
    full.piece_off.release();
    const u64 n = full.n_contigs;
    plan.n_contigs = n;
    if (P == 0) return KATOME_OK;
    const u64* contig_idx = full.contig_idx.as<u64>();
    DevBuf first(stream);
    KCHECK(first.alloc((n + 1) * 8));
    KLAUNCH(contig_first_kernel, P, stream, pieces, P, contig_idx, n, first.as<u64>());
    KCHECK_HIP(hipGetLastError());
    KCHECK(dev_find_mirrors(pieces, P, twin, contig_idx, first.as<u64>(), n, plan.mirror, &plan.n_mirrored, &plan.n_self_mirror, stream));
    first.release();
    DevBuf keep(stream), kept_at(stream), piece_keep(stream), piece_at(stream);
    KCHECK(keep.alloc((n + 1) * 4)); KCHECK(kept_at.alloc((n + 2) * 8)); KCHECK(piece_keep.alloc((P + 1) * 4)); KCHECK(piece_at.alloc((P + 2) * 8));
    {
        KernelScope ks(K_UNIQUE_SELECT, stream, P);
        KLAUNCH(keep_flag_kernel, n, stream, n, plan.mirror.as<u64>(), keep.as<u32>());
        KCHECK_HIP(hipGetLastError());
        KCHECK(dev_scan_counts(keep.as<u32>(), n, kept_at.as<u64>(), stream));
        KLAUNCH(piece_keep_kernel, P, stream, P, contig_idx, keep.as<u32>(), piece_keep.as<u32>());
        KCHECK_HIP(hipGetLastError());
        KCHECK(dev_scan_counts(piece_keep.as<u32>(), P, piece_at.as<u64>(), stream));
        KCHECK_HIP(hipMemcpyAsync(&plan.n_kept, kept_at.as<u64>() + n, 8, hipMemcpyDeviceToHost, stream));
        KCHECK_HIP(hipMemcpyAsync(&plan.n_kept_pieces, piece_at.as<u64>() + P, 8, hipMemcpyDeviceToHost, stream));
        KCHECK_HIP(hipStreamSynchronize(stream));
        KCHECK(plan.name.alloc(plan.n_kept * 8 + 16)); KCHECK(plan.pieces.alloc(plan.n_kept_pieces * 4 + 16));
        KLAUNCH(compact_kernel, P, stream, pieces, P, contig_idx, kept_at.as<u64>(), piece_at.as<u64>(), plan.pieces.as<u32>(), plan.name.as<u64>());
        KCHECK_HIP(hipGetLastError());
    }
    keep.release(); kept_at.release(); piece_keep.release(); piece_at.release(); full.contig_idx.release();
    KCHECK(dev_text_plan(k, label, label_off, n_labels, plan.pieces.as<u32>(), plan.n_kept_pieces, layout, 0, plan.text, stream, plan.name.as<u64>()));
    if (plan.text.n_contigs != plan.n_kept) {
        set_error("unique_contigs: %llu contigs kept, %llu in the compacted pieces", (unsigned long long)plan.n_kept, (unsigned long long)plan.text.n_contigs);
        return KATOME_E_DEVICE;
    }
    return KATOME_OK;
}

int dev_unique_write(uint32_t k, const uint8_t* label, const uint64_t* label_off, uint32_t layout, const UniquePlan& plan, uint64_t* kept_off, uint32_t* kept_len,
                     uint8_t* text, hipStream_t stream) {
    return dev_text_write(k, label, label_off, plan.pieces.as<u32>(), plan.n_kept_pieces, layout, 0, plan.text, kept_off, kept_len, text, stream, plan.name.as<u64>());
}

// the whole result in buffers of its own
static int dev_unique(uint32_t k, const uint8_t* label, const uint64_t* label_off, uint64_t n_labels, const uint32_t* twin, const uint32_t* pieces, uint64_t n_pieces,
                      uint32_t layout, UniqueOutput& out, hipStream_t stream) {
    out.n_contigs = out.n_mirrored = out.n_self_mirror = out.n_kept = out.text_bytes = 0; out.layout = layout;
    UniquePlan plan;
    KCHECK(dev_unique_plan(k, label, label_off, n_labels, twin, pieces, n_pieces, layout, plan, stream));
    KCHECK(out.kept_off.alloc((plan.n_kept + 1) * 8, stream)); KCHECK(out.kept_len.alloc((plan.n_kept + 1) * 4, stream));
    KCHECK(out.text.alloc((plan.text.text_bytes + 15) / 16 * 16 + 16, stream));
    KCHECK(dev_unique_write(k, label, label_off, layout, plan, out.kept_off.as<u64>(), out.kept_len.as<u32>(), out.text.as<uint8_t>(), stream));
    KCHECK_HIP(hipStreamSynchronize(stream));
    out.contig_mirror.stream = out.kept_name.stream = stream;
    out.contig_mirror.adopt(plan.mirror); out.kept_name.adopt(plan.name);
    out.n_contigs = plan.n_contigs; out.n_mirrored = plan.n_mirrored; out.n_self_mirror = plan.n_self_mirror; out.n_kept = plan.n_kept;
    out.text_bytes = plan.text.text_bytes;
    return KATOME_OK;
}

}  // namespace katome

extern "C" {

int katome_dev_unique_contigs_arrays(int device, uint32_t k, const uint8_t* d_label, const uint64_t* d_label_off, uint64_t n_labels, const uint64_t* d_edge_twin,
                                     const uint32_t* d_pieces, uint64_t n_pieces, uint32_t layout, uint64_t* d_contig_mirror, uint64_t contig_cap,
                                     uint64_t* d_kept_name, uint64_t* d_kept_off, uint32_t* d_kept_len, uint64_t kept_cap, uint8_t* d_text, uint64_t text_cap,
                                     uint64_t* counts, void* stream_) {
    if (!counts) { set_error("null argument"); return KATOME_E_ARG; }
    for (int i = 0; i < 5; ++i) counts[i] = 0;
    KCHECK(use_device(device));
    KCHECK(check_k(k));
    hipStream_t stream = (hipStream_t)stream_;
    const u64 E = n_labels;
    if (E >= 0xFFFFFFFFull) { set_error("unique_contigs: %llu labels, at most 2^32 - 2", (unsigned long long)E); return KATOME_E_UNSUPPORTED; }
    if (n_pieces >= 0x80000000ull) { set_error("unique_contigs: %llu pieces, at most 2^31 - 1", (unsigned long long)n_pieces); return KATOME_E_UNSUPPORTED; }
    if ((uintptr_t)d_label & 3) { set_error("text: d_label must be 4-byte aligned (the kernel reads the aligned words around the bytes it needs)"); return KATOME_E_ARG; }
    if ((E && !d_edge_twin) || (n_pieces && !d_pieces)) { set_error("null argument"); return KATOME_E_ARG; }
    // KATOME_UNIQUE_TRACE=1: the kernels' own times on stderr (there is no builder whose profile could hold them)
    ArraysTrace trace("KATOME_UNIQUE_TRACE", "katome_dev_unique_contigs_arrays");
    UniquePlan plan;
    {
        PhaseScope ps(trace.prof, PH_UNIQUE_CONTIGS, stream);
        DevBuf twin(stream);
        KCHECK(twin.alloc(E * 4));
        KCHECK(dev_strand_twin_check("unique_contigs", E, d_edge_twin, twin.as<u32>(), stream));
        KCHECK(dev_unique_plan(k, d_label, d_label_off, n_labels, twin.as<u32>(), d_pieces, n_pieces, layout, plan, stream));
        counts[0] = plan.n_contigs; counts[1] = plan.n_kept; counts[2] = plan.text.text_bytes; counts[3] = plan.n_mirrored; counts[4] = plan.n_self_mirror;
        if (!d_text) return KATOME_OK;
        if ((plan.n_contigs && !d_contig_mirror) || contig_cap < plan.n_contigs || (plan.n_kept && (!d_kept_name || !d_kept_off || !d_kept_len)) ||
            kept_cap < plan.n_kept || !text_fits(plan.text.text_bytes, text_cap, d_text)) {
            set_error("unique_contigs: %llu contigs, %llu kept and %llu bytes (rounded up to 16, 16-byte aligned) do not fit the caller's arrays",
                      (unsigned long long)plan.n_contigs, (unsigned long long)plan.n_kept, (unsigned long long)plan.text.text_bytes);
            return KATOME_E_ARG;
        }
        KCHECK(dev_unique_write(k, d_label, d_label_off, layout, plan, d_kept_off, d_kept_len, d_text, stream));
        if (plan.n_contigs) KCHECK_HIP(hipMemcpyAsync(d_contig_mirror, plan.mirror.p, plan.n_contigs * 8, hipMemcpyDeviceToDevice, stream));
        if (plan.n_kept) KCHECK_HIP(hipMemcpyAsync(d_kept_name, plan.name.p, plan.n_kept * 8, hipMemcpyDeviceToDevice, stream));
    }
    KCHECK_HIP(hipStreamSynchronize(stream));
    trace.print(K_GFASP_SIGS, K_UNIQUE_SELECT, plan.text.text_bytes, n_pieces, "pieces", plan.n_contigs, "contigs");
    return KATOME_OK;
}

// for the builder's last katome_dev_collapse: the twins of the shrunk graph its pieces name (gfa_strands.hip's, without the link join),
// then the selection and the text
int katome_dev_collapse_unique(katome_builder* b, uint32_t layout, katome_dev_unique_assembly* out, void* stream_) {
    if (!b || !out) { set_error("null argument"); return KATOME_E_ARG; }
    hipStream_t stream = (hipStream_t)stream_;
    KCHECK_HIP(hipSetDevice(b->s.device));
    memset(out, 0, sizeof *out);
    out->layout = layout;
    if (layout > KATOME_TEXT_FASTA) { set_error("collapse_unique: unknown layout %u", layout); return KATOME_E_ARG; }
    if (!b->collapse_valid) { set_error("collapse_unique: no collapse result"); return KATOME_E_ARG; }
    const ShrinkOutput& sh = b->collapse_shrunk;
    UniqueOutput& o = b->unique;
    o.n_contigs = o.n_mirrored = o.n_self_mirror = o.n_kept = o.text_bytes = 0; o.layout = layout;
    if (b->collapse_n_pieces) {
        PhaseScope ps(b->prof, PH_UNIQUE_CONTIGS, stream);
        DevBuf twin(stream);
        KCHECK(dev_strand_twins(gfa_graph_of(b->s.k, sh), twin, true, stream));
        KCHECK(dev_unique(b->s.k, sh.edge_label.as<uint8_t>(), sh.edge_label_off.as<u64>(), sh.n_edges, twin.as<u32>(), b->collapse_pieces.as<u32>(),
                          b->collapse_n_pieces, layout, o, stream));
    }
    if (o.n_contigs == 0) return KATOME_OK;
    out->n_contigs = o.n_contigs; out->n_mirrored = o.n_mirrored; out->n_self_mirror = o.n_self_mirror; out->n_kept = o.n_kept; out->text_bytes = o.text_bytes;
    out->d_contig_mirror = o.contig_mirror.as<u64>(); out->d_kept_name = o.kept_name.as<u64>(); out->d_kept_off = o.kept_off.as<u64>();
    out->d_kept_len = o.kept_len.as<u32>(); out->d_text = o.text.as<uint8_t>();
    return KATOME_OK;
}

}  // extern "C"
