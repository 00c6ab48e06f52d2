// gfa_paths.hip -- collapse's contigs as GFA 1 P lines over the segments of the shrunk graph (include/katome_gpu.h has the format):
//   P\tkatome_<c>\t<s0>+,<s1>+,...,<sn>+\t*\n            run 0 of contig c
//   P\tkatome_<c>.<r>\t<s..>+,...\t*\n                    run r = 1, 2, ... of contig c
// Piece p of the collapse names the shrunk edge appended at step p: segment <id> of that graph's GFA (gfa.hip).  A contig is a path
// over segments, but not always ONE path: after a simple loop (collapser.rs:181-193; collapse_exact.h:176-180) the walk appends the
// entering edge b->c, the return edge c->b and goes on FROM c, so the next piece does not start where the last one ended and the two
// have no L line.  A piece therefore starts a RUN when it begins a contig (KATOME_PIECE_WHOLE) or edge_dst[id(p - 1)] != edge_src[id(p)]
// (a jump), and every run is a P line of its own: n_paths = n_contigs + n_jumps.
//   The plan: path_flag_kernel checks every piece (an id below n_edges, a first piece that begins a contig) before anything is read
//   through an id, and flags the pieces that start a run and those that start a contig; two scans give every piece its path and its
//   contig, path_fill_kernel every path its contig and first piece and every contig its first path (the run index is the difference);
//   path_size_kernel counts a piece's bytes -- "<id>+," or, on a run's last piece, "<id>+\t*\n", behind the line's head on its first
//   -- and a third scan gives the 64-bit byte offsets (2^31 - 1 pieces can be tens of GB).
//   gfa_paths_write_kernel loops over the tile both path texts share (write_piece_tile of gfa_path_lines.h: partitioned by OUTPUT bytes,
//   every piece formatted once into the LDS image of gfa_image.h, 128-bit stores) with this text's name of a piece: its id and '+'.
//   Neither a thread per piece nor one per path touches global memory: one path can be 10^6 pieces and the next 10^6 paths one piece
//   each.
#include "builder.h"
#include "gfa_path_lines.h"

namespace katome {
namespace {

constexpr u32 WHOLE = KATOME_PIECE_WHOLE;
enum { ERR_PIECE = 1, ERR_FIRST = 2 };

// piece p: checked, then run[p] = it starts a run, whole[p] = it starts a contig
__global__ __launch_bounds__(BLOCK) void path_flag_kernel(u64 E, const u64* __restrict__ src, const u64* __restrict__ dst, const u32* __restrict__ pieces, u64 P,
                                                          u32* __restrict__ run, u32* __restrict__ whole, u32* __restrict__ err) {
    for (u64 p = (u64)blockIdx.x * BLOCK + threadIdx.x; p < P; p += (u64)gridDim.x * BLOCK) {
        const u32 w = pieces[p], id = w & ~WHOLE;
        u32 starts = w >> 31;
        run[p] = whole[p] = 0;
        if (id >= E) { atomicOr(err, (u32)ERR_PIECE); continue; }
        if (p == 0) {
            if (!starts) atomicOr(err, (u32)ERR_FIRST);
        } else if (!starts) {
            const u32 before = pieces[p - 1] & ~WHOLE;                 // (an id that names no edge is reported by its own piece)
            if (before < E && dst[before] != src[id]) starts = 1;      // a jump
        }
        whole[p] = w >> 31; run[p] = starts;
    }
}

// path_idx / contig_idx: the exclusive scans of the two flags (one entry more than pieces): a piece that starts a run is the first
// of path path_idx[p], and lies in contig contig_idx[p + 1] - 1
__global__ __launch_bounds__(BLOCK) void path_fill_kernel(const u32* __restrict__ pieces, u64 P, const u64* __restrict__ path_idx, const u64* __restrict__ contig_idx,
                                                          u64* __restrict__ path_contig, u64* __restrict__ path_first_piece, u64* __restrict__ contig_first_path) {
    if (blockIdx.x == 0 && threadIdx.x == 0) path_first_piece[path_idx[P]] = P;
    for (u64 p = (u64)blockIdx.x * BLOCK + threadIdx.x; p < P; p += (u64)gridDim.x * BLOCK) {
        const u64 path = path_idx[p];
        if (path_idx[p + 1] == path) continue;
        const u64 c = contig_idx[p + 1] - 1;                           // (>= 0: the first piece begins a contig)
        path_contig[path] = c; path_first_piece[path] = p;
        if (pieces[p] >> 31) contig_first_path[c] = path;
    }
}

__global__ __launch_bounds__(BLOCK) void path_size_kernel(const u32* __restrict__ pieces, u64 P, const u64* __restrict__ path_idx, const u64* __restrict__ path_contig,
                                                          const u64* __restrict__ contig_first_path, u32* __restrict__ size) {
    for (u64 p = (u64)blockIdx.x * BLOCK + threadIdx.x; p < P; p += (u64)gridDim.x * BLOCK) {
        u32 n = decimal_digits(pieces[p] & ~WHOLE) + 2;                // "<id>+,"
        const u64 path = path_idx[p];
        if (path_idx[p + 1] != path) { const u64 c = path_contig[path]; n += run_head_bytes(c, path - contig_first_path[c]); }
        if (p + 1 == P || path_idx[p + 2] != path_idx[p + 1]) n += 2;  // "<id>+\t*\n"
        size[p] = n;
    }
}

__global__ __launch_bounds__(BLOCK) void path_line_off_kernel(u64 P, const u64* __restrict__ path_idx, const u64* __restrict__ piece_off, u64* __restrict__ path_line_off) {
    if (blockIdx.x == 0 && threadIdx.x == 0) path_line_off[path_idx[P]] = piece_off[P];
    for (u64 p = (u64)blockIdx.x * BLOCK + threadIdx.x; p < P; p += (u64)gridDim.x * BLOCK)
        if (path_idx[p + 1] != path_idx[p]) path_line_off[path_idx[p]] = piece_off[p];
}

__global__ __launch_bounds__(BLOCK) void gfa_paths_write_kernel(const u32* __restrict__ pieces, u32 P, const u64* __restrict__ path_idx, const u64* __restrict__ piece_off,
                                                                const u64* __restrict__ path_contig, const u64* __restrict__ contig_first_path, u64 total,
                                                                uint8_t* __restrict__ text) {
    const auto name = [=](u32 p) { return PieceName{pieces[p] & ~WHOLE, '+'}; };
    for (u64 base = (u64)blockIdx.x * TILE; base < total; base += (u64)gridDim.x * TILE) {
        const int len = tile_len(base, total);
        write_piece_tile(name, P, workgroup_search(piece_off, P, base), workgroup_search(piece_off, P, base + len - 1), base, len, path_idx, piece_off, path_contig,
                         contig_first_path, total, text);
    }
}

}  // namespace

int dev_gfa_paths_runs(uint64_t n_edges, const uint64_t* edge_src, const uint64_t* edge_dst, const uint32_t* pieces, uint64_t n_pieces, GfaPathsPlan& plan,
                       DevBuf& run, hipStream_t stream) {
    plan.n_paths = plan.n_contigs = plan.text_bytes = 0;
    const u64 P = n_pieces, E = n_edges;
    if (P >= 0x80000000ull) { set_error("gfa_paths: %llu pieces, at most 2^31 - 1", (unsigned long long)P); return KATOME_E_ARG; }
    plan.path_idx.stream = plan.piece_off.stream = plan.contig_first_path.stream = plan.path_line_off.stream = plan.path_contig.stream = plan.path_first_piece.stream = stream;
    if (P == 0) {                                                       // no pieces: an empty region, path_line_off = path_first_piece = {0}
        KCHECK(plan.path_line_off.alloc(8)); KCHECK(plan.path_first_piece.alloc(8)); KCHECK(plan.path_contig.alloc(8));
        KCHECK_HIP(hipMemsetAsync(plan.path_line_off.p, 0, 8, stream)); KCHECK_HIP(hipMemsetAsync(plan.path_first_piece.p, 0, 8, stream));
        KCHECK_HIP(hipStreamSynchronize(stream));
        return KATOME_OK;
    }
    if (!pieces || (E && (!edge_src || !edge_dst))) { set_error("null argument"); return KATOME_E_ARG; }
    const dim3 grid(grid_for(P, BLOCK, 256u * 32u)), blk(BLOCK);
    DevBuf whole(stream), contig_idx(stream), tail(stream);
    run.stream = stream;
    KCHECK(run.alloc(P * 4)); KCHECK(whole.alloc(P * 4)); KCHECK(tail.alloc(16));
    KCHECK(plan.path_idx.alloc((P + 1) * 8)); KCHECK(contig_idx.alloc((P + 1) * 8));
    KCHECK_HIP(hipMemsetAsync(tail.p, 0, 16, stream));
    hipLaunchKernelGGL(path_flag_kernel, grid, blk, 0, stream, E, edge_src, edge_dst, pieces, P, run.as<u32>(), whole.as<u32>(), tail.as<u32>());
    KCHECK_HIP(hipGetLastError());
    u32 err = 0;
    KCHECK_HIP(hipMemcpyAsync(&err, tail.p, 4, hipMemcpyDeviceToHost, stream));
    KCHECK_HIP(hipStreamSynchronize(stream));
    if (err & ERR_FIRST) { set_error("gfa_paths: the first piece does not begin a contig"); return KATOME_E_ARG; }
    if (err & ERR_PIECE) { set_error("gfa_paths: a piece names an edge that is not below n_edges"); return KATOME_E_ARG; }
    KCHECK(dev_scan_counts(run.as<u32>(), P, plan.path_idx.as<u64>(), stream));
    KCHECK(dev_scan_counts(whole.as<u32>(), P, contig_idx.as<u64>(), stream));
    u64 n_paths = 0, n_contigs = 0;
    KCHECK_HIP(hipMemcpyAsync(&n_paths, plan.path_idx.as<u64>() + P, 8, hipMemcpyDeviceToHost, stream));
    KCHECK_HIP(hipMemcpyAsync(&n_contigs, contig_idx.as<u64>() + P, 8, hipMemcpyDeviceToHost, stream));
    KCHECK_HIP(hipStreamSynchronize(stream));
    whole.release();
    KCHECK(plan.path_contig.alloc(n_paths * 8)); KCHECK(plan.path_first_piece.alloc((n_paths + 1) * 8)); KCHECK(plan.path_line_off.alloc((n_paths + 1) * 8));
    KCHECK(plan.contig_first_path.alloc(n_contigs * 8)); KCHECK(plan.piece_off.alloc((P + 1) * 8));
    hipLaunchKernelGGL(path_fill_kernel, grid, blk, 0, stream, pieces, P, plan.path_idx.as<u64>(), contig_idx.as<u64>(), plan.path_contig.as<u64>(),
                       plan.path_first_piece.as<u64>(), plan.contig_first_path.as<u64>());
    KCHECK_HIP(hipGetLastError());
    KCHECK_HIP(hipStreamSynchronize(stream));                           // (contig_idx is freed on return)
    plan.n_paths = n_paths; plan.n_contigs = n_contigs;
    return KATOME_OK;
}

// size: every piece's bytes -> piece_off, path_line_off, text_bytes (no pieces: dev_gfa_paths_runs has left the empty region)
int dev_gfa_paths_offsets(uint64_t n_pieces, const uint32_t* size, GfaPathsPlan& plan, hipStream_t stream) {
    const u64 P = n_pieces;
    if (P == 0) return KATOME_OK;
    KCHECK(dev_scan_counts(size, P, plan.piece_off.as<u64>(), stream));
    hipLaunchKernelGGL(path_line_off_kernel, dim3(grid_for(P, BLOCK, 256u * 32u)), dim3(BLOCK), 0, stream, P, plan.path_idx.as<u64>(), plan.piece_off.as<u64>(),
                       plan.path_line_off.as<u64>());
    KCHECK_HIP(hipGetLastError());
    KCHECK_HIP(hipMemcpyAsync(&plan.text_bytes, plan.piece_off.as<u64>() + P, 8, hipMemcpyDeviceToHost, stream));
    KCHECK_HIP(hipStreamSynchronize(stream));
    return KATOME_OK;
}

int dev_gfa_paths_plan(uint64_t n_edges, const uint64_t* edge_src, const uint64_t* edge_dst, const uint32_t* pieces, uint64_t n_pieces, GfaPathsPlan& plan,
                       hipStream_t stream) {
    DevBuf size(stream);                                                // (the run flags first, then every piece's bytes)
    KCHECK(dev_gfa_paths_runs(n_edges, edge_src, edge_dst, pieces, n_pieces, plan, size, stream));
    if (n_pieces == 0) return KATOME_OK;
    hipLaunchKernelGGL(path_size_kernel, dim3(grid_for(n_pieces, BLOCK, 256u * 32u)), dim3(BLOCK), 0, stream, pieces, (u64)n_pieces, plan.path_idx.as<u64>(),
                       plan.path_contig.as<u64>(), plan.contig_first_path.as<u64>(), size.as<u32>());
    KCHECK_HIP(hipGetLastError());
    return dev_gfa_paths_offsets(n_pieces, size.as<u32>(), plan, stream);
}

int dev_gfa_paths_write(const uint32_t* pieces, uint64_t n_pieces, const GfaPathsPlan& plan, uint8_t* text, hipStream_t stream) {
    if (n_pieces == 0 || plan.text_bytes == 0) return KATOME_OK;
    const u64 tiles = (plan.text_bytes + TILE - 1) / TILE;
    KernelScope ks(K_GFA_PATHS_WRITE, stream, plan.text_bytes);
    hipLaunchKernelGGL(gfa_paths_write_kernel, dim3(grid_for(tiles, 1, 256u * 16u)), dim3(BLOCK), 0, stream, pieces, (u32)n_pieces, plan.path_idx.as<u64>(),
                       plan.piece_off.as<u64>(), plan.path_contig.as<u64>(), plan.contig_first_path.as<u64>(), plan.text_bytes, text);
    KCHECK_HIP(hipGetLastError());
    return KATOME_OK;
}

}  // namespace katome

extern "C" {

int katome_dev_gfa_paths_arrays(int device, uint64_t n_edges, const uint64_t* d_edge_src, const uint64_t* d_edge_dst, const uint32_t* d_pieces, uint64_t n_pieces,
                                uint64_t* d_path_line_off, uint64_t* d_path_contig, uint64_t* d_path_first_piece, uint64_t path_cap, uint8_t* d_text,
                                uint64_t text_cap, uint64_t* counts, void* stream_) {
    if (!counts) { set_error("null argument"); return KATOME_E_ARG; }
    counts[0] = counts[1] = counts[2] = 0;
    KCHECK(use_device(device));
    hipStream_t stream = (hipStream_t)stream_;
    GfaPathsPlan plan;
    KCHECK(dev_gfa_paths_plan(n_edges, d_edge_src, d_edge_dst, d_pieces, n_pieces, plan, stream));
    counts[0] = plan.n_paths; counts[1] = plan.n_paths - plan.n_contigs; counts[2] = plan.text_bytes;
    if (!d_text) return KATOME_OK;
    if (!d_path_line_off || !d_path_first_piece || (plan.n_paths && !d_path_contig) || path_cap < plan.n_paths ||
        !text_fits(plan.text_bytes, text_cap, d_text)) {
        set_error("gfa_paths: %llu paths and %llu bytes (rounded up to 16, 16-byte aligned) do not fit the caller's arrays", (unsigned long long)plan.n_paths,
                  (unsigned long long)plan.text_bytes);
        return KATOME_E_ARG;
    }
    // KATOME_GFA_PATHS_TRACE=1: the writer's own time on stderr (there is no builder whose profile could hold it; tools/bench_gfa_paths.py)
    ArraysTrace trace("KATOME_GFA_PATHS_TRACE", "katome_dev_gfa_paths_arrays");
    {
        PhaseScope ps(trace.prof, PH_GFA_PATHS, stream);
        KCHECK(dev_gfa_paths_write(d_pieces, n_pieces, plan, d_text, stream));
    }
    KCHECK_HIP(hipMemcpyAsync(d_path_line_off, plan.path_line_off.p, (plan.n_paths + 1) * 8, hipMemcpyDeviceToDevice, stream));
    KCHECK_HIP(hipMemcpyAsync(d_path_first_piece, plan.path_first_piece.p, (plan.n_paths + 1) * 8, hipMemcpyDeviceToDevice, stream));
    if (plan.n_paths) KCHECK_HIP(hipMemcpyAsync(d_path_contig, plan.path_contig.p, plan.n_paths * 8, hipMemcpyDeviceToDevice, stream));
    KCHECK_HIP(hipStreamSynchronize(stream));
    trace.print(K_GFA_PATHS_WRITE, K_GFA_PATHS_WRITE, plan.text_bytes, n_pieces, "pieces", plan.n_paths, "paths");
    return KATOME_OK;
}

// the whole text for the builder's last katome_dev_collapse: the GFA of the shrunk graph its pieces name (gfa.hip), then the paths
int katome_dev_collapse_gfa(katome_builder* b, katome_dev_gfa_paths* out, void* stream_) {
    if (!b || !out) { set_error("null argument"); return KATOME_E_ARG; }
    hipStream_t stream = (hipStream_t)stream_;
    KCHECK_HIP(hipSetDevice(b->s.device));
    memset(out, 0, sizeof *out);
    if (!b->collapse_valid) { set_error("collapse_gfa: no collapse result"); return KATOME_E_ARG; }
    const ShrinkOutput& sh = b->collapse_shrunk;
    const GfaGraph g = gfa_graph_of(b->s.k, sh);
    GfaPathsOutput& o = b->gfa_paths;
    o.n_segments = o.n_links = o.text_bytes = o.n_paths = o.n_jumps = o.path_bytes = 0;
    {
        PhaseScope ps(b->prof, PH_GFA_PATHS, stream);
        GfaPlan plan;
        GfaPathsPlan paths;
        KCHECK(dev_gfa_plan(g, plan, stream));
        KCHECK(dev_gfa_paths_plan(sh.n_edges, g.edge_src, g.edge_dst, b->collapse_pieces.as<u32>(), b->collapse_n_pieces, paths, stream));
        const u64 path_at = (plan.text_bytes + 15) / 16 * 16;
        KCHECK(o.text.alloc(path_at + (paths.text_bytes + 15) / 16 * 16 + 16, stream));
        KCHECK(dev_gfa_write(g, plan, o.text.as<uint8_t>(), stream));
        KCHECK(dev_gfa_paths_write(b->collapse_pieces.as<u32>(), b->collapse_n_pieces, paths, o.text.as<uint8_t>() + path_at, stream));
        KCHECK_HIP(hipStreamSynchronize(stream));
        o.segment_off.stream = o.link_first.stream = o.path_line_off.stream = o.path_contig.stream = o.path_first_piece.stream = stream;
        o.segment_off.adopt(plan.segment_off); o.link_first.adopt(plan.link_first);
        o.path_line_off.adopt(paths.path_line_off); o.path_contig.adopt(paths.path_contig); o.path_first_piece.adopt(paths.path_first_piece);
        o.n_segments = sh.n_edges; o.n_links = plan.n_links; o.text_bytes = plan.text_bytes;
        o.n_paths = paths.n_paths; o.n_jumps = paths.n_paths - paths.n_contigs; o.path_bytes = paths.text_bytes;
    }
    out->n_segments = o.n_segments; out->n_links = o.n_links; out->text_bytes = o.text_bytes;
    out->d_text = o.text.as<uint8_t>(); out->d_segment_off = o.segment_off.as<u64>(); out->d_link_first = o.link_first.as<u64>();
    out->n_paths = o.n_paths; out->n_jumps = o.n_jumps; out->path_bytes = o.path_bytes;
    out->d_path_text = o.text.as<uint8_t>() + (o.text_bytes + 15) / 16 * 16;
    out->d_path_line_off = o.path_line_off.as<u64>(); out->d_path_contig = o.path_contig.as<u64>(); out->d_path_first_piece = o.path_first_piece.as<u64>();
    return KATOME_OK;
}

}  // extern "C"
