// gfa.hip -- the unitig graph (a shrink result: n_edges merged edges over n_nodes vertices) as GFA 1, written on the device.  The
// format is fixed byte for byte in include/katome_gpu.h:
//   H\tVN:Z:1.0\n
//   S\t<i>\t<bases of edge i>\tLN:i:<bases>\tKC:i:<weight_i * kmers_i>\tew:i:<weight_i>\n      segment i = merged edge i
//   L\t<a>\t+\t<b>\t+\t<k-1>M\n                                                                every (a, b) with edge_dst[a] == edge_src[b]
// KC is what the SHRUNK edge carries: shrink keeps only the weight of a path's first k-mer (shrinker.rs:181,200), so KC is that weight
// times the k-mers merged into the edge (a 64-bit product, up to 20 digits), not the sum of the path's k-mer counts; ew is the weight.
//   The join: the edge indices are sorted by source (dev_sort on edge_src, only the key bits n_nodes needs, the index as the value;
//   the sort is stable, so the indices ascend inside a vertex), the heads and tails of the sorted runs give every vertex its range,
//   the link count of segment a is the out-degree of edge_dst[a], and a scan gives every segment its first link.  Links then come
//   out ordered by a, then b.  The input's edge_src need not be ordered (the exact shrink's is not).
//   The sizes: a line's bytes are counted once (an S line's bases from its label alone, as collapse.hip's piece_measure_kernel does,
//   plus the digits of its numbers; an L line's from the digits of a, b and k - 1) and scanned into 64-bit offsets: line 0 is the
//   header, line 1 + i segment i, line 1 + n_edges + l link l.
//   What this file shares with gfa_strands.hip lies in two headers.  gfa_lines.h has the line rules: an S and an L line's bytes,
//   check_segment, the search for a link's segment, and how a line's name, tags and numbers are formatted.  gfa_image.h has the tile
//   scheme and write_line_tile, a whole tile, which takes a line description: which lines are segments, how line r's bytes
//   that are not bases are formatted, and line r's bases.  gfa_write_kernel is the loop over the tiles round it, with one of two descriptions:
//     TextLines (gfa_write_kernel<false, .>): the one-GPU text of dev_gfa_plan / dev_gfa_write;
//     PartLines (gfa_write_kernel<true, .>, dev_gfa_part_plan / dev_gfa_part_write, katome_dev_gfa_part_arrays): one PART of a text
//     whose other parts are written elsewhere (dist_gfa.hip): names start at first_segment, links come as a table of 64-bit global
//     numbers, the header is written or not, and the S part and the L part are two regions of one buffer, each a launch of its own.
//   The coverage form (COV, the second template parameter; katome_dev_contigs_gfa_coverage, katome_dev_gfa_coverage_arrays,
//   GfaGraph::cov / GfaPart::cov): KC is the sum of the path's k-mer counts and "\tmn:i:<min>\tmx:i:<max>" follows ew.  Both
//   parameters are compile-time: an instantiation carries no branch of another's.  gfa_strands.hip has no coverage form.
//   Every segment is one strand here and every orientation +; gfa_strands.hip folds strand twins into one segment with +/- links, on
//   top of this file's join (dev_gfa_plan) and a line description of its own.
//   The entry points' common checks (gfa_graph_of, is_last_shrink, check_label_alignment, text_fits, ArraysTrace) are builder.h's.
#include "builder.h"
#include "gfa_lines.h"

namespace katome {
namespace {

static_assert(S_TAGS_MAX + COV_TAGS_MAX < (int)TILE, "a segment's tags fit a tile");

// Segment i's line: checks everything the later kernels read through (the two vertices and check_segment's), counts the line's bytes,
// and sets up the sort of the edge indices by source
template <bool COV>
__global__ __launch_bounds__(BLOCK) void gfa_measure_kernel(u32 k, u64 N, u64 E, const u64* __restrict__ src, const u64* __restrict__ dst,
                                                            const u32* __restrict__ weight, const u32* __restrict__ kmers,
                                                            const u64* __restrict__ label_off, const uint8_t* __restrict__ label, u64 label_bytes,
                                                            u32* __restrict__ size, u64* __restrict__ key, u32* __restrict__ order, u32* __restrict__ err,
                                                            const GfaCoverage cov) {
    if (blockIdx.x == 0 && threadIdx.x == 0) size[0] = HEADER_BYTES;
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < E; i += (u64)gridDim.x * BLOCK) {
        size[1 + i] = 0; key[i] = 0; order[i] = (u32)i;
        const u64 s = src[i];
        if (s >= N || dst[i] >= N) { atomicOr(err, (u32)ERR_NODE); continue; }
        u32 bases = 0;
        const u32 bad = check_segment<COV>(k, i, weight, kmers, label_off, label, label_bytes, cov, &bases);
        if (bad) { atomicOr(err, bad); continue; }
        key[i] = s;
        size[1 + i] = checked_segment_bytes<COV>(i, i, bases, weight, kmers, cov);
    }
}

// the ranges of the vertices in the edge indices sorted by source: a run's head writes where it starts, its tail where it ends (both
// zeroed before: a vertex without out-edges keeps an empty range)
__global__ __launch_bounds__(BLOCK) void gfa_vertex_range_kernel(const u64* __restrict__ key, u64 E, u32* __restrict__ first, u32* __restrict__ last) {
    for (u64 j = (u64)blockIdx.x * BLOCK + threadIdx.x; j < E; j += (u64)gridDim.x * BLOCK) {
        const u64 v = key[j];
        if (j == 0 || key[j - 1] != v) first[v] = (u32)j;
        if (j + 1 == E || key[j + 1] != v) last[v] = (u32)(j + 1);
    }
}
// links of segment a: the out-degree of the vertex it ends in
__global__ __launch_bounds__(BLOCK) void gfa_link_count_kernel(const u64* __restrict__ dst, u64 E, const u32* __restrict__ first, const u32* __restrict__ last,
                                                               u32* __restrict__ count) {
    for (u64 a = (u64)blockIdx.x * BLOCK + threadIdx.x; a < E; a += (u64)gridDim.x * BLOCK) { const u64 v = dst[a]; count[a] = last[v] - first[v]; }
}
// link l: its b is the (l - first link)-th edge out of its segment a's target; its line's bytes go behind the header's and the segments'
__global__ __launch_bounds__(BLOCK) void gfa_link_fill_kernel(u32 E, u64 L, u32 k1_digits, const u64* __restrict__ dst, const u32* __restrict__ first,
                                                              const u32* __restrict__ order, const u64* __restrict__ link_first, u32* __restrict__ link_ab,
                                                              u32* __restrict__ size) {
    for (u64 l = (u64)blockIdx.x * BLOCK + threadIdx.x; l < L; l += (u64)gridDim.x * BLOCK) {
        const u32 a = last_segment_with_first_link_le(link_first, E, l), b = order[first[dst[a]] + (u32)(l - link_first[a])];
        link_ab[2 * l] = a; link_ab[2 * l + 1] = b;
        size[l] = link_line_bytes(a, b, k1_digits);
    }
}
// segment i's first base, its line being line hdr + i and its name first + i
__global__ __launch_bounds__(BLOCK) void gfa_segment_off_kernel(u64 E, u64 first, u32 hdr, const u64* __restrict__ line_off, u64* __restrict__ segment_off) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < E; i += (u64)gridDim.x * BLOCK) segment_off[i] = segment_first_base(line_off[hdr + i], first + i);
}

// A numbered part of a text whose other parts are written elsewhere (dist_gfa.hip): segment i is named first + i, link l joins
// first + link_a[l] to link_b[l] (a global number), and the header line is there or not (hdr = 1 or 0): the part's lines are hdr
// header lines, E segments, then links.
// (An S part is launched with hdr header lines and E segments, R = hdr + E; an L part with E = 0, hdr = 0 and R links.)
struct PartNumbers { u64 first; u32 hdr; const u32* link_a; const u64* link_b; };

// ---- the line descriptions (write_line_tile of gfa_image.h) ---------------------------------------------------------------------
// what both have: the arrays behind an S line, and the S line of edge i under `name`
struct SegmentArrays {
    u32 k; const u32 *weight, *kmers; const u64 *label_off; const uint8_t* label; const u64* segment_off; GfaCoverage cov;
    template <bool COV, int NAME_ROOM, class N>
    __device__ __forceinline__ void format_segment(uint8_t* img, u32 i, N name, u64 o, int64_t rel, int64_t end, int len) const {
        put_segment_name<NAME_ROOM>(img, rel, len, (int)(segment_off[i] - o), name);
        if (end - (S_TAGS_MAX + (COV ? COV_TAGS_MAX : 0)) < len) {
            const u32 w = weight[i], km = kmers[i];
            put_segment_tags(img, end, len, km + k - 1, segment_kc<COV>(cov, i, w, km), w, [&](int p) { return put_coverage_tags<COV>(img, p, len, cov, i); });
        }
    }
    // (line r; the segments are the E lines from line `first` on)
    __device__ __forceinline__ Line line(u32 r, u32 first, u32 E, const u64* __restrict__ line_off) const {
        Line ln = line_without_bases(line_off, r, label);
        if (r >= first && r < first + E) { const u32 i = r - first; add_bases(ln, label, label_off, i, (u32)(segment_off[i] - line_off[r])); }
        return ln;
    }
};
// the one-GPU text: line 0 is the header, line 1 + i segment i, line 1 + E + l link l = (link_ab[2 l], link_ab[2 l + 1]), every orientation +
template <bool COV> struct TextLines {
    SegmentArrays s; u32 E; const u32* link_ab;
    __device__ __forceinline__ bool before_links(u32 r) const { return r <= E; }
    __device__ __forceinline__ void format(uint8_t* img, u32 r, u64 o, int64_t rel, int64_t end, int len) const {
        if (r == 0) put_header_line(img, rel, end, len);
        else if (r > E) put_link_line(img, end, len, link_ab[2 * (r - 1 - E)], '+', link_ab[2 * (r - 1 - E) + 1], '+', s.k - 1);
        else s.format_segment<COV, S_NAME_MAX>(img, r - 1, r - 1, o, rel, end, len);
    }
    __device__ __forceinline__ Line line(u32 r, const u64* __restrict__ line_off) const { return s.line(r, 1, E, line_off); }
};
// the numbered part: pn.hdr header lines, then E segments named pn.first + i, then the links (pn.first + pn.link_a[l], pn.link_b[l])
template <bool COV> struct PartLines {
    SegmentArrays s; u32 E; PartNumbers pn;
    __device__ __forceinline__ bool before_links(u32 r) const { return r < pn.hdr + E; }
    __device__ __forceinline__ void format(uint8_t* img, u32 r, u64 o, int64_t rel, int64_t end, int len) const {
        if (r < pn.hdr) put_header_line(img, rel, end, len);
        else if (r >= pn.hdr + E) put_link_line(img, end, len, pn.first + pn.link_a[r - pn.hdr - E], '+', pn.link_b[r - pn.hdr - E], '+', s.k - 1);
        else s.format_segment<COV, S_NAME_MAX_NUMBERED>(img, r - pn.hdr, pn.first + (r - pn.hdr), o, rel, end, len);
    }
    __device__ __forceinline__ Line line(u32 r, const u64* __restrict__ line_off) const { return s.line(r, pn.hdr, E, line_off); }
};

// NUMBERED and COV stay compile-time: an instantiation carries no branch and no argument's read that its text does not need
template <bool NUMBERED, bool COV>
__global__ __launch_bounds__(BLOCK) void gfa_write_kernel(u32 k, u32 E, u32 R, const u32* __restrict__ weight, const u32* __restrict__ kmers,
                                                          const u64* __restrict__ label_off, const uint8_t* __restrict__ label,
                                                          const u64* __restrict__ line_off, const u64* __restrict__ segment_off,
                                                          const u32* __restrict__ link_ab, u64 total, uint8_t* __restrict__ text, const PartNumbers pn,
                                                          const GfaCoverage cov) {
    const SegmentArrays s{k, weight, kmers, label_off, label, segment_off, cov};
    for (u64 base = (u64)blockIdx.x * TILE; base < total; base += (u64)gridDim.x * TILE) {
        const int len = tile_len(base, total);
        const u32 r_lo = workgroup_search(line_off, R, base), r_hi = workgroup_search(line_off, R, base + len - 1);
        if constexpr (NUMBERED) write_line_tile(PartLines<COV>{s, E, pn}, R, r_lo, r_hi, base, len, line_off, total, text);
        else write_line_tile(TextLines<COV>{s, E, link_ab}, R, r_lo, r_hi, base, len, line_off, total, text);
    }
}

// ---- a numbered part: the same sizes, counted with the digits of the GLOBAL numbers --------------------------------------------
// segment i of a part (named first + i): check_segment's, that its links' range ascends (link_first[0] = 0), its line's bytes
template <bool COV>
__global__ __launch_bounds__(BLOCK) void gfa_part_measure_kernel(u32 k, u64 E, u64 first, u32 hdr, const u32* __restrict__ weight, const u32* __restrict__ kmers,
                                                                 const u64* __restrict__ label_off, const uint8_t* __restrict__ label, u64 label_bytes,
                                                                 const u64* __restrict__ link_first, u32* __restrict__ size, u32* __restrict__ err,
                                                                 const GfaCoverage cov) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (hdr) size[0] = HEADER_BYTES;
        if (link_first[0] != 0) atomicOr(err, (u32)ERR_LINKS);
    }
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < E; i += (u64)gridDim.x * BLOCK) {
        size[hdr + i] = 0;
        if (link_first[i] > link_first[i + 1]) atomicOr(err, (u32)ERR_LINKS);
        u32 bases = 0;
        const u32 bad = check_segment<COV>(k, i, weight, kmers, label_off, label, label_bytes, cov, &bases);
        if (bad) { atomicOr(err, bad); continue; }
        size[hdr + i] = checked_segment_bytes<COV>(first + i, i, bases, weight, kmers, cov);
    }
}
// link l of a part: its segment and its line's bytes
__global__ __launch_bounds__(BLOCK) void gfa_part_link_kernel(u32 E, u64 L, u64 first, u32 k1_digits, const u64* __restrict__ link_first,
                                                              const u64* __restrict__ link_b, u32* __restrict__ link_a, u32* __restrict__ size) {
    for (u64 l = (u64)blockIdx.x * BLOCK + threadIdx.x; l < L; l += (u64)gridDim.x * BLOCK) {
        const u32 a = last_segment_with_first_link_le(link_first, E, l);
        link_a[l] = a;
        size[l] = link_line_bytes(first + a, link_b[l], k1_digits);
    }
}

int check_gfa_errors(u32 err) {
    if (err & ERR_LINKS) { set_error("gfa: d_link_first does not ascend from 0"); return KATOME_E_ARG; }
    if (err & ERR_NODE) { set_error("gfa: an edge's source or target is not below n_nodes"); return KATOME_E_ARG; }
    if (err & ERR_LABEL) { set_error("gfa: a label's offsets, pad byte or length (shorter than k bases) are malformed"); return KATOME_E_ARG; }
    if (err & ERR_LABEL_LEN) { set_error("gfa: a label of more than 2^31 bases"); return KATOME_E_UNSUPPORTED; }
    if (err & ERR_KMERS) { set_error("gfa: a label's bases are not edge_kmers + k - 1"); return KATOME_E_ARG; }
    if (err & ERR_COVERAGE) { set_error("gfa: a segment's coverage does not fit its weight and k-mer count"); return KATOME_E_ARG; }
    return KATOME_OK;
}

}  // namespace

// dev_gfa_plan's checks without its join: the measuring kernel into scratch of its own (16 bytes per segment), and its verdict
int dev_gfa_validate(const GfaGraph& g, hipStream_t stream) {
    const u64 E = g.n_edges;
    if (E >= (1ull << 32)) { set_error("gfa: %llu segments, at most 2^32 - 1", (unsigned long long)E); return KATOME_E_UNSUPPORTED; }
    if (E && (!g.edge_src || !g.edge_dst || !g.edge_weight || !g.edge_kmers || !g.label_off || !g.label)) { set_error("null argument"); return KATOME_E_ARG; }
    if (g.cov.any() && E && !g.cov.all()) { set_error("null argument"); return KATOME_E_ARG; }
    DevBuf key(stream), order(stream), seg_size(stream), tail(stream);
    KCHECK(key.alloc(E * 8 + 16)); KCHECK(order.alloc(E * 4 + 16)); KCHECK(seg_size.alloc((E + 1) * 4)); KCHECK(tail.alloc(16));
    KCHECK_HIP(hipMemsetAsync(tail.p, 0, 16, stream));
    hipLaunchKernelGGL(g.cov.any() ? gfa_measure_kernel<true> : gfa_measure_kernel<false>, dim3(grid_for(E, BLOCK, 256u * 32u)), dim3(BLOCK), 0, stream, g.k, g.n_nodes, E,
                       g.edge_src, g.edge_dst, g.edge_weight, g.edge_kmers, g.label_off, g.label, g.label_bytes, seg_size.as<u32>(), key.as<u64>(), order.as<u32>(),
                       tail.as<u32>(), g.cov);
    KCHECK_HIP(hipGetLastError());
    u32 err = 0;
    KCHECK_HIP(hipMemcpyAsync(&err, tail.p, 4, hipMemcpyDeviceToHost, stream));
    KCHECK_HIP(hipStreamSynchronize(stream));
    return check_gfa_errors(err);
}

int dev_gfa_plan(const GfaGraph& g, GfaPlan& plan, hipStream_t stream) {
    plan.n_links = plan.text_bytes = 0;
    const u64 E = g.n_edges, N = g.n_nodes;
    if (E >= (1ull << 32)) { set_error("gfa: %llu segments, at most 2^32 - 1", (unsigned long long)E); return KATOME_E_UNSUPPORTED; }
    if (E && (!g.edge_src || !g.edge_dst || !g.edge_weight || !g.edge_kmers || !g.label_off || !g.label)) { set_error("null argument"); return KATOME_E_ARG; }
    if (g.cov.any() && E && !g.cov.all()) { set_error("null argument"); return KATOME_E_ARG; }
    const dim3 blk(BLOCK), grid(grid_for(E, BLOCK, 256u * 32u));
    plan.line_off.stream = plan.segment_off.stream = plan.link_first.stream = plan.link_ab.stream = stream;
    DevBuf key(stream), order(stream), seg_size(stream), count(stream), range(stream), size(stream), tail(stream);
    KCHECK(key.alloc(E * 8 + 16)); KCHECK(order.alloc(E * 4 + 16)); KCHECK(seg_size.alloc((E + 1) * 4)); KCHECK(tail.alloc(16));
    KCHECK(plan.link_first.alloc((E + 1) * 8)); KCHECK(plan.segment_off.alloc(E * 8 + 16));
    KCHECK_HIP(hipMemsetAsync(tail.p, 0, 16, stream));
    {
        KernelScope ks(K_GFA_SIZES, stream, E);
        hipLaunchKernelGGL(g.cov.any() ? gfa_measure_kernel<true> : gfa_measure_kernel<false>, grid, blk, 0, stream, g.k, N, E, g.edge_src, g.edge_dst, g.edge_weight,
                           g.edge_kmers, g.label_off, g.label, g.label_bytes, seg_size.as<u32>(), key.as<u64>(), order.as<u32>(), tail.as<u32>(), g.cov);
        KCHECK_HIP(hipGetLastError());
    }
    u32 err = 0;
    KCHECK_HIP(hipMemcpyAsync(&err, tail.p, 4, hipMemcpyDeviceToHost, stream));
    KCHECK_HIP(hipStreamSynchronize(stream));
    KCHECK(check_gfa_errors(err));
    u64 L = 0;
    if (E) {
        u32 key_bits = 1;
        while (key_bits < 64 && ((N - 1) >> key_bits) != 0) ++key_bits;
        {
            KernelScope ks(K_GFA_SORT, stream, E);
            KCHECK(dev_sort(key.as<u64>(), order.as<u32>(), E, 1, key_bits, stream));
        }
        KCHECK(range.alloc(N * 8)); KCHECK(count.alloc(E * 4));
        KCHECK_HIP(hipMemsetAsync(range.p, 0, N * 8, stream));
        KernelScope ks(K_GFA_SIZES, stream, E);
        u32* first = range.as<u32>();
        u32* last = first + N;
        hipLaunchKernelGGL(gfa_vertex_range_kernel, grid, blk, 0, stream, key.as<u64>(), E, first, last);
        hipLaunchKernelGGL(gfa_link_count_kernel, grid, blk, 0, stream, g.edge_dst, E, first, last, count.as<u32>());
        KCHECK_HIP(hipGetLastError());
        KCHECK(dev_scan_counts(count.as<u32>(), E, plan.link_first.as<u64>(), stream));
        KCHECK_HIP(hipMemcpyAsync(&L, plan.link_first.as<u64>() + E, 8, hipMemcpyDeviceToHost, stream));
        KCHECK_HIP(hipStreamSynchronize(stream));
    } else {
        KCHECK_HIP(hipMemsetAsync(plan.link_first.p, 0, 8, stream));
    }
    if (L >= (1ull << 32)) { set_error("gfa: %llu links, at most 2^32 - 1", (unsigned long long)L); return KATOME_E_UNSUPPORTED; }
    const u64 R = 1 + E + L;
    if (R >= 0xFFFFFFFFull) { set_error("gfa: %llu lines (%llu segments, %llu links), at most 2^32 - 2", (unsigned long long)R, (unsigned long long)E, (unsigned long long)L); return KATOME_E_UNSUPPORTED; }
    key.release(); count.release();
    KCHECK(size.alloc(R * 4)); KCHECK(plan.line_off.alloc((R + 1) * 8)); KCHECK(plan.link_ab.alloc(L * 8 + 16));
    {
        KernelScope ks(K_GFA_SIZES, stream, R);
        KCHECK_HIP(hipMemcpyAsync(size.p, seg_size.p, (E + 1) * 4, hipMemcpyDeviceToDevice, stream));
        if (L) {
            hipLaunchKernelGGL(gfa_link_fill_kernel, dim3(grid_for(L, BLOCK, 256u * 32u)), blk, 0, stream, (u32)E, L, host_digits(g.k - 1), g.edge_dst,
                               range.as<u32>(), order.as<u32>(), plan.link_first.as<u64>(), plan.link_ab.as<u32>(), size.as<u32>() + 1 + E);
            KCHECK_HIP(hipGetLastError());
        }
        KCHECK(dev_scan_counts(size.as<u32>(), R, plan.line_off.as<u64>(), stream));
        hipLaunchKernelGGL(gfa_segment_off_kernel, grid, blk, 0, stream, E, (u64)0, 1u, plan.line_off.as<u64>(), plan.segment_off.as<u64>());
        KCHECK_HIP(hipGetLastError());
    }
    KCHECK_HIP(hipMemcpyAsync(&plan.text_bytes, plan.line_off.as<u64>() + R, 8, hipMemcpyDeviceToHost, stream));
    KCHECK_HIP(hipStreamSynchronize(stream));
    plan.n_links = L;
    return KATOME_OK;
}

int dev_gfa_write(const GfaGraph& g, const GfaPlan& plan, uint8_t* text, hipStream_t stream) {
    const u64 R = 1 + g.n_edges + plan.n_links, tiles = (plan.text_bytes + TILE - 1) / TILE;
    KernelScope ks(K_GFA_WRITE, stream, plan.text_bytes);
    hipLaunchKernelGGL((g.cov.any() ? gfa_write_kernel<false, true> : gfa_write_kernel<false, false>), dim3(grid_for(tiles, 1, 256u * 16u)), dim3(BLOCK), 0, stream, g.k,
                       (u32)g.n_edges, (u32)R, g.edge_weight, g.edge_kmers, g.label_off, g.label, plan.line_off.as<u64>(), plan.segment_off.as<u64>(),
                       plan.link_ab.as<u32>(), plan.text_bytes, text, PartNumbers{0, 1, nullptr, nullptr}, g.cov);
    KCHECK_HIP(hipGetLastError());
    return KATOME_OK;
}

int dev_gfa(const GfaGraph& g, GfaOutput& out, hipStream_t stream) {
    out.n_segments = out.n_links = out.text_bytes = 0;
    GfaPlan plan;
    KCHECK(dev_gfa_plan(g, plan, stream));
    KCHECK(out.text.alloc((plan.text_bytes + 15) / 16 * 16 + 16, stream));
    KCHECK(dev_gfa_write(g, plan, out.text.as<uint8_t>(), stream));
    KCHECK_HIP(hipStreamSynchronize(stream));
    out.segment_off.stream = out.link_first.stream = stream;
    out.segment_off.adopt(plan.segment_off); out.link_first.adopt(plan.link_first);
    out.n_segments = g.n_edges; out.n_links = plan.n_links; out.text_bytes = plan.text_bytes;
    return KATOME_OK;
}

int dev_gfa_part_plan(const GfaPart& g, GfaPartPlan& plan, hipStream_t stream) {
    plan.n_links = plan.s_bytes = plan.l_bytes = 0;
    const u64 E = g.n_edges, first = g.first_segment;
    const u32 hdr = g.with_header ? 1u : 0u;
    if (E >= (1ull << 32)) { set_error("gfa: %llu segments in one part, at most 2^32 - 1", (unsigned long long)E); return KATOME_E_UNSUPPORTED; }
    if (first + E < first) { set_error("gfa: segment numbers from %llu on for %llu segments pass 2^64", (unsigned long long)first, (unsigned long long)E); return KATOME_E_UNSUPPORTED; }
    if (!g.link_first || (E && (!g.edge_weight || !g.edge_kmers || !g.label_off || !g.label))) { set_error("null argument"); return KATOME_E_ARG; }
    if (g.cov.any() && E && !g.cov.all()) { set_error("null argument"); return KATOME_E_ARG; }
    const dim3 blk(BLOCK), grid(grid_for(E, BLOCK, 256u * 32u));
    plan.s_line_off.stream = plan.l_line_off.stream = plan.segment_off.stream = plan.link_a.stream = stream;
    DevBuf size(stream), lsize(stream), tail(stream);
    KCHECK(size.alloc((hdr + E + 1) * 4)); KCHECK(tail.alloc(16)); KCHECK(plan.s_line_off.alloc((hdr + E + 1) * 8)); KCHECK(plan.segment_off.alloc(E * 8 + 16));
    KCHECK_HIP(hipMemsetAsync(tail.p, 0, 16, stream));
    {
        KernelScope ks(K_GFA_SIZES, stream, E);
        hipLaunchKernelGGL(g.cov.any() ? gfa_part_measure_kernel<true> : gfa_part_measure_kernel<false>, grid, blk, 0, stream, g.k, E, first, hdr, g.edge_weight,
                           g.edge_kmers, g.label_off, g.label, g.label_bytes, g.link_first, size.as<u32>(), tail.as<u32>(), g.cov);
        KCHECK_HIP(hipGetLastError());
    }
    u32 err = 0;
    u64 L = 0;
    KCHECK_HIP(hipMemcpyAsync(&err, tail.p, 4, hipMemcpyDeviceToHost, stream));
    KCHECK_HIP(hipMemcpyAsync(&L, g.link_first + E, 8, hipMemcpyDeviceToHost, stream));      // (the largest entry once the range is known to ascend)
    KCHECK_HIP(hipStreamSynchronize(stream));
    KCHECK(check_gfa_errors(err));
    if (L && !g.link_b) { set_error("null argument"); return KATOME_E_ARG; }
    const u64 R = hdr + E + L;
    if (L >= (1ull << 32) || R >= 0xFFFFFFFEull) {
        set_error("gfa: %llu lines in one part (%llu segments, %llu links), fewer than 2^32 - 2", (unsigned long long)R, (unsigned long long)E, (unsigned long long)L);
        return KATOME_E_UNSUPPORTED;
    }
    KernelScope ks(K_GFA_SIZES, stream, R);
    if (hdr + E) {
        KCHECK(dev_scan_counts(size.as<u32>(), hdr + E, plan.s_line_off.as<u64>(), stream));
        hipLaunchKernelGGL(gfa_segment_off_kernel, grid, blk, 0, stream, E, first, hdr, plan.s_line_off.as<u64>(), plan.segment_off.as<u64>());
        KCHECK_HIP(hipGetLastError());
        KCHECK_HIP(hipMemcpyAsync(&plan.s_bytes, plan.s_line_off.as<u64>() + hdr + E, 8, hipMemcpyDeviceToHost, stream));
    }
    if (L) {
        KCHECK(lsize.alloc(L * 4)); KCHECK(plan.link_a.alloc(L * 4)); KCHECK(plan.l_line_off.alloc((L + 1) * 8));
        hipLaunchKernelGGL(gfa_part_link_kernel, dim3(grid_for(L, BLOCK, 256u * 32u)), blk, 0, stream, (u32)E, L, first, host_digits(g.k - 1), g.link_first, g.link_b,
                           plan.link_a.as<u32>(), lsize.as<u32>());
        KCHECK_HIP(hipGetLastError());
        KCHECK(dev_scan_counts(lsize.as<u32>(), L, plan.l_line_off.as<u64>(), stream));
        KCHECK_HIP(hipMemcpyAsync(&plan.l_bytes, plan.l_line_off.as<u64>() + L, 8, hipMemcpyDeviceToHost, stream));
    }
    KCHECK_HIP(hipStreamSynchronize(stream));
    plan.n_links = L;
    return KATOME_OK;
}

// two launches of the numbered kernel: the S part's lines, then the L part's, each a text of its own that starts on a multiple of 16
int dev_gfa_part_write(const GfaPart& g, const GfaPartPlan& plan, uint8_t* text, hipStream_t stream) {
    const u32 hdr = g.with_header ? 1u : 0u, E = (u32)g.n_edges;
    KernelScope ks(K_GFA_WRITE, stream, plan.s_bytes + plan.l_bytes);
    if (plan.s_bytes) {
        const PartNumbers pn{g.first_segment, hdr, nullptr, nullptr};
        hipLaunchKernelGGL((g.cov.any() ? gfa_write_kernel<true, true> : gfa_write_kernel<true, false>), dim3(grid_for((plan.s_bytes + TILE - 1) / TILE, 1, 256u * 16u)),
                           dim3(BLOCK), 0, stream, g.k, E, hdr + E, g.edge_weight, g.edge_kmers, g.label_off, g.label, plan.s_line_off.as<u64>(),
                           plan.segment_off.as<u64>(), nullptr, plan.s_bytes, text, pn, g.cov);
    }
    if (plan.l_bytes) {
        const PartNumbers pn{g.first_segment, 0u, plan.link_a.as<u32>(), g.link_b};
        hipLaunchKernelGGL((gfa_write_kernel<true, false>), dim3(grid_for((plan.l_bytes + TILE - 1) / TILE, 1, 256u * 16u)), dim3(BLOCK), 0, stream, g.k, 0u, (u32)plan.n_links,
                           g.edge_weight, g.edge_kmers, g.label_off, g.label, plan.l_line_off.as<u64>(), plan.segment_off.as<u64>(), nullptr, plan.l_bytes,
                           text + plan.l_offset(), pn, GfaCoverage{});      // (an L part has no segments)
    }
    KCHECK_HIP(hipGetLastError());
    return KATOME_OK;
}

}  // namespace katome

extern "C" {

int katome_dev_gfa_part_arrays(int device, uint32_t k, uint64_t n_edges, const uint32_t* d_edge_weight, const uint32_t* d_edge_kmers,
                               const uint64_t* d_edge_label_off, const uint8_t* d_edge_label, uint64_t label_bytes, uint64_t first_segment, int with_header,
                               const uint64_t* d_link_first, const uint64_t* d_link_b, uint64_t* d_segment_off, uint8_t* d_text, uint64_t text_cap,
                               uint64_t* s_bytes, uint64_t* l_offset, uint64_t* l_bytes, void* stream_) {
    KCHECK(use_device(device));
    KCHECK(check_k(k));
    if (!s_bytes || !l_offset || !l_bytes) { set_error("null argument"); return KATOME_E_ARG; }
    *s_bytes = *l_offset = *l_bytes = 0;
    hipStream_t stream = (hipStream_t)stream_;
    KCHECK(check_label_alignment(d_edge_label));
    const GfaPart g{k, n_edges, d_edge_weight, d_edge_kmers, d_edge_label_off, d_edge_label, label_bytes, first_segment, with_header != 0, d_link_first, d_link_b};
    GfaPartPlan plan;
    KCHECK(dev_gfa_part_plan(g, plan, stream));
    *s_bytes = plan.s_bytes; *l_offset = plan.l_offset(); *l_bytes = plan.l_bytes;
    if (!d_text) return KATOME_OK;
    if ((n_edges && !d_segment_off) || !text_fits(plan.buffer_bytes(), text_cap, d_text)) {
        set_error("gfa: %llu + %llu bytes (each rounded up to 16, 16-byte aligned) do not fit the caller's arrays", (unsigned long long)plan.s_bytes,
                  (unsigned long long)plan.l_bytes);
        return KATOME_E_ARG;
    }
    KCHECK(dev_gfa_part_write(g, plan, d_text, stream));
    if (n_edges) KCHECK_HIP(hipMemcpyAsync(d_segment_off, plan.segment_off.p, n_edges * 8, hipMemcpyDeviceToDevice, stream));
    KCHECK_HIP(hipStreamSynchronize(stream));
    return KATOME_OK;
}


// katome_dev_contigs_gfa and its coverage form: one result, b->gfa, whichever wrote it last
static int builder_contigs_gfa(katome_builder* b, const katome_dev_contigs* c, katome_dev_gfa* out, bool coverage, void* stream_) {
    if (!b || !c || !out) { set_error("null argument"); return KATOME_E_ARG; }
    hipStream_t stream = (hipStream_t)stream_;
    KCHECK_HIP(hipSetDevice(b->s.device));
    if (!is_last_shrink(b, c)) { set_error("contigs_gfa: not the result of this builder's last katome_dev_shrink"); return KATOME_E_ARG; }
    if (coverage && (!b->shrunk_cov.valid || b->shrunk_cov.n_edges != b->shrunk.n_edges)) {
        set_error("contigs_gfa_coverage: this builder's last shrink was not a katome_dev_shrink_coverage");
        return KATOME_E_ARG;
    }
    memset(out, 0, sizeof *out);
    GfaGraph g = gfa_graph_of(b->s.k, b->shrunk);
    if (coverage) g.cov = GfaCoverage{b->shrunk_cov.kmer_sum.as<u64>(), b->shrunk_cov.kmer_min.as<u32>(), b->shrunk_cov.kmer_max.as<u32>()};
    {
        PhaseScope ps(b->prof, PH_GFA, stream);
        KCHECK(dev_gfa(g, b->gfa, stream));
    }
    out->n_segments = b->gfa.n_segments; out->n_links = b->gfa.n_links; out->text_bytes = b->gfa.text_bytes;
    out->d_text = b->gfa.text.as<uint8_t>(); out->d_segment_off = b->gfa.segment_off.as<u64>(); out->d_link_first = b->gfa.link_first.as<u64>();
    return KATOME_OK;
}

int katome_dev_contigs_gfa(katome_builder* b, const katome_dev_contigs* c, katome_dev_gfa* out, void* stream_) {
    return builder_contigs_gfa(b, c, out, false, stream_);
}
int katome_dev_contigs_gfa_coverage(katome_builder* b, const katome_dev_contigs* c, katome_dev_gfa* out, void* stream_) {
    return builder_contigs_gfa(b, c, out, true, stream_);
}

// katome_dev_gfa_arrays and its coverage form (cov: all three arrays, or none)
static int gfa_arrays(int device, uint32_t k, uint64_t n_nodes, uint64_t n_edges, const uint64_t* d_edge_src, const uint64_t* d_edge_dst,
                      const uint32_t* d_edge_weight, const uint32_t* d_edge_kmers, const GfaCoverage& cov, const uint64_t* d_edge_label_off,
                      const uint8_t* d_edge_label, uint64_t label_bytes, uint64_t* d_segment_off, uint64_t* d_link_first, uint8_t* d_text, uint64_t text_cap,
                      uint64_t* n_links, uint64_t* text_bytes, void* stream_) {
    KCHECK(use_device(device));
    KCHECK(check_k(k));
    if (!n_links || !text_bytes) { set_error("null argument"); return KATOME_E_ARG; }
    *n_links = *text_bytes = 0;
    hipStream_t stream = (hipStream_t)stream_;
    KCHECK(check_label_alignment(d_edge_label));
    const GfaGraph g{k, n_nodes, n_edges, d_edge_src, d_edge_dst, d_edge_weight, d_edge_kmers, d_edge_label_off, d_edge_label, label_bytes, cov};
    GfaPlan plan;
    KCHECK(dev_gfa_plan(g, plan, stream));
    *n_links = plan.n_links; *text_bytes = plan.text_bytes;
    if (!d_text) return KATOME_OK;
    if (!d_segment_off || !d_link_first || !text_fits(plan.text_bytes, text_cap, d_text)) {
        set_error("gfa: %llu bytes (rounded up to 16, 16-byte aligned) do not fit the caller's arrays", (unsigned long long)plan.text_bytes);
        return KATOME_E_ARG;
    }
    // KATOME_GFA_TRACE=1: the writer's own time on stderr (there is no builder whose profile could hold it; tools/bench_gfa.py times
    // the S region alone through this entry, on a graph without links)
    ArraysTrace trace("KATOME_GFA_TRACE", "katome_dev_gfa_arrays");
    {
        PhaseScope ps(trace.prof, PH_GFA, stream);
        KCHECK(dev_gfa_write(g, plan, d_text, stream));
    }
    if (n_edges) KCHECK_HIP(hipMemcpyAsync(d_segment_off, plan.segment_off.p, n_edges * 8, hipMemcpyDeviceToDevice, stream));
    KCHECK_HIP(hipMemcpyAsync(d_link_first, plan.link_first.p, (n_edges + 1) * 8, hipMemcpyDeviceToDevice, stream));
    KCHECK_HIP(hipStreamSynchronize(stream));
    trace.print(K_GFA_WRITE, K_GFA_WRITE, plan.text_bytes, n_edges, "segments", plan.n_links, "links");
    return KATOME_OK;
}

int katome_dev_gfa_arrays(int device, uint32_t k, uint64_t n_nodes, uint64_t n_edges, const uint64_t* d_edge_src, const uint64_t* d_edge_dst,
                          const uint32_t* d_edge_weight, const uint32_t* d_edge_kmers, const uint64_t* d_edge_label_off, const uint8_t* d_edge_label,
                          uint64_t label_bytes, uint64_t* d_segment_off, uint64_t* d_link_first, uint8_t* d_text, uint64_t text_cap, uint64_t* n_links,
                          uint64_t* text_bytes, void* stream_) {
    return gfa_arrays(device, k, n_nodes, n_edges, d_edge_src, d_edge_dst, d_edge_weight, d_edge_kmers, GfaCoverage{}, d_edge_label_off, d_edge_label, label_bytes,
                      d_segment_off, d_link_first, d_text, text_cap, n_links, text_bytes, stream_);
}
int katome_dev_gfa_coverage_arrays(int device, uint32_t k, uint64_t n_nodes, uint64_t n_edges, const uint64_t* d_edge_src, const uint64_t* d_edge_dst,
                                   const uint32_t* d_edge_weight, const uint32_t* d_edge_kmers, const uint64_t* d_kmer_sum, const uint32_t* d_kmer_min,
                                   const uint32_t* d_kmer_max, const uint64_t* d_edge_label_off, const uint8_t* d_edge_label, uint64_t label_bytes,
                                   uint64_t* d_segment_off, uint64_t* d_link_first, uint8_t* d_text, uint64_t text_cap, uint64_t* n_links, uint64_t* text_bytes,
                                   void* stream_) {
    if (n_edges && (!d_kmer_sum || !d_kmer_min || !d_kmer_max)) {
        if (n_links) *n_links = 0;
        if (text_bytes) *text_bytes = 0;
        set_error("null argument");
        return KATOME_E_ARG;
    }
    return gfa_arrays(device, k, n_nodes, n_edges, d_edge_src, d_edge_dst, d_edge_weight, d_edge_kmers, GfaCoverage{d_kmer_sum, d_kmer_min, d_kmer_max},
                      d_edge_label_off, d_edge_label, label_bytes, d_segment_off, d_link_first, d_text, text_cap, n_links, text_bytes, stream_);
}

}  // extern "C"
