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
//   The sizes: a line's bytes are counted once, here (an S line's bases from its label alone, as collapse.hip's piece_measure_kernel
//   does, plus the digits of its five numbers; an L line's from the digits of a, b and k - 1), and scanned into 64-bit offsets: line 0
//   is the header, line 1 + i segment i, line 1 + n_edges + l link l.
//   gfa_write_kernel is partitioned by OUTPUT bytes like text_write_kernel: a workgroup owns TILE bytes, finds the lines that
//   overlap them by the workgroup search and keeps their starts in LDS.  Everything that is not a base -- the header, an S line's
//   name and tags, whole L lines: short records full of decimal numbers -- is formatted ONCE per line, one thread per line, right to
//   left into an LDS image of the tile (a division by ten per digit, not per byte and lane).  Then every lane produces 16 consecutive
//   bytes with one 128-bit store: 16 bases of one segment straight from the 2-bit label (sixteen_bases); in the L region the image's
//   16 bytes as they are; anywhere else the image's bytes with the bases among them filled in one at a time.
//   The numbered form (gfa_write_kernel<true>, dev_gfa_part_plan / dev_gfa_part_write, katome_dev_gfa_part_arrays) writes one PART of
//   a text whose other parts are written elsewhere (dist_gfa.hip): names start at first_segment, links come as a table of 64-bit
//   global numbers, the header is written or not, and the S part and the L part are two regions of one buffer, each a launch of its
//   own.  It is a separate instantiation: gfa_write_kernel<false> is the one-GPU kernel as it was.
//   The coverage form (COV, a second template parameter of the two measure kernels and of the writer's S-tag branch): KC is the sum of
//   the path's k-mer counts and "\tmn:i:<min>\tmx:i:<max>" follows ew (katome_dev_contigs_gfa_coverage, katome_dev_gfa_coverage_arrays,
//   GfaGraph::cov / GfaPart::cov); the variants without it are the kernels as they were.  gfa_strands.hip has no coverage form.
//   Every segment is one strand here and every orientation +; gfa_strands.hip folds strand twins into one segment with +/- links, on
//   top of this file's join (dev_gfa_plan) and the tile image both writers share (gfa_image.h).
#include "builder.h"
#include "gfa_image.h"
#include "text_bases.h"

namespace katome {
namespace {

constexpr int S_NAME_MAX_NUMBERED = 2 + 20 + 1;        // ... of a numbered part: first_segment + i < 2^64
constexpr u32 L_LINE_MAX_NUMBERED = 10 + 20 + 20 + 10; // "L\t<a>\t+\t<b>\t+\t<k-1>M\n" with two 64-bit numbers: far below a tile
constexpr int S_TAGS_MAX = 3 * 6 + 10 + 20 + 10 + 1;   // "\tLN:i:<u32>\tKC:i:<u64>\tew:i:<u32>\n"
constexpr int S_TAGS_MAX_COV = S_TAGS_MAX + 2 * (6 + 10);      // ... with coverage: "\tmn:i:<u32>\tmx:i:<u32>" in front of the line's end
static_assert(S_TAGS_MAX_COV < (int)TILE, "a segment's tags fit a tile");
// (no line of either form is shorter than the header's 11 bytes -- the shortest L line, "L\t0\t+\t0\t+\t0M\n", has 13 --, so MAX_LINES and
// the 16-bit offsets hold for a numbered part too: longer numbers only make lines longer)
static_assert(L_LINE_MAX_NUMBERED < TILE && HEADER_BYTES <= 13, "a tile holds at most MAX_LINES lines");
enum { ERR_NODE = 1, ERR_LABEL = 2, ERR_LABEL_LEN = 4, ERR_KMERS = 8, ERR_LINKS = 16, ERR_COVERAGE = 32 };

// The coverage variant (COV, GfaCoverage of common.h): KC is the sum of the path's k-mer counts and the S line ends in mn / mx.  A
// compile-time variant of the two measure kernels and of the writer's S-tag branch: without it they are the kernels they were.
// a segment's coverage fits its weight and its k-mers: min <= weight <= max and min * kmers <= sum <= max * kmers (64-bit: u32 * u32)
__device__ __forceinline__ bool coverage_fits(const GfaCoverage& c, u64 i, u32 w, u32 km) {
    const u32 mn = c.kmer_min[i], mx = c.kmer_max[i];
    const u64 sum = c.kmer_sum[i];
    return mn <= w && w <= mx && (u64)mn * km <= sum && sum <= (u64)mx * km;
}
// the bytes of "\tKC:i:<sum>\tew:i:<w>\tmn:i:<min>\tmx:i:<max>\n"
__device__ __forceinline__ u32 coverage_tag_bytes(const GfaCoverage& c, u64 i, u32 w) {
    return 6 + decimal_digits(c.kmer_sum[i]) + 6 + decimal_digits(w) + 6 + decimal_digits(c.kmer_min[i]) + 6 + decimal_digits(c.kmer_max[i]) + 1;
}

// Segment i's line: checks everything the later kernels read through (the two vertices, the label's offsets, pad byte and length, and
// that the label spells edge_kmers + k - 1 bases), counts the line's bytes, and sets up the sort of the edge indices by source
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
        const int bad = label_check(label, label_off[i], label_off[i + 1], label_bytes, k, &bases);
        if (bad) { atomicOr(err, (u32)(bad == 2 ? ERR_LABEL_LEN : ERR_LABEL)); continue; }
        if ((u64)bases != (u64)kmers[i] + k - 1) { atomicOr(err, (u32)ERR_KMERS); continue; }
        const u32 w = weight[i];
        if constexpr (COV) {
            if (!coverage_fits(cov, i, w, kmers[i])) { atomicOr(err, (u32)ERR_COVERAGE); continue; }      // (no size from the bad values)
            key[i] = s;
            size[1 + i] = 2 + decimal_digits(i) + 1 + bases + 6 + decimal_digits(bases) + coverage_tag_bytes(cov, i, w);
            continue;
        }
        key[i] = s;
        size[1 + i] = 2 + decimal_digits(i) + 1 + bases + 6 + decimal_digits(bases) + 6 + decimal_digits((u64)w * kmers[i]) + 6 + decimal_digits(w) + 1;
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
// link l: its segment a is the last one whose first link is <= l (segments without links share their successor's first link and are
// passed over), its b the (l - first link)-th edge out of a's target; its line's bytes go behind the header's and the segments'
__global__ __launch_bounds__(BLOCK) void gfa_link_fill_kernel(u32 E, u64 L, u32 k1_digits, const u64* __restrict__ dst, const u32* __restrict__ first,
                                                              const u32* __restrict__ order, const u64* __restrict__ link_first, u32* __restrict__ link_ab,
                                                              u32* __restrict__ size) {
    for (u64 l = (u64)blockIdx.x * BLOCK + threadIdx.x; l < L; l += (u64)gridDim.x * BLOCK) {
        u32 lo = 0, hi = E;
        while (hi - lo > 1) { const u32 mid = lo + ((hi - lo) >> 1); if (link_first[mid] <= l) lo = mid; else hi = mid; }
        const u32 a = lo, b = order[first[dst[a]] + (u32)(l - link_first[a])];
        link_ab[2 * l] = a; link_ab[2 * l + 1] = b;
        size[l] = 10 + decimal_digits(a) + decimal_digits(b) + k1_digits;
    }
}
// segment i's first base: behind "S\t<i>\t"
__global__ __launch_bounds__(BLOCK) void gfa_segment_off_kernel(u64 E, const u64* __restrict__ line_off, u64* __restrict__ segment_off) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < E; i += (u64)gridDim.x * BLOCK) segment_off[i] = line_off[1 + i] + 3 + decimal_digits(i);
}

// (NUMBERED: a part of a sharded text, see PartNumbers below; its segments are lines hdr .. hdr + E - 1)
template <bool NUMBERED>
__device__ __forceinline__ Line load_line(u32 r, u32 E, u32 hdr, const uint8_t* __restrict__ label, const u64* __restrict__ label_off,
                                          const u64* __restrict__ segment_off, const u64* __restrict__ line_off) {
    Line ln;
    const u64 at = line_off[r];
    ln.total = (u32)(line_off[r + 1] - at);
    ln.head = ln.total; ln.bases = 0; ln.src = label;
    if (NUMBERED ? (r >= hdr && r < hdr + E) : (r >= 1 && r <= E)) {
        const u32 i = NUMBERED ? r - hdr : r - 1;
        const u64 lo = label_off[i], hi = label_off[i + 1];
        ln.src = label + lo + 1;
        ln.bases = 4 * (u32)(hi - lo - 1) - label[lo];
        ln.head = (u32)(segment_off[i] - at);       // (the name's digits were counted when the line was measured: none is counted here)
    }
    return ln;
}

// A numbered part of a text whose other parts are written elsewhere (dist_gfa.hip): segment i is named first + i, link l joins
// first + link_a[l] to link_b[l] (a global number), and the header line is there or not (hdr = 1 or 0): the part's lines are hdr
// header lines, E segments, then links.  The one-GPU text is the form without: NUMBERED = false is the kernel as it was, its
// conditions and types untouched, and takes none of these.
// (An S part is launched with hdr header lines and E segments, R = hdr + E; an L part with E = 0, hdr = 0 and R links.)
struct PartNumbers { u64 first; u32 hdr; const u32* link_a; const u64* link_b; };

template <bool NUMBERED, bool COV>
__global__ __launch_bounds__(BLOCK) void gfa_write_kernel(u32 k, u32 E, u32 R, const u32* __restrict__ weight, const u32* __restrict__ kmers,
                                                          const u64* __restrict__ label_off, const uint8_t* __restrict__ label,
                                                          const u64* __restrict__ line_off, const u64* __restrict__ segment_off,
                                                          const u32* __restrict__ link_ab, u64 total, uint8_t* __restrict__ text, const PartNumbers pn,
                                                          const GfaCoverage cov) {
    const u32 hdr = NUMBERED ? pn.hdr : 1u;
    constexpr int tags_max = COV ? S_TAGS_MAX_COV : S_TAGS_MAX;
    constexpr int name_max = NUMBERED ? S_NAME_MAX_NUMBERED : S_NAME_MAX;
    __shared__ __align__(16) uint8_t s_img[TILE];      // the tile's bytes that are not bases
    __shared__ uint16_t s_off[MAX_LINES];              // where the tile's lines start, relative to the tile
    const u32 tid = threadIdx.x;
    const u64 n_tiles = (total + TILE - 1) / TILE;
    for (u64 tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const u64 base = tile * TILE;
        const int len = (int)min((u64)TILE, total - base);
        const u32 r_lo = workgroup_search(line_off, R, base), r_hi = workgroup_search(line_off, R, base + len - 1);
        const u32 n_in = min(r_hi - r_lo + 1, MAX_LINES);
        if (tid < 16 && (u32)len + tid < TILE) s_img[(u32)len + tid] = 0;             // (behind the text, up to the next multiple of 16: zeros)
        for (u32 j = tid; j < n_in; j += BLOCK) {
            const u32 r = r_lo + j;
            const u64 o = line_off[r];
            s_off[j] = o > base ? (uint16_t)(o - base) : 0;
            const int64_t rel = (int64_t)(o - base), end = (int64_t)(line_off[r + 1] - base);      // (end >= 1: the line overlaps the tile)
            if (NUMBERED ? r < hdr : r == 0) {
                put_tag_back<3>(s_img, put_tag_back<6>(s_img, (int)end - 1, len, tag('Z', ':', '1', '.', '0', '\n')), len, tag('V', 'N', ':', 0, 0, 0));
                put_tag_back<2>(s_img, (int)rel + 1, len, tag('H', '\t', 0, 0, 0, 0));
            } else if (NUMBERED ? r >= hdr + E : r > E) {
                const u32 l = NUMBERED ? r - hdr - E : r - 1 - E;
                int p = put_tag_back<2>(s_img, (int)end - 1, len, tag('M', '\n', 0, 0, 0, 0));
                p = put_decimal_back(s_img, p, len, k - 1);
                if constexpr (NUMBERED) {
                    p = put_decimal_back(s_img, put_tag_back<3>(s_img, p, len, tag('\t', '+', '\t', 0, 0, 0)), len, pn.link_b[l]);
                    p = put_decimal_back(s_img, put_tag_back<3>(s_img, p, len, tag('\t', '+', '\t', 0, 0, 0)), len, pn.first + pn.link_a[l]);
                } else {
                    p = put_decimal_back(s_img, put_tag_back<3>(s_img, p, len, tag('\t', '+', '\t', 0, 0, 0)), len, link_ab[2 * l + 1]);
                    p = put_decimal_back(s_img, put_tag_back<3>(s_img, p, len, tag('\t', '+', '\t', 0, 0, 0)), len, link_ab[2 * l]);
                }
                put_tag_back<2>(s_img, p, len, tag('L', '\t', 0, 0, 0, 0));
            } else {
                const u32 i = NUMBERED ? r - hdr : r - 1;
                if (rel > -name_max) {                                         // "S\t<i>\t" reaches into the tile
                    int p = (int)rel + (int)(segment_off[i] - o) - 1;
                    put(s_img, p--, len, '\t');
                    if constexpr (NUMBERED) p = put_decimal_back(s_img, p, len, pn.first + i);
                    else p = put_decimal_back(s_img, p, len, i);
                    put_tag_back<2>(s_img, p, len, tag('S', '\t', 0, 0, 0, 0));
                }
                if (end - tags_max < len) {                                    // the tags behind the bases do
                    const u32 w = weight[i], km = kmers[i];
                    int p = (int)end - 1;
                    put(s_img, p--, len, '\n');
                    if constexpr (COV) {
                        p = put_tag_back<6>(s_img, put_decimal_back(s_img, p, len, cov.kmer_max[i]), len, tag('\t', 'm', 'x', ':', 'i', ':'));
                        p = put_tag_back<6>(s_img, put_decimal_back(s_img, p, len, cov.kmer_min[i]), len, tag('\t', 'm', 'n', ':', 'i', ':'));
                    }
                    p = put_tag_back<6>(s_img, put_decimal_back(s_img, p, len, w), len, tag('\t', 'e', 'w', ':', 'i', ':'));
                    p = put_tag_back<6>(s_img, put_decimal_back(s_img, p, len, COV ? cov.kmer_sum[i] : (u64)w * km), len, tag('\t', 'K', 'C', ':', 'i', ':'));
                    put_tag_back<6>(s_img, put_decimal_back(s_img, p, len, km + k - 1), len, tag('\t', 'L', 'N', ':', 'i', ':'));
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int it = 0; it < STORES; ++it) {
            const u32 rel = (u32)it * BLOCK * 16 + tid * 16;
            const u64 o = base + rel;
            if (o >= total) continue;
            u32 lo = 0, hi = n_in;                                           // the line that holds byte o
            while (hi - lo > 1) { const u32 mid = (lo + hi) >> 1; if (s_off[mid] <= rel) lo = mid; else hi = mid; }
            u32 r = r_lo + lo;
            const uint4 img = *(const uint4*)(s_img + rel);
            uint4 v = img;                                                   // (from the first link on there are no bases)
            if (NUMBERED ? r < hdr + E : r <= E) {
                u32 at = (u32)(o - line_off[r]);
                Line ln = load_line<NUMBERED>(r, E, hdr, label, label_off, segment_off, line_off);
                if (at >= ln.head && at - ln.head + 16 <= ln.bases) {
                    v = sixteen_bases(ln.src, at - ln.head);
                } else {
                    const u32 in[4] = {img.x, img.y, img.z, img.w};
                    u32 w[4] = {0, 0, 0, 0};
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        if (r < R && at >= ln.total) {
                            ++r; at = 0;
                            if (r < R) ln = load_line<NUMBERED>(r, E, hdr, label, label_off, segment_off, line_off);
                        }
                        const bool base_here = r < R && at >= ln.head && at - ln.head < ln.bases;
                        const u32 c = base_here ? one_base(ln.src, at - ln.head) : (in[i >> 2] >> (8 * (i & 3))) & 0xFF;
                        w[i >> 2] |= c << (8 * (i & 3));
                        ++at;
                    }
                    v = make_uint4(w[0], w[1], w[2], w[3]);
                }
            }
            *(uint4*)(text + o) = v;                                         // (the buffer is a multiple of 16 bytes)
        }
        __syncthreads();                                                     // (the image and s_off are rewritten by the next tile)
    }
}

// ---- a numbered part: the same sizes, counted with the digits of the GLOBAL numbers --------------------------------------------
// segment i of a part (named first + i): its label's checks, that its links' range ascends (link_first[0] = 0), its line's bytes
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
        const int bad = label_check(label, label_off[i], label_off[i + 1], label_bytes, k, &bases);
        if (bad) { atomicOr(err, (u32)(bad == 2 ? ERR_LABEL_LEN : ERR_LABEL)); continue; }
        if ((u64)bases != (u64)kmers[i] + k - 1) { atomicOr(err, (u32)ERR_KMERS); continue; }
        const u32 w = weight[i];
        if constexpr (COV) {
            if (!coverage_fits(cov, i, w, kmers[i])) { atomicOr(err, (u32)ERR_COVERAGE); continue; }
            size[hdr + i] = 2 + decimal_digits(first + i) + 1 + bases + 6 + decimal_digits(bases) + coverage_tag_bytes(cov, i, w);
            continue;
        }
        size[hdr + i] = 2 + decimal_digits(first + i) + 1 + bases + 6 + decimal_digits(bases) + 6 + decimal_digits((u64)w * kmers[i]) + 6 + decimal_digits(w) + 1;
    }
}
// link l of a part: its segment is the last one whose first link is <= l (as gfa_link_fill_kernel finds it); its line's bytes
__global__ __launch_bounds__(BLOCK) void gfa_part_link_kernel(u32 E, u64 L, u64 first, u32 k1_digits, const u64* __restrict__ link_first,
                                                              const u64* __restrict__ link_b, u32* __restrict__ link_a, u32* __restrict__ size) {
    for (u64 l = (u64)blockIdx.x * BLOCK + threadIdx.x; l < L; l += (u64)gridDim.x * BLOCK) {
        u32 lo = 0, hi = E;
        while (hi - lo > 1) { const u32 mid = lo + ((hi - lo) >> 1); if (link_first[mid] <= l) lo = mid; else hi = mid; }
        link_a[l] = lo;
        size[l] = 10 + decimal_digits(first + lo) + decimal_digits(link_b[l]) + k1_digits;
    }
}
__global__ __launch_bounds__(BLOCK) void gfa_part_segment_off_kernel(u64 E, u64 first, u32 hdr, const u64* __restrict__ line_off, u64* __restrict__ segment_off) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < E; i += (u64)gridDim.x * BLOCK) segment_off[i] = line_off[hdr + i] + 3 + decimal_digits(first + i);
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
        hipLaunchKernelGGL(gfa_segment_off_kernel, grid, blk, 0, stream, E, plan.line_off.as<u64>(), plan.segment_off.as<u64>());
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
        hipLaunchKernelGGL(gfa_part_segment_off_kernel, grid, blk, 0, stream, E, first, hdr, plan.s_line_off.as<u64>(), plan.segment_off.as<u64>());
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
    if ((uintptr_t)d_edge_label & 3) { set_error("gfa: d_edge_label must be 4-byte aligned (the kernel reads the aligned words around the bytes it needs)"); return KATOME_E_ARG; }
    const GfaPart g{k, n_edges, d_edge_weight, d_edge_kmers, d_edge_label_off, d_edge_label, label_bytes, first_segment, with_header != 0, d_link_first, d_link_b};
    GfaPartPlan plan;
    KCHECK(dev_gfa_part_plan(g, plan, stream));
    *s_bytes = plan.s_bytes; *l_offset = plan.l_offset(); *l_bytes = plan.l_bytes;
    if (!d_text) return KATOME_OK;
    if ((n_edges && !d_segment_off) || text_cap < plan.buffer_bytes() || ((uintptr_t)d_text & 15)) {
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
    const ShrinkOutput& sh = b->shrunk;
    if (c->n_edges != sh.n_edges || c->n_nodes != sh.n_nodes || c->d_edge_src != sh.edge_src.as<u64>() || c->d_edge_label != sh.edge_label.as<uint8_t>() ||
        c->d_edge_label_off != sh.edge_label_off.as<u64>()) {
        set_error("contigs_gfa: not the result of this builder's last katome_dev_shrink");
        return KATOME_E_ARG;
    }
    if (coverage && (!b->shrunk_cov.valid || b->shrunk_cov.n_edges != sh.n_edges)) {
        set_error("contigs_gfa_coverage: this builder's last shrink was not a katome_dev_shrink_coverage");
        return KATOME_E_ARG;
    }
    memset(out, 0, sizeof *out);
    GfaGraph g{b->s.k, sh.n_nodes, sh.n_edges, sh.edge_src.as<u64>(), sh.edge_dst.as<u64>(), sh.edge_weight.as<u32>(), sh.edge_kmers.as<u32>(),
               sh.edge_label_off.as<u64>(), sh.edge_label.as<uint8_t>(), sh.label_bytes};
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
    if ((uintptr_t)d_edge_label & 3) { set_error("gfa: d_edge_label must be 4-byte aligned (the kernel reads the aligned words around the bytes it needs)"); return KATOME_E_ARG; }
    const GfaGraph g{k, n_nodes, n_edges, d_edge_src, d_edge_dst, d_edge_weight, d_edge_kmers, d_edge_label_off, d_edge_label, label_bytes, cov};
    GfaPlan plan;
    KCHECK(dev_gfa_plan(g, plan, stream));
    *n_links = plan.n_links; *text_bytes = plan.text_bytes;
    if (!d_text) return KATOME_OK;
    if (!d_segment_off || !d_link_first || text_cap < (plan.text_bytes + 15) / 16 * 16 || ((uintptr_t)d_text & 15)) {
        set_error("gfa: %llu bytes (rounded up to 16, 16-byte aligned) do not fit the caller's arrays", (unsigned long long)plan.text_bytes);
        return KATOME_E_ARG;
    }
    // KATOME_GFA_TRACE=1: the writer's own time on stderr (there is no builder whose profile could hold it; tools/bench_gfa.py times
    // the S region alone through this entry, on a graph without links)
    Profiler prof;
    prof.on = getenv("KATOME_GFA_TRACE") != nullptr;
    {
        PhaseScope ps(prof, PH_GFA, stream);
        KCHECK(dev_gfa_write(g, plan, d_text, stream));
    }
    if (n_edges) KCHECK_HIP(hipMemcpyAsync(d_segment_off, plan.segment_off.p, n_edges * 8, hipMemcpyDeviceToDevice, stream));
    KCHECK_HIP(hipMemcpyAsync(d_link_first, plan.link_first.p, (n_edges + 1) * 8, hipMemcpyDeviceToDevice, stream));
    KCHECK_HIP(hipStreamSynchronize(stream));
    for (const Profiler::Ev& e : prof.evs) {
        float ms = 0;
        if (e.phase == K_GFA_WRITE && hipEventElapsedTime(&ms, e.a, e.b) == hipSuccess)
            fprintf(stderr, "[katome_dev_gfa_arrays] k:gfa_write_kernel %.4f ms, %llu bytes, %llu segments, %llu links\n", ms,
                    (unsigned long long)plan.text_bytes, (unsigned long long)n_edges, (unsigned long long)plan.n_links);
    }
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
