// gfa_lines.h -- the rules of the H, S and L lines, once: how many bytes a line has, what is checked before a segment is measured, and
// how a line's bytes that are not bases go into the image of a tile (gfa_image.h).  The format is fixed in include/katome_gpu.h:
//   H\tVN:Z:1.0\n
//   S\t<name>\t<bases>\tLN:i:<bases>\tKC:i:<kc>\tew:i:<weight><a text's own tags>\n
//   L\t<a>\t<oa>\t<b>\t<ob>\t<k-1>M\n
// The measure kernels and the line descriptions of gfa.hip (the one-GPU text, the numbered part, both with or without the coverage
// tags written here) and gfa_strands.hip (strand twins folded into one segment, with its twin tags) are made of these.
#pragma once
#include "gfa_image.h"

namespace katome {

constexpr int S_NAME_MAX = 2 + 10 + 1;                 // "S\t<i>\t", i < 2^32
constexpr int S_NAME_MAX_NUMBERED = 2 + 20 + 1;        // ... of a numbered part: first_segment + i < 2^64
constexpr u32 L_LINE_MAX = 10 + 20 + 20 + 10;          // "L\t<a>\t+\t<b>\t+\t<k-1>M\n" with two 64-bit numbers: far below a tile
// (no line is shorter than the header's 11 bytes -- the shortest L line, "L\t0\t+\t0\t+\t0M\n", has 13 and an S line more --, so
// MAX_LINES and the 16-bit offsets hold for every text: longer numbers and more tags only make lines longer)
static_assert(L_LINE_MAX < TILE && HEADER_BYTES <= 13, "a tile holds at most MAX_LINES lines");
enum { ERR_NODE = 1, ERR_LABEL = 2, ERR_LABEL_LEN = 4, ERR_KMERS = 8, ERR_LINKS = 16, ERR_COVERAGE = 32 };

#ifdef __HIPCC__
// ---- sizes -------------------------------------------------------------------------------------------------------------------------
// (extra: the bytes of the text's own tags between ew and the line's end)
__device__ __forceinline__ u32 segment_line_bytes(u64 name, u32 bases, u64 kc, u32 w, u32 extra) {
    return 2 + decimal_digits(name) + 1 + bases + 6 + decimal_digits(bases) + 6 + decimal_digits(kc) + 6 + decimal_digits(w) + 1 + extra;
}
__device__ __forceinline__ u32 link_line_bytes(u64 a, u64 b, u32 k1_digits) { return 10 + decimal_digits(a) + decimal_digits(b) + k1_digits; }
// a segment's first base: behind "S\t<name>\t"
__device__ __forceinline__ u64 segment_first_base(u64 line_at, u64 name) { return line_at + 3 + decimal_digits(name); }

// link l's segment: the last one whose first link is <= l (segments without links share their successor's first link and are passed over)
__device__ __forceinline__ u32 last_segment_with_first_link_le(const u64* __restrict__ link_first, u32 E, u64 l) {
    u32 lo = 0, hi = E;
    while (hi - lo > 1) { const u32 mid = lo + ((hi - lo) >> 1); if (link_first[mid] <= l) lo = mid; else hi = mid; }
    return lo;
}

// ---- the coverage tags (COV, GfaCoverage of common.h): KC is the sum of the path's k-mer counts, "\tmn:i:<min>\tmx:i:<max>" follows ew ----
constexpr int COV_TAGS_MAX = 2 * (6 + 10);
// a segment's coverage fits its weight and its k-mers: min <= weight <= max and min * kmers <= sum <= max * kmers (64-bit: u32 * u32)
__device__ __forceinline__ bool coverage_fits(const GfaCoverage& c, u64 i, u32 w, u32 km) {
    const u32 mn = c.kmer_min[i], mx = c.kmer_max[i];
    const u64 sum = c.kmer_sum[i];
    return mn <= w && w <= mx && (u64)mn * km <= sum && sum <= (u64)mx * km;
}
// KC as the SHRUNK edge carries it -- shrink keeps only the weight of a path's first k-mer (shrinker.rs:181,200), so the weight times
// the k-mers merged into the edge, a 64-bit product of up to 20 digits -- or, with coverage, the true sum
template <bool COV> __device__ __forceinline__ u64 segment_kc(const GfaCoverage& c, u64 i, u32 w, u32 km) {
    if constexpr (COV) return c.kmer_sum[i]; else return (u64)w * km;
}
template <bool COV> __device__ __forceinline__ int put_coverage_tags(uint8_t* img, int p, int len, const GfaCoverage& c, u64 i) {
    if constexpr (COV) {
        p = put_tag_back<6>(img, put_decimal_back(img, p, len, c.kmer_max[i]), len, tag('\t', 'm', 'x', ':', 'i', ':'));
        p = put_tag_back<6>(img, put_decimal_back(img, p, len, c.kmer_min[i]), len, tag('\t', 'm', 'n', ':', 'i', ':'));
    }
    return p;
}

// ---- checks ------------------------------------------------------------------------------------------------------------------------
// Edge i as a segment: everything the later kernels read through (the label's offsets, pad byte and length), that the label spells
// edge_kmers + k - 1 bases and, with COV, that the coverage fits.  0 and *bases, or the error bit (nothing is sized from bad values)
template <bool COV>
__device__ __forceinline__ u32 check_segment(u32 k, u64 i, const u32* __restrict__ weight, const u32* __restrict__ kmers, const u64* __restrict__ label_off,
                                             const uint8_t* __restrict__ label, u64 label_bytes, const GfaCoverage& cov, u32* bases) {
    const int bad = label_check(label, label_off[i], label_off[i + 1], label_bytes, k, bases);
    if (bad) return bad == 2 ? ERR_LABEL_LEN : ERR_LABEL;
    if ((u64)*bases != (u64)kmers[i] + k - 1) return ERR_KMERS;
    if constexpr (COV) { if (!coverage_fits(cov, i, weight[i], kmers[i])) return ERR_COVERAGE; }
    return 0;
}
// ... and its line's bytes under `name`, once it has passed
template <bool COV>
__device__ __forceinline__ u32 checked_segment_bytes(u64 name, u64 i, u32 bases, const u32* __restrict__ weight, const u32* __restrict__ kmers, const GfaCoverage& cov) {
    const u32 w = weight[i];
    u32 extra = 0;
    if constexpr (COV) extra = 6 + decimal_digits(cov.kmer_min[i]) + 6 + decimal_digits(cov.kmer_max[i]);
    return segment_line_bytes(name, bases, segment_kc<COV>(cov, i, w, kmers[i]), w, extra);
}

// ---- a line's bytes that are not bases, into the image (rel, end, len: write_line_tile of gfa_image.h) ------------------------------------
__device__ __forceinline__ void put_header_line(uint8_t* img, int64_t rel, int64_t end, int len) {
    put_tag_back<3>(img, put_tag_back<6>(img, (int)end - 1, len, tag('Z', ':', '1', '.', '0', '\n')), len, tag('V', 'N', ':', 0, 0, 0));
    put_tag_back<2>(img, (int)rel + 1, len, tag('H', '\t', 0, 0, 0, 0));
}
// "L\t<a>\t<oa>\t<b>\t<ob>\t<k1>M\n"
template <class A, class B>
__device__ __forceinline__ void put_link_line(uint8_t* img, int64_t end, int len, A a, char oa, B b, char ob, u32 k1) {
    int p = put_tag_back<2>(img, (int)end - 1, len, tag('M', '\n', 0, 0, 0, 0));
    p = put_decimal_back(img, p, len, k1);
    p = put_decimal_back(img, put_tag_back<3>(img, p, len, tag('\t', ob, '\t', 0, 0, 0)), len, b);
    p = put_decimal_back(img, put_tag_back<3>(img, p, len, tag('\t', oa, '\t', 0, 0, 0)), len, a);
    put_tag_back<2>(img, p, len, tag('L', '\t', 0, 0, 0, 0));
}
// "S\t<name>\t", head bytes long, where it reaches into the tile (the name's digits were counted when the line was measured)
template <int NAME_ROOM, class N> __device__ __forceinline__ void put_segment_name(uint8_t* img, int64_t rel, int len, int head, N name) {
    if (rel > -NAME_ROOM) {
        int p = (int)rel + head - 1;
        put(img, p--, len, '\t');
        p = put_decimal_back(img, p, len, name);
        put_tag_back<2>(img, p, len, tag('S', '\t', 0, 0, 0, 0));
    }
}
// "\tLN:i:<bases>\tKC:i:<kc>\tew:i:<w>", then what `extra` writes (right to left from the position it is given; it returns the position
// in front), then the line's end.  The caller asks first whether the tags reach into the tile: end - (S_TAGS_MAX + its own tags') < len
constexpr int S_TAGS_MAX = 3 * 6 + 10 + 20 + 10 + 1;   // "\tLN:i:<u32>\tKC:i:<u64>\tew:i:<u32>\n"
template <class Extra>
__device__ __forceinline__ void put_segment_tags(uint8_t* img, int64_t end, int len, u32 bases, u64 kc, u32 w, Extra extra) {
    int p = (int)end - 1;
    put(img, p--, len, '\n');
    p = extra(p);
    p = put_tag_back<6>(img, put_decimal_back(img, p, len, w), len, tag('\t', 'e', 'w', ':', 'i', ':'));
    p = put_tag_back<6>(img, put_decimal_back(img, p, len, kc), len, tag('\t', 'K', 'C', ':', 'i', ':'));
    put_tag_back<6>(img, put_decimal_back(img, p, len, bases), len, tag('\t', 'L', 'N', ':', 'i', ':'));
}

// ---- a line as write_line_tile reads it ----------------------------------------------------------------------------------------------
// line r without bases, and the bases of edge i added to it where it is a segment whose first base lies at first_base of the text
__device__ __forceinline__ Line line_without_bases(const u64* __restrict__ line_off, u32 r, const uint8_t* __restrict__ label) {
    Line ln;
    ln.total = (u32)(line_off[r + 1] - line_off[r]);
    ln.head = ln.total; ln.bases = 0; ln.src = label;
    return ln;
}
__device__ __forceinline__ void add_bases(Line& ln, const uint8_t* __restrict__ label, const u64* __restrict__ label_off, u32 i, u32 head) {
    const u64 lo = label_off[i], hi = label_off[i + 1];
    ln.src = label + lo + 1;
    ln.bases = 4 * (u32)(hi - lo - 1) - label[lo];
    ln.head = head;
}
#endif

}  // namespace katome
