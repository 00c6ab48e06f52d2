// gfa_image.h -- the tile scheme of every GFA writer, once.  A text is partitioned by OUTPUT bytes: a workgroup owns TILE bytes at a
// time, and everything that is not a base is formatted once per record, right to left, into an LDS image of the tile.
//   Here: the tile's constants, the image's primitives (put, put_decimal_back, put_tag_back) and write_line_tile, a whole tile of the
//   H/S/L texts.  What a line IS comes from a line description passed by value: gfa.hip has two (the one-GPU text and the
//   numbered part of a sharded text), gfa_strands.hip one (strand twins folded into one segment); their kernels loop over the tiles round it.
//   gfa_lines.h holds the line rules the descriptions are made of, gfa_path_lines.h the image-only tile of the P lines.
#pragma once
#include "common.h"
#include "text_bases.h"

namespace katome {

constexpr int STORES = 2;                              // 16-byte stores per lane and tile
constexpr u32 TILE = BLOCK * 16 * STORES;              // output bytes a workgroup owns at a time
constexpr u32 HEADER_BYTES = 11;                       // "H\tVN:Z:1.0\n": the shortest line (an L line has 13 bytes or more, an S line more still)
constexpr u32 MAX_LINES = TILE / HEADER_BYTES + 2;     // lines that can overlap one tile
static_assert(TILE <= 65536, "offsets inside a tile are kept in 16 bits");

constexpr u64 tag(char a, char b, char c, char d, char e, char f) {      // six characters, the first in the low byte
    return (u64)(uint8_t)a | (u64)(uint8_t)b << 8 | (u64)(uint8_t)c << 16 | (u64)(uint8_t)d << 24 | (u64)(uint8_t)e << 32 | (u64)(uint8_t)f << 40;
}

inline u32 host_digits(u64 v) { u32 d = 1; while (v >= 10) { v /= 10; ++d; } return d; }

struct Line {
    const uint8_t* src;       // a segment's packed bases
    u32 head, bases, total;   // bytes in front of the bases; the bases; all the line's bytes.  Not a segment: head = total, no bases
};

#ifdef __HIPCC__
// ---- the LDS image of a tile: bytes at positions relative to the tile, those outside [0, len) dropped ------------------------------
__device__ __forceinline__ void put(uint8_t* img, int pos, int len, u32 c) { if (pos >= 0 && pos < len) img[pos] = (uint8_t)c; }
// v in decimal, its last digit at `pos`; returns the position in front of its first digit
template <class T> __device__ __forceinline__ int put_decimal_back(uint8_t* img, int pos, int len, T v) {
    do { put(img, pos--, len, '0' + (u32)(v % 10)); v /= 10; } while (v);
    return pos;
}
// n characters of t (the first in the low byte), the last one at `pos`
template <int n> __device__ __forceinline__ int put_tag_back(uint8_t* img, int pos, int len, u64 t) {
#pragma unroll
    for (int j = n - 1; j >= 0; --j) put(img, pos--, len, (u32)(t >> (8 * j)) & 0xFF);
    return pos;
}

// ---- one tile of a text of R lines at line_off (one entry more than lines; `total` bytes, the buffer a multiple of 16): the bytes
// [base, base + len), which the lines r_lo .. r_hi overlap ------------------------------------------------------------------------------
// The kernel finds the lines that overlap the tile by the workgroup search; their starts are kept in LDS.  Everything that is not a
// base -- the header, an S line's name and tags, whole L lines: short records full of decimal numbers -- is formatted ONCE per line,
// one thread per line, into the image (a division by ten per digit, not per byte and lane).  Then every lane produces 16 consecutive
// bytes with one 128-bit store: 16 bases of one segment straight from the 2-bit label (sixteen_bases); from the first link on the
// image's 16 bytes as they are; anywhere else the image's bytes with the bases among them filled in one at a time.
// The line description D answers, for line r:
//   d.before_links(r)                         r is a header or a segment (from the first link on there are no bases)
//   d.format(img, r, o, rel, end, len)        r's bytes that are not bases into the image: the line starts at byte o of the text, at
//                                             rel and ends in front of end relative to the tile (end >= 1: the line overlaps the tile)
//   d.line(r, line_off)                       r's Line
// The loop over the tiles and the two searches stay in the kernel (three lines, the same in every writer): searched from inside this
// function -- one call deeper -- the compiler no longer folds the work-group size that workgroup_search's reduction reads to the
// uniform one; it keeps the choice between the group's size and the grid's remainder, two dependent loads in front of every search,
// and gfa_write_kernel took 15 % longer (profiles/gfa_writers_one_tile.md).
__device__ __forceinline__ int tile_len(u64 base, u64 total) { return (int)min((u64)TILE, total - base); }
template <class D>
__device__ __forceinline__ void write_line_tile(const D d, u32 R, u32 r_lo, u32 r_hi, u64 base, int len, const u64* __restrict__ line_off, u64 total,
                                                uint8_t* __restrict__ text) {
    __shared__ __align__(16) uint8_t s_img[TILE];      // the tile's bytes that are not bases
    __shared__ uint16_t s_off[MAX_LINES];              // where the tile's lines start, relative to the tile
    const u32 tid = threadIdx.x;
    const u32 n_in = min(r_hi - r_lo + 1, MAX_LINES);
    if (tid < 16 && (u32)len + tid < TILE) s_img[(u32)len + tid] = 0;             // (behind the text, up to the next multiple of 16: zeros)
    for (u32 j = tid; j < n_in; j += BLOCK) {
        const u32 r = r_lo + j;
        const u64 o = line_off[r];
        s_off[j] = o > base ? (uint16_t)(o - base) : 0;
        d.format(s_img, r, o, (int64_t)(o - base), (int64_t)(line_off[r + 1] - base), len);
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
        uint4 v = img;
        if (d.before_links(r)) {
            u32 at = (u32)(o - line_off[r]);
            Line ln = d.line(r, line_off);
            if (at >= ln.head && at - ln.head + 16 <= ln.bases) {
                v = sixteen_bases(ln.src, at - ln.head);
            } else {
                const u32 in[4] = {img.x, img.y, img.z, img.w};
                u32 w[4] = {0, 0, 0, 0};
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    if (r < R && at >= ln.total) {
                        ++r; at = 0;
                        if (r < R) ln = d.line(r, line_off);
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
#endif

}  // namespace katome
