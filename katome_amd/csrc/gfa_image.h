// gfa_image.h -- what the two GFA writers share (gfa.hip: one segment per merged edge; gfa_strands.hip: strand twins folded into one
// segment): the tile a workgroup owns, the bounds of its line table, and the LDS image that everything that is not a base is
// formatted into, right to left, once per line.
#pragma once
#include "common.h"

namespace katome {

constexpr int STORES = 2;                              // 16-byte stores per lane and tile
constexpr u32 TILE = BLOCK * 16 * STORES;              // output bytes a workgroup owns at a time
constexpr u32 HEADER_BYTES = 11;                       // "H\tVN:Z:1.0\n": the shortest line (an L line has 13 bytes or more, an S line more still)
constexpr u32 MAX_LINES = TILE / HEADER_BYTES + 2;     // lines that can overlap one tile
constexpr int S_NAME_MAX = 2 + 10 + 1;                 // "S\t<i>\t", i < 2^32
static_assert(TILE <= 65536, "offsets inside a tile are kept in 16 bits");

constexpr u64 tag(char a, char b, char c, char d, char e, char f) {      // six characters, the first in the low byte
    return (u64)(uint8_t)a | (u64)(uint8_t)b << 8 | (u64)(uint8_t)c << 16 | (u64)(uint8_t)d << 24 | (u64)(uint8_t)e << 32 | (u64)(uint8_t)f << 40;
}

inline u32 host_digits(u64 v) { u32 d = 1; while (v >= 10) { v /= 10; ++d; } return d; }

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
#endif

struct Line {
    const uint8_t* src;       // a segment's packed bases
    u32 head, bases, total;   // bytes in front of the bases; the bases; all the line's bytes.  Not a segment: head = total, no bases
};

}  // namespace katome
