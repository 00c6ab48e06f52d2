// gfa_path_lines.h -- what the two writers of P lines share (gfa_paths.hip: every piece "<id>+"; gfa_strand_paths.hip: "<rep><o>" over the
// merged segments): how many pieces can overlap a tile, and the head of a line, "P\tkatome_<c>[.<r>]\t".
#pragma once
#include "gfa_image.h"
#include "text_bases.h"

namespace katome {

constexpr u32 PIECE_MIN = 3;                               // "0+,": the shortest piece
constexpr int PIECE_MAX = 9 + 10 + 1 + 10 + 1 + 10 + 4;    // "P\tkatome_<c>.<r>\t<id>+\t*\n" with c, r, id < 2^31: far below a tile
constexpr u32 MAX_PIECES = TILE / PIECE_MIN + 2;           // pieces that can overlap one tile
static_assert(PIECE_MAX < (int)TILE && MAX_PIECES < 65536, "a piece fits a tile; a tile's pieces are counted in 32 bits with room to spare");

#ifdef __HIPCC__
// the bytes of "P\tkatome_<c>[.<r>]\t"
__device__ __forceinline__ u32 run_head_bytes(u64 c, u64 r) { return 9 + decimal_digits(c) + (r ? 1 + decimal_digits(r) : 0) + 1; }
// ... and the head itself, its last byte at `pos` (gfa_paths_write_kernel spells the same four lines out: written through this
// function the compiler schedules that kernel differently, and it is kept instruction for instruction what it was)
__device__ __forceinline__ void put_run_head(uint8_t* img, int pos, int len, u64 c, u64 r) {
    put(img, pos--, len, '\t');
    if (r) { pos = put_decimal_back(img, pos, len, r); put(img, pos--, len, '.'); }
    pos = put_decimal_back(img, pos, len, c);
    put_tag_back<3>(img, put_tag_back<6>(img, pos, len, tag('a', 't', 'o', 'm', 'e', '_')), len, tag('P', '\t', 'k', 0, 0, 0));
}
#endif

}  // namespace katome
