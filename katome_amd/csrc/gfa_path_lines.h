// gfa_path_lines.h -- the P lines of both path texts, once (gfa_paths.hip: every piece "<id>+"; gfa_strand_paths.hip: "<rep><o>" over the
// merged segments): how many pieces can overlap a tile, the head of a line, "P\tkatome_<c>[.<r>]\t", and write_piece_tile, a whole
// tile on gfa_image.h's LDS image.  The two kernels loop over the tiles round it and say what a piece is called.
#pragma once
#include "gfa_image.h"

namespace katome {

constexpr u32 PIECE_MIN = 3;                               // "0+,": the shortest piece
constexpr int PIECE_MAX = 9 + 10 + 1 + 10 + 1 + 10 + 4;    // "P\tkatome_<c>.<r>\t<id>+\t*\n" with c, r, id < 2^31: far below a tile
constexpr u32 MAX_PIECES = TILE / PIECE_MIN + 2;           // pieces that can overlap one tile
static_assert(PIECE_MAX < (int)TILE && MAX_PIECES < 65536, "a piece fits a tile; a tile's pieces are counted in 32 bits with room to spare");

#ifdef __HIPCC__
// the bytes of "P\tkatome_<c>[.<r>]\t"
__device__ __forceinline__ u32 run_head_bytes(u64 c, u64 r) { return 9 + decimal_digits(c) + (r ? 1 + decimal_digits(r) : 0) + 1; }
// ... and the head itself, its last byte at `pos` (gfa_paths_write_kernel used to spell these lines out, because through this function
// the compiler schedules it differently; it still does, and the kernel measures no slower: profiles/gfa_writers_one_tile.md)
__device__ __forceinline__ void put_run_head(uint8_t* img, int pos, int len, u64 c, u64 r) {
    put(img, pos--, len, '\t');
    if (r) { pos = put_decimal_back(img, pos, len, r); put(img, pos--, len, '.'); }
    pos = put_decimal_back(img, pos, len, c);
    put_tag_back<3>(img, put_tag_back<6>(img, pos, len, tag('a', 't', 'o', 'm', 'e', '_')), len, tag('P', '\t', 'k', 0, 0, 0));
}

struct PieceName { u32 number; char sign; };           // a piece reads "<number><sign>"

// One tile of a text of P lines: the bytes [base, base + len), which the pieces p_lo .. p_hi overlap (the kernel finds them by the
// workgroup search in the scanned offsets, piece_off, one entry more than pieces: the loop over the tiles and the two searches stay
// in the kernel for the reason gfa_image.h gives).  A piece is a short record of decimal numbers, so the tile is written as
// write_line_tile writes its L region: every piece is formatted ONCE, one thread per piece, right to left into the image (what falls
// outside the tile is dropped) -- "<number><sign>," or, on a run's last piece, "<number><sign>\t*\n", behind the line's head on its
// first --, and then every lane stores 16 consecutive bytes of the image with one 128-bit store.  name(p): piece p's PieceName
template <class Name>
__device__ __forceinline__ void write_piece_tile(const Name name, u32 P, u32 p_lo, u32 p_hi, u64 base, int len, const u64* __restrict__ path_idx,
                                                 const u64* __restrict__ piece_off, const u64* __restrict__ path_contig, const u64* __restrict__ contig_first_path,
                                                 u64 total, uint8_t* __restrict__ text) {
    __shared__ __align__(16) uint8_t s_img[TILE];      // the tile's bytes
    const u32 tid = threadIdx.x;
    const u32 n_in = min(p_hi - p_lo + 1, MAX_PIECES);
    if (tid < 16 && (u32)len + tid < TILE) s_img[(u32)len + tid] = 0;             // (behind the text, up to the next multiple of 16: zeros)
    for (u32 j = tid; j < n_in; j += BLOCK) {
        const u32 p = p_lo + j;
        const PieceName pn = name(p);
        const u64 path = path_idx[p];
        int pos = (int)(int64_t)(piece_off[p + 1] - base) - 1;                    // (>= 0: the piece overlaps the tile)
        if (p + 1 == P || path_idx[p + 2] != path_idx[p + 1]) pos = put_tag_back<4>(s_img, pos, len, tag(pn.sign, '\t', '*', '\n', 0, 0));
        else pos = put_tag_back<2>(s_img, pos, len, tag(pn.sign, ',', 0, 0, 0, 0));
        pos = put_decimal_back(s_img, pos, len, pn.number);
        if (path_idx[p + 1] != path && pos >= 0) {                                // the line's head, where it reaches into the tile
            const u64 c = path_contig[path];
            put_run_head(s_img, pos, len, c, path - contig_first_path[c]);
        }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < STORES; ++it) {
        const u32 rel = (u32)it * BLOCK * 16 + tid * 16;
        const u64 o = base + rel;
        if (o >= total) continue;
        *(uint4*)(text + o) = *(const uint4*)(s_img + rel);                       // (the buffer is a multiple of 16 bytes)
    }
    __syncthreads();                                                              // (the image is rewritten by the next tile)
}
#endif

}  // namespace katome
