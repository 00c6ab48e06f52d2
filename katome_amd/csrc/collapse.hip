// collapse.hip -- Collapsable::collapse for PtGraph (reference src/katome/algorithms/collapser.rs:25-273) and the text of its contigs
// (Contigs::save_to_file, asm/mod.rs:57-72).  Which contigs come out, and in which order, is a sequential walk over petgraph's own
// layout: one host core, collapse_exact.h, after shrink_exact.h.  That walk emits PIECES -- the shrunk edge appended at every step, by
// its index in the shrunk graph, with a flag on the piece that begins a contig (the whole label, name(); every other piece is the
// label from base k-1 on, remainder()).  Everything that touches a base is here, on the device: the pieces are measured from their
// labels alone, scanned into output offsets, and the text is written by a kernel that is partitioned by OUTPUT bytes -- after shrink
// one contig can be 10^7 bases and the next million pieces one base each, so neither a thread per piece nor one per contig would do.
//   text_write_kernel: a workgroup owns TILE output bytes; it finds the pieces that overlap them by two searches in the scanned
//   offsets (256 probes a round, all threads), keeps those pieces' offsets in LDS, and every lane produces 16 consecutive bytes with
//   one 128-bit store: it finds its piece in LDS and, when its 16 bytes are 16 bases of that one piece, cuts 32 bits out of the 2-bit
//   source at whatever base offset they start (k-1 is rarely a multiple of 4) and turns them into ASCII four at a time (v_perm_b32);
//   lanes whose bytes straddle a piece boundary, a FASTA header or a newline go byte by byte, and still store once.
// A FASTA header carries first_contig + the contig's index (u64, up to 20 digits): the text may be one rank's part of a larger one
// (dist_text.hip).  Its digits are counted once, when the pieces are measured; the writing kernel takes a header's length from the
// scanned sizes, so the 16-bases path does no digit arithmetic.
// The *_named kernels are the same three kernels for a text whose record i keeps the number it has in another text, name[i]
// (unique_contigs.hip): one more indexed read where a header's number is needed, over the same device functions.  They are kernels
// of their own, written out: with the number's source as a template argument of shared bodies the compiler did not leave the counted
// kernels instruction for instruction what they were.
#include <algorithm>
#include <chrono>
#include <new>

#include "collapse_exact.h"
#include "common.h"
#include "text_bases.h"

namespace katome {
namespace {

typedef uint32_t u32;
constexpr u32 WHOLE = KATOME_PIECE_WHOLE;
constexpr int STORES = 2;                              // 16-byte stores per lane and tile
constexpr u32 TILE = BLOCK * 16 * STORES;              // output bytes a workgroup owns at a time
static_assert(TILE <= 65536, "offsets inside a tile are kept in 16 bits");
constexpr u32 ACGT = TEXT_ACGT, MAX_LABEL_BYTES = TEXT_MAX_LABEL_BYTES;      // (text_bases.h: shared with gfa.hip)
enum { ERR_PIECE = 1, ERR_LABEL = 2, ERR_CONTIG_LEN = 4, ERR_LABEL_LEN = 8, ERR_FIRST = 16 };

__device__ __forceinline__ u32 piece_word(const u32* pieces, u32 p) { return pieces ? pieces[p] : (p | WHOLE); }
// bytes in front of a contig's bases (FASTA: ">katome_<i>\n"; i = the caller's first_contig + the contig's index, up to 20 digits)
__device__ __forceinline__ u32 header_bytes(u32 fasta, u64 contig) { return fasta ? 9 + decimal_digits(contig) : 0; }

__global__ __launch_bounds__(BLOCK) void piece_flag_kernel(const u32* __restrict__ pieces, u64 P, u32* __restrict__ flag) {
    for (u64 p = (u64)blockIdx.x * BLOCK + threadIdx.x; p < P; p += (u64)gridDim.x * BLOCK) flag[p] = piece_word(pieces, (u32)p) >> 31;
}

// what piece p puts into the text: its bases (from the label alone: 4 * (bytes - 1) - pad, minus k - 1 for a remainder piece), in FASTA
// layout the header in front of a contig's first piece and the newline behind its last.  Checks everything the writing kernel will
// read through: a piece names a label, the label's offsets lie inside the labels, its pad byte and length make sense.
__global__ __launch_bounds__(BLOCK) void piece_measure_kernel(u32 k, const uint8_t* __restrict__ label, const u64* __restrict__ label_off, u64 n_labels,
                                                              const u32* __restrict__ pieces, u64 P, u32 fasta, u64 first_contig,
                                                              const u64* __restrict__ contig_idx, u32* __restrict__ size, u32* __restrict__ err) {
    const u64 label_bytes = label_off[n_labels];
    for (u64 p = (u64)blockIdx.x * BLOCK + threadIdx.x; p < P; p += (u64)gridDim.x * BLOCK) {
        const u32 w = piece_word(pieces, (u32)p), id = w & ~WHOLE;
        const bool whole = w >> 31;
        size[p] = 0;
        if (p == 0 && !whole) { atomicOr(err, (u32)ERR_FIRST); continue; }
        if (id >= n_labels) { atomicOr(err, (u32)ERR_PIECE); continue; }
        const u64 lo = label_off[id], hi = label_off[id + 1];
        if (lo >= hi || hi > label_bytes || hi - lo < 2) { atomicOr(err, (u32)ERR_LABEL); continue; }
        if (hi - lo - 1 > MAX_LABEL_BYTES) { atomicOr(err, (u32)ERR_LABEL_LEN); continue; }
        const u32 pad = label[lo], packed = 4 * (u32)(hi - lo - 1);
        if (pad > 3 || packed < pad + k) { atomicOr(err, (u32)ERR_LABEL); continue; }
        u32 n = packed - pad - (whole ? 0 : k - 1);
        if (fasta) {
            if (whole) n += header_bytes(1, first_contig + contig_idx[p]);
            if (p + 1 == P || piece_word(pieces, (u32)(p + 1)) >> 31) n += 1;
        }
        size[p] = n;
    }
}

// ... with contig c's header numbered name[c].  Pieces and labels have been checked by a piece_measure_kernel over the list these
// pieces were taken from, and are checked again all the same
__global__ __launch_bounds__(BLOCK) void piece_measure_named_kernel(u32 k, const uint8_t* __restrict__ label, const u64* __restrict__ label_off, u64 n_labels,
                                                                    const u32* __restrict__ pieces, u64 P, u32 fasta, const u64* __restrict__ name,
                                                                    const u64* __restrict__ contig_idx, u32* __restrict__ size, u32* __restrict__ err) {
    const u64 label_bytes = label_off[n_labels];
    for (u64 p = (u64)blockIdx.x * BLOCK + threadIdx.x; p < P; p += (u64)gridDim.x * BLOCK) {
        const u32 w = piece_word(pieces, (u32)p), id = w & ~WHOLE;
        const bool whole = w >> 31;
        size[p] = 0;
        if (p == 0 && !whole) { atomicOr(err, (u32)ERR_FIRST); continue; }
        if (id >= n_labels) { atomicOr(err, (u32)ERR_PIECE); continue; }
        const u64 lo = label_off[id], hi = label_off[id + 1];
        if (lo >= hi || hi > label_bytes || hi - lo < 2) { atomicOr(err, (u32)ERR_LABEL); continue; }
        if (hi - lo - 1 > MAX_LABEL_BYTES) { atomicOr(err, (u32)ERR_LABEL_LEN); continue; }
        const u32 pad = label[lo], packed = 4 * (u32)(hi - lo - 1);
        if (pad > 3 || packed < pad + k) { atomicOr(err, (u32)ERR_LABEL); continue; }
        u32 n = packed - pad - (whole ? 0 : k - 1);
        if (fasta) {
            if (whole) n += header_bytes(1, name[contig_idx[p]]);
            if (p + 1 == P || piece_word(pieces, (u32)(p + 1)) >> 31) n += 1;
        }
        size[p] = n;
    }
}

// contig i's first base and its length in bases, from the pieces' offsets: the first piece of a contig writes the offset, the last
// one (a launch later) the length
__global__ __launch_bounds__(BLOCK) void contig_bounds_kernel(const u32* __restrict__ pieces, u64 P, u32 fasta, u64 first_contig,
                                                              const u64* __restrict__ contig_idx, const u64* __restrict__ piece_off, int lengths,
                                                              u64* __restrict__ contig_off, u32* __restrict__ contig_len, u32* __restrict__ err) {
    for (u64 p = (u64)blockIdx.x * BLOCK + threadIdx.x; p < P; p += (u64)gridDim.x * BLOCK) {
        if (!lengths) {
            if (piece_word(pieces, (u32)p) >> 31) { const u64 c = contig_idx[p]; contig_off[c] = piece_off[p] + header_bytes(fasta, first_contig + c); }
        } else if (p + 1 == P || piece_word(pieces, (u32)(p + 1)) >> 31) {
            const u64 c = contig_idx[p + 1] - 1, len = piece_off[p + 1] - (fasta ? 1 : 0) - contig_off[c];
            if (len > 0xFFFFFFFFull) atomicOr(err, (u32)ERR_CONTIG_LEN);
            contig_len[c] = (u32)len;
        }
    }
}

__global__ __launch_bounds__(BLOCK) void contig_bounds_named_kernel(const u32* __restrict__ pieces, u64 P, u32 fasta, const u64* __restrict__ name,
                                                                    const u64* __restrict__ contig_idx, const u64* __restrict__ piece_off, int lengths,
                                                                    u64* __restrict__ contig_off, u32* __restrict__ contig_len, u32* __restrict__ err) {
    for (u64 p = (u64)blockIdx.x * BLOCK + threadIdx.x; p < P; p += (u64)gridDim.x * BLOCK) {
        if (!lengths) {
            if (piece_word(pieces, (u32)p) >> 31) { const u64 c = contig_idx[p]; contig_off[c] = piece_off[p] + header_bytes(fasta, name[c]); }
        } else if (p + 1 == P || piece_word(pieces, (u32)(p + 1)) >> 31) {
            const u64 c = contig_idx[p + 1] - 1, len = piece_off[p + 1] - (fasta ? 1 : 0) - contig_off[c];
            if (len > 0xFFFFFFFFull) atomicOr(err, (u32)ERR_CONTIG_LEN);
            contig_len[c] = (u32)len;
        }
    }
}

struct Piece {
    const uint8_t* src;       // the label's packed bases
    u32 first;                // the piece's first base in the label (0, or k - 1 for a remainder piece)
    u32 bases, head, total;   // bases it writes; bytes in front of them; all its bytes (a newline behind the bases when total > head + bases)
    u64 contig;               // the number in its header
};
// (the header's length is what the piece's scanned size leaves over: no digit is counted here, on the way to the 16-bases store)
__device__ __forceinline__ Piece load_piece(u32 p, u32 P, u32 k, const uint8_t* __restrict__ label, const u64* __restrict__ label_off,
                                            const u32* __restrict__ pieces, u32 fasta, u64 first_contig, const u64* __restrict__ contig_idx,
                                            const u64* __restrict__ piece_off) {
    const u32 w = piece_word(pieces, p), id = w & ~WHOLE;
    const bool whole = w >> 31;
    const u64 lo = label_off[id], hi = label_off[id + 1];
    Piece pc;
    pc.src = label + lo + 1;
    pc.first = whole ? 0 : k - 1;
    pc.bases = 4 * (u32)(hi - lo - 1) - label[lo] - pc.first;
    pc.contig = fasta && whole ? first_contig + contig_idx[p] : 0;
    pc.total = (u32)(piece_off[p + 1] - piece_off[p]);
    const u32 tail = fasta && (p + 1 == P || piece_word(pieces, p + 1) >> 31) ? 1 : 0;
    pc.head = fasta && whole ? pc.total - pc.bases - tail : 0;
    return pc;
}
// byte r of a piece's output
__device__ __forceinline__ u32 piece_byte(const Piece& pc, u32 r) {
    if (r < pc.head) {
        if (r < 4) return (0x74616B3Eu >> (8 * r)) & 0xFF;               // ">kat"
        if (r < 8) return (0x5F656D6Fu >> (8 * (r - 4))) & 0xFF;         // "ome_"
        if (r == pc.head - 1) return '\n';
        u64 v = pc.contig;
        for (u32 t = pc.head - 2 - r; t > 0; --t) v /= 10;               // digits behind this one
        return '0' + v % 10;
    }
    r -= pc.head;
    if (r >= pc.bases) return '\n';
    const u32 b = pc.first + r;
    return (ACGT >> (8 * ((pc.src[b >> 2] >> (6 - 2 * (b & 3))) & 3))) & 0xFF;
}
__global__ __launch_bounds__(BLOCK) void text_write_kernel(u32 k, const uint8_t* __restrict__ label, const u64* __restrict__ label_off,
                                                           const u32* __restrict__ pieces, u32 P, u32 fasta, u64 first_contig,
                                                           const u64* __restrict__ contig_idx, const u64* __restrict__ piece_off, u64 total,
                                                           uint8_t* __restrict__ text) {
    __shared__ uint16_t s_off[TILE];       // where the tile's pieces start, relative to the tile (every piece is at least one byte)
    const u32 tid = threadIdx.x;
    const u64 n_tiles = (total + TILE - 1) / TILE;
    for (u64 tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const u64 base = tile * TILE, last = min(base + TILE, total) - 1;
        const u32 p_lo = workgroup_search(piece_off, P, base), p_hi = workgroup_search(piece_off, P, last);
        const u32 n_in = min(p_hi - p_lo + 1, TILE);
        for (u32 j = tid; j < n_in; j += BLOCK) { const u64 o = piece_off[p_lo + j]; s_off[j] = o > base ? (uint16_t)(o - base) : 0; }
        __syncthreads();
#pragma unroll
        for (int it = 0; it < STORES; ++it) {
            const u32 rel = (u32)it * BLOCK * 16 + tid * 16;
            const u64 o = base + rel;
            if (o >= total) continue;
            u32 lo = 0, hi = n_in;                                           // the piece that holds byte o
            while (hi - lo > 1) { const u32 mid = (lo + hi) >> 1; if (s_off[mid] <= rel) lo = mid; else hi = mid; }
            u32 p = p_lo + lo;
            u32 r = (u32)(o - piece_off[p]);
            Piece pc = load_piece(p, P, k, label, label_off, pieces, fasta, first_contig, contig_idx, piece_off);
            uint4 v;
            if (r >= pc.head && r - pc.head + 16 <= pc.bases) {
                v = sixteen_bases(pc.src, pc.first + r - pc.head);
            } else {
                u32 w[4] = {0, 0, 0, 0};
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    if (p < P && r >= pc.total) {
                        ++p; r = 0;
                        if (p < P) pc = load_piece(p, P, k, label, label_off, pieces, fasta, first_contig, contig_idx, piece_off);
                    }
                    if (p < P) { w[i >> 2] |= piece_byte(pc, r) << (8 * (i & 3)); ++r; }
                }
                v = make_uint4(w[0], w[1], w[2], w[3]);
            }
            *(uint4*)(text + o) = v;                                         // (the buffer is a multiple of 16 bytes)
        }
        __syncthreads();                                                     // (s_off is rewritten by the next tile)
    }
}

// piece p of a text whose record i is numbered name[i]: load_piece numbering from 0 gives the record's index, which the name replaces
__device__ __forceinline__ Piece load_named_piece(u32 p, u32 P, u32 k, const uint8_t* __restrict__ label, const u64* __restrict__ label_off,
                                                  const u32* __restrict__ pieces, u32 fasta, const u64* __restrict__ name, const u64* __restrict__ contig_idx,
                                                  const u64* __restrict__ piece_off) {
    Piece pc = load_piece(p, P, k, label, label_off, pieces, fasta, 0, contig_idx, piece_off);
    if (pc.head) pc.contig = name[pc.contig];
    return pc;
}
// text_write_kernel with that one more indexed read on a record's first piece
__global__ __launch_bounds__(BLOCK) void text_write_named_kernel(u32 k, const uint8_t* __restrict__ label, const u64* __restrict__ label_off,
                                                                 const u32* __restrict__ pieces, u32 P, u32 fasta, const u64* __restrict__ name,
                                                                 const u64* __restrict__ contig_idx, const u64* __restrict__ piece_off, u64 total,
                                                                 uint8_t* __restrict__ text) {
    __shared__ uint16_t s_off[TILE];
    const u32 tid = threadIdx.x;
    const u64 n_tiles = (total + TILE - 1) / TILE;
    for (u64 tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const u64 base = tile * TILE, last = min(base + TILE, total) - 1;
        const u32 p_lo = workgroup_search(piece_off, P, base), p_hi = workgroup_search(piece_off, P, last);
        const u32 n_in = min(p_hi - p_lo + 1, TILE);
        for (u32 j = tid; j < n_in; j += BLOCK) { const u64 o = piece_off[p_lo + j]; s_off[j] = o > base ? (uint16_t)(o - base) : 0; }
        __syncthreads();
#pragma unroll
        for (int it = 0; it < STORES; ++it) {
            const u32 rel = (u32)it * BLOCK * 16 + tid * 16;
            const u64 o = base + rel;
            if (o >= total) continue;
            u32 lo = 0, hi = n_in;
            while (hi - lo > 1) { const u32 mid = (lo + hi) >> 1; if (s_off[mid] <= rel) lo = mid; else hi = mid; }
            u32 p = p_lo + lo;
            u32 r = (u32)(o - piece_off[p]);
            Piece pc = load_named_piece(p, P, k, label, label_off, pieces, fasta, name, contig_idx, piece_off);
            uint4 v;
            if (r >= pc.head && r - pc.head + 16 <= pc.bases) {
                v = sixteen_bases(pc.src, pc.first + r - pc.head);
            } else {
                u32 w[4] = {0, 0, 0, 0};
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    if (p < P && r >= pc.total) {
                        ++p; r = 0;
                        if (p < P) pc = load_named_piece(p, P, k, label, label_off, pieces, fasta, name, contig_idx, piece_off);
                    }
                    if (p < P) { w[i >> 2] |= piece_byte(pc, r) << (8 * (i & 3)); ++r; }
                }
                v = make_uint4(w[0], w[1], w[2], w[3]);
            }
            *(uint4*)(text + o) = v;
        }
        __syncthreads();
    }
}

int check_plan_errors(u32 err) {
    if (err & ERR_FIRST) { set_error("text: the first piece does not begin a contig"); return KATOME_E_ARG; }
    if (err & ERR_PIECE) { set_error("text: a piece names a label that does not exist"); return KATOME_E_ARG; }
    if (err & ERR_LABEL) { set_error("text: a label's offsets, pad byte or length (shorter than k bases) are malformed"); return KATOME_E_ARG; }
    if (err & ERR_LABEL_LEN) { set_error("text: a label of more than 2^31 bases"); return KATOME_E_UNSUPPORTED; }
    if (err & ERR_CONTIG_LEN) { set_error("text: a contig of 2^32 bases or more"); return KATOME_E_UNSUPPORTED; }
    return KATOME_OK;
}

}  // namespace

int dev_text_plan(uint32_t k, const uint8_t* label, const uint64_t* label_off, uint64_t n_labels, const uint32_t* pieces, uint64_t n_pieces,
                  uint32_t layout, uint64_t first_contig, TextPlan& plan, hipStream_t stream, const uint64_t* names) {
    plan.n_contigs = plan.text_bytes = 0;
    if (layout > KATOME_TEXT_FASTA) { set_error("text: unknown layout %u", layout); return KATOME_E_ARG; }
    if (n_pieces >= 0x80000000ull) { set_error("text: %llu pieces, at most 2^31 - 1", (unsigned long long)n_pieces); return KATOME_E_UNSUPPORTED; }
    if (n_pieces == 0) return KATOME_OK;
    if (!label || !label_off) { set_error("null argument"); return KATOME_E_ARG; }
    const u64 P = n_pieces;
    const dim3 grid(grid_for(P, BLOCK, 256u * 32u)), blk(BLOCK);
    DevBuf counts(stream), tail(stream);
    plan.contig_idx.stream = plan.piece_off.stream = stream;
    KCHECK(counts.alloc((P + 1) * 4)); KCHECK(plan.contig_idx.alloc((P + 2) * 8)); KCHECK(plan.piece_off.alloc((P + 2) * 8)); KCHECK(tail.alloc(16));
    KCHECK_HIP(hipMemsetAsync(tail.p, 0, 16, stream));
    hipLaunchKernelGGL(piece_flag_kernel, grid, blk, 0, stream, pieces, P, counts.as<u32>());
    KCHECK_HIP(hipGetLastError());
    KCHECK(dev_scan_counts(counts.as<u32>(), P, plan.contig_idx.as<u64>(), stream));
    if (names)
        hipLaunchKernelGGL(piece_measure_named_kernel, grid, blk, 0, stream, k, label, label_off, n_labels, pieces, P, layout, names,
                           plan.contig_idx.as<u64>(), counts.as<u32>(), tail.as<u32>());
    else
        hipLaunchKernelGGL(piece_measure_kernel, grid, blk, 0, stream, k, label, label_off, n_labels, pieces, P, layout, first_contig,
                           plan.contig_idx.as<u64>(), counts.as<u32>(), tail.as<u32>());
    KCHECK_HIP(hipGetLastError());
    KCHECK(dev_scan_counts(counts.as<u32>(), P, plan.piece_off.as<u64>(), stream));
    u32 err = 0;
    KCHECK_HIP(hipMemcpyAsync(&plan.n_contigs, plan.contig_idx.as<u64>() + P, 8, hipMemcpyDeviceToHost, stream));
    KCHECK_HIP(hipMemcpyAsync(&plan.text_bytes, plan.piece_off.as<u64>() + P, 8, hipMemcpyDeviceToHost, stream));
    KCHECK_HIP(hipMemcpyAsync(&err, tail.p, 4, hipMemcpyDeviceToHost, stream));
    KCHECK_HIP(hipStreamSynchronize(stream));
    if (err) { plan.n_contigs = plan.text_bytes = 0; }
    KCHECK(check_plan_errors(err));
    if (first_contig > ~0ull - plan.n_contigs) {
        set_error("text: %llu contigs numbered from %llu on do not fit 64 bits", (unsigned long long)plan.n_contigs, (unsigned long long)first_contig);
        plan.n_contigs = plan.text_bytes = 0;
        return KATOME_E_UNSUPPORTED;
    }
    return KATOME_OK;
}

int dev_text_write(uint32_t k, const uint8_t* label, const uint64_t* label_off, const uint32_t* pieces, uint64_t n_pieces, uint32_t layout,
                   uint64_t first_contig, const TextPlan& plan, uint64_t* contig_off, uint32_t* contig_len, uint8_t* text, hipStream_t stream,
                   const uint64_t* names) {
    if (n_pieces == 0 || plan.text_bytes == 0) return KATOME_OK;
    const u64 P = n_pieces;
    const dim3 grid(grid_for(P, BLOCK, 256u * 32u)), blk(BLOCK);
    DevBuf tail(stream);
    KCHECK(tail.alloc(16));
    KCHECK_HIP(hipMemsetAsync(tail.p, 0, 16, stream));
    for (int lengths = 0; lengths < 2; ++lengths)
        if (names)
            hipLaunchKernelGGL(contig_bounds_named_kernel, grid, blk, 0, stream, pieces, P, layout, names, plan.contig_idx.as<u64>(), plan.piece_off.as<u64>(),
                               lengths, contig_off, contig_len, tail.as<u32>());
        else
            hipLaunchKernelGGL(contig_bounds_kernel, grid, blk, 0, stream, pieces, P, layout, first_contig, plan.contig_idx.as<u64>(), plan.piece_off.as<u64>(),
                               lengths, contig_off, contig_len, tail.as<u32>());
    KCHECK_HIP(hipGetLastError());
    u32 err = 0;
    KCHECK_HIP(hipMemcpyAsync(&err, tail.p, 4, hipMemcpyDeviceToHost, stream));
    KCHECK_HIP(hipStreamSynchronize(stream));
    KCHECK(check_plan_errors(err));
    const u64 tiles = (plan.text_bytes + TILE - 1) / TILE;
    if (names) {
        KernelScope ks(K_TEXT_WRITE_NAMED, stream, plan.text_bytes);
        hipLaunchKernelGGL(text_write_named_kernel, dim3(grid_for(tiles, 1, 256u * 16u)), blk, 0, stream, k, label, label_off, pieces, (u32)P, layout,
                           names, plan.contig_idx.as<u64>(), plan.piece_off.as<u64>(), plan.text_bytes, text);
        KCHECK_HIP(hipGetLastError());
    } else {
        KernelScope ks(K_TEXT_WRITE, stream, plan.text_bytes);
        hipLaunchKernelGGL(text_write_kernel, dim3(grid_for(tiles, 1, 256u * 16u)), blk, 0, stream, k, label, label_off, pieces, (u32)P, layout,
                           first_contig, plan.contig_idx.as<u64>(), plan.piece_off.as<u64>(), plan.text_bytes, text);
        KCHECK_HIP(hipGetLastError());
    }
    return KATOME_OK;
}

int dev_pieces_text(uint32_t k, const uint8_t* label, const uint64_t* label_off, uint64_t n_labels, const uint32_t* pieces, uint64_t n_pieces,
                    uint32_t layout, uint64_t first_contig, TextOutput& out, hipStream_t stream) {
    out.n_contigs = out.text_bytes = 0; out.layout = layout;
    TextPlan plan;
    KCHECK(dev_text_plan(k, label, label_off, n_labels, pieces, n_pieces, layout, first_contig, plan, stream));
    KCHECK(out.contig_off.alloc((plan.n_contigs + 1) * 8, stream)); KCHECK(out.contig_len.alloc((plan.n_contigs + 1) * 4, stream));
    KCHECK(out.text.alloc((plan.text_bytes + 15) / 16 * 16 + 16, stream));
    KCHECK(dev_text_write(k, label, label_off, pieces, n_pieces, layout, first_contig, plan, out.contig_off.as<u64>(), out.contig_len.as<u32>(),
                          out.text.as<uint8_t>(), stream));
    KCHECK_HIP(hipStreamSynchronize(stream));
    out.n_contigs = plan.n_contigs; out.text_bytes = plan.text_bytes;
    return KATOME_OK;
}

// collapse() of the graph `g`: the exact shrink (its result stays in `shrunk`: the pieces name its edges), the walk on the host, the
// text on the device.  lengths (optional): every contig's bases, known on the host after the walk from the shrunk edges' k-mer counts
int dev_collapse(const ShrinkInput& g, const uint32_t* edge_age, ShrinkOutput& shrunk, uint32_t layout, TextOutput& out,
                 katome_collapse_stats* stats, std::vector<uint64_t>* lengths, hipStream_t stream, DevBuf* keep_pieces, uint64_t* n_pieces) {
    katome_collapse_stats st;
    memset(&st, 0, sizeof st);
    out.n_contigs = out.text_bytes = 0; out.layout = layout;
    if (lengths) lengths->clear();
    if (layout > KATOME_TEXT_FASTA) { set_error("collapse: unknown layout %u", layout); return KATOME_E_ARG; }
    ShrinkExact sx;
    std::vector<uint32_t> kept;
    KCHECK(dev_shrink_exact(g, edge_age, shrunk, &st.shrink_host_ms, stream, &sx, &kept));
    const u64 H = shrunk.n_edges;
    st.shrunk_edges = H; st.shrunk_nodes = shrunk.n_nodes;
    if (H == 0) { if (stats) *stats = st; return KATOME_OK; }
    std::vector<uint32_t> weight, kmers, pieces;
    try { weight.resize(H); kmers.resize(H); }
    catch (const std::bad_alloc&) { set_error("collapse: out of host memory"); return KATOME_E_OOM; }
    KCHECK_HIP(hipMemcpyAsync(weight.data(), shrunk.edge_weight.p, H * 4, hipMemcpyDeviceToHost, stream));
    KCHECK_HIP(hipMemcpyAsync(kmers.data(), shrunk.edge_kmers.p, H * 4, hipMemcpyDeviceToHost, stream));
    KCHECK_HIP(hipStreamSynchronize(stream));
    for (u64 e = 0; e < H; ++e)
        if (weight[e] == 0) { set_error("collapse: edge %llu of the shrunk graph has weight 0 (the reference's decrement would wrap)", (unsigned long long)e); return KATOME_E_ARG; }
    const u64 P = CollapseExact::piece_count(weight.data(), (uint32_t)H);
    if (P >= 0x80000000ull) { set_error("collapse: the shrunk edges' weights add up to %llu pieces, at most 2^31 - 1", (unsigned long long)P); return KATOME_E_UNSUPPORTED; }
    try { pieces.resize(P); }
    catch (const std::bad_alloc&) { set_error("collapse: no host memory for %llu pieces", (unsigned long long)P); return KATOME_E_OOM; }
    CollapseExact walk(sx);
    const auto t0 = std::chrono::steady_clock::now();
    bool done = false;
    try {
        walk.prepare(kept, weight.data(), pieces.data(), P);
        done = walk.run();
    } catch (const std::bad_alloc&) { set_error("collapse: out of host memory"); return KATOME_E_OOM; }
    st.host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (!done || walk.n_pieces != P) {
        set_error("collapse: the walk emitted %llu pieces and left %u nodes, %u edges (the weights add up to %llu)", (unsigned long long)walk.n_pieces,
                  sx.n_nodes, sx.n_edges, (unsigned long long)P);
        return KATOME_E_DEVICE;
    }
    st.n_pieces = walk.n_pieces; st.n_contigs = walk.n_contigs; st.nodes_left = sx.n_nodes; st.edges_left = sx.n_edges;
    st.steps = walk.steps; st.ambiguity_cuts = walk.ambiguity_cuts; st.self_loops = walk.self_loops; st.simple_loops = walk.simple_loops;
    st.scc_restarts = walk.scc_restarts; st.nodes_removed = walk.nodes_removed; st.ambiguity_moves = walk.ambiguity_moves;
    {
        std::vector<uint64_t> own;
        std::vector<uint64_t>& len = lengths ? *lengths : own;
        try { len.reserve(walk.n_contigs); }
        catch (const std::bad_alloc&) { set_error("collapse: out of host memory"); return KATOME_E_OOM; }
        for (u64 p = 0; p < P; ++p) {
            const uint32_t w = pieces[p];
            if (w & WHOLE) len.push_back((u64)g.k - 1 + kmers[w & ~WHOLE]); else len.back() += kmers[w];
        }
        for (u64 i = 0; i < len.size(); ++i)
            if (len[i] > 0xFFFFFFFFull) { set_error("collapse: contig %llu has %llu bases, at most 2^32 - 1", (unsigned long long)i, (unsigned long long)len[i]); return KATOME_E_UNSUPPORTED; }
    }
    DevBuf d_pieces(stream);
    KCHECK(d_pieces.alloc(P * 4 + 16));
    const auto t1 = std::chrono::steady_clock::now();
    KCHECK_HIP(hipMemcpyAsync(d_pieces.p, pieces.data(), P * 4, hipMemcpyHostToDevice, stream));
    KCHECK(dev_pieces_text(g.k, shrunk.edge_label.as<uint8_t>(), shrunk.edge_label_off.as<u64>(), H, d_pieces.as<u32>(), P, layout, 0, out, stream));
    st.text_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
    if (out.n_contigs != walk.n_contigs) { set_error("collapse: the device counted %llu contigs, the walk %llu", (unsigned long long)out.n_contigs, (unsigned long long)walk.n_contigs); return KATOME_E_DEVICE; }
    if (keep_pieces) { keep_pieces->stream = stream; keep_pieces->adopt(d_pieces); }
    if (n_pieces) *n_pieces = P;
    if (stats) *stats = st;
    return KATOME_OK;
}

}  // namespace katome
