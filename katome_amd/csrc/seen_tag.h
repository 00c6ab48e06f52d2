// seen_tag.h -- the delta tag of a first-seen build's tagged records: the record's two sequence numbers themselves, packed into one
// word.  Host-compilable, as kmer_bits.h is (tests/hostshim/seen_tag_host.cpp checks it without a GPU).
//
// A record of such a build has two numbers: P, the first insertion of its stored orientation, and Q, that of its reverse complement.
// Both lie in the range [base_r, base_r + 2 W_r) of one read r (seq_pair.h), and the ranges of different reads are disjoint and
// ascending.  So the smallest P and the smallest Q of a key both come from the first read that holds it on either strand, and
// |Q - P| < 2 W_r holds for a record and for the two minima of a key alike:
//
//     delta tag = P << 17 | (Q - P + 65536)          P < 2^47, |Q - P| < 65536
//
// One strand only: Q = P.  Nothing in the tag names a read, so reads of any lengths pack as long as none has more than 32767
// windows.  (Reads of one length keep slot_bits.h's seen_pack: read << 32 | offset << 16 | offset.)
#pragma once
#include "kmer_bits.h"

namespace katome {

constexpr u64 DELTA_BIAS = 65536;            // |Q - P| stays below this
constexpr u32 DELTA_SHIFT = 17;              // Q - P + DELTA_BIAS takes 17 bits
constexpr u64 DELTA_P_LIMIT = 1ull << 47;    // P stays below this
constexpr u32 DELTA_MAX_WINDOWS = 32767;     // a read of at most this many windows packs wherever its records lie in it (|Q - P| < 2 W)

KD bool delta_packs(u64 P, u64 Q) { return P < DELTA_P_LIMIT && (Q >= P ? Q - P : P - Q) < DELTA_BIAS; }
KD u64 delta_pack(u64 P, u64 Q) { return P << DELTA_SHIFT | (Q - P + DELTA_BIAS); }       // (for numbers that pack: delta_packs)
KD u64 delta_p(u64 tag) { return tag >> DELTA_SHIFT; }
KD u64 delta_q(u64 tag) { return (tag >> DELTA_SHIFT) + (tag & ((1ull << DELTA_SHIFT) - 1)) - DELTA_BIAS; }
// the record in its other orientation (canonical_flip exchanged the two): P and Q swap
KD u64 delta_swap(u64 tag) { return delta_pack(delta_q(tag), delta_p(tag)); }
// Sub-window o of a tile of n_sub sub-windows, `stride` windows apart (expand_tiles_kernel's rule): it went in at P + o * stride, and
// the tile's reverse complement holds its reverse complement as sub-window n_sub - 1 - o, at Q + (n_sub - 1 - o) * stride
KD void delta_sub(u64 P, u64 Q, u32 o, u32 n_sub, u32 stride, u64& Ps, u64& Qs) {
    Ps = P + (u64)o * stride; Qs = Q + (u64)(n_sub - 1 - o) * stride;
}

}  // namespace katome
