// counted_key.h -- a two-word record that carries its count in the free bits of its first word (host and device:
// tests/hostshim/counted_key_host.cpp checks it without a GPU).
//
// A record of `bases` bases, 65 <= 2 * bases <= 78, uses hb = 2 * bases - 64 bits of w[0]; the table flags (OCC, RC_MARK) take its two
// top bits.  Between them lie 48 bits, 32 of which hold what the partition passes would otherwise move in an array of its own:
//
//     w[1]                    the key's low 64 bits, unchanged
//     w[0]  bits  0 .. 13     the key's top hb bits (the rest of the 14 clear)
//           bits 14 .. 29     clear (the top 16 bits of the key's hash rode here in an experiment: profiles/count_in_key.md)
//           bits 30 .. 61     the count, a whole u32: nothing saturates
//           bits 62, 63       clear
//
// A level whose records fit (counted_fits) moves them as keys alone -- 16 bytes, no weights array.
#pragma once
#include "kmer_bits.h"

namespace katome {

constexpr u32 COUNTED_KEY_BITS = 14, COUNTED_COUNT_SHIFT = 30, COUNTED_COUNT_BITS = 32;
static_assert(COUNTED_KEY_BITS <= COUNTED_COUNT_SHIFT, "the key's bits end below the count");
static_assert(COUNTED_COUNT_SHIFT + COUNTED_COUNT_BITS <= 62, "the count ends below RC_MARK and OCC");

// the one predicate every caller asks: records of `bases` bases are two words wide and leave the count its room (33 .. 39 bases)
KD bool counted_fits(u32 bases) { return 2 * bases > 64 && 2 * bases - 64 <= COUNTED_KEY_BITS; }

// plain: a record of a fitting width, nothing set above its bits
KD Key<2> counted_pack(const Key<2>& plain, u32 count) {
    Key<2> p;
    p.w[0] = plain.w[0] | ((u64)count << COUNTED_COUNT_SHIFT);
    p.w[1] = plain.w[1];
    return p;
}
KD u64 counted_plain_word(u64 w0) { return w0 & ((1ull << COUNTED_KEY_BITS) - 1); }
KD Key<2> counted_plain(const Key<2>& packed) { Key<2> k; k.w[0] = counted_plain_word(packed.w[0]); k.w[1] = packed.w[1]; return k; }
KD u32 counted_count_word(u64 w0) { return (u32)(w0 >> COUNTED_COUNT_SHIFT); }          // (bits 62 and 63 are clear)
KD u32 counted_count(const Key<2>& packed) { return counted_count_word(packed.w[0]); }

}  // namespace katome
