// strand_bits.h -- the bit work of gfa_strands.hip, plain enough for a host build (tests/hostshim/strand_bits_host.cpp): bases cut out
// of a 2-bit label at any alignment, a segment's two end k-mers as sort keys, one 16-base word of the comparison of a segment with
// the reverse complement of another, and the rule that picks a link's canonical spelling.
#pragma once
#include <stdint.h>

#include "kmer_bits.h"

namespace katome {

constexpr u32 NO_TWIN = 0xFFFFFFFFu;

// nb (1 .. 16) bases of a label's packed bases (first base in the top bits of a byte) from base b on, in the top 2 * nb bits; the bits
// below are not defined.  Only the aligned 32-bit words that hold a needed byte are read: the second one where the bits reach into it.
KD u32 label_bits(const uint8_t* src, u32 b, u32 nb) {
    const uintptr_t a = (uintptr_t)(src + (b >> 2));
    const uintptr_t a0 = a & ~(uintptr_t)3;
    const u32 s = 8 * (u32)(a - a0) + 2 * (b & 3);                           // 0 .. 30
    u32 v = __builtin_bswap32(*(const u32*)a0) << s;
    if (s + 2 * nb > 32) v |= __builtin_bswap32(*(const u32*)(a0 + 4)) >> (32 - s);      // (s != 0 here)
    return v;
}
// 16 bases in the opposite order: pairs of 2-bit groups, of nibbles, then the bytes
KD u32 reverse_bases(u32 x) {
    x = ((x >> 2) & 0x33333333u) | ((x & 0x33333333u) << 2);
    x = ((x >> 4) & 0x0F0F0F0Fu) | ((x & 0x0F0F0F0Fu) << 4);
    return __builtin_bswap32(x);
}
KD u32 top_bases_mask(u32 nb) { return 0xFFFFFFFFu << (32 - 2 * nb); }      // nb = 1 .. 16

KD void key_push(Key<2>& key, u32 v, u32 nb) {                                // nb more bases at the low end
    const u32 sh = 2 * nb;                                                   // 2 .. 32
    key.w[0] = (key.w[0] << sh) | (key.w[1] >> (64 - sh));
    key.w[1] = (key.w[1] << sh) | v;
}
// the k-mer at bases [0, k) of a label, right-aligned (w[0] the high word)
KD Key<2> first_kmer(const uint8_t* src, u32 k) {
    Key<2> key; key.w[0] = key.w[1] = 0;
    for (u32 c = 0; c < k; c += 16) {
        const u32 nb = k - c < 16 ? k - c : 16;
        key_push(key, label_bits(src, c, nb) >> (32 - 2 * nb), nb);
    }
    return key;
}
// the reverse complement of the k-mer at bases [n - k, n): the last bases first, complemented
KD Key<2> last_kmer_revcomp(const uint8_t* src, u32 n, u32 k) {
    Key<2> key; key.w[0] = key.w[1] = 0;
    for (u32 c = 0; c < k; c += 16) {
        const u32 nb = k - c < 16 ? k - c : 16;
        const u32 y = reverse_bases(label_bits(src, n - c - nb, nb) & top_bases_mask(nb));      // the nb bases, in the low bits
        key_push(key, ~y & (0xFFFFFFFFu >> (32 - 2 * nb)), nb);
    }
    return key;
}
// bases [at, at + 16) of an n-base text_i (at a multiple of 16, fewer at the end) against the complement of text_j read backward:
// true where one of them differs
KD bool twin_word_differs(const uint8_t* src_i, const uint8_t* src_j, u32 n, u32 at) {
    const u32 nb = n - at < 16 ? n - at : 16;
    const u32 fwd = label_bits(src_i, at, nb);
    const u32 back = reverse_bases(label_bits(src_j, n - at - nb, nb) & top_bases_mask(nb));
    return ((fwd ^ ~(back << (32 - 2 * nb))) & top_bases_mask(nb)) != 0;
}

// The link (a, b) of two merged edges whose twins are ta, tb (NO_TWIN: none) as two fields f = 2 * segment + (orientation == '-'):
// it spells (rep a, o a, rep b, o b), its conjugate (rep b, flip o b, rep a, flip o a) -- flip leaves a self-twin at +; a segment
// without a twin is flipped like a paired one -- and the smaller spelling under (x, ox, y, oy), + < -, is the one that is written
KD void canonical_link(u32 a, u32 b, u32 ta, u32 tb, u64& fx, u64& fy) {
    const u64 fa = ta < a ? 2ull * ta + 1 : 2ull * a, fb = tb < b ? 2ull * tb + 1 : 2ull * b;
    const u64 ca = ta == a ? fa : fa ^ 1, cb = tb == b ? fb : fb ^ 1;
    const bool conj = cb < fa || (cb == fa && ca < fb);
    fx = conj ? cb : fa; fy = conj ? ca : fb;
}

}  // namespace katome
