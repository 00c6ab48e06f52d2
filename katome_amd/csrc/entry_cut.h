// entry_cut.h -- the records of one list entry, cut together (host and device: tests/hostshim/entry_cut_host.cpp checks it against
// the per-record expression without a GPU).
//
// A list entry is a tile of sub_len + stride * (span - 1) bases and yields span records: record o is
//     level_orientation<NWK, RC, REP>(sub_window<NWT, NWK>(tile, sub_len, span, stride, o), sub_len)            (kmer_bits.h)
// Taken record by record that is a reverse complement per record.  Taken per entry it is ONE: the reverse complement of sub-window o
// is sub-window span - 1 - o of the tile's reverse complement, i.e. the low 2 * sub_len bits of rc(tile) >> 2 * stride * o, so
//     canonical        is the smaller of two cuts (equal cuts: the same record either way),
//     rep_orientation  is a choice between them by bit sub_len of the forward cut,
// and with one strand only the forward cut is made.  The shifts are the same for every entry (they depend on o alone), so a kernel
// whose threads walk o together shifts by scalar amounts and its branches on them do not diverge.
// revcomp() drops whatever lies above the tile's 2 * bases bits and the cuts keep 2 * sub_len bits below them: set bits above the tile
// in its top word change nothing, as they change nothing in sub_window().
#pragma once
#include "kmer_bits.h"

namespace katome {

template <int NWT, int NWK, bool RC, bool REP> struct EntryCut {
    static_assert(!REP || NWK == 1, "the representative orientation is one of one-word k-mers");
    Key<NWT> fwd, rev;          // the tile, and (RC) its reverse complement
    u32 bits, step, top;        // 2 * sub_len; 2 * stride; step * (span - 1)
    KD EntryCut(const Key<NWT>& tile, u32 sub_len, u32 span, u32 stride) : fwd(tile), rev(tile), bits(2 * sub_len), step(2 * stride), top(2 * stride * (span - 1)) {
        if (RC) rev = revcomp(tile, sub_len + stride * (span - 1));
    }
    KD Key<NWK> forward(u32 o) const { return narrow_key(key_low_bits(key_shr(fwd, top - step * o), bits), (Key<NWK>*)nullptr); }
    KD Key<NWK> reverse(u32 o) const { return narrow_key(key_low_bits(key_shr(rev, step * o), bits), (Key<NWK>*)nullptr); }
    // record o of the entry, o < span
    KD Key<NWK> record(u32 o) const {
        const Key<NWK> f = forward(o);
        if (!RC) return f;
        const Key<NWK> r = reverse(o);
        if (REP) return ((f.w[0] >> (bits >> 1)) & 1ull) ? r : f;
        return key_lt(r, f) ? r : f;
    }
};

}  // namespace katome
