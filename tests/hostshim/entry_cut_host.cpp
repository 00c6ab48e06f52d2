// Host build of katome_amd/csrc/entry_cut.h: the records of one list entry cut together, beside the per-record expression of
// kmer_bits.h they must equal bit for bit (tests/test_entry_cut_host.py asks both through ctypes and compares).
#include <stdint.h>

#include "../../katome_amd/csrc/entry_cut.h"

using namespace katome;

template <int NWT, int NWK, bool RC, bool REP>
static void cut_t(const uint64_t* tile_words, uint32_t sub_len, uint32_t span, uint32_t stride, uint64_t* by_entry, uint64_t* by_record) {
    Key<NWT> tile;
    for (int w = 0; w < NWT; ++w) tile.w[w] = tile_words[w];
    const EntryCut<NWT, NWK, RC, REP> cut(tile, sub_len, span, stride);
    for (uint32_t o = 0; o < span; ++o) {
        const Key<NWK> a = cut.record(o);
        const Key<NWK> b = level_orientation<NWK, RC, REP>(sub_window<NWT, NWK>(tile, sub_len, span, stride, o), sub_len);
        for (int w = 0; w < NWK; ++w) { by_entry[o * NWK + w] = a.w[w]; by_record[o * NWK + w] = b.w[w]; }
    }
}
template <int NWT, int NWK>
static int cut_form(const uint64_t* t, uint32_t sub_len, uint32_t span, uint32_t stride, int rc, int rep, uint64_t* e, uint64_t* r) {
    if (rep) {
        if constexpr (NWK == 1) { if (rc) cut_t<NWT, 1, true, true>(t, sub_len, span, stride, e, r); else cut_t<NWT, 1, false, true>(t, sub_len, span, stride, e, r); return 0; }
        return 1;
    }
    if (rc) cut_t<NWT, NWK, true, false>(t, sub_len, span, stride, e, r); else cut_t<NWT, NWK, false, false>(t, sub_len, span, stride, e, r);
    return 0;
}

extern "C" {
// the span records of `tile` (nwt words) as nwk-word keys: by_entry from EntryCut, by_record from level_orientation(sub_window(.));
// 0, or 1 for a form that does not exist
int hs_entry_cut(const uint64_t* tile, int nwt, int nwk, uint32_t sub_len, uint32_t span, uint32_t stride, int rc, int rep, uint64_t* by_entry, uint64_t* by_record) {
    if (nwt == 2 && nwk == 2) return cut_form<2, 2>(tile, sub_len, span, stride, rc, rep, by_entry, by_record);
    if (nwt == 2 && nwk == 1) return cut_form<2, 1>(tile, sub_len, span, stride, rc, rep, by_entry, by_record);
    if (nwt == 1 && nwk == 1) return cut_form<1, 1>(tile, sub_len, span, stride, rc, rep, by_entry, by_record);
    return 1;
}
}
