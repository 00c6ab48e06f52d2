// Host build of katome_amd/csrc/counted_key.h: a two-word record with its count in the free bits of its first word
// (tests/test_counted_key_host.py asks through ctypes).
#include <stdint.h>

#include "../../katome_amd/csrc/counted_key.h"

using namespace katome;

extern "C" {
int hs_counted_fits(uint32_t bases) { return counted_fits(bases) ? 1 : 0; }
uint64_t hs_hash_key2(const uint64_t* plain) { Key<2> k; k.w[0] = plain[0]; k.w[1] = plain[1]; return hash_key(k); }
void hs_counted_pack(const uint64_t* plain, uint32_t count, uint64_t* packed) {
    Key<2> k; k.w[0] = plain[0]; k.w[1] = plain[1];
    const Key<2> p = counted_pack(k, count);
    packed[0] = p.w[0]; packed[1] = p.w[1];
}
// out: plain w[0], plain w[1], count, hash_key of the plain key taken back out
void hs_counted_fields(const uint64_t* packed, uint64_t* out) {
    Key<2> p; p.w[0] = packed[0]; p.w[1] = packed[1];
    const Key<2> k = counted_plain(p);
    out[0] = k.w[0]; out[1] = k.w[1]; out[2] = counted_count(p); out[3] = hash_key(k);
}
}
