// slot_bits.h -- what the table in HBM (table.hip) and the counting tables in LDS (lds_count.hip) both spell: a slot's flag bits and
// the packed pair of sequence numbers in a first-seen build's tagged records -- seen_pack for reads of one length, the delta tag of
// seen_tag.h for reads of varying length (the kernels that read a tag take the format as a template parameter, DELTA).
#pragma once
#include "common.h"
#include "seen_tag.h"

namespace katome {
constexpr u64 OCC = 1ull << 63;    // slot holds a published key
constexpr u64 LOCK = 1ull << 62;   // NW=2 only: high word claimed, low word not yet visible
constexpr u64 KEYBITS = ~(OCC | LOCK);
constexpr unsigned long long SEEN_NONE = ~0ull;
__device__ __forceinline__ unsigned long long seen_pack(u64 read, u32 a, u32 b) { return read << 32 | (unsigned long long)a << 16 | b; }
}  // namespace katome
