// edge_keys.h -- device helpers shared by the files that walk key arrays (radix.hip, node_ids.hip, first_seen.hip): loads and
// stores of one-, two- and three-word keys, the workgroup scan and tile size of the run-head counts, and the marks the target merge
// leaves in edge_dst for the first-seen renumbering.
#pragma once
#include "common.h"

namespace katome {

template <int NW> __device__ __forceinline__ Key<NW> load_key(const u64* p, u64 i) {
    Key<NW> k;
    if (NW == 1) { k.w[0] = p[i]; }
    else if (NW == 2) { ulonglong2 v = *reinterpret_cast<const ulonglong2*>(p + 2 * i); k.w[0] = v.x; k.w[NW - 1] = v.y; }
    else { k.w[0] = p[3 * i]; k.w[NW > 2 ? 1 : 0] = p[3 * i + 1]; k.w[NW - 1] = p[3 * i + 2]; }      // three-word tiles (64..95 bases)
    return k;
}
// the same load for data that is read once and not again by this kernel (a pass's input): non-temporal, so that the L2 lines it
// would take stay with the partial output lines that consecutive tiles complete (radix_scatter_kernel: 42.0 -> 40.5 ms per edge sort)
typedef unsigned long long u64x2_t __attribute__((ext_vector_type(2)));
#ifndef KATOME_STREAM_LOADS
#define KATOME_STREAM_LOADS 1        // 0: plain loads; 1: the scatter pass; 2: + histogram; 3: + run sort
#endif
template <int NW> __device__ __forceinline__ Key<NW> load_key_stream(const u64* p, u64 i) {
    Key<NW> k;
    if (NW == 1) { k.w[0] = __builtin_nontemporal_load(p + i); }
    else if (NW == 2) { u64x2_t v = __builtin_nontemporal_load(reinterpret_cast<const u64x2_t*>(p + 2 * i)); k.w[0] = v.x; k.w[NW - 1] = v.y; }
    else { k.w[0] = __builtin_nontemporal_load(p + 3 * i); k.w[NW > 2 ? 1 : 0] = __builtin_nontemporal_load(p + 3 * i + 1); k.w[NW - 1] = __builtin_nontemporal_load(p + 3 * i + 2); }
    return k;
}
template <int NW> __device__ __forceinline__ void store_key(u64* p, u64 i, const Key<NW>& k) {
    if (NW == 1) p[i] = k.w[0];
    else if (NW == 2) *reinterpret_cast<ulonglong2*>(p + 2 * i) = make_ulonglong2(k.w[0], k.w[NW - 1]);
    else { p[3 * i] = k.w[0]; p[3 * i + 1] = k.w[NW > 2 ? 1 : 0]; p[3 * i + 2] = k.w[NW - 1]; }
}

// run heads are counted per tile of UNIQ_TILE keys (dev_unique; the source ids of node_ids.hip, whose blocks the group merge of
// radix.hip counts ahead: SRC_HEAD_BLOCK there)
constexpr int UNIQ_ITEMS = 8;
constexpr int UNIQ_TILE = BLOCK * UNIQ_ITEMS;

__device__ __forceinline__ u32 block_excl_scan(u32 mine, u32* wsum /*[BLOCK/64]*/, u32& total) {
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u32 incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { u32 v = __shfl_up(incl, o, 64); if (lane >= (u32)o) incl += v; }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    u32 woff = 0; total = 0;
#pragma unroll
    for (int w = 0; w < BLOCK / 64; ++w) { if (w < (int)wave) woff += wsum[w]; total += wsum[w]; }
    __syncthreads();
    return woff + incl - mine;
}

// bucket of a key in an index over its top B bits (bucket_index_kernel, radix.hip)
template <int NW> __device__ __forceinline__ u32 top_bits(const Key<NW>& k, u32 key_bits, u32 B) { return key_digit(k, key_bits - B, B); }

// an edge whose source (k-1)-mer (key >> 2) differs from the edge before: the first out-edge of a node (src_count_kernel, node_ids.hip;
// group_merge_kernel, radix.hip, counts the same heads on the way)
template <int NW> __device__ __forceinline__ bool is_src_head(const u64* keys, u64 i) {
    return i == 0 || !key_eq(key_shr(load_key<NW>(keys, i), 2), key_shr(load_key<NW>(keys, i - 1), 2));
}

// marks in edge_dst, set by dst_merge_kernel (node_ids.hip) and read by pack_edges_intro_kernel (first_seen.hip)
constexpr u64 DST_IN1 = 1ull << 40;                      // first-seen order: mark in edge_dst, "the target has this in-edge only"
constexpr u64 DST_FD = 1ull << 41;                       // ... and "this edge is the first to touch its target" (it introduces the node)
constexpr u64 DST_MARKS = DST_IN1 | DST_FD;

}  // namespace katome
