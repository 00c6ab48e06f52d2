// lds_order.h -- one group of distinct one-word keys put in key order in LDS by a workgroup of 1024 threads (the k-mer level's
// ordered count, lds_count.hip lds_count_ordered_kernel, and the merge of the reverse-complement groups, radix.hip group_merge_kernel).
#pragma once

#include "common.h"

namespace katome {

constexpr u32 LDS_ORDER_THREADS = 1024;
constexpr u32 LDS_ORDER_BUCKETS = 2 * LDS_ORDER_THREADS;      // (two 16-bit counters to a word, one word per thread in the scan)

// Every thread holds PER entries v[j] (those with bit j of keep set): remainder << 16 | 16-bit value, the remainders distinct within
// the group, so whole entries compare as their keys.  On return slot[0 .. total) holds them in ascending order; total (the kept
// entries of the whole workgroup) is returned to every thread, and on_total(total) has run on every thread between the bucket scan and
// the first write to slot (the count's cursor reservation).  bucket: LDS_ORDER_BUCKETS / 2 words, zero and visible to every thread on
// entry; wtot: LDS_ORDER_THREADS / 64 words.  bshift: the remainder's bits below its top 11 (buckets: those top 11 bits).
// A counting sort into 2048 buckets of 16-bit counters, then every key is placed by counting the keys of its bucket below it:
// independent reads of half a dozen entries at C3 -- an insertion sort per bucket instead was a chain of dependent LDS round trips that
// every wave waited out for its longest bucket, 62 % of the count kernel (profiles/r05_half_sort.md).
template <u32 PER, class OnTotal>
__device__ __forceinline__ u32 lds_order_entries(const unsigned long long (&v)[PER], u32 keep, unsigned long long* slot, u32* bucket,
                                                 u32* wtot, u32 bshift, OnTotal on_total) {
    static_assert(PER * LDS_ORDER_THREADS < (1u << 16), "a group must fit 16-bit bucket counters");
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // (2048 buckets of 16-bit counters, two to a word: a group holds fewer than 2^16 keys, so no half carries into the other)
#pragma unroll
    for (u32 j = 0; j < PER; ++j) {
        if (!((keep >> j) & 1u)) continue;
        const u32 b = (u32)((v[j] >> 16) >> bshift);
        atomicAdd(&bucket[b >> 1], 1u << ((b & 1u) * 16u));
    }
    __syncthreads();
    const u32 pair = bucket[tid], lo_cnt = pair & 0xFFFFu, cnt = lo_cnt + (pair >> 16);
    u32 incl = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { u32 t = __shfl_up(incl, o, 64); if (lane >= (u32)o) incl += t; }
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    u32 woff = 0, total = 0;
#pragma unroll
    for (u32 w = 0; w < LDS_ORDER_THREADS / 64; ++w) { if (w < wave) woff += wtot[w]; total += wtot[w]; }
    const u32 start = woff + incl - cnt;
    bucket[tid] = start | ((start + lo_cnt) << 16);
    on_total(total);
    __syncthreads();
#pragma unroll
    for (u32 j = 0; j < PER; ++j) {
        if (!((keep >> j) & 1u)) continue;
        const u32 b = (u32)((v[j] >> 16) >> bshift), sh = (b & 1u) * 16u;
        slot[(atomicAdd(&bucket[b >> 1], 1u << sh) >> sh) & 0xFFFFu] = v[j];
    }
    __syncthreads();
    // bucket b now spans [end(b - 1), end(b)): a key's place is its bucket's start plus the keys of its bucket below it
    u32 pos[PER];
#pragma unroll
    for (u32 j = 0; j < PER; ++j) {
        pos[j] = 0;
        if (!((keep >> j) & 1u)) continue;
        const u32 b = (u32)((v[j] >> 16) >> bshift), e = (bucket[b >> 1] >> ((b & 1u) * 16u)) & 0xFFFFu;
        u32 r = b ? (bucket[(b - 1) >> 1] >> (((b - 1) & 1u) * 16u)) & 0xFFFFu : 0u;
        const u32 s0 = r;
#pragma unroll 4
        for (u32 i = s0; i < e; ++i) r += slot[i] < v[j] ? 1u : 0u;
        pos[j] = r;
    }
    __syncthreads();
#pragma unroll
    for (u32 j = 0; j < PER; ++j) if ((keep >> j) & 1u) slot[pos[j]] = v[j];
    __syncthreads();
    return total;
}

}  // namespace katome
