// lds_order.h -- one group of distinct one-word keys put in key order in LDS by a workgroup of 1024 threads (the k-mer level's
// ordered count, lds_count.hip lds_count_ordered_kernel, and the merge of the reverse-complement groups, radix.hip group_merge_kernel).
#pragma once

#include "common.h"

namespace katome {

constexpr u32 LDS_ORDER_THREADS = 1024;
constexpr u32 LDS_ORDER_COARSE_BITS = 11, LDS_ORDER_FINE_BITS = 13;   // buckets: 2048 (one counter word per thread) or 8192 (four)
// the bucket words of a call: two 16-bit counters to a word, and one word behind them for the end of the last bucket
constexpr u32 lds_order_words(u32 bucket_bits) { return (1u << bucket_bits) / 2 + 1; }
// entries looked at with one wait in the rank step before the loop over the rest of a long bucket (a fine bucket holds 1.5 at C3)
constexpr u32 LDS_ORDER_RANK_UNROLL = 4;

// Every thread holds PER entries v[j] (those with bit j of keep set): remainder << 16 | 16-bit value, the remainders distinct within
// the group, so whole entries compare as their keys.  On return slot[0 .. total) holds them in ascending order; total (the kept
// entries of the whole workgroup) is returned to every thread, and on_total(total) has run on every thread between the bucket scan and
// the first write to slot (the count's cursor reservation).  bucket: lds_order_words(BB) words, 16-byte aligned, all but the last zero
// and visible to every thread on entry, and outside slot[0 .. total); wtot: LDS_ORDER_THREADS / 64 words.  bshift: the remainder's bits
// below its top BB (buckets: those top BB bits; a remainder of fewer bits fills the low buckets only).
// A counting sort into 2^BB buckets of 16-bit counters:
//   count   one LDS atomic per entry, whose return value is the entry's arrival index within its bucket (kept, two to a register);
//   scan    the counters become the buckets' starts (a group holds fewer than 2^16 entries, so no half carries into the other);
//   place   entry -> slot[start + arrival]: the buckets in order, the entries of one bucket in no order;
//   rank    thread by slot position, not by its own entries: the entry at position i belongs at its bucket's start plus the number
//           of smaller entries in its bucket.  A wave's lanes read neighbouring buckets; LDS_ORDER_RANK_UNROLL entries are read
//           without a wait in between (positions past the bucket's end read the entry itself, which counts nothing), a longer
//           bucket goes on in a loop.  At most PER positions to a thread since total <= PER * LDS_ORDER_THREADS;
//   write   the entries to their places.
// Earlier forms (profiles/r14_lds_order.md): 2048 buckets, a second returning atomic per entry to place it and a rank loop per
// thread's own entries, which every wave ran for the longest of 64 unrelated buckets of 6 entries (rounds 5 to 13); an insertion sort
// per bucket, a chain of dependent LDS round trips, 62 % of the count kernel (profiles/r05_half_sort.md).
// stamp(i), i = 0 .. 4, runs after count, scan, place, rank and write (phase clocks of experiment builds; nothing when shipped).
template <u32 PER, u32 BB, class OnTotal, class Stamp>
__device__ __forceinline__ u32 lds_order_entries(const unsigned long long (&v)[PER], u32 keep, unsigned long long* slot, u32* bucket,
                                                 u32* wtot, u32 bshift, OnTotal on_total, Stamp stamp) {
    static_assert(PER * LDS_ORDER_THREADS < (1u << 16), "a group must fit 16-bit bucket counters");
    constexpr u32 NBW = (1u << BB) / 2, WPT = NBW / LDS_ORDER_THREADS;          // counter words, and those one thread scans
    static_assert(WPT == 1 || WPT == 4, "one word or one 16-byte read per thread in the scan");
    // (the thread's index through an empty asm: what is worked out from it -- the scan's lane addresses and wave masks, the rank step's
    // positions -- would otherwise be hoisted out of the caller's loop over the groups and held in registers throughout the kernel:
    // 12 to 18 VGPRs spilled to scratch in every instantiation with hipcc 7.2.  Nothing in the build fails if a later compiler hoists
    // them again: after a compiler change check both kernels with tools/kernel_regs.py -- no scratch, no VGPR spill)
    u32 tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const u32 lane = tid & 63, wave = tid >> 6;
    // count: arrival indices, 16 bits each
    u32 arr[(PER + 1) / 2];
#pragma unroll
    for (u32 j = 0; j < (PER + 1) / 2; ++j) arr[j] = 0;
#pragma unroll
    for (u32 j = 0; j < PER; ++j) {
        if (!((keep >> j) & 1u)) continue;
        const u32 b = (u32)((v[j] >> 16) >> bshift), sh = (b & 1u) * 16u;
        arr[j >> 1] |= ((atomicAdd(&bucket[b >> 1], 1u << sh) >> sh) & 0xFFFFu) << ((j & 1u) * 16u);
    }
    __syncthreads();
    stamp(0);
    // scan: this thread's WPT words, 2 WPT buckets
    u32 cw[WPT];
    if (WPT == 4) { const uint4 q = reinterpret_cast<const uint4*>(bucket)[tid]; cw[0] = q.x; cw[1 % WPT] = q.y; cw[2 % WPT] = q.z; cw[3 % WPT] = q.w; }
    else cw[0] = bucket[tid];
    u32 cnt = 0;
#pragma unroll
    for (u32 q = 0; q < WPT; ++q) cnt += (cw[q] & 0xFFFFu) + (cw[q] >> 16);
    u32 incl = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { u32 t = __shfl_up(incl, o, 64); if (lane >= (u32)o) incl += t; }
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    u32 woff = 0, total = 0;
#pragma unroll
    for (u32 w = 0; w < LDS_ORDER_THREADS / 64; ++w) { if (w < wave) woff += wtot[w]; total += wtot[w]; }
    u32 start = woff + incl - cnt;
#pragma unroll
    for (u32 q = 0; q < WPT; ++q) {
        const u32 lo_cnt = cw[q] & 0xFFFFu, hi_cnt = cw[q] >> 16;
        cw[q] = start | ((start + lo_cnt) << 16);
        start += lo_cnt + hi_cnt;
    }
    if (WPT == 4) reinterpret_cast<uint4*>(bucket)[tid] = make_uint4(cw[0], cw[1 % WPT], cw[2 % WPT], cw[3 % WPT]);
    else bucket[tid] = cw[0];
    if (tid == 0) bucket[NBW] = total | (total << 16);       // (the last bucket's end, read as the start of the bucket behind it)
    on_total(total);
    __syncthreads();
    stamp(1);
    // place
#pragma unroll
    for (u32 j = 0; j < PER; ++j) {
        if (!((keep >> j) & 1u)) continue;
        const u32 b = (u32)((v[j] >> 16) >> bshift);
        slot[((bucket[b >> 1] >> ((b & 1u) * 16u)) & 0xFFFFu) + ((arr[j >> 1] >> ((j & 1u) * 16u)) & 0xFFFFu)] = v[j];
    }
    __syncthreads();
    stamp(2);
    // rank: position tid + t * 1024
    unsigned long long e[PER];
#pragma unroll
    for (u32 j = 0; j < (PER + 1) / 2; ++j) arr[j] = 0;       // (now the entries' places, 16 bits each)
#pragma unroll
    for (u32 t = 0; t < PER; ++t) {
        const u32 i = tid + t * LDS_ORDER_THREADS;
        e[t] = 0;
        if (i >= total) continue;
        e[t] = slot[i];
        const u32 b = (u32)((e[t] >> 16) >> bshift);
        const unsigned long long two = (unsigned long long)bucket[b >> 1] | ((unsigned long long)bucket[(b >> 1) + 1] << 32);
        const u32 s = (u32)(two >> ((b & 1u) * 16u)) & 0xFFFFu, en = (u32)(two >> ((b & 1u) * 16u + 16u)) & 0xFFFFu;
        u32 r = s;
#pragma unroll
        for (u32 u = 0; u < LDS_ORDER_RANK_UNROLL; ++u) r += slot[s + u < en ? s + u : i] < e[t] ? 1u : 0u;
        for (u32 q = s + LDS_ORDER_RANK_UNROLL; q < en; ++q) r += slot[q] < e[t] ? 1u : 0u;
        arr[t >> 1] |= r << ((t & 1u) * 16u);
    }
    __syncthreads();
    stamp(3);
#pragma unroll
    for (u32 t = 0; t < PER; ++t) if (tid + t * LDS_ORDER_THREADS < total) slot[(arr[t >> 1] >> ((t & 1u) * 16u)) & 0xFFFFu] = e[t];
    __syncthreads();
    stamp(4);
    return total;
}

}  // namespace katome
