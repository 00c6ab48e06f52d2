// lds_count.hip -- a level counted by sorting (gfx950): its records, cut into 65536 groups by radix.hip, are counted group by group in LDS
// tables and leave as oriented edges or as the list of distinct keys.  The kernels, one per slot shape, and the host code that picks one
// for a level (records_to_edges_sorted, tagged_records_sorted; sizes and planning arithmetic: lds_plan.h).  The table in HBM: table.hip.
#include <algorithm>
#include <vector>

#include "common.h"
#include "counted_key.h"
#include "lds_order.h"
#include "lds_plan.h"
#include "s2_regions.h"
#include "slot_bits.h"

namespace katome {

// ---------------------------------------------------------------------------------------------
// The last level without device-scope atomics.  The (k-mer, count) records of the distinct tiles are ordered by the top 16
// bits of their hash (two stable 8-bit passes of radix.hip, HashDigit), which cuts them into 65536 groups; a workgroup takes a
// group and counts it in an LDS table -- compare-and-swap and add in LDS --, in R sub-rounds by the next hash bits so that a
// sub-round's keys fit the table even if every record were a new key (nothing can overflow), re-reading the group from
// L2 / Infinity Cache; a sub-round's keys leave as oriented edges straight away (both strands, the remove_weak_edges
// threshold), as one contiguous stretch behind a cursor.
// ---------------------------------------------------------------------------------------------
// (-DKATOME_LC_PHASES: an experiment build that adds up, per phase of the two counting kernels, the shader clocks thread 0 of every
// workgroup sees go by -- tools/lc_phases.py reads them through katome_debug_lc_phases; never defined in the shipped library.
// 4 .. 7: the ordered kernel's REGIONS write phase -- S1 and the entries into registers, the digit count, scan and reservation, the
// reorder; the stream-out is what is left of phase 15)
#ifdef KATOME_LC_PHASES
__device__ unsigned long long lc_phase_cycles[16];
#define LC_PHASE_BEGIN() unsigned long long lc_t0 = clock64()
#define LC_PHASE(i) do { if (threadIdx.x == 0) { const unsigned long long lc_t = clock64(); atomicAdd(&lc_phase_cycles[i], lc_t - lc_t0); lc_t0 = lc_t; } } while (0)
// (the ordered kernel's phase 14 once more, step by step: the kept count and lds_order.h's count, scan, place, rank and write --
// katome_debug_lo_phases, tools/lds_order_phases.py)
__device__ unsigned long long lo_phase_cycles[8];
#define LO_PHASE_BEGIN() unsigned long long lo_t0 = clock64()
#define LO_PHASE(i) do { if (threadIdx.x == 0) { const unsigned long long lo_t = clock64(); atomicAdd(&lo_phase_cycles[i], lo_t - lo_t0); lo_t0 = lo_t; } } while (0)
#else
#define LC_PHASE_BEGIN() do {} while (0)
#define LC_PHASE(i) do {} while (0)
#define LO_PHASE_BEGIN() do {} while (0)
#define LO_PHASE(i) do {} while (0)
#endif
// LDS table: 8 B key + 4 B count per slot, LC_THREADS x PER slots (every thread reads PER slots out).  PER = 13: 13312 slots =
// 156 KiB of the CU's 160 (one workgroup of 1024 per CU either way): groups of 22 k records (2^16 groups at C3) go through in 3
// sub-rounds instead of the 4 a table of 8192 needs.  PER = 8: groups of 5.5 k records (2^18 groups: the look-back passes of
// radix.hip) fit an 8192-slot table in ONE round -- no re-read of the group, and less to clear and to read out per group.
// Any number of sub-rounds: a record's sub-round and its slot are two mulhi's of separate hash bits.
// the probe sequence of the LDS tables: s, s + step, s + 2 step ... (mod SLOTS) with an odd step < 1024 taken from hash bits the slot
// does not use, coprime to SLOTS = 1024 * PER -- LDS has no lines to stay within, and a full neighbourhood is left at once
// (-DKATOME_LC_LINEAR: step 1, the rounds 1-3 form, for the A/B)
template <int PER> KD u32 lc_step(u64 h) {
#ifdef KATOME_LC_LINEAR
    return 1u;
#else
    u32 step = (u32)((h >> 33) & 0x1FFu) * 2u + 1u;
    if ((PER & (PER - 1)) != 0 && step % (u32)PER == 0) step += 2;       // (PER = 13, 8: 13 is prime; a step of 13 j + 2 is not a multiple of it)
    return step;
#endif
}

// index[g] = first record whose hash has top `gbits` bits >= g (records ordered by those bits), g = 0 .. 2^gbits: one binary
// search per group boundary (31 dependent reads each) instead of a pass over all the records (3.4 ms at C3)
// (STRIDE: words per record -- first-seen builds carry one more word behind the k-mer's NW)
template <int NW, int STRIDE = NW>
__global__ __launch_bounds__(BLOCK) void hash_group_index_kernel(const u64* __restrict__ keys, u64 n, u32 gbits, u64* __restrict__ index) {
    for (u64 g = (u64)blockIdx.x * BLOCK + threadIdx.x; g <= (1ull << gbits); g += (u64)gridDim.x * BLOCK) {
        u64 lo = 0, hi = n;                                   // first i with (hash(keys[i]) >> (64 - gbits)) >= g
        while (lo < hi) {
            const u64 mid = lo + ((hi - lo) >> 1);
            Key<NW> a;
#pragma unroll
            for (int q = 0; q < NW; ++q) a.w[q] = keys[mid * STRIDE + q];
            if ((hash_key(a) >> (64 - gbits)) < g) lo = mid + 1; else hi = mid;
        }
        index[g] = lo;
    }
}

// ... the same boundaries of records that carry their count in the key word (counted_key.h): the hash is the plain key's
__global__ __launch_bounds__(BLOCK) void counted_group_index_kernel(const u64* __restrict__ keys, u64 n, u64* __restrict__ index) {
    for (u64 g = (u64)blockIdx.x * BLOCK + threadIdx.x; g <= (1ull << 16); g += (u64)gridDim.x * BLOCK) {
        u64 lo = 0, hi = n;
        while (lo < hi) {
            const u64 mid = lo + ((hi - lo) >> 1);
            Key<2> a; a.w[0] = counted_plain_word(keys[mid * 2]); a.w[1] = keys[mid * 2 + 1];
            if ((hash_key(a) >> 48) < g) lo = mid + 1; else hi = mid;
        }
        index[g] = lo;
    }
}
// the way back: packed records split in place into plain keys and a weights array, for the kernels that take those
__global__ __launch_bounds__(BLOCK) void counted_unpack_kernel(const u64* keys_in, u64 n, u64* keys_out, u32* __restrict__ w_out) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK) {
        const u64 w0 = keys_in[2 * i], w1 = keys_in[2 * i + 1];          // (keys_out may be keys_in: a thread reads its record before it writes it)
        keys_out[2 * i] = counted_plain_word(w0); keys_out[2 * i + 1] = w1;
        w_out[i] = counted_count_word(w0);
    }
}
int dev_counted_unpack(const uint64_t* d_in, uint64_t n, uint64_t* d_keys, uint32_t* d_weights, hipStream_t stream) {
    if (!n) return KATOME_OK;
    hipLaunchKernelGGL(counted_unpack_kernel, dim3(grid_for(n, BLOCK, 256u * 32u)), dim3(BLOCK), 0, stream, d_in, n, d_keys, d_weights);
    KCHECK_HIP(hipGetLastError());
    return KATOME_OK;
}

// (EVEN_K: only a k-mer of even length can be its own reverse complement; for odd k -- the headline's k = 31 -- the read-out's count step
// takes no reverse complement at all.  A TEMPLATE parameter, not a test of k at run time: with a uniform term inside the divergent
// condition hipcc 7.2 dropped the assignment on the divergent edge, profiles/r04_wrong_code.md)
template <bool RC, int PER, bool EVEN_K>
__global__ __launch_bounds__(LC_THREADS) void lds_count_kernel(const u64* keys, const u32* wts, const u64* __restrict__ index, u32 gbits,
                                                                u32 R, u32 k, u32 min_weight, u64* out_keys,
                                                                u32* out_w, u64 out_cap, unsigned long long* cursor,
                                                                unsigned long long* distinct, u32* err, u32 probe_limit,
                                                                unsigned long long* owner_cursor, u32 n_owners) {
    constexpr u32 LC_SLOTS = LcTable<PER>::SLOTS;
    extern __shared__ unsigned long long lc_mem[];
    unsigned long long* lkey = lc_mem;                                   // [LC_SLOTS]
    u32* lcnt = reinterpret_cast<u32*>(lc_mem + LC_SLOTS);               // [LC_SLOTS]
    __shared__ u32 wtot[LC_THREADS / 64];
    __shared__ unsigned long long base_sh;
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    u32 my_distinct = 0;
    LC_PHASE_BEGIN();
    const u32 n_groups = 1u << gbits, sub_shift = 64 - gbits - 16;     // (the group is the hash's top gbits, the sub-round its next 16)
    for (u32 g = blockIdx.x; g < n_groups; g += gridDim.x) {
        const u64 lo = index[g], hi = index[g + 1];
        if (lo == hi) continue;
        for (u32 r = 0; r < R; ++r) {
            for (u32 i = tid; i < LC_SLOTS; i += LC_THREADS) { lkey[i] = 0ull; lcnt[i] = 0u; }
            __syncthreads();
            LC_PHASE(0);
            constexpr u32 LU = KATOME_LC_LU;                            // records in flight per thread (the group is re-read from L2 / Infinity Cache)
            for (u64 i0 = lo + tid; i0 < hi; i0 += (u64)LC_THREADS * LU) {
                u64 kv[LU]; u32 wv[LU];
#pragma unroll
                for (u32 u = 0; u < LU; ++u) { const u64 i = i0 + (u64)u * LC_THREADS; kv[u] = 0; wv[u] = 0; if (i < hi) { kv[u] = keys[i]; wv[u] = wts[i]; } }
#pragma unroll
                for (u32 u = 0; u < LU; ++u) {
                    const u64 i = i0 + (u64)u * LC_THREADS;
                    if (i >= hi) continue;
                    Key<1> key; key.w[0] = kv[u];
                    const u64 h = hash_key(key);
                    if (R > 1 && (u32)((((h >> sub_shift) & 0xFFFFull) * R) >> 16) != r) continue;
                    const unsigned long long want = key.w[0] | OCC;
                    u32 s = (u32)(((h & 0x3FFFFFFFull) * LC_SLOTS) >> 30);                         // (bits 0..29: below every sub-round bit)
                    const u32 step = lc_step<PER>(h);
                    u32 probes = 0;
                    for (; probes < probe_limit; ++probes) {
                        const unsigned long long cur = atomicCAS(&lkey[s], 0ull, want);
                        if (cur == 0ull || cur == want) { atomicAdd(&lcnt[s], wv[u]); break; }
                        s += step; if (s >= LC_SLOTS) s -= LC_SLOTS;
                    }
                    // (with the guaranteed number of sub-rounds this cannot happen: a sub-round holds fewer records than slots; the
                    // optimistic first attempt -- records_to_edges_sorted -- gives up here and the host counts again)
                    if (probes == probe_limit) *err = 3;
                }
            }
            __syncthreads();
            LC_PHASE(1);
            // read-out: every thread owns LC_SLOTS / LC_THREADS consecutive slots

            Key<1> kk[PER]; u32 cc[PER], ne[PER]; u32 mine = 0;
#pragma unroll
            for (u32 j = 0; j < PER; ++j) {
                const u32 sidx = tid * PER + j;
                const unsigned long long v = lkey[sidx];
                ne[j] = 0; cc[j] = 0; kk[j].w[0] = 0;
                if (v & OCC) {
                    kk[j].w[0] = v & KEYBITS; cc[j] = lcnt[sidx];
                    ++my_distinct;
                    ne[j] = RC ? 2 : 1;
                    if (RC && EVEN_K && key_eq(revcomp(kk[j], k), kk[j])) ne[j] = 1;
                    if ((cc[j] << ((RC && ne[j] == 1) ? 1u : 0u)) < min_weight) ne[j] = 0;      // Clean::remove_weak_edges (pruner.rs:89-92)
                }
                mine += ne[j];
            }
            u32 incl = mine;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) { u32 v = __shfl_up(incl, o, 64); if (lane >= (u32)o) incl += v; }
            if (lane == 63) wtot[wave] = incl;
            __syncthreads();
            u32 woff = 0, total = 0;
#pragma unroll
            for (u32 w = 0; w < LC_THREADS / 64; ++w) { if (w < wave) woff += wtot[w]; total += wtot[w]; }
            // (owner_cursor: the group's keys go to the stretch of the rank that owns them -- groups are cut by the core's hash then)
            if (tid == 0) base_sh = !total ? 0ull : owner_cursor ? atomicAdd(&owner_cursor[core_group_owner(g, n_owners)], (unsigned long long)total)
                                                               : atomicAdd(cursor, (unsigned long long)total);
            __syncthreads();
            LC_PHASE(2);
            // the sub-round's edges leave through the table's own LDS (every thread holds its slots in registers by now): a thread's
            // edges are consecutive, so written straight from the registers a wave's store touched 64 lines, 96 bytes apart (38 % of
            // the kernel's clocks, profiles/r04_lc_phases.md); staged, the workgroup writes them as one stretch.  (C at a time: a
            // sub-round of more edges than slots -- a full table of k-mers on both strands -- takes two turns)
            {
                unsigned long long* skey = lc_mem;                     // [LC_SLOTS]
                u32* sw = lcnt;                                         // [LC_SLOTS]
                const u32 p0 = woff + (incl - mine);
                for (u32 c0 = 0; c0 < total; c0 += LC_SLOTS) {
                    u32 p = p0 - c0;                                    // (before the chunk: wraps to a large number, fails the test)
#pragma unroll
                    for (u32 j = 0; j < PER; ++j) {
                        if (!ne[j]) continue;
                        // (self-complementary k-mer: both strands are one edge.  Written as a shift: as `ne == 1 ? 2 * c : c` hipcc 7.2
                        // lowered the select to a switch on ne whose default arm left the weight register unset for the ne == 2 lanes)
                        const u32 w = cc[j] << ((RC && ne[j] == 1) ? 1u : 0u);
                        if (p < LC_SLOTS) { skey[p] = kk[j].w[0]; sw[p] = w; }
                        ++p;
                        if (ne[j] == 2) {
                            if (p < LC_SLOTS) { skey[p] = revcomp(kk[j], k).w[0]; sw[p] = w; }
                            ++p;
                        }
                    }
                    __syncthreads();
                    const u32 nc = total - c0 < LC_SLOTS ? total - c0 : LC_SLOTS;
                    const u64 o0 = base_sh + c0;
                    for (u32 i = tid; i < nc; i += LC_THREADS)
                        if (o0 + i < out_cap) { out_keys[o0 + i] = skey[i]; out_w[o0 + i] = sw[i]; }
                    __syncthreads();
                }
            }
            LC_PHASE(3);
        }
    }
    my_distinct = wave_sum(my_distinct);
    if (lane == 0 && my_distinct) atomicAdd(distinct, (unsigned long long)my_distinct);
}

// One-word k-mers, ONE visit per record: the hash that cuts the groups is a bijection of the key (mix64 = murmur3's finalizer), so
// inside group g a key IS the low 48 bits of its hash -- and a slot of 8 bytes holds them with a 16-bit count: 19456 slots where the
// 12-byte slots of lds_count_kernel are 13312, which takes C3's groups (22 k records of 12.3 k k-mers) in one round at load 0.63
// instead of two at 0.46 -- every record loaded, hashed and tested once, one table cleared and read out per group.  A record reads
// its slot first (most probes end there: a plain 8-byte read), claims an empty one with a compare-and-swap of remainder | count, or
// adds its count to the slot that holds its remainder; the read-out inverts the hash.  A count that does not fit 16 bits (or a
// record that brings one) sets err 5 and the caller counts with lds_count_kernel; a full table err 3, as there.  Both strands: odd k
// only (the caller keeps even k, where a k-mer can be its own reverse complement, with lds_count_kernel).
constexpr u32 LP_STAGE = LP_SLOTS * 8 / 12;                      // edges (8 B + 4 B) the same LDS stages at a time
template <bool RC>
__global__ __launch_bounds__(LC_THREADS) void lds_count_packed_kernel(const u64* keys, const u32* wts, const u64* __restrict__ index, u32 R, u32 k,
                                                                       u32 min_weight, u64* out_keys, u32* out_w, u64 out_cap, unsigned long long* cursor,
                                                                       unsigned long long* distinct, u32* err, u32 probe_limit) {
    constexpr unsigned long long REM = (1ull << 48) - 1;
    extern __shared__ unsigned long long lc_mem[];
    unsigned long long* slot = lc_mem;                                   // [LP_SLOTS]: remainder << 16 | count; 0 = empty
    __shared__ u32 wtot[LC_THREADS / 64];
    __shared__ unsigned long long base_sh;
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    u32 my_distinct = 0;
    LC_PHASE_BEGIN();
    for (u32 g = blockIdx.x; g < (1u << 16); g += gridDim.x) {
        const u64 lo = index[g], hi = index[g + 1];
        if (lo == hi) continue;
        for (u32 r = 0; r < R; ++r) {
            for (u32 i = tid; i < LP_SLOTS; i += LC_THREADS) slot[i] = 0ull;
            __syncthreads();
            LC_PHASE(8);
            // A wave runs as many probe steps as its slowest lane needs -- at this load ~6 with one slot per step -- and the instructions
            // of a step, not its waits, are what the insert phase costs (issuing a turn's swaps and adds together so that their LDS
            // round trips overlap made it slower: 17.7 ms against 13.8, profiles/r04_lc_phases.md).  So a step looks at FOUR slots:
            // two 16-byte buckets of two slots, one 16-byte read each, at b and b + step of the record's sequence of buckets.  A
            // record adds to the slot that holds its remainder, else claims the first empty one of the four in sequence order (slots
            // never empty again, so its remainder cannot sit behind an empty slot), else steps on -- a lane rarely needs a second step.
            constexpr u32 LU = KATOME_LC_LU;
            constexpr u32 NB = LP_SLOTS / 2;                                      // buckets: 9728 = 2^9 * 19
            for (u64 i0 = lo + tid; i0 < hi; i0 += (u64)LC_THREADS * LU) {
                u64 kv[LU]; u32 wv[LU];
#pragma unroll
                for (u32 u = 0; u < LU; ++u) { const u64 i = i0 + (u64)u * LC_THREADS; kv[u] = 0; wv[u] = 0; if (i < hi) { kv[u] = keys[i]; wv[u] = wts[i]; } }
#pragma unroll
                for (u32 u = 0; u < LU; ++u) {
                    const u64 i = i0 + (u64)u * LC_THREADS;
                    if (i >= hi) continue;
                    const u64 h = mix64(kv[u]);
                    if (R > 1 && (u32)((((h >> 32) & 0xFFFFull) * R) >> 16) != r) continue;
                    const u32 w = wv[u];
                    if (w == 0u || w > 0xFFFFu) { *err = 5; continue; }
                    const unsigned long long rem = h & REM, mine = (rem << 16) | w;
                    u32 b0 = (u32)(((h & 0x3FFFFFFFull) * NB) >> 30);
                    const u32 step = lc_step<LP_PER>(h);                            // (odd, no multiple of 19: coprime to NB)
                    u32 probes = 0;
                    for (; probes < probe_limit; ++probes) {
                        u32 b1 = b0 + step; if (b1 >= NB) b1 -= NB;
                        const ulonglong2 x = *reinterpret_cast<const ulonglong2*>(slot + 2 * b0), y = *reinterpret_cast<const ulonglong2*>(slot + 2 * b1);
                        const unsigned long long c[4] = {x.x, x.y, y.x, y.y};
                        u32 at = ~0u; bool have = false;                            // the slot to add to / to claim
#pragma unroll
                        for (int j = 3; j >= 0; --j) if ((c[j] >> 16) == rem && c[j] != 0ull) { at = (j < 2 ? 2 * b0 : 2 * b1 - 2) + j; have = true; }
                        if (!have) {
#pragma unroll
                            for (int j = 3; j >= 0; --j) if (c[j] == 0ull) at = (j < 2 ? 2 * b0 : 2 * b1 - 2) + j;
                            if (at == ~0u) { b0 = b1 + step; if (b0 >= NB) b0 -= NB; continue; }      // four slots of other k-mers: on
                            const unsigned long long cur = atomicCAS(&slot[at], 0ull, mine);
                            if (cur == 0ull) break;                                // claimed: remainder and count are in
                            if ((cur >> 16) != rem) continue;                      // (somebody else's k-mer got there first: look at the four again)
                        }
                        const unsigned long long old = atomicAdd(&slot[at], (unsigned long long)w);
                        if ((old & 0xFFFFull) + w > 0xFFFFull) *err = 5;              // (the carry went into the remainder: nothing of this attempt is used)
                        break;
                    }
                    if (probes == probe_limit) *err = 3;
                }
            }
            __syncthreads();
            LC_PHASE(9);
            // read-out: every thread LP_PER consecutive slots, their k-mers (the hash inverted) and counts in registers -- the staging
            // below overwrites the table.  Staged is ONE entry per k-mer; with both strands the writer makes two edges of it (thread o
            // takes entry o / 2 and, odd, its reverse complement): k is odd here, no k-mer is its own reverse complement
            Key<1> kk[LP_PER]; u32 cc[LP_PER]; u32 keep = 0;
#pragma unroll
            for (u32 j = 0; j < LP_PER; ++j) {
                const unsigned long long v = slot[tid * LP_PER + j];
                kk[j].w[0] = 0; cc[j] = 0;
                if (v) {
                    ++my_distinct;
                    cc[j] = (u32)v & 0xFFFFu;
                    kk[j].w[0] = unmix64(((u64)g << 48) | (v >> 16));
                    if (cc[j] >= min_weight) keep |= 1u << j;                       // Clean::remove_weak_edges (pruner.rs:89-92)
                }
            }
            const u32 mine = (u32)__popc(keep);
            u32 incl = mine;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) { u32 t = __shfl_up(incl, o, 64); if (lane >= (u32)o) incl += t; }
            if (lane == 63) wtot[wave] = incl;
            __syncthreads();
            u32 woff = 0, total = 0;
#pragma unroll
            for (u32 w = 0; w < LC_THREADS / 64; ++w) { if (w < wave) woff += wtot[w]; total += wtot[w]; }
            constexpr u32 F = RC ? 2 : 1;                                            // edges per k-mer
            if (tid == 0) base_sh = total ? atomicAdd(cursor, (unsigned long long)total * F) : 0ull;
            __syncthreads();
            LC_PHASE(10);
            {
                unsigned long long* skey = lc_mem;                                  // [LP_STAGE]
                u32* sw = reinterpret_cast<u32*>(lc_mem + LP_STAGE);                 // [LP_STAGE]
                const u32 p0 = woff + (incl - mine);
                for (u32 c0 = 0; c0 < total; c0 += LP_STAGE) {
                    u32 p = p0 - c0;                                                 // (before the chunk: wraps to a large number, fails the test)
#pragma unroll
                    for (u32 j = 0; j < LP_PER; ++j) {
                        if (!((keep >> j) & 1u)) continue;
                        if (p < LP_STAGE) { skey[p] = kk[j].w[0]; sw[p] = cc[j]; }
                        ++p;
                    }
                    __syncthreads();
                    const u32 nc = total - c0 < LP_STAGE ? total - c0 : LP_STAGE;
                    const u64 o0 = base_sh + (u64)c0 * F;
                    for (u32 o = tid; o < nc * F; o += LC_THREADS) {
                        const u32 e = RC ? o >> 1 : o;
                        Key<1> x; x.w[0] = skey[e];
                        if (RC && (o & 1u)) x = revcomp(x, k);
                        if (o0 + o < out_cap) { out_keys[o0 + o] = x.w[0]; out_w[o0 + o] = sw[e]; }
                    }
                    __syncthreads();
                }
            }
            LC_PHASE(11);
        }
    }
    my_distinct = wave_sum(my_distinct);
    if (lane == 0 && my_distinct) atomicAdd(distinct, (unsigned long long)my_distinct);
}

// The k-mer level counted so that half of its edges leave it in order (KATOME_EDGE_HALF_SORT; one-word k-mers of odd k or one strand,
// one visit per record).  The records are in their representative orientation (kmer_bits.h rep_orientation; as they are with one
// strand) and ordered by their leading 16 key bits (dev_key_order), so group g is the key range of prefix g.  The insert loop is
// lds_count_packed_kernel's, with the key's low 2k - 16 bits in the slot instead of the hash's (the probe sequence still comes from the
// hash).  At read-out the group's kept keys are put in key order in the table's own LDS (lds_order.h: a counting sort on the
// remainder's top bits, then every key is placed by counting the keys of its bucket below it) and leave as two lists:
//   S1, the representatives, ascending, from the group's first record on (s1_key + index[g]: fixed before the count, so the groups
//       stay in key order; a group has no more distinct keys than records), their number in group_count[g];
//   S2 (both strands), their reverse complements, behind a cursor in no order.
// group_merge_kernel (radix.hip) orders S2 group by group and merges it with S1 (half_merge_kernel when S2 is sorted in full).
// The buckets: the table's entries are in registers while they are ordered, so its LDS is free but for the kept entries' places
// [0, total).  Where total leaves the table's tail free (LO_FINE_MAX; always at C3, 12 300 of 19 456), 8192 buckets of 1.5 keys have
// their counters there, in the slots from LO_FINE_SLOT on, which their owners clear as they read them out; a fuller table takes the 2048
// buckets behind the table.  total is known before the ordering starts: the kept entries are added up across the barrier that the
// tail's reuse needs anyway.
// err 5 / err 3 as in lds_count_packed_kernel: the caller then counts the usual way.
static_assert(LC_THREADS == LDS_ORDER_THREADS, "the read-out orders with lds_order.h");
constexpr u32 LO_COARSE_WORDS = (lds_order_words(LDS_ORDER_COARSE_BITS) + 1) / 2 * 2;                      // (u32 words behind the table)
constexpr u32 LO_FINE_SLOT = (LP_SLOTS - (lds_order_words(LDS_ORDER_FINE_BITS) + 1) / 2) / 2 * 2;          // (an even slot: 16-byte aligned)
constexpr u32 LO_FINE_MAX = LO_FINE_SLOT;
constexpr size_t LO_LDS = (size_t)LP_SLOTS * 8 + LO_COARSE_WORDS * 4;
static_assert((LP_SLOTS - LO_FINE_SLOT) * 2 >= lds_order_words(LDS_ORDER_FINE_BITS), "the fine buckets fit the table's tail");
// REGIONS (round 22): S2 leaves by the digit of its FIRST partition pass, bits 2k - 16 .. 2k - 9 of the reverse complement -- region d
// of s2_key / s2_w / s2_digit starts at tile reg.start_tile[d], takes reg.cap[d] keys and has its append cursor at reg.cursor[d * S2_CURSOR_STEP]
// (s2_regions.h; a 128-byte line to a cursor) -- with the SECOND pass's digit, bits 2k - 8 .. 2k - 1, in the byte stream: that
// first pass then has nothing left to do (radix.hip, dev_s2_region_pass).  After S1 has left, every thread takes its entries of
// slot[0, total) into registers as reverse complements and counts their digits into 256 LDS bins (the atomic's return value is the entry's arrival index);
// the bins are scanned, threads 0 .. 255 reserve their digit's keys with one returning atomic on the region's cursor, every entry
// goes back to slot[dstart[d] + arrival] (the scatter kernel's LDS reorder) and slot[] is streamed out, consecutive lanes to
// consecutive addresses inside a digit's run.  The bins, their starts and the regions' offsets lie in the bucket words behind the
// table, free by then.  No workgroup waits for another.  A region without room for the group's keys: err[1] = d + 1 and the group
// writes no S2 (the host then rebuilds S2 from S1: s2_rebuild_kernel); the other groups go on.
constexpr u32 S2_CURSOR_STEP = 16;          // u64 words between two regions' cursors
// (32 bits each for a region's first tile and its keys: a level counted this way has fewer than 2^32 records, s2_regions_route)
struct S2RegionsOut { const u32* start_tile; const u32* cap; unsigned long long* cursor; };
// (Reg: one S2RegionsOut with REGIONS, nothing without -- the kernel's arguments are then the ones it had)
template <bool RC, bool REGIONS = false, class... Reg>
__global__ __launch_bounds__(LC_THREADS) void lds_count_ordered_kernel(const u64* keys, const u32* wts, const u64* __restrict__ index, u32 k,
                                                                        u32 min_weight, u64* s1_key, u32* s1_w, u32* group_count, u64* s2_key,
                                                                        u32* s2_w, uint8_t* s2_digit, u64 s2_cap, unsigned long long* cursor,
                                                                        unsigned long long* distinct, u32* err, u32 probe_limit, Reg... regions) {
    static_assert(!REGIONS || RC, "one strand has no S2");
    static_assert(sizeof...(Reg) == (REGIONS ? 1 : 0), "the regions come with REGIONS only");
    extern __shared__ unsigned long long lc_mem[];
    unsigned long long* slot = lc_mem;                                   // [LP_SLOTS]: remainder << 16 | count; then the kept ones in key order
    u32* bucket = reinterpret_cast<u32*>(lc_mem + LP_SLOTS);             // [LO_COARSE_WORDS]: the 2048 buckets of a table too full for ...
    u32* fine = reinterpret_cast<u32*>(lc_mem + LO_FINE_SLOT);           // ... the 8192 in the table's tail
    __shared__ u32 wtot[LC_THREADS / 64];
    __shared__ unsigned long long base_sh;
    __shared__ u32 kept_sh;
    constexpr u32 RG_BINS = 256, RG_FULL = LO_COARSE_WORDS - 1;          // (REGIONS: bucket[RG_FULL] -- a region had no room for this group's keys)
    static_assert(4 * RG_BINS < RG_FULL && lds_order_words(LDS_ORDER_COARSE_BITS) <= RG_FULL, "the bins, their starts, the regions' offsets and the flag fit the bucket words");
    const u32 tid = threadIdx.x, lane = tid & 63;
    const u32 rem_bits = 2 * k - 16;
    const u32 bshift_c = rem_bits > LDS_ORDER_COARSE_BITS ? rem_bits - LDS_ORDER_COARSE_BITS : 0;          // (bucket: the remainder's top bits)
    const u32 bshift_f = rem_bits > LDS_ORDER_FINE_BITS ? rem_bits - LDS_ORDER_FINE_BITS : 0;
    const u64 REM = (1ull << rem_bits) - 1;
    u32 my_distinct = 0;
    LC_PHASE_BEGIN();
    for (u32 g = blockIdx.x; g < (1u << 16); g += gridDim.x) {
        const u64 lo = index[g], hi = index[g + 1];
        if (lo == hi) continue;
        for (u32 i = tid; i < LP_SLOTS; i += LC_THREADS) slot[i] = 0ull;
        bucket[tid] = 0u;
        if (tid == 0) kept_sh = 0u;
        __syncthreads();
        LC_PHASE(12);
        constexpr u32 LU = KATOME_LC_LU;
        constexpr u32 NB = LP_SLOTS / 2;
        for (u64 i0 = lo + tid; i0 < hi; i0 += (u64)LC_THREADS * LU) {
            u64 kv[LU]; u32 wv[LU];
#pragma unroll
            for (u32 u = 0; u < LU; ++u) { const u64 i = i0 + (u64)u * LC_THREADS; kv[u] = 0; wv[u] = 0; if (i < hi) { kv[u] = keys[i]; wv[u] = wts[i]; } }
#pragma unroll
            for (u32 u = 0; u < LU; ++u) {
                const u64 i = i0 + (u64)u * LC_THREADS;
                if (i >= hi) continue;
                const u64 h = mix64(kv[u]);
                const u32 w = wv[u];
                if (w == 0u || w > 0xFFFFu) { *err = 5; continue; }
                const unsigned long long rem = kv[u] & REM, mine = (rem << 16) | w;
                u32 b0 = (u32)(((h & 0x3FFFFFFFull) * NB) >> 30);
                const u32 step = lc_step<LP_PER>(h);
                u32 probes = 0;
                for (; probes < probe_limit; ++probes) {
                    u32 b1 = b0 + step; if (b1 >= NB) b1 -= NB;
                    const ulonglong2 x = *reinterpret_cast<const ulonglong2*>(slot + 2 * b0), y = *reinterpret_cast<const ulonglong2*>(slot + 2 * b1);
                    const unsigned long long c[4] = {x.x, x.y, y.x, y.y};
                    u32 at = ~0u; bool have = false;
#pragma unroll
                    for (int j = 3; j >= 0; --j) if ((c[j] >> 16) == rem && c[j] != 0ull) { at = (j < 2 ? 2 * b0 : 2 * b1 - 2) + j; have = true; }
                    if (!have) {
#pragma unroll
                        for (int j = 3; j >= 0; --j) if (c[j] == 0ull) at = (j < 2 ? 2 * b0 : 2 * b1 - 2) + j;
                        if (at == ~0u) { b0 = b1 + step; if (b0 >= NB) b0 -= NB; continue; }
                        const unsigned long long cur = atomicCAS(&slot[at], 0ull, mine);
                        if (cur == 0ull) break;
                        if ((cur >> 16) != rem) continue;
                    }
                    const unsigned long long old = atomicAdd(&slot[at], (unsigned long long)w);
                    if ((old & 0xFFFFull) + w > 0xFFFFull) *err = 5;
                    break;
                }
                if (probes == probe_limit) *err = 3;
            }
        }
        __syncthreads();
        LC_PHASE(13);
        // read-out into registers; the table's LDS then takes the kept entries in bucket order
        LO_PHASE_BEGIN();
        u32 rt = tid;                                         // (through an empty asm: nothing of the read-out is hoisted out of the group loop, lds_order.h)
        asm volatile("" : "+v"(rt));
        unsigned long long v[LP_PER]; u32 keep = 0;
#pragma unroll
        for (u32 j = 0; j < LP_PER; ++j) {
            v[j] = slot[rt * LP_PER + j];
            if (v[j]) { ++my_distinct; if (((u32)v[j] & 0xFFFFu) >= min_weight) keep |= 1u << j; }      // Clean::remove_weak_edges
        }
        if ((rt + 1) * LP_PER > LO_FINE_SLOT) {               // (the fine buckets' counters: slots this thread has just read)
#pragma unroll
            for (u32 j = 0; j < LP_PER; ++j) if (rt * LP_PER + j >= LO_FINE_SLOT) slot[rt * LP_PER + j] = 0ull;
        }
        const u32 wave_kept = wave_sum((u32)__popc(keep));
        if (lane == 0 && wave_kept) atomicAdd(&kept_sh, wave_kept);
        __syncthreads();
        LO_PHASE(0);
        // the kept ones into key order in the table's LDS (lds_order.h); the group's S2 room is reserved once their number is known
        const auto reserve = [&](u32 t) {
            if (tid == 0) { group_count[g] = t; base_sh = t ? atomicAdd(cursor, (unsigned long long)t) : 0ull; }
        };
        const auto stamp = [&](u32 i) { LO_PHASE(1 + i); (void)i; };
        const u32 total = kept_sh <= LO_FINE_MAX ? lds_order_entries<LP_PER, LDS_ORDER_FINE_BITS>(v, keep, slot, fine, wtot, bshift_f, reserve, stamp)
                                                 : lds_order_entries<LP_PER, LDS_ORDER_COARSE_BITS>(v, keep, slot, bucket, wtot, bshift_c, reserve, stamp);
        LC_PHASE(14);
        if constexpr (REGIONS) {
            const S2RegionsOut reg = [](const S2RegionsOut& r) { return r; }(regions...);
            u32* hist = bucket;                                               // [256] keys per digit; then their starts in slot[]
            u32* dstart = bucket + RG_BINS;                                   // [256]
            u64* goff = reinterpret_cast<u64*>(bucket + 2 * RG_BINS);         // [256] where the digit's keys go in the region arrays
            if (rt < RG_BINS) hist[rt] = 0u;
            if (rt == 0) bucket[RG_FULL] = 0u;
            unsigned long long e[LP_PER]; u32 arr[(LP_PER + 1) / 2];
#pragma unroll
            for (u32 t = 0; t < (LP_PER + 1) / 2; ++t) arr[t] = 0;
            // (an entry turns into its reverse complement here, once: r's low 16 bits are the group's -- the reverse complement of the
            // prefix g --, so r's other bits and the 16-bit count fit the entry's 64 bits, and r is one and-or away from then on)
            Key<1> gx; gx.w[0] = (u64)g << rem_bits;
            const u32 r_low = (u32)revcomp(gx, k).w[0] & 0xFFFFu;
#pragma unroll
            for (u32 t = 0; t < LP_PER; ++t) {
                const u32 i = rt + t * LC_THREADS;
                e[t] = 0;
                if (i >= total) continue;
                e[t] = slot[i];
                Key<1> x; x.w[0] = gx.w[0] | (e[t] >> 16);
                const u32 c = (u32)e[t] & 0xFFFFu;
                if (lo + i < hi) { s1_key[lo + i] = x.w[0]; s1_w[lo + i] = c; }
                e[t] = (revcomp(x, k).w[0] & ~0xFFFFull) | c;
            }
            const auto rc_of = [&](unsigned long long en) { return (en & ~0xFFFFull) | r_low; };
            __syncthreads();
            LC_PHASE(4);
#pragma unroll
            for (u32 t = 0; t < LP_PER; ++t) {
                if (rt + t * LC_THREADS >= total) continue;
                const u32 d = (u32)(rc_of(e[t]) >> rem_bits) & (RG_BINS - 1);
                arr[t >> 1] |= atomicAdd(&hist[d], 1u) << ((t & 1u) * 16u);          // (a group holds fewer than 2^16 entries)
            }
            __syncthreads();
            LC_PHASE(5);
            // (the reservation's round trip and the loads of the region's room and start run under the scan and the reorder: thread d
            // asks for digit d's place in its region, thread 256 + d for the region's keys, thread 512 + d for its first tile -- one
            // register each --, and the three meet in LDS after the reorder)
            static_assert(LC_THREADS >= 3 * RG_BINS, "three threads per digit");
            u32 incl = 0, held = 0;
            {
                const u32 d = rt & (RG_BINS - 1), c = hist[d];
                if (rt < RG_BINS) {
                    if (c) held = (u32)atomicAdd(&reg.cursor[d * S2_CURSOR_STEP], (unsigned long long)c);
                    incl = c;
#pragma unroll
                    for (int o = 1; o < 64; o <<= 1) { const u32 up = __shfl_up(incl, o, 64); if (lane >= (u32)o) incl += up; }
                    if (lane == 63) wtot[rt >> 6] = incl;
                } else if (rt < 2 * RG_BINS) held = reg.cap[d];
                else if (rt < 3 * RG_BINS) held = reg.start_tile[d];
            }
            __syncthreads();
            if (rt < RG_BINS) {
                u32 woff = 0;
#pragma unroll
                for (u32 w = 0; w < RG_BINS / 64; ++w) if (w < (rt >> 6)) woff += wtot[w];
                dstart[rt] = woff + incl - hist[rt];
            }
            __syncthreads();
            LC_PHASE(6);
#pragma unroll
            for (u32 t = 0; t < LP_PER; ++t) {
                if (rt + t * LC_THREADS >= total) continue;
                const u32 d = (u32)(rc_of(e[t]) >> rem_bits) & (RG_BINS - 1);
                slot[dstart[d] + ((arr[t >> 1] >> ((t & 1u) * 16u)) & 0xFFFFu)] = e[t];
            }
            if (rt >= RG_BINS && rt < 2 * RG_BINS) {          // hist[d]: the last place in the region that still takes the group's keys
                const u32 d = rt - RG_BINS, c = hist[d];
                if (c > held) { bucket[RG_FULL] = 1u; err[1] = d + 1; }
                hist[d] = held - c;
            } else if (rt >= 2 * RG_BINS && rt < 3 * RG_BINS) goff[rt - 2 * RG_BINS] = (u64)held * S2_REGION_TILE;
            __syncthreads();
            if (rt < RG_BINS) {          // (a digit without keys asked for no place: held = 0)
                if (held > hist[rt]) { bucket[RG_FULL] = 1u; err[1] = rt + 1; }
                goff[rt] += held;
            }
            __syncthreads();
            LC_PHASE(7);
            if (!bucket[RG_FULL]) {          // (the same for every thread)
                for (u32 i = rt; i < total; i += LC_THREADS) {
                    const unsigned long long en = slot[i];
                    const u64 r = rc_of(en);
                    const u32 d = (u32)(r >> rem_bits) & (RG_BINS - 1);
                    const u64 to = goff[d] + (i - dstart[d]);
                    s2_key[to] = r; s2_w[to] = (u32)en & 0xFFFFu; s2_digit[to] = (uint8_t)(r >> (rem_bits + 8));
                }
            }
        } else
        for (u32 i = rt; i < total; i += LC_THREADS) {
            const unsigned long long e = slot[i];
            Key<1> x; x.w[0] = ((u64)g << rem_bits) | (e >> 16);
            const u32 c = (u32)e & 0xFFFFu;
            if (lo + i < hi) { s1_key[lo + i] = x.w[0]; s1_w[lo + i] = c; }
            if (RC && base_sh + i < s2_cap) {
                // (beside the key, the digit of S2's first partition pass -- dev_key_order, bits 2k - 16 .. 2k - 9 --, which then reads no key to count)
                const u64 r = revcomp(x, k).w[0];
                s2_key[base_sh + i] = r; s2_w[base_sh + i] = c; s2_digit[base_sh + i] = (uint8_t)(r >> rem_bits);
            }
        }
        __syncthreads();
        LC_PHASE(15);
    }
    my_distinct = wave_sum(my_distinct);
    if (lane == 0 && my_distinct) atomicAdd(distinct, (unsigned long long)my_distinct);
}

// How many of a level's ordered records have a reverse complement of first partition digit d (bits 2k - 16 .. 2k - 9), counted on
// the sample of s2_regions.h: rows `stride` apart, 256 records each.  counts: 256 words, zero on entry.
static_assert(S2_SAMPLE_ROW == BLOCK && S2_REGIONS == (u32)BLOCK, "a thread per record of a row and per bin");
__global__ __launch_bounds__(BLOCK) void s2_region_sample_kernel(const u64* __restrict__ keys, u64 n, u32 k, u64 rows, u64 stride, u32* counts) {
    __shared__ u32 h[S2_REGIONS];
    h[threadIdx.x] = 0u;
    __syncthreads();
    for (u64 r = blockIdx.x; r < rows; r += gridDim.x) {
        const u64 i = r * stride * S2_SAMPLE_ROW + threadIdx.x;
        if (i >= n) continue;
        Key<1> x; x.w[0] = keys[i];
        atomicAdd(&h[(u32)(revcomp(x, k).w[0] >> (2 * k - 16)) & (S2_REGIONS - 1)], 1u);
    }
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&counts[threadIdx.x], h[threadIdx.x]);
}

// The way back of the REGIONS count: S2 made again from S1, which is complete in place -- group g's reverse complements at
// off[g] .. off[g] + group_count[g] (off: the counts' prefix sums), with their first partition digits, as the count without regions
// leaves them but for the order, which nobody depends on
__global__ __launch_bounds__(BLOCK) void s2_rebuild_kernel(const u64* __restrict__ s1_key, const u32* __restrict__ s1_w, const u64* __restrict__ group_first,
                                                           const u32* __restrict__ group_count, const u64* __restrict__ off, u32 k, u64* s2_key,
                                                           u32* s2_w, uint8_t* s2_digit, u64 s2_cap) {
    for (u32 g = blockIdx.x; g < (1u << 16); g += gridDim.x) {
        const u64 from = group_first[g], to = off[g];
        const u32 c = group_count[g];
        for (u32 i = threadIdx.x; i < c; i += BLOCK) {
            Key<1> x; x.w[0] = s1_key[from + i];
            const u64 r = revcomp(x, k).w[0];
            if (to + i < s2_cap) { s2_key[to + i] = r; s2_w[to + i] = s1_w[from + i]; s2_digit[to + i] = (uint8_t)(r >> (2 * k - 16)); }
        }
    }
}

// in place: the level's one-word k-mer records in their representative orientation (rep) or back in the canonical one
template <bool REP>
__global__ __launch_bounds__(BLOCK) void orient_records_kernel(u64* keys, u64 n, u32 k) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK) {
        Key<1> x; x.w[0] = keys[i];
        keys[i] = (REP ? rep_orientation(x, k) : canonical(x, k)).w[0];
    }
}

// group boundaries when the records are ordered by the hash of their core (dev_hash_order_core), and the owners' first positions:
// owner p's groups are [ceil(p * 2^gbits / n), ceil((p + 1) * 2^gbits / n))
__global__ __launch_bounds__(BLOCK) void core_group_index_kernel(const u64* __restrict__ keys, u64 n, u32 gbits, u32 core_shift, u32 core_bases,
                                                                 u64* __restrict__ index) {
    for (u64 g = (u64)blockIdx.x * BLOCK + threadIdx.x; g <= (1ull << gbits); g += (u64)gridDim.x * BLOCK) {
        u64 lo = 0, hi = n;
        while (lo < hi) {
            const u64 mid = lo + ((hi - lo) >> 1);
            Key<1> a; a.w[0] = keys[mid];
            if ((core_hash(a, core_shift, core_bases) >> (64 - gbits)) < g) lo = mid + 1; else hi = mid;
        }
        index[g] = lo;
    }
}
__global__ void owner_bases_kernel(const u64* __restrict__ index, u32 gbits, u32 n_owners, unsigned long long* owner_cursor, u64* bases) {
    const u32 p = threadIdx.x;
    if (p > n_owners) return;
    const u64 g0 = (((u64)p << gbits) + n_owners - 1) / n_owners;          // first group whose owner is p (p == n_owners: one past the end)
    const u64 at = index[g0 < (1ull << gbits) ? g0 : (1ull << gbits)];
    bases[p] = at;
    if (p < n_owners) owner_cursor[p] = at;
}

// The same for k-mers of two words (k = 32..63; the reference's example configuration runs k = 40): the LDS slot stays 12 bytes
// -- a 16-byte key would halve the table -- and holds, published by ONE compare-and-swap, a 43-bit fingerprint of the key's hash
// and the position (within the group, < 2^20) of a REPRESENTATIVE record; a record whose fingerprint meets an occupied slot's
// compares its whole key with the representative's (read back from the group: L2 / Infinity Cache) and only then adds its
// count -- exact whatever the fingerprints do.  The read-out fetches each distinct key through its representative.
template <bool RC, int PER, int NW, bool EVEN_K>
__global__ __launch_bounds__(LC_THREADS) void lds_count_wide_kernel(const u64* keys, const u32* wts, const u64* __restrict__ index, u32 gbits,
                                                                     u32 R, u32 k, u32 min_weight, u64* out_keys, u32* out_w, u64 out_cap,
                                                                     unsigned long long* cursor, unsigned long long* distinct, u32* err, u32 probe_limit,
                                                                     unsigned long long* /*owner_cursor: one-word k-mers only*/, u32 /*n_owners*/) {
    constexpr u32 LC_SLOTS = LcTable<PER>::SLOTS;
    constexpr unsigned long long REP_MASK = (1ull << 20) - 1;
    extern __shared__ unsigned long long lc_mem[];
    unsigned long long* lkey = lc_mem;                                   // [LC_SLOTS]: OCC | fingerprint << 20 | representative
    u32* lcnt = reinterpret_cast<u32*>(lc_mem + LC_SLOTS);               // [LC_SLOTS]
    __shared__ u32 wtot[LC_THREADS / 64];
    __shared__ unsigned long long base_sh;
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    u32 my_distinct = 0;
    LC_PHASE_BEGIN();
    const u32 n_groups = 1u << gbits, sub_shift = 64 - gbits - 16;
    for (u32 g = blockIdx.x; g < n_groups; g += gridDim.x) {
        const u64 lo = index[g], hi = index[g + 1];
        if (lo == hi) continue;
        if (hi - lo > REP_MASK) { if (tid == 0) *err = 4; continue; }      // (a group of a million records: not k-mers of reads; the caller counts in the table)
        for (u32 r = 0; r < R; ++r) {
            for (u32 i = tid; i < LC_SLOTS; i += LC_THREADS) { lkey[i] = 0ull; lcnt[i] = 0u; }
            __syncthreads();
            LC_PHASE(4);
            constexpr u32 LU = KATOME_LC_LU;                            // records per thread and turn
            Key<NW> kv[LU]; u32 wv[LU];
            auto fetch = [&](u64 i0, Key<NW>* kk, u32* ww) {
#pragma unroll
                for (u32 u = 0; u < LU; ++u) {
                    const u64 i = i0 + (u64)u * LC_THREADS;
                    ww[u] = 0;
#pragma unroll
                    for (int q = 0; q < NW; ++q) kk[u].w[q] = 0;
                    if (i < hi) {
#pragma unroll
                        for (int q = 0; q < NW; ++q) kk[u].w[q] = keys[i * NW + q];
                        ww[u] = wts ? wts[i] : 1u;         // (no weights: every record counts once -- a level's records straight from the reads)
                    }
                }
            };
            fetch(lo + tid, kv, wv);
            for (u64 i0 = lo + tid; i0 < hi; i0 += (u64)LC_THREADS * LU) {
              Key<NW> kn[LU]; u32 wn[LU];
              fetch(i0 + (u64)LC_THREADS * LU, kn, wn);                 // the next turn's records are on their way while this turn's are counted (19.2 -> 18.4 ms at C3)
#pragma unroll
              for (u32 u = 0; u < LU; ++u) {
                const u64 i = i0 + (u64)u * LC_THREADS;
                if (i >= hi) continue;
                const Key<NW> key = kv[u];
                const u64 h = hash_key(key);
                if (R > 1 && (u32)((((h >> sub_shift) & 0xFFFFull) * R) >> 16) != r) continue;
                const unsigned long long want = OCC | (((h >> 5) & ((1ull << 43) - 1)) << 20) | (unsigned long long)(i - lo);
                const u32 w = wv[u];
                u32 s = (u32)(((h & 0x3FFFFFFFull) * LC_SLOTS) >> 30);
                const u32 step = lc_step<PER>(h);
                u32 probes = 0;
                for (; probes < probe_limit; ++probes) {
                    const unsigned long long cur = atomicCAS(&lkey[s], 0ull, want);
                    bool mine = cur == 0ull;
                    if (!mine && (cur >> 20) == (want >> 20)) {            // same fingerprint: the same key?
                        const u64 j = lo + (cur & REP_MASK);
                        mine = true;
#ifndef KATOME_LC_EXPERIMENT_NO_COMPARE          // (an experiment build only: what the representative's fetch costs -- NOT exact)
#pragma unroll
                        for (int q = 0; q < NW; ++q) mine = mine && keys[j * NW + q] == key.w[q];
#endif
                    }
                    if (mine) { atomicAdd(&lcnt[s], w); break; }
                    s += step; if (s >= LC_SLOTS) s -= LC_SLOTS;
                }
                if (probes == probe_limit) *err = 3;
              }
#pragma unroll
              for (u32 u = 0; u < LU; ++u) { kv[u] = kn[u]; wv[u] = wn[u]; }
            }
            __syncthreads();
            LC_PHASE(5);
            // (the slots' keys are fetched where they are staged, not held across the scan in between: PER keys of NW words were 2 * PER * NW
            // registers -- spilled to scratch -- and only a k-mer of even length is looked at before that)
            constexpr bool LOOK = RC && EVEN_K;                  // (then a slot's key is fetched here too, looked at and let go again)
            u32 rp[PER], cc[PER], ne[PER]; u32 mine = 0;
#pragma unroll
            for (u32 j = 0; j < (u32)PER; ++j) {
                const u32 sidx = tid * PER + j;
                const unsigned long long v = lkey[sidx];
                ne[j] = 0; cc[j] = 0; rp[j] = 0;
                if (v & OCC) {
                    rp[j] = (u32)(v & REP_MASK);
                    cc[j] = lcnt[sidx];
                    ++my_distinct;
                    ne[j] = RC ? 2 : 1;
                    if (LOOK) {
                        Key<NW> x;
#pragma unroll
                        for (int q = 0; q < NW; ++q) x.w[q] = keys[(lo + rp[j]) * NW + q];
                        if (key_eq(revcomp(x, k), x)) ne[j] = 1;
                    }
                    if ((cc[j] << ((RC && ne[j] == 1) ? 1u : 0u)) < min_weight) ne[j] = 0;      // Clean::remove_weak_edges (pruner.rs:89-92)
                }
                mine += ne[j];
            }
            u32 incl = mine;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) { u32 v = __shfl_up(incl, o, 64); if (lane >= (u32)o) incl += v; }
            if (lane == 63) wtot[wave] = incl;
            __syncthreads();
            u32 woff = 0, total = 0;
#pragma unroll
            for (u32 w = 0; w < LC_THREADS / 64; ++w) { if (w < wave) woff += wtot[w]; total += wtot[w]; }
            if (tid == 0) base_sh = total ? atomicAdd(cursor, (unsigned long long)total) : 0ull;
            __syncthreads();
            LC_PHASE(6);
            // (out through the table's LDS, SC entries at a time, as lds_count_kernel's: one stretch per workgroup instead of 64 lines per store)
            {
                constexpr u32 SC = LC_SLOTS * 12 / (8 * NW + 4);
                unsigned long long* skey = lc_mem;                     // [SC][NW]
                u32* sw = reinterpret_cast<u32*>(lc_mem + (size_t)SC * NW);      // [SC]
                const u32 p0 = woff + (incl - mine);
                for (u32 c0 = 0; c0 < total; c0 += SC) {
                    u32 p = p0 - c0;
#pragma unroll
                    for (u32 j = 0; j < (u32)PER; ++j) {
                        if (!ne[j]) continue;
                        const u32 w = cc[j] << ((RC && ne[j] == 1) ? 1u : 0u);       // (as a shift: see lds_count_kernel)
                        if (p < SC || (ne[j] == 2 && p + 1 < SC)) {
                            Key<NW> x;
#pragma unroll
                            for (int q = 0; q < NW; ++q) x.w[q] = keys[(lo + rp[j]) * NW + q];
                            if (p < SC) {
#pragma unroll
                                for (int q = 0; q < NW; ++q) skey[p * NW + q] = x.w[q];
                                sw[p] = w;
                            }
                            if (ne[j] == 2 && p + 1 < SC) {
                                const Key<NW> rk = revcomp(x, k);
#pragma unroll
                                for (int q = 0; q < NW; ++q) skey[(p + 1) * NW + q] = rk.w[q];
                                sw[p + 1] = w;
                            }
                        }
                        p += ne[j];
                    }
                    __syncthreads();
                    const u32 nc = total - c0 < SC ? total - c0 : SC;
                    const u64 o0 = base_sh + c0;
                    const u64 room = o0 < out_cap ? out_cap - o0 : 0;
                    const u32 nk = (u32)(room < nc ? room : nc);
                    for (u32 i = tid; i < nk * NW; i += LC_THREADS) out_keys[o0 * NW + i] = skey[i];
                    for (u32 i = tid; i < nk; i += LC_THREADS) out_w[o0 + i] = sw[i];
                    __syncthreads();
                }
            }
            LC_PHASE(7);
        }
    }
    my_distinct = wave_sum(my_distinct);
    if (lane == 0 && my_distinct) atomicAdd(distinct, (unsigned long long)my_distinct);
}

// Two-word keys whose DISTINCT keys per group are few (the tile levels of k <= 31: C3's groups hold 12 k records of 2.2 k / 3.7 k tiles;
// the k-mers of k = 32..63 at the benchmark shapes' coverage): the slot holds the WHOLE key -- 16 bytes + a count, 7168 slots -- so
// a record that meets its key again compares in LDS: one 16-byte read, one add.  lds_count_wide_kernel's slot has a fingerprint and
// must fetch the representative's key for every such meeting -- 64 lines from L2 per wave, 80 % of the tile records are repeats --,
// and that fetch is a third of its time (an experiment build without the comparison: 18.4 -> 11.9 ms at C3, not exact).  A slot is
// claimed word by word, each by a compare-and-swap from 0 (a word never changes again): whoever sets the first word has the slot for
// keys with that first word, the first to set the second has it for its key, a record that loses the second word moves on along
// its own probe sequence -- every key sits on its sequence behind occupied slots only.  The second word is stored XOR a salt so that
// 0 stays "not set"; the one key whose second word IS the salt cannot be stored (err 7: the caller counts with the wide kernel, as it
// does when a table fills: err 3).  Which kernel counts a level is decided by counting 256 of its groups first (records_to_edges_sorted).
// (LF_PER slots per thread: 7 -> 7168 slots of 16 + 4 bytes = 140 KiB; 4 -> 4096 slots = 80 KiB for groups of few distinct keys:
// less to clear and to read out per group)
constexpr u64 LF_SALT = 0x9E3779B97F4A7C15ull;
// COUNTED (counted_key.h): the records carry their count in the key word and there is no weights array.  After
// the load the count is taken out of the word and the word made plain; from there on the kernel is the same -- the hash for slot and
// step, A, B, the salt test, the read-out -- and the list it writes holds plain keys and u32 counts.
// (a tile level's records, the only ones that come packed, are never oriented and never thresholded: COUNTED with one strand only)
template <bool RC, bool EVEN_K, int LF_PER, bool COUNTED = false>
__global__ __launch_bounds__(LC_THREADS) void lds_count_full_kernel(const u64* keys, const u32* wts, const u64* __restrict__ index, u32 groups_run, u32 k,
                                                                     u32 min_weight, u64* out_keys, u32* out_w, u64 out_cap, unsigned long long* cursor,
                                                                     unsigned long long* distinct, u32* err, u32 probe_limit) {
    static_assert(!COUNTED || (!RC && !EVEN_K), "packed records are a tile level's");
    constexpr u32 LF_SLOTS = LfTable<LF_PER>::SLOTS;
    extern __shared__ unsigned long long lc_mem[];
    ulonglong2* slot = reinterpret_cast<ulonglong2*>(lc_mem);            // [LF_SLOTS]: {first word | OCC, second word ^ salt}
    u32* lcnt = reinterpret_cast<u32*>(lc_mem + 2 * (size_t)LF_SLOTS);   // [LF_SLOTS]
    __shared__ u32 wtot[LC_THREADS / 64];
    __shared__ unsigned long long base_sh;
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    u32 my_distinct = 0;
    for (u32 g = blockIdx.x; g < groups_run; g += gridDim.x) {
        const u64 lo = index[g], hi = index[g + 1];
        if (lo == hi) continue;
        for (u32 i = tid; i < LF_SLOTS; i += LC_THREADS) { slot[i] = make_ulonglong2(0ull, 0ull); lcnt[i] = 0u; }
        __syncthreads();
        constexpr u32 LU = KATOME_LC_LU;
        u64 ka[LU], kb[LU]; u32 wv[LU];
        auto fetch = [&](u64 i0, u64* a, u64* b, u32* w) {
#pragma unroll
            for (u32 u = 0; u < LU; ++u) {
                const u64 i = i0 + (u64)u * LC_THREADS;
                a[u] = 0; b[u] = 0; w[u] = 0;
                // (no branch around the load: past the group's end a lane reads the group's last record, which nobody looks at.  Under
                // `if (i < hi)` hipcc 7.2 waited for each of these loads before it issued the next -- four memory latencies a turn instead
                // of one, 8.46 ms at C3 for the counted form against the plain form's 8.22 with its weights array and all; the plain
                // form waited the same way for the next turn's loads until it took the clamp too)
                // (the both-strand forms keep the branch: at LF_PER = 7 they stand at 128 VGPRs and the clamped loads spilled)
                if constexpr (COUNTED || !RC) {
                    const u64 ic = i < hi ? i : hi - 1;
                    const ulonglong2 v = *reinterpret_cast<const ulonglong2*>(keys + 2 * ic); a[u] = v.x; b[u] = v.y;
                    if constexpr (!COUNTED) w[u] = wts ? wts[ic] : 1u;
                } else
                if (i < hi) { const ulonglong2 v = *reinterpret_cast<const ulonglong2*>(keys + 2 * i); a[u] = v.x; b[u] = v.y; w[u] = wts ? wts[i] : 1u; }
            }
        };
        fetch(lo + tid, ka, kb, wv);
        for (u64 i0 = lo + tid; i0 < hi; i0 += (u64)LC_THREADS * LU) {
            u64 na[LU], nb[LU]; u32 nwv[LU];
            fetch(i0 + (u64)LC_THREADS * LU, na, nb, nwv);              // (the next turn's records are on their way)
#pragma unroll
            for (u32 u = 0; u < LU; ++u) {
                if (i0 + (u64)u * LC_THREADS >= hi) continue;
                if constexpr (COUNTED) { wv[u] = counted_count_word(ka[u]); ka[u] = counted_plain_word(ka[u]); }
                Key<2> key; key.w[0] = ka[u]; key.w[1] = kb[u];
                const u64 h = hash_key(key);
                const unsigned long long A = ka[u] | OCC, B = kb[u] ^ LF_SALT;
                if (B == 0ull) { *err = 7; continue; }
                u32 s = (u32)(((h & 0x3FFFFFFFull) * LF_SLOTS) >> 30);
                const u32 step = lc_step<LF_PER>(h);
                u32 probes = 0;
                for (; probes < probe_limit; ++probes) {
                    const ulonglong2 v = slot[s];
                    unsigned long long a = v.x, b = v.y;
                    if (a == 0ull) { a = atomicCAS(&slot[s].x, 0ull, A); if (a == 0ull) a = A; }
                    if (a == A && b == 0ull) { b = atomicCAS(&slot[s].y, 0ull, B); if (b == 0ull) b = B; }
                    if (a == A && b == B) { atomicAdd(&lcnt[s], wv[u]); break; }
                    s += step; if (s >= LF_SLOTS) s -= LF_SLOTS;
                }
                if (probes == probe_limit) *err = 3;
            }
#pragma unroll
            for (u32 u = 0; u < LU; ++u) { ka[u] = na[u]; kb[u] = nb[u]; wv[u] = nwv[u]; }
        }
        __syncthreads();
        // read-out: every thread LF_PER consecutive slots, their keys in registers (the staging below overwrites the table)
        Key<2> kk[LF_PER]; u32 cc[LF_PER], ne[LF_PER]; u32 mine = 0;
#pragma unroll
        for (u32 j = 0; j < LF_PER; ++j) {
            const ulonglong2 v = slot[tid * LF_PER + j];
            ne[j] = 0; cc[j] = 0; kk[j].w[0] = 0; kk[j].w[1] = 0;
            if (v.x) {
                kk[j].w[0] = v.x & ~OCC; kk[j].w[1] = v.y ^ LF_SALT;
                cc[j] = lcnt[tid * LF_PER + j];
                ++my_distinct;
                ne[j] = RC ? 2 : 1;
                if (RC && EVEN_K && key_eq(revcomp(kk[j], k), kk[j])) ne[j] = 1;
                if ((cc[j] << ((RC && ne[j] == 1) ? 1u : 0u)) < min_weight) ne[j] = 0;      // Clean::remove_weak_edges (pruner.rs:89-92)
            }
            mine += ne[j];
        }
        u32 incl = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { u32 t = __shfl_up(incl, o, 64); if (lane >= (u32)o) incl += t; }
        if (lane == 63) wtot[wave] = incl;
        __syncthreads();
        u32 woff = 0, total = 0;
#pragma unroll
        for (u32 w = 0; w < LC_THREADS / 64; ++w) { if (w < wave) woff += wtot[w]; total += wtot[w]; }
        if (tid == 0) base_sh = total ? atomicAdd(cursor, (unsigned long long)total) : 0ull;
        __syncthreads();
        {   // out through the table's LDS, one stretch per workgroup (an entry is as large as a slot)
            unsigned long long* skey = lc_mem;                         // [LF_SLOTS][2]
            u32* sw = lcnt;                                             // [LF_SLOTS]
            const u32 p0 = woff + (incl - mine);
            for (u32 c0 = 0; c0 < total; c0 += LF_SLOTS) {
                u32 p = p0 - c0;                                        // (before the chunk: wraps to a large number, fails the tests)
#pragma unroll
                for (u32 j = 0; j < LF_PER; ++j) {
                    if (!ne[j]) continue;
                    const u32 w = cc[j] << ((RC && ne[j] == 1) ? 1u : 0u);       // (as a shift: see lds_count_kernel)
                    if (p < LF_SLOTS) { skey[2 * (size_t)p] = kk[j].w[0]; skey[2 * (size_t)p + 1] = kk[j].w[1]; sw[p] = w; }
                    ++p;
                    if (ne[j] == 2) {
                        if (p < LF_SLOTS) { const Key<2> rk = revcomp(kk[j], k); skey[2 * (size_t)p] = rk.w[0]; skey[2 * (size_t)p + 1] = rk.w[1]; sw[p] = w; }
                        ++p;
                    }
                }
                __syncthreads();
                const u32 nc = total - c0 < LF_SLOTS ? total - c0 : LF_SLOTS;
                const u64 o0 = base_sh + c0;
                const u64 room = o0 < out_cap ? out_cap - o0 : 0;
                const u32 nk = (u32)(room < nc ? room : nc);
                for (u32 i = tid; i < nk * 2; i += LC_THREADS) out_keys[o0 * 2 + i] = skey[i];
                for (u32 i = tid; i < nk; i += LC_THREADS) out_w[o0 + i] = sw[i];
                __syncthreads();
            }
        }
    }
    my_distinct = wave_sum(my_distinct);
    if (lane == 0 && my_distinct) atomicAdd(distinct, (unsigned long long)my_distinct);
}

// The same for THREE-word keys (tiles of 64..95 bases: every tile level of k = 32..63 at 150 bp; never oriented, never thresholded): 24 B
// of key in three arrays + a count, 5120 or 3072 slots; the second and third word XOR a salt each, claimed in turn.  These levels' groups
// hold a few hundred distinct tiles, so the small table is the usual one.
constexpr u64 LF_SALT2 = 0xD1B54A32D192ED03ull;
template <int PER>
__global__ __launch_bounds__(LC_THREADS) void lds_count_full3_kernel(const u64* keys, const u32* wts, const u64* __restrict__ index, u32 groups_run,
                                                                      u64* out_keys, u32* out_w, u64 out_cap, unsigned long long* cursor,
                                                                      unsigned long long* distinct, u32* err, u32 probe_limit) {
    constexpr u32 SLOTS = Lf3Table<PER>::SLOTS;
    extern __shared__ unsigned long long lc_mem[];
    unsigned long long* sa = lc_mem;                                     // [SLOTS] first word | OCC
    unsigned long long* sb = lc_mem + SLOTS;                             // [SLOTS] second word ^ salt
    unsigned long long* sc = lc_mem + 2 * (size_t)SLOTS;                 // [SLOTS] third word ^ salt
    u32* lcnt = reinterpret_cast<u32*>(lc_mem + 3 * (size_t)SLOTS);      // [SLOTS]
    __shared__ u32 wtot[LC_THREADS / 64];
    __shared__ unsigned long long base_sh;
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    u32 my_distinct = 0;
    for (u32 g = blockIdx.x; g < groups_run; g += gridDim.x) {
        const u64 lo = index[g], hi = index[g + 1];
        if (lo == hi) continue;
        for (u32 i = tid; i < SLOTS; i += LC_THREADS) { sa[i] = 0ull; sb[i] = 0ull; sc[i] = 0ull; lcnt[i] = 0u; }
        __syncthreads();
        constexpr u32 LU = 2;
        for (u64 i0 = lo + tid; i0 < hi; i0 += (u64)LC_THREADS * LU) {
            u64 ka[LU], kb[LU], kc[LU]; u32 wv[LU];
#pragma unroll
            for (u32 u = 0; u < LU; ++u) {
                const u64 i = i0 + (u64)u * LC_THREADS;
                ka[u] = 0; kb[u] = 0; kc[u] = 0; wv[u] = 0;
                if (i < hi) { ka[u] = keys[3 * i]; kb[u] = keys[3 * i + 1]; kc[u] = keys[3 * i + 2]; wv[u] = wts ? wts[i] : 1u; }
            }
#pragma unroll
            for (u32 u = 0; u < LU; ++u) {
                if (i0 + (u64)u * LC_THREADS >= hi) continue;
                Key<3> key; key.w[0] = ka[u]; key.w[1] = kb[u]; key.w[2] = kc[u];
                const u64 h = hash_key(key);
                const unsigned long long A = ka[u] | OCC, B = kb[u] ^ LF_SALT, C = kc[u] ^ LF_SALT2;
                if (B == 0ull || C == 0ull) { *err = 7; continue; }
                u32 s = (u32)(((h & 0x3FFFFFFFull) * SLOTS) >> 30);
                const u32 step = lc_step<PER>(h);
                u32 probes = 0;
                for (; probes < probe_limit; ++probes) {
                    unsigned long long a = sa[s], b = sb[s], c = sc[s];
                    if (a == 0ull) { a = atomicCAS(&sa[s], 0ull, A); if (a == 0ull) a = A; }
                    if (a == A && b == 0ull) { b = atomicCAS(&sb[s], 0ull, B); if (b == 0ull) b = B; }
                    if (a == A && b == B && c == 0ull) { c = atomicCAS(&sc[s], 0ull, C); if (c == 0ull) c = C; }
                    if (a == A && b == B && c == C) { atomicAdd(&lcnt[s], wv[u]); break; }
                    s += step; if (s >= SLOTS) s -= SLOTS;
                }
                if (probes == probe_limit) *err = 3;
            }
        }
        __syncthreads();
        Key<3> kk[PER]; u32 cc[PER]; u32 keep = 0;
#pragma unroll
        for (u32 j = 0; j < (u32)PER; ++j) {
            const u32 x = tid * PER + j;
            const unsigned long long a = sa[x];
            kk[j].w[0] = 0; kk[j].w[1] = 0; kk[j].w[2] = 0; cc[j] = 0;
            if (a) { kk[j].w[0] = a & ~OCC; kk[j].w[1] = sb[x] ^ LF_SALT; kk[j].w[2] = sc[x] ^ LF_SALT2; cc[j] = lcnt[x]; keep |= 1u << j; ++my_distinct; }
        }
        const u32 mine = (u32)__popc(keep);
        u32 incl = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { u32 t = __shfl_up(incl, o, 64); if (lane >= (u32)o) incl += t; }
        if (lane == 63) wtot[wave] = incl;
        __syncthreads();
        u32 woff = 0, total = 0;
#pragma unroll
        for (u32 w = 0; w < LC_THREADS / 64; ++w) { if (w < wave) woff += wtot[w]; total += wtot[w]; }
        if (tid == 0) base_sh = total ? atomicAdd(cursor, (unsigned long long)total) : 0ull;
        __syncthreads();
        {   // out through the table's LDS, one stretch per workgroup (an entry is as large as a slot: total <= SLOTS)
            unsigned long long* skey = lc_mem;                         // [SLOTS][3]
            u32* sw = lcnt;                                             // [SLOTS]
            u32 p = woff + (incl - mine);
#pragma unroll
            for (u32 j = 0; j < (u32)PER; ++j) {
                if (!((keep >> j) & 1u)) continue;
                skey[3 * (size_t)p] = kk[j].w[0]; skey[3 * (size_t)p + 1] = kk[j].w[1]; skey[3 * (size_t)p + 2] = kk[j].w[2]; sw[p] = cc[j];
                ++p;
            }
            __syncthreads();
            const u64 o0 = base_sh;
            const u64 room = o0 < out_cap ? out_cap - o0 : 0;
            const u32 nk = (u32)(room < total ? room : total);
            for (u32 i = tid; i < nk * 3; i += LC_THREADS) out_keys[o0 * 3 + i] = skey[i];
            for (u32 i = tid; i < nk; i += LC_THREADS) out_w[o0 + i] = sw[i];
            __syncthreads();
        }
    }
    my_distinct = wave_sum(my_distinct);
    if (lane == 0 && my_distinct) atomicAdd(distinct, (unsigned long long)my_distinct);
}

// counts the records of each hash group in an LDS table and lowers the two sequence numbers; writes every distinct k-mer as one or
// two edges {key} + {sequence number, weight}.  The slot's first word is the k-mer itself when it has one word (lds_count_kernel's
// slot) and fingerprint | representative record when it has two (lds_count_wide_kernel's: the full keys are compared in the group).
// LIST: a TILE level of such a build -- every distinct key leaves once, as key + tag (the two lowered numbers
// packed again: both come from the first read that holds the tile on either strand) in out_keys [n][NWK + 1] and its count in
// out_pairs read as u32 [n]; RC then only says whether the second number is tracked.
// DELTA: the records carry the delta tag (seen_tag.h: reads of varying length) -- lA / lB then hold the two numbers themselves, and
// seq_per_read means nothing.
template <bool RC, int NWK, bool LIST = false, bool DELTA = false>
__global__ __launch_bounds__(LC_THREADS) void lds_count_seen_kernel(const u64* recs, const u32* wts, const u64* __restrict__ index, u32 gbits, u32 R, u32 k,
                                                                     u64 seq_per_read, u64* out_keys, u64* out_pairs, u64 out_cap,
                                                                     unsigned long long* cursor, unsigned long long* distinct, u32* err, u32 probe_limit) {
    constexpr u32 SLOTS = LC_THREADS * LCS_PER;
    constexpr int STRIDE = NWK + 1;
    constexpr unsigned long long REP_MASK = (1ull << 20) - 1;
    extern __shared__ unsigned long long lcs_mem[];
    unsigned long long* lkey = lcs_mem;                                  // [SLOTS]: OCC | key, or OCC | fingerprint << 20 | representative
    unsigned long long* lA = lcs_mem + SLOTS;                            // [SLOTS]: read << 16 | offset (DELTA: the number), stored orientation
    unsigned long long* lB = lcs_mem + 2 * SLOTS;                        // [SLOTS]: ... reverse complement
    u32* lcnt = reinterpret_cast<u32*>(lcs_mem + 3 * SLOTS);             // [SLOTS]
    __shared__ u32 wtot[LC_THREADS / 64];
    __shared__ unsigned long long base_sh;
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    u32 my_distinct = 0;
    const u32 n_groups = 1u << gbits, sub_shift = 64 - gbits - 16;
    for (u32 g = blockIdx.x; g < n_groups; g += gridDim.x) {
        const u64 lo = index[g], hi = index[g + 1];
        if (lo == hi) continue;
        if (NWK > 1 && hi - lo > REP_MASK) { if (tid == 0) *err = 4; continue; }
        for (u32 r = 0; r < R; ++r) {
            for (u32 i = tid; i < SLOTS; i += LC_THREADS) { lkey[i] = 0ull; lA[i] = SEEN_NONE; lB[i] = SEEN_NONE; lcnt[i] = 0u; }
            __syncthreads();
            constexpr u32 LU = 4;                            // records in flight per thread (the group is re-read from L2 / Infinity Cache)
            for (u64 i0 = lo + tid; i0 < hi; i0 += (u64)LC_THREADS * LU) {
              Key<NWK> kv[LU]; unsigned long long tv[LU]; u32 wv[LU];
#pragma unroll
              for (u32 u = 0; u < LU; ++u) {
                  const u64 i = i0 + (u64)u * LC_THREADS;
                  tv[u] = 0; wv[u] = 0;
#pragma unroll
                  for (int q = 0; q < NWK; ++q) kv[u].w[q] = 0;
                  if (i < hi) {
#pragma unroll
                      for (int q = 0; q < NWK; ++q) kv[u].w[q] = recs[i * STRIDE + q];
                      tv[u] = recs[i * STRIDE + NWK]; wv[u] = wts ? wts[i] : 1u;        // (no counts: one each -- tiles straight from the reads)
                  }
              }
#pragma unroll
              for (u32 u = 0; u < LU; ++u) {
                const u64 i = i0 + (u64)u * LC_THREADS;
                if (i >= hi) continue;
                const Key<NWK> key = kv[u];
                const u64 h = hash_key(key);
                if (R > 1 && (u32)((((h >> sub_shift) & 0xFFFFull) * R) >> 16) != r) continue;
                const unsigned long long tag = tv[u];
                const unsigned long long want = NWK == 1 ? (OCC | key.w[0]) : (OCC | (((h >> 5) & ((1ull << 43) - 1)) << 20) | (unsigned long long)(i - lo));
                const u32 w = wv[u];
                u32 s = (u32)(((h & 0x3FFFFFFFull) * SLOTS) >> 30);
                const u32 step = lc_step<LCS_PER>(h);
                u32 probes = 0;
                for (; probes < probe_limit; ++probes) {
                    const unsigned long long cur = atomicCAS(&lkey[s], 0ull, want);
                    bool mine = cur == 0ull || (NWK == 1 && cur == want);
                    if (NWK > 1 && !mine && (cur >> 20) == (want >> 20)) {
                        const u64 j = lo + (cur & REP_MASK);
                        mine = true;
#pragma unroll
                        for (int q = 0; q < NWK; ++q) mine = mine && recs[j * STRIDE + q] == key.w[q];
                    }
                    if (mine) {
                        atomicAdd(&lcnt[s], w);
                        atomicMin(&lA[s], DELTA ? delta_p(tag) : (tag >> 32) << 16 | ((tag >> 16) & 0xFFFFull));
                        if (RC) atomicMin(&lB[s], DELTA ? delta_q(tag) : (tag >> 32) << 16 | (tag & 0xFFFFull));
                        break;
                    }
                    s += step; if (s >= SLOTS) s -= SLOTS;
                }
                if (probes == probe_limit) *err = 3;
              }
            }
            __syncthreads();
            // (a slot's numbers and count are read out with its key: the staging below overwrites the table)
            Key<NWK> kk[LCS_PER]; u32 ne[LCS_PER]; unsigned long long sa[LCS_PER], sb[LCS_PER]; u32 sc[LCS_PER]; u32 mine = 0;
#pragma unroll
            for (u32 j = 0; j < (u32)LCS_PER; ++j) {
                const unsigned long long v = lkey[tid * LCS_PER + j];
                ne[j] = 0; sa[j] = 0; sb[j] = 0; sc[j] = 0;
#pragma unroll
                for (int q = 0; q < NWK; ++q) kk[j].w[q] = 0;
                if (v & OCC) {
                    sa[j] = lA[tid * LCS_PER + j]; sb[j] = lB[tid * LCS_PER + j]; sc[j] = lcnt[tid * LCS_PER + j];
                    ++my_distinct;
                    if (NWK == 1) kk[j].w[0] = v & KEYBITS;
                    else {
                        const u64 rep = lo + (v & REP_MASK);
#pragma unroll
                        for (int q = 0; q < NWK; ++q) kk[j].w[q] = recs[rep * STRIDE + q];
                    }
                    ne[j] = (!LIST && RC && !key_eq(revcomp(kk[j], k), kk[j])) ? 2 : 1;
                }
                mine += ne[j];
            }
            u32 incl = mine;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) { u32 v = __shfl_up(incl, o, 64); if (lane >= (u32)o) incl += v; }
            if (lane == 63) wtot[wave] = incl;
            __syncthreads();
            u32 woff = 0, total = 0;
#pragma unroll
            for (u32 w = 0; w < LC_THREADS / 64; ++w) { if (w < wave) woff += wtot[w]; total += wtot[w]; }
            if (tid == 0) base_sh = total ? atomicAdd(cursor, (unsigned long long)total) : 0ull;
            __syncthreads();
            // out through the table's LDS, one stretch per workgroup (as lds_count_kernel's: a thread's entries are consecutive, so written
            // from the registers a wave's store touched 64 lines).  An entry: KW key words (+ the packed numbers of a list entry) and PW
            // words of payload -- a list entry's count, or an edge's {sequence number, count}; SC entries at a time
            {
                constexpr u32 KW = LIST ? STRIDE : NWK;
                constexpr u32 ENTRY = KW * 8 + (LIST ? 4 : 16);
                constexpr u32 SC = SLOTS * 28 / ENTRY;
                unsigned long long* skey = lcs_mem;                                 // [SC][KW]
                unsigned long long* spair = lcs_mem + (size_t)SC * KW;               // edges: [SC][2]
                u32* scount = reinterpret_cast<u32*>(spair);                        // list: [SC]
                const u32 p0 = woff + (incl - mine);
                for (u32 c0 = 0; c0 < total; c0 += SC) {
                    u32 p = p0 - c0;                                                 // (before the chunk: wraps to a large number, fails the tests)
#pragma unroll
                    for (u32 j = 0; j < (u32)LCS_PER; ++j) {
                        if (!ne[j]) continue;
                        const unsigned long long a = sa[j], b = sb[j];
                        const u64 seq_a = DELTA ? a : (a >> 16) * seq_per_read + (a & 0xFFFFull), seq_b = DELTA ? b : (b >> 16) * seq_per_read + (b & 0xFFFFull);
                        const u32 c = sc[j];
                        if (LIST) {
                            if (p < SC) {
#pragma unroll
                                for (int q = 0; q < NWK; ++q) skey[(size_t)p * KW + q] = kk[j].w[q];
                                if (DELTA) {
                                    if (!delta_packs(a, RC ? b : a)) *err = 6;          // (the two numbers of a tile too far apart: two reads -- cannot be -- or a read too long)
                                    skey[(size_t)p * KW + NWK] = delta_pack(a, RC ? b : a);
                                } else {
                                if (RC && (a >> 16) != (b >> 16)) *err = 6;              // (the two numbers of a tile from two reads: cannot be)
                                skey[(size_t)p * KW + NWK] = seen_pack(a >> 16, (u32)(a & 0xFFFFull), RC ? (u32)(b & 0xFFFFull) : 0u);
                                }
                                scount[p] = c;
                            }
                        } else if (ne[j] == 2) {
                            if (p < SC) {
#pragma unroll
                                for (int q = 0; q < NWK; ++q) skey[(size_t)p * KW + q] = kk[j].w[q];
                                spair[2 * (size_t)p] = seq_a; spair[2 * (size_t)p + 1] = c;
                            }
                            if (p + 1 < SC) {
                                const Key<NWK> rk = revcomp(kk[j], k);
#pragma unroll
                                for (int q = 0; q < NWK; ++q) skey[(size_t)(p + 1) * KW + q] = rk.w[q];
                                spair[2 * (size_t)(p + 1)] = seq_b; spair[2 * (size_t)(p + 1) + 1] = c;
                            }
                        } else {
                            // one edge: no reverse complements in this build, or a k-mer that is its own (added twice per window: both numbers
                            // are insertions of this edge)
                            if (p < SC) {
#pragma unroll
                                for (int q = 0; q < NWK; ++q) skey[(size_t)p * KW + q] = kk[j].w[q];
                                spair[2 * (size_t)p] = RC ? (seq_a < seq_b ? seq_a : seq_b) : seq_a;
                                spair[2 * (size_t)p + 1] = RC ? (u64)(c << 1) : (u64)c;
                            }
                        }
                        p += ne[j];
                    }
                    __syncthreads();
                    const u32 nc = total - c0 < SC ? total - c0 : SC;
                    const u64 o0 = base_sh + c0;
                    const u64 room = o0 < out_cap ? out_cap - o0 : 0;
                    const u32 nk = (u32)(room < nc ? room : nc);
                    for (u32 i = tid; i < nk * KW; i += LC_THREADS) out_keys[o0 * KW + i] = skey[i];
                    if (LIST) { for (u32 i = tid; i < nk; i += LC_THREADS) reinterpret_cast<u32*>(out_pairs)[o0 + i] = scount[i]; }
                    else      { for (u32 i = tid; i < nk * 2; i += LC_THREADS) out_pairs[o0 * 2 + i] = spair[i]; }
                    __syncthreads();
                }
            }
        }
    }
    my_distinct = wave_sum(my_distinct);
    if (lane == 0 && my_distinct) atomicAdd(distinct, (unsigned long long)my_distinct);
}

// ---- host side: one launch path (lc_launch), one function per strategy, records_to_edges_sorted / tagged_records_sorted on top ----
// the optimistic attempt's patience with a full table (KATOME_LC_PROBE_LIMIT: tests make the first attempt fail with it)
static u32 lc_probe_limit() { static const u32 v = (u32)std::max(1, env_int("KATOME_LC_PROBE_LIMIT", 128)); return v; }
// share of a group's records assumed distinct when the sub-rounds of the first attempt are chosen (KATOME_LC_OPTIMISM; 1 = never
// try with fewer than the guaranteed number)
static double lc_optimism() { static const double v = getenv("KATOME_LC_OPTIMISM") ? std::min(1.0, std::max(0.05, atof(getenv("KATOME_LC_OPTIMISM")))) : 0.75; return v; }
// a line of KATOME_LC_TRACE (looked up on every call)
static void lc_trace(const char* fmt, ...) {
    if (!getenv("KATOME_LC_TRACE")) return;
    va_list ap; va_start(ap, fmt); vfprintf(stderr, fmt, ap); va_end(ap);
}
// KATOME_LC_FULL=0: whole keys in the slots never, =1: without asking (tests).  KATOME_LC_FULL_PER (tests): 4 -> the small table, else the large one
static int lc_full_mode() { static const int v = env_int("KATOME_LC_FULL", -1); return v; }
static int lc_full_per() { static const int v = env_int("KATOME_LC_FULL_PER", 0); return v; }

// The 64 bytes every counting kernel reports through: {cursor, distinct, err}.  With an OwnerSplit also the owners' cursors, started at the
// owners' first records (a group's keys are no more than its records), and those starts themselves, n_parts + 1 of them: reset() restarts both.
struct LcAux {
    DevBuf buf, owners;
    hipStream_t stream;
    const u64* index = nullptr; u32 gbits = 0, n_owners = 0;
    // (more: device words a kernel leaves beside the 64 bytes -- the ordered count's region cursors --, read back with them)
    const void* more = nullptr; void* more_host = nullptr; size_t more_bytes = 0;
    explicit LcAux(hipStream_t s) : buf(s), owners(s), stream(s) {}
    unsigned long long* cursor() const { return buf.as<unsigned long long>(); }
    unsigned long long* distinct() const { return cursor() + 1; }
    u32* err() const { return reinterpret_cast<u32*>(cursor() + 2); }
    unsigned long long* owner_cursor() const { return owners.as<unsigned long long>(); }
    int reset() {
        KCHECK_HIP(hipMemsetAsync(buf.p, 0, 64, stream));
        if (owners.p) hipLaunchKernelGGL(owner_bases_kernel, dim3(1), dim3(64), 0, stream, index, gbits, n_owners, owner_cursor(), owners.as<u64>() + KATOME_MAX_RANKS + 1);
        return KATOME_OK;
    }
};
struct LcResult { uint64_t n_out = 0, n_distinct = 0; uint32_t code = 0, full = 0; };      // full: err[1] (the ordered count's regions)

// One attempt of one counting kernel over the level's groups: counters cleared, the kernel on 256 workgroups, and what it left in
// `aux` read back (n: the level's records, for the timer)
template <class... P, class... A>
static int lc_launch(LcAux& aux, void (*kernel)(P...), size_t lds, uint64_t n, LcResult& r, A... args) {
    KCHECK(aux.reset());
    KCHECK_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    {
        KernelScope ks(K_LDS_COUNT, aux.stream, n);
        hipLaunchKernelGGL(kernel, dim3(256u), dim3(LC_THREADS), lds, aux.stream, static_cast<P>(args)...);
    }
    KCHECK_HIP(hipGetLastError());
    uint64_t h[3] = {0, 0, 0};
    KCHECK_HIP(hipMemcpyAsync(h, aux.buf.p, 24, hipMemcpyDeviceToHost, aux.stream));
    if (aux.more) KCHECK_HIP(hipMemcpyAsync(aux.more_host, aux.more, aux.more_bytes, hipMemcpyDeviceToHost, aux.stream));
    KCHECK_HIP(hipStreamSynchronize(aux.stream));
    r.n_out = h[0]; r.n_distinct = h[1]; r.code = (uint32_t)h[2]; r.full = (uint32_t)(h[2] >> 32);
    return KATOME_OK;
}

// f(RC, EVEN_K): one strand; both strands of an odd k; both of an even k (EVEN_K only ever with RC: no other kernel is instantiated)
template <class F> static int with_strands(bool rc, uint32_t k, F f) {
    if (!rc) return f(BoolC<false>{}, BoolC<false>{});
    return (k & 1) ? f(BoolC<true>{}, BoolC<false>{}) : f(BoolC<true>{}, BoolC<true>{});
}

// First with fewer sub-rounds than would hold a group of DISTINCT records (lc_optimism): the k-mers of reads repeat (C3: 1.8 records
// per k-mer at this level), so the table is half empty at the guaranteed number.  An attempt that fills its table gives up after
// lc_probe_limit() = 128 probes (err 3, nothing it wrote is used) and the guaranteed number runs.
template <class Count>
static int count_optimistic(const char* what, u32 R_try, u32 R, u32 guaranteed_limit, const LcResult& r, Count count) {
    if (R_try < R) {
        KCHECK(count(R_try, lc_probe_limit()));
        if (r.code != 3) return KATOME_OK;
        lc_trace("[lds count] %s: the attempt with %u sub-rounds filled a table; counting again with %u\n", what, R_try, R);
    }
    return count(R, guaranteed_limit);
}

// Tagged records [n][nwk + 1] (key, read << 32 | offset << 16 | offset -- or the delta tag, `tag`) with their counts -> two hash passes on the key, counted in LDS
// with the two numbers lowered (lds_count_seen_kernel).  list == false: the oriented edges, out_keys [e][nwk] + out_second [e][2] =
// {sequence number, weight}.  list == true (a tile level): the distinct keys with their tags, out_keys [d][nwk + 1], and their counts,
// out_second [d] u32.  The records come back permuted.
int tagged_records_sorted(DevBuf& recs, DevBuf& wts, uint64_t n, uint32_t k, bool rc, SeenTag tag, bool list, DevBuf& edge_key,
                          DevBuf& seq_weight, uint64_t* n_edges, uint64_t* n_distinct, hipStream_t stream, uint32_t* first_counts) {
    *n_edges = 0; *n_distinct = 0;
    const uint32_t nwk = (uint32_t)key_words_for_k(k), stride = nwk + 1;
    if (nwk > 2 || !tag.packs() || !lcs_level_fits(n)) return KATOME_E_UNSUPPORTED;
    const uint64_t seq_per_read = tag.seq_per_read;
    LcAux aux(stream);
    KCHECK(aux.buf.alloc(64));
    KCHECK(aux.reset());
    if (n == 0) { KCHECK(edge_key.alloc(16, stream)); KCHECK(seq_weight.alloc(16, stream)); return KATOME_OK; }
    const u64* ko = nullptr; const u32* wo = nullptr;
    u32 gbits = 16;
    DevBuf kb(stream), wb(stream);
    const bool unit = wts.p == nullptr;                  // (no counts: every record counts once, and the passes move the records only)
    KCHECK(kb.alloc((n + 1) * 8 * stride));
    if (!unit) KCHECK(wb.alloc((n + 1) * 4));
    KCHECK(dev_hash_order_tagged(recs.as<u64>(), wts.as<u32>(), n, nwk, kb.as<u64>(), recs.as<u64>(), wb.as<u32>(), wts.as<u32>(), &ko, &wo, &gbits, stream, first_counts));
    kb.release(); wb.release();                                      // (two passes: the result is back in recs / wts)
    const u64 avg = n >> gbits;
    const u32 R = lc_rounds(avg, LcsTable::FILL);
    if (R > LC_MAX_ROUNDS) return KATOME_E_UNSUPPORTED;
    DevBuf index(stream);
    KCHECK(index.alloc(((1ull << gbits) + 1) * 8));
    {
        KernelScope ks(K_GROUP_INDEX, stream, n);
        const dim3 igrid(grid_for((1ull << gbits) + 1, BLOCK));
        if (nwk == 1) hipLaunchKernelGGL((hash_group_index_kernel<1, 2>), igrid, dim3(BLOCK), 0, stream, ko, n, gbits, index.as<u64>());
        else          hipLaunchKernelGGL((hash_group_index_kernel<2, 3>), igrid, dim3(BLOCK), 0, stream, ko, n, gbits, index.as<u64>());
    }
    const uint64_t out_cap = ((rc && !list) ? 2 : 1) * n + 2;
    KCHECK(edge_key.alloc(out_cap * 8 * (list ? stride : nwk), stream));
    KCHECK(seq_weight.alloc(out_cap * (list ? 4 : 16), stream));
    LcResult r;
    auto count = [&](u32 rounds, u32 probe_limit) -> int {
        auto launch = [&](auto kernel) {
            return lc_launch(aux, kernel, (size_t)LcsTable::SLOTS * 28, n, r, ko, wo, index.as<u64>(), gbits, rounds, k, seq_per_read, edge_key.as<u64>(),
                             seq_weight.as<u64>(), out_cap, aux.cursor(), aux.distinct(), aux.err(), probe_limit);
        };
        return with_bool(rc, [&](auto rcv) { return with_bool(list, [&](auto lv) { return with_bool(tag.delta, [&](auto dv) {
            constexpr bool RC = decltype(rcv)::value, LIST = decltype(lv)::value, DELTA = decltype(dv)::value;
            return nwk == 1 ? launch(lds_count_seen_kernel<RC, 1, LIST, DELTA>) : launch(lds_count_seen_kernel<RC, 2, LIST, DELTA>);
        }); }); });
    };
    KCHECK(count_optimistic("first-seen order", lc_rounds_try(avg, lc_optimism(), LcsTable::FILL), R, LcsTable::SLOTS, r, count));
    if (r.code == 4 || r.code == 6) return KATOME_E_UNSUPPORTED;
    if (r.code) { set_error("counting in LDS (first-seen order): a sub-round did not fit its table (code %u)", (unsigned)r.code); return KATOME_E_DEVICE; }
    *n_edges = r.n_out; *n_distinct = r.n_distinct;
    return KATOME_OK;
}

// in place: the level's one-word k-mer records in their representative orientation (rep) or back in the canonical one
int table_orient_records(uint64_t* d_keys, uint64_t n, uint32_t k, bool rep, hipStream_t stream) {
    if (!n) return KATOME_OK;
    KernelScope ks(K_RECORDS, stream, n);
    if (rep) hipLaunchKernelGGL(orient_records_kernel<true>, dim3(grid_for(n, BLOCK, 256u * 32u)), dim3(BLOCK), 0, stream, d_keys, n, k);
    else     hipLaunchKernelGGL(orient_records_kernel<false>, dim3(grid_for(n, BLOCK, 256u * 32u)), dim3(BLOCK), 0, stream, d_keys, n, k);
    KCHECK_HIP(hipGetLastError());
    return KATOME_OK;
}

static bool s2_group_sort_on() { static const bool on = env_flag("KATOME_S2_GROUP_SORT", true); return on; }
// KATOME_S2_REGIONS: S2 written by its first partition digit (lds_count_ordered_kernel with REGIONS; one partition pass instead of
// two in half_sort_finish).  0: never; 1: for a level of S2_REGIONS_MIN_RECORDS (2^30) or more; 2: however small (tests).  Not with
// KATOME_S2_GROUP_SORT=0, whose full sort takes S2 as it comes.  KATOME_S2_REGION_CAP=n: no region takes more than n keys (tests of
// the way back)
static bool s2_regions_route(uint64_t n) {
    static const int mode = env_int("KATOME_S2_REGIONS", 1);
    return mode && s2_group_sort_on() && (n >= S2_REGIONS_MIN_RECORDS || mode == 2) && n < (1ull << 32);
}
static uint64_t s2_region_cap_limit() {
    static const uint64_t cap = [] { const char* e = getenv("KATOME_S2_REGION_CAP"); return e ? strtoull(e, nullptr, 10) : UINT64_MAX; }();
    return cap;
}
// The regions of a level of n ordered records ko: their sizes from a sample of the records (s2_regions.h), S2's arrays that large,
// {start, cap} and the cleared cursors on the device.  *on = false: no memory for them (they may exceed the n + 1 keys of the count
// without regions by n / 16 + 512 tiles) -- the caller takes that route, nothing is allocated
static int s2_regions_open(const u64* ko, uint64_t n, uint32_t k, HalfSort& hs, DevBuf& table, DevBuf& cursors, hipStream_t stream, bool* on) {
    *on = false;
    const S2Sample sp = s2_sample_plan(n);
    DevBuf counts(stream);
    KCHECK(counts.alloc(S2_REGIONS * 4));
    KCHECK_HIP(hipMemsetAsync(counts.p, 0, S2_REGIONS * 4, stream));
    hipLaunchKernelGGL(s2_region_sample_kernel, dim3(grid_for(sp.rows, 1)), dim3(BLOCK), 0, stream, ko, n, k, sp.rows, sp.stride, counts.as<u32>());
    KCHECK_HIP(hipGetLastError());
    uint32_t h[S2_REGIONS];
    KCHECK_HIP(hipMemcpyAsync(h, counts.p, sizeof h, hipMemcpyDeviceToHost, stream));
    KCHECK_HIP(hipStreamSynchronize(stream));
    uint32_t cap[2 * S2_REGIONS];          // (the regions' first tiles, and behind them their keys, in one upload)
    {
        uint64_t c[S2_REGIONS];
        s2_region_caps(h, s2_sample_records(n, sp), n, c);
        s2_region_starts(c, hs.region_start);
        for (uint32_t d = 0; d < S2_REGIONS; ++d) {
            cap[d] = (uint32_t)(hs.region_start[d] / S2_REGION_TILE);
            cap[S2_REGIONS + d] = (uint32_t)std::min<uint64_t>(std::min(c[d], s2_region_cap_limit()), UINT32_MAX);
        }
    }
    const uint64_t total = hs.region_start[S2_REGIONS];
    if (hs.s2_key.alloc(total * 8, stream) != KATOME_OK || hs.s2_w.alloc(total * 4, stream) != KATOME_OK || hs.s2_digit.alloc(total, stream) != KATOME_OK ||
        table.alloc(sizeof cap) != KATOME_OK || cursors.alloc((size_t)S2_REGIONS * S2_CURSOR_STEP * 8) != KATOME_OK) {
        hs.s2_key.release(); hs.s2_w.release(); hs.s2_digit.release(); table.release(); cursors.release();
        lc_trace("[half sort] S2 regions: no memory for %llu keys; S2 behind one cursor\n", (unsigned long long)total);
        return KATOME_OK;
    }
    KCHECK_HIP(hipMemcpyAsync(table.p, cap, sizeof cap, hipMemcpyHostToDevice, stream));
    KCHECK_HIP(hipMemsetAsync(cursors.p, 0, cursors.bytes, stream));
    *on = true;
    return KATOME_OK;
}
// ... and the way back when a region filled: S2 again from S1, behind the groups' prefix sums, with its first-pass digits
static int s2_rebuild(HalfSort& hs, uint64_t n_out, uint32_t k, hipStream_t stream) {
    const u64 s2_cap = n_out + 1;
    KCHECK(hs.s2_key.alloc(s2_cap * 8, stream)); KCHECK(hs.s2_w.alloc(s2_cap * 4, stream));
    KCHECK(hs.s2_digit.alloc(dev_digit_stream_bytes(s2_cap, 1), stream));
    DevBuf off(stream);
    KCHECK(off.alloc(((1ull << 16) + 1) * 8));
    KCHECK(dev_scan_counts(hs.group_count.as<u32>(), 1ull << 16, off.as<u64>(), stream));
    hipLaunchKernelGGL(s2_rebuild_kernel, dim3(grid_for(1ull << 16, 1)), dim3(BLOCK), 0, stream, hs.s1_key.as<u64>(), hs.s1_w.as<u32>(), hs.group_first.as<u64>(),
                       hs.group_count.as<u32>(), off.as<u64>(), k, hs.s2_key.as<u64>(), hs.s2_w.as<u32>(), hs.s2_digit.as<uint8_t>(), s2_cap);
    KCHECK_HIP(hipGetLastError());
    return KATOME_OK;
}

// The ordered count of records_to_edges_sorted (lds_count_ordered_kernel).  KATOME_E_UNSUPPORTED: not this way -- the level's shape, a
// group of more distinct keys than the table holds (err 3: key ranges are far less even than hash ranges on skewed or low-complexity
// input) or a count beyond 16 bits (err 5); the records are then still all there, ordered by key, in their representative orientation.
static int ordered_count(DevBuf& keys, DevBuf& weights, uint64_t n, uint32_t k, bool rc, uint32_t min_weight, HalfSort& hs, uint64_t* n_edges,
                         uint64_t* n_distinct, hipStream_t stream, uint32_t* first_counts, RecordSource* src) {
    const bool pending = src && src->pending;          // (the records are still to be made: keys / weights come with the first pass)
    // (one visit per record: a group must fit the 8-byte-slot table at lds_count_packed_kernel's planning load)
    if (!n || (!weights.p && !pending) || k < 9 || 2 * k > 62 || (rc && !(k & 1)) || !lp_group_fits(n >> 16)) {
        if (pending) KCHECK(table_materialise_records(*src));          // (a refusal leaves the records there)
        return KATOME_E_UNSUPPORTED;
    }
    const u64* ko = nullptr; const u32* wo = nullptr;
    {
        DevBuf kb(stream), wb(stream);
        KCHECK(kb.alloc((n + 1) * 8)); KCHECK(wb.alloc((n + 1) * 4));
        KCHECK(dev_key_order(keys.as<u64>(), weights.as<u32>(), n, k, kb.as<u64>(), keys.as<u64>(), wb.as<u32>(), weights.as<u32>(), &ko, &wo, stream, first_counts,
                             nullptr, src));
    }
    KCHECK(hs.group_first.alloc(((1ull << 16) + 1) * 8, stream));
    KCHECK(dev_key_group_index(ko, n, 2 * k - 16, hs.group_first.as<u64>(), stream));
    KCHECK(hs.group_count.alloc((1ull << 16) * 4, stream));
    KCHECK_HIP(hipMemsetAsync(hs.group_count.p, 0, (1ull << 16) * 4, stream));
    KCHECK(hs.s1_key.alloc((n + 1) * 8, stream)); KCHECK(hs.s1_w.alloc((n + 1) * 4, stream));
    const u64 s2_cap = rc ? n + 1 : 0;          // (a reverse complement per distinct key: no more than the records)
    bool regions = false;
    DevBuf rg_table(stream), rg_cursors(stream);
    if (rc && s2_regions_route(n)) KCHECK(s2_regions_open(ko, n, k, hs, rg_table, rg_cursors, stream, &regions));
    if (rc && !regions) {
        KCHECK(hs.s2_key.alloc(s2_cap * 8, stream)); KCHECK(hs.s2_w.alloc(s2_cap * 4, stream));
        KCHECK(hs.s2_digit.alloc(dev_digit_stream_bytes(s2_cap, 1), stream));
    }
    LcAux aux(stream);
    KCHECK(aux.buf.alloc(64));
    std::vector<unsigned long long> cursors(regions ? (size_t)S2_REGIONS * S2_CURSOR_STEP : 0);          // (read back with the counters: no sync of their own)
    if (regions) { aux.more = rg_cursors.p; aux.more_host = cursors.data(); aux.more_bytes = cursors.size() * 8; }
    const S2RegionsOut rg{rg_table.as<u32>(), rg_table.as<u32>() + S2_REGIONS, rg_cursors.as<unsigned long long>()};
    LcResult r;
    auto launch = [&](auto kernel, auto... region_out) {
        return lc_launch(aux, kernel, LO_LDS, n, r, ko, wo, hs.group_first.as<u64>(), k,
                         min_weight, hs.s1_key.as<u64>(), hs.s1_w.as<u32>(), hs.group_count.as<u32>(), hs.s2_key.as<u64>(), hs.s2_w.as<u32>(),
                         hs.s2_digit.as<uint8_t>(), s2_cap, aux.cursor(), aux.distinct(), aux.err(), std::min<u32>(lc_probe_limit(), LP_SLOTS), region_out...);
    };
    if (regions) KCHECK(launch(lds_count_ordered_kernel<true, true, S2RegionsOut>, rg));
    else KCHECK(with_bool(rc, [&](auto rcv) { return launch(lds_count_ordered_kernel<decltype(rcv)::value>); }));
    lc_trace("[lds count] in key order, 8-byte slots, 1 visit(s) per record: code %u\n", (unsigned)r.code);
    if (r.code) {
        lc_trace("[lds count] in key order: %s; counting by hash groups\n", r.code == 5 ? "a count over 16 bits" : "a group filled its table");
        hs.release();
        return KATOME_E_UNSUPPORTED;
    }
    if (regions && r.full) {
        lc_trace("[half sort] S2 regions: region %u full; rebuilt from S1\n", (unsigned)(r.full - 1));
        KCHECK(s2_rebuild(hs, r.n_out, k, stream));
    } else if (regions) {
        uint64_t sum = 0;
        for (uint32_t d = 0; d < S2_REGIONS; ++d) sum += hs.region_used[d] = cursors[(size_t)d * S2_CURSOR_STEP];
        if (sum != r.n_out) { set_error("ordered count: the regions hold %llu keys of %llu", (unsigned long long)sum, (unsigned long long)r.n_out); return KATOME_E_DEVICE; }
        uint32_t fullest = 0;          // (how tight the sampled sizes were: the region that used the largest share of its room)
        const auto room = [&](uint32_t d) { return hs.region_start[d + 1] - hs.region_start[d]; };
        for (uint32_t d = 1; d < S2_REGIONS; ++d) if (hs.region_used[d] * room(fullest) > hs.region_used[fullest] * room(d)) fullest = d;
        lc_trace("[half sort] S2 regions: %llu keys of room in all, region %u the fullest with %llu of %llu\n", (unsigned long long)hs.region_start[S2_REGIONS],
                 (unsigned)fullest, (unsigned long long)hs.region_used[fullest], (unsigned long long)room(fullest));
        hs.regions = true;
    }
    hs.n_s1 = r.n_out; hs.n_s2 = rc ? r.n_out : 0; hs.k = k; hs.taken = true;
    *n_edges = hs.n_s1 + hs.n_s2; *n_distinct = r.n_distinct;
    return KATOME_OK;
}

// KATOME_S2_GROUP_SORT=0: S2 sorted in full and half_merge_kernel, as before group_merge_kernel.  KATOME_S2_GROUP_CAP=n: groups of more
// than n keys (and always more than the kernel's LDS holds) take that route too -- tests of the way back
static uint64_t s2_group_cap() {
    static const uint64_t cap = [] {
        const char* e = getenv("KATOME_S2_GROUP_CAP");
        const uint64_t c = e ? strtoull(e, nullptr, 10) : UINT64_MAX;
        return std::min<uint64_t>(c, dev_group_merge_cap());
    }();
    return cap;
}

// S2 ordered per 16-bit group only, in LDS inside the merge (group_merge_kernel), when its largest group fits: two partition passes
// instead of four and no run sort.  Otherwise, or with KATOME_S2_GROUP_SORT=0, S2 is sorted in full and half_merge_kernel merges it
// (a full sort of the partitioned S2 leaves the same groups, so b_first stands).
// KATOME_MERGE_HEADS=0: the merge counts no source run heads for the node numbering (head_counts comes back empty)
int half_sort_finish(HalfSort& hs, DevBuf& edge_key, DevBuf& edge_weight, hipStream_t stream, DevBuf* head_counts) {
    if (head_counts) head_counts->release();
    if (!hs.taken) { set_error("half sort: no ordered count to finish"); return KATOME_E_ARG; }
    const uint32_t k = hs.k;
    DevBuf b_first(stream), a_off(stream);
    KCHECK(b_first.alloc(((1ull << 16) + 1) * 8)); KCHECK(a_off.alloc(((1ull << 16) + 1) * 8));
    bool grouped = false;
    if (hs.n_s2 && s2_group_sort_on()) {
        if (hs.regions) {          // (the count placed S2 by its first digit and left the second pass's digits: that pass alone, into dense arrays)
            DevBuf tk(stream), tw(stream);
            KCHECK(tk.alloc((hs.n_s2 + 1) * 8)); KCHECK(tw.alloc((hs.n_s2 + 1) * 4));
            uint64_t tiles = 0;
            KCHECK(dev_s2_region_pass(hs.s2_key.as<u64>(), hs.s2_w.as<u32>(), hs.s2_digit.as<uint8_t>(), k, hs.region_start, hs.region_used, tk.as<u64>(),
                                      tw.as<u32>(), &tiles, stream));
            lc_trace("[half sort] S2 regions: %llu keys in %llu tiles, one pass, counted from its writer's digits\n", (unsigned long long)hs.n_s2,
                     (unsigned long long)tiles);
            hs.s2_key.adopt(tk); hs.s2_w.adopt(tw);          // (the regions are released)
        } else {
            DevBuf tk(stream), tw(stream);
            KCHECK(tk.alloc((hs.n_s2 + 1) * 8)); KCHECK(tw.alloc((hs.n_s2 + 1) * 4));
            const u64* ko = nullptr; const u32* wo = nullptr;
            KCHECK(dev_key_order(hs.s2_key.as<u64>(), hs.s2_w.as<u32>(), hs.n_s2, k, tk.as<u64>(), hs.s2_key.as<u64>(), tw.as<u32>(),
                                 hs.s2_w.as<u32>(), &ko, &wo, stream, nullptr, hs.s2_digit.as<uint8_t>()));
        }
        hs.s2_digit.release();
        KCHECK(dev_key_group_index(hs.s2_key.as<u64>(), hs.n_s2, 2 * k - 16, b_first.as<u64>(), stream));
        KCHECK(dev_key_group_max(b_first.as<u64>(), a_off.as<u64>(), stream));      // (a_off: scratch until the scan below)
        uint64_t largest = 0;
        KCHECK_HIP(hipMemcpyAsync(&largest, a_off.p, 8, hipMemcpyDeviceToHost, stream));
        KCHECK_HIP(hipStreamSynchronize(stream));
        grouped = largest <= s2_group_cap();
        lc_trace("[half sort] S2: %llu keys, largest group %llu: %s\n", (unsigned long long)hs.n_s2, (unsigned long long)largest,
                 grouped ? "ordered per group in the merge" : "too large for the merge's LDS; sorted in full");
        if (!grouped) KCHECK(dev_sort_bufs(hs.s2_key, &hs.s2_w, hs.n_s2, 1, 2 * k, stream, true));
    } else if (hs.n_s2) {
        KCHECK(dev_sort_bufs(hs.s2_key, &hs.s2_w, hs.n_s2, 1, 2 * k, stream, true));
        KCHECK(dev_key_group_index(hs.s2_key.as<u64>(), hs.n_s2, 2 * k - 16, b_first.as<u64>(), stream));
    } else KCHECK_HIP(hipMemsetAsync(b_first.p, 0, b_first.bytes, stream));
    KCHECK(dev_scan_counts(hs.group_count.as<u32>(), 1ull << 16, a_off.as<u64>(), stream));
    const uint64_t n_out = hs.n_s1 + hs.n_s2;
    KCHECK(edge_key.alloc((n_out + 1) * 8, stream)); KCHECK(edge_weight.alloc((n_out + 1) * 4, stream));
    if (grouped) {
        static const bool heads = env_flag("KATOME_MERGE_HEADS", true);
        if (head_counts && heads && n_out) KCHECK(head_counts->alloc(dev_source_head_blocks(n_out) * 4, stream));
        KCHECK(dev_group_merge(hs.s1_key.as<u64>(), hs.s1_w.as<u32>(), hs.group_first.as<u64>(), hs.group_count.as<u32>(), a_off.as<u64>(),
                               hs.s2_key.as<u64>(), hs.s2_w.as<u32>(), b_first.as<u64>(), k, edge_key.as<u64>(), edge_weight.as<u32>(), n_out, stream,
                               head_counts ? head_counts->as<u32>() : nullptr));
    } else
        KCHECK(dev_half_merge(hs.s1_key.as<u64>(), hs.s1_w.as<u32>(), hs.group_first.as<u64>(), hs.group_count.as<u32>(), a_off.as<u64>(),
                              hs.s2_key.as<u64>(), hs.s2_w.as<u32>(), b_first.as<u64>(), edge_key.as<u64>(), edge_weight.as<u32>(), n_out, stream));
    hs.release();
    return KATOME_OK;
}

// A level ready to be counted: its records ordered by group, the groups' index, where the result goes, and the counters
struct LcLevel {
    LcAux& aux;
    const u64* ko = nullptr; const u32* wo = nullptr;      // the ordered records (wo null: every record counts once)
    bool counted = false;                                  // ... which carry their counts in the key word (counted_key.h; wo null)
    const u64* index = nullptr; u32 gbits = 16;
    uint64_t n; uint32_t k, nw; bool rc; uint32_t min_weight;
    u64* out_keys = nullptr; u32* out_w = nullptr; uint64_t out_cap = 0;
    OwnerSplit* split;
    u64 avg = 0;                                           // records per group
};

// 12-byte slots in `rounds` sub-rounds (lds_count_kernel; keys of two and three words: lds_count_wide_kernel): the smaller table when
// a group fits it in one round (less to clear and to read out per group)
static int count_sub_rounds(const LcLevel& c, u32 rounds, u32 probe_limit, LcResult& r) {
    auto with_table = [&](auto per) {
        constexpr int PER = decltype(per)::value;
        auto launch = [&](auto kernel) {
            return lc_launch(c.aux, kernel, (size_t)LcTable<PER>::SLOTS * 12, c.n, r, c.ko, c.wo, c.index, c.gbits, rounds, c.k, c.min_weight, c.out_keys, c.out_w,
                             c.out_cap, c.aux.cursor(), c.aux.distinct(), c.aux.err(), std::min<u32>(probe_limit, LcTable<PER>::SLOTS), c.aux.owner_cursor(), c.aux.n_owners);
        };
        if (c.nw == 3) return launch(lds_count_wide_kernel<false, PER, 3, false>);      // (a tile level's records are never oriented)
        return with_strands(c.rc, c.k, [&](auto rcv, auto even) {
            constexpr bool RC = decltype(rcv)::value, EVEN_K = decltype(even)::value;
            return c.nw == 1 ? launch(lds_count_kernel<RC, PER, EVEN_K>) : launch(lds_count_wide_kernel<RC, PER, 2, EVEN_K>);
        });
    };
    return c.avg <= LcTable<8>::FILL ? with_table(IntC<8>{}) : with_table(IntC<13>{});
}

// Keys of two and three words: whole keys in the slots when a group's distinct keys fit that smaller table.  How many they are is
// known only by counting: the first 256 groups are counted for it (1/256 of the records, nothing written: out_cap 0).
struct WholeKeys2 {                     // lds_count_full_kernel
    template <int PER> using Table = LfTable<PER>;
    static constexpr int SMALL = 4, LARGE = 7, SLOT_BYTES = 20;
    static constexpr const char* WHAT = "whole keys";
    template <int PER, class... A> static int launch(const LcLevel& c, size_t lds, LcResult& r, u32 groups, A... tail) {
        if (c.counted) return lc_launch(c.aux, lds_count_full_kernel<false, false, PER, true>, lds, c.n, r, c.ko, c.wo, c.index, groups, c.k, c.min_weight, tail...);
        return with_strands(c.rc, c.k, [&](auto rcv, auto even) {
            return lc_launch(c.aux, lds_count_full_kernel<decltype(rcv)::value, decltype(even)::value, PER>, lds, c.n, r, c.ko, c.wo, c.index, groups, c.k, c.min_weight, tail...);
        });
    }
};
struct WholeKeys3 {                     // lds_count_full3_kernel: never oriented, never thresholded -- no k, no min_weight
    template <int PER> using Table = Lf3Table<PER>;
    static constexpr int SMALL = 3, LARGE = 5, SLOT_BYTES = 28;
    static constexpr const char* WHAT = "whole three-word keys";
    template <int PER, class... A> static int launch(const LcLevel& c, size_t lds, LcResult& r, u32 groups, A... tail) {
        return lc_launch(c.aux, lds_count_full3_kernel<PER>, lds, c.n, r, c.ko, c.wo, c.index, groups, tail...);
    }
};
template <class T> static int count_whole_keys(const LcLevel& c, LcResult& r, bool* done) {
    typedef typename T::template Table<T::SMALL> Small; typedef typename T::template Table<T::LARGE> Large;
    if (c.split || c.gbits != 16) return KATOME_OK;
    auto count = [&](u32 groups, u64 cap, bool small) {
        auto go = [&](auto per) {
            typedef typename T::template Table<decltype(per)::value> Tab;
            return T::template launch<decltype(per)::value>(c, (size_t)Tab::SLOTS * T::SLOT_BYTES, r, groups, c.out_keys, c.out_w, cap, c.aux.cursor(), c.aux.distinct(),
                                                            c.aux.err(), std::min<u32>(lc_probe_limit(), Tab::SLOTS));
        };
        return small ? go(IntC<T::SMALL>{}) : go(IntC<T::LARGE>{});
    };
    const u32 all = 1u << c.gbits, sample = 256u;
    bool take = lc_full_mode() == 1, small = lc_full_per() == 4;
    if (lc_full_mode() < 0 && c.avg > 0 && c.avg <= 8ull * Large::FILL) {        // (eight records to a key: more repetition than that is not planned with)
        KCHECK(count(sample, 0, false));
        const u64 per_group = r.n_distinct / sample;
        take = r.code == 0 && per_group <= Large::FILL;
        // (the smaller table only where it stays a third full: at 0.55 -- C3's big tiles -- its longer probe sequences cost more than
        // its shorter clear and read-out save: 16.2 against 15.5 ms; at 0.35 -- k = 63's k-mers -- 4.5 against 4.9.  The three-word
        // table takes the two-word one's rule as it stands)
        if (!lc_full_per()) small = lf_small_table(per_group, Small::SLOTS);
    }
    if (!take) return KATOME_OK;
    KCHECK(count(all, c.out_cap, small));
    lc_trace("[lds count] %s in the slots (%d per thread): code %u\n", T::WHAT, small ? T::SMALL : T::LARGE, (unsigned)r.code);
    if (r.code == 3 && small) {               // (a group of more distinct keys than the sample promised: the larger table)
        KCHECK(count(all, c.out_cap, false));
        lc_trace("[lds count] %s in the slots (%d per thread): code %u\n", T::WHAT, T::LARGE, (unsigned)r.code);
    }
    *done = r.code == 0;
    return KATOME_OK;
}

// One-word k-mers whose groups would take several visits: 8-byte slots, one visit (lds_count_packed_kernel), sized on the guess that
// 56 % of a group's records are distinct (more and the table fills: err 3, then as before).  KATOME_LC_PACKED=0: never
static int count_packed(const LcLevel& c, u32 R_try, LcResult& r, bool* done) {
    static const int packed_mode = env_int("KATOME_LC_PACKED", 1);      // (2: whenever the keys allow -- tests)
    if (c.nw != 1 || c.split || !c.wo || c.gbits != 16 || !(R_try > 1 || packed_mode == 2) || (c.rc && (c.k & 1) == 0)) return KATOME_OK;
    const u32 R_p = lp_rounds(c.avg);
    if (!(packed_mode == 2 || (packed_mode && R_p < R_try))) return KATOME_OK;
    KCHECK(with_bool(c.rc, [&](auto rcv) {
        return lc_launch(c.aux, lds_count_packed_kernel<decltype(rcv)::value>, (size_t)LP_SLOTS * 8, c.n, r, c.ko, c.wo, c.index, R_p, c.k, c.min_weight, c.out_keys,
                         c.out_w, c.out_cap, c.aux.cursor(), c.aux.distinct(), c.aux.err(), std::min<u32>(lc_probe_limit(), LP_SLOTS));
    }));
    lc_trace("[lds count] 8-byte slots, %u visit(s) per record: code %u\n", R_p, (unsigned)r.code);
    *done = r.code == 0;
    if (r.code) lc_trace("[lds count] 8-byte slots: %s; counting with the 12-byte slots\n", r.code == 5 ? "a count beyond 16 bits" : "a table filled");
    return KATOME_OK;
}

// (k-mer, count) records in any order -> oriented edges (both strands with rc, weights summed per k-mer, threshold applied): counted
// by sorting instead of in a table (see lds_count_kernel).  keys/weights: the records (consumed).  KATOME_E_UNSUPPORTED when
// the input is out of the kernels' range (the caller counts in the table instead).
int records_to_edges_sorted(DevBuf& keys, DevBuf& weights, uint64_t n, uint32_t k, bool rc, uint32_t min_weight, DevBuf& edge_key,
                            DevBuf& edge_weight, uint64_t* n_edges, uint64_t* n_distinct, hipStream_t stream, OwnerSplit* split,
                            uint32_t* first_counts, HalfSort* half, RecordSource* src) {
    *n_edges = 0; *n_distinct = 0;
    // (src: records still to be made.  Whatever wants them before the first partition pass has them written here first)
    auto records = [&]() { return src && src->pending ? table_materialise_records(*src) : (int)KATOME_OK; };
    if (half) {
        half->taken = false;
        if (split) KCHECK(records());
        const int orc = split ? KATOME_E_UNSUPPORTED : ordered_count(keys, weights, n, k, rc, min_weight, *half, n_edges, n_distinct, stream, first_counts, src);
        if (orc != KATOME_E_UNSUPPORTED) return orc;
        if (rc) KCHECK(table_orient_records(keys.as<u64>(), n, k, false, stream));      // (the usual route and the table take canonical k-mers)
        first_counts = nullptr;
    }
    const uint32_t nw = (uint32_t)key_words_for_k(k);
    if (nw > 3 || (nw == 3 && (rc || min_weight))) { KCHECK(records()); return KATOME_E_UNSUPPORTED; }      // (three words: tiles of 64..95 bases -- never k-mers, so never oriented)
    if (split && (nw != 1 || rc || min_weight || split->n_parts == 0 || split->n_parts > (uint32_t)KATOME_MAX_RANKS)) {
        set_error("records by owner: one-word k-mers, one record per k-mer"); return KATOME_E_ARG;
    }
    if (!lc_level_fits(n, LcTable<13>::FILL)) { KCHECK(records()); return KATOME_E_UNSUPPORTED; }
    if (split) KCHECK(records());          // (the core's hash: that order reads records)
    LcAux aux(stream);
    LcLevel c{aux};
    c.n = n; c.k = k; c.nw = nw; c.rc = rc; c.min_weight = min_weight; c.split = split;
    // (weights not allocated: every record counts once; the passes move keys only.  Two-word keys: lds_count_wide_kernel)
    const bool unit = weights.p == nullptr && !(src && src->pending);
    // (a list-fed level whose records carry their counts in the key word, counted_key.h: no weights either, until somebody unpacks them)
    c.counted = !split && dev_hash_order_counts_in_key(src, nw, first_counts);
    if (unit && (nw < 2 || split)) { set_error("records without weights: keys of two or three words"); return KATOME_E_ARG; }
    {
        DevBuf kb(stream), wb(stream);
        KCHECK(kb.alloc((n + 1) * 8 * nw));
        if (!unit && !c.counted) KCHECK(wb.alloc((n + 1) * 4));
        // two passes: the first one's output goes to the scratch, the second one's lands in keys / weights again
        if (split) KCHECK(dev_hash_order_core(keys.as<u64>(), weights.as<u32>(), n, split->core_shift, split->core_bases, kb.as<u64>(), keys.as<u64>(), wb.as<u32>(),
                                              weights.as<u32>(), &c.ko, &c.wo, &c.gbits, stream));
        else KCHECK(dev_hash_order(keys.as<u64>(), weights.as<u32>(), n, nw, kb.as<u64>(), keys.as<u64>(), wb.as<u32>(), weights.as<u32>(), &c.ko, &c.wo, &c.gbits, stream, first_counts, src));
    }
    c.avg = n >> c.gbits;
    const u32 fill = c.avg <= LcTable<8>::FILL ? LcTable<8>::FILL : LcTable<13>::FILL;
    const u32 R = lc_rounds(c.avg, fill);          // sub-rounds: a group's share fits even if all new
    if (R > LC_MAX_ROUNDS) return KATOME_E_UNSUPPORTED;
    DevBuf index(stream);
    KCHECK(index.alloc(((1ull << c.gbits) + 1) * 8));
    KCHECK(aux.buf.alloc(64));
    c.index = index.as<u64>();
    {
        KernelScope ks(K_GROUP_INDEX, stream, n);
        const dim3 igrid(grid_for((1ull << c.gbits) + 1, BLOCK));
        if (split)   hipLaunchKernelGGL(core_group_index_kernel, igrid, dim3(BLOCK), 0, stream, c.ko, n, c.gbits, split->core_shift, split->core_bases, index.as<u64>());
        else if (nw == 1) hipLaunchKernelGGL(hash_group_index_kernel<1>, igrid, dim3(BLOCK), 0, stream, c.ko, n, c.gbits, index.as<u64>());
        else if (nw == 3) hipLaunchKernelGGL(hash_group_index_kernel<3>, igrid, dim3(BLOCK), 0, stream, c.ko, n, c.gbits, index.as<u64>());
        else if (c.counted) hipLaunchKernelGGL(counted_group_index_kernel, igrid, dim3(BLOCK), 0, stream, c.ko, n, index.as<u64>());
        else         hipLaunchKernelGGL(hash_group_index_kernel<2>, igrid, dim3(BLOCK), 0, stream, c.ko, n, c.gbits, index.as<u64>());
    }
    c.out_cap = (rc ? 2 : 1) * n + 1;
    KCHECK(edge_key.alloc(c.out_cap * 8 * nw, stream));
    KCHECK(edge_weight.alloc(c.out_cap * 4, stream));
    c.out_keys = edge_key.as<u64>(); c.out_w = edge_weight.as<u32>();
    if (split) {
        KCHECK(aux.owners.alloc((2 * KATOME_MAX_RANKS + 2) * 8));
        aux.index = c.index; aux.gbits = c.gbits; aux.n_owners = split->n_parts;
    }
    LcResult r;
    bool done = false;
    if (nw == 2) KCHECK(count_whole_keys<WholeKeys2>(c, r, &done));
    if (nw == 3) KCHECK(count_whole_keys<WholeKeys3>(c, r, &done));
    if (!done && c.counted) {
        // the way back (the sample said no, KATOME_LC_FULL=0, a table filled, the salt word): the records become plain keys and a weights
        // array where they lie -- the group index holds, the order is the same -- and the kernels below count them as they always did
        if (c.ko != keys.as<u64>()) { set_error("counting in LDS: packed records outside their buffer"); return KATOME_E_DEVICE; }
        KCHECK(weights.alloc((n + 1) * 4, stream));
        KCHECK(dev_counted_unpack(c.ko, n, keys.as<u64>(), weights.as<u32>(), stream));
        lc_trace("[count_in_key] %llu records unpacked into plain keys and a weights array\n", (unsigned long long)n);
        c.wo = weights.as<u32>(); c.counted = false;
    }
    const u32 R_try = lc_rounds_try(c.avg, lc_optimism(), fill);
    if (!done) KCHECK(count_packed(c, R_try, r, &done));
    if (!done) {
        KCHECK(count_optimistic("packed key", R_try, R, ~0u, r, [&](u32 rounds, u32 probe_limit) { return count_sub_rounds(c, rounds, probe_limit, r); }));
        lc_trace("[lds count] 12-byte slots, %u sub-round(s): code %u\n", R, (unsigned)r.code);
        if (r.code == 4) { set_error("counting in LDS: a group of more than 2^20 records"); return KATOME_E_UNSUPPORTED; }          // (a group too large for the representative's 20 bits: the caller counts in the table)
        if (r.code) { set_error("counting in LDS: a sub-round did not fit its table (code %u)", (unsigned)r.code); return KATOME_E_DEVICE; }
    }
    *n_edges = r.n_out; *n_distinct = r.n_distinct;
    if (split) {
        uint64_t hb[2 * KATOME_MAX_RANKS + 2];
        KCHECK_HIP(hipMemcpyAsync(hb, aux.owners.p, sizeof hb, hipMemcpyDeviceToHost, stream));
        KCHECK_HIP(hipStreamSynchronize(stream));
        uint64_t total = 0;
        for (uint32_t p = 0; p < split->n_parts; ++p) {
            split->base[p] = hb[KATOME_MAX_RANKS + 1 + p];
            split->count[p] = hb[p] - split->base[p];
            total += split->count[p];
        }
        *n_edges = total;             // (the records: scattered over the owners' stretches of edge_key / edge_weight)
    }
    return KATOME_OK;
}

// a list-fed two-word level on its own (test entry: see common.h)
int dev_count_in_key_level(const uint64_t* d_tiles, const uint32_t* d_counts, uint64_t n_tiles, uint32_t tile_bases, uint32_t k, uint32_t span, uint32_t stride,
                           bool rc, bool packed, uint64_t* const d_pass_keys[2], uint32_t* const d_pass_weights[2], uint64_t* d_out_keys,
                           uint32_t* d_out_weights, uint64_t* n_out, int* took_packed, hipStream_t stream) {
    *n_out = 0; *took_packed = 0;
    if (key_words_for_k(tile_bases) != 2 || key_words_for_k(k) != 2) { set_error("count in key: tiles and sub-windows of two words"); return KATOME_E_UNSUPPORTED; }
    if (!n_tiles) return KATOME_OK;
    struct Forced { Forced(int v) { dev_count_in_key_force(v); } ~Forced() { dev_count_in_key_force(-1); } } forced(packed ? 1 : 0);
    DevBuf mk(stream), mw(stream), counts(stream), ok(stream), ow(stream);
    RecordSource src;
    u64 n = 0, n_list = 0, distinct = 0;
    KCHECK(table_list_to_records(d_tiles, d_counts, n_tiles, tile_bases, k, span, stride, rc, mk, mw, &n, stream, 0, &counts, false, &src));
    if (!src.pending) { set_error("count in key: the records were written (KATOME_FUSED_RECORDS, KATOME_FUSED_HIST)"); return KATOME_E_UNSUPPORTED; }
    for (int p = 0; p < 2; ++p) { src.tap_keys[p] = d_pass_keys[p]; src.tap_weights[p] = d_pass_weights[p]; }
    *took_packed = dev_hash_order_counts_in_key(&src, 2, counts.as<u32>()) ? 1 : 0;
    TileLevelScope tl;
    KCHECK(records_to_edges_sorted(mk, mw, n, k, false, 0, ok, ow, &n_list, &distinct, stream, nullptr, counts.as<u32>(), nullptr, &src));
    if (n_list > n) { set_error("count in key: %llu distinct keys of %llu records", (unsigned long long)n_list, (unsigned long long)n); return KATOME_E_DEVICE; }
    KCHECK_HIP(hipMemcpyAsync(d_out_keys, ok.p, n_list * 16, hipMemcpyDeviceToDevice, stream));
    KCHECK_HIP(hipMemcpyAsync(d_out_weights, ow.p, n_list * 4, hipMemcpyDeviceToDevice, stream));
    KCHECK_HIP(hipStreamSynchronize(stream));
    *n_out = n_list;
    return KATOME_OK;
}

}  // namespace katome

#ifdef KATOME_LC_PHASES
// (experiment builds only: the clocks added up per phase -- 0-3 lds_count_kernel's clear / insert / read-out + scan / write, 4-7 the
// wide kernel's --, and back to zero)
extern "C" int katome_debug_lc_phases(uint64_t* out16) {
    unsigned long long h[16];
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(katome::lc_phase_cycles), sizeof h) != hipSuccess) return -1;
    for (int i = 0; i < 16; ++i) out16[i] = h[i];
    memset(h, 0, sizeof h);
    return hipMemcpyToSymbol(HIP_SYMBOL(katome::lc_phase_cycles), h, sizeof h) == hipSuccess ? 0 : -1;
}
// (the ordered kernel's read-out step by step: 0 the table into registers and the kept count, 1-5 lds_order.h's count, scan, place, rank
// and write; and back to zero)
extern "C" int katome_debug_lo_phases(uint64_t* out8) {
    unsigned long long h[8];
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(katome::lo_phase_cycles), sizeof h) != hipSuccess) return -1;
    for (int i = 0; i < 8; ++i) out8[i] = h[i];
    memset(h, 0, sizeof h);
    return hipMemcpyToSymbol(HIP_SYMBOL(katome::lo_phase_cycles), h, sizeof h) == hipSuccess ? 0 : -1;
}
#endif
