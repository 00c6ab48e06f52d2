// radix.hip -- hand-written device primitives for gfx950 wave64: LSD radix sort (keys, optional
// u32 values, 64- or 128-bit keys), partition-by-owner (the same pass with a different digit),
// the group merges, unique, scan, rank-in-sorted-array, and the plain gathers.  The graph is read off the
// sorted edges in node_ids.hip and brought into first-seen order in first_seen.hip; the key loads and
// stores all three share are in edge_keys.h.  All streaming, HBM-bound passes; no MFMA (integer keys).
#include <algorithm>
#include <type_traits>

#include "common.h"
#include "counted_key.h"
#include "edge_keys.h"
#include "entry_cut.h"
#include "lds_order.h"
#include "lds_plan.h"
#include "s2_regions.h"

namespace katome {

constexpr int RADIX_BITS = 8;
constexpr int RADIX = 1 << RADIX_BITS;
#ifndef KATOME_SORT_ITEMS
#define KATOME_SORT_ITEMS 16
#endif
#ifndef KATOME_SORT_ITEMS_WIDE
#define KATOME_SORT_ITEMS_WIDE 8
#endif
#ifndef KATOME_SORT_ITEMS_3
#define KATOME_SORT_ITEMS_3 5
#endif
#ifndef KATOME_SORT_WAVES
#define KATOME_SORT_WAVES 4      // workgroups per CU the scatter kernel is compiled for (register budget)
#endif
// keys per thread and per workgroup tile: 4096 one-word keys, 2048 wider ones -- the same 32 KiB of LDS and the same
// 128 bytes per digit run either way (a 64 KiB tile of 128-bit keys left two workgroups per CU: C5's passes 13.5 -> 10 ms)
template <int NW> struct SortTile {
    // (three-word records -- 95-base tiles, two-word keys with a tag: 1280 of them = 30 KiB, four workgroups per CU like the others;
    // at 2048 = 48 KiB there were two)
    static constexpr int ITEMS = NW == 1 ? KATOME_SORT_ITEMS : NW == 2 ? KATOME_SORT_ITEMS_WIDE : KATOME_SORT_ITEMS_3;
    static constexpr int KEYS = BLOCK * ITEMS;
};
// workgroups per offset chunk: the chunk kernel walks a chunk's workgroups serially, the offsets kernel walks the chunks
// serially -- about the square root of the workgroup count keeps both short (4 M keys per chunk at most: < 2^32)
static inline unsigned chunk_blocks_for(unsigned long long nblocks) {
    unsigned c = 64;
    while (c < 1024 && (unsigned long long)c * c < nblocks) c <<= 1;
    return c;
}
static_assert(BLOCK == RADIX, "one thread per digit in the offset kernels");

template <int NW> struct RadixDigit {
    u32 shift, bits;
    __device__ __forceinline__ u32 operator()(const Key<NW>& k) const { return key_digit(k, shift, bits); }
};
template <int NW> struct OwnerDigit {
    u64 n_parts;
    u32 core_shift, core_bases;          // core_bases == 0: owner by the whole key; else kmer_bits.h core_owner
    u32 minimizer = 0;                   // ... or, > 0, by the core's minimizer of that many bases (kmer_bits.h minimizer_owner)
    __device__ __forceinline__ u32 operator()(const Key<NW>& k0) const {
        if (!key_valid(k0)) return (u32)n_parts;
        Key<NW> k = k0;
        k.w[0] &= ~RC_MARK;              // first-seen-order records carry the orientation they dropped: not part of the key
        if (minimizer) return (u32)minimizer_owner(k, core_shift, core_bases, minimizer, n_parts);
        return core_bases ? (u32)core_owner(k, core_shift, core_bases, n_parts) : (u32)whole_key_owner(k, n_parts);
    }
};
// supermer records name their owner themselves (kmer_bits.h): a slot a read did not fill is invalid and goes last
struct SupermerOwnerDigit {
    u32 n_parts;
    __device__ __forceinline__ u32 operator()(const Key<2>& k) const { return key_valid(k) ? supermer_owner(k) : n_parts; }
};
// owner = the part of an ascending list of u64 values a value falls into: bounds[p] = first value of part p + 1
// (n_parts - 1 of them); used to spread sequence numbers over the ranks for a global ranking
struct RangeDigit {
    const u64* bounds; u32 n_parts;
    __device__ __forceinline__ u32 operator()(const Key<1>& k) const {
        u32 p = 0;
        for (u32 i = 0; i + 1 < n_parts; ++i) p += k.w[0] >= bounds[i];
        return p;
    }
};

// table-region digit: the table slot is mulhi(hash, capacity), monotone in the hash, so the top bits of
// the hash name the region of the table a record will land in
template <int NW> struct HashDigit {
    u32 shift;
    __device__ __forceinline__ u32 operator()(const Key<NW>& k) const { return (u32)(hash_key(k) >> shift) & (RADIX - 1); }
};

// the same digit for records that carry one more word behind the k-mer (first-seen builds: the packed sequence numbers travel as
// the record's last word; only the k-mer's NW - 1 words are hashed)
template <int NW> struct HashTaggedDigit {
    u32 shift;
    __device__ __forceinline__ u32 operator()(const Key<NW>& k) const {
        Key<NW - 1> c;
#pragma unroll
        for (int q = 0; q < NW - 1; ++q) c.w[q] = k.w[q];
        return (u32)(hash_key(c) >> shift) & (RADIX - 1);
    }
};

// ... and for a rank's own distinct k-mers on their way to their owners: the digit comes from the hash of the k-mer's CORE, whose
// top bits name the owner (kmer_bits.h core_owner), so that the groups of the LDS count are grouped by owner as well
template <int NW> struct CoreHashDigit {
    u32 shift, core_shift, core_bases;
    __device__ __forceinline__ u32 operator()(const Key<NW>& k) const { return (u32)(core_hash(k, core_shift, core_bases) >> shift) & (RADIX - 1); }
};

// ... and the k-mer level's KEY digit for the ordered count (lds_count.hip, lds_count_ordered_kernel): the records are in their
// representative orientation and ordered by their leading 16 key bits, so that group g is a contiguous key range
struct LevelKeyDigit {
    u32 shift;
    __device__ __forceinline__ u32 operator()(const Key<1>& k) const { return (u32)(k.w[0] >> shift) & (RADIX - 1); }
};

// ... and HashDigit<2> for a record that carries its count in its first word (counted_key.h): the hash is the plain key's
struct CountedDigit {
    u32 shift;
    __device__ __forceinline__ u32 operator()(const Key<2>& k) const { return (u32)(hash_key(counted_plain(k)) >> shift) & (RADIX - 1); }
};

// ---- pass 1: per-workgroup digit histogram -> counts[block][digit] ----------------------------
template <int NW, class Digit>
__global__ __launch_bounds__(BLOCK) void radix_hist_kernel(const u64* __restrict__ keys, u64 n, Digit dg, u32* __restrict__ counts) {
    __shared__ u32 h[RADIX];
    const u32 tid = threadIdx.x;
    h[tid] = 0;
    __syncthreads();
    constexpr int SORT_ITEMS = SortTile<NW>::ITEMS, SORT_TILE = SortTile<NW>::KEYS;
    const u64 base = (u64)blockIdx.x * SORT_TILE;
    // A whole tile (every tile of a pass but its last) loads its keys without a test, so that the loads go out together: behind
    // `if (i < n)` hipcc 7.2 waited for each load before it issued the next, SORT_ITEMS memory latencies in a row instead of one
    if (base + SORT_TILE <= n) {
        Key<NW> key[SORT_ITEMS];
#pragma unroll
        for (int j = 0; j < SORT_ITEMS; ++j) {
#if KATOME_STREAM_LOADS >= 2
            key[j] = load_key_stream<NW>(keys, base + (u64)j * BLOCK + tid);
#else
            key[j] = load_key<NW>(keys, base + (u64)j * BLOCK + tid);
#endif
        }
#pragma unroll
        for (int j = 0; j < SORT_ITEMS; ++j) atomicAdd(&h[dg(key[j])], 1u);
    } else {
        // the pass's last tile (base < n): a thread past the end reads the last key and does not count it
        Key<NW> key[SORT_ITEMS];
#pragma unroll
        for (int j = 0; j < SORT_ITEMS; ++j) {
            const u64 i = base + (u64)j * BLOCK + tid, ic = i < n ? i : n - 1;
#if KATOME_STREAM_LOADS >= 2
            key[j] = load_key_stream<NW>(keys, ic);
#else
            key[j] = load_key<NW>(keys, ic);
#endif
        }
#pragma unroll
        for (int j = 0; j < SORT_ITEMS; ++j) if (base + (u64)j * BLOCK + tid < n) atomicAdd(&h[dg(key[j])], 1u);
    }
    __syncthreads();
    counts[(u64)blockIdx.x * RADIX + tid] = h[tid];
}

// ... the same counts from the pass's digits themselves, one byte per record at the record's index, left there by whoever placed the
// records (radix_scatter_kernel with a next digit, lds_count_ordered_kernel): 1 byte read per record instead of the key's 8 * NW, and no hash.
// A workgroup takes the bytes of one sort tile, VEC of them per load.  The stream is allocated in whole tiles (digit_stream_bytes),
// so the last tile's loads stay inside it; bytes at n and beyond are not counted.
typedef u32 u32x2_t __attribute__((ext_vector_type(2)));
typedef u32 u32x4_t __attribute__((ext_vector_type(4)));
template <int NW> struct DigitVec { typedef u32 T; };                   // 1280 bytes per tile: 320 words
template <> struct DigitVec<1> { typedef u32x4_t T; };                  // 4096 bytes: one 16-byte load per thread
template <> struct DigitVec<2> { typedef u32x2_t T; };                  // 2048 bytes: one 8-byte load per thread
// Where a pass's tiles lie (the SRC of radix_scatter_kernel below).  ArraySource: tile t at records t * SORT_TILE on.  RegionSource
// (round 22): the one-word records lie in the 256 regions of s2_regions.h and the pass walks their used parts as one list of
// LOGICAL tiles in digit order -- tile_first[d] .. tile_first[d + 1] are region d's, the last of them partial --, so that the counts,
// the offsets and the tile order stay what they are for an array and only the tile's address and its records come from the source.
// PLACED: origin(base) of the logical tile at base says where it lies and what it holds.
struct ArraySource {
    static constexpr bool PLACED = false;
    struct Origin {};
    __device__ __forceinline__ Origin origin(u64) const { return Origin{}; }
};
struct RegionSource {
    static constexpr bool PLACED = true;
    const u32* tile_first;          // [S2_REGIONS + 1]
    const u64* start;               // [S2_REGIONS] ...
    const u64* used;                // ... and [S2_REGIONS] behind it
    struct Origin { u64 base; u32 cnt; };
    __device__ __forceinline__ Origin origin(u64 base) const {          // (s2_regions.h, s2_region_tile)
        const u32 t = (u32)(base / S2_REGION_TILE);
        u32 lo = 0, hi = S2_REGIONS;
        while (hi - lo > 1) { const u32 mid = (lo + hi) / 2; if (tile_first[mid] <= t) lo = mid; else hi = mid; }
        const u64 at = (u64)(t - tile_first[lo]) * S2_REGION_TILE, left = used[lo] - at;
        return Origin{start[lo] + at, (u32)(left < S2_REGION_TILE ? left : S2_REGION_TILE)};
    }
};
static_assert(S2_REGION_TILE == (u64)SortTile<1>::KEYS && S2_REGIONS == (u32)RADIX, "a region is whole sort tiles, one region per digit");
// (Src: where tile blockIdx.x lies -- at its own index, or where a RegionSource says)
template <int NW, class Src = ArraySource>
__global__ __launch_bounds__(BLOCK) void digit_hist_kernel(const uint8_t* __restrict__ digits, u64 n, u32* __restrict__ counts, Src from) {
    typedef typename DigitVec<NW>::T V;
    constexpr u32 SORT_TILE = SortTile<NW>::KEYS, VEC = sizeof(V), WORDS = VEC / 4, LOADS = SORT_TILE / VEC;
    static_assert(SORT_TILE % VEC == 0, "whole loads per tile");
    __shared__ u32 h[RADIX];
    const u32 tid = threadIdx.x;
    h[tid] = 0;
    __syncthreads();
    u64 base = (u64)blockIdx.x * SORT_TILE;
    u32 cnt = (u32)((n - base) < (u64)SORT_TILE ? (n - base) : (u64)SORT_TILE);
    if constexpr (Src::PLACED) { const typename Src::Origin at = from.origin(base); base = at.base; cnt = at.cnt; }
    const V* src = reinterpret_cast<const V*>(digits + base);
    for (u32 l = tid; l < LOADS; l += BLOCK) {
        const V v = __builtin_nontemporal_load(src + l);
        u32 w[WORDS];
        __builtin_memcpy(w, &v, VEC);
        const u32 at = l * VEC;
#pragma unroll
        for (u32 q = 0; q < WORDS; ++q) {
#pragma unroll
            for (u32 b = 0; b < 4; ++b)
                if (at + q * 4 + b < cnt) atomicAdd(&h[(w[q] >> (8 * b)) & 255u], 1u);
        }
    }
    __syncthreads();
    counts[(u64)blockIdx.x * RADIX + tid] = h[tid];
}
// Does a first pass that leaves the second one's digits pay for records of nw words?  The byte store costs the scatter about 1.2 ms
// per 10^9 records whatever their width (as many write requests again as the keys'), the byte histogram 0.4; the key-reading
// histogram it replaces costs 1.7 ms per 10^9 one-word records and 3 ms per 10^9 two-word ones, which are also hashed
// (profiles/r11_histogram_reads.md: one-word records came out level, -0.2 ms per C3 build, so they stay on the keys)
constexpr bool digit_stream_pays(int nw) { return nw >= 2; }
bool dev_digit_stream_pays(uint32_t nw) { return digit_stream_pays((int)nw); }
static bool order_trace() {          // KATOME_LC_TRACE: one line per ordered level (tests read them)
    static const bool on = getenv("KATOME_LC_TRACE") != nullptr;
    return on;
}
// bytes of a digit stream for n records of NW words: whole sort tiles (digit_hist_kernel loads whole vectors)
static inline size_t digit_stream_bytes(u64 n, int nw) {
    const u64 tile = nw == 1 ? SortTile<1>::KEYS : nw == 2 ? SortTile<2>::KEYS : SortTile<3>::KEYS;
    return (size_t)((n + tile - 1) / tile * tile);
}

// ---- pass 2a: per chunk of workgroups, per digit: sum; counts become exclusive prefixes inside
// the chunk (u32), chunk_sum[chunk][digit] holds the chunk totals ---------------------------------
__global__ __launch_bounds__(BLOCK) void radix_chunk_kernel(u32* __restrict__ counts, u64 nblocks, u64* __restrict__ chunk_sum, u32 chunk_blocks) {
    const u32 d = threadIdx.x;
    const u64 b0 = (u64)blockIdx.x * chunk_blocks;
    const u64 b1 = b0 + chunk_blocks < nblocks ? b0 + chunk_blocks : nblocks;
    u32 run = 0;
    // (eight rows' loads in flight before the first store: a walk that waited for every load -- 1024 rows, one after the other, with
    // 1.5 workgroups per CU -- took 0.4-0.5 ms per pass)
    constexpr int U = 8;
    u64 b = b0;
    for (; b + U <= b1; b += U) {
        u32 c[U];
#pragma unroll
        for (int j = 0; j < U; ++j) c[j] = counts[(b + j) * RADIX + d];
#pragma unroll
        for (int j = 0; j < U; ++j) { counts[(b + j) * RADIX + d] = run; run += c[j]; }
    }
    for (; b < b1; ++b) {
        u32 c = counts[b * RADIX + d];
        counts[b * RADIX + d] = run;
        run += c;
    }
    chunk_sum[(u64)blockIdx.x * RADIX + d] = run;
}

// ---- pass 2b: one workgroup turns chunk sums into global exclusive offsets, digit-major --------
// chunk_sum[chunk][digit] -> chunk_off[chunk][digit]; digit_total[digit] gets each digit's count
__global__ __launch_bounds__(BLOCK) void radix_offsets_kernel(u64* __restrict__ chunk_sum, u64 nchunks, u64* __restrict__ digit_total) {
    __shared__ u64 tot[RADIX];
    const u32 d = threadIdx.x;
    u64 t = 0;
    for (u64 c = 0; c < nchunks; ++c) t += chunk_sum[c * RADIX + d];
    tot[d] = t;
    if (digit_total) digit_total[d] = t;
    __syncthreads();
    u64 start = 0;
    for (u32 e = 0; e < d; ++e) start += tot[e];
    constexpr int U = 8;                       // (as in radix_chunk_kernel: the loads of eight chunks before the first store)
    u64 c = 0;
    for (; c + U <= nchunks; c += U) {
        u64 v[U];
#pragma unroll
        for (int j = 0; j < U; ++j) v[j] = chunk_sum[(c + j) * RADIX + d];
#pragma unroll
        for (int j = 0; j < U; ++j) { chunk_sum[(c + j) * RADIX + d] = start; start += v[j]; }
    }
    for (; c < nchunks; ++c) {
        u64 v = chunk_sum[c * RADIX + d];
        chunk_sum[c * RADIX + d] = start;
        start += v;
    }
}

// ---- pass 3: stable scatter ----------------------------------------------------------------------
// Each wave owns 1024 consecutive keys of the tile and ranks them 64 at a time with ballot-built
// match masks (rank = keys of the same digit earlier in the wave); a cross-wave prefix gives the
// key's place in the tile's digit-sorted order, the tile is reordered through LDS and written out
// so that consecutive lanes store consecutive addresses of each digit's run.
// STABLE = false (round 4): a pass that nothing depends on the order of -- the FIRST pass of a level's two hash passes and of a sort
// of distinct keys: whatever order the records arrive in is as good as any other -- ranks a record with one LDS atomic on its digit's
// counter instead of the eight ballots of the match step.  Built to close the gap to the pass's memory-pattern ceiling
// (profiles/r04_scatter_ceiling.txt: 0.80 of it) and measured at C3 on one box, A/B/A/B: 203.8 / 205.8 / 207.3 / 205.1 ms per build --
// nothing: the LDS atomics cost what the ballots cost.  Kept behind KATOME_UNSTABLE_FIRST=1, off by default.
// NEXT (round 11): the pass after this one partitions the same records by another digit, nx(key).  The output loop holds the key it
// stores, so it leaves that digit, one byte, at the key's index of next_out, and the next pass counts its tiles from those bytes
// (digit_hist_kernel) instead of reading the keys again.  NoNextDigit: a last pass -- nothing is computed or stored, the code is the
// one the kernel had before.
// SRC (round 15): where the tile's records come from.  ArraySource: keys_in / vals_in at the record's index, the code the kernel had
// before.  ListSource: the records do not exist yet -- record p is sub-window p % span of list entry p / span in its level's
// orientation, with that entry's count (table.hip, list_to_records_kernel) --, and the pass that would read them first cuts them out
// of the list, a fifth or a sixth of the bytes, so that they are neither written nor read back.  The workgroup divides its first
// record's index by span once; a record q places behind that entry's first one lies in entry mulhi(q, inv), inv = 2^32 / span + 1
// (q / span while q * span < 2^32).  Consecutive lanes read the same entry span times over: plain loads, the lines are shared.
struct NoNextDigit {};
// ENTRY (entry_cut.h): the tile's records are cut once per list ENTRY instead of once per record.  Before the ranking loop a thread
// takes whole entries -- one load of the entry, one reverse complement for its span records, shifts by amounts all lanes share -- and
// leaves the records that lie in the tile at their index in the tile's LDS buffer, which is free until the reorder; the ranking loop
// then reads record idx there, neighbouring lanes neighbouring words, and only the count is still fetched per record.  The first and
// the last entry of a tile straddle its ends (neither 4096 nor 2048 is a multiple of 5 or 6): their records outside are dropped.
// The tile, its record order and so the pass's output are what load() gives.
template <int NWT, int NWK, bool RC, bool REP, bool ENTRY_CUT = true> struct ListSource {
    static constexpr bool PLACED = false, ENTRY = ENTRY_CUT, COUNTED = false;
    const u64* tiles; const u32* counts; u32 k, span, stride, inv;
    struct Origin { u64 t0; u32 o0; };
    __device__ __forceinline__ Origin origin(u64 base) const { const u64 t0 = base / span; return Origin{t0, (u32)(base - t0 * span)}; }
    __device__ __forceinline__ void load(const Origin& at, u32 idx, Key<NWK>& key, u32& val) const {
        const u32 q = at.o0 + idx, tr = __umulhi(q, inv), o = q - tr * span;
        const u64 t = at.t0 + tr;
        Key<NWT> tile;
#pragma unroll
        for (int w = 0; w < NWT; ++w) tile.w[w] = tiles[t * NWT + w];
        key = level_orientation<NWK, RC, REP>(sub_window<NWT, NWK>(tile, k, span, stride, o), k);
        val = counts[t];
    }
    // records [0, cnt) of the tile at `at` into skeys[idx * NWK ..]; the caller's barrier ends it
    __device__ __forceinline__ void stage(const Origin& at, u32 cnt, u64* skeys, u32 tid) const {
        const u32 n_ent = (at.o0 + cnt + span - 1) / span;          // (entries that hold a record of the tile: the last is (o0 + cnt - 1) / span)
        for (u32 e = tid; e < n_ent; e += BLOCK) {
            Key<NWT> tile;
#pragma unroll
            for (int w = 0; w < NWT; ++w) tile.w[w] = tiles[(at.t0 + e) * NWT + w];
            const EntryCut<NWT, NWK, RC, REP> cut(tile, k, span, stride);
            const u32 first = e * span - at.o0;                     // (index of the entry's record 0; wraps for records before the tile)
            for (u32 o = 0; o < span; ++o) {
                const u32 idx = first + o;
                if (idx < cnt) {
                    const Key<NWK> x = cut.record(o);
#pragma unroll
                    for (int w = 0; w < NWK; ++w) skeys[idx * NWK + w] = x.w[w];
                }
            }
        }
    }
    __device__ __forceinline__ u32 count_of(const Origin& at, u32 idx) const { return counts[at.t0 + __umulhi(at.o0 + idx, inv)]; }
};
// The keys-only form of ListSource<2, 2, RC, false, true> (counted_key.h): stage() takes the entry's count once, and what it leaves
// in the tile's LDS buffer is counted_pack(record, count).  The pass then moves keys alone (HAS_VAL = false: one trip through the LDS
// buffer, no count fetched per record) with CountedDigit for HashDigit<2>.
template <bool RC> struct CountedListSource {
    static constexpr bool PLACED = false, ENTRY = true, COUNTED = true;
    const u64* tiles; const u32* counts; u32 k, span, stride;
    struct Origin { u64 t0; u32 o0; };
    __device__ __forceinline__ Origin origin(u64 base) const { const u64 t0 = base / span; return Origin{t0, (u32)(base - t0 * span)}; }
    __device__ __forceinline__ void stage(const Origin& at, u32 cnt, u64* skeys, u32 tid) const {
        const u32 n_ent = (at.o0 + cnt + span - 1) / span;
        for (u32 e = tid; e < n_ent; e += BLOCK) {
            Key<2> tile;
            tile.w[0] = tiles[(at.t0 + e) * 2]; tile.w[1] = tiles[(at.t0 + e) * 2 + 1];
            const u32 c = counts[at.t0 + e];
            const EntryCut<2, 2, RC, false> cut(tile, k, span, stride);
            const u32 first = e * span - at.o0;                     // (wraps for records before the tile, as in ListSource)
            for (u32 o = 0; o < span; ++o) {
                const u32 idx = first + o;
                if (idx < cnt) {
                    const Key<2> x = counted_pack(cut.record(o), c);
                    skeys[idx * 2] = x.w[0]; skeys[idx * 2 + 1] = x.w[1];
                }
            }
        }
    }
};
template <class Src, bool LISTED> constexpr bool listed_keys_only() { if constexpr (LISTED) return Src::COUNTED; else return false; }
template <class Next> struct NextDigitOut {
    Next nx; uint8_t* out;
    __device__ __forceinline__ void put(u64 at, u32 d) const { out[at] = (uint8_t)d; }
};
template <> struct NextDigitOut<NoNextDigit> {};
template <int NW, bool HAS_VAL, class Digit, bool STABLE = true, class Next = NoNextDigit, class Src = ArraySource>
__global__ __launch_bounds__(BLOCK, KATOME_SORT_WAVES) void radix_scatter_kernel(const u64* __restrict__ keys_in, const u32* __restrict__ vals_in,
                                                               u64 n, Digit dg, const u32* __restrict__ rel,
                                                               const u64* __restrict__ chunk_off, u64* __restrict__ keys_out,
                                                               u32* __restrict__ vals_out, u32 chunk_blocks, u32 xcd_tiles, NextDigitOut<Next> next, Src src) {
    constexpr bool NEXT = !std::is_same<Next, NoNextDigit>::value, PLACED = Src::PLACED, LISTED = !std::is_same<Src, ArraySource>::value && !PLACED;
    static_assert(!LISTED || HAS_VAL != listed_keys_only<Src, LISTED>(), "a list's records carry its counts: beside the key, or in it");
    constexpr int SORT_ITEMS = SortTile<NW>::ITEMS, SORT_TILE = SortTile<NW>::KEYS;
    extern __shared__ u64 smem[];
    u64* skeys = smem;                                            // [SORT_TILE * NW]; reused for the values afterwards
    __shared__ u32 whist[BLOCK / 64][RADIX];
    __shared__ u32 dstart[RADIX];
    __shared__ u64 gbase[RADIX];
    __shared__ u32 wsum[BLOCK / 64];

    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // Workgroups are dealt out round-robin over the 8 XCDs, each with an L2 of its own; tiles that follow each other write
    // stretches that follow each other in every digit's run.  With xcd_tiles (tiles per XCD) > 0 workgroup i takes tile
    // (i % 8) * xcd_tiles + i / 8, so that an XCD works through consecutive tiles and the halves of a cache line two tiles share
    // meet in ONE L2 instead of being written back from two.
    const u64 bid = xcd_tiles ? (u64)(blockIdx.x & 7u) * xcd_tiles + (blockIdx.x >> 3) : (u64)blockIdx.x;
    const u64 base = bid * SORT_TILE;
    if (base >= n) return;                                  // (the grid is rounded up to 8 x xcd_tiles)
    u32 cnt = (u32)((n - base) < (u64)SORT_TILE ? (n - base) : (u64)SORT_TILE);
    for (u32 i = tid; i < (BLOCK / 64) * RADIX; i += BLOCK) (&whist[0][0])[i] = 0;
    if constexpr (LISTED) if constexpr (Src::ENTRY) src.stage(src.origin(base), cnt, skeys, tid);      // (the records, once per entry; read below)
    __syncthreads();

    Key<NW> key[SORT_ITEMS]; u32 val[SORT_ITEMS]; u32 dig[SORT_ITEMS]; u32 rnk[SORT_ITEMS];
    const u64 lt_mask = lane ? (~0ull >> (64 - lane)) : 0ull;
    const typename Src::Origin from = src.origin(base);
    u64 in0 = base;                                         // (the tile's first record in keys_in / vals_in)
    if constexpr (PLACED) { in0 = from.base; cnt = from.cnt; }
    // Keys alone, read from an array, by a pass that also leaves the next pass's digits: the tile's loads go out before the ranking
    // loop, and a whole tile's (every tile of a pass but its last) without a test.  Inside the loop, behind `if (valid)`, hipcc 7.2
    // waited for each load before it issued the next -- SORT_ITEMS memory latencies to a tile instead of one: 6.7 -> 5.9 ms for the
    // big tiles' first pass at C3 (profiles/load_chains.md).  The same keys-only pass without a next digit waits the same way but
    // already ran at 5.6 ms, and with its loads ahead it did not run faster (5.8), so it keeps the loop as it was; with values the
    // loop's loads already go out in pairs behind partial waits.
    constexpr bool LOAD_AHEAD = !LISTED && !HAS_VAL && !std::is_same<Next, NoNextDigit>::value;
    if constexpr (LOAD_AHEAD) {
        const u64 at = in0 + wave * (64 * SORT_ITEMS) + lane;
        if (cnt == (u32)SORT_TILE) {
#pragma unroll
            for (int j = 0; j < SORT_ITEMS; ++j) {
#if KATOME_STREAM_LOADS >= 1
                key[j] = load_key_stream<NW>(keys_in, at + j * 64);
#else
                key[j] = load_key<NW>(keys_in, at + j * 64);
#endif
            }
        } else {
#pragma unroll
            for (int j = 0; j < SORT_ITEMS; ++j) {
                if (wave * (64 * SORT_ITEMS) + j * 64 + lane < cnt) {
#if KATOME_STREAM_LOADS >= 1
                    key[j] = load_key_stream<NW>(keys_in, at + j * 64);
#else
                    key[j] = load_key<NW>(keys_in, at + j * 64);
#endif
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < SORT_ITEMS; ++j) {
        const u32 idx = wave * (64 * SORT_ITEMS) + j * 64 + lane;
        const bool valid = idx < cnt;
        u32 d = 0;
        if (valid) {
            if constexpr (LISTED) {
                if constexpr (Src::ENTRY) {
#pragma unroll
                    for (int q = 0; q < NW; ++q) key[j].w[q] = skeys[idx * NW + q];
                    if constexpr (HAS_VAL) val[j] = src.count_of(from, idx);
                } else src.load(from, idx, key[j], val[j]);
            } else if constexpr (!LOAD_AHEAD) {
#if KATOME_STREAM_LOADS >= 1
            key[j] = load_key_stream<NW>(keys_in, in0 + idx);
            if (HAS_VAL) val[j] = __builtin_nontemporal_load(&vals_in[in0 + idx]);
#else
            key[j] = load_key<NW>(keys_in, in0 + idx);
            if (HAS_VAL) val[j] = vals_in[in0 + idx];
#endif
            }
            d = dg(key[j]);
        }
        if (!STABLE) {
            dig[j] = d;
            rnk[j] = valid ? atomicAdd(&whist[0][d], 1u) : 0u;       // (place among the tile's records of this digit, in arrival order)
            continue;
        }
        // the lanes of this row that hold the same digit: a lane differs from another where, for some bit, the row's vote on that bit
        // and its own bit disagree.  `mine` is the lane's bit spread over a word (0 / ~0), so a bit costs one compare (the vote), two
        // xors and two ors; as `bit ? vote : ~vote` on 64-bit masks hipcc 7.2 spent eleven VALU operations per bit and so many
        // scalar pairs that the kernel's arguments lived in VGPR lanes (538 v_readlane per tile): 183 -> 117 VALU operations per key
        const u64 vmask = __ballot(valid);
        u32 diff_lo = 0, diff_hi = 0;
#pragma unroll
        for (int b = 0; b < RADIX_BITS; ++b) {
            const u32 mine = (u32)((int)(d << (31 - b)) >> 31);
            const u64 vote = __ballot(mine != 0);
            diff_lo |= (u32)vote ^ mine;
            diff_hi |= (u32)(vote >> 32) ^ mine;
        }
        const u64 m = ~((u64)diff_hi << 32 | diff_lo) & vmask;
        const u32 prior = __popcll(m & lt_mask);
        u32 old = 0;
        if (valid) old = whist[wave][d];
        if (valid && prior == 0) whist[wave][d] = old + __popcll(m);
        dig[j] = d;
        rnk[j] = old + prior;
    }
    __syncthreads();

    {   // thread = digit: wave-exclusive prefixes, tile-wide digit starts, global run bases
        const u32 d = tid;
        u32 run = 0;
        if (!STABLE) { run = whist[0][d]; whist[0][d] = 0; }       // (one counter per digit: the ranks are tile-wide already)
        else {
#pragma unroll
        for (int w = 0; w < BLOCK / 64; ++w) { u32 c = whist[w][d]; whist[w][d] = run; run += c; }
        }
        u32 incl = run;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { u32 v = __shfl_up(incl, o, 64); if (lane >= (u32)o) incl += v; }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        u32 woff = 0;
#pragma unroll
        for (int w = 0; w < BLOCK / 64; ++w) if (w < (int)wave) woff += wsum[w];
        dstart[d] = woff + incl - run;
        gbase[d] = chunk_off[(bid / chunk_blocks) * RADIX + d] + rel[bid * RADIX + d];
    }
    __syncthreads();

    // the tile goes through LDS twice, keys first and then the values through the same buffer: half the LDS per
    // workgroup means twice the workgroups (and bytes in flight) per CU, which is what bounds this kernel
    u32 pos[SORT_ITEMS];
#pragma unroll
    for (int j = 0; j < SORT_ITEMS; ++j) {
        const u32 idx = wave * (64 * SORT_ITEMS) + j * 64 + lane;
        pos[j] = idx < cnt ? dstart[dig[j]] + whist[wave][dig[j]] + rnk[j] : 0;
        if (idx < cnt) {
#pragma unroll
            for (int q = 0; q < NW; ++q) skeys[pos[j] * NW + q] = key[j].w[q];
        }
    }
    __syncthreads();
    u32 dout[SORT_ITEMS];            // digit of the key this thread writes out in row j (needed again for its value)
#pragma unroll
    for (int j = 0; j < SORT_ITEMS; ++j) {
        const u32 i = j * BLOCK + tid;
        dout[j] = 0;
        if (i < cnt) {
            Key<NW> k;
#pragma unroll
            for (int q = 0; q < NW; ++q) k.w[q] = skeys[i * NW + q];
            const u32 d = dg(k);
            dout[j] = d;
            store_key<NW>(keys_out, gbase[d] + (i - dstart[d]), k);
            if constexpr (NEXT) next.put(gbase[d] + (i - dstart[d]), next.nx(k));       // (a hash digit: another byte of the hash dg took)
        }
    }
    if (HAS_VAL) {
        u32* svals = reinterpret_cast<u32*>(smem);
        __syncthreads();
#pragma unroll
        for (int j = 0; j < SORT_ITEMS; ++j) {
            const u32 idx = wave * (64 * SORT_ITEMS) + j * 64 + lane;
            if (idx < cnt) svals[pos[j]] = val[j];
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < SORT_ITEMS; ++j) {
            const u32 i = j * BLOCK + tid;
            if (i < cnt) vals_out[gbase[dout[j]] + (i - dstart[dout[j]])] = svals[i];
        }
    }
}

struct PassBuffers {
    DevBuf counts, chunk, totals;
    // (first: the first pass's digit counts per tile, [nblocks][RADIX], made by whoever wrote the records.  That pass works IN this
    // buffer -- radix_chunk_kernel turns the counts into prefixes in place -- so the buffer's owner must not read it afterwards)
    u32* first = nullptr;
    u64 nblocks = 0, nchunks = 0;
    u32 chunk_blocks = 64;
    int init(u64 n, int nw, hipStream_t stream) {
        counts.stream = chunk.stream = totals.stream = stream;
        const u64 tile = nw == 1 ? SortTile<1>::KEYS : nw == 2 ? SortTile<2>::KEYS : SortTile<3>::KEYS;
        nblocks = (n + tile - 1) / tile;
        chunk_blocks = chunk_blocks_for(nblocks);
        nchunks = (nblocks + chunk_blocks - 1) / chunk_blocks;
        KCHECK(counts.alloc(nblocks * RADIX * sizeof(u32)));
        KCHECK(chunk.alloc(nchunks * RADIX * sizeof(u64)));
        KCHECK(totals.alloc(RADIX * sizeof(u64)));
        return KATOME_OK;
    }
};

// which per-kernel timer (common.h K_*) a pass with this digit reports to
template <class Digit> struct DigitTimers { static constexpr int HIST = K_SORT_HIST, SCATTER = K_SORT_SCATTER; };
template <int NW> struct DigitTimers<HashDigit<NW>> { static constexpr int HIST = K_HASH_HIST, SCATTER = K_HASH_SCATTER; };
template <int NW> struct DigitTimers<HashTaggedDigit<NW>> { static constexpr int HIST = K_HASH_HIST, SCATTER = K_HASH_SCATTER; };
template <> struct DigitTimers<LevelKeyDigit> { static constexpr int HIST = K_HASH_HIST, SCATTER = K_HASH_SCATTER; };
template <> struct DigitTimers<CountedDigit> { static constexpr int HIST = K_HASH_HIST, SCATTER = K_HASH_SCATTER; };
template <int NW> struct DigitTimers<CoreHashDigit<NW>> { static constexpr int HIST = K_HASH_HIST, SCATTER = K_HASH_SCATTER; };
template <int NW> struct DigitTimers<OwnerDigit<NW>> { static constexpr int HIST = K_OWNER_HIST, SCATTER = K_OWNER_SCATTER; };
template <> struct DigitTimers<SupermerOwnerDigit> { static constexpr int HIST = K_OWNER_HIST, SCATTER = K_OWNER_SCATTER; };
template <> struct DigitTimers<RangeDigit> { static constexpr int HIST = K_OWNER_HIST, SCATTER = K_OWNER_SCATTER; };

static bool unstable_first() {
    static const bool on = env_flag("KATOME_UNSTABLE_FIRST", false);      // (off: measured, no gain -- see the kernel)
    return on;
}
// digits_in: this pass's digit of every record, one byte each at the record's index (see digit_hist_kernel) -- the per-tile counts are
// then made from them and the keys are read by the scatter alone.  nx / digits_out: the scatter also leaves the NEXT pass's digits.
// src: the records are made from a list by the scatter itself (ListSource; kin / vin are not read, and the counts must be there)
template <int NW, bool HAS_VAL, class Digit, bool STABLE = true, class Next = NoNextDigit, class Src = ArraySource>
static int radix_pass(const u64* kin, const u32* vin, u64 n, Digit dg, u64* kout, u32* vout, PassBuffers& pb, hipStream_t stream,
                      bool have_counts = false, const uint8_t* digits_in = nullptr, Next nx = Next{}, uint8_t* digits_out = nullptr, Src src = Src{}) {
    if (!std::is_same<Src, ArraySource>::value && !Src::PLACED && !have_counts) { set_error("radix pass: records off a list and no counts of them"); return KATOME_E_ARG; }
    if (pb.nblocks > 0x7fffffffull) { set_error("radix pass: %llu keys exceed the grid limit", (unsigned long long)n); return KATOME_E_ARG; }
    if (!std::is_same<Next, NoNextDigit>::value && !digits_out) { set_error("radix pass: a next digit and nowhere to write it"); return KATOME_E_ARG; }
    dim3 block(BLOCK);
    u32* const counts = have_counts && pb.first ? pb.first : pb.counts.as<u32>();
    if (!have_counts) {          // (have_counts: whoever wrote the records counted this pass's digits per tile as it went -- pb.first, or pb.counts, holds them)
        KernelScope ks(DigitTimers<Digit>::HIST, stream, n);
        if constexpr (Src::PLACED) {
            if (!digits_in) { set_error("radix pass: records in regions and no digits of them"); return KATOME_E_ARG; }
            hipLaunchKernelGGL((digit_hist_kernel<NW, Src>), dim3((unsigned)pb.nblocks), block, 0, stream, digits_in, n, counts, src);
        } else
        if (digits_in) hipLaunchKernelGGL((digit_hist_kernel<NW>), dim3((unsigned)pb.nblocks), block, 0, stream, digits_in, n, counts, ArraySource{});
        else hipLaunchKernelGGL((radix_hist_kernel<NW, Digit>), dim3((unsigned)pb.nblocks), block, 0, stream, kin, n, dg, counts);
    }
    {
        KernelScope ks(K_PASS_OFFSETS, stream, n);
        hipLaunchKernelGGL(radix_chunk_kernel, dim3((unsigned)pb.nchunks), block, 0, stream, counts, pb.nblocks, pb.chunk.as<u64>(), pb.chunk_blocks);
        hipLaunchKernelGGL(radix_offsets_kernel, dim3(1), block, 0, stream, pb.chunk.as<u64>(), pb.nchunks, pb.totals.as<u64>());
    }
    constexpr bool NEXT = !std::is_same<Next, NoNextDigit>::value;
    static_assert(!NEXT || STABLE, "the next digit is written by the stable scatter");
    const size_t lds = (size_t)SortTile<NW>::KEYS * NW * 8;
    if (lds > (64u << 10)) {          // three-word records: 96 KiB of the CU's 160 KiB
        KCHECK_HIP(hipFuncSetAttribute((const void*)radix_scatter_kernel<NW, HAS_VAL, Digit, STABLE, Next, Src>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    }
    {
        static const bool xcd_aware = env_flag("KATOME_XCD_TILES", true);       // (0: workgroup i takes tile i)
        const u32 xcd_tiles = xcd_aware && pb.nblocks >= 64 ? (u32)((pb.nblocks + 7) / 8) : 0u;
        KernelScope ks((!HAS_VAL && DigitTimers<Digit>::SCATTER == K_SORT_SCATTER) ? (int)K_SORT_SCATTER_KEYS : (int)DigitTimers<Digit>::SCATTER, stream, n);
        NextDigitOut<Next> next;
        if constexpr (NEXT) { next.nx = nx; next.out = digits_out; }
        hipLaunchKernelGGL((radix_scatter_kernel<NW, HAS_VAL, Digit, STABLE, Next, Src>), dim3(xcd_tiles ? xcd_tiles * 8u : (unsigned)pb.nblocks), block, lds, stream, kin, vin, n, dg,
                           counts, pb.chunk.as<u64>(), kout, vout, pb.chunk_blocks, xcd_tiles, next, src);
    }
    KCHECK_HIP(hipGetLastError());
    return KATOME_OK;
}

// After a stable sort on the TOP bits only (bits [low, key_bits)) the keys are in order except inside the runs that share
// those bits.  With 8 * passes >= log2(n) top bits such runs are a handful of records wherever the keys are spread out
// (k-mers of a genome: the top 16 bases), so the remaining passes -- half of them for k = 31, three quarters for k = 63 --
// are replaced by ONE streaming pass: every record finds its run by scanning its neighbours in LDS (left while the top
// bits agree, then right), counts the records of the run that must precede it (smaller key, or equal key further left:
// stable) and is written to run start + count.  A workgroup stages its tile plus a halo on both sides; a run that leaves
// the staged window raises `overflow` and the caller falls back to the remaining passes.
#ifndef KATOME_RUN_TILE
#define KATOME_RUN_TILE 4096
#endif
#ifndef KATOME_RUN_HALO
#define KATOME_RUN_HALO 512
#endif
#ifndef KATOME_RUN_TILE_WIDE
#define KATOME_RUN_TILE_WIDE 2048
#endif
// records a workgroup places: 4096 one-word keys (40 KiB staged with the halo), 2048 wider ones (48 KiB; 4096 of them
// took 80 KiB and left one workgroup per CU: C5's run sort 28 -> 15 ms)
template <int NW> struct RunTile { static constexpr u32 KEYS = NW == 1 ? KATOME_RUN_TILE : KATOME_RUN_TILE_WIDE; };
constexpr u32 RUN_HALO = KATOME_RUN_HALO;               // longest run that can be followed on either side
template <int NW, bool HAS_VAL>
__global__ __launch_bounds__(BLOCK) void run_sort_kernel(const u64* __restrict__ keys_in, const u32* __restrict__ vals_in, u64 n, u32 low,
                                                          u64* __restrict__ keys_out, u32* __restrict__ vals_out, u32* __restrict__ overflow) {
    extern __shared__ u64 lk[];                        // [(RUN_TILE + 2 * RUN_HALO) * NW]
    constexpr u32 RUN_TILE = RunTile<NW>::KEYS;
    constexpr u32 SPAN = RUN_TILE + 2 * RUN_HALO, PER = SPAN / BLOCK, OWN = RUN_TILE / BLOCK;
    static_assert(SPAN % BLOCK == 0 && RUN_TILE % BLOCK == 0, "whole rows per thread");
    const u64 n_tiles = (n + RUN_TILE - 1) / RUN_TILE;
    for (u64 tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const u64 t0 = tile * RUN_TILE;
        const u64 g0 = t0 >= RUN_HALO ? t0 - RUN_HALO : 0;
        const u64 t1 = t0 + RUN_TILE < n ? t0 + RUN_TILE : n;
        const u64 g1 = t1 + RUN_HALO < n ? t1 + RUN_HALO : n;
        const u32 cnt = (u32)(g1 - g0), off = (u32)(t0 - g0), own = (u32)(t1 - t0);
        // all loads of the tile are issued before the first one is waited for (a load per loop trip would serialise ~20
        // memory latencies per workgroup and tile)
        Key<NW> stage[PER];
#pragma unroll
        for (u32 r = 0; r < PER; ++r) {
            const u32 j = r * BLOCK + threadIdx.x;
            if (j < cnt) stage[r] = load_key<NW>(keys_in, g0 + j);
        }
        u32 val[OWN];
        if (HAS_VAL) {
#pragma unroll
            for (u32 r = 0; r < OWN; ++r) {
                const u32 i = r * BLOCK + threadIdx.x;
                if (i < own) val[r] = vals_in[t0 + i];
            }
        }
#pragma unroll
        for (u32 r = 0; r < PER; ++r) {
            const u32 j = r * BLOCK + threadIdx.x;
            if (j < cnt) {
#pragma unroll
                for (int q = 0; q < NW; ++q) lk[j * NW + q] = stage[r].w[q];
            }
        }
        __syncthreads();
        // A scan step is one LDS round trip whose result decides whether there is a next one, and a wave scans for as long as
        // its longest run: U records per thread are scanned in lockstep so that U reads are in flight per step
        constexpr u32 U = 8;
        static_assert(OWN % U == 0, "whole groups");
#pragma unroll
        for (u32 r0 = 0; r0 < OWN; r0 += U) {
            Key<NW> key[U], top[U];
            u32 before[U], lo[U], hi[U], live = 0, lost = 0;
#pragma unroll
            for (u32 u = 0; u < U; ++u) {
                const u32 i = (r0 + u) * BLOCK + threadIdx.x, j = off + i;
                before[u] = 0; lo[u] = j; hi[u] = j + 1;
                if (i < own) {
                    live |= 1u << u;
#pragma unroll
                    for (int q = 0; q < NW; ++q) key[u].w[q] = lk[j * NW + q];
                    top[u] = key_shr(key[u], low);
                }
            }
            u32 go = live;
            while (go) {                                // to the left: records of the run with a key <= this one come first
#pragma unroll
                for (u32 u = 0; u < U; ++u) {
                    if (!(go & (1u << u))) continue;
                    if (lo[u] == 0) { if (g0 > 0) lost |= 1u << u; go &= ~(1u << u); continue; }
                    Key<NW> x;
#pragma unroll
                    for (int q = 0; q < NW; ++q) x.w[q] = lk[(lo[u] - 1) * NW + q];
                    if (!key_eq(key_shr(x, low), top[u])) { go &= ~(1u << u); continue; }
                    before[u] += key_lt(key[u], x) ? 0u : 1u;
                    --lo[u];
                }
            }
            go = live;
            while (go) {                                // to the right: only strictly smaller keys
#pragma unroll
                for (u32 u = 0; u < U; ++u) {
                    if (!(go & (1u << u))) continue;
                    if (hi[u] == cnt) { if (g1 < n) lost |= 1u << u; go &= ~(1u << u); continue; }
                    Key<NW> x;
#pragma unroll
                    for (int q = 0; q < NW; ++q) x.w[q] = lk[hi[u] * NW + q];
                    if (!key_eq(key_shr(x, low), top[u])) { go &= ~(1u << u); continue; }
                    before[u] += key_lt(x, key[u]) ? 1u : 0u;
                    ++hi[u];
                }
            }
#pragma unroll
            for (u32 u = 0; u < U; ++u) {
                if (!(live & (1u << u))) continue;
                const u32 j = off + (r0 + u) * BLOCK + threadIdx.x;
                u64 out = g0 + lo[u] + before[u];
                if (lost & (1u << u)) { *overflow = 1; out = g0 + j; }   // (the result is discarded; keep the store in bounds)
                store_key<NW>(keys_out, out, key[u]);
                if (HAS_VAL) vals_out[out] = val[r0 + u];
            }
        }
        __syncthreads();
    }
}

// The same placement without LDS: where the keys are spread out a run is a few records, so a wave takes a stretch of records with
// RW_REACH more on either side and every lane finds its run among its neighbours' keys by wave shuffles -- no staging, no
// round trips to LDS whose results decide whether there is another one.  A run that leaves the shuffled window (or the wave's
// stretch) is walked in global memory by the lanes it concerns (rare: a window of 2 * RW_REACH + 1 records of equal top bits);
// one longer than RW_LONGEST raises `overflow` like the staged kernel.
constexpr u32 RW_REACH = 7, RW_OWN = 64 - 2 * RW_REACH, RW_LONGEST = 1u << 12;
template <int NW> __device__ __forceinline__ Key<NW> shfl_key_up(const Key<NW>& k, u32 s) {
    Key<NW> r;
#pragma unroll
    for (int q = 0; q < NW; ++q) r.w[q] = __shfl_up(k.w[q], s, 64);
    return r;
}
template <int NW> __device__ __forceinline__ Key<NW> shfl_key_down(const Key<NW>& k, u32 s) {
    Key<NW> r;
#pragma unroll
    for (int q = 0; q < NW; ++q) r.w[q] = __shfl_down(k.w[q], s, 64);
    return r;
}
template <int NW, bool HAS_VAL>
__global__ __launch_bounds__(BLOCK) void run_sort_wave_kernel(const u64* __restrict__ keys_in, const u32* __restrict__ vals_in, u64 n, u32 low,
                                                               u64* __restrict__ keys_out, u32* __restrict__ vals_out, u32* __restrict__ overflow) {
    const u32 lane = threadIdx.x & 63;
    const u64 n_chunks = (n + RW_OWN - 1) / RW_OWN;
    // every XCD (workgroup index mod 8) works through its own eighth of the stretches: neighbouring stretches share cache lines,
    // which then meet in one L2 (see radix_scatter_kernel); the grid is a multiple of 8 workgroups
    const u64 per_xcd = (n_chunks + 7) / 8, xcd = blockIdx.x & 7u;
    const u64 wave = ((u64)(blockIdx.x >> 3) * BLOCK + threadIdx.x) >> 6, n_waves = ((u64)(gridDim.x >> 3) * BLOCK) >> 6;
    const u64 c_end = (xcd + 1) * per_xcd < n_chunks ? (xcd + 1) * per_xcd : n_chunks;
    // A wave works through a CONTIGUOUS block of stretches (round 4): the 2 * RW_REACH records two neighbouring stretches share are
    // then in this wave's own registers -- the last lanes of the stretch before -- and every key is fetched once (with the stretches
    // dealt out round-robin the halo was fetched again by another wave: 1.5 x the algorithmic read, profiles/r03_summary.md).
    const u64 per_wave = (per_xcd + n_waves - 1) / n_waves;
    const u64 c_first = xcd * per_xcd + wave * per_wave, c_last = c_first + per_wave < c_end ? c_first + per_wave : c_end;
    // (the next stretch's loads are issued before this one is worked on; `all`: every lane loads, else only the lanes whose record the
    // stretch before did not hold)
    auto fetch = [&](u64 c, bool all, Key<NW>& key, u32& val) {
        const long long j = (long long)(c * RW_OWN) - (long long)RW_REACH + (long long)lane;
        const bool there = c < n_chunks && j >= 0 && (u64)j < n, fresh = there && (all || lane >= 2 * RW_REACH);
#pragma unroll
        for (int q = 0; q < NW; ++q) key.w[q] = 0;
        val = 0;
        // (a value is only ever read by the lane that owns its record: every own lane loads its own, carried key or not)
#if KATOME_STREAM_LOADS >= 3
        if (fresh) key = load_key_stream<NW>(keys_in, (u64)j);
        if (HAS_VAL && there && lane >= RW_REACH && lane < RW_REACH + RW_OWN) val = __builtin_nontemporal_load(&vals_in[j]);
#else
        if (fresh) key = load_key<NW>(keys_in, (u64)j);
        if (HAS_VAL && there && lane >= RW_REACH && lane < RW_REACH + RW_OWN) val = vals_in[j];
#endif
    };
    Key<NW> key_next; u32 val_next;
    fetch(c_first < c_last ? c_first : n_chunks, true, key_next, val_next);
    for (u64 c = c_first; c < c_last; ++c) {
        const long long j = (long long)(c * RW_OWN) - (long long)RW_REACH + (long long)lane;         // the record this lane looks at
        const bool there = j >= 0 && (u64)j < n;
        const bool own = there && lane >= RW_REACH && lane < RW_REACH + RW_OWN;
        const Key<NW> key = key_next;
        const u32 val = val_next;
        fetch(c + 1 < c_last ? c + 1 : n_chunks, false, key_next, val_next);
        {   // the first 2 * RW_REACH records of the next stretch are this stretch's last ones: lane l takes lane l + RW_OWN's
            Key<NW> carried;
#pragma unroll
            for (int q = 0; q < NW; ++q) carried.w[q] = __shfl(key.w[q], (int)((lane + RW_OWN) & 63u), 64);
            if (lane < 2 * RW_REACH && c + 1 < c_last) key_next = carried;
        }
        const Key<NW> top = key_shr(key, low);
        // to the left: records of the run with a key <= this one come first; to the right: only strictly smaller keys
        u32 left = 0, before = 0;
        bool open = there, more_left = false, more_right = false;
#pragma unroll
        for (u32 s = 1; s <= RW_REACH; ++s) {
            const Key<NW> x = shfl_key_up<NW>(key, s);
            const bool has = lane >= s && j - (long long)s >= 0;
            const bool same = open && has && key_eq(key_shr(x, low), top);
            left += same ? 1u : 0u;
            before += (same && !key_lt(key, x)) ? 1u : 0u;
            open = same;
        }
        more_left = open && j - (long long)RW_REACH > 0;              // the window ended inside the run
        open = there;
#pragma unroll
        for (u32 s = 1; s <= RW_REACH; ++s) {
            const Key<NW> x = shfl_key_down<NW>(key, s);
            const bool has = lane + s < 64 && (u64)j + s < n;
            const bool same = open && has && key_eq(key_shr(x, low), top);
            before += (same && key_lt(x, key)) ? 1u : 0u;
            open = same;
        }
        more_right = open && (u64)j + RW_REACH + 1 < n;
        if (own && (more_left || more_right)) {       // a long run: the rest of it from global memory
            u64 a = (u64)j - left, b = (u64)j + 1;
            u32 steps = 0;
            if (more_left) {
                while (a > 0 && steps < RW_LONGEST) {
                    const Key<NW> x = load_key<NW>(keys_in, a - 1);
                    if (!key_eq(key_shr(x, low), top)) break;
                    before += key_lt(key, x) ? 0u : 1u; ++left; --a; ++steps;
                }
            }
            // (the right side is counted afresh: the window's share of it is in `before` already only for the first RW_REACH records)
            if (more_right) {
                b = (u64)j + RW_REACH + 1;
                while (b < n && steps < RW_LONGEST) {
                    const Key<NW> x = load_key<NW>(keys_in, b);
                    if (!key_eq(key_shr(x, low), top)) break;
                    before += key_lt(x, key) ? 1u : 0u; ++b; ++steps;
                }
            }
            if (steps >= RW_LONGEST) { *overflow = 1; before = left; }       // (the result is discarded; the store stays in bounds)
        }
        if (own) {
            const u64 out = (u64)j - left + before;
            store_key<NW>(keys_out, out, key);
            if (HAS_VAL) vals_out[out] = val;
        }
    }
}

// (A one-kernel pass -- digit offsets of all passes from one read of the keys, tile offsets by decoupled look-back over tiles
// numbered in the order they start -- was built and measured in round 3 and removed again: profiles/r03_lookback.md.  The
// look-back words must be read at agent scope, past the XCD's own L2, and every tile waits for that chain before it can write:
// C3's four sort passes 53 + 10 + 3 ms -> 67 ms (75 ms with eight look-back loads in flight per digit), the two 9-bit hash
// passes 23 + 5 + 1 -> 38 ms.)
// passes over the top bits before the run sort takes over: the fewest with 2^(8 * passes) >= n
static u32 top_passes_for(u64 n) {
    u32 t = 1;
    while (t < 8 && (n >> (8 * t)) != 0) ++t;
    return t;
}

// own_k / own_v (optional): the buffers that hold d_keys / d_vals.  An odd number of passes leaves the result in the
// temporaries; with the owners given they simply take those over (no copy back: 24 B per pair saved).
template <int NW, bool HAS_VAL>
static int sort_t(u64* d_keys, u32* d_vals, u64 n, u32 key_bits, hipStream_t stream, DevBuf* own_k = nullptr, DevBuf* own_v = nullptr,
                  bool distinct_keys = false) {
    if (n < 2) return KATOME_OK;
    PassBuffers pb;
    KCHECK(pb.init(n, NW, stream));
    DevBuf tk(stream), tv(stream);
    KCHECK(tk.alloc(own_k ? std::max<size_t>(n * 8 * NW, own_k->bytes) : n * 8 * NW));       // (a swapped-in buffer must be no smaller)
    if (HAS_VAL) KCHECK(tv.alloc(own_v ? std::max<size_t>(n * 4, own_v->bytes) : n * 4));
    u64* kin = d_keys; u64* kout = tk.as<u64>();
    u32* vin = d_vals; u32* vout = tv.as<u32>();
    auto flip = [&]() { u64* t = kin; kin = kout; kout = t; u32* tv2 = vin; vin = vout; vout = tv2; };
    bool first = true;
    auto pass = [&](u32 shift) -> int {
        RadixDigit<NW> dg{shift, (key_bits - shift) < (u32)RADIX_BITS ? (key_bits - shift) : (u32)RADIX_BITS};
        // (keys that are all different end up in key order whatever order equal DIGITS keep in the first pass; later passes must keep
        // what earlier ones established)
        if (first && distinct_keys && unstable_first()) KCHECK((radix_pass<NW, HAS_VAL, RadixDigit<NW>, false>(kin, vin, n, dg, kout, vout, pb, stream)));
        else KCHECK((radix_pass<NW, HAS_VAL>(kin, vin, n, dg, kout, vout, pb, stream)));
        first = false;
        flip();
        return KATOME_OK;
    };
    const u32 all_passes = (key_bits + RADIX_BITS - 1) / RADIX_BITS, top_passes = top_passes_for(n);
    u32 low = 0;                                            // bits below `low` are left to the run sort
    // the run sort costs about one pass: worth it from two saved passes on
    if (top_passes + 2 <= all_passes && n >= (1u << 16) && !getenv("KATOME_FULL_SORT")) low = key_bits - top_passes * RADIX_BITS;
    for (u32 shift = low; shift < key_bits; shift += RADIX_BITS) KCHECK(pass(shift));
    if (low) {
        DevBuf overflow(stream);
        KCHECK(overflow.alloc(16));
        KCHECK_HIP(hipMemsetAsync(overflow.p, 0, 4, stream));
        constexpr u32 RUN_TILE = RunTile<NW>::KEYS;
        const size_t lds = (size_t)(RUN_TILE + 2 * RUN_HALO) * NW * 8;
        if (lds > (64u << 10)) KCHECK_HIP(hipFuncSetAttribute((const void*)run_sort_kernel<NW, HAS_VAL>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        {
            static const int by_waves = env_int("KATOME_RUN_SORT", 2);      // 1: the staged kernel (A/B)
            KernelScope ks(HAS_VAL ? K_RUN_SORT : K_RUN_SORT_KEYS, stream, n);
            if (by_waves == 2)
                hipLaunchKernelGGL((run_sort_wave_kernel<NW, HAS_VAL>), dim3((grid_for(n, (BLOCK / 64) * RW_OWN * 4, 256u * 32u) + 7u) & ~7u), dim3(BLOCK), 0, stream, kin, vin, n,
                                   low, kout, vout, overflow.as<u32>());
            else
                hipLaunchKernelGGL((run_sort_kernel<NW, HAS_VAL>), dim3(grid_for(n, RUN_TILE, 256u * 16u)), dim3(BLOCK), lds, stream, kin, vin, n, low,
                                   kout, vout, overflow.as<u32>());
        }
        KCHECK_HIP(hipGetLastError());
        u32 h = 0;
        KCHECK_HIP(hipMemcpyAsync(&h, overflow.p, 4, hipMemcpyDeviceToHost, stream));
        KCHECK_HIP(hipStreamSynchronize(stream));
        if (!h) flip();
        else {                                              // a long run of keys sharing their top bits: the passes that were left out, then
            for (u32 shift = 0; shift < low; shift += RADIX_BITS) {      // the top ones again (LSD order)
                RadixDigit<NW> dg{shift, (low - shift) < (u32)RADIX_BITS ? (low - shift) : (u32)RADIX_BITS};
                KCHECK((radix_pass<NW, HAS_VAL>(kin, vin, n, dg, kout, vout, pb, stream)));
                flip();
            }
            for (u32 shift = low; shift < key_bits; shift += RADIX_BITS) KCHECK(pass(shift));
        }
    }
    if (kin != d_keys) {
        if (own_k && (!HAS_VAL || own_v)) {                 // the owners take the temporaries over, the old buffers go back to the cache
            { void* q = tk.take(); const size_t b = own_k->bytes; void* old = own_k->take(); own_k->adopt(q, b); tk.adopt(old, b); }
            if (HAS_VAL) { void* q = tv.take(); const size_t b = own_v->bytes; void* old = own_v->take(); own_v->adopt(q, b); tv.adopt(old, b); }
        } else {
            KCHECK_HIP(hipMemcpyAsync(d_keys, kin, n * 8 * NW, hipMemcpyDeviceToDevice, stream));
            if (HAS_VAL) KCHECK_HIP(hipMemcpyAsync(d_vals, vin, n * 4, hipMemcpyDeviceToDevice, stream));
        }
    }
    return KATOME_OK;      // temporaries go back to the stream-ordered cache
}

// keys (and values) held in DevBufs: sorted "in place" from the caller's point of view, but the buffers may be exchanged for
// the sort's temporaries instead of copied back (pointers taken from them before the call are stale afterwards)
int dev_sort_bufs(DevBuf& keys, DevBuf* vals, uint64_t n, uint32_t nw, uint32_t key_bits, hipStream_t stream, bool distinct_keys) {
    if (nw != 1 && nw != 2) { set_error("key_words must be 1 or 2"); return KATOME_E_ARG; }
    if (key_bits == 0 || key_bits > 64 * nw) { set_error("key_bits out of range"); return KATOME_E_ARG; }
    if (keys.bytes < n * 8 * nw || (vals && vals->bytes < n * 4)) { set_error("sort: buffer too small"); return KATOME_E_ARG; }
    if (nw == 1) return vals ? sort_t<1, true>(keys.as<u64>(), vals->as<u32>(), n, key_bits, stream, &keys, vals, distinct_keys) : sort_t<1, false>(keys.as<u64>(), nullptr, n, key_bits, stream, &keys, nullptr, distinct_keys);
    return vals ? sort_t<2, true>(keys.as<u64>(), vals->as<u32>(), n, key_bits, stream, &keys, vals, distinct_keys) : sort_t<2, false>(keys.as<u64>(), nullptr, n, key_bits, stream, &keys, nullptr, distinct_keys);
}
int dev_sort(uint64_t* d_keys, uint32_t* d_vals, uint64_t n, uint32_t nw, uint32_t key_bits, hipStream_t stream) {
    if (nw != 1 && nw != 2) { set_error("key_words must be 1 or 2"); return KATOME_E_ARG; }
    if (key_bits == 0 || key_bits > 64 * nw) { set_error("key_bits out of range"); return KATOME_E_ARG; }
    if (nw == 1) return d_vals ? sort_t<1, true>(d_keys, d_vals, n, key_bits, stream) : sort_t<1, false>(d_keys, nullptr, n, key_bits, stream);
    return d_vals ? sort_t<2, true>(d_keys, d_vals, n, key_bits, stream) : sort_t<2, false>(d_keys, nullptr, n, key_bits, stream);
}

// group records by owner rank; invalid records go last (part n_parts) and are not counted.
// Optional u32 values travel with their records.
int dev_partition(const uint64_t* d_in, const uint32_t* v_in, uint64_t n, uint32_t nw, uint32_t n_parts, uint64_t* d_out,
                  uint32_t* v_out, uint64_t* h_counts, hipStream_t stream, uint32_t core_shift, uint32_t core_bases, uint32_t minimizer) {
    if (core_bases && (core_shift + 2 * core_bases > 64u * nw || 2 * core_bases > 190)) { set_error("partition: core outside the key"); return KATOME_E_ARG; }
    if (minimizer && (minimizer > 16 || minimizer > core_bases)) { set_error("partition: minimizer longer than the core (or than 16 bases)"); return KATOME_E_ARG; }
    if (n_parts == 0 || n_parts >= (u32)RADIX) { set_error("n_parts must be 1..255"); return KATOME_E_ARG; }
    if (nw < 1 || nw > 3) { set_error("key_words must be 1..3"); return KATOME_E_ARG; }
    if ((v_in == nullptr) != (v_out == nullptr)) { set_error("partition: values in and out must both be given"); return KATOME_E_ARG; }
    for (u32 p = 0; p < n_parts; ++p) h_counts[p] = 0;
    if (n == 0) return KATOME_OK;
    PassBuffers pb;
    KCHECK(pb.init(n, (int)nw, stream));
    if (nw == 1) {
        OwnerDigit<1> dg{n_parts, core_shift, core_bases, minimizer};
        if (v_in) KCHECK((radix_pass<1, true>(d_in, v_in, n, dg, d_out, v_out, pb, stream)));
        else      KCHECK((radix_pass<1, false>(d_in, nullptr, n, dg, d_out, nullptr, pb, stream)));
    } else if (nw == 2) {
        OwnerDigit<2> dg{n_parts, core_shift, core_bases, minimizer};
        if (v_in) KCHECK((radix_pass<2, true>(d_in, v_in, n, dg, d_out, v_out, pb, stream)));
        else      KCHECK((radix_pass<2, false>(d_in, nullptr, n, dg, d_out, nullptr, pb, stream)));
    } else {                          // three-word tiles (k > 32 with a useful span: C5's 90-mers)
        OwnerDigit<3> dg{n_parts, core_shift, core_bases, minimizer};
        if (v_in) KCHECK((radix_pass<3, true>(d_in, v_in, n, dg, d_out, v_out, pb, stream)));
        else      KCHECK((radix_pass<3, false>(d_in, nullptr, n, dg, d_out, nullptr, pb, stream)));
    }
    u64 totals[RADIX];
    KCHECK_HIP(hipMemcpyAsync(totals, pb.totals.p, sizeof totals, hipMemcpyDeviceToHost, stream));
    KCHECK_HIP(hipStreamSynchronize(stream));
    for (u32 p = 0; p < n_parts; ++p) h_counts[p] = totals[p];
    return KATOME_OK;
}

// supermer records (two words, owner inside: kmer_bits.h) grouped by owner; slots left invalid are dropped
int dev_partition_supermers(const uint64_t* d_in, uint64_t n, uint32_t n_parts, uint64_t* d_out, uint64_t* h_counts, hipStream_t stream) {
    if (n_parts == 0 || n_parts > 16) { set_error("supermers: 1..16 owners"); return KATOME_E_ARG; }
    for (u32 p = 0; p < n_parts; ++p) h_counts[p] = 0;
    if (n == 0) return KATOME_OK;
    PassBuffers pb;
    KCHECK(pb.init(n, 2, stream));
    SupermerOwnerDigit dg{n_parts};
    KCHECK((radix_pass<2, false>(d_in, nullptr, n, dg, d_out, nullptr, pb, stream)));
    u64 totals[RADIX];
    KCHECK_HIP(hipMemcpyAsync(totals, pb.totals.p, sizeof totals, hipMemcpyDeviceToHost, stream));
    KCHECK_HIP(hipStreamSynchronize(stream));
    for (u32 p = 0; p < n_parts; ++p) h_counts[p] = totals[p];
    return KATOME_OK;
}

// group u64 values (with their u32 companions) by the range they fall into: part p = [bounds[p-1], bounds[p]), d_bounds on the
// device (n_parts - 1 of them, ascending).  Stable.  Used to spread sequence numbers over the ranks (dist.hip global_rank).
int dev_partition_range(const uint64_t* d_vals, const uint32_t* idx_in, uint64_t n, const uint64_t* d_bounds, uint32_t n_parts,
                        uint64_t* d_out, uint32_t* idx_out, uint64_t* h_counts, hipStream_t stream) {
    if (n_parts == 0 || n_parts >= (u32)RADIX) { set_error("n_parts must be 1..255"); return KATOME_E_ARG; }
    for (u32 p = 0; p < n_parts; ++p) h_counts[p] = 0;
    if (n == 0) return KATOME_OK;
    PassBuffers pb;
    KCHECK(pb.init(n, 1, stream));
    RangeDigit dg{d_bounds, n_parts};
    KCHECK((radix_pass<1, true>(d_vals, idx_in, n, dg, d_out, idx_out, pb, stream)));
    u64 totals[RADIX];
    KCHECK_HIP(hipMemcpyAsync(totals, pb.totals.p, sizeof totals, hipMemcpyDeviceToHost, stream));
    KCHECK_HIP(hipStreamSynchronize(stream));
    for (u32 p = 0; p < n_parts; ++p) h_counts[p] = totals[p];
    return KATOME_OK;
}

// ---- a first pass that makes its records from a list (RecordSource, common.h) ------------------------------------------------------
template <int NWT, int NWK, bool RC, bool REP, bool ENTRY> static ListSource<NWT, NWK, RC, REP, ENTRY> list_source(const RecordSource& s) {
    return ListSource<NWT, NWK, RC, REP, ENTRY>{s.tiles, s.counts, s.k, s.span, s.stride, (u32)((1ull << 32) / s.span) + 1};
}
static bool source_by_key(const RecordSource& s) {          // dev_key_order's first pass can take it
    return s.rep && key_words_for_k(s.k) == 1 && fused_records_takes((u32)key_words_for_k(s.tile_bases), 1, true, s.span);
}
static bool source_by_hash(const RecordSource& s, u32 nw) {          // dev_hash_order's
    return !s.rep && nw == 2 && (u32)key_words_for_k(s.k) == 2 && fused_records_takes((u32)key_words_for_k(s.tile_bases), 2, false, s.span);
}
// the first pass of dev_key_order over the records of s, into ka / wa (pb.first: their counts per tile)
static int list_pass_by_key(const RecordSource& s, u64 n, u32 k, u64* ka, u32* wa, PassBuffers& pb, hipStream_t stream) {
    const LevelKeyDigit dg{2 * k - 16};
    return with_bool(s.rc, [&](auto rcv) { return with_bool(entry_cut_on(), [&](auto cutv) {
        constexpr bool RC = decltype(rcv)::value, CUT = decltype(cutv)::value;
        if (key_words_for_k(s.tile_bases) == 2)
            return radix_pass<1, true, LevelKeyDigit, true, NoNextDigit>(nullptr, nullptr, n, dg, ka, wa, pb, stream, true, nullptr, NoNextDigit{}, nullptr, list_source<2, 1, RC, true, CUT>(s));
        return radix_pass<1, true, LevelKeyDigit, true, NoNextDigit>(nullptr, nullptr, n, dg, ka, wa, pb, stream, true, nullptr, NoNextDigit{}, nullptr, list_source<1, 1, RC, true, CUT>(s));
    }); });
}
// the first pass of dev_hash_order over two-word records of s, leaving the second pass's digits
static int list_pass_by_hash(const RecordSource& s, u64 n, u64* ka, u32* wa, PassBuffers& pb, uint8_t* digits, hipStream_t stream) {
    const HashDigit<2> dg{48u}, nx{56u};
    return with_bool(s.rc, [&](auto rcv) { return with_bool(entry_cut_on(), [&](auto cutv) {
        return radix_pass<2, true, HashDigit<2>, true, HashDigit<2>>(nullptr, nullptr, n, dg, ka, wa, pb, stream, true, nullptr, nx, digits,
                                                                      list_source<2, 2, decltype(rcv)::value, false, decltype(cutv)::value>(s));
    }); });
}

// Does dev_hash_order carry the records of s with their count in the key word (counted_key.h)?  Where its first pass
// makes them off the list, per entry, and their width leaves the room.  KATOME_COUNT_IN_KEY=0: never.  The caller then allocates no
// weights for the level and gets none back; the records it gets are packed.
static int count_in_key_forced = -1;          // (the test entry's flag: 0 / 1 instead of the switch, -1 the switch)
void dev_count_in_key_force(int v) { count_in_key_forced = v; }
static bool count_in_key_on() {
    static const bool on = env_flag("KATOME_COUNT_IN_KEY", true);
    return count_in_key_forced < 0 ? on : count_in_key_forced != 0;
}
static bool list_feeds_hash_order(const RecordSource* src, u32 nw, int passes, const u32* first_counts) {
    return src && src->pending && passes == 2 && first_counts && digit_stream_pays((int)nw) && !unstable_first() && source_by_hash(*src, nw);
}
// Packed records pay where lds_count_full_kernel counts them as they are; where it refuses the level they are unpacked first, a pass
// over all of them (30-fold coverage of 10^9 bases, 2.9 * 10^9 mid records: 722 / 725 -> 730 / 726 ms per build).  It refuses groups
// of more distinct keys than LfTable<7>::FILL, and a level has about as many distinct records as the list it is cut from has
// entries, or more (C3: 1.64 times as many): a list of more entries to a group than that keeps the plain form.  A guess about time
// only -- either form counts any level.
static bool counted_list_small_enough(const RecordSource& s) { return (s.n_tiles >> 16) <= (u64)LfTable<7>::FILL; }
bool dev_hash_order_counts_in_key(const RecordSource* src, uint32_t nw, const uint32_t* first_counts) {
    return list_feeds_hash_order(src, nw, 2, first_counts) && counted_fits(src->k) && entry_cut_on() && count_in_key_on() && counted_list_small_enough(*src);
}
static int tap_records(const RecordSource& s, int pass, const u64* k, const u32* w, u64 n, int nw, hipStream_t stream) {      // (RecordSource::tap_keys)
    if (!s.tap_keys[pass]) return KATOME_OK;
    KCHECK_HIP(hipMemcpyAsync(s.tap_keys[pass], k, n * 8 * nw, hipMemcpyDeviceToDevice, stream));
    KCHECK_HIP(hipMemcpyAsync(s.tap_weights[pass], w, n * 4, hipMemcpyDeviceToDevice, stream));
    return KATOME_OK;
}
// the two passes of that route: the first makes packed records off the list into ka, the second orders them into the source's keys
static int counted_hash_order(RecordSource& s, u64 n, u64* ka, PassBuffers& pb, const u64** k_out, hipStream_t stream) {
    DevBuf digits(stream);
    KCHECK(digits.alloc(digit_stream_bytes(n, 2)));
    const CountedDigit dg{48u}, nx{56u};
    KCHECK(with_bool(s.rc, [&](auto rcv) {
        constexpr bool RC = decltype(rcv)::value;
        return radix_pass<2, false, CountedDigit, true, CountedDigit>(nullptr, nullptr, n, dg, ka, nullptr, pb, stream, true, nullptr, nx, digits.as<uint8_t>(),
                                                                        CountedListSource<RC>{s.tiles, s.counts, s.k, s.span, s.stride});
    }));
    if (s.tap_keys[0]) KCHECK(dev_counted_unpack(ka, n, s.tap_keys[0], s.tap_weights[0], stream));
    s.weight_bytes = 0;          // (no weights on this route; whoever unpacks the records allocates them)
    KCHECK(s.first_pass_done());
    u64* const kb = s.keys->as<u64>();
    KCHECK((radix_pass<2, false, CountedDigit>(ka, nullptr, n, nx, kb, nullptr, pb, stream, false, digits.as<uint8_t>())));
    if (s.tap_keys[1]) KCHECK(dev_counted_unpack(kb, n, s.tap_keys[1], s.tap_weights[1], stream));
    *k_out = kb;
    return KATOME_OK;
}

// order records by the table region they hash to (1 or 2 stable 8-bit passes over the top hash bits), so
// that the insert kernel that follows works through the table one cache-sized region at a time.
// Result lands in `bufs[passes & 1]` where bufs = {scratch_a, scratch_b}; returns that pointer.
template <int NW>
static int region_order_t(const u64* d_in, const u32* w_in, u64 n, int passes, u64* ka, u64* kb, u32* wa, u32* wb,
                          const u64** k_out, const u32** w_out, hipStream_t stream, u32* first_counts = nullptr, RecordSource* src = nullptr) {
    PassBuffers pb;
    KCHECK(pb.init(n, NW, stream));
    // (src: records still to be made.  Where this order's first pass cannot make them, they are written now; either way the input
    // and the second destination are the source's buffers)
    const bool listed = list_feeds_hash_order(src, NW, passes, first_counts);
    if (src && src->pending && order_trace()) {          // (one line per list-fed level: which form its records take)
        const bool counted = passes == 2 && dev_hash_order_counts_in_key(src, NW, first_counts);
        fprintf(stderr, "[count_in_key] %llu records of %u bases: %s\n", (unsigned long long)n, src->k,
                counted ? "count in the key word, no weights array"
                : !listed ? "plain keys and a weights array (records written before their first pass)"
                : !counted_fits(src->k) ? "plain keys and a weights array (no room in the key word)"
                : !entry_cut_on() ? "plain keys and a weights array (KATOME_ENTRY_CUT=0)"
                : !counted_list_small_enough(*src) ? "plain keys and a weights array (more keys to a group than the whole-key table holds)"
                : "plain keys and a weights array (KATOME_COUNT_IN_KEY=0)");
    }
    if (src && src->pending && !listed) {
        KCHECK(table_materialise_records(*src));
        d_in = kb = src->keys->as<u64>(); w_in = wb = src->weights->as<u32>();
    }
    if constexpr (NW == 2) if (passes == 2 && dev_hash_order_counts_in_key(src, NW, first_counts)) {
        pb.first = first_counts;
        if (order_trace())
            fprintf(stderr, "[order] by hash: %llu records of 2 words, first pass counted from its writer's counts, second from the digit stream\n", (unsigned long long)n);
        *w_out = nullptr;
        return counted_hash_order(*src, n, ka, pb, k_out, stream);
    }
    // (first_counts: the first pass's digit counts per tile, [ceil(n / dev_sort_tile_keys)][256], made while the records were written;
    // the pass works in that buffer and leaves prefixes in it)
    pb.first = first_counts;
    DevBuf digits(stream);
    const u64* kin = d_in; const u32* win = w_in;
    u64* kdst[2] = {ka, kb}; u32* wdst[2] = {wa, wb};
    const bool has_w = w_in || listed;          // (a list's records carry its counts)
    for (int p = 0; p < passes; ++p) {
        HashDigit<NW> dg{(u32)(64 - 8 * (passes - p))};     // least significant region byte first
        const bool have = p == 0 && first_counts != nullptr;
        if (order_trace() && passes == 2 && p == 0)
            fprintf(stderr, "[order] by hash: %llu records of %d words, first pass counted from %s, second from %s\n", (unsigned long long)n, NW,
                    have ? "its writer's counts" : "the keys", digit_stream_pays(NW) && !unstable_first() ? "the digit stream" : "the keys");
        if constexpr (digit_stream_pays(NW)) if (passes == 2 && !unstable_first()) {          // (the first pass leaves the second one's digits: no second read of the keys, no second hash)
            if (p == 0) {
                KCHECK(digits.alloc(digit_stream_bytes(n, NW)));
                const HashDigit<NW> nx{56u};
                if (listed) {
                    if constexpr (NW == 2) KCHECK(list_pass_by_hash(*src, n, kdst[0], wdst[0], pb, digits.as<uint8_t>(), stream));
                    KCHECK(tap_records(*src, 0, kdst[0], wdst[0], n, NW, stream));
                    KCHECK(src->first_pass_done());          // (the list may go; the second pass's destination comes only now)
                    kdst[1] = src->keys->as<u64>(); wdst[1] = src->weights->as<u32>();
                    kin = kdst[0]; win = wdst[0];
                    continue;
                }
                if (w_in) KCHECK((radix_pass<NW, true, HashDigit<NW>, true, HashDigit<NW>>(kin, win, n, dg, kdst[0], wdst[0], pb, stream, have, nullptr, nx, digits.as<uint8_t>())));
                else      KCHECK((radix_pass<NW, false, HashDigit<NW>, true, HashDigit<NW>>(kin, nullptr, n, dg, kdst[0], nullptr, pb, stream, have, nullptr, nx, digits.as<uint8_t>())));
            } else {
                if (has_w) KCHECK((radix_pass<NW, true>(kin, win, n, dg, kdst[1], wdst[1], pb, stream, false, digits.as<uint8_t>())));
                else      KCHECK((radix_pass<NW, false>(kin, nullptr, n, dg, kdst[1], nullptr, pb, stream, false, digits.as<uint8_t>())));
            }
            kin = kdst[p & 1]; win = has_w ? wdst[p & 1] : nullptr;
            continue;
        }
        if (p == 0 && unstable_first()) {          // (nothing is ordered yet: the first pass need not be stable)
            if (w_in) KCHECK((radix_pass<NW, true, HashDigit<NW>, false>(kin, win, n, dg, kdst[p & 1], wdst[p & 1], pb, stream, have)));
            else      KCHECK((radix_pass<NW, false, HashDigit<NW>, false>(kin, nullptr, n, dg, kdst[p & 1], nullptr, pb, stream, have)));
        } else
        if (w_in) KCHECK((radix_pass<NW, true>(kin, win, n, dg, kdst[p & 1], wdst[p & 1], pb, stream, have)));
        else      KCHECK((radix_pass<NW, false>(kin, nullptr, n, dg, kdst[p & 1], nullptr, pb, stream, have)));
        kin = kdst[p & 1]; win = w_in ? wdst[p & 1] : nullptr;
    }
    if (listed) KCHECK(tap_records(*src, 1, kin, win, n, NW, stream));
    *k_out = kin; *w_out = win;
    return KATOME_OK;
}
// (k-mer, count) records of one to three words ordered by the top 16 bits of the k-mer's hash, for the counting in LDS (lds_count.hip): two
// stable 8-bit passes.  The result is where *k_out / *w_out point (one of the two buffer pairs); *group_bits = 16.
int dev_hash_order(const uint64_t* d_in, const uint32_t* w_in, uint64_t n, uint32_t nw, uint64_t* ka, uint64_t* kb, uint32_t* wa, uint32_t* wb,
                   const uint64_t** k_out, const uint32_t** w_out, uint32_t* group_bits, hipStream_t stream, uint32_t* first_counts, RecordSource* src) {
    *group_bits = 16;
    if (nw == 1) return region_order_t<1>(d_in, w_in, n, 2, ka, kb, wa, wb, k_out, w_out, stream, first_counts, src);
    if (nw == 3) return region_order_t<3>(d_in, w_in, n, 2, ka, kb, wa, wb, k_out, w_out, stream, first_counts, src);      // (tiles of 64..95 bases)
    return region_order_t<2>(d_in, w_in, n, 2, ka, kb, wa, wb, k_out, w_out, stream, first_counts, src);
}
// one-word (k-mer, count) records ordered by their leading 16 key bits (bits 2k - 16 .. 2k - 1): two stable 8-bit passes, the
// result where *k_out / *w_out point (first_counts: the first pass's digit counts per tile, made while the records were written)
int dev_key_order(const uint64_t* d_in, const uint32_t* w_in, uint64_t n, uint32_t k, uint64_t* ka, uint64_t* kb, uint32_t* wa, uint32_t* wb,
                  const uint64_t** k_out, const uint32_t** w_out, hipStream_t stream, uint32_t* first_counts, const uint8_t* first_digits, RecordSource* src) {
    if (k < 8 || 2 * k > 64) { set_error("key order: k = %u", k); return KATOME_E_ARG; }
    PassBuffers pb;
    KCHECK(pb.init(n, 1, stream));
    pb.first = first_counts;
    // (src: records still to be made -- by the first pass where it can; the second pass's destination is then allocated after it)
    const bool listed = src && src->pending && first_counts && source_by_key(*src);
    if (src && src->pending && !listed) {
        KCHECK(table_materialise_records(*src));
        d_in = kb = src->keys->as<u64>(); w_in = wb = src->weights->as<u32>();
    }
    // (one-word records: digit_stream_pays says no, so the second pass counts from the keys; the first from first_counts, else
    // first_digits, else the keys)
    if (order_trace())
        fprintf(stderr, "[order] by key: %llu records of 1 words, first pass counted from %s, second from the keys\n", (unsigned long long)n,
                first_counts ? "its writer's counts" : first_digits ? "its writer's digits" : "the keys");
    if (listed) {
        KCHECK(list_pass_by_key(*src, n, k, ka, wa, pb, stream));
        KCHECK(src->first_pass_done());
        kb = src->keys->as<u64>(); wb = src->weights->as<u32>();
    } else
    KCHECK((radix_pass<1, true>(d_in, w_in, n, LevelKeyDigit{2 * k - 16}, ka, wa, pb, stream, first_counts != nullptr, first_digits)));
    KCHECK((radix_pass<1, true>(ka, wa, n, LevelKeyDigit{2 * k - 8}, kb, wb, pb, stream)));
    *k_out = kb; *w_out = wb;
    return KATOME_OK;
}

// S2 of the ordered count out of its regions (common.h): the second of dev_key_order's two passes, the first being done by whoever
// placed the keys.  The tile table is made here from the used counts and uploaded with the regions' starts.
int dev_s2_region_pass(const uint64_t* d_keys, const uint32_t* d_w, const uint8_t* d_digits, uint32_t k, const uint64_t* start, const uint64_t* used,
                       uint64_t* k_out, uint32_t* w_out, uint64_t* n_tiles, hipStream_t stream) {
    if (k < 8 || 2 * k > 64) { set_error("region pass: k = %u", k); return KATOME_E_ARG; }
    struct { uint64_t start[S2_REGIONS], used[S2_REGIONS]; uint32_t tile_first[S2_REGIONS + 1]; } h;
    for (u32 d = 0; d < S2_REGIONS; ++d) { h.start[d] = start[d]; h.used[d] = used[d]; }
    s2_region_tiles(used, h.tile_first);
    const u64 tiles = h.tile_first[S2_REGIONS];
    if (n_tiles) *n_tiles = tiles;
    if (!tiles) return KATOME_OK;
    DevBuf table(stream);
    KCHECK(table.alloc(sizeof h));
    KCHECK_HIP(hipMemcpyAsync(table.p, &h, sizeof h, hipMemcpyHostToDevice, stream));
    const RegionSource src{reinterpret_cast<const u32*>(table.as<u64>() + 2 * S2_REGIONS), table.as<u64>(), table.as<u64>() + S2_REGIONS};
    PassBuffers pb;
    const u64 n = tiles * S2_REGION_TILE;          // (the logical tiles' records, the partial tiles counted whole: the source knows what each holds)
    KCHECK(pb.init(n, 1, stream));
    return radix_pass<1, true, LevelKeyDigit, true, NoNextDigit, RegionSource>(d_keys, d_w, n, LevelKeyDigit{2 * k - 8}, k_out, w_out, pb, stream, false, d_digits,
                                                                              NoNextDigit{}, nullptr, src);
}

// the first partition pass over a list's records, both ways (test entry: see common.h)
int dev_list_first_pass(const uint64_t* d_tiles, const uint32_t* d_counts, uint64_t n_tiles, uint32_t tile_bases, uint32_t k, uint32_t span, uint32_t stride,
                        bool rc, bool rep, bool fused, uint64_t* d_keys, uint32_t* d_weights, uint32_t* d_digit_counts, hipStream_t stream) {
    const u32 nwt = (u32)key_words_for_k(tile_bases), nwk = (u32)key_words_for_k(k);
    if (!fused_records_takes(nwt, nwk, rep, span)) { set_error("first pass off a list: tiles of %u words into windows of %u, span %u", nwt, nwk, span); return KATOME_E_UNSUPPORTED; }
    DevBuf rk(stream), rw(stream), counts(stream), digits(stream);
    RecordSource src;
    u64 n = 0;
    KCHECK(table_list_to_records(d_tiles, d_counts, n_tiles, tile_bases, k, span, stride, rc, rk, rw, &n, stream, 0, &counts, rep, fused ? &src : nullptr));
    if (!n) return KATOME_OK;
    if (src.pending != fused || !counts.p) { set_error("first pass off a list: the records were written (KATOME_FUSED_RECORDS, KATOME_FUSED_HIST)"); return KATOME_E_UNSUPPORTED; }
    PassBuffers pb;
    KCHECK(pb.init(n, (int)nwk, stream));
    pb.first = counts.as<u32>();
    KCHECK_HIP(hipMemcpyAsync(d_digit_counts, counts.p, pb.nblocks * RADIX * sizeof(u32), hipMemcpyDeviceToDevice, stream));
    if (rep) {
        if (fused) KCHECK(list_pass_by_key(src, n, k, d_keys, d_weights, pb, stream));
        else KCHECK((radix_pass<1, true>(rk.as<u64>(), rw.as<u32>(), n, LevelKeyDigit{2 * k - 16}, d_keys, d_weights, pb, stream, true)));
    } else {
        KCHECK(digits.alloc(digit_stream_bytes(n, 2)));
        if (fused) KCHECK(list_pass_by_hash(src, n, d_keys, d_weights, pb, digits.as<uint8_t>(), stream));
        else KCHECK((radix_pass<2, true, HashDigit<2>, true, HashDigit<2>>(rk.as<u64>(), rw.as<u32>(), n, HashDigit<2>{48u}, d_keys, d_weights, pb, stream, true, nullptr,
                                                                             HashDigit<2>{56u}, digits.as<uint8_t>())));
    }
    KCHECK_HIP(hipStreamSynchronize(stream));
    return KATOME_OK;
}

// index[g] = first of n ascending-by-leading-bits one-word keys whose bits [shift, shift + 16) are >= g, g = 0 .. 65536
__global__ __launch_bounds__(BLOCK) void key_group_index_kernel(const u64* __restrict__ keys, u64 n, u32 shift, u64* __restrict__ index) {
    for (u64 g = (u64)blockIdx.x * BLOCK + threadIdx.x; g <= (1ull << 16); g += (u64)gridDim.x * BLOCK) {
        u64 lo = 0, hi = n;
        while (lo < hi) {
            const u64 mid = lo + ((hi - lo) >> 1);
            if ((keys[mid] >> shift) < g) lo = mid + 1; else hi = mid;
        }
        index[g] = lo;
    }
}
int dev_key_group_index(const uint64_t* d_keys, uint64_t n, uint32_t shift, uint64_t* d_index, hipStream_t stream) {
    KernelScope ks(K_GROUP_INDEX, stream, n);
    hipLaunchKernelGGL(key_group_index_kernel, dim3(grid_for((1ull << 16) + 1, BLOCK)), dim3(BLOCK), 0, stream, d_keys, n, shift, d_index);
    KCHECK_HIP(hipGetLastError());
    return KATOME_OK;
}

// The edge list of the ordered k-mer count in one streaming pass: for every 16-bit key prefix g, A = the representatives of group g
// (a_key + a_first[g], a_count[g] of them, ascending: lds_count_ordered_kernel) and B = the sorted reverse complements with that
// prefix (b_key + b_first[g] .. b_first[g + 1]) are merged into out + a_off[g] + b_first[g].  A and B are disjoint and every key
// is distinct, so the order is the one a sort of both lists together gives.  A workgroup walks its prefix's two runs through two
// LDS rings of MW keys: each step tops both rings up to MW (or to the run's end), and the first min(MW, loaded) of their merge are
// final -- a key among them from one ring is below every key still unloaded in the other, whose ring is full or done.  Every
// thread places MI outputs by a merge-path search in the rings (MT = 512 threads: 24 waves per CU beside the rings' 48 KiB; with
// 256 threads and 8 outputs each the steps' loads and barriers were not hidden -- 14.6 ms at C3, 2.6 TB/s)
constexpr u32 MW = 2048, MT = 512, MI = MW / MT;
__global__ __launch_bounds__(MT) void half_merge_kernel(const u64* __restrict__ a_key, const u32* __restrict__ a_w, const u64* __restrict__ a_first,
                                                          const u32* __restrict__ a_count, const u64* __restrict__ a_off, const u64* __restrict__ b_key,
                                                          const u32* __restrict__ b_w, const u64* __restrict__ b_first, u64* __restrict__ out_key,
                                                          u32* __restrict__ out_w, u64 out_cap) {
    __shared__ u64 ak[MW], bk[MW];
    __shared__ u32 aw[MW], bw[MW];
    __shared__ u32 used_a;
    const u32 tid = threadIdx.x;
    for (u32 g = blockIdx.x; g < (1u << 16); g += gridDim.x) {
        const u64* ap = a_key + a_first[g]; const u32* awp = a_w + a_first[g];
        const u64 b0 = b_first[g];
        const u64* bp = b_key + b0; const u32* bwp = b_w + b0;
        const u32 na = a_count[g], nb = (u32)(b_first[g + 1] - b0);
        u64 o = a_off[g] + b0;
        u32 ca = 0, cb = 0, la = 0, lb = 0;                   // consumed / loaded of each run
        while (ca < na || cb < nb) {
            const u32 ea = na - ca < MW ? na : ca + MW, eb = nb - cb < MW ? nb : cb + MW;
#pragma unroll 4
            for (u32 i = la + tid; i < ea; i += MT) { ak[i & (MW - 1)] = ap[i]; aw[i & (MW - 1)] = awp[i]; }
#pragma unroll 4
            for (u32 i = lb + tid; i < eb; i += MT) { bk[i & (MW - 1)] = bp[i]; bw[i & (MW - 1)] = bwp[i]; }
            la = ea; lb = eb;
            __syncthreads();
            const u32 va = la - ca, vb = lb - cb, c = va + vb < MW ? va + vb : MW;
            const u32 d0 = tid * MI;
            if (d0 < c) {
                // merge path: the number of A keys among the first d0 outputs
                u32 lo = d0 > vb ? d0 - vb : 0, hi = d0 < va ? d0 : va;
                while (lo < hi) {
                    const u32 m = (lo + hi) >> 1;
                    if (ak[(ca + m) & (MW - 1)] < bk[(cb + d0 - m - 1) & (MW - 1)]) lo = m + 1; else hi = m;
                }
                u32 i = lo, j = d0 - lo;
                const u32 d1 = d0 + MI < c ? d0 + MI : c;
                for (u32 d = d0; d < d1; ++d) {
                    const bool take_a = i < va && (j >= vb || ak[(ca + i) & (MW - 1)] < bk[(cb + j) & (MW - 1)]);
                    u64 key; u32 w;
                    if (take_a) { key = ak[(ca + i) & (MW - 1)]; w = aw[(ca + i) & (MW - 1)]; ++i; }
                    else        { key = bk[(cb + j) & (MW - 1)]; w = bw[(cb + j) & (MW - 1)]; ++j; }
                    if (o + d < out_cap) { out_key[o + d] = key; out_w[o + d] = w; }
                }
                if (d1 == c) used_a = i;                      // (the thread that places the step's last output)
            }
            __syncthreads();
            ca += used_a; cb += c - used_a; o += c;
            __syncthreads();                                  // (used_a is read before the next step's last thread writes it)
        }
    }
}
int dev_half_merge(const uint64_t* a_key, const uint32_t* a_w, const uint64_t* a_first, const uint32_t* a_count, const uint64_t* a_off,
                   const uint64_t* b_key, const uint32_t* b_w, const uint64_t* b_first, uint64_t* out_key, uint32_t* out_w, uint64_t n_out,
                   hipStream_t stream) {
    KernelScope ks(K_HALF_MERGE, stream, n_out);
    hipLaunchKernelGGL(half_merge_kernel, dim3(2048u), dim3(MT), 0, stream, a_key, a_w, a_first, a_count, a_off, b_key, b_w, b_first, out_key, out_w, n_out);
    KCHECK_HIP(hipGetLastError());
    return KATOME_OK;
}

// The same merge without a sort of B (KATOME_S2_GROUP_SORT): the reverse complements are only partitioned by their 16-bit prefix
// (dev_key_order), b_first[g] .. b_first[g + 1] of group g in no order.  A workgroup takes group g and
//   loads   its B keys into registers, GM_PER to a thread, as remainder << 16 | weight: 2k - 16 <= 46 bits of remainder, and a B
//           weight is its representative's count, below 2^16 in the ordered count.  At most GM_CAP of them (the caller checks);
//   orders  them in LDS with the count's read-out (lds_order.h -- the remainders of a group are distinct), in 8192 buckets;
//   merges  them with A[g], in the same form, through an LDS ring of GM_RING = 2 GM_STEP entries.  Every step places GM_STEP outputs
//           (or what is left), GM_MI to a thread after a merge-path search; they are final when the ring holds GM_STEP unconsumed
//           entries or A's end, since B is all in LDS (as in half_merge_kernel).  A is read GM_STEP entries ahead into registers:
//           a block goes into the ring once there is room, and the next block's loads are in flight during the step's merge.
// LDS: 160 KiB -- B (the last 16 words hold the scan's wave totals, the step's A count and HEADS' words, so GM_CAP is 16 short of
// 16 Ki) and the ring, whose first half holds the buckets while B is ordered.  One workgroup of 1024 per CU.
// (-DKATOME_LC_PHASES, experiment builds: the shader clocks of thread 0 per phase -- 0 B's load, 1-5 the ordering's count, scan, place,
// rank and write, 6 the merge steps --, read through katome_debug_gm_phases)
// HEADS: the kernel also counts, per block of SRC_HEAD_BLOCK (source_ids_t's UNIQ_TILE) output edges, the source run heads among them (is_src_head: key >> 2 differs
// from the edge before, or edge 0) into head_counts -- what src_count_kernel would read the whole list again for.  A step's
// outputs [o, o + c), c <= GM_STEP = SRC_HEAD_BLOCK, lie in at most two such blocks; blocks straddle groups that other workgroups merge,
// so head_counts starts at zero and is added to.  Output d is a head iff it is its group's first (the 16-bit prefix changed, and
// 2k - 16 >= 2) or its entry differs from its predecessor's above the weight and the last base (e >> 18).  The predecessor of a
// thread's first output is the larger of the two entries before its merge-path split; of the step's first output, the last output
// of the step before, kept in one of two LDS words by step parity (never ring[ca - 1]: a full ring has overwritten it).
constexpr u32 GM_THREADS = LDS_ORDER_THREADS, GM_PER = 16, GM_WORDS = GM_THREADS * GM_PER, GM_CAP = GM_WORDS - 16;
constexpr u32 GM_STEP = 2048, GM_RING = 2 * GM_STEP, GM_MI = GM_STEP / GM_THREADS, GM_PF = GM_STEP / GM_THREADS;
constexpr size_t GM_LDS = ((size_t)GM_WORDS + GM_RING) * 8;
constexpr u32 GM_LOAD = 8;                    // B key + weight pairs a thread has in flight at once
static_assert(GM_PER % GM_LOAD == 0, "the load of B goes in whole chunks");
constexpr u32 SRC_HEAD_BLOCK = 2048;          // edges to a count of source_ids_t (node_ids.hip: its UNIQ_TILE)
static_assert(SRC_HEAD_BLOCK == UNIQ_TILE, "group_merge_kernel counts the heads of exactly src_count_kernel's blocks");
// the GM_WORDS - GM_CAP spare words behind B, as u32: the scan's wave totals, the step's A count, and (HEADS) the last entry of the
// step before by step parity (two u64, so on an even u32) and the step's two head counts
constexpr u32 GM_SP_WTOT = 0, GM_SP_USED_A = GM_SP_WTOT + GM_THREADS / 64, GM_SP_LAST_E = (GM_SP_USED_A + 1 + 1) / 2 * 2,
              GM_SP_STEP_HEADS = GM_SP_LAST_E + 2 * 2, GM_SP_END = GM_SP_STEP_HEADS + 2;
static_assert(lds_order_words(LDS_ORDER_FINE_BITS) * 4 <= GM_RING * 8 && GM_SP_END <= 2 * (GM_WORDS - GM_CAP), "aliases in the merge's LDS");
#ifdef KATOME_LC_PHASES
__device__ unsigned long long gm_phase_cycles[8];
#define GM_PHASE_BEGIN() unsigned long long gm_t0 = clock64()
#define GM_PHASE(i) do { if (threadIdx.x == 0) { const unsigned long long gm_t = clock64(); atomicAdd(&gm_phase_cycles[i], gm_t - gm_t0); gm_t0 = gm_t; } } while (0)
#else
#define GM_PHASE_BEGIN() do {} while (0)
#define GM_PHASE(i) do {} while (0)
#endif
template <bool HEADS>
__global__ __launch_bounds__(GM_THREADS) void group_merge_kernel(const u64* __restrict__ a_key, const u32* __restrict__ a_w, const u64* __restrict__ a_first,
                                                                   const u32* __restrict__ a_count, const u64* __restrict__ a_off, const u64* __restrict__ b_key,
                                                                   const u32* __restrict__ b_w, const u64* __restrict__ b_first, u32 k,
                                                                   u64* __restrict__ out_key, u32* __restrict__ out_w, u64 out_cap,
                                                                   u32* __restrict__ head_counts) {
    extern __shared__ unsigned long long gm_mem[];
    unsigned long long* bs = gm_mem;                                     // [GM_CAP]: the group's B in key order
    u32* spare = reinterpret_cast<u32*>(gm_mem + GM_CAP);                // (GM_SP_*)
    u32* wtot = spare + GM_SP_WTOT;                                      // [GM_THREADS / 64]
    u32* used_a = spare + GM_SP_USED_A;
    unsigned long long* last_e = reinterpret_cast<unsigned long long*>(spare + GM_SP_LAST_E);      // [2] (HEADS): the last entry placed by the step before, by step parity
    u32* step_heads = spare + GM_SP_STEP_HEADS;                          // [2] (HEADS): this step's heads in its first and its second block
    static_assert(!HEADS || GM_STEP == SRC_HEAD_BLOCK, "a step's outputs lie in at most two blocks of head_counts");
    if (HEADS && threadIdx.x < 2) step_heads[threadIdx.x] = 0u;          // (ordered before the first step by the barriers in between)
    unsigned long long* ring = gm_mem + GM_WORDS;                        // [GM_RING]: A
    u32* bucket = reinterpret_cast<u32*>(ring);                          // [lds_order_words(LDS_ORDER_FINE_BITS)], while B is ordered
    const u32 tid = threadIdx.x;
    const u32 rem_bits = 2 * k - 16, bshift = rem_bits > LDS_ORDER_FINE_BITS ? rem_bits - LDS_ORDER_FINE_BITS : 0;      // (bucket: the remainder's top 13 bits)
    const u64 REM = (1ull << rem_bits) - 1;
    GM_PHASE_BEGIN();
    for (u32 g = blockIdx.x; g < (1u << 16); g += gridDim.x) {
        const u64 b0 = b_first[g], a0 = a_first[g];
        const u32 na = a_count[g], nb = (u32)(b_first[g + 1] - b0);
        const u64* ap = a_key + a0; const u32* awp = a_w + a0;
        u64 o = a_off[g] + b0;
        unsigned long long v[GM_PER]; u32 keep = 0;
#pragma unroll
        for (u32 j = 0; j < GM_PER; ++j) v[j] = 0;
        // (no branch around a load: a lane past the group's end reads the group's last key, which it drops.  Behind `if (i < nb)`
        // hipcc 7.2 waited for each key and weight before it issued the next pair -- up to GM_PER memory latencies a group, and one
        // workgroup to a CU has nobody to hide them.  GM_LOAD pairs go out together, 14.3 -> 13.6 ms at C3 (profiles/load_chains.md);
        // sixteen, 48 registers of loads beside v's 32 under a bound of 128, were not tried.)
        if (nb) {
            const u64 last = b0 + nb - 1;
#pragma unroll
            for (u32 j0 = 0; j0 < GM_PER; j0 += GM_LOAD) {
                if (j0 * GM_THREADS >= nb) break;             // (the whole workgroup is past the end)
                u64 bk[GM_LOAD]; u32 bw[GM_LOAD];
#pragma unroll
                for (u32 j = 0; j < GM_LOAD; ++j) {
                    const u32 i = tid + (j0 + j) * GM_THREADS;
                    const u64 ic = i < nb ? b0 + i : last;
                    bk[j] = b_key[ic]; bw[j] = b_w[ic];
                }
#pragma unroll
                for (u32 j = 0; j < GM_LOAD; ++j) {
                    if (tid + (j0 + j) * GM_THREADS < nb) { v[j0 + j] = ((bk[j] & REM) << 16) | bw[j]; keep |= 1u << (j0 + j); }
                }
            }
        }
        reinterpret_cast<uint4*>(bucket)[tid] = make_uint4(0u, 0u, 0u, 0u);
        __syncthreads();                                  // (the last group's merge is done with the ring and bs)
        GM_PHASE(0);
        lds_order_entries<GM_PER, LDS_ORDER_FINE_BITS>(v, keep, bs, bucket, wtot, bshift, [](u32) {}, [&](u32 i) { GM_PHASE(1 + i); (void)i; });
        // A's next block [la, la + pn) in registers
        u64 pk[GM_PF]; u32 pw[GM_PF];
        u32 ca = 0, cb = 0, la = 0, pn = na < GM_STEP ? na : GM_STEP;          // A consumed and in the ring, B consumed
        u32 step = 0;                                     // (HEADS) steps of this group so far
#pragma unroll
        for (u32 r = 0; r < GM_PF; ++r) { const u32 i = tid + r * GM_THREADS; if (i < pn) { pk[r] = ap[i]; pw[r] = awp[i]; } }
        while (ca < na || cb < nb) {
            if (pn && la - ca + pn <= GM_RING) {          // (otherwise more than GM_STEP are in the ring already)
#pragma unroll
                for (u32 r = 0; r < GM_PF; ++r) {
                    const u32 i = tid + r * GM_THREADS;
                    if (i < pn) ring[(la + i) & (GM_RING - 1)] = ((pk[r] & REM) << 16) | pw[r];
                }
                la += pn;
                pn = na - la < GM_STEP ? na - la : GM_STEP;
#pragma unroll
                for (u32 r = 0; r < GM_PF; ++r) { const u32 i = tid + r * GM_THREADS; if (i < pn) { pk[r] = ap[la + i]; pw[r] = awp[la + i]; } }
            }
            __syncthreads();
            const u32 va = la - ca, vb = nb - cb, c = va + vb < GM_STEP ? va + vb : GM_STEP;
            const u32 d0 = tid * GM_MI;
            u32 h_lo = 0, h_hi = 0;                           // (HEADS) bit r: this thread's output r is a head in the step's first / second block
            if (d0 < c) {
                // merge path: the number of A entries among the first d0 outputs
                u32 lo = d0 > vb ? d0 - vb : 0, hi = d0 < va ? d0 : va;
                while (lo < hi) {
                    const u32 m = (lo + hi) >> 1;
                    if (ring[(ca + m) & (GM_RING - 1)] < bs[cb + d0 - m - 1]) lo = m + 1; else hi = m;
                }
                u32 i = lo, j = d0 - lo;
                const u32 d1 = d0 + GM_MI < c ? d0 + GM_MI : c;
                unsigned long long prev = 0;                  // (HEADS) the entry placed before this thread's next one
                bool first = false;                           // ... or none: the group's first output
                if (HEADS) {
                    if (d0 == 0) { first = step == 0; if (!first) prev = last_e[(step - 1) & 1]; }
                    else {
                        const unsigned long long pa = i ? ring[(ca + i - 1) & (GM_RING - 1)] : 0ull, pb = j ? bs[cb + j - 1] : 0ull;
                        prev = pa > pb ? pa : pb;             // (d0 > 0: one of the two exists, and entries are distinct above bit 16)
                    }
                }
                for (u32 d = d0; d < d1; ++d) {
                    unsigned long long e;
                    if (i < va && (j >= vb || ring[(ca + i) & (GM_RING - 1)] < bs[cb + j])) e = ring[(ca + i++) & (GM_RING - 1)];
                    else e = bs[cb + j++];
                    if (o + d < out_cap) {
                        out_key[o + d] = ((u64)g << rem_bits) | (e >> 16); out_w[o + d] = (u32)e & 0xFFFFu;
                        if (HEADS && (first || (e >> 18) != (prev >> 18))) {
                            if ((o + d) / SRC_HEAD_BLOCK != o / SRC_HEAD_BLOCK) h_hi |= 1u << (d - d0); else h_lo |= 1u << (d - d0);
                        }
                    }
                    if (HEADS) { prev = e; first = false; }
                }
                if (d1 == c) { *used_a = i; if (HEADS) last_e[step & 1] = prev; }      // (the thread that places the step's last output)
            }
            if (HEADS) {
                u32 n_lo = 0, n_hi = 0;
#pragma unroll
                for (u32 r = 0; r < GM_MI; ++r) { n_lo += __popcll(__ballot((h_lo >> r) & 1u)); n_hi += __popcll(__ballot((h_hi >> r) & 1u)); }
                if ((tid & 63) == 0) { if (n_lo) atomicAdd(&step_heads[0], n_lo); if (n_hi) atomicAdd(&step_heads[1], n_hi); }
            }
            __syncthreads();
            const u32 ua = *used_a;
            if (HEADS && tid == 0) {                          // (one thread: a global atomic per touched block and step)
                const u64 blk = o / SRC_HEAD_BLOCK;
                if (step_heads[0]) { atomicAdd(&head_counts[blk], step_heads[0]); step_heads[0] = 0u; }
                if (step_heads[1]) { atomicAdd(&head_counts[blk + 1], step_heads[1]); step_heads[1] = 0u; }
            }
            ca += ua; cb += c - ua; o += c; ++step;
            __syncthreads();                                  // (used_a is read before the next step's last thread writes it)
        }
        GM_PHASE(6);
    }
}
uint32_t dev_group_merge_cap() { return GM_CAP; }
uint64_t dev_source_head_blocks(uint64_t n_edges) { return (n_edges + SRC_HEAD_BLOCK - 1) / SRC_HEAD_BLOCK; }
int dev_group_merge(const uint64_t* a_key, const uint32_t* a_w, const uint64_t* a_first, const uint32_t* a_count, const uint64_t* a_off,
                    const uint64_t* b_key, const uint32_t* b_w, const uint64_t* b_first, uint32_t k, uint64_t* out_key, uint32_t* out_w,
                    uint64_t n_out, hipStream_t stream, uint32_t* head_counts) {
    if (k < 9 || 2 * k > 62) { set_error("group merge: k = %u", k); return KATOME_E_ARG; }
    // (head_counts: ceil(n_out / SRC_HEAD_BLOCK) counts, added to by every workgroup whose group reaches into the block)
    if (head_counts) KCHECK_HIP(hipMemsetAsync(head_counts, 0, dev_source_head_blocks(n_out) * sizeof(u32), stream));
    const auto kernel = head_counts ? group_merge_kernel<true> : group_merge_kernel<false>;
    KCHECK_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)GM_LDS));
    KernelScope ks(K_GROUP_MERGE, stream, n_out);
    hipLaunchKernelGGL(kernel, dim3(256u), dim3(GM_THREADS), GM_LDS, stream, a_key, a_w, a_first, a_count, a_off, b_key, b_w, b_first, k, out_key, out_w, n_out,
                       head_counts);
    KCHECK_HIP(hipGetLastError());
    return KATOME_OK;
}

__global__ __launch_bounds__(BLOCK) void key_group_max_kernel(const u64* __restrict__ index, unsigned long long* __restrict__ out) {
    unsigned long long m = 0;
    for (u32 g = blockIdx.x * BLOCK + threadIdx.x; g < (1u << 16); g += gridDim.x * BLOCK) m = max(m, (unsigned long long)(index[g + 1] - index[g]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned long long)__shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0 && m) atomicMax(out, m);
}
int dev_key_group_max(const uint64_t* d_index, uint64_t* d_out, hipStream_t stream) {
    KCHECK_HIP(hipMemsetAsync(d_out, 0, 8, stream));
    KernelScope ks(K_GROUP_INDEX, stream, 1ull << 16);
    hipLaunchKernelGGL(key_group_max_kernel, dim3(64u), dim3(BLOCK), 0, stream, d_index, reinterpret_cast<unsigned long long*>(d_out));
    KCHECK_HIP(hipGetLastError());
    return KATOME_OK;
}

// records per tile of a partition pass over records of nw words, and the digit of dev_hash_order's first pass (for a kernel that
// writes such records and counts that pass's digits per tile as it goes: table.hip, list_to_records_kernel)
size_t dev_digit_stream_bytes(uint64_t n, uint32_t nw) { return digit_stream_bytes(n, (int)nw); }
uint32_t dev_sort_tile_keys(uint32_t nw) { return nw == 1 ? SortTile<1>::KEYS : nw == 2 ? SortTile<2>::KEYS : SortTile<3>::KEYS; }
// records of nwk + 1 words (k-mer, tag) with their counts, ordered by the top 16 bits of the K-MER's hash (two stable passes)
template <int NW>
static int tagged_order_t(const u64* d_in, const u32* w_in, u64 n, u64* ka, u64* kb, u32* wa, u32* wb, const u64** k_out, const u32** w_out, hipStream_t stream,
                          u32* first_counts = nullptr) {
    PassBuffers pb;
    KCHECK(pb.init(n, NW, stream));
    pb.first = first_counts;
    const u64* kin = d_in; const u32* win = w_in;
    u64* kdst[2] = {ka, kb}; u32* wdst[2] = {wa, wb};
    for (int p = 0; p < 2; ++p) {
        HashTaggedDigit<NW> dg{(u32)(64 - 8 * (2 - p))};
        const bool have = p == 0 && first_counts != nullptr;       // (counted by whoever wrote the records: table.hip list_to_tagged_records_kernel)
        if (p == 0 && unstable_first()) {
            if (w_in) KCHECK((radix_pass<NW, true, HashTaggedDigit<NW>, false>(kin, win, n, dg, kdst[p & 1], wdst[p & 1], pb, stream, have)));
            else      KCHECK((radix_pass<NW, false, HashTaggedDigit<NW>, false>(kin, nullptr, n, dg, kdst[p & 1], nullptr, pb, stream, have)));
        } else
        if (w_in) KCHECK((radix_pass<NW, true>(kin, win, n, dg, kdst[p & 1], wdst[p & 1], pb, stream, have)));
        else      KCHECK((radix_pass<NW, false>(kin, nullptr, n, dg, kdst[p & 1], nullptr, pb, stream, have)));      // (records that count once each)
        kin = kdst[p & 1]; win = w_in ? wdst[p & 1] : nullptr;
    }
    *k_out = kin; *w_out = win;
    return KATOME_OK;
}
// one-word (k-mer, count) records ordered by the top 16 bits of the hash of their core (see CoreHashDigit)
int dev_hash_order_core(const uint64_t* d_in, const uint32_t* w_in, uint64_t n, uint32_t core_shift, uint32_t core_bases, uint64_t* ka, uint64_t* kb,
                        uint32_t* wa, uint32_t* wb, const uint64_t** k_out, const uint32_t** w_out, uint32_t* group_bits, hipStream_t stream) {
    *group_bits = CORE_GROUP_BITS;
    PassBuffers pb;
    KCHECK(pb.init(n, 1, stream));
    const u64* kin = d_in; const u32* win = w_in;
    u64* kdst[2] = {ka, kb}; u32* wdst[2] = {wa, wb};
    for (int p = 0; p < 2; ++p) {
        CoreHashDigit<1> dg{(u32)(64 - 8 * (2 - p)), core_shift, core_bases};
        KCHECK((radix_pass<1, true>(kin, win, n, dg, kdst[p & 1], wdst[p & 1], pb, stream)));
        kin = kdst[p & 1]; win = wdst[p & 1];
    }
    *k_out = kin; *w_out = win;
    return KATOME_OK;
}
int dev_hash_order_tagged(const uint64_t* d_in, const uint32_t* w_in, uint64_t n, uint32_t nwk, uint64_t* ka, uint64_t* kb, uint32_t* wa, uint32_t* wb,
                          const uint64_t** k_out, const uint32_t** w_out, uint32_t* group_bits, hipStream_t stream, uint32_t* first_counts) {
    *group_bits = 16;
    if (nwk == 1) return tagged_order_t<2>(d_in, w_in, n, ka, kb, wa, wb, k_out, w_out, stream, first_counts);
    if (nwk == 2) return tagged_order_t<3>(d_in, w_in, n, ka, kb, wa, wb, k_out, w_out, stream, first_counts);
    set_error("tagged records: k-mers of one or two words");
    return KATOME_E_UNSUPPORTED;
}
int dev_region_order(const uint64_t* d_in, const uint32_t* w_in, uint64_t n, uint32_t nw, int passes, uint64_t* ka, uint64_t* kb,
                     uint32_t* wa, uint32_t* wb, const uint64_t** k_out, const uint32_t** w_out, hipStream_t stream) {
    if (nw == 1) return region_order_t<1>(d_in, w_in, n, passes, ka, kb, wa, wb, k_out, w_out, stream);
    return region_order_t<2>(d_in, w_in, n, passes, ka, kb, wa, wb, k_out, w_out, stream);
}

// ---- unique -------------------------------------------------------------------------------------

template <int NW> __device__ __forceinline__ bool is_head(const u64* keys, u64 i) {
    return i == 0 || !key_eq(load_key<NW>(keys, i), load_key<NW>(keys, i - 1));
}

template <int NW>
__global__ __launch_bounds__(BLOCK) void uniq_count_kernel(const u64* __restrict__ keys, u64 n, u32* __restrict__ block_counts) {
    __shared__ u32 wsum[BLOCK / 64];
    const u64 base = (u64)blockIdx.x * UNIQ_TILE + (u64)threadIdx.x * UNIQ_ITEMS;
    u32 mine = 0;
#pragma unroll
    for (int j = 0; j < UNIQ_ITEMS; ++j) if (base + j < n && is_head<NW>(keys, base + j)) ++mine;
    u32 total;
    (void)block_excl_scan(mine, wsum, total);
    if (threadIdx.x == 0) block_counts[blockIdx.x] = total;
}

// exclusive scan of m u32 counts into u64 offsets, one workgroup; offs[m] = grand total
template <class T>
__global__ __launch_bounds__(1024) void scan_counts_kernel(const T* __restrict__ counts, u64 m, u64* __restrict__ offs) {
    __shared__ u64 wsum[16];
    __shared__ u64 carry_s;
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) carry_s = 0;
    __syncthreads();
    for (u64 b0 = 0; b0 < m; b0 += 1024) {
        u64 i = b0 + tid;
        u64 v = i < m ? (u64)counts[i] : 0;
        u64 incl = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { u64 t = __shfl_up(incl, o, 64); if (lane >= (u32)o) incl += t; }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        u64 woff = 0, tot = 0;
        for (int w = 0; w < 16; ++w) { if (w < (int)wave) woff += wsum[w]; tot += wsum[w]; }
        const u64 carry = carry_s;
        if (i < m) offs[i] = carry + woff + incl - v;
        __syncthreads();
        if (tid == 0) carry_s = carry + tot;
        __syncthreads();
    }
    if (tid == 0) offs[m] = carry_s;
}
// long arrays: every workgroup sums SCAN_CHUNK counts, one workgroup scans those sums, every workgroup scans its chunk
// again from its sum's offset (one workgroup walking 600 k counts alone took 2 ms, as long as a pass over 10 GB)
constexpr u32 SCAN_CHUNK = 4096;
__global__ __launch_bounds__(1024) void scan_chunk_sums_kernel(const u32* __restrict__ counts, u64 m, u64* __restrict__ sums) {
    __shared__ u64 wsum[16];
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u64 base = (u64)blockIdx.x * SCAN_CHUNK;
    u64 v = 0;
    for (u32 j = tid; j < SCAN_CHUNK; j += 1024) if (base + j < m) v += counts[base + j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if (lane == 0) wsum[wave] = v;
    __syncthreads();
    if (tid == 0) { u64 t = 0; for (int w = 0; w < 16; ++w) t += wsum[w]; sums[blockIdx.x] = t; }
}
__global__ __launch_bounds__(1024) void scan_chunks_kernel(const u32* __restrict__ counts, u64 m, const u64* __restrict__ chunk_offs,
                                                           u64* __restrict__ offs) {
    __shared__ u64 wsum[16];
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u64 base = (u64)blockIdx.x * SCAN_CHUNK + (u64)tid * (SCAN_CHUNK / 1024);       // 4 consecutive counts per thread
    u64 c[SCAN_CHUNK / 1024], mine = 0;
#pragma unroll
    for (u32 j = 0; j < SCAN_CHUNK / 1024; ++j) { c[j] = base + j < m ? (u64)counts[base + j] : 0; mine += c[j]; }
    u64 incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { u64 t = __shfl_up(incl, o, 64); if (lane >= (u32)o) incl += t; }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    u64 run = chunk_offs[blockIdx.x] + incl - mine;
    for (int w = 0; w < 16; ++w) if (w < (int)wave) run += wsum[w];
#pragma unroll
    for (u32 j = 0; j < SCAN_CHUNK / 1024; ++j) { if (base + j < m) offs[base + j] = run; run += c[j]; }
    if (blockIdx.x == gridDim.x - 1 && tid == 1023) offs[m] = chunk_offs[gridDim.x];
}

template <int NW>
__global__ __launch_bounds__(BLOCK) void uniq_write_kernel(const u64* __restrict__ keys, u64 n, const u64* __restrict__ block_offs,
                                                            u64* __restrict__ out) {
    __shared__ u32 wsum[BLOCK / 64];
    const u64 base = (u64)blockIdx.x * UNIQ_TILE + (u64)threadIdx.x * UNIQ_ITEMS;
    bool head[UNIQ_ITEMS]; u32 mine = 0;
#pragma unroll
    for (int j = 0; j < UNIQ_ITEMS; ++j) { head[j] = base + j < n && is_head<NW>(keys, base + j); mine += head[j]; }
    u32 total;
    u64 pos = block_offs[blockIdx.x] + block_excl_scan(mine, wsum, total);
#pragma unroll
    for (int j = 0; j < UNIQ_ITEMS; ++j) if (head[j]) { store_key<NW>(out, pos, load_key<NW>(keys, base + j)); ++pos; }
}

int dev_scan_counts(const uint32_t* d_counts, uint64_t m, uint64_t* d_offs, hipStream_t stream) {
    if (m <= 16 * SCAN_CHUNK) {
        hipLaunchKernelGGL(scan_counts_kernel<u32>, dim3(1), dim3(1024), 0, stream, d_counts, m, d_offs);
    } else {
        const u64 chunks = (m + SCAN_CHUNK - 1) / SCAN_CHUNK;
        DevBuf sums(stream), chunk_offs(stream);
        KCHECK(sums.alloc(chunks * 8 + 16)); KCHECK(chunk_offs.alloc((chunks + 1) * 8 + 16));
        hipLaunchKernelGGL(scan_chunk_sums_kernel, dim3((unsigned)chunks), dim3(1024), 0, stream, d_counts, m, sums.as<u64>());
        hipLaunchKernelGGL(scan_counts_kernel<u64>, dim3(1), dim3(1024), 0, stream, sums.as<u64>(), chunks, chunk_offs.as<u64>());
        hipLaunchKernelGGL(scan_chunks_kernel, dim3((unsigned)chunks), dim3(1024), 0, stream, d_counts, m, chunk_offs.as<u64>(), d_offs);
    }
    KCHECK_HIP(hipGetLastError());
    return KATOME_OK;
}

int dev_unique(uint64_t* d_keys, uint64_t n, uint32_t nw, uint64_t* n_out, hipStream_t stream) {
    *n_out = n;
    if (n < 2) return KATOME_OK;
    const u64 nblocks = (n + UNIQ_TILE - 1) / UNIQ_TILE;
    if (nblocks > 0x7fffffffull) { set_error("unique: too many keys"); return KATOME_E_ARG; }
    DevBuf counts(stream), offs(stream), tmp(stream);
    KCHECK(counts.alloc(nblocks * 4));
    KCHECK(offs.alloc((nblocks + 1) * 8));
    KCHECK(tmp.alloc(n * 8 * nw));
    if (nw == 1) hipLaunchKernelGGL(uniq_count_kernel<1>, dim3((unsigned)nblocks), dim3(BLOCK), 0, stream, d_keys, n, counts.as<u32>());
    else         hipLaunchKernelGGL(uniq_count_kernel<2>, dim3((unsigned)nblocks), dim3(BLOCK), 0, stream, d_keys, n, counts.as<u32>());
    hipLaunchKernelGGL(scan_counts_kernel, dim3(1), dim3(1024), 0, stream, counts.as<u32>(), nblocks, offs.as<u64>());
    if (nw == 1) hipLaunchKernelGGL(uniq_write_kernel<1>, dim3((unsigned)nblocks), dim3(BLOCK), 0, stream, d_keys, n, offs.as<u64>(), tmp.as<u64>());
    else         hipLaunchKernelGGL(uniq_write_kernel<2>, dim3((unsigned)nblocks), dim3(BLOCK), 0, stream, d_keys, n, offs.as<u64>(), tmp.as<u64>());
    KCHECK_HIP(hipGetLastError());
    KCHECK_HIP(hipMemcpyAsync(n_out, offs.as<u64>() + nblocks, 8, hipMemcpyDeviceToHost, stream));
    KCHECK_HIP(hipStreamSynchronize(stream));
    KCHECK_HIP(hipMemcpyAsync(d_keys, tmp.p, *n_out * 8 * nw, hipMemcpyDeviceToDevice, stream));
    return KATOME_OK;
}

// ---- rank of query keys in a sorted unique array ------------------------------------------------
// A bucket index over the top B bits (index[b] = first position whose top bits are >= b) narrows
// each lookup to a few consecutive keys; a binary search inside the bucket finishes it.

template <int NW>
__global__ __launch_bounds__(BLOCK) void bucket_index_kernel(const u64* __restrict__ sorted, u64 n, u32 key_bits, u32 B, u64* __restrict__ index) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i <= n; i += (u64)gridDim.x * BLOCK) {
        long long prev = i > 0 ? (long long)top_bits(load_key<NW>(sorted, i - 1), key_bits, B) : -1ll;
        long long cur = i < n ? (long long)top_bits(load_key<NW>(sorted, i), key_bits, B) : (1ll << B);
        for (long long b = prev + 1; b <= cur; ++b) index[b] = i;
    }
}

template <int NW>
__global__ __launch_bounds__(BLOCK) void rank_kernel(const u64* __restrict__ sorted, u64 n, u32 key_bits, u32 B,
                                                      const u64* __restrict__ index, const u64* __restrict__ q, u64 nq,
                                                      u64* __restrict__ out) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < nq; i += (u64)gridDim.x * BLOCK) {
        Key<NW> key = load_key<NW>(q, i);
        u32 b = top_bits(key, key_bits, B);
        u64 lo = index[b], hi = index[b + 1];
        while (lo < hi) {
            u64 mid = (lo + hi) >> 1;
            if (key_lt(load_key<NW>(sorted, mid), key)) lo = mid + 1; else hi = mid;
        }
        out[i] = (lo < n && key_eq(load_key<NW>(sorted, lo), key)) ? lo : ~0ull;
    }
}

int dev_bucket_index(const uint64_t* d_sorted, uint64_t n, uint32_t nw, uint32_t key_bits, uint32_t B, uint64_t* d_index, hipStream_t stream) {
    if (nw == 1) hipLaunchKernelGGL(bucket_index_kernel<1>, dim3(grid_for(n + 1, BLOCK)), dim3(BLOCK), 0, stream, d_sorted, n, key_bits, B, d_index);
    else         hipLaunchKernelGGL(bucket_index_kernel<2>, dim3(grid_for(n + 1, BLOCK)), dim3(BLOCK), 0, stream, d_sorted, n, key_bits, B, d_index);
    KCHECK_HIP(hipGetLastError());
    return KATOME_OK;
}

int dev_rank(const uint64_t* d_sorted, uint64_t n_sorted, uint32_t nw, uint32_t key_bits, const uint64_t* d_q, uint64_t nq,
             uint64_t* d_out, hipStream_t stream) {
    if (nq == 0) return KATOME_OK;
    u32 B = 1;
    while ((2ull << B) <= n_sorted / 8 && B < 27) ++B;
    if (B > key_bits) B = key_bits;
    DevBuf index(stream);
    KCHECK(index.alloc(((1ull << B) + 2) * 8));
    KCHECK(dev_bucket_index(d_sorted, n_sorted, nw, key_bits, B, index.as<u64>(), stream));
    const dim3 grid(grid_for(nq, BLOCK, 256u * 32u)), block(BLOCK);
    if (nw == 1) hipLaunchKernelGGL(rank_kernel<1>, grid, block, 0, stream, d_sorted, n_sorted, key_bits, B, index.as<u64>(), d_q, nq, d_out);
    else         hipLaunchKernelGGL(rank_kernel<2>, grid, block, 0, stream, d_sorted, n_sorted, key_bits, B, index.as<u64>(), d_q, nq, d_out);
    KCHECK_HIP(hipGetLastError());
    return KATOME_OK;
}

// ---- small permutation helpers ---------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void iota_kernel(u32* __restrict__ out, u64 n) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK) out[i] = (u32)i;
}
template <class T>
__global__ __launch_bounds__(BLOCK) void gather_kernel(const T* __restrict__ src, const u32* __restrict__ idx, u64 n, T* __restrict__ dst) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK) dst[i] = src[idx[i]];
}
template <int NW>
__global__ __launch_bounds__(BLOCK) void gather_keys_kernel(const u64* __restrict__ src, const u32* __restrict__ idx, u64 n, u64* __restrict__ dst) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK) store_key<NW>(dst, i, load_key<NW>(src, idx[i]));
}
int dev_iota(uint32_t* d, uint64_t n, hipStream_t stream) {
    if (n) hipLaunchKernelGGL(iota_kernel, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, stream, d, n);
    KCHECK_HIP(hipGetLastError());
    return KATOME_OK;
}
__global__ __launch_bounds__(BLOCK) void fill_u32_kernel(u32* __restrict__ d, u64 n, u32 v) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK) d[i] = v;
}
int dev_fill_u32(uint32_t* d, uint64_t n, uint32_t v, hipStream_t stream) {
    if (n) hipLaunchKernelGGL(fill_u32_kernel, dim3(grid_for(n, BLOCK, 256u * 8u)), dim3(BLOCK), 0, stream, d, n, v);
    KCHECK_HIP(hipGetLastError());
    return KATOME_OK;
}
// {sequence number, weight} pairs (table.hip emit, first-seen order) brought into the order of idx[] and split
__global__ __launch_bounds__(BLOCK) void gather_seq_weight_kernel(const ulonglong2* __restrict__ pairs, const u32* __restrict__ idx, u64 n,
                                                                  u64* __restrict__ seq, u32* __restrict__ weight) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK) {
        const ulonglong2 p = pairs[idx[i]];
        seq[i] = p.x; weight[i] = (u32)p.y;
    }
}
int dev_gather_seq_weight(const uint64_t* pairs, const uint32_t* idx, uint64_t n, uint64_t* seq, uint32_t* weight, hipStream_t stream) {
    if (n) hipLaunchKernelGGL(gather_seq_weight_kernel, dim3(grid_for(n, BLOCK, 256u * 32u)), dim3(BLOCK), 0, stream,
                              reinterpret_cast<const ulonglong2*>(pairs), idx, n, seq, weight);
    KCHECK_HIP(hipGetLastError());
    return KATOME_OK;
}
int dev_gather_u32(const uint32_t* src, const uint32_t* idx, uint64_t n, uint32_t* dst, hipStream_t stream) {
    if (n) hipLaunchKernelGGL(gather_kernel<u32>, dim3(grid_for(n, BLOCK, 256u * 32u)), dim3(BLOCK), 0, stream, src, idx, n, dst);
    KCHECK_HIP(hipGetLastError());
    return KATOME_OK;
}
int dev_gather_u64(const uint64_t* src, const uint32_t* idx, uint64_t n, uint64_t* dst, hipStream_t stream) {
    if (n) hipLaunchKernelGGL(gather_kernel<u64>, dim3(grid_for(n, BLOCK, 256u * 32u)), dim3(BLOCK), 0, stream, src, idx, n, dst);
    KCHECK_HIP(hipGetLastError());
    return KATOME_OK;
}
int dev_gather_keys(const uint64_t* src, const uint32_t* idx, uint64_t n, uint32_t nw, uint64_t* dst, hipStream_t stream) {
    if (n) {
        if (nw == 1) hipLaunchKernelGGL(gather_keys_kernel<1>, dim3(grid_for(n, BLOCK, 256u * 32u)), dim3(BLOCK), 0, stream, src, idx, n, dst);
        else         hipLaunchKernelGGL(gather_keys_kernel<2>, dim3(grid_for(n, BLOCK, 256u * 32u)), dim3(BLOCK), 0, stream, src, idx, n, dst);
    }
    KCHECK_HIP(hipGetLastError());
    return KATOME_OK;
}

}  // namespace katome

#ifdef KATOME_LC_PHASES
// (experiment builds only: group_merge_kernel's clocks per phase, and back to zero)
extern "C" int katome_debug_gm_phases(uint64_t* out8) {
    unsigned long long h[8];
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(katome::gm_phase_cycles), sizeof h) != hipSuccess) return -1;
    for (int i = 0; i < 8; ++i) out8[i] = h[i];
    memset(h, 0, sizeof h);
    return hipMemcpyToSymbol(HIP_SYMBOL(katome::gm_phase_cycles), h, sizeof h) == hipSuccess ? 0 : -1;
}
#endif
