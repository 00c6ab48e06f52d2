// table.hip -- open-address k-mer -> weight table in HBM (gfx950).
//
// Restates, for a whole batch at once, PtGraphBuilder::add_single_edge_fastaq (reference
// src/katome/collections/graphs/pt_graph.rs:172-198): "find the edge, else add it with weight 1,
// else weight += 1".  An edge (source (k-1)-mer, target (k-1)-mer) IS its k-mer (compress_kmer,
// compress.rs:18-28), so the table is keyed by the packed k-mer; the (k-1)-mer -> <=4 out-edges
// shape of HmGIR (collections/girs/hm_gir.rs:22) falls out of the key order at finalize.
// Weights are u32 and wrap like EdgeWeight (prelude.rs:9, pt_graph.rs:190).
//
// Random-access kernel: algorithmic traffic per insertion = 8*NW B record + 16*NW B slot
// (key compare + weight read-modify-write).  Integer/atomic work, no MFMA.
#include <atomic>
#include <cstdio>
#include <vector>

#include "common.h"
#include "lds_order.h"
#include "seq_pair.h"

namespace katome {

constexpr u64 OCC = 1ull << 63;    // slot holds a published key
constexpr u64 LOCK = 1ull << 62;   // NW=2 only: high word claimed, low word not yet visible
constexpr u64 KEYBITS = ~(OCC | LOCK);

struct Slot1 { u64 key; u32 count; u32 pad; };
struct Slot2 { u64 hi; u64 lo; u32 count; u32 pad[3]; };
struct Slot3 { u64 hi; u64 mid; u64 lo; u32 count; u32 pad; };     // tiles of 64..95 bases (k > 32 with a useful span)
static_assert(sizeof(Slot1) == 16 && sizeof(Slot2) == 32 && sizeof(Slot3) == 32, "slot layout");

__device__ __forceinline__ u64 ld_agent(const u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_agent(u64* p, u64 v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// find-or-insert `key`, add `add` to its weight; returns 1 if the key was new.
// `err` is set if the probe sequence wraps the whole table (cannot happen under the host's
// load-factor policy; bounds the loop all the same).
__device__ __forceinline__ u32 upsert(Slot1* slots, u64 cap, Key<1> key, u32 add, u32* err, u64* slot_out = nullptr) {
    const u64 want = key.w[0] | OCC;
    u64 s = hash_to_range(hash_key(key), cap);
    for (u64 probes = 0; probes < cap; ++probes) {
        u64 cur = slots[s].key;     // a stale 0 is caught by the CAS; a non-zero key never changes
        u32 fresh = 0;
        if (cur == 0) {
            cur = atomicCAS(&slots[s].key, 0ull, want);
            if (cur == 0) { cur = want; fresh = 1; }
        }
        if (cur == want) {
            atomicAdd(&slots[s].count, add);
            if (slot_out) *slot_out = s;
            return fresh;
        }
        if (++s == cap) s = 0;
    }
    *err = 1;
    return 0;
}
// (One-word keys claimed like the longer ones -- bit 62 is free -- so that their first count is a plain store too: measured,
// no gain: C3's last expansion level 89 -> 90 ms.  A single CAS publishes them; the count follows as an atomic.)

// First-seen-order mode, keys of two and three words: the thread that puts a key in also writes the key's first two sequence
// numbers, with plain stores inside the claim (nobody can reach seen[slot] before the key is published), instead of two
// atomicMin afterwards.  (One-word keys are published by a single CAS; giving them a claim window for this was measured and
// costs more than the two atomics it saves: C3's last expansion level 162 -> 174 ms.)
struct SeenInit { u64* seen; u64 a, b; bool both; };
__device__ __forceinline__ void seen_store(const SeenInit& si, u64 s) {
    st_agent(&si.seen[2 * s], si.a);
    if (si.both) st_agent(&si.seen[2 * s + 1], si.b);
}
// (Publication with C++ release/acquire atomics at agent scope instead of the waitcnt below was built and measured in round 3
// -- tools/make_publish_variant.py, KATOME_LIB=build_variants/libkatome_gpu_ra.so: on gfx950 a release store is
// `buffer_wbl2 sc1; s_waitcnt; store` and an acquire load `load sc1; s_waitcnt; buffer_inv sc1` -- an L2 write-back / invalidate
// per upsert: C3's tile insertion 41.7 -> 1029 ms, the mid-tile expansion 45 -> 1105 ms per build (profiles/r03_summary.md).
// The payload words are agent-scope (sc1, write-through) stores already; what the protocol needs between them and the
// publishing store is their completion, which is what `s_waitcnt vmcnt(0)` is.)
// 128-bit keys: there is no 128-bit CAS, so the high word is claimed with LOCK set, the low word
// is stored, drained (s_waitcnt: a hardware wait and, with its memory clobber, a compiler barrier) and then the high word is
// re-published with OCC.  Readers take the high word first and the rest after a compiler barrier (below).  A lane never
// waits while it holds a claim (claim and publication are one straight-line block), so lanes of
// one wave cannot deadlock each other; a lane that meets a LOCKed slot with ITS high word simply
// re-reads the slot on its next loop trip.
__device__ __forceinline__ u32 upsert(Slot2* slots, u64 cap, Key<2> key, u32 add, u32* err, u64* slot_out = nullptr, const SeenInit* si = nullptr) {
    u64 s = hash_to_range(hash_key(key), cap);
    u64 spins = 0;
    for (u64 probes = 0; probes < cap;) {
        // Fast path: a plain (L1/L2-cached) read.  A slot only ever moves 0 -> hi|LOCK -> hi|OCC, so a cached
        // view can lag but never lie: if it shows OCC the key is final and its low word is in the same line;
        // if it shows LOCK the slot is re-read coherently (agent scope) before anything is decided.
        u64 cur = slots[s].hi;
        bool cached_view = true;
        // (an empty view goes straight to the claim: a failed compare-and-swap hands back the word as it is now, which is
        // the coherent second look -- one memory-side round trip less per new key)
        if (cur != 0 && !(cur & OCC)) { cur = ld_agent(&slots[s].hi); cached_view = false; }
        // the other words are read AFTER the first one, in program order (loads of a wave are issued and returned in order, so
        // what they see is no older): the compiler must not hoist them above it
        asm volatile("" ::: "memory");
        if (cur == 0) {
            cur = atomicCAS(&slots[s].hi, 0ull, key.w[0] | LOCK);
            cached_view = false;
            if (cur == 0) {
                // nobody touches the slot before the key is published: its first count is a plain store, not an atomic
                st_agent(&slots[s].lo, key.w[1]);
                __hip_atomic_store(&slots[s].count, add, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (si) seen_store(*si, s);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                st_agent(&slots[s].hi, key.w[0] | OCC);
                if (slot_out) *slot_out = s;
                return 1;
            }
        }
        if ((cur & KEYBITS) == key.w[0]) {
            if (cur & LOCK) {                       // same high word, low word in flight: look again
                if (++spins > (1ull << 24)) { *err = 2; return 0; }
                __builtin_amdgcn_s_sleep(1);
                continue;
            }
            const u64 lo = cached_view ? slots[s].lo : ld_agent(&slots[s].lo);
            if (lo == key.w[1]) {
                atomicAdd(&slots[s].count, add);
                if (slot_out) *slot_out = s;
                return 0;
            }
        }
        if (++s == cap) s = 0;
        ++probes;
    }
    *err = 1;
    return 0;
}

// three-word keys: the same claim / publish protocol with two payload words
__device__ __forceinline__ u32 upsert(Slot3* slots, u64 cap, Key<3> key, u32 add, u32* err, u64* slot_out = nullptr, const SeenInit* si = nullptr) {
    u64 s = hash_to_range(hash_key(key), cap);
    u64 spins = 0;
    for (u64 probes = 0; probes < cap;) {
        u64 cur = slots[s].hi;
        bool cached_view = true;
        // (an empty view goes straight to the claim: a failed compare-and-swap hands back the word as it is now, which is
        // the coherent second look -- one memory-side round trip less per new key)
        if (cur != 0 && !(cur & OCC)) { cur = ld_agent(&slots[s].hi); cached_view = false; }
        // the other words are read AFTER the first one, in program order (loads of a wave are issued and returned in order, so
        // what they see is no older): the compiler must not hoist them above it
        asm volatile("" ::: "memory");
        if (cur == 0) {
            cur = atomicCAS(&slots[s].hi, 0ull, key.w[0] | LOCK);
            cached_view = false;
            if (cur == 0) {
                st_agent(&slots[s].mid, key.w[1]);
                st_agent(&slots[s].lo, key.w[2]);
                __hip_atomic_store(&slots[s].count, add, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (si) seen_store(*si, s);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                st_agent(&slots[s].hi, key.w[0] | OCC);
                if (slot_out) *slot_out = s;
                return 1;
            }
        }
        if ((cur & KEYBITS) == key.w[0]) {
            if (cur & LOCK) {
                if (++spins > (1ull << 24)) { *err = 2; return 0; }
                __builtin_amdgcn_s_sleep(1);
                continue;
            }
            const u64 mid = cached_view ? slots[s].mid : ld_agent(&slots[s].mid);
            const u64 lo = cached_view ? slots[s].lo : ld_agent(&slots[s].lo);
            if (mid == key.w[1] && lo == key.w[2]) {
                atomicAdd(&slots[s].count, add);
                if (slot_out) *slot_out = s;
                return 0;
            }
        }
        if (++s == cap) s = 0;
        ++probes;
    }
    *err = 1;
    return 0;
}

__device__ __forceinline__ u32 upsert_seen(Slot1* slots, u64 cap, Key<1> key, u32 add, u32* err, u64* slot_out, const SeenInit& si) {
    const u32 fresh = upsert(slots, cap, key, add, err, slot_out);
    if (fresh) {                                   // (others may already be lowering the pair: atomics)
        atomicMin((unsigned long long*)&si.seen[2 * *slot_out], (unsigned long long)si.a);
        if (si.both) atomicMin((unsigned long long*)&si.seen[2 * *slot_out + 1], (unsigned long long)si.b);
    }
    return fresh;
}
__device__ __forceinline__ u32 upsert_seen(Slot2* slots, u64 cap, Key<2> key, u32 add, u32* err, u64* slot_out, const SeenInit& si) { return upsert(slots, cap, key, add, err, slot_out, &si); }
__device__ __forceinline__ u32 upsert_seen(Slot3* slots, u64 cap, Key<3> key, u32 add, u32* err, u64* slot_out, const SeenInit& si) { return upsert(slots, cap, key, add, err, slot_out, &si); }

struct TableAux { u64 occupied; u32 err; u32 pad; };

template <int NW> struct SlotOf;
template <> struct SlotOf<1> { typedef Slot1 type; };
template <> struct SlotOf<2> { typedef Slot2 type; };
template <> struct SlotOf<3> { typedef Slot3 type; };

__device__ __forceinline__ u32 wave_sum(u32 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// First-seen-order mode.  The reference numbers edges and nodes in the order its sequential loop first meets them
// (petgraph indices: pt_graph.rs:149,194).  Per read r it adds the forward windows i = 0..W-1 and then the windows of
// the reverse complement, last window first (pt_graph.rs:282-308): window i goes in at sequence number r*2W + i and
// rc(window i) at r*2W + 2W-1-i.  A tile covering windows i0..i0+s-1 therefore puts its o-th window in at P + o with
// P = r*2W + i0, and its reverse complement puts ITS o-th window in at Q + o with Q = r*2W + 2W - i0 - s.  Beside every
// table sits seen[slot] = {earliest base of the stored orientation, earliest base of its reverse complement}
// (atomicMin); sub-windows inherit base + offset when tiles are expanded, so every k-mer ends up with the sequence
// number of its first insertion, for each strand.
struct SeenParams {
    u64* seen;            // [cap][2]
    u64 read0;            // index of the read the first record of this launch belongs to ...
    u64 rec0;             // ... and that record's index within the read-ordered stream of this batch
    u32 per_read;         // records per read (W / span)
    u32 span;             // windows per record
    u32 windows;          // W
    u32 rc;
    u32 win0;             // first window covered in every read
    const u64* win_prefix; // variable-length reads (SeenOrigin): windows before each read of the batch, [n_reads + 1]
    u64 n_reads, seq_base;
    const u64* rec_prefix; // records of this launch's kind before each read (== win_prefix for one record per window)
    u32 mode;              // 0 every window, 1 whole tiles of `span` windows, 2 the windows after the last whole tile
    // sharded build (SeenOrigin): index of every record in its source rank's batch + the segments, or explicit pairs
    const u32* idx; u32 n_seg;
    u64 seg_off[KATOME_MAX_RANKS + 1], seg_read0[KATOME_MAX_RANKS];
    const u64* pairs;
};

// seen[slot] = min(seen[slot], {a, b}).  The numbers only ever go down, so a plain look first is safe: a pair that is
// already no greater stays as it is and costs no atomic (device-scope atomics run at the memory side, ~2.5e10/s; most
// insertions of a k-mer that is seen many times are not its earliest).  The thread that has just put the key in skips
// the look -- the pair is still all-ones.
__device__ __forceinline__ void lower_seen(u64* seen, u64 slot, u64 a, u64 b, bool both, u32 was_fresh) {
    u64 cur_a = ~0ull, cur_b = ~0ull;
    if (!was_fresh) {
        const ulonglong2 cur = *reinterpret_cast<const ulonglong2*>(seen + 2 * slot);
        cur_a = cur.x; cur_b = cur.y;
    }
    if (a < cur_a) atomicMin((unsigned long long*)&seen[2 * slot], (unsigned long long)a);
    if (both && b < cur_b) atomicMin((unsigned long long*)&seen[2 * slot + 1], (unsigned long long)b);
}

template <int NW, bool SEEN>
__global__ __launch_bounds__(BLOCK) void insert_kernel(typename SlotOf<NW>::type* slots, u64 cap,
                                                        const u64* __restrict__ rec, const u32* __restrict__ wts, u64 n,
                                                        u64* occupied, u32* err, SeenParams sp) {
    u32 fresh = 0;
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK) {
        Key<NW> key;
#pragma unroll
        for (int j = 0; j < NW; ++j) key.w[j] = rec[i * NW + j];
        if (!key_valid(key)) continue;
        if (SEEN) {
            const bool flipped = (key.w[0] & RC_MARK) != 0;
            key.w[0] &= ~RC_MARK;
            const u64 g = sp.rec0 + i;
            u64 P, Q;
            if (sp.pairs) {             // both numbers came with the record (already relative to the stored orientation)
                P = sp.pairs[2 * g]; Q = sp.pairs[2 * g + 1];
            } else if (sp.idx) {        // record idx[g] of the batch its source rank cut from reads seg_read0[source]...
                u32 seg = 0;
                while (seg + 1 < sp.n_seg && g >= sp.seg_off[seg + 1]) ++seg;
                const u64 j = sp.idx[g];
                const u64 r = sp.seg_read0[seg] + j / sp.per_read, i0 = sp.win0 + (j % sp.per_read) * sp.span;
                P = r * 2 * sp.windows + i0; Q = r * 2 * sp.windows + 2 * sp.windows - i0 - sp.span;
            } else if (sp.win_prefix) {        // a read's forward windows take 2*prefix + [0, W), its reverse complement's the next W
                var_seq_pair(sp.win_prefix, sp.rec_prefix, sp.n_reads, sp.mode, sp.span, sp.seq_base, g, P, Q);
            } else {
                const u64 r = sp.read0 + g / sp.per_read, i0 = sp.win0 + (g % sp.per_read) * sp.span;
                P = r * 2 * sp.windows + i0; Q = r * 2 * sp.windows + 2 * sp.windows - i0 - sp.span;
            }
            const SeenInit si{sp.seen, flipped ? Q : P, flipped ? P : Q, sp.rc != 0};
            u64 slot = 0;
            const u32 was_fresh = upsert_seen(slots, cap, key, wts ? wts[i] : 1u, err, &slot, si);   // (a new key gets the pair inside the claim)
            fresh += was_fresh;
            if (!was_fresh) lower_seen(sp.seen, slot, si.a, si.b, si.both, 0);
        } else {
            fresh += upsert(slots, cap, key, wts ? wts[i] : 1u, err);
        }
    }
    fresh = wave_sum(fresh);
    if ((threadIdx.x & 63) == 0 && fresh) atomicAdd(occupied, (u64)fresh);
}

// move every (key, weight) of an old table into a bigger one
__device__ __forceinline__ bool slot_key(const Slot1& s, Key<1>& k) { k.w[0] = s.key & KEYBITS; return (s.key & OCC) != 0; }
__device__ __forceinline__ bool slot_key(const Slot2& s, Key<2>& k) { k.w[0] = s.hi & KEYBITS; k.w[1] = s.lo; return (s.hi & OCC) != 0; }
__device__ __forceinline__ bool slot_key(const Slot3& s, Key<3>& k) { k.w[0] = s.hi & KEYBITS; k.w[1] = s.mid; k.w[2] = s.lo; return (s.hi & OCC) != 0; }

template <int NW>
__global__ __launch_bounds__(BLOCK) void rehash_kernel(const typename SlotOf<NW>::type* __restrict__ old_slots, u64 old_cap,
                                                        typename SlotOf<NW>::type* slots, u64 cap, u64* occupied, u32* err,
                                                        const u64* __restrict__ old_seen, u64* seen) {
    u32 fresh = 0;
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < old_cap; i += (u64)gridDim.x * BLOCK) {
        typename SlotOf<NW>::type o = old_slots[i];
        Key<NW> key;
        if (!slot_key(o, key)) continue;
        u64 slot;
        fresh += upsert(slots, cap, key, o.count, err, &slot);
        if (seen) { seen[2 * slot] = old_seen[2 * i]; seen[2 * slot + 1] = old_seen[2 * i + 1]; }   // one writer per key
    }
    fresh = wave_sum(fresh);
    if ((threadIdx.x & 63) == 0 && fresh) atomicAdd(occupied, (u64)fresh);
}

// ---------------------------------------------------------------------------------------------
// Tiled counting.  Adding 1 to the weight of each of the W k-mers of a read costs W device-scope atomics,
// and the atomic rate (~2.5e10/s on MI355X, wherever the slots live) bounds the whole build.  The reads are
// therefore first counted as TILES -- the (k+span-1)-mers that cover `span` consecutive windows, W/span per
// read -- and each distinct tile then adds its count to its `span` k-mers at once.  The weights are the
// same sums (pt_graph.rs:186-191 is `+= 1` per window; addition commutes), with ~span x fewer atomics.
// ---------------------------------------------------------------------------------------------
template <int NWT, int NWK, bool RC, bool TO_TABLE>
__global__ __launch_bounds__(BLOCK) void expand_tiles_kernel(const typename SlotOf<NWT>::type* __restrict__ tiles, u64 slot0, u64 tile_cap,
                                                              u32 k, u32 span, u32 stride, typename SlotOf<NWK>::type* kmers, u64 kmer_cap,
                                                              u64* occupied, u32* err, u64* __restrict__ out_keys,
                                                              u32* __restrict__ out_w, u64* cursor,
                                                              const u64* __restrict__ tile_seen, u64* kmer_seen) {
    // The tile table is sparse (10-25 % occupied) and every tile has `span` sub-windows: the occupied tiles of
    // each run of BLOCK slots are first compacted into LDS, then the (tile, sub-window) pairs are dealt out
    // evenly over the lanes, so that every lane has an independent upsert in flight.
    __shared__ u64 lkey[BLOCK * NWT];
    __shared__ u64 lseen[BLOCK * 2];      // first-seen-order mode: the tile's two sequence bases
    __shared__ u32 lcnt[BLOCK];
    __shared__ u32 wtot[BLOCK / 64];
    __shared__ u64 bbase;
    u32 fresh = 0;
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (u64 i0 = slot0 + (u64)blockIdx.x * BLOCK; i0 < tile_cap; i0 += (u64)gridDim.x * BLOCK) {
        const u64 i = i0 + threadIdx.x;
        Key<NWT> tile; u32 n = 0; bool have = false;
        if (i < tile_cap) {
            typename SlotOf<NWT>::type s = tiles[i];
            have = slot_key(s, tile);
            n = s.count;
        }
        const u64 m = __ballot(have);
        const u32 before = __popcll(m & (lane ? (~0ull >> (64 - lane)) : 0ull));
        if (lane == 0) wtot[wave] = __popcll(m);
        __syncthreads();
        u32 woff = 0, total = 0;
#pragma unroll
        for (int w = 0; w < BLOCK / 64; ++w) { if (w < (int)wave) woff += wtot[w]; total += wtot[w]; }
        if (have) {
#pragma unroll
            for (int q = 0; q < NWT; ++q) lkey[(woff + before) * NWT + q] = tile.w[q];
            lcnt[woff + before] = n;
            if (tile_seen) { lseen[2 * (woff + before)] = tile_seen[2 * i]; lseen[2 * (woff + before) + 1] = tile_seen[2 * i + 1]; }
        }
        if (!TO_TABLE && threadIdx.x == 0 && total) bbase = atomicAdd(cursor, (u64)total * span);
        __syncthreads();
        const u32 pairs = total * span;
        for (u32 p = threadIdx.x; p < pairs; p += BLOCK) {
            const u32 t = p / span, o = p - t * span;
            Key<NWT> tk;
#pragma unroll
            for (int q = 0; q < NWT; ++q) tk.w[q] = lkey[t * NWT + q];
            Key<NWK> x = sub_window<NWT, NWK>(tk, k, span, stride, o);
            bool flipped = false;
            if (RC) x = canonical_flip(x, k, flipped);
            u64 seq_fwd = 0, seq_rev = 0;          // records with sequence numbers: read now (see below)
            if (!TO_TABLE && tile_seen) { seq_fwd = lseen[2 * t] + (u64)o * stride; seq_rev = lseen[2 * t + 1] + (u64)(span - 1 - o) * stride; }
            if (TO_TABLE) {
                if (kmer_seen) {
                    // the o-th sub-window of the tile was first put in at base + o*stride; the reverse complement of
                    // the tile holds its reverse complement as sub-window span-1-o
                    const u64 fwd = lseen[2 * t] + (u64)o * stride, rev = lseen[2 * t + 1] + (u64)(span - 1 - o) * stride;
                    const SeenInit si{kmer_seen, flipped ? rev : fwd, flipped ? fwd : rev, RC};
                    u64 slot = 0;
                    const u32 was_fresh = upsert_seen(kmers, kmer_cap, x, lcnt[t], err, &slot, si);
                    fresh += was_fresh;
                    if (!was_fresh) lower_seen(kmer_seen, slot, si.a, si.b, si.both, 0);
                } else {
                    fresh += upsert(kmers, kmer_cap, x, lcnt[t], err);
                }
            } else {
#pragma unroll
                for (int q = 0; q < NWK; ++q) out_keys[(bbase + p) * NWK + q] = x.w[q];
                out_w[bbase + p] = lcnt[t];
                if (tile_seen) {        // (kmer_seen is the records' [n][2] output here)
                    // (The pair is read from LDS above, before the key and weight stores.  Round 2 saw this kernel put wrong keys into
                    // ~0.2 % of its records when the read stood here instead; round 3 found why, and it is not the stores: with the
                    // late read the kernel needs exactly 32 VGPRs and keeps sub_window's shift amount in v31, the last register of its
                    // allocation, and on gfx950 a 64-bit shift whose amount sits there sometimes shifts by v0 -- the thread id -- instead
                    // (LLVM's Shift64HighRegBug, worked around by the compiler for gfx90a only).  Evidence, stand-alone reproducer and
                    // the build-time ISA check that keeps every kernel of the library clear of the shape: profiles/r03_shift64_erratum.md,
                    // tools/probe_shift64_top_vgpr.hip, tools/scan_shift64_top_vgpr.py, KATOME_SHIFT64_GUARD in common.h.)
                    __hip_atomic_store(&kmer_seen[2 * (bbase + p)], flipped ? seq_rev : seq_fwd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(&kmer_seen[2 * (bbase + p) + 1], flipped ? seq_fwd : seq_rev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
        __syncthreads();
    }
    if (TO_TABLE) {
        fresh = wave_sum(fresh);
        if (lane == 0 && fresh) atomicAdd(occupied, (u64)fresh);
    }
}

// ---------------------------------------------------------------------------------------------
// Table -> distinct oriented edges.  With reverse_complement the table holds canonical k-mers;
// the reference adds a read's forward windows and then the windows of its reverse complement
// (pt_graph.rs:282-308), so both orientations are edges with the same weight, and a k-mer that is
// its own reverse complement (even k only) was added twice per window.
// ---------------------------------------------------------------------------------------------
// slots per thread and tile: 8 when an edge is 12 bytes, 4 when it travels with its sequence number (LDS for the tile's edges)
template <int EMIT_ITEMS> struct EmitCap { static constexpr u32 value = BLOCK * EMIT_ITEMS * 2; };    // edges a tile of slots can yield

// A tile of BLOCK * EMIT_ITEMS slots is read in rows (coalesced), the edges it yields are numbered by a block scan, parked in
// LDS in that order and written out as one contiguous stretch behind a cursor (one atomic per tile): every store instruction
// covers consecutive addresses.  (Each thread writing its own few edges straight to HBM -- neighbouring lanes a variable number
// of records apart -- cost 1.5 x the algorithmic bytes in partial lines.)
template <int NW, bool RC, int EMIT_ITEMS>
__global__ __launch_bounds__(BLOCK) void emit_edges_kernel(const typename SlotOf<NW>::type* __restrict__ slots, u64 cap, u32 k,
                                                            u32 min_weight, u64* __restrict__ out_keys, u32* __restrict__ out_w,
                                                            u64* cursor, const u64* __restrict__ seen, u64* __restrict__ out_seq) {
    constexpr u32 EMIT_CAP = EmitCap<EMIT_ITEMS>::value;
    extern __shared__ u64 lmem[];
    u64* lk = lmem;                                       // [EMIT_CAP * NW] keys
    u64* ls = lk + EMIT_CAP * NW;                         // seen: [EMIT_CAP * 2] {sequence number, weight}; else [EMIT_CAP / 2] weights (u32)
    u32* lw = reinterpret_cast<u32*>(ls);
    __shared__ u32 wave_tot[BLOCK / 64];
    __shared__ u64 block_base;
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u64 tile = (u64)BLOCK * EMIT_ITEMS;
    for (u64 t0 = (u64)blockIdx.x * tile; t0 < cap; t0 += (u64)gridDim.x * tile) {
        Key<NW> key[EMIT_ITEMS]; u32 cnt[EMIT_ITEMS]; u32 nemit[EMIT_ITEMS]; u32 mine = 0;
#pragma unroll
        for (int j = 0; j < EMIT_ITEMS; ++j) {
            u64 i = t0 + (u64)j * BLOCK + tid;
            nemit[j] = 0; cnt[j] = 0;
            if (i < cap) {
                typename SlotOf<NW>::type s = slots[i];
                if (slot_key(s, key[j])) {
                    cnt[j] = s.count;
                    nemit[j] = 1;
                    if (RC && !key_eq(revcomp(key[j], k), key[j])) nemit[j] = 2;
                    // Clean::remove_weak_edges (pruner.rs:89-92): edges below the threshold are not emitted
                    if ((cnt[j] << ((RC && nemit[j] == 1) ? 1u : 0u)) < min_weight) nemit[j] = 0;
                }
            }
            mine += nemit[j];
        }
        // block exclusive scan of `mine`
        u32 incl = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { u32 v = __shfl_up(incl, o, 64); if (lane >= (u32)o) incl += v; }
        if (lane == 63) wave_tot[wave] = incl;
        __syncthreads();
        u32 wave_off = 0, total = 0;
#pragma unroll
        for (int w = 0; w < BLOCK / 64; ++w) { if (w < (int)wave) wave_off += wave_tot[w]; total += wave_tot[w]; }
        if (tid == 0) block_base = total ? atomicAdd(cursor, (u64)total) : 0;
        u32 pos = wave_off + (incl - mine);
#pragma unroll
        for (int j = 0; j < EMIT_ITEMS; ++j) {
            if (!nemit[j]) continue;
            Key<NW> rc = RC ? revcomp(key[j], k) : key[j];
            const u32 w = cnt[j] << ((RC && nemit[j] == 1) ? 1u : 0u);      // self-complementary k-mer (as a shift: see lds_count_kernel)
            u64 s0 = 0, s1 = 0;
            if (seen) {
                const u64 slot = t0 + (u64)j * BLOCK + tid;
                s0 = seen[2 * slot]; s1 = seen[2 * slot + 1];
                if (RC && nemit[j] == 1) s0 = s0 < s1 ? s0 : s1;      // both strands are the same edge
            }
#pragma unroll
            for (int q = 0; q < NW; ++q) lk[pos * NW + q] = key[j].w[q];
            if (seen) { ls[2 * pos] = s0; ls[2 * pos + 1] = w; }      // first-seen order: {sequence number, weight} side by side
            else lw[pos] = w;
            ++pos;
            if (nemit[j] == 2) {
#pragma unroll
                for (int q = 0; q < NW; ++q) lk[pos * NW + q] = rc.w[q];
                if (seen) { ls[2 * pos] = s1; ls[2 * pos + 1] = w; }
                else lw[pos] = w;
                ++pos;
            }
        }
        __syncthreads();
        if (total) {
            const u64 base = block_base;
            for (u32 i = tid; i < total * NW; i += BLOCK) out_keys[base * NW + i] = lk[i];
            if (seen) { for (u32 i = tid; i < total * 2; i += BLOCK) out_seq[base * 2 + i] = ls[i]; }
            else { for (u32 i = tid; i < total; i += BLOCK) out_w[base + i] = lw[i]; }
        }
        __syncthreads();
    }
}

// every key of a table with its count [and its two sequence numbers], compacted behind a cursor (one atomic per tile of slots;
// the tile's records go through LDS so that they leave as one contiguous stretch, like emit_edges_kernel's)
template <int NW>
__global__ __launch_bounds__(BLOCK) void table_records_kernel(const typename SlotOf<NW>::type* __restrict__ slots, u64 cap, u64* __restrict__ out_keys,
                                                               u32* __restrict__ out_w, u64* cursor, const u64* __restrict__ seen, u64* __restrict__ out_seen) {
    constexpr int ITEMS = 4;
    constexpr u32 CAP = BLOCK * ITEMS;
    extern __shared__ u64 lmem[];
    u64* lk = lmem;                                       // [CAP * NW]
    u64* lp = lk + CAP * NW;                              // [CAP * 2] the pairs (first-seen order only)
    u32* lw = reinterpret_cast<u32*>(lp + (seen ? CAP * 2 : 0));       // [CAP]
    __shared__ u32 wave_tot[BLOCK / 64];
    __shared__ u64 block_base;
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u64 tile = (u64)CAP;
    for (u64 t0 = (u64)blockIdx.x * tile; t0 < cap; t0 += (u64)gridDim.x * tile) {
        Key<NW> key[ITEMS]; u32 cnt[ITEMS]; bool have[ITEMS]; u32 mine = 0;
#pragma unroll
        for (int j = 0; j < ITEMS; ++j) {
            const u64 i = t0 + (u64)j * BLOCK + tid;
            have[j] = false; cnt[j] = 0;
            if (i < cap) {
                typename SlotOf<NW>::type s = slots[i];
                have[j] = slot_key(s, key[j]);
                cnt[j] = s.count;
            }
            mine += have[j];
        }
        u32 incl = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { u32 v = __shfl_up(incl, o, 64); if (lane >= (u32)o) incl += v; }
        if (lane == 63) wave_tot[wave] = incl;
        __syncthreads();
        u32 wave_off = 0, total = 0;
#pragma unroll
        for (int w = 0; w < BLOCK / 64; ++w) { if (w < (int)wave) wave_off += wave_tot[w]; total += wave_tot[w]; }
        if (tid == 0) block_base = total ? atomicAdd(cursor, (u64)total) : 0;
        u32 pos = wave_off + (incl - mine);
#pragma unroll
        for (int j = 0; j < ITEMS; ++j) {
            if (!have[j]) continue;
#pragma unroll
            for (int q = 0; q < NW; ++q) lk[pos * NW + q] = key[j].w[q];
            lw[pos] = cnt[j];
            if (seen) { const u64 slot = t0 + (u64)j * BLOCK + tid; lp[2 * pos] = seen[2 * slot]; lp[2 * pos + 1] = seen[2 * slot + 1]; }
            ++pos;
        }
        __syncthreads();
        if (total) {
            const u64 base = block_base;
            for (u32 i = tid; i < total * NW; i += BLOCK) out_keys[base * NW + i] = lk[i];
            for (u32 i = tid; i < total; i += BLOCK) out_w[base + i] = lw[i];
            if (seen) { for (u32 i = tid; i < total * 2; i += BLOCK) out_seen[base * 2 + i] = lp[i]; }
        }
        __syncthreads();
    }
}

// Distinct tiles -> (sub-window, count) records, for the sorted counting below: a workgroup takes 2048 slots per trip (rows of
// 256: coalesced), parks the occupied tiles in LDS, takes its stretch of the output with one cursor atomic and deals the
// (tile, sub-window) pairs out over the lanes -- consecutive lanes write consecutive records.  (expand_tiles_kernel does the
// same 256 slots at a time: two barriers and an atomic per ~600 records, which is fine beside table upserts and 3x too slow
// for a streaming pass.)
constexpr u32 TR_ITEMS = 8;
template <int NWT, int NWK, bool RC>
__global__ __launch_bounds__(BLOCK) void tiles_to_records_kernel(const typename SlotOf<NWT>::type* __restrict__ tiles, u64 tile_cap, u32 k, u32 span,
                                                                  u32 stride, u64* __restrict__ out_keys, u32* __restrict__ out_w, u64* cursor) {
    __shared__ u64 lkey[BLOCK * TR_ITEMS * NWT];
    __shared__ u32 lcnt[BLOCK * TR_ITEMS];
    __shared__ u32 wtot[BLOCK / 64];
    __shared__ u64 bbase;
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u64 trip = (u64)BLOCK * TR_ITEMS;
    for (u64 t0 = (u64)blockIdx.x * trip; t0 < tile_cap; t0 += (u64)gridDim.x * trip) {
        Key<NWT> tk[TR_ITEMS]; u32 tc[TR_ITEMS]; bool have[TR_ITEMS]; u32 mine = 0;
#pragma unroll
        for (u32 j = 0; j < TR_ITEMS; ++j) {
            const u64 i = t0 + (u64)j * BLOCK + tid;
            have[j] = false; tc[j] = 0;
            if (i < tile_cap) {
                typename SlotOf<NWT>::type s = tiles[i];
                have[j] = slot_key(s, tk[j]);
                tc[j] = s.count;
            }
            mine += have[j];
        }
        u32 incl = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { u32 v = __shfl_up(incl, o, 64); if (lane >= (u32)o) incl += v; }
        if (lane == 63) wtot[wave] = incl;
        __syncthreads();
        u32 woff = 0, total = 0;
#pragma unroll
        for (u32 w = 0; w < BLOCK / 64; ++w) { if (w < wave) woff += wtot[w]; total += wtot[w]; }
        u32 at = woff + (incl - mine);
#pragma unroll
        for (u32 j = 0; j < TR_ITEMS; ++j) {
            if (!have[j]) continue;
#pragma unroll
            for (int q = 0; q < NWT; ++q) lkey[at * NWT + q] = tk[j].w[q];
            lcnt[at] = tc[j];
            ++at;
        }
        if (tid == 0 && total) bbase = atomicAdd((unsigned long long*)cursor, (unsigned long long)total * span);
        __syncthreads();
        const u32 pairs = total * span;
        const u64 base = bbase;
        for (u32 p = tid; p < pairs; p += BLOCK) {
            const u32 t = p / span, o = p - t * span;
            Key<NWT> tile;
#pragma unroll
            for (int q = 0; q < NWT; ++q) tile.w[q] = lkey[t * NWT + q];
            Key<NWK> x = sub_window<NWT, NWK>(tile, k, span, stride, o);
            if (RC) x = canonical(x, k);
#pragma unroll
            for (int q = 0; q < NWK; ++q) out_keys[(base + p) * NWK + q] = x.w[q];
            out_w[base + p] = lcnt[t];
        }
        __syncthreads();
    }
}

// a compact list of distinct tiles with their counts (what the sorted counting of a level leaves) -> the (sub-window, count) records
// of the next level: record p is sub-window p % span of tile p / span; consecutive lanes write consecutive records
// (REP: one-word k-mers of the ordered count, lds_count_ordered_kernel -- the representative orientation instead of the canonical one)
template <int NWK, bool RC, bool REP> __device__ __forceinline__ Key<NWK> level_orientation(const Key<NWK>& x, u32 k) {
    if constexpr (REP) { static_assert(NWK == 1, "one-word k-mers"); return RC ? rep_orientation(x, k) : x; }
    else return RC ? canonical(x, k) : x;
}
template <int NWT, int NWK, bool RC, bool REP = false>
__global__ __launch_bounds__(BLOCK) void list_to_records_kernel(const u64* __restrict__ tiles, const u32* __restrict__ counts, u64 n_tiles, u32 k, u32 span,
                                                                 u32 stride, u64* __restrict__ out_keys, u32* __restrict__ out_w) {
    const u64 n = n_tiles * span;
    for (u64 p = (u64)blockIdx.x * BLOCK + threadIdx.x; p < n; p += (u64)gridDim.x * BLOCK) {
        const u64 t = p / span;
        const u32 o = (u32)(p - t * span);
        Key<NWT> tile;
#pragma unroll
        for (int q = 0; q < NWT; ++q) tile.w[q] = tiles[t * NWT + q];
        const Key<NWK> x = level_orientation<NWK, RC, REP>(sub_window<NWT, NWK>(tile, k, span, stride, o), k);
#pragma unroll
        for (int q = 0; q < NWK; ++q) out_keys[p * NWK + q] = x.w[q];
        out_w[p] = counts[t];
    }
}

// The same records written tile by tile of the partition pass that follows -- `tile_keys` consecutive records per trip of a workgroup
// -- with that pass's digit (bits 48..55 of the record's hash: dev_hash_order's first pass) counted per tile in LDS as they are made:
// counts[tile][digit] is what radix_hist_kernel would count, without reading the records back (C3: 17 + 15 GB not read per build).
// (REP: the ordered count's records and the first digit of dev_key_order, bits 2k - 16 .. 2k - 9 of the key)
template <int NWT, int NWK, bool RC, bool REP = false>
__global__ __launch_bounds__(BLOCK) void list_to_records_hist_kernel(const u64* __restrict__ tiles, const u32* __restrict__ counts, u64 n_tiles, u32 k, u32 span,
                                                                      u32 stride, u64* __restrict__ out_keys, u32* __restrict__ out_w, u32 tile_keys,
                                                                      u32* __restrict__ digit_counts) {
    static_assert(BLOCK == 256, "one thread per digit");
    __shared__ u32 h[256];
    const u64 n = n_tiles * span, n_out_tiles = (n + tile_keys - 1) / tile_keys;
    for (u64 ot = blockIdx.x; ot < n_out_tiles; ot += gridDim.x) {
        h[threadIdx.x] = 0;
        __syncthreads();
        const u64 p0 = ot * tile_keys, p1 = p0 + tile_keys < n ? p0 + tile_keys : n;
        for (u64 p = p0 + threadIdx.x; p < p1; p += BLOCK) {
            const u64 t = p / span;
            const u32 o = (u32)(p - t * span);
            Key<NWT> tile;
#pragma unroll
            for (int q = 0; q < NWT; ++q) tile.w[q] = tiles[t * NWT + q];
            const Key<NWK> x = level_orientation<NWK, RC, REP>(sub_window<NWT, NWK>(tile, k, span, stride, o), k);
#pragma unroll
            for (int q = 0; q < NWK; ++q) out_keys[p * NWK + q] = x.w[q];
            out_w[p] = counts[t];
            atomicAdd(&h[(REP ? (u32)(x.w[0] >> (2 * k - 16)) : (u32)(hash_key(x) >> 48)) & 255u], 1u);
        }
        __syncthreads();
        digit_counts[ot * 256 + threadIdx.x] = h[threadIdx.x];
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------
// The last level without device-scope atomics.  The (k-mer, count) records of the distinct tiles are ordered by the top 16
// bits of their hash (two stable 8-bit passes of radix.hip, HashDigit), which cuts them into 65536 groups; a workgroup takes a
// group and counts it in an LDS table -- compare-and-swap and add in LDS --, in R sub-rounds by the next hash bits so that a
// sub-round's keys fit the table even if every record were a new key (nothing can overflow), re-reading the group from
// L2 / Infinity Cache; a sub-round's keys leave as oriented edges straight away (both strands, the remove_weak_edges
// threshold), as one contiguous stretch behind a cursor.
// ---------------------------------------------------------------------------------------------
constexpr u32 LC_THREADS = 1024;
// (-DKATOME_LC_PHASES: an experiment build that adds up, per phase of the two counting kernels, the shader clocks thread 0 of every
// workgroup sees go by -- tools/lc_phases.py reads them through katome_debug_lc_phases; never defined in the shipped library)
#ifdef KATOME_LC_PHASES
__device__ unsigned long long lc_phase_cycles[16];
#define LC_PHASE_BEGIN() unsigned long long lc_t0 = clock64()
#define LC_PHASE(i) do { if (threadIdx.x == 0) { const unsigned long long lc_t = clock64(); atomicAdd(&lc_phase_cycles[i], lc_t - lc_t0); lc_t0 = lc_t; } } while (0)
#else
#define LC_PHASE_BEGIN() do {} while (0)
#define LC_PHASE(i) do {} while (0)
#endif
#ifndef KATOME_LC_LU
#define KATOME_LC_LU 4          // records in flight per thread in the counting loops
#endif
// LDS table: 8 B key + 4 B count per slot, LC_THREADS x PER slots (every thread reads PER slots out).  PER = 13: 13312 slots =
// 156 KiB of the CU's 160 (one workgroup of 1024 per CU either way): groups of 22 k records (2^16 groups at C3) go through in 3
// sub-rounds instead of the 4 a table of 8192 needs.  PER = 8: groups of 5.5 k records (2^18 groups: the look-back passes of
// radix.hip) fit an 8192-slot table in ONE round -- no re-read of the group, and less to clear and to read out per group.
// Any number of sub-rounds: a record's sub-round and its slot are two mulhi's of separate hash bits.
template <int PER> struct LcTable {
    static constexpr u32 SLOTS = LC_THREADS * PER;
    static constexpr u32 FILL = (u32)(SLOTS / 4096.0 * 2900);   // records a sub-round may hold at most on average (all new: load 0.71)
};
constexpr u32 LC_MAX_ROUNDS = 32;
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
// the optimistic attempt's patience with a full table (KATOME_LC_PROBE_LIMIT: tests make the first attempt fail with it)
static u32 lc_probe_limit() {
    static const u32 v = getenv("KATOME_LC_PROBE_LIMIT") ? (u32)std::max(1, atoi(getenv("KATOME_LC_PROBE_LIMIT"))) : 128u;
    return v;
}
static void lc_trace(const char* what, u32 tried, u32 guaranteed) {
    if (getenv("KATOME_LC_TRACE")) fprintf(stderr, "[lds count] %s: the attempt with %u sub-rounds filled a table; counting again with %u\n", what, tried, guaranteed);
}
// share of a group's records assumed distinct when the sub-rounds of the first attempt are chosen (KATOME_LC_OPTIMISM; 1 = never
// try with fewer than the guaranteed number)
static double lc_optimism() {
    static const double v = getenv("KATOME_LC_OPTIMISM") ? std::min(1.0, std::max(0.05, atof(getenv("KATOME_LC_OPTIMISM")))) : 0.75;
    return v;
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
constexpr u32 LP_PER = 19;
constexpr u32 LP_SLOTS = LC_THREADS * LP_PER;                    // 19456 x 8 B = 152 KiB
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
// hash).  At read-out the group's kept keys are put in key order in the table's own LDS -- a counting sort on the remainder's top 11
// bits into 2048 buckets, then every key is placed by counting the keys of its bucket (about 6 at C3) below it -- and leave as two lists:
//   S1, the representatives, ascending, from the group's first record on (s1_key + index[g]: fixed before the count, so the groups
//       stay in key order; a group has no more distinct keys than records), their number in group_count[g];
//   S2 (both strands), their reverse complements, behind a cursor in no order.
// group_merge_kernel (radix.hip) orders S2 group by group and merges it with S1 (half_merge_kernel when S2 is sorted in full).
// err 5 / err 3 as in lds_count_packed_kernel: the caller then counts the usual way.
constexpr u32 LO_BUCKETS = LDS_ORDER_BUCKETS;
static_assert(LC_THREADS == LDS_ORDER_THREADS, "the read-out orders with lds_order.h");
template <bool RC>
__global__ __launch_bounds__(LC_THREADS) void lds_count_ordered_kernel(const u64* keys, const u32* wts, const u64* __restrict__ index, u32 k,
                                                                        u32 min_weight, u64* s1_key, u32* s1_w, u32* group_count, u64* s2_key,
                                                                        u32* s2_w, uint8_t* s2_digit, u64 s2_cap, unsigned long long* cursor,
                                                                        unsigned long long* distinct, u32* err, u32 probe_limit) {
    extern __shared__ unsigned long long lc_mem[];
    unsigned long long* slot = lc_mem;                                   // [LP_SLOTS]: remainder << 16 | count; then the kept ones in key order
    u32* bucket = reinterpret_cast<u32*>(lc_mem + LP_SLOTS);             // [LO_BUCKETS / 2]: counters of buckets 2i (low half), 2i + 1
    __shared__ u32 wtot[LC_THREADS / 64];
    __shared__ unsigned long long base_sh;
    const u32 tid = threadIdx.x, lane = tid & 63;
    const u32 rem_bits = 2 * k - 16, bshift = rem_bits > 11 ? rem_bits - 11 : 0;            // (bucket: the remainder's top 11 bits)
    const u64 REM = (1ull << rem_bits) - 1;
    u32 my_distinct = 0;
    LC_PHASE_BEGIN();
    for (u32 g = blockIdx.x; g < (1u << 16); g += gridDim.x) {
        const u64 lo = index[g], hi = index[g + 1];
        if (lo == hi) continue;
        for (u32 i = tid; i < LP_SLOTS; i += LC_THREADS) slot[i] = 0ull;
        bucket[tid] = 0u;
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
        unsigned long long v[LP_PER]; u32 keep = 0;
#pragma unroll
        for (u32 j = 0; j < LP_PER; ++j) {
            v[j] = slot[tid * LP_PER + j];
            if (v[j]) { ++my_distinct; if (((u32)v[j] & 0xFFFFu) >= min_weight) keep |= 1u << j; }      // Clean::remove_weak_edges
        }
        // the kept ones into key order in the table's LDS (lds_order.h); the group's S2 room is reserved once their number is known
        const u32 total = lds_order_entries<LP_PER>(v, keep, slot, bucket, wtot, bshift, [&](u32 t) {
            if (tid == 0) { group_count[g] = t; base_sh = t ? atomicAdd(cursor, (unsigned long long)t) : 0ull; }
        });
        LC_PHASE(14);
        for (u32 i = tid; i < total; i += LC_THREADS) {
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
template <int LF_PER> struct LfTable {
    static constexpr u32 SLOTS = LC_THREADS * LF_PER;
    static constexpr u32 FILL = SLOTS / 20 * 11;                  // distinct keys a group may hold (load 0.55)
};
constexpr u64 LF_SALT = 0x9E3779B97F4A7C15ull;
template <bool RC, bool EVEN_K, int LF_PER>
__global__ __launch_bounds__(LC_THREADS) void lds_count_full_kernel(const u64* keys, const u32* wts, const u64* __restrict__ index, u32 groups_run, u32 k,
                                                                     u32 min_weight, u64* out_keys, u32* out_w, u64 out_cap, unsigned long long* cursor,
                                                                     unsigned long long* distinct, u32* err, u32 probe_limit) {
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
template <int PER> struct Lf3Table {
    static constexpr u32 SLOTS = LC_THREADS * PER;                // PER = 5: 5120 x 28 B = 140 KiB; 3: 3072 x 28 B = 84 KiB
    static constexpr u32 FILL = SLOTS / 20 * 11;
};
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

// ---- first-seen builds: the last level counted by sorting ------------------------------------------------------------------------
// A k-mer record of such a build has two sequence numbers: the first insertion of the stored (canonical) k-mer and the first
// insertion of its reverse complement (pt_graph.rs:282-308 adds a read's forward windows, then those of its reverse complement).
// Both fall into the range of ONE read -- the first read that holds the k-mer on either strand --, so with reads of a fixed length
// (S sequence numbers each) the pair packs into one word: read << 32 | offset of the one << 16 | offset of the other.  The records
// (k-mer, packed pair) + count go through the same two hash passes as the headline build's (the k-mer's words are hashed, the
// tag rides along) and are counted in LDS, where the two numbers are lowered by 64-bit atomicMin's of read << 16 | offset.
constexpr unsigned long long SEEN_NONE = ~0ull;
__device__ __forceinline__ unsigned long long seen_pack(u64 read, u32 a, u32 b) { return read << 32 | (unsigned long long)a << 16 | b; }

// The windows left over after a batch's tiles, kept aside for the sorted last level: the valid ones (a skipped read's records are
// all-ones) are appended behind a device cursor, one atomic per workgroup and trip.  TAGGED (first-seen order): plain k-mer records
// that carry RC_MARK when the stored orientation is the reverse complement's become tagged records -- record i is window
// win0 + i % per_read of read read0 + i / per_read.
constexpr int KR_ITEMS = 8;            // records per thread and trip: one atomic on the cursor per 2048 records (one per 256 made a batch of
                                       // 5e7 records wait 3 ms for its 2e5 turns at that one address)
template <int NW, bool TAGGED>
__global__ __launch_bounds__(BLOCK) void keep_rest_kernel(const u64* __restrict__ rec, u64 n, u64 read0, u32 per_read, u32 win0, u32 seq_per_read,
                                                           u64* __restrict__ out, unsigned long long* cursor, u32 win_stride, u32 span) {
    constexpr int WORDS = NW + (TAGGED ? 1 : 0);
    constexpr u32 TILE = BLOCK * KR_ITEMS;
    __shared__ u32 wtot[KR_ITEMS][BLOCK / 64];       // valid records of row j in wave w; then their offset inside the workgroup's claim
    __shared__ unsigned long long base_sh;
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u64 lt_mask = lane ? (~0ull >> (64 - lane)) : 0ull;
    for (u64 t0 = (u64)blockIdx.x * TILE; t0 < n; t0 += (u64)gridDim.x * TILE) {
        Key<NW> key[KR_ITEMS];
        u32 before[KR_ITEMS];
#pragma unroll
        for (int j = 0; j < KR_ITEMS; ++j) {
            const u64 i = t0 + (u64)j * BLOCK + tid;
            key[j] = key_invalid<NW>();
            if (i < n) {
#pragma unroll
                for (int q = 0; q < NW; ++q) key[j].w[q] = rec[i * NW + q];
            }
            const u64 m = __ballot(key_valid(key[j]));
            before[j] = __popcll(m & lt_mask);
            if (lane == 0) wtot[j][wave] = __popcll(m);
        }
        __syncthreads();
        if (tid == 0) {
            u32 run = 0;
#pragma unroll
            for (int j = 0; j < KR_ITEMS; ++j)
#pragma unroll
                for (u32 w = 0; w < BLOCK / 64; ++w) { const u32 c = wtot[j][w]; wtot[j][w] = run; run += c; }
            base_sh = run ? atomicAdd(cursor, (unsigned long long)run) : 0ull;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < KR_ITEMS; ++j) {
            if (!key_valid(key[j])) continue;
            const u64 i = t0 + (u64)j * BLOCK + tid;
            const u64 at = (base_sh + wtot[j][wave] + before[j]) * WORDS;
            const bool flipped = TAGGED && (key[j].w[0] & RC_MARK) != 0;
            if (TAGGED) key[j].w[0] &= ~RC_MARK;
#pragma unroll
            for (int q = 0; q < NW; ++q) out[at + q] = key[j].w[q];
            if (TAGGED) {
                const u64 read = read0 + i / per_read;
                // (insert_kernel's P and Q within the read.  A tile of `span` windows, win_stride apart from the next: its first window goes
                // in at w; its reverse complement is the read's reverse complement's window W - span - w, number 2W - span - w)
                const u32 w = win0 + (u32)(i % per_read) * win_stride, fwd = w, rev = seq_per_read - span - w;
                out[at + NW] = seen_pack(read, flipped ? rev : fwd, flipped ? fwd : rev);
            }
        }
        __syncthreads();
    }
}
// ... and back into (key, {first insertion of the stored orientation, of its reverse complement}) for the k-mer table
template <int NW>
__global__ __launch_bounds__(BLOCK) void tagged_to_pairs_kernel(const u64* __restrict__ tagged, u64 n, u64 seq_per_read, u64* __restrict__ keys,
                                                                 u64* __restrict__ pairs) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK) {
#pragma unroll
        for (int q = 0; q < NW; ++q) keys[i * NW + q] = tagged[i * (NW + 1) + q];
        const u64 tag = tagged[i * (NW + 1) + NW], base = (tag >> 32) * seq_per_read;
        pairs[2 * i] = base + ((tag >> 16) & 0xFFFFull); pairs[2 * i + 1] = base + (tag & 0xFFFFull);
    }
}

// every distinct tile of the last level -> its `span` k-mers as records of NWK + 1 words + the tile's count (tiles_to_records_kernel's
// shape: 2048 slots per trip).  read = fwd / seq_per_read as a multiplication by `magic` = floor(2^64 / seq_per_read) + 1: exact for
// numbers below 2^64 / seq_per_read, which 2^32 reads of < 2^16 numbers each stay under.
template <int NWT, int NWK, bool RC>
__global__ __launch_bounds__(BLOCK) void seen_records_kernel(const typename SlotOf<NWT>::type* __restrict__ tiles, const u64* __restrict__ tile_seen, u64 tile_cap,
                                                              u32 k, u32 span, u64 seq_per_read, u64 magic, u64* __restrict__ out, u32* __restrict__ out_w,
                                                              u64* cursor, u32* err) {
    extern __shared__ u64 sr_mem[];
    u64* lkey = sr_mem;                                               // [BLOCK * TR_ITEMS * NWT]
    u64* lread = lkey + BLOCK * TR_ITEMS * NWT;                       // [BLOCK * TR_ITEMS]
    u32* loff = reinterpret_cast<u32*>(lread + BLOCK * TR_ITEMS);     // [BLOCK * TR_ITEMS * 2]
    u32* lcnt = loff + BLOCK * TR_ITEMS * 2;                          // [BLOCK * TR_ITEMS]
    __shared__ u32 wtot[BLOCK / 64];
    __shared__ u64 bbase;
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u64 trip = (u64)BLOCK * TR_ITEMS;
    for (u64 t0 = (u64)blockIdx.x * trip; t0 < tile_cap; t0 += (u64)gridDim.x * trip) {
        Key<NWT> tk[TR_ITEMS]; u32 tc[TR_ITEMS]; u64 fwd[TR_ITEMS], rev[TR_ITEMS]; bool have[TR_ITEMS]; u32 mine = 0;
#pragma unroll
        for (u32 j = 0; j < TR_ITEMS; ++j) {
            const u64 i = t0 + (u64)j * BLOCK + tid;
            have[j] = false; tc[j] = 0; fwd[j] = rev[j] = 0;
            if (i < tile_cap) {
                typename SlotOf<NWT>::type sl = tiles[i];
                have[j] = slot_key(sl, tk[j]);
                tc[j] = sl.count;
                if (have[j]) { fwd[j] = tile_seen[2 * i]; if (RC) rev[j] = tile_seen[2 * i + 1]; }
            }
            mine += have[j];
        }
        u32 incl = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { u32 v = __shfl_up(incl, o, 64); if (lane >= (u32)o) incl += v; }
        if (lane == 63) wtot[wave] = incl;
        __syncthreads();
        u32 woff = 0, total = 0;
#pragma unroll
        for (u32 w = 0; w < BLOCK / 64; ++w) { if (w < wave) woff += wtot[w]; total += wtot[w]; }
        u32 at = woff + (incl - mine);
#pragma unroll
        for (u32 j = 0; j < TR_ITEMS; ++j) {
            if (!have[j]) continue;
#pragma unroll
            for (int q = 0; q < NWT; ++q) lkey[at * NWT + q] = tk[j].w[q];
            lcnt[at] = tc[j];
            const u64 read = __umul64hi(fwd[j], magic);
            const u64 a = fwd[j] - read * seq_per_read, b = RC ? rev[j] - read * seq_per_read : 0;        // (no reverse complements: one number)
            if (read >> 32 || a >= seq_per_read || a + span > 0xFFFFu || (RC && (rev[j] < read * seq_per_read || b > 0xFFFFu))) *err = 5;   // (does not pack)
            lread[at] = read; loff[2 * at] = (u32)a; loff[2 * at + 1] = (u32)b;
            ++at;
        }
        if (tid == 0 && total) bbase = atomicAdd((unsigned long long*)cursor, (unsigned long long)total * span);
        __syncthreads();
        const u32 pairs = total * span;
        const u64 base = bbase;
        for (u32 p = tid; p < pairs; p += BLOCK) {
            const u32 t = p / span, o = p - t * span;
            Key<NWT> tile;
#pragma unroll
            for (int q = 0; q < NWT; ++q) tile.w[q] = lkey[t * NWT + q];
            Key<NWK> x = sub_window<NWT, NWK>(tile, k, span, 1, o);
            bool flipped = false;
            if (RC) x = canonical_flip(x, k, flipped);
            // window o of the tile went in at fwd + o; the tile's reverse complement holds its reverse complement as window span-1-o
            const u32 a = loff[2 * t] + o, b = loff[2 * t + 1] + (span - 1 - o);
            const u64 rec = (base + p) * (NWK + 1);
#pragma unroll
            for (int q = 0; q < NWK; ++q) out[rec + q] = x.w[q];
            out[rec + NWK] = seen_pack(lread[t], flipped ? b : a, flipped ? a : b);
            out_w[base + p] = lcnt[t];
        }
        __syncthreads();
    }
}

// counts the records of each hash group in an LDS table and lowers the two sequence numbers; writes every distinct k-mer as one or
// two edges {key} + {sequence number, weight}.  The slot's first word is the k-mer itself when it has one word (lds_count_kernel's
// slot) and fingerprint | representative record when it has two (lds_count_wide_kernel's: the full keys are compared in the group).
constexpr int LCS_PER = 5;                                        // 5120 slots of 28 bytes = 140 KiB
// LIST: a TILE level of such a build -- every distinct key leaves once, as key + tag (the two lowered numbers
// packed again: both come from the first read that holds the tile on either strand) in out_keys [n][NWK + 1] and its count in
// out_pairs read as u32 [n]; RC then only says whether the second number is tracked.
template <bool RC, int NWK, bool LIST = false>
__global__ __launch_bounds__(LC_THREADS) void lds_count_seen_kernel(const u64* recs, const u32* wts, const u64* __restrict__ index, u32 gbits, u32 R, u32 k,
                                                                     u64 seq_per_read, u64* out_keys, u64* out_pairs, u64 out_cap,
                                                                     unsigned long long* cursor, unsigned long long* distinct, u32* err, u32 probe_limit) {
    constexpr u32 SLOTS = LC_THREADS * LCS_PER;
    constexpr int STRIDE = NWK + 1;
    constexpr unsigned long long REP_MASK = (1ull << 20) - 1;
    extern __shared__ unsigned long long lcs_mem[];
    unsigned long long* lkey = lcs_mem;                                  // [SLOTS]: OCC | key, or OCC | fingerprint << 20 | representative
    unsigned long long* lA = lcs_mem + SLOTS;                            // [SLOTS]: read << 16 | offset, stored orientation
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
                        atomicMin(&lA[s], (tag >> 32) << 16 | ((tag >> 16) & 0xFFFFull));
                        if (RC) atomicMin(&lB[s], (tag >> 32) << 16 | (tag & 0xFFFFull));
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
                        const u64 seq_a = (a >> 16) * seq_per_read + (a & 0xFFFFull), seq_b = (b >> 16) * seq_per_read + (b & 0xFFFFull);
                        const u32 c = sc[j];
                        if (LIST) {
                            if (p < SC) {
#pragma unroll
                                for (int q = 0; q < NWK; ++q) skey[(size_t)p * KW + q] = kk[j].w[q];
                                if (RC && (a >> 16) != (b >> 16)) *err = 6;              // (the two numbers of a tile from two reads: cannot be)
                                skey[(size_t)p * KW + NWK] = seen_pack(a >> 16, (u32)(a & 0xFFFFull), RC ? (u32)(b & 0xFFFFull) : 0u);
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

// a list of distinct tiles with their tags and counts (lds_count_seen_kernel, LIST) -> the tagged records of the next level: record p is
// sub-window p % n_sub of tile p / n_sub; its numbers are the tile's plus the sub-window's place in it (expand_tiles_kernel's rule)
// (digit_counts: written tile by tile of the partition pass that follows -- tile_keys records per trip --, that pass's digit counted per
// tile on the way, as list_to_records_hist_kernel does; without: a plain grid-stride walk)
template <int NWT, int NWK, bool RC>
__global__ __launch_bounds__(BLOCK) void list_to_tagged_records_kernel(const u64* __restrict__ list, const u32* __restrict__ counts, u64 n_tiles, u32 sub_len,
                                                                        u32 n_sub, u32 stride, u64* __restrict__ out, u32* __restrict__ out_w,
                                                                        u32 tile_keys, u32* __restrict__ digit_counts) {
    KATOME_SHIFT64_GUARD(24);        // (<2, 2, false> needs 24 VGPRs with sub_window's shift amount in v23: the gfx950 erratum, common.h)
    __shared__ u32 h[256];
    const u64 n = n_tiles * n_sub;
    const u64 n_out_tiles = digit_counts ? (n + tile_keys - 1) / tile_keys : 1;
    for (u64 ot = digit_counts ? blockIdx.x : 0; ot < n_out_tiles; ot += digit_counts ? gridDim.x : 1) {
    if (digit_counts) { h[threadIdx.x] = 0; __syncthreads(); }
    const u64 p_first = digit_counts ? ot * tile_keys + threadIdx.x : (u64)blockIdx.x * BLOCK + threadIdx.x;
    const u64 p_end = digit_counts ? (ot * tile_keys + tile_keys < n ? ot * tile_keys + tile_keys : n) : n;
    const u64 p_step = digit_counts ? (u64)BLOCK : (u64)gridDim.x * BLOCK;
    for (u64 p = p_first; p < p_end; p += p_step) {
        const u64 t = p / n_sub;
        const u32 o = (u32)(p - t * n_sub);
        Key<NWT> tile;
#pragma unroll
        for (int q = 0; q < NWT; ++q) tile.w[q] = list[t * (NWT + 1) + q];
        const u64 tag = list[t * (NWT + 1) + NWT];
        Key<NWK> x = sub_window<NWT, NWK>(tile, sub_len, n_sub, stride, o);
        bool flipped = false;
        if (RC) x = canonical_flip(x, sub_len, flipped);
        const u32 a = (u32)((tag >> 16) & 0xFFFFull) + o * stride, b = RC ? (u32)(tag & 0xFFFFull) + (n_sub - 1 - o) * stride : 0u;
#pragma unroll
        for (int q = 0; q < NWK; ++q) out[p * (NWK + 1) + q] = x.w[q];
        out[p * (NWK + 1) + NWK] = seen_pack(tag >> 32, flipped ? b : a, flipped ? a : b);
        out_w[p] = counts[t];
        if (digit_counts) atomicAdd(&h[(u32)(hash_key(x) >> 48) & 255u], 1u);        // (HashTaggedDigit: the key's words only)
    }
    if (digit_counts) { __syncthreads(); digit_counts[ot * 256 + threadIdx.x] = h[threadIdx.x]; __syncthreads(); }
    }
}

// ---- host side --------------------------------------------------------------------------------

int table_alloc(Table& t, uint32_t nw, uint64_t cap, hipStream_t stream) {
    if (cap < 1024) cap = 1024;
    t.nw = nw; t.cap = cap;
    KCHECK(t.slots.alloc(cap * t.slot_bytes(), stream));
    KCHECK(t.counter.alloc(sizeof(TableAux), stream));
    if (t.track_seen) {
        KCHECK(t.seen.alloc(cap * 16, stream));
        // All-ones also where the pair is stored inside the claim (keys of two and three words): lower_seen looks at the pair
        // through the caches first, and a cached line may predate the claim -- a stale all-ones only costs an atomicMin, stale
        // left-overs of an earlier table would make it skip one it needs (seen as a 1-in-8 wrong order on a two-rank build).
        KCHECK_HIP(hipMemsetAsync(t.seen.p, 0xFF, cap * 16, stream));
    }
    KCHECK_HIP(hipMemsetAsync(t.slots.p, 0, cap * t.slot_bytes(), stream));
    KCHECK_HIP(hipMemsetAsync(t.counter.p, 0, sizeof(TableAux), stream));
    return KATOME_OK;
}

int table_occupied(Table& t, uint64_t* out, hipStream_t stream) {
    TableAux aux;
    KCHECK_HIP(hipMemcpyAsync(&aux, t.counter.p, sizeof aux, hipMemcpyDeviceToHost, stream));
    KCHECK_HIP(hipStreamSynchronize(stream));
    if (aux.err) { set_error("k-mer table probe failure (code %u): table full or claim stuck", aux.err); return KATOME_E_DEVICE; }
    *out = aux.occupied;
    return KATOME_OK;
}

int table_insert(Table& t, const uint64_t* d_records, const uint32_t* d_weights, uint64_t n, hipStream_t stream,
                 const SeenOrigin* origin) {
    if (n == 0) return KATOME_OK;
    TableAux* aux = t.counter.as<TableAux>();
    dim3 grid(grid_for(n, BLOCK, 256u * 32u)), block(BLOCK);
    SeenParams sp{};
    if (t.track_seen) {
        if (!origin) { set_error("first-seen order: records must come with their position in the read stream"); return KATOME_E_ARG; }
        sp.seen = t.seen.as<u64>(); sp.read0 = origin->read0; sp.rec0 = origin->rec0; sp.per_read = origin->per_read;
        sp.span = origin->span; sp.windows = origin->windows; sp.rc = origin->rc; sp.win0 = origin->win0;
        sp.win_prefix = origin->win_prefix; sp.n_reads = origin->n_reads; sp.seq_base = origin->seq_base;
        sp.rec_prefix = origin->rec_prefix ? origin->rec_prefix : origin->win_prefix; sp.mode = origin->mode;
        sp.idx = origin->idx; sp.n_seg = origin->n_seg; sp.pairs = origin->pairs;
        for (int i = 0; i <= KATOME_MAX_RANKS; ++i) sp.seg_off[i] = origin->seg_off[i];
        for (int i = 0; i < KATOME_MAX_RANKS; ++i) sp.seg_read0[i] = origin->seg_read0[i];
        if (t.nw == 1)
            hipLaunchKernelGGL((insert_kernel<1, true>), grid, block, 0, stream, t.slots.as<Slot1>(), t.cap, d_records, d_weights, n, &aux->occupied, &aux->err, sp);
        else if (t.nw == 2)
            hipLaunchKernelGGL((insert_kernel<2, true>), grid, block, 0, stream, t.slots.as<Slot2>(), t.cap, d_records, d_weights, n, &aux->occupied, &aux->err, sp);
        else
            hipLaunchKernelGGL((insert_kernel<3, true>), grid, block, 0, stream, t.slots.as<Slot3>(), t.cap, d_records, d_weights, n, &aux->occupied, &aux->err, sp);
    } else if (t.nw == 1)
        hipLaunchKernelGGL((insert_kernel<1, false>), grid, block, 0, stream, t.slots.as<Slot1>(), t.cap, d_records, d_weights, n, &aux->occupied, &aux->err, sp);
    else if (t.nw == 2)
        hipLaunchKernelGGL((insert_kernel<2, false>), grid, block, 0, stream, t.slots.as<Slot2>(), t.cap, d_records, d_weights, n, &aux->occupied, &aux->err, sp);
    else
        hipLaunchKernelGGL((insert_kernel<3, false>), grid, block, 0, stream, t.slots.as<Slot3>(), t.cap, d_records, d_weights, n, &aux->occupied, &aux->err, sp);
    KCHECK_HIP(hipGetLastError());
    return KATOME_OK;
}

int table_grow(Table& t, uint64_t new_cap, hipStream_t stream) {
    Table nt;
    nt.track_seen = t.track_seen;
    KCHECK(table_alloc(nt, t.nw, new_cap, stream));
    TableAux* aux = nt.counter.as<TableAux>();
    dim3 grid(grid_for(t.cap, BLOCK, 256u * 32u)), block(BLOCK);
    const u64* os = t.track_seen ? t.seen.as<u64>() : nullptr; u64* ns = t.track_seen ? nt.seen.as<u64>() : nullptr;
    if (t.nw == 1)
        hipLaunchKernelGGL(rehash_kernel<1>, grid, block, 0, stream, t.slots.as<Slot1>(), t.cap, nt.slots.as<Slot1>(), nt.cap, &aux->occupied, &aux->err, os, ns);
    else if (t.nw == 2)
        hipLaunchKernelGGL(rehash_kernel<2>, grid, block, 0, stream, t.slots.as<Slot2>(), t.cap, nt.slots.as<Slot2>(), nt.cap, &aux->occupied, &aux->err, os, ns);
    else
        hipLaunchKernelGGL(rehash_kernel<3>, grid, block, 0, stream, t.slots.as<Slot3>(), t.cap, nt.slots.as<Slot3>(), nt.cap, &aux->occupied, &aux->err, os, ns);
    KCHECK_HIP(hipGetLastError());
    t.slots.adopt(nt.slots.take(), new_cap * t.slot_bytes());
    t.counter.adopt(nt.counter.take(), sizeof(TableAux));
    if (t.track_seen) t.seen.adopt(nt.seen.take(), new_cap * 16);
    t.cap = new_cap;
    return KATOME_OK;
}

// tile-table slots [slot0, slot1); every tile holds `span` windows of `k` bases, `stride` bases apart
template <bool TO_TABLE>
static int expand_launch(Table& tiles, u64 slot0, u64 slot1, Table* kmers, uint32_t k, uint32_t span, uint32_t stride, bool rc,
                         u64* out_keys, u32* out_w, u64* cursor, hipStream_t stream, u64* out_seen = nullptr) {
    const uint32_t nwk = (uint32_t)key_words_for_k(k);
    TableAux* aux = kmers ? kmers->counter.as<TableAux>() : nullptr;
    if (slot1 <= slot0) return KATOME_OK;
    dim3 grid(grid_for(slot1 - slot0, BLOCK, 256u * 32u)), block(BLOCK);
    KernelScope ks(K_EXPAND, stream, slot1 - slot0);
#define KATOME_EXPAND(NWT, NWK, RCV)                                                                                          \
    hipLaunchKernelGGL((expand_tiles_kernel<NWT, NWK, RCV, TO_TABLE>), grid, block, 0, stream, tiles.slots.as<SlotOf<NWT>::type>(), \
                       slot0, slot1, k, span, stride, kmers ? kmers->slots.as<SlotOf<NWK>::type>() : nullptr, kmers ? kmers->cap : 0,     \
                       aux ? &aux->occupied : nullptr, aux ? &aux->err : nullptr, out_keys, out_w, cursor,                      \
                       ((kmers && kmers->track_seen) || out_seen) ? tiles.seen.as<u64>() : nullptr,                            \
                       (kmers && kmers->track_seen) ? kmers->seen.as<u64>() : out_seen)
    if (tiles.nw == 1) { if (rc) KATOME_EXPAND(1, 1, true); else KATOME_EXPAND(1, 1, false); }
    else if (tiles.nw == 2) {
        if (nwk == 1) { if (rc) KATOME_EXPAND(2, 1, true); else KATOME_EXPAND(2, 1, false); }
        else          { if (rc) KATOME_EXPAND(2, 2, true); else KATOME_EXPAND(2, 2, false); }
    } else {                   // three-word tiles: into mid tiles of three or two words, or into k-mers of two
        if (nwk == 3)      { if (rc) KATOME_EXPAND(3, 3, true); else KATOME_EXPAND(3, 3, false); }
        else if (nwk == 2) { if (rc) KATOME_EXPAND(3, 2, true); else KATOME_EXPAND(3, 2, false); }
        else { set_error("expand: three-word tiles of one-word windows"); return KATOME_E_ARG; }
    }
#undef KATOME_EXPAND
    KCHECK_HIP(hipGetLastError());
    return KATOME_OK;
}

int table_expand_tiles(Table& tiles, uint64_t slot0, uint64_t slot1, Table& kmers, uint32_t k, uint32_t span, uint32_t stride,
                       bool rc, hipStream_t stream) {
    return expand_launch<true>(tiles, slot0, slot1, &kmers, k, span, stride, rc, nullptr, nullptr, nullptr, stream);
}

int table_expand_tiles_to_records(Table& tiles, uint32_t k, uint32_t span, bool rc, DevBuf& keys, DevBuf& weights,
                                  uint64_t* n_records, hipStream_t stream, DevBuf* seen) {
    return table_expand_tiles_to_subtiles(tiles, k, span, 1, rc, keys, weights, n_records, stream, seen);
}
// every distinct tile -> its `span` sub-windows of `k` bases, `stride` bases apart (stride 1: its k-mers; stride > 1: the
// shorter tiles of the next level), each with the tile's count [and its two sequence numbers]
int table_expand_tiles_to_subtiles(Table& tiles, uint32_t k, uint32_t span, uint32_t stride, bool rc, DevBuf& keys, DevBuf& weights,
                                   uint64_t* n_records, hipStream_t stream, DevBuf* seen) {
    uint64_t occ = 0;
    KCHECK(table_occupied(tiles, &occ, stream));
    const uint32_t nwk = (uint32_t)key_words_for_k(k);
    KCHECK(keys.alloc((occ * span + 1) * 8 * nwk, stream));
    KCHECK(weights.alloc((occ * span + 1) * 4, stream));
    u64* out_seen = nullptr;
    if (seen && tiles.track_seen) { KCHECK(seen->alloc((occ * span + 1) * 16, stream)); out_seen = seen->as<u64>(); }
    DevBuf cursor(stream);
    KCHECK(cursor.alloc(8));
    KCHECK_HIP(hipMemsetAsync(cursor.p, 0, 8, stream));
    if (!out_seen && tiles.nw == 2 && nwk == 2) {
        // two-word tiles into two-word sub-tiles without sequence numbers (C3's 60-mers into 36-mers on the sharded route): the
        // compacting kernel of the last level, 3.0 -> 0.6 ms for an eighth of C3
        dim3 grid(grid_for(tiles.cap, BLOCK * TR_ITEMS, 256u * 8u)), block(BLOCK);
        KernelScope ks(K_RECORDS, stream, tiles.cap);
        if (rc) hipLaunchKernelGGL((tiles_to_records_kernel<2, 2, true>), grid, block, 0, stream, tiles.slots.as<Slot2>(), tiles.cap, k, span, stride, keys.as<u64>(), weights.as<u32>(), cursor.as<u64>());
        else    hipLaunchKernelGGL((tiles_to_records_kernel<2, 2, false>), grid, block, 0, stream, tiles.slots.as<Slot2>(), tiles.cap, k, span, stride, keys.as<u64>(), weights.as<u32>(), cursor.as<u64>());
        KCHECK_HIP(hipGetLastError());
    } else
    KCHECK(expand_launch<false>(tiles, 0, tiles.cap, nullptr, k, span, stride, rc, keys.as<u64>(), weights.as<u32>(), cursor.as<u64>(), stream, out_seen));
    KCHECK_HIP(hipMemcpyAsync(n_records, cursor.p, 8, hipMemcpyDeviceToHost, stream));
    KCHECK_HIP(hipStreamSynchronize(stream));
#ifdef KATOME_DEBUG_DUMP
    // diagnostic builds only (tools/make_pair_store_variants.py): the records as the kernel left them, one file per call
    if (const char* prefix = getenv("KATOME_DUMP_RECORDS")) {
        static std::atomic<int> calls{0};
        char path[512];
        snprintf(path, sizeof path, "%s.%d.bin", prefix, calls.fetch_add(1));
        const uint64_t n = *n_records;
        std::vector<uint64_t> hk(n * nwk + 1), hs(out_seen ? 2 * n + 1 : 1);
        std::vector<uint32_t> hw(n + 1);
        KCHECK_HIP(hipMemcpy(hk.data(), keys.p, n * nwk * 8, hipMemcpyDeviceToHost));
        KCHECK_HIP(hipMemcpy(hw.data(), weights.p, n * 4, hipMemcpyDeviceToHost));
        if (out_seen) KCHECK_HIP(hipMemcpy(hs.data(), out_seen, n * 16, hipMemcpyDeviceToHost));
        if (FILE* f = fopen(path, "wb")) {
            const uint64_t head[8] = {n, nwk, k, span, stride, out_seen ? 1u : 0u, tiles.nw, tiles.cap};
            fwrite(head, 8, 8, f); fwrite(hk.data(), 8, n * nwk, f); fwrite(hw.data(), 4, n, f);
            if (out_seen) fwrite(hs.data(), 8, 2 * n, f);
            fclose(f);
        }
    }
#endif
    return KATOME_OK;
}

// (key, count[, both sequence numbers]) of every key in the table: what a rank of the sharded build sends to the keys' owners
int table_to_records(Table& t, DevBuf& keys, DevBuf& weights, uint64_t* n_records, hipStream_t stream, DevBuf* seen_pairs) {
    uint64_t occ = 0;
    KCHECK(table_occupied(t, &occ, stream));
    KCHECK(keys.alloc((occ + 1) * 8 * t.nw, stream));
    KCHECK(weights.alloc((occ + 1) * 4, stream));
    const u64* seen = nullptr; u64* out_seen = nullptr;
    if (seen_pairs && t.track_seen) { KCHECK(seen_pairs->alloc((occ + 1) * 16, stream)); seen = t.seen.as<u64>(); out_seen = seen_pairs->as<u64>(); }
    DevBuf cursor(stream);
    KCHECK(cursor.alloc(8));
    KCHECK_HIP(hipMemsetAsync(cursor.p, 0, 8, stream));
    const u32 cap_rec = BLOCK * 4;
    const size_t lds = (size_t)cap_rec * (8 * t.nw + 4 + (seen ? 16 : 0));
    dim3 grid(grid_for(t.cap, cap_rec, 256u * 16u)), block(BLOCK);
    if (t.nw == 1) hipLaunchKernelGGL(table_records_kernel<1>, grid, block, lds, stream, t.slots.as<Slot1>(), t.cap, keys.as<u64>(), weights.as<u32>(), cursor.as<u64>(), seen, out_seen);
    else           hipLaunchKernelGGL(table_records_kernel<2>, grid, block, lds, stream, t.slots.as<Slot2>(), t.cap, keys.as<u64>(), weights.as<u32>(), cursor.as<u64>(), seen, out_seen);
    KCHECK_HIP(hipGetLastError());
    KCHECK_HIP(hipMemcpyAsync(n_records, cursor.p, 8, hipMemcpyDeviceToHost, stream));
    KCHECK_HIP(hipStreamSynchronize(stream));
    return KATOME_OK;
}

// the (sub-window, count) records of a compact list of distinct tiles (list_to_records_kernel); extra_room: see below
int table_list_to_records(const uint64_t* d_tiles, const uint32_t* d_counts, uint64_t n_tiles, uint32_t tile_bases, uint32_t k, uint32_t span, uint32_t stride, bool rc,
                          DevBuf& keys, DevBuf& weights, uint64_t* n_records, hipStream_t stream, uint64_t extra_room, DevBuf* first_counts, bool rep) {
    const uint32_t nwt = (uint32_t)key_words_for_k(tile_bases), nwk = (uint32_t)key_words_for_k(k);
    if (rep && (nwk != 1 || nwt > 2 || k < 9 || (rc && !(k & 1)))) { set_error("records in their representative orientation: one-word k-mers, k >= 9, odd k or one strand"); return KATOME_E_ARG; }
    *n_records = n_tiles * span;
    KCHECK(keys.alloc((*n_records + extra_room + 1) * 8 * nwk, stream));
    KCHECK(weights.alloc((*n_records + extra_room + 1) * 4, stream));
    if (*n_records == 0) return KATOME_OK;
    // (first_counts: the caller sorts exactly these records next -- nothing appended -- and wants the first pass's digit counts per tile;
    // KATOME_FUSED_HIST=0: the pass counts them itself)
    static const bool fused_hist = !getenv("KATOME_FUSED_HIST") || atoi(getenv("KATOME_FUSED_HIST")) != 0;
    if (first_counts && fused_hist && !extra_room && ((nwt == 3 && nwk >= 2) || (nwt == 2 && nwk <= 2) || (nwt == 1 && nwk == 1))) {
        const uint32_t tile_keys = dev_sort_tile_keys(nwk);
        const uint64_t n_out_tiles = (*n_records + tile_keys - 1) / tile_keys;
        KCHECK(first_counts->alloc(n_out_tiles * 256 * 4 + 16, stream));
        const dim3 hgrid(grid_for(n_out_tiles, 1, 256u * 32u)), block(BLOCK);
        KernelScope ks(K_RECORDS, stream, n_tiles);
#define KATOME_LRH_REP(NWT, RCV) hipLaunchKernelGGL((list_to_records_hist_kernel<NWT, 1, RCV, true>), hgrid, block, 0, stream, d_tiles, d_counts, n_tiles, k, span, stride, keys.as<u64>(), weights.as<u32>(), tile_keys, first_counts->as<u32>())
#define KATOME_LRH(NWT, NWK)                                                                                                            \
        do {                                                                                                                          \
            if (rc) hipLaunchKernelGGL((list_to_records_hist_kernel<NWT, NWK, true>), hgrid, block, 0, stream, d_tiles, d_counts, n_tiles, k, span, stride, keys.as<u64>(), weights.as<u32>(), tile_keys, first_counts->as<u32>()); \
            else    hipLaunchKernelGGL((list_to_records_hist_kernel<NWT, NWK, false>), hgrid, block, 0, stream, d_tiles, d_counts, n_tiles, k, span, stride, keys.as<u64>(), weights.as<u32>(), tile_keys, first_counts->as<u32>()); \
        } while (0)
        if (rep) {               // (the ordered count's records: dev_key_order's first digit)
            if (nwt == 2) { if (rc) KATOME_LRH_REP(2, true); else KATOME_LRH_REP(2, false); }
            else          { if (rc) KATOME_LRH_REP(1, true); else KATOME_LRH_REP(1, false); }
        } else
        if (nwt == 3 && nwk == 3) KATOME_LRH(3, 3);
        else if (nwt == 3 && nwk == 2) KATOME_LRH(3, 2);
        else if (nwt == 2 && nwk == 2) KATOME_LRH(2, 2);
        else if (nwt == 2 && nwk == 1) KATOME_LRH(2, 1);
        else KATOME_LRH(1, 1);
#undef KATOME_LRH
#undef KATOME_LRH_REP
        KCHECK_HIP(hipGetLastError());
        return KATOME_OK;
    }
    if (first_counts) first_counts->release();
    const dim3 grid(grid_for(*n_records, BLOCK, 256u * 32u)), block(BLOCK);
    KernelScope ks(K_RECORDS, stream, n_tiles);
#define KATOME_LR_REP(NWT, RCV) hipLaunchKernelGGL((list_to_records_kernel<NWT, 1, RCV, true>), grid, block, 0, stream, d_tiles, d_counts, n_tiles, k, span, stride, keys.as<u64>(), weights.as<u32>())
#define KATOME_LR(NWT, NWK)                                                                                                             \
    do {                                                                                                                              \
        if (rc) hipLaunchKernelGGL((list_to_records_kernel<NWT, NWK, true>), grid, block, 0, stream, d_tiles, d_counts, n_tiles, k, span, stride, keys.as<u64>(), weights.as<u32>()); \
        else    hipLaunchKernelGGL((list_to_records_kernel<NWT, NWK, false>), grid, block, 0, stream, d_tiles, d_counts, n_tiles, k, span, stride, keys.as<u64>(), weights.as<u32>()); \
    } while (0)
    if (rep) {
        if (nwt == 2) { if (rc) KATOME_LR_REP(2, true); else KATOME_LR_REP(2, false); }
        else          { if (rc) KATOME_LR_REP(1, true); else KATOME_LR_REP(1, false); }
    } else
    if (nwt == 3 && nwk == 3) KATOME_LR(3, 3);
    else if (nwt == 3 && nwk == 2) KATOME_LR(3, 2);
    else if (nwt == 2 && nwk == 2) KATOME_LR(2, 2);
    else if (nwt == 2 && nwk == 1) KATOME_LR(2, 1);
    else if (nwt == 1 && nwk == 1) KATOME_LR(1, 1);
    else { set_error("records of a tile list: tiles of %u words into windows of %u", nwt, nwk); return KATOME_E_UNSUPPORTED; }
#undef KATOME_LR
#undef KATOME_LR_REP
    KCHECK_HIP(hipGetLastError());
    return KATOME_OK;
}

// the (k-mer, count) records of every distinct tile of the last level (no sequence numbers), written by the streaming kernel
int table_tiles_to_records_fast(Table& tiles, uint32_t k, uint32_t span, bool rc, DevBuf& keys, DevBuf& weights, uint64_t* n_records, hipStream_t stream,
                                uint64_t extra_room) {
    uint64_t occ = 0;
    KCHECK(table_occupied(tiles, &occ, stream));
    const uint32_t nwk = (uint32_t)key_words_for_k(k);
    const bool streaming = (nwk == 1 && (tiles.nw == 1 || tiles.nw == 2)) || (nwk == 2 && (tiles.nw == 2 || tiles.nw == 3));
    if (!streaming) {
        if (extra_room) { set_error("records of this tile shape cannot be extended"); return KATOME_E_UNSUPPORTED; }
        return table_expand_tiles_to_records(tiles, k, span, rc, keys, weights, n_records, stream, nullptr);
    }
    KCHECK(keys.alloc((occ * span + extra_room + 1) * 8 * nwk, stream));
    KCHECK(weights.alloc((occ * span + extra_room + 1) * 4, stream));
    DevBuf cursor(stream);
    KCHECK(cursor.alloc(8));
    KCHECK_HIP(hipMemsetAsync(cursor.p, 0, 8, stream));
    dim3 grid(grid_for(tiles.cap, BLOCK * TR_ITEMS, 256u * 8u)), block(BLOCK);
    KernelScope ks(K_RECORDS, stream, tiles.cap);
#define KATOME_TR(NWT, NWK)                                                                                                                       \
    do {                                                                                                                                          \
        if (rc) hipLaunchKernelGGL((tiles_to_records_kernel<NWT, NWK, true>), grid, block, 0, stream, tiles.slots.as<SlotOf<NWT>::type>(), tiles.cap, k, span, 1u, keys.as<u64>(), weights.as<u32>(), cursor.as<u64>()); \
        else    hipLaunchKernelGGL((tiles_to_records_kernel<NWT, NWK, false>), grid, block, 0, stream, tiles.slots.as<SlotOf<NWT>::type>(), tiles.cap, k, span, 1u, keys.as<u64>(), weights.as<u32>(), cursor.as<u64>()); \
    } while (0)
    if (nwk == 1) { if (tiles.nw == 1) KATOME_TR(1, 1); else KATOME_TR(2, 1); }
    else          { if (tiles.nw == 2) KATOME_TR(2, 2); else KATOME_TR(3, 2); }
#undef KATOME_TR
    KCHECK_HIP(hipGetLastError());
    KCHECK_HIP(hipMemcpyAsync(n_records, cursor.p, 8, hipMemcpyDeviceToHost, stream));
    KCHECK_HIP(hipStreamSynchronize(stream));
    return KATOME_OK;
}

int table_keep_rest(const uint64_t* d_rec, uint64_t n, uint32_t nw, bool tagged, uint64_t read0, uint32_t per_read, uint32_t win0, uint32_t seq_per_read,
                    uint64_t* d_out, uint64_t* d_cursor, hipStream_t stream, uint32_t win_stride, uint32_t span) {
    if (n == 0) return KATOME_OK;
    const dim3 grid(grid_for(n, BLOCK * KR_ITEMS, 256u * 8u)), block(BLOCK);
    unsigned long long* cur = reinterpret_cast<unsigned long long*>(d_cursor);
    if (!per_read) per_read = 1;
#define KATOME_KR(NWV, TAG) hipLaunchKernelGGL((keep_rest_kernel<NWV, TAG>), grid, block, 0, stream, d_rec, n, read0, per_read, win0, seq_per_read, d_out, cur, win_stride, span)
    if (nw == 3 && tagged) { set_error("tagged records: keys of one or two words"); return KATOME_E_UNSUPPORTED; }
    if (nw == 1) { if (tagged) KATOME_KR(1, true); else KATOME_KR(1, false); }
    else if (nw == 3) KATOME_KR(3, false);
    else         { if (tagged) KATOME_KR(2, true); else KATOME_KR(2, false); }
#undef KATOME_KR
    KCHECK_HIP(hipGetLastError());
    return KATOME_OK;
}
int table_tagged_to_pairs(const uint64_t* d_tagged, uint64_t n, uint32_t nw, uint64_t seq_per_read, uint64_t* d_keys, uint64_t* d_pairs, hipStream_t stream) {
    if (n == 0) return KATOME_OK;
    const dim3 grid(grid_for(n, BLOCK, 256u * 16u)), block(BLOCK);
    if (nw == 1) hipLaunchKernelGGL(tagged_to_pairs_kernel<1>, grid, block, 0, stream, d_tagged, n, seq_per_read, d_keys, d_pairs);
    else         hipLaunchKernelGGL(tagged_to_pairs_kernel<2>, grid, block, 0, stream, d_tagged, n, seq_per_read, d_keys, d_pairs);
    KCHECK_HIP(hipGetLastError());
    return KATOME_OK;
}

// the tagged records of the next level out of a list of distinct tiles with their tags and counts (list_to_tagged_records_kernel)
int table_list_to_tagged_records(const uint64_t* d_list, const uint32_t* d_counts, uint64_t n_tiles, uint32_t tile_bases, uint32_t sub_len, uint32_t n_sub,
                                 uint32_t stride, bool rc, DevBuf& recs, DevBuf& weights, uint64_t* n_records, hipStream_t stream, uint64_t extra_room,
                                 DevBuf* first_counts) {
    const uint32_t nwt = (uint32_t)key_words_for_k(tile_bases), nwk = (uint32_t)key_words_for_k(sub_len);
    *n_records = n_tiles * n_sub;
    KCHECK(recs.alloc((*n_records + extra_room + 1) * 8 * (nwk + 1), stream));
    KCHECK(weights.alloc((*n_records + extra_room + 1) * 4, stream));
    if (*n_records == 0) { if (first_counts) first_counts->release(); return KATOME_OK; }
    static const bool fused_hist = !getenv("KATOME_FUSED_HIST") || atoi(getenv("KATOME_FUSED_HIST")) != 0;
    const bool with_counts = first_counts && fused_hist && !extra_room;
    const uint32_t tile_keys = dev_sort_tile_keys(nwk + 1);
    const uint64_t n_out_tiles = (*n_records + tile_keys - 1) / tile_keys;
    u32* d_digit_counts = nullptr;
    if (with_counts) { KCHECK(first_counts->alloc(n_out_tiles * 256 * 4 + 16, stream)); d_digit_counts = first_counts->as<u32>(); }
    else if (first_counts) first_counts->release();
    const dim3 grid(with_counts ? grid_for(n_out_tiles, 1, 256u * 32u) : grid_for(*n_records, BLOCK, 256u * 32u)), block(BLOCK);
    KernelScope ks(K_RECORDS, stream, n_tiles);
#define KATOME_LT(NWT, NWK)                                                                                                             \
    do {                                                                                                                              \
        if (rc) hipLaunchKernelGGL((list_to_tagged_records_kernel<NWT, NWK, true>), grid, block, 0, stream, d_list, d_counts, n_tiles, sub_len, n_sub, stride, recs.as<u64>(), weights.as<u32>(), tile_keys, d_digit_counts); \
        else    hipLaunchKernelGGL((list_to_tagged_records_kernel<NWT, NWK, false>), grid, block, 0, stream, d_list, d_counts, n_tiles, sub_len, n_sub, stride, recs.as<u64>(), weights.as<u32>(), tile_keys, d_digit_counts); \
    } while (0)
    if (nwt == 2 && nwk == 2) KATOME_LT(2, 2);
    else if (nwt == 2 && nwk == 1) KATOME_LT(2, 1);
    else if (nwt == 1 && nwk == 1) KATOME_LT(1, 1);
    else { set_error("tagged records of a tile list: tiles of %u words into windows of %u", nwt, nwk); return KATOME_E_UNSUPPORTED; }
#undef KATOME_LT
    KCHECK_HIP(hipGetLastError());
    return KATOME_OK;
}

int tiles_to_edges_sorted_seen(Table& tiles, uint32_t k, uint32_t span, bool rc, uint64_t seq_per_read, DevBuf& edge_key, DevBuf& seq_weight,
                               uint64_t* n_edges, uint64_t* n_distinct, hipStream_t stream, const uint64_t* d_extra, uint64_t n_extra) {
    *n_edges = 0; *n_distinct = 0;
    const uint32_t nwk = (uint32_t)key_words_for_k(k), stride = nwk + 1;
    const bool shapes = tiles.track_seen && ((nwk == 1 && tiles.nw <= 2) || (nwk == 2 && (tiles.nw == 2 || tiles.nw == 3)));
    if (!shapes || seq_per_read == 0 || seq_per_read > 0xFFFFu) return KATOME_E_UNSUPPORTED;
    uint64_t occ = 0;
    KCHECK(table_occupied(tiles, &occ, stream));
    const u64 bound = occ * span + n_extra;
    constexpr u32 FILL = (u32)(LC_THREADS * LCS_PER / 4096.0 * 2900);
    if (bound >= (1ull << 32) || (bound >> 16) > (u64)LC_MAX_ROUNDS * FILL) return KATOME_E_UNSUPPORTED;
    DevBuf recs(stream), wts(stream), aux(stream);
    KCHECK(recs.alloc((bound + 1) * 8 * stride));
    KCHECK(wts.alloc((bound + 1) * 4));
    KCHECK(aux.alloc(64));
    KCHECK_HIP(hipMemsetAsync(aux.p, 0, 64, stream));
    u32* err = reinterpret_cast<u32*>(aux.as<unsigned long long>() + 2);
    u64* rec_cursor = aux.as<u64>() + 3;
    {
        KernelScope ks(K_RECORDS, stream, tiles.cap);
        const dim3 grid(grid_for(tiles.cap, BLOCK * TR_ITEMS, 256u * 8u)), block(BLOCK);
        const u64 magic = ~0ull / seq_per_read + 1;
#define KATOME_SR(NWT, NWK)                                                                                                              \
        do {                                                                                                                             \
            const size_t lds = (size_t)BLOCK * TR_ITEMS * (8 * NWT + 8 + 8 + 4);                                                         \
            if (rc) { KCHECK_HIP(hipFuncSetAttribute((const void*)seen_records_kernel<NWT, NWK, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
                      hipLaunchKernelGGL((seen_records_kernel<NWT, NWK, true>), grid, block, lds, stream, tiles.slots.as<SlotOf<NWT>::type>(), tiles.seen.as<u64>(), tiles.cap, k, span, seq_per_read, magic, recs.as<u64>(), wts.as<u32>(), rec_cursor, err); } \
            else    { KCHECK_HIP(hipFuncSetAttribute((const void*)seen_records_kernel<NWT, NWK, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
                      hipLaunchKernelGGL((seen_records_kernel<NWT, NWK, false>), grid, block, lds, stream, tiles.slots.as<SlotOf<NWT>::type>(), tiles.seen.as<u64>(), tiles.cap, k, span, seq_per_read, magic, recs.as<u64>(), wts.as<u32>(), rec_cursor, err); } \
        } while (0)
        if (nwk == 1) { if (tiles.nw == 1) KATOME_SR(1, 1); else KATOME_SR(2, 1); }
        else          { if (tiles.nw == 2) KATOME_SR(2, 2); else KATOME_SR(3, 2); }
#undef KATOME_SR
        KCHECK_HIP(hipGetLastError());
    }
    uint64_t h[4] = {0, 0, 0, 0};
    KCHECK_HIP(hipMemcpyAsync(h, aux.p, 32, hipMemcpyDeviceToHost, stream));
    KCHECK_HIP(hipStreamSynchronize(stream));
    if ((uint32_t)h[2]) return KATOME_E_UNSUPPORTED;                 // (sequence numbers that do not pack)
    u64 n = h[3];
    if (n_extra) {                                                   // the left-over windows behind them, one each
        KCHECK_HIP(hipMemcpyAsync(recs.as<u64>() + n * stride, d_extra, n_extra * 8 * stride, hipMemcpyDeviceToDevice, stream));
        KCHECK(dev_fill_u32(wts.as<u32>() + n, n_extra, 1u, stream));
        n += n_extra;
    }
    return tagged_records_sorted(recs, wts, n, k, rc, seq_per_read, false, edge_key, seq_weight, n_edges, n_distinct, stream);
}

// Tagged records [n][nwk + 1] (key, read << 32 | offset << 16 | offset) with their counts -> two hash passes on the key, counted in LDS
// with the two numbers lowered (lds_count_seen_kernel).  list == false: the oriented edges, out_keys [e][nwk] + out_second [e][2] =
// {sequence number, weight}.  list == true (a tile level): the distinct keys with their tags, out_keys [d][nwk + 1], and their counts,
// out_second [d] u32.  The records come back permuted.
int tagged_records_sorted(DevBuf& recs, DevBuf& wts, uint64_t n, uint32_t k, bool rc, uint64_t seq_per_read, bool list, DevBuf& edge_key,
                          DevBuf& seq_weight, uint64_t* n_edges, uint64_t* n_distinct, hipStream_t stream, uint32_t* first_counts) {
    *n_edges = 0; *n_distinct = 0;
    const uint32_t nwk = (uint32_t)key_words_for_k(k), stride = nwk + 1;
    constexpr u32 FILL = (u32)(LC_THREADS * LCS_PER / 4096.0 * 2900);
    if (nwk > 2 || seq_per_read == 0 || seq_per_read > 0xFFFFu || n >= (1ull << 32) || (n >> 16) > (u64)LC_MAX_ROUNDS * FILL) return KATOME_E_UNSUPPORTED;
    DevBuf aux(stream);
    KCHECK(aux.alloc(64));
    KCHECK_HIP(hipMemsetAsync(aux.p, 0, 64, stream));
    unsigned long long* cursor = aux.as<unsigned long long>();
    unsigned long long* distinct = cursor + 1;
    u32* err = reinterpret_cast<u32*>(cursor + 2);
    uint64_t h[4] = {0, 0, 0, 0};
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
    const u32 R = (u32)std::max<u64>(1, (avg + FILL - 1) / FILL);
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
    auto count = [&](u32 rounds, u32 probe_limit) -> int {
        KCHECK_HIP(hipMemsetAsync(aux.p, 0, 24, stream));
        const size_t lds = (size_t)LC_THREADS * LCS_PER * 28;
        KernelScope ks(K_LDS_COUNT, stream, n);
#define KATOME_LCS(RCV, NWKV, LISTV)                                                                                                     \
        do {                                                                                                                             \
            KCHECK_HIP(hipFuncSetAttribute((const void*)lds_count_seen_kernel<RCV, NWKV, LISTV>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
            hipLaunchKernelGGL((lds_count_seen_kernel<RCV, NWKV, LISTV>), dim3(256u), dim3(LC_THREADS), lds, stream, ko, wo, index.as<u64>(), gbits, rounds, k, \
                               seq_per_read, edge_key.as<u64>(), seq_weight.as<u64>(), out_cap, cursor, distinct, err, probe_limit);     \
        } while (0)
        if (list)          { if (nwk == 1) { if (rc) KATOME_LCS(true, 1, true); else KATOME_LCS(false, 1, true); }
                             else          { if (rc) KATOME_LCS(true, 2, true); else KATOME_LCS(false, 2, true); } }
        else if (nwk == 1) { if (rc) KATOME_LCS(true, 1, false); else KATOME_LCS(false, 1, false); }
        else               { if (rc) KATOME_LCS(true, 2, false); else KATOME_LCS(false, 2, false); }
#undef KATOME_LCS
        KCHECK_HIP(hipGetLastError());
        KCHECK_HIP(hipMemcpyAsync(h, aux.p, 24, hipMemcpyDeviceToHost, stream));
        KCHECK_HIP(hipStreamSynchronize(stream));
        return KATOME_OK;
    };
    // first with fewer sub-rounds than would hold a group of distinct records (lc_optimism): records of reads repeat
    const u32 R_try = (u32)std::max<u64>(1, (u64)std::ceil((double)avg * lc_optimism() / FILL));
    if (R_try < R) { KCHECK(count(R_try, lc_probe_limit())); if ((uint32_t)h[2] == 3) { lc_trace("first-seen order", R_try, R); KCHECK(count(R, LC_THREADS * LCS_PER)); } }
    else KCHECK(count(R, LC_THREADS * LCS_PER));
    if ((uint32_t)h[2] == 4 || (uint32_t)h[2] == 6) return KATOME_E_UNSUPPORTED;
    if ((uint32_t)h[2]) { set_error("counting in LDS (first-seen order): a sub-round did not fit its table (code %u)", (unsigned)h[2]); return KATOME_E_DEVICE; }
    *n_edges = h[0]; *n_distinct = h[1];
    return KATOME_OK;
}

// (k-mer, count) records in any order -> oriented edges (both strands with rc, weights summed per k-mer, threshold applied): counted
// by sorting instead of in a table (see lds_count_kernel).  keys/weights: the records (consumed).  KATOME_E_UNSUPPORTED when
// the input is out of the kernel's range (the caller counts in the table instead).
int table_orient_records(uint64_t* d_keys, uint64_t n, uint32_t k, bool rep, hipStream_t stream) {
    if (!n) return KATOME_OK;
    KernelScope ks(K_RECORDS, stream, n);
    if (rep) hipLaunchKernelGGL(orient_records_kernel<true>, dim3(grid_for(n, BLOCK, 256u * 32u)), dim3(BLOCK), 0, stream, d_keys, n, k);
    else     hipLaunchKernelGGL(orient_records_kernel<false>, dim3(grid_for(n, BLOCK, 256u * 32u)), dim3(BLOCK), 0, stream, d_keys, n, k);
    KCHECK_HIP(hipGetLastError());
    return KATOME_OK;
}

// The ordered count of records_to_edges_sorted (lds_count_ordered_kernel).  KATOME_E_UNSUPPORTED: not this way -- the level's shape, a
// group of more distinct keys than the table holds (err 3: key ranges are far less even than hash ranges on skewed or low-complexity
// input) or a count beyond 16 bits (err 5); the records are then still all there, ordered by key, in their representative orientation.
static int ordered_count(DevBuf& keys, DevBuf& weights, uint64_t n, uint32_t k, bool rc, uint32_t min_weight, HalfSort& hs, uint64_t* n_edges,
                         uint64_t* n_distinct, hipStream_t stream, uint32_t* first_counts) {
    // (one visit per record: a group must fit the 8-byte-slot table at lds_count_packed_kernel's planning load)
    const u64 avg = n >> 16;
    if (!n || !weights.p || k < 9 || 2 * k > 62 || (rc && !(k & 1)) || (double)avg * 0.56 > LP_SLOTS * 0.66) return KATOME_E_UNSUPPORTED;
    const u64* ko = nullptr; const u32* wo = nullptr;
    {
        DevBuf kb(stream), wb(stream);
        KCHECK(kb.alloc((n + 1) * 8)); KCHECK(wb.alloc((n + 1) * 4));
        KCHECK(dev_key_order(keys.as<u64>(), weights.as<u32>(), n, k, kb.as<u64>(), keys.as<u64>(), wb.as<u32>(), weights.as<u32>(), &ko, &wo, stream,
                             first_counts));
    }
    KCHECK(hs.group_first.alloc(((1ull << 16) + 1) * 8, stream));
    KCHECK(dev_key_group_index(ko, n, 2 * k - 16, hs.group_first.as<u64>(), stream));
    KCHECK(hs.group_count.alloc((1ull << 16) * 4, stream));
    KCHECK_HIP(hipMemsetAsync(hs.group_count.p, 0, (1ull << 16) * 4, stream));
    KCHECK(hs.s1_key.alloc((n + 1) * 8, stream)); KCHECK(hs.s1_w.alloc((n + 1) * 4, stream));
    const u64 s2_cap = rc ? n + 1 : 0;          // (a reverse complement per distinct key: no more than the records)
    if (rc) {
        KCHECK(hs.s2_key.alloc(s2_cap * 8, stream)); KCHECK(hs.s2_w.alloc(s2_cap * 4, stream));
        KCHECK(hs.s2_digit.alloc(dev_digit_stream_bytes(s2_cap, 1), stream));
    }
    DevBuf aux(stream);
    KCHECK(aux.alloc(64));
    KCHECK_HIP(hipMemsetAsync(aux.p, 0, 64, stream));
    unsigned long long* cursor = aux.as<unsigned long long>();
    const size_t lds = (size_t)LP_SLOTS * 8 + LO_BUCKETS * 2;
    {
#define KATOME_LO_LAUNCH(RCV)                                                                                                               \
        do {                                                                                                                              \
            KCHECK_HIP(hipFuncSetAttribute((const void*)lds_count_ordered_kernel<RCV>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
            KernelScope ks(K_LDS_COUNT, stream, n);                                                                                       \
            hipLaunchKernelGGL((lds_count_ordered_kernel<RCV>), dim3(256u), dim3(LC_THREADS), lds, stream, ko, wo, hs.group_first.as<u64>(), k, min_weight, \
                               hs.s1_key.as<u64>(), hs.s1_w.as<u32>(), hs.group_count.as<u32>(), hs.s2_key.as<u64>(), hs.s2_w.as<u32>(), hs.s2_digit.as<uint8_t>(), s2_cap,   \
                               cursor, cursor + 1, reinterpret_cast<u32*>(cursor + 2), std::min<u32>(lc_probe_limit(), LP_SLOTS));              \
        } while (0)
        if (rc) KATOME_LO_LAUNCH(true); else KATOME_LO_LAUNCH(false);
#undef KATOME_LO_LAUNCH
    }
    KCHECK_HIP(hipGetLastError());
    uint64_t h[3] = {0, 0, 0};
    KCHECK_HIP(hipMemcpyAsync(h, aux.p, 24, hipMemcpyDeviceToHost, stream));
    KCHECK_HIP(hipStreamSynchronize(stream));
    if (getenv("KATOME_LC_TRACE")) fprintf(stderr, "[lds count] in key order, 8-byte slots, 1 visit(s) per record: code %u\n", (unsigned)h[2]);
    if ((uint32_t)h[2]) {
        if (getenv("KATOME_LC_TRACE")) fprintf(stderr, "[lds count] in key order: %s; counting by hash groups\n", (uint32_t)h[2] == 5 ? "a count over 16 bits" : "a group filled its table");
        hs.release();
        return KATOME_E_UNSUPPORTED;
    }
    hs.n_s1 = h[0]; hs.n_s2 = rc ? h[0] : 0; hs.k = k; hs.taken = true;
    *n_edges = hs.n_s1 + hs.n_s2; *n_distinct = h[1];
    return KATOME_OK;
}

// KATOME_S2_GROUP_SORT=0: S2 sorted in full and half_merge_kernel, as before group_merge_kernel.  KATOME_S2_GROUP_CAP=n: groups of more
// than n keys (and always more than the kernel's LDS holds) take that route too -- tests of the way back
static bool s2_group_sort_on() {
    static const bool on = !getenv("KATOME_S2_GROUP_SORT") || atoi(getenv("KATOME_S2_GROUP_SORT")) != 0;
    return on;
}
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
        {
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
        if (getenv("KATOME_LC_TRACE"))
            fprintf(stderr, "[half sort] S2: %llu keys, largest group %llu: %s\n", (unsigned long long)hs.n_s2, (unsigned long long)largest,
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
        static const bool heads = !getenv("KATOME_MERGE_HEADS") || atoi(getenv("KATOME_MERGE_HEADS")) != 0;
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

int records_to_edges_sorted(DevBuf& keys, DevBuf& weights, uint64_t n, uint32_t k, bool rc, uint32_t min_weight, DevBuf& edge_key,
                            DevBuf& edge_weight, uint64_t* n_edges, uint64_t* n_distinct, hipStream_t stream, OwnerSplit* split,
                            uint32_t* first_counts, HalfSort* half) {
    *n_edges = 0; *n_distinct = 0;
    if (half) {
        half->taken = false;
        const int orc = split ? KATOME_E_UNSUPPORTED : ordered_count(keys, weights, n, k, rc, min_weight, *half, n_edges, n_distinct, stream, first_counts);
        if (orc != KATOME_E_UNSUPPORTED) return orc;
        if (rc) KCHECK(table_orient_records(keys.as<u64>(), n, k, false, stream));      // (the usual route and the table take canonical k-mers)
        first_counts = nullptr;
    }
    const uint32_t nw = (uint32_t)key_words_for_k(k);
    if (nw > 3 || (nw == 3 && (rc || min_weight))) return KATOME_E_UNSUPPORTED;      // (three words: tiles of 64..95 bases -- never k-mers, so never oriented)
    if (split && (nw != 1 || rc || min_weight || split->n_parts == 0 || split->n_parts > (uint32_t)KATOME_MAX_RANKS)) {
        set_error("records by owner: one-word k-mers, one record per k-mer"); return KATOME_E_ARG;
    }
    if ((n >> 16) > (u64)LC_MAX_ROUNDS * LcTable<13>::FILL) return KATOME_E_UNSUPPORTED;
    const u64* ko = nullptr; const u32* wo = nullptr;
    u32 gbits = 16;
    // (weights not allocated: every record counts once; the passes move keys only.  Two-word keys: lds_count_wide_kernel)
    const bool unit = weights.p == nullptr;
    if (unit && (nw < 2 || split)) { set_error("records without weights: keys of two or three words"); return KATOME_E_ARG; }
    {
        DevBuf kb(stream), wb(stream);
        KCHECK(kb.alloc((n + 1) * 8 * nw));
        if (!unit) KCHECK(wb.alloc((n + 1) * 4));
        // two passes: the first one's output goes to the scratch, the second one's lands in keys / weights again
        if (split) KCHECK(dev_hash_order_core(keys.as<u64>(), weights.as<u32>(), n, split->core_shift, split->core_bases, kb.as<u64>(), keys.as<u64>(), wb.as<u32>(),
                                              weights.as<u32>(), &ko, &wo, &gbits, stream));
        else KCHECK(dev_hash_order(keys.as<u64>(), weights.as<u32>(), n, nw, kb.as<u64>(), keys.as<u64>(), wb.as<u32>(), weights.as<u32>(), &ko, &wo, &gbits, stream,
                                   first_counts));
    }
    // the smaller table when a group fits it in one round (less to clear and to read out per group)
    const u64 avg = n >> gbits;
    const bool small = avg <= LcTable<8>::FILL;
    const u32 fill = small ? LcTable<8>::FILL : LcTable<13>::FILL;
    const u32 R = (u32)std::max<u64>(1, (avg + fill - 1) / fill);          // sub-rounds: a group's share fits even if all new
    if (R > LC_MAX_ROUNDS) return KATOME_E_UNSUPPORTED;
    DevBuf index(stream), aux(stream);
    KCHECK(index.alloc(((1ull << gbits) + 1) * 8));
    KCHECK(aux.alloc(64));
    {
        KernelScope ks(K_GROUP_INDEX, stream, n);
        const dim3 igrid(grid_for((1ull << gbits) + 1, BLOCK));
        if (split)   hipLaunchKernelGGL(core_group_index_kernel, igrid, dim3(BLOCK), 0, stream, ko, n, gbits, split->core_shift, split->core_bases, index.as<u64>());
        else if (nw == 1) hipLaunchKernelGGL(hash_group_index_kernel<1>, igrid, dim3(BLOCK), 0, stream, ko, n, gbits, index.as<u64>());
        else if (nw == 3) hipLaunchKernelGGL(hash_group_index_kernel<3>, igrid, dim3(BLOCK), 0, stream, ko, n, gbits, index.as<u64>());
        else         hipLaunchKernelGGL(hash_group_index_kernel<2>, igrid, dim3(BLOCK), 0, stream, ko, n, gbits, index.as<u64>());
    }
    const uint64_t out_cap = (rc ? 2 : 1) * n + 1;
    KCHECK(edge_key.alloc(out_cap * 8 * nw, stream));
    KCHECK(edge_weight.alloc(out_cap * 4, stream));
    unsigned long long* cursor = aux.as<unsigned long long>();
    unsigned long long* distinct = cursor + 1;
    u32* err = reinterpret_cast<u32*>(cursor + 2);
    uint64_t h[3] = {0, 0, 0};
    // (with a split: the owners' cursors, started at the owners' first records -- a group's keys are no more than its records --, and
    // those starts themselves, n_parts + 1 of them)
    DevBuf owners(stream);
    unsigned long long* owner_cursor = nullptr;
    u64* owner_base = nullptr;
    if (split) {
        KCHECK(owners.alloc((2 * KATOME_MAX_RANKS + 2) * 8));
        owner_cursor = owners.as<unsigned long long>(); owner_base = owners.as<u64>() + KATOME_MAX_RANKS + 1;
    }
    const u32 n_owners = split ? split->n_parts : 0;
    auto count = [&](u32 rounds, u32 probe_limit) -> int {
        KCHECK_HIP(hipMemsetAsync(aux.p, 0, 64, stream));
        if (split) hipLaunchKernelGGL(owner_bases_kernel, dim3(1), dim3(64), 0, stream, index.as<u64>(), gbits, n_owners, owner_cursor, owner_base);
#define KATOME_LC_LAUNCH(KERNEL, PERV)                                                                                                  \
        do {                                                                                                                          \
            const size_t lds = (size_t)LcTable<PERV>::SLOTS * 12;                                                                     \
            KCHECK_HIP(hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));               \
            KernelScope ks(K_LDS_COUNT, stream, n);                                                                                   \
            hipLaunchKernelGGL(KERNEL, dim3(256u), dim3(LC_THREADS), lds, stream, ko, wo, index.as<u64>(), gbits, rounds, k,           \
                               min_weight, edge_key.as<u64>(), edge_weight.as<u32>(), out_cap, cursor, distinct, err,                  \
                               std::min<u32>(probe_limit, LcTable<PERV>::SLOTS), owner_cursor, n_owners);                              \
        } while (0)
        const bool even = (k & 1) == 0;          // (only read when rc: a tile level's records are never oriented)
        if (nw == 1) {
            if (small) { if (!rc) KATOME_LC_LAUNCH((lds_count_kernel<false, 8, false>), 8); else if (even) KATOME_LC_LAUNCH((lds_count_kernel<true, 8, true>), 8); else KATOME_LC_LAUNCH((lds_count_kernel<true, 8, false>), 8); }
            else       { if (!rc) KATOME_LC_LAUNCH((lds_count_kernel<false, 13, false>), 13); else if (even) KATOME_LC_LAUNCH((lds_count_kernel<true, 13, true>), 13); else KATOME_LC_LAUNCH((lds_count_kernel<true, 13, false>), 13); }
        } else if (nw == 3) {
            if (small) KATOME_LC_LAUNCH((lds_count_wide_kernel<false, 8, 3, false>), 8); else KATOME_LC_LAUNCH((lds_count_wide_kernel<false, 13, 3, false>), 13);
        } else {
            if (small) { if (!rc) KATOME_LC_LAUNCH((lds_count_wide_kernel<false, 8, 2, false>), 8); else if (even) KATOME_LC_LAUNCH((lds_count_wide_kernel<true, 8, 2, true>), 8); else KATOME_LC_LAUNCH((lds_count_wide_kernel<true, 8, 2, false>), 8); }
            else       { if (!rc) KATOME_LC_LAUNCH((lds_count_wide_kernel<false, 13, 2, false>), 13); else if (even) KATOME_LC_LAUNCH((lds_count_wide_kernel<true, 13, 2, true>), 13); else KATOME_LC_LAUNCH((lds_count_wide_kernel<true, 13, 2, false>), 13); }
        }
#undef KATOME_LC_LAUNCH
        KCHECK_HIP(hipGetLastError());
        KCHECK_HIP(hipMemcpyAsync(h, aux.p, 24, hipMemcpyDeviceToHost, stream));
        KCHECK_HIP(hipStreamSynchronize(stream));
        return KATOME_OK;
    };
    // Two-word keys: whole keys in the slots (lds_count_full_kernel) when a group's distinct keys fit that smaller table.  How many
    // they are is known only by counting: the first 256 groups are counted for it (1/256 of the records, nothing written: out_cap 0).
    // KATOME_LC_FULL=0: never, =1: without asking (tests)
    if (nw == 2 && !split && gbits == 16) {
        static const int full_mode = getenv("KATOME_LC_FULL") ? atoi(getenv("KATOME_LC_FULL")) : -1;
        const bool even = (k & 1) == 0;
        auto count_full = [&](u32 groups, u64 cap, int per) -> int {
            KCHECK_HIP(hipMemsetAsync(aux.p, 0, 64, stream));
#define KATOME_LF_LAUNCH(RCV, EVENV, PERV)                                                                                              \
            do {                                                                                                                      \
                const size_t lds = (size_t)LfTable<PERV>::SLOTS * 20;                                                                 \
                KCHECK_HIP(hipFuncSetAttribute((const void*)lds_count_full_kernel<RCV, EVENV, PERV>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
                KernelScope ks(K_LDS_COUNT, stream, n);                                                                               \
                hipLaunchKernelGGL((lds_count_full_kernel<RCV, EVENV, PERV>), dim3(256u), dim3(LC_THREADS), lds, stream, ko, wo, index.as<u64>(), groups, k, \
                                   min_weight, edge_key.as<u64>(), edge_weight.as<u32>(), cap, cursor, distinct, err, std::min<u32>(lc_probe_limit(), LfTable<PERV>::SLOTS)); \
            } while (0)
#define KATOME_LF_PICK(PERV)                                                                                                            \
            do { if (!rc) KATOME_LF_LAUNCH(false, false, PERV); else if (even) KATOME_LF_LAUNCH(true, true, PERV); else KATOME_LF_LAUNCH(true, false, PERV); } while (0)
            if (per == 4) KATOME_LF_PICK(4); else KATOME_LF_PICK(7);
#undef KATOME_LF_PICK
#undef KATOME_LF_LAUNCH
            KCHECK_HIP(hipGetLastError());
            KCHECK_HIP(hipMemcpyAsync(h, aux.p, 24, hipMemcpyDeviceToHost, stream));
            KCHECK_HIP(hipStreamSynchronize(stream));
            return KATOME_OK;
        };
        const u32 all = 1u << gbits, sample = 256u;
        static const int full_per = getenv("KATOME_LC_FULL_PER") ? atoi(getenv("KATOME_LC_FULL_PER")) : 0;      // (4 or 7: tests)
        bool take = full_mode == 1;
        int per = full_per == 4 ? 4 : 7;
        if (full_mode < 0 && avg > 0 && avg <= 8ull * LfTable<7>::FILL) {        // (eight records to a key: more repetition than that is not planned with)
            KCHECK(count_full(sample, 0, 7));
            const u64 per_group = h[1] / sample;
            take = (uint32_t)h[2] == 0 && per_group <= LfTable<7>::FILL;
            // (the smaller table only where it stays a third full: at 0.55 -- C3's big tiles -- its longer probe sequences cost more than
            // its shorter clear and read-out save: 16.2 against 15.5 ms; at 0.35 -- k = 63's k-mers -- 4.5 against 4.9)
            if (!full_per) per = per_group <= LfTable<4>::SLOTS / 20 * 7 ? 4 : 7;
        }
        if (take) {
            KCHECK(count_full(all, out_cap, per));
            if (getenv("KATOME_LC_TRACE")) fprintf(stderr, "[lds count] whole keys in the slots (%d per thread): code %u\n", per, (unsigned)h[2]);
            if ((uint32_t)h[2] == 3 && per == 4) {               // (a group of more distinct keys than the sample promised: the larger table)
                KCHECK(count_full(all, out_cap, 7));
                if (getenv("KATOME_LC_TRACE")) fprintf(stderr, "[lds count] whole keys in the slots (7 per thread): code %u\n", (unsigned)h[2]);
            }
            if ((uint32_t)h[2] == 0) { *n_edges = h[0]; *n_distinct = h[1]; return KATOME_OK; }
        }
    }
    // ... and three-word keys (lds_count_full3_kernel), chosen the same way
    if (nw == 3 && !split && gbits == 16) {
        static const int full_mode = getenv("KATOME_LC_FULL") ? atoi(getenv("KATOME_LC_FULL")) : -1;
        static const int full_per = getenv("KATOME_LC_FULL_PER") ? atoi(getenv("KATOME_LC_FULL_PER")) : 0;      // (tests: 4 -> the small table, 7 -> the large one)
        auto count_full3 = [&](u32 groups, u64 cap, int per) -> int {
            KCHECK_HIP(hipMemsetAsync(aux.p, 0, 64, stream));
#define KATOME_LF3_LAUNCH(PERV)                                                                                                         \
            do {                                                                                                                      \
                const size_t lds = (size_t)Lf3Table<PERV>::SLOTS * 28;                                                                \
                KCHECK_HIP(hipFuncSetAttribute((const void*)lds_count_full3_kernel<PERV>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
                KernelScope ks(K_LDS_COUNT, stream, n);                                                                               \
                hipLaunchKernelGGL((lds_count_full3_kernel<PERV>), dim3(256u), dim3(LC_THREADS), lds, stream, ko, wo, index.as<u64>(), groups,  \
                                   edge_key.as<u64>(), edge_weight.as<u32>(), cap, cursor, distinct, err, std::min<u32>(lc_probe_limit(), Lf3Table<PERV>::SLOTS)); \
            } while (0)
            if (per == 3) KATOME_LF3_LAUNCH(3); else KATOME_LF3_LAUNCH(5);
#undef KATOME_LF3_LAUNCH
            KCHECK_HIP(hipGetLastError());
            KCHECK_HIP(hipMemcpyAsync(h, aux.p, 24, hipMemcpyDeviceToHost, stream));
            KCHECK_HIP(hipStreamSynchronize(stream));
            return KATOME_OK;
        };
        const u32 all = 1u << gbits, sample = 256u;
        bool take = full_mode == 1;
        int per = full_per == 4 ? 3 : 5;
        if (full_mode < 0 && avg > 0 && avg <= 8ull * Lf3Table<5>::FILL) {
            KCHECK(count_full3(sample, 0, 5));
            const u64 per_group = h[1] / sample;
            take = (uint32_t)h[2] == 0 && per_group <= Lf3Table<5>::FILL;
            if (!full_per) per = per_group <= Lf3Table<3>::SLOTS / 20 * 7 ? 3 : 5;
        }
        if (take) {
            KCHECK(count_full3(all, out_cap, per));
            if (getenv("KATOME_LC_TRACE")) fprintf(stderr, "[lds count] whole three-word keys in the slots (%d per thread): code %u\n", per, (unsigned)h[2]);
            if ((uint32_t)h[2] == 3 && per == 3) {
                KCHECK(count_full3(all, out_cap, 5));
                if (getenv("KATOME_LC_TRACE")) fprintf(stderr, "[lds count] whole three-word keys in the slots (5 per thread): code %u\n", (unsigned)h[2]);
            }
            if ((uint32_t)h[2] == 0) { *n_edges = h[0]; *n_distinct = h[1]; return KATOME_OK; }
        }
    }
    const u32 R_try = (u32)std::max<u64>(1, (u64)std::ceil((double)avg * lc_optimism() / fill));
    // One-word k-mers whose groups would take several visits: 8-byte slots, one visit (lds_count_packed_kernel), sized on the guess that
    // 56 % of a group's records are distinct (C3: 0.56; more and the table fills: err 3, then as before).  KATOME_LC_PACKED=0: never
    static const int packed_mode = getenv("KATOME_LC_PACKED") ? atoi(getenv("KATOME_LC_PACKED")) : 1;      // (2: whenever the keys allow -- tests)
    if (nw == 1 && !split && !unit && gbits == 16 && (R_try > 1 || packed_mode == 2) && !(rc && (k & 1) == 0)) {
        const u32 R_p = (u32)std::max<u64>(1, (u64)std::ceil((double)avg * 0.56 / (LP_SLOTS * 0.66)));
        if (packed_mode == 2 || (packed_mode && R_p < R_try)) {
            KCHECK_HIP(hipMemsetAsync(aux.p, 0, 64, stream));
            const size_t lds = (size_t)LP_SLOTS * 8;
#define KATOME_LP_LAUNCH(RCV)                                                                                                           \
            do {                                                                                                                      \
                KCHECK_HIP(hipFuncSetAttribute((const void*)lds_count_packed_kernel<RCV>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
                KernelScope ks(K_LDS_COUNT, stream, n);                                                                               \
                hipLaunchKernelGGL((lds_count_packed_kernel<RCV>), dim3(256u), dim3(LC_THREADS), lds, stream, ko, wo, index.as<u64>(), R_p, k,  \
                                   min_weight, edge_key.as<u64>(), edge_weight.as<u32>(), out_cap, cursor, distinct, err, std::min<u32>(lc_probe_limit(), LP_SLOTS)); \
            } while (0)
            if (!rc) KATOME_LP_LAUNCH(false); else KATOME_LP_LAUNCH(true);
#undef KATOME_LP_LAUNCH
            KCHECK_HIP(hipGetLastError());
            KCHECK_HIP(hipMemcpyAsync(h, aux.p, 24, hipMemcpyDeviceToHost, stream));
            KCHECK_HIP(hipStreamSynchronize(stream));
            if (getenv("KATOME_LC_TRACE")) fprintf(stderr, "[lds count] 8-byte slots, %u visit(s) per record: code %u\n", R_p, (unsigned)h[2]);
            if ((uint32_t)h[2] == 0) { *n_edges = h[0]; *n_distinct = h[1]; return KATOME_OK; }
            if (getenv("KATOME_LC_TRACE")) fprintf(stderr, "[lds count] 8-byte slots: %s; counting with the 12-byte slots\n", (uint32_t)h[2] == 5 ? "a count beyond 16 bits" : "a table filled");
        }
    }
    // First with fewer sub-rounds than would hold a group of DISTINCT records: the k-mers of reads repeat (C3: 1.8 records per
    // k-mer at this level), so the table is half empty at the guaranteed number.  An attempt that fills its table gives up after
    // lc_probe_limit() = 128 probes (err 3, nothing it wrote is used) and the guaranteed number runs.
    if (R_try < R) { KCHECK(count(R_try, lc_probe_limit())); if ((uint32_t)h[2] == 3) { lc_trace("packed key", R_try, R); KCHECK(count(R, ~0u)); } }
    else KCHECK(count(R, ~0u));
    if ((uint32_t)h[2] == 4) return KATOME_E_UNSUPPORTED;          // (a group too large for the representative's 20 bits: the caller counts in the table)
    if ((uint32_t)h[2]) { set_error("counting in LDS: a sub-round did not fit its table (code %u)", (unsigned)h[2]); return KATOME_E_DEVICE; }
    *n_edges = h[0]; *n_distinct = h[1];
    if (split) {
        uint64_t hb[2 * KATOME_MAX_RANKS + 2];
        KCHECK_HIP(hipMemcpyAsync(hb, owners.p, sizeof hb, hipMemcpyDeviceToHost, stream));
        KCHECK_HIP(hipStreamSynchronize(stream));
        uint64_t total = 0;
        for (uint32_t p = 0; p < n_owners; ++p) {
            split->base[p] = hb[KATOME_MAX_RANKS + 1 + p];
            split->count[p] = hb[p] - split->base[p];
            total += split->count[p];
        }
        *n_edges = total;             // (the records: scattered over the owners' stretches of edge_key / edge_weight)
    }
    return KATOME_OK;
}

int table_emit_edges(Table& t, uint32_t k, bool rc, uint32_t min_weight, DevBuf& keys, DevBuf& weights, uint64_t* n_edges,
                     hipStream_t stream, DevBuf* seqs) {
    uint64_t occ = 0;
    KCHECK(table_occupied(t, &occ, stream));
    const uint64_t upper = occ * (rc ? 2 : 1);
    KCHECK(keys.alloc((upper + 1) * 8 * t.nw, stream));
    const u64* seen = nullptr; u64* out_seq = nullptr;
    // first-seen order: the weights travel with the sequence numbers ([upper][2] u64 in `seqs`, one gather later); `weights` stays empty
    if (seqs && t.track_seen) { KCHECK(seqs->alloc((upper + 1) * 16, stream)); seen = t.seen.as<u64>(); out_seq = seqs->as<u64>(); }
    else KCHECK(weights.alloc((upper + 1) * 4, stream));
    DevBuf cursor(stream);
    KCHECK(cursor.alloc(8));
    KCHECK_HIP(hipMemsetAsync(cursor.p, 0, 8, stream));
    const int items = (seen || t.nw > 1) ? 4 : 8;          // (LDS per workgroup: 24-64 KiB)
    dim3 grid(grid_for(t.cap, BLOCK * items, 256u * 16u)), block(BLOCK);
    const size_t lds = (size_t)BLOCK * items * 2 * (8 * t.nw + (seen ? 16 : 4));
#define KATOME_EMIT(NWV, RCV, ITEMS)                                                                                                      \
    do {                                                                                                                                  \
        if (lds > (64u << 10)) KCHECK_HIP(hipFuncSetAttribute((const void*)emit_edges_kernel<NWV, RCV, ITEMS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
        hipLaunchKernelGGL((emit_edges_kernel<NWV, RCV, ITEMS>), grid, block, lds, stream, t.slots.as<SlotOf<NWV>::type>(), t.cap, k, min_weight,      \
                           keys.as<u64>(), weights.as<u32>(), cursor.as<u64>(), seen, out_seq);                                          \
    } while (0)
    if (t.nw == 1) {
        if (seen) { if (rc) KATOME_EMIT(1, true, 4); else KATOME_EMIT(1, false, 4); }
        else      { if (rc) KATOME_EMIT(1, true, 8); else KATOME_EMIT(1, false, 8); }
    } else {
        if (rc) KATOME_EMIT(2, true, 4); else KATOME_EMIT(2, false, 4);
    }
#undef KATOME_EMIT
    KCHECK_HIP(hipGetLastError());
    KCHECK_HIP(hipMemcpyAsync(n_edges, cursor.p, 8, hipMemcpyDeviceToHost, stream));
    KCHECK_HIP(hipStreamSynchronize(stream));
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
#endif
