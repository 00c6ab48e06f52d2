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
#include "entry_cut.h"
#include "lds_plan.h"
#include "seq_pair.h"
#include "slot_bits.h"

namespace katome {

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

// The same counts and no records: the first partition pass makes its tiles from the list itself (radix.hip, ListSource), so all that
// is needed beforehand is counts[tile][digit] of the tiles it will cut.  A workgroup divides its tile's first record index by span
// once; inside the tile the entry of record q (counted from that entry's first record) is mulhi(q, inv), inv = 2^32 / span + 1, which
// is q / span while q * span < 2^32.  REP: the digit is bits 2k - 16 .. 2k - 9 of the representative orientation -- the sub-window's own
// when its middle base says so, else the complement of its bases 4..7 from the right, in reverse: no reverse complement is built.
// ENTRY (entry_cut.h): a thread takes a list entry instead of a record -- one load of it, one reverse complement where the hash wants
// the canonical record, and for REP no cut at all: with s = 2 * stride * (span - 1 - o), window o's own digit is the tile's bits
// s + 2k - 16 .. s + 2k - 9, the other one comes from its bits s + 8 .. s + 15 and bit s + k chooses, all at offsets every lane shares.
// Only the records inside the tile are counted: its first and last entry straddle its ends.
template <int NWT, int NWK, bool RC, bool REP = false, bool ENTRY = true>
__global__ __launch_bounds__(BLOCK) void list_digit_counts_kernel(const u64* __restrict__ tiles, u64 n_tiles, u32 k, u32 span, u32 stride, u32 inv, u32 tile_keys,
                                                                   u32* __restrict__ digit_counts) {
    static_assert(BLOCK == 256, "one thread per digit");
    __shared__ u32 h[256];
    const u64 n = n_tiles * span, n_out_tiles = (n + tile_keys - 1) / tile_keys;
    for (u64 ot = blockIdx.x; ot < n_out_tiles; ot += gridDim.x) {
        h[threadIdx.x] = 0;
        __syncthreads();
        const u64 p0 = ot * tile_keys, t0 = p0 / span;
        const u32 o0 = (u32)(p0 - t0 * span), cnt = (u32)(n - p0 < (u64)tile_keys ? n - p0 : (u64)tile_keys);
        if constexpr (ENTRY) {
            const u32 n_ent = (o0 + cnt + span - 1) / span;
            for (u32 e = threadIdx.x; e < n_ent; e += BLOCK) {
                Key<NWT> tile;
#pragma unroll
                for (int w = 0; w < NWT; ++w) tile.w[w] = tiles[(t0 + e) * NWT + w];
                const u32 first = e * span - o0;          // (index of the entry's record 0 in the tile; wraps for records before it)
                if constexpr (REP) {
                    for (u32 o = 0; o < span; ++o) {
                        const u32 s = 2 * stride * (span - 1 - o);
                        const u32 own = key_digit(tile, s + 2 * k - 16, 8);
                        u32 v = ~key_digit(tile, s + 8, 8) & 255u;
                        v = ((v & 0x0Fu) << 4) | (v >> 4);
                        v = ((v & 0x33u) << 2) | ((v >> 2) & 0x33u);
                        const u32 d = RC && key_digit(tile, s + k, 1) ? v : own;
                        if (first + o < cnt) atomicAdd(&h[d], 1u);
                    }
                } else {
                    const EntryCut<NWT, NWK, RC, false> cut(tile, k, span, stride);
                    for (u32 o = 0; o < span; ++o)
                        if (first + o < cnt) atomicAdd(&h[(u32)(hash_key(cut.record(o)) >> 48) & 255u], 1u);
                }
            }
        } else
        for (u32 i = threadIdx.x; i < cnt; i += BLOCK) {
            const u32 q = o0 + i, tr = __umulhi(q, inv), o = q - tr * span;
            const u64 t = t0 + tr;
            Key<NWT> tile;
#pragma unroll
            for (int w = 0; w < NWT; ++w) tile.w[w] = tiles[t * NWT + w];
            const Key<NWK> x = sub_window<NWT, NWK>(tile, k, span, stride, o);
            u32 d;
            if constexpr (REP) {
                const u32 own = (u32)(x.w[0] >> (2 * k - 16)) & 255u;
                u32 v = ~(u32)(x.w[0] >> 8) & 255u;                          // the reverse complement's: pairs of bits in reverse
                v = ((v & 0x0Fu) << 4) | (v >> 4);
                v = ((v & 0x33u) << 2) | ((v >> 2) & 0x33u);
                d = RC && ((x.w[0] >> k) & 1ull) ? v : own;
            } else d = (u32)(hash_key(level_orientation<NWK, RC, false>(x, k)) >> 48) & 255u;
            atomicAdd(&h[d], 1u);
        }
        __syncthreads();
        digit_counts[ot * 256 + threadIdx.x] = h[threadIdx.x];
        __syncthreads();
    }
}

// ---- first-seen builds: the last level counted by sorting ------------------------------------------------------------------------
// A k-mer record of such a build has two sequence numbers: the first insertion of the stored (canonical) k-mer and the first
// insertion of its reverse complement (pt_graph.rs:282-308 adds a read's forward windows, then those of its reverse complement).
// Both fall into the range of ONE read -- the first read that holds the k-mer on either strand --, so with reads of a fixed length
// (S sequence numbers each) the pair packs into one word: read << 32 | offset of the one << 16 | offset of the other.  The records
// (k-mer, packed pair) + count go through the same two hash passes as the headline build's (the k-mer's words are hashed, the
// tag rides along) and are counted in LDS, where the two numbers are lowered by 64-bit atomicMin's of read << 16 | offset.

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
// keep_rest_kernel<NW, true> for a batch of variable-length reads: record g's numbers are var_seq_pair's (seq_pair.h: the function the
// table's insert uses) and leave as a delta tag (seen_tag.h).  One thread per record finds its read by the same binary search over
// rec_prefix that extract_general_kernel ran to cut the record (a batch's prefix stays in L2), the KR_ITEMS searches of a thread in
// step; the host has checked that every read of the batch packs (table_max_windows), so no record is refused here.
template <int NW, bool RC>
__global__ __launch_bounds__(BLOCK) void keep_var_kernel(const u64* __restrict__ rec, u64 n, const u64* __restrict__ win_prefix, const u64* __restrict__ rec_prefix,
                                                          u64 n_reads, u32 mode, u32 span, u64 seq_base, u64* __restrict__ out, unsigned long long* cursor) {
    constexpr int WORDS = NW + 1;
    constexpr u32 TILE = BLOCK * KR_ITEMS;
    __shared__ u32 wtot[KR_ITEMS][BLOCK / 64];       // as keep_rest_kernel's
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
        // var_seq_pair's search for the thread's KR_ITEMS records, step by step side by side: a step's loads are in flight together
        // (one record after the other, the kernel waited for KR_ITEMS x log2(reads) dependent loads in a row)
        u64 lo[KR_ITEMS], hi[KR_ITEMS];
#pragma unroll
        for (int j = 0; j < KR_ITEMS; ++j) { lo[j] = 0; hi[j] = key_valid(key[j]) ? n_reads : 1; }
        for (bool more = true; more;) {
            more = false;
            u64 at_mid[KR_ITEMS];
#pragma unroll
            for (int j = 0; j < KR_ITEMS; ++j) at_mid[j] = rec_prefix[(lo[j] + hi[j]) >> 1];       // (a finished search reads [lo] once more: in bounds)
#pragma unroll
            for (int j = 0; j < KR_ITEMS; ++j) {
                if (hi[j] - lo[j] <= 1) continue;
                const u64 mid = (lo[j] + hi[j]) >> 1;
                if (at_mid[j] <= t0 + (u64)j * BLOCK + tid) lo[j] = mid; else hi[j] = mid;
                more = more || hi[j] - lo[j] > 1;
            }
        }
#pragma unroll
        for (int j = 0; j < KR_ITEMS; ++j) {
            if (!key_valid(key[j])) continue;
            const u64 i = t0 + (u64)j * BLOCK + tid;
            const u64 at = (base_sh + wtot[j][wave] + before[j]) * WORDS;
            const bool flipped = (key[j].w[0] & RC_MARK) != 0;
            key[j].w[0] &= ~RC_MARK;
#pragma unroll
            for (int q = 0; q < NW; ++q) out[at + q] = key[j].w[q];
            u64 P, Q;
            var_pair_in_read(win_prefix, rec_prefix, lo[j], mode, span, seq_base, i, P, Q);
            if (!RC) Q = P;                          // (one strand: one number)
            out[at + NW] = flipped ? delta_pack(Q, P) : delta_pack(P, Q);
        }
        __syncthreads();
    }
}
// the most windows any read of a batch has (prefix[r + 1] - prefix[r])
__global__ __launch_bounds__(BLOCK) void max_windows_kernel(const u64* __restrict__ win_prefix, u64 n_reads, unsigned long long* out) {
    u64 m = 0;
    for (u64 r = (u64)blockIdx.x * BLOCK + threadIdx.x; r < n_reads; r += (u64)gridDim.x * BLOCK) {
        const u64 w = win_prefix[r + 1] - win_prefix[r];
        m = w > m ? w : m;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const u64 v = __shfl_xor(m, o, 64); m = v > m ? v : m; }
    if ((threadIdx.x & 63) == 0 && m) atomicMax(out, (unsigned long long)m);
}
// ... and back into (key, {first insertion of the stored orientation, of its reverse complement}) for the k-mer table
// (DELTA: the delta tag of seen_tag.h -- the two numbers themselves)
template <int NW, bool DELTA>
__global__ __launch_bounds__(BLOCK) void tagged_to_pairs_kernel(const u64* __restrict__ tagged, u64 n, u64 seq_per_read, u64* __restrict__ keys,
                                                                 u64* __restrict__ pairs) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK) {
#pragma unroll
        for (int q = 0; q < NW; ++q) keys[i * NW + q] = tagged[i * (NW + 1) + q];
        const u64 tag = tagged[i * (NW + 1) + NW], base = (tag >> 32) * seq_per_read;
        pairs[2 * i] = DELTA ? delta_p(tag) : base + ((tag >> 16) & 0xFFFFull); pairs[2 * i + 1] = DELTA ? delta_q(tag) : base + (tag & 0xFFFFull);
    }
}

// every distinct tile of the last level -> its `span` k-mers as records of NWK + 1 words + the tile's count (tiles_to_records_kernel's
// shape: 2048 slots per trip).  read = fwd / seq_per_read as a multiplication by `magic` = floor(2^64 / seq_per_read) + 1: exact for
// numbers below 2^64 / seq_per_read, which 2^32 reads of < 2^16 numbers each stay under.
// DELTA (reads of varying length): the tile's pair packs as it is (seen_tag.h) -- lread holds P, loff Q - P + DELTA_BIAS --, no division.
template <int NWT, int NWK, bool RC, bool DELTA>
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
            if (DELTA) {
                const u64 P = fwd[j], Q = RC ? rev[j] : fwd[j], gap = Q >= P ? Q - P : P - Q;
                // (a sub-window's numbers are P + o and Q + span - 1 - o: the gap grows by less than span)
                if (P + span >= DELTA_P_LIMIT || Q + span >= DELTA_P_LIMIT || gap + span >= DELTA_BIAS) *err = 5;      // (does not pack)
                lread[at] = P; loff[2 * at] = (u32)(Q - P + DELTA_BIAS); loff[2 * at + 1] = 0u;
            } else {
            const u64 read = __umul64hi(fwd[j], magic);
            const u64 a = fwd[j] - read * seq_per_read, b = RC ? rev[j] - read * seq_per_read : 0;        // (no reverse complements: one number)
            if (read >> 32 || a >= seq_per_read || a + span > 0xFFFFu || (RC && (rev[j] < read * seq_per_read || b > 0xFFFFu))) *err = 5;   // (does not pack)
            lread[at] = read; loff[2 * at] = (u32)a; loff[2 * at + 1] = (u32)b;
            }
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
            if (DELTA) {
                u64 Ps, Qs;
                delta_sub(lread[t], lread[t] + loff[2 * t] - DELTA_BIAS, o, span, 1, Ps, Qs);
                if (!RC) Qs = Ps;
                out[rec + NWK] = flipped ? delta_pack(Qs, Ps) : delta_pack(Ps, Qs);
            } else
            out[rec + NWK] = seen_pack(lread[t], flipped ? b : a, flipped ? a : b);
            out_w[base + p] = lcnt[t];
        }
        __syncthreads();
    }
}

// a list of distinct tiles with their tags and counts (lds_count_seen_kernel, LIST) -> the tagged records of the next level: record p is
// sub-window p % n_sub of tile p / n_sub; its numbers are the tile's plus the sub-window's place in it (expand_tiles_kernel's rule)
// (digit_counts: written tile by tile of the partition pass that follows -- tile_keys records per trip --, that pass's digit counted per
// tile on the way, as list_to_records_hist_kernel does; without: a plain grid-stride walk)
// DELTA: list and records carry the delta tag (seen_tag.h)
template <int NWT, int NWK, bool RC, bool DELTA>
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
        if (DELTA) {
            u64 Ps, Qs;
            delta_sub(delta_p(tag), delta_q(tag), o, n_sub, stride, Ps, Qs);
            if (!RC) Qs = Ps;
            out[p * (NWK + 1) + NWK] = flipped ? delta_pack(Qs, Ps) : delta_pack(Ps, Qs);
        } else
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

// list_to_records_kernel over a whole list, into buffers that hold n_tiles * span records
static int launch_list_to_records(const uint64_t* d_tiles, const uint32_t* d_counts, uint64_t n_tiles, uint32_t nwt, uint32_t nwk, uint32_t k, uint32_t span,
                                  uint32_t stride, bool rc, bool rep, u64* d_keys, u32* d_weights, hipStream_t stream) {
    const dim3 grid(grid_for(n_tiles * span, BLOCK, 256u * 32u)), block(BLOCK);
    KernelScope ks(K_RECORDS, stream, n_tiles);
#define KATOME_LR(NWT, NWK, REP) with_bool(rc, [&](auto rcv) { hipLaunchKernelGGL((list_to_records_kernel<NWT, NWK, decltype(rcv)::value, REP>), grid, block, 0, stream, d_tiles, d_counts, n_tiles, k, span, stride, d_keys, d_weights); return 0; })
    if (rep) { if (nwt == 2) KATOME_LR(2, 1, true); else KATOME_LR(1, 1, true); }
    else if (nwt == 3 && nwk == 3) KATOME_LR(3, 3, false);
    else if (nwt == 3 && nwk == 2) KATOME_LR(3, 2, false);
    else if (nwt == 2 && nwk == 2) KATOME_LR(2, 2, false);
    else if (nwt == 2 && nwk == 1) KATOME_LR(2, 1, false);
    else if (nwt == 1 && nwk == 1) KATOME_LR(1, 1, false);
    else { set_error("records of a tile list: tiles of %u words into windows of %u", nwt, nwk); return KATOME_E_UNSUPPORTED; }
#undef KATOME_LR
    KCHECK_HIP(hipGetLastError());
    return KATOME_OK;
}

bool fused_records_takes(uint32_t nwt, uint32_t nwk, bool rep, uint32_t span) {
    if (span < 2 || span > 64) return false;          // (the kernels' reciprocal of span: 2^32 / span + 1 in 32 bits)
    return rep ? (nwk == 1 && nwt <= 2) : (nwt == 2 && nwk == 2);
}

// the records of a source that somebody wants before its first pass: written out as they always were, in this one place
int table_materialise_records(RecordSource& s) {
    if (!s.pending) return KATOME_OK;
    KCHECK(s.keys->alloc(s.key_bytes, s.stream));
    KCHECK(s.weights->alloc(s.weight_bytes, s.stream));
    if (getenv("KATOME_LC_TRACE")) fprintf(stderr, "[records] %llu records written after all: wanted before their first pass\n", (unsigned long long)s.n_records());
    KCHECK(launch_list_to_records(s.tiles, s.counts, s.n_tiles, (uint32_t)key_words_for_k(s.tile_bases), (uint32_t)key_words_for_k(s.k), s.k, s.span, s.stride,
                                  s.rc, s.rep, s.keys->as<u64>(), s.weights->as<u32>(), s.stream));
    s.pending = false; s.tiles = nullptr; s.counts = nullptr;
    s.own_tiles.release(); s.own_counts.release();
    return KATOME_OK;
}

// the (sub-window, count) records of a compact list of distinct tiles (list_to_records_kernel); extra_room: see below
int table_list_to_records(const uint64_t* d_tiles, const uint32_t* d_counts, uint64_t n_tiles, uint32_t tile_bases, uint32_t k, uint32_t span, uint32_t stride, bool rc,
                          DevBuf& keys, DevBuf& weights, uint64_t* n_records, hipStream_t stream, uint64_t extra_room, DevBuf* first_counts, bool rep,
                          RecordSource* src) {
    const uint32_t nwt = (uint32_t)key_words_for_k(tile_bases), nwk = (uint32_t)key_words_for_k(k);
    if (rep && (nwk != 1 || nwt > 2 || k < 9 || (rc && !(k & 1)))) { set_error("records in their representative orientation: one-word k-mers, k >= 9, odd k or one strand"); return KATOME_E_ARG; }
    *n_records = n_tiles * span;
    // (first_counts: the caller sorts exactly these records next -- nothing appended -- and wants the first pass's digit counts per tile;
    // KATOME_FUSED_HIST=0: the pass counts them itself)
    const bool counted = first_counts && fused_hist_on() && !extra_room && ((nwt == 3 && nwk >= 2) || (nwt == 2 && nwk <= 2) || (nwt == 1 && nwk == 1));
    // (src: ... and can do without the records until its first pass has made them -- KATOME_FUSED_RECORDS=0: never)
    const bool fused = src && counted && *n_records && fused_records_on() && fused_records_takes(nwt, nwk, rep, span);
    if (src && getenv("KATOME_LC_TRACE"))
        fprintf(stderr, "[records] %llu records of %u words off a list of %llu: %s\n", (unsigned long long)*n_records, nwk, (unsigned long long)n_tiles,
                fused ? "made by their first partition pass" : !fused_records_on() ? "written (KATOME_FUSED_RECORDS=0)"
                : extra_room ? "written (left-over windows go behind them)" : !counted ? "written (no counts for the first pass)"
                : !*n_records ? "written (none)" : "written (this shape's first pass reads records)");
    const uint32_t tile_keys = dev_sort_tile_keys(nwk);
    const uint64_t n_out_tiles = (*n_records + tile_keys - 1) / tile_keys;
    const dim3 hgrid(grid_for(n_out_tiles, 1, 256u * 32u)), block(BLOCK);
    if (fused) {
        keys.release(); weights.release();
        KCHECK(first_counts->alloc(n_out_tiles * 256 * 4 + 16, stream));
        const uint32_t inv = (uint32_t)((1ull << 32) / span) + 1;
        if (getenv("KATOME_LC_TRACE")) fprintf(stderr, "[entry_cut] %s\n", entry_cut_on() ? "once per list entry" : "once per record (KATOME_ENTRY_CUT=0)");
        KernelScope ks(K_RECORDS, stream, n_tiles);
#define KATOME_LDC(NWT, NWK, REP) with_bool(rc, [&](auto rcv) { return with_bool(entry_cut_on(), [&](auto cutv) { hipLaunchKernelGGL((list_digit_counts_kernel<NWT, NWK, decltype(rcv)::value, REP, decltype(cutv)::value>), hgrid, block, 0, stream, d_tiles, n_tiles, k, span, stride, inv, tile_keys, first_counts->as<u32>()); return 0; }); })
        if (rep) { if (nwt == 2) KATOME_LDC(2, 1, true); else KATOME_LDC(1, 1, true); }
        else KATOME_LDC(2, 2, false);
#undef KATOME_LDC
        KCHECK_HIP(hipGetLastError());
        src->tiles = d_tiles; src->counts = d_counts; src->n_tiles = n_tiles;
        src->tile_bases = tile_bases; src->k = k; src->span = span; src->stride = stride; src->rc = rc; src->rep = rep;
        src->keys = &keys; src->weights = &weights; src->key_bytes = (*n_records + 1) * 8 * nwk; src->weight_bytes = (*n_records + 1) * 4;
        src->stream = stream; src->pending = true;
        return KATOME_OK;
    }
    KCHECK(keys.alloc((*n_records + extra_room + 1) * 8 * nwk, stream));
    KCHECK(weights.alloc((*n_records + extra_room + 1) * 4, stream));
    if (*n_records == 0) return KATOME_OK;
    if (counted) {
        KCHECK(first_counts->alloc(n_out_tiles * 256 * 4 + 16, stream));
        KernelScope ks(K_RECORDS, stream, n_tiles);
#define KATOME_LRH(NWT, NWK, REP) with_bool(rc, [&](auto rcv) { hipLaunchKernelGGL((list_to_records_hist_kernel<NWT, NWK, decltype(rcv)::value, REP>), hgrid, block, 0, stream, d_tiles, d_counts, n_tiles, k, span, stride, keys.as<u64>(), weights.as<u32>(), tile_keys, first_counts->as<u32>()); return 0; })
        if (rep) { if (nwt == 2) KATOME_LRH(2, 1, true); else KATOME_LRH(1, 1, true); }      // (the ordered count's records: dev_key_order's first digit)
        else if (nwt == 3 && nwk == 3) KATOME_LRH(3, 3, false);
        else if (nwt == 3 && nwk == 2) KATOME_LRH(3, 2, false);
        else if (nwt == 2 && nwk == 2) KATOME_LRH(2, 2, false);
        else if (nwt == 2 && nwk == 1) KATOME_LRH(2, 1, false);
        else KATOME_LRH(1, 1, false);
#undef KATOME_LRH
        KCHECK_HIP(hipGetLastError());
        return KATOME_OK;
    }
    if (first_counts) first_counts->release();
    return launch_list_to_records(d_tiles, d_counts, n_tiles, nwt, nwk, k, span, stride, rc, rep, keys.as<u64>(), weights.as<u32>(), stream);
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
#define KATOME_TR(NWT, NWK) with_bool(rc, [&](auto rcv) { hipLaunchKernelGGL((tiles_to_records_kernel<NWT, NWK, decltype(rcv)::value>), grid, block, 0, stream, tiles.slots.as<SlotOf<NWT>::type>(), tiles.cap, k, span, 1u, keys.as<u64>(), weights.as<u32>(), cursor.as<u64>()); return 0; })
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
int table_tagged_to_pairs(const uint64_t* d_tagged, uint64_t n, uint32_t nw, SeenTag tag, uint64_t* d_keys, uint64_t* d_pairs, hipStream_t stream) {
    if (n == 0) return KATOME_OK;
    const dim3 grid(grid_for(n, BLOCK, 256u * 16u)), block(BLOCK);
    with_bool(tag.delta, [&](auto dv) {
        constexpr bool DELTA = decltype(dv)::value;
        if (nw == 1) hipLaunchKernelGGL((tagged_to_pairs_kernel<1, DELTA>), grid, block, 0, stream, d_tagged, n, tag.seq_per_read, d_keys, d_pairs);
        else         hipLaunchKernelGGL((tagged_to_pairs_kernel<2, DELTA>), grid, block, 0, stream, d_tagged, n, tag.seq_per_read, d_keys, d_pairs);
        return 0;
    });
    KCHECK_HIP(hipGetLastError());
    return KATOME_OK;
}

int table_keep_var_tagged(const uint64_t* d_rec, uint64_t n, uint32_t nw, bool rc, const uint64_t* d_win_prefix, const uint64_t* d_rec_prefix, uint64_t n_reads,
                          uint32_t mode, uint32_t span, uint64_t seq_base, uint64_t* d_out, uint64_t* d_cursor, hipStream_t stream) {
    if (n == 0) return KATOME_OK;
    if (nw > 2 || !n_reads || !d_win_prefix || !d_rec_prefix) { set_error("tagged records: keys of one or two words, cut from a batch of reads"); return KATOME_E_UNSUPPORTED; }
    const dim3 grid(grid_for(n, BLOCK * KR_ITEMS, 256u * 8u)), block(BLOCK);
    unsigned long long* cur = reinterpret_cast<unsigned long long*>(d_cursor);
    with_bool(rc, [&](auto rcv) {
        constexpr bool RC = decltype(rcv)::value;
        if (nw == 1) hipLaunchKernelGGL((keep_var_kernel<1, RC>), grid, block, 0, stream, d_rec, n, d_win_prefix, d_rec_prefix, n_reads, mode, span, seq_base, d_out, cur);
        else         hipLaunchKernelGGL((keep_var_kernel<2, RC>), grid, block, 0, stream, d_rec, n, d_win_prefix, d_rec_prefix, n_reads, mode, span, seq_base, d_out, cur);
        return 0;
    });
    KCHECK_HIP(hipGetLastError());
    return KATOME_OK;
}
int table_max_windows(const uint64_t* d_win_prefix, uint64_t n_reads, uint64_t* max_windows, hipStream_t stream) {
    *max_windows = 0;
    if (!n_reads) return KATOME_OK;
    DevBuf out(stream);
    KCHECK(out.alloc(8));
    KCHECK_HIP(hipMemsetAsync(out.p, 0, 8, stream));
    hipLaunchKernelGGL(max_windows_kernel, dim3(grid_for(n_reads, BLOCK, 256u * 8u)), dim3(BLOCK), 0, stream, d_win_prefix, n_reads, out.as<unsigned long long>());
    KCHECK_HIP(hipGetLastError());
    KCHECK_HIP(hipMemcpyAsync(max_windows, out.p, 8, hipMemcpyDeviceToHost, stream));
    KCHECK_HIP(hipStreamSynchronize(stream));
    return KATOME_OK;
}

// the tagged records of the next level out of a list of distinct tiles with their tags and counts (list_to_tagged_records_kernel)
int table_list_to_tagged_records(const uint64_t* d_list, const uint32_t* d_counts, uint64_t n_tiles, uint32_t tile_bases, uint32_t sub_len, uint32_t n_sub,
                                 uint32_t stride, bool rc, DevBuf& recs, DevBuf& weights, uint64_t* n_records, hipStream_t stream, uint64_t extra_room,
                                 DevBuf* first_counts, bool delta) {
    const uint32_t nwt = (uint32_t)key_words_for_k(tile_bases), nwk = (uint32_t)key_words_for_k(sub_len);
    *n_records = n_tiles * n_sub;
    KCHECK(recs.alloc((*n_records + extra_room + 1) * 8 * (nwk + 1), stream));
    KCHECK(weights.alloc((*n_records + extra_room + 1) * 4, stream));
    if (*n_records == 0) { if (first_counts) first_counts->release(); return KATOME_OK; }
    const bool with_counts = first_counts && fused_hist_on() && !extra_room;
    const uint32_t tile_keys = dev_sort_tile_keys(nwk + 1);
    const uint64_t n_out_tiles = (*n_records + tile_keys - 1) / tile_keys;
    u32* d_digit_counts = nullptr;
    if (with_counts) { KCHECK(first_counts->alloc(n_out_tiles * 256 * 4 + 16, stream)); d_digit_counts = first_counts->as<u32>(); }
    else if (first_counts) first_counts->release();
    const dim3 grid(with_counts ? grid_for(n_out_tiles, 1, 256u * 32u) : grid_for(*n_records, BLOCK, 256u * 32u)), block(BLOCK);
    KernelScope ks(K_RECORDS, stream, n_tiles);
#define KATOME_LT(NWT, NWK) with_bool(rc, [&](auto rcv) { return with_bool(delta, [&](auto dv) { hipLaunchKernelGGL((list_to_tagged_records_kernel<NWT, NWK, decltype(rcv)::value, decltype(dv)::value>), grid, block, 0, stream, d_list, d_counts, n_tiles, sub_len, n_sub, stride, recs.as<u64>(), weights.as<u32>(), tile_keys, d_digit_counts); return 0; }); })
    if (nwt == 2 && nwk == 2) KATOME_LT(2, 2);
    else if (nwt == 2 && nwk == 1) KATOME_LT(2, 1);
    else if (nwt == 1 && nwk == 1) KATOME_LT(1, 1);
    else { set_error("tagged records of a tile list: tiles of %u words into windows of %u", nwt, nwk); return KATOME_E_UNSUPPORTED; }
#undef KATOME_LT
    KCHECK_HIP(hipGetLastError());
    return KATOME_OK;
}

int tiles_to_edges_sorted_seen(Table& tiles, uint32_t k, uint32_t span, bool rc, SeenTag tag, DevBuf& edge_key, DevBuf& seq_weight,
                               uint64_t* n_edges, uint64_t* n_distinct, hipStream_t stream, const uint64_t* d_extra, uint64_t n_extra) {
    *n_edges = 0; *n_distinct = 0;
    const uint32_t nwk = (uint32_t)key_words_for_k(k), stride = nwk + 1;
    const bool shapes = tiles.track_seen && ((nwk == 1 && tiles.nw <= 2) || (nwk == 2 && (tiles.nw == 2 || tiles.nw == 3)));
    if (!shapes || !tag.packs()) return KATOME_E_UNSUPPORTED;
    const uint64_t seq_per_read = tag.seq_per_read;
    uint64_t occ = 0;
    KCHECK(table_occupied(tiles, &occ, stream));
    const u64 bound = occ * span + n_extra;
    if (!lcs_level_fits(bound)) return KATOME_E_UNSUPPORTED;          // (tagged_records_sorted's own bound, asked before the records are made)
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
        const u64 magic = tag.delta ? 0 : ~0ull / seq_per_read + 1;
#define KATOME_SR(NWT, NWK) KCHECK(with_bool(rc, [&](auto rcv) -> int { return with_bool(tag.delta, [&](auto dv) -> int {              \
            const auto kernel = seen_records_kernel<NWT, NWK, decltype(rcv)::value, decltype(dv)::value>;                                \
            const size_t lds = (size_t)BLOCK * TR_ITEMS * (8 * NWT + 8 + 8 + 4);                                                         \
            KCHECK_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));                  \
            hipLaunchKernelGGL(kernel, grid, block, lds, stream, tiles.slots.as<SlotOf<NWT>::type>(), tiles.seen.as<u64>(), tiles.cap, k, span, seq_per_read, magic, recs.as<u64>(), wts.as<u32>(), rec_cursor, err); \
            return KATOME_OK; }); }))
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
    return tagged_records_sorted(recs, wts, n, k, rc, tag, false, edge_key, seq_weight, n_edges, n_distinct, stream);
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
