// depth.hip -- katome_dev_depth / katome_dev_depth_arrays (include/katome_gpu.h has the semantics): every window of every query
// sequence looked up among the graph's edges, reduced per sequence, without a record array in between.
//
//   index    the edge keys in ascending order (the graph's own array where it ascends strictly, else a sorted copy with the
//            permutation back to edge indices) and dev_bucket_index's directory over their top B bits, B by dev_rank's rule.
//   kernel   work is cut by WINDOWS: a workgroup takes a tile of DEPTH_TILE consecutive windows of the whole query, a lane
//            DEPTH_WPL consecutive windows of it.  The lane builds its first k-mer from k - 1 bases and then rolls one base per
//            window (the reverse complement beside it under EITHER_STRAND); where its stretch runs into the next sequence it
//            starts again there.  Neighbouring windows land in unrelated buckets, so the kernel waits for memory: a lane keeps
//            DEPTH_PF lookups in flight (directory entries, then the bucket's binary search in lockstep, then the weights).
//   results  a lane sums what it found while the sequence stays the same and hands the run to the sequence's LDS slot (the first
//            DEPTH_SLOTS sequences of a tile; later ones go straight to the outputs' atomics).  A sequence wholly inside the
//            tile is then written plainly, one that straddles tiles gets one atomic add / min / max per tile on outputs that
//            were initialised beforehand.  Everything is an integer: the outcome does not depend on the order.
//            The per-window values are staged in LDS and written coalesced; the per-edge hit counts are u32 atomics on the edge's slot.
#include <algorithm>

#include "builder.h"
#include "edge_keys.h"

namespace {

constexpr int DEPTH_WPL = 16;                       // consecutive windows per lane
constexpr int DEPTH_TILE = BLOCK * DEPTH_WPL;       // windows per workgroup
constexpr int DEPTH_PF = 4;                         // lookups a lane keeps in flight
constexpr int DEPTH_SLOTS = 512;                    // sequences of a tile that are reduced in LDS
constexpr u64 NOWHERE = ~0ull;
typedef unsigned long long ull;

struct DepthQuery { const uint8_t* seq; const u64* byte_off; const u32* len; const u64* win_off; u64 n_seqs, n_windows; };
struct DepthIndexView { const u64* keys; const u32* perm; const u64* dir; const u32* weight; u64 n; u32 key_bits, B; };
struct DepthPtrs { u64 *present, *invalid, *sum; u32 *mn, *mx; u64* window_off; u64* window_edge; u32* edge_hits; u64* totals; };

// dev_rank's sizing rule (radix.hip): the B with 2^B <= n / 8 < 2^(B + 1), 8 to 16 keys to a bucket
u32 bucket_bits(u64 n, u32 key_bits) {
    u32 B = 1;
    while ((2ull << B) <= n / 8 && B < 27) ++B;
    return B > key_bits ? key_bits : B;
}

// ---- the query's offsets, checked before anything is read through them; every sequence's windows; the outputs' start values ------
template <bool ASCII>
__global__ __launch_bounds__(BLOCK) void depth_windows_kernel(u32 k, const u64* __restrict__ byte_off, const u32* __restrict__ len, u64 n_seqs, u64 seq_bytes,
                                                              u32* __restrict__ counts, ull* __restrict__ bad, DepthPtrs out) {
    for (u64 s = (u64)blockIdx.x * BLOCK + threadIdx.x; s < n_seqs; s += (u64)gridDim.x * BLOCK) {
        const u64 off = byte_off[s];
        const u32 l = len[s];
        const u64 need = ASCII ? (u64)l : ((u64)l + 3) / 4;
        const bool ok = off <= seq_bytes && need <= seq_bytes - off && (s == 0 || byte_off[s - 1] <= off);
        if (!ok) atomicMin(bad, (ull)s);
        counts[s] = l >= k ? l - k + 1 : 0;
        out.present[s] = 0; out.invalid[s] = 0; out.sum[s] = 0; out.mn[s] = ~0u; out.mx[s] = 0;
    }
}

// ---- index: does the key array ascend strictly?  which sorted neighbours are equal? ---------------------------------------------
template <int NW>
__global__ __launch_bounds__(BLOCK) void depth_order_kernel(const u64* __restrict__ keys, u64 n, u32* __restrict__ descents) {
    bool any = false;
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x + 1; i < n; i += (u64)gridDim.x * BLOCK)
        any |= !key_lt(load_key<NW>(keys, i - 1), load_key<NW>(keys, i));
    if (any) atomicOr(descents, 1u);
}
template <int NW>
__global__ __launch_bounds__(BLOCK) void depth_equal_kernel(const u64* __restrict__ sorted, u64 n, ull* __restrict__ where) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x + 1; i < n; i += (u64)gridDim.x * BLOCK)
        if (key_eq(load_key<NW>(sorted, i - 1), load_key<NW>(sorted, i))) atomicMin(where, (ull)i);
}
__global__ __launch_bounds__(BLOCK) void depth_hit_edges_kernel(const u32* __restrict__ hits, u64 n, ull* __restrict__ total) {
    u32 mine = 0;
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK) mine += hits[i] != 0;
    mine = wave_sum(mine);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(total, (ull)mine);
}

// ---- the k-mer of a window, rolled ------------------------------------------------------------------------------------------------
template <int NW> __device__ __forceinline__ void roll_fwd(Key<NW>& f, u32 c, u64 mask0) {
    if constexpr (NW == 1) f.w[0] = ((f.w[0] << 2) | c) & mask0;
    else { f.w[0] = ((f.w[0] << 2) | (f.w[1] >> 62)) & mask0; f.w[1] = (f.w[1] << 2) | c; }
}
// the reverse complement takes the new base's complement at its top (bit `top` = 2k - 2 of the key)
template <int NW> __device__ __forceinline__ void roll_rev(Key<NW>& r, u32 c, u32 top) {
    const u64 in = (u64)(3u - c);
    if constexpr (NW == 1) r.w[0] = (r.w[0] >> 2) | (in << top);
    else {
        r.w[1] = (r.w[1] >> 2) | (r.w[0] << 62);
        r.w[0] >>= 2;
        if (top >= 64) r.w[0] |= in << (top - 64); else r.w[1] |= in << top;
    }
}
template <bool ASCII> __device__ __forceinline__ u32 fetch_base(const uint8_t* __restrict__ p, u64 i, bool& bad) {
    if constexpr (ASCII) {
        const uint8_t ch = p[i];
        const u32 c = ch == 'A' ? 0u : ch == 'C' ? 1u : ch == 'G' ? 2u : ch == 'T' ? 3u : 4u;
        bad = c == 4u;
        return c & 3u;
    } else {
        bad = false;
        return (u32)(p[i >> 2] >> (6 - 2 * (u32)(i & 3))) & 3u;
    }
}
// the sequence that holds window g: the last s in [s_lo, s_hi] with win_off[s] <= g (win_off[s_lo] <= g < win_off[s_hi + 1])
__device__ __forceinline__ u64 seq_of_window(const u64* __restrict__ win_off, u64 s_lo, u64 s_hi, u64 g) {
    u64 lo = s_lo + 1, hi = s_hi + 1;
    while (lo < hi) { const u64 mid = lo + ((hi - lo) >> 1); if (win_off[mid] > g) hi = mid; else lo = mid + 1; }
    return lo - 1;
}

// DEPTH_PF lookups side by side: pos[j] = where q[j] lies among the sorted keys, NOWHERE if it does not (or is not wanted)
template <int NW>
__device__ __forceinline__ void probe(const DepthIndexView& ix, const Key<NW> (&q)[DEPTH_PF], const bool (&want)[DEPTH_PF], u64 (&pos)[DEPTH_PF]) {
    u64 lo[DEPTH_PF], hi[DEPTH_PF];
#pragma unroll
    for (int j = 0; j < DEPTH_PF; ++j) {
        lo[j] = hi[j] = 0;
        if (want[j]) { const u32 b = top_bits(q[j], ix.key_bits, ix.B); lo[j] = ix.dir[b]; hi[j] = ix.dir[b + 1]; }
    }
    bool more = true;
    while (more) {
        more = false;
        u64 mid[DEPTH_PF];
        Key<NW> at[DEPTH_PF];
#pragma unroll
        for (int j = 0; j < DEPTH_PF; ++j) {
            mid[j] = lo[j] + ((hi[j] - lo[j]) >> 1);
            at[j] = q[j];
            if (lo[j] < hi[j]) at[j] = load_key<NW>(ix.keys, mid[j]);
        }
#pragma unroll
        for (int j = 0; j < DEPTH_PF; ++j)
            if (lo[j] < hi[j]) {
                if (key_lt(at[j], q[j])) lo[j] = mid[j] + 1; else hi[j] = mid[j];
                more |= lo[j] < hi[j];
            }
    }
    Key<NW> at[DEPTH_PF];
#pragma unroll
    for (int j = 0; j < DEPTH_PF; ++j) {
        at[j] = q[j];
        if (want[j] && lo[j] < ix.n) at[j] = load_key<NW>(ix.keys, lo[j]);
    }
#pragma unroll
    for (int j = 0; j < DEPTH_PF; ++j) pos[j] = (want[j] && lo[j] < ix.n && key_eq(at[j], q[j])) ? lo[j] : NOWHERE;
}

template <int NW, bool ASCII, bool EITHER, bool WINDOWS>
__global__ __launch_bounds__(BLOCK) void depth_kernel(u32 k, DepthQuery Q, DepthIndexView ix, DepthPtrs out) {
    __shared__ ull s_sum[DEPTH_SLOTS];
    __shared__ u32 s_present[DEPTH_SLOTS], s_invalid[DEPTH_SLOTS], s_min[DEPTH_SLOTS], s_max[DEPTH_SLOTS];
    __shared__ u64 s_stage[WINDOWS ? DEPTH_TILE : 1];
    __shared__ u64 s_range[2];
    __shared__ ull s_tot[3];
    const u32 t = threadIdx.x;
    const u64 base = (u64)blockIdx.x * DEPTH_TILE, end = min(base + (u64)DEPTH_TILE, Q.n_windows);
    if (base >= end) return;
    if (t < 2) s_range[t] = seq_of_window(Q.win_off, 0, Q.n_seqs - 1, t == 0 ? base : end - 1);
    if (t < 3) s_tot[t] = 0;
    for (u32 i = t; i < DEPTH_SLOTS; i += BLOCK) { s_sum[i] = 0; s_present[i] = 0; s_invalid[i] = 0; s_min[i] = ~0u; s_max[i] = 0; }
    __syncthreads();
    const u64 s_first = s_range[0], s_last = s_range[1];

    const u64 mask0 = NW == 1 ? (1ull << (2 * k)) - 1 : (2 * k == 64 ? 0ull : (1ull << (2 * k - 64)) - 1);
    const u32 top = 2 * k - 2;
    const u64 g0 = base + (u64)t * DEPTH_WPL;
    // where the lane reads
    u64 s = 0, s_beg = 0, s_end = 0, p = 0;
    const uint8_t* sp = nullptr;
    bool primed = false;
    long long last_bad = -1;
    Key<NW> f, r;
    for (int i = 0; i < NW; ++i) f.w[i] = r.w[i] = 0;
    if (g0 < end) {
        s = seq_of_window(Q.win_off, s_first, s_last, g0);
        s_beg = Q.win_off[s]; s_end = Q.win_off[s + 1];
        sp = Q.seq + Q.byte_off[s];
    }
    // what the lane has found in the sequence it is in
    u64 acc_s = NOWHERE, a_sum = 0;
    u32 a_present = 0, a_invalid = 0, a_min = ~0u, a_max = 0;
    u64 t_present = 0, t_invalid = 0, t_sum = 0;
    auto flush = [&]() {
        if (acc_s == NOWHERE) return;
        const u64 slot = acc_s - s_first;
        if (slot < (u64)DEPTH_SLOTS) {
            if (a_present) { atomicAdd(&s_present[slot], a_present); atomicAdd(&s_sum[slot], (ull)a_sum); atomicMin(&s_min[slot], a_min); atomicMax(&s_max[slot], a_max); }
            if (a_invalid) atomicAdd(&s_invalid[slot], a_invalid);
        } else {
            if (a_present) {
                atomicAdd((ull*)&out.present[acc_s], (ull)a_present); atomicAdd((ull*)&out.sum[acc_s], (ull)a_sum);
                atomicMin(&out.mn[acc_s], a_min); atomicMax(&out.mx[acc_s], a_max);
            }
            if (a_invalid) atomicAdd((ull*)&out.invalid[acc_s], (ull)a_invalid);
        }
        t_present += a_present; t_invalid += a_invalid; t_sum += a_sum;
        a_sum = 0; a_present = a_invalid = 0; a_min = ~0u; a_max = 0;
    };

    for (int c0 = 0; c0 < DEPTH_WPL; c0 += DEPTH_PF) {
        Key<NW> q[DEPTH_PF], qr[DEPTH_PF];
        bool want[DEPTH_PF], inval[DEPTH_PF];
        u64 sj[DEPTH_PF];
#pragma unroll
        for (int j = 0; j < DEPTH_PF; ++j) {
            const u64 g = g0 + c0 + j;
            want[j] = inval[j] = false; sj[j] = NOWHERE; q[j] = f; qr[j] = r;
            if (g < end) {
                if (g >= s_end) {
                    do { ++s; s_end = Q.win_off[s + 1]; } while (s_end <= g);
                    s_beg = Q.win_off[s];
                    sp = Q.seq + Q.byte_off[s];
                    primed = false;
                }
                if (!primed) {
                    p = g - s_beg;
                    for (int i = 0; i < NW; ++i) f.w[i] = r.w[i] = 0;
                    last_bad = -1;
                    for (u32 i = 0; i + 1 < k; ++i) {
                        bool bad;
                        const u32 c = fetch_base<ASCII>(sp, p + i, bad);
                        roll_fwd<NW>(f, c, mask0);
                        if constexpr (EITHER) roll_rev<NW>(r, c, top);
                        if (bad) last_bad = (long long)(p + i);
                    }
                    primed = true;
                }
                bool bad;
                const u32 c = fetch_base<ASCII>(sp, p + k - 1, bad);
                roll_fwd<NW>(f, c, mask0);
                if constexpr (EITHER) roll_rev<NW>(r, c, top);
                if (bad) last_bad = (long long)(p + k - 1);
                inval[j] = last_bad >= (long long)p;
                want[j] = !inval[j];
                q[j] = f; qr[j] = r; sj[j] = s;
                ++p;
            }
        }
        u64 pos[DEPTH_PF], val[DEPTH_PF];
        u32 w[DEPTH_PF];
        probe<NW>(ix, q, want, pos);
        if constexpr (EITHER) {
            bool want2[DEPTH_PF];
            u64 pos2[DEPTH_PF];
#pragma unroll
            for (int j = 0; j < DEPTH_PF; ++j) want2[j] = want[j] && pos[j] == NOWHERE;
            probe<NW>(ix, qr, want2, pos2);
#pragma unroll
            for (int j = 0; j < DEPTH_PF; ++j) {
                val[j] = pos[j] != NOWHERE ? 0 : KATOME_DEPTH_REVERSE;
                if (pos[j] == NOWHERE) pos[j] = pos2[j];
            }
        } else {
#pragma unroll
            for (int j = 0; j < DEPTH_PF; ++j) val[j] = 0;
        }
        // the edges' indices, then their weights: independent loads again
#pragma unroll
        for (int j = 0; j < DEPTH_PF; ++j)
            if (pos[j] != NOWHERE && ix.perm) pos[j] = ix.perm[pos[j]];
#pragma unroll
        for (int j = 0; j < DEPTH_PF; ++j) {
            w[j] = 0;
            if (pos[j] != NOWHERE) { w[j] = ix.weight[pos[j]]; val[j] |= pos[j]; }
            else val[j] = inval[j] ? KATOME_DEPTH_INVALID : KATOME_DEPTH_ABSENT;
        }
#pragma unroll
        for (int j = 0; j < DEPTH_PF; ++j) {
            if (sj[j] == NOWHERE) continue;
            if (sj[j] != acc_s) { flush(); acc_s = sj[j]; }
            if (pos[j] != NOWHERE) {
                ++a_present; a_sum += w[j]; a_min = min(a_min, w[j]); a_max = max(a_max, w[j]);
                if (out.edge_hits) atomicAdd(&out.edge_hits[pos[j]], 1u);
            } else if (inval[j]) ++a_invalid;
            if constexpr (WINDOWS) s_stage[t * DEPTH_WPL + c0 + j] = val[j];
        }
    }
    flush();
    if (t_present) atomicAdd(&s_tot[0], (ull)t_present);
    if (t_invalid) atomicAdd(&s_tot[1], (ull)t_invalid);
    if (t_sum) atomicAdd(&s_tot[2], (ull)t_sum);
    __syncthreads();

    // the tile's sequences: s_first .. s_last, the first DEPTH_SLOTS of them from LDS
    const u64 n_here = min(s_last - s_first + 1, (u64)DEPTH_SLOTS);
    for (u64 i = t; i < n_here; i += BLOCK) {
        const u64 q_s = s_first + i;
        const bool inside = Q.win_off[q_s] >= base && Q.win_off[q_s + 1] <= end;
        if (inside) {
            out.present[q_s] = s_present[i]; out.invalid[q_s] = s_invalid[i]; out.sum[q_s] = s_sum[i]; out.mn[q_s] = s_min[i]; out.mx[q_s] = s_max[i];
        } else {
            if (s_present[i]) {
                atomicAdd((ull*)&out.present[q_s], (ull)s_present[i]); atomicAdd((ull*)&out.sum[q_s], s_sum[i]);
                atomicMin(&out.mn[q_s], s_min[i]); atomicMax(&out.mx[q_s], s_max[i]);
            }
            if (s_invalid[i]) atomicAdd((ull*)&out.invalid[q_s], (ull)s_invalid[i]);
        }
    }
    if (t < 3 && s_tot[t]) atomicAdd((ull*)&out.totals[t], s_tot[t]);
    if constexpr (WINDOWS)
        for (u64 i = t; i < end - base; i += BLOCK) out.window_edge[base + i] = s_stage[i];
}

template <int NW, bool ASCII>
void launch_depth(bool either, bool windows, unsigned grid, hipStream_t stream, u32 k, const DepthQuery& Q, const DepthIndexView& ix, const DepthPtrs& out) {
    const dim3 g(grid), blk(BLOCK);
    if (either) {
        if (windows) hipLaunchKernelGGL((depth_kernel<NW, ASCII, true, true>), g, blk, 0, stream, k, Q, ix, out);
        else         hipLaunchKernelGGL((depth_kernel<NW, ASCII, true, false>), g, blk, 0, stream, k, Q, ix, out);
    } else {
        if (windows) hipLaunchKernelGGL((depth_kernel<NW, ASCII, false, true>), g, blk, 0, stream, k, Q, ix, out);
        else         hipLaunchKernelGGL((depth_kernel<NW, ASCII, false, false>), g, blk, 0, stream, k, Q, ix, out);
    }
}

// ---- the index ------------------------------------------------------------------------------------------------------------------
// refuse_equal: two equal keys are KATOME_E_ARG naming one such pair (the arrays entry; a builder's keys are what they are)
int build_index(const u64* d_key, u64 n, u32 nw, u32 key_bits, DepthIndex& ix, bool refuse_equal, hipStream_t stream) {
    ix.drop();
    ix.keys.stream = ix.perm.stream = ix.dir.stream = stream;
    KernelScope ks(K_DEPTH_INDEX, stream, n);
    bool ascends = true;
    if (n >= 2) {
        DevBuf flag(stream);
        KCHECK(flag.alloc(16));
        KCHECK_HIP(hipMemsetAsync(flag.p, 0, 4, stream));
        if (nw == 1) KLAUNCH(depth_order_kernel<1>, n, stream, d_key, n, flag.as<u32>());
        else         KLAUNCH(depth_order_kernel<2>, n, stream, d_key, n, flag.as<u32>());
        KCHECK_HIP(hipGetLastError());
        u32 descents = 0;
        KCHECK_HIP(hipMemcpyAsync(&descents, flag.p, 4, hipMemcpyDeviceToHost, stream));
        KCHECK_HIP(hipStreamSynchronize(stream));
        ascends = descents == 0;
    }
    const u64* sorted = d_key;
    if (!ascends) {
        if (n >> 32) { set_error("depth: %llu edges that do not ascend by key: the permutation back to edge indices is 32 bits wide", (unsigned long long)n); return KATOME_E_UNSUPPORTED; }
        KCHECK(ix.keys.alloc(n * 8 * nw));
        KCHECK(ix.perm.alloc(n * 4));
        KCHECK_HIP(hipMemcpyAsync(ix.keys.p, d_key, n * 8 * nw, hipMemcpyDeviceToDevice, stream));
        KCHECK(dev_iota(ix.perm.as<u32>(), n, stream));
        KCHECK(dev_sort(ix.keys.as<u64>(), ix.perm.as<u32>(), n, nw, key_bits, stream));
        sorted = ix.keys.as<u64>();
        if (refuse_equal) {
            DevBuf where(stream);
            KCHECK(where.alloc(16));
            KCHECK_HIP(hipMemsetAsync(where.p, 0xFF, 8, stream));
            if (nw == 1) KLAUNCH(depth_equal_kernel<1>, n, stream, sorted, n, where.as<ull>());
            else         KLAUNCH(depth_equal_kernel<2>, n, stream, sorted, n, where.as<ull>());
            KCHECK_HIP(hipGetLastError());
            u64 at = NOWHERE;
            KCHECK_HIP(hipMemcpyAsync(&at, where.p, 8, hipMemcpyDeviceToHost, stream));
            KCHECK_HIP(hipStreamSynchronize(stream));
            if (at != NOWHERE) {
                u32 pair[2] = {0, 0};
                KCHECK_HIP(hipMemcpyAsync(pair, ix.perm.as<u32>() + at - 1, 8, hipMemcpyDeviceToHost, stream));
                KCHECK_HIP(hipStreamSynchronize(stream));
                set_error("depth: keys %u and %u are equal (the edge keys must be distinct)", std::min(pair[0], pair[1]), std::max(pair[0], pair[1]));
                ix.drop();
                return KATOME_E_ARG;
            }
        }
    }
    ix.B = bucket_bits(n, key_bits);
    KCHECK(ix.dir.alloc(((1ull << ix.B) + 2) * 8));
    KCHECK(dev_bucket_index(sorted, n, nw, key_bits, ix.B, ix.dir.as<u64>(), stream));
    ix.of_keys = d_key; ix.n = n; ix.valid = true;
    return KATOME_OK;
}

constexpr uint32_t ALL_FLAGS = KATOME_DEPTH_EITHER_STRAND | KATOME_DEPTH_WINDOWS | KATOME_DEPTH_EDGE_HITS;
int check_depth_args(uint32_t encoding, uint32_t flags) {
    if (encoding > KATOME_DEPTH_ASCII) { set_error("depth: unknown encoding %u", encoding); return KATOME_E_ARG; }
    if (flags & ~ALL_FLAGS) { set_error("depth: unknown flag bits 0x%x", flags & ~ALL_FLAGS); return KATOME_E_ARG; }
    return KATOME_OK;
}

// the query against an index.  out: the per-sequence arrays and window_off (n_seqs + 1) are there; window_edge / edge_hits are made by
// `make_optional` once the number of windows is known (it may leave them null).  totals: {n_windows, n_present, n_invalid, weight_sum, n_edges_hit}
template <class F>
int run_depth(u32 k, u32 nw, const DepthIndex& ix, const u64* d_edge_key, const u32* d_edge_weight, u64 n_edges, uint32_t encoding, uint32_t flags,
              const uint8_t* d_seq, u64 seq_bytes, const u64* d_byte_off, const u32* d_len, u64 n_seqs, DepthPtrs out, F make_optional, u64 totals[5],
              hipStream_t stream) {
    for (int i = 0; i < 5; ++i) totals[i] = 0;
    const bool ascii = encoding == KATOME_DEPTH_ASCII;
    if (n_seqs >> 40) { set_error("depth: %llu sequences in one call", (unsigned long long)n_seqs); return KATOME_E_UNSUPPORTED; }
    DevBuf counts(stream), small(stream);
    KCHECK(counts.alloc(n_seqs * 4 + 16));
    KCHECK(small.alloc(64));                     // [0]: the first sequence with a bad offset; [1..4]: the kernel's totals
    KCHECK_HIP(hipMemsetAsync(small.p, 0, 64, stream));
    KCHECK_HIP(hipMemsetAsync(small.p, 0xFF, 8, stream));
    out.totals = small.as<u64>() + 1;
    if (n_seqs) {
        if (ascii) KLAUNCH(depth_windows_kernel<true>, n_seqs, stream, k, d_byte_off, d_len, n_seqs, seq_bytes, counts.as<u32>(), small.as<ull>(), out);
        else       KLAUNCH(depth_windows_kernel<false>, n_seqs, stream, k, d_byte_off, d_len, n_seqs, seq_bytes, counts.as<u32>(), small.as<ull>(), out);
        KCHECK_HIP(hipGetLastError());
        KCHECK(dev_scan_counts(counts.as<u32>(), n_seqs, out.window_off, stream));
    } else {
        KCHECK_HIP(hipMemsetAsync(out.window_off, 0, 8, stream));
    }
    u64 bad = NOWHERE, n_windows = 0;
    KCHECK_HIP(hipMemcpyAsync(&bad, small.p, 8, hipMemcpyDeviceToHost, stream));
    KCHECK_HIP(hipMemcpyAsync(&n_windows, out.window_off + n_seqs, 8, hipMemcpyDeviceToHost, stream));
    KCHECK_HIP(hipStreamSynchronize(stream));
    if (bad != NOWHERE) {
        u64 off[2] = {0, 0};
        u32 len = 0;
        KCHECK_HIP(hipMemcpyAsync(off, d_byte_off + (bad ? bad - 1 : 0), bad ? 16 : 8, hipMemcpyDeviceToHost, stream));
        KCHECK_HIP(hipMemcpyAsync(&len, d_len + bad, 4, hipMemcpyDeviceToHost, stream));
        KCHECK_HIP(hipStreamSynchronize(stream));
        const u64 mine = bad ? off[1] : off[0];
        if (bad && off[0] > mine) set_error("depth: byte_off does not ascend: sequence %llu starts at %llu, the one before it at %llu", (unsigned long long)bad,
                                            (unsigned long long)mine, (unsigned long long)off[0]);
        else set_error("depth: sequence %llu (offset %llu, %u bases) runs past seq_bytes = %llu", (unsigned long long)bad, (unsigned long long)mine, len,
                       (unsigned long long)seq_bytes);
        return KATOME_E_ARG;
    }
    if (n_windows >> 32) {
        set_error("depth: %llu windows in one call, 2^32 or more: query in batches", (unsigned long long)n_windows);
        return KATOME_E_UNSUPPORTED;
    }
    totals[0] = n_windows;
    KCHECK(make_optional(n_windows, out));
    if ((flags & KATOME_DEPTH_EDGE_HITS) && out.edge_hits && n_edges) KCHECK_HIP(hipMemsetAsync(out.edge_hits, 0, n_edges * 4, stream));
    if (!(flags & KATOME_DEPTH_EDGE_HITS)) out.edge_hits = nullptr;
    const bool windows = (flags & KATOME_DEPTH_WINDOWS) && out.window_edge;
    if (n_windows) {
        const DepthQuery Q{d_seq, d_byte_off, d_len, out.window_off, n_seqs, n_windows};
        const DepthIndexView view{ix.keys.p ? ix.keys.as<u64>() : d_edge_key, ix.perm.p ? ix.perm.as<u32>() : nullptr, ix.dir.as<u64>(), d_edge_weight, n_edges, 2 * k, ix.B};
        const unsigned grid = (unsigned)((n_windows + DEPTH_TILE - 1) / DEPTH_TILE);
        const bool either = (flags & KATOME_DEPTH_EITHER_STRAND) != 0;
        KernelScope ks(K_DEPTH_KERNEL, stream, n_windows);
        if (nw == 1) { if (ascii) launch_depth<1, true>(either, windows, grid, stream, k, Q, view, out); else launch_depth<1, false>(either, windows, grid, stream, k, Q, view, out); }
        else         { if (ascii) launch_depth<2, true>(either, windows, grid, stream, k, Q, view, out); else launch_depth<2, false>(either, windows, grid, stream, k, Q, view, out); }
        KCHECK_HIP(hipGetLastError());
        if (out.edge_hits && n_edges) {
            KLAUNCH(depth_hit_edges_kernel, n_edges, stream, out.edge_hits, n_edges, (ull*)(out.totals + 3));
            KCHECK_HIP(hipGetLastError());
        }
    }
    KCHECK_HIP(hipMemcpyAsync(totals + 1, out.totals, 32, hipMemcpyDeviceToHost, stream));
    KCHECK_HIP(hipStreamSynchronize(stream));
    return KATOME_OK;
}

}  // namespace

extern "C" {

int katome_dev_depth(katome_builder* b, uint32_t encoding, uint32_t flags, const uint8_t* d_seq, uint64_t seq_bytes, const uint64_t* d_byte_off,
                     const uint32_t* d_len, uint64_t n_seqs, katome_dev_depth_result* out, void* stream_) {
    if (!b || !out) { set_error("null argument"); return KATOME_E_ARG; }
    memset(out, 0, sizeof *out);
    if (!b->finalized) { set_error("depth: call katome_dev_finalize first"); return KATOME_E_ARG; }
    KCHECK(check_depth_args(encoding, flags));
    if (n_seqs && (!d_byte_off || !d_len)) { set_error("null argument"); return KATOME_E_ARG; }
    hipStream_t stream = (hipStream_t)stream_;
    KCHECK_HIP(hipSetDevice(b->s.device));
    PhaseScope ps(b->prof, PH_DEPTH, stream);
    DepthIndex& ix = b->depth_index;
    if (!ix.valid || ix.of_keys != b->edge_key.p || ix.n != b->n_edges)
        KCHECK(build_index(b->edge_key.as<u64>(), b->n_edges, b->nw, 2 * b->s.k, ix, false, stream));
    DepthOutput& o = b->depth;
    o.window_edge.release(); o.edge_hits.release();
    KCHECK(o.present.alloc(n_seqs * 8 + 16, stream)); KCHECK(o.invalid.alloc(n_seqs * 8 + 16, stream)); KCHECK(o.sum.alloc(n_seqs * 8 + 16, stream));
    KCHECK(o.mn.alloc(n_seqs * 4 + 16, stream)); KCHECK(o.mx.alloc(n_seqs * 4 + 16, stream)); KCHECK(o.window_off.alloc((n_seqs + 1) * 8 + 16, stream));
    DepthPtrs p{o.present.as<u64>(), o.invalid.as<u64>(), o.sum.as<u64>(), o.mn.as<u32>(), o.mx.as<u32>(), o.window_off.as<u64>(), nullptr, nullptr, nullptr};
    const uint64_t n_edges = b->n_edges;
    auto make_optional = [&](u64 n_windows, DepthPtrs& q) -> int {
        if (flags & KATOME_DEPTH_WINDOWS) { KCHECK(o.window_edge.alloc(n_windows * 8 + 16, stream)); q.window_edge = o.window_edge.as<u64>(); }
        if (flags & KATOME_DEPTH_EDGE_HITS) { KCHECK(o.edge_hits.alloc(n_edges * 4 + 16, stream)); q.edge_hits = o.edge_hits.as<u32>(); }
        return KATOME_OK;
    };
    u64 totals[5];
    KCHECK(run_depth(b->s.k, b->nw, ix, b->edge_key.as<u64>(), b->edge_weight.as<u32>(), n_edges, encoding, flags, d_seq, seq_bytes, d_byte_off, d_len, n_seqs, p,
                     make_optional, totals, stream));
    out->n_seqs = n_seqs; out->n_windows = totals[0]; out->n_present = totals[1]; out->n_invalid = totals[2]; out->weight_sum = totals[3];
    out->n_edges = n_edges; out->n_edges_hit = totals[4];
    out->d_seq_present = p.present; out->d_seq_invalid = p.invalid; out->d_seq_sum = p.sum; out->d_seq_min = p.mn; out->d_seq_max = p.mx;
    out->d_seq_window_off = p.window_off;
    out->d_window_edge = (flags & KATOME_DEPTH_WINDOWS) ? o.window_edge.as<u64>() : nullptr;
    out->d_edge_hits = (flags & KATOME_DEPTH_EDGE_HITS) ? o.edge_hits.as<u32>() : nullptr;
    return KATOME_OK;
}

uint64_t katome_dev_depth_index_bytes(katome_builder* b) { return b ? b->depth_index.bytes() : 0; }

int katome_dev_depth_arrays(int device, uint32_t k, const uint64_t* d_edge_key, const uint32_t* d_edge_weight, uint64_t n_edges, uint32_t encoding,
                            uint32_t flags, const uint8_t* d_seq, uint64_t seq_bytes, const uint64_t* d_byte_off, const uint32_t* d_len, uint64_t n_seqs,
                            uint64_t* d_seq_present, uint64_t* d_seq_invalid, uint64_t* d_seq_sum, uint32_t* d_seq_min, uint32_t* d_seq_max,
                            uint64_t* d_seq_window_off, uint64_t* d_window_edge, uint64_t window_cap, uint32_t* d_edge_hits, uint64_t totals[5], void* stream_) {
    KCHECK(use_device(device));
    KCHECK(check_k(k));
    KCHECK(check_depth_args(encoding, flags));
    if (!totals || !d_seq_window_off || (n_seqs && (!d_byte_off || !d_len || !d_seq_present || !d_seq_invalid || !d_seq_sum || !d_seq_min || !d_seq_max)) ||
        (n_edges && (!d_edge_key || !d_edge_weight)) || ((flags & KATOME_DEPTH_EDGE_HITS) && n_edges && !d_edge_hits)) {
        set_error("null argument");
        return KATOME_E_ARG;
    }
    hipStream_t stream = (hipStream_t)stream_;
    const u32 nw = (u32)key_words_for_k(k);
    DepthIndex ix;
    KCHECK(build_index(d_edge_key, n_edges, nw, 2 * k, ix, true, stream));
    DepthPtrs p{d_seq_present, d_seq_invalid, d_seq_sum, d_seq_min, d_seq_max, d_seq_window_off, d_window_edge, d_edge_hits, nullptr};
    auto make_optional = [&](u64 n_windows, DepthPtrs& q) -> int {
        if ((flags & KATOME_DEPTH_WINDOWS) && n_windows && (!q.window_edge || window_cap < n_windows)) {
            set_error("depth: %llu windows do not fit the caller's d_window_edge (%llu)", (unsigned long long)n_windows, (unsigned long long)(q.window_edge ? window_cap : 0));
            return KATOME_E_ARG;
        }
        return KATOME_OK;
    };
    return run_depth(k, nw, ix, d_edge_key, d_edge_weight, n_edges, encoding, flags, d_seq, seq_bytes, d_byte_off, d_len, n_seqs, p, make_optional, totals, stream);
}

}  // extern "C"
