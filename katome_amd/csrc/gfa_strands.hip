// gfa_strands.hip -- the unitig graph as bidirected GFA 1: a merged edge and its reverse complement (its strand twin) are ONE segment,
// and strand is spelled in the links' orientations.  The format is fixed byte for byte in include/katome_gpu.h:
//   H\tVN:Z:1.0\n
//   S\t<r>\t<bases of r>\tLN:i:<bases>\tKC:i:<w_r * kmers_r>\tew:i:<w_r>[\trc:i:<j>\trw:i:<w_j>]\n     one per representative r, ascending
//   L\t<x>\t<ox>\t<y>\t<oy>\t<k-1>M\n                                                                     canonical, distinct, ascending
// twin(i) = the j with text_j == revcomp(text_i); rep(i) = min(i, twin(i)); o(i) = '-' where twin(i) < i.  A segment without a twin
// stays on its own (the pruning stages are not strand-symmetric), a segment that is its own reverse complement is a self-twin.
//   Keys: a k-mer lies on one merged edge, so a segment's first k-mer names it.  strand_keys_kernel cuts the first k-mer and
//   revcomp(last k-mer) out of every label (any pad, any byte alignment; one word up to k = 32, two above), dev_sort orders the first
//   k-mers with the index as value, equal neighbours are refused, and strand_search_kernel looks every probe up through a bucket
//   index over the sorted keys (dev_bucket_index): a candidate, if it has the segment's length and names it back.
//   Verification (the hot path: every label is read once): the candidate pairs i <= j that name each other are compared base for base,
//   text_i forward against the complement of text_j backward, a 32-bit word (16 bases) at a time: the 2-bit groups reversed, NOT, both
//   sides cut out of their labels by a funnel shift.  The work is partitioned by WORDS, not by segment (a workgroup owns a stretch of the
//   scanned word counts and finds its pairs by the workgroup search), so one long pair spreads over many workgroups.  A mismatch ORs
//   all-ones into the two twin entries; the matching path has no atomic.
//   Links: gfa.hip's join (dev_gfa_plan, unchanged) gives every (a, b); strand_link_kernel maps it to the smaller of its two spellings
//   (rep a, o a, rep b, o b) and (rep b, flip o b, rep a, flip o a) -- flip leaves a self-twin at + -- as one key
//   (x, ox, y, oy); dev_sort and dev_unique leave the distinct links in the order they are written in.
//   The writer loops over the tile every H/S/L text shares (write_line_tile of gfa_image.h: partitioned by output bytes, every line
//   formatted once into the LDS image, bases by 128-bit stores) with this text's line description, StrandLines: S lines exist for
//   representatives only (a compacted list), carry two more tags where there is a twin, and a link's two names and orientation bytes
//   come from its key.  A line's sizes and the formatting of its fields are gfa_lines.h's, as in gfa.hip.
//   The merged GFA of the sharded shrink without a gather is not written here.
#include "builder.h"
#include "edge_keys.h"
#include "gfa_lines.h"
#include "strand_bits.h"

namespace katome {
namespace {

constexpr u32 NONE = NO_TWIN;
constexpr int TWIN_TAGS_MAX = 2 * (6 + 10);            // "\trc:i:<u32>\trw:i:<u32>": a twin's tags, between ew and the line's end
static_assert(S_TAGS_MAX + TWIN_TAGS_MAX < (int)TILE, "a segment's tags fit a tile");
constexpr u32 VERIFY_WORDS = 4;                        // 16-base words a thread compares per stretch
constexpr u32 VERIFY_TILE = BLOCK * VERIFY_WORDS;

template <int NW> __device__ __forceinline__ Key<NW> narrow(const Key<2>& a) {
    Key<NW> r;
    r.w[0] = NW == 1 ? a.w[1] : a.w[0];
    r.w[NW - 1] = a.w[1];
    return r;
}

// segment i (validated by dev_gfa_plan: kmers[i] + k - 1 bases): its first k-mer with its index, and the probe revcomp(last k-mer)
template <int NW>
__global__ __launch_bounds__(BLOCK) void strand_keys_kernel(u32 k, u64 E, const u32* __restrict__ kmers, const u64* __restrict__ label_off,
                                                            const uint8_t* __restrict__ label, u64* __restrict__ first_key, u64* __restrict__ probe,
                                                            u32* __restrict__ order) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < E; i += (u64)gridDim.x * BLOCK) {
        const uint8_t* src = label + label_off[i] + 1;
        store_key<NW>(first_key, i, narrow<NW>(first_kmer(src, k)));
        store_key<NW>(probe, i, narrow<NW>(last_kmer_revcomp(src, kmers[i] + k - 1, k)));
        order[i] = (u32)i;
    }
}
// two segments with one first k-mer: the lowest such place in the sorted keys
template <int NW>
__global__ __launch_bounds__(BLOCK) void strand_equal_keys_kernel(const u64* __restrict__ sorted, u64 E, u32* __restrict__ where) {
    for (u64 j = (u64)blockIdx.x * BLOCK + threadIdx.x + 1; j < E; j += (u64)gridDim.x * BLOCK)
        if (key_eq(load_key<NW>(sorted, j), load_key<NW>(sorted, j - 1))) atomicMin(where, (u32)j);
}
// segment i's candidate: the segment whose first k-mer is i's probe, if it has i's length.  index: dev_bucket_index over the top B bits
// of the sorted keys, which leaves a few consecutive keys to search
template <int NW>
__global__ __launch_bounds__(BLOCK) void strand_search_kernel(u64 E, u32 key_bits, u32 B, const u64* __restrict__ index, const u64* __restrict__ sorted,
                                                              const u32* __restrict__ order, const u64* __restrict__ probe, const u32* __restrict__ kmers,
                                                              u32* __restrict__ cand) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < E; i += (u64)gridDim.x * BLOCK) {
        const Key<NW> q = load_key<NW>(probe, i);
        const u32 b = top_bits(q, key_bits, B);
        u64 lo = index[b], hi = index[b + 1];                                // the first key that is not below q
        while (lo < hi) { const u64 mid = lo + ((hi - lo) >> 1); if (key_lt(load_key<NW>(sorted, mid), q)) lo = mid + 1; else hi = mid; }
        u32 c = NONE;
        if (lo < E && key_eq(load_key<NW>(sorted, lo), q)) { const u32 j = order[lo]; if (kmers[j] == kmers[i]) c = j; }
        cand[i] = c;
    }
}
// the pairs that name each other: a tentative twin for both, and the words to compare for the smaller index (a self-twin is its own pair)
__global__ __launch_bounds__(BLOCK) void strand_pair_kernel(u32 k, u64 E, const u32* __restrict__ cand, const u32* __restrict__ kmers, u32* __restrict__ twin,
                                                            u32* __restrict__ words) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < E; i += (u64)gridDim.x * BLOCK) {
        const u32 j = cand[i];
        const bool paired = j != NONE && cand[j] == (u32)i;
        twin[i] = paired ? j : NONE;
        words[i] = paired && (u32)i <= j ? (kmers[i] + k - 1 + 15) / 16 : 0;
    }
}
// word g of all the words to compare: its pair is the last segment whose first word is <= g (segments without words are passed over)
__global__ __launch_bounds__(BLOCK) void strand_verify_kernel(u32 k, u32 E, u64 W, const u64* __restrict__ word_off, const u32* __restrict__ cand,
                                                              const u32* __restrict__ kmers, const u64* __restrict__ label_off, const uint8_t* __restrict__ label,
                                                              u32* __restrict__ twin) {
    const u64 n_tiles = (W + VERIFY_TILE - 1) / VERIFY_TILE;
    for (u64 tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const u64 base = tile * VERIFY_TILE, last = min(base + VERIFY_TILE, W) - 1;
        const u32 r_lo = workgroup_search(word_off, E, base), r_hi = workgroup_search(word_off, E, last);
#pragma unroll
        for (u32 it = 0; it < VERIFY_WORDS; ++it) {
            const u64 g = base + it * BLOCK + threadIdx.x;
            if (g > last) continue;
            u32 lo = r_lo, hi = r_hi + 1;
            while (hi - lo > 1) { const u32 mid = lo + ((hi - lo) >> 1); if (word_off[mid] <= g) lo = mid; else hi = mid; }
            const u32 i = lo, j = cand[i], n = kmers[i] + k - 1;
            if (twin_word_differs(label + label_off[i] + 1, label + label_off[j] + 1, n, 16 * (u32)(g - word_off[i]))) { atomicOr(&twin[i], NONE); atomicOr(&twin[j], NONE); }
        }
    }
}
// the twins are final: who is written as a segment, and how many stay alone or are their own twin (count: {unpaired, self-twins})
__global__ __launch_bounds__(BLOCK) void strand_rep_kernel(u64 E, const u32* __restrict__ twin, u32* __restrict__ is_rep, unsigned long long* __restrict__ count) {
    u32 alone = 0, self = 0;
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < E; i += (u64)gridDim.x * BLOCK) {
        const u32 t = twin[i];
        is_rep[i] = t >= (u32)i ? 1u : 0u;                                   // (NONE is above every index)
        alone += t == NONE; self += t == (u32)i;
    }
    alone = wave_sum(alone); self = wave_sum(self);
    if ((threadIdx.x & 63) == 0) { if (alone) atomicAdd(&count[0], (unsigned long long)alone); if (self) atomicAdd(&count[1], (unsigned long long)self); }
}
// the representatives in index order, each with the bytes of its line
__global__ __launch_bounds__(BLOCK) void strand_segment_kernel(u32 k, u64 E, const u32* __restrict__ twin, const u64* __restrict__ rep_off, const u32* __restrict__ weight,
                                                               const u32* __restrict__ kmers, u32* __restrict__ name, u32* __restrict__ size) {
    if (blockIdx.x == 0 && threadIdx.x == 0) size[0] = HEADER_BYTES;
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < E; i += (u64)gridDim.x * BLOCK) {
        const u32 t = twin[i];
        if (t < (u32)i) continue;
        const u64 s = rep_off[i];
        const u32 w = weight[i], km = kmers[i], bases = km + k - 1;
        name[s] = (u32)i; size[1 + s] = segment_line_bytes(i, bases, (u64)w * km, w, t != NONE ? 6 + decimal_digits(t) + 6 + decimal_digits(weight[t]) : 0);
    }
}

// ---- links: a key is (x, ox, y, oy) as two fields f = 2 * segment + (o == '-'), fx above fy: one word while both fit 64 bits ------
struct LinkKeys { const u64* keys; u32 words, field_bits; };
__device__ __forceinline__ void link_fields(const LinkKeys& lk, u64 l, u64& fx, u64& fy) {
    if (lk.words == 1) { const u64 v = lk.keys[l]; fx = v >> lk.field_bits; fy = v & ((1ull << lk.field_bits) - 1); }
    else { fx = lk.keys[2 * l]; fy = lk.keys[2 * l + 1]; }
}
__global__ __launch_bounds__(BLOCK) void strand_link_kernel(u64 L, const u32* __restrict__ link_ab, const u32* __restrict__ twin, u64* __restrict__ keys, u32 words,
                                                            u32 field_bits) {
    for (u64 l = (u64)blockIdx.x * BLOCK + threadIdx.x; l < L; l += (u64)gridDim.x * BLOCK) {
        const u32 a = link_ab[2 * l], b = link_ab[2 * l + 1];
        u64 fx, fy;
        canonical_link(a, b, twin[a], twin[b], fx, fy);
        if (words == 1) keys[l] = fx << field_bits | fy;
        else { keys[2 * l] = fx; keys[2 * l + 1] = fy; }
    }
}
__global__ __launch_bounds__(BLOCK) void strand_link_size_kernel(u64 L, u32 k1_digits, const LinkKeys lk, u32* __restrict__ size) {
    for (u64 l = (u64)blockIdx.x * BLOCK + threadIdx.x; l < L; l += (u64)gridDim.x * BLOCK) {
        u64 fx, fy;
        link_fields(lk, l, fx, fy);
        size[l] = link_line_bytes(fx >> 1, fy >> 1, k1_digits);
    }
}
// segment s's first link: the first one whose x is not below its name (link_first[S] = L); its first base: behind "S\t<name>\t"
__global__ __launch_bounds__(BLOCK) void strand_segment_off_kernel(u64 S, u64 L, const u32* __restrict__ name, const LinkKeys lk, const u64* __restrict__ line_off,
                                                                   u64* __restrict__ segment_off, u64* __restrict__ link_first) {
    for (u64 s = (u64)blockIdx.x * BLOCK + threadIdx.x; s <= S; s += (u64)gridDim.x * BLOCK) {
        if (s == S) { link_first[s] = L; continue; }
        const u64 want = 2ull * name[s];
        u64 lo = 0, hi = L;
        while (lo < hi) { const u64 mid = lo + ((hi - lo) >> 1); u64 fx, fy; link_fields(lk, mid, fx, fy); if (fx < want) lo = mid + 1; else hi = mid; }
        link_first[s] = lo;
        segment_off[s] = segment_first_base(line_off[1 + s], name[s]);
    }
}
// the 32-bit names and twins as the 64-bit arrays of the interface (all-ones: no twin)
__global__ __launch_bounds__(BLOCK) void strand_widen_kernel(u64 n, const u32* __restrict__ in, u64* __restrict__ out) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK) { const u32 v = in[i]; out[i] = v == NONE ? ~0ull : (u64)v; }
}

// The line description of the merged text (write_line_tile of gfa_image.h): line 0 the header, line 1 + s representative name[s] --
// S lines exist for representatives only, carry two more tags where there is a twin --, line 1 + S + l link l, its two names and
// orientation bytes out of its key
struct StrandLines {
    u32 k, S; const u32 *weight, *kmers; const u64* label_off; const uint8_t* label; const u32 *name, *twin; const u64* segment_off; LinkKeys lk;
    __device__ __forceinline__ bool before_links(u32 r) const { return r <= S; }
    __device__ __forceinline__ void format(uint8_t* img, u32 r, u64 o, int64_t rel, int64_t end, int len) const {
        if (r == 0) {
            put_header_line(img, rel, end, len);
        } else if (r > S) {
            u64 fx, fy;
            link_fields(lk, r - 1 - S, fx, fy);
            put_link_line(img, end, len, (u32)(fx >> 1), (fx & 1) ? '-' : '+', (u32)(fy >> 1), (fy & 1) ? '-' : '+', k - 1);
        } else {
            const u32 i = name[r - 1];
            put_segment_name<S_NAME_MAX>(img, rel, len, (int)(segment_off[r - 1] - o), i);
            if (end - (S_TAGS_MAX + TWIN_TAGS_MAX) < len) {
                const u32 w = weight[i], km = kmers[i], t = twin[i];
                put_segment_tags(img, end, len, km + k - 1, (u64)w * km, w, [&](int p) {
                    if (t != NONE) {
                        p = put_tag_back<6>(img, put_decimal_back(img, p, len, weight[t]), len, tag('\t', 'r', 'w', ':', 'i', ':'));
                        p = put_tag_back<6>(img, put_decimal_back(img, p, len, t), len, tag('\t', 'r', 'c', ':', 'i', ':'));
                    }
                    return p;
                });
            }
        }
    }
    __device__ __forceinline__ Line line(u32 r, const u64* __restrict__ line_off) const {
        Line ln = line_without_bases(line_off, r, label);
        if (r >= 1 && r <= S) add_bases(ln, label, label_off, name[r - 1], (u32)(segment_off[r - 1] - line_off[r]));
        return ln;
    }
};

__global__ __launch_bounds__(BLOCK) void gfa_strands_write_kernel(u32 k, u32 S, u32 R, const u32* __restrict__ weight, const u32* __restrict__ kmers,
                                                                  const u64* __restrict__ label_off, const uint8_t* __restrict__ label, const u32* __restrict__ name,
                                                                  const u32* __restrict__ twin, const u64* __restrict__ line_off, const u64* __restrict__ segment_off,
                                                                  const LinkKeys lk, u64 total, uint8_t* __restrict__ text) {
    const StrandLines d{k, S, weight, kmers, label_off, label, name, twin, segment_off, lk};
    for (u64 base = (u64)blockIdx.x * TILE; base < total; base += (u64)gridDim.x * TILE) {
        const int len = tile_len(base, total);
        write_line_tile(d, R, workgroup_search(line_off, R, base), workgroup_search(line_off, R, base + len - 1), base, len, line_off, total, text);
    }
}

template <int NW>
int find_candidates(const GfaGraph& g, u32* cand, hipStream_t stream) {
    const u64 E = g.n_edges;
    const dim3 blk(BLOCK), grid(grid_for(E, BLOCK, 256u * 32u));
    DevBuf first_key(stream), probe(stream), order(stream), where(stream);
    KCHECK(first_key.alloc(E * 8 * NW + 16)); KCHECK(probe.alloc(E * 8 * NW + 16)); KCHECK(order.alloc(E * 4 + 16)); KCHECK(where.alloc(16));
    KCHECK_HIP(hipMemsetAsync(where.p, 0xFF, 4, stream));
    u32 at = NONE;
    {
        KernelScope ks(K_GFAS_KEYS, stream, E);
        hipLaunchKernelGGL(strand_keys_kernel<NW>, grid, blk, 0, stream, g.k, E, g.edge_kmers, g.label_off, g.label, first_key.as<u64>(), probe.as<u64>(), order.as<u32>());
        KCHECK_HIP(hipGetLastError());
        KCHECK(dev_sort(first_key.as<u64>(), order.as<u32>(), E, NW, 2 * g.k, stream));
        hipLaunchKernelGGL(strand_equal_keys_kernel<NW>, grid, blk, 0, stream, first_key.as<u64>(), E, where.as<u32>());
        KCHECK_HIP(hipGetLastError());
        KCHECK_HIP(hipMemcpyAsync(&at, where.p, 4, hipMemcpyDeviceToHost, stream));
    }
    KCHECK_HIP(hipStreamSynchronize(stream));
    if (at != NONE) {
        u32 pair[2] = {0, 0};
        KCHECK_HIP(hipMemcpyAsync(pair, order.as<u32>() + at - 1, 8, hipMemcpyDeviceToHost, stream));
        KCHECK_HIP(hipStreamSynchronize(stream));
        set_error("gfa_strands: segments %u and %u start with the same k-mer (a k-mer lies on one merged edge of a shrink result)", std::min(pair[0], pair[1]),
                  std::max(pair[0], pair[1]));
        return KATOME_E_ARG;
    }
    KernelScope ks(K_GFAS_SEARCH, stream, E);
    u32 B = 1;                                                               // (dev_rank's choice: about 16 keys to a bucket)
    while ((2ull << B) <= E / 8 && B < 27) ++B;
    if (B > 2 * g.k) B = 2 * g.k;
    DevBuf index(stream);
    KCHECK(index.alloc(((1ull << B) + 2) * 8));
    KCHECK(dev_bucket_index(first_key.as<u64>(), E, NW, 2 * g.k, B, index.as<u64>(), stream));
    hipLaunchKernelGGL(strand_search_kernel<NW>, grid, blk, 0, stream, E, 2 * g.k, B, index.as<u64>(), first_key.as<u64>(), order.as<u32>(), probe.as<u64>(),
                       g.edge_kmers, cand);
    KCHECK_HIP(hipGetLastError());
    return KATOME_OK;
}

}  // namespace

int dev_strand_twins(const GfaGraph& g, DevBuf& twin, bool validate, hipStream_t stream) {
    const u64 E = g.n_edges;
    if (validate) KCHECK(dev_gfa_validate(g, stream));
    const dim3 blk(BLOCK), grid(grid_for(E, BLOCK, 256u * 32u));
    twin.stream = stream;
    DevBuf cand(stream), words(stream), word_off(stream);
    KCHECK(twin.alloc(E * 4 + 16));
    if (E == 0) return KATOME_OK;
    KCHECK(cand.alloc(E * 4 + 16)); KCHECK(words.alloc(E * 4 + 16)); KCHECK(word_off.alloc((E + 1) * 8));
    if (2 * g.k <= 64) KCHECK(find_candidates<1>(g, cand.as<u32>(), stream));
    else KCHECK(find_candidates<2>(g, cand.as<u32>(), stream));
    u64 W = 0;
    KernelScope ks(K_GFAS_VERIFY, stream, E);
    hipLaunchKernelGGL(strand_pair_kernel, grid, blk, 0, stream, g.k, E, cand.as<u32>(), g.edge_kmers, twin.as<u32>(), words.as<u32>());
    KCHECK_HIP(hipGetLastError());
    KCHECK(dev_scan_counts(words.as<u32>(), E, word_off.as<u64>(), stream));
    KCHECK_HIP(hipMemcpyAsync(&W, word_off.as<u64>() + E, 8, hipMemcpyDeviceToHost, stream));
    KCHECK_HIP(hipStreamSynchronize(stream));
    if (W) {
        hipLaunchKernelGGL(strand_verify_kernel, dim3(grid_for((W + VERIFY_TILE - 1) / VERIFY_TILE, 1, 256u * 32u)), blk, 0, stream, g.k, (u32)E, W, word_off.as<u64>(),
                           cand.as<u32>(), g.edge_kmers, g.label_off, g.label, twin.as<u32>());
        KCHECK_HIP(hipGetLastError());
    }
    return KATOME_OK;
}

int dev_gfa_strands_plan(const GfaGraph& g, GfaStrandsPlan& plan, hipStream_t stream) {
    plan.n_segments = plan.n_links = plan.text_bytes = plan.n_unpaired = plan.n_self_twins = 0;
    const u64 E = g.n_edges;
    GfaPlan join;                                        // validates everything read through below; every (a, b) with edge_dst[a] == edge_src[b]
    KCHECK(dev_gfa_plan(g, join, stream));
    join.line_off.release(); join.segment_off.release(); join.link_first.release();
    const u64 L_in = join.n_links;
    const dim3 blk(BLOCK), grid(grid_for(E, BLOCK, 256u * 32u));
    plan.line_off.stream = plan.segment_off.stream = plan.link_first.stream = plan.name.stream = plan.twin.stream = plan.link_keys.stream = stream;
    DevBuf words(stream), word_off(stream), count(stream), seg_size(stream), size(stream);
    KCHECK(dev_strand_twins(g, plan.twin, false, stream));
    KCHECK(words.alloc(E * 4 + 16)); KCHECK(word_off.alloc((E + 1) * 8)); KCHECK(count.alloc(16));
    KCHECK_HIP(hipMemsetAsync(count.p, 0, 16, stream));
    u64 S = 0;
    if (E) {
        KernelScope ks(K_GFAS_SIZES, stream, E);
        // (words and word_off hold the representatives' flags and their scan)
        hipLaunchKernelGGL(strand_rep_kernel, grid, blk, 0, stream, E, plan.twin.as<u32>(), words.as<u32>(), count.as<unsigned long long>());
        KCHECK_HIP(hipGetLastError());
        KCHECK(dev_scan_counts(words.as<u32>(), E, word_off.as<u64>(), stream));
        u64 counted[2] = {0, 0};
        KCHECK_HIP(hipMemcpyAsync(&S, word_off.as<u64>() + E, 8, hipMemcpyDeviceToHost, stream));
        KCHECK_HIP(hipMemcpyAsync(counted, count.p, 16, hipMemcpyDeviceToHost, stream));
        KCHECK_HIP(hipStreamSynchronize(stream));
        plan.n_unpaired = counted[0]; plan.n_self_twins = counted[1];
    }
    KCHECK(plan.name.alloc(S * 4 + 16)); KCHECK(seg_size.alloc((S + 1) * 4));
    {
        KernelScope ks(K_GFAS_SIZES, stream, E);
        hipLaunchKernelGGL(strand_segment_kernel, grid, blk, 0, stream, g.k, E, plan.twin.as<u32>(), word_off.as<u64>(), g.edge_weight, g.edge_kmers, plan.name.as<u32>(),
                           seg_size.as<u32>());
        KCHECK_HIP(hipGetLastError());
    }
    words.release(); word_off.release();
    // the links: one key per (a, b), the distinct ones in ascending order
    u32 seg_bits = 1;
    while (seg_bits < 32 && ((E ? E - 1 : 0) >> seg_bits) != 0) ++seg_bits;
    plan.field_bits = seg_bits + 1;
    plan.key_words = 2 * plan.field_bits <= 64 ? 1 : 2;
    u64 L = 0;
    if (L_in) {
        KernelScope ks(K_GFAS_LINKS, stream, L_in);
        KCHECK(plan.link_keys.alloc(L_in * 8 * plan.key_words + 16));
        hipLaunchKernelGGL(strand_link_kernel, dim3(grid_for(L_in, BLOCK, 256u * 32u)), blk, 0, stream, L_in, join.link_ab.as<u32>(), plan.twin.as<u32>(),
                           plan.link_keys.as<u64>(), plan.key_words, plan.field_bits);
        KCHECK_HIP(hipGetLastError());
        join.link_ab.release();
        KCHECK(dev_sort(plan.link_keys.as<u64>(), nullptr, L_in, plan.key_words, plan.key_words == 1 ? 2 * plan.field_bits : 64 + plan.field_bits, stream));
        KCHECK(dev_unique(plan.link_keys.as<u64>(), L_in, plan.key_words, &L, stream));
        KCHECK_HIP(hipStreamSynchronize(stream));
    }
    const u64 R = 1 + S + L;
    const LinkKeys lk{plan.link_keys.as<u64>(), plan.key_words, plan.field_bits};
    KCHECK(size.alloc(R * 4)); KCHECK(plan.line_off.alloc((R + 1) * 8)); KCHECK(plan.segment_off.alloc(S * 8 + 16)); KCHECK(plan.link_first.alloc((S + 1) * 8));
    {
        KernelScope ks(K_GFAS_SIZES, stream, R);
        KCHECK_HIP(hipMemcpyAsync(size.p, seg_size.p, (S + 1) * 4, hipMemcpyDeviceToDevice, stream));
        if (L) {
            hipLaunchKernelGGL(strand_link_size_kernel, dim3(grid_for(L, BLOCK, 256u * 32u)), blk, 0, stream, L, host_digits(g.k - 1), lk, size.as<u32>() + 1 + S);
            KCHECK_HIP(hipGetLastError());
        }
        KCHECK(dev_scan_counts(size.as<u32>(), R, plan.line_off.as<u64>(), stream));
        hipLaunchKernelGGL(strand_segment_off_kernel, dim3(grid_for(S + 1, BLOCK, 256u * 32u)), blk, 0, stream, S, L, plan.name.as<u32>(), lk, plan.line_off.as<u64>(),
                           plan.segment_off.as<u64>(), plan.link_first.as<u64>());
        KCHECK_HIP(hipGetLastError());
    }
    KCHECK_HIP(hipMemcpyAsync(&plan.text_bytes, plan.line_off.as<u64>() + R, 8, hipMemcpyDeviceToHost, stream));
    KCHECK_HIP(hipStreamSynchronize(stream));
    plan.n_segments = S; plan.n_links = L;
    return KATOME_OK;
}

int dev_gfa_strands_write(const GfaGraph& g, const GfaStrandsPlan& plan, uint8_t* text, uint64_t* segment_name, uint64_t* edge_twin, hipStream_t stream) {
    const u64 R = 1 + plan.n_segments + plan.n_links, tiles = (plan.text_bytes + TILE - 1) / TILE;
    {
        KernelScope ks(K_GFAS_WRITE, stream, plan.text_bytes);
        hipLaunchKernelGGL(gfa_strands_write_kernel, dim3(grid_for(tiles, 1, 256u * 16u)), dim3(BLOCK), 0, stream, g.k, (u32)plan.n_segments, (u32)R, g.edge_weight, g.edge_kmers,
                           g.label_off, g.label, plan.name.as<u32>(), plan.twin.as<u32>(), plan.line_off.as<u64>(), plan.segment_off.as<u64>(),
                           LinkKeys{plan.link_keys.as<u64>(), plan.key_words, plan.field_bits}, plan.text_bytes, text);
    }
    if (plan.n_segments) hipLaunchKernelGGL(strand_widen_kernel, dim3(grid_for(plan.n_segments, BLOCK, 256u * 32u)), dim3(BLOCK), 0, stream, plan.n_segments, plan.name.as<u32>(), segment_name);
    if (g.n_edges) hipLaunchKernelGGL(strand_widen_kernel, dim3(grid_for(g.n_edges, BLOCK, 256u * 32u)), dim3(BLOCK), 0, stream, g.n_edges, plan.twin.as<u32>(), edge_twin);
    KCHECK_HIP(hipGetLastError());
    return KATOME_OK;
}

int dev_gfa_strands(const GfaGraph& g, GfaStrandsOutput& out, hipStream_t stream) {
    out.n_segments = out.n_links = out.text_bytes = out.n_unpaired = out.n_self_twins = 0;
    GfaStrandsPlan plan;
    KCHECK(dev_gfa_strands_plan(g, plan, stream));
    KCHECK(out.text.alloc((plan.text_bytes + 15) / 16 * 16 + 16, stream));
    KCHECK(out.segment_name.alloc(plan.n_segments * 8 + 16, stream)); KCHECK(out.edge_twin.alloc(g.n_edges * 8 + 16, stream));
    KCHECK(dev_gfa_strands_write(g, plan, out.text.as<uint8_t>(), out.segment_name.as<u64>(), out.edge_twin.as<u64>(), stream));
    KCHECK_HIP(hipStreamSynchronize(stream));
    out.segment_off.stream = out.link_first.stream = stream;
    out.segment_off.adopt(plan.segment_off); out.link_first.adopt(plan.link_first);
    out.n_segments = plan.n_segments; out.n_links = plan.n_links; out.text_bytes = plan.text_bytes;
    out.n_unpaired = plan.n_unpaired; out.n_self_twins = plan.n_self_twins;
    return KATOME_OK;
}

}  // namespace katome

extern "C" {

int katome_dev_contigs_gfa_strands(katome_builder* b, const katome_dev_contigs* c, katome_dev_gfa_strands* out, void* stream_) {
    if (!b || !c || !out) { set_error("null argument"); return KATOME_E_ARG; }
    hipStream_t stream = (hipStream_t)stream_;
    KCHECK_HIP(hipSetDevice(b->s.device));
    if (!is_last_shrink(b, c)) { set_error("contigs_gfa_strands: not the result of this builder's last katome_dev_shrink"); return KATOME_E_ARG; }
    memset(out, 0, sizeof *out);
    const GfaGraph g = gfa_graph_of(b->s.k, b->shrunk);
    GfaStrandsOutput& r = b->gfa_strands;
    {
        PhaseScope ps(b->prof, PH_GFA_STRANDS, stream);
        KCHECK(dev_gfa_strands(g, r, stream));
    }
    out->n_segments = r.n_segments; out->n_links = r.n_links; out->text_bytes = r.text_bytes; out->n_unpaired = r.n_unpaired; out->n_self_twins = r.n_self_twins;
    out->d_text = r.text.as<uint8_t>(); out->d_segment_name = r.segment_name.as<u64>(); out->d_segment_off = r.segment_off.as<u64>();
    out->d_link_first = r.link_first.as<u64>(); out->d_edge_twin = r.edge_twin.as<u64>();
    return KATOME_OK;
}

int katome_dev_gfa_strands_arrays(int device, uint32_t k, uint64_t n_nodes, uint64_t n_edges, const uint64_t* d_edge_src, const uint64_t* d_edge_dst,
                                  const uint32_t* d_edge_weight, const uint32_t* d_edge_kmers, const uint64_t* d_edge_label_off, const uint8_t* d_edge_label,
                                  uint64_t label_bytes, uint64_t* d_segment_name, uint64_t* d_segment_off, uint64_t* d_link_first, uint64_t* d_edge_twin,
                                  uint8_t* d_text, uint64_t text_cap, uint64_t* counts, void* stream_) {
    KCHECK(use_device(device));
    KCHECK(check_k(k));
    if (!counts) { set_error("null argument"); return KATOME_E_ARG; }
    for (int i = 0; i < 5; ++i) counts[i] = 0;
    hipStream_t stream = (hipStream_t)stream_;
    KCHECK(check_label_alignment(d_edge_label));
    const GfaGraph g{k, n_nodes, n_edges, d_edge_src, d_edge_dst, d_edge_weight, d_edge_kmers, d_edge_label_off, d_edge_label, label_bytes};
    GfaStrandsPlan plan;
    KCHECK(dev_gfa_strands_plan(g, plan, stream));
    counts[0] = plan.n_segments; counts[1] = plan.n_links; counts[2] = plan.text_bytes; counts[3] = plan.n_unpaired; counts[4] = plan.n_self_twins;
    if (!d_text) return KATOME_OK;
    if (!d_segment_name || !d_segment_off || !d_link_first || !d_edge_twin || !text_fits(plan.text_bytes, text_cap, d_text)) {
        set_error("gfa_strands: %llu bytes (rounded up to 16, 16-byte aligned) do not fit the caller's arrays", (unsigned long long)plan.text_bytes);
        return KATOME_E_ARG;
    }
    KCHECK(dev_gfa_strands_write(g, plan, d_text, d_segment_name, d_edge_twin, stream));
    if (plan.n_segments) KCHECK_HIP(hipMemcpyAsync(d_segment_off, plan.segment_off.p, plan.n_segments * 8, hipMemcpyDeviceToDevice, stream));
    KCHECK_HIP(hipMemcpyAsync(d_link_first, plan.link_first.p, (plan.n_segments + 1) * 8, hipMemcpyDeviceToDevice, stream));
    KCHECK_HIP(hipStreamSynchronize(stream));
    return KATOME_OK;
}

}  // extern "C"
