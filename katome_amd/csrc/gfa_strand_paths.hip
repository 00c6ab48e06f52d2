// gfa_strand_paths.hip -- collapse's contigs as GFA 1 P lines over the MERGED segments of the bidirected GFA (gfa_strands.hip), and every
// path's mirror (include/katome_gpu.h has the format):
//   P\tkatome_<c>\t<r0><o0>,<r1><o1>,...,<rn><on>\t*\n        run 0 of contig c
//   P\tkatome_<c>.<r>\t...\t*\n                                run r = 1, 2, ... of contig c
// A piece with shrunk edge i reads <rep i><o i> as gfa_strands.hip defines them: rep = min(i, twin i), or i without a twin; '-' only
// where twin(i) < i.  The runs are gfa_paths.hip's, decided on the two-strand arrays: merging cannot heal a seam, because the conjugate
// of a pair (x, y) is (twin y, twin x), and that pair is adjacent only if x and y were.  So dev_gfa_paths_runs gives the checks and
// the run structure unchanged (n_paths, path_contig, path_first_piece equal the two-strand result's); only a piece's bytes differ.
//   The plan: strand_piece_kernel maps every piece ONCE into its oriented name rep << 1 | (o == '-') -- the one random read of the
//   twin map per piece: sizing needs the digits of rep anyway -- and counts its bytes, "<rep><o>," or, on a run's last piece,
//   "<rep><o>\t*\n", behind the line's head on its first; dev_gfa_paths_offsets scans them into 64-bit byte offsets.
//   gfa_strand_paths_write_kernel loops over the tile both path texts share (write_piece_tile of gfa_path_lines.h) with this text's name
//   of a piece: the halves of its oriented name.  It reads the names in order: no twin lookup, no 64-bit shift by a variable amount.
//   Mirrors.  mirror(j) = the smallest q with as many pieces as j and id_q[t] == twin(id_j[n - 1 - t]) for every t; a piece without a
//   twin matches nothing.  Partitioned by PIECES throughout (one path can be 10^6 pieces and the next 10^6 paths one piece each):
//   mirror_sig_kernel gives every path two 64-bit signatures, the sum over its pieces of hash(id, t) and of hash(twin id, n - 1 - t) --
//   a segmented sum inside each wave, one atomic add per wave and path; sums commute, so the result does not depend on the order --,
//   dev_sort orders the forward signatures with the path as value (stable: equal signatures ascend by path), mirror_search_kernel
//   finds the first forward signature equal to a path's mirror signature, and mirror_verify_kernel compares the candidate piece for
//   piece.  A signature only nominates: a candidate that fails makes mirror_settle_kernel move on to the next equal signature, and
//   the rounds repeat until no path is pending.  Identical paths have identical signatures and all verify, so the first candidate --
//   the smallest path -- is the answer; a round after the first needs two different paths with one 64-bit signature.
#include "builder.h"
#include "gfa_path_lines.h"
#include "strand_bits.h"

namespace katome {
namespace {

constexpr u32 WHOLE = KATOME_PIECE_WHOLE;
constexpr u32 NONE = NO_TWIN;
static_assert(PIECE_MIN == 3, "\"0+,\" and \"0-,\" are the shortest pieces: MAX_PIECES holds for the merged names");
enum { ERR_TWIN = 1, ERR_INVOLUTION = 2 };

// the caller's twin map (64-bit, all ones: none) as the 32-bit one, checked: an entry is all ones or below E, and names its edge back
__global__ __launch_bounds__(BLOCK) void strand_twin_check_kernel(u64 E, const u64* __restrict__ twin64, u32* __restrict__ twin, u32* __restrict__ err) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < E; i += (u64)gridDim.x * BLOCK) {
        const u64 t = twin64[i];
        twin[i] = NONE;
        if (t == ~0ull) continue;
        if (t >= E) { atomicOr(err, (u32)ERR_TWIN); continue; }
        if (twin64[t] != i) { atomicOr(err, (u32)ERR_INVOLUTION); continue; }
        twin[i] = (u32)t;
    }
}

// piece p (checked by dev_gfa_paths_runs): its oriented name and its bytes
__global__ __launch_bounds__(BLOCK) void strand_piece_kernel(const u32* __restrict__ pieces, u64 P, const u32* __restrict__ twin, const u64* __restrict__ path_idx,
                                                             const u64* __restrict__ path_contig, const u64* __restrict__ contig_first_path,
                                                             u32* __restrict__ oname, u32* __restrict__ size) {
    for (u64 p = (u64)blockIdx.x * BLOCK + threadIdx.x; p < P; p += (u64)gridDim.x * BLOCK) {
        const u32 id = pieces[p] & ~WHOLE, t = twin[id];
        const u32 minus = t < id ? 1u : 0u, rep = minus ? t : id;      // (NONE is above every id; a self-twin stays at +)
        oname[p] = rep << 1 | minus;
        u32 n = decimal_digits(rep) + 2;                               // "<rep><o>,"
        const u64 path = path_idx[p];
        if (path_idx[p + 1] != path) { const u64 c = path_contig[path]; n += run_head_bytes(c, path - contig_first_path[c]); }
        if (p + 1 == P || path_idx[p + 2] != path_idx[p + 1]) n += 2;  // "<rep><o>\t*\n"
        size[p] = n;
    }
}

__global__ __launch_bounds__(BLOCK) void gfa_strand_paths_write_kernel(const u32* __restrict__ oname, u32 P, const u64* __restrict__ path_idx,
                                                                       const u64* __restrict__ piece_off, const u64* __restrict__ path_contig,
                                                                       const u64* __restrict__ contig_first_path, u64 total, uint8_t* __restrict__ text) {
    const auto name = [=](u32 p) { const u32 on = oname[p]; return PieceName{on >> 1, (on & 1) ? '-' : '+'}; };
    for (u64 base = (u64)blockIdx.x * TILE; base < total; base += (u64)gridDim.x * TILE) {
        const int len = tile_len(base, total);
        write_piece_tile(name, P, workgroup_search(piece_off, P, base), workgroup_search(piece_off, P, base + len - 1), base, len, path_idx, piece_off, path_contig,
                         contig_first_path, total, text);
    }
}

// ---- mirrors -----------------------------------------------------------------------------------------------------------------------
// piece p lies in path path_idx[p + 1] - 1 (path_idx is the EXCLUSIVE scan of the run flags), at place p - path_first_piece[path]
__device__ __forceinline__ u64 piece_hash(u32 id, u32 place) {         // (splitmix64's finalizer on the pair)
    u64 z = ((u64)id << 32 | place) + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// fwd[j] += hash(id, t), mir[j] += hash(twin id, n - 1 - t) over the pieces of path j; cand[j] = 1 where a piece has no twin (fwd, mir
// and cand zeroed by the caller).  A wave owns 64 consecutive pieces: their paths ascend, so a segmented sum leaves one add per path
__global__ __launch_bounds__(BLOCK) void mirror_sig_kernel(const u32* __restrict__ pieces, u64 P, const u32* __restrict__ twin, const u64* __restrict__ path_idx,
                                                           const u64* __restrict__ first, unsigned long long* __restrict__ fwd,
                                                           unsigned long long* __restrict__ mir, u32* __restrict__ cand) {
    const u32 lane = threadIdx.x & 63;
    for (u64 base = (u64)blockIdx.x * BLOCK + (threadIdx.x - lane); base < P; base += (u64)gridDim.x * BLOCK) {      // (the whole wave stays in the loop)
        const u64 p = base + lane;
        const bool in = p < P;
        unsigned long long path = ~0ull, f = 0, m = 0;
        if (in) {
            path = path_idx[p + 1] - 1;
            const u64 lo = first[path], n = first[path + 1] - lo;
            const u32 id = pieces[p] & ~WHOLE, tw = twin[id], t = (u32)(p - lo);
            f = piece_hash(id, t);
            if (tw == NONE) cand[path] = 1;
            else m = piece_hash(tw, (u32)(n - 1) - t);
        }
#pragma unroll
        for (u32 d = 1; d < 64; d <<= 1) {
            const unsigned long long pk = __shfl_up(path, d, 64), pf = __shfl_up(f, d, 64), pm = __shfl_up(m, d, 64);
            if (lane >= d && pk == path) { f += pf; m += pm; }
        }
        const unsigned long long next = __shfl_down(path, 1, 64);
        if (in && (lane == 63 || next != path)) { atomicAdd(&fwd[path], f); atomicAdd(&mir[path], m); }
    }
}

// path j: mirror[j] = none; cand[j] = the first place in the sorted forward signatures that holds j's mirror signature, or NONE
// (count[0]: the paths that have a candidate)
__global__ __launch_bounds__(BLOCK) void mirror_search_kernel(u64 n, const u64* __restrict__ sorted, const u64* __restrict__ mir, u32* __restrict__ cand,
                                                              u64* __restrict__ mirror, unsigned long long* __restrict__ count) {
    u32 found = 0;
    for (u64 j = (u64)blockIdx.x * BLOCK + threadIdx.x; j < n; j += (u64)gridDim.x * BLOCK) {
        mirror[j] = ~0ull;
        u32 c = NONE;
        if (!cand[j]) {                                                // (1: a piece without a twin)
            const u64 q = mir[j];
            u64 lo = 0, hi = n;                                        // the first signature that is not below q
            while (lo < hi) { const u64 mid = lo + ((hi - lo) >> 1); if (sorted[mid] < q) lo = mid + 1; else hi = mid; }
            if (lo < n && sorted[lo] == q) { c = (u32)lo; ++found; }
        }
        cand[j] = c;
    }
    found = wave_sum(found);
    if ((threadIdx.x & 63) == 0 && found) atomicAdd(&count[0], (unsigned long long)found);
}

// piece p of a path j with a candidate q = order[cand[j]]: fail[j] = 1 unless q has j's length and its piece n - 1 - t is twin(id(p))
__global__ __launch_bounds__(BLOCK) void mirror_verify_kernel(const u32* __restrict__ pieces, u64 P, const u32* __restrict__ twin, const u64* __restrict__ path_idx,
                                                              const u64* __restrict__ first, const u32* __restrict__ order, const u32* __restrict__ cand,
                                                              u32* __restrict__ fail) {
    for (u64 p = (u64)blockIdx.x * BLOCK + threadIdx.x; p < P; p += (u64)gridDim.x * BLOCK) {
        const u64 path = path_idx[p + 1] - 1;
        const u32 at = cand[path];
        if (at == NONE) continue;
        const u64 q = order[at], lo = first[path], n = first[path + 1] - lo, q_lo = first[q];
        if (first[q + 1] - q_lo != n) { fail[path] = 1; continue; }
        if ((pieces[q_lo + (n - 1 - (p - lo))] & ~WHOLE) != twin[pieces[p] & ~WHOLE]) fail[path] = 1;
    }
}

// path j with a candidate: verified -- it is the mirror --, or on to the next equal signature, if there is one (count[0]: still pending)
__global__ __launch_bounds__(BLOCK) void mirror_settle_kernel(u64 n, const u64* __restrict__ sorted, const u32* __restrict__ order, const u64* __restrict__ mir,
                                                              u32* __restrict__ cand, u32* __restrict__ fail, u64* __restrict__ mirror,
                                                              unsigned long long* __restrict__ count) {
    u32 pending = 0;
    for (u64 j = (u64)blockIdx.x * BLOCK + threadIdx.x; j < n; j += (u64)gridDim.x * BLOCK) {
        const u32 at = cand[j];
        if (at == NONE) continue;
        u32 next = NONE;
        if (!fail[j]) mirror[j] = order[at];
        else if ((u64)at + 1 < n && sorted[at + 1] == mir[j]) { next = at + 1; ++pending; }
        cand[j] = next; fail[j] = 0;
    }
    pending = wave_sum(pending);
    if ((threadIdx.x & 63) == 0 && pending) atomicAdd(&count[0], (unsigned long long)pending);
}

// count[1]: paths with a mirror; count[2]: paths that are their own
__global__ __launch_bounds__(BLOCK) void mirror_count_kernel(u64 n, const u64* __restrict__ mirror, unsigned long long* __restrict__ count) {
    u32 mirrored = 0, self = 0;
    for (u64 j = (u64)blockIdx.x * BLOCK + threadIdx.x; j < n; j += (u64)gridDim.x * BLOCK) { const u64 q = mirror[j]; mirrored += q != ~0ull; self += q == j; }
    mirrored = wave_sum(mirrored); self = wave_sum(self);
    if ((threadIdx.x & 63) == 0) { if (mirrored) atomicAdd(&count[1], (unsigned long long)mirrored); if (self) atomicAdd(&count[2], (unsigned long long)self); }
}

}  // namespace

// The mirrors of n groups of consecutive pieces -- the paths of this file, or collapse's contigs (unique_contigs.hip): group_idx is the
// EXCLUSIVE scan of the flags that begin a group (piece p lies in group group_idx[p + 1] - 1; P + 1 entries), first every group's
// first piece (n + 1 entries).  mirror: allocated here, [n] u64.  twin is trusted; synchronises
int dev_find_mirrors(const uint32_t* pieces, uint64_t P, const uint32_t* twin, const uint64_t* path_idx, const uint64_t* first, uint64_t n, DevBuf& mirror,
                     uint64_t* n_mirrored, uint64_t* n_self_mirror, hipStream_t stream) {
    *n_mirrored = *n_self_mirror = 0;
    mirror.stream = stream;
    KCHECK(mirror.alloc(n * 8));
    if (n == 0) return KATOME_OK;
    const dim3 blk(BLOCK), by_piece(grid_for(P, BLOCK, 256u * 32u)), by_path(grid_for(n, BLOCK, 256u * 32u));
    DevBuf fwd(stream), mir(stream), order(stream), cand(stream), fail(stream), count(stream);
    KCHECK(fwd.alloc(n * 8 + 16)); KCHECK(mir.alloc(n * 8)); KCHECK(order.alloc(n * 4 + 16)); KCHECK(cand.alloc(n * 4)); KCHECK(fail.alloc(n * 4)); KCHECK(count.alloc(24));
    KCHECK_HIP(hipMemsetAsync(fwd.p, 0, n * 8, stream)); KCHECK_HIP(hipMemsetAsync(mir.p, 0, n * 8, stream));
    KCHECK_HIP(hipMemsetAsync(cand.p, 0, n * 4, stream)); KCHECK_HIP(hipMemsetAsync(fail.p, 0, n * 4, stream));
    KCHECK_HIP(hipMemsetAsync(count.p, 0, 24, stream));
    {
        KernelScope ks(K_GFASP_SIGS, stream, P);
        hipLaunchKernelGGL(mirror_sig_kernel, by_piece, blk, 0, stream, pieces, P, twin, path_idx, first, fwd.as<unsigned long long>(), mir.as<unsigned long long>(),
                           cand.as<u32>());
        KCHECK_HIP(hipGetLastError());
    }
    {
        KernelScope ks(K_GFASP_SORT, stream, n);
        KCHECK(dev_iota(order.as<u32>(), n, stream));
        KCHECK(dev_sort(fwd.as<u64>(), order.as<u32>(), n, 1, 64, stream));
    }
    {
        KernelScope ks(K_GFASP_SEARCH, stream, n);
        hipLaunchKernelGGL(mirror_search_kernel, by_path, blk, 0, stream, n, fwd.as<u64>(), mir.as<u64>(), cand.as<u32>(), mirror.as<u64>(),
                           count.as<unsigned long long>());
        KCHECK_HIP(hipGetLastError());
    }
    for (;;) {                                                          // (a round per candidate of the path that needs the most: see the head of the file)
        u64 pending = 0;
        KCHECK_HIP(hipMemcpyAsync(&pending, count.p, 8, hipMemcpyDeviceToHost, stream));
        KCHECK_HIP(hipStreamSynchronize(stream));
        if (!pending) break;
        KCHECK_HIP(hipMemsetAsync(count.p, 0, 8, stream));
        KernelScope ks(K_GFASP_VERIFY, stream, P);
        hipLaunchKernelGGL(mirror_verify_kernel, by_piece, blk, 0, stream, pieces, P, twin, path_idx, first, order.as<u32>(), cand.as<u32>(), fail.as<u32>());
        hipLaunchKernelGGL(mirror_settle_kernel, by_path, blk, 0, stream, n, fwd.as<u64>(), order.as<u32>(), mir.as<u64>(), cand.as<u32>(), fail.as<u32>(),
                           mirror.as<u64>(), count.as<unsigned long long>());
        KCHECK_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(mirror_count_kernel, by_path, blk, 0, stream, n, mirror.as<u64>(), count.as<unsigned long long>());
    KCHECK_HIP(hipGetLastError());
    u64 counted[3] = {0, 0, 0};
    KCHECK_HIP(hipMemcpyAsync(counted, count.p, 24, hipMemcpyDeviceToHost, stream));
    KCHECK_HIP(hipStreamSynchronize(stream));
    *n_mirrored = counted[1]; *n_self_mirror = counted[2];
    return KATOME_OK;
}

// a caller's twin map (64-bit, all ones: none) checked on the device and narrowed to the 32-bit one; `who` begins the messages; synchronises
int dev_strand_twin_check(const char* who, uint64_t E, const uint64_t* twin64, uint32_t* twin, hipStream_t stream) {
    if (E == 0) return KATOME_OK;
    DevBuf tail(stream);
    KCHECK(tail.alloc(16));
    KCHECK_HIP(hipMemsetAsync(tail.p, 0, 16, stream));
    u32 err = 0;
    hipLaunchKernelGGL(strand_twin_check_kernel, dim3(grid_for(E, BLOCK, 256u * 32u)), dim3(BLOCK), 0, stream, E, twin64, twin, tail.as<u32>());
    KCHECK_HIP(hipGetLastError());
    KCHECK_HIP(hipMemcpyAsync(&err, tail.p, 4, hipMemcpyDeviceToHost, stream));
    KCHECK_HIP(hipStreamSynchronize(stream));
    if (err & ERR_TWIN) { set_error("%s: a twin entry is neither all ones nor below n_edges", who); return KATOME_E_ARG; }
    if (err & ERR_INVOLUTION) { set_error("%s: twin(twin(i)) != i for some edge i", who); return KATOME_E_ARG; }
    return KATOME_OK;
}

int dev_gfa_strand_paths_plan(uint64_t n_edges, const uint64_t* edge_src, const uint64_t* edge_dst, const uint32_t* twin, const uint32_t* pieces,
                              uint64_t n_pieces, GfaStrandPathsPlan& plan, hipStream_t stream) {
    const u64 P = n_pieces;
    plan.oname.stream = plan.mirror.stream = stream;
    DevBuf size(stream);
    KCHECK(dev_gfa_paths_runs(n_edges, edge_src, edge_dst, pieces, P, plan.runs, size, stream));
    if (P) {
        if (!twin) { set_error("null argument"); return KATOME_E_ARG; }
        KCHECK(plan.oname.alloc(P * 4));
        hipLaunchKernelGGL(strand_piece_kernel, dim3(grid_for(P, BLOCK, 256u * 32u)), dim3(BLOCK), 0, stream, pieces, P, twin, plan.runs.path_idx.as<u64>(),
                           plan.runs.path_contig.as<u64>(), plan.runs.contig_first_path.as<u64>(), plan.oname.as<u32>(), size.as<u32>());
        KCHECK_HIP(hipGetLastError());
        KCHECK(dev_gfa_paths_offsets(P, size.as<u32>(), plan.runs, stream));
    }
    size.release();
    return dev_find_mirrors(pieces, P, twin, plan.runs.path_idx.as<u64>(), plan.runs.path_first_piece.as<u64>(), plan.runs.n_paths, plan.mirror, &plan.n_mirrored,
                            &plan.n_self_mirror, stream);
}

int dev_gfa_strand_paths_write(uint64_t n_pieces, const GfaStrandPathsPlan& plan, uint8_t* text, hipStream_t stream) {
    const u64 total = plan.runs.text_bytes;
    if (n_pieces == 0 || total == 0) return KATOME_OK;
    const u64 tiles = (total + TILE - 1) / TILE;
    KernelScope ks(K_GFASP_WRITE, stream, total);
    hipLaunchKernelGGL(gfa_strand_paths_write_kernel, dim3(grid_for(tiles, 1, 256u * 16u)), dim3(BLOCK), 0, stream, plan.oname.as<u32>(), (u32)n_pieces,
                       plan.runs.path_idx.as<u64>(), plan.runs.piece_off.as<u64>(), plan.runs.path_contig.as<u64>(), plan.runs.contig_first_path.as<u64>(), total, text);
    KCHECK_HIP(hipGetLastError());
    return KATOME_OK;
}

}  // namespace katome

extern "C" {

int katome_dev_gfa_strand_paths_arrays(int device, uint64_t n_edges, const uint64_t* d_edge_src, const uint64_t* d_edge_dst, const uint64_t* d_edge_twin,
                                       const uint32_t* d_pieces, uint64_t n_pieces, uint64_t* d_path_line_off, uint64_t* d_path_contig,
                                       uint64_t* d_path_first_piece, uint64_t* d_path_mirror, uint64_t path_cap, uint8_t* d_text, uint64_t text_cap,
                                       uint64_t* counts, void* stream_) {
    if (!counts) { set_error("null argument"); return KATOME_E_ARG; }
    for (int i = 0; i < 5; ++i) counts[i] = 0;
    KCHECK(use_device(device));
    hipStream_t stream = (hipStream_t)stream_;
    const u64 E = n_edges;
    if (E >= 0xFFFFFFFFull) { set_error("gfa_strand_paths: %llu edges, at most 2^32 - 2", (unsigned long long)E); return KATOME_E_UNSUPPORTED; }
    if (E && !d_edge_twin) { set_error("null argument"); return KATOME_E_ARG; }
    // KATOME_GFA_STRAND_PATHS_TRACE=1: the kernels' own times on stderr (there is no builder whose profile could hold them; tools/bench_gfa_strand_paths.py)
    ArraysTrace trace("KATOME_GFA_STRAND_PATHS_TRACE", "katome_dev_gfa_strand_paths_arrays");
    GfaStrandPathsPlan plan;
    {
        PhaseScope ps(trace.prof, PH_GFA_STRAND_PATHS, stream);
        DevBuf twin(stream);
        KCHECK(twin.alloc(E * 4));
        KCHECK(dev_strand_twin_check("gfa_strand_paths", E, d_edge_twin, twin.as<u32>(), stream));
        KCHECK(dev_gfa_strand_paths_plan(E, d_edge_src, d_edge_dst, twin.as<u32>(), d_pieces, n_pieces, plan, stream));
        const GfaPathsPlan& r = plan.runs;
        counts[0] = r.n_paths; counts[1] = r.n_paths - r.n_contigs; counts[2] = r.text_bytes; counts[3] = plan.n_mirrored; counts[4] = plan.n_self_mirror;
        if (!d_text) return KATOME_OK;
        if (!d_path_line_off || !d_path_first_piece || (r.n_paths && (!d_path_contig || !d_path_mirror)) || path_cap < r.n_paths ||
            !text_fits(r.text_bytes, text_cap, d_text)) {
            set_error("gfa_strand_paths: %llu paths and %llu bytes (rounded up to 16, 16-byte aligned) do not fit the caller's arrays", (unsigned long long)r.n_paths,
                      (unsigned long long)r.text_bytes);
            return KATOME_E_ARG;
        }
        KCHECK(dev_gfa_strand_paths_write(n_pieces, plan, d_text, stream));
        KCHECK_HIP(hipMemcpyAsync(d_path_line_off, r.path_line_off.p, (r.n_paths + 1) * 8, hipMemcpyDeviceToDevice, stream));
        KCHECK_HIP(hipMemcpyAsync(d_path_first_piece, r.path_first_piece.p, (r.n_paths + 1) * 8, hipMemcpyDeviceToDevice, stream));
        if (r.n_paths) {
            KCHECK_HIP(hipMemcpyAsync(d_path_contig, r.path_contig.p, r.n_paths * 8, hipMemcpyDeviceToDevice, stream));
            KCHECK_HIP(hipMemcpyAsync(d_path_mirror, plan.mirror.p, r.n_paths * 8, hipMemcpyDeviceToDevice, stream));
        }
    }
    KCHECK_HIP(hipStreamSynchronize(stream));
    trace.print(K_GFASP_WRITE, K_GFASP_VERIFY, plan.runs.text_bytes, n_pieces, "pieces", plan.runs.n_paths, "paths");
    return KATOME_OK;
}

// the whole text for the builder's last katome_dev_collapse: the bidirected GFA of the shrunk graph its pieces name (gfa_strands.hip), then
// the paths over its merged segments
int katome_dev_collapse_gfa_strands(katome_builder* b, katome_dev_gfa_strand_paths* out, void* stream_) {
    if (!b || !out) { set_error("null argument"); return KATOME_E_ARG; }
    hipStream_t stream = (hipStream_t)stream_;
    KCHECK_HIP(hipSetDevice(b->s.device));
    memset(out, 0, sizeof *out);
    if (!b->collapse_valid) { set_error("collapse_gfa_strands: no collapse result"); return KATOME_E_ARG; }
    const ShrinkOutput& sh = b->collapse_shrunk;
    const GfaGraph g = gfa_graph_of(b->s.k, sh);
    GfaStrandPathsOutput& o = b->gfa_strand_paths;
    o.n_segments = o.n_links = o.text_bytes = o.n_unpaired = o.n_self_twins = o.n_paths = o.n_jumps = o.path_bytes = o.n_mirrored = o.n_self_mirror = 0;
    {
        PhaseScope ps(b->prof, PH_GFA_STRAND_PATHS, stream);
        GfaStrandsPlan plan;
        GfaStrandPathsPlan paths;
        KCHECK(dev_gfa_strands_plan(g, plan, stream));
        KCHECK(dev_gfa_strand_paths_plan(sh.n_edges, g.edge_src, g.edge_dst, plan.twin.as<u32>(), b->collapse_pieces.as<u32>(), b->collapse_n_pieces, paths, stream));
        const u64 path_at = (plan.text_bytes + 15) / 16 * 16;
        KCHECK(o.text.alloc(path_at + (paths.runs.text_bytes + 15) / 16 * 16 + 16, stream));
        KCHECK(o.segment_name.alloc(plan.n_segments * 8 + 16, stream)); KCHECK(o.edge_twin.alloc(sh.n_edges * 8 + 16, stream));
        KCHECK(dev_gfa_strands_write(g, plan, o.text.as<uint8_t>(), o.segment_name.as<u64>(), o.edge_twin.as<u64>(), stream));
        KCHECK(dev_gfa_strand_paths_write(b->collapse_n_pieces, paths, o.text.as<uint8_t>() + path_at, stream));
        KCHECK_HIP(hipStreamSynchronize(stream));
        o.segment_off.stream = o.link_first.stream = o.path_line_off.stream = o.path_contig.stream = o.path_first_piece.stream = o.path_mirror.stream = stream;
        o.segment_off.adopt(plan.segment_off); o.link_first.adopt(plan.link_first);
        o.path_line_off.adopt(paths.runs.path_line_off); o.path_contig.adopt(paths.runs.path_contig); o.path_first_piece.adopt(paths.runs.path_first_piece);
        o.path_mirror.adopt(paths.mirror);
        o.n_segments = plan.n_segments; o.n_links = plan.n_links; o.text_bytes = plan.text_bytes; o.n_unpaired = plan.n_unpaired; o.n_self_twins = plan.n_self_twins;
        o.n_paths = paths.runs.n_paths; o.n_jumps = paths.runs.n_paths - paths.runs.n_contigs; o.path_bytes = paths.runs.text_bytes;
        o.n_mirrored = paths.n_mirrored; o.n_self_mirror = paths.n_self_mirror;
    }
    out->n_segments = o.n_segments; out->n_links = o.n_links; out->text_bytes = o.text_bytes; out->n_unpaired = o.n_unpaired; out->n_self_twins = o.n_self_twins;
    out->d_text = o.text.as<uint8_t>(); out->d_segment_name = o.segment_name.as<u64>(); out->d_segment_off = o.segment_off.as<u64>();
    out->d_link_first = o.link_first.as<u64>(); out->d_edge_twin = o.edge_twin.as<u64>();
    out->n_paths = o.n_paths; out->n_jumps = o.n_jumps; out->path_bytes = o.path_bytes;
    out->d_path_text = o.text.as<uint8_t>() + (o.text_bytes + 15) / 16 * 16;
    out->d_path_line_off = o.path_line_off.as<u64>(); out->d_path_contig = o.path_contig.as<u64>(); out->d_path_first_piece = o.path_first_piece.as<u64>();
    out->n_mirrored = o.n_mirrored; out->n_self_mirror = o.n_self_mirror; out->d_path_mirror = o.path_mirror.as<u64>();
    out->n_edges = sh.n_edges;
    return KATOME_OK;
}

}  // extern "C"
