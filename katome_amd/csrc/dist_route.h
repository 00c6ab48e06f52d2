// dist_route.h -- what the stages on the sharded graph (dist_prune.hip, dist_stages.hip) share: launch helpers, appends of
// a wave / a workgroup to one cursor, and the Router, which sends records to the rank named in their top byte and answers
// them over the mirrored exchange.  Everything is internal to the file that includes it.
#pragma once
#include <chrono>
#include <cstring>

#include "dist_builder.h"

namespace {

// whole waves stay in the loop together (wave_append votes)
#define WLOOP(i, n) for (u64 i##0 = (u64)blockIdx.x * BLOCK, i = i##0 + threadIdx.x; i##0 < (n); i##0 += (u64)gridDim.x * BLOCK, i = i##0 + threadIdx.x)

constexpr u64 NONE64 = ~0ull;
constexpr u32 NONE32 = 0xFFFFFFFFu;
constexpr u64 LOW56 = (1ull << 56) - 1;

__device__ __forceinline__ u64 wave_append(bool have, unsigned long long* cursor) {
    const u64 mask = __ballot(have);
    if (!mask) return 0;
    const u32 lane = threadIdx.x & 63;
    u64 base = 0;
    const int leader = __ffsll((unsigned long long)mask) - 1;
    if ((int)lane == leader) base = atomicAdd(cursor, (unsigned long long)__popcll(mask));
    base = __shfl(base, leader, 64);
    return base + __popcll(mask & (lane ? (~0ull >> (64 - lane)) : 0ull));
}

// The same for a whole workgroup and CA_ITEMS items per thread: ONE cursor atomic per 2048 items.  (A million waves adding to one
// address take milliseconds -- same-address atomics serialise --, which is what the kernels that look at every edge or node
// of the rank cost while they appended wave by wave: 4-8 ms each per pass, measured, for 0.3 ms of memory traffic.)
// Every thread of the workgroup calls it, the same number of times; returns where this thread's first item goes.
constexpr int CA_ITEMS = 8;
__device__ __forceinline__ u64 block_append(u32 mine, unsigned long long* cursor) {
    __shared__ u32 ca_wtot[BLOCK / 64];
    __shared__ unsigned long long ca_base;
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u32 incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const u32 v = __shfl_up(incl, o, 64); if (lane >= (u32)o) incl += v; }
    __syncthreads();                                         // (the previous call's readers are done with the shared words)
    if (lane == 63) ca_wtot[wave] = incl;
    __syncthreads();
    u32 woff = 0, total = 0;
#pragma unroll
    for (int w = 0; w < BLOCK / 64; ++w) { if (w < (int)wave) woff += ca_wtot[w]; total += ca_wtot[w]; }
    if (threadIdx.x == 0) ca_base = total ? atomicAdd(cursor, (unsigned long long)total) : 0ull;
    __syncthreads();
    return ca_base + woff + (incl - mine);
}
#define TLOOP(t0, n) for (u64 t0 = (u64)blockIdx.x * BLOCK * CA_ITEMS; t0 < (n); t0 += (u64)gridDim.x * BLOCK * CA_ITEMS)
#define KLAUNCH_T(kernel, n, stream, ...) hipLaunchKernelGGL(kernel, dim3(grid_for((n), BLOCK * CA_ITEMS, 256u * 16u)), dim3(BLOCK), 0, stream, __VA_ARGS__)
__global__ __launch_bounds__(BLOCK) void narrow_kernel(const u64* __restrict__ in, u64 n, u32* __restrict__ out) { WLOOP(i, n) if (i < n) out[i] = (u32)in[i]; }
__global__ __launch_bounds__(BLOCK) void widen_kernel(const u32* __restrict__ in, u64 n, u64* __restrict__ out) { WLOOP(i, n) if (i < n) out[i] = in[i]; }
__global__ __launch_bounds__(BLOCK) void iota32_kernel(u32* __restrict__ out, u64 n) { WLOOP(i, n) if (i < n) out[i] = (u32)i; }
// ---- the result -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void alive_list_kernel(const unsigned char* __restrict__ alive, u64 n, u32* __restrict__ out, unsigned long long* cursor) {
    TLOOP(t0, n) {
        u32 mine = 0, have = 0;
#pragma unroll
        for (int k = 0; k < CA_ITEMS; ++k) {
            const u64 i = t0 + (u64)k * BLOCK + threadIdx.x;
            if (i < n && alive[i]) { have |= 1u << k; ++mine; }
        }
        u64 at = block_append(mine, cursor);
#pragma unroll
        for (int k = 0; k < CA_ITEMS; ++k) if (have & (1u << k)) out[at++] = (u32)(t0 + (u64)k * BLOCK + threadIdx.x);
    }
}
__global__ __launch_bounds__(BLOCK) void scatter_by_idx_kernel(const u64* __restrict__ vals, const u32* __restrict__ at, u64 n, u64* __restrict__ out) {
    WLOOP(i, n) if (i < n) out[at[i]] = vals[i];
}
// ... records of `words` u64 each (Router::reply with a width)
__global__ __launch_bounds__(BLOCK) void scatter_wide_by_idx_kernel(const u64* __restrict__ vals, const u32* __restrict__ at, u64 n, u32 words, u64* __restrict__ out) {
    WLOOP(i, n) if (i < n) for (u32 q = 0; q < words; ++q) out[(u64)at[i] * words + q] = vals[i * words + q];
}
template <class T>
__global__ __launch_bounds__(BLOCK) void gather_by_kernel(const T* __restrict__ src, const u32* __restrict__ keep, u64 n, T* __restrict__ out) {
    WLOOP(i, n) if (i < n) out[i] = src[keep[i]];
}
template <int NW>
__global__ __launch_bounds__(BLOCK) void gather_keys_by_kernel(const u64* __restrict__ src, const u32* __restrict__ keep, u64 n, u64* __restrict__ out) {
    WLOOP(i, n) if (i < n) {
#pragma unroll
        for (int q = 0; q < NW; ++q) out[i * NW + q] = src[(u64)keep[i] * NW + q];
    }
}

// two columns as one 16-byte record per element (one exchange instead of two), and back
__global__ __launch_bounds__(BLOCK) void zip2_kernel(const u64* __restrict__ pa, const u64* __restrict__ B, const u32* __restrict__ pidx, u64 n, u64* __restrict__ out) {
    WLOOP(i, n) if (i < n) { out[2 * i] = pa[i]; out[2 * i + 1] = B[pidx[i]]; }
}
__global__ __launch_bounds__(BLOCK) void unzip2_kernel(const u64* __restrict__ in, u64 n, u64* __restrict__ a, u64* __restrict__ b) {
    WLOOP(i, n) if (i < n) { a[i] = in[2 * i]; b[i] = in[2 * i + 1]; }
}
// records with their destination rank in the top byte of column A [and a second column] -> their destinations
struct Routed {
    DevBuf a, b, pidx;
    std::vector<uint64_t> counts, rcnt;
    uint64_t n = 0, n_sent = 0, pair_max = 0;      // pair_max: the largest (rank -> peer) count of the whole exchange
    uint64_t moved = 0;                            // records on the move between ANY two ranks in this exchange
    explicit Routed(hipStream_t s) : a(s), b(s), pidx(s) {}
};
struct Router {
    katome_dist_builder* d; hipStream_t stream; DevBuf bounds;
    double t_part = 0, t_counts = 0, t_xchg = 0, t_gather = 0; uint64_t n_send = 0, n_reply = 0;      // host wall time per kind of step (KATOME_DIST_PRUNE_TRACE)
    Router(katome_dist_builder* d_, hipStream_t s) : d(d_), stream(s), bounds(s) {}
    int init() {
        const int world = d->world();
        std::vector<uint64_t> h(std::max(world - 1, 1), ~0ull);
        for (int p = 0; p + 1 < world; ++p) h[p] = (uint64_t)(p + 1) << 56;
        KCHECK(bounds.alloc(h.size() * 8));
        KCHECK_HIP(hipMemcpyAsync(bounds.p, h.data(), h.size() * 8, hipMemcpyHostToDevice, stream));
        KCHECK_HIP(hipStreamSynchronize(stream));
        return KATOME_OK;
    }
    int send(const u64* A, const u64* B, uint64_t n, Routed& out) {
        const int world = d->world();
        out.counts.assign(world, 0); out.rcnt.assign(world, 0); out.n_sent = n;
        DevBuf idx(stream), pa(stream), zipped(stream), landed(stream);
        KCHECK(idx.alloc((n + 1) * 4)); KCHECK(pa.alloc((n + 1) * 8)); KCHECK(out.pidx.alloc((n + 1) * 4));
        ++n_send;
        double t0 = now_ms();
        if (n) {
            KCHECK(dev_iota(idx.as<u32>(), n, stream));
            KCHECK(dev_partition_range(A, idx.as<u32>(), n, bounds.as<u64>(), (uint32_t)world, pa.as<u64>(), out.pidx.as<u32>(), out.counts.data(), stream));
        }
        t_part += now_ms() - t0; t0 = now_ms();
        KCHECK(d->comm->exchange_counts(out.counts.data(), out.rcnt.data(), &out.pair_max, &out.moved));
        t_counts += now_ms() - t0; t0 = now_ms();
        out.n = 0;
        for (uint64_t c : out.rcnt) out.n += c;
        KCHECK(out.a.alloc((out.n + 1) * 8));
        if (B) KCHECK(out.b.alloc((out.n + 1) * 8));
        if (out.moved == 0) return KATOME_OK;                          // nothing travels anywhere: no exchange at all
        if (!B) {
            KCHECK(d->xchg(X_PRUNE, pa.p, out.counts.data(), out.a.p, out.rcnt.data(), 8, stream, false, out.pair_max));
        } else {                                                        // both columns in one exchange of 16-byte records
            KCHECK(zipped.alloc((n + 1) * 16)); KCHECK(landed.alloc((out.n + 1) * 16));
            if (n) KLAUNCH(zip2_kernel, n, stream, pa.as<u64>(), B, out.pidx.as<u32>(), n, zipped.as<u64>());
            KCHECK(d->xchg(X_PRUNE, zipped.p, out.counts.data(), landed.p, out.rcnt.data(), 16, stream, false, out.pair_max));
            if (out.n) KLAUNCH(unzip2_kernel, out.n, stream, landed.as<u64>(), out.n, out.a.as<u64>(), out.b.as<u64>());
            KCHECK_HIP(hipGetLastError());
        }
        KCHECK_HIP(hipStreamSynchronize(stream));
        t_xchg += now_ms() - t0;
        return KATOME_OK;
    }
    // every rank's records (n_mine elements of `elem` bytes) to every rank, in rank order: the same send buffer for all peers
    int allgather(const void* mine, uint64_t n_mine, size_t elem, DevBuf& out, uint64_t* total) {
        const int world = d->world();
        std::vector<uint64_t> all(world, 0);
        KCHECK(d->comm->allgather(n_mine, all.data()));
        uint64_t sum = 0, biggest = 0;
        std::vector<uint64_t> roff(world, 0);
        for (int p = 0; p < world; ++p) { roff[p] = sum; sum += all[p]; biggest = std::max(biggest, all[p]); }
        *total = sum;
        KCHECK(out.alloc((sum + 1) * elem));
        if (sum == 0) return KATOME_OK;
        const uint64_t chunk = std::max<uint64_t>(1, d->comm->max_message_bytes / elem);
        std::vector<uint64_t> so(world), sc(world), ro(world), rc(world);
        for (uint64_t done = 0; done < biggest; done += chunk) {
            for (int p = 0; p < world; ++p) {
                so[p] = std::min(n_mine, done); sc[p] = std::min(n_mine - so[p], chunk);
                const uint64_t rb = std::min(all[p], done);
                ro[p] = roff[p] + rb; rc[p] = std::min(all[p] - rb, chunk);
            }
            KCHECK(d->comm->t->alltoallv(mine, so.data(), sc.data(), out.p, ro.data(), rc.data(), elem, 1, stream));
        }
        katome::ExchangeStats& x = d->xstats[X_PRUNE];
        x.calls += 1; x.bytes_out += n_mine * elem * (uint64_t)(world - 1);
        KCHECK_HIP(hipStreamSynchronize(stream));
        return KATOME_OK;
    }
    // answers aligned with what `r` received travel back; out[i] = the answer to the i-th record of the sender's list (`words`
    // u64 per answer: out[i * words ..])
    int reply(const Routed& r, const u64* ans, u64* out, uint32_t words = 1) {
        ++n_reply;
        const double t0 = now_ms();
        DevBuf back(stream);
        KCHECK(back.alloc((r.n_sent + 1) * 8 * words));
        KCHECK(d->xchg(X_PRUNE, ans, r.rcnt.data(), back.p, r.counts.data(), 8 * (size_t)words, stream, false, r.pair_max));
        if (r.n_sent && words == 1) KLAUNCH(scatter_by_idx_kernel, r.n_sent, stream, back.as<u64>(), r.pidx.as<u32>(), r.n_sent, out);
        else if (r.n_sent) KLAUNCH(scatter_wide_by_idx_kernel, r.n_sent, stream, back.as<u64>(), r.pidx.as<u32>(), r.n_sent, words, out);
        KCHECK_HIP(hipGetLastError());
        KCHECK_HIP(hipStreamSynchronize(stream));
        t_xchg += now_ms() - t0;
        return KATOME_OK;
    }
};

}  // namespace
