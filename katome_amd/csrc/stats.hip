// stats.hip -- Stats<CollectionStats> for PtGraph (reference src/katome/stats/collections.rs:137-168, logged five times per
// assembly by assemble_with_graph, asm/basic_assembler.rs:58-75) and the weight spectrum, on arrays that stay in HBM.
//
// CollectionStats is three passes: the edges' endpoints into one packed degree word per node (in-degree low half, out-degree
// high half, as standardize.hip's adjacency_kernel keeps them), the weights into a maximum and a u64 sum, and the degree
// words into two maxima, the two externals() counts and the out-degree sum.  Every pass reduces inside the workgroup first
// and ends in a handful of global atomics per workgroup; the two averages are one f64 division each on the host.
//
// The spectrum counts in workgroup-private u32 counters in LDS and flushes them as 64-bit adds.  Real spectra are skewed:
// most distinct edges of a read set are error k-mers of weight 1 or 2, so the 64 LDS adds of a wave would hit one or two
// addresses and serialise.  Two things take that out (spectrum_kernel<true>): the bins below SPECTRUM_LOW are counted in
// registers, and above them the value the wave's first lane holds is added once for all lanes that hold it.
// KATOME_SPECTRUM_PLAIN=1 counts every record with an LDS add of its own (the measurement of what the handling buys).
#include <algorithm>

#include "common.h"

namespace katome {
namespace {

typedef u32 u32x4_t __attribute__((ext_vector_type(4)));
typedef unsigned long long ull;
typedef ull ull2_t __attribute__((ext_vector_type(2)));

__device__ __forceinline__ u64 wave_sum64(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const u32 lo = __shfl_down((u32)v, o, 64), hi = __shfl_down((u32)(v >> 32), o, 64);
        v += ((u64)hi << 32) | lo;
    }
    return v;
}
__device__ __forceinline__ u32 wave_max(u32 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const u32 x = __shfl_down(v, o, 64); v = x > v ? x : v; }
    return v;
}

// one packed word per node: in-degree (low half) / out-degree (high half); a self-loop counts once in and once out
__global__ __launch_bounds__(BLOCK) void stats_degree_kernel(const u64* __restrict__ src, const u64* __restrict__ dst, u64 E, u64* __restrict__ deg) {
    for (u64 e = (u64)blockIdx.x * BLOCK + threadIdx.x; e < E; e += (u64)gridDim.x * BLOCK) {
        atomicAdd((ull*)&deg[src[e]], 1ull << 32);
        atomicAdd((ull*)&deg[dst[e]], 1ull);
    }
}

// res[0] += sum of the weights, res[1] = max(res[1], largest weight).  The weights [head, head + 4 * nvec) are read as
// 16-byte vectors (w + head is 16-byte aligned); workgroup 0 takes the few in front of and behind them
__global__ __launch_bounds__(BLOCK) void stats_weight_kernel(const u32* __restrict__ w, u64 n, u64 head, u64 nvec, u64* __restrict__ res) {
    __shared__ ull s_sum;
    __shared__ u32 s_max;
    if (threadIdx.x == 0) { s_sum = 0; s_max = 0; }
    __syncthreads();
    u64 sum = 0;
    u32 mx = 0;
    const u32x4_t* v = reinterpret_cast<const u32x4_t*>(w + head);
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < nvec; i += (u64)gridDim.x * BLOCK) {
        const u32x4_t x = v[i];
        sum += (u64)x.x + x.y + x.z + x.w;
        const u32 a = x.x > x.y ? x.x : x.y, b = x.z > x.w ? x.z : x.w, c = a > b ? a : b;
        mx = c > mx ? c : mx;
    }
    if (blockIdx.x == 0 && threadIdx.x < n - 4 * nvec) {
        const u64 j = threadIdx.x < head ? threadIdx.x : 4 * nvec + threadIdx.x;
        const u32 x = w[j];
        sum += x;
        mx = x > mx ? x : mx;
    }
    sum = wave_sum64(sum);
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) { if (sum) atomicAdd(&s_sum, (ull)sum); if (mx) atomicMax(&s_max, mx); }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_sum) atomicAdd((ull*)&res[0], s_sum);
        if (s_max) atomicMax((ull*)&res[1], (ull)s_max);
    }
}

// the degree words of N nodes -> res[2] max in-degree, res[3] max out-degree, res[4] nodes without in-edges (externals(Incoming),
// isolated nodes included), res[5] nodes without out-edges (externals(Outgoing)), res[6] sum of the out-degrees
__global__ __launch_bounds__(BLOCK) void stats_node_kernel(const u64* __restrict__ deg, u64 N, u64* __restrict__ res) {
    __shared__ ull s_sum_out;
    __shared__ u32 s_max_in, s_max_out, s_in0, s_out0;
    if (threadIdx.x == 0) { s_sum_out = 0; s_max_in = 0; s_max_out = 0; s_in0 = 0; s_out0 = 0; }
    __syncthreads();
    u64 sum_out = 0;
    u32 max_in = 0, max_out = 0, in0 = 0, out0 = 0;
    auto take = [&](u64 d) {
        const u32 in = (u32)d, out = (u32)(d >> 32);
        max_in = in > max_in ? in : max_in; max_out = out > max_out ? out : max_out;
        in0 += in == 0; out0 += out == 0;
        sum_out += out;
    };
    const ull2_t* v = reinterpret_cast<const ull2_t*>(deg);
    const u64 nvec = N / 2;
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < nvec; i += (u64)gridDim.x * BLOCK) { const ull2_t x = v[i]; take(x.x); take(x.y); }
    if (blockIdx.x == 0 && threadIdx.x == 0 && (N & 1)) take(deg[N - 1]);
    sum_out = wave_sum64(sum_out);
    max_in = wave_max(max_in); max_out = wave_max(max_out);
    in0 = wave_sum(in0); out0 = wave_sum(out0);
    if ((threadIdx.x & 63) == 0) {
        if (sum_out) atomicAdd(&s_sum_out, (ull)sum_out);
        if (max_in) atomicMax(&s_max_in, max_in);
        if (max_out) atomicMax(&s_max_out, max_out);
        if (in0) atomicAdd(&s_in0, in0);
        if (out0) atomicAdd(&s_out0, out0);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_max_in) atomicMax((ull*)&res[2], (ull)s_max_in);
        if (s_max_out) atomicMax((ull*)&res[3], (ull)s_max_out);
        if (s_in0) atomicAdd((ull*)&res[4], (ull)s_in0);
        if (s_out0) atomicAdd((ull*)&res[5], (ull)s_out0);
        if (s_sum_out) atomicAdd((ull*)&res[6], s_sum_out);
    }
}

// bins[min(w, n_bins - 1)] += 1 for n < 2^32 records (a workgroup's counters are u32), counted in LDS (n_bins u32, dynamic)
constexpr u32 SPECTRUM_LOW = 4;           // bins counted in registers
constexpr int SPECTRUM_MAX_BLOCK = 1024;
template <bool COMBINE>
__global__ __launch_bounds__(SPECTRUM_MAX_BLOCK) void spectrum_kernel(const u32* __restrict__ w, u64 n, u64 head, u64 nvec, u32 n_bins, u64* __restrict__ bins) {
    extern __shared__ u32 s_bins[];
    for (u32 i = threadIdx.x; i < n_bins; i += blockDim.x) s_bins[i] = 0;
    __syncthreads();
    const u32 top = n_bins - 1, lane = threadIdx.x & 63;
    u32 c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    auto count = [&](u32 x) {
        const u32 b = x < top ? x : top;
        if (!COMBINE) { atomicAdd(&s_bins[b], 1u); return; }
        c0 += b == 0; c1 += b == 1; c2 += b == 2; c3 += b == 3;
        if (b >= SPECTRUM_LOW) {
            // the lanes here that hold what the first of them holds are counted by that lane, in one add
            const u32 f = __builtin_amdgcn_readfirstlane(b);
            const u64 same = __ballot(b == f);
            if (b != f) atomicAdd(&s_bins[b], 1u);
            else if ((u32)(__ffsll((ull)same) - 1) == lane) atomicAdd(&s_bins[f], (u32)__popcll(same));
        }
    };
    const u32x4_t* v = reinterpret_cast<const u32x4_t*>(w + head);
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += 2 * stride) {      // (two loads in flight per thread)
        const bool second = i + stride < nvec;
        const u32x4_t x = v[i];
        u32x4_t y = {0, 0, 0, 0};
        if (second) y = v[i + stride];
        count(x.x); count(x.y); count(x.z); count(x.w);
        if (second) { count(y.x); count(y.y); count(y.z); count(y.w); }
    }
    if (blockIdx.x == 0 && threadIdx.x < n - 4 * nvec) count(w[threadIdx.x < head ? threadIdx.x : 4 * nvec + threadIdx.x]);
    if (COMBINE) {
        c0 = wave_sum(c0); c1 = wave_sum(c1); c2 = wave_sum(c2); c3 = wave_sum(c3);
        if (lane == 0) {                 // (a bin at or above n_bins - 1 was never counted here: min(w, top) is below it)
            if (c0) atomicAdd(&s_bins[0], c0);
            if (c1) atomicAdd(&s_bins[1], c1);
            if (c2) atomicAdd(&s_bins[2], c2);
            if (c3) atomicAdd(&s_bins[3], c3);
        }
    }
    __syncthreads();
    for (u32 i = threadIdx.x; i < n_bins; i += blockDim.x) { const u32 c = s_bins[i]; if (c) atomicAdd((ull*)&bins[i], (ull)c); }
}

// KATOME_STATS_TRACE (set to anything; tools/bench_graph_stats.py): every kernel of this file is timed with HIP events on its
// stream and printed on stderr, one line per launch: its name, its milliseconds and the elements it processed.  Waits for the kernel.
struct KernelTrace {
    const char* name; hipStream_t stream; uint64_t elements; hipEvent_t a = nullptr, b = nullptr;
    KernelTrace(const char* name_, hipStream_t s, uint64_t n) : name(name_), stream(s), elements(n) {
        if (!getenv("KATOME_STATS_TRACE")) return;
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess || hipEventRecord(a, stream) != hipSuccess) { done(); }
    }
    ~KernelTrace() {
        float ms = 0;
        if (a && b && hipEventRecord(b, stream) == hipSuccess && hipEventSynchronize(b) == hipSuccess && hipEventElapsedTime(&ms, a, b) == hipSuccess)
            fprintf(stderr, "[katome_stats] %s: %.4f ms, %llu elements\n", name, ms, (unsigned long long)elements);
        done();
    }
    void done() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); a = b = nullptr; }
};

// the stretch of a u32 array that 16-byte loads cover: `head` elements in front of it, then nvec vectors
void vector_stretch(const uint32_t* w, uint64_t n, uint64_t* head, uint64_t* nvec) {
    *head = std::min<uint64_t>(n, ((16 - ((uintptr_t)w & 15)) & 15) / 4);
    *nvec = (n - *head) / 4;
}

// adds the histogram of n weights to d_bins (device, n_bins u64)
int dev_weight_spectrum_device(const uint32_t* weight, uint64_t n, uint64_t* d_bins, uint32_t n_bins, hipStream_t stream) {
    const bool plain = env_flag("KATOME_SPECTRUM_PLAIN", false);
    // (many bins leave room for two workgroups on a CU: large ones keep it busy)
    const unsigned block = n_bins > 4096 ? SPECTRUM_MAX_BLOCK : BLOCK;
    const uint64_t piece = 1ull << 31;                  // a workgroup's counters are u32
    for (uint64_t at = 0; at < n; at += piece) {
        const uint64_t cnt = std::min(n - at, piece);
        uint64_t head = 0, nvec = 0;
        vector_stretch(weight + at, cnt, &head, &nvec);
        const dim3 grid(grid_for((nvec + 1) / 2, block, 2048u));
        KernelScope ks(K_SPECTRUM, stream, cnt);
        KernelTrace kt(plain ? "spectrum_kernel<plain>" : "spectrum_kernel", stream, cnt);
        if (plain) hipLaunchKernelGGL(spectrum_kernel<false>, grid, dim3(block), n_bins * 4, stream, weight + at, cnt, head, nvec, n_bins, d_bins);
        else       hipLaunchKernelGGL(spectrum_kernel<true>, grid, dim3(block), n_bins * 4, stream, weight + at, cnt, head, nvec, n_bins, d_bins);
        KCHECK_HIP(hipGetLastError());
    }
    return KATOME_OK;
}

}  // namespace

int dev_weight_max_sum(const uint32_t* weight, uint64_t n, uint64_t* d_res, hipStream_t stream) {
    if (n == 0) return KATOME_OK;
    uint64_t head = 0, nvec = 0;
    vector_stretch(weight, n, &head, &nvec);
    KernelScope ks(K_STATS_WEIGHTS, stream, n);
    KernelTrace kt("stats_weight_kernel", stream, n);
    hipLaunchKernelGGL(stats_weight_kernel, dim3(grid_for(nvec, BLOCK, 2048u)), dim3(BLOCK), 0, stream, weight, n, head, nvec, d_res);
    KCHECK_HIP(hipGetLastError());
    return KATOME_OK;
}

int dev_degree_reduce(const uint64_t* d_deg, uint64_t N, uint64_t* d_res, hipStream_t stream) {
    if (N == 0) return KATOME_OK;
    KernelScope ks(K_STATS_NODES, stream, N);
    KernelTrace kt("stats_node_kernel", stream, N);
    hipLaunchKernelGGL(stats_node_kernel, dim3(grid_for(N / 2, BLOCK, 2048u)), dim3(BLOCK), 0, stream, d_deg, N, d_res);
    KCHECK_HIP(hipGetLastError());
    return KATOME_OK;
}

void fill_stats(uint64_t n_nodes, uint64_t n_edges, const uint64_t res[STATS_WORDS], katome_stats* out) {
    memset(out, 0, sizeof *out);
    out->node_count = n_nodes; out->edge_count = n_edges;
    out->max_edge_weight = (uint32_t)res[1];
    out->avg_edge_weight = (double)res[0] / (double)n_edges;            // (no edges: NaN, as the reference's 0.0 / 0.0)
    out->max_in_degree = res[2]; out->max_out_degree = res[3];
    out->avg_out_degree = (double)res[6] / (double)n_nodes;
    out->incoming_vert_count = res[4]; out->outgoing_vert_count = res[5];
}

int dev_graph_stats(const uint64_t* src, const uint64_t* dst, const uint32_t* weight, uint64_t E, uint64_t N, katome_stats* out, hipStream_t stream) {
    if (E >= (1ull << 32)) { set_error("graph stats: 2^32 edges or more on one GPU"); return KATOME_E_UNSUPPORTED; }
    if (E && !N) { set_error("graph stats: edges without nodes"); return KATOME_E_ARG; }
    uint64_t h[STATS_WORDS] = {0};
    if (N) {
        DevBuf deg(stream), res(stream);
        KCHECK(deg.alloc(N * 8)); KCHECK(res.alloc(STATS_WORDS * 8));
        KCHECK_HIP(hipMemsetAsync(deg.p, 0, N * 8, stream));
        KCHECK_HIP(hipMemsetAsync(res.p, 0, STATS_WORDS * 8, stream));
        if (E) {
            KernelScope ks(K_STATS_DEGREES, stream, E);
            KernelTrace kt("stats_degree_kernel", stream, E);
            hipLaunchKernelGGL(stats_degree_kernel, dim3(grid_for(E, BLOCK, 256u * 32u)), dim3(BLOCK), 0, stream, src, dst, E, deg.as<u64>());
            KCHECK_HIP(hipGetLastError());
        }
        KCHECK(dev_weight_max_sum(weight, E, res.as<u64>(), stream));
        KCHECK(dev_degree_reduce(deg.as<u64>(), N, res.as<u64>(), stream));
        KCHECK_HIP(hipMemcpyAsync(h, res.p, sizeof h, hipMemcpyDeviceToHost, stream));
        KCHECK_HIP(hipStreamSynchronize(stream));
    }
    fill_stats(N, E, h, out);
    return KATOME_OK;
}

int check_spectrum_bins(const uint64_t* bins, uint32_t n_bins) {
    if (!bins) { set_error("null argument"); return KATOME_E_ARG; }
    if (n_bins < 2 || n_bins > 16384) { set_error("weight spectrum: n_bins = %u (2..16384)", n_bins); return KATOME_E_ARG; }
    return KATOME_OK;
}

int dev_weight_spectrum(const uint32_t* weight, uint64_t n, uint64_t* bins, uint32_t n_bins, hipStream_t stream) {
    memset(bins, 0, (size_t)n_bins * 8);
    if (n == 0) return KATOME_OK;
    DevBuf d_bins(stream);
    KCHECK(d_bins.alloc((size_t)n_bins * 8));
    KCHECK_HIP(hipMemsetAsync(d_bins.p, 0, (size_t)n_bins * 8, stream));
    KCHECK(dev_weight_spectrum_device(weight, n, d_bins.as<u64>(), n_bins, stream));
    KCHECK_HIP(hipMemcpyAsync(bins, d_bins.p, (size_t)n_bins * 8, hipMemcpyDeviceToHost, stream));
    KCHECK_HIP(hipStreamSynchronize(stream));
    return KATOME_OK;
}

}  // namespace katome

using namespace katome;

extern "C" {

int katome_dev_stats_arrays(int device, const uint64_t* d_edge_src, const uint64_t* d_edge_dst, const uint32_t* d_edge_weight, uint64_t n_edges,
                            uint64_t n_nodes, katome_stats* out, void* stream) {
    if (!out || (n_edges && (!d_edge_src || !d_edge_dst || !d_edge_weight))) { set_error("null argument"); return KATOME_E_ARG; }
    KCHECK(use_device(device));
    return dev_graph_stats(d_edge_src, d_edge_dst, d_edge_weight, n_edges, n_nodes, out, (hipStream_t)stream);
}

int katome_dev_weight_spectrum_arrays(int device, const uint32_t* d_weight, uint64_t n, uint64_t* bins, uint32_t n_bins, void* stream) {
    KCHECK(check_spectrum_bins(bins, n_bins));
    if (n && !d_weight) { set_error("null argument"); return KATOME_E_ARG; }
    KCHECK(use_device(device));
    return dev_weight_spectrum(d_weight, n, bins, n_bins, (hipStream_t)stream);
}

}  // extern "C"
