// dist_contigs.hip -- the RANKED route of katome_dist_standardize_contigs (standardizer.rs:72-122) on the SHARDED graph: what
// dist_stages.hip's replicated table computes, bit for bit, with memory per rank that does not grow with the whole graph.
//   * a vertex is PASS-THROUGH when in-degree = out-degree = 1 (the table route's word that is neither T_AMBIGUOUS nor T_END).
//     A contig starts at an edge whose source is not pass-through (its HEAD), runs through pass-through vertices and ends at
//     the edge whose target is not pass-through (its LAST edge).  That is dist_shrink.hip's INNER (dist_links.h), with two
//     things to note: cycles of pass-through vertices belong to no contig and keep their weights; a self-loop at a vertex with
//     in = out = 1 counts as a head, a contig of one edge whose mean is its own weight (no contig reaches it either way).
//   * list ranking by pointer jumping with sums: per edge the state is (P, S, C): P = RESOLVED | head address or the address of
//     an edge further back on its path, S = the u64 sum of the weights over the span between that edge (exclusive) and this one
//     (inclusive; from the head, inclusive, once resolved), C = the edges of that span.  An edge asks the rank of P for that
//     edge's state (p, s, c) and becomes (p, S + s, C + c): correct whatever the asked edge's state is at that moment, because the
//     count travels with the sum (dist_shrink.hip implies it as 2^round, which ties it to the state at the start of the round).
//     So the state is updated in place, and the questions of a round go in CHUNKS of at most KATOME_DIST_CONTIGS_CHUNK
//     (default 2^24) per rank and exchange: the answers of a chunk are applied before the next chunk asks; the answering and
//     the applying kernel are separate launches, so an answer never sees half an update.  The rounds stop when nothing is
//     unresolved, or when a whole round resolved nothing anywhere: on every path the unresolved edge nearest the head points at
//     a resolved one, so what is left then lies on cycles of pass-through vertices.  Rounds: ceil(log2 L) for the longest
//     contig L, one more when cycles are left.
//   * means: the last edge of a contig holds its whole sum and count, computes (u32)round((double)sum / (double)L) -- the table
//     route's expression -- writes its own weight and sends (head address, mean) to the head's rank, which keeps the mean per
//     own head edge and writes the head's weight.  Every other edge of a contig asks its head's rank (the same chunks).
// The sums are made of the weights as they stood when the call began: weights are written only after the ranking.
// Memory beyond the share: 21 B per own node and 28 B per own edge for the links, then 33 B per own edge while the rounds run
// (the state 20, the last-edge flags 1, the round's question list 12) and 49 B while the mean records are made, beside 48 to
// 80 B per record or question of the chunk in flight; nothing grows with the whole graph.  Limits, agreed on every
// rank: a share below 2^32 edges and nodes, a contig below 2^32 edges (KATOME_E_UNSUPPORTED); a broken invariant counted by a
// kernel is KATOME_E_DEVICE.
#include <cstdio>
#include <cstdlib>

#include "dist_links.h"

namespace {

constexpr u64 RESOLVED = 1ull << 55;                  // state word P: the head's address follows (bits 56.. rank, 0..31 index)
constexpr u64 ADDR = (0xFFull << 56) | 0xFFFFFFFFull;
constexpr u64 DEFAULT_CHUNK = 1ull << 24;
enum Flag { F_BAD = 0, F_TOO_LONG = 1, F_LONGEST = 2, F_HEADS = 3 };      // words of the flags buffer

// heads start resolved with their own weight and a count of 1; every other edge points at its predecessor
__global__ __launch_bounds__(BLOCK) void cg_init_kernel(u64 E, const u32* __restrict__ lsrc, const unsigned char* __restrict__ inner,
                                                        const u64* __restrict__ in_edge, const u64* __restrict__ dst_inner, const u32* __restrict__ weight,
                                                        u64 me, u64* __restrict__ P, u64* __restrict__ S, u32* __restrict__ Cn, unsigned char* __restrict__ last) {
    WLOOP(e, E) if (e < E) {
        const u32 l = lsrc[e];
        P[e] = inner[l] ? in_edge[l] : (RESOLVED | (me << 56) | e);
        S[e] = weight[e]; Cn[e] = 1u;
        last[e] = dst_inner[e] == 0;
    }
}
// the unresolved edges: their pointer (the question) and themselves
__global__ __launch_bounds__(BLOCK) void cg_active_kernel(const u64* __restrict__ P, u64 E, u64* __restrict__ q, u32* __restrict__ who, unsigned long long* cursor) {
    TLOOP(t0, E) {
        u32 mine = 0, have = 0;
#pragma unroll
        for (int k = 0; k < CA_ITEMS; ++k) {
            const u64 e = t0 + (u64)k * BLOCK + threadIdx.x;
            if (e < E && !(P[e] & RESOLVED)) { have |= 1u << k; ++mine; }
        }
        u64 at = block_append(mine, cursor);
#pragma unroll
        for (int k = 0; k < CA_ITEMS; ++k) if (have & (1u << k)) { const u64 e = t0 + (u64)k * BLOCK + threadIdx.x; q[at] = P[e] & ADDR; who[at] = (u32)e; ++at; }
    }
}
// the asked edge's state as it stands (a pointer at no edge of this rank: counted, and the asker stays as it is)
__global__ __launch_bounds__(BLOCK) void cg_answer_kernel(const u64* __restrict__ A, u64 n, u64 E, const u64* __restrict__ P, const u64* __restrict__ S,
                                                          const u32* __restrict__ Cn, u64* __restrict__ ans_p, u64* __restrict__ ans_s, u64* __restrict__ ans_c,
                                                          unsigned long long* flags) {
    WLOOP(i, n) if (i < n) {
        const u32 l = local_of(A[i]);
        if (l < E) { ans_p[i] = P[l]; ans_s[i] = S[l]; ans_c[i] = Cn[l]; }
        else { ans_p[i] = A[i] & ADDR; ans_s[i] = 0; ans_c[i] = 0; atomicAdd(&flags[F_BAD], 1ull); }
    }
}
// (P, S, C) <- (p, S + s, C + c); the count saturates on the cycles, where it means nothing; a resolved one must fit 32 bits
__global__ __launch_bounds__(BLOCK) void cg_apply_kernel(const u32* __restrict__ who, u64 n, const u64* __restrict__ got_p, const u64* __restrict__ got_s,
                                                         const u64* __restrict__ got_c, u64* __restrict__ P, u64* __restrict__ S, u32* __restrict__ Cn,
                                                         unsigned long long* flags) {
    WLOOP(i, n) if (i < n) {
        const u32 e = who[i];
        const u64 p = got_p[i], c = (u64)Cn[e] + got_c[i];
        P[e] = p; S[e] += got_s[i];
        Cn[e] = c > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)c;
        if ((p & RESOLVED) && c > 0xFFFFFFFFull) atomicAdd(&flags[F_TOO_LONG], 1ull);
    }
}
// the last edge of every contig: its mean, written on itself and sent to the head; the heads of this rank and the longest
// contig counted per wave
__global__ __launch_bounds__(BLOCK) void cg_mean_kernel(u64 E, const u64* __restrict__ P, const u64* __restrict__ S, const u32* __restrict__ Cn,
                                                        const unsigned char* __restrict__ last, u64 me, u32* __restrict__ weight, u64* __restrict__ A,
                                                        u64* __restrict__ B, unsigned long long* cursor, unsigned long long* flags) {
    WLOOP(e, E) {
        const bool ok = e < E;
        const u64 p = ok ? P[e] : 0;
        const bool done = ok && (p & RESOLVED), is_last = done && last[e], head = done && p == (RESOLVED | (me << 56) | e);
        const u64 at = wave_append(is_last, cursor);
        u32 len = 0;
        if (is_last) {
            len = Cn[e];
            const u32 mean = (u32)round((double)S[e] / (double)len);
            weight[e] = mean;
            A[at] = p & ADDR; B[at] = mean;
        }
        const u64 heads = __ballot(head);
        if (__ballot(is_last)) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) { const u32 t = __shfl_xor(len, o, 64); if (t > len) len = t; }
        }
        if ((threadIdx.x & 63) == 0) {
            if (heads) atomicAdd(&flags[F_HEADS], (unsigned long long)__popcll(heads));
            if (len) atomicMax(&flags[F_LONGEST], (unsigned long long)len);
        }
    }
}
// on the head's rank: the mean per own head edge (a record that names no head of this rank is counted)
__global__ __launch_bounds__(BLOCK) void cg_place_kernel(const u64* __restrict__ A, const u64* __restrict__ B, u64 n, u64 E, const u64* __restrict__ P, u64 me,
                                                         u64* __restrict__ head_mean, u32* __restrict__ weight, unsigned long long* flags) {
    WLOOP(i, n) if (i < n) {
        const u32 l = local_of(A[i]);
        if (l < E && P[l] == (RESOLVED | (me << 56) | l)) { head_mean[l] = B[i]; weight[l] = (u32)B[i]; }
        else atomicAdd(&flags[F_BAD], 1ull);
    }
}
// the edges of a contig that are neither its head nor its last edge ask the head's rank; a head without a mean is counted
__global__ __launch_bounds__(BLOCK) void cg_ask_kernel(const u64* __restrict__ P, const unsigned char* __restrict__ last, const u64* __restrict__ head_mean, u64 E,
                                                       u64 me, u64* __restrict__ q, u32* __restrict__ who, unsigned long long* cursor, unsigned long long* flags) {
    TLOOP(t0, E) {
        u32 mine = 0, have = 0, orphans = 0;
#pragma unroll
        for (int k = 0; k < CA_ITEMS; ++k) {
            const u64 e = t0 + (u64)k * BLOCK + threadIdx.x;
            if (e >= E) continue;
            const u64 p = P[e];
            if (!(p & RESOLVED)) continue;
            if (p == (RESOLVED | (me << 56) | e)) { if (head_mean[e] == NONE64) ++orphans; }
            else if (!last[e]) { have |= 1u << k; ++mine; }
        }
        if (orphans) atomicAdd(&flags[F_BAD], (unsigned long long)orphans);      // (a broken invariant only)
        u64 at = block_append(mine, cursor);
#pragma unroll
        for (int k = 0; k < CA_ITEMS; ++k) if (have & (1u << k)) { const u64 e = t0 + (u64)k * BLOCK + threadIdx.x; q[at] = P[e] & ADDR; who[at] = (u32)e; ++at; }
    }
}
__global__ __launch_bounds__(BLOCK) void cg_mean_answer_kernel(const u64* __restrict__ A, u64 n, u64 E, const u64* __restrict__ P, u64 me,
                                                               const u64* __restrict__ head_mean, u64* __restrict__ ans, unsigned long long* flags) {
    WLOOP(i, n) if (i < n) {
        const u32 l = local_of(A[i]);
        const u64 m = (l < E && P[l] == (RESOLVED | (me << 56) | l)) ? head_mean[l] : NONE64;
        ans[i] = m;
        if (m == NONE64) atomicAdd(&flags[F_BAD], 1ull);
    }
}
__global__ __launch_bounds__(BLOCK) void cg_mean_apply_kernel(const u32* __restrict__ who, u64 n, const u64* __restrict__ got, u32* __restrict__ weight) {
    WLOOP(i, n) if (i < n && got[i] != NONE64) weight[who[i]] = (u32)got[i];
}

// a number from the environment, asked for on every call; `unset` when it is not there
long long env_ll(const char* name, long long unset) {
    const char* e = getenv(name);
    return e && *e ? atoll(e) : unset;
}

struct Ranked {
    katome_dist_builder* d; hipStream_t stream; int rank, world; uint64_t E, chunk;
    Router router; DevBuf cursors, flags;
    Ranked(katome_dist_builder* d_, hipStream_t s) : d(d_), stream(s), rank(d_->rank()), world(d_->world()), E(d_->n_edges), router(d_, s), cursors(s), flags(s) {
        const long long c = env_ll("KATOME_DIST_CONTIGS_CHUNK", (long long)DEFAULT_CHUNK);
        chunk = c < 1 ? 1 : (uint64_t)c;
    }
    unsigned long long* cur() { return cursors.as<unsigned long long>(); }
    unsigned long long* flg() { return flags.as<unsigned long long>(); }
    int init() {
        KCHECK(d->comm->allreduce(&chunk, 1, OP_MIN));       // (process ranks may see different environments: the smallest holds)
        KCHECK(cursors.alloc(64)); KCHECK(flags.alloc(64));
        KCHECK_HIP(hipMemsetAsync(flags.p, 0, 64, stream));
        return router.init();
    }
    int reset() { KCHECK_HIP(hipMemsetAsync(cursors.p, 0, 64, stream)); return KATOME_OK; }
    int read(const DevBuf& from, uint64_t* h, int n) {
        KCHECK_HIP(hipMemcpyAsync(h, from.p, 8 * n, hipMemcpyDeviceToHost, stream));
        KCHECK_HIP(hipStreamSynchronize(stream));
        return KATOME_OK;
    }
    uint64_t chunks_of(uint64_t n) const { return (n + chunk - 1) / chunk; }
};

}  // namespace

// the ranked route of katome_dist_standardize_contigs (dist_stages.hip chooses the route and checks the builder); collective
int dist_contigs_ranked(katome_dist_builder* d, hipStream_t stream, katome_dist_standardize_stats* st) {
    Ranked R(d, stream);
    KCHECK(R.init());
    const uint64_t E = R.E, me = (uint64_t)R.rank;
    const int world = R.world;
    u32* weight = d->b->edge_weight.as<u32>();
    // ---- degrees and links (dist_links.h); then the state -----------------------------------------------------------------
    DevBuf P(stream), S(stream), Cn(stream), last(stream);
    {
        Links links(stream);
        KCHECK(dist_links(d, R.router, stream, links, R.chunk));
        KCHECK(P.alloc((E + 1) * 8)); KCHECK(S.alloc((E + 1) * 8)); KCHECK(Cn.alloc((E + 1) * 4)); KCHECK(last.alloc(E + 16));
        if (E) KLAUNCH(cg_init_kernel, E, stream, E, links.lsrc.as<u32>(), links.inner.as<unsigned char>(), links.in_edge.as<u64>(), links.dst_inner.as<u64>(),
                       weight, me, P.as<u64>(), S.as<u64>(), Cn.as<u32>(), last.as<unsigned char>());
        KCHECK_HIP(hipGetLastError());
        KCHECK_HIP(hipStreamSynchronize(stream));
    }
    // ---- ranking with sums ------------------------------------------------------------------------------------------------
    // KATOME_DIST_CONTIGS_FAIL=<rank> (tests): that rank reports a failure after the first ranking round
    const long long fail_at = env_ll("KATOME_DIST_CONTIGS_FAIL", -1);
    constexpr uint64_t KNOB = 1ull << 40, FAILS = 1ull << 41, COUNT = KNOB - 1;      // beside the count in a rank's allgathered word
    const uint64_t in_flight = std::min<uint64_t>(E, R.chunk);
    DevBuf q(stream), who(stream), got_p(stream), got_s(stream), got_c(stream), ans_p(stream), ans_s(stream), ans_c(stream);
    KCHECK(q.alloc((E + 1) * 8)); KCHECK(who.alloc((E + 1) * 4));
    KCHECK(got_p.alloc((in_flight + 1) * 8)); KCHECK(got_s.alloc((in_flight + 1) * 8)); KCHECK(got_c.alloc((in_flight + 1) * 8));
    std::vector<uint64_t> per_rank(world, 0);
    uint64_t prev = ~0ull, U = 0, exchanges = 0;
    uint32_t t = 0;
    for (;; ++t) {
        KCHECK(R.reset());
        if (E) KLAUNCH_T(cg_active_kernel, E, stream, P.as<u64>(), E, q.as<u64>(), who.as<u32>(), R.cur());
        KCHECK_HIP(hipGetLastError());
        uint64_t n_act = 0;
        KCHECK(R.read(R.cursors, &n_act, 1));
        // one collective per round: every rank's count of unresolved edges, and what the test knob says there
        KCHECK(d->comm->allgather(n_act | (fail_at >= 0 ? KNOB : 0) | (fail_at == (long long)R.rank && t == 1 ? FAILS : 0), per_rank.data()));
        uint64_t n_max = 0;
        bool knob = false;
        int who_failed = -1;
        U = 0;
        for (int p = 0; p < world; ++p) {
            const uint64_t n = per_rank[p] & COUNT;
            U += n; n_max = std::max(n_max, n);
            knob = knob || (per_rank[p] & KNOB);
            if ((per_rank[p] & FAILS) && who_failed < 0) who_failed = p;
        }
        if (who_failed >= 0) {
            if (who_failed == R.rank) set_error("katome_dist_standardize_contigs: KATOME_DIST_CONTIGS_FAIL=%lld: rank %d fails after ranking round 1", fail_at, R.rank);
            else set_error("katome_dist_standardize_contigs: rank %d failed after ranking round 1", who_failed);
            return KATOME_E_UNSUPPORTED;
        }
        const bool stop = U == 0 || U == prev;               // all resolved, or a whole round resolved nothing: cycles are left
        // (the knob strikes after round 1 even when the ranking needs fewer: with the knob set, a ranking that needs no round
        // still makes one, empty, and rank_rounds says 1 -- also when the knob names a rank outside the world)
        if (stop && !(knob && t < 1)) break;
        if (t >= 72) { set_error("katome_dist_standardize_contigs: the ranking did not converge"); return KATOME_E_DEVICE; }
        prev = U;
        const uint64_t n_chunks = R.chunks_of(n_max);        // (n_max and the chunk: the same on every rank)
        for (uint64_t c = 0; c < n_chunks; ++c) {
            const uint64_t at = std::min(n_act, c * R.chunk), cnt = std::min(n_act - at, R.chunk);
            Routed asked(stream);
            KCHECK(R.router.send(q.as<u64>() + at, nullptr, cnt, asked));
            KCHECK(ans_p.alloc((asked.n + 1) * 8)); KCHECK(ans_s.alloc((asked.n + 1) * 8)); KCHECK(ans_c.alloc((asked.n + 1) * 8));
            if (asked.n) KLAUNCH(cg_answer_kernel, asked.n, stream, asked.a.as<u64>(), asked.n, E, P.as<u64>(), S.as<u64>(), Cn.as<u32>(), ans_p.as<u64>(),
                                 ans_s.as<u64>(), ans_c.as<u64>(), R.flg());
            KCHECK_HIP(hipGetLastError());
            KCHECK(R.router.reply(asked, ans_p.as<u64>(), got_p.as<u64>()));
            KCHECK(R.router.reply(asked, ans_s.as<u64>(), got_s.as<u64>()));
            KCHECK(R.router.reply(asked, ans_c.as<u64>(), got_c.as<u64>()));
            if (cnt) KLAUNCH(cg_apply_kernel, cnt, stream, who.as<u32>() + at, cnt, got_p.as<u64>(), got_s.as<u64>(), got_c.as<u64>(), P.as<u64>(), S.as<u64>(),
                             Cn.as<u32>(), R.flg());
            KCHECK_HIP(hipGetLastError());
        }
        exchanges += n_chunks;
    }
    got_p.release(); got_s.release(); got_c.release(); ans_p.release(); ans_s.release(); ans_c.release();
    const uint32_t rounds = t;
    const uint64_t cycle_edges = U;
    {
        uint64_t h[8] = {0};
        KCHECK(R.read(R.flags, h, 8));
        uint64_t bad[2] = {h[F_BAD], h[F_TOO_LONG]};
        KCHECK(d->comm->allreduce(bad, 2, OP_MAX));
        if (bad[0]) { set_error("katome_dist_standardize_contigs: %llu ranking questions name no edge of the rank they went to", (unsigned long long)bad[0]); return KATOME_E_DEVICE; }
        if (bad[1]) { set_error("katome_dist_standardize_contigs: a contig of 2^32 edges or more"); return KATOME_E_UNSUPPORTED; }
    }
    // ---- means: last edge -> head's rank; every other edge of a contig asks there -------------------------------------------
    DevBuf head_mean(stream), B(stream);
    KCHECK(head_mean.alloc((E + 1) * 8));
    KCHECK_HIP(hipMemsetAsync(head_mean.p, 0xFF, (E + 1) * 8, stream));
    // (the records reuse the question list's room: one per contig that ends here)
    KCHECK(B.alloc((E + 1) * 8));
    KCHECK(R.reset());
    if (E) KLAUNCH(cg_mean_kernel, E, stream, E, P.as<u64>(), S.as<u64>(), Cn.as<u32>(), last.as<unsigned char>(), me, weight, q.as<u64>(), B.as<u64>(), R.cur(),
                   R.flg());
    KCHECK_HIP(hipGetLastError());
    uint64_t n_last = 0, h[8] = {0};
    KCHECK(R.read(R.cursors, &n_last, 1));
    KCHECK(R.read(R.flags, h, 8));
    S.release(); Cn.release();
    uint64_t n_placed = 0, rec_chunks = R.chunks_of(n_last);
    KCHECK(d->comm->allreduce(&rec_chunks, 1, OP_MAX));
    for (uint64_t c = 0; c < rec_chunks; ++c) {
        const uint64_t at = std::min(n_last, c * R.chunk), cnt = std::min(n_last - at, R.chunk);
        Routed r(stream);
        KCHECK(R.router.send(q.as<u64>() + at, B.as<u64>() + at, cnt, r));
        n_placed += r.n;
        if (r.n) KLAUNCH(cg_place_kernel, r.n, stream, r.a.as<u64>(), r.b.as<u64>(), r.n, E, P.as<u64>(), me, head_mean.as<u64>(), weight, R.flg());
        KCHECK_HIP(hipGetLastError());
    }
    KCHECK_HIP(hipStreamSynchronize(stream));
    B.release();
    KCHECK(R.reset());
    if (E) KLAUNCH_T(cg_ask_kernel, E, stream, P.as<u64>(), last.as<unsigned char>(), head_mean.as<u64>(), E, me, q.as<u64>(), who.as<u32>(), R.cur(), R.flg());
    KCHECK_HIP(hipGetLastError());
    uint64_t n_ask = 0;
    KCHECK(R.read(R.cursors, &n_ask, 1));
    // agreed: the chunks of the questions, the contigs and the longest one; every head got one mean
    uint64_t mx[2] = {R.chunks_of(n_ask), h[F_LONGEST]}, sums[3] = {h[F_HEADS], n_last, n_placed != h[F_HEADS] ? 1ull : 0ull};
    KCHECK(d->comm->allreduce(mx, 2, OP_MAX));
    KCHECK(d->comm->allreduce(sums, 3, OP_SUM));
    if (sums[0] != sums[1] || sums[2]) { set_error("katome_dist_standardize_contigs: %llu heads, %llu last edges: a contig without one last edge", (unsigned long long)sums[0], (unsigned long long)sums[1]); return KATOME_E_DEVICE; }
    {
        DevBuf got(stream), ans(stream);
        KCHECK(got.alloc((std::min<uint64_t>(n_ask, R.chunk) + 1) * 8));
        for (uint64_t c = 0; c < mx[0]; ++c) {
            const uint64_t at = std::min(n_ask, c * R.chunk), cnt = std::min(n_ask - at, R.chunk);
            Routed asked(stream);
            KCHECK(R.router.send(q.as<u64>() + at, nullptr, cnt, asked));
            KCHECK(ans.alloc((asked.n + 1) * 8));
            if (asked.n) KLAUNCH(cg_mean_answer_kernel, asked.n, stream, asked.a.as<u64>(), asked.n, E, P.as<u64>(), me, head_mean.as<u64>(), ans.as<u64>(), R.flg());
            KCHECK_HIP(hipGetLastError());
            KCHECK(R.router.reply(asked, ans.as<u64>(), got.as<u64>()));
            if (cnt) KLAUNCH(cg_mean_apply_kernel, cnt, stream, who.as<u32>() + at, cnt, got.as<u64>(), weight);
            KCHECK_HIP(hipGetLastError());
        }
        exchanges += mx[0];
    }
    {
        uint64_t f[8] = {0};
        KCHECK(R.read(R.flags, f, 8));
        uint64_t bad = f[F_BAD];
        KCHECK(d->comm->allreduce(&bad, 1, OP_MAX));
        if (bad) { set_error("katome_dist_standardize_contigs: %llu mean records or questions name no head of the rank they went to", (unsigned long long)bad); return KATOME_E_DEVICE; }
    }
    st->rank_rounds = rounds; st->exchanges = exchanges; st->contigs = sums[0]; st->longest_contig = mx[1]; st->cycle_edges = cycle_edges;
    return KATOME_OK;
}

extern "C" {

int katome_dist_standardize_stats_read(katome_dist_builder* d, katome_dist_standardize_stats* out) {
    if (!d || !out) { set_error("null argument"); return KATOME_E_ARG; }
    if (!d->contigs_stats_valid) { set_error("katome_dist_standardize_stats_read: no katome_dist_standardize_contigs has finished on this builder"); return KATOME_E_ARG; }
    *out = d->contigs_stats;
    return KATOME_OK;
}

}  // extern "C"
