// Host build of katome_amd/csrc/mem_pool.h over a fake backend, for tests/test_mem_pool_trim_host.py: SegmentPool::trim.
// As a shared library it is driven from Python; with -DMEM_POOL_TRIM_MAIN it is a program that runs random traffic against the
// pool and checks the blocks itself (the sanitizer build).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "../../katome_amd/csrc/mem_pool.h"

namespace {
struct FakeBackend {
    typedef int Stream;
    static size_t& used() { static size_t u = 0; return u; }
    static long& allocs() { static long n = 0; return n; }
    static long& syncs() { static long n = 0; return n; }
    static std::map<void*, size_t>& sizes() { static std::map<void*, size_t> m; return m; }
    // address space only: nothing touches the memory, so "segments" are reservations of fake addresses
    void* alloc(size_t bytes, int) {
        static uintptr_t next = 1ull << 40;
        void* p = reinterpret_cast<void*>(next);
        next += bytes + (1ull << 30);
        used() += bytes; allocs() += 1; sizes()[p] = bytes;
        return p;
    }
    void release(void* p) { used() -= sizes()[p]; sizes().erase(p); }
    void sync(int) { syncs() += 1; }
};
typedef katome::SegmentPool<FakeBackend> Pool;
Pool* pool() { static Pool p; return &p; }
}  // namespace

extern "C" {
uint64_t hs_pool_alloc(uint64_t bytes, int stream) { return (uint64_t)(uintptr_t)pool()->allocate(bytes, 0, stream); }
int hs_pool_free(uint64_t p, int stream) { return pool()->deallocate((void*)(uintptr_t)p, stream, true) ? 1 : 0; }
uint64_t hs_pool_trim(uint64_t p, uint64_t keep) { return pool()->trim((void*)(uintptr_t)p, keep); }
void hs_pool_release() { pool()->release_free_segments(-1); }
uint64_t hs_pool_round(uint64_t bytes) { return Pool::round_size(bytes); }
uint64_t hs_pool_keep() { return Pool::KEEP; }
uint64_t hs_pool_small() { return Pool::SMALL; }
void hs_pool_stats(uint64_t* out) {      // backend bytes, backend allocations, free bytes, segment bytes, live blocks, free blocks, syncs
    out[0] = FakeBackend::used(); out[1] = (uint64_t)FakeBackend::allocs(); out[2] = pool()->free_bytes();
    out[3] = pool()->segment_bytes(); out[4] = pool()->live_blocks(); out[5] = pool()->free_blocks(); out[6] = (uint64_t)FakeBackend::syncs();
}
}

#ifdef MEM_POOL_TRIM_MAIN
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "line %d: %s\n", __LINE__, #c); return 1; } } while (0)
int main(int argc, char** argv) {
    const int steps = argc > 1 ? atoi(argv[1]) : 20000;
    static const uint64_t sizes[] = {64, 4096, 3ull << 20, 9ull << 20, 40ull << 20, 300ull << 20, 2ull << 30, 7ull << 30};
    std::map<uint64_t, uint64_t> live;            // address -> the block's size as far as the caller knows it
    long trims = 0;
    for (int step = 0; step < steps; ++step) {
        const uint64_t r = rnd() % 100;
        if (!live.empty() && (r < 35 || live.size() > 60)) {
            auto it = live.begin(); std::advance(it, rnd() % live.size());
            REQUIRE(hs_pool_free(it->first, (int)(rnd() & 1)) == 1);
            live.erase(it);
        } else if (!live.empty() && r < 60) {
            auto it = live.begin(); std::advance(it, rnd() % live.size());
            const uint64_t keep = rnd() % (it->second + 1);
            const uint64_t left = hs_pool_trim(it->first, keep);
            REQUIRE(left != 0 && left >= (keep < it->second ? keep : it->second));
            // (left > the rounded request: untouched, and a remainder not worth keeping rides along with the block)
            if (left < it->second) { REQUIRE(left == hs_pool_round(keep < Pool::SMALL ? Pool::SMALL : keep)); ++trims; it->second = left; }
        } else {
            const uint64_t n = sizes[rnd() % 8] / 2 + rnd() % sizes[rnd() % 8];
            const uint64_t p = hs_pool_alloc(n, (int)(rnd() & 1));
            REQUIRE(p && !live.count(p));
            live[p] = hs_pool_round(n);
        }
        if (step % 53 == 0) {
            uint64_t end = 0, sum = 0;
            for (const auto& kv : live) { REQUIRE(kv.first >= end); end = kv.first + kv.second; sum += kv.second; }
            uint64_t s[7]; hs_pool_stats(s);
            REQUIRE(s[4] == live.size() && s[3] == s[0] && s[2] + sum <= s[3]);
        }
    }
    REQUIRE(hs_pool_trim(12345, 1) == 0);
    for (const auto& kv : live) REQUIRE(hs_pool_free(kv.first, 0) == 1);
    uint64_t s[7]; hs_pool_stats(s);
    REQUIRE(s[4] == 0 && s[2] == s[3] && s[3] == s[0]);
    hs_pool_release();
    hs_pool_stats(s);
    REQUIRE(s[0] == 0);
    printf("ok %d %ld\n", steps, trims);
    return 0;
}
#endif
