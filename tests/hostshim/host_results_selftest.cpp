// Host-only driver of the host results of katome_amd/csrc/host_build.cpp (the owner of a result, the handle that holds one under
// construction, the copier that fills its arrays) for sanitizer runs (tests/test_host_results_host.py).  No device: the HIP calls
// the copies make are stubbed below, "device" memory is host memory, and a copy can be told to fail.
// usage: host_results_selftest  -> "ok <checks>"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define KATOME_HOST_RESULTS_ONLY
#include "../../katome_amd/csrc/host_build.cpp"

// the caching device allocator is not part of this build (ingest.cpp, linked for the error state, names it)
namespace katome {
int dev_malloc(void**, size_t, hipStream_t) { return KATOME_E_DEVICE; }
void dev_free(void*, hipStream_t) {}
}

static int copies_left = -1;      // (-1: every copy works; n: the n-th copy from now fails)
extern "C" hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind) {
    if (copies_left == 0) return hipErrorInvalidValue;
    if (copies_left > 0) --copies_left;
    memcpy(dst, src, bytes);
    return hipSuccess;
}
extern "C" const char* hipGetErrorString(hipError_t) { return "stubbed copy failure"; }
extern "C" hipError_t hipGetLastError(void) { return hipErrorInvalidValue; }

static int checks = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } ++checks; } while (0)

// a katome_contigs of n edges filled through the copier; fail_at: the copy that fails (-1: none)
static int fill(Result<katome_contigs>& c, uint64_t n, int fail_at) {
    std::vector<uint64_t> src(n), off(n + 1);
    std::vector<uint32_t> w(n);
    for (uint64_t i = 0; i < n; ++i) { src[i] = 3 * i + 1; w[i] = (uint32_t)(i ^ 5); off[i + 1] = off[i] + 2; }
    std::vector<uint8_t> label(2 * n, 0x5A);
    if (!(c = make_result<katome_contigs>())) return KATOME_E_OOM;
    c->n_edges = n; c->label_bytes = label.size();
    copies_left = fail_at;
    Copier<katome_contigs> down{c.get()};
    down(&c->edge_src, src.data(), n);
    down(&c->edge_weight, w.data(), n);
    down(&c->edge_label_off, off.data(), n ? n + 1 : 0);
    down(&c->edge_label, label.data(), label.size());      // (n = 0: an array of 0 bytes, which still gets room for one element)
    copies_left = -1;
    if (down.rc) return down.rc;
    for (uint64_t i = 0; i < n; ++i) CHECK(c->edge_src[i] == 3 * i + 1 && c->edge_weight[i] == (uint32_t)(i ^ 5) && c->edge_label_off[i + 1] == 2 * (i + 1));
    for (uint64_t i = 0; i < 2 * n; ++i) CHECK(c->edge_label[i] == 0x5A);
    return KATOME_OK;
}

int main() {
    {   // made in full, handed out and freed through the public free
        Result<katome_contigs> c;
        CHECK(fill(c, 1000, -1) == KATOME_OK);
        CHECK(owner_of(c.get())->mem.size() == 4);
        CHECK(c->n_nodes == 0 && c->node_key == nullptr);               // (zeroed where nothing was filled in)
        katome_contigs* handed_out = c.release();
        CHECK(!c);
        katome_contigs_free(handed_out);
    }
    {   // nothing to copy: every array is still there, and its one element can be written
        Result<katome_contigs> c;
        CHECK(fill(c, 0, -1) == KATOME_OK);
        CHECK(c->edge_src && c->edge_weight && c->edge_label_off && c->edge_label);
        const_cast<uint64_t*>(c->edge_label_off)[0] = 0;
        const_cast<uint8_t*>(c->edge_label)[0] = 0;
    }                                                                    // (the handle frees it)
    for (int fail_at = 0; fail_at < 4; ++fail_at) {                      // a copy fails half-way: the first failure stays, the rest is skipped
        Result<katome_contigs> c;
        CHECK(fill(c, 100, fail_at) == KATOME_E_DEVICE);
        CHECK(owner_of(c.get())->mem.size() == (size_t)fail_at + 1);     // (the failing array was taken, nothing after it)
        CHECK(strstr(get_error(), "stubbed copy failure") != nullptr);
    }
    {   // two texts back to back in one array; and the same with the second copy failing
        const char first[] = "H\tVN:Z:1.0\nS\t0\tACGT\n", second[] = "P\tkatome_0\t0+\t*\n";
        const uint64_t n1 = sizeof first - 1, n2 = sizeof second - 1;
        Result<katome_gfa_paths> g = make_result<katome_gfa_paths>();
        CHECK(g);
        Copier<katome_gfa_paths> down{g.get()};
        down.back_to_back(&g->text, first, n1, second, n2);
        CHECK(down.rc == KATOME_OK && memcmp(g->text, first, n1) == 0 && memcmp(g->text + n1, second, n2) == 0);
        down.back_to_back(&g->text, first, 0, second, 0);               // (both empty: room for one byte)
        CHECK(down.rc == KATOME_OK && g->text != nullptr);
        copies_left = 1;
        down.back_to_back(&g->text, first, n1, second, n2);
        copies_left = -1;
        CHECK(down.rc == KATOME_E_DEVICE);
        down(&g->segment_off, first, 1);                                // (skipped: the copier has failed)
        CHECK(g->segment_off == nullptr && owner_of(g.get())->mem.size() == 3);
    }
    {   // an array past the huge-page threshold: reserved aligned, touched by several threads, freed with free()
        Result<katome_gfa> g = make_result<katome_gfa>();
        CHECK(g);
        const size_t big = ((size_t)64 << 20) + 4096 + 3;
        std::vector<uint8_t> from(big, 7);
        Copier<katome_gfa> down{g.get()};
        down(&g->text, from.data(), big);
        CHECK(down.rc == KATOME_OK && ((uintptr_t)g->text & (((size_t)2 << 20) - 1)) == 0 && g->text[0] == 7 && g->text[big - 1] == 7);
    }
    katome_graph_free(nullptr);
    katome_unique_assembly_free(nullptr);
    CHECK(!Result<katome_assembly>());
    printf("ok %d\n", checks);
    return 0;
}
