// Host-only driver of the query scanner of katome_depth_paths (katome_amd/csrc/ingest.cpp: scan_query, ingest_query_files) for
// sanitizer runs (tests/test_depth_query_host.py): literal cases on buffers in memory, then the files named on the command line.
// usage: depth_query_selftest <file_type> [files...]  -> "ok <cases>" and, with files, "status n_records text_bytes: len len ..."
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../katome_amd/csrc/common.h"

using namespace katome;

// the caching device allocator is not part of this build: the scanner never touches the device
namespace katome {
int dev_malloc(void**, size_t, hipStream_t) { return KATOME_E_DEVICE; }
void dev_free(void*, hipStream_t) {}
}

static int cases = 0;
static void fail(const char* what, const std::string& text) {
    fprintf(stderr, "case failed: %s on <<%s>>: %s\n", what, text.c_str(), get_error());
    exit(1);
}
// the records the scanner keeps, as strings; status checked against `want_status`
static std::vector<std::string> scan(uint32_t ft, const std::string& text, int want_status) {
    HostQuery q;
    // (an exact-size heap copy: a read one byte past the text is the sanitizer's to find)
    uint8_t* buf = (uint8_t*)malloc(text.size() ? text.size() : 1);
    memcpy(buf, text.data(), text.size());
    const int st = scan_query(ft, buf, text.size(), q);
    free(buf);
    if (st != want_status) fail("status", text);
    std::vector<std::string> out;
    if (q.off.size() != q.len.size()) fail("arrays", text);
    for (size_t i = 0; i < q.len.size(); ++i) {
        if (q.off[i] + q.len[i] > q.text.size()) fail("record past the text", text);
        out.push_back(q.len[i] ? std::string((const char*)q.text.data() + q.off[i], q.len[i]) : std::string());
    }
    ++cases;
    return out;
}
static void expect(uint32_t ft, const std::string& text, const std::vector<std::string>& want) {
    if (scan(ft, text, KATOME_OK) != want) fail("records", text);
}

int main(int argc, char** argv) {
    // FASTA: lines joined, records with N, shorter than k, empty; nothing dropped
    expect(0, ">a\nACGT\nAC\n>n\nACNNGT\n>s\nAC\n>e\n>e2\n\n>last\nGG", {"ACGTAC", "ACNNGT", "AC", "", "", "GG"});
    expect(0, ">a desc\r\nACGT  \r\nTT\r\n", {"ACGTTT"});
    expect(0, ">lower\nacgt\n", {"acgt"});
    expect(0, "", {});
    expect(0, ">only header", {""});
    scan(0, "ACGT\n>a\nAC\n", KATOME_E_PARSE);
    // FASTQ: four lines a record, the second is the sequence
    expect(1, "@a\nACGT\n+\nIIII\n@n\nANNT\n+\n@@@@\n@s\nA\n+\nI\n", {"ACGT", "ANNT", "A"});
    expect(1, "@e\n\n+\n\n@b\nAC \n+\nII\n", {"", "AC"});          // an empty record: its quality line is there, empty
    expect(1, "@a\nACGT\n+\nIIII", {"ACGT"});                      // no newline at the end
    expect(1, "", {});
    scan(1, "@a\nACGT\n+\n", KATOME_E_PARSE);
    scan(1, "@a\nACGT\n", KATOME_E_PARSE);
    scan(1, "@a", KATOME_E_PARSE);
    scan(1, "a\nACGT\n+\nIIII\n", KATOME_E_PARSE);
    // BFCounter and anything else is no query type
    scan(2, "ACGT\t3\n", KATOME_E_ARG);
    scan(7, "", KATOME_E_ARG);
    printf("ok %d\n", cases);
    if (argc > 2) {
        HostQuery q;
        const int st = ingest_query_files((uint32_t)atoi(argv[1]), (const char* const*)(argv + 2), (size_t)(argc - 2), q);
        printf("%d %zu %zu:", st, q.len.size(), q.text.size());
        for (uint32_t l : q.len) printf(" %u", l);
        printf("\n");
        if (st) fprintf(stderr, "%s\n", get_error());
    }
    return 0;
}
