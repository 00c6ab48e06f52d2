// C entry to katome_amd/csrc/contig_select.h (and contig_stats.h, what it must equal) for tests/test_contig_select_host.py (no GPU)
#include "../../katome_amd/csrc/contig_select.h"

using namespace katome;

extern "C" {

void* hs_select_new(uint32_t k, uint64_t genome_len) { return new ContigSelect(k, genome_len); }
void hs_select_free(void* h) { delete (ContigSelect*)h; }
// the pass to come and the four prefixes a contig's decided high bits are matched against in it
int hs_select_pass(const void* h, uint32_t* prefix4) {
    const ContigSelect* s = (const ContigSelect*)h;
    for (int i = 0; i < SELECTS; ++i) prefix4[i] = s->prefix[i];
    return s->pass;
}
// bins: [4][256]{count, sum of k-mers} over all shards -> 1 while another pass is needed
int hs_select_step(void* h, const uint64_t* bins) { return ((ContigSelect*)h)->step(bins) ? 1 : 0; }
int hs_select_result(const void* h, uint64_t* out4) {
    ContigStats st;
    const int rc = ((const ContigSelect*)h)->result(&st);
    out4[0] = st.n50; out4[1] = st.l50; out4[2] = st.n90; out4[3] = st.ng50;
    return rc;
}
int hs_select_reference(const uint64_t* lengths, uint64_t n, uint64_t genome_len, uint64_t* out4) {
    ContigStats st;
    const int rc = contig_stats(lengths, n, genome_len, &st);
    out4[0] = st.n50; out4[1] = st.l50; out4[2] = st.n90; out4[3] = st.ng50;
    return rc;
}

}
