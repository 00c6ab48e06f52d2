// Host build of katome_amd/csrc/strand_bits.h for the CPU tests (tests/test_gfa_strands_host.py).  Built as a shared library for the
// tests, or with -DSTRAND_BITS_MAIN as a stand-alone program (its own main: a self-check that a sanitizer build can run).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../katome_amd/csrc/strand_bits.h"

using namespace katome;

namespace {
// a label's packed bases (without the pad byte) at byte `shift` of a 4-byte aligned buffer that ends on a multiple of 4
struct Packed {
    std::vector<uint32_t> words;
    uint8_t* at;
    Packed(const uint8_t* bytes, uint64_t n, uint32_t shift) : words((shift + n + 3) / 4 + 1, 0xA5A5A5A5u) {
        at = reinterpret_cast<uint8_t*>(words.data()) + shift;
        memcpy(at, bytes, n);
    }
};
}  // namespace

extern "C" {

void hs_strand_first_kmer(const uint8_t* packed, uint64_t n_bytes, uint32_t shift, uint32_t k, uint64_t* out) {
    Packed p(packed, n_bytes, shift);
    const Key<2> key = first_kmer(p.at, k);
    out[0] = key.w[0]; out[1] = key.w[1];
}
void hs_strand_last_kmer_revcomp(const uint8_t* packed, uint64_t n_bytes, uint32_t shift, uint32_t n, uint32_t k, uint64_t* out) {
    Packed p(packed, n_bytes, shift);
    const Key<2> key = last_kmer_revcomp(p.at, n, k);
    out[0] = key.w[0]; out[1] = key.w[1];
}
// the first base at which text_i and revcomp(text_j) differ, rounded down to its 16-base word; -1: none
int64_t hs_strand_first_difference(const uint8_t* packed_i, const uint8_t* packed_j, uint64_t n_bytes, uint32_t shift_i, uint32_t shift_j, uint32_t n) {
    Packed a(packed_i, n_bytes, shift_i), b(packed_j, n_bytes, shift_j);
    for (uint32_t at = 0; at < n; at += 16)
        if (twin_word_differs(a.at, b.at, n, at)) return at;
    return -1;
}
void hs_strand_canonical_link(uint32_t a, uint32_t b, uint32_t ta, uint32_t tb, uint64_t* out) { canonical_link(a, b, ta, tb, out[0], out[1]); }

}

#ifdef STRAND_BITS_MAIN
static std::vector<uint8_t> pack(const std::string& s) {
    std::vector<uint8_t> out((s.size() + 3) / 4, 0);
    for (size_t i = 0; i < s.size(); ++i) out[i / 4] |= (uint8_t)(strchr("ACGT", s[i]) - "ACGT") << (6 - 2 * (i % 4));
    return out;
}
static std::string revcomp(const std::string& s) {
    std::string r(s.rbegin(), s.rend());
    for (char& c : r) c = "TGCA"[strchr("ACGT", c) - "ACGT"];
    return r;
}
int main() {
    uint64_t seed = 12345;
    auto next = [&]() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(seed >> 33); };
    int checked = 0;
    for (uint32_t n = 3; n < 200; ++n) {
        std::string s(n, 'A');
        for (char& c : s) c = "ACGT"[next() & 3];
        const std::string r = revcomp(s);
        const std::vector<uint8_t> ps = pack(s), pr = pack(r);
        for (uint32_t si = 0; si < 4; ++si)
            for (uint32_t sj = 0; sj < 4; ++sj) {
                if (hs_strand_first_difference(ps.data(), pr.data(), ps.size(), si, sj, n) != -1) { printf("FAIL: a twin of %u bases differs\n", n); return 1; }
                const uint32_t at = next() % n;
                std::string bad = r;
                bad[n - 1 - at] = "ACGT"[((strchr("ACGT", bad[n - 1 - at]) - "ACGT") + 1 + next() % 3) & 3];
                const std::vector<uint8_t> pb = pack(bad);
                if (hs_strand_first_difference(ps.data(), pb.data(), ps.size(), si, sj, n) != (int64_t)(at / 16 * 16)) { printf("FAIL: base %u of %u\n", at, n); return 1; }
                ++checked;
            }
        for (uint32_t k = 3; k <= 63 && k <= n; ++k) {
            uint64_t f[2], l[2], want[2];
            hs_strand_first_kmer(pr.data(), pr.size(), n & 3, k, f);
            hs_strand_last_kmer_revcomp(ps.data(), ps.size(), (n + 1) & 3, n, k, l);
            want[0] = want[1] = 0;
            for (uint32_t i = 0; i < k; ++i) {
                const uint64_t c = (uint64_t)(strchr("ACGT", r[i]) - "ACGT");
                want[0] = (want[0] << 2) | (want[1] >> 62); want[1] = (want[1] << 2) | c;
            }
            if (f[0] != want[0] || f[1] != want[1] || l[0] != want[0] || l[1] != want[1]) { printf("FAIL: end k-mers, n = %u, k = %u\n", n, k); return 1; }
            ++checked;
        }
    }
    printf("strand_bits: %d checks passed\n", checked);
    return 0;
}
#endif
