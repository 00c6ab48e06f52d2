// contig_stats.h -- Stats<ContigsStats> for Contigs (reference src/katome/stats/contigs.rs:31-89) as a pure function of the contigs'
// lengths and original_genome_length, written the way the reference computes it: lengths sorted ascending, n_metrics accumulating
// from the SMALLEST contig up and returning the last length it added, l50 counted from the largest.  Host-only, no HIP.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace katome {

struct ContigStats { uint64_t n50 = 0, l50 = 0, n90 = 0, ng50 = 0; };

// n_metrics (contigs.rs:75-89); false = the reference's `.last().unwrap()` on an empty scan (a tipping point of 0)
inline bool n_metrics(const std::vector<uint64_t>& sorted, uint64_t tipping_point, uint64_t* out) {
    uint64_t acc = 0, last = 0;
    bool any = false;
    for (const uint64_t x : sorted) {
        if (acc >= tipping_point) break;
        last = x; acc += x; any = true;
    }
    *out = last;
    return any;
}

// 0: fine; 1, 2, 3: the tipping point of n50 (sum / 2), n90 ((0.1 * sum) truncated) or ng50 (original_genome_length / 2) is 0 with
// contigs present, where the reference panics
inline int contig_stats(const uint64_t* lengths, uint64_t n, uint64_t original_genome_length, ContigStats* out) {
    *out = ContigStats();
    if (n == 0) return 0;
    std::vector<uint64_t> contigs(lengths, lengths + n);
    std::sort(contigs.begin(), contigs.end());
    uint64_t sum = 0;
    for (const uint64_t x : contigs) sum += x;
    if (!n_metrics(contigs, sum / 2, &out->n50)) return 1;
    if (!n_metrics(contigs, (uint64_t)(0.1 * (double)sum), &out->n90)) return 2;
    if (!n_metrics(contigs, original_genome_length / 2, &out->ng50)) return 3;
    uint64_t acc = 0, i_last = 0;                       // (sum / 2 > 0 here, so the scan below yields at least once)
    for (uint64_t i = 0; i < n; ++i) {
        if (acc >= sum / 2) break;
        i_last = i; acc += contigs[n - 1 - i];
    }
    out->l50 = i_last + 1;
    return 0;
}

}  // namespace katome
