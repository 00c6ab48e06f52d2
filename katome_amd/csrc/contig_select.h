// contig_select.h -- Contigs::stats (contig_stats.h; reference src/katome/stats/contigs.rs:31-89) of contigs that no single place
// holds: the reference's scans over the sorted lengths, restated as SELECTIONS that need only sums over all contigs.  Host-only, no
// HIP: dist_text.hip feeds it the allreduced bins of its kernel, tests/hostshim plays the same passes over lists cut into shards.
//
// A contig is its k-mer count m (u32, katome_dist_contigs.d_edge_kmers); its length is m + k - 1, so the order of the lengths is the
// order of m.  With F(v) = sum of the lengths of the contigs with m <= v and G(v) = the same for m >= v:
//   n_metrics(T), T > 0   the scan from the smallest contig up stops once it holds T bases and returns the last length added: the
//                         smallest v with F(v) >= T, or the largest contig when all of them together stay below T (NG50 of a genome
//                         longer than the assembly)
//   L50, H = sum / 2      the scan from the largest down counts contigs until it holds H bases: with v the largest value with
//                         G(v) >= H, all contigs above v and then copies of v, #{m > v} + ceil((H - sum of lengths above v) / length(v))
// The four thresholds (n50, n90, ng50, l50) are found together, 32 bits in four 8-bit digits from the top.  Per pass the caller counts,
// for each selection s, the contigs whose decided high bits equal prefix(s) into 256 bins by their next digit -- (count, sum of m) each
// -- over ALL contigs (one allreduce of SELECT_WORDS words), and step() picks the four digits.  The first pass also yields the count
// and the sum of all lengths, which set the tipping points exactly as contig_stats() computes them.
#pragma once
#include <stdint.h>

#include "contig_stats.h"

namespace katome {

constexpr int SELECTS = 4, SELECT_BINS = 256, SELECT_PASSES = 4;
constexpr int SELECT_WORDS = SELECTS * SELECT_BINS * 2;      // [selection][bin]{count, sum of m}
enum { SEL_N50 = 0, SEL_N90 = 1, SEL_NG50 = 2, SEL_L50 = 3 };

struct ContigSelect {
    uint32_t k = 0;
    uint64_t genome_len = 0;
    int pass = 0;                   // passes done
    int error = 0;                  // contig_stats()'s 1, 2, 3: which tipping point is 0
    uint64_t n = 0, sum = 0;        // contigs; bases of all of them (after the first pass)
    uint64_t tip[3] = {0, 0, 0};    // tipping points of n50, n90, ng50; tip[0] is L50's H as well
    bool largest = false;           // ng50: the genome is longer than the assembly, the answer is the largest contig
    uint32_t prefix[SELECTS] = {0, 0, 0, 0};     // the digits decided so far, low bits
    uint64_t far_sum[SELECTS] = {0, 0, 0, 0};    // bases of the contigs known to lie before the answer in scan order ...
    uint64_t far_cnt[SELECTS] = {0, 0, 0, 0};    // ... and how many they are

    ContigSelect(uint32_t k_, uint64_t genome_len_) : k(k_), genome_len(genome_len_) {}

    // bits of m below the digit of pass p
    static uint32_t shift_of(int p) { return 24u - 8u * (uint32_t)p; }
    // does m take part in selection s of the pass to come, and with which digit
    bool matches(int s, uint32_t m) const { return pass == 0 || (m >> (shift_of(pass) + 8)) == prefix[s]; }
    uint32_t digit(uint32_t m) const { return (m >> shift_of(pass)) & 255u; }

    uint64_t bin_bases(const uint64_t* bins, int s, int b) const {
        const uint64_t* w = bins + ((size_t)s * SELECT_BINS + b) * 2;
        return w[1] + w[0] * (uint64_t)(k - 1);
    }
    static uint64_t bin_count(const uint64_t* bins, int s, int b) { return bins[((size_t)s * SELECT_BINS + b) * 2]; }

    // contig_stats() returns at the first tipping point of 0 with what it has computed until then: n50 before 2, n50 and n90 before 3
    bool wanted(int s) const { return error == 0 || (error == 2 && s == SEL_N50) || (error == 3 && (s == SEL_N50 || s == SEL_N90)); }

    // the bins of pass `pass`, summed over all contigs -> true while another pass is needed
    bool step(const uint64_t* bins) {
        if (error == 1 || error < 0 || pass >= SELECT_PASSES) return false;
        if (pass == 0) {
            for (int b = 0; b < SELECT_BINS; ++b) { n += bin_count(bins, 0, b); sum += bin_bases(bins, 0, b); }
            if (n == 0) { pass = SELECT_PASSES; return false; }
            tip[0] = sum / 2; tip[1] = (uint64_t)(0.1 * (double)sum); tip[2] = genome_len / 2;      // contig_stats.h, in its order
            for (int t = 0; t < 3 && !error; ++t) if (tip[t] == 0) error = t + 1;
            if (error == 1) return false;          // (contig_stats() has filled in nothing yet; after 2 or 3 it has: those go on)
            largest = sum < tip[2];
        }
        for (int s = 0; s < SELECTS; ++s) {
            if (!wanted(s)) continue;
            int pick = -1;
            if (s == SEL_L50) {                      // from the top: the largest digit at which the bases from there up reach H
                uint64_t acc = far_sum[s], cnt = far_cnt[s];
                for (int b = SELECT_BINS - 1; b >= 0; --b) {
                    const uint64_t bases = bin_bases(bins, s, b);
                    if (bin_count(bins, s, b) && acc + bases >= tip[0]) { pick = b; break; }
                    acc += bases; cnt += bin_count(bins, s, b);
                }
                if (pick >= 0) { far_sum[s] = acc; far_cnt[s] = cnt; }
            } else if (s == SEL_NG50 && largest) {   // the largest contig there is
                for (int b = SELECT_BINS - 1; b >= 0 && pick < 0; --b) if (bin_count(bins, s, b)) pick = b;
            } else {                                 // from the bottom: the smallest digit at which the bases up to there reach T
                uint64_t acc = far_sum[s], cnt = far_cnt[s];
                for (int b = 0; b < SELECT_BINS; ++b) {
                    const uint64_t bases = bin_bases(bins, s, b);
                    if (bin_count(bins, s, b) && acc + bases >= tip[s]) { pick = b; break; }
                    acc += bases; cnt += bin_count(bins, s, b);
                }
                if (pick >= 0) { far_sum[s] = acc; far_cnt[s] = cnt; }
            }
            if (pick < 0) { error = -1; return false; }      // the bins are not those of one list of contigs
            prefix[s] = (prefix[s] << 8) | (uint32_t)pick;
        }
        return ++pass < SELECT_PASSES;
    }

    // after the last pass: 0 and the stats, or contig_stats()'s 1, 2, 3 with the fields it had filled in by then (-1: inconsistent bins)
    int result(ContigStats* out) const {
        *out = ContigStats();
        if (n == 0 || error == 1 || error < 0) return error;
        const uint64_t add = (uint64_t)(k - 1);
        out->n50 = prefix[SEL_N50] + add;
        if (error == 2) return error;
        out->n90 = prefix[SEL_N90] + add;
        if (error == 3) return error;
        out->ng50 = prefix[SEL_NG50] + add;
        const uint64_t v = prefix[SEL_L50] + add, need = tip[0] - far_sum[SEL_L50];      // (G above v stays below H: need > 0)
        out->l50 = far_cnt[SEL_L50] + (need + v - 1) / v;
        return 0;
    }
};

}  // namespace katome
