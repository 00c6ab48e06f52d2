"""tests/count_model.py, the dictionary that tests/test_gpu_count_records.py holds the LDS counting kernels against, pinned itself:
against the oracle's build on literal reads that hold self-complementary k-mers (ACGT, AATT, GAATTC) once, twice and three times,
with Clean::remove_weak_edges at 2, 3 and 4; and, for the one rule the oracle cannot show, on three literal sums that pass 32 bits
(table.hip:8: "Weights are u32 and wrap like EdgeWeight")."""
import numpy as np
import pytest

import count_model as cm
from helpers import int_to_kmer, kmer_to_int, revcomp_str, windows_multiset

MOTIFS = ("ACGT", "AATT", "GAATTC")
L = 20


def _reads(times):
    """every motif `times` times at the head of a read of L bases, the rest a filler without palindromes of its own; and two reads
    that hold plain k-mers in both orientations"""
    rows = [(m * times + "CCACCTCCACCTCCACCTCC")[:L] for m in MOTIFS]
    rows += ["GATTACAGATTACAGATTAC", revcomp_str("GATTACAGATTACAGATTAC"), "TTGCATGCAAGGCTTAAGCC"]
    return np.frombuffer("".join(rows).encode(), np.uint8).reshape(len(rows), L)


def _records(reads, k):
    """the canonical window of every window, weighted with that window's occurrences: several records to a k-mer met in both orientations"""
    recs, wts = [], []
    for s, c in sorted(windows_multiset(reads, k, False).items()):
        recs.append(cm.canonical(kmer_to_int(s), k))
        wts.append(c)
    return recs, wts


def test_revcomp_is_the_strings():
    rng = np.random.default_rng(5)
    for k in (1, 3, 4, 5, 16, 31, 32, 33, 40, 63, 64, 95):
        for _ in range(20):
            s = "".join("ACGT"[c] for c in rng.integers(0, 4, k))
            assert int_to_kmer(cm.revcomp(kmer_to_int(s), k), k) == revcomp_str(s)
    assert cm.revcomp(kmer_to_int("ACGT"), 4) == kmer_to_int("ACGT") and cm.revcomp(kmer_to_int("GAATTC"), 6) == kmer_to_int("GAATTC")
    assert cm.revcomp(0, 5) == 4 ** 5 - 1


@pytest.mark.parametrize("k", [4, 6])
@pytest.mark.parametrize("times", [1, 2, 3])
def test_both_strands_and_the_threshold_are_the_oracles(oracle, k, times):
    reads = _reads(times)
    recs, wts = _records(reads, k)
    assert len(recs) > len(set(recs))                            # (some k-mer came in both orientations: its records are summed)
    palindromes = {m for m in MOTIFS if len(m) == k}
    for threshold in (None, 2, 3, 4):
        ref = oracle.build_ascii(reads, k, True, remove_weak_edges=threshold, stages=None if threshold is None else "w")
        got = [(int_to_kmer(key, k), w) for key, w in cm.count(recs, wts, k, True, threshold or 0)]
        assert got == ref.multiset(), (k, times, threshold)
        if threshold is None:
            have = dict(got)
            for m in palindromes:                                # once in the list, with twice its occurrences (at least)
                assert have[m] >= 2 * times and have[m] % 2 == 0 and [s for s, _ in got].count(m) == 1
    # one strand: the windows as they stand
    ref = oracle.build_ascii(reads, k, False)
    plain = sorted(windows_multiset(reads, k, False).items())
    got = cm.count([kmer_to_int(s) for s, _ in plain], [c for _, c in plain], k, False, 0)
    assert [(int_to_kmer(key, k), w) for key, w in got] == ref.multiset()


def test_the_threshold_meets_the_doubled_weight(oracle):
    """ACGT once in a read is an edge of weight 2: it stays at 2, goes at 3"""
    reads = np.frombuffer(b"ACGTC", np.uint8).reshape(1, 5)
    recs, wts = _records(reads, 4)
    for threshold, stays in ((2, True), (3, False)):
        ref = oracle.build_ascii(reads, 4, True, remove_weak_edges=threshold, stages="w").multiset()
        got = [(int_to_kmer(key, 4), w) for key, w in cm.count(recs, wts, 4, True, threshold)]
        assert got == ref and (("ACGT", 2) in got) == stays


def test_sums_wrap_in_32_bits():
    a, b, c, p = kmer_to_int("AAAC"), kmer_to_int("CCGA"), kmer_to_int("GTTG"), kmer_to_int("ACGT")
    recs = [a, b, a, c, b, c, c]
    wts = [0xFFFFFFFF, 0x80000000, 1, 0xFFFFFFFF, 0x80000005, 0xFFFFFFFF, 9]
    # 2^32 -> 0, 2^32 + 5 -> 5, 2^33 + 7 -> 7
    assert cm.count(recs, wts, 4, False, 0) == sorted([(a, 0), (b, 5), (c, 7)])
    assert cm.count(recs, wts, 4, False, 1) == sorted([(b, 5), (c, 7)])          # a weight of 0 stays only at threshold 0
    assert cm.count(recs, wts, 4, False, 6) == [(c, 7)]
    # the doubling wraps too: 2 * 2^31 = 0, 2 * (2^31 + 3) = 6
    assert cm.count([p], [0x80000000], 4, True, 0) == [(p, 0)] and cm.count([p], [0x80000000], 4, True, 1) == []
    assert cm.count([p, p], [0x80000000, 3], 4, True, 6) == [(p, 6)] and cm.count([p, p], [0x80000000, 3], 4, True, 7) == []
    assert cm.count([a, a, b], None, 4, False, 2) == [(a, 2)] and cm.n_distinct([a, a, b]) == 2


def test_both_orientations_among_the_records_are_refused():
    x = kmer_to_int("AAAC")
    with pytest.raises(ValueError):
        cm.count([x, cm.revcomp(x, 4)], [1, 1], 4, True, 0)


def test_owners_are_the_librarys():
    keys = [0, 4 ** 31 - 1, 12345678901234567]
    for n_parts in (1, 3, 16):
        own = cm.owners(keys, 31, n_parts)
        assert all(0 <= p < n_parts for p in own)
        # the outer bases are not part of the core
        assert cm.owners([key ^ 1 for key in keys], 31, n_parts) == own and cm.owners([key ^ (3 << 60) for key in keys], 31, n_parts) == own
